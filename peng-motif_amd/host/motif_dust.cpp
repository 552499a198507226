#include "motif_dust.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "device.h"

std::string masked_runs_tsv(const uint32_t* a, const uint32_t* b, const int64_t* offs, const uint32_t* lens, size_t n_seq,
                            unsigned long long index0) {
  std::string out;
  char line[96];
  for (size_t i = 0; i < n_seq; ++i) {
    const uint64_t w0 = (uint64_t)offs[i] >> 5;
    const uint32_t L = lens[i], nw = (L + 31u) >> 5;
    bool in = false;
    uint32_t start = 0;
    for (uint32_t j = 0; j < nw; ++j) {
      uint32_t x = a[w0 + j] ^ b[w0 + j];
      if (!in && !x) continue;
      if (in && x == 0xFFFFFFFFu) continue;
      for (uint32_t k = 0; k < 32u; ++k) {
        const bool bit = (x >> k) & 1u;
        if (bit == in) continue;
        if (bit) {
          start = 32u * j + k;
        } else {
          snprintf(line, sizeof line, "%llu\t%u\t%u\n", index0 + i, start, 32u * j + k);
          out += line;
        }
        in = bit;
      }
    }
    if (in) {  // (a run to the last bit of the last word: the sequence's end)
      snprintf(line, sizeof line, "%llu\t%u\t%u\n", index0 + i, start, std::min(L, 32u * nw));
      out += line;
    }
  }
  return out;
}

namespace {
using pengk_host::check;
using pengk_host::DeviceBuffer;

void dump_file(const std::string& path, const void* p, size_t bytes) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(p, 1, bytes, f) != bytes) {
    std::cerr << "Error: PENGK_DUMP_TABLES: cannot write " << path << std::endl;
    exit(1);
  }
  fclose(f);
}

// mask and pack one set; h_valid / h_out: the validity words before and behind the mask (this rank's), downloaded only
// when a report or a dump wants them
void mask_set(const ScanInput& in, int W, int threshold, MaskedSet* ms, std::vector<uint32_t>* h_valid, std::vector<uint32_t>* h_out,
              bool want_out) {
  pengk_ctx* ctx = pengk_host::context();
  const size_t n_local = in.n_local;
  ms->d_valid.resize((size_t)in.n_words);
  DeviceBuffer<uint64_t> d_cnt(2);
  check(pengk_memset(ctx, d_cnt.get(), 0, 2 * sizeof(uint64_t)), "pengk_memset");
  check(pengk_mask_low_complexity(ctx, in.d_words.get(), in.d_valid.get(), in.d_offs.get(), in.d_lens.get(), n_local, threshold,
                                  ms->d_valid.get(), d_cnt.get()),
        "pengk_mask_low_complexity");
  uint64_t cnt[2] = {0, 0};
  d_cnt.download(cnt, 2);
  h_valid->assign(want_out ? (size_t)in.n_words : 0, 0u);
  h_out->assign(want_out ? (size_t)in.n_words : 0, 0u);
  if (n_local && want_out) {
    in.d_valid.download(h_valid->data(), (size_t)in.n_words);
    ms->d_valid.download(h_out->data(), (size_t)in.n_words);
  }
  // (the valid bases were counted on the host while the scan layout was built: nothing is copied back for them)
  long long tot[4] = {(long long)cnt[0], (long long)in.valid_bases, (long long)cnt[1], (long long)n_local};
  SequenceSet::allreduceSum(tot, 4);
  ms->bases_masked = (unsigned long long)tot[0];
  ms->bases_valid = (unsigned long long)tot[1];
  ms->seqs_touched = (unsigned long long)tot[2];
  ms->seqs = (unsigned long long)tot[3];
  if (ms->bases_masked == 0) return;
  // the masked set in the count layout
  DeviceBuffer<uint64_t> d_seq_base(n_local), d_seq_item(n_local);
  pengk_packed pk;
  check(pengk_pack_scan_sizes(ctx, ms->d_valid.get(), in.d_offs.get(), in.d_lens.get(), n_local, W, 0, d_seq_base.get(),
                              d_seq_item.get(), &pk),
        "pengk_pack_scan_sizes");
  ms->d_words.resize(pk.n_words);
  ms->d_items.resize(pk.n_items + 1);
  check(pengk_pack_scan(ctx, in.d_words.get(), ms->d_valid.get(), in.d_offs.get(), in.d_lens.get(), n_local, W, 0, d_seq_base.get(),
                        d_seq_item.get(), ms->d_words.get(), pk.n_words, ms->d_items.get(), pk.n_items),
        "pengk_pack_scan");
  check(pengk_synchronize(ctx), "pengk_synchronize");  // (the offset arrays leave scope here)
  ms->packed.W = W;
  ms->packed.item_windows = pk.item_windows;
  ms->packed.d_words = ms->d_words.get();
  ms->packed.d_items = ms->d_items.get();
  ms->packed.n_words = pk.n_words;
  ms->packed.n_items = pk.n_items;
  ms->packed.n_windows = pk.n_windows;
  ms->packed.max_bin_bound = pk.max_bin_bound;
  ms->packed.all_whole = pk.all_whole;
}

void say(const char* what, int threshold, const MaskedSet& ms) {
  std::cout << "low-complexity mask (threshold " << threshold << ") of the " << what << ": " << ms.bases_masked << " of "
            << ms.bases_valid << " bases masked in " << ms.seqs_touched << " of " << ms.seqs << " sequences";
  if (ms.bases_masked == 0) std::cout << "; nothing to mask, the " << what << " is counted as it is";
  std::cout << std::endl;
}

// rank 0 writes its own lines and then every other rank's, in rank order
void write_report(const std::string& own, const char* path) {
  const int R = pengk_host::world(), me = pengk_host::rank();
  std::vector<std::string> streams(R);
  if (R > 1) {
    uint64_t mine = own.size();
    std::vector<uint64_t> total(R, 0);
    check(pengk_comm_host_allgather(&mine, total.data(), sizeof(uint64_t)), "pengk_comm_host_allgather");
    const uint64_t longest = *std::max_element(total.begin(), total.end());
    const uint64_t C = std::min<uint64_t>(longest, 64ull << 20);
    if (C) {
      std::vector<char> send(C), recv((size_t)R * C);
      for (uint64_t off = 0; off < longest; off += C) {
        const uint64_t n = own.size() > off ? std::min<uint64_t>(C, own.size() - off) : 0;
        if (n) memcpy(send.data(), own.data() + off, n);
        check(pengk_comm_host_allgather(send.data(), recv.data(), C), "pengk_comm_host_allgather");
        if (me == 0)
          for (int r = 1; r < R; ++r)
            if (total[r] > off) streams[r].append(recv.data() + (size_t)r * C, std::min<uint64_t>(C, total[r] - off));
      }
    }
  }
  if (me != 0) return;
  FILE* f = fopen(path, "wb");
  bool ok = f != nullptr;
  ok = ok && fwrite(own.data(), 1, own.size(), f) == own.size();
  for (int r = 1; r < R && ok; ++r) ok = fwrite(streams[r].data(), 1, streams[r].size(), f) == streams[r].size();
  if (f) ok = (fclose(f) == 0) && ok;
  if (!ok) {
    std::cerr << "Error: cannot write " << path << std::endl;
    exit(1);
  }
}
}  // namespace

void mask_low_complexity(SequenceSet& input, const ScanInput& scan, SequenceSet* control, int W, int threshold,
                         const char* report_path, LowComplexityMask* out) {
  pengk_host::Lap lap("  mask: ");
  const char* dump_dir = pengk_host::rank() == 0 ? std::getenv("PENGK_DUMP_TABLES") : nullptr;
  std::vector<uint32_t> h_valid, h_out;
  mask_set(scan, W, threshold, &out->input, &h_valid, &h_out, dump_dir || report_path);
  lap("input: mask + pack");
  say("input", threshold, out->input);
  if (dump_dir) {  // test hook: rank 0's validity words behind the mask and the global figures
    dump_file(std::string(dump_dir) + "/mask_valid.u32", h_out.data(), h_out.size() * sizeof(uint32_t));
    const uint64_t c[4] = {out->input.bases_masked, out->input.bases_valid, out->input.seqs_touched, out->input.seqs};
    dump_file(std::string(dump_dir) + "/mask_counts.u64", c, sizeof c);
  }
  if (report_path) {
    std::vector<int64_t> offs(std::max<size_t>(scan.n_local, 1));
    std::vector<uint32_t> lens(std::max<size_t>(scan.n_local, 1));
    if (scan.n_local) {
      scan.d_offs.download(offs.data(), scan.n_local);
      scan.d_lens.download(lens.data(), scan.n_local);
    }
    write_report(masked_runs_tsv(h_valid.data(), h_out.data(), offs.data(), lens.data(), scan.n_local, input.getLocalBase()),
                 report_path);
    lap("report");
  }
  if (out->input.bases_masked) {
    pengk_host::override_packed_input(&input, &out->input.packed);
    out->attached = true;
  }
  if (control) {
    out->control_scan.reset(new ScanInput);
    build_scan_input(*control, out->control_scan.get());
    mask_set(*out->control_scan, W, threshold, &out->control, &h_valid, &h_out, dump_dir != nullptr);  // (no report of the control)
    lap("control: scan layout + mask + pack");
    say("control set", threshold, out->control);
    if (dump_dir) dump_file(std::string(dump_dir) + "/mask_control_valid.u32", h_out.data(), h_out.size() * sizeof(uint32_t));
    if (out->control.bases_masked) {
      pengk_host::override_control_input(control, &out->control.packed);
      out->control_attached = true;
    }
    out->control_scan.reset();  // (the count layout stays; the scan layout of the control has done its duty)
  }
}
