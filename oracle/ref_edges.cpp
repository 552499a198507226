// ref_edges.cpp -- second fixture generator on the REAL reference classes (built by oracle/Makefile's `ref` target into
// oracle/_ref/ref_edges; never shipped, never copied from).  Where ref_dump.cpp runs the reference over FASTA files, this
// one INJECTS constructed tables into the reference's private members and re-runs single stages on them, so that the
// value edges of tests/table_edges_model.py and tests/em_edges_model.py get a reference-side answer
// (tests/golden/make_edge_golden.py writes the jobs and turns the answers into tests/golden/edges_*.npz).
//
// TEST INFRASTRUCTURE ONLY.
//
// usage: ref_edges <mode> <dir>      reads <dir>/job.txt and raw little-endian arrays, writes raw arrays back into <dir>.
// Floats in job.txt are written as the 8 hex digits of their bits (NaN, -0.0 and infinities travel unchanged).
//
//   bg     job: one line per case "<name> <K> <alpha0> <alpha1> <alpha2>"; <name>.n.i32 = the counters n[0] | n[1] | n[2] of
//          the orders used, written into BackgroundModel::n_; calculateV(); -> <name>.V.f32
//   sweep  job: "<W> <BOTH|PLUS> <k> <max_k> <ltot> <from_V>" and then one line per seed selection
//          "<z_threshold> <count_threshold> <filter_neighbors>".  from_V = 1: V.f32 (84 floats) goes into
//          BackgroundModel::v_ and the BasePattern constructor itself runs calculate_bg_probabilities and
//          aggregate_double_strand_background; from_V = 0: bgp.f32 is written over pattern_bg_probabilities[k].
//          counts.u32 -> pattern_counter, ltot -> ltot; calculate_expected_counts / calculate_log_pvalues /
//          calculate_zscores; -> bgp<o>.f32 (from_V = 1), expected.f32, logp.f32, z.f32, seeds<i>.u64 (or seeds_undefined)
//   iupac  job: the sweep line (from_V = 0), then "<n ids>"; ids.u64; per id aggregate_attributes_from_basepatterns and
//          count_combined_occurences (a child process per id) -> sites.u64, cc.u64, stats.f32 [n][4] = bg_p, expected, z,
//          log-p, died.u8 (1 = the reference's own assert on bg_p aborted this id)
//   em     job: "<W> <n PWMs> <saturation> <threshold> <cap> <cap> ..."; counts.u32, bg.f32, pwms.f32 [n][W][4];
//          one Peng::em_optimize_pwms call per (cap, PWM), its stdout swallowed -> out.f32 [caps][n][W][4], the PWM of the
//          returned IUPACPattern (the constructor's extra normalisation included)
//   sim    job: "<n> <max_len> <BOTH|PLUS>"; pwms.f32 [n][max_len][4], lens.i32, sites.u64, bg.f32 [4];
//          IUPACPattern::calculate_S for every pair, j = 0 .. n-1, i = 0 .. j-1 -> S.f32

#include <algorithm>
#include <array>
#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <map>
#include <memory>
#include <set>
#include <sstream>
#include <string>
#include <tuple>
#include <vector>

#include <signal.h>
#include <sys/wait.h>
#include <unistd.h>

// the reference keeps its tables private; this generator writes them.
#define private public
#include "base_pattern.h"
#include "iupac_alphabet.h"
#include "iupac_pattern.h"
#include "peng.h"
#undef private

static std::string DIR;

template <class T>
static std::vector<T> load(const std::string& name) {
  const std::string path = DIR + "/" + name;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) {
    perror(path.c_str());
    exit(2);
  }
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<T> v(n / sizeof(T));
  if (fread(v.data(), sizeof(T), v.size(), f) != v.size()) exit(2);
  fclose(f);
  return v;
}

template <class T>
static void dump(const std::string& name, const T* p, size_t n) {
  const std::string path = DIR + "/" + name;
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) {
    perror(path.c_str());
    exit(2);
  }
  fwrite(p, sizeof(T), n, f);
  fclose(f);
}

static float hexf(const std::string& s) {
  const uint32_t u = (uint32_t)strtoul(s.c_str(), nullptr, 16);
  float f;
  memcpy(&f, &u, 4);
  return f;
}

static void need(bool ok, const char* what) {
  if (!ok) {
    fprintf(stderr, "ref_edges: %s\n", what);
    exit(2);
  }
}

// a sequence set to construct the reference's objects over; every table it leaves behind is overwritten
static SequenceSet* tiny_sequences() {
  const std::string path = DIR + "/tiny.fa";
  FILE* f = fopen(path.c_str(), "w");
  fprintf(f, ">a\nACGTTGCAAGGCTCATTACGGATC\n>b\nTTGACCAGTAGGCATCGATTACCA\n");
  fclose(f);
  return new SequenceSet(path, true);
}

struct Sweep {
  int W, k, max_k, from_V;
  Strand strand;
  size_t ltot;
  BackgroundModel* bg;
  BasePattern* bp;
  size_t NP;
};

// the injected BasePattern of the modes sweep and iupac
static Sweep make_sweep(std::istream& job, SequenceSet* ss) {
  Sweep s;
  std::string strand;
  unsigned long long ltot;
  job >> s.W >> strand >> s.k >> s.max_k >> ltot >> s.from_V;
  need(!job.fail() && s.k <= s.max_k && s.max_k <= 2 && s.max_k < s.W, "bad sweep line");
  s.strand = strand == "PLUS" ? Strand::PLUS_STRAND : Strand::BOTH_STRANDS;
  s.ltot = (size_t)ltot;
  s.bg = new BackgroundModel(*ss, 2, std::vector<float>{1.f, 1.f, 1.f}, true);
  if (s.from_V) {
    const std::vector<float> V = load<float>("V.f32");
    need(V.size() == 84, "V.f32 holds 84 floats");
    for (int k = 0, at = 0; k <= 2; ++k)
      for (int y = 0; y < (1 << (2 * (k + 1))); ++y) s.bg->v_[k][y] = V[at++];
  }
  IUPACAlphabet::init(Alphabet::getAlphabet());
  IUPACPattern::init(17, s.bg->getV()[0]);
  s.bp = new BasePattern(s.W, s.strand, s.k, s.max_k, ss, s.bg);
  s.NP = s.bp->getNumberPatterns();
  if (!s.from_V) {
    const std::vector<float> t = load<float>("bgp.f32");
    need(t.size() == s.NP, "bgp table size");
    memcpy(s.bp->pattern_bg_probabilities[s.k], t.data(), 4 * s.NP);
  }
  const std::vector<uint32_t> c = load<uint32_t>("counts.u32");
  need(c.size() == s.NP, "counts table size");
  for (size_t i = 0; i < s.NP; ++i) s.bp->pattern_counter[i] = c[i];
  s.bp->ltot = s.ltot;
  s.bp->calculate_expected_counts();
  s.bp->calculate_log_pvalues();
  s.bp->calculate_zscores();
  return s;
}

static int mode_bg(std::istream& job, SequenceSet* ss) {
  std::string name, a[3];
  int K;
  while (job >> name >> K >> a[0] >> a[1] >> a[2]) {
    need(K >= 0 && K <= 2, "bad order");
    std::vector<float> alpha;
    for (int k = 0; k <= K; ++k) alpha.push_back(hexf(a[k]));
    BackgroundModel bg(*ss, K, alpha, true);
    const std::vector<int32_t> n = load<int32_t>(name + ".n.i32");
    size_t at = 0;
    for (int k = 0; k <= K; ++k)
      for (int y = 0; y < (1 << (2 * (k + 1))); ++y) bg.n_[k][y] = n.at(at++);
    need(at == n.size(), "counter file size");
    bg.calculateV();
    std::vector<float> V;
    for (int k = 0; k <= K; ++k)
      for (int y = 0; y < (1 << (2 * (k + 1))); ++y) V.push_back(bg.getV()[k][y]);
    dump(name + ".V.f32", V.data(), V.size());
  }
  return 0;
}

static int mode_sweep(std::istream& job, SequenceSet* ss) {
  Sweep s = make_sweep(job, ss);
  if (s.from_V)
    for (int o = 0; o <= s.max_k; ++o) dump("bgp" + std::to_string(o) + ".f32", s.bp->pattern_bg_probabilities[o], s.NP);
  dump("expected.f32", s.bp->expected_counts, s.NP);
  dump("logp.f32", s.bp->pattern_logp, s.NP);
  dump("z.f32", s.bp->pattern_zscore, s.NP);
  std::string zt;
  unsigned long long ct;
  int filter;
  // select_base_patterns sorts the ids with `z[i] > z[j]` (src/base_pattern.cpp:458, 171): with a NaN among the z-scores
  // that is no strict weak ordering and std::sort is undefined -- no selection is run then, and seeds_undefined says so
  bool nan_z = false;
  for (size_t i = 0; i < s.NP; ++i) nan_z |= std::isnan(s.bp->pattern_zscore[i]);
  if (nan_z) {
    const uint8_t one = 1;
    dump("seeds_undefined", &one, 1);
    return 0;
  }
  for (int i = 0; job >> zt >> ct >> filter; ++i) {
    std::vector<size_t> seeds = s.bp->select_base_patterns(hexf(zt), (size_t)ct, s.strand == Strand::PLUS_STRAND, filter != 0);
    std::vector<uint64_t> out(seeds.begin(), seeds.end());
    dump("seeds" + std::to_string(i) + ".u64", out.data(), out.size());
  }
  return 0;
}

static int mode_iupac(std::istream& job, SequenceSet* ss) {
  Sweep s = make_sweep(job, ss);
  size_t n;
  job >> n;
  const std::vector<uint64_t> ids = load<uint64_t>("ids.u64");
  need(!job.fail() && ids.size() == n, "ids.u64 size");
  // one child process per id: the reference asserts 0 <= bg_p <= 1 (src/iupac_pattern.cpp:443) and aborts where the float32
  // sum of a large pattern's members passes 1 -- such an id is reported in died.u8 and its row left 0
  std::vector<uint64_t> sites(n), cc(n);
  std::vector<float> st(4 * n);
  std::vector<uint8_t> died(n);
  fflush(nullptr);
  for (size_t i = 0; i < n; ++i) {
    int fd[2];
    need(pipe(fd) == 0, "pipe");
    const pid_t child = fork();
    need(child >= 0, "fork");
    if (child == 0) {
      fclose(stderr);
      IUPACPattern p((size_t)ids[i], s.W);
      p.aggregate_attributes_from_basepatterns(s.bp);
      struct { uint64_t sites, cc; float st[4]; } r = {p.get_sites(), p.count_combined_occurences(s.bp, (size_t)ids[i]),
                                                       {p.get_bg_p(), p.getExpectedCounts(), p.getZscore(), p.getLogPval()}};
      const bool ok = write(fd[1], &r, sizeof r) == (ssize_t)sizeof r;
      _exit(ok ? 0 : 3);
    }
    close(fd[1]);
    struct { uint64_t sites, cc; float st[4]; } r;
    const bool got = read(fd[0], &r, sizeof r) == (ssize_t)sizeof r;
    close(fd[0]);
    int status = 0;
    waitpid(child, &status, 0);
    if (got && WIFEXITED(status) && WEXITSTATUS(status) == 0) {
      sites[i] = r.sites;
      cc[i] = r.cc;
      memcpy(&st[4 * i], r.st, sizeof r.st);
    } else {
      need(WIFSIGNALED(status) && WTERMSIG(status) == SIGABRT, "an id's child ended in something else than the reference's assert");
      died[i] = 1;
    }
  }
  dump("died.u8", died.data(), n);
  dump("sites.u64", sites.data(), n);
  dump("cc.u64", cc.data(), n);
  dump("stats.f32", st.data(), st.size());
  return 0;
}

static float** new_pwm(int len, const float* src) {
  float** m = new float*[len];
  for (int p = 0; p < len; ++p) {
    m[p] = new float[4];
    for (int a = 0; a < 4; ++a) m[p][a] = src[4 * p + a];
  }
  return m;
}

static int mode_em(std::istream& job, SequenceSet* ss) {
  int W, n;
  std::string sat, thr;
  job >> W >> n >> sat >> thr;
  need(!job.fail(), "bad em line");
  std::vector<int> caps;
  for (int c; job >> c;) caps.push_back(c);
  const float saturation = hexf(sat), threshold = hexf(thr);
  BackgroundModel* bg = new BackgroundModel(*ss, 2, std::vector<float>{1.f, 1.f, 1.f}, true);
  Peng peng(Strand::PLUS_STRAND, 0, 0, ss, bg);  // (initialises the IUPAC alphabet and factors)
  BasePattern* bp = new BasePattern(W, Strand::PLUS_STRAND, 0, 0, ss, bg);
  const size_t NP = bp->getNumberPatterns();
  const std::vector<uint32_t> counts = load<uint32_t>("counts.u32");
  std::vector<float> bgp = load<float>("bg.f32");
  const std::vector<float> pwms = load<float>("pwms.f32");
  need(counts.size() == NP && bgp.size() == NP && pwms.size() == (size_t)n * W * 4, "em table sizes");
  for (size_t i = 0; i < NP; ++i) bp->pattern_counter[i] = counts[i];
  std::vector<float> out;
  std::ostringstream sink;
  std::streambuf* keep = std::cout.rdbuf(sink.rdbuf());
  for (int cap : caps)
    for (int i = 0; i < n; ++i) {
      IUPACPattern start(0, W);
      for (int p = 0; p < W; ++p) start.local_n_sites[p] = 0;
      start.pwm = new_pwm(W, pwms.data() + (size_t)i * W * 4);
      std::vector<IUPACPattern*> in{&start}, res;
      peng.em_optimize_pwms(in, bp, saturation, threshold, cap, bgp.data(), res);
      need(res.size() == 1, "em_optimize_pwms returned no pattern");
      for (int p = 0; p < W; ++p)
        for (int a = 0; a < 4; ++a) out.push_back(res[0]->get_pwm()[p][a]);
      delete res[0];
      sink.str("");
    }
  std::cout.rdbuf(keep);
  dump("out.f32", out.data(), out.size());
  return 0;
}

static int mode_sim(std::istream& job, SequenceSet* ss) {
  int n, max_len;
  std::string strand;
  job >> n >> max_len >> strand;
  need(!job.fail(), "bad sim line");
  const Strand s = strand == "PLUS" ? Strand::PLUS_STRAND : Strand::BOTH_STRANDS;
  const std::vector<float> pwms = load<float>("pwms.f32");
  const std::vector<int32_t> lens = load<int32_t>("lens.i32");
  const std::vector<uint64_t> sites = load<uint64_t>("sites.u64");
  std::vector<float> bg = load<float>("bg.f32");
  need(pwms.size() == (size_t)n * max_len * 4 && lens.size() == (size_t)n && sites.size() == (size_t)n && bg.size() == 4, "sim sizes");
  std::vector<IUPACPattern*> pat;
  for (int i = 0; i < n; ++i) {
    IUPACPattern* p = new IUPACPattern(0, lens[i]);
    p->pwm = new_pwm(lens[i], pwms.data() + (size_t)i * max_len * 4);
    p->calculate_comp_pwm();
    p->n_sites = (size_t)sites[i];
    pat.push_back(p);
  }
  std::vector<float> S;
  for (int j = 0; j < n; ++j)
    for (int i = 0; i < j; ++i) S.push_back(std::get<0>(IUPACPattern::calculate_S(pat[i], pat[j], s, bg.data())));
  dump("S.f32", S.data(), S.size());
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s bg|sweep|iupac|em|sim dir\n", argv[0]);
    return 2;
  }
  const std::string mode = argv[1];
  DIR = argv[2];
  std::ifstream job(DIR + "/job.txt");
  need(job.good(), "no job.txt");
  Alphabet::init("STANDARD");
  SequenceSet* ss = tiny_sequences();
  if (mode == "bg") return mode_bg(job, ss);
  if (mode == "sweep") return mode_sweep(job, ss);
  if (mode == "iupac") return mode_iupac(job, ss);
  if (mode == "em") return mode_em(job, ss);
  if (mode == "sim") return mode_sim(job, ss);
  fprintf(stderr, "unknown mode %s\n", mode.c_str());
  return 2;
}
