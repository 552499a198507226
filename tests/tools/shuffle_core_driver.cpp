// shuffle_core_driver -- the per-sequence body of shuffle_sequences_kernel (csrc/shuffle_core.h) on the CPU.
// stdin: one line per sequence, "seed g all_valid letters" (letters: digits 0..4, 4 = not A/C/G/T; "-" = empty;
// all_valid = 1 passes no validity words, as d_valid = NULL does).  stdout: the shuffled letters, one line each, then
// the output words and validity words in hex, so that the padding bits are compared too.
// Built and run by tests/test_motif_shuffle_cpu.py; a sanitizer build needs nothing else:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I peng-motif_amd/csrc tests/tools/shuffle_core_driver.cpp
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "shuffle_core.h"

int main() {
  unsigned long long seed, g;
  int all_valid;
  std::string s;
  while (std::cin >> seed >> g >> all_valid >> s) {
    if (s == "-") s.clear();
    const uint32_t L = (uint32_t)s.size(), nw = (L + 31u) >> 5;
    std::vector<uint64_t> w(nw, 0), ow(nw, ~0ull);
    std::vector<uint32_t> v(nw, 0), ov(nw, ~0u);
    for (uint32_t p = 0; p < L; ++p) {
      const uint32_t a = (uint32_t)(s[p] - '0');
      if (a < 4) {
        w[p >> 5] |= (uint64_t)a << (2 * (p & 31));
        v[p >> 5] |= 1u << (p & 31);
      }
    }
    uint32_t cnt[25];
    if (L) pengk::shuffle_sequence<1>(seed, g, w.data(), all_valid ? nullptr : v.data(), L, cnt, ow.data(), ov.data());
    std::string o(L, '0');
    for (uint32_t p = 0; p < L; ++p)
      o[p] = (ov[p >> 5] >> (p & 31)) & 1u ? (char)('0' + ((ow[p >> 5] >> (2 * (p & 31))) & 3u)) : '4';
    printf("%s", L ? o.c_str() : "-");
    for (uint32_t j = 0; j < nw; ++j) printf(" %016llx:%08x", (unsigned long long)ow[j], ov[j]);
    printf("\n");
  }
  return 0;
}
