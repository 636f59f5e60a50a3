// identity_check.cpp — the host statement of the sketch mode's definition (pyani_amd/csrc/pg_sketch_core.h), printed for
// tests/test_sketch_k_cpu.py to compare with the numpy statement (tests/sketch_k_cases.py) bit for bit.  A stand-alone program:
//   identity_check <record.txt>      (one record of ASCII bases; anything but ACGTacgt is an ambiguity symbol)
// Build: g++ -O2 -std=c++17 -ffp-contract=off -Ipyani_amd/csrc (the library's own floating-point rule), a second time with
// -fsanitize=address,undefined.  For every k of {8, 11, 15, 16} it prints
//   I <k> <h> <n> <bits of frag_identity(h, n, k)>          over every 2 <= h <= n <= 400 and h in {2, n/2, n} at n in {1000, 2985, 4096}
//   W <k> <p> <forward> <reverse complement> <canonical> <sampled at scale 16>      for every window of k unambiguous bases starting at p
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pg_sketch_core.h"

static void print_identity(int k, uint32_t h, uint32_t n) {
  const double y = pgs::frag_identity(h, n, k);
  uint64_t bits;
  std::memcpy(&bits, &y, sizeof bits);
  std::printf("I %d %u %u %016llx\n", k, h, n, (unsigned long long)bits);
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: identity_check <record.txt>\n"); return 2; }
  std::FILE* fh = std::fopen(argv[1], "rb");
  if (!fh) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::string rec;
  char buf[4096];
  for (size_t got; (got = std::fread(buf, 1, sizeof buf, fh)) > 0;) rec.append(buf, got);
  std::fclose(fh);
  while (!rec.empty() && (rec.back() == '\n' || rec.back() == '\r')) rec.pop_back();
  std::vector<int> code(rec.size());
  for (size_t i = 0; i < rec.size(); ++i) {
    switch (rec[i]) {
      case 'A': case 'a': code[i] = 0; break;
      case 'C': case 'c': code[i] = 1; break;
      case 'G': case 'g': code[i] = 2; break;
      case 'T': case 't': code[i] = 3; break;
      default: code[i] = -1;
    }
  }
  const int ks[4] = {8, 11, 15, 16};
  for (int k : ks) {
    for (uint32_t n = 2; n <= 400; ++n)
      for (uint32_t h = 2; h <= n; ++h) print_identity(k, h, n);
    const uint32_t big[3] = {1000, 2985, 4096};
    for (uint32_t n : big) { print_identity(k, 2, n); print_identity(k, n / 2, n); print_identity(k, n, n); }
    uint32_t f = 0, r = 0;
    size_t run = 0;      // unambiguous bases in a row, ending here
    for (size_t i = 0; i < code.size(); ++i) {
      const uint32_t c = code[i] < 0 ? 0u : (uint32_t)code[i];
      f = pgs::roll_fwd(f, c, k); r = pgs::roll_rc(r, c, k);
      run = code[i] < 0 ? 0 : run + 1;
      if (run < (size_t)k) continue;
      const uint32_t canon = f < r ? f : r;
      std::printf("W %d %zu %08x %08x %08x %d\n", k, i + 1 - (size_t)k, f, r, canon, pgs::sampled(canon, 16u) ? 1 : 0);
    }
  }
  return 0;
}
