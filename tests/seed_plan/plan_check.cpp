// Stand-alone check of pyani_amd/csrc/pg_seed_plan.h (tests/test_seed_plan_cpu.py builds and runs it, once plain and once under
// the address and undefined-behaviour sanitizers): for every table size S and group size n below, the passes cover [0, n)
// exactly once and in order, none exceeds H = S / 2, there is one pass exactly when n <= H, and n == 0 gives one empty pass.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "pg_seed_plan.h"

int main() {
  int bad = 0, cases = 0;
  const uint32_t sizes[] = {256u, 512u, 16384u};
  for (uint32_t S : sizes) {
    const uint32_t H = pg_seed_pass_entries(S);
    if (H != S / 2) { std::printf("WRONG S=%u: H=%u\n", S, H); ++bad; }
    const uint32_t ns[] = {0u, 1u, H - 1, H, H + 1, 2 * H - 1, 2 * H, 2 * H + 1, 9000u, 1000000u};
    for (uint32_t n : ns) {
      ++cases;
      const uint32_t P = pg_seed_pass_count(n, S);
      bool ok = P >= 1 && (P == 1) == (n <= H) && P == (n == 0 ? 1u : (uint32_t)(((uint64_t)n + H - 1) / H));
      std::vector<uint8_t> seen(n, 0);   // how often each entry is taken
      uint32_t at = 0;                   // the passes come in order and leave no gap
      for (uint32_t p = 0; p < P; ++p) {
        const PgSeedPass R = pg_seed_pass_range(n, S, p);
        ok = ok && R.begin == at && R.begin <= R.end && R.end <= n && R.end - R.begin <= H;
        ok = ok && R.begin == p * H && R.end == (n < (p + 1) * H ? n : (p + 1) * H);
        if (!ok) break;
        for (uint32_t e = R.begin; e < R.end; ++e) ++seen[e];
        at = R.end;
      }
      ok = ok && at == n;
      for (uint32_t e = 0; ok && e < n; ++e) ok = seen[e] == 1;
      if (n == 0) { const PgSeedPass R = pg_seed_pass_range(0, S, 0); ok = ok && P == 1 && R.begin == 0 && R.end == 0; }
      std::printf("%s S=%u n=%u passes=%u\n", ok ? "ok" : "WRONG", S, n, P);
      bad += !ok;
    }
  }
  {   // a group size near 2^32 must not wrap (the lists index entries with 32 bits)
    const uint32_t n = 0xFFFFFFFFu, S = 16384u, P = pg_seed_pass_count(n, S);
    const PgSeedPass L = pg_seed_pass_range(n, S, P - 1);
    const bool ok = P == 524288u && L.begin == (P - 1) * 8192u && L.end == n;
    std::printf("%s S=%u n=%u passes=%u\n", ok ? "ok" : "WRONG", S, n, P);
    bad += !ok; ++cases;
  }
  std::printf("%d cases, %d wrong\n", cases, bad);
  return bad ? 1 : 0;
}
