// tri_check — host checker of pyani_amd/csrc/pg_screen_core.h (tests/test_screen_cpu.py builds it with -fsanitize=address,undefined and
// runs it): the triangle decode of the screen's count kernel, and the cut of the slice bins into parts.
#include <cstdint>
#include <cstdio>

#include "pg_screen_core.h"

static int wrong = 0;
static void check(bool ok, const char* what, uint64_t a, uint64_t b) {
  if (!ok && wrong++ < 20) std::printf("WRONG %s at (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
}

int main() {
  // 1. the first and the last item of every row, every m
  uint64_t n_checked = 0;
  for (uint32_t m = 2; m <= pgscr::MAX_GENOMES; ++m) {
    uint64_t t = 0;
    for (uint32_t i = 0; i + 1 < m; ++i) {
      uint32_t a, b;
      check(pgscr::tri_row_start(i, m) == t, "row_start", m, i);
      pgscr::screen_tri_decode(t, m, &a, &b);
      check(a == i && b == i + 1, "first item of a row", m, i);
      t += m - 1 - i;
      pgscr::screen_tri_decode(t - 1, m, &a, &b);
      check(a == i && b == m - 1, "last item of a row", m, i);
      n_checked += 2;
    }
    check(t == pgscr::tri_items(m), "items of a group", m, t);
  }
  std::printf("ok rows %llu\n", (unsigned long long)n_checked);
  // 2. every item, small m
  n_checked = 0;
  for (uint32_t m = 2; m <= 64; ++m) {
    uint64_t t = 0;
    for (uint32_t i = 0; i + 1 < m; ++i)
      for (uint32_t j = i + 1; j < m; ++j, ++t) {
        uint32_t a, b;
        pgscr::screen_tri_decode(t, m, &a, &b);
        check(a == i && b == j, "item", m, t);
        ++n_checked;
      }
  }
  std::printf("ok items %llu\n", (unsigned long long)n_checked);
  // 3. the parts partition the bins
  for (uint32_t n_parts = 1; n_parts <= 8; ++n_parts) {
    check(pgscr::part_begin(0, n_parts) == 0 && pgscr::part_begin(n_parts, n_parts) == pgscr::N_BINS, "ends of the parts", n_parts, 0);
    for (uint32_t bin = 0; bin < pgscr::N_BINS; ++bin) {
      uint32_t owners = 0;
      for (uint32_t p = 0; p < n_parts; ++p) owners += bin >= pgscr::part_begin(p, n_parts) && bin < pgscr::part_begin(p + 1, n_parts);
      check(owners == 1, "owners of a bin", n_parts, bin);
    }
  }
  std::printf("ok parts\n");
  // 4. a bin is one of the 4096, whatever the scale; a k-mer's bin reads the hash bits above the sampling's
  for (uint32_t log2_scale = 0; log2_scale <= 16; ++log2_scale)
    for (uint32_t x = 0; x < 100000; x += 7) {
      const uint32_t canon = x * 2654435761u;
      check(pgscr::bin_of(canon, log2_scale) < pgscr::N_BINS, "bin range", canon, log2_scale);
      check(pgscr::bin_of(canon, log2_scale) == ((pgs::mix32(canon) >> log2_scale) & 4095u), "bin", canon, log2_scale);
    }
  check(pgscr::valid_scale(1) && pgscr::valid_scale(65536) && !pgscr::valid_scale(3) && !pgscr::valid_scale(0) && !pgscr::valid_scale(131072), "scales", 0, 0);
  std::printf("ok bins\n");
  return wrong ? 1 : 0;
}
