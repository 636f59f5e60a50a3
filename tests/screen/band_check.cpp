// band_check — host checker of the index helpers of pyani_amd/csrc/pg_screen_core.h (tests/test_screen_index_cpu.py builds it with
// -fsanitize=address,undefined and runs it): the default band, the band ranges, the item decode of the band count kernel and the search
// for a band's members in a group.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pg_screen_core.h"

static int wrong = 0;
static void check(bool ok, const char* what, uint64_t a, uint64_t b) {
  if (!ok && wrong++ < 20) std::printf("WRONG %s at (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
}

// every row of n genomes lies in exactly one band of `rows` rows, the bands ascend and none is empty
static void check_bands(uint32_t n, uint32_t rows) {
  const uint32_t nb = pgscr::band_count(n, rows);
  uint32_t next = 0;
  for (uint32_t b = 0; b < nb; ++b) {
    uint32_t r0, r1;
    pgscr::band_range(b, rows, n, &r0, &r1);
    check(r0 == next && r1 > r0 && r1 - r0 <= rows && r1 <= n, "band range", n, b);
    check(b + 1 == nb || r1 - r0 == rows, "a short band that is not the last", n, b);
    next = r1;
  }
  check(next == n, "the bands cover the rows", n, rows);
  uint32_t r0, r1;
  pgscr::band_range(nb, rows, n, &r0, &r1);
  check(r0 == n && r1 == n, "the band after the last is empty", n, rows);
}

int main() {
  // 1. the default band: the largest rows <= min(8192, n) with rows * n <= 2^29, checked against its definition
  uint64_t n_checked = 0;
  auto check_default = [&](uint32_t n) {
    const uint32_t rows = pgscr::band_default_rows(n);
    const uint32_t cap = n < pgscr::MAX_BAND_ROWS ? n : pgscr::MAX_BAND_ROWS;
    check(rows >= 1 && rows <= cap && (uint64_t)rows * n <= pgscr::MAX_BAND_CELLS, "default rows", n, rows);
    check(rows == cap || (uint64_t)(rows + 1u) * n > pgscr::MAX_BAND_CELLS, "default rows are the largest", n, rows);
    check(pgscr::band_rows(0, n) == rows && pgscr::band_rows(7, n) == 7, "band setting", n, rows);
    ++n_checked;
  };
  for (uint32_t n = 1; n <= 20000; ++n) check_default(n);
  for (uint32_t n = 65536 - 3; n <= 65536 + 3; ++n) check_default(n);
  for (uint32_t n = pgscr::INDEX_MAX_GENOMES - 1000; n <= pgscr::INDEX_MAX_GENOMES; ++n) check_default(n);
  check(pgscr::band_default_rows(8192) == 8192 && pgscr::band_default_rows(65536) == 8192 && pgscr::band_default_rows(65537) == 8191 &&
            pgscr::band_default_rows(pgscr::INDEX_MAX_GENOMES) == 512,
        "default rows at the named sizes", 0, 0);
  std::printf("ok default %llu\n", (unsigned long long)n_checked);
  // 2. the ranges: every n and rows at small sizes, the default and the extremes at both ends of large ones
  for (uint32_t n = 1; n <= 70; ++n)
    for (uint32_t rows = 1; rows <= 72; ++rows) check_bands(n, rows);
  for (uint32_t n : {8191u, 8192u, 8193u, 65536u, pgscr::INDEX_MAX_GENOMES - 1u, pgscr::INDEX_MAX_GENOMES})
    for (uint32_t rows : {1u, 3000u, 8191u, 8192u, pgscr::band_default_rows(n)}) check_bands(n, rows);
  std::printf("ok ranges\n");
  // 3. the item decode: every item at small sizes; the first and the last item of every band row at the largest group
  n_checked = 0;
  for (uint32_t m = 2; m <= 40; ++m)
    for (uint32_t mb = 1; mb <= m; ++mb) {
      uint64_t t = 0;
      for (uint32_t i = 0; i < mb; ++i)
        for (uint32_t j = 0; j < m; ++j, ++t) {
          uint32_t a, b;
          pgscr::band_item_decode(t, m, &a, &b);
          check(a == i && b == j, "item", m, t);
          ++n_checked;
        }
      check(t == pgscr::band_items(mb, m), "items of a group", m, mb);
    }
  for (uint32_t m : {8192u, 8200u, pgscr::INDEX_MAX_GENOMES - 1u, pgscr::INDEX_MAX_GENOMES}) {
    const uint32_t mb = m < pgscr::MAX_BAND_ROWS ? m : pgscr::MAX_BAND_ROWS;
    for (uint32_t i = 0; i < mb; ++i) {
      uint32_t a, b;
      pgscr::band_item_decode((uint64_t)i * m, m, &a, &b);
      check(a == i && b == 0, "first item of a band row", m, i);
      pgscr::band_item_decode((uint64_t)i * m + m - 1u, m, &a, &b);
      check(a == i && b == m - 1u, "last item of a band row", m, i);
      n_checked += 2;
    }
  }
  check(pgscr::band_items(pgscr::MAX_BAND_ROWS, pgscr::INDEX_MAX_GENOMES) == 1ull << 33, "items beyond 32 bits", 0, 0);
  std::printf("ok items %llu\n", (unsigned long long)n_checked);
  // 4. the members of a group inside a band: the two searches against a linear count, groups with gaps, every band
  n_checked = 0;
  for (uint32_t step = 1; step <= 5; ++step)
    for (uint32_t len = 0; len <= 33; ++len) {
      std::vector<uint32_t> mem(len + 6u, 0xdeadbeefu);      // (three guard entries on either side: the search reads none of them)
      for (uint32_t i = 0; i < len; ++i) mem[3 + i] = 2u + i * step + (i > len / 2 ? 7u : 0u);
      for (uint32_t r0 = 0; r0 <= 190; r0 += 3)
        for (uint32_t r1 : {r0 + 1u, r0 + 4u, r0 + 50u}) {
          const uint64_t a = pgscr::lower_bound_u32(mem.data(), 3, 3 + len, r0), b = pgscr::lower_bound_u32(mem.data(), a, 3 + len, r1);
          uint32_t inside = 0, before = 0;
          for (uint32_t i = 0; i < len; ++i) { inside += mem[3 + i] >= r0 && mem[3 + i] < r1; before += mem[3 + i] < r0; }
          check(a == 3u + before && b - a == inside, "members in a band", len, r0);
          ++n_checked;
        }
    }
  std::printf("ok search %llu\n", (unsigned long long)n_checked);
  return wrong ? 1 : 0;
}
