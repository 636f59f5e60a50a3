// pg_screen_core.h — the definition of the SCREEN mode ("optional k-mer sketch pre-filter to skip hopeless pairs"),
// plain C++ for the device (pg_screen.hip) and for the host checker of the tests (tests/screen/tri_check.cpp).  Built on pgs:: of
// pg_sketch_core.h: the same k-mers, canonical form and FracMinHash sampling, but ONE set per genome and no fragments.
//
//   * parameters: 8 <= k <= 16 (default 16); scale a power of two, 1 ... 65 536 (default 256; scale 1 keeps every k-mer);
//   * S(g) = the set of DISTINCT canonical k-mers of genome g with pgs::sampled(canon, scale), over all records and either strand; only
//     windows of k unambiguous bases inside one record count (the validity rule of the sketch mode's scan); size[g] = |S(g)|;
//   * shared[a][b] = |S(a) ∩ S(b)|, symmetric, shared[a][a] = size[a];
//   * the device produces these INTEGERS only; containment = shared / size[a], jaccard and identity = containment^(1/k) are computed on
//     the host (pyani_amd/screen.py);
//   * the work is cut by k-mer: bin(canon) = (mix32(canon) >> log2(scale)) & 4095 — the hash bits above the ones the sampling reads, so
//     the sampled k-mers spread evenly — and a part or a slice is a contiguous range of bins.  Every k-mer lies in exactly one bin,
//     every bin in exactly one part and one slice, and the counts are integers: the result does not depend on the cut.
//
// An ESTIMATE for triage, with its own outputs: never written into the exact ANIm / ANIb matrices.
#pragma once
#include <stdint.h>

#include "pg_sketch_core.h"

namespace pgscr {

constexpr uint32_t N_BINS = 4096;
constexpr uint32_t MAX_GENOMES = 8192;            // per call: the limit of classify and the heatmap; a 256 MB matrix
constexpr int32_t MAX_SCALE = 65536;
constexpr int32_t DEFAULT_KMER = 16, DEFAULT_SCALE = 256;
constexpr uint64_t DEFAULT_MAX_KEYS = 1ull << 28; // (k-mer, genome) keys of one slice: 2 GB, twice for the sort
constexpr uint64_t LIMIT_MAX_KEYS = 1ull << 30;   // the largest budget pg_screen_set_budget takes

PGS_HD bool valid_scale(int32_t scale) { return scale >= 1 && scale <= MAX_SCALE && (scale & (scale - 1)) == 0; }
// the slice bin of a sampled k-mer
PGS_HD uint32_t bin_of_hash(uint32_t mixed, uint32_t log2_scale) { return (mixed >> log2_scale) & (N_BINS - 1u); }
PGS_HD uint32_t bin_of(uint32_t canon, uint32_t log2_scale) { return bin_of_hash(pgs::mix32(canon), log2_scale); }
// part p of n_parts (1 <= n_parts <= N_BINS) owns the bins [part_begin(p), part_begin(p + 1))
PGS_HD uint32_t part_begin(uint32_t part, uint32_t n_parts) { return (uint32_t)(((uint64_t)N_BINS * part) / n_parts); }

// A group of m genomes (2 <= m <= MAX_GENOMES) that hold one k-mer owns m (m - 1) / 2 items: the cells (i, j), i < j, of its upper
// triangle in row-major order.  Row i starts at item i (2 m - i - 1) / 2 and holds m - 1 - i items.
PGS_HD uint64_t tri_items(uint32_t m) { return (uint64_t)m * (m - 1u) / 2u; }
PGS_HD uint64_t tri_row_start(uint32_t i, uint32_t m) { return (uint64_t)i * (2ull * m - i - 1ull) / 2ull; }
// item t (0 <= t < tri_items(m)) -> (i, j).  The row comes from the root of i^2 - (2 m - 1) i + 2 t = 0 in double precision and is then
// moved by whole rows until row_start(i) <= t < row_start(i + 1): the root may be off by one near a row's first item, the fix-up is exact.
PGS_HD void screen_tri_decode(uint64_t t, uint32_t m, uint32_t* i_out, uint32_t* j_out) {
  const double b = 2.0 * (double)m - 1.0;
  double d = b * b - 8.0 * (double)t;
  if (d < 0.0) d = 0.0;
  int64_t i = (int64_t)((b - pgs::sqrt_rn(d)) * 0.5);
  if (i < 0) i = 0;
  if (i > (int64_t)m - 2) i = (int64_t)m - 2;
  while (i > 0 && tri_row_start((uint32_t)i, m) > t) --i;
  while (i < (int64_t)m - 2 && tri_row_start((uint32_t)i + 1u, m) <= t) ++i;
  *i_out = (uint32_t)i;
  *j_out = (uint32_t)i + 1u + (uint32_t)(t - tri_row_start((uint32_t)i, m));
}

// ---- the screen index: collections beyond MAX_GENOMES, worked a BAND of matrix rows at a time ---------------------------
constexpr uint32_t INDEX_MAX_GENOMES = 1u << 20;  // per pg_screen_index call
constexpr uint32_t MAX_BAND_ROWS = 8192;          // the largest pg_screen_set_band takes, and the default's cap
constexpr uint64_t MAX_BAND_CELLS = 1ull << 29;   // the default band: rows * n <= 2^29 cells (2 GiB of uint32)

// the default band of n >= 1 genomes: the largest rows <= min(MAX_BAND_ROWS, n) with rows * n <= MAX_BAND_CELLS (>= 1 for n <= 2^29)
PGS_HD uint32_t band_default_rows(uint32_t n) {
  uint64_t rows = MAX_BAND_CELLS / n;
  if (rows > MAX_BAND_ROWS) rows = MAX_BAND_ROWS;
  if (rows > n) rows = n;
  return (uint32_t)rows;
}
// setting: what pg_screen_set_band holds (0 = the default)
PGS_HD uint32_t band_rows(uint32_t setting, uint32_t n) { return setting ? setting : band_default_rows(n); }
PGS_HD uint32_t band_count(uint32_t n, uint32_t rows) { return (uint32_t)(((uint64_t)n + rows - 1u) / rows); }
// band b (< band_count) covers the rows [r0, r1) = [b rows, min(n, (b + 1) rows))
PGS_HD void band_range(uint32_t b, uint32_t rows, uint32_t n, uint32_t* r0, uint32_t* r1) {
  const uint64_t lo = (uint64_t)b * rows, hi = lo + rows;
  *r0 = (uint32_t)(lo < n ? lo : n);
  *r1 = (uint32_t)(hi < n ? hi : n);
}
// the search: a chunk of query rows against the n >= 1 columns of a collection.  The same setting; the default is not capped
// by n — the rows are other genomes than the columns — only by MAX_BAND_ROWS and MAX_BAND_CELLS (>= 512 rows for n <= INDEX_MAX_GENOMES)
PGS_HD uint32_t search_default_rows(uint32_t n) {
  const uint64_t rows = MAX_BAND_CELLS / n;
  return (uint32_t)(rows > MAX_BAND_ROWS ? MAX_BAND_ROWS : (rows < 1 ? 1 : rows));
}
PGS_HD uint32_t search_rows(uint32_t setting, uint32_t n) { return setting ? setting : search_default_rows(n); }
// A group of m members, mb of them in the band, owns mb m items: item t (< mb m <= 2^13 2^20) -> (i, j) = (member of the band, member of
// the group), row-major, so that consecutive items run j upward along one band row.
PGS_HD uint64_t band_items(uint32_t mb, uint32_t m) { return (uint64_t)mb * m; }
PGS_HD void band_item_decode(uint64_t t, uint32_t m, uint32_t* i_out, uint32_t* j_out) {
  *i_out = (uint32_t)(t / m);
  *j_out = (uint32_t)(t % m);
}
// the first position p in [lo, hi) of an ascending array with a[p] >= x (hi where there is none)
PGS_HD uint64_t lower_bound_u32(const uint32_t* a, uint64_t lo, uint64_t hi, uint32_t x) {
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2u;
    if (a[mid] < x) lo = mid + 1u; else hi = mid;
  }
  return lo;
}

}  // namespace pgscr
