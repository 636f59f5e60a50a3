// pg_screen.hip — the SCREEN mode on the GPU ("k-mer sketch pre-filter"; definition: pg_screen_core.h).  One call gives the
// n x n matrix of shared sampled k-mers of n genomes without a pair loop: all genomes' (k-mer, genome) keys are sorted once and every k-mer
// held by m genomes adds one to m (m - 1) / 2 cells.  Pairs that share nothing cost nothing.  Integer work over the 2-bit packed genomes
// already resident in HBM; no MFMA.  An ESTIMATE for triage with its own outputs — nothing here touches the exact ANIm / ANIb results or
// the caches of the sketch mode and the ANIm seed lists; every buffer of a call is released before it returns.
//
//   C1 screen_scan_kernel   ALL genomes of the call in one launch: a work item is 256 chunks of 32 start positions of one genome, found
//                           through a prefix table over the genomes; the rolling and validity code is the sketch mode's scan (three code
//                           words, two mask words per lane).  Count pass: the sampled k-mers of the part's bins counted per slice bin in an
//                           LDS histogram, one 64-bit atomic per bin and workgroup into the device histogram.  The host cuts the bins into
//                           contiguous slices of at most max_keys keys.  Fill pass (one per slice): key = canon << 32 | index of the genome
//                           in the call, appended through one cursor, one atomic per wave and position step.
//   C2 sort and group       hipcub radix sort over bits 0 ... 32 + 2 k; hipcub Unique drops a k-mer's second occurrence in one genome;
//                           screen_head_kernel adds the survivors to size[g] (LDS histogram over the genomes) and marks, among the
//                           survivors, the first and the last entry of every k-mer held by >= 2 genomes; two flagged selections give the
//                           groups' first and last entries (the genomes of a group stand in ascending call index: the index is the low half
//                           of the key); screen_weight_kernel + an exclusive scan (uint64) give every group its item range and the total P.
//   C3 screen_count_kernel  balanced by ITEM: a workgroup owns a contiguous range of the P items, finds its first group by binary search and
//                           walks forward 256 items at a time (the window of group offsets it needs: 257 entries in LDS).  Item t of a group
//                           decodes to (i, j), i < j, row-major over the upper triangle (pgscr::screen_tri_decode), so consecutive lanes run
//                           j upward in one matrix row; shared[g_i * n + g_j] += 1 by a uint32 atomic in HBM — integer adds: the result
//                           does not depend on the order of arrival.
//   C4 screen_finish_kernel after the last slice: the upper triangle mirrored, the diagonal = size.
//
// The SELECTION: pg_screen_hold / pg_screen_load leave an n x n matrix resident on the context (ScreenState), and
// pg_screen_select packs the cells a != b with shared[a][b] >= min(need[a], need[b]) as (a, b, shared[a][b]) in row-major order:
//   C5 screen_select_kernel a wave task is SEL_CELLS consecutive cells of one row, 64 at a time (coalesced).  Count pass: the popcounts of the
//                           task's ballots, one uint64 per task; hipcub exclusive scan; fill pass: the same ballots again, every kept cell
//                           written at its task's offset + the kept cells before it in the task.  No cursor, no atomic: the order is the
//                           order of the cells.  Two streaming passes over 4 n^2 bytes.
//
// The INDEX, for collections beyond MAX_GENOMES: C1 and C2 are one front half (screen_front) with two back halves.  The
// dense calls count every grouped slice into the matrix (DenseBack: C3, C4).  pg_screen_index appends the grouped entries to a resident
// compressed-row structure instead (IndexBack: group_start, member; sizes by screen_head_wide_kernel), and pg_screen_index_select /
// _band form the matrix a BAND of rows at a time:
//   B1 band_prep_kernel     per group the members inside the band's rows (two binary searches); the groups with none are compacted away
//   B2 band_weight_kernel   + an exclusive scan: item ranges of the remaining groups, mb m items each
//   B3 band_count_kernel    C3's balance by item; item t -> (t / m, t % m), uint32 atomics into the band
//   B4 band_diag_kernel     the cell of a genome with itself = size
//   B5 band_select_kernel   C5's rule and passes on the rectangle; the kept triples go to the host as the band finishes
//
// The COMPONENTS: which genomes belong together.  pg_screen_components (a list from the host) and
// pg_screen_index_components (the bands' kept triples, where B5 left them on the device) hook a union-find forest that only atomics write
// and sum two 64-bit counts per node; K1 ... K3 stand with their state at the end of this file.
#include <algorithm>
#include <hipcub/hipcub.hpp>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "pg_internal.h"
#include "pg_screen_core.h"

namespace {

struct ScreenGenome {      // one genome of the call
  uint64_t arena_start;    // bases: codes + arena_start / 16, mask + arena_start / 32
  int64_t stream_len;
  uint64_t item0;          // first work item (256 chunks of 32 start positions) of the genome; items of all genomes back to back
};

constexpr uint32_t SCAN_CHUNKS = 256;      // chunks of one work item: one per lane

// counters: [0] the fill pass's append cursor
template <bool FILL, int K>
__global__ __launch_bounds__(256) void screen_scan_kernel(const uint32_t* __restrict__ arena_codes, const uint32_t* __restrict__ arena_mask,
                                                           const ScreenGenome* __restrict__ tab, uint32_t n, uint64_t n_items, uint32_t scale,
                                                           uint32_t log2_scale, uint32_t bin_lo, uint32_t bin_hi, unsigned long long* __restrict__ hist,
                                                           unsigned long long* __restrict__ keys, unsigned long long keys_cap,
                                                           unsigned long long* __restrict__ counters) {
  __shared__ uint32_t lhist[FILL ? 1 : pgscr::N_BINS];
  if (!FILL) {
    for (uint32_t i = threadIdx.x; i < pgscr::N_BINS; i += blockDim.x) lhist[i] = 0u;
    __syncthreads();
  }
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
    uint32_t lo = 0, hi = n - 1u;      // the genome of the item: the last one whose first item is <= item (uniform over the workgroup)
    while (lo < hi) { const uint32_t mid = (lo + hi + 1u) >> 1; if (tab[mid].item0 <= item) lo = mid; else hi = mid - 1u; }
    const uint32_t g = lo;
    const int64_t stream_len = tab[g].stream_len;
    const uint32_t* codes = arena_codes + tab[g].arena_start / 16;
    const uint32_t* mask = arena_mask + tab[g].arena_start / 32;
    const int64_t n_chunks = (stream_len + 31) / 32;
    const int64_t c = (int64_t)(item - tab[g].item0) * SCAN_CHUNKS + threadIdx.x;
    const bool active = c < n_chunks;
    // bases 32 c .. 32 c + 47 = code words 2 c, 2 c + 1, 2 c + 2; mask words c, c + 1 (the arena is padded: reads past the stream see dirty bases)
    uint64_t c01 = 0, m = 0;
    uint32_t c2 = 0;
    if (active) {
      c01 = (uint64_t)codes[2 * c] | ((uint64_t)codes[2 * c + 1] << 32);
      c2 = codes[2 * c + 2];
      m = (uint64_t)mask[c] | ((uint64_t)mask[c + 1] << 32);
    }
    uint32_t f = 0, r = 0;
    constexpr uint64_t WINDOW = (1ull << K) - 1ull;      // the K mask bits of a window
    for (int t = 0; t < 32 + K - 1; ++t) {      // base 32 c + t enters the window; the k-mer that ENDS on it starts at 32 c + t - (K - 1)
      const uint32_t code = t < 32 ? (uint32_t)(c01 >> (2 * t)) & 3u : (c2 >> (2 * (t - 32))) & 3u;
      f = pgs::roll_fwd(f, code, K); r = pgs::roll_rc(r, code, K);
      const int s = t - (K - 1);
      if (s < 0) continue;      // (uniform)
      const int64_t p = 32 * c + s;
      const uint32_t canon = f < r ? f : r;
      const uint32_t h = pgs::mix32(canon);
      const uint32_t bin = pgscr::bin_of_hash(h, log2_scale);
      // an inactive lane has m = 0; an ambiguity symbol, a record end or the stream's end fail the window test
      const bool take = active && p + K <= stream_len && ((m >> s) & WINDOW) == WINDOW && (h & (scale - 1u)) == 0u && bin >= bin_lo && bin < bin_hi;
      if (!FILL) {
        if (take) atomicAdd(&lhist[bin], 1u);
      } else {      // one atomic per wave: every lane of the wave is here (no divergent exit above)
        const unsigned long long bal = __ballot(take);
        if (bal) {
          const int leader = __ffsll(bal) - 1;
          unsigned long long base = 0;
          if ((int)lane == leader) base = atomicAdd(&counters[0], (unsigned long long)__popcll(bal));
          const uint32_t b_lo = __shfl((uint32_t)base, leader, 64), b_hi = __shfl((uint32_t)(base >> 32), leader, 64);
          if (take) {
            const unsigned long long at = (((unsigned long long)b_hi << 32) | b_lo) + (unsigned long long)__popcll(bal & ((1ull << lane) - 1ull));
            if (at < keys_cap) keys[at] = ((unsigned long long)canon << 32) | g;
          }
        }
      }
    }
  }
  if (!FILL) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < pgscr::N_BINS; i += blockDim.x)
      if (lhist[i]) atomicAdd(&hist[i], (unsigned long long)lhist[i]);
  }
}

template <bool FILL>
auto screen_scan_of(int32_t kmer) -> decltype(&screen_scan_kernel<FILL, 16>) {
  switch (kmer) {
    case 8: return screen_scan_kernel<FILL, 8>;
    case 9: return screen_scan_kernel<FILL, 9>;
    case 10: return screen_scan_kernel<FILL, 10>;
    case 11: return screen_scan_kernel<FILL, 11>;
    case 12: return screen_scan_kernel<FILL, 12>;
    case 13: return screen_scan_kernel<FILL, 13>;
    case 14: return screen_scan_kernel<FILL, 14>;
    case 15: return screen_scan_kernel<FILL, 15>;
    case 16: return screen_scan_kernel<FILL, 16>;
  }
  return nullptr;      // (pg_screen_matrix refuses every other k before it gets here)
}

// u: the nu distinct keys of a slice, sorted.  sizes[g] += the entries of genome g; flags[i]: bit 0 = the first, bit 1 = the last entry of
// a k-mer held by two or more genomes
__global__ __launch_bounds__(256) void screen_head_kernel(const unsigned long long* __restrict__ u, uint64_t nu, uint32_t n, uint32_t* __restrict__ sizes,
                                                           uint8_t* __restrict__ flags) {
  __shared__ uint32_t lsize[pgscr::MAX_GENOMES];
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) lsize[i] = 0u;
  __syncthreads();
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nu; i += (uint64_t)gridDim.x * blockDim.x) {
    const unsigned long long key = u[i];
    const uint32_t canon = (uint32_t)(key >> 32), g = (uint32_t)key;
    const bool same_prev = i > 0 && (uint32_t)(u[i - 1] >> 32) == canon;
    const bool same_next = i + 1 < nu && (uint32_t)(u[i + 1] >> 32) == canon;
    flags[i] = (uint8_t)((!same_prev && same_next ? 1u : 0u) | (same_prev && !same_next ? 2u : 0u));
    if (g < n) atomicAdd(&lsize[g], 1u);
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x)
    if (lsize[i]) atomicAdd(&sizes[i], lsize[i]);
}

// The head kernel of the index (n up to 2^20: no LDS histogram of the genomes fits).  sizes[g] += 1 by a uint32 atomic in HBM, one per
// entry, no return value.  The keys stand in (k-mer, genome) order, so the genomes of neighbouring lanes differ inside a group and are
// unrelated across groups: a wave finds next to nothing to aggregate.  flags as above, and bit 2 = the entry belongs to
// a k-mer held by two or more genomes (what the index keeps).
__global__ __launch_bounds__(256) void screen_head_wide_kernel(const unsigned long long* __restrict__ u, uint64_t nu, uint32_t n, uint32_t* __restrict__ sizes,
                                                                uint8_t* __restrict__ flags) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nu; i += (uint64_t)gridDim.x * blockDim.x) {
    const unsigned long long key = u[i];
    const uint32_t canon = (uint32_t)(key >> 32), g = (uint32_t)key;
    const bool same_prev = i > 0 && (uint32_t)(u[i - 1] >> 32) == canon;
    const bool same_next = i + 1 < nu && (uint32_t)(u[i + 1] >> 32) == canon;
    flags[i] = (uint8_t)((!same_prev && same_next ? 1u : 0u) | (same_prev && !same_next ? 2u : 0u) | (same_prev || same_next ? 4u : 0u));
    if (g < n) atomicAdd(&sizes[g], 1u);
  }
}

struct FlagBit {      // the flag array read as one of its bits
  uint32_t bit;
  __host__ __device__ __forceinline__ uint8_t operator()(uint8_t f) const { return (uint8_t)((f >> bit) & 1u); }
};

// w[g] = items of group g (its genomes' pairs), w[ng] = 0: the input of the exclusive scan
__global__ __launch_bounds__(256) void screen_weight_kernel(const uint32_t* __restrict__ first, const uint32_t* __restrict__ last, uint32_t ng,
                                                             unsigned long long* __restrict__ w) {
  for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g <= ng; g += gridDim.x * blockDim.x)
    w[g] = g < ng ? (unsigned long long)pgscr::tri_items(last[g] - first[g] + 1u) : 0ull;
}

// off: [ng + 1] item offsets of the groups (every group owns at least one item), off[ng] = P.  Workgroup b owns the items [b per, (b + 1) per).
__global__ __launch_bounds__(256) void screen_count_kernel(const unsigned long long* __restrict__ u, const uint32_t* __restrict__ first,
                                                            const uint32_t* __restrict__ last, const unsigned long long* __restrict__ off, uint32_t ng,
                                                            unsigned long long P, unsigned long long per, uint32_t n, uint32_t* __restrict__ shared) {
  __shared__ unsigned long long loff[257];
  __shared__ uint32_t next_group;
  const unsigned long long a = (unsigned long long)blockIdx.x * per;
  const unsigned long long b = a + per < P ? a + per : P;
  if (a >= b) return;
  uint32_t lo = 0, hi = ng - 1u;      // the group of item a: the last one whose offset is <= a (uniform over the workgroup)
  while (lo < hi) { const uint32_t mid = (lo + hi + 1u) >> 1; if (off[mid] <= a) lo = mid; else hi = mid - 1u; }
  uint32_t gc = lo;
  for (unsigned long long ta = a; ta < b; ta += 256ull) {
    // items ta ... ta + 255 lie in the groups gc ... gc + 255 at most (a group owns an item or more): their offsets, and the one after
    for (uint32_t w = threadIdx.x; w < 257u; w += blockDim.x) loff[w] = (unsigned long long)gc + w <= ng ? off[gc + w] : P;
    __syncthreads();
    const unsigned long long t = ta + threadIdx.x;
    if (t < b) {
      uint32_t wl = 0, wh = 255;      // the last window entry whose offset is <= t (entries past the last group hold P > t)
      while (wl < wh) { const uint32_t mid = (wl + wh + 1u) >> 1; if (loff[mid] <= t) wl = mid; else wh = mid - 1u; }
      const uint32_t g = gc + wl;
      if (g < ng) {
        const uint32_t s = first[g], m = last[g] - s + 1u;
        uint32_t i, j;
        pgscr::screen_tri_decode(t - loff[wl], m, &i, &j);
        const uint32_t gi = (uint32_t)u[s + i], gj = (uint32_t)u[s + j];
        if (j < m && gi < n && gj < n) atomicAdd(&shared[(size_t)gi * n + gj], 1u);
      }
      if (threadIdx.x == 255u) next_group = loff[wl + 1u] <= t + 1ull ? g + 1u : g;      // the group of item ta + 256
    }
    __syncthreads();
    gc = next_group;      // (read only when another round follows: then lane 255 had an item)
  }
}

__global__ __launch_bounds__(256) void screen_finish_kernel(uint32_t* __restrict__ shared, const uint32_t* __restrict__ sizes, uint32_t n) {
  const uint64_t cells = (uint64_t)n * n;
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < cells; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t a = (uint32_t)(x / n), b = (uint32_t)(x % n);
    if (a == b) shared[x] = sizes[a];
    else if (a > b) shared[x] = shared[(size_t)b * n + a];
  }
}

constexpr uint32_t SEL_STEPS = 8;                  // 64-cell steps of one wave task
constexpr uint32_t SEL_CELLS = 64u * SEL_STEPS;    // cells of one wave task: a piece of ONE matrix row

// Tasks row-major: task = row * tpr + piece (tpr = pieces per row).  !FILL: counts[task] = kept cells of the task, counts[n_tasks] = 0 (the
// scan's total lands there).  FILL: counts = the scanned offsets; total = their last entry, the room of the three output arrays.
template <bool FILL>
__global__ __launch_bounds__(256) void screen_select_kernel(const uint32_t* __restrict__ shared, const uint32_t* __restrict__ need, uint32_t n, uint32_t tpr,
                                                             uint32_t n_tasks, unsigned long long* __restrict__ counts, unsigned long long total,
                                                             int32_t* __restrict__ a_out, int32_t* __restrict__ b_out, uint32_t* __restrict__ s_out) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), n_waves = gridDim.x * (blockDim.x >> 6);
  const unsigned long long below = (1ull << lane) - 1ull;
  for (uint32_t task = wave; task < n_tasks; task += n_waves) {      // (uniform over the wave: every lane reaches every ballot)
    const uint32_t row = task / tpr, col0 = (task % tpr) * SEL_CELLS;
    const uint32_t need_row = need[row];
    const uint32_t* __restrict__ cells = shared + (size_t)row * n;
    uint32_t v[SEL_STEPS];
    bool keep[SEL_STEPS];
#pragma unroll
    for (uint32_t u = 0; u < SEL_STEPS; ++u) {
      const uint32_t col = col0 + 64u * u + lane;
      const bool in = col < n;
      v[u] = in ? cells[col] : 0u;
      const uint32_t need_col = in ? need[col] : 0u;
      keep[u] = in && col != row && v[u] >= (need_row < need_col ? need_row : need_col);
    }
    if (!FILL) {
      uint32_t c = 0;
#pragma unroll
      for (uint32_t u = 0; u < SEL_STEPS; ++u) c += (uint32_t)__popcll(__ballot(keep[u]));
      if (lane == 0) counts[task] = c;
    } else {
      unsigned long long at = counts[task];
#pragma unroll
      for (uint32_t u = 0; u < SEL_STEPS; ++u) {
        const unsigned long long bal = __ballot(keep[u]);
        const unsigned long long mine = at + (unsigned long long)__popcll(bal & below);
        if (keep[u] && mine < total) {
          a_out[mine] = (int32_t)row; b_out[mine] = (int32_t)(col0 + 64u * u + lane); s_out[mine] = v[u];
        }
        at += (unsigned long long)__popcll(bal);
      }
    }
  }
  if (!FILL && blockIdx.x == 0 && threadIdx.x == 0) counts[n_tasks] = 0ull;
}

// ---- the index path: the groups stay resident in compressed-row form, the matrix is formed a band of rows at a time ------
struct LowHalf {      // the genome of a key
  __host__ __device__ __forceinline__ uint32_t operator()(unsigned long long key) const { return (uint32_t)key; }
};
struct NonZero {
  __host__ __device__ __forceinline__ uint8_t operator()(uint32_t x) const { return x ? 1 : 0; }
};

// w[g] = members of slice group g, w[ng] = 0: the input of the scan that continues group_start
__global__ __launch_bounds__(256) void index_size_kernel(const uint32_t* __restrict__ first, const uint32_t* __restrict__ last, uint32_t ng,
                                                          unsigned long long* __restrict__ w) {
  for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g <= ng; g += gridDim.x * blockDim.x)
    w[g] = g < ng ? (unsigned long long)(last[g] - first[g] + 1u) : 0ull;
}

// B1 prep: the members of every group that fall into the rows [r0, r1) — they ascend: two binary searches.  lo[g] = the first of them,
// counted from the group's start; mb[g] = how many.  in_band[0] += the sum of mb (one 64-bit atomic per wave).
__global__ __launch_bounds__(256) void band_prep_kernel(const unsigned long long* __restrict__ start, const uint32_t* __restrict__ member, uint64_t G,
                                                         uint32_t r0, uint32_t r1, uint32_t* __restrict__ lo, uint32_t* __restrict__ mb,
                                                         unsigned long long* __restrict__ in_band) {
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < G; base += (uint64_t)gridDim.x * blockDim.x) {      // (uniform: every lane reaches the shuffles)
    const uint64_t g = base + threadIdx.x;
    uint32_t mine = 0;
    if (g < G) {
      const uint64_t s = start[g], e = start[g + 1];
      const uint64_t a = pgscr::lower_bound_u32(member, s, e, r0);
      const uint64_t b = pgscr::lower_bound_u32(member, a, e, r1);
      lo[g] = (uint32_t)(a - s);
      mb[g] = mine = (uint32_t)(b - a);
    }
    for (int d = 32; d > 0; d >>= 1) mine += __shfl_down(mine, d, 64);      // (at most 64 x 8192)
    if ((threadIdx.x & 63u) == 0u && mine) atomicAdd(in_band, (unsigned long long)mine);
  }
}

// B2 the weights of the groups with a member in the band (active: their indices, ascending): w[i] = mb m, w[na] = 0
__global__ __launch_bounds__(256) void band_weight_kernel(const unsigned long long* __restrict__ active, uint64_t na, const unsigned long long* __restrict__ start,
                                                           const uint32_t* __restrict__ mb, unsigned long long* __restrict__ w) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= na; i += (uint64_t)gridDim.x * blockDim.x) {
    unsigned long long x = 0ull;
    if (i < na) { const uint64_t g = active[i]; x = pgscr::band_items(mb[g], (uint32_t)(start[g + 1] - start[g])); }
    w[i] = x;
  }
}

// B3 count: screen_count_kernel's balance by item over the ACTIVE groups (each owns an item or more: the 257-offset window holds).  Item t
// of a group -> (i, j) = (t / m, t % m): band[(member[lo + i] - r0) n + member[s + j]] += 1; the cell of a genome with itself is left to
// band_diag_kernel.
__global__ __launch_bounds__(256) void band_count_kernel(const unsigned long long* __restrict__ start, const uint32_t* __restrict__ member,
                                                          const unsigned long long* __restrict__ active, const uint32_t* __restrict__ lo,
                                                          const unsigned long long* __restrict__ off, uint64_t na, unsigned long long P, unsigned long long per,
                                                          uint32_t n, uint32_t r0, uint32_t r1, uint32_t* __restrict__ band) {
  __shared__ unsigned long long loff[257];
  __shared__ uint64_t next_group;
  const unsigned long long a = (unsigned long long)blockIdx.x * per;
  const unsigned long long b = a + per < P ? a + per : P;
  if (a >= b) return;
  uint64_t glo = 0, ghi = na - 1u;      // the active group of item a: the last one whose offset is <= a (uniform over the workgroup)
  while (glo < ghi) { const uint64_t mid = (glo + ghi + 1u) >> 1; if (off[mid] <= a) glo = mid; else ghi = mid - 1u; }
  uint64_t gc = glo;
  for (unsigned long long ta = a; ta < b; ta += 256ull) {
    for (uint32_t w = threadIdx.x; w < 257u; w += blockDim.x) loff[w] = gc + w <= na ? off[gc + w] : P;
    __syncthreads();
    const unsigned long long t = ta + threadIdx.x;
    if (t < b) {
      uint32_t wl = 0, wh = 255;      // the last window entry whose offset is <= t (entries past the last group hold P > t)
      while (wl < wh) { const uint32_t mid = (wl + wh + 1u) >> 1; if (loff[mid] <= t) wl = mid; else wh = mid - 1u; }
      const uint64_t ga = gc + wl;
      if (ga < na) {
        const uint64_t g = active[ga];
        const uint64_t s = start[g];
        const uint32_t m = (uint32_t)(start[g + 1] - s);
        uint32_t i, j;
        pgscr::band_item_decode(t - loff[wl], m, &i, &j);
        const uint64_t pi = s + lo[g] + i;
        if (pi < s + m) {
          const uint32_t gi = member[pi], gj = member[s + j];
          if (gi >= r0 && gi < r1 && gj < n && gi != gj) atomicAdd(&band[(size_t)(gi - r0) * n + gj], 1u);
        }
      }
      if (threadIdx.x == 255u) next_group = loff[wl + 1u] <= t + 1ull ? ga + 1u : ga;      // the group of item ta + 256
    }
    __syncthreads();
    gc = next_group;      // (read only when another round follows: then lane 255 had an item)
  }
}

// B4 the diagonal: the cell of row genome a with column genome a = sizes[a]
__global__ __launch_bounds__(256) void band_diag_kernel(uint32_t* __restrict__ band, const uint32_t* __restrict__ sizes, uint32_t r0, uint32_t r1, uint32_t n) {
  for (uint32_t r = r0 + blockIdx.x * blockDim.x + threadIdx.x; r < r1; r += gridDim.x * blockDim.x) band[(size_t)(r - r0) * n + r] = sizes[r];
}

// B5 select: the rule of screen_select_kernel on the rectangle of the rows [r0, r0 + rows) x n columns.  Tasks row-major: task = band row
// * tpr + piece, SEL_CELLS cells of ONE row; counts / total as there.  The output carries the GLOBAL row r0 + band row.
template <bool FILL>
__global__ __launch_bounds__(256) void band_select_kernel(const uint32_t* __restrict__ band, const uint32_t* __restrict__ need, uint32_t n, uint32_t r0, uint32_t tpr,
                                                           uint32_t n_tasks, unsigned long long* __restrict__ counts, unsigned long long total,
                                                           int32_t* __restrict__ a_out, int32_t* __restrict__ b_out, uint32_t* __restrict__ s_out) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), n_waves = gridDim.x * (blockDim.x >> 6);
  const unsigned long long below = (1ull << lane) - 1ull;
  for (uint32_t task = wave; task < n_tasks; task += n_waves) {      // (uniform over the wave: every lane reaches every ballot)
    const uint32_t brow = task / tpr, col0 = (task % tpr) * SEL_CELLS;
    const uint32_t row = r0 + brow;
    const uint32_t need_row = need[row];
    const uint32_t* __restrict__ cells = band + (size_t)brow * n;
    uint32_t v[SEL_STEPS];
    bool keep[SEL_STEPS];
#pragma unroll
    for (uint32_t u = 0; u < SEL_STEPS; ++u) {
      const uint32_t col = col0 + 64u * u + lane;
      const bool in = col < n;
      v[u] = in ? cells[col] : 0u;
      const uint32_t need_col = in ? need[col] : 0u;
      keep[u] = in && col != row && v[u] >= (need_row < need_col ? need_row : need_col);
    }
    if (!FILL) {
      uint32_t c = 0;
#pragma unroll
      for (uint32_t u = 0; u < SEL_STEPS; ++u) c += (uint32_t)__popcll(__ballot(keep[u]));
      if (lane == 0) counts[task] = c;
    } else {
      unsigned long long at = counts[task];
#pragma unroll
      for (uint32_t u = 0; u < SEL_STEPS; ++u) {
        const unsigned long long bal = __ballot(keep[u]);
        const unsigned long long mine = at + (unsigned long long)__popcll(bal & below);
        if (keep[u] && mine < total) {
          a_out[mine] = (int32_t)row; b_out[mine] = (int32_t)(col0 + 64u * u + lane); s_out[mine] = v[u];
        }
        at += (unsigned long long)__popcll(bal);
      }
    }
  }
  if (!FILL && blockIdx.x == 0 && threadIdx.x == 0) counts[n_tasks] = 0ull;
}

struct IndexState {      // the resident k-mer index of pg_screen_index and the latest selection over it
  uint32_t n = 0;
  uint64_t G = 0, E = 0;                        // groups (k-mers held by >= 2 genomes), grouped entries
  PgDevBuf<unsigned long long> d_start;         // group_start: G + 1
  PgDevBuf<uint32_t> d_member;                  // E: the call indices of a group's genomes, ascending inside a group
  PgDevBuf<uint32_t> d_sizes;                   // n
  bool selected = false;
  std::vector<int32_t> a, b;                    // the kept triples of the latest pg_screen_index_select, on the host: bands go as they finish
  std::vector<uint32_t> s;
};

IndexState* index_of(pg_ctx* ctx) { return static_cast<IndexState*>(ctx->screen_index_state); }

struct ScreenState {      // the resident matrix of pg_screen_hold / pg_screen_load and the latest selection over it
  uint32_t n = 0;
  PgDevBuf<uint32_t> d_shared;      // n x n
  bool selected = false;
  uint64_t n_sel = 0;
  PgDevBuf<int32_t> d_a, d_b;       // n_sel each
  PgDevBuf<uint32_t> d_s;
};

ScreenState* state_of(pg_ctx* ctx) { return static_cast<ScreenState*>(ctx->screen_state); }

struct ScreenEvents {      // pg_screen_last: event pairs on the context's stream, summed per stage after the call's last synchronisation
  std::vector<hipEvent_t> ev;
  std::vector<int> stage;      // of the pair ev[2 i], ev[2 i + 1]
  bool ok = true;
  ~ScreenEvents() { for (auto e : ev) (void)hipEventDestroy(e); }
  void mark(hipStream_t s) {
    hipEvent_t e = nullptr;
    if (!ok || hipEventCreate(&e) != hipSuccess) { (void)hipGetLastError(); ok = false; return; }
    ev.push_back(e);
    if (hipEventRecord(e, s) != hipSuccess) { (void)hipGetLastError(); ok = false; }
  }
  void begin(int st, hipStream_t s) { if (ok) { stage.push_back(st); mark(s); } }
  void end(hipStream_t s) { if (ok) mark(s); }
  void sum(double* ms, int n_stages = 3) {
    for (int i = 0; i < n_stages; ++i) ms[i] = 0.0;
    if (!ok) return;
    for (size_t i = 0; i < stage.size() && 2 * i + 1 < ev.size(); ++i) {
      float x = 0.f;
      if (hipEventElapsedTime(&x, ev[2 * i], ev[2 * i + 1]) == hipSuccess) ms[stage[i]] += (double)x; else (void)hipGetLastError();
    }
  }
};

uint32_t grid_for(uint64_t items, uint32_t per_block, uint32_t cap) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + per_block - 1) / per_block, cap));
}

}  // namespace

extern "C" int pg_screen_set_budget(pg_ctx* ctx, uint64_t max_keys) {
  if (!ctx) return PG_E_ARG;
  if (max_keys > pgscr::LIMIT_MAX_KEYS) return pg_fail(ctx, PG_E_ARG, "screen: the key budget of a slice is at most 2^30");
  ctx->screen_max_keys = max_keys;
  return PG_OK;
}

extern "C" int pg_screen_last(pg_ctx* ctx, uint64_t* out5, double* ms3) {
  if (!ctx || !out5 || !ms3) return pg_fail(ctx, PG_E_ARG, "bad argument");
  for (int i = 0; i < 5; ++i) out5[i] = ctx->screen_last[i];
  for (int i = 0; i < 3; ++i) ms3[i] = ctx->screen_ms[i];
  return PG_OK;
}

namespace {

// the argument checks of pg_screen_matrix and pg_screen_hold (want_shared: the call has a matrix to copy out, shared_out)
int screen_check(pg_ctx* ctx, const int32_t* genome_ids, uint32_t n, int32_t kmer, int32_t scale, uint32_t part, uint32_t n_parts, const uint32_t* sizes_out,
                 bool want_shared, const uint32_t* shared_out, uint32_t max_n = pgscr::MAX_GENOMES,
                 const char* too_many = "screen: more than 8192 genomes in one call") {
  if (n > max_n) return pg_fail(ctx, PG_E_ARG, too_many);      // (before the ids are read)
  if (n && (!genome_ids || !sizes_out || (want_shared && !shared_out))) return pg_fail(ctx, PG_E_ARG, "bad argument");
  if (kmer < pgs::K_MIN || kmer > pgs::K_MAX) return pg_fail(ctx, PG_E_ARG, "screen: the k-mer size must be 8 ... 16");
  if (!pgscr::valid_scale(scale)) return pg_fail(ctx, PG_E_ARG, "screen: scale must be a power of two, 1 ... 65536");
  if (n_parts < 1 || n_parts > pgscr::N_BINS || part >= n_parts) return pg_fail(ctx, PG_E_ARG, "screen: 1 <= n_parts <= 4096 and part < n_parts");
  std::vector<char> seen(ctx->genomes.size(), 0);
  for (uint32_t i = 0; i < n; ++i) {
    if (genome_ids[i] < 0 || (size_t)genome_ids[i] >= ctx->genomes.size()) return pg_fail(ctx, PG_E_ARG, "genome id out of range");
    if (seen[genome_ids[i]]) return pg_fail(ctx, PG_E_ARG, "screen: genome id " + std::to_string(genome_ids[i]) + " is given twice");
    seen[genome_ids[i]] = 1;
  }
  return PG_OK;
}

struct SliceGroups {      // one slice, sorted and grouped, on the device: what the front half hands to a back half
  const unsigned long long* u;      // the nu distinct keys, sorted
  uint64_t nu;
  const uint8_t* flags;             // of the head kernel, one per key
  const uint32_t* first;            // the first and the last entry of each of the ng k-mers held by >= 2 genomes
  const uint32_t* last;
  uint64_t ng;
  void* tmp;                        // temporary storage of the library calls: what the front half needs, and what prepare() asked for
  size_t tmp_bytes;
};

struct FrontTotals { uint64_t keys = 0, distinct = 0, groups = 0, slices = 0; };

// The FRONT HALF of a screen of checked arguments (n >= 1), shared by the dense calls and the index: the count pass, slices of whole bins
// under the budget, and per slice the fill pass, the radix sort, Unique and the head kernel's sizes and first / last marks (C1, C2 above).
// What becomes of a grouped slice is the back half's: back.prepare(all keys, keys of the largest slice, its bound of groups, tmp bytes to
// raise) once before the first slice, back.slice(S, T) per slice.  d_sizes (the caller's, empty) holds the finished sizes on return.
// wide_head: screen_head_wide_kernel (any n, bit 2 of the flags) instead of the LDS histogram of at most MAX_GENOMES genomes.
template <typename Back>
int screen_front(pg_ctx* ctx, const int32_t* genome_ids, uint32_t n, int32_t kmer, int32_t scale, uint32_t part, uint32_t n_parts, bool wide_head,
                 PgDevBuf<uint32_t>& d_sizes, ScreenEvents& T, FrontTotals& tot, Back& back) {
  int rc;
  const auto scan_count = screen_scan_of<false>(kmer);
  const auto scan_fill = screen_scan_of<true>(kmer);
  if (!scan_count || !scan_fill) return pg_fail(ctx, PG_E_ARG, "screen: no scan kernel for this k-mer size");
  uint32_t log2_scale = 0;
  while ((1 << log2_scale) < scale) ++log2_scale;
  const uint32_t bin_lo = pgscr::part_begin(part, n_parts), bin_hi = pgscr::part_begin(part + 1u, n_parts);
  const uint64_t max_keys = ctx->screen_max_keys ? ctx->screen_max_keys : pgscr::DEFAULT_MAX_KEYS;
  hipStream_t st = ctx->stream;
  const uint32_t cu_blocks = (uint32_t)ctx->num_cu * 8u;

  // the prefix table over the genomes
  std::vector<ScreenGenome> tab(n);
  uint64_t n_items = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const PgGenome& G = ctx->genomes[genome_ids[i]];
    tab[i].arena_start = G.arena_start; tab[i].stream_len = (int64_t)G.stream_len; tab[i].item0 = n_items;
    const uint64_t chunks = (G.stream_len + 31) / 32;
    n_items += (chunks + SCAN_CHUNKS - 1) / SCAN_CHUNKS;
  }
  PgDevBuf<ScreenGenome> d_tab;
  PgDevBuf<unsigned long long> d_hist, d_counters;      // [N_BINS] | [0] append cursor, [1] distinct keys, [2] groups
  if ((rc = sk_malloc(ctx, d_tab, n)) || (rc = sk_malloc(ctx, d_hist, pgscr::N_BINS)) || (rc = sk_malloc(ctx, d_counters, 4)) ||
      (rc = sk_malloc(ctx, d_sizes, n)))
    return rc;
  PG_HIP(ctx, hipMemcpyAsync(d_tab, tab.data(), (size_t)n * sizeof(ScreenGenome), hipMemcpyHostToDevice, st));
  PG_HIP(ctx, hipMemsetAsync(d_hist, 0, pgscr::N_BINS * 8, st));
  PG_HIP(ctx, hipMemsetAsync(d_sizes, 0, (size_t)n * 4, st));
  const dim3 scan_grid(grid_for(n_items, 1, cu_blocks));
  std::vector<unsigned long long> hist(pgscr::N_BINS, 0ull);
  if (n_items) {
    T.begin(0, st);
    hipLaunchKernelGGL(scan_count, scan_grid, dim3(256), 0, st, ctx->d_codes.p, ctx->d_mask.p, d_tab.p, n, n_items, (uint32_t)scale, log2_scale, bin_lo,
                       bin_hi, d_hist.p, (unsigned long long*)nullptr, 0ull, (unsigned long long*)nullptr);
    T.end(st);
    PG_HIP(ctx, hipGetLastError());
    PG_HIP(ctx, hipMemcpyAsync(hist.data(), d_hist, pgscr::N_BINS * 8, hipMemcpyDeviceToHost, st));
    PG_HIP(ctx, hipStreamSynchronize(st));
  }
  // contiguous slices of at most max_keys keys
  struct Slice { uint32_t lo, hi; uint64_t keys; };
  std::vector<Slice> slices;
  uint64_t total_keys = 0, slice_max = 0;
  {
    Slice cur{bin_lo, bin_lo, 0};
    for (uint32_t bin = bin_lo; bin < bin_hi; ++bin) {
      const uint64_t c = hist[bin];
      if (c > max_keys)
        return pg_fail(ctx, PG_E_NOMEM, "screen: slice bin " + std::to_string(bin) + " alone holds " + std::to_string(c) + " keys, more than the budget of " +
                                            std::to_string(max_keys) + " keys of one slice (pg_screen_set_budget; a larger scale or more parts make the bins smaller)");
      if (cur.keys + c > max_keys) { slices.push_back(cur); cur = Slice{bin, bin, 0}; }
      cur.keys += c; cur.hi = bin + 1u;
    }
    if (cur.keys) slices.push_back(cur);
    for (const Slice& s : slices) { total_keys += s.keys; slice_max = std::max(slice_max, s.keys); }
  }
  tot.keys = total_keys; tot.slices = slices.size();
  if (!slices.empty()) {
    PgDevBuf<unsigned long long> keys_a, keys_b;
    PgDevBuf<uint32_t> first, last;
    PgDevBuf<uint8_t> flags, tmp;
    const size_t max_groups = (size_t)(slice_max / 2 + 2);
    if ((rc = sk_malloc(ctx, keys_a, (size_t)slice_max + 1)) || (rc = sk_malloc(ctx, keys_b, (size_t)slice_max + 1)) ||
        (rc = sk_malloc(ctx, flags, (size_t)slice_max + 1)) || (rc = sk_malloc(ctx, first, max_groups)) || (rc = sk_malloc(ctx, last, max_groups)))
      return rc;
    // temporary storage of the library calls: the largest any of them asks for at the largest slice
    const int end_bit = 32 + 2 * kmer;
    unsigned long long* d_nu = d_counters.p + 1;
    unsigned long long* d_ng = d_counters.p + 2;
    hipcub::CountingInputIterator<uint32_t> counting(0u);
    hipcub::TransformInputIterator<uint8_t, FlagBit, const uint8_t*> is_first(flags.p, FlagBit{0u}), is_last(flags.p, FlagBit{1u});
    size_t tmp_bytes = 0, need = 0;
    PG_HIP(ctx, hipcub::DeviceRadixSort::SortKeys(nullptr, need, (const unsigned long long*)keys_a.p, keys_b.p, (int64_t)slice_max, 0, end_bit, st));
    tmp_bytes = std::max(tmp_bytes, need);
    PG_HIP(ctx, hipcub::DeviceSelect::Unique(nullptr, need, (const unsigned long long*)keys_b.p, keys_a.p, d_nu, (int64_t)slice_max, st));
    tmp_bytes = std::max(tmp_bytes, need);
    PG_HIP(ctx, hipcub::DeviceSelect::Flagged(nullptr, need, counting, is_first, first.p, d_ng, (int64_t)slice_max, st));
    tmp_bytes = std::max(tmp_bytes, need);
    if ((rc = back.prepare(total_keys, slice_max, max_groups, tmp_bytes))) return rc;
    if ((rc = sk_malloc(ctx, tmp, tmp_bytes + 16))) return rc;

    for (const Slice& S : slices) {
      // fill
      T.begin(0, st);
      PG_HIP(ctx, hipMemsetAsync(d_counters, 0, 4 * 8, st));
      hipLaunchKernelGGL(scan_fill, scan_grid, dim3(256), 0, st, ctx->d_codes.p, ctx->d_mask.p, d_tab.p, n, n_items, (uint32_t)scale, log2_scale, S.lo, S.hi,
                         (unsigned long long*)nullptr, keys_a.p, (unsigned long long)S.keys, d_counters.p);
      T.end(st);
      PG_HIP(ctx, hipGetLastError());
      // sort, drop a genome's repeats, mark the groups
      T.begin(1, st);
      size_t tb = tmp_bytes;
      PG_HIP(ctx, hipcub::DeviceRadixSort::SortKeys((void*)tmp.p, tb, (const unsigned long long*)keys_a.p, keys_b.p, (int64_t)S.keys, 0, end_bit, st));
      tb = tmp_bytes;
      PG_HIP(ctx, hipcub::DeviceSelect::Unique((void*)tmp.p, tb, (const unsigned long long*)keys_b.p, keys_a.p, d_nu, (int64_t)S.keys, st));
      unsigned long long cnt[3] = {0, 0, 0};      // cursor, distinct, (groups)
      PG_HIP(ctx, hipMemcpyAsync(cnt, d_counters, 2 * 8, hipMemcpyDeviceToHost, st));
      PG_HIP(ctx, hipStreamSynchronize(st));
      if (cnt[0] != S.keys)
        return pg_fail(ctx, PG_E_INTERNAL, "screen: the fill pass appended " + std::to_string(cnt[0]) + " keys where the count pass saw " + std::to_string(S.keys));
      const uint64_t nu = cnt[1];
      tot.distinct += nu;
      hipLaunchKernelGGL(wide_head ? screen_head_wide_kernel : screen_head_kernel, dim3(grid_for(nu, 256 * 16, cu_blocks)), dim3(256), 0, st,
                         (const unsigned long long*)keys_a.p, nu, n, d_sizes.p, flags.p);
      PG_HIP(ctx, hipGetLastError());
      tb = tmp_bytes;
      PG_HIP(ctx, hipcub::DeviceSelect::Flagged((void*)tmp.p, tb, counting, is_first, first.p, d_ng, (int64_t)nu, st));
      tb = tmp_bytes;
      PG_HIP(ctx, hipcub::DeviceSelect::Flagged((void*)tmp.p, tb, counting, is_last, last.p, d_ng, (int64_t)nu, st));
      PG_HIP(ctx, hipMemcpyAsync(&cnt[2], d_ng, 8, hipMemcpyDeviceToHost, st));
      T.end(st);
      PG_HIP(ctx, hipStreamSynchronize(st));
      const uint64_t ng = cnt[2];
      if (ng + 1 > max_groups) return pg_fail(ctx, PG_E_INTERNAL, "screen: more groups than half the keys");
      tot.groups += ng;
      const SliceGroups G{keys_a.p, nu, flags.p, first.p, last.p, ng, (void*)tmp.p, tmp_bytes};
      if ((rc = back.slice(G, T))) return rc;
    }
  }
  return PG_OK;
}

// The back half of the dense calls (C2's item ranges, C3): every grouped slice is counted into the n x n matrix.
struct DenseBack {
  pg_ctx* ctx;
  uint32_t n;
  uint32_t* d_shared;
  PgDevBuf<unsigned long long> wts, off;
  uint64_t n_incr = 0;
  int prepare(uint64_t, uint64_t, size_t max_groups, size_t& tmp_bytes) {
    int rc;
    if ((rc = sk_malloc(ctx, wts, max_groups)) || (rc = sk_malloc(ctx, off, max_groups))) return rc;
    size_t need = 0;
    PG_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, need, wts.p, off.p, (int64_t)max_groups, ctx->stream));
    tmp_bytes = std::max(tmp_bytes, need);
    return PG_OK;
  }
  int slice(const SliceGroups& S, ScreenEvents& T) {
    hipStream_t st = ctx->stream;
    unsigned long long P = 0;
    if (S.ng) {
      T.begin(1, st);
      hipLaunchKernelGGL(screen_weight_kernel, dim3(grid_for(S.ng + 1, 256, (uint32_t)ctx->num_cu * 8u)), dim3(256), 0, st, S.first, S.last, (uint32_t)S.ng, wts.p);
      PG_HIP(ctx, hipGetLastError());
      size_t tb = S.tmp_bytes;
      PG_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(S.tmp, tb, wts.p, off.p, (int64_t)(S.ng + 1), st));
      PG_HIP(ctx, hipMemcpyAsync(&P, off.p + S.ng, 8, hipMemcpyDeviceToHost, st));
      T.end(st);
      PG_HIP(ctx, hipStreamSynchronize(st));
    }
    n_incr += P;
    if (P) {
      const uint64_t n_wg = std::max<uint64_t>(1, std::min<uint64_t>((P + 2047) / 2048, (uint64_t)ctx->num_cu * 32));
      const unsigned long long per = (P + n_wg - 1) / n_wg;
      T.begin(2, st);
      hipLaunchKernelGGL(screen_count_kernel, dim3((uint32_t)((P + per - 1) / per)), dim3(256), 0, st, S.u, S.first, S.last, (const unsigned long long*)off.p,
                         (uint32_t)S.ng, P, per, n, d_shared);
      T.end(st);
      PG_HIP(ctx, hipGetLastError());
    }
    return PG_OK;
  }
};

// The screen of checked arguments.  The finished matrix is left in d_shared (the caller's: pg_screen_matrix lets it go, pg_screen_hold keeps
// it); sizes_out, and shared_out where it is given, are on the host when this returns.
int screen_run(pg_ctx* ctx, const int32_t* genome_ids, uint32_t n, int32_t kmer, int32_t scale, uint32_t part, uint32_t n_parts, uint32_t* sizes_out,
               uint32_t* shared_out, PgDevBuf<uint32_t>& d_shared) {
  for (int i = 0; i < 5; ++i) ctx->screen_last[i] = 0;
  for (int i = 0; i < 3; ++i) ctx->screen_ms[i] = 0.0;
  if (n == 0) return PG_OK;
  PG_HIP(ctx, hipSetDevice(ctx->device));
  int rc;
  if ((rc = pg_upload(ctx))) return rc;
  hipStream_t st = ctx->stream;
  if ((rc = sk_malloc(ctx, d_shared, (size_t)n * n))) return rc;
  PG_HIP(ctx, hipMemsetAsync(d_shared, 0, (size_t)n * n * 4, st));
  PgDevBuf<uint32_t> d_sizes;
  ScreenEvents T;
  FrontTotals tot;
  DenseBack back{ctx, n, d_shared.p};
  if ((rc = screen_front(ctx, genome_ids, n, kmer, scale, part, n_parts, false, d_sizes, T, tot, back))) return rc;
  hipLaunchKernelGGL(screen_finish_kernel, dim3(grid_for((uint64_t)n * n, 256 * 4, (uint32_t)ctx->num_cu * 8u)), dim3(256), 0, st, d_shared.p,
                     (const uint32_t*)d_sizes.p, n);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(sizes_out, d_sizes, (size_t)n * 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && shared_out) e = hipMemcpyAsync(shared_out, d_shared, (size_t)n * n * 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return pg_fail(ctx, PG_E_HIP, std::string("screen: ") + hipGetErrorString(e));
  ctx->screen_last[0] = tot.keys; ctx->screen_last[1] = tot.distinct; ctx->screen_last[2] = tot.groups; ctx->screen_last[3] = back.n_incr;
  ctx->screen_last[4] = tot.slices;
  T.sum(ctx->screen_ms);
  return PG_OK;
}

}  // namespace

extern "C" int pg_screen_matrix(pg_ctx* ctx, const int32_t* genome_ids, uint32_t n, int32_t kmer, int32_t scale, uint32_t part, uint32_t n_parts,
                                uint32_t* sizes_out, uint32_t* shared_out) {
  if (!ctx) return PG_E_ARG;
  int rc;
  if ((rc = screen_check(ctx, genome_ids, n, kmer, scale, part, n_parts, sizes_out, true, shared_out))) return rc;
  PgDevBuf<uint32_t> d_shared;
  return screen_run(ctx, genome_ids, n, kmer, scale, part, n_parts, sizes_out, shared_out, d_shared);
}

// ---- the resident matrix and the selection over it ---------------------------------------------------------------------------------------
void pg_screen_drop(pg_ctx* ctx) {
  if (!ctx->screen_state) return;
  delete state_of(ctx);
  ctx->screen_state = nullptr;
}

extern "C" int pg_screen_release(pg_ctx* ctx) {
  if (!ctx) return PG_E_ARG;
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  pg_screen_drop(ctx);
  return PG_OK;
}

extern "C" int pg_screen_hold(pg_ctx* ctx, const int32_t* genome_ids, uint32_t n, int32_t kmer, int32_t scale, uint32_t part, uint32_t n_parts,
                              uint32_t* sizes_out) {
  if (!ctx) return PG_E_ARG;
  int rc;
  if ((rc = screen_check(ctx, genome_ids, n, kmer, scale, part, n_parts, sizes_out, false, nullptr))) return rc;
  if ((rc = pg_screen_release(ctx))) return rc;      // the matrix of an earlier call goes before the new one is made: never two at a time
  PgDevBuf<uint32_t> d_shared;
  if ((rc = screen_run(ctx, genome_ids, n, kmer, scale, part, n_parts, sizes_out, nullptr, d_shared))) return rc;
  if (n == 0) return PG_OK;      // (nothing to hold: a selection needs a matrix of one genome or more)
  ScreenState* S = new ScreenState();
  S->n = n;
  S->d_shared = std::move(d_shared);
  ctx->screen_state = S;
  return PG_OK;
}

extern "C" int pg_screen_load(pg_ctx* ctx, const uint32_t* shared, uint32_t n) {
  if (!ctx) return PG_E_ARG;
  if (n > pgscr::MAX_GENOMES) return pg_fail(ctx, PG_E_ARG, "screen: more than 8192 genomes in one call");      // (before the matrix is read)
  if (n == 0 || !shared) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  int rc;
  if ((rc = pg_screen_release(ctx))) return rc;
  PgDevBuf<uint32_t> d_shared;
  if ((rc = sk_malloc(ctx, d_shared, (size_t)n * n))) return rc;
  PG_HIP(ctx, hipMemcpyAsync(d_shared, shared, (size_t)n * n * 4, hipMemcpyHostToDevice, ctx->stream));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ScreenState* S = new ScreenState();
  S->n = n;
  S->d_shared = std::move(d_shared);
  ctx->screen_state = S;
  return PG_OK;
}

extern "C" int pg_screen_fetch(pg_ctx* ctx, uint32_t* shared_out) {
  if (!ctx) return PG_E_ARG;
  ScreenState* S = state_of(ctx);
  if (!S) return pg_fail(ctx, PG_E_ARG, "screen: no resident matrix (call pg_screen_hold or pg_screen_load first)");
  if (!shared_out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PG_HIP(ctx, hipMemcpyAsync(shared_out, S->d_shared, (size_t)S->n * S->n * 4, hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PG_OK;
}

extern "C" int pg_screen_select(pg_ctx* ctx, const uint32_t* need, uint32_t n, uint64_t* n_pairs_out) {
  if (!ctx) return PG_E_ARG;
  ScreenState* S = state_of(ctx);
  if (!S) return pg_fail(ctx, PG_E_ARG, "screen: no resident matrix (call pg_screen_hold or pg_screen_load first)");
  if (n != S->n) return pg_fail(ctx, PG_E_ARG, "screen: the resident matrix is of " + std::to_string(S->n) + " genomes, not " + std::to_string(n));
  if (!need || !n_pairs_out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  S->selected = false;
  S->n_sel = 0;
  // (pg_dev_alloc, not sk_malloc: what sk_malloc gives up when memory is short includes the matrix this call reads)
  const uint32_t tpr = (n + SEL_CELLS - 1) / SEL_CELLS, n_tasks = n * tpr;      // at most 8192 x 16
  const dim3 grid(grid_for(n_tasks, 4, (uint32_t)ctx->num_cu * 8u));
  PgDevBuf<uint32_t> d_need;
  PgDevBuf<unsigned long long> d_cnt, d_off;
  PgDevBuf<uint8_t> tmp;
  int rc;
  if ((rc = pg_dev_alloc(ctx, "screen", d_need, n, "the thresholds")) || (rc = pg_dev_alloc(ctx, "screen", d_cnt, (size_t)n_tasks + 1, "the task counts")) ||
      (rc = pg_dev_alloc(ctx, "screen", d_off, (size_t)n_tasks + 1, "the task offsets")))
    return rc;
  size_t tmp_bytes = 0;
  PG_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, d_cnt.p, d_off.p, (int64_t)n_tasks + 1, st));
  if ((rc = pg_dev_alloc(ctx, "screen", tmp, tmp_bytes + 16, "the scan's temporary storage"))) return rc;
  PG_HIP(ctx, hipMemcpyAsync(d_need, need, (size_t)n * 4, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(screen_select_kernel<false>, grid, dim3(256), 0, st, (const uint32_t*)S->d_shared.p, (const uint32_t*)d_need.p, n, tpr, n_tasks, d_cnt.p, 0ull,
                     (int32_t*)nullptr, (int32_t*)nullptr, (uint32_t*)nullptr);
  PG_HIP(ctx, hipGetLastError());
  PG_HIP(ctx, hipcub::DeviceScan::ExclusiveSum((void*)tmp.p, tmp_bytes, d_cnt.p, d_off.p, (int64_t)n_tasks + 1, st));
  unsigned long long total = 0;
  PG_HIP(ctx, hipMemcpyAsync(&total, d_off.p + n_tasks, 8, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipStreamSynchronize(st));
  if (total > (unsigned long long)n * (n - 1u)) return pg_fail(ctx, PG_E_INTERNAL, "screen: the selection counted more cells than the matrix has off its diagonal");
  if (total) {
    if ((rc = pg_dev_alloc(ctx, "screen", S->d_a, (size_t)total, "the selected pairs")) || (rc = pg_dev_alloc(ctx, "screen", S->d_b, (size_t)total, "the selected pairs")) ||
        (rc = pg_dev_alloc(ctx, "screen", S->d_s, (size_t)total, "the selected pairs")))
      return rc;
    hipLaunchKernelGGL(screen_select_kernel<true>, grid, dim3(256), 0, st, (const uint32_t*)S->d_shared.p, (const uint32_t*)d_need.p, n, tpr, n_tasks, d_off.p, total,
                       S->d_a.p, S->d_b.p, S->d_s.p);
    PG_HIP(ctx, hipGetLastError());
    PG_HIP(ctx, hipStreamSynchronize(st));      // (d_need and d_off go with this scope)
  }
  S->selected = true;
  S->n_sel = total;
  *n_pairs_out = total;
  return PG_OK;
}

extern "C" int pg_screen_select_read(pg_ctx* ctx, int32_t* a_out, int32_t* b_out, uint32_t* shared_out) {
  if (!ctx) return PG_E_ARG;
  ScreenState* S = state_of(ctx);
  if (!S || !S->selected) return pg_fail(ctx, PG_E_ARG, "screen: no selection (call pg_screen_select first)");
  if (S->n_sel == 0) return PG_OK;
  if (!a_out || !b_out || !shared_out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PG_HIP(ctx, hipMemcpyAsync(a_out, S->d_a, S->n_sel * 4, hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipMemcpyAsync(b_out, S->d_b, S->n_sel * 4, hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipMemcpyAsync(shared_out, S->d_s, S->n_sel * 4, hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PG_OK;
}

// ---- the screen index and its bands ----------------------------------------------------------------------------------------
namespace {

// The back half of pg_screen_index: the grouped entries of every slice are appended to group_start / member; nothing is counted.
struct IndexBack {
  pg_ctx* ctx;
  IndexState* I;
  PgDevBuf<unsigned long long> wts, d_sel;      // the groups' sizes of a slice | [0] the entries Flagged kept
  size_t cap_groups = 0, cap_entries = 0;
  int prepare(uint64_t total_keys, uint64_t slice_max, size_t max_groups, size_t& tmp_bytes) {
    // every grouped entry is a distinct key and every group holds two of them or more: E <= keys, G <= keys / 2
    cap_entries = (size_t)total_keys;
    cap_groups = (size_t)(total_keys / 2);
    hipStream_t st = ctx->stream;
    int rc;
    if ((rc = sk_malloc(ctx, wts, max_groups)) || (rc = sk_malloc(ctx, d_sel, 1))) return rc;
    if (sk_malloc(ctx, I->d_member, cap_entries + 1) || sk_malloc(ctx, I->d_start, cap_groups + 2))
      return pg_fail(ctx, PG_E_NOMEM, "screen: no device memory for an index of up to " + std::to_string(cap_entries) + " entries (4 bytes each) in " +
                                          std::to_string(cap_groups) + " groups (8 bytes each)");
    PG_HIP(ctx, hipMemsetAsync(I->d_start, 0, 8, st));
    hipcub::TransformInputIterator<uint32_t, LowHalf, const unsigned long long*> genome((const unsigned long long*)nullptr, LowHalf{});
    hipcub::TransformInputIterator<uint8_t, FlagBit, const uint8_t*> grouped((const uint8_t*)nullptr, FlagBit{2u});
    size_t need = 0;
    PG_HIP(ctx, hipcub::DeviceSelect::Flagged(nullptr, need, genome, grouped, I->d_member.p, d_sel.p, (int64_t)slice_max, st));
    tmp_bytes = std::max(tmp_bytes, need);
    PG_HIP(ctx, hipcub::DeviceScan::ExclusiveScan(nullptr, need, wts.p, I->d_start.p, hipcub::Sum(), 0ull, (int64_t)max_groups, st));
    tmp_bytes = std::max(tmp_bytes, need);
    return PG_OK;
  }
  int slice(const SliceGroups& S, ScreenEvents& T) {
    if (!S.ng) return PG_OK;
    hipStream_t st = ctx->stream;
    if (I->G + S.ng > cap_groups) return pg_fail(ctx, PG_E_INTERNAL, "screen: more groups than half the keys");
    T.begin(1, st);
    // group_start continues at E: the slice's group sizes scanned from there; the entry after the last group is the next slice's first
    hipLaunchKernelGGL(index_size_kernel, dim3(grid_for(S.ng + 1, 256, (uint32_t)ctx->num_cu * 8u)), dim3(256), 0, st, S.first, S.last, (uint32_t)S.ng, wts.p);
    PG_HIP(ctx, hipGetLastError());
    size_t tb = S.tmp_bytes;
    PG_HIP(ctx, hipcub::DeviceScan::ExclusiveScan(S.tmp, tb, wts.p, I->d_start.p + I->G, hipcub::Sum(), (unsigned long long)I->E, (int64_t)(S.ng + 1), st));
    // member: the genomes of the grouped entries, in key order (inside a group the call index ascends: it is the low half of the key)
    hipcub::TransformInputIterator<uint32_t, LowHalf, const unsigned long long*> genome(S.u, LowHalf{});
    hipcub::TransformInputIterator<uint8_t, FlagBit, const uint8_t*> grouped(S.flags, FlagBit{2u});
    tb = S.tmp_bytes;
    PG_HIP(ctx, hipcub::DeviceSelect::Flagged(S.tmp, tb, genome, grouped, I->d_member.p + I->E, d_sel.p, (int64_t)S.nu, st));   // (at most nu <= the slice's keys: room by cap_entries)
    unsigned long long kept = 0, end = 0;
    PG_HIP(ctx, hipMemcpyAsync(&kept, d_sel.p, 8, hipMemcpyDeviceToHost, st));
    PG_HIP(ctx, hipMemcpyAsync(&end, I->d_start.p + I->G + S.ng, 8, hipMemcpyDeviceToHost, st));
    T.end(st);
    PG_HIP(ctx, hipStreamSynchronize(st));
    if (end != I->E + kept || I->E + kept > cap_entries)
      return pg_fail(ctx, PG_E_INTERNAL, "screen: the index took " + std::to_string(kept) + " entries of a slice whose groups hold " + std::to_string(end - I->E));
    I->G += S.ng; I->E += kept;
    return PG_OK;
  }
};

// the band setting of the context against an index of n genomes
uint32_t rows_for(const pg_ctx* ctx, uint32_t n) { return pgscr::band_rows(ctx->screen_band_rows, n); }

struct BandWork {      // the device buffers of the band calls: one band and what prep, count and select need beside it
  PgDevBuf<uint32_t> band, lo, mb, need, s;
  PgDevBuf<unsigned long long> active, wts, off, counters, cnt, coff;      // counters: [0] active groups, [1] members in the band
  PgDevBuf<int32_t> a, b;
  PgDevBuf<uint8_t> tmp;
  size_t tmp_bytes = 0;
};

// (pg_dev_alloc, not sk_malloc: the band calls leave the resident matrix of pg_screen_hold / _load alone, however short memory is)
int band_alloc(pg_ctx* ctx, const IndexState* I, uint32_t rows, bool select, BandWork& W) {
  hipStream_t st = ctx->stream;
  const size_t G = (size_t)I->G;
  int rc;
  if ((rc = pg_dev_alloc(ctx, "screen", W.band, (size_t)rows * I->n, "a band of the index")) || (rc = pg_dev_alloc(ctx, "screen", W.lo, G, "the band's group ranges")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.mb, G, "the band's group ranges")) || (rc = pg_dev_alloc(ctx, "screen", W.active, G, "the band's groups")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.wts, G + 1, "the band's group weights")) || (rc = pg_dev_alloc(ctx, "screen", W.off, G + 1, "the band's item offsets")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.counters, 2, "the band's counters")))
    return rc;
  hipcub::CountingInputIterator<unsigned long long> counting(0ull);
  hipcub::TransformInputIterator<uint8_t, NonZero, const uint32_t*> has((const uint32_t*)W.mb.p, NonZero{});
  size_t need = 0;
  PG_HIP(ctx, hipcub::DeviceSelect::Flagged(nullptr, need, counting, has, W.active.p, W.counters.p, (int64_t)G, st));
  W.tmp_bytes = std::max(W.tmp_bytes, need);
  PG_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, need, W.wts.p, W.off.p, (int64_t)G + 1, st));
  W.tmp_bytes = std::max(W.tmp_bytes, need);
  if (select) {
    const uint32_t tpr = (I->n + SEL_CELLS - 1) / SEL_CELLS;
    const size_t n_tasks = (size_t)rows * tpr;
    if ((rc = pg_dev_alloc(ctx, "screen", W.need, I->n, "the thresholds")) || (rc = pg_dev_alloc(ctx, "screen", W.cnt, n_tasks + 1, "the task counts")) ||
        (rc = pg_dev_alloc(ctx, "screen", W.coff, n_tasks + 1, "the task offsets")))
      return rc;
    PG_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, need, W.cnt.p, W.coff.p, (int64_t)n_tasks + 1, st));
    W.tmp_bytes = std::max(W.tmp_bytes, need);
  }
  return pg_dev_alloc(ctx, "screen", W.tmp, W.tmp_bytes + 16, "the library calls' temporary storage");
}

// B1 ... B4: the rows [r0, r1) of the matrix in W.band, the diagonal included.  *incr += the increments of the count kernel.
int band_fill(pg_ctx* ctx, const IndexState* I, uint32_t r0, uint32_t r1, BandWork& W, uint64_t* incr) {
  hipStream_t st = ctx->stream;
  const uint32_t n = I->n, cu_blocks = (uint32_t)ctx->num_cu * 8u;
  PG_HIP(ctx, hipMemsetAsync(W.band, 0, (size_t)(r1 - r0) * n * 4, st));
  if (I->G) {
    PG_HIP(ctx, hipMemsetAsync(W.counters, 0, 2 * 8, st));
    hipLaunchKernelGGL(band_prep_kernel, dim3(grid_for(I->G, 256, cu_blocks)), dim3(256), 0, st, (const unsigned long long*)I->d_start.p, (const uint32_t*)I->d_member.p,
                       I->G, r0, r1, W.lo.p, W.mb.p, W.counters.p + 1);
    PG_HIP(ctx, hipGetLastError());
    hipcub::CountingInputIterator<unsigned long long> counting(0ull);
    hipcub::TransformInputIterator<uint8_t, NonZero, const uint32_t*> has((const uint32_t*)W.mb.p, NonZero{});
    size_t tb = W.tmp_bytes;
    PG_HIP(ctx, hipcub::DeviceSelect::Flagged((void*)W.tmp.p, tb, counting, has, W.active.p, W.counters.p, (int64_t)I->G, st));
    unsigned long long c[2] = {0, 0};
    PG_HIP(ctx, hipMemcpyAsync(c, W.counters, 2 * 8, hipMemcpyDeviceToHost, st));
    PG_HIP(ctx, hipStreamSynchronize(st));
    const uint64_t na = c[0];
    if (na > I->G) return pg_fail(ctx, PG_E_INTERNAL, "screen: more groups in a band than in the index");
    if (na) {
      unsigned long long P = 0;
      hipLaunchKernelGGL(band_weight_kernel, dim3(grid_for(na + 1, 256, cu_blocks)), dim3(256), 0, st, (const unsigned long long*)W.active.p, na,
                         (const unsigned long long*)I->d_start.p, (const uint32_t*)W.mb.p, W.wts.p);
      PG_HIP(ctx, hipGetLastError());
      tb = W.tmp_bytes;
      PG_HIP(ctx, hipcub::DeviceScan::ExclusiveSum((void*)W.tmp.p, tb, W.wts.p, W.off.p, (int64_t)(na + 1), st));
      PG_HIP(ctx, hipMemcpyAsync(&P, W.off.p + na, 8, hipMemcpyDeviceToHost, st));
      PG_HIP(ctx, hipStreamSynchronize(st));
      if (P < c[1]) return pg_fail(ctx, PG_E_INTERNAL, "screen: fewer items in a band than members");
      *incr += P - c[1];      // every member of the band meets itself once among its group's items: no increment (band_count_kernel)
      const uint64_t n_wg = std::max<uint64_t>(1, std::min<uint64_t>((P + 2047) / 2048, (uint64_t)ctx->num_cu * 32));
      const unsigned long long per = (P + n_wg - 1) / n_wg;
      hipLaunchKernelGGL(band_count_kernel, dim3((uint32_t)((P + per - 1) / per)), dim3(256), 0, st, (const unsigned long long*)I->d_start.p,
                         (const uint32_t*)I->d_member.p, (const unsigned long long*)W.active.p, (const uint32_t*)W.lo.p, (const unsigned long long*)W.off.p, na, P, per,
                         n, r0, r1, W.band.p);
      PG_HIP(ctx, hipGetLastError());
    }
  }
  hipLaunchKernelGGL(band_diag_kernel, dim3(grid_for(r1 - r0, 256, cu_blocks)), dim3(256), 0, st, W.band.p, (const uint32_t*)I->d_sizes.p, r0, r1, n);
  PG_HIP(ctx, hipGetLastError());
  return PG_OK;
}

// B1 ... B5 of one band: the rows [r0, r1) counted (band_fill, event stage fill_stage) and selected by W.need (event stage select_stage,
// LEFT OPEN: the caller ends it once it has queued what it does with the triples).  On return the *total kept triples of the band stand in
// W.a, W.b, W.s in row-major order and the stream is idle.  Shared by pg_screen_index_select and pg_screen_index_components.
int band_select(pg_ctx* ctx, const IndexState* I, uint32_t r0, uint32_t r1, uint32_t tpr, BandWork& W, ScreenEvents& T, int fill_stage, int select_stage,
                uint64_t* incr, unsigned long long* total_out) {
  hipStream_t st = ctx->stream;
  const uint32_t n = I->n;
  T.begin(fill_stage, st);
  int rc = band_fill(ctx, I, r0, r1, W, incr);
  T.end(st);
  if (rc) return rc;
  const uint32_t n_tasks = (r1 - r0) * tpr;      // rows * n <= 2^33 cells in pieces of 512: below 2^32
  const dim3 grid(grid_for(n_tasks, 4, (uint32_t)ctx->num_cu * 8u));
  T.begin(select_stage, st);
  hipLaunchKernelGGL(band_select_kernel<false>, grid, dim3(256), 0, st, (const uint32_t*)W.band.p, (const uint32_t*)W.need.p, n, r0, tpr, n_tasks, W.cnt.p, 0ull,
                     (int32_t*)nullptr, (int32_t*)nullptr, (uint32_t*)nullptr);
  PG_HIP(ctx, hipGetLastError());
  size_t tb = W.tmp_bytes;
  PG_HIP(ctx, hipcub::DeviceScan::ExclusiveSum((void*)W.tmp.p, tb, W.cnt.p, W.coff.p, (int64_t)n_tasks + 1, st));
  unsigned long long total = 0;
  PG_HIP(ctx, hipMemcpyAsync(&total, W.coff.p + n_tasks, 8, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipStreamSynchronize(st));
  if (total > (unsigned long long)(r1 - r0) * n) return pg_fail(ctx, PG_E_INTERNAL, "screen: the selection counted more cells than the band has");
  if (total) {
    if (W.a.reserve((size_t)total) != hipSuccess || W.b.reserve((size_t)total) != hipSuccess || W.s.reserve((size_t)total) != hipSuccess) {
      (void)hipGetLastError();
      return pg_fail(ctx, PG_E_NOMEM, "screen: no device memory for the " + std::to_string(total) + " selected pairs of a band");
    }
    hipLaunchKernelGGL(band_select_kernel<true>, grid, dim3(256), 0, st, (const uint32_t*)W.band.p, (const uint32_t*)W.need.p, n, r0, tpr, n_tasks, W.coff.p, total,
                       W.a.p, W.b.p, W.s.p);
    PG_HIP(ctx, hipGetLastError());
  }
  *total_out = total;
  return PG_OK;
}

}  // namespace

void pg_screen_index_drop(pg_ctx* ctx) {
  if (!ctx->screen_index_state) return;
  delete index_of(ctx);
  ctx->screen_index_state = nullptr;
}

extern "C" int pg_screen_index_release(pg_ctx* ctx) {
  if (!ctx) return PG_E_ARG;
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  pg_screen_index_drop(ctx);
  return PG_OK;
}

extern "C" int pg_screen_set_band(pg_ctx* ctx, uint32_t rows) {
  if (!ctx) return PG_E_ARG;
  if (rows > pgscr::MAX_BAND_ROWS) return pg_fail(ctx, PG_E_ARG, "screen: a band is of at most 8192 rows");
  ctx->screen_band_rows = rows;
  return PG_OK;
}

extern "C" int pg_screen_index_last(pg_ctx* ctx, uint64_t* counts_out, double* ms_out) {
  if (!ctx || !counts_out || !ms_out) return pg_fail(ctx, PG_E_ARG, "bad argument");
  for (int i = 0; i < 7; ++i) counts_out[i] = ctx->screen_index_last[i];
  for (int i = 0; i < 4; ++i) ms_out[i] = ctx->screen_index_ms[i];
  return PG_OK;
}

extern "C" int pg_screen_index(pg_ctx* ctx, const int32_t* genome_ids, uint32_t n, int32_t kmer, int32_t scale, uint32_t* sizes_out) {
  if (!ctx) return PG_E_ARG;
  int rc;
  if ((rc = screen_check(ctx, genome_ids, n, kmer, scale, 0, 1, sizes_out, false, nullptr, pgscr::INDEX_MAX_GENOMES,
                         "screen: more than 1048576 (2^20) genomes in one index")))
    return rc;
  if ((rc = pg_screen_index_release(ctx))) return rc;      // the index of an earlier call goes before the new one is made: never two at a time
  for (int i = 0; i < 7; ++i) ctx->screen_index_last[i] = 0;
  for (int i = 0; i < 4; ++i) ctx->screen_index_ms[i] = 0.0;
  if (n == 0) return PG_OK;      // (nothing to index)
  PG_HIP(ctx, hipSetDevice(ctx->device));
  if ((rc = pg_upload(ctx))) return rc;
  hipStream_t st = ctx->stream;
  std::unique_ptr<IndexState> I(new IndexState());
  I->n = n;
  ScreenEvents T;
  FrontTotals tot;
  {
    IndexBack back{ctx, I.get()};
    if ((rc = screen_front(ctx, genome_ids, n, kmer, scale, 0, 1, true, I->d_sizes, T, tot, back))) return rc;
  }      // (the slices' buffers are gone here)
  if (!I->d_start.p) {      // no slice at all: an index without groups
    if ((rc = sk_malloc(ctx, I->d_start, 1)) || (rc = sk_malloc(ctx, I->d_member, 1))) return rc;
    PG_HIP(ctx, hipMemsetAsync(I->d_start, 0, 8, st));
  }
  PG_HIP(ctx, hipMemcpyAsync(sizes_out, I->d_sizes, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipStreamSynchronize(st));
  // the arrays were sized by the keys before anything was grouped: an index that is much smaller moves into blocks of its own size
  if (I->d_member.cap > 2 * (size_t)I->E + 1024) {
    PgDevBuf<uint32_t> m;
    PgDevBuf<unsigned long long> s;
    if (m.reserve((size_t)I->E + 1) == hipSuccess && s.reserve((size_t)I->G + 1) == hipSuccess) {
      PG_HIP(ctx, hipMemcpyAsync(m, I->d_member, (size_t)I->E * 4, hipMemcpyDeviceToDevice, st));
      PG_HIP(ctx, hipMemcpyAsync(s, I->d_start, ((size_t)I->G + 1) * 8, hipMemcpyDeviceToDevice, st));
      PG_HIP(ctx, hipStreamSynchronize(st));
      I->d_member = std::move(m); I->d_start = std::move(s);
    } else {
      (void)hipGetLastError();      // (no room for the copy: the index stays where it is)
    }
  }
  ctx->screen_index_last[0] = tot.keys; ctx->screen_index_last[1] = tot.distinct; ctx->screen_index_last[2] = I->E; ctx->screen_index_last[3] = I->G;
  ctx->screen_index_last[4] = tot.slices;
  double ms[3];
  T.sum(ms);
  ctx->screen_index_ms[0] = ms[0]; ctx->screen_index_ms[1] = ms[1];
  ctx->screen_index_state = I.release();
  return PG_OK;
}

extern "C" int pg_screen_index_band(pg_ctx* ctx, uint32_t band, uint32_t* out) {
  if (!ctx) return PG_E_ARG;
  IndexState* I = index_of(ctx);
  if (!I) return pg_fail(ctx, PG_E_ARG, "screen: no resident index (call pg_screen_index first)");
  const uint32_t rows = rows_for(ctx, I->n), n_bands = pgscr::band_count(I->n, rows);
  if (band >= n_bands) return pg_fail(ctx, PG_E_ARG, "screen: band " + std::to_string(band) + " does not exist (the index has " + std::to_string(n_bands) + " bands of " +
                                                         std::to_string(rows) + " rows)");
  if (!out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  uint32_t r0, r1;
  pgscr::band_range(band, rows, I->n, &r0, &r1);
  BandWork W;
  uint64_t incr = 0;
  int rc;
  if ((rc = band_alloc(ctx, I, r1 - r0, false, W)) || (rc = band_fill(ctx, I, r0, r1, W, &incr))) return rc;
  PG_HIP(ctx, hipMemcpyAsync(out, W.band, (size_t)(r1 - r0) * I->n * 4, hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PG_OK;
}

extern "C" int pg_screen_index_select(pg_ctx* ctx, const uint32_t* need, uint32_t n, uint32_t band_first, uint32_t band_step, uint64_t* n_pairs_out) {
  if (!ctx) return PG_E_ARG;
  IndexState* I = index_of(ctx);
  if (!I) return pg_fail(ctx, PG_E_ARG, "screen: no resident index (call pg_screen_index first)");
  if (n != I->n) return pg_fail(ctx, PG_E_ARG, "screen: the resident index is of " + std::to_string(I->n) + " genomes, not " + std::to_string(n));
  if (band_step < 1) return pg_fail(ctx, PG_E_ARG, "screen: band_step must be 1 or more");
  if (!need || !n_pairs_out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  I->selected = false;
  I->a.clear(); I->b.clear(); I->s.clear();
  ctx->screen_index_last[5] = ctx->screen_index_last[6] = 0;
  ctx->screen_index_ms[2] = ctx->screen_index_ms[3] = 0.0;
  const uint32_t rows = rows_for(ctx, n), n_bands = pgscr::band_count(n, rows);
  const uint32_t tpr = (n + SEL_CELLS - 1) / SEL_CELLS;
  uint64_t incr = 0, worked = 0;
  ScreenEvents T;
  if (band_first < n_bands) {
    BandWork W;
    int rc;
    if ((rc = band_alloc(ctx, I, std::min(rows, n), true, W))) return rc;
    PG_HIP(ctx, hipMemcpyAsync(W.need, need, (size_t)n * 4, hipMemcpyHostToDevice, st));
    for (uint64_t band = band_first; band < n_bands; band += band_step) {
      uint32_t r0, r1;
      pgscr::band_range((uint32_t)band, rows, n, &r0, &r1);
      unsigned long long total = 0;
      if ((rc = band_select(ctx, I, r0, r1, tpr, W, T, 2, 3, &incr, &total))) return rc;
      if (total) {
        // the band's triples go to the host as it finishes: the device never holds more than one band
        const size_t at = I->a.size();
        try {
          I->a.resize(at + total); I->b.resize(at + total); I->s.resize(at + total);
        } catch (const std::bad_alloc&) {
          I->a.clear(); I->b.clear(); I->s.clear();
          return pg_fail(ctx, PG_E_NOMEM, "screen: no host memory for " + std::to_string(at + total) + " selected pairs");
        }
        PG_HIP(ctx, hipMemcpyAsync(I->a.data() + at, W.a, (size_t)total * 4, hipMemcpyDeviceToHost, st));
        PG_HIP(ctx, hipMemcpyAsync(I->b.data() + at, W.b, (size_t)total * 4, hipMemcpyDeviceToHost, st));
        PG_HIP(ctx, hipMemcpyAsync(I->s.data() + at, W.s, (size_t)total * 4, hipMemcpyDeviceToHost, st));
      }
      T.end(st);
      PG_HIP(ctx, hipStreamSynchronize(st));
      ++worked;
    }
  }
  double ms[4];
  T.sum(ms, 4);
  ctx->screen_index_ms[2] = ms[2]; ctx->screen_index_ms[3] = ms[3];
  ctx->screen_index_last[5] = worked; ctx->screen_index_last[6] = incr;
  I->selected = true;
  *n_pairs_out = I->a.size();
  return PG_OK;
}

extern "C" int pg_screen_index_read(pg_ctx* ctx, int32_t* a_out, int32_t* b_out, uint32_t* shared_out) {
  if (!ctx) return PG_E_ARG;
  IndexState* I = index_of(ctx);
  if (!I || !I->selected) return pg_fail(ctx, PG_E_ARG, "screen: no selection over an index (call pg_screen_index_select first)");
  if (I->a.empty()) return PG_OK;
  if (!a_out || !b_out || !shared_out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  std::copy(I->a.begin(), I->a.end(), a_out);
  std::copy(I->b.begin(), I->b.end(), b_out);
  std::copy(I->s.begin(), I->s.end(), shared_out);
  return PG_OK;
}

// ---- the connected components of the kept pairs -------------------------------------------------------------------------------
// A union-find forest over the n nodes in ONE array, parent[v] <= v, a root being its own parent.  Only atomics write it: the hook is a
// compare-and-swap on a root's own cell, the path halving an atomic minimum.  So a cell only ever DECREASES, a cell that has left its own
// index never returns to it, and every value a cell has held is a smaller node of the same tree.  Every plain or stale read of the array is
// therefore harmless — it names a node of the right tree, no larger than the one it was read for — and what is decided rests on the value
// a compare-and-swap returned.  No thread waits for another: every loop below walks a strictly decreasing node index (§16.3 has the argument).
//   K1 components_init_kernel     parent[v] = v, entries = weight = 0
//   K2 components_hook_kernel     one pass over a list (a chunk of the host's, or a band's kept triples): accumulate — a run of equal a
//                                 inside a wave is summed by a segmented shuffle reduction and adds ONCE to entries[a] and weight[a], 64-bit
//                                 atomics without return value — and hook: both roots found, the larger hooked under the smaller
//   K3 components_flatten_kernel  root[v] = the root of v's tree (halving as it goes); the roots counted, one atomic per wave
namespace {

struct ComponentsState {      // the resident result of the latest accepted components call
  uint32_t n = 0;
  PgDevBuf<uint32_t> d_parent;                      // n: the forest
  PgDevBuf<int32_t> d_root;                         // n: flattened
  PgDevBuf<unsigned long long> d_entries, d_weight; // n each
  PgDevBuf<unsigned long long> d_count;             // [0] the roots
};

ComponentsState* components_of(pg_ctx* ctx) { return static_cast<ComponentsState*>(ctx->screen_components_state); }

constexpr uint64_t COMPONENTS_CHUNK = 1ull << 24;      // host entries uploaded at a time: 192 MB of device memory whatever m is

__global__ __launch_bounds__(256) void components_init_kernel(uint32_t* __restrict__ parent, unsigned long long* __restrict__ entries,
                                                               unsigned long long* __restrict__ weight, uint32_t n) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) { parent[v] = v; entries[v] = 0ull; weight[v] = 0ull; }
}

__device__ __forceinline__ uint32_t components_peek(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// A root-looking node of u's tree, no larger than u (u < n): u moves to a strictly smaller node every round, so at most u rounds.  What it
// returns may have been hooked since — the caller's compare-and-swap finds that out.
__device__ __forceinline__ uint32_t components_find(uint32_t* parent, uint32_t u) {
  for (;;) {
    const uint32_t p = components_peek(parent + u);
    if (p >= u) return u;                      // (p == u: a root as far as this read knows; p > u never happens, and would not be followed)
    const uint32_t g = components_peek(parent + p);
    if (g >= p) return p;
    atomicMin(parent + u, g);                  // halving: g < p < u is a node of u's tree; no return value
    u = g;
  }
}

__global__ __launch_bounds__(256) void components_hook_kernel(const int32_t* __restrict__ a, const int32_t* __restrict__ b, const uint32_t* __restrict__ s,
                                                               uint64_t m, uint32_t n, uint32_t* parent, unsigned long long* __restrict__ entries,
                                                               unsigned long long* __restrict__ weight) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  for (uint64_t base = wave * 64ull; base < m; base += n_waves * 64ull) {      // (uniform over the wave: every lane reaches the shuffles)
    const uint64_t e = base + lane;
    const bool in = e < m;
    const uint32_t ua = in ? (uint32_t)a[e] : 0xFFFFFFFFu, ub = in ? (uint32_t)b[e] : 0xFFFFFFFFu;
    const bool work = in && ua != ub && ua < n && ub < n;      // (the host has refused an index outside [0, n): the bound is kept for the memory's sake)
    unsigned long long cnt = work ? 1ull : 0ull, w = work ? (s ? (unsigned long long)s[e] : 1ull) : 0ull;
    // accumulate: runs of equal a in consecutive lanes; run = the number of run heads up to this lane, so equal run numbers are one run
    const uint32_t prev = __shfl_up(ua, 1, 64);
    const bool head = lane == 0u || ua != prev;
    const unsigned long long heads = __ballot(head);
    const uint32_t run = (uint32_t)__popcll(heads & ((2ull << lane) - 1ull));      // (lane 63: 2 << 63 wraps to 0, minus one = every bit)
    for (uint32_t d = 1; d < 64u; d <<= 1) {
      const uint32_t r2 = __shfl_down(run, d, 64);
      const unsigned long long c2 = __shfl_down(cnt, d, 64), w2 = __shfl_down(w, d, 64);
      if (lane + d < 64u && r2 == run) { cnt += c2; w += w2; }
    }
    if (head && cnt) { atomicAdd(entries + ua, cnt); atomicAdd(weight + ua, w); }
    // hook
    if (work) {
      uint32_t u = components_find(parent, ua), v = components_find(parent, ub);
      while (u != v) {      // u in a's tree, v in b's; max(u, v) drops with every failed round
        if (u < v) { const uint32_t t = u; u = v; v = t; }
        const uint32_t old = atomicCAS(parent + u, u, v);
        if (old == u) break;      // u was a root and now hangs under v < u
        if (old > u) break;       // (never: a cell only decreases; kept so that a broken array cannot spin)
        u = components_find(parent, old);      // old < u: u's parent when the swap looked; on from its tree's top
      }
    }
  }
}

__global__ __launch_bounds__(256) void components_flatten_kernel(uint32_t* parent, uint32_t n, int32_t* __restrict__ root, unsigned long long* __restrict__ count) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {      // (uniform over the workgroup)
    const uint32_t v = base + threadIdx.x;
    bool is_root = false;
    if (v < n) {
      const uint32_t r = components_find(parent, v);      // (no hook runs beside this kernel: what looks like a root is one)
      root[v] = (int32_t)r;
      is_root = r == v;
    }
    const unsigned long long roots = __ballot(is_root);
    if (lane == 0u && roots) atomicAdd(count, (unsigned long long)__popcll(roots));
  }
}

int components_alloc(pg_ctx* ctx, uint32_t n, ComponentsState& C) {
  int rc;
  if ((rc = pg_dev_alloc(ctx, "screen", C.d_parent, n, "the components' forest")) || (rc = pg_dev_alloc(ctx, "screen", C.d_root, n, "the components' roots")) ||
      (rc = pg_dev_alloc(ctx, "screen", C.d_entries, n, "the components' entry counts")) || (rc = pg_dev_alloc(ctx, "screen", C.d_weight, n, "the components' weights")) ||
      (rc = pg_dev_alloc(ctx, "screen", C.d_count, 1, "the components' counter")))
    return rc;
  C.n = n;
  hipLaunchKernelGGL(components_init_kernel, dim3(grid_for(n, 256, (uint32_t)ctx->num_cu * 8u)), dim3(256), 0, ctx->stream, C.d_parent.p, C.d_entries.p, C.d_weight.p, n);
  PG_HIP(ctx, hipGetLastError());
  PG_HIP(ctx, hipMemsetAsync(C.d_count, 0, 8, ctx->stream));
  return PG_OK;
}

// K2 over m triples that stand on the device (s may be null: every entry counts 1)
int components_hook(pg_ctx* ctx, ComponentsState& C, const int32_t* d_a, const int32_t* d_b, const uint32_t* d_s, uint64_t m) {
  if (!m) return PG_OK;
  hipLaunchKernelGGL(components_hook_kernel, dim3(grid_for(m, 256 * 4, (uint32_t)ctx->num_cu * 8u)), dim3(256), 0, ctx->stream, d_a, d_b, d_s, m, C.n, C.d_parent.p,
                     C.d_entries.p, C.d_weight.p);
  PG_HIP(ctx, hipGetLastError());
  return PG_OK;
}

// K3, the count read back, and the finished state made the context's (the earlier one goes here, not before)
int components_finish(pg_ctx* ctx, std::unique_ptr<ComponentsState>& C, ScreenEvents& T, uint64_t worked, uint64_t ignored, uint32_t* n_components_out) {
  hipStream_t st = ctx->stream;
  T.begin(2, st);
  hipLaunchKernelGGL(components_flatten_kernel, dim3(grid_for(C->n, 256, (uint32_t)ctx->num_cu * 8u)), dim3(256), 0, st, C->d_parent.p, C->n, C->d_root.p, C->d_count.p);
  T.end(st);
  PG_HIP(ctx, hipGetLastError());
  unsigned long long count = 0;
  PG_HIP(ctx, hipMemcpyAsync(&count, C->d_count, 8, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipStreamSynchronize(st));
  if (count < 1 || count > C->n) return pg_fail(ctx, PG_E_INTERNAL, "screen: " + std::to_string(count) + " components of " + std::to_string(C->n) + " nodes");
  pg_screen_components_drop(ctx);
  ctx->screen_components_last[0] = C->n; ctx->screen_components_last[1] = worked; ctx->screen_components_last[2] = ignored; ctx->screen_components_last[3] = count;
  T.sum(ctx->screen_components_ms, 3);
  ctx->screen_components_state = C.release();
  *n_components_out = (uint32_t)count;
  return PG_OK;
}

}  // namespace

void pg_screen_components_drop(pg_ctx* ctx) {
  if (!ctx->screen_components_state) return;
  delete components_of(ctx);
  ctx->screen_components_state = nullptr;
  for (int i = 0; i < 4; ++i) ctx->screen_components_last[i] = 0;
  for (int i = 0; i < 3; ++i) ctx->screen_components_ms[i] = 0.0;
}

extern "C" int pg_screen_components_release(pg_ctx* ctx) {
  if (!ctx) return PG_E_ARG;
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  pg_screen_components_drop(ctx);
  return PG_OK;
}

extern "C" int pg_screen_components_last(pg_ctx* ctx, uint64_t* counts_out, double* ms_out) {
  if (!ctx || !counts_out || !ms_out) return pg_fail(ctx, PG_E_ARG, "bad argument");
  for (int i = 0; i < 4; ++i) counts_out[i] = ctx->screen_components_last[i];
  for (int i = 0; i < 3; ++i) ms_out[i] = ctx->screen_components_ms[i];
  return PG_OK;
}

extern "C" int pg_screen_components_read(pg_ctx* ctx, int32_t* root_out, uint64_t* entries_out, uint64_t* weight_out) {
  if (!ctx) return PG_E_ARG;
  ComponentsState* C = components_of(ctx);
  if (!C) return pg_fail(ctx, PG_E_ARG, "screen: no resident components (call pg_screen_components or pg_screen_index_components first)");
  if (!root_out || !entries_out || !weight_out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  PG_HIP(ctx, hipMemcpyAsync(root_out, C->d_root, (size_t)C->n * 4, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipMemcpyAsync(entries_out, C->d_entries, (size_t)C->n * 8, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipMemcpyAsync(weight_out, C->d_weight, (size_t)C->n * 8, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipStreamSynchronize(st));
  return PG_OK;
}

extern "C" int pg_screen_components(pg_ctx* ctx, const int32_t* a, const int32_t* b, const uint32_t* shared, uint64_t m, uint32_t n, uint32_t* n_components_out) {
  if (!ctx) return PG_E_ARG;
  if (n < 1 || n > pgscr::INDEX_MAX_GENOMES) return pg_fail(ctx, PG_E_ARG, "screen: components are of 1 ... 1048576 (2^20) nodes, not " + std::to_string(n));
  if (!n_components_out || (m && (!a || !b))) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  uint64_t ignored = 0;
  uint32_t outside = 0;
  for (uint64_t i = 0; i < m; ++i) {      // before anything is copied or replaced (one branch-free pass; a negative index is a large unsigned one)
    outside |= (uint32_t)((uint32_t)a[i] >= n) | (uint32_t)((uint32_t)b[i] >= n);
    ignored += a[i] == b[i] ? 1u : 0u;
  }
  for (uint64_t i = 0; outside && i < m; ++i)
    if ((uint32_t)a[i] >= n || (uint32_t)b[i] >= n)
      return pg_fail(ctx, PG_E_ARG, "screen: entry " + std::to_string(i) + " names node " + std::to_string((uint32_t)a[i] >= n ? a[i] : b[i]) + " outside [0, " +
                                        std::to_string(n) + ")");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  uint64_t chunk = COMPONENTS_CHUNK;
  if (const char* x = pg_dev_env("PYANI_COMPONENTS_CHUNK")) { const long long c = atoll(x); if (c >= 1) chunk = (uint64_t)c; }      // (tests: several chunks of a small list)
  chunk = std::min<uint64_t>(chunk, std::max<uint64_t>(m, 1));
  std::unique_ptr<ComponentsState> C(new ComponentsState());
  PgDevBuf<int32_t> d_a, d_b;
  PgDevBuf<uint32_t> d_s;
  int rc;
  if ((rc = components_alloc(ctx, n, *C)) || (rc = pg_dev_alloc(ctx, "screen", d_a, (size_t)chunk, "a chunk of the entries")) ||
      (rc = pg_dev_alloc(ctx, "screen", d_b, (size_t)chunk, "a chunk of the entries")) ||
      (shared && (rc = pg_dev_alloc(ctx, "screen", d_s, (size_t)chunk, "a chunk of the entries"))))
    return rc;
  ScreenEvents T;
  for (uint64_t at = 0; at < m; at += chunk) {
    const uint64_t c = std::min(chunk, m - at);
    PG_HIP(ctx, hipMemcpyAsync(d_a, a + at, (size_t)c * 4, hipMemcpyHostToDevice, st));
    PG_HIP(ctx, hipMemcpyAsync(d_b, b + at, (size_t)c * 4, hipMemcpyHostToDevice, st));
    if (shared) PG_HIP(ctx, hipMemcpyAsync(d_s, shared + at, (size_t)c * 4, hipMemcpyHostToDevice, st));
    T.begin(1, st);
    rc = components_hook(ctx, *C, d_a.p, d_b.p, shared ? d_s.p : nullptr, c);
    T.end(st);
    if (rc) return rc;
  }
  rc = components_finish(ctx, C, T, m - ignored, ignored, n_components_out);      // (its synchronisation comes before the chunk buffers go)
  if (rc) (void)hipStreamSynchronize(st);
  return rc;
}

extern "C" int pg_screen_index_components(pg_ctx* ctx, const uint32_t* need, uint32_t n, uint32_t band_first, uint32_t band_step, uint32_t* n_components_out,
                                          uint64_t* n_pairs_out) {
  if (!ctx) return PG_E_ARG;
  IndexState* I = index_of(ctx);
  if (!I) return pg_fail(ctx, PG_E_ARG, "screen: no resident index (call pg_screen_index first)");
  if (n != I->n) return pg_fail(ctx, PG_E_ARG, "screen: the resident index is of " + std::to_string(I->n) + " genomes, not " + std::to_string(n));
  if (band_step < 1) return pg_fail(ctx, PG_E_ARG, "screen: band_step must be 1 or more");
  if (!need || !n_components_out || !n_pairs_out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const uint32_t rows = rows_for(ctx, n), n_bands = pgscr::band_count(n, rows);
  const uint32_t tpr = (n + SEL_CELLS - 1) / SEL_CELLS;
  std::unique_ptr<ComponentsState> C(new ComponentsState());
  int rc;
  if ((rc = components_alloc(ctx, n, *C))) return rc;
  uint64_t incr = 0, kept = 0;
  ScreenEvents T;
  if (band_first < n_bands) {
    BandWork W;
    if ((rc = band_alloc(ctx, I, std::min(rows, n), true, W))) return rc;
    PG_HIP(ctx, hipMemcpyAsync(W.need, need, (size_t)n * 4, hipMemcpyHostToDevice, st));
    for (uint64_t band = band_first; band < n_bands; band += band_step) {
      uint32_t r0, r1;
      pgscr::band_range((uint32_t)band, rows, n, &r0, &r1);
      unsigned long long total = 0;
      if ((rc = band_select(ctx, I, r0, r1, tpr, W, T, 0, 0, &incr, &total))) { (void)hipStreamSynchronize(st); return rc; }
      T.end(st);
      // the band's triples stay where the selection left them: hooked and accumulated there, before the next band overwrites them (one stream)
      T.begin(1, st);
      rc = components_hook(ctx, *C, W.a.p, W.b.p, W.s.p, total);
      T.end(st);
      if (rc) { (void)hipStreamSynchronize(st); return rc; }
      kept += total;
    }
    PG_HIP(ctx, hipStreamSynchronize(st));      // (W goes with this scope)
  }
  if ((rc = components_finish(ctx, C, T, kept, 0, n_components_out))) { (void)hipStreamSynchronize(st); return rc; }
  *n_pairs_out = kept;
  return PG_OK;
}
