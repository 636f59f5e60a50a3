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
#include <algorithm>
#include <hipcub/hipcub.hpp>
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
  void sum(double* ms3) {
    ms3[0] = ms3[1] = ms3[2] = 0.0;
    if (!ok) return;
    for (size_t i = 0; i < stage.size() && 2 * i + 1 < ev.size(); ++i) {
      float x = 0.f;
      if (hipEventElapsedTime(&x, ev[2 * i], ev[2 * i + 1]) == hipSuccess) ms3[stage[i]] += (double)x; else (void)hipGetLastError();
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
                 bool want_shared, const uint32_t* shared_out) {
  if (n > pgscr::MAX_GENOMES) return pg_fail(ctx, PG_E_ARG, "screen: more than 8192 genomes in one call");      // (before the ids are read)
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
  PgDevBuf<uint32_t> d_sizes;
  if ((rc = sk_malloc(ctx, d_tab, n)) || (rc = sk_malloc(ctx, d_hist, pgscr::N_BINS)) || (rc = sk_malloc(ctx, d_counters, 4)) ||
      (rc = sk_malloc(ctx, d_sizes, n)) || (rc = sk_malloc(ctx, d_shared, (size_t)n * n)))
    return rc;
  PG_HIP(ctx, hipMemcpyAsync(d_tab, tab.data(), (size_t)n * sizeof(ScreenGenome), hipMemcpyHostToDevice, st));
  PG_HIP(ctx, hipMemsetAsync(d_hist, 0, pgscr::N_BINS * 8, st));
  PG_HIP(ctx, hipMemsetAsync(d_sizes, 0, (size_t)n * 4, st));
  PG_HIP(ctx, hipMemsetAsync(d_shared, 0, (size_t)n * n * 4, st));
  ScreenEvents T;
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
  uint64_t n_distinct = 0, n_groups = 0, n_incr = 0;
  if (!slices.empty()) {
    PgDevBuf<unsigned long long> keys_a, keys_b, wts, off;
    PgDevBuf<uint32_t> first, last;
    PgDevBuf<uint8_t> flags, tmp;
    const size_t max_groups = (size_t)(slice_max / 2 + 2);
    if ((rc = sk_malloc(ctx, keys_a, (size_t)slice_max + 1)) || (rc = sk_malloc(ctx, keys_b, (size_t)slice_max + 1)) ||
        (rc = sk_malloc(ctx, flags, (size_t)slice_max + 1)) || (rc = sk_malloc(ctx, first, max_groups)) || (rc = sk_malloc(ctx, last, max_groups)) ||
        (rc = sk_malloc(ctx, wts, max_groups)) || (rc = sk_malloc(ctx, off, max_groups)))
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
    PG_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, need, wts.p, off.p, (int64_t)max_groups, st));
    tmp_bytes = std::max(tmp_bytes, need);
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
      n_distinct += nu;
      hipLaunchKernelGGL(screen_head_kernel, dim3(grid_for(nu, 256 * 16, cu_blocks)), dim3(256), 0, st, (const unsigned long long*)keys_a.p, nu, n, d_sizes.p,
                         flags.p);
      PG_HIP(ctx, hipGetLastError());
      tb = tmp_bytes;
      PG_HIP(ctx, hipcub::DeviceSelect::Flagged((void*)tmp.p, tb, counting, is_first, first.p, d_ng, (int64_t)nu, st));
      tb = tmp_bytes;
      PG_HIP(ctx, hipcub::DeviceSelect::Flagged((void*)tmp.p, tb, counting, is_last, last.p, d_ng, (int64_t)nu, st));
      PG_HIP(ctx, hipMemcpyAsync(&cnt[2], d_ng, 8, hipMemcpyDeviceToHost, st));
      PG_HIP(ctx, hipStreamSynchronize(st));
      const uint64_t ng = cnt[2];
      if (ng + 1 > max_groups) return pg_fail(ctx, PG_E_INTERNAL, "screen: more groups than half the keys");
      unsigned long long P = 0;
      if (ng) {
        hipLaunchKernelGGL(screen_weight_kernel, dim3(grid_for(ng + 1, 256, cu_blocks)), dim3(256), 0, st, (const uint32_t*)first.p, (const uint32_t*)last.p,
                           (uint32_t)ng, wts.p);
        PG_HIP(ctx, hipGetLastError());
        tb = tmp_bytes;
        PG_HIP(ctx, hipcub::DeviceScan::ExclusiveSum((void*)tmp.p, tb, wts.p, off.p, (int64_t)(ng + 1), st));
        PG_HIP(ctx, hipMemcpyAsync(&P, off.p + ng, 8, hipMemcpyDeviceToHost, st));
      }
      T.end(st);
      PG_HIP(ctx, hipStreamSynchronize(st));
      n_groups += ng; n_incr += P;
      // count
      if (P) {
        const uint64_t n_wg = std::max<uint64_t>(1, std::min<uint64_t>((P + 2047) / 2048, (uint64_t)ctx->num_cu * 32));
        const unsigned long long per = (P + n_wg - 1) / n_wg;
        T.begin(2, st);
        hipLaunchKernelGGL(screen_count_kernel, dim3((uint32_t)((P + per - 1) / per)), dim3(256), 0, st, (const unsigned long long*)keys_a.p,
                           (const uint32_t*)first.p, (const uint32_t*)last.p, (const unsigned long long*)off.p, (uint32_t)ng, P, per, n, d_shared.p);
        T.end(st);
        PG_HIP(ctx, hipGetLastError());
      }
    }
  }
  hipLaunchKernelGGL(screen_finish_kernel, dim3(grid_for((uint64_t)n * n, 256 * 4, cu_blocks)), dim3(256), 0, st, d_shared.p, (const uint32_t*)d_sizes.p, n);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(sizes_out, d_sizes, (size_t)n * 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && shared_out) e = hipMemcpyAsync(shared_out, d_shared, (size_t)n * n * 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return pg_fail(ctx, PG_E_HIP, std::string("screen: ") + hipGetErrorString(e));
  ctx->screen_last[0] = total_keys; ctx->screen_last[1] = n_distinct; ctx->screen_last[2] = n_groups; ctx->screen_last[3] = n_incr;
  ctx->screen_last[4] = slices.size();
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
