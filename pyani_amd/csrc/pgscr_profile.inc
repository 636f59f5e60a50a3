// pgscr_profile.inc — part of pg_screen.hip: the PROFILE of a partition over the resident search index (DESIGN.md §16.13).  The index keeps
// every distinct sampled k-mer d with the ascending list of its holders H(d), h(d) = |H(d)| >= 1.  Under a partition `label` a CELL is a pair
// (d, c) with occ(d, c) = |H(d) & c| > 0; it is core (occ == size[c]), soft (occ >= core_need[c]), shell (shell_need[c] <= occ < core_need[c]),
// private (occ == h(d)) and a marker (private and soft).  The cells are counted per cluster, with the spectrum of their occupancies, and
// every (k-mer, holder) entry per genome; the marker cells are listed.  Integer atomics without a return value only, so nothing depends on
// an order of arrival; kernel boundaries are the only ordering, no thread waits for another, every store goes through vector memory.
// A cluster is named by its node c = label[v] everywhere: the ascending naming nodes ARE the ascending cluster ordinals.
//   F1 profile_off_kernel        size[v] where v names a cluster, 0 elsewhere; one exclusive scan gives off, the spectrum's rows
//   The k-mers go three ways by h(d), and all three reach ONE accounting body (profile_flags, profile_member, profile_cell):
//   F2 profile_lane_kernel       h <= lane_limit (<= 8): a thread per k-mer, its holders' clusters in registers, quadratic compare.  A run
//                                of equal cluster (and of equal spectrum word) in consecutive lanes is reduced inside the wave by the
//                                segmented shuffle of the evaluation (evaluate_segment) before ONE set of atomics from the run's head.
//   F3 profile_wave_kernel       lane_limit < h <= wave_limit (<= 64): a wave per k-mer, a holder per lane.  The first unaccounted lane's
//                                cluster is broadcast, the lanes that equal it balloted, the popcount is occ: one turn per distinct
//                                cluster, uniform over the wave, no barrier.
//   F4 profile_keys_kernel, F5 profile_head_kernel, F6 profile_first_kernel, F7 profile_entry_kernel
//                                everything larger, in batches of at most batch_keys entries cut at k-mer boundaries (a larger k-mer is a
//                                batch of its own): key = position in the batch << 40 | cluster << 20 | member, one hipcub radix sort over
//                                bits 20 ... 40 + the positions' bits; the runs of equal (k-mer, cluster) are the cells: heads marked,
//                                numbered by one inclusive scan, their first entries scattered (one writer each), and every entry
//                                accounts for itself with its run's length, the run's first entry for the cell.
//   F8 profile_marker_kernel     a private cell is its k-mer's only cell, so a k-mer has at most one marker: the tiers leave mark[d] = its
//                                cluster (one writer per d).  The listed ones are compacted in index order (a flagged selection: no cursor
//                                atomic decides a position) and sorted by cluster with ONE stable radix sort: ascending cluster, then index
//                                position — the contract's order, not an order of arrival.
namespace {

constexpr uint32_t PROFILE_LANE_MAX = 8, PROFILE_WAVE_MAX = 64, PROFILE_LANE_DEFAULT = 8, PROFILE_WAVE_DEFAULT = 64;      // (DESIGN.md §16.13 has the measured table)
constexpr uint32_t PROFILE_NONE = 0xFFFFFFFFu;
constexpr uint32_t PROFILE_POS_BITS_MAX = 24;      // k-mers of one sorted batch: 24 + 20 + 20 bits of key
constexpr uint64_t PROFILE_BATCH_MAX = 1ull << 31; // entries of one sorted batch: positions in 32 bits

struct ProfileState {      // the resident result of the latest accepted profile
  uint32_t n = 0;
  uint64_t n_markers = 0;
  PgDevBuf<uint32_t> held, core_held, private_held, alone, foreign;      // n each, per genome
  PgDevBuf<uint32_t> c_size;                                                // n each, by naming node
  PgDevBuf<unsigned long long> c_kmers, c_core, c_soft, c_shell, c_private, c_marker;
  PgDevBuf<unsigned long long> spectrum;                                    // n
  PgDevBuf<int32_t> m_cluster;                                              // n_markers each
  PgDevBuf<uint32_t> m_kmer, m_occ;
};

ProfileState* profile_of(pg_ctx* ctx) { return static_cast<ProfileState*>(ctx->screen_profile_state); }

struct ProfileView {      // what the accounting body reads and adds to
  uint32_t n, marker_min;
  const int32_t* label;
  const uint32_t *size, *core_need, *shell_need;
  const unsigned long long* off;
  uint32_t *held, *core_held, *private_held, *alone, *foreign;
  unsigned long long *c_kmers, *c_core, *c_soft, *c_shell, *c_private, *c_marker, *spectrum;
  uint32_t* mark;      // D: the cluster of k-mer d's listed marker cell, PROFILE_NONE without one
};

// The kinds of the cell (d, c) with occ of the k-mer's h holders, one byte each so that up to 64 cells add up in one word:
// byte 0 the cell itself, 1 core, 2 soft, 3 shell, 4 private, 5 marker.
__device__ __forceinline__ unsigned long long profile_flags(const ProfileView& P, uint32_t c, uint32_t occ, uint32_t h) {
  const uint32_t need = P.core_need[c];
  const bool soft = occ >= need, priv = occ == h;
  unsigned long long f = 1ull;
  if (occ == P.size[c]) f |= 1ull << 8;
  if (soft) f |= 1ull << 16;
  else if (occ >= P.shell_need[c]) f |= 1ull << 24;
  if (priv) f |= 1ull << 32;
  if (priv && soft) f |= 1ull << 40;
  return f;
}

// One (k-mer, holder) entry: v holds a k-mer whose cell in v's cluster has the kinds f.
__device__ __forceinline__ void profile_member(const ProfileView& P, uint32_t v, unsigned long long f, uint32_t occ, uint32_t h) {
  atomicAdd(P.held + v, 1u);      // no return values, here and below
  if (f & (1ull << 16)) atomicAdd(P.core_held + v, 1u);
  if (f & (1ull << 32)) atomicAdd(P.private_held + v, 1u);
  if (occ == 1u) {
    atomicAdd(P.alone + v, 1u);
    if (h > 1u) atomicAdd(P.foreign + v, 1u);
  }
}

// The summed kinds of up to 64 cells of cluster c.
__device__ __forceinline__ void profile_cell(const ProfileView& P, uint32_t c, unsigned long long sum) {
  const unsigned long long k = sum & 0xFFull, co = (sum >> 8) & 0xFFull, so = (sum >> 16) & 0xFFull, sh = (sum >> 24) & 0xFFull, pr = (sum >> 32) & 0xFFull,
                           mk = (sum >> 40) & 0xFFull;
  if (k) atomicAdd(P.c_kmers + c, k);
  if (co) atomicAdd(P.c_core + c, co);
  if (so) atomicAdd(P.c_soft + c, so);
  if (sh) atomicAdd(P.c_shell + c, sh);
  if (pr) atomicAdd(P.c_private + c, pr);
  if (mk) atomicAdd(P.c_marker + c, mk);
}

// The word of the spectrum that a cell of c with occ counts in (occ <= size[c]: below off of the next cluster).
__device__ __forceinline__ uint32_t profile_spectrum_at(const ProfileView& P, uint32_t c, uint32_t occ) {
  const unsigned long long at = P.off[c] + occ - 1u;
  return at < P.n ? (uint32_t)at : PROFILE_NONE;      // (never NONE: kept for the memory's sake)
}

// k-mer d's only cell is private: listed where it is a marker of a cluster large enough.
__device__ __forceinline__ void profile_mark(const ProfileView& P, uint32_t d, uint32_t c, unsigned long long f) {
  if ((f & (1ull << 40)) && P.size[c] >= P.marker_min) P.mark[d] = c;
}

// `val` summed over the run of equal dest in consecutive lanes (every lane of the wave calls this); true at the run's head, which holds the sum.
__device__ __forceinline__ bool profile_run_sum(uint32_t dest, uint32_t lane, unsigned long long& val) {
  bool head;
  const uint32_t run = evaluate_segment(dest, lane, head);
  for (uint32_t d = 1; d < 64u; d <<= 1) {
    const uint32_t r2 = __shfl_down(run, d, 64);
    const unsigned long long v2 = __shfl_down(val, d, 64);
    if (lane + d < 64u && r2 == run) val += v2;
  }
  return head && dest != PROFILE_NONE;
}

__global__ __launch_bounds__(256) void profile_off_kernel(uint32_t n, const int32_t* __restrict__ label, const uint32_t* __restrict__ size, unsigned long long* __restrict__ named) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) named[v] = (uint32_t)label[v] == v ? (unsigned long long)size[v] : 0ull;
}

// F2: a thread per k-mer of the WHOLE index; the ones outside 1 ... lane_limit holders are another tier's.
__global__ __launch_bounds__(256) void profile_lane_kernel(const unsigned long long* __restrict__ start, const uint32_t* __restrict__ member, uint64_t D, uint64_t E,
                                                            uint32_t lane_limit, ProfileView P) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  for (uint64_t base = wave * 64ull; base < D; base += n_waves * 64ull) {      // (uniform over the wave: every lane reaches the shuffles)
    const uint64_t d = base + lane;
    uint32_t h = 0u, cl[PROFILE_LANE_MAX], mv[PROFILE_LANE_MAX];
    if (d < D) {
      const unsigned long long s = start[d], e = start[d + 1];
      if (e > s && e - s <= lane_limit && e <= E) {
        h = (uint32_t)(e - s);
#pragma unroll
        for (uint32_t i = 0; i < PROFILE_LANE_MAX; ++i) {
          mv[i] = i < h ? member[s + i] : PROFILE_NONE;
          if (i < h && mv[i] >= P.n) h = 0u;      // (never: the build and the import checked the members; kept for the memory's sake)
        }
#pragma unroll
        for (uint32_t i = 0; i < PROFILE_LANE_MAX; ++i) cl[i] = i < h ? (uint32_t)P.label[mv[i]] : PROFILE_NONE;
      }
    }
#pragma unroll
    for (uint32_t i = 0; i < PROFILE_LANE_MAX; ++i) {
      if (!__any(i < h)) break;      // (uniform: the ballot is the wave's)
      uint32_t occ = 0u;
      bool first = i < h;
#pragma unroll
      for (uint32_t j = 0; j < PROFILE_LANE_MAX; ++j) {
        const bool same = j < h && i < h && cl[j] == cl[i];
        occ += same ? 1u : 0u;
        if (same && j < i) first = false;
      }
      unsigned long long f = 0ull;
      if (i < h) {
        f = profile_flags(P, cl[i], occ, h);
        profile_member(P, mv[i], f, occ, h);
        if (first) profile_mark(P, (uint32_t)d, cl[i], f);
      }
      unsigned long long cells = first ? f : 0ull, one = first ? 1ull : 0ull;
      const uint32_t c = first ? cl[i] : PROFILE_NONE, at = first ? profile_spectrum_at(P, cl[i], occ) : PROFILE_NONE;
      if (profile_run_sum(c, lane, cells)) profile_cell(P, c, cells);
      if (profile_run_sum(at, lane, one)) atomicAdd(P.spectrum + at, one);
    }
  }
}

// F3: a wave per k-mer of the list (h <= 64), a holder per lane.
__global__ __launch_bounds__(256) void profile_wave_kernel(const uint32_t* __restrict__ list, uint32_t n_list, const unsigned long long* __restrict__ start,
                                                            const uint32_t* __restrict__ member, uint64_t D, uint64_t E, ProfileView P) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  for (uint64_t w = wave; w < n_list; w += n_waves) {      // (uniform over the wave)
    const uint32_t d = list[w];
    if (d >= D) continue;
    const unsigned long long s = start[d], e = start[d + 1];
    if (e <= s || e - s > PROFILE_WAVE_MAX || e > E) continue;
    const uint32_t h = (uint32_t)(e - s);
    uint32_t v = PROFILE_NONE, cl = PROFILE_NONE;
    if (lane < h) {
      v = member[s + lane];
      if (v < P.n) cl = (uint32_t)P.label[v];
    }
    unsigned long long left = __ballot(cl != PROFILE_NONE);
    while (left) {      // one turn per distinct cluster among the holders
      const uint32_t at = (uint32_t)__ffsll((long long)left) - 1u;
      const uint32_t c = (uint32_t)__shfl((int)cl, (int)at, 64);
      const unsigned long long same = __ballot(cl == c);
      const uint32_t occ = (uint32_t)__popcll(same);
      const unsigned long long f = profile_flags(P, c, occ, h);
      if (cl == c) profile_member(P, v, f, occ, h);
      if (lane == at) {
        profile_cell(P, c, f);
        const uint32_t sp = profile_spectrum_at(P, c, occ);
        if (sp != PROFILE_NONE) atomicAdd(P.spectrum + sp, 1ull);
        profile_mark(P, d, c, f);
      }
      left &= ~same;
    }
  }
}

struct ProfileTier {      // the k-mers with lo < h(d) <= hi, for the selections over the index's positions
  const unsigned long long* start;
  uint32_t lo, hi;
  __host__ __device__ __forceinline__ bool operator()(uint32_t d) const {
    const unsigned long long h = start[d + 1] - start[d];
    return h > lo && h <= hi;
  }
};

struct ProfileWiden {      // a genome counter as a 64-bit term of a sum
  __host__ __device__ __forceinline__ unsigned long long operator()(uint32_t x) const { return (unsigned long long)x; }
};

struct ProfileMarked {      // the k-mers with a listed marker cell
  const uint32_t* mark;
  __host__ __device__ __forceinline__ bool operator()(uint32_t d) const { return mark[d] != PROFILE_NONE; }
};

// The holders of the large k-mers, one more word than k-mers so that the exclusive scan ends with the total.
__global__ __launch_bounds__(256) void profile_large_size_kernel(const uint32_t* __restrict__ large, uint32_t n_large, const unsigned long long* __restrict__ start,
                                                                  unsigned long long* __restrict__ wts) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= n_large; i += gridDim.x * blockDim.x) wts[i] = i < n_large ? start[large[i] + 1] - start[large[i]] : 0ull;
}

// One thread: the batch that begins at large k-mer b0 ends before b1 = the last one with koff[b1] - koff[b0] <= batch_keys, at least one
// k-mer (a k-mer larger than the batch is a batch of its own) and at most 2^24.  out[0] = b1, out[1] = its entries.
__global__ void profile_cut_kernel(const unsigned long long* __restrict__ koff, uint32_t n_large, uint32_t b0, unsigned long long batch_keys, unsigned long long* __restrict__ out) {
  if (blockIdx.x || threadIdx.x) return;
  uint32_t lo = b0 + 1u, hi = n_large;      // koff[lo] - koff[b0] may exceed the batch: then lo itself is the end
  if (hi - b0 > (1u << PROFILE_POS_BITS_MAX)) hi = b0 + (1u << PROFILE_POS_BITS_MAX);
  const unsigned long long from = koff[b0];
  while (lo < hi) {      // the last b in [lo, hi] with koff[b] - from <= batch_keys, lo when there is none
    const uint32_t mid = lo + (hi - lo + 1u) / 2u;
    if (koff[mid] - from <= batch_keys) lo = mid; else hi = mid - 1u;
  }
  out[0] = lo;
  out[1] = koff[lo] - from;
}

// F4: entry t of the batch [b0, b1): its k-mer by binary search over the offsets.
__global__ __launch_bounds__(256) void profile_keys_kernel(const uint32_t* __restrict__ large, const unsigned long long* __restrict__ koff, uint32_t b0, uint32_t b1, uint32_t nk,
                                                            const unsigned long long* __restrict__ start, const uint32_t* __restrict__ member, uint64_t E,
                                                            const int32_t* __restrict__ label, uint32_t n, unsigned long long* __restrict__ keys) {
  const unsigned long long from = koff[b0];
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < nk; t += gridDim.x * blockDim.x) {
    const unsigned long long g = from + t;
    uint32_t lo = b0, hi = b1 - 1u;      // the last k-mer with koff <= g
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo + 1u) / 2u;
      if (koff[mid] <= g) lo = mid; else hi = mid - 1u;
    }
    const unsigned long long at = start[large[lo]] + (g - koff[lo]);
    const uint32_t v = at < E ? member[at] : 0u;
    const uint32_t c = v < n ? (uint32_t)label[v] : 0u;      // (v < n: the build and the import checked; kept for the memory's sake)
    keys[t] = ((unsigned long long)(lo - b0) << 40) | ((unsigned long long)(c & 0xFFFFFu) << 20) | (unsigned long long)(v < n ? v : 0u);
  }
}

// F5: head[i] = entry i begins a run of equal (k-mer, cluster).
__global__ __launch_bounds__(256) void profile_head_kernel(const unsigned long long* __restrict__ keys, uint32_t nk, uint32_t* __restrict__ head) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nk; i += gridDim.x * blockDim.x) head[i] = i == 0u || (keys[i - 1] >> 20) != (keys[i] >> 20) ? 1u : 0u;
}

// F6: run r (numbered from 1 by the inclusive scan) begins at first[r - 1]: one writer per run.
__global__ __launch_bounds__(256) void profile_first_kernel(const uint32_t* __restrict__ head, const uint32_t* __restrict__ rid, uint32_t nk, uint32_t* __restrict__ first) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nk; i += gridDim.x * blockDim.x)
    if (head[i] && rid[i] >= 1u && rid[i] <= nk) first[rid[i] - 1u] = i;
}

// F7: every entry of the sorted batch accounts for itself, the first of a run for its cell.
__global__ __launch_bounds__(256) void profile_entry_kernel(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ rid, const uint32_t* __restrict__ first,
                                                             uint32_t nk, const uint32_t* __restrict__ large, uint32_t b0, uint32_t b1,
                                                             const unsigned long long* __restrict__ start, ProfileView P) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nk; i += gridDim.x * blockDim.x) {
    const unsigned long long key = keys[i];
    const uint32_t pos = (uint32_t)(key >> 40), c = (uint32_t)(key >> 20) & 0xFFFFFu, v = (uint32_t)key & 0xFFFFFu;
    const uint32_t r = rid[i], runs = rid[nk - 1u];
    if (r < 1u || r > runs || runs > nk || pos >= b1 - b0 || c >= P.n || v >= P.n) continue;      // (never: kept for the memory's sake)
    const uint32_t s = first[r - 1u], e = r < runs ? first[r] : nk;
    if (s > i || e <= i || e > nk) continue;
    const uint32_t occ = e - s, d = large[b0 + pos];
    const unsigned long long h64 = start[d + 1] - start[d];
    const uint32_t h = h64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)h64;
    const unsigned long long f = profile_flags(P, c, occ, h);
    profile_member(P, v, f, occ, h);
    if (i == s) {
      profile_cell(P, c, f);
      const uint32_t sp = profile_spectrum_at(P, c, occ);
      if (sp != PROFILE_NONE) atomicAdd(P.spectrum + sp, 1ull);
      profile_mark(P, d, c, f);
    }
  }
}

// F8: the listed k-mers' clusters as sort keys, and after the sort the three columns of the list.
__global__ __launch_bounds__(256) void profile_marker_key_kernel(const uint32_t* __restrict__ at, uint64_t m, const uint32_t* __restrict__ mark, uint32_t* __restrict__ key) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) key[i] = mark[at[i]];
}

__global__ __launch_bounds__(256) void profile_marker_kernel(const uint32_t* __restrict__ key, const uint32_t* __restrict__ at, uint64_t m, const uint32_t* __restrict__ kmer,
                                                              const unsigned long long* __restrict__ start, int32_t* __restrict__ m_cluster, uint32_t* __restrict__ m_kmer,
                                                              uint32_t* __restrict__ m_occ) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t d = at[i];
    m_cluster[i] = (int32_t)key[i];
    m_kmer[i] = kmer[d];
    m_occ[i] = (uint32_t)(start[d + 1] - start[d]);      // a marker cell is private: occ = h
  }
}

struct ProfileWork {      // what one call needs beside the index; released when it returns
  PgDevBuf<int32_t> label;
  PgDevBuf<uint32_t> core_need, shell_need, mark, wave_list, large, head, rid, first, m_at_out, m_key, m_key_out;
  PgDevBuf<unsigned long long> named, off, koff_w, koff, keys_in, keys_out, sel;      // sel: [0] a selection's count, [1 ... 2] a batch's cut
  PgDevBuf<uint8_t> tmp;
  size_t tmp_bytes = 0;
};

int profile_zero(pg_ctx* ctx, uint32_t n, ProfileState& R) {
  hipStream_t st = ctx->stream;
  for (PgDevBuf<uint32_t>* b : {&R.held, &R.core_held, &R.private_held, &R.alone, &R.foreign}) PG_HIP(ctx, hipMemsetAsync(b->p, 0, (size_t)n * 4, st));
  for (PgDevBuf<unsigned long long>* b : {&R.c_kmers, &R.c_core, &R.c_soft, &R.c_shell, &R.c_private, &R.c_marker, &R.spectrum}) PG_HIP(ctx, hipMemsetAsync(b->p, 0, (size_t)n * 8, st));
  return PG_OK;
}

}  // namespace

void pg_screen_profile_drop(pg_ctx* ctx) {
  if (!ctx->screen_profile_state) return;
  delete profile_of(ctx);
  ctx->screen_profile_state = nullptr;
  ctx->screen_profile_stats = PgScreenProfileStats{};
}

extern "C" int pg_screen_search_profile_release(pg_ctx* ctx) {
  if (!ctx) return PG_E_ARG;
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  pg_screen_profile_drop(ctx);
  return PG_OK;
}

extern "C" int pg_screen_search_profile_set(pg_ctx* ctx, uint32_t lane_limit, uint32_t wave_limit, uint64_t batch_keys) {
  if (!ctx) return PG_E_ARG;
  if (lane_limit > PROFILE_LANE_MAX && lane_limit != PG_SCREEN_PROFILE_DEFAULT)
    return pg_fail(ctx, PG_E_ARG, "screen: the profile's lane limit is 0 ... 8 holders (or PG_SCREEN_PROFILE_DEFAULT), not " + std::to_string(lane_limit));
  if (wave_limit > PROFILE_WAVE_MAX && wave_limit != PG_SCREEN_PROFILE_DEFAULT)
    return pg_fail(ctx, PG_E_ARG, "screen: the profile's wave limit is 0 ... 64 holders (or PG_SCREEN_PROFILE_DEFAULT), not " + std::to_string(wave_limit));
  ctx->screen_profile_lane = lane_limit;      // (PG_SCREEN_PROFILE_DEFAULT and 0 keys stay as they are: the call reads the defaults)
  ctx->screen_profile_wave = wave_limit;
  ctx->screen_profile_batch = batch_keys;
  return PG_OK;
}

extern "C" int pg_screen_search_profile_last(pg_ctx* ctx, uint64_t* counts_out, double* ms_out) {
  if (!ctx || !counts_out || !ms_out) return pg_fail(ctx, PG_E_ARG, "bad argument");
  const PgScreenProfileStats& L = ctx->screen_profile_stats;
  counts_out[0] = L.nodes; counts_out[1] = L.clusters; counts_out[2] = L.kmers; counts_out[3] = L.entries; counts_out[4] = L.cells;
  counts_out[5] = L.lane_kmers; counts_out[6] = L.wave_kmers; counts_out[7] = L.sorted_kmers; counts_out[8] = L.batches; counts_out[9] = L.markers;
  ms_out[0] = L.relabel_ms; ms_out[1] = L.lane_ms; ms_out[2] = L.wave_ms; ms_out[3] = L.sorted_ms; ms_out[4] = L.marker_ms;
  return PG_OK;
}

namespace {

// Everything after the checks; size: the host's, 0 where a node names no cluster.  The finished state is made the context's by the caller.
int profile_run(pg_ctx* ctx, const SearchState* I, const int32_t* label, const uint32_t* core_need, const uint32_t* shell_need, const std::vector<uint32_t>& size,
                uint32_t marker_min, uint64_t clusters, ProfileState& R, PgScreenProfileStats& L) {
  hipStream_t st = ctx->stream;
  const uint32_t n = I->n, cu_blocks = (uint32_t)ctx->num_cu * 8u;
  const uint64_t D = I->D, E = I->E;
  const uint32_t lane_limit = ctx->screen_profile_lane == PG_SCREEN_PROFILE_DEFAULT ? PROFILE_LANE_DEFAULT : ctx->screen_profile_lane;
  const uint32_t wave_limit = std::max(lane_limit, ctx->screen_profile_wave == PG_SCREEN_PROFILE_DEFAULT ? PROFILE_WAVE_DEFAULT : ctx->screen_profile_wave);
  const uint64_t batch_keys = std::min<uint64_t>(PROFILE_BATCH_MAX, ctx->screen_profile_batch ? ctx->screen_profile_batch
                                                                                              : (ctx->screen_max_keys ? ctx->screen_max_keys : pgscr::DEFAULT_MAX_KEYS));
  if (D > 0xFFFFFFFEull) return pg_fail(ctx, PG_E_ARG, "screen: a profile is of an index of fewer than 2^32 - 1 k-mers");
  const dim3 node_grid(grid_for(n, 256, cu_blocks));
  ProfileWork W;
  ScreenEvents T;
  int rc;
  const unsigned long long* d_start = I->d_start.p;
  const uint32_t* d_member = I->d_member.p;
  hipcub::CountingInputIterator<uint32_t> counting(0u);
  PG_HIP(ctx, tmp_room(W.tmp_bytes, [&](size_t& b) { return hipcub::DeviceScan::ExclusiveSum(nullptr, b, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (int64_t)n, st); }));
  PG_HIP(ctx, tmp_room(W.tmp_bytes, [&](size_t& b) {
    return hipcub::DeviceReduce::Sum(nullptr, b, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (int64_t)n, st); }));
  PG_HIP(ctx, tmp_room(W.tmp_bytes, [&](size_t& b) {
    return hipcub::DeviceReduce::Sum(nullptr, b, hipcub::TransformInputIterator<unsigned long long, ProfileWiden, const uint32_t*>((const uint32_t*)nullptr, ProfileWiden{}),
                                     (unsigned long long*)nullptr, (int64_t)n, st); }));
  PG_HIP(ctx, tmp_room(W.tmp_bytes, [&](size_t& b) {
    return hipcub::DeviceSelect::If(nullptr, b, counting, (uint32_t*)nullptr, (unsigned long long*)nullptr, (int64_t)D, ProfileTier{d_start, 0u, 0u}, st); }));
  PG_HIP(ctx, tmp_room(W.tmp_bytes, [&](size_t& b) {
    return hipcub::DeviceSelect::If(nullptr, b, counting, (uint32_t*)nullptr, (unsigned long long*)nullptr, (int64_t)D, ProfileMarked{nullptr}, st); }));
  if ((rc = pg_dev_alloc(ctx, "screen", R.held, n, "the profile")) || (rc = pg_dev_alloc(ctx, "screen", R.core_held, n, "the profile")) ||
      (rc = pg_dev_alloc(ctx, "screen", R.private_held, n, "the profile")) || (rc = pg_dev_alloc(ctx, "screen", R.alone, n, "the profile")) ||
      (rc = pg_dev_alloc(ctx, "screen", R.foreign, n, "the profile")) || (rc = pg_dev_alloc(ctx, "screen", R.c_size, n, "the profile's clusters")) ||
      (rc = pg_dev_alloc(ctx, "screen", R.c_kmers, n, "the profile's clusters")) || (rc = pg_dev_alloc(ctx, "screen", R.c_core, n, "the profile's clusters")) ||
      (rc = pg_dev_alloc(ctx, "screen", R.c_soft, n, "the profile's clusters")) || (rc = pg_dev_alloc(ctx, "screen", R.c_shell, n, "the profile's clusters")) ||
      (rc = pg_dev_alloc(ctx, "screen", R.c_private, n, "the profile's clusters")) || (rc = pg_dev_alloc(ctx, "screen", R.c_marker, n, "the profile's clusters")) ||
      (rc = pg_dev_alloc(ctx, "screen", R.spectrum, n, "the profile's spectrum")) || (rc = pg_dev_alloc(ctx, "screen", W.label, n, "the labels")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.core_need, n, "the thresholds")) || (rc = pg_dev_alloc(ctx, "screen", W.shell_need, n, "the thresholds")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.named, n, "the clusters' sizes")) || (rc = pg_dev_alloc(ctx, "screen", W.off, n, "the spectrum's rows")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.mark, (size_t)D, "the k-mers' marks")) || (rc = pg_dev_alloc(ctx, "screen", W.wave_list, (size_t)D, "the wave tier's k-mers")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.large, (size_t)D, "the sorted tier's k-mers")) || (rc = pg_dev_alloc(ctx, "screen", W.sel, 3, "the profile's counters")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.tmp, W.tmp_bytes + 16, "the scans' temporary storage")))
    return rc;
  R.n = n;
  if ((rc = profile_zero(ctx, n, R))) return rc;
  PG_HIP(ctx, hipMemcpyAsync(W.label, label, (size_t)n * 4, hipMemcpyHostToDevice, st));
  PG_HIP(ctx, hipMemcpyAsync(W.core_need, core_need, (size_t)n * 4, hipMemcpyHostToDevice, st));
  PG_HIP(ctx, hipMemcpyAsync(W.shell_need, shell_need, (size_t)n * 4, hipMemcpyHostToDevice, st));
  PG_HIP(ctx, hipMemcpyAsync(R.c_size, size.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
  if (D) PG_HIP(ctx, hipMemsetAsync(W.mark, 0xFF, (size_t)D * 4, st));
  {
    ScreenEvents::Stage relabel(T, ST_RELABEL, st);
    hipLaunchKernelGGL(profile_off_kernel, node_grid, dim3(256), 0, st, n, (const int32_t*)W.label.p, (const uint32_t*)R.c_size.p, W.named.p);
    PG_HIP(ctx, hipGetLastError());
    size_t tb = W.tmp_bytes;
    PG_HIP(ctx, hipcub::DeviceScan::ExclusiveSum((void*)W.tmp.p, tb, W.named.p, W.off.p, (int64_t)n, st));
  }
  const ProfileView P{n, marker_min, W.label.p, R.c_size.p, W.core_need.p, W.shell_need.p, W.off.p, R.held.p, R.core_held.p, R.private_held.p, R.alone.p, R.foreign.p,
                      R.c_kmers.p, R.c_core.p, R.c_soft.p, R.c_shell.p, R.c_private.p, R.c_marker.p, R.spectrum.p, W.mark.p};
  // the k-mers of the wave tier and of the sorted tier, in index order; the lane tier walks the whole index
  unsigned long long n_wave = 0, n_large = 0;
  if (D) {
    {
      ScreenEvents::Stage wave(T, ST_WAVE, st);
      size_t tb = W.tmp_bytes;
      PG_HIP(ctx, hipcub::DeviceSelect::If((void*)W.tmp.p, tb, counting, W.wave_list.p, W.sel.p, (int64_t)D, ProfileTier{d_start, lane_limit, wave_limit}, st));
    }
    PG_HIP(ctx, hipMemcpyAsync(&n_wave, W.sel.p, 8, hipMemcpyDeviceToHost, st));
    {
      ScreenEvents::Stage sorted(T, ST_SORTED, st);
      size_t tb = W.tmp_bytes;
      PG_HIP(ctx, hipcub::DeviceSelect::If((void*)W.tmp.p, tb, counting, W.large.p, W.sel.p, (int64_t)D, ProfileTier{d_start, wave_limit, 0xFFFFFFFFu}, st));
    }
    PG_HIP(ctx, hipMemcpyAsync(&n_large, W.sel.p, 8, hipMemcpyDeviceToHost, st));
    PG_HIP(ctx, hipStreamSynchronize(st));
    if (n_wave + n_large > D) return pg_fail(ctx, PG_E_INTERNAL, "screen: more k-mers in the profile's tiers than in the index");
  }
  if (D && lane_limit) {
    ScreenEvents::Stage lane(T, ST_LANE, st);
    hipLaunchKernelGGL(profile_lane_kernel, dim3(grid_for(D, 256, cu_blocks)), dim3(256), 0, st, d_start, d_member, D, E, lane_limit, P);
    PG_HIP(ctx, hipGetLastError());
  }
  if (n_wave) {
    ScreenEvents::Stage wave(T, ST_WAVE, st);
    hipLaunchKernelGGL(profile_wave_kernel, dim3(grid_for(n_wave, 4, cu_blocks)), dim3(256), 0, st, (const uint32_t*)W.wave_list.p, (uint32_t)n_wave, d_start, d_member, D, E, P);
    PG_HIP(ctx, hipGetLastError());
  }
  uint64_t batches = 0;
  if (n_large) {
    const uint32_t NL = (uint32_t)n_large;
    unsigned long long total = 0;
    if ((rc = pg_dev_alloc(ctx, "screen", W.koff_w, (size_t)NL + 1, "the sorted tier's offsets")) || (rc = pg_dev_alloc(ctx, "screen", W.koff, (size_t)NL + 1, "the sorted tier's offsets")))
      return rc;
    {
      size_t need = 0;
      PG_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, need, W.koff_w.p, W.koff.p, (int64_t)NL + 1, st));
      if (need > W.tmp_bytes) { W.tmp.release(); W.tmp_bytes = need; if ((rc = pg_dev_alloc(ctx, "screen", W.tmp, W.tmp_bytes + 16, "the scans' temporary storage"))) return rc; }
    }
    {
      ScreenEvents::Stage sorted(T, ST_SORTED, st);
      hipLaunchKernelGGL(profile_large_size_kernel, dim3(grid_for((uint64_t)NL + 1, 256, cu_blocks)), dim3(256), 0, st, (const uint32_t*)W.large.p, NL, d_start, W.koff_w.p);
      PG_HIP(ctx, hipGetLastError());
      size_t tb = W.tmp_bytes;
      PG_HIP(ctx, hipcub::DeviceScan::ExclusiveSum((void*)W.tmp.p, tb, W.koff_w.p, W.koff.p, (int64_t)NL + 1, st));
    }
    PG_HIP(ctx, hipMemcpyAsync(&total, W.koff.p + NL, 8, hipMemcpyDeviceToHost, st));
    PG_HIP(ctx, hipStreamSynchronize(st));
    if (total < n_large || total > E) return pg_fail(ctx, PG_E_INTERNAL, "screen: the sorted tier's k-mers hold " + std::to_string(total) + " of " + std::to_string(E) + " entries");
    // a batch holds at most batch_keys entries, or one k-mer's (at most n)
    const size_t cap = (size_t)std::min<uint64_t>(total, std::max<uint64_t>(batch_keys, n));
    size_t sort_bytes = 0;
    PG_HIP(ctx, tmp_room(sort_bytes, [&](size_t& b) {
      return hipcub::DeviceRadixSort::SortKeys(nullptr, b, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (int64_t)cap, 20, 64, st); }));
    PG_HIP(ctx, tmp_room(sort_bytes, [&](size_t& b) { return hipcub::DeviceScan::InclusiveSum(nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr, (int64_t)cap, st); }));
    if (sort_bytes > W.tmp_bytes) { W.tmp.release(); W.tmp_bytes = sort_bytes; if ((rc = pg_dev_alloc(ctx, "screen", W.tmp, W.tmp_bytes + 16, "the sort's temporary storage"))) return rc; }
    if ((rc = pg_dev_alloc(ctx, "screen", W.keys_in, cap, "the sorted tier's keys")) || (rc = pg_dev_alloc(ctx, "screen", W.keys_out, cap, "the sorted tier's keys")) ||
        (rc = pg_dev_alloc(ctx, "screen", W.head, cap, "the sorted tier's runs")) || (rc = pg_dev_alloc(ctx, "screen", W.rid, cap, "the sorted tier's runs")) ||
        (rc = pg_dev_alloc(ctx, "screen", W.first, cap, "the sorted tier's runs")))
      return rc;
    uint32_t b0 = 0;
    while (b0 < NL) {
      unsigned long long cut[2] = {0, 0};
      hipLaunchKernelGGL(profile_cut_kernel, dim3(1), dim3(64), 0, st, (const unsigned long long*)W.koff.p, NL, b0, (unsigned long long)batch_keys, W.sel.p + 1);
      PG_HIP(ctx, hipGetLastError());
      PG_HIP(ctx, hipMemcpyAsync(cut, W.sel.p + 1, 16, hipMemcpyDeviceToHost, st));
      PG_HIP(ctx, hipStreamSynchronize(st));
      const uint32_t b1 = (uint32_t)cut[0];
      if (cut[0] <= b0 || cut[0] > NL || cut[1] < 1 || cut[1] > cap) return pg_fail(ctx, PG_E_INTERNAL, "screen: a sorted batch of " + std::to_string(cut[1]) + " entries");
      const uint32_t nk = (uint32_t)cut[1];
      int pos_bits = 1;
      while ((1ull << pos_bits) < (uint64_t)(b1 - b0)) ++pos_bits;
      const dim3 key_grid(grid_for(nk, 256 * 4, cu_blocks));
      ScreenEvents::Stage sorted(T, ST_SORTED, st);
      hipLaunchKernelGGL(profile_keys_kernel, key_grid, dim3(256), 0, st, (const uint32_t*)W.large.p, (const unsigned long long*)W.koff.p, b0, b1, nk, d_start, d_member, E,
                         (const int32_t*)W.label.p, n, W.keys_in.p);
      PG_HIP(ctx, hipGetLastError());
      size_t tb = W.tmp_bytes;
      PG_HIP(ctx, hipcub::DeviceRadixSort::SortKeys((void*)W.tmp.p, tb, (const unsigned long long*)W.keys_in.p, W.keys_out.p, (int64_t)nk, 20, 40 + pos_bits, st));
      hipLaunchKernelGGL(profile_head_kernel, key_grid, dim3(256), 0, st, (const unsigned long long*)W.keys_out.p, nk, W.head.p);
      PG_HIP(ctx, hipGetLastError());
      tb = W.tmp_bytes;
      PG_HIP(ctx, hipcub::DeviceScan::InclusiveSum((void*)W.tmp.p, tb, W.head.p, W.rid.p, (int64_t)nk, st));
      hipLaunchKernelGGL(profile_first_kernel, key_grid, dim3(256), 0, st, (const uint32_t*)W.head.p, (const uint32_t*)W.rid.p, nk, W.first.p);
      PG_HIP(ctx, hipGetLastError());
      hipLaunchKernelGGL(profile_entry_kernel, key_grid, dim3(256), 0, st, (const unsigned long long*)W.keys_out.p, (const uint32_t*)W.rid.p, (const uint32_t*)W.first.p, nk,
                         (const uint32_t*)W.large.p, b0, b1, d_start, P);
      PG_HIP(ctx, hipGetLastError());
      b0 = b1;
      ++batches;
    }
  }
  // the list: the marked k-mers in index order, then one stable sort by cluster
  unsigned long long n_markers = 0;
  if (D) {
    {
      ScreenEvents::Stage markers(T, ST_MARKERS, st);
      // (the wave tier's list is dead: the marked positions take its place)
      size_t tb = W.tmp_bytes;
      PG_HIP(ctx, hipcub::DeviceSelect::If((void*)W.tmp.p, tb, counting, W.wave_list.p, W.sel.p, (int64_t)D, ProfileMarked{W.mark.p}, st));
    }
    PG_HIP(ctx, hipMemcpyAsync(&n_markers, W.sel.p, 8, hipMemcpyDeviceToHost, st));
    PG_HIP(ctx, hipStreamSynchronize(st));
    if (n_markers > D) return pg_fail(ctx, PG_E_INTERNAL, "screen: more markers than k-mers");
  }
  if (n_markers) {
    const size_t m = (size_t)n_markers;
    size_t sort_bytes = 0;
    PG_HIP(ctx, tmp_room(sort_bytes, [&](size_t& b) {
      return hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int64_t)m, 0, 20, st); }));
    if (sort_bytes > W.tmp_bytes) { W.tmp.release(); W.tmp_bytes = sort_bytes; if ((rc = pg_dev_alloc(ctx, "screen", W.tmp, W.tmp_bytes + 16, "the sort's temporary storage"))) return rc; }
    if ((rc = pg_dev_alloc(ctx, "screen", W.m_key, m, "the markers")) || (rc = pg_dev_alloc(ctx, "screen", W.m_key_out, m, "the markers")) ||
        (rc = pg_dev_alloc(ctx, "screen", W.m_at_out, m, "the markers")) || (rc = pg_dev_alloc(ctx, "screen", R.m_cluster, m, "the markers")) ||
        (rc = pg_dev_alloc(ctx, "screen", R.m_kmer, m, "the markers")) || (rc = pg_dev_alloc(ctx, "screen", R.m_occ, m, "the markers")))
      return rc;
    ScreenEvents::Stage markers(T, ST_MARKERS, st);
    const dim3 m_grid(grid_for(m, 256, cu_blocks));
    hipLaunchKernelGGL(profile_marker_key_kernel, m_grid, dim3(256), 0, st, (const uint32_t*)W.wave_list.p, (uint64_t)m, (const uint32_t*)W.mark.p, W.m_key.p);
    PG_HIP(ctx, hipGetLastError());
    size_t tb = W.tmp_bytes;
    PG_HIP(ctx, hipcub::DeviceRadixSort::SortPairs((void*)W.tmp.p, tb, (const uint32_t*)W.m_key.p, W.m_key_out.p, (const uint32_t*)W.wave_list.p, W.m_at_out.p, (int64_t)m, 0, 20, st));
    hipLaunchKernelGGL(profile_marker_kernel, m_grid, dim3(256), 0, st, (const uint32_t*)W.m_key_out.p, (const uint32_t*)W.m_at_out.p, (uint64_t)m, (const uint32_t*)I->d_kmer.p,
                       d_start, R.m_cluster.p, R.m_kmer.p, R.m_occ.p);
    PG_HIP(ctx, hipGetLastError());
  }
  R.n_markers = n_markers;
  // the cells, and the entries once more from the genomes' side: every entry was accounted for exactly once
  // (two device sums, two words read back; the batches' cut words are dead and receive them)
  unsigned long long sums[2] = {0, 0};
  {
    hipcub::TransformInputIterator<unsigned long long, ProfileWiden, const uint32_t*> held64((const uint32_t*)R.held.p, ProfileWiden{});
    size_t tb = W.tmp_bytes;
    PG_HIP(ctx, hipcub::DeviceReduce::Sum((void*)W.tmp.p, tb, (const unsigned long long*)R.c_kmers.p, W.sel.p + 1, (int64_t)n, st));
    tb = W.tmp_bytes;
    PG_HIP(ctx, hipcub::DeviceReduce::Sum((void*)W.tmp.p, tb, held64, W.sel.p + 2, (int64_t)n, st));
  }
  PG_HIP(ctx, hipMemcpyAsync(sums, W.sel.p + 1, 16, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipStreamSynchronize(st));
  const uint64_t n_cells = sums[0], n_held = sums[1];
  if (n_held != E) return pg_fail(ctx, PG_E_INTERNAL, "screen: the profile accounted for " + std::to_string(n_held) + " of the index's " + std::to_string(E) + " entries");
  L = PgScreenProfileStats{};
  L.nodes = n; L.clusters = clusters; L.kmers = D; L.entries = E; L.cells = n_cells;
  L.lane_kmers = D - n_wave - n_large; L.wave_kmers = n_wave; L.sorted_kmers = n_large; L.batches = batches; L.markers = n_markers;
  L.relabel_ms = T.ms(ST_RELABEL); L.lane_ms = T.ms(ST_LANE); L.wave_ms = T.ms(ST_WAVE); L.sorted_ms = T.ms(ST_SORTED); L.marker_ms = T.ms(ST_MARKERS);
  return PG_OK;
}

}  // namespace

extern "C" int pg_screen_search_profile(pg_ctx* ctx, const int32_t* label, const uint32_t* core_need, const uint32_t* shell_need, uint32_t n, uint32_t marker_min_size,
                                        uint64_t* n_markers_out) {
  if (!ctx) return PG_E_ARG;
  const SearchState* I = search_of(ctx);
  if (!I) return pg_fail(ctx, PG_E_ARG, "screen: no resident search index (call pg_screen_search_index first)");
  static_assert(pgscr::INDEX_MAX_GENOMES == 1u << 20, "the sorted tier's keys and the marker sort hold a cluster and a member in 20 bits each");
  if (n < 1 || n > pgscr::INDEX_MAX_GENOMES) return pg_fail(ctx, PG_E_ARG, "screen: a profile is of 1 ... 1048576 (2^20) genomes, not " + std::to_string(n));
  if (n != I->n) return pg_fail(ctx, PG_E_ARG, "screen: the resident search index is of " + std::to_string(I->n) + " genomes, not " + std::to_string(n));
  if (!label) return pg_fail(ctx, PG_E_ARG, "screen: the profile needs a label for every genome");
  if (!core_need || !shell_need) return pg_fail(ctx, PG_E_ARG, "screen: the profile needs both thresholds for every genome");
  if (marker_min_size < 1) return pg_fail(ctx, PG_E_ARG, "screen: the smallest cluster whose markers are listed has 1 member or more, not 0");
  std::vector<uint32_t> size(n, 0u);
  for (uint32_t v = 0; v < n; ++v) {      // before anything is copied or replaced
    const uint32_t c = (uint32_t)label[v];
    if (c >= n) return pg_fail(ctx, PG_E_ARG, "screen: node " + std::to_string(v) + " has the label " + std::to_string(label[v]) + " outside [0, " + std::to_string(n) + ")");
    if ((uint32_t)label[c] != c)
      return pg_fail(ctx, PG_E_ARG, "screen: node " + std::to_string(v) + " has the label " + std::to_string(c) + ", which does not name itself (label[label[v]] == label[v])");
    ++size[c];
  }
  uint64_t clusters = 0;
  for (uint32_t c = 0; c < n; ++c) {
    if (!size[c]) continue;
    ++clusters;
    if (shell_need[c] < 1 || shell_need[c] > core_need[c] || core_need[c] > size[c])
      return pg_fail(ctx, PG_E_ARG, "screen: node " + std::to_string(c) + " names a cluster of " + std::to_string(size[c]) + " with the thresholds " + std::to_string(shell_need[c]) +
                                        " and " + std::to_string(core_need[c]) + " (1 <= shell_need <= core_need <= size)");
  }
  PG_HIP(ctx, hipSetDevice(ctx->device));
  std::unique_ptr<ProfileState> R(new ProfileState());
  PgScreenProfileStats L;
  const int rc = profile_run(ctx, I, label, core_need, shell_need, size, marker_min_size, clusters, *R, L);
  if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }      // (a queued copy may still read the caller's arrays; the earlier result stays)
  pg_screen_profile_drop(ctx);
  ctx->screen_profile_stats = L;
  if (n_markers_out) *n_markers_out = R->n_markers;
  ctx->screen_profile_state = R.release();
  return PG_OK;
}

namespace {
template <typename T, typename D>
int profile_copy(pg_ctx* ctx, T* out, const PgDevBuf<D>& src, uint64_t n) {
  static_assert(sizeof(T) == sizeof(D), "the same words on both sides");
  if (out && n) PG_HIP(ctx, hipMemcpyAsync(out, src.p, (size_t)n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
  return PG_OK;
}
const char* const PROFILE_ABSENT = "screen: no resident profile (call pg_screen_search_profile first)";
}  // namespace

extern "C" int pg_screen_search_profile_read(pg_ctx* ctx, uint32_t* held_out, uint32_t* core_held_out, uint32_t* private_held_out, uint32_t* alone_out, uint32_t* foreign_out) {
  if (!ctx) return PG_E_ARG;
  ProfileState* R = profile_of(ctx);
  if (!R) return pg_fail(ctx, PG_E_ARG, PROFILE_ABSENT);
  PG_HIP(ctx, hipSetDevice(ctx->device));
  int rc;
  if ((rc = profile_copy(ctx, held_out, R->held, R->n)) || (rc = profile_copy(ctx, core_held_out, R->core_held, R->n)) ||
      (rc = profile_copy(ctx, private_held_out, R->private_held, R->n)) || (rc = profile_copy(ctx, alone_out, R->alone, R->n)) ||
      (rc = profile_copy(ctx, foreign_out, R->foreign, R->n))) {
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
  }
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PG_OK;
}

extern "C" int pg_screen_search_profile_read_clusters(pg_ctx* ctx, uint32_t* size_out, uint64_t* kmers_out, uint64_t* core_out, uint64_t* soft_out, uint64_t* shell_out,
                                                      uint64_t* private_out, uint64_t* marker_out) {
  if (!ctx) return PG_E_ARG;
  ProfileState* R = profile_of(ctx);
  if (!R) return pg_fail(ctx, PG_E_ARG, PROFILE_ABSENT);
  PG_HIP(ctx, hipSetDevice(ctx->device));
  int rc;
  if ((rc = profile_copy(ctx, size_out, R->c_size, R->n)) || (rc = profile_copy(ctx, kmers_out, R->c_kmers, R->n)) || (rc = profile_copy(ctx, core_out, R->c_core, R->n)) ||
      (rc = profile_copy(ctx, soft_out, R->c_soft, R->n)) || (rc = profile_copy(ctx, shell_out, R->c_shell, R->n)) ||
      (rc = profile_copy(ctx, private_out, R->c_private, R->n)) || (rc = profile_copy(ctx, marker_out, R->c_marker, R->n))) {
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
  }
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PG_OK;
}

extern "C" int pg_screen_search_profile_read_spectrum(pg_ctx* ctx, uint64_t* spectrum_out) {
  if (!ctx) return PG_E_ARG;
  ProfileState* R = profile_of(ctx);
  if (!R) return pg_fail(ctx, PG_E_ARG, PROFILE_ABSENT);
  PG_HIP(ctx, hipSetDevice(ctx->device));
  const int rc = profile_copy(ctx, spectrum_out, R->spectrum, R->n);
  if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PG_OK;
}

extern "C" int pg_screen_search_profile_read_markers(pg_ctx* ctx, int32_t* cluster_out, uint32_t* kmer_out, uint32_t* occ_out) {
  if (!ctx) return PG_E_ARG;
  ProfileState* R = profile_of(ctx);
  if (!R) return pg_fail(ctx, PG_E_ARG, PROFILE_ABSENT);
  PG_HIP(ctx, hipSetDevice(ctx->device));
  int rc;
  if ((rc = profile_copy(ctx, cluster_out, R->m_cluster, R->n_markers)) || (rc = profile_copy(ctx, kmer_out, R->m_kmer, R->n_markers)) ||
      (rc = profile_copy(ctx, occ_out, R->m_occ, R->n_markers))) {
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
  }
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PG_OK;
}
