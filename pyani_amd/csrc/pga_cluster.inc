// pga_cluster.inc — part of pg_anim.hip (included inside its anonymous namespace; not a translation unit of its own):
// A3: MUM filter, mgaps clustering, chain extraction (wave primitives, prep kernel, wave kernel).

constexpr int CHAIN_RANGES_MAX = 64;
constexpr int CHAIN_RANGE_ENTRIES = 1024;   // nominal range length (host: ranges of a unit = matches / this, 1..CHAIN_RANGES_MAX)
struct BigUnit { uint32_t u, w0, n_ranges, reserved; };   // unit, its first range work item, how many ranges
struct RangeOut { int32_t t0, n_chains, n_cm, reserved; };

struct ClusterOut {   // per-match arrays are sliced by moff[] (a chain has >= 1 match, so chains fit the same slices)
  const uint32_t* moff; // [U + 1]
  Match* cm;
  Chain* chains;
  int32_t* n_chains;    // [U]
  int32_t* order;       // chains sorted by first-match ref start
  int32_t* status;      // [P]
};

// query record of a match that starts at strand position q (only equality matters: segment label of the per-record MUM filter)
__device__ __forceinline__ int32_t unit_qrec(const UnitDesc& U, int32_t q) {
  if (U.n_rec <= 1) return 0;
  return record_of(U.rec_start, U.n_rec, U.strand ? U.len - 1 - q : q);
}

__device__ __forceinline__ int32_t from_lane_below(int32_t v, int32_t fill) {  // lane l <- lane l-1 (lane 0 <- fill)
  return __builtin_amdgcn_update_dpp(fill, v, 0x138 /*wave_shr:1*/, 0xf, 0xf, false);
}
// the same shifts for unsigned DP keys whose "nothing there" value is 0: bound_ctrl delivers it, no fill register needed
__device__ __forceinline__ uint32_t dpp_from_above0(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130 /*wave_shl:1*/, 0xf, 0xf, true);
}
__device__ __forceinline__ uint32_t dpp_from_below0(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138 /*wave_shr:1*/, 0xf, 0xf, true);
}
__device__ __forceinline__ long long wave_max64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}
// Wave-wide max / min of a 32-bit value through DPP (no LDS crossbar: a handful of cycles instead of six dependent
// ds_bpermute round trips).  Every lane gets the result.
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#define PG_DPP_MAX(ctrl, rmask) { const uint32_t t_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, rmask, 0xf, false); v = t_ > v ? t_ : v; }
  PG_DPP_MAX(0xB1, 0xf)    // quad_perm [1,0,3,2]
  PG_DPP_MAX(0x4E, 0xf)    // quad_perm [2,3,0,1]
  PG_DPP_MAX(0x141, 0xf)   // row_half_mirror
  PG_DPP_MAX(0x140, 0xf)   // row_mirror: every lane of a row holds the row's max
  PG_DPP_MAX(0x142, 0xa)   // row_bcast15 into rows 1 and 3
  PG_DPP_MAX(0x143, 0xc)   // row_bcast31 into rows 2 and 3: lane 63 holds the wave's max
#undef PG_DPP_MAX
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) { return ~wave_max_u32(~v); }

// =====================================================================================================================
// A3, wave-cooperative: one WAVE per (pair, strand) unit.  Same results as the scalar statement (pga::mum_filter +
// pga::mgaps_strand in pg_anim_core.h): stable LSD radix sorts instead of heapsorts, wave scans
// for the containment flags, a lock-free union-find, and a chain DP whose 64-deep look-back lives in the 64 lanes.
// =====================================================================================================================
__device__ __forceinline__ uint64_t lanemask_lt() { return (1ull << (threadIdx.x & 63)) - 1ull; }

// Orders this wave's LDS accesses (cross-lane read-after-write through LDS) without waiting for its outstanding global
// stores, which a __syncthreads() of a one-wave workgroup would do (s_waitcnt vmcnt(0): ~1-2 us per use).
__device__ __forceinline__ void wave_lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// Stable LSD radix sort of packed (key << 32 | val) words by `passes` 8-bit digits of the key.  Returns the buffer that
// holds the result (a or b).  One 8-byte scattered store per element and pass; a pass whose digit is the same for
// every element moves nothing; global loads are issued four 64-element rows ahead of their use.  hist: 256 words of LDS.
__device__ uint64_t* wave_radix_sort(uint64_t* a, uint64_t* b, int n, int passes, uint32_t* hist) {
  const int lane = threadIdx.x & 63;
  constexpr int U = 4;
  uint64_t *src = a, *dst = b;
  for (int pass = 0; pass < passes; ++pass) {
    const int shift = 32 + 8 * pass;
    __syncthreads();   // the previous pass's (or the caller's) global stores have landed
    for (int i = lane; i < 256; i += 64) hist[i] = 0;
    wave_lds_fence();
    for (int base = 0; base < n; base += 64 * U) {
      uint64_t kk[U];
#pragma unroll
      for (int t = 0; t < U; ++t) { const int i = base + 64 * t + lane; kk[t] = i < n ? src[i] : 0ull; }
#pragma unroll
      for (int t = 0; t < U; ++t) if (base + 64 * t + lane < n) atomicAdd(&hist[(uint32_t)(kk[t] >> shift) & 255u], 1u);
    }
    wave_lds_fence();
    uint32_t c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
    if (__any(c0 == (uint32_t)n || c1 == (uint32_t)n || c2 == (uint32_t)n || c3 == (uint32_t)n)) continue;   // constant digit
    {  // exclusive scan of the 256 bins: 4 bins per lane
      const uint32_t tot = c0 + c1 + c2 + c3;
      uint32_t incl = tot;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
      uint32_t ex = incl - tot;
      wave_lds_fence();
      hist[4 * lane] = ex; ex += c0;
      hist[4 * lane + 1] = ex; ex += c1;
      hist[4 * lane + 2] = ex; ex += c2;
      hist[4 * lane + 3] = ex;
    }
    wave_lds_fence();
    for (int base = 0; base < n; base += 64 * U) {
      uint64_t kk[U];
#pragma unroll
      for (int t = 0; t < U; ++t) { const int i = base + 64 * t + lane; kk[t] = i < n ? src[i] : 0ull; }
#pragma unroll
      for (int t = 0; t < U; ++t) {   // rows in order: the sort is stable
        const bool act = base + 64 * t + lane < n;
        const uint32_t d = (uint32_t)(kk[t] >> shift) & 255u;
        uint64_t peers = __ballot(act);
#pragma unroll
        for (int bb = 0; bb < 8; ++bb) {
          const uint64_t vote = __ballot((d >> bb) & 1u);
          peers &= ((d >> bb) & 1u) ? vote : ~vote;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & lanemask_lt());
        uint32_t pos = 0;
        if (act) pos = hist[d] + rank;
        wave_lds_fence();   // every lane has read its bin before the bin's first lane advances it
        if (act && rank == 0) hist[d] += (uint32_t)__popcll(peers);
        wave_lds_fence();
        if (act) dst[pos] = kk[t];
      }
    }
    uint64_t* tmp = src; src = dst; dst = tmp;
  }
  __syncthreads();
  return src;
}

// containment flags over elements in sorted order (segment asc, start asc, ties: longer first): flag[idx] |= 1 if an earlier
// element OF THE SAME SEGMENT reaches at least as far, or if the next element has the same segment, start and length.
// Segments: the query record of the match when `qstart` is given (the reference-interval pass: `mummer` tests query-side
// uniqueness per query sequence), one segment otherwise.  The running maximum is taken over (segment << 32 | end): a new
// segment's first key exceeds every key of the segments before it, so nothing carries across.
__device__ void wave_containment_flags(const uint64_t* order, const int32_t* start, const int32_t* len, int n, int32_t* flag,
                                       const UnitDesc& U, const int32_t* qstart) {
  const int lane = threadIdx.x & 63;
  long long carry = -1;
  for (int base = 0; base < n; base += 64) {
    const int t = base + lane;
    const bool act = t < n;
    const uint32_t idx = act ? (uint32_t)order[t] : 0u;
    const int32_t st = act ? start[idx] : 0, ln = act ? len[idx] : 0;
    const int32_t sg = act && qstart ? unit_qrec(U, qstart[idx]) : 0;
    const long long e = act ? ((long long)sg << 32) | (uint32_t)(st + ln) : -1;
    long long incl = e;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const long long v = __shfl_up(incl, o, 64); if (lane >= o && v > incl) incl = v; }
    long long excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = -1;
    const long long prevmax = excl > carry ? excl : carry;
    if (act) {
      bool f = e <= prevmax;
      if (!f && t + 1 < n) {
        const uint32_t nx = (uint32_t)order[t + 1];
        f = start[nx] == st && len[nx] == ln && (!qstart || unit_qrec(U, qstart[nx]) == sg);
      }
      if (f) flag[idx] = 1;
    }
    const long long last = __shfl(incl, 63, 64);
    if (last > carry) carry = last;
  }
}

// (single-exit loops throughout: on this hardware a divergent loop with break / continue / return inside compiles to a
// state machine of exec-mask bookkeeping that costs more than the work)
__device__ __forceinline__ int uf_find(int32_t* parent, int x) {
  // with path halving: links only ever move to an ancestor (a smaller index), so the races are benign
  int p = parent[x];
  while (p != x) {
    const int gp = parent[p];
    if (gp != p) parent[x] = gp;
    x = gp;          // == p when p is the root: the loop then ends
    p = parent[x];
  }
  return x;
}
__device__ __forceinline__ void uf_union(int32_t* parent, int a, int b) {   // larger root -> smaller root (deterministic roots)
  bool done = false;
  while (!done) {
    a = uf_find(parent, a); b = uf_find(parent, b);
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    done = a == b || atomicCAS(&parent[hi], hi, lo) == hi;
  }
}

// =====================================================================================================================
// A3a, workgroup-cooperative: the front half of the per-unit work (MUM filter, union-find, grouping by cluster) run by
// PREP_WAVES waves per unit, so that the largest unit of a launch no longer sets the launch time on one wave's latency
// chain.  Same algorithms as the wave versions above (which remain as the single-wave statement): the stable counting
// sort gives every wave a contiguous chunk and its own histogram row, offsets are the prefix over (digit, wave).
// =====================================================================================================================
constexpr int PREP_WAVES = 16, PREP_THREADS = PREP_WAVES * 64;

__device__ uint64_t* block_radix_sort(uint64_t* a, uint64_t* b, int n, int passes, uint32_t* hist /*[PREP_WAVES][256]*/,
                                      uint32_t* s_misc /*[4]*/) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int U = 4;
  const int chunk = ((n + PREP_WAVES - 1) / PREP_WAVES + 63) & ~63;   // whole rows per wave
  const int c0 = wave * chunk < n ? wave * chunk : n, c1 = c0 + chunk < n ? c0 + chunk : n;
  uint64_t *src = a, *dst = b;
  uint32_t* myh = hist + wave * 256;
  for (int pass = 0; pass < passes; ++pass) {
    const int shift = 32 + 8 * pass;
    __syncthreads();   // previous pass's (or the caller's) global stores have landed; hist free
    for (int i = tid; i < PREP_WAVES * 256; i += PREP_THREADS) hist[i] = 0;
    if (tid == 0) s_misc[0] = 0;
    __syncthreads();
    for (int base = c0; base < c1; base += 64 * U) {
      uint64_t kk[U];
#pragma unroll
      for (int t = 0; t < U; ++t) { const int i = base + 64 * t + lane; kk[t] = i < c1 ? src[i] : 0ull; }
#pragma unroll
      for (int t = 0; t < U; ++t) if (base + 64 * t + lane < c1) atomicAdd(&myh[(uint32_t)(kk[t] >> shift) & 255u], 1u);
    }
    __syncthreads();
    // digit totals, constant-digit test, exclusive prefix over (digit, wave): thread d owns digit d
    uint32_t col = 0;
    if (tid < 256) {
      for (int w = 0; w < PREP_WAVES; ++w) col += hist[w * 256 + tid];
      if (col == (uint32_t)n) s_misc[0] = 1;
    }
    __syncthreads();
    if (s_misc[0]) continue;   // every key has the same digit: nothing moves (uniform decision)
    if (wave == 0) {           // exclusive scan of the 256 totals by wave 0 (4 per lane), result into s_tot via hist row reuse
      uint32_t t0 = 0, t1 = 0, t2 = 0, t3 = 0;
      for (int w = 0; w < PREP_WAVES; ++w) {
        t0 += hist[w * 256 + 4 * lane]; t1 += hist[w * 256 + 4 * lane + 1];
        t2 += hist[w * 256 + 4 * lane + 2]; t3 += hist[w * 256 + 4 * lane + 3];
      }
      const uint32_t tot = t0 + t1 + t2 + t3;
      uint32_t incl = tot;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
      uint32_t ex = incl - tot;
      // turn every column into running offsets: hist[w][d] = base[d] + sum_{w' < w} count[w'][d]
      uint32_t basev[4] = {ex, ex + t0, ex + t0 + t1, ex + t0 + t1 + t2};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        uint32_t run = basev[k];
        for (int w = 0; w < PREP_WAVES; ++w) { const uint32_t c = hist[w * 256 + 4 * lane + k]; hist[w * 256 + 4 * lane + k] = run; run += c; }
      }
    }
    __syncthreads();
    for (int base = c0; base < c1; base += 64 * U) {
      uint64_t kk[U];
#pragma unroll
      for (int t = 0; t < U; ++t) { const int i = base + 64 * t + lane; kk[t] = i < c1 ? src[i] : 0ull; }
#pragma unroll
      for (int t = 0; t < U; ++t) {   // rows in order: the sort is stable
        const bool act = base + 64 * t + lane < c1;
        const uint32_t d = (uint32_t)(kk[t] >> shift) & 255u;
        uint64_t peers = __ballot(act);
#pragma unroll
        for (int bb = 0; bb < 8; ++bb) {
          const uint64_t vote = __ballot((d >> bb) & 1u);
          peers &= ((d >> bb) & 1u) ? vote : ~vote;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & lanemask_lt());
        uint32_t pos = 0;
        if (act) pos = myh[d] + rank;
        wave_lds_fence();
        if (act && rank == 0) myh[d] += (uint32_t)__popcll(peers);
        wave_lds_fence();
        if (act) dst[pos] = kk[t];
      }
    }
    uint64_t* tmp = src; src = dst; dst = tmp;
  }
  __syncthreads();
  return src;
}

// containment flags (see wave_containment_flags): every wave scans its chunk of the sorted order; the running maximum
// entering a chunk is the maximum of the earlier chunks' (segment << 32 | end) keys.
__device__ void block_containment_flags(const uint64_t* order, const int32_t* start, const int32_t* len, int n, int32_t* flag,
                                        long long* s_carry /*[PREP_WAVES]*/, const UnitDesc& U, const int32_t* qstart) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int chunk = ((n + PREP_WAVES - 1) / PREP_WAVES + 63) & ~63;
  const int c0 = wave * chunk < n ? wave * chunk : n, c1 = c0 + chunk < n ? c0 + chunk : n;
  long long mx = -1;
  for (int t = c0 + lane; t < c1; t += 64) {
    const uint32_t idx = (uint32_t)order[t];
    const long long e = ((long long)(qstart ? unit_qrec(U, qstart[idx]) : 0) << 32) | (uint32_t)(start[idx] + len[idx]);
    mx = e > mx ? e : mx;
  }
  mx = wave_max64(mx);
  if (lane == 0) s_carry[wave] = mx;
  __syncthreads();
  long long carry = -1;
  for (int w = 0; w < wave; ++w) carry = s_carry[w] > carry ? s_carry[w] : carry;
  for (int base = c0; base < c1; base += 64) {
    const int t = base + lane;
    const bool act = t < c1;
    const uint32_t idx = act ? (uint32_t)order[t] : 0u;
    const int32_t st = act ? start[idx] : 0, ln = act ? len[idx] : 0;
    const int32_t sg = act && qstart ? unit_qrec(U, qstart[idx]) : 0;
    const long long e = act ? ((long long)sg << 32) | (uint32_t)(st + ln) : -1;
    long long incl = e;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const long long v = __shfl_up(incl, o, 64); if (lane >= o && v > incl) incl = v; }
    long long excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = -1;
    const long long prevmax = excl > carry ? excl : carry;
    if (act) {
      bool f = e <= prevmax;
      if (!f && t + 1 < n) {
        const uint32_t nx = (uint32_t)order[t + 1];
        f = start[nx] == st && len[nx] == ln && (!qstart || unit_qrec(U, qstart[nx]) == sg);
      }
      if (f) flag[idx] = 1;
    }
    const long long last = __shfl(incl, 63, 64);
    if (last > carry) carry = last;
  }
  __syncthreads();
}

__global__ __launch_bounds__(PREP_THREADS) void anim_cluster_prep_kernel(const RefDesc* __restrict__ refs, const UnitDesc* __restrict__ units,
                                                                         Match* __restrict__ mem, const uint32_t* __restrict__ mem_count,
                                                                         int32_t* __restrict__ iscratch, ClusterOut O, int maxmatch,
                                                                         const BigUnit* __restrict__ big) {
  __shared__ uint32_t hist[PREP_WAVES * 256];
  __shared__ uint32_t s_misc[4];
  __shared__ long long s_carry[PREP_WAVES];
  __shared__ uint32_t s_cnt[PREP_WAVES];
  const uint32_t u = big[blockIdx.x].u;   // the front half of the big units only
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const UnitDesc U = units[u];
  const RefDesc R = refs[U.ref];
  const size_t off = O.moff[u];
  const uint32_t cap = O.moff[u + 1] - O.moff[u];
  uint32_t n0 = mem_count[u];
  if (n0 > cap) { if (tid == 0) atomicOr(&O.status[U.pair], 1); n0 = cap; }
  if (n0 == 0) { if (tid == 0) O.n_chains[u] = 0; return; }
  Match* m = mem + off;
  int32_t* sa = iscratch + off * 8;
  int32_t *sb = sa + cap, *sc = sa + 2 * (size_t)cap, *sd = sa + 3 * (size_t)cap, *se = sa + 4 * (size_t)cap,
          *sf = sa + 5 * (size_t)cap, *sg = sa + 6 * (size_t)cap, *sh = sa + 7 * (size_t)cap;
  uint64_t *P0 = reinterpret_cast<uint64_t*>(sa), *P1 = reinterpret_cast<uint64_t*>(sc);
  const int n_in = (int)n0;
  // ---- MUM filter (as in the wave kernel) ---------------------------------------------------------------------------
  for (int i = tid; i < n_in; i += PREP_THREADS) { const Match t = m[i]; se[i] = t.r; sf[i] = t.q; sg[i] = t.len; sh[i] = 0; }
  __syncthreads();
  const int start_passes = (R.len > U.len ? R.len : U.len) < (1 << 24) ? 3 : 4;
  const int qrec_passes = U.n_rec <= 256 ? 1 : U.n_rec <= 65536 ? 2 : U.n_rec <= (1 << 24) ? 3 : 4;
  const uint64_t* qsorted = nullptr;
  for (int side = maxmatch ? 0 : 1; side >= 0; --side) {
    const int32_t* start = side == 0 ? sf : se;
    uint64_t* r0 = P0;
    if (maxmatch) {   // --maxmatch keeps every maximal match: no uniqueness filter; mgaps' order is (query start, reference start) — By_Start2
      for (int i = tid; i < n_in; i += PREP_THREADS) P0[i] = ((uint64_t)(uint32_t)se[i] << 32) | (uint32_t)i;
      r0 = block_radix_sort(P0, P1, n_in, start_passes, hist, s_misc);
    } else {
      for (int i = tid; i < n_in; i += PREP_THREADS) {
        const uint32_t l = (uint32_t)sg[i];
        P0[i] = ((uint64_t)(0xFFFFFFu - (l > 0xFFFFFFu ? 0xFFFFFFu : l)) << 32) | (uint32_t)i;
      }
    }
    uint64_t* r1 = maxmatch ? r0 : block_radix_sort(r0, r0 == P0 ? P1 : P0, n_in, 3, hist, s_misc);      // (the length key belongs to the uniqueness filter)
    for (int i = tid; i < n_in; i += PREP_THREADS) { const uint32_t idx = (uint32_t)r1[i]; r1[i] = ((uint64_t)(uint32_t)start[idx] << 32) | idx; }
    uint64_t* r2 = block_radix_sort(r1, r1 == P0 ? P1 : P0, n_in, start_passes, hist, s_misc);
    const bool by_qrec = side == 1 && U.n_rec > 1;   // the reference-interval pass runs per query record (see mum_filter)
    if (by_qrec) {
      for (int i = tid; i < n_in; i += PREP_THREADS) { const uint32_t idx = (uint32_t)r2[i]; r2[i] = ((uint64_t)(uint32_t)unit_qrec(U, sf[idx]) << 32) | idx; }
      r2 = block_radix_sort(r2, r2 == P0 ? P1 : P0, n_in, qrec_passes, hist, s_misc);
    }
    if (!maxmatch) block_containment_flags(r2, start, sg, n_in, sh, s_carry, U, by_qrec ? sf : nullptr);
    qsorted = r2;
  }
  // survivors in q order: ordered compaction over the waves' chunks
  int n = 0;
  {
    uint32_t* keepidx = reinterpret_cast<uint32_t*>(qsorted == P0 ? P1 : P0);
    const int chunk = ((n_in + PREP_WAVES - 1) / PREP_WAVES + 63) & ~63;
    const int c0 = wave * chunk < n_in ? wave * chunk : n_in, c1 = c0 + chunk < n_in ? c0 + chunk : n_in;
    uint32_t mine = 0;
    for (int base = c0; base < c1; base += 64) {
      const int t = base + lane;
      const bool keep = t < c1 && sh[(uint32_t)qsorted[t]] == 0;
      mine += (uint32_t)__popcll(__ballot(keep));
    }
    if (lane == 0) s_cnt[wave] = mine;
    __syncthreads();
    uint32_t at = 0;
    for (int w = 0; w < PREP_WAVES; ++w) { if (w < wave) at += s_cnt[w]; n += (int)s_cnt[w]; }
    for (int base = c0; base < c1; base += 64) {
      const int t = base + lane;
      const uint32_t idx = t < c1 ? (uint32_t)qsorted[t] : 0u;
      const bool keep = t < c1 && sh[idx] == 0;
      const uint64_t bm = __ballot(keep);
      if (keep) keepidx[at + __popcll(bm & lanemask_lt())] = idx;
      at += (uint32_t)__popcll(bm);
    }
    __syncthreads();
    for (int i = tid; i < n; i += PREP_THREADS) { const uint32_t idx = keepidx[i]; m[i] = Match{se[idx], sf[idx], sg[idx], U.strand}; }
    __syncthreads();
  }
  // ---- clustering (mgaps): union-find over all threads, then grouping by root -------------------------------------------
  int32_t *rrec = sa, *qrec = sb, *parent = sc, *order = sh;
  uint64_t *Q0 = reinterpret_cast<uint64_t*>(sd), *Q1 = reinterpret_cast<uint64_t*>(sf);
  for (int i = tid; i < n; i += PREP_THREADS) {
    rrec[i] = record_of(R.rec_start, R.n_rec, m[i].r);
    const int32_t qf = U.strand ? U.len - 1 - m[i].q : m[i].q;
    qrec[i] = record_of(U.rec_start, U.n_rec, qf);
    parent[i] = i;
  }
  __threadfence_block();
  __syncthreads();
  for (int i = tid; i < n; i += PREP_THREADS) {
    const Match mi = m[i];
    const int32_t iend = mi.q + mi.len, idiag = mi.q - mi.r;
    int j = i + 1;
    int32_t sep = j < n ? m[j].q - iend : MAX_GAP + 1;
    while (sep <= MAX_GAP) {
      const Match mj = m[j];
      if (qrec[i] == qrec[j]) {   // (the reference is one joined text to mgaps: see pga::mgaps_strand)
        int32_t dd = (mj.q - mj.r) - idiag;
        if (dd < 0) dd = -dd;
        int32_t lim = (int32_t)(DIAG_FACTOR * sep);
        if (lim < DIAG_DIFF) lim = DIAG_DIFF;
        if (dd <= lim) uf_union(parent, i, j);
      }
      ++j;
      sep = j < n ? m[j].q - iend : MAX_GAP + 1;
    }
  }
  __threadfence_block();
  __syncthreads();
  for (int i = tid; i < n; i += PREP_THREADS) Q0[i] = ((uint64_t)(uint32_t)uf_find(parent, i) << 32) | (uint32_t)i;
  __syncthreads();
  const uint64_t* rs_ = block_radix_sort(Q0, Q1, n, 4, hist, s_misc);
  for (int i = tid; i < n; i += PREP_THREADS) { const uint64_t x = rs_[i]; parent[i] = (int32_t)(x >> 32); order[i] = (int32_t)(uint32_t)x; }
  if (tid == 0) O.n_chains[u] = n;   // handed to the chain kernel (which overwrites it with the chain count)
}

#ifdef PGA_DP_STATS
__device__ unsigned long long g_cl_stats[16];   // per phase: sum of cycles [0..5], max [6..11], max n_in [12]
#define CL_MARK(ph) do { const unsigned long long t_now = __builtin_readcyclecounter(); if (lane == 0) { \
    atomicAdd(&g_cl_stats[ph], t_now - t_mark); atomicMax(&g_cl_stats[6 + ph], t_now - t_mark); } t_mark = t_now; } while (0)
#else
#define CL_MARK(ph) do {} while (0)
#endif
constexpr int WALK_CHUNK = 1024;   // 4 KiB: keeps 32 one-wave workgroups per CU

// Chain extraction over the grouped list positions [g_begin, n) of one unit (n = a cluster boundary or the list's end):
// order[t] = match index, parent[t] = its root; from / adj are indexed by LIST POSITION; a cluster's live entries are kept
// contiguous in order[g0 .. g0 + live).  Chains are appended at chains[n_chains], their matches at cm[n_cm] (both counters
// are ABSOLUTE slots of the unit's slices, so a range of the list can append at its own positions — anim_chain_range_kernel).
__device__ __forceinline__ void extract_chains(const int g_begin, const int n, int& n_chains, int& n_cm, const int limit,
                                               const Match* __restrict__ m, const int32_t* __restrict__ rrec,
                                               const int32_t* __restrict__ qrec, const int32_t* parent, int32_t* order,
                                               int32_t* from, int32_t* adj, int32_t* scv, Chain* chains, Match* cm, const int strand,
                                               const int lane, int32_t* s_from) {
  // scv: one more plane of the unit's scratch, indexed by list position like from / adj: the chain score of every entry of the
  // cluster being worked on (general path), for the entries that have to look beyond the 64-entry window (pga::mgaps_strand)
  int g0 = g_begin;
  while (g0 < n) {
    // ---- fast path: clusters of at most 64 matches (nearly all of them) are handled in registers -----------------------
    // One window = the next 64 list positions, lane t <-> position g0 + t: two rounds of global latency per window
    // instead of a dozen per cluster.  A cluster that reaches the window's end is retried at the start of the next
    // window; only one that starts at lane 0 and still does not end takes the general path below.
    {
      const int posn = g0 + lane;
      const bool valid = posn < n;
      const int32_t root = valid ? parent[posn] : -1;
      const int32_t idx = valid ? order[posn] : 0;
      Match mt{0, 0, 0, 0};
      int32_t rr = 0, qq = 0;
      if (valid) { mt = m[idx]; rr = rrec[idx]; qq = qrec[idx]; }
      int c0 = 0;
      bool general = false;
      while (c0 < 64 && g0 + c0 < n) {
        const int32_t r0 = __builtin_amdgcn_readlane(root, c0);
        const uint64_t diff = __ballot(root != r0) & ~((1ull << c0) - 1ull);
        const int c1 = diff ? __ffsll((long long)diff) - 1 : 64;
        if (c1 == 64 && g0 + 64 < n) { general = c0 == 0; break; }
        uint64_t L = (c1 == 64 ? ~0ull : (1ull << c1) - 1ull) & ~((1ull << c0) - 1ull);   // live members
        while (L) {
          int32_t my_sc = NEG_INF, my_from = -1, my_adj = 0, my_tot = 0, my_cnt = 0;
          int32_t best_sc = NEG_INF, best_k = -1;
          uint64_t done = 0;
          for (uint64_t rem = L; rem; rem &= rem - 1) {
            const int k = __ffsll((long long)rem) - 1;
            const int32_t mr = __builtin_amdgcn_readlane(mt.r, k), mq = __builtin_amdgcn_readlane(mt.q, k), ml = __builtin_amdgcn_readlane(mt.len, k);
            int32_t cand = NEG_INF, ol = 0;
            if ((done >> lane) & 1ull) {
              ol = mt.r + mt.len - mr;
              if (ol < 0) ol = 0;
              const int32_t ol2 = mt.q + mt.len - mq;
              if (ol2 > ol) ol = ol2;
              int32_t dd = (mq - mr) - (mt.q - mt.r);
              if (dd < 0) dd = -dd;
              cand = my_sc + ml - (ol + dd);
            }
            // best candidate: max cand, ties -> the EARLIEST predecessor (smallest lane): mgaps scans j = 0 .. i-1 with a strict >
            // (chain scores are sums of match lengths: < 2^24; invalid candidates become key 0)
            const uint32_t key = wave_max_u32(cand > NEG_INF / 2 ? ((uint32_t)(cand + (1 << 24)) << 6) | (uint32_t)(63 - lane) : 0u);
            const int32_t bc = key ? (int32_t)(key >> 6) - (1 << 24) : NEG_INF;
            const int bl = 63 - (int)(key & 63u);
            int32_t sc_k = ml, fr_k = -1, ad_k = 0, tot_k = ml, cnt_k = 1;
            if (bc > sc_k) {
              sc_k = bc; fr_k = bl; ad_k = __builtin_amdgcn_readlane(ol, bl);
              tot_k += __builtin_amdgcn_readlane(my_tot, bl); cnt_k += __builtin_amdgcn_readlane(my_cnt, bl);
            }
            if (lane == k) { my_sc = sc_k; my_from = fr_k; my_adj = ad_k; my_tot = tot_k; my_cnt = cnt_k; }
            if (sc_k > best_sc) { best_sc = sc_k; best_k = k; }
            done |= 1ull << k;
          }
          const int32_t total = __builtin_amdgcn_readlane(my_tot, best_k), cnt = __builtin_amdgcn_readlane(my_cnt, best_k);
          const bool emit = total >= MIN_CLUSTER && n_chains < limit && n_cm + cnt <= limit;
          uint64_t M = 0;
          int32_t my_pos = -1;
          {
            int kk = best_k, pos = n_cm + cnt;
            while (kk >= 0) {
              M |= 1ull << kk;
              --pos;
              if (lane == kk) my_pos = pos;
              kk = __builtin_amdgcn_readlane(my_from, kk);
            }
          }
          if (emit) {
            if (lane == best_k) {
              Chain c;
              c.first = n_cm; c.count = cnt; c.strand = strand; c.rrec = rr; c.qrec = qq;
              chains[n_chains] = c;
            }
            if ((M >> lane) & 1ull) {
              Match t = mt;
              t.r += my_adj; t.q += my_adj; t.len -= my_adj;
              cm[my_pos] = t;
            }
            n_chains += 1; n_cm += cnt;
          }
          L &= ~M;
        }
        c0 = c1;
      }
      if (!general) { g0 += c0; continue; }
    }
    // ---- general path: a cluster of more than 64 matches ----------------------------------------------------------------
#ifdef PGA_DP_STATS
    const unsigned long long t_gen = __builtin_readcyclecounter();
#endif
    int g1 = g0 + 1;
    {  // cluster end: first position whose root differs (wave search)
      const int32_t root = parent[g0];
      for (;;) {
        const int t = g1 + lane;
        const uint64_t diff = __ballot(t >= n || parent[t] != root);
        if (diff) { g1 += __ffsll((long long)diff) - 1; break; }
        g1 += 64;
      }
    }
    int live = g1 - g0;
    while (live > 0) {
#ifdef PGA_DP_STATS
      if (lane == 0) { atomicAdd(&g_cl_stats[13], 1ull); atomicAdd(&g_cl_stats[14], (unsigned long long)live); }
#endif
      // Chain DP over the live entries order[g0 .. g0+live), 64 at a time: the entries are gathered lane-parallel (one
      // round of global latency per 64), then handed out one by one through readlane.  Lane l's window registers hold
      // the entry at position k-1-l: start, length, best score, and the matched bases / members of the best chain
      // ending there, so the winner's totals are known without walking it.
      int32_t wr = 0, wq = 0, wl = 0, wsc = NEG_INF, wtot = 0, wcnt = 0;
      int32_t best_sc = NEG_INF, best_k = -1, best_tot = 0, best_cnt = 0;
      // mgaps looks at ALL earlier entries of the cluster; the window holds the latest 64.  An entry that has left it yields at
      // most its score + this match's length (and, being earlier, wins ties): while that stays below the window's best candidate
      // the window's answer is mgaps' (always, along a collinear run: scores grow by a match length per entry); when it does not
      // (overlapping matches of tandem repeats under --maxmatch) the entries outside are scanned too, 64 per step.
      int32_t win_out = NEG_INF;      // the largest score among the entries that have left the window (uniform)
      bool far_link = false;          // some entry took a predecessor outside the window: the best chain's totals are recounted
      for (int kb = 0; kb < live; kb += 64) {
        const int kt = kb + lane;
        Match mt{0, 0, 0, 0};
        if (kt < live) mt = m[order[g0 + kt]];
        int32_t my_from = -1, my_adj = 0, my_sc = 0;
        const int kend = live - kb < 64 ? live - kb : 64;
        for (int t = 0; t < kend; ++t) {
          const int k = kb + t;
          const int32_t mr = __builtin_amdgcn_readlane(mt.r, t), mq = __builtin_amdgcn_readlane(mt.q, t),
                        ml = __builtin_amdgcn_readlane(mt.len, t);
          int32_t cand = NEG_INF, ol = 0;
          if (lane < k && wsc > NEG_INF / 2) {
            ol = wr + wl - mr;
            if (ol < 0) ol = 0;
            const int32_t ol2 = wq + wl - mq;
            if (ol2 > ol) ol = ol2;
            int32_t dd = (mq - mr) - (wq - wr);
            if (dd < 0) dd = -dd;
            cand = wsc + ml - (ol + dd);
          }
          // best candidate: max cand, ties -> the EARLIEST predecessor in the window (largest lane = largest distance)
          const uint32_t key = wave_max_u32(cand > NEG_INF / 2 ? ((uint32_t)(cand + (1 << 24)) << 6) | (uint32_t)lane : 0u);
          const int32_t bc = key ? (int32_t)(key >> 6) - (1 << 24) : NEG_INF;
          const int bl = (int)(key & 63u);
          int32_t sc_k = ml, fr_k = -1, ad_k = 0, tot_k = ml, cnt_k = 1;
          int32_t o_bc = NEG_INF, o_pos = -1, o_ol = 0;
          if (win_out > NEG_INF / 2 && win_out + ml >= bc) {      // (uniform) the entries at list positions 0 .. k - 65, in order
            __threadfence_block();
            __syncthreads();      // their scores (stored block by block below) are visible
            for (int p0 = 0; p0 < k - 64; p0 += 64) {
              const int pp = p0 + lane;
              int32_t c2 = NEG_INF, ol_o = 0;
              if (pp < k - 64) {
                const Match mj = m[order[g0 + pp]];
                ol_o = mj.r + mj.len - mr;
                if (ol_o < 0) ol_o = 0;
                const int32_t ol2 = mj.q + mj.len - mq;
                if (ol2 > ol_o) ol_o = ol2;
                int32_t dd = (mq - mr) - (mj.q - mj.r);
                if (dd < 0) dd = -dd;
                c2 = scv[g0 + pp] + ml - (ol_o + dd);
              }
              const uint32_t key2 = wave_max_u32(c2 > NEG_INF / 2 ? ((uint32_t)(c2 + (1 << 24)) << 6) | (uint32_t)(63 - lane) : 0u);
              if (key2) {
                const int32_t c = (int32_t)(key2 >> 6) - (1 << 24);
                const int l2 = 63 - (int)(key2 & 63u);
                if (c > o_bc) { o_bc = c; o_pos = p0 + l2; o_ol = __builtin_amdgcn_readlane(ol_o, l2); }      // (blocks in ascending order: the earliest best stays)
              }
            }
          }
          if (o_bc >= bc && o_bc > sc_k) {      // an entry outside the window: earlier than every window entry, so it wins ties
            sc_k = o_bc; fr_k = o_pos; ad_k = o_ol; far_link = true;      // (tot_k / cnt_k: recounted below if this chain wins)
          } else if (bc > sc_k) {
            sc_k = bc; fr_k = k - 1 - bl; ad_k = __builtin_amdgcn_readlane(ol, bl);
            tot_k += __builtin_amdgcn_readlane(wtot, bl); cnt_k += __builtin_amdgcn_readlane(wcnt, bl);
          }
          if (lane == t) { my_from = fr_k; my_adj = ad_k; my_sc = sc_k; }
          if (sc_k > best_sc) { best_sc = sc_k; best_k = k; best_tot = tot_k; best_cnt = cnt_k; }
          // the entry in lane 63 (entry k - 64) leaves the window
          if (k >= 64) { const int32_t gone = __builtin_amdgcn_readlane(wsc, 63); win_out = gone > win_out ? gone : win_out; }
          // slide the window: lane l <- lane l-1, lane 0 <- entry k
          wr = from_lane_below(wr, mr); wq = from_lane_below(wq, mq); wl = from_lane_below(wl, ml);
          wsc = from_lane_below(wsc, sc_k); wtot = from_lane_below(wtot, tot_k); wcnt = from_lane_below(wcnt, cnt_k);
        }
        if (kt < live) { from[g0 + kt] = my_from; adj[g0 + kt] = my_adj; scv[g0 + kt] = my_sc; }
      }
      if (far_link) {      // the window's riding totals do not cover links beyond it: walk the best chain once for its totals
        __threadfence_block();
        __syncthreads();
        int32_t tot = 0, cn = 0;
        for (int k = best_k; k >= 0; k = from[g0 + k]) { tot += m[order[g0 + k]].len; ++cn; }
        best_tot = tot; best_cnt = cn;
      }
      __threadfence_block();
      __syncthreads();
      const int32_t total = best_tot, cnt = best_cnt;
      const bool emit = total >= MIN_CLUSTER && n_chains < limit && n_cm + cnt <= limit;
      if (emit && lane == 0) {
        const int first_idx = order[g0 + best_k];
        Chain c;
        c.first = n_cm; c.count = cnt; c.strand = strand; c.rrec = rrec[first_idx]; c.qrec = qrec[first_idx];
        chains[n_chains] = c;
      }
      // Walk the best chain backwards (from[k] < k always) and tag its members from[k] = -3 - (slot in cm), or -2 if
      // the chain is dropped.  The pointer chase runs in LDS: from[] is staged WALK_CHUNK entries at a time, high to low.
      {
        int k = best_k, pos = n_cm + cnt;
        for (int chunk = (best_k / WALK_CHUNK) * WALK_CHUNK; chunk >= 0 && k >= 0; chunk -= WALK_CHUNK) {
          const int hi = chunk + WALK_CHUNK < live ? chunk + WALK_CHUNK : live;
          for (int t = chunk + lane; t < hi; t += 64) s_from[t - chunk] = from[g0 + t];
          __syncthreads();
          if (lane == 0) {
            while (k >= chunk) {
              const int nx = s_from[k - chunk];
              from[g0 + k] = emit ? -3 - (--pos) : -2;
              k = nx;
            }
          }
          k = __shfl(k, 0, 64); pos = __shfl(pos, 0, 64);
          __syncthreads();
        }
      }
      __threadfence_block();
      __syncthreads();
      // gather the tagged members into cm (lane-parallel) and compact the live list (drop them), preserving order
      int kept = 0;
      for (int base = 0; base < live; base += 64) {
        const int k = base + lane;
        const int32_t f = k < live ? from[g0 + k] : 0;
        const bool keep = k < live && f > -2;
        const int32_t idx = k < live ? order[g0 + k] : 0;
        if (k < live && f <= -3) {
          Match t = m[idx];
          const int32_t a = adj[g0 + k];
          t.r += a; t.q += a; t.len -= a;
          cm[-3 - f] = t;
        }
        const uint64_t bmask = __ballot(keep);
        __syncthreads();
        if (keep) order[g0 + kept + __popcll(bmask & lanemask_lt())] = idx;
        kept += (int)__popcll(bmask);
        __syncthreads();
      }
      if (emit) { n_chains += 1; n_cm += cnt; }
      live = kept;
    }
    g0 = g1;
#ifdef PGA_DP_STATS
    if (lane == 0) atomicAdd(&g_cl_stats[15], __builtin_readcyclecounter() - t_gen);
#endif
  }
}

// pga::split_chains_by_ref_record for one wave: a chain whose matches lie in more than one reference record is cut where the
// record changes (postnuc maps mgaps' joined-reference clusters back to records).  The chains' matches are contiguous in cm
// in chain order, so the new chain list is simply every position that starts a chain or follows a record change, in order.
// mark: n_cm words of scratch.  Returns the new chain count (chains[] has one slot per match: enough).
__device__ int split_chains_wave(const RefDesc& R, const UnitDesc& U, const int n_chains, Chain* chains, const Match* cm,
                                 int32_t* mark, const int lane) {
  if (R.n_rec <= 1 || n_chains == 0) return n_chains;
  __threadfence_block();
  __syncthreads();
  const Chain last = chains[n_chains - 1];
  const int n_cm = last.first + last.count;
  for (int i = lane; i < n_cm; i += 64) mark[i] = 0;
  __threadfence_block();
  __syncthreads();
  for (int c = lane; c < n_chains; c += 64) mark[chains[c].first] = 1;
  __threadfence_block();
  __syncthreads();
  int changes = 0;
  for (int base = 0; base < n_cm; base += 64) {
    const int i = base + lane;
    const bool ch = i < n_cm && i > 0 && mark[i] == 0 && record_of(R.rec_start, R.n_rec, cm[i].r) != record_of(R.rec_start, R.n_rec, cm[i - 1].r);
    if (ch) mark[i] = 1;
    changes += (int)__popcll(__ballot(ch));
  }
  if (!changes) return n_chains;
  __threadfence_block();
  __syncthreads();
  int k = 0;
  for (int base = 0; base < n_cm; base += 64) {
    const int i = base + lane;
    const bool st = i < n_cm && mark[i] != 0;
    const uint64_t bm = __ballot(st);
    if (st) {
      Chain c;
      c.first = i; c.count = 0; c.strand = U.strand;
      c.rrec = record_of(R.rec_start, R.n_rec, cm[i].r); c.qrec = unit_qrec(U, cm[i].q);
      chains[k + (int)__popcll(bm & lanemask_lt())] = c;
    }
    k += (int)__popcll(bm);
  }
  __threadfence_block();
  __syncthreads();
  int32_t nxt[1];
  for (int base = 0; base < k; base += 64) {     // counts: up to the next start (read a row before any of it is written)
    const int sidx = base + lane;
    nxt[0] = sidx + 1 < k ? chains[sidx + 1].first : n_cm;
    if (sidx < k) chains[sidx].count = nxt[0] - chains[sidx].first;
  }
  __threadfence_block();
  __syncthreads();
  return k;
}

// Chains of one unit in reference order (pga::chain_before: start of the first match, then extraction order).  Q0 / Q1: sort buffers of n_chains words each; hist: 256 words of LDS.
__device__ __forceinline__ void order_chains(const int n_chains, const Chain* chains, const Match* cm, uint64_t* Q0, uint64_t* Q1,
                                             uint32_t* hist, int32_t* co, const int lane) {
  {
    __syncthreads();
    // pga::chain_before: (reference start, query start, index) — LSD: the query starts first, then the reference starts
    for (int i = lane; i < n_chains; i += 64) Q0[i] = ((uint64_t)(uint32_t)cm[chains[i].first].q << 32) | (uint32_t)i;
    __syncthreads();
    uint64_t* cq_ = wave_radix_sort(Q0, Q1, n_chains, 4, hist);
    for (int i = lane; i < n_chains; i += 64) { const uint32_t idx = (uint32_t)cq_[i]; cq_[i] = ((uint64_t)(uint32_t)cm[chains[idx].first].r << 32) | idx; }
    __syncthreads();
    const uint64_t* cs_ = wave_radix_sort(cq_, cq_ == Q0 ? Q1 : Q0, n_chains, 4, hist);
    for (int i = lane; i < n_chains; i += 64) co[i] = (int32_t)(uint32_t)cs_[i];
    __threadfence_block();
    __syncthreads();
  }
}

__global__ __launch_bounds__(64) void anim_cluster_wave_kernel(const RefDesc* __restrict__ refs, const UnitDesc* __restrict__ units,
                                                               Match* __restrict__ mem, const uint32_t* __restrict__ mem_count,
                                                               int32_t* __restrict__ iscratch, ClusterOut O, int prepared, int maxmatch, int split_min) {
  __shared__ uint32_t hist[256];
  __shared__ int32_t s_from[WALK_CHUNK];
  const uint32_t u = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const UnitDesc U = units[u];
  const RefDesc R = refs[U.ref];
  const size_t off = O.moff[u];
  const uint32_t cap = O.moff[u + 1] - O.moff[u];
  uint32_t n0 = mem_count[u];
  if (n0 > cap) { if (lane == 0) atomicOr(&O.status[U.pair], 1); n0 = cap; }
  if (n0 == 0) { if (lane == 0) O.n_chains[u] = 0; return; }
  Match* m = mem + off;
  Match* cm = O.cm + off;
  // scratch slices (8 x cap ints): a..h; (a,b) and (c,d) double as the two packed sort buffers
  int32_t* sa = iscratch + off * 8;
  int32_t *sb = sa + cap, *sc = sa + 2 * (size_t)cap, *sd = sa + 3 * (size_t)cap, *se = sa + 4 * (size_t)cap,
          *sf = sa + 5 * (size_t)cap, *sg = sa + 6 * (size_t)cap, *sh = sa + 7 * (size_t)cap;
  uint64_t *P0 = reinterpret_cast<uint64_t*>(sa), *P1 = reinterpret_cast<uint64_t*>(sc);
  const int n_in = (int)n0;
#ifdef PGA_DP_STATS
  unsigned long long t_mark = __builtin_readcyclecounter();
  if (lane == 0) atomicMax(&g_cl_stats[12], (unsigned long long)n_in);
#endif
  int n = 0;
  int32_t *rrec = sa, *qrec = sb, *parent = sc, *from = se, *adj = sf, *order = sh;
  uint64_t *Q0 = reinterpret_cast<uint64_t*>(sd), *Q1 = reinterpret_cast<uint64_t*>(sf);   // (sd,se) and (sf,sg): sort buffers
  const bool big = (int)n0 >= split_min;   // big units: the front half only, chains by anim_chain_range_kernel + anim_chain_merge_kernel
  if (prepared && big) return;   // anim_cluster_prep_kernel has left the grouped list and its length (O.n_chains[u])
  {
  // ---- MUM filter -----------------------------------------------------------------------------------------------
  // SoA copies: se = r, sf = q, sg = len; flags in sh
  for (int i = lane; i < n_in; i += 64) { const Match t = m[i]; se[i] = t.r; sf[i] = t.q; sg[i] = t.len; sh[i] = 0; }
  __syncthreads();
  const int start_passes = (R.len > U.len ? R.len : U.len) < (1 << 24) ? 3 : 4;
  const int qrec_passes = U.n_rec <= 256 ? 1 : U.n_rec <= 65536 ? 2 : U.n_rec <= (1 << 24) ? 3 : 4;
  const uint64_t* qsorted = nullptr;
  for (int side = maxmatch ? 0 : 1; side >= 0; --side) {
    const int32_t* start = side == 0 ? sf : se;   // reference intervals first, then query intervals (whose order is reused)
    // sort by (start asc, len desc): LSD = len-desc key first, then start
    uint64_t* r0 = P0;
    if (maxmatch) {   // --maxmatch keeps every maximal match: no uniqueness filter; mgaps' order is (query start, reference start) — By_Start2
      for (int i = lane; i < n_in; i += 64) P0[i] = ((uint64_t)(uint32_t)se[i] << 32) | (uint32_t)i;
      r0 = wave_radix_sort(P0, P1, n_in, start_passes, hist);
    } else {
      for (int i = lane; i < n_in; i += 64) {
        const uint32_t l = (uint32_t)sg[i];
        P0[i] = ((uint64_t)(0xFFFFFFu - (l > 0xFFFFFFu ? 0xFFFFFFu : l)) << 32) | (uint32_t)i;
      }
    }
    uint64_t* r1 = maxmatch ? r0 : wave_radix_sort(r0, r0 == P0 ? P1 : P0, n_in, 3, hist);      // (the length key belongs to the uniqueness filter)
    for (int i = lane; i < n_in; i += 64) { const uint32_t idx = (uint32_t)r1[i]; r1[i] = ((uint64_t)(uint32_t)start[idx] << 32) | idx; }
    uint64_t* r2 = wave_radix_sort(r1, r1 == P0 ? P1 : P0, n_in, start_passes, hist);
    const bool by_qrec = side == 1 && U.n_rec > 1;   // the reference-interval pass runs per query record (see mum_filter)
    if (by_qrec) {
      for (int i = lane; i < n_in; i += 64) { const uint32_t idx = (uint32_t)r2[i]; r2[i] = ((uint64_t)(uint32_t)unit_qrec(U, sf[idx]) << 32) | idx; }
      r2 = wave_radix_sort(r2, r2 == P0 ? P1 : P0, n_in, qrec_passes, hist);
    }
    if (!maxmatch) wave_containment_flags(r2, start, sg, n_in, sh, U, by_qrec ? sf : nullptr);
    __syncthreads();
    qsorted = r2;
  }
  // survivors in q order (distinct q among survivors): the query-side order is still there -> compact
  {
    uint32_t* keepidx = reinterpret_cast<uint32_t*>(qsorted == P0 ? P1 : P0);   // the other sort buffer is free
    for (int base = 0; base < n_in; base += 64) {
      const int t = base + lane;
      const uint32_t idx = t < n_in ? (uint32_t)qsorted[t] : 0u;
      const bool keep = t < n_in && sh[idx] == 0;
      const uint64_t bm = __ballot(keep);
      if (keep) keepidx[n + __popcll(bm & lanemask_lt())] = idx;
      n += (int)__popcll(bm);
    }
    __syncthreads();
    for (int i = lane; i < n; i += 64) { const uint32_t idx = keepidx[i]; m[i] = Match{se[idx], sf[idx], sg[idx], U.strand}; }
    __syncthreads();
  }
  CL_MARK(0);
  // ---- clustering (mgaps) ------------------------------------------------------------------------------------------
  for (int i = lane; i < n; i += 64) {
    rrec[i] = record_of(R.rec_start, R.n_rec, m[i].r);
    const int32_t qf = U.strand ? U.len - 1 - m[i].q : m[i].q;
    qrec[i] = record_of(U.rec_start, U.n_rec, qf);
    parent[i] = i;
  }
  __syncthreads();
  for (int i = lane; i < n; i += 64) {
    const Match mi = m[i];
    const int32_t iend = mi.q + mi.len, idiag = mi.q - mi.r;
    int j = i + 1;
    int32_t sep = j < n ? m[j].q - iend : MAX_GAP + 1;
    while (sep <= MAX_GAP) {
      const Match mj = m[j];
      if (qrec[i] == qrec[j]) {   // (the reference is one joined text to mgaps: see pga::mgaps_strand)
        int32_t dd = (mj.q - mj.r) - idiag;
        if (dd < 0) dd = -dd;
        int32_t lim = (int32_t)(DIAG_FACTOR * sep);
        if (lim < DIAG_DIFF) lim = DIAG_DIFF;
        if (dd <= lim) uf_union(parent, i, j);
      }
      ++j;
      sep = j < n ? m[j].q - iend : MAX_GAP + 1;
    }
  }
  __threadfence_block();
  __syncthreads();
  CL_MARK(1);
  {  // group by root (stable: q order inside a cluster): radix sort of (root, index)
    for (int i = lane; i < n; i += 64) Q0[i] = ((uint64_t)(uint32_t)uf_find(parent, i) << 32) | (uint32_t)i;
    __syncthreads();
    const uint64_t* rs_ = wave_radix_sort(Q0, Q1, n, 4, hist);
    for (int i = lane; i < n; i += 64) { const uint64_t x = rs_[i]; parent[i] = (int32_t)(x >> 32); order[i] = (int32_t)(uint32_t)x; }
    __syncthreads();   // parent[] now = root id of the i-th element in grouped order
  }
  }
  CL_MARK(2);
  if (big) { if (lane == 0) O.n_chains[u] = n; return; }   // grouped list of n entries in the unit's scratch slices
  // ---- chain extraction per cluster ----------------------------------------------------------------------------------
  int n_chains = 0, n_cm = 0;
  Chain* chains = O.chains + off;
  extract_chains(0, n, n_chains, n_cm, (int)cap, m, rrec, qrec, parent, order, from, adj, sd, chains, cm, U.strand, lane, s_from);
  n_chains = split_chains_wave(R, U, n_chains, chains, cm, sa, lane);
  CL_MARK(3);
  // ---- chains in reference order + neighbours ------------------------------------------------------------------------
  order_chains(n_chains, chains, cm, Q0, Q1, hist, O.order + off, lane);
  if (lane == 0) O.n_chains[u] = n_chains;
  CL_MARK(4);
}

// ---- big units: the chains of a unit's clusters, extracted by many waves ---------------------------------------------------
// A launch takes as long as its slowest workgroup, and a unit with tens of thousands of matches spends most of its time
// walking its clusters one after the other (measured, 5 Mb pairs: 82 M cycles in the slowest unit, 71 M of them here).  The
// clusters are independent: the grouped list of a big unit (>= split_min matches) is cut at cluster boundaries into up to
// CHAIN_RANGES_MAX ranges, one wave each; a range appends its chains / chained matches at its OWN list positions (a range of
// k entries yields at most k of either), and anim_chain_merge_kernel moves them together in range order — the arrays come
// out exactly as one wave walking the whole list writes them.
// first list position >= x that starts a cluster (or n)
__device__ __forceinline__ int cluster_boundary(const int32_t* parent, int x, const int n, const int lane) {
  if (x <= 0) return 0;
  while (x < n) {
    const int t = x + lane;
    const uint64_t hit = __ballot(t >= n || parent[t] != parent[t - 1]);
    if (hit) return x + __ffsll((long long)hit) - 1;
    x += 64;
  }
  return n;
}

__global__ __launch_bounds__(64) void anim_chain_range_kernel(const UnitDesc* __restrict__ units, const Match* __restrict__ mem,
                                                              int32_t* __restrict__ iscratch, ClusterOut O,
                                                              const BigUnit* __restrict__ big, const uint2* __restrict__ ranges,
                                                              RangeOut* __restrict__ range_out) {
  __shared__ int32_t s_from[WALK_CHUNK];
  const uint32_t w = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const BigUnit B = big[ranges[w].x];
  const int r = (int)ranges[w].y, R = (int)B.n_ranges;
  const uint32_t u = B.u;
  const size_t off = O.moff[u];
  const uint32_t cap = O.moff[u + 1] - O.moff[u];
  const int n = O.n_chains[u];   // length of the grouped list (front half)
  int32_t* sa = iscratch + off * 8;
  int32_t *rrec = sa, *qrec = sa + cap, *parent = sa + 2 * (size_t)cap, *from = sa + 4 * (size_t)cap, *adj = sa + 5 * (size_t)cap,
          *order = sa + 7 * (size_t)cap;
  const int t0 = cluster_boundary(parent, (int)((long long)n * r / R), n, lane);
  const int t1 = r + 1 == R ? n : cluster_boundary(parent, (int)((long long)n * (r + 1) / R), n, lane);
  int n_chains = t0, n_cm = t0;
  if (t0 < t1)
    extract_chains(t0, t1, n_chains, n_cm, t1, mem + off, rrec, qrec, parent, order, from, adj, sa + 3 * (size_t)cap, O.chains + off, O.cm + off,
                   units[u].strand, lane, s_from);
  if (lane == 0) range_out[w] = RangeOut{t0, n_chains - t0, n_cm - t0, 0};
}

__global__ __launch_bounds__(64) void anim_chain_merge_kernel(const RefDesc* __restrict__ refs, const UnitDesc* __restrict__ units,
                                                              int32_t* __restrict__ iscratch, ClusterOut O, const BigUnit* __restrict__ big,
                                                              const RangeOut* __restrict__ range_out) {
  __shared__ uint32_t hist[256];
  const BigUnit B = big[blockIdx.x];
  const int lane = threadIdx.x & 63;
  const uint32_t u = B.u;
  const size_t off = O.moff[u];
  const uint32_t cap = O.moff[u + 1] - O.moff[u];
  Chain* chains = O.chains + off;
  Match* cm = O.cm + off;
  int NC = 0, NCM = 0;
  for (uint32_t r = 0; r < B.n_ranges; ++r) {
    const RangeOut ro = range_out[B.w0 + r];
    // moves go towards lower slots (NC <= t0, NCM <= t0) in 64-entry rows, every row read before it is written
    if (ro.t0 != NC)
      for (int base = 0; base < ro.n_chains; base += 64) {
        const int k = base + lane;
        Chain c{};
        if (k < ro.n_chains) { c = chains[ro.t0 + k]; c.first += NCM - ro.t0; }
        __syncthreads();
        if (k < ro.n_chains) chains[NC + k] = c;
      }
    if (ro.t0 != NCM)
      for (int base = 0; base < ro.n_cm; base += 64) {
        const int k = base + lane;
        Match t{};
        if (k < ro.n_cm) t = cm[ro.t0 + k];
        __syncthreads();
        if (k < ro.n_cm) cm[NCM + k] = t;
      }
    NC += ro.n_chains; NCM += ro.n_cm;
  }
  __threadfence_block();
  __syncthreads();
  int32_t* sa = iscratch + off * 8;
  uint64_t *Q0 = reinterpret_cast<uint64_t*>(sa + 3 * (size_t)cap), *Q1 = reinterpret_cast<uint64_t*>(sa + 5 * (size_t)cap);
  { const UnitDesc U = units[u]; NC = split_chains_wave(refs[U.ref], U, NC, chains, cm, sa, lane); }
  order_chains(NC, chains, cm, Q0, Q1, hist, O.order + off, lane);
  if (lane == 0) O.n_chains[u] = NC;
}
