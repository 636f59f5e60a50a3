// pga_postnuc.inc — part of pg_anim.hip (included inside its anonymous namespace; not a translation unit of its own):
// A4x, the extension stage as MUMmer's postnuc defines it (pg_nucmer_core.h), one WAVE per (pair, query strand) unit.
//
// The policy code (pgn::postnuc_unit: extendClusters with its target / shadow / fusion rules) is the shared scalar code, run
// redundantly by the 64 lanes of the unit's wave; the alignment engine underneath it is wave-cooperative: the lanes are the
// CELLS of the current anti-diagonal (cell j of anti-diagonal Dct is (i = Dct - j, j), lane = (j - lo) mod 64, as many chunks
// of 64 as the band is wide), three anti-diagonals rotate through LDS (four planes of packed words: DELETE, INSERT, MATCH and
// the best of the three), the running best is one wave-wide max of (score | j - lo) per anti-diagonal — ties go to the larger
// j exactly as MUMmer's ">=" scan does — and the band is trimmed from its edges with two ballots.  Same cells, same tie order
// and the same riding error counts as pgn::ScalarEngine (tests: GPU == host statement == MUMmer's own output files).
// A band wider than PN_LDS_CELLS (forced re-alignments of long backward extensions: MUMmer fills the whole rectangle there)
// runs the same code on the wave's slice of a global scratch buffer.
//
// Cost model (MI355X): a step is ~7 LDS reads + 4 writes per cell and ~110 wave instructions per chunk; integer / LDS work,
// no MFMA.  The band holds 60-100 live cells at 80-99 % identity (MUMmer trims at 600 below the best score only), three times
// the 32 of the banded64 extender: this stage is where the exact engine pays for being exact.

// the record bounds of a cluster's (reference record, query record) in stream / strand coordinates
__device__ __forceinline__ void chain_bounds(const RefDesc& R, const UnitDesc& U, const Chain& c, int32_t& r_lo, int32_t& r_hi,
                                             int32_t& q_lo, int32_t& q_hi) {
  r_lo = R.rec_start[c.rrec]; r_hi = R.rec_start[c.rrec + 1] - 1;
  q_lo = U.rec_start[c.qrec]; q_hi = U.rec_start[c.qrec + 1] - 1;
  if (U.strand) { const int32_t a = U.len - q_hi, b = U.len - q_lo; q_lo = a; q_hi = b; }
}
__device__ __forceinline__ uint32_t rev_fields2(uint32_t x) {   // the 16 two-bit fields of x in reverse order
  x = __brev(x);
  return ((x & 0x55555555u) << 1) | ((x >> 1) & 0x55555555u);
}
__device__ __forceinline__ uint32_t spread16(uint32_t x) {   // bit k of the low half -> bit 2k
  x = (x | (x << 8)) & 0x00FF00FFu;
  x = (x | (x << 4)) & 0x0F0F0F0Fu;
  x = (x | (x << 2)) & 0x33333333u;
  return (x | (x << 1)) & 0x55555555u;
}
// work list entries (unit, chain) of unit u at wl[choff[u] .. choff[u+1])
__global__ __launch_bounds__(64) void anim_wl_kernel(const uint32_t* __restrict__ choff, uint2* __restrict__ wl) {
  const uint32_t u = blockIdx.x, b = choff[u], n = choff[u + 1] - b;
  for (uint32_t c = threadIdx.x; c < n; c += 64) wl[b + c] = make_uint2(u, c);
}

// development counters (read back and printed when PYANI_PN_STATS is set): [0] calls / [1] anti-diagonals / [2] cells of the register
// engine, [3..5] LDS engine, [6..8] global-memory engine, [9] window moves, [10] register-engine overflows, [11] units, [12] clusters
__device__ unsigned long long g_pn_stats[32];
// per kernel (0 gaps, 1 forward, 2 backward-ahead, 3 walks, 4 forced narrow, 5 forced 512-1024, 6 forced 2048): calls, anti-diagonals, cells of the diagonal engine;
// the fourth word of classes 0 .. 3: ticks / rows of the walk kernel's shadow scans, ticks / calls of its reverse-target scans
__device__ unsigned long long g_pn_kstats[32];
// The counters are kept per WAVE in LDS and reach the global arrays once, when the wave ends (pn_stats_flush): one atomic per
// engine call on the same few addresses — 85 million per C4 launch — serialised in the L2's atomic unit and cost the gap and
// forward kernels ~0.3 s each (round 4: found when neither occupancy nor prefetching moved them).
__device__ __forceinline__ unsigned long long* pn_stats_lds() { __shared__ unsigned long long s_pn[64]; return s_pn; }      // [0..31] g_pn_stats, [32..63] g_pn_kstats
__device__ __forceinline__ void pn_stats_begin() {
  unsigned long long* s = pn_stats_lds();
  s[threadIdx.x & 63] = 0ull;
  __syncthreads();
}
__device__ __forceinline__ void pn_stats_flush() {
  __syncthreads();
  unsigned long long* s = pn_stats_lds();
  const int t = threadIdx.x & 63;
  const unsigned long long v = threadIdx.x < 64 ? s[t] : 0ull;      // ONE wave flushes: in a workgroup of several waves every wave used to add the same slot
  if (v) {
    if (t < 32) { if (t == 14 || t == 15 || t == 16 || t == 18 || t == 19 || t == 20) atomicMax(&g_pn_stats[t], v); else atomicAdd(&g_pn_stats[t], v); }
    else atomicAdd(&g_pn_kstats[t - 32], v);
  }
}
__device__ __forceinline__ void pn_stat(int k, unsigned long long v) { if ((threadIdx.x & 63) == 0 && v) atomicAdd(&pn_stats_lds()[k], v); }      // (LDS atomics: the walk kernel has two waves per workgroup)
// [13..16] units kernel / [17..20] forced kernel: busy ticks summed (100 MHz wall clock), longest single item as ticks << 20 | size,
// latest end and (complemented) earliest start — how much of a launch is one sequential item and how much is throughput
__device__ __forceinline__ void pn_stat_max(int k, unsigned long long v) { if ((threadIdx.x & 63) == 0) atomicMax(&pn_stats_lds()[k], v); }
__device__ __forceinline__ void pn_kstat(int k, unsigned long long calls, unsigned long long steps, unsigned long long cells) {
  if ((threadIdx.x & 63) == 0) { unsigned long long* s = pn_stats_lds() + 32 + 4 * k; atomicAdd(&s[0], calls); atomicAdd(&s[1], steps); atomicAdd(&s[2], cells); }
}
__device__ __forceinline__ void pn_stat_item(int k, unsigned long long t0, unsigned long long size) {
  const unsigned long long t1 = wall_clock64(), sz = size < 0xFFFFFull ? size : 0xFFFFFull;
  pn_stat(k, t1 - t0); pn_stat_max(k + 1, ((t1 - t0) << 20) | sz); pn_stat_max(k + 2, t1); pn_stat_max(k + 3, ~t0);
}

constexpr int PN_LDS_CELLS = 256;        // cells of one anti-diagonal kept in LDS (power of two)
constexpr int PN_GLOBAL_CELLS = 16384;   // ... in the wave's global scratch (>= MAX_ALIGNMENT_LENGTH + 1, power of two)
constexpr size_t PN_GLOBAL_WORDS = (size_t)3 * 4 * PN_GLOBAL_CELLS;

template <bool GLOBAL>
struct PnStore {
  static constexpr int CAP = GLOBAL ? PN_GLOBAL_CELLS : PN_LDS_CELLS;
  uint32_t* base;   // [3 diagonals][4 planes][CAP]
  __device__ __forceinline__ uint32_t* at(int d, int plane, int32_t j) const { return base + ((d * 4 + plane) * CAP + (j & (CAP - 1))); }
  __device__ __forceinline__ uint32_t ld(int d, int plane, int32_t j) const {
    if (GLOBAL) return __hip_atomic_load(at(d, plane, j), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return *at(d, plane, j);
  }
  __device__ __forceinline__ void st(int d, int plane, int32_t j, uint32_t v) const {
    if (GLOBAL) __hip_atomic_store(at(d, plane, j), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *at(d, plane, j) = v;
  }
};

// Cross-lane read-after-write through the store: LDS operations of a wave execute in order (wave_lds_fence keeps the compiler
// from moving them); the global variant has to wait for its stores (agent-scope, past the vector L1) before reading them back.
template <bool GLOBAL>
__device__ __forceinline__ void pn_fence() {
  // (no workgroup barrier: the walk kernel runs two independent waves per workgroup; the stores and loads of the global store are
  // agent-scope atomics past the vector L1, so what a wave needs is its own stores complete before its next loads)
  if (GLOBAL) { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent"); __builtin_amdgcn_wave_barrier(); } else wave_lds_fence();
}

// pgn::ScalarEngine::align, the lanes being the cells of an anti-diagonal.  Returns false if the band outgrew the store.
template <bool GLOBAL>
__device__ bool pn_align_wave(const SeqView& R, const StrandView& Q, uint32_t* mem, int32_t Astart, int32_t& Aend, int32_t Bstart,
                              int32_t& Bend, unsigned m_o, int32_t band_w, int32_t& errors, int32_t& score, bool& reached) {
  using namespace pgn;
  const PnStore<GLOBAL> S{mem};
  const int lane = threadIdx.x & 63;
  const bool fwd = m_o & DIRECTION_BIT, forced = m_o & FORCED_BIT;
  const int32_t N = fwd ? Aend - Astart + 1 : Astart - Aend + 1, M = fwd ? Bend - Bstart + 1 : Bstart - Bend + 1;
  int ip2 = 0, ip1 = 1, icur = 2;
  int32_t p2lo = 0, p2hi = -1, p1lo = 0, p1hi = 0;
  pn_fence<GLOBAL>();   // the previous call's reads are done
  if (lane == 0) { S.st(ip1, 0, 0, 0u); S.st(ip1, 1, 0, 0u); S.st(ip1, 2, 0, w_make(0, 0, ST_MATCH)); S.st(ip1, 3, 0, w_make(0, 0, ST_MATCH)); }
  pn_fence<GLOBAL>();
  int32_t high = -(1 << 30), FinishCt = 0, FinishJ = 0;
  uint32_t high_w = 0;
  int32_t jlo = 0, jhi = 1, Dct;
  bool fits = true;
  unsigned long long stat_cells = 0;
  for (Dct = 1; Dct <= N + M && (forced || Dct - FinishCt <= pgn::BREAK_LEN) && jlo <= jhi; ++Dct) {
    int32_t lo = jlo, hi = jhi;
    if (lo < Dct - N) lo = Dct - N;
    if (lo < 0) lo = 0;
    if (hi > M) hi = M;
    if (hi > Dct) hi = Dct;
    if (band_w >= 0) forced_band_clip(Dct, N, M, band_w, lo, hi);
    if (lo > hi) break;
    if (hi - lo + 1 > PnStore<GLOBAL>::CAP) { fits = false; break; }
    stat_cells += (unsigned long long)(hi - lo + 1);
    uint32_t bestk = 0, bestw = 0;
    for (int32_t c0 = lo; c0 <= hi; c0 += 64) {
      const int32_t j = c0 + lane, i = Dct - j;
      const bool act = j <= hi;
      const bool hasL = act && j >= 1 && j - 1 >= p1lo && j - 1 <= p1hi, hasU = act && i >= 1 && j >= p1lo && j <= p1hi;
      const bool hasG = act && i >= 1 && j >= 1 && j - 1 >= p2lo && j - 1 <= p2hi;
      Cell L{0, 0, 0, 0}, U{0, 0, 0, 0};
      uint32_t G = 0;
      bool sm = false;
      if (hasL) { L.D = S.ld(ip1, 0, j - 1); L.I = S.ld(ip1, 1, j - 1); L.M = S.ld(ip1, 2, j - 1); }
      if (hasU) { U.D = S.ld(ip1, 0, j); U.I = S.ld(ip1, 1, j); U.M = S.ld(ip1, 2, j); }
      if (hasG) {
        G = S.ld(ip2, 3, j - 1);
        const int64_t pa = fwd ? (int64_t)Astart + i - 1 : (int64_t)Astart - i + 1, pb = fwd ? (int64_t)Bstart + j - 1 : (int64_t)Bstart - j + 1;
        sm = R.clean(pa) && Q.clean(pb) && R.base(pa) == Q.base(pb);
      }
      const Cell c = cell_update(L, U, G, sm);
      if (act) {
        S.st(icur, 0, j, c.D); S.st(icur, 1, j, c.I); S.st(icur, 2, j, c.M); S.st(icur, 3, j, c.X);
        const uint32_t key = (c.X & ~(W_ONE - 1u)) | (uint32_t)(j - lo);   // score field | position in the band
        if (key >= bestk) { bestk = key; bestw = c.X; }
      }
    }
    pn_fence<GLOBAL>();
    {
      const uint32_t gk = wave_max_u32(bestk);
      const uint64_t who = __ballot(bestk == gk);
      const uint32_t gw = (uint32_t)__builtin_amdgcn_readlane((int)bestw, __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(who)));
      const int32_t s = w_score(gk);
      if (s >= high) { high = s; high_w = gw; FinishCt = Dct; FinishJ = lo + (int32_t)(gk & (W_ONE - 1u)); }
    }
    int32_t tlo = lo, thi = hi;
    if (!forced) {
      tlo = hi + 1;
      for (int32_t c0 = lo; c0 <= hi; c0 += 64) {
        const int32_t j = c0 + lane;
        const bool ok = j <= hi && !(high - w_score(S.ld(icur, 3, j)) > MAX_DIFF);
        const uint64_t b = __ballot(ok);
        if (b) { tlo = c0 + (int32_t)__builtin_ctzll(b); break; }
      }
      thi = tlo - 1;
      for (int32_t c1 = hi; c1 >= tlo; c1 -= 64) {
        const int32_t j = c1 - 63 + lane;
        const bool ok = j >= tlo && j <= hi && !(high - w_score(S.ld(icur, 3, j)) > MAX_DIFF);
        const uint64_t b = __ballot(ok);
        if (b) { thi = c1 - 63 + (63 - (int32_t)__builtin_clzll(b)); break; }
      }
    }
    jlo = tlo; jhi = thi + 1;
    if (tlo > thi) { jlo = 1; jhi = 0; }
    const int t = ip2; ip2 = ip1; ip1 = icur; icur = t;
    p2lo = p1lo; p2hi = p1hi; p1lo = lo; p1hi = hi;
  }
  pn_stat(GLOBAL ? 6 : 3, 1); pn_stat(GLOBAL ? 7 : 4, (unsigned long long)Dct); pn_stat(GLOBAL ? 8 : 5, stat_cells);
  if (!fits) return false;
  --Dct;
  reached = false;
  uint32_t fin_w = high_w;
  if (Dct == N + M) {
    if (!(m_o & OPTIMAL_BIT)) { reached = true; FinishCt = N + M; FinishJ = M; fin_w = S.ld(ip1, 3, M); }
    else if (FinishCt == Dct) reached = true;
  }
  const int32_t fi = FinishCt - FinishJ, fj = FinishJ;
  Aend = fwd ? Astart + fi - 1 : Astart - fi + 1;
  Bend = fwd ? Bstart + fj - 1 : Bstart - fj + 1;
  errors = (int32_t)w_errors(fin_w);
  score = w_score(fin_w);
  return true;
}

// ---- the same engine with the band in REGISTERS ------------------------------------------------------------------------------
// Lane f of register set s holds column j = base + 64 s + f: the three state words of its cell on the previous anti-diagonal
// (the cell ABOVE the one it computes next, since i = Dct - j moves with Dct), the best-state word of the one before that, and
// the B base of column j.  The left neighbour's words arrive by one DPP wave shift each (lane 0 of a set takes lane 63 of the set
// below through readlane), the A bases slide the same way — one lane per anti-diagonal — with a fresh base entering at the
// lowest live set, so a step touches no memory at all: one v_max3 per state thanks to the word format, one wave max for the
// running best, one ballot per live set for the trimming.  The window [base, base + 64 S) follows the band in whole sets: when
// column lo - 1 (the last one still read) has left set 0, every set moves down by one — pure register renaming.  Only the sets
// that hold columns lo - 1 .. max(hi, previous hi) are touched in a step.  S sets hold bands of up to 64 (S - 1) - 1 cells:
// S = 3 for MUMmer's own (trimmed) bands — the widest seen on any fixture is 110 cells — and for the first certified bands of
// forced runs, S = 5 / 9 / 17 for the wider certified bands (divergent genomes need them: ~55 % of all cells of the C3 grid are
// forced re-alignments of 250-1000 cells per anti-diagonal); anything wider starts over in the LDS / global engines above.
// Wave-uniform values, said so: everything an engine call is given (coordinates, mode, sequence views) is the same in all 64 lanes,
// but it arrives through vector loads, so the compiler would keep the whole band bookkeeping (lo, hi, base, the set range, the
// running best) in vector registers under exec masks.  One v_readfirstlane each puts it in scalar registers: the step loop's control
// flow becomes scalar branches and its arithmetic SALU, next to the VALU work of the cells.
__device__ __forceinline__ int32_t pn_uni(int32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint32_t pn_uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ int64_t pn_uni(int64_t v) {
  const uint32_t lo = pn_uni((uint32_t)(uint64_t)v), hi = pn_uni((uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
template <class T> __device__ __forceinline__ T* pn_uni(T* p) { return (T*)(uintptr_t)pn_uni((int64_t)(uintptr_t)p); }
__device__ __forceinline__ SeqView pn_uni(const SeqView& v) { return SeqView{pn_uni(v.codes), pn_uni(v.mask), pn_uni(v.len)}; }
__device__ __forceinline__ StrandView pn_uni(const StrandView& v) { return StrandView{pn_uni(v.s), pn_uni(v.rc)}; }

__device__ __forceinline__ uint32_t pn_shr1(uint32_t v, uint32_t carry_in) {   // lane l <- lane l - 1, lane 0 <- carry_in (uniform)
  uint32_t r = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, true);   // wave_shr:1, lane 0 <- 0
  return (threadIdx.x & 63) == 0 ? carry_in : r;
}
__device__ __forceinline__ uint32_t pn_lane(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }

struct PnRegSet { uint32_t D1, I1, M1, X1, X2, b, a; };   // b / a: base codes (0-3; 5 / 4 = not a clean base, never equal)

// Strips: a forced run wider than the widest register engine is cut into column strips [j0, j1) of at most 64 (S - 1) - 1
// columns, swept one after the other over all their anti-diagonals (forced runs have neither trimming nor a break, so the DP is a
// plain global alignment and any evaluation order of its cells gives the same words).  A strip reads the state words of the
// column to its left, row by row, from `bin` (written by the strip before it, 4 words per row, fetched 64 rows at a time: one
// lane per row, then a readlane per step) and writes its own last column to `bout`.
struct PnStrip { int32_t j0, j1; const uint32_t* bin; uint32_t* bout; };
struct PnRunInfo { unsigned long long cells; int32_t wmax; };      // of one engine call: what a traceback of the same call has to store

template <int S>
__device__ bool pn_align_regs(const SeqView& R_, const StrandView& Q_, int32_t Astart_, int32_t& Aend, int32_t Bstart_, int32_t& Bend,
                              unsigned m_o_, int32_t band_w_, int32_t& errors, int32_t& score, bool& reached,
                              const PnStrip* strip_ = nullptr, PnRunInfo* info = nullptr) {
  using namespace pgn;
  constexpr int32_t MAX_WIDTH = 64 * (S - 1) - 1;
  const int lane = threadIdx.x & 63;
  const SeqView R = pn_uni(R_);
  const StrandView Q = pn_uni(Q_);
  const int32_t Astart = pn_uni(Astart_), Bstart = pn_uni(Bstart_), Aend0 = pn_uni(Aend), Bend0 = pn_uni(Bend), band_w = pn_uni(band_w_);
  const unsigned m_o = pn_uni((uint32_t)m_o_);
  PnStrip strip_u{0, 0, nullptr, nullptr};
  if (strip_) strip_u = PnStrip{pn_uni(strip_->j0), pn_uni(strip_->j1), pn_uni(strip_->bin), pn_uni(strip_->bout)};
  const PnStrip* strip = strip_ ? &strip_u : nullptr;
  const bool fwd = m_o & DIRECTION_BIT, forced = m_o & FORCED_BIT;
  const int32_t N = fwd ? Aend0 - Astart + 1 : Astart - Aend0 + 1, M = fwd ? Bend0 - Bstart + 1 : Bstart - Bend0 + 1;
  const int32_t j0 = strip ? strip->j0 : 0, j1 = strip ? strip->j1 : M + 1;      // columns of this call
  const auto a_code = [&](int32_t i) -> uint32_t {   // A base of row i (1-based), 4 outside / dirty
    const int64_t p = fwd ? (int64_t)Astart + i - 1 : (int64_t)Astart - i + 1;
    return (i >= 1 && i <= N && R.clean(p)) ? (uint32_t)R.base(p) : 4u;
  };
  const auto b_code = [&](int32_t j) -> uint32_t {
    const int64_t p = fwd ? (int64_t)Bstart + j - 1 : (int64_t)Bstart - j + 1;
    return (j >= 1 && j <= M && Q.clean(p)) ? (uint32_t)Q.base(p) : 5u;
  };
  PnRegSet T[S];
#pragma unroll
  for (int s = 0; s < S; ++s) T[s] = PnRegSet{0u, 0u, 0u, 0u, 0u, 5u, 4u};
  int32_t base = j0;
  int s_hi_loaded = 0;        // sets 0 .. s_hi_loaded carry valid b / a bases
  T[0].b = b_code(base + lane);
  if (j0 == 0 && lane == 0) { T[0].M1 = w_make(0, 0, ST_MATCH); T[0].X1 = T[0].M1; }   // anti-diagonal 0: the cell (0, 0), as step 1's "previous"
  int32_t d_first = j0 > 0 ? j0 : 1;
  int32_t d_last = strip ? (N + j1 - 1 < N + M ? N + j1 - 1 : N + M) : N + M;
  // A strip of a BANDED run only walks the anti-diagonals on which the band crosses its columns (diagonals k = j - i = 2 j - Dct
  // within [kmin, kmax]): a 10 000 x 10 000 run at w = 1020 touches ~2 500 of a strip's 10 500 anti-diagonals.  Everything
  // outside the band is dead (zero words) by definition, so the strip starts from zeroed registers at its first live
  // anti-diagonal, and rows of the left neighbour column outside the band read as zeros without being fetched (the strip before
  // this one did not walk them either).
  int32_t brow_lo = 0, brow_hi = N;
  if (strip && band_w >= 0) {
    const int32_t kmin = (M - N < 0 ? M - N : 0) - band_w, kmax = (M - N > 0 ? M - N : 0) + band_w;
    const int32_t ds = 2 * j0 - kmax, de = 2 * (j1 - 1) - kmin;
    if (ds > d_first) d_first = ds;
    if (de < d_last) d_last = de;
    brow_lo = (j0 - 1) - kmax; brow_hi = (j0 - 1) - kmin;
    if (brow_lo < 0) brow_lo = 0;
    if (brow_hi > N) brow_hi = N;
  }
  if (j0 > 0) T[0].a = a_code(d_first - 1 - (base + lane));
  // the A base entering the lowest live set: column fcol takes row Dct - fcol; rows f_i0 .. f_i0 + 63 are held one per lane
  int32_t fcol = j0, f_i0 = d_first - j0;
  uint32_t afeed = a_code(f_i0 + lane);
  // strip input: rows g_i0 .. g_i0 + 63 of the left neighbour column, one per lane
  int32_t g_i0 = -64;
  uint32_t gD = 0u, gI = 0u, gM = 0u, gX = 0u;
  // strip output: rows o_i0 .. o_i0 + o_n - 1 of this strip's last column, one per lane, not yet stored
  int32_t o_i0 = -1, o_n = 0;
  uint32_t oD = 0u, oI = 0u, oM = 0u, oX = 0u;
  int32_t high = -(1 << 30), FinishCt = 0, FinishJ = 0;
  uint32_t high_w = 0;
  int32_t jlo = j0, jhi = j0 > 0 ? j0 : 1, Dct;
  int32_t phi = j0, pphi = j0;   // computed upper ends of the last two anti-diagonals (their columns still hold data)
  unsigned long long stat_cells = 0, stat_moves = 0;
  int32_t stat_wmax = 0;
  // (two loops: the window move — every set's registers renamed — stays out of the step loop, whose loop-carried registers then
  // need no copies; after a move the same anti-diagonal is taken up again)
  // ONE exit from the step loop (`why`, computed without branches): with several, the compiler's loop-exit unification copies every
  // live state register into exit temporaries and back on each iteration (2 x 26 v_mov per step)
  int why = 4;      // 1: done (end / break length / band empty), 2: band empty after clipping, 3: wider than the engine, 4: window move
  int32_t move_lo = base + 1;
  Dct = d_first;
  while (why == 4) {
  while (move_lo - 1 - base >= 64) {
#pragma unroll
    for (int s = 0; s + 1 < S; ++s) T[s] = T[s + 1];
    T[S - 1] = PnRegSet{0u, 0u, 0u, 0u, 0u, 5u, 4u};
    base += 64;
    s_hi_loaded = s_hi_loaded > 0 ? s_hi_loaded - 1 : 0;
    ++stat_moves;
  }
  for (;; ++Dct) {
    int32_t lo = jlo, hi = jhi;
    if (strip) { lo = j0; hi = j1 - 1; }              // a forced run: every cell of the (band-clipped) rectangle
    if (lo < Dct - N) lo = Dct - N;
    if (lo < 0) lo = 0;
    if (hi > M) hi = M;
    if (hi > Dct) hi = Dct;
    if (band_w >= 0) forced_band_clip(Dct, N, M, band_w, lo, hi);
    if (strip) { if (lo < j0) lo = j0; if (hi > j1 - 1) hi = j1 - 1; }
    const bool go = (Dct <= d_last) & (forced | (Dct - FinishCt <= pgn::BREAK_LEN)) & ((strip != nullptr) | (jlo <= jhi));
    // columns below lo - 1 are never read again: once they fill set 0, every set moves down by one (outside this loop)
    why = !go ? 1 : ((lo > hi) & (strip == nullptr)) ? 2 : (hi - lo + 1 > MAX_WIDTH) ? 3 : ((strip == nullptr) & (lo - 1 - base >= 64)) ? 4 : 0;
    move_lo = lo;
    if (why) break;
    if (hi >= lo) stat_cells += (unsigned long long)(hi - lo + 1);
    if (hi - lo + 1 > stat_wmax) stat_wmax = hi - lo + 1;
    int32_t first = lo - 1 > base ? lo - 1 : base;              // lowest column touched: lo - 1 is read, not computed
    int32_t top = hi > phi ? (hi > pphi ? hi : pphi) : (phi > pphi ? phi : pphi);   // highest column that holds or gets data
    if (strip) { first = base; if (top < base) top = base; if (top > j1 - 1) top = j1 - 1; }   // (a strip keeps all its sets in step)
    const int s_lo = (first - base) >> 6, s_top = (top - base) >> 6;
    // sets that come into play (again): their B bases, and the A rows their lanes would have received so far; a set the band
    // has left is forgotten, its A bases stop sliding
    if (s_hi_loaded > s_top) s_hi_loaded = s_top;
    while (s_hi_loaded < s_top) {
      ++s_hi_loaded;
#pragma unroll
      for (int s = 1; s < S; ++s)
        if (s == s_hi_loaded) { const int32_t j = base + 64 * s + lane; T[s].b = b_code(j); T[s].a = a_code(Dct - 1 - j); }
    }
    // the A base for the first lane of set s_lo
    const int32_t col0 = base + 64 * s_lo;
    if (col0 != fcol || Dct - col0 - f_i0 >= 64 || Dct - col0 - f_i0 < 0) { fcol = col0; f_i0 = Dct - col0; afeed = a_code(f_i0 + lane); }
    const uint32_t a_in = pn_lane(afeed, __builtin_amdgcn_readfirstlane(Dct - col0 - f_i0));
    uint32_t bestk = 0, bestw = 0;
    uint32_t cD = 0u, cI = 0u, cM = 0u, cX2 = 0u, cA = a_in;       // carries into lane 0 of the set being processed
    if (strip && strip->bin) {
      // the left neighbour column (j0 - 1) of this strip: row i = Dct - j0 on the previous anti-diagonal, row i - 1 two back
      const int32_t i = Dct - j0;
      if (i - g_i0 >= 64 || i < g_i0) {
        g_i0 = i;
        const int32_t r = g_i0 + lane;
        const bool in = r >= brow_lo && r <= brow_hi;
        const uint32_t* e = strip->bin + (size_t)(in ? r : 0) * 4;
        gD = in ? __hip_atomic_load(e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        gI = in ? __hip_atomic_load(e + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        gM = in ? __hip_atomic_load(e + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        gX = in ? __hip_atomic_load(e + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
      }
      const int at = __builtin_amdgcn_readfirstlane(i - g_i0);
      cD = pn_lane(gD, at); cI = pn_lane(gI, at); cM = pn_lane(gM, at);
      // row i - 1: the lane before, or (at a block start) what the previous block's last lane held — kept in cX2_prev
      cX2 = at > 0 ? pn_lane(gX, at - 1) : 0u;
      if (at == 0 && i - 1 >= brow_lo && i - 1 <= brow_hi) cX2 = __hip_atomic_load(strip->bin + (size_t)(i - 1) * 4 + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    int32_t tlo = hi + 1, thi = lo - 1;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      if (s < s_lo || s > s_top) continue;                          // (uniform)
      const int32_t j = base + 64 * s + lane;
      const bool act = j >= lo && j <= hi;
      // this set's lane 63 feeds the next set's lane 0: taken before the set is overwritten
      const uint32_t nD = pn_lane(T[s].D1, 63), nI = pn_lane(T[s].I1, 63), nM = pn_lane(T[s].M1, 63), nX2 = pn_lane(T[s].X2, 63), nA = pn_lane(T[s].a, 63);
      const Cell L{pn_shr1(T[s].D1, cD), pn_shr1(T[s].I1, cI), pn_shr1(T[s].M1, cM), 0u};
      const Cell U{T[s].D1, T[s].I1, T[s].M1, 0u};
      const uint32_t G = pn_shr1(T[s].X2, cX2);
      T[s].a = pn_shr1(T[s].a, cA);
      Cell c = cell_update(L, U, G, T[s].a == T[s].b);
      if (!act) c = Cell{0u, 0u, 0u, 0u};
      T[s].X2 = T[s].X1; T[s].D1 = c.D; T[s].I1 = c.I; T[s].M1 = c.M; T[s].X1 = c.X;
      cD = nD; cI = nI; cM = nM; cX2 = nX2; cA = nA;
      const uint32_t key = act ? ((c.X & ~(W_ONE - 1u)) | (uint32_t)(j - lo)) : 0u;
      if (key >= bestk) { bestk = key; bestw = c.X; }
    }
    if (strip && strip->bout) {
      // this strip's last column, row i = Dct - (j1 - 1): its words of this anti-diagonal (zeros where the band does not reach).
      // Rows come one per step; they are staged one per LANE and leave 64 rows at a time as one coalesced 1 KiB store (round 3
      // wrote every row with four 4-byte write-through stores from one lane: 16 x write amplification on partial lines, 110 GB
      // of WRITE_SIZE per launch for ~15 GB of boundary data).
      const int32_t i = Dct - (j1 - 1), f = j1 - 1 - base;
      if (i >= 0 && i <= N) {
        uint32_t vD = 0u, vI = 0u, vM = 0u, vX = 0u;
#pragma unroll
        for (int s = 0; s < S; ++s)
          if ((f >> 6) == s && s >= s_lo && s <= s_top) {
            const int fl = __builtin_amdgcn_readfirstlane(f & 63);
            vD = pn_lane(T[s].D1, fl); vI = pn_lane(T[s].I1, fl); vM = pn_lane(T[s].M1, fl); vX = pn_lane(T[s].X1, fl);
          }
        if (o_i0 < 0) o_i0 = i;
        if (i - o_i0 >= 64) {      // the staged block is full: out it goes
          *reinterpret_cast<uint4*>(strip->bout + (size_t)(o_i0 + lane) * 4) = make_uint4(oD, oI, oM, oX);
          o_i0 = i;
        }
        if (lane == i - o_i0) { oD = vD; oI = vI; oM = vM; oX = vX; }
        o_n = i - o_i0 + 1;
      }
    }
    if (!strip) {
      const uint32_t gk = wave_max_u32(bestk);
      const uint64_t who = __ballot(bestk == gk);
      const uint32_t gw = pn_lane(bestw, __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(who)));
      const int32_t sc = w_score(gk);
      if (sc >= high) { high = sc; high_w = gw; FinishCt = Dct; FinishJ = lo + (int32_t)(gk & (W_ONE - 1u)); }
    }
    if (!forced) {
#pragma unroll
      for (int s = 0; s < S; ++s) {
        if (s < s_lo || s > s_top) continue;
        const int32_t j = base + 64 * s + lane;
        const uint64_t ok = __ballot(j >= lo && j <= hi && !(high - w_score(T[s].X1) > MAX_DIFF));
        if (ok) {
          if (tlo > hi) tlo = base + 64 * s + (int32_t)__builtin_ctzll(ok);
          thi = base + 64 * s + 63 - (int32_t)__builtin_clzll(ok);
        }
      }
    } else { tlo = lo; thi = hi; }
    jlo = tlo; jhi = thi + 1;
    if (tlo > thi) { jlo = 1; jhi = 0; }
    pphi = phi; phi = hi >= lo ? hi : phi;
  }
  }
  if (strip && strip->bout && o_i0 >= 0 && lane < o_n)
    *reinterpret_cast<uint4*>(strip->bout + (size_t)(o_i0 + lane) * 4) = make_uint4(oD, oI, oM, oX);
  if (why == 3) { pn_stat(10, 1); return false; }
  if (info) { info->cells = stat_cells; info->wmax = stat_wmax; }
  pn_stat(0, 1); pn_stat(1, (unsigned long long)(Dct - d_first)); pn_stat(2, stat_cells); pn_stat(9, stat_moves);
  --Dct;
  reached = false;
  uint32_t fin_w = high_w;
  if (Dct == N + M) {
    if (!(m_o & OPTIMAL_BIT)) {
      reached = true; FinishCt = N + M; FinishJ = M;
      const int32_t f = M - base;
      fin_w = 0u;
#pragma unroll
      for (int s = 0; s < S; ++s) if (f >= 64 * s && f < 64 * s + 64) fin_w = pn_lane(T[s].X1, __builtin_amdgcn_readfirstlane(f - 64 * s));
    } else if (FinishCt == Dct) reached = true;
  }
  const int32_t fi = FinishCt - FinishJ, fj = FinishJ;
  Aend = fwd ? Astart + fi - 1 : Astart - fi + 1;
  Bend = fwd ? Bstart + fj - 1 : Bstart - fj + 1;
  errors = (int32_t)w_errors(fin_w);
  score = w_score(fin_w);
  return true;
}

#include "pga_postnuc_diag.inc"

// A forced re-alignment put off: it only adds its error count to one alignment (pg_nucmer_core.h, postnuc_unit), so the unit's wave
// does not wait for it — anim_postnuc_forced_kernel runs them all, one wave each, after the units are done.  More than half of
// the cells of a divergent job are such runs (whole rectangles for MUMmer; certified bands of 30-1000 cells here): inside their
// units they would serialise behind one another, on their own they fill the GPU, and the units' kernel keeps the register
// budget of the narrow engine (3 waves per SIMD instead of 1).
struct PnForcedReq { int32_t A0, A1, B0, B1; uint32_t unit; int32_t w; pgn::PnAln* dst; };      // w: the band it certified with (-1: the whole rectangle), set by the forced kernel

// DIAG_ONLY: the engine of the pre-pass kernels (match-to-match, forward, backward-ahead): a call whose band outgrows the
// 256-diagonal window is not retried on the column / LDS / global engines but reported (overflow) and left to the unit's walk,
// which has them — a thousand of 24 million calls per C4 launch — so these kernels carry ~50 vector registers instead of ~90 and
// run eight waves per SIMD: the short calls of the gap kernel wait on their first loads two thirds of the time.
template <bool DIAG_ONLY>
struct PnWaveEngineT {
  const SeqView R;
  const StrandView Q;
  uint32_t* lds;
  uint32_t* glob;
  int32_t overflow;
  PnForcedReq* reqs;          // deferred forced runs of the launch (null: run them in place)
  uint32_t* n_reqs;
  uint32_t req_cap, unit;
  const pgn::PnGap* gaps;     // the unit's match-to-match alignments, by match slot (anim_postnuc_gap_kernel ran before)
  __device__ bool gap_ready(int32_t slot, pgn::PnGap& g) const { if (!gaps) return false; g = gaps[slot]; return g.reached >= 0; }      // reached < 0: left to the walk
  // pgn::ScalarEngine::gap_run, 64 matches per step: lane l looks at the alignment from match m + l to the next one; the run ends at
  // the first that is not ready, did not reach its target or did not end on it
  __device__ int gap_run(const Match* mm, int32_t first_slot, int m, int count, int32_t& errors) const {
    if (!gaps || pieces) return m;
    const int lane = threadIdx.x & 63;
    int32_t add = 0;
    for (;;) {
      const int t = m + lane;
      bool ok = false;
      int32_t e = 0;
      if (t + 1 < count) {
        const pgn::PnGap g = gaps[first_slot + t];
        const Match Mn = mm[t + 1];
        ok = g.reached > 0 && g.eA == Mn.r && g.eB == Mn.q;
        e = g.errors;
      }
      const uint64_t okm = __ballot(ok);
      const int n_ok = okm == ~0ull ? 64 : (int)__builtin_ctzll(~okm);
      int32_t v = lane < n_ok ? e : 0;
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      add += v;
      m += n_ok;
      if (n_ok < 64) break;
    }
    errors += add;
    return m;
  }
  const pgn::PnFwd* fwd;      // the unit's forward extensions, by position in `order` (anim_postnuc_fwd_kernel ran before); reached < 0: not there
  __device__ bool fwd_ready(int k, pgn::PnFwd& f) const {
    if (!fwd) return false;
    f = fwd[k];
    if (kstat == 3) pn_stat(32 + 19, 1);      // development counter: forward results the WALK took (÷ the forward kernel's calls = consumed fraction)
    return f.reached >= 0;
  }
  // traceback runs (pg_anim_alignments_batch with indel lists): the walk lists its pieces (pg_nucmer_core.h, PnPiece) and aligns
  // everything itself (no pre-passes: gaps == fwd == nullptr), so that every piece carries the arguments of its engine call
  pgn::PnPiece* pieces = nullptr;
  int32_t piece_cap = 0, n_pieces = 0;
  uint32_t last_cells = 0, last_wmax = 0, last_req = 0;
  int kstat = -1;      // development counters: which kernel this engine runs in (g_pn_kstats)
  const pgn::PnBwd* bwd = nullptr;      // the unit's backward searches run ahead (anim_postnuc_bwd_kernel), by position in `order`
  __device__ bool bwd_ready(int k, pgn::PnBwd& b) const {
    if (!bwd) return false;
    b = bwd[k];
    if (kstat == 3) pn_stat(32 + 23, b.state == 2 ? 1 : 0);      // development counter: backward searches the walk found run ahead (taken if the arguments agree: 1 - walk searches / these)
    return b.state == 2;
  }
  __device__ void bwd_key(int, int32_t, int32_t, int32_t, int32_t, unsigned) {}
  __device__ void piece(uint32_t kind, int32_t aln, int32_t A0, int32_t B0, int32_t A1, int32_t B1, int32_t tA, int32_t tB, unsigned m_o) {
    if (!pieces) return;
    if (n_pieces < piece_cap && (threadIdx.x & 63) == 0)
      pieces[n_pieces] = pgn::PnPiece{aln, kind, m_o, A0, B0, A1, B1, tA, tB, last_cells, last_wmax, last_req};
    ++n_pieces;
  }
  // ---- the scans of extendClusters, 64 candidates per step (pg_nucmer_core.h: same answers as the scalar walks) ----------------
  // Done serially by every lane, the shadow test alone is O(clusters x alignments) dependent global loads: seconds per unit.
  __device__ bool shadowed(const Chain* chains, const pgn::PnAln* al, int from, int c, int32_t sA, int32_t eA, int32_t sB, int32_t eB) const {
    const int lane = threadIdx.x & 63;
    for (int t0 = from; t0 >= 0; t0 -= 64) {
      const int t = t0 - lane;
      const bool hit = t >= 0 && pgn::pn_shadow_hit(chains, al[t], c, sA, eA, sB, eB);
      if (__ballot(hit)) return true;
    }
    return false;
  }
  // the earliest of the unit's alignments that contains the cluster (-1: none), 64 per step
  __device__ int shadow_first(const Chain* chains, const pgn::PnAln* al, int n_al, int c, int32_t sA, int32_t eA, int32_t sB, int32_t eB) const {
    const int lane = threadIdx.x & 63;
    const unsigned long long w0 = wall_clock64();
    int found = -1, t0 = 0;
    for (; t0 < n_al; t0 += 64) {
      const int t = t0 + lane;
      const uint64_t hit = __ballot(t < n_al && pgn::pn_shadow_hit(chains, al[t], c, sA, eA, sB, eB));
      if (hit) { found = t0 + (int)__builtin_ctzll(hit); break; }
    }
    if (kstat == 3) { pn_stat(32 + 3, wall_clock64() - w0); pn_stat(32 + 7, (unsigned long long)(t0 / 64 + 1)); }      // development counters of the walk kernel: ticks / rows of this scan
    return found;
  }
  // the latest close-enough alignment wins; failing that, the smallest distance below `dist` (ties: the later alignment)
  __device__ int reverse_target(const Chain* chains, const pgn::PnAln* al, int cura, int c, int32_t sA, int32_t sB, int32_t dist) const {
    const int lane = threadIdx.x & 63;
    int tgt = -1;
    const unsigned long long w0 = wall_clock64();
    struct Done { const unsigned long long w0; const int kstat; __device__ ~Done() { if (kstat == 3) { pn_stat(32 + 11, wall_clock64() - w0); pn_stat(32 + 15, 1); } } } done{w0, kstat};
    for (int t0 = cura - 1; t0 >= 0; t0 -= 64) {
      const int t = t0 - lane;     // lane 0 = the latest alignment of this block
      pgn::PnCand x{false, false, 0, 0, 0};
      if (t >= 0) x = pgn::pn_reverse_cand(chains, al[t], c, sA, sB);
      const uint64_t close = __ballot(x.valid && x.close);
      // candidates before the first close one (in scan order = ascending lane) may still lower the distance
      const int stop = close ? (int)__builtin_ctzll(close) : 64;
      const uint32_t key = (x.valid && lane < stop && x.dist < dist) ? (((uint32_t)x.dist << 6) | (uint32_t)lane) : 0xFFFFFFFFu;
      const uint32_t best = wave_min_u32(key);        // distances here are < 2^25: smallest distance, then the earliest lane
      if (best != 0xFFFFFFFFu) { tgt = t0 - (int)(best & 63u); dist = (int32_t)(best >> 6); }
      if (close) return t0 - stop;
    }
    return tgt;
  }
  // the first close-enough cluster in reference order wins; failing that, the smallest distance below `dist` (ties: the earlier)
  __device__ int forward_target(const Chain* chains, const Match* cm, const int32_t* order, int n, int curk, int c, int32_t sA,
                                int32_t sB, int32_t dist, int32_t& targetA, int32_t& targetB) const {
    const int lane = threadIdx.x & 63;
    int targetk = -1;
    const int32_t my_rrec = pn_uni(chains[c].rrec);
    for (int k0 = curk + 1; k0 < n; k0 += 64) {
      // the clusters are in reference order, so their reference records never go down: past this cluster's record no candidate is
      // valid any more (pn_same_records) — the scan of a cluster with nothing close ahead ends with its record, not with the unit
      if (pn_uni(chains[pn_uni(order[k0])].rrec) > my_rrec) break;
      const int k = k0 + lane;
      pgn::PnCand x{false, false, 0, 0, 0};
      if (k < n) x = pgn::pn_forward_cand(chains, cm, order[k], c, sA, sB);
      const uint64_t close = __ballot(x.valid && x.close);
      const int stop = close ? (int)__builtin_ctzll(close) : 64;
      const uint32_t key = (x.valid && lane < stop && x.dist < dist) ? (((uint32_t)x.dist << 6) | (uint32_t)lane) : 0xFFFFFFFFu;
      const uint32_t best = wave_min_u32(key);
      int pick = -1;
      if (best != 0xFFFFFFFFu) { pick = (int)(best & 63u); dist = (int32_t)(best >> 6); }
      if (close) pick = stop;
      if (pick >= 0) {
        targetk = k0 + pick;
        targetA = __builtin_amdgcn_readlane(x.a, __builtin_amdgcn_readfirstlane(pick));
        targetB = __builtin_amdgcn_readlane(x.b, __builtin_amdgcn_readfirstlane(pick));
      }
      if (close) break;
    }
    return targetk;
  }
  // MUMmer's own band (searches and alignments): the 127-cell register engine, then LDS, then global memory
  __device__ bool align(int32_t Astart, int32_t& Aend, int32_t Bstart, int32_t& Bend, unsigned m_o, int32_t& errors) {
    int32_t score = 0, a = Aend, b = Bend;
    bool reached = false;
    const unsigned long long t0 = wall_clock64();
    PnRunInfo info{0ull, 0};
    // the diagonal window of 256 first (pga_postnuc_diag.inc); a band that outgrows it (> ~125 cells per anti-diagonal: a thousand
    // of 24 million calls per C4 launch) starts over on the 512-diagonal window, and what even that cannot hold on the wave's slice
    // of global memory (exact at any width, slow: never seen).  Round 5: the column-layout register engine and the LDS engine of
    // round 3 used to stand in between — they cost the walk kernel 222 VGPRs (two waves per SIMD) for calls that are this rare,
    // and the walks are latency-bound: what they need is waves in flight.
    PnRunInfo* const ip = pieces ? &info : nullptr;      // (only a listing walk needs the call's bookkeeping)
    bool in_regs = pn_align_diag<4>(R, Q, Astart, a, Bstart, b, m_o, -1, errors, score, reached, ip, kstat);
    if (DIAG_ONLY) {
      if (!in_regs) { overflow = 1; a = Astart; b = Bstart; errors = 0; reached = false; }
      Aend = a; Bend = b;
      return reached;
    }
    if (!in_regs) { a = Aend; b = Bend; in_regs = pn_align_diag<8>(R, Q, Astart, a, Bstart, b, m_o, -1, errors, score, reached, ip, kstat); }
    last_cells = in_regs && info.cells < 0xFFFFFFFFull ? (uint32_t)info.cells : 0xFFFFFFFFu; last_wmax = (uint32_t)info.wmax;
    pn_stat(21, (unsigned long long)wall_clock64() - t0); pn_stat(22, 1);      // [21] ticks inside the engine, [22] calls (units + gap kernels)
    if (in_regs) { Aend = a; Bend = b; return reached; }
    a = Aend; b = Bend;
    if (!pn_align_wave<true>(R, Q, glob, Astart, a, Bstart, b, m_o, -1, errors, score, reached)) { overflow = 1; a = Astart; b = Bstart; errors = 0; reached = false; }
    Aend = a; Bend = b;
    return reached;
  }
  // a forced run: deferred (its errors reach *dst later)
  // (the long ones are listed from the back of the array and run first: the forced kernel's tail is its largest rectangle)
  __device__ int32_t forced_errors(int32_t A0, int32_t A1, int32_t B0, int32_t B1, pgn::PnAln* dst) {
    const bool big = (A1 - A0) + (B1 - B0) > 1500;
    uint32_t at = 0;
    if ((threadIdx.x & 63) == 0) at = atomicAdd(big ? n_reqs + 6 : n_reqs, 1u);      // n_reqs[6]: the count of long runs
    at = (uint32_t)__builtin_amdgcn_readfirstlane((int)at);
    // The short list grows up from slot 0, the long one down from the last slot of the SAME array.  The walk starts at most one
    // alignment per MATCH (per cluster, or per match whose in-cluster target was not reached) and records at most one run per
    // alignment started, and the array has a slot per match slot of the launch (pg_anim.hip: req_cap): the two lists cannot meet.
    if (at < req_cap) { if ((threadIdx.x & 63) == 0) reqs[big ? req_cap - 1 - at : at] = PnForcedReq{A0, A1, B0, B1, unit, 0, dst}; }
    else overflow = 1;
    last_req = big ? req_cap - 1 - at : at;
    return 0;
  }
};
using PnWaveEngine = PnWaveEngineT<false>;
using PnWaveEngineDiag = PnWaveEngineT<true>;

// One forced run on whichever engine holds its band: the certified-band loop of pgn::ScalarEngine::align, in two kernels.  The
// NARROW kernel takes every run through the bands whose diagonal span fits a window of 256 / 512 diagonals (two thirds of all
// passes: every run's first one, and all of a close pair's) — it needs few registers and runs at five waves per SIMD; a run that
// asks for a wider band is handed, with that band, to the WIDE kernel (windows of 1024 / 2048 diagonals: 64 / 128 state registers,
// two waves per SIMD; beyond that the column strips of pn_align_regs<9>).
// Returns 0: certified (errors / w_used set); 1: continue at band w_next in the wide kernel; 2: failed (capacity).
template <bool WIDE, bool STRIPS = false>
__device__ int pn_forced_wave(const SeqView& R, const StrandView& Q, uint32_t* lds, uint32_t* glob, int32_t A0, int32_t A1, int32_t B0,
                              int32_t B1, int32_t w_start, int32_t& errors, int32_t& w_used, int32_t& w_next, uint32_t win_max = 2048u) {
  // win_max: the widest single-wave window this launch may use (2048; development / tests: smaller values push runs on to the next
  // kernel, so that the group engine and the strips see ordinary runs too)
  const unsigned m_o = pgn::FORCED_FORWARD_ALIGN;
  A0 = pn_uni(A0); A1 = pn_uni(A1); B0 = pn_uni(B0); B1 = pn_uni(B1);
  const int32_t N = A1 - A0 + 1, M = B1 - B0 + 1;
  const int32_t mn = N < M ? N : M, mx = N < M ? M : N;
  int32_t score = 0;
  for (int32_t w = pn_uni(w_start);;) {
    int32_t a = A1, b = B1;
    const bool whole = w >= mx;
    const int32_t widest = whole ? mn + 1 : ((mx - mn + 2 * w) >> 1) + 2, bw = whole ? -1 : w;
    bool reached = false, done = false;
    // diagonals the run spans (certified band: |M - N| + 2 w + 1; whole rectangle: N + M + 1) + the window's margins
    const int64_t span = (whole ? (int64_t)N + M + 1 : (int64_t)(mx - mn) + 2 * (int64_t)w + 1) + 5;
    if (!WIDE && (!pgd::diag_window_holds(span, 8) || win_max < 128u)) { w_next = w; return 1; }
    const unsigned long long t0 = wall_clock64();
    const int cls = span <= 256 ? 0 : span <= 512 ? 1 : span <= 2048 ? 2 : 3;      // [23 + cls] ticks, [27 + cls] passes, by window (3: column strips)
    // the smallest window that is sure to hold the band (diag_window_holds: whole-lane placement costs up to DPL - 1 diagonals of
    // either margin): a lane computes DPL / 2 cells per step whether they are inside the band or not
#define PN_TRY_DIAG(DPL_, KSTAT_) \
    if (!done && 64u * DPL_ <= win_max && pgd::diag_window_holds(span, DPL_)) { a = A1; b = B1; done = pn_align_diag<DPL_>(R, Q, A0, a, B0, b, m_o, bw, errors, score, reached, nullptr, KSTAT_); }
    if (!WIDE) {
      PN_TRY_DIAG(2, 4) PN_TRY_DIAG(4, 4) PN_TRY_DIAG(6, 4) PN_TRY_DIAG(8, 4)      // (w = 28, where two thirds of all runs certify: 57 + |M - N| diagonals -> the 128-diagonal window, one cell per lane and step)
      if (!done) { w_next = w; return 1; }
    } else {
      PN_TRY_DIAG(8, 5) PN_TRY_DIAG(12, 5) PN_TRY_DIAG(16, 5) PN_TRY_DIAG(24, 6) PN_TRY_DIAG(32, 6)
#undef PN_TRY_DIAG
      if (done) {}
      else if (!STRIPS) { w_next = w; return 1; }      // beyond one wave's window: the group kernel (anim_postnuc_forced_huge_kernel)
      else if ((size_t)(N + 1) * 8 <= PN_GLOBAL_WORDS) {
        // column strips of 511 through the 9-set engine; the boundary columns ping-pong between the two halves of the wave's scratch
        done = true;
        uint32_t* buf[2] = {glob, glob + PN_GLOBAL_WORDS / 2};
        int k = 0;
        for (int32_t j0 = 0; j0 <= M && done; j0 += 511, ++k) {
          const int32_t j1 = j0 + 511 < M + 1 ? j0 + 511 : M + 1;
          const PnStrip st{j0, j1, j0 > 0 ? buf[(k + 1) & 1] : nullptr, j1 < M + 1 ? buf[k & 1] : nullptr};
          a = A1; b = B1;
          __syncthreads();      // the boundary column written by the strip before is complete (and past the vector L1)
          done = pn_align_regs<9>(R, Q, A0, a, B0, b, m_o, bw, errors, score, reached, &st);
        }
      }
      if (!done) { a = A1; b = B1; if (widest <= PN_LDS_CELLS) done = pn_align_wave<false>(R, Q, lds, A0, a, B0, b, m_o, bw, errors, score, reached); }
      if (!done) { a = A1; b = B1; done = pn_align_wave<true>(R, Q, glob, A0, a, B0, b, m_o, bw, errors, score, reached); }
    }
    pn_stat(23 + cls, (unsigned long long)wall_clock64() - t0); pn_stat(27 + cls, 1);
    if (!done) { if (!WIDE) { w_next = w; return 1; } return 2; }
    const int v = pgn::forced_verdict(reached, score, whole, N, M, w);
    if (v == 2) return 2;      // the corner stays unreachable: flagged on the unit, not counted
    if (v == 0) { w_used = bw; return 0; }
    w = pgn::forced_band_after(w, N, M, score);
  }
}

template <bool WIDE>
__device__ __forceinline__ void pn_forced_body(const RefDesc* __restrict__ refs, const UnitDesc* __restrict__ units, PnForcedReq* __restrict__ reqs,
                                               const uint32_t* __restrict__ n_reqs, uint32_t req_cap, uint32_t* __restrict__ cursor,
                                               int32_t* __restrict__ pn_n, uint32_t* __restrict__ gscratch, uint32_t* __restrict__ wide,
                                               uint32_t* __restrict__ n_wide, uint32_t* lds, uint32_t* s_i, uint32_t win_max,
                                               uint32_t* __restrict__ huge = nullptr, uint32_t* __restrict__ n_huge = nullptr) {
  const int lane = threadIdx.x & 63;
  pn_stats_begin();
  const uint32_t n_small = n_reqs[0] < req_cap ? n_reqs[0] : req_cap, n_big = n_reqs[6] < req_cap ? n_reqs[6] : req_cap;
  const uint32_t n_items = WIDE ? *n_wide : n_small + n_big;
  for (;;) {
    __syncthreads();
    if (lane == 0) *s_i = atomicAdd(cursor, 1u);
    __syncthreads();
    const uint32_t i = pn_uni(*s_i);
    if (i >= n_items) break;
    const uint32_t slot = WIDE ? pn_uni(wide[i]) : (i < n_big ? req_cap - 1 - i : i - n_big);      // long runs first
    const PnForcedReq q = reqs[slot];
    const unsigned long long t0 = wall_clock64();
    const UnitDesc U = units[q.unit];
    const RefDesc Rd = refs[U.ref];
    int32_t err = 0, w_used = 0, w_next = 0;
    const int st = pn_forced_wave<WIDE>(SeqView{Rd.codes, Rd.mask, Rd.len}, StrandView{SeqView{U.codes, U.mask, U.len}, U.strand}, lds,
                                        WIDE ? gscratch + (size_t)blockIdx.x * PN_GLOBAL_WORDS : nullptr, q.A0, q.A1, q.B0, q.B1,
                                        WIDE ? q.w : pgn::FORCED_BAND_FIRST, err, w_used, w_next, win_max);
    if (lane == 0) {
      if (st == 1) { reqs[slot].w = w_next; if (WIDE) huge[atomicAdd(n_huge, 1u)] = slot; else wide[atomicAdd(n_wide, 1u)] = slot; }      // (at most one entry per request and list: the lists have req_cap slots)
      else {
        reqs[slot].w = w_used;      // (read by the traceback pass only)
        if (st == 2) { const int32_t v = pn_n[q.unit]; if (v >= 0) pn_n[q.unit] = -1 - v; }      // capacity: flagged on the unit
        else if (err) atomicAdd(&q.dst->errors, err);
      }
    }
    pn_stat_item(17, t0, (unsigned long long)((q.A1 - q.A0) + (q.B1 - q.B0)));
  }
  pn_stats_flush();
}
__global__ __launch_bounds__(64) void anim_postnuc_forced_kernel(const RefDesc* __restrict__ refs, const UnitDesc* __restrict__ units,
                                                                 PnForcedReq* __restrict__ reqs, const uint32_t* __restrict__ n_reqs,
                                                                 uint32_t req_cap, uint32_t* __restrict__ cursor, int32_t* __restrict__ pn_n,
                                                                 uint32_t* __restrict__ wide, uint32_t* __restrict__ n_wide, uint32_t win_max) {
  __shared__ uint32_t s_i;
  pn_forced_body<false>(refs, units, reqs, n_reqs, req_cap, cursor, pn_n, nullptr, wide, n_wide, nullptr, &s_i, win_max);
}
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3))) void anim_postnuc_forced_wide_kernel(
    const RefDesc* __restrict__ refs, const UnitDesc* __restrict__ units, PnForcedReq* __restrict__ reqs, const uint32_t* __restrict__ n_reqs,
    uint32_t req_cap, uint32_t* __restrict__ cursor, int32_t* __restrict__ pn_n, uint32_t* __restrict__ gscratch, uint32_t* __restrict__ wide,
    uint32_t* __restrict__ n_wide, uint32_t* __restrict__ huge, uint32_t* __restrict__ n_huge, uint32_t win_max) {
  __shared__ uint32_t lds[3 * 4 * PN_LDS_CELLS];
  __shared__ uint32_t s_i;
  pn_forced_body<true>(refs, units, reqs, n_reqs, req_cap, cursor, pn_n, gscratch, wide, n_wide, lds, &s_i, win_max, huge, n_huge);
}

// The runs whose certified band spans more than 2048 diagonals: one WORKGROUP of PN_HUGE_WAVES waves per run (pga_postnuc_diag.inc,
// pn_forced_diag_group: 3072 ... 8192 diagonals).  What even that cannot hold (the whole rectangle of a 10 000 x 10 000 run: never
// seen certified that late) is handed on to anim_postnuc_forced_strips_kernel (the column strips of the round-3 engine inside this
// kernel cost it 256 VGPRs and 283 spilled SGPRs; alone the group engine needs 242 — still two waves per SIMD: a third would
// spill 112 registers).  group_max: the widest band the group takes (8184; development / tests: 0 sends every run to the strips).
constexpr int PN_HUGE_WAVES = 4;
__global__ __launch_bounds__(64 * PN_HUGE_WAVES) __attribute__((amdgpu_waves_per_eu(2, 2))) void anim_postnuc_forced_huge_kernel(
    const RefDesc* __restrict__ refs, const UnitDesc* __restrict__ units, PnForcedReq* __restrict__ reqs, uint32_t* __restrict__ cursor,
    int32_t* __restrict__ pn_n, const uint32_t* __restrict__ huge, const uint32_t* __restrict__ n_huge, uint32_t* __restrict__ strips,
    uint32_t* __restrict__ n_strips, uint32_t group_max) {
  __shared__ uint32_t xch[2 * PN_HUGE_WAVES * 4 + 4];
  __shared__ uint32_t s_i;
  const int wave = (int)(threadIdx.x >> 6);
  pn_stats_begin();
  const uint32_t n_items = *n_huge;
  for (;;) {
    __syncthreads();
    if (threadIdx.x == 0) s_i = atomicAdd(cursor, 1u);
    __syncthreads();
    const uint32_t i = pn_uni(s_i);
    if (i >= n_items) break;
    const uint32_t slot = pn_uni(huge[i]);
    const PnForcedReq q = reqs[slot];
    const unsigned long long t0 = wall_clock64();
    const UnitDesc U = units[q.unit];
    const RefDesc Rd = refs[U.ref];
    const SeqView R{Rd.codes, Rd.mask, Rd.len};
    const StrandView Q{SeqView{U.codes, U.mask, U.len}, U.strand};
    const int32_t A0 = pn_uni(q.A0), A1 = pn_uni(q.A1), B0 = pn_uni(q.B0), B1 = pn_uni(q.B1);
    const int32_t N = A1 - A0 + 1, M = B1 - B0 + 1, mn = N < M ? N : M, mx = N < M ? M : N;
    int32_t errors = 0, score = 0, w_used = 0;
    bool handed = false, failed = false;
    for (int32_t w = pn_uni(q.w);;) {
      const bool whole = w >= mx;
      const int32_t bw = whole ? -1 : w;
      const int64_t span = (whole ? (int64_t)N + M + 1 : (int64_t)(mx - mn) + 2 * (int64_t)w + 1) + 5;
      bool done = false;
      const unsigned long long t1 = wall_clock64();
      if (span <= (int64_t)group_max) {
        if (span <= 64 * 12 * PN_HUGE_WAVES - 8) done = pn_forced_diag_group<PN_HUGE_WAVES, 12>(R, Q, A0, A1, B0, B1, bw, xch, errors, score, 7);
        else if (span <= 64 * 16 * PN_HUGE_WAVES - 8) done = pn_forced_diag_group<PN_HUGE_WAVES, 16>(R, Q, A0, A1, B0, B1, bw, xch, errors, score, 7);
        else if (span <= 64 * 24 * PN_HUGE_WAVES - 8) done = pn_forced_diag_group<PN_HUGE_WAVES, 24>(R, Q, A0, A1, B0, B1, bw, xch, errors, score, 7);
        else if (span <= 64 * 32 * PN_HUGE_WAVES - 8) done = pn_forced_diag_group<PN_HUGE_WAVES, 32>(R, Q, A0, A1, B0, B1, bw, xch, errors, score, 7);
      }
      if (!done) {      // (uniform: `done` is the same in every wave) on to the strips, from this band on
        if (threadIdx.x == 0) { reqs[slot].w = w; strips[atomicAdd(n_strips, 1u)] = slot; }
        handed = true;
        break;
      }
      if (wave == 0) { pn_stat(26, (unsigned long long)wall_clock64() - t1); pn_stat(30, 1); }
      const int v = pgn::forced_verdict(true, score, whole, N, M, w);
      if (v == 2) { failed = true; break; }
      if (v == 0) { w_used = bw; break; }
      w = pgn::forced_band_after(w, N, M, score);
    }
    if (threadIdx.x == 0 && !handed) {
      reqs[slot].w = w_used;
      if (failed) { const int32_t v = pn_n[q.unit]; if (v >= 0) pn_n[q.unit] = -1 - v; }      // the corner stays unreachable: flagged on the unit
      else if (errors) atomicAdd(&q.dst->errors, errors);
    }
    if (wave == 0) pn_stat_item(17, t0, (unsigned long long)((q.A1 - q.A0) + (q.B1 - q.B0)));
  }
  pn_stats_flush();
}
// The last resort: one wave per run on the column strips of the round-3 engine (and its LDS / global-memory forms behind them).
__global__ __launch_bounds__(64) void anim_postnuc_forced_strips_kernel(const RefDesc* __restrict__ refs, const UnitDesc* __restrict__ units,
                                                                        PnForcedReq* __restrict__ reqs, uint32_t* __restrict__ cursor,
                                                                        int32_t* __restrict__ pn_n, uint32_t* __restrict__ gscratch,
                                                                        const uint32_t* __restrict__ strips, const uint32_t* __restrict__ n_strips) {
  __shared__ uint32_t lds[3 * 4 * PN_LDS_CELLS];
  __shared__ uint32_t s_i;
  const int lane = threadIdx.x & 63;
  pn_stats_begin();
  const uint32_t n_items = *n_strips;
  for (;;) {
    __syncthreads();
    if (lane == 0) s_i = atomicAdd(cursor, 1u);
    __syncthreads();
    const uint32_t i = pn_uni(s_i);
    if (i >= n_items) break;
    const uint32_t slot = pn_uni(strips[i]);
    const PnForcedReq q = reqs[slot];
    const unsigned long long t0 = wall_clock64();
    const UnitDesc U = units[q.unit];
    const RefDesc Rd = refs[U.ref];
    int32_t err = 0, w_used = 0, w_next = 0;
    const int st = pn_forced_wave<true, true>(SeqView{Rd.codes, Rd.mask, Rd.len}, StrandView{SeqView{U.codes, U.mask, U.len}, U.strand}, lds,
                                              gscratch + (size_t)blockIdx.x * PN_GLOBAL_WORDS, q.A0, q.A1, q.B0, q.B1, q.w, err, w_used, w_next, 0u);
    if (lane == 0) {
      reqs[slot].w = w_used;
      if (st != 0) { const int32_t v = pn_n[q.unit]; if (v >= 0) pn_n[q.unit] = -1 - v; }      // capacity: flagged on the unit
      else if (err) atomicAdd(&q.dst->errors, err);
    }
    pn_stat_item(17, t0, (unsigned long long)((q.A1 - q.A0) + (q.B1 - q.B0)));
  }
  pn_stats_flush();
}

// ---- small match-to-match gaps, one LANE each -------------------------------------------------------------------------------
// A gap whose rectangle has N, M <= PN_SMALL (both boundary bases included) cannot be trimmed and cannot break: every cell is
// reachable by min(i, j) diagonal steps and one gap, so it scores at least -7 max(i, j) - 3 >= -416, the best score is at most
// 3 min(N, M) <= 177, and the two stay within MAX_DIFF = 600 of each other; N + M <= 118 < BREAK_LEN.  MUMmer's band is then the
// whole rectangle and its target is always reached, so the alignment is the plain global one: filled here row by row, one gap
// per lane, the previous row's INSERT / best words in registers (statically indexed columns), same cell arithmetic as the wave
// engines (pgn::diag_cell's two-candidate gap states, state-labelled words, riding errors).  ~27 VALU per cell for 64 gaps at
// once, against ~250 per anti-diagonal for ONE gap in the wave engine: at 88 % identity a cluster's matches sit 10-60 bases apart.
constexpr int PN_SMALL = 59;
struct PnGapTask { uint32_t unit, slot; };      // slot: the match slot (moff-relative) of the gap's first match

template <int C>   // columns 0 .. C (C >= M)
__global__ __launch_bounds__(64) void anim_postnuc_gaplane_kernel(const RefDesc* __restrict__ refs, const UnitDesc* __restrict__ units, ClusterOut O,
                                                                  const PnGapTask* __restrict__ tasks, const uint32_t* __restrict__ n_tasks,
                                                                  pgn::PnGap* __restrict__ gaps) {
  using namespace pgn;
  const uint32_t n = *n_tasks;
  for (uint32_t t0 = blockIdx.x * 64u; t0 < n; t0 += gridDim.x * 64u) {
    const uint32_t t = t0 + (threadIdx.x & 63);
    const bool live = t < n;
    const PnGapTask T = tasks[live ? t : 0];
    const UnitDesc U = units[T.unit];
    const RefDesc Rd = refs[U.ref];
    const size_t off = O.moff[T.unit];
    const Match a = O.cm[off + T.slot], b = O.cm[off + T.slot + 1];
    const int32_t A0 = a.r + a.len - 1, B0 = a.q + a.len - 1;           // rows 1 .. N are A0 .., columns 1 .. M are B0 ..
    const int32_t N = live ? b.r - A0 + 1 : 0, M = live ? b.q - B0 + 1 : 0;
    const StrandView Q{SeqView{U.codes, U.mask, U.len}, U.strand};
    uint64_t aw[2], bw[2]; uint32_t ak[2], bk[2];
    packed_window(Rd.codes, Rd.mask, Rd.len, A0, aw[0], ak[0]);
    packed_window(Rd.codes, Rd.mask, Rd.len, (int64_t)A0 + 32, aw[1], ak[1]);
    strand_window(Q, B0, bw[0], bk[0]);
    strand_window(Q, (int64_t)B0 + 32, bw[1], bk[1]);
    // row 0: the origin and the DELETE run to its right
    uint32_t X[C + 1], I[C + 1];
    X[0] = w_make(0, 0, ST_MATCH); I[0] = 0u;
#pragma unroll
    for (int j = 1; j <= C; ++j) {
      const uint32_t d = j == 1 ? w_gap(X[0], OPEN_GAP_SCORE) : w_gap(X[j - 1], CONT_GAP_SCORE);
      X[j] = w_relabel(d, ST_DELETE); I[j] = 0u;
    }
    uint32_t ans = 0u;
    const int32_t nmax = (int32_t)wave_max_u32((uint32_t)N);
    // the B columns as words of 16 bases and their clean bits spread over the 2-bit fields (once per gap): a row's match bits for ALL
    // columns are then one xor / shift / or / and per word — per cell a sign-extended bit extract is left, where the base compare,
    // the clean test and their combination (lane masks: scalar-unit work) cost eight instructions (round 6)
    constexpr int NWORD = (C + 15) / 16;
    uint32_t bword[NWORD], bclean[NWORD];
#pragma unroll
    for (int h = 0; h < NWORD; ++h) {
      bword[h] = (uint32_t)(bw[h / 2] >> (32 * (h & 1)));
      bclean[h] = pgd::spread16(bk[h / 2] >> (16 * (h & 1)));
    }
    for (int32_t i = 1; i <= nmax; ++i) {
      const uint32_t abase = (uint32_t)((i <= 32 ? aw[0] >> (2 * (i - 1)) : aw[1] >> (2 * (i - 33))) & 3u);
      const uint32_t aclean = 0u - ((i <= 32 ? ak[0] >> (i - 1) : ak[1] >> (i - 33)) & 1u);      // all ones: the row's base is a clean one
      const uint32_t arep = abase * 0x55555555u;
      uint32_t eqw[NWORD];      // bit 2 t of word h: column 16 h + t + 1 matches this row
#pragma unroll
      for (int h = 0; h < NWORD; ++h) { const uint32_t x = bword[h] ^ arep; eqw[h] = ~(x | (x >> 1)) & (bclean[h] & aclean); }
      // column 0: only the INSERT run from above
      uint32_t G = X[0];
      {
        const uint32_t ic = w_gap(I[0], CONT_GAP_SCORE), ix = w_gap(X[0], OPEN_GAP_SCORE);
        I[0] = w_relabel(ic > ix ? ic : ix, ST_INSERT); X[0] = I[0];
      }
      uint32_t Dl = 0u, Xl = X[0], rowans = M == 0 ? X[0] : 0u;
#pragma unroll
      for (int j = 1; j <= C; ++j) {
        const uint32_t up_x = X[j];
        const uint32_t dc = w_gap(Dl, CONT_GAP_SCORE), dx = w_gap(Xl, OPEN_GAP_SCORE);
        const uint32_t ic = w_gap(I[j], CONT_GAP_SCORE), ix = w_gap(up_x, OPEN_GAP_SCORE);
        const uint32_t d = w_relabel(dc > dx ? dc : dx, ST_DELETE), ins = w_relabel(ic > ix ? ic : ix, ST_INSERT);
        const uint32_t m = w_relabel(w_step_mask(G, w_bit_mask(eqw[(j - 1) / 16], 2 * ((j - 1) % 16))), ST_MATCH);
        const uint32_t x = w_max3(d, ins, m);
        G = up_x; I[j] = ins; X[j] = x; Dl = d; Xl = x;
        rowans = j == M ? x : rowans;
      }
      ans = i == N ? rowans : ans;
    }
    if (live) gaps[off + T.slot] = PnGap{b.r, b.q, (int32_t)w_errors(ans), 1};
  }
}

__device__ __forceinline__ bool pn_gap_is_small(const Match& a, const Match& b) {
  const int32_t N = b.r - (a.r + a.len - 1) + 1, M = b.q - (a.q + a.len - 1) + 1;
  return N >= 1 && M >= 1 && N <= PN_SMALL && M <= PN_SMALL;
}
// the small gaps of every chain of the work list, by size class (0: N, M <= 16; 1: <= 32; 2: <= PN_SMALL): one thread per chain
__global__ __launch_bounds__(256) void anim_postnuc_gaplist_kernel(const UnitDesc* __restrict__ units, ClusterOut O, const uint2* __restrict__ wl,
                                                                   uint32_t n_wl, PnGapTask* __restrict__ tasks, size_t cap, uint32_t* __restrict__ n_tasks) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const bool valid = i < n_wl;
  const int lane = threadIdx.x & 63;
  size_t off = 0;
  Chain ch{};
  ch.count = 0;
  uint32_t u = 0;
  if (valid) { u = wl[i].x; off = O.moff[u]; ch = O.chains[off + (int32_t)wl[i].y]; }
  const Match* mm = O.cm + off + ch.first;
  // slots by class: counted per thread, one atomic per wave and class (one per gap serialises ~10^8 atomics on three addresses)
  uint32_t cnt[4] = {0u, 0u, 0u, 0u};
  for (int m = 0; m + 1 < ch.count; ++m) {
    const Match a = mm[m], b = mm[m + 1];
    if (!pn_gap_is_small(a, b)) { cnt[3] += 1u; continue; }
    const int32_t N = b.r - (a.r + a.len - 1) + 1, M = b.q - (a.q + a.len - 1) + 1, mx = N > M ? N : M;
    cnt[mx <= 16 ? 0 : mx <= 32 ? 1 : 2] += 1u;
  }
  uint32_t at[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    uint32_t incl = cnt[c];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)incl, d, 64); if (lane >= d) incl += t; }
    const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);
    uint32_t base = 0;
    if (lane == 63 && total) base = atomicAdd(&n_tasks[c < 3 ? c : 7], total);      // (n_tasks = cursor + 4; the wave-engine list's count sits at cursor[11])
    base = (uint32_t)__shfl((int)base, 63, 64);
    at[c] = base + incl - cnt[c];
  }
  for (int m = 0; m + 1 < ch.count; ++m) {
    const Match a = mm[m], b = mm[m + 1];
    const int32_t N = b.r - (a.r + a.len - 1) + 1, M = b.q - (a.q + a.len - 1) + 1, mx = N > M ? N : M;
    const int cls = !pn_gap_is_small(a, b) ? 3 : mx <= 16 ? 0 : mx <= 32 ? 1 : 2;
    const uint32_t slot = cls == 0 ? at[0]++ : cls == 1 ? at[1]++ : cls == 2 ? at[2]++ : at[3]++;
    if (slot < cap) tasks[(size_t)cls * cap + slot] = PnGapTask{u, (uint32_t)(ch.first + m)};
  }
}

// The match-to-match alignments of every cluster, one wave per (unit, chain) of the work list: independent of everything else
// (pg_nucmer_core.h, postnuc_unit), so they run here, spread over the whole GPU, instead of inside their units' sequential walks
// — three quarters of all trimmed-search anti-diagonals of a divergent job are these, ~15 per cluster, ~120 steps each.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void anim_postnuc_gapbig_kernel(const RefDesc* __restrict__ refs, const UnitDesc* __restrict__ units, ClusterOut O,
                                                                 uint32_t* __restrict__ cursor, pgn::PnGap* __restrict__ gaps,
                                                                 const PnGapTask* __restrict__ big, const uint32_t* __restrict__ n_big) {
  // the gaps the lane kernels did not take, from anim_postnuc_gaplist_kernel's fourth list: one gap per turn.  (Walking the
  // chains in anim_postnuc_gap_kernel — two dependent match loads per gap just to find that the lanes have it — took 0.54 s per
  // C4 launch, as long with the diagonal engine as with the column engine: 85 % of a cluster's gaps are small.)
  __shared__ uint32_t s_i;
  const int lane = threadIdx.x & 63;
  pn_stats_begin();
  const uint32_t n = *n_big;
  for (;;) {
    __syncthreads();
    if (lane == 0) s_i = atomicAdd(cursor, 8u);
    __syncthreads();
    const uint32_t i0 = pn_uni(s_i);
    if (i0 >= n) break;
    const uint32_t i1 = i0 + 8 < n ? i0 + 8 : n;
    for (uint32_t i = i0; i < i1; ++i) {
      const PnGapTask T = big[i];
      const uint32_t u = pn_uni(T.unit);
      const UnitDesc U = units[u];
      const RefDesc Rd = refs[U.ref];
      const size_t off = O.moff[u];
      const uint32_t slot = pn_uni(T.slot);
      const Match a = O.cm[off + slot], b = O.cm[off + slot + 1];
      PnWaveEngineDiag eng{SeqView{Rd.codes, Rd.mask, Rd.len}, StrandView{SeqView{U.codes, U.mask, U.len}, U.strand}, nullptr, nullptr, 0,
                           nullptr, nullptr, 0u, u, nullptr, nullptr};
      eng.kstat = 0;
      int32_t tA = b.r, tB = b.q, err = 0;
      const bool reached = eng.align(a.r + a.len - 1, tA, a.q + a.len - 1, tB, pgn::FORWARD_ALIGN, err);
      if (lane == 0) gaps[off + slot] = pgn::PnGap{tA, tB, err, eng.overflow ? -1 : reached ? 1 : 0};
    }
  }
  pn_stats_flush();
}
// (every gap of every chain on the wave engine: the form without the lane kernels, PYANI_ANIM_GAP_LANES=0 — tests hold the two against each other)
__global__ __launch_bounds__(64) void anim_postnuc_gap_kernel(const RefDesc* __restrict__ refs, const UnitDesc* __restrict__ units, ClusterOut O,
                                                              const uint2* __restrict__ wl, uint32_t n_wl, uint32_t* __restrict__ cursor,
                                                              pgn::PnGap* __restrict__ gaps, uint32_t* __restrict__ gscratch) {
  uint32_t* const lds = nullptr;      // no LDS engine here (a trimmed search never outgrows the register engine; if one does: global memory): the waves per CU are the registers'
  __shared__ uint32_t s_i;
  const int lane = threadIdx.x & 63;
  pn_stats_begin();
  for (;;) {
    __syncthreads();
    if (lane == 0) s_i = atomicAdd(cursor, 64u);     // 64 chains at a time: most have a handful of short gaps
    __syncthreads();
    const uint32_t i0 = pn_uni(s_i);
    if (i0 >= n_wl) break;
    const uint32_t i1 = i0 + 64 < n_wl ? i0 + 64 : n_wl;
    for (uint32_t i = i0; i < i1; ++i) {
      const uint32_t u = wl[i].x;
      const int32_t c = (int32_t)wl[i].y;
      const UnitDesc U = units[u];
      const RefDesc Rd = refs[U.ref];
      const size_t off = O.moff[u];
      const Chain ch = O.chains[off + c];
      if (ch.count < 2) continue;
      PnWaveEngine eng{SeqView{Rd.codes, Rd.mask, Rd.len}, StrandView{SeqView{U.codes, U.mask, U.len}, U.strand}, lds,
                       gscratch + (size_t)blockIdx.x * PN_GLOBAL_WORDS, 0, nullptr, nullptr, 0u, u, nullptr, nullptr};
      const Match* mm = O.cm + off + ch.first;
      for (int m = 0; m + 1 < ch.count; ++m) {
        const Match a = mm[m], b = mm[m + 1];
        int32_t tA = b.r, tB = b.q, err = 0;
        const bool reached = eng.align(a.r + a.len - 1, tA, a.q + a.len - 1, tB, pgn::FORWARD_ALIGN, err);
        if (lane == 0) gaps[off + ch.first + m] = pgn::PnGap{tA, tB, err, (reached && !eng.overflow) ? 1 : 0};
      }
    }
  }
  pn_stats_flush();
}

// The forward extension off every cluster's last match, one wave per (unit, cluster): pgn::postnuc_forward is a function of the
// unit's clusters alone, so — like the match-to-match alignments above — it does not have to wait for the unit's sequential walk.
// Between close genomes this is most of a unit's search work (a chain of fused clusters is one forward extension after the
// other, each up to 2 x 10 000 anti-diagonals long): inside the walk the longest unit of a launch alone took as long as the launch.
// wl[i] = (unit, k): k is taken as the position in the unit's `order` (both number the unit's clusters 0 .. n - 1).
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void anim_postnuc_fwd_kernel(const RefDesc* __restrict__ refs, const UnitDesc* __restrict__ units, ClusterOut O,
                                                              const uint2* __restrict__ wl, uint32_t n_wl, uint32_t* __restrict__ cursor,
                                                              pgn::PnFwd* __restrict__ fwd, uint32_t* __restrict__ gscratch) {
  __shared__ uint32_t s_i;
  const int lane = threadIdx.x & 63;
  pn_stats_begin();
  for (;;) {
    __syncthreads();
    if (lane == 0) s_i = atomicAdd(cursor, 4u);
    __syncthreads();
    const uint32_t i0 = pn_uni(s_i);
    if (i0 >= n_wl) break;
    const uint32_t i1 = i0 + 4 < n_wl ? i0 + 4 : n_wl;
    for (uint32_t i = i0; i < i1; ++i) {
      const uint32_t u = pn_uni(wl[i].x);
      const int k = (int)pn_uni(wl[i].y);
      const UnitDesc U = units[u];
      const RefDesc Rd = refs[U.ref];
      const size_t off = O.moff[u];
      const int n = O.n_chains[u];
      PnWaveEngineDiag eng{SeqView{Rd.codes, Rd.mask, Rd.len}, StrandView{SeqView{U.codes, U.mask, U.len}, U.strand}, nullptr, nullptr, 0,
                           nullptr, nullptr, 0u, u, nullptr, nullptr};
      eng.kstat = 1;
      const Chain* chains = O.chains + off;
      pgn::PnFwd f = pgn::postnuc_forward(eng, chains, O.cm + off, O.order + off, n, k,
                             [&](int c, int32_t& r_lo, int32_t& r_hi, int32_t& q_lo, int32_t& q_hi) { chain_bounds(Rd, U, chains[c], r_lo, r_hi, q_lo, q_hi); });
      if (eng.overflow) f.reached = -1;      // (the walk runs it again and flags the unit)
      if (lane == 0) fwd[off + k] = f;
    }
  }
  pn_stats_flush();
}

// ---- backward searches ahead of the walk ---------------------------------------------------------------------------------------
// What is left in a unit's walk once the match-to-match and forward alignments are hoisted: one backward search per alignment
// started, each waiting for the one before it (its target is an earlier alignment's END).  Between divergent genomes every one
// of them runs thousands of anti-diagonals (+0.3 per column never breaks), and the longest unit of a launch — 858 clusters,
// 2.4 s — was the launch's tail.  But the ENDS of alignments do not depend on backward searches (those move starts and merge
// alignments; an alignment merged into its target hands over exactly the end it would have had), so a DP-free rehearsal of the
// walk (pgn::PnRehearsal: every backward search answered "found nothing") predicts each search's arguments — all of them on the
// synthetic families, 98 % on the Caulobacter fixtures (host statement: tools/anim_debug, ANIM_BWD_AHEAD) — the searches then
// run one wave each, and the real walk takes a result only when its own arguments are the predicted ones.
__device__ __forceinline__ void pn_rehearse_body(const RefDesc* __restrict__ refs, const UnitDesc* __restrict__ units,
                                                                   uint32_t n_units, ClusterOut O, uint32_t* __restrict__ cursor,
                                                                   pgn::PnAln* __restrict__ pn, uint8_t* __restrict__ fused,
                                                                   uint32_t* __restrict__ gscratch, const pgn::PnGap* __restrict__ gaps,
                                                                   const pgn::PnFwd* __restrict__ fwd, const uint32_t* __restrict__ unit_order,
                                                                   pgn::PnBwd* __restrict__ bwd, uint32_t& s_u) {

  uint32_t* const lds = nullptr;      // (no LDS engine: see PnWaveEngineT::align)
  const int lane = threadIdx.x & 63;
  pn_stats_begin();
  for (;;) {
    __syncthreads();
    if (lane == 0) s_u = atomicAdd(cursor, 1u);
    __syncthreads();
    if (s_u >= n_units) break;
    const uint32_t u = pn_uni(unit_order[pn_uni(s_u)]);
    const UnitDesc U = units[u];
    const RefDesc Rd = refs[U.ref];
    const size_t off = O.moff[u];
    const int n = O.n_chains[u];
    if (n <= 0) continue;
    const int cap = (int)(O.moff[u + 1] - off);
    PnWaveEngine eng{SeqView{Rd.codes, Rd.mask, Rd.len}, StrandView{SeqView{U.codes, U.mask, U.len}, U.strand}, lds,
                     gscratch + (size_t)blockIdx.x * PN_GLOBAL_WORDS, 0, nullptr, nullptr, 0u, u, gaps + off, fwd + off};
    pgn::PnRehearsal<PnWaveEngine> dry{eng, bwd + off};
    const Chain* chains = O.chains + off;
    pgn::PnNoSync alone;      // (the rehearsal walks its strand by itself: a wrong guess costs time, never a result)
    (void)pgn::postnuc_unit(dry, chains, O.cm + off, O.order + off, n,
                            [&](int c, int32_t& r_lo, int32_t& r_hi, int32_t& q_lo, int32_t& q_hi) { chain_bounds(Rd, U, chains[c], r_lo, r_hi, q_lo, q_hi); },
                            fused + off, pn + off, cap, alone, U.strand);
  }
  pn_stats_flush();
}
__global__ __launch_bounds__(64) void anim_postnuc_rehearse_kernel(const RefDesc* __restrict__ refs, const UnitDesc* __restrict__ units, uint32_t n_units, ClusterOut O, uint32_t* __restrict__ cursor,
                                                                   pgn::PnAln* __restrict__ pn, uint8_t* __restrict__ fused, uint32_t* __restrict__ gscratch,
                                                                   const pgn::PnGap* __restrict__ gaps, const pgn::PnFwd* __restrict__ fwd,
                                                                   const uint32_t* __restrict__ unit_order, pgn::PnBwd* __restrict__ bwd) {
  __shared__ uint32_t s_u;
  pn_rehearse_body(refs, units, n_units, O, cursor, pn, fused, gscratch, gaps, fwd, unit_order, bwd, s_u);
}
// one wave per predicted search (wl[i] = (unit, position in the unit's order))
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void anim_postnuc_bwd_kernel(const RefDesc* __restrict__ refs, const UnitDesc* __restrict__ units, ClusterOut O,
                                                              const uint2* __restrict__ wl, uint32_t n_wl, uint32_t* __restrict__ cursor,
                                                              pgn::PnBwd* __restrict__ bwd, uint32_t* __restrict__ gscratch) {
  __shared__ uint32_t s_i;
  const int lane = threadIdx.x & 63;
  pn_stats_begin();
  for (;;) {
    __syncthreads();
    if (lane == 0) s_i = atomicAdd(cursor, 8u);
    __syncthreads();
    const uint32_t i0 = pn_uni(s_i);
    if (i0 >= n_wl) break;
    const uint32_t i1 = i0 + 8 < n_wl ? i0 + 8 : n_wl;
    for (uint32_t i = i0; i < i1; ++i) {
      const uint32_t u = pn_uni(wl[i].x);
      const int k = (int)pn_uni(wl[i].y);
      const size_t off = O.moff[u];
      pgn::PnBwd b = bwd[off + k];
      if (pn_uni(b.state) != 1) continue;
      const UnitDesc U = units[u];
      const RefDesc Rd = refs[U.ref];
      PnWaveEngineDiag eng{SeqView{Rd.codes, Rd.mask, Rd.len}, StrandView{SeqView{U.codes, U.mask, U.len}, U.strand}, nullptr, nullptr, 0,
                           nullptr, nullptr, 0u, u, nullptr, nullptr};
      eng.kstat = 2;
      int32_t a = b.tA, q = b.tB, err = 0;
      const bool reached = eng.align(b.sA, a, b.sB, q, b.m_o, err);
      if (eng.overflow) continue;      // (the walk searches itself and flags the unit)
      if (lane == 0) { b.rA = a; b.rB = q; b.reached = reached ? 1 : 0; b.state = 2; bwd[off + k] = b; }
    }
  }
  pn_stats_flush();
}

// ---- traceback pass (optional: pg_anim_alignments_batch with indel lists) ----------------------------------------------------
// Pieces of unit u live at pn_piece_base(moff[u], choff[u], u): at most 3 per match (the match, its alignment onwards, a forced
// run in front of it) + 4 per cluster + a few.
__host__ __device__ inline size_t pn_piece_base(size_t moff_u, uint32_t choff_u, uint32_t u) { return 3 * moff_u + 4 * (size_t)choff_u + 16 * (size_t)u; }
__host__ __device__ inline size_t pn_piece_cap(size_t matches_u, uint32_t chains_u) { return 3 * matches_u + 4 * (size_t)chains_u + 16; }

// One search / forced piece per THREAD: the scalar engine (pg_nucmer_core.h — the definition the wave engines follow cell for
// cell) repeats the call with its backpointer store, walks back from the finish cell and leaves the path, run-length coded, in the
// launch's output arena.  The host sized every job's slab from the wave engine's own bookkeeping of the call (cells computed,
// widest anti-diagonal) — the same band comes out, so the store is exact.  A traceback pass is bookkeeping for output files:
// 0.1-1 % of a grid's pairs are ever written, and a thread per piece keeps 10^5 of them in flight.
struct PnTraceJob {
  uint32_t unit, m_o;
  int32_t A0, B0, tA, tB, A1, B1;      // start, the target given to the engine, where it finished (forced: target = finish)
  int32_t band_w;                      // forced: the certified band (-1: whole rectangle); searches: -1
  uint32_t cap, dcap, rle_cap;         // cells per anti-diagonal, anti-diagonals (+ slack), path entries
  uint64_t bp_cap, slab;               // cells stored; byte offset of the job's slab in the arena
};
__global__ __launch_bounds__(64) void anim_trace_kernel(const RefDesc* __restrict__ refs, const UnitDesc* __restrict__ units,
                                                        const PnTraceJob* __restrict__ jobs, uint32_t n_jobs, uint8_t* __restrict__ arena,
                                                        uint32_t* __restrict__ out, unsigned long long out_cap, unsigned long long* __restrict__ out_cursor,
                                                        unsigned long long* __restrict__ out_off, int32_t* __restrict__ out_cnt) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n_jobs) return;
  const PnTraceJob J = jobs[i];
  const UnitDesc U = units[J.unit];
  const RefDesc Rd = refs[U.ref];
  const SeqView R{Rd.codes, Rd.mask, Rd.len};
  const StrandView Q{SeqView{U.codes, U.mask, U.len}, U.strand};
  pgn::Cell* d0 = reinterpret_cast<pgn::Cell*>(arena + J.slab);
  uint32_t* doff = reinterpret_cast<uint32_t*>(d0 + 3 * (size_t)J.cap);
  int32_t* dlo = reinterpret_cast<int32_t*>(doff + J.dcap);
  uint32_t* rle = reinterpret_cast<uint32_t*>(dlo + J.dcap);
  uint8_t* bp = reinterpret_cast<uint8_t*>(rle + J.rle_cap);
  pgn::ScalarEngine<SeqView, StrandView> eng{R, Q, d0, d0 + J.cap, d0 + 2 * (size_t)J.cap, (int32_t)J.cap};
  pgn::PnTrace tr{bp, J.bp_cap, doff, dlo, (int32_t)J.dcap, 0, 0, 0, 0};
  eng.trace = &tr;
  int32_t a = J.tA, b = J.tB, err = 0;
  eng.run(J.A0, a, J.B0, b, J.m_o, J.band_w, err);
  int32_t cnt = -1;
  if (!eng.overflow && !tr.overflow && a == J.A1 && b == J.B1) cnt = pgn::pn_trace_back(tr, rle, (int32_t)J.rle_cap);
  unsigned long long off = 0;
  if (cnt > 0) {
    off = atomicAdd(out_cursor, (unsigned long long)cnt);
    if (off + (unsigned long long)cnt <= out_cap) for (int32_t k = 0; k < cnt; ++k) out[off + k] = rle[k];
    else cnt = -2;
  }
  out_off[i] = off; out_cnt[i] = cnt;
}

// How the two walks of a pair (pgn::PnPairSync) reach each other on the GPU: the two waves of a workgroup.  Positions and log lengths
// live in LDS (sh[0 .. 1]: the waves' keys, sh[2 .. 3]: their log lengths); the logs and the alignments' birth keys are global
// memory, written by lane 0 with agent-scope stores and read past the vector L1.
struct PnWavePrim {
  volatile int32_t* sh;
  int me;
  __device__ int32_t ld(const int32_t* p) const { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ void st(int32_t* p, int32_t v) const { if ((threadIdx.x & 63) == 0) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  // The two waves share a CU (one workgroup): its vector L1 is write-through and the readers load past it (agent-scope atomic
  // loads), so a WORKGROUP-scope release — this wave's stores acknowledged — is all the log needs before its length is announced;
  // an agent-scope fence here (an L2 write-back per turn, 10^7 turns per launch) doubled the kernel's time.
  __device__ void publish_log(int32_t n_log) const {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if ((threadIdx.x & 63) == 0) sh[2 + me] = n_log;
  }
  __device__ void publish_key(int32_t key) const { if ((threadIdx.x & 63) == 0) sh[me] = key; }      // (LDS stores of a wave stay in order: the length before the key)
  __device__ int32_t other_key() const { const int32_t k = sh[1 - me]; __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); return pn_uni(k); }
  __device__ int32_t other_nlog() const { return pn_uni((int32_t)sh[3 - me]); }
  __device__ void pause() const { __builtin_amdgcn_s_sleep(8); }
};

// Persistent workgroups of TWO waves, one PAIR at a time from a shared cursor (pairs with the most clusters first: the launch ends
// with its short ones): wave s walks the pair's strand-s unit, and the two walks consult each other where MUMmer's single walk over
// both strands would have (pgn::PnPairSync).  pn[]: the unit's alignments in the slice of its matches (a unit has at most as many
// alignments as chains, and a chain has at least one match); pn_n[u]: how many (< 0: capacity).
__device__ __forceinline__ void pn_walk_body(const RefDesc* __restrict__ refs, const UnitDesc* __restrict__ units,
                                                           uint32_t n_pairs, ClusterOut O, uint32_t* __restrict__ cursor,
                                                           pgn::PnAln* __restrict__ pn, uint8_t* __restrict__ fused,
                                                           int32_t* __restrict__ pn_n, uint32_t* __restrict__ gscratch,
                                                           PnForcedReq* __restrict__ reqs, uint32_t* __restrict__ n_reqs, uint32_t req_cap,
                                                           const pgn::PnGap* __restrict__ gaps, const pgn::PnFwd* __restrict__ fwd,
                                                           const uint32_t* __restrict__ pair_order, pgn::PnPiece* __restrict__ pieces,
                                                           uint32_t* __restrict__ n_pieces, const uint32_t* __restrict__ choff,
                                                           const pgn::PnBwd* __restrict__ bwd, pgn::PnTurn* __restrict__ tlog,
                                                           int32_t* __restrict__ born, uint32_t& s_p, int32_t* s_sync) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  pn_stats_begin();
  for (;;) {
    __syncthreads();
    if (threadIdx.x == 0) { s_p = atomicAdd(cursor, 1u); s_sync[0] = -1; s_sync[1] = -1; s_sync[2] = 0; s_sync[3] = 0; }
    __syncthreads();
    if (s_p >= n_pairs) break;
    const uint32_t u = 2u * pn_uni(pair_order[pn_uni(s_p)]) + (uint32_t)wave;      // (units are laid out pair-major: strand s of pair p is unit 2 p + s)
    const unsigned long long t0 = wall_clock64();
    const UnitDesc U = units[u];
    const RefDesc Rd = refs[U.ref];
    const size_t off = O.moff[u];
    const int n = O.n_chains[u];
    int na = 0;
    if (n > 0) {
      const int cap = (int)(O.moff[u + 1] - off);
      PnWaveEngine eng{SeqView{Rd.codes, Rd.mask, Rd.len}, StrandView{SeqView{U.codes, U.mask, U.len}, U.strand}, nullptr,
                       gscratch + ((size_t)blockIdx.x * 2 + wave) * PN_GLOBAL_WORDS, 0, reqs, n_reqs, req_cap, u, gaps ? gaps + off : nullptr,
                       fwd ? fwd + off : nullptr};
      if (pieces) { eng.pieces = pieces + pn_piece_base(off, choff[u], u); eng.piece_cap = (int32_t)pn_piece_cap((size_t)cap, (uint32_t)n); }
      if (bwd) eng.bwd = bwd + off;
      eng.kstat = 3;
      const Chain* chains = O.chains + off;
      pgn::PnPairSync<PnWavePrim> sync{PnWavePrim{s_sync, wave}, tlog + off, tlog + O.moff[u ^ 1u], born + off};
      na = pgn::postnuc_unit(eng, chains, O.cm + off, O.order + off, n,
                             [&](int c, int32_t& r_lo, int32_t& r_hi, int32_t& q_lo, int32_t& q_hi) { chain_bounds(Rd, U, chains[c], r_lo, r_hi, q_lo, q_hi); },
                             fused + off, pn + off, cap, sync, U.strand);
      if (eng.overflow && na >= 0) na = -1 - na;
      if (pieces && lane == 0) n_pieces[u] = (uint32_t)eng.n_pieces;
      pn_stat(31, (unsigned long long)sync.asked);      // [31] shadow tests that needed the synteny's current alignment (a containing alignment existed)
    } else {
      if (lane == 0) s_sync[wave] = pgn::PN_KEY_DONE;      // (a strand without clusters: the other walk never waits for it)
      if (pieces && lane == 0) n_pieces[u] = 0u;
    }
    pn_stat(11, 1); pn_stat(12, (unsigned long long)(n > 0 ? n : 0));
    if (n > 0) pn_stat_item(13, t0, (unsigned long long)n);
    if (lane == 0) pn_n[u] = na;
  }
  pn_stats_flush();
}

// The walks are latency-bound (dependent loads per cluster, one wave per strand).  The compiler gives the body 219 VGPRs (two waves
// per SIMD); capped at 128 (amdgpu_waves_per_eu(4, 4): three waves per SIMD reached, ~500 B of scratch per lane for the spilled
// state) the kernel was SLOWER on MI355X — 291 vs 214 ms on the heaviest C4 tile (profiles/r05_walk_register_cap.txt): the span
// of a launch is its longest unit, not its occupancy.
__global__ __launch_bounds__(128) void anim_postnuc_kernel(const RefDesc* __restrict__ refs, const UnitDesc* __restrict__ units, uint32_t n_pairs, ClusterOut O, uint32_t* __restrict__ cursor,
                                                           pgn::PnAln* __restrict__ pn, uint8_t* __restrict__ fused, int32_t* __restrict__ pn_n, uint32_t* __restrict__ gscratch,
                                                           PnForcedReq* __restrict__ reqs, uint32_t* __restrict__ n_reqs, uint32_t req_cap,
                                                           const pgn::PnGap* __restrict__ gaps, const pgn::PnFwd* __restrict__ fwd,
                                                           const uint32_t* __restrict__ pair_order, pgn::PnPiece* __restrict__ pieces,
                                                           uint32_t* __restrict__ n_pieces, const uint32_t* __restrict__ choff,
                                                           const pgn::PnBwd* __restrict__ bwd, pgn::PnTurn* __restrict__ tlog, int32_t* __restrict__ born) {
  __shared__ uint32_t s_p;
  __shared__ int32_t s_sync[4];
  pn_walk_body(refs, units, n_pairs, O, cursor, pn, fused, pn_n, gscratch, reqs, n_reqs, req_cap, gaps, fwd, pair_order, pieces, n_pieces, choff, bwd, tlog, born, s_p, s_sync);
}

// ---- development: directed searches (pg_anim_searches) ------------------------------------------------------------------------
// Caller-chosen trimmed searches of ONE (reference, query strand), one wave per search, on the product's own engines: nothing here
// but the cursor loop of the pre-pass kernels and the calls the product makes.  engine (wave-uniform):
//   PREPASS      PnWaveEngineDiag::align as the gap-big / forward / backward kernels call it (the host launches one list per kernel,
//                with that kernel's chunk size); its overflow comes back as held = 0
//   WALK         PnWaveEngine::align with the wave's slice of global scratch: the ladder 256 -> 512 -> global memory as the walk runs it
//   RUNG_*       pn_align_diag<4> / pn_align_diag<8> / pn_align_wave<true> called directly, held = their own return value
// A search that was not held leaves zeros.  (LANES does not come here: the host builds chains and runs launch_gaps.)
enum PnSearchEngine : int { PN_SEARCH_PREPASS = 0, PN_SEARCH_WALK = 1, PN_SEARCH_RUNG_256 = 2, PN_SEARCH_RUNG_512 = 3, PN_SEARCH_RUNG_GLOBAL = 4, PN_SEARCH_LANES = 5 };
struct PnSearchReq { int32_t A0, B0, tA, tB; uint32_t m_o; };
struct PnSearchOut { int32_t eA, eB, errors, reached, held; };
__global__ __launch_bounds__(64) void anim_postnuc_searches_kernel(const RefDesc* __restrict__ refs, const UnitDesc* __restrict__ units,
                                                                   const PnSearchReq* __restrict__ reqs, const uint32_t* __restrict__ list, uint32_t n,
                                                                   uint32_t chunk, int engine_, uint32_t* __restrict__ cursor,
                                                                   PnSearchOut* __restrict__ out, uint32_t* __restrict__ gscratch) {
  __shared__ uint32_t s_i;
  const int lane = threadIdx.x & 63;
  const int engine = pn_uni((int32_t)engine_);
  pn_stats_begin();
  const UnitDesc U = units[0];
  const RefDesc Rd = refs[U.ref];
  const SeqView R{Rd.codes, Rd.mask, Rd.len};
  const StrandView Q{SeqView{U.codes, U.mask, U.len}, U.strand};
  uint32_t* const glob = gscratch ? gscratch + (size_t)blockIdx.x * PN_GLOBAL_WORDS : nullptr;
  for (;;) {
    __syncthreads();
    if (lane == 0) s_i = atomicAdd(cursor, chunk);
    __syncthreads();
    const uint32_t i0 = pn_uni(s_i);
    if (i0 >= n) break;
    const uint32_t i1 = i0 + chunk < n ? i0 + chunk : n;
    for (uint32_t i = i0; i < i1; ++i) {
      const uint32_t k = pn_uni(list[i]);
      const PnSearchReq S = reqs[k];
      const int32_t A0 = pn_uni(S.A0), B0 = pn_uni(S.B0);
      const unsigned m_o = pn_uni(S.m_o);
      __builtin_assume(m_o < 16u);      // (checked by the host: direction, search and best-cell bits, as every caller of the engines passes — the engines' own code stays the batch's, instruction for instruction)
      int32_t a = pn_uni(S.tA), b = pn_uni(S.tB), err = 0, score = 0;
      bool reached = false, held = false;
      if (engine == PN_SEARCH_PREPASS) {
        PnWaveEngineDiag eng{R, Q, nullptr, nullptr, 0, nullptr, nullptr, 0u, 0u, nullptr, nullptr};
        reached = eng.align(A0, a, B0, b, m_o, err);
        held = !eng.overflow;
      } else if (engine == PN_SEARCH_WALK) {
        PnWaveEngine eng{R, Q, nullptr, glob, 0, nullptr, nullptr, 0u, 0u, nullptr, nullptr};
        reached = eng.align(A0, a, B0, b, m_o, err);
        held = !eng.overflow;
      } else if (engine == PN_SEARCH_RUNG_256) held = pn_align_diag<4>(R, Q, A0, a, B0, b, m_o, -1, err, score, reached);
      else if (engine == PN_SEARCH_RUNG_512) held = pn_align_diag<8>(R, Q, A0, a, B0, b, m_o, -1, err, score, reached);
      else if (engine == PN_SEARCH_RUNG_GLOBAL) held = pn_align_wave<true>(R, Q, glob, A0, a, B0, b, m_o, -1, err, score, reached);
      if (lane == 0) out[k] = held ? PnSearchOut{a, b, err, reached ? 1 : 0, 1} : PnSearchOut{0, 0, 0, 0, 0};
    }
  }
  pn_stats_flush();
}
