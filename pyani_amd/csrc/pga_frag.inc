// pga_frag.inc — part of pg_anim.hip (included inside its anonymous namespace; not a translation unit of its own):
// fragment mode (ANIb, BASELINE.json configs[4]): the 1020-nt fragments of a query genome against a subject genome, best
// local alignment per fragment in BLAST's table columns (pg_anib_core.h has the scalar statement and what it restates of
// blastn; the CPU checker is a host build of it), then parse_blast_tab's reduction per ordered pair (pyani/anib.py:641-665).
//
//   seeds     the ANIm seeding stage as it is (anim_seed_kernel -> anim_hit_kernel -> anim_scatter_kernel) with the match
//             threshold lowered from 20 to 16: per (pair, query strand) unit the maximal exact matches that contain a sampled
//             16-mer of the query strand.  Subject = the LDS-table role, fragmented genome = the streamed role.
//   F1 anib_bucket_kernel   one workgroup per unit: matches clipped to the fragments they overlap, counting-sorted by fragment
//             (the counters of a genome's fragments live in LDS up to 15 872 of them, in HBM beyond); per-fragment offsets + the clipped seeds
//   F2 anib_frag_kernel     one WAVE per (pair, fragment): up to two anchors per strand (pga::frag_pick_anchors), each grown
//             into an HSP by two X-drop extensions.  The DP band (256 diagonals, following the alignment) lives in registers, four
//             diagonals per lane; a cell reads only diagonals of the other parity, so an anti-diagonal is updated in place
//             with four lane shuffles per step.  Rows (<= 4) are written best score first.
//   F3 anib_reduce_pairs_kernel   one thread per pair: first row per fragment that passes coverage > 0.7 and identity > 0.3,
//             sums and the mean of pident (printed to 3 decimals as BLAST does) in fragment order.

struct FragPair {            // one per pair of the batch
  const int32_t* frag_pos;   // stream position of every fragment of the query genome (n_frags entries)
  const int32_t* frag_len;
  const int32_t* rec_frag0;  // first fragment of every record (n_rec entries)
  int32_t n_frags;
  uint32_t slot0;            // first (pair, fragment) slot of the pair
};

constexpr int FRAG_MAX_FRAGS = (int)PG_FRAG_MAX_FRAGS;    // fragments per genome whose counters fit LDS (62 KiB): genomes up to 16.1 Mb at 1020 nt; larger ones count in HBM
constexpr int FRAG_ROWS = FRAG_KEEP_ROWS;      // rows kept per (pair, fragment): the best-scoring ones

struct FragRow { int32_t frag, length, mismatch, gaps, nident, qlen, qstart, qend, sstart, send, srec, score; };   // = pg_anib_row

// forward interval of a match in the query genome and the fragments it overlaps
__device__ __forceinline__ void frag_span(const UnitDesc& U, const FragPair& P, const Match& m, int32_t fragsize, int32_t& a, int32_t& b,
                                          int32_t& f_lo) {
  a = U.strand ? U.len - m.q - m.len : m.q;
  b = a + m.len;
  const int rec = record_of(U.rec_start, U.n_rec, a);
  f_lo = P.rec_frag0[rec] + (a - U.rec_start[rec]) / fragsize;
}

__global__ __launch_bounds__(256) void anib_bucket_kernel(const UnitDesc* __restrict__ units, const FragPair* __restrict__ pairs,
                                                          const Match* __restrict__ mem, const uint32_t* __restrict__ moff,
                                                          const uint32_t* __restrict__ mem_count, const uint64_t* __restrict__ ebase,
                                                          int32_t fragsize, uint32_t* __restrict__ frag_off, FragSeed* __restrict__ entries) {
  __shared__ uint32_t s_cnt[FRAG_MAX_FRAGS];
  __shared__ uint32_t s_part[256];
  const uint32_t unit = blockIdx.x, tid = threadIdx.x;
  const UnitDesc U = units[unit];
  const FragPair P = pairs[U.pair];
  const uint32_t nf = (uint32_t)P.n_frags;
  uint32_t* off = frag_off + 2 * (size_t)P.slot0 + 2 * (size_t)U.pair + (size_t)U.strand * (nf + 1);   // nf + 1 offsets per unit
  // the per-fragment counters: LDS for genomes of up to FRAG_MAX_FRAGS fragments (16.1 Mb at 1020 nt: every bacterial genome); a
  // larger genome (round 5: there used to be a hard limit) counts in its own offset array in HBM — global atomics, slower, rare —
  // and gets its offsets back from the cursors at the end
  const bool in_lds = nf <= (uint32_t)FRAG_MAX_FRAGS;
  uint32_t* cnt = in_lds ? s_cnt : off;
  for (uint32_t i = tid; i < nf; i += 256) cnt[i] = 0;
  if (!in_lds) __threadfence();
  __syncthreads();
  const Match* mine = mem + moff[unit];
  const uint32_t n = mem_count[unit];
  const uint32_t per = (nf + 255) / 256, r_lo = tid * per < nf ? tid * per : nf, r_hi = r_lo + per < nf ? r_lo + per : nf;
  for (int pass = 0; pass < 2; ++pass) {
    for (uint32_t i = tid; i < n; i += 256) {
      const Match m = mine[i];
      int32_t a, b, f;
      frag_span(U, P, m, fragsize, a, b, f);
      for (; f < (int32_t)nf && P.frag_pos[f] < b; ++f) {
        const int32_t fp = P.frag_pos[f], fe = fp + P.frag_len[f];
        const int32_t lo = a > fp ? a : fp, hi = b < fe ? b : fe;
        if (hi - lo < FRAG_MIN_CLIP) continue;
        const uint32_t at = atomicAdd(&cnt[f], 1u);
        if (pass) {
          FragSeed e;
          e.len = hi - lo;
          if (!U.strand) { e.q = lo - fp; e.s = m.r + (lo - a); }
          else { e.q = fe - hi; e.s = m.r + (b - hi); }
          entries[ebase[unit] + at] = e;
        }
      }
    }
    if (!in_lds) __threadfence();
    __syncthreads();
    if (pass) break;
    // exclusive prefix of the counters -> offsets (also the write cursors of pass 1)
    uint32_t sum = 0;
    for (uint32_t i = r_lo; i < r_hi; ++i) sum += cnt[i];
    s_part[tid] = sum;
    __syncthreads();
    if (tid == 0) { uint32_t run = 0; for (int i = 0; i < 256; ++i) { const uint32_t t = s_part[i]; s_part[i] = run; run += t; } off[nf] = run; }
    __syncthreads();
    uint32_t run = s_part[tid];
    for (uint32_t i = r_lo; i < r_hi; ++i) { const uint32_t c = cnt[i]; off[i] = run; cnt[i] = run; run += c; }
    if (!in_lds) __threadfence();
    __syncthreads();
  }
  if (!in_lds) {      // the cursors have run to the ends of their buckets: bucket i starts where bucket i - 1 ended
    const uint32_t before = r_lo > 0 && r_lo < nf ? off[r_lo - 1] : 0u;
    __syncthreads();
    for (uint32_t i = r_hi; i-- > r_lo + 1;) off[i] = off[i - 1];
    if (r_lo < r_hi) off[r_lo] = before;
  }
}

// ---- the X-drop extension, one wave, band in REGISTERS (same cells and rules as pga::frag_extend) -----------------------------
// Lane L owns the four diagonals k = 4L .. 4L + 3 of the 256-diagonal band (6 state words each).  On an anti-diagonal only the
// diagonals of one parity have a cell, i.e. per lane either {0, 2} or {1, 3}; their neighbours k +- 1 are the lane's own other
// two diagonals, except the lower neighbour of diagonal 0 (lane - 1's diagonal 3) and the upper neighbour of diagonal 3
// (lane + 1's diagonal 0): four lane shuffles per step, no LDS traffic, no barrier.  (The first version kept the band in LDS:
// 48 LDS operations per lane and step made the CU's LDS pipe the bound, ~0.7 us per wave step.)  LDS is used only to re-centre
// the band (every 16 steps, when the best diagonal has drifted) and for the staged sequence bytes.
struct FragBandLds { int32_t h[FRAG_BAND], x[FRAG_BAND], y[FRAG_BAND], hs[FRAG_BAND], xs[FRAG_BAND], ys[FRAG_BAND]; };
static_assert(FRAG_BAND == 256, "four diagonals per lane");

// (a template on the kernel's mode only so that each instantiation of anib_frag_kernel owns a copy: it stays a called function, and the
// LDS addresses every call site of one kernel passes are constants the compiler folds into that copy — a copy shared by two kernels
// takes them as arguments and the default kernel's register allocation changes)
template <bool ALL_DIAGS>
__device__ FragExt frag_extend_wave(FragBandLds& B, const uint8_t* __restrict__ qb, int32_t qmax, const uint8_t* __restrict__ sb, int32_t smax,
                                    int32_t abs_floor = FRAG_NEG, int32_t xdrop = FRAG_XDROP) {
  const int lane = threadIdx.x & 63;
  if (qmax <= 0 || smax <= 0) return FragExt{0, 0, 0, 0, 0};   // (uniform)
  const FragCellIn dead{FRAG_NEG, FRAG_NEG, FRAG_NEG, 0, 0, 0};
  FragCellIn S0 = dead, S1 = dead, S2 = dead, S3 = dead;
  int32_t koff = -FRAG_BAND / 2;
  if (lane == FRAG_BAND / 8) S0.h = 0;        // the anchor cell (0, 0): diagonal 0 = band index 128 = lane 32, slot 0
  int32_t b_score = 0, b_d = 0, b_K = 0, b_stat = 0;     // lane-local best (strict >: earliest cell wins); i, j follow from d, K
  int32_t xbest = 0;
  int dead_run = 0;
  for (int32_t d = 1; d <= qmax + smax; ++d) {
    if ((d % FRAG_TRACK) == 0) {            // re-centre the band on the best live H (ties: lowest diagonal)
      int32_t mh = FRAG_NEG / 2, mk = FRAG_BAND;
      if (S0.h > mh) { mh = S0.h; mk = 4 * lane; }
      if (S1.h > mh) { mh = S1.h; mk = 4 * lane + 1; }
      if (S2.h > mh) { mh = S2.h; mk = 4 * lane + 2; }
      if (S3.h > mh) { mh = S3.h; mk = 4 * lane + 3; }
      for (int o = 32; o > 0; o >>= 1) {
        const int32_t oh = __shfl_xor(mh, o, 64), ok_ = __shfl_xor(mk, o, 64);
        if (oh > mh || (oh == mh && ok_ < mk)) { mh = oh; mk = ok_; }
      }
      if (mk < FRAG_BAND) {
        int32_t s = mk - FRAG_BAND / 2;
        if (s > FRAG_SHIFT_MAX) s = FRAG_SHIFT_MAX;
        if (s < -FRAG_SHIFT_MAX) s = -FRAG_SHIFT_MAX;
        s &= ~1;
        if (s != 0) {                       // (uniform) through LDS: new state of diagonal k = old state of k + s
          const FragCellIn* own[4] = {&S0, &S1, &S2, &S3};
          __syncthreads();
          for (int t = 0; t < 4; ++t) {
            const int k = 4 * lane + t;
            B.h[k] = own[t]->h; B.x[k] = own[t]->x; B.y[k] = own[t]->y; B.hs[k] = own[t]->hs; B.xs[k] = own[t]->xs; B.ys[k] = own[t]->ys;
          }
          __syncthreads();
          FragCellIn n[4];
          for (int t = 0; t < 4; ++t) {
            const int f = 4 * lane + t + s;
            n[t] = (f >= 0 && f < FRAG_BAND) ? FragCellIn{B.h[f], B.x[f], B.y[f], B.hs[f], B.xs[f], B.ys[f]} : dead;
          }
          S0 = n[0]; S1 = n[1]; S2 = n[2]; S3 = n[3];
          koff += s;
        }
      }
    }
    if ((d % FRAG_XSYNC) == 0) {            // the wave's shared X-drop reference: best score so far
      int32_t v = b_score;
      for (int o = 32; o > 0; o >>= 1) { const int32_t w = __shfl_xor(v, o, 64); v = w > v ? w : v; }
      xbest = v;
    }
    bool alive = false;
    // one cell: slot t of this lane, neighbours u (diagonal + 1) and l (diagonal - 1), own previous state g.  Straight-line:
    // a cell outside the rectangle has no predecessor at all, which makes it the dead state by itself.
    auto cell = [&](int t, const FragCellIn& u, bool has_u_lane, const FragCellIn& l, bool has_l_lane, FragCellIn& g) {
      const int k = 4 * lane + t;
      const int32_t K = k + koff;
      const int32_t i = (d - K) / 2, j = (d + K) / 2;
      const bool in = (i >= 0) & (j >= 0) & (i <= qmax) & (j <= smax);
      int32_t iq = i - 1, js = j - 1;      // (clamped: lanes outside the rectangle read a valid byte they do not use)
      iq = iq < 0 ? 0 : (iq > FRAG_SIZE + 3 ? FRAG_SIZE + 3 : iq);
      js = js < 0 ? 0 : (js > FRAG_SIZE + FRAG_SLACK + 3 ? FRAG_SIZE + FRAG_SLACK + 3 : js);
      const uint8_t qv = qb[iq], sv = sb[js];
      const bool inner = in & (i >= 1) & (j >= 1);
      const FragCellIn c = frag_cell(in & (i >= 1) & has_u_lane, u, in & (j >= 1) & has_l_lane, l, inner, g, inner & (qv < 4) & (qv == sv), xbest, abs_floor, xdrop);
      g = c;
      alive = alive | (c.h > FRAG_NEG / 2) | (c.x > FRAG_NEG / 2) | (c.y > FRAG_NEG / 2);
      const bool better = c.h > b_score;
      b_score = better ? c.h : b_score; b_d = better ? d : b_d; b_K = better ? K : b_K; b_stat = better ? c.hs : b_stat;
    };
    if (((d + koff) & 1) == 0) {            // slots 0 and 2 have a cell (4 * lane is even)
      FragCellIn lm = dead;                 // lane - 1's slot 3 = diagonal k - 1 of slot 0
      // (DPP wave shifts: a VALU move each, not a trip through the LDS crossbar; lane 0's fill value is never used)
      lm.h = from_lane_below(S3.h, FRAG_NEG); lm.y = from_lane_below(S3.y, FRAG_NEG); lm.hs = from_lane_below(S3.hs, 0); lm.ys = from_lane_below(S3.ys, 0);
      const FragCellIn o1 = S1, o3 = S3;    // neighbours of the other parity: not written on this anti-diagonal
      cell(0, o1, true, lm, lane > 0, S0);
      cell(2, o3, true, o1, true, S2);
    } else {                                // slots 1 and 3
      FragCellIn up = dead;                 // lane + 1's slot 0 = diagonal k + 1 of slot 3
      up.h = (int32_t)dpp_from_above0((uint32_t)S0.h); up.x = (int32_t)dpp_from_above0((uint32_t)S0.x);
      up.hs = (int32_t)dpp_from_above0((uint32_t)S0.hs); up.xs = (int32_t)dpp_from_above0((uint32_t)S0.xs);   // (lane 63: 0, never used)
      const FragCellIn o0 = S0, o2 = S2;
      cell(1, o2, true, o0, true, S1);
      cell(3, up, lane < 63, o2, true, S3);
    }
    dead_run = __ballot(alive) ? 0 : dead_run + 1;
    if (dead_run >= 2) break;
  }
  // best cell of the wave: highest score, ties -> earliest anti-diagonal, then lowest diagonal
  for (int o = 32; o > 0; o >>= 1) {
    const int32_t os = __shfl_xor(b_score, o, 64), od = __shfl_xor(b_d, o, 64), oK = __shfl_xor(b_K, o, 64), ot = __shfl_xor(b_stat, o, 64);
    if (os > b_score || (os == b_score && (od < b_d || (od == b_d && oK < b_K)))) { b_score = os; b_d = od; b_K = oK; b_stat = ot; }
  }
  const int32_t b_i = (b_d - b_K) / 2, b_j = (b_d + b_K) / 2;
  FragExt e;
  e.score = b_score; e.di = b_score > 0 ? b_i : 0; e.dj = b_score > 0 ? b_j : 0;
  e.mm = b_score > 0 ? b_stat >> 16 : 0; e.gaps = b_score > 0 ? b_stat & 0xFFFF : 0;
  return e;
}

// ---- the word tier: blastn's 11-mer seeds for the fragments the 16-mer seeds leave without a reportable HSP -----------------
// (statement and rationale: the CPU checker's `word_tier_seeds` (anib_cpu.cpp), pg_anib_core.h WORD_*.)  Per subject genome a direct index of
// its 11-mers lives in HBM (4^11 + 1 bucket offsets = 16.8 MB, one position per clean 11-mer: ~37 MB for 5 Mb, built on first
// use by three small kernels and kept with the genome's seed lists); a second pass of anib_frag_kernel over the failed fragments
// of every pair that has at least one reportable fragment looks all 2 x ~1010 words of a fragment up (one lane per position),
// keeps the hits whose 32-base flank on either side matches in >= WORD_FLANK_MIN positions, turns each into the maximal exact
// match around it and adds those to the fragment's seeds before the anchors are chosen again.
struct WordIdx { const uint32_t* start; const int32_t* pos; };   // per reference of the batch (null: not built)
constexpr uint32_t WORD_BUCKETS = 1u << (2 * WORD_K);

__device__ __forceinline__ int window_matches(uint64_t a, uint32_t aok, uint64_t b, uint32_t bok) {
  const uint64_t x = a ^ b;
  const uint64_t eq = ~(x | (x >> 1)) & 0x5555555555555555ull;
  const uint32_t ok = aok & bok;
  const uint64_t okf = (uint64_t)spread16(ok & 0xFFFFu) | ((uint64_t)spread16(ok >> 16) << 32);
  return __popcll(eq & okf);
}

__global__ __launch_bounds__(256) void anib_word_count_kernel(const uint32_t* __restrict__ codes, const uint32_t* __restrict__ mask, int32_t len,
                                                              uint32_t* __restrict__ cnt, int32_t* __restrict__ pos, int fill) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;    // word start
  if (p + WORD_K > len) return;
  uint64_t c; uint32_t ok;
  packed_window(codes, mask, len, p, c, ok);
  if ((ok & ((1u << WORD_K) - 1u)) != ((1u << WORD_K) - 1u)) return;
  // the word value as the host statement builds it: first base in the highest bits
  uint32_t v = 0;
#pragma unroll
  for (int t = 0; t < WORD_K; ++t) v = (v << 2) | (uint32_t)((c >> (2 * t)) & 3u);
  const uint32_t at = atomicAdd(&cnt[v], 1u);
  if (fill) pos[at] = (int32_t)p;
}
// exclusive scan of WORD_BUCKETS counters in place (+ the total at [WORD_BUCKETS]): 4096 per block, then the block sums
__global__ __launch_bounds__(1024) void anib_word_scan1_kernel(uint32_t* __restrict__ cnt, uint32_t* __restrict__ bsum) {
  __shared__ uint32_t s[1024];
  const uint32_t t = threadIdx.x, base = blockIdx.x * 4096u + t * 4u;
  const uint32_t a = cnt[base], b = cnt[base + 1], c = cnt[base + 2], d = cnt[base + 3];
  s[t] = a + b + c + d;
  __syncthreads();
  for (uint32_t o = 1; o < 1024; o <<= 1) { const uint32_t v = t >= o ? s[t - o] : 0u; __syncthreads(); s[t] += v; __syncthreads(); }
  const uint32_t excl = s[t] - (a + b + c + d);
  cnt[base] = excl; cnt[base + 1] = excl + a; cnt[base + 2] = excl + a + b; cnt[base + 3] = excl + a + b + c;
  if (t == 1023) bsum[blockIdx.x] = s[t];
}
__global__ __launch_bounds__(1024) void anib_word_scan2_kernel(uint32_t* __restrict__ bsum, uint32_t n_blocks, uint32_t* __restrict__ total) {
  __shared__ uint32_t s[1024];
  const uint32_t t = threadIdx.x;
  const uint32_t v0 = t < n_blocks ? bsum[t] : 0u;
  s[t] = v0;
  __syncthreads();
  for (uint32_t o = 1; o < 1024; o <<= 1) { const uint32_t v = t >= o ? s[t - o] : 0u; __syncthreads(); s[t] += v; __syncthreads(); }
  if (t < n_blocks) bsum[t] = s[t] - v0;
  if (t == 1023) *total = s[t];
}
__global__ __launch_bounds__(1024) void anib_word_scan3_kernel(uint32_t* __restrict__ cnt, const uint32_t* __restrict__ bsum, uint32_t* __restrict__ cursor) {
  const uint32_t i = blockIdx.x * 1024u + threadIdx.x;
  const uint32_t v = cnt[i] + bsum[i >> 12];
  cnt[i] = v; cursor[i] = v;
}

// the slots to search again: fragments without a reportable row in pairs that have some (0 < kept < fragments)
__global__ __launch_bounds__(256) void anib_failed_kernel(const FragPair* __restrict__ pairs, const uint32_t* __restrict__ slot_pair, uint32_t n_slots,
                                                          const FragRow* __restrict__ rows, const uint32_t* __restrict__ n_rows,
                                                          const pg_anib_result* __restrict__ res, const WordIdx* __restrict__ widx,
                                                          const UnitDesc* __restrict__ units, uint32_t* __restrict__ list, uint32_t* __restrict__ n_list) {
  const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
  if (slot >= n_slots) return;
  const uint32_t pair = slot_pair[slot];
  const pg_anib_result r = res[pair];
  if (r.n_kept <= 0 || r.n_kept >= r.n_frags || widx[units[2 * pair].ref].start == nullptr) return;
  const uint32_t n = n_rows[slot];
  for (uint32_t i = 0; i < n; ++i) {
    const FragRow x = rows[(size_t)slot * FRAG_ROWS + i];
    const int32_t alnlen = x.length - x.gaps;
    if ((double)alnlen / (double)x.qlen > 0.7 && (double)(alnlen - x.mismatch) / (double)x.qlen > 0.3) return;
  }
  list[atomicAdd(n_list, 1u)] = slot;
}

// match(p) of the start-point choice (pg_anib_core.h: frag_diag_best_init, frag_start_point) for one lane's diagonal: query base p of
// the staged strand == subject base p + diag, both clean, the subject base inside [s_lo, s_hi).  The walks go base by base but in
// order, so the lane keeps the answers of 32 consecutive positions in a register: two packed 32-base windows (fragment strand from
// LDS, subject from HBM) per refill instead of two dependent global loads per base (the first version: 2.6 x the whole C5 grid).
struct DiagMatch {
  const uint32_t* qpk; const uint32_t* qok; int32_t qlen;
  const uint32_t* scodes; const uint32_t* smask; int32_t slen;
  int64_t diag, s_lo, s_hi;
  int32_t w0;
  uint32_t bits;
  __device__ __forceinline__ void refill(int32_t p) {
    w0 = p & ~31;
    uint64_t qc, sc; uint32_t qk, sk;
    packed_window(qpk, qok, qlen, w0, qc, qk);
    packed_window(scodes, smask, slen, (int64_t)w0 + diag, sc, sk);
    const uint64_t x = qc ^ sc;
    uint64_t e = ~(x | (x >> 1)) & 0x5555555555555555ull;          // bit 2t set: bases t equal
    e = (e | (e >> 1)) & 0x3333333333333333ull;                     // compact the even bits into 32
    e = (e | (e >> 2)) & 0x0F0F0F0F0F0F0F0Full;
    e = (e | (e >> 4)) & 0x00FF00FF00FF00FFull;
    e = (e | (e >> 8)) & 0x0000FFFF0000FFFFull;
    e = (e | (e >> 16)) & 0x00000000FFFFFFFFull;
    uint32_t in = 0xFFFFFFFFu;                                      // subject positions inside the record
    const int64_t a = s_lo - ((int64_t)w0 + diag), b = s_hi - ((int64_t)w0 + diag);
    if (a > 0) in &= a >= 32 ? 0u : ~((1u << a) - 1u);
    if (b < 32) in &= b <= 0 ? 0u : ((1u << b) - 1u);
    bits = (uint32_t)e & qk & sk & in;
  }
  __device__ __forceinline__ bool operator()(int32_t p) {
    if ((p & ~31) != w0) refill(p);
    return (bits >> (p & 31)) & 1u;
  }
};

// Three waves per SIMD (168 VGPRs, 5 spilled) instead of the two that 184 VGPRs allow: the kernel waits on dependent loads and lane-0
// sections, not on issue — measured on C5: 3.72 -> 3.33 s of kernel time per two steps, 99.5 -> 94.1 s per grid; the LDS (16 KB per
// wave) caps it at ten waves per CU, so a fourth would need the word tier's seed list out of LDS first.
#ifndef PGA_FRAG_WAVES
#define PGA_FRAG_WAVES 3
#endif
#define PGA_FRAG_ATTR __attribute__((amdgpu_waves_per_eu(PGA_FRAG_WAVES, PGA_FRAG_WAVES)))
// ALL_DIAGS (PG_ANIB_SEARCH_ALL_DIAGS, pg_anib_set_search): the preliminary stage also walks the diagonals of a candidate's band that hold
// no seed (the CPU checker's ANIB_ALL_DIAGS) — blastn takes its initial HSPs from every 11-mer diagonal.  FRAG_XDIAGS diagonals per
// candidate, one lane each in two rounds; their initial HSPs (best [0, FRAG_XDIAGS), second [FRAG_XDIAGS, 2 FRAG_XDIAGS), the diagonal
// implied by the index) live in 3 KiB of LDS that only this instantiation has.  <false> is the kernel as it was.
constexpr int FRAG_XDIAGS = 2 * FRAG_VOTE_FAR - 1;
// (with them the block's LDS allows two waves per SIMD, so that is what ALL_DIAGS asks for; the default asks for what it always has)
#define PGA_FRAG_ATTR_MODE __attribute__((amdgpu_waves_per_eu(ALL_DIAGS ? 2 : PGA_FRAG_WAVES, PGA_FRAG_WAVES)))
template <bool ALL_DIAGS>
__global__ __launch_bounds__(64) PGA_FRAG_ATTR_MODE void anib_frag_kernel(const RefDesc* __restrict__ refs, const UnitDesc* __restrict__ units,
                                                       const FragPair* __restrict__ pairs, const uint32_t* __restrict__ slot_pair,
                                                       const uint32_t* __restrict__ frag_off, const FragSeed* __restrict__ entries,
                                                       const uint64_t* __restrict__ ebase, FragRow* __restrict__ rows,
                                                       uint32_t* __restrict__ n_rows, const uint32_t* __restrict__ slot_list,
                                                       const WordIdx* __restrict__ widx) {
  // (the band's LDS copy — used only while an extension re-centres — and the word tier's seed list — used only before the anchors are
  // chosen — share their 6 KiB: with the per-strand initial HSPs below the block stays at 8 per CU, which its registers allow anyway)
  __shared__ union FragScratch { FragBandLds band; FragSeed w[WORD_MAX_SEEDS]; __device__ FragScratch() {} } s_u;
  FragBandLds& B = s_u.band;
  FragSeed* const s_w = s_u.w;                  // word tier: the union of the fragment's seeds and the word seeds
  __shared__ uint8_t s_q[FRAG_SIZE + 4], s_s[FRAG_SIZE + FRAG_SLACK + 4];
  __shared__ FragSeed s_e[FRAG_MAX_SEEDS];
  __shared__ uint32_t s_qpk2[2][FRAG_SIZE / 16 + 4], s_qok2[2][FRAG_SIZE / 32 + 4];   // the fragment's two strands, packed like a genome
  __shared__ uint32_t s_nw;
  __shared__ FragInit s_init2[2][2 * FRAG_MAX_SEEDS];   // per strand: best initial HSP of every seed diagonal [0, 64), its second [64, 128)
  __shared__ int64_t s_diag2[2][FRAG_MAX_SEEDS];
  __shared__ int s_n[2];                        // seed diagonals of the strand
  __shared__ FragSeed s_anchor[2][FRAG_MAX_CAND];      // the start point as a one-base anchor
  __shared__ int32_t s_votes[2][FRAG_MAX_CAND];        // the candidates' initial-HSP scores
  __shared__ int s_members[2][FRAG_MAX_CAND];          // ... and how many initial HSPs their locus holds (frag_init_is_lone_weak)
  __shared__ FragPrelim s_pbest[FRAG_MAX_CAND];        // pass 2: the best preliminary alignment of every candidate of the strand
  __shared__ int s_have[FRAG_MAX_CAND];
  __shared__ int s_nc[2];
  __shared__ FragRow s_rows[FRAG_ROWS];
  __shared__ int s_nrows;
  [[maybe_unused]] FragInit* s_x = nullptr;     // ALL_DIAGS: the initial HSPs of the current candidate's seedless diagonals
  if constexpr (ALL_DIAGS) {
    __shared__ FragInit s_xinit[3 * 64];        // (2 FRAG_XDIAGS used; the tail stays 0: three ballots of 64 cover it)
    static_assert(2 * FRAG_XDIAGS <= 3 * 64, "three entries per lane");
    s_x = s_xinit;
    for (int t = threadIdx.x; t < 3 * 64; t += 64) s_xinit[t] = FragInit{0, 0, 0, 0};
  }
  const bool word = slot_list != nullptr;       // second pass: the failed fragments, with blastn-sized word seeds added
  const uint32_t slot = word ? slot_list[blockIdx.x] : blockIdx.x;
  const int lane = threadIdx.x;
  const uint32_t pair = slot_pair[slot];
  const FragPair P = pairs[pair];
  const int32_t f = (int32_t)(slot - P.slot0);
  const int32_t fp = P.frag_pos[f], qlen = P.frag_len[f];
  if (lane == 0) s_nrows = 0;
  __syncthreads();
  // pass 1: the anchors of both strands (a weak candidate is dropped when the fragment has a strong one: frag_keep_candidate)
  for (int strand = 0; strand < 2; ++strand) {
    const uint32_t unit = 2 * pair + strand;
    const uint32_t* off = frag_off + 2 * (size_t)P.slot0 + 2 * (size_t)pair + (size_t)strand * (P.n_frags + 1);
    const uint32_t e0 = off[f], n_all = off[f + 1] - e0;
    uint32_t* const s_qpk = s_qpk2[strand];
    uint32_t* const s_qok = s_qok2[strand];
    FragInit* const s_init = s_init2[strand];
    int64_t* const s_diag = s_diag2[strand];
    if (lane == 0) { s_nc[strand] = 0; s_n[strand] = 0; }
    if (n_all == 0 && !word) continue;        // (uniform)
    const FragSeed* mine = entries + ebase[unit] + e0;
    // the seeds of this fragment; more than FRAG_MAX_SEEDS (repeats): the first 64 in the order (len desc, q asc, s asc)
    int n = (int)n_all;
    __syncthreads();
    if (n_all <= (uint32_t)FRAG_MAX_SEEDS) {
      if (lane < n) s_e[lane] = mine[lane];
    } else {
      for (uint32_t a = lane; a < n_all; a += 64) {
        const FragSeed x = mine[a];
        uint32_t rank = 0;
        for (uint32_t b = 0; b < n_all; ++b) {
          const FragSeed y = mine[b];
          rank += (y.len > x.len || (y.len == x.len && (y.q < x.q || (y.q == x.q && (y.s < x.s || (y.s == x.s && b < a)))))) ? 1u : 0u;
        }
        if (rank < (uint32_t)FRAG_MAX_SEEDS) s_e[rank] = x;
      }
      n = FRAG_MAX_SEEDS;
    }
    __syncthreads();
    if (word) {
      // ---- word tier: every 11-mer of this strand of the fragment against the subject's word index ----
      const UnitDesc Uw = units[unit];
      const RefDesc Rw = refs[Uw.ref];
      const WordIdx W = widx[Uw.ref];
      const SeqView QVw{Uw.codes, Uw.mask, Uw.len};
      for (int t = lane; t < FRAG_SIZE / 16 + 4; t += 64) s_qpk[t] = 0;
      for (int t = lane; t < FRAG_SIZE / 32 + 4; t += 64) s_qok[t] = 0;
      if (lane == 0) s_nw = 0;
      __syncthreads();
      for (int32_t t = lane; t < qlen; t += 64) {     // stage the strand: bytes (s_q) and the packed form
        const int64_t g = strand ? fp + (qlen - 1 - t) : fp + t;
        const bool okb = QVw.clean(g);
        const uint32_t b = okb ? (uint32_t)(strand ? 3 - QVw.base(g) : QVw.base(g)) : 0u;
        s_q[t] = okb ? (uint8_t)b : (uint8_t)4;
        atomicOr(&s_qpk[t >> 4], b << (2 * (t & 15)));
        if (okb) atomicOr(&s_qok[t >> 5], 1u << (t & 31));
      }
      __syncthreads();
      for (int32_t i = lane; i + WORD_K <= qlen; i += 64) {
        uint64_t qc; uint32_t qk;
        packed_window(s_qpk, s_qok, qlen, i, qc, qk);
        if ((qk & ((1u << WORD_K) - 1u)) != ((1u << WORD_K) - 1u)) continue;
        uint32_t v = 0;
#pragma unroll
        for (int t = 0; t < WORD_K; ++t) v = (v << 2) | (uint32_t)((qc >> (2 * t)) & 3u);
        const uint32_t h0 = W.start[v], h1 = W.start[v + 1];
        for (uint32_t h = h0; h < h1; ++h) {
          const int32_t p = W.pos[h];
          // the first word of its exact match inside the fragment only
          if (i > 0) {
            uint64_t sc1; uint32_t so1;
            packed_window(Rw.codes, Rw.mask, Rw.len, (int64_t)p - 1, sc1, so1);
            if (s_q[i - 1] < 4 && (so1 & 1u) && (uint32_t)(sc1 & 3u) == (uint32_t)s_q[i - 1]) continue;
          }
          uint64_t ql, sl, qr, sr; uint32_t qlo, slo, qro, sro;
          packed_window(s_qpk, s_qok, qlen, (int64_t)i - WORD_FLANK, ql, qlo);
          packed_window(Rw.codes, Rw.mask, Rw.len, (int64_t)p - WORD_FLANK, sl, slo);
          packed_window(s_qpk, s_qok, qlen, (int64_t)i + WORD_K, qr, qro);
          packed_window(Rw.codes, Rw.mask, Rw.len, (int64_t)p + WORD_K, sr, sro);
          if (window_matches(ql, qlo, sl, slo) < WORD_FLANK_MIN && window_matches(qr, qro, sr, sro) < WORD_FLANK_MIN) continue;
          int32_t L = WORD_K;      // the maximal exact match to the right (to the left it starts here)
          for (;;) {
            uint64_t a, b2; uint32_t ao, bo;
            packed_window(s_qpk, s_qok, qlen, (int64_t)i + L, a, ao);
            packed_window(Rw.codes, Rw.mask, Rw.len, (int64_t)p + L, b2, bo);
            const uint64_t x = a ^ b2;
            uint64_t ne = (x | (x >> 1)) & 0x5555555555555555ull;          // differing bases
            const uint32_t bad = ~(ao & bo);
            ne |= (uint64_t)spread16(bad & 0xFFFFu) | ((uint64_t)spread16(bad >> 16) << 32);
            const int run = ne ? (int)(__builtin_ctzll(ne) >> 1) : 32;
            L += run;
            if (run < 32) break;
          }
          // not a piece of one of the fragment's own seeds (same diagonal, inside it)
          bool dup = false;
          for (int y = 0; y < n; ++y) dup = dup || (s_e[y].s - s_e[y].q == p - i && i >= s_e[y].q && i + L <= s_e[y].q + s_e[y].len);
          if (dup) continue;
          const uint32_t at = atomicAdd(&s_nw, 1u);
          if (at < (uint32_t)(WORD_MAX_SEEDS - FRAG_MAX_SEEDS)) s_w[FRAG_MAX_SEEDS + at] = FragSeed{p, i, L};
        }
      }
      __syncthreads();
      const uint32_t m = s_nw;
      if (m > 0 && m <= (uint32_t)(WORD_MAX_SEEDS - FRAG_MAX_SEEDS)) {   // (more: a repeat family, the tier leaves the fragment as it is)
        // the word seeds come FIRST (pg_anib_core.h FRAG_WORD_FIRST: the longest ones, at most half of the list), then the fragment's own
        // seeds — each group ranked (len desc, q asc, s asc) — until the list holds FRAG_MAX_SEEDS
        if (lane < n) s_w[lane] = s_e[lane];
        __syncthreads();
        const int mw = (int)m < FRAG_WORD_FIRST ? (int)m : FRAG_WORD_FIRST;
        const int tot = n + (int)m;
        for (int a = lane; a < tot; a += 64) {
          const bool own = a < n;
          const FragSeed x = own ? s_w[a] : s_w[FRAG_MAX_SEEDS + (a - n)];
          const int b0 = own ? 0 : n, b1 = own ? n : tot;
          int rank = 0;
          for (int b = b0; b < b1; ++b) {
            const FragSeed y = b < n ? s_w[b] : s_w[FRAG_MAX_SEEDS + (b - n)];
            rank += (y.len > x.len || (y.len == x.len && (y.q < x.q || (y.q == x.q && (y.s < x.s || (y.s == x.s && b < a)))))) ? 1 : 0;
          }
          const int at = own ? mw + rank : (rank < mw ? rank : FRAG_MAX_SEEDS);
          if (at < FRAG_MAX_SEEDS) s_e[at] = x;
        }
        n = n + mw < FRAG_MAX_SEEDS ? n + mw : FRAG_MAX_SEEDS;
      }
      __syncthreads();
      if (n == 0) continue;                   // (uniform)
    }
    // ---- blastn's start points (pg_anib_core.h): one diagonal walk per distinct seed diagonal, one lane each ----
    {
      const UnitDesc Ud = units[unit];
      const RefDesc Rd = refs[Ud.ref];
      const SeqView QVd{Ud.codes, Ud.mask, Ud.len};
      if (!word) {                          // (the word tier has staged the strand already: s_qpk / s_qok)
        for (int t = lane; t < FRAG_SIZE / 16 + 4; t += 64) s_qpk[t] = 0;
        for (int t = lane; t < FRAG_SIZE / 32 + 4; t += 64) s_qok[t] = 0;
        __syncthreads();
        for (int32_t t = lane; t < qlen; t += 64) {
          const int64_t g = strand ? fp + (qlen - 1 - t) : fp + t;
          const bool okb = QVd.clean(g);
          const uint32_t b = okb ? (uint32_t)(strand ? 3 - QVd.base(g) : QVd.base(g)) : 0u;
          atomicOr(&s_qpk[t >> 4], b << (2 * (t & 15)));
          if (okb) atomicOr(&s_qok[t >> 5], 1u << (t & 31));
        }
      }
      __syncthreads();
      if (lane < n) {
        const FragSeed me = s_e[lane];
        const int64_t diag = (int64_t)me.s - me.q;
        bool dup = false;                     // the diagonal's walk belongs to its LONGEST seed (frag_seed_before: s_e is in no particular order here)
        for (int u = 0; u < n; ++u) dup = dup || (u != lane && (int64_t)s_e[u].s - s_e[u].q == diag && frag_seed_before(s_e[u], me));
        FragInit in{0, 0, 0, 0}, in2{0, 0, 0, 0};
        if (!dup) {
          const int srec = record_of(Rd.rec_start, Rd.n_rec, me.s);
          DiagMatch match{s_qpk, s_qok, qlen, Rd.codes, Rd.mask, (int32_t)Rd.len, diag, Rd.rec_start[srec], Rd.rec_start[srec + 1] - 1, -64, 0u};
          in = frag_diag_best_init(match, qlen, diag, me.q, &in2);
        }
        s_init[lane] = in;
        s_init[FRAG_MAX_SEEDS + lane] = in2;
        s_diag[lane] = diag;
      }
      __syncthreads();
      if (lane == 0) {
        int pick[FRAG_MAX_CAND], members[FRAG_MAX_CAND] = {};
        const int nc = frag_pick_inits(s_init, s_diag, n, pick, members, FRAG_MAX_CAND);
        s_nc[strand] = nc;
        s_n[strand] = n;
        for (int c = 0; c < nc; ++c) { s_anchor[strand][c] = FragSeed{(int32_t)(s_init[pick[c]].q_off + s_diag[pick[c]]), s_init[pick[c]].q_off, 1}; s_votes[strand][c] = s_init[pick[c]].score; s_members[strand][c] = members[c]; }
      }
      __syncthreads();
      if (lane < s_nc[strand] && frag_init_is_lone_weak(s_votes[strand][lane], s_members[strand][lane])) {
        // a lone chance-sized hit: the start rule, one lane per candidate — the word becomes the one-base anchor the HSP grows from
        // (the others keep their word as the anchor: their start point comes out of the preliminary stage, pass 2)
        const FragSeed w = s_anchor[strand][lane];
        const int64_t diag = (int64_t)w.s - w.q;
        const int srec = record_of(Rd.rec_start, Rd.n_rec, w.s);
        const int64_t s_lo = Rd.rec_start[srec], s_hi = Rd.rec_start[srec + 1] - 1;
        DiagMatch match{s_qpk, s_qok, qlen, Rd.codes, Rd.mask, (int32_t)Rd.len, diag, s_lo, s_hi, -64, 0u};
        const int64_t lo64 = s_lo - diag, hi64 = s_hi - diag;
        const int32_t lo = lo64 > 0 ? (int32_t)lo64 : 0, hi = hi64 < qlen ? (int32_t)hi64 : qlen;
        const int32_t g = frag_start_point(match, qlen, w.q, (int64_t)w.s - s_lo, lo, hi, s_votes[strand][lane]);
        s_anchor[strand][lane] = FragSeed{(int32_t)(g + diag), g, 1};
      }
      __syncthreads();
    }
  }
  __syncthreads();
  int32_t vmax = 0;
  for (int strand = 0; strand < 2; ++strand)
    for (int c = 0; c < s_nc[strand]; ++c) vmax = s_votes[strand][c] > vmax ? s_votes[strand][c] : vmax;
  // pass 2: the extensions
  for (int strand = 0; strand < 2; ++strand) {
    const uint32_t unit = 2 * pair + strand;
    const int nc = s_nc[strand];
    if (nc == 0) continue;
    const UnitDesc U = units[unit];
    const RefDesc R = refs[U.ref];
    const SeqView SV{R.codes, R.mask, R.len}, QV{U.codes, U.mask, U.len};
    // phase 0: the preliminary stage of every candidate that is not a lone chance-sized hit; more than two such candidates (a
    // repeat family): the two best preliminary alignments go on.  phase 1: the final alignments, in the candidates' order.
    if (lane < FRAG_MAX_CAND) s_have[lane] = 0;
    __syncthreads();
    for (int phase = 0; phase < 2; ++phase) {
    if (phase == 1) {
      __syncthreads();
      if (lane == 0) {
        int n_have = 0;
        for (int c = 0; c < nc; ++c) n_have += s_have[c];
        while (n_have > FRAG_MAX_FINALS) {
          int worst = -1;
          for (int c = 0; c < nc; ++c) if (s_have[c] && (worst < 0 || !frag_prelim_before(s_pbest[c], s_pbest[worst]))) worst = c;
          s_have[worst] = 0; --n_have;
        }
      }
      __syncthreads();
    }
    for (int c = 0; c < nc; ++c) {
      if (!frag_keep_init(s_votes[strand][c], vmax)) continue;   // (uniform)
      FragSeed A = s_anchor[strand][c];
      const int srec = record_of(R.rec_start, R.n_rec, A.s);
      const int32_t s_lo = R.rec_start[srec], s_hi = R.rec_start[srec + 1] - 1;
      auto q_at = [&](int32_t p) -> uint8_t {
        if (p < 0 || p >= qlen) return 4;
        const int64_t g = strand ? fp + (qlen - 1 - p) : fp + p;
        if (!QV.clean(g)) return 4;
        return (uint8_t)(strand ? 3 - QV.base(g) : QV.base(g));
      };
      auto s_at = [&](int32_t p) -> uint8_t { return (p >= s_lo && p < s_hi && SV.clean(p)) ? (uint8_t)SV.base(p) : 5; };
      const int32_t cap = FRAG_SIZE + FRAG_SLACK;
      const bool weak = frag_init_is_lone_weak(s_votes[strand][c], s_members[strand][c]);
      const int64_t db_len = (int64_t)R.rec_start[R.n_rec] - R.rec_start[0] - R.n_rec;
      if (weak && phase == 0) continue;      // (uniform)
      if (!weak && phase == 1 && !s_have[c]) continue;
      if (!weak && phase == 0) {
        // ---- blastn's preliminary stage (pg_anib_core.h, FragPrelim): the initial HSPs of the candidate's neighbourhood, best first, each
        // grown under the preliminary X-drop unless a better preliminary alignment holds it; the final alignment starts where the best one did
        const FragInit* const inits = s_init2[strand];
        const int64_t* const diags = s_diag2[strand];
        const int n = s_n[strand];
        const int64_t diag_c = (int64_t)A.s - A.q;
        auto eligible = [&](int x) -> bool {      // entry x: x < 64 the diagonal's best initial HSP, else its second
          const int t = x & (FRAG_MAX_SEEDS - 1);
          if (t >= n || inits[t].score <= 0 || inits[x].score <= 0) return false;
          const int64_t dd = diags[t] - diag_c;
          if (dd >= FRAG_VOTE_FAR || -dd >= FRAG_VOTE_FAR) return false;
          for (int p = 0; p < c; ++p) {      // (the neighbourhood of an earlier candidate)
            const int64_t d1 = diags[t] - ((int64_t)s_anchor[strand][p].s - s_anchor[strand][p].q);
            if (d1 < FRAG_VOTE_FAR && -d1 < FRAG_VOTE_FAR) return false;
          }
          return record_of(R.rec_start, R.n_rec, (int32_t)(inits[t].q_off + diags[t])) == srec;
        };
        if constexpr (ALL_DIAGS) {
          // the band's diagonals that hold no seed and lie outside every earlier candidate's neighbourhood: one lane walks one whole
          // diagonal.  DiagMatch answers false for every subject position outside [s_lo, s_hi) and packed_window reads nothing outside
          // the subject's arrays, so a diagonal that runs off either end of the subject, or into another record, is walked like any other.
          for (int j = lane; j < FRAG_XDIAGS; j += 64) {
            const int64_t d2 = diag_c - (FRAG_VOTE_FAR - 1) + j;
            bool skip = false;
            for (int t = 0; t < n; ++t) skip = skip || diags[t] == d2;
            for (int p = 0; p < c; ++p) {
              const int64_t d1 = d2 - ((int64_t)s_anchor[strand][p].s - s_anchor[strand][p].q);
              skip = skip || (d1 < FRAG_VOTE_FAR && -d1 < FRAG_VOTE_FAR);
            }
            FragInit in{0, 0, 0, 0}, in2{0, 0, 0, 0};
            if (!skip) {
              DiagMatch match{s_qpk2[strand], s_qok2[strand], qlen, R.codes, R.mask, (int32_t)R.len, d2, (int64_t)s_lo, (int64_t)s_hi, -64, 0u};
              in = frag_diag_walk(match, qlen, d2, &in2);
              if (in.score <= 0 || record_of(R.rec_start, R.n_rec, (int32_t)(in.q_off + d2)) != srec) in = in2 = FragInit{0, 0, 0, 0};
            }
            s_x[j] = in;
            s_x[FRAG_XDIAGS + j] = in2;
          }
          __syncthreads();
        }
        // every lane ranks its two entries (lane, 64 + lane) among the eligible ones in blastn's order; ALL_DIAGS: word w >= 2 of the masks is
        // entries [64 (w - 2), 64 (w - 1)) of s_x, three more per lane
        constexpr int NW = ALL_DIAGS ? 5 : 2;
        unsigned long long el[NW];      // (uniform masks)
        int rank[NW];
        int n_elig;
        [[maybe_unused]] auto ent = [&](int v, int t) -> FragInit { return v >= 2 ? s_x[64 * (v - 2) + t] : inits[64 * v + t]; };
        [[maybe_unused]] auto ent_diag = [&](int v, int t) -> int64_t {
          if (v < 2) return diags[t];
          const int j = 64 * (v - 2) + t;
          return diag_c - (FRAG_VOTE_FAR - 1) + (j >= FRAG_XDIAGS ? j - FRAG_XDIAGS : j);
        };
        if constexpr (!ALL_DIAGS) {
          el[0] = __ballot(eligible(lane)); el[1] = __ballot(eligible(64 + lane));
          rank[0] = rank[1] = -1;
          for (int w = 0; w < 2; ++w) {
            if (!((el[w] >> lane) & 1ull)) continue;
            const FragInit me = inits[64 * w + lane];
            const int64_t md = diags[lane];
            int r = 0;
            for (int v = 0; v < 2; ++v)
              for (unsigned long long m = el[v]; m; m &= m - 1) {
                const int t = (int)__builtin_ctzll(m);
                if ((v != w || t != lane) && frag_init_before(inits[64 * v + t], diags[t], me, md)) ++r;
              }
            rank[w] = r;
          }
          n_elig = __popcll(el[0]) + __popcll(el[1]);
        } else {
          el[0] = __ballot(eligible(lane)); el[1] = __ballot(eligible(64 + lane));
          for (int k = 0; k < 3; ++k) el[2 + k] = __ballot(s_x[64 * k + lane].score > 0);
          n_elig = 0;
          for (int w = 0; w < NW; ++w) {
            n_elig += __popcll(el[w]);
            rank[w] = -1;
            if (!((el[w] >> lane) & 1ull)) continue;
            const FragInit me = ent(w, lane);
            const int64_t md = ent_diag(w, lane);
            int r = 0;
            for (int v = 0; v < NW; ++v)
              for (unsigned long long m = el[v]; m; m &= m - 1) {
                const int t = (int)__builtin_ctzll(m);
                if ((v != w || t != lane) && frag_init_before(ent(v, t), ent_diag(v, t), me, md)) ++r;
              }
            rank[w] = r;
          }
        }
        FragPrelim pre[BL_MAX_PRELIMS], first{0, 0, 0, 0, 0, 0, 0};
        int np = 0, tried = 0;
        for (int r = 0; r < n_elig && tried < BL_MAX_PRELIMS; ++r) {      // (uniform)
          FragInit J;
          int64_t dj;
          if constexpr (!ALL_DIAGS) {
            const unsigned long long m0 = __ballot(rank[0] == r), m1 = __ballot(rank[1] == r);
            const int x = m0 ? (int)__builtin_ctzll(m0) : 64 + (int)__builtin_ctzll(m1);
            J = inits[x];
            dj = diags[x & (FRAG_MAX_SEEDS - 1)];
          } else {
            int xv = -1, xt = 0;
            for (int w = NW - 1; w >= 0; --w) {
              const unsigned long long mw = __ballot(rank[w] == r);
              if (mw) { xv = w; xt = (int)__builtin_ctzll(mw); }
            }
            if (xv < 0) continue;      // (uniform; no entry of this rank means two of equal rank: frag_init_before is total on distinct (diagonal, q_start))
            J = ent(xv, xt);
            dj = ent_diag(xv, xt);
          }
          bool inside = false;
          for (int u = 0; u < np; ++u) inside = inside || frag_init_contained(J, dj, pre[u]);
          if (inside) continue;
          const int32_t g0 = frag_word_start(J.q_off, (int64_t)J.q_off + dj - s_lo, qlen);
          const int32_t as = (int32_t)(g0 + dj);
          const int32_t pq_r = qlen - (g0 + 1), pq_l = g0;
          int32_t ps_r = s_hi - (as + 1); if (ps_r > cap) ps_r = cap; if (ps_r < 0) ps_r = 0;
          int32_t ps_l = as - s_lo; if (ps_l > cap) ps_l = cap; if (ps_l < 0) ps_l = 0;
          __syncthreads();
          for (int32_t t = lane; t < pq_r; t += 64) s_q[t] = q_at(g0 + 1 + t);
          for (int32_t t = lane; t < ps_r; t += 64) s_s[t] = s_at(as + 1 + t);
          __syncthreads();
          const FragExt Rp = frag_extend_wave<ALL_DIAGS>(B, s_q, pq_r, s_s, ps_r, FRAG_NEG, FRAG_XDROP_PRELIM);
          __syncthreads();
          for (int32_t t = lane; t < pq_l; t += 64) s_q[t] = q_at(g0 - 1 - t);
          for (int32_t t = lane; t < ps_l; t += 64) s_s[t] = s_at(as - 1 - t);
          __syncthreads();
          const FragExt Lp = frag_extend_wave<ALL_DIAGS>(B, s_q, pq_l, s_s, ps_l, FRAG_NEG, FRAG_XDROP_PRELIM);
          const FragPrelim Pp{Rp.score + Lp.score + FRAG_MATCH, g0 - Lp.di, g0 + 1 + Rp.di, g0, (int64_t)as - Lp.dj, (int64_t)as + 1 + Rp.dj, dj};
          if (tried++ == 0) first = Pp;
          if (frag_evalue_ok_db(Pp.score, qlen, db_len, R.n_rec)) pre[np++] = Pp;
        }
        int bi = -1;
        for (int u = 0; u < np; ++u) if (bi < 0 || frag_prelim_before(pre[u], pre[bi])) bi = u;
        FragPrelim best = first;
        if (bi >= 0) best = pre[bi];
        const bool ok = bi >= 0 || (tried > 0 && first.score >= BL_PRELIM_RESCUE);
        __syncthreads();
        if (lane == 0 && ok) { s_pbest[c] = best; s_have[c] = 1; }
        __syncthreads();
        continue;      // (uniform)
      }
      if (!weak) {      // phase 1: blastn's start rule inside the best preliminary alignment's box
        const FragPrelim best = s_pbest[c];
        const int32_t rec_lo = s_lo - best.diag > 0 ? (int32_t)(s_lo - best.diag) : 0;
        DiagMatch match{s_qpk2[strand], s_qok2[strand], qlen, R.codes, R.mask, (int32_t)R.len, best.diag, (int64_t)s_lo, (int64_t)s_hi, -64, 0u};
        const int32_t g = frag_start_point_boxed(match, best.g, best.g + best.diag, best.q0, best.q1, best.s0, best.s1, rec_lo);
        A = FragSeed{(int32_t)(g + best.diag), g, 1};
      }
      // rightward
      const int32_t qmax_r = qlen - (A.q + A.len);
      int32_t smax_r = s_hi - (A.s + A.len); if (smax_r > cap) smax_r = cap; if (smax_r < 0) smax_r = 0;
      __syncthreads();
      for (int32_t t = lane; t < qmax_r; t += 64) s_q[t] = q_at(A.q + A.len + t);
      for (int32_t t = lane; t < smax_r; t += 64) s_s[t] = s_at(A.s + A.len + t);
      __syncthreads();
      // a chance hit gets blastn's PRELIMINARY look first (frag_hsp, pg_anib_core.h): X-drop 30 bits; what misses the e-value there is dropped
      FragExt Rp{0, 0, 0, 0, 0};
      if (weak) Rp = frag_extend_wave<ALL_DIAGS>(B, s_q, qmax_r, s_s, smax_r, FRAG_NEG, FRAG_XDROP_PRELIM);
      FragExt Rr = weak ? Rp : frag_extend_wave<ALL_DIAGS>(B, s_q, qmax_r, s_s, smax_r);
      // leftward
      const int32_t qmax_l = A.q;
      int32_t smax_l = A.s - s_lo; if (smax_l > cap) smax_l = cap; if (smax_l < 0) smax_l = 0;
      __syncthreads();
      for (int32_t t = lane; t < qmax_l; t += 64) s_q[t] = q_at(A.q - 1 - t);
      for (int32_t t = lane; t < smax_l; t += 64) s_s[t] = s_at(A.s - 1 - t);
      __syncthreads();
      FragExt Ll;
      bool dropped = false;
      if (weak) {
        const FragExt Lp = frag_extend_wave<ALL_DIAGS>(B, s_q, qmax_l, s_s, smax_l, FRAG_NEG, FRAG_XDROP_PRELIM);
        dropped = !frag_prelim_goes_on(Rp.score + Lp.score + FRAG_MATCH * A.len, [&](int32_t sc) { return frag_evalue_ok_db(sc, qlen, db_len, R.n_rec); });      // (uniform)
        Ll = Lp;
        if (!dropped) {      // it passed: the final alignment of both sides
          Ll = frag_extend_wave<ALL_DIAGS>(B, s_q, qmax_l, s_s, smax_l);
          __syncthreads();
          for (int32_t t = lane; t < qmax_r; t += 64) s_q[t] = q_at(A.q + A.len + t);
          for (int32_t t = lane; t < smax_r; t += 64) s_s[t] = s_at(A.s + A.len + t);
          __syncthreads();
          Rr = frag_extend_wave<ALL_DIAGS>(B, s_q, qmax_r, s_s, smax_r);
          __syncthreads();
          for (int32_t t = lane; t < qmax_l; t += 64) s_q[t] = q_at(A.q - 1 - t);
          for (int32_t t = lane; t < smax_l; t += 64) s_s[t] = s_at(A.s - 1 - t);
          __syncthreads();
        }
      } else {
        Ll = frag_extend_wave<ALL_DIAGS>(B, s_q, qmax_l, s_s, smax_l);
      }
      if (dropped) { __syncthreads(); continue; }      // (uniform)
      // the second look (pg_anib_core.h, frag_second_look): a side grown again under the floor the other side's total sets (uniform)
      const int32_t r_total = Rr.score + FRAG_MATCH * A.len, l_total = Ll.score;
      const bool again = frag_evalue_ok_db(r_total + l_total, qlen, db_len, R.n_rec);      // (a row that fails the e-value already is not looked at again)
      if (again && frag_second_look(r_total, Ll.score)) Ll = frag_extend_wave<ALL_DIAGS>(B, s_q, qmax_l, s_s, smax_l, -r_total);
      if (again && frag_second_look(l_total, Rr.score)) {
        __syncthreads();
        for (int32_t t = lane; t < qmax_r; t += 64) s_q[t] = q_at(A.q + A.len + t);
        for (int32_t t = lane; t < smax_r; t += 64) s_s[t] = s_at(A.s + A.len + t);
        __syncthreads();
        Rr = frag_extend_wave<ALL_DIAGS>(B, s_q, qmax_r, s_s, smax_r, -l_total);
      }
      if (lane == 0) {
        const FragHit h = frag_join(Ll, Rr, A.q, A.s, A.len);
        if (frag_evalue_ok_db(h.score, qlen, db_len, R.n_rec)) {
          FragRow r;
          r.frag = f; r.length = h.length; r.mismatch = h.mismatch; r.gaps = h.gaps; r.nident = h.nident; r.qlen = qlen;
          r.srec = srec; r.score = h.score;
          if (!strand) { r.qstart = h.qs + 1; r.qend = h.qe; r.sstart = h.ss - s_lo + 1; r.send = h.se - s_lo; }
          else { r.qstart = qlen - h.qe + 1; r.qend = qlen - h.qs; r.sstart = h.se - s_lo; r.send = h.ss - s_lo + 1; }
          // stable insertion, best score first
          int at = s_nrows;
          if (at == FRAG_ROWS) {      // full (a repeat family: up to FRAG_MAX_FINALS rows per strand): the lowest row goes
            if (s_rows[at - 1].score >= r.score) at = -1; else --at;
          }
          if (at >= 0) {
            while (at > 0 && s_rows[at - 1].score < r.score) { s_rows[at] = s_rows[at - 1]; --at; }
            s_rows[at] = r;
            if (s_nrows < FRAG_ROWS) s_nrows = s_nrows + 1;
          }
        }
      }
      __syncthreads();
    }
    }      // phase
  }
  __syncthreads();
  if (lane == 0) {
    // rows that share a start or an end point with a better one go (frag_rows_share_end), then -max_target_seqs 1: only the subject
    // record of the best row is reported
    int kept = 0;
    for (int i = 0; i < s_nrows; ++i) {
      const FragRow r = s_rows[i];
      bool drop = kept > 0 && r.srec != s_rows[0].srec;
      for (int k = 0; k < kept; ++k) drop = drop || frag_rows_share_end(s_rows[k].qstart, s_rows[k].qend, s_rows[k].sstart, s_rows[k].send, r.qstart, r.qend, r.sstart, r.send);
      if (!drop) s_rows[kept++] = r;
    }
    n_rows[slot] = (uint32_t)kept;
    for (int i = 0; i < kept; ++i) rows[(size_t)slot * FRAG_ROWS + i] = s_rows[i];
  }
}

// parse_blast_tab (pyani/anib.py:641-665) over the rows of one pair
__global__ __launch_bounds__(64) void anib_reduce_pairs_kernel(const FragPair* __restrict__ pairs, uint32_t n_pairs, const FragRow* __restrict__ rows,
                                                               const uint32_t* __restrict__ n_rows, pg_anib_result* __restrict__ out) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  const FragPair P = pairs[p];
  int64_t aln = 0, err = 0;
  double sum = 0.0;
  int32_t kept = 0;
  for (int32_t f = 0; f < P.n_frags; ++f) {
    const uint32_t slot = P.slot0 + (uint32_t)f;
    const uint32_t n = n_rows[slot];
    for (uint32_t i = 0; i < n; ++i) {
      const FragRow r = rows[(size_t)slot * FRAG_ROWS + i];
      const int32_t alnlen = r.length - r.gaps, ids = alnlen - r.mismatch;
      const double cov = (double)alnlen / (double)r.qlen, pid = (double)ids / (double)r.qlen;
      if (!(cov > 0.7 && pid > 0.3)) continue;
      // pident as BLAST prints it: 100 * nident / length to 3 decimals (round-half-even on the exact quotient = printf("%.3f"))
      const int64_t num = 100000ll * r.nident;
      int64_t milli = num / r.length;
      const int64_t rem2 = 2 * (num % r.length);
      if (rem2 > r.length || (rem2 == r.length && (milli & 1))) ++milli;
      aln += alnlen; err += (int64_t)r.mismatch + r.gaps;
      sum = sum + (double)milli / 1000.0;
      ++kept;
      break;
    }
  }
  pg_anib_result o;
  o.aln_length = aln; o.sim_errors = err; o.pid = kept ? sum / (double)kept : 0.0; o.n_frags = P.n_frags; o.n_kept = kept; o.status = 0; o.reserved = 0;
  out[p] = o;
}

// ---- packed rows of a launch (pg_anib_rows_batch) ---------------------------------------------------------------------------
// The tables of every pair of a launch, compacted on the device: an exclusive scan over the per-slot row counts gives every slot
// its place (off[slot]; off[n_slots] = the launch's rows), a pack pass copies the live rows there.  Slots in launch order are pairs
// in launch order and fragments in fragment order, rows of a slot keep their stored order (best score first): what the host loop
// over the padded scratch of pair 0 produces (anib_frag_stage), for every pair at once, with no atomics.  Launched after the word
// tier, so the rows are final.  The scan is the word scan's three passes with a bound (n_slots is no multiple of the tile) and
// wave shuffles in place of the LDS ladder: 4096 slots per block, then the <= 1024 block sums, then the add.
constexpr uint32_t ROWS_SCAN_TILE = 4096;         // slots per block: 1024 threads x 4
constexpr uint32_t ROWS_SCAN_MAX_BLOCKS = 1024;   // block sums one workgroup scans: 4 Mi slots per launch (ANIB_MAX_SLOTS)
static_assert(FRAG_ROWS == 4, "anib_rows_pack_kernel: one thread per (slot, row), four to a slot");
static_assert(sizeof(FragRow) == 48, "a row is three 16-byte accesses");

// inclusive scan of one value per thread over a workgroup of 1024 (16 waves); s_wave: 16 words of LDS
__device__ __forceinline__ uint32_t rows_block_scan(uint32_t v, uint32_t* s_wave) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(v, o, 64); if (lane >= (uint32_t)o) v += u; }
  if (lane == 63) s_wave[wave] = v;
  __syncthreads();
  if (wave == 0) {
    uint32_t w = lane < 16 ? s_wave[lane] : 0u;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) { const uint32_t u = __shfl_up(w, o, 64); if (lane >= (uint32_t)o) w += u; }
    if (lane < 16) s_wave[lane] = w;
  }
  __syncthreads();
  return v + (wave ? s_wave[wave - 1] : 0u);
}
__device__ __forceinline__ uint32_t rows_live(uint32_t n) { return n < (uint32_t)FRAG_ROWS ? n : (uint32_t)FRAG_ROWS; }

__global__ __launch_bounds__(1024) void anib_rows_scan1_kernel(const uint32_t* __restrict__ n_rows, uint32_t n_slots, uint32_t* __restrict__ off,
                                                               uint32_t* __restrict__ bsum) {
  __shared__ uint32_t s_wave[16];
  const uint32_t t = threadIdx.x, base = blockIdx.x * ROWS_SCAN_TILE + t * 4u;
  uint32_t a = 0, b = 0, c = 0, d = 0;
  if (base + 3u < n_slots) {
    const uint4 x = *reinterpret_cast<const uint4*>(n_rows + base);
    a = rows_live(x.x); b = rows_live(x.y); c = rows_live(x.z); d = rows_live(x.w);
  } else {
    if (base < n_slots) a = rows_live(n_rows[base]);
    if (base + 1u < n_slots) b = rows_live(n_rows[base + 1]);
    if (base + 2u < n_slots) c = rows_live(n_rows[base + 2]);
  }
  const uint32_t incl = rows_block_scan(a + b + c + d, s_wave), excl = incl - (a + b + c + d);
  if (base + 3u < n_slots) {
    *reinterpret_cast<uint4*>(off + base) = make_uint4(excl, excl + a, excl + a + b, excl + a + b + c);
  } else {
    if (base < n_slots) off[base] = excl;
    if (base + 1u < n_slots) off[base + 1] = excl + a;
    if (base + 2u < n_slots) off[base + 2] = excl + a + b;
  }
  if (t == 1023) bsum[blockIdx.x] = incl;
}
// n_blocks <= ROWS_SCAN_MAX_BLOCKS; *total = off[n_slots]
__global__ __launch_bounds__(1024) void anib_rows_scan2_kernel(uint32_t* __restrict__ bsum, uint32_t n_blocks, uint32_t* __restrict__ total) {
  __shared__ uint32_t s_wave[16];
  const uint32_t t = threadIdx.x;
  const uint32_t v0 = t < n_blocks ? bsum[t] : 0u;
  const uint32_t incl = rows_block_scan(v0, s_wave);
  if (t < n_blocks) bsum[t] = incl - v0;
  if (t == 1023) *total = incl;
}
__global__ __launch_bounds__(1024) void anib_rows_scan3_kernel(uint32_t* __restrict__ off, uint32_t n_slots, const uint32_t* __restrict__ bsum) {
  const uint32_t i = blockIdx.x * 1024u + threadIdx.x;
  if (i < n_slots) off[i] += bsum[i / ROWS_SCAN_TILE];
}

// One thread per (slot, row): the live rows of a slot go to packed[off[slot] + i].  The live lanes of a wave write consecutive
// 48-byte rows (three 16-byte stores each), so a wave's stores cover one contiguous span.  The first n_pairs threads also leave
// their pair's row count (off is complete: off[n_slots] = total).
__global__ __launch_bounds__(256) void anib_rows_pack_kernel(const FragRow* __restrict__ rows, const uint32_t* __restrict__ n_rows,
                                                             const uint32_t* __restrict__ off, uint32_t n_slots, const FragPair* __restrict__ pairs,
                                                             uint32_t n_pairs, FragRow* __restrict__ packed, uint32_t* __restrict__ pair_rows) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t < n_pairs) {
    const FragPair P = pairs[t];
    pair_rows[t] = off[P.slot0 + (uint32_t)P.n_frags] - off[P.slot0];
  }
  const uint32_t slot = t >> 2, i = t & 3u;
  if (slot >= n_slots || i >= rows_live(n_rows[slot])) return;
  const uint4* src = reinterpret_cast<const uint4*>(rows + (size_t)slot * FRAG_ROWS + i);
  uint4* dst = reinterpret_cast<uint4*>(packed + (size_t)off[slot] + i);
  const uint4 x0 = src[0], x1 = src[1], x2 = src[2];
  dst[0] = x0; dst[1] = x1; dst[2] = x2;
}
