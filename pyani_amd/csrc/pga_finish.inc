// pga_finish.inc — part of pg_anim.hip (included inside its anonymous namespace; not a translation unit of its own):
// A5: the 1-to-1 filter (delta-filter -1) and the parse_delta reduction over the postnuc stage's alignments.

struct FinishScratch {   // per-alignment arrays: pair p owns the slice [moff[2p], moff[2p+2])
  Aln* alns;
  int32_t* a_rrec;
  int32_t* a_qrec;
  int32_t* idx;
  int32_t* from;
  double* sc;
};

// pga::lis_filter with the O(n^2) look-back spread over the lanes of one wave.  Every lane runs the (cheap) serial parts
// redundantly and writes identical values, so no intra-wave memory ordering is needed; candidates are evaluated by the
// same expression as the scalar code and the reduction keeps its tie rule (the earliest predecessor reaching the max).
__device__ void lis_filter_wave(Aln* a, int n, int side, const int32_t* grp, const int32_t* ogrp, int32_t* idx, double* sc_, int32_t* from) {
  const int lane = threadIdx.x & 63;
  int64_t* sc = reinterpret_cast<int64_t*>(sc_);
  auto lo = [&](int i) { return side == 0 ? a[i].rs : a[i].qs; };
  auto hi = [&](int i) { return side == 0 ? a[i].re : a[i].qe; };
  auto olo = [&](int i) { return side == 0 ? a[i].qs : a[i].rs; };
  bool ok;
  for (int i = 0; i < n; ++i) { idx[i] = i; sc[i] = lis_gain(hi(i) - lo(i), 1, 0, lis_idy(a[i]), ok); }
  heapsort(idx, n, [&](int x, int y) {
    if (grp[x] != grp[y]) return grp[x] < grp[y];
    if (lo(x) != lo(y)) return lo(x) < lo(y);
    if (sc[x] != sc[y]) return sc[x] > sc[y];
    if (ogrp[x] != ogrp[y]) return ogrp[x] < ogrp[y];
    if (olo(x) != olo(y)) return olo(x) < olo(y);
    if (a[x].strand != a[y].strand) return a[x].strand < a[y].strand;
    return x < y; });
  int g0 = 0;
  while (g0 < n) {
    int g1 = g0;
    while (g1 < n && grp[idx[g1]] == grp[idx[g0]]) ++g1;
    int best = -1;
    for (int k = g0; k < g1; ++k) {
      const int i = idx[k];
      const int64_t len = hi(i) - lo(i);
      const double idy = lis_idy(a[i]);
      const int32_t lo_i = lo(i);
      long long bc = sc[i];   // own score; this lane's best candidate and its predecessor's rank (kk)
      int bk = 0x7FFFFFFF;
      for (int kk = g0 + lane; kk < k; kk += 64) {
        const int j = idx[kk];
        int64_t ol = (int64_t)hi(j) - lo_i;
        if (ol < 0) ol = 0;
        bool allowed;
        const int64_t g = lis_gain(len, hi(j) - lo(j), ol, idy, allowed);
        if (!allowed) continue;
        const long long cand = sc[j] + g;
        if (cand > bc) { bc = cand; bk = kk; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const long long oc = __shfl_xor(bc, o, 64);
        const int ok2 = __shfl_xor(bk, o, 64);
        if (oc > bc || (oc == bc && ok2 < bk)) { bc = oc; bk = ok2; }
      }
      sc[i] = bc;
      from[i] = bk == 0x7FFFFFFF ? -1 : idx[bk];
      if (best < 0 || sc[i] > sc[best]) best = i;
    }
    for (int i = best; i >= 0; i = from[i]) a[i].keep |= (1 << side);
    g0 = g1;
  }
}

// One WAVE per ordered pair: both strands' alignments, 1-to-1 filter, parse_delta reduction.
__global__ __launch_bounds__(64) void anim_finish_kernel(const RefDesc* __restrict__ refs, const UnitDesc* __restrict__ units, uint32_t n_pairs,
                                                         ClusterOut O, const pgn::PnAln* __restrict__ pn, const int32_t* __restrict__ pn_n,
                                                         FinishScratch S, int filter_1to1, pg_anim_result* __restrict__ out) {
  const uint32_t p = blockIdx.x;
  if (p >= n_pairs) return;
  const RefDesc R = refs[units[2 * p].ref];
  const size_t poff = O.moff[2 * p];
  const int cap_a = (int)(O.moff[2 * p + 2] - O.moff[2 * p]);
  Aln* alns = S.alns + poff;
  int32_t* a_rrec = S.a_rrec + poff;
  int32_t* a_qrec = S.a_qrec + poff;
  int32_t* idx = S.idx + poff;
  int32_t* from = S.from + poff;
  double* sc = S.sc + poff;
  int n = 0;
  bool pn_short = false;
  for (int strand = 0; strand < 2; ++strand) {
    const uint32_t u = 2 * p + strand;  // units are laid out pair-major: (pair, fwd), (pair, rev)
    const UnitDesc U = units[u];
    const size_t off = O.moff[u];
    const int before = n;
    {   // the postnuc stage's alignments (inclusive stream coordinates) as they are
      int na = pn_n[u];
      if (na < 0) { pn_short = true; na = -1 - na; }
      for (int i = 0; i < na && n < cap_a; ++i) {
        const pgn::PnAln x = pn[off + i];
        alns[n++] = Aln{x.sA, x.eA + 1, x.sB, x.eB + 1, x.errors, strand, 0};
      }
    }
    for (int i = before; i < n; ++i) {
      Aln& a = alns[i];
      a_rrec[i] = record_of(R.rec_start, R.n_rec, a.rs);
      if (strand) { const int32_t qs = U.len - a.qe, qe = U.len - a.qs; a.qs = qs; a.qe = qe; }  // forward coordinates
      a_qrec[i] = record_of(U.rec_start, U.n_rec, a.qs);
    }
  }
  if (filter_1to1) {
    lis_filter_wave(alns, n, 0, a_rrec, a_qrec, idx, sc, from);
    lis_filter_wave(alns, n, 1, a_qrec, a_rrec, idx, sc, from);
  } else {
    for (int i = 0; i < n; ++i) alns[i].keep = 3;
  }
  const PairResult r = reduce_pair(alns, n, a_rrec, a_qrec, idx);
  pg_anim_result o;
  o.ref_aln_len = r.ref_aln_len;
  o.qry_aln_len = r.qry_aln_len;
  o.sim_errors = r.sim_errors;
  o.n_alignments = r.n_alignments;
  o.identity = r.aligned > 0 ? (double)r.weighted / (double)r.aligned : 0.0;  // int/int true division (anim.py:396)
  o.status = (O.status[p] || pn_short) ? PG_E_CAPACITY : (r.n_alignments == 0 ? PG_ANIM_NO_ALIGNMENT : 0);
  o.reserved = n;   // alignments before the filter
  if ((threadIdx.x & 63) == 0) out[p] = o;
}

// reduction of caller-supplied alignment records (pg_anim_reduce): one thread per pair
__global__ __launch_bounds__(64) void anim_reduce_kernel(uint32_t n_pairs, const uint64_t* __restrict__ offsets, Aln* alns,
                                                         const int32_t* __restrict__ rgrp, const int32_t* __restrict__ qgrp,
                                                         int32_t* idx, int32_t* from, double* sc, int apply_filter,
                                                         pg_anim_result* __restrict__ out) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  const uint64_t o = offsets[p];
  const int n = (int)(offsets[p + 1] - o);
  if (apply_filter) {
    lis_filter(alns + o, n, 0, rgrp + o, qgrp + o, idx + o, sc + o, from + o);
    lis_filter(alns + o, n, 1, qgrp + o, rgrp + o, idx + o, sc + o, from + o);
  }
  const PairResult r = reduce_pair(alns + o, n, rgrp + o, qgrp + o, idx + o);
  pg_anim_result res;
  res.ref_aln_len = r.ref_aln_len; res.qry_aln_len = r.qry_aln_len; res.sim_errors = r.sim_errors;
  res.n_alignments = r.n_alignments;
  res.identity = r.aligned > 0 ? (double)r.weighted / (double)r.aligned : 0.0;
  res.status = r.n_alignments == 0 ? PG_ANIM_NO_ALIGNMENT : 0;
  res.reserved = 0;
  out[p] = res;
}
