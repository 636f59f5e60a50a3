// pgscr_abund.inc — part of pg_screen.hip: the gather's abundances (DESIGN.md §16.8).  pg_screen_gather_count_abund is the gather's count
// with the multiplicity a(query, k-mer) of every kept entry beside it (the front half's run lengths, pgscr_front.inc) and the queries' weights
// W and MW.  pg_screen_gather_abund runs AFTER a pg_screen_gather over such a count and gives every recorded row the statistics of the
// multiplicities of the k-mers it claimed: the entry (i, x) belongs to the row of the smallest rank among the holders of x that won in
// query i.  The pass reads the kept entries, their abundances, the index and the recorded rows; it writes none of them, and the rounds'
// kernels are not touched.  Integers throughout, in forms that do not depend on the order in which anything arrives.
//   W1 abund_rank_kernel       one thread per row: rank_of[query n + db] = the row's rank (q x n uint32, "none" elsewhere)
//   W2 abund_attribute_kernel  a wave per 64 entries; for each live entry the whole wave walks the k-mer's holders and reduces the minimum
//                              of rank_of over them; key = query << 48 | rank << 32 | abundance, ~0 = belongs to no row
//   W3 one radix sort of the keys: row r owns the sorted range [off[r], off[r + 1]), ascending by abundance inside it
//   W4 abund_stats_kernel      a workgroup per chunk of ABUND_CHUNK keys of a row: sum, sum of squares (two words), min, max by atomics;
//                              the median's two elements read where they stand; every key checked against its row
namespace {

constexpr unsigned long long ABUND_NO_ROW = ~0ull;      // the key of an entry that belongs to no row: a query is below 2^16 - 1, so no real key
constexpr uint32_t ABUND_CHUNK = 4096;                  // keys of one W4 workgroup: 16 a lane
// the control words (uint64): entries attributed | not attributed | holders walked | checks failed
enum { AC_ATTRIBUTED, AC_UNATTRIBUTED, AC_WALKED, AC_BAD, AC_WORDS };

// W1: the rows stand by query, then rank: the rank of row r = r - the first row of its query (a binary search over the rows before it)
__global__ __launch_bounds__(256) void abund_rank_kernel(const int32_t* __restrict__ row_q, const int32_t* __restrict__ row_db, uint64_t n_rows, uint32_t q, uint32_t n,
                                                          uint64_t cells, uint32_t* __restrict__ rank_of, uint32_t* __restrict__ row_rank,
                                                          unsigned long long* __restrict__ ctl) {
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += (uint64_t)gridDim.x * blockDim.x) {
    const int32_t qi = row_q[r], b = row_db[r];
    uint64_t lo = 0, hi = r;
    while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2u; if (row_q[mid] < qi) lo = mid + 1u; else hi = mid; }
    const uint64_t rank = r - lo, cell = (uint64_t)(uint32_t)qi * n + (uint32_t)b;
    row_rank[r] = GATHER_NONE;
    if (qi < 0 || (uint32_t)qi >= q || b < 0 || (uint32_t)b >= n || rank >= GATHER_MAX_RANKS || cell >= cells) { atomicAdd(&ctl[AC_BAD], 1ull); continue; }
    row_rank[r] = (uint32_t)rank;
    rank_of[cell] = (uint32_t)rank;
  }
}

struct RowEntries {      // the keys of row r: its unique
  typedef uint32_t Index;
  const uint32_t* row_unique;
  __device__ unsigned long long operator()(uint32_t r) const { return row_unique[r]; }
};
struct RowChunks {       // the W4 workgroups of row r: one or more
  typedef uint32_t Index;
  const uint32_t* row_unique;
  __device__ unsigned long long operator()(uint32_t r) const { const uint32_t m = row_unique[r]; return m ? (m + ABUND_CHUNK - 1u) / ABUND_CHUNK : 1u; }
};

// W2: as the claim kernel (pgscr_gather.inc), a wave takes 64 consecutive entries and ballots the live ones; for each of them the WHOLE
// wave walks the k-mer's holders member[start[g], start[g + 1]) — lane j takes holder j, j + 64, ... — keeps the minimum of rank_of over
// the holders it read, and a wave reduction gives the entry's rank.  Every index is checked against q, n, D, E and M; an entry that fails
// a check belongs to no row.
__global__ __launch_bounds__(256) void abund_attribute_kernel(const unsigned long long* __restrict__ entry, const uint32_t* __restrict__ abund, uint64_t m_entries,
                                                               const unsigned long long* __restrict__ start, const uint32_t* __restrict__ member, uint64_t D, uint64_t E,
                                                               const uint32_t* __restrict__ rank_of, uint32_t q, uint32_t n, uint64_t cells,
                                                               unsigned long long* __restrict__ key_out, unsigned long long* __restrict__ ctl) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  unsigned long long attributed = 0ull, unattributed = 0ull, walked = 0ull;      // (the wave's: the same in every lane)
  for (uint64_t base = wave * 64ull; base < m_entries; base += n_waves * 64ull) {      // (uniform over the wave)
    const uint64_t e = base + lane;
    bool live = false;
    uint32_t qi = GATHER_NONE, m = 0u, mine = GATHER_NONE;
    unsigned long long s = 0ull;
    if (e < m_entries) {
      const unsigned long long x = entry[e];
      if (x != GATHER_DEAD) {
        qi = (uint32_t)(x >> GATHER_G_BITS);
        const unsigned long long g = x & GATHER_G_MASK;
        if (qi < q && g < D) {
          s = start[g];
          const unsigned long long e1 = start[g + 1ull];
          if (s < e1 && e1 <= E && e1 - s <= (unsigned long long)n) { live = true; m = (uint32_t)(e1 - s); }
        }
      }
    }
    unsigned long long bal = __ballot(live);
    while (bal) {
      const int src = __ffsll((long long)bal) - 1;
      bal &= bal - 1ull;
      const uint32_t cq = __shfl(qi, src, 64), cm = __shfl(m, src, 64);
      const unsigned long long cs = __shfl(s, src, 64);
      uint32_t best = GATHER_NONE;
      for (uint32_t j = lane; j < cm; j += 64u) {
        const uint32_t col = member[cs + j];
        const uint64_t cell = (uint64_t)cq * n + col;
        if (col < n && cell < cells) { const uint32_t r = rank_of[cell]; best = r < best ? r : best; }
      }
      for (int d = 32; d > 0; d >>= 1) { const uint32_t other = __shfl_xor(best, d, 64); best = other < best ? other : best; }
      if ((int)lane == src) mine = best;
      walked += cm;
    }
    const bool has_row = live && mine < GATHER_MAX_RANKS;
    attributed += (unsigned long long)__popcll(__ballot(has_row));
    unattributed += (unsigned long long)__popcll(__ballot(e < m_entries && !has_row));
    if (e < m_entries) key_out[e] = has_row ? ((unsigned long long)qi << 48) | ((unsigned long long)mine << 32) | abund[e] : ABUND_NO_ROW;
  }
  if (lane == 0u) {
    if (attributed) atomicAdd(&ctl[AC_ATTRIBUTED], attributed);
    if (unattributed) atomicAdd(&ctl[AC_UNATTRIBUTED], unattributed);
    if (walked) atomicAdd(&ctl[AC_WALKED], walked);
  }
}

// W4: workgroup c (and c + the grid, ...) owns chunk c: the row whose chunks hold it (binary search over coff), and the keys
// [off[r] + k CHUNK, ... + CHUNK) of that row's range.  Every key must carry the row's (query, rank) in its upper half; the lower half is
// the abundance a < 2^32.  Per lane: sum a (below 2^64: fewer than 2^32 keys), sum a^2 in two words with the carry taken at every
// addition; wave and workgroup reductions of the same form; then one atomic per statistic and workgroup — the carry into the high word
// of the sum of squares comes from the old value the low word's atomic returns, so the 128-bit total is the same in any order.  The keys
// of a row stand ascending by abundance: the chunk-0 workgroup reads the median's two elements where they stand.  The first key after the
// last row's range must be ABUND_NO_ROW, or the end.  A violation counts into ctl[AC_BAD].
__global__ __launch_bounds__(256) void abund_stats_kernel(const unsigned long long* __restrict__ sorted, uint64_t m_entries, const int32_t* __restrict__ row_q,
                                                           const uint32_t* __restrict__ row_rank, const unsigned long long* __restrict__ off,
                                                           const unsigned long long* __restrict__ coff, uint32_t n_rows, unsigned long long n_chunks,
                                                           unsigned long long* __restrict__ sum_out, unsigned long long* __restrict__ sumsq_out,
                                                           unsigned long long* __restrict__ median2_out, uint32_t* __restrict__ min_out, uint32_t* __restrict__ max_out,
                                                           unsigned long long* __restrict__ ctl) {
  __shared__ unsigned long long w_sum[4], w_lo[4], w_hi[4];
  __shared__ uint32_t w_min[4], w_max[4], w_bad[4];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  if (blockIdx.x == 0u && threadIdx.x == 0u) {
    const unsigned long long total = off[n_rows];
    if (total > m_entries || (total < m_entries && sorted[total] != ABUND_NO_ROW)) atomicAdd(&ctl[AC_BAD], 1ull);
  }
  for (unsigned long long c = blockIdx.x; c < n_chunks; c += gridDim.x) {      // (uniform over the workgroup)
    uint32_t lo = 0, hi = n_rows - 1u;      // the row of chunk c: the last one whose first chunk is <= c
    while (lo < hi) { const uint32_t mid = (lo + hi + 1u) >> 1; if (coff[mid] <= c) lo = mid; else hi = mid - 1u; }
    const uint32_t r = lo;
    const unsigned long long a = off[r], b = off[r + 1u], k = c - coff[r];
    const unsigned long long c0 = a + k * ABUND_CHUNK, c1 = c0 + ABUND_CHUNK < b ? c0 + ABUND_CHUNK : b;
    const unsigned long long want = ((unsigned long long)(uint32_t)row_q[r] << 16) | row_rank[r];
    unsigned long long sum = 0ull, sq_lo = 0ull, sq_hi = 0ull;
    uint32_t mn = ~0u, mx = 0u, bad = (b > m_entries || row_rank[r] >= GATHER_MAX_RANKS || c0 > b) ? 1u : 0u;
    if (!bad) {
      for (unsigned long long i = c0 + threadIdx.x; i < c1; i += 256ull) {
        const unsigned long long x = sorted[i];
        if ((x >> 32) != want) { bad = 1u; continue; }
        const uint32_t v = (uint32_t)x;
        const unsigned long long sq = (unsigned long long)v * v;
        sum += v;
        sq_lo += sq; sq_hi += sq_lo < sq ? 1ull : 0ull;
        mn = v < mn ? v : mn; mx = v > mx ? v : mx;
      }
    }
    for (int d = 32; d > 0; d >>= 1) {
      const unsigned long long o_sum = __shfl_down(sum, d, 64), o_lo = __shfl_down(sq_lo, d, 64), o_hi = __shfl_down(sq_hi, d, 64);
      const uint32_t o_mn = __shfl_down(mn, d, 64), o_mx = __shfl_down(mx, d, 64), o_bad = __shfl_down(bad, d, 64);
      sum += o_sum;
      sq_lo += o_lo; sq_hi += o_hi + (sq_lo < o_lo ? 1ull : 0ull);
      mn = o_mn < mn ? o_mn : mn; mx = o_mx > mx ? o_mx : mx; bad |= o_bad;
    }
    if (lane == 0u) { w_sum[wv] = sum; w_lo[wv] = sq_lo; w_hi[wv] = sq_hi; w_min[wv] = mn; w_max[wv] = mx; w_bad[wv] = bad; }
    __syncthreads();
    if (threadIdx.x == 0u) {
      for (uint32_t w = 1; w < 4u; ++w) {
        sum += w_sum[w];
        sq_lo += w_lo[w]; sq_hi += w_hi[w] + (sq_lo < w_lo[w] ? 1ull : 0ull);
        mn = w_min[w] < mn ? w_min[w] : mn; mx = w_max[w] > mx ? w_max[w] : mx; bad |= w_bad[w];
      }
      if (bad) atomicAdd(&ctl[AC_BAD], 1ull);
      else if (c0 < c1) {
        atomicAdd(&sum_out[r], sum);
        const unsigned long long old = atomicAdd(&sumsq_out[2ull * r], sq_lo);
        const unsigned long long up = sq_hi + (old + sq_lo < old ? 1ull : 0ull);
        if (up) atomicAdd(&sumsq_out[2ull * r + 1ull], up);
        atomicMin(&min_out[r], mn);
        atomicMax(&max_out[r], mx);
        if (k == 0ull) {      // twice the median, exact for both parities (a <= the two indices < b <= M)
          const unsigned long long m = b - a;
          median2_out[r] = (unsigned long long)(uint32_t)sorted[a + (m - 1ull) / 2ull] + (unsigned long long)(uint32_t)sorted[a + m / 2ull];
        }
      }
    }
    __syncthreads();
  }
}

// every device buffer of one pg_screen_gather_abund: gone with the call unless it is moved into the state
struct AbundWork {
  PgDevBuf<uint32_t> rank_of, row_rank, mn, mx;
  PgDevBuf<unsigned long long> key_a, key_b, wts, off, coff, ctl, sum, sumsq, median2;
  PgDevBuf<uint8_t> tmp;
};

// The pass, after the checks: returns with an error code or the work issued and its counts read.
int abund_run(pg_ctx* ctx, SearchState* I, AbundWork& W, ScreenEvents& T, unsigned long long* ctl) {
  hipStream_t st = ctx->stream;
  const uint32_t q = I->q, n = I->n, cu_blocks = (uint32_t)ctx->num_cu * 8u;
  const uint64_t cells = (uint64_t)q * n, M = I->M, R = I->n_rows;
  int rc;
  if (R >= (1ull << 32)) return pg_fail(ctx, PG_E_INTERNAL, "screen: 2^32 rows or more");
  if (W.rank_of.reserve((size_t)cells) != hipSuccess) {
    (void)hipGetLastError();
    return pg_fail(ctx, PG_E_NOMEM, "screen: no device memory for the rank table of an abundance pass: " + std::to_string(q) + " x " + std::to_string(n) + " uint32, " +
                                        std::to_string(cells * 4ull) + " bytes");
  }
  if ((rc = pg_dev_alloc(ctx, "screen", W.row_rank, (size_t)R, "the rows' ranks")) || (rc = pg_dev_alloc(ctx, "screen", W.key_a, (size_t)M, "the keys of an abundance pass")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.key_b, (size_t)M, "the keys of an abundance pass")) || (rc = pg_dev_alloc(ctx, "screen", W.wts, (size_t)R + 1, "the rows' ranges")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.off, (size_t)R + 1, "the rows' ranges")) || (rc = pg_dev_alloc(ctx, "screen", W.coff, (size_t)R + 1, "the rows' ranges")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.ctl, AC_WORDS, "the control words")) || (rc = pg_dev_alloc(ctx, "screen", W.sum, (size_t)R, "the rows' statistics")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.sumsq, 2 * (size_t)R, "the rows' statistics")) || (rc = pg_dev_alloc(ctx, "screen", W.median2, (size_t)R, "the rows' statistics")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.mn, (size_t)R, "the rows' statistics")) || (rc = pg_dev_alloc(ctx, "screen", W.mx, (size_t)R, "the rows' statistics")))
    return rc;
  size_t tmp_bytes = 0;
  PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& b) { return hipcub::DeviceScan::ExclusiveSum(nullptr, b, W.wts.p, W.off.p, (int64_t)(R + 1), st); }));
  PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& b) {
    return hipcub::DeviceRadixSort::SortKeys(nullptr, b, (const unsigned long long*)W.key_a.p, W.key_b.p, (int64_t)std::max<uint64_t>(M, 1), 0, 64, st); }));
  if ((rc = pg_dev_alloc(ctx, "screen", W.tmp, tmp_bytes + 16, "the sort's temporary storage"))) return rc;
  PG_HIP(ctx, hipMemsetAsync(W.ctl, 0, AC_WORDS * 8, st));
  PG_HIP(ctx, hipMemsetAsync(W.sum, 0, (size_t)R * 8, st));
  PG_HIP(ctx, hipMemsetAsync(W.sumsq, 0, (size_t)R * 16, st));
  PG_HIP(ctx, hipMemsetAsync(W.median2, 0, (size_t)R * 8, st));
  PG_HIP(ctx, hipMemsetAsync(W.mn, 0xFF, (size_t)R * 4, st));
  PG_HIP(ctx, hipMemsetAsync(W.mx, 0, (size_t)R * 4, st));
  unsigned long long total = 0, n_chunks = 0;
  {      // the rank table, the rows' ranges and chunks, every entry's key
    ScreenEvents::Stage attribute(T, ST_ATTRIBUTE, st);
    PG_HIP(ctx, hipMemsetAsync(W.rank_of, 0xFF, (size_t)cells * 4, st));
    hipLaunchKernelGGL(abund_rank_kernel, dim3(grid_for(R, 256, cu_blocks)), dim3(256), 0, st, (const int32_t*)I->d_row_q.p, (const int32_t*)I->d_row_db.p, R, q, n, cells,
                       W.rank_of.p, W.row_rank.p, W.ctl.p);
    PG_HIP(ctx, hipGetLastError());
    size_t tb = tmp_bytes;
    PG_HIP(ctx, screen_weights(ctx, R, W.wts.p, RowEntries{I->d_row_unique.p}));
    PG_HIP(ctx, hipcub::DeviceScan::ExclusiveSum((void*)W.tmp.p, tb, W.wts.p, W.off.p, (int64_t)(R + 1), st));
    tb = tmp_bytes;
    PG_HIP(ctx, screen_weights(ctx, R, W.wts.p, RowChunks{I->d_row_unique.p}));
    PG_HIP(ctx, hipcub::DeviceScan::ExclusiveSum((void*)W.tmp.p, tb, W.wts.p, W.coff.p, (int64_t)(R + 1), st));
    if (M) {
      hipLaunchKernelGGL(abund_attribute_kernel, dim3(grid_for(M, 256, cu_blocks)), dim3(256), 0, st, (const unsigned long long*)I->d_entry.p, (const uint32_t*)I->d_abund.p, M,
                         (const unsigned long long*)I->d_start.p, (const uint32_t*)I->d_member.p, I->D, I->E, (const uint32_t*)W.rank_of.p, q, n, cells, W.key_a.p, W.ctl.p);
      PG_HIP(ctx, hipGetLastError());
    }
  }
  PG_HIP(ctx, hipMemcpyAsync(&total, W.off.p + R, 8, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipMemcpyAsync(&n_chunks, W.coff.p + R, 8, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipMemcpyAsync(ctl, W.ctl, AC_WORDS * 8, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipStreamSynchronize(st));
  if (ctl[AC_BAD]) return pg_fail(ctx, PG_E_INTERNAL, "screen: a recorded row of a gather names no cell of the rectangle");
  if (total > M || n_chunks < R || n_chunks > total / ABUND_CHUNK + R)
    return pg_fail(ctx, PG_E_INTERNAL, "screen: the rows of a gather claim " + std::to_string(total) + " of " + std::to_string(M) + " entries");
  if (ctl[AC_ATTRIBUTED] != total || ctl[AC_ATTRIBUTED] + ctl[AC_UNATTRIBUTED] != M)
    return pg_fail(ctx, PG_E_INTERNAL, "screen: " + std::to_string(ctl[AC_ATTRIBUTED]) + " entries belong to a row where the rows' unique add up to " + std::to_string(total));
  if (M) {
    ScreenEvents::Stage sort(T, ST_SORT, st);
    size_t tb = tmp_bytes;
    PG_HIP(ctx, hipcub::DeviceRadixSort::SortKeys((void*)W.tmp.p, tb, (const unsigned long long*)W.key_a.p, W.key_b.p, (int64_t)M, 0, 64, st));
  }
  {
    ScreenEvents::Stage stats(T, ST_STATS, st);
    hipLaunchKernelGGL(abund_stats_kernel, dim3(grid_for(n_chunks, 1, cu_blocks * 4u)), dim3(256), 0, st, (const unsigned long long*)W.key_b.p, M, (const int32_t*)I->d_row_q.p,
                       (const uint32_t*)W.row_rank.p, (const unsigned long long*)W.off.p, (const unsigned long long*)W.coff.p, (uint32_t)R, n_chunks, W.sum.p, W.sumsq.p,
                       W.median2.p, W.mn.p, W.mx.p, W.ctl.p);
    PG_HIP(ctx, hipGetLastError());
  }
  PG_HIP(ctx, hipMemcpyAsync(ctl, W.ctl, AC_WORDS * 8, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipStreamSynchronize(st));
  if (ctl[AC_BAD]) return pg_fail(ctx, PG_E_INTERNAL, "screen: the sorted keys of an abundance pass do not stand in their rows' ranges");
  return PG_OK;
}

}  // namespace

extern "C" int pg_screen_gather_count_abund(pg_ctx* ctx, const int32_t* query_ids, uint32_t q, uint32_t* sizes_out, uint64_t* weight_out) {
  return search_count(ctx, query_ids, q, sizes_out, KEEP_ABUND, weight_out);
}

extern "C" int pg_screen_gather_abund(pg_ctx* ctx, uint64_t* n_rows_out) {
  if (!ctx) return PG_E_ARG;
  SearchState* I = search_of(ctx);
  if (!I) return pg_fail(ctx, PG_E_ARG, "screen: no resident search index (call pg_screen_search_index first)");
  if (!I->counted || !I->kept || !I->abund_kept) return pg_fail(ctx, PG_E_ARG, "screen: the latest count kept no abundances (call pg_screen_gather_count_abund first)");
  if (!I->gathered) return pg_fail(ctx, PG_E_ARG, "screen: no gathered rows since that count (call pg_screen_gather first)");
  if (!n_rows_out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PgScreenGatherAbundStats& L = ctx->screen_gather_abund_stats;
  if (I->q == 0 || I->n_rows == 0) {      // (no rows: every entry belongs to none)
    I->drop_abund_rows();
    I->abund_done = true;
    L.attributed = L.walked = L.rank_bytes = 0;
    L.unattributed = I->M;
    L.attribute_ms = L.sort_ms = L.stats_ms = 0.0;
    *n_rows_out = 0;
    return PG_OK;
  }
  AbundWork W;
  ScreenEvents T;
  unsigned long long ctl[AC_WORDS] = {0, 0, 0, 0};
  const int rc = abund_run(ctx, I, W, T, ctl);
  const hipError_t es = hipStreamSynchronize(ctx->stream);      // (on errors too: W goes with this scope)
  if (rc) return rc;
  PG_HIP(ctx, es);
  I->d_ab_sum = std::move(W.sum); I->d_ab_sumsq = std::move(W.sumsq); I->d_ab_median2 = std::move(W.median2);
  I->d_ab_min = std::move(W.mn); I->d_ab_max = std::move(W.mx);
  I->n_abund_rows = I->n_rows;
  I->abund_done = true;
  L.attributed = ctl[AC_ATTRIBUTED]; L.unattributed = ctl[AC_UNATTRIBUTED]; L.walked = ctl[AC_WALKED];
  L.rank_bytes = (uint64_t)I->q * I->n * 4ull;
  L.attribute_ms = T.ms(ST_ATTRIBUTE); L.sort_ms = T.ms(ST_SORT); L.stats_ms = T.ms(ST_STATS);
  *n_rows_out = I->n_abund_rows;
  return PG_OK;
}

extern "C" int pg_screen_gather_abund_read(pg_ctx* ctx, uint64_t* sum_out, uint64_t* sumsq_out, uint64_t* median2_out, uint32_t* min_out, uint32_t* max_out) {
  if (!ctx) return PG_E_ARG;
  SearchState* I = search_of(ctx);
  if (!I || !I->abund_done) return pg_fail(ctx, PG_E_ARG, "screen: no abundance statistics (call pg_screen_gather_abund first)");
  if (I->n_abund_rows == 0) return PG_OK;
  if (!sum_out || !sumsq_out || !median2_out || !min_out || !max_out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  const uint64_t R = I->n_abund_rows;
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PG_HIP(ctx, hipMemcpyAsync(sum_out, I->d_ab_sum, R * 8, hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipMemcpyAsync(sumsq_out, I->d_ab_sumsq, R * 16, hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipMemcpyAsync(median2_out, I->d_ab_median2, R * 8, hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipMemcpyAsync(min_out, I->d_ab_min, R * 4, hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipMemcpyAsync(max_out, I->d_ab_max, R * 4, hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PG_OK;
}

extern "C" int pg_screen_gather_abund_matched(pg_ctx* ctx, uint64_t* matched_weight_out) {
  if (!ctx) return PG_E_ARG;
  SearchState* I = search_of(ctx);
  if (!I || !I->counted || !I->kept || !I->abund_kept)
    return pg_fail(ctx, PG_E_ARG, "screen: the latest count kept no abundances (call pg_screen_gather_count_abund first)");
  if (I->q == 0) return PG_OK;
  if (!matched_weight_out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PG_HIP(ctx, hipMemcpyAsync(matched_weight_out, I->d_matched_weight, (size_t)I->q * 8, hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PG_OK;
}

extern "C" int pg_screen_gather_abund_last(pg_ctx* ctx, uint64_t* counts_out, double* ms_out) {
  if (!ctx || !counts_out || !ms_out) return pg_fail(ctx, PG_E_ARG, "bad argument");
  const PgScreenGatherAbundStats& L = ctx->screen_gather_abund_stats;
  counts_out[0] = L.attributed; counts_out[1] = L.unattributed; counts_out[2] = L.walked; counts_out[3] = L.rank_bytes;
  ms_out[0] = L.weight_ms; ms_out[1] = L.attribute_ms; ms_out[2] = L.sort_ms; ms_out[3] = L.stats_ms;
  return PG_OK;
}
