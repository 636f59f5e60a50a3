// pg_tree.hip — neighbour joining on the GPU: the unrooted tree of a distance matrix.  fp64 VALU work; no MFMA.
//
// Contract: the joins and the branch lengths are EQUAL, bit for bit, to pyani_amd.tree.nj_of_matrix, the numpy statement: every
// operation below is rounded on its own (-ffp-contract=off in the build line), the row sums are carried and UPDATED as the statement
// updates them, never re-summed, and a tie of the criterion goes to the smallest (lower node id, higher node id).  Because ties are
// decided by node id and not by where a node is stored, the matrix may be laid out as the device likes: the live nodes are kept in
// slots 0 .. m - 1 of the symmetric n x n square (the new node takes the lower slot of the joined pair, the last live slot moves into
// the higher one), so that every step scans m (m - 1) / 2 cells and no dead one.
//
//   K1 nj_check_kernel    finite, symmetric bit for bit, zero diagonal: one workgroup per 64 x 64 tile of the upper triangle; the
//                         mirrored tile goes through LDS so that both reads are contiguous.
//   K2 nj_rowsum_kernel   r[i] = sum over k ascending of d[k][i] (= d[i][k]), one thread per row, reads down the columns.
//   K3 nj_argmin_kernel   wide step, first half: Q(i, j) = (m - 2) d(i, j) - (r[i] + r[j]) over the 64 x 64 tiles (bi <= bj) of the live
//                         upper triangle, the smallest (Q, lower id, higher id) per thread, per wave by shuffles, per workgroup
//                         through LDS; one partial per workgroup, with the number of cells it evaluated.
//   K4 nj_join_kernel     wide step, second half, one workgroup: reduces the partials, writes the record, the new row and its mirrored
//                         column, updates r, moves the last live slot into the freed one and keeps the slot -> id table.
//   K5 nj_tail_kernel     one workgroup runs every remaining step from m <= tail_limit down to 3 with workgroup barriers (below that
//                         size a launch costs more than the scan) and writes the three last branches; the whole problem for small n.
//
// Kernel boundaries are the only ordering between workgroups; the host knows m at every step and reads nothing back inside the loop.
// A non-finite Q or row sum raises the flag; every later launch leaves at once and the call returns PG_E_NONFINITE.
#include <algorithm>
#include <vector>

#include "pg_internal.h"
#include "pg_devbuf.h"

namespace {

constexpr uint32_t NJ_MAX_N = 8192, NJ_TILE = 64, NJ_THREADS = 256, NJ_WG = 1024, NJ_TAIL_MAX = 1024;
constexpr int NJ_F_NONFINITE = 1, NJ_F_ASYM = 2, NJ_F_DIAG = 4;
constexpr double NJ_DBL_MAX = 1.79769313486231570815e308;

struct NjBest {      // a candidate pair: the criterion, its node ids as (lower id << 32 | higher id), and the cells counted on the way
  double q;
  unsigned long long key;
  uint32_t cells, pad;
};

struct NjState {
  double* w;           // n x n working matrix, the live nodes in slots 0 .. m - 1
  double* r;           // row sums by slot
  int32_t* ids;        // slot -> node id
  int32_t* join;       // (n - 3) x 2
  double* len;         // (n - 3) x 2
  int32_t* last;       // 3
  double* last_len;    // 3
  NjBest* partial;     // one per workgroup of the arg-min
  unsigned long long* cells;
  int* flag;
  uint32_t n;
};

__device__ __forceinline__ bool nj_finite(double x) { return fabs(x) <= NJ_DBL_MAX; }

__device__ __forceinline__ NjBest nj_none() {
  NjBest b;
  b.q = __longlong_as_double(0x7ff0000000000000ll);      // +inf: any finite Q is smaller
  b.key = ~0ull;
  b.cells = b.pad = 0;
  return b;
}

// (Q, lower id, higher id) lexicographically; Q by <, so -0 equals +0
__device__ __forceinline__ bool nj_less(double q, unsigned long long key, const NjBest& b) {
  if (q < b.q) return true;
  if (b.q < q) return false;
  return key < b.key;
}

__device__ __forceinline__ unsigned long long nj_key(int32_t a, int32_t b) {      // node ids are below 2^31
  return a < b ? ((unsigned long long)(uint32_t)a << 32) | (uint32_t)b : ((unsigned long long)(uint32_t)b << 32) | (uint32_t)a;
}

__device__ __forceinline__ void nj_combine(NjBest& a, const NjBest& o) {
  const uint32_t cells = a.cells + o.cells;
  if (nj_less(o.q, o.key, a)) a = o;
  a.cells = cells;
}

__device__ __forceinline__ NjBest nj_wave_reduce(NjBest b) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    NjBest o;
    o.q = __shfl_xor(b.q, off, 64);
    o.key = __shfl_xor(b.key, off, 64);
    o.cells = __shfl_xor(b.cells, off, 64);
    o.pad = 0;
    nj_combine(b, o);
  }
  return b;
}

// every thread of the workgroup returns the workgroup's best; lds holds (waves + 1) entries and is free again on return
__device__ NjBest nj_block_reduce(NjBest b, NjBest* lds) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
  b = nj_wave_reduce(b);
  if (lane == 0) lds[wave] = b;
  __syncthreads();
  if (wave == 0) {
    NjBest c = lane < n_waves ? lds[lane] : nj_none();
    c = nj_wave_reduce(c);
    if (lane == 0) lds[n_waves] = c;
  }
  __syncthreads();
  b = lds[n_waves];
  __syncthreads();
  return b;
}

__global__ __launch_bounds__(NJ_THREADS) void nj_check_kernel(const double* __restrict__ w, uint32_t n, uint32_t n_tiles, int* __restrict__ flag) {
  __shared__ double mirror[NJ_TILE][NJ_TILE + 1];
  const uint32_t tid = threadIdx.x, x = tid & 63u, y0 = tid >> 6;
  uint32_t bi = 0, rest = blockIdx.x;      // tile (bi, bj), bi <= bj, from the linear index over the upper triangle
  while (rest >= n_tiles - bi) { rest -= n_tiles - bi; ++bi; }
  const uint32_t bj = bi + rest, i0 = bi * NJ_TILE, j0 = bj * NJ_TILE;
#pragma unroll 4
  for (uint32_t e = 0; e < 16; ++e) {      // tile (bj, bi) as it lies
    const uint32_t y = y0 + 4 * e, gi = j0 + y, gj = i0 + x;
    mirror[y][x] = (gi < n && gj < n) ? w[(size_t)gi * n + gj] : 0.0;
  }
  __syncthreads();
  int f = 0;
#pragma unroll 4
  for (uint32_t e = 0; e < 16; ++e) {
    const uint32_t y = y0 + 4 * e, i = i0 + y, j = j0 + x;
    if (i >= n || j >= n) continue;
    const double v = w[(size_t)i * n + j], t = mirror[x][y];      // d[i][j], d[j][i]
    if (!nj_finite(v) || !nj_finite(t)) f |= NJ_F_NONFINITE;
    if (__double_as_longlong(v) != __double_as_longlong(t)) f |= NJ_F_ASYM;
    if (i == j && !(v == 0.0)) f |= NJ_F_DIAG;
  }
  if (f) atomicOr(flag, f);
}

__global__ __launch_bounds__(64) void nj_rowsum_kernel(const double* __restrict__ w, uint32_t n, double* __restrict__ r, int32_t* __restrict__ ids,
                                                       int* __restrict__ flag) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
#pragma unroll 8
  for (uint32_t k = 0; k < n; ++k) s = s + w[(size_t)k * n + i];      // k ascending, one thread: the statement's order
  r[i] = s;
  ids[i] = (int32_t)i;
  if (!nj_finite(s)) atomicOr(flag, NJ_F_NONFINITE);
}

__global__ __launch_bounds__(NJ_THREADS) void nj_argmin_kernel(NjState s, uint32_t m, uint32_t n_tiles) {
  __shared__ NjBest lds[NJ_THREADS / 64 + 1];
  if (*s.flag) return;
  const uint32_t tid = threadIdx.x, x = tid & 63u, y0 = tid >> 6;
  uint32_t bi = 0, rest = blockIdx.x;
  while (rest >= n_tiles - bi) { rest -= n_tiles - bi; ++bi; }
  const uint32_t bj = bi + rest, i0 = bi * NJ_TILE, j0 = bj * NJ_TILE;
  const uint32_t j = j0 + x;
  const size_t ld = s.n;
  const double mm2 = (double)(m - 2);
  const double rj = j < m ? s.r[j] : 0.0;
  const int32_t idj = j < m ? s.ids[j] : 0;
  NjBest best = nj_none();
  bool bad = false;
#pragma unroll 4
  for (uint32_t e = 0; e < 16; ++e) {      // a wave reads 64 contiguous cells of one row
    const uint32_t i = i0 + y0 + 4 * e;
    if (!(i < j && j < m)) continue;
    const double d = s.w[(size_t)i * ld + j];
    const double q = mm2 * d - (s.r[i] + rj);
    const unsigned long long key = nj_key(s.ids[i], idj);
    bad |= !nj_finite(q);
    ++best.cells;
    if (nj_less(q, key, best)) { best.q = q; best.key = key; }
  }
  if (bad) atomicOr(s.flag, NJ_F_NONFINITE);
  best = nj_block_reduce(best, lds);
  if (tid == 0) s.partial[blockIdx.x] = best;
}

// One join by the whole workgroup: the pair of nodes in best.key, of m live ones, becomes node n + t; their slots are looked up in the
// id table (lds_int[1], lds_int[2]), so nothing but the criterion and the ids travels through the reductions.  Returns, to every thread,
// whether a row sum left the finite range (gathered in lds_int[0]).  Ends with a barrier.  Every barrier here is __syncthreads(): it
// orders the GLOBAL stores of one phase before the loads of the next (a workgroup reduction such as __syncthreads_or waits for LDS
// only, and the next step's scan then reads cells that are still on their way).
__device__ bool nj_join_step(const NjState& s, uint32_t m, uint32_t t, const NjBest& best, int* lds_int) {
  const uint32_t tid = threadIdx.x, step = blockDim.x;
  const size_t ld = s.n;
  const int32_t lo = (int32_t)(best.key >> 32), hi = (int32_t)(best.key & 0xffffffffu);
  if (tid == 0) lds_int[0] = 0;
  for (uint32_t k = tid; k < m; k += step) {
    const int32_t id = s.ids[k];
    if (id == lo) lds_int[1] = (int)k;
    if (id == hi) lds_int[2] = (int)k;
  }
  __syncthreads();
  const uint32_t sa = (uint32_t)lds_int[1], sb = (uint32_t)lds_int[2], last = m - 1;      // the slots of the lower and the higher id
  const uint32_t p = sa < sb ? sa : sb, q = sa < sb ? sb : sa;                              // p < q <= last
  const double d = s.w[(size_t)sa * ld + sb], ra = s.r[sa], rb = s.r[sb];
  __syncthreads();      // everything above is read before anything below is written
  bool bad = false;
  for (uint32_t k = tid; k < m; k += step) {
    if (k == p || k == q) continue;
    const double da = s.w[(size_t)sa * ld + k], db = s.w[(size_t)sb * ld + k];
    const double du = ((da + db) - d) / 2.0;
    const double rk = ((s.r[k] - da) - db) + du;
    bad |= !nj_finite(rk);
    s.r[k] = rk;
    s.w[(size_t)p * ld + k] = du;      // the cells of rows sa, sb that this thread has just read, and of row k, which nobody reads
    s.w[(size_t)k * ld + p] = du;
  }
  if (tid == 0) {
    const double mm2 = (double)(m - 2);
    const double len_a = d / 2.0 + (ra - rb) / (2.0 * mm2);
    const double ru = ((ra + rb) - (double)m * d) / 2.0;
    bad |= !nj_finite(ru);
    s.join[2 * t] = lo;
    s.join[2 * t + 1] = hi;
    s.len[2 * t] = len_a;
    s.len[2 * t + 1] = d - len_a;
    s.r[p] = ru;
    s.ids[p] = (int32_t)(s.n + t);
  }
  if (bad) atomicOr(&lds_int[0], 1);
  __syncthreads();
  if (q != last) {      // the last live slot moves into the freed one, row and column; p < q, so the new row stays where it is
    for (uint32_t k = tid; k < last; k += step) {
      if (k == q) continue;
      const double v = s.w[(size_t)last * ld + k];      // k == p: the new node's distance, written above
      s.w[(size_t)q * ld + k] = v;
      s.w[(size_t)k * ld + q] = v;
    }
    if (tid == 0) {
      s.r[q] = s.r[last];
      s.ids[q] = s.ids[last];
    }
  }
  __syncthreads();
  return lds_int[0] != 0;
}

__global__ __launch_bounds__(NJ_WG) void nj_join_kernel(NjState s, uint32_t m, uint32_t n_partials, uint32_t t) {
  __shared__ NjBest lds[NJ_WG / 64 + 1];
  __shared__ int lds_int[4];
  if (*s.flag) return;
  NjBest best = nj_none();
  for (uint32_t k = threadIdx.x; k < n_partials; k += blockDim.x) nj_combine(best, s.partial[k]);
  best = nj_block_reduce(best, lds);
  if (threadIdx.x == 0) *s.cells += best.cells;
  if (nj_join_step(s, m, t, best, lds_int) && threadIdx.x == 0) atomicOr(s.flag, NJ_F_NONFINITE);
}

__global__ __launch_bounds__(NJ_WG) void nj_tail_kernel(NjState s, uint32_t m0, uint32_t t0) {
  __shared__ NjBest lds[NJ_WG / 64 + 1];
  __shared__ int lds_int[4];
  if (*s.flag) return;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, n_waves = blockDim.x >> 6;
  const size_t ld = s.n;
  uint32_t t = t0;
  for (uint32_t m = m0; m > 3; --m, ++t) {
    const double mm2 = (double)(m - 2);
    NjBest best = nj_none();
    bool bad = false;
    if (tid == 0) lds_int[0] = 0;
    __syncthreads();
    for (uint32_t i = wave; i + 1 < m; i += n_waves) {      // a wave per row, its lanes along the row
      const double ri = s.r[i];
      const int32_t idi = s.ids[i];
      for (uint32_t j = i + 1 + lane; j < m; j += 64) {
        const double q = mm2 * s.w[(size_t)i * ld + j] - (ri + s.r[j]);
        const unsigned long long key = nj_key(idi, s.ids[j]);
        bad |= !nj_finite(q);
        if (nj_less(q, key, best)) { best.q = q; best.key = key; }
      }
    }
    if (bad) atomicOr(&lds_int[0], 1);
    __syncthreads();
    bad = lds_int[0] != 0;
    if (!bad) {
      best = nj_block_reduce(best, lds);
      bad = nj_join_step(s, m, t, best, lds_int);
    }
    if (bad) {      // the same answer in every thread
      if (tid == 0) atomicOr(s.flag, NJ_F_NONFINITE);
      return;
    }
  }
  if (tid == 0) {      // the three survivors, by id: x < y < z
    uint32_t a = 0, b = 1, c = 2, h;
    if (s.ids[a] > s.ids[b]) { h = a; a = b; b = h; }
    if (s.ids[b] > s.ids[c]) { h = b; b = c; c = h; }
    if (s.ids[a] > s.ids[b]) { h = a; a = b; b = h; }
    const double dxy = s.w[(size_t)a * ld + b], dxz = s.w[(size_t)a * ld + c], dyz = s.w[(size_t)b * ld + c];
    s.last[0] = s.ids[a];
    s.last[1] = s.ids[b];
    s.last[2] = s.ids[c];
    s.last_len[0] = ((dxy + dxz) - dyz) / 2.0;
    s.last_len[1] = ((dxy + dyz) - dxz) / 2.0;
    s.last_len[2] = ((dxz + dyz) - dxy) / 2.0;
  }
}

uint32_t nj_tiles(uint32_t m) {
  const uint32_t t = (m + NJ_TILE - 1) / NJ_TILE;
  return t * (t + 1) / 2;
}

struct NjEvents {      // validate (0 -> 1) | wide steps (2 -> 3) | tail (3 -> 4): marks on the context's stream while profiling is on
  hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  bool open = false;
  explicit NjEvents(pg_ctx* ctx) {
    if (!ctx->profiling) return;
    open = true;
    for (auto& x : e)
      if (hipEventCreate(&x) != hipSuccess) { (void)hipGetLastError(); x = nullptr; open = false; }
  }
  void mark(pg_ctx* ctx, int k) { if (open) open = hipEventRecord(e[k], ctx->stream) == hipSuccess; }
  void read(double* ms) {      // after hipStreamSynchronize
    const int from[3] = {0, 2, 3};
    for (int k = 0; k < 3; ++k) {
      float v = 0.f;
      if (open && hipEventElapsedTime(&v, e[from[k]], e[from[k] + 1]) == hipSuccess) ms[k] = v;
    }
  }
  ~NjEvents() {
    for (auto x : e)
      if (x) (void)hipEventDestroy(x);
  }
};

}  // namespace

extern "C" int pg_tree_nj(pg_ctx* ctx, const double* d, uint32_t n, int32_t* join_out, double* len_out, int32_t* last_out, double* last_len_out) {
  if (!ctx) return PG_E_ARG;
  if (!d) return pg_fail(ctx, PG_E_ARG, "tree: bad argument");
  if (n < 3) return pg_fail(ctx, PG_E_ARG, "tree: fewer than three nodes");
  if (n > NJ_MAX_N) return pg_fail(ctx, PG_E_ARG, "tree: more than 8192 nodes");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  int rc;
  PgDevBuf<double> d_w, d_r, d_len, d_last_len;
  PgDevBuf<int32_t> d_ids, d_join, d_last;
  PgDevBuf<NjBest> d_partial;
  PgDevBuf<unsigned long long> d_cells;
  PgDevBuf<int> d_flag;
  const size_t n_joins = n - 3;
  if ((rc = pg_dev_alloc(ctx, "tree", d_w, (size_t)n * n, "the working matrix (8 n^2 bytes)")) || (rc = pg_dev_alloc(ctx, "tree", d_r, n, "the row sums")) ||
      (rc = pg_dev_alloc(ctx, "tree", d_ids, n, "the id table")) || (rc = pg_dev_alloc(ctx, "tree", d_join, 2 * n_joins, "the joins")) ||
      (rc = pg_dev_alloc(ctx, "tree", d_len, 2 * n_joins, "the lengths")) || (rc = pg_dev_alloc(ctx, "tree", d_last, 3, "the last node")) ||
      (rc = pg_dev_alloc(ctx, "tree", d_last_len, 3, "the last lengths")) || (rc = pg_dev_alloc(ctx, "tree", d_partial, nj_tiles(n), "the partials")) ||
      (rc = pg_dev_alloc(ctx, "tree", d_cells, 1, "the counter")) || (rc = pg_dev_alloc(ctx, "tree", d_flag, 1, "the flag")))
    return rc;
  NjState s{};
  s.w = d_w; s.r = d_r; s.ids = d_ids; s.join = d_join; s.len = d_len; s.last = d_last; s.last_len = d_last_len;
  s.partial = d_partial; s.cells = d_cells; s.flag = d_flag; s.n = n;
  for (auto& c : ctx->tree_counts) c = 0;
  for (auto& v : ctx->tree_ms) v = 0.0;
  NjEvents ev(ctx);
  uint64_t launches = 0;
  int h_flag = 0;
  hipError_t e = hipMemcpyAsync(d_w, d, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_flag, 0, sizeof(int), ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_cells, 0, sizeof(unsigned long long), ctx->stream);
  if (e == hipSuccess) {
    ev.mark(ctx, 0);
    const uint32_t t = (n + NJ_TILE - 1) / NJ_TILE;
    hipLaunchKernelGGL(nj_check_kernel, dim3(nj_tiles(n)), dim3(NJ_THREADS), 0, ctx->stream, (const double*)d_w, n, t, (int*)d_flag);
    hipLaunchKernelGGL(nj_rowsum_kernel, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, (const double*)d_w, n, (double*)d_r, (int32_t*)d_ids, (int*)d_flag);
    launches += 2;
    ev.mark(ctx, 1);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&h_flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);      // the one read-back before the loop: the refusals
  if (e != hipSuccess) return pg_fail(ctx, PG_E_HIP, std::string("tree: ") + hipGetErrorString(e));
  if (h_flag & NJ_F_NONFINITE) return pg_fail(ctx, PG_E_NONFINITE, "tree: a distance or a row sum is not finite (NaN or infinite cell, or overflow)");
  if (h_flag & NJ_F_ASYM) return pg_fail(ctx, PG_E_ARG, "tree: the matrix is not symmetric bit for bit");
  if (h_flag & NJ_F_DIAG) return pg_fail(ctx, PG_E_ARG, "tree: the diagonal is not zero");

  const uint32_t tail = std::max<uint32_t>(3, std::min<uint32_t>(ctx->tree_tail_limit, NJ_TAIL_MAX));
  uint32_t wg = NJ_WG;      // development: PYANI_TREE_WG = the threads of the join and tail workgroup, so that small problems reach its loops' later rounds
  if (const char* v = pg_dev_env("PYANI_TREE_WG")) {
    const int k = atoi(v);
    if (k >= 64 && k <= (int)NJ_WG && k % 64 == 0) wg = (uint32_t)k;
  }
  uint32_t m = n, t = 0;
  uint64_t wide = 0;
  ev.mark(ctx, 2);
  for (; m > tail; --m, ++t, ++wide) {
    const uint32_t tiles_1d = (m + NJ_TILE - 1) / NJ_TILE, tiles = nj_tiles(m);
    hipLaunchKernelGGL(nj_argmin_kernel, dim3(tiles), dim3(NJ_THREADS), 0, ctx->stream, s, m, tiles_1d);
    hipLaunchKernelGGL(nj_join_kernel, dim3(1), dim3(wg), 0, ctx->stream, s, m, tiles, t);
    launches += 2;
  }
  ev.mark(ctx, 3);
  hipLaunchKernelGGL(nj_tail_kernel, dim3(1), dim3(wg), 0, ctx->stream, s, m, t);
  ++launches;
  ev.mark(ctx, 4);
  e = hipGetLastError();
  unsigned long long h_cells = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&h_flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(&h_cells, d_cells, sizeof(h_cells), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);      // the flag decides whether anything is fetched
  if (e != hipSuccess) return pg_fail(ctx, PG_E_HIP, std::string("tree: ") + hipGetErrorString(e));
  if (h_flag) return pg_fail(ctx, PG_E_NONFINITE, "tree: a criterion or a row sum is not finite (overflow)");
  if (e == hipSuccess && join_out && n_joins) e = hipMemcpyAsync(join_out, d_join, 2 * n_joins * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && len_out && n_joins) e = hipMemcpyAsync(len_out, d_len, 2 * n_joins * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && last_out) e = hipMemcpyAsync(last_out, d_last, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && last_len_out) e = hipMemcpyAsync(last_len_out, d_last_len, 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return pg_fail(ctx, PG_E_HIP, std::string("tree: ") + hipGetErrorString(e));
  ctx->tree_counts[0] = n;
  ctx->tree_counts[1] = wide;
  ctx->tree_counts[2] = n_joins - wide;
  ctx->tree_counts[3] = launches;
  ctx->tree_counts[4] = h_cells;
  ev.read(ctx->tree_ms);
  return PG_OK;
}

extern "C" int pg_tree_nj_set(pg_ctx* ctx, uint32_t tail_limit) {
  if (!ctx) return PG_E_ARG;
  if (tail_limit < 3 || tail_limit > NJ_TAIL_MAX) return pg_fail(ctx, PG_E_ARG, "tree: tail_limit outside 3 ... 1024");
  ctx->tree_tail_limit = tail_limit;
  return PG_OK;
}

extern "C" int pg_tree_nj_last(pg_ctx* ctx, uint64_t* counts_out, double* ms_out) {
  if (!ctx) return PG_E_ARG;
  if (counts_out)
    for (int k = 0; k < 5; ++k) counts_out[k] = ctx->tree_counts[k];
  if (ms_out)
    for (int k = 0; k < 3; ++k) ms_out[k] = ctx->profiling ? ctx->tree_ms[k] : 0.0;
  return PG_OK;
}
