// pg_cluster.hip — the ordering arithmetic of `pyani plot` on the GPU: the two hierarchical clusterings that order every heatmap
// (reference interface it stands in for: pyani/pyani_graphics/mpl/__init__.py:84-136, add_dendrogram: pdist(dfr) / pdist(dfr.T),
// linkage(method="complete"); pyani/pyani_graphics/sns/__init__.py:130, clustermap: the same with method="average";
// pyani/scripts/subcommands/subcmd_plot.py:130-139: five matrices per run).  fp64 VALU work; no MFMA (it fuses and re-associates).
//
// Contract: results are EQUAL to scipy's, bit for bit, so every operation below is rounded on its own
// (-ffp-contract=off in the build line; the golden tests are what keeps it true) and every sum runs in the reference's order.
//
//   K1 cluster_pdist_kernel    Euclidean distances between the n observations of an fp64 matrix, rows (observation i, element k at
//                              x[i * ld + k]) or columns (x[k * ld + i]: the same matrix, no transposed copy).  One workgroup of 256
//                              threads per 64 x 64 tile of the UPPER triangle of the pair grid, a 4 x 4 register tile of pairs per
//                              thread.  The k-panels (16 deep) of both observation blocks go through LDS k-major, double-buffered:
//                              the next panel is loaded into registers before the current one is consumed and stored after it, one
//                              barrier per panel.  Global reads are contiguous in both orientations (rows: 4 threads x 32 B along k
//                              per observation; columns: 16 threads x 32 B along the observations per k); the LDS image is the same.
//                              One thread carries a pair's sum through all of k in ascending order: s = s + d * d, so the result does
//                              not depend on the tiling.  Panel cells past the end of k hold 0 for both observations: s + 0 * 0 = s.
//                              Writes the condensed vector (scipy's order) and / or the symmetric square working matrix of K2, and
//                              raises a flag for any non-finite distance.
//   K2 cluster_linkage_kernel  (pg_cluster_linkage.h: the screen's linkage of the kept pairs runs it too)
//                              scipy's nearest-neighbour chain for "complete" and "average".  One workgroup per problem.  The chain
//                              is serial; a chain step is a row argmin over the live clusters: per-thread scan in ascending index
//                              order, wave64 reduction on (value, index) with "lowest index wins", cross-wave reduction through LDS,
//                              then the strict comparison with the incumbent.  The Lance-Williams update of a merge goes across the
//                              workgroup.  Working matrix: symmetric n x n square (every row read is contiguous; the update writes a
//                              row and its mirror column).  Cluster sizes and the chain sit in LDS.  Output: the n - 1 merge
//                              records (x, y, height, size) in merge order; the stable sort and the relabelling are the host's.
#include <algorithm>
#include <vector>

#include "pg_internal.h"
#include "pg_devbuf.h"

namespace {

#include "pg_cluster_linkage.h"      // CLU_MAX_N, ClusterProblem, K2

constexpr int CLU_TILE = 64, CLU_KP = 16, CLU_LDS_ROW = CLU_TILE + 4;      // rows padded: the transposing store of the row orientation spreads over banks

template <bool COLS>
__device__ __forceinline__ void pdist_fetch(const double* __restrict__ x, uint32_t n, uint32_t m, size_t ld, uint32_t obs0, uint32_t k0,
                                            uint32_t tid, double (&r)[4]) {
  // ROWS: thread -> observation tid / 4, k = 4 (tid % 4) .. + 3.   COLS: thread -> k = tid / 16, observations 4 (tid % 16) .. + 3.
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint32_t o = COLS ? obs0 + 4u * (tid & 15u) + e : obs0 + (tid >> 2);
    const uint32_t k = COLS ? k0 + (tid >> 4) : k0 + 4u * (tid & 3u) + e;
    r[e] = (o < n && k < m) ? (COLS ? x[(size_t)k * ld + o] : x[(size_t)o * ld + k]) : 0.0;
  }
}

template <bool COLS>
__device__ __forceinline__ void pdist_stage(double (*panel)[CLU_LDS_ROW], uint32_t tid, const double (&r)[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (COLS) panel[tid >> 4][4u * (tid & 15u) + e] = r[e];
    else panel[4u * (tid & 3u) + e][tid >> 2] = r[e];
  }
}

template <bool COLS>
__global__ __launch_bounds__(256, 2) void cluster_pdist_kernel(const double* __restrict__ x, uint32_t n, uint32_t m, size_t ld, uint32_t n_tiles,
                                                             double* __restrict__ condensed, double* __restrict__ square, int* __restrict__ flag) {
  __shared__ double lds[2][2][CLU_KP][CLU_LDS_ROW];      // [buffer][block i / block j][k][observation]
  const uint32_t tid = threadIdx.x, tx = tid & 15u, ty = tid >> 4;
  // tile (bi, bj), bi <= bj, from the linear index over the upper triangle
  uint32_t bi = 0, rest = blockIdx.x;
  while (rest >= n_tiles - bi) { rest -= n_tiles - bi; ++bi; }
  const uint32_t bj = bi + rest;
  const uint32_t i0 = bi * CLU_TILE, j0 = bj * CLU_TILE;

  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;

  double ra[4], rb[4];
  pdist_fetch<COLS>(x, n, m, ld, i0, 0, tid, ra);
  pdist_fetch<COLS>(x, n, m, ld, j0, 0, tid, rb);
  pdist_stage<COLS>(lds[0][0], tid, ra);
  pdist_stage<COLS>(lds[0][1], tid, rb);
  __syncthreads();
  int buf = 0;
  for (uint32_t k0 = 0; k0 < m; k0 += CLU_KP) {
    const bool more = k0 + CLU_KP < m;
    if (more) {
      pdist_fetch<COLS>(x, n, m, ld, i0, k0 + CLU_KP, tid, ra);
      pdist_fetch<COLS>(x, n, m, ld, j0, k0 + CLU_KP, tid, rb);
    }
#pragma unroll 4
    for (int k = 0; k < CLU_KP; ++k) {
      double u[4], v[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) u[a] = lds[buf][0][k][4 * ty + a];
#pragma unroll
      for (int b = 0; b < 4; ++b) v[b] = lds[buf][1][k][4 * tx + b];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const double d = u[a] - v[b];
          acc[a][b] = acc[a][b] + d * d;      // two roundings: the build line forbids contraction
        }
    }
    if (more) {      // the other buffer was last read before the previous barrier
      pdist_stage<COLS>(lds[buf ^ 1][0], tid, ra);
      pdist_stage<COLS>(lds[buf ^ 1][1], tid, rb);
    }
    __syncthreads();
    buf ^= 1;
  }

  bool bad = false;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const uint32_t i = i0 + 4 * ty + a;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t j = j0 + 4 * tx + b;
      if (i >= n || j >= n) continue;
      if (i == j) {
        if (square) square[(size_t)i * n + i] = 0.0;
        continue;
      }
      if (i > j) continue;      // lower half of a diagonal tile
      const double d = sqrt(acc[a][b]);
      bad |= !(fabs(d) <= 1.79769313486231570815e308);
      if (condensed) condensed[(size_t)i * n - ((size_t)i * (i + 1)) / 2 + (j - i - 1)] = d;
      if (square) {
        square[(size_t)i * n + j] = d;
        square[(size_t)j * n + i] = d;
      }
    }
  }
  if (bad) atomicOr(flag, 1);
}

int clu_check_shape(pg_ctx* ctx, const double* x, uint32_t rows, uint32_t cols, uint32_t min_obs, int columns, uint32_t* n, uint32_t* m) {
  if (!x || rows == 0 || cols == 0) return pg_fail(ctx, PG_E_ARG, "cluster: bad argument");
  *n = columns ? cols : rows;
  *m = columns ? rows : cols;
  if (*n > CLU_MAX_N) return pg_fail(ctx, PG_E_ARG, "cluster: more than 8192 observations (cluster sizes and the chain live in LDS)");
  if (*n < min_obs) return pg_fail(ctx, PG_E_ARG, "cluster: fewer than two observations");
  return PG_OK;
}

void clu_launch_pdist(pg_ctx* ctx, const double* d_x, uint32_t rows, uint32_t cols, int columns, double* d_cond, double* d_square, int* d_flag) {
  const uint32_t n = columns ? cols : rows, m = columns ? rows : cols;
  const uint32_t t = (n + CLU_TILE - 1) / CLU_TILE, blocks = t * (t + 1) / 2;
  pg_prof_begin(ctx, PG_K_CLUSTER_PDIST);
  if (columns)
    hipLaunchKernelGGL(cluster_pdist_kernel<true>, dim3(blocks), dim3(256), 0, ctx->stream, d_x, n, m, (size_t)cols, t, d_cond, d_square, d_flag);
  else
    hipLaunchKernelGGL(cluster_pdist_kernel<false>, dim3(blocks), dim3(256), 0, ctx->stream, d_x, n, m, (size_t)cols, t, d_cond, d_square, d_flag);
  pg_prof_end(ctx);
}

}  // namespace

extern "C" int pg_cluster_pdist(pg_ctx* ctx, const double* x, uint32_t rows, uint32_t cols, int columns, double* out) {
  if (!ctx) return PG_E_ARG;
  uint32_t n, m;
  int rc;
  if ((rc = clu_check_shape(ctx, x, rows, cols, 1, columns, &n, &m))) return rc;
  const size_t n_pairs = (size_t)n * (n - 1) / 2;
  if (n_pairs == 0) return PG_OK;
  if (!out) return pg_fail(ctx, PG_E_ARG, "cluster: bad argument");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PgDevBuf<double> d_x, d_c;
  PgDevBuf<int> d_f;
  if ((rc = pg_dev_alloc(ctx, "cluster", d_x, (size_t)rows * cols, "the matrix")) || (rc = pg_dev_alloc(ctx, "cluster", d_c, n_pairs, "the distances")) ||
      (rc = pg_dev_alloc(ctx, "cluster", d_f, 1, "the flag")))
    return rc;
  int h_flag = 0;
  hipError_t e = hipMemcpyAsync(d_x, x, (size_t)rows * cols * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_f, 0, sizeof(int), ctx->stream);
  if (e == hipSuccess) {
    clu_launch_pdist(ctx, d_x, rows, cols, columns, d_c, nullptr, d_f);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_c, n_pairs * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(&h_flag, d_f, sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return pg_fail(ctx, PG_E_HIP, std::string("cluster: ") + hipGetErrorString(e));
  if (h_flag) return pg_fail(ctx, PG_E_NONFINITE, "cluster: a distance is not finite (NaN or infinite cell, or overflow)");
  return PG_OK;
}

extern "C" int pg_cluster_linkage_batch(pg_ctx* ctx, pg_cluster_problem* problems, uint32_t n_problems) {
  if (!ctx) return PG_E_ARG;
  if (!problems || n_problems == 0) return pg_fail(ctx, PG_E_ARG, "cluster: bad argument");
  int rc;
  uint32_t n_max = 0;
  std::vector<uint32_t> ns(n_problems);
  for (uint32_t p = 0; p < n_problems; ++p) {
    pg_cluster_problem& q = problems[p];
    uint32_t m;
    if ((rc = clu_check_shape(ctx, q.x, q.rows, q.cols, 2, q.columns, &ns[p], &m))) return rc;
    if (!q.merges || (q.method != PG_CLUSTER_COMPLETE && q.method != PG_CLUSTER_AVERAGE)) return pg_fail(ctx, PG_E_ARG, "cluster: bad argument");
    q.status = PG_OK;
    n_max = std::max(n_max, ns[p]);
  }
  PG_HIP(ctx, hipSetDevice(ctx->device));
  // device buffers: one copy of every distinct caller matrix, a working matrix and the records per problem, the flags, the descriptors
  std::vector<PgDevBuf<double>> bufs(3 * (size_t)n_problems);
  size_t nb = 0;
  std::vector<double*> d_x(n_problems, nullptr);
  std::vector<ClusterProblem> h_prob(n_problems);
  PgDevBuf<int> d_flags;
  PgDevBuf<ClusterProblem> d_prob;
  if ((rc = pg_dev_alloc(ctx, "cluster", d_flags, n_problems, "the flags")) || (rc = pg_dev_alloc(ctx, "cluster", d_prob, n_problems, "the problem table")))
    return rc;
  hipError_t e = hipMemsetAsync(d_flags, 0, n_problems * sizeof(int), ctx->stream);
  for (uint32_t p = 0; p < n_problems && e == hipSuccess; ++p) {
    const pg_cluster_problem& q = problems[p];
    for (uint32_t o = 0; o < p; ++o)      // both orientations of one matrix share its upload
      if (problems[o].x == q.x && problems[o].rows == q.rows && problems[o].cols == q.cols) { d_x[p] = d_x[o]; break; }
    if (!d_x[p]) {
      if ((rc = pg_dev_alloc(ctx, "cluster", bufs[nb], (size_t)q.rows * q.cols, "a matrix"))) return rc;
      d_x[p] = bufs[nb++];
      e = hipMemcpyAsync(d_x[p], q.x, (size_t)q.rows * q.cols * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    }
    const uint32_t n = ns[p];
    if ((rc = pg_dev_alloc(ctx, "cluster", bufs[nb], (size_t)n * n, "a working matrix")) || (rc = pg_dev_alloc(ctx, "cluster", bufs[nb + 1], (size_t)(n - 1) * 4, "the merge records")))
      return rc;
    h_prob[p].work = bufs[nb++];
    h_prob[p].merges = bufs[nb++];
    h_prob[p].flag = d_flags + p;
    h_prob[p].n = n;
    h_prob[p].method = q.method;
  }
  const uint32_t threads = clu_linkage_threads(n_max);
  const size_t lds_bytes = clu_linkage_lds(n_max);
  if (e == hipSuccess && lds_bytes > 48 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(cluster_linkage_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess) {
    (void)hipGetLastError();
    return pg_fail(ctx, PG_E_CAPACITY, "cluster: the linkage needs " + std::to_string(lds_bytes) + " bytes of LDS per workgroup, which this device does not grant");
  }
  if (e == hipSuccess) e = hipMemcpyAsync(d_prob, h_prob.data(), n_problems * sizeof(ClusterProblem), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    for (uint32_t p = 0; p < n_problems; ++p)
      clu_launch_pdist(ctx, d_x[p], problems[p].rows, problems[p].cols, problems[p].columns, nullptr, h_prob[p].work, d_flags + p);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    pg_prof_begin(ctx, PG_K_CLUSTER_LINKAGE);
    hipLaunchKernelGGL(cluster_linkage_kernel, dim3(n_problems), dim3(threads), lds_bytes, ctx->stream, d_prob);
    pg_prof_end(ctx);
    e = hipGetLastError();
  }
  std::vector<int> h_flags(n_problems, 0);
  if (e == hipSuccess) e = hipMemcpyAsync(h_flags.data(), d_flags, n_problems * sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);      // h_prob must outlive its copy; the flags decide what is fetched
  for (uint32_t p = 0; p < n_problems && e == hipSuccess; ++p) {
    if (h_flags[p]) { problems[p].status = PG_E_NONFINITE; continue; }
    e = hipMemcpyAsync(problems[p].merges, h_prob[p].merges, (size_t)(ns[p] - 1) * 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return pg_fail(ctx, PG_E_HIP, std::string("cluster: ") + hipGetErrorString(e));
  return PG_OK;
}

extern "C" int pg_cluster_linkage(pg_ctx* ctx, const double* x, uint32_t rows, uint32_t cols, int columns, int method, double* merges_out) {
  if (!ctx) return PG_E_ARG;
  pg_cluster_problem q{};
  q.x = x;
  q.rows = rows;
  q.cols = cols;
  q.columns = columns;
  q.method = method;
  q.merges = merges_out;
  const int rc = pg_cluster_linkage_batch(ctx, &q, 1);
  if (rc != PG_OK) return rc;
  if (q.status == PG_E_NONFINITE) return pg_fail(ctx, PG_E_NONFINITE, "cluster: a distance is not finite (NaN or infinite cell, or overflow)");
  return q.status;
}
