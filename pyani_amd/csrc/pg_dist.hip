// pg_dist.hip — the arithmetic of `pyani plot`'s distribution plots on the GPU: histogram and Gaussian kernel density estimate over
// all cells of a result matrix (reference interface it stands in for: pyani/pyani_graphics/mpl/__init__.py:139-175, distribution:
// hist(data, bins=50) and scipy.stats.gaussian_kde(data) on a 200-point grid; pyani/pyani_graphics/sns/__init__.py:192-233: histplot
// and kdeplot of the same values; pyani/scripts/subcommands/subcmd_plot.py:141-153: five matrices per run).  fp64 VALU and integer
// work; no MFMA.
//
// Contract: minimum, maximum and every count are exact (they do not depend on order).  The density sums are
// deterministic: their order is fixed by compile-time constants alone, never by the device or the launch.  The host owns everything
// that fixes floats (bin edges, grid, bandwidth, normalisation).
//
//   D1 dist_stats_kernel   one pass over the values: minimum and maximum over the non-NaN ones, the number of NaN and of +-inf cells.
//                          Grid-stride scan, wave64 butterfly, one partial record per workgroup through LDS; dist_stats_final_kernel
//                          (one workgroup) folds the records.  No float atomics.
//   D2 dist_hist_kernel    counts for B <= 4096 bins from B + 1 ascending edges, numpy's rule: value x -> the largest i with
//                          edges[i] <= x, x == edges[B] -> bin B - 1, NaN and values outside [edges[0], edges[B]] not counted.  Edges
//                          and private uint32 bins per workgroup in LDS.  UNIFORM: the bin is guessed arithmetically and corrected
//                          against the edges (exact for any ascending edges, fast when they are evenly spaced); else binary search.
//                          LDS bins are flushed to the 64-bit global counts with one vector atomic per non-empty bin.
//   D3 dist_kde_kernel     sums[j] = sum_i exp(-((p_j - x_i) / h)^2 / 2) over the non-NaN values, m <= 1024 grid points.  The values are
//                          cut into slices of DIST_SLICE; one workgroup per slice stages it in LDS; thread j owns point j and walks the
//                          slice in ascending order (every LDS read is a broadcast; no reduction inside the workgroup) and writes
//                          partial[slice][j].  dist_kde_sum_kernel adds a point's partials in slice order.  fp64 throughout, the device
//                          library's exp, no fast-math.
#include <algorithm>
#include <cmath>

#include "pg_internal.h"
#include "pg_devbuf.h"

namespace {

constexpr uint64_t DIST_MAX_N = 8192ull * 8192ull;      // values: every cell of the largest matrix the cluster calls accept
constexpr uint32_t DIST_MAX_BINS = 4096;                // (B + 1) edges + B bins in LDS: 49 160 B at the limit
constexpr uint32_t DIST_MAX_POINTS = 1024;              // one thread per grid point, one workgroup per slice
constexpr uint32_t DIST_SLICE = 2048;                   // values per slice: 489 workgroups for a 1000 x 1000 matrix (256 CUs), 16 KiB of LDS
constexpr uint32_t DIST_STATS_BLOCKS = 1024, DIST_THREADS = 256;

struct DistPartial {      // one per workgroup of D1
  double mn, mx;
  unsigned long long n_nan, n_inf;
};

struct DistState {
  uint64_t n = 0;
  PgDevBuf<double> d_x;
};

__device__ __forceinline__ void dist_fold(DistPartial& a, double mn, double mx, unsigned long long n_nan, unsigned long long n_inf) {
  a.mn = mn < a.mn ? mn : a.mn;
  a.mx = mx > a.mx ? mx : a.mx;
  a.n_nan += n_nan;
  a.n_inf += n_inf;
}

// folds the workgroup's records into thread 0's; blockDim = DIST_THREADS
__device__ __forceinline__ void dist_block_fold(DistPartial& a, DistPartial* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    dist_fold(a, __shfl_xor(a.mn, off, 64), __shfl_xor(a.mx, off, 64), __shfl_xor(a.n_nan, off, 64), __shfl_xor(a.n_inf, off, 64));
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0) lds[wave] = a;
  __syncthreads();
  if (threadIdx.x == 0)
    for (uint32_t w = 1; w < DIST_THREADS / 64; ++w) dist_fold(a, lds[w].mn, lds[w].mx, lds[w].n_nan, lds[w].n_inf);
}

__global__ __launch_bounds__(DIST_THREADS) void dist_stats_kernel(const double* __restrict__ x, uint64_t n, DistPartial* __restrict__ partials) {
  __shared__ DistPartial lds[DIST_THREADS / 64];
  const double INF = __builtin_huge_val();
  DistPartial a{INF, -INF, 0ull, 0ull};
  for (uint64_t i = (uint64_t)blockIdx.x * DIST_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * DIST_THREADS) {
    const double v = x[i];
    if (v != v) { ++a.n_nan; continue; }
    a.n_inf += (v == INF || v == -INF);
    a.mn = v < a.mn ? v : a.mn;
    a.mx = v > a.mx ? v : a.mx;
  }
  dist_block_fold(a, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = a;
}

__global__ __launch_bounds__(DIST_THREADS) void dist_stats_final_kernel(const DistPartial* __restrict__ partials, uint32_t n_partials,
                                                                        DistPartial* __restrict__ out) {
  __shared__ DistPartial lds[DIST_THREADS / 64];
  const double INF = __builtin_huge_val();
  DistPartial a{INF, -INF, 0ull, 0ull};
  for (uint32_t i = threadIdx.x; i < n_partials; i += DIST_THREADS) dist_fold(a, partials[i].mn, partials[i].mx, partials[i].n_nan, partials[i].n_inf);
  dist_block_fold(a, lds);
  if (threadIdx.x == 0) *out = a;
}

// scale = B / (edges[B] - edges[0]) (UNIFORM only)
template <bool UNIFORM>
__global__ __launch_bounds__(DIST_THREADS) void dist_hist_kernel(const double* __restrict__ x, uint64_t n, const double* __restrict__ edges, uint32_t B,
                                                                 double scale, unsigned long long* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* e = reinterpret_cast<double*>(smem);                    // [B + 1]
  uint32_t* bins = reinterpret_cast<uint32_t*>(e + (B + 1));      // [B]
  for (uint32_t i = threadIdx.x; i <= B; i += DIST_THREADS) e[i] = edges[i];
  for (uint32_t i = threadIdx.x; i < B; i += DIST_THREADS) bins[i] = 0u;
  __syncthreads();
  const double lo = e[0], hi = e[B];
  for (uint64_t i = (uint64_t)blockIdx.x * DIST_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * DIST_THREADS) {
    const double v = x[i];
    if (!(v >= lo && v <= hi)) continue;      // NaN fails both
    uint32_t b;
    if (UNIFORM) {
      const double g = (v - lo) * scale;      // 0 <= g, about <= B
      b = g < (double)(B - 1) ? (uint32_t)g : B - 1;
      while (b > 0 && v < e[b]) --b;
      while (b + 1 < B && v >= e[b + 1]) ++b;
    } else {
      uint32_t l = 0, h = B;      // invariant: e[l] <= v; everything above h is > v
      while (l < h) { const uint32_t mid = (l + h + 1) >> 1; if (e[mid] <= v) l = mid; else h = mid - 1; }
      b = l < B ? l : B - 1;
    }
    atomicAdd(&bins[b], 1u);
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < B; i += DIST_THREADS)
    if (bins[i]) atomicAdd(&counts[i], (unsigned long long)bins[i]);
}

__global__ __launch_bounds__(1024) void dist_kde_kernel(const double* __restrict__ x, uint64_t n, const double* __restrict__ points, uint32_t m, double h,
                                                        double* __restrict__ partial) {
  __shared__ double slice[DIST_SLICE];
  const uint64_t i0 = (uint64_t)blockIdx.x * DIST_SLICE;
  const uint32_t len = (uint32_t)(n - i0 < DIST_SLICE ? n - i0 : DIST_SLICE);
  for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) slice[i] = x[i0 + i];
  __syncthreads();
  const uint32_t j = threadIdx.x;
  if (j >= m) return;
  const double p = points[j];
  double s = 0.0;
#pragma unroll 4
  for (uint32_t i = 0; i < len; ++i) {
    const double v = slice[i];      // the same address in every lane: a broadcast
    if (v != v) continue;           // uniform over the workgroup
    const double t = (p - v) / h;
    s = s + exp(-(t * t) / 2.0);
  }
  partial[(size_t)blockIdx.x * m + j] = s;
}

__global__ __launch_bounds__(64) void dist_kde_sum_kernel(const double* __restrict__ partial, uint32_t n_slices, uint32_t m, double* __restrict__ sums) {
  const uint32_t j = blockIdx.x * 64u + threadIdx.x;
  if (j >= m) return;
  double s = 0.0;
#pragma unroll 8
  for (uint32_t k = 0; k < n_slices; ++k) s = s + partial[(size_t)k * m + j];
  sums[j] = s;
}

DistState* state_of(pg_ctx* ctx) { return static_cast<DistState*>(ctx->dist_state); }

// Kernel time of one call, outside the profile slots (their count is published): with pg_profile_enable on, a pair of events round the
// call's kernels on the engine's stream; read after the call's own synchronisation.
struct DistTimer {
  pg_ctx* ctx;
  int which;
  hipEvent_t a = nullptr, b = nullptr;
  bool open = false;
  DistTimer(pg_ctx* c, int w) : ctx(c), which(w) {
    ctx->dist_ms[which] = 0.0;
    if (!ctx->profiling) return;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { (void)hipGetLastError(); return; }
    open = true;
  }
  void start() { if (open) open = hipEventRecord(a, ctx->stream) == hipSuccess; }      // after the call's uploads: kernels only
  void stop() { if (open) open = hipEventRecord(b, ctx->stream) == hipSuccess; }
  void read() {      // after hipStreamSynchronize
    float ms = 0.f;
    if (open && hipEventElapsedTime(&ms, a, b) == hipSuccess) ctx->dist_ms[which] = ms;
  }
  ~DistTimer() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

}  // namespace

void pg_dist_drop(pg_ctx* ctx) {
  if (!ctx->dist_state) return;
  delete state_of(ctx);
  ctx->dist_state = nullptr;
}

extern "C" int pg_dist_release(pg_ctx* ctx) {
  if (!ctx) return PG_E_ARG;
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  pg_dist_drop(ctx);
  return PG_OK;
}

extern "C" int pg_dist_load(pg_ctx* ctx, const double* x, uint64_t n, pg_dist_stats* stats_out) {
  if (!ctx) return PG_E_ARG;
  if (!x || n == 0 || !stats_out) return pg_fail(ctx, PG_E_ARG, "dist: bad argument");
  if (n > DIST_MAX_N) return pg_fail(ctx, PG_E_ARG, "dist: more than 8192 x 8192 values");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  pg_dist_drop(ctx);
  DistState* S = new DistState();
  ctx->dist_state = S;
  PgDevBuf<DistPartial> d_part;
  const uint32_t blocks = (uint32_t)std::min<uint64_t>(DIST_STATS_BLOCKS, (n + DIST_THREADS - 1) / DIST_THREADS);
  int rc;
  if ((rc = pg_dev_alloc(ctx, "dist", S->d_x, n, "the values")) || (rc = pg_dev_alloc(ctx, "dist", d_part, blocks + 1, "the partial records"))) {
    pg_dist_drop(ctx);
    return rc;
  }
  DistPartial h{};
  DistTimer timer(ctx, 0);
  hipError_t e = hipMemcpyAsync(S->d_x, x, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    timer.start();
    hipLaunchKernelGGL(dist_stats_kernel, dim3(blocks), dim3(DIST_THREADS), 0, ctx->stream, S->d_x, n, d_part);
    hipLaunchKernelGGL(dist_stats_final_kernel, dim3(1), dim3(DIST_THREADS), 0, ctx->stream, d_part, blocks, d_part + blocks);
    timer.stop();
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&h, d_part + blocks, sizeof(h), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    pg_dist_drop(ctx);
    return pg_fail(ctx, PG_E_HIP, std::string("dist: ") + hipGetErrorString(e));
  }
  timer.read();
  S->n = n;
  stats_out->min = h.mn;
  stats_out->max = h.mx;
  stats_out->n_nan = h.n_nan;
  stats_out->n_inf = h.n_inf;
  return PG_OK;
}

extern "C" int pg_dist_hist(pg_ctx* ctx, const double* edges, uint32_t n_bins, uint64_t* counts_out) {
  if (!ctx) return PG_E_ARG;
  if (!edges || !counts_out || n_bins == 0) return pg_fail(ctx, PG_E_ARG, "dist: bad argument");
  DistState* S = state_of(ctx);
  if (!S || S->n == 0) return pg_fail(ctx, PG_E_ARG, "dist: no values loaded (call pg_dist_load first)");
  if (n_bins > DIST_MAX_BINS) return pg_fail(ctx, PG_E_ARG, "dist: more than 4096 bins (edges and private bins live in LDS)");
  for (uint32_t i = 0; i <= n_bins; ++i)
    if (!(edges[i] == edges[i]) || (i && edges[i] < edges[i - 1])) return pg_fail(ctx, PG_E_ARG, "dist: the bin edges must be ascending numbers");
  // evenly spaced (every edge within one bin width of its place on the line): the arithmetic guess needs few corrections
  const double span = edges[n_bins] - edges[0], width = span / n_bins;
  bool uniform = span > 0.0 && std::isfinite(span) && width > 0.0 && std::isfinite((double)n_bins / span);
  for (uint32_t i = 0; uniform && i <= n_bins; ++i) uniform = std::fabs(edges[i] - (edges[0] + i * width)) <= width;
  PG_HIP(ctx, hipSetDevice(ctx->device));
  const size_t lds_bytes = (size_t)(n_bins + 1) * sizeof(double) + (size_t)n_bins * sizeof(uint32_t);
  const void* fn = uniform ? reinterpret_cast<const void*>(dist_hist_kernel<true>) : reinterpret_cast<const void*>(dist_hist_kernel<false>);
  if (lds_bytes > 48 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess) {
    (void)hipGetLastError();
    return pg_fail(ctx, PG_E_CAPACITY, "dist: the histogram needs " + std::to_string(lds_bytes) + " bytes of LDS per workgroup, which this device does not grant");
  }
  PgDevBuf<double> d_edges;
  PgDevBuf<unsigned long long> d_counts;
  int rc;
  if ((rc = pg_dev_alloc(ctx, "dist", d_edges, n_bins + 1, "the bin edges")) || (rc = pg_dev_alloc(ctx, "dist", d_counts, n_bins, "the counts"))) return rc;
  // every value is counted once whatever the grid; enough workgroups to fill the device, few enough to keep the flushes small
  const uint32_t blocks = (uint32_t)std::min<uint64_t>((uint64_t)ctx->num_cu * 8, (S->n + 4 * DIST_THREADS - 1) / (4 * DIST_THREADS));
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "counts are copied out as they lie");
  DistTimer timer(ctx, 1);
  hipError_t e = hipMemcpyAsync(d_edges, edges, (size_t)(n_bins + 1) * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_counts, 0, (size_t)n_bins * sizeof(unsigned long long), ctx->stream);
  if (e == hipSuccess) {
    timer.start();
    if (uniform)
      hipLaunchKernelGGL(dist_hist_kernel<true>, dim3(blocks), dim3(DIST_THREADS), lds_bytes, ctx->stream, S->d_x, S->n, d_edges, n_bins,
                         (double)n_bins / span, d_counts);
    else
      hipLaunchKernelGGL(dist_hist_kernel<false>, dim3(blocks), dim3(DIST_THREADS), lds_bytes, ctx->stream, S->d_x, S->n, d_edges, n_bins, 0.0, d_counts);
    timer.stop();
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(counts_out, d_counts, (size_t)n_bins * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return pg_fail(ctx, PG_E_HIP, std::string("dist: ") + hipGetErrorString(e));
  timer.read();
  return PG_OK;
}

extern "C" int pg_dist_kde(pg_ctx* ctx, const double* points, uint32_t n_points, double bandwidth, double* sums_out) {
  if (!ctx) return PG_E_ARG;
  if (!points || !sums_out || n_points == 0) return pg_fail(ctx, PG_E_ARG, "dist: bad argument");
  DistState* S = state_of(ctx);
  if (!S || S->n == 0) return pg_fail(ctx, PG_E_ARG, "dist: no values loaded (call pg_dist_load first)");
  if (n_points > DIST_MAX_POINTS) return pg_fail(ctx, PG_E_ARG, "dist: more than 1024 grid points (one thread per point)");
  if (!(bandwidth > 0.0) || !std::isfinite(bandwidth)) return pg_fail(ctx, PG_E_ARG, "dist: the bandwidth must be finite and positive");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  const uint32_t n_slices = (uint32_t)((S->n + DIST_SLICE - 1) / DIST_SLICE);
  const uint32_t threads = (n_points + 63u) & ~63u;
  PgDevBuf<double> d_points, d_partial, d_sums;
  int rc;
  if ((rc = pg_dev_alloc(ctx, "dist", d_points, n_points, "the grid")) || (rc = pg_dev_alloc(ctx, "dist", d_partial, (size_t)n_slices * n_points, "the partial sums")) ||
      (rc = pg_dev_alloc(ctx, "dist", d_sums, n_points, "the sums")))
    return rc;
  DistTimer timer(ctx, 2);
  hipError_t e = hipMemcpyAsync(d_points, points, (size_t)n_points * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    timer.start();
    hipLaunchKernelGGL(dist_kde_kernel, dim3(n_slices), dim3(threads), 0, ctx->stream, S->d_x, S->n, d_points, n_points, bandwidth, d_partial);
    hipLaunchKernelGGL(dist_kde_sum_kernel, dim3((n_points + 63) / 64), dim3(64), 0, ctx->stream, d_partial, n_slices, n_points, d_sums);
    timer.stop();
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(sums_out, d_sums, (size_t)n_points * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return pg_fail(ctx, PG_E_HIP, std::string("dist: ") + hipGetErrorString(e));
  timer.read();
  return PG_OK;
}

extern "C" int pg_dist_last_ms(pg_ctx* ctx, double* out) {
  if (!ctx) return PG_E_ARG;
  if (!out) return pg_fail(ctx, PG_E_ARG, "dist: bad argument");
  for (int k = 0; k < 3; ++k) out[k] = ctx->profiling ? ctx->dist_ms[k] : 0.0;
  return PG_OK;
}
