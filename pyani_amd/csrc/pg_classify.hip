// pg_classify.hip — the CLASSIFY stage on the GPU: pyani's clique sweep over identity thresholds (reference interface it stands in for:
// pyani/pyani_classify.py:61-165, build_graph_from_results / analyse_cliques / remove_low_weight_edges, and
// pyani/scripts/subcommands/subcmd_classify.py:122-171, trimmed_graph_sequence).  Integer / bit work on two N x N fp64 matrices; no MFMA.
//
// Formulation: the reference removes edges step by step from one graph; step k therefore sees exactly the edges whose
// identity is > theta[k], for a non-decreasing list theta the host derives from the sorted edge identities.  Given theta the steps are
// independent: an edge is alive at step k iff k < death(edge), death = the number of thetas that are < its identity.
//
//   C1 classify_edge_kernel   one thread per (i, j), i < j: the two ordered minima (Python's min(a, b) = b if b < a else a, NaN order
//                             included), the two floor tests, the pair's identity into the N x N weight table (NaN = no edge), a
//                             wave-aggregated append to the list of edge identities, and "the last genome has an edge" (the
//                             reference's node set is every endpoint plus every label but the last, pyani_classify.py:108).
//   C2 classify_death_kernel  one thread per (i, j), i < j: death index by binary search in theta, written to both halves of a symmetric
//                             N x N uint32 table (0 = never alive).  Part of the sweep's profile slot.
//   C3 classify_sweep_kernel  one workgroup per step (grid-stride).  The step's adjacency as a bit matrix, one wave per row: 64 coalesced
//                             death words -> one ballot = one 64-bit word, degree = popcount on the way.  Components by min-label
//                             propagation over the bit rows with one pointer jump per visit (labels only decrease and always name a
//                             member of the own component, so the in-place update needs no double buffer); the fixed point is the
//                             smallest member index.  Component sizes by LDS atomics; a step is "all k-complete" iff every node's degree
//                             is its component's size - 1.  The bit matrix sits in LDS up to N = 1024 (rows padded to an odd number of
//                             words: conflict-free 8-byte reads; 151 568 B with the per-node arrays at N = 1024) and in a per-workgroup slice of
//                             device memory beyond (word-major there, so that the row scans coalesce).
#include <algorithm>

#include "pg_internal.h"
#include "pg_devbuf.h"

namespace {

constexpr uint32_t CL_MAX_N = 8192;          // per-node arrays of the sweep: 3 x 4 x N bytes of LDS (96 KiB at the limit)
constexpr uint32_t CL_LDS_MAX_N = 1024;      // bit matrix in LDS up to here
constexpr size_t CL_LDS_LIMIT = 160 * 1024;

struct ClassifyState {
  uint32_t n = 0, n_nodes = 0;
  uint64_t n_edges = 0;
  PgDevBuf<double> d_w;            // n x n: identity of the pair's edge at [i * n + j], i < j (NaN: no edge)
  PgDevBuf<double> d_edges;        // n_edges identities, unordered
  PgDevBuf<uint32_t> d_death;      // n x n, made by every sweep call
};

// counters: [0] number of edges (the append cursor), [1] != 0: the last genome has an edge
__global__ __launch_bounds__(256) void classify_edge_kernel(const double* __restrict__ ident, const double* __restrict__ cov, uint32_t n, double id_min,
                                                             double cov_min, double* __restrict__ w, double* __restrict__ edges,
                                                             unsigned long long* __restrict__ counters) {
  const uint32_t i = blockIdx.y, j = blockIdx.x * blockDim.x + threadIdx.x;
  const bool pair = j < n && i < j;
  bool edge = false;
  double wi = 0.0;
  if (pair) {
    // column i, column j of the reference's frames: a = M[row j, col i], b = M[row i, col j]; min(a, b) returns b only if b < a
    const size_t ji = (size_t)j * n + i, ij = (size_t)i * n + j;
    const double ia = ident[ji], ib = ident[ij], ca = cov[ji], cb = cov[ij];
    wi = ib < ia ? ib : ia;
    const double wc = cb < ca ? cb : ca;
    edge = wi > id_min && wc > cov_min;
    w[ij] = edge ? wi : __builtin_nan("");
  }
  const unsigned long long m = __ballot(edge);      // wave-uniform; one atomic per wave
  if (m == 0ull) return;
  const int lane = threadIdx.x & 63;
  unsigned long long base = 0;
  if (lane == __builtin_ctzll(m)) base = atomicAdd(&counters[0], (unsigned long long)__popcll(m));
  base = __shfl(base, __builtin_ctzll(m), 64);
  if (edge) {
    edges[base + __popcll(m & ((1ull << lane) - 1ull))] = wi;
    if (j == n - 1) counters[1] = 1ull;
  }
}

__global__ __launch_bounds__(256) void classify_death_kernel(const double* __restrict__ w, uint32_t n, const double* __restrict__ theta, uint32_t n_steps,
                                                              uint32_t* __restrict__ death) {
  const uint32_t i = blockIdx.y, j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n || i > j) return;
  if (i == j) { death[(size_t)i * n + i] = 0u; return; }
  const double x = w[(size_t)i * n + j];
  uint32_t lo = 0;
  if (x == x) {      // an edge: the number of thetas below its identity = the first step that no longer sees it
    uint32_t hi = n_steps;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (theta[mid] < x) lo = mid + 1; else hi = mid; }
  }
  death[(size_t)i * n + j] = lo;
  death[(size_t)j * n + i] = lo;
}

// Nodes 0 .. n_active - 1 form the node set (only the last genome can be outside it).  row_stride: LDS path = words per row, padded odd.
template <bool LDS_ADJ>
__global__ __launch_bounds__(1024) void classify_sweep_kernel(const uint32_t* __restrict__ death, uint32_t n, uint32_t n_active, uint32_t n_words,
                                                               uint32_t row_stride, uint32_t n_steps, unsigned long long* __restrict__ scratch,
                                                               int32_t* __restrict__ n_sub_out, uint8_t* __restrict__ complete_out,
                                                               int32_t* __restrict__ labels_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t np = (n + 3u) & ~3u;
  unsigned long long* adj;
  volatile int* label;
  if (LDS_ADJ) {
    adj = reinterpret_cast<unsigned long long*>(smem);
    label = reinterpret_cast<volatile int*>(smem + (((size_t)n * row_stride * 8 + 15) & ~(size_t)15));
  } else {
    adj = scratch + (size_t)blockIdx.x * n * n_words;
    label = reinterpret_cast<volatile int*>(smem);
  }
  int* deg = const_cast<int*>(label) + np;
  int* size = deg + np;
  int* cnt = size + np;      // [0] components, [1] some node's degree differs from its component's size - 1
  const uint32_t tid = threadIdx.x, nt = blockDim.x, lane = tid & 63u, wave = tid >> 6, n_waves = nt >> 6;
  auto at = [&](uint32_t row, uint32_t word) -> size_t { return LDS_ADJ ? (size_t)row * row_stride + word : (size_t)word * n + row; };

  for (uint32_t step = blockIdx.x; step < n_steps; step += gridDim.x) {
    // 1. the step's adjacency bits and degrees
    for (uint32_t row = wave; row < n; row += n_waves) {
      const uint32_t* __restrict__ drow = death + (size_t)row * n;
      int d = 0;
      for (uint32_t wd = 0; wd < n_words; ++wd) {
        const uint32_t j = 64u * wd + lane;
        const unsigned long long bits = __ballot(j < n && drow[j] > step);
        if (lane == 0) adj[at(row, wd)] = bits;
        d += __popcll(bits);
      }
      if (lane == 0) { deg[row] = d; label[row] = (int)row; size[row] = 0; }
    }
    if (tid == 0) { cnt[0] = 0; cnt[1] = 0; }
    __syncthreads();
    // 2. components: every node takes the smallest label among itself and its neighbours, then that label's label
    for (;;) {
      int changed = 0;
      for (uint32_t i = tid; i < n_active; i += nt) {
        const int cur = label[i];
        int m = cur;
        for (uint32_t wd = 0; wd < n_words; ++wd) {
          unsigned long long bits = adj[at(i, wd)];
          while (bits) {
            const int l = label[64u * wd + (uint32_t)__builtin_ctzll(bits)];
            bits &= bits - 1ull;
            m = l < m ? l : m;
          }
        }
        const int l2 = label[m];
        m = l2 < m ? l2 : m;
        if (m < cur) { label[i] = m; changed = 1; }
      }
      if (!__syncthreads_or(changed)) break;
    }
    // 3. component sizes, then the count and the completeness test
    for (uint32_t i = tid; i < n_active; i += nt) atomicAdd(&size[label[i]], 1);
    __syncthreads();
    int roots = 0, bad = 0;
    for (uint32_t i = tid; i < n; i += nt) {
      int l = -1;
      if (i < n_active) {
        l = label[i];
        roots += l == (int)i;
        bad |= deg[i] != size[l] - 1;
      }
      if (labels_out) labels_out[(size_t)step * n + i] = l;
    }
    if (roots) atomicAdd(&cnt[0], roots);
    if (bad) cnt[1] = 1;
    __syncthreads();
    if (tid == 0) { n_sub_out[step] = cnt[0]; complete_out[step] = cnt[1] ? 0 : 1; }
  }
}

ClassifyState* state_of(pg_ctx* ctx) { return static_cast<ClassifyState*>(ctx->classify_state); }

}  // namespace

void pg_classify_drop(pg_ctx* ctx) {
  if (!ctx->classify_state) return;
  delete state_of(ctx);
  ctx->classify_state = nullptr;
}

extern "C" int pg_classify_release(pg_ctx* ctx) {
  if (!ctx) return PG_E_ARG;
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  pg_classify_drop(ctx);
  return PG_OK;
}

extern "C" int pg_classify_edges(pg_ctx* ctx, const double* identity, const double* coverage, uint32_t n, double id_min, double cov_min,
                                 uint64_t* n_edges_out, uint32_t* n_nodes_out) {
  if (!ctx || !identity || !coverage || n == 0) return pg_fail(ctx, PG_E_ARG, "classify: bad argument");
  if (n > CL_MAX_N) return pg_fail(ctx, PG_E_ARG, "classify: more than 8192 genomes (the sweep's per-node arrays live in LDS)");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  pg_classify_drop(ctx);
  ClassifyState* S = new ClassifyState();
  ctx->classify_state = S;
  const size_t nn = (size_t)n * n;
  PgDevBuf<double> pi, pc;
  PgDevBuf<unsigned long long> pk;
  int rc;
  if ((rc = pg_dev_alloc(ctx, "classify", pi, nn, "the identity matrix")) || (rc = pg_dev_alloc(ctx, "classify", pc, nn, "the coverage matrix")) ||
      (rc = pg_dev_alloc(ctx, "classify", pk, 2, "the edge counters")) || (rc = pg_dev_alloc(ctx, "classify", S->d_w, nn, "the edge weight table")) ||
      (rc = pg_dev_alloc(ctx, "classify", S->d_edges, nn / 2, "the edge list"))) {
    pg_classify_drop(ctx);
    return rc;
  }
  unsigned long long h_cnt[2] = {0, 0};
  hipError_t e = hipMemcpyAsync(pi, identity, nn * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(pc, coverage, nn * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(pk, 0, sizeof(h_cnt), ctx->stream);
  if (e == hipSuccess) {
    pg_prof_begin(ctx, PG_K_CLASSIFY_EDGE);
    hipLaunchKernelGGL(classify_edge_kernel, dim3((n + 255) / 256, n), dim3(256), 0, ctx->stream, pi, pc, n, id_min, cov_min, S->d_w, S->d_edges, pk);
    pg_prof_end(ctx);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h_cnt, pk, sizeof(h_cnt), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    pg_classify_drop(ctx);
    return pg_fail(ctx, PG_E_HIP, std::string("classify: ") + hipGetErrorString(e));
  }
  S->n = n;
  S->n_edges = h_cnt[0];
  S->n_nodes = n - 1 + (h_cnt[1] ? 1u : 0u);
  if (n_edges_out) *n_edges_out = S->n_edges;
  if (n_nodes_out) *n_nodes_out = S->n_nodes;
  return PG_OK;
}

extern "C" int pg_classify_edge_identities(pg_ctx* ctx, double* out, uint64_t cap) {
  if (!ctx) return PG_E_ARG;
  ClassifyState* S = state_of(ctx);
  if (!S || S->n == 0) return pg_fail(ctx, PG_E_ARG, "classify: no edge state (call pg_classify_edges first)");
  if (cap < S->n_edges || (S->n_edges && !out)) return pg_fail(ctx, PG_E_ARG, "classify: the buffer is smaller than the number of edges");
  if (S->n_edges == 0) return PG_OK;
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PG_HIP(ctx, hipMemcpyAsync(out, S->d_edges, S->n_edges * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PG_OK;
}

extern "C" int pg_classify_sweep(pg_ctx* ctx, const double* theta, uint64_t n_steps, int32_t* n_subgraphs_out, uint8_t* complete_out,
                                 int32_t* labels_out) {
  if (!ctx || !theta || !n_subgraphs_out || !complete_out || n_steps == 0) return pg_fail(ctx, PG_E_ARG, "classify: bad argument");
  ClassifyState* S = state_of(ctx);
  if (!S || S->n == 0) return pg_fail(ctx, PG_E_ARG, "classify: no edge state (call pg_classify_edges first)");
  if (n_steps >= (1ull << 31)) return pg_fail(ctx, PG_E_ARG, "classify: more than 2^31 - 1 steps in one call");
  for (uint64_t k = 0; k < n_steps; ++k)
    if (!(theta[k] == theta[k]) || (k && theta[k] < theta[k - 1]))
      return pg_fail(ctx, PG_E_ARG, "classify: the thresholds must be non-decreasing numbers");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  const uint32_t n = S->n, steps = (uint32_t)n_steps, n_words = (n + 63) / 64, np = (n + 3u) & ~3u;
  const size_t nn = (size_t)n * n;
  const bool lds_adj = n <= CL_LDS_MAX_N && !pg_dev_env("PYANI_CLASSIFY_GLOBAL");      // (development switch: the device-memory path at any N)
  const uint32_t row_stride = n_words | 1u;
  const size_t node_bytes = (size_t)3 * np * 4 + 16;
  const size_t lds_bytes = node_bytes + (lds_adj ? (((size_t)n * row_stride * 8 + 15) & ~(size_t)15) : 0);
  if (lds_bytes > CL_LDS_LIMIT) return pg_fail(ctx, PG_E_INTERNAL, "classify: LDS budget exceeded");
  const uint32_t threads = std::min<uint32_t>(1024u, std::max<uint32_t>(64u, (n + 63u) & ~63u));
  const uint32_t per_cu = (uint32_t)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(8, 2048 / threads), CL_LDS_LIMIT / lds_bytes));
  const uint32_t grid = (uint32_t)std::min<uint64_t>(steps, (uint64_t)ctx->num_cu * (lds_adj ? per_cu : 1u));
  int rc;
  if (!S->d_death && (rc = pg_dev_alloc(ctx, "classify", S->d_death, nn, "the death-index table"))) return rc;
  PgDevBuf<double> d_theta;
  PgDevBuf<int32_t> d_sub, d_lab;
  PgDevBuf<uint8_t> d_comp;
  PgDevBuf<unsigned long long> d_scr;
  if ((rc = pg_dev_alloc(ctx, "classify", d_theta, steps, "the thresholds"))) return rc;
  if ((rc = pg_dev_alloc(ctx, "classify", d_sub, steps, "the component counts"))) return rc;
  if ((rc = pg_dev_alloc(ctx, "classify", d_comp, steps, "the completeness flags"))) return rc;
  if (labels_out && (rc = pg_dev_alloc(ctx, "classify", d_lab, (size_t)steps * n, "the per-step labels (ask for fewer steps per call)"))) return rc;
  if (!lds_adj && (rc = pg_dev_alloc(ctx, "classify", d_scr, (size_t)grid * n * n_words, "the adjacency scratch"))) return rc;
  const void* fn = lds_adj ? reinterpret_cast<const void*>(classify_sweep_kernel<true>) : reinterpret_cast<const void*>(classify_sweep_kernel<false>);
  if (lds_bytes > 48 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess) {
    (void)hipGetLastError();
    return pg_fail(ctx, PG_E_CAPACITY, "classify: the sweep needs " + std::to_string(lds_bytes) + " bytes of LDS per workgroup, which this device does not grant");
  }
  hipError_t e = hipMemcpyAsync(d_theta, theta, (size_t)steps * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    pg_prof_begin(ctx, PG_K_CLASSIFY_SWEEP);
    hipLaunchKernelGGL(classify_death_kernel, dim3((n + 255) / 256, n), dim3(256), 0, ctx->stream, S->d_w, n, d_theta, steps, S->d_death);
    if (lds_adj)
      hipLaunchKernelGGL(classify_sweep_kernel<true>, dim3(grid), dim3(threads), lds_bytes, ctx->stream, S->d_death, n, S->n_nodes, n_words, row_stride,
                         steps, d_scr, d_sub, d_comp, d_lab);
    else
      hipLaunchKernelGGL(classify_sweep_kernel<false>, dim3(grid), dim3(threads), lds_bytes, ctx->stream, S->d_death, n, S->n_nodes, n_words, row_stride,
                         steps, d_scr, d_sub, d_comp, d_lab);
    pg_prof_end(ctx);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(n_subgraphs_out, d_sub, (size_t)steps * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(complete_out, d_comp, (size_t)steps, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && labels_out) e = hipMemcpyAsync(labels_out, d_lab, (size_t)steps * n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return pg_fail(ctx, PG_E_HIP, std::string("classify: ") + hipGetErrorString(e));
  return PG_OK;
}
