// pgscr_linkage.inc — part of pg_screen.hip: SPECIES CLUSTERS BY LINKAGE inside every connected component of a list of pairs with distances
// (DESIGN.md §16.11; pyani_amd.screen.linkage_of_pairs is the statement).  Average or complete linkage by scipy's nearest-neighbour chain on
// the component's distance matrix (the maximum over the entries joining two nodes, `fill` where none does), the tree cut at `cutoff`, one
// representative per cluster by score.  Kernel boundaries are the only ordering; no thread waits for another; every store goes through
// vector memory.
//   L1 linkage_init_kernel     parent[v] = v (both forests), best[v] = 0
//   L2 linkage_hook_kernel     one pass over the entries: the hook of the components' K2 (components_hook_nodes); K3 flattens: root
//   L3 linkage_keys_kernel     key[v] = root[v], value[v] = v; ONE stable hipcub radix sort over 20 bits orders the nodes by (root, node);
//                              a component's first node in that order is its root
//   L4 linkage_head_kernel     head[i] = the node at position i is its own root; an exclusive scan numbers the components by ascending root
//   L5 linkage_place_kernel    per position: the component, start[c] at a head; per node: its position and its component.  The local
//                              index of a node is its position minus its component's start.  The host reads `start` once.
//   L6 linkage_scatter_kernel  one thread per entry of the batch's components: both mirror cells take a 64-bit atomic maximum of the
//                              distance's bit pattern WITH THE SIGN BIT SET.  The cells start as 0 bits; a distance is >= 0, so a pattern
//                              with the sign bit is above every untouched cell, and among themselves such patterns order as the doubles do.
//   L7 linkage_fix_kernel      one thread per cell of the batch (its component by binary search over the batch's offsets): a touched cell
//                              loses the sign bit, an untouched one becomes 0.0 on the diagonal and `fill` elsewhere
//   L8 linkage_wave_kernel     components of 2 ... small_limit nodes, ONE WAVE each, launched by class (up to 8, 16, 32, 64 nodes) so that
//                              a wave takes the LDS of its class: the matrix in the wave's own LDS (rows of top | 1 doubles), lane i
//                              owns column i of the row scan, the argmin a butterfly minimum over the lanes that can hold a cluster and
//                              then the lowest lane that attains it ("lowest index wins"), the Lance-Williams update across the lanes,
//                              sizes and chain one register per lane.  No workgroup barrier: the waves of a workgroup run different
//                              components; a wave orders its own LDS traffic.
//   K2 cluster_linkage_kernel  (pg_cluster_linkage.h) every larger component, one workgroup each, in place on its working matrix
//   L9 linkage_cut_kernel      one thread per merge record: height <= cutoff hooks the two slots' nodes into the second forest; K3: cluster
//   L10 linkage_rank_kernel    ranks from the stable radix sort of (~score, index), as the representatives' P1 / P2
//   L11 linkage_best_kernel    best[cluster[v]] = max(0xFFFFFFFF - rank[v]), a run of equal clusters in consecutive lanes reduced first
//   L12 linkage_rep_kernel     rep[v] = order[0xFFFFFFFF - best[cluster[v]]]
// L8 and K2 give the same bits: the minimum and its lowest index do not depend on how the row is divided, and the update is per cell.
namespace {

#include "pg_cluster_linkage.h"      // CLU_MAX_N, ClusterProblem, K2

struct LinkageState {      // the resident result of the latest accepted linkage call
  uint32_t n = 0;
  uint64_t rows = 0;                // n - components: the merge records
  PgDevBuf<int32_t> d_root, d_cluster, d_rep;      // n each
  PgDevBuf<double> d_merges;        // rows x 4
};

LinkageState* linkage_of(pg_ctx* ctx) { return static_cast<LinkageState*>(ctx->screen_linkage_state); }

constexpr uint32_t LINKAGE_SMALL_MAX = 64u, LINKAGE_SMALL_DEFAULT = 32u;
constexpr uint64_t LINKAGE_WORK_DEFAULT = 1ull << 30;      // bytes of working matrices per batch
constexpr unsigned long long LINKAGE_TOUCHED = 0x8000000000000000ull;
constexpr uint32_t LINKAGE_NONE = 0xFFFFFFFFu;

__global__ __launch_bounds__(256) void linkage_init_kernel(uint32_t* __restrict__ parent, uint32_t* __restrict__ best, uint32_t n) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
    parent[v] = v;
    if (best) best[v] = 0u;
  }
}

__global__ __launch_bounds__(256) void linkage_hook_kernel(const int32_t* __restrict__ a, const int32_t* __restrict__ b, uint64_t m, uint32_t n, uint32_t* parent) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t ua = (uint32_t)a[e], ub = (uint32_t)b[e];
    if (ua != ub && ua < n && ub < n) (void)components_hook_nodes(parent, ua, ub);      // (the host has refused an index outside [0, n))
  }
}

__global__ __launch_bounds__(256) void linkage_keys_kernel(const int32_t* __restrict__ root, uint32_t* __restrict__ key, uint32_t* __restrict__ iota, uint32_t n) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) { key[v] = (uint32_t)root[v]; iota[v] = v; }
}

__global__ __launch_bounds__(256) void linkage_head_kernel(const uint32_t* __restrict__ skey, const uint32_t* __restrict__ snode, uint32_t* __restrict__ head, uint32_t n) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) head[i] = skey[i] == snode[i] ? 1u : 0u;
}

__global__ __launch_bounds__(256) void linkage_place_kernel(const uint32_t* __restrict__ snode, const uint32_t* __restrict__ head, const uint32_t* __restrict__ before,
                                                             uint32_t n, uint32_t n_comp, uint32_t* __restrict__ scomp, uint32_t* __restrict__ npos,
                                                             uint32_t* __restrict__ ncomp, uint32_t* __restrict__ start) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t v = snode[i], h = head[i];
    const uint32_t c = before[i] + h - 1u;      // heads up to and including this position, minus one (position 0 is a head)
    if (v >= n || c >= n_comp) continue;        // (never: the sort permutes [0, n), the heads are the roots the flatten counted)
    scomp[i] = c; npos[v] = i; ncomp[v] = c;
    if (h) start[c] = i;
  }
}

__global__ __launch_bounds__(256) void linkage_scatter_kernel(const int32_t* __restrict__ a, const int32_t* __restrict__ b, const double* __restrict__ dist, uint64_t m,
                                                               uint32_t n, const uint32_t* __restrict__ npos, const uint32_t* __restrict__ ncomp,
                                                               const uint32_t* __restrict__ start, const uint32_t* __restrict__ cbatch,
                                                               const unsigned long long* __restrict__ cmat, uint32_t batch, unsigned long long* ws,
                                                               unsigned long long ws_cells) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t ua = (uint32_t)a[e], ub = (uint32_t)b[e];
    if (ua == ub || ua >= n || ub >= n) continue;
    const uint32_t c = ncomp[ua];
    if (ncomp[ub] != c || cbatch[c] != batch) continue;      // (the two ends of an entry share their component)
    const uint32_t st = start[c], s = start[c + 1] - st, i = npos[ua] - st, j = npos[ub] - st;
    const unsigned long long at = cmat[c];
    if (i >= s || j >= s || at + (unsigned long long)s * s > ws_cells) continue;      // (never; kept for the memory's sake)
    const unsigned long long bits = (unsigned long long)__double_as_longlong(dist[e] + 0.0) | LINKAGE_TOUCHED;      // (+ 0.0: -0.0 becomes 0.0)
    atomicMax(ws + at + (unsigned long long)i * s + j, bits);      // no return value
    atomicMax(ws + at + (unsigned long long)j * s + i, bits);
  }
}

__global__ __launch_bounds__(256) void linkage_fix_kernel(unsigned long long* __restrict__ ws, unsigned long long cells, const unsigned long long* __restrict__ w_off,
                                                           const uint32_t* __restrict__ w_size, uint32_t count, double fill) {
  const unsigned long long fill_bits = (unsigned long long)__double_as_longlong(fill);
  for (unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; t < cells; t += (unsigned long long)gridDim.x * blockDim.x) {
    uint32_t lo = 0, hi = count;      // the last k with w_off[k] <= t (w_off[0] == 0)
    while (hi - lo > 1u) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (w_off[mid] <= t) lo = mid; else hi = mid;
    }
    const unsigned long long r = t - w_off[lo];
    const uint32_t s = w_size[lo];
    const unsigned long long raw = ws[t];
    ws[t] = (raw & LINKAGE_TOUCHED) ? (raw & ~LINKAGE_TOUCHED) : (r / s == r % s ? 0ull : fill_bits);
  }
}

// The wave's own LDS traffic in program order: what its lanes stored before is what its lanes load after.
__device__ __forceinline__ void linkage_wave_order() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ double linkage_uniform(double v) {      // the first lane's value, for the scalar unit (every lane holds the same)
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(u >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__global__ __launch_bounds__(256) void linkage_wave_kernel(const uint32_t* __restrict__ list, uint32_t count, const unsigned long long* __restrict__ w_off,
                                                            const uint32_t* __restrict__ w_size, const unsigned long long* __restrict__ w_row,
                                                            const double* __restrict__ ws, double* __restrict__ merges, uint32_t limit, uint32_t ld, int method) {
  extern __shared__ __attribute__((aligned(16))) unsigned char linkage_lds[];
  const uint32_t lane = threadIdx.x & 63u, wib = threadIdx.x >> 6;
  const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + wib;
  if (wave >= count) return;      // (the last workgroup may be partly filled; nothing below meets another wave)
  const uint32_t k = list[wave];
  const uint32_t s = w_size[k];
  if (s < 2u || s > limit || limit > LINKAGE_SMALL_MAX || ld < limit) return;      // (never: the records stay unwritten and the result is refused)
  double* D = reinterpret_cast<double*>(linkage_lds) + (size_t)wib * limit * ld;
  const double* src = ws + w_off[k];
  for (uint32_t t = lane; t < s * s; t += 64u) {
    const uint32_t i = t / s;
    D[i * ld + (t - i * s)] = src[t];
  }
  linkage_wave_order();
  double* rec = merges + w_row[k] * 4ull;
  const double INF = __builtin_huge_val();
  uint32_t size = lane < s ? 1u : 0u;      // of cluster `lane`
  uint32_t span = 2u;                      // the power of two that covers the s lanes
  while (span < s) span <<= 1;
  uint32_t chain = 0u;                     // element `lane` of the chain
  uint32_t len = 0, x = 0, prev = 0;
  double cur = INF;
  for (uint32_t merge = 0; merge + 1 < s; ++merge) {
    if (len == 0) {
      const unsigned long long live = __ballot(size != 0u);
      if (!live) return;      // (never)
      x = (uint32_t)__ffsll((long long)live) - 1u;      // the lowest live index
      if (lane == 0u) chain = x;
      len = 1;
      cur = INF;
    }
    for (uint32_t step = 0;; ++step) {
      if (step > LINKAGE_SMALL_MAX + 1u) return;      // (never: a step ends the chain or lengthens it, and it holds at most s clusters)
      // row argmin over the live clusters other than x: the minimum over lanes 0 ... span - 1 (a butterfly: lane 0 ends with it), then
      // the LOWEST lane that holds it — scipy's ascending scan with strict <
      const bool live = lane < s && lane != x && size != 0u;
      const double mine = live ? D[x * ld + lane] : INF;
      double bv = mine;
      for (uint32_t off = span >> 1; off > 0u; off >>= 1) {
        const double ov = __shfl_xor(bv, (int)off, 64);
        if (ov < bv) bv = ov;
      }
      bv = linkage_uniform(bv);
      const unsigned long long at = __ballot(live && mine == bv);
      const uint32_t bi = at ? (uint32_t)__ffsll((long long)at) - 1u : LINKAGE_NONE;
      uint32_t y = prev;
      if (bv < cur) { cur = bv; y = bi; }
      if (len > 1 && y == prev) break;
      if (y >= s || len >= s) return;      // (never: a matrix that is not finite)
      if (lane == len) chain = y;
      ++len;
      prev = x;
      x = y;
    }
    // merge the tip and the element under it
    len -= 2;
    const uint32_t lo = x < prev ? x : prev, hi = x < prev ? prev : x;
    const uint32_t nlo = __shfl(size, (int)lo, 64), nhi = __shfl(size, (int)hi, 64);
    if (lane == 0u) {
      rec[(size_t)merge * 4 + 0] = (double)lo;
      rec[(size_t)merge * 4 + 1] = (double)hi;
      rec[(size_t)merge * 4 + 2] = cur;
      rec[(size_t)merge * 4 + 3] = (double)(nlo + nhi);
    }
    const double flo = (double)nlo, fhi = (double)nhi, fsum = (double)(nlo + nhi);
    if (lane < s && lane != lo && lane != hi && size != 0u) {
      const double a = D[lo * ld + lane], b = D[hi * ld + lane];
      double v;
      if (method == PG_CLUSTER_AVERAGE) {
        const double pa = flo * a, pb = fhi * b;
        v = (pa + pb) / fsum;
      } else {
        v = a > b ? a : b;
      }
      D[hi * ld + lane] = v;
      D[lane * ld + hi] = v;
    }
    if (lane == lo) size = 0u;
    if (lane == hi) size = nlo + nhi;
    linkage_wave_order();
    if (len >= 1) {
      x = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl(chain, (int)(len - 1), 64));
      if (len >= 2) {
        prev = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl(chain, (int)(len - 2), 64));
        if (x >= s || prev >= s) return;      // (never)
        cur = linkage_uniform(D[x * ld + prev]);
      } else {
        cur = INF;
      }
    }
  }
}

__global__ __launch_bounds__(256) void linkage_cut_kernel(const uint32_t* __restrict__ snode, const uint32_t* __restrict__ head, const uint32_t* __restrict__ scomp,
                                                           const uint32_t* __restrict__ start, const double* __restrict__ merges, uint32_t n, unsigned long long rows,
                                                           double cutoff, uint32_t* parent) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    if (head[i]) continue;      // a component of s nodes owns s - 1 records: one per position behind its head
    const uint32_t c = scomp[i], st = start[c], s = start[c + 1] - st;
    const unsigned long long row = (unsigned long long)i - c - 1ull;      // (start[c] - c) + (i - start[c] - 1)
    if (row >= rows) continue;      // (never)
    const double* rec = merges + row * 4ull;
    const double x = rec[0], y = rec[1];
    if (!(rec[2] <= cutoff) || !(x >= 0.0 && x < (double)s) || !(y >= 0.0 && y < (double)s)) continue;      // (an unwritten record is NaN everywhere)
    const uint32_t u = snode[st + (uint32_t)x], v = snode[st + (uint32_t)y];
    if (u != v && u < n && v < n) (void)components_hook_nodes(parent, u, v);
  }
}

__global__ __launch_bounds__(256) void linkage_rank_kernel(unsigned long long* __restrict__ keys, uint32_t* __restrict__ iota, uint32_t n) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) { keys[v] = ~keys[v]; iota[v] = v; }
}

__global__ __launch_bounds__(256) void linkage_best_kernel(const int32_t* __restrict__ cluster, const uint32_t* __restrict__ rank, uint32_t n, uint32_t* __restrict__ best) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {      // (uniform over the workgroup: every lane reaches the shuffles)
    const uint32_t v = base + threadIdx.x;
    uint32_t dest = LINKAGE_NONE, val = 0u;
    if (v < n) { dest = (uint32_t)cluster[v]; val = 0xFFFFFFFFu - rank[v]; }
    // runs of equal destination in consecutive lanes, as the representatives' assign: the run's maximum ends at its head
    const uint32_t before = __shfl_up(dest, 1, 64);
    const bool is_head = lane == 0u || dest != before;
    const unsigned long long heads = __ballot(is_head);
    const uint32_t run = (uint32_t)__popcll(heads & ((2ull << lane) - 1ull));      // (lane 63: 2 << 63 wraps to 0, minus one = every bit)
    for (uint32_t d = 1; d < 64u; d <<= 1) {
      const uint32_t r2 = __shfl_down(run, d, 64), v2 = __shfl_down(val, d, 64);
      if (lane + d < 64u && r2 == run && v2 > val) val = v2;
    }
    if (is_head && dest < n) atomicMax(best + dest, val);      // no return value
  }
}

__global__ __launch_bounds__(256) void linkage_rep_kernel(const int32_t* __restrict__ cluster, const uint32_t* __restrict__ best, const uint32_t* __restrict__ order, uint32_t n,
                                                           int32_t* __restrict__ rep) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
    const uint32_t c = (uint32_t)cluster[v];
    const uint32_t at = c < n ? 0xFFFFFFFFu - best[c] : LINKAGE_NONE;      // the rank of the cluster's best member
    rep[v] = at < n ? (int32_t)order[at] : -1;                            // (-1: never — every cluster has a member; the host refuses such a result)
  }
}

struct LinkagePlan {      // what the host makes of the components' sizes: the work list (components of >= 2 nodes, ascending root) cut into batches
  std::vector<unsigned long long> w_off, w_row;      // cell offset inside its batch's working matrices; first merge record
  std::vector<uint32_t> w_size, w_comp;
  std::vector<uint32_t> cbatch;                      // per component: its batch, LINKAGE_NONE for a singleton
  std::vector<unsigned long long> cmat;              // per component: w_off
  struct Batch { uint32_t k0, k1; unsigned long long cells; uint32_t small0[5]; uint32_t large0[4]; };      // small0 / large0[q] ... [q + 1]: class q
  std::vector<Batch> batches;
  std::vector<uint32_t> small;                       // work-list indices, batch after batch
  std::vector<ClusterProblem> large;                 // batch after batch, class after class
  unsigned long long max_cells = 0;
  uint32_t largest = 0;
};

constexpr uint32_t LINKAGE_WAVE_TOP[4] = {8u, 16u, 32u, LINKAGE_SMALL_MAX};      // L8's launches: a wave's LDS is sized by its class (each top capped by small_limit)
constexpr uint32_t LINKAGE_CLASS_TOP[3] = {64u, 256u, CLU_MAX_N};      // K2's launches: problems of up to 64, 256 and 8192 nodes (64, 256, 1024 threads)

}  // namespace

void pg_screen_linkage_drop(pg_ctx* ctx) {
  if (!ctx->screen_linkage_state) return;
  delete linkage_of(ctx);
  ctx->screen_linkage_state = nullptr;
  ctx->screen_linkage_stats = PgScreenLinkageStats{};
}

extern "C" int pg_screen_linkage_release(pg_ctx* ctx) {
  if (!ctx) return PG_E_ARG;
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  pg_screen_linkage_drop(ctx);
  return PG_OK;
}

extern "C" int pg_screen_linkage_set(pg_ctx* ctx, uint32_t small_limit, uint64_t work_bytes) {
  if (!ctx) return PG_E_ARG;
  if (small_limit > LINKAGE_SMALL_MAX && small_limit != PG_SCREEN_LINKAGE_DEFAULT)
    return pg_fail(ctx, PG_E_ARG, "screen: the linkage's small limit is 0 ... 64 nodes (or PG_SCREEN_LINKAGE_DEFAULT), not " + std::to_string(small_limit));
  if (work_bytes > (1ull << 40)) return pg_fail(ctx, PG_E_ARG, "screen: the linkage's working matrices take at most 2^40 bytes per batch, not " + std::to_string(work_bytes));
  ctx->screen_linkage_small = small_limit;      // (PG_SCREEN_LINKAGE_DEFAULT and 0 bytes stay as they are: the call reads the defaults)
  ctx->screen_linkage_work = work_bytes;
  return PG_OK;
}

extern "C" int pg_screen_linkage_last(pg_ctx* ctx, uint64_t* counts_out, double* ms_out) {
  if (!ctx || !counts_out || !ms_out) return pg_fail(ctx, PG_E_ARG, "bad argument");
  const PgScreenLinkageStats& L = ctx->screen_linkage_stats;
  counts_out[0] = L.nodes; counts_out[1] = L.worked; counts_out[2] = L.ignored; counts_out[3] = L.components; counts_out[4] = L.worked_components;
  counts_out[5] = L.largest; counts_out[6] = L.clusters; counts_out[7] = L.batches;
  ms_out[0] = L.group_ms; ms_out[1] = L.fill_ms; ms_out[2] = L.small_ms; ms_out[3] = L.large_ms; ms_out[4] = L.cut_ms;
  return PG_OK;
}

extern "C" int pg_screen_linkage_read(pg_ctx* ctx, int32_t* root_out, int32_t* cluster_out, int32_t* rep_out) {
  if (!ctx) return PG_E_ARG;
  LinkageState* S = linkage_of(ctx);
  if (!S) return pg_fail(ctx, PG_E_ARG, "screen: no resident linkage (call pg_screen_linkage first)");
  if (!root_out || !cluster_out || !rep_out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  PG_HIP(ctx, hipMemcpyAsync(root_out, S->d_root, (size_t)S->n * 4, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipMemcpyAsync(cluster_out, S->d_cluster, (size_t)S->n * 4, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipMemcpyAsync(rep_out, S->d_rep, (size_t)S->n * 4, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipStreamSynchronize(st));
  return PG_OK;
}

extern "C" int pg_screen_linkage_read_merges(pg_ctx* ctx, double* merges_out) {
  if (!ctx) return PG_E_ARG;
  LinkageState* S = linkage_of(ctx);
  if (!S) return pg_fail(ctx, PG_E_ARG, "screen: no resident linkage (call pg_screen_linkage first)");
  if (!S->rows) return PG_OK;      // every component is one node: nothing to copy, merges_out may be NULL
  if (!merges_out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PG_HIP(ctx, hipMemcpyAsync(merges_out, S->d_merges, (size_t)S->rows * 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PG_OK;
}

namespace {

// The batches of the components whose sizes stand in start[0 ... n_comp] (start[n_comp] == n).  PG_E_CAPACITY for a component beyond K2's limit.
int linkage_plan(pg_ctx* ctx, const std::vector<uint32_t>& start, uint32_t n_comp, uint64_t work_bytes, LinkagePlan& P) {
  P.cbatch.assign(n_comp, LINKAGE_NONE);
  P.cmat.assign(n_comp, 0ull);
  for (uint32_t c = 0; c < n_comp; ++c) {
    if (start[c + 1] <= start[c]) return pg_fail(ctx, PG_E_INTERNAL, "screen: the linkage's components do not stand in ascending order");
    P.largest = std::max(P.largest, start[c + 1] - start[c]);
  }
  if (P.largest > CLU_MAX_N)
    return pg_fail(ctx, PG_E_CAPACITY, "screen: a component of " + std::to_string(P.largest) + " nodes is beyond the linkage's " + std::to_string(CLU_MAX_N) +
                                           " (its sizes and chain live in LDS); a tighter screen threshold splits it");
  const unsigned long long budget_cells = std::max<uint64_t>(work_bytes / 8, 1);
  LinkagePlan::Batch B{};
  bool open = false;
  const auto close = [&]() {
    if (!open) return;
    B.k1 = (uint32_t)P.w_size.size();
    P.max_cells = std::max(P.max_cells, B.cells);
    P.batches.push_back(B);
    open = false;
  };
  for (uint32_t c = 0; c < n_comp; ++c) {
    const uint32_t s = start[c + 1] - start[c];
    if (s < 2) continue;
    const unsigned long long cells = (unsigned long long)s * s;
    if (open && B.cells + cells > budget_cells) close();      // (a component beyond the budget has a batch to itself)
    if (!open) { B = LinkagePlan::Batch{}; B.k0 = (uint32_t)P.w_size.size(); open = true; }
    P.cbatch[c] = (uint32_t)P.batches.size();
    P.cmat[c] = B.cells;
    P.w_off.push_back(B.cells); P.w_row.push_back((unsigned long long)start[c] - c); P.w_size.push_back(s); P.w_comp.push_back(c);
    B.cells += cells;
  }
  close();
  return PG_OK;
}

// The launch lists of the plan: per batch the small components' work-list indices and K2's problems by class (ws, merges: the device blocks).
void linkage_lists(LinkagePlan& P, uint32_t small_limit, double* ws, double* merges, const int* flag, int method) {
  for (auto& B : P.batches) {
    for (int q = 0; q < 4; ++q) {
      B.small0[q] = (uint32_t)P.small.size();
      const uint32_t top = std::min(LINKAGE_WAVE_TOP[q], small_limit), under = q ? std::min(LINKAGE_WAVE_TOP[q - 1], small_limit) : 1u;
      for (uint32_t k = B.k0; k < B.k1; ++k)
        if (P.w_size[k] > under && P.w_size[k] <= top) P.small.push_back(k);
    }
    B.small0[4] = (uint32_t)P.small.size();
    for (int q = 0; q < 3; ++q) {
      B.large0[q] = (uint32_t)P.large.size();
      for (uint32_t k = B.k0; k < B.k1; ++k) {
        const uint32_t s = P.w_size[k];
        if (s <= small_limit || s > LINKAGE_CLASS_TOP[q] || (q && s <= LINKAGE_CLASS_TOP[q - 1])) continue;
        ClusterProblem c;
        c.work = ws + P.w_off[k]; c.merges = merges + P.w_row[k] * 4ull; c.flag = flag; c.n = s; c.method = method;
        P.large.push_back(c);
      }
    }
    B.large0[3] = (uint32_t)P.large.size();
  }
}

}  // namespace

extern "C" int pg_screen_linkage(pg_ctx* ctx, const int32_t* a, const int32_t* b, const double* dist, uint64_t m, uint32_t n, const uint64_t* score, int method,
                                 double cutoff, double fill, uint32_t* n_clusters_out) {
  if (!ctx) return PG_E_ARG;
  if (n < 1 || n > pgscr::INDEX_MAX_GENOMES) return pg_fail(ctx, PG_E_ARG, "screen: a linkage is of 1 ... 1048576 (2^20) nodes, not " + std::to_string(n));
  if (!score) return pg_fail(ctx, PG_E_ARG, "screen: the linkage needs a score for every node");
  if (!n_clusters_out || (m && (!a || !b || !dist))) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  if (method != PG_CLUSTER_AVERAGE && method != PG_CLUSTER_COMPLETE) return pg_fail(ctx, PG_E_ARG, "screen: the linkage's method is PG_CLUSTER_AVERAGE or PG_CLUSTER_COMPLETE");
  const double top = 1.79769313486231570815e308;
  if (!(cutoff >= 0.0 && cutoff <= top) || !(fill >= 0.0 && fill <= top) || !(cutoff < fill))
    return pg_fail(ctx, PG_E_ARG, "screen: the linkage needs finite 0 <= cutoff < fill");
  uint64_t ignored = 0;
  for (uint64_t i = 0; i < m; ++i) {      // before anything is copied or replaced
    if ((uint32_t)a[i] >= n || (uint32_t)b[i] >= n)
      return pg_fail(ctx, PG_E_ARG, "screen: entry " + std::to_string(i) + " names node " + std::to_string((uint32_t)a[i] >= n ? a[i] : b[i]) + " outside [0, " +
                                        std::to_string(n) + ")");
    if (!(dist[i] >= 0.0 && dist[i] <= top)) return pg_fail(ctx, PG_E_ARG, "screen: the distance of entry " + std::to_string(i) + " is not finite and >= 0");
    ignored += a[i] == b[i] ? 1u : 0u;
  }
  PG_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const uint32_t small_limit = ctx->screen_linkage_small == PG_SCREEN_LINKAGE_DEFAULT ? LINKAGE_SMALL_DEFAULT : ctx->screen_linkage_small;
  const uint64_t work_bytes = ctx->screen_linkage_work ? ctx->screen_linkage_work : LINKAGE_WORK_DEFAULT;
  const uint32_t cu_blocks = (uint32_t)ctx->num_cu * 8u;
  const dim3 node_grid(grid_for(n, 256, cu_blocks)), entry_grid(grid_for(m, 256, cu_blocks * 4u));

  std::unique_ptr<LinkageState> S(new LinkageState());
  PgDevBuf<int32_t> d_a, d_b;
  PgDevBuf<double> d_dist, d_ws;
  PgDevBuf<uint32_t> parent, key, iota, skey, snode, head, before, scomp, npos, ncomp, start, cbatch, w_size, small, best, order, rank;
  PgDevBuf<unsigned long long> count, cmat, w_off, w_row, keys_in, keys_out;
  PgDevBuf<ClusterProblem> large;
  PgDevBuf<int> flag;
  PgDevBuf<uint8_t> tmp;
  size_t tmp_bytes = 0;
  LinkagePlan P;
  std::vector<uint32_t> h_start;
  ScreenEvents T;
  unsigned long long n_comp = 0, n_clusters = 0;

  const auto run = [&]() -> int {
    int rc;
    PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& bytes) {
      return hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int64_t)n, 0, 20, st);
    }));
    PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& bytes) {
      return hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                                (int64_t)n, 0, 64, st);
    }));
    PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& bytes) { return hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int64_t)n, st); }));
    if ((rc = pg_dev_alloc(ctx, "screen", S->d_root, n, "the linkage's roots")) || (rc = pg_dev_alloc(ctx, "screen", S->d_cluster, n, "the linkage's clusters")) ||
        (rc = pg_dev_alloc(ctx, "screen", S->d_rep, n, "the linkage's representatives")) || (rc = pg_dev_alloc(ctx, "screen", d_a, (size_t)m, "the entries")) ||
        (rc = pg_dev_alloc(ctx, "screen", d_b, (size_t)m, "the entries")) || (rc = pg_dev_alloc(ctx, "screen", d_dist, (size_t)m, "the entries' distances")) ||
        (rc = pg_dev_alloc(ctx, "screen", parent, n, "the linkage's forest")) || (rc = pg_dev_alloc(ctx, "screen", key, n, "the nodes' roots")) ||
        (rc = pg_dev_alloc(ctx, "screen", iota, n, "the nodes")) || (rc = pg_dev_alloc(ctx, "screen", skey, n, "the sorted roots")) ||
        (rc = pg_dev_alloc(ctx, "screen", snode, n, "the sorted nodes")) || (rc = pg_dev_alloc(ctx, "screen", head, n, "the components' heads")) ||
        (rc = pg_dev_alloc(ctx, "screen", before, n, "the components' numbers")) || (rc = pg_dev_alloc(ctx, "screen", scomp, n, "the positions' components")) ||
        (rc = pg_dev_alloc(ctx, "screen", npos, n, "the nodes' positions")) || (rc = pg_dev_alloc(ctx, "screen", ncomp, n, "the nodes' components")) ||
        (rc = pg_dev_alloc(ctx, "screen", best, n, "the clusters' best ranks")) || (rc = pg_dev_alloc(ctx, "screen", order, n, "the order of the nodes")) ||
        (rc = pg_dev_alloc(ctx, "screen", rank, n, "the ranks of the nodes")) || (rc = pg_dev_alloc(ctx, "screen", keys_in, n, "the score keys")) ||
        (rc = pg_dev_alloc(ctx, "screen", keys_out, n, "the score keys")) || (rc = pg_dev_alloc(ctx, "screen", count, 2, "the linkage's counters")) ||
        (rc = pg_dev_alloc(ctx, "screen", flag, 1, "the linkage's flag")) || (rc = pg_dev_alloc(ctx, "screen", tmp, tmp_bytes, "the sort's temporary storage")))
      return rc;
    S->n = n;
    if (m) {
      PG_HIP(ctx, hipMemcpyAsync(d_a, a, (size_t)m * 4, hipMemcpyHostToDevice, st));
      PG_HIP(ctx, hipMemcpyAsync(d_b, b, (size_t)m * 4, hipMemcpyHostToDevice, st));
      PG_HIP(ctx, hipMemcpyAsync(d_dist, dist, (size_t)m * 8, hipMemcpyHostToDevice, st));
    }
    PG_HIP(ctx, hipMemcpyAsync(keys_in, score, (size_t)n * 8, hipMemcpyHostToDevice, st));
    PG_HIP(ctx, hipMemsetAsync(count, 0, 16, st));
    PG_HIP(ctx, hipMemsetAsync(flag, 0, sizeof(int), st));
    // 1. group
    {
      ScreenEvents::Stage group(T, ST_GROUP, st);
      hipLaunchKernelGGL(linkage_init_kernel, node_grid, dim3(256), 0, st, parent.p, (uint32_t*)nullptr, n);
      if (m) hipLaunchKernelGGL(linkage_hook_kernel, entry_grid, dim3(256), 0, st, (const int32_t*)d_a.p, (const int32_t*)d_b.p, m, n, parent.p);
      hipLaunchKernelGGL(components_flatten_kernel, node_grid, dim3(256), 0, st, parent.p, n, S->d_root.p, count.p);
      hipLaunchKernelGGL(linkage_keys_kernel, node_grid, dim3(256), 0, st, (const int32_t*)S->d_root.p, key.p, iota.p, n);
      PG_HIP(ctx, hipGetLastError());
      size_t tb = tmp_bytes;
      PG_HIP(ctx, hipcub::DeviceRadixSort::SortPairs((void*)tmp.p, tb, (const uint32_t*)key.p, skey.p, (const uint32_t*)iota.p, snode.p, (int64_t)n, 0, 20, st));
      hipLaunchKernelGGL(linkage_head_kernel, node_grid, dim3(256), 0, st, (const uint32_t*)skey.p, (const uint32_t*)snode.p, head.p, n);
      PG_HIP(ctx, hipGetLastError());
      tb = tmp_bytes;
      PG_HIP(ctx, hipcub::DeviceScan::ExclusiveSum((void*)tmp.p, tb, (const uint32_t*)head.p, before.p, (int64_t)n, st));
    }
    PG_HIP(ctx, hipMemcpyAsync(&n_comp, count, 8, hipMemcpyDeviceToHost, st));
    PG_HIP(ctx, hipStreamSynchronize(st));
    if (n_comp < 1 || n_comp > n) return pg_fail(ctx, PG_E_INTERNAL, "screen: " + std::to_string(n_comp) + " components of " + std::to_string(n) + " nodes");
    const uint32_t C = (uint32_t)n_comp;
    if ((rc = pg_dev_alloc(ctx, "screen", start, (size_t)C + 1, "the components' starts"))) return rc;
    h_start.assign((size_t)C + 1, 0u);
    h_start[C] = n;
    PG_HIP(ctx, hipMemsetAsync(start, 0xFF, ((size_t)C + 1) * 4, st));
    PG_HIP(ctx, hipMemcpyAsync(start.p + C, h_start.data() + C, 4, hipMemcpyHostToDevice, st));
    {
      ScreenEvents::Stage group(T, ST_GROUP, st);
      hipLaunchKernelGGL(linkage_place_kernel, node_grid, dim3(256), 0, st, (const uint32_t*)snode.p, (const uint32_t*)head.p, (const uint32_t*)before.p, n, C, scomp.p, npos.p,
                         ncomp.p, start.p);
      PG_HIP(ctx, hipGetLastError());
    }
    PG_HIP(ctx, hipMemcpyAsync(h_start.data(), start, (size_t)C * 4, hipMemcpyDeviceToHost, st));
    PG_HIP(ctx, hipStreamSynchronize(st));
    if (h_start[0] != 0u) return pg_fail(ctx, PG_E_INTERNAL, "screen: the linkage's first component does not start at 0");
    if ((rc = linkage_plan(ctx, h_start, C, work_bytes, P))) return rc;      // (PG_E_CAPACITY: before any matrix is allocated)
    S->rows = (uint64_t)n - C;
    const size_t W = P.w_size.size();
    if ((rc = pg_dev_alloc(ctx, "screen", S->d_merges, (size_t)S->rows * 4, "the merge records")) ||
        (rc = pg_dev_alloc(ctx, "screen", d_ws, (size_t)P.max_cells, "the working matrices (pg_screen_linkage_set takes a smaller budget)")) ||
        (rc = pg_dev_alloc(ctx, "screen", cbatch, C, "the components' batches")) || (rc = pg_dev_alloc(ctx, "screen", cmat, C, "the components' matrices")) ||
        (rc = pg_dev_alloc(ctx, "screen", w_off, W, "the work list")) || (rc = pg_dev_alloc(ctx, "screen", w_row, W, "the work list")) ||
        (rc = pg_dev_alloc(ctx, "screen", w_size, W, "the work list")))
      return rc;
    linkage_lists(P, small_limit, d_ws.p, S->d_merges.p, flag.p, method);
    if ((rc = pg_dev_alloc(ctx, "screen", small, P.small.size(), "the small components")) || (rc = pg_dev_alloc(ctx, "screen", large, P.large.size(), "the large components")))
      return rc;
    PG_HIP(ctx, hipMemsetAsync(S->d_merges, 0xFF, std::max<size_t>((size_t)S->rows * 32, 8), st));      // NaN until written
    PG_HIP(ctx, hipMemcpyAsync(cbatch, P.cbatch.data(), (size_t)C * 4, hipMemcpyHostToDevice, st));
    PG_HIP(ctx, hipMemcpyAsync(cmat, P.cmat.data(), (size_t)C * 8, hipMemcpyHostToDevice, st));
    if (W) {
      PG_HIP(ctx, hipMemcpyAsync(w_off, P.w_off.data(), W * 8, hipMemcpyHostToDevice, st));
      PG_HIP(ctx, hipMemcpyAsync(w_row, P.w_row.data(), W * 8, hipMemcpyHostToDevice, st));
      PG_HIP(ctx, hipMemcpyAsync(w_size, P.w_size.data(), W * 4, hipMemcpyHostToDevice, st));
    }
    if (!P.small.empty()) PG_HIP(ctx, hipMemcpyAsync(small, P.small.data(), P.small.size() * 4, hipMemcpyHostToDevice, st));
    if (!P.large.empty()) PG_HIP(ctx, hipMemcpyAsync(large, P.large.data(), P.large.size() * sizeof(ClusterProblem), hipMemcpyHostToDevice, st));
    // the launch shapes of the two linkage kernels
    const auto wave_shape = [&](int q, uint32_t& top, uint32_t& ld, uint32_t& waves) -> size_t {      // the LDS bytes of a workgroup of class q
      top = std::min(LINKAGE_WAVE_TOP[q], small_limit);
      ld = top | 1u;
      waves = top <= 32u ? 4u : 2u;
      return (size_t)waves * top * ld * sizeof(double);
    };
    uint32_t top3, ld3, waves3;
    const size_t wave_lds = wave_shape(3, top3, ld3, waves3);      // the largest of the four
    if (!P.small.empty() && wave_lds > 48 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(linkage_wave_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)wave_lds) != hipSuccess) {
      (void)hipGetLastError();
      return pg_fail(ctx, PG_E_CAPACITY, "screen: the wave linkage needs " + std::to_string(wave_lds) + " bytes of LDS per workgroup, which this device does not grant");
    }
    const size_t top_lds = clu_linkage_lds(std::max(P.largest, 2u));
    if (!P.large.empty() && top_lds > 48 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(cluster_linkage_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)top_lds) != hipSuccess) {
      (void)hipGetLastError();
      return pg_fail(ctx, PG_E_CAPACITY, "screen: the linkage needs " + std::to_string(top_lds) + " bytes of LDS per workgroup, which this device does not grant");
    }
    // 2. fill, 3. linkage: batch after batch on the one block of working matrices
    for (uint32_t q = 0; q < P.batches.size(); ++q) {
      const LinkagePlan::Batch& B = P.batches[q];
      {
        ScreenEvents::Stage fill_stage(T, ST_FILL, st);
        PG_HIP(ctx, hipMemsetAsync(d_ws, 0, (size_t)B.cells * 8, st));
        hipLaunchKernelGGL(linkage_scatter_kernel, entry_grid, dim3(256), 0, st, (const int32_t*)d_a.p, (const int32_t*)d_b.p, (const double*)d_dist.p, m, n,
                           (const uint32_t*)npos.p, (const uint32_t*)ncomp.p, (const uint32_t*)start.p, (const uint32_t*)cbatch.p, (const unsigned long long*)cmat.p, q,
                           reinterpret_cast<unsigned long long*>(d_ws.p), B.cells);
        hipLaunchKernelGGL(linkage_fix_kernel, dim3(grid_for(B.cells, 256, cu_blocks * 4u)), dim3(256), 0, st, reinterpret_cast<unsigned long long*>(d_ws.p), B.cells,
                           (const unsigned long long*)(w_off.p + B.k0), (const uint32_t*)(w_size.p + B.k0), B.k1 - B.k0, fill);
        PG_HIP(ctx, hipGetLastError());
      }
      if (B.small0[4] > B.small0[0]) {
        ScreenEvents::Stage small_stage(T, ST_SMALL, st);
        for (int k = 0; k < 4; ++k) {
          const uint32_t cnt = B.small0[k + 1] - B.small0[k];
          if (!cnt) continue;
          uint32_t top, ld, waves;
          const size_t lds = wave_shape(k, top, ld, waves);
          hipLaunchKernelGGL(linkage_wave_kernel, dim3((cnt + waves - 1) / waves), dim3(64 * waves), lds, st, (const uint32_t*)(small.p + B.small0[k]), cnt,
                             (const unsigned long long*)w_off.p, (const uint32_t*)w_size.p, (const unsigned long long*)w_row.p, (const double*)d_ws.p, S->d_merges.p, top, ld, method);
        }
        PG_HIP(ctx, hipGetLastError());
      }
      if (B.large0[3] > B.large0[0]) {
        ScreenEvents::Stage large_stage(T, ST_LARGE, st);
        for (int k = 0; k < 3; ++k) {
          const uint32_t cnt = B.large0[k + 1] - B.large0[k];
          if (!cnt) continue;
          const uint32_t top = std::min(LINKAGE_CLASS_TOP[k], std::max(P.largest, 2u));
          hipLaunchKernelGGL(cluster_linkage_kernel, dim3(cnt), dim3(clu_linkage_threads(top)), clu_linkage_lds(top), st, (const ClusterProblem*)(large.p + B.large0[k]));
        }
        PG_HIP(ctx, hipGetLastError());
      }
    }
    // 4. cut and representatives
    {
      ScreenEvents::Stage cut(T, ST_CUT, st);
      hipLaunchKernelGGL(linkage_init_kernel, node_grid, dim3(256), 0, st, parent.p, best.p, n);
      hipLaunchKernelGGL(linkage_cut_kernel, node_grid, dim3(256), 0, st, (const uint32_t*)snode.p, (const uint32_t*)head.p, (const uint32_t*)scomp.p, (const uint32_t*)start.p,
                         (const double*)S->d_merges.p, n, (unsigned long long)S->rows, cutoff, parent.p);
      hipLaunchKernelGGL(components_flatten_kernel, node_grid, dim3(256), 0, st, parent.p, n, S->d_cluster.p, count.p + 1);
      hipLaunchKernelGGL(linkage_rank_kernel, node_grid, dim3(256), 0, st, keys_in.p, iota.p, n);
      PG_HIP(ctx, hipGetLastError());
      size_t tb = tmp_bytes;
      PG_HIP(ctx, hipcub::DeviceRadixSort::SortPairs((void*)tmp.p, tb, (const unsigned long long*)keys_in.p, keys_out.p, (const uint32_t*)iota.p, order.p, (int64_t)n, 0, 64, st));
      hipLaunchKernelGGL(representatives_rank_kernel, node_grid, dim3(256), 0, st, (const uint32_t*)order.p, rank.p, n);
      hipLaunchKernelGGL(linkage_best_kernel, node_grid, dim3(256), 0, st, (const int32_t*)S->d_cluster.p, (const uint32_t*)rank.p, n, best.p);
      hipLaunchKernelGGL(linkage_rep_kernel, node_grid, dim3(256), 0, st, (const int32_t*)S->d_cluster.p, (const uint32_t*)best.p, (const uint32_t*)order.p, n, S->d_rep.p);
      PG_HIP(ctx, hipGetLastError());
    }
    PG_HIP(ctx, hipMemcpyAsync(&n_clusters, count.p + 1, 8, hipMemcpyDeviceToHost, st));
    PG_HIP(ctx, hipStreamSynchronize(st));
    if (n_clusters < n_comp || n_clusters > n)
      return pg_fail(ctx, PG_E_INTERNAL, "screen: " + std::to_string(n_clusters) + " clusters of " + std::to_string(n_comp) + " components and " + std::to_string(n) + " nodes");
    return PG_OK;
  };
  const int rc = run();
  if (rc) { (void)hipStreamSynchronize(st); return rc; }      // the rule of band_loop: a queued copy may still read the caller's arrays
  pg_screen_linkage_drop(ctx);
  PgScreenLinkageStats& L = ctx->screen_linkage_stats;
  L.nodes = n; L.worked = m - ignored; L.ignored = ignored; L.components = n_comp; L.worked_components = P.w_size.size(); L.largest = P.largest; L.clusters = n_clusters;
  L.batches = P.batches.size();
  L.group_ms = T.ms(ST_GROUP); L.fill_ms = T.ms(ST_FILL); L.small_ms = T.ms(ST_SMALL); L.large_ms = T.ms(ST_LARGE); L.cut_ms = T.ms(ST_CUT);
  ctx->screen_linkage_state = S.release();
  *n_clusters_out = (uint32_t)n_clusters;
  return PG_OK;
}
