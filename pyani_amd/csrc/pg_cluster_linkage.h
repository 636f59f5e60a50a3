// pg_cluster_linkage.h — scipy's nearest-neighbour chain for "complete" and "average" on a prepared symmetric working matrix: K2 of
// pg_cluster.hip (its header has the description), shared with the screen's linkage of the kept pairs (pgscr_linkage.inc, DESIGN.md
// §16.11).  Included INSIDE the unnamed namespace of each of the two translation units: every one has its own copy of the kernel.
// Contract: results EQUAL scipy's bit for bit; the build line forbids contraction.

constexpr uint32_t CLU_MAX_N = 8192;      // observations: sizes + chain in LDS (64 KiB at the limit), 512 MiB working matrix

struct ClusterProblem {      // one linkage problem on the device
  double* work;              // n x n symmetric working matrix
  double* merges;            // (n - 1) x 4
  const int* flag;           // != 0: a distance was not finite, the problem is skipped
  uint32_t n;
  int32_t method;
};

struct ValIdx {
  double v;
  uint32_t i;
};

__device__ __forceinline__ bool clu_better(double v, uint32_t i, double bv, uint32_t bi) { return v < bv || (v == bv && i < bi); }

__global__ __launch_bounds__(1024) void cluster_linkage_kernel(const ClusterProblem* __restrict__ problems) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const ClusterProblem P = problems[blockIdx.x];
  if (*P.flag != 0) return;      // uniform: the whole workgroup leaves
  const uint32_t n = P.n, tid = threadIdx.x, nt = blockDim.x, lane = tid & 63u, wave = tid >> 6, n_waves = nt >> 6;
  double* D = P.work;      // read and written: no __restrict__
  ValIdx* red = reinterpret_cast<ValIdx*>(smem);                 // [2][16]
  uint32_t* size = reinterpret_cast<uint32_t*>(smem + 2 * 16 * sizeof(ValIdx));
  uint32_t* chain = size + n;
  const double INF = __builtin_huge_val();

  for (uint32_t i = tid; i < n; i += nt) size[i] = 1u;
  __syncthreads();

  uint32_t len = 0, first_live = 0, par = 0;
  uint32_t x = 0, prev = 0;      // the chain's tip and the element under it (valid for len >= 1 / len >= 2)
  double cur = INF;              // D[x, prev], or +inf for a chain of one
  for (uint32_t merge = 0; merge + 1 < n; ++merge) {
    if (len == 0) {
      while (size[first_live] == 0u) ++first_live;      // lowest live index never decreases; uniform
      x = first_live;
      if (tid == 0) chain[0] = x;
      len = 1;
      cur = INF;
    }
    for (;;) {
      // row argmin over the live clusters other than x: ascending scan, strict <, so the lowest index attaining the minimum
      double bv = INF;
      uint32_t bi = 0xFFFFFFFFu;
      const double* row = D + (size_t)x * n;
      for (uint32_t i = tid; i < n; i += nt) {
        if (i == x || size[i] == 0u) continue;
        const double v = row[i];
        if (v < bv) { bv = v; bi = i; }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(bv, off, 64);
        const uint32_t oi = __shfl_xor(bi, off, 64);
        if (clu_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
      }
      if (lane == 0) { red[par * 16 + wave].v = bv; red[par * 16 + wave].i = bi; }
      __syncthreads();
      bv = red[par * 16].v;
      bi = red[par * 16].i;
      for (uint32_t w = 1; w < n_waves; ++w) {
        const double ov = red[par * 16 + w].v;
        const uint32_t oi = red[par * 16 + w].i;
        if (clu_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
      }
      par ^= 1u;      // the other pair of slots next time: one barrier per chain step
      uint32_t y = prev;
      if (bv < cur) { cur = bv; y = bi; }
      if (len > 1 && y == prev) break;
      if (tid == 0) chain[len] = y;
      ++len;
      prev = x;
      x = y;
    }
    // merge the tip and the element under it
    len -= 2;
    const uint32_t lo = x < prev ? x : prev, hi = x < prev ? prev : x;
    const uint32_t nlo = size[lo], nhi = size[hi];
    if (tid == 0) {
      double* rec = P.merges + (size_t)merge * 4;
      rec[0] = (double)lo;
      rec[1] = (double)hi;
      rec[2] = cur;
      rec[3] = (double)(nlo + nhi);
    }
    const double flo = (double)nlo, fhi = (double)nhi, fsum = (double)(nlo + nhi);
    const double* rlo = D + (size_t)lo * n;
    double* rhi = D + (size_t)hi * n;
    for (uint32_t i = tid; i < n; i += nt) {
      if (i == lo || i == hi || size[i] == 0u) continue;
      const double a = rlo[i], b = rhi[i];
      double v;
      if (P.method == PG_CLUSTER_AVERAGE) {
        const double pa = flo * a, pb = fhi * b;
        v = (pa + pb) / fsum;
      } else {
        v = a > b ? a : b;
      }
      rhi[i] = v;
      D[(size_t)i * n + hi] = v;
    }
    __syncthreads();      // every size[] read and every update of this merge is done
    if (tid == 0) { size[lo] = 0u; size[hi] = nlo + nhi; }
    if (len >= 1) {       // chain[] below len was written before earlier barriers
      x = chain[len - 1];
      if (len >= 2) { prev = chain[len - 2]; cur = D[(size_t)x * n + prev]; }
      else cur = INF;
    }
    __syncthreads();
  }
}

// the launch shape of K2 for problems of at most n_max observations
inline uint32_t clu_linkage_threads(uint32_t n_max) { return std::min<uint32_t>(1024u, std::max<uint32_t>(64u, (n_max + 63u) & ~63u)); }
inline size_t clu_linkage_lds(uint32_t n_max) { return 2 * 16 * sizeof(ValIdx) + (size_t)2 * n_max * sizeof(uint32_t); }
