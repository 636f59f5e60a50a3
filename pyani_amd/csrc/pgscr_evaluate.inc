// pgscr_evaluate.inc — part of pg_screen.hip: the EVALUATION of a partition of the kept pairs (DESIGN.md §16.12).  Given the list of entries
// the representatives read and a partition `label` (label[label[v]] == label[v]), every DISTINCT pair {u, v} — its weight the maximum over
// its entries — is inside (label[u] == label[v]) or outside, and the pairs are reduced per node and per cluster: centrality sums, the
// weakest inside pair, the medoid, the nearest outside node and the nearest other cluster.  Kernel boundaries are the only ordering, no
// thread waits for another, every store goes through vector memory.
//   E1 evaluate_keys_kernel      list path: key[e] = min(a, b) << 20 | max(a, b) (40 bits), a self entry the sentinel 2^40 - 1 that sorts
//                                last; one hipcub radix sort over exactly those bits and one reduce-by-key with maximum give the distinct
//                                pairs in ascending (lo, hi).  The index path's list (representatives_collect) is distinct already.
//   P1 representatives_keys_kernel, P2 representatives_rank_kernel: the ranks, from the representatives' one stable sort of (~score, index)
//   E2 evaluate_init_kernel      the identities of the minima and maxima
//   E3 evaluate_pair_kernel      pair pass: per pair four destinations — the node lo, the node hi, the cluster label[lo] and (outside pairs)
//                                the cluster label[hi].  For each, a run of equal destination in consecutive lanes is reduced inside the
//                                wave by a segmented shuffle (evaluate_flush) before ONE set of atomics from the run's head: after the sort
//                                equal lo, and so equal label[lo], are adjacent — a star's hub or one huge cluster costs one set per wave.
//                                Outside pairs: a 64-bit atomic maximum of w << 32 | ~other per node and w << 32 | ~label[other] per
//                                cluster; ~other is never 0 (other < 2^20), so a key of 0 is "no pair" and a weight of 0 stays a pair.
//   E4 evaluate_size_kernel      node pass: size[label[v]] += 1 and best[label[v]] = max(in_weight[v]), runs of equal label reduced first
//   E5 evaluate_medoid_kernel    node pass: the members that reach best: best_rank[label[v]] = min(rank[v]) — two steps, because in_weight
//                                (52 bits) and a rank do not fit one 64-bit key
//   E6 evaluate_finish_kernel    node pass: the keys unpacked, medoid = order[best_rank]; 0 / -1 where a node names no cluster; the clusters
//                                and the inside pairs counted, one atomic per wave
//   E7 evaluate_medoid_pair_kernel  a last pair pass: to_medoid — a pair is distinct, so every word has one writer
namespace {

struct EvaluateState {      // the resident result of the latest accepted evaluate call
  uint32_t n = 0;
  PgDevBuf<uint32_t> in_pairs, in_min, out_pairs, out_weight, to_medoid;      // n each
  PgDevBuf<unsigned long long> in_weight;
  PgDevBuf<int32_t> out_node;
  PgDevBuf<uint32_t> c_size, c_min, c_near_weight;
  PgDevBuf<unsigned long long> c_pairs, c_weight;
  PgDevBuf<int32_t> c_medoid, c_near_cluster;
};

EvaluateState* evaluate_of(pg_ctx* ctx) { return static_cast<EvaluateState*>(ctx->screen_evaluate_state); }

constexpr unsigned long long EVAL_SELF = (1ull << 40) - 1ull;      // lo == hi == 2^20 - 1: no pair's key (lo < hi)
constexpr uint32_t EVAL_NONE = 0xFFFFFFFFu;

struct EvaluateWork {      // what one call needs beside the entries; released when it returns
  PgDevBuf<unsigned long long> keys_in, keys_out;      // the pairs' keys; after the reduce keys_in holds the distinct ones
  PgDevBuf<uint32_t> vals_in, vals_out;
  PgDevBuf<unsigned long long> score_in, score_out, out_key, near_key, best, count;      // count: runs, clusters, inside pairs
  PgDevBuf<uint32_t> iota, order, rank, best_rank;
  PgDevBuf<int32_t> label;
  PgDevBuf<uint8_t> tmp;
  size_t tmp_bytes = 0;
};

__global__ __launch_bounds__(256) void evaluate_keys_kernel(const int32_t* __restrict__ a, const int32_t* __restrict__ b, const uint32_t* __restrict__ w, uint64_t m, uint32_t n,
                                                             unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t ua = (uint32_t)a[e], ub = (uint32_t)b[e];
    const uint32_t lo = ua < ub ? ua : ub, hi = ua < ub ? ub : ua;
    keys[e] = (lo == hi || hi >= n) ? EVAL_SELF : ((unsigned long long)lo << 20) | hi;      // (hi < n: the host checked; kept for the memory's sake)
    vals[e] = w ? w[e] : 1u;
  }
}

__global__ __launch_bounds__(256) void evaluate_init_kernel(uint32_t n, uint32_t* __restrict__ in_min, unsigned long long* __restrict__ out_key, uint32_t* __restrict__ to_medoid,
                                                             uint32_t* __restrict__ c_size, unsigned long long* __restrict__ c_pairs, unsigned long long* __restrict__ c_weight,
                                                             uint32_t* __restrict__ c_min, unsigned long long* __restrict__ near_key, unsigned long long* __restrict__ best,
                                                             uint32_t* __restrict__ best_rank) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
    in_min[v] = EVAL_NONE; out_key[v] = 0ull; to_medoid[v] = 0u;
    c_size[v] = 0u; c_pairs[v] = 0ull; c_weight[v] = 0ull; c_min[v] = EVAL_NONE; near_key[v] = 0ull; best[v] = 0ull; best_rank[v] = EVAL_NONE;
  }
}

// The run of equal `dest` in consecutive lanes that a lane belongs to, numbered from 1 along the wave, and whether the lane is its head.
__device__ __forceinline__ uint32_t evaluate_segment(uint32_t dest, uint32_t lane, bool& head) {
  const uint32_t prev = __shfl_up(dest, 1, 64);
  head = lane == 0u || dest != prev;
  const unsigned long long heads = __ballot(head);
  return (uint32_t)__popcll(heads & ((2ull << lane) - 1ull));      // (lane 63: 2 << 63 wraps to 0, minus one = every bit)
}

// One destination's share of 64 pairs: inside count, weight sum and minimum, outside count and the greatest outside key, reduced over the
// run of equal dest (every lane of the wave calls this) and added by the run's head.  out_cnt may be null (a cluster counts no outside
// pairs).  Count: uint32 per node, 64-bit per cluster.
template <typename Count>
__device__ __forceinline__ void evaluate_flush(uint32_t dest, uint32_t lane, uint32_t cnt_in, unsigned long long sum_in, uint32_t min_in, uint32_t cnt_out, unsigned long long key_out,
                                               Count* in_cnt, unsigned long long* in_sum, uint32_t* in_min, uint32_t* out_cnt, unsigned long long* out_key) {
  bool head;
  const uint32_t run = evaluate_segment(dest, lane, head);
  for (uint32_t d = 1; d < 64u; d <<= 1) {
    const uint32_t r2 = __shfl_down(run, d, 64);
    const uint32_t ci2 = __shfl_down(cnt_in, d, 64), mi2 = __shfl_down(min_in, d, 64), co2 = __shfl_down(cnt_out, d, 64);
    const unsigned long long s2 = __shfl_down(sum_in, d, 64), k2 = __shfl_down(key_out, d, 64);
    if (lane + d < 64u && r2 == run) {
      cnt_in += ci2; sum_in += s2; cnt_out += co2;
      if (mi2 < min_in) min_in = mi2;
      if (k2 > key_out) key_out = k2;
    }
  }
  if (!head || dest == EVAL_NONE) return;
  if (cnt_in) {      // no return values
    atomicAdd(in_cnt + dest, (Count)cnt_in);
    atomicAdd(in_sum + dest, sum_in);
    atomicMin(in_min + dest, min_in);
  }
  if (cnt_out) {
    if (out_cnt) atomicAdd(out_cnt + dest, cnt_out);
    atomicMax(out_key + dest, key_out);
  }
}

// The pair of entry e: from the distinct keys (the list path) or from the index path's list (a < b).  false: none (past the end, the sentinel).
__device__ __forceinline__ bool evaluate_pair(const unsigned long long* __restrict__ keys, const int32_t* __restrict__ a, const int32_t* __restrict__ b, uint64_t e, uint64_t P,
                                              uint32_t n, uint32_t& lo, uint32_t& hi) {
  if (e >= P) return false;
  if (keys) {
    const unsigned long long k = keys[e];
    lo = (uint32_t)(k >> 20); hi = (uint32_t)(k & 0xFFFFFull);
    return k < EVAL_SELF && lo < hi && hi < n;
  }
  const uint32_t ua = (uint32_t)a[e], ub = (uint32_t)b[e];
  lo = ua < ub ? ua : ub; hi = ua < ub ? ub : ua;
  return lo < hi && hi < n;
}

__global__ __launch_bounds__(256) void evaluate_pair_kernel(const unsigned long long* __restrict__ keys, const int32_t* __restrict__ a, const int32_t* __restrict__ b,
                                                             const uint32_t* __restrict__ w, uint64_t P, uint32_t n, const int32_t* __restrict__ label, uint32_t* in_pairs,
                                                             unsigned long long* in_weight, uint32_t* in_min, uint32_t* out_pairs, unsigned long long* out_key,
                                                             unsigned long long* c_pairs, unsigned long long* c_weight, uint32_t* c_min, unsigned long long* near_key) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  for (uint64_t base = wave * 64ull; base < P; base += n_waves * 64ull) {      // (uniform over the wave: every lane reaches the shuffles)
    const uint64_t e = base + lane;
    uint32_t lo = 0u, hi = 0u, l_lo = EVAL_NONE, l_hi = EVAL_NONE, wt = 0u;
    const bool live = evaluate_pair(keys, a, b, e, P, n, lo, hi);
    bool inside = false;
    if (live) {
      l_lo = (uint32_t)label[lo]; l_hi = (uint32_t)label[hi]; wt = w[e];
      inside = l_lo == l_hi;
      if (l_lo >= n || l_hi >= n) { l_lo = l_hi = EVAL_NONE; }      // (never: the host checked the labels; kept for the memory's sake)
    }
    const bool ok = live && l_lo != EVAL_NONE;
    const uint32_t ci = ok && inside ? 1u : 0u, co = ok && !inside ? 1u : 0u, mi = ci ? wt : EVAL_NONE;
    const unsigned long long si = ci ? (unsigned long long)wt : 0ull, wk = (unsigned long long)wt << 32;
    evaluate_flush<uint32_t>(ok ? lo : EVAL_NONE, lane, ci, si, mi, co, co ? wk | (unsigned long long)(~hi) : 0ull, in_pairs, in_weight, in_min, out_pairs, out_key);
    evaluate_flush<uint32_t>(ok ? hi : EVAL_NONE, lane, ci, si, mi, co, co ? wk | (unsigned long long)(~lo) : 0ull, in_pairs, in_weight, in_min, out_pairs, out_key);
    evaluate_flush<unsigned long long>(ok ? l_lo : EVAL_NONE, lane, ci, si, mi, co, co ? wk | (unsigned long long)(~l_hi) : 0ull, c_pairs, c_weight, c_min, nullptr, near_key);
    evaluate_flush<unsigned long long>(co ? l_hi : EVAL_NONE, lane, 0u, 0ull, EVAL_NONE, co, co ? wk | (unsigned long long)(~l_lo) : 0ull, c_pairs, c_weight, c_min, nullptr, near_key);
  }
}

__global__ __launch_bounds__(256) void evaluate_size_kernel(uint32_t n, const int32_t* __restrict__ label, const unsigned long long* __restrict__ in_weight, uint32_t* c_size,
                                                             unsigned long long* best) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {      // (uniform over the workgroup)
    const uint32_t v = base + threadIdx.x;
    uint32_t dest = EVAL_NONE, cnt = 0u;
    unsigned long long iw = 0ull;
    if (v < n) {
      dest = (uint32_t)label[v];
      if (dest < n) { cnt = 1u; iw = in_weight[v]; } else dest = EVAL_NONE;
    }
    bool head;
    const uint32_t run = evaluate_segment(dest, lane, head);
    for (uint32_t d = 1; d < 64u; d <<= 1) {
      const uint32_t r2 = __shfl_down(run, d, 64), c2 = __shfl_down(cnt, d, 64);
      const unsigned long long w2 = __shfl_down(iw, d, 64);
      if (lane + d < 64u && r2 == run) { cnt += c2; if (w2 > iw) iw = w2; }
    }
    if (head && dest != EVAL_NONE) {
      atomicAdd(c_size + dest, cnt);
      if (iw) atomicMax(best + dest, iw);
    }
  }
}

__global__ __launch_bounds__(256) void evaluate_medoid_kernel(uint32_t n, const int32_t* __restrict__ label, const unsigned long long* __restrict__ in_weight,
                                                               const unsigned long long* __restrict__ best, const uint32_t* __restrict__ rank, uint32_t* best_rank) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {      // (uniform over the workgroup)
    const uint32_t v = base + threadIdx.x;
    uint32_t dest = EVAL_NONE, rk = EVAL_NONE;
    if (v < n) {
      const uint32_t c = (uint32_t)label[v];
      if (c < n && in_weight[v] == best[c]) { dest = c; rk = rank[v]; }
    }
    bool head;
    const uint32_t run = evaluate_segment(dest, lane, head);
    for (uint32_t d = 1; d < 64u; d <<= 1) {
      const uint32_t r2 = __shfl_down(run, d, 64), k2 = __shfl_down(rk, d, 64);
      if (lane + d < 64u && r2 == run && k2 < rk) rk = k2;
    }
    if (head && dest != EVAL_NONE) atomicMin(best_rank + dest, rk);
  }
}

__global__ __launch_bounds__(256) void evaluate_finish_kernel(uint32_t n, const int32_t* __restrict__ label, const unsigned long long* __restrict__ out_key,
                                                               const unsigned long long* __restrict__ near_key, const uint32_t* __restrict__ best_rank,
                                                               const uint32_t* __restrict__ order, uint32_t* __restrict__ out_weight, int32_t* __restrict__ out_node,
                                                               const unsigned long long* __restrict__ c_pairs, uint32_t* __restrict__ c_min, int32_t* __restrict__ c_medoid,
                                                               uint32_t* __restrict__ c_near_weight, int32_t* __restrict__ c_near_cluster, unsigned long long* count) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {      // (uniform over the workgroup)
    const uint32_t v = base + threadIdx.x;
    bool names = false;
    unsigned long long inside = 0ull;
    if (v < n) {
      const unsigned long long ok = out_key[v];
      out_weight[v] = (uint32_t)(ok >> 32);
      out_node[v] = ok ? (int32_t)~(uint32_t)ok : -1;
      names = (uint32_t)label[v] == v;
      if (names) {
        const unsigned long long nk = near_key[v];
        const uint32_t at = best_rank[v];
        c_medoid[v] = at < n ? (int32_t)order[at] : -1;      // (-1: never — a cluster has a member that reaches its own maximum)
        c_near_weight[v] = (uint32_t)(nk >> 32);
        c_near_cluster[v] = nk ? (int32_t)~(uint32_t)nk : -1;
        inside = c_pairs[v];
      } else {      // size, pairs and weight stayed 0: nothing adds to a node that names no cluster
        c_min[v] = 0u; c_medoid[v] = -1; c_near_weight[v] = 0u; c_near_cluster[v] = -1;
      }
    }
    const unsigned long long naming = __ballot(names);
    for (uint32_t d = 32u; d; d >>= 1) inside += __shfl_down(inside, d, 64);      // (lanes past the wave read their own value: only lane 0's sum is used)
    if (lane == 0u && naming) { atomicAdd(count + 1, (unsigned long long)__popcll(naming)); if (inside) atomicAdd(count + 2, inside); }
  }
}

__global__ __launch_bounds__(256) void evaluate_medoid_pair_kernel(const unsigned long long* __restrict__ keys, const int32_t* __restrict__ a, const int32_t* __restrict__ b,
                                                                    const uint32_t* __restrict__ w, uint64_t P, uint32_t n, const int32_t* __restrict__ label,
                                                                    const int32_t* __restrict__ c_medoid, uint32_t* __restrict__ to_medoid) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < P; e += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t lo, hi;
    if (!evaluate_pair(keys, a, b, e, P, n, lo, hi)) continue;
    const uint32_t c = (uint32_t)label[lo];
    if (c >= n || c != (uint32_t)label[hi]) continue;
    const uint32_t med = (uint32_t)c_medoid[c];
    if (med == lo) to_medoid[hi] = w[e];
    else if (med == hi) to_medoid[lo] = w[e];
  }
}

// What both entry points check of the partition and the scores, before anything is copied or replaced.
int evaluate_check(pg_ctx* ctx, uint32_t n, const int32_t* label, const uint64_t* score) {
  if (n < 1 || n > pgscr::INDEX_MAX_GENOMES) return pg_fail(ctx, PG_E_ARG, "screen: an evaluation is of 1 ... 1048576 (2^20) nodes, not " + std::to_string(n));
  if (!label) return pg_fail(ctx, PG_E_ARG, "screen: the evaluation needs a label for every node");
  if (!score) return pg_fail(ctx, PG_E_ARG, "screen: the evaluation needs a score for every node");
  for (uint32_t v = 0; v < n; ++v) {
    const uint32_t c = (uint32_t)label[v];
    if (c >= n) return pg_fail(ctx, PG_E_ARG, "screen: node " + std::to_string(v) + " has the label " + std::to_string(label[v]) + " outside [0, " + std::to_string(n) + ")");
    if ((uint32_t)label[c] != c)
      return pg_fail(ctx, PG_E_ARG, "screen: node " + std::to_string(v) + " has the label " + std::to_string(c) + ", which does not name itself (label[label[v]] == label[v])");
  }
  return PG_OK;
}

// Everything after the entries stand on the device — (d_a, d_b, d_w) with m entries; distinct = true: a list of distinct pairs a < b with
// weights (the index path), otherwise any list (d_w may be null: every entry weighs 1) — and the finished state made the context's (the
// earlier one goes here, not before).  label and score are the host's.
int evaluate_run(pg_ctx* ctx, uint32_t n, const int32_t* d_a, const int32_t* d_b, const uint32_t* d_w, uint64_t m, bool distinct, const int32_t* label, const uint64_t* score,
                 ScreenEvents& T, uint64_t worked, uint64_t ignored) {
  hipStream_t st = ctx->stream;
  const uint32_t cu_blocks = (uint32_t)ctx->num_cu * 8u;
  const dim3 node_grid(grid_for(n, 256, cu_blocks));
  std::unique_ptr<EvaluateState> R(new EvaluateState());
  EvaluateWork W;
  int rc;
  const bool sorted = !distinct && m;
  PG_HIP(ctx, tmp_room(W.tmp_bytes, [&](size_t& bytes) {
    return hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                              (int64_t)n, 0, 64, st);
  }));
  if (sorted) {
    PG_HIP(ctx, tmp_room(W.tmp_bytes, [&](size_t& bytes) {
      return hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                                (int64_t)m, 0, 40, st);
    }));
    PG_HIP(ctx, tmp_room(W.tmp_bytes, [&](size_t& bytes) {
      return hipcub::DeviceReduce::ReduceByKey(nullptr, bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                               (unsigned long long*)nullptr, hipcub::Max(), (int64_t)m, st);
    }));
  }
  if ((rc = pg_dev_alloc(ctx, "screen", R->in_pairs, n, "the evaluation")) || (rc = pg_dev_alloc(ctx, "screen", R->in_weight, n, "the evaluation")) ||
      (rc = pg_dev_alloc(ctx, "screen", R->in_min, n, "the evaluation")) || (rc = pg_dev_alloc(ctx, "screen", R->out_pairs, n, "the evaluation")) ||
      (rc = pg_dev_alloc(ctx, "screen", R->out_weight, n, "the evaluation")) || (rc = pg_dev_alloc(ctx, "screen", R->out_node, n, "the evaluation")) ||
      (rc = pg_dev_alloc(ctx, "screen", R->to_medoid, n, "the evaluation")) || (rc = pg_dev_alloc(ctx, "screen", R->c_size, n, "the evaluation's clusters")) ||
      (rc = pg_dev_alloc(ctx, "screen", R->c_pairs, n, "the evaluation's clusters")) || (rc = pg_dev_alloc(ctx, "screen", R->c_weight, n, "the evaluation's clusters")) ||
      (rc = pg_dev_alloc(ctx, "screen", R->c_min, n, "the evaluation's clusters")) || (rc = pg_dev_alloc(ctx, "screen", R->c_medoid, n, "the evaluation's clusters")) ||
      (rc = pg_dev_alloc(ctx, "screen", R->c_near_weight, n, "the evaluation's clusters")) ||
      (rc = pg_dev_alloc(ctx, "screen", R->c_near_cluster, n, "the evaluation's clusters")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.score_in, n, "the score keys")) || (rc = pg_dev_alloc(ctx, "screen", W.score_out, n, "the score keys")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.out_key, n, "the outside keys")) || (rc = pg_dev_alloc(ctx, "screen", W.near_key, n, "the clusters' outside keys")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.best, n, "the clusters' maxima")) || (rc = pg_dev_alloc(ctx, "screen", W.best_rank, n, "the clusters' ranks")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.count, 3, "the evaluation's counters")) || (rc = pg_dev_alloc(ctx, "screen", W.iota, n, "the nodes")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.order, n, "the order of the nodes")) || (rc = pg_dev_alloc(ctx, "screen", W.rank, n, "the ranks of the nodes")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.label, n, "the labels")) || (rc = pg_dev_alloc(ctx, "screen", W.tmp, W.tmp_bytes, "the sort's temporary storage")))
    return rc;
  if (sorted && ((rc = pg_dev_alloc(ctx, "screen", W.keys_in, (size_t)m, "the pairs' keys")) || (rc = pg_dev_alloc(ctx, "screen", W.keys_out, (size_t)m, "the pairs' keys")) ||
                 (rc = pg_dev_alloc(ctx, "screen", W.vals_in, (size_t)m, "the pairs' weights")) || (rc = pg_dev_alloc(ctx, "screen", W.vals_out, (size_t)m, "the pairs' weights"))))
    return rc;
  R->n = n;
  PG_HIP(ctx, hipMemcpyAsync(W.score_in, score, (size_t)n * 8, hipMemcpyHostToDevice, st));
  PG_HIP(ctx, hipMemcpyAsync(W.label, label, (size_t)n * 4, hipMemcpyHostToDevice, st));
  PG_HIP(ctx, hipMemsetAsync(W.count, 0, 3 * 8, st));
  // the pairs the passes read: the distinct keys with their weights (list path), or the list as it stands
  const unsigned long long* p_keys = nullptr;
  const uint32_t* p_w = d_w;
  uint64_t P = m;
  {
    ScreenEvents::Stage sort(T, ST_SORT, st);
    // P1 zeroes three node arrays beside the keys: here the two pair counts and the inside sums, which start at 0 as its states do
    hipLaunchKernelGGL(representatives_keys_kernel, node_grid, dim3(256), 0, st, W.score_in.p, W.iota.p, R->in_pairs.p, R->out_pairs.p, R->in_weight.p, n);
    PG_HIP(ctx, hipGetLastError());
    size_t tb = W.tmp_bytes;
    PG_HIP(ctx, hipcub::DeviceRadixSort::SortPairs((void*)W.tmp.p, tb, (const unsigned long long*)W.score_in.p, W.score_out.p, (const uint32_t*)W.iota.p, W.order.p, (int64_t)n, 0, 64, st));
    hipLaunchKernelGGL(representatives_rank_kernel, node_grid, dim3(256), 0, st, (const uint32_t*)W.order.p, W.rank.p, n);
    hipLaunchKernelGGL(evaluate_init_kernel, node_grid, dim3(256), 0, st, n, R->in_min.p, W.out_key.p, R->to_medoid.p, R->c_size.p, R->c_pairs.p, R->c_weight.p, R->c_min.p,
                       W.near_key.p, W.best.p, W.best_rank.p);
    PG_HIP(ctx, hipGetLastError());
    if (sorted) {
      hipLaunchKernelGGL(evaluate_keys_kernel, dim3(grid_for(m, 256 * 4, cu_blocks)), dim3(256), 0, st, d_a, d_b, d_w, m, n, W.keys_in.p, W.vals_in.p);
      PG_HIP(ctx, hipGetLastError());
      tb = W.tmp_bytes;
      PG_HIP(ctx, hipcub::DeviceRadixSort::SortPairs((void*)W.tmp.p, tb, (const unsigned long long*)W.keys_in.p, W.keys_out.p, (const uint32_t*)W.vals_in.p, W.vals_out.p, (int64_t)m, 0, 40, st));
      tb = W.tmp_bytes;      // (the sort's inputs are dead: the distinct keys and their maxima take their place)
      PG_HIP(ctx, hipcub::DeviceReduce::ReduceByKey((void*)W.tmp.p, tb, (const unsigned long long*)W.keys_out.p, W.keys_in.p, (const uint32_t*)W.vals_out.p, W.vals_in.p, W.count.p,
                                                    hipcub::Max(), (int64_t)m, st));
    }
  }
  if (sorted) {
    unsigned long long runs = 0;
    PG_HIP(ctx, hipMemcpyAsync(&runs, W.count, 8, hipMemcpyDeviceToHost, st));
    PG_HIP(ctx, hipStreamSynchronize(st));
    if (runs < 1 || runs > m) return pg_fail(ctx, PG_E_INTERNAL, "screen: " + std::to_string(runs) + " distinct keys of " + std::to_string(m) + " entries");
    P = runs - (ignored ? 1u : 0u);      // (the self entries are ONE run, the last)
    p_keys = W.keys_in.p; p_w = W.vals_in.p;
  }
  const dim3 pair_grid(grid_for(P, 256 * 4, cu_blocks));
  {
    ScreenEvents::Stage pairs(T, ST_FILL, st);
    if (P) hipLaunchKernelGGL(evaluate_pair_kernel, pair_grid, dim3(256), 0, st, p_keys, d_a, d_b, p_w, P, n, (const int32_t*)W.label.p, R->in_pairs.p, R->in_weight.p, R->in_min.p,
                              R->out_pairs.p, W.out_key.p, R->c_pairs.p, R->c_weight.p, R->c_min.p, W.near_key.p);
    PG_HIP(ctx, hipGetLastError());
  }
  {
    ScreenEvents::Stage nodes(T, ST_STATS, st);
    hipLaunchKernelGGL(evaluate_size_kernel, node_grid, dim3(256), 0, st, n, (const int32_t*)W.label.p, (const unsigned long long*)R->in_weight.p, R->c_size.p, W.best.p);
    hipLaunchKernelGGL(evaluate_medoid_kernel, node_grid, dim3(256), 0, st, n, (const int32_t*)W.label.p, (const unsigned long long*)R->in_weight.p,
                       (const unsigned long long*)W.best.p, (const uint32_t*)W.rank.p, W.best_rank.p);
    hipLaunchKernelGGL(evaluate_finish_kernel, node_grid, dim3(256), 0, st, n, (const int32_t*)W.label.p, (const unsigned long long*)W.out_key.p,
                       (const unsigned long long*)W.near_key.p, (const uint32_t*)W.best_rank.p, (const uint32_t*)W.order.p, R->out_weight.p, R->out_node.p,
                       (const unsigned long long*)R->c_pairs.p, R->c_min.p, R->c_medoid.p, R->c_near_weight.p, R->c_near_cluster.p, W.count.p);
    PG_HIP(ctx, hipGetLastError());
  }
  {
    ScreenEvents::Stage pairs(T, ST_FILL, st);
    if (P) hipLaunchKernelGGL(evaluate_medoid_pair_kernel, pair_grid, dim3(256), 0, st, p_keys, d_a, d_b, p_w, P, n, (const int32_t*)W.label.p, (const int32_t*)R->c_medoid.p,
                              R->to_medoid.p);
    PG_HIP(ctx, hipGetLastError());
  }
  unsigned long long count[3] = {};
  PG_HIP(ctx, hipMemcpyAsync(count, W.count, 3 * 8, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipStreamSynchronize(st));
  if (count[1] < 1 || count[1] > n || count[2] > P) return pg_fail(ctx, PG_E_INTERNAL, "screen: " + std::to_string(count[1]) + " clusters of " + std::to_string(n) + " nodes");
  pg_screen_evaluate_drop(ctx);
  PgScreenEvaluateStats& L = ctx->screen_evaluate_stats;
  L.nodes = n; L.worked = worked; L.ignored = ignored; L.pairs = P; L.inside = count[2]; L.clusters = count[1];
  L.select_ms = T.ms(ST_SELECT); L.sort_ms = T.ms(ST_SORT); L.pair_ms = T.ms(ST_FILL); L.node_ms = T.ms(ST_STATS);
  ctx->screen_evaluate_state = R.release();
  return PG_OK;
}

}  // namespace

void pg_screen_evaluate_drop(pg_ctx* ctx) {
  if (!ctx->screen_evaluate_state) return;
  delete evaluate_of(ctx);
  ctx->screen_evaluate_state = nullptr;
  ctx->screen_evaluate_stats = PgScreenEvaluateStats{};
}

extern "C" int pg_screen_evaluate_release(pg_ctx* ctx) {
  if (!ctx) return PG_E_ARG;
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  pg_screen_evaluate_drop(ctx);
  return PG_OK;
}

extern "C" int pg_screen_evaluate_last(pg_ctx* ctx, uint64_t* counts_out, double* ms_out) {
  if (!ctx || !counts_out || !ms_out) return pg_fail(ctx, PG_E_ARG, "bad argument");
  const PgScreenEvaluateStats& L = ctx->screen_evaluate_stats;
  counts_out[0] = L.nodes; counts_out[1] = L.worked; counts_out[2] = L.ignored; counts_out[3] = L.pairs; counts_out[4] = L.inside; counts_out[5] = L.clusters;
  ms_out[0] = L.select_ms; ms_out[1] = L.sort_ms; ms_out[2] = L.pair_ms; ms_out[3] = L.node_ms;
  return PG_OK;
}

namespace {
template <typename T, typename D>
int evaluate_copy(pg_ctx* ctx, T* out, const PgDevBuf<D>& src, uint32_t n) {
  static_assert(sizeof(T) == sizeof(D), "the same words on both sides");
  if (out) PG_HIP(ctx, hipMemcpyAsync(out, src.p, (size_t)n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
  return PG_OK;
}
}  // namespace

extern "C" int pg_screen_evaluate_read(pg_ctx* ctx, uint32_t* in_pairs_out, uint64_t* in_weight_out, uint32_t* in_min_out, uint32_t* out_pairs_out, uint32_t* out_weight_out,
                                       int32_t* out_node_out, uint32_t* to_medoid_out) {
  if (!ctx) return PG_E_ARG;
  EvaluateState* R = evaluate_of(ctx);
  if (!R) return pg_fail(ctx, PG_E_ARG, "screen: no resident evaluation (call pg_screen_evaluate or pg_screen_index_evaluate first)");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  int rc;
  if ((rc = evaluate_copy(ctx, in_pairs_out, R->in_pairs, R->n)) || (rc = evaluate_copy(ctx, in_weight_out, R->in_weight, R->n)) ||
      (rc = evaluate_copy(ctx, in_min_out, R->in_min, R->n)) || (rc = evaluate_copy(ctx, out_pairs_out, R->out_pairs, R->n)) ||
      (rc = evaluate_copy(ctx, out_weight_out, R->out_weight, R->n)) || (rc = evaluate_copy(ctx, out_node_out, R->out_node, R->n)) ||
      (rc = evaluate_copy(ctx, to_medoid_out, R->to_medoid, R->n))) {
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
  }
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PG_OK;
}

extern "C" int pg_screen_evaluate_read_clusters(pg_ctx* ctx, uint32_t* size_out, uint64_t* pairs_out, uint64_t* weight_out, uint32_t* min_out, int32_t* medoid_out,
                                                uint32_t* near_weight_out, int32_t* near_cluster_out) {
  if (!ctx) return PG_E_ARG;
  EvaluateState* R = evaluate_of(ctx);
  if (!R) return pg_fail(ctx, PG_E_ARG, "screen: no resident evaluation (call pg_screen_evaluate or pg_screen_index_evaluate first)");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  int rc;
  if ((rc = evaluate_copy(ctx, size_out, R->c_size, R->n)) || (rc = evaluate_copy(ctx, pairs_out, R->c_pairs, R->n)) ||
      (rc = evaluate_copy(ctx, weight_out, R->c_weight, R->n)) || (rc = evaluate_copy(ctx, min_out, R->c_min, R->n)) ||
      (rc = evaluate_copy(ctx, medoid_out, R->c_medoid, R->n)) || (rc = evaluate_copy(ctx, near_weight_out, R->c_near_weight, R->n)) ||
      (rc = evaluate_copy(ctx, near_cluster_out, R->c_near_cluster, R->n))) {
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
  }
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PG_OK;
}

extern "C" int pg_screen_evaluate(pg_ctx* ctx, const int32_t* a, const int32_t* b, const uint32_t* weight, uint64_t m, uint32_t n, const int32_t* label, const uint64_t* score) {
  if (!ctx) return PG_E_ARG;
  int rc;
  if ((rc = evaluate_check(ctx, n, label, score))) return rc;
  if (m > 0xFFFFFFFFull) return pg_fail(ctx, PG_E_ARG, "screen: an evaluation is of at most 4294967295 (2^32 - 1) entries, not " + std::to_string(m));
  if (m && (!a || !b)) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  uint64_t ignored = 0;
  uint32_t outside = 0;
  for (uint64_t i = 0; i < m; ++i) {      // before anything is copied or replaced (one branch-free pass; a negative index is a large unsigned one)
    outside |= (uint32_t)((uint32_t)a[i] >= n) | (uint32_t)((uint32_t)b[i] >= n);
    ignored += a[i] == b[i] ? 1u : 0u;
  }
  for (uint64_t i = 0; outside && i < m; ++i)
    if ((uint32_t)a[i] >= n || (uint32_t)b[i] >= n)
      return pg_fail(ctx, PG_E_ARG, "screen: entry " + std::to_string(i) + " names node " + std::to_string((uint32_t)a[i] >= n ? a[i] : b[i]) + " outside [0, " +
                                        std::to_string(n) + ")");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  PgDevBuf<int32_t> d_a, d_b;
  PgDevBuf<uint32_t> d_w;
  if ((rc = pg_dev_alloc(ctx, "screen", d_a, (size_t)m, "the entries")) || (rc = pg_dev_alloc(ctx, "screen", d_b, (size_t)m, "the entries")) ||
      (weight && (rc = pg_dev_alloc(ctx, "screen", d_w, (size_t)m, "the entries' weights"))))
    return rc;
  const auto run = [&]() -> int {
    if (m) {
      PG_HIP(ctx, hipMemcpyAsync(d_a, a, (size_t)m * 4, hipMemcpyHostToDevice, st));
      PG_HIP(ctx, hipMemcpyAsync(d_b, b, (size_t)m * 4, hipMemcpyHostToDevice, st));
      if (weight) PG_HIP(ctx, hipMemcpyAsync(d_w, weight, (size_t)m * 4, hipMemcpyHostToDevice, st));
    }
    ScreenEvents T;
    return evaluate_run(ctx, n, d_a.p, d_b.p, weight ? d_w.p : nullptr, m, false, label, score, T, m - ignored, ignored);
  };
  rc = run();
  if (rc) (void)hipStreamSynchronize(st);      // the rule of band_loop: a queued copy may still read the caller's arrays
  return rc;
}

extern "C" int pg_screen_index_evaluate(pg_ctx* ctx, const uint32_t* need, uint32_t n, const int32_t* label, const uint64_t* score, uint64_t* n_pairs_out) {
  if (!ctx) return PG_E_ARG;
  IndexState* I = nullptr;
  int rc;
  if ((rc = band_check(ctx, need, n, 1, n_pairs_out != nullptr, &I))) return rc;
  if ((rc = evaluate_check(ctx, n, label, score))) return rc;
  PG_HIP(ctx, hipSetDevice(ctx->device));
  KeptList L;
  ScreenEvents T;
  BandTotals tot;
  if ((rc = representatives_collect(ctx, I, need, T, L, tot))) return rc;
  if ((rc = evaluate_run(ctx, n, L.a.p, L.b.p, L.w.p, L.held, true, label, score, T, L.held, 0))) { (void)hipStreamSynchronize(ctx->stream); return rc; }
  *n_pairs_out = tot.kept;
  return PG_OK;
}
