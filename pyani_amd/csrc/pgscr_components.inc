// pgscr_components.inc — part of pg_screen.hip: the connected components of the kept pairs (DESIGN.md §16.3).
// A union-find forest over the n nodes in ONE array, parent[v] <= v, a root being its own parent.  Only atomics write it: the hook is a
// compare-and-swap on a root's own cell, the path halving an atomic minimum.  So a cell only ever DECREASES, a cell that has left its own
// index never returns to it, and every value a cell has held is a smaller node of the same tree.  Every plain or stale read of the array is
// therefore harmless — it names a node of the right tree, no larger than the one it was read for — and what is decided rests on the value
// a compare-and-swap returned.  No thread waits for another: every loop below walks a strictly decreasing node index (§16.3 has the argument).
//   K1 components_init_kernel     parent[v] = v, entries = weight = 0
//   K2 components_hook_kernel     one pass over a list (a chunk of the host's, or a band's kept triples): accumulate — a run of equal a
//                                 inside a wave is summed by a segmented shuffle reduction and adds ONCE to entries[a] and weight[a], 64-bit
//                                 atomics without return value — and hook: both roots found, the larger hooked under the smaller; its
//                                 body, components_hook_entry, is the sweep's bucket pass as well (pgscr_sweep.inc)
//   K3 components_flatten_kernel  root[v] = the root of v's tree (halving as it goes); the roots counted, one atomic per wave
namespace {

struct ComponentsState {      // the resident result of the latest accepted components call
  uint32_t n = 0;
  PgDevBuf<uint32_t> d_parent;                      // n: the forest
  PgDevBuf<int32_t> d_root;                         // n: flattened
  PgDevBuf<unsigned long long> d_entries, d_weight; // n each
  PgDevBuf<unsigned long long> d_count;             // [0] the roots
};

ComponentsState* components_of(pg_ctx* ctx) { return static_cast<ComponentsState*>(ctx->screen_components_state); }

constexpr uint64_t COMPONENTS_CHUNK = 1ull << 24;      // host entries uploaded at a time: 192 MB of device memory whatever m is

__global__ __launch_bounds__(256) void components_init_kernel(uint32_t* __restrict__ parent, unsigned long long* __restrict__ entries,
                                                               unsigned long long* __restrict__ weight, uint32_t n) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) { parent[v] = v; entries[v] = 0ull; weight[v] = 0ull; }
}

__device__ __forceinline__ uint32_t components_peek(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// A root-looking node of u's tree, no larger than u (u < n): u moves to a strictly smaller node every round, so at most u rounds.  What it
// returns may have been hooked since — the caller's compare-and-swap finds that out.
__device__ __forceinline__ uint32_t components_find(uint32_t* parent, uint32_t u) {
  for (;;) {
    const uint32_t p = components_peek(parent + u);
    if (p >= u) return u;                      // (p == u: a root as far as this read knows; p > u never happens, and would not be followed)
    const uint32_t g = components_peek(parent + p);
    if (g >= p) return p;
    atomicMin(parent + u, g);                  // halving: g < p < u is a node of u's tree; no return value
    u = g;
  }
}

// The hook alone: the trees of ua and ub (both < n, ua != ub) joined, the larger root under the smaller.  Returns whether THIS call's
// compare-and-swap hooked a root.  The linkage's two forests (pgscr_linkage.inc) hook through it as well.
__device__ __forceinline__ bool components_hook_nodes(uint32_t* parent, uint32_t ua, uint32_t ub) {
  uint32_t u = components_find(parent, ua), v = components_find(parent, ub);
  while (u != v) {      // u in a's tree, v in b's; max(u, v) drops with every failed round
    if (u < v) { const uint32_t t = u; u = v; v = t; }
    const uint32_t old = atomicCAS(parent + u, u, v);
    if (old == u) return true;      // u was a root and now hangs under v < u
    if (old > u) break;       // (never: a cell only decreases; kept so that a broken array cannot spin)
    u = components_find(parent, old);      // old < u: u's parent when the swap looked; on from its tree's top
  }
  return false;
}

// The accumulate and the hook of ONE entry per lane — the body of K2, and of the sweep's bucket pass (pgscr_sweep.inc).  Every lane of the
// wave calls it (the shuffles); in = the lane holds an entry e, (ua, ub) its nodes (0xFFFFFFFF both where it holds none).  Returns whether
// THIS lane's compare-and-swap hooked a root: each success takes one tree away, so the successes of a list are n - its components.
__device__ __forceinline__ bool components_hook_entry(uint32_t lane, bool in, uint32_t ua, uint32_t ub, const uint32_t* __restrict__ s, uint64_t e, uint32_t n,
                                                      uint32_t* parent, unsigned long long* __restrict__ entries, unsigned long long* __restrict__ weight) {
  const bool work = in && ua != ub && ua < n && ub < n;      // (the host has refused an index outside [0, n): the bound is kept for the memory's sake)
  unsigned long long cnt = work ? 1ull : 0ull, w = work ? (s ? (unsigned long long)s[e] : 1ull) : 0ull;
  // accumulate: runs of equal a in consecutive lanes; run = the number of run heads up to this lane, so equal run numbers are one run
  const uint32_t prev = __shfl_up(ua, 1, 64);
  const bool head = lane == 0u || ua != prev;
  const unsigned long long heads = __ballot(head);
  const uint32_t run = (uint32_t)__popcll(heads & ((2ull << lane) - 1ull));      // (lane 63: 2 << 63 wraps to 0, minus one = every bit)
  for (uint32_t d = 1; d < 64u; d <<= 1) {
    const uint32_t r2 = __shfl_down(run, d, 64);
    const unsigned long long c2 = __shfl_down(cnt, d, 64), w2 = __shfl_down(w, d, 64);
    if (lane + d < 64u && r2 == run) { cnt += c2; w += w2; }
  }
  if (head && cnt) { atomicAdd(entries + ua, cnt); atomicAdd(weight + ua, w); }
  return work && components_hook_nodes(parent, ua, ub);
}

__global__ __launch_bounds__(256) void components_hook_kernel(const int32_t* __restrict__ a, const int32_t* __restrict__ b, const uint32_t* __restrict__ s,
                                                               uint64_t m, uint32_t n, uint32_t* parent, unsigned long long* __restrict__ entries,
                                                               unsigned long long* __restrict__ weight) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  for (uint64_t base = wave * 64ull; base < m; base += n_waves * 64ull) {      // (uniform over the wave: every lane reaches the shuffles)
    const uint64_t e = base + lane;
    const bool in = e < m;
    const uint32_t ua = in ? (uint32_t)a[e] : 0xFFFFFFFFu, ub = in ? (uint32_t)b[e] : 0xFFFFFFFFu;
    (void)components_hook_entry(lane, in, ua, ub, s, e, n, parent, entries, weight);
  }
}

__global__ __launch_bounds__(256) void components_flatten_kernel(uint32_t* parent, uint32_t n, int32_t* __restrict__ root, unsigned long long* __restrict__ count) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {      // (uniform over the workgroup)
    const uint32_t v = base + threadIdx.x;
    bool is_root = false;
    if (v < n) {
      const uint32_t r = components_find(parent, v);      // (no hook runs beside this kernel: what looks like a root is one)
      root[v] = (int32_t)r;
      is_root = r == v;
    }
    const unsigned long long roots = __ballot(is_root);
    if (lane == 0u && roots) atomicAdd(count, (unsigned long long)__popcll(roots));
  }
}

int components_alloc(pg_ctx* ctx, uint32_t n, ComponentsState& C) {
  int rc;
  if ((rc = pg_dev_alloc(ctx, "screen", C.d_parent, n, "the components' forest")) || (rc = pg_dev_alloc(ctx, "screen", C.d_root, n, "the components' roots")) ||
      (rc = pg_dev_alloc(ctx, "screen", C.d_entries, n, "the components' entry counts")) || (rc = pg_dev_alloc(ctx, "screen", C.d_weight, n, "the components' weights")) ||
      (rc = pg_dev_alloc(ctx, "screen", C.d_count, 1, "the components' counter")))
    return rc;
  C.n = n;
  hipLaunchKernelGGL(components_init_kernel, dim3(grid_for(n, 256, (uint32_t)ctx->num_cu * 8u)), dim3(256), 0, ctx->stream, C.d_parent.p, C.d_entries.p, C.d_weight.p, n);
  PG_HIP(ctx, hipGetLastError());
  PG_HIP(ctx, hipMemsetAsync(C.d_count, 0, 8, ctx->stream));
  return PG_OK;
}

// K2 over m triples that stand on the device (s may be null: every entry counts 1)
int components_hook(pg_ctx* ctx, ComponentsState& C, const int32_t* d_a, const int32_t* d_b, const uint32_t* d_s, uint64_t m) {
  if (!m) return PG_OK;
  hipLaunchKernelGGL(components_hook_kernel, dim3(grid_for(m, 256 * 4, (uint32_t)ctx->num_cu * 8u)), dim3(256), 0, ctx->stream, d_a, d_b, d_s, m, C.n, C.d_parent.p,
                     C.d_entries.p, C.d_weight.p);
  PG_HIP(ctx, hipGetLastError());
  return PG_OK;
}

// K3, the count read back, and the finished state made the context's (the earlier one goes here, not before)
int components_finish(pg_ctx* ctx, std::unique_ptr<ComponentsState>& C, ScreenEvents& T, uint64_t worked, uint64_t ignored, uint32_t* n_components_out) {
  hipStream_t st = ctx->stream;
  {
    ScreenEvents::Stage flatten(T, ST_FLATTEN, st);
    hipLaunchKernelGGL(components_flatten_kernel, dim3(grid_for(C->n, 256, (uint32_t)ctx->num_cu * 8u)), dim3(256), 0, st, C->d_parent.p, C->n, C->d_root.p, C->d_count.p);
  }
  PG_HIP(ctx, hipGetLastError());
  unsigned long long count = 0;
  PG_HIP(ctx, hipMemcpyAsync(&count, C->d_count, 8, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipStreamSynchronize(st));
  if (count < 1 || count > C->n) return pg_fail(ctx, PG_E_INTERNAL, "screen: " + std::to_string(count) + " components of " + std::to_string(C->n) + " nodes");
  pg_screen_components_drop(ctx);
  PgScreenComponentsStats& L = ctx->screen_components_stats;
  L.nodes = C->n; L.worked = worked; L.ignored = ignored; L.components = count;
  L.select_ms = T.ms(ST_SELECT); L.hook_ms = T.ms(ST_HOOK); L.flatten_ms = T.ms(ST_FLATTEN);
  ctx->screen_components_state = C.release();
  *n_components_out = (uint32_t)count;
  return PG_OK;
}

}  // namespace

void pg_screen_components_drop(pg_ctx* ctx) {
  if (!ctx->screen_components_state) return;
  delete components_of(ctx);
  ctx->screen_components_state = nullptr;
  ctx->screen_components_stats = PgScreenComponentsStats{};
}

extern "C" int pg_screen_components_release(pg_ctx* ctx) {
  if (!ctx) return PG_E_ARG;
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  pg_screen_components_drop(ctx);
  return PG_OK;
}

extern "C" int pg_screen_components_last(pg_ctx* ctx, uint64_t* counts_out, double* ms_out) {
  if (!ctx || !counts_out || !ms_out) return pg_fail(ctx, PG_E_ARG, "bad argument");
  const PgScreenComponentsStats& L = ctx->screen_components_stats;
  counts_out[0] = L.nodes; counts_out[1] = L.worked; counts_out[2] = L.ignored; counts_out[3] = L.components;
  ms_out[0] = L.select_ms; ms_out[1] = L.hook_ms; ms_out[2] = L.flatten_ms;
  return PG_OK;
}

extern "C" int pg_screen_components_read(pg_ctx* ctx, int32_t* root_out, uint64_t* entries_out, uint64_t* weight_out) {
  if (!ctx) return PG_E_ARG;
  ComponentsState* C = components_of(ctx);
  if (!C) return pg_fail(ctx, PG_E_ARG, "screen: no resident components (call pg_screen_components or pg_screen_index_components first)");
  if (!root_out || !entries_out || !weight_out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  PG_HIP(ctx, hipMemcpyAsync(root_out, C->d_root, (size_t)C->n * 4, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipMemcpyAsync(entries_out, C->d_entries, (size_t)C->n * 8, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipMemcpyAsync(weight_out, C->d_weight, (size_t)C->n * 8, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipStreamSynchronize(st));
  return PG_OK;
}

extern "C" int pg_screen_components(pg_ctx* ctx, const int32_t* a, const int32_t* b, const uint32_t* shared, uint64_t m, uint32_t n, uint32_t* n_components_out) {
  if (!ctx) return PG_E_ARG;
  if (n < 1 || n > pgscr::INDEX_MAX_GENOMES) return pg_fail(ctx, PG_E_ARG, "screen: components are of 1 ... 1048576 (2^20) nodes, not " + std::to_string(n));
  if (!n_components_out || (m && (!a || !b))) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
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
  uint64_t chunk = COMPONENTS_CHUNK;
  if (const char* x = pg_dev_env("PYANI_COMPONENTS_CHUNK")) { const long long c = atoll(x); if (c >= 1) chunk = (uint64_t)c; }      // (tests: several chunks of a small list)
  chunk = std::min<uint64_t>(chunk, std::max<uint64_t>(m, 1));
  std::unique_ptr<ComponentsState> C(new ComponentsState());
  PgDevBuf<int32_t> d_a, d_b;
  PgDevBuf<uint32_t> d_s;
  int rc;
  if ((rc = components_alloc(ctx, n, *C)) || (rc = pg_dev_alloc(ctx, "screen", d_a, (size_t)chunk, "a chunk of the entries")) ||
      (rc = pg_dev_alloc(ctx, "screen", d_b, (size_t)chunk, "a chunk of the entries")) ||
      (shared && (rc = pg_dev_alloc(ctx, "screen", d_s, (size_t)chunk, "a chunk of the entries"))))
    return rc;
  ScreenEvents T;
  for (uint64_t at = 0; at < m; at += chunk) {
    const uint64_t c = std::min(chunk, m - at);
    PG_HIP(ctx, hipMemcpyAsync(d_a, a + at, (size_t)c * 4, hipMemcpyHostToDevice, st));
    PG_HIP(ctx, hipMemcpyAsync(d_b, b + at, (size_t)c * 4, hipMemcpyHostToDevice, st));
    if (shared) PG_HIP(ctx, hipMemcpyAsync(d_s, shared + at, (size_t)c * 4, hipMemcpyHostToDevice, st));
    { ScreenEvents::Stage hook(T, ST_HOOK, st); rc = components_hook(ctx, *C, d_a.p, d_b.p, shared ? d_s.p : nullptr, c); }
    if (rc) break;
  }
  if (!rc) rc = components_finish(ctx, C, T, m - ignored, ignored, n_components_out);      // (its synchronisation comes before the chunk buffers go)
  if (rc) (void)hipStreamSynchronize(st);      // the rule of band_loop: a queued copy may still read the caller's a, b, shared
  return rc;
}

extern "C" int pg_screen_index_components(pg_ctx* ctx, const uint32_t* need, uint32_t n, uint32_t band_first, uint32_t band_step, uint32_t* n_components_out,
                                          uint64_t* n_pairs_out) {
  if (!ctx) return PG_E_ARG;
  IndexState* I = nullptr;
  int rc;
  if ((rc = band_check(ctx, need, n, band_step, n_components_out && n_pairs_out, &I))) return rc;
  PG_HIP(ctx, hipSetDevice(ctx->device));
  std::unique_ptr<ComponentsState> C(new ComponentsState());
  if ((rc = components_alloc(ctx, n, *C))) return rc;
  ScreenEvents T;
  BandTotals tot;
  // the band's triples stay where the selection left them: hooked and accumulated there, before the next band overwrites them (one stream)
  const BandStages stages{ST_SELECT, ST_SELECT, ST_HOOK, false};
  rc = band_loop(ctx, I, need, band_first, band_step, T, stages, tot,
                 [&](uint32_t, uint32_t, unsigned long long total, BandWork& W) -> int { return components_hook(ctx, *C, W.a.p, W.b.p, W.s.p, total); });
  if (rc || (rc = components_finish(ctx, C, T, tot.kept, 0, n_components_out))) return rc;
  *n_pairs_out = tot.kept;
  return PG_OK;
}
