// pgscr_sweep.inc — part of pg_screen.hip: the SWEEP of the components over a ladder of thresholds (DESIGN.md §16.10).  Every entry
// (a, b, shared) carries a LEVEL: the number of leading steps of the ladder that keep it; it is present at step s iff level > s.  The graphs
// of the steps are nested — a lower step only adds entries — so ONE descending pass over ONE forest answers every step: for s = S - 1 ... 0
// the bucket level == s + 1 is hooked and accumulated into the persistent forest and node sums of pgscr_components.inc, and a census of the
// forest gives the step's row.  The forest's invariants hold unchanged (a cell only decreases, only atomics write it, no thread waits for
// another); the kernel boundaries of one stream are the only ordering between a bucket's hooks and its census.
//   W1 sweep_monotone_kernel      index form: one thread per column of the need table [S][n]: the column does not fall
//   W2 sweep_levels_kernel        index form: one thread per kept triple of a band: binary search over the S rows for the first step that
//                                 drops it; (a << 32 | b, shared, level) appended to the resident list
//   W3 sweep_pack_kernel          list form: a chunk of the host's (a, b, level) packed the same way; an entry with a == b gets level 0
//   W4 sweep_hist_kernel          the levels counted: an LDS histogram per workgroup, 64-bit atomics for what it holds
//      one stable hipcub radix sort on the level bits only, DESCENDING (twice with the same keys when there are weights): the buckets are
//      contiguous, level S first, and runs of equal a inside a bucket survive for the run reduction of the accumulate step
//   W5 sweep_init_kernel          parent[v] = root[v] = v, entries = weight = size = 0
//   W6 sweep_hook_kernel          components_hook_entry over ONE bucket; the successful compare-and-swaps counted, one atomic per wave
//   W7 sweep_census_nodes_kernel  root[v] = find(v); a run of equal roots inside a wave adds ONCE to size[root]
//   W8 sweep_census_roots_kernel  the nodes that are their own root: count, singletons, maximum and the sum of size (size - 1), reduced per
//                                 wave and then per workgroup, one atomic each per workgroup into the step's row; size[r] cleared for
//                                 the next census
// Nothing between the sort and the last census waits for the host: the bucket offsets are the control words, read once after the sort.
namespace {

constexpr uint32_t SWEEP_MAX_STEPS = 4096, SWEEP_MAX_SNAPSHOTS = 32;
constexpr uint64_t SWEEP_MAX_TABLE = 1ull << 28;      // words of the need table of the index form: 1 GB
constexpr uint64_t SWEEP_CHUNK = 1ull << 24;          // host entries staged at a time (a, b, level: 10 bytes each)
constexpr uint32_t SWEEP_ROW = 5;                     // words of a step's row on the device: hooks of its bucket, roots, singletons, largest, pair slots

struct SweepState {      // the resident result of the latest accepted sweep call
  uint32_t n = 0, steps = 0;
  std::vector<uint64_t> entries, pair_slots;                // steps each
  std::vector<uint32_t> components, singletons, largest;    // steps each
  std::vector<uint32_t> snap_steps;                         // the caller's list, in its order
  PgDevBuf<int32_t> d_snap_root;                            // snapshots x n
  PgDevBuf<unsigned long long> d_snap_entries, d_snap_weight;
};

SweepState* sweep_of(pg_ctx* ctx) { return static_cast<SweepState*>(ctx->screen_sweep_state); }

struct SweepList {      // the whole list on the device: 14 bytes an entry (10 without weights)
  PgDevBuf<unsigned long long> ab;      // a << 32 | b
  PgDevBuf<uint32_t> s;                 // the weights (unused when there are none)
  PgDevBuf<uint16_t> key;               // the level; 0 for an entry with a == b
  uint64_t m = 0, cap = 0;
  bool weighted = true;
};

__global__ __launch_bounds__(256) void sweep_monotone_kernel(const uint32_t* __restrict__ need, uint32_t n, uint32_t steps, unsigned long long* __restrict__ bad) {
  for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x) {
    uint32_t before = need[c];
    for (uint32_t s = 1; s < steps; ++s) {
      const uint32_t now = need[(size_t)s * n + c];
      if (now < before) { atomicMin(bad, (unsigned long long)c << 32 | s); break; }      // the smallest column that falls, and where
      before = now;
    }
  }
}

__global__ __launch_bounds__(256) void sweep_levels_kernel(const int32_t* __restrict__ a, const int32_t* __restrict__ b, const uint32_t* __restrict__ s, uint64_t m,
                                                            const uint32_t* __restrict__ need, uint32_t n, uint32_t steps, unsigned long long* __restrict__ ab,
                                                            uint32_t* __restrict__ ls, uint16_t* __restrict__ key) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t ua = (uint32_t)a[e], ub = (uint32_t)b[e], sh = s[e];
    uint32_t lo = 0u, hi = steps;      // the first step with sh < min(need[step][a], need[step][b]): the columns do not fall, so neither does the minimum
    if (ua >= n || ub >= n) hi = 0u;   // (never: the selection wrote them; the bound is kept for the memory's sake)
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      const uint32_t na = need[(size_t)mid * n + ua], nb = need[(size_t)mid * n + ub];
      if (sh < (na < nb ? na : nb)) hi = mid; else lo = mid + 1u;
    }
    ab[e] = (unsigned long long)ua << 32 | ub;
    ls[e] = sh;
    key[e] = (uint16_t)(ua == ub ? 0u : lo);
  }
}

__global__ __launch_bounds__(256) void sweep_pack_kernel(const int32_t* __restrict__ a, const int32_t* __restrict__ b, const uint16_t* __restrict__ level, uint64_t m,
                                                          unsigned long long* __restrict__ ab, uint16_t* __restrict__ key) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t ua = (uint32_t)a[e], ub = (uint32_t)b[e];
    ab[e] = (unsigned long long)ua << 32 | ub;
    key[e] = ua == ub ? (uint16_t)0 : level[e];      // ignored altogether: present at no step
  }
}

__global__ __launch_bounds__(256) void sweep_hist_kernel(const uint16_t* __restrict__ key, uint64_t m, uint32_t steps, unsigned long long* __restrict__ hist) {
  __shared__ uint32_t h[SWEEP_MAX_STEPS + 1];      // (32-bit counts: a workgroup sees far fewer than 2^32 entries of a list that fits the device)
  for (uint32_t l = threadIdx.x; l <= steps; l += blockDim.x) h[l] = 0u;
  __syncthreads();
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t l = key[e];
    if (l <= steps) atomicAdd(&h[l], 1u);      // (the host has refused a level above steps)
  }
  __syncthreads();
  for (uint32_t l = threadIdx.x; l <= steps; l += blockDim.x)
    if (h[l]) atomicAdd(hist + l, (unsigned long long)h[l]);
}

__global__ __launch_bounds__(256) void sweep_init_kernel(uint32_t* __restrict__ parent, int32_t* __restrict__ root, unsigned long long* __restrict__ entries,
                                                          unsigned long long* __restrict__ weight, uint32_t* __restrict__ size, uint32_t n) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
    parent[v] = v; root[v] = (int32_t)v; entries[v] = 0ull; weight[v] = 0ull; size[v] = 0u;
  }
}

__global__ __launch_bounds__(256) void sweep_hook_kernel(const unsigned long long* __restrict__ ab, const uint32_t* __restrict__ s, uint64_t lo, uint64_t hi, uint32_t n,
                                                          uint32_t* parent, unsigned long long* __restrict__ entries, unsigned long long* __restrict__ weight,
                                                          unsigned long long* hooks) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  for (uint64_t base = lo + wave * 64ull; base < hi; base += n_waves * 64ull) {      // (uniform over the wave: every lane reaches the shuffles)
    const uint64_t e = base + lane;
    const bool in = e < hi;
    const unsigned long long x = in ? ab[e] : ~0ull;
    const bool hooked = components_hook_entry(lane, in, (uint32_t)(x >> 32), (uint32_t)x, s, e, n, parent, entries, weight);
    const unsigned long long won = __ballot(hooked);
    if (lane == 0u && won) atomicAdd(hooks, (unsigned long long)__popcll(won));
  }
}

__global__ __launch_bounds__(256) void sweep_census_nodes_kernel(uint32_t* parent, uint32_t n, int32_t* __restrict__ root, uint32_t* __restrict__ size) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {      // (uniform over the workgroup)
    const uint32_t v = base + threadIdx.x;
    uint32_t r = 0xFFFFFFFFu, cnt = 0u;
    if (v < n) {
      r = components_find(parent, v);      // (no hook runs beside this kernel: what looks like a root is one; r <= v < n)
      root[v] = (int32_t)r;
      cnt = 1u;
    }
    // runs of equal root in consecutive lanes, as the hook's sums
    const uint32_t prev = __shfl_up(r, 1, 64);
    const bool head = lane == 0u || r != prev;
    const unsigned long long heads = __ballot(head);
    const uint32_t run = (uint32_t)__popcll(heads & ((2ull << lane) - 1ull));
    for (uint32_t d = 1; d < 64u; d <<= 1) {
      const uint32_t r2 = __shfl_down(run, d, 64), c2 = __shfl_down(cnt, d, 64);
      if (lane + d < 64u && r2 == run) cnt += c2;
    }
    if (head && cnt) atomicAdd(size + r, cnt);
  }
}

__global__ __launch_bounds__(256) void sweep_census_roots_kernel(const int32_t* __restrict__ root, uint32_t n, uint32_t* __restrict__ size, unsigned long long* row) {
  __shared__ unsigned long long part[4][4];      // per wave of the workgroup (256 threads): roots, singletons, largest, pair slots
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t cnt = 0u, single = 0u, mx = 0u;
  unsigned long long slots = 0ull;
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
    if ((uint32_t)root[v] != v) continue;
    const uint32_t sz = size[v];      // (the only thread that touches the cell in this kernel)
    size[v] = 0u;
    ++cnt;
    single += sz == 1u ? 1u : 0u;
    mx = sz > mx ? sz : mx;
    slots += sz ? (unsigned long long)sz * (unsigned long long)(sz - 1u) : 0ull;
  }
  for (uint32_t d = 32u; d; d >>= 1) {      // (every lane is here: the loop above holds no wave operation)
    const uint32_t m2 = __shfl_xor(mx, d, 64);
    cnt += __shfl_xor(cnt, d, 64);
    single += __shfl_xor(single, d, 64);
    slots += __shfl_xor(slots, d, 64);
    mx = m2 > mx ? m2 : mx;
  }
  if (lane == 0u) { part[wave][0] = cnt; part[wave][1] = single; part[wave][2] = mx; part[wave][3] = slots; }
  __syncthreads();
  if (threadIdx.x == 0u) {      // one set of atomics per WORKGROUP: measured, a set per wave made the census of 2^20 nodes 1 ms of same-address atomics
    unsigned long long c = 0ull, s1 = 0ull, big = 0ull, sl = 0ull;
    for (uint32_t w = 0; w < 4u; ++w) { c += part[w][0]; s1 += part[w][1]; big = part[w][2] > big ? part[w][2] : big; sl += part[w][3]; }
    if (c) {
      atomicAdd(row + 1, c);
      if (s1) atomicAdd(row + 2, s1);
      atomicMax(row + 3, big);
      if (sl) atomicAdd(row + 4, sl);
    }
  }
}

// n, steps and the snapshot list: what both entries refuse before anything else
int sweep_check(pg_ctx* ctx, uint32_t n, uint32_t steps, const uint32_t* snapshot_steps, uint32_t n_snapshots) {
  if (n < 1 || n > pgscr::INDEX_MAX_GENOMES) return pg_fail(ctx, PG_E_ARG, "screen: a sweep is over 1 ... 1048576 (2^20) nodes, not " + std::to_string(n));
  if (steps < 1 || steps > SWEEP_MAX_STEPS) return pg_fail(ctx, PG_E_ARG, "screen: a sweep has 1 ... 4096 steps, not " + std::to_string(steps));
  if (n_snapshots > SWEEP_MAX_SNAPSHOTS) return pg_fail(ctx, PG_E_ARG, "screen: a sweep keeps at most 32 snapshots, not " + std::to_string(n_snapshots));
  if (n_snapshots && !snapshot_steps) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  for (uint32_t k = 0; k < n_snapshots; ++k)
    if (snapshot_steps[k] >= steps)
      return pg_fail(ctx, PG_E_ARG, "screen: snapshot " + std::to_string(k) + " asks for step " + std::to_string(snapshot_steps[k]) + " of a sweep of " + std::to_string(steps) + " steps");
  return PG_OK;
}

// Everything after the list stands on the device: histogram, sort, the descending pass with its censuses and snapshots, the rows read
// back ONCE, and the finished state made the context's (the earlier one goes here, not before).
int sweep_run(pg_ctx* ctx, uint32_t n, uint32_t steps, SweepList& L, const uint32_t* snapshot_steps, uint32_t n_snapshots, ScreenEvents& T, uint64_t ignored) {
  hipStream_t st = ctx->stream;
  const uint32_t cu_blocks = (uint32_t)ctx->num_cu * 8u;
  const dim3 node_grid(grid_for(n, 256, cu_blocks)), root_grid(grid_for(n, 256 * 8, (uint32_t)ctx->num_cu * 2u));
  const uint64_t m = L.m;
  std::unique_ptr<SweepState> S(new SweepState());
  PgDevBuf<uint32_t> parent, size, s2;
  PgDevBuf<int32_t> root;
  PgDevBuf<unsigned long long> entries, weight, rows, hist, ab2;
  PgDevBuf<uint16_t> key2;
  PgDevBuf<uint8_t> tmp;
  size_t tmp_bytes = 0;
  int end_bit = 1;
  while ((steps >> end_bit) != 0u) ++end_bit;      // the bits of a level 0 ... steps
  PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& bytes) {
    return hipcub::DeviceRadixSort::SortPairsDescending(nullptr, bytes, (const uint16_t*)nullptr, (uint16_t*)nullptr, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                                        (int64_t)m, 0, end_bit, st);
  }));
  PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& bytes) {
    return hipcub::DeviceRadixSort::SortPairsDescending(nullptr, bytes, (const uint16_t*)nullptr, (uint16_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int64_t)m, 0,
                                                        end_bit, st);
  }));
  int rc;
  if ((rc = pg_dev_alloc(ctx, "screen", parent, n, "the sweep's forest")) || (rc = pg_dev_alloc(ctx, "screen", root, n, "the sweep's roots")) ||
      (rc = pg_dev_alloc(ctx, "screen", entries, n, "the sweep's entry counts")) || (rc = pg_dev_alloc(ctx, "screen", weight, n, "the sweep's weights")) ||
      (rc = pg_dev_alloc(ctx, "screen", size, n, "the sweep's component sizes")) || (rc = pg_dev_alloc(ctx, "screen", rows, (size_t)steps * SWEEP_ROW, "the sweep's rows")) ||
      (rc = pg_dev_alloc(ctx, "screen", hist, (size_t)steps + 1, "the levels' histogram")) || (rc = pg_dev_alloc(ctx, "screen", ab2, (size_t)m, "the sorted entries")) ||
      (rc = pg_dev_alloc(ctx, "screen", key2, (size_t)m, "the sorted levels")) || (L.weighted && (rc = pg_dev_alloc(ctx, "screen", s2, (size_t)m, "the sorted weights"))) ||
      (rc = pg_dev_alloc(ctx, "screen", tmp, tmp_bytes + 16, "the sort's temporary storage")) ||
      (n_snapshots && ((rc = pg_dev_alloc(ctx, "screen", S->d_snap_root, (size_t)n_snapshots * n, "the sweep's snapshots")) ||
                       (rc = pg_dev_alloc(ctx, "screen", S->d_snap_entries, (size_t)n_snapshots * n, "the sweep's snapshots")) ||
                       (rc = pg_dev_alloc(ctx, "screen", S->d_snap_weight, (size_t)n_snapshots * n, "the sweep's snapshots")))))
    return rc;
  S->n = n; S->steps = steps;
  S->snap_steps.assign(snapshot_steps, snapshot_steps + n_snapshots);
  hipLaunchKernelGGL(sweep_init_kernel, node_grid, dim3(256), 0, st, parent.p, root.p, entries.p, weight.p, size.p, n);
  PG_HIP(ctx, hipGetLastError());
  PG_HIP(ctx, hipMemsetAsync(rows, 0, (size_t)steps * SWEEP_ROW * 8, st));
  PG_HIP(ctx, hipMemsetAsync(hist, 0, ((size_t)steps + 1) * 8, st));
  std::vector<unsigned long long> h((size_t)steps + 1, 0ull);
  if (m) {
    ScreenEvents::Stage sort(T, ST_SORT, st);
    hipLaunchKernelGGL(sweep_hist_kernel, dim3(grid_for(m, 256 * 16, cu_blocks)), dim3(256), 0, st, (const uint16_t*)L.key.p, m, steps, hist.p);
    PG_HIP(ctx, hipGetLastError());
    size_t tb = tmp_bytes;
    PG_HIP(ctx, hipcub::DeviceRadixSort::SortPairsDescending((void*)tmp.p, tb, (const uint16_t*)L.key.p, key2.p, (const unsigned long long*)L.ab.p, ab2.p, (int64_t)m, 0, end_bit, st));
    if (L.weighted) {
      tb = tmp_bytes;
      PG_HIP(ctx, hipcub::DeviceRadixSort::SortPairsDescending((void*)tmp.p, tb, (const uint16_t*)L.key.p, key2.p, (const uint32_t*)L.s.p, s2.p, (int64_t)m, 0, end_bit, st));
    }
    PG_HIP(ctx, hipMemcpyAsync(h.data(), hist, ((size_t)steps + 1) * 8, hipMemcpyDeviceToHost, st));
  }
  PG_HIP(ctx, hipStreamSynchronize(st));      // the ONE read of the control words: the buckets' sizes
  uint64_t counted = 0;
  for (uint32_t l = 0; l <= steps; ++l) counted += h[l];
  if (counted != m || h[0] < ignored) return pg_fail(ctx, PG_E_INTERNAL, "screen: the levels' histogram holds " + std::to_string(counted) + " of " + std::to_string(m) + " entries");
  // the descending pass: the bucket of level s + 1 stands at [at, at + h[s + 1]) of the sorted list
  const uint32_t* d_s = L.weighted ? (const uint32_t*)s2.p : nullptr;
  uint64_t at = 0, buckets = 0;
  for (uint32_t s = steps; s-- > 0u;) {
    const uint64_t c = h[s + 1];
    if (c) {
      {
        ScreenEvents::Stage hook(T, ST_HOOK, st);
        hipLaunchKernelGGL(sweep_hook_kernel, dim3(grid_for(c, 256 * 4, cu_blocks)), dim3(256), 0, st, (const unsigned long long*)ab2.p, d_s, at, at + c, n, parent.p, entries.p,
                           weight.p, rows.p + (size_t)s * SWEEP_ROW);
      }
      {
        ScreenEvents::Stage census(T, ST_CENSUS, st);
        hipLaunchKernelGGL(sweep_census_nodes_kernel, node_grid, dim3(256), 0, st, parent.p, n, root.p, size.p);
        hipLaunchKernelGGL(sweep_census_roots_kernel, root_grid, dim3(256), 0, st, (const int32_t*)root.p, n, size.p, rows.p + (size_t)s * SWEEP_ROW);
      }
      PG_HIP(ctx, hipGetLastError());
      at += c;
      ++buckets;
    }
    for (uint32_t k = 0; k < n_snapshots; ++k) {      // (root is the latest census', and nothing was hooked since; before any, sweep_init_kernel's)
      if (snapshot_steps[k] != s) continue;
      PG_HIP(ctx, hipMemcpyAsync(S->d_snap_root.p + (size_t)k * n, root, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
      PG_HIP(ctx, hipMemcpyAsync(S->d_snap_entries.p + (size_t)k * n, entries, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
      PG_HIP(ctx, hipMemcpyAsync(S->d_snap_weight.p + (size_t)k * n, weight, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
    }
  }
  std::vector<unsigned long long> r((size_t)steps * SWEEP_ROW, 0ull);
  PG_HIP(ctx, hipMemcpyAsync(r.data(), rows, (size_t)steps * SWEEP_ROW * 8, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipStreamSynchronize(st));
  S->entries.resize(steps); S->pair_slots.resize(steps); S->components.resize(steps); S->singletons.resize(steps); S->largest.resize(steps);
  uint64_t present = 0, hooks = 0;
  uint32_t comps = n, single = n, big = 1u;      // above the top step: no entry, n singletons
  uint64_t slots = 0;
  for (uint32_t s = steps; s-- > 0u;) {
    if (h[s + 1]) {
      const unsigned long long* row = r.data() + (size_t)s * SWEEP_ROW;
      present += h[s + 1];
      hooks += row[0];
      if (hooks >= n || row[1] != n - hooks || row[2] > row[1] || row[3] < 1 || row[3] > n)
        return pg_fail(ctx, PG_E_INTERNAL, "screen: step " + std::to_string(s) + " of the sweep counted " + std::to_string(row[1]) + " roots after " + std::to_string(hooks) +
                                               " hooks over " + std::to_string(n) + " nodes");
      comps = (uint32_t)row[1]; single = (uint32_t)row[2]; big = (uint32_t)row[3]; slots = row[4];
    }      // an empty bucket: the row of step s + 1
    S->entries[s] = present; S->components[s] = comps; S->singletons[s] = single; S->largest[s] = big; S->pair_slots[s] = slots;
  }
  pg_screen_sweep_drop(ctx);
  PgScreenSweepStats& Z = ctx->screen_sweep_stats;
  Z.nodes = n; Z.steps = steps; Z.worked = m - ignored; Z.ignored = ignored; Z.level0 = h[0] - ignored; Z.buckets = buckets;
  Z.select_ms = T.ms(ST_SELECT); Z.sort_ms = T.ms(ST_SORT); Z.hook_ms = T.ms(ST_HOOK); Z.census_ms = T.ms(ST_CENSUS);
  ctx->screen_sweep_state = S.release();
  return PG_OK;
}

}  // namespace

void pg_screen_sweep_drop(pg_ctx* ctx) {
  if (!ctx->screen_sweep_state) return;
  delete sweep_of(ctx);
  ctx->screen_sweep_state = nullptr;
  ctx->screen_sweep_stats = PgScreenSweepStats{};
}

extern "C" int pg_screen_sweep_release(pg_ctx* ctx) {
  if (!ctx) return PG_E_ARG;
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  pg_screen_sweep_drop(ctx);
  return PG_OK;
}

extern "C" int pg_screen_sweep_last(pg_ctx* ctx, uint64_t* counts_out, double* ms_out) {
  if (!ctx || !counts_out || !ms_out) return pg_fail(ctx, PG_E_ARG, "bad argument");
  const PgScreenSweepStats& Z = ctx->screen_sweep_stats;
  counts_out[0] = Z.nodes; counts_out[1] = Z.steps; counts_out[2] = Z.worked; counts_out[3] = Z.ignored; counts_out[4] = Z.level0; counts_out[5] = Z.buckets;
  ms_out[0] = Z.select_ms; ms_out[1] = Z.sort_ms; ms_out[2] = Z.hook_ms; ms_out[3] = Z.census_ms;
  return PG_OK;
}

extern "C" int pg_screen_sweep_read(pg_ctx* ctx, uint64_t* entries_out, uint32_t* components_out, uint32_t* singletons_out, uint32_t* largest_out, uint64_t* pair_slots_out) {
  if (!ctx) return PG_E_ARG;
  SweepState* S = sweep_of(ctx);
  if (!S) return pg_fail(ctx, PG_E_ARG, "screen: no resident sweep (call pg_screen_sweep or pg_screen_index_sweep first)");
  if (!entries_out || !components_out || !singletons_out || !largest_out || !pair_slots_out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  std::copy(S->entries.begin(), S->entries.end(), entries_out);
  std::copy(S->components.begin(), S->components.end(), components_out);
  std::copy(S->singletons.begin(), S->singletons.end(), singletons_out);
  std::copy(S->largest.begin(), S->largest.end(), largest_out);
  std::copy(S->pair_slots.begin(), S->pair_slots.end(), pair_slots_out);
  return PG_OK;
}

extern "C" int pg_screen_sweep_read_snapshot(pg_ctx* ctx, uint32_t k, int32_t* root_out, uint64_t* entries_out, uint64_t* weight_out) {
  if (!ctx) return PG_E_ARG;
  SweepState* S = sweep_of(ctx);
  if (!S) return pg_fail(ctx, PG_E_ARG, "screen: no resident sweep (call pg_screen_sweep or pg_screen_index_sweep first)");
  if (k >= S->snap_steps.size())
    return pg_fail(ctx, PG_E_ARG, "screen: snapshot " + std::to_string(k) + " does not exist (the resident sweep keeps " + std::to_string(S->snap_steps.size()) + ")");
  if (!root_out || !entries_out || !weight_out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t n = S->n;
  PG_HIP(ctx, hipMemcpyAsync(root_out, S->d_snap_root.p + (size_t)k * n, n * 4, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipMemcpyAsync(entries_out, S->d_snap_entries.p + (size_t)k * n, n * 8, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipMemcpyAsync(weight_out, S->d_snap_weight.p + (size_t)k * n, n * 8, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipStreamSynchronize(st));
  return PG_OK;
}

extern "C" int pg_screen_sweep(pg_ctx* ctx, const int32_t* a, const int32_t* b, const uint32_t* shared, const uint16_t* level, uint64_t m, uint32_t n, uint32_t steps,
                               const uint32_t* snapshot_steps, uint32_t n_snapshots) {
  if (!ctx) return PG_E_ARG;
  int rc;
  if ((rc = sweep_check(ctx, n, steps, snapshot_steps, n_snapshots))) return rc;
  if (m && (!a || !b || !level)) return pg_fail(ctx, PG_E_ARG, "screen: bad argument (a NULL array of " + std::to_string(m) + " entries)");
  uint64_t ignored = 0;
  uint32_t outside = 0, above = 0;
  for (uint64_t i = 0; i < m; ++i) {      // before anything is copied or replaced (one branch-free pass; a negative index is a large unsigned one)
    outside |= (uint32_t)((uint32_t)a[i] >= n) | (uint32_t)((uint32_t)b[i] >= n);
    above |= (uint32_t)(level[i] > steps);
    ignored += a[i] == b[i] ? 1u : 0u;
  }
  for (uint64_t i = 0; (outside || above) && i < m; ++i) {
    if ((uint32_t)a[i] >= n || (uint32_t)b[i] >= n)
      return pg_fail(ctx, PG_E_ARG, "screen: entry " + std::to_string(i) + " names node " + std::to_string((uint32_t)a[i] >= n ? a[i] : b[i]) + " outside [0, " +
                                        std::to_string(n) + ")");
    if (level[i] > steps)
      return pg_fail(ctx, PG_E_ARG, "screen: entry " + std::to_string(i) + " has level " + std::to_string(level[i]) + " in a sweep of " + std::to_string(steps) + " steps");
  }
  PG_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  uint64_t chunk = SWEEP_CHUNK;
  if (const char* x = pg_dev_env("PYANI_SWEEP_CHUNK")) { const long long c = atoll(x); if (c >= 1) chunk = (uint64_t)c; }      // (tests: several chunks of a small list)
  chunk = std::min<uint64_t>(chunk, std::max<uint64_t>(m, 1));
  // the WHOLE list stands on the device for the sort; a, b and level go up a chunk at a time and are packed there
  SweepList L;
  PgDevBuf<int32_t> c_a, c_b;
  PgDevBuf<uint16_t> c_l;
  L.m = L.cap = m;
  L.weighted = shared != nullptr;
  if ((rc = pg_dev_alloc(ctx, "screen", L.ab, (size_t)m, "the entries")) || (rc = pg_dev_alloc(ctx, "screen", L.key, (size_t)m, "the entries' levels")) ||
      (shared && (rc = pg_dev_alloc(ctx, "screen", L.s, (size_t)m, "the entries' weights"))) || (rc = pg_dev_alloc(ctx, "screen", c_a, (size_t)chunk, "a chunk of the entries")) ||
      (rc = pg_dev_alloc(ctx, "screen", c_b, (size_t)chunk, "a chunk of the entries")) || (rc = pg_dev_alloc(ctx, "screen", c_l, (size_t)chunk, "a chunk of the entries")))
    return rc;
  const auto run = [&]() -> int {
    if (m && shared) PG_HIP(ctx, hipMemcpyAsync(L.s, shared, (size_t)m * 4, hipMemcpyHostToDevice, st));
    for (uint64_t at = 0; at < m; at += chunk) {
      const uint64_t c = std::min(chunk, m - at);
      PG_HIP(ctx, hipMemcpyAsync(c_a, a + at, (size_t)c * 4, hipMemcpyHostToDevice, st));
      PG_HIP(ctx, hipMemcpyAsync(c_b, b + at, (size_t)c * 4, hipMemcpyHostToDevice, st));
      PG_HIP(ctx, hipMemcpyAsync(c_l, level + at, (size_t)c * 2, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(sweep_pack_kernel, dim3(grid_for(c, 256 * 4, (uint32_t)ctx->num_cu * 8u)), dim3(256), 0, st, (const int32_t*)c_a.p, (const int32_t*)c_b.p,
                         (const uint16_t*)c_l.p, c, L.ab.p + at, L.key.p + at);
      PG_HIP(ctx, hipGetLastError());
    }
    ScreenEvents T;
    return sweep_run(ctx, n, steps, L, snapshot_steps, n_snapshots, T, ignored);
  };
  rc = run();
  if (rc) (void)hipStreamSynchronize(st);      // the rule of band_loop: a queued copy may still read the caller's arrays
  return rc;
}

extern "C" int pg_screen_index_sweep(pg_ctx* ctx, const uint32_t* need, uint32_t n, uint32_t steps, uint32_t band_first, uint32_t band_step,
                                     const uint32_t* snapshot_steps, uint32_t n_snapshots, uint64_t* n_pairs_out) {
  if (!ctx) return PG_E_ARG;
  IndexState* I = nullptr;
  int rc;
  if (steps < 1 || steps > SWEEP_MAX_STEPS) return pg_fail(ctx, PG_E_ARG, "screen: a sweep has 1 ... 4096 steps, not " + std::to_string(steps));      // (before `need` is sized by it)
  if ((uint64_t)steps * n > SWEEP_MAX_TABLE)      // (by the caller's n: before the index is asked whether it is its own)
    return pg_fail(ctx, PG_E_ARG, "screen: a need table of " + std::to_string(steps) + " steps x " + std::to_string(n) + " genomes is more than 2^28 words (1 GB)");
  if ((rc = band_check(ctx, need, n, band_step, n_pairs_out != nullptr, &I)) || (rc = sweep_check(ctx, n, steps, snapshot_steps, n_snapshots))) return rc;
  PG_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const uint32_t cu_blocks = (uint32_t)ctx->num_cu * 8u;
  PgDevBuf<uint32_t> table;
  PgDevBuf<unsigned long long> bad;
  if ((rc = pg_dev_alloc(ctx, "screen", table, (size_t)steps * n, "the need table")) || (rc = pg_dev_alloc(ctx, "screen", bad, 1, "the need table's check"))) return rc;
  ScreenEvents T;
  unsigned long long fell = ~0ull;
  {
    const auto check = [&]() -> int {
      ScreenEvents::Stage levels(T, ST_SELECT, st);
      PG_HIP(ctx, hipMemcpyAsync(table, need, (size_t)steps * n * 4, hipMemcpyHostToDevice, st));
      PG_HIP(ctx, hipMemsetAsync(bad, 0xFF, 8, st));
      hipLaunchKernelGGL(sweep_monotone_kernel, dim3(grid_for(n, 256, cu_blocks)), dim3(256), 0, st, (const uint32_t*)table.p, n, steps, bad.p);
      PG_HIP(ctx, hipGetLastError());
      PG_HIP(ctx, hipMemcpyAsync(&fell, bad, 8, hipMemcpyDeviceToHost, st));
      return PG_OK;
    };
    rc = check();
    const hipError_t e = hipStreamSynchronize(st);      // (the caller's table may still be read: waited for whatever check returned)
    if (rc) return rc;
    PG_HIP(ctx, e);
  }
  if (fell != ~0ull)
    return pg_fail(ctx, PG_E_ARG, "screen: the need table is not monotone: column " + std::to_string(fell >> 32) + " falls at step " + std::to_string(fell & 0xFFFFFFFFull));
  // every band's kept triples get their levels where the selection left them and are appended to the list: 14 bytes each.  The room grows
  // ahead of every band by what the band kept, at least doubling, the list copied over on the device.  Row 0 of the table selects.
  SweepList L;
  BandTotals tot;
  const BandStages stages{ST_SELECT, ST_SELECT, ST_SELECT, false};
  rc = band_loop(ctx, I, need, band_first, band_step, T, stages, tot, [&](uint32_t, uint32_t, unsigned long long total, BandWork& W) -> int {
    if (!total) return PG_OK;
    if (L.m + total > L.cap) {
      const uint64_t room = std::max<uint64_t>(L.m + total, 2 * L.cap);
      PgDevBuf<unsigned long long> g_ab;
      PgDevBuf<uint32_t> g_s;
      PgDevBuf<uint16_t> g_key;
      int r;
      if ((r = pg_dev_alloc(ctx, "screen", g_ab, (size_t)room, "the kept pairs")) || (r = pg_dev_alloc(ctx, "screen", g_s, (size_t)room, "the kept pairs")) ||
          (r = pg_dev_alloc(ctx, "screen", g_key, (size_t)room, "the kept pairs' levels")))
        return r;
      if (L.m) {
        PG_HIP(ctx, hipMemcpyAsync(g_ab, L.ab, (size_t)L.m * 8, hipMemcpyDeviceToDevice, st));
        PG_HIP(ctx, hipMemcpyAsync(g_s, L.s, (size_t)L.m * 4, hipMemcpyDeviceToDevice, st));
        PG_HIP(ctx, hipMemcpyAsync(g_key, L.key, (size_t)L.m * 2, hipMemcpyDeviceToDevice, st));
        PG_HIP(ctx, hipStreamSynchronize(st));      // (the old blocks go with the moves below)
      }
      L.ab = std::move(g_ab); L.s = std::move(g_s); L.key = std::move(g_key);
      L.cap = room;
    }
    hipLaunchKernelGGL(sweep_levels_kernel, dim3(grid_for(total, 256 * 4, cu_blocks)), dim3(256), 0, st, (const int32_t*)W.a.p, (const int32_t*)W.b.p, (const uint32_t*)W.s.p,
                       (uint64_t)total, (const uint32_t*)table.p, n, steps, L.ab.p + L.m, L.s.p + L.m, L.key.p + L.m);
    PG_HIP(ctx, hipGetLastError());
    L.m += total;
    return PG_OK;
  });
  if (rc) return rc;
  if (L.m != tot.kept) return pg_fail(ctx, PG_E_INTERNAL, "screen: " + std::to_string(tot.kept) + " kept cells but " + std::to_string(L.m) + " entries with a level");
  if ((rc = sweep_run(ctx, n, steps, L, snapshot_steps, n_snapshots, T, 0))) { (void)hipStreamSynchronize(st); return rc; }
  *n_pairs_out = tot.kept;
  return PG_OK;
}
