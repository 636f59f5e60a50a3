// pgscr_representatives.inc — part of pg_screen.hip: the greedy REPRESENTATIVES of the kept pairs (DESIGN.md §16.9).  Walk the nodes from the
// best score to the worst; a node none of whose neighbours is a representative becomes one; every other node then goes to the representative
// neighbour of the greatest pair weight.  The walk is the lexicographically first maximal independent set under the priority `rank`, and
// rounds over the entries reproduce it exactly: a node becomes a representative in the round in which its last undecided neighbour of
// higher priority has been covered.  One state word per node (UNDECIDED / REP / COVERED); kernel boundaries are the only ordering, no
// thread waits for another, every store goes through vector memory.
//   P1 representatives_keys_kernel    key[v] = ~score[v], value[v] = v; a stable hipcub radix sort of the pairs gives `order`
//   P2 representatives_rank_kernel    rank[order[i]] = i
//   P3 representatives_stamp_kernel   entry pass: both ends UNDECIDED -> the end of larger rank is stamped with the round number (every
//                                     writer writes the same value, a relaxed atomic store)
//   P4 representatives_decide_kernel  node pass: an UNDECIDED node not stamped this round becomes REP
//   P5 representatives_cover_kernel   entry pass: an UNDECIDED end opposite a REP becomes COVERED (a compare-and-swap, so that each
//                                     transition is counted once); P4 and P5 take what they decided off the round's control word, one
//                                     atomic per wave
//   P6 representatives_assign_kernel  entry pass: REP r — COVERED v: key[v] = max(key[v], weight << 32 | 0xFFFFFFFF - rank[r]), a run of
//                                     equal v inside a wave reduced by a segmented shuffle first (a star's hub: one atomic per wave)
//   P7 representatives_finish_kernel  node pass: rep[v], via[v]; the representatives counted, one atomic per wave
//   P8 representatives_append_kernel  index path: a band's kept triples with a < b appended to the device list through one cursor, one
//                                     returning atomic per wave
// The rounds are issued in batches with ONE read of the control words per batch: word k of a batch holds the nodes still undecided after
// its round k, and every kernel of a round whose predecessor's word is 0 returns at once.
namespace {

struct RepresentativesState {      // the resident result of the latest accepted representatives call
  uint32_t n = 0;
  PgDevBuf<int32_t> d_rep;        // n
  PgDevBuf<uint32_t> d_via;       // n
};

RepresentativesState* representatives_of(pg_ctx* ctx) { return static_cast<RepresentativesState*>(ctx->screen_representatives_state); }

constexpr uint32_t REP_UNDECIDED = 0u, REP_REP = 1u, REP_COVERED = 2u;
constexpr uint32_t REP_BATCH_FIRST = 4u, REP_BATCH_MAX = 64u;      // rounds of the first batch; every later batch doubles, up to the maximum
constexpr uint32_t REP_NONE = 0xFFFFFFFFu;

struct RepresentativesWork {      // what one call needs beside the entries; released when it returns
  PgDevBuf<unsigned long long> keys_in, keys_out, key, ctl, count;      // ctl: REP_BATCH_MAX + 1 words
  PgDevBuf<uint32_t> iota, order, rank, state, stamp;
  PgDevBuf<uint8_t> tmp;
  size_t tmp_bytes = 0;
};

__global__ __launch_bounds__(256) void representatives_keys_kernel(unsigned long long* __restrict__ keys, uint32_t* __restrict__ iota, uint32_t* __restrict__ state,
                                                                    uint32_t* __restrict__ stamp, unsigned long long* __restrict__ key, uint32_t n) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
    keys[v] = ~keys[v];      // (ascending ~score = descending score)
    iota[v] = v; state[v] = REP_UNDECIDED; stamp[v] = 0u; key[v] = 0ull;
  }
}

__global__ __launch_bounds__(256) void representatives_rank_kernel(const uint32_t* __restrict__ order, uint32_t* __restrict__ rank, uint32_t n) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t v = order[i];
    if (v < n) rank[v] = i;      // (a permutation of [0, n): the bound is kept for the memory's sake)
  }
}

__device__ __forceinline__ uint32_t representatives_peek(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(256) void representatives_stamp_kernel(const int32_t* __restrict__ a, const int32_t* __restrict__ b, uint64_t m, uint32_t n,
                                                                     const uint32_t* __restrict__ rank, const uint32_t* __restrict__ state, uint32_t* stamp,
                                                                     uint32_t round, const unsigned long long* __restrict__ before) {
  if (*before == 0ull) return;      // nothing undecided
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t ua = (uint32_t)a[e], ub = (uint32_t)b[e];
    if (ua == ub || ua >= n || ub >= n) continue;
    if (state[ua] != REP_UNDECIDED || state[ub] != REP_UNDECIDED) continue;      // (no kernel writes the states beside this one)
    const uint32_t loser = rank[ua] > rank[ub] ? ua : ub;
    if (representatives_peek(stamp + loser) != round) __hip_atomic_store(stamp + loser, round, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(256) void representatives_decide_kernel(uint32_t n, uint32_t* __restrict__ state, const uint32_t* __restrict__ stamp, uint32_t round,
                                                                      const unsigned long long* __restrict__ before, unsigned long long* after) {
  const unsigned long long undecided = *before;
  if (undecided == 0ull) return;
  const uint32_t lane = threadIdx.x & 63u;
  if (blockIdx.x == 0u && threadIdx.x == 0u) atomicAdd(after, undecided);      // after = before - what P4 and P5 decide (sums modulo 2^64)
  for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {      // (uniform over the workgroup)
    const uint32_t v = base + threadIdx.x;
    const bool rep = v < n && state[v] == REP_UNDECIDED && stamp[v] != round;
    if (rep) state[v] = REP_REP;
    const unsigned long long reps = __ballot(rep);
    if (lane == 0u && reps) atomicAdd(after, 0ull - (unsigned long long)__popcll(reps));
  }
}

__global__ __launch_bounds__(256) void representatives_cover_kernel(const int32_t* __restrict__ a, const int32_t* __restrict__ b, uint64_t m, uint32_t n, uint32_t* state,
                                                                     const unsigned long long* __restrict__ before, unsigned long long* after) {
  if (*before == 0ull) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  for (uint64_t base = wave * 64ull; base < m; base += n_waves * 64ull) {      // (uniform over the wave: every lane reaches the ballot)
    const uint64_t e = base + lane;
    bool covered = false;
    if (e < m) {
      const uint32_t ua = (uint32_t)a[e], ub = (uint32_t)b[e];
      if (ua != ub && ua < n && ub < n) {
        const uint32_t sa = representatives_peek(state + ua), sb = representatives_peek(state + ub);      // (REP does not change here; UNDECIDED may become COVERED)
        const uint32_t v = sa == REP_REP && sb == REP_UNDECIDED ? ub : (sb == REP_REP && sa == REP_UNDECIDED ? ua : REP_NONE);
        if (v != REP_NONE) covered = atomicCAS(state + v, REP_UNDECIDED, REP_COVERED) == REP_UNDECIDED;      // one winner per node
      }
    }
    const unsigned long long won = __ballot(covered);
    if (lane == 0u && won) atomicAdd(after, 0ull - (unsigned long long)__popcll(won));
  }
}

__global__ __launch_bounds__(256) void representatives_assign_kernel(const int32_t* __restrict__ a, const int32_t* __restrict__ b, const uint32_t* __restrict__ w, uint64_t m,
                                                                      uint32_t n, const uint32_t* __restrict__ rank, const uint32_t* __restrict__ state,
                                                                      unsigned long long* __restrict__ key) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  for (uint64_t base = wave * 64ull; base < m; base += n_waves * 64ull) {      // (uniform over the wave: every lane reaches the shuffles)
    const uint64_t e = base + lane;
    uint32_t dest = REP_NONE;
    unsigned long long val = 0ull;
    if (e < m) {
      const uint32_t ua = (uint32_t)a[e], ub = (uint32_t)b[e];
      if (ua != ub && ua < n && ub < n) {
        const uint32_t sa = state[ua], sb = state[ub];
        uint32_t r = REP_NONE;
        if (sa == REP_REP && sb == REP_COVERED) { dest = ub; r = ua; }
        else if (sb == REP_REP && sa == REP_COVERED) { dest = ua; r = ub; }
        if (r != REP_NONE) val = ((unsigned long long)(w ? w[e] : 1u) << 32) | (unsigned long long)(0xFFFFFFFFu - rank[r]);
      }
    }
    // runs of equal destination in consecutive lanes, as the hook kernel's sums: the run's maximum ends at its head
    const uint32_t prev = __shfl_up(dest, 1, 64);
    const bool head = lane == 0u || dest != prev;
    const unsigned long long heads = __ballot(head);
    const uint32_t run = (uint32_t)__popcll(heads & ((2ull << lane) - 1ull));      // (lane 63: 2 << 63 wraps to 0, minus one = every bit)
    for (uint32_t d = 1; d < 64u; d <<= 1) {
      const uint32_t r2 = __shfl_down(run, d, 64);
      const unsigned long long v2 = __shfl_down(val, d, 64);
      if (lane + d < 64u && r2 == run && v2 > val) val = v2;
    }
    if (head && dest != REP_NONE) atomicMax(key + dest, val);      // no return value
  }
}

__global__ __launch_bounds__(256) void representatives_finish_kernel(uint32_t n, const uint32_t* __restrict__ state, const unsigned long long* __restrict__ key,
                                                                      const uint32_t* __restrict__ order, int32_t* __restrict__ rep, uint32_t* __restrict__ via,
                                                                      unsigned long long* __restrict__ count) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {      // (uniform over the workgroup)
    const uint32_t v = base + threadIdx.x;
    bool is_rep = false;
    if (v < n) {
      is_rep = state[v] == REP_REP;
      if (is_rep) {
        rep[v] = (int32_t)v; via[v] = 0u;
      } else {
        const unsigned long long k = key[v];
        const uint32_t at = 0xFFFFFFFFu - (uint32_t)k;      // the rank of the representative
        rep[v] = at < n ? (int32_t)order[at] : -1;          // (-1: never — a covered node has a key; the host refuses such a result)
        via[v] = (uint32_t)(k >> 32);
      }
    }
    const unsigned long long reps = __ballot(is_rep);
    if (lane == 0u && reps) atomicAdd(count, (unsigned long long)__popcll(reps));
  }
}

__global__ __launch_bounds__(256) void representatives_append_kernel(const int32_t* __restrict__ a, const int32_t* __restrict__ b, const uint32_t* __restrict__ s, uint64_t m,
                                                                      int32_t* __restrict__ la, int32_t* __restrict__ lb, uint32_t* __restrict__ lw, uint64_t cap,
                                                                      unsigned long long* cursor) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  for (uint64_t base = wave * 64ull; base < m; base += n_waves * 64ull) {      // (uniform over the wave)
    const uint64_t e = base + lane;
    const bool keep = e < m && a[e] < b[e];
    const unsigned long long kept = __ballot(keep);
    if (!kept) continue;
    unsigned long long at = 0ull;
    if (lane == 0u) at = atomicAdd(cursor, (unsigned long long)__popcll(kept));
    at = __shfl(at, 0, 64) + (unsigned long long)__popcll(kept & ((1ull << lane) - 1ull));
    if (keep && at < cap) { la[at] = a[e]; lb[at] = b[e]; lw[at] = s[e]; }      // (the host gave room for every kept triple: the bound is kept for the memory's sake)
  }
}

// The undirected kept pairs of ALL bands of the resident index, a < b, appended band by band to a list on the device: 12 bytes each.  The
// room grows ahead of every band by what the band kept (its triples with a < b cannot be more), at least doubling, the list copied over
// on the device.  Shared by pg_screen_index_representatives and pg_screen_index_evaluate; the bands are timed under ST_SELECT.
struct KeptList {
  PgDevBuf<int32_t> a, b;
  PgDevBuf<uint32_t> w;
  uint64_t held = 0;
};

int representatives_collect(pg_ctx* ctx, const IndexState* I, const uint32_t* need, ScreenEvents& T, KeptList& L, BandTotals& tot) {
  hipStream_t st = ctx->stream;
  PgDevBuf<unsigned long long> cursor;
  int rc;
  if ((rc = pg_dev_alloc(ctx, "screen", cursor, 1, "the kept pairs' cursor"))) return rc;
  PG_HIP(ctx, hipMemsetAsync(cursor, 0, 8, st));
  uint64_t cap = 0;
  uint64_t& held = L.held;
  const BandStages stages{ST_SELECT, ST_SELECT, ST_SELECT, false};
  rc = band_loop(ctx, I, need, 0, 1, T, stages, tot, [&](uint32_t, uint32_t, unsigned long long total, BandWork& W) -> int {
    if (!total) return PG_OK;
    if (held + total > cap) {
      const uint64_t room = std::max<uint64_t>(held + total, 2 * cap);
      PgDevBuf<int32_t> g_a, g_b;
      PgDevBuf<uint32_t> g_w;
      int r;
      if ((r = pg_dev_alloc(ctx, "screen", g_a, (size_t)room, "the kept pairs")) || (r = pg_dev_alloc(ctx, "screen", g_b, (size_t)room, "the kept pairs")) ||
          (r = pg_dev_alloc(ctx, "screen", g_w, (size_t)room, "the kept pairs")))
        return r;
      if (held) {
        PG_HIP(ctx, hipMemcpyAsync(g_a, L.a, (size_t)held * 4, hipMemcpyDeviceToDevice, st));
        PG_HIP(ctx, hipMemcpyAsync(g_b, L.b, (size_t)held * 4, hipMemcpyDeviceToDevice, st));
        PG_HIP(ctx, hipMemcpyAsync(g_w, L.w, (size_t)held * 4, hipMemcpyDeviceToDevice, st));
        PG_HIP(ctx, hipStreamSynchronize(st));      // (the old blocks go with the moves below)
      }
      L.a = std::move(g_a); L.b = std::move(g_b); L.w = std::move(g_w);
      cap = room;
    }
    hipLaunchKernelGGL(representatives_append_kernel, dim3(grid_for(total, 256 * 4, (uint32_t)ctx->num_cu * 8u)), dim3(256), 0, st, (const int32_t*)W.a.p, (const int32_t*)W.b.p,
                       (const uint32_t*)W.s.p, (uint64_t)total, L.a.p, L.b.p, L.w.p, cap, cursor.p);
    PG_HIP(ctx, hipGetLastError());
    unsigned long long at = 0;
    PG_HIP(ctx, hipMemcpyAsync(&at, cursor, 8, hipMemcpyDeviceToHost, st));
    PG_HIP(ctx, hipStreamSynchronize(st));
    if (at < held || at > held + total || at > cap) return pg_fail(ctx, PG_E_INTERNAL, "screen: a band appended more pairs than it kept");
    held = at;
    return PG_OK;
  });
  if (rc) return rc;
  if (held * 2 != tot.kept) return pg_fail(ctx, PG_E_INTERNAL, "screen: " + std::to_string(tot.kept) + " kept cells but " + std::to_string(held) + " undirected pairs");
  return PG_OK;
}

// Everything after the entries stand on the device (w may be null: every entry weighs 1): ranks, rounds, assign, and the finished state
// made the context's (the earlier one goes here, not before).  score is the host's.
int representatives_run(pg_ctx* ctx, uint32_t n, const int32_t* d_a, const int32_t* d_b, const uint32_t* d_w, uint64_t m, const uint64_t* score, ScreenEvents& T,
                        uint64_t worked, uint64_t ignored, uint32_t* n_representatives_out) {
  hipStream_t st = ctx->stream;
  const uint32_t cu_blocks = (uint32_t)ctx->num_cu * 8u;
  const dim3 node_grid(grid_for(n, 256, cu_blocks)), entry_grid(grid_for(m, 256 * 4, cu_blocks));
  std::unique_ptr<RepresentativesState> R(new RepresentativesState());
  RepresentativesWork W;
  int rc;
  PG_HIP(ctx, tmp_room(W.tmp_bytes, [&](size_t& bytes) {
    return hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                              (int64_t)n, 0, 64, st);
  }));
  if ((rc = pg_dev_alloc(ctx, "screen", R->d_rep, n, "the representatives")) || (rc = pg_dev_alloc(ctx, "screen", R->d_via, n, "the representatives' weights")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.keys_in, n, "the score keys")) || (rc = pg_dev_alloc(ctx, "screen", W.keys_out, n, "the score keys")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.key, n, "the assign keys")) || (rc = pg_dev_alloc(ctx, "screen", W.ctl, REP_BATCH_MAX + 1, "the control words")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.count, 1, "the representatives' counter")) || (rc = pg_dev_alloc(ctx, "screen", W.iota, n, "the nodes")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.order, n, "the order of the nodes")) || (rc = pg_dev_alloc(ctx, "screen", W.rank, n, "the ranks of the nodes")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.state, n, "the states of the nodes")) || (rc = pg_dev_alloc(ctx, "screen", W.stamp, n, "the stamps of the nodes")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.tmp, W.tmp_bytes, "the sort's temporary storage")))
    return rc;
  R->n = n;
  PG_HIP(ctx, hipMemcpyAsync(W.keys_in, score, (size_t)n * 8, hipMemcpyHostToDevice, st));
  {
    ScreenEvents::Stage sort(T, ST_SORT, st);
    hipLaunchKernelGGL(representatives_keys_kernel, node_grid, dim3(256), 0, st, W.keys_in.p, W.iota.p, W.state.p, W.stamp.p, W.key.p, n);
    PG_HIP(ctx, hipGetLastError());
    size_t tb = W.tmp_bytes;
    PG_HIP(ctx, hipcub::DeviceRadixSort::SortPairs((void*)W.tmp.p, tb, (const unsigned long long*)W.keys_in.p, W.keys_out.p, (const uint32_t*)W.iota.p, W.order.p, (int64_t)n, 0, 64, st));
    hipLaunchKernelGGL(representatives_rank_kernel, node_grid, dim3(256), 0, st, (const uint32_t*)W.order.p, W.rank.p, n);
    PG_HIP(ctx, hipGetLastError());
  }
  // The rounds.  Word 0 of the control words = the nodes undecided before the batch, word k = after its round k.  Every live round decides
  // the undecided node of smallest rank at least, so the words fall strictly until they reach 0: at most n rounds.
  unsigned long long ctl[REP_BATCH_MAX + 1] = {};
  ctl[0] = n;
  uint64_t rounds = 0, launches = 0;
  uint32_t batch = REP_BATCH_FIRST;
  PG_HIP(ctx, hipMemsetAsync(W.ctl, 0, (REP_BATCH_MAX + 1) * 8, st));
  PG_HIP(ctx, hipMemcpyAsync(W.ctl, ctl, 8, hipMemcpyHostToDevice, st));
  for (;;) {
    {
      ScreenEvents::Stage stage(T, ST_ROUNDS, st);
      for (uint32_t k = 1; k <= batch; ++k) {
        const uint32_t round = (uint32_t)rounds + k;      // (at most n + REP_BATCH_MAX: far below 2^32; 0 is no round's number)
        const unsigned long long* before = W.ctl.p + (k - 1);
        if (m) hipLaunchKernelGGL(representatives_stamp_kernel, entry_grid, dim3(256), 0, st, d_a, d_b, m, n, (const uint32_t*)W.rank.p, (const uint32_t*)W.state.p, W.stamp.p, round, before);
        hipLaunchKernelGGL(representatives_decide_kernel, node_grid, dim3(256), 0, st, n, W.state.p, (const uint32_t*)W.stamp.p, round, before, W.ctl.p + k);
        if (m) hipLaunchKernelGGL(representatives_cover_kernel, entry_grid, dim3(256), 0, st, d_a, d_b, m, n, W.state.p, before, W.ctl.p + k);
        launches += m ? 3u : 1u;
      }
      PG_HIP(ctx, hipGetLastError());
    }
    PG_HIP(ctx, hipMemcpyAsync(ctl, W.ctl, ((size_t)batch + 1) * 8, hipMemcpyDeviceToHost, st));
    PG_HIP(ctx, hipStreamSynchronize(st));
    for (uint32_t k = 1; k <= batch && ctl[k - 1]; ++k) {
      if (ctl[k] >= ctl[k - 1]) return pg_fail(ctx, PG_E_INTERNAL, "screen: a round of the representatives decided no node");
      ++rounds;
    }
    if (ctl[batch] == 0ull) break;
    ctl[0] = ctl[batch];
    PG_HIP(ctx, hipMemsetAsync(W.ctl, 0, (REP_BATCH_MAX + 1) * 8, st));
    PG_HIP(ctx, hipMemcpyAsync(W.ctl, ctl, 8, hipMemcpyHostToDevice, st));
    PG_HIP(ctx, hipStreamSynchronize(st));      // (ctl is the host's: the copy lands before the next read overwrites it)
    batch = std::min(batch * 2u, REP_BATCH_MAX);
  }
  unsigned long long count = 0;
  PG_HIP(ctx, hipMemsetAsync(W.count, 0, 8, st));
  {
    ScreenEvents::Stage assign(T, ST_ASSIGN, st);
    if (m) hipLaunchKernelGGL(representatives_assign_kernel, entry_grid, dim3(256), 0, st, d_a, d_b, d_w, m, n, (const uint32_t*)W.rank.p, (const uint32_t*)W.state.p, W.key.p);
    hipLaunchKernelGGL(representatives_finish_kernel, node_grid, dim3(256), 0, st, n, (const uint32_t*)W.state.p, (const unsigned long long*)W.key.p, (const uint32_t*)W.order.p,
                       R->d_rep.p, R->d_via.p, W.count.p);
    PG_HIP(ctx, hipGetLastError());
  }
  PG_HIP(ctx, hipMemcpyAsync(&count, W.count, 8, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipStreamSynchronize(st));
  if (count < 1 || count > n) return pg_fail(ctx, PG_E_INTERNAL, "screen: " + std::to_string(count) + " representatives of " + std::to_string(n) + " nodes");
  pg_screen_representatives_drop(ctx);
  PgScreenRepresentativesStats& L = ctx->screen_representatives_stats;
  L.nodes = n; L.worked = worked; L.ignored = ignored; L.representatives = count; L.rounds = rounds; L.launches = launches;
  L.select_ms = T.ms(ST_SELECT); L.sort_ms = T.ms(ST_SORT); L.rounds_ms = T.ms(ST_ROUNDS); L.assign_ms = T.ms(ST_ASSIGN);
  ctx->screen_representatives_state = R.release();
  *n_representatives_out = (uint32_t)count;
  return PG_OK;
}

}  // namespace

void pg_screen_representatives_drop(pg_ctx* ctx) {
  if (!ctx->screen_representatives_state) return;
  delete representatives_of(ctx);
  ctx->screen_representatives_state = nullptr;
  ctx->screen_representatives_stats = PgScreenRepresentativesStats{};
}

extern "C" int pg_screen_representatives_release(pg_ctx* ctx) {
  if (!ctx) return PG_E_ARG;
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  pg_screen_representatives_drop(ctx);
  return PG_OK;
}

extern "C" int pg_screen_representatives_last(pg_ctx* ctx, uint64_t* counts_out, double* ms_out) {
  if (!ctx || !counts_out || !ms_out) return pg_fail(ctx, PG_E_ARG, "bad argument");
  const PgScreenRepresentativesStats& L = ctx->screen_representatives_stats;
  counts_out[0] = L.nodes; counts_out[1] = L.worked; counts_out[2] = L.ignored; counts_out[3] = L.representatives; counts_out[4] = L.rounds; counts_out[5] = L.launches;
  ms_out[0] = L.select_ms; ms_out[1] = L.sort_ms; ms_out[2] = L.rounds_ms; ms_out[3] = L.assign_ms;
  return PG_OK;
}

extern "C" int pg_screen_representatives_read(pg_ctx* ctx, int32_t* rep_out, uint32_t* via_out) {
  if (!ctx) return PG_E_ARG;
  RepresentativesState* R = representatives_of(ctx);
  if (!R) return pg_fail(ctx, PG_E_ARG, "screen: no resident representatives (call pg_screen_representatives or pg_screen_index_representatives first)");
  if (!rep_out || !via_out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  PG_HIP(ctx, hipMemcpyAsync(rep_out, R->d_rep, (size_t)R->n * 4, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipMemcpyAsync(via_out, R->d_via, (size_t)R->n * 4, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipStreamSynchronize(st));
  return PG_OK;
}

extern "C" int pg_screen_representatives(pg_ctx* ctx, const int32_t* a, const int32_t* b, const uint32_t* weight, uint64_t m, uint32_t n, const uint64_t* score,
                                         uint32_t* n_representatives_out) {
  if (!ctx) return PG_E_ARG;
  if (n < 1 || n > pgscr::INDEX_MAX_GENOMES) return pg_fail(ctx, PG_E_ARG, "screen: representatives are of 1 ... 1048576 (2^20) nodes, not " + std::to_string(n));
  if (!score) return pg_fail(ctx, PG_E_ARG, "screen: the representatives need a score for every node");
  if (!n_representatives_out || (m && (!a || !b))) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
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
  // the WHOLE list stands on the device: every round reads it again (an entry with a == b is passed over by every pass)
  PgDevBuf<int32_t> d_a, d_b;
  PgDevBuf<uint32_t> d_w;
  int rc;
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
    return representatives_run(ctx, n, d_a.p, d_b.p, weight ? d_w.p : nullptr, m, score, T, m - ignored, ignored, n_representatives_out);
  };
  rc = run();
  if (rc) (void)hipStreamSynchronize(st);      // the rule of band_loop: a queued copy may still read the caller's arrays
  return rc;
}

extern "C" int pg_screen_index_representatives(pg_ctx* ctx, const uint32_t* need, uint32_t n, const uint64_t* score, uint32_t* n_representatives_out,
                                               uint64_t* n_pairs_out) {
  if (!ctx) return PG_E_ARG;
  IndexState* I = nullptr;
  int rc;
  if ((rc = band_check(ctx, need, n, 1, n_representatives_out && n_pairs_out, &I))) return rc;
  if (!score) return pg_fail(ctx, PG_E_ARG, "screen: the representatives need a score for every node");
  if (n < 1) return pg_fail(ctx, PG_E_ARG, "screen: representatives are of 1 ... 1048576 (2^20) nodes, not 0");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  KeptList L;
  ScreenEvents T;
  BandTotals tot;
  if ((rc = representatives_collect(ctx, I, need, T, L, tot))) return rc;
  if ((rc = representatives_run(ctx, n, L.a.p, L.b.p, L.w.p, L.held, score, T, L.held, 0, n_representatives_out))) { (void)hipStreamSynchronize(st); return rc; }
  *n_pairs_out = tot.kept;
  return PG_OK;
}
