// pgscr_gather.inc — part of pg_screen.hip: the gather (DESIGN.md §16.5).  A query is decomposed into the collection's genomes: round after
// round the db genome that holds most of the query's k-mers NOT YET EXPLAINED wins (ties to the smaller index), is recorded with that count
// (unique) and its count in the untouched rectangle (total), and its k-mers leave the query.  The state is the search's: the resident index
// (k-mer -> holders, ascending), the counted rectangle, and the matched entries that pg_screen_gather_count leaves behind (one per matched
// (query, k-mer): G0).  The rounds run on a working copy of the rectangle (`left`) and of the entries; the rectangle and the kept entries
// are never written, so a selection or another gather over the same count sees what the count left.  Integers throughout: the result
// does not depend on the order in which anything arrives.
namespace {

constexpr uint32_t GATHER_G_BITS = 48;                     // an entry: query << 48 | index position of the k-mer (a query is below 2^16: the band's rows)
constexpr unsigned long long GATHER_G_MASK = (1ull << GATHER_G_BITS) - 1ull;
constexpr unsigned long long GATHER_DEAD = ~0ull;          // an entry that was claimed, or whose query has finished
constexpr uint32_t GATHER_NONE = ~0u;                      // the winner of a query that has none this round
constexpr uint32_t GATHER_CHUNK = 4096;                    // cells of one arg-max workgroup: 256 lanes x 4 loads of 4 cells
constexpr uint32_t GATHER_BATCH = 16;                      // rounds issued between two reads of the control words
constexpr uint32_t GATHER_MAX_RANKS = 65536;
constexpr uint64_t GATHER_COMPACT_MIN = 256;               // entry lists shorter than this are never compacted
// the control words (uint64): queries not finished | the last round that had one | entries claimed | decrements issued | entries dropped
// with their finished query
enum { GC_UNFINISHED, GC_ROUNDS, GC_CLAIMED, GC_DECR, GC_DROPPED, GC_WORDS };

struct EntryWeight {      // G0: the items of the i-th matched run: its query holders
  typedef uint32_t Index;
  const uint32_t *active, *run_first;
  uint32_t nr;
  uint64_t nu;
  __device__ unsigned long long operator()(uint32_t i) const {
    const uint32_t r = active[i];
    if (r >= nr) return 1ull;      // (never: the expand kernel checks again)
    return (r + 1u < nr ? run_first[r + 1u] : nu) - run_first[r];
  }
};

// G0 expand: item t of matched run r = its t-th query holder; entry[off[run] + t] = query << 48 | group[r].  The caller filled the range
// with GATHER_DEAD, so an item that fails a check leaves a dead entry, never an unwritten one.  WEIGHTED (the abundance count, DESIGN.md
// §16.8): abund[off[run] + t] = mult[that holder's key], the times the query holds the k-mer; its range was filled with 0.
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void gather_expand_kernel(const unsigned long long* __restrict__ u, uint64_t nu, const uint32_t* __restrict__ run_first, uint32_t nr,
                                                             const uint32_t* __restrict__ active, const unsigned long long* __restrict__ group, uint64_t D,
                                                             const unsigned long long* __restrict__ off, uint32_t na, unsigned long long P, unsigned long long per,
                                                             uint32_t q, unsigned long long* __restrict__ entry, const uint32_t* __restrict__ mult,
                                                             uint32_t* __restrict__ abund) {
  item_walk<uint32_t>(off, na, P, per, [=](uint32_t ga, unsigned long long t) {
    const uint32_t r = active[ga];
    if (r >= nr) return;
    const unsigned long long g = group[r];
    if (g >= D || g > GATHER_G_MASK) return;
    const uint64_t sq = run_first[r], eq = r + 1u < nr ? run_first[r + 1u] : nu;
    const unsigned long long at = off[ga] + t;
    if (sq + t < eq && eq <= nu && at < P) {
      const uint32_t qi = (uint32_t)u[sq + t];
      if (qi < q) {
        entry[at] = ((unsigned long long)qi << GATHER_G_BITS) | g;
        if (WEIGHTED) abund[at] = mult[sq + t];
      }
    }
  });
}

// The sums of the abundance count, one per query: item i of `src` adds src.weight(i) to sum[src.query(i)] where that query is below q.  Through
// 64-bit sums in LDS for the first WEIGHT_LDS queries (a call of one query would otherwise send every key to one word of HBM), one atomic
// in HBM per query and workgroup; the queries beyond go to HBM directly.
constexpr uint32_t WEIGHT_LDS = 4096;
struct KeyWeight {        // the distinct keys of a slice: the key's genome, the length of its run
  const unsigned long long* u;
  const uint32_t* mult;
  __device__ uint32_t query(uint64_t i) const { return (uint32_t)u[i]; }
  __device__ uint32_t weight(uint64_t i) const { return mult[i]; }
};
struct EntryAbund {       // the kept entries: the entry's query, its abundance (a dead entry has none)
  const unsigned long long* entry;
  const uint32_t* abund;
  __device__ uint32_t query(uint64_t i) const { const unsigned long long x = entry[i]; return x == GATHER_DEAD ? GATHER_NONE : (uint32_t)(x >> GATHER_G_BITS); }
  __device__ uint32_t weight(uint64_t i) const { return abund[i]; }
};
template <typename Src>
__global__ __launch_bounds__(256) void gather_weight_kernel(Src src, uint64_t n_items, uint32_t q, unsigned long long* __restrict__ sum) {
  __shared__ unsigned long long lsum[WEIGHT_LDS];
  const uint32_t in_lds = q < WEIGHT_LDS ? q : WEIGHT_LDS;
  for (uint32_t i = threadIdx.x; i < in_lds; i += blockDim.x) lsum[i] = 0ull;
  __syncthreads();
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_items; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t qi = src.query(i);
    if (qi >= q) continue;
    const unsigned long long w = src.weight(i);
    if (qi < in_lds) atomicAdd(&lsum[qi], w); else atomicAdd(&sum[qi], w);
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < in_lds; i += blockDim.x)
    if (lsum[i]) atomicAdd(&sum[i], lsum[i]);
}

// matched[i] = the entries of query i, through a histogram in LDS (q <= the band's rows, 8192: 32 KB)
__global__ __launch_bounds__(256) void gather_matched_kernel(const unsigned long long* __restrict__ entry, uint64_t m_entries, uint32_t q, uint32_t* __restrict__ matched) {
  __shared__ uint32_t lcount[pgscr::MAX_BAND_ROWS];
  for (uint32_t i = threadIdx.x; i < q && i < pgscr::MAX_BAND_ROWS; i += blockDim.x) lcount[i] = 0u;
  __syncthreads();
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m_entries; e += (uint64_t)gridDim.x * blockDim.x) {
    const unsigned long long x = entry[e];
    const uint32_t qi = (uint32_t)(x >> GATHER_G_BITS);
    if (x != GATHER_DEAD && qi < q && qi < pgscr::MAX_BAND_ROWS) atomicAdd(&lcount[qi], 1u);
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < q && i < pgscr::MAX_BAND_ROWS; i += blockDim.x)
    if (lcount[i]) atomicAdd(&matched[i], lcount[i]);
}

// rows[i] = the cells of row i that are not zero: a query has at most that many ranks (every winner owns a positive cell of its own)
__global__ __launch_bounds__(256) void gather_nonzero_kernel(const uint32_t* __restrict__ rect, uint32_t q, uint32_t n, uint32_t* __restrict__ rows) {
  __shared__ uint32_t wsum[4];
  const uint32_t i = blockIdx.y;
  if (i >= q) return;
  const uint64_t c0 = (uint64_t)blockIdx.x * GATHER_CHUNK, c1 = c0 + GATHER_CHUNK < n ? c0 + GATHER_CHUNK : n;
  uint32_t mine = 0;
  for (uint64_t c = c0 + threadIdx.x; c < c1; c += 256u) mine += rect[(size_t)i * n + c] ? 1u : 0u;
  for (int d = 32; d > 0; d >>= 1) mine += __shfl_down(mine, d, 64);
  if ((threadIdx.x & 63u) == 0u) wsum[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0u) {
    const uint32_t all = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    if (all) atomicAdd(&rows[i], all);
  }
}

struct RankRoom {      // the row slots of query i: min(nonzero cells, max_ranks)
  typedef uint32_t Index;
  const uint32_t* rows;
  uint32_t max_ranks;
  __device__ unsigned long long operator()(uint32_t i) const { return rows[i] < max_ranks ? rows[i] : max_ranks; }
};
struct RankCount {     // the rows query i recorded
  typedef uint32_t Index;
  const uint32_t* nrank;
  __device__ unsigned long long operator()(uint32_t i) const { return nrank[i]; }
};

// G1 arg-max: workgroup (x, i) owns the cells [x CHUNK, (x + 1) CHUNK) of row i of `left`.  The row starts at cell i n of the array, which
// need not be a multiple of 4: the loads are the ALIGNED 16-byte words that cover the chunk (the array is padded by a word), and a cell
// outside the chunk is masked.  key = count << 32 | (0xFFFFFFFF - b): the largest count, among equals the smallest b; a zero cell has no
// key, and a workgroup without one issues no atomic (best starts at 0).
__global__ __launch_bounds__(256) void gather_argmax_kernel(const uint32_t* __restrict__ left, uint32_t q, uint32_t n, const uint32_t* __restrict__ done,
                                                             const unsigned long long* __restrict__ ctl, unsigned long long* __restrict__ best) {
  __shared__ unsigned long long wkey[4];
  const uint32_t i = blockIdx.y;
  if (ctl[GC_UNFINISHED] == 0ull || i >= q || done[i]) return;      // (uniform over the workgroup)
  const uint64_t row = (uint64_t)i * n;
  const uint64_t c0 = row + (uint64_t)blockIdx.x * GATHER_CHUNK;
  const uint64_t c1 = c0 + GATHER_CHUNK < row + n ? c0 + GATHER_CHUNK : row + n;
  unsigned long long key = 0ull;
  for (uint64_t v = (c0 & ~3ull) + 4ull * threadIdx.x; v < c1; v += 1024ull) {
    const uint4 x = *reinterpret_cast<const uint4*>(left + v);
    const uint32_t val[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (uint32_t w = 0; w < 4u; ++w) {
      const uint64_t c = v + w;
      if (c >= c0 && c < c1 && val[w]) {
        const unsigned long long k2 = ((unsigned long long)val[w] << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)(c - row));
        key = k2 > key ? k2 : key;
      }
    }
  }
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned long long other = __shfl_down(key, d, 64);
    key = other > key ? other : key;
  }
  if ((threadIdx.x & 63u) == 0u) wkey[threadIdx.x >> 6] = key;
  __syncthreads();
  if (threadIdx.x == 0u) {
    for (uint32_t w = 1; w < 4u; ++w) key = wkey[w] > key ? wkey[w] : key;
    if (key) atomicMax(&best[i], key);
  }
}

// G2 decide, after the kernel boundary: one thread per query.  A query that is not finished either records a row (slot room[i] + its
// rank) and names its winner, or finishes: no cell reaches need[i], it has max_ranks rows, or a check fails.  best is reset for the next
// round.  round_no: the number of this round, counted from 1.
__global__ __launch_bounds__(256) void gather_decide_kernel(uint32_t q, uint32_t n, uint32_t max_ranks, unsigned long long round_no, const uint32_t* __restrict__ need,
                                                             const unsigned long long* __restrict__ room, unsigned long long slots, unsigned long long* __restrict__ best,
                                                             uint32_t* __restrict__ done, uint32_t* __restrict__ nrank, uint32_t* __restrict__ winner,
                                                             uint32_t* __restrict__ slot_db, uint32_t* __restrict__ slot_unique, unsigned long long* __restrict__ ctl) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= q || done[i]) return;
  atomicMax(&ctl[GC_ROUNDS], round_no);
  const unsigned long long key = best[i];
  best[i] = 0ull;
  const uint32_t count = (uint32_t)(key >> 32), b = 0xFFFFFFFFu - (uint32_t)key, r = nrank[i];
  const unsigned long long slot = room[i] + r;
  if (count == 0u || count < need[i] || r >= max_ranks || b >= n || slot >= room[i + 1u] || slot >= slots) {
    done[i] = 1u;
    winner[i] = GATHER_NONE;
    atomicAdd(&ctl[GC_UNFINISHED], ~0ull);      // (minus one)
    return;
  }
  slot_db[slot] = b;
  slot_unique[slot] = count;
  nrank[i] = r + 1u;
  winner[i] = b;
}

// G3 claim: a wave takes 64 consecutive entries at a time.  A lane whose entry is alive and whose query has a winner this round looks the
// winner up among the k-mer's holders, member[start[g], start[g + 1]) (ascending: a binary search).  The claiming lanes are balloted, and
// for each of them the WHOLE wave walks that k-mer's holders — lane j takes holder j, j + 64, ... — and takes one off the cell of every
// holder in the query's row: consecutive lanes run along one row, and a k-mer of 3000 holders is 47 steps of the wave, not one lane's
// loop.  The winner is a holder, so its own cell goes down as well and ends at 0.  The entry is then dead; so is the entry of a finished
// query (dropped: no decrement).  One pair of atomics per wave for the counters.
__global__ __launch_bounds__(256) void gather_claim_kernel(unsigned long long* __restrict__ entry, uint64_t m_entries, const unsigned long long* __restrict__ start,
                                                            const uint32_t* __restrict__ member, uint64_t D, uint64_t E, const uint32_t* __restrict__ winner,
                                                            const uint32_t* __restrict__ done, uint32_t q, uint32_t n, uint64_t cells, uint32_t* __restrict__ left,
                                                            unsigned long long* __restrict__ ctl) {
  if (ctl[GC_UNFINISHED] == 0ull) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  unsigned long long claimed = 0ull, decrements = 0ull, dropped = 0ull;      // (the wave's: the same in every lane)
  for (uint64_t base = wave * 64ull; base < m_entries; base += n_waves * 64ull) {      // (uniform over the wave)
    const uint64_t e = base + lane;
    bool claim = false, drop = false;
    uint32_t qi = GATHER_NONE, m = 0u;
    unsigned long long s = 0ull;
    if (e < m_entries) {
      const unsigned long long x = entry[e];
      if (x != GATHER_DEAD) {
        qi = (uint32_t)(x >> GATHER_G_BITS);
        const unsigned long long g = x & GATHER_G_MASK;
        if (qi >= q || g >= D) drop = true;      // (never)
        else if (done[qi]) drop = true;
        else {
          const uint32_t w = winner[qi];
          if (w < n) {
            s = start[g];
            const unsigned long long e1 = start[g + 1ull];
            if (s < e1 && e1 <= E && e1 - s <= (unsigned long long)n) {
              const uint64_t p = pgscr::lower_bound_u32(member, s, e1, w);
              if (p < e1 && member[p] == w) { claim = true; m = (uint32_t)(e1 - s); }
            }
          }
        }
      }
    }
    unsigned long long bal = __ballot(claim);
    dropped += (unsigned long long)__popcll(__ballot(drop));
    while (bal) {
      const int src = __ffsll((long long)bal) - 1;
      bal &= bal - 1ull;
      const uint32_t cq = __shfl(qi, src, 64), cm = __shfl(m, src, 64);
      const unsigned long long cs = __shfl(s, src, 64);
      for (uint32_t j = lane; j < cm; j += 64u) {
        const uint32_t col = member[cs + j];
        const uint64_t cell = (uint64_t)cq * n + col;
        if (col < n && cell < cells) atomicSub(&left[cell], 1u);
      }
      claimed += 1ull;
      decrements += cm;
    }
    if (claim || drop) entry[e] = GATHER_DEAD;
  }
  if (lane == 0u) {
    if (claimed) { atomicAdd(&ctl[GC_CLAIMED], claimed); atomicAdd(&ctl[GC_DECR], decrements); }
    if (dropped) atomicAdd(&ctl[GC_DROPPED], dropped);
  }
}

struct GatherAlive {
  __host__ __device__ __forceinline__ bool operator()(unsigned long long x) const { return x != GATHER_DEAD; }
};

// the rows in their final order: slot s of the room belongs to query i (binary search over room), rank s - room[i]; it is a row iff the
// query recorded that many; then it goes to out[first[i] + rank] with total = the counted rectangle's cell
__global__ __launch_bounds__(256) void gather_rows_kernel(uint32_t q, uint32_t n, unsigned long long slots, const unsigned long long* __restrict__ room,
                                                           const unsigned long long* __restrict__ first, unsigned long long n_rows, const uint32_t* __restrict__ nrank,
                                                           const uint32_t* __restrict__ slot_db, const uint32_t* __restrict__ slot_unique,
                                                           const uint32_t* __restrict__ rect, int32_t* __restrict__ row_q, int32_t* __restrict__ row_db,
                                                           uint32_t* __restrict__ row_unique, uint32_t* __restrict__ row_total) {
  for (unsigned long long s = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; s < slots; s += (unsigned long long)gridDim.x * blockDim.x) {
    uint32_t lo = 0, hi = q - 1u;      // the last query whose room starts at or before s
    while (lo < hi) { const uint32_t mid = (lo + hi + 1u) >> 1; if (room[mid] <= s) lo = mid; else hi = mid - 1u; }
    const unsigned long long rank = s - room[lo];
    if (s >= room[lo + 1u] || rank >= nrank[lo]) continue;
    const unsigned long long at = first[lo] + rank;
    const uint32_t b = slot_db[s];
    if (at >= n_rows || b >= n) continue;
    row_q[at] = (int32_t)lo;
    row_db[at] = (int32_t)b;
    row_unique[at] = slot_unique[s];
    row_total[at] = rect[(size_t)lo * n + b];
  }
}

int gather_sink_prepare(pg_ctx* ctx, EntrySink& sink, uint64_t total_keys) {
  sink.cap = (size_t)total_keys;      // an entry is a distinct (k-mer, query) key that matched: M <= the query keys
  sink.M = 0;
  if (sk_malloc(ctx, sink.entry, sink.cap + 1))
    return pg_fail(ctx, PG_E_NOMEM, "screen: no device memory for up to " + std::to_string(sink.cap) + " matched entries of a gather (8 bytes each)");
  if (sink.weighted && sk_malloc(ctx, sink.abund, sink.cap + 1))
    return pg_fail(ctx, PG_E_NOMEM, "screen: no device memory for the abundances of up to " + std::to_string(sink.cap) + " matched entries of a gather (4 bytes each)");
  return PG_OK;
}

// The abundance count, per slice: every distinct key's multiplicity goes into its query's weight W.
int gather_sink_weight(QueryBack& B, const SliceGroups& S, ScreenEvents& T) {
  pg_ctx* ctx = B.ctx;
  if (!S.mult) return pg_fail(ctx, PG_E_INTERNAL, "screen: an abundance count over a front half that kept no multiplicities");
  ScreenEvents::Stage weight(T, ST_WEIGHT, ctx->stream);
  hipLaunchKernelGGL(gather_weight_kernel<KeyWeight>, dim3(grid_for(S.nu, 256 * 16, (uint32_t)ctx->num_cu * 4u)), dim3(256), 0, ctx->stream, KeyWeight{S.u, S.mult}, S.nu,
                     B.q, B.sink->weight.p);
  PG_HIP(ctx, hipGetLastError());
  return PG_OK;
}

// One more expansion over the matched runs of a slice (the search's own buffers: active, run_first, group; wts and off are free until the
// count stage): the weights = the runs' query holders, their scan, and G0 appends the slice's entries after the ones of the slices before.
int gather_sink_slice(QueryBack& B, const SliceGroups& S, ScreenEvents& T, uint32_t nr, uint32_t na) {
  pg_ctx* ctx = B.ctx;
  EntrySink& sink = *B.sink;
  hipStream_t st = ctx->stream;
  unsigned long long P = 0;
  {
    ScreenEvents::Stage expand(T, ST_EXPAND, st);
    PG_HIP(ctx, screen_weights(ctx, na, B.wts.p, EntryWeight{B.active.p, B.run_first.p, nr, S.nu}));
    size_t tb = S.tmp_bytes;
    PG_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(S.tmp, tb, B.wts.p, B.off.p, (int64_t)(na + 1), st));
  }
  PG_HIP(ctx, hipMemcpyAsync(&P, B.off.p + na, 8, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipStreamSynchronize(st));
  if (P < na || P > S.nu) return pg_fail(ctx, PG_E_INTERNAL, "screen: " + std::to_string(P) + " matched entries in a slice of " + std::to_string(S.nu) + " query keys");
  if (sink.M + P > sink.cap) return pg_fail(ctx, PG_E_INTERNAL, "screen: more matched entries than query keys");
  if (B.I->D > GATHER_G_MASK) return pg_fail(ctx, PG_E_INTERNAL, "screen: a search index of 2^48 k-mers or more cannot be gathered");
  const unsigned long long per = items_per_workgroup(ctx, P);
  ScreenEvents::Stage expand(T, ST_EXPAND, st);
  PG_HIP(ctx, hipMemsetAsync(sink.entry.p + sink.M, 0xFF, (size_t)P * 8, st));
  if (!sink.weighted) {
    hipLaunchKernelGGL(gather_expand_kernel<false>, dim3((uint32_t)((P + per - 1) / per)), dim3(256), 0, st, S.u, S.nu, (const uint32_t*)B.run_first.p, nr,
                       (const uint32_t*)B.active.p, (const unsigned long long*)B.group.p, B.I->D, (const unsigned long long*)B.off.p, na, P, per, B.q,
                       sink.entry.p + sink.M, (const uint32_t*)nullptr, (uint32_t*)nullptr);
  } else {      // (the abundances in step with the entries)
    if (!S.mult) return pg_fail(ctx, PG_E_INTERNAL, "screen: an abundance count over a front half that kept no multiplicities");
    PG_HIP(ctx, hipMemsetAsync(sink.abund.p + sink.M, 0, (size_t)P * 4, st));
    hipLaunchKernelGGL(gather_expand_kernel<true>, dim3((uint32_t)((P + per - 1) / per)), dim3(256), 0, st, S.u, S.nu, (const uint32_t*)B.run_first.p, nr,
                       (const uint32_t*)B.active.p, (const unsigned long long*)B.group.p, B.I->D, (const unsigned long long*)B.off.p, na, P, per, B.q,
                       sink.entry.p + sink.M, S.mult, sink.abund.p + sink.M);
  }
  PG_HIP(ctx, hipGetLastError());
  sink.M += P;
  return PG_OK;
}

// after the last slice: the entries of every query counted
int gather_sink_finish(pg_ctx* ctx, EntrySink& sink, uint32_t q, PgDevBuf<uint32_t>& matched, ScreenEvents& T) {
  hipStream_t st = ctx->stream;
  int rc;
  if (q > pgscr::MAX_BAND_ROWS) return pg_fail(ctx, PG_E_INTERNAL, "screen: more queries than a band has rows");
  if ((rc = pg_dev_alloc(ctx, "screen", matched, q, "the queries' matched counts"))) return rc;
  {
    ScreenEvents::Stage expand(T, ST_EXPAND, st);
    PG_HIP(ctx, hipMemsetAsync(matched, 0, (size_t)q * 4, st));
    if (sink.M) {
      hipLaunchKernelGGL(gather_matched_kernel, dim3(grid_for(sink.M, 256 * 16, (uint32_t)ctx->num_cu * 4u)), dim3(256), 0, st, (const unsigned long long*)sink.entry.p, sink.M, q,
                         matched.p);
      PG_HIP(ctx, hipGetLastError());
    }
  }
  if (sink.weighted && sink.M) {      // MW: the abundances of every query's entries
    ScreenEvents::Stage weight(T, ST_WEIGHT, st);
    hipLaunchKernelGGL(gather_weight_kernel<EntryAbund>, dim3(grid_for(sink.M, 256 * 16, (uint32_t)ctx->num_cu * 4u)), dim3(256), 0, st,
                       EntryAbund{sink.entry.p, sink.abund.p}, sink.M, q, sink.matched_weight.p);
    PG_HIP(ctx, hipGetLastError());
  }
  return PG_OK;
}

// every device buffer of one pg_screen_gather: gone with the call unless it is moved into the state
struct GatherWork {
  PgDevBuf<uint32_t> left, need, done, nrank, winner, nonzero, slot_db, slot_unique, row_unique, row_total;
  PgDevBuf<int32_t> row_q, row_db;
  PgDevBuf<unsigned long long> best, ctl, room, first, wts, work_a, work_b, n_alive;
  PgDevBuf<uint8_t> tmp;
};

// The rounds, after the buffers are made: returns with the stream idle or an error code.
int gather_run(pg_ctx* ctx, SearchState* I, const uint32_t* need, uint32_t q, uint32_t max_ranks, GatherWork& W, ScreenEvents& T, uint64_t* n_rows_out,
               unsigned long long* ctl_out) {
  hipStream_t st = ctx->stream;
  const uint32_t n = I->n;
  const uint64_t cells = (uint64_t)q * n;
  const uint32_t cu_blocks = (uint32_t)ctx->num_cu * 8u;
  const dim3 row_grid((n + GATHER_CHUNK - 1u) / GATHER_CHUNK, q);
  size_t tmp_bytes = 0;
  int rc;
  PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& b) { return hipcub::DeviceScan::ExclusiveSum(nullptr, b, W.wts.p, W.room.p, (int64_t)(q + 1), st); }));
  PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& b) {
    return hipcub::DeviceSelect::If(nullptr, b, W.work_a.p, W.work_b.p, W.n_alive.p, (int64_t)std::max<uint64_t>(I->M, 1), GatherAlive{}, st); }));
  if ((rc = pg_dev_alloc(ctx, "screen", W.tmp, tmp_bytes + 16, "the scan's temporary storage"))) return rc;
  // the working copies, the thresholds, and the room of every query's rows
  PG_HIP(ctx, hipMemsetAsync(W.left.p + cells, 0, 8 * 4, st));      // (the padding the arg-max's last 16-byte word may read)
  PG_HIP(ctx, hipMemcpyAsync(W.left, I->d_rect, cells * 4, hipMemcpyDeviceToDevice, st));
  if (I->M) PG_HIP(ctx, hipMemcpyAsync(W.work_a, I->d_entry, I->M * 8, hipMemcpyDeviceToDevice, st));
  PG_HIP(ctx, hipMemcpyAsync(W.need, need, (size_t)q * 4, hipMemcpyHostToDevice, st));
  PG_HIP(ctx, hipMemsetAsync(W.done, 0, (size_t)q * 4, st));
  PG_HIP(ctx, hipMemsetAsync(W.nrank, 0, (size_t)q * 4, st));
  PG_HIP(ctx, hipMemsetAsync(W.winner, 0xFF, (size_t)q * 4, st));
  PG_HIP(ctx, hipMemsetAsync(W.nonzero, 0, (size_t)q * 4, st));
  PG_HIP(ctx, hipMemsetAsync(W.best, 0, (size_t)q * 8, st));
  unsigned long long ctl[GC_WORDS] = {q, 0, 0, 0, 0};
  PG_HIP(ctx, hipMemcpyAsync(W.ctl, ctl, sizeof(ctl), hipMemcpyHostToDevice, st));
  unsigned long long slots = 0;
  {
    ScreenEvents::Stage argmax(T, ST_ARGMAX, st);
    hipLaunchKernelGGL(gather_nonzero_kernel, row_grid, dim3(256), 0, st, (const uint32_t*)I->d_rect.p, q, n, W.nonzero.p);
    PG_HIP(ctx, hipGetLastError());
    PG_HIP(ctx, screen_weights(ctx, q, W.wts.p, RankRoom{W.nonzero.p, max_ranks}));
    size_t tb = tmp_bytes;
    PG_HIP(ctx, hipcub::DeviceScan::ExclusiveSum((void*)W.tmp.p, tb, W.wts.p, W.room.p, (int64_t)(q + 1), st));
  }
  PG_HIP(ctx, hipMemcpyAsync(&slots, W.room.p + q, 8, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipStreamSynchronize(st));
  if (slots > cells || slots > (unsigned long long)q * max_ranks) return pg_fail(ctx, PG_E_INTERNAL, "screen: more row slots than cells");
  if ((rc = pg_dev_alloc(ctx, "screen", W.slot_db, (size_t)slots, "the rows of a gather")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.slot_unique, (size_t)slots, "the rows of a gather")))
    return rc;
  // The rounds, GATHER_BATCH at a time; between two batches the control words are read, and the entries move into a list of their own
  // size once fewer than half are alive (PYANI_GATHER_COMPACT=0 under PYANI_DEV_KNOBS=1: never — a development switch, same results).
  // Every round finishes a query or records a row, and a query records at most min(n, max_ranks) rows: a bound on the rounds.
  const char* knob = pg_dev_env("PYANI_GATHER_COMPACT");
  const bool compact = !(knob && atoi(knob) == 0);
  const unsigned long long max_rounds = (unsigned long long)std::min<uint32_t>(n, max_ranks) + 2ull;
  unsigned long long* cur = W.work_a.p;
  unsigned long long* other = W.work_b.p;
  uint64_t len = I->M, base_gone = 0;      // base_gone: claimed + dropped when `cur` was made
  unsigned long long round_no = 0;
  for (;;) {
    for (uint32_t k = 0; k < GATHER_BATCH; ++k) {
      ++round_no;
      {
        ScreenEvents::Stage argmax(T, ST_ARGMAX, st);
        hipLaunchKernelGGL(gather_argmax_kernel, row_grid, dim3(256), 0, st, (const uint32_t*)W.left.p, q, n, (const uint32_t*)W.done.p,
                           (const unsigned long long*)W.ctl.p, W.best.p);
        hipLaunchKernelGGL(gather_decide_kernel, dim3((q + 255u) / 256u), dim3(256), 0, st, q, n, max_ranks, round_no, (const uint32_t*)W.need.p,
                           (const unsigned long long*)W.room.p, slots, W.best.p, W.done.p, W.nrank.p, W.winner.p, W.slot_db.p, W.slot_unique.p, W.ctl.p);
      }
      if (len) {
        ScreenEvents::Stage claim(T, ST_CLAIM, st);
        hipLaunchKernelGGL(gather_claim_kernel, dim3(grid_for(len, 256, cu_blocks)), dim3(256), 0, st, cur, len, (const unsigned long long*)I->d_start.p,
                           (const uint32_t*)I->d_member.p, I->D, I->E, (const uint32_t*)W.winner.p, (const uint32_t*)W.done.p, q, n, cells, W.left.p, W.ctl.p);
      }
      PG_HIP(ctx, hipGetLastError());
    }
    PG_HIP(ctx, hipMemcpyAsync(ctl, W.ctl, sizeof(ctl), hipMemcpyDeviceToHost, st));
    PG_HIP(ctx, hipStreamSynchronize(st));
    if (ctl[GC_UNFINISHED] == 0ull) break;
    if (ctl[GC_UNFINISHED] > q || round_no > max_rounds) return pg_fail(ctx, PG_E_INTERNAL, "screen: a gather did not finish in " + std::to_string(max_rounds) + " rounds");
    const uint64_t gone = ctl[GC_CLAIMED] + ctl[GC_DROPPED] - base_gone;
    if (compact && other && len >= GATHER_COMPACT_MIN && gone <= len && (len - gone) * 2 < len) {
      unsigned long long alive = 0;
      {
        ScreenEvents::Stage claim(T, ST_CLAIM, st);
        size_t tb = tmp_bytes;
        PG_HIP(ctx, hipcub::DeviceSelect::If((void*)W.tmp.p, tb, cur, other, W.n_alive.p, (int64_t)len, GatherAlive{}, st));
      }
      PG_HIP(ctx, hipMemcpyAsync(&alive, W.n_alive, 8, hipMemcpyDeviceToHost, st));
      PG_HIP(ctx, hipStreamSynchronize(st));
      if (alive != len - gone) return pg_fail(ctx, PG_E_INTERNAL, "screen: " + std::to_string(alive) + " entries alive, not " + std::to_string(len - gone));
      std::swap(cur, other);
      len = alive;
      base_gone = ctl[GC_CLAIMED] + ctl[GC_DROPPED];
    }
  }
  // the rows, by query, then rank
  unsigned long long n_rows = 0;
  PG_HIP(ctx, screen_weights(ctx, q, W.wts.p, RankCount{W.nrank.p}));
  size_t tb = tmp_bytes;
  PG_HIP(ctx, hipcub::DeviceScan::ExclusiveSum((void*)W.tmp.p, tb, W.wts.p, W.first.p, (int64_t)(q + 1), st));
  PG_HIP(ctx, hipMemcpyAsync(&n_rows, W.first.p + q, 8, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipStreamSynchronize(st));
  if (n_rows > slots) return pg_fail(ctx, PG_E_INTERNAL, "screen: more rows than row slots");
  if ((rc = pg_dev_alloc(ctx, "screen", W.row_q, (size_t)n_rows, "the rows of a gather")) || (rc = pg_dev_alloc(ctx, "screen", W.row_db, (size_t)n_rows, "the rows of a gather")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.row_unique, (size_t)n_rows, "the rows of a gather")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.row_total, (size_t)n_rows, "the rows of a gather")))
    return rc;
  if (n_rows) {
    hipLaunchKernelGGL(gather_rows_kernel, dim3(grid_for(slots, 256, cu_blocks)), dim3(256), 0, st, q, n, slots, (const unsigned long long*)W.room.p,
                       (const unsigned long long*)W.first.p, n_rows, (const uint32_t*)W.nrank.p, (const uint32_t*)W.slot_db.p, (const uint32_t*)W.slot_unique.p,
                       (const uint32_t*)I->d_rect.p, W.row_q.p, W.row_db.p, W.row_unique.p, W.row_total.p);
    PG_HIP(ctx, hipGetLastError());
    PG_HIP(ctx, hipStreamSynchronize(st));
  }
  *n_rows_out = n_rows;
  for (int w = 0; w < GC_WORDS; ++w) ctl_out[w] = ctl[w];
  return PG_OK;
}

}  // namespace

extern "C" int pg_screen_gather_count(pg_ctx* ctx, const int32_t* query_ids, uint32_t q, uint32_t* sizes_out) {
  return search_count(ctx, query_ids, q, sizes_out, KEEP_ENTRIES);
}

extern "C" int pg_screen_gather(pg_ctx* ctx, const uint32_t* need, uint32_t q, uint32_t max_ranks, uint64_t* n_rows_out) {
  if (!ctx) return PG_E_ARG;
  SearchState* I = search_of(ctx);
  if (!I) return pg_fail(ctx, PG_E_ARG, "screen: no resident search index (call pg_screen_search_index first)");
  if (!I->counted || !I->kept) return pg_fail(ctx, PG_E_ARG, "screen: the latest count kept no entries (call pg_screen_gather_count first)");
  if (q != I->q) return pg_fail(ctx, PG_E_ARG, "screen: the counted rectangle is of " + std::to_string(I->q) + " queries, not " + std::to_string(q));
  if (max_ranks < 1 || max_ranks > GATHER_MAX_RANKS) return pg_fail(ctx, PG_E_ARG, "screen: max_ranks must be 1 ... 65536, not " + std::to_string(max_ranks));
  if ((q && !need) || !n_rows_out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PgScreenGatherStats& L = ctx->screen_gather_stats;
  if (q == 0) {      // (no rows)
    I->gathered = true;
    I->n_rows = 0;
    I->drop_abund_rows();
    I->d_left.release(); I->d_row_q.release(); I->d_row_db.release(); I->d_row_unique.release(); I->d_row_total.release();
    L.rounds = L.rows = L.claimed = L.decrements = 0;
    L.argmax_ms = L.claim_ms = 0.0;
    *n_rows_out = 0;
    return PG_OK;
  }
  const uint64_t cells = (uint64_t)q * I->n;
  GatherWork W;
  int rc;
  if ((rc = pg_dev_alloc(ctx, "screen", W.left, (size_t)cells + 8, "the working rectangle of a gather")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.work_a, (size_t)I->M, "the working entries of a gather")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.need, q, "the queries' thresholds")) || (rc = pg_dev_alloc(ctx, "screen", W.done, q, "the queries' state")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.nrank, q, "the queries' state")) || (rc = pg_dev_alloc(ctx, "screen", W.winner, q, "the queries' state")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.nonzero, q, "the queries' state")) || (rc = pg_dev_alloc(ctx, "screen", W.best, q, "the queries' state")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.ctl, GC_WORDS, "the control words")) || (rc = pg_dev_alloc(ctx, "screen", W.n_alive, 1, "the control words")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.room, (size_t)q + 1, "the queries' state")) || (rc = pg_dev_alloc(ctx, "screen", W.first, (size_t)q + 1, "the queries' state")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.wts, (size_t)q + 1, "the queries' state")))
    return rc;
  if (I->M >= GATHER_COMPACT_MIN && W.work_b.reserve((size_t)I->M) != hipSuccess) (void)hipGetLastError();      // (no room for the second list: no compaction)
  ScreenEvents T;
  uint64_t n_rows = 0;
  unsigned long long ctl[GC_WORDS] = {0, 0, 0, 0, 0};
  rc = gather_run(ctx, I, need, q, max_ranks, W, T, &n_rows, ctl);
  const hipError_t es = hipStreamSynchronize(ctx->stream);      // (on errors too: W goes with this scope)
  if (rc) return rc;
  PG_HIP(ctx, es);
  I->d_left = std::move(W.left);
  I->d_row_q = std::move(W.row_q); I->d_row_db = std::move(W.row_db); I->d_row_unique = std::move(W.row_unique); I->d_row_total = std::move(W.row_total);
  I->n_rows = n_rows;
  I->gathered = true;
  I->drop_abund_rows();      // (statistics of an earlier gather's rows)
  L.rounds = ctl[GC_ROUNDS]; L.rows = n_rows; L.claimed = ctl[GC_CLAIMED]; L.decrements = ctl[GC_DECR];
  L.argmax_ms = T.ms(ST_ARGMAX); L.claim_ms = T.ms(ST_CLAIM);
  *n_rows_out = n_rows;
  return PG_OK;
}

extern "C" int pg_screen_gather_read(pg_ctx* ctx, int32_t* query_out, int32_t* db_out, uint32_t* unique_out, uint32_t* total_out) {
  if (!ctx) return PG_E_ARG;
  SearchState* I = search_of(ctx);
  if (!I || !I->gathered) return pg_fail(ctx, PG_E_ARG, "screen: no gathered rows (call pg_screen_gather first)");
  if (I->n_rows == 0) return PG_OK;
  if (!query_out || !db_out || !unique_out || !total_out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PG_HIP(ctx, hipMemcpyAsync(query_out, I->d_row_q, I->n_rows * 4, hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipMemcpyAsync(db_out, I->d_row_db, I->n_rows * 4, hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipMemcpyAsync(unique_out, I->d_row_unique, I->n_rows * 4, hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipMemcpyAsync(total_out, I->d_row_total, I->n_rows * 4, hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PG_OK;
}

extern "C" int pg_screen_gather_fetch(pg_ctx* ctx, uint32_t* out) {
  if (!ctx) return PG_E_ARG;
  SearchState* I = search_of(ctx);
  if (!I || !I->gathered) return pg_fail(ctx, PG_E_ARG, "screen: no gathered rows (call pg_screen_gather first)");
  if (I->q == 0) return PG_OK;
  if (!out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PG_HIP(ctx, hipMemcpyAsync(out, I->d_left, (size_t)I->q * I->n * 4, hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PG_OK;
}

extern "C" int pg_screen_gather_matched(pg_ctx* ctx, uint32_t* matched_out) {
  if (!ctx) return PG_E_ARG;
  SearchState* I = search_of(ctx);
  if (!I || !I->counted || !I->kept) return pg_fail(ctx, PG_E_ARG, "screen: the latest count kept no entries (call pg_screen_gather_count first)");
  if (I->q == 0) return PG_OK;
  if (!matched_out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PG_HIP(ctx, hipMemcpyAsync(matched_out, I->d_matched, (size_t)I->q * 4, hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PG_OK;
}

extern "C" int pg_screen_gather_last(pg_ctx* ctx, uint64_t* counts_out, double* ms_out) {
  if (!ctx || !counts_out || !ms_out) return pg_fail(ctx, PG_E_ARG, "bad argument");
  const PgScreenGatherStats& L = ctx->screen_gather_stats;
  counts_out[0] = L.entries; counts_out[1] = L.rounds; counts_out[2] = L.rows; counts_out[3] = L.claimed; counts_out[4] = L.decrements;
  ms_out[0] = L.expand_ms; ms_out[1] = L.argmax_ms; ms_out[2] = L.claim_ms;
  return PG_OK;
}
