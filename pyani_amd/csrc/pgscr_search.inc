// pgscr_search.inc — part of pg_screen.hip: the search (DESIGN.md §16.4).  A collection of n genomes stays resident as a compressed-row
// structure over ALL its distinct sampled k-mers, values included (SearchBack, the third back half of screen_front), and q new genomes
// are placed against it: hits[i][b] = |S(query i) & S(db b)|, a q x n rectangle counted per slice of the queries' keys (QueryBack: S1
// lookup, S2 weights, S3 count) and selected by the one select kernel of pgscr_select.inc (two threshold arrays, no diagonal).  The
// state names the collection's genomes by call index only and nothing in the genome arena: it outlives pg_clear_genomes.
namespace {

struct HighHalf {      // the k-mer of a key
  __host__ __device__ __forceinline__ uint32_t operator()(unsigned long long key) const { return (uint32_t)(key >> 32); }
};

constexpr unsigned long long SEARCH_ABSENT = ~0ull;      // the group of a query k-mer that no collection genome holds
constexpr uint32_t SEARCH_NO_SLICE = ~0u;                // the slice of a bin that no slice of the index covers

struct SearchState {      // the resident search index of pg_screen_search_index, the latest rectangle counted against it and its selection
  uint32_t n = 0;
  int32_t kmer = 0, scale = 0;
  uint32_t log2_scale = 0;
  uint64_t D = 0, E = 0;                          // distinct k-mers (singletons included), (k-mer, genome) entries
  PgDevBuf<uint32_t> d_kmer;                      // D: the k-mer values, ascending inside a slice
  PgDevBuf<unsigned long long> d_start;           // D + 1: k-mer g owns member[start[g], start[g + 1])
  PgDevBuf<uint32_t> d_member;                    // E: the call indices of a k-mer's holders, ascending inside a k-mer
  // the slice directory: a k-mer lies in one bin (pgscr::bin_of), a bin in at most one slice, a slice's k-mers stand back to back
  uint32_t n_slices = 0;
  PgDevBuf<unsigned long long> d_slice_first;     // n_slices + 1: the first k-mer of each slice, and D
  PgDevBuf<uint32_t> d_bin_slice;                 // N_BINS: the slice of a bin; SEARCH_NO_SLICE where there is none
  // the latest pg_screen_search_count
  bool counted = false;
  uint32_t q = 0;
  PgDevBuf<uint32_t> d_rect;                      // q x n
  // the latest pg_screen_search_select
  bool selected = false;
  uint64_t n_sel = 0;
  PgDevBuf<int32_t> d_a, d_b;
  PgDevBuf<uint32_t> d_s;
  // the gather (DESIGN.md §16.5, pgscr_gather.inc): the matched entries of the latest pg_screen_gather_count and the latest decomposition
  bool kept = false;                              // the latest count kept its entries
  uint64_t M = 0;                                 // matched (query, k-mer) entries
  PgDevBuf<unsigned long long> d_entry;           // M: query << GATHER_G_BITS | index position of the k-mer; never written after the count
  PgDevBuf<uint32_t> d_matched;                   // q: the entries of each query = |S(query) & the union of the db|
  bool gathered = false;
  uint64_t n_rows = 0;
  PgDevBuf<uint32_t> d_left;                      // q x n: what the latest pg_screen_gather left of the rectangle
  PgDevBuf<int32_t> d_row_q, d_row_db;            // n_rows each, by query, then rank
  PgDevBuf<uint32_t> d_row_unique, d_row_total;
  // the abundances (DESIGN.md §16.8, pgscr_abund.inc): what pg_screen_gather_count_abund keeps beside the entries, and the latest pass
  bool abund_kept = false;                        // the latest count kept the abundances
  PgDevBuf<uint32_t> d_abund;                     // M: a(query, k-mer) of entry e, parallel to d_entry; never written after the count
  PgDevBuf<unsigned long long> d_weight;          // q: W, the sampled occurrences of each query
  PgDevBuf<unsigned long long> d_matched_weight;  // q: MW, the abundances of each query's entries summed
  bool abund_done = false;                        // a pg_screen_gather_abund over the latest gather
  uint64_t n_abund_rows = 0;
  PgDevBuf<unsigned long long> d_ab_sum, d_ab_sumsq, d_ab_median2;      // n_rows, 2 n_rows (lo, hi), n_rows
  PgDevBuf<uint32_t> d_ab_min, d_ab_max;
  void drop_abund_rows() {      // with every new gather: the statistics are of the rows they were made from
    abund_done = false;
    n_abund_rows = 0;
    d_ab_sum.release(); d_ab_sumsq.release(); d_ab_median2.release(); d_ab_min.release(); d_ab_max.release();
  }
  void drop_gather() {
    kept = gathered = abund_kept = false;
    M = n_rows = 0;
    d_entry.release(); d_matched.release(); d_left.release(); d_row_q.release(); d_row_db.release(); d_row_unique.release(); d_row_total.release();
    d_abund.release(); d_weight.release(); d_matched_weight.release();
    drop_abund_rows();
  }
};

// Where a count leaves its matched entries (pgscr_gather.inc): prepare once by the bound, per slice one more expansion over the matched runs.
struct EntrySink {
  PgDevBuf<unsigned long long> entry;
  size_t cap = 0;
  uint64_t M = 0;
  // the abundance count (DESIGN.md §16.8): abund[e] = the multiplicity of entry e; weight, matched_weight: q sums, the caller's, zeroed
  bool weighted = false;
  PgDevBuf<uint32_t> abund;
  PgDevBuf<unsigned long long> weight, matched_weight;
};
struct QueryBack;
int gather_sink_weight(QueryBack& B, const SliceGroups& S, ScreenEvents& T);
int gather_sink_prepare(pg_ctx* ctx, EntrySink& sink, uint64_t total_keys);
int gather_sink_slice(QueryBack& B, const SliceGroups& S, ScreenEvents& T, uint32_t nr, uint32_t na);
int gather_sink_finish(pg_ctx* ctx, EntrySink& sink, uint32_t q, PgDevBuf<uint32_t>& matched, ScreenEvents& T);

// An array of the index that was sized by a bound and uses `need` elements moves into a block of exactly that many, unless the bound was
// close (within a sixteenth: E is nearly the keys when few k-mers repeat inside a genome) or there is no room for the copy: then it stays.
template <typename T>
int search_fit(pg_ctx* ctx, PgDevBuf<T>& b, size_t need) {
  if (b.cap <= need + need / 16 + 64) return PG_OK;
  PgDevBuf<T> exact;
  if (exact.reserve(need) != hipSuccess) { (void)hipGetLastError(); return PG_OK; }
  PG_HIP(ctx, hipMemcpyAsync(exact, b, need * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  b = std::move(exact);
  return PG_OK;
}

SearchState* search_of(pg_ctx* ctx) { return static_cast<SearchState*>(ctx->screen_search_state); }

// the rectangle, the selection and the gather state of an earlier count go, with their statistics: before a new count, and when the index grows
void search_drop_counted(pg_ctx* ctx, SearchState* I) {
  I->counted = I->selected = false;
  I->q = 0;
  I->n_sel = 0;
  I->d_rect.release(); I->d_a.release(); I->d_b.release(); I->d_s.release();
  I->drop_gather();
  ctx->screen_gather_stats = PgScreenGatherStats{};
  ctx->screen_gather_abund_stats = PgScreenGatherAbundStats{};
  PgScreenSearchStats& L = ctx->screen_search_stats;
  L.query_keys = L.lookups = L.matched = L.increments = L.query_slices = 0;
  L.scan_ms = L.group_ms = L.lookup_ms = L.count_ms = L.select_ms = 0.0;
}

// u: the nu distinct keys of a slice, sorted.  head[i] = entry i is the first of its k-mer (EVERY k-mer: the front's marks cover only the
// ones held by two or more genomes); member_out[i] = its genome, where an output is given.
__global__ __launch_bounds__(256) void search_mark_kernel(const unsigned long long* __restrict__ u, uint64_t nu, uint8_t* __restrict__ head,
                                                           uint32_t* __restrict__ member_out) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nu; i += (uint64_t)gridDim.x * blockDim.x) {
    const unsigned long long key = u[i];
    head[i] = (uint8_t)(i == 0 || (uint32_t)(u[i - 1] >> 32) != (uint32_t)(key >> 32) ? 1u : 0u);
    if (member_out) member_out[i] = (uint32_t)key;
  }
}

// The back half of pg_screen_search_index: per slice the k-mer values, their starts and ALL entries are appended; nothing is counted.
struct SearchBack {
  pg_ctx* ctx;
  SearchState* I;
  PgDevBuf<uint8_t> head;
  PgDevBuf<unsigned long long> d_sel;      // [0] the k-mers Flagged kept
  size_t cap = 0;
  std::vector<unsigned long long> slice_first;
  std::vector<uint32_t> bin_slice;
  int prepare(uint64_t total_keys, uint64_t slice_max, size_t, size_t& tmp_bytes) {
    cap = (size_t)total_keys;      // every entry is a distinct key, every k-mer owns one or more: E <= keys, D <= keys
    hipStream_t st = ctx->stream;
    int rc;
    if ((rc = sk_malloc(ctx, head, (size_t)slice_max + 1)) || (rc = sk_malloc(ctx, d_sel, 1))) return rc;
    if (sk_malloc(ctx, I->d_member, cap + 1) || sk_malloc(ctx, I->d_kmer, cap + 1) || sk_malloc(ctx, I->d_start, cap + 2))
      return pg_fail(ctx, PG_E_NOMEM, "screen: no device memory for a search index of up to " + std::to_string(cap) + " entries (16 bytes each while it is built)");
    hipcub::TransformInputIterator<uint32_t, HighHalf, const unsigned long long*> value((const unsigned long long*)nullptr, HighHalf{});
    hipcub::CountingInputIterator<unsigned long long> at(0ull);
    PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& b) {
      return hipcub::DeviceSelect::Flagged(nullptr, b, value, (const uint8_t*)head.p, I->d_kmer.p, d_sel.p, (int64_t)slice_max, st); }));
    PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& b) {
      return hipcub::DeviceSelect::Flagged(nullptr, b, at, (const uint8_t*)head.p, I->d_start.p, d_sel.p, (int64_t)slice_max, st); }));
    return PG_OK;
  }
  int slice(const SliceGroups& S, ScreenEvents& T) {
    hipStream_t st = ctx->stream;
    if (I->E + S.nu > cap) return pg_fail(ctx, PG_E_INTERNAL, "screen: more entries in the search index than keys");
    unsigned long long kept = 0;
    if (S.nu) {
      {
        ScreenEvents::Stage group(T, ST_GROUP, st);
        hipLaunchKernelGGL(search_mark_kernel, dim3(grid_for(S.nu, 256 * 4, (uint32_t)ctx->num_cu * 8u)), dim3(256), 0, st, S.u, S.nu, head.p, I->d_member.p + I->E);
        PG_HIP(ctx, hipGetLastError());
        // the k-mers' values, and where their entries start: the positions of the first entries, counted on from E
        hipcub::TransformInputIterator<uint32_t, HighHalf, const unsigned long long*> value(S.u, HighHalf{});
        hipcub::CountingInputIterator<unsigned long long> at((unsigned long long)I->E);
        size_t tb = S.tmp_bytes;
        PG_HIP(ctx, hipcub::DeviceSelect::Flagged(S.tmp, tb, value, (const uint8_t*)head.p, I->d_kmer.p + I->D, d_sel.p, (int64_t)S.nu, st));   // (at most nu: room by cap)
        tb = S.tmp_bytes;
        PG_HIP(ctx, hipcub::DeviceSelect::Flagged(S.tmp, tb, at, (const uint8_t*)head.p, I->d_start.p + I->D, d_sel.p, (int64_t)S.nu, st));
        PG_HIP(ctx, hipMemcpyAsync(&kept, d_sel.p, 8, hipMemcpyDeviceToHost, st));
      }
      PG_HIP(ctx, hipStreamSynchronize(st));
      if (kept < 1 || kept > S.nu) return pg_fail(ctx, PG_E_INTERNAL, "screen: a slice of " + std::to_string(S.nu) + " entries gave " + std::to_string(kept) + " k-mers");
    }
    if (S.bin_lo > S.bin_hi || S.bin_hi > pgscr::N_BINS) return pg_fail(ctx, PG_E_INTERNAL, "screen: a slice outside the bins");
    for (uint32_t bin = S.bin_lo; bin < S.bin_hi; ++bin) bin_slice[bin] = (uint32_t)slice_first.size();
    slice_first.push_back((unsigned long long)I->D);
    I->D += kept; I->E += S.nu;
    return PG_OK;
  }
};

// S1 lookup: run r = the entries [run_first[r], run_first[r + 1]) of one query k-mer (the last run ends at nu).  group[r] = the k-mer's
// position in the index or SEARCH_ABSENT; found[r] says which.
__global__ __launch_bounds__(256) void search_lookup_kernel(const unsigned long long* __restrict__ u, uint64_t nu, const uint32_t* __restrict__ run_first, uint32_t nr,
                                                             uint32_t log2_scale, const uint32_t* __restrict__ bin_slice,
                                                             const unsigned long long* __restrict__ slice_first, uint32_t n_slices,
                                                             const uint32_t* __restrict__ kmer, uint64_t D, unsigned long long* __restrict__ group,
                                                             uint8_t* __restrict__ found) {
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < nr; r += gridDim.x * blockDim.x) {
    unsigned long long g = SEARCH_ABSENT;
    const uint32_t s = run_first[r];
    if (s < nu) {
      const uint32_t canon = (uint32_t)(u[s] >> 32);
      const uint32_t sl = bin_slice[pgscr::bin_of(canon, log2_scale)];
      if (sl < n_slices) {
        const uint64_t lo = slice_first[sl], hi = slice_first[sl + 1] < D ? slice_first[sl + 1] : D;
        const uint64_t p = lo < hi ? pgscr::lower_bound_u32(kmer, lo, hi, canon) : hi;
        if (p < hi && kmer[p] == canon) g = p;
      }
    }
    group[r] = g;
    found[r] = (uint8_t)(g != SEARCH_ABSENT ? 1u : 0u);
  }
}

struct SearchWeight {      // S2: the items of the i-th matched run (active: their indices, ascending): m_q m_d
  typedef uint32_t Index;
  const uint32_t *active, *run_first;
  uint32_t nr;
  uint64_t nu, D;
  const unsigned long long *group, *start;
  __device__ unsigned long long operator()(uint32_t i) const {
    const uint32_t r = active[i];
    if (r >= nr) return 1ull;      // (never, here and below: a walked group owns an item, and the count kernel checks again)
    const unsigned long long g = group[r];
    if (g >= D) return 1ull;
    const uint64_t mq = (r + 1u < nr ? run_first[r + 1u] : nu) - run_first[r];
    return pgscr::band_items((uint32_t)mq, (uint32_t)(start[g + 1] - start[g]));
  }
};

// S3 count: the balance by item over the MATCHED runs (each owns an item or more: item_walk's window of 257 offsets holds; fewer than 2^32
// of them in a slice: the walk's searches in 32 bits).  Item t of a run -> (i, j) = (t / m_d, t % m_d): consecutive lanes run j upward
// along the row of query i.  rect[query(i) n + member[s + j]] += 1.
__global__ __launch_bounds__(256) void search_count_kernel(const unsigned long long* __restrict__ u, uint64_t nu, const uint32_t* __restrict__ run_first, uint32_t nr,
                                                            const uint32_t* __restrict__ active, const unsigned long long* __restrict__ group,
                                                            const unsigned long long* __restrict__ start, const uint32_t* __restrict__ member, uint64_t D,
                                                            uint64_t E, const unsigned long long* __restrict__ off, uint32_t na, unsigned long long P,
                                                            unsigned long long per, uint32_t q, uint32_t n, uint32_t* __restrict__ rect) {
  item_walk<uint32_t>(off, na, P, per, [=](uint32_t ga, unsigned long long t) {
    const uint32_t r = active[ga];
    if (r >= nr) return;
    const unsigned long long g = group[r];
    if (g >= D) return;
    const uint64_t sq = run_first[r], eq = r + 1u < nr ? run_first[r + 1u] : nu;
    const uint64_t s = start[g];
    const uint32_t md = (uint32_t)(start[g + 1] - s);
    if (!md) return;
    uint32_t i, j;
    pgscr::band_item_decode(t, md, &i, &j);
    if (sq + i < eq && eq <= nu && s + j < E) {
      const uint32_t qi = (uint32_t)u[sq + i], col = member[s + j];
      if (qi < q && col < n) atomicAdd(&rect[(size_t)qi * n + col], 1u);
    }
  });
}

// The back half of pg_screen_search_count: every grouped slice of the queries' keys is looked up in the index and counted into the rectangle.
struct QueryBack {
  pg_ctx* ctx;
  const SearchState* I;
  uint32_t q;
  uint32_t* d_rect;
  PgDevBuf<uint8_t> head, found;
  PgDevBuf<uint32_t> run_first, active;
  PgDevBuf<unsigned long long> group, wts, off, d_sel;
  uint64_t lookups = 0, matched = 0, incr = 0;
  EntrySink* sink = nullptr;      // the gather's count: the matched entries go here as well
  int prepare(uint64_t total_keys, uint64_t slice_max, size_t, size_t& tmp_bytes) {
    const size_t room = (size_t)slice_max + 1;
    hipStream_t st = ctx->stream;
    int rc;
    if (sink && (rc = gather_sink_prepare(ctx, *sink, total_keys))) return rc;
    if ((rc = sk_malloc(ctx, head, room)) || (rc = sk_malloc(ctx, found, room)) || (rc = sk_malloc(ctx, run_first, room)) || (rc = sk_malloc(ctx, active, room)) ||
        (rc = sk_malloc(ctx, group, room)) || (rc = sk_malloc(ctx, wts, room)) || (rc = sk_malloc(ctx, off, room)) || (rc = sk_malloc(ctx, d_sel, 1)))
      return rc;
    hipcub::CountingInputIterator<uint32_t> counting(0u);
    PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& b) {
      return hipcub::DeviceSelect::Flagged(nullptr, b, counting, (const uint8_t*)head.p, run_first.p, d_sel.p, (int64_t)slice_max, st); }));
    PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& b) { return hipcub::DeviceScan::ExclusiveSum(nullptr, b, wts.p, off.p, (int64_t)room, st); }));
    return PG_OK;
  }
  int slice(const SliceGroups& S, ScreenEvents& T) {
    if (!S.nu) return PG_OK;
    hipStream_t st = ctx->stream;
    const uint32_t cu_blocks = (uint32_t)ctx->num_cu * 8u;
    hipcub::CountingInputIterator<uint32_t> counting(0u);
    unsigned long long nr = 0, na = 0, P = 0;
    if (sink && sink->weighted) { int rc; if ((rc = gather_sink_weight(*this, S, T))) return rc; }      // (every key of the slice, matched or not)
    // Each stage is timed in pieces that end before the host waits for a count, so that no event pair spans a synchronisation: the
    // lookup stage = the mark, the runs' compaction, the lookup kernel and the matched runs' compaction; the count stage = the weights,
    // their scan and the count kernel.
    {      // the runs of the distinct query k-mers
      ScreenEvents::Stage lookup(T, ST_LOOKUP, st);
      hipLaunchKernelGGL(search_mark_kernel, dim3(grid_for(S.nu, 256 * 4, cu_blocks)), dim3(256), 0, st, S.u, S.nu, head.p, (uint32_t*)nullptr);
      PG_HIP(ctx, hipGetLastError());
      size_t tb = S.tmp_bytes;
      PG_HIP(ctx, hipcub::DeviceSelect::Flagged(S.tmp, tb, counting, (const uint8_t*)head.p, run_first.p, d_sel.p, (int64_t)S.nu, st));
    }
    PG_HIP(ctx, hipMemcpyAsync(&nr, d_sel.p, 8, hipMemcpyDeviceToHost, st));
    PG_HIP(ctx, hipStreamSynchronize(st));
    if (nr < 1 || nr > S.nu) return pg_fail(ctx, PG_E_INTERNAL, "screen: a slice of " + std::to_string(S.nu) + " query entries gave " + std::to_string(nr) + " k-mers");
    {      // each looked up; the matched ones compacted
      ScreenEvents::Stage lookup(T, ST_LOOKUP, st);
      hipLaunchKernelGGL(search_lookup_kernel, dim3(grid_for(nr, 256, cu_blocks)), dim3(256), 0, st, S.u, S.nu, (const uint32_t*)run_first.p, (uint32_t)nr, I->log2_scale,
                         (const uint32_t*)I->d_bin_slice.p, (const unsigned long long*)I->d_slice_first.p, I->n_slices, (const uint32_t*)I->d_kmer.p, I->D, group.p,
                         found.p);
      PG_HIP(ctx, hipGetLastError());
      size_t tb = S.tmp_bytes;
      PG_HIP(ctx, hipcub::DeviceSelect::Flagged(S.tmp, tb, counting, (const uint8_t*)found.p, active.p, d_sel.p, (int64_t)nr, st));
    }
    PG_HIP(ctx, hipMemcpyAsync(&na, d_sel.p, 8, hipMemcpyDeviceToHost, st));
    PG_HIP(ctx, hipStreamSynchronize(st));
    if (na > nr) return pg_fail(ctx, PG_E_INTERNAL, "screen: more matched k-mers than looked up");
    lookups += nr; matched += na;
    if (!na) return PG_OK;
    if (sink) { int rc; if ((rc = gather_sink_slice(*this, S, T, (uint32_t)nr, (uint32_t)na))) return rc; }
    {
      ScreenEvents::Stage count(T, ST_COUNT, st);
      const SearchWeight weight{active.p, run_first.p, (uint32_t)nr, S.nu, I->D, group.p, I->d_start.p};
      PG_HIP(ctx, screen_weights(ctx, na, wts.p, weight));
      size_t tb = S.tmp_bytes;
      PG_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(S.tmp, tb, wts.p, off.p, (int64_t)(na + 1), st));
    }
    PG_HIP(ctx, hipMemcpyAsync(&P, off.p + na, 8, hipMemcpyDeviceToHost, st));
    PG_HIP(ctx, hipStreamSynchronize(st));
    if (P < na) return pg_fail(ctx, PG_E_INTERNAL, "screen: fewer items than matched k-mers");
    incr += P;
    const unsigned long long per = items_per_workgroup(ctx, P);
    ScreenEvents::Stage count(T, ST_COUNT, st);
    hipLaunchKernelGGL(search_count_kernel, dim3((uint32_t)((P + per - 1) / per)), dim3(256), 0, st, S.u, S.nu, (const uint32_t*)run_first.p, (uint32_t)nr,
                       (const uint32_t*)active.p, (const unsigned long long*)group.p, (const unsigned long long*)I->d_start.p, (const uint32_t*)I->d_member.p, I->D, I->E,
                       (const unsigned long long*)off.p, (uint32_t)na, P, per, q, I->n, d_rect);
    PG_HIP(ctx, hipGetLastError());
    return PG_OK;
  }
};

}  // namespace

void pg_screen_search_drop(pg_ctx* ctx) {
  if (!ctx->screen_search_state) return;
  delete search_of(ctx);
  ctx->screen_search_state = nullptr;
  ctx->screen_search_stats = PgScreenSearchStats{};
  ctx->screen_search_add_stats = PgScreenSearchAddStats{};
  ctx->screen_search_remove_stats = PgScreenSearchRemoveStats{};
  ctx->screen_gather_stats = PgScreenGatherStats{};
  ctx->screen_gather_abund_stats = PgScreenGatherAbundStats{};
}

extern "C" int pg_screen_search_index_release(pg_ctx* ctx) {
  if (!ctx) return PG_E_ARG;
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  pg_screen_search_drop(ctx);
  return PG_OK;
}

extern "C" int pg_screen_search_last(pg_ctx* ctx, uint64_t* counts_out, double* ms_out) {
  if (!ctx || !counts_out || !ms_out) return pg_fail(ctx, PG_E_ARG, "bad argument");
  const PgScreenSearchStats& L = ctx->screen_search_stats;
  counts_out[0] = L.keys; counts_out[1] = L.kmers; counts_out[2] = L.entries; counts_out[3] = L.slices;
  counts_out[4] = L.query_keys; counts_out[5] = L.lookups; counts_out[6] = L.matched; counts_out[7] = L.increments; counts_out[8] = L.query_slices;
  counts_out[9] = L.index_bytes;
  ms_out[0] = L.index_scan_ms; ms_out[1] = L.index_group_ms;
  ms_out[2] = L.scan_ms; ms_out[3] = L.group_ms; ms_out[4] = L.lookup_ms; ms_out[5] = L.count_ms; ms_out[6] = L.select_ms;
  return PG_OK;
}

extern "C" int pg_screen_search_index(pg_ctx* ctx, const int32_t* genome_ids, uint32_t n, int32_t kmer, int32_t scale, uint32_t* sizes_out) {
  if (!ctx) return PG_E_ARG;
  int rc;
  if ((rc = screen_check(ctx, genome_ids, n, kmer, scale, 0, 1, sizes_out, false, nullptr, pgscr::INDEX_MAX_GENOMES,
                         "screen: more than 1048576 (2^20) genomes in one search index")))
    return rc;
  if ((rc = pg_screen_search_index_release(ctx))) return rc;      // the index of an earlier call goes before the new one is made: never two at a time
  if (n == 0) return PG_OK;      // (nothing to index)
  PG_HIP(ctx, hipSetDevice(ctx->device));
  if ((rc = pg_upload(ctx))) return rc;
  hipStream_t st = ctx->stream;
  std::unique_ptr<SearchState> I(new SearchState());
  I->n = n; I->kmer = kmer; I->scale = scale;
  while ((1 << I->log2_scale) < scale) ++I->log2_scale;
  ScreenEvents T;
  FrontTotals tot;
  PgDevBuf<uint32_t> d_sizes;
  std::vector<unsigned long long> slice_first;
  std::vector<uint32_t> bin_slice;
  {
    SearchBack back{ctx, I.get()};
    back.bin_slice.assign(pgscr::N_BINS, SEARCH_NO_SLICE);
    if ((rc = screen_front(ctx, genome_ids, n, kmer, scale, 0, 1, true, d_sizes, T, tot, back))) return rc;
    slice_first.swap(back.slice_first);
    bin_slice.swap(back.bin_slice);
  }      // (the slices' buffers are gone here)
  // the directory (a collection without a key has no slice at all)
  I->n_slices = (uint32_t)slice_first.size();
  slice_first.push_back((unsigned long long)I->D);
  if (!I->d_start.p && ((rc = sk_malloc(ctx, I->d_start, 1)) || (rc = sk_malloc(ctx, I->d_member, 1)) || (rc = sk_malloc(ctx, I->d_kmer, 1)))) return rc;
  if ((rc = sk_malloc(ctx, I->d_slice_first, slice_first.size())) || (rc = sk_malloc(ctx, I->d_bin_slice, pgscr::N_BINS))) return rc;
  const unsigned long long end = I->E;
  PG_HIP(ctx, hipMemcpyAsync(I->d_start.p + I->D, &end, 8, hipMemcpyHostToDevice, st));
  PG_HIP(ctx, hipMemcpyAsync(I->d_slice_first, slice_first.data(), slice_first.size() * 8, hipMemcpyHostToDevice, st));
  PG_HIP(ctx, hipMemcpyAsync(I->d_bin_slice, bin_slice.data(), (size_t)pgscr::N_BINS * 4, hipMemcpyHostToDevice, st));
  PG_HIP(ctx, hipMemcpyAsync(sizes_out, d_sizes, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipStreamSynchronize(st));
  // the arrays were sized by the keys before anything was grouped: each moves into a block of its own size (D is often under half the keys)
  if ((rc = search_fit(ctx, I->d_kmer, (size_t)I->D + 1)) || (rc = search_fit(ctx, I->d_start, (size_t)I->D + 1)) || (rc = search_fit(ctx, I->d_member, (size_t)I->E + 1)))
    return rc;
  PgScreenSearchStats& L = ctx->screen_search_stats;
  L = PgScreenSearchStats{};
  L.keys = tot.keys; L.kmers = I->D; L.entries = I->E; L.slices = tot.slices;
  L.index_bytes = 4 * (uint64_t)I->d_kmer.cap + 8 * (uint64_t)I->d_start.cap + 4 * (uint64_t)I->d_member.cap + 8 * (uint64_t)I->d_slice_first.cap + 4 * (uint64_t)I->d_bin_slice.cap;
  L.index_scan_ms = T.ms(ST_SCAN); L.index_group_ms = T.ms(ST_GROUP);
  ctx->screen_search_state = I.release();
  return PG_OK;
}

// pg_screen_search_count, pg_screen_gather_count and pg_screen_gather_count_abund: one path.  keep = KEEP_ENTRIES: the matched entries stay
// resident for pg_screen_gather; KEEP_ABUND: so do their abundances and the queries' weights, for pg_screen_gather_abund (weight_out: q
// uint64, W).
enum SearchKeep { KEEP_NONE, KEEP_ENTRIES, KEEP_ABUND };
static int search_count(pg_ctx* ctx, const int32_t* query_ids, uint32_t q, uint32_t* sizes_out, SearchKeep keep, uint64_t* weight_out = nullptr) {
  if (!ctx) return PG_E_ARG;
  SearchState* I = search_of(ctx);
  if (!I) return pg_fail(ctx, PG_E_ARG, "screen: no resident search index (call pg_screen_search_index first)");
  const uint32_t rows = pgscr::search_rows(ctx->screen_band_rows, I->n);
  const std::string too_many = "screen: " + std::to_string(q) + " queries in one count, more than the band's " + std::to_string(rows) + " rows (pg_screen_set_band)";
  int rc;
  if ((rc = screen_check(ctx, query_ids, q, I->kmer, I->scale, 0, 1, sizes_out, false, nullptr, rows, too_many.c_str()))) return rc;
  if (keep == KEEP_ABUND && q && !weight_out) return pg_fail(ctx, PG_E_ARG, "bad argument");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  search_drop_counted(ctx, I);      // the rectangle and the selection of an earlier count go before the new one is made
  PgScreenSearchStats& L = ctx->screen_search_stats;
  if (q == 0) { I->q = 0; I->counted = true; I->kept = keep != KEEP_NONE; I->abund_kept = keep == KEEP_ABUND; return PG_OK; }      // (a rectangle of no rows)
  if ((rc = pg_upload(ctx))) return rc;
  hipStream_t st = ctx->stream;
  PgDevBuf<uint32_t> rect, d_sizes;
  if ((rc = pg_dev_alloc(ctx, "screen", rect, (size_t)q * I->n, "the rectangle of a search"))) return rc;
  PG_HIP(ctx, hipMemsetAsync(rect, 0, (size_t)q * I->n * 4, st));
  ScreenEvents T;
  FrontTotals tot;
  EntrySink sink;
  QueryBack back{ctx, I, q, rect.p};
  if (keep) back.sink = &sink;
  if (keep == KEEP_ABUND) {
    sink.weighted = true;
    if ((rc = pg_dev_alloc(ctx, "screen", sink.weight, q, "the queries' weights")) || (rc = pg_dev_alloc(ctx, "screen", sink.matched_weight, q, "the queries' weights"))) return rc;
    PG_HIP(ctx, hipMemsetAsync(sink.weight, 0, (size_t)q * 8, st));
    PG_HIP(ctx, hipMemsetAsync(sink.matched_weight, 0, (size_t)q * 8, st));
  }
  PgDevBuf<uint32_t> matched;
  rc = screen_front(ctx, query_ids, q, I->kmer, I->scale, 0, 1, false, d_sizes, T, tot, back, keep == KEEP_ABUND);
  if (!rc && keep) rc = gather_sink_finish(ctx, sink, q, matched, T);
  hipError_t e = rc ? hipSuccess : hipMemcpyAsync(sizes_out, d_sizes, (size_t)q * 4, hipMemcpyDeviceToHost, st);
  if (!rc && e == hipSuccess && keep == KEEP_ABUND) e = hipMemcpyAsync(weight_out, sink.weight, (size_t)q * 8, hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);      // (on errors too: the back half's buffers and `rect` go with this scope)
  if (rc) return rc;
  PG_HIP(ctx, e);
  PG_HIP(ctx, es);
  if (keep == KEEP_ABUND) {      // every key the fill pass appended is an occurrence of exactly one query
    unsigned long long all = 0;
    for (uint32_t i = 0; i < q; ++i) all += weight_out[i];
    if (all != tot.keys) return pg_fail(ctx, PG_E_INTERNAL, "screen: the queries' weights add up to " + std::to_string(all) + " where the scan took " + std::to_string(tot.keys) + " keys");
  }
  L.query_keys = tot.keys; L.lookups = back.lookups; L.matched = back.matched; L.increments = back.incr; L.query_slices = tot.slices;
  L.scan_ms = T.ms(ST_SCAN); L.group_ms = T.ms(ST_GROUP); L.lookup_ms = T.ms(ST_LOOKUP); L.count_ms = T.ms(ST_COUNT);
  I->d_rect = std::move(rect);
  I->q = q;
  I->counted = true;
  if (keep) {
    I->kept = true;
    I->M = sink.M;
    I->d_entry = std::move(sink.entry);
    I->d_matched = std::move(matched);
    ctx->screen_gather_stats.entries = sink.M;
    ctx->screen_gather_stats.expand_ms = T.ms(ST_EXPAND);
  }
  if (keep == KEEP_ABUND) {
    I->abund_kept = true;
    I->d_abund = std::move(sink.abund);
    I->d_weight = std::move(sink.weight);
    I->d_matched_weight = std::move(sink.matched_weight);
    ctx->screen_gather_abund_stats.weight_ms = T.ms(ST_WEIGHT);
  }
  return PG_OK;
}

extern "C" int pg_screen_search_count(pg_ctx* ctx, const int32_t* query_ids, uint32_t q, uint32_t* sizes_out) {
  return search_count(ctx, query_ids, q, sizes_out, KEEP_NONE);
}

extern "C" int pg_screen_search_fetch(pg_ctx* ctx, uint32_t* out) {
  if (!ctx) return PG_E_ARG;
  SearchState* I = search_of(ctx);
  if (!I) return pg_fail(ctx, PG_E_ARG, "screen: no resident search index (call pg_screen_search_index first)");
  if (!I->counted) return pg_fail(ctx, PG_E_ARG, "screen: no counted rectangle (call pg_screen_search_count first)");
  if (I->q == 0) return PG_OK;
  if (!out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PG_HIP(ctx, hipMemcpyAsync(out, I->d_rect, (size_t)I->q * I->n * 4, hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PG_OK;
}

extern "C" int pg_screen_search_select(pg_ctx* ctx, const uint32_t* need_q, uint32_t q, const uint32_t* need_db, uint32_t n, uint64_t* n_pairs_out) {
  if (!ctx) return PG_E_ARG;
  SearchState* I = search_of(ctx);
  if (!I) return pg_fail(ctx, PG_E_ARG, "screen: no resident search index (call pg_screen_search_index first)");
  if (!I->counted) return pg_fail(ctx, PG_E_ARG, "screen: no counted rectangle (call pg_screen_search_count first)");
  if (n != I->n) return pg_fail(ctx, PG_E_ARG, "screen: the resident search index is of " + std::to_string(I->n) + " genomes, not " + std::to_string(n));
  if (q != I->q) return pg_fail(ctx, PG_E_ARG, "screen: the counted rectangle is of " + std::to_string(I->q) + " queries, not " + std::to_string(q));
  if ((q && !need_q) || !need_db || !n_pairs_out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  I->selected = false;
  I->n_sel = 0;
  ctx->screen_search_stats.select_ms = 0.0;
  unsigned long long total = 0;
  if (q) {
    SelectWork W;
    PgDevBuf<uint32_t> d_need_q;
    PgDevBuf<uint8_t> tmp;
    size_t tmp_bytes = 0;
    ScreenEvents T;
    int rc;
    if ((rc = select_alloc(ctx, n, q, W, tmp_bytes)) || (rc = pg_dev_alloc(ctx, "screen", d_need_q, q, "the queries' thresholds")) ||
        (rc = pg_dev_alloc(ctx, "screen", tmp, tmp_bytes + 16, "the scan's temporary storage")))
      return rc;
    const auto run = [&]() -> int {
      PG_HIP(ctx, hipMemcpyAsync(W.need, need_db, (size_t)n * 4, hipMemcpyHostToDevice, st));
      PG_HIP(ctx, hipMemcpyAsync(d_need_q, need_q, (size_t)q * 4, hipMemcpyHostToDevice, st));
      ScreenEvents::Stage select(T, ST_SELECT, st);
      return select_rows(ctx, I->d_rect.p, (const uint32_t*)d_need_q.p, false, n, 0, q, W, (void*)tmp.p, tmp_bytes, I->d_a, I->d_b, I->d_s, &total);
    };
    rc = run();
    const hipError_t e = hipStreamSynchronize(st);      // (W goes with this scope; the caller's arrays may still be read)
    if (rc) return rc;
    PG_HIP(ctx, e);
    ctx->screen_search_stats.select_ms = T.ms(ST_SELECT);
  }
  I->selected = true;
  I->n_sel = total;
  *n_pairs_out = total;
  return PG_OK;
}

extern "C" int pg_screen_search_read(pg_ctx* ctx, int32_t* a_out, int32_t* b_out, uint32_t* shared_out) {
  if (!ctx) return PG_E_ARG;
  SearchState* I = search_of(ctx);
  if (!I || !I->selected) return pg_fail(ctx, PG_E_ARG, "screen: no selection over a search (call pg_screen_search_select first)");
  if (I->n_sel == 0) return PG_OK;
  if (!a_out || !b_out || !shared_out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PG_HIP(ctx, hipMemcpyAsync(a_out, I->d_a, I->n_sel * 4, hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipMemcpyAsync(b_out, I->d_b, I->n_sel * 4, hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipMemcpyAsync(shared_out, I->d_s, I->n_sel * 4, hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PG_OK;
}
