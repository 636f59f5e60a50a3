// pgscr_index.inc — part of pg_screen.hip: the screen index and its bands (DESIGN.md §16.2).  The groups stay resident in compressed-row
// form (IndexBack, the second back half of screen_front); the matrix is formed a band of rows at a time (B1 ... B4: band_fill) and
// selected there (B5: select_rows of pgscr_select.inc); band_loop is the one loop over the bands of a call.
namespace {

struct LowHalf {      // the genome of a key
  __host__ __device__ __forceinline__ uint32_t operator()(unsigned long long key) const { return (uint32_t)key; }
};
struct NonZero {
  __host__ __device__ __forceinline__ uint8_t operator()(uint32_t x) const { return x ? 1 : 0; }
};

struct SizeWeight {      // the members of slice group g: the input of the scan that continues group_start
  typedef uint32_t Index;
  const uint32_t *first, *last;
  __device__ unsigned long long operator()(uint32_t g) const { return last[g] - first[g] + 1u; }
};

// B1 prep: the members of every group that fall into the rows [r0, r1) — they ascend: two binary searches.  lo[g] = the first of them,
// counted from the group's start; mb[g] = how many.  in_band[0] += the sum of mb (one 64-bit atomic per wave).
__global__ __launch_bounds__(256) void band_prep_kernel(const unsigned long long* __restrict__ start, const uint32_t* __restrict__ member, uint64_t G,
                                                         uint32_t r0, uint32_t r1, uint32_t* __restrict__ lo, uint32_t* __restrict__ mb,
                                                         unsigned long long* __restrict__ in_band) {
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < G; base += (uint64_t)gridDim.x * blockDim.x) {      // (uniform: every lane reaches the shuffles)
    const uint64_t g = base + threadIdx.x;
    uint32_t mine = 0;
    if (g < G) {
      const uint64_t s = start[g], e = start[g + 1];
      const uint64_t a = pgscr::lower_bound_u32(member, s, e, r0);
      const uint64_t b = pgscr::lower_bound_u32(member, a, e, r1);
      lo[g] = (uint32_t)(a - s);
      mb[g] = mine = (uint32_t)(b - a);
    }
    for (int d = 32; d > 0; d >>= 1) mine += __shfl_down(mine, d, 64);      // (at most 64 x 8192)
    if ((threadIdx.x & 63u) == 0u && mine) atomicAdd(in_band, (unsigned long long)mine);
  }
}

struct BandWeight {      // B2: the items of the i-th group with a member in the band (active: their indices, ascending): mb m
  typedef uint64_t Index;
  const unsigned long long *active, *start;
  const uint32_t* mb;
  __device__ unsigned long long operator()(uint64_t i) const { const uint64_t g = active[i]; return pgscr::band_items(mb[g], (uint32_t)(start[g + 1] - start[g])); }
};

// B3 count: the balance by item over the ACTIVE groups (each owns an item or more: item_walk's window of 257 offsets holds).  Item t of a
// group -> (i, j) = (t / m, t % m): band[(member[lo + i] - r0) n + member[s + j]] += 1; the cell of a genome with itself is left to
// band_diag_kernel.
__global__ __launch_bounds__(256) void band_count_kernel(const unsigned long long* __restrict__ start, const uint32_t* __restrict__ member,
                                                          const unsigned long long* __restrict__ active, const uint32_t* __restrict__ lo,
                                                          const unsigned long long* __restrict__ off, uint64_t na, unsigned long long P, unsigned long long per,
                                                          uint32_t n, uint32_t r0, uint32_t r1, uint32_t* __restrict__ band) {
  item_walk<uint64_t>(off, na, P, per, [=](uint64_t ga, unsigned long long t) {
    const uint64_t g = active[ga];
    const uint64_t s = start[g];
    const uint32_t m = (uint32_t)(start[g + 1] - s);
    uint32_t i, j;
    pgscr::band_item_decode(t, m, &i, &j);
    const uint64_t pi = s + lo[g] + i;
    if (pi < s + m) {
      const uint32_t gi = member[pi], gj = member[s + j];
      if (gi >= r0 && gi < r1 && gj < n && gi != gj) atomicAdd(&band[(size_t)(gi - r0) * n + gj], 1u);
    }
  });
}

// B4 the diagonal: the cell of row genome a with column genome a = sizes[a]
__global__ __launch_bounds__(256) void band_diag_kernel(uint32_t* __restrict__ band, const uint32_t* __restrict__ sizes, uint32_t r0, uint32_t r1, uint32_t n) {
  for (uint32_t r = r0 + blockIdx.x * blockDim.x + threadIdx.x; r < r1; r += gridDim.x * blockDim.x) band[(size_t)(r - r0) * n + r] = sizes[r];
}

struct IndexState {      // the resident k-mer index of pg_screen_index and the latest selection over it
  uint32_t n = 0;
  uint64_t G = 0, E = 0;                        // groups (k-mers held by >= 2 genomes), grouped entries
  PgDevBuf<unsigned long long> d_start;         // group_start: G + 1
  PgDevBuf<uint32_t> d_member;                  // E: the call indices of a group's genomes, ascending inside a group
  PgDevBuf<uint32_t> d_sizes;                   // n
  bool selected = false;
  std::vector<int32_t> a, b;                    // the kept triples of the latest pg_screen_index_select, on the host: bands go as they finish
  std::vector<uint32_t> s;
};

IndexState* index_of(pg_ctx* ctx) { return static_cast<IndexState*>(ctx->screen_index_state); }

// The back half of pg_screen_index: the grouped entries of every slice are appended to group_start / member; nothing is counted.
struct IndexBack {
  pg_ctx* ctx;
  IndexState* I;
  PgDevBuf<unsigned long long> wts, d_sel;      // the groups' sizes of a slice | [0] the entries Flagged kept
  size_t cap_groups = 0, cap_entries = 0;
  int prepare(uint64_t total_keys, uint64_t slice_max, size_t max_groups, size_t& tmp_bytes) {
    // every grouped entry is a distinct key and every group holds two of them or more: E <= keys, G <= keys / 2
    cap_entries = (size_t)total_keys;
    cap_groups = (size_t)(total_keys / 2);
    hipStream_t st = ctx->stream;
    int rc;
    if ((rc = sk_malloc(ctx, wts, max_groups)) || (rc = sk_malloc(ctx, d_sel, 1))) return rc;
    if (sk_malloc(ctx, I->d_member, cap_entries + 1) || sk_malloc(ctx, I->d_start, cap_groups + 2))
      return pg_fail(ctx, PG_E_NOMEM, "screen: no device memory for an index of up to " + std::to_string(cap_entries) + " entries (4 bytes each) in " +
                                          std::to_string(cap_groups) + " groups (8 bytes each)");
    PG_HIP(ctx, hipMemsetAsync(I->d_start, 0, 8, st));
    hipcub::TransformInputIterator<uint32_t, LowHalf, const unsigned long long*> genome((const unsigned long long*)nullptr, LowHalf{});
    hipcub::TransformInputIterator<uint8_t, FlagBit, const uint8_t*> grouped((const uint8_t*)nullptr, FlagBit{2u});
    PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& b) { return hipcub::DeviceSelect::Flagged(nullptr, b, genome, grouped, I->d_member.p, d_sel.p, (int64_t)slice_max, st); }));
    PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& b) {
      return hipcub::DeviceScan::ExclusiveScan(nullptr, b, wts.p, I->d_start.p, hipcub::Sum(), 0ull, (int64_t)max_groups, st); }));
    return PG_OK;
  }
  int slice(const SliceGroups& S, ScreenEvents& T) {
    if (!S.ng) return PG_OK;
    hipStream_t st = ctx->stream;
    if (I->G + S.ng > cap_groups) return pg_fail(ctx, PG_E_INTERNAL, "screen: more groups than half the keys");
    unsigned long long kept = 0, end = 0;
    {
      ScreenEvents::Stage group(T, ST_GROUP, st);
      // group_start continues at E: the slice's group sizes scanned from there; the entry after the last group is the next slice's first
      PG_HIP(ctx, screen_weights(ctx, S.ng, wts.p, SizeWeight{S.first, S.last}));
      size_t tb = S.tmp_bytes;
      PG_HIP(ctx, hipcub::DeviceScan::ExclusiveScan(S.tmp, tb, wts.p, I->d_start.p + I->G, hipcub::Sum(), (unsigned long long)I->E, (int64_t)(S.ng + 1), st));
      // member: the genomes of the grouped entries, in key order (inside a group the call index ascends: it is the low half of the key)
      hipcub::TransformInputIterator<uint32_t, LowHalf, const unsigned long long*> genome(S.u, LowHalf{});
      hipcub::TransformInputIterator<uint8_t, FlagBit, const uint8_t*> grouped(S.flags, FlagBit{2u});
      tb = S.tmp_bytes;
      PG_HIP(ctx, hipcub::DeviceSelect::Flagged(S.tmp, tb, genome, grouped, I->d_member.p + I->E, d_sel.p, (int64_t)S.nu, st));   // (at most nu <= the slice's keys: room by cap_entries)
      PG_HIP(ctx, hipMemcpyAsync(&kept, d_sel.p, 8, hipMemcpyDeviceToHost, st));
      PG_HIP(ctx, hipMemcpyAsync(&end, I->d_start.p + I->G + S.ng, 8, hipMemcpyDeviceToHost, st));
    }
    PG_HIP(ctx, hipStreamSynchronize(st));
    if (end != I->E + kept || I->E + kept > cap_entries)
      return pg_fail(ctx, PG_E_INTERNAL, "screen: the index took " + std::to_string(kept) + " entries of a slice whose groups hold " + std::to_string(end - I->E));
    I->G += S.ng; I->E += kept;
    return PG_OK;
  }
};

// the band setting of the context against an index of n genomes
uint32_t rows_for(const pg_ctx* ctx, uint32_t n) { return pgscr::band_rows(ctx->screen_band_rows, n); }

struct BandWork {      // the device buffers of the band calls: one band and what prep, count and select need beside it
  PgDevBuf<uint32_t> band, lo, mb, s;
  PgDevBuf<unsigned long long> active, wts, off, counters;      // counters: [0] active groups, [1] members in the band
  SelectWork sel;
  PgDevBuf<int32_t> a, b;      // a, b, s: the kept triples of the latest band
  PgDevBuf<uint8_t> tmp;
  size_t tmp_bytes = 0;
};

// (pg_dev_alloc, not sk_malloc: the band calls leave the resident matrix of pg_screen_hold / _load alone, however short memory is)
int band_alloc(pg_ctx* ctx, const IndexState* I, uint32_t rows, bool select, BandWork& W) {
  hipStream_t st = ctx->stream;
  const size_t G = (size_t)I->G;
  int rc;
  if ((rc = pg_dev_alloc(ctx, "screen", W.band, (size_t)rows * I->n, "a band of the index")) || (rc = pg_dev_alloc(ctx, "screen", W.lo, G, "the band's group ranges")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.mb, G, "the band's group ranges")) || (rc = pg_dev_alloc(ctx, "screen", W.active, G, "the band's groups")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.wts, G + 1, "the band's group weights")) || (rc = pg_dev_alloc(ctx, "screen", W.off, G + 1, "the band's item offsets")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.counters, 2, "the band's counters")))
    return rc;
  hipcub::CountingInputIterator<unsigned long long> counting(0ull);
  hipcub::TransformInputIterator<uint8_t, NonZero, const uint32_t*> has((const uint32_t*)W.mb.p, NonZero{});
  PG_HIP(ctx, tmp_room(W.tmp_bytes, [&](size_t& b) { return hipcub::DeviceSelect::Flagged(nullptr, b, counting, has, W.active.p, W.counters.p, (int64_t)G, st); }));
  PG_HIP(ctx, tmp_room(W.tmp_bytes, [&](size_t& b) { return hipcub::DeviceScan::ExclusiveSum(nullptr, b, W.wts.p, W.off.p, (int64_t)G + 1, st); }));
  if (select && (rc = select_alloc(ctx, I->n, rows, W.sel, W.tmp_bytes))) return rc;
  return pg_dev_alloc(ctx, "screen", W.tmp, W.tmp_bytes + 16, "the library calls' temporary storage");
}

// B1 ... B4: the rows [r0, r1) of the matrix in W.band, the diagonal included.  *incr += the increments of the count kernel.
int band_fill(pg_ctx* ctx, const IndexState* I, uint32_t r0, uint32_t r1, BandWork& W, uint64_t* incr) {
  hipStream_t st = ctx->stream;
  const uint32_t n = I->n, cu_blocks = (uint32_t)ctx->num_cu * 8u;
  PG_HIP(ctx, hipMemsetAsync(W.band, 0, (size_t)(r1 - r0) * n * 4, st));
  if (I->G) {
    PG_HIP(ctx, hipMemsetAsync(W.counters, 0, 2 * 8, st));
    hipLaunchKernelGGL(band_prep_kernel, dim3(grid_for(I->G, 256, cu_blocks)), dim3(256), 0, st, (const unsigned long long*)I->d_start.p, (const uint32_t*)I->d_member.p,
                       I->G, r0, r1, W.lo.p, W.mb.p, W.counters.p + 1);
    PG_HIP(ctx, hipGetLastError());
    hipcub::CountingInputIterator<unsigned long long> counting(0ull);
    hipcub::TransformInputIterator<uint8_t, NonZero, const uint32_t*> has((const uint32_t*)W.mb.p, NonZero{});
    size_t tb = W.tmp_bytes;
    PG_HIP(ctx, hipcub::DeviceSelect::Flagged((void*)W.tmp.p, tb, counting, has, W.active.p, W.counters.p, (int64_t)I->G, st));
    unsigned long long members[2] = {0, 0};      // active groups, members in the band
    PG_HIP(ctx, hipMemcpyAsync(members, W.counters, 2 * 8, hipMemcpyDeviceToHost, st));
    PG_HIP(ctx, hipStreamSynchronize(st));
    const uint64_t na = members[0];
    if (na > I->G) return pg_fail(ctx, PG_E_INTERNAL, "screen: more groups in a band than in the index");
    if (na) {
      unsigned long long P = 0;
      PG_HIP(ctx, screen_weights(ctx, na, W.wts.p, BandWeight{W.active.p, I->d_start.p, W.mb.p}));
      tb = W.tmp_bytes;
      PG_HIP(ctx, hipcub::DeviceScan::ExclusiveSum((void*)W.tmp.p, tb, W.wts.p, W.off.p, (int64_t)(na + 1), st));
      PG_HIP(ctx, hipMemcpyAsync(&P, W.off.p + na, 8, hipMemcpyDeviceToHost, st));
      PG_HIP(ctx, hipStreamSynchronize(st));
      if (P < members[1]) return pg_fail(ctx, PG_E_INTERNAL, "screen: fewer items in a band than members");
      *incr += P - members[1];      // every member of the band meets itself once among its group's items: no increment (band_count_kernel)
      const unsigned long long per = items_per_workgroup(ctx, P);
      hipLaunchKernelGGL(band_count_kernel, dim3((uint32_t)((P + per - 1) / per)), dim3(256), 0, st, (const unsigned long long*)I->d_start.p,
                         (const uint32_t*)I->d_member.p, (const unsigned long long*)W.active.p, (const uint32_t*)W.lo.p, (const unsigned long long*)W.off.p, na, P, per,
                         n, r0, r1, W.band.p);
      PG_HIP(ctx, hipGetLastError());
    }
  }
  hipLaunchKernelGGL(band_diag_kernel, dim3(grid_for(r1 - r0, 256, cu_blocks)), dim3(256), 0, st, W.band.p, (const uint32_t*)I->d_sizes.p, r0, r1, n);
  PG_HIP(ctx, hipGetLastError());
  return PG_OK;
}

// The argument checks that pg_screen_index_select and pg_screen_index_components share (outs: the call's own output pointers are there).
// They stand apart from band_loop because each caller has work of its own between the two.  *I_out = the resident index.
int band_check(pg_ctx* ctx, const uint32_t* need, uint32_t n, uint32_t band_step, bool outs, IndexState** I_out) {
  IndexState* I = index_of(ctx);
  if (!I) return pg_fail(ctx, PG_E_ARG, "screen: no resident index (call pg_screen_index first)");
  if (n != I->n) return pg_fail(ctx, PG_E_ARG, "screen: the resident index is of " + std::to_string(I->n) + " genomes, not " + std::to_string(n));
  if (band_step < 1) return pg_fail(ctx, PG_E_ARG, "screen: band_step must be 1 or more");
  if (!need || !outs) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  *I_out = I;
  return PG_OK;
}

struct BandStages {      // the stage that B1 ... B4, B5 and the caller's work on a band are timed under
  ScreenStage fill, select, work;
  bool wait;             // the stream is waited for after every band's work, outside its stage (what the work queued must land before the next band)
};
struct BandTotals { uint64_t bands = 0, incr = 0, kept = 0; };      // bands worked, increments of the count kernel, kept triples

// The ONE loop over the bands band_first, band_first + band_step, ... of the resident index (arguments checked: band_check): the band's
// rows counted (band_fill) and selected by `need` (select_rows); then work(r0, r1, total, W) with the band's `total` kept triples in W.a,
// W.b, W.s, row-major, the fill pass queued on the stream — work may queue behind it or wait.  The stream is idle when this returns.
//
// The rule of the error paths, for band_loop and its two callers: the device buffers need no wait — ~PgDevBuf is hipFree, which waits for
// the device before it frees.  Host memory that a queued copy may still touch does: the caller's `need` and what `work` copies into.  So
// band_loop waits for the stream once, on its way out, whatever the loop returned, and the callers wait nowhere after an error.
template <typename Work>
int band_loop(pg_ctx* ctx, const IndexState* I, const uint32_t* need, uint32_t band_first, uint32_t band_step, ScreenEvents& T, BandStages stages, BandTotals& tot,
              Work work) {
  PG_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const uint32_t n = I->n, rows = rows_for(ctx, n), n_bands = pgscr::band_count(n, rows);
  if (band_first >= n_bands) return PG_OK;
  BandWork W;
  const auto bands = [&]() -> int {
    int rc;
    if ((rc = band_alloc(ctx, I, std::min(rows, n), true, W))) return rc;
    PG_HIP(ctx, hipMemcpyAsync(W.sel.need, need, (size_t)n * 4, hipMemcpyHostToDevice, st));
    for (uint64_t band = band_first; band < n_bands; band += band_step) {
      uint32_t r0, r1;
      pgscr::band_range((uint32_t)band, rows, n, &r0, &r1);
      unsigned long long total = 0;
      { ScreenEvents::Stage fill(T, stages.fill, st); rc = band_fill(ctx, I, r0, r1, W, &tot.incr); }
      if (rc) return rc;
      { ScreenEvents::Stage select(T, stages.select, st); rc = select_rows(ctx, W.band.p, (const uint32_t*)W.sel.need.p, true, n, r0, r1 - r0, W.sel, (void*)W.tmp.p, W.tmp_bytes, W.a, W.b, W.s, &total); }
      if (rc) return rc;
      { ScreenEvents::Stage working(T, stages.work, st); rc = work(r0, r1, total, W); }
      if (rc) return rc;
      if (stages.wait) PG_HIP(ctx, hipStreamSynchronize(st));
      ++tot.bands;
      tot.kept += total;
    }
    return PG_OK;
  };
  const int rc = bands();
  const hipError_t e = hipStreamSynchronize(st);      // (W goes with this scope, and see above)
  if (rc) return rc;
  PG_HIP(ctx, e);
  return PG_OK;
}

}  // namespace

void pg_screen_index_drop(pg_ctx* ctx) {
  if (!ctx->screen_index_state) return;
  delete index_of(ctx);
  ctx->screen_index_state = nullptr;
}

extern "C" int pg_screen_index_release(pg_ctx* ctx) {
  if (!ctx) return PG_E_ARG;
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  pg_screen_index_drop(ctx);
  return PG_OK;
}

extern "C" int pg_screen_set_band(pg_ctx* ctx, uint32_t rows) {
  if (!ctx) return PG_E_ARG;
  if (rows > pgscr::MAX_BAND_ROWS) return pg_fail(ctx, PG_E_ARG, "screen: a band is of at most 8192 rows");
  ctx->screen_band_rows = rows;
  return PG_OK;
}

extern "C" int pg_screen_index_last(pg_ctx* ctx, uint64_t* counts_out, double* ms_out) {
  if (!ctx || !counts_out || !ms_out) return pg_fail(ctx, PG_E_ARG, "bad argument");
  const PgScreenIndexStats& L = ctx->screen_index_stats;
  counts_out[0] = L.keys; counts_out[1] = L.distinct; counts_out[2] = L.entries; counts_out[3] = L.groups; counts_out[4] = L.slices;
  counts_out[5] = L.bands; counts_out[6] = L.pair_increments;
  ms_out[0] = L.scan_ms; ms_out[1] = L.group_ms; ms_out[2] = L.count_ms; ms_out[3] = L.select_ms;
  return PG_OK;
}

extern "C" int pg_screen_index(pg_ctx* ctx, const int32_t* genome_ids, uint32_t n, int32_t kmer, int32_t scale, uint32_t* sizes_out) {
  if (!ctx) return PG_E_ARG;
  int rc;
  if ((rc = screen_check(ctx, genome_ids, n, kmer, scale, 0, 1, sizes_out, false, nullptr, pgscr::INDEX_MAX_GENOMES,
                         "screen: more than 1048576 (2^20) genomes in one index")))
    return rc;
  if ((rc = pg_screen_index_release(ctx))) return rc;      // the index of an earlier call goes before the new one is made: never two at a time
  ctx->screen_index_stats = PgScreenIndexStats{};
  if (n == 0) return PG_OK;      // (nothing to index)
  PG_HIP(ctx, hipSetDevice(ctx->device));
  if ((rc = pg_upload(ctx))) return rc;
  hipStream_t st = ctx->stream;
  std::unique_ptr<IndexState> I(new IndexState());
  I->n = n;
  ScreenEvents T;
  FrontTotals tot;
  {
    IndexBack back{ctx, I.get()};
    if ((rc = screen_front(ctx, genome_ids, n, kmer, scale, 0, 1, true, I->d_sizes, T, tot, back))) return rc;
  }      // (the slices' buffers are gone here)
  if (!I->d_start.p) {      // no slice at all: an index without groups
    if ((rc = sk_malloc(ctx, I->d_start, 1)) || (rc = sk_malloc(ctx, I->d_member, 1))) return rc;
    PG_HIP(ctx, hipMemsetAsync(I->d_start, 0, 8, st));
  }
  PG_HIP(ctx, hipMemcpyAsync(sizes_out, I->d_sizes, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipStreamSynchronize(st));
  // the arrays were sized by the keys before anything was grouped: an index that is much smaller moves into blocks of its own size
  if (I->d_member.cap > 2 * (size_t)I->E + 1024) {
    PgDevBuf<uint32_t> m;
    PgDevBuf<unsigned long long> s;
    if (m.reserve((size_t)I->E + 1) == hipSuccess && s.reserve((size_t)I->G + 1) == hipSuccess) {
      PG_HIP(ctx, hipMemcpyAsync(m, I->d_member, (size_t)I->E * 4, hipMemcpyDeviceToDevice, st));
      PG_HIP(ctx, hipMemcpyAsync(s, I->d_start, ((size_t)I->G + 1) * 8, hipMemcpyDeviceToDevice, st));
      PG_HIP(ctx, hipStreamSynchronize(st));
      I->d_member = std::move(m); I->d_start = std::move(s);
    } else {
      (void)hipGetLastError();      // (no room for the copy: the index stays where it is)
    }
  }
  PgScreenIndexStats& L = ctx->screen_index_stats;
  L.keys = tot.keys; L.distinct = tot.distinct; L.entries = I->E; L.groups = I->G; L.slices = tot.slices;
  L.scan_ms = T.ms(ST_SCAN); L.group_ms = T.ms(ST_GROUP);
  ctx->screen_index_state = I.release();
  return PG_OK;
}

extern "C" int pg_screen_index_band(pg_ctx* ctx, uint32_t band, uint32_t* out) {
  if (!ctx) return PG_E_ARG;
  IndexState* I = index_of(ctx);
  if (!I) return pg_fail(ctx, PG_E_ARG, "screen: no resident index (call pg_screen_index first)");
  const uint32_t rows = rows_for(ctx, I->n), n_bands = pgscr::band_count(I->n, rows);
  if (band >= n_bands) return pg_fail(ctx, PG_E_ARG, "screen: band " + std::to_string(band) + " does not exist (the index has " + std::to_string(n_bands) + " bands of " +
                                                         std::to_string(rows) + " rows)");
  if (!out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  uint32_t r0, r1;
  pgscr::band_range(band, rows, I->n, &r0, &r1);
  BandWork W;
  uint64_t incr = 0;
  int rc;
  if ((rc = band_alloc(ctx, I, r1 - r0, false, W)) || (rc = band_fill(ctx, I, r0, r1, W, &incr))) return rc;
  PG_HIP(ctx, hipMemcpyAsync(out, W.band, (size_t)(r1 - r0) * I->n * 4, hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PG_OK;
}

extern "C" int pg_screen_index_select(pg_ctx* ctx, const uint32_t* need, uint32_t n, uint32_t band_first, uint32_t band_step, uint64_t* n_pairs_out) {
  if (!ctx) return PG_E_ARG;
  IndexState* I = nullptr;
  int rc;
  if ((rc = band_check(ctx, need, n, band_step, n_pairs_out != nullptr, &I))) return rc;
  PgScreenIndexStats& L = ctx->screen_index_stats;
  I->selected = false;
  I->a.clear(); I->b.clear(); I->s.clear();
  L.bands = L.pair_increments = 0;
  L.count_ms = L.select_ms = 0.0;
  hipStream_t st = ctx->stream;
  ScreenEvents T;
  BandTotals tot;
  // the band's triples go to the host as it finishes: the device never holds more than one band (waited for: the next band moves the vectors)
  const BandStages stages{ST_COUNT, ST_SELECT, ST_SELECT, true};
  rc = band_loop(ctx, I, need, band_first, band_step, T, stages, tot, [&](uint32_t, uint32_t, unsigned long long total, BandWork& W) -> int {
    if (!total) return PG_OK;
    const size_t at = I->a.size();
    try {
      I->a.resize(at + total); I->b.resize(at + total); I->s.resize(at + total);
    } catch (const std::bad_alloc&) {
      I->a.clear(); I->b.clear(); I->s.clear();
      return pg_fail(ctx, PG_E_NOMEM, "screen: no host memory for " + std::to_string(at + total) + " selected pairs");
    }
    PG_HIP(ctx, hipMemcpyAsync(I->a.data() + at, W.a, (size_t)total * 4, hipMemcpyDeviceToHost, st));
    PG_HIP(ctx, hipMemcpyAsync(I->b.data() + at, W.b, (size_t)total * 4, hipMemcpyDeviceToHost, st));
    PG_HIP(ctx, hipMemcpyAsync(I->s.data() + at, W.s, (size_t)total * 4, hipMemcpyDeviceToHost, st));
    return PG_OK;
  });
  if (rc) return rc;
  L.bands = tot.bands; L.pair_increments = tot.incr;
  L.count_ms = T.ms(ST_COUNT); L.select_ms = T.ms(ST_SELECT);
  I->selected = true;
  *n_pairs_out = I->a.size();
  return PG_OK;
}

extern "C" int pg_screen_index_read(pg_ctx* ctx, int32_t* a_out, int32_t* b_out, uint32_t* shared_out) {
  if (!ctx) return PG_E_ARG;
  IndexState* I = index_of(ctx);
  if (!I || !I->selected) return pg_fail(ctx, PG_E_ARG, "screen: no selection over an index (call pg_screen_index_select first)");
  if (I->a.empty()) return PG_OK;
  if (!a_out || !b_out || !shared_out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  std::copy(I->a.begin(), I->a.end(), a_out);
  std::copy(I->b.begin(), I->b.end(), b_out);
  std::copy(I->s.begin(), I->s.end(), shared_out);
  return PG_OK;
}
