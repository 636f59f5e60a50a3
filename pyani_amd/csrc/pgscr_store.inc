// pgscr_store.inc — part of pg_screen.hip: the resident search index LEAVES the device, COMES BACK, and LOSES genomes (DESIGN.md §16.7).
// pg_screen_search_index_export copies the five arrays out; pg_screen_search_index_import uploads five arrays that a FILE supplied and
// validates every invariant the build guarantees before anything may use them — the lookup, count and claim kernels binary-search kmer[]
// and index by start[] and member[] — in an order in which no pass indexes by a value that an earlier pass has not validated:
//   V1 store_check_kmer_kernel    one thread per k-mer and one for the end: start[0] = 0, start[D] = E, start strictly increasing (so every
//                                 value is <= E and every k-mer has a holder); the k-mer < 4^k, sampled, in the slice its bin names (the
//                                 slice of position g by a binary search over slice_first, which the host has checked), above its
//                                 neighbour inside the slice.  It indexes by g, by a masked bin and by the bounded search only.
//   V2 store_check_member_kernel  returns at once unless V1 found start[] sound; then THE pass over the entries, balanced by entry
//                                 (item_walk over the starts, as A6): member < n, strictly ascending inside a k-mer, and — only under
//                                 member < n — one uint32 atomic into the per-column histogram: the sizes are COMPUTED, not believed.
// One 64-bit counter per kind of violation is read back once.
// pg_screen_search_index_remove is the mirror of the merge of pgscr_add.inc: the old entries stream through twice and are written once.
//   R1 exclusive scan over the entries of alive(t) = the holder member[t] stays (a transform iterator: member[] is read, new_of[] gathered,
//      nothing else stored): pos[t], the entry's new position; pos[E] = E'
//   R2 exclusive scan over the k-mers of (pos[start[g + 1]] > pos[start[g]]) (a transform iterator again): gpos[g], the k-mer's new
//      position; gpos[D] = D'
//   R3 remove_place_kernel      a surviving k-mer's value and new start (= pos[start[g]]) at gpos[g]
//   R4 remove_fill_kernel       member'[pos[t]] = new_of[member[t]] for the alive entries: consecutive lanes read consecutive words
//   R5 remove_directory_kernel  slice_first'[s] = gpos[slice_first[s]]
// new_of (uint32[n], the column's new number or STORE_GONE; made on the host, n <= 2^20: 4 MB at most) stays in global memory and is read
// through L2: see DESIGN.md §16.7 for why not LDS.  The new index is built beside the old one at its exact sizes and replaces it on success.
namespace {

constexpr uint32_t STORE_GONE = ~0u;      // new_of of a removed column
enum StoreErr { SE_START0, SE_START_END, SE_START_ORDER, SE_KMER_RANGE, SE_KMER_SAMPLED, SE_KMER_SLICE, SE_KMER_ORDER, SE_MEMBER_RANGE, SE_MEMBER_ORDER, SE_KINDS };
const char* const STORE_ERR_TEXT[SE_KINDS] = {
    "start[0] is not 0", "start[D] is not E", "start is not strictly increasing (a k-mer without a holder, or an entry range past E)",
    "k-mers are not below 4^kmer", "k-mers are not sampled under the scale", "k-mers stand outside the slice of their bin",
    "k-mers are not strictly ascending inside a slice", "members are not below n", "members are not strictly ascending inside a k-mer"};

// every active lane calls this; the violations of a wave cost one atomic
__device__ __forceinline__ void store_err(unsigned long long* __restrict__ word, bool bad) {
  const unsigned long long b = __ballot(bad);
  if (bad && __lane_id() == (unsigned)(__ffsll((long long)b) - 1)) atomicAdd(word, (unsigned long long)__popcll(b));
}

// V1 (n_slices >= 1 whenever D >= 1; slice_first[0] = 0, non-decreasing, slice_first[n_slices] = D: the host's checks)
__global__ __launch_bounds__(256) void store_check_kmer_kernel(const uint32_t* __restrict__ kmer, const unsigned long long* __restrict__ start, uint64_t D, uint64_t E,
                                                                const unsigned long long* __restrict__ slice_first, uint32_t n_slices,
                                                                const uint32_t* __restrict__ bin_slice, uint32_t kmer_max, uint32_t scale, uint32_t log2_scale,
                                                                unsigned long long* __restrict__ err) {
  for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g <= D; g += (uint64_t)gridDim.x * blockDim.x) {
    const unsigned long long s0 = start[g];
    store_err(&err[SE_START0], g == 0 && s0 != 0ull);
    store_err(&err[SE_START_END], g == D && s0 != E);
    bool order = false, range = false, unsampled = false, slice = false, ascend = false;
    if (g < D) {
      order = !(s0 < start[g + 1]);
      const uint32_t canon = kmer[g];
      range = canon > kmer_max;
      unsampled = !pgs::sampled(canon, scale);
      uint32_t lo = 0, hi = n_slices - 1u;      // the slice of position g: the last one that begins at or before g
      while (lo < hi) { const uint32_t mid = (lo + hi + 1u) >> 1; if (slice_first[mid] <= g) lo = mid; else hi = mid - 1u; }
      slice = bin_slice[pgscr::bin_of(canon, log2_scale)] != lo;
      ascend = g > slice_first[lo] && kmer[g - 1] >= canon;
    }
    store_err(&err[SE_START_ORDER], order);
    store_err(&err[SE_KMER_RANGE], range);
    store_err(&err[SE_KMER_SAMPLED], unsampled);
    store_err(&err[SE_KMER_SLICE], slice);
    store_err(&err[SE_KMER_ORDER], ascend);
  }
}

// V2: entry t of k-mer g; nothing is read unless start[] passed V1 (0 = start[0] < start[1] < ... < start[D] = E: item_walk's premise)
__global__ __launch_bounds__(256) void store_check_member_kernel(const unsigned long long* __restrict__ start, const uint32_t* __restrict__ member, uint64_t D, uint64_t E,
                                                                  uint32_t n, unsigned long long per, uint32_t* __restrict__ sizes,
                                                                  unsigned long long* __restrict__ err) {
  if (err[SE_START0] | err[SE_START_END] | err[SE_START_ORDER]) return;      // (uniform over the grid: V1 has finished on the stream)
  item_walk<unsigned long long>(start, (unsigned long long)D, (unsigned long long)E, per, [=](unsigned long long g, unsigned long long t) {
    const uint64_t at = g < D ? start[g] + t : E;
    bool range = false, ascend = false;
    if (at < E) {
      const uint32_t v = member[at];
      range = v >= n;
      ascend = t > 0 && member[at - 1] >= v;
      if (!range) atomicAdd(&sizes[v], 1u);
    }
    store_err(&err[SE_MEMBER_RANGE], range);
    store_err(&err[SE_MEMBER_ORDER], ascend);
  });
}

struct StoreAlive {      // R1's input: 1 where the holder of entry t stays (entry E: 0, the scan's total lands there)
  const uint32_t *member, *new_of;
  uint64_t E;
  uint32_t n;
  __host__ __device__ __forceinline__ unsigned long long operator()(unsigned long long t) const {
    if (t >= E) return 0ull;
    const uint32_t v = member[t];
    return v < n && new_of[v] != STORE_GONE ? 1ull : 0ull;
  }
};

struct StoreKept {      // R2's input: 1 where k-mer g keeps a holder (k-mer D: 0)
  const unsigned long long *start, *pos;
  uint64_t D, E;
  __host__ __device__ __forceinline__ unsigned long long operator()(unsigned long long g) const {
    if (g >= D) return 0ull;
    const unsigned long long a = start[g], b = start[g + 1];
    return a < b && b <= E && pos[b] > pos[a] ? 1ull : 0ull;
  }
};

// R3: one thread per old k-mer and one for the end
__global__ __launch_bounds__(256) void remove_place_kernel(const uint32_t* __restrict__ kmer, const unsigned long long* __restrict__ start, uint64_t D, uint64_t E,
                                                            const unsigned long long* __restrict__ pos, const unsigned long long* __restrict__ gpos,
                                                            uint32_t* __restrict__ kmer_new, unsigned long long* __restrict__ start_new, uint64_t D_new,
                                                            uint64_t E_new) {
  for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g <= D; g += (uint64_t)gridDim.x * blockDim.x) {
    if (g == D) { start_new[D_new] = E_new; continue; }
    const unsigned long long a = start[g], b = start[g + 1];
    if (!(a < b && b <= E)) continue;
    const unsigned long long gp = gpos[g];
    if (pos[b] > pos[a] && gp < D_new) { kmer_new[gp] = kmer[g]; start_new[gp] = pos[a]; }
  }
}

// R4: the second and last read of the old entries
__global__ __launch_bounds__(256) void remove_fill_kernel(const uint32_t* __restrict__ member, uint64_t E, uint32_t n, const uint32_t* __restrict__ new_of,
                                                           const unsigned long long* __restrict__ pos, uint32_t* __restrict__ member_new, uint64_t E_new) {
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < E; t += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t v = member[t];
    if (v >= n) continue;
    const uint32_t nv = new_of[v];
    if (nv == STORE_GONE) continue;
    const unsigned long long dst = pos[t];
    if (dst < E_new) member_new[dst] = nv;
  }
}

// R5: one thread per slice and one for the end; a slice whose k-mers all went begins where the next one does
__global__ __launch_bounds__(256) void remove_directory_kernel(const unsigned long long* __restrict__ slice_first, uint32_t n_slices, uint64_t D,
                                                                const unsigned long long* __restrict__ gpos, unsigned long long* __restrict__ slice_first_new) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s > n_slices) return;
  const unsigned long long f = s < n_slices && slice_first[s] < D ? slice_first[s] : D;
  slice_first_new[s] = gpos[f];      // gpos[D] = D'
}

uint64_t search_index_bytes(const SearchState* I) {
  return 4 * (uint64_t)I->d_kmer.cap + 8 * (uint64_t)I->d_start.cap + 4 * (uint64_t)I->d_member.cap + 8 * (uint64_t)I->d_slice_first.cap + 4 * (uint64_t)I->d_bin_slice.cap;
}

// The compaction of the index I without the columns new_of marks gone (n_new of them stay): on PG_OK the new arrays stand in I; on any
// failure I is as it was.
int search_remove_compact(pg_ctx* ctx, SearchState* I, const std::vector<uint32_t>& new_of, uint32_t n_new, ScreenEvents& T) {
  hipStream_t st = ctx->stream;
  const uint32_t cu_blocks = (uint32_t)ctx->num_cu * 8u;
  const uint64_t D = I->D, E = I->E;
  int rc;
  PgDevBuf<uint32_t> d_new_of;
  PgDevBuf<unsigned long long> pos, gpos;
  PgDevBuf<uint8_t> tmp;
  if ((rc = pg_dev_alloc(ctx, "screen", d_new_of, I->n, "the columns' new numbers")) ||
      (rc = pg_dev_alloc(ctx, "screen", pos, (size_t)E + 1, "the entries' new positions (8 bytes an entry of the search index while genomes are removed)")) ||
      (rc = pg_dev_alloc(ctx, "screen", gpos, (size_t)D + 1, "the k-mers' new positions")))
    return rc;
  hipcub::CountingInputIterator<unsigned long long> counting(0ull);
  hipcub::TransformInputIterator<unsigned long long, StoreAlive, hipcub::CountingInputIterator<unsigned long long>> alive(
      counting, StoreAlive{I->d_member.p, d_new_of.p, E, I->n});
  hipcub::TransformInputIterator<unsigned long long, StoreKept, hipcub::CountingInputIterator<unsigned long long>> kept(
      counting, StoreKept{I->d_start.p, pos.p, D, E});
  size_t tmp_bytes = 0;
  PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& b) { return hipcub::DeviceScan::ExclusiveSum(nullptr, b, alive, pos.p, (int64_t)(E + 1), st); }));
  PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& b) { return hipcub::DeviceScan::ExclusiveSum(nullptr, b, kept, gpos.p, (int64_t)(D + 1), st); }));
  if ((rc = pg_dev_alloc(ctx, "screen", tmp, tmp_bytes + 16, "the scans' temporary storage"))) return rc;
  unsigned long long E_new = 0, D_new = 0;
  PG_HIP(ctx, hipMemcpyAsync(d_new_of, new_of.data(), (size_t)I->n * 4, hipMemcpyHostToDevice, st));
  {
    ScreenEvents::Stage mark(T, ST_MARK, st);
    size_t tb = tmp_bytes;
    PG_HIP(ctx, hipcub::DeviceScan::ExclusiveSum((void*)tmp.p, tb, alive, pos.p, (int64_t)(E + 1), st));
    tb = tmp_bytes;
    PG_HIP(ctx, hipcub::DeviceScan::ExclusiveSum((void*)tmp.p, tb, kept, gpos.p, (int64_t)(D + 1), st));
  }
  PG_HIP(ctx, hipMemcpyAsync(&E_new, pos.p + E, 8, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipMemcpyAsync(&D_new, gpos.p + D, 8, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipStreamSynchronize(st));
  if (E_new > E || D_new > D || D_new > E_new) return pg_fail(ctx, PG_E_INTERNAL, "screen: a remove left " + std::to_string(D_new) + " k-mers and " + std::to_string(E_new) + " entries");
  // the new index, beside the old one, at its exact sizes
  PgDevBuf<uint32_t> kmer_new, member_new;
  PgDevBuf<unsigned long long> start_new, first_new;
  if ((rc = pg_dev_alloc(ctx, "screen", kmer_new, (size_t)D_new + 1, "the k-mers of the search index after a remove (the old index stays resident)")) ||
      (rc = pg_dev_alloc(ctx, "screen", start_new, (size_t)D_new + 1, "the starts of the search index after a remove (the old index stays resident)")) ||
      (rc = pg_dev_alloc(ctx, "screen", member_new, (size_t)E_new + 1, "the entries of the search index after a remove (the old index stays resident)")) ||
      (rc = pg_dev_alloc(ctx, "screen", first_new, (size_t)I->n_slices + 1, "the directory of the search index after a remove")))
    return rc;
  {
    ScreenEvents::Stage compact(T, ST_COMPACT, st);
    hipLaunchKernelGGL(remove_place_kernel, dim3(grid_for(D + 1, 256 * 4, cu_blocks)), dim3(256), 0, st, (const uint32_t*)I->d_kmer.p, (const unsigned long long*)I->d_start.p,
                       D, E, (const unsigned long long*)pos.p, (const unsigned long long*)gpos.p, kmer_new.p, start_new.p, (uint64_t)D_new, (uint64_t)E_new);
    PG_HIP(ctx, hipGetLastError());
    if (E) {
      hipLaunchKernelGGL(remove_fill_kernel, dim3(grid_for(E, 256 * 4, cu_blocks)), dim3(256), 0, st, (const uint32_t*)I->d_member.p, E, I->n, (const uint32_t*)d_new_of.p,
                         (const unsigned long long*)pos.p, member_new.p, (uint64_t)E_new);
      PG_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(remove_directory_kernel, dim3((I->n_slices + 256u) / 256u), dim3(256), 0, st, (const unsigned long long*)I->d_slice_first.p, I->n_slices, D,
                       (const unsigned long long*)gpos.p, first_new.p);
    PG_HIP(ctx, hipGetLastError());
  }
  PG_HIP(ctx, hipStreamSynchronize(st));
  // the new index takes the old one's place (the old arrays go here)
  I->d_kmer = std::move(kmer_new);
  I->d_start = std::move(start_new);
  I->d_member = std::move(member_new);
  I->d_slice_first = std::move(first_new);
  I->D = D_new; I->E = E_new;
  I->n = n_new;
  return PG_OK;
}

}  // namespace

extern "C" int pg_screen_search_index_shape(pg_ctx* ctx, uint64_t* shape_out) {
  if (!ctx || !shape_out) return pg_fail(ctx, PG_E_ARG, "bad argument");
  const SearchState* I = search_of(ctx);
  if (!I) return pg_fail(ctx, PG_E_ARG, "screen: no resident search index (call pg_screen_search_index first)");
  shape_out[0] = I->n; shape_out[1] = (uint64_t)I->kmer; shape_out[2] = (uint64_t)I->scale; shape_out[3] = I->D; shape_out[4] = I->E;
  shape_out[5] = I->n_slices; shape_out[6] = ctx->screen_search_stats.keys;
  return PG_OK;
}

extern "C" int pg_screen_search_index_export(pg_ctx* ctx, uint32_t* kmer_out, uint64_t* start_out, uint32_t* member_out, uint64_t* slice_first_out,
                                             uint32_t* bin_slice_out) {
  if (!ctx) return PG_E_ARG;
  const SearchState* I = search_of(ctx);
  if (!I) return pg_fail(ctx, PG_E_ARG, "screen: no resident search index (call pg_screen_search_index first)");
  if ((I->D && !kmer_out) || !start_out || (I->E && !member_out) || !slice_first_out || !bin_slice_out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (I->D) PG_HIP(ctx, hipMemcpyAsync(kmer_out, I->d_kmer, (size_t)I->D * 4, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipMemcpyAsync(start_out, I->d_start, ((size_t)I->D + 1) * 8, hipMemcpyDeviceToHost, st));
  if (I->E) PG_HIP(ctx, hipMemcpyAsync(member_out, I->d_member, (size_t)I->E * 4, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipMemcpyAsync(slice_first_out, I->d_slice_first, ((size_t)I->n_slices + 1) * 8, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipMemcpyAsync(bin_slice_out, I->d_bin_slice, (size_t)pgscr::N_BINS * 4, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipStreamSynchronize(st));
  return PG_OK;
}

extern "C" int pg_screen_search_index_import(pg_ctx* ctx, const uint64_t* shape, const uint32_t* kmer, const uint64_t* start, const uint32_t* member,
                                             const uint64_t* slice_first, const uint32_t* bin_slice, uint32_t* sizes_out) {
  if (!ctx) return PG_E_ARG;
  if (!shape) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  const uint64_t n64 = shape[0], D = shape[3], E = shape[4], S = shape[5];
  // the host's checks, before anything is uploaded
  if (n64 > pgscr::INDEX_MAX_GENOMES) return pg_fail(ctx, PG_E_ARG, "screen: more than 1048576 (2^20) genomes in one search index");
  if (shape[1] < (uint64_t)pgs::K_MIN || shape[1] > (uint64_t)pgs::K_MAX) return pg_fail(ctx, PG_E_ARG, "screen: the k-mer size must be 8 ... 16");
  if (shape[2] > (uint64_t)pgscr::MAX_SCALE || !pgscr::valid_scale((int32_t)shape[2])) return pg_fail(ctx, PG_E_ARG, "screen: scale must be a power of two, 1 ... 65536");
  if (E < D) return pg_fail(ctx, PG_E_ARG, "screen: a search index of " + std::to_string(D) + " k-mers and only " + std::to_string(E) + " entries");
  if (S > pgscr::N_BINS) return pg_fail(ctx, PG_E_ARG, "screen: a search index of more than 4096 slices");
  const uint32_t n = (uint32_t)n64, n_slices = (uint32_t)S;
  if (n == 0) {
    if (D || E) return pg_fail(ctx, PG_E_ARG, "screen: a search index of no genome with k-mers or entries");
    return pg_screen_search_index_release(ctx);      // (nothing to index: no index is left, as pg_screen_search_index does)
  }
  if ((D && !kmer) || !start || (E && !member) || !slice_first || !bin_slice || !sizes_out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  if (slice_first[0] != 0) return pg_fail(ctx, PG_E_ARG, "screen: the imported index's slice_first[0] is not 0");
  for (uint32_t s = 0; s < n_slices; ++s)
    if (slice_first[s] > slice_first[s + 1]) return pg_fail(ctx, PG_E_ARG, "screen: the imported index's slice_first descends at slice " + std::to_string(s));
  if (slice_first[n_slices] != D) return pg_fail(ctx, PG_E_ARG, "screen: the imported index's slice_first does not end at D");
  for (uint32_t bin = 0; bin < pgscr::N_BINS; ++bin)
    if (bin_slice[bin] >= n_slices && bin_slice[bin] != SEARCH_NO_SLICE)
      return pg_fail(ctx, PG_E_ARG, "screen: bin " + std::to_string(bin) + " of the imported index names slice " + std::to_string(bin_slice[bin]) + " of " + std::to_string(n_slices));
  PG_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const uint32_t cu_blocks = (uint32_t)ctx->num_cu * 8u;
  // the imported index, beside any resident one, at its exact sizes
  std::unique_ptr<SearchState> I(new SearchState());
  I->n = n; I->kmer = (int32_t)shape[1]; I->scale = (int32_t)shape[2];
  while ((1 << I->log2_scale) < I->scale) ++I->log2_scale;
  I->D = D; I->E = E; I->n_slices = n_slices;
  PgDevBuf<uint32_t> d_sizes;
  PgDevBuf<unsigned long long> d_err;
  int rc;
  if ((rc = pg_dev_alloc(ctx, "screen", I->d_kmer, (size_t)D + 1, "the k-mers of the imported search index")) ||
      (rc = pg_dev_alloc(ctx, "screen", I->d_start, (size_t)D + 1, "the starts of the imported search index")) ||
      (rc = pg_dev_alloc(ctx, "screen", I->d_member, (size_t)E + 1, "the entries of the imported search index")) ||
      (rc = pg_dev_alloc(ctx, "screen", I->d_slice_first, (size_t)n_slices + 1, "the directory of the imported search index")) ||
      (rc = pg_dev_alloc(ctx, "screen", I->d_bin_slice, pgscr::N_BINS, "the directory of the imported search index")) ||
      (rc = pg_dev_alloc(ctx, "screen", d_sizes, n, "the sizes of the imported search index")) ||
      (rc = pg_dev_alloc(ctx, "screen", d_err, SE_KINDS, "the validation's counters")))
    return rc;
  unsigned long long err[SE_KINDS] = {};
  ScreenEvents T;
  const auto run = [&]() -> int {
    if (D) PG_HIP(ctx, hipMemcpyAsync(I->d_kmer, kmer, (size_t)D * 4, hipMemcpyHostToDevice, st));
    PG_HIP(ctx, hipMemcpyAsync(I->d_start, start, ((size_t)D + 1) * 8, hipMemcpyHostToDevice, st));
    if (E) PG_HIP(ctx, hipMemcpyAsync(I->d_member, member, (size_t)E * 4, hipMemcpyHostToDevice, st));
    PG_HIP(ctx, hipMemcpyAsync(I->d_slice_first, slice_first, ((size_t)n_slices + 1) * 8, hipMemcpyHostToDevice, st));
    PG_HIP(ctx, hipMemcpyAsync(I->d_bin_slice, bin_slice, (size_t)pgscr::N_BINS * 4, hipMemcpyHostToDevice, st));
    PG_HIP(ctx, hipMemsetAsync(d_sizes, 0, (size_t)n * 4, st));
    PG_HIP(ctx, hipMemsetAsync(d_err, 0, SE_KINDS * 8, st));
    {
      ScreenEvents::Stage check(T, ST_CHECK, st);
      hipLaunchKernelGGL(store_check_kmer_kernel, dim3(grid_for(D + 1, 256 * 4, cu_blocks)), dim3(256), 0, st, (const uint32_t*)I->d_kmer.p,
                         (const unsigned long long*)I->d_start.p, D, E, (const unsigned long long*)I->d_slice_first.p, n_slices, (const uint32_t*)I->d_bin_slice.p,
                         pgs::kmer_mask(I->kmer), (uint32_t)I->scale, I->log2_scale, d_err.p);
      PG_HIP(ctx, hipGetLastError());
      if (D && E) {
        const unsigned long long per = items_per_workgroup(ctx, E);
        hipLaunchKernelGGL(store_check_member_kernel, dim3((uint32_t)((E + per - 1) / per)), dim3(256), 0, st, (const unsigned long long*)I->d_start.p,
                           (const uint32_t*)I->d_member.p, D, E, n, per, d_sizes.p, d_err.p);
        PG_HIP(ctx, hipGetLastError());
      }
    }
    PG_HIP(ctx, hipMemcpyAsync(err, d_err, SE_KINDS * 8, hipMemcpyDeviceToHost, st));
    PG_HIP(ctx, hipMemcpyAsync(sizes_out, d_sizes, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    return PG_OK;
  };
  rc = run();
  const hipError_t es = hipStreamSynchronize(st);      // (on errors too: the caller's arrays may still be read, and the new buffers go with this scope)
  if (rc) return rc;
  PG_HIP(ctx, es);
  for (int k = 0; k < SE_KINDS; ++k)
    if (err[k])
      return pg_fail(ctx, PG_E_ARG, std::string("screen: the imported search index is refused: ") + STORE_ERR_TEXT[k] + " (" + std::to_string(err[k]) + " of them)");
  // accepted: the resident index, its rectangle and every statistic go, and the imported one takes the place
  const double check_ms = T.ms(ST_CHECK);
  pg_screen_search_drop(ctx);
  PgScreenSearchStats& L = ctx->screen_search_stats;
  L = PgScreenSearchStats{};
  L.keys = shape[6]; L.kmers = D; L.entries = E; L.slices = n_slices;
  L.index_bytes = search_index_bytes(I.get());
  L.index_group_ms = check_ms;      // (an imported index was neither scanned nor grouped here: its validation stands in the build's second stage)
  ctx->screen_search_state = I.release();
  return PG_OK;
}

extern "C" int pg_screen_search_remove_last(pg_ctx* ctx, uint64_t* counts_out, double* ms_out) {
  if (!ctx || !counts_out || !ms_out) return pg_fail(ctx, PG_E_ARG, "bad argument");
  const PgScreenSearchRemoveStats& R = ctx->screen_search_remove_stats;
  counts_out[0] = R.genomes; counts_out[1] = R.entries; counts_out[2] = R.kmers; counts_out[3] = R.removes;
  ms_out[0] = R.mark_ms; ms_out[1] = R.compact_ms;
  return PG_OK;
}

extern "C" int pg_screen_search_index_remove(pg_ctx* ctx, const uint32_t* columns, uint32_t m) {
  if (!ctx) return PG_E_ARG;
  SearchState* I = search_of(ctx);
  if (!I) return pg_fail(ctx, PG_E_ARG, "screen: no resident search index (call pg_screen_search_index first)");
  if (m && !columns) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  if (m > I->n) return pg_fail(ctx, PG_E_ARG, "screen: " + std::to_string(m) + " columns to remove from a search index of " + std::to_string(I->n));
  std::vector<uint32_t> new_of(I->n, 0u);
  for (uint32_t i = 0; i < m; ++i) {
    if (columns[i] >= I->n) return pg_fail(ctx, PG_E_ARG, "screen: column " + std::to_string(columns[i]) + " is not in a search index of " + std::to_string(I->n) + " genomes");
    if (new_of[columns[i]] == STORE_GONE) return pg_fail(ctx, PG_E_ARG, "screen: column " + std::to_string(columns[i]) + " is given twice");
    new_of[columns[i]] = STORE_GONE;
  }
  if (m == 0) return PG_OK;      // (nothing to remove: the index, its rectangle and its statistics stay)
  PG_HIP(ctx, hipSetDevice(ctx->device));
  if (m == I->n) return pg_screen_search_index_release(ctx);      // (every column: no index is left, as a build of no genome leaves none)
  search_drop_counted(ctx, I);      // the rectangle was n wide
  uint32_t n_new = 0;
  for (uint32_t c = 0; c < I->n; ++c)
    if (new_of[c] != STORE_GONE) new_of[c] = n_new++;
  const uint64_t D_old = I->D, E_old = I->E;
  ScreenEvents T;
  const int rc = search_remove_compact(ctx, I, new_of, n_new, T);
  const hipError_t es = hipStreamSynchronize(ctx->stream);      // (the work arrays are gone; nothing of them is in flight)
  if (rc) return rc;
  PG_HIP(ctx, es);
  PgScreenSearchStats& L = ctx->screen_search_stats;
  L.kmers = I->D; L.entries = I->E; L.slices = I->n_slices;      // (keys stays: the scans of the build and the adds)
  L.index_bytes = search_index_bytes(I);
  PgScreenSearchRemoveStats& R = ctx->screen_search_remove_stats;
  const uint64_t removes = R.removes + 1;
  R = PgScreenSearchRemoveStats{};
  R.genomes = m; R.entries = E_old - I->E; R.kmers = D_old - I->D; R.removes = removes;
  R.mark_ms = T.ms(ST_MARK); R.compact_ms = T.ms(ST_COMPACT);
  return PG_OK;
}
