// pgscr_add.inc — part of pg_screen.hip: genomes ADDED to the resident search index without a rebuild (DESIGN.md §16.6).  The m genomes get
// the call indices n, n + 1, ...: larger than every index present, so their entries go behind a k-mer's old holders and nothing of the old
// index is sorted again.  screen_front runs over the m genomes with a fourth back half (AddBack: every slice's distinct keys staged with
// the genome rebased to n + j); the staging is sorted into the index's own order (slice, k-mer, genome); then, one pass each:
//   A1 add_stage_kernel      a front slice's keys into the staging, low word n + j
//   A2 add_slice_kernel      the index slice of every staged key (only for an index of two or more slices: the second, stable sort's key)
//   A3 add_locate_kernel     one thread per run of equal k-mer: bin -> slice, lower bound p, found / absent; an absent run counts one into
//                            ins[p].  Exclusive scan of the absent flags: a_r, the absent runs before r; inclusive scan of ins: shift[g],
//                            the absent runs that go before old k-mer g.  Old k-mer g moves to g + shift[g], run r to p_r + a_r.
//   A4 add_place_old_kernel  k-mer values and holder counts of the old k-mers at their merged positions
//   A5 add_place_run_kernel  the runs: an absent one brings its value and length, a matched one adds its length.  One exclusive scan of the
//                            counts gives the merged starts.
//   A6 add_fill_old_kernel   THE pass over the old entries, balanced by ENTRY (item_walk over start[]: a workgroup owns a contiguous range
//                            of entries, finds its first k-mer by binary search and keeps a window of k-mer boundaries in LDS): entry t
//                            of k-mer g goes to start'[g + shift[g]] + t.  Consecutive lanes read and write consecutive words.
//   A7 add_fill_new_kernel   item_walk over the runs: key t of run r goes behind the old holders of its k-mer
//   A8 add_directory_kernel  slice_first'[s] = slice_first[s] + the absent runs of the slices before s
// The merged index is built beside the old one, at its exact sizes, and takes its place once everything has succeeded.
namespace {

constexpr uint64_t ADD_MAX_RUNS = 0xffffffffull;      // distinct k-mers of one batch: their ranks are 32-bit

__global__ __launch_bounds__(256) void add_stage_kernel(const unsigned long long* __restrict__ u, uint64_t nu, uint32_t n, uint32_t m,
                                                         unsigned long long* __restrict__ out) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nu; i += (uint64_t)gridDim.x * blockDim.x) {
    const unsigned long long key = u[i];
    const uint32_t j = (uint32_t)key < m ? (uint32_t)key : m - 1u;      // (never the second: the front names the call's genomes)
    out[i] = (key & 0xffffffff00000000ull) | (unsigned long long)(n + j);
  }
}

__global__ __launch_bounds__(256) void add_slice_kernel(const unsigned long long* __restrict__ keys, uint64_t nk, uint32_t log2_scale,
                                                         const uint32_t* __restrict__ bin_slice, uint32_t n_slices, uint32_t* __restrict__ slice_out) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nk; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t sl = bin_slice[pgscr::bin_of((uint32_t)(keys[i] >> 32), log2_scale)];
    slice_out[i] = sl < n_slices ? sl : n_slices - 1u;      // (a bin without a slice: the locate kernel reports it)
  }
}

// the index slice of run r; n_slices where its bin has none
__device__ __forceinline__ uint32_t add_run_slice(const unsigned long long* __restrict__ u, uint64_t nk, const unsigned long long* __restrict__ run_first, uint64_t r,
                                                  uint32_t log2_scale, const uint32_t* __restrict__ bin_slice, uint32_t n_slices) {
  const unsigned long long s = run_first[r];
  if (s >= nk) return n_slices;
  const uint32_t sl = bin_slice[pgscr::bin_of((uint32_t)(u[s] >> 32), log2_scale)];
  return sl < n_slices ? sl : n_slices;
}

// A3.  u: the nk staged keys in the index's order; run r = the keys [run_first[r], run_first[r + 1]).  pos[r] = where the run's k-mer stands
// in the index, or where it goes; found[r] says which; rank[r] = 1 for an absent run (rank[nr] = 0: the scan's total lands there) and
// ins[pos[r]] counts it.  err[0] counts the runs whose bin no slice of the index covers.
__global__ __launch_bounds__(256) void add_locate_kernel(const unsigned long long* __restrict__ u, uint64_t nk, const unsigned long long* __restrict__ run_first,
                                                          uint32_t nr, uint32_t log2_scale, const uint32_t* __restrict__ bin_slice,
                                                          const unsigned long long* __restrict__ slice_first, uint32_t n_slices,
                                                          const uint32_t* __restrict__ kmer, uint64_t D, unsigned long long* __restrict__ pos,
                                                          uint8_t* __restrict__ found, uint32_t* __restrict__ rank, uint32_t* __restrict__ ins,
                                                          uint32_t* __restrict__ err) {
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= nr; r += (uint64_t)gridDim.x * blockDim.x) {
    if (r == nr) { rank[r] = 0u; continue; }
    const uint32_t sl = add_run_slice(u, nk, run_first, r, log2_scale, bin_slice, n_slices);
    if (sl >= n_slices) {      // (never: an index with a slice covers every bin)
      atomicAdd(&err[0], 1u);
      pos[r] = D; found[r] = 1u; rank[r] = 0u;
      continue;
    }
    const uint32_t canon = (uint32_t)(u[run_first[r]] >> 32);
    const uint64_t lo = slice_first[sl] < D ? slice_first[sl] : D, hi = slice_first[sl + 1] < D ? slice_first[sl + 1] : D;
    const uint64_t p = lo < hi ? pgscr::lower_bound_u32(kmer, lo, hi, canon) : hi;
    const bool f = p < hi && kmer[p] == canon;
    pos[r] = p; found[r] = (uint8_t)(f ? 1u : 0u); rank[r] = f ? 0u : 1u;
    if (!f) atomicAdd(&ins[p], 1u);      // p <= D: ins holds D + 1
  }
}

// A4: old k-mer g stands at g + shift[g] in the merged index, with its holders' count for now
__global__ __launch_bounds__(256) void add_place_old_kernel(const uint32_t* __restrict__ kmer, const unsigned long long* __restrict__ start, uint64_t D,
                                                             const uint32_t* __restrict__ shift, uint32_t* __restrict__ kmer_new,
                                                             unsigned long long* __restrict__ cnt_new, uint64_t D_new) {
  for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < D; g += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t gp = g + shift[g];
    if (gp < D_new) { kmer_new[gp] = kmer[g]; cnt_new[gp] = start[g + 1] - start[g]; }
  }
}

// A5 (after A4 on the stream): run r at pos[r] + a[r]; one run per k-mer, so the matched k-mer's count is this thread's alone
__global__ __launch_bounds__(256) void add_place_run_kernel(const unsigned long long* __restrict__ u, uint64_t nk, const unsigned long long* __restrict__ run_first,
                                                             uint32_t nr, const unsigned long long* __restrict__ pos, const uint8_t* __restrict__ found,
                                                             const uint32_t* __restrict__ a, uint32_t* __restrict__ kmer_new,
                                                             unsigned long long* __restrict__ cnt_new, uint64_t D_new) {
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nr; r += (uint64_t)gridDim.x * blockDim.x) {
    const unsigned long long s = run_first[r], e = run_first[r + 1];
    const uint64_t gp = pos[r] + a[r];
    if (s >= e || e > nk || gp >= D_new) continue;
    if (found[r]) cnt_new[gp] += e - s;
    else { kmer_new[gp] = (uint32_t)(u[s] >> 32); cnt_new[gp] = e - s; }
  }
}

// A6: entry t of old k-mer g
__global__ __launch_bounds__(256) void add_fill_old_kernel(const unsigned long long* __restrict__ start, const uint32_t* __restrict__ member, uint64_t D, uint64_t E,
                                                            const uint32_t* __restrict__ shift, const unsigned long long* __restrict__ start_new,
                                                            uint32_t* __restrict__ member_new, uint64_t D_new, uint64_t E_new, unsigned long long per,
                                                            uint32_t n_new) {
  item_walk<unsigned long long>(start, (unsigned long long)D, (unsigned long long)E, per, [=](unsigned long long g, unsigned long long t) {
    if (g >= D) return;
    const uint64_t gp = g + shift[g];
    if (gp >= D_new) return;
    const uint64_t src = start[g] + t, dst = start_new[gp] + t;
    if (src < E && dst < E_new && dst < start_new[gp + 1]) {
      const uint32_t v = member[src];
      if (v < n_new) member_new[dst] = v;
    }
  });
}

// A7: key t of run r, behind the old holders of its k-mer
__global__ __launch_bounds__(256) void add_fill_new_kernel(const unsigned long long* __restrict__ u, uint64_t nk, const unsigned long long* __restrict__ run_first,
                                                            uint32_t nr, const unsigned long long* __restrict__ pos, const uint8_t* __restrict__ found,
                                                            const uint32_t* __restrict__ a, const unsigned long long* __restrict__ start, uint64_t D,
                                                            const unsigned long long* __restrict__ start_new, uint32_t* __restrict__ member_new,
                                                            uint64_t D_new, uint64_t E_new, unsigned long long per, uint32_t n_new) {
  item_walk<uint32_t>(run_first, nr, (unsigned long long)nk, per, [=](uint32_t r, unsigned long long t) {
    if (r >= nr) return;
    const uint64_t p = pos[r], gp = p + a[r];
    if (gp >= D_new) return;
    uint64_t old = 0;
    if (found[r]) { if (p >= D) return; old = start[p + 1] - start[p]; }
    const uint64_t i = run_first[r] + t, dst = start_new[gp] + old + t;
    if (i < nk && dst < E_new && dst < start_new[gp + 1]) {
      const uint32_t v = (uint32_t)u[i];
      if (v < n_new) member_new[dst] = v;
    }
  });
}

// A8: one thread per slice and one for the end.  The runs stand in slice order: the first run of a slice >= s has a[r] absent runs before it.
__global__ __launch_bounds__(256) void add_directory_kernel(const unsigned long long* __restrict__ u, uint64_t nk, const unsigned long long* __restrict__ run_first,
                                                             uint32_t nr, uint32_t log2_scale, const uint32_t* __restrict__ bin_slice,
                                                             const unsigned long long* __restrict__ slice_first, uint32_t n_slices, const uint32_t* __restrict__ a,
                                                             uint64_t D_new, unsigned long long* __restrict__ slice_first_new) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s > n_slices) return;
  if (s == n_slices) { slice_first_new[s] = D_new; return; }
  uint64_t lo = 0, hi = nr;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2u;
    if (add_run_slice(u, nk, run_first, mid, log2_scale, bin_slice, n_slices) < s) lo = mid + 1u; else hi = mid;
  }
  slice_first_new[s] = slice_first[s] + a[lo];      // a[nr] = all absent runs
}

// The back half of pg_screen_search_index_add: every front slice's distinct keys are staged; nothing of the index is touched.
struct AddBack {
  pg_ctx* ctx;
  uint32_t n, m;
  PgDevBuf<unsigned long long> staged;
  size_t cap = 0;
  uint64_t count = 0;
  int prepare(uint64_t total_keys, uint64_t, size_t, size_t&) {
    cap = (size_t)total_keys;      // a slice's distinct keys are at most its keys
    if (sk_malloc(ctx, staged, cap + 1))
      return pg_fail(ctx, PG_E_NOMEM, "screen: no device memory to stage the " + std::to_string(cap) + " keys of the added genomes (8 bytes each; add fewer genomes a call)");
    return PG_OK;
  }
  int slice(const SliceGroups& S, ScreenEvents& T) {
    if (!S.nu) return PG_OK;
    if (count + S.nu > cap) return pg_fail(ctx, PG_E_INTERNAL, "screen: more distinct keys than keys in the added genomes");
    ScreenEvents::Stage group(T, ST_GROUP, ctx->stream);
    hipLaunchKernelGGL(add_stage_kernel, dim3(grid_for(S.nu, 256 * 4, (uint32_t)ctx->num_cu * 8u)), dim3(256), 0, ctx->stream, S.u, S.nu, n, m, staged.p + count);
    PG_HIP(ctx, hipGetLastError());
    count += S.nu;
    return PG_OK;
  }
};

// The merge of nk staged keys (genomes n ... n + m - 1) into the index I: on PG_OK the merged arrays stand in I; on any failure I is as it was.
int search_add_merge(pg_ctx* ctx, SearchState* I, uint32_t m, PgDevBuf<unsigned long long>& staged, uint64_t nk, ScreenEvents& T, uint64_t* absent_out,
                     uint64_t* runs_out) {
  hipStream_t st = ctx->stream;
  const uint32_t cu_blocks = (uint32_t)ctx->num_cu * 8u;
  const uint64_t D = I->D, E = I->E;
  const uint32_t n_new = I->n + m;
  int rc;
  // the directory the batch is sorted by: the index's, or, for an index without a slice (no genome of it has a key), one slice over every bin
  const bool own_dir = I->n_slices == 0;
  const uint32_t n_slices = own_dir ? 1u : I->n_slices;
  PgDevBuf<uint32_t> dir_bin;
  PgDevBuf<unsigned long long> dir_first;
  if (own_dir) {
    if (D || E) return pg_fail(ctx, PG_E_INTERNAL, "screen: a search index with k-mers and no slice");
    if ((rc = pg_dev_alloc(ctx, "screen", dir_bin, pgscr::N_BINS, "the directory of the merged search index")) ||
        (rc = pg_dev_alloc(ctx, "screen", dir_first, 2, "the directory of the merged search index")))
      return rc;
    PG_HIP(ctx, hipMemsetAsync(dir_bin, 0, (size_t)pgscr::N_BINS * 4, st));
    PG_HIP(ctx, hipMemsetAsync(dir_first, 0, 2 * 8, st));
  }
  const uint32_t* bin_slice = own_dir ? dir_bin.p : I->d_bin_slice.p;
  const unsigned long long* slice_first = own_dir ? dir_first.p : I->d_slice_first.p;

  PgDevBuf<unsigned long long> sorted, run_first, pos, d_sel;
  PgDevBuf<uint32_t> slice_a, slice_b, rank, ins, d_err;
  PgDevBuf<uint8_t> head, found, tmp;
  if ((rc = sk_malloc(ctx, sorted, (size_t)nk + 1)) || (rc = sk_malloc(ctx, run_first, (size_t)nk + 1)) || (rc = sk_malloc(ctx, pos, (size_t)nk + 1)) ||
      (rc = sk_malloc(ctx, rank, (size_t)nk + 1)) || (rc = sk_malloc(ctx, head, (size_t)nk + 1)) || (rc = sk_malloc(ctx, found, (size_t)nk + 1)) ||
      (rc = sk_malloc(ctx, ins, (size_t)D + 1)) || (rc = sk_malloc(ctx, d_sel, 1)) || (rc = sk_malloc(ctx, d_err, 1)))
    return rc;
  if (n_slices > 1 && ((rc = sk_malloc(ctx, slice_a, (size_t)nk + 1)) || (rc = sk_malloc(ctx, slice_b, (size_t)nk + 1)))) return rc;
  const int end_bit = 32 + 2 * I->kmer;
  int slice_bits = 1;
  while ((1u << slice_bits) < n_slices) ++slice_bits;
  hipcub::CountingInputIterator<unsigned long long> counting(0ull);
  size_t tmp_bytes = 0;
  PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& b) {
    return hipcub::DeviceRadixSort::SortKeys(nullptr, b, (const unsigned long long*)staged.p, sorted.p, (int64_t)nk, 0, end_bit, st); }));
  if (n_slices > 1)
    PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& b) {
      return hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint32_t*)slice_a.p, slice_b.p, (const unsigned long long*)sorted.p, staged.p, (int64_t)nk, 0, slice_bits, st); }));
  PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& b) {
    return hipcub::DeviceSelect::Flagged(nullptr, b, counting, (const uint8_t*)head.p, run_first.p, d_sel.p, (int64_t)nk, st); }));
  PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& b) { return hipcub::DeviceScan::ExclusiveSum(nullptr, b, rank.p, rank.p, (int64_t)(nk + 1), st); }));
  PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& b) { return hipcub::DeviceScan::InclusiveSum(nullptr, b, ins.p, ins.p, (int64_t)(D + 1), st); }));
  PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& b) {
    return hipcub::DeviceScan::ExclusiveSum(nullptr, b, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (int64_t)(D + nk + 1), st); }));
  if ((rc = sk_malloc(ctx, tmp, tmp_bytes + 16))) return rc;

  // the staged keys in the index's order: by key, then (stable) by slice
  const unsigned long long* u = sorted.p;
  unsigned long long nr = 0;
  {
    ScreenEvents::Stage group(T, ST_GROUP, st);
    size_t tb = tmp_bytes;
    PG_HIP(ctx, hipcub::DeviceRadixSort::SortKeys((void*)tmp.p, tb, (const unsigned long long*)staged.p, sorted.p, (int64_t)nk, 0, end_bit, st));
    if (n_slices > 1) {
      hipLaunchKernelGGL(add_slice_kernel, dim3(grid_for(nk, 256 * 4, cu_blocks)), dim3(256), 0, st, (const unsigned long long*)sorted.p, nk, I->log2_scale, bin_slice,
                         n_slices, slice_a.p);
      PG_HIP(ctx, hipGetLastError());
      tb = tmp_bytes;
      PG_HIP(ctx, hipcub::DeviceRadixSort::SortPairs((void*)tmp.p, tb, (const uint32_t*)slice_a.p, slice_b.p, (const unsigned long long*)sorted.p, staged.p, (int64_t)nk, 0,
                                                     slice_bits, st));
      u = staged.p;
    }
    // the runs of equal k-mer
    hipLaunchKernelGGL(search_mark_kernel, dim3(grid_for(nk, 256 * 4, cu_blocks)), dim3(256), 0, st, u, nk, head.p, (uint32_t*)nullptr);
    PG_HIP(ctx, hipGetLastError());
    tb = tmp_bytes;
    PG_HIP(ctx, hipcub::DeviceSelect::Flagged((void*)tmp.p, tb, counting, (const uint8_t*)head.p, run_first.p, d_sel.p, (int64_t)nk, st));
    PG_HIP(ctx, hipMemcpyAsync(&nr, d_sel.p, 8, hipMemcpyDeviceToHost, st));
  }
  PG_HIP(ctx, hipStreamSynchronize(st));
  if (nr < 1 || nr > nk) return pg_fail(ctx, PG_E_INTERNAL, "screen: " + std::to_string(nk) + " added entries gave " + std::to_string(nr) + " k-mers");
  if (nr > ADD_MAX_RUNS) return pg_fail(ctx, PG_E_NOMEM, "screen: more than 2^32 - 1 distinct k-mers in one add; add fewer genomes a call");
  const unsigned long long end_key = nk;
  PG_HIP(ctx, hipMemcpyAsync(run_first.p + nr, &end_key, 8, hipMemcpyHostToDevice, st));

  // A3 and the two scans
  uint32_t absent = 0, err = 0;
  {
    ScreenEvents::Stage merge(T, ST_MERGE, st);
    PG_HIP(ctx, hipMemsetAsync(ins, 0, ((size_t)D + 1) * 4, st));
    PG_HIP(ctx, hipMemsetAsync(d_err, 0, 4, st));
    hipLaunchKernelGGL(add_locate_kernel, dim3(grid_for(nr + 1, 256, cu_blocks)), dim3(256), 0, st, u, nk, (const unsigned long long*)run_first.p, (uint32_t)nr,
                       I->log2_scale, bin_slice, slice_first, n_slices, (const uint32_t*)I->d_kmer.p, D, pos.p, found.p, rank.p, ins.p, d_err.p);
    PG_HIP(ctx, hipGetLastError());
    size_t tb = tmp_bytes;
    PG_HIP(ctx, hipcub::DeviceScan::ExclusiveSum((void*)tmp.p, tb, rank.p, rank.p, (int64_t)(nr + 1), st));
    tb = tmp_bytes;
    PG_HIP(ctx, hipcub::DeviceScan::InclusiveSum((void*)tmp.p, tb, ins.p, ins.p, (int64_t)(D + 1), st));
    PG_HIP(ctx, hipMemcpyAsync(&absent, rank.p + nr, 4, hipMemcpyDeviceToHost, st));
    PG_HIP(ctx, hipMemcpyAsync(&err, d_err.p, 4, hipMemcpyDeviceToHost, st));
  }
  PG_HIP(ctx, hipStreamSynchronize(st));
  if (err) return pg_fail(ctx, PG_E_INTERNAL, "screen: " + std::to_string(err) + " added k-mers lie in bins that no slice of the search index covers");
  if (absent > nr) return pg_fail(ctx, PG_E_INTERNAL, "screen: more new k-mers than added k-mers");
  const uint32_t* a = rank.p;           // the absent runs before run r; a[nr] = all of them
  const uint32_t* shift = ins.p;        // the absent runs that go before old k-mer g
  const uint64_t D_new = D + absent, E_new = E + nk;

  // the merged index, beside the old one, at its exact sizes
  PgDevBuf<uint32_t> kmer_new, member_new;
  PgDevBuf<unsigned long long> start_new, first_new;
  if ((rc = pg_dev_alloc(ctx, "screen", kmer_new, (size_t)D_new + 1, "the k-mers of the merged search index (the old index stays resident)")) ||
      (rc = pg_dev_alloc(ctx, "screen", start_new, (size_t)D_new + 1, "the starts of the merged search index (the old index stays resident)")) ||
      (rc = pg_dev_alloc(ctx, "screen", member_new, (size_t)E_new + 1, "the entries of the merged search index (the old index stays resident)")) ||
      (rc = pg_dev_alloc(ctx, "screen", first_new, (size_t)n_slices + 1, "the directory of the merged search index")))
    return rc;
  unsigned long long total = 0;
  {
    ScreenEvents::Stage merge(T, ST_MERGE, st);
    PG_HIP(ctx, hipMemsetAsync(start_new.p + D_new, 0, 8, st));
    if (D) {
      hipLaunchKernelGGL(add_place_old_kernel, dim3(grid_for(D, 256 * 4, cu_blocks)), dim3(256), 0, st, (const uint32_t*)I->d_kmer.p,
                         (const unsigned long long*)I->d_start.p, D, shift, kmer_new.p, start_new.p, D_new);
      PG_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(add_place_run_kernel, dim3(grid_for(nr, 256, cu_blocks)), dim3(256), 0, st, u, nk, (const unsigned long long*)run_first.p, (uint32_t)nr,
                       (const unsigned long long*)pos.p, (const uint8_t*)found.p, a, kmer_new.p, start_new.p, D_new);
    PG_HIP(ctx, hipGetLastError());
    size_t tb = tmp_bytes;
    PG_HIP(ctx, hipcub::DeviceScan::ExclusiveSum((void*)tmp.p, tb, start_new.p, start_new.p, (int64_t)(D_new + 1), st));
    PG_HIP(ctx, hipMemcpyAsync(&total, start_new.p + D_new, 8, hipMemcpyDeviceToHost, st));
  }
  PG_HIP(ctx, hipStreamSynchronize(st));
  if (total != E_new)
    return pg_fail(ctx, PG_E_INTERNAL, "screen: the merged search index counts " + std::to_string(total) + " entries where " + std::to_string(E_new) + " are due");
  {
    ScreenEvents::Stage merge(T, ST_MERGE, st);
    if (E) {
      const unsigned long long per = items_per_workgroup(ctx, E);
      hipLaunchKernelGGL(add_fill_old_kernel, dim3((uint32_t)((E + per - 1) / per)), dim3(256), 0, st, (const unsigned long long*)I->d_start.p,
                         (const uint32_t*)I->d_member.p, D, E, shift, (const unsigned long long*)start_new.p, member_new.p, D_new, E_new, per, n_new);
      PG_HIP(ctx, hipGetLastError());
    }
    const unsigned long long per = items_per_workgroup(ctx, nk);
    hipLaunchKernelGGL(add_fill_new_kernel, dim3((uint32_t)((nk + per - 1) / per)), dim3(256), 0, st, u, nk, (const unsigned long long*)run_first.p, (uint32_t)nr,
                       (const unsigned long long*)pos.p, (const uint8_t*)found.p, a, (const unsigned long long*)I->d_start.p, D,
                       (const unsigned long long*)start_new.p, member_new.p, D_new, E_new, per, n_new);
    PG_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(add_directory_kernel, dim3((n_slices + 256u) / 256u), dim3(256), 0, st, u, nk, (const unsigned long long*)run_first.p, (uint32_t)nr, I->log2_scale,
                       bin_slice, slice_first, n_slices, a, D_new, first_new.p);
    PG_HIP(ctx, hipGetLastError());
  }
  PG_HIP(ctx, hipStreamSynchronize(st));
  // the merged index takes the old one's place (the old arrays go here)
  I->d_kmer = std::move(kmer_new);
  I->d_start = std::move(start_new);
  I->d_member = std::move(member_new);
  I->d_slice_first = std::move(first_new);
  if (own_dir) I->d_bin_slice = std::move(dir_bin);
  I->n_slices = n_slices;
  I->D = D_new; I->E = E_new;
  I->n = n_new;
  *absent_out = absent;
  *runs_out = nr;
  return PG_OK;
}

}  // namespace

extern "C" int pg_screen_search_add_last(pg_ctx* ctx, uint64_t* counts_out, double* ms_out) {
  if (!ctx || !counts_out || !ms_out) return pg_fail(ctx, PG_E_ARG, "bad argument");
  const PgScreenSearchAddStats& A = ctx->screen_search_add_stats;
  counts_out[0] = A.genomes; counts_out[1] = A.keys; counts_out[2] = A.entries; counts_out[3] = A.new_kmers; counts_out[4] = A.matched_kmers; counts_out[5] = A.adds;
  ms_out[0] = A.scan_ms; ms_out[1] = A.group_ms; ms_out[2] = A.merge_ms;
  return PG_OK;
}

extern "C" int pg_screen_search_index_add(pg_ctx* ctx, const int32_t* genome_ids, uint32_t m, uint32_t* sizes_out) {
  if (!ctx) return PG_E_ARG;
  SearchState* I = search_of(ctx);
  if (!I) return pg_fail(ctx, PG_E_ARG, "screen: no resident search index (call pg_screen_search_index first)");
  const std::string too_many = "screen: " + std::to_string(I->n) + " + " + std::to_string(m) + " genomes, more than 1048576 (2^20) in one search index";
  int rc;
  if ((rc = screen_check(ctx, genome_ids, m, I->kmer, I->scale, 0, 1, sizes_out, false, nullptr, pgscr::INDEX_MAX_GENOMES - I->n, too_many.c_str()))) return rc;
  if (m == 0) return PG_OK;      // (nothing to add: the index, its rectangle and its statistics stay)
  PG_HIP(ctx, hipSetDevice(ctx->device));
  search_drop_counted(ctx, I);      // the rectangle was n wide
  if ((rc = pg_upload(ctx))) return rc;
  hipStream_t st = ctx->stream;
  ScreenEvents T;
  FrontTotals tot;
  PgDevBuf<uint32_t> d_sizes;
  AddBack back{ctx, I->n, m};
  uint64_t absent = 0, runs = 0;
  rc = screen_front(ctx, genome_ids, m, I->kmer, I->scale, 0, 1, true, d_sizes, T, tot, back);
  hipError_t e = rc ? hipSuccess : hipMemcpyAsync(sizes_out, d_sizes, (size_t)m * 4, hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);      // (on errors too: the staging goes with this scope)
  if (rc) return rc;
  PG_HIP(ctx, e);
  PG_HIP(ctx, es);
  const uint64_t nk = back.count;
  if (nk) {
    rc = search_add_merge(ctx, I, m, back.staged, nk, T, &absent, &runs);
    const hipError_t em = hipStreamSynchronize(st);      // (the merge's work arrays are gone; nothing of them is in flight)
    if (rc) return rc;
    PG_HIP(ctx, em);
  } else {
    I->n += m;      // genomes without a key: columns of zeros, and not an entry moves
  }
  PgScreenSearchStats& L = ctx->screen_search_stats;
  L.keys += tot.keys; L.kmers = I->D; L.entries = I->E; L.slices = I->n_slices;
  L.index_bytes = 4 * (uint64_t)I->d_kmer.cap + 8 * (uint64_t)I->d_start.cap + 4 * (uint64_t)I->d_member.cap + 8 * (uint64_t)I->d_slice_first.cap + 4 * (uint64_t)I->d_bin_slice.cap;
  PgScreenSearchAddStats& A = ctx->screen_search_add_stats;
  const uint64_t adds = A.adds + 1;
  A = PgScreenSearchAddStats{};
  A.genomes = m; A.keys = tot.keys; A.entries = nk; A.new_kmers = absent; A.matched_kmers = runs - absent; A.adds = adds;
  A.scan_ms = T.ms(ST_SCAN); A.group_ms = T.ms(ST_GROUP); A.merge_ms = T.ms(ST_MERGE);
  return PG_OK;
}
