// pgscr_select.inc — part of pg_screen.hip: the selection (DESIGN.md §16.1).  C5 and its one host side (select_rows), which the band
// calls of pgscr_index.inc use as well, and the resident matrix of pg_screen_hold / pg_screen_load with the selection over it.
namespace {

constexpr uint32_t SEL_STEPS = 8;                  // 64-cell steps of one wave task
constexpr uint32_t SEL_CELLS = 64u * SEL_STEPS;    // cells of one wave task: a piece of ONE matrix row

// C5: the rule on a rectangle, cells = its rows [r0, r0 + rows) x n columns (the dense selection: r0 = 0, rows = n).  Tasks row-major:
// task = row of the rectangle * tpr + piece (tpr = pieces per row).  !FILL: counts[task] = kept cells of the task, counts[n_tasks] = 0
// (the scan's total lands there).  FILL: counts = the scanned offsets; total = their last entry, the room of the three output arrays.
// The output carries the GLOBAL row r0 + row of the rectangle.  need_row (read at the global row) and need_col are one array for the
// square calls, whose rows and columns are the same genomes: diagonal = the cell col == row is the genome with itself and is never kept.
// The search (pgscr_search.inc) has queries on the rows and the collection on the columns: two arrays, and no diagonal to skip.
template <bool FILL>
__global__ __launch_bounds__(256) void screen_select_kernel(const uint32_t* __restrict__ rect, const uint32_t* __restrict__ need_row_of,
                                                             const uint32_t* __restrict__ need_col_of, bool diagonal, uint32_t n, uint32_t r0, uint32_t tpr,
                                                             uint32_t n_tasks, unsigned long long* __restrict__ counts, unsigned long long total,
                                                             int32_t* __restrict__ a_out, int32_t* __restrict__ b_out, uint32_t* __restrict__ s_out) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), n_waves = gridDim.x * (blockDim.x >> 6);
  const unsigned long long below = (1ull << lane) - 1ull;
  for (uint32_t task = wave; task < n_tasks; task += n_waves) {      // (uniform over the wave: every lane reaches every ballot)
    const uint32_t brow = task / tpr, col0 = (task % tpr) * SEL_CELLS;
    const uint32_t row = r0 + brow;
    const uint32_t need_row = need_row_of[row];
    const uint32_t* __restrict__ cells = rect + (size_t)brow * n;
    uint32_t v[SEL_STEPS];
    bool keep[SEL_STEPS];
#pragma unroll
    for (uint32_t u = 0; u < SEL_STEPS; ++u) {
      const uint32_t col = col0 + 64u * u + lane;
      const bool in = col < n;
      v[u] = in ? cells[col] : 0u;
      const uint32_t need_col = in ? need_col_of[col] : 0u;
      keep[u] = in && !(diagonal && col == row) && v[u] >= (need_row < need_col ? need_row : need_col);
    }
    if (!FILL) {
      uint32_t c = 0;
#pragma unroll
      for (uint32_t u = 0; u < SEL_STEPS; ++u) c += (uint32_t)__popcll(__ballot(keep[u]));
      if (lane == 0) counts[task] = c;
    } else {
      unsigned long long at = counts[task];
#pragma unroll
      for (uint32_t u = 0; u < SEL_STEPS; ++u) {
        const unsigned long long bal = __ballot(keep[u]);
        const unsigned long long mine = at + (unsigned long long)__popcll(bal & below);
        if (keep[u] && mine < total) {
          a_out[mine] = (int32_t)row; b_out[mine] = (int32_t)(col0 + 64u * u + lane); s_out[mine] = v[u];
        }
        at += (unsigned long long)__popcll(bal);
      }
    }
  }
  if (!FILL && blockIdx.x == 0 && threadIdx.x == 0) counts[n_tasks] = 0ull;
}

struct SelectWork {      // the device buffers of a selection beside the cells and the kept triples
  PgDevBuf<uint32_t> need;                   // n: the thresholds
  PgDevBuf<unsigned long long> cnt, off;     // tasks + 1 each: the kept cells of every task, and their scan
};

uint32_t select_tasks(uint32_t n, uint32_t rows) { return rows * ((n + SEL_CELLS - 1) / SEL_CELLS); }      // rows * n <= 2^33 cells in pieces of 512: below 2^32

// Room for the selection of up to `rows` rows of n columns; tmp_bytes is raised to what its scan asks for.
// (pg_dev_alloc, not sk_malloc: what sk_malloc gives up when memory is short includes the resident matrix — the one pg_screen_select reads,
// and the one the band calls leave alone, however short memory is)
int select_alloc(pg_ctx* ctx, uint32_t n, uint32_t rows, SelectWork& W, size_t& tmp_bytes) {
  const size_t n_tasks = select_tasks(n, rows);
  int rc;
  if ((rc = pg_dev_alloc(ctx, "screen", W.need, n, "the thresholds")) || (rc = pg_dev_alloc(ctx, "screen", W.cnt, n_tasks + 1, "the task counts")) ||
      (rc = pg_dev_alloc(ctx, "screen", W.off, n_tasks + 1, "the task offsets")))
    return rc;
  PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& b) { return hipcub::DeviceScan::ExclusiveSum(nullptr, b, W.cnt.p, W.off.p, (int64_t)n_tasks + 1, ctx->stream); }));
  return PG_OK;
}

// The one selection: the rows [r0, r0 + rows) of the matrix stand in rect, the columns' thresholds in W.need and the rows' in need_row
// (on the device, read at r0 + row; the square calls pass W.need there too, and diagonal = true).  Count pass, scan, the total read
// back (the stream is synchronised there), room for the total in a, b, s (the caller's: a buffer that has the room is left alone), fill
// pass — queued, not waited for.  *total_out = the kept triples, in row-major order.
int select_rows(pg_ctx* ctx, const uint32_t* rect, const uint32_t* need_row, bool diagonal, uint32_t n, uint32_t r0, uint32_t rows, SelectWork& W, void* tmp, size_t tmp_bytes, PgDevBuf<int32_t>& a,
                PgDevBuf<int32_t>& b, PgDevBuf<uint32_t>& s, unsigned long long* total_out) {
  hipStream_t st = ctx->stream;
  const uint32_t tpr = (n + SEL_CELLS - 1) / SEL_CELLS, n_tasks = select_tasks(n, rows);
  const dim3 grid(grid_for(n_tasks, 4, (uint32_t)ctx->num_cu * 8u));
  hipLaunchKernelGGL(screen_select_kernel<false>, grid, dim3(256), 0, st, rect, need_row, (const uint32_t*)W.need.p, diagonal, n, r0, tpr, n_tasks, W.cnt.p, 0ull, (int32_t*)nullptr,
                     (int32_t*)nullptr, (uint32_t*)nullptr);
  PG_HIP(ctx, hipGetLastError());
  PG_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, W.cnt.p, W.off.p, (int64_t)n_tasks + 1, st));
  unsigned long long total = 0;
  PG_HIP(ctx, hipMemcpyAsync(&total, W.off.p + n_tasks, 8, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipStreamSynchronize(st));
  if (total > (unsigned long long)rows * (diagonal ? n - 1u : n))
    return pg_fail(ctx, PG_E_INTERNAL, diagonal ? "screen: the selection counted more cells than its rows have off the diagonal" : "screen: the selection counted more cells than its rows have");
  if (total) {
    int rc;
    if ((rc = pg_dev_alloc(ctx, "screen", a, (size_t)total, "the selected pairs")) || (rc = pg_dev_alloc(ctx, "screen", b, (size_t)total, "the selected pairs")) ||
        (rc = pg_dev_alloc(ctx, "screen", s, (size_t)total, "the selected pairs")))
      return rc;
    hipLaunchKernelGGL(screen_select_kernel<true>, grid, dim3(256), 0, st, rect, need_row, (const uint32_t*)W.need.p, diagonal, n, r0, tpr, n_tasks, W.off.p, total, a.p, b.p, s.p);
    PG_HIP(ctx, hipGetLastError());
  }
  *total_out = total;
  return PG_OK;
}

struct ScreenState {      // the resident matrix of pg_screen_hold / pg_screen_load and the latest selection over it
  uint32_t n = 0;
  PgDevBuf<uint32_t> d_shared;      // n x n
  bool selected = false;
  uint64_t n_sel = 0;
  PgDevBuf<int32_t> d_a, d_b;       // n_sel each
  PgDevBuf<uint32_t> d_s;
};

ScreenState* state_of(pg_ctx* ctx) { return static_cast<ScreenState*>(ctx->screen_state); }

}  // namespace

void pg_screen_drop(pg_ctx* ctx) {
  if (!ctx->screen_state) return;
  delete state_of(ctx);
  ctx->screen_state = nullptr;
}

extern "C" int pg_screen_release(pg_ctx* ctx) {
  if (!ctx) return PG_E_ARG;
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  pg_screen_drop(ctx);
  return PG_OK;
}

extern "C" int pg_screen_hold(pg_ctx* ctx, const int32_t* genome_ids, uint32_t n, int32_t kmer, int32_t scale, uint32_t part, uint32_t n_parts,
                              uint32_t* sizes_out) {
  if (!ctx) return PG_E_ARG;
  int rc;
  if ((rc = screen_check(ctx, genome_ids, n, kmer, scale, part, n_parts, sizes_out, false, nullptr))) return rc;
  if ((rc = pg_screen_release(ctx))) return rc;      // the matrix of an earlier call goes before the new one is made: never two at a time
  PgDevBuf<uint32_t> d_shared;
  if ((rc = screen_run(ctx, genome_ids, n, kmer, scale, part, n_parts, sizes_out, nullptr, d_shared))) return rc;
  if (n == 0) return PG_OK;      // (nothing to hold: a selection needs a matrix of one genome or more)
  ScreenState* S = new ScreenState();
  S->n = n;
  S->d_shared = std::move(d_shared);
  ctx->screen_state = S;
  return PG_OK;
}

extern "C" int pg_screen_load(pg_ctx* ctx, const uint32_t* shared, uint32_t n) {
  if (!ctx) return PG_E_ARG;
  if (n > pgscr::MAX_GENOMES) return pg_fail(ctx, PG_E_ARG, "screen: more than 8192 genomes in one call");      // (before the matrix is read)
  if (n == 0 || !shared) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  int rc;
  if ((rc = pg_screen_release(ctx))) return rc;
  PgDevBuf<uint32_t> d_shared;
  if ((rc = sk_malloc(ctx, d_shared, (size_t)n * n))) return rc;
  PG_HIP(ctx, hipMemcpyAsync(d_shared, shared, (size_t)n * n * 4, hipMemcpyHostToDevice, ctx->stream));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ScreenState* S = new ScreenState();
  S->n = n;
  S->d_shared = std::move(d_shared);
  ctx->screen_state = S;
  return PG_OK;
}

extern "C" int pg_screen_fetch(pg_ctx* ctx, uint32_t* shared_out) {
  if (!ctx) return PG_E_ARG;
  ScreenState* S = state_of(ctx);
  if (!S) return pg_fail(ctx, PG_E_ARG, "screen: no resident matrix (call pg_screen_hold or pg_screen_load first)");
  if (!shared_out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PG_HIP(ctx, hipMemcpyAsync(shared_out, S->d_shared, (size_t)S->n * S->n * 4, hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PG_OK;
}

extern "C" int pg_screen_select(pg_ctx* ctx, const uint32_t* need, uint32_t n, uint64_t* n_pairs_out) {
  if (!ctx) return PG_E_ARG;
  ScreenState* S = state_of(ctx);
  if (!S) return pg_fail(ctx, PG_E_ARG, "screen: no resident matrix (call pg_screen_hold or pg_screen_load first)");
  if (n != S->n) return pg_fail(ctx, PG_E_ARG, "screen: the resident matrix is of " + std::to_string(S->n) + " genomes, not " + std::to_string(n));
  if (!need || !n_pairs_out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  S->selected = false;
  S->n_sel = 0;
  SelectWork W;
  PgDevBuf<uint8_t> tmp;
  size_t tmp_bytes = 0;
  int rc;
  if ((rc = select_alloc(ctx, n, n, W, tmp_bytes)) || (rc = pg_dev_alloc(ctx, "screen", tmp, tmp_bytes + 16, "the scan's temporary storage"))) return rc;
  PG_HIP(ctx, hipMemcpyAsync(W.need, need, (size_t)n * 4, hipMemcpyHostToDevice, st));
  unsigned long long total = 0;
  if ((rc = select_rows(ctx, S->d_shared.p, (const uint32_t*)W.need.p, true, n, 0, n, W, (void*)tmp.p, tmp_bytes, S->d_a, S->d_b, S->d_s, &total))) return rc;      // the band [0, n)
  if (total) PG_HIP(ctx, hipStreamSynchronize(st));      // (W goes with this scope)
  S->selected = true;
  S->n_sel = total;
  *n_pairs_out = total;
  return PG_OK;
}

extern "C" int pg_screen_select_read(pg_ctx* ctx, int32_t* a_out, int32_t* b_out, uint32_t* shared_out) {
  if (!ctx) return PG_E_ARG;
  ScreenState* S = state_of(ctx);
  if (!S || !S->selected) return pg_fail(ctx, PG_E_ARG, "screen: no selection (call pg_screen_select first)");
  if (S->n_sel == 0) return PG_OK;
  if (!a_out || !b_out || !shared_out) return pg_fail(ctx, PG_E_ARG, "screen: bad argument");
  PG_HIP(ctx, hipSetDevice(ctx->device));
  PG_HIP(ctx, hipMemcpyAsync(a_out, S->d_a, S->n_sel * 4, hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipMemcpyAsync(b_out, S->d_b, S->n_sel * 4, hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipMemcpyAsync(shared_out, S->d_s, S->n_sel * 4, hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PG_OK;
}
