// pgscr_front.inc — part of pg_screen.hip: the front half of every screen (C1 scan, C2 sort and group: screen_front), the balance by item
// that both count kernels walk (item_walk), and the back half of the dense calls (C3, C4: DenseBack, screen_run, pg_screen_matrix).
namespace {

struct ScreenGenome {      // one genome of the call
  uint64_t arena_start;    // bases: codes + arena_start / 16, mask + arena_start / 32
  int64_t stream_len;
  uint64_t item0;          // first work item (256 chunks of 32 start positions) of the genome; items of all genomes back to back
};

constexpr uint32_t SCAN_CHUNKS = 256;      // chunks of one work item: one per lane

// counters: [0] the fill pass's append cursor
template <bool FILL, int K>
__global__ __launch_bounds__(256) void screen_scan_kernel(const uint32_t* __restrict__ arena_codes, const uint32_t* __restrict__ arena_mask,
                                                           const ScreenGenome* __restrict__ tab, uint32_t n, uint64_t n_items, uint32_t scale,
                                                           uint32_t log2_scale, uint32_t bin_lo, uint32_t bin_hi, unsigned long long* __restrict__ hist,
                                                           unsigned long long* __restrict__ keys, unsigned long long keys_cap,
                                                           unsigned long long* __restrict__ counters) {
  __shared__ uint32_t lhist[FILL ? 1 : pgscr::N_BINS];
  if (!FILL) {
    for (uint32_t i = threadIdx.x; i < pgscr::N_BINS; i += blockDim.x) lhist[i] = 0u;
    __syncthreads();
  }
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
    uint32_t lo = 0, hi = n - 1u;      // the genome of the item: the last one whose first item is <= item (uniform over the workgroup)
    while (lo < hi) { const uint32_t mid = (lo + hi + 1u) >> 1; if (tab[mid].item0 <= item) lo = mid; else hi = mid - 1u; }
    const uint32_t g = lo;
    const int64_t stream_len = tab[g].stream_len;
    const uint32_t* codes = arena_codes + tab[g].arena_start / 16;
    const uint32_t* mask = arena_mask + tab[g].arena_start / 32;
    const int64_t n_chunks = (stream_len + 31) / 32;
    const int64_t c = (int64_t)(item - tab[g].item0) * SCAN_CHUNKS + threadIdx.x;
    const bool active = c < n_chunks;
    // bases 32 c .. 32 c + 47 = code words 2 c, 2 c + 1, 2 c + 2; mask words c, c + 1 (the arena is padded: reads past the stream see dirty bases)
    uint64_t c01 = 0, m = 0;
    uint32_t c2 = 0;
    if (active) {
      c01 = (uint64_t)codes[2 * c] | ((uint64_t)codes[2 * c + 1] << 32);
      c2 = codes[2 * c + 2];
      m = (uint64_t)mask[c] | ((uint64_t)mask[c + 1] << 32);
    }
    uint32_t f = 0, r = 0;
    constexpr uint64_t WINDOW = (1ull << K) - 1ull;      // the K mask bits of a window
    for (int t = 0; t < 32 + K - 1; ++t) {      // base 32 c + t enters the window; the k-mer that ENDS on it starts at 32 c + t - (K - 1)
      const uint32_t code = t < 32 ? (uint32_t)(c01 >> (2 * t)) & 3u : (c2 >> (2 * (t - 32))) & 3u;
      f = pgs::roll_fwd(f, code, K); r = pgs::roll_rc(r, code, K);
      const int s = t - (K - 1);
      if (s < 0) continue;      // (uniform)
      const int64_t p = 32 * c + s;
      const uint32_t canon = f < r ? f : r;
      const uint32_t h = pgs::mix32(canon);
      const uint32_t bin = pgscr::bin_of_hash(h, log2_scale);
      // an inactive lane has m = 0; an ambiguity symbol, a record end or the stream's end fail the window test
      const bool take = active && p + K <= stream_len && ((m >> s) & WINDOW) == WINDOW && (h & (scale - 1u)) == 0u && bin >= bin_lo && bin < bin_hi;
      if (!FILL) {
        if (take) atomicAdd(&lhist[bin], 1u);
      } else {      // one atomic per wave: every lane of the wave is here (no divergent exit above)
        const unsigned long long bal = __ballot(take);
        if (bal) {
          const int leader = __ffsll(bal) - 1;
          unsigned long long base = 0;
          if ((int)lane == leader) base = atomicAdd(&counters[0], (unsigned long long)__popcll(bal));
          const uint32_t b_lo = __shfl((uint32_t)base, leader, 64), b_hi = __shfl((uint32_t)(base >> 32), leader, 64);
          if (take) {
            const unsigned long long at = (((unsigned long long)b_hi << 32) | b_lo) + (unsigned long long)__popcll(bal & ((1ull << lane) - 1ull));
            if (at < keys_cap) keys[at] = ((unsigned long long)canon << 32) | g;
          }
        }
      }
    }
  }
  if (!FILL) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < pgscr::N_BINS; i += blockDim.x)
      if (lhist[i]) atomicAdd(&hist[i], (unsigned long long)lhist[i]);
  }
}

template <bool FILL>
auto screen_scan_of(int32_t kmer) -> decltype(&screen_scan_kernel<FILL, 16>) {
  switch (kmer) {
    case 8: return screen_scan_kernel<FILL, 8>;
    case 9: return screen_scan_kernel<FILL, 9>;
    case 10: return screen_scan_kernel<FILL, 10>;
    case 11: return screen_scan_kernel<FILL, 11>;
    case 12: return screen_scan_kernel<FILL, 12>;
    case 13: return screen_scan_kernel<FILL, 13>;
    case 14: return screen_scan_kernel<FILL, 14>;
    case 15: return screen_scan_kernel<FILL, 15>;
    case 16: return screen_scan_kernel<FILL, 16>;
  }
  return nullptr;      // (pg_screen_matrix refuses every other k before it gets here)
}

// u: the nu distinct keys of a slice, sorted.  sizes[g] += the entries of genome g; flags[i]: bit 0 = the first, bit 1 = the last entry of
// a k-mer held by two or more genomes.  !WIDE (the dense calls, n <= MAX_GENOMES): an LDS histogram of the genomes, one atomic in HBM per
// genome and workgroup.  WIDE (the index, n up to 2^20: no LDS histogram of the genomes fits): sizes[g] += 1 by a uint32 atomic in HBM,
// one per entry, no return value — the keys stand in (k-mer, genome) order, so the genomes of neighbouring lanes differ inside a group and
// are unrelated across groups: a wave finds next to nothing to aggregate (DESIGN.md §16.2) — and bit 2 of the flags = the entry belongs to
// a k-mer held by two or more genomes (what the index keeps).
template <bool WIDE>
__global__ __launch_bounds__(256) void screen_head_kernel(const unsigned long long* __restrict__ u, uint64_t nu, uint32_t n, uint32_t* __restrict__ sizes,
                                                           uint8_t* __restrict__ flags) {
  __shared__ uint32_t lsize[WIDE ? 1 : pgscr::MAX_GENOMES];
  if (!WIDE) {
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) lsize[i] = 0u;
    __syncthreads();
  }
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nu; i += (uint64_t)gridDim.x * blockDim.x) {
    const unsigned long long key = u[i];
    const uint32_t canon = (uint32_t)(key >> 32), g = (uint32_t)key;
    const bool same_prev = i > 0 && (uint32_t)(u[i - 1] >> 32) == canon;
    const bool same_next = i + 1 < nu && (uint32_t)(u[i + 1] >> 32) == canon;
    flags[i] = (uint8_t)((!same_prev && same_next ? 1u : 0u) | (same_prev && !same_next ? 2u : 0u) | (WIDE && (same_prev || same_next) ? 4u : 0u));
    if (g < n) { if (WIDE) atomicAdd(&sizes[g], 1u); else atomicAdd(&lsize[g], 1u); }
  }
  if (!WIDE) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x)
      if (lsize[i]) atomicAdd(&sizes[i], lsize[i]);
  }
}

struct FlagBit {      // the flag array read as one of its bits
  uint32_t bit;
  __host__ __device__ __forceinline__ uint8_t operator()(uint8_t f) const { return (uint8_t)((f >> bit) & 1u); }
};

// The input of an exclusive scan over n weights: w[i] = weight(i), w[n] = 0 (the scan's total lands there).  Weight::Index: the type that
// holds n (the groups of a slice are fewer than 2^32, those of the index need not be).
template <typename Weight>
__global__ __launch_bounds__(256) void screen_weight_kernel(typename Weight::Index n, unsigned long long* __restrict__ w, Weight weight) {
  typedef typename Weight::Index Index;
  for (Index i = (Index)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (Index)gridDim.x * blockDim.x) w[i] = i < n ? weight(i) : 0ull;
}
template <typename Weight>
hipError_t screen_weights(pg_ctx* ctx, uint64_t n, unsigned long long* w, Weight weight) {
  hipLaunchKernelGGL(screen_weight_kernel<Weight>, dim3(grid_for(n + 1, 256, (uint32_t)ctx->num_cu * 8u)), dim3(256), 0, ctx->stream, (typename Weight::Index)n, w,
                     weight);
  return hipGetLastError();
}

struct TriWeight {      // the items of slice group g: its genomes' pairs
  typedef uint32_t Index;
  const uint32_t *first, *last;
  __device__ unsigned long long operator()(uint32_t g) const { return pgscr::tri_items(last[g] - first[g] + 1u); }
};

// The balance by ITEM of the two count kernels.  off: [ng + 1] item offsets of the groups (every group owns at least one item), off[ng] = P.
// Workgroup b owns the items [b per, (b + 1) per): it finds the group of its first item by binary search and walks forward 256 items at a
// time through a window of 257 offsets in LDS; every lane finds its item's group in the window and calls cell(group, item within the
// group).  G is the type of a group index: the caller's, so that a walk over fewer than 2^32 groups does its searches in 32 bits.
template <typename G, typename Cell>
__device__ __forceinline__ void item_walk(const unsigned long long* __restrict__ off, G ng, unsigned long long P, unsigned long long per, Cell cell) {
  __shared__ unsigned long long loff[257];
  __shared__ G next_group;
  const unsigned long long a = (unsigned long long)blockIdx.x * per;
  const unsigned long long b = a + per < P ? a + per : P;
  if (a >= b) return;
  G lo = 0, hi = ng - 1u;      // the group of item a: the last one whose offset is <= a (uniform over the workgroup)
  while (lo < hi) { const G mid = (lo + hi + 1u) >> 1; if (off[mid] <= a) lo = mid; else hi = mid - 1u; }
  G gc = lo;
  for (unsigned long long ta = a; ta < b; ta += 256ull) {
    // items ta ... ta + 255 lie in the groups gc ... gc + 255 at most (a group owns an item or more): their offsets, and the one after
    for (uint32_t w = threadIdx.x; w < 257u; w += blockDim.x) loff[w] = (unsigned long long)gc + w <= ng ? off[gc + w] : P;
    __syncthreads();
    const unsigned long long t = ta + threadIdx.x;
    if (t < b) {
      uint32_t wl = 0, wh = 255;      // the last window entry whose offset is <= t (entries past the last group hold P > t)
      while (wl < wh) { const uint32_t mid = (wl + wh + 1u) >> 1; if (loff[mid] <= t) wl = mid; else wh = mid - 1u; }
      const G g = gc + wl;
      if (g < ng) cell(g, t - loff[wl]);
      if (threadIdx.x == 255u) next_group = loff[wl + 1u] <= t + 1ull ? g + 1u : g;      // the group of item ta + 256
    }
    __syncthreads();
    gc = next_group;      // (read only when another round follows: then lane 255 had an item)
  }
}

// C3: item t of slice group g -> (i, j), i < j, of its genomes: shared[g_i n + g_j] += 1
__global__ __launch_bounds__(256) void screen_count_kernel(const unsigned long long* __restrict__ u, const uint32_t* __restrict__ first,
                                                            const uint32_t* __restrict__ last, const unsigned long long* __restrict__ off, uint32_t ng,
                                                            unsigned long long P, unsigned long long per, uint32_t n, uint32_t* __restrict__ shared) {
  item_walk<uint32_t>(off, ng, P, per, [=](uint32_t g, unsigned long long t) {
    const uint32_t s = first[g], m = last[g] - s + 1u;
    uint32_t i, j;
    pgscr::screen_tri_decode(t, m, &i, &j);
    const uint32_t gi = (uint32_t)u[s + i], gj = (uint32_t)u[s + j];
    if (j < m && gi < n && gj < n) atomicAdd(&shared[(size_t)gi * n + gj], 1u);
  });
}

__global__ __launch_bounds__(256) void screen_finish_kernel(uint32_t* __restrict__ shared, const uint32_t* __restrict__ sizes, uint32_t n) {
  const uint64_t cells = (uint64_t)n * n;
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < cells; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t a = (uint32_t)(x / n), b = (uint32_t)(x % n);
    if (a == b) shared[x] = sizes[a];
    else if (a > b) shared[x] = shared[(size_t)b * n + a];
  }
}

// the launch shape of a walk over P items: at most 2048 items a workgroup while the device has workgroups to spare
unsigned long long items_per_workgroup(const pg_ctx* ctx, unsigned long long P) {
  const uint64_t n_wg = std::max<uint64_t>(1, std::min<uint64_t>((P + 2047) / 2048, (uint64_t)ctx->num_cu * 32));
  return (P + n_wg - 1) / n_wg;
}

// the argument checks of pg_screen_matrix and pg_screen_hold (want_shared: the call has a matrix to copy out, shared_out)
int screen_check(pg_ctx* ctx, const int32_t* genome_ids, uint32_t n, int32_t kmer, int32_t scale, uint32_t part, uint32_t n_parts, const uint32_t* sizes_out,
                 bool want_shared, const uint32_t* shared_out, uint32_t max_n = pgscr::MAX_GENOMES,
                 const char* too_many = "screen: more than 8192 genomes in one call") {
  if (n > max_n) return pg_fail(ctx, PG_E_ARG, too_many);      // (before the ids are read)
  if (n && (!genome_ids || !sizes_out || (want_shared && !shared_out))) return pg_fail(ctx, PG_E_ARG, "bad argument");
  if (kmer < pgs::K_MIN || kmer > pgs::K_MAX) return pg_fail(ctx, PG_E_ARG, "screen: the k-mer size must be 8 ... 16");
  if (!pgscr::valid_scale(scale)) return pg_fail(ctx, PG_E_ARG, "screen: scale must be a power of two, 1 ... 65536");
  if (n_parts < 1 || n_parts > pgscr::N_BINS || part >= n_parts) return pg_fail(ctx, PG_E_ARG, "screen: 1 <= n_parts <= 4096 and part < n_parts");
  std::vector<char> seen(ctx->genomes.size(), 0);
  for (uint32_t i = 0; i < n; ++i) {
    if (genome_ids[i] < 0 || (size_t)genome_ids[i] >= ctx->genomes.size()) return pg_fail(ctx, PG_E_ARG, "genome id out of range");
    if (seen[genome_ids[i]]) return pg_fail(ctx, PG_E_ARG, "screen: genome id " + std::to_string(genome_ids[i]) + " is given twice");
    seen[genome_ids[i]] = 1;
  }
  return PG_OK;
}

struct SliceGroups {      // one slice, sorted and grouped, on the device: what the front half hands to a back half
  const unsigned long long* u;      // the nu distinct keys, sorted
  uint64_t nu;
  const uint8_t* flags;             // of the head kernel, one per key
  const uint32_t* first;            // the first and the last entry of each of the ng k-mers held by >= 2 genomes
  const uint32_t* last;
  uint64_t ng;
  const uint32_t* mult;             // with_mult: the times the fill pass appended each distinct key (its run in the sorted keys); else nullptr
  void* tmp;                        // temporary storage of the library calls: what the front half needs, and what prepare() asked for
  size_t tmp_bytes;
  uint32_t bin_lo, bin_hi;          // the slice's bins [bin_lo, bin_hi)
};

struct FrontTotals { uint64_t keys = 0, distinct = 0, groups = 0, slices = 0; };

struct AsU64 {      // a run length read as a 64-bit term of a sum
  __host__ __device__ __forceinline__ unsigned long long operator()(uint32_t x) const { return x; }
};

// The FRONT HALF of a screen of checked arguments (n >= 1), shared by the dense calls and the index: the count pass, slices of whole bins
// under the budget, and per slice the fill pass, the radix sort, Unique and the head kernel's sizes and first / last marks (C1, C2).
// What becomes of a grouped slice is the back half's: back.prepare(all keys, keys of the largest slice, its bound of groups, tmp bytes to
// raise) once before the first slice, back.slice(S, T) per slice.  d_sizes (the caller's, empty) holds the finished sizes on return.
// wide_head: screen_head_kernel<true> (any n, bit 2 of the flags) instead of the LDS histogram of at most MAX_GENOMES genomes.
// with_mult (the abundance count of the gather, DESIGN.md §16.8; off for every other caller): the sorted keys go through
// DeviceRunLengthEncode::Encode in place of Unique — the same distinct keys, and SliceGroups::mult = the length of each one's run.  A
// k-mer lies in one bin, a bin in one slice and a slice holds at most 2^30 keys: a run length never reaches the uint32's end.
template <typename Back>
int screen_front(pg_ctx* ctx, const int32_t* genome_ids, uint32_t n, int32_t kmer, int32_t scale, uint32_t part, uint32_t n_parts, bool wide_head,
                 PgDevBuf<uint32_t>& d_sizes, ScreenEvents& T, FrontTotals& tot, Back& back, bool with_mult = false) {
  int rc;
  const auto scan_count = screen_scan_of<false>(kmer);
  const auto scan_fill = screen_scan_of<true>(kmer);
  if (!scan_count || !scan_fill) return pg_fail(ctx, PG_E_ARG, "screen: no scan kernel for this k-mer size");
  uint32_t log2_scale = 0;
  while ((1 << log2_scale) < scale) ++log2_scale;
  const uint32_t bin_lo = pgscr::part_begin(part, n_parts), bin_hi = pgscr::part_begin(part + 1u, n_parts);
  const uint64_t max_keys = ctx->screen_max_keys ? ctx->screen_max_keys : pgscr::DEFAULT_MAX_KEYS;
  hipStream_t st = ctx->stream;
  const uint32_t cu_blocks = (uint32_t)ctx->num_cu * 8u;

  // the prefix table over the genomes
  std::vector<ScreenGenome> tab(n);
  uint64_t n_items = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const PgGenome& G = ctx->genomes[genome_ids[i]];
    tab[i].arena_start = G.arena_start; tab[i].stream_len = (int64_t)G.stream_len; tab[i].item0 = n_items;
    const uint64_t chunks = (G.stream_len + 31) / 32;
    n_items += (chunks + SCAN_CHUNKS - 1) / SCAN_CHUNKS;
  }
  PgDevBuf<ScreenGenome> d_tab;
  PgDevBuf<unsigned long long> d_hist, d_counters;      // [N_BINS] | [0] append cursor, [1] distinct keys, [2] groups
  if ((rc = sk_malloc(ctx, d_tab, n)) || (rc = sk_malloc(ctx, d_hist, pgscr::N_BINS)) || (rc = sk_malloc(ctx, d_counters, 4)) ||
      (rc = sk_malloc(ctx, d_sizes, n)))
    return rc;
  PG_HIP(ctx, hipMemcpyAsync(d_tab, tab.data(), (size_t)n * sizeof(ScreenGenome), hipMemcpyHostToDevice, st));
  PG_HIP(ctx, hipMemsetAsync(d_hist, 0, pgscr::N_BINS * 8, st));
  PG_HIP(ctx, hipMemsetAsync(d_sizes, 0, (size_t)n * 4, st));
  const dim3 scan_grid(grid_for(n_items, 1, cu_blocks));
  std::vector<unsigned long long> hist(pgscr::N_BINS, 0ull);
  if (n_items) {
    {
      ScreenEvents::Stage scan(T, ST_SCAN, st);
      hipLaunchKernelGGL(scan_count, scan_grid, dim3(256), 0, st, ctx->d_codes.p, ctx->d_mask.p, d_tab.p, n, n_items, (uint32_t)scale, log2_scale, bin_lo,
                         bin_hi, d_hist.p, (unsigned long long*)nullptr, 0ull, (unsigned long long*)nullptr);
    }
    PG_HIP(ctx, hipGetLastError());
    PG_HIP(ctx, hipMemcpyAsync(hist.data(), d_hist, pgscr::N_BINS * 8, hipMemcpyDeviceToHost, st));
    PG_HIP(ctx, hipStreamSynchronize(st));
  }
  // contiguous slices of at most max_keys keys
  struct Slice { uint32_t lo, hi; uint64_t keys; };
  std::vector<Slice> slices;
  uint64_t total_keys = 0, slice_max = 0;
  {
    Slice cur{bin_lo, bin_lo, 0};
    for (uint32_t bin = bin_lo; bin < bin_hi; ++bin) {
      const uint64_t c = hist[bin];
      if (c > max_keys)
        return pg_fail(ctx, PG_E_NOMEM, "screen: slice bin " + std::to_string(bin) + " alone holds " + std::to_string(c) + " keys, more than the budget of " +
                                            std::to_string(max_keys) + " keys of one slice (pg_screen_set_budget; a larger scale or more parts make the bins smaller)");
      if (cur.keys + c > max_keys) { slices.push_back(cur); cur = Slice{bin, bin, 0}; }
      cur.keys += c; cur.hi = bin + 1u;
    }
    if (cur.keys) slices.push_back(cur);
    for (const Slice& s : slices) { total_keys += s.keys; slice_max = std::max(slice_max, s.keys); }
  }
  tot.keys = total_keys; tot.slices = slices.size();
  if (!slices.empty()) {
    PgDevBuf<unsigned long long> keys_a, keys_b;
    PgDevBuf<uint32_t> first, last, mult;
    PgDevBuf<uint8_t> flags, tmp;
    const size_t max_groups = (size_t)(slice_max / 2 + 2);
    if ((rc = sk_malloc(ctx, keys_a, (size_t)slice_max + 1)) || (rc = sk_malloc(ctx, keys_b, (size_t)slice_max + 1)) ||
        (rc = sk_malloc(ctx, flags, (size_t)slice_max + 1)) || (rc = sk_malloc(ctx, first, max_groups)) || (rc = sk_malloc(ctx, last, max_groups)))
      return rc;
    if (with_mult && (rc = sk_malloc(ctx, mult, (size_t)slice_max + 1))) return rc;
    // temporary storage of the library calls: the largest any of them asks for at the largest slice
    const int end_bit = 32 + 2 * kmer;
    unsigned long long* d_nu = d_counters.p + 1;
    unsigned long long* d_ng = d_counters.p + 2;
    unsigned long long* d_runs = d_counters.p + 3;      // with_mult: the sum of a slice's run lengths
    hipcub::TransformInputIterator<unsigned long long, AsU64, const uint32_t*> run_len((const uint32_t*)mult.p, AsU64{});
    hipcub::CountingInputIterator<uint32_t> counting(0u);
    hipcub::TransformInputIterator<uint8_t, FlagBit, const uint8_t*> is_first(flags.p, FlagBit{0u}), is_last(flags.p, FlagBit{1u});
    size_t tmp_bytes = 0;
    PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& b) {
      return hipcub::DeviceRadixSort::SortKeys(nullptr, b, (const unsigned long long*)keys_a.p, keys_b.p, (int64_t)slice_max, 0, end_bit, st); }));
    PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& b) {
      return hipcub::DeviceSelect::Unique(nullptr, b, (const unsigned long long*)keys_b.p, keys_a.p, d_nu, (int64_t)slice_max, st); }));
    PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& b) { return hipcub::DeviceSelect::Flagged(nullptr, b, counting, is_first, first.p, d_ng, (int64_t)slice_max, st); }));
    if (with_mult) {
      PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& b) {
        return hipcub::DeviceRunLengthEncode::Encode(nullptr, b, (const unsigned long long*)keys_b.p, keys_a.p, mult.p, d_nu, (int)slice_max, st); }));
      PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& b) { return hipcub::DeviceReduce::Sum(nullptr, b, run_len, d_runs, (int)slice_max, st); }));
    }
    if ((rc = back.prepare(total_keys, slice_max, max_groups, tmp_bytes))) return rc;
    if ((rc = sk_malloc(ctx, tmp, tmp_bytes + 16))) return rc;

    for (const Slice& S : slices) {
      {      // fill
        ScreenEvents::Stage scan(T, ST_SCAN, st);
        PG_HIP(ctx, hipMemsetAsync(d_counters, 0, 4 * 8, st));
        hipLaunchKernelGGL(scan_fill, scan_grid, dim3(256), 0, st, ctx->d_codes.p, ctx->d_mask.p, d_tab.p, n, n_items, (uint32_t)scale, log2_scale, S.lo, S.hi,
                           (unsigned long long*)nullptr, keys_a.p, (unsigned long long)S.keys, d_counters.p);
      }
      PG_HIP(ctx, hipGetLastError());
      unsigned long long cnt[3] = {0, 0, 0};      // cursor, distinct, groups
      unsigned long long runs = 0;
      uint64_t nu = 0;
      {      // sort, drop a genome's repeats, mark the groups
        ScreenEvents::Stage group(T, ST_GROUP, st);
        size_t tb = tmp_bytes;
        PG_HIP(ctx, hipcub::DeviceRadixSort::SortKeys((void*)tmp.p, tb, (const unsigned long long*)keys_a.p, keys_b.p, (int64_t)S.keys, 0, end_bit, st));
        tb = tmp_bytes;
        if (!with_mult) {
          PG_HIP(ctx, hipcub::DeviceSelect::Unique((void*)tmp.p, tb, (const unsigned long long*)keys_b.p, keys_a.p, d_nu, (int64_t)S.keys, st));
        } else {      // the distinct keys with the length of each one's run
          PG_HIP(ctx, hipcub::DeviceRunLengthEncode::Encode((void*)tmp.p, tb, (const unsigned long long*)keys_b.p, keys_a.p, mult.p, d_nu, (int)S.keys, st));
        }
        PG_HIP(ctx, hipMemcpyAsync(cnt, d_counters, 2 * 8, hipMemcpyDeviceToHost, st));
        PG_HIP(ctx, hipStreamSynchronize(st));
        if (cnt[0] != S.keys)
          return pg_fail(ctx, PG_E_INTERNAL, "screen: the fill pass appended " + std::to_string(cnt[0]) + " keys where the count pass saw " + std::to_string(S.keys));
        nu = cnt[1];
        tot.distinct += nu;
        if (with_mult) {      // every key of the slice lies in exactly one run
          if (nu > S.keys) return pg_fail(ctx, PG_E_INTERNAL, "screen: more runs than keys in a slice");
          tb = tmp_bytes;
          PG_HIP(ctx, hipcub::DeviceReduce::Sum((void*)tmp.p, tb, run_len, d_runs, (int)nu, st));
          PG_HIP(ctx, hipMemcpyAsync(&runs, d_runs, 8, hipMemcpyDeviceToHost, st));
        }
        hipLaunchKernelGGL(wide_head ? screen_head_kernel<true> : screen_head_kernel<false>, dim3(grid_for(nu, 256 * 16, cu_blocks)), dim3(256), 0, st,
                           (const unsigned long long*)keys_a.p, nu, n, d_sizes.p, flags.p);
        PG_HIP(ctx, hipGetLastError());
        tb = tmp_bytes;
        PG_HIP(ctx, hipcub::DeviceSelect::Flagged((void*)tmp.p, tb, counting, is_first, first.p, d_ng, (int64_t)nu, st));
        tb = tmp_bytes;
        PG_HIP(ctx, hipcub::DeviceSelect::Flagged((void*)tmp.p, tb, counting, is_last, last.p, d_ng, (int64_t)nu, st));
        PG_HIP(ctx, hipMemcpyAsync(&cnt[2], d_ng, 8, hipMemcpyDeviceToHost, st));
      }
      PG_HIP(ctx, hipStreamSynchronize(st));
      const uint64_t ng = cnt[2];
      if (with_mult && runs != S.keys)
        return pg_fail(ctx, PG_E_INTERNAL, "screen: the runs of a slice hold " + std::to_string(runs) + " keys where the fill pass appended " + std::to_string(S.keys));
      if (ng + 1 > max_groups) return pg_fail(ctx, PG_E_INTERNAL, "screen: more groups than half the keys");
      tot.groups += ng;
      const SliceGroups G{keys_a.p, nu, flags.p, first.p, last.p, ng, with_mult ? (const uint32_t*)mult.p : nullptr, (void*)tmp.p, tmp_bytes, S.lo, S.hi};
      if ((rc = back.slice(G, T))) return rc;
    }
  }
  return PG_OK;
}

// The back half of the dense calls (C2's item ranges, C3): every grouped slice is counted into the n x n matrix.
struct DenseBack {
  pg_ctx* ctx;
  uint32_t n;
  uint32_t* d_shared;
  PgDevBuf<unsigned long long> wts, off;
  uint64_t n_incr = 0;
  int prepare(uint64_t, uint64_t, size_t max_groups, size_t& tmp_bytes) {
    int rc;
    if ((rc = sk_malloc(ctx, wts, max_groups)) || (rc = sk_malloc(ctx, off, max_groups))) return rc;
    PG_HIP(ctx, tmp_room(tmp_bytes, [&](size_t& b) { return hipcub::DeviceScan::ExclusiveSum(nullptr, b, wts.p, off.p, (int64_t)max_groups, ctx->stream); }));
    return PG_OK;
  }
  int slice(const SliceGroups& S, ScreenEvents& T) {
    hipStream_t st = ctx->stream;
    unsigned long long P = 0;
    if (S.ng) {
      {
        ScreenEvents::Stage group(T, ST_GROUP, st);
        PG_HIP(ctx, screen_weights(ctx, S.ng, wts.p, TriWeight{S.first, S.last}));
        size_t tb = S.tmp_bytes;
        PG_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(S.tmp, tb, wts.p, off.p, (int64_t)(S.ng + 1), st));
        PG_HIP(ctx, hipMemcpyAsync(&P, off.p + S.ng, 8, hipMemcpyDeviceToHost, st));
      }
      PG_HIP(ctx, hipStreamSynchronize(st));
    }
    n_incr += P;
    if (P) {
      const unsigned long long per = items_per_workgroup(ctx, P);
      {
        ScreenEvents::Stage count(T, ST_COUNT, st);
        hipLaunchKernelGGL(screen_count_kernel, dim3((uint32_t)((P + per - 1) / per)), dim3(256), 0, st, S.u, S.first, S.last, (const unsigned long long*)off.p,
                           (uint32_t)S.ng, P, per, n, d_shared);
      }
      PG_HIP(ctx, hipGetLastError());
    }
    return PG_OK;
  }
};

// The screen of checked arguments.  The finished matrix is left in d_shared (the caller's: pg_screen_matrix lets it go, pg_screen_hold keeps
// it); sizes_out, and shared_out where it is given, are on the host when this returns.
int screen_run(pg_ctx* ctx, const int32_t* genome_ids, uint32_t n, int32_t kmer, int32_t scale, uint32_t part, uint32_t n_parts, uint32_t* sizes_out,
               uint32_t* shared_out, PgDevBuf<uint32_t>& d_shared) {
  ctx->screen_stats = PgScreenStats{};
  if (n == 0) return PG_OK;
  PG_HIP(ctx, hipSetDevice(ctx->device));
  int rc;
  if ((rc = pg_upload(ctx))) return rc;
  hipStream_t st = ctx->stream;
  if ((rc = sk_malloc(ctx, d_shared, (size_t)n * n))) return rc;
  PG_HIP(ctx, hipMemsetAsync(d_shared, 0, (size_t)n * n * 4, st));
  PgDevBuf<uint32_t> d_sizes;
  ScreenEvents T;
  FrontTotals tot;
  DenseBack back{ctx, n, d_shared.p};
  if ((rc = screen_front(ctx, genome_ids, n, kmer, scale, part, n_parts, false, d_sizes, T, tot, back))) return rc;
  hipLaunchKernelGGL(screen_finish_kernel, dim3(grid_for((uint64_t)n * n, 256 * 4, (uint32_t)ctx->num_cu * 8u)), dim3(256), 0, st, d_shared.p,
                     (const uint32_t*)d_sizes.p, n);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(sizes_out, d_sizes, (size_t)n * 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && shared_out) e = hipMemcpyAsync(shared_out, d_shared, (size_t)n * n * 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return pg_fail(ctx, PG_E_HIP, std::string("screen: ") + hipGetErrorString(e));
  PgScreenStats& L = ctx->screen_stats;
  L.keys = tot.keys; L.distinct = tot.distinct; L.groups = tot.groups; L.pair_increments = back.n_incr; L.slices = tot.slices;
  L.scan_ms = T.ms(ST_SCAN); L.group_ms = T.ms(ST_GROUP); L.count_ms = T.ms(ST_COUNT);
  return PG_OK;
}

}  // namespace

extern "C" int pg_screen_set_budget(pg_ctx* ctx, uint64_t max_keys) {
  if (!ctx) return PG_E_ARG;
  if (max_keys > pgscr::LIMIT_MAX_KEYS) return pg_fail(ctx, PG_E_ARG, "screen: the key budget of a slice is at most 2^30");
  ctx->screen_max_keys = max_keys;
  return PG_OK;
}

extern "C" int pg_screen_last(pg_ctx* ctx, uint64_t* out5, double* ms3) {
  if (!ctx || !out5 || !ms3) return pg_fail(ctx, PG_E_ARG, "bad argument");
  const PgScreenStats& L = ctx->screen_stats;
  out5[0] = L.keys; out5[1] = L.distinct; out5[2] = L.groups; out5[3] = L.pair_increments; out5[4] = L.slices;
  ms3[0] = L.scan_ms; ms3[1] = L.group_ms; ms3[2] = L.count_ms;
  return PG_OK;
}

extern "C" int pg_screen_matrix(pg_ctx* ctx, const int32_t* genome_ids, uint32_t n, int32_t kmer, int32_t scale, uint32_t part, uint32_t n_parts,
                                uint32_t* sizes_out, uint32_t* shared_out) {
  if (!ctx) return PG_E_ARG;
  int rc;
  if ((rc = screen_check(ctx, genome_ids, n, kmer, scale, part, n_parts, sizes_out, true, shared_out))) return rc;
  PgDevBuf<uint32_t> d_shared;
  return screen_run(ctx, genome_ids, n, kmer, scale, part, n_parts, sizes_out, shared_out, d_shared);
}
