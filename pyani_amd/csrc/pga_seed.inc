// pga_seed.inc — part of pg_anim.hip (included inside its anonymous namespace; not a translation unit of its own):
// A1/A2: seed lists, the probe kernel, hit verification / extension, dealing matches into unit slices.

// ---- A1/A2: seeding ------------------------------------------------------------------------------------------------
// Every maximal exact match of length >= MIN_MATCH (20) contains, whatever its offset, a query-strand position that is a
// multiple of SEED_STEP and starts a SEED_K-mer lying wholly inside the match (SEED_K + SEED_STEP - 1 == MIN_MATCH).  So
// the reference lists its 16-mers at EVERY position and the query strand is looked up at every 5th position only; of
// the sampled positions inside one match, the first (left extension < SEED_STEP) is the one that reports it.
constexpr int SEED_K = 16, SEED_STEP = 5;
static_assert(SEED_K + SEED_STEP - 1 == MIN_MATCH, "sampling must not miss a minimal-length match");

// 16-mer (first base in the low bits) of strand `strand` at strand position q (q + 16 <= len), false if a base is dirty
__device__ __forceinline__ bool seed_kmer(const uint32_t* __restrict__ codes, const uint32_t* __restrict__ mask, int32_t len,
                                          int32_t strand, int32_t q, uint32_t& k) {
  uint32_t c, m;
  if (strand == 0) {
    get16(codes, mask, q, c, m);
    k = c;
  } else {
    get16(codes, mask, len - SEED_K - q, c, m);  // forward window holding the same bases
    uint32_t x = __brev(c);
    x = ((x & 0xAAAAAAAAu) >> 1) | ((x & 0x55555555u) << 1);
    k = ~x;
  }
  return m == 0xFFFFu;
}

// Hash of a seed k-mer: the top SEED_GROUP_BITS (14) select the group (partition of the k-mer space shared by all genomes).
// The per-pair probe kernel works on COARSE groups (the top 11 bits: eight consecutive groups); the block kernel on the
// groups themselves.  Lists are laid out so that both views are contiguous (below).
constexpr int SEED_GROUP_BITS = 14, SEED_GROUPS = 1 << SEED_GROUP_BITS;
constexpr int SEED_CGROUP_BITS = 11, SEED_CGROUPS = 1 << SEED_CGROUP_BITS, SEED_SUB = SEED_GROUPS / SEED_CGROUPS;
constexpr uint32_t SEED_MAX_SLOTS = 16384;   // 128 KiB of LDS
__device__ __forceinline__ uint32_t seed_hash(uint32_t k) { return k * 0x9E3779B1u; }
__device__ __forceinline__ uint32_t seed_group(uint32_t h) { return h >> (32 - SEED_GROUP_BITS); }

// Per-genome seed lists.  role 0 (reference): every stream position, 1 sub-list per group (coarse group c = sub-lists
// [8 c, 8 c + 8)); role 1 (query): every SEED_STEP-th position of both strands, sub-list index of (group g, strand s) =
// (2 (g >> 3) + s) * 8 + (g & 7) — coarse group c and strand s = sub-lists [16 c + 8 s, 16 c + 8 s + 8).
// Entry (64 bit): [63:43] low 21 bits of the k-mer hash (the hash is a bijection of the 32-bit k-mer and its top 11 bits
// are the coarse group, so these 21 bits identify the k-mer within it; the low 18 identify it within its group) | [42:33]
// the SEED_STEP bases to the LEFT of the k-mer, nearest first | [32] 1 = all of them exist and are clean | [31:0] position.
// With both flags set, the left-maximality test of a hit needs no memory access at all.
// pass 0 counts into cnt[], pass 1 writes at goff[] + cursor (cnt[] re-zeroed in between by anim_list_scan_kernel).
constexpr uint64_t SEED_KEY_SHIFT = 43;
constexpr int LIST_BLOCK = 1024, LIST_CHUNK = 16384;   // positions (or sampled positions) per workgroup
__device__ __forceinline__ uint32_t seed_sub(uint32_t g, int role, uint32_t strand) {
  return role ? ((2u * (g >> 3) + strand) << 3) + (g & 7u) : g;
}
__global__ __launch_bounds__(LIST_BLOCK) void anim_list_kernel(const uint32_t* __restrict__ codes, const uint32_t* __restrict__ mask,
                                                               int32_t len, int role, uint32_t* __restrict__ cnt,
                                                               const uint32_t* __restrict__ goff, uint64_t* __restrict__ list, int pass,
                                                               int step) {
  // Sub-list counters are kept per workgroup in LDS (dynamic: n_sub words, 64 KiB for the reference role, 128 KiB for the
  // query role); the global counters see one atomic per (workgroup, non-empty sub-list) instead of one per k-mer.  pass 1
  // counts again, reserves a range per sub-list, then writes.
  extern __shared__ uint32_t s_cnt[];
  const int32_t strand = role ? (int32_t)blockIdx.y : 0;
  const uint32_t n_sub = role ? 2 * SEED_GROUPS : SEED_GROUPS;
  const int32_t idx0 = blockIdx.x * LIST_CHUNK;
  for (uint32_t i = threadIdx.x; i < n_sub; i += LIST_BLOCK) s_cnt[i] = 0;
  __syncthreads();
  auto kmer_of = [&](int32_t idx, uint32_t& h, int32_t& p) -> bool {
    p = role ? idx * step : idx;   // query role: every step-th strand position (SEED_STEP for ANIm, 1 in fragment mode)
    if (p + SEED_K > len) return false;
    uint32_t k;
    if (!seed_kmer(codes, mask, len, strand, p, k)) return false;
    h = seed_hash(k);
    return true;
  };
  auto sub_of = [&](uint32_t h) { return seed_sub(seed_group(h), role, (uint32_t)strand); };
  for (int32_t t = threadIdx.x; t < LIST_CHUNK; t += LIST_BLOCK) {
    uint32_t h; int32_t p;
    if (kmer_of(idx0 + t, h, p)) atomicAdd(&s_cnt[sub_of(h)], 1u);
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n_sub; i += LIST_BLOCK) {
    const uint32_t c = s_cnt[i];
    uint32_t base = 0;
    if (c) base = atomicAdd(&cnt[i], c);
    s_cnt[i] = pass ? goff[i] + base : 0;   // pass 1: this workgroup's write cursor in sub-list i
  }
  if (!pass) return;
  __syncthreads();
  const StrandView V{SeqView{codes, mask, len}, strand};
  for (int32_t t = threadIdx.x; t < LIST_CHUNK; t += LIST_BLOCK) {
    uint32_t h; int32_t p;
    if (!kmer_of(idx0 + t, h, p)) continue;
    const uint32_t at = atomicAdd(&s_cnt[sub_of(h)], 1u);
    uint64_t left = 0, flag = 1;
    for (int j = 1; j <= SEED_STEP; ++j) {
      if (!V.clean(p - j)) { flag = 0; left = 0; break; }
      left |= (uint64_t)V.base(p - j) << (2 * (j - 1));
    }
    list[at] = ((uint64_t)(h & 0x1FFFFFu) << SEED_KEY_SHIFT) | (left << 33) | (flag << 32) | (uint32_t)p;
  }
}

// goff[0..n] = exclusive prefix of cnt[0..n), goff[n + 1] = largest sub-list, goff[n + 2] = largest run of SEED_SUB
// aligned sub-lists (a coarse group of the reference role); cnt re-zeroed.  n = PER * 1024 (SEED_GROUPS or 2 * SEED_GROUPS):
// each thread owns PER consecutive counters (a multiple of SEED_SUB), loaded and stored as 16-byte vectors.
constexpr int LIST_SCAN_BLOCK = 1024;
template <int PER>
__global__ __launch_bounds__(LIST_SCAN_BLOCK) void anim_list_scan_kernel(uint32_t* __restrict__ cnt, uint32_t* __restrict__ goff) {
  static_assert(PER % SEED_SUB == 0 && PER % 4 == 0, "a thread owns whole coarse groups");
  constexpr uint32_t n = PER * LIST_SCAN_BLOCK;
  __shared__ uint32_t s_sum[LIST_SCAN_BLOCK / 64], s_mx[LIST_SCAN_BLOCK / 64], s_cmx[LIST_SCAN_BLOCK / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint4* const c4 = reinterpret_cast<uint4*>(cnt + tid * PER);
  uint32_t c[PER];
#pragma unroll
  for (int i = 0; i < PER / 4; ++i) {
    const uint4 v = c4[i];
    c[4 * i] = v.x; c[4 * i + 1] = v.y; c[4 * i + 2] = v.z; c[4 * i + 3] = v.w;
    c4[i] = make_uint4(0, 0, 0, 0);
  }
  uint32_t sum = 0, mx = 0, cmx = 0;
#pragma unroll
  for (int i = 0; i < PER; i += SEED_SUB) {
    uint32_t run8 = 0;
#pragma unroll
    for (int j = 0; j < SEED_SUB; ++j) { run8 += c[i + j]; mx = c[i + j] > mx ? c[i + j] : mx; }
    sum += run8;
    cmx = run8 > cmx ? run8 : cmx;
  }
  uint32_t incl = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o, 64); if ((int)lane >= o) incl += t; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    uint32_t t = __shfl_xor(mx, o, 64); mx = t > mx ? t : mx;
    t = __shfl_xor(cmx, o, 64); cmx = t > cmx ? t : cmx;
  }
  if (lane == 63) s_sum[wave] = incl;
  if (lane == 0) { s_mx[wave] = mx; s_cmx[wave] = cmx; }
  __syncthreads();
  uint32_t run = incl - sum;
  for (uint32_t w = 0; w < wave; ++w) run += s_sum[w];
  uint4* const g4 = reinterpret_cast<uint4*>(goff + tid * PER);
#pragma unroll
  for (int i = 0; i < PER / 4; ++i) {
    uint4 v;
    v.x = run; run += c[4 * i];
    v.y = run; run += c[4 * i + 1];
    v.z = run; run += c[4 * i + 2];
    v.w = run; run += c[4 * i + 3];
    g4[i] = v;
  }
  if (tid == LIST_SCAN_BLOCK - 1) {
    goff[n] = run;
    uint32_t m = 0, cm = 0;
    for (uint32_t w = 0; w < LIST_SCAN_BLOCK / 64; ++w) { m = s_mx[w] > m ? s_mx[w] : m; cm = s_cmx[w] > cm ? s_cmx[w] : cm; }
    goff[n + 1] = m;
    goff[n + 2] = cm;
  }
}

struct SeedRef {            // one per reference of the batch (per-pair kernel)
  const uint64_t* list;
  const uint32_t* goff;     // SEED_GROUPS + 3
  uint32_t pair_begin, pair_end;
};
struct SeedQry {            // one per pair of the batch (its query genome)
  const uint64_t* list;
  const uint32_t* goff;     // 2 * SEED_GROUPS + 3
};
// Per batch, transposed: slice[c * n_pairs + p] = where pair p's query keeps coarse group c.  A wave reads the descriptors of
// 64 of its pairs with ONE coalesced load instead of chasing pair -> offset table -> entries once per pair.
struct SeedSlice { uint32_t begin, n0, n1; };   // strand-0 entries [begin, begin + n0), strand-1 [begin + n0, begin + n0 + n1)
__global__ __launch_bounds__(256) void anim_slice_kernel(const SeedQry* __restrict__ sqry, uint32_t n_pairs, SeedSlice* __restrict__ slice) {
  const uint32_t p = blockIdx.x;
  const uint32_t* goff = sqry[p].goff;
  for (uint32_t g = threadIdx.x; g < SEED_CGROUPS; g += 256) {
    if (!goff) { slice[(size_t)g * n_pairs + p] = SeedSlice{0, 0, 0}; continue; }   // not seeded: mirrored from its partner pair
    const uint32_t o0 = goff[2 * SEED_SUB * g], o1 = goff[2 * SEED_SUB * g + SEED_SUB], o2 = goff[2 * SEED_SUB * (g + 1)];
    slice[(size_t)g * n_pairs + p] = SeedSlice{o0, o1 - o0, o2 - o1};
  }
}

// One hit of a sampled query k-mer (strand position q) on reference position r: report the maximal match it lies in,
// unless an earlier sampled position of the same match does.  Returns false if nothing is to be appended.
__device__ __forceinline__ bool seed_hit(const RefDesc& R, const SeqView& RV, const UnitDesc& U0, const StrandView& QV, int strand,
                                         int32_t r, int32_t q, int32_t left, int32_t min_match, int32_t step, Match& out) {
  if (left < 0) {   // left context not decidable from the list entries (sequence start / ambiguity symbol nearby)
    left = 0;
    while (left < step && RV.clean(r - 1 - left) && QV.clean(q - 1 - left) && RV.base(r - 1 - left) == QV.base(q - 1 - left)) ++left;
  }
  if (left >= step) return false;   // an earlier sampled position of the same match reports it
  int32_t L = SEED_K;
  // right extension, 16 bases per step (word compare of the packed codes and masks), then base by base near a sequence
  // end.  Single-exit loops (state in `n`): break / continue shapes cost a lot of exec-mask bookkeeping.
  int n = 16;
  while (n == 16 && r + L + 16 <= R.len && q + L + 16 <= U0.len) {
    uint32_t rc_, rm_, qc_, qm_;
    get16(R.codes, R.mask, r + L, rc_, rm_);
    uint32_t fc, fm;
    get16(U0.codes, U0.mask, strand == 0 ? q + L : U0.len - 16 - (q + L), fc, fm);
    uint32_t rv = __brev(fc);
    rv = ((rv & 0xAAAAAAAAu) >> 1) | ((rv & 0x55555555u) << 1);
    qc_ = strand == 0 ? fc : ~rv;
    qm_ = strand == 0 ? fm : __brev(fm) >> 16;
    const uint32_t x = rc_ ^ qc_;
    const uint32_t diff = (x | (x >> 1)) & 0x55555555u;
    const uint32_t bad = ~(rm_ & qm_) & 0xFFFFu;
    const int nd = diff ? (__ffs(diff) - 1) >> 1 : 16;
    const int nb = bad ? __ffs(bad) - 1 : 16;
    n = nd < nb ? nd : nb;
    L += n;
  }
  if (n == 16)   // fewer than 16 bases left in one of the sequences
    while (RV.clean(r + L) && QV.clean(q + L) && RV.base(r + L) == QV.base(q + L)) ++L;
  if (left + L < min_match) return false;   // MIN_MATCH (20) for ANIm; fragment mode keeps every sampled 16-mer hit
  out = Match{r - left, q - left, left + L, 0};
  return true;
}

// A hit that may start a match: handed to anim_hit_kernel (verification / extension need the sequences and many registers;
// keeping them out of the probe kernels doubles their waves per SIMD).  Staged per wave in LDS.
constexpr int SEED_BLOCK = 1024, SEED_UNROLL = 4;
constexpr uint32_t SEED_STAGE = 48;    // hits staged in LDS per wave (64 KiB table + staging: two workgroups per CU)
constexpr size_t SEED_STAGE_BYTES = (SEED_BLOCK / 64) * (SEED_STAGE * sizeof(Match) + 4);
__device__ __forceinline__ void seed_stage_hit(Match* stage, uint32_t* stage_n, uint32_t wave, const Match& m, Match* __restrict__ buf,
                                               uint32_t cap, uint32_t* __restrict__ total, uint32_t* __restrict__ hit_count) {
  const uint32_t at = atomicAdd(&stage_n[wave], 1u);
  if (at < SEED_STAGE) {
    stage[wave * SEED_STAGE + at] = m;
  } else {   // staging buffer full (a burst of hits): straight to the global buffer
    const uint32_t ga = atomicAdd(total, 1u);
    atomicAdd(&hit_count[(uint32_t)m.strand], 1u);
    if (ga < cap) buf[ga] = m;
  }
}
// Uniform point: flush once the buffer is half full (or, `last`, whatever it holds).  Staged hits sit in processing order: every run of
// one unit adds its length to its unit's hit count (one atomic per run, not per hit).
__device__ __forceinline__ void seed_stage_flush(Match* stage, uint32_t* stage_n, uint32_t wave, uint32_t lane, bool last,
                                                 Match* __restrict__ buf, uint32_t cap, uint32_t* __restrict__ total,
                                                 uint32_t* __restrict__ hit_count) {
  __builtin_amdgcn_wave_barrier();
  uint32_t n_st = stage_n[wave];
  if (n_st > SEED_STAGE) n_st = SEED_STAGE;
  if (n_st >= SEED_STAGE / 2 || (n_st && last)) {
    static_assert(SEED_STAGE <= 64, "one staged hit per lane at flush time");
    uint32_t base = 0;
    if (lane == 0) {
      base = atomicAdd(total, n_st);
      stage_n[wave] = 0;
    }
    base = __shfl(base, 0);
    int32_t mr = 0, mq = 0, ml = 0, mu = -1;   // (field by field: a Match temporary here is kept in scratch)
    if (lane < n_st) {
      const Match& st = stage[wave * SEED_STAGE + lane];
      mr = st.r; mq = st.q; ml = st.len; mu = st.strand;
    }
    const int32_t prev_unit = __shfl_up(mu, 1, 64);
    const bool start = lane < n_st && (lane == 0 || prev_unit != mu);
    const uint64_t starts = __ballot(start);
    if (start) {
      const uint64_t later = starts >> 1 >> lane;   // starts after this lane
      const uint32_t run = later ? (uint32_t)__ffsll((unsigned long long)later) : n_st - lane;
      atomicAdd(&hit_count[(uint32_t)mu], run);
    }
    if (lane < n_st && base + lane < cap) buf[base + lane] = Match{mr, mq, ml, mu};
    __builtin_amdgcn_wave_barrier();
  }
}

// Per-pair kernel (fragment mode, and PYANI_SEED_PER_PAIR=1): workgroup (c, r): LDS table of reference r's coarse group c,
// then every query of r streams its group-c entries through it.
// Each of the 16 WAVES takes every 16th pair and keeps SEED_UNROLL coalesced 512-byte loads in flight, so the stream is
// bandwidth- rather than latency-bound.  Matches are appended to one batch-wide buffer (the `strand` field carries the
// unit index until the scatter); unit_count[] is exact even when the buffer overflows, which is what the host uses to
// size the slices (and to re-run a prefix).
//
// PASSES (anim_seed_pair_kernel<true>, launched only when a planned coarse group holds more than half a table): the entries
// [goff[8 c], goff[8 (c + 1)]) are cut into passes (pg_seed_plan.h); per pass the table is cleared, filled with the pass's
// entries and probed by the whole query stream.  Only the table repeats: staging carries over, with one final flush.  The
// single-pass kernel is the instantiation without the loop and compiles to what it was before passes existed.
template <bool PASSES>
__global__ __launch_bounds__(SEED_BLOCK) void anim_seed_pair_kernel(const SeedRef* __restrict__ srefs, const SeedQry* __restrict__ sqry,
                                                                    const SeedSlice* __restrict__ slice, uint32_t n_pairs,
                                                                    uint32_t slot_mask, Match* __restrict__ buf, uint32_t cap,
                                                                    uint32_t* __restrict__ total, uint32_t* __restrict__ hit_count,
                                                                    int32_t step) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long tab[];
  Match* stage = reinterpret_cast<Match*>(tab + slot_mask + 1);                    // [waves][SEED_STAGE]
  uint32_t* stage_n = reinterpret_cast<uint32_t*>(stage + (SEED_BLOCK / 64) * SEED_STAGE);   // [waves]
  // Workgroups are numbered reference-fastest: the workgroups in flight at any moment are the SAME few groups of ALL the
  // references of the launch, and they stream the same query slices — which therefore come from L2 / the 256 MB Infinity
  // Cache for all but the first reader instead of from HBM once per reference (r01, group-fastest numbering: 6.9 x the
  // algorithmic bytes, profiles/archive/r02_anim_C4_pmc_summary.csv "before").
  const uint32_t g = blockIdx.y;
  const SeedRef SR = srefs[blockIdx.x];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  for (uint32_t i = tid; i <= slot_mask; i += SEED_BLOCK) tab[i] = SLOT_EMPTY;
  if (tid < SEED_BLOCK / 64) stage_n[tid] = 0;
  __syncthreads();
  uint32_t pass = 0, n_pass = 1, grp_begin = 0, grp_n = 0;   // (PASSES only)
  if constexpr (PASSES) {
    grp_begin = SR.goff[SEED_SUB * g];
    grp_n = SR.goff[SEED_SUB * (g + 1)] - grp_begin;
    n_pass = pg_seed_pass_count(grp_n, slot_mask + 1);   // uniform per workgroup
  }
  auto insert = [&](unsigned long long v) {
    uint32_t slot = (uint32_t)(v >> (SEED_KEY_SHIFT + 5)) & slot_mask;   // hash bits 5.. (slot_mask <= 2^14 - 1)
    while (atomicCAS(&tab[slot], SLOT_EMPTY, v) != SLOT_EMPTY) slot = (slot + 1) & slot_mask;   // <= half full per pass: ends
  };
  do {   // (single-pass instantiation: one trip, no loop)
    if constexpr (PASSES) {
      const PgSeedPass R = pg_seed_pass_range(grp_n, slot_mask + 1, pass);
      for (uint32_t e = grp_begin + R.begin + tid; e < grp_begin + R.end; e += SEED_BLOCK) insert(SR.list[e]);
    } else {
      for (uint32_t e = SR.goff[SEED_SUB * g] + tid; e < SR.goff[SEED_SUB * (g + 1)]; e += SEED_BLOCK) insert(SR.list[e]);
    }
    __syncthreads();
    // this wave's share of the reference's pairs: a contiguous range, its descriptors fetched 64 at a time
    const uint32_t n_mine_all = SR.pair_end - SR.pair_begin;
    const uint32_t per_wave = (n_mine_all + SEED_BLOCK / 64 - 1) / (SEED_BLOCK / 64);
    const uint32_t my_begin = SR.pair_begin + wave * per_wave;
    const uint32_t my_end = my_begin + per_wave < SR.pair_end ? my_begin + per_wave : SR.pair_end;
    const SeedSlice* __restrict__ row = slice + (size_t)g * n_pairs;
    for (uint32_t chunk = my_begin; chunk < my_end; chunk += 64) {
      SeedSlice mine{0, 0, 0};
      const uint64_t* mylist = nullptr;
      if (chunk + lane < my_end) { mine = row[chunk + lane]; mylist = sqry[chunk + lane].list; }
      const uint32_t in_chunk = my_end - chunk < 64 ? my_end - chunk : 64;
      // The chunk's work as a sequence of row blocks (<= SEED_UNROLL rows of 64 entries of one (pair, strand) slice),
      // software-pipelined: the loads of block k+1 are in flight while block k is looked up.
      struct Blk { uint32_t j, strand, e0, e_end; const uint64_t* list; bool valid; };
      auto slice_of = [&](uint32_t j, uint32_t strand, Blk& o) {
        const uint32_t begin = (uint32_t)__builtin_amdgcn_readlane((int)mine.begin, j);
        const uint32_t n0 = (uint32_t)__builtin_amdgcn_readlane((int)mine.n0, j), n1 = (uint32_t)__builtin_amdgcn_readlane((int)mine.n1, j);
        o.j = j; o.strand = strand;
        o.e0 = strand ? begin + n0 : begin;
        o.e_end = o.e0 + (strand ? n1 : n0);
        o.list = reinterpret_cast<const uint64_t*>(
            ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)((unsigned long long)mylist >> 32), j) << 32) |
            (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(unsigned long long)mylist, j));
      };
      auto first_from = [&](uint32_t j, uint32_t strand) {   // first non-empty slice at or after (j, strand)
        Blk o{0, 0, 0, 0, nullptr, false};
        for (; j < in_chunk; ++j, strand = 0)
          for (; strand < 2; ++strand) {
            slice_of(j, strand, o);
            if (o.e0 < o.e_end) { o.valid = true; return o; }
          }
        return o;
      };
      auto next_of = [&](const Blk& c) {
        if (c.e0 + 64 * SEED_UNROLL < c.e_end) { Blk o = c; o.e0 += 64 * SEED_UNROLL; return o; }
        return c.strand == 0 ? first_from(c.j, 1) : first_from(c.j + 1, 0);
      };
      auto load = [&](const Blk& c, unsigned long long (&qv)[SEED_UNROLL]) {
#pragma unroll
        for (int t = 0; t < SEED_UNROLL; ++t) {
          const uint32_t e = c.e0 + 64 * t + lane;
          qv[t] = e < c.e_end ? __builtin_nontemporal_load(&c.list[e]) : SLOT_EMPTY;
        }
      };
      auto process = [&](const Blk& c, const unsigned long long (&qv)[SEED_UNROLL]) {
        const uint32_t unit = 2 * (chunk + c.j) + c.strand;
#pragma unroll
        for (int t = 0; t < SEED_UNROLL; ++t) {
          if (qv[t] == SLOT_EMPTY) continue;
          const uint32_t key = (uint32_t)(qv[t] >> SEED_KEY_SHIFT);
          const uint32_t qctx = (uint32_t)(qv[t] >> 32) & 0x7FFu;   // bit 0: flag, bits 1..10: left bases
          const int32_t q = (int32_t)(uint32_t)qv[t];
          uint32_t slot_b = ((key >> 5) & slot_mask) << 3;   // byte offset of the slot (the probe steps in bytes: add + and per step)
          const uint32_t byte_mask = (slot_mask << 3) | 7u;
          const char* const tab_b = reinterpret_cast<const char*>(tab);
          // one exit condition and no break / continue inside: the compiler turns anything else into a state machine of
          // exec-mask bookkeeping, and the per-CU scalar unit is a bottleneck of this kernel
          // 32-bit tests only (64-bit integer compares are slower): an entry's low word is a position, never all ones, so the
          // low word alone says "empty"; the key sits in the top 21 bits of the high word
          const uint32_t qhi = (uint32_t)(qv[t] >> 32);
          unsigned long long v = *reinterpret_cast<const unsigned long long*>(tab_b + slot_b);
          while ((uint32_t)v != 0xFFFFFFFFu) {   // load factor <= 1/2: every probe sequence ends
            if ((((uint32_t)(v >> 32) ^ qhi) >> (SEED_KEY_SHIFT - 32)) == 0u) {
              int32_t left = -1;
              bool report = true;
              const uint32_t rctx = (uint32_t)(v >> 32) & 0x7FFu;
              if (rctx & qctx & 1u) {
                const uint32_t x = (rctx ^ qctx) >> 1;
                const uint32_t diff = (x | (x >> 1)) & 0x155u;
                left = diff ? (__ffs(diff) - 1) >> 1 : SEED_STEP;
                report = left < step;   // inside a longer match: an earlier sampled position (every step-th) reports it
              }
              if (report) seed_stage_hit(stage, stage_n, wave, Match{(int32_t)(uint32_t)v, q, left, (int32_t)unit}, buf, cap, total, hit_count);
            }
            slot_b = (slot_b + 8u) & byte_mask;
            v = *reinterpret_cast<const unsigned long long*>(tab_b + slot_b);
          }
        }
        seed_stage_flush(stage, stage_n, wave, lane, false, buf, cap, total, hit_count);
      };
      unsigned long long qa[SEED_UNROLL], qb[SEED_UNROLL];
      Blk A = first_from(0, 0);
      if (A.valid) load(A, qa);
      while (A.valid) {
        Blk B = next_of(A);
        if (B.valid) load(B, qb);
        process(A, qa);
        if (!B.valid) break;
        A = next_of(B);
        if (A.valid) load(A, qa);
        process(B, qb);
      }
    }
    if constexpr (PASSES) {
      if (++pass < n_pass) {   // the next pass's table: every wave is done with this one first
        __syncthreads();
        for (uint32_t i = tid; i <= slot_mask; i += SEED_BLOCK) tab[i] = SLOT_EMPTY;
        __syncthreads();
      }
    }
  } while (PASSES && pass < n_pass);
  seed_stage_flush(stage, stage_n, wave, lane, true, buf, cap, total, hit_count);   // what is still staged (uniform point)
}

// Unit of a block kernel hit: code = query-in-block << 6 | slot-in-block << 1 | strand; -1 when the pair (slot's reference, query)
// is not seeded in this direction.  The lookup is made at the key match, before staging: a block holds every query of its
// slots, so a reference that is also a query of the block (a row of a tiled grid), and the unseeded direction of a mirrored
// pair, match whole genomes' worth of keys that must be dropped at once (staging them and resolving at the flush made the
// kernel 1.7 x slower).  n_qry < 2^25 (checked on the host).
__device__ __forceinline__ int32_t seed_block_unit(const int32_t* __restrict__ ptab, uint32_t n_qry, uint32_t code) {
  const int32_t pair = ptab[(size_t)((code >> 1) & 31u) * n_qry + (code >> 6)];
  return pair >= 0 ? 2 * pair + (int32_t)(code & 1u) : -1;
}

// Block kernel (ANIm): the launch's seeded pairs are cut on the host into BLOCKS of reference SLOTS.  A slot is one reference
// genome with a set of its seeded pairs whose queries are distinct (a pair listed twice takes a second slot of the same
// reference); a block holds at most SEED_BLOCK_SLOTS slots whose largest groups sum to at most half the LDS table, and the
// sorted distinct queries of their pairs.  Workgroup (b, g): ONE LDS table of group g of every slot of block b, then every
// query of the block streams its group-g entries through it ONCE — each query is read once per block instead of once per
// pair.  A key match names its slot; pair_of[slot][query] names the pair, or is -1 when the pair (reference, query) is not
// seeded in this direction (no pair, or mirrored from its partner): such a hit is neither staged nor counted.
// Table entry: [63:46] hash bits 0..17 (the key within its group) | [45:35] the lists' context bits [42:32] | [34:30] slot in
// the block | [29:0] reference position.  Positions < 2^30 - 1 (checked on the host), so the low word of an entry is never all
// ones = SLOT_EMPTY's.
constexpr int SEED_BLOCK_SLOTS = 32;
constexpr int SEED_TAB_KEY_SHIFT = 46, SEED_TAB_CTX_SHIFT = 35, SEED_TAB_SLOT_SHIFT = 30;
constexpr uint32_t SEED_TAB_POS_MASK = (1u << SEED_TAB_SLOT_SHIFT) - 1u, SEED_KEY_MASK = (1u << (32 - SEED_GROUP_BITS)) - 1u;
static_assert(32 - SEED_GROUP_BITS + 11 + 5 + SEED_TAB_SLOT_SHIFT == 64 && (1 << 5) == SEED_BLOCK_SLOTS, "table entry bit budget");
struct SeedSlot { const uint64_t* list; const uint32_t* goff; };   // a slot's reference lists
struct SeedBlk {
  uint32_t slot_begin, slot_end;   // into the launch's SeedSlot array
  uint32_t qry_begin, qry_end;     // into the launch's query array (SeedQry, sorted by genome)
  uint32_t pair_tab;               // pair_of[pair_tab + slot_in_block * n_qry + query_in_block]: pair index or -1
};
// Slot of a 18-bit key in a table of slot_mask + 1 = 2^(18 - slot_shift) slots: the key's top bits (hash bits slot_shift ..
// 17, the best mixed of a multiplicative hash below the group bits).
//
// PASSES (anim_seed_kernel<true>, launched only when a planned block needs them): a slot whose group holds more than half a
// table is alone in its block (the planning rule above takes the first slot whatever its size and no second one beside it),
// so passes apply to blocks of ONE slot: its group's entries are cut into passes (pg_seed_plan.h), filled by the whole
// workgroup, and every pass is probed by the block's whole query stream.  Blocks of several slots take one pass, as in the
// single-pass kernel.  Only the table repeats; staging carries over, with one final flush.
template <bool PASSES>
__global__ __launch_bounds__(SEED_BLOCK) void anim_seed_kernel(const SeedBlk* __restrict__ blks, const SeedSlot* __restrict__ slots,
                                                               const SeedQry* __restrict__ bqry, const int32_t* __restrict__ pair_of,
                                                               uint32_t slot_mask, uint32_t slot_shift, Match* __restrict__ buf,
                                                               uint32_t cap, uint32_t* __restrict__ total, uint32_t* __restrict__ hit_count,
                                                               int32_t step) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long tab[];
  Match* stage = reinterpret_cast<Match*>(tab + slot_mask + 1);                    // [waves][SEED_STAGE]
  uint32_t* stage_n = reinterpret_cast<uint32_t*>(stage + (SEED_BLOCK / 64) * SEED_STAGE);   // [waves]
  // Workgroups are numbered block-fastest (as the per-pair kernel's reference-fastest): the workgroups in flight stream the
  // same few groups of the same queries, which come from L2 / the Infinity Cache for all but the first reader.
  const uint32_t g = blockIdx.y;
  const SeedBlk B = blks[blockIdx.x];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  for (uint32_t i = tid; i <= slot_mask; i += SEED_BLOCK) tab[i] = SLOT_EMPTY;
  if (tid < SEED_BLOCK / 64) stage_n[tid] = 0;
  __syncthreads();
  auto insert = [&](unsigned long long v, uint32_t k) {   // list entry v of slot k -> table entry
    const unsigned long long t = (((v >> SEED_KEY_SHIFT) & SEED_KEY_MASK) << SEED_TAB_KEY_SHIFT) | (((v >> 32) & 0x7FFull) << SEED_TAB_CTX_SHIFT) |
                                 ((unsigned long long)k << SEED_TAB_SLOT_SHIFT) | (uint32_t)v;
    uint32_t slot = (uint32_t)(t >> (SEED_TAB_KEY_SHIFT + slot_shift)) & slot_mask;
    while (atomicCAS(&tab[slot], SLOT_EMPTY, t) != SLOT_EMPTY) slot = (slot + 1) & slot_mask;   // <= half full per pass: ends
  };
  const bool lone = PASSES && B.slot_end - B.slot_begin == 1;   // a block of one slot: the only kind that may need passes
  uint32_t pass = 0, n_pass = 1, grp_begin = 0, grp_n = 0;      // (PASSES only; uniform per workgroup)
  const uint64_t* grp_list = nullptr;
  if constexpr (PASSES) {
    if (lone) {
      const SeedSlot S = slots[B.slot_begin];
      grp_list = S.list;
      grp_begin = S.goff[g];
      grp_n = S.goff[g + 1] - grp_begin;
      n_pass = pg_seed_pass_count(grp_n, slot_mask + 1);
    }
  }
  do {   // (single-pass instantiation: one trip, no loop)
    if (lone) {
      const PgSeedPass R = pg_seed_pass_range(grp_n, slot_mask + 1, pass);
      for (uint32_t e = grp_begin + R.begin + tid; e < grp_begin + R.end; e += SEED_BLOCK) insert(grp_list[e], 0u);
    } else {
      for (uint32_t k = wave; k < B.slot_end - B.slot_begin; k += SEED_BLOCK / 64) {   // one slot per wave at a time
        const SeedSlot S = slots[B.slot_begin + k];
        const uint32_t e_end = S.goff[g + 1];
        for (uint32_t e = S.goff[g] + lane; e < e_end; e += 64) insert(S.list[e], k);
      }
    }
    __syncthreads();
    // This wave's share of the block's queries: a contiguous range, in chunks of 32 queries = 64 slices (lane i: query i / 2,
    // strand i & 1), their group-g offsets read straight from the queries' offset tables (strand s: sub-list seed_sub(g, 1, s)).
    // A chunk's non-empty slices are packed back to back into full rows of 64 entries (a slice holds ~60 entries per strand of a
    // 5 Mb query: one row per slice would leave a third of the lanes idle and put one memory round trip behind every row).
    const uint32_t n_qry = B.qry_end - B.qry_begin;
    const int32_t* __restrict__ ptab = pair_of + B.pair_tab;
    const uint32_t per_wave = (n_qry + SEED_BLOCK / 64 - 1) / (SEED_BLOCK / 64);
    const uint32_t my_begin = wave * per_wave;
    const uint32_t my_end = my_begin + per_wave < n_qry ? my_begin + per_wave : n_qry;
    const uint32_t sub0 = seed_sub(g, 1, 0), sub1 = seed_sub(g, 1, 1);
    for (uint32_t chunk = my_begin; chunk < my_end; chunk += 32) {
      uint32_t n = 0;
      unsigned long long base = 0;   // address of the slice's entry 0
      if (chunk + (lane >> 1) < my_end) {
        const SeedQry Q = bqry[B.qry_begin + chunk + (lane >> 1)];
        const uint32_t sub = (lane & 1u) ? sub1 : sub0;
        const uint32_t b = Q.goff[sub];
        n = Q.goff[sub + 1] - b;
        base = (unsigned long long)(Q.list + b);
      }
      // compaction: lane r takes the r-th non-empty slice (src = its lane above: the slice id)
      const uint64_t ne = __ballot(n != 0);
      const uint32_t n_ne = (uint32_t)__popcll(ne);
      uint32_t src = 0;
      {
        uint64_t m = ne;   // select the (lane + 1)-th set bit: binary search on prefix popcounts
        uint32_t lo = 0;
#pragma unroll
        for (uint32_t w = 32; w > 0; w >>= 1) {
          const uint64_t low = w == 64 ? m : (m & ((1ull << w) - 1ull));
          const uint32_t c = (uint32_t)__popcll(low);
          if (lane >= lo + c) { lo += c; m >>= w; src += w; } else { m = low; }
        }
      }
      const uint32_t pulled = (uint32_t)__shfl(n, (int)src, 64);   // (all lanes: a bpermute reads 0 from an inactive lane)
      const uint32_t cn = lane < n_ne ? pulled : 0u;
      const unsigned long long cbase = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(base >> 32), (int)src, 64) << 32) |
                                       (uint32_t)__shfl((int)(uint32_t)base, (int)src, 64);
      uint32_t c = cn;   // exclusive prefix of the packed slice lengths: where slice `lane` starts in the chunk's stream
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(c, o, 64); if ((int)lane >= o) c += t; }
      const uint32_t T = (uint32_t)__shfl((int)c, 63, 64);
      c -= cn;
      const unsigned long long cstart = cbase - (unsigned long long)c * 8ull;   // entry e of the stream (in slice `lane`) at cstart + 8 e
      // row at E: lane l holds stream entry E + l, of the slice j = (slices starting at or before it) - 1
      auto load = [&](uint32_t E, unsigned long long (&qv)[SEED_UNROLL], uint32_t (&sid)[SEED_UNROLL]) {
#pragma unroll
        for (int t = 0; t < SEED_UNROLL; ++t) {
          const uint32_t R = E + 64u * (uint32_t)t;
          qv[t] = SLOT_EMPTY;
          sid[t] = 0;
          if (R < T) {
            const uint32_t before = (uint32_t)__popcll(__ballot(lane < n_ne && c < R));
            uint64_t in_row = __ballot(lane < n_ne && c >= R && c < R + 64u), S = 0;
            while (in_row) {   // (one or two slices start inside a row)
              const int i = __ffsll((unsigned long long)in_row) - 1;
              S |= 1ull << ((uint32_t)__builtin_amdgcn_readlane((int)c, i) - R);
              in_row &= in_row - 1ull;
            }
            const uint32_t at = before + __builtin_amdgcn_mbcnt_hi((uint32_t)(S >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)S, 0u)) +
                                (uint32_t)((S >> lane) & 1ull);
            const int j = (int)at - 1;
            const unsigned long long st = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(cstart >> 32), j, 64) << 32) |
                                          (uint32_t)__shfl((int)(uint32_t)cstart, j, 64);
            sid[t] = (uint32_t)__shfl((int)src, j, 64);
            if (R + lane < T) qv[t] = __builtin_nontemporal_load(reinterpret_cast<const uint64_t*>(st + 8ull * (R + lane)));
          }
        }
      };
      auto process = [&](const unsigned long long (&qv)[SEED_UNROLL], const uint32_t (&sid)[SEED_UNROLL]) {
#pragma unroll
        for (int t = 0; t < SEED_UNROLL; ++t) {
          if (qv[t] == SLOT_EMPTY) continue;
          const uint32_t qhi = (uint32_t)(qv[t] >> 32);
          const uint32_t qkey = (qhi >> (SEED_KEY_SHIFT - 32)) & SEED_KEY_MASK;
          const uint32_t qctx = qhi & 0x7FFu;   // bit 0: flag, bits 1..10: left bases
          const int32_t q = (int32_t)(uint32_t)qv[t];
          const uint32_t qcode = ((chunk + (sid[t] >> 1)) << 6) | (sid[t] & 1u);   // query in block, strand (the slot is or'ed in)
          uint32_t slot_b = ((qkey >> slot_shift) & slot_mask) << 3;   // byte offset of the slot
          const uint32_t byte_mask = (slot_mask << 3) | 7u;
          const char* const tab_b = reinterpret_cast<const char*>(tab);
          // (single exit, 32-bit tests only: see the per-pair kernel)
          unsigned long long v = *reinterpret_cast<const unsigned long long*>(tab_b + slot_b);
          while ((uint32_t)v != 0xFFFFFFFFu) {   // load factor <= 1/2: every probe sequence ends
            const uint32_t vhi = (uint32_t)(v >> 32);
            if ((vhi >> (SEED_TAB_KEY_SHIFT - 32)) == qkey) {
              int32_t left = -1;
              bool report = true;
              const uint32_t rctx = (vhi >> (SEED_TAB_CTX_SHIFT - 32)) & 0x7FFu;
              if (rctx & qctx & 1u) {
                const uint32_t x = (rctx ^ qctx) >> 1;
                const uint32_t diff = (x | (x >> 1)) & 0x155u;
                left = diff ? (__ffs(diff) - 1) >> 1 : SEED_STEP;
                report = left < step;   // inside a longer match: an earlier sampled position (every step-th) reports it
              }
              if (report) {
                const uint32_t code = qcode | ((vhi & 7u) << 3) | (((uint32_t)v >> (SEED_TAB_SLOT_SHIFT - 1)) & 6u);
                const int32_t unit = seed_block_unit(ptab, n_qry, code);
                if (unit >= 0)
                  seed_stage_hit(stage, stage_n, wave, Match{(int32_t)((uint32_t)v & SEED_TAB_POS_MASK), q, left, unit}, buf, cap, total, hit_count);
              }
            }
            slot_b = (slot_b + 8u) & byte_mask;
            v = *reinterpret_cast<const unsigned long long*>(tab_b + slot_b);
          }
        }
        seed_stage_flush(stage, stage_n, wave, lane, false, buf, cap, total, hit_count);
      };
      // software-pipelined: the loads of the next SEED_UNROLL rows are in flight while these are looked up
      unsigned long long qa[SEED_UNROLL], qb[SEED_UNROLL];
      uint32_t sa[SEED_UNROLL], sb[SEED_UNROLL];
      constexpr uint32_t STEP = 64u * SEED_UNROLL;
      if (T) load(0, qa, sa);
      for (uint32_t E = 0; E < T; E += 2 * STEP) {
        if (E + STEP < T) load(E + STEP, qb, sb);
        process(qa, sa);
        if (E + STEP >= T) break;
        if (E + 2 * STEP < T) load(E + 2 * STEP, qa, sa);
        process(qb, sb);
      }
    }
    if constexpr (PASSES) {
      if (++pass < n_pass) {   // the next pass's table: every wave is done with this one first
        __syncthreads();
        for (uint32_t i = tid; i <= slot_mask; i += SEED_BLOCK) tab[i] = SLOT_EMPTY;
        __syncthreads();
      }
    }
  } while (PASSES && pass < n_pass);
  seed_stage_flush(stage, stage_n, wave, lane, true, buf, cap, total, hit_count);   // what is still staged (uniform point)
}

// hoff[0..n] = exclusive prefix of cnt[0..n); cursor[] zeroed.  One workgroup (n <= 2 * pairs of a launch).
__global__ __launch_bounds__(1024) void anim_hoff_kernel(const uint32_t* __restrict__ cnt, uint32_t n, uint32_t* __restrict__ hoff,
                                                         uint32_t* __restrict__ cursor) {
  __shared__ uint32_t s_part[1024];
  const uint32_t tid = threadIdx.x;
  const uint32_t per = (n + 1023) / 1024, lo = tid * per, hi = lo + per < n ? lo + per : n;
  uint32_t sum = 0;
  for (uint32_t i = lo; i < hi; ++i) sum += cnt[i];
  s_part[tid] = sum;
  __syncthreads();
  if (tid == 0) { uint32_t run = 0; for (int i = 0; i < 1024; ++i) { const uint32_t t = s_part[i]; s_part[i] = run; run += t; } hoff[n] = run; }
  __syncthreads();
  uint32_t run = s_part[tid];
  for (uint32_t i = lo; i < hi; ++i) { hoff[i] = run; run += cnt[i]; cursor[i] = 0; }
}

// hits -> per-unit slices (hoff): same dealing as anim_scatter_kernel, records unchanged
__global__ __launch_bounds__(256) void anim_hit_scatter_kernel(const Match* __restrict__ buf, const uint32_t* __restrict__ n_hits, uint32_t cap,
                                                               const uint32_t* __restrict__ hoff, uint32_t* __restrict__ cursor,
                                                               Match* __restrict__ out) {
  const uint32_t n = *n_hits < cap ? *n_hits : cap;
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {
    const uint32_t i = base + threadIdx.x;
    Match m{0, 0, 0, 0};
    if (i < n) m = buf[i];
    const uint32_t u = (uint32_t)m.strand;
    bool todo = i < n;
    while (true) {
      const uint64_t rest = __ballot(todo);
      if (!rest) break;
      const int leader = __ffsll((unsigned long long)rest) - 1;
      const uint32_t lu = __shfl(u, leader);
      const uint64_t same = __ballot(todo && u == lu);
      uint32_t at = 0;
      if ((int)lane == leader) at = atomicAdd(&cursor[lu], (uint32_t)__popcll(same));
      at = __shfl(at, leader);
      if (todo && u == lu) {
        out[(size_t)hoff[u] + at + (uint32_t)__popcll(same & ((1ull << lane) - 1ull))] = m;
        todo = false;
      }
    }
  }
}

// One WORKGROUP per unit walks that unit's recorded hits {r, q, left (-1: undecided), unit}: decide the left extension
// where the list entries could not, extend to the right, and append matches of at least MIN_MATCH bases to the batch
// buffer (the `strand` field carries the unit until the scatter) while counting them — exact even if the buffer
// overflows.  A unit's hits touch only its own two genomes (≈ 4 MB packed): processed by one workgroup, i.e. on one XCD,
// they are served by that XCD's L2 instead of one HBM line fetch per access.
// mirror[pair] >= 0: the batch also holds the pair with the two genomes' roles swapped, and that pair was NOT seeded.  The
// maximal exact matches of (A, B) and (B, A) are the same set — forward: (r, q) <-> (q, r); reverse strand: A[r, r + len) on
// the reverse complement of B at strand position q  <->  B[len_B - q - len, ...) on the reverse complement of A at strand
// position len_A - r - len — so every match is appended a second time, transposed, for the partner's unit of the same strand.
__global__ __launch_bounds__(256) void anim_hit_kernel(const RefDesc* __restrict__ refs, const UnitDesc* __restrict__ units,
                                                       const Match* __restrict__ hits, const uint32_t* __restrict__ hoff,
                                                       const uint32_t* __restrict__ n_hits, uint32_t hit_cap,
                                                       Match* __restrict__ buf, uint32_t cap, uint32_t* __restrict__ total,
                                                       uint32_t* __restrict__ unit_count, int32_t min_match, int32_t step,
                                                       const int32_t* __restrict__ mirror) {
  const uint32_t unit = blockIdx.x;
  const uint32_t h0 = hoff[unit], h1 = hoff[unit + 1];
  if (h0 == h1 || *n_hits > hit_cap) return;   // (hits were dropped: the slices are incomplete, the host retries with fewer pairs)
  const uint32_t lane = threadIdx.x & 63u;
  const UnitDesc U0 = units[unit];
  const RefDesc R = refs[U0.ref];
  const SeqView RV{R.codes, R.mask, R.len};
  const StrandView QV{SeqView{U0.codes, U0.mask, U0.len}, U0.strand};
  const int32_t mp = mirror ? mirror[U0.pair] : -1;
  const uint32_t unit2 = mp >= 0 ? 2u * (uint32_t)mp + (uint32_t)U0.strand : 0u;
  for (uint32_t base = h0; base < h1; base += blockDim.x) {
    const uint32_t i = base + threadIdx.x;
    Match m{0, 0, 0, (int32_t)unit};
    bool have = false;
    if (i < h1) {
      const Match h = hits[i];
      have = seed_hit(R, RV, U0, QV, U0.strand, h.r, h.q, h.len, min_match, step, m);
    }
    const uint64_t got = __ballot(have);
    if (got) {
      uint32_t at = 0;
      const uint32_t c = (uint32_t)__popcll(got);
      if (lane == 0) {
        at = atomicAdd(total, mp >= 0 ? 2 * c : c);
        atomicAdd(&unit_count[unit], c);
        if (mp >= 0) atomicAdd(&unit_count[unit2], c);
      }
      at = __shfl(at, 0);
      if (have) {
        at += (uint32_t)__popcll(got & ((1ull << lane) - 1ull));
        m.strand = (int32_t)unit;
        if (at < cap) buf[at] = m;
        if (mp >= 0 && at + c < cap)
          buf[at + c] = U0.strand == 0 ? Match{m.q, m.r, m.len, (int32_t)unit2}
                                       : Match{U0.len - m.q - m.len, R.len - m.r - m.len, m.len, (int32_t)unit2};
      }
    }
  }
}

// Deal the appended matches into their units' slices (moff[u] .. moff[u+1]); units >= n_units wait for the next batch.
// The seed kernel flushes bursts of one unit, so a wave usually sees one to three distinct units: one atomic per
// distinct unit and wave instead of one per match.
__global__ __launch_bounds__(256) void anim_scatter_kernel(const Match* __restrict__ buf, uint32_t n, const uint32_t* __restrict__ moff,
                                                           uint32_t n_units, uint32_t* __restrict__ cursor, Match* __restrict__ mem) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  Match m{0, 0, 0, -1};
  if (i < n) m = buf[i];
  const uint32_t u = (uint32_t)m.strand;
  bool todo = i < n && u < n_units;
  while (true) {
    const uint64_t rest = __ballot(todo);
    if (!rest) break;
    const int leader = __ffsll((unsigned long long)rest) - 1;
    const uint32_t lu = __shfl(u, leader);
    const uint64_t same = __ballot(todo && u == lu);
    uint32_t base = 0;
    if ((int)lane == leader) base = atomicAdd(&cursor[lu], (uint32_t)__popcll(same));
    base = __shfl(base, leader);
    if (todo && u == lu) {
      m.strand = (int32_t)(u & 1u);
      mem[(size_t)moff[u] + base + (uint32_t)__popcll(same & ((1ull << lane) - 1ull))] = m;
      todo = false;
    }
  }
}
