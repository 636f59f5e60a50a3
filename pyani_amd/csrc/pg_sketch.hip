// pg_sketch.hip — the SKETCH mode on the GPU (definition: pg_sketch_core.h; reference interface it stands in for:
// pyani/fastani.py:193-270, construct_fastani_cmdline / parse_fastani_file).  An opt-in ESTIMATE with its own result struct — nothing
// here touches the exact ANIm / ANIb results.  Integer / byte work over the 2-bit packed genomes already resident in HBM; no MFMA.
//
//   S1 sketch_scan_kernel   once per genome (cached with its k / frag_len / scale): one coalesced pass over the packed stream; every lane
//                           rolls the canonical k-mers of 32 consecutive start positions out of three code words and two mask
//                           words (32 + k - 1 <= 47 bases for every k of 8 ... 16; k is a compile-time parameter, chosen by a host
//                           switch), keeps the sampled ones (mix32(kmer) & (scale - 1) == 0: 1 in 16), and
//                             - inserts them into the genome's k-mer SET (open addressing in HBM, <= 1/2 load: the reference role),
//                             - appends (k-mer, fragment) for those that lie inside a fragment (the query role), counting per fragment.
//                           Two launches: count (sizes the arrays exactly), then fill.
//   S2 sketch_pairs_kernel  one workgroup per (query genome, up to 4 reference genomes): the query's occurrence list streams through
//                           once (coalesced), every k-mer probes the references' sets (1.2 MB each: L2-resident while the launch
//                           works through one reference's queries), hits are counted per fragment in LDS; then per reference the
//                           fragments' identities (pgs::frag_identity) are summed in fragment order — the definition's order, so the
//                           double comes out bit-identical to the host statement.
// Cost per ordered pair of 5 Mb genomes at scale 16: 3 x 10^5 probes + 2.4 MB / 4 of list traffic: the 10^6 pairs of C4 take seconds.
//
// The MAPPED mode (pg_sketch_pairs_mapped; definition: pg_sketch_core.h, "MAPPED variant"), opt-in beside the above:
//   M1 index_scan_kernel    once per REFERENCE genome (cached with its k / scale; positions, not bins: another frag_len reuses it): the
//                           scan of S1 again, every sampled k-mer inserted into the index's own open-addressing table and appended as
//                           the key (slot << 32 | g), g = its start in the records back to back without separator (stream position
//                           minus record index).  The keys are radix-sorted (hipcub), which lays every slot's coordinates side by
//                           side in ascending order; map_unpack_kernel splits them into the positions array and finds every slot's
//                           first entry by binary search (the offsets array over the slots).
//   M2 map_pack_kernel      once per QUERY sketch: (fragment << 32 | k-mer) of the occurrence list, sorted and unpacked the same way
//                           into the GROUPED form (a fragment's occurrences side by side, offsets = prefix sums of frag_n).
//   M3 sketch_map_kernel    persistent workgroups of 4 waves; a job is one (query, reference) pair.  Every wave takes fragments in
//                           turn: its lanes probe the index with the fragment's occurrences and walk the hit slots' coordinates,
//                           counting c_b and h_w in the wave's own dense LDS counters (16 bit where frag_len <= 65 535 bounds n, two to
//                           a word, LDS atomics); bins touched for the first time go on a list, so that the maximum is found and
//                           the counters are cleared over the touched bins alone (the list overflowing: over all of them).  One 32-byte
//                           record per fragment goes into the workgroup's scratch row; after the last fragment the workgroup
//                           computes the identities, applies the one-per-bin rule in the same LDS (max over the identity's bits, then
//                           max over ~index among equals) and wave 0 makes the ordered sum.  Scratch = resident workgroups x the
//                           longest query, not pairs x fragments.
#include <algorithm>
#include <hipcub/hipcub.hpp>
#include <vector>

#include "pg_internal.h"
#include <mutex>
#include "pg_sketch_core.h"

namespace {

struct SketchGenome {
  bool built = false;
  int32_t kmer = 0, frag_len = 0, scale = 0;
  uint32_t n_frags = 0, n_occ = 0, cap_mask = 0;
  PgDevBuf<uint32_t> occ_kmer, occ_frag, frag_n, tab;
  PgDevBuf<int32_t> rec_tab;       // [2 (n_rec + 1)]: rec_start | frag_base (device)
  // the grouped form (mapped mode, built for a genome that is a query of a mapped call; goes with the sketch)
  bool grouped = false;
  PgDevBuf<uint32_t> grp_kmer, frag_off;      // [n_occ] a fragment's k-mers side by side | [n_frags + 1]
};
struct MapIndex {      // a genome in the reference role of the mapped mode: every distinct sampled k-mer's coordinates, ascending
  bool built = false;
  int32_t kmer = 0, scale = 0;
  uint32_t cap_mask = 0, n_pos = 0;
  PgDevBuf<uint32_t> tab, off, pos;      // [cap] k-mer of the slot | [cap + 1] first position of the slot | [n_pos]
};
struct SketchStore {
  std::vector<SketchGenome> g;
  PgDevBuf<uint32_t> counters;
  std::vector<MapIndex> idx;
  PgDevBuf<unsigned long long> keys_a, keys_b;      // sort scratch of the index / grouping builds (kept, grown on demand)
  PgDevBuf<uint8_t> sort_tmp;
  double map_ms[2] = {0.0, 0.0};                    // pg_sketch_map_last_ms
};

// record of stream position p (rec_start[r] <= p < rec_start[r + 1])
__device__ __forceinline__ int rec_of(const int32_t* __restrict__ rec_start, int n_rec, int32_t p) {
  int lo = 0, hi = n_rec - 1;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (rec_start[mid] <= p) lo = mid; else hi = mid - 1; }
  return lo;
}

// counters: [0] sampled k-mers (all), [1] occurrences inside fragments (fill pass: the append cursor)
template <bool FILL, int K>
__global__ __launch_bounds__(256) void sketch_scan_kernel(const uint32_t* __restrict__ codes, const uint32_t* __restrict__ mask, int64_t stream_len,
                                                           const int32_t* __restrict__ rec_tab, int n_rec, int32_t frag_len, uint32_t scale,
                                                           uint32_t log2_scale, uint32_t* __restrict__ counters, uint32_t* __restrict__ occ_kmer,
                                                           uint32_t* __restrict__ occ_frag, uint32_t* __restrict__ frag_n, uint32_t* __restrict__ tab,
                                                           uint32_t cap_mask) {
  const int32_t* rec_start = rec_tab;
  const int32_t* frag_base = rec_tab + (n_rec + 1);
  const int64_t n_chunks = (stream_len + 31) / 32;      // chunk c = start positions 32 c .. 32 c + 31
  uint32_t n_all = 0, n_in = 0;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_chunks; c += (int64_t)gridDim.x * blockDim.x) {
    // bases 32 c .. 32 c + 47 = code words 2 c, 2 c + 1, 2 c + 2; mask words c, c + 1 (the arena is padded: reads past the stream see dirty bases)
    const uint64_t c01 = (uint64_t)codes[2 * c] | ((uint64_t)codes[2 * c + 1] << 32);
    const uint32_t c2 = codes[2 * c + 2];
    const uint64_t m = (uint64_t)mask[c] | ((uint64_t)mask[c + 1] << 32);
    uint32_t f = 0, r = 0;
    int rec = -1;
    int32_t rec_lo = 0, rec_hi = -1, fb = 0, n_full = 0;
    constexpr uint64_t WINDOW = (1ull << K) - 1ull;      // the K mask bits of a window
    for (int t = 0; t < 32 + K - 1; ++t) {      // base 32 c + t enters the window; the k-mer that ENDS on it starts at 32 c + t - (K - 1)
      const uint32_t code = t < 32 ? (uint32_t)(c01 >> (2 * t)) & 3u : (c2 >> (2 * (t - 32))) & 3u;
      f = pgs::roll_fwd(f, code, K); r = pgs::roll_rc(r, code, K);
      const int s = t - (K - 1);
      if (s < 0) continue;
      const int64_t p = 32 * c + s;
      if (p + K > stream_len || ((m >> s) & WINDOW) != WINDOW) continue;      // an ambiguity symbol, a record end, the stream's end
      const uint32_t canon = f < r ? f : r;
      if (!pgs::sampled(canon, scale)) continue;
      ++n_all;
      if (FILL) {      // the genome's k-mer set
        uint32_t slot = pgs::slot_of(canon, log2_scale, cap_mask);
        for (;;) {
          const uint32_t old = atomicCAS(&tab[slot], pgs::EMPTY, canon);
          if (old == pgs::EMPTY || old == canon) break;
          slot = (slot + 1u) & cap_mask;
        }
      }
      if (p < rec_lo || p > rec_hi) {      // (a chunk of 32 positions rarely leaves its record)
        rec = rec_of(rec_start, n_rec, (int32_t)p);
        rec_lo = rec_start[rec]; rec_hi = rec_start[rec + 1] - 2;      // last base of the record
        fb = frag_base[rec]; n_full = (rec_hi - rec_lo + 1) / frag_len;
      }
      const int32_t x = (int32_t)p - rec_lo, j = x / frag_len;
      if (j >= n_full || x - j * frag_len + K > frag_len) continue;      // the record's tail, or a k-mer across two fragments
      ++n_in;
      if (FILL) {
        const uint32_t at = atomicAdd(&counters[1], 1u);
        occ_kmer[at] = canon; occ_frag[at] = (uint32_t)(fb + j);
        atomicAdd(&frag_n[fb + j], 1u);
      }
    }
  }
  if (!FILL) {      // one atomic per wave and counter
    for (int o = 32; o > 0; o >>= 1) { n_all += __shfl_xor(n_all, o, 64); n_in += __shfl_xor(n_in, o, 64); }
    if ((threadIdx.x & 63) == 0) { if (n_all) atomicAdd(&counters[0], n_all); if (n_in) atomicAdd(&counters[1], n_in); }
  }
}

struct SketchJob {      // one workgroup: a query against up to SK_REFS references
  const uint32_t *occ_kmer, *occ_frag, *frag_n;
  uint32_t n_occ, n_frags, n_refs, log2_scale;
  int32_t kmer;      // one k per call: uniform over the workgroup
  const uint32_t* tab[4];
  uint32_t cap_mask[4];
  uint32_t out[4];      // pair indices of the call
  double min_fraction;
};
constexpr int SK_REFS = 4;

__global__ __launch_bounds__(256) void sketch_pairs_kernel(const SketchJob* __restrict__ jobs, pg_sketch_result* __restrict__ out) {
  extern __shared__ uint32_t hits[];      // [n_refs][n_frags]
  const SketchJob J = jobs[blockIdx.x];
  const uint32_t nf = J.n_frags, nr = J.n_refs;
  for (uint32_t i = threadIdx.x; i < nf * nr; i += blockDim.x) hits[i] = 0u;
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < J.n_occ; i += blockDim.x) {
    const uint32_t km = __builtin_nontemporal_load(J.occ_kmer + i), fr = __builtin_nontemporal_load(J.occ_frag + i);
    const uint32_t h = pgs::mix32(km) >> J.log2_scale;
#pragma unroll
    for (uint32_t g = 0; g < SK_REFS; ++g) {
      if (g >= nr) break;
      const uint32_t* tab = J.tab[g];
      const uint32_t cm = J.cap_mask[g];
      uint32_t slot = h & cm, v;
      while ((v = tab[slot]) != pgs::EMPTY) {
        if (v == km) { atomicAdd(&hits[g * nf + fr], 1u); break; }
        slot = (slot + 1u) & cm;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < nr) {      // the definition's order: fragments ascending, one running sum (bit-identical to the host statement)
    const uint32_t g = threadIdx.x;
    double sum = 0.0;
    int32_t matches = 0;
    for (uint32_t f = 0; f < nf; ++f) {
      const uint32_t n = J.frag_n[f], h = hits[g * nf + f];
      if (n == 0u || h < 2u) continue;
      const double ident = J.kmer == 16 ? pgs::frag_identity(h, n, 16) : pgs::frag_identity(h, n, J.kmer);      // (16: the four roots alone)
      if (ident >= pgs::MIN_IDENTITY) { sum = sum + ident; ++matches; }
    }
    pg_sketch_result o;
    o.matches = matches; o.fragments = (int32_t)nf;
    const bool enough = matches > 0 && (double)matches >= J.min_fraction * (double)nf;
    o.ani = enough ? sum / (double)matches : 0.0;
    o.status = enough ? 0 : PG_SKETCH_NO_RESULT; o.reserved = 0;
    out[jobs[blockIdx.x].out[g]] = o;      // (indexed by the lane: read from memory, so that J stays in registers)
  }
}

SketchStore* store_of(pg_ctx* ctx) {
  if (!ctx->sketch_store) ctx->sketch_store = new SketchStore();
  return static_cast<SketchStore*>(ctx->sketch_store);
}

// the scan kernel of a k-mer size: K is a compile-time parameter of the kernel (window, mask constant, fragment rule)
template <bool FILL>
auto scan_kernel_of(int32_t kmer) -> decltype(&sketch_scan_kernel<FILL, 16>) {
  switch (kmer) {
    case 8: return sketch_scan_kernel<FILL, 8>;
    case 9: return sketch_scan_kernel<FILL, 9>;
    case 10: return sketch_scan_kernel<FILL, 10>;
    case 11: return sketch_scan_kernel<FILL, 11>;
    case 12: return sketch_scan_kernel<FILL, 12>;
    case 13: return sketch_scan_kernel<FILL, 13>;
    case 14: return sketch_scan_kernel<FILL, 14>;
    case 15: return sketch_scan_kernel<FILL, 15>;
    case 16: return sketch_scan_kernel<FILL, 16>;
  }
  return nullptr;      // (pg_sketch_pairs_k refuses every other k before it gets here)
}

int build_sketch(pg_ctx* ctx, SketchStore* ST, int32_t gid, int32_t kmer, int32_t frag_len, int32_t scale, uint32_t log2_scale) {
  SketchGenome& S = ST->g[gid];
  if (S.built && S.kmer == kmer && S.frag_len == frag_len && S.scale == scale) return PG_OK;
  const auto scan_count = scan_kernel_of<false>(kmer);
  const auto scan_fill = scan_kernel_of<true>(kmer);
  if (!scan_count || !scan_fill) return pg_fail(ctx, PG_E_ARG, "sketch: no scan kernel for this k-mer size");
  S = SketchGenome{};
  const PgGenome& G = ctx->genomes[gid];
  std::vector<int32_t> rec_tab(2 * (G.n_rec + 1));
  uint32_t nf = 0;
  for (uint32_t r = 0; r <= G.n_rec; ++r) {
    rec_tab[r] = G.rec_start[r];
    rec_tab[G.n_rec + 1 + r] = (int32_t)nf;
    if (r < G.n_rec) nf += (uint32_t)((G.rec_start[r + 1] - 1 - G.rec_start[r]) / frag_len);
  }
  int rc;
  if ((rc = sk_malloc(ctx, S.rec_tab, rec_tab.size()))) return rc;
  PG_HIP(ctx, hipMemcpyAsync(S.rec_tab, rec_tab.data(), rec_tab.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  if (!ST->counters && (rc = sk_malloc(ctx, ST->counters, 2))) return rc;
  PG_HIP(ctx, hipMemsetAsync(ST->counters, 0, 8, ctx->stream));
  const uint32_t* codes = ctx->d_codes + G.arena_start / 16;
  const uint32_t* mask = ctx->d_mask + G.arena_start / 32;
  const dim3 grid((uint32_t)std::min<uint64_t>((G.stream_len / 32 + 255) / 256 + 1, (uint64_t)ctx->num_cu * 8));
  hipLaunchKernelGGL(scan_count, grid, dim3(256), 0, ctx->stream, codes, mask, (int64_t)G.stream_len, S.rec_tab, (int)G.n_rec, frag_len,
                     (uint32_t)scale, log2_scale, ST->counters, nullptr, nullptr, nullptr, nullptr, 0u);
  PG_HIP(ctx, hipGetLastError());
  uint32_t cnt[2];
  PG_HIP(ctx, hipMemcpyAsync(cnt, ST->counters, 8, hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  uint32_t cap = 1024;
  while (cap < 2 * cnt[0]) cap <<= 1;
  S.cap_mask = cap - 1; S.n_occ = cnt[1]; S.n_frags = nf; S.kmer = kmer; S.frag_len = frag_len; S.scale = scale;
  if ((rc = sk_malloc(ctx, S.tab, (size_t)cap))) return rc;
  if ((rc = sk_malloc(ctx, S.occ_kmer, (size_t)cnt[1] + 1))) return rc;
  if ((rc = sk_malloc(ctx, S.occ_frag, (size_t)cnt[1] + 1))) return rc;
  if ((rc = sk_malloc(ctx, S.frag_n, (size_t)nf + 1))) return rc;
  PG_HIP(ctx, hipMemsetAsync(S.tab, 0xFF, (size_t)cap * 4, ctx->stream));
  PG_HIP(ctx, hipMemsetAsync(S.frag_n, 0, (size_t)(nf + 1) * 4, ctx->stream));
  PG_HIP(ctx, hipMemsetAsync(ST->counters, 0, 8, ctx->stream));
  hipLaunchKernelGGL(scan_fill, grid, dim3(256), 0, ctx->stream, codes, mask, (int64_t)G.stream_len, S.rec_tab, (int)G.n_rec, frag_len,
                     (uint32_t)scale, log2_scale, ST->counters, S.occ_kmer, S.occ_frag, S.frag_n, S.tab, S.cap_mask);
  PG_HIP(ctx, hipGetLastError());
  S.built = true;
  return PG_OK;
}

// ---- the mapped mode ---------------------------------------------------------------------------------------------------------------------
// M1: the scan of sketch_scan_kernel for the reference role alone.  counters[0]: sampled k-mers (count pass) / the append cursor (fill)
template <bool FILL, int K>
__global__ __launch_bounds__(256) void index_scan_kernel(const uint32_t* __restrict__ codes, const uint32_t* __restrict__ mask, int64_t stream_len,
                                                          const int32_t* __restrict__ rec_start, int n_rec, uint32_t scale, uint32_t log2_scale,
                                                          uint32_t* __restrict__ counters, uint32_t* __restrict__ tab, uint32_t cap_mask,
                                                          unsigned long long* __restrict__ keys, uint32_t keys_cap) {
  const int64_t n_chunks = (stream_len + 31) / 32;
  uint32_t n_all = 0;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_chunks; c += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t c01 = (uint64_t)codes[2 * c] | ((uint64_t)codes[2 * c + 1] << 32);
    const uint32_t c2 = codes[2 * c + 2];
    const uint64_t m = (uint64_t)mask[c] | ((uint64_t)mask[c + 1] << 32);
    uint32_t f = 0, r = 0;
    int rec = 0;
    int32_t rec_lo = 0, rec_hi = -1;
    constexpr uint64_t WINDOW = (1ull << K) - 1ull;
    for (int t = 0; t < 32 + K - 1; ++t) {
      const uint32_t code = t < 32 ? (uint32_t)(c01 >> (2 * t)) & 3u : (c2 >> (2 * (t - 32))) & 3u;
      f = pgs::roll_fwd(f, code, K); r = pgs::roll_rc(r, code, K);
      const int s = t - (K - 1);
      if (s < 0) continue;
      const int64_t p = 32 * c + s;
      if (p + K > stream_len || ((m >> s) & WINDOW) != WINDOW) continue;
      const uint32_t canon = f < r ? f : r;
      if (!pgs::sampled(canon, scale)) continue;
      ++n_all;
      if (FILL) {
        uint32_t slot = pgs::slot_of(canon, log2_scale, cap_mask);
        for (;;) {
          const uint32_t old = atomicCAS(&tab[slot], pgs::EMPTY, canon);
          if (old == pgs::EMPTY || old == canon) break;
          slot = (slot + 1u) & cap_mask;
        }
        if (p < rec_lo || p > rec_hi) {
          rec = rec_of(rec_start, n_rec, (int32_t)p);
          rec_lo = rec_start[rec]; rec_hi = rec_start[rec + 1] - 2;
        }
        const uint32_t at = atomicAdd(&counters[0], 1u);
        if (at < keys_cap) keys[at] = ((unsigned long long)slot << 32) | (uint32_t)((int32_t)p - rec);      // no separator base in g
      }
    }
  }
  if (!FILL) {
    for (int o = 32; o > 0; o >>= 1) n_all += __shfl_xor(n_all, o, 64);
    if ((threadIdx.x & 63) == 0 && n_all) atomicAdd(&counters[0], n_all);
  }
}

// M2: the occurrence list as sort keys: fragment in the high word
__global__ __launch_bounds__(256) void map_pack_kernel(const uint32_t* __restrict__ hi, const uint32_t* __restrict__ lo, uint32_t n,
                                                        unsigned long long* __restrict__ keys) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) keys[i] = ((unsigned long long)hi[i] << 32) | lo[i];
}

// sorted keys (group << 32 | value) -> the values, and for every group 0 ... n_off - 1 its first key (groups past the last key: n)
__global__ __launch_bounds__(256) void map_unpack_kernel(const unsigned long long* __restrict__ keys, uint32_t n, uint32_t* __restrict__ value,
                                                          uint32_t* __restrict__ off, uint32_t n_off) {
  const uint32_t top = n > n_off ? n : n_off;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < top; i += gridDim.x * blockDim.x) {
    if (i < n) value[i] = (uint32_t)keys[i];
    if (i < n_off) {
      uint32_t lo = 0, hi = n;      // the first key whose group is >= i
      while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if ((uint32_t)(keys[mid] >> 32) < i) lo = mid + 1; else hi = mid; }
      off[i] = lo;
    }
  }
}

constexpr int MAP_WAVES = 4;                  // waves of a workgroup, each with its own counters
constexpr uint32_t MAP_TOUCH = 512;           // bins a wave lists per fragment before it falls back to the whole counter array
constexpr uint32_t MAP_MAX_BINS = 8192;       // per wave, 16-bit counters: 4 waves x (c + h) x 8192 x 2 B = 128 KiB of the 160
constexpr uint32_t MAP_MAX_BINS_WIDE = 4096;  // ... 32-bit counters (frag_len > 65 535: n may pass 65 535)

struct MapJob {      // one (query, reference) pair.  Read through its pointer, field by field (uniform loads): never copied into a lane-indexed struct
  const uint32_t *grp_kmer, *frag_off, *tab, *off, *pos;
  uint32_t n_frags, cap_mask, nb, out;
};

// a dense array of counters in LDS words: 32 bit each (WIDE), or 16 bit two to a word.  add returns the counter's value before
template <bool WIDE>
__device__ __forceinline__ uint32_t cnt_add(uint32_t* w, uint32_t i) {
  if (WIDE) return atomicAdd(&w[i], 1u);
  const uint32_t sh = (i & 1u) * 16u;
  return (atomicAdd(&w[i >> 1], 1u << sh) >> sh) & 0xFFFFu;
}
template <bool WIDE>
__device__ __forceinline__ uint32_t cnt_get(const uint32_t* w, uint32_t i) {
  if (WIDE) return w[i];
  return (w[i >> 1] >> ((i & 1u) * 16u)) & 0xFFFFu;
}
template <bool WIDE>
__device__ __forceinline__ void cnt_clear(uint32_t* w, uint32_t i) {
  if (WIDE) w[i] = 0u; else atomicAnd(&w[i >> 1], ~(0xFFFFu << ((i & 1u) * 16u)));      // (the neighbour in the word may be cleared by another lane)
}
__device__ __forceinline__ void map_wave_sync() {      // LDS traffic of one wave: program order, seen by all its lanes
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// M3.  Dynamic LDS: [MAP_WAVES][c | h] counters (nb_stride each; reused for the one-per-bin rule: best identity bits [nb_stride] u64,
// best ~index [nb_stride] u32), [MAP_WAVES][MAP_TOUCH] touched bins, [MAP_WAVES] their counts.  nb_stride: a multiple of 8 >= every job's nb.
template <bool WIDE>
__global__ __launch_bounds__(64 * MAP_WAVES) void sketch_map_kernel(const MapJob* __restrict__ jobs, uint32_t n_jobs, pg_sketch_fragment* __restrict__ rows,
                                                                     uint64_t row_stride, pg_sketch_result* __restrict__ out, int32_t kmer, uint32_t frag_len,
                                                                     uint32_t log2_scale, double min_fraction, uint32_t nb_stride) {
  extern __shared__ __attribute__((aligned(16))) uint32_t map_lds[];
  const uint32_t arr_words = WIDE ? nb_stride : nb_stride / 2;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t* cw = map_lds + (size_t)wave * 2 * arr_words;
  uint32_t* hw = cw + arr_words;
  uint32_t* touched = map_lds + (size_t)MAP_WAVES * 2 * arr_words + wave * MAP_TOUCH;
  uint32_t* n_touched = map_lds + (size_t)MAP_WAVES * 2 * arr_words + MAP_WAVES * MAP_TOUCH + wave;
  unsigned long long* best_bits = reinterpret_cast<unsigned long long*>(map_lds);
  uint32_t* best_nidx = map_lds + 2 * (size_t)nb_stride;
  for (uint32_t i = threadIdx.x; i < MAP_WAVES * 2 * arr_words; i += blockDim.x) map_lds[i] = 0u;
  if (lane == 0) *n_touched = 0u;
  __syncthreads();
  pg_sketch_fragment* row = rows + (size_t)blockIdx.x * row_stride;
  for (uint32_t job = blockIdx.x; job < n_jobs; job += gridDim.x) {
    const MapJob* J = jobs + job;
    const uint32_t nf = J->n_frags, nb = J->nb, cm = J->cap_mask;
    const uint32_t *grp = J->grp_kmer, *foff = J->frag_off, *tab = J->tab, *off = J->off, *pos = J->pos;
    for (uint32_t f = wave; f < nf; f += MAP_WAVES) {
      const uint32_t a = foff[f], e = foff[f + 1];
      for (uint32_t i = a + lane; i < e; i += 64u) {
        const uint32_t km = grp[i];
        uint32_t slot = (pgs::mix32(km) >> log2_scale) & cm, v;
        while ((v = tab[slot]) != pgs::EMPTY) {
          if (v == km) {      // the k-mer's coordinates, ascending: a new bin is one that differs from the previous
            int32_t prev = -2;
            const uint32_t j1 = off[slot + 1];
            for (uint32_t j = off[slot]; j < j1; ++j) {
              const int32_t b = (int32_t)(pos[j] / frag_len);
              if (b == prev || (uint32_t)b >= nb) continue;
              if (cnt_add<WIDE>(cw, (uint32_t)b) == 0u) {
                const uint32_t t = atomicAdd(n_touched, 1u);
                if (t < MAP_TOUCH) touched[t] = (uint32_t)b;
              }
              if (b >= 1 && b - 1 > prev) cnt_add<WIDE>(hw, (uint32_t)b - 1u);      // window b - 1 = bins b - 1, b: not yet counted through prev
              cnt_add<WIDE>(hw, (uint32_t)b);
              prev = b;
            }
            break;
          }
          slot = (slot + 1u) & cm;
        }
      }
      map_wave_sync();
      const uint32_t nt = *n_touched;
      const bool listed = nt <= MAP_TOUCH;
      unsigned long long best = 0ull;
      if (listed) {      // a window with a hit is window b or b - 1 of a touched bin b
        for (uint32_t t = lane; t < nt; t += 64u) {
          const uint32_t b = touched[t];
          unsigned long long key = pgs::map_window_key(cnt_get<WIDE>(hw, b), b);
          if (key > best) best = key;
          if (b >= 1u) { key = pgs::map_window_key(cnt_get<WIDE>(hw, b - 1u), b - 1u); if (key > best) best = key; }
        }
      } else {
        for (uint32_t w = lane; w < nb; w += 64u) {
          const unsigned long long key = pgs::map_window_key(cnt_get<WIDE>(hw, w), w);
          if (key > best) best = key;
        }
      }
      for (int o = 32; o > 0; o >>= 1) {
        const uint32_t hi = __shfl_xor((uint32_t)(best >> 32), o, 64), lo = __shfl_xor((uint32_t)best, o, 64);
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
        if (other > best) best = other;
      }
      const uint32_t h = pgs::map_key_hits(best);
      if (lane == 0) {
        pg_sketch_fragment R;
        R.window = -1; R.bin = -1;
        if (h) {
          const uint32_t w = pgs::map_key_window(best);
          R.window = (int32_t)w;
          R.bin = pgs::map_pick_bin((int32_t)w, cnt_get<WIDE>(cw, w), w + 1u < nb ? cnt_get<WIDE>(cw, w + 1u) : 0u);
        }
        R.hits = h; R.n = e - a; R.identity = 0.0; R.kept = 0; R.reserved = 0;
        row[f] = R;
      }
      map_wave_sync();
      if (listed) {
        for (uint32_t t = lane; t < nt; t += 64u) {
          const uint32_t b = touched[t];
          cnt_clear<WIDE>(cw, b); cnt_clear<WIDE>(hw, b);
          if (b >= 1u) cnt_clear<WIDE>(hw, b - 1u);
        }
      } else {
        for (uint32_t w = lane; w < nb; w += 64u) { cnt_clear<WIDE>(cw, w); cnt_clear<WIDE>(hw, w); }
      }
      if (lane == 0) *n_touched = 0u;
      map_wave_sync();
    }
    __syncthreads();      // every record of the pair is written, every counter is zero again: the counters' LDS serves the one-per-bin rule
    for (uint32_t f = threadIdx.x; f < nf; f += blockDim.x) {
      const uint32_t h = row[f].hits, n = row[f].n;
      double ident = 0.0;
      if (n > 0u && h >= 2u) ident = kmer == 16 ? pgs::frag_identity(h, n, 16) : pgs::frag_identity(h, n, kmer);
      row[f].identity = ident;
      if (ident >= pgs::MIN_IDENTITY) atomicMax(&best_bits[row[f].bin], (unsigned long long)__double_as_longlong(ident));
    }
    __syncthreads();
    for (uint32_t f = threadIdx.x; f < nf; f += blockDim.x) {
      const double ident = row[f].identity;
      if (ident >= pgs::MIN_IDENTITY && best_bits[row[f].bin] == (unsigned long long)__double_as_longlong(ident)) atomicMax(&best_nidx[row[f].bin], ~f);
    }
    __syncthreads();
    for (uint32_t f = threadIdx.x; f < nf; f += blockDim.x) {
      const double ident = row[f].identity;
      row[f].kept = ident >= pgs::MIN_IDENTITY && best_bits[row[f].bin] == (unsigned long long)__double_as_longlong(ident) && best_nidx[row[f].bin] == ~f;
    }
    __syncthreads();
    for (uint32_t f = threadIdx.x; f < nf; f += blockDim.x)
      if (row[f].identity >= pgs::MIN_IDENTITY) { best_bits[row[f].bin] = 0ull; best_nidx[row[f].bin] = 0u; }
    if (wave == 0) {      // the definition's order: the survivors' identities in ascending fragment order, one running sum (every lane the same)
      double sum = 0.0;
      int32_t matches = 0;
      for (uint32_t base = 0; base < nf; base += 64u) {
        const uint32_t f = base + lane;
        const bool kept = f < nf && row[f].kept != 0;
        const double v = kept ? row[f].identity : 0.0;      // (x + 0.0 == x: a fragment that is not kept leaves the sum as it is)
        matches += (int32_t)__popcll(__ballot(kept));
        for (int j = 0; j < 64; ++j) sum = sum + __shfl(v, j, 64);
      }
      if (lane == 0) {
        pg_sketch_result o;
        o.matches = matches; o.fragments = (int32_t)nf;
        const bool enough = matches > 0 && (double)matches >= min_fraction * (double)nf;
        o.ani = enough ? sum / (double)matches : 0.0;
        o.status = enough ? 0 : PG_SKETCH_NO_RESULT; o.reserved = 0;
        out[J->out] = o;
      }
    }
    __syncthreads();      // the rule's LDS is zero again before the next pair counts in it
  }
}

template <bool FILL>
auto index_kernel_of(int32_t kmer) -> decltype(&index_scan_kernel<FILL, 16>) {
  switch (kmer) {
    case 8: return index_scan_kernel<FILL, 8>;
    case 9: return index_scan_kernel<FILL, 9>;
    case 10: return index_scan_kernel<FILL, 10>;
    case 11: return index_scan_kernel<FILL, 11>;
    case 12: return index_scan_kernel<FILL, 12>;
    case 13: return index_scan_kernel<FILL, 13>;
    case 14: return index_scan_kernel<FILL, 14>;
    case 15: return index_scan_kernel<FILL, 15>;
    case 16: return index_scan_kernel<FILL, 16>;
  }
  return nullptr;
}

// n keys of ST->keys_a sorted on their low `bits` bits into ST->keys_b
int map_sort_keys(pg_ctx* ctx, SketchStore* ST, uint32_t n, int bits) {
  size_t tmp = 0;
  int rc;
  PG_HIP(ctx, hipcub::DeviceRadixSort::SortKeys(nullptr, tmp, (const unsigned long long*)ST->keys_a, (unsigned long long*)ST->keys_b, (int)n, 0, bits, ctx->stream));
  if (ST->sort_tmp.cap < tmp + 1 && (rc = sk_malloc(ctx, ST->sort_tmp, tmp + 1))) return rc;
  PG_HIP(ctx, hipcub::DeviceRadixSort::SortKeys((void*)ST->sort_tmp.p, tmp, (const unsigned long long*)ST->keys_a, (unsigned long long*)ST->keys_b, (int)n, 0, bits, ctx->stream));
  return PG_OK;
}
int map_key_room(pg_ctx* ctx, SketchStore* ST, size_t n) {
  int rc;
  if (ST->keys_a.cap < n + 1 && (rc = sk_malloc(ctx, ST->keys_a, n + 1))) return rc;
  if (ST->keys_b.cap < n + 1 && (rc = sk_malloc(ctx, ST->keys_b, n + 1))) return rc;
  return PG_OK;
}
int bits_of(uint32_t x) { int b = 0; while (b < 32 && (x >> b)) ++b; return b; }      // bits that hold 0 ... x

int build_index(pg_ctx* ctx, SketchStore* ST, int32_t gid, int32_t kmer, int32_t scale, uint32_t log2_scale, bool* built_now) {
  MapIndex& X = ST->idx[gid];
  if (X.built && X.kmer == kmer && X.scale == scale) return PG_OK;
  const auto scan_count = index_kernel_of<false>(kmer);
  const auto scan_fill = index_kernel_of<true>(kmer);
  if (!scan_count || !scan_fill) return pg_fail(ctx, PG_E_ARG, "sketch: no scan kernel for this k-mer size");
  X = MapIndex{};
  *built_now = true;
  const PgGenome& G = ctx->genomes[gid];
  int rc;
  PgDevBuf<int32_t> rec_start;
  if ((rc = sk_malloc(ctx, rec_start, (size_t)G.n_rec + 1))) return rc;
  PG_HIP(ctx, hipMemcpyAsync(rec_start, G.rec_start.data(), ((size_t)G.n_rec + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
  if (!ST->counters && (rc = sk_malloc(ctx, ST->counters, 2))) return rc;
  PG_HIP(ctx, hipMemsetAsync(ST->counters, 0, 8, ctx->stream));
  const uint32_t* codes = ctx->d_codes + G.arena_start / 16;
  const uint32_t* mask = ctx->d_mask + G.arena_start / 32;
  const dim3 grid((uint32_t)std::min<uint64_t>((G.stream_len / 32 + 255) / 256 + 1, (uint64_t)ctx->num_cu * 8));
  hipLaunchKernelGGL(scan_count, grid, dim3(256), 0, ctx->stream, codes, mask, (int64_t)G.stream_len, rec_start, (int)G.n_rec, (uint32_t)scale,
                     log2_scale, ST->counters, nullptr, 0u, nullptr, 0u);
  PG_HIP(ctx, hipGetLastError());
  uint32_t n = 0;
  PG_HIP(ctx, hipMemcpyAsync(&n, ST->counters, 4, hipMemcpyDeviceToHost, ctx->stream));
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  uint32_t cap = 1024;
  while (cap < 2 * n) cap <<= 1;
  X.cap_mask = cap - 1; X.n_pos = n; X.kmer = kmer; X.scale = scale;
  if ((rc = sk_malloc(ctx, X.tab, (size_t)cap))) return rc;
  if ((rc = sk_malloc(ctx, X.off, (size_t)cap + 1))) return rc;
  if ((rc = sk_malloc(ctx, X.pos, (size_t)n + 1))) return rc;
  if ((rc = map_key_room(ctx, ST, n))) return rc;
  PG_HIP(ctx, hipMemsetAsync(X.tab, 0xFF, (size_t)cap * 4, ctx->stream));
  PG_HIP(ctx, hipMemsetAsync(ST->counters, 0, 8, ctx->stream));
  hipLaunchKernelGGL(scan_fill, grid, dim3(256), 0, ctx->stream, codes, mask, (int64_t)G.stream_len, rec_start, (int)G.n_rec, (uint32_t)scale,
                     log2_scale, ST->counters, X.tab, X.cap_mask, ST->keys_a, n);
  PG_HIP(ctx, hipGetLastError());
  if (n && (rc = map_sort_keys(ctx, ST, n, 32 + bits_of(X.cap_mask)))) return rc;
  const uint32_t top = std::max(n, cap + 1);
  hipLaunchKernelGGL(map_unpack_kernel, dim3(std::min<uint32_t>((top + 255) / 256, (uint32_t)ctx->num_cu * 8)), dim3(256), 0, ctx->stream,
                     ST->keys_b, n, X.pos, X.off, cap + 1);
  PG_HIP(ctx, hipGetLastError());
  PG_HIP(ctx, hipStreamSynchronize(ctx->stream));      // rec_start goes out of scope
  X.built = true;
  return PG_OK;
}

int build_grouped(pg_ctx* ctx, SketchStore* ST, int32_t gid, bool* built_now) {
  SketchGenome& S = ST->g[gid];
  if (S.grouped) return PG_OK;
  *built_now = true;
  int rc;
  if ((rc = sk_malloc(ctx, S.grp_kmer, (size_t)S.n_occ + 1))) return rc;
  if ((rc = sk_malloc(ctx, S.frag_off, (size_t)S.n_frags + 1))) return rc;
  if ((rc = map_key_room(ctx, ST, S.n_occ))) return rc;
  if (S.n_occ) {
    hipLaunchKernelGGL(map_pack_kernel, dim3(std::min<uint32_t>((S.n_occ + 255) / 256, (uint32_t)ctx->num_cu * 8)), dim3(256), 0, ctx->stream,
                       S.occ_frag, S.occ_kmer, S.n_occ, ST->keys_a);
    PG_HIP(ctx, hipGetLastError());
    if ((rc = map_sort_keys(ctx, ST, S.n_occ, 32 + bits_of(S.n_frags)))) return rc;
  }
  const uint32_t top = std::max(S.n_occ, S.n_frags + 1);
  hipLaunchKernelGGL(map_unpack_kernel, dim3(std::min<uint32_t>((top + 255) / 256, (uint32_t)ctx->num_cu * 8)), dim3(256), 0, ctx->stream,
                     ST->keys_b, S.n_occ, S.grp_kmer, S.frag_off, S.n_frags + 1);
  PG_HIP(ctx, hipGetLastError());
  S.grouped = true;
  return PG_OK;
}

struct MapEvents {      // pg_sketch_map_last_ms: the build section and the mapping kernel of one call, on the context's stream
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  bool ok = true;
  MapEvents() { for (auto& e : ev) if (hipEventCreate(&e) != hipSuccess) { (void)hipGetLastError(); e = nullptr; ok = false; } }
  ~MapEvents() { for (auto& e : ev) if (e) (void)hipEventDestroy(e); }
  void mark(int k, hipStream_t s) { if (ok && hipEventRecord(ev[k], s) != hipSuccess) { (void)hipGetLastError(); ok = false; } }
  double ms(int a, int b) { float x = 0.f; return ok && hipEventElapsedTime(&x, ev[a], ev[b]) == hipSuccess ? (double)x : 0.0; }
};

// The mapped call: pairs -> out (host), or with `rows_out` the fragment records of ONE pair (at most rows_cap of them; *n_rows = how many)
int run_mapped(pg_ctx* ctx, const int32_t* qry_ids, const int32_t* ref_ids, uint64_t n_pairs, int32_t kmer, int32_t frag_len, int32_t scale,
               double min_fraction, pg_sketch_result* out, pg_sketch_fragment* rows_out, uint64_t rows_cap, uint64_t* n_rows) {
  PG_HIP(ctx, hipSetDevice(ctx->device));
  int rc;
  if ((rc = pg_upload(ctx))) return rc;
  SketchStore* ST = store_of(ctx);
  if (ST->g.size() < ctx->genomes.size()) ST->g.resize(ctx->genomes.size());
  if (ST->idx.size() < ctx->genomes.size()) ST->idx.resize(ctx->genomes.size());
  ST->map_ms[0] = ST->map_ms[1] = 0.0;
  uint32_t log2_scale = 0;
  while ((1 << log2_scale) < scale) ++log2_scale;
  const bool wide = frag_len > 65535;
  const uint32_t max_bins = wide ? MAP_MAX_BINS_WIDE : MAP_MAX_BINS;
  std::vector<char> is_q(ctx->genomes.size(), 0), is_r(ctx->genomes.size(), 0);
  for (uint64_t i = 0; i < n_pairs; ++i) { is_q[qry_ids[i]] = 1; is_r[ref_ids[i]] = 1; }
  uint32_t nb_max = 1;
  for (size_t g = 0; g < is_r.size(); ++g) {
    if (!is_r[g]) continue;
    const uint64_t len = ctx->genomes[g].total_len;
    if ((len + (uint64_t)frag_len - 1) / (uint64_t)frag_len > max_bins)
      return pg_fail(ctx, PG_E_CAPACITY, "sketch (mapped): a reference genome of more than " + std::to_string((uint64_t)max_bins * (uint64_t)frag_len) +
                                             " bases at frag_len " + std::to_string(frag_len) + " (" + std::to_string(max_bins) +
                                             " bins of frag_len bases: the counters one wave keeps in LDS)");
    nb_max = std::max(nb_max, pgs::map_bins(len, (uint32_t)frag_len));
  }
  MapEvents T;
  bool built_now = false;
  T.mark(0, ctx->stream);
  for (size_t g = 0; g < is_q.size(); ++g) {
    if (is_q[g] && ((rc = build_sketch(ctx, ST, (int32_t)g, kmer, frag_len, scale, log2_scale)) || (rc = build_grouped(ctx, ST, (int32_t)g, &built_now)))) return rc;
    if (is_r[g] && (rc = build_index(ctx, ST, (int32_t)g, kmer, scale, log2_scale, &built_now))) return rc;
  }
  T.mark(1, ctx->stream);
  // jobs by reference, then query: the workgroups running side by side share a reference's index in L2
  std::vector<uint64_t> order(n_pairs);
  for (uint64_t i = 0; i < n_pairs; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return ref_ids[a] != ref_ids[b] ? ref_ids[a] < ref_ids[b] : qry_ids[a] < qry_ids[b]; });
  std::vector<MapJob> jobs(n_pairs);
  uint32_t nf_max = 1;
  for (uint64_t a = 0; a < n_pairs; ++a) {
    const SketchGenome& Q = ST->g[qry_ids[order[a]]];
    const MapIndex& X = ST->idx[ref_ids[order[a]]];
    MapJob& J = jobs[a];
    J.grp_kmer = Q.grp_kmer; J.frag_off = Q.frag_off; J.tab = X.tab; J.off = X.off; J.pos = X.pos;
    J.n_frags = Q.n_frags; J.cap_mask = X.cap_mask; J.nb = pgs::map_bins(ctx->genomes[ref_ids[order[a]]].total_len, (uint32_t)frag_len);
    J.out = (uint32_t)order[a];
    nf_max = std::max(nf_max, Q.n_frags);
  }
  const uint32_t nb_stride = (nb_max + 7u) & ~7u;
  const size_t lds = (size_t)MAP_WAVES * 2 * nb_stride * (wide ? 4 : 2) + (size_t)MAP_WAVES * MAP_TOUCH * 4 + MAP_WAVES * 4;
  const uint32_t n_wg = (uint32_t)std::min<uint64_t>(n_pairs, (uint64_t)ctx->num_cu * 4);
  PgDevBuf<MapJob> d_jobs;
  PgDevBuf<pg_sketch_result> d_out;
  PgDevBuf<pg_sketch_fragment> d_rows;      // one row of the longest query per resident workgroup
  if ((rc = sk_malloc(ctx, d_jobs, jobs.size()))) return rc;
  if ((rc = sk_malloc(ctx, d_out, (size_t)n_pairs))) return rc;
  if ((rc = sk_malloc(ctx, d_rows, (size_t)n_wg * nf_max))) return rc;
  PG_HIP(ctx, hipMemcpyAsync(d_jobs, jobs.data(), jobs.size() * sizeof(MapJob), hipMemcpyHostToDevice, ctx->stream));
  const auto kernel = wide ? sketch_map_kernel<true> : sketch_map_kernel<false>;
  if (lds > 48 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    (void)hipGetLastError();
    return pg_fail(ctx, PG_E_CAPACITY, "sketch (mapped): the bin counters need " + std::to_string(lds) + " bytes of LDS per workgroup, which this device does not grant");
  }
  T.mark(2, ctx->stream);
  pg_prof_begin(ctx, PG_K_SKETCH_PAIRS);
  hipLaunchKernelGGL(kernel, dim3(n_wg), dim3(64 * MAP_WAVES), lds, ctx->stream, d_jobs, (uint32_t)n_pairs, d_rows, (uint64_t)nf_max, d_out, kmer,
                     (uint32_t)frag_len, log2_scale, min_fraction, nb_stride);
  pg_prof_end(ctx);
  hipError_t e = hipGetLastError();
  T.mark(3, ctx->stream);
  if (e == hipSuccess && out) e = hipMemcpyAsync(out, d_out, n_pairs * sizeof(pg_sketch_result), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && n_rows) {      // (one pair, one workgroup: its row is the pair's)
    *n_rows = jobs[0].n_frags;
    const uint64_t n_copy = std::min<uint64_t>(rows_cap, jobs[0].n_frags);
    if (n_copy && rows_out) e = hipMemcpyAsync(rows_out, d_rows, n_copy * sizeof(pg_sketch_fragment), hipMemcpyDeviceToHost, ctx->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return pg_fail(ctx, PG_E_HIP, std::string("sketch (mapped): ") + hipGetErrorString(e));
  ST->map_ms[0] = built_now ? T.ms(0, 1) : 0.0;
  ST->map_ms[1] = T.ms(2, 3);
  return PG_OK;
}

int check_sketch_args(pg_ctx* ctx, int32_t kmer, int32_t frag_len, int32_t scale, double min_fraction) {
  if (kmer < pgs::K_MIN || kmer > pgs::K_MAX) return pg_fail(ctx, PG_E_ARG, "sketch: the k-mer size must be 8 ... 16");
  if (frag_len < 64 || scale < 1 || scale > 4096 || (scale & (scale - 1)) || !(min_fraction >= 0.0 && min_fraction <= 1.0))
    return pg_fail(ctx, PG_E_ARG, "sketch: frag_len >= 64, scale a power of two <= 4096, 0 <= min_fraction <= 1");
  return PG_OK;
}

}  // namespace

void pg_sketch_drop(pg_ctx* ctx) {
  delete static_cast<SketchStore*>(ctx->sketch_store);
  ctx->sketch_store = nullptr;
}

extern "C" int pg_sketch_pairs(pg_ctx* ctx, const int32_t* qry_ids, const int32_t* ref_ids, uint64_t n_pairs, int32_t frag_len, int32_t scale,
                               double min_fraction, pg_sketch_result* out) {
  return pg_sketch_pairs_k(ctx, qry_ids, ref_ids, n_pairs, 16, frag_len, scale, min_fraction, out);      // fastANI's default -k 16: one code path
}

extern "C" int pg_sketch_pairs_k(pg_ctx* ctx, const int32_t* qry_ids, const int32_t* ref_ids, uint64_t n_pairs, int32_t kmer, int32_t frag_len,
                                 int32_t scale, double min_fraction, pg_sketch_result* out) {
  if (!ctx || !out || (n_pairs && (!qry_ids || !ref_ids))) return pg_fail(ctx, PG_E_ARG, "bad argument");
  if (kmer < pgs::K_MIN || kmer > pgs::K_MAX) return pg_fail(ctx, PG_E_ARG, "sketch: the k-mer size must be 8 ... 16");
  if (frag_len < 64 || scale < 1 || scale > 4096 || (scale & (scale - 1)) || !(min_fraction >= 0.0 && min_fraction <= 1.0))
    return pg_fail(ctx, PG_E_ARG, "sketch: frag_len >= 64, scale a power of two <= 4096, 0 <= min_fraction <= 1");
  for (uint64_t i = 0; i < n_pairs; ++i)
    if (qry_ids[i] < 0 || (size_t)qry_ids[i] >= ctx->genomes.size() || ref_ids[i] < 0 || (size_t)ref_ids[i] >= ctx->genomes.size())
      return pg_fail(ctx, PG_E_ARG, "genome id out of range");
  if (n_pairs == 0) return PG_OK;
  PG_HIP(ctx, hipSetDevice(ctx->device));
  int rc;
  if ((rc = pg_upload(ctx))) return rc;
  SketchStore* ST = store_of(ctx);
  if (ST->g.size() < ctx->genomes.size()) ST->g.resize(ctx->genomes.size());
  uint32_t log2_scale = 0;
  while ((1 << log2_scale) < scale) ++log2_scale;
  std::vector<char> need(ctx->genomes.size(), 0);
  for (uint64_t i = 0; i < n_pairs; ++i) { need[qry_ids[i]] = 1; need[ref_ids[i]] = 1; }
  for (size_t g = 0; g < need.size(); ++g)
    if (need[g] && (rc = build_sketch(ctx, ST, (int32_t)g, kmer, frag_len, scale, log2_scale))) return rc;
  // jobs: the pairs by query, up to SK_REFS references per workgroup (fewer when the query's fragment counters would not fit LDS)
  std::vector<uint64_t> idx(n_pairs);
  for (uint64_t i = 0; i < n_pairs; ++i) idx[i] = i;
  std::stable_sort(idx.begin(), idx.end(), [&](uint64_t a, uint64_t b) { return qry_ids[a] != qry_ids[b] ? qry_ids[a] < qry_ids[b] : ref_ids[a] < ref_ids[b]; });
  std::vector<SketchJob> jobs;
  size_t lds_max = 0;
  for (uint64_t a = 0; a < n_pairs;) {
    const SketchGenome& Q = ST->g[qry_ids[idx[a]]];
    const size_t per_ref = (size_t)std::max<uint32_t>(Q.n_frags, 1u) * 4;
    if (per_ref > 96 * 1024) return pg_fail(ctx, PG_E_CAPACITY, "sketch: more than 24 576 fragments in one query genome");
    const uint32_t g_max = (uint32_t)std::min<size_t>(SK_REFS, (96 * 1024) / per_ref);
    SketchJob J{};
    J.occ_kmer = Q.occ_kmer; J.occ_frag = Q.occ_frag; J.frag_n = Q.frag_n; J.n_occ = Q.n_occ; J.n_frags = Q.n_frags; J.log2_scale = log2_scale; J.kmer = kmer;
    J.min_fraction = min_fraction;
    uint32_t g = 0;
    while (a < n_pairs && g < g_max && qry_ids[idx[a]] == qry_ids[idx[a - g]]) {
      const SketchGenome& Rf = ST->g[ref_ids[idx[a]]];
      J.tab[g] = Rf.tab; J.cap_mask[g] = Rf.cap_mask; J.out[g] = (uint32_t)idx[a];
      ++g; ++a;
    }
    J.n_refs = g;
    lds_max = std::max(lds_max, per_ref * g);
    jobs.push_back(J);
  }
  PgDevBuf<SketchJob> d_jobs;
  PgDevBuf<pg_sketch_result> d_out;
  if ((rc = sk_malloc(ctx, d_jobs, jobs.size()))) return rc;
  if ((rc = sk_malloc(ctx, d_out, (size_t)n_pairs))) return rc;
  PG_HIP(ctx, hipMemcpyAsync(d_jobs, jobs.data(), jobs.size() * sizeof(SketchJob), hipMemcpyHostToDevice, ctx->stream));
  if (lds_max > 48 * 1024) {      // up to 96 KiB of dynamic LDS: fits gfx950's 160 KiB per workgroup; a part that refuses it gets a clear status, not a launch failure
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(sketch_pairs_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(96 * 1024)) != hipSuccess) {
      (void)hipGetLastError();
      return pg_fail(ctx, PG_E_CAPACITY, "sketch: the job's fragment counters need up to 96 KiB of LDS per workgroup, which this device does not grant");
    }
  }
  pg_prof_begin(ctx, PG_K_SKETCH_PAIRS);
  hipLaunchKernelGGL(sketch_pairs_kernel, dim3((uint32_t)jobs.size()), dim3(256), std::max<size_t>(lds_max, 16), ctx->stream, d_jobs, d_out);
  pg_prof_end(ctx);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, n_pairs * sizeof(pg_sketch_result), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return pg_fail(ctx, PG_E_HIP, std::string("sketch: ") + hipGetErrorString(e));
  return PG_OK;
}

extern "C" int pg_sketch_pairs_mapped(pg_ctx* ctx, const int32_t* qry_ids, const int32_t* ref_ids, uint64_t n_pairs, int32_t kmer, int32_t frag_len,
                                      int32_t scale, double min_fraction, pg_sketch_result* out) {
  if (!ctx || !out || (n_pairs && (!qry_ids || !ref_ids))) return pg_fail(ctx, PG_E_ARG, "bad argument");
  int rc;
  if ((rc = check_sketch_args(ctx, kmer, frag_len, scale, min_fraction))) return rc;
  if (n_pairs > 0xFFFFFFFFull) return pg_fail(ctx, PG_E_ARG, "sketch (mapped): more than 2^32 - 1 pairs in one call");
  for (uint64_t i = 0; i < n_pairs; ++i)
    if (qry_ids[i] < 0 || (size_t)qry_ids[i] >= ctx->genomes.size() || ref_ids[i] < 0 || (size_t)ref_ids[i] >= ctx->genomes.size())
      return pg_fail(ctx, PG_E_ARG, "genome id out of range");
  if (n_pairs == 0) return PG_OK;
  return run_mapped(ctx, qry_ids, ref_ids, n_pairs, kmer, frag_len, scale, min_fraction, out, nullptr, 0, nullptr);
}

extern "C" int pg_sketch_pair_fragments(pg_ctx* ctx, int32_t qry_id, int32_t ref_id, int32_t kmer, int32_t frag_len, int32_t scale,
                                        pg_sketch_fragment* out, uint64_t cap, uint64_t* n_out) {
  if (!ctx || !n_out || (cap && !out)) return pg_fail(ctx, PG_E_ARG, "bad argument");
  int rc;
  if ((rc = check_sketch_args(ctx, kmer, frag_len, scale, 0.0))) return rc;
  if (qry_id < 0 || (size_t)qry_id >= ctx->genomes.size() || ref_id < 0 || (size_t)ref_id >= ctx->genomes.size())
    return pg_fail(ctx, PG_E_ARG, "genome id out of range");
  pg_sketch_result res;
  return run_mapped(ctx, &qry_id, &ref_id, 1, kmer, frag_len, scale, 0.0, &res, out, cap, n_out);
}

extern "C" int pg_sketch_map_last_ms(pg_ctx* ctx, double* out2) {
  if (!ctx || !out2) return pg_fail(ctx, PG_E_ARG, "bad argument");
  const SketchStore* ST = static_cast<const SketchStore*>(ctx->sketch_store);
  out2[0] = ST ? ST->map_ms[0] : 0.0;
  out2[1] = ST ? ST->map_ms[1] : 0.0;
  return PG_OK;
}
