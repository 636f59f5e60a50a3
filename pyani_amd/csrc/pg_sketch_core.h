// pg_sketch_core.h — the definition of the SKETCH mode ("fastANI-style sketch mode"), plain C++ for the device
// (pg_sketch.hip) and for the host checker of the tests.
//
// What it stands in for: pyani's fastANI wrapper (pyani/fastani.py:193-270) shells out to `fastANI -q query -r ref --fragLen 3000
// -k 16 --minFraction 0.2` and reads back one line: query, reference, ANI estimate (percent), orthologous matches, query fragments
// (parse_fastani_file -> ComparisonResult(reference, query, ani, matches, fragments)).  fastANI (third-party, absent from the
// reference tree and the image) maps every non-overlapping fragLen piece of the query to the reference through MinHash sketches of
// its 16-mers and averages the pieces' identity estimates.  This mode computes an estimate of the same SHAPE — same inputs, same
// three outputs, same minFraction rule — with an estimator that needs no mapping step:
//
//   * 8 <= k <= 16 (fastANI's --kmer, "kmer size <= 16"; default 16): a k-mer of the 2-bit alphabet IS a 2k-bit integer, first base in
//     the HIGH bits of the 2k-bit field; canonical form = min(forward, reverse complement); windows with an ambiguity symbol or across
//     a record end do not exist (the k mask bits of the packed stream, as everywhere in this engine);
//   * FracMinHash sampling: a canonical k-mer belongs to every sketch iff mix32(kmer) & (scale - 1) == 0 (scale = 16 by default:
//     ~190 sampled k-mers per 3 000-base fragment, ~3 x 10^5 per 5 Mb genome);
//   * the query genome's records are cut into non-overlapping fragments of frag_len bases (a record's tail shorter than that is
//     dropped, as fastANI does); a sampled k-mer belongs to the fragment that contains all k of its bases;
//   * per fragment: n = its sampled k-mer occurrences, h = those that occur ANYWHERE in the reference genome (either strand);
//     containment C = h / n, and since a k-mer survives iff none of its k bases changed, identity = C^(1/k).  k = 16: four square
//     roots.  k = 8 ... 15: start y = the four square roots of C (C^(1/16) >= C^(1/k): at or above the root), then EXACTLY 12 Newton
//     steps on y^k = C, each p = y; k - 2 times p = p * y; y = y - (p * y - C) / (k * p).  Every operation is correctly rounded on its
//     own on host and device (no contraction: -ffp-contract=off), so the estimate is reproducible bit for bit.  The count 12 is part
//     of the definition: after convergence the iteration flips between neighbouring doubles (within 1 ulp of the root for every
//     2 <= h <= n <= 4096; nine steps are the first count under 1 ulp at k = 8).  A step from above never goes below the root and the
//     start is below 0.80 whenever C < 0.8^16, so a tiny C that 12 steps do not finish cannot turn a non-match into a match;
//   * a fragment MATCHES iff h >= 2 and identity >= 0.80 (fastANI's floor: below that its mapper finds nothing either);
//   * ANI = mean identity of the matching fragments (summed in fragment order), matches = how many, fragments = all of them;
//     fewer matches than min_fraction * fragments: no result (fastANI writes an empty file; parse_fastani_file raises).
//
// MAPPED variant (mapping = "window", opt-in: pg_sketch_pairs_mapped).  Everything above stays — k, canonical k-mers, sampling, the
// query's fragments, which occurrence belongs to which fragment, n, frag_identity, frag_matches, the min_fraction rule — but a
// fragment's hits must fall inside ONE window of the reference, as a fastANI mapping does, and a reference bin keeps one fragment:
//   * a sampled occurrence of the reference has the coordinate g = its start in the genome's sequence with the records back to back
//     and NO separator base; with L = frag_len, bin b = g / L of nb = ceil(genome length / L) bins (map_bins); window w (0 <= w < nb)
//     is bins w and w + 1 (the last window: bin nb - 1 alone).  A window may span a record boundary;
//   * per query fragment, for every sampled occurrence x (with multiplicity, as n counts them) B(x) = the bins in which its canonical
//     k-mer occurs in the reference; c_b = occurrences with b in B(x); h_w = occurrences with B(x) meeting {w, w + 1}: an occurrence
//     counts once per bin and once per window, however many copies the reference holds;
//   * h = max h_w, w* = the LOWEST window that reaches it (map_window_key orders (h, w) that way); bin = w* if c_w* >= c_(w* + 1), else
//     w* + 1 (map_pick_bin; a c beyond nb - 1 is 0) — without this a fragment that lies exactly on bin f ties between windows f - 1 and f
//     and collides with its neighbour; h = 0: w* = bin = -1; identity = frag_identity(h, n, k), candidate iff frag_matches(h, n, k);
//   * one fragment per bin: among the candidates of one bin the larger identity (compared as doubles) wins, ties go to the lowest
//     fragment index (positive doubles order like their bit patterns: a max over the bits, then a min over the index among equals);
//   * matches = the survivors, ANI = their identities summed in fragment order / matches, fragments = all of them; min_fraction as above.
//
// It is an ESTIMATE with its own columns, never written into the exact ANIm / ANIb matrices; tests/test_sketch_gpu.py holds the GPU
// against the numpy restatement of this definition (bit-exact) and prices the estimate against the exact engine on C3 pairs.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PGS_HD __host__ __device__ __forceinline__
#else
#define PGS_HD inline
#endif

namespace pgs {

constexpr int K_MIN = 8, K_MAX = 16;
constexpr int NEWTON_STEPS = 12;             // part of the definition (see above)
constexpr double MIN_IDENTITY = 0.80;
constexpr uint32_t EMPTY = 0xFFFFFFFFu;      // (no canonical k-mer, k <= 16, has this value: min(x, rc x) < 2^32 - 1)

PGS_HD uint32_t mix32(uint32_t h) {          // murmur3's finaliser: a bijection of the 32-bit k-mer
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}
PGS_HD uint32_t kmer_mask(int k) { return k >= 16 ? 0xFFFFFFFFu : (1u << (2 * k)) - 1u; }      // the 2k-bit field
// forward word: first base in the HIGH bits of the 2k-bit field; rc word likewise for the reverse complement
PGS_HD uint32_t roll_fwd(uint32_t f, uint32_t code, int k) { return ((f << 2) | code) & kmer_mask(k); }
PGS_HD uint32_t roll_rc(uint32_t r, uint32_t code, int k) { return (r >> 2) | ((3u - code) << (2 * (k - 1))); }
PGS_HD bool sampled(uint32_t canon, uint32_t scale) { return (mix32(canon) & (scale - 1u)) == 0u; }
PGS_HD uint32_t slot_of(uint32_t canon, uint32_t log2_scale, uint32_t cap_mask) { return (mix32(canon) >> log2_scale) & cap_mask; }
PGS_HD double sqrt_rn(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dsqrt_rn(x);
#else
  return __builtin_sqrt(x);
#endif
}
// identity estimate of a fragment with h of n sampled k-mers found: (h / n)^(1/k); callers ask only with h >= 2 and n > 0
PGS_HD double frag_identity(uint32_t h, uint32_t n, int k) {
  const double c = (double)h / (double)n;
  double y = sqrt_rn(sqrt_rn(sqrt_rn(sqrt_rn(c))));
  if (k == 16) return y;
  const double kd = (double)k;
  for (int it = 0; it < NEWTON_STEPS; ++it) {
    double p = y;
    for (int j = 0; j < k - 2; ++j) p = p * y;      // y^(k - 1)
    y = y - (p * y - c) / (kd * p);
  }
  return y;
}
// ---- the mapped variant's coordinates and tie rules (see above) ----
PGS_HD uint32_t map_bins(uint64_t genome_len, uint32_t frag_len) { return (uint32_t)((genome_len + frag_len - 1u) / frag_len); }
// (hits, window) as one integer whose maximum is the most hits in the lowest window
PGS_HD uint64_t map_window_key(uint32_t h, uint32_t w) { return ((uint64_t)h << 32) | (uint64_t)(0xFFFFFFFFu - w); }
PGS_HD uint32_t map_key_hits(uint64_t key) { return (uint32_t)(key >> 32); }
PGS_HD uint32_t map_key_window(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)key; }
PGS_HD int32_t map_pick_bin(int32_t w, uint32_t c_w, uint32_t c_next) { return c_w >= c_next ? w : w + 1; }
PGS_HD bool frag_matches(uint32_t h, uint32_t n, int k) { return n > 0u && h >= 2u && frag_identity(h, n, k) >= MIN_IDENTITY; }

}  // namespace pgs
