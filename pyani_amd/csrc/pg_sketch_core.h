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
PGS_HD bool frag_matches(uint32_t h, uint32_t n, int k) { return n > 0u && h >= 2u && frag_identity(h, n, k) >= MIN_IDENTITY; }

}  // namespace pgs
