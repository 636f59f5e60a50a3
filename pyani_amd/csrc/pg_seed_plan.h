// pg_seed_plan.h — the pass arithmetic of the seeding stage (pga_seed.inc, pg_anim.hip), in one place.  Plain C++ for host and
// device, no HIP calls (tests/seed_plan/plan_check.cpp compiles it with g++).
//
// A seeding workgroup puts the reference entries of one k-mer group into an LDS hash table of S slots (a power of two) and
// streams the queries' entries of the same group through it.  The table is filled to at most half, so that every probe
// sequence meets an empty slot.  A group of n entries that does not fit is cut into passes of at most H = S / 2 consecutive
// entries of its list; every pass is filled and probed by the same query stream in turn.  A hit is a (reference entry, query
// entry) pair with equal keys, and every reference entry is in exactly one pass: every hit is found exactly once.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PG_SEED_PLAN_FN __host__ __device__ inline
#else
#define PG_SEED_PLAN_FN inline
#endif

struct PgSeedPass { uint32_t begin, end; };   // entries [begin, end) of the group's list

// entries a table of `slots` slots takes per pass
PG_SEED_PLAN_FN uint32_t pg_seed_pass_entries(uint32_t slots) { return slots / 2u; }

// passes of a group of n entries: max(1, ceil(n / H)) — an empty group still takes its (empty) pass
PG_SEED_PLAN_FN uint32_t pg_seed_pass_count(uint32_t n, uint32_t slots) {
  const uint32_t h = pg_seed_pass_entries(slots);
  const uint32_t p = n / h + (n % h ? 1u : 0u);   // (no n + h - 1: n may be close to 2^32)
  return p ? p : 1u;
}

// pass p (p < pg_seed_pass_count) of a group of n entries: [p H, min(n, (p + 1) H))
PG_SEED_PLAN_FN PgSeedPass pg_seed_pass_range(uint32_t n, uint32_t slots, uint32_t p) {
  const uint32_t h = pg_seed_pass_entries(slots);
  const uint32_t b = p * h;
  return PgSeedPass{b, n - b < h ? n : b + h};
}
