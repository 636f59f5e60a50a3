// Host check of PgDevBuf (pyani_amd/csrc/pg_devbuf.h) against the fake runtime of tests/devbuf/hip: prints one line per check,
// "ok <name>" or "WRONG <name>", and returns the number of wrong ones.
#include <cstdio>
#include <utility>
#include "pg_devbuf.h"

static int wrong = 0;
static void check(bool ok, const char* name) {
  std::printf("%s %s\n", ok ? "ok" : "WRONG", name);
  if (!ok) ++wrong;
}

// The TETRA batch scratch of the context (pg_api.cpp, ensure_batch_scratch): eight arrays that grow as a group, in this order and
// with these elements per genome (d_seg_prefix holds one more).
struct BatchGroup {
  PgDevBuf<unsigned> gid, tile0, prefix;
  PgDevBuf<unsigned long long> acc, counts;
  PgDevBuf<double> dev, ss;
  PgDevBuf<unsigned long long> keybits;
  hipError_t grow(size_t n) {
    hipError_t e = hipSuccess;
    auto one = [&](auto& b, size_t per, size_t extra = 0) { if (e == hipSuccess) e = b.reserve_items(n, per, extra); };
    one(gid, 1); one(tile0, 1); one(prefix, 1, 1); one(acc, 336); one(counts, 336); one(dev, 256); one(ss, 1); one(keybits, 4);
    return e;
  }
  bool holds(size_t n) const {      // every member has a block for n genomes
    return gid.p && gid.cap >= n && tile0.p && tile0.cap >= n && prefix.p && prefix.cap >= n + 1 && acc.p && acc.cap >= n * 336 && counts.p &&
           counts.cap >= n * 336 && dev.p && dev.cap >= n * 256 && ss.p && ss.cap >= n && keybits.p && keybits.cap >= n * 4;
  }
};
static void grow_8_to_16_failing_the_fourth(BatchGroup& g) {
  g.grow(8);
  fake_hip().fail_at = 4;
  g.grow(16);
}

// The genome arena of the context (pg_api.cpp, pg_upload): the new blocks are locals that are moved into their holders once both exist.
static hipError_t replace_arena(PgDevBuf<unsigned>& codes, PgDevBuf<unsigned>& mask, size_t words) {
  PgDevBuf<unsigned> nc, nm;
  hipError_t e = nc.reserve(2 * words);
  if (e == hipSuccess) e = nm.reserve(words);
  if (e != hipSuccess) return e;
  codes = std::move(nc);
  mask = std::move(nm);
  return hipSuccess;
}

int main() {
  FakeHip& H = fake_hip();
  {
    PgDevBuf<double> b;
    check(b.p == nullptr && b.cap == 0 && H.mallocs == 0, "a new buffer is empty and allocates nothing");
    check(b.reserve(100, 125) == hipSuccess && b.p && b.cap == 125 && H.last_bytes == 125 * sizeof(double) && H.live == 1,
          "reserve allocates the amount the caller's growth rule names");
    const double* p0 = b.p;
    const long m0 = H.mallocs;
    check(b.reserve(125, 1000) == hipSuccess && b.reserve(7) == hipSuccess && b.p == p0 && b.cap == 125 && H.mallocs == m0 && H.frees == 0,
          "need <= cap allocates nothing");
    check(b.reserve(126, 200) == hipSuccess && b.cap == 200 && H.mallocs == m0 + 1 && H.frees == 1 && H.live == 1,
          "a growing reserve frees the old block exactly once");
    H.fail_at = 1;
    const long f0 = H.frees;
    check(b.reserve(1000, 1500) == hipErrorOutOfMemory && b.p == nullptr && b.cap == 0 && H.frees == f0 + 1 && H.live == 0,
          "after a failed reserve the buffer is empty");
    const long m1 = H.mallocs;
    check(b.reserve(50) == hipSuccess && b.p && b.cap == 50 && H.mallocs == m1 + 1 && H.live == 1,
          "a following smaller reserve allocates again");
    PgDevBuf<char> z;
    check(z.reserve(0) == hipSuccess && z.p == nullptr && H.mallocs == m1 + 1, "reserve(0) on an empty buffer allocates nothing");
    check(z.reserve(1, 0) == hipSuccess && z.p && z.cap == 1, "at least one element is allocated");
    z.release();
    check(z.p == nullptr && z.cap == 0 && H.live == 1, "release frees the block and empties the buffer");
  }
  check(H.live == 0, "the destructor frees the block");
  {
    PgDevBuf<int> a, c;
    a.reserve(10);
    c.reserve(20);
    int* pa = a.p;
    PgDevBuf<int> b(std::move(a));
    check(a.p == nullptr && a.cap == 0 && b.p == pa && b.cap == 10 && H.live == 2, "a move hands the block over");
    c = std::move(b);
    check(b.p == nullptr && b.cap == 0 && c.p == pa && c.cap == 10 && H.live == 1, "a move assignment frees the block it replaces");
  }
  check(H.live == 0 && H.mallocs == H.frees, "after the moves every block has been freed exactly once");
  {   // a group that grows together (pg_anim.hip's reserve_all pattern): the third allocation fails
    PgDevBuf<int> g[4];
    for (auto& b : g) b.reserve(8);
    H.fail_at = 3;
    hipError_t e = hipSuccess;
    for (auto& b : g) if (e == hipSuccess) e = b.reserve(16);
    check(e == hipErrorOutOfMemory && g[0].cap == 16 && g[1].cap == 16 && g[2].p == nullptr && g[2].cap == 0 && g[3].cap == 8,
          "a group whose third allocation failed: no size is stale");
    e = hipSuccess;
    for (auto& b : g) if (e == hipSuccess) e = b.reserve(12);      // the smaller batch a caller sends after the failure
    check(e == hipSuccess && g[0].cap == 16 && g[2].p && g[2].cap == 12 && g[3].cap == 12, "the next, smaller call completes the group");
  }
  check(H.live == 0, "nothing is left");
  {   // the pinned sibling: the same rules over hipHostMalloc / hipHostFree
    PgPinnedBuf<double> b;
    const long m0 = H.mallocs;
    check(b.p == nullptr && b.cap == 0 && H.mallocs == m0, "pinned: a new buffer is empty and allocates nothing");
    check(b.reserve(100, 125) == hipSuccess && b.p && b.cap == 125 && H.last_bytes == 125 * sizeof(double) && H.live == 1 &&
          b.reserve(126, 200) == hipSuccess && b.cap == 200 && H.mallocs == m0 + 2 && H.live == 1,
          "pinned: a growing reserve allocates what the growth rule names and frees the old block exactly once");
    H.fail_at = 1;
    check(b.reserve(1000, 1500) == hipErrorOutOfMemory && b.p == nullptr && b.cap == 0 && H.live == 0, "pinned: after a failed reserve the buffer is empty");
    check(b.reserve(50) == hipSuccess && b.p && b.cap == 50 && H.live == 1, "pinned: a following smaller reserve allocates again");
    b.release();
    check(b.p == nullptr && b.cap == 0 && H.live == 0, "pinned: release frees the block and empties the buffer");
    PgPinnedBuf<double> c;
    b.reserve(10);
    c.reserve(20);
    double* pb = b.p;
    PgPinnedBuf<double> d(std::move(b));
    c = std::move(d);
    check(b.p == nullptr && b.cap == 0 && d.p == nullptr && d.cap == 0 && c.p == pb && c.cap == 10 && H.live == 1,
          "pinned: the moves hand the block over and free the one they replace");
  }
  check(H.live == 0 && H.mallocs == H.frees, "pinned: the destructor frees the block, none twice");
  {   // the batch scratch group, growing from 8 to 16 genomes: the fourth allocation (d_acc) fails
    BatchGroup g;
    grow_8_to_16_failing_the_fourth(g);
    check(g.gid.cap == 16 && g.tile0.cap == 16 && g.prefix.cap == 17 && g.acc.p == nullptr && g.acc.cap == 0 && g.counts.cap == 8 * 336 &&
          g.dev.cap == 8 * 256 && g.ss.cap == 8 && g.keybits.cap == 8 * 4 && H.live == 7,
          "batch group whose fourth allocation failed: no member reports a size it does not hold");
    check(!g.holds(12) && g.grow(12) == hipSuccess && g.holds(12) && H.live == 8, "batch group: the smaller call (n = 12) completes every member");
  }
  {
    BatchGroup g;
    grow_8_to_16_failing_the_fourth(g);
    const long m0 = H.mallocs, f0 = H.frees;
    check(!g.holds(6) && g.grow(6) == hipSuccess && g.holds(6) && H.mallocs == m0 + 1 && H.frees == f0 && g.acc.cap == 6 * 336 && g.counts.cap == 8 * 336,
          "batch group: a call with n = 6 allocates exactly the emptied member");
  }
  {   // the arena: two new blocks as locals, moved into their holders once both exist
    PgDevBuf<unsigned> codes, mask;
    replace_arena(codes, mask, 64);
    const unsigned *pc = codes.p, *pm = mask.p;
    const long live0 = H.live, f0 = H.frees;
    H.fail_at = 2;
    check(replace_arena(codes, mask, 128) == hipErrorOutOfMemory && H.live == live0 && codes.p == pc && codes.cap == 128 && mask.p == pm && mask.cap == 64,
          "arena whose second allocation failed: the first is freed and the holders are unchanged");
    const long f1 = H.frees;
    check(f1 == f0 + 1 && replace_arena(codes, mask, 128) == hipSuccess && H.live == live0 && H.frees == f1 + 2 && codes.cap == 256 && mask.cap == 128,
          "arena replaced: the old blocks are freed exactly once");
  }
  check(H.live == 0 && H.mallocs == H.frees, "nothing is left of the groups and the arena");
  return wrong;
}
