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
  return wrong;
}
