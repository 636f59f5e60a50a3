// forced_check.cpp — HOST unit check of the forced-run band loop on rectangles whose OPTIMAL path dips far below zero (DESIGN §4,
// deviation (3): "scores below the floor of the packed words saturate to unreachable").  MUMmer's sw_align works on plain long
// ints; the engine's state words hold 15 bits of score with a bias (pg_nucmer_core.h, SCORE_BIAS).  Such rectangles cannot come out
// of a walk (a backward search breaks 200 anti-diagonals after its last best cell, so no forced rectangle spans 200 mismatches in
// a row), hence no genome pair reaches this through the C ABI: the check drives the engines directly — pgn::ScalarEngine (the
// definition the GPU engines follow cell for cell, and what anim_trace_kernel runs) and pgd::DiagWaveEngine (the host emulation
// of the GPU's diagonal-window wave engines, same header the kernels compile).
// The referee is the plain-integer statement of sw_align's forced alignment in forced_referee.h (whole rectangle, int64 scores,
// MUMmer's tie order MATCH > INSERT > DELETE on the state of origin, errors riding along): no packed words, no band, no floor.
//   case A  20 matching bases, 700 unrelated ones, 1200 matching: the optimal path's prefix falls to about -1 650 before it recovers
//           (rounds 3-4, floor -1024: its cells saturated and the run came back with another path's error count)
//   case B  20 matching, 1500 unrelated, 2500 matching: the prefix minimum lies below the floor (-2700) on EVERY path to the corner:
//           the run must FAIL LOUDLY (engine overflow -> PG_E_CAPACITY on the pair), not return the count of an unreachable word
//   case C  1500 bases with 30 scattered mismatches: an ordinary rectangle
// Prints one line per case and engine; exit code 0 iff all are as stated.   g++ -O2 -std=c++17 -pthread -Ipyani_amd/csrc -Itools/anim_debug forced_check.cpp
#include <cstdio>
#include <string>
#include <thread>
#include <vector>
#include "pg_nucmer_diag.h"
#include "forced_referee.h"
using namespace pga;
using forced_referee::reference;

struct Packed {
  std::vector<uint32_t> codes, mask;
  int64_t len;
  explicit Packed(const std::string& s) : codes(s.size() / 16 + 2, 0), mask(s.size() / 32 + 2, 0), len((int64_t)s.size()) {
    for (size_t p = 0; p < s.size(); ++p) {
      const int c = s[p] == 'A' ? 0 : s[p] == 'C' ? 1 : s[p] == 'G' ? 2 : 3;
      codes[p >> 4] |= (uint32_t)c << (2 * (p & 15));
      mask[p >> 5] |= 1u << (p & 31);
    }
  }
  SeqView view() const { return SeqView{codes.data(), mask.data(), len}; }
};

static uint64_t rng_state = 12345;
static int rnd4() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (int)((rng_state >> 33) & 3); }

// a / b: equal where `same`, a fixed substitution elsewhere; a's bases never repeat the neighbour's, so that a shifted diagonal
// (a gap) does not line up by chance more than random
static void build(const std::vector<int>& runs, std::string& a, std::string& b) {      // runs: +n = n matching bases, -n = n mismatching ones
  const char* B = "ACGT";
  for (int r : runs)
    for (int i = 0; i < (r < 0 ? -r : r); ++i) {
      const int c = rnd4();
      a.push_back(B[c]);
      b.push_back(r < 0 ? B[(c + 1 + rnd4() % 3) & 3] : B[c]);
    }
}

int main() {
  struct Case { const char* name; std::vector<int> runs; int want_errors; bool want_fail; };
  std::vector<int> scattered;
  for (int i = 0; i < 30; ++i) { scattered.push_back(49); scattered.push_back(-1); }
  Case cases[] = {{"A deep dip", {20, -700, 1200}, 0, false}, {"B below floor", {20, -1500, 2500}, 0, true}, {"C ordinary", scattered, 0, false}};
  int bad = 0;
  // the cases are independent and the emulated window engines are slow (64 lanes in software): one thread per case
  std::string report[3];
  int bad_of[3] = {0, 0, 0};
  auto run_case = [&](int ci) {
    Case& c = cases[ci];
    char line[512];
    std::string a, b;
    build(c.runs, a, b);
    long long ref_score, ref_min; int ref_err;
    // (the engine's rectangle includes the base pair the path already stands on: cell (1, 1) = a[0] / b[0])
    reference(a, b, ref_score, ref_err, ref_min);
    c.want_errors = ref_err;
    snprintf(line, sizeof line, "%-14s plain-integer statement: score %lld, errors %d, lowest prefix of the optimal path %lld\n", c.name, ref_score, ref_err, ref_min);
    report[ci] += line;
    if (c.want_fail ? ref_min >= -(long long)pgn::SCORE_BIAS : (ref_min < -(long long)pgn::SCORE_BIAS || (c.name[0] == 'A' && ref_min > -1100))) { report[ci] += "  the case is not what it claims to be\n"; ++bad_of[ci]; }
    const Packed PA(a), PB(b);
    const SeqView R = PA.view();
    const StrandView Q{PB.view(), 0};
    const int cap = 1 << 14;
    std::vector<pgn::Cell> d0(cap), d1(cap), d2(cap);
    for (int which = 0; which < 2; ++which) {
      int32_t A1 = (int32_t)a.size() - 1, B1 = (int32_t)b.size() - 1, err = -1;
      bool reached, overflow;
      if (which == 0) {
        pgn::ScalarEngine<SeqView, StrandView> eng{R, Q, d0.data(), d1.data(), d2.data(), cap};
        reached = eng.align(0, A1, 0, B1, pgn::FORCED_FORWARD_ALIGN, err);
        overflow = eng.overflow != 0;
      } else {
        pgd::DiagWaveEngine<SeqView, StrandView> eng(R, Q, d0.data(), d1.data(), d2.data(), cap);
        reached = eng.align(0, A1, 0, B1, pgn::FORCED_FORWARD_ALIGN, err);
        overflow = eng.slow.overflow != 0;
      }
      const bool ok = c.want_fail ? (overflow && !reached) : (!overflow && reached && err == c.want_errors && A1 == (int32_t)a.size() - 1 && B1 == (int32_t)b.size() - 1);
      snprintf(line, sizeof line, "%-14s %-16s reached %d overflow %d errors %d (want %s%d) %s\n", c.name, which ? "DiagWaveEngine" : "ScalarEngine", (int)reached, (int)overflow, err,
               c.want_fail ? "failure, not " : "", c.want_errors, ok ? "ok" : "WRONG");
      report[ci] += line;
      bad_of[ci] += !ok;
    }
  };
  {
    std::thread t0(run_case, 0), t1(run_case, 1), t2(run_case, 2);
    t0.join(); t1.join(); t2.join();
  }
  for (int ci = 0; ci < 3; ++ci) { fputs(report[ci].c_str(), stdout); bad += bad_of[ci]; }
  return bad ? 1 : 0;
}
