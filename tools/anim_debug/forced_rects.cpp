// forced_rects.cpp — HOST statement of directed forced rectangles (tests/forced_cases.py): for every rectangle of every case the
// plain-integer referee (forced_referee.h), pgn::ScalarEngine (the definition the GPU engines follow cell for cell) and
// pgd::DiagWaveEngine (the host emulation of the GPU's diagonal-window wave engines), with the certified-band loop's LADDER logged:
// the band of every pass, -1 for the whole rectangle.  The loop is restated here around the engines' public run() so that it can
// log; on rectangles of up to 4 million cells each engine's own align() runs too and must agree with the restated loop, or the line says so.
// stdin:   <number of cases>, then per case:  <name> <strand 0|1> <number of rectangles>  /  <reference sequence>  /  <query sequence>
//          /  one line "A0 A1 B0 B1" per rectangle (stream positions, ends inclusive, B in strand coordinates)
// stdout:  one line per rectangle:
//   <name> <k> ref <score> <errors> <lowest prefix> scalar <status> <errors> <passes> <w ...> diag <status> <errors> <passes> <w ...> loops <ok 0|1> alt <errors under MATCH > DELETE > INSERT | -1> <under DELETE > INSERT > MATCH | -1>
//   status 0 = certified, 2 = the corner stayed unreachable (the engine's overflow: PG_E_CAPACITY on the pair).
//   g++ -O2 -std=c++17 -pthread -Ipyani_amd/csrc -Itools/anim_debug tools/anim_debug/forced_rects.cpp
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <thread>
#include <vector>
#include "pg_nucmer_diag.h"
#include "forced_referee.h"
using namespace pga;

struct Packed {      // a stream as the library packs it: 2-bit codes, clean bit only for A, C, G, T
  std::vector<uint32_t> codes, mask;
  int64_t len;
  explicit Packed(const std::string& s) : codes(s.size() / 16 + 2, 0), mask(s.size() / 32 + 2, 0), len((int64_t)s.size()) {
    for (size_t p = 0; p < s.size(); ++p) {
      if (!forced_referee::is_acgt(s[p])) continue;
      const int c = s[p] == 'A' ? 0 : s[p] == 'C' ? 1 : s[p] == 'G' ? 2 : 3;
      codes[p >> 4] |= (uint32_t)c << (2 * (p & 15));
      mask[p >> 5] |= 1u << (p & 31);
    }
  }
  SeqView view() const { return SeqView{codes.data(), mask.data(), len}; }
};

struct Case { std::string name, a, b; int strand; std::vector<int32_t> rects; };
struct Run { int status = 0, errors = 0; std::vector<int32_t> ladder; };

// the band loop of ScalarEngine::align / DiagWaveEngine::align around run(), with the band logged
template <typename RUN>
static Run band_loop(RUN&& run, int32_t A0, int32_t A1, int32_t B0, int32_t B1) {
  Run r;
  const int32_t N = A1 - A0 + 1, M = B1 - B0 + 1;
  for (int32_t w = pgn::FORCED_BAND_FIRST;;) {
    int32_t a = A1, b = B1, score = 0, err = 0;
    const bool whole = w >= (N > M ? N : M);
    r.ladder.push_back(whole ? -1 : w);
    const bool reached = run(A0, a, B0, b, whole ? -1 : w, err, score);
    const int v = pgn::forced_verdict(reached, score, whole, N, M, w);
    if (v == 2) { r.status = 2; r.errors = 0; return r; }
    if (v == 0) { r.status = 0; r.errors = err; return r; }
    w = pgn::forced_band_after(w, N, M, score);
  }
}

int main() {
  size_t n_cases = 0;
  std::cin >> n_cases;
  std::vector<Case> cases(n_cases);
  struct Job { size_t c, k; };
  std::vector<Job> jobs;
  for (Case& c : cases) {
    size_t nr = 0;
    std::cin >> c.name >> c.strand >> nr >> c.a >> c.b;
    c.rects.resize(4 * nr);
    for (int32_t& v : c.rects) std::cin >> v;
    for (size_t k = 0; k < nr; ++k) jobs.push_back(Job{(size_t)(&c - cases.data()), k});
  }
  if (!std::cin) { fprintf(stderr, "forced_rects: malformed input\n"); return 2; }
  auto area = [&](const Job& j) { const int32_t* r = &cases[j.c].rects[4 * j.k]; return (int64_t)(r[1] - r[0] + 1) * (r[3] - r[2] + 1); };
  std::stable_sort(jobs.begin(), jobs.end(), [&](const Job& x, const Job& y) { return area(x) > area(y); });      // the large rectangles first
  // a rectangle's three parts — the referee, the scalar engine, the wave emulation — are jobs of their own: the largest rectangles
  // would otherwise hold one thread for all three
  struct Out { long long ref_score = 0, ref_min = 0; int ref_err = 0, alt_err[2] = {-1, -1}; Run rs, rd; bool ok_s = true, ok_d = true; };
  std::vector<Out> outs(jobs.size());
  std::atomic<size_t> next{0};
  std::atomic<int> bad{0};
  auto worker = [&]() {
    const int cap = 1 << 14;
    std::vector<pgn::Cell> d0(cap), d1(cap), d2(cap);
    for (;;) {
      const size_t t = next.fetch_add(1);
      if (t >= 3 * jobs.size()) break;
      const size_t ji = t / 3;
      const int part = (int)(t % 3);
      Out& O = outs[ji];
      const Case& c = cases[jobs[ji].c];
      const int32_t A0 = c.rects[4 * jobs[ji].k], A1 = c.rects[4 * jobs[ji].k + 1], B0 = c.rects[4 * jobs[ji].k + 2], B1 = c.rects[4 * jobs[ji].k + 3];
      if (A0 < 0 || A1 < A0 || A1 >= (int32_t)c.a.size() || B0 < 0 || B1 < B0 || B1 >= (int32_t)c.b.size()) { ++bad; continue; }
      const int64_t area = (int64_t)(A1 - A0 + 1) * (B1 - B0 + 1);
      if (part == 0) {
        // the referee reads plain strings: the reverse strand is the complement-and-reverse of the query
        const std::string as = c.a.substr(A0, A1 - A0 + 1), bs = (c.strand ? forced_referee::reverse_complement(c.b) : c.b).substr(B0, B1 - B0 + 1);
        forced_referee::reference(as, bs, O.ref_score, O.ref_err, O.ref_min);
        // on rectangles of up to a million cells also the counts under two OTHER tie orders (MATCH > DELETE > INSERT; DELETE > INSERT >
        // MATCH): equal counts mean the rectangle cannot tell the orders apart (-1: not computed)
        if (area <= (1ll << 20))
          for (int o = 1; o <= 2; ++o) { long long s2 = 0, m2 = 0; forced_referee::reference(as, bs, s2, O.alt_err[o - 1], m2, o); }
        continue;
      }
      // the engines read the packed streams, the query through its strand view
      const Packed PA(c.a), PB(c.b);
      const SeqView R = PA.view();
      const StrandView Q{PB.view(), c.strand};
      const bool small = area <= (4ll << 20);
      if (part == 1) {
        pgn::ScalarEngine<SeqView, StrandView> eng{R, Q, d0.data(), d1.data(), d2.data(), cap};
        O.rs = band_loop([&](int32_t a0, int32_t& a, int32_t b0, int32_t& b, int32_t bw, int32_t& err, int32_t& score) {
          return eng.run(a0, a, b0, b, pgn::FORCED_FORWARD_ALIGN, bw, err, &score); }, A0, A1, B0, B1);
        O.ok_s = !eng.overflow;
        pgn::ScalarEngine<SeqView, StrandView> own{R, Q, d0.data(), d1.data(), d2.data(), cap};
        int32_t a = A1, b = B1, err = -1;
        const bool reached = small ? own.align(A0, a, B0, b, pgn::FORCED_FORWARD_ALIGN, err) : false;
        O.ok_s = O.ok_s && (!small || (O.rs.status == 2 ? (own.overflow && !reached) : (!own.overflow && reached && err == O.rs.errors && a == A1 && b == B1)));
      } else {
        pgd::DiagWaveEngine<SeqView, StrandView> eng(R, Q, d0.data(), d1.data(), d2.data(), cap);
        O.rd = band_loop([&](int32_t a0, int32_t& a, int32_t b0, int32_t& b, int32_t bw, int32_t& err, int32_t& score) {
          return eng.run(a0, a, b0, b, pgn::FORCED_FORWARD_ALIGN, bw, err, score); }, A0, A1, B0, B1);
        O.ok_d = !eng.slow.overflow;
        pgd::DiagWaveEngine<SeqView, StrandView> own(R, Q, d0.data(), d1.data(), d2.data(), cap);
        int32_t a = A1, b = B1, err = -1;
        const bool reached = small ? own.align(A0, a, B0, b, pgn::FORCED_FORWARD_ALIGN, err) : false;
        O.ok_d = O.ok_d && (!small || (O.rd.status == 2 ? (own.slow.overflow && !reached) : (!own.slow.overflow && reached && err == O.rd.errors && a == A1 && b == B1)));
      }
    }
  };
  unsigned nt = std::thread::hardware_concurrency();
  if (nt == 0) nt = 1;
  if (nt > 16) nt = 16;
  if (nt > 3 * jobs.size()) nt = jobs.empty() ? 1 : (unsigned)(3 * jobs.size());
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; ++t) th.emplace_back(worker);
  for (auto& t : th) t.join();
  if (bad) { fprintf(stderr, "forced_rects: a rectangle outside its sequences\n"); return 2; }
  for (size_t ji = 0; ji < jobs.size(); ++ji) {
    const Out& O = outs[ji];
    std::ostringstream o;
    o << cases[jobs[ji].c].name << ' ' << jobs[ji].k << " ref " << O.ref_score << ' ' << O.ref_err << ' ' << O.ref_min;
    o << " scalar " << O.rs.status << ' ' << O.rs.errors << ' ' << O.rs.ladder.size();
    for (int32_t w : O.rs.ladder) o << ' ' << w;
    o << " diag " << O.rd.status << ' ' << O.rd.errors << ' ' << O.rd.ladder.size();
    for (int32_t w : O.rd.ladder) o << ' ' << w;
    o << " loops " << (O.ok_s && O.ok_d ? 1 : 0) << " alt " << O.alt_err[0] << ' ' << O.alt_err[1] << '\n';
    fputs(o.str().c_str(), stdout);
  }
  return 0;
}
