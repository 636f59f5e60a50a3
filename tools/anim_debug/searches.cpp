// searches.cpp — HOST statement of directed TRIMMED searches (tests/search_cases.py): for every search of every case
// pgn::ScalarEngine::run (MUMmer's own band: trimmed 600 below the best score, broken 200 anti-diagonals after it — the definition the
// GPU engines follow cell for cell) and the host emulation of the GPU's diagonal-window wave engine on the 256- and the 512-diagonal
// window (pgd::DiagWaveEmu<4> / <8>), with what the emulation did: whether the window held the band (fit), how often the window
// moved and which way, the widest anti-diagonal.  For rectangles with both sides <= 59 (the one-gap-per-lane kernels' class) also
// the error count of the plain UNTRIMMED global alignment (forced_referee.h: plain integers, nothing of the engines) — the lane
// kernels rest on the proof that such a rectangle cannot be trimmed and cannot break; -1 where not computed.
// stdin:   <number of cases>, then per case:  <name> <strand 0|1> <number of searches>  /  <reference sequence>  /  <query sequence as
//          stored>  /  one line "A0 B0 tA tB m_o" per search (stream positions, B in strand coordinates; m_o = 1, 9, 2 or 10:
//          FORWARD_ALIGN, BACKWARD_SEARCH, with or without OPTIMAL_BIT)
// stdout:  one line per search:
//   <name> <k> scalar <endA> <endB> <errors> <score> <reached> <wmax> e4 <fit> <endA> <endB> <errors> <score> <reached> <moves> <moves towards
//   lower diagonals> <moves towards higher diagonals> <wmax> e8 <the same ten> global <errors | -1>
//   (an emulation whose window did not hold the band: fit 0, the results 0, the moves those made before it gave up)
//   g++ -O2 -std=c++17 -pthread -Ipyani_amd/csrc -Itools/anim_debug tools/anim_debug/searches.cpp -o tools/anim_debug/searches
#include <atomic>
#include <cstdio>
#include <iostream>
#include <memory>
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

struct Case { std::string name, a, b; int strand; std::vector<int32_t> s; std::unique_ptr<Packed> pa, pb; };
struct EmuOut { int fit = 0; int32_t a = 0, b = 0, err = 0, score = 0; int reached = 0; long moves = 0, down = 0, up = 0; unsigned wmax = 0; };
struct Out { int32_t a = 0, b = 0, err = 0, score = 0; int reached = 0; unsigned wmax = 0; EmuOut e4, e8; int global_err = -1; };

template <int DPL>
static EmuOut emulate(const SeqView& R, const StrandView& Q, int32_t A0, int32_t B0, int32_t tA, int32_t tB, unsigned m_o) {
  std::unique_ptr<pgd::DiagWaveEmu<DPL, SeqView, StrandView>> emu(new pgd::DiagWaveEmu<DPL, SeqView, StrandView>{R, Q});
  EmuOut o;
  int32_t a = tA, b = tB, err = 0, score = 0;
  bool reached = false;
  o.fit = emu->run(A0, a, B0, b, m_o, -1, err, score, reached) ? 1 : 0;
  if (o.fit) { o.a = a; o.b = b; o.err = err; o.score = score; o.reached = reached ? 1 : 0; o.wmax = emu->last_wmax; }
  o.moves = emu->moves; o.down = emu->moves_down; o.up = emu->moves_up;
  return o;
}

int main() {
  size_t n_cases = 0;
  std::cin >> n_cases;
  std::vector<Case> cases(n_cases);
  struct Job { size_t c, k; };
  std::vector<Job> jobs;
  for (Case& c : cases) {
    size_t ns = 0;
    std::cin >> c.name >> c.strand >> ns >> c.a >> c.b;
    c.s.resize(5 * ns);
    for (int32_t& v : c.s) std::cin >> v;
    for (size_t k = 0; k < ns; ++k) jobs.push_back(Job{(size_t)(&c - cases.data()), k});
    c.pa = std::make_unique<Packed>(c.a);
    c.pb = std::make_unique<Packed>(c.b);
  }
  if (!std::cin) { fprintf(stderr, "searches: malformed input\n"); return 2; }
  std::vector<Out> outs(jobs.size());
  std::atomic<size_t> next{0};
  std::atomic<int> bad{0};
  auto worker = [&]() {
    const int cap = 1 << 14;
    std::vector<pgn::Cell> d0(cap), d1(cap), d2(cap);
    for (;;) {
      const size_t t = next.fetch_add(1);
      if (t >= jobs.size()) break;
      const Case& c = cases[jobs[t].c];
      const int32_t* s = &c.s[5 * jobs[t].k];
      const int32_t A0 = s[0], B0 = s[1], tA = s[2], tB = s[3];
      const unsigned m_o = (unsigned)s[4];
      const bool fwd = m_o & pgn::DIRECTION_BIT;
      const int64_t N = fwd ? (int64_t)tA - A0 + 1 : (int64_t)A0 - tA + 1, M = fwd ? (int64_t)tB - B0 + 1 : (int64_t)B0 - tB + 1;
      const bool mode_ok = m_o == pgn::FORWARD_ALIGN || m_o == (pgn::FORWARD_ALIGN | pgn::OPTIMAL_BIT) || m_o == pgn::BACKWARD_SEARCH || m_o == (pgn::BACKWARD_SEARCH | pgn::OPTIMAL_BIT);
      if (!mode_ok || N < 1 || M < 1 || N > pgn::MAX_ALIGNMENT_LENGTH || M > pgn::MAX_ALIGNMENT_LENGTH || A0 < 0 || tA < 0 || B0 < 0 || tB < 0 ||
          A0 >= (int32_t)c.a.size() || tA >= (int32_t)c.a.size() || B0 >= (int32_t)c.b.size() || tB >= (int32_t)c.b.size()) { ++bad; continue; }
      const SeqView R = c.pa->view();
      const StrandView Q{c.pb->view(), c.strand};
      Out& O = outs[t];
      pgn::ScalarEngine<SeqView, StrandView> eng{R, Q, d0.data(), d1.data(), d2.data(), cap};
      int32_t a = tA, b = tB, err = 0, score = 0;
      O.reached = eng.run(A0, a, B0, b, m_o, -1, err, &score) ? 1 : 0;
      if (eng.overflow) { ++bad; continue; }
      O.a = a; O.b = b; O.err = err; O.score = score; O.wmax = eng.last_wmax;
      O.e4 = emulate<4>(R, Q, A0, B0, tA, tB, m_o);
      O.e8 = emulate<8>(R, Q, A0, B0, tA, tB, m_o);
      if (fwd && N <= 59 && M <= 59) {      // the plain global alignment of the rectangle, both boundary bases included
        const std::string as = c.a.substr(A0, (size_t)N), bs = (c.strand ? forced_referee::reverse_complement(c.b) : c.b).substr(B0, (size_t)M);
        long long sc = 0, mn = 0;
        forced_referee::reference(as, bs, sc, O.global_err, mn);
      }
    }
  };
  unsigned nt = std::thread::hardware_concurrency();
  if (nt == 0) nt = 1;
  if (nt > 16) nt = 16;
  if (nt > jobs.size()) nt = jobs.empty() ? 1 : (unsigned)jobs.size();
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; ++t) th.emplace_back(worker);
  for (auto& t : th) t.join();
  if (bad) { fprintf(stderr, "searches: a search outside its sequences, beyond the engines' limits, or in a mode that is no search\n"); return 2; }
  for (size_t ji = 0; ji < jobs.size(); ++ji) {
    const Out& O = outs[ji];
    std::ostringstream o;
    o << cases[jobs[ji].c].name << ' ' << jobs[ji].k << " scalar " << O.a << ' ' << O.b << ' ' << O.err << ' ' << O.score << ' ' << O.reached << ' ' << O.wmax;
    for (const EmuOut* e : {&O.e4, &O.e8})
      o << (e == &O.e4 ? " e4 " : " e8 ") << e->fit << ' ' << e->a << ' ' << e->b << ' ' << e->err << ' ' << e->score << ' ' << e->reached << ' ' << e->moves << ' '
        << e->down << ' ' << e->up << ' ' << e->wmax;
    o << " global " << O.global_err << '\n';
    fputs(o.str().c_str(), stdout);
  }
  return 0;
}
