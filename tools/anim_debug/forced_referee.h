// forced_referee.h — the plain-integer referee of a FORCED alignment (MUMmer's sw_align with FORCED_FORWARD_ALIGN): the optimal
// global path of the whole rectangle a[0 .. N) x b[0 .. M), int64 scores, MUMmer's tie order MATCH > INSERT > DELETE on the state
// of origin, the error count riding along the chosen path.  Nothing of the engines is in here: no packed words, no band, no score
// floor, no packed streams — two character strings in, three numbers out.  tools/anim_debug/forced_check.cpp and forced_rects.cpp
// hold the engines against it.
//
// Bases: a column is a MATCH only if both characters are one of A, C, G, T and equal.  Every other column of two bases — an N, any
// other letter, on either side, also when both sides hold the same such letter — is a mismatch: BAD score and one error.  (The
// engines read packed streams in which such a base is "not clean"; a cell with an unclean base never counts as a match.)
// The reverse strand of a sequence is its plain complement-and-reverse: A <-> T, C <-> G, every other character stays what it is.
#pragma once
#include <string>
#include <vector>

namespace forced_referee {

inline bool is_acgt(char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
inline std::string reverse_complement(const std::string& s) {
  std::string r(s.rbegin(), s.rend());
  for (char& c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c;
  return r;
}

// sw_align's forced (global, untrimmed) alignment of a[0 .. N) with b[0 .. M) on plain integers: score and errors of the corner,
// and the lowest score along the chosen path (what tells whether the engines' score floor can matter)
// order: 0 = MUMmer's (MATCH > INSERT > DELETE).  The others are NOT MUMmer's — 1 = MATCH > DELETE > INSERT, 2 = the reverse, DELETE >
// INSERT > MATCH — and only there to show that a case's error count depends on the order at all (a rectangle on which the orders
// count the same cannot tell an engine with a wrong preference from a right one).
// One cell: per state (0 = DELETE: a B base alone, from the left; 1 = INSERT: an A base alone, from above; 2 = MATCH column) the
// score, the errors and the lowest score along the chosen path.  A state no path reaches has score NEG (and stays there: the
// prices are tiny beside it).
const long long NEG = -(1ll << 50);
struct Cell { long long s[3], p[3]; int e[3]; };
inline void reference(const std::string& a, const std::string& b, long long& score, int& errors, long long& prefix_min, int order = 0) {
  const int N = (int)a.size(), M = (int)b.size();
  const int rank[3] = {order == 0 ? 0 : order == 1 ? 1 : 2, order == 0 ? 1 : order == 1 ? 0 : 1, order == 2 ? 0 : 2};
  int asc[3] = {0, 1, 2};      // the states by ascending rank: a later one wins a tie (MUMmer: MATCH > INSERT > DELETE, on the state of origin)
  for (int x = 0; x < 3; ++x) for (int y = x + 1; y < 3; ++y) if (rank[asc[y]] < rank[asc[x]]) { const int t = asc[x]; asc[x] = asc[y]; asc[y] = t; }
  auto best = [&asc](const long long v[3]) { int w = asc[0]; if (v[asc[1]] >= v[w]) w = asc[1]; if (v[asc[2]] >= v[w]) w = asc[2]; return w; };
  const Cell dead{{NEG, NEG, NEG}, {0, 0, 0}, {0, 0, 0}};
  std::vector<Cell> prev(M + 1, dead), cur(M + 1, dead);
  for (int i = 0; i <= N; ++i) {
    for (int j = 0; j <= M; ++j) {
      Cell c = dead;
      if (i == 0 && j == 0) c.s[2] = 0;
      else {
        if (j >= 1) {      // DELETE from the left cell's states: a gap goes on for -7, opens for -10
          const Cell& L = cur[j - 1];
          const long long v[3] = {L.s[0] - 7, L.s[1] - 10, L.s[2] - 10};
          const int w = best(v);
          if (v[w] > NEG / 2) { c.s[0] = v[w]; c.e[0] = L.e[w] + 1; c.p[0] = L.p[w] < v[w] ? L.p[w] : v[w]; }
        }
        if (i >= 1) {      // INSERT from the cell above
          const Cell& U = prev[j];
          const long long v[3] = {U.s[0] - 10, U.s[1] - 7, U.s[2] - 10};
          const int w = best(v);
          if (v[w] > NEG / 2) { c.s[1] = v[w]; c.e[1] = U.e[w] + 1; c.p[1] = U.p[w] < v[w] ? U.p[w] : v[w]; }
        }
        if (i >= 1 && j >= 1) {      // MATCH column from the best state of the diagonal cell: +3 on a match, -7 and one error otherwise
          const Cell& G = prev[j - 1];
          const int w = best(G.s);
          if (G.s[w] > NEG / 2) {
            const bool same = is_acgt(a[i - 1]) && a[i - 1] == b[j - 1];
            c.s[2] = G.s[w] + (same ? 3 : -7); c.e[2] = G.e[w] + (same ? 0 : 1); c.p[2] = G.p[w] < c.s[2] ? G.p[w] : c.s[2];
          }
        }
      }
      cur[j] = c;
    }
    prev.swap(cur);
  }
  const Cell& C = prev[M];
  const int w = best(C.s);
  score = C.s[w]; errors = C.e[w]; prefix_min = C.p[w];
}

}  // namespace forced_referee
