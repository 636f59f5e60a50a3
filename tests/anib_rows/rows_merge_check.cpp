// Host check of PgAnibRowParts (pyani_amd/csrc/pg_anib_rows.h): launches file their packed rows in any order and from several
// threads, assemble() gives the caller's order.  Prints one line per check, "ok <name>" or "WRONG <name>", and returns the number of
// wrong ones.  Built with the address and undefined-behaviour sanitizers by tests/test_anib_rows_cpu.py.
#include <cstdio>
#include <thread>
#include "pg_anib_rows.h"

static int wrong = 0;
static void check(bool ok, const char* name) {
  std::printf("%s %s\n", ok ? "ok" : "WRONG", name);
  if (!ok) ++wrong;
}

// pair p of the call owns rows_of(p) rows, row t of it carries frag = t and score = p
static uint32_t rows_of(uint64_t p) { return (uint32_t)((p * 7 + 3) % 5 == 0 ? 0 : (p * 7 + 3) % 5 + (p % 3)); }
static std::vector<pg_anib_row> launch_rows(const std::vector<uint64_t>& pairs, std::vector<uint32_t>& counts) {
  std::vector<pg_anib_row> rows;
  counts.clear();
  for (uint64_t p : pairs) {
    counts.push_back(rows_of(p));
    for (uint32_t t = 0; t < rows_of(p); ++t) { pg_anib_row r{}; r.frag = (int32_t)t; r.score = (int32_t)p; rows.push_back(r); }
  }
  return rows;
}
static bool in_caller_order(const PgAnibRowParts& P, uint64_t n) {
  std::vector<uint64_t> off(n + 1, 99);
  std::vector<pg_anib_row> out;
  P.assemble(off.data(), out);
  bool ok = off[0] == 0 && off[n] == out.size();
  for (uint64_t p = 0; p < n && ok; ++p) {
    ok = off[p + 1] - off[p] == rows_of(p);
    for (uint64_t t = off[p]; t < off[p + 1] && ok; ++t) ok = out[t].score == (int32_t)p && out[t].frag == (int32_t)(t - off[p]);
  }
  return ok;
}

int main() {
  {   // launches over shuffled, interleaved pairs, filed in an order that is not the call's
    const uint64_t n = 23;
    PgAnibRowParts P(n);
    const std::vector<std::vector<uint64_t>> launches = {{22, 3, 9}, {}, {0}, {21, 20, 1, 2, 4}, {5, 19, 6, 18, 7, 17, 8, 16}, {10, 15, 11, 14, 12, 13}};
    bool filed = true;
    for (const auto& L : launches) {
      std::vector<uint32_t> c;
      auto rows = launch_rows(L, c);
      filed = filed && P.file(std::move(rows), c.data(), L.data(), L.size());
    }
    check(filed, "every launch is filed");
    check(in_caller_order(P, n), "assemble gives the caller's order, 0-row pairs and an empty launch included");
  }
  {   // no pair at all; a call whose pairs were never launched (all PG_E_CAPACITY)
    PgAnibRowParts none(0);
    uint64_t off0[1] = {7};
    std::vector<pg_anib_row> out(3);
    none.assemble(off0, out);
    check(off0[0] == 0 && out.empty(), "no pairs: one offset, no rows");
    PgAnibRowParts idle(4);
    uint64_t off4[5];
    idle.assemble(off4, out);
    check(off4[4] == 0 && out.empty(), "pairs that were never launched own no rows");
  }
  {   // counts that do not add up to the rows are refused and change nothing
    PgAnibRowParts P(2);
    std::vector<pg_anib_row> rows(3);
    const uint32_t c[2] = {1, 1};
    const uint64_t of[2] = {0, 1};
    check(!P.file(std::move(rows), c, of, 2) && P.parts.empty() && P.count[0] == 0, "a launch whose counts do not match its rows is refused");
  }
  {   // two workers filing disjoint pairs at once
    const uint64_t n = 4000;
    PgAnibRowParts P(n);
    bool ok[2] = {true, true};
    auto worker = [&](int w) {
      for (uint64_t base = (uint64_t)w * 40; base < n; base += 80) {
        std::vector<uint64_t> L;
        for (uint64_t p = base; p < base + 40 && p < n; ++p) L.push_back(p);
        std::vector<uint32_t> c;
        auto rows = launch_rows(L, c);
        ok[w] = ok[w] && P.file(std::move(rows), c.data(), L.data(), L.size());
      }
    };
    std::thread other(worker, 1);
    worker(0);
    other.join();
    check(ok[0] && ok[1] && in_caller_order(P, n), "two workers file at once");
  }
  return wrong;
}
