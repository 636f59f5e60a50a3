// pg_anib_rows.h — host bookkeeping of pg_anib_rows_batch (pg_api.cpp): where the packed rows of the call's launches are kept while
// the launches run, and how they get back into the caller's pair order.  Depends on the C ABI header and the standard library only
// (tests/anib_rows/rows_merge_check.cpp compiles it on its own).
#pragma once
#include <cstdint>
#include <cstring>
#include <deque>
#include <mutex>
#include <vector>

#include "pyani_gpu.h"

// Every launch's packed rows are one part (a part never moves once stored: the deque only grows at its end and the vectors are
// moved in), and for every pair of the CALL it is recorded where its rows lie.  Workers file disjoint pairs; only the part list is
// shared.
struct PgAnibRowParts {
  std::mutex mu;
  std::deque<std::vector<pg_anib_row>> parts;
  std::vector<const pg_anib_row*> first;   // per pair of the call (null: no rows)
  std::vector<uint32_t> count;

  explicit PgAnibRowParts(uint64_t n_pairs) : first(n_pairs, nullptr), count(n_pairs, 0) {}

  // One launch: `rows` holds the tables of its n pairs back to back, pair k of the launch (pair_of[k] of the call) owns
  // pair_count[k] of them.  False when the counts do not add up to the rows.
  bool file(std::vector<pg_anib_row>&& rows, const uint32_t* pair_count, const uint64_t* pair_of, uint64_t n) {
    uint64_t total = 0;
    for (uint64_t k = 0; k < n; ++k) total += pair_count[k];
    if (total != rows.size()) return false;
    const pg_anib_row* at;
    {
      std::lock_guard<std::mutex> lk(mu);
      parts.push_back(std::move(rows));
      at = parts.back().data();
    }
    for (uint64_t k = 0; k < n; ++k) {
      first[pair_of[k]] = pair_count[k] ? at : nullptr;
      count[pair_of[k]] = pair_count[k];
      at += pair_count[k];
    }
    return true;
  }

  // After the last launch: row_offsets[n_pairs + 1] and the rows in the caller's pair order.
  void assemble(uint64_t* row_offsets, std::vector<pg_anib_row>& out) const {
    const uint64_t n = count.size();
    row_offsets[0] = 0;
    for (uint64_t i = 0; i < n; ++i) row_offsets[i + 1] = row_offsets[i] + count[i];
    out.resize(row_offsets[n]);
    for (uint64_t i = 0; i < n; ++i)
      if (count[i]) std::memcpy(out.data() + row_offsets[i], first[i], (size_t)count[i] * sizeof(pg_anib_row));
  }
};
