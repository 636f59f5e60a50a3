// pg_screen.hip — the SCREEN mode on the GPU ("k-mer sketch pre-filter"; definition: pg_screen_core.h).  One call gives the
// n x n matrix of shared sampled k-mers of n genomes without a pair loop: all genomes' (k-mer, genome) keys are sorted once and every k-mer
// held by m genomes adds one to m (m - 1) / 2 cells.  Pairs that share nothing cost nothing.  Integer work over the 2-bit packed genomes
// already resident in HBM; no MFMA.  An ESTIMATE for triage with its own outputs — nothing here touches the exact ANIm / ANIb results or
// the caches of the sketch mode and the ANIm seed lists; every buffer of a call is released before it returns.
//
// One translation unit; its parts live in include files, in this order (kernels and the calls that launch them side by side):
//
// pgscr_front.inc — the front half, shared by the dense calls and the index, and the dense back half:
//   C1 screen_scan_kernel   ALL genomes of the call in one launch: a work item is 256 chunks of 32 start positions of one genome, found
//                           through a prefix table over the genomes; the rolling and validity code is the sketch mode's scan (three code
//                           words, two mask words per lane).  Count pass: the sampled k-mers of the part's bins counted per slice bin in an
//                           LDS histogram, one 64-bit atomic per bin and workgroup into the device histogram.  The host cuts the bins into
//                           contiguous slices of at most max_keys keys.  Fill pass (one per slice): key = canon << 32 | index of the genome
//                           in the call, appended through one cursor, one atomic per wave and position step.
//   C2 sort and group       hipcub radix sort over bits 0 ... 32 + 2 k; hipcub Unique drops a k-mer's second occurrence in one genome;
//                           screen_head_kernel<WIDE> adds the survivors to size[g] (narrow: LDS histogram over the genomes; wide, for the
//                           index: one atomic in HBM each) and marks, among the survivors, the first and the last entry of every k-mer
//                           held by >= 2 genomes; two flagged selections give the groups' first and last entries (the genomes of a group
//                           stand in ascending call index: the index is the low half of the key); screen_weight_kernel<TriWeight> + an
//                           exclusive scan (uint64) give every group its item range and the total P.
//   C3 screen_count_kernel  balanced by ITEM (item_walk, the one body of this balance): a workgroup owns a contiguous range of the P items,
//                           finds its first group by binary search and walks forward 256 items at a time (the window of group offsets it
//                           needs: 257 entries in LDS).  Item t of a group decodes to (i, j), i < j, row-major over the upper triangle
//                           (pgscr::screen_tri_decode), so consecutive lanes run j upward in one matrix row; shared[g_i * n + g_j] += 1 by
//                           a uint32 atomic in HBM — integer adds: the result does not depend on the order of arrival.
//   C4 screen_finish_kernel after the last slice: the upper triangle mirrored, the diagonal = size.
//
// pgscr_select.inc — the SELECTION: pg_screen_hold / pg_screen_load leave an n x n matrix resident on the context
// (ScreenState), and pg_screen_select packs the cells a != b with shared[a][b] >= min(need[a], need[b]) as (a, b, shared[a][b]) in
// row-major order:
//   C5 screen_select_kernel a wave task is SEL_CELLS consecutive cells of one row of a rectangle of rows [r0, r0 + rows), 64 at a time
//                           (coalesced).  Count pass: the popcounts of the task's ballots, one uint64 per task; hipcub exclusive scan; fill
//                           pass: the same ballots again, every kept cell written at its task's offset + the kept cells before it in the
//                           task.  No cursor, no atomic: the order is the order of the cells.  Two streaming passes over the rectangle.
//                           select_rows is its one host side: the dense selection is the rectangle [0, n) of the resident matrix.  The
//                           rows' thresholds are an array of their own and the diagonal test a switch: the square calls pass one array
//                           twice and keep the test, the search (queries x collection) passes two and has no diagonal.
//
// pgscr_index.inc — the INDEX, for collections beyond MAX_GENOMES: C1 and C2 are one front half (screen_front) with two
// back halves.  The dense calls count every grouped slice into the matrix (DenseBack: C3, C4).  pg_screen_index appends the grouped
// entries to a resident compressed-row structure instead (IndexBack: group_start, member; sizes by screen_head_kernel<true>), and
// pg_screen_index_select / _band form the matrix a BAND of rows at a time (band_loop, the one loop over the bands):
//   B1 band_prep_kernel     per group the members inside the band's rows (two binary searches); the groups with none are compacted away
//   B2 screen_weight_kernel<BandWeight> + an exclusive scan: item ranges of the remaining groups, mb m items each
//   B3 band_count_kernel    C3's balance by item (item_walk); item t -> (t / m, t % m), uint32 atomics into the band
//   B4 band_diag_kernel     the cell of a genome with itself = size
//   B5 screen_select_kernel C5 on the band's rectangle (select_rows); the kept triples go to the host as the band finishes
//
// pgscr_search.inc — the SEARCH: new genomes against a resident collection.  pg_screen_search_index is screen_front with
// a third back half (SearchBack: every distinct k-mer with its value, singletons included, in compressed-row form, and a bin -> slice
// directory); pg_screen_search_count runs screen_front over the queries (QueryBack) and counts a q x n rectangle; C5 selects on it:
//   S1 search_lookup_kernel one thread per distinct query k-mer: bin -> slice, binary search over the slice's k-mer values
//   S2 screen_weight_kernel<SearchWeight> + an exclusive scan over the matched k-mers: m_q m_d items each
//   S3 search_count_kernel  C3's balance by item (item_walk); item t -> (t / m_d, t % m_d), uint32 atomics into the rectangle
//
// pgscr_add.inc — genomes ADDED to the resident search index: pg_screen_search_index_add is screen_front over the new
// genomes with a fourth back half (AddBack: the slices' distinct keys staged, the genome rebased behind the collection's) and a merge beside
// the old index; A1 ... A8 stand there:
//   A3 add_locate_kernel    one thread per distinct added k-mer: its position in the index, or where it goes
//   A6 add_fill_old_kernel  the whole index streams through once, balanced by entry (item_walk over the starts)
//
// pgscr_store.inc — the resident search index EXPORTED, IMPORTED and SHRUNK: pg_screen_search_index_export copies the
// arrays out; pg_screen_search_index_import uploads arrays a file supplied and validates every invariant of the build before anything may
// index by them; pg_screen_search_index_remove compacts the index without some columns, beside the old one; V1, V2, R1 ... R5 stand there:
//   V1 store_check_kmer_kernel   one thread per k-mer: the starts strictly increasing up to E; the k-mer sampled, in its bin's slice, ascending
//   V2 store_check_member_kernel only after V1 found the starts sound: item_walk over them; member < n, ascending, the sizes' histogram
//   R4 remove_fill_kernel        member'[pos[t]] = new_of[member[t]]: the second and last read of the old entries
//
// pgscr_gather.inc — the GATHER: a query decomposed into the collection's genomes.  pg_screen_gather_count is the search's
// count with a sink (QueryBack: G0 appends every matched (query, k-mer) entry per slice); pg_screen_gather runs greedy rounds on a copy of
// the rectangle, in batches without a synchronisation between the rounds:
//   G0 gather_expand_kernel item_walk over the matched runs, one item per query holder: entry = query << 48 | index position of the k-mer
//   G1 gather_argmax_kernel a grid over (chunk of the row, query): 16-byte loads, wave and workgroup reduction of the packed key
//                           count << 32 | ~b, one 64-bit atomic max per workgroup into best[query]
//   G2 gather_decide_kernel one thread per query: a row recorded and the winner named, or the query finished; best reset
//   G3 gather_claim_kernel  a wave per 64 entries: the winner looked up among the k-mer's holders (binary search), the claiming lanes
//                           balloted, the whole wave walks each claimed k-mer's holders with uint32 atomic decrements along the row
//
// pgscr_abund.inc — the gather's ABUNDANCES: pg_screen_gather_count_abund is the gather's count over a front half that
// run-length encodes the sorted keys (every entry keeps how many times its query holds the k-mer); pg_screen_gather_abund follows a
// pg_screen_gather and gives every recorded row the statistics of those multiplicities; W1 ... W4 stand there:
//   W2 abund_attribute_kernel a wave per 64 entries: the whole wave walks each live entry's holders for the smallest rank that won
//   W4 abund_stats_kernel     a workgroup per 4096 sorted keys of a row: integer sums by atomics, the squares' carry from the old value
//
// pgscr_components.inc — the COMPONENTS: which genomes belong together.  pg_screen_components (a list from the host) and
// pg_screen_index_components (the bands' kept triples, where B5 left them on the device) hook a union-find forest that only atomics write
// and sum two 64-bit counts per node; K1 ... K3 stand there with their state.
//
// pgscr_representatives.inc — the REPRESENTATIVES: one genome per cluster by the greedy rule.  pg_screen_representatives
// (a list from the host, uploaded whole) and pg_screen_index_representatives (the bands' kept triples with a < b, appended to a device list)
// rank the nodes by score with one radix sort, decide them in rounds of three launches and assign the covered ones by a 64-bit atomic
// maximum; P1 ... P8 stand there with their state.
//
// pgscr_sweep.inc — the SWEEP: the components over a ladder of thresholds in one descending pass.  pg_screen_sweep (a
// list with a level per entry, from the host) and pg_screen_index_sweep (the bands' kept triples, their levels found on the device from the
// resident need table) bucket the entries by level with one stable radix sort, hook bucket after bucket into ONE forest through the body of
// K2 and take a census of it after every bucket; W1 ... W8 stand there with their state.
//
// pgscr_linkage.inc — the LINKAGE: species clusters by average or complete linkage inside every component of a list of
// pairs with distances.  pg_screen_linkage groups the nodes by component (the hook of K2, one stable radix sort), fills the components'
// distance matrices by 64-bit atomic maxima, runs scipy's nearest-neighbour chain — one wave per small component (L8), the heatmap's
// workgroup kernel (pg_cluster_linkage.h) for the others — cuts the trees through a second forest and names one representative per cluster;
// L1 ... L12 stand there with their state.
//
// pgscr_evaluate.inc — the EVALUATION: how good a partition of the kept pairs is.  pg_screen_evaluate (a list from the
// host: one radix sort and one reduce-by-key give the distinct pairs) and pg_screen_index_evaluate (the list the representatives' index
// entry appends) reduce the pairs per node and per cluster — inside sums and minima, the nearest outside node and cluster by 64-bit atomic
// maxima, the medoid in two node passes; E1 ... E7 stand there with their state.
//
// pgscr_profile.inc — the PROFILE: what the genomes of a cluster share.  pg_screen_search_profile reads the resident search
// index under a partition: every (k-mer, cluster) cell with its occupancy is core, soft, shell, private or a marker; the cells are counted per
// cluster with their spectrum, the entries per genome, and the marker cells listed.  The k-mers go three ways by their holders — a thread, a
// wave, or one radix sort of (k-mer, cluster, member) keys in batches — into one accounting body; F1 ... F8 stand there with their state.
#include <algorithm>
#include <hipcub/hipcub.hpp>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "pg_internal.h"
#include "pg_screen_core.h"

namespace {

// the stages whose milliseconds pg_screen_last, pg_screen_index_last, pg_screen_components_last, pg_screen_representatives_last, pg_screen_sweep_last, pg_screen_linkage_last, pg_screen_evaluate_last, pg_screen_search_profile_last, pg_screen_search_last,
// pg_screen_search_add_last, pg_screen_search_remove_last and pg_screen_gather_last report
enum ScreenStage { ST_SCAN, ST_GROUP, ST_COUNT, ST_SELECT, ST_HOOK, ST_FLATTEN, ST_LOOKUP, ST_EXPAND, ST_ARGMAX, ST_CLAIM, ST_MERGE, ST_CHECK, ST_MARK, ST_COMPACT, ST_WEIGHT, ST_ATTRIBUTE, ST_SORT, ST_STATS, ST_ROUNDS, ST_ASSIGN, ST_CENSUS, ST_FILL, ST_SMALL, ST_LARGE, ST_CUT, ST_RELABEL, ST_LANE, ST_WAVE, ST_SORTED, ST_MARKERS };

struct ScreenEvents {      // event pairs on the context's stream, summed per stage after the call's last synchronisation
  std::vector<hipEvent_t> ev;
  std::vector<int> stage;      // of the pair ev[2 i], ev[2 i + 1]
  bool ok = true;
  ~ScreenEvents() { for (auto e : ev) (void)hipEventDestroy(e); }
  // One pair: begun where the object is made, ended where its scope is left, whichever way — the only way to a pair, so none stays open.
  struct Stage {
    ScreenEvents& T;
    hipStream_t s;
    Stage(ScreenEvents& T_, ScreenStage st, hipStream_t s_) : T(T_), s(s_) { if (T.ok) { T.stage.push_back(st); T.mark(s); } }
    ~Stage() { if (T.ok) T.mark(s); }
    Stage(const Stage&) = delete;      // (no assignment either: T is a reference)
  };
  double ms(ScreenStage st) const {      // the milliseconds of every finished pair of the stage
    double sum = 0.0;
    for (size_t i = 0; ok && i < stage.size() && 2 * i + 1 < ev.size(); ++i) {
      float x = 0.f;
      if (stage[i] != st) continue;
      if (hipEventElapsedTime(&x, ev[2 * i], ev[2 * i + 1]) == hipSuccess) sum += (double)x; else (void)hipGetLastError();
    }
    return sum;
  }
 private:
  void mark(hipStream_t s) {
    hipEvent_t e = nullptr;
    if (!ok || hipEventCreate(&e) != hipSuccess) { (void)hipGetLastError(); ok = false; return; }
    ev.push_back(e);
    if (hipEventRecord(e, s) != hipSuccess) { (void)hipGetLastError(); ok = false; }
  }
};

uint32_t grid_for(uint64_t items, uint32_t per_block, uint32_t cap) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + per_block - 1) / per_block, cap));
}

// The temporary storage of the library calls: query(bytes) is the call with a null pointer; tmp_bytes = the largest any of them asked for.
template <typename Query>
hipError_t tmp_room(size_t& tmp_bytes, Query query) {
  size_t need = 0;
  const hipError_t e = query(need);
  tmp_bytes = std::max(tmp_bytes, need);
  return e;
}

}  // namespace

#include "pgscr_front.inc"
#include "pgscr_select.inc"
#include "pgscr_index.inc"
#include "pgscr_components.inc"
#include "pgscr_representatives.inc"
#include "pgscr_sweep.inc"
#include "pgscr_linkage.inc"
#include "pgscr_evaluate.inc"
#include "pgscr_search.inc"
#include "pgscr_add.inc"
#include "pgscr_store.inc"
#include "pgscr_gather.inc"
#include "pgscr_abund.inc"
#include "pgscr_profile.inc"
