// pg_internal.h — shared declarations of libpyani_gpu.so (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <array>
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "pyani_gpu.h"
#include "pg_devbuf.h"

// ---- HBM layout of the genome store -------------------------------------------------------------------------
// One "base stream" per genome: its records back to back with ONE dirty separator base between records, then
// dirty padding up to a multiple of PG_SUPER bases (always at least one dirty base at the end).  Streams of all
// genomes are laid out in one arena:
//   codes : 2 bits/base, base s of the arena in bits [2*(s%16), +2) of codes32[s/16]   (A=0 C=1 G=2 T=3, dirty=0)
//   mask  : 1 bit/base,  bit (s%32) of mask32[s/32] = 1 iff the base is one of ACGT ("clean")
// A k-mer window is valid iff all its k mask bits are 1; separators and padding make windows that would cross a
// record or genome boundary invalid for free, so the count kernel needs no record table.
constexpr uint32_t PG_SUPER = 65536;          // bases per super-tile = one block iteration (1024 lanes x 64 bases)
constexpr uint32_t PG_ACC_WORDS = 16 + 64 + 256;  // per-genome accumulator: E2 | E3 | F4 (unsigned long long each)

struct PgGenome {
  uint64_t total_len = 0;    // sum of record lengths (pyani_files.get_sequence_lengths)
  uint32_t n_rec = 0;
  uint64_t stream_len = 0;   // total_len + (n_rec-1) separators
  uint64_t padded_len = 0;   // multiple of PG_SUPER, > stream_len
  uint64_t arena_start = 0;  // base offset in the device arena (multiple of PG_SUPER)
  bool resident = false;
  std::vector<uint32_t> codes, mask;  // host copy until uploaded
  std::array<uint32_t, 256> quirk{};  // tetramers the reference does not count (last window of each strand)
  std::vector<int32_t> rec_start;     // stream position of each record's first base; [n_rec] = stream_len + 1
};

struct PgEventPair {
  hipEvent_t a, b;
  int which;
};

// What the latest screen calls did (pg_screen.hip): counts, and milliseconds between HIP events on the context's stream.  Only the four
// entry points pg_screen_last, pg_screen_index_last, pg_screen_components_last and pg_screen_search_last know the order of these in the C ABI's arrays.
struct PgScreenStats {
  uint64_t keys = 0, distinct = 0, groups = 0, pair_increments = 0, slices = 0;      // sampled keys, distinct entries, groups of >= 2 genomes
  double scan_ms = 0.0, group_ms = 0.0, count_ms = 0.0;                              // scan, sort + group, count
};
struct PgScreenIndexStats {
  uint64_t keys = 0, distinct = 0, entries = 0, groups = 0, slices = 0;      // the build: entries = the grouped ones the index keeps
  uint64_t bands = 0, pair_increments = 0;                                   // the latest selection: bands worked, increments of its count kernel
  double scan_ms = 0.0, group_ms = 0.0;                                      // the build
  double count_ms = 0.0, select_ms = 0.0;                                    // the latest selection
};
struct PgScreenComponentsStats {
  uint64_t nodes = 0, worked = 0, ignored = 0, components = 0;      // entries worked, entries ignored (a == b)
  double select_ms = 0.0, hook_ms = 0.0, flatten_ms = 0.0;          // band count + select (index path), hook + accumulate, flatten
};

struct PgScreenRepresentativesStats {      // pg_screen_representatives_last: the resident representatives' call
  uint64_t nodes = 0, worked = 0, ignored = 0, representatives = 0, rounds = 0, launches = 0;      // launches: of the round kernels
  double select_ms = 0.0, sort_ms = 0.0, rounds_ms = 0.0, assign_ms = 0.0;                          // band count + select (index path), rank sort, rounds, assign
};

struct PgScreenSweepStats {      // pg_screen_sweep_last: the resident sweep's call
  uint64_t nodes = 0, steps = 0, worked = 0, ignored = 0, level0 = 0, buckets = 0;      // worked: entries with a != b; level0: those of them present at no step; buckets: non-empty
  double select_ms = 0.0, sort_ms = 0.0, hook_ms = 0.0, census_ms = 0.0;                // band count + select + levels (index path), histogram + sort, hook + accumulate, census
};

struct PgScreenLinkageStats {      // pg_screen_linkage_last: the resident linkage's call
  uint64_t nodes = 0, worked = 0, ignored = 0, components = 0, worked_components = 0, largest = 0, clusters = 0, batches = 0;      // worked_components: those of >= 2 nodes
  double group_ms = 0.0, fill_ms = 0.0, small_ms = 0.0, large_ms = 0.0, cut_ms = 0.0;      // group, fill, wave linkage, workgroup linkage, cut + representatives
};

struct PgScreenEvaluateStats {      // pg_screen_evaluate_last: the resident evaluation's call
  uint64_t nodes = 0, worked = 0, ignored = 0, pairs = 0, inside = 0, clusters = 0;      // pairs: distinct; inside: those with both ends in one cluster
  double select_ms = 0.0, sort_ms = 0.0, pair_ms = 0.0, node_ms = 0.0;                    // band count + select (index path), canonicalise + sort + reduce, pair passes, node passes
};

struct PgScreenProfileStats {      // pg_screen_search_profile_last: the resident profile's call
  uint64_t nodes = 0, clusters = 0, kmers = 0, entries = 0, cells = 0;                     // n, clusters, D, E of the index, cells counted
  uint64_t lane_kmers = 0, wave_kmers = 0, sorted_kmers = 0, batches = 0, markers = 0;     // k-mers per tier, batches of the sorted tier, markers listed
  double relabel_ms = 0.0, lane_ms = 0.0, wave_ms = 0.0, sorted_ms = 0.0, marker_ms = 0.0;
};

struct PgScreenSearchStats {
  uint64_t keys = 0, kmers = 0, entries = 0, slices = 0, index_bytes = 0;                // the search index: sampled keys, distinct k-mers, (k-mer, genome) entries, device bytes its buffers hold
  uint64_t query_keys = 0, lookups = 0, matched = 0, increments = 0, query_slices = 0;   // the latest count: lookups = the distinct k-mers of the queries
  double index_scan_ms = 0.0, index_group_ms = 0.0;                                      // the build
  double scan_ms = 0.0, group_ms = 0.0, lookup_ms = 0.0, count_ms = 0.0;                 // the latest count
  double select_ms = 0.0;                                                                // the latest selection
};

struct PgScreenSearchRemoveStats {      // pg_screen_search_remove_last: the latest accepted pg_screen_search_index_remove
  uint64_t genomes = 0, entries = 0, kmers = 0;      // removed columns, entries, k-mers (those whose last holder went)
  uint64_t removes = 0;                              // accepted removes since the build or the import
  double mark_ms = 0.0, compact_ms = 0.0;            // the two scans; placement, the copy of the entries, the directory
};

struct PgScreenSearchAddStats {      // pg_screen_search_add_last: the latest accepted pg_screen_search_index_add
  uint64_t genomes = 0, keys = 0, entries = 0, new_kmers = 0, matched_kmers = 0;      // of the batch: k-mers absent from / present in the index before
  uint64_t adds = 0;                                                                   // accepted adds since the build
  double scan_ms = 0.0, group_ms = 0.0, merge_ms = 0.0;
};

struct PgScreenGatherStats {      // pg_screen_gather_last: the latest pg_screen_gather_count (entries, expand) and pg_screen_gather (the rest)
  uint64_t entries = 0, rounds = 0, rows = 0, claimed = 0, decrements = 0;
  double expand_ms = 0.0, argmax_ms = 0.0, claim_ms = 0.0;      // argmax_ms: arg-max + decide
};

struct PgScreenGatherAbundStats {      // pg_screen_gather_abund_last: the latest pg_screen_gather_count_abund (weight) and pg_screen_gather_abund (the rest)
  uint64_t attributed = 0, unattributed = 0, walked = 0, rank_bytes = 0;      // entries that belong to a row | to none; holders walked; bytes of the rank table
  double weight_ms = 0.0, attribute_ms = 0.0, sort_ms = 0.0, stats_ms = 0.0;
};

struct pg_ctx {
  ~pg_ctx();   // destroys the streams (pg_api.cpp); the buffers below free themselves
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  std::mutex mu;
  std::vector<PgGenome> genomes;
  uint64_t arena_used = 0;  // bases
  // device arena
  PgDevBuf<uint32_t> d_codes, d_mask;
  uint64_t arena_cap = 0;  // bases both arena blocks hold, excluding the trailing guard super-tile (written once both exist)
  PgDevBuf<uint32_t> d_quirk;   // genomes x 256
  uint32_t n_resident = 0;
  // batch scratch (device): grown as a group by ensure_batch_scratch, every member tested by its own size
  std::vector<int32_t> batch_ids;  // ids of the cached work list
  PgDevBuf<uint32_t> d_seg_tile0;    // batch: first arena super-tile of each genome
  PgDevBuf<uint32_t> d_seg_prefix;   // batch + 1: cumulative super-tile counts
  PgDevBuf<uint32_t> d_batch_gid;
  uint32_t n_work = 0;
  PgDevBuf<unsigned long long> d_acc;      // batch x PG_ACC_WORDS (zero between passes)
  PgDevBuf<unsigned long long> d_counts;   // batch x (16+64+256): c2 | c3 | c4
  PgDevBuf<double> d_dev;                  // batch x 256 compacted deviations
  PgDevBuf<double> d_ss;                   // batch
  PgDevBuf<unsigned long long> d_keybits;  // batch x 4: bitmap of observed tetramers
  // One result block per pass so that ONE device-to-host copy returns everything:
  //   [ flags: 4 x int32 ] [ z: n x 256 f64 ] [ corr: n x n f64 ] [ present: n x 256 u8 ]
  PgDevBuf<uint8_t> d_result;
  PgPinnedBuf<uint8_t> h_result;
  // views into d_result, not owned: set by every ensure_result, null after a failed one
  int32_t* d_flags = nullptr;   // [0]=keyset mismatch, [1]=n present keys
  double* d_z = nullptr;
  double* d_corr = nullptr;
  uint8_t* d_present = nullptr;
  PgPinnedBuf<unsigned long long> h_counts;   // batch x PG_ACC_WORDS
  // profiling
  bool profiling = false;
  uint32_t prof_mask = 0xFFFFFFFFu, prof_every = 1;
  uint64_t prof_seen[PG_K__END] = {};
  std::vector<PgEventPair> events;
  double prof_ms[PG_K__END] = {};
  uint64_t prof_n[PG_K__END] = {};
  int num_cu = 256;
  void* anim_scratch = nullptr;  // AnimScratch (pg_anim.hip) of worker 0, grows on demand
  // ANIm / fragment-mode calls are split over two host workers, each with its own stream and scratch: while one worker's
  // launch is in a low-occupancy tail (one wave per unit, slowest unit = launch time) the other's kernels fill the GPU
  // result of the latest pg_anim_alignments_batch (caller's pair order)
  std::vector<pg_anim_alignment> aln_store;
  std::vector<uint64_t> aln_indel_off;
  std::vector<int64_t> aln_indels;
  // result of the latest pg_anib_rows_batch (caller's pair order); anib_rows_valid: there has been one
  std::vector<pg_anib_row> anib_rows_store;
  bool anib_rows_valid = false;
  static constexpr int MAX_WORKERS = 4;
  void* anim_scratch_w[MAX_WORKERS] = {nullptr, nullptr, nullptr, nullptr};   // workers 1.. (index 0 unused: worker 0 = anim_scratch)
  hipStream_t stream_w[MAX_WORKERS] = {nullptr, nullptr, nullptr, nullptr};   // workers 1.. (index 0 unused: worker 0 = stream)
  void* anim_lists = nullptr;      // per-genome seed lists, shared by the workers (guarded by anim_mu)
  void* sketch_store = nullptr;    // per-genome k-mer sketches of the sketch mode (pg_sketch.hip), built on first use
  void* classify_state = nullptr;  // resident edge state of the classify sweep (pg_classify.hip), replaced by every pg_classify_edges
  void* dist_state = nullptr;      // resident values of the distribution calls (pg_dist.hip), replaced by every pg_dist_load
  void* screen_state = nullptr;    // resident matrix of the screen's selection (pg_screen.hip), replaced by every pg_screen_hold / pg_screen_load
  uint64_t screen_max_keys = 0;          // pg_screen_set_budget: keys of one slice of a screen call (0: the default, pg_screen_core.h)
  PgScreenStats screen_stats;            // pg_screen_last: the latest pg_screen_matrix / pg_screen_hold
  void* screen_index_state = nullptr;    // resident k-mer index of pg_screen_index and its latest selection (pg_screen.hip); independent of screen_state
  uint32_t screen_band_rows = 0;         // pg_screen_set_band: matrix rows of one band of the index calls (0: the default, pg_screen_core.h)
  PgScreenIndexStats screen_index_stats; // pg_screen_index_last: the latest pg_screen_index and the latest selection over it
  void* screen_components_state = nullptr;      // resident components of the latest pg_screen_components / pg_screen_index_components (pg_screen.hip); independent of both above
  PgScreenComponentsStats screen_components_stats;      // pg_screen_components_last: the resident components' call
  void* screen_representatives_state = nullptr;      // resident representatives of the latest pg_screen_representatives / pg_screen_index_representatives (pg_screen.hip); independent of the three above
  PgScreenRepresentativesStats screen_representatives_stats;      // pg_screen_representatives_last: the resident representatives' call
  void* screen_sweep_state = nullptr;      // resident sweep of the latest pg_screen_sweep / pg_screen_index_sweep (pg_screen.hip); independent of the four above
  PgScreenSweepStats screen_sweep_stats;      // pg_screen_sweep_last: the resident sweep's call
  void* screen_linkage_state = nullptr;      // resident linkage of the latest pg_screen_linkage (pg_screen.hip); independent of the five above
  PgScreenLinkageStats screen_linkage_stats;      // pg_screen_linkage_last: the resident linkage's call
  uint32_t screen_linkage_small = 0xFFFFFFFFu;      // pg_screen_linkage_set: components up to here go one per wave (PG_SCREEN_LINKAGE_DEFAULT: the default, pgscr_linkage.inc)
  uint64_t screen_linkage_work = 0;                 // ... and the bytes of working matrices of one batch (0: the default)
  void* screen_evaluate_state = nullptr;      // resident evaluation of the latest pg_screen_evaluate / pg_screen_index_evaluate (pg_screen.hip); independent of the six above
  PgScreenEvaluateStats screen_evaluate_stats;      // pg_screen_evaluate_last: the resident evaluation's call
  void* screen_profile_state = nullptr;      // resident profile of the latest pg_screen_search_profile (pg_screen.hip); independent of the seven above and of the genome store
  PgScreenProfileStats screen_profile_stats;      // pg_screen_search_profile_last: the resident profile's call
  uint32_t screen_profile_lane = 0xFFFFFFFFu, screen_profile_wave = 0xFFFFFFFFu;      // pg_screen_search_profile_set: the tiers' limits (PG_SCREEN_PROFILE_DEFAULT: the defaults, pgscr_profile.inc)
  uint64_t screen_profile_batch = 0;                                                  // ... and the entries of one sorted batch (0: the budget of pg_screen_set_budget)
  void* screen_search_state = nullptr;          // resident search index of pg_screen_search_index and the latest rectangle counted against it (pg_screen.hip); independent of the three above and of the genome store
  PgScreenGatherStats screen_gather_stats;      // pg_screen_gather_last
  PgScreenGatherAbundStats screen_gather_abund_stats;      // pg_screen_gather_abund_last
  PgScreenSearchAddStats screen_search_add_stats;      // pg_screen_search_add_last
  PgScreenSearchRemoveStats screen_search_remove_stats;      // pg_screen_search_remove_last
  PgScreenSearchStats screen_search_stats;      // pg_screen_search_last: the resident search index, the latest count and selection over it
  double dist_ms[3] = {0.0, 0.0, 0.0};   // kernel milliseconds of the latest pg_dist_load / _hist / _kde while profiling is on (pg_dist_last_ms)
  uint32_t tree_tail_limit = 512;        // pg_tree_nj_set: from this many live nodes down one workgroup runs every remaining step (pg_tree.hip)
  uint64_t tree_counts[5] = {0, 0, 0, 0, 0};   // pg_tree_nj_last: n, wide steps, tail steps, launches, cells scanned of the latest pg_tree_nj
  double tree_ms[3] = {0.0, 0.0, 0.0};   // ... and its validate, wide-step and tail milliseconds while profiling is on
  std::mutex anim_mu, err_mu, prof_mu;
  int anib_word_tier = 1;      // fragment mode: search failed fragments again with blastn-sized (11-mer) seeds
  uint32_t anib_search = 0;    // fragment mode: PG_ANIB_SEARCH_SEEDS, or PG_ANIB_SEARCH_ALL_DIAGS (pg_anib_set_search)
  int anim_pn_window_max = 2048;   // forced runs: the widest single-wave window (development: smaller values push runs on to the group kernel)
  int anim_pn_group_max = 8184;    // ... and the widest band the group of four waves takes (development: 0 = everything beyond one wave on the strips)
  int anim_gap_lanes = 1;      // postnuc: small match-to-match gaps on one lane each (0: all gaps on the wave engine; tests compare the two)
  int anim_bwd_ahead = 1;      // backward searches ahead of the units' walks (pga_postnuc.inc); PYANI_ANIM_BWD_AHEAD=0 (development switch): inside them       // PG_EXTENDER_NUCMER (pg_anim_set_extender)
  int anim_workers = 2;
  // pg_anim_pairs_enqueue / _fetch: two lanes, lane L drives worker slots 2 L and 2 L + 1
  struct AnimAsync {
    std::thread th;
    std::vector<int32_t> r, q;
    std::vector<pg_anim_result> out;
    uint64_t ticket = 0;
    int rc = 0;
    bool busy = false;
  } anim_async[2];
  uint64_t anim_next_ticket = 1;
  std::mutex anim_async_mu;
  uint32_t anim_batch_pairs = 131072;         // ordered pairs in flight (split over the two workers: 65536 per launch; every launch pays its slowest unit once)
  uint64_t anim_scratch_matches_held = 0;     // match slots the workers' scratch already holds (counts as available to anim_match_budget)
  uint64_t anim_batch_matches = 512ull << 20; // exact matches in flight (~384 B of scratch each, grown on demand: at most ~136 GB of the 288 GB)
};

int pg_fail(pg_ctx* ctx, int code, const std::string& msg);
#define PG_HIP(ctx, call)                                                                                     \
  do {                                                                                                        \
    hipError_t _e = (call);                                                                                   \
    if (_e != hipSuccess)                                                                                     \
      return pg_fail((ctx), PG_E_HIP, std::string(#call) + ": " + hipGetErrorString(_e));                     \
  } while (0)
// the same with the caller's message prefix in place of the call's text
#define PG_HIP_MSG(ctx, prefix, call)                                                                         \
  do {                                                                                                        \
    hipError_t _e = (call);                                                                                   \
    if (_e != hipSuccess) return pg_fail((ctx), PG_E_HIP, std::string(prefix) + hipGetErrorString(_e));       \
  } while (0)

// `count` (at least 1) elements for a buffer of one of the modes; a refusal is PG_E_NOMEM, "<mode>: no device memory for <what>"
template <typename T>
int pg_dev_alloc(pg_ctx* ctx, const char* mode, PgDevBuf<T>& b, size_t count, const char* what) {
  if (b.reserve(count ? count : 1) == hipSuccess) return PG_OK;
  (void)hipGetLastError();
  return pg_fail(ctx, PG_E_NOMEM, std::string(mode) + ": no device memory for " + what);
}

// profiling helpers (pg_api.cpp).  Events are recorded on the calling thread's stream: pg_tls_stream when set (the ANIm
// workers), else the context's.
extern thread_local hipStream_t pg_tls_stream;
void pg_prof_begin(pg_ctx* ctx, int which);
void pg_prof_end(pg_ctx* ctx);

// kernels' host launchers (pg_tetra.hip)
int pg_launch_tetra_count(pg_ctx* ctx, uint32_t n_batch);
int pg_launch_tetra_finalize(pg_ctx* ctx, uint32_t n_batch, unsigned long long* d_acc_in);
int pg_launch_tetra_stats(pg_ctx* ctx, const double* d_z, const uint8_t* d_present, uint32_t n);
int pg_launch_tetra_pairs(pg_ctx* ctx, uint32_t n, uint32_t row0, uint32_t nrows, double* d_out, bool mirror);

// ANIm (pg_anim.hip): all pairs sharing one reference genome
int pg_anim_reduce_run(pg_ctx* ctx, uint32_t n_pairs, const uint64_t* offsets, const int32_t* rseq, const int32_t* qseq,
                       const int32_t* rs, const int32_t* re, const int32_t* qs, const int32_t* qe, const int32_t* errors,
                       int apply_filter, pg_anim_result* out);
// frag != nullptr: fragment mode (ANIb) — ref_ids are the subject genomes, qry_ids the fragmented ones; the batch stops after
// the seeding stage and runs the fragment kernels instead of clustering / extension
struct PgFragArgs {
  int32_t fragsize;
  pg_anib_result* out;        // n_pairs results (host)
  pg_anib_row* rows_out;      // optional: the rows of pair 0 (host), at most rows_cap; *n_rows_out = how many there are
  uint32_t rows_cap;
  uint32_t* n_rows_out;
  uint64_t max_slots;         // (pair, fragment) slots per launch
  struct PgRowSink* sink = nullptr;   // optional: the rows of EVERY pair of the launch, packed on the device (pg_anib_rows_batch)
  uint32_t search = 0;        // PG_ANIB_SEARCH_*: the context's setting as the call found it at entry
};
// Where a fragment-mode launch leaves its tables when PgFragArgs::sink is set: the rows of its pairs back to back in launch order
// (fragments in order, a fragment's rows best score first), and how many each pair owns.  One sink per launch chain: the caller's.
struct PgRowSink {
  std::vector<pg_anib_row> rows;
  std::vector<uint32_t> pair_count;
};
int pg_anim_run_batch(pg_ctx* ctx, const int32_t* ref_ids, const int32_t* qry_ids, uint32_t n_pairs, int filter_1to1, int maxmatch,
                      uint64_t max_matches, pg_anim_result* out_host, uint32_t* n_done,
                      const PgFragArgs* frag = nullptr);   // ref_ids grouped (equal ids adjacent)
void pg_anim_set_worker(pg_ctx* ctx, int worker);   // binds the calling thread to worker 0 .. MAX_WORKERS-1 (stream + scratch) for run_batch
void pg_anim_free_scratch(pg_ctx* ctx);
void pg_anim_release_worker_scratch(pg_ctx* ctx);   // launch scratch of every worker slot (seed lists stay); idle context only
int pg_anim_fetch_alignments(pg_ctx* ctx, int32_t ref_id, int32_t qry_id, uint32_t n, pg_anim_alignment* out);   // after a 1-pair batch
// Where pg_anim_run_batch leaves the alignment records of its pairs when the calling thread has set one (pg_anim_alignments_batch):
// appended pair after pair in the order of the call's arrays; with_indels adds the traceback pass and every alignment's .delta list.
// Development knobs (launch shapes, alternative code paths that must give the same results, counters): environment variables
// honoured ONLY under PYANI_DEV_KNOBS=1 — the test suite sets it — so that a stray variable in a production environment cannot
// change what the library launches.
inline const char* pg_dev_env(const char* name) {
  const char* on = getenv("PYANI_DEV_KNOBS");
  return on && on[0] == '1' ? getenv(name) : nullptr;
}
constexpr uint32_t PG_FRAG_MAX_FRAGS = 15872;      // fragments per query genome in fragment mode (pga_frag.inc: LDS counters)
struct PgAlnSink {
  bool with_indels = false;
  std::vector<pg_anim_alignment> alns;
  std::vector<uint32_t> pair_count;               // alignments of each pair, in arrival order
  std::vector<std::vector<int64_t>> indels;       // parallel to alns (with_indels)
};
int pg_anim_counters_read(pg_ctx* ctx, uint64_t* out /*[64]*/, int reset);
// development (pg_anim_forced_rects): n checked rectangles (A0, A1, B0, B1) of one (reference, query strand) through the forced launches
int pg_anim_forced_rects_run(pg_ctx* ctx, int32_t ref_id, int32_t qry_id, int strand, uint32_t n, const int32_t* rects, int32_t* errors,
                             int32_t* w_used, int32_t* status);
// development (pg_anim_searches): n checked trimmed searches (A0, B0, tA, tB, m_o) of one (reference, query strand) on the engine asked for
int pg_anim_searches_run(pg_ctx* ctx, int32_t ref_id, int32_t qry_id, int strand, int engine, uint32_t n, const int32_t* searches, int32_t* out);
void pg_anim_set_sink(PgAlnSink* sink);           // thread-local; nullptr = none
void pg_anim_drop_lists(pg_ctx* ctx);   // per-genome seed lists: must go when the genome store is cleared
void pg_sketch_drop(pg_ctx* ctx);       // ... and the sketches of the sketch mode (pg_sketch.hip)
void pg_classify_drop(pg_ctx* ctx);     // ... the classify sweep's edge state (pg_classify.hip): goes with the context or on request
void pg_dist_drop(pg_ctx* ctx);         // ... the distribution calls' resident values (pg_dist.hip): the same
void pg_screen_drop(pg_ctx* ctx);       // ... the screen's resident matrix and selection (pg_screen.hip): the same, and with the genome store
void pg_screen_components_drop(pg_ctx* ctx); // ... the screen's resident components (pg_screen.hip): with the context, the genome store or on request
void pg_screen_representatives_drop(pg_ctx* ctx); // ... the screen's resident representatives (pg_screen.hip): the same
void pg_screen_sweep_drop(pg_ctx* ctx); // ... the screen's resident sweep (pg_screen.hip): the same
void pg_screen_linkage_drop(pg_ctx* ctx); // ... the screen's resident linkage (pg_screen.hip): the same
void pg_screen_evaluate_drop(pg_ctx* ctx); // ... the screen's resident evaluation (pg_screen.hip): the same
void pg_screen_profile_drop(pg_ctx* ctx); // ... the screen's resident profile (pg_screen.hip): with the context or on request — NOT with the genome store, as the search index
void pg_screen_index_drop(pg_ctx* ctx); // ... the screen's resident k-mer index and its selection (pg_screen.hip): with the context, the genome store or on request
void pg_screen_search_drop(pg_ctx* ctx); // ... the screen's resident search index and rectangle (pg_screen.hip): with the context or on request — NOT with the genome store: it names genomes by call index only
int pg_anib_reduce_run(pg_ctx* ctx, uint32_t n_pairs, const uint64_t* offsets, const uint32_t* n_frags, const int32_t* frag,
                       const int32_t* length, const int32_t* mismatch, const int32_t* gaps, const int32_t* qlen,
                       const double* pident, int64_t* aln_out, int64_t* err_out, double* pid_out);

// Device memory for a sketch (pg_sketch.hip) or a screen call (pg_screen.hip).  The ANIm engine keeps its per-launch scratch and per-genome seed lists for reuse (after a 1000-genome
// grid: ~200 GB of the 288); a sketch that does not fit beside them takes their place — they are rebuilt on the next ANIm call.
template <typename T>
int sk_malloc(pg_ctx* ctx, PgDevBuf<T>& b, size_t n) {      // an empty buffer gets n elements
  // (PYANI_SKETCH_ALLOC_FAIL under PYANI_DEV_KNOBS=1: every first attempt counts as failed, so that a test can walk the fallback)
  static const bool fail_first = pg_dev_env("PYANI_SKETCH_ALLOC_FAIL") != nullptr;
  if (!fail_first && b.reserve(n) == hipSuccess) return PG_OK;
  (void)hipGetLastError();
  // The ANIm launch scratch takes the sketches' place — only on an IDLE context: never under an enqueued ANIm call (its thread is using
  // that scratch), and only after everything the worker streams were given has finished.
  {
    std::lock_guard<std::mutex> lk(ctx->anim_async_mu);
    if (ctx->anim_async[0].busy || ctx->anim_async[1].busy)
      return pg_fail(ctx, PG_E_NOMEM, "sketch: device memory is short and enqueued ANIm calls are in flight (fetch them first: their launch scratch cannot be released under them)");
  }
  PG_HIP(ctx, hipDeviceSynchronize());
  pg_anim_free_scratch(ctx);
  pg_screen_drop(ctx);      // an idle resident matrix of the screen's selection goes too (no call of its own allocates through here while it reads one)
  PG_HIP_MSG(ctx, "sketch: no device memory, the ANIm scratch released: ", b.reserve(n));
  return PG_OK;
}
