// pg_anim.hip — gfx950 kernels of the ANIm engine (kernel family 3 of BASELINE.json's north star): replaces the
// `nucmer --mum` + `delta-filter -1` processes pyani shells out to (pyani/anim.py:240-289) and the parse_delta
// reduction (anim.py:292-411) with an in-process pipeline over the 2-bit/1-bit packed genomes already resident in HBM.
//
//   A1 anim_list_kernel      per genome, once: its 16-mers as (k-mer, position) lists partitioned into 16384 hash groups
//                            (every position for the reference role, every 5th strand position for the query role)
//   A2 anim_seed_kernel      one workgroup per (block of up to 32 references, group): the group's k-mers of every reference
//                            of the block become ONE hash table in LDS; the same group of every query of the block streams
//                            through it once (coalesced, sequential HBM reads).  Fragment mode: anim_seed_pair_kernel, one
//                            workgroup per (reference, coarse group of 8 groups) and every query of that reference
//   A3 anim_cluster_wave_kernel  one WAVE per (pair, strand): MUM filter (packed radix sorts + wave-scan containment
//                            flags), mgaps clustering (lock-free union-find), chain extraction (register / LDS resident)
//   A4x the extension stage  MUMmer's own postnuc / sw_align (pga_postnuc.inc, pga_postnuc_diag.inc; statement pg_nucmer_core.h,
//                            pg_nucmer_diag.h): match-to-match gaps, forward extensions and backward searches as pre-passes
//                            (one wave or one lane per call), the units' sequential cluster walks, the forced re-alignments
//                            as certified bands on diagonal-window engines of 128 ... 8192 diagonals
//   A5 anim_finish_kernel    one wave per pair: 1-to-1 filter (delta-filter -1), parse_delta reduction -> pg_anim_result
//
// The kernels live in include files, in pipeline order: pga_seed.inc (A1/A2), pga_cluster.inc (A3), pga_postnuc.inc +
// pga_postnuc_diag.inc (A4x), pga_finish.inc (A5), pga_frag.inc (fragment mode); this file holds the shared descriptors and
// the host driver.  (The fixed-band "banded64" extender of rounds 1-2 was retired in round 5: it was not exact.)
// Host driver: a worker's device scratch is an AnimScratch of owning buffers (PgDevBuf, pg_devbuf.h: each knows its size, the
// scratch is freed by deleting it); pg_anim_run_batch is a sequence of stage functions over one Batch struct, in launch order.
//
// Every kernel has a scalar statement in pg_anim_core.h that compiles for the host (tools/anim_debug); the two are kept
// in lock-step and compared on the GPU by tests/test_anim_gpu.py.  Limits: a reference k-mer group of n entries is seeded in
// ceil(n / 8192) passes through a 16384-slot LDS table (pg_seed_plan.h: one pass for fine groups up to ~130 Mb, for the fragment
// mode's coarse groups up to ~16 Mb; more beyond, same results); a reference of 2^30 - 1 or more bases is refused by the block
// kernel's table (30 position bits, PG_E_CAPACITY); chain scores < 2^24.
#include <tuple>
#include <unordered_map>
#include "pg_internal.h"
#include "pg_devbuf.h"
#include "pg_seed_plan.h"
#include "pg_anim_core.h"
#include "pg_nucmer_core.h"
#include "pg_nucmer_diag.h"
#include "pg_anib_core.h"
#include "pg_anim_trace.h"

using namespace pga;

namespace {

constexpr unsigned long long SLOT_EMPTY = ~0ull;
constexpr int FRAG_SEED_MIN = 16;   // fragment mode keeps every sampled 16-mer hit (SEED_K)

struct RefDesc {
  const uint32_t* codes;
  const uint32_t* mask;
  int32_t len;
  const int32_t* rec_start;  // n_rec + 1 entries
  int32_t n_rec;
};

struct UnitDesc {   // one (pair, query strand)
  const uint32_t* codes;
  const uint32_t* mask;
  int32_t len;
  const int32_t* rec_start;
  int32_t n_rec;
  int32_t strand;
  int32_t pair;  // index into the batch's pair list
  int32_t ref;   // index into the batch's reference list
};

// 16 bases starting at stream position p (p + 16 <= len): codes in 32 bits (first base low), clean bits in 16
__device__ __forceinline__ void get16(const uint32_t* __restrict__ codes, const uint32_t* __restrict__ mask, int32_t p,
                                      uint32_t& c, uint32_t& m) {
  const uint32_t cw = p >> 4, cs = 2 * (p & 15);
  const uint64_t lo = (uint64_t)codes[cw] | ((uint64_t)codes[cw + 1] << 32);
  c = (uint32_t)(lo >> cs);
  const uint32_t mw = p >> 5, ms = p & 31;
  const uint64_t ml = (uint64_t)mask[mw] | ((uint64_t)mask[mw + 1] << 32);
  m = (uint32_t)(ml >> ms) & 0xFFFFu;
}

// 2-bit codes / clean bits of the n <= 32 stream positions p0 .. p0 + n - 1 of a packed genome (positions outside are not clean)
__device__ __forceinline__ void packed_window(const uint32_t* __restrict__ codes, const uint32_t* __restrict__ mask, int32_t len, int64_t p0,
                                              uint64_t& c, uint32_t& ok) {
  c = 0; ok = 0;
  if (p0 >= len || p0 + 32 <= 0) return;
  const int64_t q0 = p0 < 0 ? 0 : p0;                 // first position actually read
  const int sh = (int)(q0 - p0);                      // it lands at window slot sh
  const int32_t w = (int32_t)(q0 >> 4), lastw = (len - 1) >> 4;
  const uint32_t c0 = codes[w], c1 = codes[w + 1 <= lastw ? w + 1 : lastw], c2 = codes[w + 2 <= lastw ? w + 2 : lastw];
  const int cs = 2 * (int)(q0 & 15);
  uint64_t lo = ((uint64_t)c1 << 32) | c0;
  uint64_t win = cs ? ((lo >> cs) | ((uint64_t)c2 << (64 - cs))) : lo;
  const int32_t mw = (int32_t)(q0 >> 5), lastm = (len - 1) >> 5;
  const uint64_t m = ((uint64_t)mask[mw + 1 <= lastm ? mw + 1 : lastm] << 32) | mask[mw];
  uint32_t okw = (uint32_t)(m >> (q0 & 31));
  const int64_t avail = len - q0;                      // positions from q0 that exist
  if (avail < 32) okw &= (avail <= 0 ? 0u : ((1u << avail) - 1u));
  c = sh ? (win << (2 * sh)) : win;
  ok = sh ? (okw << sh) : okw;
}

#include "pga_seed.inc"
#include "pga_cluster.inc"
#include "pga_postnuc.inc"
#include "pga_finish.inc"
#include "pga_frag.inc"

}  // namespace

// ---- host driver ---------------------------------------------------------------------------------------------------
// One batch of ordered pairs (any mix of references): ref_ids[i] = nucmer's reference (pyani's query genome, anim.py:280).
// Scratch lives in the context and only grows.  The per-unit kernels are latency-bound single-thread code, so the
// batch should be as large as memory allows: thousands of units in flight are what fills the GPU.
namespace {
// per-genome seed lists (built once per resident genome and role, dropped by pg_clear_genomes); shared by the two workers of a
// context: built under ctx->anim_mu and complete (stream synchronised) before the lock is released
struct GenomeIdx {
  uint64_t *ref_list = nullptr, *qry_list = nullptr, *qry_list1 = nullptr;   // qry_list1: every position (fragment mode)
  uint32_t *ref_goff = nullptr, *qry_goff = nullptr, *qry_goff1 = nullptr;
  uint32_t ref_max = 0;        // largest coarse reference group (sizes the per-pair kernel's LDS table)
  uint32_t ref_max_fine = 0;   // largest reference group (the block kernel's table holds one per slot)
  uint32_t* word_start = nullptr;   // fragment mode, word tier: 4^11 + 1 bucket offsets of the genome's 11-mers ...
  int32_t* word_pos = nullptr;      // ... and their positions
};
// gidx holds views (a batch works on a copy of them); the memory behind them is `blocks`, which goes all at once (pg_anim_drop_lists)
// or, for the blocks of a call that failed, at that call's end
struct AnimLists {
  std::vector<GenomeIdx> gidx;
  std::vector<PgDevBuf<uint8_t>> blocks;
  template <typename T>
  T* adopt(PgDevBuf<T>& b) {      // takes the block over from the buffer that allocated it; returns the view
    blocks.emplace_back();
    blocks.back().p = reinterpret_cast<uint8_t*>(b.p);
    blocks.back().cap = b.cap * sizeof(T);
    T* const view = b.p;
    b.p = nullptr;
    b.cap = 0;
    return view;
  }
};
thread_local PgAlnSink* tls_sink = nullptr;      // set by pg_anim_alignments_batch around its run_batch calls
thread_local int tls_worker = 0;   // which of the context's two (stream, scratch) sets the calling thread drives

// A worker's launch scratch.  Every array owns its block and knows its size (pg_devbuf.h); arrays that grow together are
// grown by one reserve_all.  It lives in the context and only grows; deleting it frees everything.
struct AnimScratch {
  PgDevBuf<uint32_t> list_cnt;      // 2 * SEED_GROUPS counters used by this worker's list builds
  PgDevBuf<SeedRef> srefs_d;
  PgDevBuf<SeedQry> sqry_d;
  PgDevBuf<SeedSlice> slice_d;      // [SEED_CGROUPS][pairs of the batch] (per-pair kernel)
  PgDevBuf<SeedBlk> sblk_d;         // block kernel: blocks, slots, block queries, pair tables
  PgDevBuf<SeedSlot> sslot_d;
  PgDevBuf<SeedQry> sbq_d;
  PgDevBuf<int32_t> spt_d;
  PgDevBuf<int32_t> recs_d;
  PgDevBuf<RefDesc> refs_d;
  PgDevBuf<UnitDesc> units_d;
  PgDevBuf<uint32_t> mem_count, moff, choff_d;
  PgDevBuf<int32_t> nch, status;
  PgDevBuf<pg_anim_result> out;
  // per-match arrays (sliced by moff)
  PgDevBuf<Match> mem, cm;
  PgDevBuf<int32_t> iscratch, order;
  PgDevBuf<Chain> chains;
  struct {   // the finish kernel's per-alignment arrays; it takes them as a FinishScratch
    PgDevBuf<Aln> alns;
    PgDevBuf<int32_t> a_rrec, a_qrec, idx, from;
    PgDevBuf<double> sc;
    FinishScratch view() const { return FinishScratch{alns, a_rrec, a_qrec, idx, from, sc}; }
  } S;
  PgDevBuf<uint2> wl_d;
  PgDevBuf<Match> seedbuf;          // batch-wide append buffer of the seed pass
  PgDevBuf<uint32_t> seed_total;    // [0] matches appended, [1] hits recorded
  PgDevBuf<Match> hits_d;           // hits recorded by the probe kernel for anim_hit_kernel
  PgDevBuf<Match> hits_sorted;      // the same, dealt into per-unit slices (hoff)
  PgDevBuf<uint32_t> hit_count, hoff, hit_cursor;   // per unit
  PgDevBuf<int32_t> mirror_d;       // per pair: the partner pair (roles swapped) that receives this pair's matches transposed, or -1
  PgDevBuf<BigUnit> big_d;          // cluster stage: units whose chains are extracted by ranges, the range work items, their counts
  PgDevBuf<uint2> ranges_d;
  PgDevBuf<RangeOut> range_out;
  bool lds_attr_set = false;        // the probe kernels' dynamic-LDS limit has been raised on this context's device
  // A4x, the postnuc extension stage (pga_postnuc.inc)
  PgDevBuf<pgn::PnAln> pn;          // per-unit alignment lists, sliced by moff like the per-match arrays
  PgDevBuf<uint8_t> pn_fused;       // per chain: already extended / fused / shadowed
  PgDevBuf<int32_t> pn_n;           // per unit: alignments (< 0: capacity)
  PgDevBuf<uint32_t> pn_cursor;     // the persistent waves' hand-out counters (PnCursor)
  PgDevBuf<uint32_t> pn_gscratch;   // [waves][PN_GLOBAL_WORDS] anti-diagonals too wide for LDS
  PgDevBuf<uint32_t> pn_wide;       // request slots handed from the narrow forced kernel to the wide one
  PgDevBuf<PnForcedReq> pn_reqs;    // the launch's deferred forced runs (at most one per alignment started: <= chains)
  PgDevBuf<pgn::PnGap> pn_gaps;     // match-to-match alignments by match slot
  PgDevBuf<pgn::PnFwd> pn_fwd;      // forward extensions by cluster (moff-relative position in the unit's order)
  PgDevBuf<pgn::PnBwd> pn_bwd;      // backward searches run ahead of the walks, by cluster (as pn_fwd)
  PgDevBuf<pgn::PnTurn> pn_tlog;    // the walks' turn logs (pgn::PnPairSync), sliced by moff: at most one turn per cluster
  PgDevBuf<int32_t> pn_born;        // per alignment: the key of the turn that pushed it
  PgDevBuf<uint32_t> pn_porder;     // pairs by descending cluster count of their larger strand
  PgDevBuf<pgn::PnPiece> pn_pieces; // traceback runs: the walks' pieces (pn_piece_base)
  PgDevBuf<uint32_t> pn_npieces;    // per unit
  PgDevBuf<uint8_t> tr_arena;       // traceback pass: the jobs' slabs
  PgDevBuf<uint32_t> tr_out;        // ... their paths (run-length coded)
  PgDevBuf<PnTraceJob> tr_jobs;
  PgDevBuf<unsigned long long> tr_off, tr_cursor;
  PgDevBuf<int32_t> tr_cnt;
  PgDevBuf<PnGapTask> pn_tasks;     // [4][pn.cap]: small gaps for the lane kernel by size class, then the wave engine's list
  PgDevBuf<uint32_t> pn_order;      // units by descending cluster count
  size_t pn_req_n = 0;              // slots of pn_reqs the latest launch used (its req_cap)
  // fragment mode (ANIb)
  PgDevBuf<int32_t> fr_tables;      // frag_pos | frag_len | rec_frag0 of every distinct query genome of the batch
  PgDevBuf<FragPair> fr_pairs;
  PgDevBuf<uint32_t> fr_slot_pair, fr_off, fr_nrows;
  PgDevBuf<uint64_t> fr_ebase;
  PgDevBuf<FragSeed> fr_entries;
  PgDevBuf<FragRow> fr_rows;
  PgDevBuf<pg_anib_result> fr_out;
  PgDevBuf<uint32_t> fr_list, fr_nlist, fr_wtmp;   // word tier: slots to search again, their number, scan scratch
  PgDevBuf<WordIdx> fr_widx;
  PgDevBuf<uint32_t> fr_roff, fr_rsum, fr_prows;   // packed rows: slot offsets (+ the total), the scan's block sums, rows per pair
  PgDevBuf<FragRow> fr_packed;                     // ... and the launch's rows back to back
};

// Room for `need` elements in every buffer of a group, each grown to `alloc` if it is short.  Every buffer is tested by its own
// size, so a group that an allocation failure left half-grown is completed by the next call.
template <typename... B>
hipError_t reserve_all(size_t need, size_t alloc, B&... bufs) {
  hipError_t e = hipSuccess;
  ((e = e == hipSuccess ? bufs.reserve(need, alloc) : e), ...);
  return e;
}
}  // namespace

static AnimScratch* anim_scratch(pg_ctx* ctx) {
  void*& slot = tls_worker ? ctx->anim_scratch_w[tls_worker] : ctx->anim_scratch;
  if (!slot) slot = new AnimScratch();
  return static_cast<AnimScratch*>(slot);
}
static AnimLists* anim_lists(pg_ctx* ctx) {   // (callers hold ctx->anim_mu)
  if (!ctx->anim_lists) ctx->anim_lists = new AnimLists();
  return static_cast<AnimLists*>(ctx->anim_lists);
}
static hipStream_t cur_stream(pg_ctx* ctx) { return tls_worker ? ctx->stream_w[tls_worker] : ctx->stream; }
void pg_anim_set_worker(pg_ctx* ctx, int worker) {
  tls_worker = worker > 0 && worker < pg_ctx::MAX_WORKERS ? worker : 0;
  pg_tls_stream = cur_stream(ctx);
}

void pg_anim_set_sink(PgAlnSink* sink) { tls_sink = sink; }
int pg_anim_counters_read(pg_ctx* ctx, uint64_t* out, int reset) {
  PG_HIP(ctx, hipDeviceSynchronize());
  unsigned long long a[32], b[32], z[32] = {0};
  PG_HIP(ctx, hipMemcpyFromSymbol(a, HIP_SYMBOL(g_pn_stats), sizeof(a)));
  PG_HIP(ctx, hipMemcpyFromSymbol(b, HIP_SYMBOL(g_pn_kstats), sizeof(b)));
  for (int i = 0; i < 32; ++i) { out[i] = a[i]; out[32 + i] = b[i]; }
  if (reset) {
    PG_HIP(ctx, hipMemcpyToSymbol(HIP_SYMBOL(g_pn_stats), z, sizeof(z)));
    PG_HIP(ctx, hipMemcpyToSymbol(HIP_SYMBOL(g_pn_kstats), z, sizeof(z)));
  }
  return PG_OK;
}

void pg_anim_drop_lists(pg_ctx* ctx) {
  std::lock_guard<std::mutex> lk(ctx->anim_mu);
  AnimLists* A = static_cast<AnimLists*>(ctx->anim_lists);
  if (!A) return;
  A->gidx.clear();
  A->blocks.clear();
}

// Build the seed lists the batch needs and does not have yet: reference role for `ref_genomes`, query role for `qry_genomes`.
static int anim_ensure_lists(pg_ctx* ctx, AnimScratch* A, const std::vector<int32_t>& ref_genomes, const std::vector<int32_t>& qry_genomes,
                             int qstep) {
  std::lock_guard<std::mutex> lk(ctx->anim_mu);   // one worker builds at a time; a list is complete before anyone else sees it
  AnimLists* LS = anim_lists(ctx);
  if (LS->gidx.size() < ctx->genomes.size()) LS->gidx.resize(ctx->genomes.size());
  // A list counts as built when its pointer is set, and it outlives this call (shared by the workers): whatever this call
  // allocated is taken back if anything after the allocation fails, so that no later call seeds from a half-built list.
  std::vector<std::pair<uint64_t**, uint32_t**>> mine;
  const size_t blocks0 = LS->blocks.size();
  const int rc_all = [&]() -> int {
  bool built = false;
  if (!A->list_cnt) {
    PG_HIP(ctx, A->list_cnt.reserve((size_t)2 * SEED_GROUPS));
    PG_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(anim_list_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(2 * SEED_GROUPS * 4)));
  }
  std::vector<int32_t> fresh_refs;
  for (int role = 0; role < 2; ++role) {
    for (int32_t gid : role ? qry_genomes : ref_genomes) {
      GenomeIdx& X = LS->gidx[gid];
      uint64_t*& qlist = qstep == 1 ? X.qry_list1 : X.qry_list;
      uint32_t*& qgoff = qstep == 1 ? X.qry_goff1 : X.qry_goff;
      if (role ? qlist != nullptr : X.ref_list != nullptr) continue;
      const PgGenome& G = ctx->genomes[gid];
      const int32_t len = (int32_t)G.stream_len;
      const uint32_t n_sub = role ? 2 * SEED_GROUPS : SEED_GROUPS;
      const size_t bound = role ? 2 * ((size_t)len / qstep + 1) : (size_t)len + 1;
      uint64_t*& list = role ? qlist : X.ref_list;
      uint32_t*& goff = role ? qgoff : X.ref_goff;
      mine.emplace_back(&list, &goff);
      PgDevBuf<uint64_t> new_list;
      PgDevBuf<uint32_t> new_goff;
      PG_HIP(ctx, new_list.reserve(bound));      // (bound >= 1)
      PG_HIP(ctx, new_goff.reserve((size_t)n_sub + 3));
      list = LS->adopt(new_list);
      goff = LS->adopt(new_goff);
      const uint32_t* codes = ctx->d_codes + G.arena_start / 16;
      const uint32_t* mask = ctx->d_mask + G.arena_start / 32;
      const int32_t n_idx = role ? len / qstep + 1 : len;
      const dim3 grid((uint32_t)(n_idx + LIST_CHUNK - 1) / LIST_CHUNK, role ? 2 : 1);
      PG_HIP(ctx, hipMemsetAsync(A->list_cnt, 0, (size_t)n_sub * 4, cur_stream(ctx)));
      if (grid.x)   // (an empty genome still gets its all-zero offset table from the scan)
        hipLaunchKernelGGL(anim_list_kernel, grid, dim3(LIST_BLOCK), (size_t)n_sub * 4, cur_stream(ctx), codes, mask, len, role, A->list_cnt,
                           (const uint32_t*)nullptr, (uint64_t*)nullptr, 0, qstep);
      if (role)
        hipLaunchKernelGGL(anim_list_scan_kernel<2 * SEED_GROUPS / LIST_SCAN_BLOCK>, dim3(1), dim3(LIST_SCAN_BLOCK), 0, cur_stream(ctx), A->list_cnt, goff);
      else
        hipLaunchKernelGGL(anim_list_scan_kernel<SEED_GROUPS / LIST_SCAN_BLOCK>, dim3(1), dim3(LIST_SCAN_BLOCK), 0, cur_stream(ctx), A->list_cnt, goff);
      if (grid.x)
        hipLaunchKernelGGL(anim_list_kernel, grid, dim3(LIST_BLOCK), (size_t)n_sub * 4, cur_stream(ctx), codes, mask, len, role, A->list_cnt,
                           (const uint32_t*)goff, list, 1, qstep);
      if (!role) fresh_refs.push_back(gid);
      built = true;
    }
  }
  PG_HIP(ctx, hipGetLastError());
  if (built) PG_HIP(ctx, hipStreamSynchronize(cur_stream(ctx)));
  for (int32_t gid : fresh_refs) {
    uint32_t mx[2];   // largest group, largest coarse group
    PG_HIP(ctx, hipMemcpy(mx, LS->gidx[gid].ref_goff + SEED_GROUPS + 1, 8, hipMemcpyDeviceToHost));
    LS->gidx[gid].ref_max_fine = mx[0];
    LS->gidx[gid].ref_max = mx[1];
  }
  return PG_OK;
  }();
  if (rc_all != PG_OK) {
    (void)hipStreamSynchronize(cur_stream(ctx));      // nothing of this call may still be writing into them
    for (auto& pr : mine) *pr.first = nullptr, *pr.second = nullptr;
    LS->blocks.erase(LS->blocks.begin() + blocks0, LS->blocks.end());      // (the lock is held: every block past blocks0 is this call's)
  }
  return rc_all;
}

static void anim_free_one(void*& slot) {
  delete static_cast<AnimScratch*>(slot);
  slot = nullptr;
}
// the workers' launch scratch only (the per-genome seed lists stay): the context must be idle
void pg_anim_release_worker_scratch(pg_ctx* ctx) {
  (void)hipStreamSynchronize(ctx->stream);
  for (int w = 1; w < pg_ctx::MAX_WORKERS; ++w) (void)hipStreamSynchronize(ctx->stream_w[w]);
  anim_free_one(ctx->anim_scratch);
  for (int w = 1; w < pg_ctx::MAX_WORKERS; ++w) anim_free_one(ctx->anim_scratch_w[w]);
  ctx->anim_scratch_matches_held = 0;
}
void pg_anim_free_scratch(pg_ctx* ctx) {
  pg_anim_drop_lists(ctx);
  delete static_cast<AnimLists*>(ctx->anim_lists);
  ctx->anim_lists = nullptr;
  anim_free_one(ctx->anim_scratch);
  for (int w = 1; w < pg_ctx::MAX_WORKERS; ++w) anim_free_one(ctx->anim_scratch_w[w]);
  ctx->anim_scratch_matches_held = 0;
}

static_assert(sizeof(FragRow) == sizeof(pg_anib_row), "FragRow is pg_anib_row");
static int anib_frag_stage(pg_ctx* ctx, AnimScratch* A, const int32_t* qry_ids, uint32_t n_pairs, const std::vector<uint32_t>& cnt,
                           const PgFragArgs& F, const std::vector<int32_t>& ref_list, const std::vector<uint32_t>& ref_of_pair);

// The alignment records of a finished batch -> the caller's sink; with_indels: the traceback pass (anim_trace_kernel: one
// search / forced piece of the walks per thread, the scalar engine with its backpointer store) and the .delta lists
// (pg_anim_trace.h).  Host work here is list management: sizing the jobs' slabs from the wave engine's own bookkeeping,
// batching them into the arena, stitching the pieces' paths.
static int anim_collect_indels(pg_ctx* ctx, AnimScratch* A, uint32_t n_pairs, const std::vector<uint32_t>& moff, const std::vector<uint32_t>& choff,
                               const std::vector<size_t>& pair_first, PgAlnSink& sink);

// an alignment in forward stream coordinates, half-open -> MUMmer's 1-based closed coordinates within its records, which start
// at the stream positions ro (reference) and qo (query)
static pg_anim_alignment to_record(const Aln& a, int32_t ro, int32_t qo) {
  pg_anim_alignment x;
  x.rs = a.rs - ro + 1; x.re = a.re - ro;
  x.qs = a.strand ? a.qe - qo : a.qs - qo + 1;
  x.qe = a.strand ? a.qs - qo + 1 : a.qe - qo;
  x.errors = a.errors; x.kept = a.keep;
  return x;
}

static int anim_collect(pg_ctx* ctx, AnimScratch* A, const int32_t* ref_ids, const int32_t* qry_ids, uint32_t n_pairs, const pg_anim_result* res,
                        const std::vector<uint32_t>& choff, PgAlnSink& sink) {
  const uint32_t n_units = 2 * n_pairs;
  std::vector<uint32_t> moff((size_t)n_units + 1);
  PG_HIP(ctx, hipMemcpy(moff.data(), A->moff, moff.size() * 4, hipMemcpyDeviceToHost));
  const size_t total = moff[n_units];
  std::vector<Aln> al(total ? total : 1);
  std::vector<int32_t> rr(total ? total : 1), qr(total ? total : 1);
  if (total) {
    PG_HIP(ctx, hipMemcpy(al.data(), A->S.alns, total * sizeof(Aln), hipMemcpyDeviceToHost));
    PG_HIP(ctx, hipMemcpy(rr.data(), A->S.a_rrec, total * 4, hipMemcpyDeviceToHost));
    PG_HIP(ctx, hipMemcpy(qr.data(), A->S.a_qrec, total * 4, hipMemcpyDeviceToHost));
  }
  std::vector<size_t> pair_first(n_pairs);
  for (uint32_t p = 0; p < n_pairs; ++p) {
    if (res[p].status == PG_E_CAPACITY) return pg_fail(ctx, PG_E_CAPACITY, "anim: work buffers overflowed for a pair of the batch");
    const PgGenome& G = ctx->genomes[ref_ids[p]];
    const PgGenome& H = ctx->genomes[qry_ids[p]];
    const uint32_t n = (uint32_t)res[p].reserved;
    pair_first[p] = sink.alns.size();
    for (uint32_t i = 0; i < n; ++i) {
      const int32_t r_ = rr[moff[2 * p] + i], q_ = qr[moff[2 * p] + i];
      pg_anim_alignment x = to_record(al[moff[2 * p] + i], G.rec_start[r_], H.rec_start[q_]);
      x.ref_rec = r_; x.qry_rec = q_;
      sink.alns.push_back(x);
    }
    sink.pair_count.push_back(n);
  }
  if (!sink.with_indels) return PG_OK;
  sink.indels.resize(sink.alns.size());
  if (!total || !choff[n_units]) return PG_OK;      // no clusters at all: no alignments, nothing to trace
  return anim_collect_indels(ctx, A, n_pairs, moff, choff, pair_first, sink);
}

// The traceback pass of anim_collect: the .delta list of every record the sink has just received (pair p's start at pair_first[p]).
static int anim_collect_indels(pg_ctx* ctx, AnimScratch* A, uint32_t n_pairs, const std::vector<uint32_t>& moff, const std::vector<uint32_t>& choff,
                               const std::vector<size_t>& pair_first, PgAlnSink& sink) {
  const uint32_t n_units = 2 * n_pairs;
  const size_t total = moff[n_units], n_wl = choff[n_units];
  // ---- the walks' pieces
  std::vector<pgn::PnAln> pn(total);
  std::vector<int32_t> pn_n(n_units);
  std::vector<uint32_t> npieces(n_units);
  const size_t piece_total = pn_piece_base(total, (uint32_t)n_wl, n_units);
  std::vector<pgn::PnPiece> pieces(piece_total ? piece_total : 1);
  PG_HIP(ctx, hipMemcpy(pn.data(), A->pn, total * sizeof(pgn::PnAln), hipMemcpyDeviceToHost));
  PG_HIP(ctx, hipMemcpy(pn_n.data(), A->pn_n, (size_t)n_units * 4, hipMemcpyDeviceToHost));
  PG_HIP(ctx, hipMemcpy(npieces.data(), A->pn_npieces, (size_t)n_units * 4, hipMemcpyDeviceToHost));
  PG_HIP(ctx, hipMemcpy(pieces.data(), A->pn_pieces, piece_total * sizeof(pgn::PnPiece), hipMemcpyDeviceToHost));
  const size_t req_cap = A->pn_req_n;      // as the launch laid the two request lists out
  std::vector<PnForcedReq> reqs(req_cap);
  PG_HIP(ctx, hipMemcpy(reqs.data(), A->pn_reqs, req_cap * sizeof(PnForcedReq), hipMemcpyDeviceToHost));
  // ---- one job per search / forced piece
  struct JobRef { uint32_t unit; uint32_t piece; uint64_t bytes; };      // piece: index in the unit's list
  std::vector<PnTraceJob> jobs;
  std::vector<JobRef> refs_;
  for (uint32_t u = 0; u < n_units; ++u) {
    const size_t pb = pn_piece_base(moff[u], choff[u], u);
    if (pn_n[u] < 0 || npieces[u] > pn_piece_cap((size_t)moff[u + 1] - moff[u], choff[u + 1] - choff[u]))
      return pg_fail(ctx, PG_E_CAPACITY, "anim traceback: a unit's piece list overflowed");
    for (uint32_t k = 0; k < npieces[u]; ++k) {
      const pgn::PnPiece& P = pieces[pb + k];
      if (P.kind == pgn::PIECE_MATCH || P.kind == pgn::PIECE_VISIT) continue;
      PnTraceJob J{};
      J.unit = u; J.m_o = P.m_o; J.A0 = P.A0; J.B0 = P.B0; J.A1 = P.A1; J.B1 = P.B1;
      uint64_t cells = P.cells;
      uint32_t wmax = P.wmax;
      if (P.kind == pgn::PIECE_FORCED) {
        J.tA = P.A1; J.tB = P.B1;
        if (P.aux >= req_cap) return pg_fail(ctx, PG_E_INTERNAL, "anim traceback: forced piece without its request");
        J.band_w = reqs[P.aux].w;
        const int32_t N = P.A1 - P.A0 + 1, M_ = P.B1 - P.B0 + 1;
        cells = 0; wmax = 0;
        for (int32_t d = 1; d <= N + M_; ++d) {      // the cells of the certified band, as the engine clips them
          int32_t lo = d - N > 0 ? d - N : 0, hi = d < M_ ? d : M_;
          if (J.band_w >= 0) pgn::forced_band_clip(d, N, M_, J.band_w, lo, hi);
          if (hi >= lo) { cells += (uint64_t)(hi - lo + 1); if ((uint32_t)(hi - lo + 1) > wmax) wmax = (uint32_t)(hi - lo + 1); }
        }
      } else {
        J.tA = P.tA; J.tB = P.tB; J.band_w = -1;
        if (P.cells == 0xFFFFFFFFu) return pg_fail(ctx, PG_E_CAPACITY, "anim traceback: a search outgrew the register engine");
      }
      const int32_t N = J.tA - J.A0 + 1, M_ = J.tB - J.B0 + 1;
      J.cap = wmax + 2; J.dcap = (uint32_t)(N + M_ + 4); J.rle_cap = (uint32_t)(N + M_ + 4); J.bp_cap = cells;
      const uint64_t bytes = (uint64_t)J.cap * 3 * sizeof(pgn::Cell) + (uint64_t)J.dcap * 8 + (uint64_t)J.rle_cap * 4 + ((cells + 15) & ~15ull) + 16;
      jobs.push_back(J);
      refs_.push_back(JobRef{u, k, (bytes + 15) & ~15ull});
    }
  }
  // ---- batches that fit the arena (largest jobs first: threads of a wave get pieces of similar size)
  std::vector<uint32_t> order(jobs.size());
  for (uint32_t i = 0; i < order.size(); ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return refs_[a].bytes > refs_[b].bytes; });
  std::vector<std::vector<uint32_t>> rle(jobs.size());
  const uint64_t ARENA = 6ull << 30, OUT_MAX = 192ull << 20;      // bytes of slabs / path entries per launch
  PG_HIP(ctx, A->tr_cursor.reserve(2));
  for (size_t b0 = 0; b0 < order.size();) {
    uint64_t bytes = 0, outs = 0;
    size_t b1 = b0;
    while (b1 < order.size() && (b1 == b0 || (bytes + refs_[order[b1]].bytes <= ARENA && outs + jobs[order[b1]].rle_cap <= OUT_MAX))) {
      bytes += refs_[order[b1]].bytes; outs += jobs[order[b1]].rle_cap; ++b1;
    }
    const size_t nb = b1 - b0;
    std::vector<PnTraceJob> hj(nb);
    uint64_t at = 0;
    for (size_t k = 0; k < nb; ++k) { hj[k] = jobs[order[b0 + k]]; hj[k].slab = at; at += refs_[order[b0 + k]].bytes; }
    PG_HIP(ctx, A->tr_arena.reserve((size_t)bytes));
    PG_HIP(ctx, A->tr_out.reserve((size_t)outs));
    PG_HIP(ctx, A->tr_jobs.reserve(nb));
    PG_HIP(ctx, A->tr_off.reserve(nb));
    PG_HIP(ctx, A->tr_cnt.reserve(nb));
    PG_HIP(ctx, hipMemcpyAsync(A->tr_jobs, hj.data(), nb * sizeof(PnTraceJob), hipMemcpyHostToDevice, cur_stream(ctx)));
    PG_HIP(ctx, hipMemsetAsync(A->tr_cursor, 0, 8, cur_stream(ctx)));
    hipLaunchKernelGGL(anim_trace_kernel, dim3((uint32_t)((nb + 63) / 64)), dim3(64), 0, cur_stream(ctx), A->refs_d, A->units_d, A->tr_jobs, (uint32_t)nb,
                       A->tr_arena, A->tr_out, (unsigned long long)outs, A->tr_cursor, A->tr_off, A->tr_cnt);
    PG_HIP(ctx, hipGetLastError());
    std::vector<unsigned long long> off(nb);
    std::vector<int32_t> cnt(nb);
    unsigned long long used = 0;
    PG_HIP(ctx, hipMemcpyAsync(off.data(), A->tr_off, nb * 8, hipMemcpyDeviceToHost, cur_stream(ctx)));
    PG_HIP(ctx, hipMemcpyAsync(cnt.data(), A->tr_cnt, nb * 4, hipMemcpyDeviceToHost, cur_stream(ctx)));
    PG_HIP(ctx, hipMemcpyAsync(&used, A->tr_cursor, 8, hipMemcpyDeviceToHost, cur_stream(ctx)));
    PG_HIP(ctx, hipStreamSynchronize(cur_stream(ctx)));
    std::vector<uint32_t> out((size_t)used ? (size_t)used : 1);
    if (used) PG_HIP(ctx, hipMemcpy(out.data(), A->tr_out, (size_t)used * 4, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < nb; ++k) {
      if (cnt[k] < 0) return pg_fail(ctx, PG_E_INTERNAL, "anim traceback: a piece did not repeat in the scalar engine");
      rle[order[b0 + k]].assign(out.begin() + (size_t)off[k], out.begin() + (size_t)off[k] + (size_t)cnt[k]);
    }
    b0 = b1;
  }
  // ---- stitch: per unit, the paths of its alignments; then the pair's records in MUMmer's print order (PIECE_VISIT)
  size_t job_at = 0;
  for (uint32_t p = 0; p < n_pairs; ++p) {
    const size_t n_rec = (size_t)pn_n[2 * p] + (size_t)pn_n[2 * p + 1];
    if (n_rec != sink.pair_count[sink.pair_count.size() - n_pairs + p]) return pg_fail(ctx, PG_E_INTERNAL, "anim traceback: record counts differ");
    std::vector<std::vector<int64_t>> lists(n_rec);
    std::vector<std::tuple<int32_t, int32_t, int32_t>> key(n_rec);      // (visit, strand, index in the unit)
    for (uint32_t u = 2 * p; u < 2 * p + 2; ++u) {
      const size_t pb = pn_piece_base(moff[u], choff[u], u);
      std::vector<int32_t> job_of(npieces[u], -1);
      for (uint32_t k = 0; k < npieces[u]; ++k)
        if (pieces[pb + k].kind == pgn::PIECE_SEARCH || pieces[pb + k].kind == pgn::PIECE_FORCED) job_of[k] = (int32_t)job_at++;
      std::vector<std::vector<int64_t>> deltas;
      std::vector<int32_t> visit;
      std::string why;
      static const uint32_t none = 0;
      if (!pgt::unit_deltas(pieces.data() + pb, (int32_t)npieces[u], pn.data() + moff[u], pn_n[u],
                            [&](int32_t k, int32_t& c) -> const uint32_t* { const auto& v = rle[(size_t)job_of[k]]; c = (int32_t)v.size(); return v.empty() ? &none : v.data(); },
                            deltas, visit, &why))
        return pg_fail(ctx, PG_E_INTERNAL, "anim traceback: " + why);
      const size_t base = (u & 1) ? (size_t)pn_n[u - 1] : 0;
      for (int32_t i = 0; i < pn_n[u]; ++i) { lists[base + (size_t)i] = std::move(deltas[(size_t)i]); key[base + (size_t)i] = std::make_tuple(visit[(size_t)i], (int32_t)(u & 1), i); }
    }
    std::vector<size_t> perm(n_rec);
    for (size_t i = 0; i < n_rec; ++i) perm[i] = i;
    std::stable_sort(perm.begin(), perm.end(), [&](size_t a, size_t b) { return key[a] < key[b]; });
    std::vector<pg_anim_alignment> recs(n_rec);
    for (size_t i = 0; i < n_rec; ++i) recs[i] = sink.alns[pair_first[p] + perm[i]];
    for (size_t i = 0; i < n_rec; ++i) { sink.alns[pair_first[p] + i] = recs[i]; sink.indels[pair_first[p] + i] = std::move(lists[perm[i]]); }
  }
  return PG_OK;
}

// ---- the batch driver: pg_anim_run_batch and its stages, in launch order --------------------------------------------------
namespace {
// What the stages of one call share on the host.  Every vector that is uploaded with an asynchronous copy lives here, so that
// it outlives the copy.
struct Batch {
  pg_ctx* ctx;
  AnimScratch* A;
  const int32_t *ref_ids, *qry_ids;   // the call's pairs; the launch processes the first n_pairs of them
  const PgFragArgs* frag;
  int filter_1to1, maxmatch;
  uint64_t max_matches;
  uint32_t n_pairs = 0, n_units = 0;
  void set_pairs(uint32_t n) { n_pairs = n; n_units = 2 * n; }   // (frag_limit_pairs and seed_stage shorten the launch)
  int qstep = SEED_STEP;               // query-strand sampling of the seed lists
  bool use_mirror = false, use_blocks = false, trace = false;
  uint32_t max_slots = SEED_MAX_SLOTS;   // the largest LDS table either seeding kernel may use (PYANI_SEED_MAX_SLOTS lowers it)
  uint32_t blk_slots = SEED_MAX_SLOTS;   // the table size a block is planned for (<= max_slots)
  // descriptors
  std::vector<int32_t> ref_list;       // distinct references, in the order of ref_ids
  std::vector<uint32_t> ref_of_pair;
  std::vector<RefDesc> refs;
  std::vector<UnitDesc> units;
  std::vector<int32_t> recs;
  // the seed plan, made again by every attempt of seed_stage
  std::vector<int32_t> mirror;
  std::vector<uint8_t> seeded;
  std::vector<GenomeIdx> LSv;          // snapshot of the genomes' seed lists
  std::vector<SeedRef> srefs;
  std::vector<SeedQry> sqry, bqry;
  std::vector<SeedBlk> blks;
  std::vector<SeedSlot> bslots;
  std::vector<int32_t> bpair;
  uint32_t slots = 256, n_srefs = 0, n_blks = 0, slot_shift = 0;
  uint32_t seed_passes = 1;            // most passes a planned group needs (pg_seed_plan.h); > 1 launches the kernels with the pass loop
  uint32_t slice_stride = 0;           // the slice table is laid out for the whole batch even if only a prefix is seeded again
  // what the stages leave for the next ones
  std::vector<uint32_t> cnt, moff, choff;   // per unit: matches, slice offsets (moff.back() = M), cluster offsets
  std::vector<int32_t> nch;
  uint32_t total = 0;                  // matches in the append buffer
  ClusterOut O{};
};

// the counters of AnimScratch::pn_cursor, zeroed before every extension stage
enum PnCursor : uint32_t {
  PNC_UNIT = 0,            // unit cursor of the walks
  PNC_FORCED_N = 1,        // forced runs recorded ...
  PNC_FORCED_CUR = 2,      // ... and their cursor
  PNC_GAP_BIG = 3,         // chain / big-gap cursor
  PNC_GAP_LANE = 4,        // 4, 5, 6: small gaps by size class
  PNC_FORCED_LONG = 7,     // forced runs recorded: the long ones
  PNC_FWD = 8,             // cluster cursor of the forward extensions
  PNC_REHEARSE = 9,        // unit cursor of the rehearsal
  PNC_BWD = 10,            // cluster cursor of the backward searches
  PNC_GAP_WAVE = 11,       // gaps left to the wave engine
  PNC_WIDE_N = 12, PNC_WIDE_CUR = 13,       // wide forced runs: count / cursor
  PNC_HUGE_N = 14, PNC_HUGE_CUR = 15,       // huge ones
  PNC_STRIPS_N = 16, PNC_STRIPS_CUR = 17,   // the strips' list
  PNC_WORDS = 24
};
}  // namespace

// fragment mode: a launch holds at most max_slots (pair, fragment) slots
static void frag_limit_pairs(Batch& B) {
  pg_ctx* ctx = B.ctx;
  uint64_t slots = 0;
  uint32_t fit = 0;
  for (uint32_t p = 0; p < B.n_pairs; ++p) {
    const PgGenome& Q = ctx->genomes[B.qry_ids[p]];
    uint64_t nf = 0;
    for (uint32_t r = 0; r < Q.n_rec; ++r) nf += ((uint64_t)(Q.rec_start[r + 1] - 1 - Q.rec_start[r]) + B.frag->fragsize - 1) / B.frag->fragsize;
    if (p > 0 && slots + nf > B.frag->max_slots) break;
    slots += nf;
    fit = p + 1;
  }
  B.set_pairs(fit);
}

// RefDesc per distinct reference, UnitDesc per (pair, strand), the records table behind both; grows what is sized by them; uploads
static int build_descriptors(Batch& B) {
  pg_ctx* ctx = B.ctx;
  AnimScratch* A = B.A;
  const uint32_t n_pairs = B.n_pairs, n_units = B.n_units;
  B.ref_of_pair.resize(n_pairs);
  for (uint32_t p = 0; p < n_pairs; ++p) {
    if (B.ref_list.empty() || B.ref_list.back() != B.ref_ids[p]) B.ref_list.push_back(B.ref_ids[p]);
    B.ref_of_pair[p] = (uint32_t)B.ref_list.size() - 1;
  }
  const uint32_t n_refs = (uint32_t)B.ref_list.size();
  std::vector<RefDesc>& refs = B.refs;
  std::vector<int32_t>& recs = B.recs;
  refs.resize(n_refs);
  std::vector<uint32_t> ref_rec_off(n_refs), qry_rec_off(n_pairs);
  for (uint32_t r = 0; r < n_refs; ++r) {
    const PgGenome& G = ctx->genomes[B.ref_list[r]];
    refs[r].codes = ctx->d_codes + G.arena_start / 16;
    refs[r].mask = ctx->d_mask + G.arena_start / 32;
    refs[r].len = (int32_t)G.stream_len;
    refs[r].n_rec = (int32_t)G.n_rec;
    ref_rec_off[r] = (uint32_t)recs.size();
    recs.insert(recs.end(), G.rec_start.begin(), G.rec_start.end());
  }
  for (uint32_t p = 0; p < n_pairs; ++p) {
    const PgGenome& Q = ctx->genomes[B.qry_ids[p]];
    qry_rec_off[p] = (uint32_t)recs.size();
    recs.insert(recs.end(), Q.rec_start.begin(), Q.rec_start.end());
  }
  PG_HIP(ctx, A->recs_d.reserve(recs.size()));
  PG_HIP(ctx, reserve_all(n_refs, n_refs, A->refs_d, A->srefs_d));
  PG_HIP(ctx, reserve_all(n_units, n_units, A->units_d, A->mem_count, A->hit_count, A->hit_cursor, A->nch));
  PG_HIP(ctx, reserve_all((size_t)n_units + 1, (size_t)n_units + 1, A->moff, A->choff_d, A->hoff));
  PG_HIP(ctx, reserve_all(n_pairs, n_pairs, A->status, A->sqry_d, A->out, A->mirror_d));
  for (uint32_t r = 0; r < n_refs; ++r) refs[r].rec_start = A->recs_d + ref_rec_off[r];
  B.units.resize(n_units);
  for (uint32_t p = 0; p < n_pairs; ++p) {
    const PgGenome& Q = ctx->genomes[B.qry_ids[p]];
    for (int s = 0; s < 2; ++s) {
      UnitDesc& U = B.units[2 * p + s];
      U.codes = ctx->d_codes + Q.arena_start / 16;
      U.mask = ctx->d_mask + Q.arena_start / 32;
      U.len = (int32_t)Q.stream_len;
      U.rec_start = A->recs_d + qry_rec_off[p];
      U.n_rec = (int32_t)Q.n_rec;
      U.strand = s;
      U.pair = (int32_t)p;
      U.ref = (int32_t)B.ref_of_pair[p];
    }
  }
  PG_HIP(ctx, hipMemcpyAsync(A->recs_d, recs.data(), recs.size() * 4, hipMemcpyHostToDevice, cur_stream(ctx)));
  PG_HIP(ctx, hipMemcpyAsync(A->refs_d, refs.data(), n_refs * sizeof(RefDesc), hipMemcpyHostToDevice, cur_stream(ctx)));
  PG_HIP(ctx, hipMemcpyAsync(A->units_d, B.units.data(), n_units * sizeof(UnitDesc), hipMemcpyHostToDevice, cur_stream(ctx)));
  return PG_OK;
}

// Roles: when the launch holds a pair in BOTH directions, (A, B) and (B, A), only one of them is seeded — the maximal exact
// matches of the two are the same set, and anim_hit_kernel appends each match a second time, transposed, for the partner
// (`mirror`).  The seeded direction is the one whose reference has more pairs in the launch (longer query streams per LDS
// table); equal counts: decided by the ids' parity, so that every genome is the table for half of its partners.
static void assign_mirrors(Batch& B, uint32_t limit) {
  const int32_t *ref_ids = B.ref_ids, *qry_ids = B.qry_ids;
  std::vector<int32_t>& mirror = B.mirror;
  std::vector<uint8_t>& seeded = B.seeded;
  std::fill(mirror.begin(), mirror.end(), -1);
  std::fill(seeded.begin(), seeded.end(), (uint8_t)0);
  std::fill(seeded.begin(), seeded.begin() + limit, (uint8_t)1);
  if (!B.use_mirror || limit <= 1) return;
  std::vector<uint32_t> deg(B.ctx->genomes.size(), 0);
  for (uint32_t p = 0; p < limit; ++p) ++deg[ref_ids[p]];
  std::vector<uint32_t> idx(limit);
  for (uint32_t p = 0; p < limit; ++p) idx[p] = p;
  auto key = [&](uint32_t p) {   // unordered pair, then direction, then position: partners end up next to each other
    const uint32_t a = (uint32_t)ref_ids[p], b = (uint32_t)qry_ids[p];
    return std::make_tuple(a < b ? a : b, a < b ? b : a, a < b ? 0 : 1, p);
  };
  std::sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return key(x) < key(y); });
  for (uint32_t i = 0; i < limit;) {
    uint32_t j = i;
    while (j < limit && std::get<0>(key(idx[j])) == std::get<0>(key(idx[i])) && std::get<1>(key(idx[j])) == std::get<1>(key(idx[i]))) ++j;
    uint32_t m = i;   // [i, m): direction min -> max, [m, j): the other direction (a pair listed twice pairs up once)
    while (m < j && std::get<2>(key(idx[m])) == 0) ++m;
    if (ref_ids[idx[i]] != qry_ids[idx[i]])
      for (uint32_t k = 0; i + k < m && m + k < j; ++k) {
        const uint32_t p = idx[i + k], p2 = idx[m + k];
        const uint32_t a = (uint32_t)ref_ids[p], b = (uint32_t)qry_ids[p];
        const bool first = deg[a] != deg[b] ? deg[a] > deg[b] : ((a < b) != (((a + b) & 1u) != 0));
        if (first) { mirror[p] = (int32_t)p2; seeded[p2] = 0; } else { mirror[p2] = (int32_t)p; seeded[p] = 0; }
      }
    i = j;
  }
}

// The block kernel's plan for the seeded pairs of [0, limit), and its upload.
// Slots: per run of seeded pairs with one reference, a pair listed k times goes to the run's k-th slot (a slot's queries are
// distinct).  Blocks: consecutive slots while their largest groups sum to at most half the table and there are at most
// SEED_BLOCK_SLOTS of them; per block, its distinct queries (sorted) and the [slot][query] -> pair table.  The first slot of a
// block is taken whatever its size: a slot whose largest group exceeds half the largest table is therefore alone in its block,
// and its groups are seeded in passes (pg_seed_plan.h).
static int plan_seed_blocks(Batch& B, uint32_t limit) {
  pg_ctx* ctx = B.ctx;
  AnimScratch* A = B.A;
  const int32_t *ref_ids = B.ref_ids, *qry_ids = B.qry_ids;
  const std::vector<GenomeIdx>& LSv = B.LSv;
  std::vector<int32_t> slot_ref;
  std::vector<std::vector<uint32_t>> slot_pairs;
  std::unordered_map<int32_t, uint32_t> occ;
  uint32_t run_first = 0;
  int32_t run_ref = -1;
  for (uint32_t p = 0; p < limit; ++p) {
    if (!B.seeded[p]) continue;
    if (ref_ids[p] != run_ref) { run_ref = ref_ids[p]; run_first = (uint32_t)slot_ref.size(); occ.clear(); }
    const uint32_t k = occ[qry_ids[p]]++;
    if (run_first + k == slot_ref.size()) { slot_ref.push_back(run_ref); slot_pairs.emplace_back(); }
    slot_pairs[run_first + k].push_back(p);
  }
  std::vector<SeedBlk>& blks = B.blks;
  std::vector<SeedSlot>& bslots = B.bslots;
  std::vector<SeedQry>& bqry = B.bqry;
  std::vector<int32_t>& bpair = B.bpair;
  blks.clear(); bslots.clear(); bqry.clear(); bpair.clear();
  uint32_t max_sum = 1, max_lone = 0, max_shared = 0;   // largest block sum; of the blocks of one slot; of the others
  for (uint32_t s0 = 0; s0 < slot_ref.size();) {
    uint32_t s1 = s0, sum = 0;
    while (s1 < slot_ref.size() && s1 - s0 < (uint32_t)SEED_BLOCK_SLOTS) {
      const uint32_t w = LSv[slot_ref[s1]].ref_max_fine;
      if (s1 > s0 && 2 * (sum + w) > B.blk_slots) break;
      sum += w;
      ++s1;
    }
    max_sum = sum > max_sum ? sum : max_sum;
    if (s1 - s0 == 1) max_lone = sum > max_lone ? sum : max_lone;
    else max_shared = sum > max_shared ? sum : max_shared;
    std::vector<int32_t> qs;
    for (uint32_t t = s0; t < s1; ++t) {
      const PgGenome& G = ctx->genomes[slot_ref[t]];
      if (G.stream_len >= SEED_TAB_POS_MASK)
        return pg_fail(ctx, PG_E_CAPACITY, "anim seeding: a reference position does not fit the block table's 30 bits");
      bslots.push_back(SeedSlot{LSv[slot_ref[t]].ref_list, LSv[slot_ref[t]].ref_goff});
      for (uint32_t p : slot_pairs[t]) qs.push_back(qry_ids[p]);
    }
    std::sort(qs.begin(), qs.end());
    qs.erase(std::unique(qs.begin(), qs.end()), qs.end());
    if (qs.size() >= (1u << 25)) return pg_fail(ctx, PG_E_CAPACITY, "anim seeding: more than 2^25 queries in a block");
    const SeedBlk Bk{s0, s1, (uint32_t)bqry.size(), (uint32_t)(bqry.size() + qs.size()), (uint32_t)bpair.size()};
    for (int32_t qg : qs) bqry.push_back(SeedQry{LSv[qg].qry_list, LSv[qg].qry_goff});
    bpair.resize(bpair.size() + (size_t)(s1 - s0) * qs.size(), -1);
    for (uint32_t t = s0; t < s1; ++t)
      for (uint32_t p : slot_pairs[t]) {
        const size_t qi = (size_t)(std::lower_bound(qs.begin(), qs.end(), qry_ids[p]) - qs.begin());
        bpair[Bk.pair_tab + (size_t)(t - s0) * qs.size() + qi] = (int32_t)p;
      }
    blks.push_back(Bk);
    s0 = s1;
  }
  if (bpair.size() > (size_t)0x7FFFFFFF) return pg_fail(ctx, PG_E_CAPACITY, "anim seeding: block pair tables too large");
  B.slots = 256;
  while (B.slots < 2 * (uint64_t)max_sum && B.slots < B.max_slots) B.slots <<= 1;
  // Passes: only a block of one slot may need them (the kernel cuts that slot's group; it cannot cut a table shared by several).
  if (pg_seed_pass_count(max_shared, B.slots) != 1)
    return pg_fail(ctx, PG_E_INTERNAL, "anim seeding: a block of several slots does not fit half its table");
  B.seed_passes = pg_seed_pass_count(max_lone, B.slots);
  B.slot_shift = 0;
  while ((B.slots << B.slot_shift) < (1u << (32 - SEED_GROUP_BITS))) ++B.slot_shift;
  const uint32_t n_blks = B.n_blks = (uint32_t)blks.size();
  PG_HIP(ctx, A->sblk_d.reserve(n_blks));
  PG_HIP(ctx, A->sslot_d.reserve(bslots.size()));
  PG_HIP(ctx, A->sbq_d.reserve(bqry.size()));
  PG_HIP(ctx, A->spt_d.reserve(bpair.size()));
  if (n_blks) {
    PG_HIP(ctx, hipMemcpyAsync(A->sblk_d, blks.data(), n_blks * sizeof(SeedBlk), hipMemcpyHostToDevice, cur_stream(ctx)));
    PG_HIP(ctx, hipMemcpyAsync(A->sslot_d, bslots.data(), bslots.size() * sizeof(SeedSlot), hipMemcpyHostToDevice, cur_stream(ctx)));
    PG_HIP(ctx, hipMemcpyAsync(A->sbq_d, bqry.data(), bqry.size() * sizeof(SeedQry), hipMemcpyHostToDevice, cur_stream(ctx)));
    PG_HIP(ctx, hipMemcpyAsync(A->spt_d, bpair.data(), bpair.size() * sizeof(int32_t), hipMemcpyHostToDevice, cur_stream(ctx)));
  }
  PG_HIP(ctx, hipMemcpyAsync(A->mirror_d, B.mirror.data(), B.n_pairs * sizeof(int32_t), hipMemcpyHostToDevice, cur_stream(ctx)));
  return PG_OK;
}

// The per-pair kernel's plan for the seeded pairs of [0, limit): table size, one SeedRef per reference of seed_refs, the slice table.
static int plan_seed_pairs(Batch& B, uint32_t limit, const std::vector<int32_t>& seed_refs) {
  pg_ctx* ctx = B.ctx;
  AnimScratch* A = B.A;
  const std::vector<GenomeIdx>& LSv = B.LSv;
  const uint32_t n_pairs = B.n_pairs;
  uint32_t max_group = 1;
  for (int32_t g : seed_refs) if (LSv[g].ref_max > max_group) max_group = LSv[g].ref_max;
  B.slots = 256;
  while (B.slots < 2 * (uint64_t)max_group && B.slots < B.max_slots) B.slots <<= 1;
  B.seed_passes = pg_seed_pass_count(max_group, B.slots);   // a larger coarse group is seeded in passes
  PG_HIP(ctx, A->slice_d.reserve((size_t)B.slice_stride * SEED_CGROUPS));
  B.srefs.clear();   // one entry per reference with seeded pairs: [pair_begin, pair_end) spans them (pairs in between that
                     // are not seeded have empty slices)
  for (uint32_t p = 0; p < n_pairs; ++p) {
    B.sqry[p] = SeedQry{nullptr, nullptr};
    if (p >= limit || !B.seeded[p]) continue;
    const GenomeIdx& X = LSv[B.qry_ids[p]];
    B.sqry[p] = B.qstep == 1 ? SeedQry{X.qry_list1, X.qry_goff1} : SeedQry{X.qry_list, X.qry_goff};
    if (B.srefs.empty() || B.srefs.back().list != LSv[B.ref_ids[p]].ref_list)
      B.srefs.push_back(SeedRef{LSv[B.ref_ids[p]].ref_list, LSv[B.ref_ids[p]].ref_goff, p, p + 1});
    B.srefs.back().pair_end = p + 1;
  }
  B.n_srefs = (uint32_t)B.srefs.size();
  PG_HIP(ctx, hipMemcpyAsync(A->sqry_d, B.sqry.data(), n_pairs * sizeof(SeedQry), hipMemcpyHostToDevice, cur_stream(ctx)));
  PG_HIP(ctx, hipMemcpyAsync(A->mirror_d, B.mirror.data(), n_pairs * sizeof(int32_t), hipMemcpyHostToDevice, cur_stream(ctx)));
  if (B.n_srefs) PG_HIP(ctx, hipMemcpyAsync(A->srefs_d, B.srefs.data(), B.n_srefs * sizeof(SeedRef), hipMemcpyHostToDevice, cur_stream(ctx)));
  hipLaunchKernelGGL(anim_slice_kernel, dim3(n_pairs), dim3(256), 0, cur_stream(ctx), A->sqry_d, B.slice_stride, A->slice_d);
  return PG_OK;
}

// roles, seed lists and the seeding kernel's plan for the pairs [0, limit)
static int plan_seeding(Batch& B, uint32_t limit) {
  pg_ctx* ctx = B.ctx;
  assign_mirrors(B, limit);
  std::vector<int32_t> seed_refs, seed_qrys;
  for (uint32_t p = 0; p < limit; ++p)
    if (B.seeded[p]) {
      if (seed_refs.empty() || seed_refs.back() != B.ref_ids[p]) seed_refs.push_back(B.ref_ids[p]);
      seed_qrys.push_back(B.qry_ids[p]);
    }
  std::sort(seed_qrys.begin(), seed_qrys.end());
  seed_qrys.erase(std::unique(seed_qrys.begin(), seed_qrys.end()), seed_qrys.end());
  int rc;
  if ((rc = anim_ensure_lists(ctx, B.A, seed_refs, seed_qrys, B.qstep))) return rc;
  {   // (entries of genomes this batch uses are complete and never change while the genomes are resident; the vector itself
      // may be resized by another worker, so take the pointers under the lock)
    std::lock_guard<std::mutex> lk(ctx->anim_mu);
    B.LSv = anim_lists(ctx)->gidx;
  }
  return B.use_blocks ? plan_seed_blocks(B, limit) : plan_seed_pairs(B, limit, seed_refs);
}

// Seeding: LDS-resident reference groups, streamed query groups; one pass appends (unit, match) records and the per-unit
// counts it leaves are exact even if the buffer overflowed.  Leaves B.cnt and B.total, and the launch cut down to the pairs
// whose matches fit max_matches.
static int seed_stage(Batch& B) {
  pg_ctx* ctx = B.ctx;
  AnimScratch* A = B.A;
  const PgFragArgs* frag = B.frag;
  const int qstep = B.qstep;
  B.mirror.resize(B.n_pairs);
  B.seeded.resize(B.n_pairs);
  B.sqry.resize(B.n_pairs);
  B.slice_stride = B.n_pairs;
  if (!A->lds_attr_set) {   // per context = per device (the attribute is a property of the function ON a device)
    for (const void* fn : {reinterpret_cast<const void*>(anim_seed_kernel<false>), reinterpret_cast<const void*>(anim_seed_kernel<true>),
                           reinterpret_cast<const void*>(anim_seed_pair_kernel<false>), reinterpret_cast<const void*>(anim_seed_pair_kernel<true>)})
      PG_HIP(ctx, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(SEED_MAX_SLOTS * 8 + SEED_STAGE_BYTES)));
    A->lds_attr_set = true;
  }
  // The append buffer of the seed pass and the hit buffers hold the batch budget for a large call (no overflow re-runs), but no more
  // than the call can produce: a pair of genomes cannot have more maximal matches than a quarter of its bases (a one-pair call
  // — smoke(), pg_anim_pair_alignments — used to reserve 3 x 8 GB for a few MB of matches).  Both grow on overflow (below).
  size_t call_bound = 0;
  for (uint32_t p = 0; p < B.n_pairs && call_bound <= B.max_matches; ++p)
    call_bound += (size_t)(ctx->genomes[B.ref_ids[p]].stream_len + ctx->genomes[B.qry_ids[p]].stream_len) / 4 + 8192;
  const size_t budget = call_bound < B.max_matches ? call_bound : (size_t)B.max_matches;
  PG_HIP(ctx, A->seed_total.reserve(2));
  PG_HIP(ctx, A->seedbuf.reserve(budget + 1024));
  B.cnt.resize(B.n_units);
  {   // hit buffer: the matches of the budget plus the chance 16-mer hits of unrelated pairs (~1200 per 5 Mb unit)
    const size_t want = budget + (size_t)(frag ? 8 * 4096 : 4096) * B.n_units + 1024;   // (every position sampled: 5 x the chance hits)
    PG_HIP(ctx, reserve_all(want, want, A->hits_d, A->hits_sorted));
  }
  for (int attempt = 0;; ++attempt) {
    if (attempt == 8) return pg_fail(ctx, PG_E_CAPACITY, "anim seeding: buffers still overflow after repeated splitting");
    const uint32_t n_pairs = B.n_pairs, n_units = B.n_units;
    const size_t hit_room = std::min(A->hits_d.cap, A->hits_sorted.cap);   // (one size: the two grow together)
    const uint32_t hit_cap = (uint32_t)hit_room, seed_cap = (uint32_t)A->seedbuf.cap;
    uint32_t counts[2] = {0, 0};   // matches appended, hits recorded
    int rc;
    if ((rc = plan_seeding(B, n_pairs))) return rc;   // (again after a split: a pair whose partner left the launch is seeded itself)
    if (pg_dev_env("PYANI_SEED_PLAN_LOG"))   // (development: what the plan came to, one line per seeding launch; tests read it)
      fprintf(stderr, "[seed-plan] kernel=%s slots=%u passes=%u launches=%u\n", B.use_blocks ? "block" : "per_pair", B.slots, B.seed_passes,
              B.use_blocks ? B.n_blks : B.n_srefs);
    PG_HIP(ctx, hipMemsetAsync(A->mem_count, 0, n_units * 4, cur_stream(ctx)));
    PG_HIP(ctx, hipMemsetAsync(A->seed_total, 0, 8, cur_stream(ctx)));   // [0] matches, [1] hits
    PG_HIP(ctx, hipMemsetAsync(A->hit_count, 0, n_units * 4, cur_stream(ctx)));
    pg_prof_begin(ctx, PG_K_ANIM_SEED);
    // (the kernels with the pass loop only when the plan needs a second pass somewhere: the hot path keeps its code)
    if (B.use_blocks && B.n_blks)
      hipLaunchKernelGGL(B.seed_passes > 1 ? anim_seed_kernel<true> : anim_seed_kernel<false>, dim3(B.n_blks, SEED_GROUPS), dim3(SEED_BLOCK),
                         (size_t)B.slots * 8 + SEED_STAGE_BYTES, cur_stream(ctx),
                         A->sblk_d, A->sslot_d, A->sbq_d, A->spt_d, B.slots - 1, B.slot_shift, A->hits_d, hit_cap,
                         A->seed_total + 1, A->hit_count, qstep);
    else if (!B.use_blocks && B.n_srefs)
      hipLaunchKernelGGL(B.seed_passes > 1 ? anim_seed_pair_kernel<true> : anim_seed_pair_kernel<false>, dim3(B.n_srefs, SEED_CGROUPS), dim3(SEED_BLOCK),
                         (size_t)B.slots * 8 + SEED_STAGE_BYTES, cur_stream(ctx),
                         A->srefs_d, A->sqry_d, A->slice_d, B.slice_stride, B.slots - 1, A->hits_d, hit_cap, A->seed_total + 1,
                         A->hit_count, qstep);
    pg_prof_end(ctx);
    PG_HIP(ctx, hipGetLastError());   // a rejected launch (LDS size) must not surface only at the end of the batch
    pg_prof_begin(ctx, PG_K_ANIM_HIT);
    // hits -> per-unit slices, then one workgroup per unit verifies / extends them
    hipLaunchKernelGGL(anim_hoff_kernel, dim3(1), dim3(1024), 0, cur_stream(ctx), A->hit_count, n_units, A->hoff, A->hit_cursor);
    hipLaunchKernelGGL(anim_hit_scatter_kernel, dim3((uint32_t)ctx->num_cu * 8u), dim3(256), 0, cur_stream(ctx), A->hits_d, A->seed_total + 1,
                       hit_cap, A->hoff, A->hit_cursor, A->hits_sorted);
    hipLaunchKernelGGL(anim_hit_kernel, dim3(n_units), dim3(256), 0, cur_stream(ctx), A->refs_d, A->units_d, A->hits_sorted, A->hoff,
                       A->seed_total + 1, hit_cap, A->seedbuf, seed_cap, A->seed_total, A->mem_count,
                       frag ? FRAG_SEED_MIN : MIN_MATCH, qstep, B.use_mirror ? A->mirror_d.p : (const int32_t*)nullptr);
    pg_prof_end(ctx);
    PG_HIP(ctx, hipMemcpyAsync(B.cnt.data(), A->mem_count, n_units * 4, hipMemcpyDeviceToHost, cur_stream(ctx)));
    PG_HIP(ctx, hipMemcpyAsync(counts, A->seed_total, 8, hipMemcpyDeviceToHost, cur_stream(ctx)));
    PG_HIP(ctx, hipStreamSynchronize(cur_stream(ctx)));
    B.total = counts[0];
    if (counts[1] > hit_room) {   // hits were dropped: the counts are incomplete -> seed half as many pairs
      if (n_pairs == 1) PG_HIP(ctx, reserve_all((size_t)counts[1] + 1024, (size_t)counts[1] + 1024, A->hits_d, A->hits_sorted));
      else B.set_pairs((n_pairs + 1) / 2);
      continue;
    }
    uint64_t tot = 0, raw = 0;
    uint32_t pairs_fit = 0;
    for (uint32_t p = 0; p < n_pairs; ++p) {
      const uint64_t need = (uint64_t)B.cnt[2 * p] + B.cnt[2 * p + 1] + 4;   // per unit: count + 1 (never empty), rounded up to even
      if (p > 0 && tot + need > B.max_matches) break;
      tot += need;
      raw += need - 4;
      pairs_fit = p + 1;
    }
    B.set_pairs(pairs_fit);
    if (B.total <= A->seedbuf.cap) break;
    // overflow: make room for the prefix of pairs that fits the batch budget (the buffer is made anew at that size, smaller or
    // larger) and seed that prefix again
    A->seedbuf.release();
    PG_HIP(ctx, A->seedbuf.reserve((size_t)(raw + raw / 8 + 1024)));
  }
  return PG_OK;
}

// Every per-match array gets exactly the slice it needs (B.moff: even slice sizes), then the append buffer is dealt into them.
static int scatter_matches(Batch& B) {
  pg_ctx* ctx = B.ctx;
  AnimScratch* A = B.A;
  const uint32_t n_pairs = B.n_pairs, n_units = B.n_units;
  B.moff.assign((size_t)n_units + 1, 0);
  for (uint32_t u = 0; u < n_units; ++u) B.moff[u + 1] = B.moff[u] + ((B.cnt[u] + 2) & ~1u);   // even slice sizes: 8-byte aligned sub-slices
  const size_t M = B.moff[n_units], cap = M + M / 4, held = A->mem.cap;
  PG_HIP(ctx, reserve_all(M, cap, A->mem, A->cm, A->chains, A->order, A->S.alns, A->S.a_rrec, A->S.a_qrec, A->S.idx, A->S.from, A->S.sc));
  PG_HIP(ctx, A->iscratch.reserve(M * 8, cap * 8));
  if (A->mem.cap > held)      // (what pg_api.cpp's anim_match_budget may count as available)
    __atomic_fetch_add(&ctx->anim_scratch_matches_held, (uint64_t)(A->mem.cap - held), __ATOMIC_RELAXED);
  PG_HIP(ctx, hipMemcpyAsync(A->moff, B.moff.data(), ((size_t)n_units + 1) * 4, hipMemcpyHostToDevice, cur_stream(ctx)));
  PG_HIP(ctx, hipMemsetAsync(A->mem_count, 0, n_units * 4, cur_stream(ctx)));
  PG_HIP(ctx, hipMemsetAsync(A->status, 0, n_pairs * 4, cur_stream(ctx)));
  B.O = ClusterOut{A->moff, A->cm, A->chains, A->nch, A->order, A->status};
  pg_prof_begin(ctx, PG_K_ANIM_HIT);
  if (B.total)
    hipLaunchKernelGGL(anim_scatter_kernel, dim3((B.total + 255) / 256), dim3(256), 0, cur_stream(ctx), A->seedbuf, B.total, A->moff, n_units,
                       A->mem_count, A->mem);
  pg_prof_end(ctx);
  return PG_OK;
}

// A3.  Units with >= split_min matches ("big": pairs of related genomes) get their chains from many waves (pga_cluster.inc,
// anim_chain_range_kernel); every other unit is finished by the one wave that filters and clusters it.  Leaves B.nch / B.choff.
static int cluster_stage(Batch& B) {
  pg_ctx* ctx = B.ctx;
  AnimScratch* A = B.A;
  const ClusterOut& O = B.O;
  const uint32_t n_units = B.n_units;
  const int split_min = pg_dev_env("PYANI_ANIM_SPLIT_MIN") ? atoi(pg_dev_env("PYANI_ANIM_SPLIT_MIN")) : 2048;   // (<= 0: never split)
  const int range_entries = pg_dev_env("PYANI_ANIM_RANGE_ENTRIES") && atoi(pg_dev_env("PYANI_ANIM_RANGE_ENTRIES")) > 0
                                ? atoi(pg_dev_env("PYANI_ANIM_RANGE_ENTRIES")) : CHAIN_RANGE_ENTRIES;
  std::vector<BigUnit> big;
  std::vector<uint2> ranges;
  if (split_min > 0)
    for (uint32_t u = 0; u < n_units; ++u)
      if (B.cnt[u] >= (uint32_t)split_min) {
        uint32_t R = B.cnt[u] / (uint32_t)range_entries;
        R = R < 1 ? 1 : (R > (uint32_t)CHAIN_RANGES_MAX ? (uint32_t)CHAIN_RANGES_MAX : R);
        for (uint32_t r = 0; r < R; ++r) ranges.push_back(make_uint2((uint32_t)big.size(), r));
        big.push_back(BigUnit{u, (uint32_t)(ranges.size() - R), R, 0});
      }
  if (!big.empty()) {
    PG_HIP(ctx, A->big_d.reserve(big.size(), big.size() + big.size() / 4));
    PG_HIP(ctx, reserve_all(ranges.size(), ranges.size() + ranges.size() / 4, A->ranges_d, A->range_out));
    PG_HIP(ctx, hipMemcpyAsync(A->big_d, big.data(), big.size() * sizeof(BigUnit), hipMemcpyHostToDevice, cur_stream(ctx)));
    PG_HIP(ctx, hipMemcpyAsync(A->ranges_d, ranges.data(), ranges.size() * sizeof(uint2), hipMemcpyHostToDevice, cur_stream(ctx)));
  }
  const int split_arg = big.empty() ? 0x7fffffff : split_min;
  pg_prof_begin(ctx, PG_K_ANIM_CLUSTER);
  // the front half (MUM filter, union-find, grouping) of a big unit is shared by the PREP_WAVES waves of one workgroup: a
  // single wave needs ~10 ms for the sorts of 50 000 matches, and the launch would wait for the slowest of them (measured
  // on C4, cluster stage per grid: one wave per big unit 1.95 s, workgroup 0.51 s; PYANI_ANIM_WAVE_PREP=1 forces the former)
  const bool prep = !big.empty() && !pg_dev_env("PYANI_ANIM_WAVE_PREP");
  if (prep)
    hipLaunchKernelGGL(anim_cluster_prep_kernel, dim3((uint32_t)big.size()), dim3(PREP_THREADS), 0, cur_stream(ctx), A->refs_d, A->units_d,
                       A->mem, A->mem_count, A->iscratch, O, B.maxmatch, A->big_d);
  hipLaunchKernelGGL(anim_cluster_wave_kernel, dim3(n_units), dim3(64), 0, cur_stream(ctx), A->refs_d, A->units_d, A->mem,
                     A->mem_count, A->iscratch, O, prep ? 1 : 0, B.maxmatch, split_arg);
  if (!big.empty()) {
    hipLaunchKernelGGL(anim_chain_range_kernel, dim3((uint32_t)ranges.size()), dim3(64), 0, cur_stream(ctx), A->units_d, A->mem, A->iscratch,
                       O, A->big_d, A->ranges_d, A->range_out);
    hipLaunchKernelGGL(anim_chain_merge_kernel, dim3((uint32_t)big.size()), dim3(64), 0, cur_stream(ctx), A->refs_d, A->units_d, A->iscratch, O,
                       A->big_d, A->range_out);
  }
  pg_prof_end(ctx);
  B.nch.resize(n_units);
  PG_HIP(ctx, hipMemcpyAsync(B.nch.data(), A->nch, n_units * 4, hipMemcpyDeviceToHost, cur_stream(ctx)));
  PG_HIP(ctx, hipStreamSynchronize(cur_stream(ctx)));
  // (unit, chain) work list, one wave each: offsets by a host prefix over the per-unit chain counts, entries on device
  B.choff.assign((size_t)n_units + 1, 0);
  for (uint32_t u = 0; u < n_units; ++u) B.choff[u + 1] = B.choff[u] + (uint32_t)B.nch[u];
  return PG_OK;
}

// The forced re-alignments of a launch: the request array (short runs from slot 0 up, long ones from slot req_cap - 1 down; their
// counts at cur[PNC_FORCED_N] / cur[PNC_FORCED_LONG]) through the four kernels in turn.  wide: 3 * req_cap slots (the lists handed
// from kernel to kernel); gscratch: forced_scratch_waves(ctx) * PN_GLOBAL_WORDS words.  Called by the batch's extension stage and by
// pg_anim_forced_rects_run (development: caller-chosen rectangles).
static uint32_t forced_scratch_waves(const pg_ctx* ctx) { return (uint32_t)ctx->num_cu * 12u; }   // forced kernels with the LDS store: 12 KiB of LDS each: 12 per CU
static uint32_t diag_only_waves(const pg_ctx* ctx) { return (uint32_t)ctx->num_cu * 32u; }   // gap / forward / backward pre-passes and the narrow forced kernel: no LDS, diagonal engine only, <= 64 registers: 8 per SIMD
static void launch_forced(pg_ctx* ctx, const RefDesc* refs_d, const UnitDesc* units_d, PnForcedReq* reqs, uint32_t req_cap, uint32_t* cur, int32_t* pn_n,
                          uint32_t* gscratch, uint32_t* wide) {
  // narrow bands first (five waves per SIMD), then the runs that asked for a wide one (pga_postnuc.inc, pn_forced_wave)
  const uint32_t pn_waves = forced_scratch_waves(ctx);
  const uint32_t pn_waves_pre = diag_only_waves(ctx);
  const uint32_t win_max = (uint32_t)ctx->anim_pn_window_max, group_max = (uint32_t)ctx->anim_pn_group_max;
  hipLaunchKernelGGL(anim_postnuc_forced_kernel, dim3(pn_waves_pre), dim3(64), 0, cur_stream(ctx), refs_d, units_d, reqs,
                     cur + PNC_FORCED_N, req_cap, cur + PNC_FORCED_CUR, pn_n, wide, cur + PNC_WIDE_N, win_max);
  hipLaunchKernelGGL(anim_postnuc_forced_wide_kernel, dim3(pn_waves), dim3(64), 0, cur_stream(ctx), refs_d, units_d, reqs,
                     cur + PNC_FORCED_N, req_cap, cur + PNC_WIDE_CUR, pn_n, gscratch, wide, cur + PNC_WIDE_N,
                     wide + req_cap, cur + PNC_HUGE_N, win_max);
  // runs whose band spans more than one wave's 2048 diagonals: a workgroup of four waves each (2 workgroups per CU: the 8192-diagonal form holds 242 VGPRs); what the group
  // cannot hold either: the column strips, one wave per run (a list that is empty on every genome workload seen so far)
  hipLaunchKernelGGL(anim_postnuc_forced_huge_kernel, dim3((uint32_t)ctx->num_cu * 2u), dim3(64 * PN_HUGE_WAVES), 0, cur_stream(ctx), refs_d,
                     units_d, reqs, cur + PNC_HUGE_CUR, pn_n, wide + req_cap, cur + PNC_HUGE_N, wide + 2 * (size_t)req_cap,
                     cur + PNC_STRIPS_N, group_max);
  hipLaunchKernelGGL(anim_postnuc_forced_strips_kernel, dim3(pn_waves), dim3(64), 0, cur_stream(ctx), refs_d, units_d, reqs,
                     cur + PNC_STRIPS_CUR, pn_n, gscratch, wide + 2 * (size_t)req_cap, cur + PNC_STRIPS_N);
}

// The match-to-match alignments of a work list of (unit, chain): the small gaps one LANE each by size class (tasks: 4 * task_cap
// slots — three lane classes, then the list the wave engine takes), the rest one wave each; with the lane kernels off
// (PYANI_ANIM_GAP_LANES=0) every gap on the wave engine, which needs gscratch for diag_only_waves(ctx) waves.  cur: the zeroed
// cursor words.  Called by the batch's extension stage and by pg_anim_searches_run (development: caller-chosen gaps).
static void launch_gaps(pg_ctx* ctx, const RefDesc* refs_d, const UnitDesc* units_d, const ClusterOut& O, const uint2* wl, uint32_t n_wl, PnGapTask* tasks,
                        size_t task_cap, uint32_t* cur, pgn::PnGap* gaps, uint32_t* gscratch) {
  const uint32_t pn_waves_pre = diag_only_waves(ctx);
  const int lane_small = ctx->anim_gap_lanes;
  if (lane_small) {     // small gaps: one LANE each, by size class
    hipLaunchKernelGGL(anim_postnuc_gaplist_kernel, dim3((n_wl + 255) / 256), dim3(256), 0, cur_stream(ctx), units_d, O, wl, n_wl, tasks, task_cap,
                       cur + PNC_GAP_LANE);
    const dim3 lg((uint32_t)ctx->num_cu * 8u);
    hipLaunchKernelGGL((anim_postnuc_gaplane_kernel<16>), lg, dim3(64), 0, cur_stream(ctx), refs_d, units_d, O, tasks, cur + PNC_GAP_LANE, gaps);
    hipLaunchKernelGGL((anim_postnuc_gaplane_kernel<32>), lg, dim3(64), 0, cur_stream(ctx), refs_d, units_d, O, tasks + task_cap, cur + PNC_GAP_LANE + 1, gaps);
    hipLaunchKernelGGL((anim_postnuc_gaplane_kernel<PN_SMALL>), lg, dim3(64), 0, cur_stream(ctx), refs_d, units_d, O, tasks + 2 * task_cap, cur + PNC_GAP_LANE + 2, gaps);
  }
  if (lane_small)
    hipLaunchKernelGGL(anim_postnuc_gapbig_kernel, dim3(pn_waves_pre), dim3(64), 0, cur_stream(ctx), refs_d, units_d, O, cur + PNC_GAP_BIG, gaps,
                       tasks + 3 * task_cap, cur + PNC_GAP_WAVE);
  else
    hipLaunchKernelGGL(anim_postnuc_gap_kernel, dim3(pn_waves_pre), dim3(64), 0, cur_stream(ctx), refs_d, units_d, O, wl, n_wl, cur + PNC_GAP_BIG, gaps,
                       gscratch);
}

// A4x: MUMmer's own extension algorithm — the (unit, chain) work list, the pre-passes over it (match-to-match gaps, forward
// extensions, backward searches), the pairs' walks on persistent waves, then the forced re-alignments the walks deferred.
static int extend_stage(Batch& B) {
  pg_ctx* ctx = B.ctx;
  AnimScratch* A = B.A;
  const ClusterOut& O = B.O;
  const uint32_t n_pairs = B.n_pairs, n_units = B.n_units;
  const std::vector<int32_t>& nch = B.nch;
  const size_t M = B.moff[n_units], n_wl = B.choff[n_units];
  const size_t Mp = (M + 15) & ~(size_t)15;
  PG_HIP(ctx, reserve_all(Mp, Mp, A->pn, A->pn_fused, A->pn_gaps, A->pn_fwd, A->pn_bwd, A->pn_tlog, A->pn_born));
  PG_HIP(ctx, A->pn_tasks.reserve(4 * Mp));      // three lane classes + the wave engine's list
  const size_t task_cap = A->pn_tasks.cap / 4;
  PG_HIP(ctx, reserve_all(n_units, (size_t)n_units + n_units / 2, A->pn_n, A->pn_order, A->pn_porder));
  {
    std::vector<uint32_t> uorder(n_units);
    for (uint32_t u = 0; u < n_units; ++u) uorder[u] = u;
    std::stable_sort(uorder.begin(), uorder.end(), [&](uint32_t a, uint32_t b) { return nch[a] > nch[b]; });
    PG_HIP(ctx, hipMemcpyAsync(A->pn_order, uorder.data(), (size_t)n_units * 4, hipMemcpyHostToDevice, cur_stream(ctx)));
    std::vector<uint32_t> porder(n_pairs);      // the walk kernel takes PAIRS (one wave per strand): by the larger strand's cluster count
    for (uint32_t p = 0; p < n_pairs; ++p) porder[p] = p;
    std::stable_sort(porder.begin(), porder.end(), [&](uint32_t a, uint32_t b) { return std::max(nch[2 * a], nch[2 * a + 1]) > std::max(nch[2 * b], nch[2 * b + 1]); });
    PG_HIP(ctx, hipMemcpyAsync(A->pn_porder, porder.data(), (size_t)n_pairs * 4, hipMemcpyHostToDevice, cur_stream(ctx)));
    PG_HIP(ctx, hipStreamSynchronize(cur_stream(ctx)));     // (uorder / porder are locals)
  }
  PG_HIP(ctx, A->pn_cursor.reserve(PNC_WORDS));
  uint32_t* const cur = A->pn_cursor;
  const uint32_t pn_waves = forced_scratch_waves(ctx);
  const uint32_t pn_walk_waves = (uint32_t)ctx->num_cu * 8u;   // the walk / rehearsal kernels: 219 / 173 VGPRs, two waves per SIMD — one persistent wave per resident slot
  const uint32_t pn_waves_pre = diag_only_waves(ctx);
  const uint32_t pn_waves_scr = ctx->anim_gap_lanes ? (pn_waves > pn_walk_waves ? pn_waves : pn_walk_waves) : pn_waves_pre;      // (only the walks, the wide forced kernel and the all-gaps form of the gap kernel use the global scratch)
  PG_HIP(ctx, A->pn_gscratch.reserve((size_t)pn_waves_scr * PN_GLOBAL_WORDS));
  const bool trace = B.trace;      // the walks list their pieces and align everything themselves
  const bool bwd_ahead = ctx->anim_bwd_ahead != 0;
  if (trace) {
    const size_t need = pn_piece_base(Mp, (uint32_t)n_wl, n_units) + 16;
    PG_HIP(ctx, A->pn_pieces.reserve(need));
    PG_HIP(ctx, A->pn_npieces.reserve(n_units, (size_t)n_units + 16));
    PG_HIP(ctx, hipMemsetAsync(A->pn_npieces, 0, (size_t)n_units * 4, cur_stream(ctx)));
  }
  const size_t req_cap = Mp + 16;      // one slot per match slot: a walk records at most one forced run per alignment it starts, and starts at most one per match
  A->pn_req_n = req_cap;
  PG_HIP(ctx, A->pn_reqs.reserve(req_cap, req_cap + req_cap / 2));
  PG_HIP(ctx, A->pn_wide.reserve(3 * req_cap, 3 * (req_cap + req_cap / 2)));
  PG_HIP(ctx, hipMemsetAsync(cur, 0, PNC_WORDS * 4, cur_stream(ctx)));
  if (n_wl && trace) PG_HIP(ctx, hipMemcpyAsync(A->choff_d, B.choff.data(), B.choff.size() * 4, hipMemcpyHostToDevice, cur_stream(ctx)));
  if (n_wl && !trace) {     // the (unit, chain) work list, then every cluster's match-to-match alignments
    PG_HIP(ctx, A->wl_d.reserve(n_wl, n_wl + n_wl / 2));
    PG_HIP(ctx, hipMemcpyAsync(A->choff_d, B.choff.data(), B.choff.size() * 4, hipMemcpyHostToDevice, cur_stream(ctx)));
    hipLaunchKernelGGL(anim_wl_kernel, dim3(n_units), dim3(64), 0, cur_stream(ctx), A->choff_d, A->wl_d);
    pg_prof_begin(ctx, PG_K_ANIM_GAPS);
    launch_gaps(ctx, A->refs_d, A->units_d, O, A->wl_d, (uint32_t)n_wl, A->pn_tasks, task_cap, cur, A->pn_gaps, A->pn_gscratch);
    pg_prof_end(ctx);
    pg_prof_begin(ctx, PG_K_ANIM_FWD);
    hipLaunchKernelGGL(anim_postnuc_fwd_kernel, dim3(pn_waves_pre), dim3(64), 0, cur_stream(ctx), A->refs_d, A->units_d, O, A->wl_d, (uint32_t)n_wl,
                       cur + PNC_FWD, A->pn_fwd, A->pn_gscratch);
    pg_prof_end(ctx);
    pg_prof_begin(ctx, PG_K_ANIM_BWD);
    if (bwd_ahead) {     // the walks rehearsed without their backward searches, then the searches they predict, one wave each
      PG_HIP(ctx, hipMemsetAsync(A->pn_bwd, 0, (size_t)M * sizeof(pgn::PnBwd), cur_stream(ctx)));
      hipLaunchKernelGGL(anim_postnuc_rehearse_kernel, dim3(pn_walk_waves < n_units ? pn_walk_waves : n_units), dim3(64), 0, cur_stream(ctx), A->refs_d,
                         A->units_d, n_units, O, cur + PNC_REHEARSE, A->pn, A->pn_fused, A->pn_gscratch, A->pn_gaps, A->pn_fwd, A->pn_order, A->pn_bwd);
      hipLaunchKernelGGL(anim_postnuc_bwd_kernel, dim3(pn_waves_pre), dim3(64), 0, cur_stream(ctx), A->refs_d, A->units_d, O, A->wl_d, (uint32_t)n_wl,
                         cur + PNC_BWD, A->pn_bwd, A->pn_gscratch);
    }
    pg_prof_end(ctx);
  }
  pg_prof_begin(ctx, PG_K_ANIM_EXTEND);
  if (n_wl)
    hipLaunchKernelGGL(anim_postnuc_kernel, dim3(pn_walk_waves / 2 < n_pairs ? pn_walk_waves / 2 : n_pairs), dim3(128), 0, cur_stream(ctx), A->refs_d, A->units_d,
                       n_pairs, O, cur + PNC_UNIT, A->pn, A->pn_fused, A->pn_n, A->pn_gscratch, A->pn_reqs, cur + PNC_FORCED_N, (uint32_t)req_cap,
                       trace ? nullptr : A->pn_gaps.p, trace ? nullptr : A->pn_fwd.p, A->pn_porder, trace ? A->pn_pieces.p : nullptr, A->pn_npieces, A->choff_d,
                       bwd_ahead && !trace ? A->pn_bwd.p : nullptr, A->pn_tlog, A->pn_born);
  else
    PG_HIP(ctx, hipMemsetAsync(A->pn_n, 0, (size_t)n_units * 4, cur_stream(ctx)));
  pg_prof_end(ctx);
  pg_prof_begin(ctx, PG_K_ANIM_EXTLANE);     // (the forced re-alignments, deferred: pga_postnuc.inc)
  if (n_wl) launch_forced(ctx, A->refs_d, A->units_d, A->pn_reqs, (uint32_t)req_cap, cur, A->pn_n, A->pn_gscratch, A->pn_wide);
  pg_prof_end(ctx);
  return PG_OK;
}

// Development (pg_anim_forced_rects): caller-chosen rectangles through launch_forced, the product's own forced launches.  The
// descriptors are a batch's (one RefDesc; UnitDesc per rectangle, all of the same query strand: a unit entry of its own is what
// tells a failed rectangle from its neighbours, the flag being per unit), the request array is filled with forced_errors' split
// (sum of sides > 1500: from the back), every rectangle has a zeroed PnAln of its own as dst.  Ids, strand and pointers were checked
// by the caller; the rectangles are checked here: a side is at most what the walk hands one engine call (MAX_ALIGNMENT_LENGTH).
int pg_anim_forced_rects_run(pg_ctx* ctx, int32_t ref_id, int32_t qry_id, int strand, uint32_t n, const int32_t* rects, int32_t* errors,
                             int32_t* w_used, int32_t* status) {
  const PgGenome& G = ctx->genomes[ref_id];
  const PgGenome& H = ctx->genomes[qry_id];
  for (uint32_t i = 0; i < n; ++i) {
    const int64_t A0 = rects[4 * i], A1 = rects[4 * i + 1], B0 = rects[4 * i + 2], B1 = rects[4 * i + 3];
    const int64_t N = A1 - A0 + 1, M = B1 - B0 + 1;
    if (N < 1 || M < 1) return pg_fail(ctx, PG_E_ARG, "pg_anim_forced_rects: a rectangle with a side below 1");
    if (A0 < 0 || A1 >= (int64_t)G.stream_len || B0 < 0 || B1 >= (int64_t)H.stream_len) return pg_fail(ctx, PG_E_ARG, "pg_anim_forced_rects: a rectangle outside its stream");
    if (N > pgn::MAX_ALIGNMENT_LENGTH || M > pgn::MAX_ALIGNMENT_LENGTH)
      return pg_fail(ctx, PG_E_ARG, "pg_anim_forced_rects: a side longer than one engine call aligns (MAX_ALIGNMENT_LENGTH)");
  }
  AnimScratch* A = anim_scratch(ctx);
  (void)hipGetLastError();
  RefDesc ref{ctx->d_codes + G.arena_start / 16, ctx->d_mask + G.arena_start / 32, (int32_t)G.stream_len, nullptr, 0};
  std::vector<UnitDesc> units(n, UnitDesc{ctx->d_codes + H.arena_start / 16, ctx->d_mask + H.arena_start / 32, (int32_t)H.stream_len, nullptr, 0, strand, 0, 0});
  PgDevBuf<RefDesc> refs_d;
  PgDevBuf<UnitDesc> units_d;
  PgDevBuf<PnForcedReq> reqs_d;
  PgDevBuf<pgn::PnAln> dst_d;
  PgDevBuf<int32_t> pn_n_d;
  PgDevBuf<uint32_t> wide_d, cur_d;
  const uint32_t req_cap = n;
  PG_HIP(ctx, refs_d.reserve(1));
  PG_HIP(ctx, reserve_all(n, n, units_d, reqs_d, dst_d, pn_n_d));
  PG_HIP(ctx, wide_d.reserve(3 * (size_t)req_cap));
  PG_HIP(ctx, cur_d.reserve(PNC_WORDS));
  PG_HIP(ctx, A->pn_gscratch.reserve((size_t)forced_scratch_waves(ctx) * PN_GLOBAL_WORDS));
  std::vector<PnForcedReq> reqs(req_cap);
  std::vector<uint32_t> slot_of(n);
  uint32_t cur[PNC_WORDS] = {0};
  for (uint32_t i = 0; i < n; ++i) {
    const int32_t A0 = rects[4 * i], A1 = rects[4 * i + 1], B0 = rects[4 * i + 2], B1 = rects[4 * i + 3];
    const bool big = (A1 - A0) + (B1 - B0) > 1500;
    const uint32_t at = big ? cur[PNC_FORCED_LONG]++ : cur[PNC_FORCED_N]++;
    slot_of[i] = big ? req_cap - 1 - at : at;
    reqs[slot_of[i]] = PnForcedReq{A0, A1, B0, B1, i, 0, dst_d.p + i};
  }
  hipStream_t st = cur_stream(ctx);
  PG_HIP(ctx, hipMemcpyAsync(refs_d, &ref, sizeof(ref), hipMemcpyHostToDevice, st));
  PG_HIP(ctx, hipMemcpyAsync(units_d, units.data(), (size_t)n * sizeof(UnitDesc), hipMemcpyHostToDevice, st));
  PG_HIP(ctx, hipMemcpyAsync(reqs_d, reqs.data(), (size_t)n * sizeof(PnForcedReq), hipMemcpyHostToDevice, st));
  PG_HIP(ctx, hipMemcpyAsync(cur_d, cur, sizeof(cur), hipMemcpyHostToDevice, st));
  PG_HIP(ctx, hipMemsetAsync(dst_d, 0, (size_t)n * sizeof(pgn::PnAln), st));
  PG_HIP(ctx, hipMemsetAsync(pn_n_d, 0, (size_t)n * 4, st));
  launch_forced(ctx, refs_d, units_d, reqs_d, req_cap, cur_d, pn_n_d, A->pn_gscratch, wide_d);
  PG_HIP(ctx, hipGetLastError());
  std::vector<pgn::PnAln> dst(n);
  std::vector<int32_t> pn_n(n);
  PG_HIP(ctx, hipMemcpyAsync(reqs.data(), reqs_d, (size_t)n * sizeof(PnForcedReq), hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipMemcpyAsync(dst.data(), dst_d, (size_t)n * sizeof(pgn::PnAln), hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipMemcpyAsync(pn_n.data(), pn_n_d, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipStreamSynchronize(st));
  for (uint32_t i = 0; i < n; ++i) {
    const bool failed = pn_n[i] < 0;      // the unit flag: the corner stayed unreachable, or no engine held the run
    status[i] = failed ? 2 : 0;
    errors[i] = failed ? 0 : dst[i].errors;
    w_used[i] = failed ? 0 : reqs[slot_of[i]].w;
  }
  return PG_OK;
}

// Development (pg_anim_searches): caller-chosen trimmed searches (A0, B0, tA, tB, m_o) of one (reference, query strand) on the engine
// asked for.  Ids, strand, engine and pointers were checked by the caller; the searches are checked here, next to the engines' limits.
// PREPASS / WALK / RUNG_*: anim_postnuc_searches_kernel, one wave per search (PREPASS: one launch per pre-pass kernel, with that
// kernel's cursor chunk — match-to-match gaps 8, forward extensions 4, backward searches 8).  LANES: every search a chain of two
// one-base matches (start, target) in a ClusterOut of one unit, through launch_gaps — the batch's own launches; a gap no kernel
// answered comes back as held = 0.  out[5 n]: endA, endB, errors, reached, held.
int pg_anim_searches_run(pg_ctx* ctx, int32_t ref_id, int32_t qry_id, int strand, int engine, uint32_t n, const int32_t* searches, int32_t* out) {
  const PgGenome& G = ctx->genomes[ref_id];
  const PgGenome& H = ctx->genomes[qry_id];
  std::vector<PnSearchReq> reqs(n);
  for (uint32_t i = 0; i < n; ++i) {
    const int64_t A0 = searches[5 * i], B0 = searches[5 * i + 1], tA = searches[5 * i + 2], tB = searches[5 * i + 3];
    const unsigned m_o = (unsigned)searches[5 * i + 4];
    if (m_o & pgn::FORCED_BIT) return pg_fail(ctx, PG_E_ARG, "pg_anim_searches: a forced run (FORCED_BIT) is not a search: pg_anim_forced_rects has those");
    if (m_o != pgn::FORWARD_ALIGN && m_o != (pgn::FORWARD_ALIGN | pgn::OPTIMAL_BIT) && m_o != pgn::BACKWARD_SEARCH && m_o != (pgn::BACKWARD_SEARCH | pgn::OPTIMAL_BIT))
      return pg_fail(ctx, PG_E_ARG, "pg_anim_searches: m_o must be FORWARD_ALIGN or BACKWARD_SEARCH, with or without OPTIMAL_BIT");
    if (engine == PN_SEARCH_LANES && m_o != pgn::FORWARD_ALIGN) return pg_fail(ctx, PG_E_ARG, "pg_anim_searches: LANES takes FORWARD_ALIGN searches only (match-to-match gaps)");
    if (A0 < 0 || A0 >= (int64_t)G.stream_len || tA < 0 || tA >= (int64_t)G.stream_len || B0 < 0 || B0 >= (int64_t)H.stream_len || tB < 0 || tB >= (int64_t)H.stream_len)
      return pg_fail(ctx, PG_E_ARG, "pg_anim_searches: a position outside its stream");
    const bool fwd = m_o & pgn::DIRECTION_BIT;
    const int64_t N = fwd ? tA - A0 + 1 : A0 - tA + 1, M = fwd ? tB - B0 + 1 : B0 - tB + 1;
    if (N < 1 || M < 1) return pg_fail(ctx, PG_E_ARG, "pg_anim_searches: a target on the wrong side of the start for the direction");
    if (N > pgn::MAX_ALIGNMENT_LENGTH || M > pgn::MAX_ALIGNMENT_LENGTH)
      return pg_fail(ctx, PG_E_ARG, "pg_anim_searches: a side longer than one engine call aligns (MAX_ALIGNMENT_LENGTH)");
    reqs[i] = PnSearchReq{(int32_t)A0, (int32_t)B0, (int32_t)tA, (int32_t)tB, m_o};
  }
  if (engine == PN_SEARCH_LANES && !ctx->anim_gap_lanes) return pg_fail(ctx, PG_E_ARG, "pg_anim_searches: LANES with the lane kernels switched off (PYANI_ANIM_GAP_LANES=0)");
  AnimScratch* A = anim_scratch(ctx);
  (void)hipGetLastError();
  const RefDesc ref{ctx->d_codes + G.arena_start / 16, ctx->d_mask + G.arena_start / 32, (int32_t)G.stream_len, nullptr, 0};
  const UnitDesc unit{ctx->d_codes + H.arena_start / 16, ctx->d_mask + H.arena_start / 32, (int32_t)H.stream_len, nullptr, 0, strand, 0, 0};
  PgDevBuf<RefDesc> refs_d;
  PgDevBuf<UnitDesc> units_d;
  PgDevBuf<uint32_t> cur_d;
  PG_HIP(ctx, refs_d.reserve(1));
  PG_HIP(ctx, units_d.reserve(1));
  PG_HIP(ctx, cur_d.reserve(PNC_WORDS));
  hipStream_t st = cur_stream(ctx);
  PG_HIP(ctx, hipMemcpyAsync(refs_d, &ref, sizeof(ref), hipMemcpyHostToDevice, st));
  PG_HIP(ctx, hipMemcpyAsync(units_d, &unit, sizeof(unit), hipMemcpyHostToDevice, st));
  PG_HIP(ctx, hipMemsetAsync(cur_d, 0, PNC_WORDS * 4, st));
  if (engine == PN_SEARCH_LANES) {
    // the chains: matches 2 i (the start base) and 2 i + 1 (the target base) of chain i, the gap's answer at match slot 2 i
    std::vector<Match> cm(2 * (size_t)n);
    std::vector<Chain> chains(2 * (size_t)n, Chain{0, 0, strand, 0, 0});
    std::vector<uint2> wl(n);
    for (uint32_t i = 0; i < n; ++i) {
      cm[2 * i] = Match{reqs[i].A0, reqs[i].B0, 1, strand};
      cm[2 * i + 1] = Match{reqs[i].tA, reqs[i].tB, 1, strand};
      chains[i] = Chain{(int32_t)(2 * i), 2, strand, 0, 0};
      wl[i] = make_uint2(0u, i);
    }
    const uint32_t moff[2] = {0u, 2 * n};
    PgDevBuf<uint32_t> moff_d;
    PgDevBuf<Match> cm_d;
    PgDevBuf<Chain> chains_d;
    PgDevBuf<uint2> wl_d;
    PgDevBuf<PnGapTask> tasks_d;
    PgDevBuf<pgn::PnGap> gaps_d;
    const size_t task_cap = n;
    PG_HIP(ctx, moff_d.reserve(2));
    PG_HIP(ctx, reserve_all(2 * (size_t)n, 2 * (size_t)n, cm_d, chains_d, gaps_d));
    PG_HIP(ctx, wl_d.reserve(n));
    PG_HIP(ctx, tasks_d.reserve(4 * task_cap));
    PG_HIP(ctx, hipMemcpyAsync(moff_d, moff, sizeof(moff), hipMemcpyHostToDevice, st));
    PG_HIP(ctx, hipMemcpyAsync(cm_d, cm.data(), cm.size() * sizeof(Match), hipMemcpyHostToDevice, st));
    PG_HIP(ctx, hipMemcpyAsync(chains_d, chains.data(), chains.size() * sizeof(Chain), hipMemcpyHostToDevice, st));
    PG_HIP(ctx, hipMemcpyAsync(wl_d, wl.data(), wl.size() * sizeof(uint2), hipMemcpyHostToDevice, st));
    PG_HIP(ctx, hipMemsetAsync(gaps_d, 0xFF, 2 * (size_t)n * sizeof(pgn::PnGap), st));      // reached = -1: not answered
    const ClusterOut O{moff_d, cm_d, chains_d, nullptr, nullptr, nullptr};
    launch_gaps(ctx, refs_d, units_d, O, wl_d, n, tasks_d, task_cap, cur_d, gaps_d, nullptr);
    PG_HIP(ctx, hipGetLastError());
    std::vector<pgn::PnGap> gaps(2 * (size_t)n);
    PG_HIP(ctx, hipMemcpyAsync(gaps.data(), gaps_d, gaps.size() * sizeof(pgn::PnGap), hipMemcpyDeviceToHost, st));
    PG_HIP(ctx, hipStreamSynchronize(st));
    for (uint32_t i = 0; i < n; ++i) {
      const pgn::PnGap& g = gaps[2 * i];
      const bool held = g.reached >= 0;
      int32_t* o = out + 5 * (size_t)i;
      o[0] = held ? g.eA : 0; o[1] = held ? g.eB : 0; o[2] = held ? g.errors : 0; o[3] = held ? g.reached : 0; o[4] = held ? 1 : 0;
    }
    return PG_OK;
  }
  // the lists: one for every engine but PREPASS, which takes its searches as the three pre-pass kernels would (cursor chunks 8 / 4 / 8)
  std::vector<uint32_t> list;
  uint32_t first[4] = {0u, 0u, 0u, 0u};
  const uint32_t chunk_of[3] = {8u, 4u, 8u};
  const int n_lists = engine == PN_SEARCH_PREPASS ? 3 : 1;
  for (int l = 0; l < n_lists; ++l) {
    for (uint32_t i = 0; i < n; ++i) {
      const unsigned m_o = reqs[i].m_o;
      const int cls = !(m_o & pgn::DIRECTION_BIT) ? 2 : (m_o & pgn::OPTIMAL_BIT) ? 1 : 0;
      if (n_lists == 1 || cls == l) list.push_back(i);
    }
    first[l + 1] = (uint32_t)list.size();
  }
  const bool scratch = engine == PN_SEARCH_WALK || engine == PN_SEARCH_RUNG_GLOBAL;
  const uint32_t max_waves = scratch ? (uint32_t)ctx->num_cu * 8u : diag_only_waves(ctx);
  PgDevBuf<PnSearchReq> reqs_d;
  PgDevBuf<PnSearchOut> out_d;
  PgDevBuf<uint32_t> list_d;
  PG_HIP(ctx, reqs_d.reserve(n));
  PG_HIP(ctx, out_d.reserve(n));
  PG_HIP(ctx, list_d.reserve(n));
  if (scratch) PG_HIP(ctx, A->pn_gscratch.reserve((size_t)(n < max_waves ? n : max_waves) * PN_GLOBAL_WORDS));
  PG_HIP(ctx, hipMemcpyAsync(reqs_d, reqs.data(), (size_t)n * sizeof(PnSearchReq), hipMemcpyHostToDevice, st));
  PG_HIP(ctx, hipMemcpyAsync(list_d, list.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
  PG_HIP(ctx, hipMemsetAsync(out_d, 0, (size_t)n * sizeof(PnSearchOut), st));
  for (int l = 0; l < n_lists; ++l) {
    const uint32_t nl = first[l + 1] - first[l];
    if (!nl) continue;
    const uint32_t chunk = engine == PN_SEARCH_PREPASS ? chunk_of[l] : 1u;
    const uint32_t turns = (nl + chunk - 1) / chunk;
    hipLaunchKernelGGL(anim_postnuc_searches_kernel, dim3(turns < max_waves ? turns : max_waves), dim3(64), 0, st, refs_d, units_d, reqs_d, list_d + first[l],
                       nl, chunk, engine, cur_d + l, out_d, scratch ? A->pn_gscratch.p : nullptr);
  }
  PG_HIP(ctx, hipGetLastError());
  std::vector<PnSearchOut> res(n);
  PG_HIP(ctx, hipMemcpyAsync(res.data(), out_d, (size_t)n * sizeof(PnSearchOut), hipMemcpyDeviceToHost, st));
  PG_HIP(ctx, hipStreamSynchronize(st));
  for (uint32_t i = 0; i < n; ++i) {
    int32_t* o = out + 5 * (size_t)i;
    o[0] = res[i].eA; o[1] = res[i].eB; o[2] = res[i].errors; o[3] = res[i].reached; o[4] = res[i].held;
  }
  return PG_OK;
}

// PYANI_PN_STATS (development): what the engines did in this launch
static int print_pn_stats(pg_ctx* ctx) {
  PG_HIP(ctx, hipStreamSynchronize(cur_stream(ctx)));
  unsigned long long st[32], zero[32] = {0};
  PG_HIP(ctx, hipMemcpyFromSymbol(st, HIP_SYMBOL(g_pn_stats), sizeof(st)));
  PG_HIP(ctx, hipMemcpyToSymbol(HIP_SYMBOL(g_pn_stats), zero, sizeof(zero)));
  fprintf(stderr, "[pn-stats] units %llu clusters %llu | regs: calls %llu steps %llu cells %llu moves %llu overflows %llu | lds: calls %llu steps %llu cells %llu | "
                  "global: calls %llu steps %llu cells %llu\n", st[11], st[12], st[0], st[1], st[2], st[9], st[10], st[3], st[4], st[5], st[6], st[7], st[8]);
  fprintf(stderr, "[pn-stats] searches of the gap + units kernels: %llu calls, %.1f ms inside the engine (summed over waves); shadow tests that asked for the synteny's current alignment: %llu\n", st[22], st[21] / 1e5, st[31]);
  fprintf(stderr, "[pn-stats] forced passes by engine (127 / 255 / 511 cells / strips): %llu %llu %llu %llu passes, %.1f %.1f %.1f %.1f ms summed over waves\n",
          st[27], st[28], st[29], st[30], st[23] / 1e5, st[24] / 1e5, st[25] / 1e5, st[26] / 1e5);
  {
    unsigned long long ks[32], kz[32] = {0};
    PG_HIP(ctx, hipMemcpyFromSymbol(ks, HIP_SYMBOL(g_pn_kstats), sizeof(ks)));
    PG_HIP(ctx, hipMemcpyToSymbol(HIP_SYMBOL(g_pn_kstats), kz, sizeof(kz)));
    const char* kn[8] = {"gaps", "forward", "backward-ahead", "walks", "forced narrow", "forced 512-1024", "forced 2048", "forced group 8192"};
    for (int k = 0; k < 8; ++k)
      fprintf(stderr, "[pn-stats] diagonal engine in %-16s: %llu calls, %llu anti-diagonals, %llu cells\n", kn[k], ks[4 * k], ks[4 * k + 1], ks[4 * k + 2]);
    fprintf(stderr, "[pn-stats] walk kernel scans: shadow test %.1f ms over %llu rows of 64 alignments, reverse-target search %.1f ms in %llu calls (summed over waves)\n",
            ks[3] / 1e5, ks[7], ks[11] / 1e5, ks[15]);
    fprintf(stderr, "[pn-stats] run-ahead results the walk took: forward %llu of %llu computed (%.4f), backward %llu found ready of %llu searches run ahead; %llu searches left to the walk itself\n",
            ks[19], ks[4], ks[4] ? (double)ks[19] / (double)ks[4] : 0.0, ks[23], ks[8], ks[12]);
  }
  for (int k = 13; k <= 17; k += 4)      // ticks of the 100 MHz wall clock -> ms
    fprintf(stderr, "[pn-stats] %s: busy %.1f ms summed over waves, span %.1f ms, longest item %.1f ms (size %llu)\n", k == 13 ? "units" : "forced",
            st[k] / 1e5, st[k + 2] ? (st[k + 2] - ~st[k + 3]) / 1e5 : 0.0, (st[k + 1] >> 20) / 1e5, st[k + 1] & 0xFFFFFull);
  return PG_OK;
}

// A5 and the results: the pairs' pg_anim_result, and their alignment records when the calling thread has set a sink
static int finish_stage(Batch& B, pg_anim_result* out_host) {
  pg_ctx* ctx = B.ctx;
  AnimScratch* A = B.A;
  int rc;
  pg_prof_begin(ctx, PG_K_ANIM_FINISH);
  hipLaunchKernelGGL(anim_finish_kernel, dim3(B.n_pairs), dim3(64), 0, cur_stream(ctx), A->refs_d, A->units_d, B.n_pairs,
                     B.O, A->pn, A->pn_n, A->S.view(), B.filter_1to1, A->out);
  pg_prof_end(ctx);
  PG_HIP(ctx, hipGetLastError());
  PG_HIP(ctx, hipMemcpyAsync(out_host, A->out, B.n_pairs * sizeof(pg_anim_result), hipMemcpyDeviceToHost, cur_stream(ctx)));
  PG_HIP(ctx, hipStreamSynchronize(cur_stream(ctx)));
  if (tls_sink && (rc = anim_collect(ctx, A, B.ref_ids, B.qry_ids, B.n_pairs, out_host, B.choff, *tls_sink))) return rc;
  return PG_OK;
}

// One batch of ordered pairs (ref_ids grouped).  The seed pass appends every unit's matches to one buffer and counts them
// per (pair, strand) unit; a scatter then gives every per-match array exactly the slice it needs, which is what lets
// thousands of units be in flight at once within the HBM budget.
// If the batch needs more than max_matches, only its first n_done pairs are processed (the caller continues from there).
int pg_anim_run_batch(pg_ctx* ctx, const int32_t* ref_ids, const int32_t* qry_ids, uint32_t n_pairs, int filter_1to1, int maxmatch,
                      uint64_t max_matches, pg_anim_result* out_host, uint32_t* n_done, const PgFragArgs* frag) {
  Batch B{ctx, anim_scratch(ctx), ref_ids, qry_ids, frag, filter_1to1, maxmatch, max_matches};
  int rc;
  (void)hipGetLastError();   // launch checks below must only see this batch's errors
  B.set_pairs(n_pairs);
  if (frag) frag_limit_pairs(B);
  B.qstep = frag ? FRAG_QSTEP : SEED_STEP;
  B.use_mirror = !frag && !pg_dev_env("PYANI_ANIM_NO_MIRROR");
  // Seeding kernel: ANIm uses the block kernel (anim_seed_kernel); fragment mode — and ANIm under the development switch
  // PYANI_SEED_PER_PAIR=1, which tests hold against it — the per-pair kernel (anim_seed_pair_kernel).  PYANI_SEED_BLOCK_SLOTS
  // (development): the table size a block is planned for (default SEED_MAX_SLOTS).  PYANI_SEED_MAX_SLOTS (development): the
  // largest table either kernel may use, a power of two from 256 to SEED_MAX_SLOTS (anything else is ignored); blocks are planned
  // for the smaller of the two.  It lets tests force passes (pg_seed_plan.h) on genomes of a few hundred kb.  PYANI_SEED_PLAN_LOG
  // (development): seed_stage prints the planned kernel, table size and pass count of every seeding launch to stderr.
  B.use_blocks = !frag && !(pg_dev_env("PYANI_SEED_PER_PAIR") && atoi(pg_dev_env("PYANI_SEED_PER_PAIR")) == 1);
  if (pg_dev_env("PYANI_SEED_BLOCK_SLOTS")) {
    const int want = atoi(pg_dev_env("PYANI_SEED_BLOCK_SLOTS"));
    B.blk_slots = want >= 512 && want <= (int)SEED_MAX_SLOTS ? (uint32_t)want : SEED_MAX_SLOTS;
  }
  if (pg_dev_env("PYANI_SEED_MAX_SLOTS")) {
    const int want = atoi(pg_dev_env("PYANI_SEED_MAX_SLOTS"));
    if (want >= 256 && want <= (int)SEED_MAX_SLOTS && (want & (want - 1)) == 0) B.max_slots = (uint32_t)want;
  }
  if (B.blk_slots > B.max_slots) B.blk_slots = B.max_slots;
  B.trace = tls_sink && tls_sink->with_indels;
  if ((rc = build_descriptors(B))) return rc;
  if ((rc = seed_stage(B))) return rc;
  *n_done = B.n_pairs;
  if ((rc = scatter_matches(B))) return rc;
  if (frag) {   // fragment mode: the matches of every unit are in place; the rest of the batch is the fragment kernels
    PG_HIP(ctx, hipGetLastError());
    return anib_frag_stage(ctx, B.A, qry_ids, B.n_pairs, B.cnt, *frag, B.ref_list, B.ref_of_pair);
  }
  if ((rc = cluster_stage(B))) return rc;
  if ((rc = extend_stage(B))) return rc;
  if (pg_dev_env("PYANI_PN_STATS") && (rc = print_pn_stats(ctx))) return rc;
  return finish_stage(B, out_host);
}

// Fragment mode after seeding: A->mem / A->moff / A->mem_count hold every unit's exact matches (>= 16, sampled), A->units_d /
// A->refs_d the descriptors.  Builds the fragment tables of the batch's query genomes, runs F1-F3 (pga_frag.inc), returns
// the pair results (and, optionally, the rows of pair 0, or — with a sink — the rows of every pair, packed on the device).
// The word index of one genome (pga_frag.inc), built once and kept with its seed lists.
static int anib_ensure_word_index(pg_ctx* ctx, AnimScratch* A, int32_t gid) {
  std::lock_guard<std::mutex> lk(ctx->anim_mu);
  AnimLists* LS = anim_lists(ctx);
  if (LS->gidx.size() < ctx->genomes.size()) LS->gidx.resize(ctx->genomes.size());
  GenomeIdx& X = LS->gidx[gid];
  if (X.word_start) return PG_OK;
  const PgGenome& G = ctx->genomes[gid];
  const int32_t len = (int32_t)G.stream_len;
  const uint32_t* codes = ctx->d_codes + G.arena_start / 16;
  const uint32_t* mask = ctx->d_mask + G.arena_start / 32;
  PgDevBuf<uint32_t> start;      // locals until the index is complete: every earlier exit frees them
  PgDevBuf<int32_t> pos;
  PG_HIP(ctx, A->fr_wtmp.reserve((size_t)WORD_BUCKETS + 1024 + 16));   // fill cursors | block sums
  PG_HIP(ctx, start.reserve((size_t)WORD_BUCKETS + 1));
  PG_HIP(ctx, pos.reserve((size_t)(len > 0 ? len : 1)));
  hipStream_t st = cur_stream(ctx);
  const uint32_t grid = (uint32_t)((len + 255) / 256);
  hipError_t e = hipMemsetAsync(start, 0, ((size_t)WORD_BUCKETS + 1) * 4, st);
  if (e == hipSuccess && grid) hipLaunchKernelGGL(anib_word_count_kernel, dim3(grid), dim3(256), 0, st, codes, mask, len, start, pos, 0);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(anib_word_scan1_kernel, dim3(WORD_BUCKETS / 4096u), dim3(1024), 0, st, start, A->fr_wtmp + WORD_BUCKETS);
    hipLaunchKernelGGL(anib_word_scan2_kernel, dim3(1), dim3(1024), 0, st, A->fr_wtmp + WORD_BUCKETS, WORD_BUCKETS / 4096u, start + WORD_BUCKETS);
    hipLaunchKernelGGL(anib_word_scan3_kernel, dim3(WORD_BUCKETS / 1024u), dim3(1024), 0, st, start, A->fr_wtmp + WORD_BUCKETS, A->fr_wtmp);
    if (grid) hipLaunchKernelGGL(anib_word_count_kernel, dim3(grid), dim3(256), 0, st, codes, mask, len, A->fr_wtmp, pos, 1);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return pg_fail(ctx, PG_E_HIP, hipGetErrorString(e));
  X.word_start = LS->adopt(start); X.word_pos = LS->adopt(pos);     // published complete
  return PG_OK;
}

static int anib_frag_stage(pg_ctx* ctx, AnimScratch* A, const int32_t* qry_ids, uint32_t n_pairs, const std::vector<uint32_t>& cnt,
                           const PgFragArgs& F, const std::vector<int32_t>& ref_list, const std::vector<uint32_t>& ref_of_pair) {
  int rc;
  const uint32_t n_units = 2 * n_pairs;
  // fragment tables, one per distinct query genome
  std::vector<int32_t> tables;
  struct Tab { size_t pos, len, rec0; int32_t n_frags; };
  std::vector<Tab> tab_of(ctx->genomes.size(), Tab{0, 0, 0, -1});
  std::vector<FragPair> fp(n_pairs);
  std::vector<size_t> tab_ref(n_pairs);
  uint64_t slots = 0;
  for (uint32_t p = 0; p < n_pairs; ++p) {
    const int32_t gid = qry_ids[p];
    Tab& T = tab_of[gid];
    if (T.n_frags < 0) {
      const PgGenome& Q = ctx->genomes[gid];
      std::vector<int32_t> pos, len, rec0;
      for (uint32_t r = 0; r < Q.n_rec; ++r) {
        rec0.push_back((int32_t)pos.size());
        const int32_t r0 = Q.rec_start[r], r1 = Q.rec_start[r + 1] - 1;
        for (int32_t f0 = r0; f0 < r1; f0 += F.fragsize) { pos.push_back(f0); len.push_back(r1 - f0 < F.fragsize ? r1 - f0 : F.fragsize); }
      }
      T.n_frags = (int32_t)pos.size();
      T.pos = tables.size(); tables.insert(tables.end(), pos.begin(), pos.end());
      T.len = tables.size(); tables.insert(tables.end(), len.begin(), len.end());
      T.rec0 = tables.size(); tables.insert(tables.end(), rec0.begin(), rec0.end());
    }
    fp[p].n_frags = T.n_frags;
    fp[p].slot0 = (uint32_t)slots;
    slots += (uint64_t)T.n_frags;
  }
  if (slots >= (1ull << 31)) return pg_fail(ctx, PG_E_CAPACITY, "fragment mode: too many (pair, fragment) slots in one launch");
  PG_HIP(ctx, A->fr_tables.reserve(tables.size() + 1, tables.size() + 1024));
  for (uint32_t p = 0; p < n_pairs; ++p) {
    const Tab& T = tab_of[qry_ids[p]];
    fp[p].frag_pos = A->fr_tables + T.pos; fp[p].frag_len = A->fr_tables + T.len; fp[p].rec_frag0 = A->fr_tables + T.rec0;
  }
  PG_HIP(ctx, A->fr_pairs.reserve(n_pairs));
  PG_HIP(ctx, A->fr_out.reserve(n_pairs));
  PG_HIP(ctx, A->fr_ebase.reserve(n_units));
  const size_t n_off = 2 * (size_t)slots + 2 * (size_t)n_pairs;
  PG_HIP(ctx, A->fr_off.reserve(n_off, n_off + n_off / 4));
  {
    const size_t cap = (size_t)slots + (size_t)slots / 4;
    PG_HIP(ctx, reserve_all((size_t)slots, cap, A->fr_slot_pair, A->fr_nrows));
    PG_HIP(ctx, A->fr_rows.reserve((size_t)slots * FRAG_ROWS, cap * FRAG_ROWS));
  }
  std::vector<uint32_t> slot_pair((size_t)slots);
  for (uint32_t p = 0; p < n_pairs; ++p) std::fill(slot_pair.begin() + fp[p].slot0, slot_pair.begin() + fp[p].slot0 + fp[p].n_frags, p);
  // a match is clipped into at most 1 + (fragment boundaries it crosses) seeds: <= count + n_frags per unit
  std::vector<uint64_t> ebase(n_units);
  uint64_t n_entries = 0;
  for (uint32_t u = 0; u < n_units; ++u) { ebase[u] = n_entries; n_entries += (uint64_t)cnt[u] + (uint64_t)fp[u / 2].n_frags; }
  PG_HIP(ctx, A->fr_entries.reserve((size_t)n_entries, (size_t)n_entries + (size_t)n_entries / 4));
  if (!tables.empty()) PG_HIP(ctx, hipMemcpyAsync(A->fr_tables, tables.data(), tables.size() * 4, hipMemcpyHostToDevice, cur_stream(ctx)));
  PG_HIP(ctx, hipMemcpyAsync(A->fr_pairs, fp.data(), n_pairs * sizeof(FragPair), hipMemcpyHostToDevice, cur_stream(ctx)));
  if (slots) PG_HIP(ctx, hipMemcpyAsync(A->fr_slot_pair, slot_pair.data(), (size_t)slots * 4, hipMemcpyHostToDevice, cur_stream(ctx)));
  PG_HIP(ctx, hipMemcpyAsync(A->fr_ebase, ebase.data(), n_units * 8, hipMemcpyHostToDevice, cur_stream(ctx)));
  pg_prof_begin(ctx, PG_K_ANIB_BUCKET);
  hipLaunchKernelGGL(anib_bucket_kernel, dim3(n_units), dim3(256), 0, cur_stream(ctx), A->units_d, A->fr_pairs, A->mem, A->moff, A->mem_count,
                     A->fr_ebase, F.fragsize, A->fr_off, A->fr_entries);
  pg_prof_end(ctx);
  pg_prof_begin(ctx, PG_K_ANIB_FRAG);
  // (both instantiations report to the PG_K_ANIB_FRAG slot)
  const auto frag_kernel = F.search == PG_ANIB_SEARCH_ALL_DIAGS ? anib_frag_kernel<true> : anib_frag_kernel<false>;
  if (slots)
    hipLaunchKernelGGL(frag_kernel, dim3((uint32_t)slots), dim3(64), 0, cur_stream(ctx), A->refs_d, A->units_d, A->fr_pairs, A->fr_slot_pair,
                       A->fr_off, A->fr_entries, A->fr_ebase, A->fr_rows, A->fr_nrows, (const uint32_t*)nullptr, (const WordIdx*)nullptr);
  pg_prof_end(ctx);
  hipLaunchKernelGGL(anib_reduce_pairs_kernel, dim3((n_pairs + 63) / 64), dim3(64), 0, cur_stream(ctx), A->fr_pairs, n_pairs, A->fr_rows, A->fr_nrows,
                     A->fr_out);
  PG_HIP(ctx, hipGetLastError());
  PG_HIP(ctx, hipMemcpyAsync(F.out, A->fr_out, n_pairs * sizeof(pg_anib_result), hipMemcpyDeviceToHost, cur_stream(ctx)));
  PG_HIP(ctx, hipStreamSynchronize(cur_stream(ctx)));
  // ---- word tier (pga_frag.inc): pairs with some, but not all, fragments reportable get their other fragments searched again
  // with blastn-sized seeds; the subjects' word indices are built on first use
  if (slots && ctx->anib_word_tier) {
    std::vector<WordIdx> widx(ref_list.size(), WordIdx{nullptr, nullptr});
    bool any = false;
    for (uint32_t p = 0; p < n_pairs; ++p) {
      if (!(F.out[p].n_kept > 0 && F.out[p].n_kept < F.out[p].n_frags)) continue;
      const uint32_t r = ref_of_pair[p];
      if (widx[r].start) continue;
      if ((rc = anib_ensure_word_index(ctx, A, ref_list[r]))) return rc;
      const GenomeIdx& X = anim_lists(ctx)->gidx[ref_list[r]];
      widx[r] = WordIdx{X.word_start, X.word_pos};
      any = true;
    }
    if (any) {
      PG_HIP(ctx, A->fr_widx.reserve(widx.size(), widx.size() + 16));
      PG_HIP(ctx, A->fr_list.reserve((size_t)slots, (size_t)slots + (size_t)slots / 4));
      PG_HIP(ctx, A->fr_nlist.reserve(4));
      PG_HIP(ctx, hipMemcpyAsync(A->fr_widx, widx.data(), widx.size() * sizeof(WordIdx), hipMemcpyHostToDevice, cur_stream(ctx)));
      PG_HIP(ctx, hipMemsetAsync(A->fr_nlist, 0, 4, cur_stream(ctx)));
      hipLaunchKernelGGL(anib_failed_kernel, dim3((uint32_t)((slots + 255) / 256)), dim3(256), 0, cur_stream(ctx), A->fr_pairs, A->fr_slot_pair,
                         (uint32_t)slots, A->fr_rows, A->fr_nrows, A->fr_out, A->fr_widx, A->units_d, A->fr_list, A->fr_nlist);
      uint32_t n_list = 0;
      PG_HIP(ctx, hipMemcpyAsync(&n_list, A->fr_nlist, 4, hipMemcpyDeviceToHost, cur_stream(ctx)));
      PG_HIP(ctx, hipStreamSynchronize(cur_stream(ctx)));
      if (n_list) {
        pg_prof_begin(ctx, PG_K_ANIB_FRAG);
        hipLaunchKernelGGL(frag_kernel, dim3(n_list), dim3(64), 0, cur_stream(ctx), A->refs_d, A->units_d, A->fr_pairs, A->fr_slot_pair,
                           A->fr_off, A->fr_entries, A->fr_ebase, A->fr_rows, A->fr_nrows, (const uint32_t*)A->fr_list, (const WordIdx*)A->fr_widx);
        pg_prof_end(ctx);
        hipLaunchKernelGGL(anib_reduce_pairs_kernel, dim3((n_pairs + 63) / 64), dim3(64), 0, cur_stream(ctx), A->fr_pairs, n_pairs, A->fr_rows,
                           A->fr_nrows, A->fr_out);
        PG_HIP(ctx, hipGetLastError());
        PG_HIP(ctx, hipMemcpyAsync(F.out, A->fr_out, n_pairs * sizeof(pg_anib_result), hipMemcpyDeviceToHost, cur_stream(ctx)));
        PG_HIP(ctx, hipStreamSynchronize(cur_stream(ctx)));
      }
    }
  }
  if (F.sink) {   // the tables of every pair, packed on the device: one read-back of the live rows and the pairs' counts
    PgRowSink& S = *F.sink;
    std::vector<uint32_t> pair_rows(n_pairs, 0);
    if (slots) {
      const uint32_t n_slots = (uint32_t)slots, n_blocks = (n_slots + ROWS_SCAN_TILE - 1) / ROWS_SCAN_TILE;
      if (n_blocks > ROWS_SCAN_MAX_BLOCKS) return pg_fail(ctx, PG_E_CAPACITY, "fragment mode: too many (pair, fragment) slots in one launch to pack their rows");
      PG_HIP(ctx, A->fr_roff.reserve((size_t)slots + 1, (size_t)slots + (size_t)slots / 4 + 1));
      PG_HIP(ctx, A->fr_rsum.reserve(ROWS_SCAN_MAX_BLOCKS));
      PG_HIP(ctx, A->fr_prows.reserve(n_pairs, (size_t)n_pairs + n_pairs / 4));
      pg_prof_begin(ctx, PG_K_ANIB_ROWS_SCAN);
      hipLaunchKernelGGL(anib_rows_scan1_kernel, dim3(n_blocks), dim3(1024), 0, cur_stream(ctx), A->fr_nrows, n_slots, A->fr_roff, A->fr_rsum);
      hipLaunchKernelGGL(anib_rows_scan2_kernel, dim3(1), dim3(1024), 0, cur_stream(ctx), A->fr_rsum, n_blocks, A->fr_roff + n_slots);
      hipLaunchKernelGGL(anib_rows_scan3_kernel, dim3((n_slots + 1023) / 1024), dim3(1024), 0, cur_stream(ctx), A->fr_roff, n_slots, A->fr_rsum);
      pg_prof_end(ctx);
      PG_HIP(ctx, hipGetLastError());
      uint32_t total = 0;
      PG_HIP(ctx, hipMemcpyAsync(&total, A->fr_roff + n_slots, 4, hipMemcpyDeviceToHost, cur_stream(ctx)));
      PG_HIP(ctx, hipStreamSynchronize(cur_stream(ctx)));
      if ((uint64_t)total > slots * FRAG_ROWS) return pg_fail(ctx, PG_E_INTERNAL, "fragment mode: the row scan counted more rows than the slots hold");
      PG_HIP(ctx, A->fr_packed.reserve((size_t)total + 1, (size_t)total + (size_t)total / 4 + 1));
      const uint64_t n_threads = std::max<uint64_t>(slots * FRAG_ROWS, n_pairs);
      pg_prof_begin(ctx, PG_K_ANIB_ROWS_PACK);
      hipLaunchKernelGGL(anib_rows_pack_kernel, dim3((uint32_t)((n_threads + 255) / 256)), dim3(256), 0, cur_stream(ctx), A->fr_rows, A->fr_nrows,
                         A->fr_roff, n_slots, A->fr_pairs, n_pairs, A->fr_packed, A->fr_prows);
      pg_prof_end(ctx);
      PG_HIP(ctx, hipGetLastError());
      const size_t at = S.rows.size();
      S.rows.resize(at + total);
      static_assert(sizeof(pg_anib_row) == sizeof(FragRow), "FragRow is pg_anib_row");
      if (total) PG_HIP(ctx, hipMemcpyAsync(S.rows.data() + at, A->fr_packed, (size_t)total * sizeof(FragRow), hipMemcpyDeviceToHost, cur_stream(ctx)));
      PG_HIP(ctx, hipMemcpyAsync(pair_rows.data(), A->fr_prows, (size_t)n_pairs * 4, hipMemcpyDeviceToHost, cur_stream(ctx)));
      PG_HIP(ctx, hipStreamSynchronize(cur_stream(ctx)));
    }
    S.pair_count.insert(S.pair_count.end(), pair_rows.begin(), pair_rows.end());
  }
  if (F.n_rows_out) {   // the table of pair 0
    const uint32_t nf = (uint32_t)fp[0].n_frags;
    std::vector<uint32_t> nr(nf);
    std::vector<FragRow> rows((size_t)nf * FRAG_ROWS);
    if (nf) {
      PG_HIP(ctx, hipMemcpy(nr.data(), A->fr_nrows + fp[0].slot0, nf * 4, hipMemcpyDeviceToHost));
      PG_HIP(ctx, hipMemcpy(rows.data(), A->fr_rows + (size_t)fp[0].slot0 * FRAG_ROWS, rows.size() * sizeof(FragRow), hipMemcpyDeviceToHost));
    }
    uint32_t n = 0;
    for (uint32_t f = 0; f < nf; ++f)
      for (uint32_t i = 0; i < nr[f]; ++i, ++n)
        if (F.rows_out && n < F.rows_cap) F.rows_out[n] = *reinterpret_cast<const pg_anib_row*>(&rows[(size_t)f * FRAG_ROWS + i]);
    *F.n_rows_out = n;
  }
  return PG_OK;
}

// The alignment records of the pair a 1-pair batch has just processed (slice 0 of the finish scratch), converted to
// MUMmer's per-record 1-based closed coordinates.
int pg_anim_fetch_alignments(pg_ctx* ctx, int32_t ref_id, int32_t qry_id, uint32_t n, pg_anim_alignment* out) {
  AnimScratch* A = anim_scratch(ctx);
  std::vector<Aln> al(n);
  std::vector<int32_t> rr(n), qr(n);
  if (n) {
    PG_HIP(ctx, hipMemcpy(al.data(), A->S.alns, n * sizeof(Aln), hipMemcpyDeviceToHost));
    PG_HIP(ctx, hipMemcpy(rr.data(), A->S.a_rrec, n * 4, hipMemcpyDeviceToHost));
    PG_HIP(ctx, hipMemcpy(qr.data(), A->S.a_qrec, n * 4, hipMemcpyDeviceToHost));
  }
  const PgGenome& G = ctx->genomes[ref_id];
  const PgGenome& H = ctx->genomes[qry_id];
  for (uint32_t i = 0; i < n; ++i) {
    out[i] = to_record(al[i], G.rec_start[rr[i]], H.rec_start[qr[i]]);
    out[i].ref_rec = rr[i]; out[i].qry_rec = qr[i];
  }
  return PG_OK;
}

int pg_anim_reduce_run(pg_ctx* ctx, uint32_t n_pairs, const uint64_t* offsets, const int32_t* rseq, const int32_t* qseq,
                       const int32_t* rs, const int32_t* re, const int32_t* qs, const int32_t* qe, const int32_t* errors,
                       int apply_filter, pg_anim_result* out) {
  const uint64_t n = offsets[n_pairs];
  std::vector<Aln> h(n);
  for (uint64_t i = 0; i < n; ++i) {
    Aln a;
    a.strand = qs[i] > qe[i];
    a.rs = (rs[i] < re[i] ? rs[i] : re[i]) - 1; a.re = rs[i] < re[i] ? re[i] : rs[i];
    a.qs = (qs[i] < qe[i] ? qs[i] : qe[i]) - 1; a.qe = qs[i] < qe[i] ? qe[i] : qs[i];
    a.errors = errors[i];
    a.keep = apply_filter ? 0 : 3;
    h[i] = a;
  }
  const hipStream_t st = cur_stream(ctx);
  PgDevBuf<uint64_t> d_off;
  PgDevBuf<Aln> d_a;
  PgDevBuf<int32_t> d_rg, d_qg, d_idx, d_from;
  PgDevBuf<double> d_sc;
  PgDevBuf<pg_anim_result> d_out;
  PG_HIP(ctx, reserve_all(n_pairs + 1, n_pairs + 1, d_off, d_out));
  PG_HIP(ctx, reserve_all(n + 1, n + 1, d_a, d_rg, d_qg, d_idx, d_from, d_sc));
  PG_HIP_MSG(ctx, "anim reduce: ", hipMemcpyAsync(d_off, offsets, (n_pairs + 1) * 8, hipMemcpyHostToDevice, st));
  if (n) {
    PG_HIP_MSG(ctx, "anim reduce: ", hipMemcpyAsync(d_a, h.data(), n * sizeof(Aln), hipMemcpyHostToDevice, st));
    PG_HIP_MSG(ctx, "anim reduce: ", hipMemcpyAsync(d_rg, rseq, n * 4, hipMemcpyHostToDevice, st));
    PG_HIP_MSG(ctx, "anim reduce: ", hipMemcpyAsync(d_qg, qseq, n * 4, hipMemcpyHostToDevice, st));
  }
  hipLaunchKernelGGL(anim_reduce_kernel, dim3((n_pairs + 63) / 64), dim3(64), 0, st, n_pairs, d_off, d_a, d_rg, d_qg,
                     d_idx, d_from, d_sc, apply_filter, d_out);
  PG_HIP_MSG(ctx, "anim reduce: ", hipGetLastError());
  PG_HIP_MSG(ctx, "anim reduce: ", hipMemcpyAsync(out, d_out, n_pairs * sizeof(pg_anim_result), hipMemcpyDeviceToHost, st));
  PG_HIP_MSG(ctx, "anim reduce: ", hipStreamSynchronize(st));
  return PG_OK;
}

// ---- ANIb: parse_blast_tab reduction (pyani/anib.py:641-665), one thread per ordered pair ---------------------------
namespace {
__global__ __launch_bounds__(64) void anib_reduce_kernel(uint32_t n_pairs, const uint64_t* __restrict__ offsets,
                                                         const uint64_t* __restrict__ foff, const int32_t* __restrict__ frag,
                                                         const int32_t* __restrict__ length, const int32_t* __restrict__ mismatch,
                                                         const int32_t* __restrict__ gaps, const int32_t* __restrict__ qlen,
                                                         const double* __restrict__ pident, int64_t* first_row,
                                                         int64_t* __restrict__ aln_out, int64_t* __restrict__ err_out,
                                                         double* __restrict__ pid_out) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  int64_t* first = first_row + foff[p];
  const uint64_t nf = foff[p + 1] - foff[p];
  for (uint64_t f = 0; f < nf; ++f) first[f] = -1;
  for (uint64_t i = offsets[p]; i < offsets[p + 1]; ++i) {
    const int32_t alnlen = length[i] - gaps[i], alnids = alnlen - mismatch[i];
    const double cov = (double)alnlen / (double)qlen[i], pid = (double)alnids / (double)qlen[i];
    if (cov > 0.7 && pid > 0.3 && (uint64_t)frag[i] < nf && first[frag[i]] < 0) first[frag[i]] = (int64_t)i;
  }
  int64_t aln = 0, err = 0, cnt = 0;
  double sum = 0.0;
  for (uint64_t f = 0; f < nf; ++f) {
    const int64_t i = first[f];
    if (i < 0) continue;
    aln += length[i] - gaps[i];
    err += (int64_t)mismatch[i] + gaps[i];
    sum = sum + pident[i];
    ++cnt;
  }
  aln_out[p] = aln;
  err_out[p] = err;
  pid_out[p] = cnt ? sum / (double)cnt : 0.0;
}
}  // namespace

int pg_anib_reduce_run(pg_ctx* ctx, uint32_t n_pairs, const uint64_t* offsets, const uint32_t* n_frags, const int32_t* frag,
                       const int32_t* length, const int32_t* mismatch, const int32_t* gaps, const int32_t* qlen,
                       const double* pident, int64_t* aln_out, int64_t* err_out, double* pid_out) {
  const uint64_t n = offsets[n_pairs];
  std::vector<uint64_t> foff(n_pairs + 1, 0);
  for (uint32_t p = 0; p < n_pairs; ++p) foff[p + 1] = foff[p] + n_frags[p];
  const hipStream_t st = cur_stream(ctx);
  PgDevBuf<uint64_t> d_off, d_foff;
  PgDevBuf<int32_t> d_frag, d_len, d_mm, d_gap, d_ql;
  PgDevBuf<double> d_pid, d_pout;
  PgDevBuf<int64_t> d_first, d_aln, d_err;
  PG_HIP(ctx, reserve_all(n_pairs + 1, n_pairs + 1, d_off, d_foff));
  PG_HIP(ctx, reserve_all(n + 1, n + 1, d_frag, d_len, d_mm, d_gap, d_ql, d_pid));
  PG_HIP(ctx, d_first.reserve(foff[n_pairs] + 1));
  PG_HIP(ctx, reserve_all(n_pairs, n_pairs, d_aln, d_err, d_pout));
  PG_HIP_MSG(ctx, "anib reduce: ", hipMemcpyAsync(d_off, offsets, (n_pairs + 1) * 8, hipMemcpyHostToDevice, st));
  PG_HIP_MSG(ctx, "anib reduce: ", hipMemcpyAsync(d_foff, foff.data(), (n_pairs + 1) * 8, hipMemcpyHostToDevice, st));
  const struct { void* d; const void* h; size_t b; } cp[] = {{d_frag, frag, n * 4}, {d_len, length, n * 4}, {d_mm, mismatch, n * 4},
                                                           {d_gap, gaps, n * 4}, {d_ql, qlen, n * 4}, {d_pid, pident, n * 8}};
  for (const auto& c : cp)
    if (c.b) PG_HIP_MSG(ctx, "anib reduce: ", hipMemcpyAsync(c.d, c.h, c.b, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(anib_reduce_kernel, dim3((n_pairs + 63) / 64), dim3(64), 0, st, n_pairs, d_off, d_foff, d_frag, d_len,
                     d_mm, d_gap, d_ql, d_pid, d_first, d_aln, d_err, d_pout);
  PG_HIP_MSG(ctx, "anib reduce: ", hipGetLastError());
  PG_HIP_MSG(ctx, "anib reduce: ", hipMemcpyAsync(aln_out, d_aln, n_pairs * 8, hipMemcpyDeviceToHost, st));
  PG_HIP_MSG(ctx, "anib reduce: ", hipMemcpyAsync(err_out, d_err, n_pairs * 8, hipMemcpyDeviceToHost, st));
  PG_HIP_MSG(ctx, "anib reduce: ", hipMemcpyAsync(pid_out, d_pout, n_pairs * 8, hipMemcpyDeviceToHost, st));
  PG_HIP_MSG(ctx, "anib reduce: ", hipStreamSynchronize(st));
  return PG_OK;
}
