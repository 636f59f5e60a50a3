/* pyani_gpu.h — C ABI of libpyani_gpu.so, the MI355X (gfx950) engine behind pyani's hot path.
 *
 * pyani (the reference) is 100 % Python and has no FFI: the boundary this library slots behind is the
 * module API of pyani/tetra.py (and, next, the process/file boundary between pyani/anim.py and
 * nucmer/delta-filter).  Each entry point below names the reference interface it replaces (file:line,
 * relative to the reference checkout).  INTEGRATION.md shows the ctypes stub a pyani maintainer would add.
 *
 * Conventions
 *   - plain C types only; the caller owns every buffer; the library keeps no caller pointer after return.
 *   - every function returns PG_OK (0) or a negative PG_E_* code; pg_last_error(ctx) has the message.
 *   - no exceptions cross the ABI; there is NO CPU fallback: without a usable GPU pg_create fails.
 *   - one context per process and device; calls on one context must not be concurrent.
 *   - k-mer index convention: first base most significant, A=0 C=1 G=2 T=3 (== sorted() string order
 *     used by pyani/tetra.py:176), i.e. "ACGT" -> 0*64 + 1*16 + 2*4 + 3.
 */
#ifndef PYANI_GPU_H
#define PYANI_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PG_OK 0
#define PG_E_ARG (-1)      /* bad argument */
#define PG_E_NODEVICE (-2) /* no usable HIP device (the product path never falls back to CPU) */
#define PG_E_HIP (-3)      /* HIP runtime error, see pg_last_error */
#define PG_E_IO (-4)       /* file could not be read */
#define PG_E_NOMEM (-5)
#define PG_E_KEYSET (-6)   /* genomes have different observed-tetramer key sets: pyani raises AssertionError (tetra.py:174-175) */
#define PG_E_EMPTY (-7)    /* empty key set: pyani raises ZeroDivisionError (tetra.py:181) */
#define PG_E_RNA (-8)      /* sequence contains U/u: Biopython complements it asymmetrically (U->A); unsupported */
#define PG_E_CAPACITY (-9) /* a per-pair work buffer overflowed (pg_anim_result.status; pg_anim_alignments_batch) */
#define PG_E_INTERNAL (-10) /* an internal consistency check failed (traceback pass), see pg_last_error */
#define PG_E_NONFINITE (-11) /* cluster calls: a distance is NaN or infinite; scipy's linkage raises ValueError on it */

typedef struct pg_ctx pg_ctx;

/* ---- context ------------------------------------------------------------------------------------------- */
const char* pg_version(void);
/* device: HIP device ordinal (use LOCAL_RANK for one-process-per-GPU jobs). */
int pg_create(pg_ctx** out, int device);
void pg_destroy(pg_ctx* ctx);
const char* pg_last_error(const pg_ctx* ctx);
/* blocks until all work queued by this context has finished */
int pg_sync(pg_ctx* ctx);

/* ---- genome store: 2-bit codes + 1-bit "clean" mask resident in HBM ------------------------------------- */
/* Replaces Bio.SeqIO.parse(filename, "fasta") + str(rec.seq).upper() (pyani/tetra.py:98-99) and
 * pyani_files.get_sequence_lengths (pyani/pyani_files.py:128-142: total_len = sum of len(record)).
 * seq: concatenated record sequences (ASCII, any case, IUPAC allowed); rec_off[0..n_rec]: record boundaries. */
int pg_add_genome(pg_ctx* ctx, const uint8_t* seq, const uint64_t* rec_off, uint32_t n_rec, int32_t* genome_id_out);
/* Same, reading a FASTA file (records = '>' blocks; whitespace inside sequence lines removed). */
int pg_add_fasta(pg_ctx* ctx, const char* path, int32_t* genome_id_out, uint64_t* total_len_out, uint32_t* n_rec_out);
/* Many files at once: read + parse + pack on `threads` host threads (0 = all hardware threads); ids are assigned in
 * input order.  Replaces the per-file Bio.SeqIO loops of pyani_files.get_sequence_lengths (pyani_files.py:128-142) and
 * tetra.calculate_tetra_zscores (tetra.py:66-74) on the ingest side.  Any of the three output arrays may be NULL. */
int pg_add_fasta_batch(pg_ctx* ctx, const char* const* paths, uint32_t n, uint32_t threads, int32_t* genome_ids_out,
                       uint64_t* total_len_out, uint32_t* n_rec_out);
int pg_genome_count(const pg_ctx* ctx);
int pg_genome_length(const pg_ctx* ctx, int32_t genome_id, uint64_t* total_len_out, uint32_t* n_rec_out);
/* Drop all genomes (device arena is kept for reuse). */
int pg_clear_genomes(pg_ctx* ctx);
/* Push not-yet-resident genomes to HBM now (otherwise done lazily by the first compute call). */
int pg_upload(pg_ctx* ctx);
/* Bytes of the packed representation the count kernel streams for these genomes (2-bit codes + 1-bit mask,
 * padding excluded): the "algorithmic bytes" of SURVEY.md §8(d).  genome_ids == NULL means all genomes. */
int pg_tetra_algorithmic_bytes(const pg_ctx* ctx, const int32_t* genome_ids, uint32_t n, uint64_t* bytes_out,
                               uint64_t* bases_out);

/* ---- TETRA ----------------------------------------------------------------------------------------------
 * kernel 1: exact integer k-mer counts over both strands, including the reference's quirk that the last
 * tetranucleotide of each strand of each record is not counted.  Replaces the counting loops of
 * calculate_tetra_zscore (pyani/tetra.py:98-116).  c2: n x 16, c3: n x 64, c4: n x 256 (host buffers). */
int pg_tetra_counts(pg_ctx* ctx, const int32_t* genome_ids, uint32_t n, uint64_t* c2, uint64_t* c3, uint64_t* c4);

/* Z-scores from counts in the reference's IEEE-754 operation order (pyani/tetra.py:119-138), computed on the
 * device in fp64 without FMA contraction.  z: n x 256; present: n x 256 (1 where the tetramer is a key of the
 * reference's result dict, i.e. c4 > 0). */
int pg_tetra_zscores(pg_ctx* ctx, const uint64_t* c2, const uint64_t* c3, const uint64_t* c4, uint32_t n, double* z,
                     uint8_t* present);

/* kernel 2: all-vs-all Pearson matrix, bit-identical to calculate_correlations (pyani/tetra.py:158-194):
 * sequential sums in tetramer order, diagonal = 1.0.  out: n x n row-major (host).
 * PG_E_KEYSET if the present[] rows differ, PG_E_EMPTY if they are all-zero. */
int pg_tetra_corr(pg_ctx* ctx, const double* z, const uint8_t* present, uint32_t n, double* out);

/* Fused, device-resident pipeline for a batch of stored genomes: counts -> Z -> Pearson with no host round
 * trip in between; replaces calculate_tetra (scripts/average_nucleotide_identity.py:582-612).
 * Any of z_out / present_out / corr_out may be NULL.  Row/column order = order of genome_ids. */
int pg_tetra_matrix(pg_ctx* ctx, const int32_t* genome_ids, uint32_t n, double* z_out, uint8_t* present_out,
                    double* corr_out);
/* Asynchronous form used for throughput runs: queues one pass (results land in an internal pinned buffer,
 * fetched by pg_tetra_matrix_fetch after pg_sync).  Queue any number of passes, then pg_sync once. */
/* fetch_z != 0: Z and presence are copied back too (otherwise only the matrix: the reference's calculate_tetra
 * returns just the correlation DataFrame). */
int pg_tetra_matrix_enqueue(pg_ctx* ctx, const int32_t* genome_ids, uint32_t n, int fetch_z);
int pg_tetra_matrix_fetch(pg_ctx* ctx, uint32_t n, double* z_out, uint8_t* present_out, double* corr_out);

/* Multi-GPU building blocks (one process per GPU; the exchange itself is an RCCL all-gather done by the host
 * layer on these device buffers — SURVEY.md §8(e)).  d_* are DEVICE pointers owned by the caller.
 * Both calls return after their work has completed on the device. */
int pg_tetra_zscores_dev(pg_ctx* ctx, const int32_t* genome_ids, uint32_t n, double* d_z, uint8_t* d_present);
/* rows [row0, row0+nrows) of the n x n matrix from the full (all-gathered) d_z / d_present; d_out: nrows x n.
 * PG_E_KEYSET / PG_E_EMPTY as pg_tetra_corr, over all n genomes whichever rows are asked for; nrows == 0 computes
 * and checks nothing (PG_OK). */
int pg_tetra_corr_rows_dev(pg_ctx* ctx, const double* d_z, const uint8_t* d_present, uint32_t n, uint32_t row0,
                           uint32_t nrows, double* d_out);

/* ---- ANIm ------------------------------------------------------------------------------------------------
 * In-process replacement for the `nucmer --mum` + `delta-filter -1` jobs pyani builds in
 * construct_nucmer_cmdline (pyani/anim.py:240-289), runs through run_multiprocessing (run_multiprocessing.py:56-152)
 * and reduces with parse_delta (anim.py:292-411).  One result per ORDERED pair:
 *   ref_ids[i] = the genome in nucmer's *reference* role  (pyani's query genome, fname1 of anim.py:280)
 *   qry_ids[i] = the genome in nucmer's *query* role      (pyani's subject genome, fname2)
 * The tuple (ref_aln_len, qry_aln_len, identity, sim_errors) is what parse_delta returns for the pair's .filter
 * file.  status: 0 = ok; PG_ANIM_NO_ALIGNMENT = no alignment survived (parse_delta would raise ZeroDivisionError,
 * anim.py:396); PG_E_CAPACITY = internal buffers overflowed for this pair.
 * MUMmer itself is third-party and absent from the reference tree: behaviour is reconstructed and calibrated against
 * the MUMmer output files the reference's tests hold (every fixture reproduced exactly).
 * reserved = number of alignments BEFORE the 1-to-1 filter (what nucmer's .delta would hold).
 * Limits: a genome in the reference role may have any number of copies of a k-mer and any size below 2^30 - 1 bases (a reference
 * of 2^30 - 1 or more bases is refused: PG_E_CAPACITY for the call, its positions do not fit the seeding table's 30 bits).  The
 * seeding stage holds one reference k-mer group (1 of 16384 of the 16-mer space) in a table of at most 16384 slots, half full at
 * most; a group of n entries is seeded in ceil(n / 8192) passes, each of which streams the group's queries once more.  One pass
 * serves genomes up to ~130 Mb without a k-mer family of more than ~8000 copies; beyond that results are the same and seeding
 * takes that many times longer for the groups concerned. */
typedef struct {
  int64_t ref_aln_len, qry_aln_len, sim_errors, n_alignments;
  double identity;
  int32_t status;
  int32_t reserved;
} pg_anim_result;
#define PG_ANIM_NO_ALIGNMENT 1
/* maxmatch = 0: pyani's default `nucmer --mum` (anchors unique in both genomes); maxmatch != 0: `--maxmatch`
 * (anim.py:246-289: every maximal match is an anchor) — same pipeline without the uniqueness filter; no MUMmer output
 * for this mode exists among the reference's fixtures, so it is checked against the scalar CPU statement of the same search
 * (genomes with and without repeats).  filter_1to1 = 0 reproduces pyani's --nofilter (reduction over the unfiltered alignments).
 * The pairs may come in any order and may repeat; results are written in the caller's order.  pyani compares every pair in both
 * directions (anim.py:216-233): when (A, B) and (B, A) are both in ONE call they share their seeding (same maximal exact
 * matches), so one call with the whole job is up to 1.6 x faster than the directions in separate calls — same results. */
int pg_anim_pairs(pg_ctx* ctx, const int32_t* ref_ids, const int32_t* qry_ids, uint64_t n_pairs, int maxmatch,
                  int filter_1to1, pg_anim_result* out);
/* The non-blocking form (round 6; the counterpart of pg_tetra_matrix_enqueue / _fetch): pyani's runner keeps all its cores busy
 * across job boundaries (one multiprocessing.Pool for the whole job list, run_multiprocessing.py:130-144); a blocking pg_anim_pairs
 * pays the sequential tails of its last kernels (one forced re-alignment can hold a single wave for 0.1 s) with the rest of the
 * GPU idle.  pg_anim_pairs_enqueue copies the id lists, starts the call on a host thread of the context and returns a ticket at
 * once; pg_anim_pairs_fetch waits for that call and writes its n_pairs results (the status of the call is fetch's return value).
 * At most TWO calls are in flight per context (PG_E_CAPACITY beyond): they run on disjoint halves of the context's four
 * (stream, scratch) worker slots with half the match budget each, so the tail of call k overlaps the front of call k + 1.
 * Results are those of pg_anim_pairs, bit for bit.  Every ticket must be fetched (pg_destroy waits for unfetched calls). */
int pg_anim_pairs_enqueue(pg_ctx* ctx, const int32_t* ref_ids, const int32_t* qry_ids, uint64_t n_pairs, int maxmatch,
                          int filter_1to1, uint64_t* ticket);
int pg_anim_pairs_fetch(pg_ctx* ctx, uint64_t ticket, pg_anim_result* out, uint64_t n_pairs);

/* The extension algorithm after seeding and clustering is MUMmer 3.23's own postnuc (extendClusters + its alignment engine:
 * dynamic anti-diagonal band trimmed at breaklen * 3 below the best score, backward search + forced forward re-alignment,
 * MUMmer's tie order): it reproduces every alignment record (coordinates and error counts) of the nucmer output files the
 * reference's tests hold and is what replaces pyani's `nucmer` job (pyani/anim.py:240-289).  There is no other extender: the
 * approximate fixed-band one of rounds 1-2 was retired in round 5.  pg_anim_set_extender stays in the ABI for callers built against the
 * round-4 header: PG_EXTENDER_NUCMER is accepted (a no-op), every other value is PG_E_ARG. */
#define PG_EXTENDER_NUCMER 0
int pg_anim_set_extender(pg_ctx* ctx, int extender);
/* How many host worker threads (each with its own HIP stream and scratch) share one pg_anim_pairs / pg_anib_pairs call: 1 ... 4,
 * default 2 (the launches of two streams overlap: one worker's read-backs and sequential tails hide behind the other's kernels).
 * The counterpart of pyani's --workers inside ONE device (subcmd_anim.py:392-396 spreads jobs over CPU cores; over devices it is
 * pyani_amd.multi.MultiEngine).  Results do not depend on it; 1 gives un-overlapped per-stage timings (pg_profile_get). */
int pg_anim_set_workers(pg_ctx* ctx, int workers);

/* Engine counters of the nucmer extender since the last reset, for measurement (bench.py's VALU-issue roofline: cells per second
 * against the instruction count per cell): out[64].  out[0..2] = calls / anti-diagonals / DP cells of all register engines;
 * out[32 + 4 k + {0, 1, 2}] = the same for the diagonal engine in kernel class k (0 match-to-match gaps, 1 forward extensions,
 * 2 backward searches run ahead, 3 the units' walks, 4 forced runs in the narrow kernel, 5 / 6 forced runs in windows of up to 1024 /
 * 2048 diagonals, 7 forced runs on a group of four waves: 3072 ... 8192 diagonals); the rest: development counters.
 * Synchronises the context's streams. */
int pg_anim_counters(pg_ctx* ctx, uint64_t* out, int reset);

/* ---- development ------------------------------------------------------------------------------------------------------------
 * Caller-chosen rectangles through the forced re-alignment launches of the extender (the four kernels a batch runs after its
 * walks: narrow / wide windows of one wave, the group of four waves, the column strips), so that tests can place a rectangle on a
 * window boundary, a stream end or a hand-over between kernels instead of waiting for a genome pair to produce one.
 * rects[4 n]: (A0, A1, B0, B1) per rectangle as the walk hands them to its forced runs — stream positions of the resident genomes
 * ref_id / qry_id, both ends inclusive, B in the coordinates of the query strand (0 forward, 1 reverse complement).
 * Per rectangle: errors[i] = error count of the optimal global path, w_used[i] = the band it was certified with (-1: the whole
 * rectangle), status[i] = 0 certified, 2 = the corner stayed unreachable or no engine held the run (what flags a unit PG_E_CAPACITY
 * in a batch; errors and w_used are 0 then).  Every rectangle is a unit of its own, so a failure marks that rectangle alone.
 * Honoured only under PYANI_DEV_KNOBS=1 (PG_E_ARG without it).  PG_E_ARG also for a side below 1, a rectangle outside its stream
 * and a side longer than one engine call aligns (10 000 bases: MUMmer's MAX_ALIGNMENT_LENGTH).  Not while enqueued calls are in flight. */
int pg_anim_forced_rects(pg_ctx* ctx, int32_t ref_id, int32_t qry_id, int strand, uint32_t n, const int32_t* rects, int32_t* errors,
                         int32_t* w_used, int32_t* status);

/* Caller-chosen TRIMMED searches on the extender's search engines (MUMmer's own band: cut 600 below the best score, broken 200
 * anti-diagonals after it — the match-to-match gaps, forward extensions, backward searches and the walks' own calls), so that tests can
 * put a search on a window move, a window misfit, the break length, a stream end or a size class of the lane kernels instead of
 * waiting for a genome pair to produce one.  The sibling of pg_anim_forced_rects, with its conventions: two resident genomes and one
 * query strand; honoured only under PYANI_DEV_KNOBS=1 (PG_E_ARG without it); not while enqueued calls are in flight.
 * searches[5 n]: (A0, B0, tA, tB, m_o) per search — start and target as stream positions (both inclusive, B in the coordinates of
 * the query strand), m_o one of PG_SEARCH_FORWARD_ALIGN, PG_SEARCH_BACKWARD_SEARCH, each with or without PG_SEARCH_OPTIMAL_BIT
 * (without: the target corner is the finish if the matrix was walked to its end; with: the best cell is).
 * engine: which product code runs —
 *   PG_SEARCH_PREPASS      the pre-pass kernels' engine (256-diagonal window only) calling its align(), one wave per search, items taken
 *                          from a cursor in the chunk sizes of the gap, forward and backward kernels; a band the window does not hold
 *                          (the engine's overflow: left to the walk in a batch) is held = 0
 *   PG_SEARCH_WALK         the walks' engine calling its align(): 256 diagonals, then 512, then the wave's slice of global memory
 *   PG_SEARCH_RUNG_256 / _RUNG_512 / _RUNG_GLOBAL   one rung of that ladder called directly, held = its own verdict
 *   PG_SEARCH_LANES        FORWARD_ALIGN only: every search as a match-to-match gap (a chain of two one-base matches, start and target)
 *                          through the batch's gap launches — gap list, the three one-gap-per-lane kernels (sides up to 16 / 32 / 59),
 *                          and the wave kernel for every gap that is not small
 * out[5 n]: endA, endB, errors, reached, held per search; held = 0: the engine asked for did not hold the band, the other fields are 0.
 * PG_E_ARG (one bad search refuses the call) for a search with the forced bit or any other mode, a position outside its stream, a
 * target on the wrong side of the start for the direction, a side above 10 000 bases (MAX_ALIGNMENT_LENGTH), a bad id, strand or engine. */
enum { PG_SEARCH_PREPASS = 0, PG_SEARCH_WALK = 1, PG_SEARCH_RUNG_256 = 2, PG_SEARCH_RUNG_512 = 3, PG_SEARCH_RUNG_GLOBAL = 4, PG_SEARCH_LANES = 5 };
enum { PG_SEARCH_FORWARD_ALIGN = 1, PG_SEARCH_BACKWARD_SEARCH = 2, PG_SEARCH_OPTIMAL_BIT = 8 };
int pg_anim_searches(pg_ctx* ctx, int32_t ref_id, int32_t qry_id, int strand, int engine, uint32_t n, const int32_t* searches, int32_t* out);

/* Work-memory budget of pg_anim_pairs: at most max_pairs ordered pairs and max_matches exact matches in flight (about 384 bytes
 * of device scratch per match, grown on demand; default 131072 pairs / 512 Mi matches, split over the context's two workers =
 * launches of up to 65536 pairs / 256 Mi matches, ~68 GB each).  Larger calls are split transparently; results do not depend on
 * the split. */
int pg_anim_set_batch_budget(pg_ctx* ctx, uint32_t max_pairs, uint64_t max_matches);

/* The alignment records of ONE ordered pair: the content of the .delta file nucmer would write (kept == 3 marks the
 * records delta-filter -1 keeps, i.e. the .filter file), minus the indel offset lists, which parse_delta ignores
 * (anim.py:374-393); pg_anim_alignments_batch below returns them too.  Coordinates as in MUMmer's alignment header lines
 * (pyani/nucmer.py:333-351): 1-based, closed, relative to the record, qs > qe on the reverse strand; ref_rec / qry_rec
 * = ordinal of the FASTA record (the '>' line names the ids).  At most `cap` records are written, *n_out = how many
 * there are.  Used for alignment-level parity tests and to write recovery files (pyani_amd.anim.write_delta). */
typedef struct {
  int32_t ref_rec, qry_rec;
  int32_t rs, re, qs, qe;
  int32_t errors;
  int32_t kept;   /* 3 = survives delta-filter -1 (bit 0: reference-side LIS, bit 1: query-side LIS) */
} pg_anim_alignment;
int pg_anim_pair_alignments(pg_ctx* ctx, int32_t ref_id, int32_t qry_id, pg_anim_alignment* out, uint32_t cap, uint32_t* n_out);

/* The same for MANY ordered pairs in one call — what pyani's nucmer jobs leave on disk for a whole run (the .delta files of
 * pyani/anim.py:240-289, one per pair; kept == 3 marks the records of the .filter files), without running the search once per
 * pair.  aln_offsets[n_pairs + 1]: pair i owns records [aln_offsets[i], aln_offsets[i + 1]) of the result, in MUMmer's output
 * order (forward-strand alignments of the pair, then reverse-strand ones, each in the order postnuc creates them).
 * with_indels != 0 adds a traceback pass on the GPU (one thread per search / forced piece of the alignments' paths, scalar engine
 * with a backpointer store) and yields every record's .delta indel offset list (pyani/nucmer.py:170-290 parses them: positive =
 * a reference base facing a gap, negative = a query base facing a gap, distances between consecutive indels; the terminating 0
 * is not stored); *n_indels = how many numbers all lists hold together.
 * The result stays in the context until the next call; pg_anim_alignments_read copies it out: out[aln_offsets[n_pairs]],
 * indel_offsets[n_alignments + 1] and indels[*n_indels] (both may be NULL). */
int pg_anim_alignments_batch(pg_ctx* ctx, const int32_t* ref_ids, const int32_t* qry_ids, uint64_t n_pairs, int maxmatch, int with_indels,
                             uint64_t* aln_offsets, uint64_t* n_indels);
int pg_anim_alignments_read(pg_ctx* ctx, pg_anim_alignment* out, uint64_t* indel_offsets, int64_t* indels);

/* The reduction alone, on alignment records supplied by the caller (e.g. parsed from existing MUMmer .delta/.filter
 * files — pyani's --recovery mode): replaces delta-filter -1 (apply_filter != 0; scripts/delta_filter_wrapper.py:70-93)
 * and parse_delta (anim.py:292-411).  Pair p owns records [offsets[p], offsets[p+1]).  Coordinates are the 1-based
 * closed MUMmer coordinates (qs > qe for reverse-strand hits); rseq / qseq are per-pair sequence (record) ordinals. */
int pg_anim_reduce(pg_ctx* ctx, uint32_t n_pairs, const uint64_t* offsets, const int32_t* rseq, const int32_t* qseq,
                   const int32_t* rs, const int32_t* re, const int32_t* qs, const int32_t* qe, const int32_t* errors,
                   int apply_filter, pg_anim_result* out);

/* ---- ANIb reduction -------------------------------------------------------------------------------------
 * parse_blast_tab of pyani/anib.py:569-667 (mode "ANIb", BLAST+ 15-column rows) for a batch of ordered pairs.
 * Pair p owns rows [offsets[p], offsets[p+1]) in file order; frag[] = ordinal of the query fragment (0-based, < n_frags[p]).
 * Per row: ani_alnlen = length - gaps, ani_alnids = ani_alnlen - mismatch; rows with ani_alnlen/qlen > 0.7 and
 * ani_alnids/qlen > 0.3 are kept, then the first kept row of every fragment.  Outputs per pair: aln_length =
 * sum(ani_alnlen), sim_errors = sum(mismatch) + sum(gaps), pid = mean(pident) over the kept rows in fragment order
 * (0 if none) — sequential fp64 sum, within 1e-12 (relative) of pandas' pairwise mean. */
int pg_anib_reduce(pg_ctx* ctx, uint32_t n_pairs, const uint64_t* offsets, const uint32_t* n_frags, const int32_t* frag,
                   const int32_t* length, const int32_t* mismatch, const int32_t* gaps, const int32_t* qlen, const double* pident,
                   int64_t* aln_length_out, int64_t* sim_errors_out, double* pid_out);

/* ---- ANIb fragment mode -----------------------------------------------------------------------------------
 * In-process replacement for the BLAST+ jobs pyani builds in construct_blastn_cmdline (pyani/anib.py:451-471: the
 * `fragsize`-nt fragments of the query genome, anib.py:164-203, searched with blastn -task blastn against the subject
 * genome) followed by parse_blast_tab (anib.py:569-667).  One result per ORDERED pair (qry_ids[i] = the fragmented genome,
 * sbj_ids[i] = the BLAST database genome):  aln_length = sum of (length - gaps), sim_errors = sum of (mismatch + gaps),
 * pid = mean pident, each over the FIRST row of every fragment among the rows with coverage > 0.7 and identity > 0.3 (rows in
 * BLAST's order: best score first; anib.py:640-660 filters, then drops duplicates keeping the first) — the tuple parse_blast_tab
 * returns.  BLAST+ is third-party and absent from the reference tree; the search is a restatement of its documented
 * behaviour for this command line (blastn scoring 2 / -3 / 5 / 2, X-drop 150 bits, e-value 1e-15; seeds: exact 16-mers, then
 * blastn's 11-mer words for fragments those leave without a reportable hit), checked against the BLAST+ tables the reference's
 * tests hold (level of agreement per fixture).
 * Limits: fragsize <= 1020 (pyani's default and maximum in practice; larger values are rejected with PG_E_ARG — the fragment's
 * DP lives in LDS).  Query genomes of any bacterial or fungal size: up to 15 872 fragments (16.1 Mb at 1020 nt) the per-fragment
 * counters sit in LDS, beyond that in HBM (round 5: there used to be a hard limit); only a query of more than ~10^6 fragments
 * (1 Gb) comes back with status = PG_E_CAPACITY (n_frags set, everything else 0), the call going on with the others.
 * Subject genomes: no size or repeat cap from seeding either.  The seeding stage holds one coarse k-mer group of the subject (1 of
 * 2048 of the 16-mer space) in a table of at most 16384 slots, half full at most; a group of n entries is seeded in ceil(n / 8192)
 * passes, each of which streams the group's query entries once more: one pass up to ~16 Mb, two up to ~33 Mb, and so on (a
 * k-mer family of thousands of copies adds passes for its group alone).  The 2^30 - 1 base limit of ANIm's reference role belongs
 * to ANIm's seeding table and does not apply here. */
typedef struct {
  int64_t aln_length, sim_errors;
  double pid;
  int32_t n_frags, n_kept;   /* fragments of the query genome / fragments that contributed */
  int32_t status, reserved;  /* 0 = ok, PG_E_CAPACITY = the query genome has more fragments than a launch can hold (see above) */
} pg_anib_result;
int pg_anib_pairs(pg_ctx* ctx, const int32_t* qry_ids, const int32_t* sbj_ids, uint64_t n_pairs, uint32_t fragsize, pg_anib_result* out);
/* The table of ONE ordered pair, row for row as pyani reads it (anib.py:609-624): at most 4 rows per fragment (2 strands x
 * 2 anchors), best score first; frag = 0-based fragment ordinal (frag00001 = 0), coordinates 1-based as BLAST prints them
 * (sstart > send on the minus strand), srec = ordinal of the subject record, score = raw alignment score. */
typedef struct {
  int32_t frag, length, mismatch, gaps, nident, qlen, qstart, qend, sstart, send, srec, score;
} pg_anib_row;
int pg_anib_pair_rows(pg_ctx* ctx, int32_t qry_id, int32_t sbj_id, uint32_t fragsize, pg_anib_row* out, uint32_t cap, uint32_t* n_out);

/* The tables of MANY ordered pairs in one call — what pyani's blastn jobs leave on disk for a whole run (one
 * `<query>_vs_<subject>.blast_tab` per ordered pair under blastn_output/, pyani/anib.py:383-471) — without running the launch chain
 * once per pair.  out[i] is what pg_anib_pairs returns for pair i, and pair i owns rows [row_offsets[i], row_offsets[i + 1]) of the
 * result, exactly the rows pg_anib_pair_rows gives for it and in its order (fragments in order, a fragment's rows best score
 * first), in the CALLER's pair order: how the call sorts its pairs by subject, cuts them into launches and deals those to the
 * context's workers does not show.  Every launch compacts its rows on the device (an exclusive scan over the per-fragment row
 * counts, then a pack pass) and reads back the live rows and one count per pair, not the padded per-fragment scratch.
 * row_offsets: n_pairs + 1 entries.  A pair whose status is PG_E_CAPACITY owns no rows; the call goes on with the others.
 * n_pairs == 0 is PG_OK with row_offsets[0] = 0.  Argument checks as pg_anib_pairs (fragsize 1 ... 1020, ids in range: PG_E_ARG).
 * The result stays in the context until the next pg_anib_rows_batch; pg_anib_rows_read copies it out: out[row_offsets[n_pairs]]
 * (may be NULL when there is no row).  PG_E_ARG before any pg_anib_rows_batch has succeeded on the context. */
int pg_anib_rows_batch(pg_ctx* ctx, const int32_t* qry_ids, const int32_t* sbj_ids, uint64_t n_pairs, uint32_t fragsize,
                       pg_anib_result* out, uint64_t* row_offsets);
int pg_anib_rows_read(pg_ctx* ctx, pg_anib_row* out);

/* Which diagonals fragment mode takes a candidate's initial HSPs from — a per-context setting, PG_ANIB_SEARCH_SEEDS by default.
 *   PG_ANIB_SEARCH_SEEDS      the diagonals of the search's own seeds (16-mers, and the word tier's 11-mers): every table and
 *                             tuple as it has always been;
 *   PG_ANIB_SEARCH_ALL_DIAGS  opt-in: the preliminary stage also walks the diagonals within 47 of a candidate's that hold no seed,
 *                             as blastn takes its initial HSPs from every 11-mer diagonal.  Closes most of the "+-1 mismatch" rows
 *                             against blastn on 74 - 85 % pairs; costs kernel time (measured gain and cost).
 * pg_anib_pairs, pg_anib_pair_rows and pg_anib_rows_batch read the setting once, at entry.  Any other value: PG_E_ARG, the setting
 * stays.  Tables of the two modes differ in a few rows per hundred fragments at most; a run should not mix them. */
#define PG_ANIB_SEARCH_SEEDS 0u
#define PG_ANIB_SEARCH_ALL_DIAGS 1u
int pg_anib_set_search(pg_ctx* ctx, uint32_t mode);
int pg_anib_get_search(pg_ctx* ctx, uint32_t* mode);

/* ---- sketch mode: an opt-in ESTIMATE in the shape of pyani's fastANI wrapper -------------------------
 * Replaces the `fastANI -q <query> -r <ref> --fragLen 3000 -k 16 --minFraction 0.2` job of pyani/fastani.py:193-229
 * (construct_fastani_cmdline) and the line parse_fastani_file reads back (fastani.py:231-270): ANI estimate, matching fragments,
 * query fragments.  Definition (pyani_amd/csrc/pg_sketch_core.h), for a k-mer size 8 <= k <= 16 (fastANI's --kmer; default 16):
 * a canonical k-mer is a 2k-bit integer (first base in the high bits, min of forward and reverse complement), sampled 1 in `scale`
 * by a hash (FracMinHash); a window exists iff its k bases are unambiguous and inside one record; the query's records are cut into
 * non-overlapping fragments of `frag_len` bases, and a sampled k-mer belongs to the fragment that holds all k of its bases; per
 * fragment the share C = h / n of its sampled k-mers that occur anywhere in the reference, identity = C^(1/k):
 *   k = 16: four correctly rounded square roots;
 *   k = 8 ... 15: y = those four square roots (at or above the root), then exactly 12 Newton steps, each p = y; k - 2 times
 *   p = p * y; y = y - (p * y - C) / (k * p), every operation rounded on its own (the same bits on host and device);
 * a fragment matches with h >= 2 and identity >= 0.80; ani = mean identity of the matching fragments, summed in ascending fragment
 * order (a FRACTION, as ComparisonResult.ani), status PG_SKETCH_NO_RESULT when fewer than min_fraction of the fragments match
 * (fastANI writes no line then).  Sketches are built on first use and cached per genome under (k, frag_len, scale): a call with
 * other values rebuilds.  An estimate with its own columns: nothing of it enters the exact ANIm / ANIb results.
 * Limits: <= 24 576 fragments per query (PG_E_CAPACITY); kmer outside 8 ... 16: PG_E_ARG.  pg_sketch_pairs is pg_sketch_pairs_k
 * with kmer = 16. */
typedef struct {
  double ani;          /* mean identity estimate of the matching fragments, 0 ... 1 (0 when status != 0) */
  int32_t matches;     /* fragments with an identity estimate >= 0.80 */
  int32_t fragments;   /* fragments of the query genome */
  int32_t status;      /* 0 = ok, PG_SKETCH_NO_RESULT */
  int32_t reserved;
} pg_sketch_result;
#define PG_SKETCH_NO_RESULT 1
int pg_sketch_pairs(pg_ctx* ctx, const int32_t* qry_ids, const int32_t* ref_ids, uint64_t n_pairs, int32_t frag_len, int32_t scale,
                    double min_fraction, pg_sketch_result* out);
int pg_sketch_pairs_k(pg_ctx* ctx, const int32_t* qry_ids, const int32_t* ref_ids, uint64_t n_pairs, int32_t kmer, int32_t frag_len,
                      int32_t scale, double min_fraction, pg_sketch_result* out);

/* The MAPPED sketch mode (mapping = "window"; opt-in, pg_sketch_pairs / pg_sketch_pairs_k stay as they are).  A fragment's hits must
 * fall inside ONE window of the reference, and a reference bin keeps one fragment — fastANI's mapping step and its one-to-one rule,
 * which the mode above lacks (a k-mer found anywhere in the reference counts there).  Definition (pg_sketch_core.h), L = frag_len:
 * a sampled k-mer occurrence of the reference has the coordinate g = its start in the records back to back WITHOUT separator, bin
 * g / L of nb = ceil(genome length / L); window w = bins w and w + 1.  Per query fragment: c_b / h_w = its sampled occurrences whose
 * k-mer occurs in bin b / in window w (once per bin and window); hits = max h_w, window = the lowest w reaching it, bin = window if
 * c_window >= c_(window + 1), else window + 1 (both -1 when hits = 0); identity = (hits / n)^(1/k) as above; candidate iff hits >= 2 and
 * identity >= 0.80; among the candidates of one bin the larger identity wins, ties go to the lower fragment index.  matches = the
 * survivors, ani = their identities summed in fragment order / matches, fragments and the min_fraction rule as above.
 * pg_sketch_pairs_mapped: the arguments, checks and result struct of pg_sketch_pairs_k.  Each genome used as a reference gets a
 * position index (built on first use, cached under (kmer, scale): another frag_len does not rebuild it; released with the sketches by
 * pg_clear_genomes), each query the grouped form of its sketch.  Limits: a reference of more than 8 192 bins (frag_len <= 65 535;
 * 4 096 bins above that) is refused with PG_E_CAPACITY — the message names the limit in bases at the given frag_len (24.5 Mb at
 * 3 000); the query's fragment count is not limited.
 * pg_sketch_pair_fragments: one record per query fragment of ONE pair, in fragment order — where every fragment mapped.  At most
 * `cap` records are written, *n_out = how many the pair has (PG_OK either way: call again with cap >= *n_out).  identity is 0 when
 * hits < 2 or n = 0; kept = 1 for a survivor.
 * pg_sketch_map_last_ms: out2[0] = milliseconds the latest pg_sketch_pairs_mapped / pg_sketch_pair_fragments call spent building
 * position indexes and grouped sketches (0 when all were cached), out2[1] = in its mapping kernel (HIP events on the context's stream). */
typedef struct {
  int32_t window;      /* w*: the lowest window with the most hits, -1 when hits = 0 */
  int32_t bin;         /* the reference bin the fragment competes for, -1 when hits = 0 */
  uint32_t hits;       /* h = max over windows */
  uint32_t n;          /* sampled k-mer occurrences of the fragment */
  double identity;     /* (hits / n)^(1/k); 0 when hits < 2 or n = 0 */
  int32_t kept;        /* 1: candidate and the winner of its bin */
  int32_t reserved;
} pg_sketch_fragment;
int pg_sketch_pairs_mapped(pg_ctx* ctx, const int32_t* qry_ids, const int32_t* ref_ids, uint64_t n_pairs, int32_t kmer, int32_t frag_len,
                           int32_t scale, double min_fraction, pg_sketch_result* out);
int pg_sketch_pair_fragments(pg_ctx* ctx, int32_t qry_id, int32_t ref_id, int32_t kmer, int32_t frag_len, int32_t scale,
                             pg_sketch_fragment* out, uint64_t cap, uint64_t* n_out);
int pg_sketch_map_last_ms(pg_ctx* ctx, double* out2);

/* ---- screen: all-vs-all matrix of shared sampled k-mers (the pre-filter that says which pairs are worth an exact
 * comparison).  Definition (pyani_amd/csrc/pg_screen_core.h): S(g) = the DISTINCT canonical k-mers of genome g (8 <= kmer <= 16, all
 * records, either strand, windows of k unambiguous bases inside one record) with mix32(k-mer) & (scale - 1) == 0; scale a power of two,
 * 1 ... 65 536.  sizes_out[a] = |S(a)|; shared_out[a * n + b] = |S(a) & S(b)| (symmetric, the diagonal = sizes), rows and columns in the
 * order of genome_ids.  Integers only: containment, Jaccard index and the identity estimate are the caller's arithmetic
 * (pyani_amd/screen.py).  No pair loop: the (k-mer, genome) keys of all n genomes are sorted once, and a k-mer held by m genomes adds one to
 * m (m - 1) / 2 cells.  An ESTIMATE for triage, never written into the exact ANIm / ANIb results.
 * part / n_parts (1 <= n_parts <= 4096): the call counts only the k-mers of the slice bins [4096 part / n_parts, 4096 (part + 1) / n_parts),
 * bin = (mix32(k-mer) >> log2(scale)) & 4095; the sizes and matrices of all parts add up to those of n_parts = 1, exactly.
 * Limits: n <= 8192 and no id twice (PG_E_ARG; the count is checked before the ids are read); kmer or scale outside the above: PG_E_ARG.
 * The keys are worked off in slices of whole bins of at most max_keys keys (pg_screen_set_budget; 0 = the default 2^28, at most 2^30:
 * PG_E_ARG beyond); one bin holding more than that: PG_E_NOMEM, the message says so.  The result does not depend on the budget.  Every
 * device buffer of the call is released before it returns; the sketch mode's caches and the ANIm seed lists are not touched (device
 * memory running short releases the ANIm launch scratch of an idle context, as in the sketch mode).
 * pg_screen_last: of the latest pg_screen_matrix on the context, out5 = keys, distinct (k-mer, genome) entries, k-mers held by >= 2
 * genomes, pair increments, slices; ms3 = milliseconds of the scan passes, of sorting and grouping, of the count kernel (HIP events). */
int pg_screen_matrix(pg_ctx* ctx, const int32_t* genome_ids, uint32_t n, int32_t kmer, int32_t scale, uint32_t part, uint32_t n_parts,
                     uint32_t* sizes_out, uint32_t* shared_out);
int pg_screen_set_budget(pg_ctx* ctx, uint64_t max_keys);
int pg_screen_last(pg_ctx* ctx, uint64_t* out5, double* ms3);

/* ---- screen, the selection: which cells of the matrix name a pair worth an exact comparison, decided on the device so that only the kept
 * pairs come back.  One n x n uint32 matrix is RESIDENT on the context between the calls:
 * pg_screen_hold is pg_screen_matrix without the n^2 read-back: same arguments, refusals and pg_screen_last; the finished matrix stays on
 * the device and only sizes_out comes back.  n == 0 is PG_OK and leaves nothing resident.
 * pg_screen_load makes the caller's matrix (row-major, 1 <= n <= 8192: PG_E_ARG outside, the count checked before the matrix is read) the
 * resident one; it need not be symmetric nor agree with any sizes.
 * Either call, once its arguments have passed, releases the matrix and selection of an earlier one BEFORE it makes its own (never two at a
 * time): a call refused for its arguments changes nothing, one that fails later leaves no matrix resident.
 * pg_screen_select keeps the cell (a, b) iff a != b and shared[a][b] >= min(need[a], need[b]) — every cell by its OWN value, a diagonal cell
 * never — and packs the kept cells as (a, b, shared[a][b]) in row-major order (the order of numpy's nonzero; no atomics: a count pass, an
 * exclusive scan, a fill pass).  need: n uint32 (pyani_amd.screen.identity_thresholds turns an identity threshold into them);
 * *n_pairs_out = the number of kept cells.  The selection stays on the device until the next pg_screen_select on the context or the
 * release of the matrix; any number of selections may follow one hold / load.  PG_E_ARG without a resident matrix or when n is not its
 * size; PG_E_NOMEM when the kept cells (12 bytes each) do not fit.
 * pg_screen_select_read copies the latest selection to the host: a_out, b_out int32, shared_out uint32, n_pairs entries each (may be NULL
 * when nothing was kept).  PG_E_ARG before any selection over the resident matrix.
 * pg_screen_fetch copies the resident matrix to the host (n x n uint32).  PG_E_ARG without one.
 * pg_screen_release frees the matrix and the selection (PG_OK when there is none); pg_clear_genomes and pg_destroy do the same, and so does
 * a sketch or screen call that finds device memory short while the matrix sits idle. */
int pg_screen_hold(pg_ctx* ctx, const int32_t* genome_ids, uint32_t n, int32_t kmer, int32_t scale, uint32_t part, uint32_t n_parts,
                   uint32_t* sizes_out);
int pg_screen_load(pg_ctx* ctx, const uint32_t* shared, uint32_t n);
int pg_screen_select(pg_ctx* ctx, const uint32_t* need, uint32_t n, uint64_t* n_pairs_out);
int pg_screen_select_read(pg_ctx* ctx, int32_t* a_out, int32_t* b_out, uint32_t* shared_out);
int pg_screen_fetch(pg_ctx* ctx, uint32_t* shared_out);
int pg_screen_release(pg_ctx* ctx);

/* ---- screen, the index: collections beyond 8192 genomes.  The n x n matrix is never formed: the k-mers held by two or
 * more genomes stay RESIDENT on the context in compressed-row form — group_start uint64[G + 1], member uint32[E], the call indices of a
 * group's genomes in ascending order — and the matrix is made and selected a BAND of consecutive rows at a time.  The same definitions as
 * pg_screen_matrix (S(g), sampling, window validity, canonical form); the index is independent of the resident matrix of pg_screen_hold /
 * _load: either may exist without the other and neither call family touches the other's state (one exception, as for every sketch or
 * screen call: a pg_screen_index that finds device memory short releases the ANIm launch scratch and an idle resident matrix; the band
 * calls give up nothing).
 * pg_screen_index scans, sorts and groups as pg_screen_matrix does (slices under pg_screen_set_budget; PG_E_NOMEM for a bin beyond it) and
 * appends every slice's grouped entries to the index; a k-mer of one genome only counts into sizes_out[a] = |S(a)|.  Limits: n <= 2^20
 * (PG_E_ARG beyond, checked before the ids are read), no id twice, kmer and scale as for pg_screen_matrix.  PG_E_NOMEM when the index does
 * not fit; the message names the entry count.  Once the arguments have passed, the index of an earlier call is released BEFORE the new one
 * is made (never two at a time): a call refused for its arguments changes nothing, one that fails later leaves none.  n == 0 is PG_OK and
 * leaves none.  The index lives until the next such call, pg_screen_index_release (PG_OK when there is none), pg_clear_genomes or pg_destroy.
 * pg_screen_set_band: rows of one band, at most 8192 (PG_E_ARG beyond); 0 = the default, the largest rows <= min(8192, n) with
 * rows * n <= 2^29 cells.  Band b covers the rows [b rows, min(n, (b + 1) rows)).  No result depends on the setting.
 * pg_screen_index_select works the bands band_first, band_first + band_step, ... (band_step >= 1: PG_E_ARG otherwise) in ascending order.
 * Per band: the groups' members inside the band's rows by two binary searches; the cells counted with uint32 atomics, balanced by item
 * over the groups with a member in the band; the cell of a genome with itself = sizes — the band then equals those rows of
 * pg_screen_matrix's result — and the rule of pg_screen_select on the rectangle: (a, b) kept iff a != b and
 * band[a][b] >= min(need[a], need[b]), packed as (a, b, shared) with global indices in row-major order, and copied to the host as the
 * band finishes.  The device holds one band at a time; the bands' lists concatenated are in the order of pg_screen_select.  need: n
 * uint32; PG_E_ARG without an index or when n is not its size; *n_pairs_out = the kept cells of the bands worked.
 * pg_screen_index_read copies the latest selection out (n_pairs entries each; may be NULL when nothing was kept); PG_E_ARG before any.
 * pg_screen_index_band makes one band and copies it to the host: (rows of the band) x n uint32, row-major.  PG_E_ARG without an index or
 * for a band that does not exist.
 * pg_screen_index_last: counts_out[7] = keys, distinct (k-mer, genome) entries, grouped entries E, groups G, slices of the latest
 * pg_screen_index; bands worked and pair increments (the atomic adds: sum over the groups of members in the band x (members - 1)) of
 * the latest pg_screen_index_select.  ms_out[4] = scan, sort + group | count, select milliseconds of the same (HIP events). */
int pg_screen_index(pg_ctx* ctx, const int32_t* genome_ids, uint32_t n, int32_t kmer, int32_t scale, uint32_t* sizes_out);
int pg_screen_index_release(pg_ctx* ctx);
int pg_screen_set_band(pg_ctx* ctx, uint32_t rows);
int pg_screen_index_select(pg_ctx* ctx, const uint32_t* need, uint32_t n, uint32_t band_first, uint32_t band_step, uint64_t* n_pairs_out);
int pg_screen_index_read(pg_ctx* ctx, int32_t* a_out, int32_t* b_out, uint32_t* shared_out);
int pg_screen_index_band(pg_ctx* ctx, uint32_t band, uint32_t* out);
int pg_screen_index_last(pg_ctx* ctx, uint64_t* counts_out, double* ms_out);

/* ---- screen, the components: which genomes belong together.  The connected components of the graph whose edges are the
 * entries (a[e], b[e]) of a list over n nodes, direction ignored, and two sums per node, all integers that depend on neither the order of
 * the list nor any schedule:
 *   root[v]    int32   the smallest node of v's component
 *   entries[v] uint64  the list entries with a[e] == v and a[e] != b[e]
 *   weight[v]  uint64  the sum of shared[e] over those entries (shared == NULL: every entry counts 1)
 * The list may be unsorted, hold a pair in one direction only and hold an entry twice; an entry with a[e] == b[e] is ignored altogether.
 * A union-find forest in one array that only atomics write (a compare-and-swap hooks the larger root under the smaller, an atomic minimum
 * halves paths), entries and weight by 64-bit integer atomics after a run of equal a has been summed inside its wave, then one flattening
 * pass.  No thread waits for another.
 * pg_screen_components takes the list from the host: m entries (64-bit; uploaded in chunks of 2^24, so the device never holds the whole
 * list), 1 <= n <= 2^20.  PG_E_ARG, checked before anything is copied or replaced: n outside that range, an index outside [0, n), m > 0
 * with a NULL a or b.  *n_components_out = the number of components (the nodes with root[v] == v).
 * pg_screen_index_components takes it from the resident index instead: the bands band_first, band_first + band_step, ... are counted and
 * selected exactly as pg_screen_index_select does (same need, rule and band setting), and every band's kept triples are hooked and
 * accumulated where they stand on the device — no pair is copied to the host.  *n_pairs_out = the kept cells, what pg_screen_index_select
 * reports; the result is that of pg_screen_components over the list pg_screen_index_select + _read return for the same bands (dealt
 * bands: one forest per part, joined by pyani_amd.screen.merge_components).  The index, its latest selection and pg_screen_index_last
 * are left as they were.  PG_E_ARG as pg_screen_index_select.
 * The result stays RESIDENT in a state of its own, independent of the resident matrix and of the index, until the next ACCEPTED
 * components call (a refused one leaves it readable), pg_screen_components_release (PG_OK when there is none), pg_clear_genomes or
 * pg_destroy.  pg_screen_components_read copies it out: n entries each; PG_E_ARG when there is none.
 * pg_screen_components_last: counts_out[4] = n, entries worked (a != b), entries ignored (a == b), components; ms_out[3] = band count +
 * select (the index path only), hook + accumulate, flatten milliseconds (HIP events on the context's stream); all 0 when nothing is
 * resident. */
int pg_screen_components(pg_ctx* ctx, const int32_t* a, const int32_t* b, const uint32_t* shared, uint64_t m, uint32_t n, uint32_t* n_components_out);
int pg_screen_index_components(pg_ctx* ctx, const uint32_t* need, uint32_t n, uint32_t band_first, uint32_t band_step, uint32_t* n_components_out,
                               uint64_t* n_pairs_out);
int pg_screen_components_read(pg_ctx* ctx, int32_t* root_out, uint64_t* entries_out, uint64_t* weight_out);
int pg_screen_components_last(pg_ctx* ctx, uint64_t* counts_out, double* ms_out);
int pg_screen_components_release(pg_ctx* ctx);

/* ---- screen, the representatives: one genome per cluster by the greedy rule.  The list of entries (a[e], b[e],
 * weight[e]) over n nodes is that of the components: unsorted, a pair in one direction or both, once or several times, direction ignored,
 * an entry with a[e] == b[e] ignored altogether; weight == NULL weighs every entry 1.  score[v] (uint64, greater is better, ties to the
 * smaller index) gives the priority: order = the nodes by (score descending, index ascending), rank its inverse.
 *   1. Walk `order`: a node none of whose neighbours is a representative yet becomes one.
 *   2. AFTER all representatives are known, every other node v goes to the representative neighbour r of the greatest pair weight (the
 *      maximum of weight[e] over the entries joining v and r), ties to the r of smaller rank — a representative of lower priority than v
 *      may take v.
 *   rep[v] int32   the representative v belongs to; rep[v] == v for a representative
 *   via[v] uint32  the pair weight v was assigned by; 0 for a representative
 * All integers that depend on neither the order, direction or duplication of the list nor any schedule
 * (pyani_amd.screen.representatives_of_pairs is the statement).  One stable radix sort of (~score, index) gives the ranks.  The walk is
 * the lexicographically first maximal independent set under `rank`, reproduced by rounds of three launches over the entries — both ends
 * undecided: the end of larger rank is stamped; an undecided node not stamped becomes a representative; an undecided end opposite a
 * representative is covered — so that a node becomes a representative exactly when all its neighbours of higher priority are covered.
 * Every round decides at least the undecided node of smallest rank: at most n rounds (1-4 on clique-like graphs, n / 2 on a chain whose
 * scores fall along it), issued in batches with one read of the control words per batch.  The assignment is a 64-bit atomic maximum of
 * weight << 32 | 0xFFFFFFFF - rank[r] per covered node.  No thread waits for another.
 * pg_screen_representatives takes the list from the host and uploads it WHOLE (12 bytes an entry, 8 without weights: the rounds read it
 * repeatedly), 1 <= n <= 2^20.  PG_E_ARG, checked before anything is copied or replaced: n outside that range, an index outside [0, n),
 * m > 0 with a NULL a or b, a NULL score.  *n_representatives_out = the nodes with rep[v] == v.
 * pg_screen_index_representatives takes it from the resident index instead: ALL bands are counted and selected exactly as
 * pg_screen_index_select does (same need, rule and band setting), and every band's kept triples with a < b — the rule is symmetric, so
 * half is the whole graph — are appended to a list on the device, 12 bytes per undirected kept pair; no pair is copied to the host.
 * *n_pairs_out = the kept cells (both directions), what pg_screen_index_select reports; the result is that of pg_screen_representatives
 * over the list pg_screen_index_select + _read return.  The index, its latest selection and pg_screen_index_last are left as they were.
 * PG_E_ARG as pg_screen_index_select (no resident index, a `need` length that is not the index's n), and for a NULL score.
 * The result stays RESIDENT in a state of its own, independent of the resident matrix, the two indexes and the components, until the next
 * ACCEPTED representatives call (a refused one leaves it readable; an allocation that fails replaces nothing),
 * pg_screen_representatives_release (PG_OK when there is none), pg_clear_genomes or pg_destroy.  pg_screen_representatives_read copies it
 * out: n entries each; PG_E_ARG when there is none.
 * pg_screen_representatives_last: counts_out[6] = n, entries worked (the list entry: those with a != b; the index entry: the undirected
 * kept pairs), entries ignored (a == b), representatives, rounds, launches of the round kernels; ms_out[4] = band count + select (the
 * index path only), rank sort, rounds, assign milliseconds (HIP events on the context's stream); all 0 when nothing is resident. */
int pg_screen_representatives(pg_ctx* ctx, const int32_t* a, const int32_t* b, const uint32_t* weight, uint64_t m, uint32_t n, const uint64_t* score,
                              uint32_t* n_representatives_out);
int pg_screen_index_representatives(pg_ctx* ctx, const uint32_t* need, uint32_t n, const uint64_t* score, uint32_t* n_representatives_out, uint64_t* n_pairs_out);
int pg_screen_representatives_read(pg_ctx* ctx, int32_t* rep_out, uint32_t* via_out);
int pg_screen_representatives_last(pg_ctx* ctx, uint64_t* counts_out, double* ms_out);
int pg_screen_representatives_release(pg_ctx* ctx);

/* ---- screen, the sweep: the components over a ladder of thresholds in ONE pass.  The list of entries (a[e], b[e],
 * shared[e]) over n nodes is that of the components (unsorted, a pair in one direction or both, once or several times, an entry with
 * a[e] == b[e] ignored altogether; shared == NULL weighs every entry 1), and every entry carries level[e] (uint16) in 0 ... steps: the
 * number of leading steps of the ladder that keep it.  The entry is present at step s iff level[e] > s, so the graphs of the steps are
 * nested.  For every step s of 0 ... steps - 1, over the entries with a != b present at s:
 *   entries[s]    uint64  their number
 *   components[s] uint32  the connected components over all n nodes, singletons included
 *   singletons[s] uint32  the components of one node
 *   largest[s]    uint32  the size of the largest component
 *   pair_slots[s] uint64  the sum over the components of size * (size - 1)
 * and, for every step named in snapshot_steps (at most 32, each < steps; a step may be named twice), the three node arrays root, entries,
 * weight that pg_screen_components gives on the entries present at that step.  All integers that depend on neither the order of the list
 * nor any schedule (pyani_amd.screen.sweep_of_pairs is the statement).  The entries are bucketed by level with one stable radix sort and
 * hooked bucket after bucket, from level `steps` down, into ONE forest of the kind pg_screen_components builds; after every non-empty
 * bucket a census of the forest gives the step's row, and a step whose bucket is empty has the row of the step above it.
 * pg_screen_sweep takes the list from the host and keeps it WHOLE on the device for the sort (14 bytes an entry, 10 without weights, twice
 * during the call), 1 <= n <= 2^20, 1 <= steps <= 4096.  PG_E_ARG, checked before anything is copied or replaced: n or steps outside
 * their range, more than 32 snapshots or a snapshot step >= steps, m > 0 with a NULL a, b or level, an index outside [0, n), a level
 * greater than steps.
 * pg_screen_index_sweep takes the list from the resident index instead: need is a table uint32[steps][n], row s the thresholds of step s
 * (pyani_amd.screen.sweep_thresholds), every column non-decreasing in s.  The bands band_first, band_first + band_step, ... are counted
 * and selected by ROW 0 exactly as pg_screen_index_select does; every kept triple gets its level on the device — the first step s with
 * shared < min(need[s][a], need[s][b]), or steps — and is appended to a list there; no pair is copied to the host.  *n_pairs_out = the
 * kept cells, what pg_screen_index_select reports for row 0; the result is that of pg_screen_sweep over that list.  The index, its latest
 * selection and pg_screen_index_last are left as they were.  PG_E_ARG as above and as pg_screen_index_select (no resident index, n that is
 * not the index's), for steps * n > 2^28 (the table's 1 GB) and for a table with a column that falls.
 * The result stays RESIDENT in a state of its own, independent of the resident matrix, the indexes, the components and the
 * representatives, until the next ACCEPTED sweep call (a refused one leaves it readable; an allocation that fails replaces nothing),
 * pg_screen_sweep_release (PG_OK when there is none), pg_clear_genomes or pg_destroy.  pg_screen_sweep_read copies the five per-step
 * arrays out, `steps` entries each; pg_screen_sweep_read_snapshot the node arrays of snapshot k (its position in snapshot_steps), n
 * entries each; PG_E_ARG when there is no sweep or no such snapshot.
 * pg_screen_sweep_last: counts_out[6] = n, steps, entries worked (those with a != b), entries ignored (a == b), worked entries of level 0
 * (present at no step), non-empty buckets (= censuses); ms_out[4] = band count + select + levels (the index path only), histogram + sort,
 * hook + accumulate, census milliseconds (HIP events on the context's stream); all 0 when nothing is resident. */
int pg_screen_sweep(pg_ctx* ctx, const int32_t* a, const int32_t* b, const uint32_t* shared, const uint16_t* level, uint64_t m, uint32_t n, uint32_t steps,
                    const uint32_t* snapshot_steps, uint32_t n_snapshots);
int pg_screen_index_sweep(pg_ctx* ctx, const uint32_t* need, uint32_t n, uint32_t steps, uint32_t band_first, uint32_t band_step, const uint32_t* snapshot_steps,
                          uint32_t n_snapshots, uint64_t* n_pairs_out);
int pg_screen_sweep_read(pg_ctx* ctx, uint64_t* entries_out, uint32_t* components_out, uint32_t* singletons_out, uint32_t* largest_out, uint64_t* pair_slots_out);
int pg_screen_sweep_read_snapshot(pg_ctx* ctx, uint32_t k, int32_t* root_out, uint64_t* entries_out, uint64_t* weight_out);
int pg_screen_sweep_last(pg_ctx* ctx, uint64_t* counts_out, double* ms_out);
int pg_screen_sweep_release(pg_ctx* ctx);

/* ---- screen, the linkage: species clusters by average or complete linkage inside every connected component.  The
 * list of entries (a[e], b[e], dist[e]) over n nodes is that of the components (unsorted, a pair in one direction or both, once or several
 * times, an entry with a[e] == b[e] ignored altogether); dist[e] is a finite double >= 0.
 *   1. root[v] = the smallest node of v's connected component (pg_screen_components' root); the local index of a node is its position
 *      among its component's members in ascending order.
 *   2. Per component of s >= 2 nodes an s x s matrix: D[i][j] = the MAXIMUM of dist[e] over the entries joining the two nodes, in either
 *      direction; `fill` where no entry joins them; 0 on the diagonal.
 *   3. scipy's nearest-neighbour chain on it (method: PG_CLUSTER_AVERAGE or PG_CLUSTER_COMPLETE, the arithmetic and tie rules of
 *      pg_cluster_linkage): s - 1 merge records (lower slot, higher slot, height, size) in merge order, slots as local indices.
 *   4. Two nodes share a cluster iff merges of height <= cutoff join them (scipy's fcluster(Z, cutoff, "distance"));
 *      cluster[v] = the smallest node of v's cluster.
 *   5. rep[v] = the member of v's cluster of the greatest score (uint64, greater is better), ties to the smaller index.
 * Integers, and doubles whose bits the statement fixes (pyani_amd.screen.linkage_of_pairs); nothing depends on the list's order,
 * direction or duplication.  *n_clusters_out = the nodes with cluster[v] == v.
 * PG_E_ARG, checked before anything is copied or replaced: n outside 1 ... 2^20, an index outside [0, n), m > 0 with a NULL a, b or dist,
 * a NULL score, a distance that is not finite or below 0, a method other than the two, cutoff or fill not finite or below 0, cutoff not
 * STRICTLY below fill.  PG_E_CAPACITY for a component of more than 8192 nodes (the linkage kernel's own limit; the message names the size;
 * a tighter screen threshold splits such a component), found before any matrix is allocated.
 * The result stays RESIDENT in a state of its own, independent of every other resident screen state, until the next ACCEPTED linkage call
 * (a refused one leaves it readable; an allocation that fails replaces nothing), pg_screen_linkage_release (PG_OK when there is none),
 * pg_clear_genomes or pg_destroy.  pg_screen_linkage_read copies root, cluster and rep out, n entries each; pg_screen_linkage_read_merges
 * the n - components merge records, 4 doubles each: the components' blocks in ascending root order (merges_out may be NULL when there is
 * none).  PG_E_ARG when nothing is resident.
 * pg_screen_linkage_set: components of 2 ... small_limit nodes run one per WAVE, larger ones one per workgroup; small_limit is 0 (the
 * workgroup kernel only) ... 64, or PG_SCREEN_LINKAGE_DEFAULT; work_bytes is the budget for the working matrices (8 s^2 bytes a component)
 * of one batch, at most 2^40, 0 = the default (1 GiB); a component beyond the budget has a batch to itself.  Values out of range are
 * PG_E_ARG and change nothing.  The result does not depend on either setting.
 * pg_screen_linkage_last: counts_out[8] = n, entries worked (a != b), entries ignored (a == b), components, components of >= 2 nodes, the
 * largest component, clusters, batches; ms_out[5] = group, fill, wave linkage, workgroup linkage, cut + representatives milliseconds (HIP
 * events on the context's stream); all 0 when nothing is resident. */
#define PG_SCREEN_LINKAGE_DEFAULT 0xFFFFFFFFu
int pg_screen_linkage(pg_ctx* ctx, const int32_t* a, const int32_t* b, const double* dist, uint64_t m, uint32_t n, const uint64_t* score, int method, double cutoff,
                      double fill, uint32_t* n_clusters_out);
int pg_screen_linkage_read(pg_ctx* ctx, int32_t* root_out, int32_t* cluster_out, int32_t* rep_out);
int pg_screen_linkage_read_merges(pg_ctx* ctx, double* merges_out);
int pg_screen_linkage_set(pg_ctx* ctx, uint32_t small_limit, uint64_t work_bytes);
int pg_screen_linkage_last(pg_ctx* ctx, uint64_t* counts_out, double* ms_out);
int pg_screen_linkage_release(pg_ctx* ctx);

/* ---- screen, the evaluation: how good a partition of the kept pairs is.  The list of entries (a[e], b[e], weight[e])
 * over n nodes is that of the representatives (unsorted, a pair in one direction or both, once or several times, an entry with
 * a[e] == b[e] ignored altogether; weight == NULL weighs every entry 1).  label (int32[n]) is a partition given by naming nodes:
 * 0 <= label[v] < n and label[label[v]] == label[v] — rep of the representatives, cluster and rep of the linkage, root of the components.
 * score[v] (uint64, greater is better, ties to the smaller index) gives `rank` as for the representatives.
 * A PAIR is a distinct unordered {u, v}, u != v, joined by at least one entry; its weight is the MAXIMUM of weight[e] over those entries in
 * either direction.  It is INSIDE iff label[u] == label[v], otherwise OUTSIDE.  Per node v:
 *   in_pairs[v]   uint32  the inside pairs at v
 *   in_weight[v]  uint64  the sum of their weights
 *   in_min[v]     uint32  the smallest of them; 0xFFFFFFFF when in_pairs[v] == 0
 *   out_pairs[v]  uint32  the outside pairs at v
 *   out_weight[v] uint32, out_node[v] int32  the greatest outside pair weight at v and the node at its other end, ties to the smaller
 *                         node; 0, -1 when there is none (a pair of weight 0 gives 0 and its node)
 *   to_medoid[v]  uint32  the weight of the pair joining v and its cluster's medoid; 0 when there is none or v is the medoid
 * Per cluster, indexed by the naming node c = label[v] and meaningful where label[c] == c (0 or -1 elsewhere):
 *   size[c]   uint32  the members
 *   pairs[c], weight[c] uint64  the inside pairs and the sum of their weights
 *   min[c]    uint32  the weakest inside pair; 0xFFFFFFFF without one
 *   medoid[c] int32   the member of the greatest in_weight, ties to the smaller rank; the member itself in a singleton
 *   near_weight[c] uint32, near_cluster[c] int32  the greatest weight of a pair joining a member and a non-member and the label of the
 *                     non-member, ties to the smaller label; 0, -1 without one
 * All integers that depend on neither the order, direction or duplication of the list nor any schedule
 * (pyani_amd.screen.evaluate_of_pairs is the statement).  The distinct pairs come from one radix sort of the 40-bit keys
 * min(a, b) << 20 | max(a, b) (a self entry sorts last) and one reduce-by-key with maximum; the pair pass reduces runs of equal
 * destination inside a wave before its atomics; the outside maxima are 64-bit atomic maxima of weight << 32 | ~other, whose low word is
 * never 0, so that 0 means "no pair"; the medoid takes two node passes (the maximum of in_weight, then the minimum of rank among the
 * members that reach it).  No thread waits for another.
 * pg_screen_evaluate takes the list from the host and keeps it on the device for the sort (12 bytes an entry in, 24 while sorting),
 * 1 <= n <= 2^20.  PG_E_ARG, checked before anything is copied or replaced: n outside that range, a NULL label or score, a label outside
 * [0, n) or one that does not name itself (the message names the first such node), m > 2^32 - 1 (so that no 64-bit sum can overflow),
 * m > 0 with a NULL a or b, an index outside [0, n).
 * pg_screen_index_evaluate takes the list from the resident index instead, exactly as pg_screen_index_representatives does: ALL bands are
 * counted and selected as pg_screen_index_select does, every band's kept triples with a < b appended to a list on the device, which is
 * distinct already; no pair is copied to the host.  *n_pairs_out = the kept cells (both directions).  The index, its latest selection and
 * pg_screen_index_last are left as they were.  PG_E_ARG as pg_screen_index_select and as above.
 * The result stays RESIDENT in a state of its own, independent of every other resident screen state, until the next ACCEPTED evaluate
 * call (a refused one leaves it readable; an allocation that fails replaces nothing), pg_screen_evaluate_release (PG_OK when there is
 * none), pg_clear_genomes or pg_destroy.  pg_screen_evaluate_read copies the seven node arrays out and pg_screen_evaluate_read_clusters
 * the seven cluster arrays, n entries each; any pointer may be NULL (that array is skipped); PG_E_ARG when nothing is resident.
 * pg_screen_evaluate_last: counts_out[6] = n, entries worked (the list entry: those with a != b; the index entry: the undirected kept
 * pairs), entries ignored (a == b), distinct pairs, inside pairs, clusters; ms_out[4] = band count + select (the index path only),
 * canonicalise + sort + reduce (with the rank sort), pair passes, node passes milliseconds (HIP events on the context's stream); all 0
 * when nothing is resident. */
int pg_screen_evaluate(pg_ctx* ctx, const int32_t* a, const int32_t* b, const uint32_t* weight, uint64_t m, uint32_t n, const int32_t* label, const uint64_t* score);
int pg_screen_index_evaluate(pg_ctx* ctx, const uint32_t* need, uint32_t n, const int32_t* label, const uint64_t* score, uint64_t* n_pairs_out);
int pg_screen_evaluate_read(pg_ctx* ctx, uint32_t* in_pairs_out, uint64_t* in_weight_out, uint32_t* in_min_out, uint32_t* out_pairs_out, uint32_t* out_weight_out,
                            int32_t* out_node_out, uint32_t* to_medoid_out);
int pg_screen_evaluate_read_clusters(pg_ctx* ctx, uint32_t* size_out, uint64_t* pairs_out, uint64_t* weight_out, uint32_t* min_out, int32_t* medoid_out,
                                     uint32_t* near_weight_out, int32_t* near_cluster_out);
int pg_screen_evaluate_last(pg_ctx* ctx, uint64_t* counts_out, double* ms_out);
int pg_screen_evaluate_release(pg_ctx* ctx);

/* ---- screen, the search: new genomes against a resident collection.  S(g), size, kmer and scale as for
 * pg_screen_matrix.  A collection ("db") of n <= 2^20 genomes is indexed once; then, per call, q query genomes are placed against it:
 *   hits[i][b] = |S(query i) & S(db b)|, a q x n rectangle of uint32, row-major
 * There is NO diagonal: a query that is also a db genome meets itself with hits = size, a cell like any other.  The rule of
 * pg_screen_select on the rectangle: (i, b) kept iff hits[i][b] >= min(need_q[i], need_db[b]) — exactly the cells (a in queries, b in db)
 * that pg_screen_select over db + queries keeps.  Integers only; no result depends on a schedule, a slice or a chunk.
 * pg_screen_search_index scans, sorts and groups as pg_screen_index does (slices under pg_screen_set_budget) and keeps EVERY distinct
 * k-mer — its value, and the call indices of its holders, singletons included — with a directory from slice bin to slice.  Arguments
 * and refusals as pg_screen_index; sizes_out: n uint32.  The index is a state of its own, independent of the resident matrix, of the
 * index of pg_screen_index and of the components; it names the db genomes by call index only and reads nothing of the genome store
 * after the build, so it SURVIVES pg_clear_genomes: index a collection, clear the store, load query batches into the freed memory.  It
 * lives until the next pg_screen_search_index whose arguments pass (the old index goes first), pg_screen_search_index_release (PG_OK
 * when there is none) or pg_destroy.  n = 0 is accepted and leaves no index.
 * pg_screen_search_count places q resident genomes (ids of the genome store as it is NOW; none twice) against the index, with the
 * index's kmer and scale: q <= the band's rows (pg_screen_set_band; the default here min(8192, 2^29 / n): a rectangle of at most 2 GiB).
 * The queries' keys are sliced under pg_screen_set_budget on their own; per slice every distinct query k-mer is looked up (bin -> slice,
 * binary search) and every (query holder, db holder) pair of a matched k-mer adds one to its cell.  sizes_out: q uint32, the queries'
 * sizes.  The rectangle stays resident until the next accepted count, the release or pg_destroy.
 * pg_screen_search_select applies the rule to the resident rectangle (q and n must be the resident ones); *n_pairs_out = the kept
 * cells; pg_screen_search_read copies them out row-major: a_out (0 ... q - 1, the query's position in the count call), b_out (the db
 * genome's position in the index call) int32, shared_out uint32; the arrays may be NULL when nothing was kept.
 * pg_screen_search_fetch copies the rectangle out (q x n uint32).
 * PG_E_ARG, before anything is replaced: no resident search index; n or q not the resident ones; q above the band's rows; a query id
 * out of range or given twice; a NULL array with a non-zero count; select or fetch without a counted rectangle, read without a selection.
 * pg_screen_search_last: counts_out[10] = sampled keys, distinct k-mers D, (k-mer, genome) entries E, slices of the resident index | of
 * the latest count: the queries' keys, their distinct k-mers (= lookups), the matched ones, increments of the count kernel (= the sum
 * of the rectangle), slices | the device bytes the index's buffers HOLD (their allocated sizes: about 12 D + 4 E once the arrays have
 * moved into blocks of their own size — an array within a sixteenth of its bound, or one there is no room to copy, stays in the
 * block sized by the keys).  ms_out[7] = scan, sort + group of the build | scan, sort + group, lookup (the mark of the runs, their
 * compaction, the lookup kernel, the matched runs' compaction), count (weights, scan, count kernel) of the latest count | its latest
 * selection (HIP events; no pair spans a host synchronisation).  All 0 without an index. */
int pg_screen_search_index(pg_ctx* ctx, const int32_t* genome_ids, uint32_t n, int32_t kmer, int32_t scale, uint32_t* sizes_out);
int pg_screen_search_index_release(pg_ctx* ctx);
int pg_screen_search_count(pg_ctx* ctx, const int32_t* query_ids, uint32_t q, uint32_t* sizes_out);
int pg_screen_search_select(pg_ctx* ctx, const uint32_t* need_q, uint32_t q, const uint32_t* need_db, uint32_t n, uint64_t* n_pairs_out);
int pg_screen_search_read(pg_ctx* ctx, int32_t* a_out, int32_t* b_out, uint32_t* shared_out);
int pg_screen_search_fetch(pg_ctx* ctx, uint32_t* out);
int pg_screen_search_last(pg_ctx* ctx, uint64_t* counts_out, double* ms_out);

/* ---- screen, the search: genomes added to the resident index without a rebuild.  An index built from the list L of n
 * genomes grows by m genomes of the store as it is NOW (genome_ids; none twice): afterwards the state is the one
 * pg_screen_search_index(L ++ genome_ids) with the index's kmer and scale would leave — n' = n + m, added genome j is column n + j, D and
 * E are the fresh build's, and every later count, selection, fetch and gather gives the fresh build's integers in the fresh build's order.
 * Only the cut into slices may differ (nothing observable depends on it).  sizes_out: m uint32, the added genomes' sizes.
 * The ids are NOT compared with the collection — the index knows positions, not ids: a genome added in two calls is two equal columns.
 * So a collection larger than the genome store is indexed in batches: load, index, clear; load, add, clear; ...
 * PG_E_ARG, before anything is touched (the index, the counted rectangle, the selection and the gather's state stay readable): no
 * resident search index; n + m above 2^20 (checked before the ids are read); an id out of range or given twice; a NULL array with m > 0.
 * m = 0 is PG_OK and changes nothing.  An accepted add with m >= 1 drops the counted rectangle, the selection and the gather's state, as
 * a new count does (they were n wide).  The merged index is built BESIDE the old one, its arrays at their exact sizes (D' + 1, D' + 1,
 * E' + 1), and takes its place only when the call has succeeded: on PG_E_NOMEM or any other failure after the checks the OLD index is
 * resident and usable (its rectangle is gone by then).  While the call runs the device holds both, the staged keys of the batch (twice 8
 * bytes each, and 22 bytes of work arrays) and 4 (D + 1) bytes; between calls never more than one index.
 * After an add the index fields of pg_screen_search_last (keys — the sum over the build and the adds —, D, E, slices, bytes held)
 * describe the merged index.
 * pg_screen_search_add_last: the latest accepted add.  counts_out[6] = added genomes, keys scanned, new entries, new k-mers (absent
 * before), matched k-mers (present before), accepted adds since the build.  ms_out[3] = scan, sort + group (the front's and the staged
 * keys' sort into the index's order), merge (locate, scans, placement, the copy of the index) — HIP events; no pair spans a host
 * synchronisation.  All 0 after a build, a release, or without an index. */
int pg_screen_search_index_add(pg_ctx* ctx, const int32_t* genome_ids, uint32_t m, uint32_t* sizes_out);
int pg_screen_search_add_last(pg_ctx* ctx, uint64_t* counts_out, double* ms_out);

/* ---- screen, the search: the resident index exported, imported and shrunk — with the build and the add, the operations
 * of a database one maintains.  The index is six plain arrays and seven numbers:
 *   shape[7] = n, kmer, scale, D (distinct k-mers), E (entries), n_slices S, keys (the scan count pg_screen_search_last reports)
 *   kmer uint32[D], start uint64[D + 1], member uint32[E], slice_first uint64[S + 1], bin_slice uint32[4096]
 * (the sixth array, the genomes' sizes, is a function of member: it is never stored on the device and never believed).
 * pg_screen_search_index_shape and pg_screen_search_index_export copy these out and change nothing: the counted rectangle, the selection
 * and the gather's state stay.  PG_E_ARG without a resident index.
 * pg_screen_search_index_import uploads arrays that a FILE supplied and leaves exactly the state the exporting context had: every later
 * count, selection, fetch, gather and add gives the same integers in the same order, and the index fields of pg_screen_search_last (keys,
 * D, E, slices) are the exporter's; the arrays sit at their exact sizes: bytes held = 12 (D + 1) + 4 (E + 1) + 8 (S + 1) + 4 * 4096.
 * sizes_out: n uint32, COMPUTED from the entries (a count per column).  Nothing of the file is trusted.  The host checks, before anything
 * is uploaded: n <= 2^20, 8 <= kmer <= 16, scale a power of two <= 65536, E >= D, S <= 4096; n = 0 needs D = E = 0 and leaves no index
 * (an earlier one is released, as pg_screen_search_index does); slice_first[0] = 0, non-decreasing, slice_first[S] = D; every bin_slice
 * value < S or 0xFFFFFFFF (no slice).  Then the device validates every invariant the build guarantees, in an order in which no pass
 * indexes by a value an earlier pass has not validated: start[0] = 0, start[D] = E, start strictly increasing (every k-mer has a holder);
 * every k-mer < 4^kmer, sampled under scale, in the slice its bin names, strictly ascending inside a slice; only when the starts are sound
 * are the entries walked by them: every member < n, strictly ascending inside a k-mer.  One counter per kind is read back once; a nonzero
 * one is PG_E_ARG and the message names the first violated invariant and its count.  The imported index is built BESIDE any resident one
 * and takes its place only on success: after any refusal the old index and its rectangle are resident and usable, after any other failure
 * the old index.  ms_out[1] of pg_screen_search_last (sort + group of the build) holds the validation's milliseconds for an imported index,
 * ms_out[0] is 0.
 * pg_screen_search_index_remove takes m columns (current call indices; each < n, none twice) out of the index: afterwards the state is
 * the one pg_screen_search_index over the list without those genomes would leave — n' = n - m, surviving column c becomes c - (removed
 * columns below c), D' and E' are the fresh build's, holders ascend inside a k-mer, k-mers with no holder left are gone.  As for the add
 * only the cut into slices may differ: the directory keeps its slice count with slice_first rebased, and a slice may become empty.
 * PG_E_ARG before anything is touched: no resident index; a NULL array with m > 0; a column >= n or given twice.  m = 0 is PG_OK and
 * changes nothing.  Removing every column releases the index, as a build of no genome leaves none.  An accepted remove drops the counted
 * rectangle, the selection and the gather's state; the new index is built beside the old one at its exact sizes and replaces it on
 * success: on PG_E_NOMEM the old one is still resident.  While the call runs the device holds both, 8 (E + 1) + 8 (D + 1) + 4 n bytes of
 * positions and the scans' temporary storage.  The old entries are read twice and written once.  The `keys` field of
 * pg_screen_search_last is a HISTORICAL scan count (the build's and the adds'): a remove does not change it; D, E and the bytes held
 * describe the shrunk index.
 * pg_screen_search_remove_last: the latest accepted remove.  counts_out[4] = removed genomes, removed entries, removed k-mers, accepted
 * removes since the build or the import.  ms_out[2] = mark + scans, compaction (HIP events; no pair spans a host synchronisation).  All 0
 * after a build, an import, a release, or without an index. */
int pg_screen_search_index_shape(pg_ctx* ctx, uint64_t* shape_out);
int pg_screen_search_index_export(pg_ctx* ctx, uint32_t* kmer_out, uint64_t* start_out, uint32_t* member_out, uint64_t* slice_first_out,
                                  uint32_t* bin_slice_out);
int pg_screen_search_index_import(pg_ctx* ctx, const uint64_t* shape, const uint32_t* kmer, const uint64_t* start, const uint32_t* member,
                                  const uint64_t* slice_first, const uint32_t* bin_slice, uint32_t* sizes_out);
int pg_screen_search_index_remove(pg_ctx* ctx, const uint32_t* columns, uint32_t m);
int pg_screen_search_remove_last(pg_ctx* ctx, uint64_t* counts_out, double* ms_out);

/* ---- screen, the gather: a query decomposed into the collection's genomes.  For query i with Q = S(query i), R_0 = Q and
 * round t = 0, 1, ...: left_t[b] = |R_t & S(b)|; the winner w = the SMALLEST b among those with the largest left_t[b]; the query stops
 * when left_t[w] < need[i] or when it has max_ranks rows; otherwise the row (i, rank t, w, unique = left_t[w], total = hits[i][w]) is
 * recorded and R_(t + 1) = R_t \ S(w).  The queries of a call are independent.  Integers only: unique never rises along a query's
 * ranks, unique <= total, a winner's cell of `left` is 0 afterwards, and a query has at most min(n, max_ranks) rows.
 * pg_screen_gather_count is pg_screen_search_count — the same limits, refusals, rectangle and statistics; select, read and fetch work on
 * it as before — and also keeps the matched entries resident, one per (query, matched k-mer): at most the queries' keys, 8 bytes each.
 * pg_screen_search_count keeps none: either count drops what the earlier one held, the entries and the gathered rows included.
 * pg_screen_gather runs the rounds on a working copy of the rectangle and of the entries (the counted rectangle and the kept entries are
 * never written: a selection, or another gather with other thresholds, may follow).  need: q uint32 >= 1, the smallest unique count worth
 * a row; 1 <= max_ranks <= 65536; *n_rows_out = the rows of all queries.  PG_E_ARG, with any earlier result still readable: no resident
 * search index; a latest count that kept no entries; q not the counted q; need NULL with q > 0; max_ranks out of range.  q = 0: no rows.
 * pg_screen_gather_read copies the rows out, ordered by query, then rank: query_out, db_out int32 (positions in the count and the index
 * call), unique_out, total_out uint32; the arrays may be NULL when there is no row.  pg_screen_gather_fetch copies `left` out (q x n
 * uint32): what the rounds left of the rectangle.  Both are PG_E_ARG without a gather.
 * pg_screen_gather_matched copies out, per query of the latest gather count, its kept entries = |S(query i) & the union of the db| (q
 * uint32; PG_E_ARG without such a count): with it, the sum of a query's unique and what stayed unexplained add up to a known number.
 * pg_screen_gather_last: counts_out[5] = matched entries M of the latest gather count | of the latest gather: rounds run (the last
 * round in which a query was unfinished), rows, entries claimed, decrements issued.  ms_out[3] = the expansion of the entries (the
 * count's extra stage) | arg-max + decide, claim (with the entries' compaction) of the latest gather.  All 0 without either.
 * The gather's state goes with the next count, pg_screen_search_index_release and pg_destroy; it survives pg_clear_genomes. */
int pg_screen_gather_count(pg_ctx* ctx, const int32_t* query_ids, uint32_t q, uint32_t* sizes_out);
int pg_screen_gather(pg_ctx* ctx, const uint32_t* need, uint32_t q, uint32_t max_ranks, uint64_t* n_rows_out);
int pg_screen_gather_read(pg_ctx* ctx, int32_t* query_out, int32_t* db_out, uint32_t* unique_out, uint32_t* total_out);
int pg_screen_gather_fetch(pg_ctx* ctx, uint32_t* out);
int pg_screen_gather_matched(pg_ctx* ctx, uint32_t* matched_out);
int pg_screen_gather_last(pg_ctx* ctx, uint64_t* counts_out, double* ms_out);

/* ---- screen, the gather's abundances: per-row statistics of the k-mers' multiplicities.  a(i, x) = the number of
 * windows of query i, over all its records, that the scan samples and whose canonical k-mer is x (uint32).  W[i] = the sum of a(i, x)
 * over x in S(query i); MW[i] = the same sum over the matched entries of query i.  Abundance does not move a winner: the rounds, the
 * rows and their order are pg_screen_gather's.  The matched entry (i, x) belongs to the row of the SMALLEST rank among the holders of x
 * that won in query i, and to no row if none of them won: row (i, t) owns exactly the `unique` k-mers it claimed.  Over the sorted
 * multiplicities a_0 <= ... <= a_(m - 1) of a row's k-mers (m = unique): sum, sumsq = the sum of squares as two uint64 words (lo, hi),
 * min, max, and median2 = a_((m - 1) / 2) + a_(m / 2) (integer division): twice the median, exact for both parities.  Integers only.
 * pg_screen_gather_count_abund IS pg_screen_gather_count — the same limits, refusals, rectangle, sizes, entries and statistics; select,
 * read, fetch, pg_screen_gather and pg_screen_gather_matched work on it unchanged — and also keeps a(i, x) of every entry (4 bytes each)
 * and copies W out: weight_out, q uint64 (may be NULL when q = 0).
 * pg_screen_gather_abund runs the pass over the latest gather of such a count; *n_rows_out = the gather's rows.  PG_E_ARG, with any
 * earlier result still readable: no resident search index; a latest count that kept no abundances; no pg_screen_gather since that
 * count.  PG_E_NOMEM (the message names the size) when the pass's q x n uint32 rank table does not fit; PG_E_INTERNAL when one of the
 * pass's own checks fails; either leaves the earlier results readable.  q = 0 or no rows: 0 rows.  Every pg_screen_gather drops the
 * statistics of the gather before it: run the pass again after it.
 * pg_screen_gather_abund_read copies the statistics out, in the rows' order: sum_out uint64[r], sumsq_out uint64[2 r] (row j: words 2 j
 * = lo, 2 j + 1 = hi), median2_out uint64[r], min_out, max_out uint32[r]; the arrays may be NULL when there is no row.  PG_E_ARG
 * without a pass.  pg_screen_gather_abund_matched copies MW out (q uint64; PG_E_ARG without such a count).
 * pg_screen_gather_abund_last: counts_out[4] = of the latest pass: entries that belong to a row, entries that belong to none, holders
 * walked, bytes of the rank table.  ms_out[4] = the weights of the latest abundance count (its extra stage beside the expansion) | of the
 * latest pass: rank table + attribute, sort, row statistics.  All 0 without either.
 * The state goes and stays as the gather's does. */
int pg_screen_gather_count_abund(pg_ctx* ctx, const int32_t* query_ids, uint32_t q, uint32_t* sizes_out, uint64_t* weight_out);
int pg_screen_gather_abund(pg_ctx* ctx, uint64_t* n_rows_out);
int pg_screen_gather_abund_read(pg_ctx* ctx, uint64_t* sum_out, uint64_t* sumsq_out, uint64_t* median2_out, uint32_t* min_out, uint32_t* max_out);
int pg_screen_gather_abund_matched(pg_ctx* ctx, uint64_t* matched_weight_out);
int pg_screen_gather_abund_last(pg_ctx* ctx, uint64_t* counts_out, double* ms_out);

/* ---- screen, the profile: core, private and marker k-mers of every cluster.  Over the resident search index — n genomes,
 * D k-mers, E entries, H(d) the holders of k-mer d and h(d) = |H(d)| >= 1 — and a partition label int32[n] in the convention of
 * pg_screen_evaluate (label[label[v]] == label[v]; a cluster is named by the node c = label[v]; size[c] its members), with two thresholds
 * per cluster, read at naming nodes only: 1 <= shell_need[c] <= core_need[c] <= size[c].
 * A CELL is a pair (d, c) with occ(d, c) = |H(d) & c| > 0.  It is core iff occ == size[c]; soft iff occ >= core_need[c]; shell iff
 * shell_need[c] <= occ < core_need[c]; private iff occ == h(d) (no holder outside c); a marker iff private and soft.
 * Per cluster, n entries indexed by the naming node, 0 where label[c] != c: size uint32; kmers, core, soft, shell, private, marker
 * uint64, the cluster's cells of each kind (kmers: all of them).
 * Spectrum, uint64[n]: with the clusters in ascending order of their naming nodes and off the exclusive prefix sum of their sizes,
 * spectrum[off[c] + occ - 1] = the cells of c with that occ: a cluster's words add up to kmers[c], the last of them is core[c].
 * Per genome v of cluster c, uint32[n]: held = |S(v)|; core_held = its k-mers whose cell in c is soft; private_held = those whose cell in
 * c is private; alone = those with occ(d, c) == 1; foreign = those of alone with h(d) > 1 (shared with other clusters only).
 * Marker list: the marker cells of the clusters with size >= marker_min_size, as (cluster int32, the k-mer's value uint32, occ uint32),
 * by ascending cluster, then by the k-mer's position in the index.  marker[c] counts every cluster whatever marker_min_size is.
 * Integers only, equal to a statement (pyani_amd.screen.profile_of_index); nothing depends on a schedule, a tier, a batch or the index's
 * cut into slices.  The k-mers go three ways by h(d): up to lane_limit holders one thread each, up to wave_limit one wave each, the others
 * through a radix sort of (k-mer, cluster, member) keys in batches of at most batch_keys entries cut at k-mer boundaries (a larger k-mer
 * is a batch of its own); pg_screen_search_profile_set: lane_limit 0 ... 8, wave_limit 0 ... 64 (a wave limit below the lane limit counts
 * as the lane limit), either PG_SCREEN_PROFILE_DEFAULT; batch_keys 0: the budget of pg_screen_set_budget.  PG_E_ARG beyond those.
 * pg_screen_search_profile: *n_markers_out = the entries of the list (may be NULL).  PG_E_ARG, before anything is replaced: no resident
 * search index; n outside 1 ... 2^20 or not the index's; a NULL array; a label outside [0, n) or one that does not name itself (the message names the first such
 * node); a naming node whose thresholds break the inequality (sizes come from label; the message names the node); marker_min_size == 0.
 * The result is a resident state of its own until the next ACCEPTED profile (an allocation that fails replaces nothing),
 * pg_screen_search_profile_release (PG_OK when there is none) or pg_destroy; it reads nothing of the genome store and survives
 * pg_clear_genomes, as the index does.  The call reads the index and changes nothing else: the index, the counted rectangle, the selection
 * and the gather's state stay exactly as they were.
 * pg_screen_search_profile_read copies the five genome arrays out, _read_clusters the seven cluster arrays, _read_spectrum the spectrum
 * (n entries each), _read_markers the list's three columns; any pointer may be NULL (that array is skipped); PG_E_ARG without a profile.
 * pg_screen_search_profile_last: counts_out[10] = n, clusters, D, E, cells, k-mers of the lane tier, of the wave tier, of the sorted tier,
 * batches of the sorted tier, markers listed; ms_out[5] = relabel, lane tier, wave tier (with its selection), sorted tier (selection, keys,
 * sort, runs, entries), markers milliseconds (HIP events; no pair spans a host synchronisation); all 0 when nothing is resident. */
#define PG_SCREEN_PROFILE_DEFAULT 0xFFFFFFFFu
int pg_screen_search_profile(pg_ctx* ctx, const int32_t* label, const uint32_t* core_need, const uint32_t* shell_need, uint32_t n, uint32_t marker_min_size,
                             uint64_t* n_markers_out);
int pg_screen_search_profile_read(pg_ctx* ctx, uint32_t* held_out, uint32_t* core_held_out, uint32_t* private_held_out, uint32_t* alone_out, uint32_t* foreign_out);
int pg_screen_search_profile_read_clusters(pg_ctx* ctx, uint32_t* size_out, uint64_t* kmers_out, uint64_t* core_out, uint64_t* soft_out, uint64_t* shell_out,
                                           uint64_t* private_out, uint64_t* marker_out);
int pg_screen_search_profile_read_spectrum(pg_ctx* ctx, uint64_t* spectrum_out);
int pg_screen_search_profile_read_markers(pg_ctx* ctx, int32_t* cluster_out, uint32_t* kmer_out, uint32_t* occ_out);
int pg_screen_search_profile_last(pg_ctx* ctx, uint64_t* counts_out, double* ms_out);
int pg_screen_search_profile_release(pg_ctx* ctx);
int pg_screen_search_profile_set(pg_ctx* ctx, uint32_t lane_limit, uint32_t wave_limit, uint64_t batch_keys);

/* ---- classify: clique sweep over identity thresholds ------------------------------------------------------------------
 * The compute of `pyani classify`.  These calls read caller matrices only: they touch no genome, seed list or ANIm worker slot, so
 * they need no interlock with the pg_anim_pairs_enqueue / _fetch lanes and may run while enqueued ANIm calls are in flight (own
 * kernels on the context's own stream; among themselves they are serialised by the caller, as every call on a context).
 *
 * pg_classify_edges replaces the pair loop of build_graph_from_results (pyani/pyani_classify.py:90-111).  identity / coverage: n x n
 * row-major fp64 (host), rows and columns in the same label order.  For every i < j: a = M[row j, col i], b = M[row i, col j],
 * weight = b if b < a else a (Python's min(a, b), its NaN order included), for both matrices; (i, j) is an edge iff
 * identity weight > id_min and coverage weight > cov_min.  *n_nodes_out = size of the reference's node set: every edge endpoint plus
 * every label except the last (pyani_classify.py:108), i.e. n, or n - 1 when the last genome has no edge.  The edge state (weights)
 * stays resident in the context until the next pg_classify_edges, pg_classify_release or pg_destroy.  n <= 8192 (PG_E_ARG beyond);
 * PG_E_NOMEM when the tables do not fit. */
int pg_classify_edges(pg_ctx* ctx, const double* identity, const double* coverage, uint32_t n, double id_min, double cov_min,
                      uint64_t* n_edges_out, uint32_t* n_nodes_out);
/* The identities of the resident edges, in no particular order (the caller sorts them: the edge list remove_low_weight_edges sorts,
 * pyani_classify.py:160, from which the thresholds of trimmed_graph_sequence follow, subcmd_classify.py:144-157).  cap >= n_edges. */
int pg_classify_edge_identities(pg_ctx* ctx, double* out, uint64_t cap);
/* The sweep of trimmed_graph_sequence (subcmd_classify.py:159-171) with analyse_cliques (pyani_classify.py:115-148) at every step.
 * theta[n_steps]: non-decreasing; step k sees exactly the resident edges with identity > theta[k] (the reference's step-by-step
 * removal of edges <= threshold, restated per step: the steps are independent).  Per step: n_subgraphs_out = number of connected
 * components over the node set, complete_out = 1 iff every node's degree equals its component's size - 1 (all_components_k_complete);
 * labels_out (may be NULL): n_steps x n int32, the smallest member index of the node's component, -1 for a genome outside the node
 * set.  Labels cost n_steps * n * 4 bytes of device and host memory per call: callers slice long threshold lists (any sub-list of a
 * sweep's thetas gives the same per-step answers).  PG_E_ARG without edge state or for a decreasing / NaN theta. */
int pg_classify_sweep(pg_ctx* ctx, const double* theta, uint64_t n_steps, int32_t* n_subgraphs_out, uint8_t* complete_out,
                      int32_t* labels_out);
/* Frees the edge state now (otherwise: the next pg_classify_edges or pg_destroy). */
int pg_classify_release(pg_ctx* ctx);

/* ---- heatmap clustering: distance matrix and linkage --------------------------------------------------------------------
 * The arithmetic that orders every heatmap of `pyani plot`.  Like the classify calls these read caller matrices only: they touch
 * no genome, seed list or ANIm worker slot, and keep nothing resident.  x: rows x cols float64, row-major.  columns = 0: the n = rows
 * rows are the observations (length cols); columns != 0: the n = cols columns are (length rows), read in place, no transposed copy.
 * Results EQUAL scipy's bit for bit (every operation rounded on its own, sums in k order).  n <= 8192 (PG_E_ARG beyond; the
 * observation length is unbounded); PG_E_NOMEM when a working matrix (8 n^2 bytes per problem) does not fit; PG_E_NONFINITE when any
 * distance is NaN or infinite (a NaN cell, an overflow), where scipy raises ValueError.
 *
 * pg_cluster_pdist replaces scipy.spatial.distance.pdist(dfr) / pdist(dfr.T), Euclidean (pyani/pyani_graphics/mpl/__init__.py:101
 * and :107): out holds the n (n - 1) / 2 distances in condensed order (0,1), (0,2), ..., (n-2,n-1).  n = 1 writes nothing. */
int pg_cluster_pdist(pg_ctx* ctx, const double* x, uint32_t rows, uint32_t cols, int columns, double* out);
#define PG_CLUSTER_COMPLETE 0 /* linkage(dists, method="complete"): pyani_graphics/mpl/__init__.py:128 */
#define PG_CLUSTER_AVERAGE 1  /* method="average": what sns.clustermap computes, pyani_graphics/sns/__init__.py:130 */
/* pg_cluster_linkage replaces pdist + scipy.cluster.hierarchy.linkage of add_dendrogram (pyani_graphics/mpl/__init__.py:100-128).
 * merges_out: (n - 1) x 4 float64, the nearest-neighbour chain's merge records (lower cluster slot, higher slot, height, size) in
 * MERGE order; a stable sort by height and the union-find relabelling (host, pyani_amd.graphics) turn them into scipy's Z.
 * n >= 2 (PG_E_ARG below: scipy raises ValueError on an empty distance vector). */
int pg_cluster_linkage(pg_ctx* ctx, const double* x, uint32_t rows, uint32_t cols, int columns, int method, double* merges_out);
/* The clusterings of a run in one call (pyani/scripts/subcommands/subcmd_plot.py:130-139: five matrices, rows and columns each):
 * distances per problem, then ONE linkage launch with a workgroup per problem.  Problems naming the same x / rows / cols share one
 * upload.  status: PG_OK or PG_E_NONFINITE per problem (merges untouched then); the call itself fails only for bad arguments, memory
 * or the runtime. */
typedef struct {
  const double* x;
  uint32_t rows, cols;
  int32_t columns, method;
  double* merges;      /* (n - 1) x 4 */
  int32_t status, reserved;
} pg_cluster_problem;
int pg_cluster_linkage_batch(pg_ctx* ctx, pg_cluster_problem* problems, uint32_t n_problems);

/* ---- distribution plots: histogram and Gaussian kernel density estimate -------------------------------------------------
 * The arithmetic of `pyani plot`'s distribution plots over all cells of a result matrix (five matrices per run,
 * pyani/scripts/subcommands/subcmd_plot.py:141-153).  Like the classify and cluster calls these read caller arrays only and may be
 * used on any context.  The values stay resident in the context from pg_dist_load until the next pg_dist_load, pg_dist_release or
 * pg_destroy.  Minimum, maximum and all counts are exact; the density sums are deterministic (their order is fixed at compile time:
 * two calls give the same bits on any launch).  The host owns what fixes floats: bin edges, grid, bandwidth, normalisation
 * (pyani_amd.graphics.distribution_data). */
typedef struct {
  double min, max;        /* over the non-NaN values, +-inf included (+inf, -inf when every value is NaN) */
  uint64_t n_nan, n_inf;  /* NaN cells; +inf and -inf cells */
} pg_dist_stats;
/* pg_dist_load replaces `data = dfr.values.flatten()` with `min(data)`, `max(data)` (pyani_graphics/mpl/__init__.py:149-150) and the
 * range scan of np.histogram: uploads the n float64 values and makes one pass over them.  n <= 8192 * 8192 (PG_E_ARG beyond);
 * PG_E_NOMEM when the values do not fit. */
int pg_dist_load(pg_ctx* ctx, const double* x, uint64_t n, pg_dist_stats* stats_out);
/* pg_dist_hist replaces the counting of `axes[0].hist(data, bins=50)` (pyani_graphics/mpl/__init__.py:152) and of histplot
 * (pyani_graphics/sns/__init__.py:204-211), i.e. np.histogram(data, edges)[0]: edges are n_bins + 1 ascending float64 (equal
 * neighbours allowed, not necessarily evenly spaced); value x is counted in the largest i with edges[i] <= x, x == edges[n_bins] in
 * the last bin; NaN and values outside [edges[0], edges[n_bins]] are not counted.  counts_out: n_bins uint64.  PG_E_ARG when nothing
 * is loaded, when an edge is NaN or below its predecessor, or for n_bins > 4096. */
int pg_dist_hist(pg_ctx* ctx, const double* edges, uint32_t n_bins, uint64_t* counts_out);
/* pg_dist_kde replaces the sum inside `density(xvals)` of scipy.stats.gaussian_kde (pyani_graphics/mpl/__init__.py:154-156; kdeplot,
 * pyani_graphics/sns/__init__.py:213): sums_out[j] = sum over the non-NaN values x of exp(-((points[j] - x) / bandwidth)^2 / 2), fp64;
 * the caller applies the normalisation.  PG_E_ARG when nothing is loaded, when the bandwidth is not finite and positive, or for
 * n_points > 1024. */
int pg_dist_kde(pg_ctx* ctx, const double* points, uint32_t n_points, double bandwidth, double* sums_out);
/* Frees the resident values now (otherwise: the next pg_dist_load or pg_destroy). */
int pg_dist_release(pg_ctx* ctx);
/* Kernel milliseconds of the latest pg_dist_load (the stats pass), pg_dist_hist and pg_dist_kde, in this order: HIP events on the
 * context's stream round the call's kernels, taken while pg_profile_enable is on; zeros when it is off.  (These kernels have no
 * PG_K_* slot: the slot count is published.) */
int pg_dist_last_ms(pg_ctx* ctx, double* out3);

/* ---- neighbour-joining tree of a distance matrix ------------------------------------------------------------------------
 * The unrooted tree of a collection from its distance matrix (an ANI, sketch or screen matrix turned into distances:
 * pyani_amd.tree).  Like the cluster calls these read a caller matrix only: they touch no genome, index or worker slot and keep
 * nothing resident but the counters below.  d: n x n float64, row-major, finite, symmetric bit for bit, zero diagonal; 3 <= n <= 8192.
 * Leaves are nodes 0 ... n - 1, join t (t = 0 ... n - 4) creates node n + t, the last node is 2 n - 3.
 * Results EQUAL pyani_amd.tree.nj_of_matrix, the numpy statement, integers exactly and doubles bit for bit: every operation is
 * rounded on its own, the row sums are carried and updated as the statement updates them, and equal criteria go to the smallest
 * (lower node id, higher node id).
 *   join_out      (n - 3) x 2 int32: the two nodes of every join, lower id first
 *   len_out       (n - 3) x 2 float64: their branch lengths to the new node (negative lengths as they come)
 *   last_out      3 int32: the three survivors by ascending id;  last_len_out  3 float64: their lengths to node 2 n - 3
 * Any of the four may be NULL.  PG_E_ARG, before any work: n < 3, n > 8192, a NULL matrix, an asymmetric cell, a non-zero diagonal.
 * PG_E_NONFINITE: a NaN or infinite cell, or a row sum or criterion that overflows.  PG_E_NOMEM when the working matrix (8 n^2 bytes)
 * does not fit.  A refused call leaves the four outputs untouched. */
int pg_tree_nj(pg_ctx* ctx, const double* d, uint32_t n, int32_t* join_out, double* len_out, int32_t* last_out, double* last_len_out);
/* From tail_limit live nodes down, one workgroup runs every remaining step in one launch; above it a step is two launches over the
 * whole device.  3 ... 1024 (PG_E_ARG outside, the setting unchanged); 3 runs every step wide.  The result does not depend on it. */
int pg_tree_nj_set(pg_ctx* ctx, uint32_t tail_limit);
/* The latest successful pg_tree_nj: counts_out 5 uint64 (n, wide steps, tail steps, kernel launches, cells the wide steps scanned: the
 * sum of m (m - 1) / 2 over them, dead slots are not scanned); ms_out 3 float64 (validation and row sums, wide steps, tail: HIP events
 * on the context's stream, taken while pg_profile_enable is on; zeros when it is off.  These kernels have no PG_K_* slot: the slot
 * count is published).  Either may be NULL. */
int pg_tree_nj_last(pg_ctx* ctx, uint64_t* counts_out, double* ms_out);

/* ---- measurement ---------------------------------------------------------------------------------------- */
/* When enabled, every kernel launch is bracketed by HIP events on the context's stream. */
int pg_profile_enable(pg_ctx* ctx, int on);
/* Restrict event bracketing to the kernels in `kernel_mask` (bit i = PG_K_*) and to every `every_n`-th launch of
 * each, so that measuring inside a timed region costs next to nothing.  Default: all kernels, every launch. */
int pg_profile_config(pg_ctx* ctx, uint32_t kernel_mask, uint32_t every_n);
int pg_profile_reset(pg_ctx* ctx);
#define PG_K_TETRA_COUNT 0
#define PG_K_TETRA_FINALIZE 1
#define PG_K_TETRA_STATS 2
#define PG_K_TETRA_PAIRS 3
/* ANIm stages (pg_anim_pairs); SEED, CLUSTER, EXTLANE and FINISH bracket exactly one kernel per launch, the others a
 * short group of kernels that belong together */
#define PG_K_ANIM_SEED 4     /* anim_seed_kernel: LDS-resident reference groups, streamed query lists */
#define PG_K_ANIM_HIT 5      /* anim_hoff_kernel + anim_hit_scatter_kernel + anim_hit_kernel + anim_scatter_kernel */
#define PG_K_ANIM_CLUSTER 6  /* anim_cluster_wave_kernel (one launch; + anim_cluster_prep_kernel when few units) */
#define PG_K_ANIM_GAPS 7     /* anim_postnuc_gaplist / gaplane<16,32,59> / gapbig kernels (match-to-match alignments) */
#define PG_K_ANIM_EXTLANE 8  /* anim_postnuc_forced_kernel (narrow bands) + anim_postnuc_forced_wide / _huge / _strips kernels */
#define PG_K_ANIM_EXTEND 9   /* anim_postnuc_kernel (the units' walks) */
#define PG_K_ANIM_FINISH 10  /* anim_finish_kernel */
#define PG_K_ANIB_BUCKET 11  /* anib_bucket_kernel: seeds clipped to fragments, counting sort by fragment */
#define PG_K_ANIB_FRAG 12    /* anib_frag_kernel: anchors + X-drop extensions, one wave per (pair, fragment) */
#define PG_K_ANIM_FWD 13     /* anim_postnuc_fwd_kernel: the forward extension off every cluster, ahead of the units' walks */
#define PG_K_ANIM_BWD 14     /* anim_postnuc_rehearse_kernel + anim_postnuc_bwd_kernel: the walks rehearsed, their backward searches run ahead */
#define PG_K_SKETCH_PAIRS 15 /* sketch_pairs_kernel: the sketch mode's containment pass (pg_sketch_pairs); sketch_map_kernel of the mapped mode too */
#define PG_K_CLASSIFY_EDGE 16  /* classify_edge_kernel: ordered minima, floors, edge list (pg_classify_edges) */
#define PG_K_CLASSIFY_SWEEP 17 /* classify_death_kernel + classify_sweep_kernel: one workgroup per threshold step (pg_classify_sweep) */
#define PG_K_CLUSTER_PDIST 18   /* cluster_pdist_kernel: Euclidean distances, upper-triangle tiles (pg_cluster_pdist, pg_cluster_linkage*) */
#define PG_K_CLUSTER_LINKAGE 19 /* cluster_linkage_kernel: nearest-neighbour chain, one workgroup per problem (pg_cluster_linkage*) */
#define PG_K__COUNT 20
/* PG_K__COUNT is a published value (slots 0 ... 19, the numbering callers were built against) and stays 20; index 20 itself is no slot
 * (pg_kernel_name(20) is ""), and slots added since carry on after it.  PG_K__END is one past the last slot: pg_profile_get and
 * pg_kernel_name accept 0 ... PG_K__END - 1, bit i of pg_profile_config's mask is slot i as before. */
#define PG_K_ANIB_ROWS_SCAN 21 /* anib_rows_scan1 / 2 / 3 kernels: exclusive scan of a launch's per-slot row counts (pg_anib_rows_batch) */
#define PG_K_ANIB_ROWS_PACK 22 /* anib_rows_pack_kernel: the live rows of a launch copied back to back, the pairs' row counts */
#define PG_K__END 23
/* total milliseconds and number of launches of kernel `which` since the last reset (synchronises). */
int pg_profile_get(pg_ctx* ctx, int which, double* total_ms_out, uint64_t* launches_out);
const char* pg_kernel_name(int which);

#ifdef __cplusplus
}
#endif
#endif /* PYANI_GPU_H */
