/*
 * mi355dr.h -- C ABI of the MI355X-native dense-retrieval core (libmi355dr.so).
 *
 * This is the drop-in boundary for AutoRAG-Research's Vector Search hot path.  The reference
 * has no FFI of its own for this path: it dispatches two SQL operators to PostgreSQL
 * extensions.  Each entry point below cites the reference call it replaces
 * (paths relative to /root/reference):
 *
 *   mi355dr_search / _device      <->  BaseVectorRepository.vector_search_with_scores
 *                                      autorag_research/orm/repository/base.py:378-426
 *                                      (SELECT id, embedding <=> q AS distance ... ORDER BY distance LIMIT k)
 *   mi355dr_search_maxsim         <->  BaseVectorRepository.maxsim_search / maxsim_search_with_ids
 *                                      autorag_research/orm/repository/base.py:487-535, 537-571
 *                                      (embeddings @# ARRAY[...] AS distance ... ORDER BY distance LIMIT k)
 *   mi355dr_add_rows / _device    <->  the `embedding VECTOR(d)` column fill
 *                                      autorag_research/orm/service/base_ingestion.py:199-247
 *   mi355dr_add_multivec          <->  BaseVectorRepository.set_multi_vector_embedding(s_batch)
 *                                      autorag_research/orm/repository/base.py:428-485
 *
 * Semantics (identical to oracle/oracle.c, which is the checker):
 *   - cosine distance = pgvector cosine_distance: fp32 accumulators dot/|q|^2/|c|^2 (k-ascending
 *     fused-multiply-add chains), double sim = dot/sqrt(nq*nc) clamped to [-1,1], distance = 1-sim
 *     returned as double (float8), NaN when a norm is zero.
 *   - inner product distance = (double)dot * -1 (pgvector <#>).
 *   - MaxSim distance = sum over query vectors of min over doc vectors of (-dot), fp32 (VectorChord @#).
 *   - exact brute force (the reference never builds an ANN index), total order
 *     (distance asc, NaN last, row index asc).
 *   - rows are addressed by dense row index in insertion order; the caller owns the
 *     row-index -> chunk-id table (ids may be BIGINT or VARCHAR, schema_factory.py:63-76).
 *
 * Conventions: every function returns 0 on success or a negative MI355DR_E_* code; the text of the
 * last error is available from mi355dr_last_error().  The caller owns all host buffers; the
 * library owns device memory.  One search in flight per handle (internal mutex); independent
 * handles are independent.  No Python / torch types cross this boundary.
 */
#ifndef MI355DR_H
#define MI355DR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi355dr_index mi355dr_index; /* opaque */

enum {
    MI355DR_OK = 0,
    MI355DR_E_INVALID = -1,     /* bad argument */
    MI355DR_E_HIP = -2,         /* HIP runtime error (text in last_error) */
    MI355DR_E_NOMEM = -3,       /* device or host allocation failed */
    MI355DR_E_UNSUPPORTED = -4, /* valid request this build cannot serve */
    MI355DR_E_INTERNAL = -5
};

enum { MI355DR_METRIC_COSINE = 0, MI355DR_METRIC_IP = 1 };

/* Search strategies (option "path"). */
enum {
    MI355DR_PATH_AUTO = 0,   /* screen where it applies, else scan */
    MI355DR_PATH_SCREEN = 1, /* MFMA screen over the normalised shadow corpus + exact fp32 re-score (both metrics) */
    MI355DR_PATH_SCAN = 2    /* exact fp32 chain per (query,row); slow, guaranteed, also the in-library fallback */
};

/* Element type of the screen pass (option "screen_dtype").  Both are exact end to end: the screen only
 * decides which rows are re-scored, under a rigorous per-query bound on |screen value - exact cosine|. */
enum {
    MI355DR_SCREEN_AUTO = 0, /* int8 when the corpus quantises within the residual limit, else bf16 */
    MI355DR_SCREEN_BF16 = 1, /* v_mfma_f32_32x32x16_bf16 over the bf16 shadow (bound ~0.0082 at d=768) */
    MI355DR_SCREEN_I8 = 2    /* v_mfma_i32_32x32x32_i8 over the int8 shadow (bound ~0.023): half the bytes, twice the rate */
};

/* ---- lifetime ---- */
int mi355dr_create(mi355dr_index** out, int device_id, int dim, int metric);
void mi355dr_destroy(mi355dr_index* idx);
/* idx may be NULL: returns the text of the last error raised before a handle existed */
const char* mi355dr_last_error(const mi355dr_index* idx);
int mi355dr_version(void);

/* ---- corpus (single-vector) ---- */
int mi355dr_reserve(mi355dr_index* idx, int64_t n_rows);
/* rows: host, row-major [n, dim] fp32.  Appends; copies to HBM; precomputes |c|^2 and the bf16 / int8 shadows. */
int mi355dr_add_rows(mi355dr_index* idx, const float* rows, int64_t n);
/* same, rows already resident on this index's device (e.g. an embedding model's output tensor) */
int mi355dr_add_rows_device(mi355dr_index* idx, const float* rows_dev, int64_t n);
/* stored slots, live or removed (row ids are stable: only mi355dr_compact renumbers, and says how) */
int64_t mi355dr_size(const mi355dr_index* idx);
int mi355dr_dim(const mi355dr_index* idx);

/* ---- update / remove in place ----
 * The table this index mirrors is not append-only: re-embedding a chunk is a second UPDATE of the same row
 * (orm/service/base_ingestion.py:199-247), and a row whose embedding became NULL -- or a deleted chunk -- leaves
 * `WHERE embedding IS NOT NULL` at once (orm/repository/base.py:409-415).
 *   update: row row_ids[j] takes rows[j]; every later search sees the index an add_rows of the new vector would have
 *           built (norm bits, both shadows, the irregular / loose classes).  Updating a removed row revives it.
 *   remove: the row is dead -- never returned by any path, metric or k.  Its slot stays (mi355dr_size counts it,
 *           mi355dr_get_rows returns its last vector); when k exceeds the live rows the tail is NaN / -1.  A dead row is
 *           not an irregular row (those are live and are returned last with NaN).  Removing a dead row is a no-op.
 * row_ids: HOST [n], each in [0, size) and listed once per call -- otherwise MI355DR_E_INVALID and nothing changes.
 * Each call first completes whatever search is in flight on the handle and is complete on return.  Cost: O(n) rows
 * rewritten + the int8 groups (32 rows) they fall into rebuilt + one 5-byte-per-row pass over the index that recounts
 * the side lists; the screens' two corpus-wide maxima (largest bf16 residual, largest norm) never shrink.
 * A search takes its first threshold from the first rows of the index (16 k; 64 k at 33 <= k <= 128): when fewer than k of
 * them are live -- the oldest rows all removed -- searches stay exact but fall back to slower paths; compact (or rebuild) such an index.
 * mi355dr_gqr_refine addresses rows directly and does not know removed rows: do not put them in a pool. */
int mi355dr_update_rows(mi355dr_index* idx, const int64_t* row_ids, const float* rows, int64_t n); /* rows: host [n, dim] */
/* the same with the new rows on this index's device ([n, dim] fp32); row_ids stay on the host */
int mi355dr_update_rows_device(mi355dr_index* idx, const int64_t* row_ids, const float* rows_dev, int64_t n);
int mi355dr_remove_rows(mi355dr_index* idx, const int64_t* row_ids, int64_t n);
/* mi355dr_size minus the removed rows (stat "dead_rows") */
int64_t mi355dr_live_rows(const mi355dr_index* idx);
/* ---- compaction ----
 * Drop every removed row: the live rows keep their relative order and become rows 0 .. live-1.
 * new_of_old: HOST [mi355dr_size() before the call] or NULL; entry r = the new id of old row r, -1 for a removed row.
 * The call runs under the handle's mutex, first completes whatever search is in flight (its outputs carry the OLD ids) and is
 * complete on return.  With no removed row it changes nothing, moves nothing and returns the identity map.  Afterwards
 * mi355dr_size == mi355dr_live_rows == the old live count, stat "dead_rows" is 0, and every reader -- mi355dr_get_rows, the
 * searches on every path, metric and screen_dtype, the stats "irregular_rows" / "loose_rows", the debug entry points --
 * answers like an index built fresh by ONE mi355dr_add_rows of the live rows in their order; exact distance ties break by
 * the new ids.  Live irregular and loose rows stay live, are listed under their new ids and are still returned last with NaN.
 * Capacity does not shrink: the freed tail is room for later adds (stat "hbm_bytes_resident" is unchanged).  The screens' two
 * monotone maxima (largest bf16 residual, largest norm) keep their values, as after a remove: candidate counts may differ
 * from a fresh index's, results do not.  AUTO's demotion of the int8 screen (option "screen_dtype") was a verdict on the old
 * layout -- a dead head overflows every int8 list -- and is re-armed, as setting that option does.
 * Works in place through a staging buffer of option "compact_slice_rows" rows (default 65536); every allocation happens
 * before the first byte of the index is written: MI355DR_E_NOMEM means nothing has changed.  A later failure can only be a
 * device error; the handle is then unusable and must be destroyed (DESIGN.md "Compaction").
 * Stats: "compactions" (calls that moved rows), "compact_moved_rows".
 * The map is local to this handle: option "row_offset" and the communicator are not touched -- a row-sharded caller owns the
 * renumbering across its shards.  Pools for mi355dr_gqr_refine must be rebuilt from the map.  The multi-vector store is untouched. */
int mi355dr_compact(mi355dr_index* idx, int64_t* new_of_old);
/* copy stored rows back (testing / cpu baseline): out host [n, dim] */
int mi355dr_get_rows(mi355dr_index* idx, int64_t row0, int64_t n, float* out);

/* ---- search (single-vector) ----
 * queries: [B, dim] fp32.  out_dist: [B, k] double, out_rows: [B, k] int64; slots beyond the
 * number of stored (live) rows hold NaN / -1.  row_offset is added to every returned row (shards). */
int mi355dr_search(mi355dr_index* idx, const float* queries, int B, int k, double* out_dist, int64_t* out_rows);
/* device-resident queries and outputs; stream = hipStream_t (NULL: the index's own stream).
 * Returns after the work is complete on that stream (it checks the device-side status word). */
int mi355dr_search_device(mi355dr_index* idx, const float* queries_dev, int B, int k, double* out_dist_dev,
                          int64_t* out_rows_dev, void* stream);
/* The same in two halves, so that consecutive blocks follow each other on the GPU without the host's round trip (the
 * reference's caller issues its queries back to back: pipelines/retrieval/vector_search.py:157-169; here a page of query
 * blocks).  _async puts the whole search on `stream` and returns a ticket without synchronising; the outputs are valid
 * after mi355dr_search_wait(ticket) returned MI355DR_OK: it waits for the block(s), reads their status words and, in the
 * rare case that a query overflowed a candidate list or cannot be screened, recomputes those queries (blocking) into the
 * same output buffers.  queries_dev and the output buffers must stay valid and untouched until the wait.  Up to 4 blocks
 * of 1024 queries may be in flight (a fifth first completes the oldest); blocks must be issued on ONE stream (a block on
 * another stream first completes what is in flight).  mi355dr_search_wait(idx, t) completes every block up to ticket t;
 * the synchronous entry points complete whatever is in flight first. */
int mi355dr_search_device_async(mi355dr_index* idx, const float* queries_dev, int B, int k, double* out_dist_dev,
                                int64_t* out_rows_dev, void* stream, int64_t* ticket);
int mi355dr_search_wait(mi355dr_index* idx, int64_t ticket);

/* ---- search within a listed subset of rows ----
 * The restricted form of the same statement: `WHERE embedding IS NOT NULL AND id = ANY(:ids) ORDER BY distance LIMIT k`
 * (orm/repository/base.py:409-415 with a key filter) -- re-ranking a lexical candidate list by dense similarity, a search
 * scoped to one document's chunks or one tenant, scoring a pool before a fusion.
 *   mi355dr_search_subset: the top-k of every query among the listed rows only.  The float8 distance bits, the total order
 *     (distance asc, NaN last, row asc) and the NaN / -1 tail when fewer than k listed rows are live are those of
 *     mi355dr_search; the order of the list never matters.
 *   row_ids: HOST [m], GLOBAL rows as the searches return them (local row + option "row_offset"), shared by all B queries of
 *     the call.  Values outside [row_offset, row_offset + mi355dr_size) are skipped -- negative values and -1 padding
 *     included: the rule of mi355dr_maxsim_subset -- and a value listed twice counts once.
 *   Removed rows are skipped; live irregular rows come last with NaN, as on the scan path; loose rows are ordinary rows here
 *     (no screen is involved).  Both metrics, any k up to 1024 and any B that mi355dr_search accepts.  m == 0, or no live
 *     listed row: all NaN / -1.  A bad shape (m < 0, a null list with m > 0): MI355DR_E_INVALID.
 *   The call runs under the handle's mutex, first completes whatever search is in flight, and is complete on return (the
 *     _device form too: `stream`, or the index's own when NULL, is synchronised).  The list is copied, made local, sorted
 *     and uploaded as int32 into a buffer the index owns and grows; a failed allocation returns MI355DR_E_NOMEM with nothing
 *     changed.  The pass is the exact scan (MI355DR_PATH_SCAN) walking the list instead of the index: no screen, the same
 *     fp32 chains, cost proportional to m x B.  Options "chunk0_rows", "chunk_growth" and "cand_cap" apply as on that path.
 *   Stats: "subset_searches" (calls), "subset_rows_scored" ((query, listed row) pairs scored), "subset_rerun_queries" (queries
 *     whose candidate list overflowed in a chunk of the list, which was then re-run for them in list-sized pieces). */
int mi355dr_search_subset(mi355dr_index* idx, const float* queries, int B, int k, const int64_t* row_ids, int64_t m,
                          double* out_dist, int64_t* out_rows); /* all host */
/* queries_dev [B, dim], out_dist_dev [B, k], out_rows_dev [B, k] on the index's device; row_ids stay on the HOST */
int mi355dr_search_subset_device(mi355dr_index* idx, const float* queries_dev, int B, int k, const int64_t* row_ids, int64_t m,
                                 double* out_dist_dev, int64_t* out_rows_dev, void* stream);
/* The single-vector sibling of mi355dr_maxsim_subset: the exact float8 distance of every query to its OWN list of rows.
 * row_ids: host [B, m] global rows (the skipping rule above), out_dist: host [B, m]; NaN for skipped ids, for removed rows
 * and where the distance is undefined (a zero norm).  Same device code as mi355dr_debug_rescore. */
int mi355dr_score_subset(mi355dr_index* idx, const float* queries, int B, const int64_t* row_ids, int m, double* out_dist);

/* ---- MMR search: a diversity-aware top-k, selected on the device ----
 * Maximal Marginal Relevance: fetch fetch_k candidates, then pick k of them greedily, each time the candidate that is similar
 * to the query and dissimilar to what was already picked.  The candidates' vectors never leave the device.
 *   Candidate order: the library's total order (distance asc, NaN last, row asc) -- for mi355dr_search_mmr the result of the
 *     ordinary search at k = fetch_k; for mi355dr_mmr_select the caller's list put into that order: the in-index live rows,
 *     each once, as mi355dr_search_subset orders them.
 *   Eligible candidates: the leading entries with row >= 0 and a non-NaN distance; n of them.
 *   sim(dist) = 1.0 - dist (cosine), -dist (inner product).  pairdist(a, b) of two stored rows: the library's exact distance --
 *     the k-ascending fp32 fmaf chain for the dot, the stored squared norms of both rows, the float8 formula of the searches;
 *     it is symmetric.  Everything below is IEEE double, separate operations, no fused multiply-add:
 *       sq[i] = sim(dist[i]), one_m = 1.0 - lambda;  pick 0 = candidate 0;
 *       after each pick c, except the last, for every unselected i:  s = sim(pairdist(c, i));
 *           ms[i] = s at the first pick;  ms[i] = s > ms[i] ? s : ms[i] afterwards (a NaN s is ignored);
 *       pick t >= 1:  score[i] = lambda * sq[i] - one_m * ms[i] over the unselected i;  the first i, in candidate order, whose
 *           score is strictly greater than every earlier unselected score; a NaN score never wins; if none wins, the first
 *           unselected i.
 *     Stop after min(k, n) picks.  Output slot t: pick t's query distance (the bits the search returned) and its global row;
 *     slots from min(k, n) on: NaN / -1.  lambda = 1.0 reproduces the ordinary top-k over the eligible candidates bit for bit.
 *   mi355dr_search_mmr / _device: the ordinary search of the block at fetch_k (the code of mi355dr_search_device: screened,
 *     fix-ups completed) into buffers the index owns and grows, then the selection kernel on the same stream.  B above 1024
 *     runs in internal blocks.  Under the handle's mutex; first completes what is in flight; complete on return.
 *   mi355dr_mmr_select: the lower layer for explicit per-query pools (hybrid or HEAVEN candidates, a key filter).  cand_rows:
 *     HOST [B, m] GLOBAL rows under the hygiene of mi355dr_score_subset / mi355dr_search_subset (ids outside the index and -1
 *     padding skipped, duplicates once, removed rows skipped, any order); distances from the device code of
 *     mi355dr_score_subset; the host orders each list and uploads it; the same kernel.  k may exceed m (NaN / -1 tail).
 *   MI355DR_E_INVALID: lambda outside [0, 1] or NaN, k <= 0, fetch_k < k, m < 0, a null buffer with work to do, and all three
 *     on a view (ask the parent).  MI355DR_E_UNSUPPORTED: fetch_k > 1024, m > 1024.
 *   Stats: "mmr_searches" (calls), "mmr_queries", "mmr_pairs_scored" ((picked row, unselected candidate) dots). */
int mi355dr_search_mmr(mi355dr_index* idx, const float* queries, int B, int k, int fetch_k, double lambda, double* out_dist,
                       int64_t* out_rows); /* all host */
int mi355dr_search_mmr_device(mi355dr_index* idx, const float* queries_dev, int B, int k, int fetch_k, double lambda,
                              double* out_dist_dev, int64_t* out_rows_dev, void* stream);
int mi355dr_mmr_select(mi355dr_index* idx, const float* queries, int B, int k, const int64_t* cand_rows /* host [B, m] */, int m,
                       double lambda, double* out_dist, int64_t* out_rows); /* all host */

/* ---- grouped search: sub-query top-k lists fused into one on the device ----
 * Several searches per question -- the question and its decomposed sub-questions, several hypothetical passages, a set of
 * rewrites -- fused by "every row once, at its best value".  The lists never leave the device.
 *   Input: S lists of `width` (value, row) entries and G groups; group g owns lists group_offsets[g] .. group_offsets[g+1]-1
 *     (HOST int32 [G+1], starting at 0, not decreasing, ending at S).  An entry with row < 0 is no entry; an entry with a row
 *     and a NaN value is one (an irregular row's result).
 *   Result of group g: the union of its lists' entries, each row ONCE at its smallest value under the library's order
 *     (value asc, NaN last -- a row keeps a NaN only if every occurrence was NaN), sorted by (value asc, NaN last, row asc);
 *     the first k_out of them.  A number is written with the bits it came with (+0.0 and -0.0 are different values, -0.0
 *     first), a NaN as the library's NaN; rows are int64 as given.  Slots behind the union: NaN / -1.  count[g] = the number of
 *     distinct rows in the union (it may exceed k_out); an empty group gives NaN / -1 and 0.  Values are plain doubles: the
 *     MaxSim callers merge scores.
 *   mi355dr_merge_groups_device: the merge alone, over device lists.  Stateless (it reads no index state: allowed on a view,
 *     like mi355dr_merge_topk*); the offsets are copied into a buffer the index owns and grows; under the handle's mutex;
 *     complete on return; a failed allocation returns MI355DR_E_NOMEM with nothing changed.  out_count_dev may be NULL.
 *   mi355dr_search_groups / _device: the ordinary search of all S = group_offsets[G] sub-queries at fetch_k (the code of
 *     mi355dr_search_device: screened, fix-ups completed, internal blocks of 1024 queries; a group may straddle two) into
 *     buffers the index owns and grows, then ONE merge launch on the same stream.  Group g's result is the top-k under
 *     (distance asc, NaN last, row asc) of the union of its sub-queries' top-fetch_k lists, each row once at its smallest
 *     distance, with the bits the search returned and global rows.  k may exceed fetch_k (up to max_g(s_g) x fetch_k entries
 *     exist; the rest is NaN / -1).  Works on views (results under the parent's ids): it takes no global ids.  First completes
 *     what is in flight; complete on return.
 *   MI355DR_E_INVALID: G < 0, S < 0, k_out / k / fetch_k / width <= 0, a null pointer with work to do, offsets that do not start
 *     at 0, decrease, or do not end at S.  MI355DR_E_UNSUPPORTED: fetch_k > 1024, k_out / k > 4096, a group of more than 4096
 *     entries (s_g x width; the kernel sorts next_pow2 of it in 64 KiB of LDS).  G == 0 is a valid no-op.  A refused call
 *     changes nothing.
 *   Stats: "group_searches" (calls of mi355dr_search_groups*), "group_subqueries" (S, summed), "groups_merged" (groups merged,
 *     both entry families). */
int mi355dr_merge_groups_device(mi355dr_index* idx, const double* vals_dev, const int64_t* rows_dev, int S, int width,
                                const int32_t* group_offsets /* HOST [G+1] */, int G, int k_out, double* out_vals_dev,
                                int64_t* out_rows_dev, int32_t* out_count_dev /* may be NULL */, void* stream);
int mi355dr_search_groups(mi355dr_index* idx, const float* queries /* host [S, dim] */, const int32_t* group_offsets, int G, int k,
                          int fetch_k, double* out_dist /* [G,k] */, int64_t* out_rows /* [G,k] */,
                          int32_t* out_count /* [G] or NULL */); /* all host */
int mi355dr_search_groups_device(mi355dr_index* idx, const float* queries_dev, const int32_t* group_offsets /* HOST */, int G, int k,
                                 int fetch_k, double* out_dist_dev, int64_t* out_rows_dev, int32_t* out_count_dev, void* stream);

/* ---- range search: every row within a distance, counted on the device ----
 * The other half of the statement: `WHERE embedding IS NOT NULL AND embedding <=> :q <= :r ORDER BY distance LIMIT :m`, and
 * `SELECT count(*)` under the same filter -- adaptive-k retrieval, near-duplicate and semantic-cache checks, "how many chunks
 * are relevant at all" before a fusion.
 *   In range: a live row whose float8 distance d to the query -- the bits mi355dr_search returns for the pair -- satisfies
 *     d <= radius[b], compared as doubles.  A NaN distance (an irregular row, a zero-norm query under cosine) is never in
 *     range, a removed row never.  Both metrics; for inner product the radius is in the operator's own units, -dot.
 *     radius: HOST [B], any double but NaN; +inf = every row with a defined distance, -inf = none.
 *   out_count[b]: the number of in-range rows of this handle; exact, it may exceed max_results.
 *   The list: the first min(count, max_results) in-range rows under the library's total order (distance asc, row asc), with the
 *     bits of mi355dr_search and global rows (option "row_offset" added; on a view the parent's ids); slots behind it hold
 *     NaN / -1.  Equivalently: mi355dr_search at k = max_results with every entry whose distance is NaN or above the radius
 *     replaced by NaN / -1.
 *   MI355DR_E_INVALID: B <= 0, max_results < 1, a NaN radius, a null buffer.  MI355DR_E_UNSUPPORTED: max_results > 1024.  A
 *     refused call changes nothing.  B above 1024 runs in internal blocks.
 *   The call runs under the handle's mutex, first completes whatever search is in flight and is complete on return (the
 *     _device form too: `stream`, or the index's own when NULL, is synchronised).  It uses the per-search state of the handle
 *     and leaves it to the next search, which prepares all of it anew: that search returns what it would have returned
 *     without the range call.  Works on a view (it takes no global ids).
 *   Two paths with identical results, steered by option "path".  Exact range scan (MI355DR_PATH_SCAN, every query no screen
 *     can serve, every chunk a screen overflowed): the exact scan's launches with the radius as their fixed threshold, chunk by
 *     chunk; a chunk whose list overflowed is run again in list-sized pieces, unless its count alone already puts the query
 *     beyond its result buffer.  Screened (AUTO wherever a search would screen, and SCREEN): the screens of the ordinary search
 *     with the FIXED threshold the radius allows (the function the prunes publish thresholds with) -- no starter, no ladder of
 *     prunes --, every candidate re-scored by the exact chain and kept iff it is in range; rows the screens cannot see
 *     (irregular, loose) are re-scored for every query; irregular queries, a threshold that admits every row, and every
 *     (query, chunk) whose candidate list overflowed take the exact path, that query's later chunks with it.
 *   A query keeps its in-range rows in a buffer of option "range_slots" (default and most 4096, at least max_results) entries
 *     that the index owns and grows; with more rows in range than that, its list comes from the ordinary search at
 *     k = max_results (every entry of which is in range) and its count from the device counter.
 *   Options: "range_chunk_rows" (rows per screen launch / exact span, default 2097152, rounded up to whole 256-row tiles),
 *     "range_slots"; "cand_cap", "small_chunk_rows", "screen_dtype", "screen_rq", "screen_stream" and "scan_dma" apply as in a
 *     search.
 *   Stats: "range_searches" (calls), "range_queries", "range_in_range" (the counts, summed), "range_candidates" /
 *     "range_rescored" (screen path: candidates taken from the screens / of them re-scored), "range_redo_chunks" ((query, chunk)
 *     pairs run again on the exact path), "range_fallback_queries" (queries whose list the ordinary search served: that search
 *     moves the ordinary stats, nothing else of a range call does).
 *   Row-sharded: mi355dr_search_range_sharded_device (below, "the derived searches over a row-sharded index") -- counts add
 *     across shards, and the lists -- global rows, the total order -- merge like any top-k lists. */
int mi355dr_search_range(mi355dr_index* idx, const float* queries, int B, const double* radius /* host [B] */,
                         int max_results, double* out_dist /* [B, max_results] */, int64_t* out_rows /* [B, max_results] */,
                         int64_t* out_count /* [B] */); /* all host */
/* queries_dev [B, dim], out_dist_dev / out_rows_dev [B, max_results], out_count_dev [B] on the index's device; the radii stay on the HOST */
int mi355dr_search_range_device(mi355dr_index* idx, const float* queries_dev, int B, const double* radius /* HOST [B] */,
                                int max_results, double* out_dist_dev, int64_t* out_rows_dev, int64_t* out_count_dev,
                                void* stream);

/* ---- search by stored row: neighbours of rows, self excluded, on the device ----
 * The self-join form of the two statements above: `SELECT b.id FROM chunk a, chunk b WHERE a.id = :r AND b.id <> a.id ORDER BY
 * a.embedding <=> b.embedding LIMIT k`, and the same under `a.embedding <=> b.embedding <= :radius` with `count(*)` --
 * near-duplicate detection at ingest, "more like this" from a primary key, the exact k-NN graph of a corpus.  The query
 * vectors are read where they lie; they never leave the device.
 *   The query of slot b: the stored fp32 vector of row row_ids[b].  row_ids: HOST [B], GLOBAL rows (local row + option
 *     "row_offset"), under the hygiene of mi355dr_search_subset: an id outside [row_offset, row_offset + mi355dr_size) --
 *     negative values and -1 included -- and a removed row (not a row of the index, although its bytes are still there) give an
 *     all-NaN / -1 output row and count 0, and are counted in stat "rows_skipped".  An id may be listed more than once: every
 *     slot is answered.
 *   flags: 0, or MI355DR_ROWS_INCLUDE_SELF.
 *   mi355dr_search_rows: with INCLUDE_SELF exactly mi355dr_search(idx, the stored vectors, B, k) -- float8 bits, rows, NaN
 *     positions and the NaN / -1 tail.  Without it (the default) the top-k of the live rows OTHER than row_ids[b] under the
 *     library's total order (distance asc, NaN last, row asc), with the same bits.  Equivalently: take the top-(k + 1) list; if
 *     the row itself is in it, remove it and close the gap; otherwise cut the list to k -- with more than k exact copies of the
 *     row at lower ids the row itself lies behind the list.  Rows with a NaN distance stay where the ordinary search puts them:
 *     a zero-norm query row under cosine gives an all-NaN list in row order, itself taken out.
 *   mi355dr_search_range_rows: with INCLUDE_SELF mi355dr_search_range of the stored vectors.  Without it "in range" is as
 *     there, and the row itself is left out of the count and of the list.  Whether the row itself was in range is decided from
 *     the row-with-itself distance -- the bits mi355dr_search returns for the pair -- compared with the radius as doubles (a NaN
 *     is never in range), not from whether the row appears in the truncated list.  The count stays exact and may exceed
 *     max_results.  radius: HOST [B].
 *   MI355DR_E_INVALID: B < 0, k <= 0, max_results < 1, a NaN radius, a null buffer with work to do, unknown flag bits, and all
 *     four on a view (they take global ids: ask the parent).  MI355DR_E_UNSUPPORTED: without INCLUDE_SELF k + 1 > 1024 or
 *     max_results + 1 > 1024 (the inner pass needs room for the row itself); with it k or max_results > 1024.  B == 0 is a valid
 *     no-op.  A refused call changes nothing.
 *   The call runs under the handle's mutex, first completes whatever search is in flight and is complete on return (the _device
 *     forms too: `stream`, or the index's own when NULL, is synchronised).  B above 1024 runs in internal blocks.  Per block: the
 *     ids are uploaded, k_rows_gather copies the rows into a query buffer the index owns, the ordinary search of the block runs
 *     at k + 1 (the range pass at max_results + 1; k and max_results with INCLUDE_SELF) into lists the index owns, and
 *     k_rows_drop writes the outputs.  Options and paths apply as in mi355dr_search / mi355dr_search_range.
 *   Known cost: the inner pass runs at k + 1, so k = 32 is served by the 33 ... 128 class of the search (two-wave prune) and
 *     k = 128 by the class above it.
 *   Stats: "rows_searches" (calls), "rows_queries" (slots), "rows_skipped"; the ordinary and the range stats move as the inner
 *     pass moves them ("passes", "chunks", "range_in_range" -- the inner counts, the rows themselves included -- and so on; the
 *     call counters "range_searches" / "range_queries" belong to mi355dr_search_range* and stay).
 *   Not served: views (above).  Row-sharded: mi355dr_search_rows_sharded_device / mi355dr_search_range_rows_sharded_device
 *     (below, "the derived searches over a row-sharded index") -- the query row lives on one shard only, so its vector is
 *     gathered from the owner before the sharded pass at k + 1. */
#define MI355DR_ROWS_INCLUDE_SELF 1 /* flags: the query row itself stays in the result (default 0: it is left out) */
int mi355dr_search_rows(mi355dr_index* idx, const int64_t* row_ids /* HOST [B], global */, int B, int k, int flags,
                        double* out_dist /* [B, k] */, int64_t* out_rows /* [B, k] */); /* outputs on the host */
/* out_dist_dev / out_rows_dev [B, k] on the index's device; row_ids stay on the HOST */
int mi355dr_search_rows_device(mi355dr_index* idx, const int64_t* row_ids /* HOST [B] */, int B, int k, int flags,
                               double* out_dist_dev, int64_t* out_rows_dev, void* stream);
int mi355dr_search_range_rows(mi355dr_index* idx, const int64_t* row_ids /* HOST [B] */, int B, const double* radius /* HOST [B] */,
                              int max_results, int flags, double* out_dist /* [B, max_results] */,
                              int64_t* out_rows /* [B, max_results] */, int64_t* out_count /* [B] */); /* outputs on the host */
/* out_dist_dev / out_rows_dev [B, max_results], out_count_dev [B] on the index's device; row_ids and the radii stay on the HOST */
int mi355dr_search_range_rows_device(mi355dr_index* idx, const int64_t* row_ids /* HOST [B] */, int B,
                                     const double* radius /* HOST [B] */, int max_results, int flags, double* out_dist_dev,
                                     int64_t* out_rows_dev, int64_t* out_count_dev, void* stream);

/* ---- search by examples / feedback: queries built on the device from stored rows ----
 * "More like these, less like those" (the `recommend` of vector stores) and Rocchio pseudo-relevance feedback: the query is a
 * combination of stored rows, optionally with a vector of the caller's.  The rows are read where they lie; neither they nor
 * the first pass's lists of the feedback form leave the device.
 *   Inputs of slot b: an optional base vector q_b (fp32 [dim]; absent when `queries` is NULL), positives pos_ids[b, 0..mp) and
 *     negatives neg_ids[b, 0..mn) -- GLOBAL row ids, HOST arrays, -1-padded; a repeat counts once per position --, and per call
 *     the doubles alpha, beta, gamma, each finite and >= 0.
 *   A listed position is VALID iff its id lies in the shard (the rule of mi355dr_search_subset: [row_offset, row_offset +
 *     mi355dr_size)), the row is not removed, and the row's stored squared norm -- the k-ascending fp32 chain -- is finite and
 *     > 0; the same under both metrics.  Every other position (-1 padding included) is skipped and counted in stat
 *     "examples_skipped".  A base vector is valid iff its squared norm under the same chain is finite and > 0.
 *   A slot is INVALID if it has an invalid base, or no valid term at all (no base, no valid positive, no valid negative): its
 *     combined vector is all zeros, valid[b] = 0, its result line NaN / -1, and it is counted in "examples_skipped_slots".
 *   The arithmetic: IEEE double, one rounding per operation, nothing fused; sqrt and / as in the cosine distance.
 *       s(v) = 1.0 / sqrt((double)nrm2(v))   (cosine index)        s(v) = 1.0   (inner-product index)
 *       cp = beta / (double)(valid positives)     cn = gamma / (double)(valid negatives)     (none: no such term)
 *       per coordinate i:  acc = base present ? alpha * (s(q) * (double)q_i) : +0.0
 *                          each valid positive j, in list position order:  acc = acc + cp * (s_j * (double)c_ji)
 *                          each valid negative j, in list position order:  acc = acc - cn * (s_j * (double)c_ji)
 *                          q'_i = (float)acc   (round to nearest even)
 *     Whatever q' comes out is searched as mi355dr_search would search it -- a vector that cancelled to zero or overflowed
 *     included; nothing is special-cased beyond the validity rules.
 *   mi355dr_combine_rows: the combination alone -- out_vectors [B, dim] fp32, out_valid [B] int32.  Also a centroid of stored
 *     rows without a mi355dr_get_rows per id.  mp + mn <= 1024.
 *   mi355dr_search_examples: the mi355dr_search ranking of q'_b over the live rows, cut to k, after every id listed in the slot
 *     -- positive or negative, valid or not -- has been struck out.  The inner pass runs at k + mp + mn: at most that many rows
 *     can be struck, so the first k survivors are the exact answer (a duplicate of a listed row under another id stays).
 *     flags: 0, or MI355DR_EXAMPLES_KEEP: nothing is struck, the inner pass runs at k.
 *   mi355dr_search_feedback: pass 1 is mi355dr_search of `queries` at fb_k (1 <= fb_k <= 1024).  The positives of slot b are the
 *     entries of its pass-1 list with row >= 0 and a non-NaN distance, in list order (the other entries are no positions at
 *     all: not counted); there are no negatives; q' is built as above from alpha, beta and the caller's vector as base; pass 2
 *     is mi355dr_search of q' at k, nothing struck.  By construction: mi355dr_search at fb_k, then mi355dr_search_examples with
 *     those rows and KEEP.
 *   MI355DR_E_INVALID, before anything is touched: B < 0; k <= 0, fb_k <= 0, negative mp / mn; a NaN, infinite or negative
 *     weight; unknown flag bits; a null buffer with work to do; queries == NULL together with mp == 0; and all six on a view
 *     (they take global ids: ask the parent).  MI355DR_E_UNSUPPORTED: a depth above 1024 -- k + mp + mn without KEEP; k, or
 *     mp + mn, with it; mp + mn of mi355dr_combine_rows; k or fb_k of the feedback.  B == 0 is a valid no-op.  An empty index
 *     gives all NaN / -1.
 *   Each call runs under the handle's mutex, first completes whatever search is in flight and is complete on return (the
 *     _device forms too: `stream`, or the index's own when NULL, is synchronised).  B above 1024 runs in internal blocks.  Per
 *     block: the ids are uploaded, k_combine_rows writes q' into a buffer the index owns, the ordinary search of the block
 *     runs into lists the index owns, and k_examples_strike writes the outputs.  Options and paths apply as in mi355dr_search.
 *   Known cost: an inner pass at k + mp + mn may be served by the next k class of the search (<= 32 | 33 ... 128 | above).
 *   Stats: "examples_searches" (calls of the six), "examples_queries" (their slots), "examples_skipped",
 *     "examples_skipped_slots", "feedback_searches" (of the calls, the feedback ones); the ordinary stats move as the inner
 *     passes move them.
 *   Not served: views (above); a row-sharded form (the examples of a slot live on different shards, and the fixed summation
 *     order does not survive a reduction across ranks); MaxSim and the sparse store; more than one feedback round per call (a
 *     caller can loop). */
#define MI355DR_EXAMPLES_KEEP 1 /* flags: the listed rows stay in the result (default 0: they are struck out) */
int mi355dr_combine_rows(mi355dr_index* idx, const float* queries /* [B, dim] or NULL */, int B,
                         const int64_t* pos_ids /* HOST [B, mp], global */, int mp, const int64_t* neg_ids /* HOST [B, mn] */, int mn,
                         double alpha, double beta, double gamma, float* out_vectors /* [B, dim] */,
                         int32_t* out_valid /* [B] */); /* queries and outputs on the host */
/* queries_dev (or NULL), out_vectors_dev [B, dim], out_valid_dev [B] on the index's device; the ids stay on the HOST */
int mi355dr_combine_rows_device(mi355dr_index* idx, const float* queries_dev, int B, const int64_t* pos_ids /* HOST */, int mp,
                                const int64_t* neg_ids /* HOST */, int mn, double alpha, double beta, double gamma,
                                float* out_vectors_dev, int32_t* out_valid_dev, void* stream);
int mi355dr_search_examples(mi355dr_index* idx, const float* queries /* [B, dim] or NULL */, int B,
                            const int64_t* pos_ids /* HOST [B, mp] */, int mp, const int64_t* neg_ids /* HOST [B, mn] */, int mn,
                            double alpha, double beta, double gamma, int k, int flags, double* out_dist /* [B, k] */,
                            int64_t* out_rows /* [B, k] */); /* queries and outputs on the host */
/* queries_dev (or NULL), out_dist_dev / out_rows_dev [B, k] on the index's device; the ids stay on the HOST */
int mi355dr_search_examples_device(mi355dr_index* idx, const float* queries_dev, int B, const int64_t* pos_ids /* HOST */, int mp,
                                   const int64_t* neg_ids /* HOST */, int mn, double alpha, double beta, double gamma, int k,
                                   int flags, double* out_dist_dev, int64_t* out_rows_dev, void* stream);
int mi355dr_search_feedback(mi355dr_index* idx, const float* queries /* [B, dim] */, int B, int k, int fb_k, double alpha,
                            double beta, double* out_dist /* [B, k] */, int64_t* out_rows /* [B, k] */); /* all host */
/* queries_dev [B, dim], out_dist_dev / out_rows_dev [B, k] on the index's device */
int mi355dr_search_feedback_device(mi355dr_index* idx, const float* queries_dev, int B, int k, int fb_k, double alpha, double beta,
                                   double* out_dist_dev, int64_t* out_rows_dev, void* stream);

/* ---- views: a listed subset of rows / documents as an index of its own ----
 * For a list that is searched again and again -- one tenant, one document collection, one PDF's pages: the key filter of the
 * statement above, fixed for many query blocks.  mi355dr_search_subset scans the list exactly on every call (cost ~ m x B, no
 * screen); a view pays once for gathering the listed rows on the device into a handle of their own, and every search path --
 * the MFMA screens, the MaxSim screen -- then runs on that handle.  Results come back under the PARENT's ids.
 *   row_ids: HOST [m_rows], doc_ids: HOST [m_docs]; either list may be empty (NULL with a count of 0).  Ids are GLOBAL (local
 *     row / document + the parent's "row_offset").  List hygiene is that of mi355dr_search_subset: values outside the parent's
 *     shard are skipped (negative values and -1 padding included), a value listed twice counts once, the order never matters.
 *     Removed rows are left out, and so are documents without vectors.  m < 0, or a null list with m > 0: MI355DR_E_INVALID.
 *     Two empty lists make a valid empty view.
 *   The view is an ordinary mi355dr_index on the parent's device, with the parent's dim and metric and with options at their
 *     defaults; it owns its memory, stream and mutex and is released with mi355dr_destroy.  It holds the live listed rows in
 *     ascending id order and the listed documents with vectors in ascending id order, and answers as an index built fresh by
 *     one mi355dr_add_rows / mi355dr_add_multivec of exactly those would: norm bits, both shadows, the irregular and loose
 *     classes and the maxima are built by the view's own add paths, not copied (an int8 group of 32 rows depends on its
 *     neighbours).  mi355dr_size == mi355dr_live_rows == the live listed rows, mi355dr_size_multivec == the listed documents
 *     with vectors, mi355dr_get_rows(view, j, n) returns the listed rows in ascending id order.
 *   Every search entry point works on it as on any handle -- mi355dr_search / _device / _device_async + _wait,
 *     mi355dr_search_maxsim / _device, options, stats, timers, dev_* -- and RETURNS THE PARENT'S GLOBAL IDS:
 *       mi355dr_search(view, Q, k)         == mi355dr_search_subset(parent, Q, k, row_ids): float8 bits, rows, NaN positions and
 *                                             the NaN / -1 tail, on every path and screen_dtype, both metrics, any k and B (view
 *                                             order is id order, so ties break by the parent's ids);
 *       mi355dr_search_maxsim(view, ...)   == the top-k by (distance asc, document asc) of mi355dr_maxsim_subset(parent, ...)
 *                                             over the listed documents with vectors, fp32 bits.
 *   Snapshot: later update / remove / compact / set_multivec on the parent do not reach the view (after a parent compact the
 *     view still speaks the OLD ids); the parent may be destroyed first.
 *   Read-only: mi355dr_add_rows*, _update_rows*, _remove_rows, _compact, _reserve, _add_multivec*, _set_multivec* and option
 *     "row_offset" return MI355DR_E_INVALID on a view and change nothing.  So does every entry point that takes global ids or a
 *     communicator, with an error text that refers the caller to the parent: mi355dr_search_subset*, _score_subset, _search_mmr*, _mmr_select,
 *     _search_rows*, _search_range_rows*, _combine_rows*, _search_examples*, _search_feedback*, _maxsim_subset*, _search_maxsim_subset*, _gqr_refine, _gqr_refine_maxsim, _comm_init*, _search_sharded_device, and mi355dr_view_create itself (no
 *     views of views).  The stateless ones stay usable: mi355dr_merge_topk*, _pack_topk_device, _gqr_refine_scores, _merge_groups_device.
 *   The call takes the parent's mutex, first completes whatever search is in flight there, and is complete on return;
 *     afterwards the two handles are independent.  The parent is only read.  On any error *out_view is NULL, everything
 *     allocated for the view has been released and the parent is unchanged and usable (its last_error has the text); a failed
 *     allocation returns MI355DR_E_NOMEM.
 *   Memory: the view costs what a fresh index of that many rows / documents costs, plus 8 bytes per row and document for the id
 *     maps.  During the call there is on top ONE staging buffer of the parent's option "view_slice_rows" rows (default 65536,
 *     32 ... 2^22; fewer when less is listed): rows are gathered and added slice by slice, and the documents' tokens in slices
 *     of the same byte count (a document longer than a slice goes alone and sizes the buffer).  The removed rows are found by
 *     reading the m listed rows' norms back (4 m bytes), before any row is gathered.
 *   Stats on the view: "view" = 1 (0 on any other index, where the next two are 0 as well), "view_rows" / "view_docs" = what
 *     the build kept, "hbm_bytes_resident" counts the view's own memory. */
int mi355dr_view_create(mi355dr_index* parent, const int64_t* row_ids, int64_t m_rows, const int64_t* doc_ids, int64_t m_docs,
                        mi355dr_index** out_view);

/* ---- corpus + search (multi-vector, MaxSim) ----
 * vecs: host [sum_T, dim] fp32, offsets: [n_docs+1] (doc i owns rows offsets[i]..offsets[i+1]). */
int mi355dr_add_multivec(mi355dr_index* idx, const float* vecs, const int64_t* offsets, int64_t n_docs);
/* the same from DEVICE memory (an encoder's output never leaves HBM: embeddings/colpali.py:168-245 `embed_image(s)` /
 * `embed_documents` -> [T,128] patch / token tensors): vecs_dev = device [sum_T, dim], offsets = HOST [n_docs+1] */
int mi355dr_add_multivec_device(mi355dr_index* idx, const float* vecs_dev, const int64_t* offsets, int64_t n_docs);
/* documents stored, with or without vectors (document ids are stable: nothing is ever renumbered) */
int64_t mi355dr_size_multivec(const mi355dr_index* idx);

/* ---- update / remove in place (multi-vector) ----
 * The multi-vector column is not append-only either: BaseVectorRepository.set_multi_vector_embedding(s_batch)
 * (orm/repository/base.py:428-485) is an UPDATE of an existing row, and a row whose `embeddings` became NULL -- or a deleted
 * chunk -- leaves maxsim_search at once (:487-535, `embeddings IS NOT NULL`).
 *   set: document doc_ids[j] takes the vectors offsets[j] .. offsets[j+1] of vecs (the layout of mi355dr_add_multivec).  No
 *        vectors removes the document: it becomes a document without vectors -- skipped by every search, NaN in
 *        mi355dr_maxsim_subset, refused by mi355dr_gqr_refine_maxsim -- and a later set with vectors revives it.  Ids stay and
 *        mi355dr_size_multivec is unchanged.  Afterwards every entry point that reads the store (mi355dr_search_maxsim / _device,
 *        mi355dr_maxsim_subset / _ex, mi355dr_gqr_refine_maxsim) answers as a fresh store built by mi355dr_add_multivec from the
 *        current contents would, bit for bit in distances and ids.
 * doc_ids: HOST [n], each in [0, size_multivec) and listed once per call; offsets: HOST [n+1], non-decreasing -- otherwise
 * MI355DR_E_INVALID and nothing changes; a failed allocation returns MI355DR_E_NOMEM and nothing changes.  The call runs under
 * the handle's mutex and is complete on return.  A host payload is staged in slices of 32 MiB, like an add's.
 * Layout and cost: documents own consecutive 32-token blocks of one stream, so the call takes one of two paths.
 *   in place  no listed document changes its block count ceil(T/32) (re-embedding: same tokenizer, same token count; pages
 *             with a fixed patch count): only the listed documents' blocks of the fp32 and bf16 images are rewritten.
 *             O(listed blocks).
 *   relayout  some block count changes (every removal, any shorter or longer document): the cumulative block table is laid
 *             out anew, FRESH image buffers are allocated (capacity as before, more if the new total needs it), one kernel
 *             moves the blocks of the documents that were not listed, the listed ones are built from the new vectors, and
 *             the buffers are swapped at the end.  One device pass over the store; PEAK MEMORY: one extra copy of the two
 *             images (6 bytes per stored value) for the duration of the call.
 * What never shrinks: the three maxima of the screen bound (largest token norm, largest bf16-rounded token norm, largest bf16
 * residual) and the "not finite" flag move in the conservative direction only, as the single-vector maxima do -- candidate
 * counts may differ from a fresh store's, results may not; nor does the capacity.  The granule-packed copy (option
 * "maxsim_pack8") is stale after any set and is packed anew, whole, by the next pass that takes it. */
int mi355dr_set_multivec(mi355dr_index* idx, const int64_t* doc_ids, const float* vecs, const int64_t* offsets, int64_t n); /* vecs: host */
/* the same with the new vectors on this index's device ([.., dim] fp32, read in place); doc_ids and offsets stay on the host */
int mi355dr_set_multivec_device(mi355dr_index* idx, const int64_t* doc_ids, const float* vecs_dev, const int64_t* offsets, int64_t n);
/* documents that have vectors: mi355dr_size_multivec minus the removed and the empty ones */
int64_t mi355dr_live_multivec(const mi355dr_index* idx);

/* qtok: host [sum_nq, dim], q_offsets: [B+1].  out_dist: [B,k] fp32 (= -sum_i max_j <q_i,d_j>). */
int mi355dr_search_maxsim(mi355dr_index* idx, const float* qtok, const int32_t* q_offsets, int B, int k,
                          float* out_dist, int64_t* out_rows);
/* The same with the query vectors and the results in DEVICE memory of the index's GPU (an encoder's output tensor in, the
 * packed block of a row-sharded search out: BaseVectorRepository.maxsim_search behind a multi-GPU caller,
 * orm/repository/base.py:487-535).  qtok_dev: device [sum_nq, dim]; q_offsets: HOST [B+1]; out_dist_dev [B,k] fp32 and
 * out_rows_dev [B,k] int64 on the device, complete on return.  `stream`: the stream that produced qtok_dev (waited for
 * before the vectors are read; NULL: none).  The query side of a pass is small (a few hundred KiB) and its screen bound is
 * evaluated in double on the host, so the vectors are read back once; the results never leave HBM. */
int mi355dr_search_maxsim_device(mi355dr_index* idx, const float* qtok_dev, const int32_t* q_offsets, int B, int k,
                                 float* out_dist_dev, int64_t* out_rows_dev, void* stream);

/* exact MaxSim distance of every query to an explicit list of docs (candidate re-scoring: HEAVEN stage 2,
 * autorag_research/pipelines/retrieval/heaven.py:244-266 `_score_candidates`, score = -distance / n_q; GQR pools,
 * gqr_hybrid.py:366-406).  doc_ids: host [B, m] global rows (as returned by the searches; other values are skipped),
 * out_dist: host [B, m] fp32, NaN for skipped ids, docs without vectors and queries without vectors. */
int mi355dr_maxsim_subset(mi355dr_index* idx, const float* qtok, const int32_t* q_offsets, int B, const int64_t* doc_ids,
                          int m, float* out_dist);
/* The same with flags.  MI355DR_MAXSIM_CLAMP0: every query vector contributes max(0, max_j <q_i, d_j>) -- the ColBERT
 * reranker's MaxSim (autorag_research/rerankers/colbert.py:63-84: padding masked, `clamp(min=0)`, mean over the VALID query
 * tokens): pass only the valid tokens of query and documents; score = -distance / n_valid_query_tokens. */
#define MI355DR_MAXSIM_CLAMP0 1
int mi355dr_maxsim_subset_ex(mi355dr_index* idx, const float* qtok, const int32_t* q_offsets, int B, const int64_t* doc_ids,
                             int m, int flags, float* out_dist);

/* ---- MaxSim explained: the terms of the sum ----
 * Every entry point above answers with one number per (query, document), -sum_i max_j <q_i, d_j>.  These three give the terms:
 * ColBERT's token alignment (per query vector the matched document token and its dot) and ColPali's similarity map (per query
 * vector the dot with every token of a page).  The token vectors never leave the device.
 * The rule (tests/maxsim_align_ref.py restates it):
 *   - every dot is the exact kernel's k-ascending fp32 fmaf chain from 0.0f (oracle.c orc_dot), the chain mi355dr_search_maxsim
 *     and mi355dr_maxsim_subset promise;
 *   - the maximum is fmaxf from -inf over the document's tokens; a NaN dot is ignored;
 *   - out_tok is the LOWEST token index j with dot_j == maximum under float equality.  The store pads a document's last
 *     32-token block with copies of its last token; a copy is never reported: the answer is < T.  If every dot of a query
 *     vector is NaN, the maximum is -inf: out_val = -inf, out_tok = -1;
 *   - a candidate whose id is skipped (outside the shard, negative, -1 padding) or whose document has no vectors gets
 *     out_val = NaN, out_tok = -1 and out_dist = NaN;
 *   - a query without vectors owns no rows of out_val / out_tok, its out_dist row is NaN, and no pair of mi355dr_maxsim_map may
 *     name it with a non-empty slot.
 * Consequence: out_dist is bit for bit what mi355dr_maxsim_subset_ex returns for the same arguments and flags, NaN cells at the
 * same places; -out_val summed in fp32 in vector order gives the same bits; every element of a map is the orc_dot of its two
 * vectors, a map's row maxima are the unclamped out_val and their first argmax is out_tok.
 * All three run under the handle's mutex and are complete on return; a view refuses them (ask the parent).  MI355DR_E_INVALID:
 * an unknown flag, B < 0, m < 0, P < 0, n < 0, a null pointer with work to do, a decreasing q_offsets, a pair_query outside
 * [0, B), a slot of the wrong size.  MI355DR_E_UNSUPPORTED: dim > 1272 (the exact kernel's LDS bound).  Every allocation
 * precedes the first launch: MI355DR_E_NOMEM changes nothing.  B = 0, m = 0 or P = 0 is a no-op that still fills what it owns
 * with NaN / -1.  A query of more than 128 vectors (d = 768: 32) is scored in tiles of its vectors; the tiles are independent.
 * Stats: "maxsim_align_calls", "maxsim_align_pairs" ((query, document) pairs scored), "maxsim_map_calls", "maxsim_map_values"
 * (floats written).  No other stat moves. */

/* tokens of stored documents.  doc_ids: HOST [n] GLOBAL ids under the rule of mi355dr_maxsim_subset (local + "row_offset").
 * out_counts[j] = number of token vectors; 0 = a document without vectors (never given any, or removed);
 * -1 = an id outside this shard.  Read from the host table, no device work. */
int mi355dr_multivec_token_counts(mi355dr_index* idx, const int64_t* doc_ids, int64_t n, int32_t* out_counts);

/* alignment of every query with its own row of candidates (the shapes of mi355dr_maxsim_subset_ex: doc_ids HOST [B, m]).
 *   V = q_offsets[B] query vectors in all; for global query vector g = q_offsets[b] + i and candidate position p:
 *   out_val[g*m + p]  fp32: that vector's term of the sum, v = max_j <q_i, d_j> (with MI355DR_MAXSIM_CLAMP0: max(0, v)).
 *   out_tok[g*m + p]  int32: the LOWEST token index j of the document whose dot equals the unclamped maximum;
 *                     -1 where there is none (see the rule).
 *   out_dist[b*m + p] fp32, optional (NULL: not wanted): acc = 0.0f; acc = acc + (-out_val) over i ascending. */
int mi355dr_maxsim_align(mi355dr_index* idx, const float* qtok, const int32_t* q_offsets, int B, const int64_t* doc_ids, int m,
                         int flags, float* out_val, int32_t* out_tok, float* out_dist);          /* all host */

/* full similarity maps of listed (query, document) pairs.  pair_query HOST [P] in [0, B); pair_doc HOST [P] global ids;
 * out_offsets HOST [P+1], non-decreasing element offsets into out.
 * Slot p must hold exactly nq_p * max(T_p, 0) floats, T_p as mi355dr_multivec_token_counts reports it;
 * any other size is MI355DR_E_INVALID and nothing is written.
 * out[out_offsets[p] + i*T_p + j] = <q_i, d_j>. */
int mi355dr_maxsim_map(mi355dr_index* idx, const float* qtok, const int32_t* q_offsets, int B, const int32_t* pair_query,
                       const int64_t* pair_doc, int64_t P, const int64_t* out_offsets, float* out); /* all host */

/* ---- MaxSim search within a listed subset of documents ----
 * `embeddings @# q ... WHERE embeddings IS NOT NULL AND id = ANY(:ids) ORDER BY distance LIMIT k`: maxsim_search
 * (orm/repository/base.py:487-535) with a key filter -- one tenant's pages, one PDF's passages.  The multi-vector sibling of
 * mi355dr_search_subset: ONE list shared by all B queries, the top-k selected on the device.
 *   Result: the top-k of every query among the listed documents only.  The fp32 distance bits, the order (distance asc,
 *     document asc) and the NaN / -1 tail when fewer than k listed documents have vectors are those of mi355dr_search_maxsim.
 *     Equivalently: the (distance, document) ordering of mi355dr_maxsim_subset over the list, and mi355dr_search_maxsim on
 *     mi355dr_view_create(parent, NULL, 0, doc_ids, m).
 *   doc_ids: HOST [m], GLOBAL ids (local document + option "row_offset"), under the hygiene of mi355dr_search_subset: values
 *     outside the shard are skipped (negative values and -1 padding included), a value listed twice counts once, the order
 *     never matters.  Documents without vectors -- never given any, or removed by mi355dr_set_multivec -- are skipped.
 *   m == 0, or no listed document with vectors: every output is NaN / -1.  A query without vectors gets a NaN / -1 row.
 *     m < 0, a null list with m > 0, k <= 0 or a decreasing q_offsets: MI355DR_E_INVALID.  k > 1024: MI355DR_E_UNSUPPORTED.
 *   The call runs under the handle's mutex and is complete on return; the _device form follows the stream rule of
 *     mi355dr_search_maxsim_device (doc_ids and q_offsets stay on the HOST).  The list is made local, sorted and uploaded as
 *     int32, together with a membership table of 8 bytes per stored document, into buffers the store owns and grows, before
 *     anything is launched; a failed allocation returns MI355DR_E_NOMEM and changes nothing.
 *   Two paths with identical results, option "maxsim_subset_screen":
 *     exact list path  the exact fp32 kernel walks the list, up to 4 queries per launch, then the device top-k.  Small lists,
 *                      stores that cannot be screened (dims whose query fragments exceed the LDS, non-finite values), queries
 *                      with non-finite vectors or with more vectors than one launch stages.
 *     list screen      the one-wave-per-document bf16 MFMA screens read the listed documents where they lie (grid sized by
 *                      the list), the selection kernels see the list through the membership table, the candidates are
 *                      re-scored exactly as in mi355dr_search_maxsim.  A query with more than 8192 candidates is re-run by the
 *                      exact list path.
 *     -1 (default): screen when at least "maxsim_subset_screen_min" listed documents have vectors (default 512: the smallest
 *     measured list, 1 000 of 1 M documents, rounded down to a power of two -- the screen won at every measured size, DESIGN.md
 *     section 4.8d); 0: never; 1: whenever the store can be screened.
 *   Stats: "maxsim_subset_searches" (calls), "maxsim_subset_docs" (listed documents with vectors, summed over calls),
 *     "maxsim_subset_screened" / "maxsim_subset_exact" (queries served by the list screen / by the exact list path, fallbacks
 *     included), "maxsim_subset_fallbacks" (queries whose candidate list overflowed).  The other "maxsim_*" stats belong to
 *     mi355dr_search_maxsim and do not move. */
int mi355dr_search_maxsim_subset(mi355dr_index* idx, const float* qtok, const int32_t* q_offsets, int B, int k,
                                 const int64_t* doc_ids, int64_t m, float* out_dist, int64_t* out_rows); /* all host */
int mi355dr_search_maxsim_subset_device(mi355dr_index* idx, const float* qtok_dev, const int32_t* q_offsets, int B, int k,
                                        const int64_t* doc_ids, int64_t m, float* out_dist_dev, int64_t* out_rows_dev,
                                        void* stream); /* doc_ids and q_offsets stay on the HOST */

/* ---- sparse store: tokenised documents, weighted / BM25 top-k scored on the device ----
 * The lexical leg of the hybrid pipelines (the reference's BM25RetrievalPipeline is one SQL statement against
 * VectorChord-BM25).  That extension's float4 arithmetic and pg_tokenizer's vocabularies cannot be pinned without a
 * PostgreSQL, so THIS HEADER FIXES THE ARITHMETIC ITSELF; agreement with the reference is claimed on the interface only
 * (signatures, the sign and order of scores, result dicts), never on score bits.
 *
 * Store.  Document i is a sequence of int32 term ids, any order, repeats allowed; tf(i,t) = occurrences of t in i, L_i = the
 *   sequence's length.  Ids are dense in insertion order and stable; a returned id is the local id + option "row_offset".  A
 *   document without tokens is stored and takes an id, but is not a document for the statistics and never matches.
 *   N = documents with tokens, total_len = sum of L_i, df(t) = documents with tf(i,t) > 0.
 * Limits.  A term id outside [0, 2^20): MI355DR_E_INVALID.  tf(i,t) > 4095: MI355DR_E_UNSUPPORTED.  At most 2^31 - 2
 *   documents.  A refused add changes nothing.  Several adds answer exactly as one add of the concatenation.
 * Weighted score (mi355dr_search_sparse*).  Query j is q_terms[q_offsets[j] .. q_offsets[j+1]) with weights alongside: DISTINCT
 *   terms in [0, 2^20), finite weights with |w| <= 1e30 (else E_INVALID; more than 1024 terms: E_UNSUPPORTED).  The library
 *   sorts a query's terms ascending.  Everything is IEEE double, one rounding per operation, no fused multiply-add:
 *       avgdl  = (double)total_len / (double)N
 *       norm_i = k1 * ((1.0 - b) + b * ((double)L_i / avgdl))
 *       score  = +0.0;  for t in the query's terms, ASCENDING term id, with tf = tf(i,t) > 0:
 *                    frac  = ((double)tf * (k1 + 1.0)) / ((double)tf + norm_i)
 *                    score = score + (w_t * frac)
 *       distance(i) = -score
 *   Document i MATCHES iff it holds at least one query term (a score of zero or below still matches).  A result line is the
 *   first k matches under (distance asc, NaN last, id asc), NaN / -1 behind them; a query with no term, or none that occurs,
 *   and every query over an empty store give an all NaN / -1 line.  k1 >= 0 finite and b in [0, 1], else E_INVALID; k > 1024:
 *   E_UNSUPPORTED; B above 1024 runs in internal blocks.
 * BM25 (mi355dr_search_bm25*).  A query is a raw token sequence: repeats count once, terms with df = 0 (or outside
 *   [0, 2^20)) are dropped, and the weights are computed ON THE HOST with libm's log,
 *       w_t = log(1.0 + (((double)(N - df) + 0.5) / ((double)df + 0.5)))
 *   then the weighted search runs.  No transcendental runs on the device.
 * Calls run under the handle's mutex, first complete whatever search is in flight, and are complete on return.  The _device
 *   forms take the QUERY on the host and write the results to device memory on `stream` (null: the handle's).  A failed
 *   allocation returns E_NOMEM with nothing changed.  The term-major device layout is brought up to date by the first search
 *   after an add / set / remove (host counting sort + upload); the host keeps the documents as sorted (term, tf) pairs, 6 bytes
 *   per posting.
 * Replace and remove (mi355dr_set_sparse, mi355dr_remove_sparse).  set: document doc_ids[j] becomes the token sequence
 *   terms[offsets[j] .. offsets[j+1]), under the limits of the add.  remove: a set with an empty sequence -- the document stays
 *   stored and keeps its id, never matches and leaves N, total_len and df; a later set with tokens revives it.  Ids and
 *   mi355dr_size_sparse never change; mi355dr_live_sparse is N.  doc_ids are LOCAL ids (no "row_offset"), each in
 *   [0, mi355dr_size_sparse) and listed once per call; else, and for a null buffer with n > 0 or decreasing offsets,
 *   E_INVALID and nothing changes.  n = 0 is a no-op; a view refuses both.  CONTRACT: after any sequence of add / set / remove
 *   every search (all distance bits, ids, tails), mi355dr_sparse_df and the stats "sparse_docs", "sparse_total_len",
 *   "sparse_postings", "sparse_vocab" (the largest term id with df > 0, plus one: it can shrink) equal those of a fresh handle
 *   given ONE mi355dr_add_sparse of the current documents.
 *   On the device the store is the BASE (the layout of the last full build), one `moved` bit per document whose content is no
 *   longer the base's (replaced, emptied, or appended since), and the OVERLAY, a second layout of the same format with the
 *   current postings of the moved documents.  The first search after a mutation rebuilds the overlay alone while its postings
 *   are at most "sparse_overlay_max_pct" percent of the base's, else the whole layout (the overlay is then empty).  A store
 *   without moved documents is scored by the same kernel as before these calls existed.
 * Options: "sparse_tile_docs" (documents per LDS tile, a power of two 256 .. 8192, default 2048), "sparse_cand_cap" (slots of a
 *   query's candidate list, 16 .. 2048 [default]; a list that overflows is dropped whole and its document range run again in
 *   pieces that cannot overflow -- same results), "sparse_overlay_max_pct" (0 .. 100, default 25; 0: every mutation takes a
 *   full build).  Stats: "sparse_docs" (N), "sparse_total_len", "sparse_postings" (distinct
 *   (doc, term) pairs), "sparse_vocab" (largest term id + 1), "sparse_searches" (calls), "sparse_queries",
 *   "sparse_postings_scored", "sparse_overflows" ((query, launch) lists run again), "sparse_full_builds",
 *   "sparse_overlay_builds", "sparse_overlay_postings" (the overlay's size as last built), "sparse_dead_postings" (base postings
 *   of moved documents, as last built), "sparse_sets" (documents set or removed); the store's device bytes, overlay and
 *   `moved` included, are part of "hbm_bytes_resident".
 * Within a listed subset (mi355dr_search_sparse_subset*, mi355dr_search_bm25_subset*, mi355dr_score_sparse_subset,
 *   mi355dr_score_bm25_subset).  A FILTER, NOT A VIEW: N, total_len, avgdl, df, and so every BM25 weight and every norm_i, are
 *   those of the WHOLE store -- a listed document's distance is bit for bit the distance the unrestricted search computes for
 *   it.  doc_ids are GLOBAL ids as the searches return them (local id + option "row_offset"), on the HOST, under the rule of
 *   mi355dr_search_subset: values outside [row_offset, row_offset + mi355dr_size_sparse) are skipped (negative values and -1
 *   padding included), a value listed twice counts once, order never matters.  A listed document without tokens never matches.
 *   search_*_subset: one list [m] shared by all B queries.  A result line is the unrestricted ranking -- ALL matches under
 *     (distance asc, NaN last, id asc) -- with the unlisted documents struck out, cut to k, NaN / -1 behind.  Queries, k / k1 / b,
 *     blocks, mutex, drain, stream and the _device convention (query and list on the host, results on the device, complete on
 *     return) are those of mi355dr_search_sparse / _bm25.  m == 0, no listed document in range, or an empty store (a view's):
 *     every line all NaN / -1.  m < 0, or a null list with m > 0: E_INVALID.
 *   score_*_subset: every query has its OWN list, row q of doc_ids [B, m]; out_dist[q, j] (HOST) is the distance (-score) of
 *     query q to doc_ids[q, j], NaN where the id is skipped or the document does not match the query.  A duplicate in a row is
 *     scored in every position it occupies.  m == 0 or B == 0: no-op.  B * m must be below 2^31 (else E_UNSUPPORTED).
 *   Two exact paths serve a mutated store as well as an untouched one.  A list of at most "sparse_subset_pairs_max" local
 *     documents (option, 0 .. "sparse_cand_cap", default 2048; 0: never; above the cap: E_INVALID; a cap lowered afterwards
 *     bounds it), and every score form, looks each (query, document) pair up by binary search in the query's term slices.  A
 *     longer list runs the search's own launches over the tiles that hold a listed document, filtered by a bitmap, planned in
 *     LISTED documents (the first launch holds at most "sparse_cand_cap" of them, an overflowed one is run again in pieces of
 *     at most that many).  Same bits on both paths.
 *   Stats: "sparse_subset_searches" (calls of the four search forms; they count in "sparse_queries", not in
 *     "sparse_searches"), "sparse_subset_scores" (calls of the two score forms), "sparse_subset_pairs" ((query, document) pairs
 *     looked up), "sparse_subset_tiles" (tiles launched by the filtered pass, summed over launches).  "sparse_postings_scored"
 *     counts on both paths exactly the (query term, listed document) postings that were added (for a score form: per position).
 *     The list's device buffers belong to the store and are part of "hbm_bytes_resident".
 * Views: a view has an empty sparse store and refuses mi355dr_add_sparse / _set_sparse / _remove_sparse; mi355dr_compact does
 *   not touch the sparse store.
 * Out of scope: compaction / renumbering of sparse documents (ids are table positions in the service), views over the store,
 *   any claim of bit parity with VectorChord-BM25.  No longer on this list: fusion on the device of a sparse list with a dense
 *   one, which has its own section -- "hybrid fusion" below --, and the search over a row-sharded store with global df / avgdl,
 *   which has its own too -- "row-sharded sparse search" below. */
int mi355dr_add_sparse(mi355dr_index* idx, const int32_t* terms, const int64_t* offsets /* [n_docs + 1] */, int64_t n_docs); /* host */
int64_t mi355dr_size_sparse(const mi355dr_index* idx); /* stored documents, with or without tokens */
int mi355dr_set_sparse(mi355dr_index* idx, const int64_t* doc_ids /* HOST [n] */, const int32_t* terms,
                       const int64_t* offsets /* HOST [n + 1] */, int64_t n);
int mi355dr_remove_sparse(mi355dr_index* idx, const int64_t* doc_ids /* HOST [n] */, int64_t n);
int64_t mi355dr_live_sparse(const mi355dr_index* idx); /* documents with tokens = N of the statistics */
int mi355dr_sparse_df(mi355dr_index* idx, const int32_t* terms, int64_t n, int64_t* out_df); /* 0 for unseen / out-of-range terms */
int mi355dr_search_sparse(mi355dr_index* idx, const int32_t* q_terms, const double* q_weights, const int32_t* q_offsets /* [B + 1] */,
                          int B, int k, double k1, double b, double* out_dist /* [B, k] */, int64_t* out_rows /* [B, k] */);
int mi355dr_search_sparse_device(mi355dr_index* idx, const int32_t* q_terms, const double* q_weights, const int32_t* q_offsets,
                                 int B, int k, double k1, double b, double* out_dist_dev, int64_t* out_rows_dev, void* stream);
int mi355dr_search_bm25(mi355dr_index* idx, const int32_t* q_tokens, const int32_t* q_offsets /* [B + 1] */, int B, int k, double k1,
                        double b, double* out_dist, int64_t* out_rows);
int mi355dr_search_bm25_device(mi355dr_index* idx, const int32_t* q_tokens, const int32_t* q_offsets, int B, int k, double k1,
                               double b, double* out_dist_dev, int64_t* out_rows_dev, void* stream);
int mi355dr_search_sparse_subset(mi355dr_index* idx, const int32_t* q_terms, const double* q_weights, const int32_t* q_offsets,
                                 int B, int k, double k1, double b, const int64_t* doc_ids /* HOST [m] */, int64_t m,
                                 double* out_dist /* [B, k] */, int64_t* out_rows /* [B, k] */);
int mi355dr_search_sparse_subset_device(mi355dr_index* idx, const int32_t* q_terms, const double* q_weights, const int32_t* q_offsets,
                                        int B, int k, double k1, double b, const int64_t* doc_ids /* HOST [m] */, int64_t m,
                                        double* out_dist_dev, int64_t* out_rows_dev, void* stream);
int mi355dr_search_bm25_subset(mi355dr_index* idx, const int32_t* q_tokens, const int32_t* q_offsets, int B, int k, double k1,
                               double b, const int64_t* doc_ids /* HOST [m] */, int64_t m, double* out_dist, int64_t* out_rows);
int mi355dr_search_bm25_subset_device(mi355dr_index* idx, const int32_t* q_tokens, const int32_t* q_offsets, int B, int k, double k1,
                                      double b, const int64_t* doc_ids /* HOST [m] */, int64_t m, double* out_dist_dev,
                                      int64_t* out_rows_dev, void* stream);
int mi355dr_score_sparse_subset(mi355dr_index* idx, const int32_t* q_terms, const double* q_weights, const int32_t* q_offsets,
                                int B, double k1, double b, const int64_t* doc_ids /* HOST [B, m] */, int m,
                                double* out_dist /* HOST [B, m] */);
int mi355dr_score_bm25_subset(mi355dr_index* idx, const int32_t* q_tokens, const int32_t* q_offsets, int B, double k1, double b,
                              const int64_t* doc_ids /* HOST [B, m] */, int m, double* out_dist /* HOST [B, m] */);

/* ---- hybrid fusion: two ranked lists per query fused into one on the device ----
 * The last step of a hybrid retrieval -- Reciprocal Rank Fusion, or a convex combination of normalised scores -- over the two
 * legs' lists where the searches left them: a dense leg's (mi355dr_search_device) and a lexical leg's
 * (mi355dr_search_bm25_device).  One launch for a page of queries; the arithmetic below is fixed operation for operation.
 *   Inputs: two lists per query, vals_l [B, w_l] double and ids_l [B, w_l] int64 for l = 1, 2, with 1 <= w_l <= 1024.
 *   Entries: an entry is NO entry when its id is < 0 (wherever it stands), when its value is NaN, or when a map is given for
 *     its list and id >= map_len or map[id] < 0.  map_l: optional device int64 [map_len_l] that translates the list's ids into
 *     the common id space, NULL = identity (a dense index's rows are not table positions once a chunk has no embedding).  The
 *     rank of an entry is 1 + the number of entries before it in its list: struck-out slots do not count.  Within one list a
 *     (mapped) id occurs once; if it does not, that query's line is unspecified, but the call stays memory-safe and ends.
 *   Score of an entry, one mode per list: MI355DR_FUSE_ONE_MINUS s = 1.0 - v (a cosine distance); MI355DR_FUSE_NEGATE s = -v,
 *     a sign flip (-0.0 for +0.0; a BM25 distance); MI355DR_FUSE_AS_IS s = v.
 *   Union order ("first seen"): list 1's entries in list order, then list 2's entries whose id is not in list 1, in list 2's
 *     order.  pos(d) is a document's index in that order.
 *   Arithmetic: IEEE double, one rounding per operation, no fused multiply-add, no transcendental function; sqrt is the
 *     correctly rounded one.
 *   MI355DR_FUSE_RRF (rrf_k >= 0, and fetch_k with rrf_k + fetch_k + 1 > 0), for document d: f = 0.0; if d is in list 1 at rank
 *     r1: f = f + 1.0 / (double)(rrf_k + r1); if d is in list 2 at rank r2: f = f + 1.0 / (double)(rrf_k + r2); if d is in
 *     exactly one list: f = f + 1.0 / (double)(rrf_k + fetch_k + 1).
 *   MI355DR_FUSE_CC_MM / _CC_TMM / _CC_Z / _CC_DBSF (weight; min_1, min_2 for TMM): column l holds the scores of the union's
 *     documents that list l holds IN UNION ORDER (for list 2: the documents shared with list 1 first, in list 1's order).
 *     Statistics over a column's n present scores: min, max (the first of equal values: +0.0 / -0.0);
 *     mean = (((0.0 + s_0) + s_1) + ...) / (double)n; var = (((0.0 + (s_0 - mean) * (s_0 - mean)) + ...)) / (double)n, both
 *     plain left-to-right sums; std = sqrt(var).  Normalised score a of a present score s:
 *       MM    (s - min) / (max - min);   0.5 when max - min == 0
 *       TMM   (s - min_l) / (max - min_l);   0.5 when max - min_l == 0
 *       Z     (s - mean) / std;   0.0 when std == 0
 *       DBSF  lo = mean - 3.0 * std, span = (mean + 3.0 * std) - lo, x = (s - lo) / span, y = x < 1.0 ? x : 1.0,
 *             a = y > 0.0 ? y : 0.0;   0.5 when std == 0
 *     A document absent from a list takes the floor AFTER normalisation: MM 0.0, TMM 0.0, Z -3.0, DBSF 0.0; an empty column
 *     has no statistics and all its entries are floors.  f = (weight * a_1) + ((1.0 - weight) * a_2).
 *   Result line: the union sorted by f descending under IEEE comparison (+0.0 and -0.0 equal; NaN, which only infinite inputs
 *     produce, last), ties by pos ascending -- a stable descending sort over first-seen order.  The first k_out are written as
 *     (f with its own bits, common id); behind them NaN / -1.  count[q] = the size of the union (it may exceed k_out; the
 *     pointer may be NULL).  Two empty lists: all NaN / -1 and 0.
 *   mi355dr_fuse_lists_device: over device lists.  Stateless like mi355dr_merge_groups_device (it reads no index state: the
 *     lists may come from two handles on the same GPU; allowed on a view); under the handle's mutex; complete on return.
 *   mi355dr_fuse_lists: the same with lists, maps and results on the host, staged through buffers the index owns and grows; a
 *     failed allocation returns MI355DR_E_NOMEM with nothing changed.
 *   MI355DR_E_INVALID: B < 0, w_l <= 0, k_out <= 0, a null pointer with work to do (lists, results, opts; a map with
 *     map_len < 0), an unknown mode or method, rrf_k < 0 or rrf_k + fetch_k + 1 <= 0 (RRF), a non-finite weight (CC), a
 *     non-finite minimum (TMM).  MI355DR_E_UNSUPPORTED: w_l > 1024, k_out > 2048.  B == 0 is a valid no-op.  A refused call
 *     changes nothing.
 *   Stats: "fuse_calls", "fuse_queries" (B, summed); both entry points.
 *   Out of scope: more than two lists, MaxSim legs (their score has a per-query divisor), row-sharded hybrids. */
#define MI355DR_FUSE_RRF 0
#define MI355DR_FUSE_CC_MM 1
#define MI355DR_FUSE_CC_TMM 2
#define MI355DR_FUSE_CC_Z 3
#define MI355DR_FUSE_CC_DBSF 4
#define MI355DR_FUSE_ONE_MINUS 0
#define MI355DR_FUSE_NEGATE 1
#define MI355DR_FUSE_AS_IS 2
typedef struct {
    int method;         /* MI355DR_FUSE_RRF | _CC_MM | _CC_TMM | _CC_Z | _CC_DBSF */
    int mode_1, mode_2; /* MI355DR_FUSE_ONE_MINUS | _NEGATE | _AS_IS */
    int rrf_k, fetch_k; /* RRF */
    double weight, min_1, min_2; /* CC; the minima: TMM */
} mi355dr_fuse_opts;
int mi355dr_fuse_lists_device(mi355dr_index* idx, const double* vals1_dev, const int64_t* ids1_dev, int w1, const int64_t* map1_dev,
                              int64_t map1_len, const double* vals2_dev, const int64_t* ids2_dev, int w2, const int64_t* map2_dev,
                              int64_t map2_len, int B, int k_out, const mi355dr_fuse_opts* opts, double* out_vals_dev,
                              int64_t* out_ids_dev, int32_t* out_count_dev /* may be NULL */, void* stream);
int mi355dr_fuse_lists(mi355dr_index* idx, const double* vals1, const int64_t* ids1, int w1, const int64_t* map1, int64_t map1_len,
                       const double* vals2, const int64_t* ids2, int w2, const int64_t* map2, int64_t map2_len, int B, int k_out,
                       const mi355dr_fuse_opts* opts, double* out_vals, int64_t* out_ids, int32_t* out_count /* may be NULL */); /* all host */

/* ---- source-capped lists and search: at most c results per source, on the device ----
 * Every retrieval unit has a source -- a chunk its document, an image chunk its page, a near-duplicate its cluster -- and a top-k
 * often spends most of k on one of them.  These entry points answer "the best k, at most cap per source" (Elasticsearch's
 * collapse, Qdrant's and Milvus' group search) over lists where the searches leave them, and as a search that deepens only the
 * queries that need it.
 *   Key table: keys int64 [keys_len], indexed by the id exactly as a list carries it -- the global id as the searches return it
 *     (the parent's ids on a view, global rows under a communicator, the common id space after a fusion).  An entry HAS a key
 *     when 0 <= id < keys_len and keys[id] >= 0; otherwise it has none (a NULL table with keys_len == 0: no entry has one).
 *     Every non-negative int64, INT64_MAX included, is a real key: "no key" travels as a bit of its own, not as a value.
 *   The walk, over one list of w (value, id) entries IN THE ORDER GIVEN (the list order is the ranking; nothing is re-sorted by
 *     value): a slot with id < 0 is no entry; a slot with an id and a NaN value is one (an irregular row's result).  An entry is
 *     KEPT iff it has no key, or fewer than cap earlier entries of the same list have its key; an id listed twice is two
 *     entries.  Output: the first k_out kept entries in list order -- the value with the bits it came with (+0.0, -0.0, +-inf
 *     and NaN payloads untouched), the id as given -- and NaN / -1 behind them.  Optional outputs (NULL skips one):
 *     out_keys [B, k_out] int64, the key, -1 for no key and for tail slots; out_pos [B, k_out] int32, the entry's slot in the
 *     input list, -1 for tail slots; out_count [B] int32, kept entries of the WHOLE list (it may exceed k_out); out_entries [B]
 *     int32, entries of the list.
 *   mi355dr_collapse_lists_device: over device lists.  Stateless like mi355dr_merge_groups_device (it reads no index state: the
 *     lists may be another handle's; allowed on a view); under the handle's mutex; complete on return.
 *   mi355dr_collapse_lists: the same with lists, table and results on the host, staged through buffers the index owns and grows
 *     (they count in "hbm_bytes_resident"); a failed allocation returns MI355DR_E_NOMEM with nothing changed.
 *   MI355DR_E_INVALID: B < 0, w <= 0, cap <= 0, k_out <= 0, keys_len < 0, a null pointer with work to do (lists, results, a
 *     null table with keys_len > 0), a non-null table with keys_len == 0.  MI355DR_E_UNSUPPORTED: w > 4096, k_out > 4096.
 *     B == 0 is a valid no-op.  A refused call changes nothing.
 *   mi355dr_search_collapsed / _device: the result of query q is the walk over q's ranking -- the ordinary search's total order
 *     -- cut to its first max_fetch entries, at k_out = k.  out_count[q]: lines written, at most k.  out_state[q] has
 *     MI355DR_COLLAPSE_TRUNCATED iff fewer than k were kept ALTHOUGH the ranking was cut (it had max_fetch entries).  out_keys,
 *     out_count and out_state may be NULL.  keys: HOST in the host form, device in the _device form; keys == NULL returns the
 *     bits of mi355dr_search at k.  1 <= k <= fetch_k <= max_fetch <= 1024, else MI355DR_E_INVALID (above 1024:
 *     MI355DR_E_UNSUPPORTED); cap and the table under the rules above.
 *   Schedule: the result does not depend on fetch_k, only the cost does.  The block is searched at f = fetch_k (screened, fix-ups
 *     completed) and collapsed; a query is finished when it kept k, when its ranking ended (entries < f), or when f ==
 *     max_fetch.  The unfinished queries, and only they, are gathered and searched again at min(2 f, max_fetch), their lists
 *     collapsed into their own result lines; and so on.  Exact, because under the total order the top-f list is a prefix of the
 *     top-2f list and the verdict on an entry depends on the entries before it alone.
 *   B above 1024 runs in internal blocks; the call first completes whatever search is in flight and is complete on return; it
 *     works on a view (it takes no global ids as input: the table is indexed by the parent's ids the view returns).
 *   mi355dr_search_collapsed_sharded_device: the same over the communicator (the sharded block search in the local one's
 *     place): mi355dr_comm_init first, a view refuses, world * max_fetch <= 4096 (else MI355DR_E_UNSUPPORTED).  Every rank
 *     passes the same arguments, sees the same merged lists, takes the same decisions and makes the same collective calls.
 *   Stats: "collapse_calls" (the list forms), "collapse_searches" (the search forms), "collapse_queries" (their B, summed),
 *     "collapse_researched" ((query, round) re-searches, summed), "collapse_truncated" (queries returned truncated). */
#define MI355DR_COLLAPSE_TRUNCATED 1
int mi355dr_collapse_lists_device(mi355dr_index* idx, const double* vals_dev, const int64_t* ids_dev, int w, int B,
                                  const int64_t* keys_dev /* may be NULL */, int64_t keys_len, int cap, int k_out,
                                  double* out_vals_dev, int64_t* out_ids_dev, int64_t* out_keys_dev /* may be NULL */,
                                  int32_t* out_pos_dev /* may be NULL */, int32_t* out_count_dev /* may be NULL */,
                                  int32_t* out_entries_dev /* may be NULL */, void* stream);
int mi355dr_collapse_lists(mi355dr_index* idx, const double* vals, const int64_t* ids, int w, int B, const int64_t* keys,
                           int64_t keys_len, int cap, int k_out, double* out_vals, int64_t* out_ids, int64_t* out_keys,
                           int32_t* out_pos, int32_t* out_count, int32_t* out_entries); /* all host */
int mi355dr_search_collapsed(mi355dr_index* idx, const float* queries, int B, int k, int cap, const int64_t* keys /* HOST */,
                             int64_t keys_len, int fetch_k, int max_fetch, double* out_dist, int64_t* out_rows,
                             int64_t* out_keys /* may be NULL */, int32_t* out_count /* may be NULL */,
                             int32_t* out_state /* may be NULL */);
int mi355dr_search_collapsed_device(mi355dr_index* idx, const float* queries_dev, int B, int k, int cap, const int64_t* keys_dev,
                                    int64_t keys_len, int fetch_k, int max_fetch, double* out_dist_dev, int64_t* out_rows_dev,
                                    int64_t* out_keys_dev, int32_t* out_count_dev, int32_t* out_state_dev, void* stream);
int mi355dr_search_collapsed_sharded_device(mi355dr_index* idx, const float* queries_dev, int B, int k, int cap,
                                            const int64_t* keys_dev, int64_t keys_len, int fetch_k, int max_fetch,
                                            double* out_dist_dev, int64_t* out_rows_dev, int64_t* out_keys_dev,
                                            int32_t* out_count_dev, int32_t* out_state_dev, void* stream);

/* ---- Guided Query Refinement of candidate pools (GQR hybrid pipeline) ----
 * Replaces the per-query numpy loops of autorag_research/pipelines/retrieval/gqr_hybrid.py: `_optimize_query_embedding`
 * (:321-340), `_optimize_query_multi_embedding` (:342-362), `_optimize_in_score_space` (:306-319).  Float64 throughout
 * (the reference's arithmetic type); a block of B queries is one launch, one workgroup per query; the candidate vectors
 * are the rows already resident in HBM, named by global row id.  Pools: host [B, P], live ids first, -1 padding after
 * (P <= 2048); comp_dist: host [B, P] complementary distribution (gqr_hybrid.py:436); out_scores: host [B, P], NaN at
 * padding.  n_steps > 0, learning_rate > 0, temperature > 0, 0 <= mixture_alpha <= 1 (:202-216), else MI355DR_E_INVALID.
 *   mi355dr_gqr_refine         queries: host [B, dim] float64; candidates = single-vector rows; out = refined cosine
 *   mi355dr_gqr_refine_maxsim  qtok: host [sum_nq, dim] float64, finite (else MI355DR_E_INVALID), q_offsets [B+1] (every
 *                              query >= 1 vector); candidates = multi-vector docs (each must have vectors); out = refined
 *                              mean-of-max late-interaction score
 *   mi355dr_gqr_refine_scores  no vectors: primary_scores host [B, P] float64 are the variables, counts[b] live entries */
int mi355dr_gqr_refine(mi355dr_index* idx, const double* queries, int B, const int64_t* cand_rows, int P,
                       const double* comp_dist, int n_steps, double learning_rate, double temperature,
                       double mixture_alpha, double* out_scores);
int mi355dr_gqr_refine_maxsim(mi355dr_index* idx, const double* qtok, const int32_t* q_offsets, int B,
                              const int64_t* doc_ids, int P, const double* comp_dist, int n_steps, double learning_rate,
                              double temperature, double mixture_alpha, double* out_scores);
int mi355dr_gqr_refine_scores(mi355dr_index* idx, const double* primary_scores, const int32_t* counts, int B, int P,
                              const double* comp_dist, int n_steps, double learning_rate, double temperature,
                              double mixture_alpha, double* out_scores);

/* ---- shard merge (multi-GPU): [world, B, k] gathered (dist,row) device buffers -> [B, k] ----
 * The merge functions only enqueue work on `stream` (NULL: the index's stream); synchronise that stream (or call
 * mi355dr_synchronize for the index stream) before reading the outputs on the host.  The index's stream is NON-BLOCKING: the
 * legacy default stream (handle 0 -- what NULL means here, and what a framework's "current stream" often is) is ordered
 * against it by nothing.  A caller whose inputs were produced on the default stream either passes a real stream of its own
 * (the merge then runs ON it, behind its producers and in front of its consumers) or synchronises on both sides itself. */
int mi355dr_merge_topk_device(mi355dr_index* idx, const double* dist_all_dev, const int64_t* rows_all_dev, int world,
                              int B, int k, double* out_dist_dev, int64_t* out_rows_dev, void* stream);

/* same merge on the PACKED layout one rank produces for a single all-gather: int64 [world][2][B][k], plane 0 = the
 * float8 distance bit patterns, plane 1 = rows.  mi355dr_pack_topk_device builds one rank's [2][B][k] block. */
int mi355dr_pack_topk_device(mi355dr_index* idx, const double* dist_dev, const int64_t* rows_dev, int B, int k,
                             int64_t* packed_dev, void* stream);
int mi355dr_merge_topk_packed_device(mi355dr_index* idx, const int64_t* packed_all_dev, int world, int B, int k,
                                     double* out_dist_dev, int64_t* out_rows_dev, void* stream);

/* ---- row-sharded search inside the library: one index = one shard on one GPU, one process per GPU.
 * Replaces nothing in the reference (its engine is one PostgreSQL server); it is the data-parallel form of
 * `ORDER BY distance LIMIT k` (orm/repository/base.py:409-415): every rank searches its rows with "row_offset" set, ONE
 * ncclAllGather (RCCL over xGMI) of the packed [2,B,k] (float8 distance bits, int64 global row) block per rank, then the
 * world*k -> k merge under the same total order: bit-identical to the single-GPU result on every rank.
 * RCCL is bound at run time (dlopen): a host that never calls these needs no librccl.  The 128-byte ncclUniqueId is
 * created on one rank (mi355dr_comm_unique_id) and handed to every rank through the host's own channel. */
int mi355dr_comm_unique_id(void* out_128_bytes, size_t len);
int mi355dr_comm_init(mi355dr_index* idx, int rank, int world, const void* nccl_unique_id, size_t id_len);
int mi355dr_comm_world(const mi355dr_index* idx);  /* 0 before mi355dr_comm_init */
/* the rank count RCCL itself reports for the communicator (ncclCommCount): what a caller logs to show that the collective
 * really spans N ranks; 0 before mi355dr_comm_init */
int mi355dr_comm_count(mi355dr_index* idx, int* out);
/* Transport plug-in: the same sharded search over an all-gather the HOST provides instead of RCCL -- MPI / UCX hosts, a node
 * whose ranks cannot meet in one RCCL communicator (RCCL refuses two ranks on one device: the two-ranks-on-one-GPU parity test
 * of tests/test_gpu_world2.py runs mi355dr_search_sharded_device through this entry).  `fn` gathers `bytes_per_rank` bytes from
 * every rank's `send_dev` into `recv_dev` (rank-major, device memory), either ordered on `stream` or complete on return, and
 * returns 0 on success; it is called from the thread that calls mi355dr_search_sharded_device, once per block, in the same
 * order on every rank.  Replaces a communicator set by mi355dr_comm_init (and vice versa); mi355dr_comm_count then reports
 * `world` as given. */
typedef int (*mi355dr_allgather_fn)(const void* send_dev, void* recv_dev, size_t bytes_per_rank, void* stream, void* user);
int mi355dr_comm_init_custom(mi355dr_index* idx, int rank, int world, mi355dr_allgather_fn fn, void* user);
/* device buffers in / out like mi355dr_search_device; every rank passes the same queries and receives the same result.
 * Blocks of 1024 queries are software-pipelined: block i + 1 is searched while block i's all-gather + merge run on the
 * index's communication stream (two packed / gathered buffers).  Asynchronous on `stream` (NULL = the index's own stream):
 * on return `stream` has been made to wait for the last merge. */
int mi355dr_search_sharded_device(mi355dr_index* idx, const float* queries_dev, int B, int k, double* out_dist_dev,
                                  int64_t* out_rows_dev, void* stream);

/* ---- the derived searches over a row-sharded index: range, by stored row, MMR ----
 * The contract of mi355dr_search_sharded_device: every rank passes the same arguments, and every rank receives what ONE index
 * holding the rows of all shards would have returned from the local entry point of the same name -- float8 bits, global rows,
 * NaN positions, NaN / -1 tails and counts.  All need a communicator (mi355dr_comm_init or mi355dr_comm_init_custom; else
 * MI355DR_E_INVALID) and refuse a view (ask the parent); otherwise they carry the argument rules of their local forms.
 *   mi355dr_search_range_sharded_device: the list and count of mi355dr_search_range on the union of the shards.  Each rank's
 *     local list is its shard's first max_results in-range rows, so the world x max_results -> max_results merge under the
 *     total order gives the global list; the counts add.  One all-gather per block of [2, nb, max_results] + [nb] int64.
 *   mi355dr_search_rows_sharded_device / mi355dr_search_range_rows_sharded_device: the query of slot b is the stored vector of
 *     row_ids[b] (HOST, global) on whichever rank owns it.  A slot nobody owns -- an id outside every shard, -1, a removed row
 *     -- gives NaN / -1 and count 0 and adds one to "rows_skipped" on every rank.  Self-exclusion, MI355DR_ROWS_INCLUDE_SELF and
 *     the range form's "was the row itself in range, decided from the row-with-itself distance" are as in the local forms (the
 *     owner computes that distance).  Per block one all-gather of the slots' payloads -- nb x dim floats, nb int32 valid, nb
 *     double self distances, each part padded to 8 bytes --, folded on the device (the lowest rank whose valid is set), then
 *     the sharded pass at k + 1 / max_results + 1 (k / max_results with INCLUDE_SELF) and the local form's k_rows_drop.
 *   mi355dr_search_mmr_sharded_device / mi355dr_mmr_select_sharded: the picks of mi355dr_search_mmr / mi355dr_mmr_select on the
 *     union.  The candidate list is the sharded search at fetch_k, or the caller's pool (HOST, global rows, the hygiene of
 *     mi355dr_mmr_select: every rank scores the listed rows it owns, one all-gather of [2, nb, m] int64 -- global row or -1
 *     for "not mine", distance bits -- and every rank orders the union alike).  The similarity of two stored rows uses the
 *     same fp32 fmaf chain and the same stored norms whichever GPUs the rows lie on: per sub-block of queries the owners stage
 *     each candidate's vector, |row|^2 and an owned flag, one all-gather, and the selection of k_mmr_select reads candidate i
 *     from its owner's stage.  Option "shard_stage_bytes" (default 256 MiB, any value >= 1; never below one query's worth)
 *     caps the gathered stage: world x round_up4(queries x width x (dim + 2)) floats per sub-block.
 *   MI355DR_E_UNSUPPORTED beyond the local rules: world x width > 4096 (the merge's sort), width = k + 1 / max_results + 1 (k /
 *     max_results with INCLUDE_SELF), max_results for the range form, fetch_k for the MMR search.  A refused call changes
 *     nothing and enters no collective; all checks run before the first collective and depend on the arguments and `world`
 *     alone, so every rank refuses alike.  B == 0 is a valid no-op where the local form has it (not the range form).
 *   Unlike mi355dr_search_sharded_device these calls are complete on return, like their local forms, and are not pipelined
 *     across blocks; B above 1024 runs in internal blocks.  A rank whose shard is empty still enters every collective.  A
 *     transport error returns MI355DR_E_HIP after the stream has been drained.  The transport plug-in's `fn` is called once
 *     per all-gather with the call's stream; the payload is complete before it is called.
 *   Stats: "sharded_range_searches" / "sharded_rows_searches" / "sharded_mmr_searches" (calls), "shard_gather_bytes" (bytes this
 *     rank received through the all-gathers of these entry points: world x bytes_per_rank each).  The local stats move as the
 *     inner work moves them: "range_queries", "range_in_range" (this shard's counts), "rows_queries", "rows_skipped" (slots NO
 *     rank owned), "mmr_queries", "mmr_pairs_scored"; the call counters of the local entry points stay. */
int mi355dr_search_range_sharded_device(mi355dr_index* idx, const float* queries_dev, int B, const double* radius /* HOST [B] */,
                                        int max_results, double* out_dist_dev, int64_t* out_rows_dev, int64_t* out_count_dev,
                                        void* stream);
int mi355dr_search_rows_sharded_device(mi355dr_index* idx, const int64_t* row_ids /* HOST [B], global */, int B, int k, int flags,
                                       double* out_dist_dev, int64_t* out_rows_dev, void* stream);
int mi355dr_search_range_rows_sharded_device(mi355dr_index* idx, const int64_t* row_ids /* HOST [B] */, int B,
                                             const double* radius /* HOST [B] */, int max_results, int flags,
                                             double* out_dist_dev, int64_t* out_rows_dev, int64_t* out_count_dev, void* stream);
int mi355dr_search_mmr_sharded_device(mi355dr_index* idx, const float* queries_dev, int B, int k, int fetch_k, double lambda,
                                      double* out_dist_dev, int64_t* out_rows_dev, void* stream);
int mi355dr_mmr_select_sharded(mi355dr_index* idx, const float* queries, int B, int k, const int64_t* cand_rows /* host [B, m], global */,
                               int m, double lambda, double* out_dist, int64_t* out_rows); /* all host */

/* ---- row-sharded sparse search: weighted / BM25 over shards with global statistics ----
 * One handle is one shard on one GPU: it holds a CONTIGUOUS run of the documents, with option "row_offset" set to the global id
 * of its first document, and a communicator (mi355dr_comm_init or mi355dr_comm_init_custom).  Arguments are those of the local
 * entry point of the same name: the search forms take queries and lists on the HOST, write results to device memory and take a
 * `stream`; the score forms are all host.
 * CONTRACT.  Every rank passes the same arguments, and every rank receives what the local entry point returns on ONE handle that
 *   was given ONE mi355dr_add_sparse of all shards' current documents in global id order: all distance bits, global ids and
 *   NaN / -1 tails; for the score forms the NaN positions too.  A shard that scored with its own N, total_len and df would
 *   return other bits, so the statistics are those of ALL shards:
 *   per call every rank contributes int64 [2 + T] -- its N (documents with tokens), its total_len, and its df of each of the T
 *   distinct in-range terms of the call's queries, ascending (BM25 forms; T = 0 for the weighted forms, whose weights are the
 *   caller's) --, one all-gather, and the rows are SUMMED on the device.  They are integers, so the sums are exact and the same
 *   on every rank.  Each rank then drops the terms with global df = 0 and computes avgdl, norm_i and w_t by the formulas of the
 *   sparse store above from the global N, total_len and df.  Weights are not exchanged: every rank calls log() on the same
 *   integers, and RANKS ARE ASSUMED TO RUN THE SAME libm (one that differs in the last bit of log breaks the parity, nothing
 *   else).
 *   search forms: per block of at most 1024 queries the shard is searched by the local machinery (a listed id outside the shard
 *   is skipped by the subset rule, so the shared list filters itself), the kept lists leave as the packed [2, nb, k] block of
 *   mi355dr_pack_topk_device, one all-gather, one world * k -> k merge (mi355dr_merge_topk_packed_device).  The store's keys and
 *   the merge sort under the same order -- distance ascending (-0.0 before +0.0), then id ascending --, so the merged list is
 *   the one handle's list.
 *   score forms: each rank writes its [B, m] distances, NaN for a pair it does not own or that does not match; one all-gather
 *   per launch; per position the value of the lowest rank whose value is not NaN -- at most one rank owns a document.
 * Rules.  Without a communicator: MI355DR_E_INVALID.  A view refuses (ask the parent).  world * k > 4096 (the merge's sort):
 *   MI355DR_E_UNSUPPORTED.  Otherwise the local form's rules.  Every check runs before the first collective and depends on the
 *   arguments and `world` alone, so all ranks refuse alike; a refused call changes nothing.  A rank whose shard has no document
 *   with tokens -- one that never called mi355dr_add_sparse included -- still enters every collective.  Global N = 0: every
 *   result line is NaN / -1 (every score NaN).  B == 0 (and m == 0 for the score forms) is a no-op without a collective.  Calls
 *   are complete on return; B above 1024 runs in internal blocks.  A transport error returns MI355DR_E_HIP after the stream has
 *   been drained.
 * Mutations (mi355dr_add_sparse / _set_sparse / _remove_sparse) on any rank are local, and the next sharded call sees them: the
 *   statistics are gathered on every call.  The local entry points on the same handle keep answering with the shard's own
 *   statistics; the norms are cached per (k1, b, avgdl), so the two kinds of call recompute them only when they alternate.
 * Stats: "sharded_sparse_searches" (calls of the four search forms), "sharded_sparse_scores" (calls of the two score forms);
 *   the gathered bytes add to "shard_gather_bytes".  The local "sparse_*" counters move as the inner work moves them
 *   ("sparse_queries", "sparse_postings_scored", "sparse_overflows", "sparse_subset_pairs", "sparse_subset_tiles", the builds);
 *   the call counters of the local entry points stay.  The payload buffers belong to the store ("hbm_bytes_resident").
 * Out of scope: fusing a sharded lexical list with a sharded dense one on the device (the hybrid fusion above stays one handle's). */
int mi355dr_search_sparse_sharded_device(mi355dr_index* idx, const int32_t* q_terms, const double* q_weights, const int32_t* q_offsets,
                                         int B, int k, double k1, double b, double* out_dist_dev, int64_t* out_rows_dev, void* stream);
int mi355dr_search_bm25_sharded_device(mi355dr_index* idx, const int32_t* q_tokens, const int32_t* q_offsets, int B, int k, double k1,
                                       double b, double* out_dist_dev, int64_t* out_rows_dev, void* stream);
int mi355dr_search_sparse_subset_sharded_device(mi355dr_index* idx, const int32_t* q_terms, const double* q_weights,
                                                const int32_t* q_offsets, int B, int k, double k1, double b,
                                                const int64_t* doc_ids /* HOST [m], global */, int64_t m, double* out_dist_dev,
                                                int64_t* out_rows_dev, void* stream);
int mi355dr_search_bm25_subset_sharded_device(mi355dr_index* idx, const int32_t* q_tokens, const int32_t* q_offsets, int B, int k,
                                              double k1, double b, const int64_t* doc_ids /* HOST [m], global */, int64_t m,
                                              double* out_dist_dev, int64_t* out_rows_dev, void* stream);
int mi355dr_score_sparse_subset_sharded(mi355dr_index* idx, const int32_t* q_terms, const double* q_weights, const int32_t* q_offsets,
                                        int B, double k1, double b, const int64_t* doc_ids /* HOST [B, m], global */, int m,
                                        double* out_dist /* HOST [B, m] */);
int mi355dr_score_bm25_subset_sharded(mi355dr_index* idx, const int32_t* q_tokens, const int32_t* q_offsets, int B, double k1, double b,
                                      const int64_t* doc_ids /* HOST [B, m], global */, int m, double* out_dist /* HOST [B, m] */);

/* ---- options / stats / timing ----
 * options: "path" (MI355DR_PATH_*), "screen_dtype" (MI355DR_SCREEN_*), "row_offset", "profile" (0/1: HIP-event
 *          timing of the dominant kernel), "chunk0_rows", "chunk_growth", "cand_cap", "prefilter16" (1: int8 screen only, a bf16 second
 *          screen of the surviving candidates before the exact re-score; default 0, same results), "maxsim_screen" (1: bf16 MFMA screen
 *          over every doc + exact re-score of the candidates [default], 0: exact kernel over every doc; same results),
 *          "screen_stream" (1 [default]: query blocks of at most 64 are screened by the streaming kernel -- resident query
 *          block, ring of row stages --, 0: by the tile kernel; same results), "screen_rq" (1 [default]: query blocks of more
 *          than 128 over an int8 shadow of at most 768 bytes per row are screened by k_screen_rq -- query operand resident in
 *          registers, rows alone through the LDS --, 0: by k_screen256c; same results).
 *          Round 3, all with identical results (A/B switches of the pass schedule): "starter" (1 [default]: sampled threshold
 *          estimator instead of the three smallest chunks, k <= 32), "defer_round_b" (1 [default]: prunes before the last one
 *          carry their survivors over instead of re-scoring them), "prune_companion" (1 [default]: general-form prune launch
 *          behind every one-wave prune), "scan_dma" (1 [default]: k_scan32, LDS-DMA staging, for dims that are a multiple
 *          of 32), "maxsim_persistent" (0 [default]), "maxsim_coop" (exact MaxSim on candidate lists: -1 [default] one workgroup per
 *          candidate for stores of long documents, 0 one wave, 1 always one workgroup), "i8_min_budget_x100" (AUTO keeps the int8 screen while the chunk-growth
 *          budget at this k is at least value / 100; default 25 = k <= 133).
 *          Round 4, MaxSim, all with identical results (A/B switches of the 16-query pass, dims <= 128): "maxsim_pass_groups"
 *          (1..4 [default 4] groups of <= 4 queries per screen pass), "maxsim_wg" (screen form from 8/9 column blocks of query
 *          vectors up: -1 [default] workgroup form, per-document sums parked for short documents / at once for long ones,
 *          0 one wave per document, 1 parked, 2 at once), "maxsim_wg_bps" (4 [default] / 2 token blocks per ring stage),
 *          "maxsim_wg_pipe" (1 [default]: a block's maxima folded between the next block's MFMAs), "maxsim_wg_min" (8 [default]
 *          / 9: fewest column blocks that take the workgroup form), "maxsim_aligned" (1 [default]: queries that are exactly
 *          one 32-column block are summed by the wave that holds them), "maxsim_tighten" (1 [default]: candidate band from the
 *          exact distances of the screen's top-k), "maxsim_subset_screen" (-1 [default] / 0 / 1) and "maxsim_subset_screen_min"
 *          (512 [default]): the two paths of mi355dr_search_maxsim_subset, described there; round 6: "prune_wide" (1 [default]: passes at 33 <= k <= 128 use the
 *          two-wave prune, a starter over "starter_rows_wide" [65536] rows and chunk ratios up to 4; 0 = the round-5 schedule),
 *          "screen_flush_sync" (1 [default]: the waves of a k_screen_rq workgroup flush their hit-lane queues at the same tiles;
 *          "screen_flush_lanes" [48] / "screen_flush_alone" [40] tune the period), "chunk_taper_x100" (0 [default] = 120 for
 *          prune_wide passes, 100 = uniform chunk ratios otherwise), "wide_inflation_x10" (the budget's inflation figure); "view_slice_rows" (staging slice of mi355dr_view_create);
 *          "maxsim_pack8" (MaxSim screen, passes of 32-vector queries in the workgroup form and passes of up to four column blocks: a second bf16 shadow whose documents are
 *          rounded up to 8-token granules instead of 32-token blocks, built on the first such pass and extended by the next one after an add -- -1
 *          [default]: when it has at least 5 % fewer blocks than the padded copy and its memory is there, 1: always, 0: never;
 *          identical results); "range_chunk_rows" and "range_slots" (mi355dr_search_range, described there).
 *          The speculative one-chunk pass (identical results): "speculate" (1 [default]: a first attempt at a
 *          k with an admissible m(k) -- 2 <= k <= 19 -- on a corpus of at least "spec_min_rows" [1048576] rows screens all rows
 *          in ONE launch at a threshold predicted from the starter's sample and verifies it against its own k-th best; 0: the
 *          chunk ladder; setting it also ends a suspension), "spec_shift_milli" (lab option, [-20000, 20000], default 0: moves
 *          the predicted threshold by value / 1000 standard deviations of the sample, so that a test can make it wrong).
 * stats:   "screen_launches", "screen_ns" (profile=1), "screen_rows" (all screen launches) and their k_screen256 share
 *          "screen256_launches", "screen256_ns", "screen256_rows"; "candidates", "rescored",
 *          "spec_passes" (speculative passes), "spec_miss_queries" / "spec_overflow_queries" (their queries whose k-th best did
 *          not justify the threshold / whose candidate list overflowed: re-run by the ladder, counted in "retry_queries" too,
 *          never held against the int8 screen), "spec_suspended" (1 while speculation is suspended: more than 1 % of a block
 *          failed; 16 passes that would have speculated, doubling up to 4096 with every later block that fails),
 *          "fallback_queries" (queries recomputed by the exact scan), "retry_queries" (queries whose candidate list
 *          overflowed and that were re-screened with the bf16 bound and slower chunk growth first), "i8_demoted" (AUTO
 *          gave up the int8 screen for this index after > 1 % of a block overflowed -- from "i8_demoted_k", the k of that
 *          block, upwards; smaller k keep int8), "starters", "chunks", "passes", "irregular_rows", "loose_rows" (rows outside the int8 shadow,
 *          irregular ones included), "screen_dtype_active" (MI355DR_SCREEN_BF16 / _I8: what AUTO resolves to now),
 *          "maxsim_screened" (queries served by the MaxSim screen), "maxsim_candidates" (docs re-scored exactly for them),
 *          "maxsim_fallbacks" (queries re-run by the exact full scan), "maxsim_screen_launches" / "maxsim_screen_ns" /
 *          "maxsim_exact_launches" / "maxsim_exact_ns" (profile=1), "maxsim_packed_launches" / "maxsim_packed_blocks" / "maxsim_packed_built" (screen launches over the
 *          granule-packed copy / its 32-token blocks / blocks written into it so far: a store that grows is packed from its new granules on), "maxsim_screen_cols" (query columns the screen launches
 *          multiplied every token by), "maxsim_set_docs" (documents rewritten by mi355dr_set_multivec) / "maxsim_moved_blocks"
 *          (32-token blocks its relayouts copied; 0 on the in-place path), "subset_searches" / "subset_rows_scored" /
 *          "subset_rerun_queries" (mi355dr_search_subset: calls, pairs scored, queries re-run in list-sized pieces),
 *          "mmr_searches" / "mmr_queries" / "mmr_pairs_scored" (mi355dr_search_mmr* and mi355dr_mmr_select, described there),
 *          "group_searches" / "group_subqueries" / "groups_merged" (mi355dr_search_groups* and mi355dr_merge_groups_device, described there),
 *          "fuse_calls" / "fuse_queries" (mi355dr_fuse_lists*, described there),
 *          "collapse_calls" / "collapse_searches" / "collapse_queries" / "collapse_researched" / "collapse_truncated"
 *          (mi355dr_collapse_lists* and mi355dr_search_collapsed*, described there),
 *          "range_searches" / "range_queries" / "range_in_range" / "range_candidates" / "range_rescored" / "range_redo_chunks" /
 *          "range_fallback_queries" (mi355dr_search_range*, described there),
 *          "rows_searches" / "rows_queries" / "rows_skipped" (mi355dr_search_rows* and mi355dr_search_range_rows*, described there),
 *          "examples_searches" / "examples_queries" / "examples_skipped" / "examples_skipped_slots" / "feedback_searches" (search by
 *          examples / feedback, described there),
 *          "maxsim_subset_searches" / "maxsim_subset_docs" / "maxsim_subset_screened" / "maxsim_subset_exact" /
 *          "maxsim_subset_fallbacks" (mi355dr_search_maxsim_subset, described there),
 *          "maxsim_align_calls" / "maxsim_align_pairs" / "maxsim_map_calls" / "maxsim_map_values" (MaxSim explained, described
 *          there),
 *          "view" / "view_rows" / "view_docs" (mi355dr_view_create: 1 on a view / the rows / the documents it holds),
 *          "hbm_bytes_resident" (the single-vector corpus with its shadows at its capacity + the multi-vector store's two
 *          images, offset table and granule-packed copy as allocated now + the staging and block state of the source-capped
 *          forms as grown so far). */
int mi355dr_set_option(mi355dr_index* idx, const char* key, int64_t value);
int mi355dr_get_stat(mi355dr_index* idx, const char* key, int64_t* out);
int mi355dr_reset_stats(mi355dr_index* idx);
/* HIP-event stopwatch on the index's stream (bench.py: kernel-side time of a timed region) */
int mi355dr_timer_start(mi355dr_index* idx);
int mi355dr_timer_stop(mi355dr_index* idx, double* elapsed_ms);
int mi355dr_synchronize(mi355dr_index* idx);

/* ---- raw device memory helpers for hosts that have no device allocator of their own (tests, bench) ---- */
int mi355dr_dev_alloc(mi355dr_index* idx, size_t bytes, void** out);
int mi355dr_dev_free(mi355dr_index* idx, void* p);
int mi355dr_dev_upload(mi355dr_index* idx, void* dst_dev, const void* src_host, size_t bytes);
int mi355dr_dev_download(mi355dr_index* idx, void* dst_host, const void* src_dev, size_t bytes);

/* ---- test hooks (used by tests/ only; exercise the production kernels on small inputs) ----
 * dense screen values t[b, r] for rows [row0,row0+n), n <= 2048: runs the screen kernel with thresholds at -inf.  With the
 * default options a range this short is below small_chunk_rows, so the kernel it reaches is k_screen (the 128 x 128 tile),
 * or k_screen_stream for B <= 64 -- whatever B is; k_screen256c and k_screen_rq are reached by mi355dr_debug_screen_hits. */
int mi355dr_debug_screen_dense(mi355dr_index* idx, const float* queries, int B, int64_t row0, int64_t n, float* out_t);
/* one production screen launch over rows [row0, row0 + n) with the caller's thresholds: the raw candidate lists.
 * thr: host [B], finite or -inf.  cap: list slots per query, 16 .. the capacity the lists are allocated for (4096).
 * out_count [B]: the device's counter (may exceed cap: the list then holds its first cap entries);
 * out_rows / out_vals: host [B, cap]; out_status [B]: the status word (bit 0 = a wave queue overflowed);
 * *out_kernel: which kernel the launch took (0 k_screen, 1 k_screen_stream, 2 k_screen256c, 3 k_screen_rq) -- steered by
 * the options small_chunk_rows, screen_rq, screen_stream, screen_dtype as in a search.
 * row0 must be a multiple of the tile edge (128; 256 if B > 128) and row0 + n <= size; n is not limited.
 * int8 screen: an entry whose row lies outside the int8 shadow (a loose, irregular or removed row: its accumulator is a
 * stale 0, the prune drops it) is marked by out_rows = -1 - row.
 * k_screen_rq's common flush period, which a search derives from k and the rows already seen, is two tiles here
 * (option screen_flush_sync = 0: none, as in a search). */
int mi355dr_debug_screen_hits(mi355dr_index* idx, const float* queries, int B, int64_t row0, int64_t n, const float* thr,
                              int cap, int* out_count, int32_t* out_rows, float* out_vals, int* out_status, int* out_kernel);
/* ONE pass of the MaxSim search, through the functions mi355dr_search_maxsim[_subset] itself calls, in their order (scratch and
 * constants, the pass plan, the query upload, the screen launch and -- k <= 64 -- the fast path's selection, lists and re-score),
 * handing back what the pass computed.  qtok / q_offsets / B / k as in mi355dr_search_maxsim; doc_ids / m as in
 * mi355dr_search_maxsim_subset (doc_ids = NULL: every document).  Before the screen launch the pass's rows of the screen
 * distances are filled with the bit pattern 0xFFFFFFFF: a word the screen did not write is recognisable.
 * MI355DR_E_INVALID, the handle as it was: the queries do not all fit one pass (at most 16, at most 512 vectors together for
 * dims <= 128, else the first group of four), a query has more vectors than one launch stages, the handle is a view or has no
 * multi-vector store, no listed document has vectors.  Moves no statistic and no option.
 * Outputs, all host:
 *   out_live [B]          row of each query in the pass, -1 for a query without vectors; n_live = the rows
 *   out_screen [B, n_docs] rows 0 .. n_live - 1: the screen distances as the kernel left them (row stride n_docs)
 *   out_two_e [B]         rows 0 .. n_live - 1: 2E as handed to the device (float, rounded up)
 *   out_lists [3, B, list_cap] / out_ctl [3, B, 2]: sections 0 = wide, 1 = starter, 2 = final list of each row and their
 *                         (count, overflow flag), k <= 64 only; a list holds min(count, 8192) entries, the first
 *                         min(.., list_cap) are copied.  With option maxsim_tighten = 0 there is no starter and the final list
 *                         IS the wide list: section 2 then repeats section 0.
 *   out_wide_sd [B, list_cap]  the screen distance stored with every entry of the wide list (maxsim_tighten = 1; else untouched)
 *   out_form [8]          family (MI355DR_MS_FORM_*), column blocks (0: the generic forms), waves per workgroup, and for the
 *                         workgroup forms blocks per stage, software-pipelined, epilogue at once; the grid; 0
 *   out_info [4]          n_live, the lists' capacity (8192), 1 if the lists were produced (k <= 64 and the pass screened), the
 *                         longest starter the tightening uses (1024) */
#define MI355DR_MS_FORM_NONE 0         /* the pass was not screened: non-finite store or query, screen off, dim > 640 */
#define MI355DR_MS_FORM_GENERIC 1      /* k_maxsim16<false> */
#define MI355DR_MS_FORM_D128 2         /* k_maxsim16_d128<NCB, NW, false>: one wave per document */
#define MI355DR_MS_FORM_D128_PACKED 3  /* k_maxsim16_d128<NCB, 4, true>: the same over the granule-packed copy */
#define MI355DR_MS_FORM_WG 4           /* k_maxsim16_wg<NCB, DEFER, BPS, PIPE> */
#define MI355DR_MS_FORM_WG_PACKED 5    /* k_maxsim16_wg8 */
#define MI355DR_MS_FORM_LIST_GENERIC 6 /* k_maxsim16<true> */
#define MI355DR_MS_FORM_LIST_D128 7    /* k_maxsim16_d128<NCB, NW, false, true> */
int mi355dr_debug_maxsim_pass(mi355dr_index* idx, const float* qtok, const int32_t* q_offsets, int B, int k, const int64_t* doc_ids,
                              int64_t m, int list_cap, int* out_live, float* out_screen, float* out_two_e, int32_t* out_lists,
                              int* out_ctl, float* out_wide_sd, int* out_form, int* out_info);
/* the per-query screen bound E of the active screen dtype: exact cosine <= screen value + E  (bf16 screen: also
 * |screen value - exact cosine| <= E; int8 screen: the screen value already carries its row group's share of the bound) */
int mi355dr_debug_screen_bound(mi355dr_index* idx, const float* queries, int B, float* out_E);
/* int8 screen: per query the step S_q and the factor kq = 1.0001 + 3 e_q; per group of 32 rows [g0, g0 + n_groups) the
 * step S_g and the measured residual norm e_g.  Screen value of (query, row) = S_q S_g (q8 . c8) + e_g kq. */
int mi355dr_debug_i8_state(mi355dr_index* idx, const float* queries, int B, float* out_sq, float* out_kq, int64_t g0,
                           int64_t n_groups, float* out_step, float* out_err);
/* m(k) of the speculative pass as compiled in: the rows its predicted threshold expects above it; 0 = this k never
 * speculates.  Needs no index and no device. */
int mi355dr_debug_spec_m(int k);
/* The head of a speculative pass at k for B <= 1024 host queries, observed: prepare, the starter screen, the thr_only prune --
 * the launches a search puts in front of its one chunk, decided as a search decides them -- once without the model (the
 * rigorous threshold the sample's k-th best gives) and once with it.  MI355DR_E_UNSUPPORTED where a first attempt at k would
 * not speculate now (k outside the table, fewer than spec_min_rows rows, option speculate off, speculation suspended, no
 * screen).  Host only: it launches the search's kernels and changes none.  Like a search at k it sets the k the other hooks
 * take their screen type from; it moves no statistic (the per-query words behind "candidates" / "rescored", which its prunes
 * count in, are put back as they were) and no probation counter.  Outputs, all host:
 *   out_moments [B, 256, 2]  filled as [B, *out_slabs, 2]: per query and 64-row slab of the sample the sum and the sum of
 *                            squares of the screen's estimate (int8: without the group's share of the bound)
 *   out_thr_rigorous [B]     st.thr behind the plain starter (+inf for a query the screen cannot rank)
 *   out_thr_used [B]         the threshold the one chunk would run at: max(rigorous, model); -inf where there is no rigorous one
 *   *out_zq                  Phi^-1(1 - m(k) / size) + spec_shift_milli / 1000, before its rounding to float
 *   *out_sample_rows, *out_slabs   rows the sums run over (the divisor), slabs per query
 *   *out_i8                  1 if the int8 screen served */
int mi355dr_debug_spec_model(mi355dr_index* idx, const float* queries, int B, int k, float* out_moments, float* out_thr_rigorous,
                             float* out_thr_used, double* out_zq, int64_t* out_sample_rows, int* out_slabs, int* out_i8);
/* exact fp32 chain + distance for explicit (query,row) pairs, computed by the re-score device code */
int mi355dr_debug_rescore(mi355dr_index* idx, const float* queries, int B, const int32_t* pair_q,
                          const int64_t* pair_row, int64_t n_pairs, float* out_dot, double* out_dist);

/* ---- measurement support (bench.py; SURVEY 8(d): "re-measure with ... an MFMA microbench on the box and use the measured
 * peaks in the report") -- no reference counterpart.  A BARE stream of the MFMA instruction a screen kernel issues (format 0:
 * v_mfma_i32_32x32x32_i8 on Gaussian int8 operands like the int8 shadow's; 1: v_mfma_f32_32x32x16_bf16), operands in registers,
 * every CU busy, no memory traffic, for `seconds`; *out_tops = the settled rate in 10^12 operations per second.  Needs no
 * index; allocates and frees its own 4 MiB. */
int mi355dr_diag_mfma_stream(int device, int format, double seconds, double* out_tops);

#ifdef __cplusplus
}
#endif
#endif /* MI355DR_H */
