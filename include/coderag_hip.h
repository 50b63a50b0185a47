/*
 * coderag_hip.h -- C ABI of libcoderag_hip.so (MI355X / gfx950).
 *
 * The drop-in boundary of this repo.  The reference (iAmLakshya/code-rag, Python
 * package `lattice`) reaches its vector store through qdrant-client gRPC calls and
 * its encoder through torch/transformers; it has no FFI of its own.  These entry
 * points are what a ctypes binding for that path binds instead (INTEGRATION.md shows
 * the stub).  Each entry cites the reference interface it replaces.
 *
 * Conventions
 *  - every function returns 0 on success, <0 on error (CRH_E_*);
 *    crh_last_error() returns a thread-local message for the last failure;
 *  - no C++ types, no torch types, no exceptions across this boundary;
 *  - the caller owns every buffer it passes in; the library copies what it keeps;
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *  - a handle is used from one thread at a time (the store holds a lock; the
 *    provider uses a 1-thread executor like providers/unixcoder_provider.py:260);
 *  - "dev" pointers are device memory on the handle's device, "host" pointers are
 *    ordinary process memory; `*_on_device` flags say which one a dual-mode
 *    argument is.
 */
#ifndef CODERAG_HIP_H
#define CODERAG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRH_ABI_VERSION 4

/* status codes */
#define CRH_OK 0
#define CRH_E_INVALID (-1)  /* bad argument */
#define CRH_E_HIP (-2)      /* a HIP runtime call failed */
#define CRH_E_CAPACITY (-3) /* index full / k too large */
#define CRH_E_NODEVICE (-4) /* no usable gfx950 device */
#define CRH_E_INTERNAL (-5)

/* stored precision of the corpus */
#define CRH_DTYPE_F32 0  /* bf16 scan copy + f32 master copy; ids exact vs f32 oracle */
#define CRH_DTYPE_BF16 1 /* bf16 only; ids exact vs oracle on the bf16-rounded corpus */

#define CRH_MAX_FILTERS 8
#define CRH_MAX_K 1024

typedef struct crh_index crh_index; /* opaque */

/* One payload equality predicate: column `col` of the dictionary-coded payload must equal
 * `code`.  Replaces one models.FieldCondition(key, MatchValue(value)) of
 * embeddings/client.py:171-176; the string<->code dictionaries stay in host Python. */
typedef struct crh_filter {
    int32_t col;
    int32_t code;
} crh_filter;

/* One payload SET condition: the code of column `col` is (negate = 0) or is not (negate != 0) one of the n codes of `codes`
 * (host int32[n], any order, repeats allowed; the library copies them and keeps the set in device memory -- n is bounded by
 * memory, not by CRH_MAX_FILTERS, which bounds the number of CONDITIONS of one filter).  negate = 0 replaces
 * models.FieldCondition(key, match=MatchAny(any=[...])) -- and MatchValue for n = 1; negate != 0 replaces the same condition
 * under Filter(must_not=[...]) / MatchExcept(**{"except": [...]}).  The reference itself only ever sends MatchValue
 * (embeddings/client.py:171-176) and filters the rest on the host (query/vector_search.py:199-215).
 * An empty set has no member: "in" matches no row, "not in" every row.  A row whose code is -1 (key absent from its payload)
 * is a member of no set: it fails every "in" and passes every "not in"; negative codes in `codes` are ignored.
 *
 * `negate` is the condition's MODE.  0 = in and 1 = not in, as above; every other non-zero value but the four below keeps the
 * meaning "not in".  CRH_COND_BETWEEN (2) is a numeric RANGE over a column that stores values instead of dictionary codes (line
 * numbers: Qdrant's FieldCondition(key, range=Range(gte, lte)); the reference has no counterpart): n must be 2 and the row's value
 * v satisfies codes[0] <= v <= codes[1], both ends inclusive; codes[0] > codes[1] is an empty range.  CRH_COND_NOT_BETWEEN (3) is
 * its complement (the same Range under must_not).  A row whose value is negative (-1: absent) is inside no range: it fails every
 * BETWEEN and passes every NOT_BETWEEN whatever the bounds -- the set rule.  Mode 2 or 3 with n != 2 is CRH_E_INVALID.  A range
 * uploads nothing; every entry point that takes crh_condition (search_cond / _multi / _range, match_rows_cond, tombstone_cond)
 * takes ranges, with the mask cache and the sparse route as for sets.  sizeof(crh_condition) is 24 as before.
 *
 * CRH_COND_WORDS (4) is a ROW BITMAP somebody else computed (crh_text_match: the rows whose text holds a string): `codes` is a
 * DEVICE pointer to n u32 validity words (bit i of word t = row 32 t + i, as crh_index_row_mask writes them), cast to const
 * int32_t *; the words must be complete on the search's stream before the call and stay untouched until the search has finished;
 * n must be at least ceil(count / 32), anything less -- or a NULL pointer with rows in the index -- is CRH_E_INVALID.  `col` is no
 * column here but a caller-chosen TAG.  The row passes iff its bit is set; CRH_COND_NOT_WORDS (5) iff it is clear.  Like every mode
 * the pass is ANDed with `alive` and the other conditions, the mask is kept and the sparse route taken as for sets, also when it is
 * the only condition.  The mask cache cannot look into the buffer: two such conditions are EQUAL iff pointer, n, mode and tag are
 * all equal, so whoever rewrites a buffer must change the tag.  Taken by crh_search_cond, crh_search_range,
 * crh_index_match_rows_cond and crh_index_row_mask; crh_search_multi and crh_index_tombstone_cond answer CRH_E_INVALID. */
#define CRH_COND_IN 0
#define CRH_COND_NOT_IN 1
#define CRH_COND_BETWEEN 2
#define CRH_COND_NOT_BETWEEN 3
#define CRH_COND_WORDS 4
#define CRH_COND_NOT_WORDS 5
typedef struct crh_condition {
    int32_t col;
    int32_t negate;
    int64_t n;
    const int32_t *codes;
} crh_condition;

/* Counters of the most recent crh_search* call on a handle (diagnostics / bench). */
typedef struct crh_search_stats {
    int64_t rows;            /* rows scanned */
    int64_t tiles;           /* 32-row tiles scanned */
    int64_t seed_tiles;      /* tiles in the threshold-seeding sample */
    int64_t candidates;      /* (score,row) pairs that passed the scan threshold, all queries */
    int64_t max_query_cands; /* largest per-query candidate count */
    int32_t fallback_used;   /* bit 0: a batch was re-run with larger candidate buffers; bit 1: a grid-wide wait of the
                                one-launch scan timed out and the index went back to the three-launch form */
    int32_t batches;         /* 64-query batches processed */
} crh_search_stats;

int crh_abi_version(void);
const char *crh_last_error(void);

/* Number of HIP devices / name+arch of one ("gfx950..." expected).  */
int crh_device_count(int *count);
int crh_device_info(int device, char *name_out, int name_cap, char *arch_out, int arch_cap,
                    int64_t *hbm_bytes_out, int *cu_count_out);

/* ------------------------------------------------------------------ index ------ */

/* Create an empty HBM-resident cosine index.  Replaces
 * QdrantManager._create_collection_with_indexes (embeddings/client.py:93-113):
 * VectorParams(size=dim, distance=COSINE) + `n_code_cols` keyword payload indexes.
 * dim: 384, 768 (UniXcoder; the tuned case), 1024 or 1536 (the reference's EMBEDDING_DIMENSIONS default,
 * config/settings.py:53). */
int crh_index_create(int dim, int dtype, int64_t capacity_rows, int n_code_cols, int device,
                     crh_index **out);
int crh_index_destroy(crh_index *h);

/* Append n vectors (raw, un-normalised f32 [n, dim]; host or device).  Each is passed
 * through Qdrant's cosine_preprocess and stored; rows are numbered consecutively from
 * the current count, the first new row is returned.  codes: [n, n_code_cols] int32
 * (same memory space as vecs) or NULL when n_code_cols == 0.
 * Replaces the vector half of QdrantManager.upsert (embeddings/client.py:115-130). */
int crh_index_append(crh_index *h, int64_t n, const float *vecs, int on_device,
                     const int32_t *codes, int64_t *first_row_out, void *stream);

/* Same, for vectors that already went through cosine_preprocess (rows read back with crh_index_read_rows, and only those:
 * the scan's exactness margin assumes unit or zero rows): stored verbatim.  (Whole-index snapshots use crh_index_export /
 * crh_index_import, which move the stored image itself.) */
int crh_index_append_preprocessed(crh_index *h, int64_t n, const float *vecs, int on_device,
                                  const int32_t *codes, int64_t *first_row_out, void *stream);

/* Mark rows deleted (they stop matching; the space comes back with crh_index_compact).  rows: host int64[n].
 * Replaces the point-removal half of QdrantManager.delete (embeddings/client.py:159-169);
 * which rows a payload filter selects is resolved by the host-side payload table. */
int crh_index_tombstone(crh_index *h, int64_t n, const int64_t *rows);

/* Delete by payload filter on the device: every alive row matching ALL the (column == code) predicates stops matching;
 * n_cleared_out receives how many.  Replaces QdrantManager.delete -> client.delete(FilterSelector(filter))
 * (embeddings/client.py:159-169) without resolving the filter to row numbers on the host. */
int crh_index_tombstone_filter(crh_index *h, const crh_filter *filters, int n_filters, int64_t *n_cleared_out);

/* The same with set conditions (at least one): ONE call deletes the rows of any number of values -- what
 * ProjectCleanupService's MatchText delete (projects/cleanup.py:41-61) resolves to, and the per-file deletes of a re-index
 * (embeddings/indexer.py:61-64), which the reference issues as one client.delete per file. */
int crh_index_tombstone_cond(crh_index *h, const crh_condition *conds, int n_conds, int64_t *n_cleared_out);

/* Reclaim the rows of deleted points -- what Qdrant's optimizer does when it vacuums a segment.  The reference's indexing
 * flow deletes and re-inserts every chunk of a file on every run (embeddings/indexer.py:61-64, called with force=True from
 * pipeline/orchestrator.py:630-650), so without this the scan streams one more corpus of dead rows per re-index.
 * Device-side stable compaction of everything stored per row (the tiled bf16 image, the f32 master, the code columns): the
 * alive rows move down in their old order, so row numbers stay ascending in insertion order and ties keep "lower row first";
 * afterwards count == alive and the scan reads only live tiles.  old_to_new_host (may be NULL): int64 per OLD row, its new
 * row number or -1 for a deleted one -- what the caller's host tables (ids, payloads, side columns) are remapped with.
 * rows_after (may be NULL) receives the new row count.  Capacity is unchanged. */
int crh_index_compact(crh_index *h, int64_t *old_to_new_host, int64_t *rows_after);

/* Snapshot support -- what Qdrant's on-disk volume does for the reference (docker-compose.yml:42-43): the stored image moves
 * VERBATIM between HBM and host buffers (typically an mmap of a file) in chunks of 32-row tiles, so a restored index answers
 * with identical bits.  Per chunk of n_tiles tiles starting at first_tile:
 *   tiles   n_tiles * (dim/16) KiB  the tiled bf16 image the scan streams (ABI 3: inside a 1-KiB piece the 16-byte chunk of
 *                                   row r, half h sits at slot 2r + h; ABI 2 had h * 32 + r -- ffi.Index.load reorders such files)
 *   master  n_tiles * 32 * dim f32  the normalised f32 rows (dtype F32 only; NULL otherwise)
 *   alive   n_tiles u32             one validity word per tile (tombstones included)
 *   codes   [n_code_cols][n_tiles*32] int32, column after column (NULL when the index has no code columns)
 * export: any pointer may be NULL to skip that part.  import: appends at the end of the index (first_tile must be the first
 * unused tile; capacity must have been reserved), `rows_after` = the row count once this chunk is in (it ends inside the
 * chunk's last tile). */
int crh_index_export(crh_index *h, int64_t first_tile, int64_t n_tiles, void *tiles_host, float *master_host,
                     uint32_t *alive_host, int32_t *codes_host);
int crh_index_import(crh_index *h, int64_t first_tile, int64_t n_tiles, int64_t rows_after, const void *tiles_host,
                     const float *master_host, const uint32_t *alive_host, const int32_t *codes_host);

/* rows appended so far / rows still alive (CollectionInfo.points_count, query/engine.py:299-302). */
int crh_index_count(crh_index *h, int64_t *rows_out, int64_t *alive_out);

/* Drop every row (QdrantManager.clear_collections, embeddings/client.py:213-222). */
int crh_index_clear(crh_index *h);

/* Grow the row capacity (no-op if already that large); contents and row numbers are kept.
 * Qdrant collections grow without bound; the HBM arrays are re-allocated and copied device-side. */
int crh_index_reserve(crh_index *h, int64_t capacity_rows);

/* Copy stored (preprocessed) vectors back as f32 [n, dim] to host: rows first..first+n.
 * For dtype BF16 these are the bf16-rounded values.  Test / persistence support. */
int crh_index_read_rows(crh_index *h, int64_t first, int64_t n, float *out_host);

/* -------------------------------------------------------------- search --------- */

/* Cosine top-k of nq raw f32 queries [nq, dim] (host or device) against the alive rows
 * that satisfy every filter.  Writes scores [nq, k] f32 and rows [nq, k] int64 (host or
 * device per out_on_device), descending score, ties by lower row, padded with
 * (-inf, -1) when fewer than k rows qualify.  `row_base` is added to every returned
 * row (shard offset of a row-sharded corpus).
 * Replaces QdrantManager.search -> client.query_points (embeddings/client.py:132-157),
 * batched: the reference issues one query per RPC.
 * With host outputs the call returns after the results have landed.  With device
 * outputs it only enqueues on `stream`; call crh_search_finish() before trusting the
 * buffers (it re-runs the exact fallback if a candidate buffer overflowed). */
int crh_search(crh_index *h, int nq, const float *queries, int queries_on_device, int k,
               const crh_filter *filters, int n_filters, int64_t row_base, float *out_scores,
               int64_t *out_rows, int out_on_device, void *stream);

/* crh_search with set conditions: the alive rows that satisfy EVERY condition.  Replaces client.query_points with
 * query_filter=Filter(must=[... MatchAny ...], must_not=[...]) (embeddings/client.py:132-157 builds only the must/MatchValue
 * form), and with it the host-side exclusion of query/vector_search.py:199-215 (find_similar_code over-fetches by 5 and drops
 * the excluded file's chunks).  Everything else -- outputs, padding, row_base, device outputs and crh_search_finish -- as
 * crh_search.  n_conds: 0..CRH_MAX_FILTERS.  Bad columns, n < 0 and NULL codes with n > 0 are CRH_E_INVALID. */
int crh_search_cond(crh_index *h, int nq, const float *queries, int queries_on_device, int k,
                    const crh_condition *conds, int n_conds, int64_t row_base, float *out_scores,
                    int64_t *out_rows, int out_on_device, void *stream);

/* A batch whose queries carry DIFFERENT filters, served by shared corpus passes (the reference sends its own payload filter
 * with every query -- project_name always, language / entity_type often: query/vector_search.py:83-93 -- one query per RPC).
 * A CLASS is one distinct filter: an AND of 0..CRH_MAX_FILTERS conditions, empty = every alive row.  Class c owns
 * conds[class_off[c] .. class_off[c+1]) (class_off: host int32[n_classes + 1], ascending); query i belongs to class
 * query_class[i] (host int32[nq]).  n_classes: 1..CRH_MAX_CLASSES.  nq may be any count: it is cut into batches of 64 queries
 * (32 at dim 1536) in caller order, and each batch is ONE pass over the corpus in which every query's rows are tested
 * against its own class's mask.  Row i of the output equals, id for id and f32 score bit for bit, what crh_search_cond
 * returns for query i alone with its class's conditions.  Outputs, padding, tie order, row_base, device outputs and
 * crh_search_finish, the overflow regrowth and crh_search_stats are those of crh_search_cond; bad columns, class ids outside
 * 0..n_classes-1 and n_classes out of range are CRH_E_INVALID.
 * A mixed batch always runs the three-launch bf16 scan in its classed form, whatever crh_index_set_nomination allows: the
 * int8 pass, the one-launch scan and the wide scan have no classed variant.  (So a call whose queries all share ONE filter
 * is better served by crh_search_cond.)  With the sparse route enabled, a batch whose classes TOGETHER leave at most one tile
 * in max_fraction_den populated walks the list of the union's tiles.  The class masks are kept between calls like the mask of
 * a single filter, separately from it. */
#define CRH_MAX_CLASSES 8
int crh_search_multi(crh_index *h, int nq, const float *queries, int queries_on_device, int k,
                     const crh_condition *conds, const int32_t *class_off, int n_classes,
                     const int32_t *query_class, int64_t row_base, float *out_scores, int64_t *out_rows,
                     int out_on_device, void *stream);

/* Score threshold and exact in-range counts.  The reference puts its `limit` hits straight into an LLM prompt however bad they
 * are (query/vector_search.py:83-110); Qdrant's counterpart is query_points(..., score_threshold=...), which the reference never
 * sends -- and Qdrant has no count of the points above a score.  The definition is this repository's own and exact (DESIGN.md
 * 3.18).  With s(q, x) the score crh_search gives row x (canonical f32) and thr = thresholds_host[i], finite:
 *   IN RANGE  row x is alive, passes the conditions and s(q, x) >= thr as f32 values -- inclusive: a row whose score has
 *             exactly the threshold's bits is in;
 *   LIST      the exact top-k of the corpus cut after its last in-range entry (the first min(k, count) in-range rows):
 *             descending score, ties to the lower row, the tail padded with (-inf, -1);
 *   COUNT     out_counts[i] = the number of in-range rows, however many: not clipped at k or at CRH_MAX_K.
 * thresholds_host: host f32 [nq], copied by the call.  out_counts: int64 [nq] in the memory space of the outputs, or NULL for
 * the list alone -- then a threshold can only RAISE the scan's own nomination threshold: a high one nominates fewer rows than
 * crh_search_cond, a low one costs nothing extra.  With counts every row at or above thr - margin is listed in the candidate
 * buffers; they regrow as for any batch, and a threshold so low that one query's candidates exceed the workspace budget ends in
 * CRH_E_CAPACITY naming that query's candidate count -- never in a wrong or clipped count.
 * nq may be any count: it is cut into batches of 64 queries (32 at dim 1536) in caller order.  A range batch always runs the
 * three-launch bf16 scan (over every tile, or over the tile list of a sparse mask), whatever crh_index_set_nomination allows:
 * the int8 pass, the one-launch scan and the wide scan are not used.  Device outputs and crh_search_finish, row_base, padding,
 * tie order and crh_search_stats as for crh_search_cond (with counts no tiles are sampled: seed_tiles is 0).  A NaN or infinite
 * threshold, k outside 1..CRH_MAX_K and bad columns are CRH_E_INVALID with nothing launched.  A threshold above every score, an
 * empty index and an empty tile list give an all-padding list and count 0. */
int crh_search_range(crh_index *h, int nq, const float *queries, int queries_on_device, int k,
                     const float *thresholds_host /* [nq], copied by the call */,
                     const crh_condition *conds, int n_conds, int64_t row_base,
                     float *out_scores, int64_t *out_rows,       /* [nq, k] as crh_search_cond */
                     int64_t *out_counts /* [nq], same memory space as the outputs; NULL: list only */,
                     int out_on_device, void *stream);

/* (No counterpart in the reference: Qdrant's payload indexes make a filtered query cost about what the matching rows cost,
 * embeddings/client.py:93-113.)  A filtered search of up to 64 queries (32 at dim 1536) whose mask leaves at most one 32-row
 * tile in `max_fraction_den` populated reads only those tiles: their ascending list is made with the mask and kept with it,
 * and the three-launch bf16 scan walks the list.  Ids and score bits are those of the dense route; crh_search_stats.rows /
 * tiles / seed_tiles count what was read.  Larger calls are cut into such batches while the mask is that sparse.
 * enable: 1 / 0, negative = keep; max_fraction_den: > 0 sets it, otherwise kept (default 4: DESIGN.md section 3). */
int crh_index_set_sparse_route(crh_index *h, int enable, int max_fraction_den);

/* Completes every search enqueued with device outputs since the last finish (crh_search, _cond, _multi, _range): waits for
 * the streams those calls were enqueued on -- every one of them, whichever `stream` is passed here; the index remembers them
 * -- reads each batch's status, and runs again, on the batch's own stream, every batch whose candidate buffers overflowed or
 * whose one-launch scan timed out.  The outputs are final when the call returns.
 * What the caller owes a pending search UNTIL then: its queries, its outputs, the out_counts buffer of a range search and the
 * bitmap of a CRH_COND_WORDS condition stay allocated and untouched -- a batch that is run again reads and writes them again.
 * Calls on several streams may be pending at once; a call on another stream than the pending call before it is put behind
 * that one on the device (they share the index's workspace).
 * The index itself may be changed while searches are pending: crh_index_append / _append_preprocessed, the three tombstone
 * calls, crh_index_import, crh_index_reserve and crh_index_clear complete the pending searches FIRST -- as crh_search_finish
 * does, at its cost: one wait for their streams -- so every search answers for the index as it was at its call, also when
 * it had to run again.  With nothing pending that costs nothing.  crh_index_compact alone refuses (CRH_E_INVALID) while
 * searches are pending: finish them first.  At most 1024 batches stay pending: the call that would enqueue one more completes
 * them itself.  Batches completed that way, or by a mutation, stay in crh_search_stats until the caller's own finish. */
int crh_search_finish(crh_index *h, void *stream);

int crh_search_get_stats(crh_index *h, crh_search_stats *out);

/* HIP-event timing of the dominant kernel (the corpus scan; behind the int8 copy: the pass, the third of that scan's three
 * launches), recorded on the search stream around each launch while enabled; totals since the last enable.  enable = 2: behind
 * the int8 copy the two events bracket all three launches of the scan (sample tiles, thresholds, pass) -- the span one launch
 * covered in rounds 3-4.  Measurement support for bench.py. */
int crh_index_set_profiling(crh_index *h, int enable);
int crh_index_get_profile(crh_index *h, double *scan_ms_total, int64_t *scan_launches);

/* Tuning knobs (0 / negative = keep default): seed sample tiles, per-wave candidate
 * capacity, per-query candidate capacity, force_fallback (testing): 1 = start from tiny candidate buffers so the
 * regrow-and-rerun path runs (behind the int8 scan: its one regrowth), 3 = the same with that regrowth refused (its batches go to
 * the bf16 scan: the strike path), 2 = make the one-launch bf16 scan's grid-wide wait time out so its recovery path runs, 0 = off. */
int crh_index_set_tuning(crh_index *h, int seed_tiles, int wave_cand_cap, int query_cand_cap,
                         int force_fallback);

/* (No counterpart in the reference: it leaves the search strategy to the Qdrant server, embeddings/client.py:96-102,132-157.)
 * How a batch of up to 64 queries is NOMINATED (every returned id and score is decided by the canonical f32 arithmetic on the
 * stored rows whatever the mode; results are bit-identical across modes):
 *   CRH_NOMINATE_BF16_3  seed scan, threshold, main scan over the bf16 tiles as three launches
 *   CRH_NOMINATE_BF16    the same in one launch (grid-wide waits; needs the whole grid resident)
 *   CRH_NOMINATE_INT8    sample tiles, thresholds and the pass over the int8 copy of the rows, three launches, no grid-wide
 *                        wait (half the bytes of the pass; +1 byte per element and 4 per row of device memory, and for a bf16
 *                        store +2 bytes per element for the row-major rows its selection step reads -- all derived from the
 *                        stored rows, never part of a snapshot) -- the default at every supported dim, from 1M rows up, for
 *                        k <= 256.
 * set: the most advanced mode the index may use.  It still falls back by itself: no memory for the copy; a grid-wide wait of
 * the one-launch bf16 scan that timed out (the wait is bounded by eight times the pass's own time, at least 2 ms; the batch is
 * run again in the three-launch form and the index stays off the one-launch form for 0.2 s, doubling with every further time-out
 * up to 5 s -- the int8 nomination, which waits for nobody, stays in use); int8 candidate buffers that
 * overflowed (they grow ONCE to the observed need when that is at most 2 % of the rows per query; otherwise the batch goes to the
 * bf16 scan, and three such batches in a row rest the copy for 4096 batches, then one more try).  get: the mode the next batch
 * would use. */
#define CRH_NOMINATE_BF16_3 0
#define CRH_NOMINATE_BF16 1
#define CRH_NOMINATE_INT8 2
int crh_index_set_nomination(crh_index *h, int mode);
int crh_index_get_nomination(crh_index *h, int *mode_out);


/* Merge nlists sorted per-shard lists ([nlists, nq, k] device f32 / int64, padded with
 * (-inf,-1)) into [nq, k]: the step after the all-gather of a row-sharded search
 * (does not exist in the reference). */
int crh_merge_topk(int nlists, int nq, int k, const float *scores_dev, const int64_t *rows_dev,
                   float *out_scores_dev, int64_t *out_rows_dev, void *stream);
/* Same, with list l at scores_dev + l * score_list_stride and rows_dev + l * row_list_stride (elements, each >= nq * k): lets
 * every rank send ONE [scores | rows] record through ONE all-gather and merge straight out of the gathered buffer. */
int crh_merge_topk_strided(int nlists, int nq, int k, const float *scores_dev, const int64_t *rows_dev,
                           int64_t score_list_stride, int64_t row_list_stride, float *out_scores_dev,
                           int64_t *out_rows_dev, void *stream);

/* ---- hybrid re-rank of the vector branch (BASELINE config 5; replaces, for vector-only candidate lists, the per-query
 * host loop of HybridRanker.rank_results, src/lattice/query/ranking/ranker.py:24-54 + scorer.py:80-126 + ranker.py:171-229).
 * Scores are computed in f64 with the reference's operand order: bit-identical to the Python result. */
#define CRH_RR_NAME_BYTES 64    /* bytes of the lower-cased entity name kept per row */
#define CRH_RR_MAX_ENTITIES 8   /* query entities per query handled on the device */
#define CRH_RR_ENTITY_BYTES 48

/* What score_vector_result reads of one query (scorer.py:80-126): RankingConfig.weights_for(plan.primary_intent) and the
 * lower-cased names of plan.entities.  n_entities outside 0..CRH_RR_MAX_ENTITIES sends the query back to the host. */
typedef struct crh_rerank_query {
    double vector_weight;
    double centrality_weight;
    int32_t n_entities;
    int32_t entity_len[CRH_RR_MAX_ENTITIES];
    uint8_t entity[CRH_RR_MAX_ENTITIES][CRH_RR_ENTITY_BYTES];
    int32_t pad_;
} crh_rerank_query;

/* Per-candidate side data, device arrays of nq*k entries in candidate order (crh_gather_rows_* fills them from per-row
 * columns): len(content) in characters (0 = empty); total_degree of the row's graph node (-1 = the graph has no answer);
 * dictionary codes of file_path, of the merge key "file:entity_name:start_line" (models.py:55-56) and of the centrality
 * key (graph_node_id or entity_name, scorer.py:48-54); the lower-cased UTF-8 entity name, zero padded to
 * CRH_RR_NAME_BYTES, with its true byte length (a longer name sends its query back to the host). */
typedef struct crh_rerank_columns {
    const int32_t *content_len;
    const int32_t *degree;
    const int32_t *file_code;
    const int32_t *key_code;
    const int32_t *node_code;
    const int32_t *name_len;
    const uint8_t *name;
} crh_rerank_columns;

/* out[i] = col[rows[i] - row_base] for rows owned by this shard (row_base <= row < row_base + n_local), `fill` (bytes: 0)
 * otherwise -- so that the columns of a merged multi-shard candidate list are the sum over the shards' gathers. */
int crh_gather_rows_i32(int64_t n, const int64_t *rows_dev, int64_t row_base, int64_t n_local, const int32_t *col_dev, int32_t fill,
                        int32_t *out_dev, void *stream);
int crh_gather_rows_bytes(int64_t n, const int64_t *rows_dev, int64_t row_base, int64_t n_local, const uint8_t *col_dev, int width,
                          uint8_t *out_dev, void *stream);
/* The seven of them in ONE launch: `cols` holds this shard's PER-ROW columns (device pointers; `name` 4-byte aligned), the output
 * is one int32 buffer -- the six integer columns in the order of the struct, n entries each, then n x CRH_RR_NAME_BYTES name
 * bytes -- i.e. the per-candidate arrays crh_rerank_vector takes are views of it, and a row-sharded caller completes the
 * table of a merged candidate list with one all-reduce(sum) over it (rows of other shards give zeros). */
int crh_gather_rerank_columns(int64_t n, const int64_t *rows_dev, int64_t row_base, int64_t n_local, const crh_rerank_columns *cols,
                              int32_t *out_packed_dev, void *stream);

/* Re-rank nq candidate lists of k vector hits (scores/rows as crh_search or crh_merge_topk return them; rows < 0 = padding).
 * The centrality table of a query holds the first `centrality_top` named hits, as QueryEngine._get_centrality_scores builds
 * it for a query without graph results (query/engine.py:348-377).  Outputs, per query, in final order: index into the
 * candidate list, final score, the four signals (vector_similarity, query_entity_match, centrality, code_quality), flag
 * bit 0 = "hybrid" (entries sharing a merge key were fused); out_count[q] = survivors (<= max_total), or -1 when the host
 * must rank this query (too many entities, a truncated name); the slots behind a query's survivors are written as (-1, 0, ...):
 * the outputs need no clearing before a call.  `queries_dev` is a device copy of nq crh_rerank_query. */
int crh_rerank_vector(int nq, int k, const float *scores_dev, const int64_t *rows_dev, const crh_rerank_columns *cols,
                      const crh_rerank_query *queries_dev, double entity_match_bonus, int max_per_file, int max_total,
                      int centrality_top, int32_t *out_index_dev, double *out_score_dev, double *out_signals_dev,
                      int32_t *out_count_dev, int32_t *out_flags_dev, void *stream);

/* ---- diversity-aware top-k (maximal marginal relevance) on the device.  No counterpart in the reference: it only sends
 * query_points(query, limit, filter) (embeddings/client.py:142-148).  What it stands in for is Qdrant's Mmr(diversity,
 * candidates_limit) query and the max_marginal_relevance_search of the RAG frameworks' Qdrant adaptors -- known by description
 * only, not checkable offline: the arithmetic and the tie rule below are this repository's own definition. */

/* out[i, :] = the stored row rows[i] - row_base as f32 [n, dim] when this index owns it (row_base <= rows[i] < row_base +
 * count), zeros otherwise (padding -1 included): the vector counterpart of crh_gather_rows_*, so the vectors of a merged
 * multi-shard candidate list are the sum over the shards' gathers.  The values are those of crh_index_read_rows (the f32 master
 * of an F32 store; the bf16-rounded values of a BF16 store, read from the row-major side copy while the int8 nomination copy
 * is live, from the tiled image otherwise).  Tombstoned rows still gather (a candidate list never names one).  Enqueues only;
 * `stream` is the stream of the searches that made the list (the side copy is brought up to date on it). */
int crh_index_gather_vectors(crh_index *h, int64_t n, const int64_t *rows_dev, int64_t row_base, float *out_dev, void *stream);

/* Greedy MMR over nq candidate lists of c entries (scores f32 descending / rows int64 as crh_search or crh_merge_topk return
 * them, rows < 0 = padding, at the end) with the candidates' stored vectors vecs_dev f32 [nq, c, dim] (16-byte aligned).  With
 * rel[i] the candidate's score and sim(i, s) the CANONICAL dot of two candidate rows (acc = acc + x_i[e] * x_s[e], e ascending,
 * product and sum rounded separately in f32): pick 1 is position 0; pick t > 1 is, among the real candidates not yet picked,
 * the largest  obj = (1 - diversity) * rel[i] - diversity * max over picked s of sim(i, s)  -- lam = 1 - diversity, lam * rel,
 * diversity * max and the difference each rounded to f32, no fused multiply-add; ties go to the lower position.  Padding is
 * never picked (a list whose position 0 is padding is empty).  Per pick: out_pos (int32 position in the list), out_rows, out_scores
 * (rel: the hit's score stays its cosine to the query) and out_obj (obj at the moment of the pick; lam * rel for pick 1), each
 * [nq, k]; with fewer than k real candidates the tail is (-1, -1, -inf, -inf).  diversity = 0 returns the first k candidates
 * unchanged; the first j picks of a k-pick call are the j-pick call.  1 <= k <= c <= CRH_MAX_K, nq >= 0, dim 384 / 768 / 1024 /
 * 1536; diversity outside [0, 1] or NaN is CRH_E_INVALID.  Needs no index handle (launches on the current device, like
 * crh_rerank_vector).  Enqueues only; writes every output slot, so the outputs need no clearing. */
int crh_mmr_select(int nq, int c, int k, int dim, const float *scores_dev, const int64_t *rows_dev, const float *vecs_dev,
                   float diversity, int32_t *out_pos_dev, int64_t *out_rows_dev, float *out_scores_dev, float *out_obj_dev,
                   void *stream);

/* ---- exact per-group cap on the device (group_by / group_size).  The reference caps results per file AFTER the fetch
 * (ResultReranker.deduplicate(max_per_file=3), query/reranker.py:122-145; RankingConfig.max_per_file) and is left short when one
 * file owns the list; Qdrant's query_points_groups(group_by, limit, group_size) is "best effort".  The definition here is this
 * repository's own and exact: a candidate's GROUP is its code in one column, its RANK IN ITS GROUP the number
 * of earlier candidates of the list with the same code; a candidate is kept iff that rank is < group_size.  A negative code
 * (-1: the key is absent) belongs to no group and is always kept. */

/* out[i] = the code of column `col` of row rows[i] - row_base when this index owns that row (row_base <= rows[i] < row_base +
 * count); every other position (padding -1, other shards' rows) is left UNTOUCHED: the caller pre-fills the buffer with -1, the
 * shards of one process write into the same buffer, and across processes one all-reduce(MAX) completes it (stored codes are
 * >= -1).  Tombstoned rows still gather.  col outside 0..n_code_cols-1 is CRH_E_INVALID.  Enqueues only. */
int crh_index_gather_codes(crh_index *h, int col, int64_t n, const int64_t *rows_dev, int64_t row_base, int32_t *out_codes_dev,
                           void *stream);

/* Capped walk over nq candidate lists of c entries (scores f32 / rows int64 as crh_search or crh_merge_topk* return them, rows
 * < 0 = padding; codes int32 [nq, c] as crh_index_gather_codes completes them).  The kept candidates (real, and code < 0 or rank
 * in group < group_size; padding neither counts nor is kept) are written in list order, the first k of them: out_pos (int32
 * position in the list), out_rows, out_scores (the score's bits, unchanged), out_codes, each [nq, k]; the tail is (-1, -1, -inf,
 * -1).  out_info int32 [nq, 2] = (kept: kept candidates of the WHOLE list, not clipped at k; real: non-padding candidates).
 * group_size >= c returns the first k candidates unchanged; the first j outputs of a k-output call are the j-output call.
 * 1 <= k <= c <= CRH_MAX_K, group_size >= 1, nq >= 0, anything else CRH_E_INVALID.  Needs no index handle (launches on the
 * current device, like crh_mmr_select).  Deterministic; enqueues only; writes every output slot. */
int crh_group_select(int nq, int c, int k, int group_size, const float *scores_dev, const int64_t *rows_dev,
                     const int32_t *codes_dev, int32_t *out_pos_dev, int64_t *out_rows_dev, float *out_scores_dev,
                     int32_t *out_codes_dev, int32_t *out_info_dev, void *stream);

/* ---- overlap-free hit lists on the device (max_overlap).  The reference's chunker emits an entity for a class and one for each
 * of its methods and splits long entities into parts that share trailing lines (embeddings/indexer.py:85-133), so a good query
 * returns the same lines two or three times; the reference has no answer and Qdrant no counterpart.  The definition is this
 * repository's own and exact.
 *
 * nq candidate lists of c entries (scores f32 / rows int64 as crh_search or crh_merge_topk* return them, rows < 0 = padding, at
 * the end) with, per candidate, file_codes / lo / hi int32 [nq, c] as crh_index_gather_codes completes them over buffers
 * pre-filled with -1: the code of its file, its first and its last line.  A real candidate HAS A SPAN iff file_code >= 0, lo >= 0
 * and hi >= lo; its length is hi - lo + 1.  The walk, in list order: padding is skipped; a candidate without a span is kept; a
 * candidate i with a span is REDUNDANT iff some earlier KEPT candidate j with a span and the same file code has
 *   ov = min(hi_i, hi_j) - max(lo_i, lo_j) + 1 > 0   and   (int64)ov * 1000 > (int64)max_overlap_permille * min(len_i, len_j);
 * otherwise it is kept.  Integer arithmetic only, nothing rounded.  The first k kept candidates are written in list order, each
 * [nq, k]: out_pos (int32 position in the list), out_rows, out_scores (the score's bits, unchanged), out_file, out_lo, out_hi
 * (the candidate's three values as given); the tail is (-1, -1, -inf, -1, -1, -1).  out_info int32 [nq, 2] = (kept: kept
 * candidates of the WHOLE list, not clipped at k; real: non-padding candidates).  max_overlap_permille = 1000 returns the first k
 * candidates unchanged, 0 drops on any shared line; the first j outputs of a k-output call are the j-output call.
 * 1 <= k <= c <= CRH_MAX_K, nq >= 0, 0 <= max_overlap_permille <= 1000, anything else CRH_E_INVALID with nothing launched.  Needs
 * no index handle (launches on the current device, like crh_group_select).  Deterministic; enqueues only; writes every output
 * slot. */
int crh_span_select(int nq, int c, int k, int max_overlap_permille, const float *scores_dev, const int64_t *rows_dev,
                    const int32_t *file_codes_dev, const int32_t *lo_dev, const int32_t *hi_dev, /* each [nq, c] */
                    int32_t *out_pos_dev, int64_t *out_rows_dev, float *out_scores_dev, int32_t *out_file_dev, int32_t *out_lo_dev,
                    int32_t *out_hi_dev, /* each [nq, k] */ int32_t *out_info_dev /* [nq, 2] */, void *stream);

/* ---- multi-query fusion on the device (reciprocal-rank fusion / best match).  The reference's planner writes reformulations of
 * a question (QueryPlan.sub_queries[].query_text, query/query_planner.py:66-91) and its engine searches the original text only
 * (query/engine.py:315-346); Qdrant's counterpart is query_points(prefetch=[...], query=FusionQuery(RRF)).  The definition here
 * is this repository's own.
 *
 * Per logical query: m lists of c entries (scores f32 descending / rows int64 as crh_search or crh_merge_topk* return them, rows
 * < 0 = padding, at the end of each list), [nq, m, c]; entry (j, p) has flat index u = j * c + p; padding takes no part.
 *   contribution of (j, p):  RRF  w_j / (float)(rrf_k + p + 1) -- one f32 division, correctly rounded; weights_host[j] or 1
 *                            MAX  the entry's score
 *   fused score of a row:    RRF  +0.0f plus the contributions of its entries in ascending u, every addition rounded to f32
 *                            MAX  its largest contribution
 *   cos = its largest score, lists = bit j set when list j holds it, first = its smallest u.
 * "Largest" and the output order compare the order-preserving integer image of f32 (-0.0 < +0.0).  Outputs, each [nq, k]: the
 * first k distinct rows by descending fused score, ties to the lower row -- out_rows, out_fused, out_cos, out_lists, out_first;
 * the tail is (-1, -inf, -inf, 0, -1).  out_info int32 [nq, 2] = (distinct rows of the m lists, real entries).  The first j
 * outputs of a k-output call are the j-output call; m = 1 returns the list itself; MAX with c >= k is the exact top-k of the
 * corpus under max_j cos(q_j, x) when every list is an exact top-c.
 * 1 <= m <= CRH_MAX_LISTS, c >= 1, m * c <= CRH_MAX_K, 1 <= k <= m * c, nq >= 0, rrf_k >= 0, weights finite and >= 0 (NULL: all
 * 1; non-NULL with MAX is refused), anything else CRH_E_INVALID with nothing launched.  Needs no index handle (launches on the
 * current device, like crh_group_select).  Deterministic; enqueues only; writes every output slot. */
#define CRH_FUSE_RRF 0
#define CRH_FUSE_MAX 1
#define CRH_MAX_LISTS 16
int crh_fuse_select(int nq, int m, int c, int k, int method, int rrf_k, const float *weights_host /* [m] or NULL */,
                    const float *scores_dev, const int64_t *rows_dev,            /* [nq, m, c] */
                    int64_t *out_rows_dev, float *out_fused_dev, float *out_cos_dev, int32_t *out_lists_dev,
                    int32_t *out_first_dev, /* each [nq, k] */ int32_t *out_info_dev /* [nq, 2] */, void *stream);

/* ---- recommend by example on the device ("more like these, not like those").  The reference's planner has a find_similar
 * intent and can only embed a snippet for it; Qdrant's counterpart is RecommendQuery(positive, negative, strategy), known by
 * description only.  The definitions here are this repository's own.
 *
 * A logical query is P positive and N negative EXAMPLES, each a stored row as crh_index_gather_vectors returns it.  Its slots
 * are [P positives | N negatives]; n_pos_host / n_neg_host (int32 [nq], host, copied by the call; NULL: every slot is live) give
 * ragged sets: the first n_pos positives and the first n_neg negatives of a query are live, 1 <= n_pos <= P, 0 <= n_neg <= N. */
#define CRH_MAX_POS 8
#define CRH_MAX_NEG 8
#define CRH_RECOMMEND_AVERAGE 0
#define CRH_RECOMMEND_BEST 1

/* The "average" query: out[q, i] = (ap + ap) - an with ap = sp / (float)n_pos, an = sn / (float)n_neg, sp / sn = +0.0f plus the
 * live positives' / negatives' elements in ascending slot order; with n_neg = 0, out[q, i] = ap.  Every operation is rounded to
 * f32 separately (no fused multiply-add).  examples_dev f32 [nq, P + N, dim], out_queries_dev f32 [nq, dim].  nq >= 0, 1 <= P <=
 * CRH_MAX_POS, 0 <= N <= CRH_MAX_NEG, dim 384 / 768 / 1024 / 1536, counts in range; anything else CRH_E_INVALID with nothing
 * launched.  Needs no index handle; deterministic; enqueues only. */
int crh_recommend_query(int nq, int P, int N, int dim, const float *examples_dev, const int32_t *n_pos_host,
                        const int32_t *n_neg_host, float *out_queries_dev, void *stream);

/* The selection.  Method BEST: scores_dev f32 / rows_dev int64 [nq, P, c] are the exact top-c lists of the P positives (rows < 0
 * = padding, at the end of a list; the lists of slots that are not live must be all padding), cand_vecs_dev f32 [nq, P * c, dim]
 * the candidates' stored vectors, examples_dev f32 [nq, P + N, dim] the RAW examples (both 16-byte aligned), example_rows_dev
 * int64 [nq, P + N] their rows (-1: unused slot).  s(e, x) is the score crh_search gives row x for the raw query e: Qdrant's
 * cosine_preprocess of e in sequential f32 arithmetic (then rounded to bf16 when round_bf16 = 1: the store's dtype is BF16),
 * then the canonical dot (acc = acc + e[i] * x[i], i ascending, product and sum rounded separately).  Per distinct row (its
 * first flat entry stands for it): p = max over the live positives of s, best = the lowest slot that attains it, n = max over
 * the live negatives (-inf without one).  A row is KEPT iff it is no example row and ord(p) > ord(n) on the order-preserving
 * integer image of f32 (-0.0 < +0.0).  Outputs, each [nq, k]: the first k kept rows by descending p, ties to the lower row --
 * out_rows, out_score (p), out_neg (n), out_best (int32); the tail is (-1, -inf, -inf, -1).  out_info int32 [nq, 4] = (kept,
 * settled, distinct real candidates, vetoed = distinct - kept), none clipped at k.  SETTLED: with T the largest last score over
 * the lists whose c entries are all real, the kept rows with ord(p) > ord(T) -- every row of the corpus with p > T is in some
 * list, so they are a prefix of the exact answer; without a full list every kept row is settled.
 * Method AVERAGE: ONE list per query, [nq, 1, c] (the search for crh_recommend_query's vector); it only removes the example rows:
 * out_score is the list's score, out_neg -inf, out_best -1, every kept row settled; cand_vecs_dev / examples_dev are not read.
 * The first j outputs of a k-output call are the j-output call.  With `lists` = P (BEST) or 1 (AVERAGE): c >= 1, lists * c <=
 * CRH_MAX_K, 1 <= k <= lists * c, P / N / dim / counts as above, round_bf16 0 or 1; anything else CRH_E_INVALID with nothing
 * launched.  Needs no index handle (launches on the current device, like crh_fuse_select).  Deterministic; enqueues only;
 * writes every output slot. */
int crh_recommend_select(int nq, int P, int N, int c, int k, int dim, int method, int round_bf16, const float *scores_dev,
                         const int64_t *rows_dev, const float *cand_vecs_dev, const float *examples_dev,
                         const int64_t *example_rows_dev, const int32_t *n_pos_host, const int32_t *n_neg_host,
                         int64_t *out_rows_dev, float *out_score_dev, float *out_neg_dev, int32_t *out_best_dev, /* each [nq, k] */
                         int32_t *out_info_dev /* [nq, 4] */, void *stream);

/* Filter-only fetch: first `limit` alive rows (ascending) matching the filters, host int64 out;
 * n_out receives how many (rows_out_host may be NULL to count only).  Replaces QdrantManager.search(query_vector=None, ...) as used by
 * query/context/builder.py:111-119 and the scroll of embeddings/client.py:178-202. */
int crh_index_match_rows(crh_index *h, const crh_filter *filters, int n_filters, int64_t limit,
                         int64_t *rows_out_host, int64_t *n_out);

/* The same with set conditions (n_conds 0..CRH_MAX_FILTERS): the scroll of embeddings/client.py:178-202 and
 * client.count(count_filter=Filter(...MatchText...)) of projects/cleanup.py:41-61, any number of values in one call. */
int crh_index_match_rows_cond(crh_index *h, const crh_condition *conds, int n_conds, int64_t limit,
                              int64_t *rows_out_host, int64_t *n_out);

/* ---- facets: exact per-value counts of one dictionary column, under any filter or score threshold.  Qdrant's counterpart is
 * client.facet(collection_name, key, facet_filter, limit, exact); the reference's callers fetch hits and count them in Python.
 * The definitions are this repository's own and exact.  A row COUNTS iff it is alive and passes the conditions
 * -- and, in the semantic form, is IN RANGE as crh_search_range defines it (canonical f32 score >= thr, inclusive).  With c the
 * code of a counting row in column `col`: bins[c] += 1 for 0 <= c < n_bins, missing += 1 for c < 0 (-1: the key is absent),
 * out_of_range += 1 for c >= n_bins (written nowhere).  info = (counted, missing, out_of_range), counted = sum(bins) + missing +
 * out_of_range = what crh_index_match_rows_cond / crh_search_range count for the same arguments.  All sums are integer atomics:
 * integer additions commute, so the result is deterministic -- the same on every call and on a batch that is run again. */
#define CRH_FACET_LDS_BINS 8192 /* up to this many bins a workgroup counts in LDS; above, waves aggregate runs of equal codes */

/* Replaces client.facet(key, facet_filter, exact=True) before its ordering.  The mask is built (or found) by the same routine
 * and mask cache crh_index_row_mask and a search use; every condition mode of crh_index_match_rows_cond is taken, row bitmaps
 * (CRH_COND_WORDS / _NOT_WORDS) included.  A tile whose mask word is 0 does not have its codes read.  n_bins chooses the
 * kernel's route and nothing else: both give the same bins.  out_bins_dev int64 [n_bins], out_info_dev int64
 * [3], device memory; every slot is overwritten (an empty index writes zeros).  col outside 0..n_code_cols-1 and n_bins < 1 are
 * CRH_E_INVALID with nothing launched; the index does not know which of its columns hold dictionary codes and which values
 * (CRH_COND_BETWEEN): a histogram of a numeric column is refused by the store.  Enqueues on `stream`. */
int crh_index_facet(crh_index *h, int col, const crh_condition *conds, int n_conds, int n_bins,
                    int64_t *out_bins_dev /* [n_bins] */, int64_t *out_info_dev /* [3]: counted, missing, out_of_range */,
                    void *stream);

/* The semantic form -- client.facet under a filter Qdrant cannot express: "at cosine >= thr to this query".  A range batch with
 * counts (crh_search_range: thresholds, batches of 64 / 32 queries, the three-launch bf16 scan, CRH_E_CAPACITY for a threshold
 * so low that a query's candidates exceed the workspace budget) whose counting kernel adds every in-range row to its query's
 * bins, lanes with equal codes aggregated per wave.  out_bins_dev int64 [nq, n_bins], out_info_dev int64 [nq, 3], device
 * memory, overwritten: there is no accumulate mode -- the shards of one process each get a slab of their own and the caller
 * sums them.  A batch's bins and info rows are cleared on the stream before its scan, so a batch that is run again because its
 * candidate lists overflowed gives what a first run gives.  The batches are finished before the call returns (no
 * crh_search_finish is needed); info[i][0] is crh_search_range's out_counts[i].  A NaN or infinite threshold, a bad column and
 * n_bins < 1 are CRH_E_INVALID with nothing launched. */
int crh_search_range_facet(crh_index *h, int nq, const float *queries, int queries_on_device,
                           const float *thresholds_host /* [nq], copied by the call */,
                           const crh_condition *conds, int n_conds, int col, int n_bins,
                           int64_t *out_bins_dev /* [nq, n_bins] */, int64_t *out_info_dev /* [nq, 3] */, void *stream);

/* The FACET LIST of nq histograms (int64 [nq, n_bins], counts >= 0 -- the bins above, summed over shards and ranks by the
 * caller): the bins with count > 0 ordered by count descending, ties to the LOWER CODE -- the value stored first; Qdrant's
 * client.facet breaks ties by the value itself -- cut at k.  out_codes_dev int32 / out_counts_dev int64, each [nq, k], the tail
 * (-1, 0): a zero count is never returned.  out_info_dev int64 [nq, 2] = (bins with count > 0, sum of the bins).  The first j
 * entries of a k-entry list are the j-entry list.  Exact for any non-negative int64 counts (radix select of the k-th largest,
 * ordered compaction, sort of the survivors).  1 <= k <= CRH_MAX_K, n_bins >= 1, nq >= 0, anything else CRH_E_INVALID with
 * nothing launched.  Needs no index handle (launches on the current device, like crh_group_select).  Deterministic; enqueues
 * only; writes every output slot. */
int crh_facet_select(int nq, int n_bins, int k, const int64_t *bins_dev /* [nq, n_bins] */,
                     int32_t *out_codes_dev /* [nq, k] */, int64_t *out_counts_dev /* [nq, k] */,
                     int64_t *out_info_dev /* [nq, 2] */, void *stream);

/* ---- exact BM25 keyword search on the device.  Qdrant's counterpart is a sparse (BM25) vector searched beside the dense one,
 * query_points(prefetch=[dense, sparse], query=FusionQuery(RRF)); the fusion half is crh_fuse_select.  The definitions are this
 * repository's own and exact.
 *
 * The validity words a search of `h` under these conditions uses -- alive AND filter, one u32 per 32-row tile, bit i = row
 * 32 t + i -- copied to out_mask_dev (n_words >= ceil(rows / 32), anything less is CRH_E_INVALID; words behind the last tile are
 * not written).  n_conds = 0 gives the alive words.  Built (or found) by the same routine and mask cache a search uses;
 * enqueues on `stream`.  This is how tombstones and filters reach a crh_lex. */
int crh_index_row_mask(crh_index *h, const crh_condition *conds, int n_conds, uint32_t *out_mask_dev, int64_t n_words, void *stream);

/* A crh_lex is a FORWARD index whose rows are numbered like the rows of the crh_index it accompanies: per row its distinct term
 * ids (u32, strictly ascending) with their frequencies tf (u8, 1..255, saturated) and its length dl (int32, the number of terms
 * before de-duplication) -- CSR: row_off int64 [rows + 1], 5 bytes per entry.  What a term is, is the caller's business (the
 * store hashes sub-words of identifiers).  Buffers grow by doubling on append; a search releases nothing. */
typedef struct crh_lex crh_lex; /* opaque */
#define CRH_LEX_MAX_QUERY_TERMS 32

int crh_lex_create(int device, int64_t capacity_rows, crh_lex **out);
int crh_lex_destroy(crh_lex *l);
int crh_lex_clear(crh_lex *l); /* forget every row, keep the buffers */
int crh_lex_count(crh_lex *l, int64_t *rows_out, int64_t *entries_out);

/* n rows behind the existing ones, all host pointers: row_off [n + 1] starting at 0, terms / tf one per entry, dl one per row.
 * CRH_E_INVALID, with nothing stored, when offsets do not start at 0 or decrease, a row's ids are not strictly ascending, a tf is
 * 0, or a dl is smaller than the sum of the row's tf.  A row without entries is allowed.  Synchronous. */
int crh_lex_append(crh_lex *l, int64_t n, const int64_t *row_off_host, const uint32_t *terms_host, const uint8_t *tf_host,
                   const int32_t *dl_host);

/* Over the rows whose bit is set in mask_dev (words as crh_index_row_mask writes them, complete before the call; NULL: every
 * row): df_out_host[i] = the number of such rows holding terms_host[i] (nt >= 0 terms, repeats allowed), *rows_out their number,
 * *sum_dl_out the sum of their dl.  Integers only.  Synchronous (runs on the default stream). */
int crh_lex_stats(crh_lex *l, const uint32_t *mask_dev, int64_t nt, const uint32_t *terms_host, int64_t *df_out_host,
                  int64_t *rows_out, int64_t *sum_dl_out);

/* BM25, exact.  Query q's terms are q_terms_host[q_off_host[q] .. q_off_host[q + 1]) -- at most CRH_LEX_MAX_QUERY_TERMS ids,
 * strictly ascending -- with q_idf_host beside them.  With c = (float)tf and len = (float)dl, every operation rounded to f32 on
 * its own (no fused multiply-add, divisions correctly rounded):
 *     norm    = k1 * ((1.0f - b) + b * (len / avgdl))
 *     contrib = idf_t * ((c * (k1 + 1.0f)) / (c + norm))
 *     score   = +0.0f, then + contrib for each of the query's terms the row holds, in ASCENDING term id.
 * idf and avgdl are inputs: the host derives them from crh_lex_stats, so device and host never disagree about a logarithm.  A
 * row QUALIFIES for a query iff its mask bit is set (mask_dev NULL: every row) and it holds at least one of the query's terms.
 * Outputs [nq, k]: the qualifying rows by descending score (order-preserving integer image of f32), ties to the lower row,
 * row_base added; the tail is (-inf, -1); every slot is written.  out_count_dev int64 [nq] = the number of qualifying rows,
 * exact, never clipped at k.  A query without terms returns an empty list and 0.
 * 1 <= k <= CRH_MAX_K, nq >= 0 (run in passes of 64 queries), avgdl finite and > 0; more than CRH_LEX_MAX_QUERY_TERMS terms or
 * ids that do not ascend are CRH_E_INVALID with nothing launched.  Deterministic; waits on `stream` (the candidate lists are sized
 * to what a first pass over the index counted). */
int crh_lex_search(crh_lex *l, int nq, const int64_t *q_off_host, const uint32_t *q_terms_host, const float *q_idf_host, float k1,
                   float b, float avgdl, int k, const uint32_t *mask_dev, int64_t row_base, float *out_scores_dev,
                   int64_t *out_rows_dev, int64_t *out_count_dev, void *stream);

/* ---- literal substring match on the device.  Qdrant's counterpart is FieldCondition(key, match=MatchText(text)) on a field
 * without a full-text index: an exact substring match.  The definitions are this repository's own and exact.
 *
 * A crh_text is an ARENA whose rows are numbered like the rows of the crh_index it accompanies: row_off int64 [rows + 1] and the
 * rows' bytes one behind the other, both in device memory.  What the bytes are is the caller's business (the store keeps the
 * UTF-8 of a chunk's content).  Buffers grow by doubling on append; a match releases nothing. */
typedef struct crh_text crh_text; /* opaque */
#define CRH_TEXT_MAX_PATTERNS 8
#define CRH_TEXT_MAX_PATTERN_BYTES 64
#define CRH_TEXT_ALL 0 /* a row matches iff it holds every pattern */
#define CRH_TEXT_ANY 1 /* ... at least one pattern */

int crh_text_create(int device, int64_t capacity_rows, int64_t capacity_bytes, crh_text **out);
int crh_text_destroy(crh_text *t);
int crh_text_clear(crh_text *t); /* forget every row, keep the buffers */
int crh_text_count(crh_text *t, int64_t *rows_out, int64_t *bytes_out);

/* n rows behind the existing ones, host pointers: row_off [n + 1] starting at 0, bytes_host row_off[n] bytes.  CRH_E_INVALID,
 * with nothing stored, when n < 0 or the offsets do not start at 0 or decrease.  A row without bytes is allowed.  Synchronous. */
int crh_text_append(crh_text *t, int64_t n, const int64_t *row_off_host, const uint8_t *bytes_host);

/* Which rows hold the patterns.  Pattern p is pat_bytes_host[pat_off_host[p] .. pat_off_host[p + 1]): 1..CRH_TEXT_MAX_PATTERNS
 * patterns of 1..CRH_TEXT_MAX_PATTERN_BYTES bytes each (repeats allowed).
 *   A row MATCHES pattern p iff p's bytes occur contiguously inside that row's own bytes; a match never spans two rows.
 *   fold_case != 0 maps ASCII A..Z to a..z, on the text and on the pattern; every other byte compares as itself ('@', '[', '`',
 *   '{', NUL and all bytes >= 0x80: no Unicode case folding).
 *   combine: CRH_TEXT_ALL / CRH_TEXT_ANY.
 * Bit r of out_words_dev (u32 [ceil(rows / 32)], every word written) is set iff the row's bit is set in mask_dev (words as
 * crh_index_row_mask writes them, complete on `stream` before the call; NULL: every row < rows) and the row matches; bits at or
 * past `rows` are 0.  A tile whose mask word is 0 costs no read of its text.  out_count_host (int64, may be NULL) receives the
 * number of set bits, exact; with it the call waits for `stream`, without it it only enqueues.  Any violation of the limits, a
 * NULL pointer or an unknown `combine` is CRH_E_INVALID with nothing launched; an arena without rows is CRH_OK, count 0, no
 * launch.  Deterministic. */
int crh_text_match(crh_text *t, int n_pat, const int64_t *pat_off_host, const uint8_t *pat_bytes_host, int fold_case, int combine,
                   const uint32_t *mask_dev /* or NULL */, uint32_t *out_words_dev, int64_t *out_count_host /* or NULL */,
                   void *stream);

/* Which rows a regular expression matches, as a byte DFA the CALLER compiled (the store compiles Python's `re` syntax in
 * regex_dfa.py; a C host can bring a DFA from any compiler).  The semantics are the table's alone:
 *   s = 0; for each byte b of the row: s = trans[s * n_classes + class_of[b]]; then s = trans[s * n_classes + end_class];
 *   the row MATCHES iff s == accept_state.
 * Only the row's own bytes are walked: a match never sees a neighbouring row.  Checked on the host, CRH_E_INVALID with nothing
 * launched otherwise: n_states 1..CRH_REGEX_MAX_STATES, n_classes 2..257, n_states * n_classes <= CRH_REGEX_MAX_TABLE_BYTES,
 * every class_of[b] and end_class < n_classes, every trans entry and accept_state < n_states, and the accept state's row
 * ABSORBING (every entry is accept_state: the walk of a row stops early once it is reached).  mask_dev, out_words_dev,
 * out_count_host, `stream`, bits at or past `rows` and the arena without rows behave exactly as in crh_text_match.  The table
 * travels through a copy the handle owns: the caller may free its arrays on return.  At most ONE crh_text_match or
 * crh_text_regex per handle may be in flight (they share the handle's counter and table buffer).  A pair of tiles whose two mask
 * words are 0 costs no read of its text; otherwise a row costs a serial walk of its bytes, and 64 rows advance as fast as the
 * longest of them.  Deterministic. */
#define CRH_REGEX_MAX_STATES 256
#define CRH_REGEX_MAX_TABLE_BYTES 32768 /* n_states * n_classes */
int crh_text_regex(crh_text *t, int n_states, int n_classes, const uint8_t *class_of_host /* [256] */, int end_class,
                   const uint8_t *trans_host /* [n_states * n_classes] */, int accept_state, const uint32_t *mask_dev /* or NULL */,
                   uint32_t *out_words_dev, int64_t *out_count_host /* or NULL */, void *stream);

/* Which rows hold the pattern within a bounded number of byte edits: approximate substring match.  A row's
 * DISTANCE is the minimum over all substrings S of the row of Levenshtein(pattern, S), where the insertion, the deletion and
 * the substitution of one BYTE cost 1 each (a transposition therefore 2): min over j of D[len][j] of Sellers' table, D[0][j] = 0,
 * D[i][0] = i.  The empty row's distance is len.  The work is on bytes, like crh_text_regex: a multi-byte UTF-8 character is as
 * many edits as bytes of it differ.  fold_case folds the ASCII letters of both sides, exactly as crh_text_match does.
 * out_words_dev receives max_edits + 1 LEVELS of ceil(rows / 32) words each, level d behind level d - 1: bit r of level d is set
 * iff row r's distance is <= d and its bit of mask_dev is set -- the levels are nested, level max_edits is the filter's bitmap,
 * level 0 equals crh_text_match of the same pattern.  out_counts_host, when given, receives the max_edits + 1 levels' set bits
 * and makes the call wait on `stream`; without it the call only enqueues.  CRH_E_INVALID with nothing launched: len outside
 * 1..CRH_TEXT_MAX_PATTERN_BYTES, max_edits outside 0..CRH_FUZZY_MAX_EDITS, len <= max_edits (every row would match), NULL
 * pointers.  mask_dev, bits at or past `rows`, the arena without rows (CRH_OK, nothing launched, counts 0) and the one call in
 * flight per handle are as in crh_text_match.  A pair of tiles whose two mask words are 0 costs no read of its text; otherwise a
 * row costs a serial walk of its bytes, and 64 rows advance as fast as the longest of them.  Deterministic. */
#define CRH_FUZZY_MAX_EDITS 3
int crh_text_fuzzy(crh_text *t, const uint8_t *pat_host, int len, int max_edits, int fold_case,
                   const uint32_t *mask_dev /* or NULL */, uint32_t *out_words_dev /* [max_edits + 1][ceil(rows / 32)] */,
                   int64_t *out_counts_host /* [max_edits + 1] or NULL */, void *stream);

/* ---- the call graph on the device.  The reference keeps it in Memgraph (query/graph_reasoning/queries.py:
 * FIND_TRANSITIVE_CALLERS / _CALLEES, FIND_CALL_CHAIN); here it lies beside the index, and a set of reached nodes becomes a row
 * bitmap a search takes as CRH_COND_WORDS.  Every result is a set or a minimum depth: exact, and the same from run to run.
 *
 * A crh_graph holds up to CRH_GRAPH_MAX_RELATIONS relations ("calls", "extends", ...: the caller numbers them) over ONE node id
 * space 0 .. n_nodes - 1.  A relation is two CSRs in device memory: the forward one lists a node's targets (along the edges),
 * the reverse one its sources (against them); offsets int64 [n_nodes + 1], adjacency int32 [n_edges]. */
typedef struct crh_graph crh_graph; /* opaque */
#define CRH_GRAPH_MAX_RELATIONS 8
#define CRH_GRAPH_MAX_QUERIES 64   /* source sets of one crh_graph_bfs: bit q of a node's word belongs to set q */
#define CRH_GRAPH_MAX_HOPS 16
#define CRH_GRAPH_MAX_LIMIT (1 << 24) /* list entries per query of one crh_graph_list */
#define CRH_GRAPH_WAVE_DEGREE 64   /* an adjacency list of at least so many entries is walked by a whole wave, a shorter one by one lane */
#define CRH_GRAPH_ALONG 0   /* travel along the edges: from a caller to what it calls (callees) */
#define CRH_GRAPH_AGAINST 1 /* against them (callers) */
#define CRH_GRAPH_BOTH 2    /* either way */

int crh_graph_create(int device, int64_t n_nodes, crh_graph **out);
int crh_graph_destroy(crh_graph *g);
/* *nodes_out = n_nodes; *edges_out = the edges of relation `rel`, -1 while it is not set.  Either pointer may be NULL. */
int crh_graph_count(crh_graph *g, int rel, int64_t *nodes_out, int64_t *edges_out);

/* Sets or replaces relation `rel` (0 .. CRH_GRAPH_MAX_RELATIONS - 1) from host arrays.  Checked on the host, CRH_E_INVALID with the
 * relation left as it was: both offset arrays start at 0, never decrease and end at n_edges; every adjacency entry is a node.
 * That the two CSRs hold the same edges, without repeats, each list ascending, is the caller's business (a repeat costs time,
 * never exactness; crh_graph_path's tie rule reads the lists as they are).  Synchronous. */
int crh_graph_set_relation(crh_graph *g, int rel, int64_t n_edges, const int64_t *off_fwd_host, const int32_t *adj_fwd_host,
                           const int64_t *off_rev_host, const int32_t *adj_rev_host);

/* Breadth-first search from nq (1..CRH_GRAPH_MAX_QUERIES) SOURCE SETS at once.  Set q is src_nodes[src_off[q] .. src_off[q + 1]);
 * src_off (int64 [nq + 1], from 0) is a HOST array always, src_nodes a host array (sources_on_device = 0; an entry that is
 * neither a node nor -1 is CRH_E_INVALID) or a device array complete on `stream` (!= 0; an entry that is no node is skipped).
 * -1 is padding; an empty set and a repeated source are fine.
 *   levels_dev u64 [max_hops + 1][n_nodes]: bit q of levels[d][v] is set iff node v is at MINIMUM depth d from set q in
 *     `direction` (CRH_GRAPH_*); level 0 holds the sources.  Every word is written.
 *   seen_dev   u64 [n_nodes]: the OR of the levels; with include_self = 0 the bits of level 0 are cleared from it (they stay in
 *     level 0; a source that lies on a cycle is not listed a second time at the cycle's length).
 *   active_dev u64 [max_hops + 1]: the OR of level d's words.
 * 1 <= max_hops <= CRH_GRAPH_MAX_HOPS.  One launch per level, none waits for another workgroup; a level behind a dead frontier
 * leaves at once.  Enqueues on `stream` and returns (a host source list is uploaded first, and the call waits for that upload
 * only).  One BFS per handle may be in flight.  A graph without nodes is CRH_OK with nothing launched. */
int crh_graph_bfs(crh_graph *g, int rel, int direction, int nq, const int64_t *src_off_host, const int32_t *src_nodes,
                  int sources_on_device, int max_hops, int include_self, uint64_t *levels_dev, uint64_t *seen_dev,
                  uint64_t *active_dev, void *stream);

/* What a BFS reached, per query, from its levels: the nodes of levels first_level .. max_hops (1: without the sources) ordered by
 * (depth, node id) into out_nodes_dev / out_depth_dev int32 [nq][limit], padding -1, every slot written; out_count_dev int64
 * [nq] = how many there are, exact, never clipped at limit.  0 <= limit <= CRH_GRAPH_MAX_LIMIT (0: the counts alone).  Enqueues. */
int crh_graph_list(crh_graph *g, int nq, const uint64_t *levels_dev, int max_hops, int first_level, int limit, int32_t *out_nodes_dev,
                   int32_t *out_depth_dev, int64_t *out_count_dev, void *stream);

/* The reached nodes of query q as a ROW BITMAP: bit i of word t is set iff 32 t + i < n_rows, v = row_node_dev[32 t + i] is a node
 * (0 <= v < n_nodes; -1: the row's key is no node) and bit q of seen_dev[v] is set.  u32 [n_words], n_words >= ceil(n_rows / 32);
 * the layout crh_index_row_mask writes; tail bits and the words beyond the rows are 0.  Runs on the CURRENT device; enqueues. */
int crh_graph_row_words(const int32_t *row_node_dev, int64_t n_rows, const uint64_t *seen_dev, int64_t n_nodes, int q,
                        uint32_t *out_words_dev, int64_t n_words, void *stream);

/* One shortest path of query q to `target`, from the levels of a crh_graph_bfs with the same rel, direction and max_hops: walks
 * back from the target's level, at every step to the SMALLEST node id among the neighbours that lie in the level before.
 * out_nodes_host int32 [max_hops + 1] receives the nodes from a source to the target, *out_len how many (1: the target is a
 * source; 0: not reached within max_hops).  Waits on `stream`. */
int crh_graph_path(crh_graph *g, int rel, int direction, const uint64_t *levels_dev, int q, int64_t target, int max_hops,
                   int32_t *out_nodes_host, int *out_len, void *stream);

/* ---- chains in full: how many shortest chains, the K first of them, the nodes between two sets, a BFS that avoids a node
 * (DESIGN.md 3.32).  Exact integers over the levels of a crh_graph_bfs(rel, direction, ..., max_hops, include_self = 1); the
 * definitions are this repository's own and a CPU restatement of the text below gives the same words.  direction is
 * CRH_GRAPH_ALONG or CRH_GRAPH_AGAINST: CRH_GRAPH_BOTH is CRH_E_INVALID.  "u's pull list" is the list that BFS pulls through
 * (ALONG: u's sources, the reverse CSR; AGAINST: its targets), read as it is; the host builder makes every list ascending.
 * Every call enqueues on `stream`; a bad argument is CRH_E_INVALID with nothing launched, a graph without nodes CRH_OK with
 * nothing launched.
 *
 * crh_graph_sigma: sigma_out_dev u64 [n_nodes][QS], QS the smallest power of two >= nq, column q = query q, the columns from nq
 * on 0, every word written.  sigma[v][q] = 1 where bit q of levels[0][v] is set; for d = 1 .. max_hops and u with bit q in
 * levels[d][u], sigma[u][q] = the SATURATING sum, min(true sum, 2^64 - 1), of sigma[v][q] over the entries v of u's pull list
 * with bit q in levels[d - 1][v]; 0 everywhere else.  All terms are >= 0, so the saturated sum does not depend on the order of
 * addition.  sigma[t][q] is the number of SHORTEST chains from source set q to t (0: not reached within max_hops; 2^64 - 1: at
 * least that many).  active_dev is the BFS's: a level whose word is 0 leaves at once.  One launch for level 0 and the zeros,
 * one per level after it; an entry has one writer. */
int crh_graph_sigma(crh_graph *g, int rel, int direction, int nq, const uint64_t *levels_dev, const uint64_t *active_dev, int max_hops,
                    uint64_t *sigma_out_dev, void *stream);

/* The K first shortest chains of every query q to its target t_q (targets: int32 [nq], a host array -- an entry that is
 * neither a node nor -1 is CRH_E_INVALID, -1 has no chain -- or, targets_on_device != 0, a device array complete on `stream`,
 * where an entry that is no node yields count 0).  levels_dev and sigma_dev are crh_graph_bfs' and crh_graph_sigma's for the
 * same rel, direction, nq and max_hops.  Chains are ORDERED by their node ids read BACKWARDS from the target: the node before
 * the target first, then the one before that.  Chain r, 0 <= r < min(K, count), is found by unranking: rem = r, u = t_q, d =
 * the target's level; while d > 0 walk u's pull list in order over the entries v with bit q in levels[d - 1][v] -- if rem <
 * sigma[v][q] step to v (d - 1), otherwise rem -= sigma[v][q].  A saturated sigma compares as the true one would, since rem <
 * K <= CRH_GRAPH_MAX_CHAINS.  Chain 0 is, node for node, crh_graph_path's.
 *   out_nodes_dev int32 [nq][K][max_hops + 1]: from a source to the target, padded with -1; every slot written.
 *   out_len_dev   int32 [nq]: the nodes of each chain (1: the target is a source), 0 when the target is not reached.
 *   out_count_dev u64 [nq]: sigma[t_q][q].
 * One wave per (query, rank), 64 list entries per step. */
#define CRH_GRAPH_MAX_CHAINS 64
int crh_graph_chains(crh_graph *g, int rel, int direction, int nq, const uint64_t *levels_dev, const uint64_t *sigma_dev, int max_hops,
                     const int32_t *targets, int targets_on_device, int K, int32_t *out_nodes_dev, int32_t *out_len_dev,
                     uint64_t *out_count_dev, void *stream);

/* The nodes BETWEEN source set q and target set q.  levels_fwd_dev: a BFS from the source sets; levels_back_dev: a BFS in the
 * OPPOSITE direction from the target sets; both with this max_hops and include_self = 1.  With dF and dB a node's two minimum
 * depths, bit q of out_words_dev[v] (u64 [n_nodes], the layout of seen_dev, which crh_graph_row_words takes) is set iff both
 * exist and
 *   CRH_GRAPH_BETWEEN_ANY       dF + dB <= max_hops: v lies on a WALK of at most max_hops edges from the one set to the other
 *                               (a walk, not a simple path: the two halves may share a node); the ends are included
 *   CRH_GRAPH_BETWEEN_SHORTEST  dF + dB == D_q, the least dF + dB over all nodes, where that is <= max_hops: v lies on a
 *                               shortest chain
 * out_dist_dev int32 [nq], or NULL: D_q, -1 where the sets do not meet within max_hops.  meet_dev u64 [max_hops + 1] is the
 * caller's work array (meet[d] = the queries with a node at dF + dB = d).  Two launches; runs on the CURRENT device. */
#define CRH_GRAPH_BETWEEN_ANY 0
#define CRH_GRAPH_BETWEEN_SHORTEST 1
int crh_graph_between(int64_t n_nodes, int nq, const uint64_t *levels_fwd_dev, const uint64_t *levels_back_dev, int max_hops, int mode,
                      uint64_t *meet_dev /* u64 [max_hops + 1], caller-owned */, uint64_t *out_words_dev, int32_t *out_dist_dev /* or NULL */,
                      void *stream);

/* crh_graph_bfs with an AVOIDED node set per query: avoid_dev u64 [n_nodes], bit q at v = query q never enters v.  Level 0 =
 * sources & ~avoid, next[u] = pulled & ~seen[u] & ~avoid[u]; everything else as crh_graph_bfs.  With it "v is a MUST-PASS node
 * of (S, t)" is decided: v is neither t nor a source, t is reached from S within max_hops, and is not once v may not be
 * entered.  The statement is bounded by max_hops: a detour longer than that does not count.  Such a v lies on every chain,
 * hence on chain 0: its interior nodes are the candidates. */
int crh_graph_bfs_avoiding(crh_graph *g, int rel, int direction, int nq, const int64_t *src_off_host, const int32_t *src_nodes,
                           int sources_on_device, int max_hops, int include_self, const uint64_t *avoid_dev, uint64_t *levels_dev,
                           uint64_t *seen_dev, uint64_t *active_dev, void *stream);

/* ---- graph-propagated relevance: personalised PageRank seeded by hits or by named nodes.  The definition is
 * this repository's own, and it is exact: the device result is the same BITS as a CPU restatement that follows the text below.
 *
 * For a relation and a direction, node u's PULL LIST is the one crh_graph_bfs pulls through: ALONG its sources (the reverse
 * CSR's list), AGAINST its targets (the forward list), BOTH the reverse list, then the forward list, multiplicity kept.  out(v)
 * is the length of the OPPOSITE list or lists (ALONG: v's forward list; AGAINST: its reverse list; BOTH: the sum of the two);
 * inv[v] = 1.0f / (float)out(v), 0 where out(v) == 0.
 *   Seeds.  Query q has c entries (node, weight), 1 <= c <= CRH_MAX_K; node == -1 or weight == 0 is padding.  w_q[v] = the f32 sum
 *     of the weights of v's entries in list order, S_q = the f32 sum of all real weights in list order, p0[v] = w_q[v] / S_q.
 *     A query whose S_q is not a finite value > 0 has p0 = 0 everywhere, and every score 0.  A HOST list is checked (a node
 *     outside -1 .. n_nodes - 1, a weight that is not finite and >= 0: CRH_E_INVALID); a DEVICE list is clamped by the kernel:
 *     an entry that is no node is padding, a negative, NaN or infinite weight counts as +0.  seed_weights NULL: every weight 1.
 *   Steps.  restart is an f32 inside (0, 1), a = 1.0f - restart in f32.  For t = 0 .. steps - 1, 1 <= steps <= CRH_GRAPH_PPR_MAX_STEPS:
 *       contrib[v] = p_t[v] * inv[v]
 *       acc[u]     = 0.0f, then += contrib[v] for v in u's pull list, IN LIST ORDER, each addition rounded to f32
 *       p_{t+1}[u] = (restart * p0[u]) + (a * acc[u])
 *     Every operation is a separate f32 rounding (no fused multiply-add); subnormals are kept.  The mass of a node with out == 0
 *     is dropped: at the fixed point that ranks like "dangling nodes jump back to the seeds" (the two solutions are
 *     proportional) and needs no grid-wide sum.  The result is p_steps; every score is >= +0.
 *   No float atomics, no tree or strided reduction of a pull list (a hub's list is walked in order by the lanes that own the
 *   hub), nothing grid-wide inside a launch: one launch per step over ping-pong buffers.
 *
 * State layout: f32 [n_nodes][QS], QS the smallest power of two >= nq (1 .. 64); column q belongs to query q, the columns from
 * nq on are 0.  work_dev holds 3 * n_nodes * QS floats, out_dev n_nodes * QS; both are caller-owned and overwritten (every word
 * of out_dev is written).  Seeds int32 / f32 [nq][c], on the host (seeds_on_device = 0; uploaded first, and the call waits for
 * that upload only) or on the device, complete on `stream`.  The first call for a (relation, direction) builds inv and waits
 * for it; crh_graph_set_relation drops it.  Enqueues.  Any bad argument is CRH_E_INVALID with nothing launched; a graph without
 * nodes is CRH_OK with nothing launched.  One PPR per handle may be in flight with host seeds. */
#define CRH_GRAPH_PPR_MAX_STEPS 64
int crh_graph_ppr(crh_graph *g, int rel, int direction, int nq, int c, const int32_t *seed_nodes /* [nq, c] */,
                  const float *seed_weights /* [nq, c] or NULL */, int seeds_on_device, float restart, int steps,
                  float *work_dev /* [3, n_nodes, QS] */, float *out_dev /* [n_nodes, QS] */, void *stream);

/* The scores of a crh_graph_ppr (same nq) as the histograms crh_facet_select takes: out_bins_dev int64 [nq][n_nodes], bins[q][v]
 * = the bit pattern of p[v][q], which orders like the value for every f32 >= +0.  exclude_dev int32 [nq][c] (c 0..CRH_MAX_K; NULL
 * with c = 0): the nodes named in row q get 0 in query q; an entry that is no node is skipped.  crh_facet_select over these bins
 * is the top-k nodes by descending score, ties to the lower node id, a zero score never returned.  Runs on the CURRENT device;
 * enqueues. */
int crh_graph_ppr_bins(int64_t n_nodes, int nq, const float *scores_dev /* [n_nodes, QS] */, int c,
                       const int32_t *exclude_dev /* [nq, c] or NULL */, int64_t *out_bins_dev /* [nq, n_nodes] */, void *stream);

/* A candidate table (rows int64 / cosine f32 as a search returns them, rows < 0 = padding; nodes int32, -1: the row's key is no
 * node; each [nq][c], 1 <= c <= CRH_MAX_K) as the TWO lists crh_fuse_select fuses with m = 2, out_fuse_scores_dev f32 /
 * out_fuse_rows_dev int64 [nq][2][c]: list 0 is the table as it stands; list 1 holds the candidates with graph_score > 0 by
 * descending graph_score, ties to the EARLIER position, padded with (-1, -inf).  graph_score[i] = p[node_i][q], 0 for padding and
 * for a row without a node; out_graph_score_dev f32 [nq][c] keeps it per position (crh_fuse_select's out_first of a row is its
 * position in list 0).  One workgroup per query, rank by counting.  Runs on the CURRENT device; enqueues. */
int crh_graph_ppr_order(int64_t n_nodes, int nq, int c, const float *scores_dev /* [n_nodes, QS] */, const int64_t *rows_dev,
                        const float *cosine_dev, const int32_t *nodes_dev, float *out_fuse_scores_dev, int64_t *out_fuse_rows_dev,
                        float *out_graph_score_dev, void *stream);

/* ---- the structure of the whole graph: strongly connected components and the layers of the condensation.
 * Every result is a uniquely defined integer: exact, and the same from run to run.  Every phase is a sequence of SWEEPS, one
 * launch each, one lane per node (a list of CRH_GRAPH_WAVE_DEGREE entries or more is walked by the node's whole wave), none of
 * which waits for another workgroup.  A sweep is monotone towards a fixed point that does not depend on the order of updates,
 * so it updates in place; it makes one atomicOr per workgroup into a `changed` word, the next launch reads that word and leaves
 * at once when it is 0, and the host reads the words back once per 16 sweeps.
 *
 * crh_graph_scc: comp_out_dev int32 [n_nodes], comp[v] = the SMALLEST node id of v's strongly connected component in relation
 * `rel` (both CSRs are read; an entry u == v of a list is ignored).  Rounds of
 *   trim      an unassigned node without an unassigned in-neighbour, or without an unassigned out-neighbour: comp[v] = v;
 *   colour    colour[v] = v, then min with the colours of the unassigned in-neighbours: the smallest unassigned id that reaches v;
 *   back-mark colour[r] == r: comp[r] = r; then an unassigned v joins comp[v] = colour[v] once an out-neighbour w has
 *             comp[w] == colour[v]
 * each to its fixed point, until a trim leaves no node unassigned.  work_dev int32 [n_nodes + CRH_GRAPH_SCC_WORK_EXTRA],
 * caller-owned, overwritten.  info_host int64 [4] = (components, components of two nodes or more, the nodes in those, sweeps
 * launched, those that left at once included); a self-loop is unknown here: crh_graph_scc_bins counts with them.
 * BOUND.  A trim sweep that changes something assigns a node (at most n of them in all) and each of the at most n + 1 rounds
 * ends with one that changes nothing; with m nodes left, a colour or a label travels a simple path, so the colour and the
 * back-mark phase change something in at most m - 1 sweeps each and run one more; every round assigns its smallest id at
 * least, so m <= n, n - 1, ...: in all at most n + (n + 1) + n (n + 1) < CRH_GRAPH_SCC_MAX_SWEEPS(n) sweeps that run.  The host
 * loop stops there with CRH_E_INTERNAL (unreachable for CSRs that hold the same edges) and never loops on.
 * WAITS on `stream` (it reads the changed words between batches of sweeps), unlike the "enqueues" calls.  Any bad argument is
 * CRH_E_INVALID with nothing launched, info zeroed where there is one; a graph without nodes is CRH_OK with nothing launched. */
#define CRH_GRAPH_SCC_WORK_EXTRA 32
#define CRH_GRAPH_SCC_MAX_SWEEPS(n) (((int64_t)(n) + 2) * ((int64_t)(n) + 2))
#define CRH_GRAPH_LAYERS_MAX_SWEEPS(n) ((int64_t)(n) + 1)
int crh_graph_scc(crh_graph *g, int rel, int32_t *comp_out_dev /* [n_nodes] */, int32_t *work_dev /* [n_nodes + CRH_GRAPH_SCC_WORK_EXTRA] */,
                  int64_t *info_host /* [4] */, void *stream);

/* The CYCLIC components as the histogram crh_facet_select takes: out_bins_dev int64 [n_nodes], bins[c] = the number of nodes v
 * with comp[v] == c when that number is at least 2, or is 1 and c is in self_nodes_dev (int32, sorted ascending, distinct; NULL
 * with n_self = 0: the nodes that carry a self-loop, which the CSRs do not keep); 0 otherwise.  A label outside 0 .. n_nodes - 1
 * counts nowhere.  Integer atomics: exact whatever the order.  crh_facet_select(1, n_nodes, k, bins, ...) is then the k largest
 * cyclic components, ties to the lower label, and its info (cyclic components, nodes in them).  Runs on the CURRENT device;
 * enqueues; every bin is written.  Bad arguments (n_self outside 0 .. n_nodes, NULL pointers) are CRH_E_INVALID with nothing
 * launched; n_nodes = 0 is CRH_OK with nothing launched. */
int crh_graph_scc_bins(int64_t n_nodes, const int32_t *comp_dev, const int32_t *self_nodes_dev /* or NULL */, int64_t n_self,
                       int64_t *out_bins_dev /* [n_nodes] */, void *stream);

/* The longest-path layer of every node's component in the CONDENSATION (every component shrunk to one node), comp_dev as
 * crh_graph_scc wrote it for the same relation: out_dev int32 [n_nodes] = the least fixed point, from zeros, of
 *   layer[v] = max over u of layer[u] + (comp[u] != comp[v]),
 * u running over v's in-neighbours for CRH_GRAPH_ALONG (DEPTH: 0 for a node nobody outside its own cycle calls) and over its
 * out-neighbours for CRH_GRAPH_AGAINST (HEIGHT: 0 for a node that calls nothing outside its own cycle); CRH_GRAPH_BOTH is
 * CRH_E_INVALID.  Bellman-Ford with weights 0 and 1: a longest walk can be taken simple (a cycle lies inside a component and
 * weighs 0), so a value travels at most n - 1 edges: at most n sweeps run, and the host loop stops at
 * CRH_GRAPH_LAYERS_MAX_SWEEPS(n) with CRH_E_INTERNAL -- which is what labels that are no components of this relation get.
 * Labels are compared, never used as an index.  work_dev int32 [CRH_GRAPH_SCC_WORK_EXTRA].  info_host int64 [2] = (layers =
 * the largest value + 1, sweeps launched).  WAITS on `stream`.  Argument handling as crh_graph_scc. */
int crh_graph_layers(crh_graph *g, int rel, int direction, const int32_t *comp_dev, int32_t *out_dev /* [n_nodes] */,
                     int32_t *work_dev /* [CRH_GRAPH_SCC_WORK_EXTRA] */, int64_t *info_host /* [2] */, void *stream);

/* A condition on every node as the `seen` words of a BFS, for crh_graph_row_words: out_words_dev u64 [n_nodes], word v = 1 << q
 * where the condition holds and 0 elsewhere (every word is written), x = values_dev[v] (int32 [n_nodes]):
 *   CRH_GRAPH_WORDS_IN_CYCLE        0 <= x < n_nodes and bins_dev[x] > 0 (values = components, bins = crh_graph_scc_bins')
 *   CRH_GRAPH_WORDS_SAME_COMPONENT  x == lo                               (values = components, lo = a label)
 *   CRH_GRAPH_WORDS_RANGE           lo <= x <= hi                         (values = layers; lo > hi is an empty range)
 * bins_dev is read by the first mode only and may be NULL otherwise.  0 <= q < CRH_GRAPH_MAX_QUERIES.  Runs on the CURRENT
 * device; enqueues.  Bad arguments are CRH_E_INVALID with nothing launched; n_nodes = 0 is CRH_OK with nothing launched. */
#define CRH_GRAPH_WORDS_IN_CYCLE 0
#define CRH_GRAPH_WORDS_SAME_COMPONENT 1
#define CRH_GRAPH_WORDS_RANGE 2
int crh_graph_node_words(int64_t n_nodes, int mode, const int32_t *values_dev, const int64_t *bins_dev /* or NULL */, int64_t lo,
                         int64_t hi, int q, uint64_t *out_words_dev /* [n_nodes] */, void *stream);

/* ---- the hybrid re-rank with both branches on the device.  QueryEngine.search (query/engine.py:222-260) hands
 * HybridRanker.rank_results a graph context AND the vector hits; crh_rerank_vector above covers lists of vector hits only.  The
 * three entry points below turn the BFS lists of crh_graph_list into graph candidates and rank them together with the hits. */

/* A node's REPRESENTATIVE ROW: the lowest alive global row (row_base + local) whose entry of the row -> node column is that
 * node -- the row whose payload (file, lines, summary) stands for the node in a result.  row_node_dev int32 [n_rows] (-1 or
 * anything outside 0 .. n_nodes - 1: the row's key is no node); alive_words_dev u32 [ceil(n_rows / 32)], bit i of word t =
 * local row 32 t + i is alive (the layout crh_index_row_mask writes), or NULL: every row is alive.  node_rows_dev int64
 * [n_nodes] is PRE-FILLED with -1 by the caller; one lane per row takes a 64-bit atomic minimum on the unsigned view, where -1
 * is the maximum, so the shards of a collection call this one after the other on the same array and the result is exact
 * whatever the order.  A node without an alive row keeps -1: it can never become a graph result.  Runs on the CURRENT device;
 * enqueues. */
int crh_graph_node_rows(int64_t n_rows, const int32_t *row_node_dev, const uint32_t *alive_words_dev, int64_t row_base, int64_t n_nodes,
                        int64_t *node_rows_dev, void *stream);

/* The roles of a graph result, in the order HybridRanker walks them (ranker.py:70-169: primary entities, callers, callees,
 * methods, parent classes, child classes). */
#define CRH_ROLE_PRIMARY 0
#define CRH_ROLE_CALLER 1
#define CRH_ROLE_CALLEE 2
#define CRH_ROLE_METHOD 3
#define CRH_ROLE_PARENT 4
#define CRH_ROLE_CHILD 5
#define CRH_GRAPH_CAND_MAX_QUERIES 1024
#define CRH_GRAPH_CAND_MAX_SEGMENTS (1 << 20)

/* One run of graph candidates of one query: an explicit node (node >= 0: a primary entity; list_row and take are not read), or
 * the first `take` entries of row list_row of a crh_graph_list table (node < 0). */
typedef struct crh_graph_segment {
    int32_t query;
    int32_t role;     /* CRH_ROLE_* */
    int32_t node;
    int32_t list_row;
    int32_t take;
    int32_t pad_;
} crh_graph_segment;

/* The per-query graph candidate table.  segments_host holds n_segments segments sorted by query; within a query they stand in
 * the reference's order (all primaries, all caller lists in primary order, all callee lists, methods, parents, children).
 * list_nodes_dev / list_depth_dev int32 [n_lists][limit] are what crh_graph_list wrote (several calls' tables laid end to
 * end); node_rows_dev int64 [n_nodes] is crh_graph_node_rows' array.  Per query the entries of its segments are written in order
 * into out_node / out_role / out_depth int32 [nq][G] and out_row int64 [nq][G] (the representative row); a -1 list entry and a
 * node without a representative row are dropped IN PLACE (the order of the rest is kept), entries beyond G are cut, the slots
 * behind the last entry are (-1, -1, -1, -1): every slot is written.  An explicit node has depth 0.  Checked on the host in the
 * manner of crh_graph_set_relation, CRH_E_INVALID with nothing launched: queries ascending and < nq, roles, explicit nodes <
 * n_nodes, list rows < n_lists, take >= 0 (a take beyond `limit` reads `limit` entries) -- no lane is handed an index outside
 * its arrays.  segments_dev [n_segments] and seg_off_dev int32 [nq + 1] are caller-provided device scratch the call fills.  One
 * wave per query.  nq <= CRH_GRAPH_CAND_MAX_QUERIES.  Runs on the CURRENT device; uploads the table on `stream`, waits for that
 * upload only (segments_host is free on return, as crh_graph_bfs' source list) and enqueues the kernel. */
int crh_graph_candidates(int nq, int G, int n_segments, const crh_graph_segment *segments_host, const int32_t *list_nodes_dev,
                         const int32_t *list_depth_dev, int n_lists, int limit, const int64_t *node_rows_dev, int64_t n_nodes,
                         crh_graph_segment *segments_dev, int32_t *seg_off_dev, int32_t *out_node_dev, int64_t *out_row_dev,
                         int32_t *out_role_dev, int32_t *out_depth_dev, void *stream);

#define CRH_RR_MAX_HYBRID 512      /* graph + vector candidates of one query: 84 bytes of LDS each, 42 KB */
#define CRH_RR_HYBRID_SIGNALS 7    /* graph_match, query_entity_match, relationship_relevance, centrality, context_richness,
                                      vector_similarity, code_quality -- the order of out_signals and of the presence bits */
#define CRH_RR_HYBRID_TABLE 128    /* distinct centrality keys one query's table holds; more sends the query to the host */

/* crh_rerank_query + what score_graph_result reads (scorer.py:9-77): the intent's graph and context weights
 * (RankingConfig.weights_for) and RankingConfig.relationship_bonus. */
typedef struct crh_rerank_hybrid_query {
    crh_rerank_query base;
    double graph_weight;
    double context_weight;
    double relationship_bonus;
} crh_rerank_hybrid_query;

/* HybridRanker.rank_results (ranker.py:24-54) for nq queries, one workgroup each.  A query's candidates are its G graph entries
 * (g_rows_dev / g_role_dev / g_depth_dev [nq][G] as crh_graph_candidates wrote them, g_rows < 0 = padding; g_cols = the side
 * columns of the representative rows, crh_gather_rerank_columns; g_rich_dev int32 [nq][G] = richness bits of those rows: bit 0
 * summary, bit 1 docstring, bit 2 signature) FOLLOWED BY its k vector hits exactly as crh_rerank_vector takes them.  1 <= G + k <=
 * CRH_RR_MAX_HYBRID, either may be 0 (its pointers are then not read); more is CRH_E_INVALID.
 *   graph entry (scorer.py:9-77): graph_match = max(0.3, 1.0 - (depth - 1) * 0.2) for callers and callees (depth 0 counts as 1),
 *     1.0 otherwise; relationship_relevance 1.0 / 0.8 / 0.7 / 0.5 (primary / caller / callee / other); query_entity_match and
 *     centrality as for a hit; context_richness = 0.3 summary + 0.2 docstring + 0.2 signature summed in that order from 0.0 (a
 *     graph node carries no content); score = the five products with graph_weight, entity_match_bonus, relationship_bonus,
 *     centrality_weight, context_weight, summed left to right.
 *   vector entry: crh_rerank_vector's formula (scorer.py:80-126).
 *   centrality table (engine.py:348-377, insertion-ordered): the keys of the first primary_top PRIMARY graph entries, then of the
 *     named ones among the first centrality_top hits, one entry per key, cut at centrality_limit keys; a key whose degree is < 0
 *     answers no lookup.
 *   merge (ranker.py:171-202): the first entry of a key absorbs the later ones in list order, c = (f + f_j) / 2; c = c * 1.1; the
 *     signals are a UNION, the larger value where both carry one; any merge makes the result "hybrid".
 *   stable descending sort, per-file cap, total cap as in crh_rerank_vector.
 * Outputs per query in final order, [nq][max_total]: out_index (position in the concatenated list; < G: a graph entry, whose
 * role and depth the caller reads there), out_score f64, out_signals f64 [..][CRH_RR_HYBRID_SIGNALS] with out_mask's bit t set
 * iff signal t is PRESENT (absent is not 0.0), out_flags bit 0 = hybrid, bit 1 = the first entry was a graph entry.
 * out_count[q] = survivors, or -1: the host must rank this query (entities outside 0..CRH_RR_MAX_ENTITIES, a name longer than
 * CRH_RR_NAME_BYTES, more than CRH_RR_HYBRID_TABLE centrality keys).  The slots behind the survivors are written (-1, 0, ...).
 * All arithmetic in f64 in the reference's operand order.  Runs on the CURRENT device; enqueues. */
int crh_rerank_hybrid(int nq, int G, int k, const int64_t *g_rows_dev, const int32_t *g_role_dev, const int32_t *g_depth_dev,
                      const crh_rerank_columns *g_cols, const int32_t *g_rich_dev, const float *scores_dev, const int64_t *rows_dev,
                      const crh_rerank_columns *cols, const crh_rerank_hybrid_query *queries_dev, double entity_match_bonus,
                      int max_per_file, int max_total, int primary_top, int centrality_top, int centrality_limit, int32_t *out_index_dev,
                      double *out_score_dev, double *out_signals_dev, int32_t *out_mask_dev, int32_t *out_count_dev, int32_t *out_flags_dev,
                      void *stream);

/* ------------------------------------------------------------- encoder --------- */
/* UniXcoder = RoBERTa-base geometry encoder (providers/unixcoder_provider.py:137-155 and
 * the HF RobertaModel it wraps).  All pointers are device pointers; activations bf16,
 * LayerNorm / softmax / accumulation f32.  T = total tokens (sum of padded rows). */

/* y[T, N] = act(x[T, K] @ w[N, K]^T + bias[N]); act: 0 none, 1 erf-GELU.  out bf16. */
int crh_gemm_bf16_bias(const void *x, const void *w, const float *bias, void *y, int T, int N, int K,
                       int act, void *stream);

/* y[T, N] = LayerNorm(x @ w^T + bias + residual) * gamma + beta  (post-LN block end). N == 768. */
int crh_gemm_bf16_bias_res_ln(const void *x, const void *w, const float *bias, const void *residual,
                              const float *gamma, const float *beta, float eps, void *y, int T, int N,
                              int K, void *stream);

/* The same with the RESIDUAL STREAM IN F32 (ABI 4; opt-in fidelity lever: the reference's forward is fp32 throughout,
 * unixcoder_provider.py:137-155): y[T, 768] = bf16(LayerNorm(bf16(x @ w^T + bias) + residual_f32)) for the next GEMM, and
 * residual_f32[T, 768] is REPLACED by the same LayerNorm output in f32 -- the next residual.  N == 768. */
int crh_gemm_bf16_bias_res32_ln(const void *x, const void *w, const float *bias, float *residual_f32, const float *gamma, const float *beta,
                                float eps, void *y, int T, int N, int K, void *stream);

/* The same post-LN block with the LayerNorm FOLDED into the GEMMs around it (ABI 4; modeling_roberta.py:329-340,387-398 --
 * RobertaSelfOutput / RobertaOutput: dense, dropout, LayerNorm(hidden + input): the arithmetic these two entry points split
 * differently).  The residual stream stays UN-normalised between kernels; no [T, 768] tensor is read or written just to be
 * normalised (crh_encoder.hip, "LayerNorm folded into the GEMMs around it").
 *
 * crh_gemm_bf16_res_lnstats -- the producer (O-projection, FFN2): y[T, 768] = bf16(x @ w^T + bias + h), h = the previous
 *   LayerNorm's output worked out from ITS un-normalised rows: h = (residual * rstd + nmr) * res_gamma (+ its beta, which the
 *   caller folds into `bias`), with res_stats[T][2] = (rstd, nmr = -mu * rstd); res_stats == NULL: h = residual as it is.
 *   Also writes stats_out[T][2] = (rstd, nmr) of the rows of y as stored (what the next LayerNorm needs); `partials` is
 *   caller-provided scratch of T * (N / 32) * 2 floats.  y must not alias residual.  N == 768.
 * crh_gemm_bf16_lnin -- the consumer (QKV, FFN1): y[T, N] = act(LayerNorm(x) @ w^T + bias) computed as
 *   rstd * (x @ w_scaled^T - mu * colsum) + bias_folded, with x the un-normalised rows, row_stats[T][2] = (rstd, nmr) from the
 *   call above, w_scaled[N, K] = w * gamma (per k, rounded to bf16), colsum[N] = sum_k w_scaled[n][k] (of the ROUNDED values),
 *   bias_folded[N] = bias + w @ beta. */
int crh_gemm_bf16_res_lnstats(const void *x, const void *w, const float *bias, const void *residual, const float *res_stats,
                              const float *res_gamma, float eps, void *y, float *partials, float *stats_out, int T, int N, int K,
                              void *stream);
int crh_gemm_bf16_lnin(const void *x, const float *row_stats, const void *w_scaled, const float *colsum, const float *bias_folded,
                       void *y, int T, int N, int K, int act, void *stream);
/* y[T, 768] = bf16((x * rstd + nmr) * gamma + beta): the LayerNorm output itself from statistics already known (the last layer of a
 * folded forward: the masked mean pool, unixcoder_provider.py:152-154, reads normalised rows).  y may be x. */
int crh_layernorm_apply(const void *x, const float *row_stats, const float *gamma, const float *beta, void *y, int T, int N, void *stream);

/* Bidirectional self-attention with key masking.  qkv [B*L, 3*H*64] bf16 exactly as the QKV GEMM writes it
 * (q | k | v thirds, head-major inside each), out [B*L, H*64] bf16.  kmask: uint64 [B, ceil(L/64)], bit j of word t
 * set when token 64t+j of the row is a real token (ids != pad) -- the reference's `mask` (unixcoder_provider.py:148).
 * L % 16 == 0 (padding granularity of a length bucket), L <= 1024.  Rows of up to 512 tokens run k_attn (a row's K/V staged
 * whole in LDS); 513..1024 run k_attn_long (K/V streamed through LDS in 256-key windows), which gives a row that would fit
 * k_attn the same bits as k_attn does. */
int crh_attn_fwd_varlen(const void *qkv, const uint64_t *kmask, void *out, int B, int L, int H, void *stream);

/* out[b, t, :] = LN((word[ids[b,t]] + type[0]) + pos[pos_id]); pos_id = cumsum(ids != pad) * (ids != pad) + pad.
 * ids int32 [B, L]; tables bf16; out bf16 [B, L, 768].  Also writes kmask (see above).
 * The library is not told the table heights: every id must index a row of `word`, and `pos` must hold
 * pad_id + L + 1 rows -- the caller checks (the Python driver does, encoder.py `_check_ids`). */
int crh_embed_ln(const int32_t *ids, const void *word, const void *pos, const void *type0,
                 const float *gamma, const float *beta, float eps, int pad_id, void *out,
                 uint64_t *kmask, int B, int L, int D, void *stream);

/* sent[b, :] = sum over real tokens of tok[b, t, :] / #real tokens  (f32 out, no L2 normalisation). */
int crh_masked_mean_pool(const void *tok, const uint64_t *kmask, float *sent, int B, int L, int D,
                         void *stream);

/* Packed rows: the same three kernels on a batch WITHOUT padding.  Row b of the batch is the tokens
 * [row_off[b], row_off[b+1]) of one flat token axis of T tokens (ids int32 [T], activations [T, ...]); Lmax (a multiple of
 * 16, >= every row's length, <= 1024) sizes the key-mask stride (ceil(Lmax/64) words per row) and the launch (Lmax > 512:
 * the long-row attention kernel, the same bits for every row).  The GEMM /
 * LayerNorm entry points above take T tokens as they are.  What it buys: the padded form rounds every row up to its bucket's
 * length (a multiple of 16) -- ~4 % of the tokens of a mean-200 mix -- and every kernel of the forward pays for them.
 * row_off lives on the device, so the library cannot look at it when a call is made: every kernel CLAMPS what it reads from
 * it to the T tokens the buffers hold (a bad offsets array can produce wrong rows, never an access outside the buffers), and
 * crh_embed_ln_packed -- the first call of a forward -- also launches a check of the whole array (row_off[0] == 0,
 * non-decreasing, every row <= Lmax, row_off[B] == T) whose verdict is reported as CRH_E_INVALID by the next packed entry
 * point called after the check has run, and in any case by crh_encoder_finish. */
int crh_embed_ln_packed(const int32_t *ids, const int32_t *row_off, const void *word, const void *pos, const void *type0,
                        const float *gamma, const float *beta, float eps, int pad_id, void *out, uint64_t *kmask, int B,
                        int T, int Lmax, int D, void *stream);
int crh_attn_fwd_packed(const void *qkv, const int32_t *row_off, const uint64_t *kmask, void *out, int B, int T, int Lmax,
                        int H, void *stream);
int crh_masked_mean_pool_packed(const void *tok, const int32_t *row_off, const uint64_t *kmask, float *sent, int B, int T,
                                int Lmax, int D, void *stream);
/* Waits for `stream` and returns the verdict of the device-side checks of the packed entry points launched on this device
 * since the last call (CRH_OK, or CRH_E_INVALID with the reason in crh_last_error) -- the sync point of a forward. */
int crh_encoder_finish(void *stream);

/* ------------------------------------------------------------- debug build only --------- */
/* Exported ONLY by libcoderag_hip_debug.so (code-rag_amd/build.sh compiles the same sources a second time with
 * -DCRH_ENABLE_DEBUG for tools/ and the kernel-selection tests); the product library has no crh_debug_* symbol. */
#ifdef CRH_ENABLE_DEBUG
/* Measurement support: launches the main scan's loads alone (same grid, same tile walk, same nt loads; no MFMA, no
 * candidates) over the whole corpus -- the HBM read rate this access pattern reaches on the device at hand, the ceiling
 * the scan's achieved GB/s is to be read against (tools/read_ceiling.py). */
int crh_debug_read_ceiling(crh_index *h, void *stream);

/* Measurement support: moves the int8 nomination copy of an index to a fresh device allocation (taken before the old one is
 * released) and marks it for requantisation -- lets one index try several places in HBM (tools/i8_places.py). */
int crh_debug_i8_move(crh_index *h);

/* Test support: what the int8 scan computes before it nominates, taken from the product's own launches (requantisation, query
 * preparation, the sample launch over every tile, the threshold launch) -- never a restatement of their arithmetic.  For up to
 * 64 raw queries (host, [nq][dim]) and the rows of an index of at most 8192 tiles (CRH_E_INVALID beyond; also when the index
 * does not nominate from its int8 copy at this k, or a search is pending):
 *   hi_rec [nq][rows]  upper end of each row's interval as the sample launch records it (bf16, rounded up)
 *   hi, lo [nq][rows]  both ends as f32, as the kernel evaluates them
 *   srow   [rows]      per-row scale;  qpar [64][4]: s_q, Qn, gn, 0 per query (zeros beyond nq);  dn, c_abs: one float each
 *   tau    [nq]        the threshold of each query for this k under the given filters (alive rows only)
 * All outputs are host pointers.  tests/test_i8_intervals_gpu.py. */
int crh_debug_i8_intervals(crh_index *h, int nq, const float *queries, int k, const crh_filter *filters, int n_filters,
                           float *hi_rec_out, float *hi_out, float *lo_out, float *srow_out, float *qpar_out, float *dn_out,
                           float *c_abs_out, float *tau_out);

/* Test support: the workgroup-wide selection helpers every returned id and score passes through (crh_kernels.hpp), called by
 * thin harness kernels with the product's own template arguments on key sets the caller supplies.  All pointers are host
 * pointers; bad arguments are CRH_E_INVALID and launch nothing.  tests/select_cases.py, tests/test_select_gpu.py.
 *
 * crh_debug_kth_largest: key_out[s] = the k[s]-th largest (1-based, 1 <= k[s] <= n) of keys[s][0..n), s < nsets.  `variant` is
 * one of the product's instantiations: CRH_DEBUG_SEL_FAST_* = wg_kth_largest_fast<NT, NB, 256> with NT = NB = 1024 / 512 / 256
 * (u32 keys; keys <= floor_key stay out of the bucket range), CRH_DEBUG_SEL_RADIX_* = wg_kth_largest<u32, NT> (floor_key
 * unused), and CRH_DEBUG_SEL_RADIX_1024 / _256 | CRH_DEBUG_SEL_U64 = wg_kth_largest<u64, NT> on u64 keys.  Workgroup b of
 * nblocks takes sets b, b + nblocks, ... one after the other on the same scratch.  CRH_E_INTERNAL when the threads of a
 * workgroup came back with different keys. */
#define CRH_DEBUG_SEL_FAST_1024 0
#define CRH_DEBUG_SEL_FAST_512 1
#define CRH_DEBUG_SEL_FAST_256 2
#define CRH_DEBUG_SEL_RADIX_1024 3
#define CRH_DEBUG_SEL_RADIX_512 4
#define CRH_DEBUG_SEL_RADIX_256 5
#define CRH_DEBUG_SEL_U64 8 /* or-ed in: the keys are 64 bits wide */
int crh_debug_kth_largest(int variant, const void *keys, unsigned nsets, unsigned n, const unsigned *k, unsigned floor_key,
                          unsigned nblocks, unsigned long long *key_out);

/* select_tail<1024> (CRH_DEBUG_TAIL_1024: k_select's) or select_tail<256> (CRH_DEBUG_TAIL_256: k_select_final's) on Ms keys
 * (ord(score) << 32) | ~row, unique apart from 0 = "no key": the top k (1..CRH_MAX_K) as scores_out [k] / rows_out [k] with
 * row_base added, padding (-inf, -1).  The keys are ranked out of LDS or by the general path by the kernels' own rule. */
#define CRH_DEBUG_TAIL_1024 0
#define CRH_DEBUG_TAIL_256 1
int crh_debug_select_tail(int variant, const unsigned long long *keys, unsigned Ms, int k, int64_t row_base, float *scores_out,
                          int64_t *rows_out);

/* The tile list of a row mask (the two launches a filtered search makes): the ascending numbers of the non-zero words of
 * mask_words [ntiles] into list_out, their count into *len_out.  list_out [ntiles] is read first -- it is what the list buffer
 * holds before the launches -- and copied back whole, so the caller sees what lies past the count. */
int crh_debug_tile_list(const uint32_t *mask_words, int64_t ntiles, uint32_t *list_out, uint32_t *len_out);

/* Timing ablations of the GEMM main loop (variant 0 = the real kernel; others skip a pipeline stage and return
 * garbage).  Development aid used by tools/gemm_ablate.py; not part of the product path. */
int crh_debug_gemm_variant(const void *x, const void *w, const float *bias, void *y, int T, int N, int K,
                           int variant, void *stream);

#endif /* CRH_ENABLE_DEBUG */

#ifdef __cplusplus
}
#endif
#endif /* CODERAG_HIP_H */
