/* include/bydb_gpu.h — C-ABI of the MI355X-native measure scan+aggregate
 * engine (libbydb_gpu.so).
 *
 * This is the drop-in boundary a Go host binds over cgo.  Each entry point
 * names the reference interface it replaces (apache/skywalking-banyandb):
 *
 *  - session/configure/consume/finalize mirror the lifecycle of
 *    vectorized.BreakerOperator (pkg/query/vectorized/operator.go:65-70:
 *    Init / Consume / Finalize / NextBatch / Close) as built for
 *    BatchAggregation by BuildOperators
 *    (pkg/query/vectorized/measure/plan.go:61-131) — one session per
 *    pipeline, sticky errors, Close releases everything.
 *  - part upload replaces the storage seam
 *    model.MeasureBatchResult.PullBatch (pkg/query/model/batch.go:45-55) +
 *    blockCursor.loadData/block.mustReadFrom (banyand/measure/block.go:818,
 *    324): instead of decoding on the host, the encoded block streams are
 *    made resident in HBM and decode+fold happens in HIP kernels.
 *  - the partial layout mirrors aggregation.Partial[N]
 *    (pkg/query/aggregation/aggregation.go:36-55) with MEAN's count sidecar
 *    (vectorized/measure/aggregation.go meanCountSuffix) and AggModeMap /
 *    AggModeReduce semantics (aggregation.go:57-64).
 *
 * Plain pointers and sizes only; no torch types.  See INTEGRATION.md for
 * the cgo binding a BanyanDB maintainer would add.
 */
#ifndef BYDB_GPU_H
#define BYDB_GPU_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* EncodeType — pkg/encoding/encoding.go:86-98 */
enum {
    BYDB_ENC_UNKNOWN = 0,
    BYDB_ENC_CONST = 1,
    BYDB_ENC_DELTA_CONST = 2,
    BYDB_ENC_DELTA = 3,
    BYDB_ENC_DELTA_OF_DELTA = 4,
    BYDB_ENC_CONST_WV = 5,
    BYDB_ENC_DELTA_CONST_WV = 6,
    BYDB_ENC_DELTA_WV = 7,
    BYDB_ENC_DELTA_OF_DELTA_WV = 8,
    BYDB_ENC_PLAIN = 9,
    BYDB_ENC_DICTIONARY = 10,
};

/* ValueType — pkg/pb/v1/valuetype */
enum { BYDB_VT_INT64 = 2, BYDB_VT_FLOAT64 = 3 };

/* AggFunc — pkg/query/vectorized/measure/aggregation.go:95-107 */
enum {
    BYDB_AGG_SUM = 0,
    BYDB_AGG_COUNT = 1,
    BYDB_AGG_MIN = 2,
    BYDB_AGG_MAX = 3,
    BYDB_AGG_MEAN = 4,
};

/* AggMode — vectorized/measure/aggregation.go:57-64 */
enum { BYDB_MODE_ALL = 0, BYDB_MODE_MAP = 1, BYDB_MODE_REDUCE = 2 };

/* Status codes (0 = ok).  Sticky per session, mirroring the operator's
 * sticky Go error contract. */
enum {
    BYDB_OK = 0,
    BYDB_ERR = -1,
    BYDB_ERR_HIP = -2,
    BYDB_ERR_BAD_ARG = -3,
    BYDB_ERR_BAD_DATA = -4,
    BYDB_ERR_STATE = -5,
    BYDB_ERR_NO_GPU = -6,
    BYDB_ERR_OOM = -7,
};

/* One (series, block) entry of the resident part directory.  Field
 * semantics follow blockMetadata + timestampsMetadata + columnMetadata
 * (banyand/measure/block_metadata.go:254-311, column_metadata.go:47-52):
 * the column payload headers ([type][exp][firstValue], column.go:183-263)
 * are parsed at load time on the host, so kernels see pure streams. */
typedef struct {
    uint64_t series_id;
    uint32_t count;               /* rows in block, <= 8192 (measure.go:41-46) */
    uint8_t ts_enc_with_version;  /* timestampsMetadata.encodeType */
    uint8_t version_enc;
    uint8_t field_enc;            /* common EncodeType of the field column */
    uint8_t field_vtype;          /* BYDB_VT_* */
    int64_t ts_min;               /* == first timestamp (block ascending) */
    int64_t ts_max;
    int64_t version_first;
    int64_t field_first;          /* decoded firstValue of the field column */
    int16_t exp;                  /* float64 decimal exponent (float.go:69) */
    uint8_t _pad[6];
    uint64_t ts_off;              /* ts varint stream (header-free) */
    uint64_t ts_len;
    uint64_t field_off;           /* field varint stream (header-free) */
    uint64_t field_len;
    uint64_t tag_off;             /* tag column payload incl. type byte, or 0 */
    uint64_t tag_len;             /* slot 0; slots 1-2 below (conjunctive) */
    uint64_t tag2_off;
    uint64_t tag2_len;
    uint64_t tag3_off;
    uint64_t tag3_len;
    uint32_t group_code;          /* dense group index (group-by), else 0 */
    uint32_t _pad2;
} bydb_block_desc;

/* Dense per-group partial accumulator — one slot per group.
 * sum_i/count are exact (wrapping) int64; min/max are on the int64 domain
 * (for float64 fields these are the decimal-int min/max, restored to
 * float64 at finalize — restore is monotone, float.go:69-102); sum_f is
 * the float64 mantissa sum (double).                                      */
typedef struct {
    int64_t sum_i;
    int64_t count;
    int64_t min_i;
    int64_t max_i;
    double sum_f;
    double _pad;
} bydb_partial;

/* Finalised per-group result (AggModeAll shape). */
typedef struct {
    int64_t sum_i;
    double sum_f;
    int64_t count;
    int64_t min_i;
    int64_t max_i;
    double min_f;
    double max_f;
    int64_t mean_i;   /* meanFunc.Val with the >=1 clamp (function.go:30-45) */
    double mean_f;
} bydb_result;

typedef struct bydb_session bydb_session;

/* ---- session lifecycle (BreakerOperator Init/Close) ---- */
bydb_session *bydb_session_create(int device);
void bydb_session_destroy(bydb_session *s);
const char *bydb_last_error(bydb_session *s);

/* ---- part residency (storage seam) ----
 * reserve once, then append payload chunks + their block descs; offsets in
 * descs are absolute within the whole part payload. */
int bydb_part_reserve(bydb_session *s, uint64_t payload_bytes, int64_t n_blocks);
int bydb_part_append(bydb_session *s, const uint8_t *payload, uint64_t len,
                     const bydb_block_desc *blocks, int64_t n_blocks);
int bydb_part_clear(bydb_session *s);

/* ---- aggregation configure (BuildOperators / AggSpec) ----
 * funcs: bitmask of (1<<BYDB_AGG_*); n_groups >= 1 (1 = scalar aggregate,
 * matching aggAllIterator).  field_vtype selects int64/float64 semantics. */
int bydb_agg_configure(bydb_session *s, int field_vtype, uint32_t func_mask,
                       uint32_t n_groups, int mode);

/* Optional: accumulate partials into an external device buffer of
 * n_groups * sizeof(bydb_partial) bytes (e.g. a torch CUDA tensor for an
 * RCCL merge).  Pass NULL to use the session's own buffer. */
int bydb_set_partials_buffer(bydb_session *s, void *dev_ptr, uint64_t len);

/* ---- consume (BreakerOperator.Consume over the resident part) ----
 * min_ts/max_ts: inclusive row clamp (timestamp.FindRange,
 * pkg/timestamp/range.go:143-170).  pred: optional tag-equality predicate
 * value bytes on tag slot 0 (dictionary or plain column), pred_len 0 =
 * none.  The EQ-only form of bydb_consume_filter below: one BYDB_OP_EQ
 * string condition.  Asynchronous: returns after launch; bydb_finalize
 * syncs. */
int bydb_consume(bydb_session *s, int64_t min_ts, int64_t max_ts,
                 const uint8_t *pred, uint64_t pred_len);

/* Conjunctive multi-tag predicate (<=3 values; preds[i] applies to the
 * block's tag slot i).  pred_lens[i] == 0 disables slot i (preds[i] may
 * then be NULL).  The EQ-only form of bydb_consume_filter below: one
 * BYDB_OP_EQ string condition per enabled slot, resolved by the same
 * stage.  BYDB_ERR_BAD_ARG when n_preds is outside 0..3. */
int bydb_consume_multi(bydb_session *s, int64_t min_ts, int64_t max_ts,
                       const uint8_t *const *preds, const uint64_t *pred_lens,
                       int n_preds);

/* ---- tag filter operators (measure query conditions) ----
 * The reference builds one TagFilter per modelv1.Condition in parseFilter
 * (pkg/query/logical/tag_filter.go:144-193).  The eight operators that
 * apply to scalar string and int tags are pushed down here; HAVING,
 * NOT_HAVING (array tags) and MATCH (analyzed text) stay with the host.
 * BYDB_OP_* carry the numeric values of modelv1.Condition.BinaryOp
 * (api/proto/banyandb/model/v1/query.proto:54-65).
 *
 * A tag value is a byte string or nil.  A nil dictionary entry / plain row
 * has stored length 0; a block with no column on the slot is all-nil.  The
 * empty string is a real value, distinct from nil.
 *
 *   op      matches a value v                                  nil row
 *   EQ      bytes(v) == literal  (eqTag.Match, :426-432;       false
 *           nullLiteral.Equal is false)
 *   NE      notTag(eqTag): !EQ   (:168, :370-376)              TRUE
 *   IN      v equals any list element (inTag.Match :405-411,   false
 *           BelongTo, expr_literal.go:84-92, 260-268)
 *   NOT_IN  notTag(inTag): !IN   (:189)                        TRUE
 *   GT      c < 0    with c = literal.Compare(v)               false
 *   GE      c <= 0   (rangeTag.Match, :465-503; Compare        false
 *   LT      c > 0     returns ok=false on nil, which           false
 *   LE      c >= 0    rejects the row)                         false
 *
 * Compare, string type: strings.Compare — bytewise lexicographic, a proper
 * prefix sorts first (expr_literal.go:241-246).  Compare, int type:
 * int(lit - val) with Go's WRAPPING int64 subtraction
 * (expr_literal.go:65-70): both 8-byte sign-flip cells (convert/
 * number.go:33-46) are decoded to int64, subtracted in uint64, and the
 * sign of the difference decides — so pairs more than 2^63 apart take the
 * reference's wrapped answer, not the mathematical one.  A stored value
 * that is not 8 bytes long never matches an int range.  Int literals are
 * passed as the stored 8-byte cell; EQ/NE/IN/NOT_IN compare cells by
 * bytes for both tag types.
 *
 * bydb_consume_filter ANDs its conditions (andLogicalNode); several may
 * target one slot (200 <= code < 300 is two).  AND / OR criteria trees over
 * the same conditions go through bydb_consume_filter_tree below. */
enum {
    BYDB_OP_EQ = 1,
    BYDB_OP_NE = 2,
    BYDB_OP_LT = 3,
    BYDB_OP_GT = 4,
    BYDB_OP_LE = 5,
    BYDB_OP_GE = 6,
    BYDB_OP_IN = 9,
    BYDB_OP_NOT_IN = 10,
};

/* tag type of a condition's literal(s) — databasev1.TagType scalar kinds */
enum { BYDB_TAG_STRING = 1, BYDB_TAG_INT = 2 };

#define BYDB_FILTER_MAX_CONDS 8      /* conditions per call */
#define BYDB_FILTER_MAX_VALUES 4096  /* literal values per call, all conds */

typedef struct {
    int32_t slot;                /* block tag slot 0-2 */
    int32_t op;                  /* BYDB_OP_* */
    int32_t tag_type;            /* BYDB_TAG_* */
    uint32_t n_values;           /* IN / NOT_IN: >= 1; every other op: 1 */
    const uint8_t *values;       /* concatenated literal bytes */
    const uint64_t *value_offs;  /* n_values + 1 prefix offsets into values */
} bydb_tag_cond;

/* Scan with ANDed tag conditions.  Same asynchronous and sticky-error
 * contract as the equality entry points above; n_conds == 0 is an
 * unfiltered scan.  BYDB_ERR_BAD_ARG (session stays usable) when n_conds
 * is outside 0..BYDB_FILTER_MAX_CONDS, a slot / op / tag type is unknown,
 * IN / NOT_IN carry no value, another op carries other than exactly one,
 * an int-typed GT / GE / LT / LE literal is not 8 bytes, or the call
 * carries more than BYDB_FILTER_MAX_VALUES values in total. */
int bydb_consume_filter(bydb_session *s, int64_t min_ts, int64_t max_ts,
                        const bydb_tag_cond *conds, int n_conds);

/* ---- AND / OR criteria trees over tag conditions ----
 * BuildTagFilter (pkg/query/logical/tag_filter.go:84-142) turns a
 * modelv1.Criteria into a binary tree of andLogicalNode / orLogicalNode
 * over the per-condition filters above.  A node's Match is isMatch
 * (:259-274): its children are evaluated left to right and folded with the
 * node's merge — andLogicalNode.merge (:288-295) is true when every input
 * is, orLogicalNode.merge (:323-330) when any input is.  Leaves keep their
 * own nil rule under either node: NE / NOT_IN are true on a nil row, so
 * `NE x OR ...` selects every nil row, and `EQ x OR NE y` selects a nil row
 * through its right leaf.
 *
 * The reference drops DummyFilter children (conditions on entity tags it
 * resolves through the series index, skipped tag names) before the tree is
 * built: logicalNode.append ignores them (:251-257), and a node whose two
 * children are both dummy is itself dummy (:124-126).  A host does the
 * same before calling: a node left with one child is replaced by that
 * child, so the tree passed here is a proper binary tree over the
 * conditions that remain.  Trees with more than BYDB_FILTER_MAX_CONDS
 * leaves stay on the host.
 *
 * Encoding: `nodes` is the tree in post-order — both children of a node
 * have smaller indices than the node, the root is the last node.  A LEAF's
 * `left` is an index into `conds` (`right` is unused, 0); an AND / OR
 * node's `left` / `right` are node indices.  n_nodes == 2 * n_conds - 1,
 * every condition is referenced by exactly one leaf and every node but the
 * root by exactly one parent.  BYDB_NODE_AND / BYDB_NODE_OR carry the
 * values of modelv1.LogicalExpression.LogicalOp (query.proto:93-95). */
enum { BYDB_NODE_LEAF = 0, BYDB_NODE_AND = 1, BYDB_NODE_OR = 2 };

typedef struct {
    int32_t op;     /* BYDB_NODE_* */
    int32_t left;   /* LEAF: condition index; AND / OR: node index */
    int32_t right;  /* LEAF: unused (0);      AND / OR: node index */
} bydb_filter_node;

/* Scan under a criteria tree.  Same asynchronous and sticky-error contract
 * as bydb_consume_filter, and the same rules for every condition;
 * n_conds == 0 with n_nodes == 0 is an unfiltered scan.  BYDB_ERR_BAD_ARG
 * (session stays usable) when n_conds is outside
 * 1..BYDB_FILTER_MAX_CONDS, n_nodes != 2 * n_conds - 1, a node's op is
 * unknown, a child index is not below its parent's, a condition is
 * referenced twice or never, or a node has two parents.  A tree without an
 * OR node takes exactly the bydb_consume_filter path.  A tree with one
 * waits once for its resolve stage (to size the row-bitmap arena) before
 * the scan is launched; the scan itself stays asynchronous. */
int bydb_consume_filter_tree(bydb_session *s, int64_t min_ts, int64_t max_ts,
                             const bydb_tag_cond *conds, int n_conds,
                             const bydb_filter_node *nodes, int n_nodes);

/* Pure host, no GPU: validate the tree (rules above) and write its truth
 * table.  Bit `sig` of the 256-bit table (word sig >> 6, bit sig & 63) is
 * the tree's result when condition i evaluates to bit i of `sig`; bits at
 * and above 2^n_conds are zero.  The device evaluates trees through this
 * table alone.  BYDB_OK or BYDB_ERR_BAD_ARG. */
int bydb_filter_tree_table(const bydb_filter_node *nodes, int n_nodes,
                           int n_conds, uint64_t table[4]);

/* How the blocks of the last bydb_consume_filter_tree call resolved:
 * out[0] every row matches (folded unpredicated), out[1] no row matches
 * (skipped), out[2] walked through one slot's dictionary code mask, out[3]
 * walked through a per-row match bitmap.  All zero after a tree without an
 * OR node (the bydb_consume_filter path keeps no census) and after an
 * unfiltered scan. */
int bydb_filter_tree_stats(bydb_session *s, uint64_t out[4]);

/* ---- cross-part version dedup (the measure query's merge) ----
 * bydb_part_append accepts blocks from any number of on-disk parts.  When
 * the same (seriesID, timestamp) appears in more than one of them — a
 * re-sent data point, or a late correction flushed into a newer part that
 * is not merged yet — the reference's measure query keeps exactly one row,
 * the one with the highest version: for equal series and timestamp
 * queryResult.Less orders versions descending, queryResult.merge copies the
 * first row and lets a later row of the same timestamp replace it only when
 * its version is greater than lastVersion (banyand/measure/
 * query.go:913-943, 966-1026; TestQueryResult "multiple parts with
 * duplicated data ...", query_test.go:61-1234).
 *
 * With row dedup on, a row (series_id, ts, version) of block b (b = block
 * index in append order) is SUPERSEDED when another resident row has the
 * same series_id and ts and either a greater version, or an equal version
 * and a smaller block index.  Exactly one row per (series_id, ts) survives.
 * The equal-version tie is unspecified in the reference (the heap order of
 * equal keys is arbitrary); "the earliest appended block wins" is this
 * engine's choice.
 *
 * Superseded rows do not exist for the rest of the query.  They are removed
 * BEFORE tag conditions are evaluated, as the reference's merge sits below
 * its filter: a higher-versioned row that fails the filter still hides the
 * lower-versioned row that would have passed.  They contribute no group
 * key, and a block whose rows are all superseded is a skipped block.
 * Duplicates inside one block are the part builder's job (part.go:178,
 * 192-198); blocks of different series never interact.
 *
 * Which rows survive is derived state over the resident part: it is built
 * on the first consume with dedup on (that consume waits once for the
 * build) and rebuilt after bydb_part_reserve / bydb_part_append.  A part
 * without overlapping blocks, or without superseded rows, scans exactly as
 * with dedup off.  A partially superseded block is scanned through a
 * per-row bitmap predicate, so the bydb_group_first_seen caveat for bitmap
 * predicates inside row-varying group merges applies to it. */

/* Sticky per session, default 0 (off: nothing in the session changes).
 * BYDB_ERR_BAD_ARG (session stays usable) for any value but 0 or 1.  If
 * the build cannot allocate its device arenas, the consume returns
 * BYDB_ERR_OOM naming the size and dedup is turned off. */
int bydb_set_row_dedup(bydb_session *s, int on);

/* What the build found (query.go:913-943, 966-1026 applied to the resident
 * part): out[0] blocks that overlap at least one other block of their
 * series, out[1] blocks with some but not all rows superseded, out[2]
 * blocks with every row superseded, out[3] rows superseded.  Valid after
 * the first consume with dedup on; all zero before that and whenever dedup
 * is off. */
int bydb_row_dedup_stats(bydb_session *s, uint64_t out[4]);

/* Pure host, no GPU, no session: the overlap planner the device stage is
 * driven by (the blocks whose cursors the reference's heap could ever
 * compare, query.go:913-943).  Two blocks are peers when they have the
 * same series_id and their [ts_min, ts_max] ranges intersect, both ends
 * inclusive.  Output is a symmetric CSR: block i's peers are
 * peers[peer_offs[i] .. peer_offs[i + 1]), ascending by block index.
 * peer_offs (n_blocks + 1 entries) and *n_peers are always written;
 * BYDB_ERR_OOM when peers_cap < *n_peers (peers is then untouched, so a
 * first call with peers_cap 0 sizes the list), BYDB_ERR_BAD_ARG on null
 * outputs. */
int bydb_row_dedup_peers(const bydb_block_desc *blocks, int64_t n_blocks,
                         uint64_t *peer_offs /* n_blocks + 1 */,
                         uint32_t *peers, uint64_t peers_cap,
                         uint64_t *n_peers);

/* ---- finalize + emit (Finalize/NextBatch) ----
 * Syncs the stream, downloads partials and finalises per-group results
 * (MEAN = sum/count with the >=1 clamp; float64 restore per float.go).
 * out must hold n_groups entries.  Resets partials for the next epoch. */
int bydb_finalize(bydb_session *s, bydb_result *out, int64_t n_groups);

/* Finalize partials only (AggModeMap: emit Partial state for an external
 * reduce — e.g. RCCL — without applying Val()).  Leaves device partials
 * in the accumulation buffer; host copy written to out. */
int bydb_finalize_partials(bydb_session *s, bydb_partial *out, int64_t n_groups);

/* Reset accumulators to the fold identity (Map.Reset, function.go). */
int bydb_reset(bydb_session *s);

/* Per-group first-seen keys ((item << 13) | row in storage order; ~0 =
 * group never entered).  Sorting group ids by these keys reproduces the
 * reference's first-seen group materialisation order (computeKey creates
 * groups in row-iteration order, vectorized/measure/aggregation.go:523),
 * so the Go twin can emit NextBatch rows in reference order from the
 * host-domain result buffers.  out holds n_groups entries. */
int bydb_group_first_seen(bydb_session *s, uint64_t *out, int64_t n_groups);

/* Combine external partials (AggModeReduce Combine semantics,
 * aggregation_reduce.go:120-138) into results on the host.  parts is
 * [n_parts_per_group][n_groups]; float_exp selects the float64 restore
 * domain (BYDB_FLOAT_RAW_EXP = raw IEEE-754 cells). */
int bydb_reduce_partials2(const bydb_partial *parts, int64_t n_parts_per_group,
                          int64_t n_groups, int field_vtype, int16_t float_exp,
                          bydb_result *out);

/* How the closed-form scan (sum/count, no predicate, no tag group-by) loads
 * the dense one-byte delta streams.  CACHED: plain loads, every line is
 * installed in the caches — right for a part small enough to stay resident
 * in the last-level cache between passes.  STREAMING: non-temporal loads —
 * right for a read-once pass over a part larger than that cache.  AUTO (the
 * default) picks STREAMING when the resident payload exceeds the cache
 * (256 MiB), CACHED otherwise.  Results do not depend on the policy.
 * BYDB_ERR_BAD_ARG (session stays usable) for any other value. */
enum {
    BYDB_STREAM_AUTO = 0,
    BYDB_STREAM_CACHED = 1,
    BYDB_STREAM_STREAMING = 2,
};
int bydb_set_stream_policy(bydb_session *s, int policy);

/* What `policy` resolves to for a resident payload of payload_bytes:
 * BYDB_STREAM_CACHED or BYDB_STREAM_STREAMING (host-only, no session), or
 * BYDB_ERR_BAD_ARG for an unknown policy. */
int bydb_stream_policy_pick(int policy, uint64_t payload_bytes);

/* ---- nibble-packed dense field streams ----
 * A dense one-byte delta stream whose deltas all lie in [-8, 7] (zigzag
 * bytes <= 15) carries four bits per byte.  Parts are immutable and stay
 * resident, so the session keeps a 4-bit copy of such streams and the
 * closed-form streaming scan (sum/count, no predicate, no tag group-by,
 * the kernels BYDB_STREAM_STREAMING selects) reads it in place of the byte
 * stream for every block it folds whole: half the bytes.  A block cut by
 * the timestamp clamp, and every other kind of scan, reads the byte stream.
 * Results do not depend on the mode.
 *
 * The copy is derived state over the resident part, like the dedup
 * survivors: built on the first consume that reads it (that consume waits
 * once for the build), rebuilt after bydb_part_reserve / bydb_part_append,
 * freed by bydb_part_reserve, by a change of mode and with the session.  It
 * costs device memory: up to half the dense
 * field bytes again, plus four bytes per block.
 *
 * A block is a CANDIDATE when field_enc == BYDB_ENC_DELTA, 2 <= count <=
 * 8192, field_len == count - 1 and the field stream is not in the sidecar.
 * Every candidate gets a slot; the build fills it if every byte of the
 * stream is <= 15, otherwise the block stays unpacked and the slot is
 * wasted.
 *
 * AUTO (default): pack when the stream-load policy resolves to streaming
 * for the session (bydb_stream_policy_pick(...) == BYDB_STREAM_STREAMING);
 * a part that fits the last-level cache is bound by a memory round trip,
 * not by bandwidth.  If the arena cannot be allocated the scan reads the
 * byte streams: no error, and the stats show no packed block.
 * OFF: never read (and never build) the copy.
 * A call that changes the mode frees the copy; the first consume that reads
 * packed data under the new mode builds it again.
 * ON: pack for any size; the closed-form scan then takes the streaming
 * kernels whatever the stream-load policy says, since only they read packed
 * data.  If the arena cannot be allocated the consume returns BYDB_ERR_OOM
 * naming the size; the session stays usable, unpacked.
 * BYDB_ERR_BAD_ARG (session stays usable) for any other value. */
enum { BYDB_PACK_AUTO = 0, BYDB_PACK_OFF = 1, BYDB_PACK_ON = 2 };
int bydb_set_field_pack(bydb_session *s, int mode);

/* What the build did: out[0] candidate blocks, out[1] packed blocks, out[2]
 * packed payload bytes (ceil((count-1)/2) per packed block), out[3] bytes
 * of the slot arena (the slot table's 4 bytes per block come on top).
 * Valid after the first consume that built the copy; all zero before that,
 * whenever the current mode and stream-load policy would not read packed
 * data (OFF; AUTO on a part the policy resolves to cached), and out[1..3]
 * when nothing could be packed. */
int bydb_field_pack_stats(bydb_session *s, uint64_t out[4]);

/* Pure host, no GPU, no session: the slot planner of the build.  Candidate
 * block i gets slot_len[i] = ceil((count-1)/2) rounded up to a multiple of
 * 128 bytes at slot_off[i], a multiple of 128; slots are laid end to end in
 * block order, so they are pairwise disjoint and share no 128-byte memory
 * line, and a full 8192-row block takes exactly 4 KiB.  Other blocks get
 * slot_len 0 (slot_off 0).  *arena_bytes is the sum of the slots.
 * BYDB_ERR_BAD_ARG on null outputs. */
int bydb_field_pack_plan(const bydb_block_desc *blocks, int64_t n_blocks,
                         uint64_t *slot_off /* n_blocks */,
                         uint32_t *slot_len /* n_blocks */,
                         uint64_t *arena_bytes);

/* Timing of the last consume's kernels in milliseconds (HIP events on the
 * session stream) — feeds bench.py's roofline.achieved. */
double bydb_last_consume_ms(bydb_session *s);

/* ---- host-side part builder (fixture writer) ----
 * Mirrors the reference block write path: mustInitFromDataPoints ->
 * block.mustWriteTo (block.go:60,139), mustWriteTimestampsTo
 * (block.go:386-404), column.mustWriteTo (column.go:157-278).  Pure host
 * code; no GPU needed.  Produces payload bytes + bydb_block_desc entries
 * whose encoded streams are byte-identical to the reference's (validated
 * against the oracle in tests/).                                          */
typedef struct bydb_part_builder bydb_part_builder;
bydb_part_builder *bydb_part_builder_create(void);
void bydb_part_builder_destroy(bydb_part_builder *b);
const char *bydb_part_builder_error(bydb_part_builder *b);

int bydb_part_builder_add_block_i64(bydb_part_builder *b, uint64_t series_id,
                                    const int64_t *ts, const int64_t *versions,
                                    const int64_t *vals, int64_t n,
                                    uint32_t group_code);
int bydb_part_builder_add_block_f64(bydb_part_builder *b, uint64_t series_id,
                                    const int64_t *ts, const int64_t *versions,
                                    const double *vals, int64_t n,
                                    uint32_t group_code);
/* Raw-float sentinel for bydb_set_float_exp / bydb_reduce_partials2:
 * sessions over null-bearing FLOAT64 columns (Plain IEEE-754 cell blocks,
 * convert/number.go:128-132) fold in the raw-bits domain — ordered-bit
 * min/max keys, direct double sums — selected by this exponent value.
 * Mixing raw and decimal float blocks in one session is a loud error. */
#define BYDB_FLOAT_RAW_EXP ((int16_t)-32768)

int bydb_part_builder_add_block_f64_nullable(
    bydb_part_builder *b, uint64_t series_id, const int64_t *ts,
    const int64_t *versions, const double *vals, const uint8_t *valid,
    int64_t n, uint32_t group_code);
/* null-bearing int64 column (valid[i]==0 -> row i null): stored as the
 * reference's Plain fallback — a bytes block of 8-B sign-flip cells with
 * nil rows zero-length (column.go:214-233, convert/number.go:33-46);
 * the fold skips nulls (vectorized/measure/aggregation.go:310) */
int bydb_part_builder_add_block_i64_nullable(
    bydb_part_builder *b, uint64_t series_id, const int64_t *ts,
    const int64_t *versions, const int64_t *vals, const uint8_t *valid,
    int64_t n, uint32_t group_code);
/* attach a dictionary-encoded tag column to the block just added:
 * tag value of row i = tag_values[codes[i]] (code order = first-seen) */
int bydb_part_builder_set_block_tag(bydb_part_builder *b, const uint8_t *data,
                                    const int64_t *lens, int64_t n);

uint64_t bydb_part_builder_payload_len(bydb_part_builder *b);
const uint8_t *bydb_part_builder_payload(bydb_part_builder *b);
int64_t bydb_part_builder_n_blocks(bydb_part_builder *b);
const bydb_block_desc *bydb_part_builder_blocks(bydb_part_builder *b);
/* drop payload bytes + descs already consumed, keep absolute offsets
 * running (chunked upload) */
int bydb_part_builder_drain(bydb_part_builder *b);

/* ---- synthetic workload generator (BASELINE.json section 8d) ----
 * Generates one series' datapoints and appends its blocks (<=8192 rows
 * each).  values = base + i*ramp + noise, noise in [-3,3] from
 * splitmix64(seed ^ series_index).  threads: host threads for encoding. */
int bydb_gen_series_i64(bydb_part_builder *b, uint64_t series_index,
                        int64_t n_dp, int64_t t0, int64_t stride_ns,
                        int64_t base, int64_t ramp, uint64_t seed,
                        uint32_t group_code);
int bydb_gen_series_f64(bydb_part_builder *b, uint64_t series_index,
                        int64_t n_dp, int64_t t0, int64_t stride_ns,
                        double base, double ramp, uint64_t seed,
                        uint32_t group_code);
/* bulk generators: n_series consecutive series (first_index ...) encoded
 * on `threads` host threads; base = series_index * base_step.
 * group_mod > 0 assigns group_code = series_index %% group_mod. */
int bydb_gen_series_bulk_i64(bydb_part_builder *b, uint64_t first_index,
                             int64_t n_series, int64_t n_dp, int64_t t0,
                             int64_t stride_ns, int64_t base_step, int64_t ramp,
                             uint64_t seed, uint32_t group_mod, int threads);
int bydb_gen_series_bulk_f64(bydb_part_builder *b, uint64_t first_index,
                             int64_t n_series, int64_t n_dp, int64_t t0,
                             int64_t stride_ns, double base_step, double ramp,
                             uint64_t seed, uint32_t group_mod, int threads);
/* entity-tag table for the generators: every generated block gets
 * values[series_index %% n_values] as a constant tag column in `slot`.
 * data = concatenated values; lens[i] < 0 marks a nil value. */
int bydb_part_builder_set_tag_table(bydb_part_builder *b, int slot,
                                    const uint8_t *data, const int64_t *lens,
                                    int64_t n_values);
/* raw helpers used by the part reader */
int bydb_part_builder_append_raw(bydb_part_builder *b, const uint8_t *data,
                                 uint64_t len);
int bydb_part_builder_append_desc(bydb_part_builder *b,
                                  const bydb_block_desc *d);

/* ---- per-row group-by on dictionary tag columns ----
 * computeKey/appendKeyComponent semantics (vectorized/measure/
 * aggregation.go:523 + groupby.go:287-364) with a host-supplied group
 * DOMAIN: dense group id = index into the domain value list (the host
 * layer controls materialisation order; the reference's is first-seen).
 * Nil or out-of-domain rows drop.  dom_blob = concatenated values,
 * dom_offs[n_values+1] prefix offsets. */
int bydb_agg_configure_by_tag(bydb_session *s, int field_vtype,
                              uint32_t func_mask, int tag_slot,
                              const uint8_t *dom_blob,
                              const uint64_t *dom_offs, uint32_t n_values,
                              int mode);
/* composite key over up to 3 tag slots: gid = g0 + n0*g1 + n0*n1*g2 */
int bydb_agg_configure_by_tags(bydb_session *s, int field_vtype,
                               uint32_t func_mask, const int *slots,
                               int n_slots, const uint8_t *const *dom_blobs,
                               const uint64_t *const *dom_offs,
                               const uint32_t *n_values, int mode);

/* ---- on-disk part directory (Appendix A; banyand/measure/part.go:37-56)
 * write_dir emits metadata.json / meta.bin / primary.bin / timestamps.bin
 * / fv.bin / <family>.tfm/.tf in the reference's exact layout; read_dir
 * loads a part directory (ours or the reference's) into a builder. */
int bydb_part_write_dir(bydb_part_builder *b, const char *path,
                        const char *field_name, const char *tag_family,
                        const char *const *tag_names, int n_tags);
int bydb_part_read_dir(bydb_part_builder *b, const char *path);

/* ---- columnar wire frame codec (egress / Map->Reduce transport) ----
 * Byte-stable layout per pkg/query/vectorized/frame (frame.go:26-95,
 * encode.go:42-170): magic "\0VFR", version, uvarint nrows/ncols, per
 * column [role, type, name, family, validity bitmap (1=null, LE
 * bit-packed), data (numeric = N x 8B LE; var = uvarint len + bytes)]. */
typedef struct bydb_frame_builder bydb_frame_builder;
typedef struct bydb_frame_reader bydb_frame_reader;
bydb_frame_builder *bydb_frame_builder_create(uint64_t nrows);
void bydb_frame_builder_destroy(bydb_frame_builder *b);
const char *bydb_frame_builder_error(bydb_frame_builder *b);
int bydb_frame_add_i64(bydb_frame_builder *b, uint8_t role, const char *name,
                       const char *family, const int64_t *vals,
                       const uint8_t *nulls);
int bydb_frame_add_f64(bydb_frame_builder *b, uint8_t role, const char *name,
                       const char *family, const double *vals,
                       const uint8_t *nulls);
int bydb_frame_add_str(bydb_frame_builder *b, uint8_t role, const char *name,
                       const char *family, const uint8_t *data,
                       const int64_t *lens);
int bydb_frame_add_bytes(bydb_frame_builder *b, uint8_t role, const char *name,
                         const char *family, const uint8_t *data,
                         const int64_t *lens);
/* minimal TagValue/FieldValue proto cells (raw_emit.go egress shape);
 * field_value selects FieldValue (type 6) over TagValue (type 5) */
int bydb_frame_add_tagvalue_str(bydb_frame_builder *b, uint8_t role,
                                const char *name, const char *family,
                                const uint8_t *data, const int64_t *lens,
                                int field_value);
int bydb_frame_add_tagvalue_int(bydb_frame_builder *b, uint8_t role,
                                const char *name, const char *family,
                                const int64_t *vals, const uint8_t *nulls,
                                int field_value);
int bydb_frame_finish(bydb_frame_builder *b);
uint64_t bydb_frame_len(bydb_frame_builder *b);
const uint8_t *bydb_frame_data(bydb_frame_builder *b);
bydb_frame_reader *bydb_frame_open(const uint8_t *data, uint64_t len);
void bydb_frame_close(bydb_frame_reader *r);
const char *bydb_frame_reader_error(bydb_frame_reader *r);
uint64_t bydb_frame_nrows(bydb_frame_reader *r);
uint64_t bydb_frame_ncols(bydb_frame_reader *r);
int bydb_frame_col_info(bydb_frame_reader *r, uint64_t ci, uint8_t *role,
                        uint8_t *type, char *name, uint64_t name_cap,
                        char *family, uint64_t family_cap);
int bydb_frame_col_null(bydb_frame_reader *r, uint64_t ci, uint64_t row);
int bydb_frame_col_i64(bydb_frame_reader *r, uint64_t ci, int64_t *out);
int bydb_frame_col_var(bydb_frame_reader *r, uint64_t ci, uint8_t *data_out,
                       uint64_t data_cap, int64_t *lens_out,
                       uint64_t *data_len);

/* ---- BatchTop ordering over group results ----
 * top.go:31-121 + ApplyTopToReduce (reduce.go:290): asc keeps the lowest
 * k (smallest first), desc the highest k; ties keep insertion order;
 * empty groups are nulls and sort lowest.  value_sel: 0 sum_i, 1 count,
 * 2 min_i, 3 max_i, 4 mean_i, 5 sum_f, 6 min_f, 7 max_f, 8 mean_f. */
int bydb_top_groups(const bydb_result *results, int64_t n_groups,
                    int value_sel, int64_t k, int asc, int64_t *out_idx,
                    int64_t *out_n);

/* ---- top-N data points by field value: raw-row BatchTop ----
 * A measure query's plan is Scan -> [GroupByAgg] -> [Top] -> Limit
 * (pkg/query/vectorized/measure/plan/analyzer.go:118-151).  With `top` and
 * no `agg`, measure.BatchTop runs over every data point the scan yields, in
 * one global heap (plan/top.go:28-46, top.go:30-199): a whole-result top-N,
 * "the 10 highest response times in the last hour where env = prod".  This
 * is that operator on the same seam (BreakerOperator Init / Consume /
 * Finalize / NextBatch): the session selects rows instead of folding them.
 *
 * Order contract (top.go:30-34, 66-82, 190-199): desc keeps the N highest,
 * highest first; asc the N lowest, lowest first.  Equal values surface in
 * input order and the earlier row wins a place.  Input order is storage
 * order, seq = (item << 13) | row — the key bydb_group_first_seen documents
 * as the reference's row-iteration order.
 *
 * Two limits of this version:
 *  - Null-bearing field blocks (BYDB_ENC_PLAIN cells) rank nulls lowest in
 *    the reference (top.go:95-105).  Here a top consume that selects any
 *    row of such a block is a loud device error (bydb_top_finalize returns
 *    BYDB_ERR_BAD_DATA); a null row is never dropped silently.  A Plain
 *    block the clamp or the filter leaves no row of is not an error.
 *    Raw-float sessions (BYDB_FLOAT_RAW_EXP) consist of such blocks and are
 *    out of scope.
 *  - float64 keys are compared as decimal mantissas rescaled exactly to the
 *    session exponent (the rescale the min/max aggregates use; an overflow
 *    is the same loud device error).  The reference compares restored
 *    doubles, so two different decimals that round to the same double tie
 *    there and are ordered by their decimals here.  That needs mantissas
 *    beyond 2^53. */
#define BYDB_TOP_ROWS_MAX 1024
typedef struct {
    uint64_t series_id;
    int64_t  ts;
    int64_t  version;
    int64_t  value_i;   /* int64 field: the value; float64 field: the row's
                           decimal mantissa in its own block's exponent */
    double   value_f;   /* float64 field: restore(value_i, block exp), the
                           same restore finalize applies (float.go:69-102);
                           int64 field: 0 */
    uint64_t seq;       /* (item << 13) | row, storage order */
} bydb_top_row;         /* 48 bytes */

/* BuildOperators' Top stage (plan/top.go:28-46) in place of
 * BatchAggregation: makes the session a BatchTop operator over raw rows; a
 * later bydb_agg_configure* switches it back.  BYDB_ERR_BAD_ARG (session
 * stays usable, configuration unchanged) when n < 0, n > BYDB_TOP_ROWS_MAX,
 * field_vtype is not int64 / float64, or the session exponent is
 * BYDB_FLOAT_RAW_EXP (also checked by the consume).  n == 0 is legal and
 * the reference's no-op (top.go:152-157): consume launches nothing,
 * finalize returns 0 rows.  For float64 fields the session exponent
 * (bydb_set_float_exp) means what it means for aggregates: the part's
 * minimum exponent, the domain every key is compared in.
 *
 * Every consume entry point (bydb_consume, _multi, _filter, _filter_tree,
 * with or without bydb_set_row_dedup) then selects under exactly the
 * aggregate path's rules: clamp, skip verdicts, code-mask and bitmap
 * walkers, dedup survivors removed before the filter (BatchTop.Consume,
 * top.go:152-188).  One consume per epoch: a second one before
 * bydb_top_finalize or bydb_reset is BYDB_ERR_STATE.  bydb_last_consume_ms
 * reports the event-timed span of all top kernels. */
int bydb_top_configure(bydb_session *s, int field_vtype, int64_t n, int asc);

/* BatchTop.Finalize / NextBatch (top.go:190-199): syncs, then writes
 * min(n, selected rows) rows sorted by (value, then seq ascending) and
 * their count to *out_n, and closes the epoch.  BYDB_ERR_OOM when cap is
 * smaller than that count: *out_n holds the needed count and the epoch
 * stays open.  BYDB_ERR_STATE when the session is not a top session,
 * BYDB_ERR_BAD_DATA on a device error (sticky until bydb_reset). */
int bydb_top_finalize(bydb_session *s, bydb_top_row *out, int64_t cap,
                      int64_t *out_n);

/* Pure host, no GPU, no session: the reduce side for time-bucket shards
 * (ApplyTopToReduce, reduce.go:290, over raw rows) — a stable N-way merge
 * of per-shard bydb_top_finalize results.  On equal values the earlier
 * list wins, then the smaller seq.  int64 rows compare by value_i; float64
 * rows by value_f, as the reference does (shards restore in their own
 * exponents).  out holds min(n, total rows) rows and must not alias a
 * list.  BYDB_ERR_BAD_ARG on null outputs, negative counts or an unknown
 * field_vtype. */
int bydb_top_rows_merge(const bydb_top_row *const *lists, const int64_t *lens,
                        int n_lists, int field_vtype, int64_t n, int asc,
                        bydb_top_row *out, int64_t *out_n);

/* ---- time-ordered rows with offset and limit: Scan -> Limit ----
 * With neither `agg` nor `top` a measure query's plan is Scan -> Limit
 * (pkg/query/vectorized/measure/plan/analyzer.go:118-157): "the 100 latest
 * data points of these series in the last hour where env = prod", or "rows
 * 200..299 in time order".  In the reference that is two pieces.
 * queryResult's heap merges the block cursors of all parts
 * (banyand/measure/query.go:913-943, 962-1026): by timestamp (orderByTS,
 * ascending by default; SORT_DESC walks the cursors backwards, :286-296),
 * equal timestamps by seriesID ascending, and equal (series, timestamp)
 * keeps only the highest version.  BatchLimit then keeps rows
 * [offset, offset + limit) of that stream (limit.go:81-108).  This is both
 * on the operator seam of the top-N section: the session selects rows
 * instead of folding them.
 *
 * Order contract, a total order on the selected rows: (ts in the requested
 * direction, series_id ascending, seq ascending), seq = (item << 13) | row.
 * ts compares as a signed 64-bit value, series_id as an unsigned one.
 *  - With bydb_set_row_dedup(s, 1), (series_id, ts) is unique among the
 *    selected rows, so the order is exactly the reference's:
 *    queryResult.Less gives the first two components and merge keeps the
 *    highest version.
 *  - With row dedup off, every resident duplicate surfaces, in seq order
 *    after (ts, series_id).  The reference always dedups in its merge; this
 *    is this engine's rule for the off case.
 *
 * One limit, kept from top-N: a consume that selects any row of a
 * null-bearing field block (BYDB_ENC_PLAIN cells) is a loud device error
 * (bydb_rows_finalize returns BYDB_ERR_BAD_DATA); a null is never returned
 * as a value.  A Plain block the clamp or the filter leaves no row of is
 * not an error.  Raw-float sessions (BYDB_FLOAT_RAW_EXP) consist of such
 * blocks and are out of scope. */
enum { BYDB_ORDER_TS_ASC = 0, BYDB_ORDER_TS_DESC = 1 };

/* BuildOperators' plan without GroupByAgg and Top (analyzer.go:118-157):
 * makes the session a row-scan operator that keeps rows
 * [offset, offset + limit) of the ordered selection (NewBatchLimit,
 * limit.go:40-53); a later bydb_agg_configure* or bydb_top_configure
 * switches it back.  BYDB_ERR_BAD_ARG (session stays usable, configuration
 * unchanged) when offset < 0, limit < 0, offset + limit >
 * BYDB_TOP_ROWS_MAX, order is not one of BYDB_ORDER_TS_*, field_vtype is
 * not int64 / float64, or the session exponent is BYDB_FLOAT_RAW_EXP (also
 * checked by the consume).  limit == 0 is legal: consume launches nothing,
 * finalize returns 0 rows; substituting the analyzer's defaultLimit
 * (analyzer.go:153-157) is the host's job.  field_vtype names the field
 * whose value each row carries; for float64 the session exponent
 * (bydb_set_float_exp) is the part's minimum exponent, as for aggregates.
 *
 * Every consume entry point (bydb_consume, _multi, _filter, _filter_tree,
 * with or without bydb_set_row_dedup) then selects under exactly the
 * aggregate path's rules: clamp, skip verdicts, code-mask and bitmap
 * walkers, dedup survivors removed before the filter.  One consume per
 * epoch: a second one before bydb_rows_finalize or bydb_reset is
 * BYDB_ERR_STATE.  bydb_last_consume_ms reports the event-timed span of all
 * row-scan kernels. */
int bydb_rows_configure(bydb_session *s, int field_vtype,
                        int64_t offset, int64_t limit, int order);

/* BatchLimit.Process over the merged stream (limit.go:81-108): syncs, then
 * writes rows [offset, offset + limit) of the ordered selection — fewer, or
 * none, when the selection is shorter — and their count to *out_n, and
 * closes the epoch.  Every field of bydb_top_row is filled as
 * bydb_top_finalize fills it: value_i is the row's value (float64: its
 * decimal mantissa in its own block's exponent), value_f the restore of
 * that.  BYDB_ERR_OOM when cap is smaller than the count: *out_n holds the
 * needed count and the epoch stays open.  BYDB_ERR_STATE when the session
 * is not a row-scan session, BYDB_ERR_BAD_DATA on a device error (sticky
 * until bydb_reset). */
int bydb_rows_finalize(bydb_session *s, bydb_top_row *out, int64_t cap,
                       int64_t *out_n);

/* Pure host, no GPU, no session: the reduce side for time-bucket shards.
 * Each shard is configured with offset 0 and limit offset + limit; this
 * merges the per-shard bydb_rows_finalize results by (ts in the requested
 * direction, series_id ascending) — on a full tie the earlier list first,
 * then the smaller seq — and then cuts [offset, offset + limit).  out holds
 * at most `limit` rows and must not alias a list.  BYDB_ERR_BAD_ARG on
 * null outputs, negative counts, offset + limit > BYDB_TOP_ROWS_MAX or an
 * unknown order. */
int bydb_rows_merge(const bydb_top_row *const *lists, const int64_t *lens,
                    int n_lists, int64_t offset, int64_t limit, int order,
                    bydb_top_row *out, int64_t *out_n);

/* ---- tag projection for raw-row results: tag values by seq ----
 * A measure query without `agg` returns data points with their projected
 * tags: blockCursor.copyTo / copyAllTo (banyand/measure/block.go:509-776)
 * decode every projected tag column of each emitted row through
 * mustDecodeTagValue (query.go:641), and the raw-row egress frame carries
 * them as TagValue columns (bydb_frame_add_tagvalue_*).  This is that seam
 * for the rows bydb_top_finalize / bydb_rows_finalize return: a gather over
 * the encoded tag streams already resident on the device, so the host never
 * decodes a winning block's whole tag column.
 *
 * Contract.  For i in [0, n) the tag value on block tag slot `slot` (0-2)
 * of row (seqs[i] & 8191) of block (seqs[i] >> 13) is
 * data[offs[i] .. offs[i+1]): values lie back to back in request order,
 * offs[0] == 0, and *data_len receives the total byte count.  nil[i] == 1
 * marks a nil value, whose length is 0: a nil dictionary entry, a nil plain
 * row (stored length 0), or a block with no column on the slot.  The empty
 * string is a real value: nil[i] == 0 with length 0 — the distinction the
 * filter section above draws.  The bytes are the stored cell bytes; for int
 * tags the 8-byte sign-flip cell (convert.Int64ToBytes).  Mapping cells to
 * typed TagValues is the host's job, as mustDecodeTagValue does it.
 * Duplicated and unsorted seqs are legal.
 *
 * It is a gather over the resident part, not part of an epoch: legal
 * whenever a part is resident, in any session mode, with an epoch open or
 * closed.  It leaves the consumed state, the sticky device error,
 * bydb_last_consume_ms and every top / rows / aggregate buffer untouched.
 * It runs on the session stream and returns after it has synchronised:
 * unlike the consume entry points the call is synchronous.
 *
 * Errors; none is sticky, the session stays usable after each:
 *  - BYDB_ERR_BAD_ARG: n < 0 or n > BYDB_TAG_FETCH_MAX; slot outside 0..2; a
 *    null seqs / offs / nil / data_len with n > 0; a seq whose block index
 *    is >= the resident block count or whose row is >= that block's count
 *    (the message names the first offending index).
 *  - BYDB_ERR_STATE: no part is resident.
 *  - BYDB_ERR_OOM: data_cap < *data_len, or data is null with a non-zero
 *    total.  *data_len, offs and nil are valid and data is untouched, so a
 *    first call with data_cap == 0 sizes the buffer.  Also when the
 *    session's output arena cannot be allocated (the message names the
 *    size).
 *  - BYDB_ERR_BAD_DATA: a tag stream that cannot be parsed — an unknown
 *    encoding byte, a plain column that was not host-normalised or whose
 *    row count disagrees with the block's, a dictionary whose sections,
 *    entries or value would leave the stream, whose runs end before the
 *    row, or whose code is >= its value count.  The message names the
 *    block.  Nothing is read outside the stream to find this out.
 *  - n == 0: BYDB_OK; offs[0] = 0 is written if offs is non-null. */
#define BYDB_TAG_FETCH_MAX BYDB_TOP_ROWS_MAX   /* rows per call */

int bydb_rows_fetch_tags(bydb_session *s, const uint64_t *seqs, int64_t n,
                         int slot,
                         uint8_t *data, uint64_t data_cap,
                         uint64_t *offs /* n + 1 */, uint8_t *nil /* n */,
                         uint64_t *data_len);

/* Pure host, no GPU, no session: bydb_rows_merge and bydb_top_rows_merge
 * with the origin of every merged row.  seq is shard-local, so a host that
 * merges shards needs to know which shard's session to ask for a merged
 * row's tags: out[i] == lists[out_list[i]][out_index[i]].  Order and error
 * rules are exactly those of the two functions above, which are these with
 * null origin outputs; out_list / out_index may each be null. */
int bydb_rows_merge_src(const bydb_top_row *const *lists, const int64_t *lens,
                        int n_lists, int64_t offset, int64_t limit, int order,
                        bydb_top_row *out, int32_t *out_list, int64_t *out_index,
                        int64_t *out_n);
int bydb_top_rows_merge_src(const bydb_top_row *const *lists, const int64_t *lens,
                            int n_lists, int field_vtype, int64_t n, int asc,
                            bydb_top_row *out, int32_t *out_list,
                            int64_t *out_index, int64_t *out_n);

/* ---- AggModeReduce over raw map frames, with replica dedup ----
 * Restates the liaison reduce (aggregation_reduce.go:83-138 +
 * ReduceRawFrames, reduce.go:78): rows keyed by the key columns
 * (appendKeyComponent semantics); the FIRST row per (shard_id, group_key)
 * pair Combines, replica duplicates drop; MEAN count sidecars are located
 * by the "__agg_count" name walk; Val() applies meanReduce's >=1 clamp.
 * shard_col < 0 dedups on the group key alone (the reference's
 * shardIDIdx == -1 fallback).  Outputs in first-seen group order:
 * out_i64/out_f64 are [n_groups][n_specs] finals (int64 or float64
 * meaningful per the value column's frame type); key_buf/key_offs
 * (optional) receive the packed group keys.  Returns BYDB_OK and
 * *out_n_groups, or BYDB_ERR_OOM when out_cap/key_buf_cap are small. */
typedef struct {
    int32_t input_col;   /* frame column index of the partial value */
    int32_t func;        /* BYDB_AGG_* */
} bydb_reduce_spec;
int bydb_reduce_frames(const uint8_t *const *frames,
                       const uint64_t *frame_lens, int n_frames,
                       int shard_col, const int32_t *key_cols, int n_key_cols,
                       const bydb_reduce_spec *specs, int n_specs,
                       int64_t out_cap, int64_t *out_i64, double *out_f64,
                       uint8_t *key_buf, uint64_t key_buf_cap,
                       uint64_t *key_offs, int64_t *out_n_groups);

#ifdef __cplusplus
}
#endif
#endif /* BYDB_GPU_H */
