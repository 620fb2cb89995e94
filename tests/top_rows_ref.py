"""Reference model of the raw-row top-N — measure.BatchTop restated per row
(pkg/query/vectorized/measure/top.go:30-199).

The rows are what the scan yields, in storage order: the rows that
row_dedup_ref (superseded rows removed BEFORE the filter), filter_ref /
filter_tree_ref and the timestamp clamp leave, in (block, row) order.  They
go through BatchTop's own algorithm: a heap bounded by n whose root is the
worst retained row (Less, :68-82: on equal values the LATER row sits nearer
the root), a strictly better candidate replaces the root (shouldReplace,
:190-199), and Finalize pops everything and reverses (:202-215).  Nulls
sort lowest (cmpTopVal, :95-122).

A float64 key is the row's decimal (mantissa, exponent) compared exactly —
the engine's contract; the reference compares the restored doubles, which
differs only when two different decimals round to one double (mantissas
beyond 2^53)."""
import heapq

import oracle as o

import filter_ref as fr
import filter_tree_ref as ftr
import row_dedup_ref as rdr
from banyandb_amd import TagCond, OP_EQ


def cmp_val(a, b):
    """cmpTopVal: -1 / 0 / +1, None (null) lowest."""
    if a is None and b is None:
        return 0
    if a is None:
        return -1
    if b is None:
        return 1
    return (a > b) - (a < b)


class _HeapRow:
    """One retained row; __lt__ is topHeap.Less."""

    def __init__(self, key, seq, row, asc):
        self.key, self.seq, self.row, self.asc = key, seq, row, asc

    def __lt__(self, other):
        c = cmp_val(self.key, other.key)
        if c != 0:
            return c > 0 if self.asc else c < 0
        return self.seq > other.seq


def batch_top(keys, n, asc):
    """Indices into `keys` (input order; None = null) of the rows BatchTop
    returns, in its output order."""
    if n <= 0:
        return []
    heap = []
    for seq, k in enumerate(keys):
        cand = _HeapRow(k, seq, seq, asc)
        if len(heap) < n:
            heapq.heappush(heap, cand)
            continue
        c = cmp_val(k, heap[0].key)
        if (c < 0) if asc else (c > 0):
            heapq.heapreplace(heap, cand)
    out = []
    while heap:
        out.append(heapq.heappop(heap).row)
    out.reverse()
    return out


class Row:
    """One expected output row, field for field a bydb_top_row."""

    def __init__(self, series_id, ts, version, value_i, value_f, seq, key):
        self.series_id, self.ts, self.version = series_id, ts, version
        self.value_i, self.value_f, self.seq = value_i, value_f, seq
        self.key = key

    def astuple(self):
        return (self.series_id, self.ts, self.version, self.value_i,
                self.value_f, self.seq)


def block_decimals(vals):
    """(mantissas, exponent) of one float64 block — the reference's
    per-block decimal conversion (float.go:36-67) through the oracle."""
    return o.float_to_decimal([float(v) for v in vals])


def scan_rows(blocks, is_float=False, conds=None, tree=None, pred=None,
              min_ts=None, max_ts=None, dedup=False):
    """The rows the scan yields, in (block, row) order, as Row objects whose
    key is comparable across blocks (int value, or an exact fraction of the
    decimal)."""
    keep = rdr.survivors(blocks) if dedup else \
        [list(range(len(b.ts))) for b in blocks]
    if pred is not None:
        conds = [TagCond(0, OP_EQ, [pred])]
    rows = []
    for bi, (b, rs) in enumerate(zip(blocks, keep)):
        mants, exp, restored = None, 0, None
        if is_float and rs:
            mants, exp = block_decimals(b.vals)
            restored = o.decimal_to_float(mants, exp)
        for r in rs:
            t = b.ts[r]
            if min_ts is not None and t < min_ts:
                continue
            if max_ts is not None and t > max_ts:
                continue
            tags = [col[r] for col in b.tags]
            if tree is not None:
                if not ftr.row_selected(tree, tags):
                    continue
            elif conds and not fr.row_selected(conds, tags):
                continue
            seq = (bi << 13) | r
            if is_float:
                m = mants[r]
                # exact decimal, scaled to a common integer domain
                key = m * 10 ** (exp + 400)
                rows.append(Row(b.sid, t, b.vers[r], m, restored[r], seq,
                                key))
            else:
                v = b.vals[r]
                rows.append(Row(b.sid, t, b.vers[r], v, 0.0, seq, v))
    return rows


def top_rows(blocks, n, asc=False, **kw):
    """Expected bydb_top_finalize output for a consume over `blocks`."""
    rows = scan_rows(blocks, **kw)
    return [rows[i] for i in batch_top([r.key for r in rows], n, asc)]


def scen_top_rows(scen, n, asc=False, dedup=False):
    """top_rows for a row_dedup_cases.Scen."""
    return top_rows(scen.blocks, n, asc, is_float=scen.kind == "f64",
                    conds=scen.conds, tree=scen.tree, pred=scen.pred,
                    min_ts=scen.min_ts, max_ts=scen.max_ts, dedup=dedup)
