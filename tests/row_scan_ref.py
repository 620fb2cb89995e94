"""Reference model of the time-ordered row scan — Scan -> Limit restated per
row (banyand/measure/query.go:913-943, 962-1026;
pkg/query/vectorized/measure/limit.go:81-108).

The rows are what the scan yields: the rows that row_dedup_ref (superseded
rows removed BEFORE the filter), filter_ref / filter_tree_ref and the
timestamp clamp leave (top_rows_ref.scan_rows).  queryResult's heap orders
them by timestamp in the requested direction, equal timestamps by seriesID
ascending (queryResult.Less); with dedup on, (series, timestamp) is unique
and that is a total order.  With dedup off the engine's own rule decides the
rest: storage order, seq = (block << 13) | row.  BatchLimit keeps rows
[offset, offset + limit) of that stream.

series_id compares as an unsigned 64-bit value, ts as a signed one."""
import top_rows_ref as trr

U64 = (1 << 64) - 1


def row_key(r, desc):
    return (-r.ts if desc else r.ts, r.series_id & U64, r.seq)


def ordered(rows, desc=False):
    return sorted(rows, key=lambda r: row_key(r, desc))


def batch_limit(batches, offset, limit, prior_selection=None):
    """BatchLimit.Process over consecutive batches (lengths `batches`;
    prior_selection: the first batch's active indices, None = all).  Returns
    the kept indices per batch; batches after the window closes are never
    pulled and keep nothing."""
    seen, end, out, closed = 0, offset + limit, [], False
    for bi, n in enumerate(batches):
        active = list(range(n))
        if bi == 0 and prior_selection is not None:
            active = list(prior_selection)
        kept = []
        if not closed:
            for idx in active:
                if offset <= seen < end:
                    kept.append(idx)
                seen += 1
                if seen >= end:
                    closed = True
                    break
        out.append(kept)
    return out


def window(rows, offset, limit):
    """BatchLimit over one stream."""
    kept = batch_limit([len(rows)], offset, limit)[0]
    return [rows[i] for i in kept]


def scan_window(blocks, offset, limit, desc=False, **kw):
    """Expected bydb_rows_finalize output for a consume over `blocks`."""
    return window(ordered(trr.scan_rows(blocks, **kw), desc), offset, limit)


def scen_scan_rows(scen, offset, limit, desc=False, dedup=False):
    """scan_window for a row_dedup_cases.Scen."""
    return scan_window(scen.blocks, offset, limit, desc,
                       is_float=scen.kind == "f64", conds=scen.conds,
                       tree=scen.tree, pred=scen.pred, min_ts=scen.min_ts,
                       max_ts=scen.max_ts, dedup=dedup)


def merge(lists, offset, limit, desc=False):
    """Expected bydb_rows_merge: rows (anything with ts, series_id, seq) of
    all lists by (ts direction, series unsigned); on a full tie the earlier
    list first, then the smaller seq; then the window."""
    flat = [(r, li) for li, rows in enumerate(lists) for r in rows]
    flat.sort(key=lambda e: (-e[0].ts if desc else e[0].ts,
                             e[0].series_id & U64, e[1], e[0].seq))
    return window([r for r, _ in flat], offset, limit)
