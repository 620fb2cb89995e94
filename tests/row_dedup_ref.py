"""Reference model of the cross-part version dedup — the reference's
measure query merge restated per row.

For equal (seriesID, timestamp) queryResult.Less orders versions descending
and queryResult.merge keeps the first row, replacing it only by a later row
of greater version (banyand/measure/query.go:913-943, 966-1026): exactly
one row per (series, timestamp) survives, the one with the highest version.
Equal versions are unordered there; this engine keeps the row of the
earliest appended block, so the survivor is the maximum of
(version, -block index).

A block is any object with .sid, .ts and .vers (block index = position in
the list, i.e. append order).  Rows inside one block have distinct,
ascending timestamps (the part builder folds duplicates itself)."""
import copy


def survivors(blocks):
    """Per block, the ascending list of surviving row indices."""
    best = {}
    for b, blk in enumerate(blocks):
        for r, (t, v) in enumerate(zip(blk.ts, blk.vers)):
            key = (blk.sid, t)
            cand = (v, -b)
            if key not in best or cand > best[key][0]:
                best[key] = (cand, b, r)
    out = [[] for _ in blocks]
    for _cand, b, r in best.values():
        out[b].append(r)
    for rows in out:
        rows.sort()
    return out


def peers(blocks):
    """Brute-force O(n^2) pairing: same series, [ts_min, ts_max] ranges
    intersect (both ends inclusive); ascending block indices per block."""
    out = [[] for _ in blocks]
    for i, a in enumerate(blocks):
        for j, b in enumerate(blocks):
            if i != j and a.sid == b.sid and a.ts[0] <= b.ts[-1] \
                    and b.ts[0] <= a.ts[-1]:
                out[i].append(j)
    return out


def stats(blocks):
    """[overlapping blocks, partially superseded blocks, fully superseded
    blocks, superseded rows] — what bydb_row_dedup_stats reports."""
    keep = survivors(blocks)
    overlap = sum(1 for p in peers(blocks) if p)
    partial = sum(1 for blk, k in zip(blocks, keep) if 0 < len(k) < len(blk.ts))
    full = sum(1 for k in keep if not k)
    rows = sum(len(blk.ts) - len(k) for blk, k in zip(blocks, keep))
    return [overlap, partial, full, rows]


def merged(blocks):
    """The blocks with their superseded rows deleted and emptied blocks
    dropped; series, group code and tags are kept.  Feeding these to the
    existing checkers gives the expected aggregates."""
    out = []
    for blk, keep in zip(blocks, survivors(blocks)):
        if not keep:
            continue
        nb = copy.copy(blk)
        nb.ts = [blk.ts[r] for r in keep]
        nb.vers = [blk.vers[r] for r in keep]
        nb.vals = [blk.vals[r] for r in keep]
        nb.tags = [[col[r] for r in keep] for col in blk.tags]
        out.append(nb)
    return out
