#!/usr/bin/env python3
"""Tag-projection legs on one MI355X, one process.

Leg one — the part of tools/row_scan_bench.py (8192 series x 1M datapoints
on one DeltaConst time axis, entity tag tables of cardinality 4 / 16 / 256
on the three slots): a latest-N row scan for N = 10 / 100 / 1000, then
Session.fetch_tags of the rows it returned, on each slot.  Every winner sits
in a single-run dictionary block: the best case of the locate walk.

Leg two — a small part whose winners sit in the worst blocks for the locate
walk: dictionary columns of 8192 rows in 8192 runs (slot 0), and plain
columns of 8192 rows (slot 1); the latest-N rows are the last rows of their
blocks, so the run walk takes all 128 steps and the plain walk all 128
chunks.

fetch wall_ms is host time round fetch_tags — both C calls, the sizing one
and the fetching one, and the Python list building.  fetch_c_ms is host time
round the second C call alone (upload, locate, offsets, first wait, copy,
download).  The row scan's wall_ms is host time from the consume call to the
end of scan_rows, its kernel_ms bydb_last_consume_ms.  Medians over --iters
after --warmup.  Every fetched value is checked.  Nothing is gated: this
records what was measured.

Usage: python tools/tag_fetch_bench.py [--series N] [--dp N] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

T0 = 1_700_000_000_000_000_000
STRIDE = 10 ** 6


def med(xs):
    return statistics.median(xs)


def fetch_c_ms(ba, sess, rows, slot):
    """The fetching C call alone, its buffer sized beforehand."""
    n = len(rows)
    arr = (C.c_uint64 * n)(*[r.seq for r in rows])
    offs = (C.c_uint64 * (n + 1))()
    nil = (C.c_uint8 * n)()
    total = C.c_uint64(0)
    lib = ba.lib()
    lib.bydb_rows_fetch_tags(sess._h, arr, n, slot, None, 0, offs, nil,
                             C.byref(total))
    data = (C.c_uint8 * max(total.value, 1))()
    t0 = time.perf_counter()
    rc = lib.bydb_rows_fetch_tags(sess._h, arr, n, slot, data, total.value,
                                  offs, nil, C.byref(total))
    t1 = time.perf_counter()
    if rc != 0:
        raise SystemExit(f"fetch rc={rc}")
    return (t1 - t0) * 1e3


def run_leg(ba, sess, n, slots, want_of, iters, warmup):
    scan_w, scan_k = [], []
    fetch_w = {sl: [] for sl in slots}
    fetch_c = {sl: [] for sl in slots}
    for it in range(warmup + iters):
        sess.configure_rows(ba.VT_INT64, 0, n, True)
        t0 = time.perf_counter()
        sess.consume()
        rows = sess.scan_rows()
        t1 = time.perf_counter()
        if len(rows) != n:
            raise SystemExit(f"latest{n}: {len(rows)} rows")
        rec = it >= warmup
        if rec:
            scan_w.append((t1 - t0) * 1e3)
            scan_k.append(sess.last_consume_ms())
        for sl in slots:
            t0 = time.perf_counter()
            vals = sess.fetch_tags(rows, sl)
            t1 = time.perf_counter()
            for r, v in zip(rows, vals):
                if v != want_of(r, sl):
                    raise SystemExit(f"latest{n} slot {sl} seq {r.seq}: {v!r}")
            c_ms = fetch_c_ms(ba, sess, rows, sl)
            if rec:
                fetch_w[sl].append((t1 - t0) * 1e3)
                fetch_c[sl].append(c_ms)
    out = {"n": n,
           "row_scan_wall_ms_median": med(scan_w),
           "row_scan_kernel_ms_median": med(scan_k),
           "fetch": {}}
    for sl in slots:
        out["fetch"]["slot%d" % sl] = {
            "wall_ms_median": med(fetch_w[sl]),
            "wall_ms_min": min(fetch_w[sl]), "wall_ms_max": max(fetch_w[sl]),
            "c_call_ms_median": med(fetch_c[sl]),
            "c_call_ms_min": min(fetch_c[sl]),
            "c_call_ms_max": max(fetch_c[sl]),
            "wall_over_row_scan_wall": med(fetch_w[sl]) / med(scan_w),
        }
    out["fetch_all_slots_wall_ms_median"] = sum(
        med(fetch_w[sl]) for sl in slots)
    out["fetch_all_slots_over_row_scan_wall"] = \
        out["fetch_all_slots_wall_ms_median"] / med(scan_w)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=8192)
    ap.add_argument("--dp", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import banyandb_amd as ba

    # ---- leg one: entity tag tables ----
    tables = [[b"prod", b"dev", b"staging", b"qa"],
              [ba.i64_tag_cell(i) for i in range(16)],
              [b"s%d" % i for i in range(256)]]
    threads = min(16, os.cpu_count() or 8)
    n_series, n_dp = args.series, args.dp
    bps = (n_dp + 8191) // 8192
    sess = ba.Session(0)
    sess.reserve(int(n_series * n_dp * 1.05) + n_series * (1 + bps) * 256,
                 n_series * bps)
    t_gen = time.perf_counter()
    b = ba.PartBuilder()
    for slot, table in enumerate(tables):
        b.set_tag_table(slot, table)
    s0 = 0
    while s0 < n_series:
        ns = min(500, n_series - s0)
        b.gen_bulk_i64(s0, ns, n_dp, T0, STRIDE, 1000, 1, 0xB4DB,
                       threads=threads)
        sess.append(b)
        b.drain()
        s0 += ns
    gen_s = time.perf_counter() - t_gen

    # block index -> series: blocks are appended series by series
    def entity_want(r, sl):
        series = (r.seq >> 13) // bps
        return tables[sl][series % len(tables[sl])]
    entity = {}
    for n in (10, 100, 1000):
        entity["latest%d" % n] = run_leg(ba, sess, n, (0, 1, 2), entity_want,
                                         args.iters, args.warmup)
    sess.close()

    # ---- leg two: the worst blocks for the locate walk ----
    n_blk, rows_blk = 128, 8192
    pb = ba.PartBuilder()
    cols = []
    for k in range(n_blk):
        ts = [T0 + (i * n_blk + k) * STRIDE for i in range(rows_blk)]
        pb.add_block_i64(k + 1, ts, [1] * rows_blk, list(range(rows_blk)))
        runs = [b"even-%d" % k if i % 2 == 0 else b"odd-%d" % k
                for i in range(rows_blk)]
        plain = [b"req-%d-%d" % (k, i) for i in range(rows_blk)]
        pb.set_block_tag(runs)
        pb.set_block_tag(plain)
        cols.append((runs, plain))
    sess = ba.Session(0)
    sess.upload_part(pb)

    def worst_want(r, sl):
        return cols[r.seq >> 13][sl][r.seq & 8191]
    worst = {}
    for n in (10, 100, 1000):
        worst["latest%d" % n] = run_leg(ba, sess, n, (0, 1), worst_want,
                                        args.iters, args.warmup)
    sess.close()

    out = {
        "tool": "tools/tag_fetch_bench.py",
        "entity_part": {"series": n_series, "datapoints_per_series": n_dp,
                        "blocks": n_series * bps,
                        "tag_cardinalities": [4, 16, 256],
                        "generate_upload_s": round(gen_s, 1)},
        "worst_part": {"blocks": n_blk, "rows_per_block": rows_blk,
                       "slot0": "dictionary, 8192 runs per block",
                       "slot1": "plain, 8192 distinct values per block"},
        "iters": args.iters, "warmup": args.warmup,
        "entity_legs": entity, "worst_legs": worst,
    }
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
