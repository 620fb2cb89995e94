#!/usr/bin/env python3
"""Time-ordered row-scan legs on one MI355X, one process, one session.

The part is tools/filter_bench.py's synthetic int64 part (8192 series x 1M
datapoints on one DeltaConst time axis, three entity tags of cardinality
4 / 16 / 256).  Every leg alternates, per iteration, a COUNT aggregate
consume, a top-N consume (bydb_top_configure) and the row scan of the same
part and selection:

  latest100 / earliest100       unfiltered, full range
  latest10 / latest1000         the same at other N
  latest100_clamp / earliest100_clamp
                                under a clamp that starts and ends inside a
                                block of every series (one range cuts two
                                blocks per series; the blocks between are
                                covered whole, the rest lie outside), so the
                                winners' timestamps come from the closed-form
                                DeltaConst path
  latest100_eq3 / earliest100_eq3
                                under three entity-tag EQ conditions

kernel_ms is bydb_last_consume_ms: for a row-scan consume the HIP-event span
of all its kernels (block keys, both two-word selections, row keys,
resolve), for the COUNT consume the scan launches.  wall_ms is host time
from the consume call to the end of finalize.  Medians over --iters after
--warmup.  Each row-scan leg is checked for its length, its order and its
first timestamp.  Nothing is gated: this records what was measured.

Usage: python tools/row_scan_bench.py [--series N] [--dp N] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

T0 = 1_700_000_000_000_000_000
STRIDE = 10 ** 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=8192)
    ap.add_argument("--dp", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import banyandb_amd as ba
    from banyandb_amd import TagCond, OP_EQ, TAG_INT, INT64_MIN, INT64_MAX

    envs = [b"prod", b"dev", b"staging", b"qa"]
    regions = [ba.i64_tag_cell(i) for i in range(16)]
    svcs = [b"s%d" % i for i in range(256)]
    threads = min(16, os.cpu_count() or 8)

    n_series, n_dp = args.series, args.dp
    blocks_per_series = (n_dp + 8191) // 8192
    sess = ba.Session(0)
    sess.reserve(int(n_series * n_dp * 1.05) +
                 n_series * (1 + blocks_per_series) * 256,
                 n_series * blocks_per_series)
    t_gen = time.perf_counter()
    b = ba.PartBuilder()
    for slot, table in enumerate((envs, regions, svcs)):
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

    # series s carries envs[s % 4], regions[s % 16], svcs[s % 256]
    eq_conds = [TagCond(0, OP_EQ, [envs[0]]),
                TagCond(1, OP_EQ, [regions[4]], TAG_INT),
                TagCond(2, OP_EQ, [svcs[4]])]
    full = (INT64_MIN, INT64_MAX)
    cut = min(4096, n_dp // 4)
    clamp = (T0 + cut * STRIDE, T0 + (n_dp - 1 - cut) * STRIDE)

    def consume(conds, rng):
        if conds:
            sess.consume_filter(conds, rng[0], rng[1])
        else:
            sess.consume(rng[0], rng[1])

    def run_count(conds, rng):
        sess.configure(ba.VT_INT64, [ba.AGG_COUNT])
        t0 = time.perf_counter()
        consume(conds, rng)
        r = sess.finalize()[0]
        t1 = time.perf_counter()
        return r.count, sess.last_consume_ms(), (t1 - t0) * 1e3

    def run_top(n, conds, rng):
        sess.configure_top(ba.VT_INT64, n)
        t0 = time.perf_counter()
        consume(conds, rng)
        rows = sess.top_rows()
        t1 = time.perf_counter()
        return rows, sess.last_consume_ms(), (t1 - t0) * 1e3

    def run_rows(n, desc, conds, rng):
        sess.configure_rows(ba.VT_INT64, 0, n, desc)
        t0 = time.perf_counter()
        consume(conds, rng)
        rows = sess.scan_rows()
        t1 = time.perf_counter()
        return rows, sess.last_consume_ms(), (t1 - t0) * 1e3

    def med(xs):
        return statistics.median(xs)

    legs = {}
    for name, n, desc, conds, rng in (
            ("latest100", 100, True, None, full),
            ("earliest100", 100, False, None, full),
            ("latest10", 10, True, None, full),
            ("latest1000", 1000, True, None, full),
            ("latest100_clamp", 100, True, None, clamp),
            ("earliest100_clamp", 100, False, None, clamp),
            ("latest100_eq3", 100, True, eq_conds, full),
            ("earliest100_eq3", 100, False, eq_conds, full)):
        lo = max(rng[0], T0)
        hi = min(rng[1], T0 + (n_dp - 1) * STRIDE)
        k = {"rows": [], "count": [], "top": []}
        w = {"rows": [], "count": [], "top": []}
        for it in range(args.warmup + args.iters):
            cnt, kc, wc = run_count(conds, rng)
            top, kt, wt = run_top(n, conds, rng)
            rows, kr, wr = run_rows(n, desc, conds, rng)
            if len(rows) != min(n, cnt) or len(top) != len(rows):
                raise SystemExit(f"{name}: {len(rows)} rows, {len(top)} top "
                                 f"rows, count {cnt}")
            keys = [(-r.ts if desc else r.ts, r.series_id, r.seq)
                    for r in rows]
            if keys != sorted(keys) or len(set(keys)) != len(keys):
                raise SystemExit(f"{name}: rows out of order")
            if rows[0].ts != (hi if desc else lo):
                raise SystemExit(f"{name}: first timestamp {rows[0].ts}")
            if it >= args.warmup:
                for key, kv, wv in (("rows", kr, wr), ("count", kc, wc),
                                    ("top", kt, wt)):
                    k[key].append(kv)
                    w[key].append(wv)
        legs[name] = {
            "n": n, "desc": desc, "conditions": len(conds or []),
            "clamped": rng is clamp, "selected_rows": cnt,
            "rows_kernel_ms_median": med(k["rows"]),
            "rows_kernel_ms_min": min(k["rows"]),
            "rows_kernel_ms_max": max(k["rows"]),
            "count_scan_kernel_ms_median": med(k["count"]),
            "count_scan_kernel_ms_min": min(k["count"]),
            "count_scan_kernel_ms_max": max(k["count"]),
            "top_kernel_ms_median": med(k["top"]),
            "top_kernel_ms_min": min(k["top"]),
            "top_kernel_ms_max": max(k["top"]),
            "rows_over_count_scan_kernel": med(k["rows"]) / med(k["count"]),
            "rows_over_top_kernel": med(k["rows"]) / med(k["top"]),
            "rows_wall_ms_median": med(w["rows"]),
            "count_scan_wall_ms_median": med(w["count"]),
            "top_wall_ms_median": med(w["top"]),
            "first_ts": rows[0].ts, "last_ts": rows[-1].ts,
        }
    sess.close()

    out = {
        "tool": "tools/row_scan_bench.py",
        "part": {"series": n_series, "datapoints_per_series": n_dp,
                 "blocks": n_series * blocks_per_series,
                 "tag_cardinalities": [4, 16, 256],
                 "clamp_rows_cut_each_end": cut,
                 "generate_upload_s": round(gen_s, 1)},
        "iters": args.iters, "warmup": args.warmup,
        "legs": legs,
    }
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
