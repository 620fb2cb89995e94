#!/usr/bin/env python3
"""Raw-row top-N legs on one MI355X, one process, one session.

The part is tools/filter_bench.py's synthetic int64 part (8192 series x 1M
datapoints, three entity tags of cardinality 4 / 16 / 256).  Every top leg
sits next to a MAX aggregate consume of the same part and selection, the
two alternating per iteration:

  top10 / top100 / top1000      desc, unfiltered, against MAX unfiltered
  top100_eq3                    desc under three entity-tag EQ conditions,
                                against MAX under the same conditions

kernel_ms is bydb_last_consume_ms: for a top consume the HIP-event span of
all its kernels (bounds, both selections, row keys, resolve), for the MAX
consume the scan launches.  wall_ms is host time from the consume call to
the end of finalize.  Medians over --iters after --warmup.  Each top leg is
checked against the MAX leg (the best row's value is the maximum) and for
its order.  Nothing is gated: this records what was measured.

Usage: python tools/top_rows_bench.py [--series N] [--dp N] [--out FILE]
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
    from banyandb_amd import TagCond, OP_EQ, TAG_INT

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

    def consume(conds):
        if conds:
            sess.consume_filter(conds)
        else:
            sess.consume()

    def run_max(conds):
        sess.configure(ba.VT_INT64, [ba.AGG_MAX])
        t0 = time.perf_counter()
        consume(conds)
        r = sess.finalize()[0]
        t1 = time.perf_counter()
        return r.max_i, sess.last_consume_ms(), (t1 - t0) * 1e3

    def run_top(n, conds):
        sess.configure_top(ba.VT_INT64, n)
        t0 = time.perf_counter()
        consume(conds)
        rows = sess.top_rows()
        t1 = time.perf_counter()
        return rows, sess.last_consume_ms(), (t1 - t0) * 1e3

    legs = {}
    for name, n, conds in (("top10", 10, None), ("top100", 100, None),
                           ("top1000", 1000, None),
                           ("top100_eq3", 100, eq_conds)):
        k_top, k_max, w_top, w_max = [], [], [], []
        for it in range(args.warmup + args.iters):
            mx, km, wm = run_max(conds)
            rows, kt, wt = run_top(n, conds)
            if len(rows) != n or rows[0].value_i != mx:
                raise SystemExit(f"{name}: {len(rows)} rows, best "
                                 f"{rows[0].value_i if rows else None} != "
                                 f"max {mx}")
            keys = [(-r.value_i, r.seq) for r in rows]
            if keys != sorted(keys) or len(set(keys)) != n:
                raise SystemExit(f"{name}: rows out of order")
            if it >= args.warmup:
                k_top.append(kt)
                k_max.append(km)
                w_top.append(wt)
                w_max.append(wm)
        legs[name] = {
            "n": n, "conditions": len(conds or []),
            "top_kernel_ms_median": statistics.median(k_top),
            "top_kernel_ms_min": min(k_top), "top_kernel_ms_max": max(k_top),
            "max_scan_kernel_ms_median": statistics.median(k_max),
            "max_scan_kernel_ms_min": min(k_max),
            "max_scan_kernel_ms_max": max(k_max),
            "top_over_max_scan_kernel": statistics.median(k_top) /
            statistics.median(k_max),
            "top_wall_ms_median": statistics.median(w_top),
            "max_scan_wall_ms_median": statistics.median(w_max),
            "best_value": rows[0].value_i, "worst_value": rows[-1].value_i,
        }
    sess.close()

    out = {
        "tool": "tools/top_rows_bench.py",
        "part": {"series": n_series, "datapoints_per_series": n_dp,
                 "blocks": n_series * blocks_per_series,
                 "tag_cardinalities": [4, 16, 256],
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
