#!/usr/bin/env python3
"""Same-box A/B of the tag filter entry point against the equality one.

One synthetic part with three entity tags (set_tag_table) of cardinality
4 (env, string), 16 (region code, int cells) and 256 (service, string);
one process, one session, the three legs interleaved per iteration:

  (a) consume(preds=[...])        three EQ values through the equality
                                  wrapper, which builds EQ conditions and
                                  runs the same resolve stage as (b)
  (b) consume_filter              the same three EQ conditions
  (c) consume_filter              4-value IN + two-sided int range + NE

Since the two entry points share one stage, (a) against (b) prices the
wrapper, not a second implementation; the gate is kept as a guard on that.
kernel_ms is bydb_last_consume_ms (HIP events around the scan launches —
the resolve prepasses run before the start event); wall_ms is host time
from the consume call to the end of finalize, so it also prices
validation, the literal upload and the resolve prepasses.  Medians over --iters after
--warmup.  Gate: (b) kernel_ms within 10 % of (a) (the README's stated
box-to-box variance; this is a same-box A/B).  (c) is recorded only.

Usage: python tools/filter_bench.py [--series N] [--dp N] [--out FILE]
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
    if args.iters < 10:
        ap.error("--iters must be at least 10")

    import banyandb_amd as ba
    from banyandb_amd import (TagCond, OP_EQ, OP_NE, OP_LT, OP_GE, OP_IN,
                              TAG_INT)

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
    sess.configure(ba.VT_INT64, [ba.AGG_SUM, ba.AGG_COUNT])

    # series s carries envs[s % 4], regions[s % 16], svcs[s % 256]
    eq_vals = [envs[0], regions[4], svcs[4]]
    eq_conds = [TagCond(0, OP_EQ, [eq_vals[0]]),
                TagCond(1, OP_EQ, [eq_vals[1]], TAG_INT),
                TagCond(2, OP_EQ, [eq_vals[2]])]
    in_svcs = [svcs[4], svcs[20], svcs[36], svcs[52]]
    wide_conds = [TagCond(2, OP_IN, in_svcs),
                  TagCond(1, OP_GE, [4], TAG_INT),
                  TagCond(1, OP_LT, [8], TAG_INT),
                  TagCond(0, OP_NE, [b"dev"])]
    legs = {
        "a_consume_eq3": lambda: sess.consume(preds=eq_vals),
        "b_filter_eq3": lambda: sess.consume_filter(eq_conds),
        "c_filter_in4_range_ne": lambda: sess.consume_filter(wide_conds),
    }
    want_rows = {
        "a_consume_eq3": n_dp * sum(1 for s in range(n_series)
                                    if s % 256 == 4),
        "c_filter_in4_range_ne": n_dp * sum(1 for s in range(n_series)
                                            if s % 256 in (4, 20, 36, 52)),
    }
    want_rows["b_filter_eq3"] = want_rows["a_consume_eq3"]

    kernel_ms = {k: [] for k in legs}
    wall_ms = {k: [] for k in legs}
    results = {}
    for it in range(args.warmup + args.iters):
        for name, run in legs.items():
            sess.reset()
            t0 = time.perf_counter()
            run()
            r = sess.finalize()[0]
            t1 = time.perf_counter()
            if r.count != want_rows[name]:
                raise SystemExit(f"{name}: count {r.count} != "
                                 f"{want_rows[name]}")
            results[name] = (r.count, r.sum_i)
            if it >= args.warmup:
                kernel_ms[name].append(sess.last_consume_ms())
                wall_ms[name].append((t1 - t0) * 1e3)
    if results["a_consume_eq3"] != results["b_filter_eq3"]:
        raise SystemExit("EQ legs disagree: %r" % (results,))
    sess.close()

    med = {k: statistics.median(v) for k, v in kernel_ms.items()}
    wmed = {k: statistics.median(v) for k, v in wall_ms.items()}
    ratio = med["b_filter_eq3"] / med["a_consume_eq3"]
    out = {
        "tool": "tools/filter_bench.py",
        "part": {"series": n_series, "datapoints_per_series": n_dp,
                 "blocks": n_series * blocks_per_series,
                 "tag_cardinalities": [4, 16, 256],
                 "generate_upload_s": round(gen_s, 1)},
        "iters": args.iters, "warmup": args.warmup,
        "kernel_ms_median": med,
        "kernel_ms_min": {k: min(v) for k, v in kernel_ms.items()},
        "kernel_ms_max": {k: max(v) for k, v in kernel_ms.items()},
        "wall_ms_median": wmed,
        "rows_selected": {k: v[0] for k, v in results.items()},
        "b_over_a_kernel": ratio,
        "b_over_a_wall": wmed["b_filter_eq3"] / wmed["a_consume_eq3"],
        "gate": "b_over_a_kernel <= 1.10",
        "pass": ratio <= 1.10,
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0 if out["pass"] else 1


if __name__ == "__main__":
    sys.exit(main())
