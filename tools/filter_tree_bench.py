#!/usr/bin/env python3
"""Criteria-tree legs on one MI355X, one process.

Part 1 is tools/filter_bench.py's synthetic part: three entity tags
(set_tag_table) of cardinality 4 (env, string), 16 (region code, int
cells) and 256 (service, string); one session, legs interleaved per
iteration:

  (a) consume_filter              three EQ conditions
  (b) consume_filter_tree         the same three as an AND tree — no OR
                                  node, so the same code path; the gate
                                  guards that delegation
  (c) consume_filter_tree         env = prod OR region = 4: every block is
                                  one truth-table lookup
  (d) consume_filter_tree         (env = prod AND region < 4) OR svc IN [4]

Part 2 is small: every block carries two row-varying dictionary tags, so
under a cross-slot OR every block is a row-bitmap block:

  (e_or)  consume_filter_tree     env = prod OR code >= 404
  (e_and) consume_filter          the same two leaves ANDed (two code-mask
                                  walkers in the run merge)

kernel_ms is bydb_last_consume_ms (HIP events around the scan launches —
the resolve kernels run before the start event); wall_ms is host time from
the consume call to the end of finalize, so it also prices validation, the
literal upload, the resolve kernels and, on the OR path, the census
read-back.  wall_ms - kernel_ms is therefore everything but the scan: the
resolve kernels plus host overhead (Python, ctypes, finalize's sync and
download); for part 2 it is reported per block as resolve_plus_host next
to the scan's kernel_ms per block, and only the difference between two
legs' resolve_plus_host says anything about the resolve kernels.
Medians over --iters after --warmup.  Gate: (b) kernel_ms within 10 % of
(a) (the README's stated box-to-box variance; this is a same-box A/B).
Everything else is recorded only.

Usage: python tools/filter_tree_bench.py [--series N] [--dp N]
                                         [--row-blocks N] [--out FILE]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

T0 = 1_700_000_000_000_000_000
STRIDE = 10 ** 6


def run_legs(sess, legs, want_rows, iters, warmup):
    """legs: name -> (callable, goes through consume_filter_tree)."""
    kernel_ms = {k: [] for k in legs}
    wall_ms = {k: [] for k in legs}
    results, stats = {}, {}
    for it in range(warmup + iters):
        for name, (run, is_tree) in legs.items():
            sess.reset()
            t0 = time.perf_counter()
            run()
            r = sess.finalize()[0]
            t1 = time.perf_counter()
            if r.count != want_rows[name]:
                raise SystemExit(f"{name}: count {r.count} != "
                                 f"{want_rows[name]}")
            results[name] = (r.count, r.sum_i)
            # the census belongs to the last tree consume: other legs
            # would read a stale one
            stats[name] = sess.filter_tree_stats() if is_tree else None
            if it >= warmup:
                kernel_ms[name].append(sess.last_consume_ms())
                wall_ms[name].append((t1 - t0) * 1e3)
    return kernel_ms, wall_ms, results, stats


def summarise(kernel_ms, wall_ms, results, stats):
    return {
        "kernel_ms_median": {k: statistics.median(v)
                             for k, v in kernel_ms.items()},
        "kernel_ms_min": {k: min(v) for k, v in kernel_ms.items()},
        "kernel_ms_max": {k: max(v) for k, v in kernel_ms.items()},
        "wall_ms_median": {k: statistics.median(v)
                           for k, v in wall_ms.items()},
        "rows_selected": {k: v[0] for k, v in results.items()},
        "tree_stats_clear_skip_mask_rows": stats,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=8192)
    ap.add_argument("--dp", type=int, default=1_000_000)
    ap.add_argument("--row-blocks", type=int, default=512)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.iters < 10:
        ap.error("--iters must be at least 10")

    import banyandb_amd as ba
    from banyandb_amd import (TagCond, And, Or, OP_EQ, OP_LT, OP_GE, OP_IN,
                              TAG_INT)

    envs = [b"prod", b"dev", b"staging", b"qa"]
    regions = [ba.i64_tag_cell(i) for i in range(16)]
    svcs = [b"s%d" % i for i in range(256)]
    threads = min(16, os.cpu_count() or 8)

    # ---- part 1: entity tags ----
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
    eq_conds = [TagCond(0, OP_EQ, [envs[0]]),
                TagCond(1, OP_EQ, [regions[4]], TAG_INT),
                TagCond(2, OP_EQ, [svcs[4]])]
    in_svcs = [svcs[4], svcs[20], svcs[36], svcs[52]]
    or2 = Or(TagCond(0, OP_EQ, [envs[0]]),
             TagCond(1, OP_EQ, [regions[4]], TAG_INT))
    and_or = Or(And(TagCond(0, OP_EQ, [envs[0]]),
                    TagCond(1, OP_LT, [4], TAG_INT)),
                TagCond(2, OP_IN, in_svcs))
    legs = {
        "a_filter_eq3": (lambda: sess.consume_filter(eq_conds), False),
        "b_tree_and_eq3": (lambda: sess.consume_filter_tree(And(*eq_conds)),
                           True),
        "c_tree_or_2_entity_tags": (lambda: sess.consume_filter_tree(or2),
                                    True),
        "d_tree_and_or_in": (lambda: sess.consume_filter_tree(and_or), True),
    }
    sr = range(n_series)
    want_rows = {
        "a_filter_eq3": n_dp * sum(1 for s in sr if s % 256 == 4),
        "c_tree_or_2_entity_tags":
            n_dp * sum(1 for s in sr if s % 4 == 0 or s % 16 == 4),
        "d_tree_and_or_in":
            n_dp * sum(1 for s in sr if (s % 4 == 0 and s % 16 < 4)
                       or s % 256 in (4, 20, 36, 52)),
    }
    want_rows["b_tree_and_eq3"] = want_rows["a_filter_eq3"]
    k1, w1, res1, st1 = run_legs(sess, legs, want_rows, args.iters,
                                 args.warmup)
    if res1["a_filter_eq3"] != res1["b_tree_and_eq3"]:
        raise SystemExit("AND-tree leg disagrees: %r" % (res1,))
    sess.close()

    # ---- part 2: two row-varying dictionary tags on every block ----
    rng = random.Random(0xB17)
    codes = [200, 302, 404, 500, 503]
    n = 8192
    variants = []
    for _ in range(8):
        col0, col1 = [], []
        for col, pool, maxrun in ((col0, envs, 40),
                                  (col1, [ba.i64_tag_cell(c) for c in codes],
                                   25)):
            while len(col) < n:
                run = min(rng.randint(1, maxrun), n - len(col))
                col.extend([pool[rng.randrange(len(pool))]] * run)
        sel_or = sum(1 for e, c in zip(col0, col1)
                     if e == b"prod" or c >= ba.i64_tag_cell(404))
        sel_and = sum(1 for e, c in zip(col0, col1)
                      if e == b"prod" and c >= ba.i64_tag_cell(404))
        variants.append((col0, col1, sel_or, sel_and))
    ts = [T0 + i * STRIDE for i in range(n)]
    vals = [(i * 37) % 1000 for i in range(n)]
    ver = [1] * n
    b2 = ba.PartBuilder()
    want_or = want_and = 0
    for blk in range(args.row_blocks):
        col0, col1, sel_or, sel_and = variants[blk % len(variants)]
        b2.add_block_i64(blk + 1, ts, ver, vals)
        b2.set_block_tag(col0)
        b2.set_block_tag(col1)
        want_or += sel_or
        want_and += sel_and
    sess2 = ba.Session(0)
    sess2.upload_part(b2)
    sess2.configure(ba.VT_INT64, [ba.AGG_SUM, ba.AGG_COUNT])
    leaves = [TagCond(0, OP_EQ, [b"prod"]), TagCond(1, OP_GE, [404], TAG_INT)]
    legs2 = {
        "e_or_row_bitmap": (lambda: sess2.consume_filter_tree(Or(*leaves)),
                            True),
        "e_and_mask_walkers": (lambda: sess2.consume_filter(leaves), False),
    }
    k2, w2, res2, st2 = run_legs(
        sess2, legs2, {"e_or_row_bitmap": want_or,
                       "e_and_mask_walkers": want_and},
        args.iters, args.warmup)
    sess2.close()
    if st2["e_or_row_bitmap"][3] != args.row_blocks:
        raise SystemExit("part 2: not every block is a row-bitmap block: "
                         "%r" % (st2,))

    part1 = summarise(k1, w1, res1, st1)
    part2 = summarise(k2, w2, res2, st2)
    nb2 = args.row_blocks
    part2["per_block_us"] = {
        k: {"scan_kernel": 1e3 * part2["kernel_ms_median"][k] / nb2,
            "resolve_plus_host": 1e3 * (part2["wall_ms_median"][k] -
                                        part2["kernel_ms_median"][k]) / nb2}
        for k in legs2}
    med = part1["kernel_ms_median"]
    ratio = med["b_tree_and_eq3"] / med["a_filter_eq3"]
    out = {
        "tool": "tools/filter_tree_bench.py",
        "iters": args.iters, "warmup": args.warmup,
        "entity_tag_part": dict(
            part={"series": n_series, "datapoints_per_series": n_dp,
                  "blocks": n_series * blocks_per_series,
                  "tag_cardinalities": [4, 16, 256],
                  "generate_upload_s": round(gen_s, 1)}, **part1),
        "row_bitmap_part": dict(
            part={"blocks": nb2, "rows_per_block": n,
                  "tags": "env (4 values, runs <= 40), code (5 int values, "
                          "runs <= 25), both row-varying dictionaries"},
            **part2),
        "b_over_a_kernel": ratio,
        "b_over_a_wall": (part1["wall_ms_median"]["b_tree_and_eq3"] /
                          part1["wall_ms_median"]["a_filter_eq3"]),
        "gate": "b_over_a_kernel <= 1.10",
        "pass": ratio <= 1.10,
    }
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0 if out["pass"] else 1


if __name__ == "__main__":
    sys.exit(main())
