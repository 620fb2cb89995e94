#!/usr/bin/env python3
"""Cross-part version dedup legs on one MI355X, one process.

Part 1 is the synthetic int64 part of tools/filter_tree_bench.py (8192
series x 1M datapoints, sum + count).  A "second on-disk part" re-sends a
share of its blocks byte for byte at version 2, so each re-sent block
fully supersedes its original.  One session:

  (a) dedup off, no overlap          today's scan
  (b) dedup on, no overlap           the same kernels; the first consume
                                     pays the planner once
  (c) dedup on, 1 % re-sent          the re-sent blocks' originals are
                                     PF_SKIP; the whole part goes through
                                     the predicated (EN_PREDS) scan
  (c_off) dedup off, 1 % re-sent     double-counts, as before the feature
  (d) dedup on, 10 % re-sent
  (d_off) dedup off, 10 % re-sent

Part 2 is small: --partial-blocks blocks of 8192 rows in pairs on one
timestamp axis, versions 1 against alternating 2 / 0, so every block is
partially superseded:

  (e_off) dedup off
  (e) dedup on                       every block walks a merged bitmap

kernel_ms is bydb_last_consume_ms (HIP events around the scan launches:
k_dedup_apply runs before the start event); wall_ms is host time from the
consume call to the end of finalize.  build_ms is the wall time of the
first consume after the resident part changed minus the steady wall time of
that leg: descriptor read-back, planner, k_dedup_decode, k_dedup_mark and
the counter read-back.  apply_plus_host_us_per_block for part 2 is
((wall - kernel) of (e) - (wall - kernel) of (e_off)) / blocks.
Medians over --iters after --warmup.  Nothing is gated: the issue's figures
were unmeasured, this records them.

Usage: python tools/row_dedup_bench.py [--series N] [--dp N]
                                       [--partial-blocks N] [--out FILE]
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


def timed(sess, iters, warmup, want_count):
    kernel, wall = [], []
    t0 = time.perf_counter()
    sess.reset()
    sess.consume()
    r = sess.finalize()[0]
    first_wall = (time.perf_counter() - t0) * 1e3
    if r.count != want_count:
        raise SystemExit(f"count {r.count} != {want_count}")
    for it in range(warmup + iters):
        sess.reset()
        t0 = time.perf_counter()
        sess.consume()
        r = sess.finalize()[0]
        t1 = time.perf_counter()
        if r.count != want_count:
            raise SystemExit(f"count {r.count} != {want_count}")
        if it >= warmup:
            kernel.append(sess.last_consume_ms())
            wall.append((t1 - t0) * 1e3)
    wall_med = statistics.median(wall)
    return {"kernel_ms_median": statistics.median(kernel),
            "kernel_ms_min": min(kernel), "kernel_ms_max": max(kernel),
            "wall_ms_median": wall_med,
            "first_consume_wall_ms": first_wall,
            "build_ms": max(first_wall - wall_med, 0.0),
            "rows": r.count, "sum": r.sum_i,
            "dedup_stats": sess.row_dedup_stats()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=8192)
    ap.add_argument("--dp", type=int, default=1_000_000)
    ap.add_argument("--partial-blocks", type=int, default=512)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import banyandb_amd as ba
    lib = ba.lib()
    threads = min(16, os.cpu_count() or 8)
    n_series, n_dp = args.series, args.dp
    bps = (n_dp + 8191) // 8192
    n_blocks = n_series * bps
    n_dup10 = n_blocks // 10
    n_dup1 = n_blocks // 100

    # ---- part 1 ----
    sess = ba.Session(0)
    base_bytes = int(n_series * n_dp * 1.05) + n_series * (1 + bps) * 256
    sess.reserve(base_bytes + base_bytes // 8, n_blocks + n_dup10)
    t_gen = time.perf_counter()
    b = ba.PartBuilder()
    appended = 0
    dup_bytes, dup_descs = [], []     # the "second part": every 10th block
    dup_len = 0
    seen = 0
    s0 = 0
    while s0 < n_series:
        ns = min(500, n_series - s0)
        b.gen_bulk_i64(s0, ns, n_dp, T0, STRIDE, 1000, 1, 0xB4DB,
                       threads=threads)
        sess.append(b)
        descs = b.blocks_ptr()
        buf = (C.c_ubyte * b.payload_len).from_address(
            C.addressof(b.raw_payload_ptr().contents))
        for i in range(b.n_blocks):
            if seen % 10 == 0 and len(dup_descs) < n_dup10:
                d = descs[i]
                lo = d.ts_off - appended
                hi = d.field_off + d.field_len - appended
                nd = ba.BlockDesc()
                C.memmove(C.addressof(nd), C.addressof(d),
                          C.sizeof(ba.BlockDesc))
                nd.version_first = 2          # Const version list
                nd.field_off = dup_len + (d.field_off - d.ts_off)
                nd.ts_off = dup_len           # rebased when appended
                dup_bytes.append(bytes(buf[lo:hi]))
                dup_descs.append(nd)
                dup_len += hi - lo
            seen += 1
        appended += b.payload_len
        b.drain()
        s0 += ns
    gen_s = time.perf_counter() - t_gen
    sess.configure(ba.VT_INT64, [ba.AGG_SUM, ba.AGG_COUNT])
    rows = n_series * n_dp

    def append_dups(first, last):
        """append second-part blocks [first, last) behind what is resident"""
        nonlocal appended
        n = last - first
        blob = b"".join(dup_bytes[first:last])
        start = dup_descs[first].ts_off
        arr = (ba.BlockDesc * n)()
        for k in range(n):
            C.memmove(C.addressof(arr[k]), C.addressof(dup_descs[first + k]),
                      C.sizeof(ba.BlockDesc))
            arr[k].ts_off += appended - start
            arr[k].field_off += appended - start
        pbuf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
        sess._ck(lib.bydb_part_append(sess._h, pbuf, len(blob), arr, n))
        appended += len(blob)
        return sum(d.count for d in dup_descs[first:last])

    legs = {}
    sess.set_row_dedup(0)
    legs["a_off_no_overlap"] = timed(sess, args.iters, args.warmup, rows)
    sess.set_row_dedup(1)
    legs["b_on_no_overlap"] = timed(sess, args.iters, args.warmup, rows)
    dup_rows = append_dups(0, n_dup1)
    legs["c_on_1pct_resent"] = timed(sess, args.iters, args.warmup, rows)
    sess.set_row_dedup(0)
    legs["c_off_1pct_resent"] = timed(sess, args.iters, args.warmup,
                                      rows + dup_rows)
    dup_rows += append_dups(n_dup1, n_dup10)
    sess.set_row_dedup(1)
    legs["d_on_10pct_resent"] = timed(sess, args.iters, args.warmup, rows)
    sess.set_row_dedup(0)
    legs["d_off_10pct_resent"] = timed(sess, args.iters, args.warmup,
                                       rows + dup_rows)
    sess.close()
    for k in ("c_on_1pct_resent", "d_on_10pct_resent"):
        if legs[k]["sum"] != legs["a_off_no_overlap"]["sum"]:
            raise SystemExit(f"{k}: deduped sum differs from the plain part")

    # ---- part 2: every block partially superseded ----
    n = 8192
    ts = [T0 + i * STRIDE for i in range(n)]
    vals = [(i * 37) % 1000 for i in range(n)]
    v_a = [1] * n
    v_b = [2 if i % 2 == 0 else 0 for i in range(n)]
    b2 = ba.PartBuilder()
    pairs = args.partial_blocks // 2
    for p in range(pairs):
        b2.add_block_i64(p + 1, ts, v_a, vals)
    for p in range(pairs):
        b2.add_block_i64(p + 1, ts, v_b, vals)
    sess2 = ba.Session(0)
    sess2.upload_part(b2)
    sess2.configure(ba.VT_INT64, [ba.AGG_SUM, ba.AGG_COUNT])
    sess2.set_row_dedup(0)
    e_off = timed(sess2, args.iters, args.warmup, 2 * pairs * n)
    sess2.set_row_dedup(1)
    e_on = timed(sess2, args.iters, args.warmup, pairs * n)
    sess2.close()
    nb2 = 2 * pairs
    if e_on["dedup_stats"] != [nb2, nb2, 0, pairs * n]:
        raise SystemExit("part 2: not every block is partial: %r"
                         % (e_on["dedup_stats"],))
    per_block = {
        "build_decode_mark_plus_host": 1e3 * e_on["build_ms"] / nb2,
        "apply_plus_host": 1e3 * ((e_on["wall_ms_median"] -
                                   e_on["kernel_ms_median"]) -
                                  (e_off["wall_ms_median"] -
                                   e_off["kernel_ms_median"])) / nb2,
        "scan_bitmap_walker": 1e3 * e_on["kernel_ms_median"] / nb2,
        "scan_dedup_off": 1e3 * e_off["kernel_ms_median"] / nb2,
    }

    a = legs["a_off_no_overlap"]["kernel_ms_median"]
    out = {
        "tool": "tools/row_dedup_bench.py",
        "iters": args.iters, "warmup": args.warmup,
        "part": {"series": n_series, "datapoints_per_series": n_dp,
                 "blocks": n_blocks, "resent_blocks_1pct": n_dup1,
                 "resent_blocks_10pct": n_dup10,
                 "generate_upload_s": round(gen_s, 1)},
        "legs": legs,
        "kernel_ms_over_a": {k: v["kernel_ms_median"] / a
                             for k, v in legs.items()},
        "wall_ms_over_a": {k: v["wall_ms_median"] /
                           legs["a_off_no_overlap"]["wall_ms_median"]
                           for k, v in legs.items()},
        "all_partial_part": {"blocks": nb2, "rows_per_block": n,
                             "e_off": e_off, "e_on": e_on,
                             "per_block_us": per_block},
    }
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
