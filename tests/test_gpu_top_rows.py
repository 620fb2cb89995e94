"""GPU parity of the raw-row top-N (bydb_top_configure / bydb_top_finalize).

Expected side: tests/top_rows_ref.py — the rows that row_dedup_ref, the
filter models and the clamp leave, in storage order, through BatchTop's own
bounded heap.  Every case compares all six fields of every returned row,
bit for bit (value_f through its IEEE-754 bytes; the restore comes from the
oracle on the row's own mantissa and exponent)."""
import json
import os
import random
import struct
import subprocess

import pytest

import banyandb_amd as ba
from banyandb_amd import (Session, PartBuilder, TagCond, VT_INT64, VT_FLOAT64,
                          AGG_SUM, AGG_COUNT, AGG_MIN, AGG_MAX, OP_EQ,
                          INT64_MIN, INT64_MAX, FLOAT_RAW_EXP)
import clamp_cases as cc
import row_dedup_cases as rdc
import top_rows_ref as ref
from row_dedup_cases import DBlk, Scen, T0, MS
from test_top_rows_cpu import GOLDEN, build_consumer

pytestmark = pytest.mark.gpu

BAD_ARG, STATE = -3, -5
BOTH = (False, True)


def norm(t):
    """A row tuple with value_f as its bytes: bit-exact comparison."""
    return t[:4] + (struct.pack("<d", t[4]),) + t[5:]


def is_float(scen):
    return scen.kind == rdc.F64


def consume(s, scen):
    lo = INT64_MIN if scen.min_ts is None else scen.min_ts
    hi = INT64_MAX if scen.max_ts is None else scen.max_ts
    if scen.tree is not None:
        s.consume_filter_tree(scen.tree, lo, hi)
    elif scen.conds is not None:
        s.consume_filter(scen.conds, lo, hi)
    elif scen.pred is not None:
        s.consume(lo, hi, pred=scen.pred)
    else:
        s.consume(lo, hi)


def open_session(scen, dedup=0):
    part = scen.part()
    s = Session(0)
    s.upload_part(part)
    s.set_row_dedup(dedup)
    fe = min(d.exp for d in part.blocks()) if is_float(scen) else 0
    return s, (VT_FLOAT64 if is_float(scen) else VT_INT64), fe


def engine(scen, queries, dedup=0):
    """One session, one top epoch per (n, asc) of `queries`."""
    s, vt, fe = open_session(scen, dedup)
    out = []
    try:
        for n, asc in queries:
            s.configure_top(vt, n, asc, float_exp=fe)
            consume(s, scen)
            out.append([norm(r.astuple()) for r in s.top_rows()])
    finally:
        s.close()
    return out


def check(scen, queries, dedup=0):
    """Engine against model for every query; returns rows compared."""
    got = engine(scen, queries, dedup)
    compared = 0
    for (n, asc), g in zip(queries, got):
        want = [norm(r.astuple())
                for r in ref.scen_top_rows(scen, n, asc, dedup=bool(dedup))]
        assert len(g) == len(want), (n, asc, len(g), len(want))
        for i, (a, b) in enumerate(zip(g, want)):
            assert a == b, ("row", i, "n", n, "asc", asc, a, b)
        compared += len(want)
    return compared


def both_ways(ns):
    return [(n, asc) for n in ns for asc in BOTH]


# ---- the reference's own vectors, one block each ----
def golden_cases():
    with open(GOLDEN) as f:
        return [c for c in json.load(f)["cases"] if None not in c["values"]]


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_golden_vectors_through_the_engine(case):
    vals = case["values"]
    scen = Scen([DBlk(7, rdc.arith_ts(len(vals)), [1] * len(vals), vals)])
    got = engine(scen, [(case["n"], case["asc"])])[0]
    assert [g[3] for g in got] == case["want"]
    assert [g[5] for g in got] == case["want_input_rows"]
    check(scen, [(case["n"], case["asc"])])


# ---- block lengths x N ----
@pytest.mark.parametrize("rows", [1, 2, 63, 64, 65, 129, 8192])
def test_block_lengths_and_n(rows):
    rng = random.Random(5100 + rows)
    blocks = [DBlk(s + 1, rdc.arith_ts(rows), [1] * rows,
                   [rng.randint(-40, 40) for _ in range(rows)])
              for s in range(2)]
    total = 2 * rows
    ns = sorted(n for n in {1, 2, 63, 64, 65, total, total + 1, 1024}
                if n <= ba.TOP_ROWS_MAX)
    assert check(Scen(blocks), both_ways(ns)) > 0


def test_n_zero_returns_nothing_and_limits_are_bad_arg():
    scen = Scen([DBlk(1, rdc.arith_ts(10), [1] * 10, list(range(10)))])
    s, vt, fe = open_session(scen)
    lib = ba.lib()
    try:
        s.configure_top(vt, 0)
        s.consume()
        assert s.top_rows() == []
        assert lib.bydb_top_configure(s._h, vt, 1025, 0) == BAD_ARG
        assert lib.bydb_top_configure(s._h, vt, -1, 0) == BAD_ARG
        assert lib.bydb_top_configure(s._h, 99, 3, 0) == BAD_ARG
        lib.bydb_set_float_exp(s._h, FLOAT_RAW_EXP)
        assert lib.bydb_top_configure(s._h, VT_FLOAT64, 3, 0) == BAD_ARG
        lib.bydb_set_float_exp(s._h, 0)
        # still the n = 0 top session it was, and still usable
        s.consume()
        assert s.top_rows() == []
        s.configure_top(vt, 3)
        s.consume()
        assert [r.value_i for r in s.top_rows()] == [9, 8, 7]
    finally:
        s.close()


# ---- more blocks than one selector chunk ----
def test_thousands_of_small_blocks_cross_the_chunk_scan():
    rng = random.Random(5200)
    blocks = []
    for b in range(3000):
        n = 1 + (b % 2)
        blocks.append(DBlk(b + 1, rdc.arith_ts(n, T0 + b * MS), [1] * n,
                           [rng.randint(-6, 6) for _ in range(n)]))
    assert check(Scen(blocks), both_ways([1, 100, 1024])) > 0


# ---- ties ----
def test_all_equal_cut_inside_the_second_block():
    blocks = [DBlk(s + 1, rdc.arith_ts(100), [1] * 100, [5] * 100)
              for s in range(3)]
    scen = Scen(blocks)
    check(scen, both_ways([150]))
    got = engine(scen, [(150, False)])[0]
    assert [g[5] for g in got] == list(range(100)) + \
        [(1 << 13) | r for r in range(50)]


def test_five_blocks_share_the_best_value_first_two_win():
    rng = random.Random(5300)
    blocks = []
    for s in range(5):
        vals = [rng.randint(0, 50) for _ in range(70)]
        vals[rng.randrange(70)] = 99
        blocks.append(DBlk(s + 1, rdc.arith_ts(70), [1] * 70, vals))
    scen = Scen(blocks)
    check(scen, [(2, False)])
    got = engine(scen, [(2, False)])[0]
    assert [g[5] >> 13 for g in got] == [0, 1]
    lows = Scen([DBlk(b.sid, b.ts, b.vers, [-v for v in b.vals])
                 for b in blocks])
    check(lows, [(2, True)])


def test_values_from_minus_one_zero_one():
    rng = random.Random(5301)
    blocks = [DBlk(s + 1, rdc.arith_ts(n), [1] * n,
                   [rng.choice([-1, 0, 1]) for _ in range(n)])
              for s, n in enumerate((65, 300, 1, 129, 64))]
    check(Scen(blocks), both_ways([1, 7, 64, 200, 1024]))


# ---- field encodings and value extremes ----
def test_field_encodings():
    rng = random.Random(5400)
    n = 300
    kinds = {"const": rdc.ENC_CONST, "delta_const": rdc.ENC_DELTA_CONST,
             "dense": rdc.ENC_DELTA, "multi_byte": rdc.ENC_DELTA,
             "dod": rdc.ENC_DOD}
    blocks, want_enc = [], []
    for rep in range(2):
        for kind, enc in kinds.items():
            blocks.append(DBlk(len(blocks) + 1, rdc.arith_ts(n), [1] * n,
                               cc.field_values(rng, kind, n)))
            want_enc.append((kind, enc))
    # Delta with varints of every length from 2 to 10 bytes
    steps = [1 << (7 * k + 3) for k in range(1, 9)] + [1 << 62]
    v, mixed = 0, [0]
    for i in range(n - 1):
        v = cc.wrap64(v + rng.choice(steps) * rng.choice([-1, 1]))
        mixed.append(v)
    blocks.append(DBlk(len(blocks) + 1, rdc.arith_ts(n), [1] * n, mixed))
    want_enc.append(("mixed", rdc.ENC_DELTA))
    scen = Scen(blocks)
    part = scen.part()            # keeps the descriptors alive
    descs = part.blocks()
    for d, (kind, enc) in zip(descs, want_enc):
        assert d.field_enc == enc, kind
        if kind == "dense":
            assert d.field_len == d.count - 1
        if kind in ("multi_byte", "mixed"):
            assert d.field_len > d.count - 1
    lens = set(cc.varint_lengths(bytes(
        part.payload[descs[-1].field_off:
                     descs[-1].field_off + descs[-1].field_len])))
    assert set(range(2, 11)) <= lens, lens
    check(scen, both_ways([1, 10, 700]))


def test_value_extremes_negatives_and_wrapping_deltas():
    hi, lo = INT64_MAX, INT64_MIN
    shapes = [
        [hi, lo, 0, -1, lo + 1, hi - 1, 5],
        [lo, hi, lo, hi],
        [-5, -4, -3, -9, -1000, -2],
        [hi - 3 + i for i in range(4)] + [lo + i for i in range(60)],
        [lo],
        [hi],
    ]
    blocks = [DBlk(s + 1, rdc.arith_ts(len(v)), [1] * len(v), v)
              for s, v in enumerate(shapes)]
    check(Scen(blocks), both_ways([1, 3, 8, 1024]))


# ---- timestamps and versions of the returned rows ----
def test_timestamp_and_version_encodings():
    rng = random.Random(5500)
    n = 200
    irregular = rdc.irregular_ts(rng, n)
    blocks = [
        DBlk(1, [T0 + 5], [7], [rng.randint(0, 99)]),                # Const
        DBlk(2, rdc.arith_ts(n, step=3 * MS), [4] * n, rdc.ivals(rng, n)),
        DBlk(3, irregular, rdc.mixed_versions(rng, n), rdc.ivals(rng, n)),
        DBlk(4, irregular, rdc.rising_versions(rng, n), rdc.ivals(rng, n),
             raw_delta_ts=True),
        DBlk(5, rdc.arith_ts(n), rdc.mixed_versions(rng, n),
             rdc.ivals(rng, n)),
    ]
    scen = Scen(blocks)
    part = scen.part()
    descs = part.blocks()
    tcs = [d.ts_enc_with_version - 4 if d.ts_enc_with_version >= 5
           else d.ts_enc_with_version for d in descs]
    assert tcs == [rdc.ENC_CONST, rdc.ENC_DELTA_CONST, rdc.ENC_DOD,
                   rdc.ENC_DELTA, rdc.ENC_DELTA_CONST]
    assert [d.version_enc == rdc.ENC_CONST for d in descs] == \
        [True, True, False, False, False]
    check(scen, both_ways([1, 40, 1024]))


@pytest.mark.parametrize("shape", ["two_byte", "mixed", "wide", "ten_byte"])
def test_wide_varint_timestamps(shape):
    scen = rdc.wide_varint_case(shape, 5510)()
    check(scen, both_ways([3, 1024]))
    check(scen, both_ways([3, 1024]), dedup=1)


# ---- float64 ----
def test_float_one_exponent():
    rng = random.Random(5600)
    blocks = [DBlk(s + 1, rdc.arith_ts(n), [1] * n, rdc.fvals(rng, n))
              for s, n in enumerate((300, 65, 1, 129))]
    scen = Scen(blocks, kind=rdc.F64)
    part = scen.part()
    assert len({d.exp for d in part.blocks() if d.count > 1}) == 1
    check(scen, both_ways([1, 9, 1024]))


def test_float_mixed_exponents_tie_goes_to_the_earlier_block():
    blocks = [DBlk(1, rdc.arith_ts(3), [1] * 3, [0.5, 1.5, 0.25 * 2]),
              DBlk(2, rdc.arith_ts(3), [1] * 3, [1.25, 1.50, 0.75]),
              DBlk(3, rdc.arith_ts(2), [1] * 2, [3.0, 1.0])]
    scen = Scen(blocks, kind=rdc.F64)
    part = scen.part()
    assert [d.exp for d in part.blocks()] == [-1, -2, 0]
    check(scen, both_ways([1, 2, 3, 8]))
    got = engine(scen, [(3, False)])[0]
    # 3.0, then 1.5 (mantissa 15 at -1) before 1.50 (150 at -2)
    assert [(g[5] >> 13, g[3]) for g in got] == [(2, 3), (0, 15), (1, 150)]


def test_float_rescale_overflow_is_loud():
    blocks = [DBlk(1, rdc.arith_ts(2), [1] * 2,
                   [1234567890123456.0, 1234567890123457.0]),
              DBlk(2, rdc.arith_ts(2), [1] * 2, [0.0001, 0.0003])]
    scen = Scen(blocks, kind=rdc.F64)
    part = scen.part()
    assert [d.exp for d in part.blocks()] == [0, -4]
    s, vt, fe = open_session(scen)
    try:
        s.configure_top(vt, 2, float_exp=fe)
        s.consume()
        with pytest.raises(RuntimeError, match="decode error 5"):
            s.top_rows()
    finally:
        s.close()


# ---- selection: clamp, verdicts, walkers, bitmaps, trees, dedup ----
def test_clamp_cuts_the_best_row_out():
    vals = list(range(100))
    vals[50] = 10 ** 6
    ts = rdc.arith_ts(100)
    a = DBlk(1, ts, [1] * 100, vals)
    b = DBlk(2, ts, [1] * 100, [v // 2 for v in vals])
    for lo, hi in ((0, 49), (51, 99), (50, 50), (49, 51)):
        check(Scen([a, b], min_ts=ts[lo], max_ts=ts[hi]), both_ways([1, 5]))


SELECTION = [c for c in rdc.CASES if c[0].startswith("clamp_")
             or c[0] in ("uniform_tag_clear_skip", "equality_pred",
                         "mask_walker", "plain_tag", "three_slots",
                         "or_tree_row_bitmap", "middle_third",
                         "three_versions", "varying_versions",
                         "identical_65_high_second", "float64",
                         "delta_x_delta", "dod_x_arith1")]


@pytest.mark.parametrize("name,make", SELECTION, ids=[c[0] for c in SELECTION])
def test_selection_paths(name, make):
    scen = make()
    check(scen, [(5, False), (100, True)], dedup=0)
    check(scen, [(5, True), (100, False)], dedup=1)


def test_dedup_superseded_row_holds_the_maximum():
    ts = rdc.arith_ts(80)
    vals = list(range(80))
    vals[33] = 10 ** 9
    a = DBlk(1, ts, [1] * 80, vals)
    b = DBlk(1, [ts[33]], [2], [-5])
    scen = Scen([a, b])
    check(scen, both_ways([1, 3]), dedup=1)
    assert engine(scen, [(1, False)], dedup=1)[0][0][3] == 79
    assert engine(scen, [(1, False)], dedup=0)[0][0][3] == 10 ** 9


def test_dedup_fully_superseded_block():
    scen = rdc.identical_case(129, False)()
    check(scen, both_ways([1, 200]), dedup=1)
    got = engine(scen, [(1024, False)], dedup=1)[0]
    assert len(got) == 129 and all(g[5] >> 13 == 1 for g in got)


def test_dedup_higher_version_failing_the_filter_hides_the_lower():
    ts = rdc.arith_ts(10)
    a = DBlk(1, ts, [1] * 10, [100 + i for i in range(10)],
             [[b"prod"] * 10])
    b = DBlk(1, [ts[9]], [2], [7], [[b"dev"]])
    scen = Scen([a, b], conds=[TagCond(0, OP_EQ, [b"prod"])])
    check(scen, both_ways([1, 20]), dedup=1)
    assert engine(scen, [(1, False)], dedup=1)[0][0][3] == 108


# ---- state ----
def nullable_part():
    """Block 0 plain int64, block 1 null-bearing, later in time."""
    pb = PartBuilder()
    pb.add_block_i64(1, rdc.arith_ts(50), [1] * 50, list(range(50)))
    pb.add_block_i64_nullable(2, rdc.arith_ts(50, T0 + 1000 * MS), [1] * 50,
                              [None if i % 3 == 0 else i for i in range(50)])
    return pb


def test_second_consume_is_state_and_reset_clears_it():
    scen = Scen([DBlk(1, rdc.arith_ts(10), [1] * 10, list(range(10)))])
    s, vt, fe = open_session(scen)
    try:
        s.configure_top(vt, 2)
        s.consume()
        with pytest.raises(RuntimeError, match="rc=%d" % STATE):
            s.consume()
        s.reset()
        s.consume()
        assert [r.value_i for r in s.top_rows()] == [9, 8]
        s.consume()                       # finalize closed the epoch
        assert [r.value_i for r in s.top_rows()] == [9, 8]
    finally:
        s.close()


def test_nullable_block_selected_is_loud_outside_the_clamp_is_not():
    s = Session(0)
    try:
        s.upload_part(nullable_part())
        s.configure_top(VT_INT64, 3)
        s.consume(T0, T0 + 49 * MS)
        assert [r.value_i for r in s.top_rows()] == [49, 48, 47]
        s.consume()
        with pytest.raises(RuntimeError, match="decode error 7"):
            s.top_rows()
        s.reset()
        s.consume(T0, T0 + 49 * MS)
        assert [r.value_i for r in s.top_rows()] == [49, 48, 47]
    finally:
        s.close()


def test_aggregate_after_a_top_epoch_is_unchanged():
    scen = rdc.mask_walker_case()
    funcs = [AGG_SUM, AGG_COUNT, AGG_MIN, AGG_MAX]
    s, vt, fe = open_session(scen)

    def aggregate():
        s.configure(vt, funcs)
        consume(s, scen)
        g = s.finalize()[0]
        return (g.count, g.sum_i, g.min_i, g.max_i)
    try:
        before = aggregate()
        s.configure_top(vt, 10)
        consume(s, scen)
        assert len(s.top_rows()) == 10
        assert s.last_consume_ms() > 0
        assert aggregate() == before
    finally:
        s.close()


# ---- seeded random leg over the existing generators ----
RANDOM_SEEDS = tuple(range(7100, 7140))


def test_random_scenarios():
    drawn = compared = 0
    for seed in RANDOM_SEEDS:
        scen = rdc.random_scenario(seed)
        assert scen.kind == rdc.I64          # nullable kinds never generated
        rng = random.Random(seed ^ 0x70B)
        queries = [(rng.choice([1, 2, 17, 64, 65, 300, 1024]),
                    rng.random() < 0.5) for _ in range(2)]
        dedup = rng.randrange(2)
        drawn += len(queries)
        check(scen, queries, dedup)
        compared += len(queries)
    assert compared == drawn == 2 * len(RANDOM_SEEDS)


# ---- the pure-C consumer ----
def test_c_consumer_runs(tmp_path):
    exe = str(tmp_path / "cabi_top_rows_check")
    build_consumer(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "top rows consumer OK" in r.stdout
