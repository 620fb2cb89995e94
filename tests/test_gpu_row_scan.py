"""GPU parity of the time-ordered row scan (bydb_rows_configure /
bydb_rows_finalize): Scan -> Limit.

Expected side: tests/row_scan_ref.py — the rows that row_dedup_ref, the
filter models and the clamp leave, sorted by (ts in the requested direction,
series_id unsigned, seq) and cut to [offset, offset + limit).  Every case
compares all six fields of every returned row, bit for bit (value_f through
its IEEE-754 bytes; the restore comes from the oracle on the row's own
mantissa and exponent)."""
import random
import struct
import subprocess

import pytest

import banyandb_amd as ba
from banyandb_amd import (Session, PartBuilder, TagCond, VT_INT64, VT_FLOAT64,
                          AGG_SUM, AGG_COUNT, AGG_MIN, AGG_MAX, OP_EQ, OP_IN,
                          INT64_MIN, INT64_MAX, FLOAT_RAW_EXP)
import clamp_cases as cc
import row_dedup_cases as rdc
import row_scan_ref as ref
import top_rows_ref as trr
from row_dedup_cases import DBlk, Scen, T0, MS
from test_row_scan_cpu import build_consumer

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
    """One session, one row-scan epoch per (offset, limit, desc)."""
    s, vt, fe = open_session(scen, dedup)
    out = []
    try:
        for offset, limit, desc in queries:
            s.configure_rows(vt, offset, limit, desc, float_exp=fe)
            consume(s, scen)
            out.append([norm(r.astuple()) for r in s.scan_rows()])
    finally:
        s.close()
    return out


def check(scen, queries, dedup=0):
    """Engine against model for every query; returns rows compared."""
    got = engine(scen, queries, dedup)
    compared = 0
    for (offset, limit, desc), g in zip(queries, got):
        want = [norm(r.astuple()) for r in ref.scen_scan_rows(
            scen, offset, limit, desc, dedup=bool(dedup))]
        assert len(g) == len(want), (offset, limit, desc, len(g), len(want))
        for i, (a, b) in enumerate(zip(g, want)):
            assert a == b, ("row", i, "window", offset, limit, "desc", desc,
                            a, b)
        compared += len(want)
    return compared


def both_ways(windows):
    return [(o, l, desc) for o, l in windows for desc in BOTH]


# ---- the window boundary inside a tie group ----
def shuffled_series(rng, n):
    sids = list(range(1, n + 1))
    rng.shuffle(sids)
    if n > 2 and sids == sorted(sids):
        sids.reverse()
    return sids


def test_boundary_inside_a_tie_group_forty_series_two_blocks_each():
    """Every timestamp is shared by 40 series (and by two blocks of each):
    the 12 best rows lie inside one timestamp's tie group, which only the
    series word — and, dedup off, the block index — can order."""
    rng = random.Random(6100)
    ts = rdc.arith_ts(70)
    blocks = [DBlk(sid, ts, [1 + rep] * 70, rdc.ivals(rng, 70))
              for rep in range(2) for sid in shuffled_series(rng, 40)]
    scen = Scen(blocks)
    assert check(scen, both_ways([(5, 7)]), dedup=0) == 14
    assert check(scen, both_ways([(5, 7)]), dedup=1) == 14
    got = engine(scen, [(5, 7, False)], dedup=1)[0]
    assert [g[0] for g in got] == list(range(6, 13))
    assert all(g[1] == ts[0] and g[2] == 2 for g in got)


@pytest.mark.parametrize("n_blocks", [1, 63, 64, 65, 129])
def test_boundary_inside_a_tie_group_block_counts(n_blocks):
    rng = random.Random(6110 + n_blocks)
    ts = rdc.arith_ts(70)
    blocks = [DBlk(sid, ts, [1] * 70, rdc.ivals(rng, 70))
              for sid in shuffled_series(rng, n_blocks)]
    scen = Scen(blocks)
    assert check(scen, both_ways([(5, 7), (0, 1), (60, 70)])) > 0


def test_one_block_of_8192_rows():
    rng = random.Random(6120)
    n = 8192
    blocks = [DBlk(9, rdc.arith_ts(n), [1] * n, rdc.ivals(rng, n)),
              DBlk(4, rdc.arith_ts(3, T0 + 100 * MS), [1] * 3, [7, 8, 9])]
    scen = Scen(blocks)
    check(scen, both_ways([(5, 7), (95, 12), (0, 1024)]))
    check(Scen(blocks[:1]), both_ways([(5, 7), (1000, 24)]))


# ---- key extremes ----
def test_negative_and_positive_timestamps_and_series_extremes():
    rng = random.Random(6200)
    sids = [0x0100, 0x0101, 0x01FF,                       # lowest byte only
            0x0100000000000100, 0x0200000000000100,       # highest byte only
            0x7F00000000000100,
            (1 << 63) - 1, 1 << 63, (1 << 63) + 1, (1 << 64) - 1, 1]
    rng.shuffle(sids)
    far = (1 << 62) - 1                  # a delta still fits an int64
    axes = [[-3 * MS, -2 * MS, -1, 0, 1, 2 * MS, 3 * MS],
            [-far, -2 * MS, 0, 3 * MS, far],
            [-1, 0, 1]]
    blocks = []
    for i, sid in enumerate(sids):
        ts = axes[i % len(axes)]
        blocks.append(DBlk(sid, ts, [1] * len(ts), rdc.ivals(rng, len(ts))))
    scen = Scen(blocks)
    total = scen.n_rows
    assert check(scen, both_ways([(0, 5), (3, 9), (0, total), (total - 4, 9)]))
    got = engine(scen, [(0, 1024, False)])[0]
    at_zero = [g[0] for g in got if g[1] == 0]
    assert at_zero == sorted(sids)          # unsigned, ascending
    assert got[0][1] == -far and got[-1][1] == far


# ---- timestamp sources ----
def ts_source_blocks(rng):
    n = 300
    irregular = rdc.irregular_ts(rng, n)
    return [
        DBlk(5, [T0 + 40 * MS], [7], [11]),                          # Const
        DBlk(6, [T0 + 41 * MS], [1], [12]),                          # Const
        DBlk(2, rdc.arith_ts(n, step=3 * MS), [4] * n, rdc.ivals(rng, n)),
        DBlk(3, irregular, rdc.mixed_versions(rng, n), rdc.ivals(rng, n)),
        DBlk(4, irregular, rdc.rising_versions(rng, n), rdc.ivals(rng, n),
             raw_delta_ts=True),
        DBlk(1, rdc.arith_ts(n), rdc.mixed_versions(rng, n),
             rdc.ivals(rng, n)),
    ]


def test_timestamp_sources_and_clamps():
    rng = random.Random(6300)
    blocks = ts_source_blocks(rng)
    part = Scen(blocks).part()
    descs = part.blocks()
    tcs = [d.ts_enc_with_version - 4 if d.ts_enc_with_version >= 5
           else d.ts_enc_with_version for d in descs]
    assert tcs == [rdc.ENC_CONST, rdc.ENC_CONST, rdc.ENC_DELTA_CONST,
                   rdc.ENC_DOD, rdc.ENC_DELTA, rdc.ENC_DELTA_CONST]
    irregular = blocks[3].ts
    windows = both_ways([(0, 9), (4, 30), (0, 1024)])
    check(Scen(blocks), windows)
    # cuts every list inside, on a row and between rows
    for lo, hi in ((irregular[17], irregular[250]),
                   (irregular[17] + 1, irregular[250] - 1),
                   (T0 + 40 * MS, T0 + 41 * MS),
                   (T0 + 100 * MS + 1, T0 + 500 * MS - 1)):
        check(Scen(blocks, min_ts=lo, max_ts=hi), windows)


def test_clamp_that_leaves_one_row_and_one_that_leaves_none():
    rng = random.Random(6310)
    blocks = ts_source_blocks(rng)
    irregular = blocks[3].ts
    gap = next(t for t, u in zip(irregular, irregular[1:]) if u - t > MS)
    last = max(b.ts[-1] for b in blocks)
    only_dod = next(t for t in irregular[100:]
                    if (t - T0) % (3 * MS) and t > T0 + 300 * MS)
    for coded in (blocks[3], blocks[4]):        # DeltaOfDelta, Delta
        one = Scen([blocks[2], coded, blocks[0]], min_ts=only_dod,
                   max_ts=only_dod)
        assert len(ref.scen_scan_rows(one, 0, 10)) == 1
        assert check(one, both_ways([(0, 10), (0, 1), (1, 1)])) == 4
    both = Scen(blocks, min_ts=last, max_ts=INT64_MAX)
    assert len(ref.scen_scan_rows(both, 0, 10)) == 2    # the last row, twice
    check(both, both_ways([(0, 10), (1, 3)]))
    none = Scen(blocks[2:], min_ts=gap + 1, max_ts=gap + 1)
    assert ref.scen_scan_rows(none, 0, 10) == []
    assert engine(none, both_ways([(0, 10)])) == [[], []]
    assert engine(Scen(blocks, min_ts=last + 1), both_ways([(0, 10)])) == \
        [[], []]


# ---- walkers: each kind, ascending and descending ----
WALKERS = [c for c in rdc.CASES
           if c[0] in ("uniform_tag_clear_skip", "equality_pred",
                       "mask_walker", "plain_tag", "three_slots",
                       "or_tree_row_bitmap")]


@pytest.mark.parametrize("name,make", WALKERS, ids=[c[0] for c in WALKERS])
def test_walkers(name, make):
    scen = make()
    windows = both_ways([(0, 6), (5, 7), (40, 100)])
    assert check(scen, windows, dedup=0) > 0
    assert check(scen, windows, dedup=1) > 0


def test_descending_finds_the_last_match_behind_a_forward_cursor():
    """A multi-run dictionary column: the last matching row of each block
    lies behind many runs, and differs from block to block."""
    n = 400
    ts = rdc.arith_ts(n)
    blocks = []
    for s, last in enumerate((399, 64, 63, 0, 200, 398)):
        col = [rdc.ENVS[(r // 5) % 2] for r in range(n)]     # prod / other
        col = [b"qa" if v == b"prod" else v for v in col]
        for r in (last, last // 2):
            col[r] = b"prod"
        blocks.append(DBlk(s + 1, ts, [1] * n, list(range(s * n, s * n + n)),
                           [col]))
    scen = Scen(blocks, conds=[TagCond(0, OP_EQ, [b"prod"])])
    assert check(scen, both_ways([(0, 3), (2, 6), (0, 100)])) > 0
    got = engine(scen, [(0, 2, True)])[0]
    assert [(g[0], g[1]) for g in got] == [(1, ts[399]), (6, ts[398])]


SELECTION = [c for c in rdc.CASES if c[0].startswith("clamp_")
             or c[0] in ("middle_third", "three_versions", "varying_versions",
                         "identical_65_high_second", "delta_x_delta",
                         "dod_x_arith1", "one_row_x_delta",
                         "different_series")]


@pytest.mark.parametrize("name,make", SELECTION, ids=[c[0] for c in SELECTION])
def test_selection_paths(name, make):
    scen = make()
    check(scen, [(0, 5, False), (3, 100, True)], dedup=0)
    check(scen, [(0, 5, True), (3, 100, False)], dedup=1)


@pytest.mark.parametrize("shape", ["two_byte", "mixed", "wide", "ten_byte"])
def test_wide_varint_timestamps(shape):
    scen = rdc.wide_varint_case(shape, 6510)()
    check(scen, both_ways([(0, 3), (2, 1022)]))
    check(scen, both_ways([(0, 3), (2, 1022)]), dedup=1)


# ---- dedup ----
def late_correction():
    ts = rdc.arith_ts(80)
    a = DBlk(1, ts, [1] * 80, list(range(80)))
    other = DBlk(2, ts, [1] * 80, list(range(1000, 1080)))
    b = DBlk(1, [ts[33]], [2], [-5])
    return Scen([a, other, b]), ts


def test_dedup_on_a_late_correction_surfaces_once():
    scen, ts = late_correction()
    check(scen, both_ways([(0, 1024), (60, 10)]), dedup=1)
    got = engine(scen, [(0, 1024, False)], dedup=1)[0]
    hit = [g for g in got if g[0] == 1 and g[1] == ts[33]]
    assert [(g[2], g[3], g[5]) for g in hit] == [(2, -5, 2 << 13)]
    assert len(got) == 160


def test_dedup_off_both_rows_surface_in_seq_order():
    scen, ts = late_correction()
    check(scen, both_ways([(0, 1024), (60, 10)]), dedup=0)
    for desc in BOTH:
        got = engine(scen, [(0, 1024, desc)], dedup=0)[0]
        hit = [g for g in got if g[0] == 1 and g[1] == ts[33]]
        assert [(g[2], g[3], g[5]) for g in hit] == \
            [(1, 33, 33), (2, -5, 2 << 13)]
        assert len(got) == 161


def test_dedup_higher_version_failing_the_filter_hides_the_lower():
    ts = rdc.arith_ts(10)
    a = DBlk(1, ts, [1] * 10, [100 + i for i in range(10)],
             [[b"prod"] * 10])
    b = DBlk(1, [ts[9]], [2], [7], [[b"dev"]])
    scen = Scen([a, b], conds=[TagCond(0, OP_EQ, [b"prod"])])
    check(scen, both_ways([(0, 20), (1, 3)]), dedup=1)
    assert engine(scen, [(0, 1, True)], dedup=1)[0][0][3] == 108
    assert engine(scen, [(0, 1, True)], dedup=0)[0][0][3] == 109


def test_dedup_fully_superseded_block():
    scen = rdc.identical_case(129, False)()
    check(scen, both_ways([(0, 200), (100, 50)]), dedup=1)
    got = engine(scen, [(0, 1024, False)], dedup=1)[0]
    assert len(got) == 129 and all(g[5] >> 13 == 1 for g in got)


# ---- window ----
def test_window_edges():
    rng = random.Random(6600)
    blocks = [DBlk(s + 1, rdc.arith_ts(20, T0 + s * MS), [1] * 20,
                   rdc.ivals(rng, 20)) for s in range(3)]
    scen = Scen(blocks)
    assert engine(scen, both_ways([(60, 5), (1000, 24)])) == [[]] * 4
    assert check(scen, both_ways([(55, 10)])) == 10       # the tail, 5 rows
    assert check(scen, both_ways([(59, 1), (0, 60), (0, 61)])) == 2 * 121
    s, vt, fe = open_session(scen)
    try:
        s.configure_rows(vt, 7, 0)
        s.consume()
        assert s.scan_rows() == []
        s.configure_rows(vt, 0, 0, desc=True)
        s.consume()
        assert s.scan_rows() == []
    finally:
        s.close()


def test_n_1024_over_1100_blocks_of_3_rows():
    rng = random.Random(6610)
    blocks = []
    for b in range(1100):
        t0 = T0 + rng.randrange(0, 400) * MS
        blocks.append(DBlk(1 + rng.randrange(50), [t0, t0 + MS, t0 + 5 * MS],
                           [1 + b] * 3, rdc.ivals(rng, 3)))
    scen = Scen(blocks)
    assert check(scen, both_ways([(0, 1024), (1000, 24)])) == 2 * 1048
    assert check(scen, [(24, 1000, True)], dedup=1) == 1000


# ---- field values ----
def test_float_mixed_block_exponents():
    rng = random.Random(6700)
    blocks = [DBlk(1, rdc.arith_ts(3), [1] * 3, [0.5, 1.5, 0.25 * 2]),
              DBlk(2, rdc.arith_ts(3), [1] * 3, [1.25, 1.50, 0.75]),
              DBlk(3, rdc.arith_ts(2), [1] * 2, [3.0, 1.0]),
              DBlk(4, rdc.arith_ts(150), [1] * 150, rdc.fvals(rng, 150))]
    scen = Scen(blocks, kind=rdc.F64)
    part = scen.part()
    assert [d.exp for d in part.blocks()][:3] == [-1, -2, 0]
    check(scen, both_ways([(0, 4), (2, 9), (0, 1024)]))
    got = engine(scen, [(0, 3, False)])[0]
    # value_i is the mantissa in the row's own block exponent
    assert [(g[0], g[3], struct.unpack("<d", g[4])[0]) for g in got] == \
        [(1, 5, 0.5), (2, 125, 1.25), (3, 3, 3.0)]


def test_float_two_parts_with_dedup():
    scen = rdc.float_case()
    check(scen, both_ways([(0, 7), (30, 200)]), dedup=0)
    check(scen, both_ways([(0, 7), (30, 200)]), dedup=1)


def test_int64_field_encodings():
    rng = random.Random(6710)
    n = 300
    kinds = {"const": rdc.ENC_CONST, "delta_const": rdc.ENC_DELTA_CONST,
             "dense": rdc.ENC_DELTA, "multi_byte": rdc.ENC_DELTA,
             "dod": rdc.ENC_DOD}
    blocks, want_enc = [], []
    for kind, enc in kinds.items():
        blocks.append(DBlk(len(blocks) + 1, rdc.arith_ts(n), [1] * n,
                           cc.field_values(rng, kind, n)))
        want_enc.append((kind, enc))
    scen = Scen(blocks)
    part = scen.part()
    for d, (kind, enc) in zip(part.blocks(), want_enc):
        assert d.field_enc == enc, kind
        if kind == "dense":
            assert d.field_len == d.count - 1
        if kind == "multi_byte":
            assert d.field_len > d.count - 1
    check(scen, both_ways([(0, 10), (700, 300), (1010, 14)]))


# ---- errors and state ----
def nullable_part():
    """Block 0 plain int64, block 1 null-bearing, later in time."""
    pb = PartBuilder()
    pb.add_block_i64(1, rdc.arith_ts(50), [1] * 50, list(range(50)))
    pb.add_block_i64_nullable(2, rdc.arith_ts(50, T0 + 1000 * MS), [1] * 50,
                              [None if i % 3 == 0 else i for i in range(50)])
    return pb


def test_nullable_block_selected_is_loud_clamped_out_is_not():
    s = Session(0)
    try:
        s.upload_part(nullable_part())
        s.configure_rows(VT_INT64, 0, 3, desc=True)
        s.consume(T0, T0 + 49 * MS)
        assert [r.value_i for r in s.scan_rows()] == [49, 48, 47]
        s.consume()
        with pytest.raises(RuntimeError, match="decode error 7"):
            s.scan_rows()
        s.reset()
        s.consume(T0, T0 + 49 * MS)
        assert [r.value_i for r in s.scan_rows()] == [49, 48, 47]
    finally:
        s.close()


def test_second_consume_is_state_and_reset_clears_it():
    scen = Scen([DBlk(1, rdc.arith_ts(10), [1] * 10, list(range(10)))])
    s, vt, fe = open_session(scen)
    try:
        s.configure_rows(vt, 1, 2)
        s.consume()
        with pytest.raises(RuntimeError, match="rc=%d" % STATE):
            s.consume()
        s.reset()
        s.consume()
        assert [r.value_i for r in s.scan_rows()] == [1, 2]
        s.consume()                       # finalize closed the epoch
        assert [r.value_i for r in s.scan_rows()] == [1, 2]
    finally:
        s.close()


def test_bad_arg_leaves_the_configuration_unchanged():
    scen = Scen([DBlk(1, rdc.arith_ts(10), [1] * 10, list(range(10)))])
    s, vt, fe = open_session(scen)
    lib = ba.lib()
    try:
        s.configure_rows(vt, 2, 3, desc=True)
        for args in ((vt, -1, 3, 0), (vt, 0, -1, 0), (vt, 1, 1024, 0),
                     (vt, 1025, 0, 0), (vt, 0, 3, 2), (vt, 0, 3, -1),
                     (99, 0, 3, 0)):
            assert lib.bydb_rows_configure(s._h, *args) == BAD_ARG, args
        lib.bydb_set_float_exp(s._h, FLOAT_RAW_EXP)
        assert lib.bydb_rows_configure(s._h, VT_FLOAT64, 0, 3, 0) == BAD_ARG
        lib.bydb_set_float_exp(s._h, 0)
        s.consume()
        assert [r.value_i for r in s.scan_rows()] == [7, 6, 5]
        # a top session says so, and a row-scan session is no top session
        s.top_n = 3
        with pytest.raises(RuntimeError, match="rc=%d" % STATE):
            s.top_rows()
        s.configure_top(vt, 2)
        s.consume()
        with pytest.raises(RuntimeError, match="rc=%d" % STATE):
            s.scan_rows()
    finally:
        s.close()


def test_aggregate_after_a_row_scan_epoch_and_back():
    scen = rdc.mask_walker_case()
    funcs = [AGG_SUM, AGG_COUNT, AGG_MIN, AGG_MAX]
    s, vt, fe = open_session(scen)

    def aggregate(finalize=True):
        s.configure(vt, funcs)
        consume(s, scen)
        if not finalize:
            return None
        g = s.finalize()[0]
        return (g.count, g.sum_i, g.min_i, g.max_i)
    try:
        before = aggregate()
        aggregate(finalize=False)         # an open aggregate epoch ...
        s.configure_rows(vt, 0, 10)       # ... ends here, and is not returned
        assert s.finalize()[0].count == 0
        consume(s, scen)
        rows = s.scan_rows()
        assert [norm(r.astuple()) for r in rows] == \
            [norm(r.astuple()) for r in ref.scen_scan_rows(scen, 0, 10)]
        assert s.last_consume_ms() > 0
        assert aggregate() == before
    finally:
        s.close()


def test_top_and_row_scan_alternate_on_one_session():
    """The two operators share their scratch; the row grid is resized when
    the shapes differ (5 / 256 / 300 slots)."""
    scen = rdc.three_slot_case()
    s, vt, fe = open_session(scen, dedup=1)
    try:
        for n in (5, 300, 256, 5):
            s.configure_top(vt, n)
            consume(s, scen)
            got = [norm(r.astuple()) for r in s.top_rows()]
            want = trr.scen_top_rows(scen, n, False, dedup=True)
            assert got == [norm(r.astuple()) for r in want], n
            for desc in BOTH:
                s.configure_rows(vt, 2, n - 2, desc)
                consume(s, scen)
                got = [norm(r.astuple()) for r in s.scan_rows()]
                want = ref.scen_scan_rows(scen, 2, n - 2, desc, dedup=True)
                assert got == [norm(r.astuple()) for r in want], (n, desc)
    finally:
        s.close()


# ---- seeded random leg ----
FIELD_KINDS = ("ivals",) + cc.FIELD_KINDS
RANDOM_CHUNK = 25
RANDOM_BASES = tuple(range(7200, 7200 + 10 * RANDOM_CHUNK, RANDOM_CHUNK))


def random_row_scan_scenario(seed):
    """row_dedup_cases.random_scenario (timestamp / version encodings,
    filter kinds, clamps, parts) with a field encoding drawn per block."""
    scen = rdc.random_scenario(seed)
    assert scen.kind == rdc.I64          # nullable kinds never generated
    rng = random.Random(seed ^ 0x5CA7)
    for b in scen.blocks:
        kind = rng.choice(FIELD_KINDS)
        if kind != "ivals":
            b.vals = cc.field_values(rng, kind, len(b.ts))
    total = scen.n_rows
    queries = []
    for _ in range(2):
        offset = rng.choice([0, 0, 1, 5, 63, 64, total // 2, total + 3])
        offset = min(offset, 1000)
        limit = rng.choice([1, 2, 7, 64, 65, 300, 1024])
        queries.append((offset, min(limit, 1024 - offset),
                        rng.random() < 0.5))
    return scen, queries, rng.randrange(2)


@pytest.mark.parametrize(
    "base", RANDOM_BASES,
    ids=["seeds_%d_%d" % (b, b + RANDOM_CHUNK - 1) for b in RANDOM_BASES])
def test_random_scenarios(base):
    compared = 0
    for seed in range(base, base + RANDOM_CHUNK):
        scen, queries, dedup = random_row_scan_scenario(seed)
        try:
            compared += check(scen, queries, dedup)
        except AssertionError as e:
            raise AssertionError("seed %d dedup %d: %s" % (seed, dedup, e))
    assert compared > 10 * RANDOM_CHUNK


# ---- shards ----
def test_three_time_bucket_shards_merge_to_the_single_session_answer():
    rng = random.Random(6900)
    n = 240
    series = []
    for sid in (7, 3, 5, 1 << 63):
        ts = rdc.irregular_ts(rng, n) if sid == 3 else rdc.arith_ts(n)
        series.append((sid, ts, rdc.ivals(rng, n),
                       rdc.env_runs(rng, n, nil_p=0.0)))
    cuts = [INT64_MIN, T0 + 70 * MS, T0 + 165 * MS, INT64_MAX]
    shards = []
    for a, b in zip(cuts, cuts[1:]):
        shard = []
        for sid, ts, vals, col in series:
            rows = [r for r in range(n) if a <= ts[r] < b]
            if rows:
                shard.append(DBlk(sid, [ts[r] for r in rows], [1] * len(rows),
                                  [vals[r] for r in rows],
                                  [[col[r] for r in rows]]))
        shards.append(shard)
    assert all(len(shard) == 4 for shard in shards)
    conds = [TagCond(0, OP_IN, [b"prod", b"qa"])]
    union = Scen([blk for shard in shards for blk in shard], conds=conds)
    for desc in BOTH:
        for offset, limit in ((0, 10), (37, 50), (300, 400)):
            lists = [engine(Scen(shard, conds=conds),
                            [(0, offset + limit, desc)])[0]
                     for shard in shards]
            rows = [[ba.TopRow(g[0], g[1], g[2], g[3],
                               struct.unpack("<d", g[4])[0], g[5])
                     for g in lst] for lst in lists]
            merged = ba.rows_merge(rows, offset, limit, desc)
            want = engine(union, [(offset, limit, desc)])[0]
            # seq is shard-local: compare the other five fields
            assert [norm(r.astuple())[:5] for r in merged] == \
                [w[:5] for w in want]
            assert len(want) == len(ref.scen_scan_rows(union, offset, limit,
                                                       desc))
    check(union, both_ways([(37, 50)]))


# ---- the pure-C consumer ----
def test_c_consumer_runs(tmp_path):
    exe = str(tmp_path / "cabi_row_scan_check")
    build_consumer(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "row scan consumer OK" in r.stdout
