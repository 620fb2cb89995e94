"""GPU parity of the cross-part version dedup (bydb_set_row_dedup).

Expected side: tests/row_dedup_ref.py says which rows survive (the
reference's queryResult.Less / merge restated per row); the aggregates come
from the existing checkers — filter_ref, filter_tree_ref or
helpers.oracle_scan — over the same blocks with the superseded rows
deleted and the emptied blocks dropped.  count, min, max and the int64 sum
are bit-exact, the float64 sum and mean within rel 1e-9.  Every case also
checks bydb_row_dedup_stats against the model's census."""
import json
import math
import os
import subprocess

import pytest

import banyandb_amd as ba
from banyandb_amd import (Session, TagCond, Or, VT_INT64, VT_FLOAT64,
                          AGG_SUM, AGG_COUNT, AGG_MIN, AGG_MAX, AGG_MEAN,
                          MODE_MAP, OP_EQ, INT64_MIN, INT64_MAX,
                          FLOAT_RAW_EXP)
import filter_ref as fr
import filter_tree_ref as ftr
from helpers import oracle_scan
import row_dedup_cases as rdc
import row_dedup_ref as ref

pytestmark = pytest.mark.gpu

FUNCS = [AGG_SUM, AGG_COUNT, AGG_MIN, AGG_MAX]
BAD_ARG = -3
NEVER = (1 << 64) - 1
GOLDEN = os.path.join(os.path.dirname(__file__), "golden",
                      "query_merge_vectors.json")


def wrap64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def is_float(scen):
    return scen.kind in (rdc.F64, rdc.F64N)


def float_exp(scen, part):
    if scen.kind == rdc.F64N:
        return FLOAT_RAW_EXP
    if scen.kind == rdc.F64:
        return min(d.exp for d in part.blocks())
    return 0


def configure(s, scen, part, funcs=FUNCS, mode=ba.MODE_ALL):
    vt = VT_FLOAT64 if is_float(scen) else VT_INT64
    fe = float_exp(scen, part)
    if scen.group is None:
        s.configure(vt, funcs, mode=mode, float_exp=fe)
    elif scen.group[0] == "code":
        s.configure(vt, funcs, n_groups=scen.group[1], mode=mode,
                    float_exp=fe)
    else:
        s.configure_by_tag(vt, funcs, scen.group[1], scen.group[2],
                           mode=mode, float_exp=fe)


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


def gpu(scen, dedup=1, funcs=FUNCS):
    part = scen.part()
    s = Session(0)
    s.upload_part(part)
    configure(s, scen, part, funcs)
    s.set_row_dedup(dedup)
    consume(s, scen)
    out = s.finalize()
    stats = s.row_dedup_stats()
    s.close()
    return out, stats


class Want:
    """count / sum / min / max of one group, from a Fold or an AggResult."""

    def __init__(self, count, sum_, mn, mx):
        self.count, self.sum, self.min, self.max = count, sum_, mn, mx


def expected(scen, blocks):
    """Per-group Want over `blocks` (already merged, or all rows for the
    dedup-off legs) from the existing checkers."""
    fl = is_float(scen)
    nullable = scen.kind in (rdc.I64N, rdc.F64N)
    if fl or nullable or (scen.group and scen.group[0] == "code"):
        # the CPU oracle over a part built from the same rows (the part
        # builder's own encodings: the rows decide the result, not how a
        # block's timestamps were coded)
        assert scen.conds is None and scen.tree is None and scen.pred is None
        vt = VT_FLOAT64 if fl else VT_INT64
        kw = {}
        if scen.min_ts is not None:
            kw.update(min_ts=scen.min_ts, max_ts=scen.max_ts)
        n_groups = scen.group[1] if scen.group else 1
        res = oracle_scan(rdc.builder(blocks, scen.kind), vt,
                          n_groups=n_groups, **kw)
        return [Want(r.count, r.sum_f if fl else r.sum_i,
                     r.min_f if fl else r.min_i, r.max_f if fl else r.max_i)
                for r in res]
    conds = scen.conds
    if scen.pred is not None:
        conds = [TagCond(0, OP_EQ, [scen.pred])]
    if scen.group is not None:
        _, slot, domain = scen.group
        if scen.tree is not None:
            folds = ftr.fold_by_tag(blocks, scen.tree, slot, domain,
                                    scen.min_ts, scen.max_ts)
        else:
            folds = fr.fold_by_tag(blocks, conds or [], slot, domain,
                                   scen.min_ts, scen.max_ts)
    elif scen.tree is not None:
        folds = [ftr.fold(blocks, scen.tree, scen.min_ts, scen.max_ts)]
    else:
        folds = [fr.fold(blocks, conds or [], scen.min_ts, scen.max_ts)]
    return [Want(f.count, f.sum_i, f.min if f.count else None,
                 f.max if f.count else None) for f in folds]


def assert_parity(scen, got, want, what=""):
    assert len(got) == len(want)
    for gi, (g, w) in enumerate(zip(got, want)):
        if is_float(scen):
            print(what, gi, "gpu", (g.count, g.sum_f), "ref", (w.count, w.sum))
            assert g.count == w.count, (what, gi)
            if w.count:
                assert (g.min_f, g.max_f) == (w.min, w.max), (what, gi)
                assert math.isclose(g.sum_f, w.sum, rel_tol=1e-9), (what, gi)
        else:
            print(what, gi, "gpu", (g.count, g.sum_i), "ref", (w.count, w.sum))
            assert g.count == w.count, (what, gi)
            assert g.sum_i == w.sum, (what, gi)
            if w.count:
                assert (g.min_i, g.max_i) == (w.min, w.max), (what, gi)


# ---- cases 1-5, 7, 10: parity and census on every scenario ----
@pytest.mark.parametrize("name,make", rdc.CASES, ids=rdc.CASE_IDS)
def test_dedup_parity(name, make):
    scen = make()
    want = expected(scen, ref.merged(scen.blocks))
    census = ref.stats(scen.blocks)
    got, stats = gpu(scen)
    print(name, "stats", stats, "model", census)
    assert stats == census
    assert_parity(scen, got, want, name)
    if name in rdc.NOTHING_DROPPED:
        assert stats[1:] == [0, 0, 0]
        if name == "interleaved_none_equal":
            assert stats[0] > 0
    elif scen.min_ts is None:
        # the scenario is one the feature changes: all rows fold differently
        every = expected(scen, scen.blocks)
        assert [w.count for w in every] != [w.count for w in want]


# ---- 10: function masks and MODE_MAP partials ----
@pytest.mark.parametrize("funcs", [[AGG_MIN, AGG_MAX], [AGG_SUM, AGG_COUNT],
                                   [AGG_MEAN]],
                         ids=["min_max", "sum_count", "mean"])
@pytest.mark.parametrize("make", [rdc.varying_versions_case,
                                  rdc.mask_walker_case, rdc.float_case],
                         ids=["plain", "filtered", "float64"])
def test_function_masks(make, funcs):
    scen = make()
    want = expected(scen, ref.merged(scen.blocks))[0]
    g = gpu(scen, funcs=funcs)[0][0]
    fl = is_float(scen)
    if AGG_MIN in funcs:
        assert ((g.min_f, g.max_f) if fl else (g.min_i, g.max_i)) == \
            (want.min, want.max)
    if AGG_COUNT in funcs or AGG_MEAN in funcs:
        assert g.count == want.count
    if AGG_SUM in funcs:
        if fl:
            assert math.isclose(g.sum_f, want.sum, rel_tol=1e-9)
        else:
            assert g.sum_i == want.sum
    if AGG_MEAN in funcs:
        if fl:
            assert math.isclose(g.mean_f, want.sum / want.count, rel_tol=1e-9)
        else:
            import oracle as o
            assert g.mean_i == o.mean_val_i64(want.sum, want.count)


def test_finalize_partials_in_mode_map():
    scen = rdc.tag_group_filter_case()
    want = expected(scen, ref.merged(scen.blocks))
    part = scen.part()
    s = Session(0)
    s.upload_part(part)
    configure(s, scen, part, mode=MODE_MAP)
    s.set_row_dedup(1)
    consume(s, scen)
    parts = s.finalize_partials()
    s.close()
    assert sum(w.count for w in want) > 0
    for p, w in zip(parts, want):
        assert (p.count, p.sum_i) == (w.count, w.sum)
        if w.count:
            assert (p.min_i, p.max_i) == (w.min, w.max)


# ---- 6: equal (ts, version) in two blocks: the earlier block's row ----
def test_equal_version_tie_keeps_the_earliest_block():
    ts = rdc.arith_ts(100)
    vals = list(range(100))
    blocks = [rdc.DBlk(1, ts, [4] * 100, vals, [[b"first"] * 100]),
              rdc.DBlk(1, ts, [4] * 100, vals, [[b"second"] * 100])]
    for lit, count in ((b"first", 100), (b"second", 0)):
        scen = rdc.Scen(blocks, conds=[TagCond(0, OP_EQ, [lit])])
        got, stats = gpu(scen)
        assert stats == [2, 0, 1, 100]
        assert got[0].count == count
        assert_parity(scen, got, expected(scen, ref.merged(blocks)), lit)
    got, _ = gpu(rdc.Scen(blocks))
    assert (got[0].count, got[0].sum_i) == (100, sum(vals))
    # per-row ties inside partial blocks: where versions are equal the
    # first block's row stays, elsewhere the higher version
    va = [1 + (i % 3 == 0) for i in range(100)]
    vb = [1 + (i % 5 == 0) for i in range(100)]
    blocks = [rdc.DBlk(1, ts, va, vals, [[b"first"] * 100]),
              rdc.DBlk(1, ts, vb, vals, [[b"second"] * 100])]
    second_wins = sum(1 for a, b in zip(va, vb) if b > a)
    scen = rdc.Scen(blocks, conds=[TagCond(0, OP_EQ, [b"second"])])
    got, stats = gpu(scen)
    assert got[0].count == second_wins > 0
    assert stats == [2, 2, 0, 100]
    assert_parity(scen, got, expected(scen, ref.merged(blocks)), "ties")


# ---- 8: a fully superseded block is a skipped block ----
def test_fully_superseded_block_materialises_no_group_key():
    ts = rdc.arith_ts(200)
    domain = [b"old", b"new", b"other"]
    blocks = [rdc.DBlk(1, ts, [1] * 200, [1] * 200, [[b"old"] * 200]),
              rdc.DBlk(1, ts, [2] * 200, [5] * 200, [[b"new"] * 200]),
              rdc.DBlk(2, ts, [1] * 200, [7] * 200, [[b"other"] * 200])]
    part = rdc.builder(blocks)
    s = Session(0)
    s.upload_part(part)
    s.configure_by_tag(VT_INT64, FUNCS, 0, domain)
    s.set_row_dedup(1)
    s.consume()
    gs = s.finalize()
    seen = s.group_first_seen()
    assert s.row_dedup_stats() == [2, 0, 1, 200]
    assert [g.count for g in gs] == [0, 200, 200]
    assert [g.sum_i for g in gs] == [0, 1000, 1400]
    assert seen[0] == NEVER and seen[1] != NEVER and seen[2] != NEVER
    # with dedup off the key is there
    s.set_row_dedup(0)
    s.reset()
    s.consume()
    assert [g.count for g in s.finalize()] == [200, 200, 200]
    assert s.group_first_seen()[0] != NEVER
    s.close()


# ---- 9: dedup comes before the filter ----
def test_higher_version_failing_the_filter_still_hides_the_lower():
    ts = rdc.arith_ts(120)
    vals = rdc.ivals(__import__("random").Random(5), 120)
    # rows 40..79 are corrected by version 2, which carries tag b
    a = rdc.DBlk(1, ts, [1] * 120, vals, [[b"a"] * 120, [b"x"] * 120])
    b = rdc.DBlk(1, ts[40:80], [2] * 40, [0] * 40,
                 [[b"b"] * 40, [b"x"] * 40])
    for blocks in ([a, b], [b, a]):
        scen = rdc.Scen(blocks, conds=[TagCond(0, OP_EQ, [b"a"])])
        got, stats = gpu(scen)
        assert stats == [2, 1, 0, 40]
        keep = [v for i, v in enumerate(vals) if not 40 <= i < 80]
        assert (got[0].count, got[0].sum_i) == (80, sum(keep))
        assert_parity(scen, got, expected(scen, ref.merged(blocks)), "and")
        # filter-then-dedup would have kept all 120 version-1 rows
        off, _ = gpu(scen, dedup=0)
        assert off[0].count == 120
        # the same under an OR tree
        tree = Or(TagCond(0, OP_EQ, [b"a"]), TagCond(1, OP_EQ, [b"absent"]))
        scen = rdc.Scen(blocks, tree=tree)
        got, _ = gpu(scen)
        assert (got[0].count, got[0].sum_i) == (80, sum(keep))
        # and with the row-varying tag that takes the walker
        mixed = rdc.DBlk(1, ts, [1] * 120, vals,
                         [[b"a" if i % 7 else b"c" for i in range(120)],
                          [b"x"] * 120])
        blocks2 = [mixed if blk is a else blk for blk in blocks]
        scen = rdc.Scen(blocks2, conds=[TagCond(0, OP_EQ, [b"a"])])
        got, _ = gpu(scen)
        assert_parity(scen, got, expected(scen, ref.merged(blocks2)), "walk")
        assert got[0].count == sum(1 for i in range(120)
                                   if i % 7 and not 40 <= i < 80)


# ---- 11: dedup off is today's behaviour ----
@pytest.mark.parametrize("make", [rdc.middle_third_case,
                                  rdc.varying_versions_case,
                                  rdc.three_slot_case, rdc.tag_group_case,
                                  rdc.float_case],
                         ids=["middle_third", "varying", "three_slots",
                              "tag_group", "float64"])
def test_dedup_off_folds_every_row(make):
    scen = make()
    got, stats = gpu(scen, dedup=0)
    assert stats == [0, 0, 0, 0]
    assert_parity(scen, got, expected(scen, scen.blocks), "off")
    if scen.conds is None and scen.group is None:
        assert got[0].count == scen.n_rows
    # never set at all: the same
    part = scen.part()
    s = Session(0)
    s.upload_part(part)
    configure(s, scen, part)
    consume(s, scen)
    assert_parity(scen, s.finalize(), expected(scen, scen.blocks), "default")
    s.close()


# ---- 12: dedup on over a part without overlap ----
def test_no_overlap_is_identical_to_dedup_off():
    import random
    rng = random.Random(12)
    blocks = [rdc.DBlk(s + 1, rdc.arith_ts(900, rdc.T0 + k * 1000 * rdc.MS),
                       [1] * 900, rdc.ivals(rng, 900),
                       [rdc.env_runs(rng, 900)])
              for s in range(3) for k in range(2)]
    assert ref.stats(blocks) == [0, 0, 0, 0]
    part = rdc.builder(blocks)
    s = Session(0)
    s.upload_part(part)
    s.configure(VT_INT64, FUNCS)
    outs = []
    for on in (0, 1, 1):
        s.set_row_dedup(on)
        for conds in ([], [TagCond(0, OP_EQ, [b"prod"])]):
            s.reset()
            s.consume_filter(conds)
            p = s.finalize_partials()[0]
            outs.append((p.sum_i, p.count, p.min_i, p.max_i))
            assert s.row_dedup_stats() == [0, 0, 0, 0]
            assert s.last_consume_ms() > 0.0
    assert outs[0:2] == outs[2:4] == outs[4:6]
    assert outs[0][1] == 5400 and 0 < outs[1][1] < 5400
    s.close()


# ---- 13: lifecycle ----
def test_lifecycle_append_clear_reconsume_and_toggle():
    import random
    rng = random.Random(13)
    a = rdc.DBlk(1, rdc.arith_ts(400), [1] * 400, rdc.ivals(rng, 400))
    b = rdc.resend(rng, a, range(50, 150), [2] * 100)
    c = rdc.resend(rng, a, range(100, 300), [3] * 200)
    pa, pb, pc = (rdc.builder([x]) for x in (a, b, c))
    total = pa.payload_len + pb.payload_len + pc.payload_len

    def shifted(builder, base):
        """the builder's descriptors with offsets moved to `base`"""
        descs = builder.blocks()
        arr = (ba.BlockDesc * len(descs))()
        for i, d in enumerate(descs):
            arr[i] = d
            arr[i].ts_off += base
            arr[i].field_off += base
        return arr

    lib = ba.lib()
    s = Session(0)
    s.reserve(total, 3)
    s.configure(VT_INT64, FUNCS)
    s.set_row_dedup(1)
    assert s.row_dedup_stats() == [0, 0, 0, 0]      # nothing consumed yet
    base = 0
    resident = []
    for builder, blk in ((pa, a), (pb, b), (pc, c)):
        s._ck(lib.bydb_part_append(s._h, builder.raw_payload_ptr(),
                                   builder.payload_len,
                                   shifted(builder, base), 1))
        base += builder.payload_len
        resident.append(blk)
        scen = rdc.Scen(list(resident))
        for _ in range(2):                          # two consumes per part
            s.reset()
            s.consume()
            assert_parity(scen, s.finalize(),
                          expected(scen, ref.merged(resident)),
                          "resident %d" % len(resident))
            assert s.row_dedup_stats() == ref.stats(resident)
        # two consumes in one epoch accumulate twice the survivors
        s.reset()
        s.consume()
        s.consume()
        want = expected(scen, ref.merged(resident))[0]
        g = s.finalize()[0]
        assert (g.count, g.sum_i) == (2 * want.count, wrap64(2 * want.sum))
    final = ref.stats(resident)
    assert final == [3, 2, 0, 300] == s.row_dedup_stats()
    # toggling: off folds every row and reports zeros, on again is as before
    scen = rdc.Scen(resident)
    s.set_row_dedup(0)
    s.reset()
    s.consume()
    assert s.finalize()[0].count == 700
    assert s.row_dedup_stats() == [0, 0, 0, 0]
    s.set_row_dedup(1)
    s.reset()
    s.consume()
    assert_parity(scen, s.finalize(), expected(scen, ref.merged(resident)),
                  "on again")
    assert s.row_dedup_stats() == final
    # bad values are refused and change nothing
    for bad in (2, -1, 7):
        assert lib.bydb_set_row_dedup(s._h, bad) == BAD_ARG
    s.reset()
    s.consume()
    assert s.finalize()[0].count == 400
    # part_clear followed by a new part: the build follows the new part
    s.clear_part()
    fresh = [rdc.DBlk(9, rdc.arith_ts(64), [1] * 64, list(range(64))),
             rdc.DBlk(9, rdc.arith_ts(64), [2] * 64, list(range(64, 128)))]
    s.upload_part(rdc.builder(fresh))
    s.configure(VT_INT64, FUNCS)
    s.consume()
    g = s.finalize()[0]
    assert (g.count, g.sum_i) == (64, sum(range(64, 128)))
    assert s.row_dedup_stats() == [2, 0, 1, 64]
    s.close()


# ---- a descending block is a device error, as in the scan ----
def test_descending_timestamps_are_a_device_error():
    ts = rdc.arith_ts(100)
    blocks = [rdc.DBlk(1, ts, [1] * 100, list(range(100))),
              rdc.DBlk(1, ts, [2] * 100, list(range(100)),
                       raw_delta_ts=True)]
    raw = rdc.RawPart(blocks)
    # flip one delta of the hand-encoded list: the block descends there
    d = raw.blocks_ptr()[1]
    raw._buf[d.ts_off + 39] |= 1          # first byte of a varint; zigzag:
                                          # odd = negative
    s = Session(0)
    s.upload_part(raw)
    s.configure(VT_INT64, FUNCS)
    s.set_row_dedup(1)
    s.consume()
    with pytest.raises(RuntimeError, match="device decode error 3"):
        s.finalize()
    # and it stays one after a reset
    s.reset()
    s.consume()
    with pytest.raises(RuntimeError, match="device decode error"):
        s.finalize()
    s.close()


# ---- 14: seeded random leg ----
def test_random_scenarios():
    for seed in rdc.RANDOM_SEEDS:
        scen = rdc.random_scenario(seed)
        census = ref.stats(scen.blocks)
        assert census[3] > 0 and census[1] > 0, seed
        try:
            got, stats = gpu(scen)
            assert stats == census
            assert_parity(scen, got, expected(scen, ref.merged(scen.blocks)),
                          "seed %d" % seed)
        except Exception:
            print("FAILING SEED %d: rdc.random_scenario(%d)" % (seed, seed))
            raise


# ---- 15: the reference's recorded vectors end to end ----
def test_golden_vectors_on_the_gpu():
    with open(GOLDEN) as f:
        doc = json.load(f)
    for case in doc["cases"]:
        blocks = rdc.golden_blocks(doc["inputs"], case["parts"])
        s = Session(0)
        s.upload_part(rdc.builder(blocks, rdc.I64N))
        s.configure(VT_INT64, [AGG_SUM, AGG_COUNT], n_groups=3)
        s.set_row_dedup(1)
        s.consume(case["min_ts"], case["max_ts"])
        gs = s.finalize()
        s.close()
        for w in case["want"]:
            g = gs[w["series"] - 1]
            vals = w["intField"] or []
            assert (g.count, g.sum_i) == (len(vals), sum(vals)), case["name"]


# ---- the pure-C consumer ----
def test_c_consumer_runs_a_deduped_scan(tmp_path):
    """tools/cabi_row_dedup_check.c: the planner and one deduped scan
    through the header alone, checked against its own host loop."""
    exe = str(tmp_path / "cabi_row_dedup_check")
    rdc.build_consumer(exe)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stderr + p.stdout
    assert "row dedup consumer OK" in p.stdout
