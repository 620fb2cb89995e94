"""The second trip round every per-block kernel loop, against a reference.

The parts of loop_trip_cases.py hold more blocks than the launches have
waves (k_scan_agg_t, k_top_bounds, k_rows_bounds: SCAN_MAX_WGS workgroups of
four waves) or workgroups (the 64-thread pack, resolve and dedup kernels:
BLOCK_KERNEL_MAX_WGS), and put different kinds of block at the two indices
one wave handles.  test_loop_trips_cpu.py checks that structure on the host.
Here every result is compared per group with the C oracle over the encoded
part or with the per-row models (filter_ref, filter_tree_ref, row_dedup_ref,
top_rows_ref, row_scan_ref): count, min, max and the int64 sum bit for bit,
float64 sum and mean within the suite's rel 1e-9.

Not reached: the first loop of k_dedup_apply (64 fully superseded blocks per
workgroup) goes round again only past 4.19 million fully superseded
blocks."""
import functools
import math
import struct

import pytest

from banyandb_amd import (Session, TagCond, VT_INT64, VT_FLOAT64, AGG_SUM,
                          AGG_COUNT, AGG_MIN, AGG_MAX, AGG_MEAN, OP_EQ,
                          INT64_MIN, INT64_MAX, STREAM_STREAMING, PACK_OFF,
                          PACK_ON)
import field_pack_ref as fpr
import filter_ref as fr
import filter_tree_ref as ftr
import loop_trip_cases as ltc
import row_dedup_ref as rdr
from helpers import oracle_scan

pytestmark = pytest.mark.gpu

TWO = [AGG_SUM, AGG_COUNT]
FOUR = [AGG_SUM, AGG_COUNT, AGG_MIN, AGG_MAX]
EQ = [TagCond(1, OP_EQ, [ltc.LIT])]
FULL = (INT64_MIN, INT64_MAX)


def _session(name, coded=False):
    s = Session(0)
    s.upload_part(ltc.part(name, coded))
    return s


@pytest.fixture(scope="module")
def sess_s():
    s = _session("s")
    yield s
    s.close()


@pytest.fixture(scope="module")
def sess_f():
    s = _session("f")
    yield s
    s.close()


@pytest.fixture(scope="module")
def sess_twin():
    s = _session("twin")
    yield s
    s.close()


@pytest.fixture(scope="module")
def sess_b():
    s = _session("b")
    yield s
    s.close()


@pytest.fixture(scope="module")
def sess_d():
    s = _session("d")
    s.set_row_dedup(1)
    yield s
    s.close()


def _consume(s, pred, clamp):
    lo, hi = ltc.CLAMP if clamp else FULL
    if pred:
        s.consume_filter(EQ, lo, hi)
    else:
        s.consume(lo, hi)


def _assert_i64(got, want, minmax, what):
    """got: engine results; want: objects with count / sum_i / min_i /
    max_i per group."""
    assert len(got) == len(want)
    for gi, (g, w) in enumerate(zip(got, want)):
        print(what, gi, "gpu", (g.count, g.sum_i), "ref", (w.count, w.sum_i))
        assert g.count == w.count, (what, gi)
        assert g.sum_i == w.sum_i, (what, gi)
        if minmax and w.count:
            assert (g.min_i, g.max_i) == (w.min_i, w.max_i), (what, gi)


class _Fold:
    """A filter_ref.Fold under the oracle's field names."""

    def __init__(self, f):
        self.count, self.sum_i = f.count, f.sum_i
        self.min_i = f.min if f.count else None
        self.max_i = f.max if f.count else None


# ---- a. the scan matrix on part S ----
@pytest.mark.parametrize("q", ltc.MATRIX, ids=ltc.matrix_id)
def test_scan_matrix(sess_s, q):
    """One query per combination of {SUM, COUNT} / {SUM, COUNT, MIN, MAX},
    no predicate / EQ on slot 1, no group / group-by on a row-varying tag,
    whole range / clamp.  The group-by is on slot 1; under the predicate it
    is on slot 2, a second tag of the same make, because EQ on the grouped
    slot leaves one group and a wave's partial nothing to flush (such a case
    passes with the reset in WavePartial::add taken out).  launch_scan picks k_scan_agg_t<EN_VALUES, EN_PREDS, EN_GROUPS,
    EN_WALK, EN_CLAMP> from them (ltc.instantiations):

      EN_VALUES  MIN or MAX asked for
      EN_PREDS   a predicate: a light pass <.., 1, .., 0, ..> over the
                 PF_CLEAR blocks and a heavy pass <.., 1, .., 1, ..> over
                 the PF_WALK blocks, both launched by every such query
      EN_GROUPS  configure_by_tag
      EN_CLAMP   the range does not cover the part

      sumcount-nopred-nogroup-full   <0,0,0,0,0>
      sumcount-nopred-nogroup-clamp  <0,0,0,0,1>
      sumcount-nopred-bytag-full     <0,0,1,0,0>
      sumcount-nopred-bytag-clamp    <0,0,1,0,1>
      sumcount-pred-nogroup-full     <0,1,0,0,0> <0,1,0,1,0>
      sumcount-pred-nogroup-clamp    <0,1,0,0,1> <0,1,0,1,1>
      sumcount-pred-bytag-full       <0,1,1,0,0> <0,1,1,1,0>
      sumcount-pred-bytag-clamp      <0,1,1,0,1> <0,1,1,1,1>
      minmax-...                     the same with EN_VALUES = 1

    16 light and 8 heavy instantiations: all 24 that are not the streaming
    pair (test_pack_on_off_and_oracle runs those past the cap).  The part is
    small enough for the cached policy, so no query here streams."""
    v, p, g, c = q
    s = sess_s
    funcs = FOUR if v else TWO
    if g:
        s.configure_by_tag(VT_INT64, funcs, *ltc.group_slot(p))
    else:
        s.configure(VT_INT64, funcs)
    s.reset()
    _consume(s, p, c)
    want = ltc.oracle_agg("s", p, "tag" if g else None, c)
    assert all(w.count > 0 for w in want)
    _assert_i64(s.finalize(), want, v, ltc.matrix_id(q))


@pytest.mark.parametrize("clamp", [False, True], ids=["full", "clamp"])
@pytest.mark.parametrize("funcs", [TWO, FOUR], ids=["sumcount", "minmax"])
def test_block_code_groups(funcs, clamp):
    """The unpredicated, ungrouped instantiations with three block-code
    groups (index % 3): a wave's second block is never in the group of its
    first, so its partial is flushed and reset."""
    s = _session("s", coded=True)
    try:
        s.configure(VT_INT64, funcs, n_groups=3)
        _consume(s, False, clamp)
        want = ltc.oracle_agg("s", False, "code", clamp)
        _assert_i64(s.finalize(), want, funcs is FOUR, "code groups")
    finally:
        s.close()


# ---- b. part F ----
@pytest.mark.parametrize("clamp", [False, True], ids=["full", "clamp"])
@pytest.mark.parametrize("group", [False, True], ids=["nogroup", "bytag"])
@pytest.mark.parametrize("pred", [False, True], ids=["nopred", "pred"])
def test_float64_exponents_change_between_trips(sess_f, pred, group, clamp):
    s = sess_f
    funcs = FOUR + [AGG_MEAN]
    fe = min(d.exp for d in ltc.part("f").blocks())
    if group:
        s.configure_by_tag(VT_FLOAT64, funcs, *ltc.group_slot(pred),
                           float_exp=fe)
    else:
        s.configure(VT_FLOAT64, funcs, float_exp=fe)
    s.reset()
    _consume(s, pred, clamp)
    got = s.finalize()
    want = ltc.oracle_agg("f", pred, "tag" if group else None, clamp)
    assert len(got) == len(want)
    for gi, (g, w) in enumerate(zip(got, want)):
        print(gi, "gpu", (g.count, g.sum_f), "ref", (w.count, w.sum_f))
        assert g.count == w.count, gi
        if w.count:
            assert struct.pack("<dd", g.min_f, g.max_f) == \
                struct.pack("<dd", w.min_f, w.max_f), gi
            assert math.isclose(g.sum_f, w.sum_f, rel_tol=1e-9), gi
            assert math.isclose(g.mean_f, w.sum_f / w.count, rel_tol=1e-9), gi


# ---- c. filter operators and trees on part S ----
@functools.lru_cache(maxsize=None)
def _filter_want(what, grouped):
    blocks = ltc.model("s")
    if what == "conds":
        folds = fr.fold_by_tag(blocks, ltc.CONDS, 1, ltc.DOMAIN) if grouped \
            else [fr.fold(blocks, ltc.CONDS)]
    else:
        folds = ftr.fold_by_tag(blocks, ltc.TREE, 1, ltc.DOMAIN) if grouped \
            else [ftr.fold(blocks, ltc.TREE)]
    return [_Fold(f) for f in folds]


@pytest.mark.parametrize("grouped", [False, True], ids=["nogroup", "bytag"])
@pytest.mark.parametrize("what", ["conds", "tree"])
def test_filter_conditions_and_trees(sess_s, what, grouped):
    """NE on the entity tag AND IN on the row-varying tag through
    consume_filter; a three-leaf OR through consume_filter_tree."""
    s = sess_s
    if grouped:
        s.configure_by_tag(VT_INT64, FOUR, 1, ltc.DOMAIN)
    else:
        s.configure(VT_INT64, FOUR)
    s.reset()
    if what == "conds":
        s.consume_filter(ltc.CONDS)
    else:
        s.consume_filter_tree(ltc.TREE)
    want = _filter_want(what, grouped)
    assert all(w.count > 0 for w in want)
    _assert_i64(s.finalize(), want, True, what)


# ---- d. top-N and time-ordered rows on the twin of part S ----
def _norm(t):
    """A row tuple with value_f as its bytes."""
    return t[:4] + (struct.pack("<d", t[4]),) + t[5:]


def _consume_sel(s, sel):
    kw = ltc.SELECTIONS[sel]
    lo, hi = kw.get("min_ts", INT64_MIN), kw.get("max_ts", INT64_MAX)
    if "conds" in kw:
        s.consume_filter(kw["conds"], lo, hi)
    else:
        s.consume(lo, hi)


def _assert_rows(got, want, what):
    got = [_norm(r.astuple()) for r in got]
    want = [_norm(t) for t in want]
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (what, "row", i, a, b)


@pytest.mark.parametrize("asc", [False, True], ids=["desc", "asc"])
@pytest.mark.parametrize("n", ltc.TOP_NS)
@pytest.mark.parametrize("sel", list(ltc.SELECTIONS))
def test_top_rows_past_the_cap(sess_twin, sel, n, asc):
    """The winners lie in blocks on both sides of the scan cap; a single
    winner lies past it."""
    s = sess_twin
    s.configure_top(VT_INT64, n, asc)
    _consume_sel(s, sel)
    want = ltc.top_expected(sel, n, asc)
    assert ltc.sides(want, ltc.scan_waves()) == \
        ({"below", "past"} if n > 1 else {"past"})
    _assert_rows(s.top_rows(), want, (sel, n, asc))


@pytest.mark.parametrize("desc", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("window", ltc.ROW_WINDOWS, ids=["first", "900+124"])
@pytest.mark.parametrize("sel", list(ltc.SELECTIONS))
def test_row_scan_past_the_cap(sess_twin, sel, window, desc):
    s = sess_twin
    offset, limit = window
    s.configure_rows(VT_INT64, offset, limit, desc)
    _consume_sel(s, sel)
    want = ltc.rows_expected(sel, offset, limit, desc)
    assert ltc.sides(want, ltc.scan_waves()) == \
        ({"below", "past"} if limit > 1 else {"past"})
    _assert_rows(s.scan_rows(), want, (sel, window, desc))


# ---- e. part B: the 64-thread pack and resolve kernels ----
def test_pack_on_off_and_oracle(sess_b):
    """k_pack_fields and the two streaming instantiations, whole range and
    clamped: packing off and on give the same bits, the oracle's, and the
    build packs exactly the blocks the reference rule packs — on both
    sides of the workgroup cap."""
    s = sess_b
    p = ltc.part("b")
    cand, hit, nbytes = fpr.census(p)
    clamps = ({}, dict(min_ts=ltc.T0 + 2 * ltc.MS, max_ts=ltc.T0 + 33 * ltc.MS))
    s.configure(VT_INT64, TWO)
    s.set_stream_policy(STREAM_STREAMING)
    out = {}
    wants = [oracle_scan(p, VT_INT64, **kw)[0] for kw in clamps]
    assert 0 < wants[1].count < wants[0].count
    for mode in (PACK_OFF, PACK_ON):
        s.set_field_pack(mode)
        for k, (kw, want) in enumerate(zip(clamps, wants)):
            s.reset()
            s.consume(**kw)
            g = s.finalize()[0]
            out[mode, k] = struct.pack("<qqd", g.count, g.sum_i, g.sum_f)
            assert (g.count, g.sum_i) == (want.count, want.sum_i), (mode, kw)
        stats = s.field_pack_stats()
        if mode == PACK_OFF:
            assert stats == [0, 0, 0, 0]
        else:
            assert stats[:3] == [cand, hit, nbytes], (stats, cand, hit)
    for k in range(len(clamps)):
        assert out[PACK_OFF, k] == out[PACK_ON, k]
    s.set_field_pack(PACK_OFF)


def test_predicate_on_the_plain_slot(sess_b):
    s = sess_b
    s.configure(VT_INT64, FOUR)
    s.reset()
    s.consume_filter(ltc.B_CONDS)
    want = _Fold(fr.fold(ltc.rows_of("b"), ltc.B_CONDS))
    assert want.count > 0
    _assert_i64(s.finalize(), [want], True, "plain filter")


def test_group_by_on_the_plain_slot(sess_b):
    s = sess_b
    s.configure_by_tag(VT_INT64, FOUR, 0, ltc.B_PLAIN_DOMAIN)
    s.reset()
    s.consume()
    want = [_Fold(f) for f in fr.fold_by_tag(ltc.rows_of("b"), [], 0,
                                             ltc.B_PLAIN_DOMAIN)]
    assert all(w.count > 0 for w in want)
    _assert_i64(s.finalize(), want, True, "plain group-by")


def test_tree_that_needs_row_bitmaps(sess_b):
    s = sess_b
    s.configure(VT_INT64, FOUR)
    s.reset()
    s.consume_filter_tree(ltc.B_TREE)
    want = _Fold(ftr.fold(ltc.rows_of("b"), ltc.B_TREE))
    stats = s.filter_tree_stats()
    print("tree stats", stats)
    assert stats[3] > 0            # blocks resolved into per-row bitmaps
    _assert_i64(s.finalize(), [want], True, "row-bitmap tree")


# ---- f. part D: the dedup build and apply ----
@functools.lru_cache(maxsize=None)
def _d_merged():
    return rdr.merged(list(ltc.rows_of("d")))


@pytest.mark.parametrize("conds", [None, ltc.D_COND], ids=["all", "eq"])
def test_deduped_aggregate(sess_d, conds):
    s = sess_d
    s.configure(VT_INT64, FOUR)
    s.reset()
    if conds is None:
        s.consume()
    else:
        s.consume_filter(conds)
    got = s.finalize()
    assert s.row_dedup_stats() == ltc.d_census()
    want = _Fold(fr.fold(_d_merged(), conds or []))
    assert want.count > 0
    _assert_i64(got, [want], True, "dedup")


def test_deduped_latest_rows(sess_d):
    s = sess_d
    s.configure_rows(VT_INT64, 0, 100, desc=True)
    s.consume()
    want = ltc.rows_expected("all", 0, 100, True, name="d", dedup=True)
    cap = ltc.caps()["BLOCK_KERNEL_MAX_WGS"]
    assert ltc.sides(want, cap) == {"below", "past"}
    _assert_rows(s.scan_rows(), want, "latest 100")
