"""The row clamp over stream-coded (delta-of-delta) timestamps: one-byte,
two-byte, interleaved, 7-8-byte and 10-byte d2 streams, block sizes around
the 64-byte step of the stream counter, and bounds on, one below and one
above stored timestamps.  Every block is its own group, so each clamp
compares every block's partial with the oracle's (which
test_clamp_cases_cpu pins against a per-row restatement)."""
import functools

import pytest

import clamp_cases as cc
import oracle as o
from banyandb_amd import (Session, VT_INT64, VT_FLOAT64, AGG_SUM, AGG_COUNT,
                          AGG_MIN, AGG_MAX)
from helpers import oracle_blocks
from test_gpu_fuzz import f64_sum_close

pytestmark = pytest.mark.gpu

CLOSED_FORM = [AGG_SUM, AGG_COUNT]
VALUE_SCAN = [AGG_SUM, AGG_COUNT, AGG_MIN, AGG_MAX]
FUNC_SETS = [pytest.param(CLOSED_FORM, id="sum_count"),
             pytest.param(VALUE_SCAN, id="sum_count_min_max")]
WHOLE = (0, 0, 0, 0, cc.INT64_MIN, cc.INT64_MAX)


def _tuples(res, float_vals):
    if float_vals:
        return [(g.count, g.sum_f, g.min_f, g.max_f) for g in res]
    return [(g.count, g.sum_i, g.min_i, g.max_i) for g in res]


@functools.lru_cache(maxsize=None)
def _oracle(part, clamp_list, pred=b""):
    """Per clamp, per block (count, sum, min, max); computed once and
    shared by the func sets."""
    vtype = VT_FLOAT64 if part.float_vals else VT_INT64
    payload, blocks = oracle_blocks(part.builder())
    return [_tuples(o.scan_agg(payload, blocks, vtype, min_ts=c[4],
                               max_ts=c[5], pred=pred,
                               n_groups=part.n_groups), part.float_vals)
            for c in clamp_list]


def _session(part, funcs):
    s = Session(0)
    s.upload_part(part.builder())
    s.configure(VT_FLOAT64 if part.float_vals else VT_INT64, funcs,
                n_groups=part.n_groups, float_exp=part.float_exp())
    return s


def _compare(part, got, want, funcs, clamp):
    """One clamp: every block's partial against the oracle's."""
    descs = part.builder().blocks()
    minmax = AGG_MIN in funcs
    assert len(got) == len(want) == part.n_groups
    for i, (g, w) in enumerate(zip(got, want)):
        where = (part.name, i, part.blocks[i].n, part.blocks[i].kind,
                 o.ENC_NAMES[descs[i].field_enc], clamp[:4])
        assert g[0] == w[0], ("count",) + where
        if not w[0]:
            continue
        if part.float_vals:
            assert f64_sum_close(g[1], w[1], w[0]), ("sum",) + where
        else:
            assert g[1] == w[1], ("sum",) + where
        if minmax:
            assert g[2:] == w[2:], ("min/max",) + where


def _sweep(part, clamp_list, funcs, pred=b""):
    want = _oracle(part, clamp_list, pred)
    s = _session(part, funcs)
    try:
        for clamp, w in zip(clamp_list, want):
            s.reset()
            s.consume(min_ts=clamp[4], max_ts=clamp[5], pred=pred)
            _compare(part, _tuples(s.finalize(), part.float_vals), w, funcs,
                     clamp)
    finally:
        s.close()
    # the sweep did select rows, and did select none, somewhere
    assert any(any(b[0] for b in w) for w in want)
    return len(clamp_list)


@pytest.mark.parametrize("funcs", FUNC_SETS)
@pytest.mark.parametrize("shape", cc.TS_SHAPES)
def test_stream_clamp(shape, funcs):
    clamp_list, dropped = cc.clamps(shape)
    assert dropped * 20 < len(clamp_list) + dropped
    n = _sweep(cc.ts_part(shape), clamp_list, funcs)
    print(f"clamps[{shape}]: {n}")


def test_stream_clamp_f64():
    """Float session over the interleaved shape; min/max exact, the sum
    under the fuzz's rule (the oracle adds per-row doubles)."""
    part = cc.ts_part("mixed", True)
    assert part.float_exp() == -2
    n = _sweep(part, cc.clamps("mixed")[0], VALUE_SCAN)
    print(f"clamps[mixed f64]: {n}")


@pytest.mark.parametrize("funcs", FUNC_SETS)
@pytest.mark.parametrize("shape", cc.TS_SHAPES)
def test_full_cover_clamp_equals_unclamped(shape, funcs):
    """Finite bounds that cover the part: the host picks the clamp-free
    instantiation, and the result is the unclamped one."""
    part = cc.ts_part(shape)
    axis = cc.ts_axis(shape)
    covers = [(0, len(axis) - 1, dl, dh, axis[0] + dl, axis[-1] + dh)
              for dl, dh in ((0, 0), (-1, 1), (-1, 0), (0, 1))]
    clamp_list = (WHOLE,) + tuple(covers)
    want = _oracle(part, clamp_list)
    assert all(w == want[0] for w in want)
    assert all(b[0] == blk.n for b, blk in zip(want[0], part.blocks))
    _sweep(part, clamp_list, funcs)


def _check_bytag(part, clamp_list):
    payload, blocks = oracle_blocks(part.builder())
    s = Session(0)
    s.upload_part(part.builder())
    s.configure_by_tag(VT_INT64, VALUE_SCAN, 0, cc.TAGS)
    n_sel = 0
    try:
        for clamp in clamp_list:
            orc = o.scan_agg_bytag(payload, blocks, VT_INT64, 0, cc.TAGS,
                                   clamp[4], clamp[5])
            s.reset()
            s.consume(min_ts=clamp[4], max_ts=clamp[5])
            for t, g, w in zip(cc.TAGS, s.finalize(), orc):
                where = (part.name, t, clamp[:4])
                assert g.count == w.count, ("count",) + where
                assert g.sum_i == w.sum_i, ("sum",) + where
                if w.count:
                    n_sel += 1
                    assert (g.min_i, g.max_i) == (w.min_i, w.max_i), \
                        ("min/max",) + where
    finally:
        s.close()
    assert n_sel > 0


def test_tag_groupby_under_stream_clamp():
    """Per-row tag group-by: the fold ranges are cut by the run merge and
    by the clamp at once."""
    clamp_list = cc.tag_clamps()
    assert 35 <= len(clamp_list) <= 45
    _check_bytag(cc.tag_part(), clamp_list)


def test_row_predicate_under_stream_clamp():
    """Row-varying tag predicate: the walker path with r0 / r1."""
    part = cc.tag_part()
    clamp_list = cc.tag_clamps()
    for k, pred in enumerate(cc.TAGS[:3]):
        _sweep(part, clamp_list[k::3], VALUE_SCAN, pred=pred)
