"""The dense one-byte delta fold on data that fills the byte lanes:
deltas over the whole one-byte span -64..63 (zigzag bytes up to 0x7e and
0x7f), runs of +63 and of -64 that drive the per-batch int32 accumulators
towards their bound, and values that wrap through INT64_MAX.  Sum, count,
min and max are exact against the oracle, per block."""
import functools

import pytest

import clamp_cases as cc
import oracle as o
from banyandb_amd import (PartBuilder, Session, VT_INT64, VT_FLOAT64,
                          AGG_SUM, AGG_COUNT, AGG_MIN, AGG_MAX)
from helpers import oracle_blocks
from test_gpu_dense_wide import _clamp_rows, _is_dense
from test_gpu_fuzz import f64_sum_close

pytestmark = pytest.mark.gpu

CLOSED_FORM = [AGG_SUM, AGG_COUNT]
VALUE_SCAN = [AGG_SUM, AGG_COUNT, AGG_MIN, AGG_MAX]
FUNC_SETS = [pytest.param(CLOSED_FORM, id="sum_count"),
             pytest.param(VALUE_SCAN, id="sum_count_min_max")]


def _tuples(res):
    return [(g.count, g.sum_i, g.min_i, g.max_i) for g in res]


def _scan(pb, funcs, n_groups, clamps=({},)):
    """One session; per clamp the per-group (count, sum, min, max)."""
    s = Session(0)
    s.upload_part(pb)
    s.configure(VT_INT64, funcs, n_groups=n_groups)
    out = []
    try:
        for kw in clamps:
            s.reset()
            s.consume(**kw)
            out.append(_tuples(s.finalize()))
    finally:
        s.close()
    return out


def _assert_groups(got, want, funcs, where):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0], ("count", i) + where
        assert g[1] == w[1], ("sum", i) + where
        if w[0] and AGG_MIN in funcs:
            assert g[2:] == w[2:], ("min/max", i) + where


@functools.lru_cache(maxsize=None)
def _extreme_pairs():
    descs = cc.extremes_part().builder().blocks()
    assert all(_is_dense(d) for d in descs)
    aligns = sorted({d.field_off % 16 for d in descs})
    return tuple(_clamp_rows(aligns))


@functools.lru_cache(maxsize=None)
def _extreme_oracle():
    """Whole range first, then one entry per row clamp."""
    part = cc.extremes_part()
    payload, blocks = oracle_blocks(part.builder())
    clamps = [{}] + [dict(min_ts=cc.T0 + r0 * cc.MS, max_ts=cc.T0 + r1 * cc.MS)
                     for r0, r1 in _extreme_pairs()]
    return clamps, [_tuples(o.scan_agg(payload, blocks, VT_INT64,
                                       n_groups=part.n_groups, **kw))
                    for kw in clamps]


@pytest.mark.parametrize("funcs", FUNC_SETS)
def test_extreme_shapes_full_range(funcs):
    part = cc.extremes_part()
    clamps, want = _extreme_oracle()
    got = _scan(part.builder(), funcs, part.n_groups)[0]
    assert all(w[0] == cc.N_EXT for w in want[0])
    _assert_groups(got, want[0], funcs, ("whole",))


@pytest.mark.parametrize("funcs", FUNC_SETS)
def test_extreme_shapes_clamp_sweep(funcs):
    """The lane / chunk boundary clamps of the dense sweep, for the
    alignments these blocks have, now with min and max."""
    part = cc.extremes_part()
    clamps, want = _extreme_oracle()
    got = _scan(part.builder(), funcs, part.n_groups, clamps[1:])
    for pair, g, w in zip(_extreme_pairs(), got, want[1:]):
        assert all(b[0] == pair[1] - pair[0] + 1 for b in w)
        _assert_groups(g, w, funcs, (pair,))
    print(f"clamps[extremes]: {len(got)}")


def test_length_sweep_whole_part():
    pb = cc.lengths_builder()
    n = pb.n_blocks
    payload, blocks = oracle_blocks(pb)
    want = _tuples(o.scan_agg(payload, blocks, VT_INT64, n_groups=n))
    _assert_groups(_scan(pb, VALUE_SCAN, n)[0], want, VALUE_SCAN, ("part",))


def test_length_sweep_each_block_last():
    """Each dense block as the last stream of a part of its own, behind
    its filler, so that the reads past its end leave the part."""
    n_dense, aligns = 0, set()
    for i, case in enumerate(cc.length_cases()):
        pb = PartBuilder()
        cc.add_length_case(pb, case, 0)
        d = pb.blocks()[-1]
        if not _is_dense(d):
            continue
        n_dense += 1
        aligns.add(d.field_off % 16)
        assert d.field_off + d.field_len == pb.payload_len
        payload, blocks = oracle_blocks(pb)
        want = _tuples(o.scan_agg(payload, blocks, VT_INT64, n_groups=2))
        _assert_groups(_scan(pb, VALUE_SCAN, 2)[0], want, VALUE_SCAN,
                       (i, d.field_off % 16, d.field_len))
    assert aligns == set(range(16)) and n_dense >= 80


def test_extreme_f64():
    part = cc.extremes_f64_part()
    pb = part.builder()
    d = pb.blocks()[0]
    assert _is_dense(d) and d.field_first == 10 ** 6
    payload, blocks = oracle_blocks(pb)
    w = o.scan_agg(payload, blocks, VT_FLOAT64)[0]
    s = Session(0)
    s.upload_part(pb)
    s.configure(VT_FLOAT64, VALUE_SCAN, float_exp=part.float_exp())
    s.consume()
    g = s.finalize()[0]
    s.close()
    assert g.count == w.count == cc.N_EXT
    assert (g.min_f, g.max_f) == (w.min_f, w.max_f)
    assert f64_sum_close(g.sum_f, w.sum_f, w.count)


def test_tag_groupby_across_the_wrap():
    """Shapes 2 and 5 under a per-row tag: min/max over runs that the
    int64 wrap cuts through."""
    part = cc.extremes_tag_part()
    pb = part.builder()
    payload, blocks = oracle_blocks(pb)
    orc = o.scan_agg_bytag(payload, blocks, VT_INT64, 0, cc.TAGS)
    s = Session(0)
    s.upload_part(pb)
    s.configure_by_tag(VT_INT64, VALUE_SCAN, 0, cc.TAGS)
    s.consume()
    gs = s.finalize()
    s.close()
    assert sum(w.count for w in orc) > cc.N_EXT
    for t, g, w in zip(cc.TAGS, gs, orc):
        assert w.count > 0
        assert (g.count, g.sum_i, g.min_i, g.max_i) == \
            (w.count, w.sum_i, w.min_i, w.max_i), t
