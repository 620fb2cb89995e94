"""The clamp / value-extreme inputs, checked without a GPU: first that
they reach the encodings the GPU tests rely on (conditions on the block
descriptors), then that the oracle agrees with a per-row restatement of
the scan on every part and clamp, so the reference is pinned before the
GPU is compared with it."""
import math

import pytest

import clamp_cases as cc
from banyandb_amd import VT_INT64, VT_FLOAT64
from helpers import oracle_blocks
from test_gpu_fuzz import f64_sum_close
import oracle as o


def _dense(d):
    return d.field_enc == cc.ENC_DELTA and d.field_len == d.count - 1


# ---- selection asserts ------------------------------------------------
@pytest.mark.parametrize("shape", cc.TS_SHAPES)
def test_timestamps_are_stream_coded(shape):
    pb = cc.ts_part(shape).builder()
    descs = pb.blocks()
    assert len(descs) == len(cc.shape_sizes(shape)) * len(cc.FIELD_KINDS)
    for d in descs:
        if d.count >= 3:
            assert d.ts_enc_with_version == cc.ENC_DOD_WV, d.count
    if shape == "one_byte":
        for d in descs:
            assert d.ts_len == d.count - 1, d.count
    if shape == "ten_byte":
        for d in descs:
            assert d.count == 8 and d.ts_len == 61 and d.ts_min < 0


def test_mixed_interleaves_varint_lengths():
    pb = cc.ts_part("mixed").builder()
    d = next(d for d in pb.blocks() if d.count == 8192)
    lens = cc.varint_lengths(pb.payload[d.ts_off:d.ts_off + d.ts_len])
    assert len(lens) == d.count - 1
    assert len(set(lens)) >= 4, sorted(set(lens))
    # and varints do straddle the 64-byte steps of the row clamp
    ends, pos = set(), 0
    for ln in lens[1:]:             # the d2 stream starts after d1
        pos += ln
        ends.add(pos)
    assert any(k not in ends for k in range(64, pos, 64))


def test_field_kinds_reach_their_encodings():
    """At the full block size each field kind is the encoding it is named
    for, on every shape that has that size."""
    want = {"const": 1, "delta_const": 2, "dense": 3, "multi_byte": 3,
            "dod": 4}
    for shape in ("one_byte", "two_byte", "mixed"):
        part = cc.ts_part(shape)
        for blk, d in zip(part.blocks, part.builder().blocks()):
            if blk.n < 1000:
                continue
            assert d.field_enc == want[blk.kind], (shape, blk.n, blk.kind)
            assert _dense(d) == (blk.kind == "dense"), (shape, blk.n)


def test_extreme_shapes_are_dense_delta():
    part = cc.extremes_part()
    for blk, d in zip(part.blocks, part.builder().blocks()):
        assert _dense(d) and d.count == cc.N_EXT, blk.kind
        stream = part.builder().payload[d.field_off:d.field_off + d.field_len]
        if blk.kind in ("extreme1", "extreme2", "extreme6", "extreme7"):
            assert 0x7e in stream and 0x7f in stream, blk.kind
    for p in (cc.extremes_tag_part(), cc.tag_part()):
        for blk, d in zip(p.blocks, p.builder().blocks()):
            assert _dense(d) == blk.kind.startswith("extreme"), blk.kind
    d = cc.extremes_f64_part().builder().blocks()[0]
    assert _dense(d) and d.exp == -2


def test_extreme_values_cross_the_int64_wrap():
    for k in (5, 6):
        vals = cc.extreme_values(k)
        assert min(vals) < -2 ** 62 and max(vals) > 2 ** 62, k


def test_length_sweep_covers_every_alignment():
    descs = cc.lengths_builder().blocks()
    assert len(descs) == 2 * len(cc.length_cases())
    dense = [d for d in descs[1::2] if _dense(d)]
    assert {d.field_off % 16 for d in dense} == set(range(16))
    assert {d.field_len for d in dense} >= {n for n in cc.LENGTHS if n >= 15}


@pytest.mark.parametrize("shape", cc.TS_SHAPES)
def test_dropped_bounds_under_5_percent(shape):
    kept, dropped = cc.clamps(shape)
    assert dropped * 20 < len(kept) + dropped
    if shape != "ten_byte":
        assert dropped == 0
    rows = set(cc.boundary_rows(shape))
    last = len(cc.ts_axis(shape)) - 1
    assert {0, 1, last - 1, last} <= rows
    if last > 130:
        assert {62, 63, 64, 65, 126, 127, 128, 129} <= rows


# ---- oracle vs per-row restatement -------------------------------------
def _check_part(part, clamp_list):
    vtype = VT_FLOAT64 if part.float_vals else VT_INT64
    payload, blocks = oracle_blocks(part.builder())
    n_sel = 0
    for r0, r1, dl, dh, lo, hi in clamp_list:
        orc = o.scan_agg(payload, blocks, vtype, min_ts=lo, max_ts=hi,
                         n_groups=part.n_groups)
        ref = cc.ref_part(part, lo, hi)
        for i, (g, (cnt, s, mn, mx)) in enumerate(zip(orc, ref)):
            where = (part.name, i, part.blocks[i].n, part.blocks[i].kind,
                     (r0, r1, dl, dh))
            assert g.count == cnt, where
            if not cnt:
                continue
            n_sel += 1
            if part.float_vals:
                assert (g.min_f, g.max_f) == (mn, mx), where
                assert f64_sum_close(g.sum_f, math.fsum(s), cnt), where
            else:
                assert (g.sum_i, g.min_i, g.max_i) == (s, mn, mx), where
    return n_sel


@pytest.mark.parametrize("shape", cc.TS_SHAPES)
def test_oracle_matches_per_row_i64(shape):
    assert _check_part(cc.ts_part(shape), cc.clamps(shape)[0]) > 0


@pytest.mark.parametrize("shape", cc.TS_SHAPES)
def test_oracle_matches_per_row_f64(shape):
    assert _check_part(cc.ts_part(shape, True), cc.clamps(shape)[0]) > 0


def test_oracle_matches_per_row_extremes():
    whole = [(0, 0, 0, 0, cc.INT64_MIN, cc.INT64_MAX)]
    for part in (cc.extremes_part(), cc.extremes_f64_part()):
        rows = [(r0, r1, 0, 0, cc.T0 + r0 * cc.MS, cc.T0 + r1 * cc.MS)
                for r0, r1 in ((0, 8191), (1, 8190), (4000, 4002),
                               (4001, 4001), (17, 8175))]
        assert _check_part(part, whole + rows) > 0


def test_oracle_matches_per_row_length_sweep():
    pb = cc.lengths_builder()
    payload, blocks = oracle_blocks(pb)
    orc = o.scan_agg(payload, blocks, VT_INT64, n_groups=len(blocks))
    for i, case in enumerate(cc.length_cases()):
        vals = case[2]
        g = orc[2 * i + 1]
        assert (g.count, g.sum_i, g.min_i, g.max_i) == (
            len(vals), cc.wrap64(sum(vals)), min(vals), max(vals)), i


def _tag_keep(tag):
    return lambda blk, i: blk.tags[i] == tag


def test_oracle_matches_per_row_tagged():
    """Group-by and predicate on the per-row tag, under the clamps the GPU
    tests use and unclamped."""
    whole = (0, 0, 0, 0, cc.INT64_MIN, cc.INT64_MAX)
    for part, cl in ((cc.tag_part(), cc.tag_clamps()),
                     (cc.extremes_tag_part(), [whole])):
        payload, blocks = oracle_blocks(part.builder())
        for r0, r1, dl, dh, lo, hi in cl:
            by = o.scan_agg_bytag(payload, blocks, VT_INT64, 0, cc.TAGS,
                                  lo, hi)
            for t, g in zip(cc.TAGS, by):
                ref = cc.ref_part(part, lo, hi, keep=_tag_keep(t))
                cnt = sum(r[0] for r in ref)
                assert g.count == cnt, (part.name, t, r0, r1, dl, dh)
                if cnt:
                    assert g.sum_i == cc.wrap64(sum(r[1] for r in ref))
                    assert g.min_i == min(r[2] for r in ref if r[0])
                    assert g.max_i == max(r[3] for r in ref if r[0])
            pred = cc.TAGS[(r0 + r1) % len(cc.TAGS)]
            orc = o.scan_agg(payload, blocks, VT_INT64, min_ts=lo, max_ts=hi,
                             pred=pred, n_groups=part.n_groups)
            ref = cc.ref_part(part, lo, hi, keep=_tag_keep(pred))
            for g, (cnt, s, mn, mx) in zip(orc, ref):
                assert g.count == cnt, (part.name, pred, r0, r1, dl, dh)
                if cnt:
                    assert (g.sum_i, g.min_i, g.max_i) == (s, mn, mx)
