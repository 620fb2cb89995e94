"""The generic 64-byte varint window step in its three consumers, on
the lists of varint_walk_cases: varints of 2, 3, 5, 9 and 10 bytes that
cross the window boundary behind 1 to 9 carried bytes, as Delta and as
DeltaOfDelta lists.

  field column   scan_stream          oracle.scan_agg per block
  timestamps     clamp_count_stream   oracle.scan_agg per block and clamp
  dedup          dedup_decode_stream  row_dedup_ref survivors, then the oracle

The CPU test at the top reads the encoded streams and decides whether the
lists are the ones described."""
import pytest

import clamp_cases as cc
import oracle as o
import row_dedup_cases as rdc
import row_dedup_ref as ref
import varint_walk_cases as vw
from banyandb_amd import (Session, VT_INT64, AGG_SUM, AGG_COUNT, AGG_MIN,
                          AGG_MAX)
from helpers import oracle_blocks
from test_gpu_row_dedup import assert_parity, expected, gpu as run_scen
from test_gpu_ts_clamp import VALUE_SCAN, _sweep

gpu = pytest.mark.gpu


# ---------------------------------------------------------------------
# what the streams hold (CPU)
# ---------------------------------------------------------------------
def _field_streams():
    pb = vw.field_part().builder()
    payload = pb.payload
    for d in pb.blocks():
        yield d.field_enc, bytes(payload[d.field_off:d.field_off + d.field_len])


def _ts_streams():
    blocks = vw.clamp_blocks()
    rp = rdc.RawPart(list(blocks))
    for d, b in zip(rp.blocks(), blocks):
        enc = d.ts_enc_with_version
        assert enc == (rdc.ENC_DELTA_WV if b.raw_delta_ts else cc.ENC_DOD_WV)
        yield (vw.ENC_DELTA if b.raw_delta_ts else vw.ENC_DOD,
               bytes(rp._buf[d.ts_off:d.ts_off + d.ts_len]))


@pytest.mark.parametrize("streams", [_field_streams, _ts_streams],
                         ids=["field", "timestamps"])
def test_lists_cross_the_window_with_every_carry(streams):
    carries = {vw.ENC_DELTA: set(), vw.ENC_DOD: set()}
    longest = {vw.ENC_DELTA: 0, vw.ENC_DOD: 0}
    n = 0
    for enc, stream in streams():
        assert enc in carries, enc
        start = vw.skip_varint(stream) if enc == vw.ENC_DOD else 0
        for carried, length in vw.crossings(stream, start):
            carries[enc].add(carried)
        longest[enc] = max(longest[enc],
                           max(cc.varint_lengths(stream[start:])))
        n += 1
    assert n == 2 * len(vw.SHAPES)
    for enc in carries:
        assert carries[enc] >= set(range(1, 10)), (enc, sorted(carries[enc]))
        assert longest[enc] == 10, (enc, longest[enc])


def test_first_crossing_is_the_shape_s():
    """Each list's first crossing varint is `width` bytes long behind
    64 - pad bytes, whenever the shape says it crosses."""
    streams = list(_field_streams())
    for k, (pad, w) in enumerate(vw.SHAPES):
        for enc, stream in streams[2 * k:2 * k + 2]:
            start = vw.skip_varint(stream) if enc == vw.ENC_DOD else 0
            cr = vw.crossings(stream, start)
            if pad + w > 64:
                assert cr[0] == (64 - pad, w), (pad, w, enc, cr[:2])
            # the second pair starts on the last byte of the window at 128
            assert (1, w) in cr, (pad, w, enc, cr)


# ---------------------------------------------------------------------
# 1. field column: scan_stream
# ---------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("pred", [b"", cc.TAGS[0]], ids=["plain", "walkers"])
def test_field_value_scan(pred):
    """SUM/COUNT/MIN/MAX per block: the whole range (the clamp-free
    instantiation), two clamps ending in the wide varints' rows (the
    selecting branch), and all three under a row-varying tag predicate,
    where every window takes the generic step."""
    part = vw.field_part()
    encs = [d.field_enc for d in part.builder().blocks()]
    assert encs == [vw.ENC_DELTA, vw.ENC_DOD] * len(vw.SHAPES)
    _sweep(part, vw.field_clamps(), VALUE_SCAN, pred=pred)


# ---------------------------------------------------------------------
# 2. timestamps: clamp_count_stream
# ---------------------------------------------------------------------
@gpu
def test_timestamp_clamp_counts():
    blocks = list(vw.clamp_blocks())
    n = len(blocks)
    payload, oblocks = oracle_blocks(rdc.builder(blocks))
    clamps = vw.ts_clamps()
    s = Session(0)
    s.upload_part(rdc.RawPart(blocks))
    s.configure(VT_INT64, [AGG_SUM, AGG_COUNT], n_groups=n)
    n_sel = 0
    try:
        for lo, hi in clamps:
            want = o.scan_agg(payload, oblocks, VT_INT64, min_ts=lo, max_ts=hi,
                              n_groups=n)
            s.reset()
            s.consume(min_ts=lo, max_ts=hi)
            got = s.finalize()
            for i, (g, w) in enumerate(zip(got, want)):
                assert (g.count, g.sum_i) == (w.count, w.sum_i), \
                    (i, blocks[i].raw_delta_ts, lo, hi)
                n_sel += bool(w.count)
    finally:
        s.close()
    print("clamps", len(clamps), "selecting block partials", n_sel)
    assert n_sel >= len(clamps)


# ---------------------------------------------------------------------
# 3. dedup: dedup_decode_stream
# ---------------------------------------------------------------------
@gpu
def test_dedup_survivors():
    blocks = list(vw.dedup_blocks())
    scen = rdc.Scen(blocks, group=("code", len(blocks) // 3))
    want = expected(scen, ref.merged(scen.blocks))
    got, stats = run_scen(scen, funcs=[AGG_SUM, AGG_COUNT, AGG_MIN, AGG_MAX])
    census = ref.stats(scen.blocks)
    print("stats", stats, "model", census)
    assert stats == census
    assert_parity(scen, got, want, "varint_walk")
    # every axis keeps exactly one row per timestamp
    assert [w.count for w in want] == [len(b.ts) for b in blocks[::3]]
