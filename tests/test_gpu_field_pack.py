"""The nibble-packed dense field streams on the GPU (bydb_set_field_pack).

Every case scans the same resident part with packing OFF and ON under the
streaming policy: the results must be byte-identical, exact against the
oracle, and bydb_field_pack_stats must report exactly the blocks that the
Python reference rule (field_pack_ref.packs) packs — so a build that
silently packed nothing, or something else, fails.  The stats come from the
build: that the scan then reads the slots (and not the byte streams beside
them) shows only in its traffic and its time, which profiles/field_pack.txt
records; what these cases pin down is that whichever stream a block is
folded from, the result is the same.  Every input named "packed" is checked
here, on the host, to pack all of its candidate blocks."""
import functools
import random
import struct

import pytest

from banyandb_amd import (PartBuilder, Session, VT_INT64, VT_FLOAT64, AGG_SUM,
                          AGG_COUNT, STREAM_AUTO, STREAM_CACHED,
                          STREAM_STREAMING, PACK_AUTO, PACK_OFF, PACK_ON, lib)
import field_pack_ref as ref
from field_pack_ref import (ENC_CONST, ENC_DELTA_CONST, ENC_DELTA, ENC_DOD,
                            RawPart, T0, MS, I64)
from helpers import oracle_scan

gpu = pytest.mark.gpu

TOP, BOT = I64 - 1, -I64
LAUNCH_WAVES = 8192 * 4
SIZES = [2, 3, 4, 33, 34, 2049, 2050, 4097, 8191, 8192]


def _bits(res):
    """Everything a sum+count scan defines, as bytes."""
    return [struct.pack("<qqd", g.count, g.sum_i, g.sum_f) for g in res]


def _pairs(res):
    return [(g.count, g.sum_i) for g in res]


def _scan(part, n_groups, pack, policy=STREAM_STREAMING, clamps=({},),
          vtype=VT_INT64, float_exp=0, dedup=0):
    """One session: per clamp the finalized results, then the pack stats."""
    s = Session(0)
    out = []
    try:
        s.upload_part(part)
        s.configure(vtype, [AGG_SUM, AGG_COUNT], n_groups=n_groups,
                    float_exp=float_exp)
        s.set_stream_policy(policy)
        s.set_field_pack(pack)
        s.set_row_dedup(dedup)
        for kw in clamps:
            s.reset()
            s.consume(**kw)
            out.append(s.finalize())
        return out, s.field_pack_stats()
    finally:
        s.close()


def _on_off_oracle(part, n_groups, clamps=({},), all_packed=True):
    """The condition every case shares; returns the ON results."""
    cand, hit, nbytes = ref.census(part)
    if all_packed:
        assert cand == hit == part.n_blocks > 0
    off, st_off = _scan(part, n_groups, PACK_OFF, clamps=clamps)
    on, st_on = _scan(part, n_groups, PACK_ON, clamps=clamps)
    assert st_off == [0, 0, 0, 0]
    assert st_on[:3] == [cand, hit, nbytes], (st_on, cand, hit, nbytes)
    assert st_on[3] == sum(ref.slot_bytes(d.count) for d in part.blocks()
                           if ref.candidate(d))
    for kw, a, b in zip(clamps, on, off):
        assert _bits(a) == _bits(b), kw
        want = oracle_scan(part, VT_INT64, n_groups=n_groups, **kw)
        assert _pairs(a) == _pairs(want), kw
    return on


def _patterns(n_deltas):
    alt = [(-8, 7)[j % 2] for j in range(n_deltas)]
    return [[-8] * n_deltas, [7] * n_deltas, alt, [-x - 1 for x in alt]]


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_single_blocks_at_the_extremes(n):
    """All deltas -8, all +7 and the two alternating, first value at both
    int64 extremes (the sums wrap mod 2^64); one block per group.  The sizes
    put the last nibble on either half of a byte, on both sides of the lane
    boundary (32 nibbles) and the chunk boundary (2048), in one to four
    chunks."""
    p = RawPart()
    g = 0
    for first in (TOP, BOT):
        for deltas in _patterns(n - 1):
            p.add_delta(g + 1, first, deltas, group_code=g)
            g += 1
    res = _on_off_oracle(p, g)[0]
    assert [r.count for r in res] == [n] * g
    for r, d in zip(res, p.blocks()):
        stream = p.payload[d.field_off:d.field_off + d.field_len]
        deltas = [(z >> 1) ^ -(z & 1) for z in stream]
        assert r.sum_i == ref.wrap(sum(ref.block_values(d.field_first,
                                                        deltas)))


@gpu
@pytest.mark.parametrize("n", [34, 2050, 8192])
def test_one_delta_out_of_range_stays_unpacked(n):
    """One delta of +8 or -9 at the first, the middle or the last position
    keeps its block on the byte stream, among packed neighbours."""
    rng = random.Random(n)
    p = RawPart()
    g = 0
    bad_at = []
    for bad in (8, -9):
        for pos in (0, (n - 1) // 2, n - 2):
            for odd in (False, True):
                deltas = [rng.randint(-8, 7) for _ in range(n - 1)]
                if odd:
                    deltas[pos] = bad
                    bad_at.append(g)
                p.add_delta(g + 1, rng.choice((TOP, BOT, 12345)), deltas,
                            group_code=g)
                g += 1
    got = [ref.packs(p.payload, d) for d in p.blocks()]
    assert got == [i not in bad_at for i in range(g)] and len(bad_at) == 6
    _on_off_oracle(p, g, all_packed=False)


@functools.lru_cache(maxsize=None)
def _other_encodings():
    """One block each that is no candidate: multi-byte delta, delta of
    delta, const, delta-const."""
    rng = random.Random(0x07E4)
    b = PartBuilder()
    n = 40
    ts = [T0 + i * MS for i in range(n)]

    def accum(span):
        out, v = [0], 0
        for i in range(n - 1):
            v += rng.randint(-span, span) if i >= 2 else (span, -span)[i]
            out.append(v)
        return out
    b.add_block_i64(1, ts, [1] * n, [ref.wrap(TOP - 10 ** 6 + x)
                                     for x in accum(10 ** 9)], group_code=3)
    b.add_block_i64(2, ts, [1] * n, [ref.wrap(BOT + 5 + x) for x in accum(3)],
                    group_code=4)
    b.add_block_i64(3, ts, [1] * n, [BOT] * n, group_code=5)
    b.add_block_i64(4, ts, [1] * n, [ref.wrap(TOP - 7 + 5 * i)
                                     for i in range(n)], group_code=6)
    descs = b.blocks()
    assert [d.field_enc for d in descs] == [ENC_DELTA, ENC_DOD, ENC_CONST,
                                            ENC_DELTA_CONST]
    assert descs[0].field_len > n - 1
    return b


@functools.lru_cache(maxsize=None)
def _interleaved():
    """More blocks than the launch has waves, every kind next to every
    other, so each wave goes round the kernel loop with the table entry
    fetched one block ahead: packed, unpacked dense, and the four other
    encodings; a period of 11 blocks, which does not divide the wave
    count."""
    rng = random.Random(0x1EAF)
    p = RawPart()
    others = _other_encodings()
    sid = 0
    while p.n_blocks <= LAUNCH_WAVES + 3000:
        for k in range(7):
            n = rng.choice((2, 3, 9, 34, 65, 130))
            wide = k in (2, 5)
            lo, hi = (-64, 63) if wide else (-8, 7)
            deltas = [rng.randint(lo, hi) for _ in range(n - 1)]
            if wide:
                deltas[rng.randrange(n - 1)] = rng.choice((8, -9, 63, -64))
            sid += 1
            p.add_delta(sid, rng.choice((TOP, BOT, rng.randint(-99, 99))),
                        deltas, group_code=1 if wide else (0, 2)[k % 2])
        p.add_builder(others, sid0=sid)
        sid += others.n_blocks
    return p


@gpu
def test_interleaved_kinds_more_blocks_than_waves():
    p = _interleaved()
    assert p.n_blocks > LAUNCH_WAVES
    cand, hit, _ = ref.census(p)
    per = p.n_blocks // 11
    assert (cand, hit) == (7 * per, 5 * per) and p.n_blocks == 11 * per
    # rows 0..33: the blocks of up to 34 rows whole, the longer ones cut
    clamps = ({}, dict(min_ts=T0, max_ts=T0 + 33 * MS))
    on = _on_off_oracle(p, 7, clamps=clamps, all_packed=False)
    assert all(r.count > 0 for r in on[0])


@gpu
def test_time_clamps_cover_packed_blocks_whole_and_cut_one():
    """Six packed 1000-row blocks in a row on the time axis, one group
    each: a clamp that covers a block whole folds its nibbles, the block a
    clamp cuts folds from its byte stream."""
    rng = random.Random(0xC1A3)
    p = RawPart()
    rows = 1000
    for g in range(6):
        p.add_delta(1, rng.choice((TOP, BOT)),
                    [rng.randint(-8, 7) for _ in range(rows - 1)],
                    group_code=g, row0=g * rows)
    spans = [(0, 5999), (1000, 3999), (1000, 4500), (999, 3999), (1001, 3999),
             (2500, 2500), (2000, 2999), (2000, 2998), (0, 0), (5999, 5999),
             (3000, 5998), (500, 5500)]
    clamps = [dict(min_ts=T0 + a * MS, max_ts=T0 + b * MS) for a, b in spans]
    on = _on_off_oracle(p, 6, clamps=clamps)
    for (a, b), res in zip(spans, on):
        assert sum(r.count for r in res) == b - a + 1


@gpu
def test_block_code_grouping_over_packed_blocks():
    """The group256 shape, shrunk: generated series (ramp 1, noise -3..3),
    two blocks each, 256 block-code groups."""
    b = PartBuilder()
    n_series, n_dp = 300, 9000
    b.gen_bulk_i64(0, n_series, n_dp, T0, MS, 1000, 1, 0xB4DB, group_mod=256,
                   threads=4)
    assert b.n_blocks == 2 * n_series
    on = _on_off_oracle(b, 256)[0]
    assert sum(r.count for r in on) == n_series * n_dp


@gpu
def test_float64_decimal_session():
    """sum+count of a float64 decimal session whose mantissa deltas
    qualify.  One block per group: a group's sum is one exact integer times
    10^exp, so it is the same bits whichever stream was read."""
    rng = random.Random(0xF10A)
    b = PartBuilder()
    cents_of = []
    for g, n in enumerate((2050, 8192, 35, 4097)):
        cents = [rng.randint(10 ** 4, 10 ** 6)]
        for i in range(n - 1):
            cents.append(cents[-1] + ((1, -2)[i] if i < 2
                                      else rng.randint(-8, 7)))
        ts = [T0 + i * MS for i in range(n)]
        b.add_block_f64(g + 1, ts, [1] * n, [c / 100.0 for c in cents],
                        group_code=g)
        cents_of.append(cents)
    descs = b.blocks()
    assert all(d.exp == -2 and d.field_enc == ENC_DELTA for d in descs)
    cand, hit, nbytes = ref.census(b)
    assert cand == hit == 4
    kw = dict(vtype=VT_FLOAT64, float_exp=-2)
    off, st_off = _scan(b, 4, PACK_OFF, **kw)
    on, st_on = _scan(b, 4, PACK_ON, **kw)
    assert st_off == [0, 0, 0, 0] and st_on[:3] == [4, 4, nbytes]
    assert _bits(on[0]) == _bits(off[0])
    want = oracle_scan(b, VT_FLOAT64, n_groups=4)
    for r, w, cents in zip(on[0], want, cents_of):
        assert r.count == w.count == len(cents)
        # the tolerance of the float64 parity tests: the oracle adds row by
        # row, the engine one exact mantissa sum per block
        assert r.sum_f == pytest.approx(w.sum_f, rel=1e-9)


@functools.lru_cache(maxsize=None)
def _dedup_part(resend):
    rng = random.Random(0xDED0)
    p = RawPart()
    rows = 500
    for g in range(5):
        p.add_delta(g + 1, rng.randint(-10 ** 6, 10 ** 6),
                    [rng.randint(-8, 7) for _ in range(rows - 1)],
                    group_code=g)
    if resend:
        d = p.blocks()[2]
        stream = p.payload[d.field_off:d.field_off + d.field_len]
        p.add_delta(3, d.field_first, [(z >> 1) ^ -(z & 1) for z in stream],
                    group_code=2)
    return p


@gpu
def test_row_dedup_without_peers_scans_packed():
    p = _dedup_part(False)
    want = _pairs(oracle_scan(p, VT_INT64, n_groups=5))
    off, _ = _scan(p, 5, PACK_OFF, dedup=1)
    on, st = _scan(p, 5, PACK_ON, dedup=1)
    assert st[:2] == [5, 5]
    assert _bits(on[0]) == _bits(off[0]) and _pairs(on[0]) == want


@gpu
def test_row_dedup_with_a_resent_block_leaves_packed_data_unused():
    """A re-sent block (same series, timestamps and version) is superseded
    whole; the scan then runs predicated and builds no packed copy."""
    want = _pairs(oracle_scan(_dedup_part(False), VT_INT64, n_groups=5))
    p = _dedup_part(True)
    assert ref.census(p)[:2] == (6, 6)
    off, _ = _scan(p, 5, PACK_OFF, dedup=1)
    on, st = _scan(p, 5, PACK_ON, dedup=1)
    assert st == [0, 0, 0, 0]
    assert _bits(on[0]) == _bits(off[0]) and _pairs(on[0]) == want


def _small(base, sid0, kinds):
    """kinds: per block True for deltas in -8..7, False for one beyond."""
    rng = random.Random(sid0)
    p = RawPart(base)
    for k, packed in enumerate(kinds):
        deltas = [rng.randint(-8, 7) for _ in range(99)]
        if not packed:
            deltas[50] = 20
        p.add_delta(sid0 + k, 1000 * k, deltas)
    return p


@gpu
def test_state_follows_append_clear_and_reserve():
    s = Session(0)
    try:
        a = _small(0, 1, [True, True, False])
        b = _small(a.payload_len, 10, [True, False])
        ab = _small(0, 1, [True, True, False])
        ab.extend(b)
        c = _small(0, 20, [False, True, True, True])
        s.reserve(a.payload_len + b.payload_len + c.payload_len, 16)
        s.configure(VT_INT64, [AGG_SUM, AGG_COUNT])
        s.set_stream_policy(STREAM_STREAMING)
        s.set_field_pack(PACK_ON)

        def step(part):
            s.reset()
            s.consume()
            got = _pairs(s.finalize())
            assert got == _pairs(oracle_scan(part, VT_INT64))
            cand, hit, nbytes = ref.census(part)
            assert s.field_pack_stats()[:3] == [cand, hit, nbytes]
            return hit
        assert s.field_pack_stats() == [0, 0, 0, 0]      # nothing built yet
        s.append(a)
        assert step(a) == 2
        s.append(b)                                       # rebuilt: 5 blocks
        assert step(ab) == 3
        s.set_field_pack(PACK_OFF)
        assert s.field_pack_stats() == [0, 0, 0, 0]
        s.set_field_pack(PACK_AUTO)       # streaming is forced: AUTO packs
        assert step(ab) == 3
        s.set_stream_policy(STREAM_AUTO)  # a small part resolves to cached:
        assert s.field_pack_stats() == [0, 0, 0, 0]   # nothing is read
        s.set_stream_policy(STREAM_STREAMING)
        s.set_field_pack(PACK_ON)         # a change of mode builds again
        assert step(ab) == 3
        s.clear_part()
        s.append(c)
        assert step(c) == 3
        s.upload_part(a)                                  # a new reserve
        assert step(a) == 2
    finally:
        s.close()


@gpu
def test_auto_follows_the_stream_policy():
    """AUTO packs exactly when the stream-load policy resolves to streaming:
    not for a small part under the default policy, yes once streaming is
    forced.  ON packs for any size, whatever the policy."""
    p = _small(0, 1, [True, True, False, True])
    assert lib().bydb_stream_policy_pick(STREAM_AUTO, p.payload_len) == \
        STREAM_CACHED
    want = _pairs(oracle_scan(p, VT_INT64))
    for pack, policy, packed in ((PACK_AUTO, STREAM_AUTO, 0),
                                 (PACK_AUTO, STREAM_CACHED, 0),
                                 (PACK_AUTO, STREAM_STREAMING, 3),
                                 (PACK_OFF, STREAM_STREAMING, 0),
                                 (PACK_ON, STREAM_AUTO, 3),
                                 (PACK_ON, STREAM_CACHED, 3)):
        res, st = _scan(p, 1, pack, policy=policy)
        assert _pairs(res[0]) == want, (pack, policy)
        assert st[1] == packed, (pack, policy, st)
        assert st[0] == (4 if packed else 0)
    s = Session(0)
    try:
        assert lib().bydb_set_field_pack(s._h, 3) < 0
        assert lib().bydb_set_field_pack(s._h, -1) < 0
    finally:
        s.close()
