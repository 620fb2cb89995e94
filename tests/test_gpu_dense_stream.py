"""The dense one-byte delta fold of the closed-form scan under both stream
load policies, cached (plain loads) and streaming (non-temporal loads):

- long dense blocks on every head offset 0..127 within a 128-byte memory
  line, with and without a ninth chunk, whole part, as the last stream of
  a part, and clamped around the lane, line and chunk boundaries;
- parts with more blocks than the launch has waves (8192 workgroups x 4),
  so a wave goes round the kernel loop again (prefetched descriptor,
  per-wave partial carried over);
- const, delta-const, multi-byte delta, delta-of-delta and dense blocks at
  the int64 extremes in front of such a part.

Sums and counts are exact against the oracle."""
import functools
import random

import pytest

from banyandb_amd import (PartBuilder, Session, VT_INT64, AGG_SUM, AGG_COUNT,
                          STREAM_AUTO, STREAM_CACHED, STREAM_STREAMING, lib)
from helpers import oracle_scan

gpu = pytest.mark.gpu

T0 = 1_700_000_000_000_000_000
MS = 10 ** 6
ENC_CONST, ENC_DELTA_CONST, ENC_DELTA, ENC_DOD = 1, 2, 3, 4
LINE = 128
CHUNK = 1024
# the scan launches at most 8192 workgroups of 4 waves; a part with more
# blocks than this sends waves round the kernel loop a second time
LAUNCH_WAVES = 8192 * 4
POLICIES = [pytest.param(STREAM_CACHED, id="cached"),
            pytest.param(STREAM_STREAMING, id="streaming")]
I64 = 1 << 63


def _wrap(v):
    return (v + I64) % (1 << 64) - I64


def _is_dense(d):
    return d.field_enc == ENC_DELTA and d.field_len == d.count - 1


def _ts(n):
    return [T0 + i * MS for i in range(n)]


def _walk(rng, n, span, start=None):
    """Non-monotone walk from a positive start: the encoder takes Delta,
    and every zigzag delta fits one byte (-64..63)."""
    v = rng.randint(10 ** 8, 10 ** 9) if start is None else start
    out = [v]
    for i in range(n - 1):
        # one rise, one fall first: neither monotone nor const
        v += rng.randint(-span - 1, span) if i >= 2 else (1, -2)[i]
        out.append(v)
    return [_wrap(x) for x in out]


def _add_dense(b, sid, vals, group_code=0):
    n = len(vals)
    b.add_block_i64(sid, _ts(n), [1] * n, vals, group_code=group_code)


def _add_filler(b, rng, sid, k, group_code=0):
    """A small dense block whose encoded size grows by one byte per row, so
    the next block's field_off lands where it is wanted."""
    assert k >= 3
    _add_dense(b, sid, _walk(rng, k, 3), group_code)


@functools.lru_cache(maxsize=None)
def _layout():
    """(bytes a k-row filler takes beyond k, field_off of a long block
    relative to the payload length before it)."""
    rng = random.Random(1)
    b = PartBuilder()
    _add_filler(b, rng, 1, 3)
    s3 = b.payload_len
    _add_filler(b, rng, 2, 50)
    s50 = b.payload_len - s3
    assert s50 - 50 == s3 - 3
    p = b.payload_len
    _add_dense(b, 3, _walk(rng, 8192, 3))
    return s3 - 3, b.blocks()[-1].field_off - p


def _add_at(b, rng, sid, head, vals, group_code=0, filler_group=None):
    """Append a filler and then `vals` so that field_off % 128 == head."""
    c0, rel = _layout()
    k = 3 + (head - (b.payload_len + c0 + 3 + rel)) % LINE
    _add_filler(b, rng, sid, k,
                group_code if filler_group is None else filler_group)
    _add_dense(b, sid + 1, vals, group_code)
    d = b.blocks()[-1]
    assert _is_dense(d) and d.field_off % LINE == head, (head, d.field_off)


@functools.lru_cache(maxsize=None)
def _head_part():
    """Per head offset 0..127 a full-length block (needs the ninth chunk
    from offset 2 on) and one short enough never to need it; deltas over
    -3..3 and over the whole one-byte span alternate.  Every block is its
    own group, so no two errors cancel."""
    rng = random.Random(0x5EED)
    b = PartBuilder()
    g = 0
    for head in range(LINE):
        for n in (8192, 8050 + head % 7):
            span = 3 if (head + n) % 2 else 63
            _add_at(b, rng, 2 * g + 1, head, _walk(rng, n, span),
                    group_code=g)
            g += 1
    return b, g


def _check_head_part():
    b, _ = _head_part()
    long_ = [d for d in b.blocks() if _is_dense(d) and d.count >= 8050]
    assert {d.field_off % LINE for d in long_} == set(range(LINE))
    nine = [d for d in long_ if d.field_off % LINE + d.field_len > 8 * CHUNK]
    eight = [d for d in long_ if d.field_off % LINE + d.field_len <= 8 * CHUNK]
    assert {d.field_off % LINE for d in eight} == set(range(LINE))
    assert {d.field_off % LINE for d in nine} == set(range(2, LINE))


def _pairs(res):
    return [(g.count, g.sum_i) for g in res]


def _scan(b, n_groups, policy, clamps=({},)):
    s = Session(0)
    out = []
    try:
        s.upload_part(b)
        s.configure(VT_INT64, [AGG_SUM, AGG_COUNT], n_groups=n_groups)
        s.set_stream_policy(policy)
        for kw in clamps:
            s.reset()
            s.consume(**kw)
            out.append(_pairs(s.finalize()))
    finally:
        s.close()
    return out


@functools.lru_cache(maxsize=None)
def _head_oracle():
    b, g = _head_part()
    return _pairs(oracle_scan(b, VT_INT64, n_groups=g))


def test_policy_follows_payload_size():
    """Host side: what auto resolves to, and that a forced policy holds."""
    pick = lib().bydb_stream_policy_pick
    cache = 256 << 20
    for nbytes, want in ((0, STREAM_CACHED), (220 * 10 ** 6, STREAM_CACHED),
                         (cache, STREAM_CACHED), (cache + 1, STREAM_STREAMING),
                         (10 ** 10, STREAM_STREAMING)):
        assert pick(STREAM_AUTO, nbytes) == want, nbytes
        assert pick(STREAM_CACHED, nbytes) == STREAM_CACHED
        assert pick(STREAM_STREAMING, nbytes) == STREAM_STREAMING
    assert pick(3, 0) < 0 and pick(-1, 0) < 0


def test_head_sweep_selects_every_offset():
    _check_head_part()


@gpu
@pytest.mark.parametrize("policy", POLICIES)
def test_head_sweep_whole_part(policy):
    _check_head_part()
    b, g = _head_part()
    got = _scan(b, g, policy)[0]
    want = _head_oracle()
    assert all(w[0] >= 8050 for w in want) and len(want) == 2 * LINE
    bad = [i for i in range(g) if got[i] != want[i]]
    assert not bad, [(i, b.blocks()[2 * i + 1].field_off % LINE) for i in bad]


@gpu
@pytest.mark.parametrize("policy", POLICIES)
def test_head_offsets_block_last(policy):
    """A full-length and a five-byte block as the last stream of a part of
    their own: the reads below the stream and past its end leave it."""
    rng = random.Random(0x1A57)
    for head in (0, 1, 15, 16, 17, 112, 127):
        for n in (8192, 6):
            b = PartBuilder()
            _add_at(b, rng, 1, head, _walk(rng, n, 63))
            d = b.blocks()[-1]
            assert d.field_off + d.field_len == b.payload_len
            want = _pairs(oracle_scan(b, VT_INT64))
            assert _scan(b, 1, policy)[0] == want, (head, n)


@functools.lru_cache(maxsize=None)
def _clamp_part():
    rng = random.Random(0xC1A4)
    heads = (0, 1, 77, 127)
    b = PartBuilder()
    for g, head in enumerate(heads):
        # the fillers share a group of their own, the last
        _add_at(b, rng, 2 * g + 1, head, _walk(rng, 8192, 63), group_code=g,
                filler_group=len(heads))
    return b, heads


def _clamp_rows(heads):
    """Delta byte j-1 of a stream at head offset a sits a + j - 1 bytes
    past the start of its 128-byte line, so for each offset (and for 0,
    the stream-relative view) the rows land -1, 0, +1 around the lane,
    line and chunk boundaries in memory and around the five-chunk batch of
    the clamped fold."""
    last = 8191
    rows = set()
    for a in sorted({0} | set(heads)):
        for m in (16, 128, 256, 1024, 1152, 2048, 4096, 5120, 5248, 7168,
                  8064, 8192):
            for k in (-1, 0, 1):
                r = m - a + k
                if 0 <= r <= last:
                    rows.add(r)
    pairs = [(r, last) for r in sorted(rows | {0, 1, 2, last - 1, last})]
    pairs += [(0, r) for r in sorted(rows | {0, 1, last - 2, last - 1})]
    pairs += [(127, 129), (128, 128), (1023, 1025), (1024, 1024),
              (129, 8063), (1025, 5119), (5121, 5121), (last, last)]
    return pairs


@functools.lru_cache(maxsize=None)
def _clamp_oracle():
    b, heads = _clamp_part()
    clamps = [dict(min_ts=T0 + r0 * MS, max_ts=T0 + r1 * MS)
              for r0, r1 in _clamp_rows(heads)]
    return clamps, [_pairs(oracle_scan(b, VT_INT64, n_groups=len(heads) + 1,
                                       **kw))
                    for kw in clamps]


@gpu
@pytest.mark.parametrize("policy", POLICIES)
def test_clamp_sweep_line_and_chunk_boundaries(policy):
    b, heads = _clamp_part()
    clamps, want = _clamp_oracle()
    got = _scan(b, len(heads) + 1, policy, clamps)
    for pair, g, w in zip(_clamp_rows(heads), got, want):
        assert all(c == pair[1] - pair[0] + 1 for c, _ in w[:-1])
        assert g == w, pair


N_BULK = 36000
BULK_CLAMP = dict(min_ts=T0 + 7 * MS, max_ts=T0 + 33 * MS)


@functools.lru_cache(maxsize=None)
def _bulk(group_mod):
    b = PartBuilder()
    b.gen_bulk_i64(0, N_BULK, 40, T0, MS, 1000, 1, 0xB4DB,
                   group_mod=group_mod, threads=4)
    n_groups = max(group_mod, 1)
    want = [_pairs(oracle_scan(b, VT_INT64, n_groups=n_groups, **kw))
            for kw in ({}, BULK_CLAMP)]
    return b, n_groups, want


@gpu
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("group_mod", [0, 3])
def test_more_blocks_than_waves(group_mod, policy):
    b, n_groups, want = _bulk(group_mod)
    descs = b.blocks()
    assert len(descs) == N_BULK > LAUNCH_WAVES
    assert all(_is_dense(d) for d in descs)
    assert sum(c for c, _ in want[0]) == N_BULK * 40
    assert sum(c for c, _ in want[1]) == N_BULK * 27
    got = _scan(b, n_groups, policy, ({}, BULK_CLAMP))
    assert got == want


@functools.lru_cache(maxsize=None)
def _mixed():
    """Hand-made blocks of every closed-form encoding at the int64
    extremes, two group codes, then enough generated dense blocks that the
    waves of the hand-made ones come round again."""
    rng = random.Random(0x3A1D)
    top, bot = I64 - 1, -I64
    b = PartBuilder()
    n_hand = 0
    for k in range(60):
        n = (5, 40, 257, 1030, 41)[k % 5]
        g = k % 2
        shapes = [
            [top if k % 4 < 2 else bot] * n,                       # const
            [_wrap(top - 7 + (3 + k) * i) for i in range(n)],      # delta-const
            [_wrap(top - 10 ** 6 + x)
             for x in _accum(rng, n, 10 ** 9)],                    # multi-byte
            [_wrap(bot + 5 + x) for x in _accum(rng, n, 3)],       # dod (first < 0)
            _walk(rng, n, 63, start=top - 40),                     # dense
        ]
        for vals in shapes:
            n_hand += 1
            b.add_block_i64(n_hand, _ts(n), [1] * n, vals, group_code=g)
    encs = [d.field_enc for d in b.blocks()]
    descs = b.blocks()
    assert encs.count(ENC_CONST) == 60 and encs.count(ENC_DELTA_CONST) == 60
    assert encs.count(ENC_DOD) >= 60
    assert sum(1 for d in descs if _is_dense(d)) >= 60
    assert sum(1 for d in descs
               if d.field_enc == ENC_DELTA and not _is_dense(d)) >= 60
    b.gen_bulk_i64(1000, N_BULK, 40, T0, MS, 1000, 1, 0xB4DB,
                   group_mod=2, threads=4)
    assert b.n_blocks == n_hand + N_BULK > LAUNCH_WAVES + n_hand
    assert all(_is_dense(d) for d in b.blocks()[n_hand:])
    want = [_pairs(oracle_scan(b, VT_INT64, n_groups=2, **kw))
            for kw in ({}, BULK_CLAMP)]
    return b, want


def _accum(rng, n, span):
    """Offsets of a non-monotone walk that starts at 0, steps up to span."""
    out, v = [0], 0
    for i in range(n - 1):
        v += rng.randint(-span, span) if i >= 2 else (span, -span)[i]
        out.append(v)
    return out


@gpu
@pytest.mark.parametrize("policy", POLICIES)
def test_mixed_encodings_then_dense(policy):
    b, want = _mixed()
    assert all(c > 0 for c, _ in want[0])
    got = _scan(b, 2, policy, ({}, BULK_CLAMP))
    assert got == want
