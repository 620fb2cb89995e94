"""Dense all-1-byte delta fold read as 16-byte lanes in 1-KiB chunks:
every stream alignment and length class, clamps around chunk and lane
boundaries, and the per-wave group flush.  Sums and counts are exact
against the oracle."""
import functools
import random

import pytest

from banyandb_amd import PartBuilder, Session, VT_INT64, AGG_SUM, AGG_COUNT
from helpers import oracle_scan

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000_000_000_000
MS = 10 ** 6
ENC_DELTA = 3

# stream lengths (= rows - 1): around the lane (16 B), the dword loop of
# old (4 B), the chunk (1 KiB) and the full block, where a ninth chunk
# appears once head offset + length passes 8 KiB
LENGTHS = ([1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257,
            1007, 1008, 1009, 1023, 1024, 1025, 4095, 4096, 4097] +
           list(range(8170, 8192)))
# the encoder picks delta-of-delta for about two thirds of these walks;
# six repetitions leave 42 long dense blocks on all 16 alignments
REPS = 6


def _walk(rng, n):
    v = rng.randint(-10 ** 9, 10 ** 9)
    out = []
    for _ in range(n):
        v += rng.randint(-3, 3)     # zigzag delta < 64: one byte
        out.append(v)
    return out


def _add_filler(b, rng, sid):
    """A block of varying encoded size, so the next field_off moves."""
    k = rng.randint(1, 24)
    ts = [T0 + i * MS for i in range(k)]
    b.add_block_i64(sid, ts, [1] * k,
                    [rng.randint(-2 ** 40, 2 ** 40) for _ in range(k)])


def _is_dense(d):
    return d.field_enc == ENC_DELTA and d.field_len == d.count - 1


@functools.lru_cache(maxsize=None)
def _sweep_cases():
    """(filler seed, ts, vals) per swept block, the same for every test."""
    rng = random.Random(0xD15E)
    cases = []
    for _ in range(REPS):
        for ln in LENGTHS:
            n = ln + 1
            cases.append((rng.randrange(1 << 30),
                          tuple(T0 + i * MS for i in range(n)),
                          tuple(_walk(rng, n))))
    return cases


def _add_case(b, case, sid):
    fseed, ts, vals = case
    _add_filler(b, random.Random(fseed), sid)
    b.add_block_i64(sid + 1, list(ts), [1] * len(ts), list(vals))


@functools.lru_cache(maxsize=None)
def _sweep_part():
    """One part with every swept block; a short dense block (length <= 5)
    last, so the over-read past the part's last stream starts near its
    end."""
    cases = _sweep_cases()
    probe = PartBuilder()
    for i, case in enumerate(cases):
        _add_case(probe, case, 2 * i + 1)
    descs = probe.blocks()
    short = [i for i in range(len(cases))
             if _is_dense(descs[2 * i + 1]) and len(cases[i][1]) - 1 <= 5]
    assert short, "no short dense block among the swept cases"
    order = [i for i in range(len(cases)) if i != short[-1]] + [short[-1]]
    b = PartBuilder()
    for k, i in enumerate(order):
        _add_case(b, cases[i], 2 * k + 1)
    return b


def _scan_exact(b, **clamp):
    orc = oracle_scan(b, VT_INT64, **clamp)[0]
    s = Session(0)
    s.upload_part(b)
    s.configure(VT_INT64, [AGG_SUM, AGG_COUNT])
    s.consume(**clamp)
    g = s.finalize()[0]
    s.close()
    return (g.count, g.sum_i), (orc.count, orc.sum_i)


def test_sweep_selects_every_alignment():
    """The selection the sweep relies on, asserted on the descriptors
    before any GPU work."""
    b = _sweep_part()
    descs = b.blocks()
    assert descs[-1].field_len <= 5 and _is_dense(descs[-1])
    dense = [d for d in descs if _is_dense(d)]
    # condition 1: dense Delta blocks cover all 16 stream alignments
    assert {d.field_off % 16 for d in dense} == set(range(16))
    # condition 2: so do the long ones, and one needs the ninth chunk
    long_ = [d for d in dense if d.field_len >= 8178]
    assert {d.field_off % 16 for d in long_} == set(range(16))
    assert any(d.field_off % 16 + d.field_len > 8192 for d in long_)


def test_alignment_length_sweep_whole_part():
    test_sweep_selects_every_alignment()
    got, want = _scan_exact(_sweep_part())
    assert got == want


def test_alignment_length_sweep_each_block_last():
    """Each dense block as the last stream of a part of its own, behind
    the same filler (so at a moving alignment)."""
    test_sweep_selects_every_alignment()
    n_dense = 0
    for i, case in enumerate(_sweep_cases()):
        b = PartBuilder()
        _add_case(b, case, 1)
        d = b.blocks()[-1]
        if not _is_dense(d):
            continue
        n_dense += 1
        assert d.field_off + d.field_len == b.payload_len
        got, want = _scan_exact(b)
        assert got == want, (i, d.field_off % 16, d.field_len)
    assert n_dense >= 16


@functools.lru_cache(maxsize=None)
def _clamp_part():
    """Full-length blocks on one time axis; two dense ones at different
    alignments are required."""
    rng = random.Random(0xC1A3)
    n = 8192
    ts = [T0 + i * MS for i in range(n)]
    b = PartBuilder()
    for k in range(8):
        _add_filler(b, rng, 2 * k + 1)
        b.add_block_i64(2 * k + 2, ts, [1] * n, _walk(rng, n))
    return b


def _clamp_rows(aligns):
    """(r0, r1) row pairs.  Delta byte j-1 of a stream at field_off % 16
    == a sits at in-memory offset a + j - 1 from the 16-byte boundary the
    fold starts from, so for each alignment in `aligns` (and for 0, the
    stream-relative view) the rows land -1, 0, +1 around the 16-byte lane
    and 1-KiB chunk boundaries as the kernel sees them."""
    n = 8192
    last = n - 1                       # last row; its delta is byte last-1
    r0s, r1s = set(), set()
    for a in sorted({0} | set(aligns)):
        for m in (16, 32, 1024, 2048, 4096, 7168, 8176, 8192):
            for k in (-1, 0, 1):
                r = m - a + k
                if 0 <= r <= last:
                    r0s.add(r)
                    r1s.add(r)
    r0s |= {0, 1, 2, last - 1, last}
    r1s |= {0, 1, last - 2, last - 1, last}
    pairs = [(r0, last) for r0 in sorted(r0s)]
    pairs += [(0, r1) for r1 in sorted(r1s)]
    # both ends inside, in one chunk and chunks apart
    pairs += [(15, 17), (16, 16), (1023, 1025), (1024, 1024), (17, 8175),
              (1025, 7167), (4097, 4097), (last, last)]
    return pairs


def test_clamp_sweep_two_alignments():
    b = _clamp_part()
    dense = [d for d in b.blocks() if _is_dense(d) and d.count == 8192]
    aligns = sorted({d.field_off % 16 for d in dense})
    # two different in-memory alignments, at least one off the boundary
    assert len(aligns) >= 2 and aligns[-1] != 0
    s = Session(0)
    s.upload_part(b)
    s.configure(VT_INT64, [AGG_SUM, AGG_COUNT])
    for r0, r1 in _clamp_rows(aligns):
        clamp = dict(min_ts=T0 + r0 * MS, max_ts=T0 + r1 * MS)
        orc = oracle_scan(b, VT_INT64, **clamp)[0]
        s.reset()
        s.consume(**clamp)
        g = s.finalize()[0]
        assert (g.count, g.sum_i) == (orc.count, orc.sum_i), (r0, r1)
    s.close()


def test_group_flush_dense_blocks():
    """Per-block group codes cycling over 4 groups: each wave flushes its
    register partial on every group change."""
    rng = random.Random(0x6F1A)
    n_groups = 4
    b = PartBuilder()
    for k in range(176):
        n = (257, 1030, 2500, 8192)[k % 4] if k % 11 else 5
        ts = [T0 + i * MS for i in range(n)]
        b.add_block_i64(k + 1, ts, [1] * n, _walk(rng, n),
                        group_code=(k * 7 + k // 5) % n_groups)
    assert sum(1 for d in b.blocks() if _is_dense(d)) >= 64
    orc = oracle_scan(b, VT_INT64, n_groups=n_groups)
    s = Session(0)
    s.upload_part(b)
    s.configure(VT_INT64, [AGG_SUM, AGG_COUNT], n_groups=n_groups)
    s.consume()
    gs = s.finalize()
    s.close()
    assert len(gs) == n_groups
    for g, w in zip(gs, orc):
        assert w.count > 0
        assert (g.count, g.sum_i) == (w.count, w.sum_i)
