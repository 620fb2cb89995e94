"""Host side of the nibble-packed dense field streams: the slot planner
(bydb_field_pack_plan) over hand-made descriptor lists, and the Python
restatement of the build's eligibility rule that the GPU tests count
packed blocks with.  No GPU."""
import random

from banyandb_amd import BlockDesc, PartBuilder, VT_INT64, field_pack_plan, lib
import field_pack_ref as ref
from field_pack_ref import (ENC_CONST, ENC_DELTA_CONST, ENC_DELTA, ENC_PLAIN,
                            ENCODINGS, SIDECAR_BIT, SLOT, RawPart)
from helpers import oracle_scan


def _desc(enc, count, field_len=None, field_off=4096):
    d = BlockDesc()
    d.field_enc = enc
    d.count = count
    d.field_len = count - 1 if field_len is None else field_len
    d.field_off = field_off
    return d


def _check(descs):
    """The planner's promises over one descriptor list; returns the lens."""
    offs, lens, arena = field_pack_plan(descs)
    assert len(offs) == len(lens) == len(descs)
    spans = []
    for d, off, ln in zip(descs, offs, lens):
        if not ref.candidate(d):
            assert (off, ln) == (0, 0), (d.field_enc, d.count)
            continue
        assert ln == ref.slot_bytes(d.count)
        assert ln > 0 and ln % SLOT == 0 and off % SLOT == 0
        assert 2 * ln >= d.count - 1            # one nibble per delta
        assert ln - SLOT < (d.count - 1 + 1) // 2 <= ln   # and no line spare
        spans.append((off, off + ln))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))   # disjoint
    assert arena == sum(lens)
    if spans:
        assert spans[0][0] == 0 and spans[-1][1] == arena
    return lens


def test_counts_of_one_and_two_and_odd_and_even_delta_counts():
    counts = [1, 2, 3, 4, 5, 256, 257, 258, 8190, 8191, 8192]
    lens = _check([_desc(ENC_DELTA, c) for c in counts])
    assert lens[0] == 0                          # one row: no delta at all
    assert lens[1:] == [128, 128, 128, 128, 128, 128, 256, 4096, 4096, 4096]
    # 255 and 256 nibbles fill one line exactly, 257 need a second
    assert ref.slot_bytes(256) == ref.slot_bytes(257) == 128
    assert ref.slot_bytes(258) == 256
    assert ref.slot_bytes(8192) == 4096          # four 1-KiB chunks


def test_every_encoding_and_sidecar_fields():
    descs = []
    for enc in ENCODINGS:
        for count in (1, 2, 7, 8192):
            descs.append(_desc(enc, count))
    lens = _check(descs)
    for d, ln in zip(descs, lens):
        assert (ln > 0) == (d.field_enc == ENC_DELTA and d.count >= 2)
    # a Delta stream that lives in the sidecar, multi-byte Delta streams,
    # a stream shorter than its count, and a count beyond a block's maximum
    odd = [_desc(ENC_DELTA, 100, field_off=SIDECAR_BIT | 64),
           _desc(ENC_DELTA, 100, field_len=100),
           _desc(ENC_DELTA, 100, field_len=98),
           _desc(ENC_DELTA, 8193),
           _desc(ENC_PLAIN, 100, field_off=SIDECAR_BIT | 128),
           _desc(ENC_DELTA, 100)]
    assert _check(odd) == [0, 0, 0, 0, 0, 128]


def test_random_descriptor_lists():
    rng = random.Random(0x9ACC)
    for _ in range(50):
        descs = []
        for _ in range(rng.randint(0, 60)):
            count = rng.choice([1, 2, 3, 255, 256, 257, 258, 4097, 8192,
                                rng.randint(1, 8192)])
            enc = rng.choice([ENC_DELTA] * 3 + ENCODINGS)
            flen = rng.choice([None, None, None, count, count + 5])
            off = rng.choice([4096, 4096, SIDECAR_BIT | 4096])
            descs.append(_desc(enc, count, flen, off))
        _check(descs)


def test_empty_list_and_bad_arguments():
    assert field_pack_plan([]) == ([], [], 0)
    assert lib().bydb_field_pack_plan(None, 1, None, None, None) < 0


def test_eligibility_rule_on_encoded_blocks():
    """packs() against blocks as the encoder writes them: deltas -8..7 are
    the zigzag bytes 0..15; -9 and +8 are 17 and 16."""
    assert [ref.zigzag(d) for d in (0, -1, 1, -8, 7, -9, 8, -64, 63)] == \
        [0, 1, 2, 15, 14, 17, 16, 127, 126]
    p = RawPart()
    kinds = {
        "low": [-8] * 9, "high": [7] * 9, "alt": [-8, 7] * 5,
        "over": [7, 8, 7], "under": [-8, -9, -8], "one": [3],
    }
    for i, deltas in enumerate(kinds.values()):
        p.add_delta(i + 1, 1000, deltas)
    got = [ref.packs(p.payload, d) for d in p.blocks()]
    assert got == [True, True, True, False, False, True]
    assert ref.census(p) == (6, 4, 5 + 5 + 5 + 1)   # ceil(deltas / 2) each
    # the encoder's own output: a small-step walk packs, a wide one does
    # not, other encodings are no candidates
    b = PartBuilder()
    rng = random.Random(7)
    n = 300
    ts = [ref.T0 + i * ref.MS for i in range(n)]
    small = [10 ** 6]
    wide = [10 ** 6]
    for i in range(n - 1):
        small.append(small[-1] + ((1, -2)[i] if i < 2 else rng.randint(-8, 7)))
        wide.append(wide[-1] + ((1, -2)[i] if i < 2 else rng.randint(-64, 63)))
    b.add_block_i64(1, ts, [1] * n, small)
    b.add_block_i64(2, ts, [1] * n, wide)
    b.add_block_i64(3, ts, [1] * n, [5] * n)
    b.add_block_i64(4, ts, [1] * n, [5 + 3 * i for i in range(n)])
    descs = b.blocks()
    assert [d.field_enc for d in descs] == [ENC_DELTA, ENC_DELTA, ENC_CONST,
                                            ENC_DELTA_CONST]
    assert [ref.candidate(d) for d in descs] == [True, True, False, False]
    assert [ref.packs(b.payload, d) for d in descs] == [True, False, False,
                                                        False]
    assert max(b.payload[descs[1].field_off:][:n - 1]) > 15


def test_raw_part_reads_back_through_the_oracle():
    """RawPart's hand-written Delta blocks decode to the values they were
    made from, at both int64 extremes."""
    top, bot = ref.I64 - 1, -ref.I64
    p = RawPart()
    cases = [(top, [7] * 33), (bot, [-8] * 34), (top - 3, [-8, 7] * 40),
             (5, [1])]
    for g, (first, deltas) in enumerate(cases):
        p.add_delta(g + 1, first, deltas, group_code=g)
    res = oracle_scan(p, VT_INT64, n_groups=len(cases))
    for (first, deltas), r in zip(cases, res):
        vals = ref.block_values(first, deltas)
        assert r.count == len(vals)
        assert r.sum_i == ref.wrap(sum(vals))
