"""Part builders shared by the CPU and GPU tests of the tag projection
(bydb_rows_fetch_tags).  The expected side is the Python lists a part was
built from: the part builder keeps row order for strictly ascending
timestamps (DBlk asserts them), so the value of seq is
blocks[seq >> 13].tags[slot][seq & 8191], or nil when the block has fewer
columns than slot + 1.

Every builder asserts the shape of its own fixture where the payload shows
it — the first byte of a block's tag stream is BYDB_ENC_DICTIONARY or
BYDB_ENC_PLAIN — so a case cannot silently test the wrong path."""
import ctypes as C
import random

from banyandb_amd import BlockDesc
import filter_cases as fc
import row_dedup_cases as rdc
from row_dedup_cases import DBlk

ENC_PLAIN, ENC_DICTIONARY = 9, 10
DICT, PLAIN, ABSENT = "dict", "plain", "absent"
T0, MS = fc.T0, fc.MS
ROW_BITS = 13
LONG_VALUE = b"L" * 300     # two-byte stored length; five 64-byte copy steps


def seq_of(block, row):
    return (block << ROW_BITS) | row


def expect(blocks, seqs, slot):
    """The fixture's value (bytes or None) of every requested row."""
    out = []
    for s in seqs:
        b = blocks[s >> ROW_BITS]
        out.append(b.tags[slot][s & 8191] if slot < len(b.tags) else None)
    return out


def slot_streams(desc):
    return [(desc.tag_off, desc.tag_len), (desc.tag2_off, desc.tag2_len),
            (desc.tag3_off, desc.tag3_len)]


def stream_kind(payload, desc, slot):
    off, ln = slot_streams(desc)[slot]
    if ln == 0:
        return ABSENT
    return {ENC_DICTIONARY: DICT, ENC_PLAIN: PLAIN}[payload[off]]


def build(blocks, kinds):
    """PartBuilder of `blocks`; kinds[i] lists the stream kind each slot of
    block i must have come out as."""
    pb = rdc.builder(blocks)
    payload = pb.payload
    descs = pb.blocks()
    assert len(descs) == len(blocks) == len(kinds)
    for i, (d, b, want) in enumerate(zip(descs, blocks, kinds)):
        assert d.count == len(b.ts), i
        got = [stream_kind(payload, d, sl) for sl in range(3)]
        assert got == list(want) + [ABSENT] * (3 - len(want)), (i, got, want)
    return pb


def run_bounds(col):
    """[start, end) of every run of equal values."""
    out, start = [], 0
    for i in range(1, len(col) + 1):
        if i == len(col) or col[i] != col[start]:
            out.append((start, i))
            start = i
    return out


def blk(sid, n, tags, rng):
    return DBlk(sid, fc.ts_of(n), [1] * n, rdc.ivals(rng, n), tags)


# ---- dictionary blocks ----
def entity_blocks(rng):
    """Single-run columns (entity tags), and two two-run blocks whose
    first-seen order differs: b"aa" is code 0 in one, code 1 in the other."""
    return [
        blk(1, 500, [[b"prod"] * 500, [b"zone-a"] * 500], rng),
        blk(2, 500, [[b"dev"] * 500], rng),
        blk(3, 200, [[b"aa"] * 100 + [b"bbb"] * 100], rng),
        blk(4, 200, [[b"bbb"] * 100 + [b"aa"] * 100], rng),
    ], [(DICT, DICT), (DICT,), (DICT,), (DICT,)]


def rowvary_block(rng, sid=5, n=3000):
    """> 128 runs with nil runs; an int-cell dictionary beside it."""
    col = fc.runs(rng, n, fc.ENVS, maxrun=12, nil_p=0.15)
    assert len(run_bounds(col)) > 128
    cells = fc.runs(rng, n, [fc.icell(c) for c in fc.CODES], maxrun=60)
    return blk(sid, n, [col, cells], rng), (DICT, DICT)


def alternating_block(rng, sid=6):
    """8192 rows, 8192 runs: the most a block can hold."""
    col = [b"x" if i % 2 == 0 else b"yy" for i in range(8192)]
    return blk(sid, 8192, [col], rng), (DICT,)


def svc_block(rng, sid=7, n=1500):
    """256 values, first-seen order == SVCS order, so code == index.  The
    sections are past 128 bytes: zstd'd in the part, host-normalised."""
    col = list(fc.SVCS) + fc.runs(rng, n - 256, fc.SVCS, maxrun=6)
    return blk(sid, n, [col], rng), (DICT,)


def empty_nil_block(rng, sid=8):
    col = ([b""] * 7 + [None] * 5 + [b"v"] * 3) * 20
    return blk(sid, len(col), [col], rng), (DICT,)


# ---- plain blocks ----
def plain_block(rng, sid, n, long_at=None):
    col = fc.plain_col(rng, n)
    if long_at is not None:
        col[long_at] = LONG_VALUE
    assert len(set(col)) > 256
    assert None in col and b"" in col
    return blk(sid, n, [col], rng), (PLAIN,)


def mixed_part():
    """Every block kind in one part: (blocks, kinds, index-by-name)."""
    rng = random.Random(7100)
    blocks, kinds = entity_blocks(rng)
    names = {"entity_a": 0, "entity_b": 1, "order_ab": 2, "order_ba": 3}
    for name, (b, k) in (
            ("rowvary", rowvary_block(rng)),
            ("alternating", alternating_block(rng)),
            ("svc", svc_block(rng)),
            ("empty_nil", empty_nil_block(rng)),
            ("plain321", plain_block(rng, 9, 321)),
            ("plain3000", plain_block(rng, 10, 3000, long_at=1234)),
            ("no_tags", (blk(11, 100, [], rng), ()))):
        names[name] = len(blocks)
        blocks.append(b)
        kinds.append(k)
    return blocks, kinds, names


def first_section_marker(payload, off):
    """compress_block marker of a dictionary's lengths section: 0 plain
    (< 128 bytes, parsed in the payload), 1 zstd (host-normalised)."""
    p = off + 1
    while payload[p] >= 0x80:
        p += 1
    return payload[p + 1]


def mixed_built():
    """(PartBuilder, blocks, names) of mixed_part, both framings present."""
    blocks, kinds, names = mixed_part()
    pb = build(blocks, kinds)
    payload, descs = pb.payload, pb.blocks()
    assert first_section_marker(payload, descs[names["svc"]].tag_off) == 1
    assert first_section_marker(payload, descs[names["rowvary"]].tag_off) == 0
    return pb, blocks, names


def three_slot_blocks():
    """filter_cases.three_slot_case's data (dictionary, plain, int
    dictionary) as DBlk, with its conditions."""
    scen = fc.three_slot_case()
    blocks = [DBlk(b.sid, b.ts, [1] * len(b.ts), b.vals, b.tags)
              for b in scen.blocks]
    return blocks, [(DICT, PLAIN, DICT)] * len(blocks), scen.conds


# ---- corrupt streams ----
class PatchedPart:
    """A part whose payload bytes were patched after the build, in the shape
    Session.upload_part reads (as row_dedup_cases.RawPart)."""

    def __init__(self, pb, patches):
        payload = bytearray(pb.payload)
        for off, data in patches:
            payload[off:off + len(data)] = data
        descs = pb.blocks()
        out = (BlockDesc * len(descs))()
        for i, d in enumerate(descs):
            C.memmove(C.addressof(out[i]), C.addressof(d), C.sizeof(BlockDesc))
        self._buf = (C.c_uint8 * len(payload)).from_buffer(payload)
        self._descs = out
        self.payload_len = len(payload)
        self.n_blocks = len(descs)

    def raw_payload_ptr(self):
        return C.cast(self._buf, C.POINTER(C.c_uint8))

    def blocks_ptr(self):
        return self._descs

    def blocks(self):
        return list(self._descs)


def dict_entry_header(payload, off, ln):
    """Byte offset of the 32-bit big-endian entry count of a payload-framed
    dictionary stream: [10][varuint count][0][u8 len][lengths][0][u8 len]
    [values][u32 entries][u8 width][entries]."""
    assert payload[off] == ENC_DICTIONARY
    p = off + 1
    while payload[p] >= 0x80:
        p += 1
    p += 1
    for _ in range(2):                       # lengths section, values section
        assert payload[p] == 0, "section is not plain-framed"
        p += 2 + payload[p + 1]
    assert p + 5 <= off + ln
    return p


def corrupt_blocks():
    """Two copies of a three-run block and one healthy block.  Block 0 gets
    its entry count cut to one run (the counts end at row 10 of 30); block 1
    gets an entry count whose entries would extend far past tag_len."""
    rng = random.Random(7200)
    col = [b"a"] * 10 + [b"bb"] * 10 + [b"a"] * 10
    blocks = [blk(1, 30, [list(col)], rng), blk(2, 30, [list(col)], rng),
              blk(3, 30, [list(col)], rng)]
    pb = build(blocks, [(DICT,)] * 3)
    payload = pb.payload
    descs = pb.blocks()
    patches = []
    for i, count in ((0, 2), (1, 0x00FFFFFF)):
        at = dict_entry_header(payload, descs[i].tag_off, descs[i].tag_len)
        assert int.from_bytes(payload[at:at + 4], "big") == 6   # 3 runs
        patches.append((at, count.to_bytes(4, "big")))
    return blocks, PatchedPart(pb, patches)
