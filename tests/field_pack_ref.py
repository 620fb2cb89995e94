"""Reference rules and part-building support for the nibble-packed dense
field streams (bydb_set_field_pack), shared by test_field_pack_cpu.py and
test_gpu_field_pack.py.

- candidate() / packs(): which blocks get a slot and which slots the build
  fills (every zigzag byte of the stream <= 15), restated from
  include/bydb_gpu.h;
- RawPart: a part whose Delta blocks are written byte by byte, so that
  streams the encoder would never choose (all deltas equal, one delta) can
  be scanned; it quacks like a PartBuilder for Session.upload_part and
  helpers.oracle_scan."""
import ctypes as C
import functools

from banyandb_amd import BlockDesc, PartBuilder

ENC_CONST, ENC_DELTA_CONST, ENC_DELTA, ENC_DOD, ENC_PLAIN = 1, 2, 3, 4, 9
ENCODINGS = list(range(0, 11))
SIDECAR_BIT = 1 << 63
SLOT = 128
MAX_ROWS = 8192
T0 = 1_700_000_000_000_000_000
MS = 10 ** 6
I64 = 1 << 63


def wrap(v):
    return (v + I64) % (1 << 64) - I64


def candidate(d):
    return (d.field_enc == ENC_DELTA and 2 <= d.count <= MAX_ROWS
            and d.field_len == d.count - 1
            and not d.field_off & SIDECAR_BIT)


def slot_bytes(count):
    """ceil((count-1)/2) bytes, rounded up to the 128-byte line."""
    return -(-(count // 2) // SLOT) * SLOT   # ceil((count-1)/2) == count//2


def packs(payload, d):
    """The build's eligibility rule: a candidate whose zigzag bytes are all
    <= 15, that is whose deltas all lie in [-8, 7]."""
    return candidate(d) and max(
        payload[d.field_off:d.field_off + d.field_len]) <= 15


def census(part):
    """(candidate blocks, blocks the build packs, packed payload bytes)."""
    payload, descs = part.payload, part.blocks()
    cand = [d for d in descs if candidate(d)]
    hit = [d for d in cand if packs(payload, d)]
    return len(cand), len(hit), sum(d.count // 2 for d in hit)


def zigzag(d):
    assert -64 <= d <= 63, d
    return (d << 1) ^ (d >> 63)


@functools.lru_cache(maxsize=None)
def _template(n, row0):
    """Everything of an n-row block but its field stream: the bytes in front
    of it (timestamps from row0 on, const versions) and the descriptor."""
    b = PartBuilder()
    ts = [T0 + (row0 + i) * MS for i in range(n)]
    b.add_block_i64(1, ts, [1] * n, [0] * n)
    d = b.blocks()[0]
    assert d.field_enc == ENC_CONST and d.field_len == 0
    assert d.ts_off == 0 and d.field_off == b.payload_len
    raw = bytes(C.string_at(C.addressof(d), C.sizeof(BlockDesc)))
    return b.payload, raw


class RawPart:
    def __init__(self, base=0):
        """base: payload bytes already resident in front of this part (a
        descriptor's offsets are absolute within the whole resident part)."""
        self._base = base
        self._payload = bytearray()
        self._descs = []

    def add_delta(self, sid, first, deltas, group_code=0, row0=0):
        """A Delta block: values first, first + deltas[0], ... (mod 2^64),
        one zigzag byte per delta."""
        n = len(deltas) + 1
        head, raw = _template(n, row0)
        d = BlockDesc.from_buffer_copy(raw)
        base = self._base + len(self._payload)
        self._payload += head
        d.series_id = sid
        d.ts_off += base
        d.field_enc = ENC_DELTA
        d.field_first = first
        d.field_off = self._base + len(self._payload)
        d.field_len = n - 1
        d.group_code = group_code
        self._payload += bytes(zigzag(x) for x in deltas)
        self._descs.append(d)
        return d

    def add_builder(self, b, sid0=0):
        """Every block of a PartBuilder whose blocks carry no tag column,
        series ids raised by sid0."""
        base = self._base + len(self._payload)
        self._payload += b.payload
        for src in b.blocks():
            assert src.tag_len == src.tag2_len == src.tag3_len == 0
            d = BlockDesc.from_buffer_copy(
                bytes(C.string_at(C.addressof(src), C.sizeof(BlockDesc))))
            d.series_id += sid0
            d.ts_off += base
            d.field_off += base
            self._descs.append(d)

    def extend(self, other):
        """The blocks of a RawPart that was built with base = this part's
        end."""
        assert other._base == self._base + len(self._payload)
        self._payload += other._payload
        self._descs += other._descs

    # ---- the PartBuilder surface the session and the oracle bridge use ----
    @property
    def payload(self):
        return bytes(self._payload)

    @property
    def payload_len(self):
        return len(self._payload)

    @property
    def n_blocks(self):
        return len(self._descs)

    def blocks(self):
        return list(self._descs)

    def raw_payload_ptr(self):
        return (C.c_uint8 * max(len(self._payload), 1)).from_buffer_copy(
            bytes(self._payload) or b"\0")

    def blocks_ptr(self):
        return (BlockDesc * max(len(self._descs), 1))(*self._descs)


def block_values(first, deltas):
    out, v = [first], first
    for x in deltas:
        v = wrap(v + x)
        out.append(v)
    return out
