"""Inputs shared by the CPU and GPU clamp / value-extreme tests: irregular
timestamp axes whose delta-of-delta streams reach every branch of the
stream row clamp, and one-byte delta columns that saturate the byte
lanes of the dense fold.  Everything is seeded here; every part keeps the
rows it was built from, so a per-row reference needs no decoder."""
import functools
import random

from banyandb_amd import PartBuilder
from test_gpu_dense_wide import LENGTHS
from test_gpu_fuzz import TAGS, random_tags

T0 = 1_700_000_000_000_000_000
MS = 10 ** 6
INT64_MIN = -(2 ** 63)
INT64_MAX = 2 ** 63 - 1
M64 = (1 << 64) - 1

ENC_DELTA = 3
ENC_DOD_WV = 8


def wrap64(v):
    """Python int -> the int64 it wraps to."""
    v &= M64
    return v - (1 << 64) if v >> 63 else v


# ---------------------------------------------------------------------
# timestamp shapes
# ---------------------------------------------------------------------
SIZES = (2, 3, 4, 63, 64, 65, 66, 127, 128, 129, 130, 1000, 8192)
W10 = 4_620_000_000_000_000_000          # zigzag(d2) needs 64 bits
TS_STEPS = {
    "one_byte": (0x7501, [1, 2, 3, 5, 20, 31]),
    "two_byte": (0x7502, [100, 900, 3000]),
    "mixed": (0x7503, [1, 1, 1, 10 ** 3, 10 ** 6, 10 ** 9, 10 ** 12]),
    "wide": (0x7504, [10 ** 15, 3 * 10 ** 15]),
}
TS_SHAPES = ("one_byte", "two_byte", "mixed", "wide", "ten_byte")
FIELD_KINDS = ("const", "delta_const", "dense", "multi_byte", "dod")
FIELD_SEED = 0xF1E1D
PAIR_SEED = 0x9A125
OFFSETS = ((0, 0), (-1, 1), (1, -1), (-1, 0))
BOUNDARY_ROWS = (0, 1, 2, 62, 63, 64, 65, 126, 127, 128, 129)


def shape_sizes(shape):
    if shape == "ten_byte":
        return (8,)
    if shape == "wide":
        return tuple(n for n in SIZES if n <= 1000)
    return SIZES


@functools.lru_cache(maxsize=None)
def ts_axis(shape):
    """The shape's one timestamp axis; a block of n rows uses its first n."""
    if shape == "ten_byte":
        ts = [-9_200_000_000_000_000_000]
        for step in (1, W10, 1, W10, 1, W10, 1):
            ts.append(ts[-1] + step)
    else:
        seed, steps = TS_STEPS[shape]
        rng = random.Random(seed)
        ts = [T0]
        for _ in range(max(shape_sizes(shape)) - 1):
            ts.append(ts[-1] + rng.choice(steps))
    assert INT64_MIN <= ts[0] and ts[-1] <= INT64_MAX
    return tuple(ts)


def dense_walk(rng, n, first, lo=-64, hi=63):
    v, out = first, [first]
    for _ in range(n - 1):
        v = wrap64(v + rng.randint(lo, hi))
        out.append(v)
    return out


def field_values(rng, kind, n):
    if kind == "const":
        return [rng.randint(-10 ** 9, 10 ** 9)] * n
    if kind == "delta_const":
        a, d = rng.randint(-10 ** 9, 10 ** 9), rng.randint(-10 ** 4, 10 ** 4)
        return [a + i * d for i in range(n)]
    if kind == "dense":         # one-byte zigzag deltas over their full span
        return dense_walk(rng, n, rng.randint(0, 10 ** 9))
    if kind == "multi_byte":
        # a negative first value would make the encoder pick DeltaOfDelta
        return [rng.randint(0, 2 ** 61)] + \
            [rng.randint(-2 ** 61, 2 ** 61) for _ in range(n - 1)]
    assert kind == "dod"
    v, out = rng.randint(0, 10 ** 9), []
    for _ in range(n):
        v += rng.randint(0, 50)
        out.append(v)
    return out


def to_cents(v):
    """Bound a mantissa so that f64_sum_close's magnitude rule holds."""
    return v % 10 ** 12 - 5 * 10 ** 11


class Blk:
    """One block: its rows (vals are floats in a float part), the field
    kind it was generated as, an optional per-row tag column."""

    def __init__(self, ts, vals, kind, tags=None):
        self.ts, self.vals, self.kind, self.tags = ts, vals, kind, tags
        self.n = len(ts)


class Part:
    """Blocks with group_code == block index (n_groups == len(blocks)), so
    a scan returns one partial per block."""

    def __init__(self, name, blocks, float_vals=False):
        self.name, self.blocks, self.float_vals = name, blocks, float_vals
        self._pb = None

    @property
    def n_groups(self):
        return len(self.blocks)

    def builder(self):
        if self._pb is not None:
            return self._pb
        pb = self._pb = PartBuilder()
        add = pb.add_block_f64 if self.float_vals else pb.add_block_i64
        for i, b in enumerate(self.blocks):
            add(i + 1, list(b.ts), [1] * b.n, list(b.vals), group_code=i)
            if b.tags is not None:
                pb.set_block_tag(b.tags)
        return pb

    def float_exp(self):
        return min(d.exp for d in self.builder().blocks()) \
            if self.float_vals else 0


@functools.lru_cache(maxsize=None)
def ts_part(shape, float_vals=False):
    """Every (size, field kind) of the shape as one block each."""
    axis = ts_axis(shape)
    rng = random.Random(FIELD_SEED + TS_SHAPES.index(shape))
    blocks = []
    for n in shape_sizes(shape):
        ts = axis[:n]           # one tuple per size, shared by its blocks
        for kind in FIELD_KINDS:
            vals = field_values(rng, kind, n)
            if float_vals:
                vals = [to_cents(v) / 100.0 for v in vals]
            blocks.append(Blk(ts, vals, kind))
    return Part(shape + ("_f64" if float_vals else ""), blocks, float_vals)


def boundary_rows(shape):
    rows = set()
    for n in shape_sizes(shape):
        for r in BOUNDARY_ROWS + (n // 2, n - 3, n - 2, n - 1):
            if 0 <= r < n:
                rows.add(r)
    return sorted(rows)


@functools.lru_cache(maxsize=None)
def clamp_pairs(shape):
    """(r0, r1) rows of the axis the clamp bounds are taken from."""
    last = len(ts_axis(shape)) - 1
    rows = boundary_rows(shape)
    pairs = [(r, last) for r in rows]
    pairs += [(0, r) for r in rows]
    pairs += [(r, r) for r in rows]
    pairs += [(r, min(r + 1, last)) for r in rows]
    rng = random.Random(PAIR_SEED + TS_SHAPES.index(shape))
    for _ in range(50):
        a, b = rng.randint(0, last), rng.randint(0, last)
        pairs.append((min(a, b), max(a, b)))
    return tuple(dict.fromkeys(pairs))      # ordered, no duplicates


@functools.lru_cache(maxsize=None)
def clamps(shape):
    """((r0, r1, dl, dh, min_ts, max_ts), ...) and the number of bounds
    dropped for leaving int64 (the only omission there is)."""
    axis = ts_axis(shape)
    out, dropped = [], 0
    for r0, r1 in clamp_pairs(shape):
        for dl, dh in OFFSETS:
            lo, hi = axis[r0] + dl, axis[r1] + dh
            if lo < INT64_MIN or hi > INT64_MAX or lo > INT64_MAX \
                    or hi < INT64_MIN:
                dropped += 1
                continue
            out.append((r0, r1, dl, dh, lo, hi))
    return tuple(out), dropped


def varint_lengths(stream):
    """Byte length of each varint in an encoded stream."""
    out, run = [], 0
    for b in stream:
        run += 1
        if b < 0x80:
            out.append(run)
            run = 0
    return out


# ---------------------------------------------------------------------
# a per-row tag on the mixed axis: group-by and predicate under a clamp
# ---------------------------------------------------------------------
TAG_SEED = 0x7A65


@functools.lru_cache(maxsize=None)
def tag_part():
    axis = ts_axis("mixed")
    n = len(axis)
    rng = random.Random(TAG_SEED)
    cols = [extreme_values(k) for k in (1, 2, 5, 6)]
    cols += [field_values(rng, "multi_byte", n) for _ in range(2)]
    kinds = ["extreme%d" % k for k in (1, 2, 5, 6)] + ["multi_byte"] * 2
    return Part("mixed_tagged",
                [Blk(axis, vals, kind, random_tags(rng, n, 2))
                 for vals, kind in zip(cols, kinds)])


def tag_clamps(k=40):
    """About k clamps spread evenly over the mixed shape's list."""
    cl = clamps("mixed")[0]
    return cl[::max(1, len(cl) // k)]


# ---------------------------------------------------------------------
# extreme dense value shapes (regular 1 ms timestamps)
# ---------------------------------------------------------------------
N_EXT = 8192
EXT_SEED = 0xE87
EXT_SHAPES = (1, 2, 3, 4, 5, 6, 7)
ODD_ROW = 4001


def ms_axis(n):
    return tuple(T0 + i * MS for i in range(n))


@functools.lru_cache(maxsize=None)
def extreme_values(shape, n=N_EXT):
    rng = random.Random(EXT_SEED + shape)
    if shape == 1:
        return tuple(dense_walk(rng, n, 5))
    if shape in (2, 3, 4):
        first = 10 ** 9 if shape == 4 else 10 ** 6
        v, out = first, [first]
        for i in range(1, n):
            if shape == 2:
                d = 63 if i % 2 else -64
            elif shape == 3:
                d = -64 if i == ODD_ROW else 63
            else:
                d = 63 if i == ODD_ROW else -64
            v = wrap64(v + d)
            out.append(v)
        return tuple(out)
    first, deltas = {5: (2 ** 63 - 1001, (63, 62, -1)),
                     6: (2 ** 63 - 5, None),
                     7: (7, (-64, 63, 0, -1, 1))}[shape]
    if deltas is None:
        return tuple(dense_walk(rng, n, first))
    v, out = first, [first]
    for _ in range(n - 1):
        v = wrap64(v + rng.choice(deltas))
        out.append(v)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def extremes_part():
    ts = ms_axis(N_EXT)
    return Part("extremes", [Blk(ts, extreme_values(k), "extreme%d" % k)
                             for k in EXT_SHAPES])


@functools.lru_cache(maxsize=None)
def extremes_f64_part():
    """Decimal mantissas following shape 1 from 10**6."""
    rng = random.Random(EXT_SEED + 100)
    cents = dense_walk(rng, N_EXT, 10 ** 6)
    return Part("extremes_f64",
                [Blk(ms_axis(N_EXT), [c / 100.0 for c in cents], "extreme1")],
                float_vals=True)


@functools.lru_cache(maxsize=None)
def extremes_tag_part():
    """Shapes 2 and 5 under a per-row tag (unclamped group-by)."""
    rng = random.Random(EXT_SEED + 200)
    ts = ms_axis(N_EXT)
    return Part("extremes_tagged",
                [Blk(ts, extreme_values(k), "extreme%d" % k,
                     random_tags(rng, N_EXT, 2)) for k in (2, 5)])


# shape 8: shape 1 at every swept stream length, each behind a filler
# block of varying encoded size so that field_off lands on every alignment
LEN_REPS = 2
LEN_SEED = 0x1E85


@functools.lru_cache(maxsize=None)
def length_cases():
    """(filler seed, ts, vals) per swept block."""
    rng = random.Random(LEN_SEED)
    cases = []
    for _ in range(LEN_REPS):
        for ln in LENGTHS:
            cases.append((rng.randrange(1 << 30), ms_axis(ln + 1),
                          tuple(dense_walk(rng, ln + 1, 5))))
    return tuple(cases)


def add_length_case(pb, case, gid):
    """Filler as group gid, the swept block as group gid + 1."""
    fseed, ts, vals = case
    frng = random.Random(fseed)
    k = frng.randint(1, 24)
    pb.add_block_i64(gid + 1, [T0 + i * MS for i in range(k)], [1] * k,
                     [frng.randint(-2 ** 40, 2 ** 40) for _ in range(k)],
                     group_code=gid)
    pb.add_block_i64(gid + 2, list(ts), [1] * len(ts), list(vals),
                     group_code=gid + 1)


@functools.lru_cache(maxsize=None)
def lengths_builder():
    pb = PartBuilder()
    for i, case in enumerate(length_cases()):
        add_length_case(pb, case, 2 * i)
    return pb


# ---------------------------------------------------------------------
# the per-row restatement
# ---------------------------------------------------------------------
def ref_part(part, lo, hi, keep=None):
    """Per block (count, sum, min, max) of the rows with lo <= ts <= hi
    (and keep(block, row) if given).  The int sum wraps to int64; a float
    part returns the selected values instead, for math.fsum.  Blocks that
    share one timestamp tuple share the row selection."""
    sels, out = {}, []
    for blk in part.blocks:
        sel = sels.get(id(blk.ts))
        if sel is None:
            sel = sels[id(blk.ts)] = [i for i, t in enumerate(blk.ts)
                                      if lo <= t <= hi]
        if keep is not None:
            sel = [i for i in sel if keep(blk, i)]
        if sel and sel[-1] - sel[0] + 1 == len(sel):
            vals = blk.vals[sel[0]:sel[-1] + 1]     # the same rows, sliced
        else:
            vals = [blk.vals[i] for i in sel]
        if not vals:
            out.append((0, [] if part.float_vals else 0, None, None))
            continue
        s = list(vals) if part.float_vals else wrap64(sum(vals))
        out.append((len(vals), s, min(vals), max(vals)))
    return out
