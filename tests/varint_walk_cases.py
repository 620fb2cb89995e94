"""Inputs of the varint window walk tests: delta and delta-of-delta lists
whose varints of 2 to 10 bytes straddle the 64-byte window boundary with
every carry count from 1 to 9, as field columns and as timestamp axes.

One layout per (pad, width), in varint byte lengths:
    pad one-byte varints, a pair of `width`-byte ones (the first crosses
    byte 64 whenever pad + width > 64, with 64 - pad bytes before it), one-
    byte varints up to byte 128, 255 more up to byte 383, a second pair (its
    first byte is the last of the 256-byte window at 128), six one-byte
    varints.
That is 373 to 389 varints: the 256-byte window has to lie wholly behind the
64-byte window that completes the carried varint, so a list cannot be
shorter and still pass from a quad window into the generic step and back.
The wide varints come in pairs because an ascending delta-of-delta axis has
to undo a wide second difference at once."""
import functools
import random

import clamp_cases as cc
import row_dedup_cases as rdc
from test_gpu_fuzz import TAGS

PADS = tuple(range(55, 64))
WIDTHS = (2, 3, 5, 9, 10)
SHAPES = tuple((pad, w) for w in WIDTHS for pad in PADS)
SEED = 0x5A1C
ENC_DELTA, ENC_DOD = 3, 4
TS_START = -9_200_000_000_000_000_000
TS_D1 = 40_000              # first step of a delta-of-delta axis


def layout(pad, width):
    return [1] * pad + [width] * 2 + [1] * (128 - pad - 2 * width) + \
        [1] * 255 + [width] * 2 + [1] * 6


def zz_dec(u):
    return (u >> 1) if u & 1 == 0 else -(u >> 1) - 1


def zz_bounds(width):
    """Zigzag values whose varint is `width` bytes long: [lo, hi)."""
    return (0 if width == 1 else 1 << 7 * (width - 1)), min(1 << 7 * width,
                                                            1 << 64)


def signed_of_width(rng, width):
    lo, hi = zz_bounds(width)
    return zz_dec(rng.randrange(lo, hi))


def wide_step(rng, width):
    """A positive step whose varint is `width` bytes, from the low eighth of
    the range so that a few of them fit into int64."""
    lo = zz_bounds(width)[0] // 2
    return lo + lo // 16 + rng.randrange(lo // 16 + 1)


# ---------------------------------------------------------------------
# field columns (values wrap)
# ---------------------------------------------------------------------
def field_delta_values(rng, pad, width):
    """First value and two leading deltas that rule out the const, delta-
    const, monotone and incremental forms: the encoder writes Delta."""
    steps = [signed_of_width(rng, w) for w in layout(pad, width)]
    steps[0], steps[1] = 5, -1
    out = [1000]
    for d in steps:
        out.append(cc.wrap64(out[-1] + d))
    return out


def field_dod_values(rng, pad, width):
    """A negative first value: the encoder writes DeltaOfDelta."""
    out = [-1000, -997]
    d1 = 3
    for w in layout(pad, width):
        d1 = cc.wrap64(d1 + signed_of_width(rng, w))
        out.append(cc.wrap64(out[-1] + d1))
    return out


def short_runs(rng, n):
    """A tag column in runs of 1 to 5 rows over two values and nil, so that
    a predicate on either value selects rows in every window."""
    tags = []
    while len(tags) < n:
        tags += [rng.choice((TAGS[0], TAGS[0], TAGS[1], None))] * \
            rng.randint(1, 5)
    return tags[:n]


@functools.lru_cache(maxsize=None)
def field_part():
    """Every shape as a Delta and as a DeltaOfDelta field column on a 1 ms
    axis, under a row-varying tag; blocks[2k] is Delta, blocks[2k+1]
    DeltaOfDelta of SHAPES[k]."""
    rng = random.Random(SEED)
    blocks = []
    for pad, w in SHAPES:
        for gen, kind in ((field_delta_values, "delta"),
                          (field_dod_values, "dod")):
            vals = gen(rng, pad, w)
            n = len(vals)
            blocks.append(cc.Blk(cc.ms_axis(n), vals,
                                 "%s_%d_%d" % (kind, pad, w),
                                 short_runs(rng, n)))
    return cc.Part("varint_walk_field", blocks)


def pair_rows(pad, width, dod):
    """Rows of the first wide varint of each pair of a shape's list: the
    stream's varint k is row k + 1, or k + 2 of a delta-of-delta list."""
    off = 2 if dod else 1
    return pad + off, 385 - 2 * width + off


def field_clamps():
    """Whole range, and two clamps whose ends lie in the rows of the wide
    varints (rows 56..66 and, for the second pair, 366..384)."""
    ts = cc.ms_axis(400)
    whole = (0, 0, 0, 0, cc.INT64_MIN, cc.INT64_MAX)
    return (whole, (3, 60, 0, 0, ts[3], ts[60]),
            (58, 375, 0, 0, ts[58], ts[375]))


# ---------------------------------------------------------------------
# timestamp axes (ascending, inside int64)
# ---------------------------------------------------------------------
def n_pairs(width):
    """Wide pairs an axis can hold: a 10-byte step is at least 2^62."""
    return 1 if width == 10 else 2


def ts_delta_axis(rng, pad, width):
    ts, seen = [TS_START], 0
    for w in layout(pad, width):
        if w > 1 and seen < 2 * n_pairs(width):
            seen += 1
            step = wide_step(rng, width)
        else:
            step = rng.randint(1, 63)
        ts.append(ts[-1] + step)
    return ts


def ts_dod_axis(rng, pad, width):
    """Second differences by the layout; a wide one is undone by the next,
    so exactly one row per pair takes the wide step."""
    lo = zz_bounds(width)[0] // 2
    k = min(60, lo // 32)
    ts, d1 = [TS_START, TS_START + TS_D1], TS_D1
    seen, undo = 0, None
    for w in layout(pad, width):
        if w > 1 and seen < 2 * n_pairs(width):
            seen += 1
            if undo is None:
                undo = wide_step(rng, width)
                d2 = undo
            else:
                d2 = -(undo + rng.randint(-k, k))
                undo = None
        else:
            d2 = rng.randint(-64, 63)
        d1 += d2
        ts.append(ts[-1] + d1)
    return ts


@functools.lru_cache(maxsize=None)
def ts_axes():
    """(pad, width, raw_delta, axis) per shape and coding."""
    rng = random.Random(SEED + 1)
    out = []
    for pad, w in SHAPES:
        out.append((pad, w, True, tuple(ts_delta_axis(rng, pad, w))))
        out.append((pad, w, False, tuple(ts_dod_axis(rng, pad, w))))
    for _, _, _, ts in out:
        assert cc.INT64_MIN <= ts[0] and ts[-1] <= cc.INT64_MAX
        assert all(a < b for a, b in zip(ts, ts[1:]))
    return tuple(out)



@functools.lru_cache(maxsize=None)
def clamp_blocks():
    """One block per axis, group code = block index."""
    rng = random.Random(SEED + 2)
    return tuple(rdc.DBlk(i + 1, ts, [1] * len(ts), rdc.ivals(rng, len(ts)),
                          group_code=i, raw_delta_ts=raw)
                 for i, (_, _, raw, ts) in enumerate(ts_axes()))


def ts_clamps():
    """Per axis, bounds on the rows on either side of each pair's two wide
    varints (rows a, a + 1 and b, b + 1): up to a - 1, a .. b - 1,
    a + 1 .. b, and from b + 1 on."""
    out = []
    for pad, w, raw, ts in ts_axes():
        a, b = pair_rows(pad, w, not raw)
        out += [(ts[0], ts[a - 1]), (ts[a], ts[b - 1]), (ts[a + 1], ts[b]),
                (ts[b + 1], ts[-1])]
    return tuple(dict.fromkeys(out))


def wide_versions(rng, n):
    """Versions with multi-byte deltas of both signs."""
    v = [2, 0, 3]
    while len(v) < n:
        v.append(rng.choice([rng.randint(0, 3), rng.randint(10 ** 3, 10 ** 9),
                             rng.randint(10 ** 12, 10 ** 15)]))
    return v[:n]


@functools.lru_cache(maxsize=None)
def dedup_blocks():
    """Per axis three blocks of one series, group code = axis index: two
    over the same timestamps and one over the axis without its first row.
    The third block's stream is the same varints one place earlier, so
    every window boundary falls elsewhere and row i of it has to meet row
    i + 1 of the others: a decode that went wrong the same way in two
    equal lists would still pair their rows, not these."""
    rng = random.Random(SEED + 3)
    blocks = []
    for i, (_, _, raw, ts) in enumerate(ts_axes()):
        for rows in (ts, ts, ts[1:]):
            blocks.append(rdc.DBlk(i + 1, rows, wide_versions(rng, len(rows)),
                                   rdc.ivals(rng, len(rows)), group_code=i,
                                   raw_delta_ts=raw))
    return tuple(blocks)


# ---------------------------------------------------------------------
# what the encoded streams hold
# ---------------------------------------------------------------------
def crossings(stream, start=0):
    """(carried bytes, varint length) of every varint of stream[start:]
    that crosses a multiple of 64 counted from `start`."""
    out, a = [], start
    for i in range(start, len(stream)):
        if stream[i] < 0x80:
            lo, hi = a - start, i - start       # first and last byte
            if lo // 64 != hi // 64:
                out.append((64 * (hi // 64) - lo, hi - lo + 1))
            a = i + 1
    return out


def skip_varint(stream):
    """Length of the leading varint (a delta-of-delta stream's d1)."""
    return next(i for i, b in enumerate(stream) if b < 0x80) + 1
