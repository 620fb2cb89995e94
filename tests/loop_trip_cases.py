"""Parts with more blocks than the per-block kernels have waves or
workgroups, shared by test_loop_trips_cpu.py and test_gpu_loop_trips.py.

Every per-block kernel launches a capped grid and goes round a grid-stride
loop past the cap (banyandb_amd/csrc/kernels.hip: SCAN_MAX_WGS workgroups of
4 waves for k_scan_agg_t / k_top_bounds / k_rows_bounds, BLOCK_KERNEL_MAX_WGS
workgroups for the 64-thread kernels).  The parts here put different kinds of
block at the two indices one wave (one workgroup) handles, so state carried
from its first trip into its second shows in the result:

  part S   int64, 4 x 8192 + 1500 blocks of 1..5 rows (a few of 65 and 130)
  twin     part S with the nulls of its Plain blocks filled in (the top-N and
           row scans take no null-bearing blocks)
  part F   the same skeleton in float64 decimals with three block exponents
  part B   65535 + 500 blocks, one-row fillers around the blocks the
           64-thread resolve / pack kernels work on
  part D   pairs of two-row blocks with crossed versions: every block is
           involved in the dedup and partially superseded

The block counts below are literals on purpose: test_loop_trips_cpu.py
compares them with the caps it reads from kernels.hip, so raising a cap
fails there instead of silently turning these into one-trip parts."""
import ctypes as C
import functools
import os
import random
import re

from banyandb_amd import (PartBuilder, BlockDesc, TagCond, Or, OP_EQ, OP_NE,
                          OP_IN, OP_GE, VT_INT64, VT_FLOAT64, INT64_MIN,
                          INT64_MAX)
import oracle as o
from helpers import oracle_blocks
import filter_cases as fc
import row_dedup_cases as rdc
from row_dedup_cases import DBlk, T0, MS

KERNELS = os.path.join(rdc.REPO, "banyandb_amd", "csrc", "kernels.hip")

N_S = 4 * 8192 + 1500          # blocks of parts S, twin and F
N_B = 65535 + 500              # blocks of part B
N_D_PAIRS = 32768 + 300        # part D: two blocks per pair, plus D_FULL
MAX_ROWS = 150_000             # per part: the per-row models stay quick

ENC_CONST, ENC_DELTA_CONST, ENC_DELTA, ENC_DOD, ENC_PLAIN = 1, 2, 3, 4, 9
IMIN, IMAX = INT64_MIN, INT64_MAX


@functools.lru_cache(maxsize=None)
def caps():
    """{'SCAN_MAX_WGS': .., 'BLOCK_KERNEL_MAX_WGS': ..} from the #define
    lines of kernels.hip."""
    with open(KERNELS) as f:
        text = f.read()
    out = {}
    for name in ("SCAN_MAX_WGS", "BLOCK_KERNEL_MAX_WGS"):
        m = re.findall(r"^#define[ \t]+%s[ \t]+(\d+)[ \t]*$" % name, text,
                       re.M)
        assert len(m) == 1, (name, m)
        out[name] = int(m[0])
    return out


def scan_waves():
    return 4 * caps()["SCAN_MAX_WGS"]


class PartView:
    """A built part under patched descriptors: the same payload, every
    block's group code replaced (a session without groups refuses codes
    above 0)."""

    def __init__(self, pb, group_code=None):
        self._pb = pb
        n = pb.n_blocks
        self._descs = (BlockDesc * n)()
        C.memmove(self._descs, pb.blocks_ptr(), C.sizeof(BlockDesc) * n)
        if group_code is not None:
            for d in self._descs:
                d.group_code = group_code
        self.n_blocks = n
        self.payload_len = pb.payload_len

    @property
    def payload(self):
        return self._pb.payload

    def raw_payload_ptr(self):
        return self._pb.raw_payload_ptr()

    def blocks_ptr(self):
        return self._descs

    def blocks(self):
        return list(self._descs)


# ---------------------------------------------------------------- part S
# kind of block i: KINDS[i % 11].  11 does not divide the wave count, and
# neighbours in the cycle differ, so the two blocks of a wave differ in kind.
KINDS = ("const", "dconst", "dense", "multi", "dod", "plain", "dense",
         "const", "multi", "dod", "dconst")
MIN_ROWS = {"const": 1, "dconst": 2, "dense": 3, "multi": 3, "dod": 3,
            "plain": 1}
ENVS = fc.ENVS[:4]
DOMAIN = [b"a", b"b", b"c"]      # slot 1
DOMAIN2 = [b"p", b"q", b"r"]     # slot 2
LIT = b"b"                       # the EQ predicate on slot 1
N_SHAPES = 9                     # slot-1 shapes, by i % 9
N_SHAPES2 = 7                    # slot-2 shapes, by i % 7
# off the microsecond grid the block starts lie on: only the rows placed
# here on purpose (block EDGES) have these timestamps
CLAMP = (T0 + 3 * MS - 500, T0 + 12 * MS + 500_500)
# Cycles of all kinds at fixed places.  Past the scan cap: one touching
# INT64_MAX, one touching INT64_MIN — every true extreme of the part lies in
# a block that a wave reaches on its second trip only.  Below the cap: the
# values next to them, so the best rows lie on both sides.
EXT_LO, EXT_HI = 22, 4 * 8192 + 330
TOUCH_MAX = {"const": [IMAX] * 3, "dconst": [IMAX - 10, IMAX - 5, IMAX],
             "dense": [IMAX - 3, IMAX, IMAX - 2],
             "multi": [IMAX - 10 ** 6, IMAX, IMAX - 500],
             "dod": [IMAX - 100, IMAX - 30, IMAX],
             "plain": [IMAX, None, IMAX - 1]}
TOUCH_MIN = {"const": [IMIN] * 3, "dconst": [IMIN, IMIN + 5, IMIN + 10],
             "multi": [5, IMIN, 3], "dod": [IMIN, IMIN + 7, IMIN + 3],
             "plain": [IMIN, None, IMIN + 1]}
NEAR_MAX = {"const": [IMAX - 50] * 3,
            "dconst": [IMAX - 70, IMAX - 65, IMAX - 60],
            "dense": [IMAX - 83, IMAX - 80, IMAX - 82],
            "dod": [IMAX - 200, IMAX - 130, IMAX - 100],
            "plain": [IMAX - 90, None, IMAX - 91]}
NEAR_MIN = {"const": [IMIN + 50] * 3,
            "dconst": [IMIN + 60, IMIN + 65, IMIN + 70],
            "dod": [IMIN + 80, IMIN + 87, IMIN + 83],
            "plain": [IMIN + 90, None, IMIN + 91]}
FIXED_VALUES = ((EXT_LO, NEAR_MIN), (EXT_LO + 11, NEAR_MAX),
                (EXT_HI, TOUCH_MAX), (EXT_HI + 11, TOUCH_MIN))
# two blocks past the scan cap that hold the first and the last row of every
# selection the row scans use (slot 1 = LIT on all their rows): LATEST ends
# the part; EDGES has the earliest row of the part and one row on either end
# of the clamp
LATEST = 4 * 8192 + 701
EDGES = 4 * 8192 + 702
EDGES_TS = [T0 - 5 * MS, CLAMP[0], CLAMP[1]]


def kind_of(i, flt=False):
    k = KINDS[i % len(KINDS)]
    return "const" if flt and k == "plain" else k


def n_rows_of(i, flt=False):
    if i == LATEST:
        return 131
    if i == EDGES:
        return 3
    if i % 149 == 5:
        return 65
    if i % 293 == 11:
        return 130
    return max(1 + i % 5, MIN_ROWS[kind_of(i, flt)])


def ts_of(i, n):
    """Start on a 13-step grid (so a clamp covers, cuts and misses blocks)
    plus a sub-millisecond offset that interleaves the blocks of both sides
    of the cap in time order; every fourth block irregular."""
    if i == EDGES:
        return list(EDGES_TS)
    t = T0 + (i % 13) * 2 * MS + ((i * 7919) % 1000) * 1000
    if i == LATEST:
        t = T0 + 24 * MS + 999_999
    out = [t]
    for r in range(1, n):
        t += (1 + (r * r + i) % 3) * MS if i % 4 == 1 else MS
        out.append(t)
    return out


def ints_of(rng, kind, n, big):
    """n values the part builder encodes as `kind`."""
    if kind == "const":
        return [rng.randint(-big, big)] * n
    if kind == "dconst":
        v, step = rng.randint(-big, big), rng.choice((-7, 3, 1000))
        return [v + j * step for j in range(n)]
    v = rng.randint(big // 8, big)
    out = [v]
    for j in range(n - 1):
        if kind == "dense":       # mixed signs, every |delta| < 64
            v += (1, -2)[j] if j < 2 else rng.randint(-60, 60)
        elif kind == "multi":     # mixed signs, deltas of 2 and 3 bytes
            v += (10 ** 5, -3 * 10 ** 4)[j] if j < 2 else \
                rng.randint(-big // 1000, big // 1000)
        else:                     # monotone, not arithmetic: delta of delta
            v += (1, 2)[j] if j < 2 else rng.randint(1, 50)
        out.append(v)
    return out


def slot1_of(i, n):
    """The row-varying dictionary tag; nils in shapes 4, 5 and 6."""
    s = i % N_SHAPES
    if s in (0, 1) or i in (LATEST, EDGES):
        return [b"b"] * n
    if s == 2:
        return [b"a"] * n
    if s == 3:
        return [DOMAIN[(i + r) % 3] for r in range(n)]
    if s == 4:
        return [None if r % 3 == 1 else DOMAIN[(i + r) % 3] for r in range(n)]
    if s == 5:
        return [None] * n
    if s == 6:
        return [None if r % 2 else b"b" for r in range(n)]
    if s == 7:
        return [(b"a", b"c")[(i + r) % 2] for r in range(n)]
    return [b"c"] * n


def slot2_of(i, n):
    """A second row-varying dictionary tag, for a group-by under the
    predicate on slot 1 (EQ on the grouped slot itself would leave one
    group); shapes 0 and 1 are equal, so the two blocks of a wave can share
    a group."""
    s = i % N_SHAPES2
    if s in (0, 1):
        return [b"p"] * n
    if s == 2:
        return [b"q"] * n
    if s == 3:
        return [DOMAIN2[(i + r) % 3] for r in range(n)]
    if s == 4:
        return [None if r % 3 == 2 else DOMAIN2[(i + 2 * r) % 3]
                for r in range(n)]
    if s == 5:
        return [b"r"] * n
    return [(b"q", b"r")[(i + r) % 2] for r in range(n)]


@functools.lru_cache(maxsize=None)
def s_rows(flt=False):
    """Blocks of part S (flt: part F) as DBlk; a Plain block's vals hold
    None for its nulls.  Group code i % 3."""
    rng = random.Random(0xF10A7 if flt else 0x5CA9)
    big = 10 ** 5 if flt else 10 ** 9
    out = []
    for i in range(N_S):
        kind = kind_of(i, flt)
        n = n_rows_of(i, flt)
        vals = ints_of(rng, kind, n, big)
        if kind == "plain":
            vals = [None if n > 1 and (r == 1 or rng.random() < 0.3) else v
                    for r, v in enumerate(vals)]
        if not flt:
            for start, fixed in FIXED_VALUES:
                if start <= i < start + 11 and kind in fixed:
                    vals, n = fixed[kind], 3
        else:
            # exponent class i % 3: quarters, halves, whole numbers (exact
            # in binary, so per-row double sums are exact)
            vals = [v * (0.25, 0.5, 1.0)[i % 3] for v in vals]
        tags = [[ENVS[(i // 3) % 4]] * n, slot1_of(i, n), slot2_of(i, n)]
        blk = DBlk(i + 1, ts_of(i, n), [1] * n, vals, tags, i % 3)
        blk.nullable = kind == "plain"      # a Plain cell block, even when
        out.append(blk)                     # its only row is not null
    return tuple(out)


@functools.lru_cache(maxsize=None)
def twin_rows():
    """Part S with the nulls filled in."""
    out = []
    for b in s_rows():
        vals = [7 * (r + 1) if v is None else v for r, v in enumerate(b.vals)]
        out.append(DBlk(b.sid, b.ts, b.vers, vals, b.tags, b.group_code))
    return tuple(out)


def _build(blocks, flt=False):
    pb = PartBuilder()
    for b in blocks:
        if flt:
            add = pb.add_block_f64
        elif getattr(b, "nullable", False):
            add = pb.add_block_i64_nullable
        else:
            add = pb.add_block_i64
        add(b.sid, b.ts, b.vers, b.vals, group_code=b.group_code)
        for col in b.tags:
            pb.set_block_tag(col)
    return pb


@functools.lru_cache(maxsize=None)
def part(name, coded=False):
    """name: 's', 'twin', 'f', 'b', 'd'.  coded=False: every group code 0
    (sessions without block-code groups)."""
    return PartView(_builder(name), None if coded else 0)


def rows_of(name):
    return {"s": s_rows, "twin": twin_rows, "f": lambda: s_rows(True),
            "b": b_rows, "d": d_rows}[name]()


@functools.lru_cache(maxsize=None)
def _builder(name):
    return _build(rows_of(name), flt=name == "f")


@functools.lru_cache(maxsize=None)
def model(name):
    """The rows the engine folds, for the per-row models: null rows
    deleted, emptied blocks dropped (the fold skips nulls)."""
    out = []
    for b in rows_of(name):
        keep = [r for r, v in enumerate(b.vals) if v is not None]
        if len(keep) == len(b.vals):
            out.append(b)
        elif keep:
            out.append(DBlk(b.sid, [b.ts[r] for r in keep],
                            [b.vers[r] for r in keep],
                            [b.vals[r] for r in keep],
                            [[col[r] for r in keep] for col in b.tags],
                            b.group_code))
    return out


@functools.lru_cache(maxsize=None)
def _oracle_input(name, coded):
    return oracle_blocks(part(name, coded))


def group_slot(pred):
    """(slot, domain) of the tag group-by: slot 1, the issue's choice —
    except under the EQ predicate on slot 1, which would leave that group-by
    a single group (and a wave's partial nothing to flush): then slot 2."""
    return (2, DOMAIN2) if pred else (1, DOMAIN)


@functools.lru_cache(maxsize=None)
def oracle_agg(name, pred=False, group=None, clamp=False):
    """The C oracle over the encoded part.  group: None, 'tag' (group_slot)
    or 'code' (3 block-code groups).  Returns AggResult per group."""
    payload, blocks = _oracle_input(name, group == "code")
    vt = VT_FLOAT64 if name == "f" else VT_INT64
    lo, hi = CLAMP if clamp else (INT64_MIN, INT64_MAX)
    preds = [b"", LIT] if pred else None
    if group == "tag":
        slot, domain = group_slot(pred)
        return o.scan_agg_bytags(payload, blocks, vt, [slot], [domain], lo,
                                 hi, preds=preds)
    return o.scan_agg(payload, blocks, vt, lo, hi, preds=preds,
                      n_groups=3 if group == "code" else 1)


# the 16 queries of the scan matrix: (all four functions, predicate, tag
# group-by, clamp)
MATRIX = [(v, p, g, c) for v in (False, True) for p in (False, True)
          for g in (False, True) for c in (False, True)]


def matrix_id(q):
    v, p, g, c = q
    return "%s-%s-%s-%s" % ("minmax" if v else "sumcount",
                            "pred" if p else "nopred",
                            "bytag" if g else "nogroup",
                            "clamp" if c else "full")


def instantiations(q):
    """k_scan_agg_t<EN_VALUES, EN_PREDS, EN_GROUPS, EN_WALK, EN_CLAMP> that
    launch_scan picks for the query: the light pass, and with a predicate
    the heavy (EN_WALK) pass as well."""
    v, p, g, c = (int(x) for x in q)
    out = [(v, p, g, 0, c)]
    if p:
        out.append((v, p, g, 1, c))
    return out


# filter cases on part S
CONDS = [TagCond(0, OP_NE, [ENVS[1]]), TagCond(1, OP_IN, list(DOMAIN))]
TREE = Or(TagCond(1, OP_EQ, [b"b"]), TagCond(0, OP_EQ, [ENVS[1]]),
          TagCond(1, OP_EQ, [b"c"]))

TOP_NS = (1, 100, 1024)
ROW_WINDOWS = ((0, 1), (900, 124))
# how the top-N and row scans are filtered: name -> Scen keywords
SELECTIONS = {
    "all": {},
    "clamp": dict(min_ts=CLAMP[0], max_ts=CLAMP[1]),
    "pred": dict(conds=[TagCond(1, OP_EQ, [LIT])]),
}


@functools.lru_cache(maxsize=None)
def _scan_rows(name, sel, dedup=False):
    import top_rows_ref as trr
    return tuple(trr.scan_rows(list(rows_of(name)), dedup=dedup,
                               **SELECTIONS[sel]))


@functools.lru_cache(maxsize=None)
def _ordered(name, sel, desc, dedup=False):
    import row_scan_ref as rsr
    return tuple(rsr.ordered(_scan_rows(name, sel, dedup), desc))


@functools.lru_cache(maxsize=None)
def top_expected(sel, n, asc, name="twin"):
    """top_rows_ref over the twin: tuples of the expected rows."""
    import top_rows_ref as trr
    rows = _scan_rows(name, sel)
    return tuple(rows[i].astuple()
                 for i in trr.batch_top([r.key for r in rows], n, asc))


@functools.lru_cache(maxsize=None)
def rows_expected(sel, offset, limit, desc, name="twin", dedup=False):
    """row_scan_ref over the twin (or the deduped part D)."""
    import row_scan_ref as rsr
    return tuple(r.astuple() for r in rsr.window(
        _ordered(name, sel, desc, dedup), offset, limit))


def sides(tuples, cap):
    """Which sides of block index `cap` the rows (astuple, seq last) lie
    on: a set out of {'below', 'past'}."""
    return {"past" if (t[5] >> 13) >= cap else "below" for t in tuples}


def verdict(b):
    """PF_* verdict of the EQ predicate over one block, from its rows."""
    hit = [v == LIT for v in b.tags[1]]
    return "clear" if all(hit) else "walk" if any(hit) else "skip"


def group_shape(b, slot=1):
    return "uniform" if len(set(b.tags[slot])) == 1 else "varying"


def clamp_shape(b):
    inside = [CLAMP[0] <= t <= CLAMP[1] for t in b.ts]
    return "whole" if all(inside) else "cut" if any(inside) else "missed"


# ---------------------------------------------------------------- part B
B_WORK = 500                     # work blocks lie in [0, B_WORK) and in
B_HI = 65535                     # [B_HI, B_HI + B_WORK)
B_PLAIN_DOMAIN = [b"u%d" % k for k in (3, 17, 140, 260)]
B_CONDS = [TagCond(0, OP_GE, [b"u3"])]
B_TREE = Or(TagCond(0, OP_EQ, [b"prod"]), TagCond(1, OP_EQ, [b"y"]))


def _b_kind(j):
    """j: index relative to the start of a work window."""
    if j % 25 == 3:
        return "plain"           # > 256 distinct values on slot 0
    if j % 10 == 1:
        return "hit"             # dense, every delta in [-8, 7]
    if j % 10 == 6:
        return "nohit"           # dense, one delta beyond
    if j % 10 == 8:
        return "bitmap"          # two row-varying dictionary slots
    return "filler"


@functools.lru_cache(maxsize=None)
def b_rows():
    rng = random.Random(0xB10C)
    out = []
    for i in range(N_B):
        j = i if i < B_WORK else i - B_HI if i >= B_HI else -1
        kind = _b_kind(j) if j >= 0 else "filler"
        if kind == "filler":
            n, vals = 1, [rng.randint(-10 ** 6, 10 ** 6)]
            tags = [[(b"f", b"u9")[i % 2]], [b"z"]]
        elif kind == "plain":
            n = 270
            vals = rdc.ivals(rng, n)
            tags = [rdc.plain_col(rng, n), [b"z"] * n]
        elif kind in ("hit", "nohit"):
            n = rng.choice((3, 4, 34, 65, 130))
            v = rng.randint(10 ** 6, 10 ** 9)
            vals = [v]
            for r in range(n - 1):
                v += (1, -2)[r] if r < 2 else rng.randint(-8, 7)
                vals.append(v)
            if kind == "nohit":
                vals[-1] -= 20
            tags = [[b"f"] * n, [b"z"] * n]
        else:
            n = 40
            vals = rdc.ivals(rng, n)
            tags = [fc.runs(rng, n, fc.ENVS, maxrun=6, nil_p=0.1),
                    fc.runs(rng, n, [b"x", b"y", b"z"], maxrun=5, nil_p=0.1)]
        out.append(DBlk(i + 1, rdc.arith_ts(n), [1] * n, vals, tags, 0))
    return tuple(out)


def b_kinds():
    """index -> kind of every work block of part B."""
    out = {}
    for base in (0, B_HI):
        for j in range(B_WORK):
            if base + j < N_B and _b_kind(j) != "filler":
                out[base + j] = _b_kind(j)
    return out


# ---------------------------------------------------------------- part D
D_FULL = (5, 90, 32768 + 40, 32768 + 250)   # pairs followed by a third,
                                            # fully superseded block
D_COND = [TagCond(0, OP_EQ, [b"x"])]


@functools.lru_cache(maxsize=None)
def d_rows():
    """Pair p: one series, two timestamps, block A at versions (1, 3) and
    block B at (2, 2): A keeps its second row, B its first.  After the pairs
    in D_FULL a block C at versions (0, 0) loses both rows."""
    rng = random.Random(0xDD)
    out = []
    for p in range(N_D_PAIRS):
        t = T0 + ((p * 7919) % N_D_PAIRS) * 10 * MS
        if p >= 32768 and p % 12 == 0:      # 25 pairs past the cap hold the
            t += N_D_PAIRS * 10 * MS        # latest rows of the part
        ts = [t, t + MS]
        x, y = ((b"x", b"y"), (b"y", b"x"))[p % 2]
        for vers, tags in (((1, 3), [x, y]), ((2, 2), [y, b"x"])):
            out.append(DBlk(p + 1, ts, list(vers), rdc.ivals(rng, 2), [tags]))
        if p in D_FULL:
            out.append(DBlk(p + 1, ts, [0, 0], rdc.ivals(rng, 2),
                            [[b"x", b"x"]]))
    return tuple(out)


def d_census():
    """row_dedup_ref.stats of part D.  Blocks of different series never
    pair, and every figure of the census adds over series, so the model's
    quadratic pairing runs per series."""
    import row_dedup_ref as ref
    by_sid = {}
    for b in d_rows():
        by_sid.setdefault(b.sid, []).append(b)
    total = [0, 0, 0, 0]
    for blocks in by_sid.values():
        total = [a + b for a, b in zip(total, ref.stats(blocks))]
    return total
