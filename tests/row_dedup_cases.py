"""Scenario builders shared by the CPU and GPU cross-part version dedup
tests.  A scenario is a list of blocks in append order (several on-disk
parts appended to one resident part) that keeps the rows it was generated
from: row_dedup_ref says which rows survive, and the existing checkers
(filter_ref, filter_tree_ref, helpers.oracle_scan) fold the survivors."""
import ctypes as C
import os
import random
import subprocess

from banyandb_amd import (PartBuilder, TagCond, Or, OP_EQ, OP_NE, OP_GE,
                          OP_IN, TAG_INT, BlockDesc)
import oracle as o
import filter_cases as fc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T0 = fc.T0
MS = fc.MS
ENVS = fc.ENVS
CODES = [fc.icell(c) for c in (200, 404, 500, 503)]

ENC_CONST, ENC_DELTA_CONST, ENC_DELTA, ENC_DOD = 1, 2, 3, 4
ENC_DELTA_WV = 7

I64, F64, I64N, F64N = "i64", "f64", "i64n", "f64n"


def build_consumer(exe):
    """Compile tools/cabi_row_dedup_check.c against the header alone."""
    subprocess.run(
        ["gcc", "-std=c99", "-Wall", "-Werror", "-I",
         os.path.join(REPO, "include"),
         os.path.join(REPO, "tools", "cabi_row_dedup_check.c"),
         "-L", os.path.join(REPO, "banyandb_amd"), "-lbydb_gpu",
         "-Wl,-rpath," + os.path.join(REPO, "banyandb_amd"), "-o", exe],
        check=True)


class DBlk:
    """One block: rows with versions, per-slot tag columns, and the block
    group code.  raw_delta_ts: store the timestamps as a plain Delta list
    (see RawPart)."""

    def __init__(self, sid, ts, vers, vals, tags=(), group_code=0,
                 raw_delta_ts=False):
        assert len(ts) == len(vers) == len(vals)
        assert all(a < b for a, b in zip(ts, ts[1:]))
        self.sid, self.ts, self.vers, self.vals = sid, list(ts), list(vers), \
            list(vals)
        self.tags = [list(c) for c in tags]
        self.group_code = group_code
        self.raw_delta_ts = raw_delta_ts


def builder(blocks, kind=I64):
    pb = PartBuilder()
    add = {I64: pb.add_block_i64, F64: pb.add_block_f64,
           I64N: pb.add_block_i64_nullable,
           F64N: pb.add_block_f64_nullable}[kind]
    for b in blocks:
        add(b.sid, b.ts, b.vers, b.vals, group_code=b.group_code)
        for col in b.tags:
            pb.set_block_tag(col)
    return pb


class RawPart:
    """A part with hand-patched descriptors, in the shape Session.upload_part
    reads.  The part builder writes ascending timestamps as Const,
    DeltaConst or DeltaOfDelta lists (an ascending list always passes the
    encoder's delta-of-delta test); the Delta form — which the decoder side
    must read all the same — is produced here: the block's timestamps are
    re-encoded as first value + zigzag varint deltas, followed by a copy of
    the block's version list, at the end of the payload."""

    def __init__(self, blocks, kind=I64):
        pb = builder(blocks, kind)
        payload = bytearray(pb.payload)
        descs = pb.blocks()
        out = (BlockDesc * len(descs))()
        for i, (d, b) in enumerate(zip(descs, blocks)):
            C.memmove(C.addressof(out[i]), C.addressof(d), C.sizeof(BlockDesc))
            if not b.raw_delta_ts:
                continue
            vers = bytes(payload[d.ts_off + d.ts_len: d.field_off])
            stream = o.varint_encode([y - x for x, y in zip(b.ts, b.ts[1:])])
            out[i].ts_off = len(payload)
            out[i].ts_len = len(stream)
            out[i].ts_enc_with_version = ENC_DELTA_WV
            payload.extend(stream + vers)
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


class Scen:
    """blocks + how they are queried.  group: None, ("code", n_groups) or
    ("tag", slot, domain).  At most one of conds / tree / pred."""

    def __init__(self, blocks, kind=I64, conds=None, tree=None, pred=None,
                 min_ts=None, max_ts=None, group=None):
        self.blocks = blocks
        self.kind = kind
        self.conds = conds
        self.tree = tree
        self.pred = pred
        self.min_ts = min_ts
        self.max_ts = max_ts
        self.group = group

    def part(self, blocks=None):
        blocks = self.blocks if blocks is None else blocks
        if any(b.raw_delta_ts for b in blocks):
            return RawPart(blocks, self.kind)
        return builder(blocks, self.kind)

    @property
    def n_rows(self):
        return sum(len(b.ts) for b in self.blocks)


# ---- row generators ----
def arith_ts(n, t0=T0, step=MS):
    return [t0 + i * step for i in range(n)]


def irregular_ts(rng, n, t0=T0, steps=(1, 2, 3, 5, 20, 31)):
    """Ascending, irregular: a DeltaOfDelta list."""
    ts = [t0]
    while len(ts) < n:
        ts.append(ts[-1] + rng.choice(steps) * MS)
    return ts


def ivals(rng, n):
    return [rng.randint(-10 ** 9, 10 ** 9) for _ in range(n)]


def fvals(rng, n):
    return [rng.randint(-10 ** 7, 10 ** 7) / 100.0 for _ in range(n)]


def mixed_versions(rng, n, hi=3):
    """Per-row versions in 0..hi with steps of both signs: a Delta list (a
    leading 2, 0, 3 rules out the const, delta-const and incremental
    forms)."""
    v = [2, 0, 3] + [rng.randint(0, hi) for _ in range(n - 3)]
    return v[:n]


def rising_versions(rng, n):
    v, out = 1, []
    for _ in range(n):
        v += rng.randint(0, 3)
        out.append(v)
    return out


def env_runs(rng, n, nil_p=0.1):
    return fc.runs(rng, n, ENVS, maxrun=40, nil_p=nil_p)


def code_runs(rng, n):
    return fc.runs(rng, n, CODES, maxrun=25, nil_p=0.05)


def plain_col(rng, n):
    col = [b"u%d" % i for i in range(min(n, 270))]
    col += [None if rng.random() < 0.1 else b"u%d" % rng.randrange(400)
            for _ in range(n - len(col))]
    rng.shuffle(col)
    return col


def resend(rng, blk, rows, vers, vals=None, tags=None, extra_ts=()):
    """A later part's block re-sending `rows` of blk (plus new timestamps
    extra_ts) with the given versions."""
    ts = [blk.ts[r] for r in rows] + list(extra_ts)
    n = len(ts)
    vals = ivals(rng, n) if vals is None else vals
    tags = tags if tags is not None else \
        [[rng.choice([v for v in col if v is not None] or [None])
          for _ in range(n)] for col in blk.tags]
    return DBlk(blk.sid, ts, vers, vals, tags, blk.group_code)


# ---- 1. identical series and timestamps, versions 1 against 2 ----
ROW_COUNTS = (1, 63, 64, 65, 129, 8192)


def identical_case(n, high_first):
    def make():
        rng = random.Random(9100 + n + high_first)
        ts = arith_ts(n)
        va, vb = (2, 1) if high_first else (1, 2)
        return Scen([DBlk(1, ts, [va] * n, ivals(rng, n)),
                     DBlk(1, ts, [vb] * n, ivals(rng, n))])
    return make


# ---- 2. partial overlap ----
def middle_third_case():
    rng = random.Random(9201)
    a = DBlk(1, arith_ts(300), [1] * 300, ivals(rng, 300))
    return Scen([a, resend(rng, a, range(100, 200), [2] * 100)])


def straddle_end_case():
    rng = random.Random(9202)
    a = DBlk(1, arith_ts(300), [1] * 300, ivals(rng, 300))
    extra = arith_ts(100, T0 + 300 * MS)
    return Scen([a, resend(rng, a, range(250, 300), [2] * 150,
                           extra_ts=extra)])


def interleaved_case():
    rng = random.Random(9203)
    a = DBlk(1, arith_ts(200, step=2 * MS), [1] * 200, ivals(rng, 200))
    b = DBlk(1, arith_ts(200, T0 + 101 * MS, 2 * MS), [2] * 200,
             ivals(rng, 200))
    return Scen([a, b])


# ---- 3. three blocks with versions 1, 3, 2 ----
def three_versions_case():
    rng = random.Random(9301)
    ts = arith_ts(150)
    return Scen([DBlk(1, ts, [v] * 150, ivals(rng, 150)) for v in (1, 3, 2)])


# ---- 4. per-row varying versions (Delta-coded version lists) ----
def varying_versions_case():
    rng = random.Random(9401)
    ts = arith_ts(500)
    return Scen([DBlk(1, ts, mixed_versions(rng, 500), ivals(rng, 500)),
                 DBlk(1, ts, mixed_versions(rng, 500), ivals(rng, 500))])


# ---- 5. timestamp encodings on both sides of a pair ----
def _axis(rng, enc, n):
    if enc == "arith1":
        return arith_ts(n), False
    if enc == "arith3":
        return arith_ts(n, step=3 * MS), False
    if enc == "dod":
        return irregular_ts(rng, n), False
    assert enc == "delta"
    return irregular_ts(rng, n), True


def encoding_pair_case(enc_a, enc_b, seed):
    """Block A on its own axis; block B re-sends every second timestamp of
    A that its own kind of axis can hold, with version 2."""
    def make():
        rng = random.Random(seed)
        ts_a, raw_a = _axis(rng, enc_a, 400)
        a = DBlk(1, ts_a, rising_versions(rng, 400), ivals(rng, 400),
                 raw_delta_ts=raw_a)
        if enc_b in ("arith1", "arith3"):
            ts_b, raw_b = _axis(rng, enc_b, 400)
        else:
            ts_b, raw_b = sorted(rng.sample(ts_a, 170)), enc_b == "delta"
        top = max(a.vers) + 1
        b = DBlk(1, ts_b, [top] * len(ts_b), ivals(rng, len(ts_b)),
                 raw_delta_ts=raw_b)
        return Scen([a, b])
    return make


def one_row_case(enc, seed):
    """A one-row Const block against an arith / stream-coded block."""
    def make():
        rng = random.Random(seed)
        ts_a, raw_a = _axis(rng, enc, 300)
        a = DBlk(1, ts_a, [1] * 300, ivals(rng, 300), raw_delta_ts=raw_a)
        hit = DBlk(1, [ts_a[137]], [2], [7])
        lose = DBlk(1, [ts_a[20]], [0], [9])
        return Scen([hit, a, lose])
    return make


W10 = 4_620_000_000_000_000_000          # zigzag(d2) needs 64 bits
WIDE_STEPS = {
    "two_byte": [100, 900, 3000],
    "mixed": [1, 1, 1, 10 ** 3, 10 ** 6, 10 ** 9, 10 ** 12],
    "wide": [10 ** 15, 3 * 10 ** 15],
}


def wide_varint_case(shape, seed):
    """Stream-coded timestamps whose varints are two to ten bytes long."""
    def make():
        rng = random.Random(seed)
        if shape == "ten_byte":
            ts = [-9_200_000_000_000_000_000]
            for step in (1, W10, 1, W10, 1, W10, 1):
                ts.append(ts[-1] + step)
            keep = [0, 2, 3, 5, 7]
        else:
            ts = [T0]
            for _ in range(299):
                ts.append(ts[-1] + rng.choice(WIDE_STEPS[shape]))
            keep = sorted(rng.sample(range(300), 120))
        n = len(ts)
        a = DBlk(1, ts, mixed_versions(rng, n, 5) if n > 8 else [1] * n,
                 ivals(rng, n))
        b = DBlk(1, [ts[r] for r in keep], [3] * len(keep),
                 ivals(rng, len(keep)))
        return Scen([a, b])
    return make


# ---- 7. same timestamps in different series ----
def different_series_case():
    rng = random.Random(9701)
    ts = arith_ts(200)
    return Scen([DBlk(s + 1, ts, [s + 1] * 200, ivals(rng, 200))
                 for s in range(3)])


# ---- 10. composition ----
def two_parts(rng, n_series=3, n=700, irregular=False, tag_cols=(),
              vers_b="const", vals=ivals, groups=1):
    """Part one: one block per series, version 1.  Part two: per series a
    block re-sending a stretch of those rows plus newer timestamps."""
    first, second = [], []
    for s in range(n_series):
        ts = irregular_ts(rng, n) if irregular else arith_ts(n)
        a = DBlk(s + 1, ts, [1] * n, vals(rng, n),
                 [gen(rng, n) for gen in tag_cols], s % groups)
        lo = rng.randrange(n // 4, n // 2)
        hi = rng.randrange(lo + n // 8, n - 1)
        rows = [r for r in range(lo, hi) if rng.random() < 0.7]
        extra = [ts[-1] + (k + 1) * 7 * MS for k in range(rng.randrange(0, 60))]
        m = len(rows) + len(extra)
        vers = [2] * m if vers_b == "const" else mixed_versions(rng, m)
        b = DBlk(s + 1, [ts[r] for r in rows] + extra, vers, vals(rng, m),
                 [gen(rng, m) for gen in tag_cols], s % groups)
        first.append(a)
        second.append(b)
    return first + second


def clamp_cases():
    out = []
    for irregular in (False, True):
        rng = random.Random(10100 + irregular)
        ts = irregular_ts(rng, 300) if irregular else arith_ts(300)
        a = DBlk(1, ts, [1] * 300, ivals(rng, 300))
        b = resend(rng, a, range(100, 200), mixed_versions(rng, 100))
        # the overlap is rows 100..199 of a
        for name, lo, hi in (("inside", 120, 180), ("on", 100, 199),
                             ("left", 0, 99), ("right", 200, 299),
                             ("across_lo", 50, 150), ("across_hi", 150, 250),
                             ("one_row", 137, 137)):
            tag = "%s_%s" % ("dod" if irregular else "arith", name)
            out.append(("clamp_" + tag, (lambda a=a, b=b, lo=lo, hi=hi:
                                         Scen([a, b], min_ts=a.ts[lo],
                                              max_ts=a.ts[hi]))))
            out.append(("clamp_off_by_one_" + tag,
                        (lambda a=a, b=b, lo=lo, hi=hi:
                         Scen([a, b], min_ts=a.ts[lo] + 1,
                              max_ts=a.ts[hi] - 1 if hi > lo else a.ts[hi]))))
    return out


def uniform_tag_case():
    """Per-block uniform dictionary tag: the filter alone gives CLEAR / SKIP
    verdicts."""
    rng = random.Random(10201)
    blocks = two_parts(rng, n_series=4, n=400)
    for b in blocks:
        b.tags = [[rng.choice(ENVS[:3])] * len(b.ts)]
    return Scen(blocks, conds=[TagCond(0, OP_EQ, [b"prod"])])


def equality_pred_case():
    rng = random.Random(10202)
    return Scen(two_parts(rng, tag_cols=(env_runs,)), pred=b"prod")


def mask_walker_case():
    rng = random.Random(10203)
    return Scen(two_parts(rng, tag_cols=(env_runs,), vers_b="mixed"),
                conds=[TagCond(0, OP_IN, [b"prod", b"qa"])])


def plain_tag_case():
    rng = random.Random(10204)
    return Scen(two_parts(rng, n=900, tag_cols=(plain_col,)),
                conds=[TagCond(0, OP_GE, [b"u3"])])


def three_slot_case():
    rng = random.Random(10205)
    return Scen(two_parts(rng, n=900, vers_b="mixed",
                          tag_cols=(env_runs, plain_col, code_runs)),
                conds=[TagCond(0, OP_NE, [b"dev"]),
                       TagCond(1, OP_GE, [b"u2"]),
                       TagCond(2, OP_GE, [404], TAG_INT)])


def or_tree_case():
    rng = random.Random(10206)
    return Scen(two_parts(rng, tag_cols=(env_runs, code_runs)),
                tree=Or(TagCond(0, OP_EQ, [b"prod"]),
                        TagCond(1, OP_EQ, [404], TAG_INT)))


def block_groups_case():
    rng = random.Random(10207)
    return Scen(two_parts(rng, n_series=6, n=300, groups=3),
                group=("code", 3))


def tag_group_case():
    rng = random.Random(10208)
    return Scen(two_parts(rng, tag_cols=(env_runs,), vers_b="mixed"),
                group=("tag", 0, ENVS))


def tag_group_filter_case():
    rng = random.Random(10209)
    return Scen(two_parts(rng, tag_cols=(env_runs, code_runs)),
                conds=[TagCond(1, OP_GE, [404], TAG_INT)],
                group=("tag", 0, ENVS))


def float_case():
    rng = random.Random(10210)
    return Scen(two_parts(rng, vals=fvals, vers_b="mixed"), kind=F64)


def _nullable(gen):
    def vals(rng, n):
        return [None if rng.random() < 0.3 else v for v in gen(rng, n)]
    return vals


def nullable_i64_case():
    rng = random.Random(10211)
    return Scen(two_parts(rng, vals=_nullable(ivals)), kind=I64N)


def nullable_f64_case():
    rng = random.Random(10212)
    return Scen(two_parts(rng, vals=_nullable(fvals)), kind=F64N)


CASES = []
for _n in ROW_COUNTS:
    CASES.append(("identical_%d_high_first" % _n, identical_case(_n, True)))
    CASES.append(("identical_%d_high_second" % _n, identical_case(_n, False)))
CASES += [
    ("middle_third", middle_third_case),
    ("straddle_end", straddle_end_case),
    ("interleaved_none_equal", interleaved_case),
    ("three_versions", three_versions_case),
    ("varying_versions", varying_versions_case),
    ("arith1_x_arith3", encoding_pair_case("arith1", "arith3", 9501)),
    ("arith3_x_arith1", encoding_pair_case("arith3", "arith1", 9502)),
    ("dod_x_arith1", encoding_pair_case("dod", "arith1", 9503)),
    ("arith1_x_dod", encoding_pair_case("arith1", "dod", 9504)),
    ("dod_x_dod", encoding_pair_case("dod", "dod", 9505)),
    ("delta_x_arith1", encoding_pair_case("delta", "arith1", 9506)),
    ("dod_x_delta", encoding_pair_case("dod", "delta", 9507)),
    ("delta_x_delta", encoding_pair_case("delta", "delta", 9508)),
    ("one_row_x_arith", one_row_case("arith1", 9511)),
    ("one_row_x_dod", one_row_case("dod", 9512)),
    ("one_row_x_delta", one_row_case("delta", 9513)),
    ("varint_two_byte", wide_varint_case("two_byte", 9521)),
    ("varint_mixed", wide_varint_case("mixed", 9522)),
    ("varint_wide", wide_varint_case("wide", 9523)),
    ("varint_ten_byte", wide_varint_case("ten_byte", 9524)),
    ("different_series", different_series_case),
]
CASES += clamp_cases()
CASES += [
    ("uniform_tag_clear_skip", uniform_tag_case),
    ("equality_pred", equality_pred_case),
    ("mask_walker", mask_walker_case),
    ("plain_tag", plain_tag_case),
    ("three_slots", three_slot_case),
    ("or_tree_row_bitmap", or_tree_case),
    ("block_code_groups", block_groups_case),
    ("tag_group", tag_group_case),
    ("tag_group_filter", tag_group_filter_case),
    ("float64", float_case),
    ("nullable_i64", nullable_i64_case),
    ("nullable_f64", nullable_f64_case),
]
CASE_IDS = [c[0] for c in CASES]
# cases in which, by construction, nothing is superseded
NOTHING_DROPPED = ("interleaved_none_equal", "different_series")


# ---- 14. seeded random leg ----
RANDOM_SEEDS = tuple(range(7000, 7040))


def random_scenario(seed):
    """2-4 parts over 1-6 series, random timestamp / version encodings and
    an optional filter, clamp, tree or grouping.  Series 1 always re-sends
    a strict subset of its first block at a higher version, so at least
    one row is dropped and at least one block is partial."""
    rng = random.Random(seed)
    n_parts = rng.randint(2, 4)
    n_series = rng.randint(1, 6)
    axes = []
    for _ in range(n_series):
        n = rng.randint(40, 500)
        axes.append(irregular_ts(rng, n) if rng.random() < 0.5
                    else arith_ts(n, step=rng.choice([1, 3]) * MS))
    blocks = []
    for part in range(n_parts):
        for s in range(n_series):
            ts = axes[s]
            if part == 0:
                rows = list(range(len(ts)))
            elif part == 1 and s == 0:
                rows = sorted(rng.sample(range(len(ts)),
                                         rng.randint(1, len(ts) - 1)))
            elif rng.random() < 0.7:
                lo = rng.randrange(len(ts))
                hi = rng.randint(lo + 1, len(ts))
                rows = [r for r in range(lo, hi) if rng.random() < 0.8] \
                    or [lo]
            else:
                continue
            m = len(rows)
            how = rng.choice(["const", "mixed", "rising"])
            if part == 1 and s == 0:
                vers = [10 ** 6] * m
            elif how == "const" or m < 4:
                vers = [rng.randint(0, 3)] * m
            elif how == "mixed":
                vers = mixed_versions(rng, m)
            else:
                vers = rising_versions(rng, m)
            blocks.append(DBlk(s + 1, [ts[r] for r in rows], vers,
                               ivals(rng, m),
                               [env_runs(rng, m), code_runs(rng, m)],
                               s % 3,
                               raw_delta_ts=(rng.random() < 0.2 and m > 2)))
    scen = Scen(blocks)
    opt = rng.choice(["none", "filter", "clamp", "tree", "code", "tag",
                      "tag_filter"])
    if opt in ("filter", "tag_filter"):
        scen.conds = [TagCond(1, OP_GE, [404], TAG_INT)]
    if opt == "tree":
        scen.tree = Or(TagCond(0, OP_EQ, [b"prod"]),
                       TagCond(1, OP_EQ, [404], TAG_INT))
    if opt == "clamp" or rng.random() < 0.3:
        ts = axes[0]
        a, b = sorted((rng.randrange(len(ts)), rng.randrange(len(ts))))
        scen.min_ts, scen.max_ts = ts[a], ts[b]
    if opt == "code":
        scen.group = ("code", 3)
    else:
        for b in blocks:        # block group codes need a session with groups
            b.group_code = 0
    if opt in ("tag", "tag_filter"):
        scen.group = ("tag", 0, ENVS)
    return scen


# ---- 15. the golden vectors as parts ----
def golden_blocks(inputs, parts):
    """One block per (part, series) of the named inputs, in part order;
    group code = series - 1, a missing intField is a null."""
    blocks = []
    for name in parts:
        for row in inputs[name]:
            blocks.append(DBlk(row["series"], [row["ts"]], [row["version"]],
                               [row["intField"]],
                               group_code=row["series"] - 1))
    return blocks
