"""Scenario builders shared by the CPU and GPU tag-filter tests.  Every
scenario keeps the rows it generated, so the reference side is folded by
filter_ref from those rows — the oracle knows equality only."""
import random

from banyandb_amd import (PartBuilder, TagCond, i64_tag_cell, OP_EQ, OP_NE,
                          OP_LT, OP_GT, OP_LE, OP_GE, OP_IN, OP_NOT_IN,
                          TAG_STRING, TAG_INT, INT64_MAX)

T0 = 1_700_000_000_000_000_000
MS = 10 ** 6
ENVS = [b"prod", b"dev", b"staging", b"qa"]
CODES = [-300, -5, 0, 7, 200, 404, 500, 503]
SVCS = [b"service_%03d" % i for i in range(256)]  # zstd'd dict sections

PARTIAL, ALL, NONE = "partial", "all", "none"


class Blk:
    def __init__(self, sid, ts, vals, tags):
        self.sid, self.ts, self.vals, self.tags = sid, ts, vals, tags


class Scenario:
    def __init__(self, blocks, conds, min_ts=None, max_ts=None,
                 float_vals=False):
        self.blocks = blocks
        self.conds = conds
        self.min_ts = min_ts
        self.max_ts = max_ts
        self.float_vals = float_vals

    @property
    def n_rows(self):
        return sum(len(b.ts) for b in self.blocks)

    def builder(self):
        pb = PartBuilder()
        for b in self.blocks:
            add = pb.add_block_f64 if self.float_vals else pb.add_block_i64
            add(b.sid, b.ts, [1] * len(b.ts), b.vals)
            for col in b.tags:
                pb.set_block_tag(col)
        return pb


def icell(v):
    return i64_tag_cell(v)


def runs(rng, n, choices, maxrun=120, nil_p=0.0):
    out = []
    while len(out) < n:
        run = min(rng.randint(1, maxrun), n - len(out))
        v = None if rng.random() < nil_p else choices[rng.randrange(len(choices))]
        out.extend([v] * run)
    return out


def ts_of(n):
    return [T0 + i * MS for i in range(n)]


def ivals(rng, n):
    return [rng.randint(-10 ** 9, 10 ** 9) for _ in range(n)]


def rowvary(rng, choices, n_series=4, n=1500, nil_p=0.12):
    return [Blk(sid + 1, ts_of(n), ivals(rng, n),
                [runs(rng, n, choices, nil_p=nil_p)])
            for sid in range(n_series)]


# ---- per-operator cases on a row-varying dictionary tag with nil runs ----
STR_OPS = [
    ("eq", OP_EQ, [b"prod"]), ("ne", OP_NE, [b"prod"]),
    ("lt", OP_LT, [b"prod"]), ("le", OP_LE, [b"prod"]),
    ("gt", OP_GT, [b"prod"]), ("ge", OP_GE, [b"prod"]),
    ("in", OP_IN, [b"dev", b"qa", b"absent"]),
    ("not_in", OP_NOT_IN, [b"dev", b"qa", b"absent"]),
]
INT_OPS = [
    ("eq", OP_EQ, [404]), ("ne", OP_NE, [404]),
    ("lt", OP_LT, [7]), ("le", OP_LE, [7]),
    ("gt", OP_GT, [200]), ("ge", OP_GE, [200]),
    ("in", OP_IN, [-5, 500, 999]), ("not_in", OP_NOT_IN, [-5, 500, 999]),
]


def str_op_case(seed, op, lits):
    def make():
        rng = random.Random(seed)
        return Scenario(rowvary(rng, ENVS), [TagCond(0, op, lits)])
    return make


def int_op_case(seed, op, lits):
    def make():
        rng = random.Random(seed)
        return Scenario(rowvary(rng, [icell(c) for c in CODES]),
                        [TagCond(0, op, lits, TAG_INT)])
    return make


def wrapped_case():
    # GT MaxInt64 selects exactly the values more than 2^63 below it: the
    # reference's wrapped int64 subtraction (expr_literal.go:65-70)
    rng = random.Random(1201)
    cells = [icell(v) for v in (-2, 5, -100, 3, INT64_MAX)]
    return Scenario(rowvary(rng, cells),
                    [TagCond(0, OP_GT, [INT64_MAX], TAG_INT)])


# ---- dictionary sizes at mask word boundaries ----
def dict_values(card):
    if card <= 65:      # 1-byte values keep the sections plain-framed
        return [bytes([33 + i]) for i in range(card)]
    return [icell(i) for i in range(card)]


def dict_edge_part(rng, card, n=1500):
    vals = dict_values(card)
    blocks = []
    for sid in range(2):
        # first-seen order == value order, so dict code == value index
        col = list(vals) + runs(rng, n - card, vals, maxrun=6)
        blocks.append(Blk(sid + 1, ts_of(n), ivals(rng, n), [col]))
    return blocks, vals


def dict_range_case(card):
    def make():
        rng = random.Random(1300 + card)
        blocks, vals = dict_edge_part(rng, card)
        # codes lo..hi straddle a 64-bit mask word boundary
        lo, hi = {65: (58, 64), 129: (120, 128), 256: (185, 200)}[card]
        tt = TAG_STRING if card <= 65 else TAG_INT
        return Scenario(blocks, [TagCond(0, OP_GE, [vals[lo]], tt),
                                 TagCond(0, OP_LE, [vals[hi]], tt)])
    return make


def dict_in_case(card):
    def make():
        rng = random.Random(1400 + card)
        blocks, vals = dict_edge_part(rng, card)
        tt = TAG_STRING if card <= 65 else TAG_INT
        return Scenario(blocks, [TagCond(0, OP_IN, [vals[0], vals[-1]], tt)])
    return make


def zstd_dict_case(op, lits):
    def make():
        rng = random.Random(1500 + op)
        blocks = [Blk(sid + 1, ts_of(2500), ivals(rng, 2500),
                      [runs(rng, 2500, SVCS, maxrun=40)]) for sid in range(3)]
        conds = [TagCond(0, op, [lits[0]])]
        if len(lits) > 1:
            conds.append(TagCond(0, OP_LT, [lits[1]]))
        return Scenario(blocks, conds)
    return make


# ---- plain (>256-distinct) columns ----
def plain_col(rng, n):
    """> 256 distinct values, mixed lengths, empty strings and nils."""
    col = []
    for i in range(n):
        r = rng.random()
        if i < 270:
            col.append(b"u%d" % i)          # 270 distinct: plain for sure
        elif r < 0.10:
            col.append(None)
        elif r < 0.18:
            col.append(b"")
        else:
            col.append(b"u%d" % rng.randrange(400))
    rng.shuffle(col)
    return col


def plain_blocks(rng):
    return [Blk(i + 1, ts_of(n), ivals(rng, n), [plain_col(rng, n)])
            for i, n in enumerate((321, 3000, 1000))]


PLAIN_OPS = [
    ("ne", OP_NE, [b"u7"]), ("in", OP_IN, [b"u1", b"u22", b"u333", b""]),
    ("not_in", OP_NOT_IN, [b"u1", b"u22", b"u333", b""]),
    ("ge", OP_GE, [b"u3"]), ("lt", OP_LT, [b"u3"]),
]


def plain_case(seed, op, lits):
    def make():
        rng = random.Random(seed)
        return Scenario(plain_blocks(rng), [TagCond(0, op, lits)])
    return make


# ---- combinations ----
def closed_open_case():
    rng = random.Random(1701)
    return Scenario(rowvary(rng, [icell(c) for c in CODES]),
                    [TagCond(0, OP_GE, [200], TAG_INT),
                     TagCond(0, OP_LT, [500], TAG_INT)])


def three_slot_case():
    rng = random.Random(1702)
    blocks = []
    for sid in range(3):
        n = 2000
        blocks.append(Blk(sid + 1, ts_of(n), ivals(rng, n), [
            runs(rng, n, ENVS, nil_p=0.1),              # slot 0: dictionary
            plain_col(rng, n),                          # slot 1: plain
            runs(rng, n, [icell(c) for c in CODES], maxrun=60),  # slot 2
        ]))
    return Scenario(blocks, [TagCond(0, OP_NE, [b"dev"]),
                             TagCond(1, OP_GE, [b"u2"]),
                             TagCond(2, OP_IN, [200, 404, 503], TAG_INT)])


def clamp_case():
    rng = random.Random(1703)
    return Scenario(rowvary(rng, ENVS, n=3000),
                    [TagCond(0, OP_GT, [b"dev"])],
                    min_ts=T0 + 500 * MS, max_ts=T0 + 2500 * MS)


def arith_blocks_case(op, lits):
    def make():
        rng = random.Random(1704)
        n = 1500
        return Scenario([
            Blk(1, ts_of(n), [42] * n, [[ENVS[i % 3] for i in range(n)]]),
            Blk(2, ts_of(n), [7 * i for i in range(n)],
                [[None if (i // 25) % 5 == 4 else ENVS[(i // 10) % 4]
                  for i in range(n)]]),
            Blk(3, ts_of(n), [rng.randint(0, 100) for _ in range(n)],
                [[b"prod"] * n]),
        ], [TagCond(0, op, lits)])
    return make


def float_case():
    rng = random.Random(1705)
    blocks = []
    for sid in range(4):
        n = 2048
        cents = [rng.randint(-10 ** 6, 10 ** 6) for _ in range(n)]
        blocks.append(Blk(sid + 1, ts_of(n), [c / 100.0 for c in cents],
                          [runs(rng, n, [icell(c) for c in CODES],
                                nil_p=0.1)]))
    return Scenario(blocks, [TagCond(0, OP_GE, [200], TAG_INT)],
                    float_vals=True)


# ---- verdict shortcuts ----
def ne_absent_case():
    rng = random.Random(1801)
    return Scenario(rowvary(rng, ENVS), [TagCond(0, OP_NE, [b"absent"])])


def empty_range_case():
    rng = random.Random(1802)
    return Scenario(rowvary(rng, [icell(c) for c in CODES]),
                    [TagCond(0, OP_GT, [503], TAG_INT),
                     TagCond(0, OP_LT, [10 ** 6], TAG_INT)])


def no_column_part(rng):
    n = 1000
    return [Blk(1, ts_of(n), ivals(rng, n), [runs(rng, n, ENVS)]),
            Blk(2, ts_of(n), ivals(rng, n), [])]      # no tag column at all


def no_column_case(op, lits):
    def make():
        return Scenario(no_column_part(random.Random(1803)),
                        [TagCond(0, op, lits)])
    return make


CASES = []
for _i, (_n, _op, _l) in enumerate(STR_OPS):
    CASES.append((f"str_{_n}", str_op_case(1000 + _i, _op, _l), PARTIAL))
for _i, (_n, _op, _l) in enumerate(INT_OPS):
    CASES.append((f"int_{_n}", int_op_case(1100 + _i, _op, _l), PARTIAL))
CASES.append(("int_wrapped_gt", wrapped_case, PARTIAL))
for _c in (65, 129, 256):
    CASES.append((f"dict{_c}_range", dict_range_case(_c), PARTIAL))
    CASES.append((f"dict{_c}_in_first_last", dict_in_case(_c), PARTIAL))
CASES.append(("zstd_dict_range",
              zstd_dict_case(OP_GE, [b"service_100", b"service_140"]),
              PARTIAL))
CASES.append(("zstd_dict_ne", zstd_dict_case(OP_NE, [b"service_007"]),
              PARTIAL))
for _i, (_n, _op, _l) in enumerate(PLAIN_OPS):
    CASES.append((f"plain_{_n}", plain_case(1600 + _i, _op, _l), PARTIAL))
CASES.append(("closed_open_range", closed_open_case, PARTIAL))
CASES.append(("three_slots_dict_plain", three_slot_case, PARTIAL))
CASES.append(("time_clamp", clamp_case, PARTIAL))
CASES.append(("const_deltaconst_ne", arith_blocks_case(OP_NE, [b"prod"]),
              PARTIAL))
CASES.append(("const_deltaconst_range", arith_blocks_case(OP_LE, [b"prod"]),
              PARTIAL))
CASES.append(("float64_range", float_case, PARTIAL))
CASES.append(("ne_absent_multirun", ne_absent_case, ALL))
CASES.append(("range_selects_nothing", empty_range_case, NONE))
CASES.append(("no_column_ne", no_column_case(OP_NE, [b"prod"]), PARTIAL))
CASES.append(("no_column_not_in", no_column_case(OP_NOT_IN, [b"prod", b"qa"]),
              PARTIAL))
CASES.append(("no_column_eq", no_column_case(OP_EQ, [b"prod"]), PARTIAL))
CASE_IDS = [c[0] for c in CASES]


# ---- randomised leg ----
ALL_OPS = [OP_EQ, OP_NE, OP_LT, OP_LE, OP_GT, OP_GE, OP_IN, OP_NOT_IN]


def random_scenario(seed):
    """One scenario over (op, type, dictionary|plain, nil rate, number of
    conditions, clamp), fully determined by the seed."""
    rng = random.Random(seed)
    n_slots = rng.randint(1, 3)
    kinds = []
    for _ in range(n_slots):
        kinds.append((rng.choice(["str", "int"]),
                      rng.choice(["dict", "dict", "plain"]),
                      rng.choice([0.0, 0.1, 0.5])))
    pools = []
    for typ, enc, _ in kinds:
        card = rng.choice([3, 9, 70]) if enc == "dict" else 330
        span = 500 if enc == "dict" else 10 ** 5
        if typ == "int":
            pools.append([icell(rng.randint(-span, span) if rng.random() < 0.9
                                else rng.choice([INT64_MAX, -INT64_MAX - 1]))
                          for _ in range(card)])
        else:
            pools.append([b"v%d" % rng.randrange(10 ** rng.randint(1, 4)
                                                 if enc == "dict" else span)
                          for _ in range(card)] + [b""])
    blocks = []
    for sid in range(rng.randint(1, 3)):
        n = rng.choice([1, 63, 64, 65, 500, 500, 777, 777])
        tags = []
        for (typ, enc, nil_p), pool in zip(kinds, pools):
            if enc == "plain" and n > 300:
                col = [None if rng.random() < nil_p
                       else pool[rng.randrange(len(pool))] for _ in range(n)]
                col[:300] = pool[:300]      # force > 256 distinct
            else:
                col = runs(rng, n, pool, maxrun=rng.choice([1, 8, 200]),
                           nil_p=nil_p)
            tags.append(col)
        if rng.random() < 0.15:
            tags = tags[:rng.randrange(len(tags))]   # drop trailing columns
        blocks.append(Blk(sid + 1, ts_of(n), ivals(rng, n), tags))
    conds = []
    for _ in range(rng.choice([1, 1, 2, 2, 3, 4])):
        sl = rng.randrange(n_slots)
        typ = kinds[sl][0]
        op = rng.choice(ALL_OPS)
        pool = pools[sl]
        nv = rng.randint(1, 5) if op in (OP_IN, OP_NOT_IN) else 1
        lits = [rng.choice(pool) for _ in range(nv)]
        conds.append(TagCond(sl, op, lits,
                             TAG_INT if typ == "int" else TAG_STRING))
    lo = hi = None
    if rng.random() < 0.4:
        lo, hi = T0 + rng.randint(0, 40) * MS, T0 + rng.randint(50, 700) * MS
    return Scenario(blocks, conds, lo, hi)
