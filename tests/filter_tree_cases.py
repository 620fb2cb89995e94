"""Scenario builders shared by the CPU and GPU criteria-tree tests.  Every
scenario keeps the rows it generated, so the reference side is folded by
filter_tree_ref from those rows.

predict_stats restates the resolve stage's verdict table (DESIGN.md,
"criteria trees") over those rows, so a test can assert which path each
block took: [clear, skip, code-mask walk, row-bitmap walk]."""
import itertools
import os
import random
import subprocess

from banyandb_amd import (TagCond, TreeNode, And, Or, NODE_LEAF, NODE_AND,
                          NODE_OR, OP_EQ, OP_NE, OP_LT, OP_LE, OP_GE, OP_IN,
                          OP_NOT_IN, TAG_STRING, TAG_INT, INT64_MAX)

import filter_cases as fc
import filter_ref as fr
import filter_tree_ref as ftr
from filter_cases import (Blk, ENVS, CODES, SVCS, T0, MS, icell, runs, ts_of,
                          ivals, plain_col)

UNIFORM, MASK, ROWS = "uniform", "mask", "rows"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_tree_consumer(exe):
    """Compile tools/cabi_filter_tree_check.c against the header alone."""
    subprocess.run(
        ["gcc", "-std=c99", "-Wall", "-Werror", "-I",
         os.path.join(REPO, "include"),
         os.path.join(REPO, "tools", "cabi_filter_tree_check.c"),
         "-L", os.path.join(REPO, "banyandb_amd"), "-lbydb_gpu",
         "-Wl,-rpath," + os.path.join(REPO, "banyandb_amd"), "-o", exe],
        check=True)


class TreeScenario:
    def __init__(self, blocks, tree, min_ts=None, max_ts=None,
                 float_vals=False, expect=None):
        self.blocks = blocks
        self.tree = tree
        self.min_ts = min_ts
        self.max_ts = max_ts
        self.float_vals = float_vals
        self.expect = expect      # UNIFORM / MASK / ROWS: the path under test

    @property
    def n_rows(self):
        return sum(len(b.ts) for b in self.blocks)

    def builder(self):
        return fc.Scenario(self.blocks, [],
                           float_vals=self.float_vals).builder()


# ---- the verdict table, restated over the generated rows ----
def predict_stats(blocks, tree):
    ls = ftr.leaves(tree)
    if not ftr.has_or(tree):
        return [0, 0, 0, 0]       # delegated to the conjunctive path
    slots = sorted({c.slot for c in ls})
    stats = [0, 0, 0, 0]
    for b in blocks:
        varying = []              # (slot, kind, leaf-result tuples)
        fixed = {}                # id(leaf) -> bool
        for sl in slots:
            mine = [c for c in ls if c.slot == sl]
            col = b.tags[sl] if sl < len(b.tags) else [None]
            distinct = set(col)
            if len(distinct) == 1:      # no column, or a single-run dictionary
                v = next(iter(distinct))
                for c in mine:
                    fixed[id(c)] = fr.match(c.op, c.tag_type, c.values, v)
            elif len(distinct) > 256:   # plain column: any combination
                varying.append((mine, "plain", set(
                    itertools.product([False, True], repeat=len(mine)))))
            else:
                varying.append((mine, "dict", {
                    tuple(fr.match(c.op, c.tag_type, c.values, v)
                          for c in mine) for v in distinct}))
        results = set()
        for combo in itertools.product(*[sorted(v[2]) for v in varying]):
            vals = dict(fixed)
            for (mine, _, _), res in zip(varying, combo):
                for c, r in zip(mine, res):
                    vals[id(c)] = r
            results.add(ftr.evaluate(tree, lambda c: vals[id(c)]))
        if results == {True}:
            stats[0] += 1
        elif results == {False}:
            stats[1] += 1
        elif len(varying) == 1 and varying[0][1] == "dict":
            stats[2] += 1
        else:
            stats[3] += 1
    return stats


def path_taken(stats):
    if stats[3] > 0:
        return ROWS
    if stats[2] > 0:
        return MASK
    return UNIFORM


# ---- tree construction helpers ----
def random_tree(rng, conds):
    """A random binary AND / OR tree over conds, in the given leaf order."""
    if len(conds) == 1:
        return conds[0]
    cut = rng.randint(1, len(conds) - 1)
    return TreeNode(rng.choice([NODE_AND, NODE_OR]),
                    random_tree(rng, conds[:cut]),
                    random_tree(rng, conds[cut:]))


def dummy_conds(n):
    return [TagCond(i % 3, OP_EQ, [b"v%d" % i]) for i in range(n)]


def left_deep(conds, ops):
    node = conds[0]
    for c, op in zip(conds[1:], ops):
        node = TreeNode(op, node, c)
    return node


def right_deep(conds, ops):
    node = conds[-1]
    for c, op in zip(reversed(conds[:-1]), ops):
        node = TreeNode(op, c, node)
    return node


# malformed trees as raw (n_conds, [(op, left, right), ...])
L = NODE_LEAF
MALFORMED = [
    ("condition referenced twice",
     2, [(L, 0, 0), (L, 0, 0), (NODE_OR, 0, 1)]),
    ("condition never referenced",
     2, [(L, 0, 0), (L, 2, 0), (NODE_OR, 0, 1)]),
    ("leaf with a negative condition index",
     2, [(L, 0, 0), (L, -1, 0), (NODE_OR, 0, 1)]),
    ("child above its parent",
     2, [(NODE_OR, 1, 2), (L, 0, 0), (L, 1, 0)]),
    ("node is its own child",
     2, [(L, 0, 0), (L, 1, 0), (NODE_OR, 0, 2)]),
    ("negative child index",
     2, [(L, 0, 0), (L, 1, 0), (NODE_OR, -1, 1)]),
    ("node with two parents",
     3, [(L, 0, 0), (L, 1, 0), (L, 2, 0), (NODE_OR, 0, 1), (NODE_AND, 1, 3)]),
    ("same child twice",
     2, [(L, 0, 0), (L, 1, 0), (NODE_AND, 1, 1)]),
    ("n_nodes too small", 2, [(L, 0, 0), (L, 1, 0)]),
    ("n_nodes too large",
     2, [(L, 0, 0), (L, 1, 0), (NODE_OR, 0, 1), (L, 1, 0)]),
    ("unknown op", 2, [(L, 0, 0), (L, 1, 0), (3, 0, 1)]),
    ("nine leaves", 9,
     [(L, 0, 0)] + [x for i in range(1, 9)
                    for x in ((L, i, 0), (NODE_OR, 2 * i - 2, 2 * i - 1))]),
    ("no conditions but nodes", 0, [(L, 0, 0)]),
]


# ---- parts ----
def two_dict_blocks(rng, sizes, maxrun0, maxrun1, pool0=ENVS, pool1=None,
                    nil_p=0.1):
    pool1 = [icell(c) for c in CODES] if pool1 is None else pool1
    return [Blk(i + 1, ts_of(n), ivals(rng, n),
                [runs(rng, n, pool0, maxrun=maxrun0, nil_p=nil_p),
                 runs(rng, n, pool1, maxrun=maxrun1, nil_p=nil_p)])
            for i, n in enumerate(sizes)]


CROSS_OR = Or(TagCond(0, OP_EQ, [b"prod"]),
              TagCond(1, OP_GE, [404], TAG_INT))


# 1. single-slot OR on a row-varying dictionary with nil runs
def int_or_case():
    rng = random.Random(4101)
    return TreeScenario(
        fc.rowvary(rng, [icell(c) for c in CODES]),
        Or(TagCond(0, OP_EQ, [404], TAG_INT),
           TagCond(0, OP_GE, [500], TAG_INT)), expect=MASK)


def env_or_blocks():
    return fc.rowvary(random.Random(4102), ENVS)


# 2. cross-slot OR over entity tags (one value per block)
def entity_or_case():
    rng = random.Random(4201)
    n = 1500
    blocks = [Blk(i + 1, ts_of(n), ivals(rng, n),
                  [[ENVS[i % 4]] * n, [SVCS[i % 3]] * n]) for i in range(4)]
    return TreeScenario(blocks, Or(TagCond(0, OP_EQ, [b"dev"]),
                                   TagCond(1, OP_EQ, [SVCS[2]])),
                        expect=UNIFORM)


# 3. one uniform slot, one row-varying dictionary slot: the mask walker
def uniform_plus_varying_case():
    rng = random.Random(4301)
    n = 2000
    blocks = [Blk(i + 1, ts_of(n), ivals(rng, n),
                  [[ENVS[i % 4]] * n,
                   runs(rng, n, [icell(c) for c in CODES], nil_p=0.1)])
              for i in range(4)]
    return TreeScenario(blocks, CROSS_OR, expect=MASK)


# 4. cross-slot OR over two row-varying dictionary slots: row bitmaps
EDGE_SIZES = [1, 63, 64, 65, 777, 8192]


def two_slot_edges_case(maxrun):
    def make():
        rng = random.Random(4400 + maxrun)
        return TreeScenario(
            two_dict_blocks(rng, EDGE_SIZES, maxrun, maxrun), CROSS_OR,
            expect=ROWS)
    return make


def big_dict_case():
    """A full 256-value dictionary (zstd'd sections) on slot 1; the leaves
    on it select codes 192..253 and 255 — the fourth 64-entry word of the
    signature table and the last code the dictionary defines."""
    rng = random.Random(4450)
    blocks = []
    for sid, n in enumerate((2000, 2500)):
        # every value first, in order: the dictionary holds all 256 and
        # dict code == value index
        blocks.append(Blk(sid + 1, ts_of(n), ivals(rng, n), [
            runs(rng, n, ENVS, maxrun=8, nil_p=0.05),
            list(SVCS) + runs(rng, n - 256, SVCS, maxrun=40)]))
    tree = Or(TagCond(0, OP_EQ, [b"prod"]),
              And(TagCond(1, OP_GE, [SVCS[192]]),
                  TagCond(1, OP_NE, [SVCS[254]])))
    return TreeScenario(blocks, tree, expect=ROWS)


def dict_boundary_case():
    """65- and 129-value dictionaries: the selected codes 64 and 120..128
    sit across a 64-entry word boundary of the mask / signature table."""
    rng = random.Random(4460)
    n = 1500
    v65, v129 = fc.dict_values(65), fc.dict_values(129)
    blocks = []
    for sid in range(2):
        # first-seen order == value order, so dict code == value index
        blocks.append(Blk(sid + 1, ts_of(n), ivals(rng, n), [
            list(v65) + runs(rng, n - 65, v65, maxrun=6),
            list(v129) + runs(rng, n - 129, v129, maxrun=6)]))
    tree = Or(TagCond(0, OP_IN, [v65[0], v65[64]]),
              And(TagCond(1, OP_GE, [v129[120]], TAG_INT),
                  TagCond(1, OP_LE, [v129[128]], TAG_INT)))
    return TreeScenario(blocks, tree, expect=ROWS)


# 5. plain columns
def plain_alone_case():
    rng = random.Random(4501)
    return TreeScenario(fc.plain_blocks(rng),
                        Or(TagCond(0, OP_EQ, [b""]),
                           TagCond(0, OP_GE, [b"u3"])), expect=ROWS)


def dict_or_plain_case():
    rng = random.Random(4502)
    blocks = [Blk(i + 1, ts_of(n), ivals(rng, n),
                  [runs(rng, n, ENVS, nil_p=0.1), plain_col(rng, n)])
              for i, n in enumerate((2000, 1700))]
    return TreeScenario(blocks, Or(TagCond(0, OP_EQ, [b"prod"]),
                                   TagCond(1, OP_IN, [b"u1", b"u22", b""])),
                        expect=ROWS)


# 6. three slots
def three_slot_case():
    blocks = fc.three_slot_case().blocks     # dict, plain, dict
    tree = Or(And(TagCond(0, OP_EQ, [b"prod"]), TagCond(1, OP_GE, [b"u2"])),
              TagCond(2, OP_IN, [200, 503], TAG_INT))
    return TreeScenario(blocks, tree, expect=ROWS)


def _depth3_leaves():
    return (TagCond(0, OP_EQ, [b"prod"]), TagCond(1, OP_EQ, [404], TAG_INT),
            TagCond(0, OP_EQ, [b"qa"]), TagCond(1, OP_EQ, [500], TAG_INT))


def depth3_and_or_case():
    rng = random.Random(4601)
    a, b, c, d = _depth3_leaves()
    return TreeScenario(two_dict_blocks(rng, [2000, 1500, 2500], 30, 30),
                        And(Or(a, b), Or(c, d)), expect=ROWS)


def depth3_or_and_case():
    rng = random.Random(4602)
    a, b, c, d = _depth3_leaves()
    return TreeScenario(two_dict_blocks(rng, [2000, 1500, 2500], 30, 30),
                        Or(And(a, b), And(c, d)), expect=ROWS)


def eight_leaf_case():
    rng = random.Random(4603)
    n = 2000
    blocks = [Blk(sid + 1, ts_of(n), ivals(rng, n), [
        runs(rng, n, ENVS, nil_p=0.1),
        runs(rng, n, [icell(c) for c in CODES], maxrun=60, nil_p=0.1),
        runs(rng, n, SVCS[:40], maxrun=25)]) for sid in range(3)]
    tree = Or(And(TagCond(0, OP_NE, [b"dev"]),
                  TagCond(1, OP_GE, [200], TAG_INT),
                  TagCond(1, OP_LT, [500], TAG_INT)),
              And(TagCond(2, OP_GE, [b"service_030"]),
                  Or(TagCond(0, OP_EQ, [b"qa"]),
                     TagCond(1, OP_NOT_IN, [0, 7, 404], TAG_INT))),
              And(TagCond(2, OP_IN, [SVCS[1], SVCS[2], SVCS[3]]),
                  TagCond(0, OP_LE, [b"prod"])))
    assert len(ftr.leaves(tree)) == 8
    return TreeScenario(blocks, tree, expect=ROWS)


# 7. blocks without the column
def missing_column_blocks():
    rng = random.Random(4701)
    n = 1500
    return [Blk(1, ts_of(n), ivals(rng, n),
                [runs(rng, n, ENVS, nil_p=0.1),
                 runs(rng, n, [icell(c) for c in CODES])]),
            Blk(2, ts_of(n), ivals(rng, n),
                [runs(rng, n, ENVS, nil_p=0.1)])]   # no slot-1 column


def missing_column_case(op, lits):
    def make():
        return TreeScenario(missing_column_blocks(),
                            Or(TagCond(1, op, lits, TAG_INT),
                               TagCond(0, OP_EQ, [b"prod"])))
    return make


# 8. composition over a row-bitmap tree
def clamp_case():
    rng = random.Random(4801)
    return TreeScenario(two_dict_blocks(rng, [3000, 3000], 40, 40), CROSS_OR,
                        min_ts=T0 + 500 * MS, max_ts=T0 + 2500 * MS,
                        expect=ROWS)


def arith_blocks_case():
    """Const and DeltaConst field blocks (the values of
    filter_cases.arith_blocks_case) under two row-varying slots."""
    rng = random.Random(4802)
    n = 1500
    fields = [[42] * n, [7 * i for i in range(n)],
              [rng.randint(0, 100) for _ in range(n)]]
    blocks = [Blk(i + 1, ts_of(n), f,
                  [runs(rng, n, ENVS, maxrun=25, nil_p=0.1),
                   runs(rng, n, [icell(c) for c in CODES], maxrun=10)])
              for i, f in enumerate(fields)]
    return TreeScenario(blocks, CROSS_OR, expect=ROWS)


def float_case():
    rng = random.Random(4803)
    blocks = []
    for sid in range(3):
        n = 2048
        cents = [rng.randint(-10 ** 6, 10 ** 6) for _ in range(n)]
        blocks.append(Blk(sid + 1, ts_of(n), [c / 100.0 for c in cents],
                          [runs(rng, n, ENVS, nil_p=0.1),
                           runs(rng, n, [icell(c) for c in CODES],
                                nil_p=0.1)]))
    return TreeScenario(blocks, CROSS_OR, float_vals=True, expect=ROWS)


def grouped_case():
    rng = random.Random(4804)
    return TreeScenario(two_dict_blocks(rng, [2000, 2000, 1500], 50, 70),
                        CROSS_OR, expect=ROWS)


CASES = [
    ("int_eq_or_ge", int_or_case),
    ("entity_tags_cross_slot", entity_or_case),
    ("uniform_slot_or_varying_slot", uniform_plus_varying_case),
    ("two_slots_runs1", two_slot_edges_case(1)),
    ("two_slots_runs8", two_slot_edges_case(8)),
    ("two_slots_runs200", two_slot_edges_case(200)),
    ("two_slots_dict256", big_dict_case),
    ("two_slots_dict65_dict129", dict_boundary_case),
    ("plain_alone", plain_alone_case),
    ("dict_or_plain", dict_or_plain_case),
    ("three_slots_and_or_in", three_slot_case),
    ("depth3_and_or", depth3_and_or_case),
    ("depth3_or_and", depth3_or_and_case),
    ("eight_leaves", eight_leaf_case),
    ("missing_column_ne", missing_column_case(OP_NE, [404])),
    ("missing_column_not_in", missing_column_case(OP_NOT_IN, [404, 500])),
    ("missing_column_eq", missing_column_case(OP_EQ, [404])),
    ("time_clamp", clamp_case),
    ("const_deltaconst_fields", arith_blocks_case),
    ("float64_field", float_case),
]
CASE_IDS = [c[0] for c in CASES]


# ---- randomised leg ----
def scenario_space(seed):
    """The slot kinds and literal pools filter_cases.random_scenario(seed)
    draws: the same first draws from the same generator, so the pools are
    the ones its blocks were filled from."""
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
    return kinds, pools


def random_tree_scenario(seed):
    """random_scenario(seed)'s blocks, pools and clamp under a random tree
    of 1-6 conditions drawn from those pools."""
    base = fc.random_scenario(seed)
    kinds, pools = scenario_space(seed)
    rng = random.Random(seed * 7919 + 17)
    conds = []
    for _ in range(rng.randint(1, 6)):
        sl = rng.randrange(len(kinds))
        op = rng.choice(fc.ALL_OPS)
        nv = rng.randint(1, 5) if op in (OP_IN, OP_NOT_IN) else 1
        lits = [rng.choice(pools[sl]) for _ in range(nv)]
        conds.append(TagCond(sl, op, lits,
                             TAG_INT if kinds[sl][0] == "int" else TAG_STRING))
    return TreeScenario(base.blocks, random_tree(rng, conds), base.min_ts,
                        base.max_ts)


# 40 seeds, chosen on the CPU by scanning 5000.. in order and passing over
# a seed once 8 seeds that select no row or every row (by the reference), or
# 5 seeds whose tree has no OR node, were already taken: at most a quarter
# are trivial, and 18 have a row-bitmap block by predict_stats.
RANDOM_SEEDS = [
    5000, 5001, 5002, 5003, 5004, 5005, 5006, 5007, 5008, 5009,
    5010, 5011, 5012, 5013, 5014, 5015, 5016, 5018, 5019, 5020,
    5022, 5023, 5024, 5025, 5028, 5031, 5032, 5034, 5035, 5038,
    5039, 5044, 5046, 5050, 5054, 5056, 5057, 5058, 5060, 5062,
]
