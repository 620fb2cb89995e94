"""CPU checks for AND / OR criteria trees: the tree evaluator
(tests/filter_tree_ref.py) against the reference's own measure cases
(tests/golden/tag_filter_tree_vectors.json), the host truth-table builder
bydb_filter_tree_table against the evaluator, the tree validation rules,
the pure-C consumer, and the non-vacuity of the GPU cases."""
import ctypes
import json
import os
import random

import pytest

import banyandb_amd as ba
from banyandb_amd import (TagCond, TreeNode, And, Or, NODE_AND, NODE_OR,
                          OP_EQ, OP_NE, OP_LT, OP_GT, OP_LE, OP_GE, OP_IN,
                          OP_NOT_IN)
import filter_cases as fc
import filter_ref as fr
import filter_tree_cases as ftc
import filter_tree_ref as ftr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "tag_filter_tree_vectors.json")
OPS = {"EQ": OP_EQ, "NE": OP_NE, "LT": OP_LT, "LE": OP_LE, "GT": OP_GT,
       "GE": OP_GE, "IN": OP_IN, "NOT_IN": OP_NOT_IN}
BAD_ARG = -3


def _golden():
    return json.load(open(GOLDEN))


def _tree(node, tags):
    if "tag" in node:
        return TagCond(tags.index(node["tag"]), OPS[node["op"]],
                       [node["value"].encode()])
    op = {"AND": NODE_AND, "OR": NODE_OR}[node["op"]]
    return TreeNode(op, _tree(node["left"], tags), _tree(node["right"], tags))


def golden_trees():
    g = _golden()
    return [(c["name"], _tree(c["criteria"], g["tags"])) for c in g["cases"]]


def test_golden_file_holds_the_five_reference_cases():
    g = _golden()
    assert [c["name"] for c in g["cases"]] == [
        "linked_or", "complex_and_or", "gen_tree_depth2_or",
        "gen_tree_depth3_and_or", "gen_tree_depth3_or_and"]
    assert len(g["rows"]) == 6
    want = {c["name"]: c["want_rows"] for c in g["cases"]}
    ents = [r["entity_id"] for r in g["rows"]]
    assert [ents[i] for i in want["linked_or"]] == ["entity_4", "entity_5"]
    assert [(g["rows"][i]["id"], ents[i]) for i in want["complex_and_or"]] \
        == [("svc1", "entity_1"), ("svc3", "entity_6")]


def test_evaluator_reproduces_every_golden_vector():
    g = _golden()
    for case in g["cases"]:
        tree = _tree(case["criteria"], g["tags"])
        got = [i for i, r in enumerate(g["rows"]) if ftr.row_selected(
            tree, [r[t].encode() for t in g["tags"]])]
        assert got == sorted(case["want_rows"]), case["name"]


def _check_table(tree, what):
    want = ftr.truth_table(tree)
    got = ba.filter_tree_table(tree)
    assert got == want, (what, hex(got), hex(want))
    n = len(ftr.leaves(tree))
    assert got >> (1 << n) == 0, what      # no bit above 2^n_conds


def test_table_equals_evaluator_on_golden_trees():
    for name, tree in golden_trees():
        _check_table(tree, name)


def test_table_equals_evaluator_on_random_trees():
    rng = random.Random(6001)
    sizes = set()
    for i in range(200):
        n = rng.randint(1, 8)
        sizes.add(n)
        _check_table(ftc.random_tree(rng, ftc.dummy_conds(n)), f"tree {i}")
    assert sizes == set(range(1, 9))


def test_table_of_single_leaf_and_deep_chains():
    _check_table(TagCond(0, OP_EQ, [b"x"]), "single leaf")
    assert ba.filter_tree_table(TagCond(0, OP_EQ, [b"x"])) == 0b10
    rng = random.Random(6002)
    for _ in range(8):
        ops = [rng.choice([NODE_AND, NODE_OR]) for _ in range(7)]
        _check_table(ftc.left_deep(ftc.dummy_conds(8), ops), ("left", ops))
        _check_table(ftc.right_deep(ftc.dummy_conds(8), ops), ("right", ops))
    # the n-ary helpers fold left, as isMatch merges its sub-nodes
    conds = ftc.dummy_conds(8)
    assert ba.filter_tree_table(Or(*conds)) == \
        ftr.truth_table(ftc.left_deep(conds, [NODE_OR] * 7)) == \
        (1 << 256) - 2
    assert ba.filter_tree_table(And(*conds)) == 1 << 255


def test_leaf_order_is_condition_order():
    """A tree whose post-order visits conditions out of index order: the
    table's bit i must follow condition i, not visit order."""
    # conds 0, 1, 2; tree = c2 AND (c0 OR c1), written by hand in post-order
    nodes = [(0, 2, 0), (0, 0, 0), (0, 1, 0), (NODE_OR, 1, 2),
             (NODE_AND, 0, 3)]
    want = 0
    for sig in range(8):
        c0, c1, c2 = sig & 1, (sig >> 1) & 1, (sig >> 2) & 1
        if c2 and (c0 or c1):
            want |= 1 << sig
    assert ba.filter_nodes_table(nodes, 3) == want


@pytest.mark.parametrize("what,n_conds,nodes", ftc.MALFORMED,
                         ids=[m[0].replace(" ", "_") for m in ftc.MALFORMED])
def test_malformed_tree_is_bad_arg(what, n_conds, nodes):
    arr = (ba.FilterNodeC * max(len(nodes), 1))(
        *[ba.FilterNodeC(*n) for n in nodes])
    out = (ctypes.c_uint64 * 4)()
    rc = ba.lib().bydb_filter_tree_table(arr, len(nodes), n_conds, out)
    assert rc == BAD_ARG, what


def test_struct_and_exports():
    assert ctypes.sizeof(ba.FilterNodeC) == 12
    lib = ctypes.CDLL(os.path.join(REPO, "banyandb_amd", "libbydb_gpu.so"))
    for sym in ("bydb_consume_filter_tree", "bydb_filter_tree_table",
                "bydb_filter_tree_stats"):
        assert hasattr(lib, sym), sym
    assert (ba.NODE_LEAF, ba.NODE_AND, ba.NODE_OR) == (0, 1, 2)
    assert callable(ba.Session.consume_filter_tree)
    assert callable(ba.Session.filter_tree_stats)


def test_flatten_tree_is_post_order():
    a, b, c = ftc.dummy_conds(3)
    conds, nodes = ba.flatten_tree(Or(And(a, b), c))
    assert conds == [a, b, c]
    assert nodes == [(0, 0, 0), (0, 1, 0), (NODE_AND, 0, 1), (0, 2, 0),
                     (NODE_OR, 2, 3)]
    assert ba.flatten_tree(None) == ([], [])


def test_tree_consumer_compiles_as_c99(tmp_path):
    """tools/cabi_filter_tree_check.c makes one OR-tree scan through the
    header alone; it must build with plain gcc."""
    ftc.build_tree_consumer(str(tmp_path / "cabi_filter_tree_check"))


# ---- the GPU cases, checked by the reference alone ----
@pytest.mark.parametrize("name,make", ftc.CASES, ids=ftc.CASE_IDS)
def test_gpu_cases_are_not_vacuous_and_take_their_path(name, make):
    scen = make()
    sel = ftr.fold(scen.blocks, scen.tree, scen.min_ts, scen.max_ts).count
    total = ftr.fold(scen.blocks, None, scen.min_ts, scen.max_ts).count
    assert 0 < sel < total, (name, sel, total)
    stats = ftc.predict_stats(scen.blocks, scen.tree)
    assert sum(stats) == len(scen.blocks)
    if scen.expect is not None:
        assert ftc.path_taken(stats) == scen.expect, (name, stats)
    assert len(scen.blocks) <= 6
    assert all(len(b.ts) <= 8192 for b in scen.blocks)


def test_edge_size_case_covers_the_bitmap_word_edges():
    for maxrun in (1, 8, 200):
        scen = ftc.two_slot_edges_case(maxrun)()
        assert [len(b.ts) for b in scen.blocks] == [1, 63, 64, 65, 777, 8192]
        # the 8192-row block is a row-bitmap block: all 128 words are used
        assert ftc.predict_stats(scen.blocks[-1:], scen.tree)[3] == 1


def test_dict256_case_fills_the_dictionary_and_selects_its_last_codes():
    scen = ftc.big_dict_case()
    leaves1 = [c for c in ftr.leaves(scen.tree) if c.slot == 1]
    for b in scen.blocks:
        col = b.tags[1]
        assert col[:256] == fc.SVCS and None not in col
        assert len(set(col)) == 256             # dictionary of 256 values
        assert len(b"".join(fc.SVCS)) >= 128    # sections are zstd'd
        # rows past the first 256 carry codes of the last table word,
        # among them code 255 selected and code 254 rejected
        tail = set(col[256:])
        sel = {fc.SVCS.index(v) for v in tail
               if all(fr.match(c.op, c.tag_type, c.values, v)
                      for c in leaves1)}
        assert sel and min(sel) >= 192 and 254 not in sel
    sel_all = {fc.SVCS.index(v) for v in fc.SVCS
               if all(fr.match(c.op, c.tag_type, c.values, v)
                      for c in leaves1)}
    assert sel_all == set(range(192, 254)) | {255}
    assert ftc.predict_stats(scen.blocks, scen.tree) == [0, 0, 0, 2]


def test_missing_column_cases_resolve_as_documented():
    ne = ftc.missing_column_case(OP_NE, [404])()
    eq = ftc.missing_column_case(OP_EQ, [404])()
    bare = ne.blocks[1:]
    # NE on the missing slot is true on nil: the bare block is CLEAR
    assert ftc.predict_stats(bare, ne.tree) == [1, 0, 0, 0]
    assert ftr.fold(bare, ne.tree).count == len(bare[0].ts)
    # EQ on it is false: the tree reduces to the other slot's mask
    assert ftc.predict_stats(bare, eq.tree) == [0, 0, 1, 0]
    assert 0 < ftr.fold(bare, eq.tree).count < len(bare[0].ts)


def test_random_seed_list_keeps_its_cap():
    assert len(ftc.RANDOM_SEEDS) == len(set(ftc.RANDOM_SEEDS)) == 40
    trivial = rows = 0
    for seed in ftc.RANDOM_SEEDS:
        scen = ftc.random_tree_scenario(seed)
        assert 1 <= len(ftr.leaves(scen.tree)) <= 6
        sel = ftr.fold(scen.blocks, scen.tree, scen.min_ts, scen.max_ts).count
        total = ftr.fold(scen.blocks, None, scen.min_ts, scen.max_ts).count
        if sel == 0 or sel == total:
            trivial += 1
        if ftc.predict_stats(scen.blocks, scen.tree)[3] > 0:
            rows += 1
    assert trivial <= 10, trivial
    assert rows >= 10, rows


def test_scenario_space_replays_the_pools_of_random_scenario():
    for seed in ftc.RANDOM_SEEDS:
        kinds, pools = ftc.scenario_space(seed)
        for b in fc.random_scenario(seed).blocks:
            for sl, col in enumerate(b.tags):
                assert {v for v in col if v is not None} <= set(pools[sl]), \
                    (seed, sl)
