"""GPU parity for AND / OR criteria trees (bydb_consume_filter_tree) against
the tree evaluator in tests/filter_tree_ref.py, folded over the rows each
test generated.  int64 sum / count / min / max are bit-exact; float64
checks min / max exactly and the sum to rel 1e-9 (the project's stated
tolerance).  Every case also checks, through filter_tree_stats, which
resolve path its blocks took — against filter_tree_cases.predict_stats, the
verdict table restated over the generated rows."""
import math
import random
import subprocess

import pytest

import banyandb_amd as ba
from banyandb_amd import (Session, TagCond, FilterNodeC, And, Or,
                          VT_INT64, VT_FLOAT64, AGG_SUM, AGG_COUNT, AGG_MIN,
                          AGG_MAX, OP_EQ, OP_NE, OP_GE, OP_IN, TAG_INT,
                          INT64_MIN, INT64_MAX)
import filter_ref as fr
import filter_cases as fc
import filter_tree_cases as ftc
import filter_tree_ref as ftr

pytestmark = pytest.mark.gpu

FUNCS = [AGG_SUM, AGG_COUNT, AGG_MIN, AGG_MAX]
BAD_ARG = -3


def clamp_args(scen):
    return (INT64_MIN if scen.min_ts is None else scen.min_ts,
            INT64_MAX if scen.max_ts is None else scen.max_ts)


def gpu_tree(builder, tree, vtype=VT_INT64, lo=INT64_MIN, hi=INT64_MAX,
             float_exp=0):
    s = Session(0)
    s.upload_part(builder)
    s.configure(vtype, FUNCS, float_exp=float_exp)
    s.consume_filter_tree(tree, lo, hi)
    g = s.finalize()[0]
    stats = s.filter_tree_stats()
    s.close()
    return g, stats


def assert_i64(g, ref, what=""):
    print(what, "gpu", (g.count, g.sum_i), "ref", (ref.count, ref.sum_i))
    assert g.count == ref.count, what
    assert g.sum_i == ref.sum_i, what
    if ref.count:
        assert (g.min_i, g.max_i) == (ref.min, ref.max), what


def assert_stats(stats, scen, what=""):
    want = ftc.predict_stats(scen.blocks, scen.tree)
    print(what, "stats", stats, "predicted", want)
    assert stats == want, what
    if scen.expect is not None:
        assert ftc.path_taken(stats) == scen.expect, what


@pytest.mark.parametrize("name,make", ftc.CASES, ids=ftc.CASE_IDS)
def test_tree_parity(name, make):
    scen = make()
    lo, hi = clamp_args(scen)
    ref = ftr.fold(scen.blocks, scen.tree, scen.min_ts, scen.max_ts)
    b = scen.builder()
    if scen.float_vals:
        g, stats = gpu_tree(b, scen.tree, VT_FLOAT64, lo, hi,
                            float_exp=b.blocks()[0].exp)
        print(name, "gpu", (g.count, g.sum_f), "ref", (ref.count, ref.sum_f))
        assert g.count == ref.count > 0
        assert (g.min_f, g.max_f) == (ref.min, ref.max)
        assert math.isclose(g.sum_f, ref.sum_f, rel_tol=1e-9)
    else:
        g, stats = gpu_tree(b, scen.tree, VT_INT64, lo, hi)
        assert_i64(g, ref, name)
        assert 0 < g.count < scen.n_rows
    assert_stats(stats, scen, name)


# ---- single-slot OR on a row-varying dictionary ----
def test_eq_or_eq_equals_in_bit_for_bit():
    blocks = ftc.env_or_blocks()
    b = fc.Scenario(blocks, []).builder()
    s = Session(0)
    s.upload_part(b)
    s.configure(VT_INT64, FUNCS)
    s.consume_filter([TagCond(0, OP_IN, [b"prod", b"qa"])])
    want = s.finalize_partials()[0]
    s.reset()
    s.consume_filter_tree(Or(TagCond(0, OP_EQ, [b"prod"]),
                             TagCond(0, OP_EQ, [b"qa"])))
    got = s.finalize_partials()[0]
    stats = s.filter_tree_stats()
    s.close()
    assert 0 < want.count < sum(len(blk.ts) for blk in blocks)
    assert (got.sum_i, got.count, got.min_i, got.max_i) == \
        (want.sum_i, want.count, want.min_i, want.max_i)
    assert stats[2] > 0 and stats[3] == 0, stats


def test_ne_or_eq_selects_every_row_nil_included():
    blocks = ftc.env_or_blocks()
    assert any(v is None for blk in blocks for v in blk.tags[0])
    tree = Or(TagCond(0, OP_NE, [b"dev"]), TagCond(0, OP_EQ, [b"dev"]))
    g, stats = gpu_tree(fc.Scenario(blocks, []).builder(), tree)
    assert_i64(g, ftr.fold(blocks, tree), "ne or eq")
    assert g.count == sum(len(blk.ts) for blk in blocks)
    assert stats == [len(blocks), 0, 0, 0], stats


def test_or_of_absent_values_skips_every_block():
    blocks = ftc.env_or_blocks()
    tree = Or(TagCond(0, OP_EQ, [b"absent"]), TagCond(0, OP_EQ, [b"absent2"]))
    g, stats = gpu_tree(fc.Scenario(blocks, []).builder(), tree)
    assert g.count == 0
    assert stats == [0, len(blocks), 0, 0], stats


# ---- grouped sessions over a row-bitmap tree ----
def test_grouped_by_tag_on_a_row_varying_slot():
    scen = ftc.grouped_case()
    domain = [b"prod", b"dev", b"qa"]
    s = Session(0)
    s.upload_part(scen.builder())
    s.configure_by_tag(VT_INT64, FUNCS, 0, domain)
    s.consume_filter_tree(scen.tree)
    gs = s.finalize()
    stats = s.filter_tree_stats()
    s.close()
    refs = ftr.fold_by_tag(scen.blocks, scen.tree, 0, domain)
    unfiltered = ftr.fold_by_tag(scen.blocks, None, 0, domain)
    assert 0 < sum(r.count for r in refs) < sum(r.count for r in unfiltered)
    for gi, (g, ref) in enumerate(zip(gs, refs)):
        assert_i64(g, ref, f"group {gi}")
    assert_stats(stats, scen, "by_tag")


def test_grouped_by_two_tags():
    scen = ftc.grouped_case()
    domains = [[b"prod", b"dev", b"qa"],
               [fc.icell(c) for c in (200, 404, 500, 503)]]
    s = Session(0)
    s.upload_part(scen.builder())
    s.configure_by_tags(VT_INT64, FUNCS, [0, 1], domains)
    s.consume_filter_tree(scen.tree)
    gs = s.finalize()
    stats = s.filter_tree_stats()
    s.close()
    refs = ftr.fold_by_tags(scen.blocks, scen.tree, [0, 1], domains)
    assert len(gs) == len(refs) == 12
    assert sum(1 for r in refs if r.count) >= 6
    for gi, (g, ref) in enumerate(zip(gs, refs)):
        assert_i64(g, ref, f"group {gi}")
    assert_stats(stats, scen, "by_tags")


# ---- a tree with no OR node is the conjunctive path ----
def test_and_tree_equals_consume_filter():
    scen = fc.three_slot_case()          # dictionary, plain, dictionary
    b = scen.builder()
    s = Session(0)
    s.upload_part(b)
    s.configure(VT_INT64, FUNCS)
    s.consume_filter(scen.conds)
    want = s.finalize_partials()[0]
    for tree in (And(*scen.conds),
                 And(scen.conds[0], And(scen.conds[1], scen.conds[2]))):
        s.reset()
        s.consume_filter_tree(tree)
        got = s.finalize_partials()[0]
        assert want.count > 0
        assert (got.sum_i, got.count, got.min_i, got.max_i) == \
            (want.sum_i, want.count, want.min_i, want.max_i)
        assert s.filter_tree_stats() == [0, 0, 0, 0]
    # a bare leaf and the empty tree
    s.reset()
    s.consume_filter_tree(scen.conds[0])
    assert_i64(s.finalize()[0], fr.fold(scen.blocks, scen.conds[:1]), "leaf")
    s.reset()
    s.consume_filter_tree(None)
    assert s.finalize()[0].count == scen.n_rows
    assert s.filter_tree_stats() == [0, 0, 0, 0]
    s.close()


def test_stats_reset_between_calls_and_arena_is_kept():
    """A row-bitmap consume, a conjunctive one, then a larger row-bitmap
    part on the same session: stats follow the last tree call and the
    bitmap arena grows with the census."""
    small = ftc.grouped_case()
    s = Session(0)
    s.upload_part(small.builder())
    s.configure(VT_INT64, FUNCS)
    s.consume_filter_tree(small.tree)
    assert_i64(s.finalize()[0], ftr.fold(small.blocks, small.tree), "small")
    assert s.filter_tree_stats()[3] == len(small.blocks)
    s.reset()
    s.consume_filter_tree(And(*ftr.leaves(small.tree)))
    s.finalize()
    assert s.filter_tree_stats() == [0, 0, 0, 0]
    big = ftc.TreeScenario(
        ftc.two_dict_blocks(random.Random(4901), [700] * 6, 20, 20),
        small.tree)
    s.upload_part(big.builder())
    s.configure(VT_INT64, FUNCS)
    for _ in range(2):      # second pass reuses the grown arena
        s.reset()
        s.consume_filter_tree(big.tree)
        assert_i64(s.finalize()[0], ftr.fold(big.blocks, big.tree), "big")
        assert s.filter_tree_stats()[3] == 6
    s.close()


# ---- error contract ----
def test_malformed_trees_are_bad_arg_and_session_survives():
    scen = ftc.grouped_case()
    want = ftr.fold(scen.blocks, scen.tree)
    s = Session(0)
    s.upload_part(scen.builder())
    s.configure(VT_INT64, FUNCS)
    lib = ba.lib()
    for what, n_conds, nodes in ftc.MALFORMED:
        conds, keep = ba._conds_c(ftc.dummy_conds(n_conds))
        arr = (FilterNodeC * max(len(nodes), 1))(
            *[FilterNodeC(*n) for n in nodes])
        rc = lib.bydb_consume_filter_tree(s._h, INT64_MIN, INT64_MAX, conds,
                                          n_conds, arr, len(nodes))
        assert rc == BAD_ARG, what
        assert lib.bydb_last_error(s._h), what
        # still usable: the next good call folds the right answer
        s.reset()
        s.consume_filter_tree(scen.tree)
        assert_i64(s.finalize()[0], want, f"after {what}")
    # a bad leaf is rejected by the rules of consume_filter
    s.reset()
    with pytest.raises(RuntimeError):
        s.consume_filter_tree(Or(TagCond(0, OP_IN, []),
                                 TagCond(1, OP_GE, [404], TAG_INT)))
    s.consume_filter_tree(scen.tree)
    assert_i64(s.finalize()[0], want, "after a bad leaf")
    s.close()


# ---- randomised leg ----
def test_randomised_trees():
    with_rows = 0
    for seed in ftc.RANDOM_SEEDS:
        scen = ftc.random_tree_scenario(seed)
        lo, hi = clamp_args(scen)
        ref = ftr.fold(scen.blocks, scen.tree, scen.min_ts, scen.max_ts)
        try:
            g, stats = gpu_tree(scen.builder(), scen.tree, VT_INT64, lo, hi)
            assert_i64(g, ref, f"seed {seed}")
            assert_stats(stats, scen, f"seed {seed}")
        except Exception:
            print(f"FAILING SEED {seed}: ftc.random_tree_scenario({seed})")
            raise
        with_rows += stats[3] > 0
    assert with_rows >= 10, with_rows


# ---- the pure-C consumer ----
def test_c_consumer_runs_tree_scan(tmp_path):
    """tools/cabi_filter_tree_check.c: one OR-tree scan through the header
    alone, checked against its own host loop."""
    exe = str(tmp_path / "cabi_filter_tree_check")
    ftc.build_tree_consumer(exe)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stderr + p.stdout
    assert "filter tree consumer OK" in p.stdout
