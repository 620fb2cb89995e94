"""CPU checks for the tag filter operators: the reference evaluator
(tests/filter_ref.py) against the golden truth table and the pinned
oracle, the new C-ABI export, the pure-C consumer, and the non-vacuity of
the GPU parity cases."""
import ctypes
import json
import os
import random
import subprocess

import pytest

import banyandb_amd as ba
from banyandb_amd import (TagCond, i64_tag_cell, OP_EQ, OP_NE, OP_LT, OP_GT,
                          OP_LE, OP_GE, OP_IN, OP_NOT_IN, TAG_STRING, TAG_INT,
                          VT_INT64)
import filter_ref as fr
import filter_cases as fc
from helpers import oracle_scan

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "tag_filter_vectors.json")
OPS = {"EQ": OP_EQ, "NE": OP_NE, "LT": OP_LT, "LE": OP_LE, "GT": OP_GT,
       "GE": OP_GE, "IN": OP_IN, "NOT_IN": OP_NOT_IN}


def _vectors():
    return json.load(open(GOLDEN))["vectors"]


def _decode(vec):
    is_int = vec["type"] == "int"
    enc = i64_tag_cell if is_int else (lambda s: s.encode())
    lits = [enc(x) for x in vec["lits"]]
    if "value_hex" in vec:
        val = bytes.fromhex(vec["value_hex"])
    else:
        val = None if vec["value"] is None else enc(vec["value"])
    return OPS[vec["op"]], TAG_INT if is_int else TAG_STRING, lits, val


def test_golden_table_covers_the_required_rows():
    vs = _vectors()
    for typ in ("string", "int"):
        nil_ops = {v["op"] for v in vs
                   if v["type"] == typ and "value" in v and v["value"] is None}
        assert nil_ops == set(OPS), (typ, nil_ops)
    assert any(v["type"] == "string" and v["lits"] == [""] and
               v.get("value", 0) is None for v in vs)
    assert any(v["type"] == "string" and v["lits"] == ["abc"] and
               v.get("value") == "ab" for v in vs)
    assert any(v["type"] == "int" and isinstance(v.get("value"), int) and
               v["value"] < 0 for v in vs)
    assert any(v["type"] == "int" and isinstance(v.get("value"), int) and
               abs(v["lits"][0] - v["value"]) > 2 ** 63 for v in vs)


def test_evaluator_reproduces_every_golden_vector():
    bad = []
    for vec in _vectors():
        op, tt, lits, val = _decode(vec)
        if fr.match(op, tt, lits, val) != vec["expected"]:
            bad.append(vec)
    assert not bad, bad


def test_evaluator_eq_agrees_with_oracle():
    """EQ-only conditions through the evaluator equal the pinned oracle's
    equality predicate over the same built parts (entity tags, row-varying
    runs with nils, a plain column, two slots)."""
    rng = random.Random(2001)
    scen = fc.Scenario(fc.rowvary(rng, fc.ENVS, n_series=3, n=800), [])
    for pred in (b"prod", b"qa", b"absent"):
        scen.conds = [TagCond(0, OP_EQ, [pred])]
        orc = oracle_scan(scen.builder(), VT_INT64, pred=pred)[0]
        ref = fr.fold(scen.blocks, scen.conds)
        assert (ref.count, ref.sum_i) == (orc.count, orc.sum_i), pred
        if ref.count:
            assert (ref.min, ref.max) == (orc.min_i, orc.max_i), pred
    n = 700
    blocks = [fc.Blk(sid + 1, fc.ts_of(n), fc.ivals(rng, n),
                     [[fc.ENVS[sid % 4]] * n, fc.plain_col(rng, n)])
              for sid in range(4)]
    scen = fc.Scenario(blocks, [TagCond(0, OP_EQ, [b"dev"]),
                                TagCond(1, OP_EQ, [b"u5"])])
    lo, hi = fc.T0 + 100 * fc.MS, fc.T0 + 600 * fc.MS
    orc = oracle_scan(scen.builder(), VT_INT64, preds=[b"dev", b"u5"],
                      min_ts=lo, max_ts=hi)[0]
    ref = fr.fold(scen.blocks, scen.conds, lo, hi)
    assert ref.count > 0
    assert (ref.count, ref.sum_i, ref.min, ref.max) == \
        (orc.count, orc.sum_i, orc.min_i, orc.max_i)


def test_library_exports_consume_filter():
    lib = ctypes.CDLL(os.path.join(REPO, "banyandb_amd", "libbydb_gpu.so"))
    assert hasattr(lib, "bydb_consume_filter")
    assert ctypes.sizeof(ba.TagCondC) == 32
    assert callable(ba.Session.consume_filter)


def test_filter_consumer_compiles_as_c99(tmp_path):
    """tools/cabi_filter_check.c makes one filtered scan through the header
    alone; it must build with plain gcc."""
    subprocess.run(
        ["gcc", "-std=c99", "-Wall", "-Werror", "-I",
         os.path.join(REPO, "include"),
         os.path.join(REPO, "tools", "cabi_filter_check.c"),
         "-L", os.path.join(REPO, "banyandb_amd"), "-lbydb_gpu",
         "-Wl,-rpath," + os.path.join(REPO, "banyandb_amd"),
         "-o", str(tmp_path / "cabi_filter_check")], check=True)


@pytest.mark.parametrize("name,make,expect", fc.CASES, ids=fc.CASE_IDS)
def test_gpu_cases_are_not_vacuous(name, make, expect):
    scen = make()
    sel = fr.fold(scen.blocks, scen.conds, scen.min_ts, scen.max_ts).count
    total = fr.fold(scen.blocks, [], scen.min_ts, scen.max_ts).count
    assert total > 0
    if expect == fc.PARTIAL:
        assert 0 < sel < total, (name, sel, total)
    elif expect == fc.ALL:
        assert sel == total == scen.n_rows
    else:
        assert sel == 0


def test_case_blocks_stay_small():
    for name, make, _ in fc.CASES:
        scen = make()
        assert len(scen.blocks) <= 8, name
        assert all(len(b.ts) <= 3000 for b in scen.blocks), name
