"""CPU side of the raw-row top-N: the per-row model against the reference's
own BatchTop vectors, the host shard merge against the model, the ABI
layout, and the pure-C consumer's compile."""
import ctypes as C
import json
import os
import random
import subprocess

import pytest

import banyandb_amd as ba
from banyandb_amd import TopRow, VT_INT64, VT_FLOAT64
import top_rows_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(__file__), "golden",
                      "top_rows_vectors.json")
GOLDEN_NAMES = [
    "TestBatchTop_AscendingHeap_KeepsLowestN",
    "TestBatchTop_DescendingHeap_KeepsHighestN",
    "TestBatchTop_FewerInputThanN_ReturnsAll_InOrder",
    "TestBatchTop_TieBreaker_Stable",
    "TestBatchTop_NullField_TreatedAsLowest",
    "TestBatchTop_ZeroN_NoOp",
]
BAD_ARG = -3


def golden_cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def test_golden_holds_the_named_cases():
    assert [c["name"] for c in golden_cases()] == GOLDEN_NAMES


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_model_reproduces_reference_vectors(name):
    case = next(c for c in golden_cases() if c["name"] == name)
    got = ref.batch_top(case["values"], case["n"], case["asc"])
    assert got == case["want_input_rows"]
    assert [case["values"][i] for i in got] == case["want"]


def test_model_against_a_full_sort():
    """The bounded heap equals a stable sort cut at n, nulls lowest."""
    rng = random.Random(4100)
    for _ in range(200):
        m = rng.randint(0, 40)
        keys = [None if rng.random() < 0.1 else rng.randint(-3, 3)
                for _ in range(m)]
        n = rng.randint(0, 45)
        asc = rng.random() < 0.5
        lowest = min([k for k in keys if k is not None] or [0]) - 1
        val = [lowest if k is None else k for k in keys]
        order = sorted(range(m), key=lambda i: (val[i] if asc else -val[i], i))
        assert ref.batch_top(keys, n, asc) == order[:n]


# ---- bydb_top_rows_merge ----
def mk_row(sid, ts, ver, vi, vf, seq):
    return TopRow(sid, ts, ver, vi, vf, seq)


def shard_lists(rng, n_lists, max_len, values, is_float, asc):
    """Per-shard results as bydb_top_finalize returns them: sorted by value,
    then seq ascending."""
    lists = []
    for l in range(n_lists):
        m = rng.randint(0, max_len)
        rows = []
        for seq in sorted(rng.sample(range(1 << 20), m)):
            v = rng.choice(values)
            rows.append(mk_row(100 + l, 5000 + seq, l, 0 if is_float else v,
                               float(v) / 4 if is_float else 0.0, seq))
        key = (lambda r: r.value_f) if is_float else (lambda r: r.value_i)
        rows.sort(key=lambda r: (key(r) if asc else -key(r), r.seq))
        lists.append(rows)
    return lists


def check_merge(lists, is_float, n, asc):
    vt = VT_FLOAT64 if is_float else VT_INT64
    got = ba.top_rows_merge(lists, vt, n, asc)
    flat = [r for rows in lists for r in rows]
    keys = [r.value_f if is_float else r.value_i for r in flat]
    want = [flat[i] for i in ref.batch_top(keys, n, asc)]
    assert [r.astuple() for r in got] == [r.astuple() for r in want]


@pytest.mark.parametrize("is_float", [False, True])
@pytest.mark.parametrize("asc", [False, True])
def test_merge_matches_the_model_over_the_concatenation(is_float, asc):
    rng = random.Random(4200 + 2 * is_float + asc)
    for _ in range(60):
        # few distinct values: ties inside and across lists
        lists = shard_lists(rng, rng.randint(1, 5), 12, [-1, 0, 1, 7],
                            is_float, asc)
        for n in (0, 1, 3, 10, 1024):
            check_merge(lists, is_float, n, asc)


def test_merge_ties_across_lists_earlier_list_wins():
    a = [mk_row(1, 10, 1, 5, 0.0, 900), mk_row(1, 11, 1, 5, 0.0, 901)]
    b = [mk_row(2, 20, 1, 5, 0.0, 3), mk_row(2, 21, 1, 4, 0.0, 4)]
    got = ba.top_rows_merge([a, b], VT_INT64, 3, False)
    assert [(r.series_id, r.seq) for r in got] == [(1, 900), (1, 901), (2, 3)]
    got = ba.top_rows_merge([b, a], VT_INT64, 2, False)
    assert [(r.series_id, r.seq) for r in got] == [(2, 3), (1, 900)]


def test_merge_short_and_empty_lists():
    a = [mk_row(1, 10, 1, 9, 0.0, 1)]
    assert ba.top_rows_merge([], VT_INT64, 5) == []
    assert ba.top_rows_merge([[], []], VT_INT64, 5) == []
    got = ba.top_rows_merge([[], a, []], VT_INT64, 5)
    assert [r.astuple() for r in got] == [a[0].astuple()]
    assert ba.top_rows_merge([a], VT_INT64, 0) == []


def test_merge_rejects_bad_arguments():
    got = C.c_int64(7)
    out = (TopRow * 1)()
    lib = ba.lib()
    assert lib.bydb_top_rows_merge(None, None, 0, VT_INT64, -1, 0, out,
                                   C.byref(got)) == BAD_ARG
    assert lib.bydb_top_rows_merge(None, None, 0, 99, 1, 0, out,
                                   C.byref(got)) == BAD_ARG
    assert lib.bydb_top_rows_merge(None, None, 0, VT_INT64, 1, 0, out,
                                   None) == BAD_ARG


# ---- ABI ----
def test_top_row_is_48_bytes_and_symbols_exist():
    assert C.sizeof(TopRow) == 48
    assert ba.TOP_ROWS_MAX == 1024
    lib = ba.lib()
    for sym in ("bydb_top_configure", "bydb_top_finalize",
                "bydb_top_rows_merge"):
        assert getattr(lib, sym) is not None
    assert [f[0] for f in TopRow._fields_] == [
        "series_id", "ts", "version", "value_i", "value_f", "seq"]


def test_c_consumer_compiles(tmp_path):
    exe = str(tmp_path / "cabi_top_rows_check")
    build_consumer(exe)
    assert os.path.exists(exe)


def build_consumer(exe):
    """Compile tools/cabi_top_rows_check.c against the header alone."""
    subprocess.run(
        ["gcc", "-std=c99", "-Wall", "-Werror", "-I",
         os.path.join(REPO, "include"),
         os.path.join(REPO, "tools", "cabi_top_rows_check.c"),
         "-L", os.path.join(REPO, "banyandb_amd"), "-lbydb_gpu",
         "-Wl,-rpath," + os.path.join(REPO, "banyandb_amd"), "-o", exe],
        check=True)
