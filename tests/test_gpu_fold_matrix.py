"""GPU parity: the field fold over every encoding, from both of its callers.

The scan kernel folds rows [r0, r1] of a block; the row-varying group-by
run merge folds sub-ranges [a, b] of it.  Each field shape below is one
part with one block per row count, and each part is scanned in every
caller mode, over the full range and clamps, with and without MIN/MAX,
against the CPU oracle (as tests/test_gpu_groupby_tag.py does).

Row counts: 1 (no stream), 2 (delta-of-delta has a row 1 and no second-
order delta), 3 (the first second-order delta), 64 / 65 (the wave edge),
257 (one row past a 256-row scan window), 8192 (the largest block, varint
shapes only).

The int-list encoder stores every 1-row list as Const and every 2-row list
as DeltaConst.  A 2-row Delta or DeltaOfDelta stream holds the same single
varint as the DeltaConst one, so those blocks are built by relabelling the
descriptor; 1-row blocks stay Const.  Blocks too small for the encoder's
plain-tag bail (more than 256 distinct values) need a hand-written plain
column, so the plain tag of every block is written by hand in the
reference layout ([ENC_PLAIN][bytes block]) behind the builder's payload,
as tests/test_gpu_plain_tag.py does.

Every block has timestamps T0 + i*MS, so one clamp cannot end on row n-2
of every size: beside the clamps [1, 62] and [2, 63] (ends on rows 1 and 2
of every block that has them, on n-2 of the 64- and 65-row blocks) there
is one clamp per remaining size whose upper end is that size's row n-2.
"""
import ctypes as C
import math
import random

import pytest

import oracle as o
from banyandb_amd import (PartBuilder, Session, lib, VT_INT64, VT_FLOAT64,
                          FLOAT_RAW_EXP, AGG_SUM, AGG_COUNT, AGG_MIN, AGG_MAX)
from helpers import oracle_blocks

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000_000_000_000
MS = 10 ** 6
ENVS = [b"prod", b"dev", b"staging", b"qa"]
REGIONS = [b"r0", b"r1", b"r2", b"r3"]
USER = b"user_003"
ENC_CONST, ENC_DELTA_CONST, ENC_DELTA, ENC_DOD, ENC_PLAIN = 1, 2, 3, 4, 9

SIZES = [1, 2, 3, 64, 65, 257]
VARINT_SHAPES = ("delta_dense", "delta_multi", "dod")
SHAPES = ["const", "delta_const", "delta_dense", "delta_multi", "dod",
          "plain_i64", "plain_f64", "decimal_f64"]

# (first row, last row) of each range; None is the full range
RANGES = [None, (1, 62), (2, 63), (2, 255), (1, 8190), (0, 1), (0, 0)]
FUNC_SETS = [[AGG_SUM, AGG_COUNT], [AGG_SUM, AGG_COUNT, AGG_MIN, AGG_MAX]]

# caller modes: (group-by slot 0, predicates per tag slot)
MODES = {
    "no_tags": (False, None),
    "dict_pred": (False, [b"prod"]),
    "plain_pred": (False, [b"", USER]),
    "groupby": (True, None),
    "groupby_dict_pred": (True, [b"", b"", b"r0"]),
    "groupby_plain_pred": (True, [b"", USER, b""]),
}


def _values(shape, rng, n, k):
    """Field values of block k (n rows) of a shape."""
    if shape == "const":
        return [1000 + k] * n
    if shape == "delta_const":
        return [-500 + 7 * k + (3 + k) * i for i in range(n)]
    if shape in ("delta_dense", "delta_multi"):
        # both delta signs and small drops of a large value: neither a
        # delta list nor an incremental one, so the encoder keeps Delta
        v = [10 ** 12]
        for i in range(1, n):
            if shape == "delta_dense":
                d = rng.randint(1, 63)
            elif i == 1:
                d = 10 ** 6          # the stream is never all one-byte
            else:
                d = rng.randint(1, rng.choice([63, 8000, 10 ** 6, 10 ** 9]))
            v.append(v[-1] + (d if i % 2 else -d))
        return v
    if shape == "dod":
        v = [-10 ** 6]
        for i in range(1, n):
            # no two neighbouring increments are equal: never DeltaConst
            v.append(v[-1] + rng.choice([1, 40, 900, 70000, 10 ** 7]) + i % 2)
        return v
    if shape == "plain_i64":
        return [None if rng.random() < 0.3 else rng.randint(-10 ** 12, 10 ** 12)
                for _ in range(n)]
    if shape == "plain_f64":
        # mostly large positives so that no group sum cancels to near zero
        return [None if rng.random() < 0.3 else
                rng.uniform(-1e4, -1.0) if rng.random() < 0.2 else
                rng.uniform(1e5, 1e6) for _ in range(n)]
    if shape == "decimal_f64":
        # even blocks carry two decimals, odd blocks one: the exponents
        # differ and the merge rescales the odd blocks' partials
        if k % 2 == 0:
            cents = [rng.randint(-1000, 10 ** 6) | 1 for _ in range(n)]
            return [c / 100.0 for c in cents]
        return [(rng.randint(-100, 10 ** 5) * 10 + 3) / 10.0 for _ in range(n)]
    raise AssertionError(shape)


def _natural_enc(shape, n):
    """The encoding the int-list encoder gives a block of the shape."""
    if shape in ("plain_i64", "plain_f64"):
        return ENC_PLAIN
    if n == 1 or shape == "const":
        return ENC_CONST
    if n == 2 or shape == "delta_const":
        return ENC_DELTA_CONST
    return ENC_DOD if shape == "dod" else ENC_DELTA


def _intended_enc(shape, n):
    if n == 2 and shape in VARINT_SHAPES:
        return ENC_DOD if shape == "dod" else ENC_DELTA
    return _natural_enc(shape, n)


def _runs(rng, n, k, table, nil_p):
    """Row-varying tag column whose runs break after rows 0, 1 and n-2."""
    head = [table[0], table[1]] if k % 2 == 0 else [table[1], table[0]]
    tags = head[:n]
    while len(tags) < n:
        run = min(rng.randint(1, 40), n - len(tags))
        v = rng.choice([t for t in table if t != tags[-1]])
        if rng.random() < nil_p:
            v = None
        tags.extend([v] * run)
    if n >= 3 and tags[n - 1] == tags[n - 2]:
        tags[n - 1] = next(t for t in table if t != tags[n - 2])
    return tags


def _plain_tag(rng, n, k):
    """Plain tag column: USER on about half the rows, more than 256
    other values on the rest where the block is large enough."""
    col = [USER if rng.random() < 0.5 else b"user_%03d" % rng.randrange(4, 304)
           for _ in range(n)]
    for row, hit in ((0, k % 2 == 0), (1, k % 2 == 1), (2, True),
                     (n - 2, k % 2 == 0), (n - 1, True)):
        if 0 <= row < n:
            col[row] = USER if hit else b"user_%03d" % (4 + row % 300)
    return col


class _Part:
    """What helpers.oracle_blocks reads of a builder."""

    def __init__(self, payload, descs):
        self.payload = bytes(payload)
        self._descs = descs

    def blocks(self):
        return list(self._descs)


def _build(shape):
    rng = random.Random(SHAPES.index(shape) + 900)
    sizes = SIZES + ([8192] if shape in VARINT_SHAPES else [])
    b = PartBuilder()
    plain_cols = []
    for k, n in enumerate(sizes):
        ts = [T0 + i * MS for i in range(n)]
        vals = _values(shape, rng, n, k)
        add = {"plain_i64": b.add_block_i64_nullable,
               "plain_f64": b.add_block_f64_nullable,
               "decimal_f64": b.add_block_f64}.get(shape, b.add_block_i64)
        add(k + 1, ts, [1] * n, vals)
        b.set_block_tag(_runs(rng, n, k, ENVS, 0.1))        # slot 0: dict
        b.set_block_tag([b"x"] * n)       # slot 1: replaced by the plain column
        b.set_block_tag(_runs(rng, n, k, REGIONS, 0.0))     # slot 2: dict
        plain_cols.append(_plain_tag(rng, n, k))
    payload = bytearray(b.payload)
    built = b.blocks()
    descs = (type(built[0]) * len(built))(*built)
    for k, n in enumerate(sizes):
        d = descs[k]
        assert d.count == n
        if shape == "decimal_f64":
            assert d.field_enc != ENC_PLAIN
        else:
            assert d.field_enc == _natural_enc(shape, n), (shape, n, d.field_enc)
            d.field_enc = _intended_enc(shape, n)
        if shape == "delta_dense" and n >= 2:
            assert d.field_len == n - 1          # every delta in one byte
        if shape == "delta_multi" and n >= 2:
            assert d.field_len > n - 1
        stream = bytes([ENC_PLAIN]) + o.bytes_block_encode(plain_cols[k])
        d.tag2_off, d.tag2_len = len(payload), len(stream)
        payload.extend(stream)
    exp = 0
    if shape == "plain_f64":
        exp = FLOAT_RAW_EXP
    elif shape == "decimal_f64":
        exps = {d.exp for d in descs}
        assert len(exps) >= 2, exps
        exp = min(exps)
    return payload, descs, exp


def _check(shape, funcs, got, want, where):
    want_mm = AGG_MIN in funcs
    for g, oc in zip(got, want):
        assert g.count == oc.count, where
        if shape in ("plain_f64", "decimal_f64"):
            if oc.count:
                if want_mm:
                    assert g.min_f == oc.min_f and g.max_f == oc.max_f, where
                assert math.isclose(g.sum_f, oc.sum_f, rel_tol=1e-9,
                                    abs_tol=1e-6 if shape == "plain_f64"
                                    else 0.0), where
        else:
            assert g.sum_i == oc.sum_i, where
            if want_mm and oc.count:
                assert g.min_i == oc.min_i and g.max_i == oc.max_i, where


@pytest.mark.parametrize("shape", SHAPES)
def test_fold_matrix(shape):
    payload, descs, exp = _build(shape)
    vtype = VT_FLOAT64 if shape in ("plain_f64", "decimal_f64") else VT_INT64
    opayload, oblocks = oracle_blocks(_Part(payload, descs))
    # the oracle does not depend on the aggregate set: one run per
    # (mode, range), shared by both
    want = {}
    for mode, (grouped, preds) in MODES.items():
        for rg in RANGES:
            kw = {}
            if rg is not None:
                kw = dict(min_ts=T0 + rg[0] * MS, max_ts=T0 + rg[1] * MS)
            if grouped:
                want[mode, rg] = o.scan_agg_bytags(
                    opayload, oblocks, vtype, [0], [ENVS], preds=preds, **kw)
            else:
                want[mode, rg] = o.scan_agg(opayload, oblocks, vtype,
                                            preds=preds, **kw)
    assert all(sum(oc.count for oc in want[mode, None]) > 0 for mode in MODES)

    s = Session(0)
    buf = (C.c_uint8 * len(payload)).from_buffer(payload)
    s._ck(lib().bydb_part_reserve(s._h, len(payload), len(descs)))
    s._ck(lib().bydb_part_append(s._h, buf, len(payload), descs, len(descs)))
    for funcs in FUNC_SETS:
        for mode, (grouped, preds) in MODES.items():
            if grouped:
                s.configure_by_tag(vtype, funcs, 0, ENVS, float_exp=exp)
            else:
                s.configure(vtype, funcs, float_exp=exp)
            for rg in RANGES:
                kw = {}
                if rg is not None:
                    kw = dict(min_ts=T0 + rg[0] * MS, max_ts=T0 + rg[1] * MS)
                s.reset()
                s.consume(preds=preds, **kw)
                _check(shape, funcs, s.finalize(), want[mode, rg],
                       (shape, mode, rg, funcs))
    s.close()
