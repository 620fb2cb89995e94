"""The structure test_gpu_loop_trips.py relies on, checked without a GPU:
the parts of loop_trip_cases are larger than the grid caps that kernels.hip
names, and every category of block the GPU tests mean to cross a cap with
lies on both sides of it — so those tests cannot pass vacuously, and a
raised cap fails here."""
import collections
import re

import pytest

import field_pack_ref as fpr
import filter_ref as fr
import loop_trip_cases as ltc
import row_dedup_ref as rdr
from banyandb_amd import TagCond, OP_EQ

ENC = {"const": ltc.ENC_CONST, "dconst": ltc.ENC_DELTA_CONST,
       "dense": ltc.ENC_DELTA, "multi": ltc.ENC_DELTA, "dod": ltc.ENC_DOD,
       "plain": ltc.ENC_PLAIN}
BOTH = {"below", "past"}


def side(i, cap):
    return "past" if i >= cap else "below"


def both_sides(pairs, cap):
    """pairs: (block index, category).  category -> the sides it lies on."""
    out = collections.defaultdict(set)
    for i, cat in pairs:
        out[cat].add(side(i, cap))
    return dict(out)


def test_the_caps_are_named_once_and_the_parts_exceed_them():
    caps = ltc.caps()
    with open(ltc.KERNELS) as f:
        text = f.read()
    # every launch site takes the named value, none a literal
    assert len(re.findall(r"<\s*SCAN_MAX_WGS\b", text)) == 3
    assert len(re.findall(r"<\s*BLOCK_KERNEL_MAX_WGS\b", text)) == 6
    assert not re.findall(r"<\s*(8192|65535)\s*\?", text)
    waves = ltc.scan_waves()
    assert waves == 4 * caps["SCAN_MAX_WGS"]
    # at least a thousand waves (workgroups) take a second trip, none a third
    assert waves + 1000 < ltc.N_S < 2 * waves
    assert caps["BLOCK_KERNEL_MAX_WGS"] + 400 < ltc.N_B < \
        2 * caps["BLOCK_KERNEL_MAX_WGS"]
    assert ltc.B_HI >= caps["BLOCK_KERNEL_MAX_WGS"]
    assert ltc.EXT_HI >= waves and ltc.LATEST >= waves
    for name, n in (("s", ltc.N_S), ("twin", ltc.N_S), ("f", ltc.N_S),
                    ("b", ltc.N_B)):
        assert ltc.part(name).n_blocks == n
        rows = sum(len(b.ts) for b in ltc.rows_of(name))
        assert rows <= ltc.MAX_ROWS, (name, rows)
    d = ltc.part("d")
    assert d.n_blocks == 2 * ltc.N_D_PAIRS + len(ltc.D_FULL)
    assert d.n_blocks > caps["BLOCK_KERNEL_MAX_WGS"]
    assert 2 * d.n_blocks <= ltc.MAX_ROWS


def test_the_kind_period_does_not_divide_the_wave_count():
    waves = ltc.scan_waves()
    period = len(ltc.KINDS)
    assert period % 2 == 1 and waves % period != 0
    assert waves % ltc.N_SHAPES != 0 and waves % 13 != 0 and waves % 3 != 0
    for flt in (False, True):
        for w in range(ltc.N_S - waves):
            assert ltc.kind_of(w, flt) != ltc.kind_of(w + waves, flt)


def test_the_matrix_names_every_non_streaming_instantiation():
    seen = {i for q in ltc.MATRIX for i in ltc.instantiations(q)}
    assert len(ltc.MATRIX) == 16 and len(seen) == 24
    assert len({i for i in seen if i[3]}) == 8      # the EN_WALK passes


def test_part_s_encodings_lie_on_both_sides_of_the_scan_cap():
    waves = ltc.scan_waves()
    rows, descs = ltc.rows_of("s"), ltc.part("s").blocks()
    cats, ts_encs, sizes = [], [], []
    for i, (b, d) in enumerate(zip(rows, descs)):
        kind = ltc.kind_of(i)
        assert d.field_enc == ENC[kind], (i, kind, d.field_enc)
        assert d.count == len(b.ts)
        if kind == "dense":
            assert d.field_len == d.count - 1, i       # one byte per delta
        if kind == "multi":
            assert d.field_len > d.count - 1, i
        cats.append((i, kind))
        if kind == "plain" and None in b.vals:
            cats.append((i, "plain with nulls"))
        ts_encs.append((i, d.ts_enc_with_version))
        sizes.append((i, len(b.ts)))
        assert d.group_code == 0 and b.group_code == i % 3
    got = both_sides(cats, waves)
    assert set(got) == set(ENC) | {"plain with nulls"}
    assert all(v == BOTH for v in got.values()), got
    # const, delta-const and stream-coded (delta of delta) timestamp lists
    got = both_sides(ts_encs, waves)
    assert len(got) >= 3 and all(v == BOTH for v in got.values()), got
    got = both_sides(sizes, waves)
    assert {1, 2, 3, 4, 5, 65, 130} <= set(got)
    assert all(v == BOTH for v in got.values() if v != {"past"}), got
    # the coded view keeps index % 3
    assert [d.group_code for d in ltc.part("s", True).blocks()[:7]] == \
        [0, 1, 2, 0, 1, 2, 0]
    # every kind touches an int64 extreme, in blocks past the cap only (the
    # best single row must come from there); the values next to the
    # extremes lie below it
    touch = collections.defaultdict(set)
    near = set()
    for i, b in enumerate(rows):
        for v in b.vals:
            if v in (ltc.IMIN, ltc.IMAX):
                touch[ltc.kind_of(i)].add(v)
                assert i >= waves
            elif v is not None and i < waves and \
                    min(v - ltc.IMIN, ltc.IMAX - v) < 1000:
                near.add(v > 0)
    assert set(touch) == set(ENC) and near == {False, True}
    assert set().union(*touch.values()) == {ltc.IMIN, ltc.IMAX}
    # the twin: same skeleton, no Plain block
    for b, d in zip(ltc.rows_of("twin"), ltc.part("twin").blocks()):
        assert d.field_enc != ltc.ENC_PLAIN and None not in b.vals
        assert d.count == len(b.ts)


def test_part_f_exponents_differ_between_a_waves_two_trips():
    waves = ltc.scan_waves()
    descs = ltc.part("f").blocks()
    got = both_sides([(i, d.exp) for i, d in enumerate(descs)], waves)
    assert sum(1 for v in got.values() if v == BOTH) >= 3, got
    differ = sum(1 for w in range(ltc.N_S - waves)
                 if descs[w].exp != descs[w + waves].exp)
    assert differ > 1000
    encs = both_sides([(i, d.field_enc) for i, d in enumerate(descs)], waves)
    assert len(encs) >= 4 and all(v == BOTH for v in encs.values())
    # quarters, halves and whole numbers of modest size: double sums exact
    for b in ltc.rows_of("f"):
        assert all(v * 4 == int(v * 4) and abs(v) < 2 ** 24 for v in b.vals)


@pytest.mark.parametrize("name", ["s", "twin", "f"])
def test_predicate_group_and_clamp_categories_on_both_sides(name):
    waves = ltc.scan_waves()
    rows = ltc.rows_of(name)
    for what, want in ((ltc.verdict, {"clear", "skip", "walk"}),
                       (ltc.group_shape, {"uniform", "varying"}),
                       (lambda b: ltc.group_shape(b, 2),
                        {"uniform", "varying"}),
                       (ltc.clamp_shape, {"whole", "cut", "missed"})):
        got = both_sides([(i, what(b)) for i, b in enumerate(rows)], waves)
        assert set(got) == want and all(v == BOTH for v in got.values()), got
    # about a third of the blocks carry nils on slot 1
    nils = sum(1 for b in rows if None in b.tags[1])
    assert 0.25 < nils / len(rows) < 0.4
    # slot 0: an entity tag, uniform per block, four values
    assert all(len(set(b.tags[0])) == 1 for b in rows)
    assert len({b.tags[0][0] for b in rows}) == 4


def test_both_branches_of_the_wave_partial_run_on_the_second_trip():
    """A wave's second block falls in the group of its first (the partial
    merges) or in another (it is flushed and reset).  By tag: both occur
    among the uniform blocks, on slot 1 and — among the blocks the
    predicate does not skip — on slot 2.  By block code: always another.
    Without groups: always the same."""
    waves = ltc.scan_waves()
    rows = ltc.rows_of("s")
    for pred in (False, True):
        slot, domain = ltc.group_slot(pred)
        same = other = 0
        for w in range(ltc.N_S - waves):
            a, b = rows[w], rows[w + waves]
            assert a.group_code != b.group_code
            if pred and "skip" in (ltc.verdict(a), ltc.verdict(b)):
                continue
            if ltc.group_shape(a, slot) == ltc.group_shape(b, slot) == \
                    "uniform" and a.tags[slot][0] in domain and \
                    b.tags[slot][0] in domain:
                if a.tags[slot][0] == b.tags[slot][0]:
                    same += 1
                else:
                    other += 1
        assert same >= 30 and other >= 30, (pred, same, other)


def test_every_expected_result_names_no_empty_group():
    """The oracle's results for every query of the GPU matrix: a non-zero
    count in every group."""
    assert ltc.group_slot(False) == (1, ltc.DOMAIN)
    assert ltc.group_slot(True)[0] != 1
    for name in ("s", "f"):
        for _v, pred, group, clamp in ltc.MATRIX:
            res = ltc.oracle_agg(name, pred, "tag" if group else None, clamp)
            assert len(res) == (3 if group else 1)
            assert all(r.count > 0 for r in res), (name, pred, group, clamp)
        for clamp in (False, True):
            res = ltc.oracle_agg(name, False, "code", clamp)
            assert len(res) == 3 and all(r.count > 0 for r in res)
    # the clamp and the predicate both bite
    full = ltc.oracle_agg("s")[0].count
    assert full == sum(1 for b in ltc.rows_of("s") for v in b.vals
                       if v is not None)
    assert 0 < ltc.oracle_agg("s", clamp=True)[0].count < full
    assert 0 < ltc.oracle_agg("s", pred=True)[0].count < full


def test_the_oracle_and_the_per_row_models_agree_on_part_s():
    blocks = ltc.model("s")
    cond = [TagCond(1, OP_EQ, [ltc.LIT])]
    for pred in (False, True):
        for clamp in (False, True):
            lo, hi = ltc.CLAMP if clamp else (None, None)
            f = fr.fold(blocks, cond if pred else [], lo, hi)
            w = ltc.oracle_agg("s", pred, None, clamp)[0]
            assert (f.count, f.sum_i, f.min, f.max) == \
                (w.count, w.sum_i, w.min_i, w.max_i)
            slot, domain = ltc.group_slot(pred)
            fs = fr.fold_by_tag(blocks, cond if pred else [], slot, domain,
                                lo, hi)
            ws = ltc.oracle_agg("s", pred, "tag", clamp)
            assert [(f.count, f.sum_i) for f in fs] == \
                [(w.count, w.sum_i) for w in ws]


def test_filter_cases_select_rows_on_both_sides():
    import filter_tree_ref as ftr
    waves = ltc.scan_waves()
    blocks = ltc.model("s")
    for picked in (fr.select_rows(blocks, ltc.CONDS),
                   ftr.select_rows(blocks, ltc.TREE)):
        got = {side(b.sid - 1, waves) for b, _ in picked}
        assert got == BOTH
    for folds in (fr.fold_by_tag(blocks, ltc.CONDS, 1, ltc.DOMAIN),
                  ftr.fold_by_tag(blocks, ltc.TREE, 1, ltc.DOMAIN)):
        assert all(f.count > 0 for f in folds)


def test_top_and_row_scan_winners_lie_on_both_sides():
    waves = ltc.scan_waves()
    for sel in ltc.SELECTIONS:
        for asc in (False, True):
            for n in ltc.TOP_NS:
                # several winners: on both sides; a single one: past the cap
                want = ltc.top_expected(sel, n, asc)
                assert len(want) == n
                assert ltc.sides(want, waves) == \
                    (BOTH if n > 1 else {"past"}), (sel, n, asc)
        for desc in (False, True):
            for offset, limit in ltc.ROW_WINDOWS:
                want = ltc.rows_expected(sel, offset, limit, desc)
                assert len(want) == limit
                assert ltc.sides(want, waves) == \
                    (BOTH if limit > 1 else {"past"}), (sel, desc)
    assert ltc.top_expected("all", 1, False)[0][3] == ltc.IMAX
    assert ltc.top_expected("all", 1, True)[0][3] == ltc.IMIN


def test_part_b_work_blocks_lie_below_500_and_past_the_cap():
    cap = ltc.caps()["BLOCK_KERNEL_MAX_WGS"]
    rows, p = ltc.rows_of("b"), ltc.part("b")
    kinds = ltc.b_kinds()
    got = both_sides(kinds.items(), cap)
    assert set(got) == {"plain", "hit", "nohit", "bitmap"}
    assert all(v == BOTH for v in got.values()), got
    # the workgroup of a block below 500 takes a work block past the cap too
    assert all((i + cap in kinds) for i in kinds if i < ltc.B_WORK
               and i + cap < ltc.N_B)
    descs = p.blocks()
    for i, b in enumerate(rows):
        kind = kinds.get(i, "filler")
        d = descs[i]
        assert fpr.candidate(d) == (kind in ("hit", "nohit")), (i, kind)
        if fpr.candidate(d):
            assert fpr.packs(p.payload, d) == (kind == "hit"), i
        plain = len({v for v in b.tags[0] if v is not None}) > 256
        assert plain == (kind == "plain")
        if kind == "bitmap":
            assert all(len(set(col)) > 1 for col in b.tags)
        if kind == "filler":
            assert len(b.ts) == 1
    cand, hit, nbytes = fpr.census(p)
    n_hit = sum(1 for k in kinds.values() if k == "hit")
    n_nohit = sum(1 for k in kinds.values() if k == "nohit")
    assert (cand, hit) == (n_hit + n_nohit, n_hit) and nbytes > 0
    assert sum(1 for k in kinds.values() if k == "plain") <= 40
    # the plain-slot predicate and group-by, and the tree, select rows of
    # work blocks on both sides
    import filter_tree_ref as ftr
    for picked in (fr.select_rows(rows, ltc.B_CONDS),
                   ftr.select_rows(rows, ltc.B_TREE)):
        got = {side(b.sid - 1, cap) for b, _ in picked
               if b.sid - 1 in kinds}
        assert got == BOTH
    folds = fr.fold_by_tag(rows, [], 0, ltc.B_PLAIN_DOMAIN)
    assert all(f.count > 0 for f in folds)


def test_part_d_every_block_is_involved_and_partially_superseded():
    cap = ltc.caps()["BLOCK_KERNEL_MAX_WGS"]
    rows = ltc.rows_of("d")
    census = ltc.d_census()
    n_full = len(ltc.D_FULL)
    assert census == [len(rows), len(rows) - n_full, n_full,
                      len(rows) + n_full]
    assert census[0] > cap and census[1] > cap
    keep = rdr.survivors(rows)
    full = [i for i, k in enumerate(keep) if not k]
    assert {side(i, cap) for i in full} == BOTH and len(full) == n_full
    assert all(len(k) == 1 for i, k in enumerate(keep) if i not in full)
    # the condition keeps some survivors and drops others, on both sides
    merged = rdr.merged(rows)
    f_all, f_eq = fr.fold(merged, []), fr.fold(merged, ltc.D_COND)
    assert 0 < f_eq.count < f_all.count == ltc.N_D_PAIRS * 2
    # the latest 100 surviving rows come from both sides of the cap
    want = ltc.rows_expected("all", 0, 100, True, name="d", dedup=True)
    assert len(want) == 100 and ltc.sides(want, cap) == BOTH
