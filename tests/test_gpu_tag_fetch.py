"""GPU parity of the tag projection for raw-row results
(bydb_rows_fetch_tags): tag values by seq.

Expected side: the Python lists the part was built from
(tag_fetch_cases.expect).  Every case compares the value bytes and the nil
flag of every requested row, exactly: None is nil, b"" is the empty value."""
import ctypes as C
import random
import subprocess

import pytest

import banyandb_amd as ba
from banyandb_amd import (Session, TopRow, VT_INT64, AGG_SUM, AGG_COUNT,
                          AGG_MIN, AGG_MAX, INT64_MIN, INT64_MAX)
from banyandb_amd.frame import (FrameBuilder, FrameReader, ROLE_TIMESTAMP,
                                ROLE_TAG, ROLE_FIELD)
import filter_cases as fc
import filter_ref as fr
import row_dedup_cases as rdc
import tag_fetch_cases as tfc
from tag_fetch_cases import seq_of
from test_tag_fetch_cpu import build_consumer

pytestmark = pytest.mark.gpu

BAD_ARG, BAD_DATA, STATE, OOM = -3, -4, -5, -7


def check(s, blocks, seqs, slot):
    """Fetch against the fixture, row for row; returns rows compared."""
    got = s.fetch_tags(seqs, slot)
    want = tfc.expect(blocks, seqs, slot)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, ("request", i, "block", seqs[i] >> 13, "row",
                        seqs[i] & 8191, "slot", slot, g, w)
    return len(want)


def raw_fetch(s, seqs, slot, cap=0, n=None):
    """The C entry point as it is: (rc, total, offs, nil, data bytes)."""
    n = len(seqs) if n is None else n
    arr = (C.c_uint64 * max(len(seqs), 1))(*seqs)
    offs = (C.c_uint64 * (max(n, 0) + 1))(*([77] * (max(n, 0) + 1)))
    nil = (C.c_uint8 * max(n, 1))(*([77] * max(n, 1)))
    data = (C.c_uint8 * max(cap, 1))(*([0xEE] * max(cap, 1)))
    total = C.c_uint64(77)
    rc = ba.lib().bydb_rows_fetch_tags(s._h, arr, n, slot, data, cap, offs,
                                       nil, C.byref(total))
    return rc, total.value, list(offs), list(nil), bytes(data)


def last_error(s):
    return ba.lib().bydb_last_error(s._h).decode()


@pytest.fixture(scope="module")
def mixed():
    pb, blocks, names = tfc.mixed_built()
    s = Session(0)
    s.upload_part(pb)
    yield s, blocks, names
    s.close()


# ---- dictionary columns ----
def test_single_run_blocks_first_and_last_row(mixed):
    s, blocks, names = mixed
    seqs = []
    for name in ("entity_a", "entity_b"):
        b = names[name]
        seqs += [seq_of(b, 0), seq_of(b, len(blocks[b].ts) - 1)]
    assert s.fetch_tags(seqs, 0) == [b"prod", b"prod", b"dev", b"dev"]
    assert check(s, blocks, seqs, 0) == 4
    assert check(s, blocks, seqs, 1) == 4      # entity_b: no second column


def test_value_at_code_zero_and_at_a_later_code(mixed):
    s, blocks, names = mixed
    ab, ba_ = names["order_ab"], names["order_ba"]
    seqs = [seq_of(ab, 0), seq_of(ab, 99), seq_of(ab, 100), seq_of(ab, 199),
            seq_of(ba_, 0), seq_of(ba_, 99), seq_of(ba_, 100), seq_of(ba_, 199)]
    assert s.fetch_tags(seqs, 0) == [b"aa", b"aa", b"bbb", b"bbb",
                                     b"bbb", b"bbb", b"aa", b"aa"]


def test_row_varying_runs_with_nil_runs(mixed):
    """First and last row of runs on both sides of the 64th run (the second
    step of the 64-runs-per-step walk), nil runs, the block's last row."""
    s, blocks, names = mixed
    b = names["rowvary"]
    col = blocks[b].tags[0]
    bounds = tfc.run_bounds(col)
    assert len(bounds) > 128
    rows = []
    for r in (0, 1, 62, 63, 64, 65, 127, 128, 129, len(bounds) - 1):
        rows += [bounds[r][0], bounds[r][1] - 1]
    nil_runs = [k for k, (lo, _) in enumerate(bounds) if col[lo] is None]
    assert nil_runs and nil_runs[-1] >= 64
    rows += [bounds[nil_runs[0]][0], bounds[nil_runs[-1]][1] - 1]
    rows.append(len(col) - 1)
    seqs = [seq_of(b, r) for r in rows]
    assert check(s, blocks, seqs, 0) == len(rows)
    assert None in tfc.expect(blocks, seqs, 0)
    # every row of the block, in calls of at most 1024
    everything = [seq_of(b, r) for r in range(len(col))]
    for at in range(0, len(everything), 1024):
        check(s, blocks, everything[at:at + 1024], 0)


def test_8192_runs_in_one_block(mixed):
    s, blocks, names = mixed
    b = names["alternating"]
    rows = [8191, 8190, 0, 1, 63, 64, 127, 128, 4095, 4096]
    assert check(s, blocks, [seq_of(b, r) for r in rows], 0) == len(rows)
    assert s.fetch_tags([seq_of(b, 8191)], 0) == [b"yy"]


def test_dictionary_of_256_values_in_the_sidecar(mixed):
    """Codes 0, 63, 64 and 255: the length-prefix sum over more than one
    64-value stride, on the host-normalised framing."""
    s, blocks, names = mixed
    b = names["svc"]
    rows = [0, 63, 64, 255, 1, 128, 254, 256, 1499]
    got = s.fetch_tags([seq_of(b, r) for r in rows], 0)
    assert got[:4] == [fc.SVCS[0], fc.SVCS[63], fc.SVCS[64], fc.SVCS[255]]
    assert check(s, blocks, [seq_of(b, r) for r in rows], 0) == len(rows)


def test_empty_string_is_a_value_and_nil_is_nil(mixed):
    s, blocks, names = mixed
    b = names["empty_nil"]
    seqs = [seq_of(b, r) for r in range(30)]
    got = s.fetch_tags(seqs, 0)
    assert got[:15] == [b""] * 7 + [None] * 5 + [b"v"] * 3
    check(s, blocks, seqs, 0)
    rc, total, offs, nil, _ = raw_fetch(s, seqs[:15], 0, cap=16)
    assert (rc, total) == (0, 3)
    assert nil == [0] * 7 + [1] * 5 + [0] * 3
    assert offs == [0] * 13 + [1, 2, 3]


def test_int_cells_come_back_byte_exact(mixed):
    s, blocks, names = mixed
    b = names["rowvary"]
    seqs = [seq_of(b, r) for r in range(0, 3000, 7)]
    check(s, blocks, seqs, 1)
    got = s.fetch_tags(seqs, 1)
    assert all(len(g) == 8 for g in got)
    assert {fr.cell_to_i64(g) for g in got} <= set(fc.CODES)
    assert len({g for g in got}) > 3


# ---- plain columns ----
@pytest.mark.parametrize("name,rows", [
    ("plain321", [0, 63, 64, 320]),
    ("plain3000", [0, 63, 64, 320, 2999, 1234]),
])
def test_plain_column_chunk_boundaries_nil_and_empty(mixed, name, rows):
    s, blocks, names = mixed
    b = names[name]
    col = blocks[b].tags[0]
    rows = rows + [col.index(None), col.index(b""),
                   len(col) - 1 - col[::-1].index(None)]
    seqs = [seq_of(b, r) for r in rows]
    assert check(s, blocks, seqs, 0) == len(rows)
    got = s.fetch_tags(seqs, 0)
    assert None in got and b"" in got
    if name == "plain3000":
        assert got[5] == tfc.LONG_VALUE and len(got[5]) == 300
    everything = [seq_of(b, r) for r in range(len(col))]
    for at in range(0, len(everything), 1024):
        check(s, blocks, everything[at:at + 1024], 0)


# ---- absent slots ----
def test_absent_slot_is_all_nil_mixed_with_present(mixed):
    s, blocks, names = mixed
    a, b, nt = names["entity_a"], names["entity_b"], names["no_tags"]
    seqs = [seq_of(b, 0), seq_of(a, 5), seq_of(nt, 99), seq_of(b, 499),
            seq_of(a, 499)]
    assert s.fetch_tags(seqs, 1) == [None, b"zone-a", None, None, b"zone-a"]
    assert s.fetch_tags(seqs, 2) == [None] * 5
    assert s.fetch_tags([seq_of(nt, 0)], 0) == [None]
    rc, total, offs, nil, _ = raw_fetch(s, seqs, 2)
    assert (rc, total, nil, offs) == (0, 0, [1] * 5, [0] * 6)


# ---- request shape ----
def test_request_of_zero_one_and_1024(mixed):
    s, blocks, names = mixed
    assert s.fetch_tags([], 0) == []
    rc, total, offs, _, _ = raw_fetch(s, [], 0)
    assert (rc, total, offs) == (0, 0, [0])
    assert ba.lib().bydb_rows_fetch_tags(s._h, None, 0, 0, None, 0, None,
                                         None, None) == 0
    assert check(s, blocks, [seq_of(names["svc"], 700)], 0) == 1
    rng = random.Random(7500)
    seqs = []
    while len(seqs) < 1000:                      # unsorted, every block kind
        b = rng.randrange(len(blocks))
        seqs.append(seq_of(b, rng.randrange(len(blocks[b].ts))))
    seqs += seqs[:24]                            # duplicates
    assert len(seqs) == 1024 and seqs != sorted(seqs)
    assert check(s, blocks, seqs, 0) == 1024
    assert check(s, blocks, seqs, 1) == 1024
    rc = raw_fetch(s, seqs + [seqs[0]], 0)[0]
    assert rc == BAD_ARG and "BYDB_TAG_FETCH_MAX" in last_error(s)
    assert raw_fetch(s, seqs, 0, n=-1)[0] == BAD_ARG
    assert check(s, blocks, seqs[:5], 0) == 5


# ---- errors: none sticky ----
def test_errors_leave_the_session_usable(mixed):
    s, blocks, names = mixed
    good = [seq_of(names["order_ab"], 150), seq_of(names["svc"], 64)]
    want = [b"bbb", fc.SVCS[64]]
    for slot in (3, -1):
        assert raw_fetch(s, good, slot)[0] == BAD_ARG
        assert s.fetch_tags(good, 0) == want
    # block index == n_blocks
    rc = raw_fetch(s, good + [seq_of(len(blocks), 0)], 0)[0]
    assert rc == BAD_ARG and "seqs[2]" in last_error(s)
    assert s.fetch_tags(good, 0) == want
    # row == count, first offender named
    b = names["order_ab"]
    rc = raw_fetch(s, [seq_of(b, 199), seq_of(b, 200), seq_of(b, 201)], 0)[0]
    assert rc == BAD_ARG and "seqs[1]" in last_error(s)
    assert s.fetch_tags(good, 0) == want
    # null outputs with n > 0
    arr = (C.c_uint64 * 2)(*good)
    assert ba.lib().bydb_rows_fetch_tags(s._h, arr, 2, 0, None, 0, None, None,
                                         None) == BAD_ARG
    assert s.fetch_tags(good, 0) == want


def test_short_buffer_sizes_the_call(mixed):
    s, blocks, names = mixed
    b = names["plain3000"]
    seqs = [seq_of(b, r) for r in (1234, 0, 5, 2999)] + \
        [seq_of(names["entity_a"], 1)]
    want = tfc.expect(blocks, seqs, 0)
    need = sum(len(w) for w in want if w is not None)
    w_offs = [0]
    for w in want:
        w_offs.append(w_offs[-1] + (len(w) if w is not None else 0))
    w_nil = [1 if w is None else 0 for w in want]
    for cap in (0, need - 1):
        rc, total, offs, nil, data = raw_fetch(s, seqs, 0, cap=cap)
        assert (rc, total, offs, nil) == (OOM, need, w_offs, w_nil)
        assert data == b"\xEE" * max(cap, 1)          # data untouched
    rc, total, offs, nil, data = raw_fetch(s, seqs, 0, cap=need)
    assert (rc, total, offs, nil) == (0, need, w_offs, w_nil)
    assert data == b"".join(w for w in want if w is not None)


def test_no_part_resident_is_a_state_error():
    s = Session(0)
    try:
        assert raw_fetch(s, [0], 0)[0] == STATE
        blocks, kinds = tfc.entity_blocks(random.Random(7600))
        s.upload_part(tfc.build(blocks, kinds))
        assert check(s, blocks, [seq_of(0, 0), seq_of(3, 199)], 0) == 2
        s.clear_part()
        assert raw_fetch(s, [0], 0)[0] == STATE
        assert "resident" in last_error(s)
    finally:
        s.close()


def test_corrupt_streams_are_bad_data_not_reads():
    """Both are caught by a compare before the load: runs that end before
    the requested row, and an entry count whose entries would leave the
    stream."""
    blocks, part = tfc.corrupt_blocks()
    s = Session(0)
    try:
        s.upload_part(part)
        healthy = [seq_of(2, r) for r in (0, 10, 29)]
        assert s.fetch_tags(healthy, 0) == [b"a", b"bb", b"a"]
        # block 0: one run of 10 rows left; rows inside it still resolve
        assert s.fetch_tags([seq_of(0, 0), seq_of(0, 9)], 0) == [b"a", b"a"]
        rc = raw_fetch(s, [seq_of(2, 0), seq_of(0, 15)], 0)[0]
        assert rc == BAD_DATA and "block 0" in last_error(s)
        assert s.fetch_tags(healthy, 0) == [b"a", b"bb", b"a"]
        # block 1: 0xFFFFFF entries claimed
        rc = raw_fetch(s, [seq_of(1, 0)], 0)[0]
        assert rc == BAD_DATA and "block 1" in last_error(s)
        assert s.fetch_tags(healthy, 0) == [b"a", b"bb", b"a"]
    finally:
        s.close()


# ---- not part of an epoch ----
def test_fetch_inside_an_open_epoch_changes_nothing(mixed):
    s, blocks, names = mixed
    lo, hi = tfc.T0 + 10 * tfc.MS, tfc.T0 + 2000 * tfc.MS
    s.configure_rows(VT_INT64, 2, 40, desc=True)
    s.consume(lo, hi)
    plain = [r.astuple() for r in s.scan_rows()]
    ms = s.last_consume_ms()
    assert len(plain) == 40
    s.configure_rows(VT_INT64, 2, 40, desc=True)
    s.consume(lo, hi)
    arbitrary = [seq_of(names["plain3000"], 77), seq_of(names["svc"], 300)]
    assert check(s, blocks, arbitrary, 0) == 2
    assert s.last_consume_ms() == ms
    assert [r.astuple() for r in s.scan_rows()] == plain
    # an aggregate epoch
    funcs = [AGG_SUM, AGG_COUNT, AGG_MIN, AGG_MAX]
    s.configure(VT_INT64, funcs)
    s.consume(lo, hi)
    g = s.finalize()[0]
    want = (g.count, g.sum_i, g.min_i, g.max_i)
    s.configure(VT_INT64, funcs)
    s.consume(lo, hi)
    assert check(s, blocks, arbitrary, 0) == 2
    g = s.finalize()[0]
    assert (g.count, g.sum_i, g.min_i, g.max_i) == want and g.count > 0


# ---- end to end with the selection ----
def fetch_triples(s, rows):
    cols = [s.fetch_tags(rows, sl) for sl in range(3)]
    return [tuple(c[i] for c in cols) for i in range(len(rows))]


def check_selection(s, blocks, conds, rows):
    assert rows
    seqs = [r.seq for r in rows]
    want = list(zip(*[tfc.expect(blocks, seqs, sl) for sl in range(3)]))
    got = fetch_triples(s, rows)
    assert got == want
    for r, t in zip(rows, got):
        b = blocks[r.seq >> 13]
        assert (b.sid, b.ts[r.seq & 8191]) == (r.series_id, r.ts)
        assert fr.row_selected(conds, list(t)), (r.seq, t)
    return len(rows)


def test_row_scan_and_top_n_rows_with_their_tags():
    blocks, kinds, conds = tfc.three_slot_blocks()
    lo, hi = tfc.T0 + 100 * tfc.MS, tfc.T0 + 1800 * tfc.MS
    s = Session(0)
    try:
        s.upload_part(tfc.build(blocks, kinds))
        for desc in (False, True):
            s.configure_rows(VT_INT64, 3, 60, desc=desc)
            s.consume_filter(conds, lo, hi)
            rows = s.scan_rows()
            assert check_selection(s, blocks, conds, rows) == 60
            assert all(lo <= r.ts <= hi for r in rows)
        s.configure_top(VT_INT64, 50)
        s.consume_filter(conds, lo, hi)
        assert check_selection(s, blocks, conds, s.top_rows()) == 50
    finally:
        s.close()


def test_deduped_row_scan_with_its_tags():
    scen = rdc.three_slot_case()
    s = Session(0)
    try:
        s.upload_part(scen.part())
        s.set_row_dedup(1)
        s.configure_rows(VT_INT64, 0, 200, desc=True)
        s.consume_filter(scen.conds)
        rows = s.scan_rows()
        assert check_selection(s, scen.blocks, scen.conds, rows) == 200
        assert len({(r.series_id, r.ts) for r in rows}) == len(rows)
    finally:
        s.close()


# ---- two shards ----
def test_two_shards_merge_with_origin_then_one_fetch_per_shard():
    rng = random.Random(7700)
    shards = []
    for k in range(2):
        blocks = []
        for sid in range(3):
            n = 400
            ts = [tfc.T0 + (2 * i + k) * tfc.MS for i in range(n)]
            blocks.append(rdc.DBlk(
                10 * k + sid + 1, ts, [1] * n, rdc.ivals(rng, n),
                [fc.runs(rng, n, fc.ENVS, maxrun=5, nil_p=0.1),
                 [b"shard%d-%d-%d" % (k, sid, i) for i in range(n)]]))
        shards.append(blocks)
    sessions = []
    try:
        lists = []
        for blocks in shards:
            s = Session(0)
            sessions.append(s)
            s.upload_part(tfc.build(blocks, [(tfc.DICT, tfc.PLAIN)] * 3))
            s.configure_rows(VT_INT64, 0, 30, desc=True)
            s.consume()
            lists.append(s.scan_rows())
        merged, src_l, src_i = ba.rows_merge(lists, 4, 20, desc=True,
                                             with_src=True)
        assert len(merged) == 20 and set(src_l) == {0, 1}
        for slot in (0, 1):
            tags = [None] * len(merged)
            filled = [False] * len(merged)
            for k, s in enumerate(sessions):          # one fetch per shard
                mine = [i for i, l in enumerate(src_l) if l == k]
                vals = s.fetch_tags([lists[k][src_i[i]] for i in mine], slot)
                for i, v in zip(mine, vals):
                    tags[i], filled[i] = v, True
            assert all(filled)
            want = [tfc.expect(shards[l], [r.seq], slot)[0]
                    for r, l in zip(merged, src_l)]
            assert tags == want
            if slot == 1:
                assert all(t.startswith(b"shard%d-" % l)
                           for t, l in zip(tags, src_l))
    finally:
        for s in sessions:
            s.close()


# ---- wire frame ----
def test_rows_and_fetched_tags_through_the_wire_frame():
    blocks, kinds, conds = tfc.three_slot_blocks()
    # a clamp of 22 timestamps (the blocks share them) round a nil env row
    at = next(b.tags[0].index(None) for b in blocks if None in b.tags[0])
    assert 10 <= at < len(blocks[0].ts) - 11
    lo, hi = blocks[0].ts[at - 10], blocks[0].ts[at + 11]
    s = Session(0)
    try:
        s.upload_part(tfc.build(blocks, kinds))
        s.configure_rows(VT_INT64, 0, 64)
        s.consume(lo, hi)
        rows = s.scan_rows()
        assert len(rows) == 64
        env, user, code = [s.fetch_tags(rows, sl) for sl in range(3)]
    finally:
        s.close()
    seqs = [r.seq for r in rows]
    assert [env, user, code] == [tfc.expect(blocks, seqs, sl)
                                 for sl in range(3)]
    assert None in env and None in user        # nil cells reach the frame

    def frame(env, user, code):
        fb = FrameBuilder(len(rows))
        fb.add_i64(ROLE_TIMESTAMP, "ts", "", [r.ts for r in rows])
        fb.add_i64(ROLE_FIELD, "value", "", [r.value_i for r in rows])
        fb.add_tagvalue_str(ROLE_TAG, "env", "default", env)
        fb.add_tagvalue_str(ROLE_TAG, "user", "default", user)
        fb.add_tagvalue_int(ROLE_TAG, "code", "default",
                            [0 if c is None else fr.cell_to_i64(c)
                             for c in code],
                            [1 if c is None else 0 for c in code])
        return fb.finish()
    data = frame(env, user, code)
    assert data == frame(*[tfc.expect(blocks, seqs, sl) for sl in range(3)])
    rd = FrameReader(data)
    assert (rd.nrows, rd.ncols) == (len(rows), 5)
    assert rd.col_i64(0) == [r.ts for r in rows]
    assert rd.col_i64(1) == [r.value_i for r in rows]
    for ci, col in ((2, env), (3, user), (4, code)):
        assert rd.col_nulls(ci) == [v is None for v in col]
    for ci, col in ((2, env), (3, user)):
        cells = rd.col_var(ci)
        for cell, v in zip(cells, col):
            if v is None:
                assert cell is None
            else:
                assert cell.endswith(v) and len(cell) <= len(v) + 4


# ---- the pure-C consumer ----
def test_c_consumer_runs(tmp_path):
    exe = str(tmp_path / "cabi_tag_fetch_check")
    build_consumer(exe)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "tag fetch consumer OK" in out.stdout
