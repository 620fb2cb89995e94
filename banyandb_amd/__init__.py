"""banyandb_amd — MI355X-native BanyanDB measure scan+aggregate engine.

Python here is plumbing only (device setup, torch.distributed/RCCL merge,
test drivers).  The product is libbydb_gpu.so: C++ host + HIP/CDNA4 kernels
behind the C-ABI in include/bydb_gpu.h.  On a GPU box the HIP extension is
REQUIRED — if the .so is missing or a GPU call fails, errors are raised
loudly; there is no CPU fallback anywhere in this package.
"""
import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_PKG, "libbydb_gpu.so")

VT_INT64 = 2
VT_FLOAT64 = 3
AGG_SUM, AGG_COUNT, AGG_MIN, AGG_MAX, AGG_MEAN = range(5)
MODE_ALL, MODE_MAP, MODE_REDUCE = range(3)
STREAM_AUTO, STREAM_CACHED, STREAM_STREAMING = range(3)
PACK_AUTO, PACK_OFF, PACK_ON = range(3)
INT64_MIN = -(2 ** 63)
FLOAT_RAW_EXP = -32768  # sessions over nullable float64 columns
INT64_MAX = 2 ** 63 - 1


class BlockDesc(C.Structure):
    # must mirror bydb_block_desc in include/bydb_gpu.h exactly
    _fields_ = [
        ("series_id", C.c_uint64),
        ("count", C.c_uint32),
        ("ts_enc_with_version", C.c_uint8),
        ("version_enc", C.c_uint8),
        ("field_enc", C.c_uint8),
        ("field_vtype", C.c_uint8),
        ("ts_min", C.c_int64),
        ("ts_max", C.c_int64),
        ("version_first", C.c_int64),
        ("field_first", C.c_int64),
        ("exp", C.c_int16),
        ("_pad", C.c_uint8 * 6),
        ("ts_off", C.c_uint64),
        ("ts_len", C.c_uint64),
        ("field_off", C.c_uint64),
        ("field_len", C.c_uint64),
        ("tag_off", C.c_uint64),
        ("tag_len", C.c_uint64),
        ("tag2_off", C.c_uint64),
        ("tag2_len", C.c_uint64),
        ("tag3_off", C.c_uint64),
        ("tag3_len", C.c_uint64),
        ("group_code", C.c_uint32),
        ("_pad2", C.c_uint32),
    ]


class Partial(C.Structure):
    _fields_ = [
        ("sum_i", C.c_int64),
        ("count", C.c_int64),
        ("min_i", C.c_int64),
        ("max_i", C.c_int64),
        ("sum_f", C.c_double),
        ("_pad", C.c_double),
    ]


class Result(C.Structure):
    _fields_ = [
        ("sum_i", C.c_int64),
        ("sum_f", C.c_double),
        ("count", C.c_int64),
        ("min_i", C.c_int64),
        ("max_i", C.c_int64),
        ("min_f", C.c_double),
        ("max_f", C.c_double),
        ("mean_i", C.c_int64),
        ("mean_f", C.c_double),
    ]


# tag filter operators (modelv1.Condition.BinaryOp values) and tag types
OP_EQ, OP_NE, OP_LT, OP_GT, OP_LE, OP_GE = 1, 2, 3, 4, 5, 6
OP_IN, OP_NOT_IN = 9, 10
TAG_STRING, TAG_INT = 1, 2
FILTER_MAX_CONDS = 8
TOP_ROWS_MAX = 1024
TAG_FETCH_MAX = TOP_ROWS_MAX   # rows per fetch_tags call
ERR_OOM = -7
ORDER_TS_ASC, ORDER_TS_DESC = 0, 1


class TopRow(C.Structure):
    """One data point of a raw-row top-N (bydb_top_row).  value_i: the int64
    value, or a float64 row's decimal mantissa in its own block's exponent;
    value_f: the restored float64 (0.0 for int64 fields); seq: storage order,
    (block << 13) | row."""
    _fields_ = [
        ("series_id", C.c_uint64),
        ("ts", C.c_int64),
        ("version", C.c_int64),
        ("value_i", C.c_int64),
        ("value_f", C.c_double),
        ("seq", C.c_uint64),
    ]

    def astuple(self):
        return (self.series_id, self.ts, self.version, self.value_i,
                self.value_f, self.seq)

FILTER_MAX_VALUES = 4096


class TagCondC(C.Structure):
    # must mirror bydb_tag_cond in include/bydb_gpu.h exactly
    _fields_ = [
        ("slot", C.c_int32),
        ("op", C.c_int32),
        ("tag_type", C.c_int32),
        ("n_values", C.c_uint32),
        ("values", C.POINTER(C.c_uint8)),
        ("value_offs", C.POINTER(C.c_uint64)),
    ]


class TagCond:
    """One tag condition for Session.consume_filter: `op` (OP_*) on the
    block tag slot 0-2, literal value(s) as stored bytes.  Int literals
    may be given as Python ints with tag_type=TAG_INT; they are stored as
    i64_tag_cell bytes.  IN / NOT_IN take a list, every other op one
    value."""

    def __init__(self, slot, op, values, tag_type=TAG_STRING):
        if isinstance(values, (bytes, int)):
            values = [values]
        self.slot = slot
        self.op = op
        self.tag_type = tag_type
        self.values = [i64_tag_cell(v) if isinstance(v, int) else bytes(v)
                       for v in values]


# criteria tree nodes (AND / OR = modelv1.LogicalExpression.LogicalOp)
NODE_LEAF, NODE_AND, NODE_OR = 0, 1, 2


class FilterNodeC(C.Structure):
    # must mirror bydb_filter_node in include/bydb_gpu.h exactly
    _fields_ = [
        ("op", C.c_int32),
        ("left", C.c_int32),
        ("right", C.c_int32),
    ]


class TreeNode:
    """Binary AND / OR node of a criteria tree; children are TagCond leaves
    or TreeNodes."""

    def __init__(self, op, left, right):
        self.op = op
        self.left = left
        self.right = right


def _fold_nodes(op, children):
    if not children:
        raise ValueError("And / Or need at least one child")
    node = children[0]
    for c in children[1:]:      # left fold, as isMatch merges its sub-nodes
        node = TreeNode(op, node, c)
    return node


def And(*children):
    """AND of TagCond leaves / sub-trees, folded left into binary nodes."""
    return _fold_nodes(NODE_AND, children)


def Or(*children):
    """OR of TagCond leaves / sub-trees, folded left into binary nodes."""
    return _fold_nodes(NODE_OR, children)


def flatten_tree(tree):
    """(conds, nodes) of a criteria tree: conditions in leaf order and
    (op, left, right) nodes in post-order, the bydb_filter_node encoding.
    None is the empty tree ([], [])."""
    conds, nodes = [], []

    def walk(t):
        if isinstance(t, TagCond):
            conds.append(t)
            nodes.append((NODE_LEAF, len(conds) - 1, 0))
        else:
            left = walk(t.left)
            right = walk(t.right)
            nodes.append((t.op, left, right))
        return len(nodes) - 1

    if tree is not None:
        walk(tree)
    return conds, nodes


def _nodes_c(nodes):
    arr = (FilterNodeC * max(len(nodes), 1))()
    for i, (op, left, right) in enumerate(nodes):
        arr[i].op, arr[i].left, arr[i].right = op, left, right
    return arr


def _conds_c(conds):
    """TagCondC array of TagCond objects plus the buffers it points into."""
    arr = (TagCondC * max(len(conds), 1))()
    keep = []
    for i, c in enumerate(conds):
        blob = b"".join(c.values)
        offs = [0]
        for v in c.values:
            offs.append(offs[-1] + len(v))
        buf = (C.c_uint8 * max(len(blob), 1)).from_buffer_copy(blob or b"\0")
        oa = (C.c_uint64 * len(offs))(*offs)
        keep.append((buf, oa))
        arr[i].slot = c.slot
        arr[i].op = c.op
        arr[i].tag_type = c.tag_type
        arr[i].n_values = len(c.values)
        arr[i].values = C.cast(buf, C.POINTER(C.c_uint8))
        arr[i].value_offs = oa
    return arr, keep


def filter_tree_table(tree):
    """The 256-bit truth table of a criteria tree as a Python int: bit sig
    is the tree's result when leaf i (in leaf order) evaluates to bit i of
    sig.  Pure host; raises ValueError on a malformed tree."""
    conds, nodes = flatten_tree(tree)
    return filter_nodes_table(nodes, len(conds))


def filter_nodes_table(nodes, n_conds):
    """filter_tree_table over raw (op, left, right) nodes."""
    out = (C.c_uint64 * 4)()
    rc = _lib.bydb_filter_tree_table(_nodes_c(nodes), len(nodes), n_conds, out)
    if rc != 0:
        raise ValueError(f"bydb_filter_tree_table rc={rc}")
    return sum(int(out[w]) << (64 * w) for w in range(4))


def field_pack_plan(descs):
    """The slot planner of the nibble-packed dense field streams over a list
    of BlockDesc: ([slot_off], [slot_len], arena_bytes); slot_len 0 marks a
    block that is no candidate.  Pure host."""
    n = len(descs)
    arr = (BlockDesc * max(n, 1))(*descs)
    offs = (C.c_uint64 * max(n, 1))()
    lens = (C.c_uint32 * max(n, 1))()
    arena = C.c_uint64(0)
    rc = _lib.bydb_field_pack_plan(arr, n, offs, lens, C.byref(arena))
    if rc != 0:
        raise ValueError(f"bydb_field_pack_plan rc={rc}")
    return ([int(offs[i]) for i in range(n)],
            [int(lens[i]) for i in range(n)], int(arena.value))


def row_dedup_peers(descs):
    """The overlap planner of the cross-part version dedup over a list of
    BlockDesc (only series_id, ts_min and ts_max are read): per block the
    ascending list of blocks of the same series whose [ts_min, ts_max]
    intersects its own.  Pure host."""
    n = len(descs)
    arr = (BlockDesc * max(n, 1))(*descs)
    offs = (C.c_uint64 * (n + 1))()
    need = C.c_uint64(0)
    rc = _lib.bydb_row_dedup_peers(arr, n, offs, None, 0, C.byref(need))
    if rc not in (0, -7):
        raise ValueError(f"bydb_row_dedup_peers rc={rc}")
    peers = (C.c_uint32 * max(need.value, 1))()
    rc = _lib.bydb_row_dedup_peers(arr, n, offs, peers, need.value,
                                   C.byref(need))
    if rc != 0:
        raise ValueError(f"bydb_row_dedup_peers rc={rc}")
    return [[int(peers[k]) for k in range(offs[i], offs[i + 1])]
            for i in range(n)]


def _build_if_possible():
    from banyandb_amd.build import build
    return build(verbose=False)


def _load():
    # Load torch's bundled HIP runtime FIRST: our .so and torch both carry
    # libamdhip64 with the same soname; whichever loads first is reused by
    # the other.  The engine runs fine on torch's runtime, but torch breaks
    # on the system one — so pin the order here (observed on the MI355X
    # box: torch-first OK both ways, engine-first torch.cuda dead).
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    if not os.path.exists(_SO):
        try:
            _build_if_possible()
        except Exception as e:  # loud: no silent fallback
            raise RuntimeError(
                f"libbydb_gpu.so missing and build failed: {e}. "
                "Run `python banyandb_amd/build.py`."
            ) from e
    lib = C.CDLL(_SO)
    u8p = C.POINTER(C.c_uint8)
    i64p = C.POINTER(C.c_int64)
    f64p = C.POINTER(C.c_double)
    bp = C.POINTER(BlockDesc)

    lib.bydb_session_create.restype = C.c_void_p
    lib.bydb_session_create.argtypes = [C.c_int]
    lib.bydb_session_destroy.argtypes = [C.c_void_p]
    lib.bydb_last_error.restype = C.c_char_p
    lib.bydb_last_error.argtypes = [C.c_void_p]
    lib.bydb_part_reserve.restype = C.c_int
    lib.bydb_part_reserve.argtypes = [C.c_void_p, C.c_uint64, C.c_int64]
    lib.bydb_part_append.restype = C.c_int
    lib.bydb_part_append.argtypes = [C.c_void_p, u8p, C.c_uint64, bp, C.c_int64]
    lib.bydb_part_clear.restype = C.c_int
    lib.bydb_part_clear.argtypes = [C.c_void_p]
    lib.bydb_agg_configure.restype = C.c_int
    lib.bydb_agg_configure.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_int]
    lib.bydb_agg_configure_by_tags.restype = C.c_int
    lib.bydb_agg_configure_by_tags.argtypes = [C.c_void_p, C.c_int, C.c_uint32,
                                               C.POINTER(C.c_int), C.c_int,
                                               C.POINTER(u8p),
                                               C.POINTER(C.POINTER(C.c_uint64)),
                                               C.POINTER(C.c_uint32), C.c_int]
    lib.bydb_agg_configure_by_tag.restype = C.c_int
    lib.bydb_agg_configure_by_tag.argtypes = [C.c_void_p, C.c_int, C.c_uint32,
                                              C.c_int, u8p,
                                              C.POINTER(C.c_uint64), C.c_uint32,
                                              C.c_int]
    lib.bydb_set_partials_buffer.restype = C.c_int
    lib.bydb_set_partials_buffer.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    lib.bydb_reset.restype = C.c_int
    lib.bydb_reset.argtypes = [C.c_void_p]
    lib.bydb_consume.restype = C.c_int
    lib.bydb_consume.argtypes = [C.c_void_p, C.c_int64, C.c_int64, u8p, C.c_uint64]
    lib.bydb_consume_multi.restype = C.c_int
    lib.bydb_consume_multi.argtypes = [C.c_void_p, C.c_int64, C.c_int64,
                                       C.POINTER(u8p), C.POINTER(C.c_uint64),
                                       C.c_int]
    lib.bydb_consume_filter.restype = C.c_int
    lib.bydb_consume_filter.argtypes = [C.c_void_p, C.c_int64, C.c_int64,
                                        C.POINTER(TagCondC), C.c_int]
    lib.bydb_consume_filter_tree.restype = C.c_int
    lib.bydb_consume_filter_tree.argtypes = [C.c_void_p, C.c_int64, C.c_int64,
                                             C.POINTER(TagCondC), C.c_int,
                                             C.POINTER(FilterNodeC), C.c_int]
    lib.bydb_filter_tree_table.restype = C.c_int
    lib.bydb_filter_tree_table.argtypes = [C.POINTER(FilterNodeC), C.c_int,
                                           C.c_int, C.POINTER(C.c_uint64)]
    lib.bydb_filter_tree_stats.restype = C.c_int
    lib.bydb_filter_tree_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    lib.bydb_set_row_dedup.restype = C.c_int
    lib.bydb_set_row_dedup.argtypes = [C.c_void_p, C.c_int]
    lib.bydb_row_dedup_stats.restype = C.c_int
    lib.bydb_row_dedup_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    lib.bydb_row_dedup_peers.restype = C.c_int
    lib.bydb_row_dedup_peers.argtypes = [bp, C.c_int64,
                                         C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint32), C.c_uint64,
                                         C.POINTER(C.c_uint64)]
    lib.bydb_finalize.restype = C.c_int
    lib.bydb_finalize.argtypes = [C.c_void_p, C.POINTER(Result), C.c_int64]
    lib.bydb_finalize_partials.restype = C.c_int
    lib.bydb_finalize_partials.argtypes = [C.c_void_p, C.POINTER(Partial), C.c_int64]
    lib.bydb_set_float_exp.restype = C.c_int
    lib.bydb_set_float_exp.argtypes = [C.c_void_p, C.c_int16]
    lib.bydb_set_stream_policy.restype = C.c_int
    lib.bydb_set_stream_policy.argtypes = [C.c_void_p, C.c_int]
    lib.bydb_stream_policy_pick.restype = C.c_int
    lib.bydb_stream_policy_pick.argtypes = [C.c_int, C.c_uint64]
    lib.bydb_set_field_pack.restype = C.c_int
    lib.bydb_set_field_pack.argtypes = [C.c_void_p, C.c_int]
    lib.bydb_field_pack_stats.restype = C.c_int
    lib.bydb_field_pack_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    lib.bydb_field_pack_plan.restype = C.c_int
    lib.bydb_field_pack_plan.argtypes = [bp, C.c_int64,
                                         C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint32),
                                         C.POINTER(C.c_uint64)]
    lib.bydb_last_consume_ms.restype = C.c_double
    lib.bydb_last_consume_ms.argtypes = [C.c_void_p]
    lib.bydb_group_first_seen.restype = C.c_int
    lib.bydb_group_first_seen.argtypes = [C.c_void_p, C.POINTER(C.c_uint64),
                                          C.c_int64]
    lib.bydb_top_configure.restype = C.c_int
    lib.bydb_top_configure.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int]
    lib.bydb_top_finalize.restype = C.c_int
    lib.bydb_top_finalize.argtypes = [C.c_void_p, C.POINTER(TopRow), C.c_int64,
                                      C.POINTER(C.c_int64)]
    lib.bydb_top_rows_merge.restype = C.c_int
    lib.bydb_top_rows_merge.argtypes = [C.POINTER(C.POINTER(TopRow)),
                                        C.POINTER(C.c_int64), C.c_int, C.c_int,
                                        C.c_int64, C.c_int, C.POINTER(TopRow),
                                        C.POINTER(C.c_int64)]
    lib.bydb_rows_configure.restype = C.c_int
    lib.bydb_rows_configure.argtypes = [C.c_void_p, C.c_int, C.c_int64,
                                        C.c_int64, C.c_int]
    lib.bydb_rows_finalize.restype = C.c_int
    lib.bydb_rows_finalize.argtypes = [C.c_void_p, C.POINTER(TopRow),
                                       C.c_int64, C.POINTER(C.c_int64)]
    lib.bydb_rows_merge.restype = C.c_int
    lib.bydb_rows_merge.argtypes = [C.POINTER(C.POINTER(TopRow)),
                                    C.POINTER(C.c_int64), C.c_int, C.c_int64,
                                    C.c_int64, C.c_int, C.POINTER(TopRow),
                                    C.POINTER(C.c_int64)]
    lib.bydb_rows_fetch_tags.restype = C.c_int
    lib.bydb_rows_fetch_tags.argtypes = [C.c_void_p, C.POINTER(C.c_uint64),
                                         C.c_int64, C.c_int,
                                         C.POINTER(C.c_uint8), C.c_uint64,
                                         C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint8),
                                         C.POINTER(C.c_uint64)]
    lib.bydb_rows_merge_src.restype = C.c_int
    lib.bydb_rows_merge_src.argtypes = [C.POINTER(C.POINTER(TopRow)),
                                        C.POINTER(C.c_int64), C.c_int,
                                        C.c_int64, C.c_int64, C.c_int,
                                        C.POINTER(TopRow),
                                        C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int64),
                                        C.POINTER(C.c_int64)]
    lib.bydb_top_rows_merge_src.restype = C.c_int
    lib.bydb_top_rows_merge_src.argtypes = [C.POINTER(C.POINTER(TopRow)),
                                            C.POINTER(C.c_int64), C.c_int,
                                            C.c_int, C.c_int64, C.c_int,
                                            C.POINTER(TopRow),
                                            C.POINTER(C.c_int32),
                                            C.POINTER(C.c_int64),
                                            C.POINTER(C.c_int64)]
    lib.bydb_reduce_partials2.restype = C.c_int
    lib.bydb_reduce_partials2.argtypes = [C.POINTER(Partial), C.c_int64, C.c_int64,
                                          C.c_int, C.c_int16, C.POINTER(Result)]

    lib.bydb_part_builder_create.restype = C.c_void_p
    lib.bydb_part_builder_destroy.argtypes = [C.c_void_p]
    lib.bydb_part_builder_error.restype = C.c_char_p
    lib.bydb_part_builder_error.argtypes = [C.c_void_p]
    lib.bydb_part_builder_add_block_f64_nullable.restype = C.c_int
    lib.bydb_part_builder_add_block_f64_nullable.argtypes = [
        C.c_void_p, C.c_uint64, i64p, i64p, C.POINTER(C.c_double), u8p,
        C.c_int64, C.c_uint32]
    lib.bydb_part_builder_add_block_i64_nullable.restype = C.c_int
    lib.bydb_part_builder_add_block_i64_nullable.argtypes = [
        C.c_void_p, C.c_uint64, i64p, i64p, i64p, u8p, C.c_int64, C.c_uint32]
    lib.bydb_part_builder_add_block_i64.restype = C.c_int
    lib.bydb_part_builder_add_block_i64.argtypes = [C.c_void_p, C.c_uint64, i64p,
                                                    i64p, i64p, C.c_int64, C.c_uint32]
    lib.bydb_part_builder_add_block_f64.restype = C.c_int
    lib.bydb_part_builder_add_block_f64.argtypes = [C.c_void_p, C.c_uint64, i64p,
                                                    i64p, f64p, C.c_int64, C.c_uint32]
    lib.bydb_part_builder_set_block_tag.restype = C.c_int
    lib.bydb_part_builder_set_block_tag.argtypes = [C.c_void_p, u8p, i64p, C.c_int64]
    lib.bydb_part_builder_set_tag_table.restype = C.c_int
    lib.bydb_part_builder_set_tag_table.argtypes = [C.c_void_p, C.c_int, u8p, i64p,
                                                    C.c_int64]
    lib.bydb_part_builder_payload_len.restype = C.c_uint64
    lib.bydb_part_builder_payload_len.argtypes = [C.c_void_p]
    lib.bydb_part_builder_payload.restype = u8p
    lib.bydb_part_builder_payload.argtypes = [C.c_void_p]
    lib.bydb_part_builder_n_blocks.restype = C.c_int64
    lib.bydb_part_builder_n_blocks.argtypes = [C.c_void_p]
    lib.bydb_part_builder_blocks.restype = bp
    lib.bydb_part_builder_blocks.argtypes = [C.c_void_p]
    lib.bydb_part_builder_drain.restype = C.c_int
    lib.bydb_part_builder_drain.argtypes = [C.c_void_p]
    lib.bydb_gen_series_i64.restype = C.c_int
    lib.bydb_gen_series_i64.argtypes = [C.c_void_p, C.c_uint64, C.c_int64, C.c_int64,
                                        C.c_int64, C.c_int64, C.c_int64, C.c_uint64,
                                        C.c_uint32]
    lib.bydb_gen_series_f64.restype = C.c_int
    lib.bydb_gen_series_f64.argtypes = [C.c_void_p, C.c_uint64, C.c_int64, C.c_int64,
                                        C.c_int64, C.c_double, C.c_double, C.c_uint64,
                                        C.c_uint32]
    lib.bydb_gen_series_bulk_i64.restype = C.c_int
    lib.bydb_gen_series_bulk_i64.argtypes = [C.c_void_p, C.c_uint64, C.c_int64,
                                             C.c_int64, C.c_int64, C.c_int64,
                                             C.c_int64, C.c_int64, C.c_uint64,
                                             C.c_uint32, C.c_int]
    lib.bydb_part_write_dir.restype = C.c_int
    lib.bydb_part_write_dir.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p,
                                        C.c_char_p, C.POINTER(C.c_char_p), C.c_int]
    lib.bydb_part_read_dir.restype = C.c_int
    lib.bydb_part_read_dir.argtypes = [C.c_void_p, C.c_char_p]
    lib.bydb_gen_series_bulk_f64.restype = C.c_int
    lib.bydb_gen_series_bulk_f64.argtypes = [C.c_void_p, C.c_uint64, C.c_int64,
                                             C.c_int64, C.c_int64, C.c_int64,
                                             C.c_double, C.c_double, C.c_uint64,
                                             C.c_uint32, C.c_int]
    return lib


_lib = _load()


def lib():
    return _lib


class PartBuilder:
    """Host-side fixture writer (mirrors the reference block write path)."""

    def __init__(self):
        self._h = _lib.bydb_part_builder_create()
        if not self._h:
            raise RuntimeError("part builder create failed")

    def _ck(self, rc):
        if rc != 0:
            raise RuntimeError(
                f"part builder error rc={rc}: "
                f"{_lib.bydb_part_builder_error(self._h).decode()}")

    def add_block_i64(self, series_id, ts, versions, vals, group_code=0):
        n = len(ts)
        self._ck(_lib.bydb_part_builder_add_block_i64(
            self._h, series_id, (C.c_int64 * n)(*ts), (C.c_int64 * n)(*versions),
            (C.c_int64 * n)(*vals), n, group_code))

    def add_block_i64_nullable(self, series_id, ts, versions, vals,
                               group_code=0):
        """Null-bearing int64 field column: vals[i] is None for null rows
        (stored as the reference's Plain cell block; the fold skips
        nulls)."""
        n = len(ts)
        valid = (C.c_uint8 * n)(*[0 if v is None else 1 for v in vals])
        vv = (C.c_int64 * n)(*[0 if v is None else v for v in vals])
        self._ck(_lib.bydb_part_builder_add_block_i64_nullable(
            self._h, series_id, (C.c_int64 * n)(*ts),
            (C.c_int64 * n)(*versions), vv, valid, n, group_code))

    def add_block_f64_nullable(self, series_id, ts, versions, vals,
                               group_code=0):
        """Null-bearing float64 column (raw IEEE-754 cells; configure the
        session with float_exp=FLOAT_RAW_EXP)."""
        n = len(ts)
        valid = (C.c_uint8 * n)(*[0 if v is None else 1 for v in vals])
        vv = (C.c_double * n)(*[0.0 if v is None else v for v in vals])
        self._ck(_lib.bydb_part_builder_add_block_f64_nullable(
            self._h, series_id, (C.c_int64 * n)(*ts),
            (C.c_int64 * n)(*versions), vv, valid, n, group_code))

    def add_block_f64(self, series_id, ts, versions, vals, group_code=0):
        n = len(ts)
        self._ck(_lib.bydb_part_builder_add_block_f64(
            self._h, series_id, (C.c_int64 * n)(*ts), (C.c_int64 * n)(*versions),
            (C.c_double * n)(*vals), n, group_code))

    def set_tag_table(self, slot, values):
        """Entity-tag table: generators attach values[series %% len] as a
        constant tag column (slot) to every generated block."""
        data = b"".join(v for v in values if v is not None)
        lens = [(-1 if v is None else len(v)) for v in values]
        buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
        self._ck(_lib.bydb_part_builder_set_tag_table(
            self._h, slot, buf, (C.c_int64 * len(values))(*lens), len(values)))

    def set_block_tag(self, values):
        """values: list of bytes-or-None, one per row of the last block."""
        data = b"".join(v for v in values if v is not None)
        lens = [(-1 if v is None else len(v)) for v in values]
        n = len(values)
        buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
        self._ck(_lib.bydb_part_builder_set_block_tag(
            self._h, buf, (C.c_int64 * n)(*lens), n))

    def gen_series_i64(self, series_index, n_dp, t0, stride_ns, base, ramp,
                       seed, group_code=0):
        self._ck(_lib.bydb_gen_series_i64(self._h, series_index, n_dp, t0,
                                          stride_ns, base, ramp, seed, group_code))

    def gen_series_f64(self, series_index, n_dp, t0, stride_ns, base, ramp,
                       seed, group_code=0):
        self._ck(_lib.bydb_gen_series_f64(self._h, series_index, n_dp, t0,
                                          stride_ns, base, ramp, seed, group_code))

    def gen_bulk_i64(self, first_index, n_series, n_dp, t0, stride_ns,
                     base_step, ramp, seed, group_mod=0, threads=None):
        threads = threads or os.cpu_count() or 8
        self._ck(_lib.bydb_gen_series_bulk_i64(
            self._h, first_index, n_series, n_dp, t0, stride_ns, base_step,
            ramp, seed, group_mod, threads))

    def gen_bulk_f64(self, first_index, n_series, n_dp, t0, stride_ns,
                     base_step, ramp, seed, group_mod=0, threads=None):
        threads = threads or os.cpu_count() or 8
        self._ck(_lib.bydb_gen_series_bulk_f64(
            self._h, first_index, n_series, n_dp, t0, stride_ns, base_step,
            ramp, seed, group_mod, threads))

    @property
    def payload(self) -> bytes:
        n = _lib.bydb_part_builder_payload_len(self._h)
        if n == 0:
            return b""
        ptr = _lib.bydb_part_builder_payload(self._h)
        # NOT string_at: its size argument is a C int, so payloads past
        # 2 GiB would truncate (mod 2^32) silently
        return bytes((C.c_ubyte * n).from_address(
            C.addressof(ptr.contents)))

    @property
    def payload_len(self) -> int:
        return _lib.bydb_part_builder_payload_len(self._h)

    def raw_payload_ptr(self):
        return _lib.bydb_part_builder_payload(self._h)

    @property
    def n_blocks(self) -> int:
        return _lib.bydb_part_builder_n_blocks(self._h)

    def blocks_ptr(self):
        return _lib.bydb_part_builder_blocks(self._h)

    def blocks(self):
        ptr = _lib.bydb_part_builder_blocks(self._h)
        return [ptr[i] for i in range(self.n_blocks)]

    def write_dir(self, path, field_name="value", tag_family="default",
                  tag_names=()):
        """Write the part as a reference-layout on-disk part directory."""
        arr = (C.c_char_p * max(len(tag_names), 1))(
            *[t.encode() for t in tag_names] or [b""])
        self._ck(_lib.bydb_part_write_dir(self._h, path.encode(),
                                          field_name.encode(),
                                          tag_family.encode(), arr,
                                          len(tag_names)))

    def read_dir(self, path):
        """Load a part directory written by write_dir (or the reference)."""
        self._ck(_lib.bydb_part_read_dir(self._h, path.encode()))

    def drain(self):
        self._ck(_lib.bydb_part_builder_drain(self._h))

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.bydb_part_builder_destroy(self._h)
        except Exception:
            pass  # interpreter shutdown
        self._h = None


class Session:
    """GPU session over the C-ABI (BreakerOperator lifecycle)."""

    def __init__(self, device=0):
        self._h = _lib.bydb_session_create(device)
        if not self._h:
            raise RuntimeError(
                "bydb_session_create failed — no GPU visible? The HIP engine "
                "has no CPU fallback.")
        self.n_groups = 1
        self.field_vtype = VT_INT64

    def _ck(self, rc):
        if rc != 0:
            raise RuntimeError(
                f"bydb error rc={rc}: {_lib.bydb_last_error(self._h).decode()}")

    def upload_part(self, builder: PartBuilder):
        self._ck(_lib.bydb_part_reserve(self._h, builder.payload_len,
                                        builder.n_blocks))
        self._ck(_lib.bydb_part_append(self._h, builder.raw_payload_ptr(),
                                       builder.payload_len, builder.blocks_ptr(),
                                       builder.n_blocks))

    def reserve(self, payload_bytes, n_blocks):
        self._ck(_lib.bydb_part_reserve(self._h, payload_bytes, n_blocks))

    def append(self, builder: PartBuilder):
        self._ck(_lib.bydb_part_append(self._h, builder.raw_payload_ptr(),
                                       builder.payload_len, builder.blocks_ptr(),
                                       builder.n_blocks))

    def clear_part(self):
        """Drop the resident part (the reservation is kept)."""
        self._ck(_lib.bydb_part_clear(self._h))

    def configure(self, field_vtype, funcs, n_groups=1, mode=MODE_ALL,
                  float_exp=0):
        mask = 0
        for f in funcs:
            mask |= 1 << f
        self.n_groups = n_groups
        self.field_vtype = field_vtype
        self._ck(_lib.bydb_agg_configure(self._h, field_vtype, mask, n_groups, mode))
        self._ck(_lib.bydb_set_float_exp(self._h, float_exp))

    def configure_by_tag(self, field_vtype, funcs, tag_slot, domain,
                         mode=MODE_ALL, float_exp=0):
        """Per-row group-by on the dictionary tag in tag_slot; group id =
        index into domain (list of bytes values)."""
        mask = 0
        for f in funcs:
            mask |= 1 << f
        blob = b"".join(domain)
        offs = [0]
        for v in domain:
            offs.append(offs[-1] + len(v))
        self.n_groups = len(domain)
        self.field_vtype = field_vtype
        buf = (C.c_uint8 * max(len(blob), 1)).from_buffer_copy(blob or b"\0")
        self._ck(_lib.bydb_agg_configure_by_tag(
            self._h, field_vtype, mask, tag_slot, buf,
            (C.c_uint64 * len(offs))(*offs), len(domain), mode))
        self._ck(_lib.bydb_set_float_exp(self._h, float_exp))

    def configure_by_tags(self, field_vtype, funcs, slots, domains,
                          mode=MODE_ALL, float_exp=0):
        """Composite group-by over multiple dictionary tags; group id =
        g0 + n0*g1 + n0*n1*g2 (domains in slot-list order)."""
        mask = 0
        for f in funcs:
            mask |= 1 << f
        u8p = C.POINTER(C.c_uint8)
        bufs = []
        blob_ptrs = (u8p * len(domains))()
        off_ptrs = (C.POINTER(C.c_uint64) * len(domains))()
        nvals = (C.c_uint32 * len(domains))()
        total = 1
        for i, dom in enumerate(domains):
            blob = b"".join(dom)
            offs = [0]
            for v in dom:
                offs.append(offs[-1] + len(v))
            buf = (C.c_uint8 * max(len(blob), 1)).from_buffer_copy(blob or b"\0")
            oa = (C.c_uint64 * len(offs))(*offs)
            bufs.append((buf, oa))
            blob_ptrs[i] = C.cast(buf, u8p)
            off_ptrs[i] = oa
            nvals[i] = len(dom)
            total *= len(dom)
        self.n_groups = total
        self.field_vtype = field_vtype
        self._ck(_lib.bydb_agg_configure_by_tags(
            self._h, field_vtype, mask, (C.c_int * len(slots))(*slots),
            len(slots), blob_ptrs, off_ptrs, nvals, mode))
        self._ck(_lib.bydb_set_float_exp(self._h, float_exp))

    def configure_top(self, field_vtype, n, asc=False, float_exp=0):
        """Make the session a raw-row BatchTop operator (top.go:30-199): the
        next consume selects the n highest (asc: lowest) field values among
        the rows it would have aggregated; top_rows() returns them.  Equal
        values surface in storage order.  configure*() switches back."""
        self._ck(_lib.bydb_set_float_exp(self._h, float_exp))
        self._ck(_lib.bydb_top_configure(self._h, field_vtype, n,
                                         1 if asc else 0))
        self.n_groups = 1
        self.field_vtype = field_vtype
        self.top_n = n

    def top_rows(self):
        """Finalize a top epoch: at most n TopRow, best first."""
        cap = max(int(self.top_n), 1)
        out = (TopRow * cap)()
        got = C.c_int64(0)
        self._ck(_lib.bydb_top_finalize(self._h, out, cap, C.byref(got)))
        return [out[i] for i in range(got.value)]

    def configure_rows(self, field_vtype, offset, limit, desc=False,
                       float_exp=0):
        """Make the session a Scan -> Limit operator (query.go:913-1026,
        limit.go:81-108): the next consume selects rows [offset, offset +
        limit) of the rows it would have aggregated, ordered by (timestamp,
        descending when `desc`; series_id ascending; storage order);
        scan_rows() returns them.  configure*() switches back."""
        self._ck(_lib.bydb_set_float_exp(self._h, float_exp))
        self._ck(_lib.bydb_rows_configure(
            self._h, field_vtype, offset, limit,
            ORDER_TS_DESC if desc else ORDER_TS_ASC))
        self.n_groups = 1
        self.field_vtype = field_vtype
        self.rows_limit = limit

    def scan_rows(self):
        """Finalize a row-scan epoch: at most `limit` TopRow, in order."""
        cap = max(int(self.rows_limit), 1)
        out = (TopRow * cap)()
        got = C.c_int64(0)
        self._ck(_lib.bydb_rows_finalize(self._h, out, cap, C.byref(got)))
        return [out[i] for i in range(got.value)]

    def fetch_tags(self, seqs_or_rows, slot):
        """Tag values of result rows on one block tag slot (block.go:509-776
        copyTo, query.go:641 mustDecodeTagValue): a list, in request order,
        of the stored cell bytes, None for a nil value (b"" is a real
        value).  Takes the TopRow of top_rows() / scan_rows() or plain seq
        ints, at most TAG_FETCH_MAX a call.  A gather over the resident
        part: it belongs to no epoch and changes none."""
        seqs = [r.seq if isinstance(r, TopRow) else int(r)
                for r in seqs_or_rows]
        n = len(seqs)
        arr = (C.c_uint64 * max(n, 1))(*seqs)
        offs = (C.c_uint64 * (n + 1))()
        nil = (C.c_uint8 * max(n, 1))()
        total = C.c_uint64(0)
        # a first call without a buffer sizes it
        rc = _lib.bydb_rows_fetch_tags(self._h, arr, n, slot, None, 0, offs,
                                       nil, C.byref(total))
        if rc == ERR_OOM and total.value > 0:
            data = (C.c_uint8 * total.value)()
            rc = _lib.bydb_rows_fetch_tags(self._h, arr, n, slot, data,
                                           total.value, offs, nil,
                                           C.byref(total))
        else:
            data = (C.c_uint8 * 1)()
        self._ck(rc)
        raw = bytes(data)
        return [None if nil[i] else raw[offs[i]:offs[i + 1]]
                for i in range(n)]

    def set_partials_buffer(self, dev_ptr, nbytes):
        self._ck(_lib.bydb_set_partials_buffer(self._h, dev_ptr, nbytes))

    def reset(self):
        self._ck(_lib.bydb_reset(self._h))

    def consume(self, min_ts=INT64_MIN, max_ts=INT64_MAX, pred=b"", preds=None):
        if preds is not None:
            bufs = [(C.c_uint8 * max(len(p), 1)).from_buffer_copy(p or b"\0")
                    for p in preds]
            arr = (C.POINTER(C.c_uint8) * len(preds))(
                *[C.cast(b, C.POINTER(C.c_uint8)) for b in bufs])
            lens = (C.c_uint64 * len(preds))(*[len(p) for p in preds])
            self._ck(_lib.bydb_consume_multi(self._h, min_ts, max_ts, arr,
                                             lens, len(preds)))
            return
        buf = (C.c_uint8 * max(len(pred), 1)).from_buffer_copy(pred or b"\0")
        self._ck(_lib.bydb_consume(self._h, min_ts, max_ts, buf, len(pred)))

    def consume_filter(self, conds, min_ts=INT64_MIN, max_ts=INT64_MAX):
        """Scan under ANDed TagCond conditions (EQ, NE, LT, LE, GT, GE, IN,
        NOT_IN); an empty list is an unfiltered scan."""
        arr, _keep = _conds_c(conds)
        self._ck(_lib.bydb_consume_filter(self._h, min_ts, max_ts, arr,
                                          len(conds)))

    def consume_filter_tree(self, tree, min_ts=INT64_MIN, max_ts=INT64_MAX):
        """Scan under an AND / OR criteria tree built with And(...) /
        Or(...) over TagCond leaves (a bare TagCond is a one-leaf tree, None
        an unfiltered scan); at most FILTER_MAX_CONDS leaves."""
        conds, nodes = flatten_tree(tree)
        arr, _keep = _conds_c(conds)
        self._ck(_lib.bydb_consume_filter_tree(
            self._h, min_ts, max_ts, arr, len(conds), _nodes_c(nodes),
            len(nodes)))

    def filter_tree_stats(self):
        """Blocks of the last consume_filter_tree by verdict: [clear, skip,
        code-mask walk, row-bitmap walk]; zeros when the tree had no OR."""
        out = (C.c_uint64 * 4)()
        self._ck(_lib.bydb_filter_tree_stats(self._h, out))
        return [int(x) for x in out]

    def set_row_dedup(self, on):
        """Cross-part version dedup (the measure query's merge,
        banyand/measure/query.go:913-943, 966-1026): with on=1 a row is
        dropped when another resident row of its series and timestamp has
        a greater version, or an equal version and an earlier block.
        Sticky; off by default."""
        self._ck(_lib.bydb_set_row_dedup(self._h, int(on)))

    def row_dedup_stats(self):
        """[overlapping blocks, partially superseded blocks, fully
        superseded blocks, superseded rows] of the resident part; zeros
        before the first consume with dedup on and whenever it is off."""
        out = (C.c_uint64 * 4)()
        self._ck(_lib.bydb_row_dedup_stats(self._h, out))
        return [int(x) for x in out]

    def finalize(self):
        out = (Result * self.n_groups)()
        self._ck(_lib.bydb_finalize(self._h, out, self.n_groups))
        return list(out)

    def finalize_partials(self):
        out = (Partial * self.n_groups)()
        self._ck(_lib.bydb_finalize_partials(self._h, out, self.n_groups))
        return list(out)

    def set_stream_policy(self, policy):
        """STREAM_AUTO (default), STREAM_CACHED or STREAM_STREAMING: how
        the closed-form scan loads the dense delta streams."""
        self._ck(_lib.bydb_set_stream_policy(self._h, policy))

    def set_field_pack(self, mode):
        """PACK_AUTO (default), PACK_OFF or PACK_ON: whether the closed-form
        streaming scan reads a 4-bit copy of the dense delta streams whose
        deltas all lie in [-8, 7]."""
        self._ck(_lib.bydb_set_field_pack(self._h, mode))

    def field_pack_stats(self):
        """[candidate blocks, packed blocks, packed payload bytes, slot
        arena bytes] of the resident part; zeros before the build."""
        out = (C.c_uint64 * 4)()
        self._ck(_lib.bydb_field_pack_stats(self._h, out))
        return [int(x) for x in out]

    def last_consume_ms(self):
        return _lib.bydb_last_consume_ms(self._h)

    def group_first_seen(self):
        """Per-group first-seen keys; sorting group ids by them gives the
        reference first-seen materialisation order (2^64-1 = group never
        entered)."""
        out = (C.c_uint64 * self.n_groups)()
        self._ck(_lib.bydb_group_first_seen(self._h, out, self.n_groups))
        return list(out)

    def groups_in_first_seen_order(self):
        ks = self.group_first_seen()
        return [g for g, k in sorted(enumerate(ks), key=lambda t: t[1])
                if ks[g] != (1 << 64) - 1]

    def close(self):
        if self._h:
            _lib.bydb_session_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


def reduce_partials(parts_flat, n_parts_per_group, n_groups, field_vtype,
                    float_exp=0):
    """Host AggModeReduce combine (aggregation_reduce.go semantics)."""
    arr = (Partial * (n_parts_per_group * n_groups))(*parts_flat)
    out = (Result * n_groups)()
    rc = _lib.bydb_reduce_partials2(arr, n_parts_per_group, n_groups,
                                    field_vtype, float_exp, out)
    if rc != 0:
        raise RuntimeError(f"reduce_partials rc={rc}")
    return list(out)


def _with_src(out, src_l, src_i, got):
    n = got.value
    return ([out[i] for i in range(n)], [src_l[i] for i in range(n)],
            [src_i[i] for i in range(n)])


def top_rows_merge(lists, field_vtype, n, asc=False, with_src=False):
    """Host reduce side of a sharded raw-row top-N: a stable N-way merge of
    per-shard top_rows() results (lists of TopRow).  On equal values the
    earlier list wins, then the smaller seq.  with_src: return (rows,
    list_idx, row_idx) with rows[i] == lists[list_idx[i]][row_idx[i]] — seq
    is shard-local, so this names the session to fetch a row's tags from."""
    arrs = [(TopRow * max(len(l), 1))(*l) for l in lists]
    ptrs = (C.POINTER(TopRow) * max(len(lists), 1))(
        *[C.cast(a, C.POINTER(TopRow)) for a in arrs])
    lens = (C.c_int64 * max(len(lists), 1))(*[len(l) for l in lists])
    total = sum(len(l) for l in lists)
    cap = max(min(total, max(n, 0)), 1)
    out = (TopRow * cap)()
    got = C.c_int64(0)
    if with_src:
        src_l, src_i = (C.c_int32 * cap)(), (C.c_int64 * cap)()
        rc = _lib.bydb_top_rows_merge_src(ptrs, lens, len(lists), field_vtype,
                                          n, 1 if asc else 0, out, src_l,
                                          src_i, C.byref(got))
    else:
        rc = _lib.bydb_top_rows_merge(ptrs, lens, len(lists), field_vtype, n,
                                      1 if asc else 0, out, C.byref(got))
    if rc != 0:
        raise RuntimeError(f"top_rows_merge rc={rc}")
    if with_src:
        return _with_src(out, src_l, src_i, got)
    return [out[i] for i in range(got.value)]


def rows_merge(lists, offset, limit, desc=False, with_src=False):
    """Host reduce side of a sharded row scan: per-shard scan_rows() results
    (each configured with offset 0 and limit offset + limit) merged by
    (timestamp, series_id), the earlier list first on a full tie, then cut
    to [offset, offset + limit).  with_src: as for top_rows_merge."""
    arrs = [(TopRow * max(len(l), 1))(*l) for l in lists]
    ptrs = (C.POINTER(TopRow) * max(len(lists), 1))(
        *[C.cast(a, C.POINTER(TopRow)) for a in arrs])
    lens = (C.c_int64 * max(len(lists), 1))(*[len(l) for l in lists])
    cap = max(limit, 1)
    out = (TopRow * cap)()
    got = C.c_int64(0)
    order = ORDER_TS_DESC if desc else ORDER_TS_ASC
    if with_src:
        src_l, src_i = (C.c_int32 * cap)(), (C.c_int64 * cap)()
        rc = _lib.bydb_rows_merge_src(ptrs, lens, len(lists), offset, limit,
                                      order, out, src_l, src_i, C.byref(got))
    else:
        rc = _lib.bydb_rows_merge(ptrs, lens, len(lists), offset, limit, order,
                                  out, C.byref(got))
    if rc != 0:
        raise RuntimeError(f"rows_merge rc={rc}")
    if with_src:
        return _with_src(out, src_l, src_i, got)
    return [out[i] for i in range(got.value)]


def i64_tag_cell(v: int) -> bytes:
    """Stored bytes of an int64 tag value: the reference's order-preserving
    sign-flip 8-byte BE cell (convert/number.go:33-46 Int64ToBytes) — the
    raw value bytes measure tag columns hold for ValueTypeInt64
    (batch_decode.go:48-53 decodes with convert.BytesToInt64).  Use these
    as tag values / group domains for numeric group keys."""
    u = (v | (1 << 63)) if v >= 0 else ((1 << 63) - (-v)) % (1 << 64)
    return u.to_bytes(8, "big")


def f64_tag_cell(v: float) -> bytes:
    """Stored bytes of a float64 tag value: IEEE-754 big-endian
    (convert/number.go:128-132 Float64ToBytes)."""
    import struct
    return struct.pack(">d", v)
