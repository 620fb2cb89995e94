"""Reference evaluator for AND / OR criteria trees — the reference's
BuildTagFilter tree (pkg/query/logical/tag_filter.go:84-142) restated over
Python values: a node evaluates its children left to right and folds them
with its merge (isMatch :259-274; andLogicalNode.merge :288-295 is all(),
orLogicalNode.merge :323-330 is any()); leaves are filter_ref.match, so
each keeps its own nil rule under either node.

A tree is a TagCond (leaf), a banyandb_amd.TreeNode (what And / Or build),
or None (no criteria: every row)."""
from banyandb_amd import TagCond, NODE_AND, NODE_OR

import filter_ref as fr


def leaves(tree):
    """TagCond leaves in left-to-right order (the condition order
    flatten_tree gives the C-ABI)."""
    if tree is None:
        return []
    if isinstance(tree, TagCond):
        return [tree]
    return leaves(tree.left) + leaves(tree.right)


def has_or(tree):
    if tree is None or isinstance(tree, TagCond):
        return False
    return tree.op == NODE_OR or has_or(tree.left) or has_or(tree.right)


def evaluate(tree, leaf_value):
    """Fold the tree over leaf_value(TagCond) -> bool."""
    if tree is None:
        return True
    if isinstance(tree, TagCond):
        return leaf_value(tree)
    left = evaluate(tree.left, leaf_value)
    right = evaluate(tree.right, leaf_value)
    if tree.op == NODE_AND:
        return left and right
    assert tree.op == NODE_OR, tree.op
    return left or right


def row_selected(tree, row_tags):
    """row_tags: per-slot value-or-None of one row (missing column = None)."""
    def leaf(c):
        v = row_tags[c.slot] if c.slot < len(row_tags) else None
        return fr.match(c.op, c.tag_type, c.values, v)
    return evaluate(tree, leaf)


def truth_table(tree):
    """The 256-bit table as an int: bit sig = the tree's result when leaf i
    (leaf order) evaluates to bit i of sig."""
    ls = leaves(tree)
    index = {id(c): i for i, c in enumerate(ls)}
    table = 0
    for sig in range(1 << len(ls)):
        if evaluate(tree, lambda c: bool((sig >> index[id(c)]) & 1)):
            table |= 1 << sig
    return table


def select_rows(blocks, tree, min_ts=None, max_ts=None):
    """Yield (block, row index) of every selected row.  blocks: objects
    with .ts, .vals, .tags (list of per-slot value lists)."""
    for b in blocks:
        for i, t in enumerate(b.ts):
            if min_ts is not None and t < min_ts:
                continue
            if max_ts is not None and t > max_ts:
                continue
            if row_selected(tree, [col[i] for col in b.tags]):
                yield b, i


def fold(blocks, tree, min_ts=None, max_ts=None):
    f = fr.Fold()
    for b, i in select_rows(blocks, tree, min_ts, max_ts):
        f.add(b.vals[i])
    return f


def fold_by_tags(blocks, tree, slots, domains, min_ts=None, max_ts=None):
    """Composite per-row group-by: gid = g0 + n0*g1 + n0*n1*g2 over the
    domains (slot-list order); a row with a nil or out-of-domain value on
    any grouped slot drops."""
    idx = [{v: g for g, v in enumerate(dom)} for dom in domains]
    total = 1
    for dom in domains:
        total *= len(dom)
    out = [fr.Fold() for _ in range(total)]
    for b, i in select_rows(blocks, tree, min_ts, max_ts):
        gid, mul = 0, 1
        for slot, ix, dom in zip(slots, idx, domains):
            v = b.tags[slot][i] if slot < len(b.tags) else None
            if v is None or v not in ix:
                gid = None
                break
            gid += mul * ix[v]
            mul *= len(dom)
        if gid is not None:
            out[gid].add(b.vals[i])
    return out


def fold_by_tag(blocks, tree, slot, domain, min_ts=None, max_ts=None):
    return fold_by_tags(blocks, tree, [slot], [domain], min_ts, max_ts)
