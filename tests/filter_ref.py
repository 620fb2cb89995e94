"""Reference evaluator for the tag filter operators — the per-row match
rules of the reference's TagFilter tree, restated over Python values.

A tag value is bytes or None (nil).  A condition is (op, tag_type,
literals) with literals a list of bytes (int literals as the stored 8-byte
sign-flip cell, convert/number.go:33-46).

  EQ      eqTag.Match (pkg/query/logical/tag_filter.go:426-432): bytes
          equal; nil never matches (nullLiteral.Equal is false)
  NE      notTag(eqTag) (:168, :370-376): true wherever EQ is false,
          nil rows included
  IN      inTag.Match -> BelongTo (:405-411, expr_literal.go:84-92,
          260-268): value equals any list element; nil is false
  NOT_IN  notTag(inTag) (:189): nil is true
  GT GE LT LE  rangeTag.Match (:465-503) with c = literal.Compare(value):
          c<0, c<=0, c>0, c>=0; nil never (Compare gives ok=false).
          string: c = strings.Compare (expr_literal.go:241-246);
          int: c = int(lit - val), WRAPPING int64 (expr_literal.go:65-70);
          a stored value that is not 8 bytes never matches an int range.
Conditions are ANDed (andLogicalNode)."""
import math

from banyandb_amd import (OP_EQ, OP_NE, OP_LT, OP_GT, OP_LE, OP_GE, OP_IN,
                          OP_NOT_IN, TAG_INT)

NEGATED = (OP_NE, OP_NOT_IN)


def cell_to_i64(b):
    u = int.from_bytes(b, "big") ^ (1 << 63)
    return u - (1 << 64) if u >= (1 << 63) else u


def compare(tag_type, lit, val):
    """Sign of literal.Compare(value), or None when not comparable."""
    if tag_type == TAG_INT:
        if len(val) != 8 or len(lit) != 8:
            return None
        d = (cell_to_i64(lit) - cell_to_i64(val)) % (1 << 64)  # Go wraps
        return 0 if d == 0 else (-1 if d >= (1 << 63) else 1)
    return (lit > val) - (lit < val)      # bytes order == strings.Compare


def match(op, tag_type, lits, val):
    if op in (OP_EQ, OP_NE):
        eq = val is not None and val == lits[0]
        return eq if op == OP_EQ else not eq
    if op in (OP_IN, OP_NOT_IN):
        isin = val is not None and val in lits
        return isin if op == OP_IN else not isin
    if val is None:
        return False
    c = compare(tag_type, lits[0], val)
    if c is None:
        return False
    return {OP_GT: c < 0, OP_GE: c <= 0, OP_LT: c > 0, OP_LE: c >= 0}[op]


def row_selected(conds, row_tags):
    """conds: TagCond-like objects (slot, op, tag_type, values); row_tags:
    per-slot value-or-None of one row (missing column = None)."""
    for c in conds:
        v = row_tags[c.slot] if c.slot < len(row_tags) else None
        if not match(c.op, c.tag_type, c.values, v):
            return False
    return True


class Fold:
    """sum / count / min / max over the selected rows (int64 sums wrap)."""

    def __init__(self):
        self.vals = []

    def add(self, v):
        self.vals.append(v)

    @property
    def count(self):
        return len(self.vals)

    @property
    def sum_i(self):
        s = sum(self.vals) % (1 << 64)
        return s - (1 << 64) if s >= (1 << 63) else s

    @property
    def sum_f(self):
        return math.fsum(self.vals)

    @property
    def min(self):
        return min(self.vals)

    @property
    def max(self):
        return max(self.vals)


def select_rows(blocks, conds, min_ts=None, max_ts=None):
    """Yield (block, row index) of every selected row.  blocks: objects
    with .ts, .vals, .tags (list of per-slot value lists)."""
    for b in blocks:
        for i, t in enumerate(b.ts):
            if min_ts is not None and t < min_ts:
                continue
            if max_ts is not None and t > max_ts:
                continue
            if row_selected(conds, [col[i] for col in b.tags]):
                yield b, i


def fold(blocks, conds, min_ts=None, max_ts=None):
    f = Fold()
    for b, i in select_rows(blocks, conds, min_ts, max_ts):
        f.add(b.vals[i])
    return f


def fold_by_tag(blocks, conds, slot, domain, min_ts=None, max_ts=None):
    """Per-row group-by on `slot` over `domain`; nil and out-of-domain rows
    drop (computeKey semantics with a host-supplied domain)."""
    idx = {v: g for g, v in enumerate(domain)}
    out = [Fold() for _ in domain]
    for b, i in select_rows(blocks, conds, min_ts, max_ts):
        v = b.tags[slot][i] if slot < len(b.tags) else None
        if v is not None and v in idx:
            out[idx[v]].add(b.vals[i])
    return out
