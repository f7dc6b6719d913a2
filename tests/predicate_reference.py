"""The checker of predicate trees (qsx_select_in, qsx_select_in_char, qsx_bitmap_eval and the host layer's PredicateNode),
in numpy.  TEST INFRASTRUCTURE: nothing here is product code.

The semantics are the reference's, two-valued:

  * a comparison with a NULL operand is not true (types/operations/comparisons/LiteralComparators-inl.hpp:330-370);
  * OR unions the children's matches (expressions/predicate/DisjunctionPredicate.cpp:109-157), AND intersects them;
  * NOT inverts the child's matches inside the filter and the existence map (expressions/predicate/NegationPredicate.cpp:
    70-90) - so NOT (x = 5) SELECTS a row whose x is NULL, unlike SQL's three-valued logic;
  * IN is a disjunction of equalities (query_optimizer/expressions/InValueList.cpp:40-65), NOT IN a negation over it: a NULL
    test value is in no list and therefore selected by NOT IN.  Equality is the type's own ==: NaN is in no list, -0.0
    equals 0.0; on CHAR it is strcmpHelper's (AsciiStringComparators.hpp:218-251): texts end at their first NUL or their width.

A tree is nested tuples:
    ("cmp", attr, op, literal)   op one of "=", "<>", "<", "<=", ">", ">="
    ("in", attr, [literals])
    ("and", [children]) / ("or", [children]) / ("not", child)
`columns[attr]` is a numpy array (numeric, or uint8 of shape (n, width) for CHAR), `nulls.get(attr)` a boolean array or None.

Two evaluations of one definition: `eval_tree` over whole columns and `eval_tree_row` one row at a time with Python values;
tests/test_predicate_reference.py pins one against the other and both against tests/golden/predicate_unittest.json.
`compile_tree` turns a tree into what qsx_bitmap_eval takes (leaf bitmaps + a postfix program, a nullable attribute's null
bitmap as one more leaf) and `eval_program` restates the evaluator over MSB-first bitmap words.
"""
import operator

import numpy as np

from like_reference import field_text, pack_bitmap, unpack_bitmap  # noqa: F401  (re-exported: one bitmap layout for all checkers)

BOOL_AND, BOOL_OR, BOOL_NOT = -1, -2, -3
MAX_BOOL_LEAVES, MAX_BOOL_INSTRS, MAX_BOOL_DEPTH = 32, 64, 8
MAX_IN_LIST = 32
DATE_MASK = np.uint64(0x0000FFFFFFFFFFFF)      # year, month, day of a raw DateLit; the two padding bytes never take part

_OPS = {"=": operator.eq, "<>": operator.ne, "<": operator.lt, "<=": operator.le, ">": operator.gt, ">=": operator.ge}


# ---------------------------------------------------------------------------------------------------------------- leaves
def in_rows(col, literals, negate=False, date=False):
    """((col == some literal) XOR negate) over a numeric stripe: what qsx_select_in computes before the filter.  date: col and
    literals are raw DateLit words, compared by year, month and day."""
    col = np.asarray(col)
    hit = np.zeros(col.shape[0], dtype=bool)
    for lit in literals:
        if date:
            hit |= (col.view(np.uint64) & DATE_MASK) == (np.uint64(int(lit) & 0xFFFFFFFFFFFFFFFF) & DATE_MASK)
        else:
            hit |= col == col.dtype.type(lit)      # numpy's == is IEEE's on floats
    return hit != bool(negate)


def text_equal(field, literal):
    """strcmpHelper equality of a CHAR field's bytes and a literal: both end at their first NUL."""
    return field_text(field) == field_text(literal)


def in_char_rows(col, literals, negate=False):
    col = np.ascontiguousarray(col, dtype=np.uint8)
    wanted = {field_text(lit) for lit in literals}
    hit = np.fromiter((field_text(col[i].tobytes()) in wanted for i in range(col.shape[0])), dtype=bool, count=col.shape[0])
    return hit != bool(negate)


def _is_char(col):
    return col.ndim == 2


def leaf_rows(node, columns):
    """A leaf as a pure function of the rows' stored values (no NULL handling)."""
    kind, attr = node[0], node[1]
    col = columns[attr]
    if kind == "in":
        return in_char_rows(col, node[2]) if _is_char(col) else in_rows(col, node[2])
    op, literal = node[2], node[3]
    if _is_char(col):
        lit = field_text(literal)
        return np.fromiter((_OPS[op](field_text(col[i].tobytes()), lit) for i in range(col.shape[0])), dtype=bool, count=col.shape[0])
    return _OPS[op](col, col.dtype.type(literal))


# ------------------------------------------------------------------------------------------------------------------ trees
def eval_tree(tree, columns, nulls=None, n=None):
    nulls = nulls or {}
    kind = tree[0]
    if kind in ("cmp", "in"):
        rows = leaf_rows(tree, columns)
        null = nulls.get(tree[1])
        return rows & ~np.asarray(null, dtype=bool) if null is not None else rows
    if kind == "not":
        return ~eval_tree(tree[1], columns, nulls)
    parts = [eval_tree(child, columns, nulls) for child in tree[1]]
    out = parts[0].copy()
    for part in parts[1:]:
        out = (out & part) if kind == "and" else (out | part)
    return out


def _value(columns, attr, i):
    col = columns[attr]
    return field_text(col[i].tobytes()) if _is_char(col) else col[i].item()


def eval_tree_row(tree, columns, nulls, i):
    """The same, one row at a time on Python values: a second implementation to pin the first."""
    kind = tree[0]
    if kind in ("cmp", "in"):
        null = (nulls or {}).get(tree[1])
        if null is not None and null[i]:
            return False                                        # a NULL operand: not true
        value = _value(columns, tree[1], i)
        if kind == "in":
            return any(value == (field_text(lit) if isinstance(value, bytes) else columns[tree[1]].dtype.type(lit).item())
                       for lit in tree[2])
        literal = field_text(tree[3]) if isinstance(value, bytes) else columns[tree[1]].dtype.type(tree[3]).item()
        return bool(_OPS[tree[2]](value, literal))
    if kind == "not":
        return not eval_tree_row(tree[1], columns, nulls, i)
    results = [eval_tree_row(child, columns, nulls, i) for child in tree[1]]
    return all(results) if kind == "and" else any(results)


def tree_attributes(tree):
    if tree[0] in ("cmp", "in"):
        return {tree[1]}
    if tree[0] == "not":
        return tree_attributes(tree[1])
    return set().union(*[tree_attributes(child) for child in tree[1]])


def _leaf_key(node):
    return (node[0], node[1], tuple(node[2]) if node[0] == "in" else node[2], None if node[0] == "in" else node[3])


def compile_tree(tree, nullable=()):
    """-> (leaves, program): leaves is a list of ("leaf", node) / ("null", attr), program the postfix codes.  Identical leaves
    are one leaf; a nullable attribute's null bitmap is one leaf, and every leaf over it becomes `leaf AND NOT null`."""
    leaves, index, program = [], {}, []

    def leaf(key, entry):
        if key not in index:
            index[key] = len(leaves)
            leaves.append(entry)
        return index[key]

    def walk(node):
        kind = node[0]
        if kind in ("cmp", "in"):
            program.append(leaf(_leaf_key(node), ("leaf", node)))
            if node[1] in nullable:
                program.extend([leaf(("null", node[1]), ("null", node[1])), BOOL_NOT, BOOL_AND])
        elif kind == "not":
            walk(node[1])
            program.append(BOOL_NOT)
        else:
            for k, child in enumerate(node[1]):
                walk(child)
                if k:
                    program.append(BOOL_AND if kind == "and" else BOOL_OR)

    walk(tree)
    return leaves, program


def program_ok(num_leaves, program):
    """What qsx_bitmap_eval accepts: known codes, leaves below num_leaves, no underflow, at most MAX_BOOL_DEPTH values on the
    stack, exactly one at the end, 1..MAX_BOOL_INSTRS instructions."""
    if not 1 <= num_leaves <= MAX_BOOL_LEAVES or not 1 <= len(program) <= MAX_BOOL_INSTRS:
        return False
    depth = 0
    for code in program:
        if code >= 0:
            depth += 1
            if code >= num_leaves or depth > MAX_BOOL_DEPTH:
                return False
        elif code == BOOL_NOT:
            if depth < 1:
                return False
        elif code in (BOOL_AND, BOOL_OR):
            if depth < 2:
                return False
            depth -= 1
        else:
            return False
    return depth == 1


def program_depth(program):
    depth = deepest = 0
    for code in program:
        depth += 1 if code >= 0 else (-1 if code in (BOOL_AND, BOOL_OR) else 0)
        deepest = max(deepest, depth)
    return deepest


def eval_program(leaves, program, n, filter_words=None):
    """The evaluator over MSB-first uint64 words: leaves[k] is an array of (n+63)//64 words or None (all zero).  Returns
    (words, count): the single value left on the stack, ANDed with the filter, bits at positions >= n cleared."""
    assert program_ok(len(leaves), program)
    words = (n + 63) // 64
    stack = []
    for code in program:
        if code >= 0:
            stack.append(np.zeros(words, dtype=np.uint64) if leaves[code] is None
                         else np.ascontiguousarray(leaves[code], dtype=np.uint64)[:words].copy())
        elif code == BOOL_NOT:
            stack.append(~stack.pop())
        else:
            b, a = stack.pop(), stack.pop()
            stack.append((a & b) if code == BOOL_AND else (a | b))
    out = stack.pop()
    if filter_words is not None:
        out = out & np.ascontiguousarray(filter_words, dtype=np.uint64)[:words]
    if n % 64:
        out[-1] &= np.uint64((0xFFFFFFFFFFFFFFFF << (64 - n % 64)) & 0xFFFFFFFFFFFFFFFF)
    return out, int(sum(bin(int(w)).count("1") for w in out))


def random_program(rng, num_leaves, length=None, want_depth=None):
    """A valid random postfix program of exactly `length` codes (default: random, 1..MAX_BOOL_INSTRS) over num_leaves leaves.
    want_depth: its deepest stack is exactly that (the program begins with that many pushes)."""
    max_depth = want_depth or MAX_BOOL_DEPTH
    if length is None:
        length = int(rng.integers(2 * want_depth - 1 if want_depth else 1, MAX_BOOL_INSTRS + 1))
    program, depth = [], 0
    while len(program) < length:
        remaining = length - len(program)
        if want_depth and len(program) < want_depth:
            options = ["push"]
        elif depth >= 1 and depth - 1 == remaining:
            options = ["binary"]                    # just enough room left to come back to one value
        else:
            options = []
            if depth < max_depth and depth <= remaining - 1:
                options.append("push")
            if depth >= 2:
                options.append("binary")
            if depth >= 1 and depth - 1 <= remaining - 1:
                options.append("not")
        pick = options[int(rng.integers(0, len(options)))]
        if pick == "push":
            program.append(int(rng.integers(0, num_leaves)))
            depth += 1
        elif pick == "binary":
            program.append(BOOL_AND if rng.random() < 0.5 else BOOL_OR)
            depth -= 1
        else:
            program.append(BOOL_NOT)
    assert program_ok(num_leaves, program) and (want_depth is None or program_depth(program) == want_depth)
    return program


def random_tree(rng, attrs, depth=3):
    """A random tree over INT attributes `attrs` with literals 0..7."""
    if depth == 0 or rng.random() < 0.3:
        attr = attrs[int(rng.integers(0, len(attrs)))]
        if rng.random() < 0.4:
            return ("in", attr, [int(v) for v in rng.integers(0, 8, size=int(rng.integers(1, 5)))])
        return ("cmp", attr, list(_OPS)[int(rng.integers(0, 6))], int(rng.integers(0, 8)))
    kind = ("and", "or", "not")[int(rng.integers(0, 3))]
    if kind == "not":
        return ("not", random_tree(rng, attrs, depth - 1))
    return (kind, [random_tree(rng, attrs, depth - 1) for _ in range(int(rng.integers(2, 4)))])
