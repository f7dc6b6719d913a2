"""ctypes mirror of the descriptor structs and enums of include/qsx.h.

Shared by the product binding (quickstep_amd.capi) and by the test-only CPU
checker's binding so that a test hands the *same* descriptor bytes to both
sides.  Pure data definitions: no library is loaded here.
"""
import ctypes as C

# qsx_type_t (numbering of types/TypeID.hpp:32-43 in the reference)
ACC_SUM_F64, ACC_SUM_I64, ACC_MIN_I64, ACC_MAX_I64 = 0, 1, 2, 3      # qsx_agg_state_image_layout column kinds
ABI_VERSION = 19                                                    # QSX_ABI_VERSION of include/qsx.h
INT, LONG, FLOAT, DOUBLE, CHAR = 0, 1, 2, 3, 4
DATE = 6   # the reference's 8-byte DateLit {int32 year; uint8 month, day; 2 bytes padding}, carried as int64 raw bytes
# qsx_cmp_t (types/operations/comparisons/ComparisonID.hpp:36-42)
EQ, NE, LT, LE, GT, GE = range(6)
CODE_EQ, CODE_NE, CODE_LT, CODE_GE, CODE_RANGE = range(5)            # qsx_code_cmp_t
MAX_LIKE_PATTERN = 64                                               # QSX_MAX_LIKE_PATTERN (qsx_select_like)
MAX_CHAR_LITERAL = 64                                               # QSX_MAX_CHAR_LITERAL (qsx_select_cmp_char, qsx_select_in_char)
MAX_IN_LIST = 32                                                    # QSX_MAX_IN_LIST (qsx_select_in, qsx_select_in_char)
MAX_BOOL_LEAVES, MAX_BOOL_INSTRS, MAX_BOOL_DEPTH = 32, 64, 8        # QSX_MAX_BOOL_* (qsx_bitmap_eval)
BOOL_AND, BOOL_OR, BOOL_NOT = -1, -2, -3                            # QSX_BOOL_* postfix codes of qsx_bitmap_eval
DATE_YEAR, DATE_MONTH = 0, 1                                        # QSX_DATE_YEAR / QSX_DATE_MONTH (qsx_eval_date_extract)
UNARY_DATE_FIELD, UNARY_SUBSTRING = 0, 1                            # QSX_UNARY_* (qsx_select_cmp_unary, qsx_select_in_unary)
# qsx_agg_strategy_t
AGG_SINGLE_STATE, AGG_COMPACT_KEY, AGG_COLLISION_FREE, AGG_GENERIC = range(4)
# qsx_agg_fn_t
AGG_COUNT_STAR, AGG_SUM, AGG_AVG, AGG_MIN, AGG_MAX, AGG_COUNT = range(6)
# qsx_operand_kind_t
OPD_COLUMN, OPD_CONST, OPD_TEMP = range(3)
OPD_NULL = 3                                                        # QSX_OPD_NULL: the NULL literal, a branch value of qsx_eval_case only
# qsx_expr_op_t
EX_ADD, EX_SUB, EX_MUL, EX_DIV = range(4)
EX_IADD, EX_ISUB, EX_IMUL, EX_IDIV = range(4, 8)                    # the same in integer arithmetic (include/qsx.h)
# qsx_lip_kind_t
LIP_SINGLE_IDENTITY_HASH, LIP_BITVECTOR_EXACT = range(2)

MAX_COLUMNS, MAX_KEYS, MAX_AGGS, MAX_INSTRS, MAX_TEMPS, MAX_CONSTS, MAX_PRED_TERMS = 16, 4, 8, 16, 8, 8, 4
MAX_CASE_WHENS = 8                                                  # QSX_MAX_CASE_WHENS

TYPE_WIDTH = {INT: 4, LONG: 8, FLOAT: 4, DOUBLE: 8, DATE: 8}


def date_raw(year, month, day, padding=0):
    """The 8 bytes of a DateLit as a (signed) 64-bit integer; `padding` fills the two unused bytes."""
    v = (int(year) & 0xFFFFFFFF) | (int(month) & 0xFF) << 32 | (int(day) & 0xFF) << 40 | (int(padding) & 0xFFFF) << 48
    return v - (1 << 64) if v >= 1 << 63 else v

# status codes
OK = 0
ERR_INVALID_ARGUMENT, ERR_NO_DEVICE, ERR_OUT_OF_MEMORY, ERR_HIP = -1, -2, -3, -4
ERR_CAPACITY, ERR_UNSUPPORTED, ERR_TOO_MANY_GROUPS, ERR_HASH_COLLISION, ERR_COMM = -5, -6, -7, -8, -9
GROUPS_HASH_COLLISION = -1   # qsx_agg_finalize's group count when a wide-key state saw two keys under one hash


class Operand(C.Structure):
    _fields_ = [("kind", C.c_int32), ("index", C.c_int32)]


class UnaryOperand(C.Structure):
    """qsx_unary_operand_t: the left operand of qsx_select_cmp_unary / qsx_select_in_unary."""
    _fields_ = [("kind", C.c_int32), ("unit", C.c_int32), ("start", C.c_int32), ("length", C.c_int32)]


def date_field(unit):
    """EXTRACT(unit FROM date) as a predicate's operand: unit is DATE_YEAR or DATE_MONTH."""
    return UnaryOperand(UNARY_DATE_FIELD, int(unit), 0, 0)


def substring_of(start, length):
    """SUBSTRING(char FROM start + 1 FOR length) as a predicate's operand: start is 0-based."""
    return UnaryOperand(UNARY_SUBSTRING, 0, int(start), int(length))


class ExprInstr(C.Structure):
    _fields_ = [("op", C.c_int32), ("dst", C.c_int32), ("a", Operand), ("b", Operand)]


class AggDesc(C.Structure):
    _fields_ = [("fn", C.c_int32), ("arg", Operand)]


class CaseDesc(C.Structure):                                         # qsx_case_desc_t
    _fields_ = [("num_whens", C.c_int32), ("value", Operand * (MAX_CASE_WHENS + 1)), ("out_type", C.c_int32)]


class PredLiteral(C.Union):
    _fields_ = [("i32", C.c_int32), ("i64", C.c_int64), ("f32", C.c_float), ("f64", C.c_double)]


class PredTerm(C.Structure):
    _fields_ = [("column", C.c_int32), ("op", C.c_int32), ("literal", PredLiteral)]


class AggConfig(C.Structure):
    _fields_ = [
        ("strategy", C.c_int32),
        ("num_columns", C.c_int32),
        ("column_type", C.c_int32 * MAX_COLUMNS),
        ("column_width", C.c_int32 * MAX_COLUMNS),
        ("num_keys", C.c_int32),
        ("key_column", C.c_int32 * MAX_KEYS),
        ("num_instrs", C.c_int32),
        ("instrs", ExprInstr * MAX_INSTRS),
        ("consts", C.c_double * MAX_CONSTS),
        ("num_aggs", C.c_int32),
        ("aggs", AggDesc * MAX_AGGS),
        ("num_pred_terms", C.c_int32),
        ("pred", PredTerm * MAX_PRED_TERMS),
        ("est_groups", C.c_int64),
        ("num_entries", C.c_int64),
        ("column_code_width", C.c_int32 * MAX_COLUMNS),
        ("column_nullable", C.c_int32 * MAX_COLUMNS),
    ]


def col(i):
    return Operand(OPD_COLUMN, i)


def const(i):
    return Operand(OPD_CONST, i)


def temp(i):
    return Operand(OPD_TEMP, i)


def null():
    return Operand(OPD_NULL, 0)


def make_case_desc(values, out_type):
    """qsx_case_desc_t: values = the THEN operand of every WHEN, then the ELSE operand (T.null(): NULL)."""
    d = CaseDesc()
    d.num_whens = len(values) - 1
    for k, v in enumerate(values[:MAX_CASE_WHENS + 1]):
        d.value[k] = v
    d.out_type = out_type
    return d


def make_agg_config(strategy, columns, keys=(), instrs=(), consts=(), aggs=(), pred=(),
                    est_groups=0, num_entries=0, code_widths=None, nullable=()):
    """Build an AggConfig.

    columns: list of (type, width) — width may be None for numeric types
    keys:    list of column indices (GROUP BY order)
    instrs:  list of (op, dst, Operand a, Operand b)
    aggs:    list of (fn, Operand-or-None)
    pred:    list of (column, cmp, literal)
    nullable: column indices whose attribute type is nullable (their null bitmaps go to update_nullable)
    """
    cfg = AggConfig()
    cfg.strategy = strategy
    cfg.num_columns = len(columns)
    for i, (t, w) in enumerate(columns):
        cfg.column_type[i] = t
        cfg.column_width[i] = TYPE_WIDTH[t] if w is None else w
    cfg.num_keys = len(keys)
    for i, k in enumerate(keys):
        cfg.key_column[i] = k
    cfg.num_instrs = len(instrs)
    for i, (op, dst, a, b) in enumerate(instrs):
        cfg.instrs[i] = ExprInstr(op, dst, a, b)
    for i, v in enumerate(consts):
        cfg.consts[i] = v
    cfg.num_aggs = len(aggs)
    for i, (fn, arg) in enumerate(aggs):
        cfg.aggs[i] = AggDesc(fn, arg if arg is not None else Operand(OPD_COLUMN, 0))
    cfg.num_pred_terms = len(pred)
    for i, (column, op, literal) in enumerate(pred):
        term = PredTerm()
        term.column = column
        term.op = op
        t = columns[column][0]
        if t == INT:
            term.literal.i32 = int(literal)
        elif t in (LONG, DATE):
            term.literal.i64 = int(literal)
        elif t == FLOAT:
            term.literal.f32 = float(literal)
        else:
            term.literal.f64 = float(literal)
        cfg.pred[i] = term
    cfg.est_groups = est_groups
    cfg.num_entries = num_entries
    for i, w in enumerate(code_widths or ()):      # 0 = plain column, 1 / 2 / 4 = compressed attribute (codes)
        cfg.column_code_width[i] = w
    for i in nullable:
        cfg.column_nullable[i] = 1
    return cfg


def int_operand_type(cfg, operand, temp_types):
    """INT or LONG for an operand an integer instruction (EX_IADD .. EX_IDIV) accepts, else None: an INT / LONG column, a temp
    of an integer instruction, an integral constant with |c| <= 2^53 (INT when it fits 32 bits)."""
    if operand.kind == OPD_COLUMN:
        t = cfg.column_type[operand.index]
        return t if t in (INT, LONG) else None
    if operand.kind == OPD_CONST:
        v = cfg.consts[operand.index]
        if not (-2.0 ** 53 <= v <= 2.0 ** 53) or v != int(v):
            return None
        return INT if -2 ** 31 <= int(v) < 2 ** 31 else LONG
    return temp_types.get(operand.index)


def temp_types(cfg):
    """{temp: INT | LONG | None (a double)} after the whole program: a temp has the type of its latest definition."""
    types = {}
    for k in range(cfg.num_instrs):
        ins = cfg.instrs[k]
        if ins.op >= EX_IADD:
            ta, tb = int_operand_type(cfg, ins.a, types), int_operand_type(cfg, ins.b, types)
            types[ins.dst] = None if ta is None or tb is None else (INT if ta == INT and tb == INT else LONG)
        else:
            types[ins.dst] = None
    return types


def agg_argument_type(cfg, a):
    """Type of aggregate `a`'s argument: the column's, INT / LONG for an integer temp, DOUBLE for a double temp."""
    arg = cfg.aggs[a].arg
    if arg.kind == OPD_COLUMN:
        return cfg.column_type[arg.index]
    t = temp_types(cfg).get(arg.index)
    return DOUBLE if t is None else t


def agg_output_dtype(cfg, a):
    """numpy dtype name of the value column qsx_agg_finalize writes for aggregate `a`: int64 for COUNT
    and SUM over INT/LONG (a column or an integer expression), float64 for the other SUMs and AVG, the argument's own type
    for MIN/MAX."""
    fn = cfg.aggs[a].fn
    if fn in (AGG_MIN, AGG_MAX):
        return {INT: "int32", LONG: "int64", FLOAT: "float32", DOUBLE: "float64"}[agg_argument_type(cfg, a)]
    return "int64" if agg_output_is_int(cfg, a) else "float64"


def agg_output_is_int(cfg, a):
    """True when aggregate `a` finalizes to int64 (COUNT, SUM over INT/LONG: a column or an integer expression)."""
    fn = cfg.aggs[a].fn
    if fn in (AGG_COUNT_STAR, AGG_COUNT):
        return True
    if fn == AGG_AVG:
        return False
    return agg_argument_type(cfg, a) in (INT, LONG)


MAX_PROJECTED = 16                                                  # QSX_MAX_PROJECTED


class JoinProjection(C.Structure):                                   # qsx_join_projection_t
    _fields_ = [("num_columns", C.c_int32), ("width", C.c_int32 * MAX_PROJECTED), ("on_build", C.c_int32 * MAX_PROJECTED),
                ("probe_stripes", C.POINTER(C.c_void_p)), ("num_build_segments", C.c_int32),
                ("build_first_tids", C.POINTER(C.c_int64)), ("build_stripes", C.POINTER(C.c_void_p)),
                ("out_columns", C.POINTER(C.c_void_p))]


class SortKey(C.Structure):                                          # qsx_sort_key_t
    _fields_ = [("col_dev", C.c_void_p), ("null_bitmap_dev", C.c_void_p), ("type", C.c_int32), ("width", C.c_int32),
                ("descending", C.c_int32), ("nulls_first", C.c_int32)]
