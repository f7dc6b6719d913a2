"""GPU: every evaluator of a scalar expression program against tests/expr_reference.py, node by node and bit for bit.

  - qsx_eval_expression (eval_expression_kernel) over the double programs D1 - D5, qsx_eval_expression_long
    (eval_expression_long_kernel) over the integer programs I1 - I6 in both encodings of the ops: every definition step is read
    back through the program cut off behind it and every temp again after the whole program, so the first wrong label names the
    instruction;
  - the evaluators fused into the aggregation (the interpreter and the run-time plan shape of csrc/agg_hash_update.hpp, the
    collision-free kernels): one row per group, so MIN, MAX and SUM of a temp are that row's value;
  - the argument checks of both entry points.

The comparison rule: outputs are bit-equal; where the reference is NaN the device value must be a NaN and its bits are not
compared (expr_reference.same_bits).  Signed zeros, infinities and subnormals are compared by their bits.

Sizes follow the kernels.  eval_expression_kernel: 256 lanes with two rows each, the second a whole grid further on — 255 / 256 /
257 and 511 / 512 / 513 are the rows where no, some and all lanes have a second row; the grid stops growing at 2048 workgroups
of 512 rows, so 2048 * 512 + 257 rows make a second trip of the grid-stride loop with a ragged second row.
eval_expression_long_kernel: a workgroup of 256 lanes per 1024 rows, so 257 rows are a second trip of one workgroup, 1025 rows
two workgroups with a third trip."""
import ctypes as C

import numpy as np
import pytest
import torch

import case_reference as CR
import expr_reference as E
from quickstep_amd import types as T
from test_gpu_agg import finalize_np, run_hip

pytestmark = pytest.mark.gpu

DOUBLE_SIZES = (1, 2, 255, 256, 257, 511, 512, 513, 100_003)
SECOND_TRIP = 2048 * 512 + 257
LONG_SIZES = (1, 2, 255, 256, 257, 1023, 1024, 1025, 100_003)
TORCH_INT = {CR.INT: torch.int32, CR.LONG: torch.int64}
NP_INT = {CR.INT: np.int32, CR.LONG: np.int64}

_battery, _readbacks = {}, {}


def columns(n):
    """The battery of n rows: computed once per size and never modified."""
    if n not in _battery:
        _battery[n] = E.battery(np.random.default_rng([E.SEED, n]), n)
        for c in _battery[n].values():
            c.setflags(write=False)
    return _battery[n]


def readbacks(program, n):
    if (program.name, n) not in _readbacks:
        _readbacks[program.name, n] = E.readbacks(program, columns(n))
        for entry in _readbacks[program.name, n]:
            entry[3].setflags(write=False)
    return _readbacks[program.name, n]


def up(host, dev):
    """A device copy of a (read-only) host column."""
    return torch.from_numpy(np.array(host)).to(dev)


def describe(label, bad, got, want):
    return f"{label}: {bad.size} rows differ, first row {bad[0]}: got {got[bad[0]]!r}, reference {want[bad[0]]!r}"


def check_double(capi, program, n, dcols):
    consts = E.abi_consts(program)
    for label, count, o, want, _ in readbacks(program, n):
        got = capi.eval_expression(dcols, E.abi_instrs(program, count), consts, E.abi_operand(o)).cpu().numpy()
        bad = E.same_bits(got, want)
        assert bad.size == 0, describe(f"n = {n}, {label}", bad, got, want)


def check_long(capi, program, n, dcols):
    consts = E.abi_consts(program)
    for label, count, o, want, kind in readbacks(program, n):
        want = want.astype(NP_INT[kind])
        outs = []
        for integer_codes in (False, True):          # ops 0 .. 3, then EX_IADD .. EX_IDIV: synonyms here
            got = capi.eval_expression_long(dcols, E.abi_instrs(program, count, integer_codes), consts, E.abi_operand(o),
                                            out_dtype=TORCH_INT[kind]).cpu().numpy()
            bad = E.same_bits(got, want)
            assert bad.size == 0, describe(f"n = {n}, {label}, integer op codes {integer_codes}", bad, got, want)
            outs.append(got)
        assert outs[0].tobytes() == outs[1].tobytes()


@pytest.mark.parametrize("n", DOUBLE_SIZES)
@pytest.mark.parametrize("name", list(E.DOUBLE_PROGRAMS))
def test_double_projection_is_the_reference_bit_for_bit(capi, dev, name, n):
    program = E.DOUBLE_PROGRAMS[name]
    check_double(capi, program, n, [up(columns(n)[c], dev) for c in program.cols])


@pytest.mark.parametrize("name", ["D2", "D3"])
def test_double_projection_on_the_second_trip_of_the_grid(capi, dev, name):
    program = E.DOUBLE_PROGRAMS[name]
    check_double(capi, program, SECOND_TRIP, [up(columns(SECOND_TRIP)[c], dev) for c in program.cols])


@pytest.mark.parametrize("n", LONG_SIZES)
@pytest.mark.parametrize("name", list(E.LONG_PROGRAMS))
def test_integer_projection_is_the_reference_exactly(capi, dev, name, n):
    program = E.LONG_PROGRAMS[name]
    check_long(capi, program, n, [up(columns(n)[c], dev) for c in program.cols])


# ---- the entry points called directly: the caller's own output buffer ----------------------------------------------------------
def _arrays(dcols, instrs):
    count = max(len(dcols), 1)
    ptrs = (C.c_void_p * count)(*[None if c is None else c.data_ptr() for c in dcols])
    types = (C.c_int32 * count)(*[T.INT if c is None else capi_type(c) for c in dcols])
    prog = (T.ExprInstr * max(len(instrs), 1))(*[T.ExprInstr(op, dst, a, b) for op, dst, a, b in instrs])
    return ptrs, types, prog


def capi_type(c):
    return {torch.int32: T.INT, torch.int64: T.LONG, torch.float32: T.FLOAT, torch.float64: T.DOUBLE}[c.dtype]


def call_double(capi, dcols, instrs, consts, result, n, out, num_instrs=None, num_columns=None, types=None):
    ptrs, own_types, prog = _arrays(dcols, instrs)
    if types is not None:
        own_types = (C.c_int32 * len(types))(*types)
    cs = None if consts is None else (C.c_double * T.MAX_CONSTS)(*consts)
    return capi.lib.qsx_eval_expression(len(dcols) if num_columns is None else num_columns, ptrs, own_types,
                                        len(instrs) if num_instrs is None else num_instrs, prog, cs, result, n, out.data_ptr(), None)


def call_long(capi, dcols, instrs, consts, result, n, out, out_width=None, num_instrs=None, num_columns=None, types=None):
    ptrs, own_types, prog = _arrays(dcols, instrs)
    if types is not None:
        own_types = (C.c_int32 * len(types))(*types)
    cs = None if consts is None else (C.c_int64 * T.MAX_CONSTS)(*consts)
    return capi.lib.qsx_eval_expression_long(len(dcols) if num_columns is None else num_columns, ptrs, own_types,
                                             len(instrs) if num_instrs is None else num_instrs, prog, cs, result, n,
                                             out.element_size() if out_width is None else out_width, out.data_ptr(), None)


def off_alignment(host, dev, offset_bytes):
    """A device copy of `host` whose base lies offset_bytes behind a 16-byte boundary (an 8-byte stripe cannot sit 4 bytes off:
    it gets 8)."""
    shift = max(offset_bytes // host.itemsize, 1)
    buf = torch.zeros(host.size + 4, dtype=torch.from_numpy(host[:1].copy()).dtype, device=dev)
    view = buf[shift:shift + host.size]
    view.copy_(up(host, dev))
    assert view.data_ptr() % 16 == shift * host.itemsize % 16 != 0
    return view


SENTINEL = 0x5A


def guarded(n, dtype, dev, shift=0, behind=8):
    """(buffer of sentinel bytes, its n elements from `shift` on)."""
    buf = torch.full(((shift + n + behind) * torch.empty(0, dtype=dtype).element_size(),), SENTINEL, dtype=torch.uint8, device=dev).view(dtype)
    return buf, buf[shift:shift + n]


def assert_guards(buf, shift, n):
    raw = buf.cpu().numpy()
    assert np.all(raw[:shift].view(np.uint8) == SENTINEL) and np.all(raw[shift + n:].view(np.uint8) == SENTINEL), "bytes outside the n results were written"


@pytest.mark.parametrize("offset_bytes", [4, 8])
@pytest.mark.parametrize("name", ["D2", "D4"])
def test_double_projection_with_stripes_off_16_byte_alignment(capi, dev, name, offset_bytes):
    """Every column base 4 / 8 bytes past a 16-byte boundary and the output 8: no 16-byte load or store may be assumed.  D4 reads
    INT, LONG, FLOAT and DOUBLE stripes."""
    n = 1000
    program = E.DOUBLE_PROGRAMS[name]
    dcols = [off_alignment(columns(n)[c], dev, offset_bytes) for c in program.cols]
    for label, count, o, want, _ in readbacks(program, n):
        buf, out = guarded(n, torch.float64, dev, shift=1)
        assert out.data_ptr() % 16 == 8
        assert call_double(capi, dcols, E.abi_instrs(program, count), E.abi_consts(program), E.abi_operand(o), n, out) == T.OK
        got = out.cpu().numpy()
        bad = E.same_bits(got, want)
        assert bad.size == 0, describe(label, bad, got, want)
        assert_guards(buf, 1, n)


@pytest.mark.parametrize("offset_bytes", [4, 8])
@pytest.mark.parametrize("name", ["I2", "I5b"])
def test_integer_projection_with_stripes_off_16_byte_alignment(capi, dev, name, offset_bytes):
    n = 1000
    program = E.LONG_PROGRAMS[name]
    dcols = [off_alignment(columns(n)[c], dev, offset_bytes) for c in program.cols]
    for label, count, o, want, kind in readbacks(program, n):
        width = 4 if kind == CR.INT else 8
        shift = max(offset_bytes // width, 1)
        buf, out = guarded(n, TORCH_INT[kind], dev, shift=shift)
        assert out.data_ptr() % 16 == shift * width
        assert call_long(capi, dcols, E.abi_instrs(program, count), E.abi_consts(program), E.abi_operand(o), n, out) == T.OK
        got = out.cpu().numpy()
        bad = E.same_bits(got, want.astype(NP_INT[kind]))
        assert bad.size == 0, describe(label, bad, got, want)
        assert_guards(buf, shift, n)


@pytest.mark.parametrize("n", [1, 257, 1025])
def test_integer_projection_writes_n_values_of_out_width_bytes(capi, dev, n):
    """An INT result written with out_width 4 and a LONG one with 8 leave the bytes behind the n-th element alone."""
    program = E.I1                                                   # t0 = i + j: INT
    dcols = [up(columns(n)[c], dev) for c in program.cols]
    want = readbacks(program, n)[0][3]
    buf, out = guarded(n, torch.int32, dev, behind=11)
    assert call_long(capi, dcols, E.abi_instrs(program, 1), E.abi_consts(program), T.temp(0), n, out) == T.OK
    assert np.array_equal(out.cpu().numpy(), want.astype(np.int32))
    assert_guards(buf, 0, n)
    program = E.I2                                                   # t0 = l * 3: LONG
    dcols = [up(columns(n)[c], dev) for c in program.cols]
    want = readbacks(program, n)[0][3]
    buf, out = guarded(n, torch.int64, dev, behind=5)
    assert call_long(capi, dcols, E.abi_instrs(program, 1), E.abi_consts(program), T.temp(0), n, out) == T.OK
    assert np.array_equal(out.cpu().numpy(), want)
    assert_guards(buf, 0, n)
    buf, out = guarded(n, torch.float64, dev, behind=5)
    program = E.D2
    dcols = [up(columns(n)[c], dev) for c in program.cols]
    assert call_double(capi, dcols, E.abi_instrs(program, 1), E.abi_consts(program), T.temp(0), n, out) == T.OK
    assert E.same_bits(out.cpu().numpy(), readbacks(program, n)[0][3]).size == 0
    assert_guards(buf, 0, n)


# ---- the evaluators fused into the aggregation -----------------------------------------------------------------------------------
FUSED_PROGRAMS = {name: E.fused(p) for name, p in list(E.DOUBLE_PROGRAMS.items()) + list(E.LONG_PROGRAMS.items())
                  if name in ("D2", "D3", "I1", "I2", "I3")}
# two temps per configuration: MIN, MAX and SUM of each are six of the QSX_MAX_AGGS = 8 aggregates (an odd last temp comes with
# its predecessor again: every configuration has the same six accumulators and takes the same kernels)
FUSED_CONFIGS = [(name, tuple(temps[min(k, len(temps) - 2):][:2])) for name, p in FUSED_PROGRAMS.items()
                 for temps in [sorted({dst for _, dst, _, _ in p.instrs})] for k in range(0, len(temps), 2)]
INTERPRETER, RUN_TIME_SHAPE = str(1 << 60), "0"
FUSED_EVALUATORS = [pytest.param("generic", INTERPRETER, id="generic-interpreter"), pytest.param("generic", RUN_TIME_SHAPE, id="generic-run_time_shape"),
                    pytest.param("collision_free", INTERPRETER, id="collision_free-interpreter")]
FUSED_POOL = 8192
_fused = {}


def fused_rows(name, n):
    """(columns, {temp: (values, type)}) of the first n rows of the battery whose every node of the program is finite."""
    if (name, n) not in _fused:
        program = FUSED_PROGRAMS[name]
        pool = columns(FUSED_POOL)
        finite = np.ones(FUSED_POOL, dtype=bool)
        for step in E.evaluate(program, pool):
            for values, kind in step.values():
                if kind == CR.DOUBLE:
                    finite &= np.isfinite(values)
        rows = np.nonzero(finite)[0][:n]
        assert rows.size == n
        cols = {c: np.ascontiguousarray(pool[c][rows]) for c in program.cols}
        temps = E.evaluate(program, cols)[-1]
        for values, _ in temps.values():
            values.setflags(write=False)
        _fused[name, n] = (cols, temps)
    return _fused[name, n]


@pytest.mark.parametrize("n", [257, 4099])
@pytest.mark.parametrize("strategy,min_rows", FUSED_EVALUATORS)
@pytest.mark.parametrize("name,temps", FUSED_CONFIGS, ids=[name + "-" + "".join(f"t{t}" for t in temps) for name, temps in FUSED_CONFIGS])
def test_fused_evaluators_give_every_row_its_reference_value(capi, dev, monkeypatch, name, temps, strategy, min_rows, n):
    """One row per group (a permuted unique INT key): MIN(t), MAX(t) and SUM(t) of a group are the row's t.  Doubles compare with
    ==, which lets SUM turn a -0.0 into +0.0 and nothing else; integers exactly, in the output type of the temp."""
    monkeypatch.setenv("QSX_AGG_JIT_MIN_ROWS", min_rows)
    monkeypatch.delenv("QSX_AGG_NO_SPECIALIZE", raising=False)
    monkeypatch.delenv("QSX_AGG_JIT", raising=False)
    program = FUSED_PROGRAMS[name]
    cols, reference = fused_rows(name, n)
    key = np.random.default_rng([E.SEED, n, 1]).permutation(n).astype(np.int32)
    data = [key] + [cols[c] for c in program.cols]
    layout = [(T.INT, None)] + [({CR.INT: T.INT, CR.LONG: T.LONG, CR.FLOAT: T.FLOAT, CR.DOUBLE: T.DOUBLE}[CR.NP_TYPE[cols[c].dtype]], None)
                                for c in program.cols]
    aggs = [(fn, T.temp(t)) for t in temps for fn in (T.AGG_MIN, T.AGG_MAX, T.AGG_SUM)]
    kw = dict(keys=[0], instrs=E.abi_instrs(program, first=1), consts=program.consts, aggs=aggs)
    if strategy == "generic":
        cfg = T.make_agg_config(T.AGG_GENERIC, layout, est_groups=n, **kw)
    else:
        cfg = T.make_agg_config(T.AGG_COLLISION_FREE, layout, num_entries=n, **kw)
    st = run_hip(capi, dev, cfg, data)
    if min_rows == RUN_TIME_SHAPE:
        state_of = capi.lib.qsx_debug_agg_jit_state
        state_of.restype = C.c_int
        assert state_of(st._h, 0) == 1, "the run-time plan shape did not serve this update"
    keys, vals, nulls = finalize_np(st, dev)
    order = np.argsort(keys[0], kind="stable")
    assert np.array_equal(keys[0][order], np.arange(n)), "groups lost, doubled or invented"
    by_key = np.argsort(key)                                         # by_key[g]: the row of group g
    for a, (fn, _) in enumerate(aggs):
        t = temps[a // 3]
        values, kind = reference[t]
        want = values[by_key]
        got = vals[a][order]
        what = f"{name} {('MIN', 'MAX', 'SUM')[a % 3]}(t{t})"
        assert not nulls[a].any(), what
        if kind == CR.DOUBLE:
            assert got.dtype == np.float64, what
        else:
            assert got.dtype == (np.int64 if fn == T.AGG_SUM else NP_INT[kind]), what
            want = want.astype(got.dtype)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, f"{what}: {bad.size} groups differ, first group {bad[0]}: got {got[bad[0]]!r}, reference {want[bad[0]]!r}"


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_the_argument_checks_of_both_entry_points(capi, dev):
    """Every refused call leaves the output as it was: it is filled with a sentinel before each call."""
    n = 8
    bad, unsupported = T.ERR_INVALID_ARGUMENT, T.ERR_UNSUPPORTED
    host = columns(n)
    int_cols = [up(host[c], dev) for c in ("i", "l")]
    float_cols = [up(host[c], dev) for c in ("f", "d0")]
    consts = [1] * T.MAX_CONSTS

    def double(instrs, result, cols=int_cols + float_cols, consts=[1.0] * T.MAX_CONSTS, rows=n, **kw):
        buf, out = guarded(n, torch.float64, dev)
        rc = call_double(capi, cols, instrs, consts, result, rows, out, **kw)
        torch.cuda.synchronize()
        untouched = bool(np.all(buf.cpu().numpy().view(np.uint8) == SENTINEL))
        assert untouched or rc == T.OK, "a refused call wrote to the output"
        return rc, untouched

    def long(instrs, result, cols=int_cols, consts=consts, rows=n, width=8, **kw):
        buf, out = guarded(n, torch.int64, dev)
        rc = call_long(capi, cols, instrs, consts, result, rows, out, out_width=width, **kw)
        torch.cuda.synchronize()
        untouched = bool(np.all(buf.cpu().numpy().view(np.uint8) == SENTINEL))
        assert untouched or rc == T.OK, "a refused call wrote to the output"
        return rc, untouched

    def both(instrs, result, **kw):
        return double(instrs, result, **kw)[0], long(instrs, result, **kw)[0]

    add = lambda op=T.EX_ADD, dst=0, a=T.col(0), b=T.col(1): [(op, dst, a, b)]      # noqa: E731
    assert both(add(), T.temp(0)) == (T.OK, T.OK)
    assert double(add(), T.temp(0))[1] is False and long(add(), T.temp(0))[1] is False        # an accepted call does write
    # the op code
    for op in (-1, 8):
        assert both(add(op), T.temp(0)) == (bad, bad), op
    for op in (T.EX_IADD, T.EX_ISUB, T.EX_IMUL, T.EX_IDIV):
        assert both(add(op), T.temp(0)) == (bad, T.OK), op
    # the destination
    for dst in (-1, T.MAX_TEMPS):
        assert both(add(dst=dst), T.col(0)) == (bad, bad), dst
    assert both(add(dst=T.MAX_TEMPS - 1), T.temp(T.MAX_TEMPS - 1)) == (T.OK, T.OK)
    # a temp read before its definition: as an operand, as its own first operand, as the result
    assert both(add(a=T.temp(1)), T.temp(0)) == (bad, bad)
    assert both(add(b=T.temp(0)), T.temp(0)) == (bad, bad)
    assert both(add(), T.temp(1)) == (bad, bad)
    assert both([], T.temp(0)) == (bad, bad)
    assert both(add(a=T.temp(T.MAX_TEMPS)), T.temp(0)) == (bad, bad) and both(add(), T.temp(-1)) == (bad, bad)
    # column and constant indices
    assert double(add(b=T.col(4)), T.temp(0))[0] == bad and long(add(b=T.col(2)), T.temp(0))[0] == bad      # index = num_columns
    assert double(add(), T.col(4))[0] == bad and long(add(), T.col(2))[0] == bad
    assert both(add(b=T.col(-1)), T.temp(0)) == (bad, bad)
    assert both(add(b=T.const(T.MAX_CONSTS)), T.temp(0)) == (bad, bad) and both(add(b=T.const(-1)), T.temp(0)) == (bad, bad)
    assert both(add(), T.const(T.MAX_CONSTS)) == (bad, bad)
    assert both(add(b=T.const(T.MAX_CONSTS - 1)), T.temp(0)) == (T.OK, T.OK)
    # a constant operand without constants
    assert both(add(b=T.const(0)), T.temp(0), consts=None) == (bad, bad)
    assert both(add(), T.const(0), consts=None) == (bad, bad)
    assert both(add(), T.temp(0), consts=None) == (T.OK, T.OK)                                 # no constant is read
    # the operand kind
    for kind in (T.OPD_NULL, -1):
        assert both(add(b=T.Operand(kind, 0)), T.temp(0)) == (bad, bad), kind
        assert both(add(), T.Operand(kind, 0)) == (bad, bad), kind
    # the number of instructions
    full = add() + [(T.EX_ADD, k % T.MAX_TEMPS, T.temp(0), T.col(1)) for k in range(1, T.MAX_INSTRS)]
    assert len(full) == T.MAX_INSTRS and both(full, T.temp(0)) == (T.OK, T.OK)
    assert both(full + add(), T.temp(0)) == (bad, bad)
    assert both(add(), T.temp(0), num_instrs=-1) == (bad, bad)
    # the number of columns
    many = [int_cols[0]] * (T.MAX_COLUMNS + 1)
    assert both(add(), T.temp(0), cols=many[:T.MAX_COLUMNS]) == (T.OK, T.OK)
    assert both(add(), T.temp(0), cols=many) == (bad, bad)
    assert both(add(), T.temp(0), num_columns=-1) == (bad, bad)
    # the number of rows; a column without a stripe
    assert both(add(), T.temp(0), rows=-1) == (bad, bad)
    assert both(add(), T.temp(0), cols=[int_cols[0], None]) == (bad, bad)
    assert double(add(), T.temp(0), cols=[int_cols[0], None], rows=0) == (T.OK, True)
    assert long(add(), T.temp(0), cols=[int_cols[0], None], rows=0) == (T.OK, True)
    assert double(add(), T.temp(0), rows=0) == (T.OK, True) and long(add(), T.temp(0), rows=0) == (T.OK, True)
    # the column types
    for column_type in (T.CHAR, T.DATE):
        assert both(add(), T.temp(0), cols=int_cols, types=[T.INT, column_type]) == (unsupported, unsupported), column_type
        assert both(add(a=T.col(0), b=T.col(0)), T.temp(0), cols=int_cols, types=[T.INT, column_type]) == (unsupported, unsupported)
    assert double(add(a=T.col(2), b=T.col(3)), T.temp(0))[0] == T.OK
    assert long(add(), T.temp(0), cols=int_cols + float_cols[:1])[0] == unsupported            # a FLOAT column, not even read
    assert long(add(), T.temp(0), cols=int_cols + float_cols[1:])[0] == unsupported            # a DOUBLE column
    # the output width
    for width in (0, 2, 16, -4):
        assert long(add(), T.temp(0), width=width)[0] == bad, width
    assert long(add(), T.temp(0), width=4) == (T.OK, False)
    # the output itself
    ptrs, types, prog = _arrays(int_cols, add())
    assert capi.lib.qsx_eval_expression(2, ptrs, types, 1, prog, None, T.temp(0), n, None, None) == bad
    assert capi.lib.qsx_eval_expression_long(2, ptrs, types, 1, prog, None, T.temp(0), n, 8, None, None) == bad
    assert capi.lib.qsx_eval_expression(2, ptrs, types, 1, None, None, T.temp(0), n, None, None) == bad
    torch.cuda.synchronize()
