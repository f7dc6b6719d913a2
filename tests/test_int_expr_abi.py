"""CPU: the integer expression instructions (QSX_EX_IADD .. IDIV, include/qsx.h) through the host-only hooks of the library — how
translate() types and refuses programs, that every flavour of a run-time plan shape compiles for gfx950 with them, that the
shape's text tells IADD from ADD, and that a plan with an integer node does not factor through dictionary codes.  No GPU: hipcc /
hipRTC cross-compile, nothing is launched."""
import ctypes as C
import os

import pytest

import int_expr_reference as X
from quickstep_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = [(T.INT, None)]
TYPE_OF_DTYPE = {"int32": T.INT, "int64": T.LONG, "float32": T.FLOAT, "float64": T.DOUBLE}


def _translate(capi, cfg):
    fn = capi.lib.qsx_debug_agg_translate
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(T.AggConfig), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int]
    types, is_int = (C.c_int32 * T.MAX_AGGS)(), (C.c_int32 * T.MAX_AGGS)()
    rc = fn(C.byref(cfg), types, is_int, T.MAX_AGGS)
    return rc, list(types)[:cfg.num_aggs], list(is_int)[:cfg.num_aggs]


def _compile(capi):
    fn = capi.lib.qsx_debug_jit_compile
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(T.AggConfig), C.c_int, C.POINTER(C.c_size_t)]
    return fn


def test_abi_version_and_struct_did_not_move(capi):
    header = open(os.path.join(ROOT, "include", "qsx.h")).read()
    assert capi.lib.qsx_abi_version() == T.ABI_VERSION == 19 and "#define QSX_ABI_VERSION 19" in header
    assert capi.lib.qsx_abi_sizeof_agg_config() == C.sizeof(T.AggConfig)
    assert (T.EX_IADD, T.EX_ISUB, T.EX_IMUL, T.EX_IDIV) == (4, 5, 6, 7)
    assert "QSX_EX_IADD = 4, QSX_EX_ISUB = 5, QSX_EX_IMUL = 6, QSX_EX_IDIV = 7" in header
    assert "qsx_debug_agg_translate" not in header and "qsx_debug_agg_translate" not in capi.EXPORTED


# (the hook's flavour bits: 1 filter, 2 group directory, 4 run of blocks, 8 dense state in LDS, 16 register groups)
FLAVOURS = [(T.AGG_COMPACT_KEY, {}, bits) for bits in (0, 1, 2, 4, 16)] + [(T.AGG_GENERIC, {}, 0)] + \
           [(T.AGG_COLLISION_FREE, {"num_entries": 5000}, bits) for bits in (0, 4, 8)]


@pytest.mark.parametrize("plan", ["E1", "E2"])
def test_plan_shapes_with_integer_instructions_compile(capi, plan):
    fn = _compile(capi)
    for strategy, extra, bits in FLAVOURS:
        cfg = X.make_config(plan, KEY, strategy, **extra)
        size = C.c_size_t(0)
        assert fn(C.byref(cfg), bits, C.byref(size)) == 0, (strategy, bits)
        assert size.value > 1000
    # nullable j and k (E2: all eight accumulators in use)
    cfg = X.make_config(plan, KEY, T.AGG_GENERIC, nullable=("j", "k"))
    size = C.c_size_t(0)
    assert fn(C.byref(cfg), 0, C.byref(size)) == 0 and size.value > 1000


def test_shape_text_tells_integer_ops_from_double_ops(capi, tmp_path, monkeypatch):
    """The shape's text is its cache key (agg_jit.hip): i + j with IADD and with ADD are two shapes."""
    fn = _compile(capi)
    layout = KEY + [(T.INT, None), (T.INT, None)]
    texts = {}
    for name, op in (("iadd", T.EX_IADD), ("add", T.EX_ADD)):
        cfg = T.make_agg_config(T.AGG_GENERIC, layout, keys=[0], instrs=[(op, 0, T.col(1), T.col(2))],
                                aggs=[(T.AGG_SUM, T.temp(0)), (T.AGG_COUNT_STAR, None)])
        dump = tmp_path / f"{name}.hip"
        monkeypatch.setenv("QSX_JIT_DUMP", str(dump))
        size = C.c_size_t(0)
        assert fn(C.byref(cfg), 0, C.byref(size)) == 0 and size.value > 1000
        text = dump.read_text()
        texts[name] = text[text.index("jit_make_dev"):]
    assert texts["iadd"] != texts["add"]


def test_the_compiled_integer_form_holds_no_fp64_arithmetic(capi, tmp_path, monkeypatch):
    """E1 is purely integer (AVG divides in finalize): its compiled update kernel keeps nothing in scratch and converts nothing
    to double."""
    import shutil
    import subprocess
    objdump, bundler = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/clang-offload-bundler"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not all(os.path.exists(p) for p in (objdump, bundler, readelf)):
        pytest.skip("no llvm-objdump / clang-offload-bundler in this image")
    fn = _compile(capi)
    cfg = X.make_config("E1", KEY, T.AGG_GENERIC, est=64)
    code = tmp_path / "e1.co"
    monkeypatch.setenv("QSX_JIT_DUMP_CODE", str(code))
    size = C.c_size_t(0)
    assert fn(C.byref(cfg), 0, C.byref(size)) == 0 and size.value > 1000
    elf = tmp_path / "e1.elf"
    r = subprocess.run([bundler, "--unbundle", "--type=o", f"--input={code}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--output={elf}"], capture_output=True)
    if r.returncode != 0:           # (hipRTC hands out the bare code object)
        shutil.copy(code, elf)
    notes = subprocess.run([readelf, "--notes", str(elf)], capture_output=True, text=True).stdout
    assert ".private_segment_fixed_size: 0" in notes
    asm = subprocess.run([objdump, "-d", str(elf)], capture_output=True, text=True).stdout
    assert "s_endpgm" in asm
    for mnemonic in ("v_cvt_f64_i32", "v_cvt_f64_u32", "v_add_f64", "v_mul_f64", "v_fma_f64"):
        assert mnemonic not in asm, mnemonic


def test_a_plan_with_an_integer_node_does_not_factor(capi):
    fn = capi.lib.qsx_debug_agg_factored_plan
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(T.AggConfig), C.POINTER(C.c_int32), C.c_int]

    def factors(cfg):
        out = (C.c_int32 * 16)()
        assert fn(C.byref(cfg), out, 16) == 0
        return out[0]
    # key, l LONG (plain), k INT (1-byte dictionary codes): SUM(l * k) is affine in l once k is fixed
    layout = [(T.INT, None), (T.LONG, None), (T.INT, None)]
    for op, want in ((T.EX_MUL, 1), (T.EX_IMUL, 0)):
        cfg = T.make_agg_config(T.AGG_COMPACT_KEY, layout, keys=[0], code_widths=[0, 0, 1], instrs=[(op, 0, T.col(1), T.col(2))],
                                aggs=[(T.AGG_SUM, T.temp(0)), (T.AGG_COUNT_STAR, None)], est_groups=6)
        assert factors(cfg) == want, (op, want)


# ---- translate(): what it refuses and how it types ---------------------------------------------------------------------------------
LAYOUT = [(T.INT, None), (T.INT, None), (T.LONG, None), (T.DOUBLE, None), (T.FLOAT, None), (T.CHAR, 4), (T.DATE, None)]
I_, L_, D_, F_, CH_, DT_ = (T.col(c) for c in range(1, 7))


def _cfg(instrs, aggs, consts=()):
    return T.make_agg_config(T.AGG_GENERIC, LAYOUT, keys=[0], instrs=instrs, consts=consts, aggs=aggs)


REFUSED = {
    "double_column": _cfg([(T.EX_IADD, 0, I_, D_)], [(T.AGG_SUM, T.temp(0))]),
    "float_column": _cfg([(T.EX_IMUL, 0, F_, I_)], [(T.AGG_SUM, T.temp(0))]),
    "char_column": _cfg([(T.EX_IADD, 0, I_, CH_)], [(T.AGG_SUM, T.temp(0))]),
    "date_column": _cfg([(T.EX_ISUB, 0, DT_, I_)], [(T.AGG_SUM, T.temp(0))]),
    "double_temp": _cfg([(T.EX_ADD, 0, I_, I_), (T.EX_IADD, 1, T.temp(0), I_)], [(T.AGG_SUM, T.temp(1))]),
    "redefined_as_double": _cfg([(T.EX_IADD, 0, I_, I_), (T.EX_MUL, 0, T.temp(0), D_), (T.EX_IADD, 1, T.temp(0), I_)], [(T.AGG_SUM, T.temp(1))]),
    "constant_half": _cfg([(T.EX_IMUL, 0, I_, T.const(0))], [(T.AGG_SUM, T.temp(0))], consts=[0.5]),
    "constant_beyond_2_53": _cfg([(T.EX_IADD, 0, L_, T.const(0))], [(T.AGG_SUM, T.temp(0))], consts=[2.0**53 + 2]),
    "constant_nan": _cfg([(T.EX_IADD, 0, L_, T.const(0))], [(T.AGG_SUM, T.temp(0))], consts=[float("nan")]),
    "op_8": _cfg([(8, 0, I_, I_)], [(T.AGG_SUM, T.temp(0))]),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_translate_refuses(capi, name):
    assert _translate(capi, REFUSED[name])[0] == T.ERR_INVALID_ARGUMENT


FIVE_E9 = 5_000_000_000.0
ACCEPTED = {
    # name: (config, [(type of the value column, accumulator is int64)] per aggregate)
    "int_int": (_cfg([(T.EX_IADD, 0, I_, I_)], [(T.AGG_SUM, T.temp(0)), (T.AGG_MIN, T.temp(0)), (T.AGG_AVG, T.temp(0))]),
                [(T.INT, 1), (T.INT, 1), (T.INT, 1)]),
    "int_long": (_cfg([(T.EX_ISUB, 0, I_, L_)], [(T.AGG_MAX, T.temp(0)), (T.AGG_SUM, T.temp(0))]), [(T.LONG, 1), (T.LONG, 1)]),
    "int_small_constant": (_cfg([(T.EX_IDIV, 0, I_, T.const(0))], [(T.AGG_MIN, T.temp(0))], consts=[-7.0]), [(T.INT, 1)]),
    "int_wide_constant": (_cfg([(T.EX_IMUL, 0, I_, T.const(0))], [(T.AGG_MIN, T.temp(0))], consts=[FIVE_E9]), [(T.LONG, 1)]),
    "constant_2_53": (_cfg([(T.EX_IADD, 0, I_, T.const(0))], [(T.AGG_MAX, T.temp(0))], consts=[-2.0**53]), [(T.LONG, 1)]),
    "int_temp_chain": (_cfg([(T.EX_IADD, 0, I_, I_), (T.EX_IMUL, 1, T.temp(0), T.temp(0)), (T.EX_IADD, 2, T.temp(1), L_)],
                            [(T.AGG_MIN, T.temp(1)), (T.AGG_MIN, T.temp(2))]), [(T.INT, 1), (T.LONG, 1)]),
    "double_over_int_temp": (_cfg([(T.EX_IADD, 0, I_, I_), (T.EX_MUL, 1, T.temp(0), T.const(0))],
                                  [(T.AGG_SUM, T.temp(1)), (T.AGG_MAX, T.temp(1)), (T.AGG_SUM, T.temp(0))], consts=[0.5]),
                             [(T.DOUBLE, 0), (T.DOUBLE, 0), (T.INT, 1)]),
    "latest_definition": (_cfg([(T.EX_IADD, 0, I_, I_), (T.EX_IADD, 0, T.temp(0), L_)], [(T.AGG_MIN, T.temp(0))]), [(T.LONG, 1)]),
    "redefined_as_integer": (_cfg([(T.EX_ADD, 0, D_, D_), (T.EX_IADD, 0, I_, I_)], [(T.AGG_MAX, T.temp(0))]), [(T.INT, 1)]),
    "plain_ops_stay_double": (_cfg([(T.EX_ADD, 0, I_, L_)], [(T.AGG_SUM, T.temp(0)), (T.AGG_MIN, T.temp(0))]), [(T.DOUBLE, 0), (T.DOUBLE, 0)]),
    "columns": (_cfg([], [(T.AGG_SUM, I_), (T.AGG_MIN, L_), (T.AGG_MAX, F_), (T.AGG_SUM, D_)]),
                [(T.INT, 1), (T.LONG, 1), (T.FLOAT, 0), (T.DOUBLE, 0)]),
}
for _plan in ("E1", "E2", "PLAIN"):
    ACCEPTED[_plan] = (X.make_config(_plan, KEY, T.AGG_GENERIC), None)


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_translate_types_and_the_binding_agrees(capi, name):
    cfg, want = ACCEPTED[name]
    rc, types, is_int = _translate(capi, cfg)
    assert rc == T.OK
    for a in range(cfg.num_aggs):
        fn = cfg.aggs[a].fn
        if fn in (T.AGG_COUNT_STAR, T.AGG_COUNT):
            assert T.agg_output_dtype(cfg, a) == "int64"
            continue
        if want is not None:
            assert (types[a], is_int[a]) == want[a], (name, a)
        dtype = T.agg_output_dtype(cfg, a)
        if fn in (T.AGG_MIN, T.AGG_MAX):
            assert TYPE_OF_DTYPE[dtype] == types[a], (name, a)
        elif fn == T.AGG_SUM:
            assert dtype == ("int64" if is_int[a] else "float64") and T.agg_output_is_int(cfg, a) == bool(is_int[a]), (name, a)
        else:
            assert dtype == "float64" and not T.agg_output_is_int(cfg, a)
    if name in X.EXPECTED_DTYPES:
        assert [T.agg_output_dtype(cfg, a) for a in range(cfg.num_aggs)] == X.EXPECTED_DTYPES[name]
