"""CPU checks of two-sided loops: the new entry points are declared and exported (test_cabi_cpu covers every declared symbol), the
host-side validation of mugiq_hip_loop_create_two_sided rejects inconsistent vector sets before any device work, the Python layer
refuses coarse sets, and the C++ overload of Loop_Mugiq compiles against the C ABI."""
import ctypes
import os
import subprocess

import pytest

from util import ROOT

NEW = ["mugiq_hip_displaced_loop_contraction_fused_two_sided", "mugiq_hip_loop_create_two_sided", "mugiq_hip_loop_get_entry_kernel"]


def test_new_entry_points_are_declared_and_exported(hip):
    hdr = open(os.path.join(ROOT, "include", "mugiq_hip.h")).read()
    lib = hip._lib.load()
    for name in NEW:
        assert name + "(" in hdr
        assert hasattr(lib, name) and name in hip._lib.SIGNATURES


def _desc(X=(4, 4, 4, 4), prec=8, order=2, data=16):
    from mugiq_amd._lib import SpinorDesc
    d = SpinorDesc()
    d.data = ctypes.c_void_p(data)            # never dereferenced: validation fails before any device work
    d.precision, d.field_order, d.nParity = prec, order, 2
    v = X[0] * X[1] * X[2] * X[3] // 2
    d.volumeCB, d.stride, d.parity_offset = v, v, 12 * v
    for i in range(4):
        d.X[i] = X[i]
    return d


@pytest.mark.parametrize("case", ["precision", "order", "geometry", "n0", "null_left"])
def test_loop_create_two_sided_rejects_inconsistent_sets(hip, case):
    from mugiq_amd.loop import _CLoopParam
    lib = hip._lib.load()
    n = 2
    R = (hip._lib.SpinorDesc * n)(*[_desc() for _ in range(n)])
    bad = {"precision": dict(prec=4), "order": dict(order=4), "geometry": dict(X=(4, 4, 4, 8))}.get(case, {})
    L = (hip._lib.SpinorDesc * n)(*[_desc(**bad) for _ in range(n)])
    sg = (ctypes.c_double * n)(1.0, 2.0)
    p = _CLoopParam()
    h = ctypes.c_void_p()
    st = lib.mugiq_hip_loop_create_two_sided(ctypes.byref(h), ctypes.byref(p), None if case == "null_left" else L, R, sg,
                                             0 if case == "n0" else n, None, None)
    assert st == 1 and not h.value          # MUGIQ_HIP_ERROR_INVALID_ARGUMENT, no loop object
    msg = lib.mugiq_hip_last_error().decode()
    want = {"precision": "left vector 0 differs in precision, order or geometry from the right vectors",
            "order": "left vector 0 differs in precision, order or geometry from the right vectors",
            "geometry": "left vector 0 differs in precision, order or geometry from the right vectors",
            "n0": "nEv = 0 must be >= 1", "null_left": "NULL argument"}[case]
    assert msg.startswith("Loop_Mugiq(two-sided): ") and want in msg, msg
    assert lib.mugiq_hip_loop_get_entry_kernel(None, 0) == -1


def test_python_two_sided_loop_refuses_coarse_sets(hip):
    coarse = [object(), object()]
    with pytest.raises(hip.MugiqHipError):
        hip.Loop_Mugiq(hip.MugiqLoopParam(), coarse, [1.0, 1.0], transfer=object(), eVecsLeft=coarse)
    with pytest.raises(hip.MugiqHipError):
        hip.Loop_Mugiq(hip.MugiqLoopParam(), coarse, [1.0, 1.0], eVecsLeft=coarse)   # not fine-level SpinorFields
    with pytest.raises(hip.MugiqHipError):
        hip.Loop_Mugiq(hip.MugiqLoopParam(), coarse, [1.0, 1.0], eVecsLeft=coarse[:1])


def test_cpp_two_sided_overload_compiles(tmp_path):
    """The Loop_Mugiq overload of include/mugiq_hip_operators.hpp, in the style of the stand-in syntax checks: -fsyntax-only."""
    tu = tmp_path / "two_sided_tu.cpp"
    tu.write_text('#include "mugiq_hip_operators.hpp"\n'
                  "void use(mugiq_hip::MugiqLoopParam *lp, const std::vector<MugiqHipSpinorField> &l,\n"
                  "         const std::vector<MugiqHipSpinorField> &r, const std::vector<double> &s) {\n"
                  "  mugiq_hip::Loop_Mugiq<double, 2> loop(lp, l, r, s);\n"
                  "  loop.computeCoarseLoop();\n"
                  "  (void)loop.entryKernel(0);\n"
                  "}\n")
    cc = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cc):
        pytest.skip("no clang++")
    r = subprocess.run([cc, "-std=c++17", "-fsyntax-only", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-Wall", "-I", os.path.join(ROOT, "include"),
                        "-I", "/opt/rocm/include", str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_two_sided_random_sweep_reaches_both_tiles_and_every_refusal():
    """The cases of test_two_sided_random_shapes (default seed count), through the restated decision of the driver
    (two_sided_workers.two_sided_entry_kernel): several column-tile entries, several of them along axes of extent 16 or 24, several
    row-tile entries, and step-by-step entries for every reason (length past 8, past the extent, no tile geometry, reduced storage on a
    row shape without a row tile); N_ev <= 4 and padded strides occur."""
    import collections
    import two_sided_workers as w
    n = collections.Counter()
    for seed in range(w.DEFAULT_SEEDS):
        c = w.random_two_sided_case(5000 + seed)
        for e, (kind, reason) in zip(c["entry"].split(";"), w.predicted_entry_kernels(c)):
            n[kind] += 1
            n[reason] += 1
            if kind == "MFMA_COLUMN" and c["X"]["xyzt".index(e[1])] >= 16:
                n["column_16_24"] += 1
        n["nev<=4"] += c["nev"] <= 4
        n["padded"] += c["pad"] > 0
    assert n["MFMA_COLUMN"] >= 12 and n["column_16_24"] >= 8 and n["MFMA_ROW"] >= 6, n
    for reason in ("kmax>8", "kmax>extent", "no geometry", "reduced row", "nev<=4", "padded"):
        assert n[reason] >= 1, (reason, n)


def test_two_sided_decision_restatement_matches_known_cases():
    """Spot checks of the restated decision against the kernels the fixed-shape GPU tests assert"""
    import two_sided_workers as w
    k = lambda X, p, o, d, a, b: w.two_sided_entry_kernel(X, p, o, d, a, b)[0]
    assert k((24, 8, 8, 8), 8, 2, 0, 1, 3) == "MFMA_ROW" and k((24, 8, 8, 8), 4, 4, 0, 1, 3) == "STEPWISE"
    assert k((8, 8, 8, 16), 8, 2, 2, 1, 8) == "MFMA_COLUMN" and k((8, 8, 8, 16), 8, 2, 1, 1, 9) == "STEPWISE"
    assert k((4, 4, 2, 4), 8, 2, 3, 1, 2) == "MFMA_COLUMN" and k((4, 4, 2, 2), 8, 2, 2, 1, 1) == "STEPWISE"
