"""CPU checks of low-mode deflation (mugiq_hip_deflate_low_modes, mugiq_hip_loop_deflate): the entry points are declared and exported,
every validation error is returned before any device work (the descriptors point at nothing), and the C++ mirror compiles against
the C ABI."""
import ctypes
import os
import subprocess

import pytest

from util import ROOT

NEW = ["mugiq_hip_deflate_low_modes", "mugiq_hip_loop_deflate"]


def test_deflate_entry_points_are_declared_and_exported(hip):
    hdr = open(os.path.join(ROOT, "include", "mugiq_hip.h")).read()
    lib = hip._lib.load()
    for name in NEW:
        assert name + "(" in hdr
        assert hasattr(lib, name) and name in hip._lib.SIGNATURES
    assert hasattr(hip, "deflateLowModes") and hasattr(hip.Loop_Mugiq, "deflate")


def _desc(X=(4, 4, 4, 4), prec=8, order=2, data=1 << 20, pad=0, nParity=2):
    from mugiq_amd._lib import SpinorDesc
    d = SpinorDesc()
    d.data = ctypes.c_void_p(data)            # never dereferenced: validation fails before any device work
    d.precision, d.field_order, d.nParity = prec, order, nParity
    v = X[0] * X[1] * X[2] * X[3] // 2
    d.volumeCB, d.stride, d.parity_offset = v, v + pad, 12 * (v + pad)
    for i in range(4):
        d.X[i] = X[i]
    return d


SPAN = 2 * 12 * 128 * 16     # bytes of one 4^4 fp64 field


def _arr(descs):
    from mugiq_amd._lib import SpinorDesc
    return (SpinorDesc * len(descs))(*descs)


CASES = {
    # name: (dst kwargs list, src kwargs list, eigenvector kwargs list, sigma, nVec, nEv, expected message fragment)
    "null_dst": "NULL argument",
    "null_src": "NULL argument",
    "null_evecs": "NULL argument",
    "nvec0": "nVec = 0 must be >= 1",
    "nev0": "nEv = 0 must be >= 1",
    "nparity": "Full Site Subset",
    "precision": "precision = 2 (must be 4 or 8)",
    "order": "field_order = 3 (must be 2 or 4)",
    "null_data": "->data is NULL",
    "ev_mismatch": "eigenvector 1 differs",
    "src_mismatch": "src / dst vector 1 differs",
    "dst_prec": "src / dst vector 0 differs",
    "geometry": "differ in field order, geometry, stride or parity offset",
    "stride": "differ in field order, geometry, stride or parity offset",
    "order_sets": "differ in field order, geometry, stride or parity offset",
    "sigma_zero": "sigma[1] is zero",
    "partial_alias": "dst vector 0 overlaps src vector 0 without being identical",
    "cross_alias": "dst vector 1 overlaps src vector 0 without being identical",
}


def _case(name):
    base = 1 << 24
    ev = [_desc(data=base + i * SPAN) for i in range(2)]
    src = [_desc(data=base + (10 + i) * SPAN) for i in range(2)]
    dst = [_desc(data=base + (20 + i) * SPAN) for i in range(2)]
    sigma = [1.0, -2.0]
    nVec, nEv = 2, 2
    if name == "nparity":
        src[0] = _desc(data=src[0].data, nParity=1)
    elif name == "precision":
        ev[0].precision = 2
    elif name == "order":
        dst[1].field_order = 3
    elif name == "null_data":
        src[1].data = None
    elif name == "ev_mismatch":
        ev[1] = _desc(data=ev[1].data, prec=4)
    elif name == "src_mismatch":
        src[1] = _desc(data=src[1].data, prec=4)
    elif name == "dst_prec":
        dst[0] = _desc(data=dst[0].data, prec=4)
    elif name == "geometry":
        src = [_desc(X=(4, 4, 4, 8), data=s.data) for s in src]
        dst = [_desc(X=(4, 4, 4, 8), data=s.data) for s in dst]
    elif name == "stride":
        src = [_desc(pad=16, data=s.data) for s in src]
        dst = [_desc(pad=16, data=s.data) for s in dst]
    elif name == "order_sets":
        src = [_desc(order=4, data=s.data) for s in src]
        dst = [_desc(order=4, data=s.data) for s in dst]
    elif name == "sigma_zero":
        sigma = [1.0, 0.0]
    elif name == "partial_alias":
        dst[0].data = src[0].data + 4096
    elif name == "cross_alias":
        dst[1].data = src[0].data
    elif name == "nvec0":
        nVec = 0
    elif name == "nev0":
        nEv = 0
    return dst, src, ev, sigma, nVec, nEv


@pytest.mark.parametrize("name", sorted(CASES))
def test_deflate_validation_errors(hip, name):
    lib = hip._lib.load()
    dst, src, ev, sigma, nVec, nEv = _case(name)
    sg = (ctypes.c_double * 2)(*sigma)
    args = [None if name == "null_dst" else _arr(dst), None if name == "null_src" else _arr(src), nVec,
            None if name == "null_evecs" else _arr(ev), sg, nEv, 1, None, None, None]
    st = lib.mugiq_hip_deflate_low_modes(*args)
    msg = lib.mugiq_hip_last_error().decode()
    assert st == 1, (st, msg)                       # MUGIQ_HIP_ERROR_INVALID_ARGUMENT
    assert msg.startswith("deflateLowModes: ") and CASES[name] in msg, msg


def test_loop_deflate_rejects_null_loop(hip):
    lib = hip._lib.load()
    dst, src, ev, sigma, nVec, nEv = _case("none")
    st = lib.mugiq_hip_loop_deflate(None, _arr(dst), _arr(src), 2, 1, None)
    assert st == 1 and "Loop_Mugiq::deflate: loop is NULL" in lib.mugiq_hip_last_error().decode()


def test_python_deflate_checks_sizes(hip):
    with pytest.raises(hip.MugiqHipError):
        hip.deflateLowModes([], [], [object()])
    with pytest.raises(hip.MugiqHipError):
        hip.deflateLowModes([object()], [object(), object()], [object()])


def test_cpp_deflate_mirror_compiles(tmp_path):
    """deflateLowModes and Loop_Mugiq::deflate of include/mugiq_hip_operators.hpp, -fsyntax-only against the header."""
    tu = tmp_path / "deflate_tu.cpp"
    tu.write_text('#include "mugiq_hip_operators.hpp"\n'
                  "void use(mugiq_hip::MugiqLoopParam *lp, const std::vector<MugiqHipSpinorField> &ev, const std::vector<double> &s,\n"
                  "         const std::vector<MugiqHipSpinorField> &x, const std::vector<MugiqHipSpinorField> &xi, const MugiqHipComm *comm) {\n"
                  "  std::vector<std::complex<double>> c;\n"
                  "  mugiq_hip::deflateLowModes(x, xi, ev, s, true, &c, comm);\n"
                  "  mugiq_hip::deflateLowModes(x, x, ev);\n"
                  "  mugiq_hip::Loop_Mugiq<double, 2> loop(lp, ev, s, comm);\n"
                  "  loop.deflate(x, xi, true, &c);\n"
                  "  loop.deflate(x, x, false);\n"
                  "}\n")
    cc = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cc):
        pytest.skip("no clang++")
    r = subprocess.run([cc, "-std=c++17", "-fsyntax-only", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-Wall", "-I", os.path.join(ROOT, "include"),
                        "-I", "/opt/rocm/include", str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_deflate_random_sweep_reaches_its_regimes():
    """The cases of test_deflate_random_shapes (default seed count) reach what the sweep is there for, by the restated geometry of
    deflate_low_modes (deflate_workers.deflate_geometry): several 64-eigenvector blocks with a partial last one, several segments per
    pass-1 chunk with empty chunks behind the last one with work, every right-hand-side block width, several blocks in one call,
    FLOAT4 with a partial last segment, every storage combination, and dst aliasing src for some r only.  (A partial last chunk is
    not asked for: nSeg is a multiple of 12, so it needs segsPerChunk = 5 or more, i.e. fields far past the sweep's 32k sites.)"""
    import deflate_workers as w
    seen = set()
    for seed in range(w.DEFAULT_SEEDS):
        c = w.random_deflate_case(8000 + seed)
        g = w.deflate_geometry(c["X"], c["order"], c["nev"], c["nvec"])
        seen |= {k for k, v in g.items() if v is True}
        seen |= {("RB", rb) for rb in g["RBs"]} | {("storage", c["pe"], c["order"], c["ps"])}
        if len(g["RBs"]) > 1:
            seen.add("multi_block")
        if c["order"] == 4 and g["partial_last_segment"]:
            seen.add("float4_partial_segment")
        if 0 < len(c["alias"]) < c["nvec"]:
            seen.add("mixed_alias")
        if not c["overlaps"]:
            seen.add("stream_ordered")
    want = {"partial_last_block", "multi_segment", "empty_chunks", "multi_block", "float4_partial_segment", "mixed_alias",
            "stream_ordered"} | {("RB", rb) for rb in (4, 8, 12, 16)} | {("storage",) + s for s in w.STORAGE}
    assert want <= seen, sorted(map(str, want - seen))
