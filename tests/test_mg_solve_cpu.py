"""CPU checks of the two-grid preconditioned GCR (mugiq_hip_mg_solve, mugiq_hip_mg_precondition): the numpy restatement of
tests/mg_solve_ref.py against the dense solve on both 4^4 fields of tests/mg_solve_cases.py, the homogeneity of K, the coarse-space condition
(null vectors from the low modes beat random ones), the margin of every reference history to its tolerance, every validation error before
any device work (the descriptors point at nothing), the defaults, and the C++ mirror against the C ABI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import coarse_op_cases as coc
import mg_solve_cases as cases
import mg_solve_ref as mgr
import wilson_ref as wr
from util import ROOT, rel_err

NEW = ["mugiq_hip_mg_solve_param_default", "mugiq_hip_mg_precondition", "mugiq_hip_mg_solve"]


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", ["hot", "smooth"])
def test_dense_matrix_is_the_stencil(field):
    """The dense M of the cases, filled block by block, against wilson_ref.wilson_M on a random vector; the smooth field is nearly singular."""
    v = cases.rhs(field)[1]
    want = wr.wilson_M(v, cases.links(field)[1], cases.KAPPA[field], cases.X4)
    assert rel_err((cases.dense_M(field) @ v.reshape(-1)).reshape(v.shape), want) < 1e-14
    low = np.abs(cases.low_modes(field)[0][0])
    assert (0.01 < low < 0.02) if field == "smooth" else low > 0.2, low


@pytest.mark.parametrize("field,nKrylov,nuPost", cases.SOLVES)
def test_restatement_matches_the_dense_solve(field, nKrylov, nuPost):
    """mg_solve_ref converges on both fields, with and without restarts, at the default tolerance, where its recursive residual is the
    true one; and its x matches numpy.linalg.solve to 1e-9 in the max norm (util.rel_err, the measure of the CG tests) at the tolerance
    of mg_solve_cases.solve_tolerance, whose a-priori bound guarantees 5e-10 (measured 6e-12 .. 1e-11)."""
    want = cases.dense_solution(field, 0)
    xt, itt, tight = cases.tight_solve(field, nKrylov, nuPost)
    smin = np.abs(cases.low_modes(field)[0][0])
    assert tight * np.linalg.norm(cases.rhs(field)[0]) / (smin * np.max(np.abs(want))) <= 0.5 * cases.X_BOUND
    e = rel_err(xt, want)
    print("x against the dense solve: %.3e at tol %.3e, %d iterations" % (e, tight, itt))
    assert e < cases.X_BOUND, e
    x, it, hist, tol = cases.reference_solve(field, nKrylov, nuPost)
    assert 0 < it <= itt < 200 and len(hist) == it and hist[-1] <= tol < (hist[-2] if it > 1 else 1.0)
    b = cases.rhs(field)[0]
    true = np.linalg.norm(b - cases.problem(field).M(x)) / np.linalg.norm(b)
    assert abs(true - hist[-1]) < 1e-3 * true, (true, hist[-1])          # the recursive residual is the true one


def test_restatement_trivial_right_hand_side():
    P = cases.problem("hot")
    x, it, hist, ok = mgr.solve(P, np.zeros_like(cases.rhs("hot")[0]))
    assert ok and it == 0 and len(hist) == 0 and not np.any(x)


@pytest.mark.parametrize("param", [dict(nuPre=0, nuPost=2, coarseIters=4), dict(nuPre=1, nuPost=1, coarseIters=8),
                                   dict(nuPre=0, nuPost=0, coarseIters=4), dict(nuPre=2, nuPost=0, coarseIters=0)])
def test_K_is_homogeneous(param):
    """K(c r) = c K(r) for real c > 0, to 1e-13; and K moves by less than 1e-14 under 1-ulp perturbations of r (measured 6e-16),
    three orders below the 1e-12 the device is held to."""
    P, r = cases.problem("smooth"), cases.rhs("smooth")[0]
    z = mgr.K(P, r, **param)
    for c in (3.7, 1e-6):
        assert rel_err(mgr.K(P, c * r, **param), c * z) < 1e-13
    assert max(rel_err(mgr.K(P, mgr.ulp_perturbed(r, s), **param), z) for s in (1, 2, 3)) < 1e-14
    assert not np.any(mgr.K(P, np.zeros_like(r), **param))               # the guards: no 0 / 0


@pytest.mark.parametrize("shape", [cases.RAGGED, coc.SHAPES[0]], ids=["ragged", "4x4x4x4"])
@pytest.mark.parametrize("clover", [False, True])
def test_chain_variant_has_the_K_of_the_explicit_matrices(shape, clover):
    """mg_solve_ref.ChainProblem (A_c = R M P applied as a chain, what the GPU tests compare with where the matrices take too long to
    build) against mg_solve_ref.Problem on the explicit matrices: K of every parameter set the GPU tests use, to 1e-13 of the max norm
    (measured 9e-16: the two coarse operators differ by rounding, and K moves by less than 1e-14 under 1-ulp perturbations); and K(0) = 0
    exactly in both -- d > 0.0 fails in the MR step, nu == 0.0 in the GCR step."""
    pe, pc = cases.shape_problem(*shape, clover=clover), cases.shape_problem(*shape, clover=clover, chain=True)
    assert pc.Mc is None and pe.Xc == pc.Xc
    r = cases.shape_rhs(shape[0])[0]
    for prm in cases.K_PARAMS + cases.EDGE_PARAMS:
        z = mgr.K(pe, r, **prm)
        e = rel_err(mgr.K(pc, r, **prm), z)
        assert np.all(np.isfinite(z)) and e < 1e-13, (prm, e)
        assert max(rel_err(mgr.K(pc, mgr.ulp_perturbed(r, s), **prm), z) for s in (1, 2, 3)) < 1e-14
        for p in (pe, pc):
            z0 = mgr.K(p, np.zeros_like(r), **prm)
            assert np.all(z0 == 0.0), prm                                  # (a NaN is != 0.0)


def test_new_shapes_launch_as_the_scale_tests_say():
    """The arithmetic the shapes of tests/test_gpu_mg_solve_scale.py were chosen by, against the constants of csrc/mg_solve.hip."""
    src = open(os.path.join(ROOT, "mugiq_amd", "csrc", "mg_solve.hip")).read()
    assert "constexpr int kMgThreads = 256;" in src and "constexpr int kMgMaxGroups = 256;" in src and "constexpr int kMgSlots = 32;" in src
    total = lambda X: 24 * int(np.prod(X)) // 2                          # noqa: E731  complex elements of a fine vector
    assert total(cases.LARGE[0]) == 98304 and 256 * 256 < total(cases.LARGE[0]) < 2 * 256 * 256      # a second trip for some workgroups only
    assert total((8, 8, 8, 8)) < 256 * 256                                # the largest field of test_gpu_mg_solve.py: one trip
    vcb = int(np.prod(cases.RAGGED[0])) // 2
    assert vcb == 432 and total(cases.RAGGED[0]) % 256 == 128 and vcb % 64 != 0 and (2 * vcb) % 64 != 0
    X, bs, nvec = coc.SHAPES[5]
    assert 2 * 2 * nvec * (int(np.prod(X)) // int(np.prod(bs)) // 2) == 1536 and 2 * 15 <= 32


def test_wide_index_switch_is_read_and_documented(hip):
    """MUGIQ_HIP_DEBUG_WIDE_INDEX: the built library holds the name (it calls getenv with it), narrow() of csrc/mg_solve.hip depends on it,
    and internal.h, DESIGN.md and README.md name it."""
    name = "MUGIQ_HIP_DEBUG_WIDE_INDEX"
    hip._lib.load()
    assert name.encode() in open(hip._lib.LIB_PATH, "rb").read()
    src = open(os.path.join(ROOT, "mugiq_amd", "csrc", "mg_solve.hip")).read()
    assert "debug_wide_index_asked()" in src and "return !wide && L.total < (int64_t(1) << 31);" in src
    for doc in (os.path.join("mugiq_amd", "csrc", "internal.h"), "DESIGN.md", "README.md"):
        assert name in open(os.path.join(ROOT, doc)).read(), doc


def test_coarse_space_condition():
    """Smooth field, same parameters: null vectors from the low modes need at most 0.7 x the outer iterations of random ones."""
    b = cases.rhs("smooth")[0]
    counts = {kind: mgr.solve(cases.problem("smooth", kind), b)[1] for kind in ("low", "random")}
    print("outer iterations %s, recorded %s" % (counts, cases.SMOOTH_COUNTS))
    assert counts["low"] <= 0.7 * counts["random"], counts
    assert cases.SMOOTH_COUNTS["low"] <= 0.7 * cases.SMOOTH_COUNTS["random"]


@pytest.mark.parametrize("field,nKrylov,nuPost", cases.SOLVES)
def test_history_margin(field, nKrylov, nuPost):
    """No entry of a history the device is compared with lies within 1 % of its tolerance."""
    for i in (0, 1):
        _, it, hist, tol = cases.reference_solve(field, nKrylov, nuPost, i)
        assert np.all(np.abs(hist / tol - 1.0) >= 0.01) and 0.5 * cases.TOL < tol <= cases.TOL


# ---- the C ABI without a device -----------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_exported(hip):
    hdr = open(os.path.join(ROOT, "include", "mugiq_hip.h")).read()
    lib = hip._lib.load()
    for name in NEW:
        assert name + "(" in hdr
        assert hasattr(lib, name) and name in hip._lib.SIGNATURES
    assert "MugiqHipMgSolveParam" in hdr and "NOT tuned" in hdr
    for name in ("mgSolve", "mgPrecondition", "MgSolveInfo", "mgSolveParam"):
        assert hasattr(hip, name)
    assert hasattr(hip.Eigsolve_Mugiq, "solveMG") and hasattr(hip.Loop_Mugiq, "solveMG")


def test_defaults(hip):
    p = hip._lib.MgSolveParam()
    assert hip._lib.load().mugiq_hip_mg_solve_param_default(ctypes.byref(p)) == 0
    assert (p.tol, p.maxIter, p.nKrylov, p.nuPre, p.nuPost, p.omega, p.coarseIters) == (1e-10, 1000, 16, 0, 4, 1.0, 8)
    assert hip._lib.load().mugiq_hip_mg_solve_param_default(None) == 1
    q = hip.mgSolveParam(nuPost=2, tol=1e-8)
    assert (q.nuPost, q.tol, q.nKrylov) == (2, 1e-8, 16)
    with pytest.raises(hip.MugiqHipError):
        hip.mgSolveParam(nuPst=2)
    assert mgr.DEFAULTS == dict(tol=p.tol, maxIter=p.maxIter, nKrylov=p.nKrylov, nuPre=p.nuPre, nuPost=p.nuPost, omega=p.omega,
                                coarseIters=p.coarseIters)


X8 = (8, 8, 8, 8)


def _spinor(data, X=X8, prec=8, order=2, pad=0):
    from mugiq_amd._lib import SpinorDesc
    d = SpinorDesc()
    v = int(np.prod(X)) // 2
    d.data, d.precision, d.field_order, d.nParity, d.volumeCB, d.stride, d.parity_offset = ctypes.c_void_p(data), prec, order, 2, v, v + pad, 12 * (v + pad)
    for i in range(4):
        d.X[i] = X[i]
    return d


def _op(X=(2, 2, 2, 2), nvec=4, prec=8, data=1 << 33):
    from mugiq_amd._lib import CoarseOperatorDesc
    d = CoarseOperatorDesc()
    d.data = ctypes.c_void_p(data)
    d.precision, d.nVec, d.volumeCB, d.kappa, d.hasClover = prec, nvec, int(np.prod(X)) // 2, 0.1, 0
    for i in range(4):
        d.X[i] = X[i]
    return d


def _transfer(X=X8, bs=(4, 4, 4, 4), nvec=4, prec=8, data=1 << 32):
    from mugiq_amd._lib import TransferDesc
    t = TransferDesc()
    t.V = ctypes.c_void_p(data)
    t.precision, t.nVec, t.spinBlockSize = prec, nvec, 2
    v = int(np.prod(X)) // 2
    t.stride, t.parity_offset = v, 12 * nvec * v
    for i in range(4):
        t.X[i], t.geoBlockSize[i] = X[i], bs[i]
    return t


def _gauge(X=X8, prec=8):
    from mugiq_amd._lib import GaugeDesc
    g = GaugeDesc()
    g.data, g.precision = ctypes.c_void_p(1 << 36), prec
    v = int(np.prod(X)) // 2
    g.stride, g.parity_offset = v, 36 * v
    for i in range(4):
        g.X[i], g.R[i] = X[i], 0
    return g


def _comm(size=1, grid=(1, 1, 1, 1), partitioned=(0, 0, 0, 0)):
    from mugiq_amd.comm import _CCommRaw
    c = _CCommRaw()
    c.rank, c.size = 0, size
    for i in range(4):
        c.grid[i], c.coord[i], c.partitioned[i] = grid[i], 0, partitioned[i]
    return c


def _arr(descs):
    return (type(descs[0]) * len(descs))(*descs)


def _param(hip, **kw):
    p = hip._lib.MgSolveParam()
    hip._lib.load().mugiq_hip_mg_solve_param_default(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


SPAN = 2 * 12 * 2048 * 16          # bytes of an 8^4 fp64 field


def _fields(base, n=2, **kw):
    return _arr([_spinor(base + i * SPAN, **kw) for i in range(n)])


@pytest.mark.parametrize("entry", ["solve", "precondition"])
def test_validation_errors(hip, entry):
    """Every refusal comes before any device work: the descriptors point at nothing, and no GPU is there."""
    lib = hip._lib.load()
    who = "mgSolve: " if entry == "solve" else "mgPrecondition: "
    out0, in0 = _fields(1 << 40), _fields(1 << 41)
    iters, relres = (ctypes.c_int * 2)(), (ctypes.c_double * 2)()

    def run(out=out0, inp=in0, n=2, g=_gauge(), c=None, t=_transfer(), op=_op(), p=_param(hip), comm=None, it=iters, rel=relres, hist=None, hs=0):
        ref = lambda x: ctypes.byref(x) if x is not None else None                                    # noqa: E731
        cm = ctypes.cast(ctypes.byref(comm), ctypes.c_void_p) if comm is not None else None
        if entry == "solve":
            return lib.mugiq_hip_mg_solve(out, inp, n, ref(g), ref(c), 0.1, ref(t), ref(op), ref(p), it, rel, hist, hs, None, cm, None)
        return lib.mugiq_hip_mg_precondition(out, inp, n, ref(g), ref(c), 0.1, ref(t), ref(op), ref(p), cm, None)

    def expect(st, frag, status=1):
        msg = lib.mugiq_hip_last_error().decode()
        assert st == status, (st, msg)
        assert msg.startswith(who) and frag in msg, msg

    for kw in (dict(out=None), dict(inp=None), dict(g=None), dict(t=None), dict(op=None)):
        expect(run(**kw), "NULL argument")
    expect(run(p=None), "param is NULL")
    expect(run(n=0), "nVec = 0 must be >= 1")
    if entry == "solve":
        expect(run(it=None), "NULL argument")
        expect(run(rel=None), "NULL argument")
        expect(run(hist=(ctypes.c_double * 8)(), hs=4), "historyStride = 4 is smaller than maxIter = 1000")
    expect(run(p=_param(hip, tol=0.0)), "tol = 0 must be positive")
    expect(run(p=_param(hip, tol=-1e-3)), "must be positive")
    expect(run(p=_param(hip, maxIter=-1)), "maxIter = -1 non-negative")
    for k, bad in (("nKrylov", (0, 17)), ("nuPre", (-1, 17)), ("nuPost", (-1, 17)), ("coarseIters", (-1, 17))):
        for v in bad:
            expect(run(p=_param(hip, **{k: v})), "%s = %d" % (k, v))
    # the limits of the coarse operator: a single domain
    expect(run(comm=_comm(size=2, grid=(1, 1, 1, 2))), "single domain", status=2)
    expect(run(comm=_comm(partitioned=(0, 1, 0, 0))), "single domain", status=2)
    # precision 4 anywhere: an fp32 hierarchy is not supported
    expect(run(t=_transfer(prec=4)), "fp64 only", status=2)
    expect(run(op=_op(prec=4)), "fp64 only", status=2)
    expect(run(out=_fields(1 << 40, prec=4)), "fp64 only", status=2)
    expect(run(inp=_fields(1 << 41, prec=4)), "fp64 only", status=2)
    # geometry
    expect(run(inp=_fields(1 << 41, pad=7)), "differs in precision, field order, geometry, stride or parity offset")
    expect(run(inp=_fields(1 << 41, order=4)), "differs in precision, field order, geometry, stride or parity offset")
    expect(run(out=_arr([_spinor(1 << 40), _spinor((1 << 40) + SPAN, X=(8, 8, 8, 4))]), inp=in0), "differs in precision")
    expect(run(op=_op(nvec=5)), "the coarse operator has n_vec 5, the transfer 4")
    expect(run(op=_op(X=(2, 2, 2, 4))), "coarse operator X[3] = 4, the transfer's coarse lattice has 2")
    expect(run(t=_transfer(X=(8, 8, 8, 16)), op=_op(X=(2, 2, 2, 4))), "the fields have X[3] = 8, the transfer 16")
    expect(run(g=_gauge(X=(8, 8, 8, 4))), "gauge X[3] = 4")
    from mugiq_amd._lib import CloverDesc
    c = CloverDesc()
    c.data, c.precision, c.volumeCB, c.stride, c.parity_offset = ctypes.c_void_p(1 << 37), 4, 2048, 2048, 36 * 2048
    for i in range(4):
        c.X[i] = 8
    expect(run(c=c), "clover precision 4 differs from the gauge precision 8")
    # the coarse operator of another M
    other = _op()
    other.kappa = 0.2
    expect(run(op=other), "the coarse operator was built for kappa = 0.2")
    other = _op()
    other.hasClover = 1
    expect(run(op=other), "the coarse operator was built with a clover field, the call is without one")
    # overlap
    o, i_ = ("x", "b") if entry == "solve" else ("z", "r")
    expect(run(out=_arr([_spinor(1 << 40), _spinor((1 << 40) + 64)])), "%s vector 1 overlaps %s vector 0" % (o, o))
    expect(run(out=in0), "%s vector 0 overlaps %s vector 0" % (o, i_))
    expect(run(out=_fields((1 << 41) + SPAN - 64)), "%s vector 0 overlaps %s vector 0" % (o, i_))


def test_python_wrappers_check_their_arguments(hip):
    with pytest.raises(hip.MugiqHipError):
        hip.mgSolve([], None, 0.1, None, None)
    with pytest.raises(hip.MugiqHipError):
        hip.mgPrecondition([object()], [], None, 0.1, None, None)
    es = hip.Eigsolve_Mugiq([], None, 0.1)
    with pytest.raises(hip.MugiqHipError, match="status 2"):
        es.solveMG([object()])


def test_cpp_mirror_compiles(tmp_path):
    """MgSolveParam, mgPrecondition and mgSolve of include/mugiq_hip_operators.hpp, -fsyntax-only against the header."""
    tu = tmp_path / "mg_solve_tu.cpp"
    tu.write_text('#include "mugiq_hip_operators.hpp"\n'
                  "bool use(const std::vector<MugiqHipSpinorField> &x, const std::vector<MugiqHipSpinorField> &b, const MugiqHipTransfer &T,\n"
                  "         const MugiqHipCloverField *clover, const MugiqHipComm *comm) {\n"
                  "  const int Xc[4] = {2, 2, 2, 2};\n"
                  "  mugiq_hip::CoarseOperator op(Xc, T.nVec, T.precision);\n"
                  "  MugiqHipGaugeField U{};\n"
                  "  mugiq_hip::MgSolveParam prm;\n"
                  "  prm.nuPost = 2;\n"
                  "  mugiq_hip::mgPrecondition(x, b, U, clover, 0.1, T, op);\n"
                  "  mugiq_hip::mgPrecondition(x, b, U, nullptr, 0.1, T, op, prm, comm);\n"
                  "  std::vector<int> iters;\n"
                  "  std::vector<double> relres;\n"
                  "  std::vector<std::vector<double>> history;\n"
                  "  int reads = 0;\n"
                  "  bool ok = mugiq_hip::mgSolve(x, b, U, clover, 0.1, T, op, prm, iters, relres);\n"
                  "  return ok && mugiq_hip::mgSolve(x, b, U, clover, 0.1, T, op, prm, iters, relres, &history, &reads, comm);\n"
                  "}\n")
    cc = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cc):
        pytest.skip("no clang++")
    r = subprocess.run([cc, "-std=c++17", "-fsyntax-only", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-Wall", "-I", os.path.join(ROOT, "include"),
                        "-I", "/opt/rocm/include", str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
