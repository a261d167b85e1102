"""CPU checks of the two-grid solve on a process grid (mugiq_hip_mg_precondition_grid, mugiq_hip_mg_solve_grid): the numpy model with
rank-blocked inner products (tests/mg_solve_grid_ref.py) makes the outer iteration counts of the global restatement; the message schedule
of the rank sum (mugiq_hip_mg_rank_sum_plan), run for every rank on a simulated network, fills every table exactly once and reads nothing
early; every refusal of the two entry points comes back before any device work (the descriptors point at nothing); the entry points are
declared, exported and bound; the C++ overloads compile."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import coarse_op_grid_ref as gr
import mg_solve_cases as mgc
import mg_solve_grid_ref as mgg
import mg_solve_ref as mgr
from test_coarse_op_cpu import _ptr
from test_coarse_op_grid_cpu import _halo, _pcomm
from test_mg_solve_cpu import SPAN, _arr, _fields, _gauge, _op, _param, _spinor, _transfer
from util import ROOT

NEW = ["mugiq_hip_mg_precondition_grid", "mugiq_hip_mg_solve_grid", "mugiq_hip_mg_rank_sum_plan"]
# global lattice, process grid
MODEL_CASES = [((4, 4, 4, 8), (1, 1, 1, 2)), ((8, 4, 4, 8), (2, 1, 1, 2)), ((4, 4, 4, 16), (1, 1, 1, 4))]
# (nKrylov, nuPost) and the outer iterations of the global restatement for the right-hand side default_rng(1) at tol 1e-10, as recorded on
# the machine that wrote this, the same on all three lattices (another BLAS may move a count by one: the model is held to the global
# restatement of the run, and the recorded counts to within one).  nKrylov 4 restarts four times
PARAMS = [(16, 4), (4, 2)]
COUNTS = {(16, 4): 10, (4, 2): 18}
PLAN_GRIDS = [(1, 1, 1, 2), (2, 1, 1, 2), (1, 1, 2, 4), (2, 2, 2, 2), (4, 1, 1, 1), (1, 1, 3, 1)]


@functools.lru_cache(maxsize=None)
def global_runs(G, nKrylov, nuPost):
    """(tol with the 1 % margin from 1e-10 downwards, [(x, iterations, history)]) of mg_solve_ref.solve on the global problem"""
    return mgc.solve_with_margin(mgg.global_problem(G), list(mgg.rhs(G)), nKrylov=nKrylov, nuPost=nuPost)


@pytest.mark.parametrize("nKrylov,nuPost", PARAMS)
@pytest.mark.parametrize("G,grid", MODEL_CASES)
def test_grid_model_keeps_the_counts_of_the_global_restatement(G, grid, nKrylov, nuPost):
    """Every inner product a sum of per-rank parts in ascending rank order: the outer iterations of mg_solve_ref.solve on the global
    problem at the margin tolerance, a history that agrees to rounding, and a true residual below tol."""
    prob = mgg.global_problem(G)
    tol, runs = global_runs(G, nKrylov, nuPost)
    x0, it0, hist0 = runs[0]
    b = mgg.rhs(G)[0]
    x, it, hist, ok = mgg.solve(prob, mgg.RankDot(G, grid), b, tol=tol, nKrylov=nKrylov, nuPost=nuPost)
    print("G %s grid %s nKrylov %d nuPost %d: %d iterations (global restatement %d, recorded %d), tol %.3e" % (G, grid, nKrylov, nuPost, it, it0,
                                                                                                             COUNTS[(nKrylov, nuPost)], tol))
    assert ok and it == it0 == len(hist)
    assert abs(it0 - COUNTS[(nKrylov, nuPost)]) <= 1 and 0.5e-10 < tol <= 1e-10
    if nKrylov == 4:
        assert it0 > 4 * nKrylov                                   # four restarts
    assert np.max(np.abs(hist - hist0) / hist0) < 1e-6
    assert np.linalg.norm(b - prob.M(x)) / np.linalg.norm(b) <= tol * (1 + 1e-6)


def test_rank_dot_is_the_global_inner_product():
    G, grid = MODEL_CASES[1]
    dot = mgg.RankDot(G, grid)
    assert sorted(np.concatenate(dot.sites[int(np.prod(G)) // 2])) == list(range(int(np.prod(G))))         # the blocks tile the lattice
    rng = np.random.default_rng(5)
    for shape in ((2, int(np.prod(G)) // 2, 4, 3), (2, int(np.prod(G)) // 32, 2, mgg.NVEC)):
        a, b = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape) for _ in range(2))
        assert abs(dot(a, b) - np.vdot(a, b)) <= 1e-13 * np.linalg.norm(a) * np.linalg.norm(b)
    one = mgg.RankDot(G, (1, 1, 1, 1))
    assert one(a, b) == np.vdot(a.reshape(-1), b.reshape(-1))


def test_K_of_the_model_is_the_K_of_the_restatement():
    G, grid = MODEL_CASES[0]
    prob = mgg.global_problem(G)
    r = mgg.rhs(G)[0]
    for prm in (mgc.K_PARAMS[1], mgc.EDGE_PARAMS[0]):
        want, got = mgr.K(prob, r, **prm), mgg.K(prob, mgg.RankDot(G, grid), r, **prm)
        assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), prm


# ---- the schedule of the rank sum ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", PLAN_GRIDS)
def test_rank_sum_plan_completes_every_table(hip, grid):
    """The plan of every rank on a simulated network: sum (grid[d] - 1) messages, t first; no message reads an entry before it was filled;
    after the last one every rank's table holds every rank's entry, each written exactly once."""
    size = int(np.prod(grid))
    tables, writes = mgg.simulate_gather(grid, lambda c: hip.mgRankSumPlan(grid, c))
    nmsg = sum(g - 1 for g in grid)
    for c in gr.ranks(grid):
        plan = hip.mgRankSumPlan(grid, c)
        assert len(plan) == nmsg
        dims = [m[0] for m in plan]
        assert dims == sorted(dims, reverse=True) and all(grid[d] > 1 for d in dims)     # fastest axis first, no axis of extent 1
        me = mgg.rank_of(c, grid)
        assert tables[me] == list(range(size)), (c, tables[me])
        assert writes[me] == [1] * size, (c, writes[me])


def test_rank_sum_plan_arguments(hip):
    lib = hip._lib.load()
    i4 = hip._lib.int4
    call = lib.mugiq_hip_mg_rank_sum_plan
    assert call(i4((1, 1, 2, 4)), i4((0, 0, 1, 3)), 0, None, None, None, None) == 4
    assert call(i4((1, 1, 1, 1)), i4((0, 0, 0, 0)), 0, None, None, None, None) == 0
    assert call(None, i4((0, 0, 0, 0)), 0, None, None, None, None) == -1
    assert call(i4((1, 1, 2, 4)), i4((0, 0, 2, 0)), 0, None, None, None, None) == -1
    assert call(i4((1, 0, 2, 4)), i4((0, 0, 0, 0)), 0, None, None, None, None) == -1
    dim = (ctypes.c_int * 2)(7, 7)                                                        # maxOps below the count: only that many are filled
    assert call(i4((1, 1, 2, 4)), i4((0, 0, 1, 3)), 1, dim, None, None, None) == 4 and list(dim) == [3, 7]
    # 1 1 2 4, rank (z 1, t 3) = 7: t sends its own entry first, then what it received; z sends the run of four
    assert hip.mgRankSumPlan((1, 1, 2, 4), (0, 0, 1, 3)) == [(3, 7, 6, 1), (3, 6, 5, 1), (3, 5, 4, 1), (2, 4, 0, 4)]
    with pytest.raises(hip.MugiqHipError):
        hip.mgRankSumPlan((1, 1, 1, 2), (0, 0, 0, 2))


# ---- the C ABI without a device -----------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound(hip):
    hdr = open(os.path.join(ROOT, "include", "mugiq_hip.h")).read()
    lib = hip._lib.load()
    for name in NEW:
        assert name + "(" in hdr
        assert hasattr(lib, name) and name in hip._lib.SIGNATURES
    assert "MugiqHipMgSolveGridInfo" in hdr
    assert [f[0] for f in hip._lib.MgSolveGridInfo._fields_] == ["fineExchanges", "coarseExchanges", "rankSums", "rankSumMessages"]
    for name in ("mgPreconditionGrid", "mgSolveGrid", "mgRankSumPlan", "MgSolveGridInfo"):
        assert hasattr(hip, name)
    with pytest.raises(hip.MugiqHipError):
        hip.mgSolveGrid([object()], None, 0.1, None, None, None)
    with pytest.raises(hip.MugiqHipError):
        hip.mgPreconditionGrid([object()], [object()], None, 0.1, None, None, None)


def _ghosted(base, n=2, dims=(0, 0, 0, 1), **kw):
    out = []
    for i in range(n):
        f = _spinor(base + i * SPAN, **kw)
        for d in range(4):
            for b in range(2):
                f.ghost[d][b] = (1 << 44) + ((i * 4 + d) * 2 + b) * (1 << 24) if dims[d] else None
        out.append(f)
    return _arr(out)


def _border_gauge(dims=(0, 0, 0, 1)):
    g = _gauge()
    R = [2 * d for d in dims] if sum(dims) % 2 else list(dims)
    v = 1
    for i in range(4):
        g.R[i] = R[i]
        v *= g.X[i] + 2 * R[i]
    g.stride, g.parity_offset = v // 2, 36 * (v // 2)
    return g


@pytest.mark.parametrize("entry", ["solve", "precondition"])
def test_grid_refusals_without_a_device(hip, entry):
    """NULL comm, a partitioned axis without a halo (or with the halo of another operator), precision 4, r without ghost zones, an
    operator that does not belong to the transfer, bad parameters, a comm that does not describe one grid: each refused with its status
    before any HIP call."""
    lib = hip._lib.load()
    who = "mgSolveGrid: " if entry == "solve" else "mgPreconditionGrid: "
    out0, in0 = _fields(1 << 40), _ghosted(1 << 41)
    iters, relres = (ctypes.c_int * 2)(), (ctypes.c_double * 2)()
    ginfo = hip._lib.MgSolveGridInfo()

    def run(out=out0, inp=in0, n=2, g=_border_gauge(), t=_transfer(), op=_op(), halo=_halo(), p=_param(hip), comm=_pcomm(), gi=ginfo, it=iters):
        ref = lambda x: ctypes.byref(x) if x is not None else None                                    # noqa: E731
        if entry == "solve":
            return lib.mugiq_hip_mg_solve_grid(out, inp, n, ref(g), None, 0.1, ref(t), ref(op), ref(halo), ref(p), it, relres, None, 0, None, ref(gi),
                                               _ptr(comm), None)
        return lib.mugiq_hip_mg_precondition_grid(out, inp, n, ref(g), None, 0.1, ref(t), ref(op), ref(halo), ref(p), _ptr(comm), None)

    def expect(st, frag, status=1):
        msg = lib.mugiq_hip_last_error().decode()
        assert st == status, (st, msg)
        assert msg.startswith(who) and frag in msg, msg

    expect(run(comm=None), "comm is NULL")
    expect(run(comm=_pcomm(sendrecv=False)), "comm->sendrecv is NULL")
    expect(run(halo=None), "partitioned axis but the coarse halo is NULL")
    expect(run(halo=None, comm=_pcomm(size=2, grid=(1, 1, 1, 2), partitioned=(0, 0, 0, 0))), "partitioned axis but the coarse halo is NULL")
    expect(run(halo=_halo(nvec=5)), "does not belong to the coarse operator")
    expect(run(halo=_halo(dims=(0, 0, 0, 1)), comm=_pcomm(partitioned=(0, 0, 1, 1))), "dimension 2 is partitioned but the coarse halo was not built for it")
    # precision 4 anywhere
    expect(run(t=_transfer(prec=4)), "fp64 only", status=2)
    expect(run(op=_op(prec=4), halo=_halo(prec=4)), "fp64 only", status=2)
    expect(run(out=_fields(1 << 40, prec=4)), "fp64 only", status=2)
    expect(run(inp=_ghosted(1 << 41, prec=4)), "fp64 only", status=2)
    # the operator and the transfer
    expect(run(op=_op(nvec=5), halo=_halo(nvec=5)), "the coarse operator has n_vec 5, the transfer 4")
    expect(run(op=_op(X=(2, 2, 2, 4)), halo=_halo(X=(2, 2, 2, 4))), "coarse operator X[3] = 4, the transfer's coarse lattice has 2")
    other = _op()
    other.kappa = 0.2
    expect(run(op=other), "the coarse operator was built for kappa = 0.2")
    # parameters
    expect(run(p=None), "param is NULL")
    expect(run(p=_param(hip, tol=0.0)), "tol = 0 must be positive")
    for k, bad in (("nKrylov", (0, 17)), ("nuPre", (-1, 17)), ("nuPost", (-1, 17)), ("coarseIters", (-1, 17))):
        for v in bad:
            expect(run(p=_param(hip, **{k: v})), "%s = %d" % (k, v))
    expect(run(n=0), "nVec = 0 must be >= 1")
    # a gauge field without a border on the partitioned axis
    expect(run(g=_gauge()), "dimension 3 is partitioned but the gauge field has no border")
    # a comm whose grid, coordinates, rank and size do not describe one grid: the rank table would be addressed outside itself
    expect(run(comm=_pcomm(size=2, grid=(1, 1, 1, 4))), "do not match size 2")
    bad = _pcomm(size=2, grid=(1, 1, 1, 2))
    bad.coord[3] = 1
    expect(run(comm=bad), "do not match size 2")
    bad = _pcomm(size=2, grid=(1, 1, 1, 2))
    bad.coord[3] = 2
    expect(run(comm=bad), "coord[3] = 2")
    if entry == "precondition":
        # r is read by the stencil in place
        expect(run(inp=_fields(1 << 41)), "dimension 3 is partitioned but r vector 0 has no ghost zones for it")
        expect(run(inp=_ghosted(1 << 41, dims=(0, 0, 0, 1)), g=_border_gauge((0, 0, 1, 1)), comm=_pcomm(partitioned=(0, 0, 1, 1))),
               "dimension 2 is partitioned but r vector 0 has no ghost zones for it")
    else:
        expect(run(gi=None), "NULL argument")
        expect(run(it=None), "NULL argument")
    # the existing entry points keep refusing a partitioned comm
    st = lib.mugiq_hip_mg_precondition(out0, in0, 2, ctypes.byref(_gauge()), None, 0.1, ctypes.byref(_transfer()), ctypes.byref(_op()),
                                       ctypes.byref(_param(hip)), _ptr(_pcomm()), None)
    assert st == 2 and "single domain" in lib.mugiq_hip_last_error().decode()


def test_cpp_mirror_compiles(tmp_path):
    """the overloads of mgPrecondition and mgSolve in include/mugiq_hip_operators.hpp that take a MugiqHipCoarseHalo, -fsyntax-only against
    the header, beside the single-domain calls they overload (no ambiguity)"""
    tu = tmp_path / "mg_solve_grid_tu.cpp"
    tu.write_text('#include "mugiq_hip_operators.hpp"\n'
                  "int use(const std::vector<MugiqHipSpinorField> &x, const std::vector<MugiqHipSpinorField> &b, const MugiqHipTransfer &T,\n"
                  "        const MugiqHipCloverField *clover, const MugiqHipCoarseHalo &halo, const MugiqHipComm *comm) {\n"
                  "  const int Xc[4] = {2, 2, 2, 2};\n"
                  "  mugiq_hip::CoarseOperator op(Xc, T.nVec, T.precision);\n"
                  "  MugiqHipGaugeField U{};\n"
                  "  mugiq_hip::MgSolveParam prm;\n"
                  "  mugiq_hip::mgPrecondition(x, b, U, clover, 0.1, T, op, halo, prm, comm);\n"
                  "  mugiq_hip::mgPrecondition(x, b, U, clover, 0.1, T, op, prm, comm);\n"
                  "  std::vector<int> iters;\n"
                  "  std::vector<double> relres;\n"
                  "  std::vector<std::vector<double>> history;\n"
                  "  int reads = 0;\n"
                  "  MugiqHipMgSolveGridInfo gi{};\n"
                  "  bool ok = mugiq_hip::mgSolve(x, b, U, clover, 0.1, T, op, halo, prm, iters, relres, gi, comm, &history, &reads);\n"
                  "  ok = ok && mugiq_hip::mgSolve(x, b, U, clover, 0.1, T, op, prm, iters, relres, &history, &reads, comm);\n"
                  "  return ok + gi.fineExchanges + gi.coarseExchanges + gi.rankSums + gi.rankSumMessages;\n"
                  "}\n")
    cc = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cc):
        pytest.skip("no clang++")
    r = subprocess.run([cc, "-std=c++17", "-fsyntax-only", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-Wall", "-I", os.path.join(ROOT, "include"),
                        "-I", "/opt/rocm/include", str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
