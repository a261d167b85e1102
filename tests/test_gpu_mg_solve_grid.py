"""GPU tests of the two-grid cycle and solve on a process grid (mugiq_hip_mg_precondition_grid, mugiq_hip_mg_solve_grid; the rank table
and mg_rank_sum_kernel).  On one rank with the partitioned path forced the stencil and the coarse application are the bits of their
single-domain forms (tests/test_gpu_wilson.py, tests/test_gpu_coarse_op_grid.py) and no sum over ranks is made, so the cycle and the whole
solve must be the BITS of mgPrecondition / mgSolve on the same fields.  On 2 and 4 gloo ranks (tests/mg_solve_grid_workers.py) every inner
product is added per rank first, so K is held to the numpy K of the global problem (1e-12 of its max norm, the bound of
tests/test_gpu_mg_solve.py) and the solve to the restatement's iteration counts, to its history within 100 x its own 1-ulp sensitivity, and
to the true residual numpy computes from the gathered x; what the ranks report must be identical bits."""
import functools

import numpy as np
import pytest
import torch.multiprocessing as mp

import clover_ref as cr
import coarse_op_grid_ref as gr
import mg_solve_cases as mgc
import mg_solve_grid_ref as mgg
import mg_solve_grid_workers as workers
import mg_solve_ref as mgr
from mg_solve_fields import field as _field, pads_are_nan as _pads_are_nan, same as _same
from test_gpu_coarse_op_grid import FORCES, _border, _comm
from test_multi_rank_cpu import free_port
from util import orc, random_gauge_lex

pytestmark = pytest.mark.gpu

CSW = 0.17
K_SETS = mgc.K_PARAMS + [mgc.EDGE_PARAMS[0]]
# the solve: restarts, and a smoothing step before the correction; on the smooth field the set of mg_solve_cases.SOLVES that restarts
SOLVE = {"hot": dict(nKrylov=4, nuPre=1, nuPost=2), "smooth": dict(nKrylov=4, nuPost=4), "ragged": dict(nKrylov=4, nuPre=1, nuPost=2)}
# name -> (X, aggregate, n_vec, kappa, clover, field order, pad, maxIter): the hot and the smooth 4^4 field of mg_solve_cases and RAGGED
# (rows that cut a wave; random null vectors, so its solve is stopped after 5 iterations: status 5 with everything filled)
SHAPES = {"hot": (mgc.X4, mgc.BS, mgc.NVEC, mgc.KAPPA["hot"], True, 2, 0, 1000),
          "smooth": (mgc.X4, mgc.BS, mgc.NVEC, mgc.KAPPA["smooth"], False, 4, 7, 1000),
          "ragged": mgc.RAGGED + (0.12, True, 2, 5, 5)}


def _c(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


class _Case:
    """the fields of one shape and the results of the EXISTING single-domain calls on them, made once"""

    def __init__(self, hip, name):
        self.X, bs, nvec, self.kappa, clover, self.order, self.pad, self.maxIter = SHAPES[name]
        X, self.prm = self.X, SOLVE[name]
        rng = np.random.default_rng(8100 + len(name))
        if name == "ragged":
            self.U_lex = random_gauge_lex(rng, X)
            V = _c(rng, (2, int(np.prod(X)) // 2, 4, 3, nvec)) / np.sqrt(12.0 * nvec)
        else:
            self.U_lex, V = mgc.links(name)[0], mgc.null_vectors(name)
        self.C = hip.CloverField(X, 8).set_logical(cr.clover_blocks_eo(self.U_lex, CSW, X)) if clover else None
        self.T = hip.Transfer(X, nvec, bs, 2, 8).set_logical(V)
        self.op = hip.computeCoarseOperator(self.T, self.gauge(hip, (0, 0, 0, 0)), self.kappa, clover=self.C)
        self.rhs = [_c(rng, (2, int(np.prod(X)) // 2, 4, 3)) for _ in range(9)]
        self.rhs[4] = np.zeros_like(self.rhs[4])                   # a zero right-hand side inside the block of 8
        self.K = {(ip, n): self.cycle(hip, None, None, ip, n) for ip in range(len(K_SETS)) for n in (1, 8, 9)}
        self.solves = {n: self.solve(hip, None, None, n) for n in (1, 9)}

    def gauge(self, hip, brd):
        return hip.GaugeField(self.X, brd, 8).set_logical(orc.extended_gauge_from_global(self.U_lex, (0, 0, 0, 0), (1, 1, 1, 1), brd))

    def fields(self, hip, n, inputs=True):
        return [_field(hip, self.X, self.rhs[k] if inputs else None, self.order, self.pad) for k in range(n)]

    def grid_operator(self, hip, force):
        comm = _comm(hip, force)
        g = self.gauge(hip, _border(force))
        return g, hip.computeCoarseOperatorGrid(self.T, g, self.kappa, comm, clover=self.C), comm

    def cycle(self, hip, grid, comm, ip, n):
        r, z = self.fields(hip, n), self.fields(hip, n, False)
        if comm is None:
            hip.mgPrecondition(z, r, self.gauge(hip, (0, 0, 0, 0)), self.kappa, self.T, self.op, clover=self.C, **K_SETS[ip])
        else:
            hip.mgPreconditionGrid(z, r, grid[0], self.kappa, self.T, grid[1], comm, clover=self.C, **K_SETS[ip])
        assert not self.pad or all(_pads_are_nan(f) for f in z + r)
        return z

    def solve(self, hip, grid, comm, n):
        b, x = self.fields(hip, n), self.fields(hip, n, False)
        kw = dict(x=x, clover=self.C, maxIter=self.maxIter, allow_unconverged=self.maxIter < 1000, **self.prm)
        if comm is None:
            _, info = hip.mgSolve(b, self.gauge(hip, (0, 0, 0, 0)), self.kappa, self.T, self.op, **kw)
            ginfo = None
        else:
            _, info, ginfo = hip.mgSolveGrid(b, grid[0], self.kappa, self.T, grid[1], comm, **kw)
        assert not self.pad or all(_pads_are_nan(f) for f in x + b)
        return x, info, ginfo

    def check(self, hip, force):
        """the grid entry points under the forced partition `force` against the stored results: every bit and every count"""
        g, opg, comm = self.grid_operator(hip, force)
        for (ip, n), want in self.K.items():
            got = self.cycle(hip, (g, opg), comm, ip, n)
            assert all(_same(a, b) for a, b in zip(got, want)), (force, K_SETS[ip], n)
        prm = dict(mgr.DEFAULTS, **self.prm)
        for n, (xw, iw, _) in self.solves.items():
            x, info, ginfo = self.solve(hip, (g, opg), comm, n)
            assert all(_same(a, b) for a, b in zip(x, xw)), (force, n)
            assert np.array_equal(info.iters, iw.iters) and np.array_equal(info.relres.view(np.int64), iw.relres.view(np.int64)), (force, n)
            assert info.hostReads == iw.hostReads and info.converged == iw.converged == (self.maxIter == 1000)
            assert all(np.array_equal(p.view(np.int64), q.view(np.int64)) for p, q in zip(info.history, iw.history)), (force, n)
            if n == 9:
                assert info.iters[4] == 0 and info.relres[4] == 0.0 and not np.any(x[4].get_logical())
            blocks = [int(np.max(info.iters[v0:v0 + 8])) for v0 in range(0, n, 8)]
            fine, coarse = (sum(e) for e in zip(*[workers.expected_exchanges(it, prm) for it in blocks]))
            assert ginfo == hip.MgSolveGridInfo(fine, coarse, 0, 0), (force, n, ginfo, blocks)


@functools.lru_cache(maxsize=None)
def _case(hip, name):
    return _Case(hip, name)


@pytest.mark.parametrize("force", FORCES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_forced_partitioning_is_the_single_domain_cycle_and_solve(hip, name, force):
    """Each axis alone, z + t and all four.  mgPreconditionGrid for five parameter sets (nuPre > 0, omega != 1, 16 coarse steps, no coarse
    step among them) in batches of 1, 8 and 9 equals mgPrecondition bit for bit; mgSolveGrid of 1 and 9 right-hand sides (a zero one inside
    the block) equals mgSolve in x, iters, relres, histories and hostReads; rankSums = rankSumMessages = 0; the exchange counts are those of
    the launch sequence.  hot: FLOAT2 with clover; smooth: FLOAT4 with NaN pads, no clover; ragged: 6 6 6 4, FLOAT2 with NaN pads."""
    _case(hip, name).check(hip, force)


def test_forced_partitioning_under_poisoned_lds(hip, monkeypatch):
    """MUGIQ_HIP_DEBUG_POISON_LDS=1: no kernel of the grid cycle reads an LDS cell it has not written"""
    c = _case(hip, "ragged")
    monkeypatch.setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")
    c.check(hip, (1, 1, 1, 1))


def test_unpartitioned_comm_is_the_existing_call_and_the_existing_calls_still_refuse(hip):
    c = _case(hip, "hot")
    g, opg, comm = c.grid_operator(hip, (0, 0, 0, 0))
    assert opg.halo is None
    z = c.cycle(hip, (g, opg), comm, 1, 9)
    assert all(_same(a, b) for a, b in zip(z, c.K[1, 9]))
    x, info, ginfo = c.solve(hip, (g, opg), comm, 9)
    assert all(_same(a, b) for a, b in zip(x, c.solves[9][0])) and np.array_equal(info.iters, c.solves[9][1].iters)
    assert ginfo == hip.MgSolveGridInfo(0, 0, 0, 0)
    part = _comm(hip, (0, 0, 0, 1))
    with pytest.raises(hip.MugiqHipError, match="status 2"):
        hip.mgSolve(c.fields(hip, 1), g, c.kappa, c.T, c.op, clover=c.C, comm=part)
    with pytest.raises(hip.MugiqHipError, match="status 2"):
        hip.mgPrecondition(c.fields(hip, 1, False), c.fields(hip, 1), g, c.kappa, c.T, c.op, clover=c.C, comm=part)
    with pytest.raises(hip.MugiqHipError, match="coarse halo is NULL"):
        hip.mgSolveGrid(c.fields(hip, 1), c.gauge(hip, (0, 0, 0, 2)), c.kappa, c.T, c.op, part, clover=c.C)


# ---- 2 and 4 ranks -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _numpy_side(G):
    """K of the global problem for the two parameter sets of the worker, and per solve parameter set the margin tolerance, the
    restatement's iterations and history for b0, and its largest relative deviation under three 1-ulp perturbations of b0 (the rule of
    mg_solve_cases.history_sensitivity)"""
    prob = mgg.global_problem(G)
    b0 = mgg.rhs(G, 2)[0]
    out = {"K%d" % ip: mgr.K(prob, b0, **prm) for ip, prm in enumerate((mgc.K_PARAMS[1], mgc.EDGE_PARAMS[0]))}
    for ks, (nKrylov, nuPost) in enumerate(((16, 4), (4, 2))):
        tol, runs = mgc.solve_with_margin(prob, [b0], nKrylov=nKrylov, nuPost=nuPost)
        _, it, hist = runs[0]
        worst = 0.0
        for seed in (1, 2, 3):
            _, it2, h2, ok = mgr.solve(prob, mgr.ulp_perturbed(b0, seed), tol=tol, nKrylov=nKrylov, nuPost=nuPost)
            assert ok and it2 == it
            worst = max(worst, float(np.max(np.abs(h2 - hist) / hist)))
        out.update({"tol%d" % ks: tol, "iters%d" % ks: it, "hist%d" % ks: hist, "scale%d" % ks: worst})
    return out


@pytest.mark.parametrize("G,grid", [((4, 4, 4, 8), (1, 1, 1, 2)), ((8, 4, 4, 8), (2, 1, 1, 2)), ((4, 4, 4, 16), (1, 1, 1, 4)), ((16, 4, 4, 4), (4, 1, 1, 1))])
def test_process_grids(G, grid, tmp_path):
    """Every rank on the one GPU through gloo, fields the rank's slices of the global problem.  Asserted in the worker: K within 1e-12 of
    the numpy K; per parameter set (nKrylov 16 / nuPost 4 and nKrylov 4 / nuPost 2) the restatement's iterations, the history within
    100 x its sensitivity, the zero right-hand side, hostReads, rankSums, rankSumMessages and the exchange counts.  Here: the true residual
    of the gathered x from numpy is <= tol and relres agrees with it to 1e-6; iters, relres, histories, hostReads and the grid info are
    identical bits on all ranks."""
    side = _numpy_side(G)
    npz = str(tmp_path / "numpy_side.npz")
    np.savez(npz, **side)
    world = int(np.prod(grid))
    prefix = str(tmp_path / "mg")
    mp.spawn(workers.solve_worker, args=(world, free_port(), grid, G, npz, prefix), nprocs=world, join=True)
    outs = [np.load("%s_%d.npz" % (prefix, r)) for r in range(world)]
    prob = mgg.global_problem(G)
    bs = mgg.rhs(G, 2)
    coords = gr.ranks(grid)
    for ks in range(2):
        same = [o["same%d" % ks] for o in outs]
        assert np.all(np.isfinite(same[0])) and all(np.array_equal(s.view(np.int64), same[0].view(np.int64)) for s in same[1:])
        tol = float(side["tol%d" % ks])
        for slot, b in ((0, bs[0]), (2, bs[1])):
            x = gr.assemble_eo({c: outs[r]["x%d_%d" % (ks, slot)] for r, c in enumerate(coords)}, G, grid)
            true = float(np.linalg.norm(b - prob.M(x)) / np.linalg.norm(b))
            relres = float(same[0][3 + slot])
            print("G %s grid %s set %d rhs %d: true residual %.3e, relres %.3e, tol %.3e" % (G, grid, ks, slot, true, relres, tol))
            assert true <= tol and abs(relres - true) <= 1e-6 * true, (ks, slot, true, relres, tol)
