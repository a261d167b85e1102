"""GPU tests of the coarse eigensolver on a process grid (mugiq_hip_coarse_gram_grid, mugiq_hip_coarse_eigensolve_grid;
chebyshev_step_pack_kernel).  On one rank with the partitioned path forced the applications are the bits of coarseApply
(tests/test_gpu_coarse_op_grid.py) and a sum over one rank adds nothing, so the whole solve must be the BITS of coarseEigensolve on the same
operator and start vectors -- under both settings of MUGIQ_HIP_EIG_PACK_IN_STEP, which differ only in who writes the send faces of an
application.  On 2 and 4 gloo ranks (tests/coarse_eig_grid_workers.py) the Gram sums are added in another order than on one domain, so the
solve is held to the numpy restatement's counts (tests/coarse_eig_ref.py; tests/test_coarse_eig_grid_cpu.py shows the rank decomposition
keeps them) and to numpy.linalg.eigvalsh under the rule of test_solver_matches_restatement_and_eigh."""
import functools

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import coarse_eig_cases as cec
import coarse_eig_grid_ref as cg
import coarse_eig_grid_workers
import coarse_op_cases as cases
import coarse_op_ref as cor
from test_gpu_coarse_op_grid import FORCES, KAPPA, _border, _comm, _gauge, _links
from test_multi_rank_cpu import free_port

pytestmark = pytest.mark.gpu

NAN = complex(float("nan"), float("nan"))
ENV = "MUGIQ_HIP_EIG_PACK_IN_STEP"
# fine X, aggregate, n_vec, (nConv, nKr)
FORCED = [cases.SHAPES[0] + (cec.SIZES[0],),                 # coarse 2^4: every site is on a face of every forced axis
          cases.SHAPES[2] + (cec.SIZES[2],),                 # extent 4 along x, N = 10: interior and face sites share a wave
          cases.ANISO[0] + ((8, 24),),                       # coarse 2 4 6 2: pairwise distinct extents, sites on no face of z, volumeCB 48
          cases.ANISO[1] + ((16, 32),),                      # coarse 6 2 4 2: the 6 on the checkerboard axis
          ((4, 8, 12, 4), (2, 2, 2, 2), 24, (16, 32))]       # vectors of 4608 elements: two Gram chunks, the second one ragged


class _Case:
    """operator, start vectors and the single-domain solve of one shape, made once"""

    def __init__(self, hip, X, bs, nvec, sizes):
        self.X, self.nvec, (self.nConv, self.nKr) = X, nvec, sizes
        V, _ = cases.null_vectors(X, bs, nvec)
        self.C = hip.CloverField(X, 8).set_logical(_links(X)[1])
        self.T = hip.Transfer(X, nvec, bs, 2, 8).set_logical(V)
        self.op = hip.computeCoarseOperator(self.T, _gauge(hip, X, (0, 0, 0, 0)), KAPPA, clover=self.C)
        rng = np.random.default_rng(7650 + sum(X) + nvec)
        shape = (2, self.op.volumeCB, 2, nvec)
        self.S = [rng.standard_normal(shape) + 1j * rng.standard_normal(shape) for _ in range(self.nKr)]
        self.ref = self.solve(hip, None, None)

    def start(self, hip, pad=0):
        out = []
        for s in self.S:
            f = hip.CoarseField(self.T.Xc, self.nvec, 8, pad)
            f.data.fill_(NAN)
            f.set_logical(s)
            if pad:
                f.data.view(2, 2 * self.nvec, f.stride)[:, :, f.volumeCB:] = NAN
            out.append(f)
        return out

    def grid_operator(self, hip, force):
        comm = _comm(hip, force)
        return hip.computeCoarseOperatorGrid(self.T, _gauge(hip, self.X, _border(force)), KAPPA, comm, clover=self.C), comm

    def solve(self, hip, opg, comm, pad=0):
        prm = dict(nConv=self.nConv, nKr=self.nKr, polyDeg=cec.POLY_DEG, tol=cec.TOL)
        start = self.start(hip, pad)
        if comm is None:
            ev, th, r, s, info = hip.coarseEigensolve(self.op, start=start, **prm)
            ginfo = None
        else:
            ev, th, r, s, info, ginfo = hip.coarseEigensolveGrid(opg, comm, start=start, **prm)
        if pad:
            pads = torch.stack([f.data.view(2, 2 * self.nvec, f.stride)[:, :, f.volumeCB:] for f in start])
            assert bool(torch.isnan(pads.real).all()) and bool(torch.isnan(pads.imag).all())
        return torch.stack([torch.view_as_real(f.data).view(torch.int64) for f in ev]).cpu(), th, r, s, info, ginfo

    def check(self, hip, force, monkeypatch, pad=0):
        """both switch settings under `force` against the single-domain solve: every bit and every count, and the branch from the grid info"""
        opg, comm = self.grid_operator(hip, force)
        want = self.ref
        assert want[4].converged
        naxes, deg = sum(force), cec.POLY_DEG
        for pack in (1, 0):
            monkeypatch.setenv(ENV, str(pack))
            got = self.solve(hip, opg, comm, pad)
            assert torch.equal(got[0], want[0]), (force, pack, "eigenvectors")
            for k, name in ((1, "theta"), (2, "residual"), (3, "sigma")):
                assert np.array_equal(got[k].view(np.int64), want[k].view(np.int64)), (force, pack, name)
            a, b = got[4], want[4]
            assert (a.iters, a.nConverged, a.opBlocks, a.hostReads, a.aMaxUsed, a.aMinLast, a.orthonormality, a.converged) == \
                   (b.iters, b.nConverged, b.opBlocks, b.hostReads, b.aMaxUsed, b.aMinLast, b.orthonormality, b.converged), (force, pack)
            g = got[5]
            F, rem = divmod(a.opBlocks - 21 - (a.iters + 1) * self.nKr // 8, deg)      # the filtered blocks of a run whose power estimate ran once
            assert rem == 0 and F > 0
            assert g.exchanges == 2 * a.opBlocks and g.rankSums == 0, (force, pack, g)
            assert g.stepPacked == ((deg - 1) * F if pack else 0), (force, pack, g, F)
            assert g.packLaunches == 2 * a.opBlocks * 2 * naxes - g.stepPacked * 2 * naxes, (force, pack, g)
        monkeypatch.delenv(ENV)


@functools.lru_cache(maxsize=None)
def _case(hip, idx):
    return _Case(hip, *FORCED[idx])


@pytest.mark.parametrize("force", FORCES)
@pytest.mark.parametrize("idx", range(len(FORCED)))
def test_forced_partitioning_is_the_single_domain_solve(hip, idx, force, monkeypatch):
    """Each axis alone, z + t and all four; MUGIQ_HIP_EIG_PACK_IN_STEP 1 and 0: eigenvectors, theta, residual, sigma, iters, opBlocks,
    hostReads, aMaxUsed and orthonormality are those of coarseEigensolve; exchanges = 2 opBlocks; (polyDeg - 1) F exchanges took their
    faces from the step kernel with the switch on, none with it off, and the pack launches are lower by 2 per partitioned axis for each."""
    _case(hip, idx).check(hip, force, monkeypatch)


def test_forced_partitioning_under_poisoned_lds(hip, monkeypatch):
    """MUGIQ_HIP_DEBUG_POISON_LDS=1: no kernel of the grid solve reads an LDS cell it has not written (the step kernel has none)"""
    c = _case(hip, 1)
    monkeypatch.setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")
    c.check(hip, (1, 1, 1, 1), monkeypatch)


def test_forced_partitioning_with_padded_start_vectors(hip, monkeypatch):
    """start vectors with a padded stride and NaN in the pads: the same bits, the pads are neither read nor written"""
    _case(hip, 2).check(hip, (1, 1, 1, 1), monkeypatch, pad=3)


# ---- coarseGramGrid ------------------------------------------------------------------------------------------------------------------------
def test_gram_grid_with_forced_partitioning_is_coarse_gram(hip):
    Xc, nvec = cec.GRAM_SHAPES[1]
    rng = np.random.default_rng(7660)
    shape = (2, int(np.prod(Xc)) // 2, 2, nvec)
    m = max(cec.GRAM_M)
    fa = [hip.CoarseField(Xc, nvec, 8, 3).set_logical(rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) for _ in range(m)]
    fb = [hip.CoarseField(Xc, nvec, 8).set_logical(rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) for _ in range(m)]
    for force in ((0, 0, 0, 0), (0, 0, 1, 1), (1, 1, 1, 1)):
        comm = _comm(hip, force)
        for mA, mB in zip(cec.GRAM_M, cec.GRAM_M[1:] + cec.GRAM_M[:1]):
            want = hip.coarseGram(fa[:mA], fb[:mB])
            got = hip.coarseGramGrid(fa[:mA], fb[:mB], comm=comm)
            assert got.shape == (mA, mB) and np.array_equal(got.view(np.int64), want.view(np.int64)), (force, mA, mB)
        own = hip.coarseGramGrid(fa[:9], comm=comm)
        assert np.array_equal(own.view(np.int64), hip.coarseGram(fa[:9]).view(np.int64))


# ---- 2 and 4 ranks -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _numpy_side(G, nvec, sizes):
    """the dense operator, its spectrum, and per (nConv, nKr) the start vectors, the restatement's counts and what the eigenpair check of
    coarse_op_ref shows on the restatement's own pairs"""
    Gc = tuple(g // 2 for g in G)
    out = {}
    for k, (nConv, nKr) in enumerate(sizes):
        Mg, D, lam, S, want = cg.global_run(G, nvec, nConv, nKr)
        assert want.status == 0
        ws = [want.evecs[:, i].reshape(cg.field_shape(Gc, nvec)) for i in range(nConv)]
        l0, r0, _ = cor.evals(Mg, ws, Gc, cor.OP_MDAGM)
        out.update({"lam": lam, "S%d" % k: S, "iters%d" % k: want.iters, "opBlocks%d" % k: want.opBlocks,
                    "cpu_l%d" % k: float(np.max(np.abs(l0 - want.theta))), "cpu_r%d" % k: float(np.max(np.abs(r0 - want.residual))),
                    "locked%d" % k: np.array(want.locked)})
    return out


@pytest.mark.parametrize("G,nvec,grid,sizes", [((4, 4, 4, 8), 4, (1, 1, 1, 2), ((8, 24),)),
                                               ((8, 4, 4, 8), 4, (2, 1, 1, 2), ((8, 24), (16, 32))),
                                               ((4, 4, 4, 16), 4, (1, 1, 1, 4), ((8, 24),)),
                                               ((16, 4, 4, 4), 5, (4, 1, 1, 1), ((8, 24),))])
def test_process_grids(G, nvec, grid, sizes, tmp_path):
    """Every rank on the one GPU through gloo, start vectors the rank's slice of a seeded global array.  Asserted in the worker: converged,
    iters and opBlocks of the restatement, theta within max(r_i, n eps lambda_max) of eigvalsh, r_i <= tol aMax, sigma = sqrt(theta),
    coarseGramGrid of the vectors, computeEvalsCoarseGrid against theta and r, the grid counts, both switch settings bit-equal, and
    coarseGramGrid against numpy within 4 eps sum |a| |b|.  Here: every rank saved identical theta, residual, counters and Gram matrix.
    The 16 / 32 run is on G 8 4 4 8 (grid 2 1 1 2), whose restatement locks 8 columns before its last round (locked 0 0 0 0 0 8 16)."""
    side = _numpy_side(G, nvec, sizes)
    if (16, 32) in sizes:
        k = sizes.index((16, 32))
        assert np.any(side["locked%d" % k][:-1] > 0), side["locked%d" % k]
    npz = str(tmp_path / "numpy_side.npz")
    np.savez(npz, **side)
    world = int(np.prod(grid))
    prefix = str(tmp_path / "eig")
    mp.spawn(coarse_eig_grid_workers.solver_worker, args=(world, free_port(), grid, G, nvec, sizes, npz, prefix), nprocs=world, join=True)
    outs = [np.load("%s_%d.npy" % (prefix, r)) for r in range(world)]
    assert len(outs) == world and np.all(np.isfinite(outs[0]))
    for o in outs[1:]:
        assert np.array_equal(o.view(np.int64), outs[0].view(np.int64))


def test_process_grid_on_pairwise_distinct_extents(tmp_path):
    """G 4 8 12 8, n_vec 5 on 1 1 1 2 (local coarse 2 4 6 2), 8 / 24: the counts of the single-domain coarseEigensolve on the global
    problem and |theta_grid - theta_single| <= r_grid + r_single + n eps aMax (asserted in the worker); identical values on both ranks."""
    prefix = str(tmp_path / "aniso")
    mp.spawn(coarse_eig_grid_workers.aniso_worker, args=(2, free_port(), (1, 1, 1, 2), (4, 8, 12, 8), 5, 8, 24, prefix), nprocs=2, join=True)
    outs = [np.load("%s_%d.npy" % (prefix, r)) for r in range(2)]
    assert np.all(np.isfinite(outs[0])) and np.array_equal(outs[1].view(np.int64), outs[0].view(np.int64))


# ---- old and new entry points --------------------------------------------------------------------------------------------------------------
def test_unpartitioned_comm_is_the_existing_solver_and_the_existing_calls_still_refuse(hip):
    c = _case(hip, 0)
    comm = _comm(hip, (0, 0, 0, 0))
    opg, _ = c.grid_operator(hip, (0, 0, 0, 0))
    assert opg.halo is None
    got, want = c.solve(hip, opg, comm), c.ref
    assert torch.equal(got[0], want[0]) and all(np.array_equal(got[k].view(np.int64), want[k].view(np.int64)) for k in (1, 2, 3))
    assert got[4][:7] == want[4][:7] and got[5] == hip.CoarseEigGridInfo(0, 0, 0, 0)
    start = c.start(hip)
    assert np.array_equal(hip.coarseGramGrid(start[:9], comm=comm).view(np.int64), hip.coarseGram(start[:9]).view(np.int64))
    part = _comm(hip, (0, 0, 0, 1))
    with pytest.raises(hip.MugiqHipError, match="status 2"):
        hip.coarseEigensolve(c.op, start=start, comm=part, nConv=c.nConv, nKr=c.nKr)
    with pytest.raises(hip.MugiqHipError, match="status 2"):
        hip.coarseGram(start[:2], comm=part)
    out = [hip.CoarseField(c.T.Xc, c.nvec, 8) for _ in range(2)]
    with pytest.raises(hip.MugiqHipError, match="status 2"):
        hip.coarseRotate(out, start[:2], np.eye(2), comm=part)
    with pytest.raises(hip.MugiqHipError, match="coarse halo is NULL"):
        hip.coarseEigensolveGrid(c.op, part, start=start, nConv=c.nConv, nKr=c.nKr)
