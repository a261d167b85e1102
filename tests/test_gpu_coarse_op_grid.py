"""GPU tests of the explicit coarse operator on a process grid (mugiq_hip_compute_coarse_operator_grid, mugiq_hip_coarse_apply_grid,
mugiq_hip_compute_evals_coarse_operator_grid).  On one rank with the partitioned path forced -- ghost faces, halo matrices and messages
with the rank as its own neighbour -- everything must be the BITS of the unpartitioned existing calls on the same fields: the sums and
their order are the same, only where an operand is read from changes -- on lattices with y = z and on two with x, y, z pairwise distinct
(coarse_op_cases.ANISO), where a face index with an extent from the wrong axis shows, and in all three forms of the ghost apply kernel
(16, 32 and 64 outputs per workgroup).  On 2 and 4 ranks (tests/coarse_op_grid_workers.py; four along x, y and t, each with four distinct
neighbours) a rank's matrices and outputs must be the bits of its slice of the single-domain ones.  The decomposition itself is pinned on the CPU
(tests/test_coarse_op_grid_cpu.py).  The eigenpair check: 1e-13 against the unpartitioned call (the bound tests/restrict_workers.py uses
for the same comparison), 1e-12 against numpy (the bound of this chain)."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import clover_ref as cr
import coarse_op_cases as cases
import coarse_op_grid_workers
from test_multi_rank_cpu import free_port
from util import orc, random_gauge_lex

pytestmark = pytest.mark.gpu

KAPPA = cases.KAPPA
COUNTS = (1, 8, 9, 17)
SCALE = 1.7
# each axis alone (gauge border 2), z + t (borders of 1 on two axes), all four
FORCES = [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (0, 0, 1, 1), (1, 1, 1, 1)]
SHAPES = [cases.SHAPES[0],      # every coarse extent 2: both ghosts of a site come from the same neighbour site, Y+ and Y- differ
          cases.SHAPES[2],      # coarse extent 4 along x: faces differ from the interior; n_vec no multiple of 4
          cases.SHAPES[4],      # sites with both x neighbours inside the aggregate
          cases.SHAPES[5],      # N = 48
          cases.LARGE_NVEC[0],  # a second, ragged chunk in both kernels
          cases.ANISO[0],       # coarse 2 4 6 2: x, y, z pairwise distinct and a 6, so every face index has two different multipliers
          cases.ANISO[1]]       # coarse 6 2 4 2: the 6 on the checkerboard axis, the face of x with y != z
FORM_ENV = "MUGIQ_HIP_COARSE_APPLY_OUT"


def _bits(t):
    return t.view(torch.float64 if t.dtype == torch.complex128 else torch.float32).view(torch.int64 if t.dtype == torch.complex128 else torch.int32)


def _same(a, b):
    return bool(torch.equal(_bits(a), _bits(b)))


def _border(force):
    return tuple((2 if sum(force) % 2 else 1) * f for f in force)


@functools.lru_cache(maxsize=None)
def _links(X):
    rng = np.random.default_rng(4400 + sum(X))
    U_lex = random_gauge_lex(rng, X)
    return U_lex, cr.clover_blocks_eo(U_lex, cases.CSW_COEFF, X)


def _gauge(hip, X, brd, prec=8):
    return hip.GaugeField(X, brd, prec).set_logical(orc.extended_gauge_from_global(_links(X)[0], (0, 0, 0, 0), (1, 1, 1, 1), brd))


def _comm(hip, force):
    return hip.GridComm((1, 1, 1, 1), device="cuda:0", force_partitioned=force)


class _Problem:
    """the fields of one shape and the results of the EXISTING unpartitioned calls on them"""

    def __init__(self, hip, X, bs, nvec, clover, prec=8, gprec=8, pad=0):
        self.X, self.nvec, self.prec, self.gprec = X, nvec, prec, gprec
        V, ws = cases.null_vectors(X, bs, nvec)
        self.C = hip.CloverField(X, gprec).set_logical(_links(X)[1]) if clover else None
        self.T = hip.Transfer(X, nvec, bs, 2, prec).set_logical(V)
        self.op = hip.computeCoarseOperator(self.T, _gauge(hip, X, (0, 0, 0, 0), gprec), KAPPA, clover=self.C)
        self.cw = [hip.CoarseField(self.T.Xc, nvec, prec, pad=pad).set_logical(w) for w in ws]
        if pad:
            for f in self.cw:
                f.data.view(2, 2 * nvec, f.stride)[:, :, f.volumeCB:] = complex(float("nan"), float("nan"))
        self.pad = pad
        self.ref = {}
        for opType in range(5):
            for n in COUNTS:
                out = self.outputs(hip, n)
                hip.coarseApply(out, self.cw[:n], self.op, opType, SCALE)
                self.ref[opType, n] = out
        self.evals = [hip.computeEvalsCoarse(self.cw, opType=o, coarseOp=self.op) for o in range(5)]

    def outputs(self, hip, n):
        out = [hip.CoarseField(self.T.Xc, self.nvec, self.prec, pad=self.pad and self.pad - 2) for _ in range(n)]
        if self.pad:
            for o in out:
                o.data.fill_(complex(float("nan"), float("nan")))
        return out

    def check(self, hip, force):
        """the grid entry points under the forced partition `force` against the stored results"""
        comm = _comm(hip, force)
        opg = hip.computeCoarseOperatorGrid(self.T, _gauge(hip, self.X, _border(force), self.gprec), KAPPA, comm, clover=self.C)
        assert opg.kappa == KAPPA and opg.hasClover == (self.C is not None) and opg.halo.dims == force
        assert _same(opg.data, self.op.data), ("matrices", force)
        for opType in range(5):
            for n in COUNTS:
                out = self.outputs(hip, n)
                hip.coarseApplyGrid(out, self.cw[:n], opg, comm, opType, SCALE)
                for k in range(n):
                    if self.pad:
                        assert np.array_equal(out[k].get_logical(), self.ref[opType, n][k].get_logical()), (force, opType, n, k)
                        pads = out[k].data.view(2, 2 * self.nvec, out[k].stride)[:, :, out[k].volumeCB:]
                        assert bool(torch.isnan(pads.real).all()) and bool(torch.isnan(pads.imag).all()), (force, opType, n, k)
                    else:
                        assert _same(out[k].data, self.ref[opType, n][k].data), (force, opType, n, k)
            got = hip.computeEvalsCoarseGrid(self.cw, opg, comm, opType)
            for a, b in zip(got, self.evals[opType]):
                assert (a is None) == (b is None)
                if a is not None:
                    e = np.max(np.abs(a - b)) / np.max(np.abs(b))
                    assert e < 1e-13, (force, opType, e)
        return opg


# ---- 1. forced partitioning on one rank ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clover", [False, True])
@pytest.mark.parametrize("X,bs,nvec", SHAPES)
def test_forced_partitioning_reproduces_the_single_domain_bits(hip, X, bs, nvec, clover):
    """Every axis alone, z + t and all four: all nine matrices of every site, the five forms with 1, 8, 9 and 17 vectors and scale 1.7 --
    bit-equal to the unpartitioned existing calls; the eigenpair check to 1e-13."""
    p = _Problem(hip, X, bs, nvec, clover)
    for force in FORCES:
        p.check(hip, force)


def _halo_is_the_own_faces(hip, X, bs, nvec):
    import coarse_op_grid_ref as gr
    p = _Problem(hip, X, bs, nvec, True)
    opg = p.check(hip, (1, 1, 1, 1))
    M, Xc = p.op.get_logical(), p.T.Xc
    for mu in range(4):
        assert np.array_equal(opg.halo.get_logical(mu, False), gr.face(M[:, :, 1 + 2 * mu], Xc, mu, 1)), mu
        assert np.array_equal(opg.halo.get_logical(mu, True), gr.face(M[:, :, 2 + 2 * mu], Xc, mu, 0)), mu


def test_halo_holds_the_neighbours_matrices(hip):
    """A rank that is its own neighbour: Yback[mu] is Y+_mu of its own high face and Yfwd[mu] Y-_mu of its own low face, in the header's
    face order (tests/coarse_op_grid_ref.face)."""
    _halo_is_the_own_faces(hip, *cases.SHAPES[2])


def test_halo_on_pairwise_distinct_extents(hip):
    """the same on coarse 2 4 6 2: the matrix pack walks faces whose three extents all differ"""
    _halo_is_the_own_faces(hip, *cases.ANISO[0])


@pytest.mark.parametrize("prec,gprec", [(4, 4), (8, 4)])
def test_forced_partitioning_in_fp32(hip, prec, gprec):
    """fp32 transfer, operator and vectors; fp32 links and clover field under an fp64 transfer"""
    X, bs, nvec = cases.SHAPES[2]
    p = _Problem(hip, X, bs, nvec, True, prec=prec, gprec=gprec)
    for force in ((1, 0, 0, 0), (0, 0, 1, 1), (1, 1, 1, 1)):
        p.check(hip, force)


@pytest.mark.parametrize("prec,gprec", [(4, 4), (8, 4)])
def test_forced_partitioning_in_fp32_on_pairwise_distinct_extents(hip, prec, gprec):
    """the same on coarse 2 4 6 2"""
    X, bs, nvec = cases.ANISO[0]
    p = _Problem(hip, X, bs, nvec, True, prec=prec, gprec=gprec)
    for force in ((1, 0, 0, 0), (0, 0, 1, 1), (1, 1, 1, 1)):
        p.check(hip, force)


def test_forced_partitioning_with_padded_vectors(hip):
    """source and destination vectors with padded strides (7 and 5) and NaN in the pads: the same values, the pads stay NaN"""
    X, bs, nvec = cases.SHAPES[2]
    p = _Problem(hip, X, bs, nvec, True, pad=7)
    for force in ((1, 0, 0, 0), (1, 1, 1, 1)):
        p.check(hip, force)


def test_forced_partitioning_with_padded_vectors_on_pairwise_distinct_extents(hip):
    """the same on coarse 2 4 6 2: a face index taken with the wrong stride or extent lands in a pad or on another site"""
    X, bs, nvec = cases.ANISO[0]
    p = _Problem(hip, X, bs, nvec, True, pad=7)
    for force in ((1, 0, 0, 0), (1, 1, 1, 1)):
        p.check(hip, force)


def test_forced_partitioning_under_poisoned_lds(hip, monkeypatch):
    """MUGIQ_HIP_DEBUG_POISON_LDS=1: no kernel of the grid path reads an LDS cell it has not written"""
    X, bs, nvec = cases.SHAPES[2]
    p = _Problem(hip, X, bs, nvec, True)
    monkeypatch.setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")
    p.check(hip, (1, 1, 1, 1))


# ---- 1b. every form of the ghost kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("X,bs,nvec", [cases.SHAPES[2],        # N = 10: one chunk, most lanes masked
                                       cases.LARGE_NVEC[0],    # N = 66: two ragged chunks of 64 outputs, three of 32, five of 16
                                       cases.ANISO[0]])        # faces with pairwise distinct extents
def test_every_form_of_the_ghost_apply_kernel(hip, X, bs, nvec, prec, monkeypatch):
    """coarse_apply_kernel<.., GHOST = true> with 16, 32 and 64 outputs per workgroup (MUGIQ_HIP_COARSE_APPLY_OUT; the rule alone picks 32
    on lattices this small), fp64 and fp32 storage, all four axes forced and x alone: the five forms with 1, 9 and 17 vectors and scale 1.7
    are the bits of coarseApply on the same fields with the variable unset -- the unpartitioned call under the default rule, not the grid
    call itself.  M and G5 M launch the M kernel, M^dag its own, the normal forms both."""
    monkeypatch.delenv(FORM_ENV, raising=False)
    p = _Problem(hip, X, bs, nvec, True, prec=prec, gprec=prec)
    assert all(hip.coarseApplyForm(p.op, n) == 32 for n in (1, 9, 17))
    for force in ((1, 1, 1, 1), (1, 0, 0, 0)):
        comm = _comm(hip, force)
        opg = hip.computeCoarseOperatorGrid(p.T, _gauge(hip, X, _border(force), prec), KAPPA, comm, clover=p.C)
        assert opg.halo.dims == force and _same(opg.data, p.op.data), force
        for form in (16, 32, 64):
            monkeypatch.setenv(FORM_ENV, str(form))
            assert hip.coarseApplyForm(opg, 17) == form
            for opType in range(5):
                for n in (1, 9, 17):
                    out = p.outputs(hip, n)
                    hip.coarseApplyGrid(out, p.cw[:n], opg, comm, opType, SCALE)
                    for k in range(n):
                        assert _same(out[k].data, p.ref[opType, n][k].data), (force, form, opType, n, k)
            monkeypatch.delenv(FORM_ENV)


def test_the_rule_selects_the_64_output_form_on_the_ghost_path(hip, monkeypatch):
    """No variable set: 41 vectors on the 96 coarse sites of the first ANISO shape are 96 x 6 blocks of vectors = 576 >= 512 workgroups of
    the 64-output grid, so the rule itself takes the 64-output form (17 vectors: 288, the 32-output form).  M, M^dag and G5 M under
    1 1 1 1 are the bits of coarseApply.  The normal forms are not in this test: they launch 8 vectors at a time, 96 workgroups, and stay on
    the 32-output form; test_every_form_of_the_ghost_apply_kernel forces them through the others."""
    monkeypatch.delenv(FORM_ENV, raising=False)
    X, bs, nvec = cases.ANISO[0]
    p = _Problem(hip, X, bs, nvec, True)
    assert hip.coarseApplyForm(p.op, 41) == 64 and hip.coarseApplyForm(p.op, 17) == 32
    rng = np.random.default_rng(4100)                     # cases.NW stays 17: the other 24 vectors are this test's own
    cw = p.cw + [hip.CoarseField(p.T.Xc, nvec, 8).set_logical(cases.c(rng, (2, p.op.volumeCB, 2, nvec))) for _ in range(41 - cases.NW)]
    force = (1, 1, 1, 1)
    comm = _comm(hip, force)
    opg = hip.computeCoarseOperatorGrid(p.T, _gauge(hip, X, _border(force)), KAPPA, comm, clover=p.C)
    assert opg.halo.dims == force and len(cw) == 41 and hip.coarseApplyForm(opg, len(cw)) == 64
    for opType in (hip.MUGIQ_EIG_OPERATOR_M, hip.MUGIQ_EIG_OPERATOR_Mdag, hip.MUGIQ_EIG_OPERATOR_H):
        want, got = p.outputs(hip, 41), p.outputs(hip, 41)
        hip.coarseApply(want, cw, p.op, opType, SCALE)
        hip.coarseApplyGrid(got, cw, opg, comm, opType, SCALE)
        for k in range(41):
            assert _same(got[k].data, want[k].data), (opType, k)
        assert not _same(want[0].data, want[40].data)


# ---- 2. two and four ranks -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,nvec,grid", [((4, 4, 4, 8), 4, (1, 1, 1, 2)),
                                         ((8, 4, 4, 8), 4, (2, 1, 1, 2)),
                                         ((4, 4, 4, 16), 4, (1, 1, 1, 4)),     # four distinct neighbours along t: a swapped direction shows
                                         ((16, 4, 4, 4), 5, (2, 1, 1, 1)),     # local coarse extent 4 along the partitioned axis
                                         # ranks are ordered x slowest, t fastest: four distinct neighbours along x (rank +- 1 is no x
                                         # neighbour) and along y; real messages with faces of pairwise distinct extents (coarse 2 4 6 2)
                                         ((16, 4, 4, 4), 4, (4, 1, 1, 1)),
                                         ((4, 16, 4, 4), 4, (1, 4, 1, 1)),
                                         ((4, 8, 12, 8), 5, (1, 1, 1, 2))])
def test_process_grids(G, nvec, grid, tmp_path):
    """Every rank on the one GPU through gloo: local matrices and outputs are the bits of the rank's slice of the single-domain ones and
    equal numpy to 1e-12, the eigenpair values equal numpy to 1e-12 (asserted in the worker) and are identical on all ranks."""
    world = int(np.prod(grid))
    prefix = str(tmp_path / "grid")
    mp.spawn(coarse_op_grid_workers.grid_worker, args=(world, free_port(), grid, G, (2, 2, 2, 2), nvec, prefix), nprocs=world, join=True)
    outs = [np.load("%s_%d.npy" % (prefix, r)) for r in range(world)]
    assert len(outs) == world and np.all(np.isfinite(outs[0]))
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])


def test_process_grid_in_fp32(tmp_path):
    """Four ranks along x with every field in fp32 storage: local matrices and outputs are the bits of the rank's slice of the
    single-domain device results in the same storage, and all ranks save identical eigenpair values.  Nothing is compared with numpy: the
    project has no fp32 bound for this chain."""
    G, nvec, grid = (16, 4, 4, 4), 4, (4, 1, 1, 1)
    prefix = str(tmp_path / "grid")
    mp.spawn(coarse_op_grid_workers.grid_worker, args=(4, free_port(), grid, G, (2, 2, 2, 2), nvec, prefix, 4), nprocs=4, join=True)
    outs = [np.load("%s_%d.npy" % (prefix, r)) for r in range(4)]
    assert np.all(np.isfinite(outs[0]))
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])


# ---- 3. old and new entry points -------------------------------------------------------------------------------------------------------
def test_unpartitioned_comm_is_the_existing_call_and_the_existing_calls_still_refuse(hip):
    X, bs, nvec = cases.SHAPES[2]
    p = _Problem(hip, X, bs, nvec, True)
    comm = _comm(hip, (0, 0, 0, 0))
    opg = hip.computeCoarseOperatorGrid(p.T, _gauge(hip, X, (0, 0, 0, 0)), KAPPA, comm, clover=p.C)
    assert opg.halo is None and _same(opg.data, p.op.data)
    for opType in range(5):
        out = p.outputs(hip, 17)
        hip.coarseApplyGrid(out, p.cw, opg, comm, opType, SCALE)
        assert all(_same(a.data, b.data) for a, b in zip(out, p.ref[opType, 17])), opType
        got = hip.computeEvalsCoarseGrid(p.cw, opg, comm, opType)
        assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(got, p.evals[opType])), opType
    part = _comm(hip, (0, 0, 0, 1))
    out = p.outputs(hip, 1)
    with pytest.raises(hip.MugiqHipError, match="status 2"):
        hip.computeCoarseOperator(p.T, _gauge(hip, X, (0, 0, 0, 2)), KAPPA, clover=p.C, comm=part)
    with pytest.raises(hip.MugiqHipError, match="status 2"):
        hip.coarseApply(out, p.cw[:1], p.op, comm=part)
    with pytest.raises(hip.MugiqHipError, match="status 2"):
        hip.computeEvalsCoarse(p.cw, coarseOp=p.op, comm=part)
    # and the grid calls refuse what they cannot serve: no halo on a partitioned comm, a gauge field without a border
    with pytest.raises(hip.MugiqHipError, match="coarse halo is NULL"):
        hip.coarseApplyGrid(out, p.cw[:1], p.op, part)
    with pytest.raises(hip.MugiqHipError, match="no border"):
        hip.computeCoarseOperatorGrid(p.T, _gauge(hip, X, (0, 0, 0, 0)), KAPPA, part, clover=p.C)


def test_halo_allocation_of_the_c_abi(hip):
    """mugiq_hip_alloc_coarse_halo / mugiq_hip_free_coarse_halo: buffers on the asked axes only, described like the operator"""
    lib = hip._lib.load()
    op = hip.CoarseOperator((4, 2, 2, 2), 5, 4)
    d, h = op.desc(), hip._lib.CoarseHaloDesc()
    assert lib.mugiq_hip_alloc_coarse_halo(ctypes.byref(h), ctypes.byref(d), hip._lib.int4((1, 0, 0, 1))) == 0
    assert [bool(h.Yback[i]) for i in range(4)] == [bool(h.Yfwd[i]) for i in range(4)] == [True, False, False, True]
    assert (h.precision, h.nVec, h.volumeCB, tuple(h.X), tuple(h.dims)) == (4, 5, 16, (4, 2, 2, 2), (1, 0, 0, 1))
    assert lib.mugiq_hip_free_coarse_halo(ctypes.byref(h)) == 0 and not any(h.Yback[i] or h.Yfwd[i] for i in range(4))
