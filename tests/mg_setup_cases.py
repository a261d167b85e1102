"""The inputs, bounds and pinned numbers the MG-setup tests share (tests/test_mg_setup_cpu.py, tests/test_gpu_mg_setup.py,
tests/test_gpu_mg_setup_scale.py), seeded and computed once: blocks for the orthonormalisation, the start vectors of the setup driver on
the two 4^4 fields of tests/mg_solve_cases.py and on its RAGGED shape with the clover blocks of tests/coarse_op_cases.py, and the runs of
the numpy restatement (tests/mg_setup_ref.py) that these files compare against.

Bounds.  What the device is held to is 100 x what the restatement itself shows against numpy.linalg.qr (diagonal made positive) on the
same input, shape by shape: RESTATEMENT[name] = (its max |B^dag B - 1|, its max distance to that Q).  Both are written down here as
measured by test_mg_setup_cpu.py (which asserts name by name that they still hold, and records them); the factor 100 covers the kernel's
other summation order.  Nothing here was fitted to the kernel.  fp32 storage: the same two numbers of the restatement's result rounded to
complex64, computed in the run (they are eps_32-sized: 6e-8 rounding of entries of size <= 1, summed over m rows)."""
import functools

import numpy as np

import coarse_op_cases as coc
import mg_setup_ref as msr
import mg_solve_cases as mgc
import mg_solve_ref as mgr

# name -> (X, aggregate, n_vec)
ORTHO_SHAPES = {
    "4^4 n1": ((4, 4, 4, 4), (2, 2, 2, 2), 1),
    "4^4 n5": ((4, 4, 4, 4), (2, 2, 2, 2), 5),
    "4^4 n24": ((4, 4, 4, 4), (2, 2, 2, 2), 24),       # two reduction rounds per column beyond 16
    "4^4 n32": ((4, 4, 4, 4), (2, 2, 2, 2), 32),
    "ragged": ((6, 6, 6, 4), (3, 3, 3, 2), 7),          # m = 324: 5.06 waves, odd aggregate extents (the parity of an aggregate's origin varies)
    "production": ((8, 8, 8, 8), (4, 4, 4, 4), 24),     # m = 1536, n_vec 24: the production block
    "many": ((16, 16, 16, 16), (2, 2, 2, 2), 8),        # 8192 blocks
}
# beyond two reduction rounds and 36 KB of dynamic LDS (tests/test_gpu_mg_setup_scale.py).  A block of m rows takes 24 m bytes (the fp64
# column and the row table); the kernel takes finished columns 16 to a round.  The three lds* shapes have the coarse lattice 2^4: 32 blocks
SCALE_SHAPES = {
    "n33": ((4, 4, 4, 4), (2, 2, 2, 2), 33),            # a third round with a single column
    "n64": ((4, 4, 4, 4), (2, 2, 2, 2), 64),            # four rounds, the largest n_vec of a finest-level transfer
    "lds55k": ((12, 8, 8, 8), (6, 4, 4, 4), 4),         # m = 2304, 55 296 B: between 48 and 64 KB; 9 rows per lane
    "lds72k": ((16, 8, 8, 8), (8, 4, 4, 4), 4),         # m = 3072, 73 728 B: the first launch that has to raise the kernel's LDS limit
    "lds144k": ((16, 16, 8, 8), (8, 8, 4, 4), 2),       # m = 6144, 147 456 B: the largest power-of-two block admitted; 24 rows per lane
}
FINEST_SHAPES = dict(ORTHO_SHAPES, **SCALE_SHAPES)
# the coarse -> coarse layout (spin_block_size 1, fine_spin 2): name -> (finer lattice, aggregate, nColor of the finer side, n_vec)
COARSE_SHAPES = {
    "coarse": ((4, 4, 4, 4), (2, 2, 2, 2), 5, 6),       # m = 5 x 16 = 80
    "coarse96": ((4, 4, 4, 4), (2, 2, 2, 2), 24, 96),   # m = 384 (1.5 rows per lane), six rounds: every coefficient slot of the kernel
    "coarse7": ((4, 4, 4, 12), (2, 2, 2, 3), 7, 20),    # m = 168: odd nColor, an odd aggregate extent, two rounds, partial waves
}
# name -> (max |B^dag B - 1|, max distance to the Q of numpy's QR) of the restatement with nPasses = 2 on that shape's input, as
# test_mg_setup_cpu.py::test_restatement_against_qr prints them, rounded up in the second digit.  That test re-asserts them name by name;
# the device is held to FACTOR x the pair of the shape it runs
RESTATEMENT = {
    "4^4 n1": (6.7e-16, 1.6e-16),
    "4^4 n5": (8.9e-16, 2.3e-16),
    "4^4 n24": (8.9e-16, 4.2e-16),
    "4^4 n32": (1.2e-15, 3.7e-16),
    "ragged": (1.4e-15, 1.9e-16),
    "production": (3.4e-15, 2.2e-16),
    "many": (1.4e-15, 4.0e-16),
    "coarse": (1.2e-15, 2.3e-16),
    # SCALE_SHAPES and the two further COARSE_SHAPES (test_restatement_against_qr and its coarse-layout twin)
    "n33": (8.9e-16, 4.5e-16),
    "n64": (1.2e-15, 5.6e-16),
    "lds55k": (3.2e-15, 2.0e-16),
    "lds72k": (3.6e-15, 1.9e-16),
    "lds144k": (3.7e-15, 1.7e-16),
    "coarse96": (1.8e-15, 3.5e-16),
    "coarse7": (1.2e-15, 3.4e-16),
}
COARSE_SHAPE = COARSE_SHAPES["coarse"]             # the one of tests/test_gpu_mg_setup.py
# the near-dependent input (a_1 = a_0 + 1e-6 noise, the other columns random): two passes, and the orthonormality one pass is left with
NEAR_RESTATEMENT_ORTH = 8.9e-16
NEAR_RESTATEMENT_DIST = 7.2e-10        # the problem is ill-conditioned: Q moves by eps / minPivotRatio whoever computes it
# One pass leaves <q_0, q_1> at the rounding of b_1 divided by its pivot: eps / minPivotRatio = 1.1e-16 / 8.8e-7 = 1.3e-10 (the restatement
# shows 6.0e-10).  A tenth of that estimate is what "measurably not orthonormal" means below; it is 100 x above the two-pass bound
NEAR_ONE_PASS_ORTH_AT_LEAST = 1e-11
FACTOR = 100.0


def _c(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


@functools.lru_cache(maxsize=None)
def random_V(name, ns=4, nc=3):
    X, bs, nvec = FINEST_SHAPES[name]
    return _c(np.random.default_rng(6100 + len(name) + nvec), (2, int(np.prod(X)) // 2, ns, nc, nvec))


@functools.lru_cache(maxsize=None)
def near_dependent_V(name="4^4 n5"):
    V = random_V(name).copy()
    V[..., 1] = V[..., 0] + 1e-6 * _c(np.random.default_rng(6200), V[..., 0].shape)
    return V


@functools.lru_cache(maxsize=None)
def reference(name, nPasses=2, near=False, precision=8):
    """(V', minPivotRatio, zeroColumns) of the restatement on the input as the device stores it"""
    X, bs, _ = FINEST_SHAPES[name]
    V = near_dependent_V(name) if near else random_V(name)
    if precision == 4:
        V = V.astype(np.complex64).astype(np.complex128)
    return msr.block_orthonormalize(V, X, bs, 2, nPasses)


@functools.lru_cache(maxsize=None)
def coarse_V(name="coarse"):
    X, bs, nc, nvec = COARSE_SHAPES[name]
    return _c(np.random.default_rng(6300 if name == "coarse" else 6300 + nvec), (2, int(np.prod(X)) // 2, 2, nc, nvec))


@functools.lru_cache(maxsize=None)
def coarse_reference(name="coarse", precision=8):
    """(V', minPivotRatio, zeroColumns) of the restatement on the coarse -> coarse input as the device stores it, and the Q of numpy's QR
    on it"""
    X, bs, _, _ = COARSE_SHAPES[name]
    V = coarse_V(name)
    if precision == 4:
        V = V.astype(np.complex64).astype(np.complex128)
    qr = msr.from_blocks(msr.qr_positive(msr.to_blocks(V, X, bs, 1)), X, bs, V.shape, 1)
    return msr.block_orthonormalize(V, X, bs, 1, 2) + (qr,)


def bounds(name):
    """(orthonormality, distance) the device is held to on the shape `name`"""
    return FACTOR * RESTATEMENT[name][0], FACTOR * RESTATEMENT[name][1]


def qr_reference(name, near=False):
    X, bs, _ = FINEST_SHAPES[name]
    V = near_dependent_V(name) if near else random_V(name)
    return msr.from_blocks(msr.qr_positive(msr.to_blocks(V, X, bs)), X, bs, V.shape)


# ---- the setup driver on the 4^4 fields ------------------------------------------------------------------------------------------------
# setupMaxIter 10: the smallest round number at which the restatement's solve on the smooth field lands strictly below the 90 iterations of
# random null vectors (mg_solve_cases.SMOOTH_COUNTS): 65, and 34 after one refinement cycle (30 iterations: about 30).  Every CG stops at the
# iteration limit, far from setupTol, so that no count hangs on a comparison with the tolerance
SETUP = dict(setupMaxIter=10, setupTol=5e-6, nBlockOrtho=2, refineIters=4)
# outer iterations of mg_solve_ref.solve for right-hand side 0 at the margin-nudged default tolerance (reference_count), with the V of the
# restatement's setup: (field, refineCycles) -> count (test_mg_setup_cpu.py::test_setup_counts re-derives and asserts them)
SETUP_COUNTS = {("smooth", 0): 65, ("smooth", 1): 34, ("hot", 0): 9, ("hot", 1): 9}


@functools.lru_cache(maxsize=None)
def starts(field):
    rng = np.random.default_rng(5100 + len(field))
    return tuple(_c(rng, (2, int(np.prod(mgc.X4)) // 2, 4, 3)) for _ in range(mgc.NVEC))


def _setup(field, refineCycles, st):
    return msr.setup(mgc.X4, mgc.links(field)[1], mgc.KAPPA[field], mgc.BS, st, refineCycles=refineCycles, **SETUP)


@functools.lru_cache(maxsize=None)
def reference_setup(field, refineCycles=0):
    """(V, CG iterations, minPivotRatio) of the restatement's pipeline"""
    return _setup(field, refineCycles, starts(field))


@functools.lru_cache(maxsize=None)
def setup_sensitivity(field, refineCycles=0):
    """the restatement's own largest deviation of V (relative to max |V|) under 1-ulp perturbations of the start vectors: two of them,
    one where a refinement cycle makes a run take seconds"""
    V = reference_setup(field, refineCycles)[0]
    worst = 0.0
    for seed in (1, 2) if refineCycles == 0 else (1,):
        V2 = _setup(field, refineCycles, [mgr.ulp_perturbed(s, 10 * seed + j) for j, s in enumerate(starts(field))])[0]
        worst = max(worst, float(np.max(np.abs(V2 - V)) / np.max(np.abs(V))))
    return worst


@functools.lru_cache(maxsize=None)
def reference_problem(field, refineCycles=0):
    return mgr.Problem(mgc.X4, mgc.links(field)[1], mgc.KAPPA[field], reference_setup(field, refineCycles)[0], mgc.BS)


@functools.lru_cache(maxsize=None)
def reference_count(field, refineCycles=0):
    """(tol, iterations) of the restatement's solve of right-hand side 0 with the setup-made V, tol nudged from the default as in
    mg_solve_cases.solve_with_margin so that a last-bit difference cannot move the count"""
    tol, runs = mgc.solve_with_margin(reference_problem(field, refineCycles), [mgc.rhs(field)[0]])
    return tol, runs[0][1]


# ---- the setup driver with a clover term, off 4^4 (tests/test_gpu_mg_setup_scale.py) ----------------------------------------------------
# mg_solve_cases.RAGGED: X (6, 6, 6, 4), aggregates (3, 3, 3, 2), n_vec 4, on the links and clover blocks of coarse_op_cases at its kappa,
# with the parameters SETUP.  (clover, refineCycles) -> minPivotRatio of the restatement's run; every CG of every run stops at its 10
# iterations.  test_mg_setup_cpu.py::test_clover_setup_pins re-derives both, the device is held to both
RAGGED_PIVOTS = {(False, 0): 0.9234190127, (False, 1): 0.6719268876, (True, 0): 0.8727221042, (True, 1): 0.6584966763}
# the second trip of field_sub_kernel (4096 workgroups of 256 lanes: beyond 1 048 576 complex elements per vector): 1 179 648
SUB_SHAPE = ((16, 16, 16, 24), (4, 4, 4, 4), 2)


@functools.lru_cache(maxsize=None)
def ragged_starts():
    rng = np.random.default_rng(5200)
    return tuple(_c(rng, (2, int(np.prod(mgc.RAGGED[0])) // 2, 4, 3)) for _ in range(mgc.RAGGED[2]))


def ragged_setup(clover, refineCycles, st, A_eo=None):
    """the restatement's pipeline at RAGGED from the start vectors st; A_eo: in place of the clover blocks of coarse_op_cases"""
    X, bs, _ = mgc.RAGGED
    Uo, blocks = coc.links(X)
    if clover and A_eo is None:
        A_eo = coc.dense12(blocks)
    return msr.setup(X, Uo, coc.KAPPA, bs, st, refineCycles=refineCycles, A_eo=A_eo, **SETUP)


@functools.lru_cache(maxsize=None)
def ragged_reference_setup(clover, refineCycles=0):
    """(V, CG iterations, minPivotRatio)"""
    return ragged_setup(clover, refineCycles, ragged_starts())


@functools.lru_cache(maxsize=None)
def ragged_setup_sensitivity(clover, refineCycles=0):
    """as setup_sensitivity: the largest deviation of V (relative to max |V|) under 1-ulp perturbations of the start vectors"""
    V = ragged_reference_setup(clover, refineCycles)[0]
    worst = 0.0
    for seed in (1, 2) if refineCycles == 0 else (1,):
        V2 = ragged_setup(clover, refineCycles, [mgr.ulp_perturbed(s, 10 * seed + j) for j, s in enumerate(ragged_starts())])[0]
        worst = max(worst, float(np.max(np.abs(V2 - V)) / np.max(np.abs(V))))
    return worst
