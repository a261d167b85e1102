"""The problems the three-level solver tests share (tests/test_mg_solve3_cpu.py, tests/test_gpu_mg_solve3.py), seeded and computed once: the
three hierarchies of tests/coarse_op2_cases.py as they are (random V on both levels, not block-orthonormal, with and without clover) and a
SMOOTH hierarchy on which the levels do what they are for:

  X = (8, 4, 4, 4), links exp(0.3 i H) as mg_solve_cases.links("smooth") makes them, kappa 0.138, no clover;
  V0 from mg_setup_ref.setup with 8 Gaussian start vectors, setupMaxIter 20, aggregates 2^4  ->  X1 = (4, 2, 2, 2), level-1 dimension 512;
  V1 = the 8 lowest eigenvectors of the dense M_1^dag M_1, block-orthonormalised on aggregates (2, 1, 1, 1)  ->  X2 = (2, 2, 2, 2).

Level-2 rows are 8 elements long on every one of them and cut every wave."""
import functools

import numpy as np

import coarse_op2_cases as c2c
import coarse_op2_ref as c2r
import mg_setup_ref as msr
import mg_solve3_ref as m3
import mg_solve_cases as mgc
import mg_solve_ref as mgr
from util import orc, rel_err

KAPPA_H = c2c.KAPPA
SMOOTH = dict(X=(8, 4, 4, 4), kappa=0.138, bs0=(2, 2, 2, 2), nv0=8, bs1=(2, 1, 1, 1), nv1=8, setupMaxIter=20)
# (params[0], params[1]) of the K^(3) comparisons: params[0] = (nuPre, nuPost, coarseIters), params[1] = (nuPre, nuPost, omega, coarseIters)
K3_PARAMS = [((0, 2, 4), (0, 2, 1.0, 4)),
             ((1, 1, 2), (1, 1, 0.85, 8)),
             ((0, 0, 4), (0, 2, 1.0, 0)),
             ((0, 2, 16), (0, 1, 1.0, 16)),
             ((0, 2, 0), (0, 2, 1.0, 4))]          # no coarse step on level 0: K with coarseIters 0, bit for bit
NRHS = 9
# the cycle of the solves: nuPost 4 and 4 flexible steps on level 0; 2 MR steps and 4 steps on M_2 on level 1
SOLVE_PARAMS = (dict(nuPost=4, coarseIters=4, nKrylov=16), dict(nuPost=2, coarseIters=4))
# outer iterations on the smooth hierarchy for right-hand side 0 at tol 1e-10, nuPost 4, nKrylov 16, as recorded on the machine that wrote
# this (another BLAS may move a count by one; tests/test_mg_solve3_cpu.py asserts the relations and prints what it finds)
SMOOTH_COUNTS3 = {"two-grid 4": 48, "exact level 1": 30, "(4, 2, 4)": 30, "(4, 0, 4)": 63}


def params(p0, p1):
    return [dict(nuPre=p0[0], nuPost=p0[1], coarseIters=p0[2]), dict(nuPre=p1[0], nuPost=p1[1], omega=p1[2], coarseIters=p1[3])]


def _c(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


@functools.lru_cache(maxsize=None)
def smooth_links():
    X = SMOOTH["X"]
    rng = np.random.default_rng(5102)
    A = _c(rng, (4, X[3], X[2], X[1], X[0], 3, 3))
    H = 0.5 * (A + np.conj(np.swapaxes(A, -1, -2)))
    H = H - np.trace(H, axis1=-2, axis2=-1)[..., None, None] * np.eye(3) / 3.0
    w, Q = np.linalg.eigh(H)
    U = np.einsum("...ij,...j,...kj->...ik", Q, np.exp(0.3j * w), np.conj(Q))
    return orc.extended_gauge_from_global(U, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))


@functools.lru_cache(maxsize=None)
def smooth():
    """dict(h: the Hierarchy, V0, V1, K1, K2, X1, X2, dense1: M_1 as a matrix, cond1: its condition number)"""
    s = SMOOTH
    X, Uo = s["X"], smooth_links()
    rng = np.random.default_rng(5103)
    vcb = int(np.prod(X)) // 2
    starts = [_c(rng, (2, vcb, 4, 3)) for _ in range(s["nv0"])]
    V0, _, _ = msr.setup(X, Uo, s["kappa"], s["bs0"], starts, setupMaxIter=s["setupMaxIter"])
    two = mgr.Problem(X, Uo, s["kappa"], V0, s["bs0"])
    X1 = two.Xc
    D1 = c2r.dense(two.Mc, X1)
    sv = np.linalg.svd(D1, compute_uv=False)
    _, vec = np.linalg.eigh(D1.conj().T @ D1)
    vcb1 = int(np.prod(X1)) // 2
    V1 = np.stack([vec[:, j].reshape(2, vcb1, 2, s["nv0"]) for j in range(s["nv1"])], axis=-1)
    V1, _, _ = msr.block_orthonormalize(V1, X1, s["bs1"], spin_bs=1)
    h = m3.Hierarchy.build(X, Uo, s["kappa"], [V0, V1], [s["bs0"], s["bs1"]], Ks=[two.Mc, c2r.build(two.Mc, V1, X1, s["bs1"])])
    return dict(h=h, two=two, V0=V0, V1=V1, K1=h.parts["Ks"][0], K2=h.parts["Ks"][1], X1=X1, X2=h.parts["Xs"][2], dense1=D1,
                cond1=float(sv[0] / sv[-1]), Uo=Uo)


@functools.lru_cache(maxsize=None)
def smooth_rhs():
    """three right-hand sides that need different iteration counts: a random one, M P_0 P_1 w and P_0 P_1 w for a random coarsest w"""
    sm = smooth()
    h, X = sm["h"], SMOOTH["X"]
    rng = np.random.default_rng(5104)
    b0 = _c(rng, (2, int(np.prod(X)) // 2, 4, 3))
    w = _c(rng, (2, int(np.prod(sm["X2"])) // 2, 2, SMOOTH["nv1"]))
    low = h.P[0](h.P[1](w))
    return b0, h.M(low), low


@functools.lru_cache(maxsize=None)
def hierarchy(i):
    """the Hierarchy of coarse_op2_cases.HIERARCHIES[i], on the matrices that file built"""
    c = c2c.hierarchy(i)
    return m3.Hierarchy.build(c["X"], c["Uo"], KAPPA_H, [c["V0"], c["V1"]], [c["bs0"], c["bs1"]], c["A_eo"], [c["K1"], c["K2"]])


@functools.lru_cache(maxsize=None)
def rhs(X, n=NRHS):
    rng = np.random.default_rng(8800 + sum(X))
    return tuple(_c(rng, (2, int(np.prod(X)) // 2, 4, 3)) for _ in range(n))


def which(name):
    """(Hierarchy, right-hand sides) of "smooth" or of a HIERARCHIES index"""
    if name == "smooth":
        return smooth()["h"], rhs(SMOOTH["X"])
    return hierarchy(name), rhs(c2c.HIERARCHIES[name][0])


@functools.lru_cache(maxsize=None)
def K3_reference(name, ip, k):
    h, bs = which(name)
    return m3.K(h, bs[k], params(*K3_PARAMS[ip]))


@functools.lru_cache(maxsize=None)
def K3_sensitivity(name, ip):
    """the restatement's own largest relative movement of K^(3)(r_0) in the max norm under three 1-ulp perturbations of r_0"""
    h, bs = which(name)
    z = K3_reference(name, ip, 0)
    return max(rel_err(m3.K(h, mgr.ulp_perturbed(bs[0], seed), params(*K3_PARAMS[ip])), z) for seed in (1, 2, 3))


@functools.lru_cache(maxsize=None)
def sloppy(name):
    return which(name)[0].sloppy()


@functools.lru_cache(maxsize=None)
def K32_model(name, ip, k):
    return m3.K32(sloppy(name), which(name)[1][k], params(*K3_PARAMS[ip]))


@functools.lru_cache(maxsize=None)
def K32_sensitivity(name, ip):
    """as mg_solve_mixed_cases.sensitivity: the model under three perturbations of r_0 by one fp32 ulp"""
    import mg_solve_mixed_ref as mxr
    z = K32_model(name, ip, 0)
    return max(rel_err(m3.K32(sloppy(name), mxr.ulp32_perturbed(which(name)[1][0], seed), params(*K3_PARAMS[ip])), z) for seed in (1, 2, 3))


def solve_with_margin3(h, bs, prm, tol=mgc.TOL, solver=None):
    """mg_solve_cases.solve_with_margin for the three-level restatement: (tol, [(x, iterations, history)])"""
    solver = solver or (lambda b, t: m3.solve(h, b, [dict(prm[0], tol=t)] + list(prm[1:])))
    for _ in range(20):
        runs = [solver(b, tol) for b in bs]
        assert all(r[3] for r in runs)
        if all(mgc._margin_ok(r[2], tol) for r in runs):
            return tol, [r[:3] for r in runs]
        tol /= 1.03
    raise AssertionError("no tolerance with a 1 % margin to every history entry")


@functools.lru_cache(maxsize=None)
def smooth_reference_solves():
    return solve_with_margin3(smooth()["h"], list(smooth_rhs()), SOLVE_PARAMS)


@functools.lru_cache(maxsize=None)
def smooth_history_sensitivity():
    """the restatement's own largest relative deviation of the history of right-hand side 0 under three 1-ulp perturbations of it"""
    tol, runs = smooth_reference_solves()
    _, it, hist = runs[0]
    worst = 0.0
    for seed in (1, 2, 3):
        _, it2, h2, ok = m3.solve(smooth()["h"], mgr.ulp_perturbed(smooth_rhs()[0], seed), [dict(SOLVE_PARAMS[0], tol=tol), SOLVE_PARAMS[1]])
        assert ok and it2 == it
        worst = max(worst, float(np.max(np.abs(h2 - hist) / hist)))
    return worst


@functools.lru_cache(maxsize=None)
def smooth_mixed_counts():
    """(tol, fp64 counts, model counts) on the smooth hierarchy, in the manner of mg_solve_mixed_cases.count_table"""
    h, hs, bs = smooth()["h"], sloppy("smooth"), list(smooth_rhs())
    tol = mgc.TOL
    for _ in range(20):
        tol, runs = solve_with_margin3(h, bs, SOLVE_PARAMS, tol)
        mixed = [m3.solve_mixed(h, hs, b, [dict(SOLVE_PARAMS[0], tol=tol), SOLVE_PARAMS[1]]) for b in bs]
        assert all(m[3] for m in mixed)
        if all(mgc._margin_ok(m[2], tol) for m in mixed):
            return tol, tuple(r[1] for r in runs), tuple(m[1] for m in mixed)
        tol /= 1.03
    raise AssertionError("no tolerance with a 1 % margin to every history entry")
