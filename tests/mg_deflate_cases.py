"""The problems the tests of the deflated coarsest solve share (tests/test_mg_deflate_cpu.py, tests/test_gpu_mg_deflate.py), computed once
and left unchanged: deflation spaces from numpy's SVD of the dense operator of level 1 or 2 of the hierarchies of
tests/mg_solve3_cases.py, the restatement's cycles and solves on them, and their own sensitivities."""
import functools

import numpy as np

import coarse_op2_ref as c2r
import mg_deflate_ref as dr
import mg_solve3_cases as c3
import mg_solve3_ref as m3
import mg_solve_cases as mgc
import mg_solve_mixed_ref as mxr
import mg_solve_ref as mgr
from util import rel_err

# the cycle of the comparisons: parameter set 1 of K3_PARAMS runs every kind of step; its two-grid form keeps params[0]
IP = 1
# the solves: two-grid on the smooth hierarchy, ONE coarse step, 32 modes
SOLVE_P0 = dict(nuPost=4, coarseIters=1, nKrylov=16)
SOLVE_NEV = 32


def hierarchy(name, level):
    """the Hierarchy whose last level is `level`: the three-level one of mg_solve3_cases.which, or (level 1) its two-grid part"""
    h = c3.which(name)[0]
    return h if level == 2 else m3.Hierarchy(h.A[:2], h.R[:1], h.P[:1], h.parts)


def cycle_params(level):
    prm = c3.params(*c3.K3_PARAMS[IP])
    return prm if level == 2 else prm[:1]


@functools.lru_cache(maxsize=None)
def _svd_rows(name, level):
    p = c3.which(name)[0].parts
    dense = c3.smooth()["dense1"] if (name, level) == ("smooth", 1) else c2r.dense(p["Ks"][level - 1], p["Xs"][level])
    return np.linalg.svd(dense)[2]


def shape(name, level):
    p = c3.which(name)[0].parts
    return (2, int(np.prod(p["Xs"][level])) // 2, 2, p["Vs"][level - 1].shape[-1])


@functools.lru_cache(maxsize=None)
def space(name, level, nEv):
    """mg_deflate_ref.space on level `level` of the hierarchy: the nEv lowest singular triplets, lowest first"""
    Vh = _svd_rows(name, level)
    N = Vh.shape[0]
    return dr.from_vectors(c3.which(name)[0].A[level], [Vh[N - 1 - n].conj().reshape(shape(name, level)) for n in range(nEv)])


@functools.lru_cache(maxsize=None)
def K_reference(name, level, nEv, k):
    return dr.K(hierarchy(name, level), space(name, level, nEv), c3.which(name)[1][k], cycle_params(level))


@functools.lru_cache(maxsize=None)
def K_sensitivity(name, level, nEv):
    """the restatement's own largest relative movement of the deflated cycle of r_0 in the max norm under three 1-ulp perturbations of r_0"""
    h, D, r = hierarchy(name, level), space(name, level, nEv), c3.which(name)[1][0]
    z = K_reference(name, level, nEv, 0)
    return max(rel_err(dr.K(h, D, mgr.ulp_perturbed(r, seed), cycle_params(level)), z) for seed in (1, 2, 3))


@functools.lru_cache(maxsize=None)
def K_undeflated_distance(name, level, nEv):
    """how far the deflated cycle of r_0 is from the undeflated one, relative in the max norm: what a call that ignored the space would miss by"""
    return rel_err(m3.K(hierarchy(name, level), c3.which(name)[1][0], cycle_params(level)), K_reference(name, level, nEv, 0))


@functools.lru_cache(maxsize=None)
def space32(name, level, nEv):
    return dr.space32(_sloppy(name, level), space(name, level, nEv))


@functools.lru_cache(maxsize=None)
def _sloppy(name, level):
    hs = c3.sloppy(name)
    return hs if level == 2 else m3.Hierarchy(hs.A[:2], hs.R[:1], hs.P[:1], hs.parts)


@functools.lru_cache(maxsize=None)
def K32_model(name, level, nEv, k):
    return dr.K32(_sloppy(name, level), space32(name, level, nEv), c3.which(name)[1][k], cycle_params(level))


@functools.lru_cache(maxsize=None)
def K32_sensitivity(name, level, nEv):
    """as mg_solve3_cases.K32_sensitivity: the model under three perturbations of r_0 by one fp32 ulp"""
    z = K32_model(name, level, nEv, 0)
    hs, D = _sloppy(name, level), space32(name, level, nEv)
    return max(rel_err(dr.K32(hs, D, mxr.ulp32_perturbed(c3.which(name)[1][0], seed), cycle_params(level)), z) for seed in (1, 2, 3))


# ---- the solves: two-grid on the smooth hierarchy ------------------------------------------------------------------------------------------
def smooth_two():
    return hierarchy("smooth", 1)


@functools.lru_cache(maxsize=None)
def reference_solves():
    """(tol, [(x, iterations, history)], undeflated iterations of right-hand side 0) for the three right-hand sides of smooth_rhs(), by the
    margin search of solve_with_margin3 -- carried on until the history of the undeflated solve of right-hand side 0 (mg_solve3_ref.solve,
    same parameters) keeps the 1 % margin to the tolerance as well, so that its count can be held against a device's too"""
    h, D, bs = smooth_two(), space("smooth", 1, SOLVE_NEV), list(c3.smooth_rhs())
    tol = mgc.TOL
    for _ in range(20):
        tol, runs = c3.solve_with_margin3(h, bs, [SOLVE_P0], tol, solver=lambda b, t: dr.solve(h, D, b, [dict(SOLVE_P0, tol=t)]))
        _, plain, hist, ok = m3.solve(h, bs[0], [dict(SOLVE_P0, tol=tol)])
        assert ok
        if mgc._margin_ok(hist, tol):
            return tol, runs, plain
        tol /= 1.03
    raise AssertionError("no tolerance with a 1 % margin to every history entry")


@functools.lru_cache(maxsize=None)
def history_sensitivity():
    """the restatement's own largest relative deviation of the history of right-hand side 0 under three 1-ulp perturbations of it"""
    tol, runs, _ = reference_solves()
    _, it, hist = runs[0]
    h, D = smooth_two(), space("smooth", 1, SOLVE_NEV)
    worst = 0.0
    for seed in (1, 2, 3):
        _, it2, h2, ok = dr.solve(h, D, mgr.ulp_perturbed(c3.smooth_rhs()[0], seed), [dict(SOLVE_P0, tol=tol)])
        assert ok and it2 == it
        worst = max(worst, float(np.max(np.abs(h2 - hist) / hist)))
    return worst


@functools.lru_cache(maxsize=None)
def mixed_counts():
    """(tol, fp64 counts, model counts) of the deflated solves, in the manner of mg_solve3_cases.smooth_mixed_counts"""
    h, hs, bs = smooth_two(), _sloppy("smooth", 1), list(c3.smooth_rhs())
    D, D32 = space("smooth", 1, SOLVE_NEV), space32("smooth", 1, SOLVE_NEV)
    tol = mgc.TOL
    for _ in range(20):
        tol, runs = c3.solve_with_margin3(h, bs, [SOLVE_P0], tol, solver=lambda b, t: dr.solve(h, D, b, [dict(SOLVE_P0, tol=t)]))
        mixed = [dr.solve_mixed(h, hs, D32, b, [dict(SOLVE_P0, tol=tol)]) for b in bs]
        assert all(m[3] for m in mixed)
        if all(mgc._margin_ok(m[2], tol) for m in mixed):
            return tol, tuple(r[1] for r in runs), tuple(m[1] for m in mixed)
        tol /= 1.03
    raise AssertionError("no tolerance with a 1 % margin to every history entry")
