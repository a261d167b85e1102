"""What the mixed-precision solver tests share (tests/test_mg_solve_mixed_cpu.py, tests/test_gpu_mg_solve_mixed.py), computed once from the
numpy model tests/mg_solve_mixed_ref.py and the fp64 restatement tests/mg_solve_ref.py -- never from the device: the sloppy problems, the
model's sensitivity to 1-ulp (fp32) perturbations of r, which sets the bound of the device's K against the model, and the table of
iteration counts, model against fp64 restatement, which sets the allowance of the device's mixed solve over its own fp64 solve."""
import functools

import numpy as np

import coarse_op_cases as coc
import mg_solve_cases as mgc
import mg_solve_mixed_ref as mxr
import mg_solve_ref as mgr
from util import rel_err

ALL_PARAMS = mgc.K_PARAMS + mgc.EDGE_PARAMS
K_MARGIN = 10.0          # device K against the model: this many times the model's own sensitivity (the stencil's fp32 arithmetic is not in it)
# the solves of the table: the four of mg_solve_cases.SOLVES on the 4^4 fields and the default parameters at the RAGGED shape
SOLVE_CASES = [("4^4",) + s for s in mgc.SOLVES] + [("ragged", "su3", 16, 4)]


def key(prm):
    return tuple(sorted(prm.items()))


def chain(shape):
    """the restatement's coarse operator: explicit matrices where they take under a second to build, the chain R M P elsewhere"""
    return shape not in (mgc.RAGGED, coc.SHAPES[0], coc.SHAPES[1])


@functools.lru_cache(maxsize=None)
def sloppy_shape_problem(shape, clover=False):
    return mxr.SloppyProblem(mgc.shape_problem(*shape, clover=clover, chain=chain(shape)))


@functools.lru_cache(maxsize=None)
def sloppy_problem(field):
    return mxr.SloppyProblem(mgc.problem(field))


@functools.lru_cache(maxsize=None)
def K_model(shape, clover, k, prm):
    """the model's K of right-hand side k of mg_solve_cases.shape_rhs (rounded to fp32 first), prm = key(dict)"""
    return mxr.K(sloppy_shape_problem(shape, clover), mgc.shape_rhs(shape[0])[k], **dict(prm))


@functools.lru_cache(maxsize=None)
def sensitivity(shape, clover, prm, k=0):
    """the largest relative movement of the model's K(r) in the max norm under three perturbations of r by one fp32 ulp"""
    sp, r = sloppy_shape_problem(shape, clover), mgc.shape_rhs(shape[0])[k]
    z = K_model(shape, clover, k, prm)
    return max(rel_err(mxr.K(sp, mxr.ulp32_perturbed(r, seed), **dict(prm)), z) for seed in (1, 2, 3))


def _problem_and_rhs(case):
    where, field, _, _ = case
    if where == "4^4":
        return mgc.problem(field), sloppy_problem(field), [mgc.rhs(field)[i] for i in mgc.RHS_USED]
    return mgc.shape_problem(*mgc.RAGGED), sloppy_shape_problem(mgc.RAGGED), list(mgc.shape_rhs(mgc.RAGGED[0])[:2])


@functools.lru_cache(maxsize=None)
def count_table(case):
    """(tol, fp64 counts, model counts) of one of SOLVE_CASES for its two right-hand sides.  tol comes from
    mg_solve_cases.solve_with_margin and is nudged further down until no entry of the model's histories lies within 1 % of it either."""
    _, _, nKrylov, nuPost = case
    prob, sp, bs = _problem_and_rhs(case)
    tol = mgc.TOL
    for _ in range(20):
        tol, runs = mgc.solve_with_margin(prob, bs, tol=tol, nKrylov=nKrylov, nuPost=nuPost)
        mixed = [mxr.solve(prob, b, sp, tol=tol, nKrylov=nKrylov, nuPost=nuPost) for b in bs]
        assert all(m[3] for m in mixed), case
        if all(mgc._margin_ok(m[2], tol) for m in mixed):
            return tol, tuple(r[1] for r in runs), tuple(m[1] for m in mixed)
        tol /= 1.03
    raise AssertionError("no tolerance with a 1 % margin to every history entry")


def gap(case):
    """the iterations the model needs beyond the fp64 restatement, at most, over the right-hand sides of the case (never below 0)"""
    _, n64, n32 = count_table(case)
    return max(0, max(b - a for a, b in zip(n64, n32)))
