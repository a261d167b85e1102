"""The problems of the three-level solver's scale tests (tests/test_mg_solve3_scale_cpu.py, tests/test_gpu_mg_solve3_scale.py), seeded and
computed once, chosen for what the level-1 and level-2 vectors and the coarse application look like inside a cycle:

  PROD   X = (8, 4, 4, 4), aggregates 2^4 with n_vec 24 -> X1 = (4, 2, 2, 2), aggregates (2, 1, 1, 1) with n_vec 32 -> X2 = (2, 2, 2, 2):
         the production colours (N_1 = 48, N_2 = 64) on the smallest lattice that carries them.  A level-1 vector has 1536 elements, 6
         workgroups of the Krylov kernels, rows of 16; a level-2 vector 1024 elements, 4 workgroups, rows of 8.  With and without clover.
  WIDE   X = (8, 8, 8, 8), aggregates 2^4 with n_vec 33 -> X1 = (4, 4, 4, 4), aggregates 2^4 with n_vec 5 -> X2 = (2, 2, 2, 2): the
         smallest hierarchy on which M_1 takes the 64-output form of coarse_apply_kernel by default (256 sites x 2 chunks of N_1 = 66, the
         last with 2 live outputs: 512 workgroups; fewer sites would need three chunks, which n_vec <= 64 forbids, and 33 columns need the
         96 degrees of freedom per chirality of a 2^4 aggregate).  N_2 = 10 is below one 16-lane chunk.  A level-1 vector has 16 896
         elements, 66 workgroups; a fine one 49 152, 192 workgroups.  Wilson-clover.

Links, clover blocks and V0 are those of coarse_op_cases; V1 is random, scaled by 1 / sqrt(n_vec0), as coarse_op2_cases.hierarchy makes it.
Nothing is block-orthonormal: nothing may assume it.

The reference is tests/mg_solve3_ref.py on the CHAIN hierarchy A_1 = R_0 M P_0, A_2 = R_1 A_1 P_1 (no matrices are built: M_1 at WIDE has
256 x 9 x 66^2 entries, and coarse_op_ref.build takes 8 s at PROD); at PROD the explicit matrices exist too, tests/test_mg_solve3_scale_cpu.py
holds the chain's K^(3) to theirs, and the fp32 model (Hierarchy.sloppy, which needs rounded matrices) is built from them."""
import functools

import numpy as np

import clover_ref as cr
import coarse_op_cases as coc
import mg_solve3_ref as m3
import mg_solve_mixed_ref as mxr
import mg_solve_ref as mgr
import restrict_ref as rr
import wilson_ref as wr
from util import orc, rel_err

KAPPA = coc.KAPPA
# name -> (X, first aggregate, n_vec0, second aggregate, n_vec1, clover)
SHAPES = {"prod": ((8, 4, 4, 4), (2, 2, 2, 2), 24, (2, 1, 1, 1), 32, False),
          "prod-clover": ((8, 4, 4, 4), (2, 2, 2, 2), 24, (2, 1, 1, 1), 32, True),
          "wide": ((8, 8, 8, 8), (2, 2, 2, 2), 33, (2, 2, 2, 2), 5, True)}
NRHS = 9
# (params[0], params[1]) as in mg_solve3_cases.K3_PARAMS.  PROD A runs every kind of step; PROD B has 15 Gram-Schmidt coefficients on level
# 1 (summed over 6 workgroups) and 16 steps on level 2 (over 4)
PROD_PARAMS = {"A": ((1, 1, 2), (1, 1, 0.85, 8)), "B": ((0, 2, 16), (0, 1, 1.0, 16))}
WIDE_PARAMS = {"A": ((1, 1, 2), (1, 1, 0.85, 4)), "C": ((0, 1, 4), (0, 2, 1.0, 4))}
WIDE_SOLVE = dict(maxIter=4, nKrylov=4)           # with WIDE_PARAMS["A"]: four iterations, not converged


def sets(name):
    return WIDE_PARAMS if name == "wide" else PROD_PARAMS


def params(p0, p1):
    return [dict(nuPre=p0[0], nuPost=p0[1], coarseIters=p0[2]), dict(nuPre=p1[0], nuPost=p1[1], omega=p1[2], coarseIters=p1[3])]


def dims(name):
    """(X, X1, X2)"""
    X, bs0, _, bs1, _, _ = SHAPES[name]
    X1 = coc.coarse_dims(X, bs0)
    return X, X1, coc.coarse_dims(X1, bs1)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(X, Uo, blocks (None without clover), A_eo, V0, V1, bs0, bs1, nv0, nv1, X1, X2)"""
    X, bs0, nv0, bs1, nv1, clover = SHAPES[name]
    Uo, blocks = coc.links(X)
    V0 = coc.null_vectors(X, bs0, nv0)[0]
    _, X1, X2 = dims(name)
    rng = np.random.default_rng(6700 + nv0 + nv1 + sum(X))
    V1 = coc.c(rng, (2, int(np.prod(X1)) // 2, 2, nv0, nv1)) / np.sqrt(1.0 * nv0)
    return dict(X=X, Uo=Uo, blocks=blocks if clover else None, A_eo=coc.dense12(blocks) if clover else None, V0=V0, V1=V1, bs0=bs0, bs1=bs1,
                nv0=nv0, nv1=nv1, X1=X1, X2=X2)


def chain_hierarchy(X, Uo, kappa, Vs, bss, A_eo=None):
    """mg_solve3_ref.Hierarchy whose coarse operators are the chains A_{l+1} = R_l A_l P_l, applied as such; parts as Hierarchy.build
    leaves them, without matrices, so that .sloppy() still builds the rounded ones"""
    Xs = [tuple(X)]
    for bs in bss:
        Xs.append(tuple(Xs[-1][d] // bs[d] for d in range(4)))

    def M(v):
        return wr.wilson_M(v, Uo, kappa, Xs[0]) if A_eo is None else cr.clover_M(v, Uo, A_eo, kappa, Xs[0])
    R = [(lambda v, l=l: rr.restrict(v, Vs[l], Xs[l], bss[l], spin_bs=2 if l == 0 else 1)) for l in range(len(Vs))]
    P = [(lambda w, l=l: orc.prolongate(w, Vs[l], Xs[l], bss[l], 2 if l == 0 else 1)) for l in range(len(Vs))]
    A = [M]
    for l in range(len(Vs)):
        A.append(lambda w, l=l: R[l](A[l](P[l](w))))
    return m3.Hierarchy(A, R, P, dict(X=Xs[0], Xs=Xs, Uo=Uo, kappa=kappa, Vs=list(Vs), bss=list(bss), A_eo=A_eo, Ks=None))


@functools.lru_cache(maxsize=None)
def chain(name):
    i = inputs(name)
    return chain_hierarchy(i["X"], i["Uo"], KAPPA, [i["V0"], i["V1"]], [i["bs0"], i["bs1"]], i["A_eo"])


@functools.lru_cache(maxsize=None)
def explicit(name):
    """the hierarchy on the matrices of coarse_op_ref.build and coarse_op2_ref.build: PROD only"""
    assert name != "wide"
    i = inputs(name)
    return m3.Hierarchy.build(i["X"], i["Uo"], KAPPA, [i["V0"], i["V1"]], [i["bs0"], i["bs1"]], i["A_eo"])


@functools.lru_cache(maxsize=None)
def sloppy(name):
    """the fp32 model's hierarchy (rounded V, matrices rebuilt from them and rounded): PROD only"""
    assert name != "wide"
    return chain(name).sloppy()


@functools.lru_cache(maxsize=None)
def rhs(X, n=NRHS):
    rng = np.random.default_rng(8900 + sum(X))
    return tuple(coc.c(rng, (2, int(np.prod(X)) // 2, 4, 3)) for _ in range(n))


@functools.lru_cache(maxsize=None)
def K3_reference(name, s, k):
    """K^(3) of the chain hierarchy for parameter set s and right-hand side k"""
    return m3.K(chain(name), rhs(SHAPES[name][0])[k], params(*sets(name)[s]))


@functools.lru_cache(maxsize=None)
def K3_explicit(name, s, k):
    return m3.K(explicit(name), rhs(SHAPES[name][0])[k], params(*sets(name)[s]))


@functools.lru_cache(maxsize=None)
def K3_sensitivity(name, s, seeds=(1, 2, 3)):
    """the chain restatement's own largest relative movement of K^(3)(r_0) in the max norm under 1-ulp perturbations of r_0"""
    z = K3_reference(name, s, 0)
    r0 = rhs(SHAPES[name][0])[0]
    return max(rel_err(m3.K(chain(name), mgr.ulp_perturbed(r0, seed), params(*sets(name)[s])), z) for seed in seeds)


@functools.lru_cache(maxsize=None)
def K32_model(name, s, k):
    return m3.K32(sloppy(name), rhs(SHAPES[name][0])[k], params(*sets(name)[s]))


@functools.lru_cache(maxsize=None)
def K32_sensitivity(name, s):
    """as mg_solve3_cases.K32_sensitivity: the model under three perturbations of r_0 by one fp32 ulp"""
    z = K32_model(name, s, 0)
    r0 = rhs(SHAPES[name][0])[0]
    return max(rel_err(m3.K32(sloppy(name), mxr.ulp32_perturbed(r0, seed), params(*sets(name)[s])), z) for seed in (1, 2, 3))
