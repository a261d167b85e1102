"""The problems the tests of the coarse -> coarse operator share (tests/test_coarse_op2_cpu.py, tests/test_gpu_coarse_op2.py), seeded and
computed once.  The kernel-level cases take RANDOM DENSE matrices as the input operator -- the definition needs no fine lattice -- the
hierarchy cases a fine Wilson(-clover) operator under two transfers."""
import functools

import numpy as np

import coarse_op2_ref as c2r
import coarse_op_cases as c1
import coarse_op_ref as cor

# (level-1 lattice, aggregate, nc, nv) -- each can go wrong in its own way
KERNEL_CASES = [((4, 2, 2, 2), (2, 1, 1, 1), 4, 3),       # all coarsest extents 2; block extent 1; extent 2 on the input lattice: x+mu = x-mu there
                ((8, 2, 2, 2), (4, 1, 1, 1), 2, 3),       # sites with both x neighbours inside the aggregate
                ((8, 4, 2, 2), (2, 2, 1, 1), 5, 6),       # coarsest extent 4 along x separates Y'+ from Y'-; odd nc
                ((4, 4, 4, 4), (2, 2, 2, 2), 24, 32),     # the production matrix sizes, N0 48 and N1 64
                ((4, 2, 2, 2), (2, 1, 1, 1), 33, 4),      # N0 > 64: a ragged last panel of K
                ((4, 2, 2, 2), (2, 1, 1, 1), 5, 33),      # N1^2 > 4096: a ragged last micro-tile in every quadrant
                ((2, 2, 2, 2), (1, 1, 1, 1), 64, 64)]     # the LDS limit
FP32_CASES = [KERNEL_CASES[0], KERNEL_CASES[3]]
# fine lattice, first aggregate, n_vec, second aggregate, n_vec1, clover
HIERARCHIES = [((8, 4, 4, 4), (2, 2, 2, 2), 4, (2, 1, 1, 1), 3, True),
               ((8, 8, 4, 4), (2, 2, 2, 2), 3, (2, 2, 1, 1), 5, False),
               ((16, 4, 4, 4), (2, 2, 2, 2), 2, (4, 1, 1, 1), 3, True)]
KAPPA = c1.KAPPA
NW = 9                                                    # coarsest vectors: a block of 8 and one more

coarse_dims = c1.coarse_dims


@functools.lru_cache(maxsize=None)
def kernel_inputs(X, bs, nc, nv):
    """(K [2, volCB, 9, 2 nc, 2 nc] random dense, V [2, volCB, 2, nc, nv] random and NOT block-orthonormal)"""
    rng = np.random.default_rng(7700 + 64 * nc + nv + sum(X) + sum(bs))
    vcb = int(np.prod(X)) // 2
    K = c1.c(rng, (2, vcb, 9, 2 * nc, 2 * nc)) / np.sqrt(2.0 * nc)
    V = c1.c(rng, (2, vcb, 2, nc, nv)) / np.sqrt(1.0 * nc)
    return K, V


@functools.lru_cache(maxsize=None)
def kernel_reference(X, bs, nc, nv, prec=8):
    """coarse_op2_ref.build of the inputs as a device of storage precision `prec` holds them"""
    K, V = kernel_inputs(X, bs, nc, nv)
    if prec == 4:
        K, V = K.astype(np.complex64).astype(np.complex128), V.astype(np.complex64).astype(np.complex128)
    return c2r.build(K, V, X, bs)


@functools.lru_cache(maxsize=None)
def hierarchy(i, clover=None):
    """everything of HIERARCHIES[i]: links, clover, both V (random, not block-orthonormal), the reference operators of both levels and
    NW coarsest vectors.  clover: None takes the table's, True / False override it (same links and vectors)"""
    X, bs0, nv0, bs1, nv1, table = HIERARCHIES[i]
    clover = table if clover is None else clover
    Uo, blocks = c1.links(X)
    A_eo = c1.dense12(blocks) if clover else None
    V0, _ = c1.null_vectors(X, bs0, nv0)
    X1 = coarse_dims(X, bs0)
    X2 = coarse_dims(X1, bs1)
    rng = np.random.default_rng(6600 + i)
    vcb1, vcb2 = int(np.prod(X1)) // 2, int(np.prod(X2)) // 2
    V1 = c1.c(rng, (2, vcb1, 2, nv0, nv1)) / np.sqrt(1.0 * nv0)
    ws = [c1.c(rng, (2, vcb2, 2, nv1)) for _ in range(NW)]
    K1 = cor.build(V0, Uo, A_eo, KAPPA, X, bs0)
    K2 = c2r.build(K1, V1, X1, bs1)
    return dict(X=X, bs0=bs0, nv0=nv0, bs1=bs1, nv1=nv1, clover=clover, Uo=Uo, blocks=blocks, A_eo=A_eo, V0=V0, V1=V1, X1=X1, X2=X2, K1=K1, K2=K2,
                ws=ws)
