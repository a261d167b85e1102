"""The problems the coarse-eigensolver tests share (tests/test_coarse_eig_cpu.py, tests/test_gpu_coarse_eig.py), built from
tests/coarse_op_cases.py (links, null_vectors, reference) and computed once: the dense A = MdagM | MMdag of the coarse operator from
coarse_op_ref applied to unit vectors, its numpy.linalg.eigh spectrum, seeded start vectors and the restatement's run."""
import functools

import numpy as np

import coarse_eig_ref as cer
import coarse_op_cases as coc
import coarse_op_ref as cor

SOLVER_SHAPES = [0, 1, 2, 5]          # indices into coarse_op_cases.SHAPES
# nConv, nKr per shape (issue: nKr 24-32, nConv 8-16); shape 1 has the locked-prefix case nConv 16, nKr 32 on dimension 256
SIZES = {0: (8, 24), 1: (16, 32), 2: (12, 32), 5: (16, 32)}
POLY_DEG = 20
TOL = 1e-10

# Gram / rotate fields: coarse X, n_vec.  The Gram chunk is 4096 complex elements, so the third shape of the issue (18 432 elements) gives
# five chunks with a ragged last one (2048 elements); the second (320 elements) is ragged against the 8-element step of a wave
GRAM_SHAPES = [((2, 2, 2, 2), 4), ((4, 2, 2, 2), 5), ((4, 4, 4, 6), 24)]
GRAM_M = [1, 7, 8, 9, 16, 17, 40]
GRAM_CHUNK = 4096


def dimension(idx):
    X, bs, nvec = coc.SHAPES[idx]
    return int(np.prod(coc.coarse_dims(X, bs))) * 2 * nvec


def field_shape(idx):
    X, bs, nvec = coc.SHAPES[idx]
    Xc = coc.coarse_dims(X, bs)
    return (2, int(np.prod(Xc)) // 2, 2, nvec)


@functools.lru_cache(maxsize=None)
def dense_M(idx, clover):
    """M_c as a dense n x n matrix over the flattened logical layout [2, volCB_c, 2, n_vec]: coarse_op_ref on unit vectors"""
    X, bs, nvec = coc.SHAPES[idx]
    Xc = coc.coarse_dims(X, bs)
    M = coc.reference(X, bs, nvec, clover)
    n, shape = dimension(idx), field_shape(idx)
    D = np.empty((n, n), dtype=np.complex128)
    e = np.zeros(n, dtype=np.complex128)
    for k in range(n):
        e[k] = 1.0
        D[:, k] = cor.apply_Mc(M, e.reshape(shape), Xc).reshape(n)
        e[k] = 0.0
    return D


@functools.lru_cache(maxsize=None)
def dense_A(idx, clover, op=cor.OP_MDAGM):
    D = dense_M(idx, clover)
    A = D.conj().T @ D if op == cor.OP_MDAGM else D @ D.conj().T
    return 0.5 * (A + A.conj().T)


@functools.lru_cache(maxsize=None)
def spectrum(idx, clover, op=cor.OP_MDAGM):
    return np.linalg.eigvalsh(dense_A(idx, clover, op))


@functools.lru_cache(maxsize=None)
def start_vectors(idx, nKr, seed=0):
    """n x nKr seeded Gaussian noise"""
    rng = np.random.default_rng(7700 + idx + 100 * seed)
    n = dimension(idx)
    return rng.standard_normal((n, nKr)) + 1j * rng.standard_normal((n, nKr))


@functools.lru_cache(maxsize=None)
def restatement(idx, clover, op=cor.OP_MDAGM, aMin=0.0, aMax=0.0, maxIter=100, nOrtho=2):
    """the restatement applies A as the device does: M_c (or its adjoint) first, then the other, never the product matrix"""
    nConv, nKr = SIZES[idx]
    D = dense_M(idx, clover)
    Dd = D.conj().T
    A = (lambda x: Dd @ (D @ x)) if op == cor.OP_MDAGM else (lambda x: D @ (Dd @ x))
    return cer.eigensolve(A, start_vectors(idx, nKr), nConv, TOL, maxIter, POLY_DEG, aMin, aMax, nOrtho)
