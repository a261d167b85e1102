"""The problems the coarse-eigensolver tests share (tests/test_coarse_eig_cpu.py, tests/test_gpu_coarse_eig.py), built from
tests/coarse_op_cases.py (links, null_vectors, reference) and computed once: the dense A = MdagM | MMdag of the coarse operator from
coarse_op_ref applied to unit vectors, its numpy.linalg.eigh spectrum, seeded start vectors and the restatement's run.  For
tests/test_gpu_coarse_eig_scale.py: the long shapes, a synthetic operator of 4224 elements per vector with its block application and
restatement, and a numpy restatement of the Gram kernel's summation tree."""
import functools

import numpy as np

import coarse_eig_ref as cer
import coarse_op_cases as coc
import coarse_op_ref as cor
from util import orc

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


# Beyond one fan run of the chunk sum and one 64-output block of the rotation (tests/test_gpu_coarse_eig_scale.py).  coarse_gram_sum_kernel
# adds the chunks GRAM_FAN to a run: 32 768 elements are exactly 8 chunks (one full run, no second); 38 016 are 10 chunks, the last of
# 1152 elements = 4.5 runs of 256, in rows of 288 that cut a wave; 67 584 are 17 chunks, the third fan run a single short chunk (2048)
LONG_SHAPES = [((4, 4, 4, 8), 32), ((4, 4, 6, 6), 33), ((8, 8, 4, 4), 33)]
WIDE_M = [64, 65, 72, 129, 200, 264]  # one block of 64 outputs / two 32-row blocks exactly, and every way past them up to nKr > 256
GRAM_LEAF, GRAM_RUN, GRAM_STEP, GRAM_FAN = 16, 256, 8, 8

# the solver at scale: 4224 elements per vector = one chunk of 4096 and a ragged one of half a run, rows of 96
SCALE_XC, SCALE_NVEC = (4, 4, 2, 6), 11
SCALE_CASES = [(66, 72, 8, 1), (8, 264, 2, 1)]  # nConv, nKr, polyDeg, maxIter


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


# ---- the solver at scale: a synthetic operator (a Galerkin build of this size costs 16-19 s of numpy, which no test may pay) -----------------
def scale_field_shape():
    return (2, int(np.prod(SCALE_XC)) // 2, 2, SCALE_NVEC)


def scale_dimension():
    return int(np.prod(scale_field_shape()))


@functools.lru_cache(maxsize=None)
def scale_operator():
    """[2, volCB, 9, N, N], seeded: the diagonal term 1 + 0.3 G / sqrt(N), the eight hop terms 0.12 G / sqrt(N), G complex Gaussian.  The
    matrices obey no relation among themselves (Y- is not the adjoint of a Y+), so M^dag is right only as the explicit adjoint"""
    rng = np.random.default_rng(7800)
    vcb, N = int(np.prod(SCALE_XC)) // 2, 2 * SCALE_NVEC
    G = (rng.standard_normal((2, vcb, 9, N, N)) + 1j * rng.standard_normal((2, vcb, 9, N, N))) / np.sqrt(N)
    M = 0.12 * G
    M[:, :, 0] = np.eye(N) + 0.3 * G[:, :, 0]
    return M


def _dag(A):
    return np.conj(np.swapaxes(A, -1, -2))


def apply_block(M, W, Xc, dagger=False):
    """coarse_op_ref.apply_Mc on a block of columns, W [2, volCB_c, N, k]: the same neighbour tables, the products through numpy.matmul"""
    vcbc = W.shape[1]
    W = W.astype(np.complex128, copy=False)
    out = np.empty_like(W)
    for p in range(2):
        coord = orc.get_coords(np.arange(vcbc), Xc, p)
        out[p] = np.matmul(_dag(M[p, :, 0]) if dagger else M[p, :, 0], W[p])
        for mu in range(4):
            f, b = orc.link_index_p1(coord, Xc, mu), orc.link_index_m1(coord, Xc, mu)
            if not dagger:
                out[p] += np.matmul(M[p, :, 1 + 2 * mu], W[1 - p, f]) + np.matmul(M[p, :, 2 + 2 * mu], W[1 - p, b])
            else:
                out[p] += np.matmul(_dag(M[1 - p, f, 2 + 2 * mu]), W[1 - p, f]) + np.matmul(_dag(M[1 - p, b, 1 + 2 * mu]), W[1 - p, b])
    return out


def scale_A(x):
    """A = M^dag (M x) of the synthetic operator on an n x k block of columns over the flattened logical layout"""
    M = scale_operator()
    vcb, N = int(np.prod(SCALE_XC)) // 2, 2 * SCALE_NVEC
    W = np.ascontiguousarray(x).reshape(2, vcb, N, x.shape[1])
    return apply_block(M, apply_block(M, W, SCALE_XC), SCALE_XC, dagger=True).reshape(x.shape)


@functools.lru_cache(maxsize=None)
def scale_start(nKr, ulp=0):
    """n x nKr seeded Gaussian noise; ulp: every real and imaginary part moved that many units in the last place upwards"""
    rng = np.random.default_rng(7900 + nKr)
    n = scale_dimension()
    S = rng.standard_normal((n, nKr)) + 1j * rng.standard_normal((n, nKr))
    for _ in range(ulp):
        S = np.nextafter(S.real, np.inf) + 1j * np.nextafter(S.imag, np.inf)
    return S


@functools.lru_cache(maxsize=None)
def scale_restatement(nConv, nKr, polyDeg, maxIter, ulp=0):
    return cer.eigensolve(scale_A, scale_start(nKr, ulp), nConv, TOL, maxIter, polyDeg)


def gram_tree_diagonal(a, leaf=None):
    """numpy emulation of the summation tree of coarse_gram_kernel / coarse_gram_sum_kernel on the diagonal G_ii = sum |a_i[e]|^2 of the
    rows of a [m, L] (kernel element order): a step of the matrix instruction adds 4 products to its accumulator, one after the other,
    each product and each sum rounded (on an MI355X the device's diagonal came out as this model to the digit); of 8 elements the even
    ones go first, re re before im im; a leaf of GRAM_LEAF elements is one chain; the leaves of a run of GRAM_RUN elements are added in
    order, the runs of a chunk in order, the chunks GRAM_FAN to a fan run, the fan runs in order.  leaf = GRAM_RUN is the tree without
    the leaf level, as the kernel was first written.  Zero padding stands for the ragged ends: adding +0 changes nothing"""
    leaf = GRAM_LEAF if leaf is None else leaf
    m, L = a.shape
    span = GRAM_CHUNK * GRAM_FAN
    Lp = (L + span - 1) // span * span
    z = np.zeros((m, Lp), dtype=np.complex128)
    z[:, :L] = a
    z = z.reshape(m, Lp // leaf, leaf // GRAM_STEP, GRAM_STEP)               # vector, leaf, trip, element of the trip
    acc = np.zeros((m, Lp // leaf))
    for trip in range(leaf // GRAM_STEP):
        for u in range(2):
            for part in (z.real, z.imag):
                for k in range(4):
                    x = part[:, :, trip, 2 * k + u]
                    acc = acc + x * x

    def chains(x, n):
        """groups of n neighbours, each added in order from zero"""
        x = x.reshape(m, -1, n)
        s = np.zeros(x.shape[:2])
        for i in range(n):
            s = s + x[:, :, i]
        return s
    fan = chains(chains(chains(acc, GRAM_RUN // leaf), GRAM_CHUNK // GRAM_RUN), GRAM_FAN)
    return chains(fan, fan.shape[1])[:, 0]
