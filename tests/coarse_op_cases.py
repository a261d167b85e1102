"""The problems the coarse-operator tests share (tests/test_coarse_op_cpu.py, tests/test_gpu_coarse_op.py), seeded and computed once:
links, clover blocks, null vectors, coarse vectors and the reference matrices of tests/coarse_op_ref.py."""
import functools

import numpy as np

import clover_ref as cr
import coarse_op_ref as cor
from util import orc, random_gauge_lex

# fine X, aggregate, n_vec -- each can go wrong in its own way
SHAPES = [((4, 4, 4, 4), (2, 2, 2, 2), 4),     # every coarse extent 2: Y+ and Y- hit the same neighbour
          ((4, 4, 4, 4), (2, 2, 2, 2), 8),
          ((8, 4, 4, 4), (2, 2, 2, 2), 5),     # extent 4 along x separates forward from backward; n_vec not a multiple of 4
          ((8, 4, 4, 4), (2, 1, 2, 2), 13),    # block extent 1: no y hop stays inside an aggregate
          ((8, 4, 4, 4), (4, 2, 2, 2), 6),     # sites with both x neighbours inside the aggregate
          ((4, 4, 4, 8), (2, 2, 2, 2), 24)]    # production matrix size N = 48
# beyond the table: a workgroup of coarse_apply_kernel takes 64 output components and one of coarse_build_kernel 4096 matrix elements;
# n_vec 33 (N = 66, N^2 = 4356) gives both kernels a second, ragged chunk
LARGE_NVEC = [((4, 4, 4, 4), (2, 2, 2, 2), 33)]
# x, y and z pairwise distinct on the fine and on the coarse lattice, one coarse extent 6 (no power of two): in every table above y = z, so
# a multiplier or a modulus taken from the wrong axis in get_coords, lex_index or a face index changes nothing there
ANISO = [((4, 8, 12, 4), (2, 2, 2, 2), 5),     # coarse (2, 4, 6, 2), 96 coarse sites
         ((12, 4, 8, 4), (2, 2, 2, 2), 4)]     # coarse (6, 2, 4, 2): the checkerboard axis carries the 6, the face of x has y != z
KAPPA = 0.12
CSW_COEFF = 0.17
NW = 17                                        # coarse vectors: two blocks of 8 and one more


def c(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def dense12(B):
    A = np.zeros(B.shape[:-3] + (12, 12), dtype=np.complex128)
    A[..., :6, :6] = B[..., 0, :, :]
    A[..., 6:, 6:] = B[..., 1, :, :]
    return A


@functools.lru_cache(maxsize=None)
def links(X, kind="su3"):
    """(links [4, 2, volCB, 3, 3] on the periodic domain X, clover blocks [2, volCB, 2, 6, 6] of the same links).  kind "su3": random
    SU(3); "scaled": every link times a random factor in [0.7, 1.3] (U^dag is then not the inverse); "fp32": rounded to complex64."""
    rng = np.random.default_rng(8800 + sum(X) + len(kind))
    U_lex = random_gauge_lex(rng, X)
    if kind == "scaled":
        U_lex = U_lex * rng.uniform(0.7, 1.3, size=U_lex.shape[:5])[..., None, None]
    elif kind == "fp32":
        U_lex = U_lex.astype(np.complex64).astype(np.complex128)
    Uo = orc.extended_gauge_from_global(U_lex, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    return Uo, cr.clover_blocks_eo(U_lex, CSW_COEFF, X)


@functools.lru_cache(maxsize=None)
def null_vectors(X, bs, nvec):
    """V [2, volCB, 4, 3, n_vec] (random, not block-orthonormal: nothing may assume it) and NW coarse vectors [2, volCB_c, 2, n_vec]"""
    rng = np.random.default_rng(9900 + nvec + sum(X) + sum(bs))
    vcb = int(np.prod(X)) // 2
    vcbc = vcb // int(np.prod(bs))
    V = c(rng, (2, vcb, 4, 3, nvec)) / np.sqrt(12.0 * nvec)
    ws = [c(rng, (2, vcbc, 2, nvec)) for _ in range(NW)]
    return V, ws


@functools.lru_cache(maxsize=None)
def reference(X, bs, nvec, clover, kind="su3"):
    """the matrices of coarse_op_ref.build, [2, volCB_c, 9, N, N]"""
    Uo, blocks = links(X, kind)
    V, _ = null_vectors(X, bs, nvec)
    return cor.build(V, Uo, dense12(blocks) if clover else None, KAPPA, X, bs)


def coarse_dims(X, bs):
    return tuple(X[d] // bs[d] for d in range(4))
