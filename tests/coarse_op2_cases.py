"""The problems the tests of the coarse -> coarse operator share (tests/test_coarse_op2_cpu.py, tests/test_gpu_coarse_op2.py), seeded and
computed once.  The kernel-level cases take RANDOM DENSE matrices as the input operator -- the definition needs no fine lattice -- the
hierarchy cases a fine Wilson(-clover) operator under two transfers."""
import functools

import numpy as np

import coarse_op2_ref as c2r
import coarse_op_cases as c1
import coarse_op_ref as cor

# ---- the launch geometry of coarse_build2_kernel, restated (csrc/coarse_op2.hip; tests/test_coarse_op2_cpu.py holds it to the source) ------
C2_THREADS, C2_TILE, C2_MAX_N, C2_MIN_PANEL, C2_LDS_TARGET = 256, 4, 64, 8, 4096
BUILD2_PANEL_EXPR = "std::min(nc, std::max(kC2MinPanel, (kC2LdsTarget - 2 * nc * nv) / (nc + nv)))"
REGIMES = ("single_panel", "even_panels", "ragged_last_panel", "multi_site", "multi_term", "both_neighbours_inside", "shadow_rows", "shadow_out",
           "rows_gt_cols", "cols_gt_rows", "lds_over_64k")


def build2_panel(nc, nv):
    """build2_panel of the source: columns of K (rows of V(x')) per panel.  int(a / b): C++ division truncates towards zero"""
    return min(nc, max(C2_MIN_PANEL, int((C2_LDS_TARGET - 2 * nc * nv) / (nc + nv))))


def build2_geometry(X, bs, nc, nv):
    """the panels, the LDS and the regimes of one coarse_build2_kernel launch: K on the lattice X, aggregates bs, nc -> nv colours"""
    assert 1 <= nc <= C2_MAX_N and 1 <= nv <= C2_MAX_N
    pk = build2_panel(nc, nv)
    panels = [min(pk, nc - p0) for p0 in range(0, nc, pk)]
    lds = 16 * (2 * nc * nv + pk * (nc + nv))
    span = C2_THREADS // 16 * C2_TILE                       # rows / columns the 16 x 16 lanes of 4 x 4 micro-tiles cover: 64
    return dict(pk=pk, panels=panels, lds=lds,
                single_panel=len(panels) == 1,
                even_panels=len(panels) > 1 and panels[-1] == pk,
                ragged_last_panel=len(panels) > 1 and panels[-1] < pk,
                multi_site=int(np.prod(bs)) > 1,
                multi_term=any(b > 1 for b in bs),          # Xd' takes K_0 and every hop that stays inside: more than one term of one site
                both_neighbours_inside=any(b >= 3 for b in bs),
                shadow_rows=nc % C2_TILE != 0 or nc < span,  # lanes past the end of T: they shadow its last row and do not store
                shadow_out=nv % C2_TILE != 0 or nv < span,   # ... past the end of the output
                rows_gt_cols=nc > nv,                       # tRow and oRow clamp differently: tRow reaches further
                cols_gt_rows=nv > nc,                       # ... oRow does
                lds_over_64k=lds > 64 * 1024)               # the launch raises the dynamic-LDS attribute


def regimes(X, bs, nc, nv):
    g = build2_geometry(X, bs, nc, nv)
    return frozenset(r for r in REGIMES if g[r])


def _for(*names):
    assert all(n in REGIMES for n in names), names
    return frozenset(names)


# (level-1 lattice, aggregate, nc, nv, the regimes of build2_geometry the case is there for) -- each can go wrong in its own way.  The sets
# are asserted in tests/test_coarse_op2_cpu.py, case by case and as a table.  Beyond them: case 0 has all coarsest extents 2 and extent 2 on
# the input lattice (x+mu = x-mu there); case 2 has coarsest extent 4 along x, which separates Y'+ from Y'-; case 3 has the production
# matrix sizes, N0 48 and N1 64.
KERNEL_CASES = [((4, 2, 2, 2), (2, 1, 1, 1), 4, 3, _for("single_panel", "multi_site", "multi_term", "shadow_rows", "shadow_out")),
                ((8, 2, 2, 2), (4, 1, 1, 1), 2, 3, _for("single_panel", "both_neighbours_inside", "cols_gt_rows")),
                ((8, 4, 2, 2), (2, 2, 1, 1), 5, 6, _for("single_panel", "multi_site", "multi_term", "shadow_rows")),
                ((4, 4, 4, 4), (2, 2, 2, 2), 24, 32, _for("single_panel", "multi_site", "multi_term", "cols_gt_rows")),
                ((4, 2, 2, 2), (2, 1, 1, 1), 33, 4, _for("single_panel", "shadow_rows", "rows_gt_cols")),      # ONE panel of 33 columns
                ((4, 2, 2, 2), (2, 1, 1, 1), 5, 33, _for("single_panel", "shadow_out", "cols_gt_rows")),       # a ragged last micro-tile of the output
                ((2, 2, 2, 2), (1, 1, 1, 1), 64, 64, _for("even_panels", "lds_over_64k")),                     # the LDS limit; one site, one term
                # more than one panel (nc^2 + 3 nc nv > 4096) together with several terms and sites
                ((4, 2, 2, 2), (2, 1, 1, 1), 40, 24, _for("ragged_last_panel", "multi_term", "multi_site", "rows_gt_cols")),   # [34, 6], 64.0 KB
                ((4, 2, 2, 2), (2, 1, 1, 1), 37, 35, _for("ragged_last_panel", "multi_term", "multi_site", "shadow_rows", "shadow_out")),  # [20, 17]
                ((4, 2, 2, 2), (2, 1, 1, 1), 40, 40, _for("ragged_last_panel", "multi_term", "multi_site")),                  # [11, 11, 11, 7]
                ((4, 2, 2, 2), (2, 1, 1, 1), 32, 48, _for("ragged_last_panel", "multi_term", "multi_site", "cols_gt_rows")),   # [12, 12, 8]
                ((8, 2, 2, 2), (4, 1, 1, 1), 48, 48, _for("even_panels", "multi_term", "multi_site", "both_neighbours_inside", "lds_over_64k")),
                ((4, 4, 2, 2), (2, 2, 1, 1), 64, 64, _for("even_panels", "multi_term", "multi_site", "lds_over_64k"))]
FP32_CASES = [KERNEL_CASES[0], KERNEL_CASES[3], KERNEL_CASES[7], KERNEL_CASES[8]]
# fine lattice, first aggregate, n_vec, second aggregate, n_vec1, clover
HIERARCHIES = [((8, 4, 4, 4), (2, 2, 2, 2), 4, (2, 1, 1, 1), 3, True),
               ((8, 8, 4, 4), (2, 2, 2, 2), 3, (2, 2, 1, 1), 5, False),
               ((16, 4, 4, 4), (2, 2, 2, 2), 2, (4, 1, 1, 1), 3, True)]
KAPPA = c1.KAPPA
NW = 9                                                    # coarsest vectors: a block of 8 and one more
# a chain at multi-panel widths, for the device alone: fine lattice, first aggregate, n_vec, second aggregate, n_vec1 (Wilson-clover).  Not in
# HIERARCHIES: coarse_op_ref.build at n_vec 36 is no sub-second reference, and two device routes need no numpy matrices
WIDE_CHAIN = ((8, 4, 4, 4), (2, 2, 2, 2), 36, (2, 1, 1, 1), 36)

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
def wide_chain():
    """the inputs of WIDE_CHAIN and nothing computed from them: links, clover blocks, two random V (not block-orthonormal) and NW coarsest
    vectors"""
    X, bs0, nv0, bs1, nv1 = WIDE_CHAIN
    Uo, blocks = c1.links(X)
    X1 = coarse_dims(X, bs0)
    X2 = coarse_dims(X1, bs1)
    rng = np.random.default_rng(6700 + nv0 + nv1)
    vcb, vcb1, vcb2 = int(np.prod(X)) // 2, int(np.prod(X1)) // 2, int(np.prod(X2)) // 2
    V0 = c1.c(rng, (2, vcb, 4, 3, nv0)) / np.sqrt(12.0 * nv0)
    V1 = c1.c(rng, (2, vcb1, 2, nv0, nv1)) / np.sqrt(1.0 * nv0)
    ws = [c1.c(rng, (2, vcb2, 2, nv1)) for _ in range(NW)]
    return dict(X=X, bs0=bs0, nv0=nv0, bs1=bs1, nv1=nv1, Uo=Uo, blocks=blocks, V0=V0, V1=V1, X1=X1, X2=X2, ws=ws)


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
