"""The explicit coarse operator on a process grid, in numpy: how the tests cut the global matrices of coarse_op_ref.build and global coarse
vectors into rank-local blocks (orc.local_block), which ghost slabs a rank should hold -- the neighbour ranks' faces of the input vectors
and, for M_c^dag, of their Y matrices (MugiqHipCoarseHalo in include/mugiq_hip.h) -- and the five forms applied rank by rank from local
data plus ghosts alone.  tests/test_coarse_op_grid_cpu.py pins the reassembled result to coarse_op_ref.apply_op on the global lattice, so
the decomposition the GPU tests compare against is itself checked.  Layouts: matrices [2, volCB, 9, N, N], vectors [2, volCB, 2, n_vec]
(even-odd, as everywhere in these tests); faces [2, faceCB, ...] indexed [parity of the face site, face index of the header]."""
import itertools

import numpy as np

import coarse_op_ref as cor
import wilson_ref as wr
from util import orc


def ranks(grid):
    """rank coordinates (x, y, z, t) in rank order: x slowest, t fastest (GridComm.coords_of)"""
    return list(itertools.product(*[range(g) for g in grid]))


def local_dims(G, grid):
    return tuple(G[d] // grid[d] for d in range(4))


def slice_eo(f_eo, G, coord, grid):
    """the block of rank `coord` of a global even-odd field [2, volCB, ...], as a local even-odd field"""
    return orc.lex_to_eo(orc.local_block(orc.eo_to_lex(f_eo, G), coord, grid), local_dims(G, grid))


def assemble_eo(blocks, G, grid):
    """the inverse: {rank coordinates: local even-odd field} -> the global even-odd field"""
    l = local_dims(G, grid)
    first = next(iter(blocks.values()))
    out = np.zeros((G[3], G[2], G[1], G[0]) + first.shape[2:], dtype=first.dtype)
    for c, b in blocks.items():
        out[c[3] * l[3]:(c[3] + 1) * l[3], c[2] * l[2]:(c[2] + 1) * l[2], c[1] * l[1]:(c[1] + 1) * l[1], c[0] * l[0]:(c[0] + 1) * l[0]] = orc.eo_to_lex(b, l)
    return orc.lex_to_eo(out, G)


def face_index(coord, X, mu):
    """the header's face index without the parity term: the three other coordinates, lowest axis fastest, halved"""
    a, b, c = [d for d in range(4) if d != mu]
    return ((coord[..., c] * X[b] + coord[..., b]) * X[a] + coord[..., a]) >> 1


def face(f_eo, X, mu, high):
    """[2, faceCB, ...]: the sites x[mu] = X[mu] - 1 (high) or 0 of a local field, by their own parity and face index"""
    vcb = f_eo.shape[1]
    out = np.zeros((2, vcb // X[mu]) + f_eo.shape[2:], dtype=f_eo.dtype)
    for p in range(2):
        coord = orc.get_coords(np.arange(vcb), X, p)
        sel = coord[:, mu] == (X[mu] - 1 if high else 0)
        out[p, face_index(coord[sel], X, mu)] = f_eo[p, sel]
    return out


def neighbour(coord, grid, mu, direction):
    c = list(coord)
    c[mu] = (c[mu] + direction) % grid[mu]
    return tuple(c)


def partitioned(grid, force=(0, 0, 0, 0)):
    return tuple(1 if (grid[d] > 1 or force[d]) else 0 for d in range(4))


def ghost_faces(blocks, coord, grid, part, X):
    """what rank `coord` holds of a field after the exchange: [mu][0] the backward neighbour's high face, [mu][1] the forward neighbour's
    low face (None on an axis that is not partitioned)"""
    return [[face(blocks[neighbour(coord, grid, mu, -1)], X, mu, 1), face(blocks[neighbour(coord, grid, mu, +1)], X, mu, 0)] if part[mu] else None
            for mu in range(4)]


def halo(Mblocks, coord, grid, part, X):
    """the MugiqHipCoarseHalo of rank `coord`: (Yback, Yfwd), Yback[mu] = Y+_mu of the backward neighbour's high face, Yfwd[mu] = Y-_mu of
    the forward neighbour's low face, [2, faceCB, N, N]"""
    Yb = [face(Mblocks[neighbour(coord, grid, mu, -1)][:, :, 1 + 2 * mu], X, mu, 1) if part[mu] else None for mu in range(4)]
    Yf = [face(Mblocks[neighbour(coord, grid, mu, +1)][:, :, 2 + 2 * mu], X, mu, 0) if part[mu] else None for mu in range(4)]
    return Yb, Yf


def apply_Mc_local(M, w, gw, Y, X, part, dagger=False, gamma5=False, read_index=face_index):
    """coarse_op_ref.apply_Mc on one rank: M, w local; gw = ghost_faces of w; Y = halo(...).  A hop along a partitioned axis that leaves the
    local lattice reads the ghost face, and for M_c^dag the neighbour's matrix from the halo; nothing else leaves the rank.  read_index:
    where a site looks into a face, face_index unless a test wants to know what a wrong one would do (the faces are always packed by
    face_index)."""
    vcb, nvec = w.shape[1], w.shape[-1]
    v = w.reshape(2, vcb, 2 * nvec).astype(np.complex128)
    out = np.zeros_like(v)
    dag = cor._dag
    for p in range(2):
        coord = orc.get_coords(np.arange(vcb), X, p)
        out[p] = cor._mv(dag(M[p, :, 0]) if dagger else M[p, :, 0], v[p])
        for mu in range(4):
            for fwd in (1, 0):
                n = (orc.link_index_p1 if fwd else orc.link_index_m1)(coord, X, mu)
                vin = v[1 - p, n].copy()
                mm = (2 if fwd else 1) + 2 * mu                              # M^dag: Y-_mu(X + mu) | Y+_mu(X - mu)
                A = M[1 - p, n, mm].copy() if dagger else M[p, :, (1 if fwd else 2) + 2 * mu]
                if part[mu]:
                    off = coord[:, mu] == (X[mu] - 1 if fwd else 0)
                    fi = read_index(coord[off], X, mu)
                    vin[off] = gw[mu][fwd][1 - p, fi].reshape(-1, 2 * nvec)
                    if dagger:
                        A[off] = (Y[1] if fwd else Y[0])[mu][1 - p, fi]
                out[p] += cor._mv(dag(A) if dagger else A, vin)
    out = out.reshape(w.shape)
    if gamma5:
        out = out * np.array([wr.G5[0], wr.G5[2]])[None, None, :, None]
    return out


def apply_op_grid(Mg, wg, Gc, grid, op, scale=1.0, force=(0, 0, 0, 0), read_index=face_index):
    """scale * A_c w of the form `op` on the global coarse lattice Gc, computed rank by rank on `grid`; returns ({rank coordinates: local
    result}, the reassembled global field).  read_index: see apply_Mc_local"""
    X, part = local_dims(Gc, grid), partitioned(grid, force)
    rs = ranks(grid)
    Mb = {c: slice_eo(Mg, Gc, c, grid) for c in rs}
    Ys = {c: halo(Mb, c, grid, part, X) for c in rs}

    def step(blocks, dagger, gamma5):
        return {c: apply_Mc_local(Mb[c], blocks[c], ghost_faces(blocks, c, grid, part, X), Ys[c], X, part, dagger, gamma5, read_index) for c in rs}
    wb = {c: slice_eo(wg, Gc, c, grid) for c in rs}
    if op == cor.OP_M:
        r = step(wb, False, False)
    elif op == cor.OP_MDAG:
        r = step(wb, True, False)
    elif op == cor.OP_H:
        r = step(wb, False, True)
    elif op == cor.OP_MDAGM:
        r = step(step(wb, False, False), True, False)
    else:
        r = step(step(wb, True, False), False, False)
    r = {c: scale * b for c, b in r.items()}
    return r, assemble_eo(r, Gc, grid)


# ---- the global problems of the grid tests (CPU and GPU), from one seed ----------------------------------------------------------------
KAPPA = 0.12
CSW_COEFF = 0.17
NW = 9                                         # coarse vectors: one block of 8 and one more


def global_problem(G, bs, nvec, seed=0):
    """links U_lex [4, T, Z, Y, X, 3, 3], null vectors V_lex [T, Z, Y, X, 4, 3, n_vec] (random, not block-orthonormal) and NW coarse
    vectors w_lex [Tc, Zc, Yc, Xc, 2, n_vec] on the global lattice G"""
    from util import random_gauge_lex
    rng = np.random.default_rng(7700 + seed + nvec + sum(G) + sum(bs))

    def c(shape):
        return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    Gc = tuple(G[d] // bs[d] for d in range(4))
    U_lex = random_gauge_lex(rng, G)
    V_lex = c((G[3], G[2], G[1], G[0], 4, 3, nvec)) / np.sqrt(12.0 * nvec)
    w_lex = [c((Gc[3], Gc[2], Gc[1], Gc[0], 2, nvec)) for _ in range(NW)]
    return U_lex, V_lex, w_lex


def global_reference(G, bs, nvec, clover, seed=0):
    """(the matrices of coarse_op_ref.build on the global lattice, the global coarse vectors, even-odd)"""
    import clover_ref as cr
    U_lex, V_lex, w_lex = global_problem(G, bs, nvec, seed)
    Gc = tuple(G[d] // bs[d] for d in range(4))
    Uo = orc.extended_gauge_from_global(U_lex, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    A = orc.lex_to_eo(cr.clover_dense(U_lex, CSW_COEFF), G) if clover else None
    M = cor.build(orc.lex_to_eo(V_lex, G), Uo, A, KAPPA, G, bs)
    return M, [orc.lex_to_eo(w, Gc) for w in w_lex]
