"""The two-grid preconditioned GCR on a process grid, in numpy (mugiq_hip_mg_solve_grid, mugiq_hip_mg_precondition_grid in
include/mugiq_hip.h): the recurrence of tests/mg_solve_ref.py -- the MR step, GCRfix with one pass of classical Gram-Schmidt, K and the
restarted outer solve -- with every inner product formed per rank block and the parts added in ascending rank order (x slowest, t fastest),
which is what the rank table and mg_rank_sum_kernel do.  The operators act on the global fields: on a grid M, M_c, R and P give the bits of
their single-domain results (tests/test_gpu_coarse_op_grid.py, tests/test_gpu_wilson.py), so only the sums know about the ranks.  Global
problems: coarse_op_grid_ref.global_problem, Wilson-clover; the blocks are cut with coarse_op_grid_ref.slice_eo.  Also the ring gather of
the rank table on a simulated network, from the plan of every rank."""
import functools

import numpy as np

import clover_ref as cr
import coarse_op_grid_ref as gr
import mg_solve_ref as mgr
from util import orc

BS = (2, 2, 2, 2)
NVEC = 8
RHS_SEED = 1


@functools.lru_cache(maxsize=None)
def global_fields(G):
    """(U_lex, V_lex, the clover blocks) on the global lattice G: 2^4 aggregates, n_vec 8, the coefficient of coarse_op_grid_ref"""
    U_lex, V_lex, _ = gr.global_problem(G, BS, NVEC)
    return U_lex, V_lex, cr.clover_blocks_eo(U_lex, gr.CSW_COEFF, G)


@functools.lru_cache(maxsize=None)
def global_problem(G):
    """mg_solve_ref.Problem on those fields with its explicit M_c, at the kappa of coarse_op_grid_ref"""
    U_lex, V_lex, _ = global_fields(G)
    Uo = orc.extended_gauge_from_global(U_lex, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    return mgr.Problem(G, Uo, gr.KAPPA, orc.lex_to_eo(V_lex, G), BS, orc.lex_to_eo(cr.clover_dense(U_lex, gr.CSW_COEFF), G))


@functools.lru_cache(maxsize=None)
def rhs(G, n=1):
    rng = np.random.default_rng(RHS_SEED)
    shape = (2, int(np.prod(G)) // 2, 4, 3)
    return tuple(rng.standard_normal(shape) + 1j * rng.standard_normal(shape) for _ in range(n))


class RankDot:
    """<a, b> of two global even-odd fields (fine [2, volCB, 4, 3] or coarse [2, volCB_c, 2, n_vec]) as the sum, in ascending rank order,
    of the inner products of the rank blocks"""

    def __init__(self, G, grid, bs=BS):
        self.sites = {}
        for L in (tuple(G), tuple(G[d] // bs[d] for d in range(4))):
            vcb = int(np.prod(L)) // 2
            idx = np.arange(2 * vcb).reshape(2, vcb)
            self.sites[vcb] = [gr.slice_eo(idx, L, c, grid).reshape(-1) for c in gr.ranks(grid)]

    def __call__(self, a, b):
        vcb = a.shape[1]
        fa, fb = a.reshape(2 * vcb, -1), b.reshape(2 * vcb, -1)
        total = 0.0
        for s in self.sites[vcb]:
            total = total + np.vdot(fa[s], fb[s])
        return total


def mr_step(M, dot, z, s, omega):
    t = M(s)
    d = dot(t, t).real
    alpha = omega * dot(t, s) / d if d > 0.0 else 0.0
    return z + alpha * s, s - alpha * t


class Directions:
    def __init__(self, dot):
        self.dot, self.p, self.q = dot, [], []

    def step(self, p, q, x, r):
        c = [self.dot(qj, q) for qj in self.q]
        for cj, pj, qj in zip(c, self.p, self.q):
            p = p - cj * pj
            q = q - cj * qj
        nu = np.sqrt(self.dot(q, q).real)
        if nu == 0.0:
            self.p.append(np.zeros_like(p)), self.q.append(np.zeros_like(q))
            return x, r
        p, q = p / nu, q / nu
        self.p.append(p), self.q.append(q)
        alpha = self.dot(q, r)
        return x + alpha * p, r - alpha * q


def gcr_fix(A, dot, b, n):
    x, r, dirs = np.zeros_like(b), b.copy(), Directions(dot)
    for _ in range(n):
        x, r = dirs.step(r, A(r), x, r)
    return x


def K(prob, dot, r, nuPre=0, nuPost=4, omega=1.0, coarseIters=8, **_):
    z, s = np.zeros_like(r), r.copy()
    for _ in range(nuPre):
        z, s = mr_step(prob.M, dot, z, s, omega)
    if coarseIters > 0:
        z = z + prob.P(gcr_fix(prob.A_c, dot, prob.R(s), coarseIters))
        s = r - prob.M(z)
    for _ in range(nuPost):
        z, s = mr_step(prob.M, dot, z, s, omega)
    return z


def solve(prob, dot, b, **param):
    """(x, iterations, history, converged), as mg_solve_ref.solve"""
    p = dict(mgr.DEFAULTS, **param)
    x, r = np.zeros_like(b), b.astype(np.complex128).copy()
    bn2 = dot(b, b).real
    hist, dirs = [], Directions(dot)
    tol2 = p["tol"] ** 2
    if not bn2 > 0.0 or bn2 <= tol2 * bn2:
        return x, 0, np.zeros(0), True
    for it in range(p["maxIter"]):
        z = K(prob, dot, r, **p)
        x, r = dirs.step(z, prob.M(z), x, r)
        rr2 = dot(r, r).real
        hist.append(np.sqrt(rr2 / bn2))
        if rr2 <= tol2 * bn2:
            return x, it + 1, np.array(hist), True
        if len(dirs.p) == p["nKrylov"]:
            dirs = Directions(dot)
    return x, p["maxIter"], np.array(hist), False


# ---- the ring gather of the rank table --------------------------------------------------------------------------------------------------
def rank_of(c, grid):
    return ((c[0] * grid[1] + c[1]) * grid[2] + c[2]) * grid[3] + c[3]


def simulate_gather(grid, plan_of):
    """Runs the plans of all ranks on a network: plan_of(coord) is the list of (dim, sendEntry, recvEntry, entries) of that rank, message m
    of every rank is posted in round m (every rank has the same number of messages), a message goes to the neighbour at +1 along its axis
    and is read at the moment it is posted.  Returns (tables, writes): tables[rank][entry] the rank whose sums the entry holds (-1: never
    filled), writes[rank][entry] how often it was written.  Raises AssertionError where a message reads an entry that holds nothing yet,
    the two ends of a message disagree about it, or an entry goes outside the table."""
    coords = gr.ranks(grid)
    size = len(coords)
    plans = {c: plan_of(c) for c in coords}
    n = len(plans[coords[0]])
    assert all(len(p) == n for p in plans.values())
    tables = {rank_of(c, grid): [-1] * size for c in coords}
    writes = {rank_of(c, grid): [0] * size for c in coords}
    for c in coords:                                        # the local sums: a rank's own entry
        tables[rank_of(c, grid)][rank_of(c, grid)] = rank_of(c, grid)
        writes[rank_of(c, grid)][rank_of(c, grid)] = 1
    for m in range(n):
        sent = {}
        for c in coords:
            dim, s, _, cnt = plans[c][m]
            assert grid[dim] > 1 and 0 <= s and s + cnt <= size
            payload = tables[rank_of(c, grid)][s:s + cnt]
            assert all(e >= 0 for e in payload), ("a message reads an entry before it was filled", c, m)
            sent[gr.neighbour(c, grid, dim, +1)] = (dim, cnt, payload)
        for c in coords:
            dim, _, r, cnt = plans[c][m]
            got = sent[c]
            assert got[0] == dim and got[1] == cnt and 0 <= r and r + cnt <= size, (c, m)
            me = rank_of(c, grid)
            tables[me][r:r + cnt] = got[2]
            for e in range(r, r + cnt):
                writes[me][e] += 1
    return tables, writes
