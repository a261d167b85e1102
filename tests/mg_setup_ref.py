"""numpy restatement of the MG setup (mugiq_hip_block_orthonormalize, mugiq_hip_transfer_orthonormality and mugiq_hip_mg_setup in
include/mugiq_hip.h), written from the contracts there: classical Gram-Schmidt per (aggregate, coarse spin) block with every coefficient
of a column taken from the un-updated column, repeated nPasses times; the null-vector recipe v = start - CG(M start); packing; refinement
by the two-grid solve.  The operators, the CG and the solve are the tests' own (wilson_ref, clover_ref, mg_solve_ref).  It shares no code with the
product, and its blocks are gathered with the oracle's aggregate map, not with the kernel's site table."""
import numpy as np

import clover_ref as cr
import mg_solve_ref as mgr
import wilson_ref as wr
from util import orc


# ---- blocks -------------------------------------------------------------------------------------------------------------------------
def _site_order(X, bs):
    """[nAgg, aggVol] indices into the flattened (parity, x_cb) axis: the sites of every aggregate"""
    cp, cx = orc.fine_to_coarse_map(X, bs)
    vcbc = int(np.prod([X[d] // bs[d] for d in range(4)])) // 2
    agg = (cp * vcbc + cx).reshape(-1)
    return np.argsort(agg, kind="stable").reshape(2 * vcbc, -1)


def to_blocks(V, X, bs, spin_bs=2):
    """V [2, volCB, ns, nc, n_vec] -> B [nAgg, ns / spin_bs, m, n_vec], m = aggVol spin_bs nc"""
    ns, nc, nvec = V.shape[2:]
    order = _site_order(X, bs)
    flat = np.asarray(V).reshape(-1, ns // spin_bs, spin_bs, nc, nvec)[order]        # [nAgg, aggVol, S, sb, nc, n]
    return np.moveaxis(flat, 2, 1).reshape(order.shape[0], ns // spin_bs, -1, nvec)


def from_blocks(B, X, bs, shape, spin_bs=2):
    ns, nc, nvec = shape[2:]
    order = _site_order(X, bs)
    flat = np.moveaxis(B.reshape(order.shape[0], ns // spin_bs, order.shape[1], spin_bs, nc, nvec), 1, 2)
    out = np.zeros((shape[0] * shape[1], ns // spin_bs, spin_bs, nc, nvec), dtype=B.dtype)
    out[order] = flat
    return out.reshape(shape)


def cgs(B, nPasses):
    """The contract on a batch of blocks B [..., m, n]: (Q, minPivotRatio, zeroColumns).  For pass < nPasses, for j: c_i = <q_i, b_j> for
    all i < j from the un-updated b_j; b_j -= sum c_i q_i; nu_j = ||b_j||; q_j = b_j / nu_j, exact zeros (and counted) for nu_j = 0."""
    Q = np.array(B, dtype=np.complex128)
    n = Q.shape[-1]
    ratio, zeros = np.inf, 0
    for p in range(nPasses):
        zeros = 0
        for j in range(n):
            b = Q[..., :, j]
            given = np.sqrt(np.sum(np.abs(b) ** 2, axis=-1))
            c = np.einsum("...mi,...m->...i", np.conj(Q[..., :, :j]), b)
            b = b - np.einsum("...mi,...i->...m", Q[..., :, :j], c)
            nu = np.sqrt(np.sum(np.abs(b) ** 2, axis=-1))
            ok = nu > 0.0
            Q[..., :, j] = np.where(ok[..., None], b / np.where(ok, nu, 1.0)[..., None], 0.0)
            zeros += int(np.sum(~ok))
            if p == 0:
                r = np.where(given > 0.0, nu / np.where(given > 0.0, given, 1.0), 0.0)
                ratio = min(ratio, float(np.min(r)))
    return Q, ratio, zeros


def qr_positive(B):
    """Q of numpy's thin QR with the diagonal of R made positive real: what the contract's result is in exact arithmetic"""
    q, r = np.linalg.qr(B)
    d = np.diagonal(r, axis1=-2, axis2=-1)
    return q * (d / np.abs(d))[..., None, :]


def gram_deviation(B):
    """max over the blocks and entries of |B^dag B - 1|"""
    G = np.einsum("...mi,...mj->...ij", np.conj(B), B)
    return float(np.max(np.abs(G - np.eye(B.shape[-1]))))


def block_orthonormalize(V, X, bs, spin_bs=2, nPasses=2):
    """(V', minPivotRatio, zeroColumns) of the contract on V [2, volCB, ns, nc, n_vec]"""
    Q, ratio, zeros = cgs(to_blocks(V, X, bs, spin_bs), nPasses)
    return from_blocks(Q, X, bs, np.shape(V), spin_bs), ratio, zeros


def orthonormality(V, X, bs, spin_bs=2):
    return gram_deviation(to_blocks(V, X, bs, spin_bs))


# ---- null vectors and the driver ----------------------------------------------------------------------------------------------------
def null_vector(M, Mdag, start, setupTol, setupMaxIter):
    """(v, CG iterations): b = M start, e = CG on the normal equations stopped at setupMaxIter or setupTol, v = start - e"""
    e, it = wr.cg_normal(M, Mdag, M(start), setupTol, setupMaxIter)
    return start - e, it


def pack(vectors):
    """V [2, volCB, 4, 3, n_vec] with V[..., j] = vectors[j]"""
    return np.stack(vectors, axis=-1)


def setup(X, Uo, kappa, bs, starts, setupMaxIter=500, setupTol=5e-6, nBlockOrtho=2, refineCycles=0, refineIters=4, A_eo=None):
    """(V, [CG iterations], minPivotRatio of the last orthonormalisation) of mugiq_hip_mg_setup.  A_eo [2, volCB, 12, 12]: the clover term,
    which then stands in M and M^dag of the null-vector CG, in the coarse operator and in the M of the refinement solve."""
    def M(v):
        return wr.wilson_M(v, Uo, kappa, X) if A_eo is None else cr.clover_M(v, Uo, A_eo, kappa, X)

    def Mdag(v):
        return wr.wilson_M(v, Uo, kappa, X, dagger=True) if A_eo is None else cr.clover_M(v, Uo, A_eo, kappa, X, dagger=True)

    vs, its = [], []
    for s in starts:
        v, it = null_vector(M, Mdag, np.asarray(s, dtype=np.complex128), setupTol, setupMaxIter)
        vs.append(v), its.append(it)
    V, ratio, _ = block_orthonormalize(pack(vs), X, bs, 2, nBlockOrtho)
    for _ in range(refineCycles):
        prob = mgr.Problem(X, Uo, kappa, V, bs, A_eo)
        vs = [v - mgr.solve(prob, M(v), tol=setupTol, maxIter=refineIters, nKrylov=refineIters)[0] for v in vs]
        V, ratio, _ = block_orthonormalize(pack(vs), X, bs, 2, nBlockOrtho)
    return V, its, ratio
