"""numpy reference of the restriction R = P^dag (QUDA Transfer::R), written directly from its formula
    coarse(X; S, j) = sum_{x in aggregate X} sum_{s: s / spin_bs = S} sum_c conj(V(x; s, c, j)) g(s) fine(x; s, c),   g = 1 | diag(g5),
on the logical layouts of oracle/mugiq_oracle.py (orc.prolongate is its adjoint), and block-orthonormal null vectors for the tests."""
import numpy as np

from util import orc

G5 = np.diag(orc.gamma_dense(15)).real          # diag(+1, +1, -1, -1) in the DeGrand-Rossi table


def restrict(fine, V, X, geo_bs=(4, 4, 4, 4), spin_bs=2, gamma5=False):
    """fine[2, volCB, nSpin_f, nColor_f], V[2, volCB, nSpin_f, nColor_f, n_vec] -> coarse[2, volCB_c, nSpin_f / spin_bs, n_vec].
    Finest level: nSpin_f 4, nColor_f 3, spin_bs 2.  Coarse -> coarse levels: nSpin_f 2, spin_bs 1 (gamma5 applies to the finest only)."""
    ns, nvec = V.shape[2], V.shape[-1]
    assert not gamma5 or ns == 4
    cp, cx = orc.fine_to_coarse_map(X, geo_bs)
    vcbc = int(np.prod([X[d] // geo_bs[d] for d in range(4)])) // 2
    out = np.zeros((2, vcbc, ns // spin_bs, nvec), dtype=np.complex128)
    for pty in range(2):
        for s in range(ns):
            g = G5[s] if gamma5 else 1.0
            term = np.einsum("xcj,xc->xj", np.conj(V[pty, :, s]), g * fine[pty, :, s])
            np.add.at(out[:, :, s // spin_bs, :], (cp[pty], cx[pty]), term)
    return out


def restrict_levels(fine, Vs, Xs, geo_bss, gamma5=False):
    """R through a hierarchy (the adjoint of orc.prolongate_levels): Vs[0] is the finest transfer."""
    v = restrict(fine, Vs[0], Xs[0], geo_bss[0], 2, gamma5)
    for l in range(1, len(Vs)):
        v = restrict(v, Vs[l], Xs[l], geo_bss[l], 1)
    return v


def block_orthonormal(V, X, geo_bs, spin_bs=2):
    """V with orthonormal columns j inside every (aggregate, coarse spin) block, by QR: then restrict(prolongate(phi)) = phi."""
    ns, nc, nvec = V.shape[2], V.shape[3], V.shape[4]
    cp, cx = orc.fine_to_coarse_map(X, geo_bs)
    vcbc = int(np.prod([X[d] // geo_bs[d] for d in range(4)])) // 2
    agg = (cp * vcbc + cx).reshape(-1)                                   # aggregate of every (parity, x_cb)
    out = np.array(V, dtype=np.complex128)
    flat = out.reshape(-1, ns, nc, nvec)                                 # a view: [2 * volCB, ...]
    for a in range(2 * vcbc):
        sites = np.nonzero(agg == a)[0]
        for S in range(ns // spin_bs):
            blk = flat[sites][:, S * spin_bs:(S + 1) * spin_bs].reshape(-1, nvec)
            assert blk.shape[0] >= nvec
            q, _ = np.linalg.qr(blk)
            flat[sites[:, None], np.arange(S * spin_bs, (S + 1) * spin_bs)[None, :]] = q.reshape(len(sites), spin_bs, nc, nvec)
    return out
