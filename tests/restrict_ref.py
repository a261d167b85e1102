"""numpy reference of the restriction R = P^dag (QUDA Transfer::R), written directly from its formula
    coarse(X; S, j) = sum_{x in aggregate X} sum_{s: s / spin_bs = S} sum_c conj(V(x; s, c, j)) g(s) fine(x; s, c),   g = 1 | diag(g5),
on the logical layouts of oracle/mugiq_oracle.py (orc.prolongate is its adjoint), block-orthonormal null vectors for the tests, and the
Galerkin operator R [g5] M P with the eigenpair check built on it."""
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


# ---- the Galerkin operator of the eigenpair check on the coarsest level --------------------------------------------------------
def galerkin_apply(w, Vs, Xs, geo_bss, Uo, A_eo, kappa, dagger=False, gamma5=False, scale=1.0, stored=None):
    """scale R [g5] M^(dag) P w through the hierarchy Vs / Xs / geo_bss (finest first; w lives on level len(Vs)): orc.prolongate_levels up,
    the numpy Wilson(-clover) operator (A_eo None: Wilson), restrict down, one level at a time.  stored: None, or the rounding of a
    storage step (the library keeps the vector after every P, after the stencil -- its scale folded in -- and after every R); the
    prolongation then goes level by level with orc.prolongate, which is what orc.prolongate_levels composes."""
    import clover_ref as cr
    import wilson_ref as wr
    if stored is None:
        f = orc.prolongate_levels(w, Vs, Xs, geo_bss)
    else:
        f = w
        for l in range(len(Vs) - 1, -1, -1):
            f = stored(orc.prolongate(f, Vs[l], Xs[l], geo_bss[l], 2 if l == 0 else 1))
    f = cr.clover_M(f, Uo, A_eo, kappa, Xs[0], dagger=dagger) if A_eo is not None else wr.wilson_M(f, Uo, kappa, Xs[0], dagger=dagger)
    f = scale * f
    if stored is not None:
        f = stored(f)
    for l in range(len(Vs)):
        f = restrict(f, Vs[l], Xs[l], geo_bss[l], 2 if l == 0 else 1, gamma5 and l == 0)
        if stored is not None:
            f = stored(f)
    return f


def coarse_evals_reference(ws, Vs, Xs, geo_bss, Uo, A_eo, kappa, op, scale, stored=None):
    """lambda, r, sigma of Eigsolve_Mugiq::computeEvals for the eigenvectors ws on the coarsest level of a hierarchy of len(Vs) levels:
    M_c = R M P, M_c^dag = R M^dag P, MdagM = M_c^dag M_c, MMdag = M_c M_c^dag, H = R g5 M P; lambda = w^dag A_c w / ||w||,
    r = ||lambda w - A_c w||, sigma = sqrt(Re lambda) for the normal forms and Re lambda for H.  The scale multiplies the last
    operator application, as in the library."""
    def Mc(w, dagger=False, gamma5=False, s=1.0):
        return galerkin_apply(w, Vs, Xs, geo_bss, Uo, A_eo, kappa, dagger, gamma5, s, stored)
    lam, res = [], []
    for w in ws:
        y = {0: lambda: Mc(w, s=scale), 1: lambda: Mc(w, True, s=scale), 2: lambda: Mc(Mc(w), True, s=scale), 3: lambda: Mc(Mc(w, True), s=scale),
             4: lambda: Mc(w, gamma5=True, s=scale)}[op]()
        l = np.vdot(w, y) / np.linalg.norm(w)
        lam.append(l)
        res.append(np.linalg.norm(l * w - y))
    lam, res = np.array(lam), np.array(res)
    sig = np.sqrt(lam.real) if op in (2, 3) else lam.real if op == 4 else None
    return lam, res, sig
