"""numpy model of the mixed-precision two-grid solve (mugiq_hip_mg_precondition_sloppy, mugiq_hip_mg_solve_mixed in include/mugiq_hip.h): the K
and the outer solve of tests/mg_solve_ref.py with V, M_c and every vector the device stores inside K rounded to complex64 at the store, and
all arithmetic in fp64 -- the rule of the device's Krylov kernels (loads widen, products and sums in fp64, one rounding on each store, scalars
in fp64).  The outer solve is mg_solve_ref.solve with p = K32(round(r)).

This is a MODEL, not a bit pin: the device's stencil computes in fp32, while here M is applied in fp64 and rounded once; and the device
sums in another order.  What the device is held to against it is therefore a bound derived from the model's own sensitivity to 1-ulp (fp32)
perturbations of its input (tests/test_mg_solve_mixed_cpu.py measures it, tests/test_gpu_mg_solve_mixed.py uses it), never equality.

The rounding points follow csrc/mg_solve.hip step by step: in a GCR step the norm nu and <q, r> are taken from the orthogonalised q before
it is stored, x and r are updated with the normalised p and q before they are stored, and the later steps read the stored ones."""
import numpy as np

import coarse_op_ref as cor
import mg_solve_ref as mgr


def rd(a):
    """one rounding to fp32 storage (round to nearest even), back in fp64"""
    return np.asarray(a).astype(np.complex64).astype(np.complex128)


def ulp32_perturbed(v, seed):
    """v (complex, fp32-representable or not) rounded to fp32 with every real number then moved by at most one fp32 ulp, seeded: the
    manner of mg_solve_ref.ulp_perturbed at the storage precision of the cycle"""
    rng = np.random.default_rng(seed)
    f = np.asarray(v).astype(np.complex64).view(np.float32)
    step = rng.integers(-1, 2, size=f.shape)
    up, dn = np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))
    return np.where(step > 0, up, np.where(step < 0, dn, f)).view(np.complex64).reshape(np.shape(v)).astype(np.complex128)


class SloppyProblem:
    """The hierarchy of an mg_solve_ref.Problem (or ChainProblem) in fp32 storage: V rounded, and M_c BUILT FROM THE ROUNDED V and then
    rounded, as the device builds it (Transfer.astype(4), computeCoarseOperator).  M stays the fp64 operator: gauge and clover fields are
    either precision on the device, and the model's M is exact arithmetic anyway."""

    def __init__(self, prob):
        self.X, self.Uo, self.kappa, self.bs, self.A_eo, self.Xc = prob.X, prob.Uo, prob.kappa, prob.bs, prob.A_eo, prob.Xc
        self.V = rd(prob.V)
        self.M = prob.M
        inner = mgr.ChainProblem(prob.X, prob.Uo, prob.kappa, self.V, prob.bs, prob.A_eo)
        self.R, self.P = inner.R, inner.P
        if prob.Mc is None:
            self.Mc, self.A_c = None, inner.A_c
        else:
            self.Mc = rd(cor.build(self.V, prob.Uo, prob.A_eo, prob.kappa, prob.X, prob.bs))
            self.A_c = lambda w: cor.apply_Mc(self.Mc, w, self.Xc)


def mr_step(M, z, s, omega, last):
    """(z, s) after one MR step; z None: z = 0 is not stored yet.  last: s is not needed again and not written"""
    t = rd(M(s))
    d = np.vdot(t, t).real
    alpha = omega * np.vdot(t, s) / d if d > 0.0 else 0.0
    z = rd(alpha * s) if z is None else rd(z + alpha * s)
    return z, (None if last else rd(s - alpha * t))


def gcr_fix(A, b, n):
    """GCRfix of mg_solve_ref with the stores of the device: b is used up as r"""
    x, r = None, b
    ps, qs = [], []
    p = r
    for k in range(n):
        q = rd(A(p))
        if k > 0:
            c = [np.vdot(qj, q) for qj in qs]
            for cj, pj, qj in zip(c, ps, qs):
                p = p - cj * pj
                q = q - cj * qj
            nu = np.sqrt(np.vdot(q, q).real)                   # from the orthogonalised q before its store
            qr = np.vdot(q, r)
            p, q = rd(p), rd(q)
        else:
            nu = np.sqrt(np.vdot(q, q).real)
            qr = np.vdot(q, r)
        if nu > 0.0:
            alpha = qr / nu
            p, q = p / nu, q / nu                              # x and r take these before they are rounded
        else:
            alpha = 0.0
            p, q = np.zeros_like(p), np.zeros_like(q)
        x = rd(alpha * p) if x is None else rd(x + alpha * p)
        r = rd(r - alpha * q)
        ps.append(rd(p)), qs.append(rd(q))
        p = r
    return x


def K(sp, r, nuPre=0, nuPost=4, omega=1.0, coarseIters=8, **_):
    """K32(r) on a SloppyProblem: r is rounded first (the hand-over of the mixed solve; a no-op for an fp32 input)"""
    r = rd(r)
    z, s = None, r
    coarse = coarseIters > 0
    for i in range(nuPre):
        z, s_new = mr_step(sp.M, z, s, omega, not coarse and nuPost == 0 and i == nuPre - 1)
        s = s if s_new is None else s_new
    if coarse:
        w = rd(sp.P(gcr_fix(sp.A_c, rd(sp.R(s)), coarseIters)))
        z = w if z is None else rd(z + w)
        if nuPost > 0:
            s = rd(r - rd(sp.M(z)))
    for i in range(nuPost):
        z, s_new = mr_step(sp.M, z, s, omega, i == nuPost - 1)
        s = s if s_new is None else s_new
    return np.zeros_like(r) if z is None else z


def solve(prob, b, sp=None, **param):
    """(x, iterations, history, converged) of the mixed solve for one right-hand side: mg_solve_ref.solve on the fp64 problem `prob`
    with p = K32(round(r)) on SloppyProblem(prob) (sp: that object, if the caller keeps one)"""
    sp = SloppyProblem(prob) if sp is None else sp
    p = dict(mgr.DEFAULTS, **param)
    x, r = np.zeros_like(b), b.astype(np.complex128).copy()
    bn2 = np.vdot(b, b).real
    hist, dirs = [], mgr.Directions()
    tol2 = p["tol"] ** 2
    if not bn2 > 0.0 or bn2 <= tol2 * bn2:
        return x, 0, np.zeros(0), True
    for it in range(p["maxIter"]):
        z = K(sp, r, **p)
        x, r = dirs.step(z, prob.M(z), x, r)
        rr2 = np.vdot(r, r).real
        hist.append(np.sqrt(rr2 / bn2))
        if rr2 <= tol2 * bn2:
            return x, it + 1, np.array(hist), True
        if len(dirs.p) == p["nKrylov"]:
            dirs = mgr.Directions()
    return x, p["maxIter"], np.array(hist), False
