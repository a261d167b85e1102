"""Time the deflated coarsest solve (csrc/mg_deflate.hip, the *_levels_deflated entry points) on the fields of tools/bench_mg_solve3.py:

    python tools/bench_mg_deflate.py [--lattice 32 32 32 32] [--block 4 4 4 4] [--nvec 24] [--block1 2 2 2 2] [--nvec1 32] [--nrhs 8]
                                     [--nev 200] [--out profiles/mg_deflate_latest.json]

Random unitary links, Wilson-clover, V_0 from mgSetup on Gaussian start vectors (seed 13), the second level from mgSetupCoarse; the
deflation vectors are coarseEigensolve's on level 1 and on level 2.  Measured, medians after a warm-up with the compared routes alternated
in the same loop and device events around every loop:
  (a) the projection (overlaps + combination, coarseDeflate on a block of right-hand sides) at level 1 with 64 and with --nev vectors and at
      level 2 with --nev vectors; against the bytes it must move (U once, then W and U once, the right-hand sides three times) at the rate
      the read probe reaches in the same run; and against TWO coarseApply calls (M and Mdag) on the same operator, the cost of the route
      that stores no U (x0 = W Theta^-1 W^dag A^dag b, r0 = b - A x0);
  (b) one cycle and the whole solve (iterations, time) for the two-grid and the three-level hierarchy: coarseIters 8 on the last level
      undeflated (the struct default) against coarseIters 1, 2 and 4 deflated.
The CG's iteration count is the measure of how well conditioned the configuration is.  One JSON record is printed and written to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mugiq_amd as hip  # noqa: E402
from bench_mg_solve import batched_q  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", type=int, nargs=4, default=[32, 32, 32, 32])
    ap.add_argument("--block", type=int, nargs=4, default=[4, 4, 4, 4])
    ap.add_argument("--nvec", type=int, default=24)
    ap.add_argument("--block1", type=int, nargs=4, default=[2, 2, 2, 2])
    ap.add_argument("--nvec1", type=int, default=32)
    ap.add_argument("--nrhs", type=int, default=8)
    ap.add_argument("--nev", type=int, default=200)
    ap.add_argument("--nkr", type=int, default=256)
    ap.add_argument("--eig-tol", type=float, default=1e-8)
    ap.add_argument("--kappa", type=float, default=0.124)
    ap.add_argument("--csw-coeff", type=float, default=0.1)
    ap.add_argument("--setup-iters", type=int, default=50)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--max-iter", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mg_deflate_latest.json"))
    a = ap.parse_args()
    X, bs, bs1 = tuple(a.lattice), tuple(a.block), tuple(a.block1)
    torch.cuda.set_device(0)
    gen = torch.Generator(device="cuda").manual_seed(12)
    vcb = int(np.prod(X)) // 2

    def crandn(*shape):
        return torch.randn(*shape, dtype=torch.complex128, device="cuda", generator=gen)

    def wall_ms(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t)

    def event_ms(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    def alternated(routes, loops, reps, warmup):
        times = {k: [] for k in routes}
        for it in range(warmup + reps):
            for k in routes:
                ms = event_ms(routes[k], loops)
                if it >= warmup:
                    times[k].append(ms)
        return times

    # ---- the hierarchy and its eigenvectors
    gauge = hip.GaugeField(X, (0, 0, 0, 0), 8)
    U = batched_q(crandn(8 * vcb, 3, 3)).reshape(2, 4, vcb, 3, 3)
    gauge.data.view(2, 4, 9, vcb).copy_(U.reshape(2, 4, vcb, 9).permute(0, 1, 3, 2))
    del U
    C = hip.CloverField(X, 8).compute(gauge, a.csw_coeff)
    vecs = hip.mgStartVectors(X, a.nvec, seed=13)
    T0, op1, _ = hip.mgSetup(gauge, a.kappa, a.nvec, bs, start=vecs, clover=C, setupMaxIter=a.setup_iters)
    del vecs
    T1, op2, _ = hip.mgSetupCoarse(op1, a.nvec1, bs1, seed=21)
    torch.cuda.empty_cache()
    eig = {}
    spaces = {}
    for level, op in ((1, op1), (2, op2)):
        t0 = time.perf_counter()
        ev, theta, res, _, einfo = hip.coarseEigensolve(op, hip.MUGIQ_EIG_OPERATOR_MdagM, seed=31 + level, nConv=a.nev, nKr=a.nkr, tol=a.eig_tol)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        spaces[(level, a.nev)] = hip.CoarseDeflation(ev, op)
        torch.cuda.synchronize()
        eig[level] = {"eigensolve_s": round(t1 - t0, 2), "build_U_s": round(time.perf_counter() - t1, 3), "iters": einfo.iters,
                      "theta_min": float(theta[0]), "theta_max": float(theta[-1]), "residual_max": float(np.max(res)),
                      "sigma_vs_sqrt_theta_max": float(np.max(np.abs(spaces[(level, a.nev)].sigma - np.sqrt(theta)) / np.sqrt(theta)))}
    n64 = min(64, a.nev)
    spaces[(1, n64)] = hip.CoarseDeflation(spaces[(1, a.nev)].W[:n64], op1)

    # ---- (a) the projection against the bytes and against two applications
    probe = torch.empty(1 << 27, dtype=torch.complex128, device="cuda")     # 2 GiB, streamed once per call
    probe.zero_()
    routes, model = {"read_probe": lambda: hip.probeReadBandwidth(probe)}, {}
    for (level, nEv), D in sorted(spaces.items()):
        op = op1 if level == 1 else op2
        cb = [hip.CoarseField(op.X, op.n_vec, 8) for _ in range(a.nrhs)]
        for f in cb:
            f.data.copy_(crandn(f.data.numel()))
        cx, cr = [hip.CoarseField(op.X, op.n_vec, 8) for _ in cb], [hip.CoarseField(op.X, op.n_vec, 8) for _ in cb]
        routes["project_l%d_%d" % (level, nEv)] = lambda cb=cb, cx=cx, cr=cr, D=D: hip.coarseDeflate(cb, D, x0=cx, r0=cr)
        vec = cb[0].data.numel() * 16
        model["project_l%d_%d" % (level, nEv)] = {"vector_MB": round(vec / 1e6, 3), "bytes_min": 3 * nEv * vec + 4 * a.nrhs * vec}
        if nEv == a.nev:
            def two(cb=cb, cx=cx, cr=cr, op=op):
                hip.coarseApply(cx, cb, op, hip.MUGIQ_EIG_OPERATOR_Mdag)
                hip.coarseApply(cr, cx, op, hip.MUGIQ_EIG_OPERATOR_M)
            routes["two_applies_l%d" % level] = two
    pt = alternated(routes, 20, 2 * a.reps, a.warmup)
    med = {k: float(np.median(v)) for k, v in pt.items()}
    probe_GBs = probe.numel() * 16 / 1e6 / med["read_probe"]
    for k, m in model.items():
        m["ms"] = round(med[k], 4)
        m["ms_min"] = round(float(np.min(pt[k])), 4)
        m["ms_at_probe_rate"] = round(m["bytes_min"] / 1e6 / probe_GBs, 4)
        m["fraction_of_probe_rate"] = round(m["ms_at_probe_rate"] / med[k], 3)
        m["over_two_applies"] = round(med[k] / med["two_applies_l%s" % k.split("_")[1][1:]], 3)
    del probe
    torch.cuda.empty_cache()

    # ---- (b) one cycle and the whole solve
    def random_fields(n):
        out = []
        for _ in range(n):
            f = hip.SpinorField(X, 8, 2)
            f.data.copy_(crandn(f.data.numel()))
            out.append(f)
        return out
    b = random_fields(a.nrhs)
    z = [hip.SpinorField(X, 8, 2) for _ in b]
    x = [hip.SpinorField(X, 8, 2) for _ in b]
    D1, D2 = spaces[(1, a.nev)], spaces[(2, a.nev)]
    cases = {"two_grid_undeflated_8": dict(T=T0, op=op1, D=None, kw=dict(coarseIters=8)),
             "three_level_undeflated_8": dict(T=[T0, T1], op=[op1, op2], D=None, kw=dict(coarseParam=dict(nuPost=2, coarseIters=8)))}
    for c in (1, 2, 4):
        cases["two_grid_deflated_%d" % c] = dict(T=T0, op=op1, D=D1, kw=dict(coarseIters=c))
        cases["three_level_deflated_%d" % c] = dict(T=[T0, T1], op=[op1, op2], D=D2, kw=dict(coarseParam=dict(nuPost=2, coarseIters=c)))
    cyc = {k: (lambda c=c: hip.mgPrecondition(z, b, gauge, a.kappa, c["T"], c["op"], clover=C, deflation=c["D"], **c["kw"])) for k, c in cases.items()}
    ct = alternated(cyc, 3, 2 * a.reps, a.warmup)
    info = {}

    def keep(name, r):
        info[name] = r[1]
    sol = {k: (lambda k=k, c=c: keep(k, hip.mgSolve(b, gauge, a.kappa, c["T"], c["op"], clover=C, x=x, deflation=c["D"], tol=a.tol, maxIter=a.max_iter,
                                                   allow_unconverged=True, **c["kw"]))) for k, c in cases.items()}
    sol["cg"] = lambda: keep("cg", hip.wilsonSolve(b, gauge, a.kappa, tol=a.tol, maxIter=20 * a.max_iter, x=x, allow_unconverged=True, clover=C))
    st = {k: [] for k in sol}
    for it in range(a.warmup + a.reps):
        for k in sol:
            ms = wall_ms(sol[k])
            if it >= a.warmup:
                st[k].append(ms)

    rec = {"workload": "deflated coarsest solve, %s fp64, aggregates %s n_vec %d then %s n_vec %d, %d right-hand sides, Wilson-clover kappa %g, random "
                       "unitary links, V_0 from mgSetup (setupMaxIter %d), V_1 from mgSetupCoarse, %d vectors per level from coarseEigensolve (tol %g)"
                       % ("x".join(map(str, X)), "x".join(map(str, bs)), a.nvec, "x".join(map(str, bs1)), a.nvec1, a.nrhs, a.kappa, a.setup_iters, a.nev,
                          a.eig_tol),
           "reps": a.reps, "warmup": a.warmup, "level1_lattice": list(op1.X), "coarsest_lattice": list(op2.X), "eigensolves": eig,
           "read_probe_GBs": round(probe_GBs, 1), "projection": model,
           "two_applies_ms": {k: round(v, 4) for k, v in med.items() if k.startswith("two_applies")},
           "cycle_ms": {k: round(float(np.median(v)), 3) for k, v in ct.items()},
           "solve_ms": {k: round(float(np.median(v)), 3) for k, v in st.items()},
           "solves": {k: {"iters": [int(n) for n in i.iters], "relres_max": float(np.max(i.relres)), "converged": bool(i.converged),
                          "hostReads": getattr(i, "hostReads", None)} for k, i in info.items()}}
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
