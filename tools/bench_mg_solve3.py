"""Time the three-level solve (mugiq_hip_mg_solve_levels: the K-cycle through the coarsest operator) against the two-grid solve and the
plain CG, and the forms of the coarse application, in one run:

    python tools/bench_mg_solve3.py [--lattice 32 32 32 32] [--block 4 4 4 4] [--nvec 24] [--block1 2 2 2 2] [--nvec1 32] [--nrhs 8]
                                    [--out profiles/mg_solve3_latest.json]

The configuration is that of tools/bench_coarse_op2.py: random unitary links, Wilson-clover, V_0 from mgSetup on Gaussian start vectors
(seed 13), the second level from mgSetupCoarse; the fp32 hierarchy is made from it on the device.  Measured, medians after a warm-up with
the compared routes alternated in the same loop:
  (a) one K against one K^(3) on the block of right-hand sides, at params[1] = (nuPost 2, coarseIters 4) and at the struct defaults, in
      fp64 and in fp32 storage (device events around loops of 5);
  (b) the operator launches of K^(3) alone -- stencil, R_0, P_0, M_1, R_1, P_1, M_2 -- as counts x times: K^(3) minus their sum is what the
      Krylov kernels and the gaps between launches take;
  (c) mgSolve (two-grid), the three-level solve and the CG on the same right-hand sides and tolerance, and the mixed pair: time, iterations,
      hostReads (host clock around calls that end in a synchronise);
  (d) coarse_apply_kernel with 16, 32 and 64 outputs per workgroup (MUGIQ_HIP_COARSE_APPLY_OUT) on M_1, on M_2 and on random operators
      of the workgroup counts between them: median, minimum and maximum of every form, so that a difference can be held against the spread.
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

FORM_ENV = "MUGIQ_HIP_COARSE_APPLY_OUT"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", type=int, nargs=4, default=[32, 32, 32, 32])
    ap.add_argument("--block", type=int, nargs=4, default=[4, 4, 4, 4])
    ap.add_argument("--nvec", type=int, default=24)
    ap.add_argument("--block1", type=int, nargs=4, default=[2, 2, 2, 2])
    ap.add_argument("--nvec1", type=int, default=32)
    ap.add_argument("--nrhs", type=int, default=8)
    ap.add_argument("--kappa", type=float, default=0.124)
    ap.add_argument("--csw-coeff", type=float, default=0.1)
    ap.add_argument("--setup-iters", type=int, default=50)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--max-iter", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--forms-only", action="store_true", help="measure (d) alone, on random operators")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mg_solve3_latest.json"))
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
                ms = event_ms(routes[k], loops[k] if isinstance(loops, dict) else loops)
                if it >= warmup:
                    times[k].append(ms)
        return times

    # ---- (d) the forms of the coarse application
    def random_operator(Xc, nvec):
        op = hip.CoarseOperator(Xc, nvec, 8)
        op.data.copy_(crandn(op.data.numel()) / np.sqrt(4.0 * nvec))
        return op

    def forms(op, label):
        src = [hip.CoarseField(op.X, op.n_vec, 8) for _ in range(8)]
        dst = [hip.CoarseField(op.X, op.n_vec, 8) for _ in range(8)]
        for f in src:
            f.data.copy_(crandn(f.data.numel()))

        def route(out):
            def run():
                os.environ[FORM_ENV] = out
                hip.coarseApply(dst, src, op, hip.MUGIQ_EIG_OPERATOR_M)
            return run
        t = alternated({o: route(o) for o in ("64", "32", "16")}, 40, 3 * a.reps, a.warmup)
        os.environ.pop(FORM_ENV, None)
        N = 2 * op.n_vec
        return {"shape": label, "lattice": list(op.X), "N": N, "workgroups_64": 2 * op.volumeCB * ((N + 63) // 64),
                "operator_MB": round(op.data.numel() * 16 / 1e6, 1),
                "ms": {o: {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)} for o, v in t.items()}}

    between = [((4, 4, 4, 6), 32), ((4, 4, 4, 8), 32), ((4, 4, 8, 8), 32), ((4, 8, 8, 8), 32)]   # 384, 512, 1024 and 2048 workgroups of 64 outputs, N = 64
    if a.forms_only:
        rec = {"apply_forms": [forms(random_operator((4, 4, 4, 4), 32), "4^4, N = 64 (random)")] +
                              [forms(random_operator(Xc, nv), "between (random)") for Xc, nv in between] +
                              [forms(random_operator((8, 8, 8, 8), 24), "8^4, N = 48 (random)")]}
        print(json.dumps(rec))
        return

    # ---- the hierarchy
    gauge = hip.GaugeField(X, (0, 0, 0, 0), 8)
    U = batched_q(crandn(8 * vcb, 3, 3)).reshape(2, 4, vcb, 3, 3)
    gauge.data.view(2, 4, 9, vcb).copy_(U.reshape(2, 4, vcb, 9).permute(0, 1, 3, 2))
    del U
    C = hip.CloverField(X, 8).compute(gauge, a.csw_coeff)
    t0 = time.perf_counter()
    vecs = hip.mgStartVectors(X, a.nvec, seed=13)
    T0, op1, _ = hip.mgSetup(gauge, a.kappa, a.nvec, bs, start=vecs, clover=C, setupMaxIter=a.setup_iters)
    del vecs
    T1, op2, _ = hip.mgSetupCoarse(op1, a.nvec1, bs1, seed=21)
    T0s, T1s = T0.astype(4), T1.astype(4)
    op1s = hip.computeCoarseOperator(T0s, gauge, a.kappa, clover=C)
    op2s = hip.computeCoarseOperatorCoarse(T1s, op1s)
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t0
    torch.cuda.empty_cache()
    Ts, ops, Tss, opss = [T0, T1], [op1, op2], [T0s, T1s], [op1s, op2s]

    def random_fields(n, prec=8):
        out = []
        for _ in range(n):
            f = hip.SpinorField(X, prec, 2)
            f.data.copy_(crandn(f.data.numel()).to(f.data.dtype))
            out.append(f)
        return out
    b = random_fields(a.nrhs)
    b32 = [hip.SpinorField(X, 4, 2) for _ in b]
    hip.mgConvertPrecision(b32, b)
    z64, z32 = [hip.SpinorField(X, 8, 2) for _ in b], [hip.SpinorField(X, 4, 2) for _ in b]
    p0 = hip.mgSolveParam(tol=a.tol, maxIter=a.max_iter)
    level1 = {"nuPost2_coarseIters4": dict(nuPost=2, coarseIters=4), "defaults": {}}

    # ---- (a) one K against one K^(3)
    K = {"K_fp64": lambda: hip.mgPrecondition(z64, b, gauge, a.kappa, T0, op1, clover=C),
         "K_fp32": lambda: hip.mgPreconditionSloppy(z32, b32, gauge, a.kappa, T0s, op1s, clover=C)}
    for name, cp in level1.items():
        K["K3_fp64_" + name] = lambda cp=cp: hip.mgPrecondition(z64, b, gauge, a.kappa, Ts, ops, clover=C, coarseParam=cp)
        K["K3_fp32_" + name] = lambda cp=cp: hip.mgPreconditionSloppy(z32, b32, gauge, a.kappa, Tss, opss, clover=C, coarseParam=cp)
    kt = alternated(K, 5, 2 * a.reps, a.warmup)

    # ---- (b) the operator launches alone
    f64 = [hip.SpinorField(X, 8, 2) for _ in b]
    c1a, c1b = [hip.CoarseField(op1.X, op1.n_vec, 8) for _ in b], [hip.CoarseField(op1.X, op1.n_vec, 8) for _ in b]
    c2a, c2b = [hip.CoarseField(op2.X, op2.n_vec, 8) for _ in b], [hip.CoarseField(op2.X, op2.n_vec, 8) for _ in b]
    hip.restrictVecs(c1a, b, T0)
    hip.restrictCoarseVecs(c2a, c1a, T1)
    parts = {"stencil": lambda: hip.wilsonApply(f64, b, gauge, a.kappa, clover=C),
             "R0": lambda: hip.restrictVecs(c1b, b, T0), "P0": lambda: hip.prolongateEvecs(f64, c1a, T0),
             "M1": lambda: hip.coarseApply(c1b, c1a, op1), "R1": lambda: hip.restrictCoarseVecs(c2b, c1a, T1),
             "P1": lambda: hip.prolongateCoarseEvecs(c1b, c2a, T1), "M2": lambda: hip.coarseApply(c2b, c2a, op2)}
    pt = alternated(parts, {k: 20 if k in ("stencil", "R0", "P0") else 40 for k in parts}, 2 * a.reps, a.warmup)
    med = {k: float(np.median(v)) for k, v in list(kt.items()) + list(pt.items())}

    def counts(q1):
        """launches of one K^(3) with params[0] = p0 and params[1] = q1 (two-grid: q1 None)"""
        c0 = p0.coarseIters
        n = {"stencil": p0.nuPre + p0.nuPost + (1 if c0 > 0 and p0.nuPost > 0 else 0), "R0": int(c0 > 0), "P0": int(c0 > 0)}
        if q1 is None:
            n.update(M1=c0, R1=0, P1=0, M2=0)
        else:
            c1 = q1.coarseIters
            n.update(M1=c0 * (1 + q1.nuPre + q1.nuPost + (1 if c1 > 0 and q1.nuPost > 0 else 0)), R1=c0 * int(c1 > 0), P1=c0 * int(c1 > 0), M2=c0 * c1)
        return n
    op_sum = {}
    for name, cp in [("K", None)] + [("K3_" + n, hip.mgSolveParam(**cp)) for n, cp in level1.items()]:
        n = counts(cp)
        op_sum[name] = {"launches": n, "ms": round(sum(n[k] * med[k] for k in n), 3)}

    # ---- (c) the solves
    info = {}
    kw = dict(tol=a.tol, maxIter=a.max_iter, allow_unconverged=True)
    xs = {k: [hip.SpinorField(X, 8, 2) for _ in b] for k in ("mg", "mg3", "mixed", "mixed3", "cg")}
    cp = level1["nuPost2_coarseIters4"]

    def keep(name, r):
        info[name] = r[1]
    solves = {"mg_solve": lambda: keep("mg", hip.mgSolve(b, gauge, a.kappa, T0, op1, clover=C, x=xs["mg"], **kw)),
              "mg3_solve": lambda: keep("mg3", hip.mgSolve(b, gauge, a.kappa, Ts, ops, clover=C, x=xs["mg3"], coarseParam=cp, **kw)),
              "mixed_solve": lambda: keep("mixed", hip.mgSolveMixed(b, gauge, a.kappa, T0s, op1s, clover=C, x=xs["mixed"], **kw)),
              "mixed3_solve": lambda: keep("mixed3", hip.mgSolveMixed(b, gauge, a.kappa, Tss, opss, clover=C, x=xs["mixed3"], coarseParam=cp, **kw)),
              "cg_solve": lambda: keep("cg", hip.wilsonSolve(b, gauge, a.kappa, tol=a.tol, maxIter=20 * a.max_iter, x=xs["cg"], allow_unconverged=True,
                                                             clover=C))}
    st = {k: [] for k in solves}
    for it in range(a.warmup + a.reps):
        for k in solves:
            ms = wall_ms(solves[k])
            if it >= a.warmup:
                st[k].append(ms)
    med.update({k: float(np.median(v)) for k, v in st.items()})

    def rel(u, v):
        return max(float(torch.linalg.vector_norm(x.data - y.data) / torch.linalg.vector_norm(y.data)) for x, y in zip(u, v))

    def solve_rec(i):
        return {"iters": [int(n) for n in i.iters], "relres_max": float(np.max(i.relres)), "converged": bool(i.converged),
                "hostReads": getattr(i, "hostReads", None)}

    # ---- (d)
    apply_forms = [forms(op2, "coarsest"), forms(op1, "level 1")] + [forms(random_operator(Xc, nv), "between (random)") for Xc, nv in between]

    rec = {"workload": "three-level GCR, %s fp64, aggregates %s n_vec %d then %s n_vec %d, %d right-hand sides, Wilson-clover kappa %g, random unitary "
                       "links, V_0 from mgSetup (setupMaxIter %d), V_1 from mgSetupCoarse"
                       % ("x".join(map(str, X)), "x".join(map(str, bs)), a.nvec, "x".join(map(str, bs1)), a.nvec1, a.nrhs, a.kappa, a.setup_iters),
           "param0": {n: getattr(p0, n) for n, _ in p0._fields_}, "param1": level1, "solve_param1": cp, "reps": a.reps, "warmup": a.warmup,
           "setup_s": round(setup_s, 2), "level1_lattice": list(op1.X), "coarsest_lattice": list(op2.X),
           "ms_median": {k: round(v, 3) for k, v in med.items()},
           "ms_min": {k: round(float(np.min(v)), 3) for k, v in list(kt.items()) + list(pt.items()) + list(st.items())},
           "K3_over_K": {k[3:]: round(med[k] / med["K_" + k[3:7]], 3) for k in med if k.startswith("K3_")},
           "operators_alone": op_sum,
           "cycle_minus_operators_ms": {"K": round(med["K_fp64"] - op_sum["K"]["ms"], 3),
                                        **{"K3_" + n: round(med["K3_fp64_" + n] - op_sum["K3_" + n]["ms"], 3) for n in level1}},
           "solves": {k: solve_rec(v) for k, v in info.items()},
           "mg3_over_mg_time": round(med["mg3_solve"] / med["mg_solve"], 3), "mixed3_over_mixed_time": round(med["mixed3_solve"] / med["mixed_solve"], 3),
           "cg_over_mg3_time": round(med["cg_solve"] / med["mg3_solve"], 3),
           "x_rel_diff_mg3_vs_mg_max": rel(xs["mg3"], xs["mg"]), "x_rel_diff_mixed3_vs_mg_max": rel(xs["mixed3"], xs["mg"]),
           "apply_forms": apply_forms}
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
