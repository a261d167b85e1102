"""Time the mixed-precision two-grid solve (mugiq_hip_mg_solve_mixed: the cycle K in fp32 storage under the fp64 GCR) against the fp64 solve
(mugiq_hip_mg_solve) and the plain CG (mugiq_hip_wilson_clover_solve) on the same right-hand sides, in one run:

    python tools/bench_mg_solve_mixed.py [--lattice 32 32 32 32] [--block 4 4 4 4] [--nvec 24] [--nrhs 8] [--out profiles/mg_solve_mixed_latest.json]

Shape, fields and null vectors are those of tools/bench_mg_solve.py (its functions are imported); the fp32 hierarchy is made on the device:
T32 = T.astype(4), op32 = computeCoarseOperator(T32, ...), and fp32 copies of the gauge and clover fields for the legs that use them.
  (a) mgSolveMixed (cycle on the fp64 links, and on the fp32 copies), mgSolve and wilsonSolve, same right-hand sides and tolerance,
      alternated in one loop, host clock around calls that end in a synchronise, medians of --reps after --warmup; iteration counts;
  (b) one K on the block of right-hand sides in fp64 and in fp32 (both link precisions), alternated, device events around loops of 5;
  (c) the operator launches of K alone in both storages (stencil, restriction, prolongation, coarse application), events around loops of
      20 to 40: K minus their sum is what the Krylov kernels and the launch gaps take in each storage;
  (d) streaming rates: the read probe (mugiq_hip_probe_read_bandwidth), and the conversion kernel, which has the access form of every
      Krylov kernel (one complex number per lane and access), as a copy in fp64, a copy in fp32, and the two conversions of the hand-over.
With --profile-only the script makes the fields, runs three K of each storage and one solve of each kind and exits: the run to put under
rocprofv3 --kernel-trace --stats for the per-kernel times (the Krylov kernels carry their storage in their names).
One JSON record is printed and written to --out."""
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
from bench_mg_solve import batched_q, null_vectors  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", type=int, nargs=4, default=[32, 32, 32, 32])
    ap.add_argument("--block", type=int, nargs=4, default=[4, 4, 4, 4])
    ap.add_argument("--nvec", type=int, default=24)
    ap.add_argument("--nrhs", type=int, default=8)
    ap.add_argument("--kappa", type=float, default=0.124)
    ap.add_argument("--csw-coeff", type=float, default=0.1)
    ap.add_argument("--setup-iters", type=int, default=20)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--max-iter", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mg_solve_mixed_latest.json"))
    for name in ("nKrylov", "nuPre", "nuPost", "coarseIters"):
        ap.add_argument("--" + name, type=int, default=None)
    a = ap.parse_args()
    X, bs = tuple(a.lattice), tuple(a.block)
    torch.cuda.set_device(0)
    gen = torch.Generator(device="cuda").manual_seed(12)
    vol, vcb = int(np.prod(X)), int(np.prod(X)) // 2
    prm = {k: getattr(a, k) for k in ("nKrylov", "nuPre", "nuPost", "coarseIters") if getattr(a, k) is not None}
    p = hip.mgSolveParam(tol=a.tol, maxIter=a.max_iter, **prm)

    def crandn(*shape):
        return torch.randn(*shape, dtype=torch.complex128, device="cuda", generator=gen)

    gauge = hip.GaugeField(X, (0, 0, 0, 0), 8)
    U = batched_q(crandn(8 * vcb, 3, 3)).reshape(2, 4, vcb, 3, 3)                     # [parity, mu, x_cb, row, col]: random unitary links
    gauge.data.view(2, 4, 9, vcb).copy_(U.reshape(2, 4, vcb, 9).permute(0, 1, 3, 2))
    del U
    C = hip.CloverField(X, 8).compute(gauge, a.csw_coeff)

    def random_fields(n):
        out = []
        for _ in range(n):
            f = hip.SpinorField(X, 8, 2)
            f.data.copy_(crandn(f.data.numel()))
            out.append(f)
        return out

    # ---- the crude null vectors, the coarse operator, and the sloppy objects from them
    t0 = time.perf_counter()
    src = random_fields(a.nvec)
    nv, _ = hip.wilsonSolve(src, gauge, a.kappa, tol=1e-12, maxIter=a.setup_iters, allow_unconverged=True, clover=C)
    T = hip.Transfer(X, a.nvec, bs, 2, 8)
    null_vectors(T, nv, X, bs)
    del src, nv
    op = hip.computeCoarseOperator(T, gauge, a.kappa, clover=C)
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    T32 = T.astype(4)
    op32 = hip.computeCoarseOperator(T32, gauge, a.kappa, clover=C)
    g32 = hip.GaugeField(X, (0, 0, 0, 0), 4)
    g32.data.copy_(gauge.data.to(torch.complex64))
    C32 = hip.CloverField(X, 4)
    C32.data.copy_(C.data.to(C32.data.dtype))
    torch.cuda.synchronize()
    sloppy_setup_s = time.perf_counter() - t0

    b = random_fields(a.nrhs)
    new64 = lambda: [hip.SpinorField(X, 8, 2) for _ in b]                             # noqa: E731
    new32 = lambda: [hip.SpinorField(X, 4, 2) for _ in b]                             # noqa: E731
    x_mg, x_mx, x_mxs, x_cg = new64(), new64(), new64(), new64()
    b32, z32, z64 = new32(), new32(), new64()
    hip.mgConvertPrecision(b32, b)
    info = {}
    kw = dict(tol=a.tol, maxIter=a.max_iter, allow_unconverged=True, **prm)

    def run_mg():
        _, info["mg"] = hip.mgSolve(b, gauge, a.kappa, T, op, clover=C, x=x_mg, **kw)

    def run_mixed():
        _, info["mixed"] = hip.mgSolveMixed(b, gauge, a.kappa, T32, op32, clover=C, x=x_mx, **kw)

    def run_mixed_sloppy_links():
        _, info["mixed_fp32_links"] = hip.mgSolveMixed(b, gauge, a.kappa, T32, op32, clover=C, gaugeSloppy=g32, cloverSloppy=C32, x=x_mxs, **kw)

    def run_cg():
        _, info["cg"] = hip.wilsonSolve(b, gauge, a.kappa, tol=a.tol, maxIter=20 * a.max_iter, x=x_cg, allow_unconverged=True, clover=C)

    K = {"K_fp64": lambda: hip.mgPrecondition(z64, b, gauge, a.kappa, T, op, clover=C, **prm),
         "K_fp32": lambda: hip.mgPreconditionSloppy(z32, b32, gauge, a.kappa, T32, op32, clover=C, **prm),
         "K_fp32_fp32_links": lambda: hip.mgPreconditionSloppy(z32, b32, g32, a.kappa, T32, op32, clover=C32, **prm)}
    solves = {"mg_solve": run_mg, "mixed_solve": run_mixed, "mixed_solve_fp32_links": run_mixed_sloppy_links, "cg_solve": run_cg}
    if a.profile_only:
        for _ in range(3):
            for fn in K.values():
                fn()
        for fn in solves.values():
            fn()
        torch.cuda.synchronize()
        print(json.dumps({"profile_only": True, "iters": {k: [int(i) for i in v.iters] for k, v in info.items()}}))
        return

    def wall_ms(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t)

    def event_ms(fn, n):
        """milliseconds per call of n calls between two events"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    st = {k: [] for k in solves}
    for it in range(a.warmup + a.reps):
        for k in solves:                                                              # alternated
            ms = wall_ms(solves[k])
            if it >= a.warmup:
                st[k].append(ms)

    # ---- one K in each storage, and its operator launches alone
    f64, f32 = new64(), new32()
    cw, cy = [hip.CoarseField(T.Xc, a.nvec, 8) for _ in b], [hip.CoarseField(T.Xc, a.nvec, 8) for _ in b]
    cw32, cy32 = [hip.CoarseField(T.Xc, a.nvec, 4) for _ in b], [hip.CoarseField(T.Xc, a.nvec, 4) for _ in b]
    hip.restrictVecs(cw, b, T)
    hip.restrictVecs(cw32, b32, T32)
    probe = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")                    # 1 GiB: far beyond the last-level cache
    c64, c32 = new64(), new32()
    parts = dict(K)
    parts.update({
        "stencil_fp64": lambda: hip.wilsonApply(f64, b, gauge, a.kappa, clover=C),
        "stencil_fp32": lambda: hip.wilsonApply(f32, b32, gauge, a.kappa, clover=C),
        "stencil_fp32_fp32_links": lambda: hip.wilsonApply(f32, b32, g32, a.kappa, clover=C32),
        "restrict_fp64": lambda: hip.restrictVecs(cy, b, T), "restrict_fp32": lambda: hip.restrictVecs(cy32, b32, T32),
        "prolong_fp64": lambda: hip.prolongateEvecs(f64, cw, T), "prolong_fp32": lambda: hip.prolongateEvecs(f32, cw32, T32),
        "coarse_apply_fp64": lambda: hip.coarseApply(cy, cw, op), "coarse_apply_fp32": lambda: hip.coarseApply(cy32, cw32, op32),
        "read_probe_1GiB": lambda: hip.probeReadBandwidth(probe),
        "copy_fp64": lambda: hip.mgConvertPrecision(c64, b), "copy_fp32": lambda: hip.mgConvertPrecision(c32, b32),
        "round_fp64_to_fp32": lambda: hip.mgConvertPrecision(c32, b), "widen_fp32_to_fp64": lambda: hip.mgConvertPrecision(c64, b32),
    })
    loop = {k: 5 if k.startswith("K_") else 40 if k.startswith("coarse") else 20 for k in parts}
    pt = {k: [] for k in parts}
    for it in range(a.warmup + 2 * a.reps):
        for k in parts:                                                               # alternated
            ms = event_ms(parts[k], loop[k])
            if it >= a.warmup:
                pt[k].append(ms)
    med = {k: float(np.median(v)) for k, v in list(st.items()) + list(pt.items())}
    n_stencil = p.nuPre + p.nuPost + (1 if p.coarseIters > 0 and p.nuPost > 0 else 0)
    co = 1 if p.coarseIters > 0 else 0

    def ops(sfx, stencil):
        return n_stencil * med[stencil] + co * (med["restrict_" + sfx] + med["prolong_" + sfx] + p.coarseIters * med["coarse_apply_" + sfx])

    ops_ms = {"K_fp64": ops("fp64", "stencil_fp64"), "K_fp32": ops("fp32", "stencil_fp32"), "K_fp32_fp32_links": ops("fp32", "stencil_fp32_fp32_links")}
    fv64, fv32 = 24 * vol * 8, 24 * vol * 4                                           # bytes of one fine vector
    gbs = {"read_probe_1GiB": probe.numel() / med["read_probe_1GiB"] / 1e6,
           "copy_fp64": 2 * a.nrhs * fv64 / med["copy_fp64"] / 1e6, "copy_fp32": 2 * a.nrhs * fv32 / med["copy_fp32"] / 1e6,
           "round_fp64_to_fp32": a.nrhs * (fv64 + fv32) / med["round_fp64_to_fp32"] / 1e6,
           "widen_fp32_to_fp64": a.nrhs * (fv64 + fv32) / med["widen_fp32_to_fp64"] / 1e6}

    def rel(u, v):
        return max(float(torch.linalg.vector_norm(x.data - y.data) / torch.linalg.vector_norm(y.data)) for x, y in zip(u, v))

    def solve_rec(i):
        return {"iters": [int(n) for n in i.iters], "relres_max": float(np.max(i.relres)), "converged": bool(i.converged),
                "hostReads": getattr(i, "hostReads", None)}

    res = {"workload": "mixed two-grid GCR (cycle in fp32 storage), %s, aggregates %s, n_vec %d, %d right-hand sides, Wilson-clover kappa %g, random unitary "
                       "links, crude null vectors (%d CG iterations, per-aggregate QR)" % ("x".join(map(str, X)), "x".join(map(str, bs)), a.nvec, a.nrhs, a.kappa,
                                                                                           a.setup_iters),
           "param": {n: getattr(p, n) for n, _ in p._fields_}, "reps": a.reps, "warmup": a.warmup, "setup_s": round(setup_s, 2),
           "sloppy_setup_s": round(sloppy_setup_s, 2),
           "ms_median": {k: round(v, 3) for k, v in med.items()}, "ms_min": {k: round(float(np.min(v)), 3) for k, v in list(st.items()) + list(pt.items())},
           "solves": {k: solve_rec(v) for k, v in info.items()},
           "mg_over_mixed_time": round(med["mg_solve"] / med["mixed_solve"], 3), "cg_over_mixed_time": round(med["cg_solve"] / med["mixed_solve"], 3),
           "mg_over_mixed_fp32_links_time": round(med["mg_solve"] / med["mixed_solve_fp32_links"], 3),
           "cg_over_mg_time": round(med["cg_solve"] / med["mg_solve"], 3),
           "K_fp64_over_K_fp32": round(med["K_fp64"] / med["K_fp32"], 3), "K_fp64_over_K_fp32_fp32_links": round(med["K_fp64"] / med["K_fp32_fp32_links"], 3),
           "K_operators_alone_ms": {k: round(v, 3) for k, v in ops_ms.items()},
           "K_minus_operators_ms": {k: round(med[k] - v, 3) for k, v in ops_ms.items()},
           # the Krylov kernels of the default K (four MR steps after the coarse correction), in fine-vector passes per right-hand side: s = r - t
           # 3; per MR step the dots read t, s (2) and the update reads s, z, t and writes z, s (5; the last step 3); the coarse level is 1/500
           "model_fine_vector_passes_krylov_in_K": 3 + 7 * max(n_stencil - 1, 0) - 2,
           "GB_per_s": {k: round(v, 1) for k, v in gbs.items()},
           "x_rel_diff_mixed_vs_mg_max": rel(x_mx, x_mg), "x_rel_diff_mixed_fp32_links_vs_mg_max": rel(x_mxs, x_mg), "x_rel_diff_mg_vs_cg_max": rel(x_mg, x_cg)}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
