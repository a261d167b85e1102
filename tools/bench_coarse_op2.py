"""Time the coarsest level of a three-level hierarchy (mugiq_hip_compute_coarse_operator_coarse and what runs on its result) on the
hierarchy tools/bench_mg_setup.py makes:

    python tools/bench_coarse_op2.py [--lattice 32 32 32 32] [--block 4 4 4 4] [--nvec 24] [--block1 2 2 2 2] [--nvec1 32]
                                     [--nconv 200] [--nkr 256] [--out profiles/coarse_op2_latest.json]

The configuration is a random one (every link a random unitary matrix), Wilson-clover, the null vectors those of the MG setup from the
Gaussian start vectors of seed 13 (setupMaxIter 50), as in tools/bench_mg_setup.py and tools/bench_coarse_eig.py; the second level is
mgSetupCoarse's own (the n_vec1 lowest eigenvectors of MdagM of the first coarse operator).  Measured, medians after a warm-up with the
compared routes alternated in the same loop:
  * the build, against its models: the complex multiply-adds of the definition (8 real flops each) and every K_m(x) and V read once at
    the rate the read probe shows on the input operator in the same loop;
  * coarseApply per block of 8 (M and MdagM) on the coarsest operator, against a streaming read of it (the probe on that operator);
  * the eigenpair check of nconv coarsest vectors on the operator against the fine route through both transfers;
  * coarseEigensolve(nconv, nkr) on the coarsest operator against the same call on the one-level operator, each run once (host clock
    around a call that ends in a synchronise): time, rounds, block applications, host reads and the host's dense share;
  * mgSetupCoarse, once.
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
from bench_mg_solve import batched_q  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", type=int, nargs=4, default=[32, 32, 32, 32])
    ap.add_argument("--block", type=int, nargs=4, default=[4, 4, 4, 4])
    ap.add_argument("--nvec", type=int, default=24)
    ap.add_argument("--block1", type=int, nargs=4, default=[2, 2, 2, 2])
    ap.add_argument("--nvec1", type=int, default=32)
    ap.add_argument("--kappa", type=float, default=0.124)
    ap.add_argument("--csw-coeff", type=float, default=0.1)
    ap.add_argument("--setup-iters", type=int, default=50)
    ap.add_argument("--nconv", type=int, default=200)
    ap.add_argument("--nkr", type=int, default=256)
    ap.add_argument("--poly-deg", type=int, default=20)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-one-level-solve", action="store_true", help="do not re-measure the solve on the one-level operator")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "coarse_op2_latest.json"))
    a = ap.parse_args()
    X, bs, bs1 = tuple(a.lattice), tuple(a.block), tuple(a.block1)
    torch.cuda.set_device(0)
    gen = torch.Generator(device="cuda").manual_seed(12)
    vcb = int(np.prod(X)) // 2

    def wall_ms(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t)

    def event_ms(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    gauge = hip.GaugeField(X, (0, 0, 0, 0), 8)
    U = batched_q(torch.randn(8 * vcb, 3, 3, dtype=torch.complex128, device="cuda", generator=gen)).reshape(2, 4, vcb, 3, 3)
    gauge.data.view(2, 4, 9, vcb).copy_(U.reshape(2, 4, vcb, 9).permute(0, 1, 3, 2))
    del U
    C = hip.CloverField(X, 8).compute(gauge, a.csw_coeff)
    vecs = hip.mgStartVectors(X, a.nvec, seed=13)
    T0, op1, setup = hip.mgSetup(gauge, a.kappa, a.nvec, bs, start=vecs, clover=C, setupMaxIter=a.setup_iters)
    del vecs
    torch.cuda.empty_cache()

    # ---- the second level, once
    made = {}

    def setup_coarse():
        made["r"] = hip.mgSetupCoarse(op1, a.nvec1, bs1, seed=21)
    setup_coarse_ms = wall_ms(setup_coarse)
    T1, op2, sinfo = made["r"]
    X1, X2 = op1.X, op2.X
    nc, nv = op1.n_vec, a.nvec1
    sites1 = int(np.prod(X1))

    # ---- the solves, each once
    def solve(op, deg):
        start = hip.coarseStartVectors(op.X, op.n_vec, a.nkr, seed=14)
        got = {}

        def run():
            got["r"] = hip.coarseEigensolve(op, start=start, nConv=a.nconv, nKr=a.nkr, polyDeg=deg, tol=a.tol, maxIter=a.max_iter, allow_unconverged=True)
        ms = wall_ms(run)
        ev, theta, res, sigma, info = got["r"]
        rec = {"total_ms": round(ms, 1), "polyDeg": deg, "converged": bool(info.converged), "iters": info.iters, "nConverged": info.nConverged,
               "opBlocks": info.opBlocks, "hostReads": info.hostReads, "hostDenseSeconds": round(info.hostDenseSeconds, 3),
               "host_dense_fraction": round(1e3 * info.hostDenseSeconds / ms, 3), "aMaxUsed": info.aMaxUsed, "theta_min": float(theta[0]),
               "theta_max_returned": float(theta[-1]), "residual_max": float(np.max(res)), "dimension": int(2 * op.volumeCB * 2 * op.n_vec)}
        return ev, theta, rec
    solves = {}
    ev2 = None
    for deg in (a.poly_deg, max(a.poly_deg // 2, 2), max(a.poly_deg // 4, 2)):      # a dependent filtered basis (status 1) is reported, then a milder filter tried
        try:
            ev2, theta2, solves["coarsest"] = solve(op2, deg)
            break
        except hip.MugiqHipError as e:
            solves.setdefault("coarsest_failures", []).append({"polyDeg": deg, "error": str(e)[:200]})
    if ev2 is None:
        raise SystemExit("the coarsest solve failed with every filter degree: %s" % solves)
    if not a.skip_one_level_solve:
        ev1, theta1, solves["one_level"] = solve(op1, a.poly_deg)
        solves["theta_first_nvec1_coarsest_minus_one_level_max"] = float(np.max(np.abs(theta2[:min(nv, a.nconv)] - theta1[:min(nv, a.nconv)])))
        del ev1
        torch.cuda.empty_cache()

    # ---- the kernels and the eigenpair checks, alternated
    OP = hip.MUGIQ_EIG_OPERATOR_MdagM
    src, dst = ev2[:8], [hip.CoarseField(X2, nv, 8) for _ in range(8)]
    res_c, res_f = [None], [None]

    def evals_op():
        res_c[0] = hip.computeEvalsCoarse(ev2, opType=OP, coarseOp=op2)

    def evals_fine():
        res_f[0] = hip.computeEvalsCoarse(ev2, [T0, T1], gauge, a.kappa, OP, clover=C)
    routes = {
        "build": lambda: hip.computeCoarseOperatorCoarse(T1, op1, op=op2),
        "read_probe_input_operator": lambda: hip.probeReadBandwidth(op1.data),
        "apply_M_block_of_8": lambda: hip.coarseApply(dst, src, op2, hip.MUGIQ_EIG_OPERATOR_M),
        "apply_MdagM_block_of_8": lambda: hip.coarseApply(dst, src, op2, OP),
        "read_probe_coarsest_operator": lambda: hip.probeReadBandwidth(op2.data),
        "evals_operator": evals_op,
        "evals_fine_route_two_transfers": evals_fine,
    }
    times = {k: [] for k in routes}
    for it in range(a.warmup + a.reps):
        for k in routes:
            ms = event_ms(routes[k])
            if it >= a.warmup:
                times[k].append(ms)
    med = {k: float(np.median(v)) for k, v in times.items()}
    big = float(np.max(np.abs(res_f[0][0])))
    evals_dev = float(max(np.max(np.abs(res_c[0][0] - res_f[0][0])), np.max(np.abs(res_c[0][1] - res_f[0][1]))) / big)

    op1_bytes, op2_bytes = op1.data.numel() * 16, op2.data.numel() * 16
    v_bytes = 2 * sites1 // 2 * 2 * nc * nv * 16
    cmadds = sites1 * 9 * (2 * nc * 2 * nv * nc + 2 * nv * 2 * nv * nc)             # T = K E(x'), then E(x)^dag T, E chirality-diagonal
    gflop = 8.0 * cmadds / 1e9
    rate1 = op1_bytes / (med["read_probe_input_operator"] * 1e-3) / 1e9             # GB/s
    rate2 = op2_bytes / (med["read_probe_coarsest_operator"] * 1e-3) / 1e9
    rec = {"workload": "coarsest operator of %s fp64, aggregates %s n_vec %d then %s n_vec %d, Wilson-clover kappa %g, random unitary links"
                       % ("x".join(map(str, X)), "x".join(map(str, bs)), nc, "x".join(map(str, bs1)), nv, a.kappa),
           "reps": a.reps, "warmup": a.warmup, "level1_lattice": list(X1), "coarsest_lattice": list(X2),
           "input_operator_GB": round(op1_bytes / 1e9, 3), "coarsest_operator_MB": round(op2_bytes / 1e6, 1), "V1_GB": round(v_bytes / 1e9, 3),
           "ms_median": {k: round(v, 3) for k, v in med.items()}, "ms_min": {k: round(float(np.min(v)), 3) for k, v in times.items()},
           "build_model_gflop": round(gflop, 1), "build_tflops": round(gflop / med["build"], 2),
           "read_probe_GBps": {"input_operator": round(rate1, 0), "coarsest_operator": round(rate2, 0)},
           "build_byte_floor_ms": round((op1_bytes + v_bytes) / (rate1 * 1e9) * 1e3, 3),
           "build_over_byte_floor": round(med["build"] / ((op1_bytes + v_bytes) / (rate1 * 1e9) * 1e3), 2),
           "apply_M_over_streaming_read": round(med["apply_M_block_of_8"] / med["read_probe_coarsest_operator"], 2),
           "apply_MdagM_over_two_streaming_reads": round(med["apply_MdagM_block_of_8"] / (2 * med["read_probe_coarsest_operator"]), 2),
           "evals_vectors": len(ev2), "evals_fine_route_over_operator": round(med["evals_fine_route_two_transfers"] / med["evals_operator"], 2),
           "evals_routes_max_relative_difference": evals_dev,
           "eigensolve": solves,
           "mg_setup_coarse": {"ms": round(setup_coarse_ms, 1), "nKr": (max(2 * nv, nv + 8) + 7) // 8 * 8, "tol": 1e-8, "iters": sinfo.eigensolve.iters,
                               "opBlocks": sinfo.eigensolve.opBlocks, "converged": bool(sinfo.eigensolve.converged),
                               "hostDenseSeconds": round(sinfo.eigensolve.hostDenseSeconds, 3), "minPivotRatio": sinfo.minPivotRatio,
                               "zeroColumns": sinfo.zeroColumns, "orthonormality": sinfo.orthonormality},
           "mg_setup": {"setupMaxIter": a.setup_iters, "orthonormality": setup.orthonormality, "minPivotRatio": setup.minPivotRatio}}
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
