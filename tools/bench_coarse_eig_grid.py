"""Time the coarse eigensolver on a process grid against the single-domain solver, on one GPU, in one run:

    python tools/bench_coarse_eig_grid.py [--lattice 32 32 32 32] [--block 4 4 4 4] [--nvec 24] [--out profiles/coarse_eig_grid_latest.json]

For the partitionings z + t and x + y + z + t, forced on one rank (GridComm(force_partitioned=): the rank is its own neighbour, every message
a device copy issued from the comm's Python callback -- the pack kernels, the fused step kernel, the ghost path of the operator and the
host side of the exchange are measured, a link is not), three routes on the same operator and start vectors:
  single   coarseEigensolve,
  grid0    coarseEigensolveGrid with MUGIQ_HIP_EIG_PACK_IN_STEP=0 (plain step kernel, a pack kernel per face and launch),
  grid1    coarseEigensolveGrid with MUGIQ_HIP_EIG_PACK_IN_STEP=1 (the step kernel writes the send faces of the next application).
The solver has no entry for its parts, so they are timed as differences of whole calls with a given aMax (no power estimate):
  filter_block   one block of 8 through polyDeg 20: a call with nKr 8, maxIter 1 and polyDeg 40 minus the same call with polyDeg 20
                 (20 applications of MdagM and 20 steps, every one of them a step that feeds another application);
  orth_rr        one orthonormalisation plus Rayleigh-Ritz round at nKr 256: a call with maxIter 0 (and the 8 returned vectors).
Wall times around calls that end in a synchronise, --reps repetitions after --warmup runs, the routes alternated; medians and ratios to
the single-domain route of the same run.  A two-round solve (nKr 32, maxIter 2) must give the same bits on all three routes (asserted,
and recorded).  One JSON record is printed and written to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mugiq_amd as hip  # noqa: E402

PARTITIONINGS = {"zt": (0, 0, 1, 1), "xyzt": (1, 1, 1, 1)}
ENV = "MUGIQ_HIP_EIG_PACK_IN_STEP"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", type=int, nargs=4, default=[32, 32, 32, 32])
    ap.add_argument("--block", type=int, nargs=4, default=[4, 4, 4, 4])
    ap.add_argument("--nvec", type=int, default=24)
    ap.add_argument("--kappa", type=float, default=0.12)
    ap.add_argument("--no-clover", action="store_true")
    ap.add_argument("--nkr", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "coarse_eig_grid_latest.json"))
    a = ap.parse_args()
    X, bs = tuple(a.lattice), tuple(a.block)
    torch.cuda.set_device(0)
    gen = torch.Generator(device="cuda").manual_seed(13)

    def fill(t, scale):
        step = 1 << 26
        for i in range(0, t.numel(), step):
            t[i:i + step].copy_(torch.randn(min(step, t.numel() - i), dtype=t.dtype, device="cuda", generator=gen) * scale)

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def bits(r):
        ev, theta, res, sig = r[:4]
        return [torch.view_as_real(f.data).view(torch.int64).clone() for f in ev], theta.view(np.int64).copy(), res.view(np.int64).copy(), r[4][:7]

    def same(x, y):
        return all(bool(torch.equal(p, q)) for p, q in zip(x[0], y[0])) and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2]) and x[3] == y[3]

    T = hip.Transfer(X, a.nvec, bs, 2, 8)
    fill(T.V, 1.0 / np.sqrt(12.0 * a.nvec * int(np.prod(bs))))
    start = hip.coarseStartVectors(T.Xc, a.nvec, a.nkr, seed=3)
    op0 = hip.CoarseOperator(T.Xc, a.nvec, 8)
    MdagM = hip.MUGIQ_EIG_OPERATOR_MdagM
    res = {"workload": "coarse eigensolver on a forced partition of one rank, %s fp64, aggregates %s, n_vec %d, MdagM, %s"
                       % ("x".join(map(str, X)), "x".join(map(str, bs)), a.nvec, "Wilson" if a.no_clover else "Wilson-clover"),
           "reps": a.reps, "warmup": a.warmup, "nKr_orth_rr": a.nkr, "polyDeg": 20, "partitionings": {}}
    for name, force in PARTITIONINGS.items():
        comm = hip.GridComm((1, 1, 1, 1), device="cuda:0", force_partitioned=force)
        gauge = hip.GaugeField(X, force, 8)
        fill(gauge.data, 1.0 / np.sqrt(6.0))
        gauge.exchangeBorders(comm)
        C = None if a.no_clover else hip.CloverField(X, 8).compute(gauge, 0.1, comm)
        hip.computeCoarseOperator(T, gauge, a.kappa, clover=C, op=op0)
        op1 = hip.computeCoarseOperatorGrid(T, gauge, a.kappa, comm, clover=C)
        # aMax once, by the power estimate of a call that does nothing else of size
        aMax = hip.coarseEigensolve(op0, MdagM, start[:8], allow_unconverged=True, nConv=1, nKr=8, maxIter=0)[4].aMaxUsed
        aMin = 0.05 * aMax  # a gentle filter: the timing calls run degree 40 on 8 vectors and must not end in a rank failure

        def solve(route, **prm):
            n = prm["nKr"]
            if route == "single":
                return hip.coarseEigensolve(op0, MdagM, start[:n], allow_unconverged=True, aMax=aMax, **prm)
            os.environ[ENV] = route[-1]
            try:
                return hip.coarseEigensolveGrid(op1, comm, MdagM, start[:n], allow_unconverged=True, aMax=aMax, **prm)
            finally:
                del os.environ[ENV]

        routes = ("single", "grid0", "grid1")
        calls = {"filter_deg20": dict(nConv=1, nKr=8, maxIter=1, polyDeg=20, aMin=aMin, rankTol=0.0),
                 "filter_deg40": dict(nConv=1, nKr=8, maxIter=1, polyDeg=40, aMin=aMin, rankTol=0.0),
                 "orth_rr": dict(nConv=8, nKr=a.nkr, maxIter=0)}
        times = {(r, c): [] for r in routes for c in calls}
        last = {}
        for it in range(a.warmup + a.reps):
            for c, prm in calls.items():
                for r in routes:
                    ms, out = wall_ms(lambda: solve(r, **prm))
                    last[r, c] = out
                    if it >= a.warmup:
                        times[r, c].append(ms)
        med = {k: float(np.median(v)) for k, v in times.items()}
        block = {r: float(np.median(np.array(times[r, "filter_deg40"]) - np.array(times[r, "filter_deg20"]))) for r in routes}
        two = {r: bits(solve(r, nConv=8, nKr=32, maxIter=2, polyDeg=20)) for r in routes}
        equal = {"two_round_solve": same(two["single"], two["grid0"]) and same(two["single"], two["grid1"]),
                 "filter_deg40": same(bits(last["single", "filter_deg40"]), bits(last["grid0", "filter_deg40"]))
                 and same(bits(last["single", "filter_deg40"]), bits(last["grid1", "filter_deg40"])),
                 "orth_rr": same(bits(last["single", "orth_rr"]), bits(last["grid1", "orth_rr"]))}
        assert all(equal.values()), (name, equal)
        g0, g1 = last["grid0", "filter_deg40"][5], last["grid1", "filter_deg40"][5]
        res["partitionings"][name] = {
            "force_partitioned": list(force), "aMax": aMax,
            "filter_block_ms": {r: round(block[r], 4) for r in routes},
            "orth_rr_ms": {r: round(med[r, "orth_rr"], 3) for r in routes},
            "call_ms_median": {"%s_%s" % (r, c): round(v, 3) for (r, c), v in med.items()},
            "ratio_over_single": {"filter_block_grid0": round(block["grid0"] / block["single"], 4), "filter_block_grid1": round(block["grid1"] / block["single"], 4),
                                  "orth_rr_grid0": round(med["grid0", "orth_rr"] / med["single", "orth_rr"], 4),
                                  "orth_rr_grid1": round(med["grid1", "orth_rr"] / med["single", "orth_rr"], 4)},
            "ratio_grid1_over_grid0_filter_block": round(block["grid1"] / block["grid0"], 4),
            "grid_info_deg40": {"grid0": list(g0), "grid1": list(g1)},
            "host_dense_seconds_orth_rr": round(last["single", "orth_rr"][4].hostDenseSeconds, 4),
            "bit_equal": equal}
        del gauge, C, comm, op1
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
