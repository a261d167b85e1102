"""Time the explicit Galerkin coarse operator against the route through the fine lattice, in one run:

    python tools/bench_coarse_op.py [--lattice 32 32 32 32] [--block 4 4 4 4] [--nvec 24] [--nev 200] [--out profiles/coarse_op_latest.json]

  (a) computeCoarseOperator: the build (once per configuration),
  (b) coarseApply of the form M on all coarse vectors: one application per block of 8,
  (c) computeEvalsCoarse(..., coarseOp=): the eigenpair check (form MdagM) on the explicit operator,
  (d) computeEvalsCoarse without coarseOp: the same check through prolongation, fine stencil and restriction.
Event times around calls that end in a synchronise, --reps repetitions after --warmup runs, (c) and (d) alternated; medians.  Models, computed
here from the shapes: the build's flop (6 N^2 complex multiply-adds per fine site and term, 9 terms) and bytes (V once, the matrices once);
the byte floor of an application, one read of the 9 N^2 matrices of every site per block of 8 vectors, next to a plain streaming read of
the same buffer.  One JSON record is printed and written to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mugiq_amd as hip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", type=int, nargs=4, default=[32, 32, 32, 32])
    ap.add_argument("--block", type=int, nargs=4, default=[4, 4, 4, 4])
    ap.add_argument("--nvec", type=int, default=24)
    ap.add_argument("--nev", type=int, default=200)
    ap.add_argument("--kappa", type=float, default=0.12)
    ap.add_argument("--no-clover", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "coarse_op_latest.json"))
    a = ap.parse_args()
    X, bs = tuple(a.lattice), tuple(a.block)
    torch.cuda.set_device(0)
    gen = torch.Generator(device="cuda").manual_seed(11)
    vol = int(np.prod(X))
    N = 2 * a.nvec

    def fill(t, scale):
        step = 1 << 26
        for i in range(0, t.numel(), step):
            t[i:i + step].copy_(torch.randn(min(step, t.numel() - i), dtype=t.dtype, device="cuda", generator=gen) * scale)

    T = hip.Transfer(X, a.nvec, bs, 2, 8)
    fill(T.V, 1.0 / np.sqrt(12.0 * a.nvec * int(np.prod(bs))))
    gauge = hip.GaugeField(X, (0, 0, 0, 0), 8)
    fill(gauge.data, 1.0 / np.sqrt(6.0))                       # links are applied as stored: random 3 x 3 matrices of unit row norm on average
    C = None if a.no_clover else hip.CloverField(X, 8).compute(gauge, 0.1)
    cw = [hip.CoarseField(T.Xc, a.nvec, 8) for _ in range(a.nev)]
    for w in cw:
        fill(w.data, 1.0 / np.sqrt(w.data.numel()))
    out = [hip.CoarseField(T.Xc, a.nvec, 8) for _ in range(a.nev)]
    op = hip.CoarseOperator(T.Xc, a.nvec, 8)
    OP = hip.MUGIQ_EIG_OPERATOR_MdagM
    res_c, res_d = [None], [None]

    def event_ms(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    def evals_op():
        res_c[0] = hip.computeEvalsCoarse(cw, opType=OP, coarseOp=op)

    def evals_fine():
        res_d[0] = hip.computeEvalsCoarse(cw, T, gauge, a.kappa, OP, clover=C)

    routes = {
        "build": lambda: hip.computeCoarseOperator(T, gauge, a.kappa, clover=C, op=op),
        "apply_M_all": lambda: hip.coarseApply(out, cw, op, hip.MUGIQ_EIG_OPERATOR_M),
        "apply_Mdag_all": lambda: hip.coarseApply(out, cw, op, hip.MUGIQ_EIG_OPERATOR_Mdag),
        "read_probe_operator": lambda: hip.probeReadBandwidth(op.data),
        "evals_operator": evals_op,
        "evals_fine_route": evals_fine,
    }
    times = {k: [] for k in routes}
    for it in range(a.warmup + a.reps):
        for k in routes:                                          # the two eigenpair checks alternate
            ms = event_ms(routes[k])
            if it >= a.warmup:
                times[k].append(ms)
    med = {k: float(np.median(v)) for k, v in times.items()}

    def dev(x, y):
        return float(np.max(np.abs(x - y)) / np.max(np.abs(y)))
    diff = max(dev(res_c[0][i], res_d[0][i]) for i in range(3))

    cb = 16                                                       # bytes of a complex double
    nblocks = (a.nev + 7) // 8
    vbytes = 12 * a.nvec * cb * vol
    opbytes = 2 * op.volumeCB * 9 * N * N * cb
    build_flop = vol * 9 * 6 * N * N * 8
    apply_floor = nblocks * opbytes
    res = {"workload": "explicit coarse operator, %s fp64, aggregates %s, n_vec %d, %d coarse vectors, %s"
                       % ("x".join(map(str, X)), "x".join(map(str, bs)), a.nvec, a.nev, "Wilson" if a.no_clover else "Wilson-clover"),
           "reps": a.reps, "warmup": a.warmup, "ms_median": {k: round(v, 4) for k, v in med.items()},
           "ms_min": {k: round(float(np.min(v)), 4) for k, v in times.items()},
           "operator_GB": round(opbytes / 1e9, 3), "V_GB": round(vbytes / 1e9, 3),
           "build_Tflop_model": round(build_flop / 1e12, 3), "build_Tflops": round(build_flop / med["build"] / 1e9, 2),
           "build_GB_floor": round((vbytes + opbytes) / 1e9, 3),
           "apply_ms_per_block_of_8": round(med["apply_M_all"] / nblocks, 4), "apply_dagger_ms_per_block_of_8": round(med["apply_Mdag_all"] / nblocks, 4),
           "apply_GB_floor_per_block": round(opbytes / 1e9, 3), "apply_GBps_model": round(apply_floor / med["apply_M_all"] / 1e6, 1),
           "apply_dagger_GBps_model": round(apply_floor / med["apply_Mdag_all"] / 1e6, 1),
           "read_probe_GBps": round(opbytes / med["read_probe_operator"] / 1e6, 1),
           "apply_fraction_of_one_read": round(med["read_probe_operator"] * nblocks / med["apply_M_all"], 3),
           "apply_dagger_fraction_of_one_read": round(med["read_probe_operator"] * nblocks / med["apply_Mdag_all"], 3),
           "evals_ratio_fine_over_operator": round(med["evals_fine_route"] / med["evals_operator"], 2),
           "builds_amortised_after_checks": round(med["build"] / max(med["evals_fine_route"] - med["evals_operator"], 1e-9), 2),
           "max_rel_diff_between_routes": diff}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
