"""Time the explicit coarse operator on a process grid against the unpartitioned calls, on one GPU, in one run:

    python tools/bench_coarse_op_grid.py [--lattice 32 32 32 32] [--block 4 4 4 4] [--nvec 24] [--out profiles/coarse_op_grid_latest.json]

For the partitionings z + t and x + y + z + t, forced on one rank (GridComm(force_partitioned=): the rank is its own neighbour, every message
a device copy issued from the comm's Python callback -- the pack kernels, the ghost path of the two kernels and the host side of the
exchange are measured, a link is not):
  (a) computeCoarseOperatorGrid: faces of V exchanged, the build with the ghost path, the Y faces exchanged into the halo,
  (b) coarseApplyGrid of M and of MdagM on one block of 8 vectors: faces packed and exchanged, one launch (MdagM: twice),
and, on the same fields, the unpartitioned computeCoarseOperator and coarseApply they are compared with.  The results must be bit-equal
(asserted, and recorded).  Event times around calls that end in a synchronise, --reps repetitions after --warmup runs, partitioned and
unpartitioned calls alternated; medians and their ratios.  One JSON record is printed and written to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mugiq_amd as hip  # noqa: E402

PARTITIONINGS = {"zt": (0, 0, 1, 1), "xyzt": (1, 1, 1, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", type=int, nargs=4, default=[32, 32, 32, 32])
    ap.add_argument("--block", type=int, nargs=4, default=[4, 4, 4, 4])
    ap.add_argument("--nvec", type=int, default=24)
    ap.add_argument("--kappa", type=float, default=0.12)
    ap.add_argument("--no-clover", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "coarse_op_grid_latest.json"))
    a = ap.parse_args()
    X, bs = tuple(a.lattice), tuple(a.block)
    torch.cuda.set_device(0)
    gen = torch.Generator(device="cuda").manual_seed(13)
    N = 2 * a.nvec

    def fill(t, scale):
        step = 1 << 26
        for i in range(0, t.numel(), step):
            t[i:i + step].copy_(torch.randn(min(step, t.numel() - i), dtype=t.dtype, device="cuda", generator=gen) * scale)

    def event_ms(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    def same(x, y):
        return bool(torch.equal(x.view(torch.float64).view(torch.int64), y.view(torch.float64).view(torch.int64)))

    T = hip.Transfer(X, a.nvec, bs, 2, 8)
    fill(T.V, 1.0 / np.sqrt(12.0 * a.nvec * int(np.prod(bs))))
    cw = [hip.CoarseField(T.Xc, a.nvec, 8) for _ in range(8)]
    for w in cw:
        fill(w.data, 1.0 / np.sqrt(w.data.numel()))
    out0 = [hip.CoarseField(T.Xc, a.nvec, 8) for _ in range(8)]
    out1 = [hip.CoarseField(T.Xc, a.nvec, 8) for _ in range(8)]
    op0, op1 = hip.CoarseOperator(T.Xc, a.nvec, 8), hip.CoarseOperator(T.Xc, a.nvec, 8)
    M, MdagM = hip.MUGIQ_EIG_OPERATOR_M, hip.MUGIQ_EIG_OPERATOR_MdagM
    cb = 16
    res = {"workload": "explicit coarse operator on a forced partition of one rank, %s fp64, aggregates %s, n_vec %d, blocks of 8 vectors, %s"
                       % ("x".join(map(str, X)), "x".join(map(str, bs)), a.nvec, "Wilson" if a.no_clover else "Wilson-clover"),
           "reps": a.reps, "warmup": a.warmup, "operator_GB": round(2 * op0.volumeCB * 9 * N * N * cb / 1e9, 3), "partitionings": {}}
    for name, force in PARTITIONINGS.items():
        comm = hip.GridComm((1, 1, 1, 1), device="cuda:0", force_partitioned=force)
        # one gauge field with a border for both routes: the unpartitioned call reads the same links through the border
        gauge = hip.GaugeField(X, force, 8)
        fill(gauge.data, 1.0 / np.sqrt(6.0))
        gauge.exchangeBorders(comm)
        C = None if a.no_clover else hip.CloverField(X, 8).compute(gauge, 0.1, comm)
        routes = {
            "build": lambda: hip.computeCoarseOperator(T, gauge, a.kappa, clover=C, op=op0),
            "build_grid": lambda: hip.computeCoarseOperatorGrid(T, gauge, a.kappa, comm, clover=C, op=op1),
            "apply_M": lambda: hip.coarseApply(out0, cw, op0, M),
            "apply_M_grid": lambda: hip.coarseApplyGrid(out1, cw, op1, comm, M),
            "apply_MdagM": lambda: hip.coarseApply(out0, cw, op0, MdagM),
            "apply_MdagM_grid": lambda: hip.coarseApplyGrid(out1, cw, op1, comm, MdagM),
        }
        times = {k: [] for k in routes}
        equal = {}
        for it in range(a.warmup + a.reps):
            for k in routes:
                ms = event_ms(routes[k])
                if it >= a.warmup:
                    times[k].append(ms)
                if k == "build_grid":
                    equal["matrices"] = same(op0.data, op1.data)
                elif k.endswith("_grid"):
                    equal[k[:-5]] = all(same(x.data, y.data) for x, y in zip(out0, out1))
        assert all(equal.values()) and len(equal) == 3, (name, equal)
        med = {k: float(np.median(v)) for k, v in times.items()}
        faceCB = [op0.volumeCB // x for x in op0.X]
        vec_halo = sum(2 * 8 * 2 * N * faceCB[d] * cb for d in range(4) if force[d])          # received per launch
        V_halo = sum(2 * 2 * 12 * a.nvec * (T.volumeCB // X[d]) * cb for d in range(4) if force[d])
        Y_halo = sum(2 * 2 * faceCB[d] * N * N * cb for d in range(4) if force[d])
        res["partitionings"][name] = {
            "force_partitioned": list(force), "ms_median": {k: round(v, 4) for k, v in med.items()},
            "ms_min": {k: round(float(np.min(v)), 4) for k, v in times.items()},
            "ratio_grid_over_unpartitioned": {k: round(med[k + "_grid"] / med[k], 3) for k in ("build", "apply_M", "apply_MdagM")},
            "messages_per_launch": 2 * sum(force), "vector_halo_MB_per_launch": round(vec_halo / 1e6, 3),
            "V_halo_GB": round(V_halo / 1e9, 3), "Y_halo_MB": round(Y_halo / 1e6, 3), "bit_equal": equal}
        del gauge, C, comm
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
