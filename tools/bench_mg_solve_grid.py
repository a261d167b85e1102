"""Time the two-grid cycle and solve on a process grid against the single-domain calls, on one GPU, in one run:

    python tools/bench_mg_solve_grid.py [--lattice 32 32 32 32] [--block 4 4 4 4] [--nvec 24] [--nrhs 8] [--out profiles/mg_solve_grid_latest.json]

The fields are those of tools/bench_mg_solve.py: random unitary links, Wilson-clover, crude null vectors (a few CG iterations on random
sources, a QR per aggregate and chirality).  For the partitionings z + t and x + y + z + t, forced on one rank (GridComm(force_partitioned=):
the rank is its own neighbour, every message a device copy issued from the comm's Python callback), two routes on the same fields:
  single   mgPrecondition / mgSolve,
  grid     mgPreconditionGrid / mgSolveGrid.
One K on the block of right-hand sides and one solve each, alternated, wall times around calls that end in a synchronise, --reps
repetitions after --warmup runs; medians and the ratio grid / single of the same run.  The results of the two routes must be the same
bits (asserted, and recorded).  What this measures: the face packs of the stencil and of the coarse application, their ghost paths, the
copies and the host side of the exchanges.  What it does not: any sum over the ranks (one rank makes none: rankSums is 0), a real link,
more than one GPU.  One JSON record is printed and written to --out."""
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

PARTITIONINGS = {"zt": (0, 0, 1, 1), "xyzt": (1, 1, 1, 1)}


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
    ap.add_argument("--nKrylov", type=int, default=8)     # 16 with ghost zones on four axes: 72 GB of directions at 32^4
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mg_solve_grid_latest.json"))
    a = ap.parse_args()
    X, bs = tuple(a.lattice), tuple(a.block)
    torch.cuda.set_device(0)
    gen = torch.Generator(device="cuda").manual_seed(12)
    prm = dict(nKrylov=a.nKrylov)

    def crandn(*shape):
        return torch.randn(*shape, dtype=torch.complex128, device="cuda", generator=gen)

    def random_fields(n):
        out = []
        for _ in range(n):
            f = hip.SpinorField(X, 8, 2)
            f.data.copy_(crandn(f.data.numel()))
            out.append(f)
        return out

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def bits(fields):
        return [torch.view_as_real(f.data).view(torch.int64) for f in fields]

    def same(x, y):
        return all(bool(torch.equal(p, q)) for p, q in zip(bits(x), bits(y)))

    b = random_fields(a.nrhs)
    p = hip.mgSolveParam(tol=a.tol, maxIter=a.max_iter, **prm)
    res = {"workload": "two-grid cycle and solve on a forced partition of one rank, %s fp64, aggregates %s, n_vec %d, %d right-hand sides, Wilson-clover "
                       "kappa %g, random unitary links, crude null vectors" % ("x".join(map(str, X)), "x".join(map(str, bs)), a.nvec, a.nrhs, a.kappa),
           "param": {n: getattr(p, n) for n, _ in p._fields_}, "reps": a.reps, "warmup": a.warmup,
           "not_measured": ["any sum over the ranks (rankSums is 0 on one rank)", "a real link", "more than one GPU"], "partitionings": {}}
    for name, force in PARTITIONINGS.items():
        # one gauge field for both routes, with a border on the forced axes (the single-domain calls take it as it is): random unitary
        # links everywhere, then the borders from the interior; clover, crude null vectors and both coarse operators from it
        comm = hip.GridComm((1, 1, 1, 1), device="cuda:0", force_partitioned=force)
        gauge = hip.GaugeField(X, force, 8)
        ve = gauge.stride
        U = batched_q(crandn(8 * ve, 3, 3)).reshape(2, 4, ve, 3, 3)
        gauge.data.view(2, 4, 9, ve).copy_(U.reshape(2, 4, ve, 9).permute(0, 1, 3, 2))
        del U
        gauge.exchangeBorders(comm)
        C = hip.CloverField(X, 8).compute(gauge, a.csw_coeff, comm)
        src = random_fields(a.nvec)
        nv, _ = hip.wilsonSolve(src, gauge, a.kappa, tol=1e-12, maxIter=a.setup_iters, allow_unconverged=True, clover=C)
        T = hip.Transfer(X, a.nvec, bs, 2, 8)
        null_vectors(T, nv, X, bs)
        del src, nv
        op0 = hip.computeCoarseOperator(T, gauge, a.kappa, clover=C)
        op1 = hip.computeCoarseOperatorGrid(T, gauge, a.kappa, comm, clover=C)
        z = {r: [hip.SpinorField(X, 8, 2) for _ in b] for r in ("single", "grid")}
        x = {r: [hip.SpinorField(X, 8, 2) for _ in b] for r in ("single", "grid")}
        calls = {
            ("single", "K"): lambda: hip.mgPrecondition(z["single"], b, gauge, a.kappa, T, op0, clover=C, **prm),
            ("grid", "K"): lambda: hip.mgPreconditionGrid(z["grid"], b, gauge, a.kappa, T, op1, comm, clover=C, **prm),
            ("single", "solve"): lambda: hip.mgSolve(b, gauge, a.kappa, T, op0, clover=C, x=x["single"], tol=a.tol, maxIter=a.max_iter, allow_unconverged=True, **prm),
            ("grid", "solve"): lambda: hip.mgSolveGrid(b, gauge, a.kappa, T, op1, comm, clover=C, x=x["grid"], tol=a.tol, maxIter=a.max_iter,
                                                       allow_unconverged=True, **prm),
        }
        times, last = {k: [] for k in calls}, {}
        for it in range(a.warmup + a.reps):
            for what in ("K", "solve"):
                for route in ("single", "grid"):                           # alternated
                    ms, out = wall_ms(calls[route, what])
                    last[route, what] = out
                    if it >= a.warmup:
                        times[route, what].append(ms)
        med = {k: float(np.median(v)) for k, v in times.items()}
        i0, (i1, g1) = last["single", "solve"][1], last["grid", "solve"][1:]
        equal = {"K": same(z["single"], z["grid"]),
                 "solve": same(x["single"], x["grid"]) and np.array_equal(i0.iters, i1.iters) and np.array_equal(i0.relres, i1.relres)
                 and all(np.array_equal(h, k) for h, k in zip(i0.history, i1.history)) and i0.hostReads == i1.hostReads}
        assert all(equal.values()), (name, equal)
        res["partitionings"][name] = {
            "force_partitioned": list(force),
            "ms_median": {"%s_%s" % k: round(v, 3) for k, v in med.items()},
            "ms_min": {"%s_%s" % k: round(float(np.min(v)), 3) for k, v in times.items()},
            "ratio_grid_over_single": {"K": round(med["grid", "K"] / med["single", "K"], 4), "solve": round(med["grid", "solve"] / med["single", "solve"], 4)},
            "iters": [int(i) for i in i1.iters], "converged": bool(i1.converged), "hostReads": i1.hostReads,
            "grid_info_solve": dict(g1._asdict()), "bit_equal": equal}
        del gauge, comm, op0, op1, C, T, z, x
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
