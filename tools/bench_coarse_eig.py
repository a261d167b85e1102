"""Time the coarse-grid eigensolver (mugiq_hip_coarse_eigensolve) on the hierarchy tools/bench_mg_setup.py makes:

    python tools/bench_coarse_eig.py [--lattice 32 32 32 32] [--block 4 4 4 4] [--nvec 24] [--nconv 200] [--nkr 256] [--out profiles/coarse_eig_latest.json]

The configuration is a random one (every link a random unitary matrix), Wilson-clover, the null vectors those of the MG setup from the
Gaussian start vectors of seed 13 (setupMaxIter 50), as in tools/bench_mg_setup.py.  Reported: the wall time of the whole solve, its
iterations, block applications of A and host reads, and the time per phase.  The solve is one call, so the phases are not timed inside it:
each device phase is timed on its own on buffers of the solve's shape (host clock around calls that end in a synchronise, medians of --reps
after a warm-up) and multiplied by the number of times the solve ran it, which follows from iters, nOrtho and opBlocks; the host's dense
work is the call's own hostDenseSeconds; `unaccounted` is the rest (pointer tables, launches, reads).  The Gram and rotation kernels are
given as fractions of the 78.6 TF fp64 matrix roof (8 real flops per complex multiply-add) and against torch.matmul on the same buffers in
the same run.  One JSON record is printed and written to --out."""
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

FP64_MATRIX_TF = 78.6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", type=int, nargs=4, default=[32, 32, 32, 32])
    ap.add_argument("--block", type=int, nargs=4, default=[4, 4, 4, 4])
    ap.add_argument("--nvec", type=int, default=24)
    ap.add_argument("--kappa", type=float, default=0.124)
    ap.add_argument("--csw-coeff", type=float, default=0.1)
    ap.add_argument("--setup-iters", type=int, default=50)
    ap.add_argument("--nconv", type=int, default=200)
    ap.add_argument("--nkr", type=int, default=256)
    ap.add_argument("--poly-deg", type=int, default=20)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "coarse_eig_latest.json"))
    a = ap.parse_args()
    X, bs = tuple(a.lattice), tuple(a.block)
    torch.cuda.set_device(0)
    gen = torch.Generator(device="cuda").manual_seed(12)
    vcb = int(np.prod(X)) // 2

    gauge = hip.GaugeField(X, (0, 0, 0, 0), 8)
    U = batched_q(torch.randn(8 * vcb, 3, 3, dtype=torch.complex128, device="cuda", generator=gen)).reshape(2, 4, vcb, 3, 3)
    gauge.data.view(2, 4, 9, vcb).copy_(U.reshape(2, 4, vcb, 9).permute(0, 1, 3, 2))
    del U
    C = hip.CloverField(X, 8).compute(gauge, a.csw_coeff)
    vecs = hip.mgStartVectors(X, a.nvec, seed=13)
    T, op, setup = hip.mgSetup(gauge, a.kappa, a.nvec, bs, start=vecs, clover=C, setupMaxIter=a.setup_iters)
    del vecs
    torch.cuda.empty_cache()

    def wall_ms(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t)

    def median_ms(fn):
        fn()
        return float(np.median([wall_ms(fn) for _ in range(a.reps)]))

    # ---- the solve
    start = hip.coarseStartVectors(op.X, a.nvec, a.nkr, seed=14)
    out = {}

    def solve():
        out["r"] = hip.coarseEigensolve(op, start=start, nConv=a.nconv, nKr=a.nkr, polyDeg=a.poly_deg, tol=a.tol, maxIter=a.max_iter, allow_unconverged=True)
    total_ms = wall_ms(solve)
    ev, theta, res, sigma, info = out["r"]
    lam, r2, _ = hip.computeEvalsCoarse(ev, opType=hip.MUGIQ_EIG_OPERATOR_MdagM, coarseOp=op)

    # ---- the phases, each on its own: buffers of the solve's shape
    m = a.nkr
    A = [hip.CoarseField(op.X, a.nvec, 8) for _ in range(m)]
    B = [hip.CoarseField(op.X, a.nvec, 8) for _ in range(m)]
    for f, s in zip(A, start):
        f.data.copy_(s.data)
    L = A[0].data.numel()
    Z = np.linalg.qr(np.random.default_rng(15).standard_normal((m, m)) + 1j * np.random.default_rng(16).standard_normal((m, m)))[0]
    ms = {"gram": median_ms(lambda: hip.coarseGram(A)),
          "rotate": median_ms(lambda: hip.coarseRotate(B, A, Z)),
          "apply_block_of_8": median_ms(lambda: hip.coarseApply(B[:8], A[:8], op, hip.MUGIQ_EIG_OPERATOR_MdagM)),
          "residual_norms_via_evals_check": median_ms(lambda: hip.computeEvalsCoarse(A[:8], opType=hip.MUGIQ_EIG_OPERATOR_MdagM, coarseOp=op))}
    At = torch.stack([f.data for f in A])                                               # [m, L]
    Zt = torch.from_numpy(Z).cuda()
    ms["torch_gram"] = median_ms(lambda: torch.matmul(At.conj(), At.T))
    ms["torch_rotate"] = median_ms(lambda: torch.matmul(Zt.T, At))
    Hm = np.random.default_rng(17).standard_normal((m, m)) + 1j * np.random.default_rng(18).standard_normal((m, m))
    t = time.perf_counter()
    hip.hermitianEigh(Hm + Hm.conj().T)
    host_eigh_ms = 1e3 * (time.perf_counter() - t)
    G = Hm.conj().T @ Hm
    t = time.perf_counter()
    hip.upperTriangularInverse(hip.choleskyUpper(G))
    host_chol_ms = 1e3 * (time.perf_counter() - t)
    H512 = np.random.default_rng(19).standard_normal((512, 512)) + 1j * np.random.default_rng(20).standard_normal((512, 512))
    t = time.perf_counter()
    hip.hermitianEigh(H512 + H512.conj().T)                                              # the largest nKr the call admits
    host_eigh_512_ms = 1e3 * (time.perf_counter() - t)

    flops = 8.0 * m * m * L
    n_rr = info.iters + 1
    n_gram = 2 * n_rr + n_rr                                                            # nOrtho 2 per orth, one per Rayleigh-Ritz step
    n_rot = 2 * n_rr + 2 * n_rr
    filter_blocks = info.opBlocks - 21 - n_rr * (m // 8)
    phases = {"filter_apply": filter_blocks * ms["apply_block_of_8"], "rayleigh_ritz_apply": n_rr * (m // 8) * ms["apply_block_of_8"],
              "power_iteration_apply": 21 * ms["apply_block_of_8"], "gram": n_gram * ms["gram"], "rotate": n_rot * ms["rotate"],
              "host_dense": 1e3 * info.hostDenseSeconds}
    phases["unaccounted"] = total_ms - sum(phases.values())
    rec = {"workload": "coarse eigensolve, %s fp64, aggregates %s, n_vec %d, Wilson-clover kappa %g, random unitary links, nConv %d, nKr %d, polyDeg %d, tol %g"
                       % ("x".join(map(str, X)), "x".join(map(str, bs)), a.nvec, a.kappa, a.nconv, a.nkr, a.poly_deg, a.tol),
           "coarse_dimension": int(L), "coarse_vector_MB": round(L * 16 / 1e6, 3), "total_ms": round(total_ms, 1), "converged": bool(info.converged),
           "iters": info.iters, "nConverged": info.nConverged, "opBlocks": info.opBlocks, "hostReads": info.hostReads,
           "aMaxUsed": info.aMaxUsed, "aMinLast": info.aMinLast, "orthonormality": info.orthonormality,
           "theta_min": float(theta[0]), "theta_max_returned": float(theta[-1]), "residual_max": float(np.max(res)),
           "independent_check_residual_max": float(np.max(r2)), "independent_check_lambda_diff_max": float(np.max(np.abs(lam - theta))),
           "unit_ms_median": {k: round(v, 3) for k, v in ms.items()}, "host_eigh_ms_n%d" % m: round(host_eigh_ms, 1),
           "host_cholesky_plus_inverse_ms_n%d" % m: round(host_chol_ms, 1), "host_eigh_ms_n512": round(host_eigh_512_ms, 1),
           "phase_ms_unit_times_count": {k: round(v, 1) for k, v in phases.items()},
           "phase_fraction": {k: round(v / total_ms, 3) for k, v in phases.items()},
           "gram_fraction_of_fp64_matrix_roof": round(flops / (ms["gram"] * 1e-3) / (FP64_MATRIX_TF * 1e12), 4),
           "rotate_fraction_of_fp64_matrix_roof": round(flops / (ms["rotate"] * 1e-3) / (FP64_MATRIX_TF * 1e12), 4),
           "gram_over_torch_matmul": round(ms["gram"] / ms["torch_gram"], 2), "rotate_over_torch_matmul": round(ms["rotate"] / ms["torch_rotate"], 2),
           "mg_setup": {"setupMaxIter": a.setup_iters, "orthonormality": setup.orthonormality, "minPivotRatio": setup.minPivotRatio}}
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
