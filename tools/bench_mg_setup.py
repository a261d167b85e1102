"""Time the MG setup on the device: the block orthonormalisation (mugiq_hip_block_orthonormalize) against the torch route that
tools/bench_mg_solve.py makes its null vectors with (null_vectors / batched_q: gather per aggregate, chunked torch.linalg.qr, scatter) on
the same vectors in the same run, and the whole mgSetup (CG null vectors, packing, orthonormalisation, coarse operator):

    python tools/bench_mg_setup.py [--lattice 32 32 32 32] [--block 4 4 4 4] [--nvec 24] [--setup-iters 50] [--out profiles/mg_setup_latest.json]

The configuration is a random one (every link a random unitary matrix), Wilson-clover, as in tools/bench_mg_solve.py.  Host clock around
calls that end in a synchronise (the orthonormalisation blocks the host itself: one read), medians of --reps after --warmup, the two routes
alternated.  The kernel is reported as a multiple of its byte floor -- one read and one write of V at 6.3 TB/s -- and as a ratio to the torch
route; the packing (setVectors), which the torch route contains, is timed beside it.  One JSON record is printed and written to --out."""
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

HBM_TBS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", type=int, nargs=4, default=[32, 32, 32, 32])
    ap.add_argument("--block", type=int, nargs=4, default=[4, 4, 4, 4])
    ap.add_argument("--nvec", type=int, default=24)
    ap.add_argument("--kappa", type=float, default=0.124)
    ap.add_argument("--csw-coeff", type=float, default=0.1)
    ap.add_argument("--setup-iters", type=int, default=50, help="setupMaxIter of the timed mgSetup (the library's default is 500)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mg_setup_latest.json"))
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

    def wall_ms(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t)

    # ---- the orthonormalisation: the kernel (packing timed apart) against the torch route, on the same vectors
    T, Tq = hip.Transfer(X, a.nvec, bs, 2, 8), hip.Transfer(X, a.nvec, bs, 2, 8)
    info = {}

    def ortho(n):
        def run():
            info[n] = T.blockOrthonormalize(n)
        return run

    parts = {"set_vectors": lambda: T.setVectors(vecs), "ortho_1_pass": ortho(1), "ortho_2_passes": ortho(2),
             "torch_route": lambda: null_vectors(Tq, vecs, X, bs)}
    ms = {k: [] for k in parts}
    for it in range(a.warmup + a.reps):
        for k in ("set_vectors", "ortho_1_pass", "torch_route"):
            t = wall_ms(parts[k])
            if it >= a.warmup:
                ms[k].append(t)
        T.setVectors(vecs)
        t = wall_ms(parts["ortho_2_passes"])
        if it >= a.warmup:
            ms["ortho_2_passes"].append(t)
    orth = {"kernel_2_passes": T.orthonormality(), "torch_route": Tq.orthonormality()}
    T.setVectors(vecs)
    T.blockOrthonormalize(1)
    orth["kernel_1_pass"] = T.orthonormality()
    diff = float(torch.max(torch.abs(torch.abs(T.V) - torch.abs(Tq.V))))          # QR fixes no phase: compare the moduli
    del Tq
    torch.cuda.empty_cache()

    # ---- the whole setup
    setup = {}

    def run_setup():
        setup["T"], setup["op"], setup["info"] = hip.mgSetup(gauge, a.kappa, a.nvec, bs, start=vecs, clover=C, transfer=T, coarseOp=setup.get("op", True),
                                                             setupMaxIter=a.setup_iters)
    run_setup()                                                                       # warm-up: allocations, first launches
    st = [wall_ms(run_setup) for _ in range(max(1, a.reps - 1))]
    op_ms = [wall_ms(lambda: hip.computeCoarseOperator(T, gauge, a.kappa, clover=C, op=setup["op"])) for _ in range(2)]
    si = setup["info"]

    med = {k: float(np.median(v)) for k, v in ms.items()}
    v_bytes = 2 * 12 * a.nvec * vcb * 16
    floor_ms = 2 * v_bytes / (HBM_TBS * 1e12) * 1e3
    m = 6 * int(np.prod(bs))
    # per block and pass: every finished column is read twice per later column (coefficients, update), every column read and written once
    model_bytes = (a.nvec * (a.nvec - 1) + 2 * a.nvec) * m * 16
    res = {"workload": "MG setup, %s fp64, aggregates %s, n_vec %d, Wilson-clover kappa %g, random unitary links, Gaussian start vectors"
                       % ("x".join(map(str, X)), "x".join(map(str, bs)), a.nvec, a.kappa),
           "reps": a.reps, "warmup": a.warmup, "ms_median": {k: round(v, 3) for k, v in med.items()},
           "ms_min": {k: round(float(np.min(v)), 3) for k, v in ms.items()},
           "V_GB": round(v_bytes / 1e9, 3), "byte_floor_ms": round(floor_ms, 3),
           "ortho_1_pass_over_floor": round(med["ortho_1_pass"] / floor_ms, 2), "ortho_2_passes_over_floor": round(med["ortho_2_passes"] / floor_ms, 2),
           "torch_route_over_pack_plus_ortho_2_passes": round(med["torch_route"] / (med["set_vectors"] + med["ortho_2_passes"]), 2),
           "torch_route_over_ortho_2_passes": round(med["torch_route"] / med["ortho_2_passes"], 2),
           "blocks": 2 * int(np.prod(X)) // int(np.prod(bs)), "rows_per_block": m,
           "model_cache_GB_per_pass": round(model_bytes * 2 * int(np.prod(X)) // int(np.prod(bs)) / 1e9, 2),
           "orthonormality": orth, "max_modulus_difference_kernel_vs_torch": diff,
           "minPivotRatio": {str(k): v[0] for k, v in info.items()}, "zeroColumns": {str(k): v[1] for k, v in info.items()},
           "mg_setup": {"setupMaxIter": a.setup_iters, "ms": [round(t, 1) for t in st], "coarse_operator_ms": round(float(np.min(op_ms)), 1),
                        "cgIters_max": int(np.max(si.cgIters)), "minPivotRatio": si.minPivotRatio, "zeroColumns": si.zeroColumns,
                        "orthonormality": si.orthonormality, "hostReads": si.hostReads, "cgHostReadsEstimate": si.cgHostReadsEstimate}}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
