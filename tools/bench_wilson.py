"""Time the fused, batched Wilson operator (mugiq_hip_wilson_apply) against the same M composed from what the library offered before
it: eight mugiq_hip_perform_covariant_displacement_vector calls per vector plus torch for the (1 -+ g_mu) sums, on the same buffers,
the two alternated in one process.  Also the cost of the eigenpair check (mugiq_hip_compute_evals) per eigenvector.

    python tools/bench_wilson.py [--lattice 32 32 32 32] [--nvec 8] [--reps 20] [--nev 200] [--no-composed] [--no-evals] [--clover]

--clover: also the Wilson-clover M (mugiq_hip_wilson_clover_apply), alternated with the unimproved M in the same loop, and one
mugiq_hip_compute_clover; the packed term adds 576 B per site and launch (fp64), 2112 -> 2688 B at four vectors a launch: 1.27 x.

Counted bytes of the fused kernel per site and vector (fp64): 192 (source, if the neighbours hit in cache) + 1152 / nVec-per-block
(links) + 192 (result); one JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mugiq_amd as hip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", type=int, nargs=4, default=[32, 32, 32, 32])
    ap.add_argument("--nvec", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nev", type=int, default=200, help="eigenvectors of the compute_evals timing")
    ap.add_argument("--kappa", type=float, default=0.12)
    ap.add_argument("--no-composed", action="store_true")
    ap.add_argument("--no-evals", action="store_true")
    ap.add_argument("--clover", action="store_true", help="time the Wilson-clover M beside the unimproved one, and compute_clover")
    ap.add_argument("--clover-coeff", type=float, default=0.15)
    a = ap.parse_args()
    X = tuple(a.lattice)
    V, vcb = int(np.prod(X)), int(np.prod(X)) // 2
    torch.cuda.set_device(0)
    gen = torch.Generator(device="cuda").manual_seed(11)
    gauge = hip.GaugeField(X, (0, 0, 0, 0), 8)
    gauge.data.copy_(torch.randn(gauge.data.numel(), dtype=torch.complex128, device="cuda", generator=gen) * 0.4)   # links need not be unitary
    src = [hip.SpinorField(X, 8, 2) for _ in range(a.nvec)]
    for f in src:
        f.data.copy_(torch.randn(f.data.numel(), dtype=torch.complex128, device="cuda", generator=gen))
    dst = [hip.SpinorField(X, 8, 2) for _ in range(a.nvec)]
    ref = [hip.SpinorField(X, 8, 2) for _ in range(a.nvec)]
    fwd, bwd = hip.SpinorField(X, 8, 2), hip.SpinorField(X, 8, 2)
    rv, ci, _, _ = hip.gammaTables()
    gam = []
    for n in (1, 2, 4, 8):
        g = np.zeros((4, 4), dtype=np.complex128)
        for i in range(4):
            g[i, ci[n, i]] = rv[n, i]
        gam.append(torch.from_numpy(g).cuda())
    one = torch.eye(4, dtype=torch.complex128, device="cuda")
    view = lambda f: f.data.view(2, 4, 3, vcb)

    def fused():
        hip.wilsonApply(dst, src, gauge, a.kappa)

    clover, t_setup = None, []
    if a.clover:
        clover = hip.CloverField(X, 8)
        dstc = [hip.SpinorField(X, 8, 2) for _ in range(a.nvec)]

    def fused_clover():
        hip.wilsonApply(dstc, src, gauge, a.kappa, clover=clover)

    def composed():
        for s, o in zip(src, ref):
            acc = view(s).clone()
            for mu in range(4):
                hip.performCovariantDisplacementVector(fwd, s, gauge, mu, hip.DispSignPlus)
                hip.performCovariantDisplacementVector(bwd, s, gauge, mu, hip.DispSignMinus)
                acc -= a.kappa * (torch.einsum("st,ptcx->pscx", one - gam[mu], view(fwd)) + torch.einsum("st,ptcx->pscx", one + gam[mu], view(bwd)))
            view(o).copy_(acc)

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    if a.clover:
        t_setup = [timed(lambda: clover.compute(gauge, a.clover_coeff)) for _ in range(3)]
    tf, tc, tcl = [], [], []
    for i in range(a.warmup + a.reps):
        f = timed(fused)
        if a.clover:
            cl = timed(fused_clover)
            if i >= a.warmup:
                tcl.append(cl)
        c = None if a.no_composed else timed(composed)
        if i >= a.warmup:
            tf.append(f)
            tc.append(c)
    nb = 4                                                    # vectors per workgroup block of the fp64 kernel (csrc/wilson.hip)
    bytes_model = V * a.nvec * (192 + 1152 / 8 + 192)        # the issue's count (links once per 8 vectors)
    bytes_block = V * a.nvec * (192 + 1152 / min(nb, a.nvec) + 192)
    med = statistics.median(tf)
    res = {"lattice": list(X), "nvec": a.nvec, "reps": a.reps, "fused_ms_median": round(med, 4), "fused_ms_min": round(min(tf), 4),
           "fused_ms_max": round(max(tf), 4), "TBps_on_528B": round(bytes_model / med / 1e9, 3),
           "frac_of_8TBps_on_528B": round(bytes_model / med / 1e9 / 8.0, 3), "TBps_on_block_count": round(bytes_block / med / 1e9, 3),
           "GFLOPs_1320_per_site": round(1320.0 * V * a.nvec / med / 1e6, 1)}
    if a.clover:
        mcl = statistics.median(tcl)
        res.update({"clover_ms_median": round(mcl, 4), "clover_ms_min": round(min(tcl), 4), "clover_ms_max": round(max(tcl), 4),
                    "clover_over_wilson": round(mcl / med, 3), "clover_over_wilson_byte_model": round((2112 + 576) / 2112, 3),
                    "compute_clover_ms_first": round(t_setup[0], 3), "compute_clover_ms": round(min(t_setup[1:]), 3)})
    if not a.no_composed:
        mc = statistics.median(tc)
        res.update({"composed_ms_median": round(mc, 3), "composed_ms_min": round(min(tc), 3), "composed_ms_max": round(max(tc), 3),
                    "composed_over_fused": round(mc / med, 2),
                    "max_rel_diff": float(max((d.data - r.data).abs().max() / r.data.abs().max() for d, r in zip(dst, ref)))})
    if not a.no_evals:
        del ref, fwd, bwd
        ev = [hip.SpinorField(X, 8, 2) for _ in range(a.nev)]
        for f in ev:
            f.data.copy_(torch.randn(f.data.numel(), dtype=torch.complex128, device="cuda", generator=gen) / np.sqrt(12 * V))
        hip.computeEvals(ev[:8], gauge, a.kappa, hip.MUGIQ_EIG_OPERATOR_MdagM)
        for op, name in ((hip.MUGIQ_EIG_OPERATOR_MdagM, "MdagM"), (hip.MUGIQ_EIG_OPERATOR_H, "H")):
            ms = timed(lambda: hip.computeEvals(ev, gauge, a.kappa, op))
            res["compute_evals_%s_ms_per_eigenvector" % name] = round(ms / a.nev, 3)
        res["compute_evals_nev"] = a.nev
    print(json.dumps(res))


if __name__ == "__main__":
    main()
