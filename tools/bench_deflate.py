"""Time low-mode deflation (mugiq_hip_deflate_low_modes) at a given per-GPU size and compare it with the same two products through
torch.matmul on complex views of the same buffers.

    python tools/bench_deflate.py --lattice 48 48 24 24 --nev 400 --nvec 12 [--prec 8] [--order 2] [--src-prec 8]

Counted bytes: the eigenvectors twice (one pass each), src once, dst read and written.  The eigenvectors are one allocation with
stride == volumeCB (no pad), so with FLOAT2 a field is one contiguous row of 12 V complex numbers and the whole set is an [nEv, 12 V]
matrix -- the view the matmul yardstick works on (gamma5 applied as a sign vector on the src rows)."""
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
    ap.add_argument("--lattice", type=int, nargs=4, default=[48, 48, 24, 24])
    ap.add_argument("--nev", type=int, default=400)
    ap.add_argument("--nvec", type=int, default=12)
    ap.add_argument("--prec", type=int, default=8, choices=[4, 8], help="eigenvector precision")
    ap.add_argument("--order", type=int, default=2, choices=[2, 4])
    ap.add_argument("--src-prec", type=int, default=None, choices=[4, 8], help="src / dst precision (default: --prec)")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-matmul", action="store_true", help="skip the torch.matmul yardstick")
    a = ap.parse_args()
    sp = a.src_prec or a.prec
    X = tuple(a.lattice)
    torch.cuda.set_device(0)
    V = int(np.prod(X))
    K = 12 * V
    cdt = lambda p: torch.complex128 if p == 8 else torch.complex64
    gen = torch.Generator(device="cuda").manual_seed(5)
    evbuf = torch.empty(a.nev, K, dtype=cdt(a.prec), device="cuda")
    for n in range(a.nev):                                   # row by row: no full-size temporaries
        evbuf[n].copy_(torch.randn(K, dtype=cdt(a.prec), device="cuda", generator=gen) / np.sqrt(K))
    srcbuf = torch.randn(a.nvec, K, dtype=cdt(sp), device="cuda", generator=gen)
    dst0 = torch.randn(a.nvec, K, dtype=cdt(sp), device="cuda", generator=gen)
    dstbuf = dst0.clone()
    ev = [hip.SpinorField(X, a.prec, a.order, data=evbuf[n]) for n in range(a.nev)]
    src = [hip.SpinorField(X, sp, a.order, data=srcbuf[r]) for r in range(a.nvec)]
    dst = [hip.SpinorField(X, sp, a.order, data=dstbuf[r]) for r in range(a.nvec)]
    sg = list(0.5 + np.arange(a.nev) * 1e-3)

    def timed(fn, iters):
        fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / iters

    ms = timed(lambda: hip.deflateLowModes(dst, src, ev, sg, gamma5=True), a.iters)
    eb, sb = 2 * a.prec * K, 2 * sp * K
    bytes_ = 2 * a.nev * eb + a.nvec * sb + 2 * a.nvec * sb
    flops = 2 * 8 * 12 * V * a.nev * a.nvec
    res = {"lattice": list(X), "nev": a.nev, "nvec": a.nvec, "prec": a.prec, "order": a.order, "src_prec": sp,
           "ms_per_call": round(ms, 3), "ms_per_pass_avg": round(ms / 2, 3), "GB_counted": round(bytes_ / 1e9, 2),
           "TBps": round(bytes_ / ms / 1e9, 3), "frac_of_8TBps": round(bytes_ / ms / 1e9 / 8.0, 3), "GFLOPs": round(flops / ms / 1e6, 1)}
    if not a.no_matmul and a.order == 2:
        # sign of gamma5 per element of a FLOAT2 field: [parity][component k = 3 s + c][x_cb], spins 2, 3 negative
        vcb = V // 2
        g5 = torch.ones(2, 12, vcb, dtype=torch.float64 if a.prec == 8 else torch.float32, device="cuda")
        g5[:, 6:, :] = -1.0
        g5 = g5.reshape(-1)
        inv = torch.tensor([1.0 / s for s in sg], dtype=g5.dtype, device="cuda")
        ydst = dst0.clone().to(cdt(a.prec))
        ysrc = srcbuf.to(cdt(a.prec))

        def yard():
            C = torch.matmul(evbuf, (ysrc * g5).conj().T).conj()          # [nEv][nVec] = V^dag g5 src
            ydst.sub_(torch.matmul((C * inv[:, None]).T, evbuf))
        mt = timed(yard, a.iters)
        # one call of each from the same dst
        dstbuf.copy_(dst0)
        hip.deflateLowModes(dst, src, ev, sg, gamma5=True)
        ydst.copy_(dst0.to(cdt(a.prec)))
        yard()
        torch.cuda.synchronize()
        res["matmul_ms_per_call"] = round(mt, 3)
        res["speedup_vs_matmul"] = round(mt / ms, 3)
        res["max_abs_diff_vs_matmul"] = float((dstbuf.to(cdt(a.prec)) - ydst).abs().max())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
