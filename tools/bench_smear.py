"""Time one stout step (mugiq_hip_stout_smear: spatial and 4D), the device-side border refresh (mugiq_hip_exchange_extended_gauge) and
the plaquette (mugiq_hip_plaquette) with HIP events, fp64 storage, beside mugiq_hip_compute_clover on the same links in the same process:
a set-up kernel of comparable shape over the same field (six planes of four leaves, 96 link loads per site; one 4D stout step: 76 link
loads and four exponentials per site), the yardstick of the ratios.

    python tools/bench_smear.py [--lattice 32 32 32 32 --lattice 48 48 24 24] [--reps 10] [--out profiles/bench_smear.json]

Counted per link of a 4D step (fp64): 19 link loads and one store, 2880 B if nothing hits in cache, 288 B if every link comes from HBM
once; 12 products for the staples and 3 for Omega, Q^2 and exp(iQ) U, about 3500 flops.  The border refresh is timed as a periodic wrap
of a field with a border of 2 along z and t (no transport).  The plaquette time includes the copy of the result to the host.  One JSON
line per lattice."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mugiq_amd as hip  # noqa: E402


def random_su3_field(X, R, gen):
    """a GaugeField of seeded random SU(3) links on every extended site (then made periodic by the border refresh)"""
    g = hip.GaugeField(X, R, 8)
    n = 4 * 2 * g.volumeExCB
    m = torch.complex(torch.randn(n, 3, 3, dtype=torch.float64, device="cuda", generator=gen),
                      torch.randn(n, 3, 3, dtype=torch.float64, device="cuda", generator=gen))
    r0 = m[:, 0] / torch.linalg.vector_norm(m[:, 0], dim=-1, keepdim=True)
    r1 = m[:, 1] - (r0.conj() * m[:, 1]).sum(-1, keepdim=True) * r0
    r1 = r1 / torch.linalg.vector_norm(r1, dim=-1, keepdim=True)
    r2 = torch.linalg.cross(r0.conj(), r1.conj())
    u = torch.stack([r0, r1, r2], dim=1).reshape(4, 2, g.volumeExCB, 9)                 # dir, parity, x, component
    g.data.view(2, 4, 9, g.stride)[..., :g.volumeExCB].copy_(u.permute(1, 0, 3, 2))
    return g.exchangeBorders()


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def bench(X, reps, warmup, rho):
    V = int(np.prod(X))
    gen = torch.Generator(device="cuda").manual_seed(11)
    g = random_su3_field(X, (0, 0, 0, 0), gen)
    out = hip.GaugeField(X, (0, 0, 0, 0), 8)
    clover = hip.CloverField(X, 8)
    gb = random_su3_field(X, (0, 0, 2, 2), gen)
    runs = {"stout_3d_step": lambda: g.stoutSmear(rho, 1, 3, out=out),
            "stout_4d_step": lambda: g.stoutSmear(rho, 1, 4, out=out),
            "border_refresh_zt2": lambda: gb.exchangeBorders(),
            "plaquette": lambda: g.plaquette(),
            "compute_clover": lambda: clover.compute(g, 0.15)}
    t = {k: [] for k in runs}
    for i in range(warmup + reps):                                                  # alternated, so that drift hits all alike
        for k, fn in runs.items():
            ms = timed(fn)
            if i >= warmup:
                t[k].append(ms)
    res = {"lattice": list(X), "precision": 8, "reps": reps, "rho": rho, "plaquette_before": g.plaquette()[0],
           "plaquette_after_4d_step": g.stoutSmear(rho, 1, 4, out=out).plaquette()[0]}
    ref = statistics.median(t["compute_clover"])
    for k in runs:
        med = statistics.median(t[k])
        res[k + "_ms_median"] = round(med, 4)
        res[k + "_ms_min"] = round(min(t[k]), 4)
        res[k + "_ms_max"] = round(max(t[k]), 4)
        if k != "compute_clover":
            res[k + "_over_compute_clover"] = round(med / ref, 3)
    med4 = statistics.median(t["stout_4d_step"])
    res["stout_4d_GBps_on_2880B_per_link"] = round(4 * V * 2880 / med4 / 1e6, 1)
    res["stout_4d_GBps_on_288B_per_link"] = round(4 * V * 288 / med4 / 1e6, 1)
    res["stout_4d_GFLOPs_on_3500_per_link"] = round(4 * V * 3500 / med4 / 1e6, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", type=int, nargs=4, action="append", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rho", type=float, default=0.1)
    ap.add_argument("--out", default="", help="also write the results, as a JSON list, to this file")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    results = []
    for X in (a.lattice or [[32, 32, 32, 32], [48, 48, 24, 24]]):
        results.append(bench(tuple(X), a.reps, a.warmup, a.rho))
        print(json.dumps(results[-1]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
