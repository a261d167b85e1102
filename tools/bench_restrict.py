"""Time the restriction and the two routes of low-mode deflation for an MG eigenvector set (coarse eigenvectors w_n, v_n = P w_n):

    python tools/bench_restrict.py [--lattice 32 32 32 32] [--block 4 4 4 4] [--nvec 24] [--nev 200] [--nrhs 8] [--out profiles/restrict_latest.json]

  (a) restrictVecs of the right-hand sides,
  (b) deflateLowModesCoarse: through the coarse space, no fine eigenvector stored,
  (c) deflateLowModes on the vectors prolonged beforehand (prolongateEvecs timed separately): the fine route.
Event times, --reps repetitions after --warmup runs, (b) and (c) alternated; medians.  GB/s on the byte model of DESIGN.md: V once per
restriction and once per prolong-and-update pass, the fine vectors read / read and written, the coarse vectors twice; the fine route
reads the N_ev fine eigenvectors twice.  One JSON record is printed and written to --out."""
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
    ap.add_argument("--nrhs", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "restrict_latest.json"))
    a = ap.parse_args()
    X, bs = tuple(a.lattice), tuple(a.block)
    torch.cuda.set_device(0)
    gen = torch.Generator(device="cuda").manual_seed(9)
    vol = int(np.prod(X))

    def fill(t, scale):
        step = 1 << 26
        for i in range(0, t.numel(), step):
            t[i:i + step].copy_(torch.randn(min(step, t.numel() - i), dtype=t.dtype, device="cuda", generator=gen) * scale)

    T = hip.Transfer(X, a.nvec, bs, 2, 8)
    fill(T.V, 1.0 / np.sqrt(12.0 * a.nvec))
    cw = [hip.CoarseField(T.Xc, a.nvec, 8) for _ in range(a.nev)]
    for w in cw:
        fill(w.data, 1.0 / np.sqrt(w.data.numel()))
    sg = list(0.5 + np.arange(a.nev) * 1e-3)
    src = [hip.SpinorField(X, 8, 2) for _ in range(a.nrhs)]
    for s in src:
        fill(s.data, 1.0)
    dst_b = [hip.SpinorField(X, 8, 2) for _ in range(a.nrhs)]
    dst_c = [hip.SpinorField(X, 8, 2) for _ in range(a.nrhs)]
    y = [hip.CoarseField(T.Xc, a.nvec, 8) for _ in range(a.nrhs)]
    fv = [hip.SpinorField(X, 8, 2) for _ in range(a.nev)]

    def event_ms(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    routes = {
        "restrict": lambda: hip.restrictVecs(y, src, T, gamma5=True),
        "deflate_coarse": lambda: hip.deflateLowModesCoarse(dst_b, src, cw, T, sg, gamma5=True),
        "prolongate": lambda: hip.prolongateEvecs(fv, cw, T),
        "deflate_fine": lambda: hip.deflateLowModes(dst_c, src, fv, sg, gamma5=True),
        "read_probe_V": lambda: hip.probeReadBandwidth(T.V),
    }
    times = {k: [] for k in routes}
    for it in range(a.warmup + a.reps):
        for k in ("prolongate", "deflate_coarse", "deflate_fine", "restrict", "read_probe_V"):      # the two routes alternate
            ms = event_ms(routes[k])
            if it >= a.warmup:
                times[k].append(ms)
    med = {k: float(np.median(v)) for k, v in times.items()}
    # one call of each route from the same dst: the two results agree
    for d, e in zip(dst_b, dst_c):
        d.data.copy_(src[0].data)
        e.data.copy_(src[0].data)
    routes["deflate_coarse"]()
    routes["deflate_fine"]()
    torch.cuda.synchronize()
    diff = max(float((d.data - e.data).abs().max()) for d, e in zip(dst_b, dst_c))

    cb = 16                                                   # bytes of a complex double
    vbytes = 12 * a.nvec * cb * vol
    fine = 12 * cb * vol
    coarse = 2 * a.nvec * cb * (vol // int(np.prod(bs)))
    b_restrict = vbytes + a.nrhs * fine + a.nrhs * coarse
    b_coarse = b_restrict + (a.nev + 2 * a.nrhs) * coarse * 2 + vbytes + 2 * a.nrhs * fine + a.nrhs * coarse
    b_fine = 2 * a.nev * fine + 3 * a.nrhs * fine
    res = {"workload": "deflation of %d right-hand sides against %d MG eigenvectors, %s fp64, aggregates %s, n_vec %d"
                       % (a.nrhs, a.nev, "x".join(map(str, X)), "x".join(map(str, bs)), a.nvec),
           "reps": a.reps, "warmup": a.warmup, "ms_median": {k: round(v, 4) for k, v in med.items()},
           "ms_min": {k: round(float(np.min(v)), 4) for k, v in times.items()},
           "GB_model": {"restrict": round(b_restrict / 1e9, 3), "deflate_coarse": round(b_coarse / 1e9, 3), "deflate_fine": round(b_fine / 1e9, 3),
                        "V": round(vbytes / 1e9, 3)},
           "GBps_model": {"restrict": round(b_restrict / med["restrict"] / 1e6, 1), "deflate_coarse": round(b_coarse / med["deflate_coarse"] / 1e6, 1),
                          "deflate_fine": round(b_fine / med["deflate_fine"] / 1e6, 1), "read_probe_V": round(vbytes / med["read_probe_V"] / 1e6, 1)},
           "model_ratio_fine_over_coarse": round(b_fine / b_coarse, 3),
           "measured_ratio_fine_over_coarse": round(med["deflate_fine"] / med["deflate_coarse"], 3),
           "restrict_over_V_read_once": round(med["restrict"] / med["read_probe_V"], 3),
           "max_abs_diff_between_routes": diff}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
