"""Time the two-grid preconditioned GCR (mugiq_hip_mg_solve) against the plain CG (mugiq_hip_wilson_solve) on the same right-hand sides, and
one preconditioner K against the operator launches it contains, in one run:

    python tools/bench_mg_solve.py [--lattice 32 32 32 32] [--block 4 4 4 4] [--nvec 24] [--nrhs 8] [--out profiles/mg_solve_latest.json]

The configuration is a random one (every link a random unitary matrix), Wilson-clover.  The null vectors are made here and are crude: a few
CG iterations (wilsonSolve, allow_unconverged) on random sources, both chiralities of every vector kept (the chirality split is the coarse
spin index), then a QR per aggregate and chirality in torch.  A real MG setup is out of scope; these vectors decide the iteration counts.
  (a) mgSolve and wilsonSolve on the same --nrhs right-hand sides to the same tolerance, alternated, host clock around calls that end in a
      synchronise (both block the host themselves), medians of --reps after --warmup;
  (b) mgPrecondition (one K on the block) against the sum of its operator launches timed alone in this run with device events around loops of 20 to 40 calls (5 for K): nuPre +
      nuPost + 1 stencils, one restriction, one prolongation and coarseIters coarse applications.
Byte model, computed here from the shapes: what the Krylov kernels of one MR step and of one outer iteration move.
One JSON record is printed and written to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mugiq_amd as hip  # noqa: E402


def site_coords(X, device):
    """[2, volumeCB, 4] coordinates of the even-odd sites (QUDA's getCoords)"""
    vcb = int(np.prod(X)) // 2
    x_cb = torch.arange(vcb, device=device)
    out = []
    for parity in range(2):
        za = x_cb // (X[0] // 2)
        zb = za // X[1]
        c1 = za - zb * X[1]
        c3 = zb // X[2]
        c2 = zb - c3 * X[2]
        c0 = 2 * x_cb + ((c1 + c2 + c3 + parity) & 1) - za * X[0]
        out.append(torch.stack([c0, c1, c2, c3], dim=-1))
    return torch.stack(out)


def batched_q(A, chunk=1 << 16):
    """the Q factor of a batch of matrices [n, rows, cols], a chunk of the batch at a time (the batched solver's work memory grows with n)"""
    Q = torch.empty_like(A)
    for i in range(0, A.shape[0], chunk):
        Q[i:i + chunk] = torch.linalg.qr(A[i:i + chunk])[0]
    return Q


def null_vectors(T, vecs, X, bs):
    """fill T.V from the fine vectors: V(x; s, c, j) = vecs[j](x; s, c), orthonormalised per aggregate and chirality"""
    nvec, vcb = len(vecs), int(np.prod(X)) // 2
    W = torch.stack([v.data.view(2, 12, vcb) for v in vecs], dim=-1).permute(0, 2, 1, 3).reshape(2 * vcb, 2, 6, nvec)     # [site, chirality, 6, j]
    c = site_coords(X, W.device).reshape(2 * vcb, 4)
    Xc = [X[d] // bs[d] for d in range(4)]
    agg = ((c[:, 3] // bs[3] * Xc[2] + c[:, 2] // bs[2]) * Xc[1] + c[:, 1] // bs[1]) * Xc[0] + c[:, 0] // bs[0]
    order = torch.argsort(agg, stable=True)
    aggVol, nAgg = int(np.prod(bs)), int(np.prod(Xc))
    A = W[order].reshape(nAgg, aggVol, 2, 6, nvec).permute(0, 2, 1, 3, 4).reshape(nAgg, 2, aggVol * 6, nvec)
    Q = batched_q(A.reshape(2 * nAgg, aggVol * 6, nvec), 1 << 10)
    Wq = torch.empty_like(W)
    Wq[order] = Q.reshape(nAgg, 2, aggVol, 6, nvec).permute(0, 2, 1, 3, 4).reshape(2 * vcb, 2, 6, nvec)
    T.V.view(2, 12, nvec, vcb).copy_(Wq.reshape(2, vcb, 12, nvec).permute(0, 2, 3, 1))


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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mg_solve_latest.json"))
    for name in ("nKrylov", "nuPre", "nuPost", "coarseIters"):
        ap.add_argument("--" + name, type=int, default=None)
    a = ap.parse_args()
    X, bs = tuple(a.lattice), tuple(a.block)
    torch.cuda.set_device(0)
    gen = torch.Generator(device="cuda").manual_seed(12)
    vol, vcb = int(np.prod(X)), int(np.prod(X)) // 2
    prm = {k: getattr(a, k) for k in ("nKrylov", "nuPre", "nuPost", "coarseIters") if getattr(a, k) is not None}
    p = hip.mgSolveParam(tol=a.tol, maxIter=a.max_iter, **prm)

    def crandn(*shape):
        return torch.randn(*shape, dtype=torch.complex128, device="cuda", generator=gen)

    gauge = hip.GaugeField(X, (0, 0, 0, 0), 8)
    U = batched_q(crandn(8 * vcb, 3, 3)).reshape(2, 4, vcb, 3, 3)                     # [parity, mu, x_cb, row, col]: random unitary links
    gauge.data.view(2, 4, 9, vcb).copy_(U.reshape(2, 4, vcb, 9).permute(0, 1, 3, 2))
    del U
    C = hip.CloverField(X, 8).compute(gauge, a.csw_coeff)

    def random_fields(n):
        out = []
        for _ in range(n):
            f = hip.SpinorField(X, 8, 2)
            f.data.copy_(crandn(f.data.numel()))
            out.append(f)
        return out

    # ---- the crude null vectors and the coarse operator
    t0 = time.perf_counter()
    src = random_fields(a.nvec)
    nv, _ = hip.wilsonSolve(src, gauge, a.kappa, tol=1e-12, maxIter=a.setup_iters, allow_unconverged=True, clover=C)
    T = hip.Transfer(X, a.nvec, bs, 2, 8)
    null_vectors(T, nv, X, bs)
    del src, nv
    op = hip.computeCoarseOperator(T, gauge, a.kappa, clover=C)
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t0

    b = random_fields(a.nrhs)
    x_mg, x_cg = [hip.SpinorField(X, 8, 2) for _ in b], [hip.SpinorField(X, 8, 2) for _ in b]
    info = {}

    def run_mg():
        _, info["mg"] = hip.mgSolve(b, gauge, a.kappa, T, op, clover=C, x=x_mg, tol=a.tol, maxIter=a.max_iter, allow_unconverged=True, **prm)

    def run_cg():
        _, info["cg"] = hip.wilsonSolve(b, gauge, a.kappa, tol=a.tol, maxIter=20 * a.max_iter, x=x_cg, allow_unconverged=True, clover=C)

    def wall_ms(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t)

    def event_ms(fn, n):
        """milliseconds per call of n calls between two events: one call of a 0.1 ms launch would mostly time the events and the host"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    solves = {"mg_solve": run_mg, "cg_solve": run_cg}
    st = {k: [] for k in solves}
    for it in range(a.warmup + a.reps):
        for k in solves:                                                              # alternated
            ms = wall_ms(solves[k])
            if it >= a.warmup:
                st[k].append(ms)

    # ---- one K against its operator launches
    z, f2 = [hip.SpinorField(X, 8, 2) for _ in b], [hip.SpinorField(X, 8, 2) for _ in b]
    cw, cy = [hip.CoarseField(T.Xc, a.nvec, 8) for _ in b], [hip.CoarseField(T.Xc, a.nvec, 8) for _ in b]
    hip.restrictVecs(cw, b, T)
    parts = {
        "K": lambda: hip.mgPrecondition(z, b, gauge, a.kappa, T, op, clover=C, **prm),
        "stencil": lambda: hip.wilsonApply(f2, b, gauge, a.kappa, clover=C),
        "restrict": lambda: hip.restrictVecs(cy, b, T),
        "prolong": lambda: hip.prolongateEvecs(f2, cw, T),
        "coarse_apply": lambda: hip.coarseApply(cy, cw, op),
    }
    pt = {k: [] for k in parts}
    loop = {"K": 5, "stencil": 20, "restrict": 20, "prolong": 20, "coarse_apply": 40}     # calls per sample
    for it in range(a.warmup + 2 * a.reps):
        for k in parts:
            ms = event_ms(parts[k], loop[k])
            if it >= a.warmup:
                pt[k].append(ms)
    med = {k: float(np.median(v)) for k, v in list(st.items()) + list(pt.items())}
    n_stencil = p.nuPre + p.nuPost + (1 if p.coarseIters > 0 and p.nuPost > 0 else 0)
    ops_ms = n_stencil * med["stencil"] + (med["restrict"] + med["prolong"] + p.coarseIters * med["coarse_apply"] if p.coarseIters > 0 else 0.0)

    mg, cg = info["mg"], info["cg"]
    diff = max(float(torch.linalg.vector_norm(u.data - v.data) / torch.linalg.vector_norm(v.data)) for u, v in zip(x_mg, x_cg))
    fv = 24 * vol * 8                                                                  # bytes of one fine fp64 vector
    kbar = (p.nKrylov - 1) / 2.0                                                      # mean number of stored directions over a cycle
    res = {"workload": "two-grid GCR, %s fp64, aggregates %s, n_vec %d, %d right-hand sides, Wilson-clover kappa %g, random unitary links, crude null "
                       "vectors (%d CG iterations, per-aggregate QR)" % ("x".join(map(str, X)), "x".join(map(str, bs)), a.nvec, a.nrhs, a.kappa, a.setup_iters),
           "param": {n: getattr(p, n) for n, _ in p._fields_}, "reps": a.reps, "warmup": a.warmup, "setup_s": round(setup_s, 2),
           "ms_median": {k: round(v, 3) for k, v in med.items()}, "ms_min": {k: round(float(np.min(v)), 3) for k, v in list(st.items()) + list(pt.items())},
           "mg_iters": [int(i) for i in mg.iters], "mg_relres_max": float(np.max(mg.relres)), "mg_converged": bool(mg.converged), "mg_hostReads": mg.hostReads,
           "cg_iters": [int(i) for i in cg.iters], "cg_relres_max": float(np.max(cg.relres)), "cg_converged": bool(cg.converged),
           # the CG does not count its reads: 2 per iteration (<Mp, Mp> and ||r||^2) and 3 per block (||b||^2, ||M^dag b||^2, the true
           # residual), read off wilson_solve_impl in csrc/wilson.hip -- a count from the source, not a measurement
           "cg_hostReads_from_source": 2 * int(np.max(cg.iters)) + 3,
           "cg_over_mg_time": round(med["cg_solve"] / med["mg_solve"], 3), "x_rel_diff_mg_vs_cg_max": diff,
           "K_operator_launches": {"stencil": n_stencil, "restrict": int(p.coarseIters > 0), "prolong": int(p.coarseIters > 0), "coarse_apply": p.coarseIters},
           "K_operators_alone_ms": round(ops_ms, 3), "K_over_operators_alone": round(med["K"] / ops_ms, 3),
           # Krylov kernels alone, in fine vectors per right-hand side.  MR step: the dots read t, s; the update reads s, z, t and writes z, s
           # (7; the stencil adds a read and a write).  Outer iteration with k stored directions: multi-dot k + 1 reads, multi-axpy 2 k + 3
           # reads and 2 writes, update 4 reads and 4 writes (3 k + 14)
           "model_GB_per_MR_step_krylov": round(a.nrhs * 7 * fv / 1e9, 3),
           "model_GB_per_outer_iteration_krylov": round(a.nrhs * fv * (3 * kbar + 14) / 1e9, 3)}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
