"""Spawned workers of tests/test_gpu_deflate.py: low-mode deflation (mugiq_hip_deflate_low_modes) on a process grid, every rank on
cuda:0, gloo transport, checked against the single-domain result computed in numpy.  Also the seeded case generator of the random
sweep and a restatement of the launch geometry of deflate_low_modes (plain Python: the CPU tests import it)."""
import numpy as np

from mp_workers import _init

STORAGE = [(pe, o, ps) for pe in (8, 4) for o in (2, 4) for ps in (8, 4)]   # (eigenvector precision, order, src / dst precision)
DEFAULT_SEEDS = 16                     # test_deflate_random_shapes; MUGIQ_TEST_SEEDS=N widens the sweep

# ---- csrc/deflate.hip: kSeg = 64 complex elements per segment, kNB = 64 eigenvectors per pass-1 workgroup, kRBMax = 16 right-hand
# sides per block, and the setup of deflate_low_modes ("// ---- setup": segsPerPlane, nSeg, nNB, nChunks (the 4096-workgroup target),
# segsPerChunk, nBlocks; the RB = (nR + 3) / 4 * 4 of the pass loops)
K_SEG, K_NB, K_RB_MAX, CHUNK_TARGET = 64, 64, 16, 4096


def deflate_geometry(X, order, nEv, nVec):
    """the pass geometry of one deflate_low_modes call, and the regimes it reaches"""
    volumeCB = int(np.prod(X)) // 2
    cpp = 1 if order == 2 else 2
    planes = 12 // cpp
    segsPerPlane = -(-cpp * volumeCB // K_SEG)
    nSeg = 2 * planes * segsPerPlane
    nNB = -(-nEv // K_NB)
    nChunks = max(1, min(nSeg, -(-CHUNK_TARGET // nNB)))
    segsPerChunk = -(-nSeg // nChunks)
    RBs = [(min(K_RB_MAX, nVec - r0) + 3) // 4 * 4 for r0 in range(0, nVec, K_RB_MAX)]
    return dict(nSeg=nSeg, nNB=nNB, nChunks=nChunks, segsPerChunk=segsPerChunk, RBs=RBs,
                partial_last_block=nNB > 1 and nEv % K_NB != 0,
                multi_segment=segsPerChunk > 1,
                partial_last_chunk=nSeg % segsPerChunk != 0,           # (then chunks past the last one with work are empty)
                empty_chunks=nChunks * segsPerChunk - nSeg >= segsPerChunk,
                partial_last_segment=(cpp * volumeCB) % K_SEG != 0)


NEV_BIAS = (1, 63, 64, 65, 128, 129)
NVEC_BIAS = (1, 4, 5, 15, 16, 17, 32, 33)
SITE_FIELDS_MAX = 2500000              # (nEv + 2 nVec) V: host memory and numpy time of one case


def random_deflate_case(seed):
    """A seeded case of test_deflate_random_shapes: dict(X, pe, order, ps, nev, nvec, pad, gamma5, sigma, alias, overlaps).  Storage:
    STORAGE[seed % 8] (every combination in every 8 consecutive seeds).  Every third seed is a large lattice past the multi-segment
    threshold of pass 1 (segsPerChunk > 1); the others up to 4096 sites.  alias: the r with dst[r] = src[r] (the same field)."""
    rng = np.random.default_rng(seed)
    pe, order, ps = STORAGE[seed % len(STORAGE)]
    big = seed % 3 == 0
    for _ in range(10000):
        nev = int(rng.choice(NEV_BIAS)) if rng.random() < 0.7 else int(rng.integers(1, 201))
        nvec = int(rng.choice(NVEC_BIAS)) if rng.random() < 0.7 else int(rng.integers(1, 41))
        X = tuple(int(v) for v in rng.choice([2, 4, 6, 8, 10, 12, 16], size=4))
        V = int(np.prod(X))
        if V > 32768 or (nev + 2 * nvec) * V > SITE_FIELDS_MAX:
            continue
        if big == deflate_geometry(X, order, nev, nvec)["multi_segment"] and (big or V <= 4096):
            break
    else:
        raise RuntimeError("random_deflate_case(%d): no case found" % seed)
    mode = int(rng.integers(3))                                        # no aliasing | all | a random subset
    alias = [] if mode == 0 else list(range(nvec)) if mode == 1 else sorted(int(r) for r in np.flatnonzero(rng.random(nvec) < 0.5))
    sigma = None if rng.integers(3) == 0 else ((0.5 + rng.random(nev)) * np.where(rng.random(nev) < 0.5, -1.0, 1.0)).tolist()
    return dict(X=X, pe=pe, order=order, ps=ps, nev=nev, nvec=nvec, pad=int(rng.choice([0, 7, 32])), gamma5=bool(rng.integers(2)),
                sigma=sigma, alias=alias, overlaps=bool(rng.integers(4)))


def deflate_worker(rank, world, port, grid, G, out_prefix, nev=7, nvec=5, pad=0, seed=31):
    """Global eigenvectors / sources / solutions from one seed; each rank deflates its local block with the grid comm.  The local
    result must equal the block of the single-domain numpy result, the overlaps must equal V^dag g5 src, and every rank's overlaps
    are saved so the test can check they are identical.  nev, nvec, seed: the job (defaults: the fixed one); pad: stride pad of every
    field, the pads filled with NaN."""
    import torch
    from util import orc, random_spinor_lex, rel_err
    dist = _init(rank, world, port)
    torch.cuda.set_device(0)
    import mugiq_amd as hip
    rng = np.random.default_rng(seed)
    ev = [random_spinor_lex(rng, G) for _ in range(nev)]
    src = [random_spinor_lex(rng, G) for _ in range(nvec)]
    dst = [random_spinor_lex(rng, G) for _ in range(nvec)]
    if nev == 7:
        sg = np.array([0.3, -0.7, 1.1, -1.9, 2.5, 0.05, -0.2])
    else:
        sg = (0.3 + rng.random(nev)) * np.where(np.arange(nev) % 2, -1.0, 1.0)
    g5 = np.diag(orc.gamma_dense(15)).real
    Vm = np.stack([v.reshape(-1, 4, 3) for v in ev])                    # [n][site][s][c]
    Sm = np.stack([s.reshape(-1, 4, 3) * g5[None, :, None] for s in src])
    C = np.einsum("nxsc,rxsc->nr", Vm.conj(), Sm)
    want = [dst[r] - np.einsum("n,nxsc->xsc", C[:, r] / sg, Vm).reshape(dst[r].shape) for r in range(nvec)]
    comm = hip.GridComm(grid, device="cuda:0")
    l = [G[d] // grid[d] for d in range(4)]

    def loc(v):
        f = hip.SpinorField(l, 8, 2, pad=pad).set_logical(orc.lex_to_eo(orc.local_block(v, comm.coord, grid), l))
        if pad:
            m = torch.ones(f.data.numel(), dtype=torch.bool)
            m[torch.from_numpy(np.asarray(f._index_table()).reshape(-1))] = False
            f.data[m.to(f.data.device)] = complex(float("nan"), float("nan"))
        return f
    fe, fs, fd = [loc(v) for v in ev], [loc(v) for v in src], [loc(v) for v in dst]
    ov = hip.deflateLowModes(fd, fs, fe, sg, gamma5=True, comm=comm, overlaps=True)
    torch.cuda.synchronize()
    assert rel_err(ov, C) < 1e-12, rel_err(ov, C)
    for r in range(nvec):
        ref = orc.lex_to_eo(orc.local_block(want[r], comm.coord, grid), l)
        got = fd[r].get_logical()
        e = np.max(np.abs(got - ref)) / np.max(np.abs(ref))
        assert e < 1e-12, (rank, r, e)
    np.save("%s_%d.npy" % (out_prefix, rank), ov)
    dist.barrier()
    dist.destroy_process_group()
