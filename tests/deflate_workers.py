"""Spawned workers of tests/test_gpu_deflate.py: low-mode deflation (mugiq_hip_deflate_low_modes) on a process grid, every rank on
cuda:0, gloo transport, checked against the single-domain result computed in numpy."""
import numpy as np

from mp_workers import _init


def deflate_worker(rank, world, port, grid, G, out_prefix):
    """Global eigenvectors / sources / solutions from one seed; each rank deflates its local block with the grid comm.  The local
    result must equal the block of the single-domain numpy result, the overlaps must equal V^dag g5 src, and every rank's overlaps
    are saved so the test can check they are identical."""
    import torch
    from util import orc, random_spinor_lex, rel_err
    dist = _init(rank, world, port)
    torch.cuda.set_device(0)
    import mugiq_amd as hip
    rng = np.random.default_rng(31)
    nev, nvec = 7, 5
    ev = [random_spinor_lex(rng, G) for _ in range(nev)]
    src = [random_spinor_lex(rng, G) for _ in range(nvec)]
    dst = [random_spinor_lex(rng, G) for _ in range(nvec)]
    sg = np.array([0.3, -0.7, 1.1, -1.9, 2.5, 0.05, -0.2])
    g5 = np.diag(orc.gamma_dense(15)).real
    Vm = np.stack([v.reshape(-1, 4, 3) for v in ev])                    # [n][site][s][c]
    Sm = np.stack([s.reshape(-1, 4, 3) * g5[None, :, None] for s in src])
    C = np.einsum("nxsc,rxsc->nr", Vm.conj(), Sm)
    want = [dst[r] - np.einsum("n,nxsc->xsc", C[:, r] / sg, Vm).reshape(dst[r].shape) for r in range(nvec)]
    comm = hip.GridComm(grid, device="cuda:0")
    l = [G[d] // grid[d] for d in range(4)]
    loc = lambda v: hip.SpinorField(l, 8, 2).set_logical(orc.lex_to_eo(orc.local_block(v, comm.coord, grid), l))
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
