"""bench.py's options and what --dump-outputs writes, on CPU tensors (no GPU needed): a plain run is the headline alone,
--steps is the number of timed steps, and the stored outputs are the loop traces of the timed path at a fixed sample of
sites, the same from run to run."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _parse(monkeypatch, *args):
    monkeypatch.setattr(sys, "argv", ["bench.py", *args])
    return bench.parse()


def test_plain_run_is_the_headline_alone(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, "")
    a = _parse(monkeypatch, "--full", "--dump-outputs", "out")
    assert a.full and a.dump_outputs == "out"


def test_steps_must_be_positive(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


def _loop(V, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.complex(torch.randn(16 * V, generator=g, dtype=torch.float64),
                         torch.randn(16 * V, generator=g, dtype=torch.float64)).to(dtype)


@pytest.mark.parametrize("dtype,npdt,npcdt", [(torch.complex128, np.float64, np.complex128), (torch.complex64, np.float32, np.complex64)])
def test_dump_outputs_sample_and_stats(tmp_path, monkeypatch, dtype, npdt, npcdt):
    V = 512
    monkeypatch.setattr(bench, "DUMP_SITES", 100)
    loop = _loop(V, dtype, 3)
    bench.dump_outputs(loop, V, str(tmp_path / "a"))
    bench.dump_outputs(loop, V, str(tmp_path / "b"))
    s = np.load(tmp_path / "a" / "loop_sample.npy")
    st = np.load(tmp_path / "a" / "loop_gamma_stats.npy")
    assert s.dtype == npdt and s.shape == (16, 100, 2) and st.dtype == npdt and st.shape == (16, 3)
    # the same sites every time
    assert np.array_equal(s, np.load(tmp_path / "b" / "loop_sample.npy"))
    assert np.array_equal(st, np.load(tmp_path / "b" / "loop_gamma_stats.npy"))
    full = loop.view(16, V).to(torch.complex128).numpy()
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(V, 100, replace=False))
    assert np.array_equal(s[..., 0] + 1j * s[..., 1], full[:, idx].astype(npcdt))
    tol = 1e-12 if dtype == torch.complex128 else 1e-5
    np.testing.assert_allclose(st[:, 0], full.real.sum(1), rtol=tol, atol=tol)
    np.testing.assert_allclose(st[:, 1], full.imag.sum(1), rtol=tol, atol=tol)
    np.testing.assert_allclose(st[:, 2], np.linalg.norm(full, axis=1), rtol=tol)


def test_dump_outputs_fit_the_budget(tmp_path):
    """the headline's 32^4 fp64 loop: the stored sample stays far below 64 MB"""
    V = 32 ** 4
    assert 16 * min(bench.DUMP_SITES, V) * 2 * 8 + 16 * 3 * 8 <= 64 << 20
    V = 4096                                         # every site when the lattice has fewer than DUMP_SITES
    bench.dump_outputs(_loop(V, torch.complex128, 5), V, str(tmp_path))
    assert np.load(tmp_path / "loop_sample.npy").shape == (16, V, 2)
