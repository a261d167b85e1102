"""CPU checks around stout smearing and the plaquette (no GPU): the numpy pin tests/smear_ref.py is anchored by known answers before
anything is compared with it -- (a) pure-gauge links are a fixed point with plaquette 1, (b) gauge covariance, (c) the closed form on
rotated abelian links, (d) unitarity, (e) rho = 0 and the untouched t links -- then (f) the host-side validation of the three C entry
points, the C++ mirror and the command-line flags."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import smear_ref as sr
from clover_ref import at, dag
from util import random_gauge_lex, random_su3
from wilson_planewave import _orthonormal_rows, pure_gauge_lex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = (4, 2, 6, 4)                                                                  # an axis of extent 2: both neighbours are the same site


def _unitary_gauge(rng, X):
    return _orthonormal_rows(random_gauge_lex(rng, X))


@pytest.mark.parametrize("dims", [3, 4])
def test_pure_gauge_is_a_fixed_point(dims):
    """(a) U_mu(x) = g(x) g^dag(x + mu): every staple is U_mu, Omega is Hermitian, Q = 0: one step returns U to 1e-14; the plaquette is 1."""
    U, _ = pure_gauge_lex(np.random.default_rng(2), X)
    assert np.max(np.abs(sr.stout_step(U, 0.1, dims) - U)) < 1e-14
    assert np.max(np.abs(np.array(sr.plaquette(U)) - 1.0)) < 1e-14


@pytest.mark.parametrize("dims", [3, 4])
def test_gauge_covariance(dims):
    """(b) smear(g U g^dag) = g smear(U) g^dag to 1e-13."""
    rng = np.random.default_rng(5)
    U = _unitary_gauge(rng, X)
    g = _orthonormal_rows(random_su3(rng, (X[3], X[2], X[1], X[0])))
    rot = lambda W: np.stack([g @ W[mu] @ dag(at(g, (mu, 1))) for mu in range(4)])
    S = sr.stout_step(U, 0.1, dims)
    assert np.max(np.abs(S - U)) > 0.05                                           # a step that does something
    assert np.max(np.abs(sr.stout_step(rot(U), 0.1, dims) - rot(S))) < 1e-13
    assert np.max(np.abs(np.array(sr.plaquette(rot(U))) - np.array(sr.plaquette(U)))) < 1e-13


@pytest.mark.parametrize("dims", [3, 4])
@pytest.mark.parametrize("degenerate", [False, True])
def test_rotated_abelian_closed_form(dims, degenerate):
    """(c) theta' = theta + rho (S - mean_c S) with S the sines of the staple angles; plaquette = mean_c cos(plaquette angle): 1e-13."""
    rng = np.random.default_rng(7)
    rho = 0.11
    U, th, g = sr.rotated_abelian_links(rng, X, degenerate=degenerate)
    th1 = sr.abelian_stout_angles(th, rho, dims)
    assert np.max(np.abs(th1 - th)) > 0.05
    assert np.max(np.abs(sr.stout_step(U, rho, dims) - sr.abelian_links(th1, g))) < 1e-13
    assert np.max(np.abs(np.array(sr.plaquette(U)) - np.array(sr.abelian_plaquette(th)))) < 1e-13
    assert abs(sr.plaquette(U)[0]) < 0.9                                          # not the trivial field


@pytest.mark.parametrize("dims", [3, 4])
def test_unitarity(dims):
    """(d) U'^dag U' - 1 and det U' - 1 below 1e-14 after every one of five steps."""
    U = _unitary_gauge(np.random.default_rng(9), X)
    for _ in range(5):
        U = sr.stout_step(U, 0.125, dims)
        assert np.max(np.abs(dag(U) @ U - np.eye(3))) < 1e-14
        assert np.max(np.abs(np.linalg.det(U) - 1.0)) < 1e-14


def test_rho_zero_and_time_links():
    """(e) rho = 0 is the identity exactly; smearDims = 3 leaves the t links bitwise untouched; five 4D steps raise the plaquette."""
    U = _unitary_gauge(np.random.default_rng(11), X)
    for dims in (3, 4):
        assert np.array_equal(sr.stout_step(U, 0.0, dims), U)
    S = sr.stout_smear(U, 0.1, 3, 3)
    assert np.array_equal(S[3], U[3]) and np.max(np.abs(S[:3] - U[:3])) > 0.05
    p = [sr.plaquette(sr.stout_smear(U, 0.1, n, 4))[0] for n in range(6)]
    assert all(b > a for a, b in zip(p, p[1:])) and p[5] > p[0] + 0.3


# ---- (f) host-side validation: INVALID_ARGUMENT (1) before any device work -------------------------------------------------------------
def _gauge(hip, X, R=(0, 0, 0, 0), data=1 << 20, prec=8):
    g = hip._lib.GaugeDesc()
    volEx = int(np.prod([X[d] + 2 * R[d] for d in range(4)])) // 2
    g.data, g.precision, g.stride, g.parity_offset = data, prec, volEx, 36 * volEx
    for i in range(4):
        g.X[i], g.R[i] = X[i], R[i]
    return g


def test_host_side_validation(hip):
    lib = hip._lib.load()
    err = lib.mugiq_hip_last_error
    B = ctypes.byref
    L = (4, 4, 4, 4)
    nbytes = 2 * 36 * 128 * 16
    a, b = _gauge(hip, L), _gauge(hip, L, data=(1 << 20) + 4 * nbytes)
    plaq = (ctypes.c_double * 3)()

    def all_three(g, comm=None, other=b):
        """(status, message) of the three entry points with this field (as `out` and as `in` of the smearing, beside `other`)"""
        return [(lib.mugiq_hip_exchange_extended_gauge(g, comm, None), err()),
                (lib.mugiq_hip_stout_smear(g, B(other), 0.1, 1, 3, comm, None), err()),
                (lib.mugiq_hip_stout_smear(B(other), g, 0.1, 1, 3, comm, None), err()),
                (lib.mugiq_hip_plaquette(g, plaq, comm, None), err())]
    names = [b"exchangeExtendedGauge", b"stoutSmear", b"stoutSmear", b"plaquette"]

    def rejected(results, word):
        for (st, msg), who in zip(results, names):
            assert st == 1 and who in msg and word in msg, (st, msg)
    # a NULL descriptor, NULL data
    rejected(all_three(None), b"NULL")
    rejected(all_three(B(_gauge(hip, L, data=None))), b"NULL")
    assert lib.mugiq_hip_plaquette(B(a), None, None, None) == 1 and b"plaquette" in err() and b"NULL" in err()
    # precision
    rejected(all_three(B(_gauge(hip, L, prec=2))), b"precision")
    # odd local dims
    rejected(all_three(B(_gauge(hip, (4, 4, 3, 4)))), b"even")
    # borders: negative, odd sum, deeper than the lattice
    rejected(all_three(B(_gauge(hip, L, (0, 0, 0, 1)))), b"even")
    neg = _gauge(hip, L)
    neg.R[2] = -1
    rejected(all_three(B(neg)), b"R[2]")
    # stride / parity offset
    short = _gauge(hip, L)
    short.stride = 100
    rejected(all_three(B(short)), b"stride")
    short = _gauge(hip, L)
    short.parity_offset = 36 * 128 - 1
    rejected(all_three(B(short)), b"parity_offset")
    # smearing: geometry and precision mismatch, overlap, nSteps, smearDims, rho
    smear = lib.mugiq_hip_stout_smear
    assert smear(B(b), B(_gauge(hip, (4, 4, 4, 8))), 0.1, 1, 3, None, None) == 1 and b"stoutSmear" in err() and b"differ" in err()
    assert smear(B(_gauge(hip, L, (2, 0, 0, 0), data=1 << 24)), B(a), 0.1, 1, 3, None, None) == 1 and b"differ" in err()
    assert smear(B(_gauge(hip, L, data=1 << 24, prec=4)), B(a), 0.1, 1, 3, None, None) == 1 and b"precision" in err()
    assert smear(B(a), B(a), 0.1, 1, 3, None, None) == 1 and b"overlap" in err()
    assert smear(B(_gauge(hip, L, data=(1 << 20) + nbytes - 16)), B(a), 0.1, 1, 3, None, None) == 1 and b"overlap" in err()
    assert smear(B(b), B(a), 0.1, -1, 3, None, None) == 1 and b"nSteps" in err()
    for dims in (2, 5):
        assert smear(B(b), B(a), 0.1, 1, dims, None, None) == 1 and b"smearDims" in err()
    for rho in (float("nan"), float("inf")):
        assert smear(B(b), B(a), rho, 1, 3, None, None) == 1 and b"rho" in err()
    # a partitioned dimension without a border (forced partitioning on one rank: no process group needed)
    comm = hip.GridComm((1, 1, 1, 1), force_partitioned=(0, 0, 0, 1))
    c = comm.c_struct()
    cp = ctypes.cast(ctypes.byref(c), ctypes.c_void_p)
    rejected(all_three(B(a), cp), b"no border")
    # ... and one without sendrecv
    raw = hip.comm._CCommRaw()
    ctypes.memmove(B(raw), B(c), ctypes.sizeof(raw))
    raw.sendrecv = None
    rp = ctypes.cast(B(raw), ctypes.c_void_p)
    rejected(all_three(B(_gauge(hip, L, (0, 0, 0, 2))), rp, _gauge(hip, L, (0, 0, 0, 2), data=1 << 26)), b"sendrecv")


def test_python_layer(hip):
    assert all(hasattr(hip.GaugeField, n) for n in ("exchangeBorders", "stoutSmear", "plaquette"))
    for name in ("mugiq_hip_exchange_extended_gauge", "mugiq_hip_stout_smear", "mugiq_hip_plaquette"):
        assert name in hip._lib.SIGNATURES


def test_cli_flags_parse_and_reject():
    from mugiq_amd import loop_cli
    ap = loop_cli.build_parser()
    a = ap.parse_args([])
    assert a.loop_gauge_stout_steps == 0 and a.loop_gauge_stout_dims == 3 and a.compute_plaquette is False
    a = ap.parse_args(["--loop-gauge-stout-steps", "2", "--loop-gauge-stout-rho", "0.1", "--loop-gauge-stout-dims", "4", "--compute-plaquette"])
    assert (a.loop_gauge_stout_steps, a.loop_gauge_stout_rho, a.loop_gauge_stout_dims, a.compute_plaquette) == (2, 0.1, 4, True)
    for bad in (["--loop-gauge-stout-dims", "5"], ["--loop-gauge-stout-steps", "-1"], ["--loop-gauge-stout-steps", "x"],
                ["--loop-gauge-stout-rho", "nan"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)


def test_cli_smears_the_loop_gauge_only(hip, tmp_path, monkeypatch, capsys):
    """main() with the device work replaced: the smeared field goes into the loop, the loaded one into --check-evals, and the plaquette
    lines are the reference's; without the flags nothing of it runs and nothing is printed."""
    from mugiq_amd import loop_cli
    seen = {}

    class FakeGauge:
        X, precision = (4, 4, 4, 4), 8

        def __init__(self, plaq=(0.5, 0.25, 0.75)):
            self.plaq = plaq

        def stoutSmear(self, rho, nSteps, smearDims=3, comm=None, out=None):
            seen["smear"] = (rho, nSteps, smearDims)
            seen["smeared"] = FakeGauge((0.875, 0.75, 1.0))
            return seen["smeared"]

        def plaquette(self, comm=None):
            seen.setdefault("plaquettes", []).append(self)
            return self.plaq

    class FakeEig:
        def __init__(self, eVecs, gauge, kappa, opType, comm=None, clover=None):
            seen["eig"] = gauge

        def computeEvals(self):
            pass

        def printEvals(self, file=None):
            pass

    class FakeLoop:
        nLoop = nData = 0

        def __init__(self, prm, *a):
            seen["loop"] = prm.gauge

        def printLoopComputeParams(self, f):
            pass

        def computeCoarseLoop(self):
            pass

        def close(self):
            pass

    class F:
        order = 2
    gauge = FakeGauge()
    monkeypatch.setattr(loop_cli, "synthetic_inputs", lambda args, rank=0, comm=None: ([F()], [1.0], gauge))
    monkeypatch.setattr(hip, "Loop_Mugiq", FakeLoop)
    monkeypatch.setattr(hip.eigsolve, "Eigsolve_Mugiq", FakeEig)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    mom = tmp_path / "momenta.txt"
    mom.write_text("0 0 0\n")
    base = ["--loop-ft-sign", "minus", "--loop-calc-type", "opt", "--momenta-filename", str(mom), "--displace-entry-string", "+z:1",
            "--loop-write-mom-space", "no", "--check-evals"]
    assert loop_cli.main(base) == 0
    out = capsys.readouterr()
    assert "smear" not in seen and "plaquettes" not in seen and seen["loop"] is gauge and seen["eig"] is gauge
    assert "plaquette" not in out.err and "plaquette" not in out.out
    seen.clear()
    assert loop_cli.main(base + ["--compute-plaquette"]) == 0
    lines = [l for l in capsys.readouterr().err.splitlines() if "plaquette" in l]
    assert lines == ["Computed plaquette is %e (spatial = %e, temporal = %e)" % (0.5, 0.25, 0.75)] and "smear" not in seen
    seen.clear()
    assert loop_cli.main(base + ["--loop-gauge-stout-steps", "2", "--loop-gauge-stout-rho", "0.1", "--loop-gauge-stout-dims", "4"]) == 0
    lines = [l for l in capsys.readouterr().err.splitlines() if "plaquette" in l]
    assert seen["smear"] == (0.1, 2, 4) and seen["loop"] is seen["smeared"] and seen["eig"] is gauge
    assert lines == ["Computed plaquette is %e (spatial = %e, temporal = %e)" % (0.5, 0.25, 0.75),
                     "Computed plaquette is %e (spatial = %e, temporal = %e)" % (0.875, 0.75, 1.0)]


def test_cpp_smear_mirror_compiles(tmp_path):
    """exchangeExtendedGauge, stoutSmear and plaquette of the C++ mirror: -fsyntax-only."""
    tu = tmp_path / "smear_tu.cpp"
    tu.write_text('#include "mugiq_hip_operators.hpp"\n'
                  "void use(const MugiqHipGaugeField &U, const MugiqHipGaugeField &V, const MugiqHipComm *comm, void *stream) {\n"
                  "  mugiq_hip::exchangeExtendedGauge(U);\n"
                  "  mugiq_hip::exchangeExtendedGauge(U, comm, stream);\n"
                  "  mugiq_hip::stoutSmear(V, U, 0.1, 2);\n"
                  "  mugiq_hip::stoutSmear(V, U, 0.1, 2, 4, comm, stream);\n"
                  "  std::array<double, 3> p = mugiq_hip::plaquette(U);\n"
                  "  p = mugiq_hip::plaquette(V, comm, stream);\n"
                  "  (void)p;\n"
                  "}\n")
    cc = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cc):
        pytest.skip("no clang++")
    r = subprocess.run([cc, "-std=c++17", "-fsyntax-only", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-Wall", "-I", os.path.join(ROOT, "include"),
                        "-I", "/opt/rocm/include", str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
