"""CPU checks around the clover term (no GPU): the numpy pin tests/clover_ref.py is anchored by known answers before anything is
compared with it -- (a) pure-gauge links give A = 1, (b) the closed form on rotated abelian links, (c) A and g5 M_clov are Hermitian,
(d) gauge covariance -- then (e) host-side validation of the new C entry points, (f) the command-line flags and (g) the C++ overloads."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import clover_ref as cr
import wilson_ref as wr
from util import orc, nonunitary_gauge_lex, random_gauge_lex, random_su3
from wilson_planewave import pure_gauge_lex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pure_gauge_gives_the_identity():
    """(a) U_mu(x) = g(x) g^dag(x + mu): every plaquette is 1, Fhat = 0, A = 1 to 1e-14."""
    X = (4, 6, 2, 8)
    U, _ = pure_gauge_lex(np.random.default_rng(2), X)
    A = cr.clover_dense(U, 0.17)
    assert np.max(np.abs(A - np.eye(12))) < 1e-14


def test_closed_form():
    """(b) Fhat_mn = g diag(i sin phi^{mn}_c) g^dag and A = 1 - coeff sum sigma_mn (x) g diag(sin phi^{mn}_c) g^dag on (4, 6, 2, 8) to 1e-13."""
    X, coeff = (4, 6, 2, 8), 0.23
    U, g, phi = cr.closed_form_links(np.random.default_rng(3), X)
    assert any(np.any(np.abs(np.sin(p)) > 0.5) for p in phi.values())                      # a field strength that is there
    for m, n in cr.PLANES:
        want = (g * (1j * np.sin(phi[(m, n)]))[None, None, None, None, None, :]) @ cr.dag(g)
        assert np.max(np.abs(cr.fhat(U, m, n) - want)) < 1e-13, (m, n)
    A = cr.clover_dense(U, coeff)
    assert np.max(np.abs(A - cr.closed_form_A(g, phi, coeff))) < 1e-13
    assert np.max(np.abs(A - np.eye(12))) > 0.1


@pytest.mark.parametrize("kind", ["su3", "gl3"])
def test_hermiticity(kind):
    """(c) A is Hermitian and block diagonal; the dense g5 M_clov on (4, 4, 2, 2) is Hermitian to 1e-13, for links as stored."""
    X, kappa, coeff = (4, 4, 2, 2), 0.12, 0.15
    rng = np.random.default_rng(4)
    U = random_gauge_lex(rng, X) if kind == "su3" else nonunitary_gauge_lex(rng, X, "gl3")[0]
    A = cr.clover_dense(U, coeff)
    assert np.max(np.abs(A - cr.dag(A))) < 1e-14
    assert cr.blocks_of(A)[1] == 0.0
    assert np.max(np.abs(A - np.eye(12))) > 0.05
    Uo = orc.extended_gauge_from_global(U, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    M = cr.dense_matrix(Uo, orc.lex_to_eo(A, X), kappa, X)
    g5 = np.tile(np.repeat(wr.G5, 3), int(np.prod(X)))
    H = g5[:, None] * M
    assert np.max(np.abs(H - H.conj().T)) < 1e-13
    # ... and the dagger flag of the reference is that adjoint
    Md = cr.dense_matrix(Uo, orc.lex_to_eo(A, X), kappa, X, cr.OP_MDAG)
    assert np.max(np.abs(Md - M.conj().T)) < 1e-13


def test_gauge_covariance():
    """(d) U'_mu(x) = g(x) U_mu(x) g^dag(x + mu)  =>  A'(x) = (1 (x) g(x)) A(x) (1 (x) g(x))^dag."""
    X, coeff = (4, 2, 6, 4), 0.2
    rng = np.random.default_rng(5)
    U = random_gauge_lex(rng, X)
    g = random_su3(rng, (X[3], X[2], X[1], X[0]))
    Ug = np.stack([g @ U[mu] @ cr.dag(cr.at(g, (mu, 1))) for mu in range(4)])
    G = np.einsum("st,...ab->...satb", np.eye(4), g).reshape(g.shape[:4] + (12, 12))
    assert np.max(np.abs(cr.clover_dense(Ug, coeff) - G @ cr.clover_dense(U, coeff) @ cr.dag(G))) < 1e-13


def test_wrong_operator_leaves_a_large_residual():
    """What the feature is for, on the pin: the lowest eigenvectors of H_clov have relative residuals far above 1e-3 under the unimproved
    H (seed and coeff of tests/test_gpu_clover.py::test_compute_evals)."""
    X, kappa, coeff = (4, 4, 2, 2), 0.12, 0.2
    U = random_gauge_lex(np.random.default_rng(1), X)
    Uo = orc.extended_gauge_from_global(U, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    g5 = np.tile(np.repeat(wr.G5, 3), int(np.prod(X)))
    Hc = g5[:, None] * cr.dense_matrix(Uo, orc.lex_to_eo(cr.clover_dense(U, coeff), X), kappa, X)
    Hw = g5[:, None] * wr.dense_matrix(Uo, kappa, X)
    lam, vec = np.linalg.eigh(0.5 * (Hc + Hc.conj().T))
    for n in np.argsort(np.abs(lam))[:8]:
        v = vec[:, n]
        w = Hw @ v
        l = np.vdot(v, w)
        assert np.linalg.norm(l * v - w) / abs(lam[n]) > 1e-3


# ---- (e) host-side validation: INVALID_ARGUMENT (1) before any device work -------------------------------------------------------------
def _desc(hip, X, data, prec=8, order=2):
    d = hip._lib.SpinorDesc()
    vcb = int(np.prod(X)) // 2
    d.data, d.precision, d.field_order, d.nParity, d.volumeCB, d.stride, d.parity_offset = data, prec, order, 2, vcb, vcb, 12 * vcb
    for i in range(4):
        d.X[i] = X[i]
    return d


def _gauge(hip, X, R=(0, 0, 0, 0), data=4096, prec=8):
    g = hip._lib.GaugeDesc()
    volEx = int(np.prod([X[d] + 2 * R[d] for d in range(4)])) // 2
    g.data, g.precision, g.stride, g.parity_offset = data, prec, volEx, 36 * volEx
    for i in range(4):
        g.X[i], g.R[i] = X[i], R[i]
    return g


def _clover(hip, X, data=8192, prec=8):
    c = hip._lib.CloverDesc()
    vcb = int(np.prod(X)) // 2
    c.data, c.precision, c.volumeCB, c.stride, c.parity_offset = data, prec, vcb, vcb, 36 * vcb
    for i in range(4):
        c.X[i] = X[i]
    return c


def test_host_side_validation_of_the_clover_entry_points(hip):
    lib = hip._lib.load()
    err = lib.mugiq_hip_last_error
    X = (4, 4, 4, 4)
    nbytes = 2 * 12 * 128 * 16
    src, dst, g, C = _desc(hip, X, 1 << 20), _desc(hip, X, (1 << 20) + 4 * nbytes), _gauge(hip, X), _clover(hip, X)
    B = ctypes.byref
    lam, res = (ctypes.c_double * 2)(), (ctypes.c_double * 1)()
    it, rr = (ctypes.c_int * 1)(), (ctypes.c_double * 1)()

    def three(clover, gauge, comm=None):
        """(status, message) of the three operator entries with this clover field"""
        out = [(lib.mugiq_hip_wilson_clover_apply(B(dst), B(src), 1, B(gauge), clover, 0.12, 0, 1.0, comm, None), err()),
               (lib.mugiq_hip_compute_evals_clover(B(src), 1, B(gauge), clover, 0.12, 2, 0, lam, res, res, comm, None), err()),
               (lib.mugiq_hip_wilson_clover_solve(B(dst), B(src), 1, B(gauge), clover, 0.12, None, None, 0, 1e-10, 10, it, rr, comm, None), err())]
        return out
    # sizes
    assert lib.mugiq_hip_clover_bytes(hip._lib.int4(X), 8) == 256 * 72 * 8 and lib.mugiq_hip_clover_bytes(hip._lib.int4(X), 4) == 256 * 72 * 4
    assert lib.mugiq_hip_clover_bytes(hip._lib.int4(X), 2) == 0
    # NULL field / NULL data
    assert lib.mugiq_hip_compute_clover(None, B(g), 0.1, None, None) == 1 and b"clover field is NULL" in err()
    assert lib.mugiq_hip_compute_clover(B(_clover(hip, X, data=None)), B(g), 0.1, None, None) == 1 and b"clover field is NULL" in err()
    assert lib.mugiq_hip_compute_clover(B(C), None, 0.1, None, None) == 1 and b"gauge field is NULL" in err()
    assert lib.mugiq_hip_alloc_clover(None, hip._lib.int4(X), 8) == 1
    assert lib.mugiq_hip_alloc_clover(B(_clover(hip, X)), hip._lib.int4((4, 4, 3, 4)), 8) == 1 and b"even" in err()
    for st, msg in three(B(_clover(hip, X, data=None)), g):
        assert st == 1 and b"clover field is NULL" in msg
    # geometry
    other = _clover(hip, (4, 4, 4, 8))
    assert lib.mugiq_hip_compute_clover(B(other), B(g), 0.1, None, None) == 1 and b"differs" in err()
    for st, msg in three(B(other), g):
        assert st == 1 and b"clover X[3]" in msg
    # precision: the gauge field's
    f32 = _clover(hip, X, prec=4)
    for st, msg in three(B(f32), g):
        assert st == 1 and b"differs from the gauge precision" in msg
    for st, msg in three(B(C), _gauge(hip, X, prec=4)):
        assert st == 1 and b"differs from the gauge precision" in msg
    bad = _clover(hip, X, prec=2)
    assert lib.mugiq_hip_compute_clover(B(bad), B(g), 0.1, None, None) == 1 and b"clover precision" in err()
    # stride / parity offset
    short = _clover(hip, X)
    short.stride = 100
    assert lib.mugiq_hip_compute_clover(B(short), B(g), 0.1, None, None) == 1 and b"stride" in err()
    assert all(st == 1 and b"stride" in msg for st, msg in three(B(short), g))
    short = _clover(hip, X)
    short.parity_offset = 36 * 128 - 1
    assert lib.mugiq_hip_compute_clover(B(short), B(g), 0.1, None, None) == 1 and b"parity_offset" in err()
    assert all(st == 1 and b"parity_offset" in msg for st, msg in three(B(short), g))
    # a partitioned dimension without a border (forced partitioning on one rank: no process group needed)
    comm = hip.GridComm((1, 1, 1, 1), force_partitioned=(0, 0, 0, 1))
    c = comm.c_struct()
    cp = ctypes.cast(ctypes.byref(c), ctypes.c_void_p)
    assert lib.mugiq_hip_compute_clover(B(C), B(g), 0.1, cp, None) == 1 and b"no border" in err()
    assert all(st == 1 and b"no border" in msg for st, msg in three(B(C), g, cp))
    # odd border sum
    assert lib.mugiq_hip_compute_clover(B(C), B(_gauge(hip, X, (0, 0, 0, 1))), 0.1, cp, None) == 1 and b"even" in err()


def test_python_layer_checks_before_the_device(hip):
    with pytest.raises(hip.MugiqHipError):
        hip.wilsonApply([], [], None, 0.12, clover=object())
    with pytest.raises(hip.MugiqHipError):
        hip.wilsonSolve([], None, 0.12, clover=object())
    from mugiq_amd.fields import clover_lower_index
    assert [clover_lower_index(i, j) for i in range(1, 6) for j in range(i)] == list(range(15))
    assert "CloverField" in hip.__all__


# ---- (f) the command line --------------------------------------------------------------------------------------------------------------
def test_cli_flags_parse_and_reach_eigsolve(hip, tmp_path, monkeypatch):
    from mugiq_amd import loop_cli
    ap = loop_cli.build_parser()
    a = ap.parse_args([])
    assert a.dslash_type == "wilson"
    a = ap.parse_args(["--dslash-type", "clover", "--clover-coeff", "0.25"])
    assert a.dslash_type == "clover" and a.clover_coeff == 0.25
    with pytest.raises(SystemExit):
        ap.parse_args(["--dslash-type", "twisted-mass"])
    # main() with the device work replaced: the field is built from the gauge field with the coefficient and handed to Eigsolve_Mugiq
    seen = {}

    class FakeGauge:
        X, precision = (4, 4, 4, 4), 8

    class FakeClover:
        def __init__(self, X, precision):
            seen["clover_init"] = (tuple(X), precision)

        def compute(self, gauge, coeff, comm=None):
            seen["compute"] = (gauge, coeff)
            return self

    class FakeEig:
        def __init__(self, eVecs, gauge, kappa, opType, comm=None, clover=None):
            seen["eig"] = (gauge, kappa, clover)

        def computeEvals(self):
            seen["computed"] = True

        def printEvals(self, file=None):
            pass

    class FakeLoop:
        nLoop = nData = 0

        def __init__(self, *a):
            pass

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
    monkeypatch.setattr(hip, "CloverField", FakeClover)
    monkeypatch.setattr(hip, "Loop_Mugiq", FakeLoop)
    monkeypatch.setattr(hip.eigsolve, "Eigsolve_Mugiq", FakeEig)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    mom = tmp_path / "momenta.txt"
    mom.write_text("0 0 0\n")
    base = ["--loop-ft-sign", "minus", "--loop-calc-type", "opt", "--momenta-filename", str(mom), "--displace-entry-string", "+z:1",
            "--loop-write-mom-space", "no", "--check-evals", "--kappa", "0.11"]
    assert loop_cli.main(base + ["--dslash-type", "clover", "--clover-coeff", "0.25"]) == 0
    assert seen["clover_init"] == ((4, 4, 4, 4), 8) and seen["compute"] == (gauge, 0.25) and seen["computed"]
    assert seen["eig"][0] is gauge and seen["eig"][1] == 0.11 and isinstance(seen["eig"][2], FakeClover)
    seen.clear()
    assert loop_cli.main(base) == 0
    assert "compute" not in seen and seen["eig"][2] is None


# ---- (g) the C++ mirror ----------------------------------------------------------------------------------------------------------------
def test_cpp_clover_mirror_compiles(tmp_path):
    """CloverField and the overloads of wilsonApply, computeEvals, wilsonSolve and Eigsolve_Mugiq that take it: -fsyntax-only."""
    tu = tmp_path / "clover_tu.cpp"
    tu.write_text('#include "mugiq_hip_operators.hpp"\n'
                  "void use(const std::vector<MugiqHipSpinorField> &ev, const std::vector<MugiqHipSpinorField> &x, const MugiqHipGaugeField &U,\n"
                  "         const MugiqHipComm *comm) {\n"
                  "  const int X[4] = {4, 4, 4, 4};\n"
                  "  mugiq_hip::CloverField C(X, 8);\n"
                  "  C.compute(U, 0.1, comm);\n"
                  "  size_t n = mugiq_hip::CloverField::bytes(X, 8);\n"
                  "  (void)n;\n"
                  "  std::vector<std::complex<double>> lam;\n"
                  "  std::vector<double> res, sig, relres;\n"
                  "  std::vector<int> iters;\n"
                  "  mugiq_hip::wilsonApply(x, ev, U, C, 0.12);\n"
                  "  mugiq_hip::wilsonApply(x, ev, U, C, 0.12, MUGIQ_HIP_EIG_OPERATOR_H, 2.0, comm);\n"
                  "  mugiq_hip::wilsonApply(x, ev, U, 0.12);\n"
                  "  mugiq_hip::computeEvals(ev, U, C, 0.12, MUGIQ_HIP_EIG_OPERATOR_H, false, lam, res, sig, comm);\n"
                  "  mugiq_hip::computeEvals(ev, U, 0.12, MUGIQ_HIP_EIG_OPERATOR_H, false, lam, res, sig, comm);\n"
                  "  bool ok = mugiq_hip::wilsonSolve(x, ev, U, C, 0.12, ev, sig, 1e-10, 100, iters, relres, comm);\n"
                  "  ok = mugiq_hip::wilsonSolve(x, ev, U, 0.12, ev, sig, 1e-10, 100, iters, relres, comm) && ok;\n"
                  "  mugiq_hip::Eigsolve_Mugiq es(ev, U, C, 0.12, MUGIQ_HIP_EIG_OPERATOR_H, comm);\n"
                  "  es.computeEvals();\n"
                  "  ok = es.solve(x, ev, 1e-10, 100, iters, relres) && ok;\n"
                  "  mugiq_hip::Eigsolve_Mugiq plain(ev, U, 0.12, MUGIQ_HIP_EIG_OPERATOR_H, comm);\n"
                  "  plain.computeEvals();\n"
                  "  (void)ok;\n"
                  "}\n")
    cc = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cc):
        pytest.skip("no clang++")
    r = subprocess.run([cc, "-std=c++17", "-fsyntax-only", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-Wall", "-I", os.path.join(ROOT, "include"),
                        "-I", "/opt/rocm/include", str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
