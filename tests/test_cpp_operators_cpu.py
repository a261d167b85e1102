"""CPU checks of the C++ operator program tests/cpp/operators.cpp (its GPU run is tests/test_gpu_cpp_operators.py): it compiles and links
against libmugiq_hip.so; its host self-test passes (detail::mgOutputs / mgHistory / mgLevels and the dense host helpers against numpy);
--parse-only round-trips a manifest written by tests/cpp_exchange.py; and a coverage guard: every function, class and public member that
include/mugiq_hip_operators.hpp declares in namespace mugiq_hip outside detail is executed by that program (its --list) or by
tests/cpp/loop.cpp -- a wrapper added later without being run fails here."""
import os
import re
import subprocess

import numpy as np

import cpp_exchange as cx
from util import ROOT

HEADER = os.path.join(ROOT, "include", "mugiq_hip_operators.hpp")
LOOP_CPP = os.path.join(ROOT, "tests", "cpp", "loop.cpp")

# what tests/cpp/loop.cpp executes by name (tests/test_cpp_host.py runs it on the GPU) and tests/cpp/operators.cpp does not
LOOP_CPP_EXECUTES = ["performLoopContraction", "Loop_Mugiq::writeLoopsHDF5", "Loop_Mugiq::handle", "Loop_Mugiq::dataMom_bcast", "GaugeParam"]


def _run(*args):
    return subprocess.run([cx.EXE] + list(args), capture_output=True, text=True, timeout=300)


def test_operator_program_compiles_and_links(hip):
    cx.build()
    assert os.path.exists(cx.EXE)


def test_host_selftest(hip, tmp_path):
    """mgOutputs: maxIter 0 gives stride 1, no history buffer unless asked for, the sizes for 3 right-hand sides; mgHistory slices
    [i stride, i stride + iters[i]), returns false for status 5 with the history filled, throws status 1, accepts a null history; mgLevels
    throws on mismatched sizes; hermitianEigh, choleskyUpper (a rank-deficient G: status 1) and upperTriangularInverse on a 5 x 5 matrix
    against numpy's values, passed in as %a"""
    cx.build_if_stale()
    rng = np.random.default_rng(55)
    A = rng.standard_normal((5, 5)) + 1j * rng.standard_normal((5, 5))
    H, G = A + A.conj().T, A.conj().T @ A + np.eye(5)
    R = np.linalg.cholesky(G).conj().T                                       # G = R^dag R, R upper triangular with a positive diagonal
    vals = np.concatenate([np.ascontiguousarray(M).view(np.float64).reshape(-1) for M in (H, G)] + [np.linalg.eigvalsh(H)] +
                          [np.ascontiguousarray(M).view(np.float64).reshape(-1) for M in (R, np.linalg.inv(R))])
    path = tmp_path / "dense.txt"
    path.write_text(" ".join(float(v).hex() for v in vals))
    out = _run("--host-selftest", str(path))
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "HOST SELFTEST PASSED" in out.stdout


def test_parse_only_round_trips_a_manifest(hip, tmp_path):
    """every kind of object with every descriptor member, an int64_t parity_offset above 2^31 and a negative-exponent %a double"""
    cx.build_if_stale()
    w = cx.CaseWriter(tmp_path)
    big = 2 ** 31 + 12 * 1027
    w.descriptor("fine", "spinor", dict(precision=8, order=4, X=[8, 4, 4, 6], volumeCB=384, stride=391, parity_offset=big))
    w.descriptor("w", "coarse", dict(precision=4, nSpin=2, nColor=24, X=[4, 2, 2, 2], volumeCB=16, stride=19, parity_offset=2 * 24 * 19))
    w.descriptor("U", "gauge", dict(precision=8, X=[4, 4, 4, 4], R=[0, 0, 2, 2], stride=1031, parity_offset=36 * 1031))
    w.descriptor("A", "clover", dict(precision=4, X=[8, 4, 4, 4], volumeCB=256, stride=261, parity_offset=36 * 261 + 5))
    w.descriptor("T1", "transfer", dict(precision=8, nVec=3, geoBlockSize=[2, 1, 1, 1], spinBlockSize=1, X=[4, 2, 2, 2], stride=19, parity_offset=2 * 4 * 3 * 19))
    w.descriptor("op", "coarseop", dict(precision=8, nVec=5, X=[2, 2, 2, 2], volumeCB=8, kappa=0.12, hasClover=1))
    w.scalars("tol", [1e-10, -0.0, 5e-324, 0.1, -1.7976931348623157e308])
    w.scalars("none", [])
    w.close()
    assert "p-34" in open(tmp_path / "manifest.txt").read()                  # 1e-10 = 0x1.b7cdfd9d7bdbbp-34
    out = _run("--parse-only", str(tmp_path))
    assert out.returncode == 0, out.stderr
    want, got = cx.read_manifest(tmp_path / "manifest.txt"), cx.read_manifest(tmp_path / "manifest.out.txt")
    assert len(want) == 8 and want[0][3]["parity_offset"] == big > 2 ** 31
    for a, b in zip(want, got):
        assert a[:3] == b[:3], (a, b)
        if a[0] == "scalars":
            assert np.array_equal(np.array(a[3]["values"]).view(np.int64), np.array(b[3]["values"]).view(np.int64)), (a, b)
        else:
            assert a[3] == b[3], (a, b)
    assert len(got) == len(want)
    bad = _run("--parse-only", str(tmp_path / "nowhere"))
    assert bad.returncode != 0


def declared_names(text):
    """the functions, classes and public members (as Class::member; a constructor counts as its class) that the header declares in
    namespace mugiq_hip outside namespace detail"""
    text = re.sub(r"^namespace detail \{.*?^\}  // namespace detail$", "", text, flags=re.S | re.M)
    assert "namespace detail" not in text
    text = re.sub(r"//[^\n]*", "", text)
    names = set(re.findall(r"^(?:template <[^>]*>\s*)?(?:inline|constexpr)\s+[^;{(=]*?\b(\w+)\(", text, flags=re.M))
    for m in re.finditer(r"^(?:template <[^>]*>\s*)?(class|struct)\s+(\w+)[^;{]*\{(.*?)^\};", text, flags=re.S | re.M):
        kind, cls, body = m.groups()
        names.add(cls)
        if kind == "class":
            body = "".join(re.findall(r"^public:(.*?)(?=^private:|\Z)", body, flags=re.S | re.M))
        for line in re.findall(r"^  (?![ }])([^\n]*\()", body, flags=re.M):
            found = re.search(r"(~?\w+)\($", line[:line.index("(") + 1])
            if not found:
                continue                                                      # a cast or an initialiser, not a declaration
            member = found.group(1)
            if member.startswith("~") or "operator" in line.split("(")[0] or re.search(r"\b%s\(const %s &\)" % (cls, cls), line):
                continue                                                      # destructors, deleted copies
            names.add(cls if member == cls else cls + "::" + member)
    return names


def test_every_declared_name_is_executed(hip):
    cx.build_if_stale()
    declared = declared_names(open(HEADER).read())
    # the parser sees what it must: free functions, templates, classes, structs, members, constructors -- and nothing of detail or private
    for name in ("mgSolve", "precisionOf", "createPhaseMatrixGPU", "CoarseOperator", "CoarseOperator::desc", "CloverField::bytes", "MgSolveParam",
                 "Eigsolve_Mugiq::getEvalsSigma", "Loop_Mugiq::deflateCoarse", "Displace::doVectorDisplacement", "Error", "computeLoop", "transferForm"):
        assert name in declared, name
    assert not declared & {"mgLevels", "mgOutputs", "mgHistory", "detail", "Loop_Mugiq::fill", "Loop_Mugiq::CParam"} and len(declared) > 90
    listed = set(_run("--list").stdout.split())
    assert listed and listed <= declared, listed - declared
    loop_src = open(LOOP_CPP).read()
    for name in LOOP_CPP_EXECUTES:
        assert name in declared and re.search(r"\b%s\b" % name.split("::")[-1], loop_src), name + " does not occur in tests/cpp/loop.cpp"
    missing = declared - listed - set(LOOP_CPP_EXECUTES)
    assert not missing, "declared in mugiq_hip_operators.hpp and executed by neither C++ program: %s" % sorted(missing)
