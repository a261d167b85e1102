"""CPU-only checks of mugiq_hip_transfer_form: the host query of the one selector (csrc/transfer_form.cpp) through which
mugiq_hip_prolongate_batched and mugiq_hip_prolongate_contract_batched choose their kernel form and launch geometry.  No GPU is touched.
The expected values were worked out by hand from the selection rules (LDS of a workgroup: 163840 bytes; a complex is 16 bytes in fp64,
8 in fp32)."""
import glob
import os

import pytest

P_MFMA, P_STAGED, P_GLOBAL = 1, 2, 3                                     # MUGIQ_HIP_PROLONG_FAMILY_*
C_COARSE_MFMA, C_COARSE_VECTOR, C_DIRECT_STAGED, C_DIRECT_GLOBAL = 1, 2, 3, 4   # MUGIQ_HIP_CONTRACT_FAMILY_*
SWITCHES = ("MG_PLAN", "MG_MFMA", "PROLONG_MFMA", "PROLONG_PASS_BLOCKS")
# the shapes of test_gpu_operators.py::test_prolongator_matches_oracle: (X, geo_block_size, n_vec) -> prolongator family (fp64 FLOAT2),
# its LDS bytes, aggregate volume
SHAPES = [
    ((8, 8, 8, 8), (4, 4, 4, 4), 24, P_MFMA, 6144 * 24, 256),
    ((8, 8, 4, 4), (4, 2, 2, 2), 24, P_MFMA, 6144 * 24, 32),
    ((8, 4, 12, 4), (2, 2, 3, 2), 6, P_STAGED, 18432, 24),
    ((4, 4, 4, 6), (2, 2, 2, 1), 3, P_STAGED, 9216, 8),
    ((4, 4, 4, 4), (2, 2, 2, 2), 64, P_GLOBAL, 0, 16),
]
X8, B4, B2 = (8, 8, 8, 8), (4, 4, 4, 4), (2, 2, 2, 2)


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv("MUGIQ_HIP_" + k, raising=False)


def _form(hip, X, bs, n_vec, prec=8, nVec=5, **kw):
    return hip.transferForm((X, bs, n_vec, prec), nVec, **kw)


def _vector_prolong(f, family, lds, X):
    vcb = X[0] * X[1] * X[2] * X[3] // 2
    assert (f["prolongFamily"], f["prolongLdsBytes"], f["prolongThreads"], f["prolongWorkgroups"], f["prolongPasses"]) == \
        (family, lds, 256, 2 * ((vcb + 15) // 16), 0), f


@pytest.mark.parametrize("mfma", [None, "0"])
@pytest.mark.parametrize("X,bs,n_vec,family,lds,aggVol", SHAPES)
def test_prolongator_shapes(hip, monkeypatch, X, bs, n_vec, family, lds, aggVol, mfma):
    if mfma is not None:
        monkeypatch.setenv("MUGIQ_HIP_PROLONG_MFMA", mfma)
    f = _form(hip, X, bs, n_vec)
    Xc = [x // b for x, b in zip(X, bs)]
    volc = Xc[0] * Xc[1] * Xc[2] * Xc[3]
    assert (f["X"], f["bs"], f["Xc"]) == (list(X), list(bs), Xc)
    assert (f["aggVol"], f["volumeCB"], f["volumeCBc"]) == (aggVol, X[0] * X[1] * X[2] * X[3] // 2, volc // 2)
    assert f["prolongWorkspaceBytes"] == 16 * volc * 2 * n_vec * 8                      # nVec 5 -> 8, whatever the family
    if family == P_MFMA and mfma is None:
        assert (f["prolongFamily"], f["prolongLdsBytes"], f["prolongThreads"], f["prolongWorkgroups"]) == (P_MFMA, lds, 512, volc), f
        assert (f["prolongPasses"], f["prolongBlocksPerPass"]) == (1, 1)
    elif family == P_MFMA:                                                              # the switch: the vector row of the same shape
        _vector_prolong(f, P_STAGED, 16 * 12 * n_vec * 16, X)
    else:
        _vector_prolong(f, family, lds, X)
    for prec, order in ((8, 4), (4, 2), (4, 4)):
        g = hip.transferForm((X, bs, n_vec, prec), 5, fineOrder=order)
        _vector_prolong(g, P_GLOBAL if (prec, n_vec) == (8, 64) else P_STAGED, 0 if (prec, n_vec) == (8, 64) else 2 * prec * 12 * n_vec * 16, X)


def test_matrix_pipe_needs_its_n_vec_and_whole_rounds(hip):
    for n_vec in range(1, 65):
        want = P_MFMA if n_vec in (8, 16, 24) else P_STAGED if n_vec <= 53 else P_GLOBAL
        assert _form(hip, X8, B4, n_vec)["prolongFamily"] == want, n_vec
    assert _form(hip, X8, B4, 8)["prolongLdsBytes"] == 6144 * 8 and _form(hip, X8, B4, 24)["prolongLdsBytes"] == 147456
    assert _form(hip, (8, 8, 8, 4), (2, 2, 2, 1), 24)["prolongFamily"] == P_STAGED      # aggregates of 8 sites
    assert _form(hip, (12, 4, 4, 4), (6, 2, 2, 1), 24)["prolongFamily"] == P_STAGED     # ... of 24


def test_vector_tile_boundaries(hip):
    f = _form(hip, X8, B4, 53)
    assert (f["prolongFamily"], f["prolongLdsBytes"]) == (P_STAGED, 162816)
    f = _form(hip, X8, B4, 54)
    assert (f["prolongFamily"], f["prolongLdsBytes"]) == (P_GLOBAL, 0)
    f = _form(hip, X8, B4, 64, prec=4)
    assert (f["prolongFamily"], f["prolongLdsBytes"]) == (P_STAGED, 98304)


@pytest.mark.parametrize("switch,nVec,passes,per", [(None, 5, 1, 1), (None, 66, 1, 9), (None, 203, 2, 13), ("7", 203, 4, 7),
                                                    ("0", 203, 2, 13), ("17", 203, 2, 13), ("16", 203, 2, 13), ("1", 17, 3, 1)])
def test_matrix_pipe_passes(hip, monkeypatch, switch, nVec, passes, per):
    if switch is not None:
        monkeypatch.setenv("MUGIQ_HIP_PROLONG_PASS_BLOCKS", switch)
    f = _form(hip, X8, B4, 24, nVec=nVec)
    blocks = (nVec + 7) // 8
    assert (f["prolongFamily"], f["prolongPasses"], f["prolongBlocksPerPass"]) == (P_MFMA, passes, per), f
    assert [min(per, blocks - b) for b in range(0, blocks, per)] == ([7, 7, 7, 5] if switch == "7" else [per] * (passes - 1) + [blocks - per * (passes - 1)])
    assert f["prolongWorkspaceBytes"] == 16 * 16 * 2 * 24 * 8 * blocks


# ---- prolong-contract.  (precision, loopPrecision) -> bytes of a stored and of an accumulated complex
PAIRS = {(8, 8): (16, 16), (4, 4): (8, 8), (4, 8): (8, 16)}


@pytest.mark.parametrize("prec,lprec", list(PAIRS))
@pytest.mark.parametrize("plan", [None, "direct", "coarse"])
@pytest.mark.parametrize("mfma", [None, "0", "1"])
def test_contract_families(hip, monkeypatch, prec, lprec, plan, mfma):
    if plan is not None:
        monkeypatch.setenv("MUGIQ_HIP_MG_PLAN", plan)                                   # only the exact string "direct" switches it off
    if mfma is not None:
        monkeypatch.setenv("MUGIQ_HIP_MG_MFMA", mfma)
    cF, cA = PAIRS[(prec, lprec)]
    nVec = 5
    for X, bs in ((X8, B4), ((8, 8, 4, 4), (4, 2, 2, 2)), ((8, 8, 8, 4), (2, 2, 2, 1))):
        aggVol = bs[0] * bs[1] * bs[2] * bs[3]
        vcb, volc = X[0] * X[1] * X[2] * X[3] // 2, X[0] * X[1] * X[2] * X[3] // aggVol
        for n_vec in range(1, 65):
            f = hip.transferForm((X, bs, n_vec, prec), nVec, loopPrecision=lprec)
            tile, red = cF * 12 * n_vec * 16, 4096 * (cA // 2)
            if n_vec in (8, 12, 16, 24, 32) and plan != "direct":
                assert f["outerB"] == (2 * n_vec + 15) // 16 and f["contractWorkgroups"] == volc
                assert f["contractScratchBytes"] == (8 * nVec + (cA // 2) * nVec + 255) // 256 * 256 + cA * volc * 4 * n_vec * n_vec
                if lprec == 8 and n_vec != 12 and aggVol % 16 == 0 and mfma != "0":
                    glds = prec == 8 and 2 * 3072 * n_vec + 512 * n_vec <= 163840
                    assert (f["contractFamily"], f["glds"], f["contractLdsBytes"], f["contractThreads"]) == \
                        (C_COARSE_MFMA, int(glds), (2 if glds else 1) * 3072 * n_vec + 512 * n_vec, 32 * n_vec), f
                    assert (f["JC"], f["SPR"], f["NH"]) == (0, 0, 0)
                else:
                    JC = 12 if n_vec % 12 == 0 else 8
                    lds = lambda spr: cA * (4 * n_vec * n_vec + 16 * spr) + cF * 4 * n_vec * spr
                    SPR = 32 if lds(64) > 153600 else 64
                    assert (f["contractFamily"], f["JC"], f["NH"], f["SPR"], f["contractLdsBytes"], f["glds"]) == \
                        (C_COARSE_VECTOR, JC, n_vec // JC, SPR, lds(SPR), 0), f
                    assert f["contractThreads"] == 4 * (n_vec // JC) * SPR <= 1024 and lds(SPR) <= 153600
            else:
                staged = tile <= 163840
                assert (f["contractFamily"], f["contractLdsBytes"]) == (C_DIRECT_STAGED if staged else C_DIRECT_GLOBAL, max(tile, red) if staged else red), f
                assert (f["contractThreads"], f["contractWorkgroups"]) == (256, 2 * ((vcb + 15) // 16))
                assert (f["outerB"], f["JC"], f["SPR"], f["NH"], f["glds"], f["contractScratchBytes"]) == (0, 0, 0, 0, 0, 0)


def test_contract_examples(hip, monkeypatch):
    seen = set()

    def q(n_vec, prec=8, lprec=0, X=X8, bs=B4):
        f = _form(hip, X, bs, n_vec, prec=prec, loopPrecision=lprec)
        seen.add(f["contractFamily"])
        return f
    f = q(24)
    assert (f["contractFamily"], f["glds"], f["contractLdsBytes"]) == (C_COARSE_MFMA, 1, 159744)
    f = q(32)
    assert (f["contractFamily"], f["glds"], f["contractLdsBytes"]) == (C_COARSE_MFMA, 0, 114688)
    assert q(24, prec=4, lprec=8)["glds"] == 0 and q(24, prec=4, lprec=4)["contractFamily"] == C_COARSE_VECTOR
    f = q(12)
    assert (f["contractFamily"], f["JC"], f["NH"], f["SPR"]) == (C_COARSE_VECTOR, 12, 1, 64)
    assert (q(64)["contractFamily"], q(64)["contractLdsBytes"]) == (C_DIRECT_GLOBAL, 4096 * 8)
    assert (q(3)["contractFamily"], q(3)["contractLdsBytes"]) == (C_DIRECT_STAGED, 4096 * 8)      # the tile (9216) is the smaller
    assert q(3, prec=4, lprec=4)["contractLdsBytes"] == 4096 * 4 and q(40)["contractLdsBytes"] == 16 * 12 * 40 * 16
    monkeypatch.setenv("MUGIQ_HIP_MG_MFMA", "0")
    f = q(32)
    assert (f["contractFamily"], f["JC"], f["NH"], f["SPR"], f["contractLdsBytes"]) == (C_COARSE_VECTOR, 8, 4, 32, 139264)
    f = q(24)
    assert (f["contractFamily"], f["JC"], f["NH"], f["SPR"], f["contractLdsBytes"]) == (C_COARSE_VECTOR, 12, 2, 64, 151552)
    assert seen == {C_COARSE_MFMA, C_COARSE_VECTOR, C_DIRECT_STAGED, C_DIRECT_GLOBAL}


def test_invalid_transfers_are_refused_like_the_compute_calls(hip):
    with pytest.raises(hip.MugiqHipError, match=r"n_vec = 65 must be in \[1, 64\]"):
        _form(hip, X8, B4, 65)
    with pytest.raises(hip.MugiqHipError, match="coarse extent 1 in dim 3 must be even"):
        _form(hip, (8, 8, 8, 4), (4, 4, 4, 4), 24)
    with pytest.raises(hip.MugiqHipError, match=r"geo_block_size\[0\] = 3 does not divide X = 8"):
        _form(hip, X8, (3, 4, 4, 4), 24)
    with pytest.raises(hip.MugiqHipError):
        _form(hip, X8, (0, 4, 4, 4), 24)
    with pytest.raises(hip.MugiqHipError):
        _form(hip, X8, B4, 24, nVec=0)
    with pytest.raises(hip.MugiqHipError, match="loop precision 4 with field precision 8"):
        _form(hip, X8, B4, 24, loopPrecision=4)


@pytest.mark.parametrize("X,bs,n_vec", [s[:3] for s in SHAPES])
def test_coarse_side_layout_and_workspace_head(hip, X, bs, n_vec):
    """The coarser side's fields as the library lays them out (restriction, coarse deflation, the driver's levels), and the head of the
    workspace computeEvalsCoarse leaves to the prolongator for its blocks of kEvBlock = 8 eigenvectors"""
    f = _form(hip, X, bs, n_vec, nVec=8)
    volc = 1
    for x, b in zip(X, bs):
        volc *= x // b
    assert (f["coarseNColor"], f["coarseStride"], f["coarseParityOffset"]) == (n_vec, volc // 2, 2 * n_vec * (volc // 2))
    assert f["prolongWorkspaceBytes"] == 16 * volc * 2 * n_vec * 8                      # sizeof(complex double) volc 2 n_vec ceil8(8)


def test_switches_are_read_in_one_place():
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mugiq_amd", "csrc")
    with open(os.path.join(src, "prolong.hip")) as f:
        assert f.read().count("getenv") == 0
    for path in glob.glob(os.path.join(src, "*")):
        if os.path.isfile(path) and os.path.basename(path) != "transfer_form.cpp":
            with open(path, errors="ignore") as f:
                text = f.read()
            for k in SWITCHES:
                assert "MUGIQ_HIP_" + k not in text, (path, k)
