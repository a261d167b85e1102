"""CPU-only checks of mugiq_hip_convert_and_project_plan: the host helper through which the launcher of the fused reorder +
momentum projection chooses its x-step kernel (general / pipelined / matrix pipe <NKS, MB>), tiling and LDS layout.  No GPU is
touched: the query runs the compute call's validation and dispatch and stops before any HIP call."""
import ctypes
import os
import re

import numpy as np
import pytest

import projection_cases as pc
from util import ROOT

GENERAL, PIPELINED, MFMA = 0, 1, 2


def _plan(hip, X, prec, npx=3, nData=16):
    return hip.convertAndProjectPlan([(p, 0, 0) for p in range(npx)], X, nData, prec)


def _instantiated():
    """The <NKS, MB> pairs csrc/momproj.hip instantiates: the one list both the dispatch and the planner expand."""
    src = open(os.path.join(ROOT, "mugiq_amd", "csrc", "momproj.hip")).read()
    m = re.search(r"#define MUGIQ_EO_MFMA_INSTANCES\(CASE\)((?:.*\\\n)*.*)\n", src)
    assert m, "the instantiation list of eo_dft_x_mfma_kernel has moved"
    pairs = {(int(a), int(b)) for a, b in re.findall(r"CASE\((\d+), (\d+)\)", m.group(1))}
    assert not re.search(r"eo_dft_x_mfma_kernel<\s*\d", src), "an instantiation outside the list"
    return pairs


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in ("MUGIQ_HIP_EO_MFMA", "MUGIQ_HIP_EO_TILES_PER_WG"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("X,nData,form,nks,mb,tChunk,perWg", [
    ((48, 48, 24, 24), 400, MFMA, 6, 3, None, 24),          # configs[2]: 25 slots, the headline shape
    ((64, 64, 32, 16), 16, MFMA, 8, 2, None, None),
    ((32, 32, 32, 32), 16, MFMA, 4, 4, None, None),
    ((48, 48, 48, 96), 16, MFMA, 6, 3, 24, None)])          # one GPU's view of 48^3 x 96
def test_production_plans(hip, X, nData, form, nks, mb, tChunk, perWg):
    """The production shapes take the forms DESIGN.md and the profiles name: matrix pipe in fp64, pipelined in fp32."""
    mom7 = [(p, 0, 0) for p in range(-3, 4)]          # p^2 <= 9: 7 distinct p_x
    p = hip.convertAndProjectPlan(mom7, X, nData, 8)
    assert (p["form"], p["nks"], p["mb"]) == (form, nks, mb), p
    assert p["nPx"] == 7 and p["ldsBytes"] <= 64 * 1024
    if tChunk is not None:
        assert p["tChunk"] == tChunk and p["nChunks"] * tChunk == X[3]
    if perWg is not None:
        assert p["tilesPerWg"] == perWg and p["workgroupsX"] == 1
    p32 = hip.convertAndProjectPlan(mom7, X, nData, 4)
    assert p32["form"] == PIPELINED and (p32["nks"], p32["mb"]) == (0, 0), p32


def test_plan_honours_the_switches(hip, monkeypatch):
    mom = [(0, 0, 0), (1, 0, 0)]
    X = (48, 6, 2, 48)
    assert hip.convertAndProjectPlan(mom, X, 16, 8)["form"] == MFMA
    monkeypatch.setenv("MUGIQ_HIP_EO_MFMA", "0")
    p = hip.convertAndProjectPlan(mom, X, 16, 8)
    assert p["form"] == PIPELINED and p["tilesPerWg"] == 1 and p["tiles"] == 6
    for want, got in ((4, 4), (6, 6), (99, 6), (0, 1)):
        monkeypatch.setenv("MUGIQ_HIP_EO_TILES_PER_WG", str(want))
        p = hip.convertAndProjectPlan(mom, X, 16, 8)
        assert p["tilesPerWg"] == got and p["workgroupsX"] == -(-6 // got)
    # the general form walks nothing
    assert hip.convertAndProjectPlan(mom, (128, 6, 2, 8), 16, 8)["tilesPerWg"] == 1


def test_plan_runs_the_compute_calls_validation(hip):
    lib = hip._lib.load()
    mom = (ctypes.c_int * 3)(0, 0, 0)
    plan = hip._lib.ProjectPlan()
    bad = [((4, 4, 4, 3), 16, 8, b"even"), ((4, 4, 4, 4), 17, 8, b"nData = nLoop * NGamma"), ((4, 4, 4, 4), 16, 2, b"Precision"),
           ((2048, 2048, 256, 4), 16, 8, b"overflows"), ((4, 4, 65538, 4), 16, 8, b"too large"), ((8192, 2, 2, 2), 16, 8, b"too large")]
    for X, nData, prec, msg in bad:
        st = lib.mugiq_hip_convert_and_project_plan(mom, 1, hip._lib.int4(X), nData, prec, ctypes.byref(plan))
        assert st == 1 and msg in lib.mugiq_hip_last_error(), (X, nData, prec, lib.mugiq_hip_last_error())
    assert lib.mugiq_hip_convert_and_project_plan(mom, 1, hip._lib.int4((4, 4, 4, 4)), 16, 8, None) == 1
    with pytest.raises(hip.MugiqHipError):
        hip.convertAndProjectPlan([(0, 0, 0)], (4, 4, 4, 4), 16, 3)


def _check_invariants(p, X, prec, npx):
    Lx, Lt = X[0], X[3]
    assert p["ldsBytes"] <= 64 * 1024, (X, prec, npx, p)
    assert p["tChunk"] >= 1 and p["tChunk"] * p["nChunks"] >= Lt and p["tChunk"] * (p["nChunks"] - 1) < Lt, (X, prec, npx, p)
    assert p["lastChunk"] == Lt - p["tChunk"] * (p["nChunks"] - 1) and 1 <= p["lastChunk"] <= p["tChunk"]
    assert p["tiles"] == (X[1] // 2) * p["nChunks"] and p["workgroupsX"] * p["tilesPerWg"] >= p["tiles"]
    assert p["nPx"] == npx and p["pxPasses"] == -(-npx // 8) and p["rowPasses"] == -(-2 * p["tChunk"] // 64)
    assert p["stagingPieces"] == -(-Lx // 64)
    # the tile ([2 tChunk rows][Lx + 1]) and the partial-sum area behind or in it fit what is asked for
    tile, red = 2 * p["tChunk"] * (Lx + 1), 2304
    assert p["redOffset"] in (0, tile) and (p["redOffset"] + red if p["redOffset"] else max(tile, red)) * 2 * prec <= p["ldsBytes"]
    if p["rowPasses"] > 1 or p["pxPasses"] > 1:
        assert p["redOffset"] == tile          # a later pass needs the rows again
    if p["form"] != GENERAL:                   # the pipelined staging: 4 waves x 12 loads of 64 / run runs each cover the 2 tChunk runs
        assert Lx <= 64 and p["lastChunk"] == p["tChunk"] and -(-2 * p["tChunk"] // (64 // Lx)) <= 48, (X, prec, npx, p)
    else:
        assert p["tilesPerWg"] == 1
    if p["form"] == MFMA:
        assert prec == 8 and 2 * p["tChunk"] <= 64 and npx <= 8 and p["rowPasses"] == 1 and p["redOffset"] == 0, (X, prec, npx, p)
        assert p["nks"] * 8 == Lx and p["mb"] == -(-2 * p["tChunk"] // 16) and 16 * p["mb"] <= 64
    else:
        assert (p["nks"], p["mb"]) == (0, 0)


def test_exhaustive_sweep_reaches_exactly_the_instantiated_matrix_pipe_kernels(hip):
    """Even Lx, Lt <= 256, 1..8 distinct p_x, both precisions: every (NKS, MB) the plan returns is instantiated (else the query
    itself fails) and every instantiation is returned for some shape -- no dead kernel that looks like coverage."""
    lib = hip._lib.load()
    plan = hip._lib.ProjectPlan()
    seen, forms = set(), {GENERAL: 0, PIPELINED: 0, MFMA: 0}
    moms = {n: (ctypes.c_int * (3 * n))(*[v for p in range(n) for v in (p - 3, 0, 0)]) for n in range(1, 9)}
    names = [n for n, _ in plan._fields_]
    for prec in (8, 4):
        for Lx in range(2, 257, 2):
            for Lt in range(2, 257, 2):
                X = hip._lib.int4((Lx, 2, 2, Lt))
                for npx in range(1, 9):
                    st = lib.mugiq_hip_convert_and_project_plan(moms[npx], npx, X, 16, prec, ctypes.byref(plan))
                    assert st == 0, (Lx, Lt, npx, prec, lib.mugiq_hip_last_error())
                    forms[plan.form] += 1
                    if plan.form == MFMA:
                        seen.add((plan.nks, plan.mb))
                    if npx in (1, 8):
                        _check_invariants({n: getattr(plan, n) for n in names}, (Lx, 2, 2, Lt), prec, npx)
    assert seen == _instantiated(), (sorted(seen), sorted(_instantiated()))
    assert all(forms.values()), forms


def test_invariants_up_to_very_long_rows(hip):
    """Lx up to several thousand, up to 20 distinct p_x: the LDS stays within 64 KiB with at least one time slice per tile, or the
    call is rejected as too large (a single time slice of the y pair does not fit) -- never a plan with tChunk = 0."""
    rejected = 0
    for prec in (8, 4):
        for Lx in list(range(258, 1024, 38)) + list(range(1024, 8200, 250)) + [2046, 2048, 4094, 4096]:
            for Lt in (2, 8, 34, 128):
                for npx in (1, 8, 9, 20):
                    try:
                        p = _plan(hip, (Lx, 2, 2, Lt), prec, npx)
                    except hip.MugiqHipError as e:
                        assert "too large" in str(e)
                        # documented rejection: even one time slice (plus the partial sums) is beyond the LDS
                        one = 2 * (Lx + 1)          # in the partial sums' place if one pass of 8 p_x covers it, else in front of them
                        assert (max(one, 2304) if npx <= 8 else one + 2304) * 2 * prec > 64 * 1024, (Lx, Lt, npx, prec)
                        rejected += 1
                        continue
                    assert p["form"] == GENERAL
                    _check_invariants(p, (Lx, 2, 2, Lt), prec, npx)
    assert rejected > 0
    for prec in (8, 4):          # and the many-p_x side of the small shapes
        for Lx in (2, 6, 24, 32, 48, 64, 66):
            for Lt in (2, 10, 34, 46, 64, 96, 250):
                for npx in (9, 16, 17):
                    _check_invariants(_plan(hip, (Lx, 2, 2, Lt), prec, npx), (Lx, 2, 2, Lt), prec, npx)


@pytest.mark.parametrize("c", pc.ALL_CASES, ids=lambda c: c["id"])
def test_gpu_table_lands_in_its_class(hip, c, monkeypatch):
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    nData = 16 * c["nLoop"]
    plan = hip.convertAndProjectPlan(pc.momenta(c["pxs"]), c["X"], nData, c["prec"])
    assert plan["nPx"] == len(c["pxs"])
    assert not pc.plan_matches(plan, c["expect"]), (c["id"], pc.plan_matches(plan, c["expect"]), plan)


def test_gpu_table_covers_what_it_claims():
    """Every instantiation and every weak spot the GPU file is there for has a row in the table."""
    assert {(c[0]["expect"]["nks"], c[0]["expect"]["mb"]) for c in pc.MFMA_CASES} == _instantiated()
    assert {len(c[0]["pxs"]) for c in pc.MFMA_CASES} == {1, 3, 7, 8}
    ex = [c["expect"] for c in pc.GENERAL_CASES + [pc.TWO_ROW_PASS_CASE]]
    assert any(e.get("ragged") for e in ex) and any(e.get("pxPasses") == 2 and e.get("redBehind") for e in ex)
    assert any(e.get("stagingPieces") == 3 for e in ex) and any(e.get("rowPasses") == 2 for e in ex)
    assert any(e["tChunk"] % 2 == 1 and e["nChunks"] > 1 for e in (c[0]["expect"] for c in pc.MFMA_CASES))          # parity follows t0
    for group in ([c for t in pc.MFMA_CASES for c in t], pc.GENERAL_CASES, pc.WALK_CASES, pc.NATURAL_WALK_CASES, pc.SLOT_CASES):
        assert any(c["grid"] != (1, 1, 1) for c in group)
    for c in pc.WALK_CASES:
        assert c["expect"]["tiles"] >= 5
    assert any(c["expect"]["tiles"] % c["expect"]["tilesPerWg"] and c["expect"]["nChunks"] > 1 for c in pc.WALK_CASES)
    assert {c["expect"]["form"] for c in pc.SLOT_CASES} == {pc.GENERAL, pc.PIPELINED, pc.MFMA}
    assert {c["expect"]["form"] for c in pc.POISON_CASES} == {pc.GENERAL, pc.PIPELINED, pc.MFMA}


def test_seeded_sweep_draws_every_form(hip):
    """The default 24 seeds of the GPU sweep reach each of the three forms at least twice (the seed base was picked for that)."""
    count = {GENERAL: 0, PIPELINED: 0, MFMA: 0}
    for seed in range(24):
        d = pc.sweep_draw(np, seed)
        count[hip.convertAndProjectPlan(d["mom"], d["X"], 16 * d["nLoop"], d["prec"])["form"]] += 1
    assert min(count.values()) >= 2, count
