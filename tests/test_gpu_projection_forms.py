"""Every kernel form of the fused reorder + momentum projection (convertAndProject) against the fp64 numpy chain of the oracle:
convert_idx_order_map_gamma -> phase_matrix -> momentum_projection_local.  The x step is dispatched by shape among the general
kernel, the pipelined kernel and ten instantiations of the matrix-pipe kernel; each case first asserts, through the plan query,
that it takes the form it is here for (tests/projection_cases.py holds the table, tests/test_projection_plan_cpu.py checks it
without a GPU), then compares.  Bounds as in test_gpu_operators.py: 1e-13 (fp64), 1e-5 (fp32), relative to the largest element.
"""
import os

import numpy as np
import pytest
import torch

import projection_cases as pc
from util import orc, rel_err

pytestmark = pytest.mark.gpu

TOL = {8: 1e-13, 4: 1e-5}
FORM_NAME = {0: "general", 1: "pipelined", 2: "mfma"}


def _cdt(prec):
    return np.complex128 if prec == 8 else np.complex64


def _tdt(prec):
    return torch.complex128 if prec == 8 else torch.complex64


def _pos(rng, n, prec):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(_cdt(prec))


def _oracle(pos, X, nLoop, mom, FTSign, tot, coord, prec):
    """The reference's sequence in fp64 on the inputs the GPU sees (phases rounded to the storage precision, as the reference's are)."""
    V, locV3, nData = int(np.prod(X)), X[0] * X[1] * X[2], 16 * nLoop
    mp_ = orc.convert_idx_order_map_gamma(pos.astype(np.complex128), nData, nLoop, 2, V // 2, X)
    ph = orc.phase_matrix(mom, locV3, FTSign, X, tot, coord, dtype=np.float64 if prec == 8 else np.float32)
    return orc.momentum_projection_local(mp_, ph.astype(np.complex128), X[3], nData, locV3, len(mom))


def _set_env(monkeypatch, env):
    for k in ("MUGIQ_HIP_EO_MFMA", "MUGIQ_HIP_EO_TILES_PER_WG"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _assert_class(hip, c, nData=None):
    """The case takes the kernel form its row names (the switches of the case are set already)."""
    plan = hip.convertAndProjectPlan(pc.momenta(c["pxs"]), c["X"], nData or 16 * c["nLoop"], c["prec"])
    bad = pc.plan_matches(plan, c["expect"])
    assert not bad, (c["id"], bad, plan)
    return plan


def _run_case(hip, c, monkeypatch, record_max, seed, signs=(1, -1)):
    """Both FT signs of one case against the oracle; returns the GPU results."""
    _set_env(monkeypatch, c["env"])
    plan = _assert_class(hip, c)
    X, prec, nLoop = c["X"], c["prec"], c["nLoop"]
    tot, coord = pc.grid_of(c)
    mom = pc.momenta(c["pxs"])
    rng = np.random.default_rng(seed)
    nData, V = 16 * nLoop, int(np.prod(X))
    pos = _pos(rng, nData * V, prec)
    pos_d = torch.from_numpy(pos).cuda()
    res = []
    for FTSign in signs:
        out = torch.full((X[3] * nData * len(mom),), float("nan"), dtype=_tdt(prec), device="cuda")
        hip.convertAndProject(out, pos_d, nData, nLoop, mom, FTSign, X, tot, coord)
        got = out.cpu().numpy()
        err = rel_err(got, _oracle(pos, X, nLoop, mom, FTSign, tot, coord, prec))
        print("%s FTSign %+d form %s rel err %.3e" % (c["id"], FTSign, FORM_NAME[plan["form"]], err))
        record_max("projection_forms_%s_fp%d" % (FORM_NAME[plan["form"]], 8 * prec), err)
        assert err < TOL[prec], (c["id"], FTSign, err, plan)
        res.append(got)
    return res


# ---- (a) the ten matrix-pipe instantiations; the same shapes through the vector form and in fp32 --------------------------------
@pytest.mark.parametrize("triple", pc.MFMA_CASES, ids=lambda t: t[0]["id"])
def test_matrix_pipe_instantiations(hip, triple, monkeypatch, record_max):
    """<NKS, MB> for NKS = Lx / 8 in {3, 4, 6, 8} and MB = 2..4 blocks of 16 rows, with 1, 3, 7 or 8 distinct p_x (zero columns of the
    phase fragments, the j < nPx guard), rows padded to 16 and chunks of odd length.  The matrix-pipe and the vector result of
    the same fp64 input agree to rounding as well: the same sums in another order."""
    c_mfma, c_vec, c_f32 = triple
    seed = 100 + 10 * c_mfma["expect"]["nks"] + c_mfma["expect"]["mb"]
    a = _run_case(hip, c_mfma, monkeypatch, record_max, seed)
    b = _run_case(hip, c_vec, monkeypatch, record_max, seed)
    for x, y in zip(a, b):
        assert rel_err(x, y) < TOL[8]
    _run_case(hip, c_f32, monkeypatch, record_max, seed)


# ---- (b) the general kernel: ragged last chunk, runs longer than a wave, uneven x classes, several passes -----------------------
@pytest.mark.parametrize("c", pc.GENERAL_CASES + [pc.TWO_ROW_PASS_CASE], ids=lambda c: c["id"])
def test_general_kernel_shapes(hip, c, monkeypatch, record_max):
    _run_case(hip, c, monkeypatch, record_max, 211)


# ---- (c) several tiles per workgroup ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", pc.WALK_CASES, ids=lambda c: c["id"])
def test_forced_tile_walk(hip, c, monkeypatch, record_max):
    """MUGIQ_HIP_EO_TILES_PER_WG = 2, 3, 4 and all tiles: the prefetch of the next tile crosses y-pair and time-chunk boundaries,
    the last workgroup is ragged for 4.  The sums do not depend on the walk: bitwise equal to one tile per workgroup."""
    walked = _run_case(hip, c, monkeypatch, record_max, 307)
    one = dict(c, id=c["id"] + "-one", env=dict(c["env"], MUGIQ_HIP_EO_TILES_PER_WG="1"),
               expect=dict(c["expect"], tilesPerWg=1, workgroupsX=c["expect"]["tiles"]))
    single = _run_case(hip, one, monkeypatch, record_max, 307)
    for x, y in zip(walked, single):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("c", pc.NATURAL_WALK_CASES, ids=lambda c: c["id"])
def test_tile_walk_chosen_by_the_heuristic(hip, c, monkeypatch, record_max):
    """Lz * nData * tiles > 8192: the launcher itself walks two tiles per workgroup (the plan says so), no switch set."""
    assert "MUGIQ_HIP_EO_TILES_PER_WG" not in c["env"]
    walked = _run_case(hip, c, monkeypatch, record_max, 353, signs=(-1,))
    one = dict(c, id=c["id"] + "-one", env=dict(c["env"], MUGIQ_HIP_EO_TILES_PER_WG="1"),
               expect=dict(c["expect"], tilesPerWg=1, workgroupsX=c["expect"]["tiles"]))
    single = _run_case(hip, one, monkeypatch, record_max, 353, signs=(-1,))
    assert np.array_equal(walked[0], single[0])


# ---- (d) slot subsets ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", pc.SLOT_SETS, ids=lambda s: "slots" + "".join(map(str, s)))
@pytest.mark.parametrize("c", pc.SLOT_CASES, ids=lambda c: c["id"])
def test_slot_subsets(hip, c, slots, monkeypatch, record_max):
    """convertAndProjectSlots: the listed slots (unsorted lists too) get the rows of the full projection, every other row of the
    output keeps its bits."""
    _set_env(monkeypatch, c["env"])
    plan = _assert_class(hip, c, nData=16 * len(slots))
    X, prec, nLoop = c["X"], c["prec"], c["nLoop"]
    tot, coord = pc.grid_of(c)
    mom = pc.momenta(c["pxs"])
    rng = np.random.default_rng(401)
    nData, V, Lt = 16 * nLoop, int(np.prod(X)), X[3]
    pos = _pos(rng, nData * V, prec)
    exp = _oracle(pos, X, nLoop, mom, 1, tot, coord, prec).reshape(len(mom), nLoop, 16 * Lt)
    sentinel = _pos(rng, Lt * nData * len(mom), prec)
    out = torch.from_numpy(sentinel.copy()).cuda()
    hip.convertAndProjectSlots(out, torch.from_numpy(pos).cuda(), nLoop, slots, mom, 1, X, tot, coord)
    got = out.cpu().numpy().reshape(len(mom), nLoop, 16 * Lt)
    err = rel_err(got[:, slots], exp[:, slots])
    print("%s slots %s rel err %.3e" % (c["id"], slots, err))
    record_max("projection_forms_slots_%s_fp%d" % (FORM_NAME[plan["form"]], 8 * prec), err)
    assert err < TOL[prec], (c["id"], slots, err)
    rest = [s for s in range(nLoop) if s not in slots]
    assert not rest or np.array_equal(got[:, rest].view(np.uint8), sentinel.reshape(len(mom), nLoop, 16 * Lt)[:, rest].view(np.uint8))


# ---- (e) poisoned LDS ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", pc.POISON_CASES, ids=lambda c: c["id"])
def test_forms_with_poisoned_lds(hip, c, monkeypatch, record_max):
    """NaN patterns in the LDS of every CU before the call: padded rows, clamped load slots, the partial-sum area and the cells of
    a ragged chunk that no one wrote must not reach a result."""
    monkeypatch.setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")
    _run_case(hip, c, monkeypatch, record_max, 503, signs=(1,))


# ---- (f) seeded sweep ---------------------------------------------------------------------------------------------------------
_SWEEP_FORMS = {}
_N_SEEDS = int(os.environ.get("MUGIQ_TEST_SEEDS", 24))


@pytest.mark.parametrize("seed", range(_N_SEEDS))
def test_random_shapes_across_forms(hip, seed, monkeypatch, record_max):
    """Random Lx from 2 to 128, Lt up to 50, momentum lists with up to 13 distinct p_x, precision, FT sign, rank coordinate and
    loop count; the form each seed takes is recorded."""
    _set_env(monkeypatch, {})
    d = pc.sweep_draw(np, seed)
    X, prec, nLoop, mom = d["X"], d["prec"], d["nLoop"], d["mom"]
    nData, V = 16 * nLoop, int(np.prod(X))
    plan = hip.convertAndProjectPlan(mom, X, nData, prec)
    _SWEEP_FORMS[seed] = FORM_NAME[plan["form"]]
    pos = _pos(d["rng"], nData * V, prec)
    out = torch.full((X[3] * nData * len(mom),), float("nan"), dtype=_tdt(prec), device="cuda")
    hip.convertAndProject(out, torch.from_numpy(pos).cuda(), nData, nLoop, mom, d["FTSign"], X, d["tot"], d["coord"])
    err = rel_err(out.cpu().numpy(), _oracle(pos, X, nLoop, mom, d["FTSign"], d["tot"], d["coord"], prec))
    print("seed %d X %s fp%d nPx %d form %s rel err %.3e" % (seed, X, 8 * prec, plan["nPx"], FORM_NAME[plan["form"]], err))
    record_max("projection_forms_sweep_%s_fp%d" % (FORM_NAME[plan["form"]], 8 * prec), err)
    assert err < TOL[prec], (seed, X, prec, nLoop, len(mom), d["coord"], plan)


def test_random_shapes_reach_every_form(hip, monkeypatch):
    """How many seeds of the sweep fall in each form (printed); each form at least twice for the default seed count."""
    _set_env(monkeypatch, {})
    count = dict.fromkeys(FORM_NAME.values(), 0)
    for seed in range(_N_SEEDS):
        d = pc.sweep_draw(np, seed)
        form = FORM_NAME[hip.convertAndProjectPlan(d["mom"], d["X"], 16 * d["nLoop"], d["prec"])["form"]]
        assert _SWEEP_FORMS.get(seed, form) == form
        count[form] += 1
    print("seeds per form:", count)
    if _N_SEEDS >= 24:
        assert min(count.values()) >= 2, count


# ---- (g) dense product of the BASIC plan ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("M,K,N,nSplit", [(1040, 600, 13, 3),          # 4 rows per lane, ragged last row block, K % 64 != 0, N % 8 != 0
                                          (2048, 1024, 8, 4),          # exact fits
                                          (520, 320, 9, 2)])           # 2 rows per lane, ragged
def test_dense_projection_row_tiles_and_splits(hip, prec, M, K, N, nSplit, record_max):
    """momproj_partial_kernel<RT = 4 | 2> with K split over workgroups (the workspace size tells the number of splits)."""
    rng = np.random.default_rng(601)
    locT, nData = M // 8, 8
    assert locT * nData == M
    assert hip._lib.load().mugiq_hip_momentum_projection_workspace(locT, nData, K, N, prec) == nSplit * M * N * 2 * prec
    A = _pos(rng, M * K, prec)
    B = _pos(rng, K * N, prec)
    out = torch.full((M * N,), float("nan"), dtype=_tdt(prec), device="cuda")
    hip.momentumProjection(out, torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(), locT, nData, K, N)
    exp = orc.momentum_projection_local(A.astype(np.complex128), B.astype(np.complex128), locT, nData, K, N)
    err = rel_err(out.cpu().numpy(), exp)
    print("dense %d x %d x %d fp%d rel err %.3e" % (M, K, N, 8 * prec, err))
    record_max("projection_dense_fp%d" % (8 * prec), err)
    assert err < TOL[prec], (M, K, N, err)
