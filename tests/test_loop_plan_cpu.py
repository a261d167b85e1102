"""CPU-only checks of mugiq_hip_loop_plan: the host function through which the loop driver decides, once per compute, what happens to
every displacement entry (reflected / step by step / fused, halo posted ahead or not, which links are built, which buffers the pool
reserves) and in which order.  No GPU is touched: the query takes descriptors and calls the planner the driver calls.  The expected
values follow from the rules of csrc/loop_plan.cpp and the byte formulas of csrc/internal.h, worked out by hand."""
import pytest

from util import momenta_p2_le

GiB = 1 << 30
REFLECTED, STEPWISE, FUSED = 0, 1, 2
K_REFLECTED, K_MFMA_COLUMN, K_MFMA_ROW, K_VECTOR_TILE, K_STREAMING, K_STEPWISE = range(6)      # MUGIQ_HIP_ENTRY_KERNEL_*
CFG2 = "+x:1,3;-x:1,3;+y:1,3;-y:1,3;+z:1,3;-z:1,3;+t:1,3;-t:1,3"
X_CFG2 = (48, 48, 24, 24)
HALO_CFG2 = 3 * 24 * 27648 * 16 * 400          # stop * 24 * faceCB * sizeof(complex double) * nEv = 12,740,198,400
GAUGE_ZT = 9 * 27 * 55296 * 16                 # 9 * (X[mu] + kmax) * (V / X[mu]) * 16 = 214,990,848
GAUGE_X = 9 * 51 * 27648 * 16                  # 203,046,912


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in ("HALO_AHEAD", "REFLECT", "REFLECT_MOM", "SELF_HALO_COPY", "HALO_BLOCKS", "CARRY_ULTRALOCAL", "TILE_MFMA", "FUSED_TILE",
              "TILE_COLS", "TILE_GLDS", "MFMA_STORAGE", "MFMA_ROW", "MFMA_ROW_WAVES", "PACK_IN_ENTRY", "GAUGE_FROM_LINKS", "MFMA_TJ",
              "TILE16_TJ"):
        monkeypatch.delenv("MUGIQ_HIP_" + k, raising=False)


def _plan(hip, entries, X, nEv, grid=None, partitioned=(0, 0, 0, 0), R=(0, 0, 0, 0), deviceBytes=288 * GiB, axialOk=(1, 1, 1, 1),
          twoSided=False, calcType=None, prec=8, order=2):
    moms = momenta_p2_le(2)
    prm = hip.MugiqLoopParam(Nmom=len(moms), momMatrix=[list(m) for m in moms], FTSign=-1, doMomProj=True,
                             calcType=hip.LOOP_CALC_TYPE_OPT_KERNEL if calcType is None else calcType).set_displace_entry_string(entries)
    comm = {"grid": grid, "partitioned": partitioned, "group": True} if grid is not None else None
    return hip.loopPlan(prm, (X, prec, order), nEv, comm=comm, twoSided=twoSided, axialOk=axialOk, deviceBytes=deviceBytes, gauge=(prec, R))


def _cfg2(hip, **kw):
    return _plan(hip, CFG2, X_CFG2, 400, grid=(1, 1, 2, 4), R=(0, 0, 2, 2), **kw)


def _reserve_of(p, X, prec=8):
    """The reservation rule restated over the per-entry results: per posted entry its link fields with two face buffers, one ghost
    buffer (two unless the rank is its own neighbour) and its gauge; then the links of the early entry."""
    fieldB = 24 * (X[0] * X[1] * X[2] * X[3] // 2) * 2 * prec
    out = []
    for e in p["entries"]:
        if e["ahead"]:
            out += [fieldB] * e["nLinkFields"] + ([e["faceBytes"]] * 2 if e["nLinkFields"] else [])
            out += [e["haloBytes"]] * (1 if e["selfAlias"] else 2) + ([e["gaugeBytes"]] if e["gaugeBytes"] else [])
    if p["earlyEntry"] >= 0:
        e = p["entries"][p["earlyEntry"]]
        out += [e["gaugeBytes"]] if e["gaugeFromField"] else [fieldB] * (e["kv"][-1] + 1)
    return out


def test_configs2_as_one_gpu_sees_it(hip):
    p = _cfg2(hip)
    E = p["entries"]
    assert [e["derivedFrom"] for e in E] == [-1, 0, -1, 2, -1, 4, -1, 6]
    assert [e["route"] for e in E] == [FUSED, REFLECTED] * 4
    # X0 = 48: rows of 24 entries, 2 per 8-wave workgroup; 8 | 48 and 8 | 24: the 8 x 16 column tile (8 + 3 <= 16 positions)
    assert [e["kernel"] for e in E] == [K_MFMA_ROW, K_REFLECTED] + [K_MFMA_COLUMN, K_REFLECTED] * 3
    assert [i for i, e in enumerate(E) if e["ahead"]] == [4, 6]
    for i in (4, 6):
        assert E[i]["haloBytes"] == HALO_CFG2 == 12740198400 and E[i]["perVecHaloBytes"] * 400 == HALO_CFG2
        assert E[i]["selfAlias"] == 0 and E[i]["gaugeFromField"] == 1 and E[i]["nLinkFields"] == 0      # 3 <= R + 1
        assert E[i]["gaugeBytes"] == GAUGE_ZT == 214990848 and E[i]["tile"] == 1 and E[i]["part"] == 1
        assert E[i]["nBlocks"] == 6 and E[i]["blockN"] == 67                                             # ceil(12.74e9 / 2 GiB) = 6
        assert E[i]["kv"] == [1, 2, 3] and E[i]["high"] == 0 and E[i]["needsMemset"] == 0
    assert p["earlyEntry"] == 0 and p["order"] == [0, 2, 4, 6, 1, 3, 5, 7, -1]
    assert p["momReflect"] == 1 and p["carryUltra"] == 1 and p["grouped"] == 1
    # the row tile takes X0 = 48 (profiles/), so the early entry's gauge comes straight from the gauge field
    assert p["reserve"] == [HALO_CFG2, HALO_CFG2, GAUGE_ZT] * 2 + [GAUGE_X]
    assert GAUGE_X == 203046912 and p["reserve"] == _reserve_of(p, X_CFG2)


def test_halo_budget_is_a_quarter_of_the_device(hip, monkeypatch):
    """2 * haloBytes = 25,480,396,800 per entry, charged in entry order against total / 4."""
    p = _cfg2(hip, deviceBytes=128 * GiB)                # 34,359,738,368: one entry fits
    assert [i for i, e in enumerate(p["entries"]) if e["ahead"]] == [4]
    assert p["entries"][6]["nLinkFields"] == 4 and p["entries"][6]["gaugeFromField"] == 0      # not posted: its links as fields
    assert p["reserve"] == [HALO_CFG2, HALO_CFG2, GAUGE_ZT, GAUGE_X]
    p = _cfg2(hip, deviceBytes=64 * GiB)                 # 17,179,869,184: none
    assert not any(e["ahead"] for e in p["entries"]) and p["earlyEntry"] == -2 and p["reserve"] == []
    assert p["order"] == [0, 2, 4, 6, 1, 3, 5, 7, -1]
    monkeypatch.setenv("MUGIQ_HIP_HALO_AHEAD", "0")
    p = _cfg2(hip)
    assert not any(e["ahead"] for e in p["entries"]) and p["earlyEntry"] == -2 and p["reserve"] == []


def test_own_neighbour_needs_one_halo_buffer(hip, monkeypatch):
    X, ent = (4, 4, 8, 8), "+x:1,3;+t:1,2;-z:1,2;+y:2;-t:2"       # the "pool_tie" entries of tests/mp_workers.py
    lens = []
    for copy, alias in ((None, 1), ("1", 0)):
        if copy:
            monkeypatch.setenv("MUGIQ_HIP_SELF_HALO_COPY", copy)
        p = _plan(hip, ent, X, 4, grid=(1, 1, 1, 1), partitioned=(0, 0, 1, 1), R=(0, 0, 2, 2))
        E = p["entries"]
        assert [e["derivedFrom"] for e in E] == [-1, -1, -1, -1, 1] and [i for i, e in enumerate(E) if e["ahead"]] == [1, 2]
        assert all(E[i]["selfAlias"] == alias and E[i]["nBlocks"] == 1 for i in (1, 2))
        assert E[1]["haloBytes"] == E[2]["haloBytes"] == 2 * 24 * 64 * 16 * 4 == 24 * 512 * 16          # as large as a link field
        assert p["reserve"] == _reserve_of(p, X)
        assert p["earlyEntry"] == 0 and E[0]["high"] == 0 and E[2]["high"] == 1
        # X0 = 4: rows of 2 entries, no matrix-pipe row tile (2 % 4), 16 rows fill a 32-line position; 8 | 8 along z, t; "+y:2" on
        # Y = 4 takes the 4 x 32 tile (4 + 2 <= 8) with the driver's gauge
        assert [e["kernel"] for e in E] == [K_VECTOR_TILE, K_MFMA_COLUMN, K_MFMA_COLUMN, K_MFMA_COLUMN, K_REFLECTED]
        lens.append(len(p["reserve"]))
    assert lens[1] == lens[0] + 2                                   # one more buffer for each of the two posted entries


def test_minus_entry_past_the_border_builds_link_fields(hip):
    X, nEv = (8, 8, 8, 8), 4
    p = _plan(hip, "-z:1,3", X, nEv, grid=(1, 1, 2, 1), R=(0, 0, 2, 0))
    e = p["entries"][0]
    assert e["ahead"] == 1 and e["gaugeFromField"] == 0 and e["nLinkFields"] == 4 and e["high"] == 1        # 3 > R
    face, field, halo = 24 * 256 * 16, 24 * 2048 * 16, 3 * 24 * 256 * 16 * nEv
    assert (e["faceBytes"], e["haloBytes"]) == (face, halo)
    assert p["reserve"][:8] == [field] * 4 + [face, face, halo, halo]
    assert p["reserve"][8:] == ([e["gaugeBytes"]] if e["gaugeBytes"] else []) and e["buildGaugeFromLinks"] == (1 if e["gaugeBytes"] else 0)
    q = _plan(hip, "+z:1,3", X, nEv, grid=(1, 1, 2, 1), R=(0, 0, 2, 0))["entries"][0]                       # "+": 3 <= R + 1
    assert q["nLinkFields"] == (0 if q["gaugeBytes"] else 4) and q["gaugeFromField"] == (1 if q["gaugeBytes"] else 0)


def test_past_the_neighbour_goes_step_by_step(hip):
    p = _plan(hip, "+t:1,5;-t:1,5", (4, 4, 4, 4), 3, grid=(1, 1, 1, 4), R=(0, 0, 0, 2))
    for e in p["entries"]:
        assert (e["route"], e["derivedFrom"], e["ahead"], e["needsMemset"], e["nLinkFields"]) == (STEPWISE, -1, 0, 1, 0)
        assert e["kernel"] == K_STEPWISE
    assert p["order"] == [0, 1, -1] and p["reserve"] == [] and p["momReflect"] == 0


def test_tile_refused_along_z(hip):
    p = _cfg2(hip, axialOk=(1, 1, 0, 1))
    E = p["entries"]
    assert all((E[i]["tile"], E[i]["gaugeBytes"]) == (0, 0) for i in (4, 5)) and E[4]["nLinkFields"] == 4
    assert E[4]["route"] == FUSED and E[4]["ahead"] == 1 and E[6]["gaugeFromField"] == 1
    assert [e["kernel"] for e in E] == [K_MFMA_ROW, K_REFLECTED, K_MFMA_COLUMN, K_REFLECTED, K_VECTOR_TILE, K_REFLECTED, K_MFMA_COLUMN, K_REFLECTED]
    assert p["reserve"] == [24 * 663552 * 16] * 4 + [24 * 27648 * 16] * 2 + [HALO_CFG2] * 2 + [HALO_CFG2, HALO_CFG2, GAUGE_ZT, GAUGE_X]
    p = _cfg2(hip, axialOk=(1, 1, 0, 1), twoSided=True)
    E = p["entries"]
    assert all(e["derivedFrom"] == -1 for e in E) and p["momReflect"] == 0
    assert [E[i]["route"] for i in (4, 5)] == [STEPWISE, STEPWISE] and all(E[i]["needsMemset"] and not E[i]["ahead"] for i in (4, 5))
    assert [e["kernel"] for e in E] == [K_MFMA_ROW] * 2 + [K_MFMA_COLUMN] * 2 + [K_STEPWISE] * 2 + [K_MFMA_COLUMN] * 2


def test_two_sided_length_nine_goes_step_by_step(hip):
    p = _plan(hip, "+z:1,9", (8, 8, 16, 8), 4, twoSided=True)
    assert p["entries"][0]["route"] == STEPWISE and p["entries"][0]["needsMemset"] == 1 and p["entries"][0]["kernel"] == K_STEPWISE
    e = _plan(hip, "+z:1,8", (8, 8, 16, 8), 4, twoSided=True)["entries"][0]
    assert e["route"] == FUSED and e["kernel"] == K_MFMA_COLUMN                                # 8 | 16, 8 + 8 <= 16 positions


def test_basic_keeps_the_reference_order(hip):
    p = _cfg2(hip, calcType=hip.LOOP_CALC_TYPE_BASIC_KERNEL)
    assert p["order"] == [-1, 0, 1, 2, 3, 4, 5, 6, 7] and p["earlyEntry"] == -2 and p["reserve"] == []
    assert all((e["derivedFrom"], e["ahead"], e["needsMemset"], e["route"], e["kernel"]) == (-1, 0, 1, STEPWISE, K_STEPWISE) for e in p["entries"])
    assert (p["carryUltra"], p["momReflect"], p["grouped"]) == (0, 0, 0)


def test_pack_targets_of_the_early_entry(hip, monkeypatch):
    """A mu = x entry first on the row tile, z / t partitioned with the rank as its own neighbour: it writes the face layers of every
    posted halo from eigenvector 0 on; a halo that travels in one block is left to its pack kernel."""
    ent = "+x:1,2;+t:1,3;-z:1,2;+z:2,3;-t:2,4;+y:1"                # the "pack" entries of tests/mp_workers.py
    kw = dict(grid=(1, 1, 1, 1), partitioned=(0, 0, 1, 1), R=(0, 0, 2, 2))
    p = _plan(hip, ent, (8, 16, 8, 8), 4, **kw)
    assert p["earlyEntry"] == 0 and p["entryPacksFrom"] == [1, 2, 3, 4] and all(p["entries"][i]["entryPacksFrom"] == 0 for i in (1, 2, 3, 4))
    assert [e["kernel"] for e in p["entries"]] == [K_MFMA_ROW] + [K_MFMA_COLUMN] * 5     # X0 = 8: 8 rows of 4 entries per 8-wave workgroup
    monkeypatch.setenv("MUGIQ_HIP_SELF_HALO_COPY", "1")            # one block per halo: from = blockN = nEv
    p = _plan(hip, ent, (8, 16, 8, 8), 4, **kw)
    assert p["entryPacksFrom"] == [] and all(e["entryPacksFrom"] == -1 for e in p["entries"])
    monkeypatch.setenv("MUGIQ_HIP_HALO_BLOCKS", "3")               # blocks of 2: the first goes out ahead
    p = _plan(hip, ent, (8, 16, 8, 8), 4, **kw)
    assert p["entryPacksFrom"] == [1, 2, 3, 4] and all(p["entries"][i]["entryPacksFrom"] == 2 for i in (1, 2, 3, 4))


def test_query_rejects_what_it_cannot_report(hip):
    with pytest.raises(hip.MugiqHipError):
        _plan(hip, ";".join(["+x:1"] * 65), (8, 8, 8, 8), 2)
    with pytest.raises(hip.MugiqHipError):
        _plan(hip, "+q:1", (8, 8, 8, 8), 2)
