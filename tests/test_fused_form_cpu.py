"""CPU-only checks of mugiq_hip_fused_form: the host query of the one selector (csrc/fused_form.cpp) through which the fused calls and the
loop driver's plan choose the kernel form of a displaced entry.  No GPU is touched.  The expected values were worked out by hand from
the admission rules (the matrix-pipe tile's geometries, the 32- and 16-line vector tiles' LDS bounds, the switches' vetoes)."""
import glob
import os

import pytest

import two_sided_workers as w

NONE, MFMA_COLUMN, MFMA_ROW, TILE32, TILE16, STREAMING = range(6)        # MUGIQ_HIP_FUSED_FAMILY_*
SWITCHES = ("FUSED_TILE", "FUSED_TUNE", "TILE_MFMA", "TILE_COLS", "TILE_GLDS", "TILE_ORDER", "TILE16_TJ", "TILE16_GLDS", "MFMA_TJ", "MFMA_ROW",
            "MFMA_ROW_WAVES", "MFMA_STORAGE", "PACK_IN_ENTRY", "GAUGE_FROM_LINKS")
A, B, C, D = (48, 48, 24, 24), (16, 16, 16, 16), (8, 8, 8, 8), (12, 6, 6, 6)
F64, F32 = (8, 2), (4, 4)                                                # fp64 FLOAT2, fp32 FLOAT4


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv("MUGIQ_HIP_" + k, raising=False)


def _two_sided_entries():
    """(case, direction, lengths, predicted kind) of the random two-sided table, with the seeds of test_two_sided_cpu.py"""
    for seed in range(w.DEFAULT_SEEDS):
        c = w.random_two_sided_case(5000 + seed)
        for e, (kind, _) in zip(c["entry"].split(";"), w.predicted_entry_kernels(c)):
            sd, lims = e.split(":")
            ab = [int(t) for t in lims.split(",")]
            yield c, "xyzt".index(sd[1]), list(range(min(ab), max(ab) + 1)), kind


def test_two_sided_table_against_the_python_predictor(hip):
    n = {"MFMA_ROW": 0, "MFMA_COLUMN": 0, "STEPWISE": 0}
    for c, d, kv, kind in _two_sided_entries():
        f = hip.fusedForm((c["X"], c["prec"], c["order"], c["pad"]), d, kv, twoSided=True, loopPrecision=c["lprec"])
        assert f["kernel"] == getattr(hip, "ENTRY_KERNEL_" + kind), (c, d, kv, f)
        n[kind] += 1
        if kind == "MFMA_ROW":
            assert (f["family"], (f["rowGroups"], f["rows"], f["waves"])) == (MFMA_ROW, w.mfma_row_geometry(c["X"], c["prec"], c["order"])), (c, f)
        elif kind == "MFMA_COLUMN":
            assert (f["family"], f["tj"]) == (MFMA_COLUMN, w.mfma_tile_tj(c["X"][d], kv[-1], w._reduced(c["prec"], c["order"]))), (c, d, kv, f)
        else:
            assert f["family"] == NONE and f["slotsPerLaunch"] == 0
        _admission_equals_launch(f)
    assert all(n.values()), n                                            # (the table reaches every kind)


# ---- one-sided: the family of every direction's entry, lengths 1 .. 3 (1 .. 8 under MFMA_TJ=4), unpartitioned, by lattice and storage.
# Matrix-pipe row tile: X0/2 a multiple of 4 and R = 2 G W / (X0/2) whole rows (G = 3 | 2 groups, W = 8 waves) dividing the row count
#   with R (X0/2 + 4) <= 8 W: A (24 entries: R = 2, G = 3), B (8: R = 4, G = 2), C (4: R = 8, G = 2); D has rows of 6 entries: none.
# Matrix-pipe column tile: 8 | extent with 8 + 3 <= 16: A, B, C; extent 6 (D): no TJ of 8, 12, 4 divides it.
# 32-line row tile: 32 / (X0/2) rows per group, twice that dividing the row count: A (1), B (4), C (8); D: 216 rows % 10.
# 16-line row tile: lcm(16, X0/2) / 16 pieces per parity: D m = 3 (1296 % 48 = 0); by default only where 32 % (X0/2) != 0: A (24), D (6).
# Vector column tiles want 4 | extent: never D.
_MFMA = [MFMA_ROW] + [MFMA_COLUMN] * 3
_D_NO_MFMA = [TILE16] + [STREAMING] * 3
ONE_SIDED = {
    None: {A: _MFMA, B: _MFMA, C: _MFMA, D: _D_NO_MFMA},
    # the x entry on X0 = 48 takes the 16-line tile (32 % 24 != 0); the column entries the 32-line tile
    ("TILE_MFMA", "0"): {A: [TILE16] + [TILE32] * 3, B: [TILE32] * 4, C: [TILE32] * 4, D: _D_NO_MFMA},
    ("TILE_GLDS", "0"): {A: [TILE16] + [TILE32] * 3, B: [TILE32] * 4, C: [TILE32] * 4, D: _D_NO_MFMA},   # ... and no matrix-pipe tile
    ("TILE_COLS", "16"): {A: [TILE16] * 4, B: [TILE16] * 4, C: [TILE16] * 4, D: _D_NO_MFMA},
    ("TILE_COLS", "32"): {A: [TILE32] * 4, B: [TILE32] * 4, C: [TILE32] * 4, D: [STREAMING] * 4},
    ("FUSED_TILE", "0"): {X: [STREAMING] * 4 for X in (A, B, C, D)},
    # no vector ROW tile; the matrix-pipe row tile is not affected
    ("FUSED_TILE", "2"): {A: _MFMA, B: _MFMA, C: _MFMA, D: [STREAMING] * 4},
}
# MFMA_TJ=4 with lengths 1 .. 8: 4 + 8 > 8 positions, no column tile (fp32 FLOAT4 has no 4 x 32 tile at all); the row tile stays.
# 12 staged positions: the 32-line tile needs 2 x 96 KiB in fp64 (refused: the 16-line tile, 2 x 48 KiB) and 2 x 48 KiB in fp32 (taken).
# D: lengths up to 8 pass the extent 6 of y, z, t (streaming); 8 < X0 = 12 keeps the 16-line row tile.
MFMA_TJ4 = {F64: {A: [MFMA_ROW] + [TILE16] * 3, B: [MFMA_ROW] + [TILE16] * 3, C: [MFMA_ROW] + [TILE16] * 3, D: _D_NO_MFMA},
            F32: {A: [MFMA_ROW] + [TILE32] * 3, B: [MFMA_ROW] + [TILE32] * 3, C: [MFMA_ROW] + [TILE32] * 3, D: _D_NO_MFMA}}
KERNEL_OF = {MFMA_COLUMN: 1, MFMA_ROW: 2, TILE32: 3, TILE16: 3, STREAMING: 4}     # MUGIQ_HIP_ENTRY_KERNEL_*


def _admission_equals_launch(f):
    """what admitted the entry is what the first launch takes: it fits the LDS of a workgroup, and stages what its geometry says"""
    if f["family"] in (MFMA_COLUMN, MFMA_ROW, TILE32, TILE16):
        assert 0 < f["ldsBytes"] <= 160 * 1024, f
    if f["family"] == MFMA_COLUMN or (f["family"] in (TILE32, TILE16) and f["m"] == 0 and f["tj"] and f["staged"] != f["tj"]):
        assert f["staged"] == f["tj"] + f["kmax"], f
    if f["family"] == TILE16 and f["m"]:
        assert f["staged"] == 2 * f["m"] == f["np"], f


@pytest.mark.parametrize("storage", [F64, F32])
@pytest.mark.parametrize("switch", list(ONE_SIDED) + [("MFMA_TJ", "4")])
def test_one_sided_table(hip, monkeypatch, switch, storage):
    if switch:
        monkeypatch.setenv("MUGIQ_HIP_" + switch[0], switch[1])
    table = MFMA_TJ4[storage] if switch == ("MFMA_TJ", "4") else ONE_SIDED[switch]
    kv = list(range(1, 9 if switch == ("MFMA_TJ", "4") else 4))
    for X, want in table.items():
        for d in range(4):
            f = hip.fusedForm((X,) + storage, d, kv)
            assert (f["family"], f["kernel"]) == (want[d], KERNEL_OF[want[d]]), (X, storage, d, switch, f)
            assert 1 <= f["nSlots"] <= f["slotsPerLaunch"] and f["kmax"] == f["nSlots"]          # the shortest lengths go first
            _admission_equals_launch(f)


def test_one_sided_geometry_examples(hip, monkeypatch):
    f = hip.fusedForm((A,) + F64, 0, [1, 2, 3])
    assert (f["rowGroups"], f["rows"], f["waves"], f["rowChunk"], f["slotsPerLaunch"], f["packCapacity"]) == (3, 2, 8, 68, 3, 4)
    assert f["gaugeBytes"] == 9 * 51 * 27648 * 16
    f = hip.fusedForm((A,) + F64, 2, [1, 2, 3])                          # three slots, not partitioned: 12 | 24, 12 + 3 <= 16
    assert (f["tj"], f["lines"], f["staged"], f["waves"], f["ldsBytes"]) == (12, 16, 15, 16, 2 * 48 * 68 * 16)
    assert hip.fusedForm((A,) + F64, 2, [1, 2, 3], partitioned=True)["tj"] == 8
    monkeypatch.setenv("MUGIQ_HIP_TILE_MFMA", "0")
    f = hip.fusedForm((A,) + F64, 1, [1, 2, 3])                          # 4 + 3 positions: pairs of 4, staged global -> LDS, 3 buffers
    assert (f["family"], f["glds"], f["ph"], f["staged"], f["ldsBytes"]) == (TILE32, 1, 4, 7, 3 * 16 * 8 * 12 * 32)
    f = hip.fusedForm((A,) + F64, 0, [1, 2, 3])                          # 2 rows = 3 pieces per parity: 6 positions x 3 slots on 9 waves
    assert (f["family"], f["m"], f["npc"], f["np"], f["waves"], f["phl"]) == (TILE16, 3, 6, 6, 9, 2)
    monkeypatch.delenv("MUGIQ_HIP_TILE_MFMA")
    monkeypatch.setenv("MUGIQ_HIP_TILE_GLDS", "0")
    f = hip.fusedForm((A,) + F64, 1, [1, 2, 3])                          # through registers: 2 buffers; and no matrix-pipe tile
    assert (f["family"], f["glds"], f["ldsBytes"]) == (TILE32, 0, 2 * 16 * 8 * 12 * 32)


def test_query_rejects_bad_arguments(hip):
    with pytest.raises(hip.MugiqHipError):
        hip.fusedForm((C,) + F64, 4, [1])
    with pytest.raises(hip.MugiqHipError):
        hip.fusedForm((C,) + F64, 0, [])


def test_switches_are_read_in_one_place():
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mugiq_amd", "csrc")
    files = glob.glob(os.path.join(src, "fused*.hip")) + [os.path.join(src, "fused_mfma_kernel.h")]
    assert len(files) >= 12
    for path in files:
        with open(path) as f:
            assert f.read().count("getenv") == 0, path
