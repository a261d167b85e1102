"""GPU tests of the eigenvector pipelines of the two vector tiles (csrc/fused_tile.hip: 32 lines per workgroup; csrc/fused_tile16.hip:
16-line items; what they share is csrc/vector_tile.h): every kernel instance -- staging through registers with two eigenvectors
(fp64 storage) or three (fp32) in flight, or global -> LDS with three tile buffers; 4 or 8 staged positions per lane (32 lines), 2, 4 or
8 staging loads per lane (16 lines); column and row tiles; the ultra-local loop carried as a fourth slot -- with 1 .. 10 and 13
eigenvectors.  A register-staged pipeline of depth d enters its branch-free steady-state loop while n + 2 d < nVec (fp64: from 5
eigenvectors, fp32: from 7), the global -> LDS one while n + 4 < nVec (from 5); the guarded tail takes the rest.  The counts enter
every steady-state loop zero, one, two and (fp32, 13 eigenvectors) three times, each with every tail length.

Each case names the instance it is there for and asserts it on the host (hip.fusedForm) before anything runs, then goes through the
OPT driver with every entry computed from the eigenvectors (MUGIQ_HIP_REFLECT=0) on the vector tiles (MUGIQ_HIP_TILE_MFMA=0).  The
reference is the numpy oracle, accumulated one eigenvector at a time: all eleven counts cost one pass.  Bounds are the driver's: 1e-12
relative to the largest element for fp64 storage, 1e-5 for fp32 loops, and 2e-6 for fp32 storage with fp64 loops (the path links W_k
are products of fp32 links either way: test_driver_mixed_precision).  Ghost layers and interior / boundary launches have their own
tests (test_gpu_driver.py)."""
import functools

import numpy as np
import pytest

from util import orc, random_gauge_lex, random_spinor_lex, sigmas, rel_err

pytestmark = pytest.mark.gpu

NEVS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 13)
POISON_NEVS = (1, 7)                     # below and above every form's steady-state threshold, once more over poisoned LDS
TILE32, TILE16 = 3, 4                    # MUGIQ_HIP_FUSED_FAMILY_*
SWITCHES = ("FUSED_TILE", "TILE_MFMA", "TILE_COLS", "TILE_GLDS", "TILE_ORDER", "TILE16_TJ", "TILE16_GLDS", "CARRY_ULTRALOCAL", "REFLECT",
            "DEBUG_POISON_LDS")
Y, R, W = (4, 8, 4, 4), (8, 4, 4, 4), (24, 4, 4, 2)      # column tiles along y; whole x rows; x rows of 12 entries (three pieces per parity)
F64, F64_4, F32, F32_4, MIXED = (8, 2, 8), (8, 4, 8), (4, 2, 4), (4, 4, 4), (4, 2, 8)      # (storage precision, order, loop precision)


def t32(ph, glds, staged):
    """what hip.fusedForm reports of a 32-line entry's first launch (without the carried slot: 12 waves)"""
    return dict(family=TILE32, glds=glds, ph=ph, waves=12, tj=4, lines=32, staged=staged)


def t16(phl, glds, waves, tj, staged):
    return dict(family=TILE16, glds=glds, phl=phl, waves=waves, tj=tj, lines=16, staged=staged)


# (name, lattice, storage, switches, [(entry, expected form)], entry that carries the ultra-local loop or -1)
CASES = [
    ("t32_col_glds_12waves", Y, F64, {"TILE_COLS": "32", "CARRY_ULTRALOCAL": "0"}, [("+y:1,3", t32(4, 1, 7)), ("-y:1,2", t32(4, 1, 6))], -1),
    ("t32_col_glds_16waves_carry", Y, F64, {"TILE_COLS": "32"}, [("+y:1,3", t32(4, 1, 7))], 0),
    ("t32_col_regs_ph4_depth2_f2", Y, F64, {"TILE_COLS": "32", "TILE_GLDS": "0"}, [("+y:1,3", t32(4, 0, 7))], -1),
    ("t32_col_regs_ph4_depth2_f4", Y, F64_4, {"TILE_COLS": "32", "TILE_GLDS": "0"}, [("+y:1,3", t32(4, 0, 7))], -1),
    # (three lengths leave no room in a 12-wave form; two do: the second entry takes the ultra-local loop along as its third slot)
    ("t32_col_regs_ph4_depth3_f2", Y, F32, {"TILE_COLS": "32"}, [("+y:1,3", t32(4, 0, 7)), ("-y:1,2", t32(4, 0, 6))], 1),
    ("t32_col_regs_ph4_depth3_f4", Y, F32_4, {"TILE_COLS": "32"}, [("+y:1,3", t32(4, 0, 7)), ("-y:1,2", t32(4, 0, 6))], 1),
    ("t32_col_regs_ph4_depth3_mixed", Y, MIXED, {"TILE_COLS": "32"}, [("+y:1,3", t32(4, 0, 7)), ("-y:1,2", t32(4, 0, 6))], 1),
    # (fp32 storage only: two fp64 buffers of 16 padded positions are 192 KB, see test_no_fp64_form_stages_8_positions_per_lane)
    ("t32_col_regs_ph8_f32", Y, F32, {"TILE_COLS": "32"}, [("+y:5,6", t32(8, 0, 10))], 0),
    ("t32_row_f64", R, F64, {"TILE_COLS": "32"}, [("+x:1,3", t32(4, 0, 4)), ("-x:1,2", t32(4, 0, 4))], 1),
    ("t32_row_f32_f4", R, F32_4, {"TILE_COLS": "32"}, [("+x:1,3", t32(4, 0, 4)), ("-x:1,2", t32(4, 0, 4))], 1),
    ("t16_col_phl4_glds", Y, F64, {"TILE_COLS": "16"}, [("+y:1,3", t16(4, 1, 6, 4, 7))], -1),
    ("t16_col_phl4_regs_f64", Y, F64, {"TILE_COLS": "16", "TILE16_GLDS": "0"}, [("+y:1,3", t16(4, 0, 6, 4, 7))], -1),
    ("t16_col_phl4_regs_f32", Y, F32, {"TILE_COLS": "16"}, [("+y:1,3", t16(4, 0, 6, 4, 7))], -1),
    ("t16_col_phl8_f64", Y, F64, {"TILE_COLS": "16"}, [("+y:5,6", t16(8, 1, 6, 4, 10))], -1),
    ("t16_col_phl8_f32_f4", Y, F32_4, {"TILE_COLS": "16"}, [("+y:5,6", t16(8, 0, 6, 4, 10))], -1),
    ("t16_col_tj8", Y, F64, {"TILE_COLS": "16", "TILE16_TJ": "8"}, [("-y:1,3", t16(4, 1, 12, 8, 11))], -1),
    ("t16_row_phl2_phl4_f64", R, F64, {"TILE_COLS": "16"}, [("+x:1,3", t16(2, 1, 3, 0, 2)), ("-x:2", t16(4, 1, 2, 0, 2))], -1),
    ("t16_row_phl2_phl4_f32", R, F32, {"TILE_COLS": "16"}, [("+x:1,3", t16(2, 0, 3, 0, 2)), ("-x:2", t16(4, 0, 2, 0, 2))], -1),
    # default selection: 12-entry rows do not fill 32-line positions (32 % 12 != 0), so the 16-line row tile takes them
    ("t16_row_phl8_three_pieces", W, F64, {}, [("+x:2", t16(8, 1, 3, 0, 6)), ("+x:1,3", t16(2, 1, 9, 0, 6))], -1),
]


@functools.lru_cache(maxsize=None)
def _inputs(X, prec):
    """13 eigenvectors and the links of lattice X, rounded to the storage precision (logical, complex128)"""
    rng = np.random.default_rng(2024)
    cdt = np.complex128 if prec == 8 else np.complex64
    ev = [orc.lex_to_eo(random_spinor_lex(rng, X), X).astype(cdt).astype(np.complex128) for _ in range(max(NEVS))]
    Uo = orc.extended_gauge_from_global(random_gauge_lex(rng, X), (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0)).astype(cdt).astype(np.complex128)
    return ev, Uo


@functools.lru_cache(maxsize=None)
def _reference(X, prec, entry):
    """{nev: the oracle's slots of `entry` (None: the ultra-local loop) summed over the first nev eigenvectors}; one pass, shared and
    never written again"""
    ev, Uo = _inputs(X, prec)
    sg = sigmas(max(NEVS))
    sg = np.float32(sg).astype(np.float64) if prec == 4 else sg
    if entry is None:
        cprm = orc.LoopComputeParam(doNonLocal=False)
    else:
        _, s, a, b = orc.parse_disp_entry_string(entry)
        cprm = orc.LoopComputeParam(s, a, b)
    V = int(np.prod(X))
    lo = 0 if entry is None else 16 * V
    acc, out = None, {}
    for n in range(max(NEVS)):
        one = orc.compute_loop_position_space([ev[n]], [sg[n]], cprm, Uo, X)[lo:]
        acc = one if acc is None else acc + one
        if n + 1 in NEVS:
            out[n + 1] = acc.copy()
            out[n + 1].setflags(write=False)
    return out


def expected(case, nev):
    """the position-space buffer of the driver: the ultra-local loop, then the slots of every entry"""
    _, X, (prec, _, _), _, entries, _ = case
    return np.concatenate([_reference(X, prec, None)[nev]] + [_reference(X, prec, e)[nev] for e, _ in entries])


def set_switches(case, setenv, delenv, poison=False):
    for k in SWITCHES:
        delenv("MUGIQ_HIP_" + k)
    setenv("MUGIQ_HIP_REFLECT", "0")
    setenv("MUGIQ_HIP_TILE_MFMA", "0")
    for k, v in case[3].items():
        setenv("MUGIQ_HIP_" + k, v)
    if poison:
        setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")


def make_fields(hip, case):
    _, X, (prec, order, _), _, _, _ = case
    ev, Uo = _inputs(X, prec)
    return [hip.SpinorField(X, prec, order).set_logical(v) for v in ev], hip.GaugeField(X, (0, 0, 0, 0), prec).set_logical(Uo)


def assert_forms(hip, case, f0):
    """the kernel instance every entry of the case is there for, from the host's own selector under the case's switches"""
    name, _, (_, _, lprec), _, entries, _ = case
    for entry, want in entries:
        _, s, a, b = orc.parse_disp_entry_string(entry)
        form = hip.fusedForm(f0, "xyzt".index(s[0][1]), list(range(a[0], b[0] + 1)), loopPrecision=lprec)
        assert form["kernel"] == hip.ENTRY_KERNEL_VECTOR_TILE, (name, entry, form)
        assert {k: form[k] for k in want} == want, (name, entry, form)


def run_case(hip, case, f, U, nev):
    """the driver's position-space buffer of the first nev eigenvectors (numpy), after the checks of what ran"""
    name, _, (_, _, lprec), _, entries, carrier = case
    prm = hip.MugiqLoopParam(gauge=U, loopPrecision=lprec).set_displace_entry_string(";".join(e for e, _ in entries))
    loop = hip.Loop_Mugiq(prm, f[:nev], sigmas(max(NEVS))[:nev])
    loop.computeCoarseLoop()
    got = loop.dataPos_d.cpu().numpy()
    assert [loop.entryKernel(i) for i in range(len(entries))] == [hip.ENTRY_KERNEL_VECTOR_TILE] * len(entries), (name, nev)
    assert loop.ultraLocalCarrier() == carrier, (name, nev, loop.ultraLocalCarrier())
    loop.close()
    return got


@pytest.mark.parametrize("X", [Y, (4, 16, 4, 4), (8, 24, 8, 8)])
def test_no_fp64_form_stages_8_positions_per_lane(hip, X, monkeypatch):
    """More than 8 staged positions (4 + kmax > 8) put the 32-line tile on its PH = 8 instance.  Over fp64 storage its two buffers of
    16 padded positions x 12 x 32 complex numbers are 192 KB, more than a workgroup's LDS whatever the lattice: such an entry goes to
    the streaming kernel, and the pipeline of that instance runs over fp32 storage only (the case above)."""
    monkeypatch.setenv("MUGIQ_HIP_TILE_MFMA", "0")
    monkeypatch.setenv("MUGIQ_HIP_TILE_COLS", "32")
    for order in (2, 4):
        assert hip.fusedForm((X, 8, order), 1, [5, 6])["kernel"] == hip.ENTRY_KERNEL_STREAMING
        assert hip.fusedForm((X, 4, order), 1, [5, 6])["ph"] == 8


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_vector_tile_pipeline(hip, case, monkeypatch, record_max):
    name, _, (prec, _, lprec), _, _, _ = case
    set_switches(case, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    f, U = make_fields(hip, case)
    assert_forms(hip, case, f[0])
    tol = 1e-12 if prec == 8 else (1e-5 if lprec == 4 else 2e-6)
    tag = "vector_tile_pipeline_%s" % ("fp64" if prec == 8 else ("fp32" if lprec == 4 else "mixed"))
    errs = {}
    for nev in NEVS:
        errs[nev] = rel_err(run_case(hip, case, f, U, nev), expected(case, nev))
        record_max(tag, errs[nev])
    set_switches(case, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False), poison=True)
    for nev in POISON_NEVS:
        errs["poisoned LDS, %d" % nev] = rel_err(run_case(hip, case, f, U, nev), expected(case, nev))
        record_max(tag, errs["poisoned LDS, %d" % nev])
    print(name, {k: "%.2e" % e for k, e in errs.items()})
    assert all(e < tol for e in errs.values()), (name, errs)          # (NaN fails)
