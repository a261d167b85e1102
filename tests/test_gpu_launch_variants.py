"""GPU parity tests of the launch variants the MUGIQ_HIP_* tuning switches select, against the CPU oracle.

  A  MUGIQ_HIP_CONTRACT_TUNE = "block,depth,nt,swz": every variant of loop_contract_kernel (csrc/contract.hip), every storage type
  B  MUGIQ_HIP_FUSED_TUNE = "nt,swz,remap": the streaming displaced kernel (csrc/fused.hip), XCD order and displacement-aligned order
  C  MUGIQ_HIP_TILE_ORDER = 0..3, MUGIQ_HIP_TILE16_TJ = 8, MUGIQ_HIP_TILE16_GLDS = 0: the workgroup -> tile maps of the tile kernels

The variants loop inside a test over one set of uploaded fields and one uploaded reference, and are compared on the device.  Every case
asserts the branch it is there for (swizzle a non-trivial map, remap on / off, nblocks mod 8) from tests/launch_variants.py, the host
restatement of the launch arithmetic that test_launch_variants_cpu.py checks, and prints it; a variant whose bits differ from the
default's is recorded through record_max as 0 / 1 (not asserted: FMA contraction may differ between instantiations of a kernel).
"""
import functools

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import launch_variant_workers
import launch_variants as lv
from fused_cases import fused_two_domains_along_t, path_links
from test_multi_rank_cpu import free_port
from util import orc, random_gauge_lex, random_spinor_lex, sigmas

pytestmark = pytest.mark.gpu

# (name, field precision, field order, loop precision): the four storage types and the mixed mode (fp32 fields, complex128 loops)
STORAGES = [("fp64_o2", 8, 2, 8), ("fp64_o4", 8, 4, 8), ("fp32_o2", 4, 2, 4), ("fp32_o4", 4, 4, 4), ("mixed_o2", 4, 2, 8), ("mixed_o4", 4, 4, 8)]
# fp64: TOL of test_gpu_operators.py; fp32: the same; mixed: test_mixed_precision_contraction_fp32_storage_fp64_accumulation
CONTRACT_TOL = {(8, 8): 1e-12, (4, 4): 1e-5, (4, 8): 1e-13}


def _np_c(prec):
    return np.complex128 if prec == 8 else np.complex64


def _t_c(prec):
    return torch.complex128 if prec == 8 else torch.complex64


def _frozen(a):
    a.setflags(write=False)
    return a


def _dev(a):
    """a (shared, read-only) host array on the device"""
    return torch.tensor(a, device="cuda")


def _field(hip, v, X, prec, order, pad=0):
    """set_logical, but the pad (stride > volumeCB) is filled with NaN: a kernel that reads it shows it"""
    f = hip.SpinorField(X, prec, order, pad=pad)
    if pad:
        buf = np.full(2 * f.parity_offset, np.nan + 1j * np.nan, dtype=_np_c(prec))
        buf[f._index_table()] = v.astype(buf.dtype)
        f.data.copy_(torch.from_numpy(buf))
        return f
    return f.set_logical(v.astype(_np_c(prec)))


# ---- A: loop_contract_kernel ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _contract_vectors(X):
    rng = np.random.default_rng(20240 + int(np.prod(X)))
    evL = [_frozen(orc.lex_to_eo(random_spinor_lex(rng, X), X)) for _ in range(lv.CONTRACT_NVEC_MAX)]
    evR = [_frozen(orc.lex_to_eo(random_spinor_lex(rng, X), X)) for _ in range(lv.CONTRACT_NVEC_MAX)]
    V = int(np.prod(X))
    init = _frozen(rng.standard_normal(16 * V) + 1j * rng.standard_normal(16 * V))               # (scaled to the loop's size by the test)
    return evL, evR, init


@functools.lru_cache(maxsize=None)
def _contract_reference(X, prec):
    """Running sums of orc.loop_contract over the inputs rounded to the storage precision (and the fp32-rounded sigma for fp32 storage,
    as test_random_geometry_contraction_and_prolongator): {same: [nVec = 1 .. 13][16 V]}, computed once per (shape, precision)."""
    evL, evR, _ = _contract_vectors(X)
    V = int(np.prod(X))
    sg = sigmas(lv.CONTRACT_NVEC_MAX)
    rnd = lambda v: v.astype(_np_c(prec)).astype(np.complex128)
    out = {}
    for same in (True, False):
        acc = np.zeros(16 * V, dtype=np.complex128)
        rows = []
        for n in range(lv.CONTRACT_NVEC_MAX):
            orc.loop_contract(acc, rnd(evL[n]), rnd(evL[n] if same else evR[n]), float(np.float32(sg[n])) if prec == 4 else sg[n])
            rows.append(acc.copy())
        out[same] = _frozen(np.stack(rows))
    return out


def _setenv(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


CONTRACT_CASES = [(X, st, 0) for X in lv.CONTRACT_SHAPES for st in STORAGES] + \
                 [((8, 8, 4, 4), STORAGES[0], 18), ((6, 6, 6, 6), STORAGES[5], 18)]          # padded stride, the pad filled with NaN


def _case_id(v):
    if isinstance(v, int):
        return "pad%d" % v
    return v[0] if isinstance(v[0], str) else "x".join(map(str, v))


@pytest.mark.parametrize("X,storage,pad", CONTRACT_CASES, ids=_case_id)
def test_contraction_every_tune_variant_matches_the_oracle(hip, record_max, monkeypatch, X, storage, pad):
    """loop_contract_kernel under MUGIQ_HIP_CONTRACT_TUNE unset, all 48 "block,depth,nt,swz", the three-field form and four rejected
    strings; L == R and L != R (depth 3 runs as 2 there); nVec = 1 .. 13 in one call each (0 .. 3 trips of the unguarded steady-state
    loop of the prefetch ring at depth 3 and every residue of its guarded tail; V = 8192 and V = 1296: nVec 1, 5, 13), one nVec on top
    of a non-zero loop buffer.  Shapes: (8,8,8,16) 16 workgroups of 512 (the XCD swizzle is not the identity), (8,8,4,4) swizzle on
    for 64 and 128 only, (8,4,4,4) for 64 only, (6,6,6,6) ragged last workgroup at every block size, (4,4,4,4) half a workgroup of 512.
    The mixed mode always launches 256: its swizzle must be decided from that (sites 256 .. V-1 stayed unwritten for
    "64,*,*,1" / "128,*,*,1" at V = 1024 and "64,*,*,1" at V = 512 when it was decided from the block size asked for)."""
    name, prec, order, lprec = storage
    V = int(np.prod(X))
    nvs = lv.CONTRACT_SHAPES[X] or tuple(range(1, lv.CONTRACT_NVEC_MAX + 1))
    on_top = nvs[len(nvs) // 2]                                          # this nVec accumulates on top of a non-zero buffer
    evL, evR, init = _contract_vectors(X)
    refs = _contract_reference(X, prec)
    sg = sigmas(lv.CONTRACT_NVEC_MAX)
    fL = [_field(hip, v, X, prec, order, pad) for v in evL]
    fR = [_field(hip, v, X, prec, order, pad) for v in evR]
    tol = CONTRACT_TOL[(prec, lprec)]
    mixed, fp64 = prec != lprec, prec == 8
    envs = [None] + lv.CONTRACT_VARIANTS + [lv.CONTRACT_THREE_FIELDS] + lv.CONTRACT_REJECTED
    nontrivial = 0
    for same in (True, False):
        ref_d = _dev(refs[same][[n - 1 for n in nvs]])
        # the seeded non-zero buffer one nVec starts from: of the size of that loop, rounded to the precision of the loop buffer
        init_d = (_dev(init) * float(np.abs(refs[same][on_top - 1]).max())).to(_t_c(lprec))
        ref_d[nvs.index(on_top)] += init_d.to(torch.complex128)
        scale = ref_d.abs().amax(dim=1)
        errs = torch.zeros(len(envs), len(nvs), dtype=torch.float64, device="cuda")
        differs = torch.zeros(len(envs), len(nvs), dtype=torch.bool, device="cuda")
        results = {}
        for ie, env in enumerate(envs):
            _setenv(monkeypatch, "MUGIQ_HIP_CONTRACT_TUNE", env)
            block, swz, sites = lv.contract_map(V, env, same, fp64 and not mixed, mixed)
            assert lv.is_bijection(sites, V)
            nontrivial += int(swz and not np.array_equal(sites, np.arange(V)))
            for i, nv in enumerate(nvs):
                loop = init_d.clone() if nv == on_top else torch.zeros(16 * V, dtype=_t_c(lprec), device="cuda")
                Ls = fL[:nv]
                hip.performLoopContractionBatched(loop, Ls, Ls if same else fR[:nv], sg[:nv])
                errs[ie, i] = (loop.to(torch.complex128) - ref_d[i]).abs().max() / scale[i]
                if env is None or env in lv.CONTRACT_REJECTED or env in (lv.CONTRACT_THREE_FIELDS, "256,2,1,0"):
                    results[(env, nv)] = loop
                if env is not None:
                    differs[ie, i] = (loop != results[(None, nv)]).any()
        errs, differs = errs.cpu().numpy(), differs.cpu().numpy()
        bad = [(envs[ie], nvs[i], errs[ie, i]) for ie in range(len(envs)) for i in range(len(nvs)) if not errs[ie, i] < tol]
        print("contract %s %s L%sR: worst rel err %.3e (bound %.0e); variants not bit-identical to the default: %s"
              % ("x".join(map(str, X)), name, "==" if same else "!=", np.nanmax(errs), tol, sorted({envs[ie] for ie in np.nonzero(differs.any(axis=1))[0]}) or "none"))
        assert not bad, (X, name, pad, same, bad[:8], len(bad))
        record_max("contract_variants_%s" % ("fp64" if lprec == 8 and prec == 8 else "fp32" if lprec == 4 else "mixed"), errs.max())
        record_max("contract_variant_not_bitwise_%s_%s" % (name, "same" if same else "two_sided"), float(differs.any()))
        for nv in nvs:
            # a rejected string leaves the defaults alone: the bits of the unset run; three fields = the fourth one 0
            for env in lv.CONTRACT_REJECTED:
                assert torch.equal(results[(env, nv)].view(torch.uint8), results[(None, nv)].view(torch.uint8)), (env, nv)
            assert torch.equal(results[(lv.CONTRACT_THREE_FIELDS, nv)].view(torch.uint8), results[("256,2,1,0", nv)].view(torch.uint8)), nv
    # the branch each shape is there for
    want = {(8, 8, 8, 16): True, (6, 6, 6, 6): False, (4, 4, 4, 4): False}.get(X)
    print("contract %s %s: %d (variant, set) pairs run a swizzle that is not the identity" % ("x".join(map(str, X)), name, nontrivial))
    record_max("contract_variants_swizzle_moves_sites_%s" % "x".join(map(str, X)), nontrivial)     # (the shape conditions, in the run's record)
    if want is not None:
        assert (nontrivial > 0) == want
    if X == (8, 8, 8, 16) and fp64 and not mixed:
        block, swz, sites = lv.contract_map(V, None, True, True, False)
        assert (block, swz) == (512, 1) and not np.array_equal(sites, np.arange(V))     # the default headline variant, sites permuted
    if X in ((8, 8, 4, 4), (8, 4, 4, 4)):
        # swizzle on for the small blocks only -- and never in the mixed mode, which launches 4 or 2 workgroups of 256
        on = {b: lv.contract_map(V, "%d,2,1,1" % b, True, fp64 and not mixed, mixed)[1] for b in lv.CONTRACT_BLOCKS}
        assert on == ({b: 0 for b in lv.CONTRACT_BLOCKS} if mixed else {64: 1, 128: int(V == 1024), 256: 0, 512: 0})


# ---- B: the streaming displaced kernel -----------------------------------------------------------------------------------------
# shape -> {direction: (remap on under "*,*,1", remapS)}; every direction of the first three and of the last runs, the others one
STREAM_SHAPES = {(128, 2, 2, 2): {0: (False, 0), 1: (True, 1), 2: (True, 2), 3: (True, 4)},        # y: strideMu 64, remapJ 2; grid 16
                 (16, 8, 2, 2): {0: (False, 0), 1: (False, 0), 2: (True, 1), 3: (True, 2)},        # z: strideMu 64
                 (12, 8, 4, 4): {0: (False, 0), 1: (False, 0), 2: (False, 0), 3: (True, 3)},       # t: strideMu 192, remapS 3
                 (8, 16, 4, 2): {2: (True, 1)},
                 (4, 8, 4, 8): {3: (True, 1)},
                 (6, 6, 6, 6): {0: (False, 0), 1: (False, 0), 2: (False, 0), 3: (False, 0)}}      # volumeCB = 648: refused
STREAM_GRID = {(128, 2, 2, 2): (16, 1), (16, 8, 2, 2): (8, 1), (12, 8, 4, 4): (24, 1), (8, 16, 4, 2): (16, 1), (4, 8, 4, 8): (16, 1),
               (6, 6, 6, 6): (21, 0)}                           # workgroups of 64 sites, and whether "*,1,*" swizzles them (grid % 8 == 0)
STREAM_LENGTHS = ([1, 2, 3], [1, 2, 3, 4], [1, 2, 3, 4, 5])      # three slots, kFusedMaxSlots, a second launch
STREAM_NEV = 3
# fp64: the free calls of test_gpu_driver.py (1e-13); fp32 storage: 1e-5 -- also with complex128 loops, because the path links
# W_k are fp32 fields there, built by k fp32 products, while the oracle multiplies the rounded links in fp64
STREAM_TOL = {8: 1e-13, 4: 1e-5}


@functools.lru_cache(maxsize=None)
def _stream_problem(X, prec):
    rng = np.random.default_rng(31000 + int(np.prod(X)) + X[0])
    cdt = _np_c(prec)
    ev = [_frozen(orc.lex_to_eo(random_spinor_lex(rng, X), X).astype(cdt).astype(np.complex128)) for _ in range(STREAM_NEV)]
    Uo = orc.extended_gauge_from_global(random_gauge_lex(rng, X), (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    return ev, _frozen(Uo.astype(cdt).astype(np.complex128))


@functools.lru_cache(maxsize=None)
def _stream_reference(X, prec, dispstr):
    """slots k = 1 .. 5 of the entry, [5 * 16 * V]"""
    ev, Uo = _stream_problem(X, prec)
    sg = sigmas(STREAM_NEV)
    cprm = orc.LoopComputeParam([dispstr], [1], [5])
    V = int(np.prod(X))
    return _frozen(orc.compute_loop_position_space(ev, np.float32(sg).astype(np.float64) if prec == 4 else sg, cprm, Uo, X)[16 * V:])


@pytest.mark.parametrize("storage", STORAGES, ids=lambda s: s[0])
@pytest.mark.parametrize("X", list(STREAM_SHAPES), ids=lambda X: "x".join(map(str, X)))
def test_streaming_kernel_every_fused_tune_matches_the_oracle(hip, record_max, monkeypatch, X, storage):
    """fused_displaced_contract_kernel (MUGIQ_HIP_FUSED_TILE=0) under MUGIQ_HIP_FUSED_TUNE unset and all eight "nt,swz,remap", both signs,
    three eigenvectors, lengths [1,2,3], [1,2,3,4] and [1,2,3,4,5], slot by slot against orc.compute_loop_position_space.  The
    displacement-aligned order (remap) needs dir >= 1, strideMu % 64 == 0 and volumeCB % 64 == 0: along y (128,2,2,2) strideMu = 64,
    remapJ = 2, grid 16 (swizzle and remap compose); along z (16,8,2,2) and (8,16,4,2) remapS = 1; along t (4,8,4,8) remapS = 1,
    (12,8,4,4) remapS = 3; (6,6,6,6) refuses it (volumeCB = 648); along x it never applies."""
    name, prec, order, lprec = storage
    monkeypatch.setenv("MUGIQ_HIP_FUSED_TILE", "0")
    V = int(np.prod(X))
    ev, Uo = _stream_problem(X, prec)
    sg = sigmas(STREAM_NEV)
    f = [hip.SpinorField(X, prec, order).set_logical(v) for v in ev]
    U = hip.GaugeField(X, (0, 0, 0, 0), prec).set_logical(Uo)
    tol = STREAM_TOL[prec]
    tunes = [None] + lv.STREAM_TUNES
    n_remap = n_swz = 0
    for dirn, (want_remap, want_s) in STREAM_SHAPES[X].items():
        # the conditions this (shape, direction) is there for, from the launch arithmetic itself
        g = lv.stream_launch(X, dirn, None)
        assert (g["remapJ"] > 0) == want_remap and g["remapS"] == want_s, (X, dirn, g)
        assert (g["grid"], g["swizzle"]) == STREAM_GRID[X]
        print("streaming %s dir %d: strideMu %d, grid %d, swizzle %d, remapJ %d, remapS %d"
              % ("x".join(map(str, X)), dirn, g["strideMu"], g["grid"], g["swizzle"], g["remapJ"], g["remapS"]))
        for sign, dispstr in ((hip.DispSignPlus, "+" + "xyzt"[dirn]), (hip.DispSignMinus, "-" + "xyzt"[dirn])):
            links = path_links(hip, X, prec, U, dirn, sign, 5)
            ref_d = _dev(_stream_reference(X, prec, dispstr)).view(5, 16 * V)
            scale = ref_d.abs().amax(dim=1)
            errs = torch.zeros(len(tunes), len(STREAM_LENGTHS), 5, dtype=torch.float64, device="cuda")
            differs = torch.zeros(len(tunes), len(STREAM_LENGTHS), dtype=torch.bool, device="cuda")
            base = {}
            for it, tune in enumerate(tunes):
                _setenv(monkeypatch, "MUGIQ_HIP_FUSED_TUNE", tune)
                g = lv.stream_launch(X, dirn, tune)
                assert lv.is_bijection(lv.stream_sites(X, dirn, tune), V)
                assert (g["remapJ"] > 0) == (want_remap and (tune is None or tune.endswith("1")))
                n_remap += g["remapJ"] > 0
                n_swz += g["swizzle"]
                for il, lengths in enumerate(STREAM_LENGTHS):
                    assert hip.fusedForm(f[0], dirn, lengths, gaugeGiven=False, loopPrecision=lprec)["kernel"] == hip.ENTRY_KERNEL_STREAMING
                    out = torch.zeros(len(lengths), 16 * V, dtype=_t_c(lprec), device="cuda")
                    hip.displacedLoopContractionFused(out, f, sg, links[:len(lengths)], lengths, dirn, sign)
                    n = len(lengths)
                    errs[it, il, :n] = (out.to(torch.complex128) - ref_d[:n]).abs().amax(dim=1) / scale[:n]
                    if tune is None:
                        base[il] = out
                    else:
                        differs[it, il] = (out != base[il]).any()
            errs, differs = errs.cpu().numpy(), differs.cpu().numpy()
            bad = [(tunes[i], STREAM_LENGTHS[j], k + 1, errs[i, j, k]) for i, j, k in zip(*np.nonzero(~(errs < tol)))]
            assert not bad, (X, name, dispstr, bad[:8], len(bad))
            record_max("fused_tune_%s" % ("fp64" if prec == 8 else "fp32" if lprec == 4 else "mixed"), errs.max())
            record_max("fused_tune_not_bitwise_%s" % name, float(differs.any()))
            if differs.any():
                print("streaming %s %s %s: tunes not bit-identical to the default: %s"
                      % ("x".join(map(str, X)), name, dispstr, [tunes[i] for i in np.nonzero(differs.any(axis=1))[0]]))
    record_max("fused_tune_remap_launches_%s" % "x".join(map(str, X)), n_remap)                  # (the shape conditions, in the run's record)
    record_max("fused_tune_swizzle_launches_%s" % "x".join(map(str, X)), n_swz)
    assert (n_remap > 0) == any(r for r, _ in STREAM_SHAPES[X].values())
    assert (n_swz > 0) == bool(STREAM_GRID[X][1])


@pytest.mark.parametrize("order", [2, 4])
def test_streaming_kernel_ghost_layers_under_the_remap(hip, monkeypatch, order):
    """The two-domain emulation of test_fused_operator_with_ghost_layers on global (4,8,4,8), local (4,8,4,4): strideMu along t = 64 and
    volumeCB = 256, so the displacement-aligned order is on where FUSED_TUNE allows it and the shifted reads of the boundary
    workgroups go to the ghost layers; "+t" and "-t", lengths 1 .. 3, every FUSED_TUNE."""
    monkeypatch.setenv("MUGIQ_HIP_FUSED_TILE", "0")
    local = (4, 8, 4, 4)
    seen = set()

    def apply(tune, field):
        _setenv(monkeypatch, "MUGIQ_HIP_FUSED_TUNE", tune)
        g = lv.stream_launch(local, 3, tune)
        assert (g["strideMu"], g["grid"]) == (64, 8)
        assert (g["remapJ"], g["remapS"]) == ((4, 1) if tune is None or tune.endswith("1") else (0, 0))
        assert lv.is_bijection(lv.stream_sites(local, 3, tune), 512)
        assert hip.fusedForm(field, 3, [1, 2, 3], partitioned=True, gaugeGiven=False)["kernel"] == hip.ENTRY_KERNEL_STREAMING
        seen.add((g["remapJ"] > 0, g["swizzle"]))

    fused_two_domains_along_t(hip, order, (4, 8, 4, 8), 1e-13, variants=[None] + lv.STREAM_TUNES, apply=apply)
    assert seen == {(a, b) for a in (False, True) for b in (0, 1)}
    print("streaming ghost layers, local 4x8x4x4 along t: remap on / off x swizzle on / off all ran")


# ---- C: the tile kernels -------------------------------------------------------------------------------------------------------
# Along y, lines = 32 | 16 | 16 | 16, tj = 4 | 4 | 8 | 8 for the 32-line tile | the 16-line tile | the 16-line tile with TILE16_TJ=8 |
# the matrix-pipe tile; nblocks = ceil(numCols / lines) * X1 / tj:
#   (8,16,4,4)  numCols 128: 4*4 = 16 | 8*4 = 32 | 8*2 = 16 | 8*2 = 16   every one a multiple of 8 and >= 16: bit 1 is a non-trivial map
#   (6,16,6,2)  numCols  72: 3*4 = 12 | 5*4 = 20 | 5*2 = 10 | 5*2 = 10   no multiple of 8: bit 1 is dropped, bit 0 survives; ragged
#   (10,16,6,2) numCols 120: 4*4 = 16 | 8*4 = 32 | 8*2 = 16 | 8*2 = 16   multiples of 8 with a ragged last column group
# jtCount = X1 / tj >= 2 and nCC >= 2 in all of them.  (8,16,4,4) also runs z, t (extent 4: one tile along mu) and x: the row tiles,
# which ignore the order.
TILE_SHAPES = {(8, 16, 4, 4): ("+y:1,3;-y:1,2;+z:1,2;-t:1,2;+x:1,2;-x:1", {"mod8": True, "ragged": False}),
               (6, 16, 6, 2): ("+y:1,3;-y:1,2", {"mod8": False, "ragged": True}),
               (10, 16, 6, 2): ("+y:1,2;-y:1,3", {"mod8": True, "ragged": True})}
TILE_NEV = 3


@functools.lru_cache(maxsize=None)
def _tile_problem(X):
    rng = np.random.default_rng(4242 + X[0])
    ev = [_frozen(orc.lex_to_eo(random_spinor_lex(rng, X), X)) for _ in range(TILE_NEV)]
    Uo = _frozen(orc.extended_gauge_from_global(random_gauge_lex(rng, X), (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0)))
    _, s, a, b = orc.parse_disp_entry_string(TILE_SHAPES[X][0])
    cprm = orc.LoopComputeParam(s, a, b)
    return ev, Uo, cprm, _frozen(orc.compute_loop_position_space(ev, sigmas(TILE_NEV), cprm, Uo, X))


def _run_tile_settings(hip, record_max, monkeypatch, X, family, settings):
    entry, want = TILE_SHAPES[X]
    ev, Uo, cprm, ref = _tile_problem(X)
    sg = sigmas(TILE_NEV)
    f = [hip.SpinorField(X, 8, 2).set_logical(v) for v in ev]
    U = hip.GaugeField(X, (0, 0, 0, 0), 8).set_logical(Uo)
    ref_d = _dev(ref)
    scale = float(np.abs(ref).max())
    mask = lv.TILE_FAMILIES[family][1]
    want_family = {"tile32": hip.FUSED_FAMILY_TILE32, "tile32_regs": hip.FUSED_FAMILY_TILE32, "tile16": hip.FUSED_FAMILY_TILE16,
                   "mfma": hip.FUSED_FAMILY_MFMA_COLUMN}[family]
    monkeypatch.setenv("MUGIQ_HIP_REFLECT", "0")                 # both signs go through the kernels
    first = None
    for tag, env in settings:
        for k in lv.TILE_SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        order_env = int(env["MUGIQ_HIP_TILE_ORDER"])
        for i in range(cprm.nDispEntries):                        # the y entries: the shape conditions
            dirn, _ = orc.parse_displacement(cprm.dispString[i])
            if dirn != 1:
                continue
            kv = list(range(cprm.dispStart[i], cprm.dispStop[i] + 1))
            form = hip.fusedForm(f[0], dirn, kv)
            assert form["family"] == want_family, (tag, i, form)
            if family == "tile32":
                assert form["glds"] == 1
            if family == "tile32_regs" or "regs" in tag:
                assert form["glds"] == 0
            assert form["tj"] == (8 if (family == "mfma" or "tj8" in tag) else 4) and form["lines"] == (32 if family.startswith("tile32") else 16)
            geo = lv.tile_geometry(X, dirn, form["tj"], form["lines"])
            order = lv.tile_block_order(order_env, mask, geo["nblocks"])
            assert geo["nJT"] >= 2 and geo["nCC"] >= 2 and geo["ragged"] == want["ragged"]
            assert (geo["nblocks"] % 8 == 0 and geo["nblocks"] >= 16) == want["mod8"] and (geo["nblocks"] % 8 != 0) == (not want["mod8"])
            assert order == (order_env & mask if want["mod8"] else order_env & mask & 1)
            record_max("tile_order_nblocks_%s_%s" % ("x".join(map(str, X)), family if "tj8" not in tag else "tile16_tj8"), geo["nblocks"])
            jt, cc = lv.tile_map(geo["nblocks"], 0, geo["nJT"], order)
            assert len(set(zip(jt.tolist(), cc.tolist()))) == geo["nblocks"]
            if order:
                assert not (np.array_equal(jt, np.arange(geo["nblocks"]) % geo["nJT"]) and np.array_equal(cc, np.arange(geo["nblocks"]) // geo["nJT"]))
            print("tile %s %s %s entry %d: tj %d, lines %d, numCols %d (ragged %s), nCC %d, jtCount %d, nblocks %d (mod 8: %d), order bits %d"
                  % ("x".join(map(str, X)), family, tag, i, form["tj"], form["lines"], geo["numCols"], geo["ragged"], geo["nCC"], geo["nJT"],
                     geo["nblocks"], geo["nblocks"] % 8, order))
        prm = hip.MugiqLoopParam(gauge=U).set_displace_entry_string(entry)
        loop = hip.Loop_Mugiq(prm, f, sg)
        loop.computeCoarseLoop()
        for i in range(cprm.nDispEntries):
            dirn, _ = orc.parse_displacement(cprm.dispString[i])
            if dirn == 1:
                assert loop.entryKernel(i) == (hip.ENTRY_KERNEL_MFMA_COLUMN if family == "mfma" else hip.ENTRY_KERNEL_VECTOR_TILE), (tag, i)
            else:
                assert loop.entryKernel(i) != hip.ENTRY_KERNEL_REFLECTED
        E = hip.loopPlan(prm, f[0], TILE_NEV, axialOk=(1, 1, 1, 1), deviceBytes=torch.cuda.mem_get_info(0)[1])["entries"]
        assert [loop.entryKernel(i) for i in range(len(E))] == [e["kernel"] for e in E]
        got = loop.dataPos_d.clone()
        loop.close()
        err = float((got - ref_d).abs().max()) / scale
        record_max("tile_order_%s" % family, err)
        assert err < 1e-12, (X, family, tag, err)             # the driver's bound for fp64
        # bits against TILE_ORDER=0 of the same family, over the slots of the y entries (the other entries may change family with the
        # setting): the orders of one kernel instance, and the TJ = 8 and register-staged instances of the 16-line tile
        per = 16 * int(np.prod(X))
        ys = torch.cat([got[per * cprm.nLoopOffset[i]:per * (cprm.nLoopOffset[i] + cprm.nLoopPerEntry[i])] for i in range(cprm.nDispEntries)
                        if orc.parse_displacement(cprm.dispString[i])[0] == 1])
        if first is None:
            first = ys
        else:
            kind = "order" if tag.startswith("order") else tag.split("_")[0]
            record_max("tile_%s_not_bitwise_%s" % (kind, family), 0.0 if torch.equal(ys, first) else 1.0)


@pytest.mark.parametrize("family", list(lv.TILE_FAMILIES))
@pytest.mark.parametrize("X", list(TILE_SHAPES), ids=lambda X: "x".join(map(str, X)))
def test_tile_kernels_every_order_matches_the_oracle(hip, record_max, monkeypatch, X, family):
    """MUGIQ_HIP_TILE_ORDER 0 .. 3 through the driver (MUGIQ_HIP_REFLECT=0) for the 32-line tile (TILE_COLS=32, staged global -> LDS and
    through registers), the 16-line tile (TILE_COLS=16; also TILE16_TJ=8 and TILE16_GLDS=0 under orders 0 and 2) and the matrix-pipe
    tile (default).  The shapes (numbers above TILE_SHAPES): (8,16,4,4) 16 or 32 workgroups along y, a multiple of 8, so bit 1 is a map
    that moves workgroups; (6,16,6,2) 12, 20 or 10 workgroups: bit 1 is dropped and bit 0 survives, the last column group ragged
    (72 lines); (10,16,6,2) a multiple of 8 with a ragged last group (120 lines).  jtCount >= 2 and nCC >= 2 throughout."""
    _run_tile_settings(hip, record_max, monkeypatch, X, family, lv.tile_settings(family))


@pytest.mark.parametrize("family,tag", [("tile32", "order1"), ("tile16", "tj8_order2")])
def test_tile_orders_do_not_read_unwritten_lds(hip, record_max, monkeypatch, family, tag):
    """One TILE_ORDER=1 case and one TILE16_TJ=8 case with the LDS of all CUs filled with NaN patterns before every entry point."""
    monkeypatch.setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")
    _run_tile_settings(hip, record_max, monkeypatch, (6, 16, 6, 2), family, [s for s in lv.tile_settings(family) if s[0] == tag])


@pytest.mark.parametrize("family", list(lv.TILE_FAMILIES))
def test_tile_orders_on_interior_and_boundary_launches(family):
    """z and t forced-partitioned on one rank (4,8,8,16): the column tiles launch once over the interior tiles along mu and once over
    the boundary tiles, so jtBegin != 0 and jtCount < nJT (where jt = jtBegin + blk / nCC of the 32-line tile's bit 0 can go wrong);
    t interior: 3 of 4 tiles along mu, 24 or 48 workgroups.  The mu = x entries run the row tiles, which ignore the order.  Every
    TILE_ORDER (and the 16-line tile's TJ = 8 and register staging) against the single-domain oracle."""
    mp.spawn(launch_variant_workers.tile_order_forced_worker,
             args=(1, free_port(), family, (4, 8, 8, 16), (0, 0, 1, 1), "+z:1,2;-z:1,2;+t:1,3;-t:1,2;+x:1,2;-x:1", 3), nprocs=1, join=True)
