"""The shapes that send the fused reorder + x step of convertAndProject through each of its kernel forms, and the class every
shape is meant to land in.  tests/test_gpu_projection_forms.py runs them on the GPU; tests/test_projection_plan_cpu.py checks,
without a GPU, that the plan query puts every one of them in its class -- so a change to the dispatch fails there and does not
silently empty a GPU test.

A case is a dict: id, X = (Lx, Ly, Lz, Lt), prec (8 | 4), pxs (the distinct p_x), nLoop, env (switches to set), grid (process grid
of the three spatial directions; the rank coordinate is grid[d] // 2), expect (members of the plan that must match; "ragged" and
"redBehind" are derived: lastChunk < tChunk, redOffset > 0).
"""
GENERAL, PIPELINED, MFMA = "general", "pipelined", "mfma"
FORM_ID = {GENERAL: 0, PIPELINED: 1, MFMA: 2}          # MUGIQ_HIP_PROJECT_FORM_*

# distinct p_x lists by length: unsorted, both signs, with and without zero ({1, 3, 7, 8}: the zero-filled columns of the matrix
# pipe's phase fragments and its j < nPx guard both vary; 9 and 11: two passes of 8)
PXS = {1: [2], 3: [0, 3, -1], 4: [0, 1, -1, 2], 7: [1, -3, 0, 2, -1, 3, -2], 8: [3, -4, 0, 1, -2, 2, -1, -3],
       9: [4, -4, 0, 1, -2, 2, -1, -3, 3], 11: [5, -5, 4, -4, 0, 1, -2, 2, -1, -3, 3]}


def momenta(pxs):
    """Two p_y and two p_z per p_x, in an order that is sorted in no direction."""
    return [(px, py, (px + py) % 2) for px in pxs for py in (0, 1)]


def case(id_, X, prec, npx, expect, env=None, nLoop=2, grid=(1, 1, 1)):
    return dict(id=id_, X=tuple(X), prec=prec, pxs=PXS[npx], nLoop=nLoop, env=dict(env or {}), grid=tuple(grid), expect=dict(expect))


def grid_of(c):
    """(totalL, commCoord) of a case: the rank in the middle (or at the far end) of its process grid."""
    g = list(c["grid"]) + [1]
    return tuple(c["X"][d] * g[d] for d in range(4)), tuple(g[d] // 2 for d in range(4))


NO_MFMA = {"MUGIQ_HIP_EO_MFMA": "0"}

# (a) the ten reachable instantiations of the matrix-pipe kernel <NKS, MB>, fp64: (shape, nPx, grid, plan of the matrix-pipe run,
#     form in fp32).  The vector run (MUGIQ_HIP_EO_MFMA=0) takes the pipelined form with the same tiling.
MFMA_SHAPES = [
    ((3, 2), (24, 6, 2, 10), 8, (1, 1, 1), dict(tChunk=10, nChunks=1, tiles=3), PIPELINED),
    ((3, 3), (24, 2, 2, 46), 3, (2, 1, 3), dict(tChunk=23, nChunks=2, tiles=2), PIPELINED),      # 46 rows pad to 48
    ((3, 4), (24, 2, 2, 32), 7, (1, 1, 1), dict(tChunk=32, nChunks=1), PIPELINED),
    ((4, 2), (32, 2, 2, 12), 1, (1, 1, 1), dict(tChunk=12, nChunks=1), PIPELINED),
    ((4, 3), (32, 2, 2, 34), 8, (1, 1, 1), dict(tChunk=17, nChunks=2), PIPELINED),               # odd chunk: parity follows t0
    ((4, 4), (32, 2, 2, 32), 3, (1, 1, 1), dict(tChunk=32, nChunks=1), PIPELINED),
    ((6, 2), (48, 2, 2, 16), 7, (1, 1, 1), dict(tChunk=16, nChunks=1), PIPELINED),
    ((6, 3), (48, 6, 2, 20), 1, (1, 2, 1), dict(tChunk=20, nChunks=1, tiles=3), PIPELINED),
    ((8, 2), (64, 2, 2, 32), 3, (1, 1, 1), dict(tChunk=16, nChunks=2), GENERAL),
    ((8, 3), (64, 2, 2, 24), 8, (1, 1, 1), dict(tChunk=24, nChunks=1), PIPELINED),
]
MFMA_CASES = []          # triples (matrix pipe, vector fp64, fp32) of one shape
for (nks, mb), X, npx, grid, tiling, form32 in MFMA_SHAPES:
    tag = "mfma%d%d" % (nks, mb)
    MFMA_CASES.append((
        case(tag, X, 8, npx, dict(form=MFMA, nks=nks, mb=mb, rowPasses=1, pxPasses=1, redBehind=False, ragged=False, **tiling), grid=grid),
        case(tag + "-vector", X, 8, npx, dict(form=PIPELINED, nks=0, mb=0, ragged=False, **tiling), env=NO_MFMA, grid=grid),
        case(tag + "-fp32", X, 4, npx, dict(form=form32), grid=grid)))

# (b) the general kernel
GENERAL_CASES = [
    case("g128x40-fp64-ragged", (128, 2, 2, 40), 8, 4, dict(form=GENERAL, tChunk=14, nChunks=3, lastChunk=12, ragged=True, stagingPieces=2)),
    case("g128x40-fp32", (128, 2, 2, 40), 4, 4, dict(form=GENERAL, tChunk=20, nChunks=2, ragged=False, stagingPieces=2)),
    case("g96x34-fp64-9px", (96, 2, 2, 34), 8, 9, dict(form=GENERAL, tChunk=9, nChunks=4, lastChunk=7, ragged=True, pxPasses=2, redBehind=True,
                                                         stagingPieces=2), grid=(3, 1, 2)),
    case("g96x48-fp64", (96, 2, 2, 48), 8, 4, dict(form=GENERAL, ragged=False, stagingPieces=2)),
    case("g96x48-fp32", (96, 2, 2, 48), 4, 4, dict(form=GENERAL, ragged=False, stagingPieces=2)),
    case("g66x30-fp64", (66, 2, 2, 30), 8, 3, dict(form=GENERAL, stagingPieces=2)),          # run = 66: a full piece and one of 2 entries
    case("g66x30-fp32", (66, 2, 2, 30), 4, 3, dict(form=GENERAL, stagingPieces=2)),
    case("g130x6-fp64", (130, 2, 2, 6), 8, 7, dict(form=GENERAL, stagingPieces=3)),          # Lx = 2 mod 4: x classes of 33, 33, 32, 32
    case("g130x6-fp32", (130, 2, 2, 6), 4, 7, dict(form=GENERAL, stagingPieces=3), grid=(2, 2, 1)),
]
# 96 rows in one tile (96 runs are more than the pipelined staging covers): two row passes, the second with 32 clamped lanes
TWO_ROW_PASS_CASE = case("g48x48-fp32-2rowpasses", (48, 2, 2, 48), 4, 4, dict(form=GENERAL, tChunk=48, nChunks=1, rowPasses=2, redBehind=True,
                                                                            stagingPieces=1))

# (c) several tiles per workgroup, forced: (shape, precision, switches, form, tiles, chunks per y pair)
WALK_SHAPES = [
    ("walk-mfma", (48, 6, 2, 48), 8, {}, MFMA, 6, 2),
    ("walk-vector", (48, 6, 2, 48), 8, NO_MFMA, PIPELINED, 6, 2),
    ("walk-fp32", (32, 10, 2, 8), 4, {}, PIPELINED, 5, 1),
]


def walk_cases():
    out = []
    for tag, X, prec, env, form, tiles, nch in WALK_SHAPES:
        for per in (2, 3, 4, tiles):
            e = dict(env)
            e["MUGIQ_HIP_EO_TILES_PER_WG"] = str(per)
            out.append(case("%s-%d" % (tag, per), X, prec, 3, dict(form=form, tiles=tiles, nChunks=nch, tilesPerWg=per, workgroupsX=-(-tiles // per)),
                            env=e, grid=(1, 3, 1) if per == 4 else (1, 1, 1)))
    return out


WALK_CASES = walk_cases()
# ... and where the work-per-CU heuristic itself asks for it (Lz * nData * tiles > 8192), no switch set
NATURAL_WALK_CASES = [
    case("natural-mfma", (24, 10, 16, 10), 8, 3, dict(form=MFMA, nks=3, mb=2, tiles=5, tilesPerWg=2, workgroupsX=3), nLoop=8),
    case("natural-vector", (24, 10, 16, 10), 8, 3, dict(form=PIPELINED, tiles=5, tilesPerWg=2, workgroupsX=3), env=NO_MFMA, nLoop=8, grid=(2, 1, 1)),
    case("natural-fp32", (8, 10, 16, 4), 4, 7, dict(form=PIPELINED, tiles=5, tilesPerWg=2, workgroupsX=3), nLoop=8),
]

# (d) slot subsets: one shape per form, nLoop = 5 (the plan is taken with nData = 16 * number of slots)
SLOT_CASES = [
    case("slots-general", (66, 2, 2, 4), 8, 3, dict(form=GENERAL), nLoop=5),
    case("slots-pipelined", (8, 4, 2, 6), 4, 9, dict(form=PIPELINED, pxPasses=2), nLoop=5, grid=(2, 1, 2)),
    case("slots-mfma", (24, 4, 2, 10), 8, 7, dict(form=MFMA, nks=3, mb=2), nLoop=5),
]
SLOT_SETS = [[3], [4, 0, 2], [0, 1, 2, 3, 4]]

# (e) poisoned LDS: one case per form, with the padded rows (46 -> 48) and a ragged chunk among them
POISON_CASES = [MFMA_CASES[1][0], MFMA_CASES[1][1], GENERAL_CASES[0], GENERAL_CASES[2], TWO_ROW_PASS_CASE, WALK_CASES[2]]

ALL_CASES = ([c for t in MFMA_CASES for c in t] + GENERAL_CASES + [TWO_ROW_PASS_CASE] + WALK_CASES + NATURAL_WALK_CASES + SLOT_CASES)


def plan_matches(plan, expect):
    """The list of (member, planned, expected) that differ."""
    got = dict(plan)
    got["ragged"] = plan["lastChunk"] < plan["tChunk"]
    got["redBehind"] = plan["redOffset"] > 0
    bad = []
    for k, v in expect.items():
        want = FORM_ID[v] if k == "form" else v
        if got[k] != want:
            bad.append((k, got[k], want))
    return bad


# (f) the seeded sweep: what seed number `seed` draws (shared, so that the CPU test can count the forms through the plan query)
SWEEP_SEED_BASE = 9100
SWEEP_LX = [2, 6, 10, 16, 24, 28, 32, 40, 48, 56, 64, 66, 96, 128]
SWEEP_MAX_SITES = 1 << 16          # local sites per case (x 16 nLoop complex numbers): the whole sweep stays within seconds


def sweep_draw(np, seed):
    rng = np.random.default_rng(SWEEP_SEED_BASE + seed)
    while True:
        X = (int(rng.choice(SWEEP_LX)), int(rng.choice([2, 4, 6])), int(rng.choice([2, 4, 6])), 2 * int(rng.integers(1, 26)))
        if X[0] * X[1] * X[2] * X[3] <= SWEEP_MAX_SITES:
            break
    grid = [int(v) for v in rng.choice([1, 1, 2, 3], size=3)] + [1]
    coord = tuple(int(rng.integers(g)) for g in grid)
    tot = tuple(X[d] * grid[d] for d in range(4))
    prec = int(rng.choice([8, 4]))
    nLoop = int(rng.integers(1, 4))
    nmom = int(rng.integers(1, 21))
    mom = [(int(rng.integers(-6, 7)), int(rng.integers(-3, 4)), int(rng.integers(-3, 4))) for _ in range(nmom)]
    FTSign = int(rng.choice([-1, 1]))
    return dict(X=X, tot=tot, coord=coord, prec=prec, nLoop=nLoop, mom=mom, FTSign=FTSign, rng=rng)
