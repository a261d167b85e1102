"""Host-side restatement of the launch arithmetic behind the MUGIQ_HIP_* launch-variant switches, for
test_launch_variants_cpu.py (which checks the maps themselves) and test_gpu_launch_variants.py (which asserts that every case it
runs exercises the branch it is there for).  Pure Python / numpy: no GPU, no library.

  contract_*   loop_contract_kernel, csrc/contract.hip        (MUGIQ_HIP_CONTRACT_TUNE = "block,depth,nt,swz")
  stream_*     fused_displaced_contract_kernel, csrc/fused.hip (MUGIQ_HIP_FUSED_TUNE = "nt,swz,remap")
  tile_*       the workgroup -> tile map of csrc/fused_tile.hip, fused_tile16.hip, fused_mfma_kernel.h (MUGIQ_HIP_TILE_ORDER)
"""
import itertools
import re

import numpy as np

# ---- loop_contract_kernel ------------------------------------------------------------------------------------------------------
CONTRACT_BLOCKS = (64, 128, 256, 512)
CONTRACT_VARIANTS = ["%d,%d,%d,%d" % v for v in itertools.product(CONTRACT_BLOCKS, (1, 2, 3), (0, 1), (0, 1))]
CONTRACT_THREE_FIELDS = "256,2,1"                     # sscanf(...) >= 3 takes it; swz stays 0
CONTRACT_REJECTED = ["100,2,1,1", "512,4,1,1", "512,3,2,1", "x"]

# the shapes of the GPU test, and the eigenvector counts each runs (None: 1 .. 13)
CONTRACT_NVEC_MAX = 13
CONTRACT_SHAPES = {(8, 8, 8, 16): (1, 5, 13),         # V = 8192: 16 workgroups of 512, per = 2: the smallest non-trivial map at 512
                   (8, 8, 4, 4): None,                # V = 1024: swizzle on for 64 and 128, off for 256 and 512
                   (8, 4, 4, 4): None,                # V = 512:  swizzle on for 64 only
                   (6, 6, 6, 6): (1, 5, 13),          # V = 1296: ragged last workgroup at every block size, swizzle off
                   (4, 4, 4, 4): None}                # V = 256:  half-empty workgroup at 512


def _scan_ints(s, most):
    """the leading "%d,%d,..." of sscanf: how many converted, and their values"""
    out, pos = [], 0
    while len(out) < most:
        m = re.compile(r"\s*([+-]?\d+)").match(s, pos)
        if not m:
            break
        out.append(int(m.group(1)))
        pos = m.end()
        if pos >= len(s) or s[pos] != ",":
            break
        pos += 1
    return out


def contract_tune(env, same, fp64_storage):
    """contract_tune of csrc/contract.hip: (block, depth, nt, swz) for MUGIQ_HIP_CONTRACT_TUNE = env (None: unset).
    fp64_storage: fp64 fields AND fp64 loop buffer."""
    t = (512, 3, 1, 1) if (same and fp64_storage) else (256, 2, 1, 1)
    if env is not None:
        v = _scan_ints(env, 4)
        if len(v) >= 3:
            b, d, n = v[:3]
            w = v[3] if len(v) > 3 else 0
            if b in CONTRACT_BLOCKS and 1 <= d <= 3 and n in (0, 1):
                t = (b, 2 if (not same and d > 2) else d, n, 1 if w else 0)
    return t


def contract_launched_block(block, mixed):
    """launch_block: the mixed mode (fp32 fields, fp64 arithmetic) is built for 256 only"""
    return 256 if mixed else block


def contract_swizzle(V, tune, mixed, decide_from_launched=True):
    """xcdSwizzle of launch_contract.  decide_from_launched=False: the decision as it was taken from the block size ASKED for."""
    block = contract_launched_block(tune[0], mixed) if decide_from_launched else tune[0]
    return 1 if (tune[3] and ((V + block - 1) // block) % 8 == 0) else 0


def contract_sites(V, block, swizzle):
    """Every site index < V the grid writes, workgroup by workgroup (loop_contract_kernel: blk -> site)."""
    grid = (V + block - 1) // block
    blk = np.arange(grid)
    if swizzle:
        blk = (blk & 7) * (grid >> 3) + (blk >> 3)
    site = (blk[:, None] * block + np.arange(block)[None, :]).reshape(-1)
    return site[site < V]


def is_bijection(sites, V):
    return sites.size == V and np.array_equal(np.sort(sites), np.arange(V))


def contract_map(V, env, same, fp64_storage, mixed, decide_from_launched=True):
    """(launched block, swizzle, sites written) of one call"""
    t = contract_tune(env, same, fp64_storage)
    block = contract_launched_block(t[0], mixed)
    swz = contract_swizzle(V, t, mixed, decide_from_launched)
    return block, swz, contract_sites(V, block, swz)


# ---- fused_displaced_contract_kernel -------------------------------------------------------------------------------------------
STREAM_TUNES = ["%d,%d,%d" % v for v in itertools.product((0, 1), repeat=3)]


def stream_launch(X, dirn, tune):
    """launch_fused of csrc/fused.hip: dict(grid, strideMu, swizzle, remapJ, remapS) for MUGIQ_HIP_FUSED_TUNE = tune (None: unset)"""
    nt, swz, remap = (1, 1, 1) if tune is None else tuple(int(v) for v in tune.split(","))
    V = int(np.prod(X))
    vcb = V // 2
    grid = (V + 63) // 64
    stride = 1
    for d in range(dirn):
        stride *= X[d]
    stride //= 2
    on = bool(remap and dirn >= 1 and stride % 64 == 0 and vcb % 64 == 0)
    return {"grid": grid, "strideMu": stride, "swizzle": 1 if (swz and grid % 8 == 0) else 0,
            "remapJ": X[dirn] if on else 0, "remapS": stride // 64 if on else 0}


def stream_sites(X, dirn, tune):
    """Every site index < V the streaming kernel's grid writes (blk -> site, the swizzle and the remap composed)."""
    g = stream_launch(X, dirn, tune)
    V = int(np.prod(X))
    vcb = V // 2
    blk = np.arange(g["grid"])
    if g["swizzle"]:
        blk = (blk & 7) * (g["grid"] >> 3) + (blk >> 3)
    if g["remapJ"]:
        p, r = blk & 1, blk >> 1
        j = r % g["remapJ"]
        r = r // g["remapJ"]
        c, hi = r % g["remapS"], r // g["remapS"]
        base = p * vcb + hi * (g["remapJ"] * g["strideMu"]) + j * g["strideMu"] + c * 64
    else:
        base = blk * 64
    site = (base[:, None] + np.arange(64)[None, :]).reshape(-1)
    return site[site < V]


# ---- the tile kernels ----------------------------------------------------------------------------------------------------------
def tile_block_order(order_env, family_mask, nblocks, row_order_off=False):
    """FusedLaunchBase::block_order: the bits of MUGIQ_HIP_TILE_ORDER a launch of nblocks workgroups keeps
    (family_mask 3: the 32-line tile, 2: the 16-line and the matrix-pipe tiles)"""
    bits = order_env & family_mask
    return 0 if row_order_off else (bits & 1 if nblocks % 8 != 0 else bits)


def tile_map(nblocks, jt_begin, jt_count, order):
    """blockIdx -> (jt, cc) of a column-tile launch (csrc/fused_tile.hip; the other two families know bit 1 only)"""
    blk = np.arange(nblocks)
    if order & 2:
        blk = (blk & 7) * (nblocks >> 3) + (blk >> 3)
    if order & 1:
        ncc = nblocks // jt_count
        return jt_begin + blk // ncc, blk % ncc
    return jt_begin + blk % jt_count, blk // jt_count


def tile_range(region, partitioned, sign_plus, njt, kmax, tj):
    """tile_range of csrc/fused_form.h: (jtBegin, jtCount) of a launch over region "all" | "interior" | "boundary" """
    if region == "all":
        return 0, njt
    nb = min(njt, (kmax + tj - 1) // tj) if partitioned else 0
    if region == "interior":
        return (0 if sign_plus else nb), njt - nb
    return (njt - nb if sign_plus else 0), nb


def tile_geometry(X, dirn, tj, lines):
    """dict(numCols, nCC, nJT, nblocks, ragged) of a column-tile launch over every tile along mu"""
    num_cols = int(np.prod(X)) // X[dirn]
    ncc, njt = (num_cols + lines - 1) // lines, X[dirn] // tj
    return {"numCols": num_cols, "nCC": ncc, "nJT": njt, "nblocks": ncc * njt, "ragged": num_cols % lines != 0}


# the four tile families of test_gpu_launch_variants.py: the switches that select them, and the TILE_ORDER bits they know
TILE_FAMILIES = {"tile32": ({"MUGIQ_HIP_TILE_COLS": "32"}, 3),
                 "tile32_regs": ({"MUGIQ_HIP_TILE_COLS": "32", "MUGIQ_HIP_TILE_GLDS": "0"}, 3),
                 "tile16": ({"MUGIQ_HIP_TILE_COLS": "16"}, 2),
                 "mfma": ({}, 2)}
TILE_SWITCHES = ("MUGIQ_HIP_TILE_COLS", "MUGIQ_HIP_TILE_GLDS", "MUGIQ_HIP_TILE_ORDER", "MUGIQ_HIP_TILE16_TJ", "MUGIQ_HIP_TILE16_GLDS",
                 "MUGIQ_HIP_FUSED_TILE", "MUGIQ_HIP_TILE_MFMA", "MUGIQ_HIP_MFMA_TJ", "MUGIQ_HIP_FUSED_TUNE")


def tile_settings(family):
    """[(tag, env)] a family runs: TILE_ORDER 0 .. 3; the 16-line tile also TILE16_TJ = 8 and TILE16_GLDS = 0 under orders 0 and 2"""
    base = TILE_FAMILIES[family][0]
    out = [("order%d" % o, dict(base, MUGIQ_HIP_TILE_ORDER=str(o))) for o in range(4)]
    if family == "tile16":
        for o in (0, 2):
            out.append(("tj8_order%d" % o, dict(base, MUGIQ_HIP_TILE_ORDER=str(o), MUGIQ_HIP_TILE16_TJ="8")))
            out.append(("regs_order%d" % o, dict(base, MUGIQ_HIP_TILE_ORDER=str(o), MUGIQ_HIP_TILE16_GLDS="0")))
    return out
