"""The workgroup -> work index maps behind the launch-variant switches, as pure index arithmetic (tests/launch_variants.py restates
csrc/contract.hip, csrc/fused.hip and the tile kernels' block order): every map the GPU tests of test_gpu_launch_variants.py run
must visit every site / tile exactly once.  No GPU and no library needed."""
import numpy as np
import pytest

import launch_variants as lv

MODES = [("fp64", True, False), ("fp32", False, False), ("mixed", False, True)]       # (name, fp64 storage, mixed)


def test_tune_string_parsing_matches_the_documented_rules():
    assert lv.contract_tune(None, True, True) == (512, 3, 1, 1) and lv.contract_tune(None, False, True) == (256, 2, 1, 1)
    assert lv.contract_tune(None, True, False) == (256, 2, 1, 1)
    assert lv.contract_tune("64,3,0,1", True, False) == (64, 3, 0, 1)
    assert lv.contract_tune("64,3,0,1", False, False) == (64, 2, 0, 1)               # depth 3 is clamped where L != R
    assert lv.contract_tune("512,1,1,7", True, True) == (512, 1, 1, 1)
    assert lv.contract_tune(lv.CONTRACT_THREE_FIELDS, True, True) == (256, 2, 1, 0)  # three fields: swizzle off
    for bad in lv.CONTRACT_REJECTED + ["", "512", "512,3", "512;3;1;1"]:
        for same in (True, False):
            for fp64 in (True, False):
                assert lv.contract_tune(bad, same, fp64) == lv.contract_tune(None, same, fp64), bad
    assert len(lv.CONTRACT_VARIANTS) == 48 and len(set(lv.CONTRACT_VARIANTS)) == 48


@pytest.mark.parametrize("block,V", [(64, 1024), (128, 1024), (64, 512)])
def test_swizzle_decided_from_the_block_asked_for_loses_sites_in_mixed_mode(block, V):
    """The mixed mode always launches workgroups of 256.  Deciding the XCD swizzle from the block size of the tune string saw a grid that
    is a multiple of 8 where the launched one (4 or 2 workgroups) is not: per = gridDim.x >> 3 = 0, every workgroup computes the
    first 256 sites and the others are never written.  The decision from the launched block size does not swizzle there."""
    env = "%d,2,1,1" % block
    launched, swz, sites = lv.contract_map(V, env, True, False, True, decide_from_launched=False)
    assert launched == 256 and swz == 1
    assert not lv.is_bijection(sites, V)
    assert np.array_equal(np.unique(sites), np.arange(256))                    # sites 256 .. V-1 are never written
    launched, swz, sites = lv.contract_map(V, env, True, False, True)
    assert launched == 256 and swz == 0 and lv.is_bijection(sites, V)
    # the same tune string with storage == arithmetic launches what it asks for: both decisions agree and swizzle
    for fp64 in (True, False):
        for old in (True, False):
            launched, swz, sites = lv.contract_map(V, env, True, fp64, False, decide_from_launched=not old)
            assert launched == block and swz == 1 and lv.is_bijection(sites, V)


def test_every_contraction_variant_of_the_gpu_test_visits_every_site_once():
    """All (V, tune string, storage mode, L == R or not) of test_gpu_launch_variants.py: a bijection with the decision as it is now;
    and the decision as it was is wrong exactly in the mixed mode."""
    envs = [None, lv.CONTRACT_THREE_FIELDS] + lv.CONTRACT_VARIANTS + lv.CONTRACT_REJECTED
    broken = set()
    for X in lv.CONTRACT_SHAPES:
        V = int(np.prod(X))
        for name, fp64, mixed in MODES:
            for same in (True, False):
                for env in envs:
                    block, swz, sites = lv.contract_map(V, env, same, fp64, mixed)
                    assert lv.is_bijection(sites, V), (X, name, same, env, block, swz)
                    if not lv.is_bijection(lv.contract_map(V, env, same, fp64, mixed, decide_from_launched=False)[2], V):
                        assert mixed
                        broken.add((V, lv.contract_tune(env, same, fp64)[0]))
                    if env is None:                                                   # the default launch is what it was
                        assert lv.contract_map(V, env, same, fp64, mixed, decide_from_launched=False)[:2] == (block, swz)
    assert broken == {(1024, 64), (1024, 128), (512, 64)}


def test_contraction_shapes_reach_the_branches_they_are_there_for():
    V = {X: int(np.prod(X)) for X in lv.CONTRACT_SHAPES}
    # block 512 with a map that is not the identity: 16 workgroups, per = 2
    block, swz, sites = lv.contract_map(V[(8, 8, 8, 16)], None, True, True, False)
    assert (block, swz) == (512, 1) and not np.array_equal(sites, np.arange(8192))
    # 8^4 (the largest volume the older tests check site by site) is the identity at 512
    assert np.array_equal(lv.contract_map(4096, None, True, True, False)[2], np.arange(4096))
    on = {b: lv.contract_swizzle(1024, (b, 2, 1, 1), False) for b in lv.CONTRACT_BLOCKS}
    assert on == {64: 1, 128: 1, 256: 0, 512: 0}
    assert {b: lv.contract_swizzle(512, (b, 2, 1, 1), False) for b in lv.CONTRACT_BLOCKS} == {64: 1, 128: 0, 256: 0, 512: 0}
    for b in lv.CONTRACT_BLOCKS:
        assert V[(6, 6, 6, 6)] % b != 0 and lv.contract_swizzle(1296, (b, 2, 1, 1), False) == 0
    assert V[(4, 4, 4, 4)] == 256


@pytest.mark.parametrize("X", [(128, 2, 2, 2), (16, 8, 2, 2), (8, 16, 4, 2), (4, 8, 4, 8), (12, 8, 4, 4), (6, 6, 6, 6), (4, 8, 4, 4)])
def test_streaming_kernel_order_visits_every_site_once(X):
    V = int(np.prod(X))
    for dirn in range(4):
        for tune in [None] + lv.STREAM_TUNES:
            assert lv.is_bijection(lv.stream_sites(X, dirn, tune), V), (X, dirn, tune)


@pytest.mark.parametrize("nblocks,jt_count", [(16, 2), (64, 4), (24, 2), (6, 2), (12, 4), (9, 3), (5, 1)])
def test_tile_order_visits_every_tile_once(nblocks, jt_count):
    for jt_begin in (0, 1):
        for env in range(4):
            order = lv.tile_block_order(env, 3, nblocks)
            assert order == (env if nblocks % 8 == 0 else env & 1)
            jt, cc = lv.tile_map(nblocks, jt_begin, jt_count, order)
            pairs = set(zip(jt.tolist(), cc.tolist()))
            assert pairs == {(jt_begin + j, c) for j in range(jt_count) for c in range(nblocks // jt_count)}
    assert lv.tile_block_order(3, 2, 16) == 2 and lv.tile_block_order(3, 2, 12) == 0 and lv.tile_block_order(3, 3, 16, True) == 0
