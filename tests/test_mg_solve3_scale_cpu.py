"""CPU checks behind tests/test_gpu_mg_solve3_scale.py: the chain hierarchy of tests/mg_solve3_scale_cases.py (A_1 = R_0 M P_0,
A_2 = R_1 A_1 P_1, no matrices) is mg_solve_ref.ChainProblem with one coarse level, bit for bit, and gives the K^(3) of the explicit
matrices at PROD; the restatement's own sensitivity to 1-ulp perturbations at PROD and WIDE, which is what lets the GPU tests keep the
bound of K (1e-12); the fp32 model's movement at PROD, from which their fp32 bound is made; the host query of the coarse application's
form (mugiq_hip_coarse_apply_outputs / coarseApplyForm) against the table of DESIGN.md 4.4h, at WIDE, and under its environment switch;
and the count relation the device-built hierarchy of the GPU tests rests on.  No GPU is touched."""
import os

import numpy as np
import pytest

import coarse_op_cases as coc
import mg_solve3_cases as c3
import mg_solve3_ref as m3
import mg_solve3_scale_cases as sc
import mg_solve_cases as mgc
import mg_solve_ref as mgr
from util import ROOT, rel_err

BOUND = 1e-12                     # what the GPU tests hold K^(3) to against the restatement
FORM_ENV = "MUGIQ_HIP_COARSE_APPLY_OUT"


# ---- the chain ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prm", [mgc.K_PARAMS[1], mgc.EDGE_PARAMS[0]], ids=["1-1-8", "omega-16"])
def test_chain_with_one_level_is_ChainProblem(prm):
    X, bs, nvec = coc.SHAPES[1]
    prob = mgc.shape_problem(X, bs, nvec, chain=True)
    h = sc.chain_hierarchy(X, prob.Uo, coc.KAPPA, [prob.V], [bs])
    r = mgc.shape_rhs(X)[0]
    assert np.array_equal(m3.K(h, r, [prm]), mgr.K(prob, r, **prm))


@pytest.mark.parametrize("name", ["prod", "prod-clover"])
def test_chain_gives_the_K3_of_the_explicit_matrices(name, record_max):
    """PROD, sets A and B, right-hand side 0: the distance must stay below BOUND / 100 for the chain to serve as the reference where no
    matrices can be had (WIDE)"""
    for s in sc.PROD_PARAMS:
        d = rel_err(sc.K3_reference(name, s, 0), sc.K3_explicit(name, s, 0))
        print("%s set %s: K^(3) of the chain against the explicit matrices %.3e" % (name, s, d))
        record_max("mg3_scale_chain_vs_explicit", d)
        assert d < BOUND / 100.0, (name, s, d)


# ---- the sensitivities the bounds come from ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["prod-clover", "wide"])
def test_restatement_is_no_more_sensitive_here(name, record_max):
    """K^(3)(r_0) under three 1-ulp perturbations of r_0 moves by a few 1e-16 of its max norm, as on the hierarchies of
    tests/mg_solve3_cases.py (3.3e-16 .. 6.3e-16): 1e-12 stays 100 times and more above it, so the bound of K is kept"""
    for s in sc.sets(name):
        v = sc.K3_sensitivity(name, s)
        print("%s set %s: 1-ulp sensitivity of the restatement %.3e" % (name, s, v))
        record_max("mg3_scale_reference_sensitivity_%s" % name.split("-")[0], v)
        assert 0.0 < 100.0 * v < BOUND, (name, s, v)


def test_fp32_model_movement_at_PROD(record_max):
    """the model under 1-ulp (fp32) perturbations of r_0: times mg_solve_mixed_cases.K_MARGIN it is the GPU test's bound, set by set"""
    for s in sc.PROD_PARAMS:
        v = sc.K32_sensitivity("prod-clover", s)
        print("prod-clover set %s: 1-ulp (fp32) movement of the model %.3e" % (s, v))
        record_max("mg3_scale_model_sensitivity", v)
        assert 1e-8 < v < 1e-5, (s, v)                   # a few fp32 ulps (6e-8): neither exact nor lost


# ---- the form of the coarse application ----------------------------------------------------------------------------------------------------
def test_form_query_is_declared_and_exported(hip):
    hdr = open(os.path.join(ROOT, "include", "mugiq_hip.h")).read()
    name = "mugiq_hip_coarse_apply_outputs"
    assert name + "(" in hdr and hasattr(hip._lib.load(), name) and name in hip._lib.SIGNATURES
    assert "coarseApplyForm" in open(os.path.join(ROOT, "include", "mugiq_hip_operators.hpp")).read()


@pytest.mark.parametrize("X,nvec,n,workgroups,want", [((4, 4, 4, 4), 32, 8, 256, 32), ((4, 4, 4, 6), 32, 8, 384, 32), ((4, 4, 4, 8), 32, 8, 512, 64),
                                                      ((8, 8, 8, 8), 24, 8, 4096, 64), ((4, 4, 4, 4), 32, 1, 256, 32), ((4, 4, 4, 4), 32, 9, 512, 64),
                                                      ((4, 4, 4, 4), 33, 8, 512, 64), ((2, 2, 2, 2), 64, 17, 96, 32)])
def test_form_follows_the_table(hip, X, nvec, n, workgroups, want, monkeypatch):
    """32 outputs below 512 workgroups of the 64-output grid -- sites x ceil(n / 8) x ceil(N / 64) -- else 64; the storage
    precision plays no part"""
    monkeypatch.delenv(FORM_ENV, raising=False)
    assert int(np.prod(X)) * ((n + 7) // 8) * ((2 * nvec + 63) // 64) == workgroups
    assert hip.coarseApplyForm((X, nvec), n) == want
    assert hip.coarseApplyForm((X, nvec, 4), n) == want


def test_form_at_WIDE_and_under_the_switch(hip, monkeypatch):
    """WIDE is what it is chosen for: M_1 takes the 64-output form by default and M_2 the 32-output one.  The switch overrides both;
    anything but 16, 32 and 64 is ignored."""
    _, _, nv0, _, nv1, _ = sc.SHAPES["wide"]
    _, X1, X2 = sc.dims("wide")
    ops = {(X1, nv0): 64, (X2, nv1): 32}
    monkeypatch.delenv(FORM_ENV, raising=False)
    for op, want in ops.items():
        assert hip.coarseApplyForm(op, 8) == want
    for out in (16, 32, 64):
        monkeypatch.setenv(FORM_ENV, str(out))
        assert all(hip.coarseApplyForm(op, 8) == out for op in ops)
    for junk in ("", "0", "48", "128", "-32", "sixty-four"):
        monkeypatch.setenv(FORM_ENV, junk)
        for op, want in ops.items():
            assert hip.coarseApplyForm(op, 8) == want, junk
    # PROD never reaches the 64-output form: 64 sites x 1 chunk, 16 sites x 1 chunk
    monkeypatch.delenv(FORM_ENV)
    _, P1, P2 = sc.dims("prod")
    assert hip.coarseApplyForm((P1, 24), 8) == 32 and hip.coarseApplyForm((P2, 32), 8) == 32


def test_form_query_refuses_what_the_application_refuses(hip):
    for bad, n in ((((4, 4, 4, 3), 8), 8), (((4, 4, 4, 4), 0), 8), (((4, 4, 4, 4), 65), 8), (((4, 4, 4, 4), 8, 2), 8), (((4, 4, 4, 4), 8), 0)):
        with pytest.raises(hip.MugiqHipError, match="coarseApplyOutputs"):
            hip.coarseApplyForm(bad, n)


# ---- what the device-built hierarchy of the GPU tests rests on -------------------------------------------------------------------------------
def test_three_levels_take_fewer_iterations_than_two_on_the_smooth_hierarchy():
    """mg_solve3_cases.SOLVE_PARAMS on the three right-hand sides of smooth_rhs(): the three-level count is strictly smaller than the
    two-grid count with the same params[0] for each (30 / 26 / 32 against 48 / 45 / 53 when this was written; another BLAS may move a count
    by one), and not marginally"""
    sm = c3.smooth()
    tol, runs = c3.smooth_reference_solves()
    two = m3.Hierarchy.of_problem(sm["two"])
    n3 = [r[1] for r in runs]
    n2 = []
    for b in c3.smooth_rhs():
        _, it, _, ok = m3.solve(two, b, [dict(c3.SOLVE_PARAMS[0], tol=tol)])
        assert ok
        n2.append(it)
    print("outer iterations on the smooth hierarchy: three levels %s, two %s" % (n3, n2))
    assert all(a < b for a, b in zip(n3, n2)) and all(a <= 0.8 * b for a, b in zip(n3, n2)), (n3, n2)
    assert all(abs(a - w) <= 1 for a, w in zip(n3, (30, 26, 32))) and all(abs(b - w) <= 1 for b, w in zip(n2, (48, 45, 53))), (n3, n2)
