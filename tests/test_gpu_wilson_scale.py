"""GPU tests of the Wilson operator, the eigenpair check, projectVector and the CG beyond one workgroup of the reductions: lattices
of 1 296 .. 1 048 576 sites, chosen for the launch shape of wilson_reduce_kernel / cg_update_kernel / lincomb_kernel (256 lanes per
group, at most 1024 groups, a grid-stride loop) -- several groups with a ragged last one, exactly the cap, a second trip for a few
sites only, a ragged second trip, four full trips.  The numpy reference costs seconds per application at these sizes, so the answers
come from tests/wilson_planewave.py: plane waves on a pure-gauge field, where M psi, the eigenpairs of H, M^dag M and M M^dag, the
iteration count of CG and the solution are known in closed form while every link is a different SU(3) matrix.
tests/test_wilson_planewave_cpu.py pins that family to tests/wilson_ref.py.

Fields of a million sites go to the device in lexicographic order and are brought into the library's layouts there by index
copies (test_fast_layouts_equal_the_slow_ones pins these to SpinorField.set_logical / GaugeField.set_logical); comparisons of whole
fields run on the device in complex128 with torch."""
import math

import numpy as np
import pytest
import torch

import wilson_planewave as pw
import wilson_ref as wr
from util import orc, random_gauge_lex, rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = {8: 1e-13, 4: 1e-5}                  # as tests/test_gpu_wilson.py
KAPPA = 0.12
# X, sites, groups of a reduction: see the module docstring
SIZES = [(6, 6, 6, 6), (8, 8, 8, 8), (16, 16, 32, 32), (18, 18, 18, 46), (24, 24, 24, 24), (32, 32, 32, 32)]
FULL = [(6, 6, 6, 6), (24, 24, 24, 24)]    # every operator and storage; the other sizes: H and M^dag M in two storages
STORAGES = [(8, 2, 0), (8, 4, 7), (4, 2, 32), (4, 4, 0)]              # precision, field order, pad (NaN-filled where not 0)
NAN = complex(float("nan"), float("nan"))


def _ids(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else None


# ---- lattices: gauge field on the host, fields on the device, all released when this module's tests are done ----------------------
class _Lattice:
    def __init__(self, X):
        self.X, self.V = X, int(np.prod(X))
        self.U_lex, self.g = pw.pure_gauge_lex(self.rng_for("gauge"), X)
        _, _, inv = orc.eo_site_tables(X)
        self.inv = torch.from_numpy(inv).to(DEV)                      # lexicographic index of (parity, x_cb)
        self.gauges, self.cache = {}, {}

    def rng_for(self, key):
        """a generator of its own per use, so that a case does not depend on which tests ran before it"""
        return np.random.default_rng([ord(c) for c in key] + list(self.X))

    def dev(self, v_lex):
        return torch.from_numpy(np.ascontiguousarray(v_lex).reshape(self.V, 12)).to(DEV)

    def field(self, n, amp, scale=1.0):
        """device [V, 12]: scale g(x) sum_k amp[k] exp(i n[k] x)"""
        return self.dev(pw.plane_wave_field(self.g, self.X, n, [scale * np.asarray(a) for a in amp]))


_LAT = {}


def _lat(X):
    if X not in _LAT:
        _LAT[X] = _Lattice(X)
    return _LAT[X]


@pytest.fixture(scope="module", autouse=True)
def _release_lattices():
    """the caches hold about 30 GB of device fields over all sizes: give them back before the next module runs"""
    yield
    _LAT.clear()
    torch.cuda.empty_cache()


def _sync():
    torch.cuda.synchronize()


def _new(hip, lat, prec, order, pad=0):
    f = hip.SpinorField(lat.X, prec, order, pad=pad, device=DEV)
    if pad:
        f.data.fill_(NAN)                                              # the body is overwritten by _upload or by the library
    return f


def _upload(lat, f, t):
    """t: device [V, 12] complex128 in lexicographic site order -> the body of f (rounded to f's precision)"""
    vcb, st = f.volumeCB, f.stride
    eo = t[lat.inv].to(f.data.dtype)                                   # [2, vcb, 12]
    if f.order == 2:
        f.data.view(2, 12, st)[:, :, :vcb] = eo.permute(0, 2, 1)
    else:
        f.data.view(2, 6, st, 2)[:, :, :vcb, :] = eo.view(2, vcb, 6, 2).permute(0, 2, 1, 3)
    return f


def _download(lat, f):
    """the body of f as device [V, 12] complex128, lexicographic"""
    vcb, st = f.volumeCB, f.stride
    if f.order == 2:
        eo = f.data.view(2, 12, st)[:, :, :vcb].permute(0, 2, 1)
    else:
        eo = f.data.view(2, 6, st, 2)[:, :, :vcb, :].permute(0, 2, 1, 3)
    out = torch.empty(lat.V, 12, dtype=torch.complex128, device=f.data.device)
    out[lat.inv.reshape(-1)] = eo.reshape(lat.V, 12).to(torch.complex128)
    return out


def _pad_view(f):
    """the elements of f outside its body"""
    vcb, st = f.volumeCB, f.stride
    return (f.data.view(2, 12, st)[:, :, vcb:] if f.order == 2 else f.data.view(2, 6, st, 2)[:, :, vcb:, :]).contiguous()


def _pads(f):
    """... as bit patterns, to see that a call left them alone"""
    return torch.view_as_real(_pad_view(f)).view(torch.int64 if f.precision == 8 else torch.int32).clone()


def _make(hip, lat, prec, order, pad, t):
    return _upload(lat, _new(hip, lat, prec, order, pad), t)


def _rounded(t, prec):
    return t if prec == 8 else t.to(torch.complex64).to(torch.complex128)


def _gauge(hip, lat, prec):
    """the pure-gauge links of the lattice in the library's layout, no border"""
    if prec not in lat.gauges:
        G = hip.GaugeField(lat.X, (0, 0, 0, 0), prec, device=DEV)
        U = torch.from_numpy(lat.U_lex.reshape(4, lat.V, 9)).to(DEV)
        eo = U[:, lat.inv].to(G.data.dtype)                            # [4, 2, vcb, 9]
        G.data.view(2, 36, G.stride)[:, :, :G.volumeExCB] = eo.permute(1, 0, 3, 2).reshape(2, 36, G.volumeExCB)
        lat.gauges[prec] = G
    return lat.gauges[prec]


def _err(got, want):
    """max-norm relative difference of two device fields, and whether `got` is finite"""
    assert bool(torch.isfinite(torch.view_as_real(got)).all())
    return float((got - want).abs().max() / want.abs().max())


def _bits_equal(a, b):
    return a.dtype == b.dtype and torch.equal(torch.view_as_real(a).view(torch.int64 if a.dtype == torch.complex128 else torch.int32),
                                              torch.view_as_real(b).view(torch.int64 if b.dtype == torch.complex128 else torch.int32))


def _ramp(rng, shape=(4, 3)):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _unit(rng, n=3):
    c = _ramp(rng, (n,))
    return c / np.linalg.norm(c)


@pytest.mark.parametrize("prec,order,pad", STORAGES)
def test_fast_layouts_equal_the_slow_ones(hip, prec, order, pad):
    """The index copies on the device that this file moves fields with, against set_logical / get_logical of the bindings."""
    X = (6, 6, 6, 6)
    lat = _lat(X)
    v = _ramp(np.random.default_rng(2), (X[3], X[2], X[1], X[0], 4, 3))
    f = _make(hip, lat, prec, order, pad, lat.dev(v))
    want = hip.SpinorField(X, prec, order, pad=pad, device=DEV).set_logical(orc.lex_to_eo(v, X))
    assert np.array_equal(f.get_logical(), want.get_logical())
    assert torch.equal(_download(lat, f), _rounded(lat.dev(v), prec))
    if pad:
        assert bool(torch.isnan(torch.view_as_real(f.data)).any()) and np.all(np.isfinite(f.get_logical()))
    Uo = orc.extended_gauge_from_global(lat.U_lex, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    assert torch.equal(_gauge(hip, lat, prec).data, hip.GaugeField(X, (0, 0, 0, 0), prec, device=DEV).set_logical(Uo).data)


# ---- a. exact eigenpairs at every size --------------------------------------------------------------------------------------------
def _eig_vectors(lat):
    """9 .. 13 single-momentum vectors u = norm / sqrt(V) w_k (x) c: distinct momenta with h >= 0.6 and |a| >= 0.25 (so that neither
    lambda(H), lambda(M^dag M) nor v^dag M v is small against ||M||: the fp32 bounds are relative to them), all four w_k in turn (both
    signs of h), every other one normalised, the rest with norms 0.55 .. 2.45."""
    if "eig" not in lat.cache:
        X, V, rng = lat.X, lat.V, lat.rng_for("eig")
        nvec = 9 + SIZES.index(X) % 5 if X in SIZES else 9
        moms = pw.pick_momenta(rng, X, KAPPA, nvec, h_min=0.6, a_min=0.25)
        odd = list(range(1, nvec, 2))
        vecs = []
        for i, n in enumerate(moms):
            sign, w = pw.h_eigvecs(n, X, KAPPA)
            k = i % 4
            norm = 1.0 if i % 2 == 0 else 0.55 + 1.9 * odd.index(i) / (len(odd) - 1)
            assert i % 2 == 0 or abs(norm - 1.0) > 0.01
            u = norm / math.sqrt(V) * np.outer(w[:, k], _unit(rng))
            vecs.append(dict(n=n, u=u, norm=norm, sign=float(sign[k]), h=pw.h_of_p(n, X, KAPPA), t=lat.field([n], [u])))
        lat.cache["eig"] = vecs
    return lat.cache["eig"]


def _eval_cases():
    out = []
    for X in SIZES:
        for prec, order, pad in (STORAGES if X in FULL else [(8, 2, 0), (4, 4, 7)]):
            out.append((X, prec, order, pad))
    return out


@pytest.mark.parametrize("X,prec,order,pad", _eval_cases(), ids=_ids)
def test_compute_evals_exact_eigenpairs(hip, X, prec, order, pad, record_max):
    """lambda, sigma and the residual of computeEvals on exact eigenvectors, against the closed form.  The library's literal formula
    is lambda = v^dag A v / ||v|| (not ||v||^2): with A v = mu v, lambda_exact = mu ||v|| and r_exact = |lambda_exact - mu| ||v||, zero
    for the normalised vectors.  fp64 bounds: those of test_compute_evals (1e-12 relative on lambda, r <= 1e-12 ||A|| ||v|| where
    r_exact = 0, 1e-11 relative on r elsewhere).  fp32 storage: vectors and links are rounded to fp32 first, so the pairs are exact to
    rounding only: 1e-5 relative on lambda and |r - r_exact| <= 1e-5 ||A v|| (TOL[4]; a plane wave has the same modulus at every
    site, so the max-norm bound carries over to the 2-norm).  M and M^dag: the literal formula on the amplitudes with the analytic
    A v; no sigma."""
    lat = _lat(X)
    V = lat.V
    vecs = _eig_vectors(lat)
    gauge = _gauge(hip, lat, prec)
    fv = [_make(hip, lat, prec, order, pad, v["t"]) for v in vecs]
    before = [_pads(f) for f in fv]
    hmax = max(v["h"] for v in vecs)
    ops = pw.OPS if X in FULL else ("H", "MdagM")
    tag = "wilson_scale_evals_fp%d_" % (8 * prec)
    for op in ops:
        for mass in ((False, True) if op == "MdagM" else (False,)):
            sc = 0.25 / KAPPA ** 2 if mass else 1.0
            args = (fv, gauge, KAPPA, pw.OPS.index(op))
            lam, res, sig = hip.computeEvals(*args, massNormalization=mass)
            lam2, res2, sig2 = hip.computeEvals(*args, massNormalization=mass)
            assert np.array_equal(lam.view(np.float64), lam2.view(np.float64)) and np.array_equal(res, res2), (op, "two calls differ")
            assert np.all(np.isfinite(lam.view(np.float64))) and np.all(np.isfinite(res))
            assert (sig is None) == (op in ("M", "Mdag"))
            if sig is not None:
                assert np.array_equal(sig, sig2) and np.all(np.isfinite(sig))
            normA = sc * (hmax if op in ("H", "M", "Mdag") else hmax ** 2)
            for i, v in enumerate(vecs):
                where = (X, op, mass, i)
                if op in ("M", "Mdag"):
                    Au = pw.op_matrix(op, v["n"], X, KAPPA) @ v["u"]
                    lam_x = V * np.vdot(v["u"], Au) / v["norm"]
                    r_x = math.sqrt(V) * np.linalg.norm(lam_x * v["u"] - Au)
                    normAv = math.sqrt(V) * np.linalg.norm(Au)
                else:
                    mu = sc * (v["sign"] * v["h"] if op == "H" else v["h"] ** 2)
                    lam_x = mu * v["norm"]
                    r_x = abs(lam_x - mu) * v["norm"]
                    normAv = abs(mu) * v["norm"]
                    sig_x = lam_x if op == "H" else math.sqrt(lam_x)
                    dsig = abs(sig[i] - sig_x) / abs(sig_x)
                    record_max(tag + "sigma_rel", dsig)
                    assert dsig <= (1e-12 if prec == 8 else 1e-5), where + (sig[i], sig_x)
                    assert op != "H" or np.sign(sig[i]) == v["sign"], where
                dlam = abs(lam[i] - lam_x) / abs(lam_x)
                record_max(tag + "lambda_rel", dlam)
                if prec == 8:
                    assert dlam <= 1e-12, where + (lam[i], lam_x)
                    if r_x == 0.0:
                        record_max(tag + "residual_exact_over_normA", res[i] / (normA * v["norm"]))
                        assert res[i] <= 1e-12 * normA * v["norm"], where + (res[i],)
                    else:
                        record_max(tag + "residual_rel", abs(res[i] - r_x) / r_x)
                        assert abs(res[i] - r_x) <= 1e-11 * r_x, where + (res[i], r_x)
                else:
                    assert dlam <= 1e-5, where + (lam[i], lam_x)
                    record_max(tag + "residual_over_normAv", abs(res[i] - r_x) / normAv)
                    assert abs(res[i] - r_x) <= 1e-5 * normAv, where + (res[i], r_x, normAv)
    if "H" in ops:
        assert any(v["sign"] < 0 for v in vecs) and any(v["sign"] > 0 for v in vecs)
    for f, b, v in zip(fv, before, vecs):
        assert torch.equal(_pads(f), b), "computeEvals wrote outside the body of an eigenvector"
        assert torch.equal(_download(lat, f), _rounded(v["t"], prec)), "computeEvals changed an eigenvector"


# ---- b. the reductions alone, against the host -------------------------------------------------------------------------------------
def _ld_sum(x):
    return np.sum(x, dtype=np.longdouble)


@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("X", [(18, 18, 18, 46), (32, 32, 32, 32)], ids=_ids)
def test_reductions_against_the_host(hip, X, prec, record_max):
    """Random fields (no eigenvectors), links that are not unitary: w = H v from wilsonApply is read back and lambda = v^dag w / ||v||
    and r = ||lambda v - w|| of computeEvals are compared with sums of the same products accumulated in long double on the host.
    Bound on lambda: |lambda - lambda_ref| ||v|| <= 1e-12 ||v|| ||w||.  A lane of the kernel adds at most ceil(sites / 262144) 48 products,
    the tree has 8 levels, the final pass at most 1024 terms: at 32^4 at most 1224 roundings of 1.1e-16 on sum |v_i| |w_i| <= ||v|| ||w||,
    i.e. 1.4e-13 in the worst case.  r is compared with the host's value for the lambda the library returned, so that only the sum of
    squares and the roundings of lambda v - w differ: bound 1e-12 (||lambda v|| + ||w||)."""
    nvec = 2
    gen = torch.Generator(device=DEV).manual_seed(5 + prec)
    cdt = torch.complex128 if prec == 8 else torch.complex64
    gauge = hip.GaugeField(X, (0, 0, 0, 0), prec, device=DEV)
    gauge.data.copy_((0.4 * torch.randn(gauge.data.numel(), dtype=torch.complex128, device=DEV, generator=gen)).to(cdt))
    fv = [hip.SpinorField(X, prec, 2, device=DEV) for _ in range(nvec)]
    fw = [hip.SpinorField(X, prec, 2, device=DEV) for _ in range(nvec)]
    for f in fv:
        f.data.copy_(torch.randn(f.data.numel(), dtype=torch.complex128, device=DEV, generator=gen).to(cdt))
    op = hip.MUGIQ_EIG_OPERATOR_H
    hip.wilsonApply(fw, fv, gauge, KAPPA, op)
    lam, res, _ = hip.computeEvals(fv, gauge, KAPPA, op)
    _sync()
    for i in range(nvec):
        v, w = fv[i].data.cpu().numpy().astype(np.complex128), fw[i].data.cpu().numpy().astype(np.complex128)
        assert np.all(np.isfinite(w.view(np.float64))) and np.isfinite(lam[i].real) and np.isfinite(lam[i].imag) and np.isfinite(res[i])
        vr, vi, wr_, wi = v.real, v.imag, w.real, w.imag
        nv = np.sqrt(_ld_sum(vr * vr) + _ld_sum(vi * vi))
        nw = np.sqrt(_ld_sum(wr_ * wr_) + _ld_sum(wi * wi))
        dot_re = _ld_sum(vr * wr_) + _ld_sum(vi * wi)
        dot_im = _ld_sum(vr * wi) - _ld_sum(vi * wr_)
        dl = float(np.hypot(np.longdouble(lam[i].real) - dot_re / nv, np.longdouble(lam[i].imag) - dot_im / nv))
        record_max("wilson_scale_reduce_fp%d_lambda_over_normw" % (8 * prec), dl / float(nw))
        assert dl * float(nv) <= 1e-12 * float(nv) * float(nw), (X, i, lam[i], dot_re / nv, dot_im / nv)
        d = lam[i] * v - w
        r_ref = np.sqrt(_ld_sum(d.real * d.real) + _ld_sum(d.imag * d.imag))
        dr = abs(float(np.longdouble(res[i]) - r_ref))
        scale = abs(lam[i]) * float(nv) + float(nw)
        record_max("wilson_scale_reduce_fp%d_residual_over_scale" % (8 * prec), dr / scale)
        assert dr <= 1e-12 * scale, (X, i, res[i], float(r_ref))


# ---- c. the operator at full size ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,order,pad", STORAGES)
@pytest.mark.parametrize("X", [(24, 24, 24, 24), (32, 32, 32, 32)], ids=_ids)
def test_apply_on_sums_of_plane_waves(hip, X, prec, order, pad, record_max):
    """M psi, M^dag psi, H psi for 9 vectors of 3 momenta each (two partial blocks of the kernel's 4 or 8), and the first 5 alone."""
    lat = _lat(X)
    if "apply" not in lat.cache:
        rng = lat.rng_for("apply")
        cases = []
        for _ in range(9):
            moms = pw.pick_momenta(rng, X, KAPPA, 3)
            amps = [_ramp(rng) for _ in moms]
            want = {op: lat.dev(pw.applied(lat.g, X, moms, amps, KAPPA, op)) for op in ("M", "Mdag", "H")}
            cases.append((lat.field(moms, amps), want))
        lat.cache["apply"] = cases
    cases = lat.cache["apply"]
    gauge = _gauge(hip, lat, prec)
    src = [_make(hip, lat, prec, order, pad, s) for s, _ in cases]
    dst = [_new(hip, lat, prec, order, pad) for _ in cases]
    before = [_pads(f) for f in dst]
    for nvec in (9, 5):
        for op in ("M", "Mdag", "H"):
            for f in dst:
                _upload(lat, f, cases[0][0])                           # something else than the answer
            hip.wilsonApply(dst[:nvec], src[:nvec], gauge, KAPPA, pw.OPS.index(op))
            _sync()
            for r in range(nvec):
                e = _err(_download(lat, dst[r]), cases[r][1][op])
                record_max("wilson_scale_apply_fp%d" % (8 * prec), e)
                assert e < TOL[prec], (X, nvec, op, r, e)
    for f, b in zip(dst, before):
        assert torch.equal(_pads(f), b), "wilsonApply wrote outside the body of dst"
    if (prec, order, pad) == STORAGES[-1]:
        del lat.cache["apply"]                                        # 36 fields: the last storage of this lattice is done


@pytest.mark.parametrize("prec", [8, 4])
def test_apply_nonunitary_links_against_composed_displacements(hip, prec, record_max):
    """32^4, random links that are not unitary: the fused M against M composed on the device from eight calls of
    performCovariantDisplacementVector per vector (pinned to the oracle in tests/test_gpu_operators.py) and torch in fp64."""
    X, nvec = (32, 32, 32, 32), 3
    vcb = int(np.prod(X)) // 2
    gen = torch.Generator(device=DEV).manual_seed(11)
    cdt = torch.complex128 if prec == 8 else torch.complex64
    gauge = hip.GaugeField(X, (0, 0, 0, 0), prec, device=DEV)
    gauge.data.copy_((0.4 * torch.randn(gauge.data.numel(), dtype=torch.complex128, device=DEV, generator=gen)).to(cdt))
    src = [hip.SpinorField(X, prec, 2, device=DEV) for _ in range(nvec)]
    dst = [hip.SpinorField(X, prec, 2, device=DEV) for _ in range(nvec)]
    for f in src:
        f.data.copy_(torch.randn(f.data.numel(), dtype=torch.complex128, device=DEV, generator=gen).to(cdt))
    hip.wilsonApply(dst, src, gauge, KAPPA)
    fwd, bwd = hip.SpinorField(X, prec, 2, device=DEV), hip.SpinorField(X, prec, 2, device=DEV)
    gam = [torch.from_numpy(orc.gamma_dense(n).astype(np.complex128)).to(DEV) for n in wr.GAMMA_MU]
    one = torch.eye(4, dtype=torch.complex128, device=DEV)
    view = lambda f: f.data.view(2, 4, 3, vcb).to(torch.complex128)
    for s, d in zip(src, dst):
        acc = view(s).clone()
        for mu in range(4):
            hip.performCovariantDisplacementVector(fwd, s, gauge, mu, hip.DispSignPlus)
            hip.performCovariantDisplacementVector(bwd, s, gauge, mu, hip.DispSignMinus)
            acc -= KAPPA * (torch.einsum("st,ptcx->pscx", one - gam[mu], view(fwd)) + torch.einsum("st,ptcx->pscx", one + gam[mu], view(bwd)))
        e = _err(view(d), acc)
        record_max("wilson_scale_apply_nonunitary_fp%d" % (8 * prec), e)
        assert e < TOL[prec], (prec, e)


def test_apply_against_the_numpy_reference_at_24(hip, record_max):
    """The one comparison with tests/wilson_ref.py above 4096 sites: M on 2 random vectors, random SU(3) links, (24, 24, 24, 24)."""
    X = (24, 24, 24, 24)
    lat = _lat(X)
    rng = np.random.default_rng(24)
    U_lex = random_gauge_lex(rng, X)
    Uo = orc.extended_gauge_from_global(U_lex, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    gauge = hip.GaugeField(X, (0, 0, 0, 0), 8, device=DEV).set_logical(Uo)
    vs = [_ramp(rng, (2, lat.V // 2, 4, 3)) for _ in range(2)]
    src = [hip.SpinorField(X, 8, 2, device=DEV).set_logical(v) for v in vs]
    dst = [hip.SpinorField(X, 8, 2, device=DEV) for _ in vs]
    hip.wilsonApply(dst, src, gauge, KAPPA)
    _sync()
    for r in range(2):
        got = dst[r].get_logical()
        assert np.all(np.isfinite(got))
        e = rel_err(got, wr.wilson_M(vs[r], Uo, KAPPA, X))
        record_max("wilson_scale_apply_vs_numpy_24", e)
        assert e < TOL[8], (r, e)


# ---- d. the solver at every size ----------------------------------------------------------------------------------------------------
N_RHS = 11
K_OF_RHS = (3, 1, 4, 0, 2, 1, 4, 2, 3, 1, 2)                          # momenta per right-hand side; 0: b = 0.  Two blocks: 8 + 3.


def _solver_cases(lat):
    """per right-hand side: K momenta whose h^2 are pairwise >= 0.05 apart (checked here, before the library is called), random
    amplitudes; b and M^-1 b on the device"""
    if "solve" not in lat.cache:
        X, rng = lat.X, lat.rng_for("solve")
        cases = []
        for K in K_OF_RHS:
            if K == 0:
                zero = torch.zeros(lat.V, 12, dtype=torch.complex128, device=DEV)
                cases.append(dict(K=0, b=zero, x=zero, cond=1.0))
                continue
            moms = pw.pick_momenta(rng, X, KAPPA, K, h_min=0.2, h2_gap=0.05)
            hs = [pw.h_of_p(n, X, KAPPA) for n in moms]
            assert all(abs(a * a - b * b) >= 0.05 for i, a in enumerate(hs) for b in hs[:i]), hs
            amps = [_ramp(rng) for _ in moms]
            cases.append(dict(K=K, b=lat.field(moms, amps), x=lat.dev(pw.exact_solution(lat.g, X, moms, amps, KAPPA)), cond=max(hs) / min(hs)))
        lat.cache["solve"] = cases
    return lat.cache["solve"]


def _check_solution(X, cases, x_lex, info, record_max, tag):
    assert info.converged
    for r, c in enumerate(cases):
        got = x_lex[r]
        assert bool(torch.isfinite(torch.view_as_real(got)).all()) and np.isfinite(info.relres[r]), (X, r)
        if c["K"] == 0:
            assert info.iters[r] == 0 and info.relres[r] <= 1e-9 and not bool((got != 0).any()), (X, r, info.iters[r], info.relres[r])
            continue
        assert 1 <= info.iters[r] <= c["K"] + 1, (X, r, c["K"], info.iters[r])
        assert info.relres[r] < 1e-9, (X, r, info.relres[r])
        err = float(torch.linalg.vector_norm(got - c["x"]) / torch.linalg.vector_norm(c["x"]))
        record_max("wilson_scale_solve_%serr_rel" % tag, err)
        record_max("wilson_scale_solve_%srelres" % tag, info.relres[r])
        record_max("wilson_scale_solve_%siters_minus_K" % tag, float(info.iters[r] - c["K"]))
        assert err <= c["cond"] * info.relres[r] + 1e-12, (X, r, err, c["cond"], info.relres[r])


@pytest.mark.parametrize("order,pad", [(2, 0), (4, 7)])
@pytest.mark.parametrize("X", SIZES, ids=_ids)
def test_solve_known_iteration_counts_and_solutions(hip, X, order, pad, record_max):
    """11 right-hand sides of 1 .. 4 momenta (one zero), tol 1e-10: M^dag M has K distinct eigenvalues h(p)^2 on the Krylov space of
    M^dag b, so exact CG takes K iterations (one spare for rounding) and ends at the closed-form solution:
    ||x - x_exact|| <= (cond relres + 1e-12) ||x_exact||, cond = max h / min h of that right-hand side (x - x_exact = M^-1 (M x - b) and
    ||b|| <= max h ||x_exact||).  Vectors leave the active mask at different iterations.  Two runs are bitwise equal.  At
    (24, 24, 24, 24) the partitioned code path on one rank gives bitwise the same x, iters and relres."""
    lat = _lat(X)
    cases = _solver_cases(lat)
    gauge = _gauge(hip, lat, 8)
    fb = [_make(hip, lat, 8, order, pad, c["b"]) for c in cases]
    x, info = hip.wilsonSolve(fb, gauge, KAPPA, tol=1e-10, maxIter=50)
    x2, info2 = hip.wilsonSolve(fb, gauge, KAPPA, tol=1e-10, maxIter=50, x=[_new(hip, lat, 8, order, pad) for _ in fb])
    _sync()
    _check_solution(X, cases, [_download(lat, f) for f in x], info, record_max, "")
    assert np.array_equal(info.iters, info2.iters) and np.array_equal(info.relres, info2.relres)
    for a, b in zip(x, x2):
        assert _bits_equal(_download(lat, a), _download(lat, b))
    if pad:
        for f in x2:
            assert bool(torch.isnan(torch.view_as_real(_pad_view(f))).all()), "wilsonSolve wrote into the pad of x"
    for f, c in zip(fb, cases):
        assert torch.equal(_download(lat, f), c["b"]), "wilsonSolve changed b"
    if X == (24, 24, 24, 24):
        del x2
        force = (0, 0, 1, 1)
        comm = hip.GridComm((1, 1, 1, 1), device="cuda:0", force_partitioned=force)
        brd = [2 * f for f in force]
        Ue = orc.extended_gauge_from_global(lat.U_lex, (0, 0, 0, 0), (1, 1, 1, 1), brd)
        gp = hip.GaugeField(X, brd, 8, device=DEV).set_logical(Ue)
        xp, infop = hip.wilsonSolve(fb, gp, KAPPA, tol=1e-10, maxIter=50, comm=comm)
        _sync()
        assert infop.converged and np.array_equal(info.iters, infop.iters) and np.array_equal(info.relres, infop.relres)
        for a, b in zip(x, xp):
            assert _bits_equal(_download(lat, a), _download(lat, b)), "the partitioned path is not bitwise equal"


def _orthonormal_set(lat, count, key):
    """`count` orthonormal exact eigenvectors of H: distinct momenta, except that the last two pairs share a momentum with orthogonal
    w_k (x) c.  [(n, u, sigma, device field)]"""
    if key not in lat.cache:
        X, V, rng = lat.X, lat.V, lat.rng_for(key)
        moms = pw.pick_momenta(rng, X, KAPPA, count - 2, h_min=0.3)
        spec = [(n, i % 4) for i, n in enumerate(moms[:count - 4])] + [(moms[-2], 0), (moms[-2], 3), (moms[-1], 1), (moms[-1], 2)]
        out = []
        for n, k in spec:
            sign, w = pw.h_eigvecs(n, X, KAPPA)
            u = np.outer(w[:, k], _unit(rng)) / math.sqrt(V)
            out.append((n, u, float(sign[k]) * pw.h_of_p(n, X, KAPPA), lat.field([n], [u])))
        lat.cache[key] = (out, moms)
    return lat.cache[key]


@pytest.mark.parametrize("order", [2, 4])
def test_solve_deflated_start_at_32(hip, order, record_max):
    """12 exact eigenpairs (v_k, sigma_k = +-h) of H as the low-mode start.  b = g5 sum_k c_k v_k: M x = b has the solution
    sum_k c_k v_k / sigma_k, which the start vector already is: 0 iterations, x to 1e-12.  One right-hand side of a momentum outside
    the set still iterates and meets the bounds of the plain solver."""
    X = (32, 32, 32, 32)
    lat = _lat(X)
    V, rng = lat.V, np.random.default_rng(32)
    vecs, used = _orthonormal_set(lat, 12, "ortho12")
    gauge = _gauge(hip, lat, 8)
    fv = [_make(hip, lat, 8, order, 0, t) for _, _, _, t in vecs]
    g5 = orc.gamma_dense(15)
    cases, fields = [], []
    for picks in ([3], [0, 5, 9, 11], list(range(12))):
        c = _ramp(rng, (len(picks),))
        ns = [vecs[k][0] for k in picks]
        b = lat.field(ns, [ck * (g5 @ vecs[k][1]) for ck, k in zip(c, picks)], math.sqrt(V))
        xs = lat.field(ns, [ck / vecs[k][2] * vecs[k][1] for ck, k in zip(c, picks)], math.sqrt(V))
        cases.append((b, xs))
    out_n = next(n for n in pw.pick_momenta(rng, X, KAPPA, 20, h_min=0.3) if n not in used)
    amp = _ramp(rng)
    outside = dict(K=1, b=lat.field([out_n], [amp]), x=lat.dev(pw.exact_solution(lat.g, X, [out_n], [amp], KAPPA)), cond=1.0)
    fb = [_make(hip, lat, 8, order, 0, b) for b, _ in cases] + [_make(hip, lat, 8, order, 0, outside["b"])]
    x, info = hip.wilsonSolve(fb, gauge, KAPPA, fv, [s for _, _, s, _ in vecs], tol=1e-10, maxIter=50)
    _sync()
    assert info.converged
    for r, (b, xs) in enumerate(cases):
        e = _err(_download(lat, x[r]), xs)
        record_max("wilson_scale_solve_deflated_start_err", e)
        assert info.iters[r] == 0 and info.relres[r] < 1e-9 and e < 1e-12, (r, info.iters[r], info.relres[r], e)
    last = len(cases)
    sub = type(info)(info.iters[last:], info.relres[last:], info.converged)
    _check_solution(X, [outside], [_download(lat, x[last])], sub, record_max, "deflated_outside_")


# ---- e. projectVector ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,pad", [(2, 7), (4, 32)])
@pytest.mark.parametrize("X", [(18, 18, 18, 46), (32, 32, 32, 32)], ids=_ids)
def test_project_vector_analytic(hip, X, order, pad, record_max):
    """10 orthonormal vectors of the family; in = a combination of 4 of them plus 2 momenta outside the set: out is the 4-term part,
    1e-13 relative as test_project_vector."""
    lat = _lat(X)
    V, rng = lat.V, np.random.default_rng(7)
    vecs, used = _orthonormal_set(lat, 10, "ortho10")
    fv = [_make(hip, lat, 8, order, pad, t) for _, _, _, t in vecs]
    picks = [1, 4, 7, 9]
    c = _ramp(rng, (4,))
    inside_n, inside_u = [vecs[k][0] for k in picks], [ck * vecs[k][1] for ck, k in zip(c, picks)]
    outs = [n for n in pw.pick_momenta(rng, X, KAPPA, 20) if n not in used][:2]
    want = lat.field(inside_n, inside_u, math.sqrt(V))
    inp = lat.field(inside_n + outs, inside_u + [_ramp(rng) / math.sqrt(V) for _ in outs], math.sqrt(V))
    fin = _make(hip, lat, 8, order, pad, inp)
    out = _make(hip, lat, 8, order, pad, inp * 3.0)
    before = _pads(out)
    hip.projectVector(out, fin, fv)
    _sync()
    e = _err(_download(lat, out), want)
    record_max("wilson_scale_project", e)
    assert e < 1e-13, (X, order, e)
    assert torch.equal(_pads(out), before) and torch.equal(_download(lat, fin), inp)
