"""Device fields for the two-grid solver's GPU tests (tests/test_gpu_mg_solve.py, tests/test_gpu_mg_solve_scale.py): fp64 spinor fields
whose pads are NaN, so that a kernel that reads or writes a pad shows it, and comparisons of fields bit for bit."""
import torch

NAN = complex(float("nan"), float("nan"))


def bits(t):
    return t.view(torch.float64).view(torch.int64)


def same(a, b):
    return bool(torch.equal(bits(a.data), bits(b.data)))


def pads(f):
    return f.data.view(2, 12, f.stride)[:, :, f.volumeCB:] if f.order == 2 else f.data.view(2, 6, f.stride, 2)[:, :, f.volumeCB:]


def field(hip, X, v=None, order=2, pad=0):
    """a field holding v with NaN pads, or (v None) an output field: zero without pads, NaN everywhere with them"""
    f = hip.SpinorField(X, 8, order, pad)
    if v is not None:
        f.set_logical(v)
        if pad:
            pads(f)[...] = NAN
    elif pad:
        f.data.fill_(NAN)
    return f


def pads_are_nan(f):
    return bool(torch.isnan(pads(f).real).all()) and bool(torch.isnan(pads(f).imag).all())
