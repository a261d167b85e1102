"""Device fields in QUDA-native layouts, as plain torch buffers + the POD descriptors of the C ABI.

These classes play the role of quda::ColorSpinorField / cudaGaugeField *as seen by the hot path*:
a device pointer plus layout and geometry.  torch is used for device memory only.
"""
import ctypes

import numpy as np
import torch

from . import _lib

FLOAT2 = 2
FLOAT4 = 4


def _cdtype(precision):
    return torch.complex128 if precision == 8 else torch.complex64


def _np_cdtype(precision):
    return np.complex128 if precision == 8 else np.complex64


def spinor_native_index(order, parity, x_cb, s, c, stride, parity_offset):
    """Complex-element index of component (s, c) at (parity, x_cb); see MugiqHipSpinorField in mugiq_hip.h."""
    k = 3 * s + c
    if order == FLOAT2:
        return parity * parity_offset + k * stride + x_cb
    return parity * parity_offset + ((k // 2) * stride + x_cb) * 2 + (k % 2)


class SpinorField:
    """nSpin=4, nColor=3 full-site-subset field in FLOAT2 or FLOAT4 order (plus optional depth-1 ghost zones)."""

    def __init__(self, X, precision=8, order=FLOAT2, pad=0, device="cuda", data=None):
        self.X = tuple(int(x) for x in X)
        assert all(x > 0 and x % 2 == 0 for x in self.X), "local dims must be even"
        self.precision = int(precision)
        self.order = int(order)
        self.volumeCB = int(np.prod(self.X)) // 2
        self.stride = self.volumeCB + int(pad)
        self.parity_offset = 12 * self.stride
        self.device = torch.device(device)
        n = 2 * self.parity_offset
        if data is None:
            self.data = torch.zeros(n, dtype=_cdtype(precision), device=self.device)
        else:
            assert data.numel() == n and data.dtype == _cdtype(precision)
            self.data = data
        self.ghost = [[None, None] for _ in range(4)]

    def face_cb(self, dim):
        return self.volumeCB // self.X[dim]

    def alloc_ghost(self, dim, bnd):
        if self.ghost[dim][bnd] is None:
            self.ghost[dim][bnd] = torch.zeros(2 * 12 * self.face_cb(dim), dtype=self.data.dtype, device=self.device)
        return self.ghost[dim][bnd]

    def desc(self):
        d = _lib.SpinorDesc()
        d.data = self.data.data_ptr()
        d.precision = self.precision
        d.field_order = self.order
        d.nParity = 2
        d.volumeCB = self.volumeCB
        d.stride = self.stride
        for i in range(4):
            d.X[i] = self.X[i]
            for b in range(2):
                g = self.ghost[i][b]
                d.ghost[i][b] = g.data_ptr() if g is not None else None
        d.parity_offset = self.parity_offset
        return d

    # ---- host <-> device plumbing in the logical shape [2, volumeCB, 4, 3] -------------------------------
    def _index_table(self, vcb=None, stride=None, parity_offset=None):
        vcb = self.volumeCB if vcb is None else vcb
        stride = self.stride if stride is None else stride
        parity_offset = self.parity_offset if parity_offset is None else parity_offset
        p = np.arange(2).reshape(2, 1, 1, 1)
        x = np.arange(vcb).reshape(1, vcb, 1, 1)
        s = np.arange(4).reshape(1, 1, 4, 1)
        c = np.arange(3).reshape(1, 1, 1, 3)
        return spinor_native_index(self.order, p, x, s, c, stride, parity_offset)

    def set_logical(self, v):
        v = np.asarray(v)
        assert v.shape == (2, self.volumeCB, 4, 3)
        buf = np.zeros(2 * self.parity_offset, dtype=_np_cdtype(self.precision))
        buf[self._index_table()] = v.astype(buf.dtype)
        self.data.copy_(torch.from_numpy(buf))
        return self

    def get_logical(self):
        buf = self.data.cpu().numpy()
        return buf[self._index_table()]

    def set_ghost_logical(self, dim, bnd, zone):
        fcb = self.face_cb(dim)
        zone = np.asarray(zone)
        assert zone.shape == (2, fcb, 4, 3)
        buf = np.zeros(2 * 12 * fcb, dtype=_np_cdtype(self.precision))
        buf[self._index_table(fcb, fcb, 12 * fcb)] = zone.astype(buf.dtype)
        self.alloc_ghost(dim, bnd).copy_(torch.from_numpy(buf))

    def zone_to_logical(self, dim, zone_tensor):
        fcb = self.face_cb(dim)
        return zone_tensor.cpu().numpy()[self._index_table(fcb, fcb, 12 * fcb)]


class GaugeField:
    """Border-extended gauge field in native FLOAT2 order, 18 reals per link (what Displace builds at
    lib/displace.cpp:104-134 of the reference)."""

    def __init__(self, X, R=(0, 0, 0, 0), precision=8, pad=0, device="cuda"):
        self.X = tuple(int(x) for x in X)
        self.R = tuple(int(r) for r in R)
        self.XE = tuple(self.X[d] + 2 * self.R[d] for d in range(4))
        self.precision = int(precision)
        self.volumeExCB = int(np.prod(self.XE)) // 2
        self.stride = self.volumeExCB + int(pad)
        self.parity_offset = 36 * self.stride
        self.device = torch.device(device)
        self.data = torch.zeros(2 * self.parity_offset, dtype=_cdtype(precision), device=self.device)

    def desc(self):
        d = _lib.GaugeDesc()
        d.data = self.data.data_ptr()
        d.precision = self.precision
        for i in range(4):
            d.X[i] = self.X[i]
            d.R[i] = self.R[i]
        d.stride = self.stride
        d.parity_offset = self.parity_offset
        return d

    def set_from_qdp_host(self, qdp_links, comm=None):
        """Displace::createExtendedCudaGaugeField (lib/displace.cpp:70-134): `qdp_links` = 4 host arrays of the LOCAL
        lattice in QDP order (loopParams.gauge[4]); borders come from the neighbours through `comm` (a GridComm)."""
        import ctypes
        import torch
        arrs = [np.ascontiguousarray(a) for a in qdp_links]
        cpu_prec = 8 if arrs[0].dtype == np.float64 else 4
        ptrs = (ctypes.c_void_p * 4)(*[a.ctypes.data for a in arrs])
        d = self.desc()
        c = comm.c_struct() if comm is not None else None
        _lib.check(_lib.load().mugiq_hip_create_extended_gauge(
            ctypes.byref(d), ptrs, cpu_prec, ctypes.byref(c) if c is not None else None,
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return self

    @staticmethod
    def _comm_ptr(comm):
        c = comm.c_struct() if comm is not None else None
        return c, (ctypes.cast(ctypes.byref(c), ctypes.c_void_p) if c is not None else None)

    def exchangeBorders(self, comm=None):
        """Refresh the R-deep borders from the interior on the device (mugiq_hip_exchange_extended_gauge): neighbour slabs through
        `comm` (a GridComm) along its partitioned dimensions, a periodic wrap along the others."""
        d = self.desc()
        c, cp = self._comm_ptr(comm)
        _lib.check(_lib.load().mugiq_hip_exchange_extended_gauge(ctypes.byref(d), cp, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return self

    def stoutSmear(self, rho, nSteps, smearDims=3, comm=None, out=None):
        """nSteps stout steps (mugiq_hip_stout_smear; smearDims 3: spatial links and staples only, 4: all) into `out`, a new field of
        the same geometry unless one is given.  This field, whose borders must be valid, is not written.  Returns `out`."""
        if out is None:
            out = GaugeField(self.X, self.R, self.precision, pad=self.stride - self.volumeExCB, device=self.device)
        if not isinstance(out, GaugeField):
            raise _lib.MugiqHipError("stoutSmear: out must be a GaugeField")
        i, o = self.desc(), out.desc()
        c, cp = self._comm_ptr(comm)
        _lib.check(_lib.load().mugiq_hip_stout_smear(ctypes.byref(o), ctypes.byref(i), float(rho), int(nSteps), int(smearDims), cp,
                                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return out

    def plaquette(self, comm=None):
        """(mean, spatial, temporal) of Re tr P / 3 over all ranks of `comm` (mugiq_hip_plaquette); 1 for unit links."""
        d = self.desc()
        c, cp = self._comm_ptr(comm)
        plaq = (ctypes.c_double * 3)()
        _lib.check(_lib.load().mugiq_hip_plaquette(ctypes.byref(d), plaq, cp, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return plaq[0], plaq[1], plaq[2]

    def get_logical(self):
        d = np.arange(4).reshape(4, 1, 1, 1, 1)
        p = np.arange(2).reshape(1, 2, 1, 1, 1)
        x = np.arange(self.volumeExCB).reshape(1, 1, -1, 1, 1)
        r = np.arange(3).reshape(1, 1, 1, 3, 1)
        c = np.arange(3).reshape(1, 1, 1, 1, 3)
        idx = p * self.parity_offset + (d * 9 + r * 3 + c) * self.stride + x
        return self.data.cpu().numpy()[idx]

    def set_logical(self, U):
        """U: [4, 2, volExCB, 3, 3] (dir, parity, extended even-odd index, row, col)."""
        U = np.asarray(U)
        assert U.shape == (4, 2, self.volumeExCB, 3, 3)
        d = np.arange(4).reshape(4, 1, 1, 1, 1)
        p = np.arange(2).reshape(1, 2, 1, 1, 1)
        x = np.arange(self.volumeExCB).reshape(1, 1, -1, 1, 1)
        r = np.arange(3).reshape(1, 1, 1, 3, 1)
        c = np.arange(3).reshape(1, 1, 1, 1, 3)
        idx = p * self.parity_offset + (d * 9 + r * 3 + c) * self.stride + x
        buf = np.zeros(2 * self.parity_offset, dtype=_np_cdtype(self.precision))
        buf[idx] = U.astype(buf.dtype)
        self.data.copy_(torch.from_numpy(buf))
        return self


def clover_lower_index(i, j):
    """Position of entry (i, j), i > j, of a 6 x 6 block among its 15 strictly-lower ones (row by row); see MugiqHipCloverField."""
    return i * (i - 1) // 2 + j


class CloverField:
    """The clover term A(x) of the Wilson-clover operator on the local sites: two Hermitian 6 x 6 blocks per site, packed as 36 pairs
    of reals (MugiqHipCloverField in mugiq_hip.h).  The buffer is a complex tensor: one element = one pair."""

    def __init__(self, X, precision=8, pad=0, device="cuda"):
        self.X = tuple(int(x) for x in X)
        assert all(x > 0 and x % 2 == 0 for x in self.X), "local dims must be even"
        self.precision = int(precision)
        self.volumeCB = int(np.prod(self.X)) // 2
        self.stride = self.volumeCB + int(pad)
        self.parity_offset = 36 * self.stride
        self.device = torch.device(device)
        self.data = torch.zeros(2 * self.parity_offset, dtype=_cdtype(precision), device=self.device)

    def desc(self):
        d = _lib.CloverDesc()
        d.data = self.data.data_ptr()
        d.precision = self.precision
        for i in range(4):
            d.X[i] = self.X[i]
        d.volumeCB, d.stride, d.parity_offset = self.volumeCB, self.stride, self.parity_offset
        return d

    def compute(self, gauge, coeff, comm=None):
        """Fill the field from the border-extended gauge field (mugiq_hip_compute_clover); coeff = kappa * c_sw.  comm: the GridComm
        whose partitioned dimensions the gauge field must have a border along."""
        d, g = self.desc(), gauge.desc()
        c = comm.c_struct() if comm is not None else None
        _lib.check(_lib.load().mugiq_hip_compute_clover(
            ctypes.byref(d), ctypes.byref(g), float(coeff), ctypes.cast(ctypes.byref(c), ctypes.c_void_p) if c is not None else None,
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return self

    def _pair_index(self):
        """pair index of (parity, x_cb, block, pair p of the block): [2, volumeCB, 2, 18]"""
        p = np.arange(2).reshape(2, 1, 1, 1)
        x = np.arange(self.volumeCB).reshape(1, -1, 1, 1)
        b = np.arange(2).reshape(1, 1, 2, 1)
        q = np.arange(18).reshape(1, 1, 1, 18)
        return p * self.parity_offset + (b * 18 + q) * self.stride + x

    def set_logical(self, A):
        """A: dense blocks [2, volumeCB, 2, 6, 6] complex (parity, x_cb, block, row, column).  The real part of the diagonal and the
        strictly-lower triangle are stored; the upper triangle is implied (A is Hermitian)."""
        A = np.asarray(A)
        assert A.shape == (2, self.volumeCB, 2, 6, 6)
        pairs = np.zeros((2, self.volumeCB, 2, 18), dtype=np.complex128)
        for q in range(3):
            pairs[..., q] = A[..., 2 * q, 2 * q].real + 1j * A[..., 2 * q + 1, 2 * q + 1].real
        for i in range(1, 6):
            for j in range(i):
                pairs[..., 3 + clover_lower_index(i, j)] = A[..., i, j]
        buf = self.data.cpu().numpy()                                                       # pads stay as they are
        buf[self._pair_index()] = pairs.astype(buf.dtype)
        self.data.copy_(torch.from_numpy(buf))
        return self

    def get_logical(self):
        """dense blocks [2, volumeCB, 2, 6, 6] complex"""
        pairs = self.data.cpu().numpy()[self._pair_index()]
        A = np.zeros((2, self.volumeCB, 2, 6, 6), dtype=pairs.dtype)
        for q in range(3):
            A[..., 2 * q, 2 * q] = pairs[..., q].real
            A[..., 2 * q + 1, 2 * q + 1] = pairs[..., q].imag
        for i in range(1, 6):
            for j in range(i):
                A[..., i, j] = pairs[..., 3 + clover_lower_index(i, j)]
                A[..., j, i] = np.conj(A[..., i, j])
        return A


class CoarseField:
    """Coarse-grid colour-spinor (nSpin 2, nColor n_vec) in FLOAT2 order: a coarse eigenvector of the MG path."""

    def __init__(self, Xc, n_vec, precision=8, pad=0, device="cuda"):
        self.X = tuple(int(x) for x in Xc)
        assert all(x > 0 and x % 2 == 0 for x in self.X), "coarse dims must be even"
        self.n_vec = int(n_vec)
        self.precision = int(precision)
        self.volumeCB = int(np.prod(self.X)) // 2
        self.stride = self.volumeCB + int(pad)
        self.parity_offset = 2 * self.n_vec * self.stride
        self.device = torch.device(device)
        self.data = torch.zeros(2 * self.parity_offset, dtype=_cdtype(precision), device=self.device)

    def desc(self):
        d = _lib.CoarseDesc()
        d.data = self.data.data_ptr()
        d.precision, d.nSpin, d.nColor = self.precision, 2, self.n_vec
        d.volumeCB, d.stride, d.parity_offset = self.volumeCB, self.stride, self.parity_offset
        for i in range(4):
            d.X[i] = self.X[i]
        return d

    def set_logical(self, phi):
        """phi: [2, volCB_c, 2, n_vec]"""
        phi = np.asarray(phi)
        assert phi.shape == (2, self.volumeCB, 2, self.n_vec)
        p = np.arange(2).reshape(2, 1, 1, 1)
        x = np.arange(self.volumeCB).reshape(1, -1, 1, 1)
        s = np.arange(2).reshape(1, 1, 2, 1)
        c = np.arange(self.n_vec).reshape(1, 1, 1, -1)
        buf = np.zeros(2 * self.parity_offset, dtype=_np_cdtype(self.precision))
        buf[p * self.parity_offset + (s * self.n_vec + c) * self.stride + x] = phi.astype(buf.dtype)
        self.data.copy_(torch.from_numpy(buf))
        return self

    def get_logical(self):
        """[2, volCB_c, 2, n_vec]"""
        p = np.arange(2).reshape(2, 1, 1, 1)
        x = np.arange(self.volumeCB).reshape(1, -1, 1, 1)
        s = np.arange(2).reshape(1, 1, 2, 1)
        c = np.arange(self.n_vec).reshape(1, 1, 1, -1)
        return self.data.cpu().numpy()[p * self.parity_offset + (s * self.n_vec + c) * self.stride + x]


class CoarseOperator:
    """The explicit Galerkin coarse operator of a transfer (MugiqHipCoarseOperator in mugiq_hip.h): nine dense N x N matrices per coarse
    site, N = 2 n_vec -- Xd, then Y+_mu and Y-_mu for mu = x, y, z, t -- matrix-contiguous and without pad.
    eigsolve.computeCoarseOperator fills it from a finest-level transfer, eigsolve.computeCoarseOperatorCoarse from a coarse -> coarse
    transfer and the operator of the level above; kappa and hasClover are those of the last build."""

    def __init__(self, Xc, n_vec, precision=8, device="cuda"):
        self.X = tuple(int(x) for x in Xc)
        assert all(x > 0 and x % 2 == 0 for x in self.X), "coarse dims must be even"
        self.n_vec = int(n_vec)
        self.N = 2 * self.n_vec
        self.precision = int(precision)
        self.volumeCB = int(np.prod(self.X)) // 2
        self.kappa, self.hasClover = 0.0, False
        self.halo = None  # the CoarseHalo of a build on a process grid (eigsolve.computeCoarseOperatorGrid)
        self.device = torch.device(device)
        self.data = torch.zeros(2 * self.volumeCB * 9 * self.N * self.N, dtype=_cdtype(precision), device=self.device)

    def desc(self):
        d = _lib.CoarseOperatorDesc()
        d.data = self.data.data_ptr()
        d.precision, d.nVec, d.volumeCB = self.precision, self.n_vec, self.volumeCB
        d.kappa, d.hasClover = float(self.kappa), int(self.hasClover)
        for i in range(4):
            d.X[i] = self.X[i]
        return d

    def get_logical(self):
        """[2, volCB_c, 9, N, N] (parity, x_cb, matrix, row, column)"""
        return self.data.cpu().numpy().reshape(2, self.volumeCB, 9, self.N, self.N)


class CoarseHalo:
    """What M_c^dag of a CoarseOperator needs from the neighbour ranks of a process grid (MugiqHipCoarseHalo in mugiq_hip.h): per axis in
    `dims` the Y+_mu matrices of the backward neighbour's high face (Yback) and the Y-_mu matrices of the forward neighbour's low face
    (Yfwd), [2 faceCB, N, N] each in the header's face-site order.  eigsolve.computeCoarseOperatorGrid fills it."""

    def __init__(self, op, dims):
        self.X, self.n_vec, self.N, self.precision, self.volumeCB, self.device = op.X, op.n_vec, op.N, op.precision, op.volumeCB, op.device
        self.dims = tuple(1 if d else 0 for d in dims)
        self.faceCB = tuple(self.volumeCB // x for x in self.X)

        def face(d):
            return torch.zeros(2 * self.faceCB[d] * self.N * self.N, dtype=_cdtype(self.precision), device=self.device) if self.dims[d] else None
        self.Yback, self.Yfwd = [face(d) for d in range(4)], [face(d) for d in range(4)]

    def desc(self):
        d = _lib.CoarseHaloDesc()
        d.precision, d.nVec, d.volumeCB = self.precision, self.n_vec, self.volumeCB
        for i in range(4):
            d.X[i], d.dims[i] = self.X[i], self.dims[i]
            d.Yback[i] = self.Yback[i].data_ptr() if self.dims[i] else None
            d.Yfwd[i] = self.Yfwd[i].data_ptr() if self.dims[i] else None
        return d

    def get_logical(self, mu, forward):
        """[2, faceCB, N, N] (parity, face index, row, column) of Yfwd[mu] (forward) or Yback[mu]"""
        t = (self.Yfwd if forward else self.Yback)[mu]
        return t.cpu().numpy().reshape(2, self.faceCB[mu], self.N, self.N)


class Transfer:
    """One level of QUDA's Transfer as the hot path sees it: the block-orthonormal null vectors V on the finer grid of
    the level (packed vector index), the aggregate size and the spin blocking.  Finest level: the finer side is the
    fine lattice (4 spins x 3 colours, spin_block_size 2).  A coarse -> coarse level: fine_spin = 2, fine_color = n_vec of
    the next finer level, spin_block_size = 1."""

    def __init__(self, X, n_vec=24, geo_block_size=(4, 4, 4, 4), spin_block_size=2, precision=8, pad=0, device="cuda",
                 fine_spin=4, fine_color=3):
        self.X = tuple(int(x) for x in X)
        self.n_vec = int(n_vec)
        self.geo_block_size = tuple(int(b) for b in geo_block_size)
        self.spin_block_size = int(spin_block_size)
        self.fine_spin, self.fine_color = int(fine_spin), int(fine_color)
        self.precision = int(precision)
        self.volumeCB = int(np.prod(self.X)) // 2
        self.stride = self.volumeCB + int(pad)
        self.parity_offset = self.fine_spin * self.fine_color * self.n_vec * self.stride
        self.device = torch.device(device)
        self.V = torch.zeros(2 * self.parity_offset, dtype=_cdtype(precision), device=self.device)
        self.Xc = tuple(self.X[d] // self.geo_block_size[d] for d in range(4))

    def desc(self):
        d = _lib.TransferDesc()
        d.V = self.V.data_ptr()
        d.precision, d.nVec, d.spinBlockSize = self.precision, self.n_vec, self.spin_block_size
        d.stride, d.parity_offset = self.stride, self.parity_offset
        for i in range(4):
            d.X[i] = self.X[i]
            d.geoBlockSize[i] = self.geo_block_size[i]
        return d

    def set_logical(self, V):
        """V: [2, volCB, fine_spin, fine_color, n_vec]"""
        V = np.asarray(V)
        ns, nc = self.fine_spin, self.fine_color
        assert V.shape == (2, self.volumeCB, ns, nc, self.n_vec)
        p = np.arange(2).reshape(2, 1, 1, 1, 1)
        x = np.arange(self.volumeCB).reshape(1, -1, 1, 1, 1)
        s = np.arange(ns).reshape(1, 1, ns, 1, 1)
        c = np.arange(nc).reshape(1, 1, 1, nc, 1)
        j = np.arange(self.n_vec).reshape(1, 1, 1, 1, -1)
        buf = np.zeros(2 * self.parity_offset, dtype=_np_cdtype(self.precision))
        buf[p * self.parity_offset + ((nc * s + c) * self.n_vec + j) * self.stride + x] = V.astype(buf.dtype)
        self.V.copy_(torch.from_numpy(buf))
        return self

    def astype(self, precision, pad=None):
        """A new Transfer of the same geometry in `precision` (4 | 8) with V copied on the device (mugiq_hip_transfer_convert): one
        rounding on the store, no trip through the host.  pad: of the new V (default: this one's).  The fp32 hierarchy of mgSolveMixed is
        T32 = T.astype(4); op32 = computeCoarseOperator(T32, gauge, kappa, clover=...)."""
        out = Transfer(self.X, self.n_vec, self.geo_block_size, self.spin_block_size, int(precision), self.stride - self.volumeCB if pad is None else pad,
                       self.device, self.fine_spin, self.fine_color)
        d, s = out.desc(), self.desc()
        _lib.check(_lib.load().mugiq_hip_transfer_convert(ctypes.byref(d), ctypes.byref(s), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return out

    # ---- MG setup on the device (csrc/mg_setup.hip) ------------------------------------------------------------------------------
    def setVectors(self, vecs):
        """V(x; s, c, j) = vecs[j](x; s, c) for n_vec fine SpinorFields of either precision and order (mugiq_hip_transfer_set_vectors);
        a finest-level transfer only."""
        vecs = list(vecs)
        d = self.desc()
        _lib.check(_lib.load().mugiq_hip_transfer_set_vectors(ctypes.byref(d), desc_array(vecs) if vecs else None, len(vecs), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return self

    def getVector(self, j, out=None):
        """column j of V as a fine SpinorField (mugiq_hip_transfer_get_vector): `out`, or a new FLOAT2 field of the transfer's precision"""
        if out is None:
            out = SpinorField(self.X, self.precision, FLOAT2, device=self.device)
        d, o = self.desc(), out.desc()
        _lib.check(_lib.load().mugiq_hip_transfer_get_vector(ctypes.byref(o), ctypes.byref(d), int(j), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return out

    def setCoarseVectors(self, vecs):
        """V(x; s, c, j) = vecs[j](x; s, c) for n_vec CoarseFields (either precision) on the finer lattice of a coarse -> coarse transfer
        (spin_block_size 1), with fine_color colours (mugiq_hip_transfer_set_coarse_vectors)."""
        vecs = list(vecs)
        d = self.desc()
        _lib.check(_lib.load().mugiq_hip_transfer_set_coarse_vectors(ctypes.byref(d), coarse_desc_array(vecs) if vecs else None, len(vecs),
                                                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return self

    def getCoarseVector(self, j, out=None):
        """column j of the V of a coarse -> coarse transfer as a CoarseField on its finer lattice (mugiq_hip_transfer_get_coarse_vector):
        `out`, or a new field of the transfer's precision"""
        if out is None:
            out = CoarseField(self.X, self.fine_color, self.precision, device=self.device)
        d, o = self.desc(), out.desc()
        _lib.check(_lib.load().mugiq_hip_transfer_get_coarse_vector(ctypes.byref(o), ctypes.byref(d), int(j), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return out

    def blockOrthonormalize(self, nPasses=2, rankTol=0.0):
        """Orthonormalise the n_vec columns inside every (aggregate, coarse spin) block of V, in place: nPasses of classical Gram-Schmidt
        in fp64 (mugiq_hip_block_orthonormalize; the second pass is what restores orthonormality for ill-conditioned blocks).  Returns
        (minPivotRatio, zeroColumns); a minPivotRatio below rankTol raises MugiqHipError (status 1) with V filled all the same."""
        d, info = self.desc(), _lib.BlockOrthoInfo()
        _lib.check(_lib.load().mugiq_hip_block_orthonormalize(ctypes.byref(d), int(nPasses), float(rankTol), ctypes.byref(info), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return float(info.minPivotRatio), int(info.zeroColumns)

    def orthonormality(self):
        """max over the blocks of max |B^dag B - 1| (mugiq_hip_transfer_orthonormality)"""
        d, out = self.desc(), (ctypes.c_double * 1)()
        _lib.check(_lib.load().mugiq_hip_transfer_orthonormality(ctypes.byref(d), out, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return float(out[0])


def transfer_desc_array(transfers):
    arr = (_lib.TransferDesc * len(transfers))()
    for i, t in enumerate(transfers):
        arr[i] = t.desc()
    return arr


def coarse_desc_array(fields):
    arr = (_lib.CoarseDesc * len(fields))()
    for i, f in enumerate(fields):
        arr[i] = f.desc()
    return arr


def desc_array(fields):
    arr = (_lib.SpinorDesc * len(fields))()
    for i, f in enumerate(fields):
        arr[i] = f.desc()
    return arr
