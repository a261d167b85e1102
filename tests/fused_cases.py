"""Bodies shared by the GPU tests of the fused displaced contraction (test_gpu_driver.py, test_gpu_launch_variants.py)."""
import numpy as np
import torch

from util import orc, random_gauge_lex, random_spinor_lex, sigmas


def path_links(hip, X, prec, U, dirn, sign, kmax):
    """W_1 .. W_kmax as FLOAT2 spinor fields on one periodic domain: E_k = D^k E_0, E_0 = the identity in (spin, colour)"""
    V = int(np.prod(X))
    E = [hip.SpinorField(X, prec, 2) for _ in range(kmax + 1)]
    ident = np.zeros((2, V // 2, 4, 3), dtype=np.complex128)
    for s in range(3):
        ident[:, :, s, s] = 1.0
    E[0].set_logical(ident)
    for k in range(1, kmax + 1):
        hip.performCovariantDisplacementVector(E[k], E[k - 1], U, dirn, sign)
    return E[1:]


def fused_two_domains_along_t(hip, order, G, tol, variants=(None,), apply=None):
    """Operator-level check of the fused kernel across a domain boundary: two domains along t emulated on one GPU, path links from
    E_k = D^k E_0 per domain, 3 ghost layers packed by pack_face_layers; "+t" and "-t", lengths 1 .. 3, every (slot, gamma) of both
    domains against the single-domain oracle, relative to the largest element of that (slot, gamma).
    variants / apply: the fused call is repeated for every v of variants after apply(v, a field of the local lattice) has run (the
    caller's switches and its assertions about the form the call takes); the fields and the reference are shared."""
    grid = (1, 1, 1, 2)
    l = (G[0], G[1], G[2], G[3] // 2)
    comm = (0, 0, 0, 1)
    brd = (0, 0, 0, 2)
    rng = np.random.default_rng(8)
    nev = 3
    ev_lex = [random_spinor_lex(rng, G) for _ in range(nev)]
    U_lex = random_gauge_lex(rng, G)
    sg = sigmas(nev)
    ranks = [(0, 0, 0, 0), (0, 0, 0, 1)]
    Vl, Vg = int(np.prod(l)), int(np.prod(G))
    for dispstr in ("+t", "-t"):
        dirn, sign = orc.parse_displacement(dispstr)
        cprm = orc.LoopComputeParam([dispstr], [1], [3])
        ref = orc.compute_loop_position_space([orc.lex_to_eo(v, G) for v in ev_lex], sg, cprm,
                                              orc.extended_gauge_from_global(U_lex, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0)), G)
        f = {r: [hip.SpinorField(l, 8, order).set_logical(orc.lex_to_eo(orc.local_block(v, r, grid), l)) for v in ev_lex] for r in ranks}
        Ue = {r: hip.GaugeField(l, brd, 8).set_logical(orc.extended_gauge_from_global(U_lex, r, grid, brd)) for r in ranks}
        high = 0 if sign == hip.DispSignPlus else 1
        # path links per rank (needs the depth-1 face of E_{k-1} from the neighbour at every step)
        E = {r: [hip.SpinorField(l, 8, 2) for _ in range(4)] for r in ranks}
        ident = np.zeros((2, Vl // 2, 4, 3), dtype=np.complex128)
        for s in range(3):
            ident[:, :, s, s] = 1.0
        for r in ranks:
            E[r][0].set_logical(ident)
        for k in range(1, 4):
            faces = {}
            for r in ranks:
                faces[r] = torch.zeros(24 * E[r][k - 1].face_cb(3), dtype=torch.complex128, device="cuda")
                hip.packFace(faces[r], E[r][k - 1], 3, high)
            for i, r in enumerate(ranks):
                E[r][k - 1].ghost[3][1 - high] = faces[ranks[1 - i]]
                hip.performCovariantDisplacementVector(E[r][k], E[r][k - 1], Ue[r], dirn, sign, comm)
        layers = {}
        for r in ranks:
            layers[r] = torch.zeros(nev * 3 * 24 * f[r][0].face_cb(3), dtype=torch.complex128, device="cuda")
            hip.packFaceLayers(layers[r], f[r], 3, high, 3)
        # the local block of every (slot, gamma) of the reference, in the even-odd order of the local lattice: [rank][3 * 16][Vl]
        exp = {}
        for r in ranks:
            rows = []
            for k in range(3):
                for ig in range(16):
                    gl = orc.eo_to_lex(ref[Vg * (16 * (1 + k) + ig):Vg * (16 * (1 + k) + ig + 1)].reshape(2, Vg // 2), G)
                    rows.append(orc.lex_to_eo(np.ascontiguousarray(orc.local_block(gl, r, grid)), l).reshape(Vl))
            exp[r] = np.stack(rows)
        for v in variants:
            if apply is not None:
                apply(v, f[ranks[0]][0])
            for i, r in enumerate(ranks):
                out = torch.zeros(3 * 16 * Vl, dtype=torch.complex128, device="cuda")
                hip.displacedLoopContractionFused(out, f[r], sg, E[r][1:], [1, 2, 3], dirn, sign, comm, layers[ranks[1 - i]], 3)
                got = out.cpu().numpy().reshape(48, Vl)
                err = np.abs(got - exp[r]).max(axis=1) / np.abs(exp[r]).max(axis=1)
                assert np.all(err < tol), (dispstr, r, v, divmod(int(np.argmax(~(err < tol))), 16), float(np.nanmax(err)))
