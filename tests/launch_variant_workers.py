"""Worker of test_gpu_launch_variants.py that needs a process group: one rank as its own neighbour (forced partitioning), the tile
kernels' workgroup orders on interior / boundary launches."""
import os

import numpy as np

import launch_variants as lv
from mp_workers import _global_problem, _init, _single_domain_reference


def tile_order_forced_worker(rank, world, port, family, G, force, entries, nev):
    """The OPT plan on one rank with `force` axes partitioned (the rank is its own neighbour): the column tiles of `family` launch
    once over the interior tiles along mu and once over the boundary tiles, so jtBegin != 0 and jtCount < nJT.  Every setting of
    lv.tile_settings(family) against the single-domain oracle (fp64, 1e-12: the driver's bound), on the device."""
    import torch
    from util import orc, momenta_p2_le
    dist = _init(rank, world, port)
    torch.cuda.set_device(0)
    import mugiq_amd as hip
    os.environ["MUGIQ_HIP_REFLECT"] = "0"                                   # both signs go through the kernels
    _, s, a, b = orc.parse_disp_entry_string(entries)
    ev_lex, U_lex, sg = _global_problem(G, nev, 4321)
    cprm, pos_g, _ = _single_domain_reference(orc, G, ev_lex, U_lex, sg, (s, a, b), momenta_p2_le(0), 1)
    ref_d = torch.from_numpy(pos_g).cuda()
    scale = float(np.abs(pos_g).max())
    comm = hip.GridComm((1, 1, 1, 1), device="cuda:0", force_partitioned=force)
    brd = [2 * f for f in force]
    U_loc = np.stack([orc.lex_to_eo(U_lex[mu], G) for mu in range(4)])
    gauge = hip.GaugeField(G, brd, 8).set_from_qdp_host(orc.gauge_to_qdp_host(U_loc), comm)
    f = [hip.SpinorField(G, 8, 2).set_logical(orc.lex_to_eo(v, G)) for v in ev_lex]
    want_family = {"tile32": hip.FUSED_FAMILY_TILE32, "tile32_regs": hip.FUSED_FAMILY_TILE32, "tile16": hip.FUSED_FAMILY_TILE16,
                   "mfma": hip.FUSED_FAMILY_MFMA_COLUMN}[family]
    first = None
    for tag, env in lv.tile_settings(family):
        for k in lv.TILE_SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        order_env = int(env["MUGIQ_HIP_TILE_ORDER"])
        seen = {"jtBegin": False, "partial": False, "bit0": False, "bit1": False}
        for i in range(cprm.nDispEntries):
            dirn, sign = orc.parse_displacement(cprm.dispString[i])
            if not force[dirn]:
                continue
            kv = list(range(cprm.dispStart[i], cprm.dispStop[i] + 1))
            form = hip.fusedForm(f[0], dirn, kv, partitioned=True)
            assert form["family"] == want_family, (tag, i, form)
            geo = lv.tile_geometry(G, dirn, form["tj"], form["lines"])
            for region in ("interior", "boundary"):
                jb, jc = lv.tile_range(region, True, sign == hip.DispSignPlus, geo["nJT"], max(kv), form["tj"])
                order = lv.tile_block_order(order_env, lv.TILE_FAMILIES[family][1], geo["nCC"] * jc)
                seen["jtBegin"] |= jb != 0 and jc > 0
                seen["partial"] |= 0 < jc < geo["nJT"]
                seen["bit0"] |= bool(order & 1) and jc >= 2 and geo["nCC"] >= 2
                seen["bit1"] |= bool(order & 2) and geo["nCC"] * jc >= 16
                print("forced %s %s entry %d %s: jtBegin %d jtCount %d of %d, nCC %d, nblocks %d (mod 8: %d), order bits %d"
                      % (family, tag, i, region, jb, jc, geo["nJT"], geo["nCC"], geo["nCC"] * jc, geo["nCC"] * jc % 8, order), flush=True)
        assert seen["jtBegin"] and seen["partial"], (tag, seen)
        assert seen["bit1"] == bool(order_env & 2), (tag, seen)
        assert seen["bit0"] == bool(order_env & lv.TILE_FAMILIES[family][1] & 1), (tag, seen)
        prm = hip.MugiqLoopParam(calcType=hip.LOOP_CALC_TYPE_OPT_KERNEL, doNonLocal=True, disp_entry=[], disp_str=s, disp_start=a,
                                 disp_stop=b, gauge=gauge)
        loop = hip.Loop_Mugiq(prm, f, sg, comm).setProfiling()
        loop.computeCoarseLoop()
        kinds = set(p["kind"] for p in loop.phases())
        assert {"entry_interior", "entry_boundary"} <= kinds, (tag, kinds)
        for i in range(cprm.nDispEntries):
            dirn, _ = orc.parse_displacement(cprm.dispString[i])
            want = (hip.ENTRY_KERNEL_MFMA_COLUMN if family == "mfma" else hip.ENTRY_KERNEL_VECTOR_TILE) if dirn else None
            assert want is None or loop.entryKernel(i) == want, (tag, i, loop.entryKernel(i))
        got = loop.dataPos_d.to(torch.complex128)
        err = float((got - ref_d).abs().max()) / scale
        print("forced %s %s: rel err %.3e, bitwise equal to %s: %s" % (family, tag, err, "order0",
              "-" if first is None else bool(torch.equal(got, first))), flush=True)
        assert err < 1e-12, (family, tag, err)
        if first is None:
            first = got.clone()
        loop.close()
    dist.barrier()
    dist.destroy_process_group()
