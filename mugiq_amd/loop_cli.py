"""The loop options of the reference's drivers, under the same flag names (tests/test_params_mugiq.cpp:77-112), and the
`setLoopParam` filler of tests/loop.cpp:620-748 -- so a command line written for `tests/loop` carries over unchanged.

The reference's driver then runs QUDA's eigensolver.  For the fine operator that part is out of scope here (eigenvectors and
sigma are the INPUTS of the loop engine), so by default `main()` feeds the engine synthetic eigenvectors of the requested shape:

    python -m mugiq_amd.loop_cli --dim 8 8 8 8 --prec double --n-ev 4 \\
        --loop-ft-sign minus --loop-calc-type opt --momenta-filename momenta.txt \\
        --displace-entry-string "+z:1,2;-x:3" --loop-mom-space-filename loops.h5

The computeCoarse branch is covered: --eig-compute-coarse runs the MG setup on the gauge field, computes the lowest eigenpairs of MdagM
of the coarse operator on the device (QUDA's flag names: --eig-nConv, --eig-nKr, --eig-tol, --eig-poly-deg, --eig-amin, --eig-amax,
--eig-max-restarts, --mg-nvec, --mg-block-size), prints the printEvals lines and runs the MG ultra-local loop on the result:

    python -m mugiq_amd.loop_cli --dim 8 8 8 8 --eig-compute-coarse --eig-nConv 16 --eig-nKr 32 --mg-nvec 8 --mg-block-size 4 4 4 4

Multi-GPU: launch with torchrun and pass --gridsize gx gy gz gt (QUDA's --gridsize); one process per GPU.
"""
import argparse
import json
import os
import sys

import numpy as np

from .loop import (LOOP_CALC_TYPE_BASIC_KERNEL, LOOP_CALC_TYPE_BLAS, LOOP_CALC_TYPE_OPT_KERNEL, MugiqLoopParam, read_momenta_file,
                   parseDisplaceEntryString)

LOOP_FT_SIGN = {"plus": 1, "minus": -1}                                                     # loop_ft_sign_map
LOOP_CALC_TYPE = {"blas": LOOP_CALC_TYPE_BLAS, "opt": LOOP_CALC_TYPE_OPT_KERNEL, "basic": LOOP_CALC_TYPE_BASIC_KERNEL}
YES_NO = {"yes": True, "no": False}


def _choice(mapping):
    def conv(s):
        if s not in mapping:
            raise argparse.ArgumentTypeError("options are %s" % "/".join(mapping))
        return mapping[s]
    return conv


def _nonneg_int(s):
    try:
        v = int(s)
    except ValueError:
        raise argparse.ArgumentTypeError("expected an integer, got %r" % s)
    if v < 0:
        raise argparse.ArgumentTypeError("must not be negative")
    return v


def _finite_float(s):
    try:
        v = float(s)
    except ValueError:
        raise argparse.ArgumentTypeError("expected a number, got %r" % s)
    if not np.isfinite(v):
        raise argparse.ArgumentTypeError("must be finite")
    return v


def add_loop_option_mugiq(parser):
    """add_loop_option_mugiq (tests/test_params_mugiq.cpp:77-112): same names, same defaults (tests/test_params_mugiq.cpp:12-24)."""
    g = parser.add_argument_group("Loop-MuGiq", "Loop Options within MuGiq")
    g.add_argument("--momenta-filename", dest="mugiq_mom_filename", default="momenta.txt",
                   help="Filename with the momenta for Fourier Transform of the loop (default 'momenta.txt')")
    g.add_argument("--loop-gauge-filename", dest="loop_gauge_filename", default="",
                   help="Gauge field that will be used for non-local currents (default ''); here: a .npy file holding the "
                        "local QDP-order links [4][V*18] (tests/loop.cpp:88,106), or empty for a synthetic random SU(3) field")
    g.add_argument("--loop-ft-sign", dest="loop_ft_sign", type=_choice(LOOP_FT_SIGN), default=None,
                   help="Sign of the Loop Fourier Transform phase (default NULL, options are plus/minus)")
    g.add_argument("--loop-calc-type", dest="loop_calc_type", type=_choice(LOOP_CALC_TYPE), default=None,
                   help="Type of loop calculation (default NULL, options are blas/opt/basic)")
    g.add_argument("--loop-write-mom-space", dest="loop_write_mom_space_hdf5", type=_choice(YES_NO), default=True,
                   help="Whether to write momentum-space loop data in HDF5 format (default yes, options are yes/no)")
    g.add_argument("--loop-write-pos-space", dest="loop_write_pos_space_hdf5", type=_choice(YES_NO), default=False,
                   help="Whether to write position-space loop data in HDF5 format (default no, options are yes/no)")
    g.add_argument("--loop-do-momproj", dest="loop_doMomProj", type=_choice(YES_NO), default=True,
                   help="Whether to perform momentum projection (Fourier Transform) on the disconnected quark loop (default yes)")
    g.add_argument("--loop-do-nonlocal", dest="loop_doNonLocal", type=_choice(YES_NO), default=True,
                   help="Whether to compute quark loops for non-local currents, requires --displace-entry-string (default yes)")
    g.add_argument("--displace-entry-string", dest="disp_entry_string", default="",
                   help="Set displacement entries in the form, e.g: +z:1,8;-x:3;+y:2,5.")
    g.add_argument("--loop-mom-space-filename", dest="fname_mom_h5", default="",
                   help="Complete path to the HDF5 filename for the momentum-space loop data")
    g.add_argument("--loop-pos-space-filename", dest="fname_pos_h5", default="",
                   help="Complete path to the HDF5 filename for the position-space loop data")
    return g


class LoopParamError(ValueError):
    """what the reference reports through errorQuda in setLoopParam"""


def setLoopParam(args, gauge=None):
    """setLoopParam (tests/loop.cpp:620-748): checks, messages and field assignments in the reference's order."""
    if args.loop_ft_sign is None:
        raise LoopParamError("setLoopParam: Loop FT sign is undefined/unsupported. Options are --loop-ft-sign plus/minus")
    if args.loop_calc_type is None:
        raise LoopParamError("setLoopParam: Loop Calculation Type is undefined/unsupported. Options are --loop-calc-type blas/opt/basic")
    p = MugiqLoopParam()
    p.FTSign = args.loop_ft_sign
    p.calcType = args.loop_calc_type
    p.writeMomSpaceHDF5 = args.loop_write_mom_space_hdf5
    p.writePosSpaceHDF5 = args.loop_write_pos_space_hdf5
    p.doMomProj = args.loop_doMomProj
    p.doNonLocal = args.loop_doNonLocal
    if args.loop_write_mom_space_hdf5 and len(args.fname_mom_h5) == 0:
        raise LoopParamError("Got --loop-write-mom-space yes but no filename was given. Set option --loop-mom-space-filename")
    if args.loop_write_pos_space_hdf5 and len(args.fname_pos_h5) == 0:
        raise LoopParamError("Got --loop-write-pos-space yes but no filename was given. Set option --loop-pos-space-filename")
    p.fname_mom_h5 = args.fname_mom_h5
    p.fname_pos_h5 = args.fname_pos_h5
    if p.doNonLocal:                                                                        # tests/loop.cpp:656-705
        if len(args.disp_entry_string) == 0:
            raise LoopParamError("Got option '--loop-do-nonlocal yes' but option --displace-entry-string is not set!")
        p.disp_entry, p.disp_str, p.disp_start, p.disp_stop = parseDisplaceEntryString(args.disp_entry_string)
    p.gauge = gauge
    if not os.path.exists(args.mugiq_mom_filename):                                         # tests/loop.cpp:721-722
        raise LoopParamError("setLoopParam: Cannot open file %s to read momenta (option --momenta-filename)" % args.mugiq_mom_filename)
    try:
        p.momMatrix = read_momenta_file(args.mugiq_mom_filename)
    except ValueError as e:
        raise LoopParamError("setLoopParam: %s" % e)
    p.Nmom = len(p.momMatrix)
    return p


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m mugiq_amd.loop_cli", description="disconnected quark loops from low modes (MuGiq loop driver, MI355X)")
    # the lattice options of QUDA's command line that the loop path depends on
    ap.add_argument("--dim", type=int, nargs=4, default=[8, 8, 8, 8], metavar=("X", "Y", "Z", "T"), help="LOCAL lattice dimensions (QUDA --dim)")
    ap.add_argument("--gridsize", type=int, nargs=4, default=[1, 1, 1, 1], help="process grid (QUDA --gridsize); launch with torchrun")
    ap.add_argument("--prec", choices=["double", "single"], default="double", help="eigenvector / link precision")
    ap.add_argument("--loop-prec", choices=["same", "double"], default="same", help="precision of the loop buffers and FT (double over single = mixed mode)")
    ap.add_argument("--field-order", type=int, choices=[2, 4], default=None, help="QUDA field order of the eigenvectors (default: FLOAT2 for double, FLOAT4 for single)")
    ap.add_argument("--n-ev", type=int, default=4, help="number of (synthetic) eigenvectors")
    ap.add_argument("--seed", type=int, default=777)
    ap.add_argument("--kappa", type=float, default=0.12, help="hopping parameter of the Wilson operator (--check-evals)")
    ap.add_argument("--dslash-type", choices=["wilson", "clover"], default="wilson",
                    help="operator of --check-evals (QUDA --dslash-type): wilson, or clover = Wilson-clover with the term computed from the links")
    ap.add_argument("--clover-coeff", type=float, default=0.1, help="kappa * c_sw of the clover term (QUDA --clover-coeff)")
    ap.add_argument("--check-evals", action="store_true",
                    help="print the printEvals lines (lambda = v^dag MdagM v / ||v||, residual, sigma) of the eigenvectors the loop runs on; "
                         "needs the gauge field of a displaced loop")
    # stout smearing of the displacement links and the plaquette: this project's own flags, the reference has none
    ap.add_argument("--loop-gauge-stout-steps", type=_nonneg_int, default=0, metavar="N",
                    help="stout-smear the gauge field of the displacements N times before the loops run on it (default 0: as loaded); "
                         "--check-evals keeps the field as loaded")
    ap.add_argument("--loop-gauge-stout-rho", type=_finite_float, default=0.1, metavar="R", help="stout weight rho (default 0.1)")
    ap.add_argument("--loop-gauge-stout-dims", type=int, choices=[3, 4], default=3,
                    help="3: spatial links with spatial staples, t links unchanged (default); 4: every link")
    ap.add_argument("--compute-plaquette", action="store_true",
                    help="print the plaquette of the gauge field of the displacements, as the reference does after plaqQuda")
    add_loop_option_mugiq(ap)
    add_eig_option_mugiq(ap)
    return ap


def _random_su3_qdp(vcb, gen):
    """seeded random SU(3) links of the local lattice in QDP order, [4][V*18] reals"""
    import torch
    m = torch.complex(torch.randn(4 * 2 * vcb, 3, 3, dtype=torch.float64, device="cuda", generator=gen),
                      torch.randn(4 * 2 * vcb, 3, 3, dtype=torch.float64, device="cuda", generator=gen))
    r0 = m[:, 0] / torch.linalg.vector_norm(m[:, 0], dim=-1, keepdim=True)
    r1 = m[:, 1] - (r0.conj() * m[:, 1]).sum(-1, keepdim=True) * r0
    r1 = r1 / torch.linalg.vector_norm(r1, dim=-1, keepdim=True)
    r2 = torch.linalg.cross(r0.conj(), r1.conj())                                  # det = 1
    u = torch.stack([r0, r1, r2], dim=1).reshape(4, 2 * vcb, 9)
    return torch.view_as_real(u).reshape(4, 2 * vcb * 18).cpu().numpy()


def add_eig_option_mugiq(parser):
    """The eigensolver and MG flags of QUDA's command line that --eig-compute-coarse reads (tests/eigensolve.cpp:251-289 of the reference
    sets the matching QudaEigParam members; tests/loop.cpp:471,492 the MG ones).  Defaults: those of mugiq_hip_coarse_eig_param_default
    where this project has one (first guesses, not tuned), QUDA's names throughout."""
    g = parser.add_argument_group("Eigensolver", "the computeCoarse branch: MG setup and coarse eigensolve on the device")
    g.add_argument("--eig-compute-coarse", action="store_true",
                   help="compute the eigenvectors instead of using synthetic ones: MG setup on the gauge field, then the lowest eigenpairs of MdagM "
                        "of the coarse operator, then the MG ultra-local loop on them (one process, double precision)")
    g.add_argument("--eig-nConv", dest="eig_nConv", type=int, default=None, help="eigenpairs wanted (default: --n-ev)")
    g.add_argument("--eig-nKr", dest="eig_nKr", type=int, default=None, help="size of the search space, a multiple of 8 (default: nConv + 8 rounded up)")
    g.add_argument("--eig-tol", dest="eig_tol", type=_finite_float, default=1e-10, help="r_i <= tol x aMax")
    g.add_argument("--eig-poly-deg", dest="eig_poly_deg", type=int, default=20, help="degree of the Chebyshev filter")
    g.add_argument("--eig-amin", dest="eig_amin", type=_finite_float, default=0.0, help="lower end of the filter interval (<= 0: adaptive)")
    g.add_argument("--eig-amax", dest="eig_amax", type=_finite_float, default=0.0, help="upper end of the filter interval (<= 0: estimated)")
    g.add_argument("--eig-max-restarts", dest="eig_max_restarts", type=_nonneg_int, default=100, help="filter / orthonormalise / Rayleigh-Ritz rounds")
    g.add_argument("--mg-nvec", dest="mg_nvec", type=int, default=24, help="null vectors of the MG setup")
    g.add_argument("--mg-block-size", dest="mg_block_size", type=int, nargs=4, default=[4, 4, 4, 4], metavar=("X", "Y", "Z", "T"), help="aggregate")
    # a second coarse level: this project's own flag names (QUDA's per-level syntax is not mirrored, as for the two flags above)
    g.add_argument("--mg-coarse-nvec", dest="mg_coarse_nvec", type=int, default=None, metavar="N",
                   help="with --mg-coarse-block-size: a third level -- N vectors of a coarse -> coarse transfer (the lowest eigenvectors of MdagM "
                        "of the first coarse operator); the eigensolve then runs on the coarsest operator")
    g.add_argument("--mg-coarse-block-size", dest="mg_coarse_block_size", type=int, nargs=4, default=None, metavar=("X", "Y", "Z", "T"),
                   help="aggregate of the second level, on the first coarse lattice")
    return g


def compute_coarse_main(args):
    """--eig-compute-coarse: gauge field -> mgSetup -> coarse eigenpairs -> Loop_Mugiq(transfer=), nothing from outside.  Prints the
    reference's printEvals lines (the solver's theta in the second column) and one JSON line."""
    import torch
    from . import CloverField, GaugeField, Loop_Mugiq
    from .eigsolve import Eigsolve_Mugiq, MUGIQ_EIG_OPERATOR_MdagM, mgSetup, mgSetupCoarse
    if (args.mg_coarse_nvec is None) != (args.mg_coarse_block_size is None):
        raise SystemExit("--mg-coarse-nvec and --mg-coarse-block-size go together")
    if int(np.prod(args.gridsize)) != 1 or int(os.environ.get("WORLD_SIZE", "1")) != 1:
        raise SystemExit("--eig-compute-coarse runs on one process: the explicit coarse operator is a single-domain object")
    if args.prec != "double":
        raise SystemExit("--eig-compute-coarse needs --prec double: the MG setup and the eigensolve are fp64")
    X = tuple(args.dim)
    gen = torch.Generator(device="cuda").manual_seed(args.seed)
    gauge = GaugeField(X, (0, 0, 0, 0), 8)
    qdp = np.load(args.loop_gauge_filename, allow_pickle=False) if args.loop_gauge_filename else _random_su3_qdp(int(np.prod(X)) // 2, gen)
    gauge.set_from_qdp_host(qdp, None)
    clover = CloverField(X, 8).compute(gauge, args.clover_coeff, None) if args.dslash_type == "clover" else None
    transfer, coarseOp, setup = mgSetup(gauge, args.kappa, args.mg_nvec, tuple(args.mg_block_size), seed=args.seed, clover=clover)
    nConv = args.eig_nConv if args.eig_nConv is not None else args.n_ev
    nKr = args.eig_nKr if args.eig_nKr is not None else (nConv + 8 + 7) // 8 * 8
    levels = None
    if args.mg_coarse_nvec is not None:                                                     # a third level, from the second alone
        transfer1, coarseOp, setup1 = mgSetupCoarse(coarseOp, args.mg_coarse_nvec, tuple(args.mg_coarse_block_size), seed=args.seed)
        transfer = [transfer, transfer1]
        levels = {"mg_coarse_nvec": args.mg_coarse_nvec, "mg_coarse_block_size": list(args.mg_coarse_block_size),
                  "coarsest_dim": list(coarseOp.X), "setupCoarseOrthonormality": setup1.orthonormality,
                  "setupCoarseIters": setup1.eigensolve.iters, "setupCoarseOpBlocks": setup1.eigensolve.opBlocks}
    es = Eigsolve_Mugiq([], gauge, args.kappa, MUGIQ_EIG_OPERATOR_MdagM, clover=clover, transfer=transfer, coarseOp=coarseOp)
    sigma = es.computeEvecs(nConv, nKr, seed=args.seed, tol=args.eig_tol, polyDeg=args.eig_poly_deg, aMin=args.eig_amin, aMax=args.eig_amax,
                            maxIter=args.eig_max_restarts)
    es.computeEvals()
    es.printEvals()
    loop = Loop_Mugiq(MugiqLoopParam(gauge=gauge), es.eVecs, sigma, transfer=transfer)
    loop.computeCoarseLoop()
    norm = float(torch.linalg.vector_norm(loop.dataPos_d))
    info = es.lastEigensolve
    out = {"local_dim": list(args.dim), "mg_nvec": args.mg_nvec, "mg_block_size": list(args.mg_block_size), "nConv": nConv, "nKr": nKr,
           "iters": info.iters, "opBlocks": info.opBlocks, "aMax": info.aMaxUsed, "hostReads": info.hostReads,
           "hostDenseSeconds": info.hostDenseSeconds, "setupOrthonormality": setup.orthonormality, "nLoop": loop.nLoop,
           "loop_norm": norm, "data": "computed: MG setup on the device, coarse eigenpairs of MdagM, MG ultra-local loop"}
    if levels is not None:
        out.update(levels)
        out["data"] = "computed: MG setup on the device over two coarse levels, eigenpairs of MdagM of the coarsest operator, MG ultra-local loop"
    print(json.dumps(out))
    loop.close()
    return 0


def synthetic_inputs(args, rank=0, comm=None):
    """The stand-in for the eigensolver: seeded eigenvectors (N(0,1) components, unit norm), sigma_n = 0.01 + 0.002 n,
    and -- for displaced loops -- the gauge field (--loop-gauge-filename, or random SU(3) links)."""
    import torch
    from . import GaugeField, SpinorField
    prec = 8 if args.prec == "double" else 4
    order = args.field_order or (2 if prec == 8 else 4)
    X = tuple(args.dim)
    vcb = int(np.prod(X)) // 2
    cdt = torch.complex128 if prec == 8 else torch.complex64
    gen = torch.Generator(device="cuda").manual_seed(args.seed + 1000 * rank)
    gauge = None
    if args.loop_doNonLocal and len(args.disp_entry_string) > 0:
        brd = [2 if args.gridsize[d] > 1 else 0 for d in range(4)]                         # lib/displace.cpp:16
        gauge = GaugeField(X, brd, prec)
        if args.loop_gauge_filename:
            qdp = np.load(args.loop_gauge_filename, allow_pickle=False)                    # [4][V*18] reals, QDP order
        else:
            qdp = _random_su3_qdp(vcb, gen)
        gauge.set_from_qdp_host(qdp, comm)
    fields = []
    for n in range(args.n_ev):
        f = SpinorField(X, prec, order)
        w = torch.complex(torch.randn(f.data.numel(), dtype=torch.float64, device="cuda", generator=gen),
                          torch.randn(f.data.numel(), dtype=torch.float64, device="cuda", generator=gen))
        f.data.copy_((w / torch.linalg.vector_norm(w)).to(cdt))
        fields.append(f)
    sigma = 0.01 + 0.002 * np.arange(args.n_ev)
    return fields, sigma, gauge


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.eig_compute_coarse:
        return compute_coarse_main(args)
    import torch
    import torch.distributed as dist
    from . import GridComm, Loop_Mugiq

    world = int(os.environ.get("WORLD_SIZE", "1"))
    comm = None
    if world > 1:
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        dist.init_process_group(os.environ.get("MUGIQ_BACKEND", "nccl"))
        comm = GridComm(args.gridsize, device="cuda:%d" % torch.cuda.current_device())
    elif int(np.prod(args.gridsize)) != 1:
        raise SystemExit("--gridsize %s needs %d processes (torchrun)" % (args.gridsize, int(np.prod(args.gridsize))))
    rank = dist.get_rank() if world > 1 else 0
    fields, sigma, gauge = synthetic_inputs(args, rank, comm)
    # the links of the displacements: the loaded field, or a stout-smeared copy of it (the operator of --check-evals keeps the loaded one)
    loop_gauge = gauge
    if args.loop_gauge_stout_steps > 0 or args.compute_plaquette:
        if gauge is None:
            raise SystemExit("--loop-gauge-stout-steps / --compute-plaquette need a gauge field: set --loop-do-nonlocal yes and --displace-entry-string")

        def print_plaquette(g):
            plaq = g.plaquette(comm)
            if rank == 0:
                print("Computed plaquette is %e (spatial = %e, temporal = %e)" % tuple(plaq), file=sys.stderr)   # tests/loop.cpp:898
        print_plaquette(gauge)
        if args.loop_gauge_stout_steps > 0:
            loop_gauge = gauge.stoutSmear(args.loop_gauge_stout_rho, args.loop_gauge_stout_steps, args.loop_gauge_stout_dims, comm)
            print_plaquette(loop_gauge)
    prm = setLoopParam(args, loop_gauge)
    if args.loop_prec == "double":
        prm.loopPrecision = 8

    if args.check_evals:
        from .eigsolve import Eigsolve_Mugiq, MUGIQ_EIG_OPERATOR_MdagM
        if gauge is None:
            raise SystemExit("--check-evals needs a gauge field: set --loop-do-nonlocal yes and --displace-entry-string")
        clover = None
        if args.dslash_type == "clover":
            from . import CloverField
            clover = CloverField(gauge.X, gauge.precision).compute(gauge, args.clover_coeff, comm)
        es = Eigsolve_Mugiq(fields, gauge, args.kappa, MUGIQ_EIG_OPERATOR_MdagM, comm, clover=clover)
        es.computeEvals()
        es.printEvals(file=sys.stderr)
    loop = Loop_Mugiq(prm, fields, sigma, comm)
    if rank == 0:
        loop.printLoopComputeParams(lambda line: print(line, file=sys.stderr))
    loop.computeCoarseLoop()
    if prm.doMomProj and prm.writeMomSpaceHDF5:
        loop.writeLoopsHDF5()
    if rank == 0:
        print(json.dumps({"local_dim": list(args.dim), "gridsize": args.gridsize, "n_ev": args.n_ev, "prec": args.prec,
                          "field_order": fields[0].order, "nLoop": loop.nLoop, "nData": loop.nData, "Nmom": prm.Nmom,
                          "calcType": prm.calcType, "FTSign": prm.FTSign,
                          "mom_space_file": prm.fname_mom_h5 if (prm.doMomProj and prm.writeMomSpaceHDF5) else None,
                          "data": "synthetic eigenvectors (seeded N(0,1), unit norm), sigma_n = 0.01 + 0.002 n"}))
    loop.close()
    if world > 1:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
