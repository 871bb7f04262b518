"""sgVAMP command line -- drop-in for the reference's src/main.py.

Same flags, defaults, validation messages, log lines and output files
({out}/{name}.bim, {name}_xhat_it_{it}.bin, {name}_r1_cohort_{k}_it_{it}.bin,
{name}_cohort_{k}.csv, {name}_metrics.csv).  Differences:

* one process per GPU instead of one MPI rank per cohort: a single process
  handles all K cohorts (python main.py ...); ``--gpus G`` starts G local
  ranks (launch.py) and the LD blocks are sharded over them.  The reference's
  own launch (mpirun -np K python main.py ..., src/main.py:16-18) also works:
  its K processes become K GPU ranks of ONE job (comm.launch_from_env maps
  Open MPI / Hydra / srun ranks; rank 0 alone writes the shared files), not K
  copies of it;
* --seed (extension): seeds the Hutchinson probes per cohort, RandomState(seed+k)
  (the reference draws from the unseeded global RNG, src/sgvamp.py:326);
* --posterior last|all, --pip-threshold (extensions): per-marker posterior
  files {name}_pip_it_{it}.bin, {name}_lodds_it_{it}.bin, {name}_postvar_it_{it}.bin
  and {name}_posterior.csv (sgvamp.VAMP's docstring); off by default;
* --bim-files may be omitted when every cohort has the same marker order;
* LD may also be given as a block manifest (*.blocks.json, see ldio.py);
* LD may be a genotype panel: an --ld-files entry ending in .bed (PLINK 1
  .bed/.bim/.fam) is turned into LD blocks on the device, each rank reading only
  its own blocks' rows.  The blocks come from --ld-block-size n (equal blocks,
  the last shorter) or --ld-blocks FILE (one size per line); exactly one of the
  two is required.  With --bim-files the panel's rows are matched to the merged
  marker order by variant id (ids only, no allele reconciliation, as the
  reference matches); without, the panel's own order is used.  --ld-window W
  (a positive number of markers of that order) keeps only the LD within W
  markers of the diagonal inside each block: the blocks -- the chromosomes or
  segments the window does not cross -- are then formed as packed bands on the
  device, cut into coupled pieces like any windowed LD (sgvamp.BAND_PIECE).
  Truncated LD need not be positive semi-definite (as with PLINK's --ld-window);
  --s is the remedy.  It needs packed LD storage (--ld-packing on, the default).
  --ld-window-kb X / --ld-window-cm X limit the LD by distance instead, by the
  .bim's base-pair or cM column (with --ld-window as well both limits apply);
  --ld-taper triangle multiplies the LD of two markers d apart by 1 - d / D, D
  the one window given, which keeps the windowed LD positive semi-definite, so
  --s 0 works.  --ld-chr-blocks makes one LD block per chromosome of the .bim (a
  third way to give the blocks): positions restart at a chromosome, so a distance
  window must not cross one.  --ld-form factor keeps every LD block as its 2-bit
  genotype rows and applies R p as G (G^T p) in every LD pass instead of forming
  and storing R (exactly positive semi-definite, 2 bits per genotype: a whole
  chromosome as one unwindowed block fits one GPU); every --ld-files entry must
  then be a .bed, and no window, taper, --ld-precision f32 or --ld-packing off
  applies.  The default, --ld-form stored, is the run without the flag.
"""
import argparse
import logging
import math
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from comm import world_from_env  # noqa: E402
from ldio import load_bed_ld, load_ld, load_plink_ld_all, load_r, load_true_signal  # noqa: E402
from ldio import merge_bims  # noqa: E402
from sgvamp import BlockLD  # noqa: E402
from sgvamp import VAMP  # noqa: E402
from sgvamp import check_pip_threshold  # noqa: E402


def build_parser():
    # src/main.py:27-50
    parser = argparse.ArgumentParser()
    parser.add_argument("-ld_files", "--ld-files", help="Path to LD matrices in .npz files, separated by comma ")
    parser.add_argument("-r_files", "--r-files", help="Path to XTy .npy files separated by comma")
    parser.add_argument("-true_signal_file", "--true-signal-file", help="Path to true signal .npy file", default=None)
    parser.add_argument("-out_dir", "--out-dir", help="Output directory")
    parser.add_argument("-out_name", "--out-name", help="Output file name")
    parser.add_argument("-N", "--N", help="Number of samples in each cohort, saparated by comma")
    parser.add_argument("-M", "--M", help="Number of markers in each cohort, separated by comma")
    parser.add_argument("-K", "--K", help="Number of cohorts", default=1)
    parser.add_argument("-L", "--L", help="Number of prior mixture components", default=2)
    parser.add_argument("-iterations", "--iterations", help="Number of iterations", default=10)
    parser.add_argument("-prior_vars", "--prior-vars", help="Prior mixture variances of different cohorts", default="0,1")
    parser.add_argument("-prior_probs", "--prior-probs", help="Prior mixture probabilites of different cohorts", default="0.99,0.01")
    parser.add_argument("-gamw", "--gamw", help="Initial noise precision", default=5)
    parser.add_argument("-gam1", "--gam1", help="Initial signal precision", default=0.000001)
    parser.add_argument("-lmmse_damp", "--lmmse-damp", help="Use LMMSE damping", default=False)
    parser.add_argument("-learn_gamw", "--learn-gamw", help="Learn or fix gamw", default=True)
    parser.add_argument("-rho", "--rho", help="Damping factor rho", default=0.5)
    parser.add_argument("-cg_maxit", "--cg-maxit", help="CG max iterations", default=500)
    parser.add_argument("-s", "--s", help="Rused = (1-s) * R + s * Id", default=0.0)
    parser.add_argument("-prior_update", "--prior-update", help="Learning prior probabilities", default="em")
    parser.add_argument("-update_prior_from", "--update-prior-from", help="Learn prior probabilities from specific iteration onwards", default=1)
    parser.add_argument("-em_prior_maxit", "--em-prior-maxit", help="Maximal number of iterations that prior-learning EM is allowed to perform", default=100)
    parser.add_argument("-bim_files", "--bim-files", help="Path to files containing list of snps", default=None)
    # extensions
    parser.add_argument("--seed", help="Seed of the Hutchinson probes (RandomState(seed + k))", default=None)
    parser.add_argument("--device", help="HIP device (default: the node-local rank)", default=None)
    parser.add_argument("--gpus", help="GPU ranks to start on this node (default: the launcher's "
                        "world size, else 1)", default=None)
    parser.add_argument("--ld-precision", choices=["f64", "f32"], default="f64",
                        help="Element type packed LD blocks are stored in: f32 rounds R once, at load, to the nearest f32, half the LD memory; all arithmetic stays f64 (the exact f64 solve of R perturbed by <= 2^-24 relative per entry)")
    parser.add_argument("--posterior", choices=["none", "last", "all"], default="none",
                        help="Per-marker posterior files of the last or of all iterations: <name>_pip_it_<it>.bin (posterior inclusion probability), <name>_lodds_it_<it>.bin (log posterior odds of inclusion, finite in the tails where 1 - pip underflows), <name>_postvar_it_<it>.bin (posterior variance on the xhat file's scale squared), and <name>_posterior.csv (it, sum_pip, sum_postvar, n_pip_ge_thr); they are the posterior at that iteration's r1, gam1 and prior, whereas xhat is the damped mean (rho); none writes no new file")
    parser.add_argument("--pip-threshold", type=pip_threshold_arg, default=0.95,
                        help="Threshold of the posterior.csv count n_pip_ge_thr (markers with pip >= it), a probability in [0, 1]; used with --posterior last or all")
    parser.add_argument("--ld-block-size", default=None,
                        help="With a .bed LD source: LD blocks of this many markers (the last one shorter)")
    parser.add_argument("--ld-blocks", default=None,
                        help="With a .bed LD source: file listing the LD block sizes, one per line")
    parser.add_argument("--ld-window", default=None,
                        help="With a .bed LD source: keep only the LD between markers at most this many markers apart (in the run's marker order, inside each LD block) and store the blocks as packed bands formed on the device; a window does not preserve positive semi-definiteness, --s is the remedy")
    parser.add_argument("--ld-window-kb", default=None,
                        help="With a .bed LD source: keep only the LD between markers at most this many kilobases apart by the .bim's base-pair column (inside each LD block, where the positions must not decrease); combines with --ld-window, both limits then apply; stored as packed bands as wide as the farthest reach")
    parser.add_argument("--ld-window-cm", default=None,
                        help="With a .bed LD source: as --ld-window-kb, in centimorgans of the .bim's genetic-position column")
    parser.add_argument("--ld-taper", choices=["none", "triangle"], default="none",
                        help="With exactly one of --ld-window / --ld-window-kb / --ld-window-cm: triangle multiplies the LD of two markers a distance d apart by 1 - d / D (D the window; W + 1 markers for --ld-window W), which keeps the windowed LD positive semi-definite, so --s 0 works")
    parser.add_argument("--ld-chr-blocks", action="store_true",
                        help="With a .bed LD source: one LD block per run of equal chromosome code in the run's marker order (instead of --ld-block-size / --ld-blocks)")
    parser.add_argument("--ld-form", choices=["stored", "factor"], default="stored",
                        help="With .bed LD sources: stored (the default) forms and stores each LD block R_b; factor keeps the block's 2-bit genotype rows on the device and applies R_b p as G_b (G_b^T p) in every LD pass: exactly positive semi-definite, about 2 bits per genotype instead of 4 bytes per pair of markers, no window needed for a chromosome-sized block; takes no window, taper, --ld-precision f32 or --ld-packing off")
    parser.add_argument("--ld-packing", choices=["on", "off"], default="on",
                        help="Packed storage of symmetric LD blocks (on, the default) or full dense squares (off)")
    return parser


def check_bed_flags(parser, args):
    """A .bed LD source needs exactly one of --ld-block-size / --ld-blocks /
    --ld-chr-blocks; the flags mean nothing without one."""
    bed = any(p.endswith(".bed") for p in (args.ld_files or "").split(","))
    given = (args.ld_block_size is not None) + (args.ld_blocks is not None)
    if args.ld_chr_blocks:
        if not bed:
            parser.error("--ld-chr-blocks applies to a .bed LD source only")
        if given:
            parser.error("--ld-chr-blocks, --ld-block-size and --ld-blocks exclude each other: give exactly one")
    if bed and given == 0 and not args.ld_chr_blocks:
        parser.error("a .bed LD source needs its LD blocks: give --ld-block-size n or --ld-blocks FILE")
    if given == 2:
        parser.error("--ld-block-size and --ld-blocks exclude each other: give exactly one")
    if given and not bed:
        parser.error("--ld-block-size / --ld-blocks apply to a .bed LD source only")
    if args.ld_block_size is not None:
        try:
            ok = int(args.ld_block_size) >= 1
        except ValueError:
            ok = False
        if not ok:
            parser.error("--ld-block-size must be a positive integer, not %r" % (args.ld_block_size,))
    if args.ld_window is not None:
        if not bed:
            parser.error("--ld-window applies to a .bed LD source only")
        try:
            ok = int(args.ld_window) >= 1
        except ValueError:
            ok = False
        if not ok:
            parser.error("--ld-window must be a positive integer (markers), not %r" % (args.ld_window,))
        if args.ld_packing == "off":
            parser.error("--ld-window stores packed bands: it cannot be combined with --ld-packing off")
    for flag, val in (("--ld-window-kb", args.ld_window_kb), ("--ld-window-cm", args.ld_window_cm)):
        if val is None:
            continue
        if not bed:
            parser.error("%s applies to a .bed LD source only" % flag)
        try:
            ok = math.isfinite(float(val)) and float(val) > 0
        except ValueError:
            ok = False
        if not ok:
            parser.error("%s must be a positive number, not %r" % (flag, val))
        if args.ld_packing == "off":
            parser.error("%s stores packed bands: it cannot be combined with --ld-packing off" % flag)
    if args.ld_window_kb is not None and args.ld_window_cm is not None:
        parser.error("--ld-window-kb and --ld-window-cm exclude each other: give one distance")
    if args.ld_taper != "none":
        windows = sum(w is not None for w in (args.ld_window, args.ld_window_kb, args.ld_window_cm))
        if not bed:
            parser.error("--ld-taper applies to a .bed LD source only")
        if windows != 1:
            parser.error("--ld-taper needs exactly one of --ld-window / --ld-window-kb / "
                         "--ld-window-cm as its distance: %d given" % windows)
        if args.ld_packing == "off":
            parser.error("--ld-taper stores packed bands: it cannot be combined with --ld-packing off")


def check_ld_form(parser, args):
    """--ld-form factor: every LD source a .bed, no stored-form option with it."""
    if args.ld_form != "factor":
        return
    paths = (args.ld_files or "").split(",")
    other = [p for p in paths if not p.endswith(".bed")]
    if other:
        parser.error("--ld-form factor needs a .bed LD source for every cohort: %s is not one"
                     % other[0])
    for flag, given in (("--ld-window", args.ld_window is not None),
                        ("--ld-window-kb", args.ld_window_kb is not None),
                        ("--ld-window-cm", args.ld_window_cm is not None),
                        ("--ld-taper", args.ld_taper != "none")):
        if given:
            parser.error("--ld-form factor applies each LD block whole: it cannot be combined "
                         "with %s" % flag)
    if args.ld_precision == "f32":
        parser.error("--ld-form factor stores no R: it cannot be combined with --ld-precision f32")
    if args.ld_packing == "off":
        parser.error("--ld-form factor stores no R: it cannot be combined with --ld-packing off")


def pip_threshold_arg(text):
    """argparse type of --pip-threshold: a float in [0, 1]."""
    try:
        return check_pip_threshold(text)
    except ValueError:
        raise argparse.ArgumentTypeError("%r is not a probability in [0, 1]" % (text,))


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    check_bed_flags(parser, args)
    check_ld_form(parser, args)
    if argv is None:            # command line: --gpus N starts the ranks (before any GPU call)
        from launch import relaunch

        rc = relaunch(None if args.gpus is None else int(args.gpus))
        if rc is not None:
            sys.exit(rc)
    comm = world_from_env()
    rank = comm.Get_rank()
    logging.basicConfig(format="%(message)s", level=logging.DEBUG)   # main.py:21
    if rank == 0:
        logging.info(" ### VAMP for summary statistics ###\n")

    # main.py:54-97
    ld_fpaths, r_fpaths = args.ld_files, args.r_files
    true_signal_fpath = args.true_signal_file
    out_dir, out_name = args.out_dir, args.out_name
    Ms, Ns = args.M, args.N
    iterations = int(args.iterations)
    K = int(args.K)
    L = int(args.L)
    prior_vars, prior_probs = args.prior_vars, args.prior_probs
    gamw = float(args.gamw)
    gam1 = float(args.gam1)
    rho = float(args.rho)
    lmmse_damp = bool(int(args.lmmse_damp))
    learn_gamw = bool(int(args.learn_gamw))
    cg_maxit = int(args.cg_maxit)
    s = float(args.s)
    prior_update = args.prior_update
    update_prior_from = int(args.update_prior_from)
    em_prior_maxit = int(args.em_prior_maxit)
    bim_fpaths = args.bim_files
    seed = None if args.seed is None else int(args.seed)

    ld_fpaths_list = ld_fpaths.split(",")
    r_fpaths_list = r_fpaths.split(",")
    N_list = [int(n) for n in Ns.split(",")]
    M_list = [int(m) for m in Ms.split(",")]
    Nt = sum(N_list)
    prior_vars_list = [float(x) for x in prior_vars.split(",")]
    prior_probs_list = [float(x) for x in prior_probs.split(",")]
    if len(ld_fpaths_list) != K:
        raise Exception("Specified number of cohorts is not equal to number of LD matrices provided!")
    if len(r_fpaths_list) != K:
        raise Exception("Specified number of cohorts is not equal to number of marginal estimates provided!")
    if len(prior_vars_list) != L:
        raise Exception("Number of prior variances must be L!")
    if len(prior_probs_list) != L:
        raise Exception("Number of prior mixture probabilites must be L!")

    if rank == 0:
        logging.info("Input arguments:")
        for flag, val in [("--ld-files", ld_fpaths), ("--r-files", r_fpaths),
                          ("--out-name", out_name), ("--out-dir", out_dir),
                          ("--true-signal-file", true_signal_fpath), ("--N", Ns), ("--M", Ms),
                          ("--K", K), ("--L", L), ("--iterations", iterations),
                          ("--prior-vars", prior_vars), ("--prior-probs", prior_probs),
                          ("--gam1", gam1), ("--gamw", gamw), ("--lmmse-damp", lmmse_damp),
                          ("--learn-gamw", learn_gamw), ("--rho", rho), ("--cg-maxit", cg_maxit),
                          ("--s", s), ("--prior-update", prior_update),
                          ("--update-prior-from", update_prior_from)]:
            logging.info(f"{flag} {val}")
        if prior_update == "em":
            logging.info(f"--em_prior_maxit {em_prior_maxit}")
        logging.info(f"--bim-files {bim_fpaths}\n")

    # .bim merge (main.py:126-165)
    ts = time.time()
    if bim_fpaths is not None:
        if rank == 0:
            logging.info("...loading .bim files\n")
        bim_ref_df, bim_list = merge_bims(bim_fpaths.split(","))
        bim_ref = list(bim_ref_df["Variant"])
        M = len(bim_ref)
        idx = {rs: i for i, rs in enumerate(bim_ref)}
        i_maps = [[idx[rs] for rs in bim_list[k]] for k in range(K)]
        if rank == 0:
            logging.info(f"Total number of markers in reference is {M} \n")
            logging.info("...Saving refenrence .bim file \n")
            bim_ref_df.iloc[:, :6].to_csv(os.path.join(out_dir, out_name + ".bim"), header=None,
                                          sep="\t", index=False)
    else:
        if len(set(M_list)) != 1:
            raise Exception("--bim-files is required when cohorts have different markers")
        M = M_list[0]
        i_maps = [list(range(M))] * K
    logging.debug(f"Rank {rank}: Handling .bim file took {time.time() - ts} seconds \n")   # main.py:165

    # r and R (main.py:167-266)
    if rank == 0:
        logging.info("...loading R matrix and r vector\n")
    ts = time.time()
    r = np.stack([load_r(r_fpaths_list[k], M_list[k], N_list[k], i_maps[k], M) for k in range(K)])
    # per-rank lines of main.py:193-194 (every rank holds all K cohorts' r here)
    logging.info(f"Rank {rank} loaded r vector with shape {r.shape}\n")
    logging.debug(f"Rank {rank}: Loading r vector took {time.time() - ts} seconds \n")
    ts = time.time()
    by_path = {}
    lds = []
    if any(p.endswith(".ld") for p in ld_fpaths_list):
        # PLINK text LD: every cohort's table plus the missing-marker exchange (main.py:203-257)
        if bim_fpaths is None or not all(p.endswith(".ld") for p in ld_fpaths_list):
            raise Exception("PLINK .ld LD needs --bim-files and a .ld file for every cohort")
        mats, r = load_plink_ld_all(ld_fpaths_list, r, bim_ref, bim_list, N_list)
        for k in range(K):
            by_path[k] = BlockLD.from_csr(mats[k], s=s)
            lds.append(by_path[k])
    else:
        for k in range(K):
            p = ld_fpaths_list[k]
            if p not in by_path:
                if p.endswith(".bed"):   # genotypes: the blocks are formed on the device
                    by_path[p] = load_bed_ld(
                        p, s, block_size=args.ld_block_size, blocks_file=args.ld_blocks,
                        variants=bim_ref if bim_fpaths is not None else None,
                        window=None if args.ld_window is None else int(args.ld_window),
                        window_kb=None if args.ld_window_kb is None else float(args.ld_window_kb),
                        window_cm=None if args.ld_window_cm is None else float(args.ld_window_cm),
                        taper=args.ld_taper, chr_blocks=args.ld_chr_blocks, form=args.ld_form)
                else:
                    by_path[p] = load_ld(p, s)
            lds.append(by_path[p])
    for L in lds:
        if L.M != M:
            raise Exception(f"LD matrix has {L.M} markers, expected {M}")
    if rank == 0:
        logging.info(f"Loaded {len(by_path)} LD matrix/matrices, blocks {lds[0].block_sizes[:8]}"
                     f"{'...' if len(lds[0].block_sizes) > 8 else ''}\n")
    # main.py:262-263 (the LD is uploaded per rank: its blocks of the partition)
    logging.info(f"Rank {rank} loaded R matrix with shape {(lds[0].M, lds[0].M)}\n")
    logging.debug(f"Rank {rank}: Loading R matrix took {time.time() - ts} seconds \n")
    if rank == 0 and args.ld_form == "factor":
        logging.info("LD form: factor (each pass applies G (G^T p) from the 2-bit genotype rows; "
                     "no R is stored)\n")

    x0 = None
    if true_signal_fpath is not None:
        x0 = load_true_signal(true_signal_fpath, M, N_list[0])
        if rank == 0:
            logging.info(f"True signals loaded. Shape: {x0.shape}\n")

    a = np.array(N_list) / sum(N_list)   # main.py:287
    sgv = VAMP(N=N_list, Nt=Nt, M=M, K=K, rho=rho, gam1=gam1, gamw=gamw, a=a,
               prior_vars=prior_vars_list, prior_probs=prior_probs_list, out_dir=out_dir,
               out_name=out_name, comm=comm, seed=seed,
               device=None if args.device is None else int(args.device),
               ld_precision=args.ld_precision, ld_packing=args.ld_packing == "on",
               posterior=None if args.posterior == "none" else args.posterior,
               pip_threshold=args.pip_threshold)
    if rank == 0:
        logging.info("...Running sgVAMP\n")
    ts = time.time()
    R = lds[0] if len(by_path) == 1 else lds
    xhat1 = sgv.infer(R, r, iterations, x0=x0, cg_maxit=cg_maxit, em_prior_maxit=em_prior_maxit,
                      learn_gamw=learn_gamw, lmmse_damp=lmmse_damp, prior_update=prior_update,
                      update_prior_from=update_prior_from)
    te = time.time()
    if rank == 0:
        logging.info(f"sgVAMP inference running time: {(te - ts):0.4f}s\n")   # main.py:324
    if x0 is not None:
        alignments, l2s = [], []
        for it in range(iterations):
            x = xhat1[it].squeeze()
            alignments.append(np.inner(x, x0.squeeze()) / np.linalg.norm(x) / np.linalg.norm(x0.squeeze()))
            l2s.append(np.linalg.norm(x - x0.squeeze()) / np.linalg.norm(x0.squeeze()))
        if rank == 0:
            logging.info(f"Alignment(x1hat, x0) over iterations: \n {alignments}\n")
            logging.info(f"L2 error(x1hat, x0) over iterations: \n {l2s}\n")
    sgv.engine.close()
    return xhat1


if __name__ == "__main__":
    main()
