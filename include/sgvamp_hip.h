/*
 * sgvamp_hip.h -- C ABI of the MI355X-native sgVAMP hot path (libsgvamp_hip.so).
 *
 * The reference (medical-genomics-group/sgVAMP-py) has no FFI layer; its hot path
 * sits behind the class seam VAMP(...)/VAMP.infer(...) (src/sgvamp.py:15,196) and
 * the operator seam con_grad(A, b, maxiter, x0) -> (x, info) (src/sgvamp.py:7,316,332).
 * Every entry point below names the reference code it replaces.  The Python host
 * (sgvamp-py_amd/sgvamp.py) binds them with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *  - Return 0 on success, a negative SGV_ERR_* code on failure; the message is in
 *    sgv_last_error(ctx) (ctx may be NULL for errors raised before a ctx exists).
 *    No C++ exception crosses the ABI.
 *  - Host arrays are caller-owned, C-contiguous, borrowed for the call only.
 *    Vectors are f64 in the rank-local DENSE marker order (the rank's blocks
 *    concatenated).  Device memory is owned by the ctx.
 *  - One ctx per process and GPU; one host thread drives it; not re-entrant.
 *  - Markers are partitioned into LD blocks (block-diagonal LD).  A rank owns a
 *    contiguous range of global blocks [blk0, blk0 + nblk).  All K cohorts of a
 *    marker live on the same rank.  Every M-length reduction is summed per LD
 *    block in a fixed order and then over blocks in global block order, so runs
 *    on 1/2/4/8 GPUs give bit-identical results.
 */
#ifndef SGVAMP_HIP_H
#define SGVAMP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGV_OK 0
#define SGV_ERR_HIP (-1)
#define SGV_ERR_ARG (-2)
#define SGV_ERR_RCCL (-3)
#define SGV_ERR_STATE (-4)

/* ABI revision of this header.  2: sgv_timers / sgv_exchange_stats take the
 * caller's buffer length (cap), sgv_comm_info added.  An integrator checks
 * sgv_abi_version() == SGV_ABI_VERSION before binding the rest.  Entry points
 * added since (sgv_posterior, the sgv_geno_* family with its _reach entries,
 * sgv_ld_pass_form and sgv_pass_form_model) change no existing signature or layout and leave the
 * revision at 2. */
#define SGV_ABI_VERSION 2
int sgv_abi_version(void);

#define SGV_MAX_COHORTS 1024 /* cohorts per context (the reference's K is its MPI
                                world size); the LMMSE batches them 8 at a time
                                (16 CG right-hand sides per LD pass), the marker
                                kernels (denoiser, EM, MLE) 32 per launch          */
#define SGV_MAX_SLABS 8     /* L - 1 slab components of the prior      */

/* vector ids for sgv_set_vector / sgv_get_vector */
#define SGV_VEC_R 0       /* r_k = X_k^T y_k            (src/main.py:176-191,266)   */
#define SGV_VEC_R1 1      /* r1_k, denoiser input        (src/sgvamp.py:204,348)     */
#define SGV_VEC_XHAT1 2   /* xhat1 (shared)              (src/sgvamp.py:273-276)     */
#define SGV_VEC_XHAT2 3   /* xhat2_k                     (src/sgvamp.py:316-323)     */
#define SGV_VEC_SIG2U 4   /* Sigma2_u_k                  (src/sgvamp.py:332-333)     */
#define SGV_VEC_X0 5      /* true signal for metrics     (src/main.py:268-285)       */

/* sgv_lmmse per-cohort outputs, out[k * SGV_LMMSE_NOUT + i] */
#define SGV_LMMSE_NOUT 8
#define SGV_O_TRSIGMA2 0  /* u^T Sigma2 u                 src/sgvamp.py:338 */
#define SGV_O_ALPHA2 1    /* alpha2 (after damping)       :340,345-346      */
#define SGV_O_GAM1 2      /* gam2 (1-alpha2)/alpha2       :347              */
#define SGV_O_Z 3         /* z (clamped at 0)             :352-354          */
#define SGV_O_TRRSIGMA2 4 /* u^T R Sigma2 u               :359              */
#define SGV_O_GAMW 5      /* 1/(z/N + TrRSigma2/N), not yet clamped at 1 :363 */
#define SGV_O_XR 6        /* xhat2^T r                    :352              */
#define SGV_O_XRX 7       /* xhat2^T R xhat2              :352              */

typedef struct sgv_ctx sgv_ctx;

/* ---- lifetime ------------------------------------------------------------ */

/* Per-rank setup; replaces src/main.py:79-97 (K, N lists), :143 (M), :287 (a)
 * and VAMP.__init__ src/sgvamp.py:15-31 for the device side.
 *   device          HIP device ordinal this rank drives
 *   K               cohorts (1..SGV_MAX_COHORTS)
 *   nld             distinct LD matrices; ld_of[k] in [0, nld)
 *   nblk, blk_sizes LD blocks owned by this rank, in marker order
 *   blk0            global index of this rank's first block
 *   nblk_global     total blocks over all ranks
 *   M_total         total markers over all ranks (np.mean denominators) */
int sgv_create(int device, int K, int nld, const int* ld_of, int nblk,
               const int64_t* blk_sizes, int blk0, int nblk_global, int64_t M_total,
               sgv_ctx** out);
void sgv_destroy(sgv_ctx* ctx);
const char* sgv_last_error(const sgv_ctx* ctx);

/* ---- multi-GPU (RCCL over xGMI) ----------------------------------------- */

/* Replaces mpi4py COMM_WORLD (src/main.py:16-18) and the per-iteration K x M
 * bcast all-gather (src/sgvamp.py:228-233), which disappears because all cohorts
 * of a marker are co-located.  What remains are ordered reductions of per-block
 * partial sums (ncclAllGather).  id: 128 bytes (ncclUniqueId) from rank 0.
 * nranks may be 1: a real one-rank communicator then carries the same gather
 * (rehearses the RCCL calls on a single GPU; results bitwise unchanged). */
int sgv_comm_unique_id(char* id_out /* 128 bytes */);
int sgv_comm_init(sgv_ctx* ctx, int nranks, int rank, const char* id /* 128 bytes */,
                  const int* nblk_per_rank /* [nranks] */);
/* Host-side exchange instead of RCCL (same ordered reductions, bitwise the same
 * results): the library copies its per-block partials to host memory and calls
 * fn(user, send, recv, count) which must all-gather `count` doubles from every
 * rank into recv[nranks][count] in rank order and return 0.  For ranks that
 * RCCL cannot connect (several ranks on one device, hosts without xGMI peers)
 * and for testing the sharded path with a host communicator. */
typedef int (*sgv_allgather_fn)(void* user, const double* send, double* recv, int64_t count);
int sgv_comm_init_host(sgv_ctx* ctx, int nranks, int rank, const int* nblk_per_rank,
                       sgv_allgather_fn fn, void* user);

/* ---- inputs -------------------------------------------------------------- */

/* Upload one dense LD block (row-major n x n, host row stride ld_host elements).
 * Replaces the R loaders src/main.py:199-202 (dense .npy / CSR .npz blocks). */
int sgv_set_ld_block(sgv_ctx* ctx, int ld, int blk_local, const double* rowmajor,
                     int64_t ld_host);
/* Upload one symmetric LD block from the CSR arrays of its upper triangle
 * (diagonal included; block-relative column indices >= the row; duplicates are
 * summed).  Replaces the sparse loaders src/main.py:199-200 (.npz CSR of any
 * sparsity) and :251-257 (PLINK .ld pairs assembled into CSR): a block whose
 * entries lie within j - i <= bw is stored as a packed BAND -- panel g (rows
 * 256g ..) keeps columns 256g .. 256g + round_up(256 + bw, 256) - 1 -- so
 * windowed LD over a whole chromosome needs n * (bw + 256..511) doubles instead
 * of n^2 / 2.  Blocks whose band is as wide as the triangle are stored as the
 * packed triangle.  Never allocates n x n on the host. */
int sgv_set_ld_block_csr(sgv_ctx* ctx, int ld, int blk_local, const int64_t* indptr /* n+1 */,
                         const int64_t* indices, const double* data);
/* R_s xhat2 and R_s Sigma2_u for gamw learning (src/sgvamp.py:352,359) and the
 * next warm start's R_s x0 (scipy iterative.py:392): on (default), carried
 * through both CG solves -- x_k = x_0 + sum a_i p_i, so R_s x_k = R_s x_0 +
 * sum a_i R_s p_i with R_s p_i written by the pass the CG makes anyway -- which
 * saves one LD pass per outer iteration; off, computed by a separate pass as
 * the reference does.  Same values in exact arithmetic; measured against the
 * reference fixtures the carried form agrees as closely (tests/). */
int sgv_set_rs_recurrence(sgv_ctx* ctx, int on);
/* Packed passes with at least nc_min right-hand sides run on the f64 matrix
 * cores (v_mfma_f64_16x16x4f64); fewer run on the VALU.  0 = never.  Default 3.
 * Results agree to rounding, not bitwise, across the two. */
int sgv_set_mfma_min(sgv_ctx* ctx, int nc_min);
/* CG and EM-loop drivers (scipy iterative.py:397-422; src/sgvamp.py:250-257):
 * on (default) the CG's stop test, beta and alpha, and the EM prior loop's
 * update and convergence test run on the device, and iteration i+1 is enqueued
 * while iteration i runs (no host round trip between iterations); off, the
 * host tests every iteration.  Same iterates and counts; env SGV_CG_PIPE=0
 * sets the default off.  Column sets of the pipelined CG: see sgv_set_cg_exact. */
int sgv_set_cg_pipeline(sgv_ctx* ctx, int on);
/* Column sets of the pipelined CG's passes.  mode 1 ("exact"): a pass over an
 * LD matrix shared by >= 3 columns carries only the columns still active after
 * its own stop test (the host reads the test while the p update runs); mode 0:
 * one iteration of look-ahead (a column stopping at that test rides along
 * unused).  The two modes can round differently where the narrower set runs
 * another pass kernel, so every rank of a run must use the same mode -- it is
 * the run's choice, not a rank's: Python's Engine sets it from the GLOBAL LD
 * size (>= 24 GB packed-triangle bytes), identical for 1 and N ranks.  mode -1
 * (default): by this rank's stored bytes at one rank, look-ahead with a
 * communicator.  SGV_CG_EXACT=0/1 (with SGV_AB=1) overrides every mode. */
int sgv_set_cg_exact(sgv_ctx* ctx, int mode);
/* Storage of LD blocks set or generated from now on: mode 1 (default) stores a
 * block that is exactly symmetric as packed upper-triangle panels (about half
 * the bytes per pass: the LD matrix of src/main.py:199-265 is symmetric by
 * construction, R = X^T X); mode 0 always stores the full square. */
int sgv_set_ld_packing(sgv_ctx* ctx, int mode);
/* fmt_out: 0 dense, 1 packed symmetric (triangle), 2 packed band, 3 factor
 * (sgv_geno_ld_factor), -1 not set. */
int sgv_ld_block_format(sgv_ctx* ctx, int ld, int blk_local, int* fmt_out);
/* Element type of PACKED blocks (triangle or band: symmetric blocks through
 * sgv_set_ld_block with packing on, every sgv_set_ld_block_csr block, the
 * blocks of sgv_synth_ld_g) set or generated from now on: bits = 64 (default)
 * or 32; anything else is SGV_ERR_ARG.  With 32 every stored element is rounded
 * ONCE, on store, to the nearest float (round to nearest even: numpy's
 * astype(float32)) -- the host upload, the CSR panel assembly (after summing
 * duplicates in f64) and the generator's store of G G^T (computed in f64) --
 * in the same panels, stored extent and row stride (a multiple of 128
 * elements) as the f64 layout, at 4 bytes per element.  Every product,
 * accumulation, CG scalar and denoiser stays f64: the pass widens each element
 * to f64 in registers and runs the same f64 MFMA chains, so a run is the exact
 * f64 solve of a problem whose R was perturbed by <= 2^-24 relative per entry.
 * A finite entry outside float's range fails the upload with SGV_ERR_ARG (the
 * block is then unset); correlations never do.  A block stored as the full
 * square (packing off, or not symmetric) stays f64 whatever the setting, and so
 * do coupling matrices (sgv_set_ld_coupling).  All packed blocks of ONE LD
 * matrix must share one precision (the first pass over a mixed matrix fails
 * with SGV_ERR_STATE, naming the matrix); different LD matrices of a context may
 * differ.  An f32 matrix runs every column count 1-16 on the 512-column MFMA
 * strips, whatever sgv_set_mfma_min says (the VALU pass and the wave-pair and
 * wide forms are f64-only; the band walks have float instances, but measured
 * 1.26-1.33x the strips' time on an f32 band at 3-8 columns, so a windowed-LD
 * matrix stored as f32 stays on the strips too and walks only with SGV_AB=1
 * SGV_F32_WALK=1: DESIGN.md 4.4; the decision is pass_form's, csrc/pass_form.cpp,
 * and sgv_ld_pass_form reports it); a block's sums are a function of the
 * block alone, within 1e-12 of the f64 product of the stored values (with
 * SGV_AB=1 SGV_F32_FORM=1, the 8-byte load form, bitwise the f64 strips').
 * Measured per pass against f64: 0.53-0.57x at 2-4 columns, 0.67-0.74x at 8,
 * 0.83-0.88x at 16.  Bytes: sgv_ld_stored_bytes and
 * sgv_timers t[2] count 4 bytes per stored element of an f32 block (the bytes
 * actually stored); t[4], the dense-equivalent bytes, stays n^2 * 8. */
int sgv_set_ld_precision(sgv_ctx* ctx, int bits);
/* bits_out: 64 or 32, the element type block blk_local is stored in; -1 not set. */
int sgv_ld_block_precision(sgv_ctx* ctx, int ld, int blk_local, int* bits_out);
/* Bytes one pass over LD matrix ld reads from this rank's blocks that are set
 * (dense n^2*8, packed triangle / band: the stored panels, 8 or 4 bytes per
 * element).  Python's Engine
 * sums it over ranks to pick the run's CG column-set mode (sgv_set_cg_exact). */
int sgv_ld_stored_bytes(sgv_ctx* ctx, int ld, double* bytes_out);
/* Coupling between consecutive band pieces gb and gb + 1 (global block
 * indices) of LD matrix ld: C = R[last nr rows of gb][first nc columns of gb+1],
 * nr x nc row-major.  A band block too long for one GPU (one chromosome of
 * windowed LD: src/main.py:199-200,251-257) is cut into pieces that ranks own
 * like LD blocks; a pass then adds C p_{gb+1}[head] to gb's last rows and
 * C^T p_gb[tail] to gb+1's first rows, in a fixed order on every rank (results
 * bitwise independent of the rank count), the halo of a coupling that spans two
 * ranks exchanged per pass.  Every rank calls this for EVERY coupling (C may be
 * NULL where the rank owns neither piece): the exchange is collective.  Pieces
 * must be stored packed (sgv_set_ld_block_csr). */
int sgv_set_ld_coupling(sgv_ctx* ctx, int ld, int gb, int nr, int nc, const double* C);
/* Download one LD block (row-major n x n into a host array of row stride
 * ld_host): exactly the stored values, symmetric (an f32 block's widened). */
int sgv_get_ld_block(sgv_ctx* ctx, int ld, int blk_local, double* rowmajor, int64_t ld_host);
/* Start a new VAMP.infer on this context (src/sgvamp.py:198-217 restarts from
 * r1 = r, xhat2 = 0, Sigma2_u_prev = 0 on every call): zeroes every solver
 * vector except r, r1 and x0 and clears the warm-start and chained-step state.
 * LD blocks, ridge and cohort sizes are kept.  Fails while a step is queued. */
int sgv_reset_solver(sgv_ctx* ctx);
/* R_s = (1 - s) R + s I, applied inside every LD pass (src/main.py:265). */
int sgv_set_ridge(sgv_ctx* ctx, double s);
/* Cohort sample size N_k (src/main.py:83-85; used by gamw learning :352,363). */
int sgv_set_cohort_n(sgv_ctx* ctx, int k, double N);

/* SGV_VEC_XHAT2 / SGV_VEC_SIG2U set the next LMMSE step's warm start: R_s x0 of a
 * non-zero vector is re-derived by one LD pass in that step; an all-zero vector
 * makes the column cold (as after sgv_reset_solver) and its stored R_s x0 is
 * zeroed with it. */
int sgv_set_vector(sgv_ctx* ctx, int which, int k, const double* host_local);
int sgv_get_vector(sgv_ctx* ctx, int which, int k, double* host_local);

/* ---- synthetic data on device (simulation/sim_gen_phen_mult.py:36-55) ------
 * Genotypes x_{in} ~ Binomial(2, 0.4) from a counter-based hash of
 * (geno_seed, global marker index, sample n); standardised per marker over the
 * Nsamp samples (population std), X_std; G = X_std / sqrt(Nsamp).
 * marker0 = global index of this rank's first marker (keys the hash, so the
 * data does not depend on how blocks are spread over ranks).
 * Step 1: for every owned block b: if ld >= 0 store R_b = G_b G_b^T into LD
 *         matrix `ld`; write g_b[n] = sum_{i in b} X_std[i][n] beta_i to
 *         g_blocks_out[b * Nsamp + n] (host, nblk x Nsamp).
 * Step 2 (after the host forms y = sum_b g_b + w): r_k,b = G_b y. */
int sgv_synth_ld_g(sgv_ctx* ctx, int ld, uint64_t geno_seed, int64_t marker0, int Nsamp,
                   const double* beta_local, double* g_blocks_out);
int sgv_synth_r(sgv_ctx* ctx, int k, uint64_t geno_seed, int64_t marker0, int Nsamp,
                const double* y);

/* ---- genotype LD source: PLINK 1 .bed rows -> LD blocks, r and g ----------
 * The reference's simulation/sim_phen.py:33-37,58-59 (bed_reader's default: x =
 * count of A1; X standardised per marker; r = X^T y / sqrt(N)) and the LD R =
 * X^T X / N of the same genotypes, formed on the device from the 2-bit codes
 * without X, G or R ever existing on the host.
 * A row is one marker, SNP-major: sample n has code (row[n / 4] >> 2 (n % 4)) & 3,
 * 0 = homozygous A1 (x = 2), 1 = missing, 2 = heterozygous (x = 1), 3 =
 * homozygous A2 (x = 0); the bits past sample nsamp of the last byte are padding
 * and are never counted.  Per marker, over its observed samples, in exact
 * integers: n_obs, S1 = sum x, S2 = sum x^2; mean = S1 / n_obs, sd = sqrt((n_obs
 * S2 - S1^2) / n_obs^2); G[i][n] = ((x - mean) / sd) / sqrt(nsamp), 0 where
 * missing (mean imputation), so R_ii = n_obs_i / nsamp.  A marker with n_obs = 0
 * or n_obs S2 = S1^2 (one value among its observed samples) has no LD.
 *
 * sgv_geno_set_block: rows = the block's n_b rows (block-local marker order),
 * consecutive rows row_bytes apart (>= ceil(nsamp / 4); no alignment needed).
 * Copies them to the device, keeps them and the per-marker tables there until
 * the next call for the block, sgv_geno_clear or sgv_destroy, and returns
 * counts_out[i * 4 + code] = samples of marker i with that code (n_b x 4).  Bad
 * shapes are SGV_ERR_ARG.  Markers without LD are not an error here: the caller
 * finds them in the counts (and reports them before asking for LD).
 * sgv_geno_ld: R_b = G_b G_b^T of block blk_local into LD matrix ld, in the
 * context's packing (sgv_set_ld_packing) and precision (sgv_set_ld_precision: 32
 * rounds each f64 sum once, on store), as sgv_synth_ld_g stores its blocks; the
 * device memory it needs beyond the block is the rows (n_b ceil(nsamp / 16) 4
 * bytes) whatever nsamp.  SGV_ERR_STATE, with the stored block (if any) left as
 * it was, when the block has no genotypes or a marker without LD.
 * sgv_geno_r: r_k = G y over every owned block (y: nsamp doubles).
 * sgv_geno_g: g_blocks_out[b * nsamp + n] = sum_{i in b} X_std[i][n] beta_i, X_std
 * = sqrt(nsamp) G, beta_i == 0 skipped (nblk x nsamp, as sgv_synth_ld_g).
 * Both need genotypes of one nsamp, without such markers, in every owned block
 * (SGV_ERR_STATE otherwise).
 * sgv_geno_clear frees the rows and tables of every block. */
int sgv_geno_set_block(sgv_ctx* ctx, int blk_local, const uint8_t* rows, int64_t row_bytes,
                       int nsamp, int64_t* counts_out);
int sgv_geno_ld(sgv_ctx* ctx, int ld, int blk_local);
int sgv_geno_r(sgv_ctx* ctx, int k, const double* y);
int sgv_geno_g(sgv_ctx* ctx, const double* beta_local, double* g_blocks_out);
int sgv_geno_clear(sgv_ctx* ctx);

/* ---- factor LD blocks: R_b p applied as G_b (G_b^T p) from the 2-bit rows -----
 * sgv_geno_ld_factor: block blk_local of LD matrix ld becomes a factor block of
 * exactly the G defined above (same integer counts, mean, sd, mean imputation,
 * G[i][n] = lut_i[code_in]).  No R_b is formed or stored: every LD pass (CG, the
 * warm-start residual, the gamw pass, sgv_ld_matvec, sgv_ld_pass_ex) applies
 *   t = G_b^T P (nsamp x ncol), Q = G_b t (n_b x ncol)
 * and then the epilogue of every other form (out = c1 Q + c2 in, the optional
 * yout, the dot partials in block order), so R_b = G_b G_b^T is positive semi-
 * definite by construction and the ridge works through c1 / c2 as always.  The
 * block holds 2 bits per genotype (the rows at their stride of whole 32-bit
 * words) plus 32 bytes of table per marker.  Every sum has a fixed order that is
 * a function of (n_b, nsamp, ncol) alone (csrc/geno_factor.hip), so results are
 * bitwise the same for every rank count and whatever else is in the launch.
 * The call TAKES OVER the rows and tables staged by sgv_geno_set_block for the
 * block (a hand-over: nothing is computed or copied); the staged block is empty
 * afterwards, so another panel can be staged for the same block of another LD
 * matrix (cohorts with distinct panels), and sgv_geno_r / sgv_geno_g need a fresh
 * sgv_geno_set_block -- or must run before this call.  sgv_destroy, and a later
 * sgv_geno_ld_factor for the same block, release what was taken over;
 * sgv_geno_clear does not touch it.
 * One form per LD matrix: SGV_ERR_STATE, with the stored block (if any) left as
 * it was, when the block has no staged genotypes, when a marker has no LD, when
 * the matrix already holds a block of another form or a coupling -- and from
 * sgv_set_ld_block, sgv_set_ld_block_csr, sgv_set_ld_coupling, sgv_synth_ld_g and
 * every sgv_geno_ld* / sgv_geno_coupling* on a matrix that holds factor blocks.
 * There is no window, taper, coupling or f32 storage of this form
 * (sgv_set_ld_precision and sgv_set_ld_packing do not apply), and
 * sgv_get_ld_block is SGV_ERR_STATE: there is no R to download.
 * sgv_ld_block_format reports 3, sgv_ld_block_precision 64, sgv_ld_stored_bytes
 * and sgv_timers t[2] the bytes a pass reads (rows at their stride + tables);
 * t[6] counts 2 ncol (2 nsamp n_b) flops per block and pass, t[5] the scratch
 * written and read (t and the first product's slab partials).  The scratch is
 * the context's: at most 256 MB, or one block's (ceil(n_b / 1024) + 1) nsamp 128
 * bytes where that is more.  sgv_ld_pass_form reports SGV_KIND_FACTOR. */
int sgv_geno_ld_factor(sgv_ctx* ctx, int ld, int blk_local);

/* ---- windowed genotype LD: packed bands and their couplings from the bits ---
 * With a window W >= 1, counted in markers of the run's marker order (block-
 * local row order here), inside each LD block:
 *   R_b[i][j] = (G_b G_b^T)[i][j]  if |i - j| <= W,
 *   R_b[i][j] = exactly 0.0        otherwise,
 * G as above (same counts, mean, sd, mean imputation, R_ii = n_obs_i / nsamp).
 * Every stored entry is the same sample-sequential sum sgv_geno_ld forms, so the
 * band equals the masked dense-triangle block entry for entry and does not
 * depend on where a band is cut into pieces.  Truncating LD to a window does not
 * preserve positive semi-definiteness (as PLINK's --ld-window); the ridge
 * (sgv_set_ridge) is the remedy.
 *
 * sgv_geno_ld_band: block blk_local of LD matrix ld from the rows staged by
 * sgv_geno_set_block, stored by sgv_set_ld_block_csr's rule: with bw = min(window,
 * n - 1) a packed band of panel extent round_up(256 + bw, 256) columns, or the
 * packed triangle (still masked to the window) where that extent is >= n; in the
 * context's precision (sgv_set_ld_precision).  The block is indistinguishable
 * from the same matrix uploaded as CSR.  SGV_ERR_ARG: window < 1; SGV_ERR_STATE:
 * packing is off (a band is a packed layout), or -- the stored block (if any)
 * left as it was -- the block has no genotypes or a marker without LD.
 * sgv_geno_coupling: the coupling between band pieces gb and gb + 1 (see
 * sgv_set_ld_coupling) from genotypes: rows = the last nr rows of piece gb, then
 * the first nc rows of piece gb + 1 (nr + nc rows, row_bytes apart).  Forms C =
 * G_tail G_head^T on the device, entry (a, c) kept iff c + nr - a <= window (the
 * two markers' distance), with precision 32 each entry rounded once to f32, and
 * registers it as sgv_set_ld_coupling does, so cut pieces plus couplings are
 * exactly the uncut band.  The same collective contract: every rank calls it for
 * every coupling; rows and counts_out may be NULL where the rank owns neither
 * piece.  counts_out[i * 4 + code] as sgv_geno_set_block's ((nr + nc) x 4);
 * SGV_ERR_STATE, nothing registered, when a row has no LD. */
int sgv_geno_ld_band(sgv_ctx* ctx, int ld, int blk_local, int64_t window);
int sgv_geno_coupling(sgv_ctx* ctx, int ld, int gb, int nr, int nc, const uint8_t* rows,
                      int64_t row_bytes, int nsamp, int64_t window, int64_t* counts_out);

/* ---- distance-windowed genotype LD: a reach per row, a PSD-preserving taper --
 * Positions.  Inside one LD block, in the run's marker order, marker i has a
 * position pos[i] (f64): a base-pair coordinate (span D = 1000 x kb), a genetic
 * position in cM (D = the cM), or, for a marker window with a taper, its index in
 * the block (D = W + 1).  Positions are finite and non-decreasing inside a block;
 * ties are allowed.
 * Reach.  hi[i] = max{ j : i <= j < n_b, pos[j] - pos[i] <= D }, the predicate
 * evaluated as that f64 subtraction and comparison (a searchsorted on pos + D is a
 * first guess only, fixed up by testing the predicate at hi and hi + 1).  With a
 * marker window W as well, hi[i] = min(hi[i], i + W): both limits apply, as in
 * PLINK.  hi is non-decreasing and hi[i] >= i.
 * Kept entries.  For j >= i, entry (i, j) is kept iff j <= hi[i]; everything else
 * is exactly 0.0; the lower triangle is the mirror.
 * Values.  Without a taper a kept entry is (G_b G_b^T)[i][j], sgv_geno_ld's
 * sample-sequential fma chain, bit for bit.  With the triangular (Bartlett) taper
 * it is acc * w, w = 1.0 - (pos[j] - pos[i]) / D, formed in exactly that order in
 * f64 (one subtraction, one IEEE division, one subtraction, one multiplication; no
 * contraction), rounded once to f32 on store when the context's precision is 32.
 * w >= 0 follows from the reach predicate; the diagonal has w = 1, so R_ii =
 * n_obs_i / nsamp as before; an entry at distance exactly D is stored as an
 * explicit 0.0.  w(d) = max(0, 1 - d / D) is a positive-definite function on the
 * line, so by the Schur product theorem R o [w(pos_i - pos_j)] is positive
 * semi-definite whenever R = G G^T is, which a hard window is not.
 * One window per taper: a taper needs exactly one of the three windows (its
 * distance would be ambiguous with two).
 * Storage.  With bw = max_i (hi[i] - i), sgv_set_ld_block_csr's rule: a packed
 * band of panel extent round_up(256 + bw, 256), the packed triangle where that is
 * >= n_b -- per block, so per band piece: the extent follows the widest reach in
 * the piece.
 *
 * sgv_geno_ld_band_reach: block blk_local from the rows staged by
 * sgv_geno_set_block, with the reach hi (n_b) and, for a taper, pos (n_b) and span
 * D (pos NULL: no taper, span ignored).  State checks, storage and "stored block
 * untouched on error" as sgv_geno_ld_band.  SGV_ERR_ARG: hi[i] outside [i, n_b -
 * 1] or decreasing; with pos: a non-finite or decreasing position, span not finite
 * or <= 0, or pos[hi[i]] - pos[i] > span (a negative weight).
 * sgv_geno_coupling_reach: sgv_geno_coupling with keep (nr), a count of head
 * columns per tail row: entry (a, c) is kept iff c < keep[a]; pos: the nr + nc
 * halo rows' positions (NULL: no taper), the weight from pos[nr + c] - pos[a].  The
 * same collective contract (rows, counts_out, keep and pos may be NULL where the
 * rank owns neither piece).  SGV_ERR_ARG: keep[a] outside [0, nc] or decreasing,
 * and the position errors above (pos[nr + keep[a] - 1] - pos[a] > span); an
 * all-zero keep registers a zero coupling. */
int sgv_geno_ld_band_reach(sgv_ctx* ctx, int ld, int blk_local, const int32_t* hi,
                           const double* pos, double span);
int sgv_geno_coupling_reach(sgv_ctx* ctx, int ld, int gb, int nr, int nc, const uint8_t* rows,
                            int64_t row_bytes, int nsamp, const int32_t* keep, const double* pos,
                            double span, int64_t* counts_out);

/* ---- scoring: a target .bed panel against saved effects ---------------------
 * gVAMP's `test` run mode: S[n][c] = sum_i X[i][n] B[i][c] over a stream of marker
 * chunks of a TARGET panel of nsamp samples (any panel: no LD needs to be set, and
 * the LD, the staged genotype blocks, the vectors and the timers of a context that
 * has them are not touched), for ncol = 1..SGV_SCORE_MAXCOL effect columns, on the
 * f64 matrix cores from the 2-bit rows (csrc/score.hip).  X[i][n] = tab_i[code_in],
 * rows and codes as in "genotype LD source" above.
 * sgv_score_begin starts a stream (a stream in progress is dropped) with S = +0.
 * sgv_score_chunk adds the next n markers: rows (n rows, row_bytes apart, >=
 * ceil(nsamp / 4)), column c's n effects at beta + c ldb (ldb >= n when ncol > 1),
 * counts_out[i * 4 + code] as sgv_geno_set_block fills it (n x 4), and tab_i by mode:
 *   SGV_SCORE_TARGET  from the chunk's own exact counts: (x - mean) / sd with the
 *                     mean and sd defined above, missing -> 0, no 1 / sqrt(nsamp); a
 *                     marker that is monomorphic or unobserved in the target gets a
 *                     zero table (it scores 0; the caller finds it in the counts);
 *   SGV_SCORE_RAW     the A1 dosage 2 / 1 / 0, missing -> S1 / n_obs (0 if unobserved);
 *   SGV_SCORE_TABLE   the caller's tab[n][4] (by code 0..3), every entry finite.
 * tab is read in SGV_SCORE_TABLE mode only.  Every chunk but the stream's last
 * holds a multiple of 1,024 markers.
 * sgv_score_end writes scores_out[c * nsamp + n] = S[n][c] and ends the stream.
 * Order of every sum: markers are cut into slabs of 1,024 by their index in the
 * stream; a slab's partial starts from +0 and takes its markers four at a time in
 * ascending order; S is the slab partials added left to right in ascending slab
 * order across chunk boundaries.  So a result is bitwise independent of the chunk
 * lengths, of the device and of which columns share a call, and the bits past
 * sample nsamp of a row never reach it.
 * SGV_ERR_ARG: nsamp < 1, ncol outside 1..SGV_SCORE_MAXCOL, a null or short array,
 * an unknown mode, a non-finite tab entry, or a chunk after one that was not a
 * multiple of 1,024 markers; SGV_ERR_STATE: sgv_score_chunk or sgv_score_end without
 * sgv_score_begin.  A refusal leaves the stream and the context as they were.
 * sgv_score_timers, since the last reset: t[0] = ms of the stream's kernels (HIP
 * events), t[1] = chunks, t[2] = 2 nsamp n ncol flops summed over chunks, t[3] = host
 * ms spent staging (repacking rows, uploads, counts); writes min(cap,
 * SGV_SCORE_TIMERS_N) values. */
#define SGV_SCORE_MAXCOL 64
#define SGV_SCORE_TARGET 0
#define SGV_SCORE_RAW 1
#define SGV_SCORE_TABLE 2
#define SGV_SCORE_TIMERS_N 4
int sgv_score_begin(sgv_ctx* ctx, int nsamp, int ncol);
int sgv_score_chunk(sgv_ctx* ctx, const uint8_t* rows, int64_t row_bytes, int n, int mode,
                    const double* tab, const double* beta, int64_t ldb, int64_t* counts_out);
int sgv_score_end(sgv_ctx* ctx, double* scores_out /* ncol x nsamp */);
int sgv_score_timers(sgv_ctx* ctx, double* t, int cap, int reset);

/* ---- Hutchinson probes (host only, no device) ----------------------------
 * src/sgvamp.py:326 u = np.random.binomial(p=1/2, n=1, size=n)*2-1 from a legacy
 * numpy RandomState (MT19937) whose state is key[624], *pos (as
 * RandomState.get_state() returns them): advances the stream by n samples and
 * writes the +-1 values of samples [lo, hi) to out[0 .. hi-lo).  Bit for bit
 * numpy's stream and values; replaces the draw each reference rank makes. */
int sgv_probe_draw(uint32_t* key, int32_t* pos, int64_t n, int64_t lo, int64_t hi,
                   int8_t* out);

/* ---- the hot path -------------------------------------------------------- */

/* One VAMP outer iteration, src/sgvamp.py:222-387 without the output files and
 * logs, with no return to the caller between its phases:
 *   flags & SGV_STEP_EM:  sgv_em (lam_io, omegas_io updated; ires[0] = steps,
 *                         res[0] = final error);
 *   sgv_denoise (damping iff SGV_STEP_DENOISE_DAMP);
 *   out_slot 0/1/2:      sgv_outputs_begin(out_slot) (xhat1, r1 for the files);
 *   SGV_STEP_METRICS:    the metric sums of xhat1 (:381-382) in res[1 + 2K .. + 4);
 *   alpha1 = der_sum / M_total, damped with alpha1_prev iff SGV_STEP_ALPHA1_DAMP
 *   (:285-291), gam2 = gam1 (1 - alpha1) / alpha1 (:305): res[1 + k], res[1 + K + k];
 *   sgv_lmmse (damping iff SGV_STEP_LMMSE_DAMP, gamw learning iff
 *   SGV_STEP_LEARN_GAMW): out, cg_out as sgv_lmmse; ires[1] = LD passes.
 * res holds 1 + 2K + 4 doubles, ires 2 ints.
 * flags & SGV_STEP_MLE: sgv_mle_update instead of sgv_em (lam_io, omegas_io and the
 *                        context's gam updated; ires[0] = its status, res[0] = gam
 *                        after it, NaN while the reference's is None); the context's
 *                        gam starts as None (sgv_create) and is set by sgv_set_mle_gam.
 * SGV_STEP_CHAIN (sgv_step_begin only): gam1s, gamw (clamped to >= 1, :374),
 * alpha1_prev, alpha2_prev, *lam_io and omegas_io are taken, when the step
 * starts, from the results of the step queued before it -- so a step can be
 * queued while the previous one runs.
 * SGV_STEP_POSTERIOR (after sgv_set_posterior_outputs(ctx, 1, thr); without it
 * the step fails with SGV_ERR_STATE): the per-marker posterior of sgv_posterior
 * is enqueued right behind the denoiser -- the same gam1s (a chained step's: the
 * chain's), the same r1, the prior after this step's EM / MLE update -- before
 * the output copies.  The slot then holds (K + 4) x M_local doubles, rows K + 1
 * .. K + 3 = pip, lodds, var, and res holds 1 + 2K + 4 + 3 doubles, the last
 * three sgv_posterior's sums.  Everything else the step computes is bitwise what
 * it computes without the flag. */
#define SGV_STEP_EM 1
#define SGV_STEP_DENOISE_DAMP 2
#define SGV_STEP_ALPHA1_DAMP 4
#define SGV_STEP_LMMSE_DAMP 8
#define SGV_STEP_LEARN_GAMW 16
#define SGV_STEP_METRICS 32
#define SGV_STEP_CHAIN 64
#define SGV_STEP_MLE 128
#define SGV_STEP_POSTERIOR 256
int sgv_step(sgv_ctx* ctx, int it, int flags, int em_maxit, int nslab, const double* sigmas,
             const double* a, double* lam_io, double* omegas_io, const double* gam1s,
             double rho, const double* gamw, const double* alpha1_prev,
             const double* alpha2_prev, const int8_t* probes, int cg_maxit, double rtol,
             int out_slot, double* res, int* ires, double* out, int* cg_out);
/* sgv_step on the context's host worker thread: returns at once; at most two
 * steps are queued and they run in order.  The caller may run host work
 * (files, logs, the next probes) that does not touch the context
 * (sgv_outputs_wait excepted) until sgv_step_end, which waits for the oldest
 * queued step and returns its status.  lam_io, omegas_io, probes and the
 * outputs must stay valid until then; the other arrays are copied. */
int sgv_step_begin(sgv_ctx* ctx, int it, int flags, int em_maxit, int nslab,
                   const double* sigmas, const double* a, double* lam_io, double* omegas_io,
                   const double* gam1s, double rho, const double* gamw,
                   const double* alpha1_prev, const double* alpha2_prev, const int8_t* probes,
                   int cg_maxit, double rtol, int out_slot, double* res, int* ires, double* out,
                   int* cg_out);
int sgv_step_end(sgv_ctx* ctx);

/* Meta denoiser + derivative over all markers: src/sgvamp.py:93-114 applied at
 * :270-291.  xhat1 <- denoiser_meta(r1s, gam1s); if damp: xhat1 <- rho*xhat1 +
 * (1-rho)*xhat1_prev.  der_sum_out[k] = sum_j der_denoiser_meta_k(r1s[:, j])
 * (the host divides by M_total: np.mean, :285). */
int sgv_denoise(sgv_ctx* ctx, const double* gam1s, const double* a, double lam,
                int nslab, const double* omegas, const double* sigmas, double rho,
                int damp, double* der_sum_out);

/* Per-marker posterior of the spike-and-slab prior at the denoiser's inputs (the
 * context's current r1 vectors, gam1s, a and the prior lam / omegas / sigmas;
 * no counterpart in the reference, which sums these away: pi of
 * prior_update_em, src/sgvamp.py:131-134, and the variance inside
 * der_denoiser_meta, :104-114).  With t = sum_k r1_k a_k gam1_k (cohort order,
 * as the denoiser), G = sum_k a_k gam1_k, q_l = 1 / (G sigma_l + 1), s2_l =
 * sigma_l q_l and D_l = log(lam omega_l / (1 - lam)) + (t^2 / 2) s2_l + log(q_l) / 2:
 *   lodds = log sum_l exp(D_l), the natural log of the posterior odds of
 *           inclusion, formed as max + log-sum-exp: finite wherever the inputs
 *           are (|z| = 40 in 65 cohorts), where 1 - P(spike) is exactly 1;
 *   pip   = the sigmoid of lodds, in the branch that does not cancel;
 *   var   = Var(x | r1) by the law of total variance from non-negative terms:
 *           with resp_l = exp(D_l - max) / sum, ms = t sum_l resp_l s2_l and vs =
 *           sum_l resp_l s2_l + sum_l resp_l (t s2_l - ms)^2, var = pip vs +
 *           pip (1 - pip) ms^2, 1 - pip from the sigmoid's other branch;
 *   resp  (nullable) [nslab][M_local]: resp_l, the slab responsibilities given
 *           inclusion (they sum to 1).
 * lam == 0 gives pip = 0, lodds = -inf, var = 0; lam == 1 gives pip = 1, lodds =
 * +inf, var = vs; no NaN either way.  These are the posterior at THIS r1 / gam1s
 * / prior; xhat1 (SGV_VEC_XHAT1) is the posterior mean damped with the previous
 * iteration's (rho), so the two differ from the second iteration on.
 * pip_local, lodds_local, var_local: [M_local], marker order (as sgv_get_vector).
 * sums_out[3] = sum pip (the expected number of non-null markers), sum var, and
 * the number of markers with pip >= thr (0 <= thr <= 1), over ALL ranks' markers
 * through the ordered reductions: bitwise independent of the block partition's
 * spread over ranks.  Fails with SGV_ERR_STATE while a step is queued. */
int sgv_posterior(sgv_ctx* ctx, const double* gam1s, const double* a, double lam, int nslab,
                  const double* omegas, const double* sigmas, double thr, double* pip_local,
                  double* lodds_local, double* var_local, double* resp_local, double* sums_out);
/* Posterior rows in the output slots.  on != 0: the pinned slots of
 * sgv_outputs_begin / sgv_outputs_wait are (K + 4) x M_local doubles, and steps may
 * carry SGV_STEP_POSTERIOR (thr: the count's threshold, 0.95 customary); a step
 * or sgv_outputs_begin without the flag then fills rows 0 .. K only.  on == 0
 * (the default): (K + 1) x M_local, as ever.  The slots are sized when first
 * used, so call this before the first step; a later call that changes the
 * layout waits for the queued copies and drops the slots (buffers returned by
 * sgv_outputs_wait become invalid), which the next sgv_outputs_begin makes again.
 * Fails with SGV_ERR_STATE while a step is queued. */
int sgv_set_posterior_outputs(sgv_ctx* ctx, int on, double thr);

/* EM prior update loop: src/sgvamp.py:116-136 driven as :250-257 (stop when the
 * relative change of omegas and lam are both < 1e-6, at most maxit steps). */
int sgv_em(sgv_ctx* ctx, const double* gam1s, const double* a, int nslab,
           const double* sigmas, int maxit, double* lam_io, double* omegas_io,
           int* steps_out, double* final_err_out);

/* LMMSE step for all cohorts: src/sgvamp.py:301-364.  For every cohort k:
 *   r2 = (xhat1 - alpha1 r1)/(1 - alpha1); mu2 = gamw r + gam2 r2;
 *   CG #1: (gamw R_s + gam2 I) xhat2 = mu2, warm start xhat2_prev   (:316)
 *   damping of xhat2 if lmmse_damp                                 (:322-323)
 *   CG #2: (gamw R_s + gam2 I) Sigma2_u = u, warm start Sigma2_u_prev (:332)
 *   alpha2, gam1, r1 update                                        (:338-348)
 *   if learn_gamw: z, TrRSigma2, new gamw                          (:350-363)
 * Both CG solves of all cohorts run batched: one pass over each LD matrix per
 * CG iteration serves every right-hand side still iterating.  The CG is
 * scipy 1.15.3's (iterative.py:375-422): rtol, atol 0, strict '<' stop test.
 *   per-cohort inputs [K]: gamw, gam2, alpha1, alpha2_prev
 *   probes: [K][M_local] int8 of +-1 (the host draws u, :326)
 *   out: [K][SGV_LMMSE_NOUT]; cg_out: [K][4] = iters1, info1, iters2, info2
 *   ld_passes_out: LD passes (full sweeps over all owned LD bytes) performed */
/* MLE prior update (--prior-update mle, src/sgvamp.py:139-194).  The host runs
 * the reference's scipy.optimize.fsolve on Lagrangian_der; these two calls
 * compute its device-side parts over all markers and cohorts (the current r1
 * vectors).  L = mixture components including the spike, sigma2[L] the
 * component variances (sigma2[0] = 1e-16, :169-171).
 * exp_max (:152): max over (k, m, l) of (-r1_km^2 / 2) / (sigma2_l + 1/gam1_k).
 * sums[l] (:155-158): sum over k, m of a_k p_kml / sum_l' p_kml' omega_l', with
 * p_kml = exp((-r1_km^2 / 2) / v_kl - exp_max) / sqrt(v_kl). */
int sgv_mle_exp_max(sgv_ctx* ctx, const double* gam1s /* K */, int L, const double* sigma2,
                    double* exp_max);
int sgv_mle_terms(sgv_ctx* ctx, const double* a /* K */, const double* gam1s /* K */, int L,
                  const double* sigma2 /* L */, const double* omega /* L */, double exp_max,
                  double* sums /* L */);
/* The whole MLE prior update in the library, src/sgvamp.py:162-194: x0 from
 * lam, omegas (nslab of them) and gam (*gam_io NaN = the reference's None: x0[-1]
 * = 1), sgv_fsolve on Lagrangian_der (:139-160, the sums from sgv_mle_terms),
 * then the reference's acceptance tests and normalisation.  *status_out: 0 =
 * lam_io, omegas_io, gam_io updated; SGV_MLE_NOT_CONVERGED (fsolve's ier != 1)
 * or SGV_MLE_NEGATIVE (a non-positive mixture weight): nothing changed, the
 * reference's "No prior update!" cases. */
#define SGV_MLE_NOT_CONVERGED 1
#define SGV_MLE_NEGATIVE 2
int sgv_mle_update(sgv_ctx* ctx, const double* gam1s /* K */, const double* a /* K */, int nslab,
                   const double* sigmas /* nslab */, double* lam_io, double* omegas_io,
                   double* gam_io, int* status_out);

/* scipy.optimize.fsolve(fcn, x0, full_output=True) with its defaults (MINPACK
 * hybrd: xtol 1.49012e-08, maxfev 200 (n + 1), forward-difference Jacobian with
 * epsfcn = machine epsilon, factor 100, automatic scaling), host only: fcn
 * writes F(x) to fvec and returns 0, or a negative value to stop the solver.
 * x_io: x0 in, the last accepted iterate out; fvec_out (may be null): F there;
 * *nfev_out (may be null): function evaluations.  Returns MINPACK's info
 * (1 = converged, 2-5 = the other terminations, < 0 = fcn's stop value, 0 =
 * bad arguments) -- the reference's `ier` (src/sgvamp.py:179-181). */
/* The MLE update's Lagrange multiplier that SGV_STEP_MLE steps use and update
 * (the reference's self.gam, src/sgvamp.py:31,178,194; NaN = None). */
int sgv_set_mle_gam(sgv_ctx* ctx, double gam);

typedef int (*sgv_fsolve_fn)(void* user, int n, const double* x, double* fvec);
int sgv_fsolve(int n, sgv_fsolve_fn fcn, void* user, double* x_io, double* fvec_out,
               int* nfev_out);

/* The per-iteration output vectors without a host wait (src/sgvamp.py:281,283):
 * sgv_outputs_begin queues this rank's slices of xhat1 and r1[0..K-1] (unscaled,
 * marker order) into pinned slot 0, 1 or 2; sgv_outputs_wait -- callable from a
 * writer thread -- waits for that copy and returns the slot's buffer
 * [(K + 1) x M_local] doubles, valid until the slot is begun again ((K + 4) x
 * M_local after sgv_set_posterior_outputs(ctx, 1, thr), which see). */
int sgv_outputs_begin(sgv_ctx* ctx, int slot);
int sgv_outputs_wait(sgv_ctx* ctx, int slot, double** data);

int sgv_lmmse(sgv_ctx* ctx, int it, const double* gamw, const double* gam2,
              const double* alpha1, const double* alpha2_prev, const int8_t* probes,
              int cg_maxit, double rtol, int lmmse_damp, double rho, int learn_gamw,
              double* out, int* cg_out, int* ld_passes_out);

/* Metrics src/sgvamp.py:379-387: out[0] = <xhat1, x0>, out[1] = |xhat1|^2,
 * out[2] = |xhat1 - x0|^2, out[3] = |x0|^2 (global sums). */
int sgv_metrics(sgv_ctx* ctx, double* out4);
/* Split form of sgv_metrics: begin queues the kernel and the ordered reduction
 * (call after sgv_denoise; xhat1/x0 must not change before end), end waits for
 * it and returns the same 4 sums.  Lets the host skip a sync per iteration. */
int sgv_metrics_begin(sgv_ctx* ctx);
int sgv_metrics_end(sgv_ctx* ctx, double* out4);

/* ---- operator seam, exposed for tests ------------------------------------ */

/* y = R_s v for LD matrix `ld` over the rank's blocks (one LD pass, up to 16
 * columns).  v, y: [ncol][M_local] host, dense.  Replaces A.matvec inside
 * scipy cg (src/sgvamp.py:316,332) and R @ x (:352,359). */
int sgv_ld_matvec(sgv_ctx* ctx, int ld, int ncol, const double* v, double* y);

/* One LD pass over the RAW R of matrix ld (the ridge is NOT applied: the caller
 * folds it into c1/c2 as the solver does) with the whole fused epilogue:
 *   out_j  = c1[j] (R in_j) + c2[j] in_j
 *   yout_j = ys1 (R in_j) + ys0 in_j          for j in yout_mask
 *   dots[j] = sum_i w_j[i] out_j[i]           for j in dot_mask (the pass's
 *             partials through the ordered reduction the CG uses)
 * in, out, yout, w: [ncol][M_local] host, dense; c1, c2, dots: [ncol]; ncol 1..16.
 * w == NULL with dot_mask != 0: dot_j aliases in_j (the CG's p.q, same pointer).
 * run: -1 = PassArgs::run null; 0 / 1 = a device word holding that value is
 * passed as PassArgs::run.  out and yout are uploaded from the caller's buffers
 * first, so a no-op pass must return them unchanged (dots are unspecified then,
 * as are the dots of columns outside dot_mask). */
int sgv_ld_pass_ex(sgv_ctx* ctx, int ld, int ncol, const double* in, const double* c1,
                   const double* c2, const double* w, uint32_t dot_mask, uint32_t yout_mask,
                   double ys1, double ys0, int run, double* out, double* yout, double* dots);

/* Batched scipy-1.15.3 CG on (c1 R_s + c2 I) x = b for ncol columns sharing LD
 * `ld` (operator seam con_grad, src/sgvamp.py:7).  x: in = x0, out = solution.
 * iters_out/info_out [ncol]. */
int sgv_cg_solve(sgv_ctx* ctx, int ld, int ncol, const double* c1, const double* c2,
                 const double* b, double* x, int maxiter, double rtol, int* iters_out,
                 int* info_out);

/* ---- timing -------------------------------------------------------------- */
/* Summed over LD passes since the last reset (HIP events on the ctx stream):
 * t[0] = kernel time (ms), t[1] = passes, t[2] = LD bytes read (the stored
 * bytes: n^2*8 dense, sum over panels H*(n - r0)*8 packed, * 4 for a block
 * stored as f32: sgv_set_ld_precision), t[3] = RHS bytes
 * (2 * ncol * M_local * 8), t[4] = dense-equivalent LD bytes (n^2*8),
 * t[5] = packed-pass partial-buffer bytes (written + read), t[6] = the passes'
 * algorithmic flops (2 per multiply-add: each column's row part over every
 * stored element, and its transpose part over the packed elements right of
 * each panel's diagonal block), t[7] / t[8] / t[9] = flops / kernel ms / passes
 * of the 9..16-column passes (f64 16x16x4 MFMA: their bound is the matrix core).
 * Writes min(cap, SGV_TIMERS_N) values (a caller built against a shorter list
 * passes its own length and gets that prefix); cap < 0 is an error.
 * reset != 0 zeroes. */
#define SGV_TIMERS_N 10
int sgv_timers(sgv_ctx* ctx, double* t, int cap, int reset);
/* Cross-rank exchange counters since the last reset (the bcast/all-gather of
 * src/sgvamp.py:228-233 and the CG/EM scalar reductions that replace it):
 * out[0] = all-gathers issued, out[1] = ms spent in them (RCCL: HIP events
 * around each ncclAllGather on the ctx stream, the wait for the slowest peer
 * included; host exchange: wall time of the callback), out[2] = bytes this rank
 * contributed, out[3] = the last EM prior loop's mode (1 replicated: r1
 * all-gathered once per loop; 0 one exchange per EM step; -1 no communicator or
 * no loop yet), out[4] = the per-all-gather latency (us) the EM cost model uses,
 * out[5] = 1 RCCL, 2 host exchange, 0 none, out[6] / out[7] = EM loops run
 * replicated / per step, out[8] / out[9] = the last decision's predicted cost
 * (us) of the replicated / per-step loop, out[10] = the steps it predicted,
 * out[11] = ms the device idled between an exact-CG iteration's p update and
 * its passes, which the host enqueues once it has read the stop test (HIP
 * events), out[12] = the latency's source (0 default 25 us, 1 env
 * SGV_XCHG_LAT_US of rank 0, 2 sgv_exchange_probe), out[13] = 1 if the
 * replicated loop can run (K <= 32, <= 128 blocks in all), out[14] / out[15] =
 * ms / count of the device-driven EM prior loops (HIP events from the loop's
 * first enqueue to its last step: the cost the model predicts in out[8..9]).
 * Writes min(cap, SGV_EXCHANGE_STATS_N) values; cap < 0 is an error.  reset != 0
 * zeroes out[0..2], out[6..7], out[11] and out[14..15]. */
#define SGV_EXCHANGE_STATS_N 16
int sgv_exchange_stats(sgv_ctx* ctx, double* out, int cap, int reset);

/* Who this context's exchange talks to, for a launch to prove its topology:
 * out[0] = transport (0 none, 1 RCCL, 2 host exchange), out[1] = ranks in the
 * communicator (RCCL: ncclCommCount; host: the nranks given), out[2] = this
 * rank in it (RCCL: ncclCommUserRank), out[3] = the HIP device the context runs
 * on (RCCL: ncclCommCuDevice), out[4] = the nranks the context was given.
 * Writes min(cap, SGV_COMM_INFO_N) values; pci_bus_id (if not null) receives
 * the device's PCI bus id ("0000:xx:00.0", NUL-terminated, at most pci_len
 * bytes). */
#define SGV_COMM_INFO_N 5
int sgv_comm_info(sgv_ctx* ctx, int* out, int cap, char* pci_bus_id, int pci_len);

/* Measure the per-all-gather latency of this job's exchange (the CG's ordered
 * reduction of 16 values: per-block sums, all-gather, ordered total; `reps`
 * times on the ctx stream) and make the maximum over ranks the EM cost model's
 * latency on every rank.  Collective (every rank, between steps); *us_out =
 * the agreed latency in us (0 without a communicator).  The probe's
 * all-gathers are not counted in sgv_exchange_stats. */
int sgv_exchange_probe(sgv_ctx* ctx, int reps, double* us_out);

/* The EM exchange cost model alone (host arithmetic, no device): predicted us
 * of one EM loop of `steps` enqueued steps over `cohort_markers` = K x M on
 * `nranks` ranks with a per-all-gather latency of `latency_us`; out2[0] =
 * replicated (one r1 all-gather, the loop over all markers on every rank;
 * src/sgvamp.py:228-259), out2[1] = one exchange per EM step.  The library
 * runs the cheaper (sgv_exchange_stats out[3], out[8..10]). */
int sgv_em_cost_model(double cohort_markers, int nranks, double latency_us, double steps,
                      double* out2);

/* The kernel form the next pass of ncol columns (1..16) over LD matrix ld would
 * take, as ints: the decision of csrc/pass_form.cpp on this context's plan,
 * sgv_set_mfma_min and the pass switches as a pass reads them (DESIGN.md
 * Appendix B).  Builds the plan's tables if a block changed, as a pass would;
 * launches nothing else.  Writes min(cap, SGV_PF_N) values:
 * form[SGV_PF_KIND]: how the packed blocks run -- SGV_KIND_NONE (no packed
 *   block), _VALU (the packed VALU pass, chunk class form[SGV_PF_VALU_CLASS]),
 *   _STRIP4 (4-wave 512-column strips), _PAIR (wave-pair strips), _WIDE
 *   (1,024-column strips on the dense triangles; the other packed blocks, if
 *   any, behind them as form[SGV_PF_REST_KIND] = _STRIP4 / _PAIR), _STRIP16
 *   (16x16x4 strips, 9-16 columns), _WALK (band walks);
 * [SGV_PF_LOAD_FORM]: bytes per lane of the MFMA kernels' matrix loads, 1 = 8 B
 *   (every f64 matrix), 2 = 16 B; [SGV_PF_FIN_FORM]: the strip finalize, 1 or 4
 *   threads per panel row (0: none runs); [SGV_PF_PK_WIDTH] / [SGV_PF_PK_PAIRED]:
 *   the packed right-hand sides' row width in doubles and column order;
 * [SGV_PF_DENSE]: the dense row-group kernel runs; [SGV_PF_SIDE] /
 *   [SGV_PF_REST_SIDE]: the set's finalizes overlap its strips on a second
 *   stream; [SGV_PF_MFMA16]: the pass counts in sgv_timers t[7..9];
 *   [SGV_PF_IDLE_EXIT]: the wide kernel's idle waves leave at the start. */
#define SGV_KIND_NONE 0
#define SGV_KIND_VALU 1
#define SGV_KIND_STRIP4 2
#define SGV_KIND_PAIR 3
#define SGV_KIND_WIDE 4
#define SGV_KIND_STRIP16 5
#define SGV_KIND_WALK 6
#define SGV_KIND_FACTOR 7   /* a factor matrix (sgv_geno_ld_factor): the VALU f64 kernels of
                             * csrc/geno_factor.hip at every column count; every other field
                             * of the form is 0 (valu_class -1); never sgv_pass_form_model's answer */
#define SGV_PF_KIND 0
#define SGV_PF_VALU_CLASS 1
#define SGV_PF_REST_KIND 2
#define SGV_PF_LOAD_FORM 3
#define SGV_PF_FIN_FORM 4
#define SGV_PF_PK_WIDTH 5
#define SGV_PF_PK_PAIRED 6
#define SGV_PF_DENSE 7
#define SGV_PF_SIDE 8
#define SGV_PF_REST_SIDE 9
#define SGV_PF_MFMA16 10
#define SGV_PF_IDLE_EXIT 11
#define SGV_PF_N 12
int sgv_ld_pass_form(sgv_ctx* ctx, int ld, int ncol, int32_t* form, int cap);

/* The same decision on the caller's values (host arithmetic, no device, no
 * context): shape[SGV_PS_N] is what a plan holds -- the packed blocks' element
 * type (64 / 32), whether it has dense row groups, packed panels, walk tables,
 * wide strips, 512-column strips beside the wide ones ("rest"), ragged / pair
 * (0 none, 1 by the launch-tail model, 2 forced) of the 512-column strip set
 * and of rest, whether the wide kernel's idle waves leave, and the block groups
 * of the three strip sets; switches[SGV_SW_N] the pass switches as read: -1
 * unset, else the switch's value (SGV_BAND_WALK 0, SGV_F32_WALK 1, SGV_MF_WIDE
 * and SGV_MF_PAIR 0 / 1, SGV_MF_WIDE_IDLE 0, SGV_F32_FORM 1 / 2, SGV_FIN_FORM
 * 1 / 4; anything else is SGV_ERR_ARG). */
#define SGV_PS_BITS 0
#define SGV_PS_DENSE 1
#define SGV_PS_PACKED 2
#define SGV_PS_WALKS 3
#define SGV_PS_WIDE 4
#define SGV_PS_REST 5
#define SGV_PS_RAGGED 6
#define SGV_PS_PAIR 7
#define SGV_PS_REST_RAGGED 8
#define SGV_PS_REST_PAIR 9
#define SGV_PS_WIDE_IDLE 10
#define SGV_PS_NGRP 11
#define SGV_PS_WIDE_NGRP 12
#define SGV_PS_REST_NGRP 13
#define SGV_PS_N 14
#define SGV_SW_BAND_WALK 0
#define SGV_SW_F32_WALK 1
#define SGV_SW_MF_WIDE 2
#define SGV_SW_MF_PAIR 3
#define SGV_SW_MF_WIDE_IDLE 4
#define SGV_SW_F32_FORM 5
#define SGV_SW_FIN_FORM 6
#define SGV_SW_N 7
int sgv_pass_form_model(const int32_t* shape, const int32_t* switches, int mfma_min, int ncol,
                        int32_t* form, int cap);

/* Synchronise the ctx stream. */
int sgv_sync(sgv_ctx* ctx);

/* The device's streaming-read rate (context for the LD passes' roofline): a
 * temporary buffer of `bytes` (rounded down to 256 KiB) read once per repeat,
 * every workgroup its own contiguous 256 KiB with 16-B nontemporal loads; the
 * best of `reps` repeats in GB/s (1e9 B/s) -> *gbps. */
int sgv_read_bw(sgv_ctx* ctx, int64_t bytes, int reps, double* gbps);

#ifdef __cplusplus
}
#endif
#endif /* SGVAMP_HIP_H */
