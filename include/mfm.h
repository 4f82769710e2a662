/* libmfm_hip -- C ABI of the MI355X-native Markovian Flow Matching inner loop.
 *
 * This is the drop-in boundary for the hot path of albcab/mfm (reference paths relative to the root of that repository):
 * every entry point replaces one jit-compiled XLA executable (or a piece of one) that the reference's `run()` loop
 * (exe_flow_matching.py:432-449) calls.  The reference has no FFI of its own (it is pure Python on JAX); the
 * binding a maintainer adds is the ctypes layer in mfm_amd/_lib.py.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no C++/torch types.  Every function returns 0 on success and a negative
 *    MFM_E* code on failure; mfm_last_error() gives the message.  No exceptions or aborts cross the boundary.
 *  - Pointers named d_* are DEVICE pointers owned by the caller (e.g. torch.Tensor.data_ptr()); h_* are host
 *    pointers.  Chain state is row-major [n_chain_local, dim] float32; log-densities are float64 [n_chain_local].
 *  - The context owns the network parameters (canonical flat float32 vector + MFMA-packed copies), the AdamW
 *    state, all workspaces and remembers the HIP stream work is queued on.  Calls are asynchronous on that stream;
 *    mfm_sync() or any h_* output synchronises.  One context per GPU per process; not thread-safe.
 *  - PRNG keys are jax-style uint32[2] passed by value as two words; draws are indexed by GLOBAL chain id
 *    (chain_offset + local row) out of n_chain_total, so results do not depend on how chains are sharded.
 *
 * Canonical flat parameter layout (mfm_set_params / mfm_get_params / gradients): for Dense_0 .. Dense_7 in flax
 * creation order (exe_flow_matching.py:74-86): kernel [in][out] row-major, then bias [out].
 */
#ifndef MFM_H
#define MFM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mfm_ctx mfm_ctx;

enum { MFM_OK = 0, MFM_EINVAL = -1, MFM_EUNSUPPORTED = -2, MFM_ETOOLARGE = -3, MFM_EHIP = -4, MFM_ENOTARGET = -5 };

enum { MFM_PHI4 = 0, MFM_GMM = 1, MFM_LGCP = 2 };                 /* distributions.py:114,42,231 */
enum { MFM_FLOW_RWMH = 0, MFM_FLOW_IMH = 1 };                      /* exe_flow_matching.py:264-278 / :246-260 */
enum { MFM_FAMILY_AUTO = 0, MFM_FAMILY_TILE = 1, MFM_FAMILY_WIDE = 2 };
enum { MFM_ACT_RELU = 0, MFM_ACT_TANH = 1, MFM_ACT_ELU = 2, MFM_ACT_GELU = 3, MFM_ACT_SWISH = 4 };   /* exe_flow_matching.py:39-45 */

#define MFM_MAX_DEPTH 3
typedef struct mfm_config {
  int32_t dim;                 /* args.dim */
  int32_t fourier_dim;         /* args.fourier_dim  (multi_modal.py:156) */
  int32_t hidden_t[2];         /* args.hidden_t     (:179)  any positive width (zero-padded to 16 inside the library) */
  int32_t hidden_x[2];         /* args.hidden_x     (:178) */
  int32_t hidden_xt[2];        /* args.hidden_xt    (:180) */
  int32_t n_chain_local;       /* chains resident on this GPU (multiple of 16) */
  int32_t n_chain_total;       /* args.num_chain over all GPUs */
  int32_t chain_offset;        /* global id of local chain 0 */
  float grad_clip;             /* args.gradient_clip if dim > 128 else 0   (exe_flow_matching.py:351) */
  float sigma;                 /* args.sigma        (:155) */
  int32_t cond_flow;           /* args.cond_flow    (:162-163) */
  int32_t hutch;               /* args.hutchs       (:158) */
  double rtol, atol;           /* args.rtol / atol  (:207-208) */
  int32_t mxstep;              /* args.mxstep       (:209) */
  int32_t n_ts;                /* 5 for "4-mode", else 2 (exe_flow_matching.py:347) */
  /* optimizer (multi_modal.py:199-205) */
  double learning_rate, adam_b1, adam_b2, adam_eps, weight_decay, update_clip;
  int32_t learning_iter, warmup_steps;
  int32_t max_eval_samples;    /* largest n passed to mfm_fm_loss / mfm_vf_apply (0: n_chain_local) */
  int32_t kernel_family;       /* MFM_FAMILY_AUTO: fused 16-chain LDS tile kernels when the network fits them, else the wide
                                  family (per-layer MFMA GEMMs on HBM-resident activations: the "pines" widths of
                                  multi_modal.py:89-96); _TILE / _WIDE force one (ETOOLARGE if _TILE does not fit) */
  int32_t activation;          /* MFM_ACT_*: args.non_linearity (multi_modal.py:177; table exe_flow_matching.py:39-45).  relu, tanh and elu
                                  run on either kernel family; gelu and swish need stored pre-activations: wide family */
  double ref_std;              /* std of the flow's reference distribution IndepGaussian(dim, var): 1 for args.ref_dist = 'stdgauss',
                                  sqrt(5) for 'widegauss' (exe_flow_matching.py:48-54, distributions.py:80-97); 0 = 1 */
  int32_t n_chain_valid;       /* 0 = n_chain_local.  args.num_chain takes any integer (multi_modal.py:169); the kernels work on tiles of
                                  16 chains, so the host pads its shard to n_chain_local (a multiple of 16) and names here how many of
                                  those rows are chains: rows >= n_chain_valid are integrated like any other but contribute nothing to
                                  the flow-matching loss and its gradient (exe_flow_matching.py:171-178) */
  /* args.hidden_t / hidden_x / hidden_xt are lists of any length (multi_modal.py:178-180, nargs='+'; the loops at
     exe_flow_matching.py:74-85).  depth_* = 0 reads the two widths above (a two-layer branch).  1 .. MFM_MAX_DEPTH: that many hidden
     layers, widths hidden_*[0], hidden_*[1], then hidden_*3.  Anything but (2, 2, 2) runs on the wide family (one GEMM launch per
     layer): MFM_FAMILY_TILE then fails with MFM_EUNSUPPORTED. */
  int32_t depth_t, depth_x, depth_xt;
  int32_t hidden_t3, hidden_x3, hidden_xt3;
  /* BUILD-SIDE MODE, not in the reference (whose integrator is the adaptive Dopri5 of jax.experimental.ode.odeint,
     exe_flow_matching.py:345-349 -- ode_method = MFM_ODE_DOPRI5, the default): the CNF solves on ode_steps EQUAL steps of classical
     RK4 (MFM_ODE_RK4) or forward Euler (MFM_ODE_EULER), the "RK4/Euler ODE integrator" BASELINE.json's north star names -- no step-size
     controller, every chain takes the same steps.  Served by the shape-specialised solver (default widths, PhiFour, relu, hutch = 1:
     random-walk flow step and the transforms), the wide family (every other network depth or width, LGCP, the exact-trace solves of
     fused-family contexts at d >= 16: both flow-step modes and the transforms) and the d = 2 four-chain tiles (the mixtures without
     --hutch: both flow-step modes and the transforms).  Still MFM_EUNSUPPORTED at the first solve: the generic 16-chain tile (d = 2
     with hutch = 1, MFM_D2_TILE=16, MFM_TILE_EXACT=1, and the fused family's other shapes), the independent flow step on the
     shape-specialised tile, and mfm_debug_replay.  rtol / atol / mxstep are ignored in this mode; n_ts > 2 needs
     ode_steps % (n_ts - 1) == 0.  mfm_get_counters: field_evals = 4 (RK4) or 1 (Euler) x attempted steps. */
  int32_t ode_method, ode_steps;
} mfm_config;

#define MFM_ODE_DOPRI5 0
#define MFM_ODE_RK4 1
#define MFM_ODE_EULER 2

const char* mfm_last_error(void);
int mfm_version(void);

/* ---- lifetime ------------------------------------------------------------------------------------------------ */
int mfm_create(const mfm_config* cfg, mfm_ctx** out);
int mfm_destroy(mfm_ctx* ctx);
int mfm_set_stream(mfm_ctx* ctx, void* hip_stream);            /* hipStream_t; NULL = default stream */
int mfm_sync(mfm_ctx* ctx);
int mfm_num_params(const mfm_ctx* ctx);                        /* P_w + P_b */

/* ---- target (distributions.py) ---------------------------------------------------------------------------------
 * MFM_PHI4: h_params = {a, beta}                                    (PhiFour.__init__, :115-129; Dirichlet 0)
 *           or {a, beta, bc_kind, bc_value}: bc_kind 0 = Dirichlet, both ends held at bc_value (finite);
 *           1 = periodic ring, bc_value ignored.  Any other kind: MFM_EINVAL.
 *           or {a, beta, bc_kind, bc_value, dim_phys}: dim_phys 1 = the chain (exactly the four-double block), 2 = an L x L
 *           lattice in row-major order, site (r, c) = element r L + c, cfg.dim = L * L: coefficient a * L, the gradient term over
 *           the bonds of both axes, each closed by the boundary (periodic: both axes wrap; Dirichlet: a frame held at bc_value).
 *           dim_phys = 2 with a cfg.dim that is no perfect square, or any other dim_phys: MFM_EINVAL.
 * MFM_GMM : h_params = {n_modes, modes[K*d], stds[K*d], weights[K]} (GaussianMixture, :43-56; stds = sqrt(covs))
 * MFM_LGCP: h_params = {mu, poisson_a, log_norm, counts[d], Kinv[d*d]}  (LogGaussianCoxPines, :233-281) */
int mfm_set_target(mfm_ctx* ctx, int kind, const double* h_params, size_t n);

/* ---- network parameters (VectorFieldNet, exe_flow_matching.py:56-90,350-353) --------------------------------- */
int mfm_set_fourier(mfm_ctx* ctx, const float* h_fourier_random);              /* [fourier_dim] */
int mfm_set_params(mfm_ctx* ctx, const float* h_flat);                          /* canonical flat layout */
int mfm_get_params(mfm_ctx* ctx, float* h_flat);
int mfm_reset_optimizer(mfm_ctx* ctx);

/* ---- K1/K2: MALA kernel API (bblackjax/mcmc/mala.py) ------------------------------------------------------------ */
/* init (mala.py:51-54) vmapped as init_fn (exe_flow_matching.py:316): logdensity and gradient of the tempered target
 * beta * loglik + logprior at d_pos. */
int mfm_mala_init(mfm_ctx* ctx, const float* d_pos, double beta, double* d_logp, float* d_grad);
/* kernel (mala.py:86-118) vmapped with per-chain keys split(key, n_chain_total) (exe_flow_matching.py:303,313).
 * State is updated in place; the MALAInfo outputs may be NULL. */
int mfm_mala_step(mfm_ctx* ctx, uint32_t key0, uint32_t key1, double beta, double step_size, int textbook,
                  float* d_pos, double* d_logp, float* d_grad,
                  float* d_acceptance_rate, uint8_t* d_is_accepted, float* d_proposed_position,
                  float* d_proposed_weight);
/* the same kernel for a caller that vmaps over its OWN per-chain keys (bblackjax/smc/base.py:122-123 ->
 * tempered.py:126-137): d_keys is uint32[n_chain_local][2], chain b uses d_keys[b] where mfm_mala_step uses
 * split(key, n_chain_total)[chain_offset + b]. */
int mfm_mala_step_keys(mfm_ctx* ctx, const uint32_t* d_keys, double beta, double step_size, int textbook,
                       float* d_pos, double* d_logp, float* d_grad,
                       float* d_acceptance_rate, uint8_t* d_is_accepted, float* d_proposed_position,
                       float* d_proposed_weight);
/* n_steps steps of the same kernel in ONE call -- the scan of inference_loop0 (mcmc_utils.py:11-25) and the host loop of
 * tempered.py:126-137.  phi-four and mixture targets: one launch, the chain stays in registers between the steps, bit-identical
 * with n_steps single-step calls; the Cox process: n_steps launches of its step back to back on the context's stream, keys
 * derived on the device.  Draws are always made in line (prefetched draws are not consulted).
 * key_mode 0 (step-major): step j uses split(key, n_steps)[j] as mfm_mala_step uses its key; d_keys is ignored.
 * key_mode 1 (chain-major): d_keys is uint32[n_chain_local][2]; step j of chain b uses split(d_keys[b], n_steps)[j] as
 *   mfm_mala_step_keys uses a chain's key; key0 / key1 are ignored.
 * State is updated in place.  Optional outputs (NULL to skip): d_n_accepted int32[B], accepted steps; d_acc_sum double[B], sum
 * of the acceptance probabilities; the MALAInfo arrays of the LAST step; with thin >= 1 (n_steps % thin == 0, at least one of
 * the two pointers) the state after every step j with (j + 1) % thin == 0: d_traj_pos float[n_steps / thin][B][dim],
 * d_traj_logp double[n_steps / thin][B].  thin == 0 keeps no trajectory. */
int mfm_mala_run(mfm_ctx* ctx, int key_mode, uint32_t key0, uint32_t key1, const uint32_t* d_keys,
                 double beta, double step_size, int textbook, int32_t n_steps, int32_t thin,
                 float* d_pos, double* d_logp, float* d_grad,
                 int32_t* d_n_accepted, double* d_acc_sum,
                 float* d_acceptance_rate, uint8_t* d_is_accepted, float* d_proposed_position, float* d_proposed_weight,
                 float* d_traj_pos, double* d_traj_logp);
/* BUILD-SIDE MODE, not on the reference's MFM path (BASELINE.json's north star names a "MALA/HMC" step; the reference's loop uses
 * MALA only and vendors no hmc.py: SURVEY.md note 7): one Hamiltonian Monte Carlo step of every local chain as in blackjax's hmc
 * kernel (oracle/hmc.py restates it): momentum ~ N(0, I) from split(key, n_chain_total)[chain_offset + b] -> split(., 2)[0],
 * num_steps velocity-Verlet steps of size step_size on beta * loglik + logprior, accept with min(1, exp(H_0 - H_end)).  State
 * updated in place like mfm_mala_step; d_acceptance_rate / d_is_accepted may be null.  phi-four and mixture targets
 * (MFM_EUNSUPPORTED for the Cox process). */
int mfm_hmc_step(mfm_ctx* ctx, uint32_t key0, uint32_t key1, double beta, double step_size, int32_t num_steps,
                 float* d_pos, double* d_logp, float* d_grad, float* d_acceptance_rate, uint8_t* d_is_accepted);
/* the same step for a caller that vmaps over its OWN per-chain keys, as mfm_mala_step_keys: d_keys is uint32[n_chain_local][2],
 * chain b uses d_keys[b] where mfm_hmc_step uses split(key, n_chain_total)[chain_offset + b]. */
int mfm_hmc_step_keys(mfm_ctx* ctx, const uint32_t* d_keys, double beta, double step_size, int32_t num_steps,
                      float* d_pos, double* d_logp, float* d_grad, float* d_acceptance_rate, uint8_t* d_is_accepted);
/* n_steps HMC steps (each of num_steps leapfrog steps) in ONE launch, what mfm_mala_run is to mfm_mala_step: the chain stays in
 * registers between the steps, bit-identical with n_steps single-step calls.
 * key_mode 0 (step-major): step j uses split(key, n_steps)[j] as mfm_hmc_step uses its key; d_keys is ignored.
 * key_mode 1 (chain-major): d_keys is uint32[n_chain_local][2]; step j of chain b uses split(d_keys[b], n_steps)[j] as
 *   mfm_hmc_step_keys uses a chain's key; key0 / key1 are ignored.
 * State is updated in place.  Optional outputs (NULL to skip): d_n_accepted int32[B], accepted steps; d_acc_sum double[B], sum of
 * the acceptance probabilities; d_acceptance_rate / d_is_accepted of the LAST step; with thin >= 1 (n_steps % thin == 0, at least
 * one of the two pointers) the state after every step j with (j + 1) % thin == 0: d_traj_pos float[n_steps / thin][B][dim],
 * d_traj_logp double[n_steps / thin][B].  thin == 0 keeps no trajectory.  phi-four and mixture targets (MFM_EUNSUPPORTED for the
 * Cox process, as mfm_hmc_step). */
int mfm_hmc_run(mfm_ctx* ctx, int key_mode, uint32_t key0, uint32_t key1, const uint32_t* d_keys,
                double beta, double step_size, int32_t num_steps /* leapfrog steps per HMC step */,
                int32_t n_steps, int32_t thin,
                float* d_pos, double* d_logp, float* d_grad,
                int32_t* d_n_accepted, double* d_acc_sum,
                float* d_acceptance_rate, uint8_t* d_is_accepted,
                float* d_traj_pos, double* d_traj_logp);
/* BUILD-SIDE MODE like the HMC entry points: one transition of the No-U-turn sampler of every local chain (nuts.hip; tests/nuts_ref.py
 * restates it).  Multinomial NUTS in the iterative, checkpointed form: momentum and leapfrog as mfm_hmc_step's (the installed inverse mass
 * included, mfm_hmc_set_inverse_mass), the tree doubled at most max_tree_depth (1 .. 16) times in directions drawn from the chain's key,
 * a leaf divergent when its energy exceeds the start's by more than divergence_threshold (> 0) or is NaN; the tree's proposal becomes
 * the state, in place.  Info per chain (each may be NULL): d_depth int32, the completed doublings; d_num_leapfrog int32; d_is_turning /
 * d_is_divergent uint8; d_acceptance_rate double, the mean of min(1, exp(H0 - H)) over every leaf integrated; d_energy double, the
 * proposal's.  phi-four and mixture targets at dim <= 256: MFM_EUNSUPPORTED for the Cox process and for a larger dim.  The tree's
 * U-turn checkpoints live in LDS; a max_tree_depth whose checkpoints exceed a CU's LDS returns MFM_EINVAL naming the largest that fits.
 * A rejected call touches nothing. */
int mfm_nuts_step(mfm_ctx* ctx, uint32_t key0, uint32_t key1, double beta, double step_size, int32_t max_tree_depth,
                  double divergence_threshold, float* d_pos, double* d_logp, float* d_grad,
                  int32_t* d_depth, int32_t* d_num_leapfrog, uint8_t* d_is_turning, uint8_t* d_is_divergent,
                  double* d_acceptance_rate, double* d_energy);
/* the same transition on the caller's OWN per-chain keys, uint32[n_chain_local][2], as mfm_hmc_step_keys */
int mfm_nuts_step_keys(mfm_ctx* ctx, const uint32_t* d_keys, double beta, double step_size, int32_t max_tree_depth,
                       double divergence_threshold, float* d_pos, double* d_logp, float* d_grad,
                       int32_t* d_depth, int32_t* d_num_leapfrog, uint8_t* d_is_turning, uint8_t* d_is_divergent,
                       double* d_acceptance_rate, double* d_energy);
/* n_steps NUTS transitions in ONE launch, the chain resident in registers: bit-identical with n_steps single-step calls.  key_mode,
 * keys, thin, d_traj_pos / d_traj_logp and their checks as mfm_hmc_run's.  Per-chain totals (each may be NULL): d_leapfrog_sum int64,
 * leapfrog steps; d_acc_sum double, the sum of the transitions' acceptance rates; d_n_divergent int32, divergent transitions;
 * d_depth_sum int32, the sum of the depths.  The info arrays take the LAST transition's. */
int mfm_nuts_run(mfm_ctx* ctx, int key_mode, uint32_t key0, uint32_t key1, const uint32_t* d_keys,
                 double beta, double step_size, int32_t max_tree_depth, double divergence_threshold,
                 int32_t n_steps, int32_t thin,
                 float* d_pos, double* d_logp, float* d_grad,
                 int64_t* d_leapfrog_sum, double* d_acc_sum, int32_t* d_n_divergent, int32_t* d_depth_sum,
                 int32_t* d_depth, int32_t* d_num_leapfrog, uint8_t* d_is_turning, uint8_t* d_is_divergent,
                 double* d_acceptance_rate, double* d_energy,
                 float* d_traj_pos, double* d_traj_logp);
/* The launch geometry of the NUTS kernels (step, run and warmup) at (dim, max_tree_depth); needs no context and no GPU.  *h_waves: the
 * chains per workgroup (1 .. 4), the count that puts the most chains on a CU, the larger count on a tie; *h_lds_bytes: the dynamic LDS of
 * one workgroup, the MALA rows and gradient scratch followed by h_waves checkpoint slabs of (max_tree_depth - 1) * 2 * dim doubles;
 * *h_workgroups_per_cu: how many such workgroups a CU's 163840 B hold.  Errors as mfm_nuts_step's for max_tree_depth and dim. */
int mfm_nuts_launch_plan(int32_t dim, int32_t max_tree_depth, int32_t* h_waves, int32_t* h_lds_bytes, int32_t* h_workgroups_per_cu);
/* STEP-SIZE WARMUP: n_steps steps of the HMC step (mfm_hmc_warmup) or of the MALA step under the textbook rule (mfm_mala_warmup) in
 * ONE launch, as mfm_hmc_run / mfm_mala_run (chain resident in registers, key_mode 0 / 1 and their key schedules), in which every
 * chain adapts its OWN step size by Nesterov dual averaging on its acceptance probability (Hoffman & Gelman 2014, algorithm 5).
 * The constants are fixed: t0 = 10, gamma = 0.05, kappa = 0.75, mu = log(10 * step0).  Per chain, in float64:
 *     x_0 = log(step0), Hbar_0 = 0, xbar_0 = 0;   for m = 1 .. n_steps:
 *     1. the step runs with eps_m = exp(x_{m-1}) (eps_1 = step0 itself, not exp(log(step0))) and has the acceptance probability
 *        p_m: the float64 value before any rounding for an info array, 0 for a NaN energy difference;
 *     2. Hbar_m = (1 - 1 / (m + t0)) * Hbar_{m-1} + (target_accept - p_m) / (m + t0);
 *     3. x_m = mu - (sqrt(m) / gamma) * Hbar_m, clamped to [log(step0) - 23, log(step0) + 23] so that eps stays finite and positive;
 *     4. eta = 1 / (sqrt(m) * sqrt(sqrt(m)))   (m^-kappa from two correctly rounded square roots: a host restatement agrees);
 *     5. xbar_m = eta * x_m + (1 - eta) * xbar_{m-1}.
 * Outputs per chain: d_step_avg[b] = exp(xbar_n), the RESULT (required); d_step_last[b] = exp(x_n) (or NULL); d_step_traj
 * double[n_steps][B], the step size USED at each step (or NULL); d_n_accepted / d_acc_sum as mfm_hmc_run.  Step m of chain b has the
 * bits of a single-step call (mfm_hmc_step_keys; mfm_mala_step_keys with textbook = 1) with the scalar step size d_step_traj[m][b]
 * and the same step key.  Chains do not communicate: the caller pools the results, e.g. exp(mean(log d_step_avg)) over the rows
 * below n_chain_valid (padding rows are stepped like any other).  State is updated in place.
 * target_accept must lie strictly inside (0, 1).  The Cox process returns MFM_EUNSUPPORTED from both (HMC: as mfm_hmc_step; MALA: its
 * run is a sequence of tile launches with a by-value step size).  mfm_mala_warmup with textbook = 0 returns MFM_EINVAL: the
 * as-written rule accepts with min(1, 1 / alpha), its acceptance does not fall as the step grows, and dual averaging has nothing to
 * steer by. */
int mfm_hmc_warmup(mfm_ctx* ctx, int key_mode, uint32_t key0, uint32_t key1, const uint32_t* d_keys,
                   double beta, double step0, int32_t num_steps /* leapfrog steps per HMC step */,
                   int32_t n_steps, double target_accept,
                   float* d_pos, double* d_logp, float* d_grad,
                   double* d_step_avg, double* d_step_last,
                   int32_t* d_n_accepted, double* d_acc_sum,
                   double* d_step_traj);
int mfm_mala_warmup(mfm_ctx* ctx, int key_mode, uint32_t key0, uint32_t key1, const uint32_t* d_keys,
                    double beta, double step0, int textbook,
                    int32_t n_steps, double target_accept,
                    float* d_pos, double* d_logp, float* d_grad,
                    double* d_step_avg, double* d_step_last,
                    int32_t* d_n_accepted, double* d_acc_sum,
                    double* d_step_traj);
/* DIAGONAL MASS MATRIX of the HMC entry points (blackjax's inverse_mass_matrix as a vector).  h_inv_mass is a HOST vector, the diagonal
 * minv of M^-1.  With it a step draws the momentum p_j = n_j / sqrt(minv_j) from the same normal draws n_j, has the energy
 * H = -logp + sum_j minv_j p_j^2 / 2, and drifts by x_j += step_size * minv_j * p_j; kicks and the accept rule are unchanged.
 * n == dim installs the vector on the context: every later mfm_hmc_step, mfm_hmc_step_keys, mfm_hmc_run and mfm_hmc_warmup call runs the
 * mass instances of its kernel with it (a vector of ones gives, bit for bit, what the call gives with none installed).  n == 0 with
 * h_inv_mass == NULL returns to unit mass and the unit instances.  Any other n, or an entry that is not finite and positive, returns
 * MFM_EINVAL naming inv_mass, and the context keeps what it had.  The call waits for the context's stream.
 * mfm_hmc_get_inverse_mass: h_out double[dim] (or NULL) takes the installed vector, ones when none is; *h_is_set (or NULL) 1 or 0. */
int mfm_hmc_set_inverse_mass(mfm_ctx* ctx, const double* h_inv_mass, int32_t n);
int mfm_hmc_get_inverse_mass(mfm_ctx* ctx, double* h_out /* [dim] */, int32_t* h_is_set);
/* ONE WINDOW of a mass-matrix adaptation: mfm_hmc_warmup, which also leaves the sums a variance estimate needs in place of a trajectory.
 * After every step the chain's state after accept / reject, the float32 position as a double, is added in step order to
 * d_pos_sum double[B][dim] and its (exact) square to d_pos_sumsq double[B][dim]; both are required and are overwritten.  It always runs
 * the mass instances, with the context's vector, or with ones when none is installed: everything else it writes then has
 * mfm_hmc_warmup's bits.  Arguments and errors otherwise as mfm_hmc_warmup. */
int mfm_hmc_warmup_window(mfm_ctx* ctx, int key_mode, uint32_t key0, uint32_t key1, const uint32_t* d_keys,
                          double beta, double step0, int32_t num_steps /* leapfrog steps per HMC step */,
                          int32_t n_steps, double target_accept,
                          float* d_pos, double* d_logp, float* d_grad,
                          double* d_step_avg, double* d_step_last,
                          int32_t* d_n_accepted, double* d_acc_sum,
                          double* d_step_traj,
                          double* d_pos_sum, double* d_pos_sumsq);
/* mfm_hmc_run with ONE LEAPFROG COUNT PER STEP: d_num_steps is int32[n_steps] in device memory, every entry in [1, 100000] (the host
 * cannot see the array: the kernel clamps an entry into that range), and step j has the bits of mfm_hmc_step / mfm_hmc_step_keys with
 * num_steps = d_num_steps[j] on mfm_hmc_run's step key.  The count is the same for every chain of a step, so the chains stay in lock
 * step: this is the sampler mfm_chees_warmup adapts, the host filling the array from the jitter sequence.  Everything else -- key_mode,
 * keys, tallies, thin and the trajectory, the checks and their order, with d_num_steps (non-null) in num_steps' place -- is
 * mfm_hmc_run's.  d_total_leapfrog (or NULL): int64 scalar, the leapfrog steps of one chain over the run, the sum of the entries. */
int mfm_hmc_run_lengths(mfm_ctx* ctx, int key_mode, uint32_t key0, uint32_t key1, const uint32_t* d_keys,
                        double beta, double step_size, const int32_t* d_num_steps /* [n_steps] leapfrog steps of each HMC step */,
                        int32_t n_steps, int32_t thin,
                        float* d_pos, double* d_logp, float* d_grad,
                        int32_t* d_n_accepted, double* d_acc_sum,
                        float* d_acceptance_rate, uint8_t* d_is_accepted,
                        float* d_traj_pos, double* d_traj_logp,
                        int64_t* d_total_leapfrog);
/* MICROCANONICAL LANGEVIN MONTE CARLO (MCLMC: Robnik, De Luca, Silverstein & Seljak 2023; Robnik & Seljak 2024; blackjax.mclmc) -- a
 * BUILD-SIDE MODE like mfm_hmc_*; tests/mclmc_ref.py restates it in float64 and is the definition.  A chain is (d_pos, d_logp, d_grad)
 * as mfm_mala_init leaves them plus a UNIT momentum d_momentum, double[n_chain_local][dim].  One step of size step_size is the
 * palindromic schedule B(b_0 eps) { A(a_k eps), value and gradient, B(b_k eps) }_k (integrator 0: leapfrog, one gradient; 1: McLachlan's
 * minimal-norm scheme, two) of the exact momentum flow B and the drift A, then the partial refresh u <- (u + nu z) / |u + nu z| with
 * nu = sqrt((exp(2 step_size / L) - 1) / dim) and z from split(chain key, 2)[0]; L = +inf gives nu = 0 and draws nothing.  There is NO
 * accept test: every step is taken; its energy change dE = sum dK - (logp_end - logp_start) is reported and the chain is not repaired
 * when it is not finite.  The calls only enqueue; shards (n_chain_total != n_chain_local) are served.
 * Checks, in this order, a rejected call touching nothing: state pointers (and keys / key_mode / n_steps / thin as mfm_hmc_run);
 * MFM_EUNSUPPORTED for the Cox process (mfm_hmc_step's message) and for an installed inverse mass (unit metric only); MFM_EINVAL naming
 * the argument for dim < 2, step_size not positive, L not positive or NaN, L so small that nu overflows, integrator outside {0, 1}.
 * mfm_mclmc_init: u_b = z / |z|, z_j = normal64(split(key, n_chain_total)[chain_offset + b], j, dim). */
int mfm_mclmc_init(mfm_ctx* ctx, uint32_t key0, uint32_t key1, double* d_momentum);
/* one step; chain b uses split(key, n_chain_total)[chain_offset + b] (or d_keys[b]).  d_energy_change / d_kinetic_change: double[B], may be null */
int mfm_mclmc_step(mfm_ctx* ctx, uint32_t key0, uint32_t key1, double beta, double step_size, double L, int integrator,
                   float* d_pos, double* d_logp, float* d_grad, double* d_momentum, double* d_energy_change, double* d_kinetic_change);
int mfm_mclmc_step_keys(mfm_ctx* ctx, const uint32_t* d_keys, double beta, double step_size, double L, int integrator,
                        float* d_pos, double* d_logp, float* d_grad, double* d_momentum, double* d_energy_change, double* d_kinetic_change);
/* n_steps steps in ONE launch, bit-identical with n_steps single-step calls; key_mode, the step keys, thin and the trajectory layout are
 * mfm_hmc_run's.  Optional outputs (NULL to skip): d_de_sum / d_de_sumsq double[B], the sums of dE and dE^2 over the steps in step
 * order; d_n_nonfinite int32[B], the steps whose dE is not finite; d_energy_trace double[n_steps][B], every step's dE. */
int mfm_mclmc_run(mfm_ctx* ctx, int key_mode, uint32_t key0, uint32_t key1, const uint32_t* d_keys,
                  double beta, double step_size, double L, int integrator, int32_t n_steps, int32_t thin,
                  float* d_pos, double* d_logp, float* d_grad, double* d_momentum,
                  double* d_de_sum, double* d_de_sumsq, int32_t* d_n_nonfinite, double* d_energy_trace,
                  float* d_traj_pos, double* d_traj_logp);
/* GENERALIZED HMC WITH PERSISTENT MOMENTUM (GHMC: Horowitz 1991, with the non-reversible slice accept; Hoffman & Sountsov 2022;
 * blackjax.ghmc) -- a BUILD-SIDE MODE like mfm_hmc_*; tests/ghmc_ref.py restates it in float64 and is the definition.  A chain is
 * (d_pos, d_logp, d_grad) as mfm_mala_init leaves them plus a momentum d_momentum, double[n_chain_local][dim], and a slice variable
 * d_slice, double[n_chain_local], in (-1, 1).  Parameters: step_size eps > 0, alpha in (0, 1], delta >= 0, and d_inverse_mass, DEVICE
 * double[dim], the diagonal of the inverse mass matrix minv (NULL: unit metric).  The mass is the CALL's argument: the inverse mass
 * installed by mfm_hmc_set_inverse_mass is not read.  One transition, with the chain key kb:
 *   1. p <- sqrt(1 - alpha) p + sqrt(alpha) n / sqrt(minv), n_j = normal64(split(kb, 2)[0], j, dim), the draw of mfm_hmc_step
 *   2. s <- fmod(s + 1 + delta, 2) - 1 (a deterministic drift)
 *   3. H_0 = -logp + 1/2 sum_j minv_j p_j^2
 *   4. ONE velocity-Verlet step as mfm_hmc_step makes it: half kick p += eps/2 g, drift x <- (float)(x + eps minv p), value and
 *      gradient at x, half kick
 *   5. H_1 likewise; dH = H_1 - H_0
 *   6. accept iff |s| <= exp(-dH); a NaN dH rejects.  Accepted: the state becomes the end point, p <- p_end, s <- s exp(dH).
 *      Rejected: x, logp and grad are kept, p <- -p (the REFRESHED momentum of 1., negated), s is kept
 *   7. info: acceptance_rate = min(1, exp(-dH)) (float), is_accepted (uint8), energy_change = dH (double); each [B], may be null
 * At alpha = 1 the proposal and acceptance_rate have the bits of mfm_hmc_step_keys at num_steps = 1 on the same keys (with an installed
 * inverse mass equal to d_inverse_mass: of its mass instances).  The calls only enqueue; shards (n_chain_total != n_chain_local) are served.
 * Checks, in this order, a rejected call touching nothing: state pointers (and keys / key_mode / n_steps / thin as mfm_hmc_run);
 * MFM_EUNSUPPORTED for the Cox process (mfm_hmc_step's message); MFM_EINVAL naming the argument for step_size not positive, alpha
 * outside (0, 1], delta negative or NaN.
 * mfm_ghmc_init: with kb = split(key, n_chain_total)[chain_offset + b], p_j = normal64(split(kb, 2)[0], j, dim) / sqrt(minv_j) and
 * s = 2 uniform(split(kb, 2)[1]) - 1. */
int mfm_ghmc_init(mfm_ctx* ctx, uint32_t key0, uint32_t key1, const double* d_inverse_mass, double* d_momentum, double* d_slice);
/* one transition; chain b uses split(key, n_chain_total)[chain_offset + b] (or d_keys[b]) */
int mfm_ghmc_step(mfm_ctx* ctx, uint32_t key0, uint32_t key1, double beta, double step_size, double alpha, double delta,
                  const double* d_inverse_mass, float* d_pos, double* d_logp, float* d_grad, double* d_momentum, double* d_slice,
                  float* d_acceptance_rate, uint8_t* d_is_accepted, double* d_energy_change);
int mfm_ghmc_step_keys(mfm_ctx* ctx, const uint32_t* d_keys, double beta, double step_size, double alpha, double delta,
                       const double* d_inverse_mass, float* d_pos, double* d_logp, float* d_grad, double* d_momentum, double* d_slice,
                       float* d_acceptance_rate, uint8_t* d_is_accepted, double* d_energy_change);
/* n_steps transitions in ONE launch, x, g, logp, p and s resident in registers, bit-identical with n_steps single-step calls; key_mode,
 * the step keys, thin and the trajectory layout are mfm_hmc_run's.  Optional outputs (NULL to skip): d_n_accepted int32[B]; d_acc_sum
 * double[B], the sum of the acceptance rates; d_energy_sum double[B], the sum of dH over the ACCEPTED steps in step order; the three
 * infos of the LAST step. */
int mfm_ghmc_run(mfm_ctx* ctx, int key_mode, uint32_t key0, uint32_t key1, const uint32_t* d_keys,
                 double beta, double step_size, double alpha, double delta, const double* d_inverse_mass, int32_t n_steps, int32_t thin,
                 float* d_pos, double* d_logp, float* d_grad, double* d_momentum, double* d_slice,
                 int32_t* d_n_accepted, double* d_acc_sum, double* d_energy_sum,
                 float* d_acceptance_rate, uint8_t* d_is_accepted, double* d_energy_change,
                 float* d_traj_pos, double* d_traj_logp);
/* MEADS WARMUP OF GHMC (Hoffman & Sountsov 2022; blackjax's meads_adaptation): n_iter GHMC transitions of ALL chains in which the step
 * size, the diagonal inverse mass, alpha and delta are set from cross-chain statistics; tests/meads_ref.py restates it in float64 and is
 * the definition.  The call only enqueues (six launches per iteration, ghmc.hip); the parameters live in device memory.
 * n_valid chains form n_folds = K folds of m = n_valid / K (K >= 2, m >= 2, K m = n_valid <= n_chain_local); rows from n_valid on are
 * stepped with fold 0's parameters and never read.  Chain perm[f m + i] is member i of fold f; perm starts as the identity and, with
 * shuffle_every = S > 0, is replaced before iterations S + 1, 2 S + 1, ... by row r - 1 (r = 1, 2, ...) of d_perms, DEVICE
 * int32[(n_iter - 1) / S][n_valid], permutations the HOST has drawn and uploaded before the call (bblackjax's meads_adaptation draws them
 * with permutation_indices from a key); entries outside [0, n_valid) are clamped.  S = 0: never.
 * Iteration t = 1 .. n_iter, for each fold f from the state BEFORE the step, in float64:
 *   1. column mean mu_f and population standard deviation sd_f (ddof 0) of the fold's positions
 *   2. Y = (x - mu_f) / sd_f and Z = grad sd_f, [m, dim] (Z not centred; both rounded to float32 for the Gram products), and
 *      lam(X) = [ (sum_ij S_ij^2 - sum_i S_ii^2) / (m (m - 1)) ] / [ sum_i S_ii / m ], S = X X^T
 *   3. eps_f = min(1, 0.5 / sqrt(lam(Z))), gamma_f = max(1 / sqrt(lam(Y)), 1 / (t eps_f)), alpha_f = 1 - exp(-2 eps_f gamma_f),
 *      delta_f = alpha_f / 2, minv_f = sd_f^2
 *   4. these become the parameters of fold (f + 1) mod K for this iteration's transition; if any of them is non-finite or eps_f <= 0
 *      the receiving fold keeps its previous ones (before iteration 1: step0, unit mass, alpha0, alpha0 / 2)
 * then one GHMC transition (mfm_ghmc_step) of every chain with its fold's parameters on the key mfm_hmc_run (n_steps = n_iter, same
 * key_mode) uses for step t - 1: the bits of mfm_ghmc_step_keys with those parameters.  After the last iteration the same statistics
 * are formed once over ALL n_valid chains with t = n_iter + 1: h_result (host, 3 doubles, or NULL) takes {eps, alpha, delta} and
 * d_inverse_mass_out (double[dim], or NULL) sd^2.  With h_result the call ends by waiting for the stream; with NULL it makes no host
 * synchronisation.  d_trace: double[n_iter][K][6] or NULL, per fold the eps, alpha, delta it USED, lam(Z) and lam(Y) it PRODUCED, its
 * mean acceptance rate; d_mass_trace: double[n_iter][K][dim] or NULL, the minv it used.
 * Checks, in this order: state pointers; key_mode / d_keys / n_iter as mfm_hmc_run; MFM_EUNSUPPORTED for the Cox process; MFM_EINVAL for
 * step0 not positive, alpha0 outside (0, 1]; MFM_EUNSUPPORTED for a shard (n_chain_total != n_chain_local: the fold statistics would
 * need an all-reduce); MFM_EINVAL for n_folds < 2, n_valid not a multiple of n_folds or giving m < 2 or above n_chain_local,
 * shuffle_every < 0, d_perms missing when a shuffle falls inside n_iter. */
int mfm_meads_warmup(mfm_ctx* ctx, int key_mode, uint32_t key0, uint32_t key1, const uint32_t* d_keys,
                     double beta, double step0, double alpha0, int32_t n_iter, int32_t n_valid, int32_t n_folds,
                     int32_t shuffle_every, const int32_t* d_perms,
                     float* d_pos, double* d_logp, float* d_grad, double* d_momentum, double* d_slice,
                     double* h_result, double* d_inverse_mass_out, double* d_trace, double* d_mass_trace);
/* host only: h_out = {m, m_pad, d_pad, Gram workgroups per iteration} of a warmup (the fold size, its rows padded to the 64-row tile,
 * dim padded to the 32-column chunk, 2 K T (T + 1) / 2 with T = m_pad / 64); MFM_EINVAL for what the warmup refuses */
int mfm_meads_plan(int32_t n_valid, int32_t n_folds, int32_t dim, int32_t* h_out);
/* ChEES-HMC WARMUP (Hoffman, Radul & Sountsov 2021; blackjax's chees_adaptation): n_iter HMC steps of ALL chains in which the step size
 * and the trajectory length are adapted ACROSS the chains; tests/chees_ref.py restates it in float64 and is the definition.  The call
 * only enqueues (four launches per iteration, chees.hip); eps_t, T_t, L_t and the optimizer's state live in device memory.
 * Iteration t = 1 .. n_iter, with eps_1 = step0 and T_1 = traj0:
 *   1. h_t = the base-2 radical inverse of t (1/2, 1/4, 3/4, 1/8, ...), tau_t = h_t T_t, L_t = min(max_leapfrog, max(1, ceil(tau_t / eps_t)));
 *   2. one HMC step of every chain with (eps_t, L_t) on the key mfm_hmc_run (n_steps = n_iter, same key_mode) uses for step t - 1: the
 *      bits of mfm_hmc_step_keys.  Kept per chain: the state before the step x, the end point x' (float32, accepted or not), the end
 *      velocity v' = minv p', alpha = min(1, exp(H_0 - H_end)), and div = !(H_end - H_0 < divergence_threshold) (NaN: divergent);
 *   3. over the first n_valid chains (rows from n_valid on are stepped but not read), in float64: the column means xbar, xbar' over
 *      all of them; over the non-divergent ones, g_k = tau_t (|x'_k - xbar'|^2 - |x_k - xbar|^2) <x'_k - xbar', v'_k>,
 *      ghat_t = sum alpha_k g_k / sum (alpha_k + 1e-20), hm_t = n / sum (1 / alpha_k) (IEEE: an alpha of 0 gives 0); all divergent: both 0;
 *   4. the step size by mfm_hmc_warmup's dual averaging, steps 2. - 5. above with p_m := hm_t, giving eps_{t+1} = exp(x_t);
 *   5. one Adam step (b1 0.9, b2 0.999, epsilon 1e-8, bias-corrected) ASCENDING log T along ghat_t; a non-finite ghat_t leaves log T and
 *      the moments as they were; then log T is clamped to [x_t, x_t + log(max_leapfrog)], T_{t+1} = exp(log T), and
 *      ma_t = decay ma_{t-1} + (1 - decay) log T_{t+1} with ma_0 = log(traj0).
 * h_result (host, or NULL) takes {exp(xbar_n), exp(ma_n), eps_{n+1}, T_{n+1}}: the step size and the trajectory length to sample with,
 * and the last iterates.  With it the call ends by waiting for the stream; with NULL it returns without any host synchronisation.
 * d_trace (or NULL): double[n_iter][7] = eps_t, T_t, L_t, hm_t, ghat_t, the number of divergent chains, the mean alpha over the valid
 * chains.  d_prop float[B][dim], d_vel double[B][dim], d_alpha double[B] (each or NULL: context scratch) are left holding the LAST
 * iteration's x', v', alpha.  State is updated in place; the context's inverse mass (mfm_hmc_set_inverse_mass) is used as given.
 * Checks: mfm_hmc_run's shared ones in its order (state and step0, key_mode / d_keys / n_iter, the Cox process: MFM_EUNSUPPORTED with
 * mfm_hmc_step's message), then n_chain_total != n_chain_local: MFM_EUNSUPPORTED (the means would need an all-reduce); n_valid outside
 * [2, n_chain_local], traj0 or learning_rate not positive, decay outside [0, 1), max_leapfrog outside [1, 100000], target_accept
 * outside (0, 1), divergence_threshold not positive: MFM_EINVAL.  A rejected call touches nothing. */
int mfm_chees_warmup(mfm_ctx* ctx, int key_mode, uint32_t key0, uint32_t key1, const uint32_t* d_keys,
                     double beta, double step0, double traj0,
                     int32_t n_iter, int32_t n_valid, double target_accept, double learning_rate,
                     int32_t max_leapfrog, double decay, double divergence_threshold,
                     float* d_pos, double* d_logp, float* d_grad,
                     double* h_result /* [4] */, double* d_trace, float* d_prop, double* d_vel, double* d_alpha);
/* PARALLEL TEMPERING (replica exchange; pt.hip, tests/pt_ref.py restates it in float64).  n_temps = K temperatures, n_ladders = R
 * independent ladders: chain b = r * K + k is slot k of ladder r and runs at h_betas[k] with step size h_step_sizes[k]; slot 0 is the one
 * that is kept (usually h_betas[0] = 1).  K * R <= n_chain_local; rows from K * R on are never read or written.  Both vectors are HOST
 * arrays of K doubles, which the library uploads itself.
 * One round t = 0 .. n_rounds - 1 of mfm_pt_run:
 *   1. n_local local steps of every chain at its own (beta_k, eps_k): HMC steps of num_steps leapfrog steps (kernel 1) or MALA steps
 *      under mfm_mala_run's textbook flag (kernel 0);
 *   2. with exchange = 1 one sweep of deterministic even-odd parity (Syed et al. 2019): the pairs (k, k + 1) with k % 2 == t % 2 in every
 *      ladder; slots without a partner at that parity are untouched.  exchange = 0: no sweep, independent tempered chains.
 * The exchange of a pair of slots (i, j = i + 1) of one ladder: c_i = the log-density and gradient of x_j at beta_i, c_j = those of x_i
 * at beta_j, each with the bits mfm_mala_init gives for that position and beta; delta = (c_i + c_j) - (lp_i + lp_j) in float64, every
 * operation rounded on its own; p = min(1, exp(delta)), a NaN delta rejects; accepted iff u < p.  On accept the two position rows swap,
 * each slot takes the candidate log-density and gradient evaluated at its own beta (the state mfm_mala_init would give), and the two
 * entries of d_replica swap.  This is Metropolis on the joint: correct for any tempering path.
 * KEY SCHEDULE, from the one key: (k_move, k_swap) = split(key, 2).  Round t's local steps are mfm_hmc_run / mfm_mala_run in key_mode 0
 * on split(k_move, n_rounds)[t] with n_steps = n_local (chain b has the bits of that call at the scalars beta_k, eps_k).  Round t's sweep
 * runs on split(k_swap, n_rounds)[t]: the pair whose LOWER slot is chain i draws u = uniform of split(that, n_chain_total)[chain_offset + i].
 * mfm_pt_exchange is one sweep of the given parity on the given key (pair keys as above).
 * Outputs of mfm_pt_run (each may be NULL; the tallies are zeroed first, the call only enqueues): d_n_accepted int32[K * R] and d_acc_sum
 * double[K * R], the local steps' accepted count and sum of acceptance probabilities per slot over all rounds; d_replica int32[K * R], IN
 * and out, which start replica sits in which slot; d_swap_accepted int32[R][K - 1] and d_swap_prob double[R][K - 1], per pair (by its
 * lower slot) the accepted swaps and the sum of p (mfm_pt_exchange ADDS to both); with thin >= 1 (n_rounds % thin == 0, at least one of
 * the two pointers) slot 0 of every ladder after the sweep of every round with (t + 1) % thin == 0: d_traj_pos float[n_rounds / thin][R][dim],
 * d_traj_logp double[n_rounds / thin][R], contiguous as mfm_autocorr / mfm_chain_sums read them.
 * Checks, in order: the state pointers; kernel in {0, 1}; num_steps as mfm_hmc_run (HMC); the Cox process and an installed inverse mass:
 * MFM_EUNSUPPORTED; n_chain_total != n_chain_local: MFM_EUNSUPPORTED (one rank only); n_temps in [2, 64]; n_ladders >= 1;
 * K * R <= n_chain_local; every beta and step size finite and positive; parity in {0, 1} (mfm_pt_exchange); n_local >= 1; n_rounds >= 1;
 * exchange in {0, 1}; thin as mfm_hmc_run with n_rounds in n_steps' place.  A rejected call touches nothing. */
int mfm_pt_exchange(mfm_ctx* ctx, uint32_t key0, uint32_t key1, const double* h_betas /* HOST double[n_temps] */,
                    int32_t n_temps, int32_t n_ladders, int32_t parity,
                    float* d_pos, double* d_logp, float* d_grad,
                    int32_t* d_replica, int32_t* d_swap_accepted, double* d_swap_prob);
int mfm_pt_run(mfm_ctx* ctx, int kernel /* 0 MALA, 1 HMC */, uint32_t key0, uint32_t key1,
               const double* h_betas, const double* h_step_sizes /* HOST double[n_temps] */,
               int32_t n_temps, int32_t n_ladders, int32_t num_steps /* leapfrog, HMC */, int textbook /* MALA */,
               int32_t n_local, int32_t n_rounds, int exchange /* 0 none, 1 even-odd */, int32_t thin,
               float* d_pos, double* d_logp, float* d_grad,
               int32_t* d_n_accepted, double* d_acc_sum, int32_t* d_replica,
               int32_t* d_swap_accepted, double* d_swap_prob,
               float* d_traj_pos, double* d_traj_logp);
/* ELLIPTICAL SLICE SAMPLING for the Cox process (Murray, Adams & MacKay 2010; eslice.hip, tests/eslice_ref.py restates it in float64):
 * BUILD-SIDE MODE like the HMC entry points.  It is the reference's bblackjax/mcmc/tess.py under the linear transport T(u) = mu + L u,
 * L the Cholesky factor of the prior covariance: the log-det is constant and |u|^2 + |m|^2 is constant on the ellipse, so the slice test
 * of tess.py:42-44 compares log-likelihoods alone.  No step size, no gradient, every transition moves.  The state of chain b is its
 * position d_pos float[B][dim] and its UNTEMPERED log-likelihood d_loglik double[B], ll(x) = sum_i (x_i c_i - a exp(x_i)).
 * One transition at inverse temperature beta (finite, >= 0; beta = 0 accepts the first proposal: an exact prior-preserving rotation):
 *   1. k_b: the chain's key exactly as mfm_mala_step / mfm_mala_step_keys derive it; (k_nu, k_u, k_theta, k_shrink) = split(k_b, 4);
 *   2. nu = L n with n = normal(k_nu, (dim,));                       3. log y = beta * ll(x) + log(uniform(k_u));
 *   4. theta = 2 pi * uniform(k_theta) (float64), lo = theta - 2 pi, hi = theta;
 *   5. evaluation subiter = 1, 2, ...: x' = mu + (x - mu) cos(theta) + nu sin(theta), accepted when beta * ll(x') is finite and > log y;
 *      otherwise theta < 0 ? lo = theta : hi = theta, theta = lo + (hi - lo) * uniform(k_shrink, (MFM_ESLICE_MAX_SUBITER,))[subiter - 1];
 *   6. after MFM_ESLICE_MAX_SUBITER evaluations the chain keeps x and ll(x) (inside the slice by construction) and counts as capped:
 *      a non-finite position ends at the cap, it does not spin.
 * mfm_set_lgcp_chol installs L (HOST double[dim * dim], row-major, lower triangular) on a context whose target is the Cox process; a call
 * of its own like mfm_hmc_set_inverse_mass.  MFM_EUNSUPPORTED for another target (MFM_ENOTARGET without one); MFM_EINVAL for a
 * non-finite entry or a non-zero entry above the diagonal; a rejected call keeps what was installed.  mfm_set_target removes the factor.
 * mfm_eslice_init: d_loglik = ll of every row of d_pos.
 * mfm_eslice_step / _step_keys: one transition, state in place.  Info of the transition (each may be NULL): d_subiter int32[B], the
 * evaluations made; d_theta double[B], the last angle evaluated (the accepted one unless capped); d_momentum float[B][dim], nu.
 * mfm_eslice_run: n_steps transitions in ONE launch, the tile's rows resident in registers (a tile of 16 chains never depends on
 * another), bit-identical with n_steps single-step calls: key_mode 0 / 1, their key schedules, thin and the trajectory layout are
 * mfm_mala_run's (d_traj_pos float[n_steps / thin][B][dim], d_traj_loglik double[n_steps / thin][B]), so mfm_autocorr and
 * mfm_chain_sums read the trajectory.  d_subiter_sum int32[B]: the evaluations of all transitions; d_n_capped int32[B]: the capped
 * transitions; d_subiter_max int32[B]: the most evaluations any one transition made; d_subiter / d_theta / d_momentum take the LAST transition's info, as mfm_mala_run's info arrays do (each may be NULL).
 * Checks, in mfm_mala_run's order: the state pointers; key_mode / d_keys / n_steps; thin; then a target other than the Cox process:
 * MFM_EUNSUPPORTED (no Gaussian prior factor); no installed factor: MFM_ENOTARGET; beta not finite or negative: MFM_EINVAL;
 * n_chain_local not a multiple of 16: MFM_EINVAL; dim beyond the instances (dim > 1664; the largest serves the 40 x 40 grid of the reference's default, dim 1600): MFM_ETOOLARGE.  A rejected call
 * touches nothing; the calls only enqueue.  A sharded context (n_chain_total, chain_offset) is served: the chains are independent.
 * mfm_eslice_launch_plan (host only, no context): *h_tpw, the column tiles per wave of the kernel instance that serves dim (1, 2, 4, 8
 * or 13), and *h_lds_bytes, the dynamic LDS of one workgroup. */
#define MFM_ESLICE_MAX_SUBITER 64
int mfm_set_lgcp_chol(mfm_ctx* ctx, const double* h_chol /* HOST [dim * dim], row-major, lower */);
int mfm_eslice_init(mfm_ctx* ctx, const float* d_pos, double* d_loglik);
int mfm_eslice_step(mfm_ctx* ctx, uint32_t key0, uint32_t key1, double beta, float* d_pos, double* d_loglik,
                    int32_t* d_subiter, double* d_theta, float* d_momentum);
int mfm_eslice_step_keys(mfm_ctx* ctx, const uint32_t* d_keys, double beta, float* d_pos, double* d_loglik,
                         int32_t* d_subiter, double* d_theta, float* d_momentum);
int mfm_eslice_run(mfm_ctx* ctx, int key_mode, uint32_t key0, uint32_t key1, const uint32_t* d_keys,
                   double beta, int32_t n_steps, int32_t thin,
                   float* d_pos, double* d_loglik, int32_t* d_subiter_sum, int32_t* d_n_capped,
                   float* d_traj_pos, double* d_traj_loglik,
                   int32_t* d_subiter, double* d_theta, float* d_momentum /* the LAST transition's info, as mfm_eslice_step's */,
                   int32_t* d_subiter_max);
int mfm_eslice_launch_plan(int32_t dim, int32_t* h_tpw, int32_t* h_lds_bytes);
/* HAMILTONIAN MONTE CARLO FOR THE COX PROCESS on the 16-chain K^-1 GEMM tile (lgcp_hmc.hip), the target that mfm_hmc_* refuses.  The
 * four calls mirror mfm_hmc_step / _step_keys / _run / _warmup argument for argument: the same keys and key schedules, the same in-place
 * state -- the MALA state, made by mfm_mala_init on this context -- the same outputs, and the same dual-averaging recursion in the warmup.
 * One step of chain b with chain key kb: k_mom = split(kb, 2)[0], k_acc = split(kb, 2)[1]; momentum p_j = normal(k_mom, (dim,))[j] in
 * float64; H0 = -logp + sum(p^2) / 2; num_steps velocity-Verlet steps, each p += eps/2 g; x = (float)(x + eps p); y = K^-1 (x - mu)
 * by ONE tile GEMM; g = beta (c - a exp(x)) - y; p += eps/2 g; the log-density of the end point from the last step's float64 row sums;
 * accepted when uniform(k_acc) < min(1, exp(H0 - H_end)) (NaN rejects).  oracle/hmc.py on targets.Tempered(dist, beta) restates it.
 * One workgroup per 16 chains; x, p and g of a tile stay in registers over the trajectory, and mfm_cox_hmc_run / _warmup make all
 * their steps in ONE launch (an accepted row stores its end point, every step reads its start from the state arrays): bit-identical with
 * n_steps single-step calls on the run's keys; step m of a warmup has the bits of mfm_cox_hmc_step_keys with the scalar step size
 * d_step_traj[m][b].  Rows of a tile adapt different step sizes at the same num_steps.
 * Checks: those of the mfm_hmc_* call of the same name, in its order; then a target other than the Cox process: MFM_EUNSUPPORTED (use
 * mfm_hmc_*); an installed inverse mass: MFM_EUNSUPPORTED (the kernel runs at unit mass); n_chain_local not a multiple of 16:
 * MFM_EINVAL; dim beyond the instances (dim > 1024, a 32 x 32 grid): MFM_ETOOLARGE.  A rejected call touches nothing; the calls only
 * enqueue.  A sharded context (n_chain_total, chain_offset) is served: the chains are independent.
 * mfm_cox_hmc_launch_plan (host only, no context): *h_tpw, the column tiles per wave of the kernel instance that serves dim (1, 2, 4 or
 * 8), and *h_lds_bytes, the dynamic LDS of one workgroup. */
int mfm_cox_hmc_step(mfm_ctx* ctx, uint32_t key0, uint32_t key1, double beta, double step_size, int32_t num_steps,
                     float* d_pos, double* d_logp, float* d_grad, float* d_acceptance_rate, uint8_t* d_is_accepted);
int mfm_cox_hmc_step_keys(mfm_ctx* ctx, const uint32_t* d_keys, double beta, double step_size, int32_t num_steps,
                          float* d_pos, double* d_logp, float* d_grad, float* d_acceptance_rate, uint8_t* d_is_accepted);
int mfm_cox_hmc_run(mfm_ctx* ctx, int key_mode, uint32_t key0, uint32_t key1, const uint32_t* d_keys,
                    double beta, double step_size, int32_t num_steps /* leapfrog steps per HMC step */,
                    int32_t n_steps, int32_t thin,
                    float* d_pos, double* d_logp, float* d_grad,
                    int32_t* d_n_accepted, double* d_acc_sum,
                    float* d_acceptance_rate, uint8_t* d_is_accepted,
                    float* d_traj_pos, double* d_traj_logp);
int mfm_cox_hmc_warmup(mfm_ctx* ctx, int key_mode, uint32_t key0, uint32_t key1, const uint32_t* d_keys,
                       double beta, double step0, int32_t num_steps /* leapfrog steps per HMC step */,
                       int32_t n_steps, double target_accept,
                       float* d_pos, double* d_logp, float* d_grad,
                       double* d_step_avg, double* d_step_last,
                       int32_t* d_n_accepted, double* d_acc_sum,
                       double* d_step_traj);
int mfm_cox_hmc_launch_plan(int32_t dim, int32_t* h_tpw, int32_t* h_lds_bytes);
/* STEP-SIZE WARMUP OF THE NO-U-TURN SAMPLER: n_steps NUTS transitions in ONE launch, as mfm_nuts_run (chain resident in registers,
 * key_mode 0 / 1 and their key schedules, max_tree_depth / divergence_threshold and the installed inverse mass as there), in which every
 * chain adapts its OWN step size by the dual averaging of mfm_hmc_warmup -- the same recursion, constants and clamp, eps_1 = step0
 * itself -- on p_m = its tree's acceptance statistic: the mean over every leaf integrated of min(1, exp(H0 - H)), the float64 value
 * mfm_nuts_step reports as d_acceptance_rate.  Outputs per chain: d_step_avg (required), d_step_last, d_step_traj double[n_steps][B] as
 * mfm_hmc_warmup's; d_acc_sum double, the sum of the p_m in step order (a transition has no accept / reject: there is no d_n_accepted);
 * d_leapfrog_sum int64, d_n_divergent int32, d_depth_sum int32 as mfm_nuts_run's (each may be NULL).  Transition m of chain b has the
 * bits of mfm_nuts_step_keys with the scalar step size d_step_traj[m][b] and the same step key.  Chains at different step sizes build
 * trees of different depths, and the launch ends with its slowest chain.  No trajectory and no last-step info are kept.
 * Errors: mfm_hmc_warmup's (n_steps, step_size, target_accept, key_mode, d_keys, d_step_avg), then mfm_nuts_step's (max_tree_depth,
 * divergence_threshold, MFM_EUNSUPPORTED for the Cox process and for dim > 256, the LDS limit).  A rejected call touches nothing. */
int mfm_nuts_warmup(mfm_ctx* ctx, int key_mode, uint32_t key0, uint32_t key1, const uint32_t* d_keys,
                    double beta, double step0, int32_t max_tree_depth, double divergence_threshold,
                    int32_t n_steps, double target_accept,
                    float* d_pos, double* d_logp, float* d_grad,
                    double* d_step_avg, double* d_step_last, double* d_acc_sum, double* d_step_traj,
                    int64_t* d_leapfrog_sum, int32_t* d_n_divergent, int32_t* d_depth_sum);
/* ONE WINDOW of a mass-matrix adaptation under NUTS: mfm_nuts_warmup, which also adds the state after every transition, the float32
 * position as a double, in step order to d_pos_sum double[B][dim] and its (exact) square to d_pos_sumsq double[B][dim]; both are required
 * and are overwritten.  As mfm_hmc_warmup_window it always runs the mass instances, with the context's vector, or with ones when none is
 * installed: everything else it writes then has mfm_nuts_warmup's bits. */
int mfm_nuts_warmup_window(mfm_ctx* ctx, int key_mode, uint32_t key0, uint32_t key1, const uint32_t* d_keys,
                           double beta, double step0, int32_t max_tree_depth, double divergence_threshold,
                           int32_t n_steps, double target_accept,
                           float* d_pos, double* d_logp, float* d_grad,
                           double* d_step_avg, double* d_step_last, double* d_acc_sum, double* d_step_traj,
                           int64_t* d_leapfrog_sum, int32_t* d_n_divergent, int32_t* d_depth_sum,
                           double* d_pos_sum, double* d_pos_sumsq);
/* vmap(dist.loglik) (exe_flow_matching.py:418) */
int mfm_loglik(mfm_ctx* ctx, const float* d_pos, double* d_out);

/* ---- K3/K4/K9: flow-matching loss and gradient (exe_flow_matching.py:151-178,362-365) ------------------------------ */
/* loss and parameter gradient on the local chains; d_grads [num_params] (canonical layout) and d_loss [1] are caller
 * owned so a multi-GPU host can all-reduce them (SUM) before mfm_adamw_step. */
int mfm_fm_loss_grad(mfm_ctx* ctx, uint32_t key0, uint32_t key1, const float* d_pos, double* d_loss, float* d_grads);
/* loss only on n samples (eval_step, :370-374); any n > 0 (a last partial 16-row tile is staged inside the library), draws
 * indexed out of n_total starting at offset */
int mfm_fm_loss(mfm_ctx* ctx, uint32_t key0, uint32_t key1, const float* d_samples, int n, int n_total, int offset,
                double* d_loss);

/* ---- K7: optimizer step (exe_flow_matching.py:129-137,184,366) ------------------------------------------------
 * apply_if_finite: on a single-rank context the finite check of the gradient that mfm_fm_loss_grad just wrote to d_grads
 * rides in its reduction, and mfm_adamw_step(d_grads) with the SAME pointer reuses that verdict.  A caller that changes the
 * buffer's contents in between (its own all-reduce, accumulation, clipping) must pass the result through a DIFFERENT buffer
 * (or call on a multi-rank context): any other pointer is checked afresh by the optimizer's own check kernel. */
int mfm_adamw_step(mfm_ctx* ctx, const float* d_grads);

/* ---- context-owned RCCL communicator for the gradient all-reduce ------------------------------
 * The reference has no distributed code: its loss sums over ALL chains (exe_flow_matching.py:178) inside one process.  With
 * the chains sharded over ranks that sum becomes ONE all-reduce(SUM) of the flow-matching gradient per train_step (:362-368),
 * over RCCL / xGMI.  A host without a collective layer of its own hands the context a communicator:
 *   rank 0: mfm_comm_unique_id(id) and ships the 128 bytes to the other ranks out of band (a file, a socket, MPI, ...);
 *   every rank, with its GPU current: mfm_comm_init(ctx, nranks, rank, id)  -- collective (ncclCommInitRank);
 *   per iteration: mfm_fm_loss_grad(...); mfm_grad_allreduce_begin(ctx, d_grads)  -- asynchronous, on the context's own
 *     communication stream, ordered after the work queued on the context's stream; the caller may queue the next MALA step
 *     (which touches neither gradient nor parameters) before mfm_adamw_step(ctx, d_grads), which waits for the all-reduce.
 *   mfm_adamw_step on a context with a communicator and no all-reduce in flight reduces first, IN LINE on the context's stream
 *     (no event hop; what mfm_train_iter does at more than one rank: training kernel with the MALA step inside, weight-gradient kernel,
 *     ncclAllReduce, AdamW -- measured 5 us per iteration above the one-rank sequence on a one-rank communicator, against 25 - 30 us
 *     for the overlapped form, whose two cross-stream event hops cost more than the 9 us MALA step they hide).
 * With more than one rank the apply_if_finite decision is taken on the REDUCED gradient, so every rank decides alike.
 * RCCL is resolved at run time (dlopen of librccl.so.1, preferring a copy the process already loaded): the library has no
 * link-time dependency on it and a single-GPU host needs none.  mfm_destroy destroys the communicator.
 * (The Python host, mfm_amd/engine.py, uses this path whenever its process group is RCCL; MFM_TORCH_ALLREDUCE=1 keeps torch.distributed's.) */
#define MFM_COMM_ID_BYTES 128
int mfm_comm_unique_id(uint8_t out[MFM_COMM_ID_BYTES]);
int mfm_comm_init(mfm_ctx* ctx, int nranks, int rank, const uint8_t id[MFM_COMM_ID_BYTES]);
int mfm_comm_destroy(mfm_ctx* ctx);
/* ranks of the context's communicator as RCCL reports them (ncclCommCount); 0 when the context owns none */
int mfm_comm_count(mfm_ctx* ctx, int32_t* h_out);
int mfm_grad_allreduce_begin(mfm_ctx* ctx, float* d_grads);
/* host copies of {step, count, notfinite_count, last_applied} and the learning rate logged at :367 */
int mfm_opt_state(mfm_ctx* ctx, int32_t h_out[4], float* h_last_lr);

/* ---- K5/K6: CNF transforms and flow-MH step (exe_flow_matching.py:206-242,246-278) ------------------------------ */
/* v(x, t) and optionally the x-JVP (d_tangent, d_jvp may be NULL); n multiple of 16 */
int mfm_vf_apply(mfm_ctx* ctx, const float* d_x, const float* d_t, const float* d_tangent, int n,
                 float* d_v, float* d_jvp);
/* direction +1: transform_and_logdet (:206-221); -1: inverse_and_logdet (:223-242).  Hutchinson keys: per_chain_keys
 * != 0 -> d_keys is uint32[n][2] (one key per sample, flow-MH steps); else key0/key1 is ONE key shared by all samples
 * (final sampling, :455).  d_nsteps (may be NULL) receives the attempted Dopri5 steps per sample. */
int mfm_ode_transform(mfm_ctx* ctx, int direction, int per_chain_keys, const uint32_t* d_keys, uint32_t key0,
                      uint32_t key1, const float* d_in, int n, float* d_out, float* d_ldj, int32_t* d_nsteps);
/* one flow-based MH step for every local chain with keys split(key, n_chain_total) (:303,312); state in place */
int mfm_flow_step(mfm_ctx* ctx, int mode, uint32_t key0, uint32_t key1, double beta,
                  float* d_pos, double* d_logp, float* d_grad,
                  float* d_acceptance_rate, uint8_t* d_is_accepted, float* d_proposed_position, int32_t* d_nsteps);

/* ---- L1: one loop iteration in one call (exe_flow_matching.py:432-439) ------------------------------------------ */
/* train_data_generator(key_gen, states, count, params, beta) (:300-314) followed by train_step(key_train, positions,
 * state) (:362-368): the flow-MH step of `flow_mode` when count % (mcmc_per_flow_steps + 1) == 0, the MALA step otherwise
 * (mcmc_per_flow_steps >= 1; the fractional / negative schedules of :304-310 are composed by the host from the separate
 * entry points), then loss and gradient on the NEW positions and, with apply_update != 0, the optimizer step.  A
 * multi-GPU host passes apply_update = 0, all-reduces d_grads (SUM) and calls mfm_adamw_step itself.  d_acceptance_rate
 * and d_nsteps may be NULL; d_nsteps is written by flow iterations only.  Returns MFM_OK or the first failing step's status.
 * On a MALA iteration of a phi-four target (relu network on the tile family) the step runs INSIDE the training kernel's workgroups
 * -- the arithmetic and draws of mfm_mala_step, bit for bit, one launch less (MFM_NO_FUSED_MALA=1 in the environment keeps the
 * two launches).  With apply_update != 0 on one rank (tile family, no context-owned communicator) the weight gradients, their
 * reduction over the chain slices, the apply_if_finite decision and AdamW are ONE launch (wgrad_sk.hip), bit-identical with
 * mfm_fm_loss_grad + mfm_adamw_step including skipped (non-finite) updates; MFM_NO_FUSED_OPT=1 keeps the optimizer apart.  That
 * launch's workgroups wait for one another: one context per device at a time (two contexts of one process launching it concurrently
 * on different streams could starve each other of workgroup slots). */
int mfm_train_iter(mfm_ctx* ctx, int64_t count, int mcmc_per_flow_steps, int flow_mode,
                   uint32_t gen_key0, uint32_t gen_key1, uint32_t train_key0, uint32_t train_key1,
                   double beta, double step_size, float* d_pos, double* d_logp, float* d_grad,
                   float* d_acceptance_rate, int32_t* d_nsteps, double* d_loss, float* d_grads, int apply_update);

/* ---- K8: annealing (exe_flow_matching.py:391-417) ------------------------------------------------------------- */
/* Bisection for the next beta on n (global) log-likelihoods; h_beta_out gets the new beta (synchronises). */
int mfm_beta_update(mfm_ctx* ctx, double prev_beta, const double* d_logliks, int n, double alpha, double* h_beta_out);

/* ---- measurement (bench.py): HIP-event timing of the kernels, recorded on the context's stream ------------------- */
/* class ids: 0 mala_step, 1 fm_fwd_bwd, 2 wgrad, 3 adamw (4 small kernels), 4 flow_step, 5 fm eval, 6 reductions */
/* ---- rows of the flow's reference distribution: out[i] = normal(keys[i], (dim,))  (distributions.py:93-97 vmapped at
 *      exe_flow_matching.py:285, :389, :453).  d_keys: uint32 [n][2]. ---- */
int mfm_normal_rows(mfm_ctx* ctx, const uint32_t* d_keys, int n, float* d_out);

/* ---- selection step of conditional importance sampling (exe_flow_matching.py:280-296, chosen when
 *      num_importance_samples > 0): given, per chain b, the pull-back of the current position (u0, vol0 from
 *      mfm_ode_transform direction -1 with key split(keys[b],4)[1]) and n_is flow samples (refs = normal rows of
 *      split(split(keys[b],4)[0], n_is), xs / vols = mfm_ode_transform of them with keys split(split(keys[b],4)[2], n_is),
 *      lps = tempered target log-density of xs; sample (b, j) at row b * n_is + j), draw the categorical choice with
 *      split(keys[b],4)[3] and update position / logdensity in place (the gradient is left as is, :295). ---- */
int mfm_cis_select(mfm_ctx* ctx, uint32_t key0, uint32_t key1, int n_is, const float* d_u0, const float* d_vol0,
                   const float* d_refs, const float* d_xs, const float* d_vols, const double* d_lps, float* d_pos,
                   double* d_logp, float* d_acc_prob, uint8_t* d_is_accepted, float* d_proposed, float* d_weight);

/* ---- sample-quality metrics: mcmc_utils.py:28-85 (stein_disc) and :88-111 (max_mean_disc), called at
 *      exe_flow_matching.py:469-487.  d_grad = grad log p of the UNTEMPERED target at d_x (mfm_mala_init at beta = 1
 *      returns it).  beta is the reference's argument (default -1/2).  Synchronise; results on the host. ---- */
int mfm_stein_disc(mfm_ctx* ctx, const float* d_x, const float* d_grad, int n, double beta, double h_u_v[2]);
int mfm_max_mean_disc(mfm_ctx* ctx, const float* d_x, const float* d_y, int m, double* h_out);

/* ---- chain diagnostics (diag.hip): autocorrelation along the time axis of a trajectory and Geyer's initial-positive-sequence
 *      estimate; mcmc_utils.py:131-165 (autocorrelation) without its FFT.  d_x is float32 [n][n_series], time-major: series s
 *      is the strided column d_x[t * n_series + s], the layout of mfm_mala_run's d_traj_pos with n_series = n_chain * dim.
 *      Per series: mean in float64, c_t = x_t - mean, A_k = sum_{t < n-k} c_t c_{t+k}, rho_k = A_k / A_0 for k < n_lags (rho_0 is
 *      exactly 1; the reference's function returns rho_k / 2, the binding halves); Gamma_m = rho_2m + rho_2m+1,
 *      tau = -1 + 2 sum of Gamma_m over the leading run of Gamma_m > 0, using only the pairs with 2m + 1 < n_lags (n_lags is the
 *      max lag), ess = n / tau; var = A_0 / n with A_0 summed in float64.  Any output may be NULL (not all of them); without
 *      d_rho no [n_lags][n_series] buffer exists anywhere and a series costs only the lags up to its truncation point; d_tau /
 *      d_ess are bit-identical with and without d_rho.  Lag sums: float32 products summed in float32 inside
 *      MFM_AUTOCORR_TIME_BLOCK time steps, float64 across (MFM_AUTOCORR_F64=1 at mfm_create: float64 throughout), MFM_AUTOCORR_LAG_BLOCK
 *      lags per pass over the series.  Deterministic (no atomics); asynchronous on the context's stream; needs no target, Fourier
 *      block or parameters.
 *      Edge semantics: a series with A_0 = 0 (constant, or n = 1) yields NaN in rho, tau and ess (the reference divides 0 / 0
 *      with the warnings silenced), var 0; a non-finite input makes the outputs of ITS series NaN and of no other.
 *      EINVAL (message names the argument): n < 1, n_series < 1, n_lags outside [1, n], d_x NULL, every output NULL. ---- */
#define MFM_AUTOCORR_LAG_BLOCK 32
#define MFM_AUTOCORR_TIME_BLOCK 256
int mfm_autocorr(mfm_ctx* ctx, const float* d_x, int64_t n, int64_t n_series, int32_t n_lags,
                 float* d_rho      /* [n_lags][n_series] or NULL */,
                 float* d_tau, float* d_ess /* [n_series] or NULL; n_lags is then the max lag */,
                 double* d_mean, double* d_var /* [n_series] or NULL; var = A_0 / n */);

/* ---- cross-chain diagnostics (diag.hip): split-R-hat and the multi-chain ("bulk") effective sample size of Gelman et al. / Stan.
 *      d_x is float32 [n][n_chain_ld][dim], time-major, the layout of d_traj_pos; only chains 0 .. n_chain - 1 of every row are
 *      read (a shard's padding rows are skipped without a copy).
 *      Sub-chains.  split = 1: n_sub = n / 2 (integer division); sub-chain (m, 0) is rows [0, n_sub), sub-chain (m, 1) rows
 *      [n - n_sub, n) (for odd n the middle row belongs to neither); M = 2 n_chain.  split = 0: n_sub = n, M = n_chain.
 *      Per sub-chain c and coordinate j: mu_cj the float64 mean, A_k,cj = sum_{t < n_sub - k} c_t c_{t+k} of the signal centred by
 *      ITS OWN mean -- the lag sums of the autocorrelation entry above, same arithmetic (float32 products inside
 *      MFM_AUTOCORR_TIME_BLOCK steps, float64 across; MFM_AUTOCORR_F64=1: float64 throughout; float64 centring), A_0 in float64.
 *      chain_sums writes d_sums, float64 [n_lags + 2][dim]:
 *        sums[0][j] = sum_c mu_cj,   sums[1][j] = sum_c mu_cj^2,   sums[2 + k][j] = sum_c A_k,cj  (k = 0 .. n_lags - 1).
 *      Every row is additive over disjoint sets of chains: chains sharded over ranks are combined by ONE all-reduce (sum) of this
 *      array and of the sub-chain count.  No [n_lags][n_chain][dim] array exists anywhere; the scratch is context-owned, grown on
 *      demand and independent of n: slabs [n_slices][n_lags + 2][dim] of float64 partial sums with n_slices = min(n_chain,
 *      max(1, MFM_CHAIN_SLICES_MAX / ceil(dim / 64))) at most (at most 128 KiB (n_lags + 2) for dim <= 16384), and the mean and A_0
 *      of every sub-chain and coordinate (2 float64 each: [2][M][dim]).  No floating-point atomics, one writer per element, a summation
 *      order fixed by (n_chain, dim) alone: the same input gives the same bits on the same build, and the rows that a call with
 *      fewer lags also has are the same bits in both.
 *      chain_diag takes the (all-reduced) sums, n_sub and the TOTAL sub-chain count M = n_subchains, per coordinate in float64:
 *        W      = sums[2] / (M (n_sub - 1))                          within-chain variance
 *        B/n    = (sums[1] - sums[0]^2 / M) / (M - 1)                variance of the sub-chain means
 *        var+   = (n_sub - 1) / n_sub * W + B/n
 *        rhat   = sqrt(var+ / W)
 *        rho_k  = 1 - (W - sums[2 + k] / (M (n_sub - 1))) / var+     (rho_0 = 1 - 0 exactly)
 *        Gamma_m = rho_2m + rho_2m+1;  tau = -1 + 2 sum of Gamma_m over the leading run of Gamma_m > 0 among the pairs with
 *        2m + 1 < n_lags: Geyer's rule exactly as in the autocorrelation entry, with NO monotone smoothing of the Gammas and NO
 *        clamp of tau or ess (Stan applies both; an antithetic coordinate gives tau < 1 here);  ess = M n_sub / tau.
 *      Outputs float32 [dim]: d_rhat, d_ess, d_tau, and d_rho [n_lags][dim]; each may be NULL, not all; rhat / ess / tau are the same
 *      bits with and without d_rho.  Both calls are asynchronous on the context's stream and need no target, Fourier block or
 *      parameters.
 *      Edge semantics: a coordinate with W = 0 (constant in every sub-chain) gives NaN in all outputs of that coordinate only; a
 *      non-finite input makes its own coordinate NaN and no other.  The subtraction in B/n cancels when |mean| >> the spread of the
 *      sub-chain means: it is taken in float64, which leaves a relative error of about 1e-16 mean^2 / (B/n) in B/n.
 *      EINVAL (message names the argument): n_sub < 2, n_chain < 1 or > n_chain_ld, dim < 1, n_subchains < 2, n_lags outside
 *      [1, n_sub], split not 0 / 1, d_x / d_sums NULL, every output of chain_diag NULL. ---- */
#define MFM_CHAIN_SLICES_MAX 256
int mfm_chain_sums(mfm_ctx* ctx, const float* d_x, int64_t n, int32_t n_chain, int32_t n_chain_ld, int32_t dim, int32_t split,
                   int32_t n_lags, double* d_sums /* [n_lags + 2][dim] */);
int mfm_chain_diag(mfm_ctx* ctx, const double* d_sums, int64_t n_sub, int64_t n_subchains, int32_t dim, int32_t n_lags,
                   float* d_rhat, float* d_ess, float* d_tau /* [dim] */, float* d_rho /* [n_lags][dim] */);

/* ---- draws of the coming iterations, produced ahead of time (noise.hip) -------------------------------------------------
 * Slot j holds the Gaussian / uniform draws of the MALA step keyed h_keys_gn[j] and of the flow-matching batch keyed
 * h_keys_step[j] (uint32 [n_slots][2] each, the keys later passed to mfm_mala_step / mfm_fm_loss_grad).  The request arms
 * the NEXT mfm_flow_step: the workgroups of its kernel whose tile of chains has finished produce the draws until the slowest
 * tile is done (the launch lasts as long as its slowest chain), so the work rides in otherwise idle CU time;
 * mfm_mala_step / mfm_fm_loss_grad then recognise their key and read the stored draws (the values they would draw in line:
 * results are bit-identical).  Call it right BEFORE mfm_flow_step with the keys of the following K iterations.  Served by the
 * shape-specialised flow-step kernel (headline network shape, PhiFour, --hutch); otherwise EUNSUPPORTED and nothing changes.
 * mfm_noise_drop forgets armed / stored draws (the kernels draw in line again). */
int mfm_noise_prefetch(mfm_ctx* ctx, int n_slots, const uint32_t* h_keys_gn, const uint32_t* h_keys_step);
int mfm_noise_drop(mfm_ctx* ctx);

/* ---- adaptive tempered SMC baseline on the same MALA kernels (exe_others.py:79-111 -> bblackjax/smc) ----------------
 * mfm_smc_delta   : ess.ess_solver + solver.dichotomy (ess.py:46-89, solver.py:20-82) on n log-likelihoods, clipped to
 *                   [0, max_delta] (adaptive_tempered.py:61-72); synchronises, result on the host.
 * mfm_smc_weights : weights = softmax(delta * loglik) (float64, [n]) and log normalising constant (base.py:125-128).
 * mfm_smc_resample: resampling.systematic (resampling.py:50-52,124-135); d_scratch: n doubles (the cumulative sum).
 * mfm_gather_rows : particles[idx] (base.py:120); dst != src. */
int mfm_smc_delta(mfm_ctx* ctx, const double* d_loglik, int n, double target_ess, double max_delta, double* h_delta);
int mfm_smc_weights(mfm_ctx* ctx, const double* d_loglik, int n, double delta, double* d_weights, double* h_lognorm);
int mfm_smc_resample(mfm_ctx* ctx, uint32_t key0, uint32_t key1, const double* d_weights, int n, double* d_scratch,
                     int32_t* d_idx);
/* the other cumulative-sum schemes of resampling.py: stratified (:55-57) and multinomial (:60-80, sorted uniforms);
 * d_scratch: 2 n + 2 doubles.  (residual, :83-121, is composed on the host from the multinomial one: mfm_amd/bblackjax/smc/resampling.py) */
#define MFM_RESAMPLE_SYSTEMATIC 0
#define MFM_RESAMPLE_STRATIFIED 1
#define MFM_RESAMPLE_MULTINOMIAL 2
int mfm_smc_resample_scheme(mfm_ctx* ctx, int scheme, uint32_t key0, uint32_t key1, const double* d_weights, int n,
                            double* d_scratch, int32_t* d_idx);
int mfm_gather_rows(mfm_ctx* ctx, const float* d_src, const int32_t* d_idx, int n, int dim, float* d_dst);
/* ---- N1: self-normalised importance resampling of the final flow samples (exe_flow_matching.py:458-459):
 *      d_idx[j] = jax.random.choice(key, n, (m,), p = exp(d_logw - max d_logw))[j]; d_scratch: n doubles (the cumulative sum,
 *      taken in index order).  Combine with mfm_gather_rows. ---- */
int mfm_choice_logw(mfm_ctx* ctx, uint32_t key0, uint32_t key1, const double* d_logw, int n, int m, double* d_scratch,
                    int32_t* d_idx);
/* d_out[0..1] = sum and sum of squares (float64) of d_x[0..n): the per-iteration acceptance statistics
 * (exe_flow_matching.py:442-443: infos.acceptance_rate.mean() / .std()) without a host round trip */
int mfm_acc_stats(mfm_ctx* ctx, const float* d_x, int n, double* d_out);

/* ---- Stein variational gradient descent (bblackjax/vi/svgd.py, optimizers/cocob.py; svgd.hip) ------------------------------------
 * Particles x_i (i < n, row-major [n][d] float32), g_i = grad log pi_beta(x_i), length scale h (ONE float64 on the device):
 *   k_ij = exp(-(1/h) |x_i - x_j|^2)                                                        (svgd.py:94-96)
 *   fg_i = -(1/n) sum_j [ k_ij g_j + (2/h) k_ij (x_i - x_j) ]                               (:74-84, the functional gradient)
 *        = -(1/n) [ (K G)_i + (2/h) ( s_i x_i - (K X)_i ) ],   s_i = sum_j k_ij
 *   x <- x + optimizer(fg)                                                                  (:86-87)
 *   h <- median^2 / log(n), median over the n (n - 1) / 2 distances |x_i - x_j|, i > j, of the NEW particles; the mean of the two
 *        middle values when their count is even                                              (:99-124, :164-166)
 * Free shapes: any n in [2, 16384] (more: MFM_ETOOLARGE) and any d >= 1.  Deterministic (no float atomics), asynchronous on the
 * context's stream, no host synchronisation; a rejected call touches nothing and its message names the argument.
 *
 * mfm_svgd_sqdist: d_D [n][n] float32, D_ij = |x_i - x_j|^2 by q_i + q_j - 2 xc_i . xc_j on the exact-f32 matrix pipe, xc = x - column
 *   mean (the mean in float64); clamped at 0, diagonal exactly 0, symmetric to the bit;
 *   |D_ij - exact| <= (d + 8) 2^-23 (q_i + q_j), q the centred squared norms.
 * mfm_svgd_median: d_length_scale[0] = ((sqrt a + sqrt b) / 2)^2 / log n in float64, a <= b the two middle order statistics (equal for
 *   an odd count) of the strict lower triangle of the float32 d_D, selected exactly.  All particles equal: 0.
 * mfm_svgd_gradient: d_fg [n_rows][d] float32 = rows [i0, i0 + n_rows) of fg, from x, g [n][d], D [n][n] and *d_length_scale; the weights
 *   exp(-D / h) are float32 and s_i sums the same weights the products use.  A row range has the bits of those rows of the full call.
 * mfm_svgd_apply: x <- x + update(fg) on n x d elements in place, in float64 per element; `count` is the number of updates ALREADY
 *   applied.  h_hyper[4] and the state arrays d_s0 .. d_s4 ([n][d] float32, NULL beyond the kind's) by kind:
 *   MFM_SVGD_SGD     {learning_rate}: x -= lr fg.
 *   MFM_SVGD_ADAGRAD {learning_rate, initial_accumulator_value, eps}, s0 = acc (created at the initial value):
 *                    acc += fg^2; x -= lr fg / sqrt(acc + eps) where acc > 0 (optax 0.1.9's form).
 *   MFM_SVGD_ADAM    {learning_rate, b1, b2, eps}, s0 = m, s1 = v: m = b1 m + (1 - b1) fg; v = b2 v + (1 - b2) fg^2; t = count + 1;
 *                    x -= lr (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps).
 *   MFM_SVGD_COCOB   {alpha, eps}, s0 .. s4 = init_particles, cumulative_gradients C, scale L (created at eps), subgradients G, reward R
 *                    (cocob.py:52-86): L = max(L, |fg|); G += |fg|; R = max(R - fg (x - x0), 0); C -= fg;
 *                    x += -x + (x0 + C / (L max(G + L, alpha L)) (L + R)).
 *   sgd / adagrad / adam restate optax's published formulas; their parity with optax itself is not pinned by a test.
 * mfm_svgd_step: n_iter whole iterations on the context's target at temperature beta, on the n_chain_valid particles of d_x
 *   [n_chain_local][dim] (padding rows are never read into a sum nor written): target gradient (the launch of mfm_mala_init), sqdist
 *   (kept from the previous iteration's last step: same bits), gradient, apply with count + iteration, then sqdist of the new
 *   particles and, unless update_median == 0, median into d_length_scale[0] (in: the scale of the first iteration).  d_ls_used (may
 *   be NULL): float64 [n_iter], the scale each iteration used.  n_chain_total != n_chain_local: MFM_EUNSUPPORTED.  The bits of n_iter
 *   calls with n_iter = 1. */
enum { MFM_SVGD_SGD = 0, MFM_SVGD_ADAGRAD = 1, MFM_SVGD_ADAM = 2, MFM_SVGD_COCOB = 3 };
int mfm_svgd_sqdist(mfm_ctx* ctx, const float* d_x, int32_t n, int32_t d, float* d_D);
int mfm_svgd_median(mfm_ctx* ctx, const float* d_D, int32_t n, double* d_length_scale);
int mfm_svgd_gradient(mfm_ctx* ctx, const float* d_x, const float* d_g, const float* d_D, const double* d_length_scale, int32_t n, int32_t d,
                      int32_t i0, int32_t n_rows, float* d_fg);
int mfm_svgd_apply(mfm_ctx* ctx, int kind, const double* h_hyper, int64_t count, int32_t n, int32_t d, float* d_x, const float* d_fg,
                   float* d_s0, float* d_s1, float* d_s2, float* d_s3, float* d_s4);
int mfm_svgd_step(mfm_ctx* ctx, double beta, int kind, const double* h_hyper, int64_t count, int32_t n_iter, int update_median, float* d_x,
                  float* d_s0, float* d_s1, float* d_s2, float* d_s3, float* d_s4, double* d_length_scale, double* d_ls_used);

/* ---- algorithmic counters (the figures roofline numbers are computed from) ----------------------
 * h_out[0] MALA chain-steps, [1] flow-matching training samples, [2] flow-matching evaluation samples (mfm_fm_loss),
 * [3] Dopri5 solves (a flow step is two per chain), [4] attempted Dopri5 steps over all solves (summed on the device),
 * [5] vector-field evaluations = 2 * [3] + 6 * [4] (odeint: f(y0), the initial-step probe, six stages per attempt),
 * [6] optimizer steps, [7] algorithmic HBM bytes of the MALA steps (4 (5 dim + 5) per chain-step).  Synchronises. */
int mfm_get_counters(mfm_ctx* ctx, int64_t h_out[8]);
int mfm_reset_counters(mfm_ctx* ctx);

/* ---- parity instrumentation: Dormand-Prince on a PRESCRIBED step sequence -------------------------------------------------
 * Arms the NEXT mfm_ode_transform (one solve per sample) or mfm_flow_step (two: 0 inverse, 1 forward) on this context: the
 * solver takes d_dt[j] as the step size of attempt j (j = 0: the initial step) and d_acc[j] as its accept decision instead
 * of its controller's, and records what the controller computed: d_ratio[j] = error ratio of attempt j, d_dt_own[0] = its
 * initial step, d_dt_own[j + 1] = the step it proposed after attempt j.  Element (solve s, sample r, attempt j) of each
 * array is at ((s * n + r) * cap + j), n = samples of the armed call; a zero d_dt entry ends the solve.  Lets two
 * implementations be compared stage for stage on the same step sequence (tests/test_gpu_replay.py); no counterpart in the
 * reference.  d_diag (may be NULL; flow step only): float64 [n][4] = {inverse log-det, forward log-det, tempered log-density
 * at the proposal, log acceptance ratio}, the terms of exe_flow_matching.py:271-274.  d_dt == NULL disarms.  Both kernel
 * families (the wide family's host-driven solver takes the same hooks in its row kernels). */
int mfm_debug_replay(mfm_ctx* ctx, int cap, const float* d_dt, const uint8_t* d_acc, float* d_ratio, float* d_dt_own,
                     double* d_diag);

/* class_mask: 0 = off; otherwise bit c enables class c (-1: all) and the record is reset.  Two event records per launch
 * cost ~6 us of stream time each side on this runtime, so a caller that is itself being timed enables only the class it
 * needs (bench.py: the flow step during the timed region, every class in a separate instrumented pass). */
int mfm_profile(mfm_ctx* ctx, int class_mask);
int mfm_profile_read(mfm_ctx* ctx, double ms_total[8], int64_t launches[8]);   /* synchronises */

/* ---- test helpers (host only, no GPU needed) ------------------------------------------------------------------- */
int mfm_pack_index(int k, int n, int KB);       /* float index of W[k][n] inside a packed layer */
int mfm_pack_index_T(int k, int n, int NB);
/* Which kernel instance an mfm_fm_loss call of n samples runs on this context (its n & ~15 full 16-row tiles; the rest always go
 * through one 16-row tile).  Nothing is launched.  0: the 16-row tile every other call uses (or the wide family's row kernels);
 * otherwise the samples per workgroup of the forward-only kernel (32 or 64: & MFM_EVAL_ROWS_MASK) plus MFM_EVAL_RELU (the ReLU is
 * a compile-time constant; else the activation is read at run time), MFM_EVAL_CHAIN (the weight stream is chained from layer to
 * layer) and MFM_EVAL_BCRT (the phi-four boundary is read at run time).  < 0: MFM_E*. */
enum { MFM_EVAL_ROWS_MASK = 0xff, MFM_EVAL_RELU = 0x100, MFM_EVAL_CHAIN = 0x200, MFM_EVAL_BCRT = 0x400 };
int mfm_fm_eval_instance(mfm_ctx* ctx, int n);
int mfm_threefry2x32(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t out[2]);
/* The stream-K weight-gradient plan (wgrad_sk.hip) for n_jobs 64 x 64 blocks, nbb 16-chain tiles and at most `cap` resident workgroups;
 * needs no context and no GPU.  U = n_jobs * nbb units over G workgroups: the first r take q + 1 consecutive units, the others q.
 * g_override = 0: the default G; otherwise the G that MFM_WSK_G would request (ignored, as there, outside [n_jobs, min(U, cap)]).
 * h_out = {G, q, r, n_slices}, n_slices the sum over the blocks of their contributor counts; h_wg (may be NULL) is int32 [G][4] =
 * {j0, bb0, cnt, n0}: workgroup w holds cnt units from tile bb0 of block j0, the first n0 of them in block j0, the rest in j0 + 1. */
int mfm_wsk_plan(int n_jobs, int nbb, int cap, int g_override, int32_t h_out[4], int32_t* h_wg);
/* Which weight-gradient kernel mfm_fm_loss_grad / mfm_train_iter launch on this context; nothing is launched.
 * h_out = {kind, n_jobs, nbb, G, q, r}.  kind 0: the slab kernels (G = n_jobs * split workgroups, slices of q or q + 1 tiles, r = nbb %
 * split); 1: stream-K (G, q, r as mfm_wsk_plan); 2: the wide family (G workgroups, q of them the workgroup-per-job tail, r = 0). */
int mfm_wgrad_info(mfm_ctx* ctx, int32_t h_out[6]);
/* Which GEMM instance the wide family (wide.hip: launch_gemm, which launches from the same function) runs for `rows` rows (a multiple of
 * 16), KB 16-wide K blocks and NT 16-feature column tiles; dual != 0: a tangent GEMM over the first KBT K blocks rides along.  Needs
 * no context and no GPU: `switches` is the OR of the MFM_WGEMM_SW_* bits of the development switches a context latches at mfm_create
 * (MFM_WIDE_NOLDS, MFM_WIDE_NO_SMALL_TILES, MFM_WIDE_WM1, MFM_WIDE_RING8).  h_out = {instance (MFM_WGEMM_*), gridDim.x, gridDim.y,
 * blockDim.x}.  The names say the kernel and the 16 x 16 tiles per wave (rows x features) of its 2 x 2 waves: 11 / 12 / 22 and BIG (4 x 2)
 * are the register-only gemm_kernel (RING8: its ring of eight K blocks), LDS the LDS-staged kernel of eight waves (WM1: of four). */
enum { MFM_WGEMM_11 = 0, MFM_WGEMM_11_DUAL = 1, MFM_WGEMM_12 = 2, MFM_WGEMM_12_DUAL = 3, MFM_WGEMM_22 = 4, MFM_WGEMM_22_DUAL = 5,
       MFM_WGEMM_22_RING8 = 6, MFM_WGEMM_22_RING8_DUAL = 7, MFM_WGEMM_BIG = 8, MFM_WGEMM_LDS = 9, MFM_WGEMM_LDS_DUAL = 10,
       MFM_WGEMM_LDS_WM1 = 11, MFM_WGEMM_LDS_WM1_DUAL = 12, MFM_WGEMM_COUNT = 13 };
enum { MFM_WGEMM_SW_NOLDS = 1, MFM_WGEMM_SW_NO_SMALL_TILES = 2, MFM_WGEMM_SW_WM1 = 4, MFM_WGEMM_SW_RING8 = 8 };
int mfm_wide_gemm_plan(int rows, int KB, int NT, int dual, int KBT, unsigned switches, int32_t h_out[4]);
/* Launches of each instance by this context since it was created or last reset: h_out[MFM_WGEMM_COUNT], counted on the host where
 * launch_gemm launches (no device work, no synchronisation).  reset != 0 zeroes the tally after the read; h_out may be NULL then. */
int mfm_wide_gemm_tally(mfm_ctx* ctx, int64_t* h_out, int reset);

#ifdef __cplusplus
}
#endif
#endif /* MFM_H */
