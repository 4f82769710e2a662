// C ABI of libmfm_hip (include/mfm.h).  Unity build: the kernel translation units are included here so one hipcc
// invocation produces the shared library.
#include "../../include/mfm.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>
#include <dlfcn.h>
#include <mutex>
#include <rccl/rccl.h>     // types and enums only: the library is resolved at run time (rccl_api), never linked

#include "mala.hip"
#include "mala_run.hip"
#include "lgcp.hip"
#include "hmc.hip"
#include "hmc_run.hip"
#include "mclmc.hip"
#include "ghmc.hip"
#include "nuts.hip"
#include "warmup.hip"
#include "nuts_warmup.hip.h"
#include "chees.hip"
#include "pt.hip"
#include "eslice.hip"
#include "lgcp_hmc.hip"
#include "fm.hip"
#include "optim.hip"
#include "wgrad_sk.hip"
#include "noise.hip"
#include "ode.hip"
#include "anneal.hip"
#include "metrics.hip"
#include "diag.hip"
#include "cis.hip"
#include "wide.hip"
#include "smc.hip"
#include "svgd.hip"

static thread_local char g_err[512] = "";
static int fail(int code, const char* fmt, ...) {
  va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
  return code;
}
#define HIPCHK(x)                                                                                        \
  do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(MFM_EHIP, "%s: %s", #x, hipGetErrorString(e_)); } while (0)
#define LAUNCHCHK()                                                                                      \
  do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return fail(MFM_EHIP, "kernel launch: %s", hipGetErrorString(e_)); } while (0)

// ---- optional per-kernel timing with HIP events on the context's stream (bench.py roofline) -----------------------
enum { PROF_MALA = 0, PROF_FM = 1, PROF_WGRAD = 2, PROF_ADAM = 3, PROF_FLOW = 4, PROF_EVAL = 5, PROF_REDUCE = 6, PROF_NCLS = 8 };
struct Prof {
  bool on = false;
  unsigned mask = ~0u;            // classes that are bracketed by events
  std::vector<hipEvent_t> ev;     // pairs
  std::vector<int> cls;
  size_t used = 0;
};

// draws of the coming MALA + training iterations, produced in the tail of the flow-step kernel (noise.hip)
struct NoiseWs {
  int cap = 0;                                  // slots allocated
  draw_t *mala_n = nullptr, *fm_x0 = nullptr, *fm_eps = nullptr; double* mala_u = nullptr;
  float* fm_t = nullptr; uint32_t* d_keys = nullptr;      // [2][cap][2]
  int* counter = nullptr;
  std::vector<uint32_t> h_keys;                 // staging copy of the keys
  std::vector<Key2> gn, st;                     // keys of the slots
  int n_armed = 0;                              // slots the NEXT flow step will fill
  int n_valid = 0, cur_gn = 0, cur_st = 0;      // slots filled by the last flow step, consumption cursors
  bool no_mala0 = false;                        // slot 0 was keyed by the flow step that filled it: its MALA draws were not produced
};

// slots of mfm_get_counters
enum { CTR_MALA = 0, CTR_FM_TRAIN = 1, CTR_FM_EVAL = 2, CTR_SOLVES = 3, CTR_ATTEMPTS = 4, CTR_FIELD_EVALS = 5, CTR_OPT_STEPS = 6, CTR_MALA_BYTES = 7 };

struct mfm_ctx {
  Prof* prof;
  NoiseWs* noise;
  mfm_config cfg;
  hipStream_t stream;
  NetDev net;
  WsLayout ws;
  bool has_target, has_fourier;
  float *master, *mu, *nu, *Wp, *WpT, *bias, *fourier;
  float *acts, *dzs, *slabs, *dacts;
  double* loss_part; int loss_cap;
  float* wsk_partials = nullptr; int* wsk_tickets = nullptr;      // stream-K weight gradients (wgrad_sk.hip): partial blocks, arrival counters [2][n_jobs]
  WskConst* wsk_const = nullptr; WskWg* wsk_wg = nullptr;           // its tables, in device memory
  int wsk_G = 0, wsk_par = 0;                                       // its grid (0: the slab kernels serve this context), parity of the arrival counters
  int wsk_q = 0, wsk_r = 0;                                         // its units per workgroup (wsk_plan)
  int sus_par = 0;                                                  // parity of the training kernel's "suspicious values" word (flag[5 + parity])
  float* eval_pad = nullptr;   // [16][dim]: the last, partial 16-row tile of a mfm_fm_loss call whose n is not a multiple of 16
  WgradJob* jobs; int n_jobs, split;
  std::vector<WgradJob> h_jobs;          // host copy (wgrad_sk.hip takes the table in its launch arguments)
  OptState* opt; int* flag;      // opt: the CURRENT optimizer scalars (opt_alt: the buffer the one-launch reduction + optimizer writes next)
  OptState* opt_alt;
  const float* checked_grads = nullptr;   // gradient whose finite check already sits in flag[0] (single-rank mfm_fm_loss_grad)
  float *gmm_mode, *gmm_std, *gmm_logw, *counts, *Kinv, *kbias, *kdiag;
  OdeWs ode;
  Replay replay;               // armed by mfm_debug_replay for the NEXT mfm_ode_transform / mfm_flow_step (dt == nullptr: off)
  int64_t ctr[8];              // mfm_get_counters: host-side tallies (slot 4, the attempted Dopri5 steps, is summed on the device)
  unsigned long long* d_att;   // device tally of attempted steps
  int* att_buf; size_t att_cap;   // per-sample attempt counts of the last solve when the caller passed no d_nsteps
  double* beta_out;
  wide::Ctx* wide;             // non-null: the wide kernel family serves the network kernels (wide.hip)
  wide::Ctx* wide_ex = nullptr;   // fused family, exact trace, d >= 16: the SOLVES run on the wide family's solver (see create_impl)
  // context-owned RCCL communicator for the gradient all-reduce (mfm_comm_init; null: the caller reduces the gradient itself)
  ncclComm_t comm = nullptr; int comm_nranks = 0;
  hipStream_t comm_stream = nullptr; hipEvent_t ev_grads = nullptr, ev_comm = nullptr;
  const float* comm_pending = nullptr;   // gradient buffer whose all-reduce is in flight on comm_stream
  Switches sw;                           // the A/B switches as read at mfm_create: installed by every entry point (use_ctx)
  FmMala fuse_mala = {};                 // on != 0 during a mfm_train_iter whose MALA step rides in the training kernel
  int opt_resident_wgs = 0;              // workgroups of reduce_adamw_kernel this device holds at once (occupancy query at create)
  void* ac_ws = nullptr; size_t ac_ws_cap = 0;     // mfm_autocorr: the series means when the caller passes no d_mean
  void* cs_ws = nullptr; size_t cs_ws_cap = 0;     // mfm_chain_sums: mean and A_0 of every sub-chain, then the slabs [n_slices][n_lags + 2][dim] of float64 partial sums
  void* run_ws = nullptr; size_t run_ws_cap = 0;  // mfm_mala_run on the Cox process: the step keys and the per-step info its tallies read
  void* meads_ws = nullptr; size_t meads_ws_cap = 0;      // mfm_meads_warmup: the folds' parameters and statistics, the staged Y / Z tiles, the Gram partials (ghmc.hip: MeadsBufs)
  void* chees_ws = nullptr; size_t chees_ws_cap = 0;      // mfm_chees_warmup: the CheesState, the column means, g, and the per-chain records the caller did not pass (chees.hip: CheesBufs)
  double* pt_ws = nullptr;                                // mfm_pt_run / mfm_pt_exchange: the ladder, betas then step sizes (pt.hip: PtVec)
  void* svgd_ws = nullptr; size_t svgd_ws_cap = 0;        // mfm_svgd_*: column means, centred coordinates, row norms, selection state (svgd.hip: Scratch)
  void* svgd_step_ws = nullptr; size_t svgd_step_ws_cap = 0;   // mfm_svgd_step: D [n][n], the functional gradient, the target's log-density and gradient
  mutable int64_t wgemm_tally[MFM_WGEMM_COUNT] = {};   // mfm_wide_gemm_tally: launches per instance of wide::launch_gemm (host side)
  // mfm_hmc_set_inverse_mass: the diagonal of the HMC kernels' inverse mass matrix.  d_inv_mass [dim] holds the installed vector, or
  // ones when none is set (mfm_hmc_warmup_window runs the mass instances either way); h_inv_mass is the host copy, empty when none is set
  double* d_inv_mass = nullptr;
  std::vector<double> h_inv_mass;
  float* lgcp_chol = nullptr;      // mfm_set_lgcp_chol: L^T of the Cox process prior, packed as Kinv is (null: none installed)
};

// The development switches (common.hip.h) are read once per mfm_create and belong to THAT context: every entry point installs its
// context's snapshot before it sizes or launches anything, so a second context created under another environment cannot change what an
// earlier one launches (its workspaces were sized from its own snapshot: e.g. the flow step's chains per workgroup, MFM_FLOW_LIVE).
static inline void use_ctx(const mfm_ctx* x) { if (x) { g_sw = x->sw; wide::g_gemm_tally = x->wgemm_tally; } }

struct ProfScope {
  mfm_ctx* x; bool active;
  ProfScope(mfm_ctx* x_, int cls);
  ~ProfScope();
};

extern "C" const char* mfm_last_error(void) { return g_err; }
extern "C" int mfm_version(void) { return 1; }
extern "C" int mfm_pack_index(int k, int n, int KB) { return pack_index(k, n, KB); }
extern "C" int mfm_pack_index_T(int k, int n, int NB) { return pack_index_T(k, n, NB); }
extern "C" int mfm_threefry2x32(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t out[2]) {
  threefry2x32(Key2{k0, k1}, c0, c1, out[0], out[1]);
  return 0;
}

ProfScope::ProfScope(mfm_ctx* x_, int cls) : x(x_), active(false) {
  Prof* p = x->prof;
  if (!p || !p->on || !(p->mask >> cls & 1u) || p->used + 2 > p->ev.size()) return;
  active = true;
  p->cls.push_back(cls);
  (void)hipEventRecord(p->ev[p->used], x->stream);
}
ProfScope::~ProfScope() {
  if (!active) return;
  Prof* p = x->prof;
  (void)hipEventRecord(p->ev[p->used + 1], x->stream);
  p->used += 2;
}

extern "C" int mfm_profile(mfm_ctx* x, int enable) { use_ctx(x);
  if (!x) return fail(MFM_EINVAL, "null ctx");
  if (!x->prof) x->prof = new Prof();
  Prof* p = x->prof;
  if (enable && p->ev.empty()) {
    p->ev.resize(2 * 16384);
    for (auto& e : p->ev) HIPCHK(hipEventCreate(&e));
  }
  p->on = enable != 0;
  p->mask = (unsigned)enable;
  if (enable) { p->used = 0; p->cls.clear(); }
  return MFM_OK;
}

extern "C" int mfm_profile_read(mfm_ctx* x, double ms[8], int64_t counts[8]) { use_ctx(x);
  if (!x || !ms || !counts) return fail(MFM_EINVAL, "null argument");
  for (int i = 0; i < 8; ++i) { ms[i] = 0.0; counts[i] = 0; }
  if (!x->prof) return MFM_OK;
  HIPCHK(hipStreamSynchronize(x->stream));
  Prof* p = x->prof;
  for (size_t i = 0; i < p->cls.size(); ++i) {
    float t = 0.f;
    HIPCHK(hipEventElapsedTime(&t, p->ev[2 * i], p->ev[2 * i + 1]));
    ms[p->cls[i]] += t; counts[p->cls[i]] += 1;
  }
  return MFM_OK;
}

// hidden widths of one branch as a list: depth 0 = the two-element array of the configuration (include/mfm.h)
static int branch_widths(int depth, const int32_t two[2], int32_t third, int out[MLP_MAX_DEPTH]) {
  const int n = depth == 0 ? 2 : depth;
  for (int i = 0; i < MLP_MAX_DEPTH; ++i) out[i] = 0;
  if (n < 1 || n > MLP_MAX_DEPTH) return -1;
  for (int i = 0; i < n && i < 2; ++i) out[i] = two[i];
  if (n > 2) out[2] = third;
  return n;
}

static void build_net(const mfm_config& c, NetDev& n) {
  memset(&n, 0, sizeof n);
  n.d = c.dim; n.dp = ceil16(c.dim); n.F = c.fourier_dim; n.F2p = ceil16(2 * c.fourier_dim);
  int ht[MLP_MAX_DEPTH], hx[MLP_MAX_DEPTH], hj[MLP_MAX_DEPTH];
  n.nT = branch_widths(c.depth_t, c.hidden_t, c.hidden_t3, ht);
  n.nX = branch_widths(c.depth_x, c.hidden_x, c.hidden_x3, hx);
  n.nJ = branch_widths(c.depth_xt, c.hidden_xt, c.hidden_xt3, hj);
  // buffer widths: padded to 16 (a hidden unit of the padding has zero weights and bias on both sides: act(0) = 0 for all five
  // activations, and its tangent / gradient meet zero weights -- exact)
  n.ht1 = ceil16(ht[0]); n.ht2 = ceil16(ht[n.nT - 1]); n.hx1 = ceil16(hx[0]); n.hx2 = ceil16(hx[n.nX - 1]); n.hj1 = ceil16(hj[0]); n.hj2 = ceil16(hj[n.nJ - 1]);
  // flax creation order (exe_flow_matching.py:74-86): time branch, x branch, gate, joint branch, output
  int K[MLP_MAXL], N[MLP_MAXL], nl = 0, prev = 2 * c.fourier_dim;
  for (int i = 0; i < n.nT; ++i) { K[nl] = prev; N[nl] = ht[i]; prev = ht[i]; ++nl; }
  prev = c.dim;
  for (int i = 0; i < n.nX; ++i) { K[nl] = prev; N[nl] = hx[i]; prev = hx[i]; ++nl; }
  K[nl] = ht[n.nT - 1]; N[nl] = c.dim; ++nl;
  prev = hx[n.nX - 1] + ht[n.nT - 1];
  const int joint0 = nl;
  for (int i = 0; i < n.nJ; ++i) { K[nl] = prev; N[nl] = hj[i]; prev = hj[i]; ++nl; }
  K[nl] = hj[n.nJ - 1]; N[nl] = c.dim; ++nl;
  int wo = 0, bo = 0, mo = 0;
  for (int l = 0; l < nl; ++l) {
    LayerDesc& L = n.L[l];
    L.K = K[l]; L.N = N[l]; L.Kp = l == joint0 ? n.hx2 + n.ht2 : ceil16(K[l]); L.Np = ceil16(N[l]);      // [sx | st]: both halves padded (mlp.hip.h: packed_row)
    L.w_off = wo; wo += L.Kp * L.Np;
    L.b_off = bo; bo += L.Np;
    L.m_w = mo; mo += K[l] * N[l];
    L.m_b = mo; mo += N[l];
  }
  for (int l = nl; l < MLP_MAXL; ++l) { n.L[l].m_w = n.L[l].m_b = mo; n.L[l].w_off = wo; n.L[l].b_off = bo; }      // never selected by a parameter index
  n.n_packed = wo; n.n_bias = bo; n.n_params = mo;
  n.grad_clip = c.grad_clip;
  n.act = c.activation;
}

static void build_ws(const NetDev& n, WsLayout& w) {
  int o = 0;
  auto take = [&](int feat) { int r = o; o += feat / 16; return r; };
  w.a_ffat = take(n.F2p); w.a_t1 = take(n.ht1); w.a_st = take(n.ht2); w.a_cond = take(n.dp);
  w.a_x1 = take(n.hx1); w.a_sx = take(n.hx2); w.a_j1 = take(n.hj1); w.a_j2 = take(n.hj2); w.a_tiles = o;
  o = 0;
  w.z_t1 = take(n.ht1); w.z_t2 = take(n.ht2); w.z_x1 = take(n.hx1); w.z_x2 = take(n.hx2);
  w.z_gate = take(n.dp); w.z_j1 = take(n.hj1); w.z_j2 = take(n.hj2); w.z_out = take(n.dp); w.z_tiles = o;
}

// Everything mfm_create allocates hangs off the context, so ONE exit path frees it: a failure below returns its status and
// mfm_create destroys the partially built context (mfm_destroy tolerates null members) -- an out-of-memory create can be
// retried in-process without leaking what was allocated before the failure.
static int create_impl(const mfm_config& c, mfm_ctx* x);

extern "C" int mfm_create(const mfm_config* cfg, mfm_ctx** out) {
  if (!cfg || !out) return fail(MFM_EINVAL, "null argument");
  *out = nullptr;
  mfm_ctx* x = new mfm_ctx();          // value-initialised: every pointer null, every counter zero
  const int rc = create_impl(*cfg, x);
  if (rc != MFM_OK) { (void)mfm_destroy(x); return rc; }
  *out = x;
  return MFM_OK;
}

static int create_impl(const mfm_config& c, mfm_ctx* x) {
  if (c.dim <= 0 || c.fourier_dim <= 0) return fail(MFM_EINVAL, "dim / fourier_dim must be positive");
  {
    int hs[3][MLP_MAX_DEPTH];
    const int nd[3] = {branch_widths(c.depth_t, c.hidden_t, c.hidden_t3, hs[0]), branch_widths(c.depth_x, c.hidden_x, c.hidden_x3, hs[1]),
                       branch_widths(c.depth_xt, c.hidden_xt, c.hidden_xt3, hs[2])};
    for (int b = 0; b < 3; ++b) {
      if (nd[b] < 0) return fail(MFM_EUNSUPPORTED, "a branch has 1 to %d hidden layers (depth_t / depth_x / depth_xt = %d / %d / %d)", MLP_MAX_DEPTH, c.depth_t, c.depth_x, c.depth_xt);
      for (int i = 0; i < nd[b]; ++i) {
        if (hs[b][i] <= 0) return fail(MFM_EINVAL, "hidden widths must be positive (got %d)", hs[b][i]);      // (not multiples of 16: zero-padded, mlp.hip.h)
      }
    }
  }
  if (c.n_chain_local <= 0 || c.n_chain_local % 16)
    return fail(MFM_EUNSUPPORTED, "n_chain_local must be a positive multiple of 16 (got %d)", c.n_chain_local);
  const int n_valid = c.n_chain_valid > 0 ? c.n_chain_valid : c.n_chain_local;
  if (n_valid > c.n_chain_local) return fail(MFM_EINVAL, "n_chain_valid=%d exceeds n_chain_local=%d", n_valid, c.n_chain_local);
  if (c.chain_offset < 0 || c.chain_offset + n_valid > c.n_chain_total)
    return fail(MFM_EINVAL, "chain shard [%d, %d) outside n_chain_total=%d", c.chain_offset,
                c.chain_offset + n_valid, c.n_chain_total);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(MFM_EHIP, "no HIP device available");
  switches_read(); x->sw = g_sw;                     // development / A-B switches: fixed from here until the next mfm_create (common.hip.h)
  {
    // reduce_adamw_kernel's grid-wide exchange (taken when a gradient partial is huge or non-finite) spins until every workgroup
    // of its grid has arrived: all of them must be RESIDENT at once.  Ask the runtime what this device (a full MI355X, a CPX
    // partition, a CU-masked queue ...) and this build of the kernel actually hold, instead of assuming 256 CUs x 8 blocks.
    int dev = 0, per_cu = 0, cus = 0;
    HIPCHK(hipGetDevice(&dev));
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reduce_adamw_kernel, 256, 0));
    x->opt_resident_wgs = per_cu * cus;
  }
  x->cfg = c;
  build_net(c, x->net);
  build_ws(x->net, x->ws);
  NetDev& n = x->net;
  if (c.activation < MFM_ACT_RELU || c.activation > MFM_ACT_SWISH) return fail(MFM_EINVAL, "unknown activation %d", c.activation);
  if (x->cfg.ref_std == 0.0) x->cfg.ref_std = 1.0;           // zero-initialised config: the default 'stdgauss'
  if (!(x->cfg.ref_std > 0.0)) return fail(MFM_EINVAL, "ref_std must be positive");
  bool use_wide = c.kernel_family == MFM_FAMILY_WIDE;
  const bool two_layer = n.nT == 2 && n.nX == 2 && n.nJ == 2;
  if (!two_layer) {             // the fused tile kernels are written layer by layer for two hidden layers per branch
    if (c.kernel_family == MFM_FAMILY_TILE)
      return fail(MFM_EUNSUPPORTED, "hidden lists of %d / %d / %d layers (t / x / xt) run on the wide kernel family only", n.nT, n.nX, n.nJ);
    use_wide = true;
  } else {
    const FmLds L = fm_lds_layout(n, true);
    size_t sm_ode; int tpw_ode;
    const bool fits = (size_t)L.total * 4 <= 160 * 1024 && (n.dp / 16 + MLP_WAVES_FM - 1) / MLP_WAVES_FM <= 2 && ode_check(n, sm_ode, tpw_ode) == 0;
    if (!fits && c.kernel_family == MFM_FAMILY_TILE)
      return fail(MFM_ETOOLARGE, "network does not fit the fused 16-chain tile kernel (LDS %zu B, dim %d)", (size_t)L.total * 4, c.dim);
    if (!fits) use_wide = true;
  }
  if (c.kernel_family < 0 || c.kernel_family > MFM_FAMILY_WIDE) return fail(MFM_EINVAL, "unknown kernel_family %d", c.kernel_family);
  if (c.ode_method < MFM_ODE_DOPRI5 || c.ode_method > MFM_ODE_EULER) return fail(MFM_EINVAL, "unknown ode_method %d", c.ode_method);
  if (c.ode_method != MFM_ODE_DOPRI5 && (c.ode_steps < 1 || (c.n_ts > 2 && c.ode_steps % (c.n_ts - 1)))) return fail(MFM_EINVAL, "ode_steps=%d: a positive number of steps (a multiple of n_ts - 1) is needed with a fixed-step ode_method", c.ode_steps);
  const int nbb = c.n_chain_local / 16;
  x->split = nbb < 8 ? nbb : 8;
  if (const char* e = getenv("MFM_WGRAD_SPLIT")) { const int v = atoi(e); if (v >= 1 && v <= nbb) x->split = v; }      // development: A/B
  // chain slices of the weight-gradient GEMM: 8 measured best at 4096 x 256 (wgrad + slab reduction 36.9 us against 41.4 at 16)
  x->loss_cap = (c.max_eval_samples > c.n_chain_local ? c.max_eval_samples : c.n_chain_local) / 16 + 1;
  // wgrad job table
  std::vector<WgradJob> jobs;
  for (int l = 0; l < 8; ++l)
    for (int nt = 0; nt < n.L[l].Np / 16; nt += 4)
      for (int kt = 0; kt < n.L[l].Kp / 16; kt += 4) jobs.push_back(WgradJob{l, kt, nt});
  x->n_jobs = (int)jobs.size(); x->h_jobs = jobs;
#define ALLOC(p, cnt) HIPCHK(hipMalloc((void**)&(p), (size_t)(cnt) * sizeof(*(p))))
  ALLOC(x->master, n.n_params); ALLOC(x->mu, n.n_params); ALLOC(x->nu, n.n_params);
  ALLOC(x->Wp, n.n_packed); ALLOC(x->WpT, n.n_packed); ALLOC(x->bias, n.n_bias); ALLOC(x->fourier, n.F);
  if (!use_wide) {       // packed activation / gradient workspaces of the fused family
    ALLOC(x->acts, (size_t)x->ws.a_tiles * nbb * 256); ALLOC(x->dzs, (size_t)x->ws.z_tiles * nbb * 256);
    if (c.activation >= MFM_ACT_GELU) ALLOC(x->dacts, (size_t)x->ws.a_tiles * nbb * 256);      // gelu / swish: f'(pre-activation), see FmArgs
    ALLOC(x->slabs, (size_t)x->split * n.n_params);
  }
  ALLOC(x->loss_part, x->loss_cap);
  ALLOC(x->eval_pad, (size_t)16 * c.dim);
  if (!use_wide && x->n_jobs <= WSK_MAXJOBS && !getenv("MFM_WGRAD_SLABS")) {      // (MFM_WGRAD_SLABS=1: the round-1..4 slab kernels, for A/B)
    // stream-K weight gradients + optimizer in one launch (wgrad_sk.hip).  Its workgroups WAIT for the other contributors of their
    // block, so every workgroup of the grid must be resident at once: the grid never exceeds what the runtime says this device (a
    // full MI355X, a partition ...) holds of this kernel; a device that cannot hold one workgroup per block keeps the slab kernels.
    int dev = 0, per_cu = 0, cus = 0;
    HIPCHK(hipGetDevice(&dev));
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, wgrad_sk_kernel, 256, 0));
    WskConst h; memset(&h, 0, sizeof h);
    int G = 0;
    const char* g_env = getenv("MFM_WSK_G");
    if (per_cu * cus >= x->n_jobs) wsk_plan(x->n_jobs, nbb, per_cu * cus, g_env ? atoi(g_env) : 0, G, h.upw_q, h.upw_r);
    if (G >= x->n_jobs && h.upw_q >= 1) {
      h.net = n; h.nbb = nbb; h.n_jobs = x->n_jobs; h.G = G;
      ALLOC(x->wsk_partials, (size_t)2 * G * WSK_PSZ); ALLOC(x->wsk_tickets, 2 * x->n_jobs); ALLOC(x->wsk_const, 1);
      HIPCHK(hipMemset(x->wsk_tickets, 0, (size_t)2 * x->n_jobs * sizeof(int)));
      h.acts = x->acts; h.dzs = x->dzs; h.partials = x->wsk_partials;
      h.master = x->master; h.mu = x->mu; h.nu = x->nu; h.Wp = x->Wp; h.WpT = x->WpT; h.bias = x->bias;
      h.lr0 = c.learning_rate; h.learning_iter = c.learning_iter; h.warmup = c.warmup_steps;
      h.b1 = c.adam_b1; h.b2 = c.adam_b2; h.eps = (float)c.adam_eps; h.wd = (float)c.weight_decay; h.clip = (float)c.update_clip; h.max_err = 10;
      for (int j = 0; j < x->n_jobs; ++j) {
        const WgradJob& J = jobs[j];
        WskJob& o = h.jobs[j];
        o.layer = J.layer; o.kt0 = J.kt0; o.nt0 = J.nt0;
        const int KT = n.L[J.layer].Kp / 16, NT = n.L[J.layer].Np / 16;
        for (int wv = 0; wv < 4; ++wv) {
          o.a_row[wv] = wgrad_a_tile(n, x->ws, J.layer, J.kt0 + wv < KT ? J.kt0 + wv : J.kt0);
          o.z_row[wv] = wgrad_z_tile(x->ws, J.layer, J.nt0 + wv < NT ? J.nt0 + wv : J.nt0);
        }
      }
      h.n_slices = wsk_n_slices(x->n_jobs, nbb, h.upw_q, h.upw_r);
      HIPCHK(hipMemcpy(x->wsk_const, &h, sizeof h, hipMemcpyHostToDevice));
      std::vector<WskWg> wg(G);
      wsk_ranges(x->n_jobs, nbb, G, h.upw_q, h.upw_r, h.jobs, wg.data());
      ALLOC(x->wsk_wg, G);
      HIPCHK(hipMemcpy(x->wsk_wg, wg.data(), sizeof(WskWg) * G, hipMemcpyHostToDevice));
      x->wsk_G = G; x->wsk_q = h.upw_q; x->wsk_r = h.upw_r;
    }
  }
  ALLOC(x->jobs, x->n_jobs); ALLOC(x->opt, 1); ALLOC(x->opt_alt, 1); ALLOC(x->flag, 8); ALLOC(x->beta_out, 4);
  ALLOC(x->d_att, 1); HIPCHK(hipMemset(x->d_att, 0, sizeof(unsigned long long)));
  HIPCHK(hipMemcpy(x->jobs, jobs.data(), jobs.size() * sizeof(WgradJob), hipMemcpyHostToDevice));
  HIPCHK(hipMemset(x->master, 0, n.n_params * 4)); HIPCHK(hipMemset(x->mu, 0, n.n_params * 4));
  HIPCHK(hipMemset(x->nu, 0, n.n_params * 4)); HIPCHK(hipMemset(x->Wp, 0, n.n_packed * 4));
  HIPCHK(hipMemset(x->WpT, 0, n.n_packed * 4)); HIPCHK(hipMemset(x->bias, 0, n.n_bias * 4));
  HIPCHK(hipMemset(x->opt, 0, sizeof(OptState))); HIPCHK(hipMemset(x->opt_alt, 0, sizeof(OptState))); HIPCHK(hipMemset(x->flag, 0, 32));
  n.Wp = x->Wp; n.WpT = x->WpT; n.bias = x->bias; n.fourier = x->fourier;
  int rc = ode_ws_alloc(n, c, x->ode);
  if (rc) return fail(rc, "ODE workspace allocation failed");
  if (use_wide) {
    rc = wide::create(n, c.n_chain_local, &x->wide);
    if (rc) return fail(rc, "workspace allocation of the wide kernel family failed");
    x->wide->exact = !c.hutch;           // exact-trace log-det (exe_flow_matching.py:216-217,236-237): wide.hip, exact_trace()
    x->wide->master = x->master;         // ... which reads two kernels in their canonical [in][out] layout
  } else if (!c.hutch && c.dim >= 16 && !g_sw.tile_exact) {
    // Exact trace (the reference's default: no --hutch) on the fused family: its generic tile pushes the d basis tangents of 16 chains
    // through the network one 16-row tile at a time -- 7.4 ms per attempted step at d = 64, whatever the chain count.  The wide family's
    // exact trace needs hx1 tangent rows per chain in a few large GEMMs over all chains (wide.hip: exact_trace): 1.2 ms per attempt at
    // 1024 chains, 0.4 ms at 64.  So the SOLVES (flow steps, transforms) of such a context go to a wide workspace kept beside the tile
    // kernels, which keep MALA, training and evaluation.  Both read the same packed weights.  MFM_TILE_EXACT=1 keeps the tile's own.
    rc = wide::create(n, c.n_chain_local, &x->wide_ex);
    if (rc) return fail(rc, "workspace allocation of the exact-trace solver failed");
    x->wide_ex->exact = true;
    x->wide_ex->master = x->master;
  }
  return MFM_OK;
}

extern "C" int mfm_destroy(mfm_ctx* x) { use_ctx(x);
  if (!x) return MFM_OK;
  hipDeviceSynchronize();
  void* ps[] = {x->master, x->mu, x->nu, x->Wp, x->WpT, x->bias, x->fourier, x->acts, x->dzs, x->dacts, x->slabs, x->loss_part, x->eval_pad, x->wsk_partials, x->wsk_tickets, x->wsk_const, x->wsk_wg,
                x->jobs, x->opt, x->opt_alt, x->flag, x->gmm_mode, x->gmm_std, x->gmm_logw, x->counts, x->Kinv, x->kbias, x->kdiag, x->beta_out,
                x->d_att, x->att_buf, x->run_ws, x->ac_ws, x->cs_ws, x->d_inv_mass, x->svgd_ws, x->svgd_step_ws, x->chees_ws, x->meads_ws, x->pt_ws, x->lgcp_chol};
  for (void* p : ps) if (p) hipFree(p);
  (void)mfm_comm_destroy(x);
  ode_ws_free(x->ode);
  wide::destroy(x->wide);
  wide::destroy(x->wide_ex);
  if (x->noise) {
    NoiseWs* w = x->noise;
    for (void* p : {(void*)w->mala_n, (void*)w->mala_u, (void*)w->fm_x0, (void*)w->fm_eps, (void*)w->fm_t, (void*)w->d_keys, (void*)w->counter}) if (p) (void)hipFree(p);
    delete w;
  }
  if (x->prof) { for (auto& e : x->prof->ev) (void)hipEventDestroy(e); delete x->prof; }
  if (wide::g_gemm_tally == x->wgemm_tally) wide::g_gemm_tally = nullptr;
  delete x;
  return MFM_OK;
}

extern "C" int mfm_set_stream(mfm_ctx* x, void* s) { use_ctx(x); if (!x) return fail(MFM_EINVAL, "null ctx"); x->stream = (hipStream_t)s; return MFM_OK; }
extern "C" int mfm_sync(mfm_ctx* x) { use_ctx(x); if (!x) return fail(MFM_EINVAL, "null ctx"); HIPCHK(hipStreamSynchronize(x->stream)); return MFM_OK; }
extern "C" int mfm_num_params(const mfm_ctx* x) { use_ctx(x); return x ? x->net.n_params : MFM_EINVAL; }

extern "C" int mfm_set_target(mfm_ctx* x, int kind, const double* p, size_t np) { use_ctx(x);
  if (!x || !p) return fail(MFM_EINVAL, "null argument");
  TargetDev& T = x->net.T;
  const int d = x->cfg.dim;
  if (x->lgcp_chol) { (void)hipFree(x->lgcp_chol); x->lgcp_chol = nullptr; }      // the factor belongs to the target it was installed on
  memset(&T, 0, sizeof T);
  T.kind = kind; T.dim = d;
  if (kind == MFM_PHI4) {
    if (np != 2 && np != 4 && np != 5) return fail(MFM_EINVAL, "phi4 target takes {a, beta}, {a, beta, bc_kind, bc_value} or {a, beta, bc_kind, bc_value, dim_phys}");
    int side = d;      // the grid side in the coefficient a * side: dim on the chain, L on the L x L lattice (dim_phys = 2, dim = L * L)
    if (np == 5) {
      if (p[4] != 1.0 && p[4] != 2.0) return fail(MFM_EINVAL, "phi4 dim_phys must be 1 or 2");
      if (p[4] == 2.0) {
        side = (int)std::lround(std::sqrt((double)d));
        if (side * side != d) return fail(MFM_EINVAL, "phi4 dim_phys = 2 needs a square dim (dim = L * L)");
        T.lat = side;
      }
    }
    T.coef = (float)(p[0] * side); T.tbeta = (float)p[1];
    if (np >= 4) {      // boundary (distributions.py:130-139): kind 0 = Dirichlet at bc_value, 1 = periodic (bc_value ignored)
      if (p[2] != 0.0 && p[2] != 1.0) return fail(MFM_EINVAL, "phi4 boundary kind must be 0 (dirichlet) or 1 (periodic)");
      T.bc = p[2] == 1.0 ? MFM_BC_PERIODIC : MFM_BC_DIRICHLET;
      if (T.bc == MFM_BC_DIRICHLET) {
        if (!std::isfinite(p[3])) return fail(MFM_EINVAL, "phi4 Dirichlet boundary value must be finite");
        T.bval = (float)p[3];
      }
    }
  } else if (kind == MFM_GMM) {
    const int K = (int)p[0];
    if (K <= 0 || K > MFM_GMM_MAX_MODES || np != (size_t)(1 + 2 * K * d + K)) return fail(MFM_EINVAL, "bad GMM parameter block");
    if (d > 8) return fail(MFM_EUNSUPPORTED, "GMM targets support dim <= 8 (the reference forces dim = 2)");
    std::vector<float> mode(K * d), sd(K * d), lw(K);
    for (int i = 0; i < K * d; ++i) { mode[i] = (float)p[1 + i]; sd[i] = (float)p[1 + K * d + i]; }
    for (int k = 0; k < K; ++k) {
      double s = std::log(p[1 + 2 * K * d + k]) - 0.5 * d * std::log(2.0 * M_PI);
      for (int j = 0; j < d; ++j) s -= std::log(p[1 + K * d + k * d + j]);
      lw[k] = (float)s;
    }
    for (float** q : {&x->gmm_mode, &x->gmm_std, &x->gmm_logw}) if (*q) { hipFree(*q); *q = nullptr; }
    ALLOC(x->gmm_mode, K * d); ALLOC(x->gmm_std, K * d); ALLOC(x->gmm_logw, K);
    HIPCHK(hipMemcpy(x->gmm_mode, mode.data(), K * d * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(x->gmm_std, sd.data(), K * d * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(x->gmm_logw, lw.data(), K * 4, hipMemcpyHostToDevice));
    T.n_modes = K; T.gmm_mode = x->gmm_mode; T.gmm_std = x->gmm_std; T.gmm_logw = x->gmm_logw;
  } else if (kind == MFM_LGCP) {
    // {mu, poisson_a, log_norm, counts[d], Kinv[d*d]} (distributions.py:249-274; Kinv = inverse of the Gram matrix :265)
    if (np != (size_t)(3 + d + (size_t)d * d)) return fail(MFM_EINVAL, "bad LGCP parameter block");
    const int dp = x->net.dp, KB = dp / 16;
    std::vector<float> cnt(dp, 0.f), kb(dp, 0.f), kp((size_t)dp * dp, 0.f);
    const double mu = p[0];
    const double* Kinv = p + 3 + d;
    for (int j = 0; j < d; ++j) cnt[j] = (float)p[3 + j];
    for (int k = 0; k < d; ++k)
      for (int j = 0; j < d; ++j) kp[pack_index(k, j, KB)] = (float)Kinv[(size_t)k * d + j];
    for (int j = 0; j < d; ++j) {
      double rs = 0.0;
      for (int k = 0; k < d; ++k) rs += Kinv[(size_t)k * d + j];
      kb[j] = (float)(-mu * rs);
    }
    for (float** q : {&x->counts, &x->Kinv, &x->kbias, &x->kdiag}) if (*q) { hipFree(*q); *q = nullptr; }
    ALLOC(x->counts, dp); ALLOC(x->kbias, dp); ALLOC(x->kdiag, dp); ALLOC(x->Kinv, (size_t)dp * dp);
    {
      std::vector<float> kd(dp, 0.f);
      for (int j = 0; j < d; ++j) kd[j] = (float)Kinv[(size_t)j * d + j];
      HIPCHK(hipMemcpy(x->kdiag, kd.data(), dp * 4, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemcpy(x->counts, cnt.data(), dp * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(x->kbias, kb.data(), dp * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(x->Kinv, kp.data(), (size_t)dp * dp * 4, hipMemcpyHostToDevice));
    T.counts = x->counts; T.KinvP = x->Kinv; T.kbias = x->kbias; T.kdiag = x->kdiag;
    T.mu = (float)mu; T.poisson_a = (float)p[1]; T.log_norm = (float)p[2];
    // the K^-1 tile buffers must fit next to the MLP tiles
    const FmLds Lf = fm_lds_layout(x->net, true);
    const OdeLds Lo = ode_lds_layout(x->net, ODE_NW);
    if (!x->wide && ((size_t)Lf.total * 4 > 160 * 1024 || (size_t)Lo.total * 4 > 160 * 1024)) {
      memset(&T, 0, sizeof T);
      return fail(MFM_ETOOLARGE, "LGCP target with dim %d does not fit the 16-chain LDS tile next to this network", d);
    }
  } else {
    return fail(MFM_EINVAL, "unknown target kind %d", kind);
  }
  x->has_target = true;
  return MFM_OK;
}

extern "C" int mfm_set_fourier(mfm_ctx* x, const float* h) { use_ctx(x);
  if (!x || !h) return fail(MFM_EINVAL, "null argument");
  HIPCHK(hipMemcpy(x->fourier, h, x->net.F * 4, hipMemcpyHostToDevice));
  x->has_fourier = true;
  return MFM_OK;
}
extern "C" int mfm_set_params(mfm_ctx* x, const float* h) { use_ctx(x);
  if (!x || !h) return fail(MFM_EINVAL, "null argument");
  HIPCHK(hipMemcpyAsync(x->master, h, (size_t)x->net.n_params * 4, hipMemcpyHostToDevice, x->stream));
  launch_pack(x->net, x->master, x->Wp, x->WpT, x->bias, x->stream);
  LAUNCHCHK();
  HIPCHK(hipStreamSynchronize(x->stream));
  return MFM_OK;
}
extern "C" int mfm_get_params(mfm_ctx* x, float* h) { use_ctx(x);
  if (!x || !h) return fail(MFM_EINVAL, "null argument");
  HIPCHK(hipStreamSynchronize(x->stream));
  HIPCHK(hipMemcpy(h, x->master, (size_t)x->net.n_params * 4, hipMemcpyDeviceToHost));
  return MFM_OK;
}
extern "C" int mfm_reset_optimizer(mfm_ctx* x) { use_ctx(x);
  if (!x) return fail(MFM_EINVAL, "null ctx");
  HIPCHK(hipMemsetAsync(x->mu, 0, (size_t)x->net.n_params * 4, x->stream));
  HIPCHK(hipMemsetAsync(x->nu, 0, (size_t)x->net.n_params * 4, x->stream));
  HIPCHK(hipMemsetAsync(x->opt, 0, sizeof(OptState), x->stream));
  return MFM_OK;
}

static int noise_take(mfm_ctx* x, Key2 key, bool step);
#define NEED_TARGET() do { if (!x) return fail(MFM_EINVAL, "null ctx"); if (!x->has_target) return fail(MFM_ENOTARGET, "mfm_set_target has not been called"); } while (0)

static MalaArgs mala_args(mfm_ctx* x, double beta) {
  MalaArgs a; memset(&a, 0, sizeof a);
  a.T = x->net.T; a.n_total = x->cfg.n_chain_total; a.chain_offset = x->cfg.chain_offset; a.B = x->cfg.n_chain_local;
  a.beta = beta;
  return a;
}
static LgcpArgs lgcp_args(mfm_ctx* x, int mode, double beta, double eps) {      // mode 0: init (eps unused, any positive value), 1: step
  LgcpArgs l; memset(&l, 0, sizeof l);
  l.T = x->net.T; l.dp = x->net.dp; l.mode = mode; l.n_total = x->cfg.n_chain_total; l.chain_offset = x->cfg.chain_offset; l.B = x->cfg.n_chain_local;
  l.beta = beta; l.eps = eps;
  return l;
}
static void count_mala_steps(mfm_ctx* x, int64_t n) { x->ctr[CTR_MALA] += n; x->ctr[CTR_MALA_BYTES] += n * 4 * (5 * x->cfg.dim + 5); }   // n single chain steps
static int too_large(mfm_ctx* x, const char* kernel) { return fail(MFM_ETOOLARGE, "dim %d too large for the %s kernel", x->cfg.dim, kernel); }

// The argument checks the sampler entry points share; each calls them in its own order (the first error of a call with several is part of the ABI)
#define CHECKED(call) do { if (const int rc_ = (call)) return rc_; } while (0)
static int check_state(const float* d_pos, const double* d_logp, const float* d_grad, double step) {
  if (!d_pos || !d_logp || !d_grad) return fail(MFM_EINVAL, "null device pointer");
  if (!(step > 0)) return fail(MFM_EINVAL, "step_size must be positive");
  return MFM_OK;
}
static int check_run_keys(int key_mode, const uint32_t* d_keys, int32_t n_steps) {
  if (key_mode != 0 && key_mode != 1) return fail(MFM_EINVAL, "key_mode must be 0 (step-major) or 1 (chain-major) (got %d)", key_mode);
  if (key_mode == 1 && !d_keys) return fail(MFM_EINVAL, "key_mode 1 needs d_keys (one key per chain)");
  if (n_steps < 1) return fail(MFM_EINVAL, "n_steps must be at least 1 (got %d)", n_steps);
  return MFM_OK;
}
static int check_thin(int32_t thin, int32_t n_steps, const float* d_traj_pos, const double* d_traj_logp) {
  if (thin < 0) return fail(MFM_EINVAL, "thin must not be negative (got %d)", thin);
  if (thin > 0 && n_steps % thin) return fail(MFM_EINVAL, "thin (%d) must divide n_steps (%d)", thin, n_steps);
  if (thin > 0 && !d_traj_pos && !d_traj_logp) return fail(MFM_EINVAL, "thin > 0 needs d_traj_pos or d_traj_logp");
  return MFM_OK;
}
// a run's or a warmup's MALA arguments: the chain's own keys in key_mode 1, state in place
static MalaArgs mala_run_args(mfm_ctx* x, int key_mode, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, double step, int textbook,
                              float* d_pos, double* d_logp, float* d_grad) {
  MalaArgs a = mala_args(x, beta);
  a.key = Key2{k0, k1}; a.keys = key_mode == 1 ? d_keys : nullptr; a.eps = step; a.textbook = textbook;
  a.pos = d_pos; a.logp = d_logp; a.grad = d_grad;
  return a;
}

// LGCP dimensions beyond the fused tile kernel (d > 1024) go through the wide family's propose / K^-1 GEMM / accept split
static int wide_mala_lgcp(mfm_ctx* x, const LgcpArgs& l) {
  if (!x->wide) return -3;
  wide::LgcpMala m; memset(&m, 0, sizeof m);
  m.T = l.T; m.mode = l.mode; m.key = l.key; m.keys = l.keys; m.n_total = l.n_total; m.chain_offset = l.chain_offset; m.rows = l.B; m.d = l.T.dim; m.dp = l.dp;
  m.beta = l.beta; m.eps = l.eps; m.textbook = l.textbook;
  m.pos = l.pos; m.logp = l.logp; m.grad = l.grad; m.acc_prob = l.acc_prob; m.accepted = l.accepted; m.proposed = l.proposed; m.prop_weight = l.prop_weight;
  return wide::mala_lgcp(x->wide, x->net, m, x->stream);
}

// The fused LGCP tile kernel runs one workgroup per 16 chains and streams K^-1 once per workgroup: right for few chains,
// but 1024 chains are only 64 workgroups on 256 CUs.  With the wide family present and >= 128 chains the K^-1 contraction
// goes through the wide GEMM (every CU busy) between a propose and an accept kernel; it also serves d > 1024.
static int lgcp_mala_dispatch(mfm_ctx* x, const LgcpArgs& l) {
  if (x->wide && l.B >= 128 && wide_mala_lgcp(x, l) == 0) return 0;
  if (launch_mala_lgcp(l, x->stream) == 0) return 0;
  return wide_mala_lgcp(x, l);
}

extern "C" int mfm_mala_init(mfm_ctx* x, const float* d_pos, double beta, double* d_logp, float* d_grad) { use_ctx(x);
  NEED_TARGET();
  if (!d_pos || !d_logp || !d_grad) return fail(MFM_EINVAL, "null device pointer");
  if (x->net.T.kind == MFM_TARGET_LGCP) {
    LgcpArgs l = lgcp_args(x, 0, beta, 1.0);
    l.pos = const_cast<float*>(d_pos); l.logp = d_logp; l.grad = d_grad;
    if (lgcp_mala_dispatch(x, l)) return too_large(x, "LGCP MALA");
  } else {
    MalaArgs a = mala_args(x, beta);
    a.pos = const_cast<float*>(d_pos); a.logp = d_logp; a.grad = d_grad;
    if (launch_mala_init(a, x->stream)) return too_large(x, "MALA");
  }
  LAUNCHCHK();
  return MFM_OK;
}

static int mala_step_common(mfm_ctx* x, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, double step, int textbook, float* d_pos,
                            double* d_logp, float* d_grad, float* d_acc, uint8_t* d_isacc, float* d_prop, float* d_pw) {
  NEED_TARGET();
  if (!d_pos || !d_logp || !d_grad) return fail(MFM_EINVAL, "null device pointer");
  if (!(step > 0)) return fail(MFM_EINVAL, "step_size must be positive");
  if (x->net.T.kind == MFM_TARGET_LGCP) {
    LgcpArgs l = lgcp_args(x, 1, beta, step);
    l.key = Key2{k0, k1}; l.keys = d_keys; l.textbook = textbook;
    l.pos = d_pos; l.logp = d_logp; l.grad = d_grad; l.acc_prob = d_acc; l.accepted = d_isacc; l.proposed = d_prop; l.prop_weight = d_pw;
    ProfScope ps_(x, PROF_MALA);
    if (lgcp_mala_dispatch(x, l)) return too_large(x, "LGCP MALA");
    LAUNCHCHK();
    count_mala_steps(x, x->cfg.n_chain_local);
    return MFM_OK;
  }
  MalaArgs a = mala_args(x, beta);
  a.key = Key2{k0, k1}; a.keys = d_keys; a.eps = step; a.textbook = textbook;
  if (!d_keys) {
    const int slot = noise_take(x, Key2{k0, k1}, false);
    if (slot >= 0) {
      const size_t B = (size_t)x->cfg.n_chain_local;
      a.pre_n = x->noise->mala_n + (size_t)slot * B * x->cfg.dim; a.pre_u = x->noise->mala_u + (size_t)slot * B;
    }
  }
  a.pos = d_pos; a.logp = d_logp; a.grad = d_grad;
  a.acc_prob = d_acc; a.accepted = d_isacc; a.proposed = d_prop; a.prop_weight = d_pw;
  ProfScope ps_(x, PROF_MALA);
  if (launch_mala_step(a, x->stream)) return too_large(x, "MALA");
  LAUNCHCHK();
  count_mala_steps(x, x->cfg.n_chain_local);
  return MFM_OK;
}

extern "C" int mfm_mala_step(mfm_ctx* x, uint32_t k0, uint32_t k1, double beta, double step, int textbook, float* d_pos,
                             double* d_logp, float* d_grad, float* d_acc, uint8_t* d_isacc, float* d_prop, float* d_pw) { use_ctx(x);
  return mala_step_common(x, k0, k1, nullptr, beta, step, textbook, d_pos, d_logp, d_grad, d_acc, d_isacc, d_prop, d_pw);
}
extern "C" int mfm_mala_step_keys(mfm_ctx* x, const uint32_t* d_keys, double beta, double step, int textbook, float* d_pos,
                                  double* d_logp, float* d_grad, float* d_acc, uint8_t* d_isacc, float* d_prop, float* d_pw) { use_ctx(x);
  if (!d_keys) return fail(MFM_EINVAL, "null key array");
  return mala_step_common(x, 0, 0, d_keys, beta, step, textbook, d_pos, d_logp, d_grad, d_acc, d_isacc, d_prop, d_pw);
}

// n_steps MALA steps in one call (mala_run.hip): the chain stays in registers between the steps.  The Cox process, whose step is the
// 16-chain tile of lgcp.hip, gets n_steps launches of that step back to back on the context's stream instead (keys and tallies on the device).
extern "C" int mfm_mala_run(mfm_ctx* x, int key_mode, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, double step, int textbook,
                            int32_t n_steps, int32_t thin, float* d_pos, double* d_logp, float* d_grad, int32_t* d_n_acc, double* d_acc_sum,
                            float* d_acc, uint8_t* d_isacc, float* d_prop, float* d_pw, float* d_traj_pos, double* d_traj_logp) { use_ctx(x);
  NEED_TARGET();
  CHECKED(check_state(d_pos, d_logp, d_grad, step));
  CHECKED(check_run_keys(key_mode, d_keys, n_steps));
  CHECKED(check_thin(thin, n_steps, d_traj_pos, d_traj_logp));
  const int B = x->cfg.n_chain_local, d = x->cfg.dim;
  if (x->net.T.kind == MFM_TARGET_LGCP) {
    // workspace: keys uint32 [B][2] | acc_prob float [B] | accepted uint8 [B]
    const size_t need = (size_t)B * (8 + 4 + 1);
    if (x->run_ws_cap < need) {
      if (x->run_ws) { HIPCHK(hipStreamSynchronize(x->stream)); (void)hipFree(x->run_ws); x->run_ws = nullptr; x->run_ws_cap = 0; }
      HIPCHK(hipMalloc(&x->run_ws, need));
      x->run_ws_cap = need;
    }
    uint32_t* ws_keys = (uint32_t*)x->run_ws;
    float* ws_acc = d_acc ? d_acc : (float*)((char*)x->run_ws + (size_t)B * 8);
    uint8_t* ws_isacc = d_isacc ? d_isacc : (uint8_t*)((char*)x->run_ws + (size_t)B * 12);
    const bool tally = d_n_acc || d_acc_sum;
    if (d_n_acc) HIPCHK(hipMemsetAsync(d_n_acc, 0, (size_t)B * sizeof(int32_t), x->stream));
    if (d_acc_sum) HIPCHK(hipMemsetAsync(d_acc_sum, 0, (size_t)B * sizeof(double), x->stream));
    LgcpArgs l = lgcp_args(x, 1, beta, step);
    l.keys = ws_keys; l.textbook = textbook;
    l.pos = d_pos; l.logp = d_logp; l.grad = d_grad;
    ProfScope ps_(x, PROF_MALA);
    const dim3 kgrid((B + 255) / 256), kblock(256);
    for (int s = 0; s < n_steps; ++s) {
      const bool last = s == n_steps - 1;
      hipLaunchKernelGGL(mala_run_keys_kernel, kgrid, kblock, 0, x->stream, key_mode, Key2{k0, k1}, d_keys, (uint32_t)n_steps, (uint32_t)s,
                         (uint32_t)x->cfg.n_chain_total, (uint32_t)x->cfg.chain_offset, B, ws_keys);
      l.acc_prob = (tally || (last && d_acc)) ? ws_acc : nullptr;        // (the caller's buffers where given: the last step leaves its info there)
      l.accepted = (tally || (last && d_isacc)) ? ws_isacc : nullptr;
      l.proposed = last ? d_prop : nullptr; l.prop_weight = last ? d_pw : nullptr;
      if (lgcp_mala_dispatch(x, l)) return too_large(x, "LGCP MALA");
      if (tally) hipLaunchKernelGGL(mala_run_tally_kernel, kgrid, kblock, 0, x->stream, B, ws_acc, ws_isacc, d_n_acc, d_acc_sum);
      LAUNCHCHK();
      if (thin > 0 && (s + 1) % thin == 0) {
        const size_t snap = (size_t)((s + 1) / thin - 1);
        if (d_traj_pos) HIPCHK(hipMemcpyAsync(d_traj_pos + snap * (size_t)B * d, d_pos, (size_t)B * d * sizeof(float), hipMemcpyDeviceToDevice, x->stream));
        if (d_traj_logp) HIPCHK(hipMemcpyAsync(d_traj_logp + snap * (size_t)B, d_logp, (size_t)B * sizeof(double), hipMemcpyDeviceToDevice, x->stream));
      }
    }
    count_mala_steps(x, (int64_t)B * n_steps);
    return MFM_OK;
  }
  MalaRunArgs r; memset(&r, 0, sizeof r);
  r.m = mala_run_args(x, key_mode, k0, k1, d_keys, beta, step, textbook, d_pos, d_logp, d_grad);
  r.m.acc_prob = d_acc; r.m.accepted = d_isacc; r.m.proposed = d_prop; r.m.prop_weight = d_pw;
  r.t = RunTail{key_mode, n_steps, thin, d_n_acc, d_acc_sum, d_traj_pos, d_traj_logp};
  ProfScope ps_(x, PROF_MALA);
  if (launch_mala_run(r, x->stream)) return too_large(x, "MALA");
  LAUNCHCHK();
  // state in and out once, the trajectory rows that were kept
  x->ctr[CTR_MALA] += (int64_t)B * n_steps;
  x->ctr[CTR_MALA_BYTES] += (int64_t)B * 4 * (4 * d + 4) + (thin > 0 ? (int64_t)(n_steps / thin) * B * (4 * (d_traj_pos ? d : 0) + (d_traj_logp ? 8 : 0)) : 0);
  return MFM_OK;
}

// ---- elliptical slice sampling for the Cox process (eslice.hip) ----
// L of the prior covariance K = L L^T, packed transposed like K^-1 (mfm_set_target): nu = n . L^T is the tile GEMM's product
extern "C" int mfm_set_lgcp_chol(mfm_ctx* x, const double* h_chol) { use_ctx(x);
  NEED_TARGET();
  if (!h_chol) return fail(MFM_EINVAL, "null argument");
  if (x->net.T.kind != MFM_TARGET_LGCP) return fail(MFM_EUNSUPPORTED, "the Cholesky factor belongs to the Cox process: this target has no Gaussian prior factor");
  const int d = x->cfg.dim, dp = x->net.dp, KB = dp / 16;
  for (int j = 0; j < d; ++j)
    for (int k = 0; k < d; ++k) {
      const double v = h_chol[(size_t)j * d + k];
      if (!std::isfinite(v)) return fail(MFM_EINVAL, "chol[%d][%d] = %g: every entry must be finite", j, k, v);
      if (k > j && v != 0.0) return fail(MFM_EINVAL, "chol[%d][%d] = %g: the factor must be lower triangular", j, k, v);
    }
  std::vector<float> lp((size_t)dp * dp, 0.f);
  for (int j = 0; j < d; ++j)
    for (int k = 0; k <= j; ++k) lp[pack_index(k, j, KB)] = (float)h_chol[(size_t)j * d + k];      // W[k][j] = L^T[k][j] = L[j][k]
  if (!x->lgcp_chol) ALLOC(x->lgcp_chol, (size_t)dp * dp);
  // stream-ordered behind the launches that still read the previous factor; the host vector is a temporary: wait
  HIPCHK(hipMemcpyAsync(x->lgcp_chol, lp.data(), (size_t)dp * dp * 4, hipMemcpyHostToDevice, x->stream));
  HIPCHK(hipStreamSynchronize(x->stream));
  return MFM_OK;
}

static EsliceArgs eslice_args(mfm_ctx* x, int mode, double beta) {
  EsliceArgs e; memset(&e, 0, sizeof e);
  e.T = x->net.T; e.dp = x->net.dp; e.cholP = x->lgcp_chol; e.mode = mode;
  e.n_total = x->cfg.n_chain_total; e.chain_offset = x->cfg.chain_offset; e.B = x->cfg.n_chain_local; e.beta = beta; e.n_steps = 1;
  return e;
}
// the checks every transition entry point makes after its own (the state pointers first, as mfm_mala_run)
static int check_eslice(mfm_ctx* x, double beta, bool need_chol) {
  if (x->net.T.kind != MFM_TARGET_LGCP)
    return fail(MFM_EUNSUPPORTED, "elliptical slice sampling serves the Cox process: this target has no Gaussian prior factor");
  if (need_chol && !x->lgcp_chol) return fail(MFM_ENOTARGET, "mfm_set_lgcp_chol has not been called");
  if (!(std::isfinite(beta) && beta >= 0)) return fail(MFM_EINVAL, "beta must be finite and not negative (got %g)", beta);
  if (x->cfg.n_chain_local % 16) return fail(MFM_EINVAL, "n_chain_local (%d) must be a multiple of 16 (one tile of 16 chains per workgroup)", x->cfg.n_chain_local);
  return MFM_OK;
}
extern "C" int mfm_eslice_init(mfm_ctx* x, const float* d_pos, double* d_loglik) { use_ctx(x);
  NEED_TARGET();
  if (!d_pos || !d_loglik) return fail(MFM_EINVAL, "null device pointer");
  CHECKED(check_eslice(x, 0.0, false));
  EsliceArgs e = eslice_args(x, 0, 0.0);
  e.pos = const_cast<float*>(d_pos); e.loglik = d_loglik;
  if (launch_eslice(e, x->stream)) return too_large(x, "elliptical slice");
  LAUNCHCHK();
  return MFM_OK;
}
static int eslice_step_common(mfm_ctx* x, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, float* d_pos, double* d_loglik,
                              int32_t* d_subiter, double* d_theta, float* d_momentum) {
  NEED_TARGET();
  if (!d_pos || !d_loglik) return fail(MFM_EINVAL, "null device pointer");
  CHECKED(check_eslice(x, beta, true));
  EsliceArgs e = eslice_args(x, 1, beta);
  e.key = Key2{k0, k1}; e.keys = d_keys;
  e.pos = d_pos; e.loglik = d_loglik; e.subiter = d_subiter; e.theta = d_theta; e.momentum = d_momentum;
  ProfScope ps_(x, PROF_MALA);
  if (launch_eslice(e, x->stream)) return too_large(x, "elliptical slice");
  LAUNCHCHK();
  x->ctr[CTR_MALA] += x->cfg.n_chain_local;
  return MFM_OK;
}
extern "C" int mfm_eslice_step(mfm_ctx* x, uint32_t k0, uint32_t k1, double beta, float* d_pos, double* d_loglik,
                               int32_t* d_subiter, double* d_theta, float* d_momentum) { use_ctx(x);
  return eslice_step_common(x, k0, k1, nullptr, beta, d_pos, d_loglik, d_subiter, d_theta, d_momentum);
}
extern "C" int mfm_eslice_step_keys(mfm_ctx* x, const uint32_t* d_keys, double beta, float* d_pos, double* d_loglik,
                                    int32_t* d_subiter, double* d_theta, float* d_momentum) { use_ctx(x);
  if (!d_keys) return fail(MFM_EINVAL, "null key array");
  return eslice_step_common(x, 0, 0, d_keys, beta, d_pos, d_loglik, d_subiter, d_theta, d_momentum);
}
// n_steps transitions in ONE launch: the tile's rows stay in registers, L^T is streamed again once per transition
extern "C" int mfm_eslice_run(mfm_ctx* x, int key_mode, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, int32_t n_steps, int32_t thin,
                              float* d_pos, double* d_loglik, int32_t* d_subiter_sum, int32_t* d_n_capped, float* d_traj_pos,
                              double* d_traj_loglik, int32_t* d_subiter, double* d_theta, float* d_momentum, int32_t* d_subiter_max) { use_ctx(x);
  NEED_TARGET();
  if (!d_pos || !d_loglik) return fail(MFM_EINVAL, "null device pointer");
  CHECKED(check_run_keys(key_mode, d_keys, n_steps));
  CHECKED(check_thin(thin, n_steps, d_traj_pos, d_traj_loglik));
  CHECKED(check_eslice(x, beta, true));
  EsliceArgs e = eslice_args(x, 2, beta);
  e.key_mode = key_mode; e.key = Key2{k0, k1}; e.keys = key_mode == 1 ? d_keys : nullptr; e.n_steps = n_steps; e.thin = thin;
  e.pos = d_pos; e.loglik = d_loglik; e.subiter_sum = d_subiter_sum; e.n_capped = d_n_capped; e.traj_pos = d_traj_pos; e.traj_loglik = d_traj_loglik;
  e.subiter = d_subiter; e.theta = d_theta; e.momentum = d_momentum; e.subiter_max = d_subiter_max;
  ProfScope ps_(x, PROF_MALA);
  if (launch_eslice(e, x->stream)) return too_large(x, "elliptical slice");
  LAUNCHCHK();
  x->ctr[CTR_MALA] += (int64_t)x->cfg.n_chain_local * n_steps;
  return MFM_OK;
}
extern "C" int mfm_eslice_launch_plan(int32_t dim, int32_t* h_tpw, int32_t* h_lds_bytes) {
  if (!h_tpw || !h_lds_bytes) return fail(MFM_EINVAL, "mfm_eslice_launch_plan: null output pointer");
  if (dim < 1) return fail(MFM_EINVAL, "mfm_eslice_launch_plan: dim must be positive (got %d)", dim);
  int tpw; size_t sm;
  eslice_plan((dim + 15) / 16 * 16, &tpw, &sm);
  if (!tpw || sm > 160 * 1024) return fail(MFM_ETOOLARGE, "dim %d too large for the elliptical slice kernel", dim);
  *h_tpw = tpw; *h_lds_bytes = (int32_t)sm;
  return MFM_OK;
}

// the HMC entry points' own two checks (shared like the ones above)
static int check_num_steps(int num_steps) {
  if (num_steps < 1 || num_steps > 100000) return fail(MFM_EINVAL, "num_steps must be in [1, 100000] (got %d)", num_steps);
  return MFM_OK;
}
static int hmc_refuse_cox(mfm_ctx* x) {
  if (x->net.T.kind == MFM_TARGET_LGCP) return fail(MFM_EUNSUPPORTED, "the HMC step serves the phi-four and mixture targets (the Cox process needs the K^-1 GEMM tile)");
  return MFM_OK;
}
// Build-side mode (hmc.hip; not on the reference's MFM path): one HMC step of every local chain, state updated in place like mfm_mala_step
static HmcArgs hmc_args(mfm_ctx* x, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, double step, int num_steps, float* d_pos,
                        double* d_logp, float* d_grad, float* d_acc, uint8_t* d_isacc) {
  HmcArgs a; memset(&a, 0, sizeof a);
  a.T = x->net.T; a.key = Key2{k0, k1}; a.keys = d_keys; a.n_total = x->cfg.n_chain_total; a.chain_offset = x->cfg.chain_offset; a.B = x->cfg.n_chain_local;
  a.num_steps = num_steps; a.beta = beta; a.eps = step;
  a.pos = d_pos; a.logp = d_logp; a.grad = d_grad; a.acc_prob = d_acc; a.accepted = d_isacc;
  a.minv = x->h_inv_mass.empty() ? nullptr : x->d_inv_mass;      // (set: the mass instances)
  return a;
}

// The diagonal of the inverse mass matrix of every later HMC call of this context (hmc.hip).  A rejected call changes nothing.
static int inv_mass_upload(mfm_ctx* x, const std::vector<double>& h) {
  if (!x->d_inv_mass) HIPCHK(hipMalloc(&x->d_inv_mass, sizeof(double) * (size_t)x->cfg.dim));
  // stream-ordered behind the launches that still read the previous vector; the host vector is a temporary or about to change: wait
  HIPCHK(hipMemcpyAsync(x->d_inv_mass, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, x->stream));
  HIPCHK(hipStreamSynchronize(x->stream));
  return MFM_OK;
}
extern "C" int mfm_hmc_set_inverse_mass(mfm_ctx* x, const double* h_inv_mass, int32_t n) { use_ctx(x);
  if (!x) return fail(MFM_EINVAL, "null ctx");
  const int d = x->cfg.dim;
  if (n == 0 && !h_inv_mass) {                       // back to unit mass and the unit instances
    if (!x->h_inv_mass.empty() && x->d_inv_mass) { if (const int rc = inv_mass_upload(x, std::vector<double>((size_t)d, 1.0))) return rc; }
    x->h_inv_mass.clear();
    return MFM_OK;
  }
  if (n != d || !h_inv_mass) return fail(MFM_EINVAL, "inv_mass must hold dim = %d entries (got n = %d%s); n = 0 with a null pointer returns to unit mass", d, n, h_inv_mass ? "" : ", null pointer");
  for (int j = 0; j < d; ++j)
    if (!(std::isfinite(h_inv_mass[j]) && h_inv_mass[j] > 0)) return fail(MFM_EINVAL, "inv_mass[%d] = %g: every entry must be finite and positive", j, h_inv_mass[j]);
  const std::vector<double> h(h_inv_mass, h_inv_mass + d);
  if (const int rc = inv_mass_upload(x, h)) return rc;
  x->h_inv_mass = h;
  return MFM_OK;
}
extern "C" int mfm_hmc_get_inverse_mass(mfm_ctx* x, double* h_out, int32_t* h_is_set) { use_ctx(x);
  if (!x) return fail(MFM_EINVAL, "null ctx");
  const bool set = !x->h_inv_mass.empty();
  if (h_out) for (int j = 0; j < x->cfg.dim; ++j) h_out[j] = set ? x->h_inv_mass[(size_t)j] : 1.0;
  if (h_is_set) *h_is_set = set ? 1 : 0;
  return MFM_OK;
}

static int hmc_step_common(mfm_ctx* x, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, double step, int num_steps, float* d_pos,
                           double* d_logp, float* d_grad, float* d_acc, uint8_t* d_isacc) {
  NEED_TARGET();
  CHECKED(check_state(d_pos, d_logp, d_grad, step));
  CHECKED(check_num_steps(num_steps));
  CHECKED(hmc_refuse_cox(x));
  const HmcArgs a = hmc_args(x, k0, k1, d_keys, beta, step, num_steps, d_pos, d_logp, d_grad, d_acc, d_isacc);
  ProfScope ps_(x, PROF_MALA);
  if (launch_hmc_step(a, x->stream)) return too_large(x, "HMC");
  LAUNCHCHK();
  x->ctr[CTR_MALA] += x->cfg.n_chain_local;
  return MFM_OK;
}

extern "C" int mfm_hmc_step(mfm_ctx* x, uint32_t k0, uint32_t k1, double beta, double step, int num_steps, float* d_pos, double* d_logp,
                            float* d_grad, float* d_acc, uint8_t* d_isacc) { use_ctx(x);
  return hmc_step_common(x, k0, k1, nullptr, beta, step, num_steps, d_pos, d_logp, d_grad, d_acc, d_isacc);
}
extern "C" int mfm_hmc_step_keys(mfm_ctx* x, const uint32_t* d_keys, double beta, double step, int num_steps, float* d_pos, double* d_logp,
                                 float* d_grad, float* d_acc, uint8_t* d_isacc) { use_ctx(x);
  if (!d_keys) return fail(MFM_EINVAL, "null key array");
  return hmc_step_common(x, 0, 0, d_keys, beta, step, num_steps, d_pos, d_logp, d_grad, d_acc, d_isacc);
}

// n_steps HMC steps in one launch (hmc_run.hip): the chain stays in registers between the steps; arguments as mfm_mala_run's
extern "C" int mfm_hmc_run(mfm_ctx* x, int key_mode, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, double step, int32_t num_steps,
                           int32_t n_steps, int32_t thin, float* d_pos, double* d_logp, float* d_grad, int32_t* d_n_acc, double* d_acc_sum,
                           float* d_acc, uint8_t* d_isacc, float* d_traj_pos, double* d_traj_logp) { use_ctx(x);
  NEED_TARGET();
  CHECKED(check_state(d_pos, d_logp, d_grad, step));
  CHECKED(check_num_steps(num_steps));
  CHECKED(check_run_keys(key_mode, d_keys, n_steps));
  CHECKED(check_thin(thin, n_steps, d_traj_pos, d_traj_logp));
  CHECKED(hmc_refuse_cox(x));
  HmcRunArgs r; memset(&r, 0, sizeof r);
  r.h = hmc_args(x, k0, k1, key_mode == 1 ? d_keys : nullptr, beta, step, num_steps, d_pos, d_logp, d_grad, d_acc, d_isacc);
  r.t = RunTail{key_mode, n_steps, thin, d_n_acc, d_acc_sum, d_traj_pos, d_traj_logp};
  ProfScope ps_(x, PROF_MALA);
  if (launch_hmc_run(r, x->stream)) return too_large(x, "HMC");
  LAUNCHCHK();
  // steps only, next to mfm_hmc_step's: CTR_MALA_BYTES is the MALA kernels' traffic and covers no HMC entry point
  x->ctr[CTR_MALA] += (int64_t)x->cfg.n_chain_local * n_steps;
  return MFM_OK;
}

// mfm_hmc_run with one leapfrog count per step (chees.hip): mfm_hmc_run's checks in its order, the array in num_steps' place
extern "C" int mfm_hmc_run_lengths(mfm_ctx* x, int key_mode, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, double step,
                                   const int32_t* d_num_steps, int32_t n_steps, int32_t thin, float* d_pos, double* d_logp, float* d_grad,
                                   int32_t* d_n_acc, double* d_acc_sum, float* d_acc, uint8_t* d_isacc, float* d_traj_pos, double* d_traj_logp,
                                   int64_t* d_total_leapfrog) { use_ctx(x);
  NEED_TARGET();
  CHECKED(check_state(d_pos, d_logp, d_grad, step));
  if (!d_num_steps) return fail(MFM_EINVAL, "d_num_steps must not be null (one leapfrog count per step)");
  CHECKED(check_run_keys(key_mode, d_keys, n_steps));
  CHECKED(check_thin(thin, n_steps, d_traj_pos, d_traj_logp));
  CHECKED(hmc_refuse_cox(x));
  HmcRunArgs r; memset(&r, 0, sizeof r);
  r.h = hmc_args(x, k0, k1, key_mode == 1 ? d_keys : nullptr, beta, step, 0, d_pos, d_logp, d_grad, d_acc, d_isacc);
  r.t = RunTail{key_mode, n_steps, thin, d_n_acc, d_acc_sum, d_traj_pos, d_traj_logp};
  ProfScope ps_(x, PROF_MALA);
  if (launch_hmc_run_lengths(r, d_num_steps, d_total_leapfrog, x->stream)) return too_large(x, "HMC");
  LAUNCHCHK();
  x->ctr[CTR_MALA] += (int64_t)x->cfg.n_chain_local * n_steps;      // (steps only, as mfm_hmc_run)
  return MFM_OK;
}

// Microcanonical Langevin Monte Carlo (mclmc.hip).  Checks in mfm_hmc_run's order, then the sampler's own: a rejected call touches nothing.
static double mclmc_refresh_scale(double step, double L, int dim) {      // nu (mclmc.hip); L = +inf: exp(0) - 1 = 0 exactly
  return std::sqrt((std::exp(2.0 * step / L) - 1.0) / (double)dim);
}
static int mclmc_check(mfm_ctx* x, double step, double L, int integrator) {
  CHECKED(hmc_refuse_cox(x));
  if (!x->h_inv_mass.empty()) return fail(MFM_EUNSUPPORTED, "MCLMC runs at unit mass: remove the installed inverse mass (mfm_hmc_set_inverse_mass with n = 0)");
  if (x->cfg.dim < 2) return fail(MFM_EINVAL, "dim must be at least 2 for MCLMC (got %d): the momentum lives on the unit sphere", x->cfg.dim);
  if (!(step > 0) || std::isinf(step)) return fail(MFM_EINVAL, "step_size must be positive and finite (got %g)", step);
  if (!(L > 0)) return fail(MFM_EINVAL, "L must be positive, +inf for no momentum refresh (got %g)", L);
  if (!std::isfinite(mclmc_refresh_scale(step, L, x->cfg.dim)))
    return fail(MFM_EINVAL, "L = %g is too small for step_size %g: the refresh scale sqrt((exp(2 step_size / L) - 1) / dim) is not finite", L, step);
  if (integrator != 0 && integrator != 1) return fail(MFM_EINVAL, "integrator must be 0 (leapfrog) or 1 (McLachlan) (got %d)", integrator);
  return MFM_OK;
}
static MclmcArgs mclmc_args(mfm_ctx* x, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, double step, double L, int integrator,
                            float* d_pos, double* d_logp, float* d_grad, double* d_mom, double* d_de, double* d_dk) {
  MclmcArgs a; memset(&a, 0, sizeof a);
  a.T = x->net.T; a.key = Key2{k0, k1}; a.keys = d_keys; a.n_total = x->cfg.n_chain_total; a.chain_offset = x->cfg.chain_offset; a.B = x->cfg.n_chain_local;
  a.beta = beta;
  // the schedule's coefficient table (tests/mclmc_ref.py: SCHEDULES): leapfrog B A B, McLachlan's minimal-norm scheme B A B A B
  const double b1 = 0.1931833275037836;
  if (integrator == 0) { a.n_stages = 1; a.hb[0] = 0.5 * step; a.hb[1] = 0.5 * step; a.ha[0] = 1.0 * step; }
  else { a.n_stages = 2; a.hb[0] = b1 * step; a.hb[1] = (1.0 - 2.0 * b1) * step; a.hb[2] = b1 * step; a.ha[0] = 0.5 * step; a.ha[1] = 0.5 * step; }
  a.nu = mclmc_refresh_scale(step, L, x->cfg.dim);
  a.pos = d_pos; a.logp = d_logp; a.grad = d_grad; a.mom = d_mom; a.energy_change = d_de; a.kinetic_change = d_dk;
  return a;
}
extern "C" int mfm_mclmc_init(mfm_ctx* x, uint32_t k0, uint32_t k1, double* d_momentum) { use_ctx(x);
  NEED_TARGET();
  if (!d_momentum) return fail(MFM_EINVAL, "null device pointer");
  CHECKED(hmc_refuse_cox(x));
  if (x->cfg.dim < 2) return fail(MFM_EINVAL, "dim must be at least 2 for MCLMC (got %d): the momentum lives on the unit sphere", x->cfg.dim);
  ProfScope ps_(x, PROF_MALA);
  launch_mclmc_init(Key2{k0, k1}, (uint32_t)x->cfg.n_chain_total, (uint32_t)x->cfg.chain_offset, x->cfg.n_chain_local, x->cfg.dim, d_momentum, x->stream);
  LAUNCHCHK();
  return MFM_OK;
}
static int mclmc_step_common(mfm_ctx* x, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, double step, double L, int integrator,
                             float* d_pos, double* d_logp, float* d_grad, double* d_mom, double* d_de, double* d_dk) {
  NEED_TARGET();
  if (!d_pos || !d_logp || !d_grad || !d_mom) return fail(MFM_EINVAL, "null device pointer");
  CHECKED(mclmc_check(x, step, L, integrator));
  const MclmcArgs a = mclmc_args(x, k0, k1, d_keys, beta, step, L, integrator, d_pos, d_logp, d_grad, d_mom, d_de, d_dk);
  ProfScope ps_(x, PROF_MALA);
  if (launch_mclmc_step(a, x->stream)) return too_large(x, "MCLMC");
  LAUNCHCHK();
  x->ctr[CTR_MALA] += x->cfg.n_chain_local;      // (steps only, as mfm_hmc_step)
  return MFM_OK;
}
extern "C" int mfm_mclmc_step(mfm_ctx* x, uint32_t k0, uint32_t k1, double beta, double step, double L, int integrator, float* d_pos, double* d_logp,
                              float* d_grad, double* d_mom, double* d_de, double* d_dk) { use_ctx(x);
  return mclmc_step_common(x, k0, k1, nullptr, beta, step, L, integrator, d_pos, d_logp, d_grad, d_mom, d_de, d_dk);
}
extern "C" int mfm_mclmc_step_keys(mfm_ctx* x, const uint32_t* d_keys, double beta, double step, double L, int integrator, float* d_pos, double* d_logp,
                                   float* d_grad, double* d_mom, double* d_de, double* d_dk) { use_ctx(x);
  if (!d_keys) return fail(MFM_EINVAL, "null key array");
  return mclmc_step_common(x, 0, 0, d_keys, beta, step, L, integrator, d_pos, d_logp, d_grad, d_mom, d_de, d_dk);
}
extern "C" int mfm_mclmc_run(mfm_ctx* x, int key_mode, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, double step, double L, int integrator,
                             int32_t n_steps, int32_t thin, float* d_pos, double* d_logp, float* d_grad, double* d_mom, double* d_de_sum,
                             double* d_de_sumsq, int32_t* d_n_nonfinite, double* d_energy_trace, float* d_traj_pos, double* d_traj_logp) { use_ctx(x);
  NEED_TARGET();
  if (!d_pos || !d_logp || !d_grad || !d_mom) return fail(MFM_EINVAL, "null device pointer");
  CHECKED(check_run_keys(key_mode, d_keys, n_steps));
  CHECKED(check_thin(thin, n_steps, d_traj_pos, d_traj_logp));
  CHECKED(mclmc_check(x, step, L, integrator));
  MclmcRunArgs r; memset(&r, 0, sizeof r);
  r.m = mclmc_args(x, k0, k1, key_mode == 1 ? d_keys : nullptr, beta, step, L, integrator, d_pos, d_logp, d_grad, d_mom, nullptr, nullptr);
  r.t = RunTail{key_mode, n_steps, thin, nullptr, nullptr, d_traj_pos, d_traj_logp};
  r.de_sum = d_de_sum; r.de_sumsq = d_de_sumsq; r.n_nonfinite = d_n_nonfinite; r.energy_trace = d_energy_trace;
  ProfScope ps_(x, PROF_MALA);
  if (launch_mclmc_run(r, x->stream)) return too_large(x, "MCLMC");
  LAUNCHCHK();
  x->ctr[CTR_MALA] += (int64_t)x->cfg.n_chain_local * n_steps;      // (steps only, as mfm_hmc_run)
  return MFM_OK;
}

// Generalized HMC with persistent momentum (ghmc.hip).  Checks in mfm_hmc_run's order, then the sampler's own: a rejected call touches nothing.
static int ghmc_check(mfm_ctx* x, double step, double alpha, double delta) {
  CHECKED(hmc_refuse_cox(x));
  if (!(step > 0) || std::isinf(step)) return fail(MFM_EINVAL, "step_size must be positive and finite (got %g)", step);
  if (!(alpha > 0 && alpha <= 1)) return fail(MFM_EINVAL, "alpha must be in (0, 1] (got %g)", alpha);
  if (!(delta >= 0) || std::isinf(delta)) return fail(MFM_EINVAL, "delta must be finite and not negative (got %g)", delta);
  return MFM_OK;
}
static GhmcArgs ghmc_args(mfm_ctx* x, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, double step, double alpha, double delta,
                          const double* d_inverse_mass, float* d_pos, double* d_logp, float* d_grad, double* d_mom, double* d_slice,
                          float* d_acc, uint8_t* d_isacc, double* d_de) {
  GhmcArgs a; memset(&a, 0, sizeof a);
  a.T = x->net.T; a.key = Key2{k0, k1}; a.keys = d_keys; a.n_total = x->cfg.n_chain_total; a.chain_offset = x->cfg.chain_offset; a.B = x->cfg.n_chain_local;
  a.beta = beta; a.eps = step; a.alpha = alpha; a.delta = delta;
  a.pos = d_pos; a.logp = d_logp; a.grad = d_grad; a.mom = d_mom; a.slice = d_slice;
  a.acc_prob = d_acc; a.accepted = d_isacc; a.energy_change = d_de;
  a.minv = d_inverse_mass;      // the call's own (non-null: the MASS instances); the context's installed inverse mass is not read
  return a;
}
extern "C" int mfm_ghmc_init(mfm_ctx* x, uint32_t k0, uint32_t k1, const double* d_inverse_mass, double* d_momentum, double* d_slice) { use_ctx(x);
  NEED_TARGET();
  if (!d_momentum || !d_slice) return fail(MFM_EINVAL, "null device pointer");
  CHECKED(hmc_refuse_cox(x));
  ProfScope ps_(x, PROF_MALA);
  launch_ghmc_init(Key2{k0, k1}, (uint32_t)x->cfg.n_chain_total, (uint32_t)x->cfg.chain_offset, x->cfg.n_chain_local, x->cfg.dim, d_inverse_mass,
                   d_momentum, d_slice, x->stream);
  LAUNCHCHK();
  return MFM_OK;
}
static int ghmc_step_common(mfm_ctx* x, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, double step, double alpha, double delta,
                            const double* d_inverse_mass, float* d_pos, double* d_logp, float* d_grad, double* d_mom, double* d_slice,
                            float* d_acc, uint8_t* d_isacc, double* d_de) {
  NEED_TARGET();
  if (!d_pos || !d_logp || !d_grad || !d_mom || !d_slice) return fail(MFM_EINVAL, "null device pointer");
  CHECKED(ghmc_check(x, step, alpha, delta));
  const GhmcArgs a = ghmc_args(x, k0, k1, d_keys, beta, step, alpha, delta, d_inverse_mass, d_pos, d_logp, d_grad, d_mom, d_slice, d_acc, d_isacc, d_de);
  ProfScope ps_(x, PROF_MALA);
  if (launch_ghmc_step(a, x->stream)) return too_large(x, "GHMC");
  LAUNCHCHK();
  x->ctr[CTR_MALA] += x->cfg.n_chain_local;      // (steps only, as mfm_hmc_step)
  return MFM_OK;
}
extern "C" int mfm_ghmc_step(mfm_ctx* x, uint32_t k0, uint32_t k1, double beta, double step, double alpha, double delta, const double* d_inverse_mass,
                             float* d_pos, double* d_logp, float* d_grad, double* d_mom, double* d_slice, float* d_acc, uint8_t* d_isacc,
                             double* d_de) { use_ctx(x);
  return ghmc_step_common(x, k0, k1, nullptr, beta, step, alpha, delta, d_inverse_mass, d_pos, d_logp, d_grad, d_mom, d_slice, d_acc, d_isacc, d_de);
}
extern "C" int mfm_ghmc_step_keys(mfm_ctx* x, const uint32_t* d_keys, double beta, double step, double alpha, double delta, const double* d_inverse_mass,
                                  float* d_pos, double* d_logp, float* d_grad, double* d_mom, double* d_slice, float* d_acc, uint8_t* d_isacc,
                                  double* d_de) { use_ctx(x);
  if (!d_keys) return fail(MFM_EINVAL, "null key array");
  return ghmc_step_common(x, 0, 0, d_keys, beta, step, alpha, delta, d_inverse_mass, d_pos, d_logp, d_grad, d_mom, d_slice, d_acc, d_isacc, d_de);
}
extern "C" int mfm_ghmc_run(mfm_ctx* x, int key_mode, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, double step, double alpha, double delta,
                            const double* d_inverse_mass, int32_t n_steps, int32_t thin, float* d_pos, double* d_logp, float* d_grad, double* d_mom,
                            double* d_slice, int32_t* d_n_acc, double* d_acc_sum, double* d_de_acc_sum, float* d_acc, uint8_t* d_isacc, double* d_de,
                            float* d_traj_pos, double* d_traj_logp) { use_ctx(x);
  NEED_TARGET();
  if (!d_pos || !d_logp || !d_grad || !d_mom || !d_slice) return fail(MFM_EINVAL, "null device pointer");
  CHECKED(check_run_keys(key_mode, d_keys, n_steps));
  CHECKED(check_thin(thin, n_steps, d_traj_pos, d_traj_logp));
  CHECKED(ghmc_check(x, step, alpha, delta));
  GhmcRunArgs r; memset(&r, 0, sizeof r);
  r.m = ghmc_args(x, k0, k1, key_mode == 1 ? d_keys : nullptr, beta, step, alpha, delta, d_inverse_mass, d_pos, d_logp, d_grad, d_mom, d_slice,
                  d_acc, d_isacc, d_de);
  r.t = RunTail{key_mode, n_steps, thin, d_n_acc, d_acc_sum, d_traj_pos, d_traj_logp};
  r.de_acc_sum = d_de_acc_sum;
  ProfScope ps_(x, PROF_MALA);
  if (launch_ghmc_run(r, x->stream)) return too_large(x, "GHMC");
  LAUNCHCHK();
  x->ctr[CTR_MALA] += (int64_t)x->cfg.n_chain_local * n_steps;      // (steps only, as mfm_hmc_run)
  return MFM_OK;
}

static size_t chees_align(size_t n);      // (defined with the ChEES warmup below: 256-byte sections of a workspace)
// MEADS warmup of GHMC (ghmc.hip): per iteration four statistics launches, the step and the acceptance mean, enqueued back to back; the
// host reads nothing until the end
extern "C" int mfm_meads_plan(int32_t n_valid, int32_t n_folds, int32_t dim, int32_t* h_out) {
  if (!h_out) return fail(MFM_EINVAL, "null output pointer");
  if (n_folds < 2) return fail(MFM_EINVAL, "n_folds must be at least 2 (got %d)", n_folds);
  if (n_valid < 2 * n_folds || n_valid % n_folds) return fail(MFM_EINVAL, "n_valid (%d) must be a multiple of n_folds (%d) with at least 2 chains per fold", n_valid, n_folds);
  if (dim < 1) return fail(MFM_EINVAL, "dim must be positive (got %d)", dim);
  const MeadsPlan p = meads_plan(n_valid, n_folds, dim);
  h_out[0] = p.m; h_out[1] = p.m_pad; h_out[2] = p.d_pad; h_out[3] = p.gram_workgroups;
  return MFM_OK;
}
extern "C" int mfm_meads_warmup(mfm_ctx* x, int key_mode, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, double step0, double alpha0,
                                int32_t n_iter, int32_t n_valid, int32_t n_folds, int32_t shuffle_every, const int32_t* d_perms, float* d_pos,
                                double* d_logp, float* d_grad, double* d_mom, double* d_slice, double* h_result, double* d_inverse_mass_out,
                                double* d_trace, double* d_mass_trace) { use_ctx(x);
  NEED_TARGET();
  if (!d_pos || !d_logp || !d_grad || !d_mom || !d_slice) return fail(MFM_EINVAL, "null device pointer");
  CHECKED(check_run_keys(key_mode, d_keys, n_iter));
  CHECKED(ghmc_check(x, step0, alpha0, 0.0));
  const int B = x->cfg.n_chain_local, d = x->cfg.dim, K = n_folds;
  if (x->cfg.n_chain_total != B)
    return fail(MFM_EUNSUPPORTED, "the MEADS warmup serves one rank (n_chain_total %d != n_chain_local %d): the fold statistics would need an all-reduce", x->cfg.n_chain_total, B);
  if (K < 2) return fail(MFM_EINVAL, "n_folds must be at least 2 (got %d)", K);
  if (n_valid < 2 * K || n_valid % K || n_valid > B)
    return fail(MFM_EINVAL, "n_valid (%d) must be a multiple of n_folds (%d) with at least 2 chains per fold and at most n_chain_local = %d", n_valid, K, B);
  if (shuffle_every < 0) return fail(MFM_EINVAL, "shuffle_every must not be negative (got %d)", shuffle_every);
  const int n_shuffles = shuffle_every > 0 ? (n_iter - 1) / shuffle_every : 0;
  if (n_shuffles > 0 && !d_perms) return fail(MFM_EINVAL, "shuffle_every > 0 needs d_perms (int32 [(n_iter - 1) / shuffle_every][n_valid], one permutation per shuffle)");
  if ((d + 63) / 64 > 32) return too_large(x, "GHMC");
  const MeadsPlan p = meads_plan(n_valid, K, d), pall = meads_plan(n_valid, 1, d);      // (pall: the closing pass, one fold of all chains)
  // workspace: par [K][8 + d] | fold_of [B] | mu, sd [K][d] | norms [2][K][m_pad] | part | acc [B] | result [4] | yz [2][K][m_pad][d_pad]
  const size_t n_part = 2 * (size_t)std::max(K * p.n_tiles, pall.n_tiles);
  const size_t o_fold = chees_align(8 * (size_t)K * (MEADS_PAR + d)), o_mu = o_fold + chees_align(4 * (size_t)B), o_sd = o_mu + chees_align(8 * (size_t)K * d),
               o_norm = o_sd + chees_align(8 * (size_t)K * d), o_part = o_norm + chees_align(16 * (size_t)K * p.m_pad), o_acc = o_part + chees_align(8 * n_part),
               o_res = o_acc + chees_align(8 * (size_t)B), o_yz = o_res + chees_align(32),
               need = o_yz + chees_align(8 * (size_t)K * p.m_pad * p.d_pad);
  if (x->meads_ws_cap < need) {
    if (x->meads_ws) { HIPCHK(hipStreamSynchronize(x->stream)); (void)hipFree(x->meads_ws); x->meads_ws = nullptr; x->meads_ws_cap = 0; }
    HIPCHK(hipMalloc(&x->meads_ws, need));
    x->meads_ws_cap = need;
  }
  char* ws = (char*)x->meads_ws;
  HIPCHK(hipMemsetAsync(ws + o_fold, 0, 4 * (size_t)B, x->stream));      // (a d_perms that is no permutation leaves entries unwritten: fold 0)
  MeadsBufs b;
  b.par = (double*)ws; b.fold_of = (int32_t*)(ws + o_fold); b.mu = (double*)(ws + o_mu); b.sd = (double*)(ws + o_sd); b.norms = (double*)(ws + o_norm);
  b.part = (double*)(ws + o_part); b.acc = (double*)(ws + o_acc); b.result = (double*)(ws + o_res); b.yz = (float*)(ws + o_yz);
  const GhmcArgs a = ghmc_args(x, k0, k1, key_mode == 1 ? d_keys : nullptr, beta, step0, alpha0, 0.0, nullptr, d_pos, d_logp, d_grad, d_mom, d_slice,
                               nullptr, nullptr, nullptr);
  ProfScope ps_(x, PROF_MALA);
  hipLaunchKernelGGL(meads_begin_kernel, dim3(std::min(64, (K * (MEADS_PAR + d) + 255) / 256)), dim3(256), 0, x->stream, b.par, K, d, step0, alpha0);
  const int32_t* perm = nullptr;
  for (int t = 1; t <= n_iter; ++t) {
    const int r = shuffle_every > 0 ? (t - 1) / shuffle_every : 0;      // the membership in force: identity, then d_perms[r - 1]
    const int32_t* pt = r == 0 ? nullptr : d_perms + (size_t)(r - 1) * n_valid;
    if (t == 1 || pt != perm) hipLaunchKernelGGL(meads_fold_kernel, dim3((B + 255) / 256), dim3(256), 0, x->stream, pt, n_valid, p.m, B, b.fold_of);
    perm = pt;
    double* trace_t = d_trace ? d_trace + (size_t)(t - 1) * K * 6 : nullptr;
    launch_meads_stats(b, d_pos, d_grad, perm, n_valid, K, d, t, 0, nullptr, trace_t, d_mass_trace ? d_mass_trace + (size_t)(t - 1) * K * d : nullptr, x->stream);
    if (launch_meads_step(a, b, K, key_mode, n_iter, t, x->stream)) return too_large(x, "GHMC");
    if (trace_t) hipLaunchKernelGGL(meads_accmean_kernel, dim3(1), dim3(256), 0, x->stream, b.acc, perm, n_valid, K, p.m, trace_t);
  }
  launch_meads_stats(b, d_pos, d_grad, nullptr, n_valid, 1, d, n_iter + 1, 1, d_inverse_mass_out, nullptr, nullptr, x->stream);
  LAUNCHCHK();
  x->ctr[CTR_MALA] += (int64_t)B * n_iter;      // (steps only, as mfm_hmc_run)
  if (h_result) {                                // the call's only read-back, after everything is enqueued: eps, alpha, delta
    HIPCHK(hipMemcpyAsync(h_result, b.result, 3 * sizeof(double), hipMemcpyDeviceToHost, x->stream));
    HIPCHK(hipStreamSynchronize(x->stream));
  }
  return MFM_OK;
}

// ChEES-HMC warmup (chees.hip): n_iter iterations of four launches each, enqueued back to back; the host reads nothing until the end
static size_t chees_align(size_t n) { return (n + 255) & ~(size_t)255; }
extern "C" int mfm_chees_warmup(mfm_ctx* x, int key_mode, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, double step0, double traj0,
                                int32_t n_iter, int32_t n_valid, double target_accept, double learning_rate, int32_t max_leapfrog, double decay,
                                double div_thr, float* d_pos, double* d_logp, float* d_grad, double* h_result, double* d_trace, float* d_prop,
                                double* d_vel, double* d_alpha) { use_ctx(x);
  NEED_TARGET();
  CHECKED(check_state(d_pos, d_logp, d_grad, step0));
  CHECKED(check_run_keys(key_mode, d_keys, n_iter));
  CHECKED(hmc_refuse_cox(x));
  const int B = x->cfg.n_chain_local, d = x->cfg.dim;
  if (x->cfg.n_chain_total != B)
    return fail(MFM_EUNSUPPORTED, "the ChEES warmup serves one rank (n_chain_total %d != n_chain_local %d): the chains' means would need an all-reduce", x->cfg.n_chain_total, B);
  if (n_valid < 2 || n_valid > B) return fail(MFM_EINVAL, "n_valid must be in [2, n_chain_local = %d] (got %d)", B, n_valid);
  if (!(traj0 > 0)) return fail(MFM_EINVAL, "trajectory_length must be positive (got %g)", traj0);
  if (!(learning_rate > 0)) return fail(MFM_EINVAL, "learning_rate must be positive (got %g)", learning_rate);
  if (!(decay >= 0 && decay < 1)) return fail(MFM_EINVAL, "decay must lie in [0, 1) (got %g)", decay);
  if (max_leapfrog < 1 || max_leapfrog > 100000) return fail(MFM_EINVAL, "max_leapfrog must be in [1, 100000] (got %d)", max_leapfrog);
  if (!(target_accept > 0 && target_accept < 1)) return fail(MFM_EINVAL, "target_accept must lie strictly inside (0, 1) (got %g)", target_accept);
  if (!(div_thr > 0)) return fail(MFM_EINVAL, "divergence_threshold must be positive (got %g)", div_thr);
  if ((d + 63) / 64 > 32) return too_large(x, "HMC");
  // workspace: CheesState | mean [2][d] | g [B] | alpha [B] | vel [B][d] | x0 [B][d] | prop [B][d] | div [B]
  const size_t bd = (size_t)B * d;
  const size_t o_mean = chees_align(sizeof(CheesState)), o_g = o_mean + chees_align(16 * (size_t)d), o_alpha = o_g + chees_align(8 * (size_t)B),
               o_vel = o_alpha + chees_align(8 * (size_t)B), o_x0 = o_vel + chees_align(8 * bd), o_prop = o_x0 + chees_align(4 * bd),
               o_div = o_prop + chees_align(4 * bd), need = o_div + chees_align((size_t)B);
  if (x->chees_ws_cap < need) {
    if (x->chees_ws) { HIPCHK(hipStreamSynchronize(x->stream)); (void)hipFree(x->chees_ws); x->chees_ws = nullptr; x->chees_ws_cap = 0; }
    HIPCHK(hipMalloc(&x->chees_ws, need));
    x->chees_ws_cap = need;
  }
  char* ws = (char*)x->chees_ws;
  CheesBufs c;
  c.st = (CheesState*)ws; c.mean = (double*)(ws + o_mean); c.g = (double*)(ws + o_g);
  c.alpha = d_alpha ? d_alpha : (double*)(ws + o_alpha); c.vel = d_vel ? d_vel : (double*)(ws + o_vel);
  c.x0 = (float*)(ws + o_x0); c.prop = d_prop ? d_prop : (float*)(ws + o_prop); c.div = (uint8_t*)(ws + o_div);
  c.trace = d_trace;
  const CheesConst k{n_iter, n_valid, max_leapfrog, target_accept, learning_rate, decay, div_thr};
  const HmcArgs a = hmc_args(x, k0, k1, key_mode == 1 ? d_keys : nullptr, beta, step0, 0, d_pos, d_logp, d_grad, nullptr, nullptr);
  ProfScope ps_(x, PROF_MALA);
  hipLaunchKernelGGL(chees_begin_kernel, dim3(1), dim3(64), 0, x->stream, c.st, step0, traj0, max_leapfrog);
  for (int t = 0; t < n_iter; ++t)
    if (launch_chees_iteration(a, c, k, key_mode, x->stream)) return too_large(x, "HMC");
  LAUNCHCHK();
  x->ctr[CTR_MALA] += (int64_t)B * n_iter;      // (steps only, as mfm_hmc_run)
  if (h_result) {                                // the call's only read-back, after everything is enqueued
    HIPCHK(hipMemcpyAsync(h_result, c.st->result, 4 * sizeof(double), hipMemcpyDeviceToHost, x->stream));
    HIPCHK(hipStreamSynchronize(x->stream));
  }
  return MFM_OK;
}

// Parallel tempering (pt.hip).  The shared checks of the two entry points, in the order the header states; a rejected call touches nothing.
static int pt_check(mfm_ctx* x, const double* h_betas, const double* h_step_sizes, int32_t n_temps, int32_t n_ladders) {
  CHECKED(hmc_refuse_cox(x));
  if (!x->h_inv_mass.empty()) return fail(MFM_EUNSUPPORTED, "parallel tempering runs at unit mass: remove the installed inverse mass (mfm_hmc_set_inverse_mass with n = 0)");
  const int B = x->cfg.n_chain_local;
  if (x->cfg.n_chain_total != B)
    return fail(MFM_EUNSUPPORTED, "parallel tempering serves one rank (n_chain_total %d != n_chain_local %d): a ladder's slots would lie on several ranks", x->cfg.n_chain_total, B);
  if (n_temps < 2 || n_temps > PT_MAX_TEMPS) return fail(MFM_EINVAL, "n_temps must be in [2, %d] (got %d)", PT_MAX_TEMPS, n_temps);
  if (n_ladders < 1) return fail(MFM_EINVAL, "n_ladders must be at least 1 (got %d)", n_ladders);
  if ((int64_t)n_temps * n_ladders > B) return fail(MFM_EINVAL, "n_temps * n_ladders (%d * %d) must not exceed n_chain_local = %d", n_temps, n_ladders, B);
  if (!h_betas) return fail(MFM_EINVAL, "h_betas must not be null (n_temps host values)");
  for (int k = 0; k < n_temps; ++k)
    if (!(std::isfinite(h_betas[k]) && h_betas[k] > 0)) return fail(MFM_EINVAL, "betas[%d] = %g: every beta must be finite and positive", k, h_betas[k]);
  if (h_step_sizes)
    for (int k = 0; k < n_temps; ++k)
      if (!(std::isfinite(h_step_sizes[k]) && h_step_sizes[k] > 0)) return fail(MFM_EINVAL, "step_sizes[%d] = %g: every step_size must be finite and positive", k, h_step_sizes[k]);
  if ((x->cfg.dim + 63) / 64 > 32) return too_large(x, "parallel tempering");
  return MFM_OK;
}
// the ladder to device memory, stream-ordered behind the launches that still read the previous one (by value: no host buffer outlives the call)
static int pt_upload(mfm_ctx* x, const double* h_betas, const double* h_step_sizes, int n_temps) {
  if (!x->pt_ws) HIPCHK(hipMalloc(&x->pt_ws, 2 * PT_MAX_TEMPS * sizeof(double)));
  PtVec b, e; memset(&b, 0, sizeof b); memset(&e, 0, sizeof e);
  for (int k = 0; k < n_temps; ++k) { b.v[k] = h_betas[k]; e.v[k] = h_step_sizes ? h_step_sizes[k] : 0.0; }
  hipLaunchKernelGGL(pt_ladder_kernel, dim3(1), dim3(PT_MAX_TEMPS), 0, x->stream, b, e, n_temps, x->pt_ws);
  return MFM_OK;
}
static int pt_sweep(mfm_ctx* x, Key2 key, int K, int R, int parity, float* d_pos, double* d_logp, float* d_grad, int32_t* d_replica,
                    int32_t* d_swap_acc, double* d_swap_prob) {
  const int pairs = (K - parity) / 2;
  MalaArgs a = mala_args(x, 1.0);
  a.B = pairs * R;
  const PtSwap s{x->pt_ws, K, parity, pairs, key, (uint32_t)x->cfg.n_chain_total, (uint32_t)x->cfg.chain_offset, d_pos, d_logp, d_grad, d_replica, d_swap_acc, d_swap_prob};
  return launch_pt_exchange(a, s, x->stream);
}

extern "C" int mfm_pt_exchange(mfm_ctx* x, uint32_t k0, uint32_t k1, const double* h_betas, int32_t n_temps, int32_t n_ladders, int32_t parity,
                               float* d_pos, double* d_logp, float* d_grad, int32_t* d_replica, int32_t* d_swap_acc, double* d_swap_prob) { use_ctx(x);
  NEED_TARGET();
  if (!d_pos || !d_logp || !d_grad) return fail(MFM_EINVAL, "null device pointer");
  CHECKED(pt_check(x, h_betas, nullptr, n_temps, n_ladders));
  if (parity != 0 && parity != 1) return fail(MFM_EINVAL, "parity must be 0 or 1 (got %d)", parity);
  CHECKED(pt_upload(x, h_betas, nullptr, n_temps));
  ProfScope ps_(x, PROF_MALA);
  if (pt_sweep(x, Key2{k0, k1}, n_temps, n_ladders, parity, d_pos, d_logp, d_grad, d_replica, d_swap_acc, d_swap_prob)) return too_large(x, "parallel tempering");
  LAUNCHCHK();
  return MFM_OK;
}

extern "C" int mfm_pt_run(mfm_ctx* x, int kernel, uint32_t k0, uint32_t k1, const double* h_betas, const double* h_step_sizes, int32_t n_temps,
                          int32_t n_ladders, int32_t num_steps, int textbook, int32_t n_local, int32_t n_rounds, int exchange, int32_t thin,
                          float* d_pos, double* d_logp, float* d_grad, int32_t* d_n_acc, double* d_acc_sum, int32_t* d_replica,
                          int32_t* d_swap_acc, double* d_swap_prob, float* d_traj_pos, double* d_traj_logp) { use_ctx(x);
  NEED_TARGET();
  if (!d_pos || !d_logp || !d_grad) return fail(MFM_EINVAL, "null device pointer");
  if (kernel != 0 && kernel != 1) return fail(MFM_EINVAL, "kernel must be 0 (MALA) or 1 (HMC) (got %d)", kernel);
  if (kernel == 1) CHECKED(check_num_steps(num_steps));
  if (!h_step_sizes) return fail(MFM_EINVAL, "h_step_sizes must not be null (n_temps host values)");
  CHECKED(pt_check(x, h_betas, h_step_sizes, n_temps, n_ladders));
  if (n_local < 1) return fail(MFM_EINVAL, "n_local must be at least 1 (got %d)", n_local);
  if (n_rounds < 1) return fail(MFM_EINVAL, "n_rounds must be at least 1 (got %d)", n_rounds);
  if (exchange != 0 && exchange != 1) return fail(MFM_EINVAL, "exchange must be 0 (none) or 1 (even-odd) (got %d)", exchange);
  CHECKED(check_thin(thin, n_rounds, d_traj_pos, d_traj_logp));
  const int K = n_temps, R = n_ladders, d = x->cfg.dim;
  const int BK = K * R;
  CHECKED(pt_upload(x, h_betas, h_step_sizes, K));
  if (d_n_acc) HIPCHK(hipMemsetAsync(d_n_acc, 0, (size_t)BK * sizeof(int32_t), x->stream));
  if (d_acc_sum) HIPCHK(hipMemsetAsync(d_acc_sum, 0, (size_t)BK * sizeof(double), x->stream));
  if (d_swap_acc) HIPCHK(hipMemsetAsync(d_swap_acc, 0, (size_t)R * (K - 1) * sizeof(int32_t), x->stream));
  if (d_swap_prob) HIPCHK(hipMemsetAsync(d_swap_prob, 0, (size_t)R * (K - 1) * sizeof(double), x->stream));
  const Key2 k_move = split_at(Key2{k0, k1}, 2, 0), k_swap = split_at(Key2{k0, k1}, 2, 1);
  const PtLocal p{x->pt_ws, x->pt_ws + PT_MAX_TEMPS, K, d_n_acc, d_acc_sum};
  ProfScope ps_(x, PROF_MALA);
  for (int t = 0; t < n_rounds; ++t) {
    const Key2 km = split_at(k_move, (uint32_t)n_rounds, (uint32_t)t);
    int rc;
    if (kernel == 1) {
      HmcRunArgs r; memset(&r, 0, sizeof r);
      r.h = hmc_args(x, km.k0, km.k1, nullptr, 1.0, 1.0, num_steps, d_pos, d_logp, d_grad, nullptr, nullptr);
      r.h.B = BK; r.h.minv = nullptr;
      r.t = RunTail{0, n_local, 0, nullptr, nullptr, nullptr, nullptr};
      rc = launch_pt_hmc_run(r, p, x->stream);
    } else {
      MalaRunArgs r; memset(&r, 0, sizeof r);
      r.m = mala_run_args(x, 0, km.k0, km.k1, nullptr, 1.0, 1.0, textbook, d_pos, d_logp, d_grad);
      r.m.B = BK;
      r.t = RunTail{0, n_local, 0, nullptr, nullptr, nullptr, nullptr};
      rc = launch_pt_mala_run(r, p, x->stream);
    }
    if (rc) return too_large(x, "parallel tempering");
    if (exchange && pt_sweep(x, split_at(k_swap, (uint32_t)n_rounds, (uint32_t)t), K, R, t & 1, d_pos, d_logp, d_grad, d_replica, d_swap_acc, d_swap_prob))
      return too_large(x, "parallel tempering");
    if (thin > 0 && (t + 1) % thin == 0) {
      const size_t snap = (size_t)((t + 1) / thin - 1);
      hipLaunchKernelGGL(pt_traj_kernel, dim3(R), dim3(256), 0, x->stream, d_pos, d_logp, K, R, d,
                         d_traj_pos ? d_traj_pos + snap * (size_t)R * d : nullptr, d_traj_logp ? d_traj_logp + snap * (size_t)R : nullptr);
    }
    LAUNCHCHK();
  }
  x->ctr[CTR_MALA] += (int64_t)BK * n_local * n_rounds;      // (steps only, as mfm_hmc_run)
  return MFM_OK;
}

// The No-U-turn sampler (nuts.hip).  Checks in mfm_hmc_run's order, then the tree's own: a rejected call touches nothing.
static int nuts_check_depth(int32_t max_tree_depth) {
  if (max_tree_depth < 1 || max_tree_depth > NUTS_MAX_DEPTH) return fail(MFM_EINVAL, "max_tree_depth must be in [1, %d] (got %d)", NUTS_MAX_DEPTH, max_tree_depth);
  return MFM_OK;
}
// the chains per workgroup of a launch at (dim, max_tree_depth): nuts_args' and mfm_nuts_launch_plan's
static int nuts_geometry(int d, int32_t max_tree_depth, int& waves) {
  if (d > NUTS_MAX_DIM) return fail(MFM_EUNSUPPORTED, "the NUTS step serves dim <= %d (got %d): the larger instances need the tree's checkpoints outside LDS", NUTS_MAX_DIM, d);
  waves = nuts_waves(d, max_tree_depth);
  if (waves < 1) return fail(MFM_EINVAL, "max_tree_depth %d needs more LDS than a CU has at dim %d: the largest depth that fits is %d", max_tree_depth, d, nuts_depth_that_fits(d));
  return MFM_OK;
}
static int nuts_args(mfm_ctx* x, NutsArgs& n, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, double step, int32_t max_tree_depth,
                     double div_thr, float* d_pos, double* d_logp, float* d_grad, int32_t* d_depth, int32_t* d_nleap, uint8_t* d_turn, uint8_t* d_div,
                     double* d_rate, double* d_energy) {
  CHECKED(nuts_check_depth(max_tree_depth));
  if (!(div_thr > 0)) return fail(MFM_EINVAL, "divergence_threshold must be positive (got %g)", div_thr);
  if (x->net.T.kind == MFM_TARGET_LGCP) return fail(MFM_EUNSUPPORTED, "the NUTS step serves the phi-four and mixture targets (the Cox process needs the K^-1 GEMM tile)");
  const int d = x->cfg.dim;
  int waves = 0;
  CHECKED(nuts_geometry(d, max_tree_depth, waves));
  memset(&n, 0, sizeof n);
  n.h = hmc_args(x, k0, k1, d_keys, beta, step, 0, d_pos, d_logp, d_grad, nullptr, nullptr);
  n.max_depth = max_tree_depth; n.waves = waves; n.div_thr = div_thr;
  n.depth = d_depth; n.n_leap = d_nleap; n.turning = d_turn; n.divergent = d_div; n.acc_rate = d_rate; n.energy = d_energy;
  return MFM_OK;
}
static int nuts_step_common(mfm_ctx* x, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, double step, int32_t max_tree_depth, double div_thr,
                            float* d_pos, double* d_logp, float* d_grad, int32_t* d_depth, int32_t* d_nleap, uint8_t* d_turn, uint8_t* d_div,
                            double* d_rate, double* d_energy) {
  NEED_TARGET();
  CHECKED(check_state(d_pos, d_logp, d_grad, step));
  NutsArgs n;
  CHECKED(nuts_args(x, n, k0, k1, d_keys, beta, step, max_tree_depth, div_thr, d_pos, d_logp, d_grad, d_depth, d_nleap, d_turn, d_div, d_rate, d_energy));
  ProfScope ps_(x, PROF_MALA);
  if (launch_nuts_step(n, x->stream)) return too_large(x, "NUTS");
  LAUNCHCHK();
  x->ctr[CTR_MALA] += x->cfg.n_chain_local;      // (steps only, as mfm_hmc_step)
  return MFM_OK;
}
extern "C" int mfm_nuts_step(mfm_ctx* x, uint32_t k0, uint32_t k1, double beta, double step, int32_t max_tree_depth, double div_thr, float* d_pos,
                             double* d_logp, float* d_grad, int32_t* d_depth, int32_t* d_nleap, uint8_t* d_turn, uint8_t* d_div, double* d_rate,
                             double* d_energy) { use_ctx(x);
  return nuts_step_common(x, k0, k1, nullptr, beta, step, max_tree_depth, div_thr, d_pos, d_logp, d_grad, d_depth, d_nleap, d_turn, d_div, d_rate, d_energy);
}
extern "C" int mfm_nuts_step_keys(mfm_ctx* x, const uint32_t* d_keys, double beta, double step, int32_t max_tree_depth, double div_thr, float* d_pos,
                                  double* d_logp, float* d_grad, int32_t* d_depth, int32_t* d_nleap, uint8_t* d_turn, uint8_t* d_div, double* d_rate,
                                  double* d_energy) { use_ctx(x);
  if (!d_keys) return fail(MFM_EINVAL, "null key array");
  return nuts_step_common(x, 0, 0, d_keys, beta, step, max_tree_depth, div_thr, d_pos, d_logp, d_grad, d_depth, d_nleap, d_turn, d_div, d_rate, d_energy);
}
extern "C" int mfm_nuts_run(mfm_ctx* x, int key_mode, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, double step, int32_t max_tree_depth,
                            double div_thr, int32_t n_steps, int32_t thin, float* d_pos, double* d_logp, float* d_grad, int64_t* d_tot_leap,
                            double* d_acc_sum, int32_t* d_n_div, int32_t* d_depth_sum, int32_t* d_depth, int32_t* d_nleap, uint8_t* d_turn,
                            uint8_t* d_div, double* d_rate, double* d_energy, float* d_traj_pos, double* d_traj_logp) { use_ctx(x);
  NEED_TARGET();
  CHECKED(check_state(d_pos, d_logp, d_grad, step));
  CHECKED(check_run_keys(key_mode, d_keys, n_steps));
  CHECKED(check_thin(thin, n_steps, d_traj_pos, d_traj_logp));
  NutsRunArgs r; memset(&r, 0, sizeof r);
  CHECKED(nuts_args(x, r.n, k0, k1, key_mode == 1 ? d_keys : nullptr, beta, step, max_tree_depth, div_thr, d_pos, d_logp, d_grad, d_depth, d_nleap,
                    d_turn, d_div, d_rate, d_energy));
  r.t = RunTail{key_mode, n_steps, thin, nullptr, nullptr, d_traj_pos, d_traj_logp};
  r.tot_leap = d_tot_leap; r.tot_acc = d_acc_sum; r.tot_div = d_n_div; r.tot_depth = d_depth_sum;
  ProfScope ps_(x, PROF_MALA);
  if (launch_nuts_run(r, x->stream)) return too_large(x, "NUTS");
  LAUNCHCHK();
  x->ctr[CTR_MALA] += (int64_t)x->cfg.n_chain_local * n_steps;      // (steps only, as mfm_hmc_run)
  return MFM_OK;
}

// Step-size warmup (warmup.hip): n_steps steps in one launch, every chain adapting its own step size by dual averaging (mfm.h)
static int warmup_check(mfm_ctx* x, int key_mode, const uint32_t* d_keys, double step0, int32_t n_steps, double target_accept, const float* d_pos,
                        const double* d_logp, const float* d_grad, const double* d_step_avg) {
  NEED_TARGET();
  CHECKED(check_state(d_pos, d_logp, d_grad, step0));
  CHECKED(check_run_keys(key_mode, d_keys, n_steps));
  if (!(target_accept > 0 && target_accept < 1)) return fail(MFM_EINVAL, "target_accept must lie strictly inside (0, 1) (got %g)", target_accept);
  if (!d_step_avg) return fail(MFM_EINVAL, "d_step_avg must not be null");
  return MFM_OK;
}

// window: mfm_hmc_warmup_window, which always runs the mass instances (the context's vector, or ones) and takes the window's sums
static int hmc_warmup_common(mfm_ctx* x, int key_mode, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, double step0, int32_t num_steps,
                             int32_t n_steps, double target_accept, float* d_pos, double* d_logp, float* d_grad, double* d_step_avg,
                             double* d_step_last, int32_t* d_n_acc, double* d_acc_sum, double* d_step_traj, bool window, double* d_pos_sum,
                             double* d_pos_sumsq) {
  CHECKED(warmup_check(x, key_mode, d_keys, step0, n_steps, target_accept, d_pos, d_logp, d_grad, d_step_avg));
  CHECKED(check_num_steps(num_steps));
  if (window && (!d_pos_sum || !d_pos_sumsq)) return fail(MFM_EINVAL, "d_pos_sum and d_pos_sumsq must not be null");
  CHECKED(hmc_refuse_cox(x));
  if (window && !x->d_inv_mass) CHECKED(inv_mass_upload(x, std::vector<double>((size_t)x->cfg.dim, 1.0)));
  HmcRunArgs r; memset(&r, 0, sizeof r);
  r.h = hmc_args(x, k0, k1, key_mode == 1 ? d_keys : nullptr, beta, step0, num_steps, d_pos, d_logp, d_grad, nullptr, nullptr);
  if (window) r.h.minv = x->d_inv_mass;
  r.t = RunTail{key_mode, n_steps, 0, d_n_acc, d_acc_sum, nullptr, nullptr};      // (a warmup keeps no trajectory)
  const WarmupArgs w{target_accept, d_step_avg, d_step_last, d_step_traj, d_pos_sum, d_pos_sumsq};
  ProfScope ps_(x, PROF_MALA);
  if (launch_hmc_warmup(r, w, x->stream)) return too_large(x, "HMC");
  LAUNCHCHK();
  x->ctr[CTR_MALA] += (int64_t)x->cfg.n_chain_local * n_steps;      // (steps only, as mfm_hmc_run)
  return MFM_OK;
}
extern "C" int mfm_hmc_warmup(mfm_ctx* x, int key_mode, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, double step0, int32_t num_steps,
                              int32_t n_steps, double target_accept, float* d_pos, double* d_logp, float* d_grad, double* d_step_avg,
                              double* d_step_last, int32_t* d_n_acc, double* d_acc_sum, double* d_step_traj) { use_ctx(x);
  return hmc_warmup_common(x, key_mode, k0, k1, d_keys, beta, step0, num_steps, n_steps, target_accept, d_pos, d_logp, d_grad, d_step_avg, d_step_last,
                           d_n_acc, d_acc_sum, d_step_traj, false, nullptr, nullptr);
}
extern "C" int mfm_hmc_warmup_window(mfm_ctx* x, int key_mode, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, double step0,
                                     int32_t num_steps, int32_t n_steps, double target_accept, float* d_pos, double* d_logp, float* d_grad,
                                     double* d_step_avg, double* d_step_last, int32_t* d_n_acc, double* d_acc_sum, double* d_step_traj,
                                     double* d_pos_sum, double* d_pos_sumsq) { use_ctx(x);
  return hmc_warmup_common(x, key_mode, k0, k1, d_keys, beta, step0, num_steps, n_steps, target_accept, d_pos, d_logp, d_grad, d_step_avg, d_step_last,
                           d_n_acc, d_acc_sum, d_step_traj, true, d_pos_sum, d_pos_sumsq);
}

extern "C" int mfm_mala_warmup(mfm_ctx* x, int key_mode, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, double step0, int textbook,
                               int32_t n_steps, double target_accept, float* d_pos, double* d_logp, float* d_grad, double* d_step_avg,
                               double* d_step_last, int32_t* d_n_acc, double* d_acc_sum, double* d_step_traj) { use_ctx(x);
  CHECKED(warmup_check(x, key_mode, d_keys, step0, n_steps, target_accept, d_pos, d_logp, d_grad, d_step_avg));
  if (x->net.T.kind == MFM_TARGET_LGCP)
    return fail(MFM_EUNSUPPORTED, "the step-size warmup serves the phi-four and mixture targets (the Cox process's run is a sequence of tile launches with a by-value step size)");
  if (!textbook)
    return fail(MFM_EINVAL, "the step-size warmup needs textbook = 1 (the as-written rule accepts with min(1, 1 / alpha): its acceptance does not fall as the step grows)");
  const int B = x->cfg.n_chain_local, d = x->cfg.dim;
  MalaRunArgs r; memset(&r, 0, sizeof r);
  r.m = mala_run_args(x, key_mode, k0, k1, d_keys, beta, step0, textbook, d_pos, d_logp, d_grad);
  r.t = RunTail{key_mode, n_steps, 0, d_n_acc, d_acc_sum, nullptr, nullptr};      // (a warmup keeps no trajectory)
  const WarmupArgs w{target_accept, d_step_avg, d_step_last, d_step_traj, nullptr, nullptr};
  ProfScope ps_(x, PROF_MALA);
  if (launch_mala_warmup(r, w, x->stream)) return too_large(x, "MALA");
  LAUNCHCHK();
  // state in and out once, as mfm_mala_run; the step sizes that were kept
  x->ctr[CTR_MALA] += (int64_t)B * n_steps;
  x->ctr[CTR_MALA_BYTES] += (int64_t)B * 4 * (4 * d + 4) + (int64_t)B * 8 * (1 + (d_step_last ? 1 : 0) + (d_step_traj ? n_steps : 0));
  return MFM_OK;
}

// ---- HMC for the Cox process on the 16-chain GEMM tile (lgcp_hmc.hip) ----
// The entry points mirror mfm_hmc_step / _step_keys / _run / _warmup argument for argument and make their checks in their order; then
// the refusals of their own below.  A rejected call touches nothing.
static int check_cox_hmc(mfm_ctx* x) {
  if (x->net.T.kind != MFM_TARGET_LGCP)
    return fail(MFM_EUNSUPPORTED, "mfm_cox_hmc_* serves the Cox process on the K^-1 GEMM tile: use mfm_hmc_* (mfm_hmc_step, mfm_hmc_run, mfm_hmc_warmup) for this target");
  if (!x->h_inv_mass.empty())
    return fail(MFM_EUNSUPPORTED, "the Cox process's HMC runs at unit mass: remove the installed inverse mass (mfm_hmc_set_inverse_mass with n = 0)");
  if (x->cfg.n_chain_local % 16) return fail(MFM_EINVAL, "n_chain_local (%d) must be a multiple of 16 (one tile of 16 chains per workgroup)", x->cfg.n_chain_local);
  int tpw; size_t sm;
  cox_hmc_plan(x->net.dp, &tpw, &sm);
  if (!tpw || sm > 160 * 1024) return too_large(x, "Cox process HMC");
  return MFM_OK;
}
static CoxHmcArgs cox_hmc_args(mfm_ctx* x, int run, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, double step, int num_steps,
                               float* d_pos, double* d_logp, float* d_grad, float* d_acc, uint8_t* d_isacc) {
  CoxHmcArgs a; memset(&a, 0, sizeof a);
  a.T = x->net.T; a.dp = x->net.dp; a.run = run; a.key = Key2{k0, k1}; a.keys = d_keys;
  a.n_total = x->cfg.n_chain_total; a.chain_offset = x->cfg.chain_offset; a.B = x->cfg.n_chain_local; a.num_steps = num_steps;
  a.beta = beta; a.eps = step;
  a.pos = d_pos; a.logp = d_logp; a.grad = d_grad; a.acc_prob = d_acc; a.accepted = d_isacc;
  a.t = RunTail{0, 1, 0, nullptr, nullptr, nullptr, nullptr};
  return a;
}
static int cox_hmc_launch(mfm_ctx* x, const CoxHmcArgs& a, bool warm) {
  ProfScope ps_(x, PROF_MALA);
  if (launch_cox_hmc(a, warm, x->stream)) return too_large(x, "Cox process HMC");
  LAUNCHCHK();
  x->ctr[CTR_MALA] += (int64_t)x->cfg.n_chain_local * a.t.n_steps;      // (steps only, as mfm_hmc_run)
  return MFM_OK;
}
static int cox_hmc_step_common(mfm_ctx* x, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, double step, int num_steps, float* d_pos,
                               double* d_logp, float* d_grad, float* d_acc, uint8_t* d_isacc) {
  NEED_TARGET();
  CHECKED(check_state(d_pos, d_logp, d_grad, step));
  CHECKED(check_num_steps(num_steps));
  CHECKED(check_cox_hmc(x));
  return cox_hmc_launch(x, cox_hmc_args(x, 0, k0, k1, d_keys, beta, step, num_steps, d_pos, d_logp, d_grad, d_acc, d_isacc), false);
}
extern "C" int mfm_cox_hmc_step(mfm_ctx* x, uint32_t k0, uint32_t k1, double beta, double step, int num_steps, float* d_pos, double* d_logp,
                                float* d_grad, float* d_acc, uint8_t* d_isacc) { use_ctx(x);
  return cox_hmc_step_common(x, k0, k1, nullptr, beta, step, num_steps, d_pos, d_logp, d_grad, d_acc, d_isacc);
}
extern "C" int mfm_cox_hmc_step_keys(mfm_ctx* x, const uint32_t* d_keys, double beta, double step, int num_steps, float* d_pos, double* d_logp,
                                     float* d_grad, float* d_acc, uint8_t* d_isacc) { use_ctx(x);
  if (!d_keys) return fail(MFM_EINVAL, "null key array");
  return cox_hmc_step_common(x, 0, 0, d_keys, beta, step, num_steps, d_pos, d_logp, d_grad, d_acc, d_isacc);
}
// n_steps HMC steps in ONE launch: the tile's x, p and g stay in registers, K^-1 is streamed again once per leapfrog step
extern "C" int mfm_cox_hmc_run(mfm_ctx* x, int key_mode, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, double step, int32_t num_steps,
                               int32_t n_steps, int32_t thin, float* d_pos, double* d_logp, float* d_grad, int32_t* d_n_acc, double* d_acc_sum,
                               float* d_acc, uint8_t* d_isacc, float* d_traj_pos, double* d_traj_logp) { use_ctx(x);
  NEED_TARGET();
  CHECKED(check_state(d_pos, d_logp, d_grad, step));
  CHECKED(check_num_steps(num_steps));
  CHECKED(check_run_keys(key_mode, d_keys, n_steps));
  CHECKED(check_thin(thin, n_steps, d_traj_pos, d_traj_logp));
  CHECKED(check_cox_hmc(x));
  CoxHmcArgs a = cox_hmc_args(x, 1, k0, k1, key_mode == 1 ? d_keys : nullptr, beta, step, num_steps, d_pos, d_logp, d_grad, d_acc, d_isacc);
  a.t = RunTail{key_mode, n_steps, thin, d_n_acc, d_acc_sum, d_traj_pos, d_traj_logp};
  return cox_hmc_launch(x, a, false);
}
// the run with a per-row step size, adapted by dual averaging on the row's owner lanes (mfm_hmc_warmup's recursion and outputs)
extern "C" int mfm_cox_hmc_warmup(mfm_ctx* x, int key_mode, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, double step0, int32_t num_steps,
                                  int32_t n_steps, double target_accept, float* d_pos, double* d_logp, float* d_grad, double* d_step_avg,
                                  double* d_step_last, int32_t* d_n_acc, double* d_acc_sum, double* d_step_traj) { use_ctx(x);
  CHECKED(warmup_check(x, key_mode, d_keys, step0, n_steps, target_accept, d_pos, d_logp, d_grad, d_step_avg));
  CHECKED(check_num_steps(num_steps));
  CHECKED(check_cox_hmc(x));
  CoxHmcArgs a = cox_hmc_args(x, 1, k0, k1, key_mode == 1 ? d_keys : nullptr, beta, step0, num_steps, d_pos, d_logp, d_grad, nullptr, nullptr);
  a.t = RunTail{key_mode, n_steps, 0, d_n_acc, d_acc_sum, nullptr, nullptr};      // (a warmup keeps no trajectory)
  a.w = WarmupArgs{target_accept, d_step_avg, d_step_last, d_step_traj, nullptr, nullptr};
  return cox_hmc_launch(x, a, true);
}
extern "C" int mfm_cox_hmc_launch_plan(int32_t dim, int32_t* h_tpw, int32_t* h_lds_bytes) {
  if (!h_tpw || !h_lds_bytes) return fail(MFM_EINVAL, "mfm_cox_hmc_launch_plan: null output pointer");
  if (dim < 1) return fail(MFM_EINVAL, "mfm_cox_hmc_launch_plan: dim must be positive (got %d)", dim);
  int tpw; size_t sm;
  cox_hmc_plan((dim + 15) / 16 * 16, &tpw, &sm);
  if (!tpw || sm > 160 * 1024) return fail(MFM_ETOOLARGE, "dim %d too large for the Cox process HMC kernel", dim);
  *h_tpw = tpw; *h_lds_bytes = (int32_t)sm;
  return MFM_OK;
}

// The NUTS warmup (nuts_warmup.hip.h): the warmup's checks, then the tree's own (nuts_args); a rejected call touches nothing.
// window: mfm_nuts_warmup_window, which always runs the mass instances (the context's vector, or ones) and takes the window's sums
static int nuts_warmup_common(mfm_ctx* x, int key_mode, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, double step0,
                              int32_t max_tree_depth, double div_thr, int32_t n_steps, double target_accept, float* d_pos, double* d_logp,
                              float* d_grad, double* d_step_avg, double* d_step_last, double* d_acc_sum, double* d_step_traj, int64_t* d_tot_leap,
                              int32_t* d_n_div, int32_t* d_depth_sum, bool window, double* d_pos_sum, double* d_pos_sumsq) {
  CHECKED(warmup_check(x, key_mode, d_keys, step0, n_steps, target_accept, d_pos, d_logp, d_grad, d_step_avg));
  if (window && (!d_pos_sum || !d_pos_sumsq)) return fail(MFM_EINVAL, "d_pos_sum and d_pos_sumsq must not be null");
  NutsRunArgs r; memset(&r, 0, sizeof r);
  CHECKED(nuts_args(x, r.n, k0, k1, key_mode == 1 ? d_keys : nullptr, beta, step0, max_tree_depth, div_thr, d_pos, d_logp, d_grad, nullptr, nullptr,
                    nullptr, nullptr, nullptr, nullptr));
  if (window && !x->d_inv_mass) CHECKED(inv_mass_upload(x, std::vector<double>((size_t)x->cfg.dim, 1.0)));
  if (window) r.n.h.minv = x->d_inv_mass;
  r.t = RunTail{key_mode, n_steps, 0, nullptr, d_acc_sum, nullptr, nullptr};      // (a warmup keeps no trajectory; a transition has no accept / reject)
  r.tot_leap = d_tot_leap; r.tot_div = d_n_div; r.tot_depth = d_depth_sum;
  const WarmupArgs w{target_accept, d_step_avg, d_step_last, d_step_traj, window ? d_pos_sum : nullptr, window ? d_pos_sumsq : nullptr};
  ProfScope ps_(x, PROF_MALA);
  if (launch_nuts_warmup(r, w, x->stream)) return too_large(x, "NUTS");
  LAUNCHCHK();
  x->ctr[CTR_MALA] += (int64_t)x->cfg.n_chain_local * n_steps;      // (steps only, as mfm_nuts_run)
  return MFM_OK;
}
extern "C" int mfm_nuts_warmup(mfm_ctx* x, int key_mode, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, double step0,
                               int32_t max_tree_depth, double div_thr, int32_t n_steps, double target_accept, float* d_pos, double* d_logp,
                               float* d_grad, double* d_step_avg, double* d_step_last, double* d_acc_sum, double* d_step_traj,
                               int64_t* d_tot_leap, int32_t* d_n_div, int32_t* d_depth_sum) { use_ctx(x);
  return nuts_warmup_common(x, key_mode, k0, k1, d_keys, beta, step0, max_tree_depth, div_thr, n_steps, target_accept, d_pos, d_logp, d_grad,
                            d_step_avg, d_step_last, d_acc_sum, d_step_traj, d_tot_leap, d_n_div, d_depth_sum, false, nullptr, nullptr);
}
extern "C" int mfm_nuts_warmup_window(mfm_ctx* x, int key_mode, uint32_t k0, uint32_t k1, const uint32_t* d_keys, double beta, double step0,
                                      int32_t max_tree_depth, double div_thr, int32_t n_steps, double target_accept, float* d_pos,
                                      double* d_logp, float* d_grad, double* d_step_avg, double* d_step_last, double* d_acc_sum,
                                      double* d_step_traj, int64_t* d_tot_leap, int32_t* d_n_div, int32_t* d_depth_sum, double* d_pos_sum,
                                      double* d_pos_sumsq) { use_ctx(x);
  return nuts_warmup_common(x, key_mode, k0, k1, d_keys, beta, step0, max_tree_depth, div_thr, n_steps, target_accept, d_pos, d_logp, d_grad,
                            d_step_avg, d_step_last, d_acc_sum, d_step_traj, d_tot_leap, d_n_div, d_depth_sum, true, d_pos_sum, d_pos_sumsq);
}

extern "C" int mfm_loglik(mfm_ctx* x, const float* d_pos, double* d_out) { use_ctx(x);
  NEED_TARGET();
  if (!d_pos || !d_out) return fail(MFM_EINVAL, "null device pointer");
  MalaArgs a = mala_args(x, 1.0);
  a.pos = const_cast<float*>(d_pos);
  if (launch_loglik(a, d_out, x->stream)) return too_large(x, "loglik");
  LAUNCHCHK();
  return MFM_OK;
}

// slot of the prefetched draws for `key` (consumed in order), or -1; the first consumer after a prefetch makes the
// context's stream wait for the side stream
static int noise_take(mfm_ctx* x, Key2 key, bool step) {
  NoiseWs* w = x->noise;
  if (!w || w->n_valid == 0) return -1;
  int& cur = step ? w->cur_st : w->cur_gn;
  const std::vector<Key2>& ks = step ? w->st : w->gn;
  for (int j = cur; j < w->n_valid; ++j)
    if (ks[j].k0 == key.k0 && ks[j].k1 == key.k1 && !(!step && j == 0 && w->no_mala0)) { cur = j + 1; return j; }      // same stream as the producer: ordered
  return -1;
}

// eval_valid > 0 (forward only): rows >= eval_valid of the launch are padding (no loss); accumulate: add to *d_loss
static int fm_common(mfm_ctx* x, uint32_t k0, uint32_t k1, const float* d_samples, int n, int n_total, int offset, bool train,
                     double* d_loss, float* d_grads = nullptr, int eval_valid = 0, bool accumulate = false) {
  if (!x->has_fourier) return fail(MFM_EINVAL, "mfm_set_fourier has not been called");
  if (n <= 0 || n % 16) return fail(MFM_EUNSUPPORTED, "sample count must be a positive multiple of 16 (got %d)", n);
  if (!x->wide && n / 16 > x->loss_cap) return fail(MFM_ETOOLARGE, "n=%d exceeds max_eval_samples given at mfm_create", n);
  x->ctr[train ? CTR_FM_TRAIN : CTR_FM_EVAL] += n;
  FmArgs a; memset(&a, 0, sizeof a);
  a.net = x->net; a.ws = x->ws;
  const Key2 key{k0, k1};
  if (x->cfg.cond_flow) {                       // exe_flow_matching.py:153
    a.key_time = split_at(key, 4, 0); a.key_ref = split_at(key, 4, 1); a.key_gauss = split_at(key, 4, 2);
  } else {                                      // :141
    a.key_time = split_at(key, 2, 0); a.key_ref = split_at(key, 2, 1);
  }
  a.n_total = n_total; a.chain_offset = offset; a.B = n; a.sigma = x->cfg.sigma; a.cond_flow = x->cfg.cond_flow;
  a.ref_std = x->cfg.ref_std;
  a.n_valid = train && x->cfg.n_chain_valid > 0 ? x->cfg.n_chain_valid : n;      // (padding rows of the chain shard: no loss, no gradient)
  if (!train && eval_valid > 0) a.n_valid = eval_valid;
  a.pos = d_samples; a.acts = x->acts; a.dzs = x->dzs; a.dacts = x->dacts; a.loss_part = x->loss_part;
  if (x->wide) {      // R rows per pass; the loss is accumulated over the passes
    wide::Ctx* w = x->wide;
    for (int r0 = 0; r0 < n; r0 += w->R) {
      wide::FmCall c;
      c.key_time = a.key_time; c.key_ref = a.key_ref; c.key_gauss = a.key_gauss; c.n_total = (uint32_t)n_total; c.chain_offset = (uint32_t)(offset + r0);
      c.sigma = a.sigma; c.cond_flow = a.cond_flow; c.ref_std = a.ref_std; c.pos = d_samples + (size_t)r0 * x->cfg.dim; c.rows = n - r0 < w->R ? n - r0 : w->R;
      c.rows_valid = a.n_valid - r0 < 0 ? 0 : (a.n_valid - r0 < c.rows ? a.n_valid - r0 : c.rows);
      // one rank, one pass: this IS the gradient the optimizer will see, so its finite check rides in the weight-gradient kernel
      const bool inline_check = train && n <= w->R && x->cfg.n_chain_total == x->cfg.n_chain_local;
      c.bad = inline_check ? x->flag : nullptr;
      int rcw;
      { ProfScope ps_(x, train ? PROF_FM : PROF_EVAL); rcw = wide::fm(w, x->net, c, train, train ? d_grads : nullptr, x->stream); }
      if (rcw) return fail(rcw, "wide fm kernels cannot be launched for this configuration");
      LAUNCHCHK();
      ProfScope ps2_(x, PROF_REDUCE);
      launch_reduce_loss(w->loss_part, (c.rows + 3) / 4, d_loss, r0 > 0 || accumulate, x->stream);
      LAUNCHCHK();
      if (inline_check) x->checked_grads = d_grads;
    }
    return MFM_OK;
  }
  if (train && x->fuse_mala.on) a.mala = x->fuse_mala;      // mfm_train_iter: the iteration's MALA step in the same launch
  if (train) { a.flags_clear = x->flag; a.sus_set = x->flag + 5 + x->sus_par; a.sus_clear = x->flag + 5 + (x->sus_par ^ 1); }
  if (train && x->cfg.cond_flow) {
    const int slot = noise_take(x, key, true);
    if (slot >= 0) {
      const size_t B = (size_t)x->cfg.n_chain_local;
      a.pre_x0 = x->noise->fm_x0 + (size_t)slot * B * x->cfg.dim; a.pre_eps = x->noise->fm_eps + (size_t)slot * B * x->cfg.dim;
      a.pre_t = x->noise->fm_t + (size_t)slot * B;
    }
  }
  int rc;
  { ProfScope ps_(x, train ? PROF_FM : PROF_EVAL); rc = launch_fm(a, train, x->stream); }
  if (rc) return fail(rc, "fm kernel cannot be launched for this configuration");
  LAUNCHCHK();
  if (train) return MFM_OK;            // the training path totals the loss partials in its slab-reduction kernel
  ProfScope ps2_(x, PROF_REDUCE);
  launch_reduce_loss(x->loss_part, fm_eval_parts(x->net, n), d_loss, accumulate ? 1 : 0, x->stream);
  LAUNCHCHK();
  return MFM_OK;
}

static AdamArgs adam_args(mfm_ctx* x, const float* grads, int n_slabs) {
  const mfm_config& c = x->cfg;
  AdamArgs a; memset(&a, 0, sizeof a);
  a.net = x->net; a.grads = grads; a.n_slabs = n_slabs;
  a.master = x->master; a.mu = x->mu; a.nu = x->nu; a.Wp = x->Wp; a.WpT = x->WpT; a.bias = x->bias;
  a.st = x->opt; a.flag = x->flag;
  a.lr0 = c.learning_rate; a.learning_iter = c.learning_iter; a.warmup = c.warmup_steps;
  a.b1 = c.adam_b1; a.b2 = c.adam_b2; a.eps = (float)c.adam_eps; a.wd = (float)c.weight_decay; a.clip = (float)c.update_clip;
  a.max_err = 10;
  return a;
}

// one rank, tile family: slab reduction + apply_if_finite + AdamW as ONE launch behind the weight-gradient kernel (optim.hip:
// reduce_adamw_kernel; every workgroup of its grid must be resident at once, hence the bound on the parameter count)
static bool opt_fusable(mfm_ctx* x) {
  // the grid (one parameter per thread) may take at most HALF of the workgroup slots the occupancy query reported at create:
  // margin for other queues' kernels and for a CU mask narrower than the device (headline: 837 of 2048 on a full MI355X; a
  // 32-CU partition holds 256 and falls back to reduce_slabs + adamw)
  const int grid = (x->net.n_params + 255) / 256;
  if (x->wsk_G) return !g_sw.no_fused_opt && !x->wide && !x->comm && x->cfg.n_chain_total == x->cfg.n_chain_local;      // (wgrad_sk.hip: its workgroups DO wait for one another; the residency guard is at mfm_create and needs no bound on the parameter count)
  return !g_sw.no_fused_opt && !x->wide && !x->comm && x->cfg.n_chain_total == x->cfg.n_chain_local && 2 * grid <= x->opt_resident_wgs;
}

static int fm_loss_grad_impl(mfm_ctx* x, uint32_t k0, uint32_t k1, const float* d_pos, double* d_loss, float* d_grads, bool with_optimizer) {
  NEED_TARGET();
  if (!d_pos || !d_loss || !d_grads) return fail(MFM_EINVAL, "null device pointer");
  x->checked_grads = nullptr;
  int rc = fm_common(x, k0, k1, d_pos, x->cfg.n_chain_local, x->cfg.n_chain_total, x->cfg.chain_offset, true, d_loss, d_grads);
  if (rc || x->wide) return rc;
  const int sus_par = x->sus_par; x->sus_par ^= 1;      // (the training kernel just wrote flag[5 + sus_par] and cleared the other word)
  if (x->wsk_G) {
    // stream-K weight gradients; every contributor of a block totals its own slice of it and, with the optimizer, updates it (wgrad_sk.hip)
    WskArgs k; memset(&k, 0, sizeof k);
    k.C = x->wsk_const; k.wg = x->wsk_wg; k.acts = x->acts; k.dzs = x->dzs; k.nbb = x->cfg.n_chain_local / 16; k.G = x->wsk_G;
    k.xcd_remap = g_sw.wsk_xcd ? 1 : 0;
    k.tickets = x->wsk_tickets + x->wsk_par * x->n_jobs; k.tickets_clear = x->wsk_tickets + (x->wsk_par ^ 1) * x->n_jobs; x->wsk_par ^= 1;
    k.out = d_grads;
    k.loss_part = x->loss_part; k.n_part = x->cfg.n_chain_local / 16; k.loss_out = d_loss;
    const bool single1 = x->cfg.n_chain_total == x->cfg.n_chain_local;
    if (with_optimizer) {
      k.fuse = 1;
      k.st = x->opt; k.st_next = x->opt_alt; k.flag = x->flag; k.suspicious = x->flag + 5 + sus_par;
      k.force_exchange = g_sw.force_exchange ? 1 : 0;
    } else {
      k.bad = single1 ? x->flag : nullptr;      // flag[0] was cleared by the training kernel (FmArgs::flags_clear)
    }
    { ProfScope ps_(x, PROF_WGRAD); launch_wgrad_sk(k, x->wsk_G, x->stream); }
    LAUNCHCHK();
    if (with_optimizer) {
      OptState* t = x->opt; x->opt = x->opt_alt; x->opt_alt = t;
      x->ctr[CTR_OPT_STEPS] += 1;
    } else x->checked_grads = single1 ? d_grads : nullptr;
    return MFM_OK;
  }
  WgradArgs w; memset(&w, 0, sizeof w);
  w.net = x->net; w.ws = x->ws; w.acts = x->acts; w.dzs = x->dzs; w.jobs = x->jobs; w.n_jobs = x->n_jobs;
  w.nbb = x->cfg.n_chain_local / 16; w.split = x->split; w.slabs = x->slabs;
  // One rank: this sum is the gradient the optimizer will see, so its finite check rides in the reduction and
  // mfm_adamw_step(d_grads) skips its check kernel.  With more ranks the check has to follow the all-reduce.
  const bool single = x->cfg.n_chain_total == x->cfg.n_chain_local;
  if (with_optimizer) {
    w.flag_partial = x->flag;                  // cleared by the training kernel (FmArgs::flags_clear)
    { ProfScope ps_(x, PROF_WGRAD); launch_wgrad(w, x->stream); }
    LAUNCHCHK();
    const int force = g_sw.force_exchange ? 1 : 0;      // tests: the grid-wide decision path on ordinary gradients
    ProfScope ps2_(x, PROF_ADAM);
    launch_reduce_adamw(adam_args(x, x->slabs, x->split), x->opt_alt, d_grads, x->loss_part, x->cfg.n_chain_local / 16, d_loss, force, x->stream);
    LAUNCHCHK();
    OptState* t = x->opt; x->opt = x->opt_alt; x->opt_alt = t;
    x->ctr[CTR_OPT_STEPS] += 1;
    return MFM_OK;
  }
  w.flag_reset = single ? x->flag : nullptr;
  { ProfScope ps_(x, PROF_WGRAD); launch_wgrad(w, x->stream); }
  LAUNCHCHK();
  ProfScope ps2_(x, PROF_REDUCE);
  launch_reduce_slabs(x->slabs, x->split, x->net.n_params, d_grads, x->loss_part, x->cfg.n_chain_local / 16, d_loss, single ? x->flag : nullptr, x->stream);
  LAUNCHCHK();
  x->checked_grads = single ? d_grads : nullptr;
  return MFM_OK;
}
extern "C" int mfm_fm_loss_grad(mfm_ctx* x, uint32_t k0, uint32_t k1, const float* d_pos, double* d_loss, float* d_grads) { use_ctx(x);
  return fm_loss_grad_impl(x, k0, k1, d_pos, d_loss, d_grads, false);
}

// rows [0, rem) of `src` followed by copies of row rem - 1: the 16-row image of a partial tile (finite padding, never counted)
__global__ void pad_tile_kernel(const float* src, int rem, int d, float* dst) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 16 * d; i += gridDim.x * blockDim.x) {
    const int r = i / d, j = i - r * d;
    dst[i] = src[(size_t)(r < rem ? r : rem - 1) * d + j];
  }
}

extern "C" int mfm_wsk_plan(int n_jobs, int nbb, int cap, int g_override, int32_t h_out[4], int32_t* h_wg) {
  if (!h_out) return fail(MFM_EINVAL, "mfm_wsk_plan: h_out is null");
  if (n_jobs < 1 || nbb < 1 || cap < n_jobs) return fail(MFM_EINVAL, "mfm_wsk_plan: n_jobs=%d nbb=%d cap=%d (all positive, cap >= n_jobs: one workgroup per block must be resident)", n_jobs, nbb, cap);
  if ((long long)n_jobs * nbb > 0x7fffffffLL) return fail(MFM_ETOOLARGE, "mfm_wsk_plan: %d x %d units", n_jobs, nbb);
  int G = 0, q = 0, r = 0;
  wsk_plan(n_jobs, nbb, cap, g_override, G, q, r);
  h_out[0] = G; h_out[1] = q; h_out[2] = r; h_out[3] = wsk_n_slices(n_jobs, nbb, q, r);
  if (h_wg) {
    std::vector<WskWg> wg(G);
    wsk_ranges(n_jobs, nbb, G, q, r, nullptr, wg.data());
    for (int w = 0; w < G; ++w) { h_wg[4 * w] = wg[w].j0; h_wg[4 * w + 1] = wg[w].bb0; h_wg[4 * w + 2] = wg[w].cnt; h_wg[4 * w + 3] = wg[w].n0; }
  }
  return MFM_OK;
}
extern "C" int mfm_nuts_launch_plan(int32_t dim, int32_t max_tree_depth, int32_t* h_waves, int32_t* h_lds_bytes, int32_t* h_workgroups_per_cu) {
  if (!h_waves || !h_lds_bytes || !h_workgroups_per_cu) return fail(MFM_EINVAL, "mfm_nuts_launch_plan: null output pointer");
  if (dim < 1) return fail(MFM_EINVAL, "mfm_nuts_launch_plan: dim must be positive (got %d)", dim);
  CHECKED(nuts_check_depth(max_tree_depth));
  int waves = 0;
  CHECKED(nuts_geometry(dim, max_tree_depth, waves));
  const size_t sm = nuts_smem(dim, max_tree_depth, waves);
  *h_waves = waves; *h_lds_bytes = (int32_t)sm; *h_workgroups_per_cu = (int32_t)(NUTS_LDS_CU / sm);
  return MFM_OK;
}
extern "C" int mfm_wgrad_info(mfm_ctx* x, int32_t h_out[6]) { use_ctx(x);
  if (!x || !h_out) return fail(MFM_EINVAL, "mfm_wgrad_info: null argument");
  const int nbb = x->cfg.n_chain_local / 16;
  if (x->wide) {
    int n_full = 0, n_tail = 0;
    wide::wgrad_grid(x->wide, x->cfg.n_chain_local, n_full, n_tail);
    h_out[0] = 2; h_out[1] = x->wide->n_jobs; h_out[2] = nbb; h_out[3] = n_full / 4 + n_tail; h_out[4] = n_tail; h_out[5] = 0;
  } else if (x->wsk_G) {
    h_out[0] = 1; h_out[1] = x->n_jobs; h_out[2] = nbb; h_out[3] = x->wsk_G; h_out[4] = x->wsk_q; h_out[5] = x->wsk_r;
  } else {
    h_out[0] = 0; h_out[1] = x->n_jobs; h_out[2] = nbb; h_out[3] = x->n_jobs * x->split; h_out[4] = nbb / x->split; h_out[5] = nbb % x->split;
  }
  return MFM_OK;
}
extern "C" int mfm_wide_gemm_plan(int rows, int KB, int NT, int dual, int KBT, unsigned switches, int32_t h_out[4]) {
  if (!h_out) return fail(MFM_EINVAL, "mfm_wide_gemm_plan: h_out is null");
  if (rows < 16 || rows % 16 || KB < 1 || NT < 1) return fail(MFM_EINVAL, "mfm_wide_gemm_plan: rows=%d KB=%d NT=%d (rows a positive multiple of 16, KB and NT positive)", rows, KB, NT);
  if (dual && (KBT < 1 || KBT > KB)) return fail(MFM_EINVAL, "mfm_wide_gemm_plan: KBT=%d outside [1, KB=%d]", KBT, KB);
  if (switches & ~15u) return fail(MFM_EINVAL, "mfm_wide_gemm_plan: unknown switch bits 0x%x", switches);
  const wide::GemmPlan p = wide::gemm_plan(rows, KB, NT, dual != 0, dual ? KBT : 0, switches);
  h_out[0] = p.inst; h_out[1] = p.gx; h_out[2] = p.gy; h_out[3] = p.block;
  return MFM_OK;
}
extern "C" int mfm_wide_gemm_tally(mfm_ctx* x, int64_t* h_out, int reset) { use_ctx(x);
  if (!x || (!h_out && !reset)) return fail(MFM_EINVAL, "mfm_wide_gemm_tally: null argument");
  for (int i = 0; i < MFM_WGEMM_COUNT; ++i) { if (h_out) h_out[i] = x->wgemm_tally[i]; if (reset) x->wgemm_tally[i] = 0; }
  return MFM_OK;
}
extern "C" int mfm_fm_eval_instance(mfm_ctx* x, int n) { use_ctx(x);
  NEED_TARGET();
  if (n <= 0) return fail(MFM_EINVAL, "sample count must be positive (got %d)", n);
  return x->wide ? 0 : fm_eval_instance(x->net, n & ~15);
}

extern "C" int mfm_fm_loss(mfm_ctx* x, uint32_t k0, uint32_t k1, const float* d_samples, int n, int n_total, int offset, double* d_loss) { use_ctx(x);
  NEED_TARGET();
  if (n <= 0) return fail(MFM_EINVAL, "sample count must be positive (got %d)", n);
  if (!d_samples || !d_loss) return fail(MFM_EINVAL, "null device pointer");
  // Any n: the kernels work on 16-row tiles, so the last n % 16 samples go through a 16-row staging tile of the context whose other
  // rows are padding with residual 0 (FmArgs::n_valid).  Every draw is indexed by the sample's GLOBAL index out of n_total, so the
  // two launches see the draws one launch over n rows would (eval_step on num_chain * eval_iter samples for ANY --num_chain,
  // exe_flow_matching.py:370-374, and for any split of them over ranks).
  const int n_main = n & ~15, rem = n - n_main;
  if (n_main) {
    const int rc = fm_common(x, k0, k1, d_samples, n_main, n_total, offset, false, d_loss);
    if (rc || !rem) return rc;
  }
  hipLaunchKernelGGL(pad_tile_kernel, dim3(16), dim3(256), 0, x->stream, d_samples + (size_t)n_main * x->cfg.dim, rem, x->cfg.dim, x->eval_pad);
  LAUNCHCHK();
  const int rc = fm_common(x, k0, k1, x->eval_pad, 16, n_total, offset + n_main, false, d_loss, nullptr, rem, n_main > 0);
  x->ctr[CTR_FM_EVAL] -= 16 - rem;      // (fm_common counted the staging tile's 16 rows)
  return rc;
}

// ---- RCCL, resolved at run time ------------------------------------------------------------------------------------------
// The library carries no link-time dependency on RCCL (a host that never calls mfm_comm_* needs none): the first call looks for
// a copy the process has already loaded (PyTorch ships one under the same soname), then for the system's.
struct RcclApi {
  ncclResult_t (*GetUniqueId)(ncclUniqueId*);
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int);
  ncclResult_t (*CommDestroy)(ncclComm_t);
  ncclResult_t (*CommCount)(const ncclComm_t, int*);
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t);
  const char* (*GetErrorString)(ncclResult_t);
};
static const char* g_rccl_why = "";
static RcclApi* rccl_api() {
  // resolved once, whichever thread comes first (std::call_once); the reason of a failed load is kept for the error text
  static RcclApi api; static bool ok = false; static std::once_flag once; static char why[256] = "";
  std::call_once(once, [] {
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) { const char* e = dlerror(); snprintf(why, sizeof why, "%s", e ? e : "dlopen failed"); return; }
    api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    api.CommInitRank = (decltype(api.CommInitRank))dlsym(h, "ncclCommInitRank");
    api.CommDestroy = (decltype(api.CommDestroy))dlsym(h, "ncclCommDestroy");
    api.CommCount = (decltype(api.CommCount))dlsym(h, "ncclCommCount");
    api.AllReduce = (decltype(api.AllReduce))dlsym(h, "ncclAllReduce");
    api.GetErrorString = (decltype(api.GetErrorString))dlsym(h, "ncclGetErrorString");
    ok = api.GetUniqueId && api.CommInitRank && api.CommDestroy && api.CommCount && api.AllReduce && api.GetErrorString;
    if (!ok) snprintf(why, sizeof why, "librccl.so.1 lacks an expected symbol");
  });
  g_rccl_why = why;
  return ok ? &api : nullptr;
}
#define RCCLCHK(call) do { const ncclResult_t r_ = (call); if (r_ != ncclSuccess) return fail(MFM_EHIP, "RCCL: %s", R->GetErrorString(r_)); } while (0)

extern "C" int mfm_comm_unique_id(uint8_t out[MFM_COMM_ID_BYTES]) {
  static_assert(sizeof(ncclUniqueId) == MFM_COMM_ID_BYTES, "ncclUniqueId size");
  RcclApi* R = rccl_api();
  if (!R) return fail(MFM_EUNSUPPORTED, "librccl.so.1 cannot be loaded: %s", g_rccl_why);
  if (!out) return fail(MFM_EINVAL, "null argument");
  ncclUniqueId id;
  RCCLCHK(R->GetUniqueId(&id));
  memcpy(out, &id, sizeof id);
  return MFM_OK;
}

extern "C" int mfm_comm_destroy(mfm_ctx* x) { use_ctx(x);
  if (!x) return fail(MFM_EINVAL, "null ctx");
  // keyed on what exists, not on the communicator: a mfm_comm_init that failed half-way leaves a stream / events behind
  if (x->comm_stream) (void)hipStreamSynchronize(x->comm_stream);
  if (x->comm) { RcclApi* R = rccl_api(); if (R) (void)R->CommDestroy(x->comm); }
  if (x->ev_grads) (void)hipEventDestroy(x->ev_grads);
  if (x->ev_comm) (void)hipEventDestroy(x->ev_comm);
  if (x->comm_stream) (void)hipStreamDestroy(x->comm_stream);
  x->comm = nullptr; x->comm_stream = nullptr; x->ev_grads = x->ev_comm = nullptr; x->comm_pending = nullptr; x->comm_nranks = 0;
  return MFM_OK;
}

extern "C" int mfm_comm_init(mfm_ctx* x, int nranks, int rank, const uint8_t id_bytes[MFM_COMM_ID_BYTES]) { use_ctx(x);
  if (!x || !id_bytes) return fail(MFM_EINVAL, "null argument");
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail(MFM_EINVAL, "bad rank %d of %d", rank, nranks);
  if (x->comm) return fail(MFM_EINVAL, "the context already owns a communicator (mfm_comm_destroy first)");
  if ((long long)x->cfg.n_chain_local * nranks != (long long)x->cfg.n_chain_total)
    return fail(MFM_EINVAL, "n_chain_total (%d) is not nranks (%d) x n_chain_local (%d)", x->cfg.n_chain_total, nranks, x->cfg.n_chain_local);
  RcclApi* R = rccl_api();
  if (!R) return fail(MFM_EUNSUPPORTED, "librccl.so.1 cannot be loaded: %s", g_rccl_why);
  ncclUniqueId id; memcpy(&id, id_bytes, sizeof id);
  int rc = MFM_OK;
  if (hipStreamCreateWithFlags(&x->comm_stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&x->ev_grads, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&x->ev_comm, hipEventDisableTiming) != hipSuccess)
    rc = fail(MFM_EHIP, "communication stream / events: %s", hipGetErrorString(hipGetLastError()));
  if (rc == MFM_OK) {
    const ncclResult_t r = R->CommInitRank(&x->comm, nranks, id, rank);
    if (r != ncclSuccess) { x->comm = nullptr; rc = fail(MFM_EHIP, "RCCL: %s", R->GetErrorString(r)); }
  }
  if (rc != MFM_OK) { (void)mfm_comm_destroy(x); return rc; }      // nothing of a failed init survives: a retry starts clean
  x->comm_nranks = nranks;
  return MFM_OK;
}

// Ranks of the context's communicator AS RCCL REPORTS THEM (ncclCommCount), 0 without a communicator: what a scaling record
// cites to show that the all-reduce spanned N ranks.
extern "C" int mfm_comm_count(mfm_ctx* x, int32_t* out) { use_ctx(x);
  if (!x || !out) return fail(MFM_EINVAL, "null argument");
  *out = 0;
  if (!x->comm) return MFM_OK;
  RcclApi* R = rccl_api();
  int n = 0;
  RCCLCHK(R->CommCount(x->comm, &n));
  *out = n;
  return MFM_OK;
}

// Starts the SUM all-reduce of the flow-matching gradient over the context's communicator on the context's communication
// stream, ordered after everything queued on the context's stream so far; returns at once.  Work the caller queues next that
// touches neither the gradient nor the parameters (the MALA step of the following iteration) overlaps it; the next
// mfm_adamw_step on the same buffer waits for it.
extern "C" int mfm_grad_allreduce_begin(mfm_ctx* x, float* d_grads) { use_ctx(x);
  if (!x || !d_grads) return fail(MFM_EINVAL, "null argument");
  if (!x->comm) return fail(MFM_EINVAL, "no communicator (mfm_comm_init)");
  if (x->comm_pending) return fail(MFM_EINVAL, "an all-reduce is already in flight: apply it with mfm_adamw_step first");
  RcclApi* R = rccl_api();
  HIPCHK(hipEventRecord(x->ev_grads, x->stream));
  HIPCHK(hipStreamWaitEvent(x->comm_stream, x->ev_grads, 0));
  RCCLCHK(R->AllReduce(d_grads, d_grads, (size_t)x->net.n_params, ncclFloat32, ncclSum, x->comm, x->comm_stream));
  HIPCHK(hipEventRecord(x->ev_comm, x->comm_stream));
  x->comm_pending = d_grads;
  return MFM_OK;
}

extern "C" int mfm_adamw_step(mfm_ctx* x, const float* d_grads) { use_ctx(x);
  if (!x || !d_grads) return fail(MFM_EINVAL, "null argument");
  AdamArgs a = adam_args(x, d_grads, 1);
  a.inline_decide = (x->checked_grads == d_grads) ? 1 : 0;
  x->checked_grads = nullptr;
  if (x->comm) {
    // the gradient every rank applies is the SUM over the communicator (exe_flow_matching.py:178 sums over ALL chains): started
    // earlier by mfm_grad_allreduce_begin, or here
    if (x->comm_pending != d_grads) {
      if (x->comm_pending) return fail(MFM_EINVAL, "an all-reduce of another buffer is in flight");
      if (!g_sw.rccl_comm_stream) {     // nothing to overlap with: the collective in line on the context's stream, no event hops
        RcclApi* R = rccl_api();
        RCCLCHK(R->AllReduce(d_grads, const_cast<float*>(d_grads), (size_t)x->net.n_params, ncclFloat32, ncclSum, x->comm, x->stream));
      } else {
        const int rc = mfm_grad_allreduce_begin(x, const_cast<float*>(d_grads));
        if (rc) return rc;
      }
    }
    if (x->comm_pending) HIPCHK(hipStreamWaitEvent(x->stream, x->ev_comm, 0));
    x->comm_pending = nullptr;
    if (x->comm_nranks > 1) a.inline_decide = 0;      // the finite check must see the reduced gradient
  }
  ProfScope ps_(x, PROF_ADAM);
  launch_adamw(a, x->stream);
  LAUNCHCHK();
  x->ctr[CTR_OPT_STEPS] += 1;
  return MFM_OK;
}

extern "C" int mfm_flow_step(mfm_ctx* x, int mode, uint32_t k0, uint32_t k1, double beta, float* d_pos, double* d_logp, float* d_grad,
                             float* d_acc, uint8_t* d_is_acc, float* d_prop, int32_t* d_nsteps);

// exe_flow_matching.py:432-439 as one call: generator (:300-314) + train_step (:362-368); see include/mfm.h
extern "C" int mfm_train_iter(mfm_ctx* x, int64_t count, int K, int flow_mode, uint32_t gk0, uint32_t gk1, uint32_t tk0, uint32_t tk1,
                              double beta, double step_size, float* d_pos, double* d_logp, float* d_grad, float* d_acc,
                              int32_t* d_nsteps, double* d_loss, float* d_grads, int apply_update) { use_ctx(x);
  if (!x) return fail(MFM_EINVAL, "null context");
  if (K < 1) return fail(MFM_EINVAL, "mfm_train_iter serves mcmc_per_flow_steps >= 1; compose the other schedules from the separate calls");
  if (count < 0) return fail(MFM_EINVAL, "count must be non-negative");
  int rc;
  const bool no_fuse = g_sw.no_fused_mala;
  if (count % ((int64_t)K + 1) == 0) rc = mfm_flow_step(x, flow_mode, gk0, gk1, beta, d_pos, d_logp, d_grad, d_acc, nullptr, nullptr, d_nsteps);
  else if (x->has_target && !x->wide && !no_fuse && fm_mala_fusable(x->net)) {
    // the MALA step rides in the training kernel (fm.hip: fm_fwd_bwd_kernel<.., MALA>): same arithmetic, same draws, one launch less
    if (!d_pos || !d_logp || !d_grad) return fail(MFM_EINVAL, "null device pointer");
    if (!(step_size > 0)) return fail(MFM_EINVAL, "step_size must be positive");
    // everything fm_loss_grad_impl / fm_common would reject is rejected HERE, before the prefetched slot of this MALA step is
    // consumed: an early error must leave the prefetch cursor where it was (a retry then finds its draws)
    if (!d_loss || !d_grads) return fail(MFM_EINVAL, "null device pointer");
    if (!x->has_fourier) return fail(MFM_EINVAL, "mfm_set_fourier has not been called");
    FmMala m; memset(&m, 0, sizeof m);
    m.on = 1; m.key = Key2{gk0, gk1}; m.beta = beta; m.eps = step_size; m.logp = d_logp; m.grad = d_grad; m.acc_prob = d_acc;
    const int slot = noise_take(x, m.key, false);
    if (slot >= 0) {
      const size_t B = (size_t)x->cfg.n_chain_local;
      m.pre_n = x->noise->mala_n + (size_t)slot * B * x->cfg.dim; m.pre_u = x->noise->mala_u + (size_t)slot * B;
    }
    x->fuse_mala = m;
    const bool with_opt = apply_update && opt_fusable(x);
    rc = fm_loss_grad_impl(x, tk0, tk1, d_pos, d_loss, d_grads, with_opt);
    x->fuse_mala.on = 0;
    // the fused step reads x, g, logp and writes x, g, logp, acc: the proposed position never leaves the workgroup (4 (4d + 4) B)
    if (rc == MFM_OK) { x->ctr[CTR_MALA] += x->cfg.n_chain_local; x->ctr[CTR_MALA_BYTES] += (int64_t)x->cfg.n_chain_local * 4 * (4 * x->cfg.dim + 4); }
    if (rc || !apply_update || with_opt) return rc;
    return mfm_adamw_step(x, d_grads);
  }
  else rc = mfm_mala_step(x, gk0, gk1, beta, step_size, 0, d_pos, d_logp, d_grad, d_acc, nullptr, nullptr, nullptr);
  if (rc) return rc;
  const bool with_opt = apply_update && x->has_target && opt_fusable(x);
  rc = fm_loss_grad_impl(x, tk0, tk1, d_pos, d_loss, d_grads, with_opt);
  if (rc || !apply_update || with_opt) return rc;
  return mfm_adamw_step(x, d_grads);
}

extern "C" int mfm_opt_state(mfm_ctx* x, int32_t out[4], float* lr) { use_ctx(x);
  if (!x || !out) return fail(MFM_EINVAL, "null argument");
  OptState s;
  HIPCHK(hipStreamSynchronize(x->stream));
  HIPCHK(hipMemcpy(&s, x->opt, sizeof s, hipMemcpyDeviceToHost));
  out[0] = s.step; out[1] = s.count; out[2] = s.notfinite_count; out[3] = s.last_applied;
  if (lr) *lr = s.last_lr;
  return MFM_OK;
}

// ---- algorithmic counters (mfm_get_counters) ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tally_attempts_kernel(const int* nsteps, int n, unsigned long long* out) {
  __shared__ unsigned long long part[4];
  unsigned long long s = 0;
  for (int i = threadIdx.x; i < n; i += 256) s += (unsigned long long)nsteps[i];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(out, part[0] + part[1] + part[2] + part[3]);
}
// the solver kernels report attempted steps per sample; where the caller did not ask for them the context lends a buffer
static int* att_buffer(mfm_ctx* x, int32_t* d_nsteps, int n) {
  if (d_nsteps) return d_nsteps;
  if ((size_t)n > x->att_cap) {
    if (x->att_buf) { (void)hipStreamSynchronize(x->stream); (void)hipFree(x->att_buf); x->att_buf = nullptr; x->att_cap = 0; }
    if (hipMalloc((void**)&x->att_buf, (size_t)n * sizeof(int)) != hipSuccess) return nullptr;
    x->att_cap = (size_t)n;
  }
  return x->att_buf;
}
static void tally_solves(mfm_ctx* x, const int* nsteps, int n, int solves_per_sample) {
  x->ctr[CTR_SOLVES] += (int64_t)n * solves_per_sample;
  if (nsteps) hipLaunchKernelGGL(tally_attempts_kernel, dim3(1), dim3(256), 0, x->stream, nsteps, n, x->d_att);
}

extern "C" int mfm_get_counters(mfm_ctx* x, int64_t h_out[8]) { use_ctx(x);
  if (!x || !h_out) return fail(MFM_EINVAL, "null argument");
  unsigned long long att = 0;
  HIPCHK(hipStreamSynchronize(x->stream));
  HIPCHK(hipMemcpy(&att, x->d_att, sizeof att, hipMemcpyDeviceToHost));
  for (int i = 0; i < 8; ++i) h_out[i] = x->ctr[i];
  h_out[CTR_ATTEMPTS] = (int64_t)att;
  if (x->cfg.ode_method != MFM_ODE_DOPRI5 && x->cfg.ode_steps > 0)          // fixed steps: four (RK4) or one (Euler) evaluation per step
    h_out[CTR_FIELD_EVALS] = (x->cfg.ode_method == MFM_ODE_RK4 ? 4 : 1) * (int64_t)att;
  else h_out[CTR_FIELD_EVALS] = 2 * x->ctr[CTR_SOLVES] + 6 * (int64_t)att;      // odeint: f(y0), the initial-step probe, six stages per attempt
  return MFM_OK;
}
extern "C" int mfm_reset_counters(mfm_ctx* x) { use_ctx(x);
  if (!x) return fail(MFM_EINVAL, "null ctx");
  for (int i = 0; i < 8; ++i) x->ctr[i] = 0;
  HIPCHK(hipMemsetAsync(x->d_att, 0, sizeof(unsigned long long), x->stream));
  return MFM_OK;
}

extern "C" int mfm_debug_replay(mfm_ctx* x, int cap, const float* d_dt, const uint8_t* d_acc, float* d_ratio, float* d_dt_own, double* d_diag) { use_ctx(x);
  if (!x) return fail(MFM_EINVAL, "null ctx");
  if (!d_dt) { memset(&x->replay, 0, sizeof x->replay); return MFM_OK; }          // disarm
  if (!d_acc || !d_ratio || !d_dt_own || cap < 2) return fail(MFM_EINVAL, "mfm_debug_replay needs all four arrays and cap >= 2");
  x->replay.dt = d_dt; x->replay.acc = d_acc; x->replay.ratio = d_ratio; x->replay.dt_own = d_dt_own; x->replay.cap = cap; x->replay.n = 0; x->replay.diag = d_diag;
  return MFM_OK;
}

extern "C" int mfm_vf_apply(mfm_ctx* x, const float* d_x, const float* d_t, const float* d_tan, int n, float* d_v, float* d_jvp) { use_ctx(x);
  NEED_TARGET();
  if (!x->has_fourier) return fail(MFM_EINVAL, "mfm_set_fourier has not been called");
  if (!d_x || !d_t || !d_v || ((d_tan == nullptr) != (d_jvp == nullptr))) return fail(MFM_EINVAL, "bad pointer arguments");
  if (n <= 0 || n % 16) return fail(MFM_EUNSUPPORTED, "n must be a positive multiple of 16");
  if (x->wide) {
    if (wide::vf_apply(x->wide, x->net, d_x, d_t, d_tan, n, d_v, d_jvp, x->stream)) return fail(MFM_EHIP, "wide vf_apply failed");
    LAUNCHCHK();
    return MFM_OK;
  }
  int rc = launch_vf_apply(x->net, d_x, d_t, d_tan, n, d_v, d_jvp, x->stream);
  if (rc) return fail(rc, "vf_apply cannot be launched for this configuration");
  LAUNCHCHK();
  return MFM_OK;
}

extern "C" int mfm_ode_transform(mfm_ctx* x, int direction, int per_chain, const uint32_t* d_keys, uint32_t k0, uint32_t k1,
                                 const float* d_in, int n, float* d_out, float* d_ldj, int32_t* d_nsteps) { use_ctx(x);
  NEED_TARGET();
  if (!x->has_fourier) return fail(MFM_EINVAL, "mfm_set_fourier has not been called");
  if (!d_in || !d_out || !d_ldj || (per_chain && !d_keys)) return fail(MFM_EINVAL, "null device pointer");
  if (direction != 1 && direction != -1) return fail(MFM_EINVAL, "direction must be +1 or -1");
  if (n <= 0 || n % 16) return fail(MFM_EUNSUPPORTED, "n must be a positive multiple of 16");
  if ((size_t)n > x->ode.rows) return fail(MFM_ETOOLARGE, "n=%d exceeds max_eval_samples given at mfm_create", n);
  OdeArgs a = ode_args(x->net, x->cfg, x->ode);
  a.direction = direction; a.per_chain_keys = per_chain; a.keys = d_keys; a.key = Key2{k0, k1};
  a.in = d_in; a.out = d_out; a.ldj = d_ldj; a.n = n;
  a.nsteps = d_nsteps = att_buffer(x, d_nsteps, n);
  a.rp = x->replay; a.rp.n = n; memset(&x->replay, 0, sizeof x->replay);      // one-shot
  if (wide::Ctx* ws = x->wide ? x->wide : x->wide_ex) {
    if (a.fixed_steps > 0 && a.rp.dt) return fail(MFM_EUNSUPPORTED, "fixed-step mode (ode_method / ode_steps): the prescribed-step replay (mfm_debug_replay) is for the adaptive solver");
    launch_probe(per_chain ? 0 : 1, d_keys, a.key, 0, 0, 0, n, x->net.d, const_cast<float*>(a.z1), x->stream);
    wide::WReplay wr{a.rp.dt, a.rp.acc, a.rp.ratio, a.rp.dt_own, a.rp.cap, a.rp.n, 0, 0, nullptr};
    const int rcw = wide::transform(ws, x->net, direction, a.rtol, a.atol, a.max_attempts, a.z1, d_in, n, d_out, d_ldj, d_nsteps, x->stream, wr,
                                    a.fixed_method, a.fixed_steps);
    if (rcw) return fail(rcw, "wide ODE transform failed: %s", hipGetErrorString(hipGetLastError()));
    LAUNCHCHK();
    tally_solves(x, d_nsteps, n, 1);
    return MFM_OK;
  }
  int rc = launch_ode_transform(a, x->stream);
  if (rc == -4) return fail(MFM_EUNSUPPORTED, "fixed-step mode (ode_method / ode_steps): not built for the generic 16-chain tile (d = 2 with --hutch, MFM_D2_TILE=16, MFM_TILE_EXACT) nor for the prescribed-step replay");
  if (rc) return fail(rc, "ODE kernel cannot be launched for this configuration");
  LAUNCHCHK();
  tally_solves(x, d_nsteps, n, 1);
  return MFM_OK;
}

extern "C" int mfm_flow_step(mfm_ctx* x, int mode, uint32_t k0, uint32_t k1, double beta, float* d_pos, double* d_logp,
                             float* d_grad, float* d_acc, uint8_t* d_isacc, float* d_prop, int32_t* d_nsteps) { use_ctx(x);
  NEED_TARGET();
  if (!x->has_fourier) return fail(MFM_EINVAL, "mfm_set_fourier has not been called");
  if (!d_pos || !d_logp || !d_grad) return fail(MFM_EINVAL, "null device pointer");
  if (mode != MFM_FLOW_RWMH && mode != MFM_FLOW_IMH) return fail(MFM_EINVAL, "unknown flow step mode %d", mode);
  OdeArgs a = ode_args(x->net, x->cfg, x->ode);
  a.n = x->cfg.n_chain_local;
  FlowArgs f; memset(&f, 0, sizeof f);
  f.mode = mode; f.key = Key2{k0, k1}; f.n_total = x->cfg.n_chain_total; f.chain_offset = x->cfg.chain_offset;
  f.beta = beta; f.ref_std = (float)x->cfg.ref_std; f.pos = d_pos; f.logp = d_logp; f.grad = d_grad; f.acc_prob = d_acc; f.accepted = d_isacc;
  f.proposed = d_prop; f.nsteps = d_nsteps = att_buffer(x, d_nsteps, a.n);
  a.rp = x->replay; a.rp.n = a.n; memset(&x->replay, 0, sizeof x->replay);    // one-shot
  // draws of the following iterations, produced by the workgroups of this launch whose tile is done (noise.hip); only the
  // shape-specialised kernel carries that tail: elsewhere the request is dropped and the consumers draw in line
  NoiseArgs nz; memset(&nz, 0, sizeof nz);
  if (x->noise) {
    NoiseWs* w = x->noise;
    w->n_valid = 0;
    const bool fast_path = !x->wide && fast::shape_ok(x->net, x->cfg.hutch) && !g_sw.generic_ode && a.fixed_steps == 0;
    if (w->n_armed > 0 && fast_path) {
      const int B = x->cfg.n_chain_local;
      nz.gn = w->d_keys; nz.st = w->d_keys + 2 * (size_t)w->n_armed; nz.n_slots = w->n_armed;
      nz.n_total = (uint32_t)x->cfg.n_chain_total; nz.chain_offset = (uint32_t)x->cfg.chain_offset; nz.B = B; nz.d = x->cfg.dim;
      nz.mala_n = w->mala_n; nz.mala_u = w->mala_u; nz.fm_x0 = w->fm_x0; nz.fm_eps = w->fm_eps; nz.fm_t = w->fm_t;
      nz.counter = w->counter; nz.groups = (B + 7) / 8; nz.n_items = nz.groups * w->n_armed;
      nz.skip_mala0 = w->gn[0].k0 == k0 && w->gn[0].k1 == k1; w->no_mala0 = nz.skip_mala0 != 0;      // (slot 0 = this flow iteration's own keys: its MALA draws are never used)
      HIPCHK(hipMemsetAsync(w->counter, 0, sizeof(int), x->stream));
      w->n_valid = w->n_armed; w->cur_gn = w->cur_st = 0;
    }
    w->n_armed = 0;
  }
  int rc = 0;
  {
    ProfScope ps_(x, PROF_FLOW);
    if (wide::Ctx* ws = x->wide ? x->wide : x->wide_ex) {
      if (a.fixed_steps > 0 && a.rp.dt) return fail(MFM_EUNSUPPORTED, "fixed-step mode (ode_method / ode_steps): the prescribed-step replay (mfm_debug_replay) is for the adaptive solver");
      launch_probe(2, nullptr, f.key, f.n_total, f.chain_offset, 0, a.n, x->net.d, const_cast<float*>(a.zgen), x->stream);     // key_gen
      launch_probe(2, nullptr, f.key, f.n_total, f.chain_offset, 3, a.n, x->net.d, const_cast<float*>(a.z1), x->stream);       // key_hutch2
      launch_probe(2, nullptr, f.key, f.n_total, f.chain_offset, 2, a.n, x->net.d, const_cast<float*>(a.z2), x->stream);       // key_hutch1
      wide::FlowCall c; memset(&c, 0, sizeof c);
      c.mode = mode; c.key = f.key; c.n_total = f.n_total; c.chain_offset = f.chain_offset; c.beta = beta; c.rows = a.n; c.ref_std = f.ref_std;
      c.rtol = a.rtol; c.atol = a.atol; c.max_attempts = a.max_attempts; c.fixed_method = a.fixed_method; c.fixed_steps = a.fixed_steps; c.z_inv = a.z1; c.z_fwd = a.z2; c.zgen = a.zgen;
      c.pos = d_pos; c.logp = d_logp; c.grad = d_grad; c.acc_prob = d_acc; c.accepted = d_isacc; c.proposed = d_prop; c.nsteps = d_nsteps;
      c.rp = wide::WReplay{a.rp.dt, a.rp.acc, a.rp.ratio, a.rp.dt_own, a.rp.cap, a.rp.n, 0, 0, a.rp.diag};
      const int rcw = wide::flow_step(ws, x->net, c, x->stream);
      if (rcw) return fail(rcw, "wide flow step failed: %s", hipGetErrorString(hipGetLastError()));
    } else {
      rc = launch_flow_step(a, f, nz, x->stream);
      if (rc == -4) return fail(MFM_EUNSUPPORTED, "fixed-step mode (ode_method / ode_steps): not built for the generic 16-chain tile (d = 2 with --hutch, MFM_D2_TILE=16, MFM_TILE_EXACT), the independent flow step of the shape-specialised tile, nor the prescribed-step replay");
      if (rc) return fail(rc, "flow step cannot be launched for this configuration");
    }
    LAUNCHCHK();
  }
  // (rows >= n_chain_valid of a padded shard are integrated like any other but are no chains: not counted)
  tally_solves(x, d_nsteps, x->cfg.n_chain_valid > 0 && x->cfg.n_chain_valid < a.n ? x->cfg.n_chain_valid : a.n, 2);
  return MFM_OK;
}

extern "C" int mfm_beta_update(mfm_ctx* x, double prev_beta, const double* d_ll, int n, double alpha, double* h_out) { use_ctx(x);
  if (!x || !d_ll || !h_out) return fail(MFM_EINVAL, "null argument");
  if (n <= 0) return fail(MFM_EINVAL, "n must be positive");
  launch_beta(prev_beta, d_ll, n, alpha, x->beta_out, x->stream);
  LAUNCHCHK();
  HIPCHK(hipMemcpyAsync(h_out, x->beta_out, sizeof(double), hipMemcpyDeviceToHost, x->stream));
  HIPCHK(hipStreamSynchronize(x->stream));
  return MFM_OK;
}

// ---- reference-distribution rows and the CIS selection step ---------------------------------------------------------
extern "C" int mfm_normal_rows(mfm_ctx* x, const uint32_t* d_keys, int n, float* d_out) { use_ctx(x);
  if (!x || !d_keys || !d_out) return fail(MFM_EINVAL, "null argument");
  if (n <= 0) return fail(MFM_EINVAL, "n must be positive");
  launch_probe(0, d_keys, Key2{0, 0}, 0, 0, 0, n, x->cfg.dim, d_out, x->stream);
  LAUNCHCHK();
  return MFM_OK;
}

extern "C" int mfm_cis_select(mfm_ctx* x, uint32_t k0, uint32_t k1, int n_is, const float* d_u0, const float* d_vol0, const float* d_refs,
                              const float* d_xs, const float* d_vols, const double* d_lps, float* d_pos, double* d_logp, float* d_acc,
                              uint8_t* d_isacc, float* d_prop, float* d_weight) { use_ctx(x);
  if (!x || !d_u0 || !d_vol0 || !d_refs || !d_xs || !d_vols || !d_lps || !d_pos || !d_logp) return fail(MFM_EINVAL, "null argument");
  if (n_is <= 0) return fail(MFM_EINVAL, "num_importance_samples must be positive");
  CisArgs a; memset(&a, 0, sizeof a);
  a.key = Key2{k0, k1}; a.n_total = x->cfg.n_chain_total; a.chain_offset = x->cfg.chain_offset;
  a.B = x->cfg.n_chain_local; a.d = x->cfg.dim; a.n_is = n_is; a.ref_std = x->cfg.ref_std;
  a.u0 = d_u0; a.vol0 = d_vol0; a.refs = d_refs; a.xs = d_xs; a.vols = d_vols; a.lps = d_lps;
  a.pos = d_pos; a.logp = d_logp; a.acc_prob = d_acc; a.accepted = d_isacc; a.proposed = d_prop; a.weight = d_weight;
  ProfScope ps_(x, PROF_FLOW);
  launch_cis_select(a, x->stream);
  LAUNCHCHK();
  return MFM_OK;
}

// ---- sample-quality metrics (mcmc_utils.py:28-111) ----------------------------------------------------------------
static int pair_call(mfm_ctx* x, int mode, const float* A, const float* GA, const float* B, const float* GB, int na, int nb, float beta, double h[2]) {
  double* ws = nullptr;
  const size_t parts = pair_sum_parts(na, nb);
  HIPCHK(hipMalloc((void**)&ws, (2 * parts + 2) * sizeof(double)));
  launch_pair_sum(mode, A, GA, B, GB, na, nb, x->cfg.dim, beta, ws + 2, ws, x->stream);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(h, ws, 2 * sizeof(double), hipMemcpyDeviceToHost, x->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(x->stream);
  (void)hipFree(ws);
  if (e != hipSuccess) return fail(MFM_EHIP, "pair-sum kernel: %s", hipGetErrorString(e));
  return MFM_OK;
}

extern "C" int mfm_stein_disc(mfm_ctx* x, const float* d_x, const float* d_grad, int n, double beta, double h_out[2]) { use_ctx(x);
  if (!x || !d_x || !d_grad || !h_out) return fail(MFM_EINVAL, "null argument");
  if (n < 2) return fail(MFM_EINVAL, "stein_disc needs at least 2 samples");
  double h[2];
  int rc = pair_call(x, 0, d_x, d_grad, d_x, d_grad, n, n, (float)(-beta), h);      /* mcmc_utils.py:54: beta = -beta */
  if (rc) return rc;
  h_out[0] = (h[0] - h[1]) / ((double)n * (double)(n - 1));                         /* :85 U-statistic */
  h_out[1] = h[0] / ((double)n * (double)n);                                        /*     V-statistic */
  return MFM_OK;
}

extern "C" int mfm_max_mean_disc(mfm_ctx* x, const float* d_x, const float* d_y, int m, double* h_out) { use_ctx(x);
  if (!x || !d_x || !d_y || !h_out) return fail(MFM_EINVAL, "null argument");
  if (m < 2) return fail(MFM_EINVAL, "max_mean_disc needs at least 2 samples");
  double xx[2], yy[2], xy[2];
  int rc = pair_call(x, 1, d_x, nullptr, d_x, nullptr, m, m, 0.f, xx); if (rc) return rc;
  rc = pair_call(x, 1, d_y, nullptr, d_y, nullptr, m, m, 0.f, yy); if (rc) return rc;
  rc = pair_call(x, 1, d_x, nullptr, d_y, nullptr, m, m, 0.f, xy); if (rc) return rc;
  const double m2 = (double)m * (double)m;
  *h_out = (xx[0] - m) / (m2 - m) - 2.0 * xy[0] / m2 + (yy[0] - m) / (m2 - m);      /* mcmc_utils.py:106-110 */
  return MFM_OK;
}

// ---- chain diagnostics (diag.hip; mcmc_utils.py:131-165) ----------------------------------------------------------------------
extern "C" int mfm_autocorr(mfm_ctx* x, const float* d_x, int64_t n, int64_t n_series, int32_t n_lags, float* d_rho, float* d_tau, float* d_ess,
                            double* d_mean, double* d_var) { use_ctx(x);
  if (!x) return fail(MFM_EINVAL, "null ctx");
  if (!d_x) return fail(MFM_EINVAL, "d_x is null");
  if (n < 1) return fail(MFM_EINVAL, "n must be at least 1 (got %lld)", (long long)n);
  if (n_series < 1) return fail(MFM_EINVAL, "n_series must be at least 1 (got %lld)", (long long)n_series);
  if (n_lags < 1 || n_lags > n) return fail(MFM_EINVAL, "n_lags must be in [1, n = %lld] (got %d)", (long long)n, n_lags);
  if (!d_rho && !d_tau && !d_ess && !d_mean && !d_var) return fail(MFM_EINVAL, "every output (d_rho, d_tau, d_ess, d_mean, d_var) is null");
  double* mean_ws = d_mean;
  if (!mean_ws) {
    const size_t need = (size_t)n_series * sizeof(double);
    if (x->ac_ws_cap < need) {
      if (x->ac_ws) { HIPCHK(hipStreamSynchronize(x->stream)); (void)hipFree(x->ac_ws); x->ac_ws = nullptr; x->ac_ws_cap = 0; }
      HIPCHK(hipMalloc(&x->ac_ws, need));
      x->ac_ws_cap = need;
    }
    mean_ws = (double*)x->ac_ws;
  }
  if (launch_autocorr(g_sw.autocorr_f64, d_x, n, n_series, n_lags, d_rho, d_tau, d_ess, mean_ws, d_var, x->stream))
    return fail(MFM_ETOOLARGE, "n_series = %lld / n_lags = %d exceed the launch grid of the autocorrelation kernel", (long long)n_series, n_lags);
  LAUNCHCHK();
  return MFM_OK;
}

extern "C" int mfm_chain_sums(mfm_ctx* x, const float* d_x, int64_t n, int32_t n_chain, int32_t n_chain_ld, int32_t dim, int32_t split, int32_t n_lags,
                              double* d_sums) { use_ctx(x);
  if (!x) return fail(MFM_EINVAL, "null ctx");
  if (!d_x) return fail(MFM_EINVAL, "d_x is null");
  if (!d_sums) return fail(MFM_EINVAL, "d_sums is null");
  if (split != 0 && split != 1) return fail(MFM_EINVAL, "split must be 0 or 1 (got %d)", split);
  const int64_t n_sub = split ? n / 2 : n;
  if (n_sub < 2) return fail(MFM_EINVAL, "n_sub must be at least 2 (n = %lld with split = %d gives n_sub = %lld)", (long long)n, split, (long long)n_sub);
  if (n_chain_ld < 1 || n_chain < 1 || n_chain > n_chain_ld)
    return fail(MFM_EINVAL, "n_chain must be in [1, n_chain_ld = %d] (got %d)", n_chain_ld, n_chain);
  if (dim < 1) return fail(MFM_EINVAL, "dim must be at least 1 (got %d)", dim);
  if (n_lags < 1 || n_lags > n_sub) return fail(MFM_EINVAL, "n_lags must be in [1, n_sub = %lld] (got %d)", (long long)n_sub, n_lags);
  const ChainPlan q = chain_plan(n_chain, dim, n_lags);
  const size_t need = (chain_stats_count(n_chain, dim, split) + (size_t)q.n_slices * ((size_t)n_lags + 2) * (size_t)dim) * sizeof(double);
  if (x->cs_ws_cap < need) {
    if (x->cs_ws) { HIPCHK(hipStreamSynchronize(x->stream)); (void)hipFree(x->cs_ws); x->cs_ws = nullptr; x->cs_ws_cap = 0; }
    HIPCHK(hipMalloc(&x->cs_ws, need));
    x->cs_ws_cap = need;
  }
  if (launch_chain_sums(g_sw.autocorr_f64, d_x, n, n_chain, n_chain_ld, dim, split, n_lags, q, (double*)x->cs_ws, d_sums, x->stream))
    return fail(MFM_ETOOLARGE, "dim = %d / n_lags = %d exceed the launch grid of the chain-sums kernel", dim, n_lags);
  LAUNCHCHK();
  return MFM_OK;
}

extern "C" int mfm_chain_diag(mfm_ctx* x, const double* d_sums, int64_t n_sub, int64_t n_subchains, int32_t dim, int32_t n_lags, float* d_rhat, float* d_ess,
                              float* d_tau, float* d_rho) { use_ctx(x);
  if (!x) return fail(MFM_EINVAL, "null ctx");
  if (!d_sums) return fail(MFM_EINVAL, "d_sums is null");
  if (n_sub < 2) return fail(MFM_EINVAL, "n_sub must be at least 2 (got %lld)", (long long)n_sub);
  if (n_subchains < 2) return fail(MFM_EINVAL, "n_subchains must be at least 2 (got %lld)", (long long)n_subchains);
  if (dim < 1) return fail(MFM_EINVAL, "dim must be at least 1 (got %d)", dim);
  if (n_lags < 1 || n_lags > n_sub) return fail(MFM_EINVAL, "n_lags must be in [1, n_sub = %lld] (got %d)", (long long)n_sub, n_lags);
  if (!d_rhat && !d_ess && !d_tau && !d_rho) return fail(MFM_EINVAL, "every output (d_rhat, d_ess, d_tau, d_rho) is null");
  launch_chain_diag(d_sums, n_sub, n_subchains, dim, n_lags, d_rhat, d_ess, d_tau, d_rho, x->stream);
  LAUNCHCHK();
  return MFM_OK;
}

// ---- Stein variational gradient descent (svgd.hip; bblackjax/vi/svgd.py, optimizers/cocob.py) -----------------------------------------
#define MFM_SVGD_MAX_N 16384      /* D [n][n] float32 passes 1 GiB beyond */
static int svgd_grow(mfm_ctx* x, void*& p, size_t& cap, size_t need) {
  if (cap >= need) return MFM_OK;
  if (p) { HIPCHK(hipStreamSynchronize(x->stream)); (void)hipFree(p); p = nullptr; cap = 0; }
  HIPCHK(hipMalloc(&p, need));
  cap = need;
  return MFM_OK;
}
static int svgd_check_shape(int32_t n, int32_t d) {
  if (n > MFM_SVGD_MAX_N) return fail(MFM_ETOOLARGE, "n = %d particles exceed %d (the distance matrix would pass 1 GiB)", n, MFM_SVGD_MAX_N);
  if (n < 2) return fail(MFM_EINVAL, "n must be at least 2 (got %d)", n);
  if (d < 1) return fail(MFM_EINVAL, "d must be at least 1 (got %d)", d);
  return MFM_OK;
}
static int svgd_scratch(mfm_ctx* x, int32_t n, int32_t d, svgd::Scratch* s) {
  CHECKED(svgd_grow(x, x->svgd_ws, x->svgd_ws_cap, svgd::scratch_bytes(n, d)));
  *s = svgd::carve(x->svgd_ws, n, d);
  return MFM_OK;
}

extern "C" int mfm_svgd_sqdist(mfm_ctx* x, const float* d_x, int32_t n, int32_t d, float* d_D) { use_ctx(x);
  if (!x) return fail(MFM_EINVAL, "null ctx");
  if (!d_x) return fail(MFM_EINVAL, "d_x is null");
  if (!d_D) return fail(MFM_EINVAL, "d_D is null");
  CHECKED(svgd_check_shape(n, d));
  svgd::Scratch s; CHECKED(svgd_scratch(x, n, d, &s));
  svgd::launch_sqdist(s, d_x, n, d, d_D, x->stream);
  LAUNCHCHK();
  return MFM_OK;
}

extern "C" int mfm_svgd_median(mfm_ctx* x, const float* d_D, int32_t n, double* d_length_scale) { use_ctx(x);
  if (!x) return fail(MFM_EINVAL, "null ctx");
  if (!d_D) return fail(MFM_EINVAL, "d_D is null");
  if (!d_length_scale) return fail(MFM_EINVAL, "d_length_scale is null");
  CHECKED(svgd_check_shape(n, 1));
  svgd::Scratch s; CHECKED(svgd_scratch(x, n, 1, &s));
  svgd::launch_median(s, d_D, n, d_length_scale, x->stream);
  LAUNCHCHK();
  return MFM_OK;
}

extern "C" int mfm_svgd_gradient(mfm_ctx* x, const float* d_x, const float* d_g, const float* d_D, const double* d_length_scale, int32_t n, int32_t d,
                                 int32_t i0, int32_t n_rows, float* d_fg) { use_ctx(x);
  if (!x) return fail(MFM_EINVAL, "null ctx");
  if (!d_x) return fail(MFM_EINVAL, "d_x is null");
  if (!d_g) return fail(MFM_EINVAL, "d_g is null");
  if (!d_D) return fail(MFM_EINVAL, "d_D is null");
  if (!d_length_scale) return fail(MFM_EINVAL, "d_length_scale is null");
  if (!d_fg) return fail(MFM_EINVAL, "d_fg is null");
  CHECKED(svgd_check_shape(n, d));
  if (i0 < 0 || n_rows < 1 || (int64_t)i0 + n_rows > n) return fail(MFM_EINVAL, "row range [i0 = %d, i0 + n_rows = %lld) must lie in [0, n = %d) and hold a row", i0, (long long)i0 + n_rows, n);
  svgd::Scratch s; CHECKED(svgd_scratch(x, n, d, &s));
  svgd::launch_gradient(s, d_x, d_g, d_D, d_length_scale, n, d, i0, n_rows, d_fg, false, x->stream);
  LAUNCHCHK();
  return MFM_OK;
}

static int svgd_check_opt(int kind, const double* h_hyper, int64_t count, float* const* st) {
  if (kind < MFM_SVGD_SGD || kind > MFM_SVGD_COCOB) return fail(MFM_EINVAL, "unknown optimizer kind %d (0 sgd, 1 adagrad, 2 adam, 3 cocob)", kind);
  if (!h_hyper) return fail(MFM_EINVAL, "h_hyper is null");
  if (count < 0) return fail(MFM_EINVAL, "count must not be negative (got %lld)", (long long)count);
  const int n_state = kind == MFM_SVGD_SGD ? 0 : kind == MFM_SVGD_ADAGRAD ? 1 : kind == MFM_SVGD_ADAM ? 2 : 5;
  for (int i = 0; i < n_state; ++i) if (!st[i]) return fail(MFM_EINVAL, "d_s%d is null (optimizer kind %d has %d state arrays)", i, kind, n_state);
  return MFM_OK;
}
static svgd::ApplyArgs svgd_apply_args(int kind, const double* h_hyper, int64_t count, int32_t n, int32_t d, float* d_x, const float* d_fg, float* const* st) {
  svgd::ApplyArgs a; a.kind = kind; a.count = count; a.total = (size_t)n * d; a.x = d_x; a.fg = d_fg;
  for (int i = 0; i < 4; ++i) a.hp[i] = h_hyper[i];
  for (int i = 0; i < 5; ++i) a.s[i] = st[i];
  return a;
}

extern "C" int mfm_svgd_apply(mfm_ctx* x, int kind, const double* h_hyper, int64_t count, int32_t n, int32_t d, float* d_x, const float* d_fg,
                              float* d_s0, float* d_s1, float* d_s2, float* d_s3, float* d_s4) { use_ctx(x);
  if (!x) return fail(MFM_EINVAL, "null ctx");
  if (!d_x) return fail(MFM_EINVAL, "d_x is null");
  if (!d_fg) return fail(MFM_EINVAL, "d_fg is null");
  float* st[5] = {d_s0, d_s1, d_s2, d_s3, d_s4};
  CHECKED(svgd_check_opt(kind, h_hyper, count, st));
  if (n < 1 || d < 1) return fail(MFM_EINVAL, "n and d must be at least 1 (got %d, %d)", n, d);
  svgd::launch_apply(svgd_apply_args(kind, h_hyper, count, n, d, d_x, d_fg, st), x->stream);
  LAUNCHCHK();
  return MFM_OK;
}

extern "C" int mfm_svgd_step(mfm_ctx* x, double beta, int kind, const double* h_hyper, int64_t count, int32_t n_iter, int update_median, float* d_x,
                             float* d_s0, float* d_s1, float* d_s2, float* d_s3, float* d_s4, double* d_length_scale, double* d_ls_used) { use_ctx(x);
  NEED_TARGET();
  if (x->cfg.n_chain_total != x->cfg.n_chain_local)
    return fail(MFM_EUNSUPPORTED, "n_chain_total = %d differs from n_chain_local = %d: SVGD over more than one rank is not built", x->cfg.n_chain_total, x->cfg.n_chain_local);
  const int32_t B = x->cfg.n_chain_local, d = x->cfg.dim;
  const int32_t n = x->cfg.n_chain_valid > 0 ? x->cfg.n_chain_valid : B;
  CHECKED(svgd_check_shape(n, d));
  if (n_iter < 1) return fail(MFM_EINVAL, "n_iter must be at least 1 (got %d)", n_iter);
  float* st[5] = {d_s0, d_s1, d_s2, d_s3, d_s4};
  CHECKED(svgd_check_opt(kind, h_hyper, count, st));
  if (!d_x) return fail(MFM_EINVAL, "d_x is null");
  if (!d_length_scale) return fail(MFM_EINVAL, "d_length_scale is null");
  svgd::Scratch s; CHECKED(svgd_scratch(x, n, d, &s));
  const size_t nD = ((size_t)n * n * 4 + 255) & ~(size_t)255, nG = ((size_t)B * d * 4 + 255) & ~(size_t)255, nF = ((size_t)n * d * 4 + 255) & ~(size_t)255;
  CHECKED(svgd_grow(x, x->svgd_step_ws, x->svgd_step_ws_cap, nD + nG + nF + (size_t)B * 8));
  char* base = (char*)x->svgd_step_ws;
  float* D = (float*)base; float* g = (float*)(base + nD); float* fg = (float*)(base + nD + nG); double* logp = (double*)(base + nD + nG + nF);
  bool have_D = false;           // D and the scratch's centred coordinates belong to the particles as they stand
  for (int32_t it = 0; it < n_iter; ++it) {
    CHECKED(mfm_mala_init(x, d_x, beta, logp, g));                 // the target's gradient at every row (the padding rows' is not read)
    if (d_ls_used) HIPCHK(hipMemcpyAsync(d_ls_used + it, d_length_scale, sizeof(double), hipMemcpyDeviceToDevice, x->stream));
    if (!have_D) svgd::launch_sqdist(s, d_x, n, d, D, x->stream);
    svgd::launch_gradient(s, d_x, g, D, d_length_scale, n, d, 0, n, fg, true, x->stream);
    svgd::launch_apply(svgd_apply_args(kind, h_hyper, count + it, n, d, d_x, fg, st), x->stream);
    have_D = false;
    if (update_median || it + 1 < n_iter) {                        // sqdist is a pure function of the particles: kept for the next iteration, same bits
      svgd::launch_sqdist(s, d_x, n, d, D, x->stream);
      have_D = true;
      if (update_median) svgd::launch_median(s, D, n, d_length_scale, x->stream);
    }
    LAUNCHCHK();
  }
  return MFM_OK;
}

// ---- noise prefetch (noise.hip)-------------------------------------------------------------------------------------------
extern "C" int mfm_noise_prefetch(mfm_ctx* x, int n_slots, const uint32_t* h_keys_gn, const uint32_t* h_keys_step) { use_ctx(x);
  NEED_TARGET();
  if (!h_keys_gn || !h_keys_step || n_slots <= 0) return fail(MFM_EINVAL, "bad arguments");
  if (x->wide || !x->cfg.cond_flow || !fast::shape_ok(x->net, x->cfg.hutch) || (x->cfg.ode_method != MFM_ODE_DOPRI5 && x->cfg.ode_steps > 0))
    return fail(MFM_EUNSUPPORTED, "the noise prefetch rides in the tail of the shape-specialised flow-step kernel (headline network shape, PhiFour, --hutch)");
  if (!x->noise) x->noise = new NoiseWs();
  NoiseWs* w = x->noise;
  const size_t B = (size_t)x->cfg.n_chain_local, d = (size_t)x->cfg.dim;
  if (n_slots > w->cap) {
    HIPCHK(hipStreamSynchronize(x->stream));
    for (void* p : {(void*)w->mala_n, (void*)w->mala_u, (void*)w->fm_x0, (void*)w->fm_eps, (void*)w->fm_t, (void*)w->d_keys}) if (p) (void)hipFree(p);
    w->cap = n_slots; w->n_valid = 0;
    ALLOC(w->mala_n, (size_t)n_slots * B * d); ALLOC(w->mala_u, (size_t)n_slots * B);
    ALLOC(w->fm_x0, (size_t)n_slots * B * d); ALLOC(w->fm_eps, (size_t)n_slots * B * d); ALLOC(w->fm_t, (size_t)n_slots * B);
    ALLOC(w->d_keys, (size_t)4 * n_slots);
    if (!w->counter) ALLOC(w->counter, 4);
  }
  // the key upload is ordered on the context's stream before the flow step that consumes it; the staging copy must outlive
  // the asynchronous copy of a pageable source, which HIP stages synchronously
  w->h_keys.assign(h_keys_gn, h_keys_gn + 2 * (size_t)n_slots);
  w->h_keys.insert(w->h_keys.end(), h_keys_step, h_keys_step + 2 * (size_t)n_slots);
  HIPCHK(hipMemcpyAsync(w->d_keys, w->h_keys.data(), w->h_keys.size() * sizeof(uint32_t), hipMemcpyHostToDevice, x->stream));
  w->gn.resize(n_slots); w->st.resize(n_slots);
  for (int j = 0; j < n_slots; ++j) {
    w->gn[j] = Key2{h_keys_gn[2 * j], h_keys_gn[2 * j + 1]};
    w->st[j] = Key2{h_keys_step[2 * j], h_keys_step[2 * j + 1]};
  }
  w->n_armed = n_slots; w->n_valid = 0;
  return MFM_OK;
}
extern "C" int mfm_noise_drop(mfm_ctx* x) { use_ctx(x);
  if (!x) return fail(MFM_EINVAL, "null ctx");
  if (x->noise) { x->noise->n_valid = 0; x->noise->n_armed = 0; }
  return MFM_OK;
}

// ---- N4: adaptive tempered SMC pieces (bblackjax/smc; exe_others.py:79-111) -------------------------------------------
extern "C" int mfm_smc_delta(mfm_ctx* x, const double* d_ll, int n, double target_ess, double max_delta, double* h_delta) { use_ctx(x);
  if (!x || !d_ll || !h_delta) return fail(MFM_EINVAL, "null argument");
  if (n <= 0) return fail(MFM_EINVAL, "n must be positive");
  hipLaunchKernelGGL(smc_delta_kernel, dim3(1), dim3(SMC_THREADS), 0, x->stream, d_ll, n, target_ess, max_delta, x->beta_out);
  LAUNCHCHK();
  HIPCHK(hipMemcpyAsync(h_delta, x->beta_out, sizeof(double), hipMemcpyDeviceToHost, x->stream));
  HIPCHK(hipStreamSynchronize(x->stream));
  return MFM_OK;
}
extern "C" int mfm_smc_weights(mfm_ctx* x, const double* d_ll, int n, double delta, double* d_weights, double* h_lognorm) { use_ctx(x);
  if (!x || !d_ll || !d_weights) return fail(MFM_EINVAL, "null argument");
  if (n <= 0) return fail(MFM_EINVAL, "n must be positive");
  hipLaunchKernelGGL(smc_weights_kernel, dim3(1), dim3(SMC_THREADS), 0, x->stream, d_ll, n, delta, d_weights, x->beta_out + 1);
  LAUNCHCHK();
  if (h_lognorm) {
    HIPCHK(hipMemcpyAsync(h_lognorm, x->beta_out + 1, sizeof(double), hipMemcpyDeviceToHost, x->stream));
    HIPCHK(hipStreamSynchronize(x->stream));
  }
  return MFM_OK;
}
extern "C" int mfm_smc_resample(mfm_ctx* x, uint32_t k0, uint32_t k1, const double* d_weights, int n, double* d_scratch, int32_t* d_idx) { use_ctx(x);
  if (!x || !d_weights || !d_scratch || !d_idx) return fail(MFM_EINVAL, "null argument");
  if (n <= 0) return fail(MFM_EINVAL, "n must be positive");
  hipLaunchKernelGGL(smc_resample_kernel, dim3(1), dim3(SMC_THREADS), 0, x->stream, Key2{k0, k1}, d_weights, n, d_scratch, d_idx);
  LAUNCHCHK();
  return MFM_OK;
}
extern "C" int mfm_smc_resample_scheme(mfm_ctx* x, int scheme, uint32_t k0, uint32_t k1, const double* d_weights, int n, double* d_scratch, int32_t* d_idx) { use_ctx(x);
  if (scheme == MFM_RESAMPLE_SYSTEMATIC) return mfm_smc_resample(x, k0, k1, d_weights, n, d_scratch, d_idx);
  if (!x || !d_weights || !d_scratch || !d_idx) return fail(MFM_EINVAL, "null argument");
  if (n <= 0) return fail(MFM_EINVAL, "n must be positive");
  if (scheme != MFM_RESAMPLE_STRATIFIED && scheme != MFM_RESAMPLE_MULTINOMIAL) return fail(MFM_EINVAL, "unknown resampling scheme %d", scheme);
  hipLaunchKernelGGL(smc_resample2_kernel, dim3(1), dim3(SMC_THREADS), 0, x->stream, scheme, Key2{k0, k1}, d_weights, n, d_scratch, d_idx);
  LAUNCHCHK();
  return MFM_OK;
}
extern "C" int mfm_choice_logw(mfm_ctx* x, uint32_t k0, uint32_t k1, const double* d_logw, int n, int m, double* d_scratch, int32_t* d_idx) { use_ctx(x);
  if (!x || !d_logw || !d_scratch || !d_idx) return fail(MFM_EINVAL, "null argument");
  if (n <= 0 || m <= 0) return fail(MFM_EINVAL, "n and m must be positive");
  hipLaunchKernelGGL(choice_logw_kernel, dim3(1), dim3(SMC_THREADS), 0, x->stream, Key2{k0, k1}, d_logw, n, m, d_scratch, d_idx);
  LAUNCHCHK();
  return MFM_OK;
}
extern "C" int mfm_acc_stats(mfm_ctx* x, const float* d_x, int n, double* d_out) { use_ctx(x);
  if (!x || !d_x || !d_out) return fail(MFM_EINVAL, "null argument");
  if (n <= 0) return fail(MFM_EINVAL, "n must be positive");
  hipLaunchKernelGGL(acc_stats_kernel, dim3(1), dim3(SMC_THREADS), 0, x->stream, d_x, n, d_out);
  LAUNCHCHK();
  return MFM_OK;
}
extern "C" int mfm_gather_rows(mfm_ctx* x, const float* d_src, const int32_t* d_idx, int n, int dim, float* d_dst) { use_ctx(x);
  if (!x || !d_src || !d_idx || !d_dst) return fail(MFM_EINVAL, "null argument");
  if (n <= 0 || dim <= 0) return fail(MFM_EINVAL, "n and dim must be positive");
  if (d_src == d_dst) return fail(MFM_EINVAL, "gather_rows is not in-place");
  const size_t tot = (size_t)n * dim;
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((tot + 255) / 256 < 4096 ? (tot + 255) / 256 : 4096)), dim3(256), 0, x->stream, d_src, d_idx, n, dim, d_dst);
  LAUNCHCHK();
  return MFM_OK;
}

#ifdef MFM_FM_STAMPS
extern "C" int mfm_debug_fm_buffer(unsigned long long* d_buf) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_fm_dbg), &d_buf, sizeof d_buf) == hipSuccess ? 0 : MFM_EHIP;
}
#endif
#ifdef MFM_WSK_STAMPS
extern "C" int mfm_debug_wsk_buffer(unsigned long long* d_buf) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_wsk_dbg), &d_buf, sizeof d_buf) == hipSuccess ? 0 : MFM_EHIP;
}
#endif
#ifdef MFM_STAMPS
extern "C" int mfm_debug_flow_buffer(unsigned long long* d_buf) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_flow_dbg), &d_buf, sizeof d_buf) == hipSuccess ? 0 : MFM_EHIP;
}
extern "C" int mfm_debug_eval_stamps(mfm_ctx* x, const float* d_x, const float* d_t, const float* d_tan, int n, int reps, unsigned long long* d_stamps) { use_ctx(x);
  int rc = launch_eval_stamps(x->net, d_x, d_t, d_tan, n, reps, d_stamps, x->stream);
  if (rc) return fail(rc, "eval_stamps cannot be launched");
  LAUNCHCHK();
  return MFM_OK;
}
#endif
