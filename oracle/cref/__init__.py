"""ctypes binding of ``libmfm_ref`` (``mfm_ref.c``): the float64 C / OpenMP restatement of the MFM inner loop.

ORACLE (test infrastructure; see oracle/__init__.py): loaded by ``tests/`` (checked against the numpy restatement) and by
``bench.py``'s ``cpu_baseline`` leg (the timed CPU port), never by ``mfm_amd``.  PARITY UNPINNED like the rest of ``oracle/``.

``CRef(model, params)`` wraps an ``oracle.vfield.VectorFieldNet`` with relu activations on a ``PhiFour``, ``GaussianMixture`` or
``LogGaussianCoxPines`` target; the methods mirror the numpy functions they restate (``targets.Tempered.value_and_grad``,
``mala.kernel`` with given draws, ``VectorFieldNet.forward`` / ``jacobian_trace``, ``fm.loss_and_grad`` on a given batch,
``ode.transform_and_logdet`` / ``inverse_and_logdet`` with given Hutchinson probes or the exact trace, ``flow.rwmh_step``).
``stein_sums`` / ``rbf_sum`` / ``stein_disc`` / ``max_mean_disc``: the float64 pair sums of ``oracle.metrics``.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from .. import prng
from ..mala import MALAInfo, MALAState
from ..vfield import flat_params, unflat_params

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(os.path.dirname(HERE), "_build", "libmfm_ref.so")
_lib = None


def build(force=False):
    """Compile ``mfm_ref.c`` (gcc, OpenMP) into ``oracle/_build/libmfm_ref.so`` unless it is up to date."""
    src = os.path.join(HERE, "mfm_ref.c")
    if force or not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(src):
        subprocess.run(["make", "-B", "-C", HERE], check=True, stdout=subprocess.DEVNULL)
    return LIB


class _Net(C.Structure):
    _fields_ = [("d", C.c_int), ("F", C.c_int), ("lt", C.c_int), ("lx", C.c_int), ("lxt", C.c_int),
                ("shapes", C.c_void_p), ("flat", C.c_void_p), ("fourier", C.c_void_p),
                ("grad_clip", C.c_double), ("coef", C.c_double), ("beta", C.c_double)]


class _Target(C.Structure):
    _fields_ = [("kind", C.c_int), ("d", C.c_int), ("K", C.c_int), ("coef", C.c_double), ("beta", C.c_double),
                ("modes", C.c_void_p), ("chol", C.c_void_p), ("covs", C.c_void_p), ("weights", C.c_void_p),
                ("mu", C.c_double), ("poisson_a", C.c_double), ("log_norm", C.c_double), ("counts", C.c_void_p), ("Kinv", C.c_void_p)]


KINDS = {"phi4": 0, "gmm": 1, "lgcp": 2}


class _TargetDesc:
    """The C descriptor of an ``oracle.targets`` object (keeps the arrays it points into alive).  LGCP: K^-1, mu, the counts and
    the log normaliser are taken from the object, not re-derived."""

    def __init__(self, dist):
        kind = getattr(dist, "kind", None)
        assert kind in KINDS, f"libmfm_ref covers the targets {sorted(KINDS)}, not {kind!r}"
        self.arrays = []
        t = _Target()
        t.kind, t.d = KINDS[kind], int(dist.dim)
        if kind == "phi4":
            t.coef, t.beta = float(dist.coef), float(dist.beta)
        elif kind == "gmm":
            modes, chol, covs, w = (_f64(a) for a in (dist.modes, dist.chol_covs, dist.covs, dist.weights))
            assert modes.shape == chol.shape == covs.shape == (w.shape[0], t.d)
            self.arrays += [modes, chol, covs, w]
            t.K, t.modes, t.chol, t.covs, t.weights = w.shape[0], _p(modes), _p(chol), _p(covs), _p(w)
        else:
            counts, kinv = _f64(dist.counts).reshape(-1), _f64(dist.Kinv)
            assert counts.shape == (t.d,) and kinv.shape == (t.d, t.d)
            self.arrays += [counts, kinv]
            t.mu, t.poisson_a, t.log_norm, t.counts, t.Kinv = float(dist.mu), float(dist.poisson_a), float(dist.log_norm), _p(counts), _p(kinv)
        self.kind, self.c = kind, t


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            build()
        _lib = C.CDLL(LIB)
        _lib.mfmref_threads.restype = C.c_int
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class CRef:
    """``target``: the target object the oracle evaluates (default ``model.dist``, the field's own; tests pass a deliberately altered
    one to plant an error)."""

    def __init__(self, model, params, target=None):
        dist = model.dist if target is None else target
        assert getattr(dist, "kind", None) in KINDS, "libmfm_ref covers the PhiFour, GaussianMixture and LGCP targets only"
        assert model.act(np.array([-1.0, 2.0])).tolist() == [0.0, 2.0], "libmfm_ref covers relu only"
        self.model, self.dist = model, dist
        self.lib = lib()
        self.d = int(model.dim)
        assert int(dist.dim) == self.d
        self._tgt = _TargetDesc(dist)
        self._shapes = np.ascontiguousarray(np.array(model.layer_shapes(), dtype=np.int32))
        self._fourier = _f64(model.f)
        self.set_params(params)

    def set_params(self, params):
        self._flat = np.ascontiguousarray(flat_params(params), dtype=np.float32)
        m = self.model
        coef, beta = (float(self.dist.coef), float(self.dist.beta)) if self.dist.kind == "phi4" else (0.0, 0.0)
        self._net = _Net(self.d, int(m.f.shape[0]), len(m.hidden_t), len(m.hidden_x), len(m.hidden_xt), _p(self._shapes), _p(self._flat),
                         _p(self._fourier), float(m.grad_clip or 0.0), coef, beta)

    @property
    def threads(self):
        return int(self.lib.mfmref_threads())

    def set_threads(self, n):
        self.lib.mfmref_set_threads(int(n))

    # targets.Tempered(dist, temper).value_and_grad
    def value_and_grad(self, x, temper=1.0):
        x = _f64(x); B = x.shape[0]
        logp, grad = np.empty(B), np.empty_like(x)
        assert self.lib.mfmref_target_value_grad(C.byref(self._tgt.c), _p(x), B, C.c_double(temper), _p(logp), _p(grad)) == 0
        return logp, grad

    # dist.hvp_logprob (untempered)
    def hvp(self, x, v):
        x, v = _f64(x), _f64(v)
        h = np.empty_like(x)
        assert self.lib.mfmref_target_hvp(C.byref(self._tgt.c), _p(x), _p(v), x.shape[0], _p(h)) == 0
        return h

    # mala.kernel with the Gaussian draws `noise` [B, d] and the uniforms `u` [B] given
    def mala_step(self, state, noise, u, step_size, temper=1.0, textbook=False):
        x, lp, g = (_f64(a).copy() for a in state)
        B = x.shape[0]
        p, acc = np.empty(B), np.empty(B, dtype=np.uint8)
        assert self.lib.mfmref_target_mala_step(C.byref(self._tgt.c), _p(x), _p(lp), _p(g), _p(_f64(noise)), _p(_f64(u)), B, C.c_double(step_size),
                                                C.c_double(temper), int(bool(textbook)), _p(p), _p(acc)) == 0
        return MALAState(x, lp, g), p, acc.astype(bool)

    # VectorFieldNet.forward(params, x, t, tangent=...)
    def forward(self, x, t, tangent=None):
        x, t = _f64(x), _f64(t).reshape(-1); B = x.shape[0]
        v = np.empty_like(x)
        tg = _f64(tangent) if tangent is not None else None
        jv = np.empty_like(x) if tangent is not None else None
        assert self.lib.mfmref_target_vfield(C.byref(self._net), C.byref(self._tgt.c), _p(x), _p(t), _p(tg), B, _p(v), _p(jv)) == 0
        return v if tangent is None else (v, jv)

    # VectorFieldNet.jacobian_trace: the sum of d JVPs with unit tangents (what the exact-trace solve integrates)
    def jacobian_trace(self, x, t):
        x = _f64(x); B, d = x.shape
        tr = np.zeros(B)
        for j in range(d):
            e = np.zeros_like(x); e[:, j] = 1.0
            tr += self.forward(x, t, tangent=e)[1][:, j]
        return tr

    # fm.loss_and_grad on a batch (t, cond, target) already built from its draws
    def fm_loss_grad(self, t, cond, target):
        cond, target, t = _f64(cond), _f64(target), _f64(t).reshape(-1)
        loss = C.c_double(0.0)
        g = np.empty(self._flat.shape[0], dtype=np.float32)
        assert self.lib.mfmref_target_fm_loss_grad(C.byref(self._net), C.byref(self._tgt.c), _p(cond), _p(target), _p(t), cond.shape[0], C.byref(loss), _p(g)) == 0
        return loss.value, unflat_params(self.model, g)

    # ode.transform_and_logdet (sign = +1) / inverse_and_logdet (-1), Hutchinson probes z [B, d] given (z = None: the exact trace),
    # n_ts output times linspace(0, 1, n_ts), the last one returned.
    # replay = dict(dt=[B, cap], acc=[B, cap]): the prescribed step sequence of ode.odeint's parity instrumentation; record = cap: the
    # chain's own sequence into stats["dt_seq"] [B, cap] / stats["acc_seq"] [B, cap] (zero past its last attempt), as ode.odeint records it.
    # drop_jvp = j (PLANTED ERROR, sensitivity tests only): the exact trace without its j-th JVP.
    def solve(self, x0, z, sign, rtol, atol, mxstep, stats=None, replay=None, record=0, n_ts=2, drop_jvp=-1):
        exact = z is None
        assert exact or self.d > 2, "libmfm_ref: the Hutchinson log-det on d = 2 is not covered (the d = 2 configurations take the exact trace)"
        assert drop_jvp < 0 or exact
        x0 = _f64(x0); B = x0.shape[0]
        z = None if exact else _f64(z)
        xo, ldj, natt = np.empty_like(x0), np.empty(B), np.empty(B, dtype=np.int64)
        nev = C.c_longlong(0)
        rp_dt = rp_acc = rec_dt = rec_acc = None
        cap = 0
        if replay is not None:
            rp_dt = _f64(replay["dt"]); cap = rp_dt.shape[1]
            acc_in = np.asarray(replay["acc"]).astype(np.uint8)          # (numpy's sequences: A + 1 step sizes, A decisions)
            rp_acc = np.zeros((B, cap), dtype=np.uint8); rp_acc[:, :min(cap, acc_in.shape[1])] = acc_in[:, :cap]
            assert rp_dt.shape == (B, cap)
        elif record:
            cap = int(record)
            rec_dt = np.zeros((B, cap)); rec_acc = np.zeros((B, cap), dtype=np.uint8)
        assert self.lib.mfmref_target_cnf_solve(C.byref(self._net), C.byref(self._tgt.c), int(exact), int(drop_jvp), int(n_ts), _p(x0), _p(z), int(sign),
                                                C.c_double(rtol), C.c_double(atol), int(mxstep), B, _p(xo), _p(ldj), _p(natt), C.byref(nev),
                                                _p(rp_dt), _p(rp_acc), _p(rec_dt), _p(rec_acc), cap) == 0
        if stats is not None:
            stats["n_attempted"], stats["n_evals_total"] = natt, int(nev.value)
            if rec_dt is not None:
                assert natt.max() < cap, "record capacity too small"
                stats["dt_seq"], stats["acc_seq"] = rec_dt, rec_acc.astype(bool)
        return xo, ldj

    # mala.kernel: one key per chain (mala.py:93 key_integrator, key_rmh), draws by oracle/prng.py, arithmetic in C
    def mala_kernel(self, keys, state, step_size, temper=1.0, textbook=False):
        kk = prng.split_rows(keys, 2)
        noise = prng.normal_rows(kk[:, 0], self.d)                   # util.py:80-82
        u = prng.uniform_rows(kk[:, 1])
        st, p, acc = self.mala_step(state, noise, u, step_size, temper, textbook)
        return st, MALAInfo(p, acc, None, None)

    # flow.rwmh_step (exe_flow_matching.py:264-278): keys and draws by oracle/prng.py, the two CNF solves and the target in C
    def rwmh_step(self, keys, prev, args, temper=1.0, stats=None, replay=None, record=0, drop_jvp=-1):
        """``replay = dict(inv=..., fwd=...)`` / ``record``: see ``solve`` (``stats["inv"]`` / ``stats["fwd"]`` carry the recorded sequences).
        The log-det is the Hutchinson estimator or the exact trace as ``args.hutchs`` says (the exact trace draws no probes), over
        ``args.n_ts`` output times."""
        d = self.d
        assert int(getattr(args, "num_importance_samples", 0) or 0) == 0, "libmfm_ref covers the random-walk flow step only (not IMH / CIS)"
        assert int(getattr(args, "ode_steps", 0) or 0) == 0, "libmfm_ref covers the adaptive Dopri5 solves only"
        kk = prng.split_rows(keys, 4)                                # :265 key_gen, key_acc, key_hutch1, key_hutch2
        o = (args.rtol, args.atol, args.mxstep)
        hutch = bool(args.hutchs)
        si, sf = {}, {}
        rp = replay or {}
        kw = dict(record=record, n_ts=int(args.n_ts), drop_jvp=drop_jvp)
        u0, vol0 = self.solve(prev.position, prng.normal_rows(kk[:, 3], d) if hutch else None, -1, *o, stats=si, replay=rp.get("inv"), **kw)   # :267
        up = u0 + (2.38 / np.sqrt(d)) * prng.normal_rows(kk[:, 0], d)                                   # :262,268
        xp, volp = self.solve(up, prng.normal_rows(kk[:, 2], d) if hutch else None, +1, *o, stats=sf, replay=rp.get("fwd"), **kw)            # :269
        lpn, gn = self.value_and_grad(xp, temper)                                                       # :270
        with np.errstate(over="ignore", invalid="ignore"):
            a = np.exp(lpn - volp - prev.logdensity - vol0)                                             # :271-274
            acc = prng.uniform_rows(kk[:, 1]) <= a                                                      # :275 (NaN: reject)
        m = acc[:, None]
        if stats is not None:
            stats.update(n_att_inv=si["n_attempted"], n_att_fwd=sf["n_attempted"], u0=u0, vol0=vol0, up=up, volp=volp,
                         log_alpha=lpn - volp - prev.logdensity - vol0, inv=si, fwd=sf)
        state = MALAState(np.where(m, xp, prev.position), np.where(acc, lpn, prev.logdensity), np.where(m, gn, prev.logdensity_grad))
        return state, MALAInfo(a, acc, xp, np.zeros_like(a))


# ---- sample-quality metrics (oracle/metrics.py, mcmc_utils.py:28-111): float64 pair sums in C ----------------------------------------
def stein_sums(X, G, beta=-0.5):
    """(sum over all ordered pairs of the Stein kernel term, sum of its i == j terms)."""
    X, G = _f64(X), _f64(G)
    n, d = X.shape
    assert G.shape == (n, d)
    tot, diag = C.c_double(0.0), C.c_double(0.0)
    assert lib().mfmref_stein_sums(_p(X), _p(G), n, d, C.c_double(beta), C.byref(tot), C.byref(diag)) == 0
    return tot.value, diag.value


def stein_disc(X, G, beta=-0.5):
    """(U-statistic, V-statistic) of ``metrics.stein_disc`` with the gradients ``G`` given."""
    tot, diag = stein_sums(X, G, beta)
    n = X.shape[0]
    return (tot - diag) / (n * (n - 1)), tot / n ** 2


def rbf_sum(A, B):
    A, B = _f64(A), _f64(B)
    assert A.shape[1] == B.shape[1]
    tot = C.c_double(0.0)
    assert lib().mfmref_rbf_sum(_p(A), A.shape[0], _p(B), B.shape[0], A.shape[1], C.byref(tot)) == 0
    return tot.value


def max_mean_disc(X, Y):
    """``metrics.max_mean_disc`` (both sample sets of m rows)."""
    m = X.shape[0]
    assert Y.shape[0] == m
    m2 = m * m
    return (rbf_sum(X, X) - m) / (m2 - m) - 2 * rbf_sum(X, Y) / m2 + (rbf_sum(Y, Y) - m) / (m2 - m)
