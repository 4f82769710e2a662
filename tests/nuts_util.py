"""Helpers shared by the No-U-turn tests (tests/test_gpu_nuts.py, tests/test_gpu_nuts_instances.py, tests/test_nuts_cases.py and the
warmup's): a case's oracle and context, the reference's burned-in start, the borderline rule and the comparison of one transition of
the kernel with tests/nuts_ref.py.  Not a test.  The rule and the bounds are described in tests/test_gpu_nuts.py's docstring.

A case's target is ``(kind, d, tail)``: ``kind`` "phi4" / "gmm4" / "gmm16"; ``tail`` None for the default phi-four chain, otherwise what
follows ``{a, beta}`` in the C ABI's target block, ``(periodic, b)`` for the chain and ``(periodic, b, 2.0)`` for the L x L lattice
(tests/phi4_bc_oracle.py, tests/phi4_2d_oracle.py: ``block()``)."""
import functools

import numpy as np

from oracle import mala as omala, prng, targets
from tests import hmc_mass_ref as hm, nuts_ref as nr

B, DEPTH, BURN, N_TRANS = 64, 6, 30, 3
INFO = ("depth", "num_leapfrog", "is_turning", "is_divergent", "acceptance_rate", "energy")
PROBE_REL, PROBE_SEED = 2.0 ** -22, 7          # the gradient perturbation of position_probe


def _setup(kind, d, tail, n=B):
    """The oracle's arguments and target for a case: ``(args, the default target of the setup, the case's oracle target)``."""
    from tests import gpu_util as gu
    if kind == "phi4":
        args, dist, *_ = gu.phi4_setup(d=d, B=n, hidden=32, F=16)
        if tail is not None:
            from tests.phi4_2d_oracle import PhiFour2D
            from tests.phi4_bc_oracle import PhiFourBC
            bc = ("pbc", 0.0) if tail[0] else ("dirichlet", float(tail[1]))
            odist = (PhiFour2D if len(tail) > 2 and tail[2] == 2 else PhiFourBC)(d, dist.a, dist.beta, bc)
            odist.init_params = dist.init_params
            assert list(odist.block()[2:]) == [float(v) for v in tail]
            return args, dist, odist
        return args, dist, dist
    args, dist, *_ = gu.gmm4_setup(B=n) if kind == "gmm4" else gu.gmm16_setup(B=n, hidden=32, F=16)
    return args, dist, dist


def _ctx(kind, d, tail, n=B):
    import torch
    from mfm_amd import _lib
    from tests import gpu_util as gu
    args, dist, odist = _setup(kind, d, tail, n)
    ctx = gu.make_ctx(dist, args)
    if tail is not None:
        ctx.set_target(_lib.PHI4, odist.block())
    return ctx, torch.as_tensor(dist.init_params.astype(np.float32)).cuda(), odist


def _tol_e(kind, logp):
    return 5e-6 * max(1.0, np.abs(logp).max()) + (5e-4 if kind.startswith("gmm") else 0.0)


def _borderline(kind, logp, info):
    t = 10 * _tol_e(kind, logp)
    return (info.margin_draw < t) | (info.margin_div < t) | (info.margin_turn < 1e-4)


def _ref_state(vg, x32):
    lp, g = vg(x32.astype(np.float64))
    return omala.MALAState(x32.astype(np.float64), lp, g.astype(np.float32).astype(np.float64))


@functools.lru_cache(maxsize=None)
def burned(kind, d, tail, eps, depth, mass):
    """A case's start: the reference's own state after BURN transitions (``max_tree_depth`` DEPTH) from the initial draw, and the
    reference-only pass of N_TRANS transitions under the limit ``depth`` from it: the share of borderline chains in each, the infos, and
    the state each transition started from.  ``tail`` a tuple or None.  Computed once per process; nothing returned may be modified."""
    _, dist, odist = _setup(kind, d, tail)
    vg = targets.Tempered(odist, 1.0).value_and_grad
    minv = hm.log_spaced_mass(d) if mass else None
    st = _ref_state(vg, dist.init_params.astype(np.float32))
    burn_divergent = 0
    for it in range(BURN):
        st, info = nr.kernel(prng.split(prng.PRNGKey(900 + it), B), st, vg, eps, DEPTH, inverse_mass=minv)
        burn_divergent += int(info.is_divergent.sum())
    start = st.position.astype(np.float32)
    shares, infos, states = [], [], []
    for it in range(N_TRANS):
        st_n, info = nr.kernel(prng.split(prng.PRNGKey(50 + it), B), st, vg, eps, depth, inverse_mass=minv)
        shares.append(_borderline(kind, st.logdensity, info).mean())
        infos.append(info)
        states.append((st, st_n))
        st = st_n
    return dict(start=start, minv=minv, shares=shares, infos=infos, states=states, burn_divergent=burn_divergent)


@functools.lru_cache(maxsize=None)
def position_probe(kind, d, tail, eps, depth, mass):
    """How far a last-place change of the float32 gradient moves a transition's end, on the reference alone: every transition of
    ``burned``'s pass is repeated from the same state and keys with the float32-rounded gradient of every leaf scaled by
    ``1 +- PROBE_REL`` (signs from ``default_rng(PROBE_SEED)``).  Returns ``(displacement, changed)``: the largest |position difference|
    over the chains that are not borderline and whose depth and leapfrog count are unchanged, and how many non-borderline chains
    changed either."""
    ref = burned(kind, d, tail, eps, depth, mass)
    _, _, odist = _setup(kind, d, tail)
    vg = targets.Tempered(odist, 1.0).value_and_grad
    rng = np.random.default_rng(PROBE_SEED)

    def noisy(x):
        lp, g = vg(x)
        g32 = np.asarray(g, dtype=np.float64).astype(np.float32).astype(np.float64)
        return lp, g32 * (1.0 + PROBE_REL * rng.choice([-1.0, 1.0], size=g32.shape))

    disp, changed = 0.0, 0
    for it, ((st, st_n), info) in enumerate(zip(ref["states"], ref["infos"])):
        st_p, info_p = nr.kernel(prng.split(prng.PRNGKey(50 + it), B), st, noisy, eps, depth, inverse_mass=ref["minv"])
        ok = ~_borderline(kind, st.logdensity, info)
        same = (info_p.depth == info.depth) & (info_p.num_leapfrog == info.num_leapfrog)
        changed += int((ok & ~same).sum())
        if (ok & same).any():
            disp = max(disp, np.abs(st_p.position - st_n.position)[ok & same].max())
    return disp, changed


def _dev_info(n):
    import torch
    return dict(depth=torch.empty(n, dtype=torch.int32, device="cuda"), num_leapfrog=torch.empty(n, dtype=torch.int32, device="cuda"),
                is_turning=torch.empty(n, dtype=torch.uint8, device="cuda"), is_divergent=torch.empty(n, dtype=torch.uint8, device="cuda"),
                acceptance_rate=torch.empty(n, dtype=torch.float64, device="cuda"), energy=torch.empty(n, dtype=torch.float64, device="cuda"))


def _init(ctx, pos0):
    import torch
    pos = pos0.clone()
    logp = torch.empty(pos.shape[0], dtype=torch.float64, device="cuda"); grad = torch.empty_like(pos)
    ctx.mala_init(pos, 1.0, logp, grad)
    return pos, logp, grad


def _keys_dev(keys):
    import torch
    return torch.as_tensor(np.ascontiguousarray(keys, dtype=np.uint32).view(np.int32)).cuda()


def _compare(kind, st, info, state_g, info_g, ok, what, pos_floor=0.0):
    """The kernel's transition against the reference's on the chains ``ok``.  ``pos_floor``: a case's own position bound where it is
    above the common one (tests/nuts_cases.py).  Returns the largest position, log-density and rate differences."""
    pos_g, logp_g = state_g[0].cpu().numpy().astype(np.float64), state_g[1].cpu().numpy()
    g = {k: v.cpu().numpy() for k, v in info_g.items()}
    tol = _tol_e(kind, st.logdensity)
    pos_tol = max(3e-6 * max(1.0, np.abs(st.position).max()), pos_floor)
    diffs = (np.abs(pos_g - st.position)[ok].max(), np.abs(logp_g - st.logdensity)[ok].max(), np.abs(g["acceptance_rate"] - info.acceptance_rate)[ok].max())
    print(f"{what}: {ok.sum()} of {ok.size} chains compared; depths {np.bincount(info.depth)}; leapfrog mean {info.num_leapfrog.mean():.1f}; "
          f"turning {info.is_turning.sum()} divergent {info.is_divergent.sum()} stopped in a subtree {info.stopped_in_subtree.sum()}; "
          f"max |pos diff| {diffs[0]:.2e} (bound {pos_tol:.2e}) max |logp diff| {diffs[1]:.2e} "
          f"max |rate diff| {diffs[2]:.2e} tol_e {tol:.2e}")
    np.testing.assert_array_equal(g["depth"][ok], info.depth[ok], err_msg=what)
    np.testing.assert_array_equal(g["num_leapfrog"][ok], info.num_leapfrog[ok], err_msg=what)
    np.testing.assert_array_equal(g["is_turning"][ok].astype(bool), info.is_turning[ok], err_msg=what)
    np.testing.assert_array_equal(g["is_divergent"][ok].astype(bool), info.is_divergent[ok], err_msg=what)
    assert diffs[0] < pos_tol, what
    lp_tol = 2e-6 * max(1.0, np.abs(st.logdensity).max()) + (5e-4 if kind.startswith("gmm") else 0.0)
    assert diffs[1] < lp_tol, what
    assert diffs[2] < tol, what
    assert np.abs(g["energy"] - info.energy)[ok].max() < tol + lp_tol, what
    return diffs


def _transitions_against_the_reference(kind, d, tail, eps, depth, minv, start, what, pos_floor=0.0):
    """N_TRANS transitions of ``nuts_step`` from ``start`` on keys 50 + it, each compared with ``nr.kernel`` on the same keys over the
    non-borderline chains; both sides continue from the KERNEL's state (a borderline tree must not cascade).  Returns the largest
    position, log-density and rate differences."""
    import torch
    ctx, _, odist = _ctx(kind, d, tail)
    ctx.set_inverse_mass(minv)
    vg = targets.Tempered(odist, 1.0).value_and_grad
    pos, logp, grad = _init(ctx, torch.as_tensor(start).cuda())
    buf = _dev_info(B)
    st = omala.MALAState(pos.cpu().numpy().astype(np.float64), logp.cpu().numpy(), grad.cpu().numpy().astype(np.float64))
    worst = np.zeros(3)
    for it in range(N_TRANS):
        key = prng.PRNGKey(50 + it)
        ctx.nuts_step(key, 1.0, eps, depth, pos, logp, grad, **buf)
        st_o, info = nr.kernel(prng.split(key, B), st, vg, eps, depth, inverse_mass=minv)
        border = _borderline(kind, st.logdensity, info)
        assert border.mean() <= 0.25, (it, border.mean())
        worst = np.maximum(worst, _compare(kind, st_o, info, (pos, logp), buf, ~border, f"{what} transition {it}", pos_floor))
        st = omala.MALAState(pos.cpu().numpy().astype(np.float64), logp.cpu().numpy(), grad.cpu().numpy().astype(np.float64))
    ctx.close()
    return worst


# ---- device only ------------------------------------------------------------------------------------------------------------
def _stepwise(ctx, state0, key, eps, n_steps, depth):
    from mfm_amd import random as jr
    pos, logp, grad = (t.clone() for t in state0)
    buf = _dev_info(pos.shape[0])
    per_chain = np.ndim(key) == 2
    step_keys = jr.split_rows(key, n_steps) if per_chain else jr.split(key, n_steps)
    out = {k: [] for k in ("pos", "logp", "grad") + INFO}
    for j in range(n_steps):
        if per_chain:
            ctx.nuts_step_keys(_keys_dev(step_keys[:, j]), 1.0, eps, depth, pos, logp, grad, **buf)
        else:
            ctx.nuts_step(step_keys[j], 1.0, eps, depth, pos, logp, grad, **buf)
        for name, t in zip(out, (pos, logp, grad) + tuple(buf[k] for k in INFO)):
            out[name].append(t.cpu().numpy().copy())
    return {k: np.stack(v) for k, v in out.items()}


def _run(ctx, state0, key, eps, n_steps, depth, thin=1):
    import torch
    pos, logp, grad = (t.clone() for t in state0)
    n, d = pos.shape
    buf = _dev_info(n)
    tot = dict(leapfrog_sum=torch.empty(n, dtype=torch.int64, device="cuda"), acc_sum=torch.empty(n, dtype=torch.float64, device="cuda"),
               n_divergent=torch.empty(n, dtype=torch.int32, device="cuda"), depth_sum=torch.empty(n, dtype=torch.int32, device="cuda"))
    tp = torch.empty(n_steps // thin, n, d, device="cuda"); tl = torch.empty(n_steps // thin, n, dtype=torch.float64, device="cuda")
    ctx.nuts_run(_keys_dev(key) if np.ndim(key) == 2 else key, 1.0, eps, depth, n_steps, pos, logp, grad, thin=thin, traj_pos=tp, traj_logp=tl, **tot, **buf)
    out = dict(pos=pos, logp=logp, grad=grad, traj_pos=tp, traj_logp=tl, **tot, **buf)
    return {k: v.cpu().numpy() for k, v in out.items()}
