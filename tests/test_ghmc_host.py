"""Host-side tests of the GHMC / MEADS surface: the library's exports and signatures, what the header states, ``mfm_meads_plan``, the
command line's flags and the refusals raised before any device work (``--mcmc_kernel ghmc``)."""
import os

import numpy as np
import pytest

from oracle import loop

NAMES = ("mfm_ghmc_init", "mfm_ghmc_step", "mfm_ghmc_step_keys", "mfm_ghmc_run", "mfm_meads_warmup", "mfm_meads_plan")


def test_surface():
    import inspect
    from mfm_amd import _lib
    for name in NAMES:
        assert name in _lib.EXPORTS and name in _lib._SIGS, name
    n_args = {k: len(_lib._SIGS[k][1]) for k in NAMES}
    assert n_args == {"mfm_ghmc_init": 6, "mfm_ghmc_step": 16, "mfm_ghmc_step_keys": 15, "mfm_ghmc_run": 25, "mfm_meads_warmup": 22, "mfm_meads_plan": 4}
    lib = _lib.load()
    for name in NAMES:
        assert getattr(lib, name) is not None                          # the symbol resolves in the built library
    step = list(inspect.signature(_lib.Context.ghmc_step).parameters)
    assert step[:11] == ["self", "key", "beta", "step_size", "alpha", "delta", "pos", "logp", "grad", "momentum", "slice_"]
    run = list(inspect.signature(_lib.Context.ghmc_run).parameters)
    assert run[:12] == ["self", "key", "beta", "step_size", "alpha", "delta", "n_steps", "pos", "logp", "grad", "momentum", "slice_"]
    warm = list(inspect.signature(_lib.Context.meads_warmup).parameters)
    assert warm[:11] == ["self", "key", "beta", "step0", "alpha0", "n_iter", "pos", "logp", "grad", "momentum", "slice_"]
    from mfm_amd import bblackjax
    from mfm_amd.bblackjax.adaptation import meads_adaptation as A
    from mfm_amd.bblackjax.mcmc import ghmc as G
    assert bblackjax.ghmc is G.ghmc and bblackjax.meads_adaptation is A.meads_adaptation
    assert G.GHMCState._fields == ("position", "momentum", "logdensity", "logdensity_grad", "slice")
    assert G.GHMCInfo._fields == ("acceptance_rate", "is_accepted", "energy_change")
    assert G.GHMCRunInfo._fields[:5] == ("acceptance_rate", "num_accepted", "last", "positions", "logdensities")      # HMCRunInfo's shape
    assert G.check_parameters(0.1, 0.4, None) == (0.1, 0.4, 0.2) and G.check_parameters(0.1, 1.0, 0.0) == (0.1, 1.0, 0.0)
    for bad in ((0.0, 0.5, None), (np.inf, 0.5, None), (0.1, 0.0, None), (0.1, 1.01, None), (0.1, np.nan, None), (0.1, 0.5, -1e-9), (0.1, 0.5, np.nan)):
        with pytest.raises(ValueError, match="ghmc needs"):
            G.check_parameters(*bad)
    assert A.check_folds(32, 4) == 8
    for bad in ((32, 1), (30, 4), (4, 4)):
        with pytest.raises(ValueError):
            A.check_folds(*bad)


def test_the_header_declares_the_entry_points_and_states_the_transition():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mfm.h")).read()
    for name in NAMES:
        assert f"int {name}(" in text, name
    for phrase in ("p <- sqrt(1 - alpha) p + sqrt(alpha) n / sqrt(minv)", "s <- fmod(s + 1 + delta, 2) - 1", "accept iff |s| <= exp(-dH)",
                   "a NaN dH rejects", "s <- s exp(dH)", "p <- -p (the REFRESHED momentum", "H_0 = -logp + 1/2 sum_j minv_j p_j^2",
                   "mfm_hmc_set_inverse_mass is not read", "eps_f = min(1, 0.5 / sqrt(lam(Z)))", "max(1 / sqrt(lam(Y)), 1 / (t eps_f))",
                   "alpha_f = 1 - exp(-2 eps_f gamma_f)", "fold (f + 1) mod K", "keeps its previous ones", "t = n_iter + 1"):
        assert phrase in text, phrase


def test_meads_plan():
    from mfm_amd import _lib
    for n_valid, K, d in ((320, 4, 64), (32, 4, 65), (4096, 4, 256), (24, 4, 64), (16, 2, 2), (130, 2, 2048)):
        m, m_pad, d_pad, wg = _lib.meads_plan(n_valid, K, d)
        T = -(-(n_valid // K) // 64)
        assert (m, m_pad, d_pad, wg) == (n_valid // K, 64 * T, 32 * -(-d // 32), 2 * K * T * (T + 1) // 2)
    for bad, word in (((320, 1, 64), "n_folds"), ((321, 4, 64), "multiple of n_folds"), ((4, 4, 64), "multiple of n_folds"), ((320, 4, 0), "dim")):
        with pytest.raises(_lib.MfmError, match=word):
            _lib.meads_plan(*bad)


# ---- the command line ----
def _args(*flags, example="phi-four"):
    from mfm_amd import multi_modal as M
    return M.build_parser().parse_args(["--seed", "1", "--example", example, *flags])


def test_flags_parse_and_default():
    from mfm_amd import exe_flow_matching as E
    a = _args("--mcmc_kernel", "ghmc")
    assert (a.mcmc_kernel, a.ghmc_alpha, a.ghmc_delta, a.meads_folds, a.meads_shuffle) == ("ghmc", 0.5, None, 4, 0)
    assert E.ghmc_delta(a) == 0.25
    a = _args("--mcmc_kernel", "ghmc", "--ghmc_alpha", "0.2", "--ghmc_delta", "0.05", "--meads_folds", "8", "--meads_shuffle", "10", "--adapt_steps", "100")
    assert (a.ghmc_alpha, a.ghmc_delta, a.meads_folds, a.meads_shuffle, a.adapt_steps) == (0.2, 0.05, 8, 10, 100) and E.ghmc_delta(a) == 0.05
    assert E.ghmc_alpha(loop.default_args(mcmc_kernel="ghmc")) == 0.5           # (a namespace without the flag: the parser's default)


def test_check_args_serve_and_refuse():
    from mfm_amd import exe_flow_matching as E
    from mfm_amd.distributions import PhiFour
    dist = PhiFour(64)
    ok = loop.default_args(mcmc_kernel="ghmc", adapt_steps=50, num_chain=32, meads_folds=4)
    assert E.check_adapt_args(ok) == 50
    E.check_ghmc_args(dist, ok)
    E.check_ghmc_args(dist, loop.default_args(mcmc_kernel="ghmc", num_chain=30))                       # not adapting: any chain count
    E.check_ghmc_args(dist, loop.default_args(mcmc_kernel="mala", ghmc_alpha=7.0))                     # (another kernel does not read the flags)
    for kw, msg in ((dict(adapt_steps=8, adapt_mass=True), "--adapt_mass is not served with --mcmc_kernel ghmc"),
                    (dict(hmc_adapt="chees"), "--hmc_adapt chees is not served with --mcmc_kernel ghmc"),
                    (dict(nuts_adapt="tree"), "--nuts_adapt tree is not served with --mcmc_kernel ghmc"),
                    (dict(do_pt=True), "--do_pt is not served with --mcmc_kernel ghmc"),
                    (dict(adapt_steps=8, num_chain=30), r"num_chain \(30\) must be a multiple of --meads_folds"),
                    (dict(adapt_steps=8, num_chain=32, meads_folds=1), "must be a multiple of --meads_folds"),
                    (dict(adapt_steps=8, num_chain=4, meads_folds=4), "at least 2 chains per fold"),
                    (dict(ghmc_alpha=0.0), "alpha in"), (dict(ghmc_alpha=1.5), "alpha in"), (dict(ghmc_delta=-0.1), "delta >= 0"),
                    (dict(step_size=0.0), "step_size > 0"), (dict(meads_shuffle=-1), "--meads_shuffle must not be negative")):
        with pytest.raises(ValueError, match=msg):
            E.check_ghmc_args(dist, loop.default_args(mcmc_kernel="ghmc", **kw))
    with pytest.raises(ValueError, match="--adapt_steps needs --mcmc_kernel hmc"):                       # (unchanged for MALA)
        E.check_adapt_args(loop.default_args(mcmc_kernel="mala", adapt_steps=8))


REFUSED = ((["--mcmc_kernel", "ghmc", "--force_dim", "64"], "pines", "--mcmc_kernel ghmc is not served with --example pines"),
           (["--mcmc_kernel", "ghmc", "--adapt_steps", "8", "--adapt_mass"], "phi-four", "--adapt_mass is not served with --mcmc_kernel ghmc"),
           (["--mcmc_kernel", "ghmc", "--adapt_steps", "8", "--hmc_adapt", "chees"], "phi-four", "--hmc_adapt chees"),
           (["--mcmc_kernel", "ghmc", "--adapt_steps", "8", "--nuts_adapt", "tree"], "phi-four", "--nuts_adapt tree"),
           (["--mcmc_kernel", "ghmc", "--do_pt"], "phi-four", r"--do_pt takes --mcmc_kernel mala or hmc as the local move \(got ghmc"),
           (["--mcmc_kernel", "ghmc", "--adapt_steps", "8", "--force_num_chain", "30"], "phi-four", "must be a multiple of --meads_folds"))


@pytest.mark.parametrize("flags,example,msg", REFUSED)
def test_cli_refusals_before_any_device_work(flags, example, msg):
    from mfm_amd import multi_modal as M
    with pytest.raises(ValueError, match=msg):
        M.main(_args(*flags, example=example))


def test_the_python_kernel_refuses_the_cox_process_before_any_device_work():
    from mfm_amd.bblackjax import ghmc, meads_adaptation
    from mfm_amd.distributions import LogGaussianCoxPines
    cox = LogGaussianCoxPines(64)
    with pytest.raises(ValueError, match="ghmc is not served on the Cox process"):
        ghmc(cox.logprob, 0.1, 0.5)
    with pytest.raises(ValueError, match="ghmc is not served on the Cox process"):
        meads_adaptation(cox.logprob, 32)
