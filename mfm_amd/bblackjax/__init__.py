"""Kernel API of the reference's vendored ``bblackjax`` on MI355X: ``mcmc`` (MALA -- the MFM hot path, SURVEY.md section 8a M1-M4 -- and
the build-side HMC / NUTS / MCLMC / GHMC), ``adaptation``, ``smc``, and ``vi`` / ``optimizers`` (Stein variational gradient descent and its optimizers)."""
from .mcmc.mala import mala  # noqa: F401
from .mcmc.mclmc import mclmc  # noqa: F401
from .mcmc.ghmc import ghmc  # noqa: F401
from .adaptation.mclmc_adaptation import mclmc_find_L_and_step_size  # noqa: F401
from .adaptation.meads_adaptation import meads_adaptation  # noqa: F401
