"""The COCOB optimizer as a descriptor for ``bblackjax.vi.svgd`` -- drop-in for ``bblackjax/optimizers/cocob.py``.

``cocob(alpha, eps)`` restates ``cocob.py:18-88`` with its five state arrays ``(init_particles, cumulative_gradients, scale,
subgradients, reward)`` (``:10-15``, created as in ``:37-50``); the update runs on the device (``mfm_svgd_apply``, kind
``MFM_SVGD_COCOB``).  What a descriptor is: the package docstring.
"""
from . import Optimizer, state_init

__all__ = ["cocob"]


def cocob(alpha: float = 100, eps: float = 1e-8):
    """The parameter-free COntinuous COin Betting optimizer (``cocob.py:18``; Orabona & Tommasi 2017, algorithm 2)."""
    return Optimizer("cocob", (float(alpha), float(eps)), state_init((None, 0.0, float(eps), 0.0, 0.0)))
