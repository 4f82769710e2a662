"""Optimizer descriptors for ``bblackjax.vi.svgd`` on MI355X: the three optax optimizers the reference's users hand to ``svgd``
(``sgd``, ``adagrad``, ``adam``) here, and ``cocob`` in the submodule ``optimizers.cocob`` (the reference's ``bblackjax/optimizers/cocob.py``:
``from mfm_amd.bblackjax.optimizers.cocob import cocob``).

The reference passes an ``optax.GradientTransformation`` (two Python closures); closures cannot cross the C ABI, so each constructor
returns an :class:`Optimizer` descriptor -- kind, hyper-parameters and ``init(particles) -> opt_state`` -- and the update runs on the
device (``mfm_svgd_apply``; the formulas stand in ``include/mfm.h``).  ``opt_state`` is ``(state tensors ..., count)``: float32 device
tensors of the particles' shape and the number of updates applied.  ``sgd`` / ``adagrad`` / ``adam`` restate optax 0.1.9's published
formulas (optax is third-party; parity with optax itself is not pinned by a test).
"""
from typing import Callable, NamedTuple, Tuple

__all__ = ["Optimizer", "sgd", "adagrad", "adam", "check_optimizer", "KINDS", "cocob"]

KINDS = ("sgd", "adagrad", "adam", "cocob")


class Optimizer(NamedTuple):
    kind: str
    hyper: Tuple[float, ...]
    init: Callable


def state_init(fills):
    """``init(particles)`` for state arrays filled with the given constants (``None``: a copy of the particles)."""
    def init(particles):
        import torch
        return tuple(particles.clone() if f is None else torch.full_like(particles, f) for f in fills) + (0,)
    return init


def sgd(learning_rate):
    return Optimizer("sgd", (float(learning_rate),), state_init(()))


def adagrad(learning_rate, initial_accumulator_value=0.1, eps=1e-7):
    return Optimizer("adagrad", (float(learning_rate), float(initial_accumulator_value), float(eps)), state_init((float(initial_accumulator_value),)))


def adam(learning_rate, b1=0.9, b2=0.999, eps=1e-8):
    return Optimizer("adam", (float(learning_rate), float(b1), float(b2), float(eps)), state_init((0.0, 0.0)))


def check_optimizer(optimizer):
    if not isinstance(optimizer, Optimizer) or optimizer.kind not in KINDS:
        raise TypeError("optimizer must be one of mfm_amd.bblackjax.optimizers' sgd(...), adagrad(...), adam(...) or optimizers.cocob's cocob(...) "
                        f"(the update runs on the device; got {type(optimizer).__name__})")
    return optimizer


from . import cocob  # noqa: E402,F401  (the submodule; its constructor is cocob.cocob)
