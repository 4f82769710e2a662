"""The phi-four target with the reference's other boundaries (distributions.py:114-165), restated in float64 for the tests.

``bc=('dirichlet', b)``: both ends held at b, d + 1 bonds including (x_0 - b) and (b - x_{d-1}).
``bc=('pbc', .)``: a periodic ring, d bonds, the last one x_0 - x_{d-1} (``jnp.pad(x, (1, 0), mode='wrap')``); the value is unused.
The Hessian-vector product's stencil sees 0 beyond a Dirichlet end (whatever b is) and wraps under periodic boundaries.

A subclass of ``oracle.targets.PhiFour``, so ``oracle.flow``, ``oracle.vfield``, ``oracle.hmc`` and ``oracle.loop`` take it as their
``dist``; with Dirichlet 0 it computes exactly what the parent does."""
import numpy as np

from oracle import targets


class PhiFourBC(targets.PhiFour):
    def __init__(self, dim, a=0.1, beta=20.0, bc=("dirichlet", 0.0)):
        super().__init__(dim, a, beta)
        if bc[0] not in ("dirichlet", "pbc"):
            raise ValueError(bc[0])
        self.bc = (bc[0], float(bc[1]) if bc[0] == "dirichlet" else 0.0)

    @property
    def periodic(self):
        return self.bc[0] == "pbc"

    def block(self):
        """The C ABI's target block for this boundary."""
        return [self.a, self.beta, 1.0 if self.periodic else 0.0, self.bc[1]]

    def _neighbours(self, x, edge):
        """(left, right) neighbour arrays of every element; ``edge`` = the value beyond a Dirichlet end."""
        if self.periodic:
            return np.roll(x, 1, axis=1), np.roll(x, -1, axis=1)
        e = np.full((x.shape[0], 1), edge)
        return np.concatenate([e, x[:, :-1]], 1), np.concatenate([x[:, 1:], e], 1)

    def loglik(self, x):
        x = np.asarray(x, np.float64)
        if self.periodic:
            diffs = x - np.roll(x, 1, axis=1)                                # d bonds
        else:
            b = self.bc[1]
            e = np.full((x.shape[0], 1), b)
            xp = np.concatenate([e, x, e], 1)
            diffs = xp[:, 1:] - xp[:, :-1]                                   # d + 1 bonds
        U = (diffs * diffs).sum(1) / 2.0 * self.coef
        q = 1.0 - x * x
        V = (q * q).sum(1) / 4.0 / self.coef
        return -self.beta * (U + V)

    def grad_loglik(self, x):
        x = np.asarray(x, np.float64)
        l, r = self._neighbours(x, self.bc[1])
        return -self.beta * (self.coef * (2.0 * x - l - r) - x * (1.0 - x * x) / self.coef)

    def grad_logprob(self, x):
        return self.grad_loglik(x)

    def hvp_logprob(self, x, v):
        x, v = np.asarray(x, np.float64), np.asarray(v, np.float64)
        l, r = self._neighbours(v, 0.0)
        return -self.beta * (self.coef * (2.0 * v - l - r) - (1.0 - 3.0 * x * x) * v / self.coef)
