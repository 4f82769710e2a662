"""The phi-four target on an L x L lattice (dim_phys = 2), in float64 for the tests.  A build-side definition (the reference's main
script builds the chain only; its ``PhiFourBase`` has the ``dim_phys == 2`` field, distributions.py:168-211):

A row x of length d = L * L is the field in row-major order, site (r, c) = element r L + c.  coef = a * L (the grid side where the
chain has ``dim``).  V = sum (1 - x^2)^2 / (4 coef) as on the chain; U = coef / 2 * sum over the bonds of BOTH axes of (dx)^2:
``bc=('pbc', .)`` wraps both axes (2 L^2 bonds, the value is unused), ``bc=('dirichlet', b)`` surrounds the lattice by a frame held
at b -- every row and every column is a Dirichlet chain of L + 1 bonds, 2 L (L + 1) in all.  loglik = -beta (U + V), logprior = 0.
The Hessian-vector product's stencil sees 0 beyond a Dirichlet edge (whatever b is) and wraps under periodic boundaries.

A subclass of ``tests.phi4_bc_oracle.PhiFourBC`` (so of ``oracle.targets.PhiFour``): ``oracle.mala``, ``oracle.hmc``, ``oracle.flow``,
``oracle.vfield``, ``oracle.fm`` and ``oracle.loop`` take it as their ``dist`` unchanged."""
import math

import numpy as np

from tests.phi4_bc_oracle import PhiFourBC


class PhiFour2D(PhiFourBC):
    def __init__(self, dim, a=0.1, beta=20.0, bc=("dirichlet", 0.0)):
        super().__init__(dim, a, beta, bc)
        self.L = math.isqrt(self.dim)
        if self.L * self.L != self.dim:
            raise ValueError(f"dim = {dim} is not a square")
        self.coef = a * self.L

    def block(self):
        """The C ABI's target block: {a, beta, kind, b, dim_phys}."""
        return super().block() + [2.0]

    def _field(self, x):
        x = np.asarray(x, np.float64)
        return x.reshape(x.shape[0], self.L, self.L)

    def _framed(self, f, edge):
        return np.pad(f, ((0, 0), (1, 1), (1, 1)), constant_values=edge)

    def _nbsum(self, x, edge):
        """Sum of the four neighbours of every site, [B, d]; ``edge`` = the value beyond a Dirichlet edge."""
        f = self._field(x)
        if self.periodic:
            s = np.roll(f, 1, 1) + np.roll(f, -1, 1) + np.roll(f, 1, 2) + np.roll(f, -1, 2)
        else:
            p = self._framed(f, edge)
            s = p[:, :-2, 1:-1] + p[:, 2:, 1:-1] + p[:, 1:-1, :-2] + p[:, 1:-1, 2:]
        return s.reshape(f.shape[0], -1)

    def bonds(self, x):
        """Sum over all bonds of (dx)^2, [B]."""
        f = self._field(x)
        if self.periodic:
            dr, dc = f - np.roll(f, 1, 1), f - np.roll(f, 1, 2)              # L^2 bonds per axis
        else:
            p = self._framed(f, self.bc[1])
            dr = p[:, 1:, 1:-1] - p[:, :-1, 1:-1]                            # (L + 1) x L bonds along the columns
            dc = p[:, 1:-1, 1:] - p[:, 1:-1, :-1]                            # L x (L + 1) bonds along the rows
        return (dr * dr).sum((1, 2)) + (dc * dc).sum((1, 2))

    def loglik(self, x):
        x = np.asarray(x, np.float64)
        U = self.bonds(x) / 2.0 * self.coef
        q = 1.0 - x * x
        V = (q * q).sum(1) / 4.0 / self.coef
        return -self.beta * (U + V)

    def grad_loglik(self, x):
        x = np.asarray(x, np.float64)
        return -self.beta * (self.coef * (4.0 * x - self._nbsum(x, self.bc[1])) - x * (1.0 - x * x) / self.coef)

    def grad_logprob(self, x):
        return self.grad_loglik(x)

    def hvp_logprob(self, x, v):
        x, v = np.asarray(x, np.float64), np.asarray(v, np.float64)
        return -self.beta * (self.coef * (4.0 * v - self._nbsum(v, 0.0)) - (1.0 - 3.0 * x * x) * v / self.coef)

    def hess_diag(self, x):
        return -self.beta * (4.0 * self.coef - (1.0 - 3.0 * x * x) / self.coef)
