"""Float64 numpy restatement of Stein variational gradient descent -- the reference the SVGD tests compare with (a helper, not a test).

Restates ``bblackjax/vi/svgd.py`` and ``bblackjax/optimizers/cocob.py`` of the reference (lines cited as ``oracle/`` does).  ``sgd``,
``adagrad`` and ``adam`` are optax's (0.1.9) published formulas: optax is third-party and not installed here, so their parity with
optax itself is unpinned, as for AdamW in ``oracle/optim.py``.
"""
import numpy as np


def sqdist(x):
    """``D_ij = |x_i - x_j|^2``, the direct form (svgd.py:95, :102-106), in float64."""
    x = np.asarray(x, dtype=np.float64)
    diff = x[:, None, :] - x[None, :, :]
    return (diff * diff).sum(-1)


def length_scale(D):
    """svgd.py:106-111: the median of the distances below the main diagonal, squared, over log n (``np.median``: the mean of the two
    middle values of an even count, as ``jnp.median``)."""
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[0]
    dist = np.sqrt(D[np.tril_indices(n, -1)])
    return float(np.median(dist)) ** 2 / np.log(n)


def functional_gradient(x, g, h, sqdist=None):
    """svgd.py:74-84 with ``k_ij = exp(-|x_i - x_j|^2 / h)`` (:94-96).  ``phi_star_summand(p, p_)`` is ``-k(p, p_) g(p) - d/dp k(p, p_)``
    and the mean runs over ``p``; with ``d/dp k(p, p_) = -(2/h) k (p - p_)`` the functional gradient at ``x_i = p_`` is
    ``fg_i = -(1/n) sum_j [k_ij g_j + (2/h) k_ij (x_i - x_j)] = -(1/n) [ (K G)_i + (2/h) (s_i x_i - (K X)_i) ]``, ``s_i = sum_j k_ij``.
    ``sqdist``: squared distances to use instead of this module's (a test feeds the device's own)."""
    x, g = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64)
    n = x.shape[0]
    D = globals()["sqdist"](x) if sqdist is None else np.asarray(sqdist, dtype=np.float64)
    K = np.exp(-(1.0 / h) * D)
    s = K.sum(1)
    return -(K @ g + (2.0 / h) * (s[:, None] * x - K @ x)) / n


def gradient_terms(x, g, h, sqdist):
    """max |K G|, max |s xc|, max |K Xc| on centred coordinates: the scale of the gradient test's tolerance."""
    x, g = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64)
    xc = x - x.mean(0)
    K = np.exp(-(1.0 / h) * np.asarray(sqdist, dtype=np.float64))
    return np.abs(K @ g).max(), np.abs(K.sum(1)[:, None] * xc).max(), np.abs(K @ xc).max()


# ---- optimizers: init(particles) -> state (tuple of arrays), update(fg, state, particles, count) -> (updates, state) ---------------
class sgd:
    def __init__(self, learning_rate):
        self.lr = float(learning_rate)

    def init(self, p):
        return ()

    def update(self, fg, state, p, count):
        return -self.lr * fg, ()


class adagrad:
    """optax 0.1.9: ``scale_by_rss(initial_accumulator_value, eps)`` then ``scale(-learning_rate)``."""

    def __init__(self, learning_rate, initial_accumulator_value=0.1, eps=1e-7):
        self.lr, self.init_acc, self.eps = float(learning_rate), float(initial_accumulator_value), float(eps)

    def init(self, p):
        return (np.full(np.shape(p), self.init_acc, dtype=np.float64),)

    def update(self, fg, state, p, count):
        acc = state[0] + fg * fg
        scale = np.where(acc > 0, 1.0 / np.sqrt(acc + self.eps), 0.0)
        return -self.lr * fg * scale, (acc,)


class adam:
    """optax.adam: bias-corrected moments, eps outside the square root (eps_root = 0)."""

    def __init__(self, learning_rate, b1=0.9, b2=0.999, eps=1e-8):
        self.lr, self.b1, self.b2, self.eps = float(learning_rate), float(b1), float(b2), float(eps)

    def init(self, p):
        return (np.zeros(np.shape(p)), np.zeros(np.shape(p)))

    def update(self, fg, state, p, count):
        m = self.b1 * state[0] + (1 - self.b1) * fg
        v = self.b2 * state[1] + (1 - self.b2) * fg * fg
        t = count + 1
        mh, vh = m / (1 - self.b1 ** t), v / (1 - self.b2 ** t)
        return -self.lr * mh / (np.sqrt(vh) + self.eps), (m, v)


class cocob:
    """cocob.py:18-88; state = (init_particles, cumulative_gradients, scale, subgradients, reward) (:10-15, :37-50)."""

    def __init__(self, alpha=100, eps=1e-8):
        self.alpha, self.eps = float(alpha), float(eps)

    def init(self, p):
        p = np.asarray(p, dtype=np.float64)
        z = np.zeros(p.shape)
        return (p.copy(), z.copy(), self.eps * np.ones(p.shape), z.copy(), z.copy())

    def update(self, fg, state, p, count):
        p0, C, L, G, R = state
        L = np.maximum(L, np.abs(fg))                                  # :55-57
        G = G + np.abs(fg)                                             # :58-60
        R = np.maximum(R - fg * (p - p0), 0)                           # :61-67
        C = C - fg                                                     # :68-70
        upd = -p + (p0 + C / (L * np.maximum(G + L, self.alpha * L)) * (L + R))      # :72-81
        return upd, (p0, C, L, G, R)


def step(x, grad_fn, h, optimizer, opt_state, count, update_median=True, sqdist_old=None):
    """One iteration (svgd.py:164-166): the kernel step (:71-89), then the median heuristic on the NEW particles.  ``grad_fn(x) -> g``.
    Returns ``(x_new, h_new, opt_state, fg)``."""
    x = np.asarray(x, dtype=np.float64)
    fg = functional_gradient(x, grad_fn(x), h, sqdist=sqdist_old)
    upd, opt_state = optimizer.update(fg, opt_state, x, count)
    x_new = x + upd
    h_new = length_scale(sqdist(x_new)) if update_median else h
    return x_new, h_new, opt_state, fg
