"""The cases of tests/test_gpu_pt.py and tests/test_pt_ref.py: ``mfm_pt_run`` / ``mfm_pt_exchange`` on the instances of their kernels,
with the float64 restatement (tests/pt_ref.py) of each.  A helper, not a test.

Start states as tests/chees_cases.py has them: chain b with sign s_b = +1, -1, ...; Dirichlet 0 on the chain: s_b sin(pi (j + 1) /
(d + 1)); periodic: the constant s_b; each plus (0.5 / d) N(0, 1) noise, rounded to float32; the 4-mode mixture starts chain b at mode
b % 4 plus N(0, 1) noise.  The two MAXIT 32 cases take start states and step sizes from tests/row_instance_cases.py.

``TOLERANCE[case]``: the bound of the GPU test's end-to-end comparison, per compared quantity (``QUANTITIES``) 4 x the largest
difference between the restatement and its ``float32_positions=True`` variant, relative to max(1, |value|); written from ``measure``
(run this module), and tests/test_pt_ref.py holds the recorded figures to the recomputation.  It also asserts what the GPU test relies
on: no local accept and no swap decision of any case has |u - p| < 1e-6.

``SAMPLING_SHARES``: slot 0's share of each of the four modes over the last 100 rounds of the sampling configuration (``sampling``),
from the restatement on the test's key and four others -- recorded by running this module."""
import functools

import numpy as np

from oracle import prng
from tests import pt_ref as pr, row_instance_cases as rc
from tests.phi4_bc_oracle import PhiFourBC

A, TBETA = 0.1, 20.0

# name: target, d, K temperatures, R ladders, padding rows (n_chain_local - K R; a context holds a multiple of 16 chains), kernel, leapfrog steps, n_local, rounds, betas, step sizes
CASES = {
    "gmm4": dict(target="gmm4", d=2, K=4, R=4, pad=0, kernel="hmc", L=3, n_local=2, n_rounds=6, betas=(1.0, 0.4, 0.15, 0.05), s=0.6),
    # odd K; K R = 15 of 16 rows: pairs straddle the workgroups of 4 chains; MALA under the textbook rule
    "phi4_d65": dict(target="d0", d=65, K=3, R=5, pad=1, kernel="mala", L=1, n_local=3, n_rounds=6, betas=(1.0, 0.9, 0.8), s=0.0008),
    # K = 2: the odd rounds have no pair at all
    "phi4_d256_pbc": dict(target="pbc", d=256, K=2, R=8, pad=0, kernel="hmc", L=2, n_local=2, n_rounds=5, betas=(1.0, 0.7), s=0.007),
    # MAXIT 16
    "phi4_d320": dict(target="d0", d=320, K=4, R=2, pad=8, kernel="hmc", L=3, n_local=2, n_rounds=4, betas=(1.0, 0.9, 0.8, 0.7), s=0.006),
    # MAXIT 32, BCRT false and true (start states and step sizes: tests/row_instance_cases.py)
    "d1025_d0": dict(target="rc", d=1025, K=2, R=2, pad=12, kernel="hmc", L=3, n_local=2, n_rounds=2, betas=(1.0, 0.95), s=None),
    "d2048_pbc": dict(target="rc", d=2048, K=2, R=2, pad=12, kernel="mala", L=1, n_local=2, n_rounds=2, betas=(1.0, 0.95), s=None),
    # K R < n_chain_local: the rows from K R on are never touched
    "padded": dict(target="d0", d=64, K=3, R=3, pad=7, kernel="hmc", L=2, n_local=2, n_rounds=4, betas=(1.0, 0.8, 0.6), s=0.03),
}

QUANTITIES = ("position", "logdensity", "logdensity_grad", "acc_sum", "swap_prob")

# case: per quantity 4 x the largest |float64 - float32 positions| / max(1, |value|) -- written from ``measure`` (run this module)
TOLERANCE = {
    "gmm4": (2.8e-07, 5.5e-07, 1.4e-06, 4.1e-07, 1.8e-06),
    "phi4_d65": (8.1e-07, 7.1e-07, 8.2e-05, 6.3e-06, 1.1e-06),
    "phi4_d256_pbc": (1.5e-06, 2.5e-06, 0.0011, 2.6e-05, 4.9e-06),
    "phi4_d320": (1.1e-06, 2e-06, 0.00065, 3.6e-05, 6.8e-06),
    "d1025_d0": (8.7e-07, 2e-06, 0.0028, 0.00015, 8e-08),
    "d2048_pbc": (6.6e-07, 2.9e-06, 0.0049, 0.001, 5.5e-06),
    "padded": (4.5e-07, 2.9e-07, 5.5e-05, 5.1e-06, 1.5e-06),
}

# key seed: slot 0's share of the modes 8 (1, 1), 8 (1, -1), 8 (-1, 1), 8 (-1, -1) -- written from ``sampling`` (run this module)
SAMPLING_KEY = 11
SAMPLING_SHARES = {
    11: (0.262, 0.287, 0.215, 0.236),   # swap rates [0.68, 0.69, 0.69, 0.7, 0.74, 0.75, 0.75]
    12: (0.268, 0.257, 0.219, 0.256),   # swap rates [0.68, 0.67, 0.68, 0.71, 0.74, 0.75, 0.74]
    13: (0.250, 0.235, 0.226, 0.289),   # swap rates [0.67, 0.69, 0.68, 0.69, 0.73, 0.76, 0.75]
    14: (0.269, 0.256, 0.206, 0.270),   # swap rates [0.68, 0.68, 0.71, 0.69, 0.73, 0.77, 0.77]
    15: (0.226, 0.245, 0.239, 0.290),   # swap rates [0.67, 0.67, 0.68, 0.7, 0.73, 0.75, 0.76]
}       # without exchange the share of mode 0 is 1.0 (key 11)


def n_chains(case):
    c = CASES[case]
    return c["K"] * c["R"] + c["pad"]


def dist(case):
    c = CASES[case]
    if c["target"] == "gmm4":
        return pr.LseMixture(8.0 * np.array([[1, 1], [1, -1], [-1, 1], [-1, -1.0]]), np.ones((4, 2)), np.ones(4) / 4)
    if c["target"] == "rc":
        return rc.oracle_dist(case)
    return PhiFourBC(c["d"], A, TBETA, ("pbc", 0.0) if c["target"] == "pbc" else ("dirichlet", 0.0))


def block(case):
    """The target block to hand ``set_target`` after the context's default, or None."""
    c = CASES[case]
    if c["target"] == "rc":
        return rc.block(case)
    return dist(case).block() if c["target"] == "pbc" else None


def betas(case):
    return np.array(CASES[case]["betas"], dtype=np.float64)


def step_sizes(case):
    """``s / sqrt(beta_k)``; the row-instance cases take ``s`` from tests/row_instance_cases.py: HMC its beta = 1 step size, MALA a quarter
    of its textbook-rule step size, which was chosen at beta = 0.37 (at this ladder's betas the full size accepts nothing)."""
    c = CASES[case]
    s = c["s"] if c["s"] is not None else (rc.STEP_SIZES[case]["hmc"]["b1"] if c["kernel"] == "hmc" else 0.25 * rc.STEP_SIZES[case]["mala"]["b037_textbook"])
    return s / np.sqrt(betas(case))


def start_state(case):
    """[n_chain_local, d] float32: the K R chains and the padding rows."""
    c = CASES[case]
    B, d = n_chains(case), c["d"]
    if c["target"] == "rc":
        return rc.start_state(case)[:B]
    noise = prng.normal_rows(prng.split(prng.PRNGKey(7100 + sorted(CASES).index(case)), B), d)
    if c["target"] == "gmm4":
        return (dist(case).modes[np.arange(B) % 4] + noise).astype(np.float32)
    sign = np.where(np.arange(B) % 2 == 0, 1.0, -1.0)[:, None]
    base = sign * (np.ones((1, d)) if c["target"] == "pbc" else np.sin(np.pi * (np.arange(d) + 1) / (d + 1))[None])
    return (base + 0.5 / d * noise).astype(np.float32)


def key(case):
    return prng.PRNGKey(9100 + sorted(CASES).index(case))


@functools.lru_cache(maxsize=None)
def reference(case, float32_positions=False):
    """The restatement's run of the case (computed once per process; the callers leave it unchanged).  The keys are split over
    n_chain_local chains, as the device's are."""
    c = CASES[case]
    KR = c["K"] * c["R"]
    x0 = start_state(case).astype(np.float64)
    return _run(case, x0[:KR], float32_positions)


def _run(case, x0, float32_positions):
    c = CASES[case]
    B = n_chains(case)
    d_, bs, es = dist(case), betas(case), step_sizes(case)
    st = pr.init(d_, bs, x0)
    replica = np.arange(x0.shape[0], dtype=np.int32)
    K, R = c["K"], c["R"]
    out = dict(n_acc=np.zeros(K * R, dtype=np.int32), acc_sum=np.zeros(K * R), swap_accepted=np.zeros((R, K - 1), dtype=np.int32),
               swap_prob=np.zeros((R, K - 1)), local=[], swaps=[], traj_pos=[], traj_logp=[])
    for t in range(c["n_rounds"]):
        km, ks = pr.round_keys(key(case), c["n_rounds"], t)
        st, rec = pr.local_steps(km, st, d_, bs, es, c["kernel"], c["L"], True, c["n_local"], n_total=B, float32_positions=float32_positions)
        out["n_acc"] += rec.accepted.sum(0).astype(np.int32)
        rs = np.zeros(K * R)
        for s in range(c["n_local"]):
            rs = rs + rec.p[s]
        out["acc_sum"] = out["acc_sum"] + rs
        st, replica, srec = pr.exchange(ks, st, d_, bs, R, t % 2, replica, n_total=B)
        out["swap_accepted"][srec.lower // K, srec.lower % K] += srec.accepted
        out["swap_prob"][srec.lower // K, srec.lower % K] += srec.p
        out["local"].append(rec); out["swaps"].append(srec)
        out["traj_pos"].append(st.position[::K].copy()); out["traj_logp"].append(st.logdensity[::K].copy())
    out.update(state=st, replica=replica, traj_pos=np.array(out["traj_pos"]), traj_logp=np.array(out["traj_logp"]))
    return out


def quantities(r):
    """The compared quantities of a run (the restatement's dict, or the device's with the same names)."""
    st = r["state"]
    return dict(position=st[0], logdensity=st[1], logdensity_grad=st[2], acc_sum=r["acc_sum"], swap_prob=r["swap_prob"])


def measure(case):
    """Per quantity 4 x the largest difference between the two variants, relative to max(1, |value|)."""
    a, b = quantities(reference(case, False)), quantities(reference(case, True))
    return tuple(float(4.0 * np.max(np.abs(a[q] - b[q]) / np.maximum(1.0, np.abs(a[q])))) for q in QUANTITIES)


def decisions_agree(case):
    """Whether the two variants made the same local and swap decisions (the tolerance means nothing otherwise)."""
    a, b = reference(case, False), reference(case, True)
    return (all((x.accepted == y.accepted).all() for x, y in zip(a["local"], b["local"]))
            and all((x.accepted == y.accepted).all() for x, y in zip(a["swaps"], b["swaps"])))


def margins(case):
    """The smallest |u - p| over the local steps and over the swap decisions of the case."""
    r = reference(case)
    loc = min(float(np.abs(rec.u - rec.p).min()) for rec in r["local"])
    sw = [float(np.abs(rec.u - rec.p).min()) for rec in r["swaps"] if rec.u.size]
    return loc, (min(sw) if sw else np.inf)


# ---- the sampling configuration --------------------------------------------------------------------------------------------------------
SAMPLING = dict(K=8, R=32, beta_min=0.01, L=4, s=0.25, n_local=4, n_rounds=200, last=100)


def sampling_setup(seed=SAMPLING_KEY):
    """``(dist, betas, step sizes, start positions [256, 2] float32, key)``: every chain starts at mode 0 + N(0, I)."""
    c = SAMPLING
    d_ = pr.LseMixture(8.0 * np.array([[1, 1], [1, -1], [-1, 1], [-1, -1.0]]), np.ones((4, 2)), np.ones(4) / 4)
    bs = np.exp(np.linspace(0.0, np.log(c["beta_min"]), c["K"]))
    bs[0] = 1.0
    B = c["K"] * c["R"]
    x0 = (d_.modes[0][None] + prng.normal_rows(prng.split(prng.PRNGKey(500), B), 2)).astype(np.float32)
    return d_, bs, c["s"] / np.sqrt(bs), x0, prng.PRNGKey(seed)


def mode_shares(traj_pos, modes):
    """The share of each mode among the rows of ``traj_pos [..., 2]`` (nearest mode)."""
    x = np.asarray(traj_pos, dtype=np.float64).reshape(-1, 2)
    near = ((x[:, None, :] - modes[None]) ** 2).sum(-1).argmin(1)
    return np.bincount(near, minlength=len(modes)) / x.shape[0]


def sampling(seed=SAMPLING_KEY, exchange=True):
    """The restatement on the sampling configuration: ``(shares of slot 0 over the last rounds, swap rates per pair)``."""
    c = SAMPLING
    d_, bs, es, x0, k = sampling_setup(seed)
    r = pr.pt_run(k, x0, d_, bs, es, c["R"], "hmc", c["L"], True, c["n_local"], c["n_rounds"], exchange_moves=exchange, thin=1)
    n_sweeps = np.array([len(range(kk % 2, c["n_rounds"], 2)) for kk in range(c["K"] - 1)])
    return mode_shares(r["traj_pos"][-c["last"]:], d_.modes), r["swap_accepted"].sum(0) / (c["R"] * n_sweeps)


if __name__ == "__main__":
    import sys
    if "sampling" not in sys.argv[1:]:
        for name in CASES:
            r = reference(name)
            print(name, "local accepted per round", [int(rec.accepted.sum()) for rec in r["local"]], "of", r["local"][0].accepted.size,
                  "swaps accepted per round", [f"{int(rec.accepted.sum())}/{rec.accepted.size}" for rec in r["swaps"]],
                  "margins (local, swap) %.3g %.3g" % margins(name), "same decisions in float32:", decisions_agree(name))
            print('    "%s": (%s),' % (name, ", ".join("%.2g" % v for v in measure(name))), flush=True)
    else:
        for seed in (SAMPLING_KEY, 12, 13, 14, 15):
            sh, rates = sampling(seed)
            print("    %d: (%s),   # swap rates %s" % (seed, ", ".join("%.3f" % v for v in sh), np.round(rates, 2).tolist()), flush=True)
        print("without exchange, mode 0:", sampling(SAMPLING_KEY, False)[0][0])
