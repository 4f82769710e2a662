"""The cases of tests/test_gpu_mcmc_bits.py and tools/make_mcmc_bits.py: every sampler kernel that goes through mcmc.hip.h, at the
smallest shapes at which each of its forms can go wrong, three consecutive steps each, in two variants (beta = 1 as written;
beta = 0.37 with the textbook rule -- beta < 1 is where multiply-add contraction showed).  ``record`` runs one case on the device and
returns its buffers; the fixture holds, per buffer and step, the SHA-256 of its raw bytes and the per-chain buffers themselves (first
16 rows) -- a fixture of a few tens of KB does not admit the [B, d] buffers, and equal digests are equal bytes.  A case of fewer than
16 chains runs as the library runs such a shard: one 16-row tile whose padding rows repeat the last chain, all 16 rows recorded.

Step sizes: chosen with the float64 oracle (``oracle_accepts`` below, on a CPU) so that the three steps of every case accept some
proposals and reject others; the recorder asserts that of the device's own decisions."""
import hashlib

import numpy as np

from oracle import hmc as ohmc, mala as omala, prng, targets

N_STEPS = 3
ROWS = 16                                           # rows of a buffer kept as an array
VARIANTS = {"b1": (1.0, False), "b037_textbook": (0.37, True)}

# name: (kind, target, d, chains, phi-four block tail or None, kernel family or None, {variant: step size})
CASES = {
    "mala_phi4_d100": ("mala", "phi4", 100, 8, None, None, {"b1": 1e-05, "b037_textbook": 0.00715}),
    "mala_phi4_d40": ("mala", "phi4", 40, 4, None, None, {"b1": 0.0001, "b037_textbook": 0.018}),
    "mala_phi4_d100_pbc": ("mala", "phi4", 100, 8, [1.0, 0.0], None, {"b1": 1e-05, "b037_textbook": 0.00715}),
    "mala_phi4_6x6_dirichlet": ("mala", "phi4", 36, 8, [0.0, 0.5, 2.0], None, {"b1": 0.0008, "b037_textbook": 0.064}),
    "mala_gmm4": ("mala", "gmm4", 2, 8, None, None, {"b1": 0.1, "b037_textbook": 6.0}),
    "mala_gmm17": ("mala", "gmm17", 2, 8, None, None, {"b1": 3.2, "b037_textbook": 6.0}),
    "cox_tile": ("mala", "lgcp", 64, 16, None, None, {"b1": 0.02, "b037_textbook": 0.4}),
    "cox_wide": ("mala", "lgcp", 64, 128, None, "wide", {"b1": 0.02, "b037_textbook": 0.4}),
    "hmc_phi4_d100": ("hmc", "phi4", 100, 8, None, None, {"b1": 0.0711, "b037_textbook": 0.116}),
    "hmc_gmm4": ("hmc", "gmm4", 2, 8, None, None, {"b1": 2.0, "b037_textbook": 2.16}),
    "cox_run": ("run", "lgcp", 64, 16, None, None, {"b1": 0.02, "b037_textbook": 0.4}),
}
HMC_LEAPFROG = 3


def setup(case):
    """(oracle distribution with ``init_params``, args, target block override or None) of a case."""
    from oracle import loop
    from tests import gpu_util as gu
    kind, target, d, B, tail, family, eps = CASES[case]
    block = None
    if target == "phi4":
        args, dist, *_ = gu.phi4_setup(d=d, B=B, hidden=32, F=16)
        if tail is not None:
            from tests.phi4_2d_oracle import PhiFour2D
            from tests.phi4_bc_oracle import PhiFourBC
            bc = ("pbc", 0.0) if tail[0] == 1.0 else ("dirichlet", tail[1])
            odist = (PhiFour2D if len(tail) == 3 else PhiFourBC)(d, dist.a, dist.beta, bc)
            odist.init_params = dist.init_params
            block, dist = [dist.a, dist.beta] + tail, odist
    elif target == "gmm4":
        args, dist, *_ = gu.gmm4_setup(B=B)
    elif target == "gmm17":                         # more than 16 modes: lane 0 evaluates the row
        ang = 2 * np.pi * np.arange(17) / 17
        dist = targets.GaussianMixture(6.0 * np.stack([np.cos(ang), np.sin(ang)], 1), np.ones((17, 2)), np.ones(17) / 17)
        args = loop.default_args(example="gaussian-mixture", dim=2, num_chain=B, step_size=0.2, seed=1, fourier_dim=16, **gu.hidden_lists(32))
        loop.setup(dist, args)
    else:
        args, dist, *_ = gu.lgcp_setup(n=8, B=B)
    return dist, args, block


def step_keys(case, j):
    """The key of step j and the per-chain keys that ``mfm_mala_step`` derives from it."""
    key = prng.split(prng.PRNGKey(1000 + sorted(CASES).index(case)), N_STEPS)[j]
    return key, prng.split(key, CASES[case][3])


RUN_KEYS = {"step_major": lambda B: prng.PRNGKey(77), "chain_major": lambda B: prng.split(prng.PRNGKey(78), B)}


def oracle_accepts(case, variant, eps=None, api=None):
    """The float64 oracle's decisions [N_STEPS, B], for choosing the step sizes (``api``: the key schedule of a run-kind case)."""
    kind, target, d, B, tail, family, sizes = CASES[case]
    beta, textbook = VARIANTS[variant]
    eps = sizes[variant] if eps is None else eps
    dist, args, _ = setup(case)
    vg = targets.Tempered(dist, beta).value_and_grad
    st = omala.init(dist.init_params.astype(np.float32).astype(np.float64), vg)
    out = []
    for j in range(N_STEPS):
        if kind == "run":
            k = RUN_KEYS[api](B)
            keys = prng.split_rows(k, N_STEPS)[:, j] if api == "chain_major" else prng.split(prng.split(k, N_STEPS)[j], B)
        else:
            keys = step_keys(case, j)[1]
        if kind == "hmc":
            st, info, _ = ohmc.kernel(keys, st, vg, eps, HMC_LEAPFROG)
        else:
            st, info, _ = omala.kernel(keys, st, vg, eps, textbook=textbook)
        out.append(info.is_accepted)
    return np.stack(out)


def _pad_rows(a, n):
    return np.concatenate([a, np.repeat(a[-1:], n - len(a), 0)])


def _keys_dev(keys):
    import torch
    return torch.as_tensor(np.ascontiguousarray(keys, dtype=np.uint32).view(np.int32)).cuda()


def record(case, variant):
    """Run one case on the device: {"<api>/<step>/<buffer>": numpy array} (HMC has no proposal buffers)."""
    import torch
    from mfm_amd import _lib
    from tests import gpu_util as gu
    kind, target, d, B, tail, family, sizes = CASES[case]
    beta, textbook = VARIANTS[variant]
    eps = sizes[variant]
    dist, args, block = setup(case)
    n_chains, B = B, -(-B // 16) * 16               # a context holds whole 16-row tiles: the rows past the chains repeat the last chain
    ctx = gu.make_ctx(dist, args, n_local=B, n_valid=n_chains, n_total=n_chains, family=_lib.FAMILY_WIDE if family == "wide" else None)
    if block is not None:
        ctx.set_target(_lib.PHI4, block)
    pos0 = torch.as_tensor(_pad_rows(dist.init_params.astype(np.float32), B)).cuda()
    out = {}

    def fresh():
        pos = pos0.clone(); logp = torch.empty(B, dtype=torch.float64, device="cuda"); grad = torch.empty_like(pos)
        ctx.mala_init(pos, beta, logp, grad)
        info = dict(acc_prob=torch.empty(B, device="cuda"), accepted=torch.empty(B, dtype=torch.uint8, device="cuda"),
                    proposed=torch.empty(B, d, device="cuda"), prop_weight=torch.empty(B, device="cuda"))
        return pos, logp, grad, info

    def keep(prefix, **bufs):
        for name, t in bufs.items():
            out[f"{prefix}/{name}"] = t.cpu().numpy().copy()

    if kind == "run":
        for api in RUN_KEYS:
            key = RUN_KEYS[api](B)
            pos, logp, grad, info = fresh()
            n_acc = torch.empty(B, dtype=torch.int32, device="cuda"); acc_sum = torch.empty(B, dtype=torch.float64, device="cuda")
            tp = torch.empty(N_STEPS, B, d, device="cuda"); tl = torch.empty(N_STEPS, B, dtype=torch.float64, device="cuda")
            ctx.mala_run(_keys_dev(key) if np.ndim(key) == 2 else key, beta, eps, N_STEPS, pos, logp, grad, thin=1, n_acc=n_acc, acc_sum=acc_sum,
                         acc=info["acc_prob"], is_acc=info["accepted"], proposed=info["proposed"], weight=info["prop_weight"], traj_pos=tp,
                         traj_logp=tl, textbook=textbook)
            for j in range(N_STEPS):
                keep(f"{api}/{j}", position=tp[j], logp=tl[j])
            keep(f"{api}/{N_STEPS - 1}", gradient=grad, n_acc=n_acc, acc_sum=acc_sum, **info)
            out[f"{api}/decisions"] = np.diff(np.concatenate([pos0.cpu().numpy()[None], tp.cpu().numpy()]), axis=0).any(-1)
    else:
        apis = ("step",) if kind == "hmc" else ("step", "step_keys")
        for api in apis:
            pos, logp, grad, info = fresh()
            if api == "step" and target == "lgcp":
                keep("init", logp=logp, gradient=grad)
            for j in range(N_STEPS):
                key, keys = step_keys(case, j)
                if kind == "hmc":
                    ctx.hmc_step(key, beta, eps, HMC_LEAPFROG, pos, logp, grad, info["acc_prob"], info["accepted"])
                    keep(f"{api}/{j}", position=pos, gradient=grad, logp=logp, acc_prob=info["acc_prob"], accepted=info["accepted"])
                    continue
                a = (info["acc_prob"], info["accepted"], info["proposed"], info["prop_weight"])
                if api == "step":
                    ctx.mala_step(key, beta, eps, pos, logp, grad, *a, textbook=textbook)
                else:
                    ctx.mala_step_keys(_keys_dev(_pad_rows(keys, B)), beta, eps, pos, logp, grad, *a, textbook=textbook)
                keep(f"{api}/{j}", position=pos, gradient=grad, logp=logp, **info)
            out[f"{api}/decisions"] = np.stack([out[f"{api}/{j}/accepted"] for j in range(N_STEPS)]).astype(bool)
    ctx.close()
    return out


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def stored(name, a):
    """What the fixture keeps of buffer ``name``: always its digest; the array itself (first ROWS rows) for per-chain buffers."""
    return digest(a), (a[:ROWS] if a.ndim == 1 else None)


def pack(digests, kept):
    """The fixture's three arrays: one "<buffer> <digest>" line per buffer, and the kept arrays' bytes end to end with one
    "<buffer> <dtype> <shape>" line each (a zip member per buffer would cost more than the buffers)."""
    names = sorted(kept)
    return dict(sha256=np.array([f"{n} {digests[n]}" for n in sorted(digests)]),
                index=np.array([f"{n} {kept[n].dtype.str} {','.join(map(str, kept[n].shape))}" for n in names]),
                blob=np.frombuffer(b"".join(np.ascontiguousarray(kept[n]).tobytes() for n in names), np.uint8))


def unpack(z):
    """(digests, kept arrays) of a fixture written from ``pack``."""
    digests = dict(str(s).split(" ") for s in z["sha256"])
    kept, off = {}, 0
    for s in z["index"]:
        n, dt, shape = str(s).split(" ")
        shape = tuple(int(v) for v in shape.split(","))
        kept[n] = np.frombuffer(z["blob"].tobytes(), np.dtype(dt), int(np.prod(shape)), off).reshape(shape)
        off += kept[n].nbytes
    return digests, kept
