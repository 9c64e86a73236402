"""Host-only reference of training on a timestep law: the CDF rule restated in numpy, the expected draw, the weighted
loss and its gradients through the oracle with torch autograd, and the per-timestep sums.  Nothing of the code under test.

Nets: `tiny` (T = 8) and `nu3` (T = 20) of the shipped catalogue, B = 70 rows (three row tiles, the last ragged).  The weight seed of
each net follows the rule of DESIGN.md 7.1: the first seed from 3 upwards at which the float32-against-float64 error of the WEIGHTED
reference stays at or below half of both caps (tests/test_timesteps_cpu.py checks the caps and prints the budgets).  Caps: the per-tensor
gradient cap of the shape catalogue (shape_ref.GRAD_CAP = 2e-5) and, for the loss, 1e-6 relative -- a tenth of the 1e-5 the GPU test
allows the device.  References are computed once per process and shared; callers must not write into them.
"""
import functools

import numpy as np
import torch

from _util import synth_params
from oracle import ddpm_oracle as O
from weights import CONFIGS

B = 70
# measured by budgets(): tiny seed 3 gives 1.5e-08 | 1.5e-05 (gradients above half the cap), seed 4 3.6e-09 | 4.0e-06; nu3 seed 3 5.4e-09 | 3.1e-06
NETS = {"tiny": dict(T=8, seed=4), "nu3": dict(T=20, seed=3)}
GRAD_CAP = 2e-5
LOSS_CAP = 1e-6
GRID = 1 << 24


def cdf24(p):
    """floor(2^24 cumsum(p) / sum(p) + 0.5) in float64, the last entry 2^24."""
    p = np.asarray(p, dtype=np.float64)
    c = np.floor(float(GRID) * np.cumsum(p) / np.sum(p) + 0.5).astype(np.int64)
    c[-1] = GRID
    return c


def expected_ts(cdf, u24):
    return np.searchsorted(np.asarray(cdf, dtype=np.int64), np.asarray(u24, dtype=np.int64), side="right")


@functools.lru_cache(maxsize=None)
def net(name, seed=None):
    return synth_params(name, NETS[name]["seed"] if seed is None else seed)


def bufs(name):
    T = NETS[name]["T"]
    return O.schedule_buffers(1.0 - O.cosine_betas(T))


@functools.lru_cache(maxsize=None)
def train_inputs(name, rows=B):
    """y, cond, ts [1, rows], noise, mask [rows, 1], drawn as the parity tests draw them."""
    c, T = CONFIGS[name], NETS[name]["T"]
    g = torch.Generator().manual_seed(rows + 1)
    y = torch.rand(rows, c["input_dim"], generator=g)
    cond = torch.rand(rows, c["cond_dim"], generator=g)
    ts = torch.randint(0, T, (1, rows), generator=g)
    noise = torch.randn(rows, c["input_dim"], generator=g)
    mask = (torch.rand(rows, 1, generator=g) < 0.9).float()
    return y, cond, ts, noise, mask


@functools.lru_cache(maxsize=None)
def weights(name):
    """float32 [T]: random weights in [0, 3] with exact zeros at two timesteps that `train_inputs` draws."""
    T = NETS[name]["T"]
    g = torch.Generator().manual_seed(17 + T)
    w = (torch.rand(T, generator=g) * 3.0).to(torch.float32)
    drawn = sorted(set(train_inputs(name)[2].reshape(-1).tolist()))
    w[drawn[0]] = 0.0
    w[drawn[len(drawn) // 2]] = 0.0
    return w


def weighted_loss_and_grads(p, plan, b, T, y, cond, ts, noise, mask, w, f64=False):
    """((w[ts][:, None] * (noise - eps)^2).mean(), its gradient for every denoiser tensor), float32 or float64 arithmetic."""
    dt = torch.float64 if f64 else torch.float32
    leaf = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in p.items()}
    bb = {k: v.to(dt) for k, v in b.items()}
    y_t = O.q_sample(bb, y.to(dt), ts, noise.to(dt))
    eps = O.unet_forward(leaf, plan, y_t, (ts / T).to(dt), cond.to(dt), mask.to(dt))
    loss = (w.to(dt)[ts.reshape(-1)][:, None] * (noise.to(dt) - eps) ** 2).mean()
    grads = torch.autograd.grad(loss, list(leaf.values()), allow_unused=True)
    return loss.detach(), {k: (g if g is not None else torch.zeros_like(v)).detach() for (k, v), g in zip(leaf.items(), grads)}


@functools.lru_cache(maxsize=None)
def weighted_ref(name, seed=None):
    """(loss32, grads32, loss64, grads64) of the weighted loss on train_inputs(name) with weights(name)."""
    plan, p = net(name, seed)
    T = NETS[name]["T"]
    args = (p, plan, bufs(name), T) + train_inputs(name) + (weights(name),)
    l32, g32 = weighted_loss_and_grads(*args)
    l64, g64 = weighted_loss_and_grads(*args, f64=True)
    return l32, g32, l64, g64


def grad_budget(g32, g64):
    """{key: max|g32 - g64| / max(max|g64_k|, 1e-3 max|g64|)}: the per-tensor error measure of the parity tests."""
    gmax = max(float(v.abs().max()) for v in g64.values())
    return {k: float((g32[k].double() - g64[k].double()).abs().max()) / max(float(g64[k].abs().max()), 1e-3 * gmax) for k in g64}


def budgets(name, seed=None):
    """(relative float32-against-float64 error of the weighted loss, worst per-tensor gradient budget)."""
    l32, g32, l64, g64 = weighted_ref(name, seed)
    return abs(float(l32) - float(l64)) / abs(float(l64)), max(grad_budget(g32, g64).values())


def per_timestep_sums(eps_hat, noise, ts, T):
    """(sq float64 [T], rows int64 [T]): the UNWEIGHTED sum over the rows with ts == t of sum_f (eps_hat - noise)^2, in float64 from the
    float32 differences, and the number of such rows."""
    d = (eps_hat.to(torch.float32) - noise.to(torch.float32)).double()
    per_row = (d * d).sum(dim=1)
    t = ts.reshape(-1).long()
    sq = torch.zeros(T, dtype=torch.float64).index_add_(0, t, per_row)
    return sq, torch.bincount(t, minlength=T)
