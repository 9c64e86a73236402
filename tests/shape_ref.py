"""UNet1D descriptors off the shipped catalogue (tests/golden/weights.py), their seeded inputs and their CPU references.

`dsg_create` accepts far more nets than the five shipped ones, and which kernels a net runs is decided from its shape by host code
(the fused-run choice, the 8-wide float32 section, the LDS phase plan, the tile-step kernel, the training tables).  Every entry of
SHAPES exists to reach one of those branches ("Descriptor space"); tests/test_shapes_cpu.py checks on the CPU that the
oracle itself is well enough conditioned on each of them for the GPU bounds to mean something, and tests/test_gpu_shapes.py runs them
on the device.  Everything here is the oracle and seeded torch draws: nothing of the code under test.

Inputs (the same tensors on the CPU and on the device): B = 70 rows -- three 32-row tiles, the last one ragged, and more than one tile
per CFG pass -- T = 5, drawn in the order the parity tests draw them (tests/test_gpu_parity.py).  References are computed once per
process and shared (functools.lru_cache); callers must not write into them.
"""
import functools

import torch

from oracle import ddpm_oracle as O
from weights import synth_weights

B, T = 70, 5
OMEGAS = (2.0, -1.0)        # a negative omega keeps the unconditional pass visible (omega = 0 hides it: eps = eps1)
SAMPLE_CAP = 1e-5           # rel(ref32, ref64) of the sampling reference at omega = 2
GRAD_CAP = 2e-5             # worst per-tensor grad_errs(ref32, ref64)


def _d(input_dim, proj_dim, cond_dim, dims, n_blocks, seed=3):
    return dict(cfg=dict(input_dim=input_dim, proj_dim=proj_dim, cond_dim=cond_dim, dims=tuple(dims), n_blocks=n_blocks), seed=seed)


# name: descriptor and weight seed (synth_weights(..., flavour="trained")).  The comment gives what the CPU check measured for the entry:
# sampling budget rel(ref32, ref64) at omega = 2 | at omega = -1 | worst per-tensor gradient budget.
# The seed is 3 unless that net misses a cap; then it is the first seed from 3 upwards with both budgets at most HALF their caps (the
# narrowest nets -- 4- and 8-wide LayerNorms -- are conditioned very differently from seed to seed: skip4 ranges over 8e-6 .. 3e-3).
# Chosen with this module alone, on the CPU.
SHAPES = {
    "allwide":  _d(7, 64, 5, (64, 64), 1),                              # 1.1e-06 | 5.7e-07 | 1.9e-06
    "widen":    _d(6, 64, 10, (128, 64), 1),                            # 1.4e-06 | 5.7e-07 | 8.4e-07
    "hill":     _d(5, 16, 6, (64, 16), 2),                              # 1.3e-06 | 1.3e-06 | 4.6e-06
    "jump":     _d(4, 128, 4, (8, 128), 1),                             # 2.4e-06 | 1.7e-06 | 3.5e-06
    "flat32":   _d(9, 32, 17, (32, 32, 32), 1),                         # 1.2e-06 | 5.6e-07 | 3.2e-06
    "flat32x4": _d(9, 32, 17, (32, 32, 32), 4),                         # 2.4e-06 | 7.8e-07 | 2.6e-06
    "nb4":      _d(3, 32, 9, (16, 8), 4),                               # 3.4e-06 | 2.8e-07 | 3.0e-06
    "nb1":      _d(3, 32, 9, (16, 8), 1),                               # 3.1e-06 | 1.0e-06 | 2.3e-06
    "deep8":    _d(12, 64, 12, (64, 32, 32, 16, 16, 8, 8, 4), 2, seed=4),  # 1.1e-06 | 4.2e-07 | 5.7e-06  (seed 3: 6.7e-05 for the gradients)
    "skip4":    _d(3, 16, 3, (4, 4), 3, seed=21),                   # 1.8e-06 | 2.2e-07 | 8.4e-06  (seed 3: 6.2e-05 for the gradients)
    "one8":     _d(2, 8, 1, (8,), 1, seed=4),                           # 1.8e-06 | 1.9e-07 | 6.0e-06  (seed 3: 2.8e-05 for sampling)
    "io128":    _d(128, 32, 300, (32, 16), 1),                          # 1.1e-06 | 2.8e-07 | 1.5e-06
    "io127":    _d(127, 128, 4096, (128,), 1),                          # 9.7e-07 | 4.7e-07 | 1.4e-06
}
NAMES = list(SHAPES)
# Outside the catalogue (and its caps): a net dsg_create accepts and samples, and whose training step is refused -- 83 residual blocks and
# 18 Linears are 267 tracked gradient tensors against kMaxGmax = 256 (test_gpu_shapes.test_training_refusal_...).
REFUSED = {"gmax267": _d(3, 8, 2, (8,) * 8, 4)}
_ALL = {**SHAPES, **REFUSED}


@functools.lru_cache(maxsize=None)
def net(name):
    """(plan, {key: float32 tensor}) of a catalogue entry."""
    e = _ALL[name]
    c = e["cfg"]
    plan = O.unet_plan(c["input_dim"], c["proj_dim"], c["cond_dim"], c["dims"], c["n_blocks"])
    w = synth_weights(O.state_shapes(plan), e["seed"], "trained")
    return plan, {k: torch.from_numpy(v) for k, v in w.items()}


def bufs():
    return O.schedule_buffers(1.0 - O.cosine_betas(T))


@functools.lru_cache(maxsize=None)
def sample_inputs(name):
    """cond [B, C], y_T [B, D], z [T - 2, B, D], drawn as test_sample_large_launch_vs_oracle draws them."""
    c = _ALL[name]["cfg"]
    g = torch.Generator().manual_seed(9)
    cond = torch.rand(B, c["cond_dim"], generator=g)
    y_T = torch.randn(B, c["input_dim"], generator=g)
    z = torch.randn(T - 2, B, c["input_dim"], generator=g)
    return cond, y_T, z


@functools.lru_cache(maxsize=None)
def train_inputs(name):
    """y, cond, ts [1, B], noise, mask [B, 1], drawn as test_train_step_vs_oracle_ragged draws them."""
    c = _ALL[name]["cfg"]
    g = torch.Generator().manual_seed(B + 1)
    y = torch.rand(B, c["input_dim"], generator=g)
    cond = torch.rand(B, c["cond_dim"], generator=g)
    ts = torch.randint(0, T, (1, B), generator=g)
    noise = torch.randn(B, c["input_dim"], generator=g)
    mask = (torch.rand(B, 1, generator=g) < 0.9).float()
    return y, cond, ts, noise, mask


@functools.lru_cache(maxsize=None)
def forward_inputs(name, rows):
    """x, t [1, rows] (already divided), cond, mask [rows, 1] (mixed), drawn as test_unet_forward_vs_oracle_ragged draws them."""
    c = _ALL[name]["cfg"]
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, c["input_dim"], generator=g)
    cond = torch.rand(rows, c["cond_dim"], generator=g)
    ts = torch.randint(0, 50, (1, rows), generator=g)
    mask = (torch.rand(rows, 1, generator=g) < 0.8).float()
    return x, ts / 50, cond, mask


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


@functools.lru_cache(maxsize=None)
def forward_ref(name, rows):
    plan, p = net(name)
    with torch.no_grad():
        return O.unet_forward(p, plan, *forward_inputs(name, rows))


@functools.lru_cache(maxsize=None)
def sample_ref(name, omega):
    """(float32 oracle samples, budget = rel(float32 oracle, float64 oracle)) on sample_inputs(name)."""
    plan, p = net(name)
    cond, y_T, z = sample_inputs(name)
    b = bufs()
    zd = {i: z[j] for j, i in enumerate(range(T - 1, 1, -1))}
    with torch.no_grad():
        ref = O.ddpm_sample(p, plan, b, T, cond, omega, y_T, zd)
        ref64 = O.ddpm_sample({k: v.double() for k, v in p.items()}, plan, {k: v.double() for k, v in b.items()}, T, cond.double(), omega,
                              y_T.double(), {i: v.double() for i, v in zd.items()})
    return ref, _rel(ref, ref64)


@functools.lru_cache(maxsize=None)
def train_ref(name):
    """(loss, float32 gradients, float64 gradients) of the oracle's autograd on train_inputs(name)."""
    plan, p = net(name)
    b = bufs()
    loss, g32 = O.ddpm_loss_and_grads(p, plan, b, T, *train_inputs(name))
    _, g64 = O.ddpm_loss_and_grads(p, plan, b, T, *train_inputs(name), f64=True)
    return loss, g32, g64


def narrow_flags(name):
    """[(operator name, narrow?)] in the library's operator order (feature_proj, down.*, middle.res1/2, up.*, final): narrow = a
    residual block or Down/Upsample Linear whose OUTPUT is at most 32 wide -- what the library's planner may fuse."""
    plan, _ = net(name)
    ops = [("feature_proj", False)]
    for side in ("down", "up"):
        if side == "up":
            ops += [("middle.res1", plan["mid_w"] <= 32), ("middle.res2", plan["mid_w"] <= 32)]
        for idx, (kind, _, o) in enumerate(plan[side]):
            ops.append((f"{side}.{idx}.{kind}", o <= 32))
    return ops + [("final", False)]


def longest_narrow_run(name):
    """(lo, hi) of the first longest consecutive run of narrow operators, (0, 0) when it has fewer than two."""
    flags = [f for _, f in narrow_flags(name)] + [False]
    best, lo = (0, 0), None
    for i, f in enumerate(flags):
        if f and lo is None:
            lo = i
        if not f and lo is not None:
            if i - lo > best[1] - best[0]:
                best = (lo, i)
            lo = None
    return best if best[1] - best[0] >= 2 else (0, 0)
