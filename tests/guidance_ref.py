"""CPU reference of per-step guidance weights (steps.with_guidance, dsg_set_step_guidance), written independently of the
package:

  * the reverse loop of `steps_ref.sample_plan` with a weight per step: step j is guided with omega_j = float32(omega) * float32(g_j)
    (one float32 multiplication), and where g_j == 0 the step makes ONE `unet_forward` call, the conditional one, whose output is eps;
  * the cases, inputs and cached references that tests/test_guidance_cpu.py (budgets) and tests/test_gpu_guidance.py (parity) share;
  * the quality table of the NU checkpoint under guidance masks (tests/golden/g19_guidance.json), with the oracle's decoder and evaluator.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

import steps_ref as R
import variants_ref as VR
from _util import synth_params
from oracle import ddpm_oracle as O
from weights import CONFIGS

Ref = namedtuple("Ref", "y32 y64 trace32 trace64")

# name: (T, K).  msr80 carries the weights of the T = 6 sampling golden (seed 31): its one-pass context runs the 64- and 128-wide forms
NETS = dict(R.NETS, msr80=(6, 4))
B = R.B                                                  # 70 rows: three 32-row tiles, the last ragged
OMEGAS = R.OMEGAS                                        # (2, -1); omega = 500 only in bit-for-bit comparisons (variants_ref.py says why)
SAMPLERS = ("identity", "strided", "ddim0", "ddim0.5")
CAP = R.CAP
# Synthetic "trained" weights of msr80: the golden's seed; tests/test_guidance_cpu.py checks that every case's budget is at most CAP / 2
# under it (the rule of DESIGN.md 7.1: otherwise the next seed)
MSR80_SEED = 31


# ------------------------------------------------------------------------------------------------ masks
def masks(K):
    """{name: K weights}: the schedules of the parity cases.  Index K-1 runs first."""
    lo, hi = K // 4, max(K // 4, (3 * K) // 4 - 1)
    return {
        "even": [1.0 if j % 2 == 0 else 0.0 for j in range(K)],
        "odd": [1.0 if j % 2 == 1 else 0.0 for j in range(K)],
        "interval": [1.0 if lo <= j <= hi else 0.0 for j in range(K)],
        "half": [0.5 if j % 3 != 1 else 0.0 for j in range(K)],            # a weight that is neither 0 nor 1, between unguided steps
        "third": [1.0 if j % 3 == 1 else 0.0 for j in range(K)],
        "ones": [1.0] * K,
        "zeros": [0.0] * K,
    }


MASKS = ("even", "odd", "interval", "half")              # the mixed schedules of the GPU parity test


# ------------------------------------------------------------------------------------------------ the loop
@torch.no_grad()
def sample_guided(p, net, plan, T, cond, omega, g, y_start, noise, dtype=torch.float32, trace=None, passes=None):
    """y_0 of the reverse loop over `plan` under the weights `g` [K]; `noise` [K-2][B][D] or None.  dtype float64 evaluates the same loop
    (float32-valued weights, table, inputs and omega_j) in float64.  `passes`: a list that receives the number of denoiser passes per step."""
    K = len(plan.taus)
    assert len(g) == K
    pp = {k: v.to(dtype) for k, v in p.items()}
    cd, y = cond.to(dtype), y_start.to(dtype)
    rows = cd.shape[0]
    m0, m1 = torch.zeros(rows, 1, dtype=dtype), torch.ones(rows, 1, dtype=dtype)
    for done, j in enumerate(range(K - 1, -1, -1)):
        t = (torch.full((1, rows), int(plan.taus[j]), dtype=torch.int64) / T).to(dtype)
        gj = np.float32(g[j])
        eps1 = O.unet_forward(pp, net, y, t, cd, m1)
        if gj == 0:
            eps = eps1                                                       # unguided: the conditional pass alone, unchanged
        else:
            w = float(np.float32(omega) * gj)                                # one float32 multiplication
            eps0 = O.unet_forward(pp, net, y, t, cd, m0)
            eps = (1 + w) * eps1 - w * eps0
        if passes is not None:
            passes.append(1 if gj == 0 else 2)
        c1, c2, c3, c4 = (plan.coef[j, q].to(dtype) for q in range(4))
        z = noise[K - 1 - j].to(dtype) if float(c4) != 0.0 else 0
        y = (y - c1 * eps) * c2 + c3 * z
        if done < plan.renorm_steps:
            y = (y - torch.mean(y)) / torch.sqrt(torch.var(y))
        if trace is not None:
            trace.append((j, y.clone(), eps.clone()))
    return y


# ------------------------------------------------------------------------------------------------ shared cases
def net_params(name, seed=None):
    if name == "msr80":
        return synth_params("msr80", MSR80_SEED if seed is None else seed)
    return R.net_params(name, seed)


@functools.lru_cache(maxsize=None)
def inputs(name, rows=B):
    """cond [rows][C], y_T [rows][D], noise [T-2][rows][D] (a K-step call uses its first K-2 rows); read-only by convention.  70 rows of a
    net of steps_ref: that module's inputs; otherwise variants_ref's (nu3: the first rows of the checkpoint golden's own inputs)."""
    if name in R.NETS and rows == R.B:
        return R.inputs(name)[:3]
    if name in R.NETS:
        return VR.inputs(name, rows)
    T, _ = NETS[name]
    cfg = CONFIGS[name]
    gen = torch.Generator().manual_seed(1900 + T + rows)
    return (torch.rand(rows, cfg["cond_dim"], generator=gen), torch.randn(rows, cfg["input_dim"], generator=gen),
            torch.randn(T - 2, rows, cfg["input_dim"], generator=gen))


def case_plan(name, sampler, renorm_steps=None):
    T, K = NETS[name]
    if sampler == "identity":
        return R.plan_of(T, "identity", renorm_steps=renorm_steps)
    kind, eta = R.SAMPLERS[sampler]
    return R.plan_of(T, kind, K, eta, renorm_steps=renorm_steps)


@functools.lru_cache(maxsize=None)
def reference(name, sampler, mask, omega, seed=None):
    """Ref(y_0 float32, y_0 float64, float32 trace, float64 trace) of a parity case, computed once per process."""
    T, _ = NETS[name]
    net, p = net_params(name, seed)
    cond, y_T, z = inputs(name)
    plan = case_plan(name, sampler)
    K = len(plan.taus)
    g = masks(K)[mask]
    tr32, tr64 = [], []
    y32 = sample_guided(p, net, plan, T, cond, omega, g, y_T, z[:K - 2], trace=tr32)
    y64 = sample_guided(p, net, plan, T, cond, omega, g, y_T, z[:K - 2], dtype=torch.float64, trace=tr64)
    return Ref(y32, y64, tr32, tr64)


def budget(name, sampler, mask, omega, seed=None):
    r = reference(name, sampler, mask, omega, seed)
    return R.rel(r.y32, r.y64)


# ------------------------------------------------------------------------------------------------ the NU checkpoint's quality table
TABLE_MASKS = ("all", "interval5_14", "even", "third")
PIN_ROWS = 128


def table_mask(row, K):
    if row == "all":
        return [1.0] * K
    if row == "none":
        return [0.0] * K
    if row == "even":
        return masks(K)["even"]
    if row == "odd":
        return masks(K)["odd"]
    if row == "third":
        return masks(K)["third"]
    if row == "interval5_14":
        return [1.0 if 5 <= j <= 14 else 0.0 for j in range(K)]
    if row == "first_quarter_off":                       # unguided on the first quarter of the call: the highest K // 4 step indices
        return [0.0 if j >= K - K // 4 else 1.0 for j in range(K)]
    raise KeyError(row)


@functools.lru_cache(maxsize=None)
def nu_golden_cell(row, rows=512, omega=500.0):
    """Less ratio of the checkpoint on its first `rows` rows with the golden's own y_T / z, all T trained steps, under a mask."""
    g = R.nu_golden()
    T, P = int(g["T"]), float(g["P_sum"])
    net, p = R.net_params("nu3")
    plan = R.plan_of(T, "identity")
    cond = torch.from_numpy(g["cond"])[:rows]
    y0 = sample_guided(p, net, plan, T, cond, omega, table_mask(row, T), torch.from_numpy(g["y_T"])[:rows], torch.from_numpy(g["z"])[:, :rows])
    Xs = cond.clone(); Xs[:, 0::2] *= 400; Xs[:, 1::2] *= 400
    return float(O.nu_rate(O.nu_decode(y0.float(), 400, 400, P), Xs).sum() / VR.label_rate(rows).sum())


@functools.lru_cache(maxsize=None)
def nu_round_rate(seed, omega, renorm, K, rows, row):
    """Rate [rows] of one round under a mask, drawn as `variants_ref.nu_round_rate` draws it."""
    g = R.nu_golden()
    T, P = int(g["T"]), float(g["P_sum"])
    net, p = R.net_params("nu3")
    gen = torch.Generator().manual_seed(seed)
    y_T = torch.randn(rows, 5, generator=gen)
    z = torch.randn(K - 2, rows, 5, generator=gen)
    plan = R.plan_of(T, "identity", renorm_steps=renorm) if K == T else R.plan_of(T, "ddim", K, 0.0, renorm_steps=renorm)
    cond = torch.from_numpy(g["cond"])[:rows]
    y0 = sample_guided(p, net, plan, T, cond, omega, table_mask(row, K), y_T, z)
    Xs = cond.clone(); Xs[:, 0::2] *= 400; Xs[:, 1::2] *= 400
    return O.nu_rate(O.nu_decode(y0.float(), 400, 400, P), Xs)


def passes_of(row, K):
    return sum(1 if w == 0 else 2 for w in table_mask(row, K))
