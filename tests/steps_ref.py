"""CPU reference of sampling on a step grid (diffsg_amd/steps.py), written independently of the package:

  * the three coefficient tables in numpy float64 from the float32 `alphas_cumprod` buffer, one cast to float32;
  * the reverse loop over a plan on `oracle.ddpm_oracle.unet_forward` with explicit time values: step index K-1 first, noise row
    K-1-j at step j, the early renorm on the first `renorm_steps` steps of the call (torch.var unbiased over all B*D elements,
    as `O.sample_step`);
  * the cases, inputs and cached references that tests/test_steps_cpu.py (budgets) and tests/test_gpu_steps.py (parity) share.
"""
import functools
import os
from collections import namedtuple

import numpy as np
import torch

from _util import GOLD, synth_params
from oracle import ddpm_oracle as O
from weights import CONFIGS

Ref = namedtuple("Ref", "y32 y64 trace32 trace64")
Plan = namedtuple("Plan", "taus t coef renorm_steps")      # what the loop needs; `diffsg_amd.steps.StepPlan` has the same fields


# ------------------------------------------------------------------------------------------------ tables
def default_taus(T, K):
    """K grid points from 0 to T-1, evenly spaced, rounded half up (exact in integers)."""
    return [(2 * j * (T - 1) + (K - 1)) // (2 * (K - 1)) for j in range(K)]


def acp64(T):
    """The registered float32 alphas_cumprod of the cosine schedule, as float64."""
    return O.schedule_buffers(1.0 - O.cosine_betas(T))["alphas_cumprod"].double().numpy()


def times(taus, T):
    return torch.tensor(list(taus), dtype=torch.int64) / T


def strided_table(acp, taus):
    acp = np.asarray(acp, dtype=np.float64)
    rows = []
    for j in range(len(taus)):
        ab_t = acp[taus[j]]
        ab_p = acp[taus[j - 1]] if j else ab_t             # c3 at j = 0 is (1 - ab_t) / (1 - ab_t)
        alpha = ab_t / acp[taus[j - 1]] if j else ab_t
        rows.append([(1 - alpha) / np.sqrt(1 - ab_t), alpha ** -0.5, (1 - ab_p) / (1 - ab_t), 1.0 if j >= 2 else 0.0])
    return np.array(rows, dtype=np.float64).astype(np.float32)


def ddim_table(acp, taus, eta):
    acp = np.asarray(acp, dtype=np.float64)
    rows = []
    for j in range(len(taus)):
        ab_t = acp[taus[j]]
        ab_p = acp[taus[j - 1]] if j else 1.0
        sigma = eta * np.sqrt((1 - ab_p) / (1 - ab_t)) * np.sqrt(max(1 - ab_t / ab_p, 0.0))
        scale = np.sqrt(ab_p / ab_t)
        # y' = scale (y - sqrt(1 - ab_t) eps) + sqrt(1 - ab_p - sigma^2) eps + sigma z = (y - c1 eps) scale + sigma z
        c1 = np.sqrt(1 - ab_t) - np.sqrt(max(1 - ab_p - sigma ** 2, 0.0)) / scale
        rows.append([c1, scale, sigma, 1.0 if (j >= 2 and eta > 0) else 0.0])
    return np.array(rows, dtype=np.float64).astype(np.float32)


def trained_table(T):
    """The trained schedule's own scalars, evaluated as `O.sample_step` evaluates them (float32 tensor operations on the buffers)."""
    b = O.schedule_buffers(1.0 - O.cosine_betas(T))
    acp = b["alphas_cumprod"]
    rows = [torch.stack((b["betas"][i] / b["sqrt_one_minus_alphas_cumprod"][i], b["reciprocal_sqrt_alphas"][i],
                         (1.0 - acp[i - 1 if i - 1 >= 0 else 0]) / (1.0 - acp[i]), torch.tensor(1.0 if i > 1 else 0.0))) for i in range(T)]
    return torch.stack(rows).numpy()


def plan_of(T, kind, K=None, eta=0.0, k=None, renorm_steps=None):
    """kind: "strided" | "ddim" (K steps of the default grid) | "identity" (all T steps) | "tail" (steps k .. 0)."""
    if kind == "identity":
        taus, coef, rn = list(range(T)), trained_table(T), min(T, 4)
    elif kind == "tail":
        taus, coef, rn = list(range(k + 1)), trained_table(T)[:k + 1], 0
    else:
        taus = default_taus(T, K)
        coef = strided_table(acp64(T), taus) if kind == "strided" else ddim_table(acp64(T), taus, eta)
        rn = min(K, 4)
    return Plan(tuple(taus), times(taus, T), torch.from_numpy(np.ascontiguousarray(coef)), rn if renorm_steps is None else renorm_steps)


# ------------------------------------------------------------------------------------------------ the loop
@torch.no_grad()
def sample_plan(p, net, plan, T, cond, omega, y_start, noise, dtype=torch.float32, trace=None):
    """y_0 of the reverse loop over `plan`; `noise` [K-2][B][D] or None.  dtype float64 evaluates the same loop (float32-valued weights,
    table and inputs) in float64: the error budget of the reference's own float32 arithmetic."""
    K = len(plan.taus)
    pp = {k: v.to(dtype) for k, v in p.items()}
    cd, y = cond.to(dtype), y_start.to(dtype)
    B = cd.shape[0]
    m0, m1 = torch.zeros(B, 1, dtype=dtype), torch.ones(B, 1, dtype=dtype)
    for done, j in enumerate(range(K - 1, -1, -1)):
        t = (torch.full((1, B), int(plan.taus[j]), dtype=torch.int64) / T).to(dtype)
        eps0 = O.unet_forward(pp, net, y, t, cd, m0)
        eps1 = O.unet_forward(pp, net, y, t, cd, m1)
        eps = (1 + omega) * eps1 - omega * eps0
        c1, c2, c3, c4 = (plan.coef[j, q].to(dtype) for q in range(4))
        z = noise[K - 1 - j].to(dtype) if float(c4) != 0.0 else 0
        y = (y - c1 * eps) * c2 + c3 * z
        if done < plan.renorm_steps:
            y = (y - torch.mean(y)) / torch.sqrt(torch.var(y))
        if trace is not None:
            trace.append((j, y.clone(), eps.clone()))
    return y


def rel(a, b):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64)
    b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ------------------------------------------------------------------------------------------------ shared cases
B = 70                                                   # three 32-row tiles, the last ragged
NETS = {"tiny": (8, 4), "nu3": (20, 10), "msr3": (12, 5)}         # name: (T, K)
OMEGAS = (2.0, -1.0)
SAMPLERS = {"strided": ("strided", 0.0), "ddim0": ("ddim", 0.0), "ddim0.5": ("ddim", 0.5)}
TAIL_KS = (0, 1, 5)
CAP = 1e-5                                               # the reference's own float32-against-float64 error of every parity case
# Synthetic "trained" weights: the first seed from 3 upwards at which every case of the net has a budget of at most CAP / 2
# (the rule of DESIGN.md 7.1; tests/test_steps_cpu.py re-derives both)
SEEDS = {"tiny": 3, "msr3": 3}


@functools.lru_cache(maxsize=None)
def nu_golden():
    return np.load(os.path.join(GOLD, "g4_sample_nu_ckpt.npz"))


def net_params(name, seed=None):
    """(oracle plan of the net, {key: float32 tensor}); nu3 carries the shipped NU checkpoint."""
    cfg = CONFIGS[name]
    if name == "nu3" and seed is None:
        g = nu_golden()
        return (O.unet_plan(cfg["input_dim"], cfg["proj_dim"], cfg["cond_dim"], cfg["dims"], cfg["n_blocks"]),
                {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w.")})
    return synth_params(name, SEEDS[name] if seed is None else seed)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """cond [B][C], y_T [B][D], noise [T-2][B][D] (a K-step plan uses its first K-2 rows), q_noise [B][D]; read-only by convention.
    nu3: the first B rows of the checkpoint golden's own inputs."""
    T, _ = NETS[name]
    cfg = CONFIGS[name]
    gen = torch.Generator().manual_seed(1700 + T)
    if name == "nu3":
        g = nu_golden()
        cond, y_T, z = torch.from_numpy(g["cond"])[:B], torch.from_numpy(g["y_T"])[:B], torch.from_numpy(g["z"])[:, :B]
    else:
        cond = torch.rand(B, cfg["cond_dim"], generator=gen)
        y_T = torch.randn(B, cfg["input_dim"], generator=gen)
        z = torch.randn(T - 2, B, cfg["input_dim"], generator=gen)
    q = torch.randn(B, cfg["input_dim"], generator=gen)
    return cond.contiguous(), y_T.contiguous(), z.contiguous(), q


def case_plan(name, sampler):
    T, K = NETS[name]
    kind, eta = SAMPLERS[sampler]
    return plan_of(T, kind, K, eta)


@functools.lru_cache(maxsize=None)
def reference(name, sampler, omega, seed=None):
    """Ref(y_0 float32, y_0 float64, float32 trace, float64 trace) of a parity case, computed once per process; a trace is
    [(step index, y after the step, guided eps)], first step of the call first."""
    T, K = NETS[name]
    net, p = net_params(name, seed)
    cond, y_T, z, _ = inputs(name)
    plan = case_plan(name, sampler)
    tr32, tr64 = [], []
    y32 = sample_plan(p, net, plan, T, cond, omega, y_T, z[:K - 2], trace=tr32)
    y64 = sample_plan(p, net, plan, T, cond, omega, y_T, z[:K - 2], dtype=torch.float64, trace=tr64)
    return Ref(y32, y64, tr32, tr64)


def trace_arrays(trace):
    """(y record, eps record) of a trace in the layout of DDPM.y_i_record / eps_i_record: (B, K*D), first step first."""
    ys, es = torch.stack([y for _, y, _ in trace]), torch.stack([e for _, _, e in trace])
    B = ys.shape[1]
    return ys.permute(1, 0, 2).reshape(B, -1).numpy(), es.permute(1, 0, 2).reshape(B, -1).numpy()


def tail_start(name, k):
    """q_sample of the case's y_T (standing in for a solution) to step k, as the reference's float32 tensor operations give it."""
    T, _ = NETS[name]
    b = O.schedule_buffers(1.0 - O.cosine_betas(T))
    _, y_T, _, q = inputs(name)
    return b["sqrt_alphas_cumprod"][k] * y_T + b["sqrt_one_minus_alphas_cumprod"][k] * q


@functools.lru_cache(maxsize=None)
def tail_reference(name, k, omega, renorm_steps=0):
    T, _ = NETS[name]
    net, p = net_params(name)
    cond, _, z, _ = inputs(name)
    plan = plan_of(T, "tail", k=k, renorm_steps=renorm_steps)
    y_k = tail_start(name, k)
    zz = z[:max(k - 1, 0)]
    return (sample_plan(p, net, plan, T, cond, omega, y_k, zz), sample_plan(p, net, plan, T, cond, omega, y_k, zz, dtype=torch.float64))


# ------------------------------------------------------------------------------------------------ the NU checkpoint's task metric
def nu_ratio(y0):
    """Less ratio (classifier_free_NU.py:350-360) of samples for the checkpoint golden's 512 rows, with the oracle's evaluators."""
    g = nu_golden()
    P = float(g["P_sum"])
    Xs = torch.from_numpy(g["cond"]).clone(); Xs[:, 0::2] *= 400; Xs[:, 1::2] *= 400
    Yt = torch.from_numpy(g["y_test"]).clone(); Yt[:, 0] *= 400; Yt[:, 1] *= 400; Yt[:, 2:] *= P
    return float(O.nu_rate(O.nu_decode(y0.float(), 400, 400, P), Xs).sum() / O.nu_rate(Yt, Xs).sum())


def nu_ratio_cell(K, kind, eta, omega=500.0):
    """One cell of the quality table: the checkpoint on its 512 rows, its own y_T and the first K-2 rows of its z."""
    g = nu_golden()
    T = int(g["T"])
    net, p = net_params("nu3")
    plan = plan_of(T, kind, K, eta)          # K = T: the trained schedule's table rebuilt in float64, not the trained table's bits
    y0 = sample_plan(p, net, plan, T, torch.from_numpy(g["cond"]), omega, torch.from_numpy(g["y_T"]), torch.from_numpy(g["z"])[:K - 2])
    return nu_ratio(y0)
