"""The cases that tests/test_philox_cpu.py (budgets) and tests/test_gpu_philox.py (parity) share: sampling with the device's own draws
against the oracle on the restated draws of tests/philox_ref.py.

Every net carries its synthetic "trained" weights (nu3: the shipped checkpoint) with the last Linear zeroed: eps is then exactly 0, the
conditioning drops out and y_0 is a known function of y_T, the noise, the coefficient table and the renorm -- while every operator of
every launch form still runs.  The reference of a case is the oracle's loop in float64 on the restated draws; its budget is

    FACTOR x (rel(oracle32, oracle64)  +  rel(oracle64 on the float32-evaluated draws, oracle64)),      capped at CAP,

both terms relative to the output's largest magnitude: what float32 arithmetic does to the loop, plus what the rounding of a float32
Box-Muller does to its result, and FACTOR = 8 of that sum.  Of the second term because the device's logf / sincosf are documented at
1-2 ulp where numpy's float32 ones keep to <= 1 ulp, with one more rounding in the final product; of the first because two float32
evaluations of one loop (torch's on the CPU, the kernels') are each that far from float64 independently of one another, not one inside
the other.  The budgets come to 1.0e-6 .. 4.3e-6; a draw taken from the wrong counter, key or stream moves the result by O(1).
"""
import functools
from collections import namedtuple

import numpy as np
import torch

import guidance_ref as G
import multistep_ref as MR
import philox_ref as P
import steps_ref as R
import variants_ref as VR
from oracle import ddpm_oracle as O
from weights import CONFIGS

CAP = 1e-4               # of the output's largest magnitude
FACTOR = 8.0
FOLD = 0x9E3779B97F4A7C15
# name: (weights of, T).  tiny70: 70 steps = 4 early steps + step graphs of 32, 32 and 2 steps: every replayed run length reads the counter
NETS = {"tiny": ("tiny", 8), "nu3": ("nu3", 20), "msr80": ("msr80", 6), "tiny70": ("tiny", 70)}
K_OF = {"tiny": 4, "nu3": 10}                                    # the step count of the plans (steps_ref.NETS)

# kind: "plain" (O.ddpm_sample, all T trained steps) | "plan" (steps_ref.sample_plan; arg = (table kind, eta)) | "dpmpp"
# (multistep_ref.sample_multistep; arg = renorm count) | "guided" (guidance_ref.sample_guided on all T steps; arg = mask name) |
# "chunks" (variants_ref.sample_variants; arg = (chunk_rows, ((omega, table kind, eta, renorm count) per chunk) or None: plain chunks)).
# seed: one int, or one per chunk.  given: "" | "y_T" | "noise": that part is injected (the float32 values of the restated draws), the
# other drawn on the device.
Case = namedtuple("Case", "id net B kind arg seed given", defaults=("",))

S0 = (1 << 40) + 12345                                            # the high half of the key is live in every plain case
PLAIN = tuple(Case(f"{net}-b{B}", net, B, "plain", None, S0 + B) for net in ("tiny", "nu3", "msr80") for B in (1, 33, 70)) + (
    Case("tiny70-b70", "tiny70", 70, "plain", None, S0 + 7),)
MIXED = (Case("tiny-b33-given-y_T", "tiny", 33, "plain", None, S0 + 33, "y_T"),
         Case("tiny-b33-given-noise", "tiny", 33, "plain", None, S0 + 33, "noise"),
         Case("msr80-b33-given-y_T", "msr80", 33, "plain", None, S0 + 33, "y_T"),
         Case("msr80-b33-given-noise", "msr80", 33, "plain", None, S0 + 33, "noise"))
REC = (Case("nu3-b33-rec", "nu3", 33, "plain", None, 99), Case("msr80-b70-rec", "msr80", 70, "plain", None, (1 << 33) + 99))
CHUNK_SEEDS = (11, (1 << 40) + 5, 77)
CHUNKED = (Case("tiny-b150-c64", "tiny", 150, "chunks", (64, None), CHUNK_SEEDS),             # n = 450: the scalar tail; last chunk 22 rows
           Case("msr80-b150-c64", "msr80", 150, "chunks", (64, None), CHUNK_SEEDS))           # quads
VARIANTS = (Case("nu3-b150-c64-variants", "nu3", 150, "chunks",
                 (64, ((2.0, "strided", 0.0, 4), (-1.0, "ddim", 0.0, 0), (2.0, "ddim", 0.5, 1))), CHUNK_SEEDS),)
PLANS = (Case("nu3-strided", "nu3", 70, "plan", ("strided", 0.0), S0 + 1), Case("nu3-ddim1", "nu3", 70, "plan", ("ddim", 1.0), S0 + 2),
         Case("nu3-ddim0-a", "nu3", 70, "plan", ("ddim", 0.0), S0 + 3), Case("nu3-ddim0-b", "nu3", 70, "plan", ("ddim", 0.0), 3),
         Case("tiny-ddim1", "tiny", 33, "plan", ("ddim", 1.0), S0 + 4),
         Case("nu3-dpmpp", "nu3", 70, "dpmpp", 0, S0 + 5), Case("nu3-dpmpp-rn4", "nu3", 70, "dpmpp", 4, S0 + 6))
GUIDED = (Case("nu3-guided-half", "nu3", 70, "guided", "half", S0 + 8), Case("tiny-guided-even", "tiny", 33, "guided", "even", S0 + 9))
HIGH = (Case("tiny-b33-seed-lo", "tiny", 33, "plain", None, 7), Case("tiny-b33-seed-hi", "tiny", 33, "plain", None, 7 | (1 << 45)))
# sharded sampling (parallel.sample_sharded): rank r's seed is seed ^ r * FOLD; two ranks' draws on 70 x 80 elements
FOLDED = tuple(Case(f"msr80-b70-rank{r}", "msr80", 70, "plain", None, (S0 + 70) ^ (r * FOLD) & (2 ** 64 - 1)) for r in (0, 1))
ALL = PLAIN + MIXED + REC + CHUNKED + VARIANTS + PLANS + GUIDED + HIGH + FOLDED
CASE = {c.id: c for c in ALL}
assert len(CASE) == len(ALL)
OMEGA = 2.0                                                       # of every call without variants; eps == 0, so it multiplies zeros

Ref = namedtuple("Ref", "y64 budget rel32 response steps")       # steps: [(step index, y64 after it, its budget)], first step first


def rel(a, b):
    return R.rel(a, b)


@functools.lru_cache(maxsize=None)
def zero_net(net):
    """(oracle plan, {key: float32 tensor}) of the net with `final` zeroed."""
    name = NETS[net][0]
    plan, p = G.net_params(name)
    p = {k: v.clone() for k, v in p.items()}
    p["final.weight"].zero_()
    p["final.bias"].zero_()
    return plan, p


@functools.lru_cache(maxsize=None)
def cond_of(net, B):
    return torch.rand(B, CONFIGS[NETS[net][0]]["cond_dim"], generator=torch.Generator().manual_seed(2100 + B))


def ref_plans(case):
    """The reference plan(s) of a case: one, or one per chunk; None for a plain call."""
    T = NETS[case.net][1]
    if case.kind == "plan":
        return R.plan_of(T, case.arg[0], K_OF[case.net], case.arg[1])
    if case.kind == "dpmpp":
        return MR.plan_of(T, K_OF[case.net], case.arg)
    if case.kind == "guided":
        return R.plan_of(T, "identity")
    if case.kind == "chunks":
        rows, var = case.arg
        nch = -(-case.B // rows)
        if var is None:
            return [R.plan_of(T, "identity")] * nch
        return [R.plan_of(T, kind, K_OF[case.net], eta, renorm_steps=rn) for _, kind, eta, rn in var]
    return None


def steps_of(case):
    pl = ref_plans(case)
    return NETS[case.net][1] if pl is None else len((pl[0] if isinstance(pl, list) else pl).taus)


def draws(case, f32=False):
    """(y_T [B][D], noise [K-2][B][D]) float64 arrays: the restated draws of the case (rows of noise-free steps are NaN)."""
    D, K, pl = CONFIGS[NETS[case.net][0]]["input_dim"], steps_of(case), ref_plans(case)
    if case.kind == "chunks":
        noisy = np.stack([p.coef[:, 3].numpy() != 0 for p in pl])
        y, z = P.sample_draws_chunked(case.seed, K, case.B, D, case.arg[0], noisy, f32)
    else:
        y, z = P.sample_draws(case.seed, K, case.B * D, None if pl is None else pl.coef[:, 3].numpy() != 0, f32)
    return y.reshape(case.B, D).astype(np.float64), z.reshape(-1, case.B, D).astype(np.float64)


def given(case):
    """The injected part of a mixed case as a float32 tensor (the restated draws, rounded once), or None."""
    y, z = draws(case)
    return {"": None, "y_T": torch.from_numpy(y.astype(np.float32)), "noise": torch.from_numpy(z.astype(np.float32))}[case.given]


@torch.no_grad()
def oracle(case, dtype, y_T, z, trace=None):
    """y_0 of the case's loop in `dtype` from the start state and noise given (float64 arrays)."""
    net, T = NETS[case.net]
    plan, p = zero_net(case.net)
    cond = cond_of(case.net, case.B)
    y_T, z = torch.from_numpy(y_T).to(dtype), torch.from_numpy(z).to(dtype)
    pl = ref_plans(case)
    if case.kind == "plain":
        dbl = (lambda d: {k: v.to(dtype) for k, v in d.items()})
        bufs = O.schedule_buffers(1.0 - O.cosine_betas(T))
        zd = {i: z[k] for k, i in enumerate(range(T - 1, 1, -1))}
        return O.ddpm_sample(dbl(p), plan, dbl(bufs), T, cond.to(dtype), OMEGA, y_T, zd, trace=trace)
    if case.kind == "plan":
        return R.sample_plan(p, plan, pl, T, cond, OMEGA, y_T, z, dtype=dtype, trace=trace)
    if case.kind == "dpmpp":
        return MR.sample_multistep(p, plan, pl, T, cond, OMEGA, y_T, z, dtype=dtype, trace=trace)
    if case.kind == "guided":
        return G.sample_guided(p, plan, pl, T, cond, OMEGA, G.masks(T)[case.arg], y_T, z, dtype=dtype, trace=trace)
    rows, var = case.arg
    omegas = [OMEGA] * len(pl) if var is None else [v[0] for v in var]
    return VR.sample_variants(p, plan, T, cond, rows, pl, omegas, y_T, z, dtype=dtype)


@functools.lru_cache(maxsize=None)
def reference(cid):
    """Ref of a case, computed once per process."""
    case = CASE[cid]
    (y, z), (yf, zf) = draws(case), draws(case, f32=True)
    r32 = lambda a: a.astype(np.float32).astype(np.float64)
    if case.given == "y_T":
        y = yf = r32(y)
    if case.given == "noise":
        z = zf = r32(z)
    t64, t32, tf = [], [], []
    y64 = oracle(case, torch.float64, y, z, t64)
    y32 = oracle(case, torch.float32, y, z, t32)
    yf64 = oracle(case, torch.float64, yf, zf, tf)
    e32, resp = rel(y32, y64), rel(yf64, y64)
    steps = [(j, a, FACTOR * (rel(b, a) + rel(c, a))) for (j, a, _), (_, b, _), (_, c, _) in zip(t64, t32, tf)]
    return Ref(y64, FACTOR * (e32 + resp), e32, resp, steps)


@functools.lru_cache(maxsize=None)
def box_muller_unit():
    """(absolute, relative to max(1, |z|)) largest deviation of the float32-evaluated Box-Muller from the float64 one on the same float32
    uniforms, over 2^20 draws: the unit of the draw bound."""
    z, zf = P.normals(123, 0, 1 << 20), P.normals(123, 0, 1 << 20, f32=True)
    d = np.abs(zf.astype(np.float64) - z)
    return float(d.max()), float((d / np.maximum(1.0, np.abs(z))).max())


def draw_bound(z_ref):
    """|z_dev - z_ref| <= FACTOR x unit x max(1, |z_ref|), elementwise."""
    return FACTOR * box_muller_unit()[1] * np.maximum(1.0, np.abs(z_ref))
