"""CPU reference of chunk variants (DDPM.sample_chunked(variants=...), dsg_set_chunk_variants), written independently of
the package:

  * a variants call is a loop over the chunks of `steps_ref.sample_plan`, each chunk with its own omega, coefficient table, renorm
    count and its own rows of the inputs (a chunk IS an independent sample() call);
  * the cases that tests/test_variants_cpu.py (budgets) and tests/test_gpu_variants.py (parity, bit-identity) share;
  * the best-of-n quality table of the NU checkpoint over sampler settings (tests/golden/g18_variants.json), with the oracle's
    decoder and evaluator.
"""
import functools
from collections import namedtuple

import torch

import steps_ref as R
from _util import synth_params
from oracle import ddpm_oracle as O
from weights import CONFIGS

# one chunk's setting: omega, the table ("identity": all T trained steps; otherwise a key of steps_ref.SAMPLERS on the net's K-step grid)
# and the number of early renormalised steps
V = namedtuple("V", "omega table renorm")
Case = namedtuple("Case", "name net B chunk_rows variants")

# chunk_rows = 32 with B = 150: five chunks, the last of 22 rows; n = 750 elements (450 on tiny) is no multiple of 4: the scalar path of the
# update.  B = 160: n = 800 (480), the quad path.  chunk_rows = 64 with B = 192: two row tiles per chunk.  Every chunk of a case differs
# from the others; between them renorm counts 0, 1, 4 and K and the three tables on one grid.
#
# omega: {2, -1, 500} on `tiny`, the omega = 500 chunks without renorm steps; on the NU checkpoint the cases compared with this reference
# keep to {2, -1}.  At omega = 500 the reference's own float32 arithmetic reproduces its float64 value only loosely, and how loosely depends
# on the rows and on the machine's float32 kernels: on the checkpoint 6e-6 .. 1.4e-5 without renorm steps and up to 3e-1 with them (four
# tables, renorm counts 0 .. 4 and K, nine row slices) -- never below steps_ref.CAP with room; on `tiny` 4e-7 .. 1.4e-6 without renorm steps
# (weight seeds 3 .. 5) but 1e-6 .. 2e-4 with them, and the same chunk measured 2.5e-6 on one machine and 6.9e-6 on another.  A bound derived
# from such a budget tests nothing.  omega = 500 with renorm steps, and on the checkpoint, is in BIT_ONLY: cases for the bit-for-bit
# comparisons with the chunks' own sample() calls, which need no reference and no budget.
CASES = (
    Case("nu3-T20-b150", "nu3", 150, 32, (V(2.0, "identity", 4), V(-1.0, "identity", 0), V(2.0, "identity", 1), V(-1.0, "identity", 20),
                                          V(2.0, "identity", 2))),
    Case("nu3-K10-b160", "nu3", 160, 32, (V(2.0, "strided", 4), V(-1.0, "ddim0", 0), V(2.0, "ddim0.5", 1), V(-1.0, "ddim0.5", 10),
                                          V(-1.0, "strided", 2))),
    Case("nu3-K10-b192-c64", "nu3", 192, 64, (V(-1.0, "ddim0", 0), V(2.0, "strided", 10), V(-1.0, "ddim0.5", 4))),
    Case("tiny-K4-b150", "tiny", 150, 32, (V(2.0, "strided", 4), V(-1.0, "ddim0", 0), V(500.0, "ddim0.5", 0), V(2.0, "ddim0.5", 1),
                                           V(-1.0, "strided", 3))),
    Case("tiny-T8-b160", "tiny", 160, 32, (V(-1.0, "identity", 8), V(2.0, "identity", 0), V(500.0, "identity", 0), V(-1.0, "identity", 1),
                                           V(2.0, "identity", 3))),
)
BIT_ONLY = (
    Case("nu3-T20-b150-w500", "nu3", 150, 32, (V(2.0, "identity", 4), V(-1.0, "identity", 0), V(500.0, "identity", 1), V(500.0, "identity", 20),
                                               V(-1.0, "identity", 2))),
    Case("nu3-K10-b160-w500", "nu3", 160, 32, (V(500.0, "strided", 4), V(-1.0, "ddim0", 0), V(500.0, "ddim0.5", 1), V(2.0, "ddim0.5", 10),
                                               V(500.0, "ddim0", 2))),
    Case("nu3-K10-b192-c64-w500", "nu3", 192, 64, (V(500.0, "ddim0", 0), V(2.0, "strided", 10), V(500.0, "ddim0.5", 4))),
    Case("tiny-T8-b160-w500", "tiny", 160, 32, (V(500.0, "identity", 8), V(2.0, "identity", 0), V(500.0, "identity", 4), V(500.0, "identity", 1),
                                                V(-1.0, "identity", 3))),
)
CASE = {c.name: c for c in CASES + BIT_ONLY}
# Synthetic "trained" weights of `tiny`: the first seed from 3 upwards at which every chunk of every tiny case has a budget of at most
# steps_ref.CAP / 2 (the rule of DESIGN.md 7.1; tests/test_variants_cpu.py re-derives it)
TINY_SEED = 3


def steps_of(case):
    """Number of steps of the case's call: T for identity tables, the net's K otherwise (one grid per call)."""
    T, K = R.NETS[case.net]
    kinds = {v.table == "identity" for v in case.variants}
    assert len(kinds) == 1, "the variants of one call share the step grid"
    return T if kinds.pop() else K


def ref_plan(net, v):
    T, K = R.NETS[net]
    if v.table == "identity":
        return R.plan_of(T, "identity", renorm_steps=v.renorm)
    kind, eta = R.SAMPLERS[v.table]
    return R.plan_of(T, kind, K, eta, renorm_steps=v.renorm)


def net_params(net, seed=None):
    if net == "nu3":
        return R.net_params("nu3")
    return synth_params(net, TINY_SEED if seed is None else seed)


@functools.lru_cache(maxsize=None)
def inputs(net, B):
    """cond [B][C], y_T [B][D], noise [T-2][B][D] (a K-step call uses its first K-2 rows); read-only by convention.  nu3: the first B rows of
    the checkpoint golden's own inputs."""
    T, _ = R.NETS[net]
    cfg = CONFIGS[net]
    if net == "nu3":
        g = R.nu_golden()
        return (torch.from_numpy(g["cond"])[:B].contiguous(), torch.from_numpy(g["y_T"])[:B].contiguous(),
                torch.from_numpy(g["z"])[:, :B].contiguous())
    gen = torch.Generator().manual_seed(1800 + T + B)
    return (torch.rand(B, cfg["cond_dim"], generator=gen), torch.randn(B, cfg["input_dim"], generator=gen),
            torch.randn(T - 2, B, cfg["input_dim"], generator=gen))


def chunk_slices(B, chunk_rows):
    return [slice(lo, min(lo + chunk_rows, B)) for lo in range(0, B, chunk_rows)]


def sample_variants(p, net_plan, T, cond, chunk_rows, plans, omegas, y_T, noise, dtype=torch.float32):
    """y_0 [B][D] of a variants call: chunk c is `steps_ref.sample_plan` on its own rows with plans[c] / omegas[c]."""
    out = []
    for c, sl in enumerate(chunk_slices(cond.shape[0], chunk_rows)):
        out.append(R.sample_plan(p, net_plan, plans[c], T, cond[sl], omegas[c], y_T[sl], noise[:, sl], dtype=dtype))
    return torch.cat(out)


@functools.lru_cache(maxsize=None)
def reference(name, seed=None):
    """(y_0 float32, y_0 float64) of a case, computed once per process."""
    case = CASE[name]
    T, _ = R.NETS[case.net]
    K = steps_of(case)
    net_plan, p = net_params(case.net, seed)
    cond, y_T, z = inputs(case.net, case.B)
    plans = [ref_plan(case.net, v) for v in case.variants]
    omegas = [v.omega for v in case.variants]
    return tuple(sample_variants(p, net_plan, T, cond, case.chunk_rows, plans, omegas, y_T, z[:K - 2], dtype=dt)
                 for dt in (torch.float32, torch.float64))


def chunk_budgets(name, seed=None):
    """The reference's own float32-against-float64 error of every chunk of a case (a chunk is a call: its error is its own)."""
    case = CASE[name]
    y32, y64 = reference(name, seed)
    return [R.rel(y32[sl], y64[sl]) for sl in chunk_slices(case.B, case.chunk_rows)]


# ------------------------------------------------------------------------------------------------ best-of-n over sampler settings
RENORM_CYCLE = (4, 0, 2, 1, 3)
OMEGA_CYCLE = (500.0, 200.0, 2000.0, 50.0)


def round_setting(row, r):
    """(omega, renorm count) of round r under a row of the quality table: "same" | "renorm" | "renorm+omega" | "omega"."""
    omega = OMEGA_CYCLE[r % len(OMEGA_CYCLE)] if row in ("renorm+omega", "omega") else 500.0
    renorm = RENORM_CYCLE[r % len(RENORM_CYCLE)] if row in ("renorm", "renorm+omega") else 4
    return omega, renorm


@functools.lru_cache(maxsize=None)
def nu_round_rate(seed, omega, renorm, K, rows):
    """Rate [rows] of one round on the NU checkpoint's first `rows` test rows: y_T = randn(rows, 5) then z = randn(K-2, rows, 5) from
    torch.Generator().manual_seed(seed); K = T: all trained steps (the trained table), otherwise DDIM eta = 0 on the K-step grid."""
    g = R.nu_golden()
    T, P = int(g["T"]), float(g["P_sum"])
    net_plan, p = R.net_params("nu3")
    gen = torch.Generator().manual_seed(seed)
    y_T = torch.randn(rows, 5, generator=gen)
    z = torch.randn(K - 2, rows, 5, generator=gen)
    plan = R.plan_of(T, "identity", renorm_steps=renorm) if K == T else R.plan_of(T, "ddim", K, 0.0, renorm_steps=renorm)
    cond = torch.from_numpy(g["cond"])[:rows]
    y0 = R.sample_plan(p, net_plan, plan, T, cond, omega, y_T, z)
    Xs = cond.clone(); Xs[:, 0::2] *= 400; Xs[:, 1::2] *= 400
    return O.nu_rate(O.nu_decode(y0.float(), 400, 400, P), Xs)


def label_rate(rows):
    g = R.nu_golden()
    P = float(g["P_sum"])
    Xs = torch.from_numpy(g["cond"])[:rows].clone(); Xs[:, 0::2] *= 400; Xs[:, 1::2] *= 400
    Yt = torch.from_numpy(g["y_test"])[:rows].clone(); Yt[:, 0] *= 400; Yt[:, 1] *= 400; Yt[:, 2:] *= P
    return O.nu_rate(Yt, Xs)


def best_of_ratio(row, seeds, K=20, rows=512):
    """Sum over the rows of the best round's rate / sum of the stored labels' rate; round r runs `round_setting(row, r)` on seeds[r]."""
    rates = torch.stack([nu_round_rate(s, *round_setting(row, r), K, rows) for r, s in enumerate(seeds)])
    return float(rates.max(dim=0).values.sum() / label_rate(rows).sum())


# The pinned cell (tests/test_variants_cpu.py): best-of-8 on the first PIN_ROWS rows, seeds PIN_SEEDS, renorm count cycled against seeds only
PIN_ROWS, PIN_SEEDS = 128, tuple(range(101, 109))
