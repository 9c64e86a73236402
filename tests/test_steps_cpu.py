"""Step plans without a device: the C ABI declares the setter, the plan tables match the independent CPU reference (tests/steps_ref.py),
that reference is tied to the oracle the goldens pin, the NU checkpoint's K-step task metric is the recorded one, the parity cases of
tests/test_gpu_steps.py have the error budgets their bound assumes, and malformed plans are refused before any device is touched."""
import json
import os
import re

import numpy as np
import pytest
import torch

import steps_ref as R
from _util import GOLD, ROOT, synth_params
from oracle import ddpm_oracle as O
from weights import CONFIGS


def make_ddpm(T, name="tiny"):
    """A DDPM on the CPU: enough for the tables and the refusals (nothing is launched)."""
    from diffsg_amd import UNet1D
    from diffsg_amd.classifier_free_MSR import DDPM
    cfg = CONFIGS[name]
    m = UNet1D(**cfg, is_attn=(False,) * len(cfg["dims"]))
    D = cfg["input_dim"]
    return DDPM(T, m, D, 10.0, 1.0 - O.cosine_betas(T), torch.device("cpu"), (1, D), None)


def ulps(a, b):
    """Largest distance in float32 units in the last place between two float32 arrays of finite values of equal sign."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape and (np.signbit(a) == np.signbit(b)).all()
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max()) if a.size else 0


# ------------------------------------------------------------------------------------------------ C ABI
def test_header_and_binding_declare_the_setter():
    from diffsg_amd import _lib
    with open(os.path.join(ROOT, "include", "diffsg.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    m = re.search(r"\bint\s+dsg_set_step_grid\s*\(([^()]*)\)\s*;", hdr)
    assert m, "include/diffsg.h does not declare dsg_set_step_grid"
    assert [a.strip() for a in m.group(1).split(",")] == ["dsg_handle* h", "const float* t_host", "int n", "int renorm_steps"]
    res, args = _lib._SIGS["dsg_set_step_grid"]
    assert len(args) == 4
    assert hasattr(_lib.lib(), "dsg_set_step_grid")


def test_the_setter_takes_no_stream():
    """By design: it does no stream-ordered work (it synchronises the handle's device, as the other settings calls)."""
    import test_streams_cpu as S
    assert "dsg_set_step_grid" not in S.stream_functions()


# ------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("T", [3, 8, 20])
def test_identity_plan_is_the_trained_table(T):
    from diffsg_amd import steps
    d = make_ddpm(T)
    for plan in (steps.strided(d, T), steps.strided(d, taus=range(T))):
        assert plan.taus == tuple(range(T))
        assert plan.coef.dtype == torch.float32 and torch.equal(plan.coef, d._coef_table())
        assert plan.t.dtype == torch.float32 and torch.equal(plan.t, torch.arange(T) / T)
        assert plan.renorm_steps == min(T, 4)
    # and the independent reference's trained table is that table too
    assert np.array_equal(R.trained_table(T), d._coef_table().numpy())


@pytest.mark.parametrize("T,K", [(20, 3), (20, 5), (20, 7), (20, 10), (1000, 50)])
def test_tables_match_the_reference(T, K):
    from diffsg_amd import steps
    d = make_ddpm(T)
    acp = R.acp64(T)
    assert np.array_equal(acp, d.alphas_cumprod.double().numpy())
    taus = R.default_taus(T, K)
    assert all(b > a for a, b in zip(taus, taus[1:])) and taus[0] == 0 and taus[-1] == T - 1 and len(taus) == K
    cases = [(steps.strided(d, K), R.strided_table(acp, taus))]
    for eta in (0.0, 0.5, 1.0):
        cases.append((steps.ddim(d, K, eta), R.ddim_table(acp, taus, eta)))
    for plan, ref in cases:
        assert plan.taus == tuple(taus)
        assert torch.equal(plan.t, R.times(taus, T)) and plan.t.dtype == torch.float32
        assert plan.coef.dtype == torch.float32 and tuple(plan.coef.shape) == (K, 4)
        assert ulps(plan.coef.numpy(), ref) <= 1
        assert plan.renorm_steps == min(K, 4)
        assert not plan.coef[:2, 3].any()
    # eta = 0 is noise free on every step; eta > 0 and strided are noisy from step index 2 up
    assert not steps.ddim(d, K, 0.0).coef[:, 3].any()
    assert steps.ddim(d, K, 0.5).coef[2:, 3].all() and steps.strided(d, K).coef[2:, 3].all()
    # an explicit grid gives the same plan as the default one
    assert torch.equal(steps.strided(d, taus=taus).coef, cases[0][0].coef)


@pytest.mark.parametrize("T,k", [(20, 0), (20, 1), (20, 5), (20, 19), (8, 7)])
def test_tail_reuses_the_trained_rows(T, k):
    from diffsg_amd import steps
    d = make_ddpm(T)
    plan = steps.tail(d, k)
    assert plan.taus == tuple(range(k + 1)) and plan.renorm_steps == 0
    assert torch.equal(plan.coef, d._coef_table()[:k + 1]) and torch.equal(plan.t, torch.arange(k + 1) / T)
    ref = R.plan_of(T, "tail", k=k)
    assert np.array_equal(ref.coef.numpy(), plan.coef.numpy()) and torch.equal(ref.t, plan.t)
    assert steps.tail(d, k, renorm_steps=min(2, k + 1)).renorm_steps == min(2, k + 1)


@pytest.mark.parametrize("T", [2, 3, 8, 20, 1000])
def test_default_grids(T):
    from diffsg_amd import steps
    d = make_ddpm(T)
    for K in sorted({2, 3, min(T, 7), T // 2 + 1, T - 1, T} - {0, 1}):
        if not 2 <= K <= T:
            continue
        taus = steps.strided(d, K).taus
        assert len(taus) == K and taus[0] == 0 and taus[-1] == T - 1
        assert all(isinstance(v, int) for v in taus) and all(b > a for a, b in zip(taus, taus[1:]))
        assert list(taus) == R.default_taus(T, K)
        assert steps.ddim(d, K).taus == taus


# ------------------------------------------------------------------------------------------------ the reference itself
def test_reference_loop_with_the_identity_plan_is_the_oracle():
    T, B = 8, 6
    net, p = synth_params("tiny", 31)
    g = torch.Generator().manual_seed(4)
    cond, y_T, z = torch.rand(B, 3, generator=g), torch.randn(B, 3, generator=g), torch.randn(T - 2, B, 3, generator=g)
    bufs = O.schedule_buffers(1.0 - O.cosine_betas(T))
    for omega in (0.0, 2.0):
        tr_o, tr_r = [], []
        ref = O.ddpm_sample(p, net, bufs, T, cond, omega, y_T, {i: z[j] for j, i in enumerate(range(T - 1, 1, -1))}, trace=tr_o)
        got = R.sample_plan(p, net, R.plan_of(T, "identity"), T, cond, omega, y_T, z, trace=tr_r)
        assert torch.equal(got, ref)
        assert [i for i, _, _ in tr_o] == [j for j, _, _ in tr_r]
        assert all(torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) for a, b in zip(tr_o, tr_r))


def test_nu_checkpoint_ratios_are_the_recorded_ones():
    """The task metric of the shipped NU checkpoint on K-step plans (512 rows, omega = 500): recomputed here, each within 1e-4 of
    tests/golden/g17_steps.json; the K = 10 values are the ones the feature was proposed on (0.90529 strided, 0.90690 DDIM eta = 0)."""
    with open(os.path.join(GOLD, "g17_steps.json")) as f:
        rec = json.load(f)
    assert (rec["omega"], rec["rows"], rec["T"]) == (500.0, 512, 20)
    cells = {f"K{K}_{key}": (K, kind, eta) for K in (10, 7, 5, 3)
             for key, kind, eta in (("strided", "strided", 0.0), ("ddim0", "ddim", 0.0), ("ddim1", "ddim", 1.0))}
    cells["K20_strided"] = (20, "strided", 0.0)
    assert sorted(cells) == sorted(rec["ratios"])
    got = {k: R.nu_ratio_cell(*v, omega=rec["omega"]) for k, v in cells.items()}
    for k in cells:
        print(f"{k}: {got[k]:.6f} (recorded {rec['ratios'][k]:.6f})")
    for k in cells:
        assert abs(got[k] - rec["ratios"][k]) <= 1e-4, (k, got[k], rec["ratios"][k])
    assert abs(got["K10_strided"] - 0.90529) <= 2e-3 and abs(got["K10_ddim0"] - 0.90690) <= 2e-3
    assert abs(got["K20_strided"] - 0.91359) <= 2e-3          # the trained schedule's known answer (g4_sample_nu_ckpt.npz)


# ------------------------------------------------------------------------------------------------ budgets of the GPU parity cases
@pytest.mark.parametrize("name", list(R.NETS))
def test_parity_case_budgets(name):
    """Every parity case of tests/test_gpu_steps.py: the reference's own float32-against-float64 error is at most CAP = 1e-5 (its bound
    is TOL + 3 x budget).  Synthetic nets: the weight seed is the first from 3 upwards whose budgets are at most CAP / 2."""
    def budgets(seed=None):
        out = {}
        for s in R.SAMPLERS:
            for om in R.OMEGAS:
                r = R.reference(name, s, om, seed)
                out[(s, om)] = R.rel(r.y32, r.y64)
        return out
    b = budgets()
    if name == "nu3":
        for k in R.TAIL_KS:
            for rn in (0, 2):
                if rn <= k + 1:
                    for om in R.OMEGAS:
                        a32, a64 = R.tail_reference(name, k, om, rn)
                        b[(f"tail{k}/{rn}", om)] = R.rel(a32, a64)
    for key, v in b.items():
        print(f"{name} {key}: budget {v:.2e}")
    assert max(b.values()) <= (R.CAP if name == "nu3" else R.CAP / 2), b
    if name != "nu3":
        for seed in range(3, R.SEEDS[name]):
            assert max(budgets(seed).values()) > R.CAP / 2, f"seed {seed} already meets the cap: the rule picks it"


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_need_no_device():
    from diffsg_amd import steps
    from diffsg_amd.steps import StepPlan
    T = 8
    d = make_ddpm(T)
    for bad in (lambda: steps.strided(d, T + 1), lambda: steps.strided(d, 1), lambda: steps.ddim(d, T + 1), lambda: steps.ddim(d, 1),
                lambda: steps.ddim(d, 4, eta=-0.1), lambda: steps.strided(d, taus=[0, 3, 3, 7]), lambda: steps.strided(d, taus=[0, 5, 2]),
                lambda: steps.ddim(d, taus=[0, 2, 8]), lambda: steps.strided(d, taus=[-1, 2]), lambda: steps.strided(d, 3, taus=[0, 7]),
                lambda: steps.tail(d, T), lambda: steps.tail(d, -1), lambda: steps.tail(d, 2, renorm_steps=4),
                lambda: d.refine(torch.zeros(4, 3), torch.zeros(4, 3), T)):
        with pytest.raises(ValueError):
            bad()
    cond = torch.zeros(4, 3)
    plan = steps.strided(d, 5)
    for call in (d.sample, d.sample_chunked):
        with pytest.raises(ValueError, match="noise must have shape"):
            call(cond, 1.0, plan=plan, noise=torch.zeros(T - 2, 4, 3))          # the trained schedule's shape, not the plan's (3, 4, 3)
        for row in (0, 1):
            coef = plan.coef.clone()
            coef[row, 3] = 1.0
            with pytest.raises(ValueError, match="noise free"):
                call(cond, 1.0, plan=StepPlan(plan.taus, plan.t, coef, plan.renorm_steps))
        with pytest.raises(ValueError):
            call(cond, 1.0, plan=StepPlan(plan.taus, plan.t[:-1], plan.coef, plan.renorm_steps))
        with pytest.raises(ValueError):
            call(cond, 1.0, plan=StepPlan(plan.taus, plan.t, plan.coef, 6))
    # a well-formed plan gets as far as the device check
    with pytest.raises(RuntimeError, match="not on a HIP device"):
        d.sample(cond, 1.0, plan=plan, noise=torch.zeros(3, 4, 3))
    # the plan is immutable
    with pytest.raises(Exception):
        plan.renorm_steps = 0
