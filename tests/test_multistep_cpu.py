"""Two-step solver plans without a device: `steps.dpmpp_2m` matches the independent table of tests/multistep_ref.py, the
two-step rule beats DDIM on an analytic denoiser by the factor the feature was proposed on, `steps.logsnr_taus`, the C ABI declares the
setter (no stream), the Python layer refuses malformed histories before any device is touched, the parity cases of
tests/test_gpu_multistep.py have the error budgets their bound assumes, and the NU checkpoint's cells are the recorded ones."""
import json
import os
import re

import numpy as np
import pytest
import torch

import multistep_ref as M
import steps_ref as R
from _util import GOLD, ROOT
from test_steps_cpu import make_ddpm


def row_ulps(got, ref):
    """Largest distance between two float32 tables in units of one float32 ulp of each row's largest coefficient."""
    got, ref = np.asarray(got, dtype=np.float32), np.asarray(ref, dtype=np.float32)
    assert got.shape == ref.shape
    top = np.maximum(np.abs(got).max(axis=1), np.abs(ref).max(axis=1)).astype(np.float32)
    ulp = np.spacing(top).astype(np.float64)
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64)).max(axis=1)
    return float((d / np.where(ulp > 0, ulp, 1.0)).max())


# ------------------------------------------------------------------------------------------------ C ABI
def test_header_and_binding_declare_the_setter():
    import ctypes
    from diffsg_amd import _lib
    with open(os.path.join(ROOT, "include", "diffsg.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    m = re.search(r"\bint\s+dsg_set_step_history\s*\(([^()]*)\)\s*;", hdr)
    assert m, "include/diffsg.h does not declare dsg_set_step_history"
    assert [a.strip() for a in m.group(1).split(",")] == ["dsg_handle* h", "const float* hist_host", "int n"]
    res, args = _lib._SIGS["dsg_set_step_history"]
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.c_int]
    assert hasattr(_lib.lib(), "dsg_set_step_history")


def test_the_setter_takes_no_stream():
    """By design: a settings call like dsg_set_step_guidance (it synchronises the handle's device before it overwrites its buffer)."""
    import test_streams_cpu as S
    assert "dsg_set_step_history" not in S.stream_functions()
    assert "dsg_sample" in S.stream_functions()


def test_the_history_kernels_live_in_their_own_header():
    with open(os.path.join(ROOT, "diffsg_amd", "csrc", "dsg_multistep.hpp")) as f:
        src = f.read()
    names = re.findall(r"__global__\s+__launch_bounds__\(256\)\s+void\s+(k_update\w*)\s*\(", src)
    assert names == ["k_update_hist", "k_update_hist_sched"]


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("rn", [None, 0, 1])
@pytest.mark.parametrize("name", list(M.NETS))
def test_table_matches_the_reference(name, rn):
    from diffsg_amd import steps
    T, K = M.NETS[name]
    d = make_ddpm(T)
    plan = steps.dpmpp_2m(d, K, renorm_steps=rn)
    ref = M.plan_of(T, K, rn)
    assert plan.taus == ref.taus == tuple(R.default_taus(T, K)) and torch.equal(plan.t, ref.t)
    assert plan.renorm_steps == (min(K, 4) if rn is None else rn)
    assert plan.guidance is None
    assert plan.coef.dtype == torch.float32 and tuple(plan.coef.shape) == (K, 4)
    assert plan.history.dtype == torch.float32 and tuple(plan.history.shape) == (K, 3)
    assert row_ulps(plan.coef.numpy(), ref.coef.numpy()) <= 1 and row_ulps(plan.history.numpy(), ref.history.numpy()) <= 1
    assert not plan.coef[:, 2:].any()                                        # deterministic: c3 = c4 = 0
    reads = (plan.history[:, 0] != 0).tolist()
    stores = ((plan.history[:, 1] != 0) | (plan.history[:, 2] != 0)).tolist()
    assert reads == M.second_order(K, plan.renorm_steps)
    assert stores == [False] + reads[:-1]                                    # p, q only where the next step (index j-1) reads
    if rn is not None:
        assert any(reads), "no second-order step: the case is vacuous"
    steps.check_history(plan.history, K)
    # an explicit grid gives the same plan as the default one
    again = steps.dpmpp_2m(d, taus=plan.taus, renorm_steps=rn)
    assert torch.equal(again.coef, plan.coef) and torch.equal(again.history, plan.history)


@pytest.mark.parametrize("name", list(M.NETS))
def test_all_first_order_table_is_ddim(name):
    from diffsg_amd import steps
    T, K = M.NETS[name]
    d = make_ddpm(T)
    plan = steps.dpmpp_2m(d, K, renorm_steps=K)                               # every step after a renormalised one
    assert not plan.history.any()
    assert row_ulps(plan.coef.numpy(), steps.ddim(d, K, 0.0).coef.numpy()) <= 1
    assert row_ulps(plan.coef.numpy(), R.ddim_table(R.acp64(T), R.default_taus(T, K), 0.0)) <= 1


@pytest.mark.parametrize("T,K", [(20, 8), (20, 20), (1000, 8), (1000, 10), (1000, 16), (1000, 20), (1000, 400)])
def test_logsnr_taus(T, K):
    from diffsg_amd import steps
    d = make_ddpm(T)
    taus = steps.logsnr_taus(d, K)
    assert isinstance(taus, tuple) and all(isinstance(v, int) for v in taus)
    assert taus[0] == 0 and taus[-1] == T - 1 and all(b > a for a, b in zip(taus, taus[1:])) and len(taus) <= K
    assert list(taus) == M.logsnr_taus(R.acp64(T), K)
    if (T, K) == (1000, 400):
        assert len(taus) < K                                                  # duplicates dropped: fewer points than asked for
    for make in (steps.strided, steps.ddim, steps.dpmpp_2m):
        assert make(d, taus=taus).taus == taus
    for bad in (1, T + 1):
        with pytest.raises(ValueError):
            steps.logsnr_taus(d, bad)


def test_make_knows_the_sampler():
    from diffsg_amd import steps
    d = make_ddpm(20)
    p, q = steps.make(d, 10, "dpmpp2m"), steps.dpmpp_2m(d, 10)
    assert torch.equal(p.coef, q.coef) and torch.equal(p.history, q.history) and p.renorm_steps == 4
    assert steps.make(d, None, "dpmpp2m") is None
    with pytest.raises(ValueError, match="dpmpp2m"):
        steps.make(d, 10, "heun")


# ------------------------------------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("T,grid,K", [(20, "default", 8), (20, "default", 10), (1000, "logsnr", 8), (1000, "logsnr", 10), (1000, "logsnr", 16),
                                      (1000, "logsnr", 20)])
def test_two_step_rule_beats_ddim_on_the_analytic_denoiser(T, grid, K):
    """Gaussian data N(mu, 0.3^2) per coordinate, whose probability-flow ODE has a closed solution; the plan's own float32 rows run in
    float64, no renorm.  Measured when the feature was proposed: at least 6.9x (T = 20) and 6.1x (T = 1000) -- the bound is 3x."""
    from diffsg_amd import steps
    d = make_ddpm(T)
    acp = R.acp64(T)
    taus = steps.logsnr_taus(d, K) if grid == "logsnr" else None
    two = steps.dpmpp_2m(d, None if taus else K, taus=taus, renorm_steps=0)
    one = steps.ddim(d, None if taus else K, 0.0, taus=taus)
    assert two.taus == one.taus
    e2 = M.gauss_error(two.coef.numpy(), two.history.numpy(), acp, two.taus)
    e1 = M.gauss_error(one.coef.numpy(), None, acp, one.taus)
    print(f"T = {T} {grid} K = {K} ({len(two.taus)} points): DDIM {e1:.2e}, two-step {e2:.2e}, {e1 / e2:.1f}x")
    assert e2 <= e1 / 3.0, (e1, e2)
    # the reference's table gives the same figure
    ref = M.plan_of(T, renorm_steps=0, taus=two.taus)
    assert abs(M.gauss_error(ref.coef.numpy(), ref.history.numpy(), acp, ref.taus) - e2) <= 1e-5 * e2 + 1e-12


# ------------------------------------------------------------------------------------------------ with_*, the refusals
def test_with_history_and_friends_share_tensors():
    from diffsg_amd import steps
    from diffsg_amd.steps import StepPlan
    T = 8
    d = make_ddpm(T)
    base = steps.dpmpp_2m(d, 5, renorm_steps=0)
    assert StepPlan(base.taus, base.t, base.coef, base.renorm_steps).history is None                 # four- and five-argument construction
    assert StepPlan(base.taus, base.t, base.coef, base.renorm_steps, None).history is None
    g = steps.with_guidance(base, [1.0, 0.0, 0.5, 0.0, 1.0])
    assert g.history is base.history and g.coef is base.coef and g.t is base.t                    # with_guidance keeps the history
    assert steps.with_guidance(g, None).history is base.history
    none = steps.with_history(g, None)
    assert none.history is None and none.guidance is g.guidance and none.coef is base.coef
    rows = base.history.tolist()
    h = steps.with_history(steps.ddim(d, 5), rows)
    assert h.history.dtype == torch.float32 and h.history.tolist() == rows and h.guidance is None
    ident = steps.with_history(d, [[0.0, 0.0, 0.0]] * T)
    assert ident.taus == tuple(range(T)) and ident.coef is d._coef_table() and ident.renorm_steps == min(T, 4)
    with pytest.raises(ValueError, match="history"):
        steps.with_renorm(base, 2)                                                                  # the table depends on the count
    assert steps.with_renorm(none, 2).renorm_steps == 2


def bad_histories(K):
    """[(rows, what the message names)]: every refusal of check_history / dsg_set_step_history on well-shaped input."""
    ok = [[0.0, 1.0, -1.0]] * K
    first = [list(r) for r in ok]; first[K - 1][0] = 0.5
    orphan = [[0.0, 0.0, 0.0] for _ in range(K)]; orphan[1][0] = -0.25            # row 2 stores nothing
    nan = [list(r) for r in ok]; nan[2][1] = float("nan")
    inf = [list(r) for r in ok]; inf[0][2] = float("-inf")
    return [(first, "first step"), (orphan, "stores none"), (nan, "finite"), (inf, "finite")]


def test_refusals_need_no_device():
    from diffsg_amd import steps
    from diffsg_amd.steps import StepPlan
    T, K = 8, 5
    d = make_ddpm(T)
    cond = torch.zeros(96, 3)
    a = steps.ddim(d, K)
    shaped = [(torch.zeros(K - 1, 3), "shape"), (torch.zeros(K, 4), "shape"), (torch.zeros(K * 3), "shape"),
              (torch.zeros(K, 3, dtype=torch.float64), "float32"), ([[0.0] * 3] * K, "float32")]
    valued = [(torch.tensor(rows, dtype=torch.float32), what) for rows, what in bad_histories(K)]
    for bad, what in shaped + valued:
        with pytest.raises(ValueError, match="history.*" + re.escape(what)):
            steps.check_history(bad, K)
        plan = StepPlan(a.taus, a.t, a.coef, a.renorm_steps, None, bad)
        for call in (lambda: d.sample(cond, 1.0, plan=plan), lambda: d.sample_chunked(cond, 1.0, 32, plan=plan)):
            with pytest.raises(ValueError, match="history.*" + re.escape(what)):
                call()
    for rows, what in bad_histories(K):
        with pytest.raises(ValueError, match="history.*" + re.escape(what)):
            steps.with_history(a, rows)
    with pytest.raises(ValueError, match="history"):
        steps.with_history(a, [[0.0] * 3] * (K + 1))
    for bad in (lambda: steps.dpmpp_2m(d, T + 1), lambda: steps.dpmpp_2m(d, 1), lambda: steps.dpmpp_2m(d, K, renorm_steps=K + 1),
                lambda: steps.dpmpp_2m(d, K, renorm_steps=-1), lambda: steps.dpmpp_2m(d, taus=[0, 3, 3, 7])):
        with pytest.raises(ValueError):
            bad()
    # variants refuse a plan with a history before any device work, naming the variant
    good = steps.dpmpp_2m(d, K, renorm_steps=0)
    with pytest.raises(ValueError, match="variant 1.*history"):
        d.sample_chunked(cond, 1.0, 32, variants=[(2.0, a), (1.0, good), (1.0, a)])
    with pytest.raises(ValueError, match="variant 0.*history"):
        d.sample_best(cond, cond, 2, variants=[(2.0, good)])
    # a well-formed plan gets as far as the device check
    for call in (lambda: d.sample(cond, 1.0, plan=good), lambda: d.sample_chunked(cond, 1.0, 32, plan=good),
                 lambda: d.sample(cond, 1.0, plan=steps.with_guidance(good, [1.0, 0.0, 1.0, 0.0, 0.5]))):
        with pytest.raises(RuntimeError, match="not on a HIP device"):
            call()


# ------------------------------------------------------------------------------------------------ the reference and its budgets
def test_reference_without_second_order_steps_is_steps_ref():
    name, omega = "tiny", 2.0
    T, K = M.NETS[name]
    net, p = M.net_params(name)
    cond, y_T, z = M.inputs(name)
    first = M.plan_of(T, K, K)
    assert not first.history.any()
    ddim = R.plan_of(T, "ddim", K, 0.0, renorm_steps=K)
    assert R.rel(first.coef, ddim.coef) <= 2e-7
    as_ddim = M.Plan(first.taus, first.t, first.coef, first.renorm_steps, None)
    assert torch.equal(M.sample_multistep(p, net, first, T, cond, omega, y_T, None),
                       R.sample_plan(p, net, as_ddim, T, cond, omega, y_T, None))
    second = M.plan_of(T, K, 0)
    assert not torch.equal(M.sample_multistep(p, net, second, T, cond, omega, y_T, None),
                           M.sample_multistep(p, net, M.Plan(*second[:4], None), T, cond, omega, y_T, None))


@pytest.mark.parametrize("name", list(M.NETS))
def test_budgets_of_the_gpu_cases(name):
    """The reference's own float32-against-float64 error of every case tests/test_gpu_multistep.py compares with it: at most CAP = 1e-5.
    Synthetic nets: the weight seed is the first from 3 upwards whose budgets are at most CAP / 2 = 5e-6, with the
    second-order cases at renorm_steps = 0 -- the fallback to 1 (no such seed up to 10) was not needed for either net:
    seed 3 has 1.4e-6 (tiny) and 1.7e-6 (msr3)."""
    assert M.SECOND[name] == 0
    T, K = M.NETS[name]
    for which in ("default", "second"):
        has_second = bool((M.plan_of(T, K, M.renorm_of(name, which)).history[:, 0] != 0).any())
        assert has_second or which == "default"
    b = M.budgets(name)
    for key, v in b.items():
        print(f"{name} {key}: budget {v:.2e}")
    assert max(b.values()) <= (M.CAP if name == "nu3" else M.CAP / 2), b
    if name != "nu3":
        for seed in range(3, M.SEEDS[name]):
            assert max(M.budgets(name, seed).values()) > M.CAP / 2, f"seed {seed} already meets the cap: the rule picks it"


# ------------------------------------------------------------------------------------------------ the quality table
QUOTED = {(10, 4): (0.90690, 0.90327), (10, 0): (0.90342, 0.90358), (7, 4): (0.88172, 0.86451), (7, 0): (0.90299, 0.90299),
          (5, 4): (0.87357, 0.87357), (5, 0): (0.90389, 0.90394)}


def test_nu_checkpoint_cells_are_the_recorded_ones():
    """The shipped NU checkpoint (512 rows, T = 20, omega = 500) under DDIM eta = 0 and the two-step rule: recomputed here, within 2e-5 of
    tests/golden/g18_multistep.json, which agrees with the six pairs the feature was proposed on (quoted to five digits)."""
    with open(os.path.join(GOLD, "g18_multistep.json")) as f:
        rec = json.load(f)
    assert (rec["omega"], rec["rows"], rec["T"]) == (500.0, 512, 20)
    got = M.nu_cells()
    assert sorted(got) == sorted(rec["ratios"])
    for k in got:
        print(f"{k}: {got[k]:.6f} (recorded {rec['ratios'][k]:.6f})")
    for k in got:
        assert abs(got[k] - rec["ratios"][k]) <= 2e-5, (k, got[k], rec["ratios"][k])
    for (K, rn), (ddim, two) in QUOTED.items():
        assert abs(rec["ratios"][f"K{K}_r{rn}_ddim0"] - ddim) <= 1e-5 and abs(rec["ratios"][f"K{K}_r{rn}_2m"] - two) <= 1e-5, (K, rn)
    # DDIM's cells with 4 renorm steps are the ones tests/golden/g17_steps.json records
    with open(os.path.join(GOLD, "g17_steps.json")) as f:
        g17 = json.load(f)["ratios"]
    for K in M.CELL_KS:
        assert abs(rec["ratios"][f"K{K}_r4_ddim0"] - g17[f"K{K}_ddim0"]) <= 2e-5
