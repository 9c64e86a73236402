"""Per-step guidance weights without a device: the C ABI declares the setter (no stream), `steps.with_guidance` shares
the plan's tensors and keeps its bounds, the two mask constructors, the Python layer refuses malformed schedules before any device is
touched, the parity cases of tests/test_gpu_guidance.py have the error budgets their bound assumes, and one cell of the quality table
is pinned with the CPU oracle."""
import json
import os
import re

import pytest
import torch

import guidance_ref as G
import steps_ref as R
from _util import GOLD, ROOT
from test_steps_cpu import make_ddpm


# ------------------------------------------------------------------------------------------------ C ABI
def test_header_and_binding_declare_the_setter():
    import ctypes
    from diffsg_amd import _lib
    with open(os.path.join(ROOT, "include", "diffsg.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    m = re.search(r"\bint\s+dsg_set_step_guidance\s*\(([^()]*)\)\s*;", hdr)
    assert m, "include/diffsg.h does not declare dsg_set_step_guidance"
    assert [a.strip() for a in m.group(1).split(",")] == ["dsg_handle* h", "const float* g_host", "int n"]
    res, args = _lib._SIGS["dsg_set_step_guidance"]
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.c_int]
    assert hasattr(_lib.lib(), "dsg_set_step_guidance")


def test_the_setter_takes_no_stream():
    """By design: a settings call like dsg_set_step_grid (it synchronises the handle's device before it overwrites its buffer)."""
    import test_streams_cpu as S
    assert "dsg_set_step_guidance" not in S.stream_functions()
    assert "dsg_sample" in S.stream_functions()


def test_the_update_keeps_its_two_kernels_and_gains_two():
    with open(os.path.join(ROOT, "diffsg_amd", "csrc", "dsg_kernels.hpp")) as f:
        src = f.read()
    names = re.findall(r"__global__\s+__launch_bounds__\(256\)\s+void\s+(k_update\w*)\s*\(", src)
    assert names == ["k_update", "k_update_var", "k_update_sched", "k_update_var_sched"]


# ------------------------------------------------------------------------------------------------ with_guidance, the masks
def test_with_guidance_shares_tensors():
    from diffsg_amd import steps
    from diffsg_amd.steps import StepPlan
    T = 8
    d = make_ddpm(T)
    base = steps.ddim(d, 5, 0.5)
    assert base.guidance is None
    assert StepPlan(base.taus, base.t, base.coef, base.renorm_steps).guidance is None          # four-argument construction keeps working
    g = [1.0, 0.0, 0.5, 0.0, 1.0]
    p = steps.with_guidance(base, g)
    assert p.taus is base.taus and p.t is base.t and p.coef is base.coef and p.renorm_steps == base.renorm_steps
    assert p.guidance.dtype == torch.float32 and p.guidance.tolist() == g
    assert steps.with_guidance(p, None).guidance is None
    assert steps.with_renorm(p, 2).guidance is p.guidance                   # with_renorm keeps the schedule
    ident = steps.with_guidance(d, [1.0] * T)
    assert ident.taus == tuple(range(T)) and ident.coef is d._coef_table() and ident.renorm_steps == min(T, 4)
    assert torch.equal(ident.t, torch.arange(T) / T)
    for bad in ([1.0] * 4, [1.0] * 6, [1.0, -1e-9, 1.0, 1.0, 1.0], [float("nan")] + [1.0] * 4, [float("inf")] + [1.0] * 4, [[1.0] * 5] * 2):
        with pytest.raises(ValueError, match="guidance"):
            steps.with_guidance(base, bad)
    with pytest.raises(ValueError, match="guidance"):
        steps.with_guidance(d, [1.0] * (T - 1))


def test_masks():
    from diffsg_amd import steps
    g = steps.guidance_interval(20, 5, 14)
    assert g.dtype == torch.float32 and g.tolist() == [1.0 if 5 <= j <= 14 else 0.0 for j in range(20)]
    assert steps.guidance_interval(4, 0, 3).tolist() == [1.0] * 4 and steps.guidance_interval(4, 2, 2).tolist() == [0.0, 0.0, 1.0, 0.0]
    assert steps.guidance_every(20, 2).tolist() == [1.0 if j % 2 == 0 else 0.0 for j in range(20)]
    assert steps.guidance_every(20, 3, 1).tolist() == [1.0 if j % 3 == 1 else 0.0 for j in range(20)]
    assert steps.guidance_every(5, 1).tolist() == [1.0] * 5
    assert int(steps.guidance_every(20, 3, 1).sum()) == 7                  # 27 passes out of 40
    for bad in (lambda: steps.guidance_interval(4, -1, 2), lambda: steps.guidance_interval(4, 3, 2), lambda: steps.guidance_interval(4, 0, 4),
                lambda: steps.guidance_every(4, 0), lambda: steps.guidance_every(4, 2, 2), lambda: steps.guidance_every(4, 2, -1)):
        with pytest.raises(ValueError):
            bad()
    # the reference's masks are these
    assert G.table_mask("interval5_14", 20) == steps.guidance_interval(20, 5, 14).tolist()
    assert G.table_mask("even", 20) == steps.guidance_every(20, 2).tolist() and G.table_mask("third", 20) == steps.guidance_every(20, 3, 1).tolist()
    assert [G.passes_of(r, 20) for r in G.TABLE_MASKS] == [40, 30, 30, 27]


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_need_no_device():
    from diffsg_amd import steps
    from diffsg_amd.steps import StepPlan
    T = 8
    d = make_ddpm(T)
    cond = torch.zeros(96, 3)
    a = steps.strided(d, 5)
    one = torch.ones(5)
    for bad, what in ((torch.ones(4), "shape"), (torch.ones(5, 1), "shape"), (torch.ones(5, dtype=torch.float64), "float32"),
                      ([1.0] * 5, "float32"), (one.clone().index_fill_(0, torch.tensor([2]), -1.0), ">= 0"),
                      (one.clone().index_fill_(0, torch.tensor([0]), float("nan")), "finite"),
                      (one.clone().index_fill_(0, torch.tensor([4]), float("inf")), "finite")):
        plan = StepPlan(a.taus, a.t, a.coef, a.renorm_steps, bad)
        for call in (lambda: d.sample(cond, 1.0, plan=plan), lambda: d.sample_chunked(cond, 1.0, 32, plan=plan),
                     lambda: d.sample_best(cond, cond, 2, variants=[(1.0, plan)])):
            with pytest.raises(ValueError, match="guidance.*" + re.escape(what)):
                call()
    # a well-formed schedule gets as far as the device check
    good = steps.with_guidance(a, [1.0, 0.0, 1.0, 0.0, 0.5])
    with pytest.raises(RuntimeError, match="not on a HIP device"):
        d.sample(cond, 1.0, plan=good)
    with pytest.raises(RuntimeError, match="not on a HIP device"):
        d.sample_chunked(cond, 1.0, 32, plan=good)


def test_variants_share_the_schedule():
    from diffsg_amd import steps
    T = 8
    d = make_ddpm(T)
    cond = torch.zeros(96, 3)
    g = [1.0, 0.0, 1.0, 0.0, 1.0]
    a, b = steps.with_guidance(steps.strided(d, 5), g), steps.with_guidance(steps.ddim(d, 5, 0.5), list(g))      # equal values, another tensor
    c = steps.with_renorm(a, 0)
    with pytest.raises(RuntimeError, match="not on a HIP device"):
        d.sample_chunked(cond, 1.0, 32, variants=[(2.0, a), (-1.0, b), (500.0, c)])
    other = steps.with_guidance(a, [1.0, 1.0, 1.0, 0.0, 1.0])
    with pytest.raises(ValueError, match="variant 2.*guidance"):
        d.sample_chunked(cond, 1.0, 32, variants=[(2.0, a), (-1.0, b), (500.0, other)])
    with pytest.raises(ValueError, match="variant 1.*guidance"):
        d.sample_chunked(cond, 1.0, 32, variants=[(2.0, a), (-1.0, steps.with_guidance(a, None)), (500.0, c)])
    with pytest.raises(ValueError, match="variant 1.*guidance"):
        d.sample_best(cond, cond, 4, variants=[(2.0, steps.strided(d, 5)), (2.0, a)])
    ident = steps.with_guidance(d, [1.0, 0.0] * 4)
    with pytest.raises(ValueError, match="variant 1.*guidance"):
        d.sample_chunked(cond, 1.0, 32, variants=[(2.0, ident), (2.0, None), (1.0, ident)])          # None is the identity plan without a schedule


# ------------------------------------------------------------------------------------------------ the reference and its budgets
def test_reference_with_ones_is_steps_ref_and_counts_passes():
    name, sampler, omega = "tiny", "ddim0.5", 2.0
    T, K = G.NETS[name]
    net, p = G.net_params(name)
    cond, y_T, z = G.inputs(name)
    plan = G.case_plan(name, sampler)
    ones = G.sample_guided(p, net, plan, T, cond, omega, [1.0] * K, y_T, z[:K - 2])
    assert torch.equal(ones, R.sample_plan(p, net, plan, T, cond, omega, y_T, z[:K - 2]))
    passes = []
    zeros = G.sample_guided(p, net, plan, T, cond, 500.0, [0.0] * K, y_T, z[:K - 2], passes=passes)
    assert passes == [1] * K
    assert torch.equal(zeros, R.sample_plan(p, net, plan, T, cond, 0.0, y_T, z[:K - 2]))
    passes = []
    G.sample_guided(p, net, plan, T, cond, omega, G.masks(K)["even"], y_T, z[:K - 2], passes=passes)
    assert passes == [1, 2, 1, 2]                      # step index 3 runs first


@pytest.mark.parametrize("name", list(G.NETS))
def test_budgets_of_the_gpu_cases(name):
    """The reference's own float32-against-float64 error of every case tests/test_gpu_guidance.py compares with it: at most CAP / 2, so
    that the bound TOL + 3 x budget stays within 2.5 x TOL (msr80: under the golden's weight seed, the rule of DESIGN.md 7.1)."""
    from test_gpu_guidance import PARITY
    worst = 0.0
    for sampler, mask in PARITY:
        for omega in G.OMEGAS:
            b = G.budget(name, sampler, mask, omega)
            worst = max(worst, b)
            assert b <= G.CAP / 2, (name, sampler, mask, omega, b)
    print(f"{name}: worst budget {worst:.2e}")


# ------------------------------------------------------------------------------------------------ the quality table
def test_pinned_cell_of_the_quality_table():
    """The checkpoint's first 128 rows with the golden's own draws, every step guided against the even step indices only."""
    with open(os.path.join(GOLD, "g19_guidance.json")) as f:
        gold = json.load(f)
    pin = gold["pinned"]
    assert pin["rows"] == G.PIN_ROWS
    for row in ("all", "even"):
        got = G.nu_golden_cell(row, G.PIN_ROWS)
        assert abs(got - pin[row]) <= 2e-6, (row, got, pin[row])
    # the table's shape: what DESIGN.md 16 quotes
    assert set(gold["T20"]) == set(G.TABLE_MASKS) and [gold["T20"][r]["passes"] for r in G.TABLE_MASKS] == [40, 30, 30, 27]
    assert gold["K10ddim0"]["all"]["passes"] == 20 and gold["K10ddim0"]["even"]["passes"] == 15
