"""Sampling on a step grid on the device (DDPM.sample(plan=...), dsg_set_step_grid) against the CPU reference
tests/steps_ref.py and against the library's own plan-less calls.

Bound of every comparison with the reference: `rel <= TOL + 3 x budget`, TOL = 1e-5 as in tests/test_gpu_parity.py and `budget` the
reference's own float32-against-float64 error on the same case (tests/test_steps_cpu.py caps it at 1e-5).  B = 70 rows (three row tiles,
the last ragged); nets: `tiny` (T = 8), `nu3` with the shipped checkpoint (T = 20), `msr3` (T = 12) -- between them the 128-wide, 64-wide
and narrow-run kernels.  All tests need an MI355X: run with `-m gpu`."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import steps_ref as R
from _util import GOLD
from oracle import ddpm_oracle as O
from weights import CONFIGS

pytestmark = pytest.mark.gpu

TOL = 1e-5
MODES = ("split_f16", "f32")


def make_ddpm(name, policy="default"):
    """The case's net under its problem's DDPM class (NU for nu3: decoder and objective of sample_best), on the device."""
    from diffsg_amd import UNet1D
    from diffsg_amd import classifier_free_MSR as MSR, classifier_free_NU as NU
    T, _ = R.NETS[name]
    cfg = CONFIGS[name]
    _, p = R.net_params(name)
    m = UNet1D(**cfg, is_attn=(False,) * len(cfg["dims"]))
    m.load_state_dict(p, strict=True)
    D, dev, alphas = cfg["input_dim"], torch.device("cuda"), 1.0 - O.cosine_betas(T)
    if name == "nu3":
        d = NU.DDPM(T, m.to("cuda"), D - 2, 18.0, alphas, dev, (1, D), {"width": 400, "height": 400})
    else:
        d = MSR.DDPM(T, m.to("cuda"), D, 20.0, alphas, dev, (1, D), None)
    d = d.to("cuda")
    if policy == "large":
        d.model.set_launch_policy(0, 0)
    return d


def device_plan(d, name, sampler):
    from diffsg_amd import steps
    _, K = R.NETS[name]
    kind, eta = R.SAMPLERS[sampler]
    return steps.strided(d, K) if kind == "strided" else steps.ddim(d, K, eta)


def check(got, ref32, ref64, tag):
    e, budget = R.rel(got, ref32), R.rel(ref32, ref64)
    print(f"{tag}: rel err vs reference {e:.2e} (reference float32 vs float64: {budget:.2e})")
    assert np.isfinite(e) and e <= TOL + 3.0 * budget, (tag, e, budget)


# 1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["default", "large"])
@pytest.mark.parametrize("name", list(R.NETS))
def test_identity_plan_is_the_plain_call_bit_for_bit(name, policy):
    from diffsg_amd import steps
    T, _ = R.NETS[name]
    d = make_ddpm(name, policy)
    cond, y_T, z, _ = R.inputs(name)
    cond = cond.cuda()
    plan = steps.strided(d, T)
    assert plan.coef is d._coef_table()
    for mode in MODES:
        d.model.set_precision(mode)
        for graph in (True, False):
            for omega in (2.0, -1.0):
                a = d.sample(cond, omega, y_T=y_T, noise=z, use_graph=graph)
                b = d.sample(cond, omega, y_T=y_T, noise=z, use_graph=graph, plan=plan)
                assert torch.isfinite(a).all() and torch.equal(a, b), (mode, graph, omega)
    d.model.set_precision("split_f16")


# 2 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", list(R.SAMPLERS))
@pytest.mark.parametrize("name", list(R.NETS))
def test_plans_against_the_reference(name, sampler):
    _, K = R.NETS[name]
    d = make_ddpm(name)
    cond, y_T, z, _ = R.inputs(name)
    cond = cond.cuda()
    plan = device_plan(d, name, sampler)
    for omega in R.OMEGAS:
        ref = R.reference(name, sampler, omega)
        for mode in MODES:
            d.model.set_precision(mode)
            y0 = d.sample(cond, omega, y_T=y_T, noise=z[:K - 2], plan=plan)
            check(y0, ref.y32, ref.y64, f"{name} {sampler} K={K} omega={omega:g} {mode}")
            assert torch.equal(d.sample(cond, omega, y_T=y_T, noise=z[:K - 2], plan=plan, use_graph=False), y0), (omega, mode)
    d.model.set_precision("split_f16")


# 3 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", R.TAIL_KS)
def test_tail_and_refine_against_the_reference(k):
    from diffsg_amd import steps
    name = "nu3"
    d = make_ddpm(name)
    cond, y_T, z, q = R.inputs(name)
    cond = cond.cuda()
    zz = z[:max(k - 1, 0)]
    for omega in R.OMEGAS:
        r32, r64 = R.tail_reference(name, k, omega)
        y0 = d.refine(cond, y_T, k, omega, q_noise=q, noise=zz)
        check(y0, r32, r64, f"refine k={k} omega={omega:g}")
        assert torch.equal(d.refine(cond, y_T, k, omega, q_noise=q, noise=zz, use_graph=False), y0)
        # the same through sample() on the reference's own start state, without and with early renorm steps
        for rn in (0, 2):
            if rn > k + 1:
                continue
            r32, r64 = R.tail_reference(name, k, omega, rn)
            y0 = d.sample(cond, omega, plan=steps.tail(d, k, renorm_steps=rn), y_T=R.tail_start(name, k), noise=zz)
            check(y0, r32, r64, f"tail k={k} renorm_steps={rn} omega={omega:g}")
    # q_noise drawn by torch when not given: reproducible under torch's seed, and a different draw than the injected one
    torch.manual_seed(3)
    a = d.refine(cond, y_T, k, 1.0, seed=9)
    torch.manual_seed(3)
    b = d.refine(cond, y_T, k, 1.0, seed=9)
    assert torch.equal(a, b) and torch.isfinite(a).all()


# 4 ------------------------------------------------------------------------------------------------
def test_recorded_trajectory_of_a_plan():
    from diffsg_amd.ddpm import DDPMCore
    name, sampler, omega = "nu3", "strided", 2.0
    _, K = R.NETS[name]
    d = make_ddpm(name)
    d._decode_recorded = lambda i, y: DDPMCore._decode_recorded(d, i, y)      # the raw states: what the library records
    cond, y_T, z, _ = R.inputs(name)
    D = CONFIGS[name]["input_dim"]
    plan = device_plan(d, name, sampler)
    ref = R.reference(name, sampler, omega)
    d.record_denoise_path = True
    y0 = d.sample(cond.cuda(), omega, y_T=y_T, noise=z[:K - 2], plan=plan)
    assert d.y_i_record.shape == (R.B, K * D) and d.eps_i_record.shape == (R.B, K * D)
    (y32, e32), (y64, e64) = R.trace_arrays(ref.trace32), R.trace_arrays(ref.trace64)
    check(d.y_i_record, y32, y64, "recorded y")
    check(d.eps_i_record, e32, e64, "recorded eps")
    assert np.array_equal(d.y_i_record[:, -D:], y0.cpu().numpy())
    d.record_denoise_path = False
    assert torch.equal(d.sample(cond.cuda(), omega, y_T=y_T, noise=z[:K - 2], plan=plan), y0)


# 5 ------------------------------------------------------------------------------------------------
def test_chunked_plan_is_the_per_chunk_calls_bit_for_bit():
    from diffsg_amd import steps
    name, B, chunk, K = "nu3", 96, 32, 7
    d = make_ddpm(name)
    g = R.nu_golden()
    cond = torch.from_numpy(g["cond"])[:B].cuda()
    seeds = [11, 2 ** 40 + 5, 77]
    for plan in (steps.strided(d, K), steps.ddim(d, K, 0.5)):
        got = d.sample_chunked(cond, 2.0, chunk, seeds=seeds, plan=plan)
        ref = torch.cat([d.sample(cond[i * chunk:(i + 1) * chunk], 2.0, seed=seeds[i], plan=plan) for i in range(B // chunk)])
        assert torch.isfinite(got).all() and torch.equal(got, ref)
    assert not torch.equal(got, d.sample_chunked(cond, 2.0, chunk, seeds=seeds))        # and the plan-less call is another call


# 6 ------------------------------------------------------------------------------------------------
def test_sample_best_with_a_plan_is_best_of_over_its_rounds():
    from diffsg_amd import best_of
    name = "nu3"
    d = make_ddpm(name)
    plan = device_plan(d, name, "strided")
    cond = R.inputs(name)[0].cuda()
    X = cond.clone() * 400.0
    seeds = [5, 6, 7]
    problem, p = d._best_of_problem()
    rounds = [d.sample(cond, 2.0, seed=s, plan=plan) for s in seeds]
    ref = best_of(problem, torch.stack(rounds), X, return_objectives=True, **p)
    got = d.sample_best(cond, X, 3, 2.0, seeds=seeds, return_objectives=True, plan=plan)
    for fname, a, b in zip(("solution", "objective", "round", "objectives"), got, ref):
        assert torch.equal(a, b), fname
    assert len(set(got.round.tolist())) > 1            # the rounds differ: more than one of them wins somewhere


# 7 ------------------------------------------------------------------------------------------------
def test_set_and_unset():
    name = "nu3"
    d = make_ddpm(name)
    plan = device_plan(d, name, "strided")
    cond = R.inputs(name)[0].cuda()
    a = d.sample(cond, 2.0, seed=21)
    p1 = d.sample(cond, 2.0, seed=21, plan=plan)
    assert getattr(d.model._native, "step_grid")[1] is plan
    b = d.sample(cond, 2.0, seed=21)
    assert getattr(d.model._native, "step_grid") is None
    p2 = d.sample(cond, 2.0, seed=21, plan=plan)
    p3 = d.sample(cond, 2.0, seed=21, plan=plan)
    assert torch.equal(a, b) and torch.equal(p1, p2) and torch.equal(p2, p3)
    assert not torch.equal(a, p1) and torch.isfinite(p1).all()


# 8 ------------------------------------------------------------------------------------------------
def test_c_abi_refuses_a_step_count_that_is_not_the_grids():
    from diffsg_amd import _lib, steps
    name, n = "tiny", 5
    d = make_ddpm(name)
    cond, y_T, z, _ = R.inputs(name)
    cond, y_T, z = cond.cuda(), y_T.cuda(), z.cuda()
    B, D = y_T.shape
    plan = steps.strided(d, n)
    plain = d.sample(cond, 2.0, y_T=y_T, noise=z)
    planned = d.sample(cond, 2.0, y_T=y_T, noise=z[:n - 2], plan=plan)      # the handle now holds the 5-step grid
    L, hd = _lib.lib(), d.model.native_handle()
    coef6 = d._coef_table()[:6].contiguous()
    out = torch.full((B, D), 123.0, device="cuda")
    torch.cuda.synchronize()

    def c_sample(coef, T, noise):
        return L.dsg_sample(hd, _lib.ptr(cond), _lib.ptr(y_T), _lib.ptr(noise), 0, 2.0, _lib.ptr(coef), T, _lib.ptr(out), B, 0, _lib.stream_ptr())

    assert c_sample(coef6, 6, z[:4].contiguous()) != 0
    msg = L.dsg_last_error().decode()
    assert "5" in msg.replace("6", "") and "6" in msg.replace("5", "") and "grid" in msg, msg
    torch.cuda.synchronize()
    assert bool((out == 123.0).all())                                       # nothing was enqueued
    # the right count goes through, on the grid the handle holds
    cdev = plan.coef.cuda().contiguous()
    assert c_sample(cdev, n, z[:n - 2].contiguous()) == 0, L.dsg_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(out, planned)
    # a refused setting leaves the grid as it was
    t = (ctypes.c_float * n)(*plan.t.tolist())
    assert L.dsg_set_step_grid(hd, t, n, n + 1) != 0 and "renorm_steps" in L.dsg_last_error().decode()
    assert L.dsg_set_step_grid(hd, t, -1, -1) != 0
    assert L.dsg_set_step_grid(hd, t, n, -2) != 0
    assert torch.equal(d.sample(cond, 2.0, y_T=y_T, noise=z[:n - 2], plan=plan), planned)
    assert torch.equal(d.sample(cond, 2.0, y_T=y_T, noise=z), plain)


# 9 ------------------------------------------------------------------------------------------------
def test_plan_on_a_non_default_stream():
    name = "nu3"
    _, K = R.NETS[name]
    d = make_ddpm(name)
    plan = device_plan(d, name, "ddim0.5")
    cond, y_T, z, _ = R.inputs(name)
    cond, y_T, z_all = cond.cuda(), y_T.cuda(), z.cuda()
    z = z_all[:K - 2].contiguous()
    ref = d.sample(cond, 2.0, y_T=y_T, noise=z, plan=plan)
    d.sample(cond, 2.0, y_T=y_T, noise=z_all)              # drop the grid: the next call sets it again, from inside the stream context
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = d.sample(cond, 2.0, y_T=y_T, noise=z, plan=plan)
        again = d.sample(cond, 2.0, y_T=y_T, noise=z, plan=plan)
    side.synchronize()
    assert torch.equal(got, ref) and torch.equal(again, ref)


# 10 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,sampler", [("K10_strided", "strided"), ("K10_ddim0", "ddim0")])
def test_nu_checkpoint_ratio_of_a_ten_step_plan(key, sampler):
    """The shipped NU checkpoint, 512 rows, omega = 500, K = 10, scored by the product's decoder and evaluator on the device: within
    2e-3 of the CPU value in tests/golden/g17_steps.json -- the margin tests/test_gpu_parity.py gives the same quantity on the trained
    schedule, because float32 itself is good to 2.6e-3 against float64 at this omega."""
    from diffsg_amd import decode
    with open(os.path.join(GOLD, "g17_steps.json")) as f:
        want = json.load(f)["ratios"][key]
    g = R.nu_golden()
    d = make_ddpm("nu3")
    plan = device_plan(d, "nu3", sampler)
    cond = torch.from_numpy(g["cond"]).cuda()
    y0 = d.sample_checked(cond, 500.0, y_T=torch.from_numpy(g["y_T"]), noise=torch.from_numpy(g["z"])[:8], plan=plan)
    P = float(g["P_sum"])
    Xs = cond.clone(); Xs[:, 0::2] *= 400; Xs[:, 1::2] *= 400
    Yt = torch.from_numpy(g["y_test"]).cuda().clone(); Yt[:, 0] *= 400; Yt[:, 1] *= 400; Yt[:, 2:] *= P
    ratio = float(decode.nu_rate(decode.nu_decode(y0, 400, 400, P), Xs).sum() / decode.nu_rate(Yt, Xs).sum())
    print(f"{key}: less ratio on the device {ratio:.5f} (CPU reference {want:.5f})")
    assert abs(ratio - want) <= 2e-3, (ratio, want)
