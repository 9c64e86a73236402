"""Per-step guidance weights on the device (steps.with_guidance, dsg_set_step_guidance): a step whose weight is 0 runs
ONE denoiser pass.  Against the CPU reference tests/guidance_ref.py and against the library's own unscheduled calls.

Bound of every comparison with the reference: `rel <= TOL + 3 x budget`, TOL = 1e-5 as in tests/test_gpu_steps.py and `budget` the
reference's own float32-against-float64 error on the same case (tests/test_guidance_cpu.py caps it at CAP / 2).  Nets: `tiny` (T = 8,
K = 4), `nu3` with the shipped checkpoint (T = 20, K = 10), `msr3` (T = 12, K = 5) and `msr80` with the weights of the T = 6 sampling
golden (K = 4), whose one-pass context runs the 64- and 128-wide forms.  70 rows (three row tiles, the last ragged); 150 rows in 32-row
chunks (the scalar path of the update) and 160 (the quad path).  All tests need an MI355X: run with `-m gpu`."""
import ctypes

import numpy as np
import pytest
import torch

import guidance_ref as G
import steps_ref as R
from oracle import ddpm_oracle as O
from weights import CONFIGS

pytestmark = pytest.mark.gpu

TOL = 1e-5
MODES = ("split_f16", "f32")
POLICIES = ("default", "large")
# (sampler, mask) of the comparisons with the reference, per net (tests/test_guidance_cpu.py derives the budgets of exactly these)
PARITY = tuple((s, m) for s in ("identity", "ddim0.5") for m in G.MASKS) + (("strided", "even"), ("ddim0", "odd"))


def make_ddpm(name, policy="default"):
    """The case's net under its problem's DDPM class (NU for nu3: decoder and objective of sample_best), on the device."""
    from diffsg_amd import UNet1D
    from diffsg_amd import classifier_free_MSR as MSR, classifier_free_NU as NU
    T, _ = G.NETS[name]
    cfg = CONFIGS[name]
    _, p = G.net_params(name)
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
    T, K = G.NETS[name]
    if sampler == "identity":
        return steps.strided(d, T)
    kind, eta = R.SAMPLERS[sampler]
    return steps.strided(d, K) if kind == "strided" else steps.ddim(d, K, eta)


def guided(plan, mask):
    from diffsg_amd import steps
    return steps.with_guidance(plan, G.masks(plan.K)[mask])


def check(got, ref32, ref64, tag):
    e, budget = R.rel(got, ref32), R.rel(ref32, ref64)
    print(f"{tag}: rel err vs reference {e:.2e} (reference float32 vs float64: {budget:.2e})")
    assert np.isfinite(e) and e <= TOL + 3.0 * budget, (tag, e, budget)


def settings(d):
    """Every (precision mode, graph or eager) of a handle; the caller's launch policy is the handle's."""
    for mode in MODES:
        d.model.set_precision(mode)
        for graph in (True, False):
            yield mode, graph
    d.model.set_precision("split_f16")


# 1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", list(G.NETS))
def test_all_ones_and_no_guidance_are_the_plain_call_bit_for_bit(name, policy):
    from diffsg_amd import steps
    d = make_ddpm(name, policy)
    cond, y_T, z = G.inputs(name)
    cond = cond.cuda()
    for sampler in ("identity", "ddim0.5"):
        plan = device_plan(d, name, sampler)
        ones = guided(plan, "ones")
        none = steps.with_guidance(plan, None)
        assert ones.coef is plan.coef and none.guidance is None
        zz = z[:plan.K - 2]
        for mode, graph in settings(d):
            for omega in (2.0, 500.0):
                kw = dict(y_T=y_T, noise=zz, use_graph=graph)
                a = d.sample(cond, omega, plan=None if sampler == "identity" else plan, **kw)
                b = d.sample(cond, omega, plan=ones, **kw)
                c = d.sample(cond, omega, plan=none, **kw)
                assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(a, c), (sampler, mode, graph, omega)


# 2 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", list(G.NETS))
def test_all_zeros_is_the_omega_zero_call_bit_for_bit(name, policy):
    """1 * e1 - 0 * e0 is e1 for finite e0: the one-pass launch's eps1 is the two-pass launch's eps1 in every form these shapes take."""
    d = make_ddpm(name, policy)
    cond, y_T, z = G.inputs(name)
    cond = cond.cuda()
    for sampler in ("identity", "ddim0.5"):
        plan = device_plan(d, name, sampler)
        zeros = guided(plan, "zeros")
        zz = z[:plan.K - 2]
        for mode, graph in settings(d):
            a = d.sample(cond, 0.0, plan=plan, y_T=y_T, noise=zz, use_graph=graph)
            for omega in (500.0, -1.0):
                b = d.sample(cond, omega, plan=zeros, y_T=y_T, noise=zz, use_graph=graph)
                assert torch.isfinite(a).all() and torch.equal(a, b), (sampler, mode, graph, omega)


# 3 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", list(G.NETS))
def test_mixed_schedules_against_the_reference(name, policy):
    d = make_ddpm(name, policy)
    cond, y_T, z = G.inputs(name)
    cond = cond.cuda()
    for sampler, mask in PARITY:
        plan = guided(device_plan(d, name, sampler), mask)
        zz = z[:plan.K - 2]
        for omega in G.OMEGAS:
            ref = G.reference(name, sampler, mask, omega)
            for mode in MODES:
                d.model.set_precision(mode)
                y0 = d.sample(cond, omega, y_T=y_T, noise=zz, plan=plan)
                check(y0, ref.y32, ref.y64, f"{name} {policy} {sampler} {mask} omega={omega:g} {mode}")
                assert torch.equal(d.sample(cond, omega, y_T=y_T, noise=zz, plan=plan, use_graph=False), y0), (sampler, mask, omega, mode)
    d.model.set_precision("split_f16")


# 4 ------------------------------------------------------------------------------------------------
def one_step_plans(plan, renorm_steps):
    """The K one-step plans of a K-step plan, in call order (step index K-1 first): row j alone, renormalised iff the call renormalises it."""
    from diffsg_amd.steps import StepPlan
    K = plan.K
    out = []
    for done, j in enumerate(range(K - 1, -1, -1)):
        out.append((j, StepPlan(plan.taus[j:j + 1], plan.t[j:j + 1].clone(), plan.coef[j:j + 1].clone(), 1 if done < renorm_steps else 0)))
    return out


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", list(G.NETS))
def test_mixed_schedule_is_the_chain_of_one_step_calls_bit_for_bit(name, policy):
    """A noise-free table (DDIM eta = 0) with injected y_T: the K-step call under a schedule is the chain of K one-step calls of the
    unscheduled API, `omega * g_j` on guided steps and 0.0 on unguided ones -- first confirmed with no guidance anywhere."""
    from diffsg_amd import steps
    d = make_ddpm(name, policy)
    cond, y_T, _ = G.inputs(name)
    cond = cond.cuda()
    _, K = G.NETS[name]
    omega = 2.0
    for rn in (0, min(K, 4)):
        base = steps.with_renorm(steps.ddim(d, K, 0.0), rn)
        for mode, graph in settings(d):
            for mask in ("ones", "even", "half", "interval"):
                g = G.masks(K)[mask]
                y = y_T.cuda()
                for j, p1 in one_step_plans(base, rn):
                    w = float(np.float32(omega) * np.float32(g[j])) if g[j] != 0 else 0.0
                    y = d.sample(cond, w, y_T=y, plan=p1, use_graph=graph)
                whole = d.sample(cond, omega, y_T=y_T, plan=base if mask == "ones" else steps.with_guidance(base, g), use_graph=graph)
                assert torch.isfinite(whole).all() and torch.equal(whole, y), (rn, mode, graph, mask)


# 5 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name,B", [("nu3", 150), ("nu3", 160), ("tiny", 150), ("msr80", 96)])
def test_chunked_call_is_the_per_chunk_calls_bit_for_bit(name, B, policy):
    d = make_ddpm(name, policy)
    chunk = 32
    cond = G.inputs(name, B)[0].cuda()
    nch = -(-B // chunk)
    seeds = [11 + 2 ** 40 * k for k in range(nch)]
    for sampler, mask in (("identity", "even"), ("ddim0.5", "half"), ("strided", "interval")):
        plan = guided(device_plan(d, name, sampler), mask)
        for mode, graph in settings(d):
            got = d.sample_chunked(cond, 2.0, chunk, seeds=seeds, plan=plan, use_graph=graph)
            ref = torch.cat([d.sample(cond[i * chunk:(i + 1) * chunk], 2.0, seed=seeds[i], plan=plan, use_graph=graph) for i in range(nch)])
            assert torch.isfinite(got).all() and torch.equal(got, ref), (sampler, mask, mode, graph)


# 6 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name,B", [("nu3", 150), ("nu3", 160), ("tiny", 160)])
def test_variants_under_one_schedule_are_the_per_chunk_calls_bit_for_bit(name, B, policy):
    from diffsg_amd import steps
    d = make_ddpm(name, policy)
    chunk = 32
    cond = G.inputs(name, B)[0].cuda()
    nch = -(-B // chunk)
    seeds = [7 + 3 * k for k in range(nch)]
    _, K = G.NETS[name]
    g = G.masks(K)["half"]
    a, b = steps.with_guidance(steps.strided(d, K), g), steps.with_guidance(steps.ddim(d, K, 0.5), g)
    variants = [(2.0, a), (-1.0, b), (500.0, steps.with_renorm(a, 0)), (2.0, steps.with_renorm(b, 1)), (-1.0, steps.with_renorm(a, K))][:nch]
    for mode, graph in settings(d):
        got = d.sample_chunked(cond, 1.0, chunk, seeds=seeds, variants=variants, use_graph=graph)
        ref = torch.cat([d.sample(cond[i * chunk:(i + 1) * chunk], om, seed=seeds[i], plan=p, use_graph=graph)
                         for i, (om, p) in enumerate(variants)])
        assert torch.isfinite(got).all() and torch.equal(got, ref), (mode, graph)
    # another schedule in one of the variants is refused, naming it
    other = steps.with_guidance(a, G.masks(K)["even"])
    with pytest.raises(ValueError, match="variant 1"):
        d.sample_chunked(cond, 1.0, chunk, seeds=seeds, variants=[variants[0], (2.0, other)] + variants[2:])


# 7 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
def test_sample_best_is_the_same_across_groupings(policy):
    name = "nu3"
    d = make_ddpm(name, policy)
    plan = guided(device_plan(d, name, "strided"), "even")
    cond = G.inputs(name, 160)[0][:64].cuda()
    X = cond.clone() * 400.0
    seeds = [5, 6, 7]
    for mode, graph in settings(d):
        kw = dict(seeds=seeds, return_objectives=True, plan=plan, use_graph=graph)
        grouped = d.sample_best(cond, X, 3, 2.0, chunk_rows=64, **kw)                      # one chunked call
        per_round = d.sample_best(cond, X, 3, 2.0, chunk_rows=64, max_rows=64, **kw)
        single = d.sample_best(cond, X, 3, 2.0, **kw)                                      # sample() per round
        for fname, a, b, c in zip(("solution", "objective", "round", "objectives"), grouped, per_round, single):
            assert torch.equal(a, b) and torch.equal(a, c), (fname, mode, graph)
        assert len(set(grouped.round.tolist())) > 1


# 8 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
def test_recorded_trajectory_carries_eps1_on_an_unguided_step(policy):
    from diffsg_amd.ddpm import DDPMCore
    name, sampler, mask, omega = "nu3", "ddim0.5", "even", 2.0
    _, K = G.NETS[name]
    d = make_ddpm(name, policy)
    d._decode_recorded = lambda i, y: DDPMCore._decode_recorded(d, i, y)      # the raw states: what the library records
    cond, y_T, z = G.inputs(name)
    cond, zz = cond.cuda(), z[:K - 2]
    D = CONFIGS[name]["input_dim"]
    base = device_plan(d, name, sampler)
    plan = guided(base, mask)
    ref = G.reference(name, sampler, mask, omega)
    (y32, e32), (y64, e64) = R.trace_arrays(ref.trace32), R.trace_arrays(ref.trace64)
    for mode, graph in settings(d):
        tag = f"{policy} {mode} {'graph' if graph else 'eager'}"
        d.record_denoise_path = True
        y0 = d.sample(cond, omega, y_T=y_T, noise=zz, plan=plan, use_graph=graph)
        assert d.y_i_record.shape == (G.B, K * D) and d.eps_i_record.shape == (G.B, K * D)
        check(d.y_i_record, y32, y64, "recorded y " + tag)
        check(d.eps_i_record, e32, e64, "recorded eps " + tag)
        assert np.array_equal(d.y_i_record[:, -D:], y0.cpu().numpy())
        # and bit for bit: with every weight 0 the recorded eps is the omega = 0 call's, which is eps1 of a two-pass step
        d.sample(cond, 500.0, y_T=y_T, noise=zz, plan=guided(base, "zeros"), use_graph=graph)
        e_zero, y_zero = d.eps_i_record.copy(), d.y_i_record.copy()
        d.sample(cond, 0.0, y_T=y_T, noise=zz, plan=base, use_graph=graph)
        assert np.array_equal(e_zero, d.eps_i_record) and np.array_equal(y_zero, d.y_i_record), tag
        d.record_denoise_path = False
        assert torch.equal(d.sample(cond, omega, y_T=y_T, noise=zz, plan=plan, use_graph=graph), y0), tag


# 9 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", ["nu3", "msr80"])
def test_plain_then_guidance_then_plain_on_one_handle(name, policy):
    d = make_ddpm(name, policy)
    cond = G.inputs(name)[0].cuda()
    base = device_plan(d, name, "strided")
    plan = guided(base, "odd")
    nat = d.model._native
    for mode, graph in settings(d):
        a = d.sample(cond, 2.0, seed=21, use_graph=graph)
        pa = d.sample(cond, 2.0, seed=21, plan=base, use_graph=graph)
        assert nat.step_guidance is None
        g1 = d.sample(cond, 2.0, seed=21, plan=plan, use_graph=graph)
        held = nat.step_guidance
        assert held is not None and held[1] == tuple(plan.guidance.tolist())
        g2 = d.sample(cond, 2.0, seed=21, plan=plan, use_graph=graph)
        assert nat.step_guidance is held                       # a repeated call sets nothing
        pb = d.sample(cond, 2.0, seed=21, plan=base, use_graph=graph)
        assert nat.step_guidance is None                       # a plan without guidance removes it
        b = d.sample(cond, 2.0, seed=21, use_graph=graph)
        g3 = d.sample(cond, 2.0, seed=21, plan=plan, use_graph=graph)
        assert torch.equal(a, b) and torch.equal(pa, pb) and torch.equal(g1, g2) and torch.equal(g1, g3), (mode, graph)
        assert not torch.equal(pa, g1) and torch.isfinite(g1).all()


# 10 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
def test_c_abi_set_unset_mismatch_and_refusals(policy):
    from diffsg_amd import _lib, steps
    name = "tiny"
    T, _ = G.NETS[name]
    d = make_ddpm(name, policy)
    cond, y_T, z = G.inputs(name)
    cond, y_T, z = cond.cuda(), y_T.cuda(), z.cuda()
    B, D = y_T.shape
    g = G.masks(T)["even"]
    L = _lib.lib()
    coef = d._coef_table()
    arr = (ctypes.c_float * T)(*g)
    for mode, graph in settings(d):
        flags = 0 if graph else 1
        plain = d.sample(cond, 2.0, y_T=y_T, noise=z, use_graph=graph)
        want = d.sample(cond, 2.0, y_T=y_T, noise=z, plan=steps.with_guidance(d, g), use_graph=graph)
        d.sample(cond, 2.0, y_T=y_T, noise=z, use_graph=graph)                  # the handle holds no schedule and no grid again
        hd = d.model.native_handle()
        out = torch.full((B, D), 123.0, device="cuda")
        torch.cuda.synchronize()

        def c_sample(T_, noise, fn="dsg_sample"):
            cf = coef[:T_].contiguous()
            if fn == "dsg_sample":
                return L.dsg_sample(hd, _lib.ptr(cond), _lib.ptr(y_T), _lib.ptr(noise), 0, 2.0, _lib.ptr(cf), T_, _lib.ptr(out), B, flags, _lib.stream_ptr())
            if fn == "dsg_sample_rec":
                return L.dsg_sample_rec(hd, _lib.ptr(cond), _lib.ptr(y_T), _lib.ptr(noise), 0, 2.0, _lib.ptr(cf), T_, _lib.ptr(out), B, flags, _lib.ptr(None),
                                        _lib.ptr(None), _lib.stream_ptr())
            sd = (ctypes.c_ulonglong * 3)(1, 2, 3)
            return L.dsg_sample_chunked(hd, _lib.ptr(cond), _lib.ptr(y_T), _lib.ptr(noise), sd, 32, 2.0, _lib.ptr(cf), T_, _lib.ptr(out), B, flags,
                                        _lib.stream_ptr())

        assert L.dsg_set_step_guidance(hd, arr, T) == 0, L.dsg_last_error().decode()
        assert c_sample(T, z) == 0, L.dsg_last_error().decode()
        torch.cuda.synchronize()
        assert torch.equal(out, want), (mode, graph)
        # another step count: refused by all three entry points before anything is enqueued, naming both numbers
        out.fill_(123.0)
        torch.cuda.synchronize()
        for fn in ("dsg_sample", "dsg_sample_rec", "dsg_sample_chunked"):
            assert c_sample(T - 2, z[:T - 4].contiguous(), fn) != 0
            msg = L.dsg_last_error().decode()
            assert str(T) in msg and str(T - 2) in msg and "dsg_set_step_guidance" in msg, msg
        torch.cuda.synchronize()
        assert bool((out == 123.0).all())
        # refused settings, under the setter's own name, leave the schedule as it was
        for bad in ([1.0, -0.5] + [1.0] * (T - 2), [float("nan")] + [1.0] * (T - 1), [float("inf")] + [0.0] * (T - 1)):
            assert L.dsg_set_step_guidance(hd, (ctypes.c_float * T)(*bad), T) != 0
            assert "dsg_set_step_guidance" in L.dsg_last_error().decode()
        assert L.dsg_set_step_guidance(hd, arr, -1) != 0 and "dsg_set_step_guidance" in L.dsg_last_error().decode()
        assert c_sample(T, z) == 0
        torch.cuda.synchronize()
        assert torch.equal(out, want), (mode, graph)
        # unset, both spellings: the plain call again
        for unset in (lambda: L.dsg_set_step_guidance(hd, None, 0), lambda: L.dsg_set_step_guidance(hd, arr, 0)):
            assert L.dsg_set_step_guidance(hd, arr, T) == 0
            assert unset() == 0
            assert c_sample(T, z) == 0
            torch.cuda.synchronize()
            assert torch.equal(out, plain), (mode, graph)


# 11 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
def test_guidance_on_a_non_default_stream(policy):
    name = "nu3"
    _, K = G.NETS[name]
    d = make_ddpm(name, policy)
    plan = guided(device_plan(d, name, "ddim0.5"), "even")
    cond, y_T, z = G.inputs(name)
    cond, y_T, z_all = cond.cuda(), y_T.cuda(), z.cuda()
    z = z_all[:K - 2].contiguous()
    side = torch.cuda.Stream()
    for mode, graph in settings(d):
        ref = d.sample(cond, 2.0, y_T=y_T, noise=z, plan=plan, use_graph=graph)
        d.sample(cond, 2.0, y_T=y_T, noise=z_all, use_graph=graph)     # drop grid and schedule: the next call sets them again, from inside the stream context
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            got = d.sample(cond, 2.0, y_T=y_T, noise=z, plan=plan, use_graph=graph)
            again = d.sample(cond, 2.0, y_T=y_T, noise=z, plan=plan, use_graph=graph)
        side.synchronize()
        assert torch.equal(got, ref) and torch.equal(again, ref), (mode, graph)


# 12 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", ["nu3", "msr80"])
def test_renorm_hook_under_a_schedule(name, policy):
    """A renorm hook (parallel.global_renorm; one shard: the reduction is the identity) with unguided steps among the early ones: the hook is
    called on exactly the plan's renorm steps, which run eagerly in the context the step asks for, and the result is the hook-less call's
    within TOL: both evaluate the same float32 arithmetic, the hook path reduces the float64 moments in another order."""
    from diffsg_amd import parallel as par
    d = make_ddpm(name, policy)
    cond, y_T, z = G.inputs(name)
    cond = cond.cuda()
    for sampler, mask in (("identity", "even"), ("ddim0.5", "odd"), ("strided", "zeros")):
        plan = guided(device_plan(d, name, sampler), mask)
        zz = z[:plan.K - 2]
        for mode, graph in settings(d):
            want = d.sample(cond, 2.0, y_T=y_T, noise=zz, plan=plan, use_graph=graph)
            calls = []
            with par.global_renorm(d, reduce=lambda stats: calls.append(1)):
                hooked = d.sample(cond, 2.0, y_T=y_T, noise=zz, plan=plan, use_graph=graph)
            assert len(calls) == plan.renorm_steps, (sampler, mask, mode, graph, calls)
            assert torch.isfinite(hooked).all() and R.rel(hooked, want) <= TOL, (sampler, mask, mode, graph)
            assert torch.equal(d.sample(cond, 2.0, y_T=y_T, noise=zz, plan=plan, use_graph=graph), want)
