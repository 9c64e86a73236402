"""The x0 clip on the device (steps.with_clip, dsg_set_xstart_clip, dsg_clip.hpp).  Against the CPU reference tests/clip_ref.py
and against the library's own calls without a clip.

Bound of every comparison with the reference: `rel <= TOL + 3 x budget`, TOL = 1e-5 and `budget` the reference's own float32-against-float64
error on the same case (tests/test_clip_cpu.py caps it).  Nets: `tiny` (T = 8, K = 4, D = 3), `nu3` with the shipped checkpoint (T = 20,
K = 10, D = 5) and `msr3` (T = 12, K = 5, D = 3).  70 rows (B*D = 210 / 350: the scalar tail of the update) and 72 rows (216 / 360: whole
16-byte quads, which straddle rows at D = 3 and 5).  All tests need an MI355X: run with `-m gpu`."""
import ctypes

import numpy as np
import pytest
import torch

import clip_ref as C
import guidance_ref as G
import multistep_ref as M
import steps_ref as R
from oracle import ddpm_oracle as O
from test_gpu_guidance import device_plan, settings
from weights import CONFIGS

pytestmark = pytest.mark.gpu

TOL = 1e-5
MODES = ("split_f16", "f32")
POLICIES = ("default", "large")
INF = float("inf")


def make_ddpm(name, policy="default"):
    """The case's net (clip_ref's weight seed) under its problem's DDPM class, on the device."""
    from diffsg_amd import UNet1D
    from diffsg_amd import classifier_free_MSR as MSR, classifier_free_NU as NU
    T, _ = C.NETS[name]
    cfg = CONFIGS[name]
    _, p = C.net_params(name)
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


def plan_of(d, name, sampler):
    from diffsg_amd import steps
    _, K = C.NETS[name]
    if sampler == "dpmpp2m":
        return steps.dpmpp_2m(d, K, renorm_steps=M.renorm_of(name, "second"))
    return device_plan(d, name, sampler)


def check(got, ref32, ref64, tag):
    e, budget = R.rel(got, ref32), R.rel(ref32, ref64)
    print(f"{tag}: rel err vs reference {e:.2e} (reference float32 vs float64: {budget:.2e})")
    assert np.isfinite(e) and e <= TOL + 3.0 * budget, (tag, e, budget)


def binding(name, rows=70, sampler="ddim0", omega=2.0):
    return C.bounds(name, sampler, omega, rows)


# 1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", C.ROWS)
@pytest.mark.parametrize("name", list(C.NETS))
def test_parity_with_the_reference(name, rows):
    from diffsg_amd import steps
    d = make_ddpm(name)
    D = CONFIGS[name]["input_dim"]
    _, K = C.NETS[name]
    cond, y_T, z = C.inputs(name, rows)
    cond, zz = cond.cuda(), z[:K - 2]
    assert (rows * D) % 4 == (2 if rows == 70 else 0) and D % 4 != 0      # the scalar tail / whole quads that straddle rows
    for sampler in C.SAMPLERS:
        base = plan_of(d, name, sampler)
        assert sampler != "dpmpp2m" or bool((base.history[:, 0] != 0).any())
        for omega in C.OMEGAS:
            ref = C.reference(name, sampler, omega, rows)
            plan = steps.with_clip(base, *C.bounds(name, sampler, omega, rows))
            for mode in MODES:
                d.model.set_precision(mode)
                y0 = d.sample(cond, omega, y_T=y_T, noise=zz, plan=plan)
                check(y0, ref.y32, ref.y64, f"{name} {rows} rows {sampler} omega={omega:g} {mode}")
                assert torch.equal(d.sample(cond, omega, y_T=y_T, noise=zz, plan=plan, use_graph=False), y0), (sampler, omega, mode)
    d.model.set_precision("split_f16")


# 2 ------------------------------------------------------------------------------------------------
def loose(D):
    """Bounds that clip nothing: infinite ones, and finite ones wider than every prediction (and a mixture per feature)."""
    return ((-INF, INF), ([-1e30] * D, [1e30] * D), ([-INF] + [-1e30] * (D - 1), [1e30] * (D - 1) + [INF]))


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", list(C.NETS))
def test_bounds_that_clip_nothing_give_the_bits_of_the_call_without_a_clip(name, policy):
    from diffsg_amd import steps
    d = make_ddpm(name, policy)
    D = CONFIGS[name]["input_dim"]
    _, K = C.NETS[name]
    mask = M.guide_mask(K)
    assert 0.0 in mask and any(w != 0.0 for w in mask)
    strided = plan_of(d, name, "strided")
    forms = {"plain": strided, "noisy ddim": plan_of(d, name, "ddim0.5"), "scheduled": steps.with_guidance(strided, mask),
             "history": plan_of(d, name, "dpmpp2m"), "history scheduled": steps.with_guidance(plan_of(d, name, "dpmpp2m"), mask),
             "identity": None}
    chunk, Bc = 32, 150                                                      # the last chunk is short
    cond_c = G.inputs(name, Bc)[0].cuda()
    nch = -(-Bc // chunk)
    seeds = [11 + 2 ** 40 * k for k in range(nch)]
    var_plans = [steps.with_renorm(strided, k % 3) if k % 2 else plan_of(d, name, "ddim0") for k in range(nch)]
    for rows in C.ROWS:
        cond, y_T, z = C.inputs(name, rows)
        cond = cond.cuda()
        for mode, graph in settings(d):
            for tag, base in forms.items():
                kw = dict(y_T=y_T, noise=z if base is None else z[:K - 2], use_graph=graph)
                want = d.sample(cond, 2.0, plan=base, **kw)
                assert torch.isfinite(want).all()
                for lo, hi in loose(D):
                    got = d.sample(cond, 2.0, plan=steps.with_clip(d if base is None else base, lo, hi), **kw)
                    assert torch.equal(got, want), (tag, rows, mode, graph, lo)
    for mode, graph in settings(d):
        for tag, base in (("plain", strided), ("scheduled", forms["scheduled"]), ("history", forms["history"])):
            want = d.sample_chunked(cond_c, 2.0, chunk, seeds=seeds, plan=base, use_graph=graph)
            for lo, hi in loose(D):
                got = d.sample_chunked(cond_c, 2.0, chunk, seeds=seeds, plan=steps.with_clip(base, lo, hi), use_graph=graph)
                assert torch.equal(got, want), ("chunked " + tag, mode, graph, lo)
        for sched in (False, True):
            vp = [steps.with_guidance(p, mask) for p in var_plans] if sched else var_plans
            want = d.sample_chunked(cond_c, 2.0, chunk, seeds=seeds, variants=[(1.0 + k, p) for k, p in enumerate(vp)], use_graph=graph)
            for lo, hi in loose(D):
                clip = steps.with_clip(vp[0], lo, hi).clip
                cl = [steps.StepPlan(p.taus, p.t, p.coef, p.renorm_steps, p.guidance, None, clip) for p in vp]
                got = d.sample_chunked(cond_c, 2.0, chunk, seeds=seeds, variants=[(1.0 + k, p) for k, p in enumerate(cl)], use_graph=graph)
                assert torch.equal(got, want), ("variants", sched, mode, graph, lo)


# 3 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", C.ROWS)
@pytest.mark.parametrize("name", list(C.NETS))
def test_binding_bounds_change_the_result_and_hold_y0_under_ddim(name, rows):
    """DDIM eta = 0, no renorm: the last step (acp_p = 1) returns the clamped prediction itself, so every element of y_0 lies inside
    its feature's bounds to rounding."""
    from diffsg_amd import steps
    d = make_ddpm(name)
    _, K = C.NETS[name]
    cond, y_T, _ = C.inputs(name, rows)
    cond = cond.cuda()
    lo, hi = binding(name, rows)
    assert len(set(lo.tolist())) == lo.numel() and len(set(hi.tolist())) == hi.numel()          # per-feature bounds that all differ
    base = steps.with_renorm(steps.ddim(d, K, 0.0), 0)
    plan = steps.with_clip(base, lo, hi)
    for mode, graph in settings(d):
        plain = d.sample(cond, 2.0, y_T=y_T, plan=base, use_graph=graph)
        y0 = d.sample(cond, 2.0, y_T=y_T, plan=plan, use_graph=graph)
        assert torch.isfinite(y0).all() and not torch.equal(y0, plain)
        lo_d, hi_d = lo.cuda(), hi.cuda()
        under = (lo_d - y0) / torch.clamp(lo_d.abs(), min=1.0)
        over = (y0 - hi_d) / torch.clamp(hi_d.abs(), min=1.0)
        worst = float(torch.maximum(under, over).max())
        print(f"{name} {rows} rows {mode} {'graph' if graph else 'eager'}: y_0 outside its bounds by at most {worst:.2e} (relative to max(1, |bound|))")
        assert worst <= 1e-5, (mode, graph, worst)
        assert bool(((y0 < lo_d) | (y0 > hi_d)).logical_not().any()) and bool((plain < lo_d).any() or (plain > hi_d).any())


# 4 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name,B", [("nu3", 150), ("tiny", 150), ("nu3", 160)])
def test_chunked_call_is_the_per_chunk_calls_bit_for_bit(name, B, policy):
    from diffsg_amd import steps
    d = make_ddpm(name, policy)
    chunk = 32
    cond = G.inputs(name, B)[0].cuda()
    nch = -(-B // chunk)
    seeds = [11 + 2 ** 40 * k for k in range(nch)]
    lo, hi = binding(name)
    for sampler in ("strided", "dpmpp2m"):
        base = plan_of(d, name, sampler)
        plan = steps.with_clip(base, lo, hi)
        for mode, graph in settings(d):
            got = d.sample_chunked(cond, 2.0, chunk, seeds=seeds, plan=plan, use_graph=graph)
            ref = torch.cat([d.sample(cond[i * chunk:(i + 1) * chunk], 2.0, seed=seeds[i], plan=plan, use_graph=graph) for i in range(nch)])
            assert torch.isfinite(got).all() and torch.equal(got, ref), (sampler, mode, graph)
            assert not torch.equal(got, d.sample_chunked(cond, 2.0, chunk, seeds=seeds, plan=base, use_graph=graph))


@pytest.mark.parametrize("policy", POLICIES)
def test_variants_under_one_clip_each_equal_their_own_call(policy):
    from diffsg_amd import steps
    name, B, chunk = "nu3", 150, 32
    d = make_ddpm(name, policy)
    _, K = C.NETS[name]
    cond = G.inputs(name, B)[0].cuda()
    nch = -(-B // chunk)
    seeds = [3 + 2 ** 33 * k for k in range(nch)]
    lo, hi = binding(name)
    strided = steps.with_clip(plan_of(d, name, "strided"), lo, hi)
    mask = M.guide_mask(K)
    for sched in (False, True):
        a = steps.with_guidance(strided, mask) if sched else strided
        plans = [steps.with_renorm(a, k % 3) if k % 2 else steps.StepPlan(a.taus, a.t, steps.ddim(d, K, 0.0).coef, a.renorm_steps, a.guidance, None, a.clip)
                 for k in range(nch)]
        assert all(p.clip is strided.clip for p in plans)
        variants = [(0.5 + k, p) for k, p in enumerate(plans)]
        for mode, graph in settings(d):
            got = d.sample_chunked(cond, 2.0, chunk, seeds=seeds, variants=variants, use_graph=graph)
            ref = torch.cat([d.sample(cond[i * chunk:(i + 1) * chunk], variants[i][0], seed=seeds[i], plan=variants[i][1], use_graph=graph)
                             for i in range(nch)])
            assert torch.isfinite(got).all() and torch.equal(got, ref), (sched, mode, graph)


def test_sample_best_is_the_same_across_groupings():
    from diffsg_amd import steps
    name = "nu3"
    d = make_ddpm(name)
    plan = steps.with_clip(plan_of(d, name, "ddim0"), *binding(name))
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
        assert torch.isfinite(grouped.solution).all()


# 5 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", C.ROWS)
def test_recorded_eps_is_the_clipped_one(rows):
    from diffsg_amd import steps
    from diffsg_amd.ddpm import DDPMCore
    name, omega = "nu3", 2.0
    _, K = C.NETS[name]
    d = make_ddpm(name)
    d._decode_recorded = lambda i, y: DDPMCore._decode_recorded(d, i, y)      # the raw states: what the library records
    cond, y_T, z = C.inputs(name, rows)
    cond = cond.cuda()
    D = CONFIGS[name]["input_dim"]
    for sampler in ("ddim0.5", "dpmpp2m"):
        plan = steps.with_clip(plan_of(d, name, sampler), *C.bounds(name, sampler, omega, rows))
        ref = C.reference(name, sampler, omega, rows)
        (y32, e32), (y64, e64) = R.trace_arrays(ref.trace32), R.trace_arrays(ref.trace64)
        for mode, graph in settings(d):
            tag = f"{sampler} {rows} rows {mode} {'graph' if graph else 'eager'}"
            d.record_denoise_path = True
            y0 = d.sample(cond, omega, y_T=y_T, noise=z[:K - 2], plan=plan, use_graph=graph)
            assert d.y_i_record.shape == (rows, K * D) and d.eps_i_record.shape == (rows, K * D)
            check(d.y_i_record, y32, y64, "recorded y " + tag)
            check(d.eps_i_record, e32, e64, "recorded eps " + tag)
            assert np.array_equal(d.y_i_record[:, -D:], y0.cpu().numpy())
            d.record_denoise_path = False
            assert torch.equal(d.sample(cond, omega, y_T=y_T, noise=z[:K - 2], plan=plan, use_graph=graph), y0), tag


# 6 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nu3", "tiny"])
def test_no_leak_between_calls(name):
    """Call A under a clip, then call B with other inputs, fewer rows and other bounds on the same handle: B is B on a fresh DDPM."""
    from diffsg_amd import steps
    d, fresh = make_ddpm(name), make_ddpm(name)
    cond, y_T, _ = C.inputs(name, 70)
    lo, hi = binding(name)
    lo_b, hi_b = lo - 0.125, hi + 0.0625
    nb = 41
    cond_b, y_b = G.inputs(name, 150)[0][100:100 + nb].cuda(), G.inputs(name, 150)[1][100:100 + nb]
    for sampler in ("ddim0", "dpmpp2m"):
        for mode, graph in settings(d):
            fresh.model.set_precision(mode)
            a = d.sample(cond.cuda(), 2.0, y_T=y_T, plan=steps.with_clip(plan_of(d, name, sampler), lo, hi), use_graph=graph)
            b = d.sample(cond_b, -1.0, y_T=y_b, plan=steps.with_clip(plan_of(d, name, sampler), lo_b, hi_b), use_graph=graph)
            want = fresh.sample(cond_b, -1.0, y_T=y_b, plan=steps.with_clip(plan_of(fresh, name, sampler), lo_b, hi_b), use_graph=graph)
            assert torch.isfinite(a).all() and torch.isfinite(b).all() and torch.equal(b, want), (sampler, mode, graph)
    fresh.model.set_precision("split_f16")


@pytest.mark.parametrize("policy", POLICIES)
def test_plain_then_clip_then_plain_on_one_handle(policy):
    from diffsg_amd import steps
    name = "nu3"
    d = make_ddpm(name, policy)
    cond = C.inputs(name, 70)[0].cuda()
    base = plan_of(d, name, "strided")
    lo, hi = binding(name)
    plan, other = steps.with_clip(base, lo, hi), steps.with_clip(base, lo - 0.25, hi + 0.25)
    ident = steps.with_clip(d, lo, hi)                       # all T trained steps under the clip
    nat = d.model._native
    for mode, graph in settings(d):
        kw = dict(seed=21, use_graph=graph)
        a = d.sample(cond, 2.0, **kw)
        pa = d.sample(cond, 2.0, plan=base, **kw)
        assert nat.x0_clip is None
        c1 = d.sample(cond, 2.0, plan=plan, **kw)
        held = nat.x0_clip
        assert held is not None and held[1][0] == tuple(lo.tolist()) and held[1][1] == tuple(hi.tolist())
        c2 = d.sample(cond, 2.0, plan=plan, **kw)
        assert nat.x0_clip is held                             # a repeated call sets nothing
        o1 = d.sample(cond, 2.0, plan=other, **kw)             # changed
        assert nat.x0_clip is not held
        i1 = d.sample(cond, 2.0, plan=ident, **kw)             # other steps, same bounds: the rows follow the plan
        pb = d.sample(cond, 2.0, plan=base, **kw)
        assert nat.x0_clip is None                             # a plan without a clip removes it
        b = d.sample(cond, 2.0, **kw)
        c3 = d.sample(cond, 2.0, plan=plan, **kw)
        o2 = d.sample(cond, 2.0, plan=other, **kw)
        i2 = d.sample(cond, 2.0, plan=ident, **kw)
        assert torch.equal(a, b) and torch.equal(pa, pb) and torch.equal(c1, c2) and torch.equal(c1, c3) and torch.equal(o1, o2) and torch.equal(i1, i2)
        assert not torch.equal(pa, c1) and not torch.equal(c1, o1) and not torch.equal(a, i1) and torch.isfinite(c1).all() and torch.isfinite(i1).all()


# 7 ------------------------------------------------------------------------------------------------
def test_c_abi_set_unset_mismatch_and_refusals():
    from diffsg_amd import _lib, steps
    from test_clip_cpu import bad_clips, bad_rows
    name = "tiny"
    _, K = C.NETS[name]
    d = make_ddpm(name)
    cond, y_T, _ = C.inputs(name, 70)
    cond, y_T = cond.cuda(), y_T.cuda()
    B, D = y_T.shape
    base = plan_of(d, name, "ddim0")
    lo, hi = binding(name)
    plan = steps.with_clip(base, lo, hi)
    rows = steps.x0_rows(d, base.taus).reshape(-1).tolist()
    L = _lib.lib()
    fl = lambda v: (ctypes.c_float * len(v))(*v)
    lo_c, hi_c, rows_c = fl(lo.tolist()), fl(hi.tolist()), fl(rows)
    for mode, graph in settings(d):
        flags = 0 if graph else 1
        want = d.sample(cond, 2.0, y_T=y_T, plan=plan, use_graph=graph)
        plain = d.sample(cond, 2.0, y_T=y_T, plan=base, use_graph=graph)          # the handle holds the grid and no clip
        assert not torch.equal(want, plain)
        hd = d.model.native_handle()
        coef = base.coef.cuda().contiguous()
        out = torch.full((B, D), 123.0, device="cuda")
        torch.cuda.synchronize()
        gen = L.dsg_generation(hd) if hasattr(L, "dsg_generation") else None

        def c_sample(T_, fn="dsg_sample"):
            cf = coef[:T_].contiguous()
            if fn == "dsg_sample":
                return L.dsg_sample(hd, _lib.ptr(cond), _lib.ptr(y_T), _lib.ptr(None), 0, 2.0, _lib.ptr(cf), T_, _lib.ptr(out), B, flags, _lib.stream_ptr())
            if fn == "dsg_sample_rec":
                return L.dsg_sample_rec(hd, _lib.ptr(cond), _lib.ptr(y_T), _lib.ptr(None), 0, 2.0, _lib.ptr(cf), T_, _lib.ptr(out), B, flags, _lib.ptr(None),
                                        _lib.ptr(None), _lib.stream_ptr())
            sd = (ctypes.c_ulonglong * 3)(1, 2, 3)
            return L.dsg_sample_chunked(hd, _lib.ptr(cond), _lib.ptr(y_T), _lib.ptr(None), sd, 32, 2.0, _lib.ptr(cf), T_, _lib.ptr(out), B, flags,
                                        _lib.stream_ptr())

        assert L.dsg_set_xstart_clip(hd, lo_c, hi_c, D, rows_c, K) == 0, L.dsg_last_error().decode()
        assert c_sample(K) == 0, L.dsg_last_error().decode()
        torch.cuda.synchronize()
        assert torch.equal(out, want), (mode, graph)
        # another row count than the call's T: refused by all three entry points before anything is enqueued, naming both numbers
        assert L.dsg_set_xstart_clip(hd, lo_c, hi_c, D, fl(rows + rows[:8]), K + 2) == 0
        out.fill_(123.0)
        torch.cuda.synchronize()
        for fn in ("dsg_sample", "dsg_sample_rec", "dsg_sample_chunked"):
            assert c_sample(K, fn) != 0
            msg = L.dsg_last_error().decode()
            assert str(K) in msg and str(K + 2) in msg and "dsg_set_xstart_clip" in msg, msg
        torch.cuda.synchronize()
        assert bool((out == 123.0).all())
        # refused settings, under the setter's own name, leave the clip as it was
        assert L.dsg_set_xstart_clip(hd, lo_c, hi_c, D, rows_c, K) == 0
        for (blo, bhi), _ in bad_clips(D):
            assert L.dsg_set_xstart_clip(hd, fl(blo), fl(bhi), D, rows_c, K) != 0
            assert "dsg_set_xstart_clip" in L.dsg_last_error().decode()
        for bad in bad_rows(rows):
            assert L.dsg_set_xstart_clip(hd, lo_c, hi_c, D, fl(bad), K) != 0
            assert "dsg_set_xstart_clip" in L.dsg_last_error().decode()
        assert L.dsg_set_xstart_clip(hd, lo_c, hi_c, D, rows_c, -1) != 0 and "dsg_set_xstart_clip" in L.dsg_last_error().decode()
        assert L.dsg_set_xstart_clip(hd, fl(lo.tolist() + [0.0]), fl(hi.tolist() + [1.0]), D + 1, rows_c, K) != 0
        msg = L.dsg_last_error().decode()
        assert "dsg_set_xstart_clip" in msg and str(D + 1) in msg and str(D) in msg, msg
        assert gen is None or L.dsg_generation(hd) == gen
        # the clip survived all of it
        assert c_sample(K) == 0
        torch.cuda.synchronize()
        assert torch.equal(out, want), (mode, graph)
        # infinite bounds are allowed and give the call without a clip
        inf_lo, inf_hi = fl([-INF] * D), fl([INF] * D)
        assert L.dsg_set_xstart_clip(hd, inf_lo, inf_hi, D, rows_c, K) == 0, L.dsg_last_error().decode()
        assert c_sample(K) == 0
        torch.cuda.synchronize()
        assert torch.equal(out, plain), (mode, graph)
        # unset, every spelling: the plan without a clip again
        for unset in (lambda: L.dsg_set_xstart_clip(hd, None, None, 0, None, 0), lambda: L.dsg_set_xstart_clip(hd, lo_c, hi_c, D, rows_c, 0),
                      lambda: L.dsg_set_xstart_clip(hd, None, hi_c, D, rows_c, K)):
            assert L.dsg_set_xstart_clip(hd, lo_c, hi_c, D, rows_c, K) == 0
            assert unset() == 0
            assert c_sample(K) == 0
            torch.cuda.synchronize()
            assert torch.equal(out, plain), (mode, graph)
        d.model._native.x0_clip = None


# 8 ------------------------------------------------------------------------------------------------
def test_clip_on_a_non_default_stream():
    from diffsg_amd import steps
    name = "nu3"
    d = make_ddpm(name)
    plan = steps.with_clip(plan_of(d, name, "ddim0"), *binding(name))
    cond, y_T, z = C.inputs(name, 70)
    cond, y_T, z_all = cond.cuda(), y_T.cuda(), z.cuda()
    cond_c = G.inputs(name, 150)[0].cuda()
    seeds = [7 + k for k in range(5)]
    side = torch.cuda.Stream()
    for mode, graph in settings(d):
        ref = d.sample(cond, 2.0, y_T=y_T, plan=plan, use_graph=graph)
        ref_c = d.sample_chunked(cond_c, 2.0, 32, seeds=seeds, plan=plan, use_graph=graph)
        d.sample(cond, 2.0, y_T=y_T, noise=z_all, use_graph=graph)     # drop grid and clip: the next call sets them again, from inside the stream context
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            got = d.sample(cond, 2.0, y_T=y_T, plan=plan, use_graph=graph)
            again = d.sample(cond, 2.0, y_T=y_T, plan=plan, use_graph=graph)
            got_c = d.sample_chunked(cond_c, 2.0, 32, seeds=seeds, plan=plan, use_graph=graph)
        side.synchronize()
        assert torch.equal(got, ref) and torch.equal(again, ref) and torch.equal(got_c, ref_c), (mode, graph)
