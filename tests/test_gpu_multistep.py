"""Two-step solver plans on the device (steps.dpmpp_2m, dsg_set_step_history, k_update_hist).  Against the CPU reference
tests/multistep_ref.py and against the library's own calls without a history.

Bound of every comparison with the reference: `rel <= TOL + 3 x budget`, TOL = 1e-5 and `budget` the reference's own float32-against-float64
error on the same case (tests/test_multistep_cpu.py caps it).  Nets: `tiny` (T = 8, K = 4, B*D = 210: the scalar tail of the update), `nu3`
with the shipped checkpoint (T = 20, K = 10) and `msr3` (T = 12, K = 5).  70 rows (three row tiles, the last ragged).  All tests need an
MI355X: run with `-m gpu`."""
import ctypes

import numpy as np
import pytest
import torch

import guidance_ref as G
import multistep_ref as M
import steps_ref as R
from test_gpu_guidance import make_ddpm, settings
from weights import CONFIGS

pytestmark = pytest.mark.gpu

TOL = 1e-5
MODES = ("split_f16", "f32")
POLICIES = ("default", "large")


def check(got, ref32, ref64, tag):
    e, budget = R.rel(got, ref32), R.rel(ref32, ref64)
    print(f"{tag}: rel err vs reference {e:.2e} (reference float32 vs float64: {budget:.2e})")
    assert np.isfinite(e) and e <= TOL + 3.0 * budget, (tag, e, budget)


def two_step(d, name, which="second"):
    from diffsg_amd import steps
    _, K = M.NETS[name]
    return steps.dpmpp_2m(d, K, renorm_steps=M.renorm_of(name, which))


def stripped(plan, rows):
    """`plan` with other history rows (a list of K rows, or None) and everything else shared."""
    from diffsg_amd import steps
    return steps.with_history(plan, rows)


# 1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.NETS))
def test_parity_with_the_reference(name):
    d = make_ddpm(name)
    cond, y_T, _ = M.inputs(name)
    cond = cond.cuda()
    if name == "tiny":
        assert (cond.shape[0] * CONFIGS[name]["input_dim"]) % 4 != 0           # the scalar tail of the update
    for which in ("default", "second"):
        plan = two_step(d, name, which)
        assert which == "default" or bool((plan.history[:, 0] != 0).any())
        for omega in M.OMEGAS:
            ref = M.reference(name, which, omega)
            for mode in MODES:
                d.model.set_precision(mode)
                y0 = d.sample(cond, omega, y_T=y_T, plan=plan)
                check(y0, ref.y32, ref.y64, f"{name} renorm={plan.renorm_steps} omega={omega:g} {mode}")
                assert torch.equal(d.sample(cond, omega, y_T=y_T, plan=plan, use_graph=False), y0), (which, omega, mode)
    d.model.set_precision("split_f16")


# 2 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", list(M.NETS))
def test_zero_m_is_the_plan_without_a_history_bit_for_bit(name, policy):
    """Rows with m = 0 add nothing, whether they store (p, q of the real table) or not (all-zero rows): the bits of the same plan without a
    history, noisy tables (DDIM eta = 0.5, injected noise) and noise-free ones."""
    from diffsg_amd import steps
    d = make_ddpm(name, policy)
    cond, y_T, z = M.inputs(name)
    cond = cond.cuda()
    _, K = M.NETS[name]
    real = two_step(d, name)
    storing = [[0.0, 1.0 / (j + 1.5), -0.25 * (j + 1)] for j in range(K)]
    for base in (steps.with_history(real, None), steps.ddim(d, K, 0.5)):
        zz = z[:K - 2]
        for mode, graph in settings(d):
            kw = dict(y_T=y_T, noise=zz, use_graph=graph)
            a = d.sample(cond, 2.0, plan=base, **kw)
            b = d.sample(cond, 2.0, plan=stripped(base, storing), **kw)
            c = d.sample(cond, 2.0, plan=stripped(base, [[0.0] * 3] * K), **kw)
            assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(a, c), (mode, graph)
    # and the real table is not that plan
    assert not torch.equal(d.sample(cond, 2.0, y_T=y_T, plan=real), d.sample(cond, 2.0, y_T=y_T, plan=steps.with_history(real, None)))


# 3 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nu3", "tiny"])
def test_no_leak_between_calls(name):
    """Call A, then call B with other inputs and fewer rows on the same handle: B is B on a fresh DDPM."""
    d, fresh = make_ddpm(name), make_ddpm(name)
    cond, y_T, _ = M.inputs(name)
    plan = two_step(d, name)
    nb = 41
    cond_b, y_b = G.inputs(name, 150)[0][100:100 + nb].cuda(), G.inputs(name, 150)[1][100:100 + nb]
    for mode, graph in settings(d):
        fresh.model.set_precision(mode)
        a = d.sample(cond.cuda(), 2.0, y_T=y_T, plan=plan, use_graph=graph)
        b = d.sample(cond_b, -1.0, y_T=y_b, plan=plan, use_graph=graph)
        want = fresh.sample(cond_b, -1.0, y_T=y_b, plan=two_step(fresh, name), use_graph=graph)
        assert torch.isfinite(a).all() and torch.isfinite(b).all() and torch.equal(b, want), (mode, graph)
    fresh.model.set_precision("split_f16")


# 4 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.NETS))
def test_history_under_a_guidance_schedule(name):
    from diffsg_amd import steps
    d = make_ddpm(name)
    cond, y_T, _ = M.inputs(name)
    cond = cond.cuda()
    _, K = M.NETS[name]
    base = two_step(d, name)
    mask = M.guide_mask(K)
    assert 0.0 in mask and any(w != 0.0 for w in mask)
    plan = steps.with_guidance(base, mask)
    assert plan.history is base.history
    ref = M.reference(name, "second", 2.0, True)
    ones = steps.with_guidance(base, [1.0] * K)
    for mode, graph in settings(d):
        y0 = d.sample(cond, 2.0, y_T=y_T, plan=plan, use_graph=graph)
        check(y0, ref.y32, ref.y64, f"{name} guided {mode} {'graph' if graph else 'eager'}")
        for omega in (2.0, 500.0):
            assert torch.equal(d.sample(cond, omega, y_T=y_T, plan=ones, use_graph=graph),
                               d.sample(cond, omega, y_T=y_T, plan=base, use_graph=graph)), (mode, graph, omega)


# 5 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name,B", [("nu3", 150), ("tiny", 150), ("nu3", 160)])
def test_chunked_call_is_the_per_chunk_calls_bit_for_bit(name, B, policy):
    d = make_ddpm(name, policy)
    chunk = 32
    cond = G.inputs(name, B)[0].cuda()
    nch = -(-B // chunk)
    assert B % chunk != 0 or name == "nu3"                                    # 150: the last chunk is short
    seeds = [11 + 2 ** 40 * k for k in range(nch)]
    plan = two_step(d, name)
    for mode, graph in settings(d):
        got = d.sample_chunked(cond, 2.0, chunk, seeds=seeds, plan=plan, use_graph=graph)
        ref = torch.cat([d.sample(cond[i * chunk:(i + 1) * chunk], 2.0, seed=seeds[i], plan=plan, use_graph=graph) for i in range(nch)])
        assert torch.isfinite(got).all() and torch.equal(got, ref), (mode, graph)


def test_sample_best_is_the_same_across_groupings():
    name = "nu3"
    d = make_ddpm(name)
    plan = two_step(d, name)
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
        assert torch.isfinite(grouped.solution).all() and len(set(grouped.round.tolist())) > 1


# 6 ------------------------------------------------------------------------------------------------
def test_recorded_trajectory():
    from diffsg_amd.ddpm import DDPMCore
    name, omega = "nu3", 2.0
    _, K = M.NETS[name]
    d = make_ddpm(name)
    d._decode_recorded = lambda i, y: DDPMCore._decode_recorded(d, i, y)      # the raw states: what the library records
    cond, y_T, _ = M.inputs(name)
    cond = cond.cuda()
    D = CONFIGS[name]["input_dim"]
    for which in ("default", "second"):
        plan = two_step(d, name, which)
        ref = M.reference(name, which, omega)
        (y32, e32), (y64, e64) = R.trace_arrays(ref.trace32), R.trace_arrays(ref.trace64)
        for mode, graph in settings(d):
            tag = f"{which} {mode} {'graph' if graph else 'eager'}"
            d.record_denoise_path = True
            y0 = d.sample(cond, omega, y_T=y_T, plan=plan, use_graph=graph)
            assert d.y_i_record.shape == (M.B, K * D) and d.eps_i_record.shape == (M.B, K * D)
            check(d.y_i_record, y32, y64, "recorded y " + tag)
            check(d.eps_i_record, e32, e64, "recorded eps " + tag)
            assert np.array_equal(d.y_i_record[:, -D:], y0.cpu().numpy())
            d.record_denoise_path = False
            assert torch.equal(d.sample(cond, omega, y_T=y_T, plan=plan, use_graph=graph), y0), tag


# 7 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
def test_plain_then_history_then_plain_on_one_handle(policy):
    from diffsg_amd import steps
    name = "nu3"
    d = make_ddpm(name, policy)
    cond = M.inputs(name)[0].cuda()
    plan = two_step(d, name)
    base = steps.with_history(plan, None)
    nat = d.model._native
    for mode, graph in settings(d):
        a = d.sample(cond, 2.0, seed=21, use_graph=graph)
        pa = d.sample(cond, 2.0, seed=21, plan=base, use_graph=graph)
        assert nat.step_history is None
        h1 = d.sample(cond, 2.0, seed=21, plan=plan, use_graph=graph)
        held = nat.step_history
        assert held is not None and held[1] == tuple(plan.history.reshape(-1).tolist())
        h2 = d.sample(cond, 2.0, seed=21, plan=plan, use_graph=graph)
        assert nat.step_history is held                        # a repeated call sets nothing
        pb = d.sample(cond, 2.0, seed=21, plan=base, use_graph=graph)
        assert nat.step_history is None                        # a plan without a history removes it
        b = d.sample(cond, 2.0, seed=21, use_graph=graph)
        h3 = d.sample(cond, 2.0, seed=21, plan=plan, use_graph=graph)
        assert torch.equal(a, b) and torch.equal(pa, pb) and torch.equal(h1, h2) and torch.equal(h1, h3), (mode, graph)
        assert not torch.equal(pa, h1) and torch.isfinite(h1).all()


# 8 ------------------------------------------------------------------------------------------------
def test_c_abi_set_unset_mismatch_and_refusals():
    from diffsg_amd import _lib
    from test_multistep_cpu import bad_histories
    name = "tiny"
    _, K = M.NETS[name]
    d = make_ddpm(name)
    cond, y_T, _ = M.inputs(name)
    cond, y_T = cond.cuda(), y_T.cuda()
    B, D = y_T.shape
    plan = two_step(d, name)
    rows = plan.history.reshape(-1).tolist()
    L = _lib.lib()
    arr = (ctypes.c_float * (3 * K))(*rows)
    for mode, graph in settings(d):
        flags = 0 if graph else 1
        want = d.sample(cond, 2.0, y_T=y_T, plan=plan, use_graph=graph)
        plain = d.sample(cond, 2.0, y_T=y_T, plan=stripped(plan, None), use_graph=graph)     # the handle holds the grid and no history
        hd = d.model.native_handle()
        coef = plan.coef.cuda().contiguous()
        out = torch.full((B, D), 123.0, device="cuda")
        torch.cuda.synchronize()

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

        assert L.dsg_set_step_history(hd, arr, K) == 0, L.dsg_last_error().decode()
        assert c_sample(K) == 0, L.dsg_last_error().decode()
        torch.cuda.synchronize()
        assert torch.equal(out, want), (mode, graph)
        # another row count than the call's T: refused by all three entry points before anything is enqueued, naming both numbers
        assert L.dsg_set_step_history(hd, (ctypes.c_float * (3 * (K + 2)))(*([0.0] * (3 * (K + 2)))), K + 2) == 0
        out.fill_(123.0)
        torch.cuda.synchronize()
        for fn in ("dsg_sample", "dsg_sample_rec", "dsg_sample_chunked"):
            assert c_sample(K, fn) != 0
            msg = L.dsg_last_error().decode()
            assert str(K) in msg and str(K + 2) in msg and "dsg_set_step_history" in msg, msg
        torch.cuda.synchronize()
        assert bool((out == 123.0).all())
        # refused settings, under the setter's own name, leave the table as it was
        assert L.dsg_set_step_history(hd, arr, K) == 0
        for bad, _ in bad_histories(K):
            flat = [v for r in bad for v in r]
            assert L.dsg_set_step_history(hd, (ctypes.c_float * (3 * K))(*flat), K) != 0
            assert "dsg_set_step_history" in L.dsg_last_error().decode()
        assert L.dsg_set_step_history(hd, arr, -1) != 0 and "dsg_set_step_history" in L.dsg_last_error().decode()
        # chunk variants and a history on one handle: the chunked call names both setters
        om = (ctypes.c_float * 3)(2.0, 2.0, 2.0)
        assert L.dsg_set_chunk_variants(hd, om, None, None, 3, 1) == 0
        assert c_sample(K, "dsg_sample_chunked") != 0
        msg = L.dsg_last_error().decode()
        assert "dsg_set_chunk_variants" in msg and "dsg_set_step_history" in msg, msg
        assert L.dsg_set_chunk_variants(hd, None, None, None, 0, 1) == 0
        # the table survived all of it
        assert c_sample(K) == 0
        torch.cuda.synchronize()
        assert torch.equal(out, want), (mode, graph)
        # unset, both spellings: the plan without a history again
        for unset in (lambda: L.dsg_set_step_history(hd, None, 0), lambda: L.dsg_set_step_history(hd, arr, 0)):
            assert L.dsg_set_step_history(hd, arr, K) == 0
            assert unset() == 0
            assert c_sample(K) == 0
            torch.cuda.synchronize()
            assert torch.equal(out, plain), (mode, graph)
        d.model._native.step_history = None


# 9 ------------------------------------------------------------------------------------------------
def test_history_on_a_non_default_stream():
    name = "nu3"
    d = make_ddpm(name)
    plan = two_step(d, name)
    cond, y_T, z = M.inputs(name)
    cond, y_T, z_all = cond.cuda(), y_T.cuda(), z.cuda()
    side = torch.cuda.Stream()
    for mode, graph in settings(d):
        ref = d.sample(cond, 2.0, y_T=y_T, plan=plan, use_graph=graph)
        d.sample(cond, 2.0, y_T=y_T, noise=z_all, use_graph=graph)     # drop grid and history: the next call sets them again, from inside the stream context
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            got = d.sample(cond, 2.0, y_T=y_T, plan=plan, use_graph=graph)
            again = d.sample(cond, 2.0, y_T=y_T, plan=plan, use_graph=graph)
        side.synchronize()
        assert torch.equal(got, ref) and torch.equal(again, ref), (mode, graph)
