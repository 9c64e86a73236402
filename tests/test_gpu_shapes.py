"""GPU parity over the net shapes dsg_create accepts, not only the five shipped ones (tests/shape_ref.py; DESIGN.md, "Descriptor space").

Which kernels a net runs is decided from its shape by host code: the fused-run choice (create_impl), the 8-wide float32 section, the LDS
phase plan and its fallbacks (prepare_fused), the tile-step kernel's validity, the training tables.  Each catalogue entry reaches one of
those branches; one test id is one descriptor times one concern (plan, forward, sampling, training, captured training), at B = 70 rows
(three row tiles, the last ragged, two or more tiles per CFG pass) and T = 5.

Bounds are those of tests/test_gpu_parity.py, imported: TOL for the forward, `TOL + 3 x budget` for sampling (as
test_sample_large_launch_vs_oracle; budget = float32 oracle against float64 oracle, capped by tests/test_shapes_cpu.py), 1e-5 relative
for the loss and `assert_grads` for every gradient tensor.  The kernel-form switches are held to the contract include/diffsg.h states
for them: bit-identical results.
"""
import ctypes

import pytest
import torch

import shape_ref as S
from oracle import ddpm_oracle as O
from test_gpu_parity import POLICIES, TOL, assert_grads, grad_errs, rel

pytestmark = pytest.mark.gpu

MODES = ["split_f16", "f32"]
T = S.T


def make_ddpm(name, policy="default", mode="split_f16"):
    from diffsg_amd import UNet1D
    from diffsg_amd.classifier_free_MSR import DDPM
    cfg = (S.SHAPES.get(name) or S.REFUSED[name])["cfg"]
    m = UNet1D(**cfg)
    m.load_state_dict(S.net(name)[1], strict=True)
    D = cfg["input_dim"]
    d = DDPM(T, m.to("cuda"), D, 10.0, 1.0 - O.cosine_betas(T), torch.device("cuda"), (1, D), None).to("cuda")
    d.model.set_precision(mode)
    if policy == "large":
        d.model.set_launch_policy(0, 0)
    return d


def plan_of(model):
    """([operator names], (fuse_lo, fuse_hi)) through the introspection the C ABI has (dsg_op_count / dsg_op_info / dsg_fused_range)."""
    from diffsg_amd import _lib
    L, hd = _lib.lib(), model.native_handle()
    names = []
    for i in range(L.dsg_op_count(hd)):
        buf = ctypes.create_string_buffer(64)
        fl, by = ctypes.c_double(), ctypes.c_double()
        _lib.check(L.dsg_op_info(hd, i, buf, ctypes.byref(fl), ctypes.byref(by)))
        names.append(buf.value.decode())
    lo, hi = ctypes.c_int(-1), ctypes.c_int(-1)
    _lib.check(L.dsg_fused_range(hd, ctypes.byref(lo), ctypes.byref(hi)))
    return names, (lo.value, hi.value)


@pytest.mark.parametrize("name", S.NAMES)
def test_plan_reaches_the_branch_the_shape_exists_for(name):
    """The operator list is the reference's module order and the fused narrow run is the first longest run of <= 32-wide operators, worked
    out here from the descriptor alone (shape_ref.longest_narrow_run): empty for `allwide`; for `hill` and `jump` narrow operators are left
    OUTSIDE it (per-operator launches on the split path, chains of one through k_fused_narrow on the exact path); for `flat32` /
    `flat32x4` it is everything between feature_proj and final.

    What the ABI does not show -- phase counts, whether a fallback was taken -- is NOT observed by any test.  What follows is arithmetic
    from the descriptors with the formulas of prepare_fused, worked out by hand, to say which branch each shape should take
    (kNarrowLdsU4 = 9472 uint4 per phase, kNarrowMaxPhases = 4;
    a 32 -> 32 block needs 2 x 128 (W1) + 2 x 2 x 128 (W2, W3) + 2 x 16 + 48 = 848 uint4 + 8 of time bias, a (32 + 32) -> 32 up block
    2 x 4 x 128 (W1, shortcut) + 512 + 2 x 24 + 48 = 1632 + 8, a 32 -> 32 Linear 2 x 128 + 8 = 264):
      * flat32 (n_blocks 1): 6 blocks x 856 + 8 up blocks x 1640 + 6 Linears x 264 = 19 840 uint4: expected three phases;
      * flat32x4: 18 x 856 + 20 x 1640 + 6 x 264 = 49 792 uint4 > 4 x 9472: a fifth phase would be needed, so the plan should be
        dropped and the large-launch policy should run the non-LDS narrow kernel (k_fused_narrow_h);
      * deep8: its run (Downsample 64 -> 32 ... the last 32-wide up block: 37 blocks, 13 Linears) needs 34 104 uint4: expected four
        phases when cut greedily, and the Upsample 32 -> 64 behind it is the tail Linear that joins the last phase only if it still fits;
      * nb4 needs 25 432 uint4 (expected three phases); nb1, skip4 and io128 two; hill, jump and one8 one;
      * nb4 / nb1 end 16 -> 8 with n_blocks outside {2, 3}: the float32 section (v8_lo / v8_hi) stays off, the 8-wide blocks run on the
        matrix cores; deep8 ends 8 -> 4, skip4 16 -> 4: off as well.  `narrow_valu8` 0 must then change nothing (asserted in the
        sampling test against the oracle);
      * the tile-step kernel needs a wide block and a fused run that starts behind feature_proj: off for allwide (no run) and for every
        all-narrow net (no wide block); `tile_step` 0 is bit-identical either way.
    None of this is asserted: the branches are covered through results only, every form being compared with the oracle under both
    launch policies."""
    names, (lo, hi) = plan_of(make_ddpm(name).model)
    flags = S.narrow_flags(name)
    assert names == [n for n, _ in flags]
    assert (lo, hi) == S.longest_narrow_run(name)
    outside = [n for i, (n, f) in enumerate(flags) if f and not lo <= i < hi]
    if name == "allwide":
        assert (lo, hi) == (0, 0) and not outside
    if name in ("hill", "jump"):
        assert hi - lo >= 2 and outside, (lo, hi)
    if name in ("flat32", "flat32x4"):
        assert (lo, hi) == (1, len(names) - 1) and not outside
    if name == "hill":
        assert lo > 3 and set(outside) >= {"down.0.res", "down.1.res"}       # the opening narrow run is not the fused one


@pytest.mark.parametrize("name", S.NAMES)
def test_forward_vs_oracle(name):
    """UNet1D.forward with per-row t and a mixed condition mask at 70 rows, and at a single row, in both precision modes and under both
    launch policies, against O.unet_forward within TOL."""
    for mode in MODES:
        for policy in POLICIES:
            model = make_ddpm(name, policy, mode).model
            for rows in (S.B, 1):
                x, t, cond, mask = S.forward_inputs(name, rows)
                got = model(x.cuda(), t.cuda(), cond.cuda(), mask.cuda())
                e = rel(got, S.forward_ref(name, rows))
                print(f"forward {name}/{mode}/{policy} rows={rows}: rel err {e:.2e}")
                assert e <= TOL, (mode, policy, rows)
            assert not model.range_exceeded()


@pytest.mark.parametrize("name", S.NAMES)
def test_sampling_vs_oracle_and_every_switch(name):
    """DDPM.sample with injected y_T / z at omega 2 and -1 (a negative omega keeps the unconditional pass visible), {split_f16, f32} x
    {default policy, (0, 0)}: within TOL + 3 x budget of O.ddpm_sample.  Per mode and policy, the eager launches and each of `tile_step`,
    `f32_pair`, `panel_half` switched off give the bits of the first (graph) result, as include/diffsg.h promises; `narrow_valu8` 0 changes
    the arithmetic of the 8-wide section where a net has one, so it is held to the oracle bound."""
    cond, y_T, z = S.sample_inputs(name)
    cond = cond.cuda()
    for mode in MODES:
        for policy in POLICIES:
            d = make_ddpm(name, policy, mode)
            for omega in S.OMEGAS:
                ref, budget = S.sample_ref(name, omega)
                first = d.sample(cond, omega, y_T=y_T, noise=z)
                e = rel(first, ref)
                print(f"sample {name}/{mode}/{policy} omega={omega:g}: rel err {e:.2e} (budget {budget:.2e})")
                assert e <= TOL + 3.0 * budget, (mode, policy, omega)
                assert torch.equal(d.sample(cond, omega, y_T=y_T, noise=z, use_graph=False), first), (mode, policy, omega, "eager")
                for opt in ("tile_step", "f32_pair", "panel_half"):
                    d.model.set_option(opt, 0)
                    try:
                        assert torch.equal(d.sample(cond, omega, y_T=y_T, noise=z), first), (mode, policy, omega, opt)
                    finally:
                        d.model.set_option(opt, 1)
                d.model.set_option("narrow_valu8", 0)
                try:
                    e8 = rel(d.sample(cond, omega, y_T=y_T, noise=z), ref)
                finally:
                    d.model.set_option("narrow_valu8", 1)
                print(f"sample {name}/{mode}/{policy} omega={omega:g} narrow_valu8=0: rel err {e8:.2e}")
                assert e8 <= TOL + 3.0 * budget, (mode, policy, omega, "narrow_valu8")
                assert torch.equal(d.sample(cond, omega, y_T=y_T, noise=z), first), (mode, policy, omega, "switches back on")
            assert not d.model.range_exceeded()


def _step(d, y, cond, ts, noise, mask):
    for q in d.model.parameters():
        q.grad = None
    loss = d(y, cond, ts=ts, noise=noise, cond_mask=mask)
    loss.backward()
    return float(loss.detach()), {k: q.grad.detach().clone() for k, q in d.model.named_parameters()}


@pytest.mark.parametrize("name", S.NAMES)
def test_train_step_vs_oracle_twice_on_one_handle(name):
    """One explicit-draws training step (ts, noise, cond_mask given) at 70 rows, both precision modes and both launch policies: loss within
    1e-5 relative and every gradient tensor within `assert_grads` of O.ddpm_loss_and_grads (float32, with the float64 budget).  The step is
    taken twice on the handle: the second one -- which finds the lazily created streams, events and cached tables of the first -- must
    repeat it bit for bit."""
    ref_loss, g32, g64 = S.train_ref(name)
    dev = [t.cuda() for t in S.train_inputs(name)]
    for mode in MODES:
        for policy in POLICIES:
            d = make_ddpm(name, policy, mode)
            loss, got = _step(d, *dev)
            print(f"train {name}/{mode}/{policy}: loss {loss:.6f} (oracle {float(ref_loss):.6f}), max grad err {max(grad_errs(got, g32).values()):.2e}")
            assert abs(loss - float(ref_loss)) <= 1e-5 * abs(float(ref_loss)), (mode, policy)
            assert_grads(got, g32, g64, f"{name}/{mode}/{policy}")
            loss2, got2 = _step(d, *dev)
            assert loss2 == loss, (mode, policy)
            for k in got:
                assert torch.equal(got2[k], got[k]), (mode, policy, k)
            assert not d.model.range_exceeded()


@pytest.mark.parametrize("name", ["hill", "deep8", "flat32x4"])
def test_graph_train_step_is_the_eager_step_bit_for_bit(name):
    """train.StepGraph on off-catalogue shapes, as test_gpu_parity.test_graph_train_step_is_the_eager_step_bit_for_bit: 3 warm-up steps
    + k replays equal 3 + k eager steps of an identical model bit for bit (losses, weights, Adam moments), and the loop continues eagerly
    where the graph left it.  hill: narrow blocks outside the fused run; deep8: 47 blocks, the largest tables; flat32x4: the longest run."""
    from diffsg_amd.train import FlatAdam, StepGraph
    k = 3
    y, cond = (t.cuda() for t in S.train_inputs(name)[:2])

    def fresh():
        d = make_ddpm(name)
        d.device_draws = 321
        return d, FlatAdam(d, lr=5e-3)

    def eager(d, opt):
        loss = d(y, cond)
        loss.backward()
        opt.step()
        opt.zero_grad()
        return float(loss.detach())

    d0, o0 = fresh()
    ref_losses = [eager(d0, o0) for _ in range(3 + k + 1)]
    d1, o1 = fresh()
    sg = StepGraph(d1, o1, y, cond, warmup=3)
    got = [float(sg.step().detach()) for _ in range(k)]
    assert got == ref_losses[3:3 + k], (got, ref_losses)
    sg.close()
    assert eager(d1, o1) == ref_losses[3 + k]
    torch.cuda.synchronize()
    assert torch.equal(o0._flat.detach(), o1._flat.detach())
    s0, s1 = o0.state[o0._flat], o1.state[o1._flat]
    assert torch.equal(s0["exp_avg"], s1["exp_avg"]) and torch.equal(s0["exp_avg_sq"], s1["exp_avg_sq"])
    assert float(s0["step"]) == float(s1["step"]) == 3 + k + 1 and d0._draw_calls == d1._draw_calls == 3 + k + 1


def test_training_refusal_of_a_net_with_too_many_gradient_tensors():
    """dsg_create accepts n_res 8 with n_blocks 4 (shape_ref.REFUSED), and sampling works; the training step tracks max|G| of 3 gradient
    tensors per residual block and 1 per Linear (83 blocks, 18 Linears: 267) in kMaxGmax = 256 slots and refuses the net.  As
    train_step_impl promises for every refusal: before anything is enqueued -- the error names the shape and the limit, the caller's
    gradient bucket and loss are untouched, and the handle samples afterwards exactly as before (and as the oracle does)."""
    from diffsg_amd import _lib
    name, omega = "gmax267", -1.0
    d = make_ddpm(name)
    cond, y_T, z = S.sample_inputs(name)
    cond = cond.cuda()
    ref, budget = S.sample_ref(name, omega)
    before = d.sample(cond, omega, y_T=y_T, noise=z)
    e = rel(before, ref)
    print(f"sample {name} omega={omega:g}: rel err {e:.2e} (budget {budget:.2e})")
    assert e <= TOL + 3.0 * budget
    # the C ABI directly, with a bucket and a loss word that would show any write
    L, hd = _lib.lib(), d.model.native_handle()
    y, c2, ts, noise, mask = (t.cuda() for t in S.train_inputs(name))
    ts32, mk = ts.reshape(-1).int().contiguous(), mask.reshape(-1).contiguous()
    bucket = torch.full((L.dsg_param_total(hd),), 7.0, device="cuda")
    loss = torch.full((1,), 7.0, device="cuda")
    rc = L.dsg_train_step(hd, _lib.ptr(y), _lib.ptr(c2), _lib.ptr(ts32), _lib.ptr(noise), _lib.ptr(mk), _lib.ptr(d.sqrt_alphas_cumprod),
                          _lib.ptr(d.sqrt_one_minus_alphas_cumprod), T, _lib.ptr(bucket), _lib.ptr(loss), S.B, _lib.stream_ptr())
    msg = L.dsg_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0 and "internal" not in msg, msg
    assert "n_res 8" in msg and "n_blocks 4" in msg and "267" in msg and "256" in msg, msg
    assert bool((bucket == 7.0).all()) and float(loss) == 7.0
    with pytest.raises(RuntimeError, match="gradient tensors"):          # and through the module
        d(y, c2, ts=ts, noise=noise, cond_mask=mask)
    assert torch.equal(d.sample(cond, omega, y_T=y_T, noise=z), before)
    assert torch.equal(d.sample(cond, omega, y_T=y_T, noise=z, use_graph=False), before)
