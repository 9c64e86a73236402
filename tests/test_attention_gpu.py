"""UNet1D with AttentionBlocks on the MI355X against the reference-generated goldens (tests/golden/g13_attn_*.npz) and, at
shapes the goldens do not cover, against the torch-CPU restatement of tests/attn_ref.py -- which tests/test_attention_host.py pins
to the golden with max|diff| = 0 (a host test: bit equality of two float32 CPU evaluations holds on the kind of CPU the goldens were
made on, not on every host that carries a GPU).

Bounds are those of tests/test_gpu_parity.py for the corresponding checks without attention, imported from there: TOL = 1e-5 for
forward and sampling goldens (test_unet_forward_vs_golden, test_sample_vs_golden_synth), `TOL + 3 x the reference's own float32
error` for the many-row sampling check (test_sample_large_launch_vs_oracle), 1e-5 relative for the loss and `assert_grads` for
the gradients (test_train_step_vs_reference_golden).  Every check runs under both precision modes, both launch policies and
with the one-launch-per-pass small-batch form (`tile_step`) on and off.
"""
import json

import numpy as np
import pytest
import torch

import attn_ref as AR
from oracle import ddpm_oracle as O
from test_gpu_parity import GTOL, POLICIES, TOL, assert_grads, grad_errs, rel

pytestmark = pytest.mark.gpu

NAMES = sorted(AR.ATTN_CONFIGS)
MODES = ["split_f16", "f32"]
TILE = [1, 0]


def make_ddpm(name, params, T, policy="default", mode="split_f16", tile=1):
    from diffsg_amd import UNet1D
    from diffsg_amd.classifier_free_MSR import DDPM
    cfg = AR.ATTN_CONFIGS[name]
    m = UNet1D(**cfg)
    m.load_state_dict(params, strict=True)
    D = cfg["input_dim"]
    d = DDPM(T, m.to("cuda"), D, 10.0, 1.0 - O.cosine_betas(T), torch.device("cuda"), (1, D), None).to("cuda")
    d.model.set_precision(mode)
    if policy == "large":
        d.model.set_launch_policy(0, 0)
    d.model.set_option("tile_step", tile)
    return d


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("tile", TILE)
def test_unet_forward_vs_golden(gold, name, mode, policy, tile):
    g = gold(f"g13_attn_{name}.npz")
    plan, p = AR.attn_params(name, int(g["w_seed"]))
    model = make_ddpm(name, p, 20, policy, mode, tile).model
    x, cond = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["cond"]).cuda()
    B = x.shape[0]
    eps = model(x, torch.from_numpy(g["a_ts"]).cuda() / int(g["a_T"]), cond, torch.from_numpy(g["a_mask"]).cuda())
    e = [rel(eps, g["a_eps"])]
    t = torch.full((1, B), int(g["b_step"]), dtype=torch.int64, device="cuda") / 20
    e.append(rel(model(x, t, cond, torch.zeros(B, 1, device="cuda")), g["b_eps"]))
    e.append(rel(model(x, t, cond, torch.ones(B, 1, device="cuda")), g["c_eps"]))
    print(f"forward {name}/{mode}/{policy}/tile={tile}: rel err {e}")
    assert max(e) <= TOL
    assert not model.range_exceeded()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("tile", TILE)
@pytest.mark.parametrize("graph", [True, False])
def test_sample_vs_golden(gold, name, mode, policy, tile, graph):
    g = gold(f"g13_attn_{name}.npz")
    plan, p = AR.attn_params(name, int(g["w_seed"]))
    T = int(g["s_T"])
    ddpm = make_ddpm(name, p, T, policy, mode, tile)
    cond = torch.from_numpy(g["s_cond"]).cuda()
    for omega in (0.0, 1.0):
        y0 = ddpm.sample(cond, omega, y_T=torch.from_numpy(g["s_y_T"]), noise=torch.from_numpy(g["s_z"]), use_graph=graph)
        e = rel(y0, g[f"s_om{omega:g}_y0"])
        print(f"sample {name}/{mode}/{policy}/tile={tile}/graph={graph} omega={omega:g}: rel err {e:.2e}")
        assert e <= TOL, omega


def qk_and_norm_views(named, cfg_keys=None):
    """[(key, tensor)] of what an AttentionBlock never touches: all of attn.norm.*, rows 0:2d of attn.projection.*"""
    out = []
    for k, v in named:
        if ".attn.norm." in k:
            out.append((k, v))
        elif ".attn.projection." in k:
            out.append((k + "[q,k rows]", v[: 2 * v.shape[0] // 3]))
    assert out
    return out


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("tile", TILE)
def test_train_step_vs_golden(gold, name, mode, policy, tile):
    g = gold(f"g13_attn_{name}.npz")
    plan, p = AR.attn_params(name, int(g["w_seed"]))
    T = int(g["t_T"])
    ddpm = make_ddpm(name, p, T, policy, mode, tile)
    t = lambda k: torch.from_numpy(g[k])
    y, cond, ts, noise, mask = t("t_y"), t("t_cond"), t("t_ts"), t("t_noise"), t("t_mask")
    ddpm(y.cuda(), cond.cuda(), ts=ts.cuda(), noise=noise.cuda(), cond_mask=mask.cuda()).backward()     # creates the bucket and the pool
    for q in ddpm.model.parameters():
        q.grad = None
    torch.cuda.synchronize()
    assert ddpm._grad_pool
    for w in ddpm._grad_pool:          # the buffer the next step's gradients land in: nothing in it may survive
        w.fill_(12345.0)
    ddpm._grad_bucket.fill_(-777.0)
    loss = ddpm(y.cuda(), cond.cuda(), ts=ts.cuda(), noise=noise.cuda(), cond_mask=mask.cuda())
    loss.backward()
    print(f"train {name}/{mode}/{policy}: loss {float(loss):.8f} golden {float(g['t_loss']):.8f}")
    assert abs(float(loss) - float(g["t_loss"])) <= 1e-5 * abs(float(g["t_loss"]))
    bufs = O.schedule_buffers(1.0 - O.cosine_betas(T))
    _, ref = AR.loss_and_grads(p, plan, bufs, T, y, cond, ts, noise, mask)
    _, ref64 = AR.loss_and_grads(p, plan, bufs, T, y, cond, ts, noise, mask, f64=True)
    got_all = {k: prm.grad for k, prm in ddpm.model.named_parameters()}
    assert all(v is not None for v in got_all.values())
    assert_grads(got_all, ref, ref64, f"attn {name}/{mode}/{policy}")
    # the reference's own autograd output, same per-tensor scale (test_train_step_vs_reference_golden)
    gmax = max(float(v.abs().max()) for v in ref.values())
    budget = grad_errs(ref, ref64)
    for k, got in got_all.items():
        got = got.detach().cpu()
        scale = max(float(ref[k].abs().max()), 1e-3 * gmax)
        tol = GTOL + 4.0 * budget[k]
        if int(g["t_full"]):
            assert float(np.abs(got.numpy() - g["t_grad." + k]).max()) / scale <= tol, k
        else:
            assert float(np.abs(got.reshape(-1)[:16].numpy() - g["t_gradhead." + k]).max()) / scale <= tol, k
    # exact zeros where the reference has None / zero rows, whatever was in the buffers before
    for k, v in qk_and_norm_views(got_all.items()):
        assert torch.count_nonzero(v).item() == 0, k
    for k in json.loads(str(g["t_none"])):
        assert torch.count_nonzero(got_all[k]).item() == 0, k
    assert not (ddpm._grad_bucket == -777.0).any() and not (ddpm._grad_bucket == 12345.0).any()


@pytest.mark.parametrize("mode", MODES)
def test_wide_config_at_4096_rows_vs_cpu_restatement(gold, mode):
    """4 096 rows (256 row tiles in two passes: the large-launch kernel forms) of the wide configuration: forward and a T = 5 sampling
    call against attn_ref (pinned to the golden by test_attention_host.test_cpu_restatement_is_the_reference)."""
    name, B, T = "wide", 4096, 5
    g = gold(f"g13_attn_{name}.npz")
    plan, p = AR.attn_params(name, int(g["w_seed"]))
    cfg = AR.ATTN_CONFIGS[name]
    # the restatement on THIS host against the reference-generated golden at the golden's shape, before it is trusted: bit equality is
    # test_attention_host's (it holds on the kind of CPU the goldens were made on); here the bound is the restatement's own float32
    # error against its float64 evaluation, x3 as in test_sample_large_launch_vs_oracle
    gt = lambda k: torch.from_numpy(g[k])
    with torch.no_grad():
        h32 = AR.unet_forward(p, plan, gt("x"), gt("a_ts") / int(g["a_T"]), gt("cond"), gt("a_mask"))
        h64 = AR.unet_forward({k: v.double() for k, v in p.items()}, plan, gt("x").double(), (gt("a_ts") / int(g["a_T"])).double(), gt("cond").double(),
                              gt("a_mask").double())
    pin, own = rel(h32, g["a_eps"]), rel(h32, h64)
    print(f"restatement vs golden on this host: {pin:.2e} (its float32 vs float64: {own:.2e})")
    assert pin <= 3.0 * own
    ddpm = make_ddpm(name, p, T, "default", mode)
    gen = torch.Generator().manual_seed(9)
    cond = torch.rand(B, cfg["cond_dim"], generator=gen)
    x = torch.randn(B, cfg["input_dim"], generator=gen)
    ts = torch.randint(0, 50, (1, B), generator=gen)
    mask = (torch.rand(B, 1, generator=gen) < 0.8).float()
    with torch.no_grad():
        ref = AR.unet_forward(p, plan, x, ts / 50, cond, mask)
    e = rel(ddpm.model(x.cuda(), (ts / 50).cuda(), cond.cuda(), mask.cuda()), ref)
    print(f"wide/{mode} B={B}: forward rel err {e:.2e}")
    assert e <= TOL                                            # test_unet_forward_vs_oracle_ragged
    y_T = torch.randn(B, cfg["input_dim"], generator=gen)
    z = torch.randn(T - 2, B, cfg["input_dim"], generator=gen)
    zd = {i: z[j] for j, i in enumerate(range(T - 1, 1, -1))}
    bufs = O.schedule_buffers(1.0 - O.cosine_betas(T))
    p64 = {k: v.double() for k, v in p.items()}
    for policy in POLICIES:
        if policy == "large":
            ddpm.model.set_launch_policy(0, 0)
        y0 = ddpm.sample(cond.cuda(), 2.0, y_T=y_T, noise=z)
        ref = AR.sample(p, plan, bufs, T, cond, 2.0, y_T, zd)
        ref64 = AR.sample(p64, plan, {k: v.double() for k, v in bufs.items()}, T, cond.double(), 2.0, y_T.double(), {i: v.double() for i, v in zd.items()})
        e, budget = rel(y0, ref), rel(ref, ref64)
        print(f"wide/{mode}/{policy} B={B} T={T}: sample rel err {e:.2e} (restatement float32 vs float64: {budget:.2e})")
        assert e <= TOL + 3.0 * budget                         # test_sample_large_launch_vs_oracle
    assert not ddpm.model.range_exceeded()


@pytest.mark.parametrize("name,B", [("nu", 512), ("wide", 2048)])
def test_graph_train_step_is_the_eager_step_bit_for_bit(name, B):
    """train.StepGraph on an attention net: 3 replays equal 3 eager steps of an identical model bit for bit (losses, weights, moments)."""
    from diffsg_amd.train import FlatAdam, StepGraph
    T, k = 20, 3
    cfg = AR.ATTN_CONFIGS[name]
    gen = torch.Generator().manual_seed(B)
    y = (torch.rand(B, cfg["input_dim"], generator=gen) * 0.25).cuda()
    cond = torch.rand(B, cfg["cond_dim"], generator=gen).cuda()

    def fresh():
        plan, p = AR.attn_params(name)
        d = make_ddpm(name, p, T)
        d.device_draws = 321
        return d, FlatAdam(d, lr=5e-3)

    def eager(d, opt):
        loss = d(y, cond)
        loss.backward()
        opt.step()
        opt.zero_grad()
        return float(loss.detach())

    d0, o0 = fresh()
    ref_losses = [eager(d0, o0) for _ in range(3 + k)]
    d1, o1 = fresh()
    sg = StepGraph(d1, o1, y, cond, warmup=3)
    got = [float(sg.step().detach()) for _ in range(k)]
    assert got == ref_losses[3:3 + k], (got, ref_losses)
    sg.close()
    torch.cuda.synchronize()
    assert torch.equal(o0._flat.detach(), o1._flat.detach())
    s0, s1 = o0.state[o0._flat], o1.state[o1._flat]
    assert torch.equal(s0["exp_avg"], s1["exp_avg"]) and torch.equal(s0["exp_avg_sq"], s1["exp_avg_sq"])
    assert len(set(ref_losses)) == len(ref_losses)              # the weights moved every step


@pytest.mark.parametrize("name", NAMES)
def test_ema_and_flat_adam_leave_the_unused_attention_tensors_alone(name):
    """attn.norm.* and the q / k rows of attn.projection.* have zero gradients: FlatAdam steps (no weight decay) leave them bit-unchanged
    and move everything else; the EMA of the stepped model sees an unchanged value there (see `want` below) and a moving one elsewhere."""
    from diffsg_amd.train import FlatAdam
    T, B = 20, 96
    cfg = AR.ATTN_CONFIGS[name]
    plan, p = AR.attn_params(name)
    d = make_ddpm(name, p, T)
    keys = list(d.model.state_dict())
    opt = FlatAdam(d, lr=2e-3)
    assert list(d.model.state_dict()) == keys
    gen = torch.Generator().manual_seed(5)
    d.ema.update_parameters(d.model)                  # first update = copy
    for step in range(2):
        y = torch.rand(B, cfg["input_dim"], generator=gen).cuda()
        cond = torch.rand(B, cfg["cond_dim"], generator=gen).cuda()
        d(y, cond).backward(); opt.step(); opt.zero_grad()
        d.ema.update_parameters(d.model)
    torch.cuda.synchronize()
    # what an untouched tensor reads: the model's is bit-unchanged; the EMA's went twice through avg = decay * avg + (1 - decay) * p with
    # p the unchanged value, which in float32 (ema.py:11-12, the reference's arithmetic) returns that value only up to the rounding of
    # the two products -- so the expectation is the library's own update applied twice to a copy, with the ORIGINAL value as its source
    from diffsg_amd import _lib

    def ema_of_constant(v0):
        avg, src = v0.cuda().clone().contiguous(), v0.cuda().contiguous()
        for _ in range(2):
            _lib.check(_lib.lib().dsg_ema_update(_lib.ptr(avg), _lib.ptr(src), d.ema.decay, 1.0 - d.ema.decay, avg.numel(), _lib.stream_ptr()))
        torch.cuda.synchronize()
        return avg.cpu()

    for tag, sd in (("model", d.model.state_dict()), ("ema", d.ema.module.state_dict())):
        for k, v in sd.items():
            v = v.detach().cpu()
            want = p[k] if tag == "model" else ema_of_constant(p[k])
            if ".attn.norm." in k:
                assert torch.equal(v, want), (tag, k)
            elif ".attn.projection." in k:
                n = 2 * v.shape[0] // 3
                assert torch.equal(v[:n], want[:n]), (tag, k)
                assert not torch.equal(v[n:], want[n:]), (tag, k)
            else:
                assert not torch.equal(v, want), (tag, k)
    # the stepped weights are what the library computes with
    x = torch.rand(B, cfg["input_dim"], generator=gen)
    cond = torch.rand(B, cfg["cond_dim"], generator=gen)
    t = torch.full((1, B), 0.5)
    m = torch.ones(B, 1)
    now = {k: v.detach().cpu() for k, v in d.model.state_dict().items()}
    with torch.no_grad():
        ref = AR.unet_forward(now, plan, x, t, cond, m)
    assert rel(d.model(x.cuda(), t.cuda(), cond.cuda(), m.cuda()), ref) <= TOL


@pytest.mark.parametrize("graph", [True, False])
def test_exact_path_sampling_of_a_net_with_two_narrow_runs(graph):
    """No attention: proj_dim 32, dims (64, 32) has a 32-wide block in front of the 64-wide ones and the narrow bottom behind them, so only
    the longer narrow run is fused and the exact path launches the other narrow operators one by one inside dsg_sample.  With two row
    tiles per pass the unconditional pass of those launches was wrong by 1e-2 (omega = 0 hides it: eps = eps1).  Bound: TOL, as
    test_sample_vs_golden_synth."""
    from diffsg_amd import UNet1D
    from diffsg_amd.classifier_free_MSR import DDPM
    from weights import synth_weights
    cfg = dict(input_dim=5, proj_dim=32, cond_dim=6, dims=(64, 32), n_blocks=1)
    plan = O.unet_plan(cfg["input_dim"], cfg["proj_dim"], cfg["cond_dim"], cfg["dims"], cfg["n_blocks"])
    p = {k: torch.from_numpy(v) for k, v in synth_weights(O.state_shapes(plan), 3, "trained").items()}
    T, B, D = 6, 40, cfg["input_dim"]
    gen = torch.Generator().manual_seed(1)
    cond = torch.rand(B, cfg["cond_dim"], generator=gen)
    y_T = torch.randn(B, D, generator=gen)
    z = torch.randn(T - 2, B, D, generator=gen)
    bufs = O.schedule_buffers(1.0 - O.cosine_betas(T))
    for mode in MODES:
        m = UNet1D(**cfg)
        m.load_state_dict(p)
        d = DDPM(T, m.to("cuda"), D, 10.0, 1.0 - O.cosine_betas(T), torch.device("cuda"), (1, D), None).to("cuda")
        d.model.set_precision(mode)
        for omega in (-1.0, 1.0):
            ref = O.ddpm_sample(p, plan, bufs, T, cond, omega, y_T, {i: z[j] for j, i in enumerate(range(T - 1, 1, -1))})
            e = rel(d.sample(cond.cuda(), omega, y_T=y_T, noise=z, use_graph=graph), ref)
            print(f"two narrow runs {mode} omega={omega:g} graph={graph}: rel err {e:.2e}")
            assert e <= TOL, (mode, omega)


def test_range_flag_of_the_split_attention_operator():
    """The >= 64-wide operator splits two RAW operands on the default path: x and v.  With output.weight = 0 the block is the identity
    plus a bias, so nothing behind it sees a large value; a v-bias of 1e5 then leaves fp16's range in ONE place only, the operand of the
    second product, and the handle's flag must come up (dsg_range_status) -- and stay down with the bias at 1, and in the exact mode,
    which splits nothing."""
    name = "wide"
    cfg = AR.ATTN_CONFIGS[name]
    plan, p = AR.attn_params(name)
    d = cfg["proj_dim"]
    gen = torch.Generator().manual_seed(3)
    B = 64
    x = torch.randn(B, cfg["input_dim"], generator=gen).cuda()
    cond = torch.rand(B, cfg["cond_dim"], generator=gen).cuda()
    t = torch.full((1, B), 0.5).cuda()
    m = torch.ones(B, 1).cuda()
    for bias, mode, want in ((1.0, "split_f16", False), (1e5, "split_f16", True), (1e5, "f32", False)):
        q = {k: v.clone() for k, v in p.items()}
        q["down.0.attn.output.weight"].zero_()
        q["down.0.attn.projection.bias"][2 * d:] = bias
        model = make_ddpm(name, q, 20, "default", mode).model
        assert not model.range_exceeded()
        out = model(x, t, cond, m)
        assert torch.isfinite(out).all()
        assert model.range_exceeded() == want, (bias, mode)
        with torch.no_grad():
            ref = AR.unet_forward(q, plan, x.cpu(), t.cpu(), cond.cpu(), m.cpu())
        if not want:
            assert rel(out, ref) <= TOL, (bias, mode)
