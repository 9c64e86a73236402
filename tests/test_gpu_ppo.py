"""PPO baseline on the device: dsg_ppo_forward / dsg_ppo_loss_grad / dsg_ppo_train_epoch and diffsg_amd.ppo.

Goldens: tests/golden/g15_ppo.npz (torch on the CPU and the reference's PPOAgent, losses and environment steps;
make_ppo_goldens.py asserts that no ratio of a golden case sits at a clip bound, no CO action at the offload threshold, and that
the reward amplifies an objective's error by at most 10: no tolerance below allows for a flipped branch).
All tests need an MI355X: run with `-m gpu`."""
import ctypes
import os

import numpy as np
import pytest
import torch

from _util import GOLD
import ppo_ref as PR

pytestmark = pytest.mark.gpu

TOL = 1e-5      # forward: max|a - b| / max|b|, the bar tests/test_gpu_parity.py holds the denoiser to
GTOL = 1e-4     # gradients, per tensor on the grad_errs scale
ATOL = 1e-3     # parameters after three Adam steps (rel), the bar of the project's three-step Adam test


@pytest.fixture(scope="module")
def g15():
    return np.load(os.path.join(GOLD, "g15_ppo.npz"))


def rel(a, b):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64)
    b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def grad_errs(got, ref):
    """tests/test_gpu_parity.py's scale: max|got - ref| / max(max|ref_k|, 1e-3 * global max|ref|) per tensor."""
    gmax = max(float(np.abs(v).max()) for v in ref.values())
    return {k: float(np.abs(np.asarray(got[k], dtype=np.float64) - ref[k]).max()) / max(float(np.abs(ref[k]).max()), 1e-3 * gmax) for k in ref}


def build(case):
    from diffsg_amd import PPOAgent
    return PPOAgent(PR.CASES[case]["S"], PR.CASES[case]["A"])


def state(g15, case, tag):
    if tag == "trained":
        return {k: g15[f"{case}.trained.w.{k}"] for k, _ in PR.case_shapes(case)}
    torch.manual_seed(int(g15[f"{case}.init.seed"]))
    return {k: v.detach().numpy().copy() for k, v in build(case).state_dict().items()}


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype).contiguous()


def desc_of(case, env=True):
    from diffsg_amd.ppo import ppo_desc
    c = PR.CASES[case]
    return ppo_desc(c["S"], c["A"], c["env"] if env else None, c["cfg"])


def golden_inputs(g15, case, tag):
    """(flat parameters, X, Y, old_logp, noise, noise2) of a golden case and state, on the device."""
    X, Y, noise, noise2 = PR.inputs(case, int(g15[f"{case}.{tag}.seed"]))
    return tuple(dev(a) for a in (PR.flat(state(g15, case, tag), case), X, Y, g15[f"{case}.{tag}.old_logp"], noise, noise2))


def adam_range(p, g, m, v, A, step, lr=PR.LR):
    """dsg_adam_step over the critic and actor range [A, P) of flat tensors (through 16-byte aligned copies: elementwise, so the
    same bits)."""
    from diffsg_amd import _lib
    t = [x[A:].clone() for x in (p, g, m, v)]
    _lib.check(_lib.lib().dsg_adam_step(_lib.ptr(t[0]), _lib.ptr(t[1]), _lib.ptr(t[2]), _lib.ptr(t[3]), t[0].numel(), lr, 0.9, 0.999, 1e-8, 0.0, 0,
                                        step, _lib.stream_ptr()))
    p[A:], m[A:], v[A:] = t[0], t[2], t[3]


FORWARD = [(c, t, PR.ROWS) for c in PR.CASES for t in ("init", "trained")] + [("nu3", "trained", r) for r in (1, 63, 257)]


@pytest.mark.parametrize("case,tag,rows", FORWARD)
def test_forward_against_goldens(g15, case, tag, rows):
    """Measured on an MI355X: mu 2.1e-07 .. 9.2e-07, value 2.3e-07 .. 8.8e-07 over the eleven cases (worst: msr3.init mu 9.21e-07,
    msr80.init value 8.81e-07); the bar is 1e-5."""
    from diffsg_amd.ppo import forward_flat
    p, X = golden_inputs(g15, case, tag)[:2]
    idx = np.arange(rows) % PR.ROWS                 # 257 rows: the golden rows again (a fifth tile, short)
    mu, value = forward_flat(desc_of(case, env=False), p, X[idx].contiguous())
    e_mu, e_v = rel(mu, g15[f"{case}.{tag}.mu"][idx]), rel(value, g15[f"{case}.{tag}.value"][idx])
    print(f"forward {case}.{tag} rows {rows}: mu {e_mu:.2e}, value {e_v:.2e}")
    assert mu.shape == (rows, PR.CASES[case]["A"]) and value.shape == (rows,)
    assert e_mu < TOL and e_v < TOL


@pytest.mark.parametrize("tag", ["init", "trained"])
@pytest.mark.parametrize("case", list(PR.CASES))
def test_one_batch_against_goldens(g15, case, tag):
    """new_logp (TOL), the reward per row within TOL * kappa_row of the golden (the objectives' 1e-5 bar carried through reward =
    1 / (|c - gt| + offset); kappa from the golden's own objectives), both losses (1e-5 * kappa_max relative), every gradient tensor
    (GTOL), the log_std slots exactly zero.
    Measured on an MI355X for co3, msr3 and msr80 (both states): new_logp 0 .. 2.4e-07 (bar 1e-5); reward, worst row as a fraction of
    its TOL * kappa bound 0.014 .. 0.056 (kappa 1.0 .. 1.85); actor loss 0 .. 2.4e-07, critic loss 0 .. 2.3e-07 (bar 1e-5 * kappa_max);
    reward sum 3.6e-08 .. 3.1e-07; worst gradient tensor 4.0e-07 .. 8.0e-07, and 1.50e-06 for msr80.init (bar 1e-4).
    NOT YET MEASURED: the two nu3 cases as they stand.  Their one device run was on an earlier golden with P_sum = 18, where kappa is
    0.0015 .. 0.01, TOL * kappa lies below one float32 ulp of the reward, and 1-ulp differences (9.6e-08) missed that bound by 2x; the
    golden's P_sum is now 1e5 (kappa 1.0 .. 1.16, tests/ppo_ref.py says why) and no device was available after that change."""
    from diffsg_amd.ppo import loss_grad
    g = lambda k: g15[f"{case}.{tag}.{k}"]      # noqa: E731
    m = build(case)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state(g15, case, tag).items()}, strict=True)
    m.to("cuda")
    _, X, Y, old, noise, _ = golden_inputs(g15, case, tag)
    out3, new_logp, reward, grads = loss_grad(m, X, Y, old, noise, dict(PR.CASES[case]["cfg"], env=PR.CASES[case]["env"]))
    kappa = (np.abs(g("cost")) + np.abs(g("gt"))) / (np.abs(g("cost") - g("gt")) + PR.OFFSET[PR.CASES[case]["env"]])
    want_r = g("reward").astype(np.float64)
    r_err = np.abs(reward.cpu().numpy().astype(np.float64) - want_r) / want_r
    a_err = abs(out3[0].item() - float(g("actor_loss"))) / abs(float(g("actor_loss")))
    c_err = abs(out3[1].item() - float(g("critic_loss"))) / float(g("critic_loss"))
    ref = {k: g("grad." + k).astype(np.float64) for k in grads if k != "log_std"}
    errs = grad_errs({k: v.cpu().numpy() for k, v in grads.items()}, ref)
    print(f"one batch {case}.{tag}: new_logp {rel(new_logp, g('new_logp')):.2e}, reward worst row {r_err.max():.2e} (worst err / (TOL kappa) "
          f"{(r_err / (TOL * kappa)).max():.3f}, kappa {kappa.min():.3g} .. {kappa.max():.3g}), actor loss {a_err:.2e}, critic loss {c_err:.2e}, "
          f"reward sum {abs(out3[2].item() - want_r.sum()) / want_r.sum():.2e}, worst grad tensor {max(errs.values()):.2e}")
    assert [tuple(v.shape) for v in grads.values()] == [s for _, s in PR.case_shapes(case)]
    assert rel(new_logp, g("new_logp")) < TOL
    assert np.all(r_err <= TOL * kappa), (r_err / (TOL * kappa)).max()
    assert a_err < 1e-5 * kappa.max() and c_err < 1e-5 * kappa.max()
    assert abs(out3[2].item() - want_r.sum()) <= TOL * kappa.max() * want_r.sum()       # the sum behind fit's "Reward:" line
    assert max(errs.values()) < GTOL, errs
    assert not grads["log_std"].any() and grads["log_std"].shape == (1, PR.CASES[case]["A"])


@pytest.mark.parametrize("tag", ["init", "trained"])
@pytest.mark.parametrize("case", list(PR.CASES))
def test_three_adam_steps_against_goldens(g15, case, tag):
    """Batches [0:64], [64:70], [0:70]: one epoch of 70 rows at batch 64 (identity order), then one of batch 70 from step 2 with the
    first epoch's new_logp as old_logp (the kernel left it there) and noise2.  The step losses are held to 1e-5 * the largest kappa
    of the three batches (1.1 .. 1.9), the parameters to 1e-3.  NOT YET MEASURED on a device: no figure is recorded here."""
    from diffsg_amd.ppo import train_epoch_flat
    desc = desc_of(case)
    p, X, Y, old, noise, noise2 = golden_inputs(g15, case, tag)
    p, old = p[None].contiguous(), old[None].contiguous()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    ident = torch.arange(PR.ROWS, device="cuda", dtype=torch.int32)[None].contiguous()
    b1 = train_epoch_flat(desc, p, m, v, X, Y, old, noise[None].contiguous(), ident, 64, PR.LR, 0)
    b2 = train_epoch_flat(desc, p, m, v, X, Y, old, noise2[None].contiguous(), ident, PR.ROWS, PR.LR, 2)
    l_err = rel(torch.cat((b1[0], b2[0]))[:, :2], g15[f"{case}.{tag}.step_loss"])
    got = PR.unflat(p[0].cpu().numpy(), case)
    errs = {k: rel(got[k], g15[f"{case}.{tag}.adam.{k}"]) for k in got}
    print(f"adam x3 {case}.{tag}: step losses {l_err:.2e}, worst tensor {max(errs.values()):.2e}")
    assert l_err < 1e-5 * float(g15[f"{case}.{tag}.step_kappa"].max())
    assert max(errs.values()) < ATOL, errs


def compose(desc, p0, X, Y, old0, noise, perm, batch, step0=0, lr=PR.LR):
    """The epoch from dsg_ppo_loss_grad + dsg_adam_step, one batch at a time, on the gathered rows."""
    from diffsg_amd.ppo import loss_grad_flat
    A = desc.action_dim
    p, m, v, old = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0), old0.clone()
    N, outs = perm.numel(), []
    for k, lo in enumerate(range(0, N, batch)):
        idx = perm[lo:lo + batch].long()
        out3, new_logp, _, g = loss_grad_flat(desc, p, X[idx].contiguous(), Y[idx].contiguous(), old[idx].contiguous(),
                                              noise[lo:lo + batch].contiguous())
        adam_range(p, g, m, v, A, step0 + k + 1, lr)
        old[idx] = new_logp
        outs.append(out3)
    return p, m, v, torch.stack(outs), old


@pytest.mark.parametrize("batch", [64, 128, 512])
@pytest.mark.parametrize("case", ["co3", "nu3", "msr80"])
def test_epoch_is_the_composition_bit_for_bit(g15, case, batch):
    """N = 150.  Batch 64: three batches, the last with 22 rows; a full batch is two tiles for msr80 (tiles of 32 rows) and ONE tile for
    co3 / nu3 (tiles of 64).  Batch 128: two batches (128 and 22 rows), the first of two tiles for co3 / nu3 and four for msr80 -- several
    batches with several tiles each on chip, NU's min / max crossing tiles.  Batch 512 > N: one batch of tiles 64 + 64 + 22."""
    from diffsg_amd.ppo import train_epoch_flat
    N = 150
    desc = desc_of(case)
    p0, X, Y, old, noise, noise2 = golden_inputs(g15, case, "trained")
    rows = torch.arange(N, device="cuda") % PR.ROWS
    X, Y = X[rows].contiguous(), Y[rows].contiguous()
    gen = torch.Generator().manual_seed(batch)
    old0 = (old[rows] + 0.05 * torch.randn(N, desc.action_dim, generator=gen).cuda()).contiguous()
    nz = torch.randn(N, desc.action_dim, generator=gen).cuda().contiguous()
    perm = torch.randperm(N, generator=gen).to(device="cuda", dtype=torch.int32)
    want = compose(desc, p0, X, Y, old0, nz, perm, batch)
    p, m, v, o = p0.clone()[None], torch.zeros_like(p0)[None], torch.zeros_like(p0)[None], old0.clone()[None]
    bo = train_epoch_flat(desc, p, m, v, X, Y, o, nz[None], perm[None].contiguous(), batch, PR.LR, 0)
    assert bo.shape == (1, (N + batch - 1) // batch, 3)
    diff = {name: (int((a != b).sum()), a.numel(), float((a - b).abs().max()))
            for name, a, b in zip(("params", "exp_avg", "exp_avg_sq", "batch_out", "old_logp"), (p[0], m[0], v[0], bo[0], o[0]), want)
            if not torch.equal(a, b)}
    assert not diff, f"(elements that differ, of, max |difference|): {diff}"
    A = desc.action_dim
    assert not torch.equal(p[0], p0) and torch.equal(p[0][:A], p0[:A]) and not torch.equal(o[0], old0)
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(bo).all())


def test_replicas_are_independent_and_deterministic(g15):
    from diffsg_amd.ppo import train_epoch_flat
    case = "nu3"
    desc = desc_of(case)
    _, X, Y, old, _, _ = golden_inputs(g15, case, "trained")
    R, batch, A = 3, 40, desc.action_dim
    p0 = torch.stack([dev(PR.flat(PR.synth_state(case, 100 + r), case)) for r in range(R)]).contiguous()
    gen = torch.Generator().manual_seed(9)
    perm = torch.stack([torch.randperm(PR.ROWS, generator=gen) for _ in range(R)]).to(device="cuda", dtype=torch.int32)
    noise = torch.randn(R, PR.ROWS, A, generator=gen).cuda()
    old0 = (old[None] + 0.05 * torch.randn(R, PR.ROWS, A, generator=gen).cuda()).contiguous()

    def run(sl, step0=5):
        p, m, v, o = p0[sl].clone(), torch.full_like(p0[sl], 0.01), torch.full_like(p0[sl], 1e-4), old0[sl].clone()
        return p, m, v, o, train_epoch_flat(desc, p, m, v, X, Y, o, noise[sl].contiguous(), perm[sl].contiguous(), batch, PR.LR, step0)

    both = run(slice(0, R))
    again = run(slice(0, R))
    assert all(torch.equal(a, b) for a, b in zip(both, again))
    for r in range(R):
        one = run(slice(r, r + 1))
        assert all(torch.equal(a[r:r + 1], b) for a, b in zip(both, one)), r
    assert not torch.equal(both[0][0], both[0][1])


def test_refusals_launch_nothing():
    from diffsg_amd import _lib
    from diffsg_amd.ppo import ppo_desc
    d = ppo_desc(9, 3, "co", dict(scaler_min=0.0, scaler_max=1.0), hidden=(64, 65, 32))
    L = _lib.lib()
    x, y = torch.rand(8, 9, device="cuda"), torch.rand(8, 3, device="cuda")
    par, mu, val = torch.zeros(40000, device="cuda"), torch.full((8, 3), -7.0, device="cuda"), torch.full((8,), -7.0, device="cuda")
    grad, out3 = torch.full((40000,), -7.0, device="cuda"), torch.full((3,), -7.0, device="cuda")
    perm = torch.arange(8, device="cuda", dtype=torch.int32)
    s = _lib.stream_ptr()
    calls = {
        "dsg_ppo_forward": lambda: L.dsg_ppo_forward(ctypes.byref(d), _lib.ptr(par), _lib.ptr(x), _lib.ptr(mu), _lib.ptr(val), 8, s),
        "dsg_ppo_loss_grad": lambda: L.dsg_ppo_loss_grad(ctypes.byref(d), _lib.ptr(par), _lib.ptr(x), _lib.ptr(y), _lib.ptr(y), _lib.ptr(y), 8,
                                                         _lib.ptr(out3), _lib.ptr(mu), _lib.ptr(val), _lib.ptr(grad), s),
        "dsg_ppo_train_epoch": lambda: L.dsg_ppo_train_epoch(ctypes.byref(d), _lib.ptr(par), _lib.ptr(grad), _lib.ptr(grad), _lib.ptr(x), _lib.ptr(y),
                                                             _lib.ptr(mu), _lib.ptr(y), _lib.ptr(perm), 8, 4, 0.005, 0.9, 0.999, 1e-8, 0,
                                                             _lib.ptr(out3), 1, s),
    }
    for name, call in calls.items():
        assert call() != 0, name
        msg = L.dsg_last_error().decode()
        assert name in msg and len(msg) > len(name) + 4, msg
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in (mu, val, grad, out3)) and bool((par == 0).all())
    ok = ppo_desc(9, 3, "co", dict(scaler_min=0.0, scaler_max=1.0))
    assert L.dsg_ppo_forward(ctypes.byref(ok), None, None, None, None, 0, s) == 0
    assert L.dsg_ppo_loss_grad(ctypes.byref(ok), None, None, None, None, None, 0, None, None, None, None, s) == 0
    assert L.dsg_ppo_train_epoch(ctypes.byref(ok), None, None, None, None, None, None, None, None, 0, 512, 0.005, 0.9, 0.999, 1e-8, 0, None, 1,
                                 s) == 0


def test_agent_forward_and_fit_on_the_co_fixture(g15):
    """PPOAgent.forward under no_grad on the device is forward_flat (and follows the parameters); eight epochs of `fit` on the 200-row
    CO fixture run, log the reference's lines and leave finite parameters; a replica trains beside the agent."""
    from diffsg_amd import PPOAgent
    from diffsg_amd.classifier_free_CO import co_data_load
    from diffsg_amd.ppo import agent_desc, fit, flat_params, forward_flat
    X_train, Y_train, _, _, cfg = co_data_load(os.path.join(GOLD, "data", "3nodes_200samples_ood.csv"))
    torch.manual_seed(1)
    a, b = PPOAgent(9, 3).to("cuda"), PPOAgent(9, 3).to("cuda")
    xd = dev(X_train)
    with torch.no_grad():
        value, dist = a(xd)
    mu, val = forward_flat(agent_desc(a), flat_params(a), xd)
    assert torch.equal(dist.mean, mu) and torch.equal(value, val[:, None]) and torch.equal(dist.stddev, a.log_std.exp().expand_as(mu))
    with torch.enable_grad():
        v2, d2 = a(xd)
    assert v2.requires_grad and rel(mu, d2.mean) < TOL and rel(val, v2[:, 0]) < TOL
    before = flat_params(a).clone()
    lines = []
    torch.manual_seed(3)
    hist = fit(a, X_train, Y_train, dict(cfg, env="co"), 8, batch_size=64, replicas=[a, b], log=lines.append)
    assert len(hist) == 8 and len(hist[0]) == 2 and len(hist[0][0]) == 3 and len(lines) == 16
    assert lines[0].startswith("Epoch: 0, Actor loss: ") and ", Critic loss: " in lines[0] and lines[1].startswith("Reward: ")
    after = flat_params(a)
    assert bool(torch.isfinite(after).all()) and bool(torch.isfinite(flat_params(b)).all()) and np.isfinite(np.array(hist)).all()
    assert not torch.equal(after, before) and torch.equal(after[:3], before[:3])        # log_std is not trained
    with torch.no_grad():                                                                # the cached flat vector follows the parameters
        moved = a(xd)[1].mean
    assert not torch.equal(moved, mu) and torch.equal(moved, forward_flat(agent_desc(a), after, xd)[0])
    with torch.no_grad(), pytest.raises(RuntimeError):
        PPOAgent(9, 3)(xd)


@pytest.mark.parametrize("problem", ["co", "msr", "nu"])
def test_drivers_run_on_the_fixture_data(problem, tmp_path):
    """ppo_co / ppo_msr / ppo_nu end to end on the 200-row fixtures, two epochs: training, the evaluation loop (CO samples, MSR and NU
    use the mean; NU decodes per evaluation batch), both scorings on the device, and the saved state dict loads strictly."""
    from diffsg_amd import PPOAgent, ppo
    path = os.path.join(GOLD, "data", {"co": "3nodes_200samples_ood.csv", "msr": "3c_10w_200samples.csv", "nu": "3u_18mW_200samples.csv"}[problem])
    save = str(tmp_path / "agent.pt")
    torch.manual_seed(4)
    agent, out = getattr(ppo, "ppo_" + problem)(path, epochs=2, batch_size=64, save_path=save, log=None)
    assert len(out["history"]) == 2 and np.isfinite(np.array(out["history"])).all()
    for k in ("sum_ratio_reference_order", "mean_diff_reference_order", "sum_ratio_aligned", "mean_diff_aligned"):
        assert np.isfinite(out[k]), (k, out[k])
    assert out["sum_ratio_aligned"] > 0
    sd = torch.load(save, map_location="cpu")
    fresh = PPOAgent(agent.state_dim, agent.action_dim)
    fresh.load_state_dict(sd, strict=True)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(agent.state_dict().values(), sd.values())) and not sd["log_std"].any()
