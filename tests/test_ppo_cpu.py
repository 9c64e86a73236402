"""PPO baseline, host side (no GPU): the float64 restatement against the goldens recorded from torch and the reference's classes,
the agent's layout and seeded initialisation, the shipped checkpoints, the composed permutations `fit` trains on, and the refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.utils.data as data

from _util import GOLD
import ppo_ref as PR

FTOL = 1e-6     # forward: float64 numpy against float32 torch, max|a - b| / max|b|
TOL = 1e-5      # losses (relative) and gradients (per tensor on the grad_errs scale)
ATOL = 1e-3     # parameters after three Adam steps (rel), the bar of the project's three-step Adam test


@pytest.fixture(scope="module")
def g15():
    return np.load(os.path.join(GOLD, "g15_ppo.npz"))


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def grad_errs(got, ref):
    gmax = max(float(np.abs(v).max()) for v in ref.values())
    return {k: float(np.abs(np.asarray(got[k], dtype=np.float64) - ref[k]).max()) / max(float(np.abs(ref[k]).max()), 1e-3 * gmax) for k in ref}


def build(case):
    from diffsg_amd import PPOAgent
    return PPOAgent(PR.CASES[case]["S"], PR.CASES[case]["A"])


def state(g15, case, tag):
    """The weight state of a golden case: `trained` is stored, `init` is the seeded construction of this package's module."""
    if tag == "trained":
        return {k: g15[f"{case}.trained.w.{k}"] for k, _ in PR.case_shapes(case)}
    torch.manual_seed(int(g15[f"{case}.init.seed"]))
    return {k: v.detach().numpy().copy() for k, v in build(case).state_dict().items()}


@pytest.mark.parametrize("tag", ["init", "trained"])
@pytest.mark.parametrize("case", list(PR.CASES))
def test_restatement_against_goldens(g15, case, tag):
    g = lambda k: g15[f"{case}.{tag}.{k}"]      # noqa: E731
    w = state(g15, case, tag)
    X, Y, noise, noise2 = PR.inputs(case, int(g("seed")))
    assert np.array_equal(PR.make_old_logp(case, w, X, noise, int(g("seed"))), g("old_logp"))
    res = PR.batch(w, case, X, Y, g("old_logp"), noise)
    assert not PR.conditions(case, res, Y)
    np.testing.assert_allclose(res["cost"], g("cost"), rtol=1e-12)
    for k in ("mu", "value", "new_logp"):
        assert rel(g(k), res[k]) < FTOL, k
    # the reward through the objectives' bar: a 1e-5 error of an objective moves the reward by at most 1e-5 * kappa (relative); not
    # below 1e-5 itself, because the golden is float32 torch: NU's log2(1 + sinr) with sinr ~ 1e-4 keeps 3 - 4 digits of the rate
    assert np.all(np.abs(g("reward") - res["reward"]) <= TOL * np.maximum(res["kappa"], 1.0) * res["reward"])
    assert abs(res["actor_loss"] - float(g("actor_loss"))) < TOL * abs(res["actor_loss"])
    assert abs(res["critic_loss"] - float(g("critic_loss"))) < TOL * res["critic_loss"]
    ref = {k: v for k, v in res["grads"].items() if k != "log_std"}
    errs = grad_errs({k: g("grad." + k) for k in ref}, ref)
    assert max(errs.values()) < TOL, errs
    p3, losses = PR.adam_steps(w, case, X, Y, g("old_logp"), noise, noise2)
    assert rel(g("step_loss"), np.array(losses)) < TOL
    assert np.array_equal(p3["log_std"], np.asarray(w["log_std"], dtype=np.float64))
    for k in p3:
        assert rel(g("adam." + k), p3[k]) < ATOL, k


@pytest.mark.parametrize("case", list(PR.CASES))
def test_agent_layout_and_seeded_init(g15, case):
    c = PR.CASES[case]
    m = build(case)
    sd = m.state_dict()
    assert list(sd) == list(g15[f"{case}.layout"]) and len(sd) == 17 and list(sd)[0] == "log_std"
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == PR.case_shapes(case)
    assert [n for n, _ in m.named_children()] == ["critic", "actor"]
    w = state(g15, case, "init")
    np.testing.assert_allclose([float(v.astype(np.float64).sum()) for v in w.values()], g15[f"{case}.init.sums"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose([float(np.abs(v.astype(np.float64)).sum()) for v in w.values()], g15[f"{case}.init.abs"], rtol=1e-9)
    # state dicts load strictly both ways, and the CPU forward of the module is the golden's
    m2 = build(case)
    m2.load_state_dict({k: torch.from_numpy(v) for k, v in state(g15, case, "trained").items()}, strict=True)
    X = PR.inputs(case, int(g15[f"{case}.trained.seed"]))[0]
    with torch.no_grad():
        value, dist = m2(torch.from_numpy(X))
    assert value.shape == (PR.ROWS, 1) and dist.mean.shape == (PR.ROWS, c["A"]) and dist.stddev.shape == (PR.ROWS, c["A"])
    assert rel(dist.mean.numpy(), g15[f"{case}.trained.mu"]) < TOL and rel(value.numpy()[:, 0], g15[f"{case}.trained.value"]) < TOL
    assert torch.equal(dist.stddev, m2.log_std.exp().expand(PR.ROWS, -1))


@pytest.mark.parametrize("name,S,A", [("ppo_co.pt", 9, 3), ("ppo_nu.pt", 6, 5)])
def test_shipped_checkpoints_load_strictly(name, S, A):
    from diffsg_amd import PPOAgent
    from diffsg_amd.ppo import ppo_desc
    sd = torch.load(os.path.join(GOLD, name), map_location="cpu")
    m = PPOAgent(S, A)
    m.load_state_dict(sd, strict=True)
    assert list(m.state_dict()) == list(sd)
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), sd.values()))
    assert sd["log_std"].shape == (1, A) and not sd["log_std"].any()
    from diffsg_amd import _lib
    assert _lib.lib().dsg_ppo_param_total(ctypes.byref(ppo_desc(S, A))) == sum(v.numel() for v in sd.values())


def test_agent_autograd_path_matches_goldens(g15):
    """The torch module with autograd on gives the reference's losses and gradients on the golden batch (CO)."""
    case, tag = "co3", "trained"
    g = lambda k: g15[f"{case}.{tag}.{k}"]      # noqa: E731
    m = build(case)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state(g15, case, tag).items()}, strict=True)
    X, Y, noise, _ = (torch.from_numpy(a) for a in PR.inputs(case, int(g("seed"))))
    value, dist = m(X)
    with torch.no_grad():
        a = noise * dist.stddev + dist.mean
    logp = dist.log_prob(a)
    assert rel(logp.detach().numpy(), g("new_logp")) < TOL
    ret = torch.from_numpy(g("reward"))[:, None] + 0.99 * 3.8
    adv = ret - value
    ratio = (logp - torch.from_numpy(g("old_logp"))).exp()
    actor_loss = -torch.min(ratio * adv, torch.clamp(ratio, 0.8, 1.2) * adv).mean()
    critic_loss = torch.nn.functional.mse_loss(value, ret)
    (actor_loss + critic_loss).backward()
    assert abs(actor_loss.item() - float(g("actor_loss"))) < TOL * abs(actor_loss.item())
    ref = {k: g("grad." + k).astype(np.float64) for k, _ in m.named_parameters() if k != "log_std"}
    errs = grad_errs({k: p.grad.numpy() for k, p in m.named_parameters()}, ref)
    assert max(errs.values()) < 1e-4, errs


@pytest.mark.parametrize("N,batch", [(70, 64), (300, 128), (7, 512)])
def test_composed_permutations_replay_the_rewrapped_loader(N, batch):
    """Three epochs of `fit`'s bookkeeping (perm and old_logp in dataset-row terms) against a literal replay of the reference's loop,
    which wraps the rows it visited, with their new log-probabilities, in a new shuffling DataLoader every epoch."""
    from diffsg_amd.mtfnn import epoch_permutation
    from diffsg_amd.ppo import compose_permutation
    X = torch.arange(N, dtype=torch.float32)[:, None] * torch.ones(1, 2)
    old0 = torch.rand(N, 1, generator=torch.Generator().manual_seed(5))
    new_of = lambda row, epoch, old: 10.0 * (epoch + 1) + row / 1000.0 + 0.5 * old      # noqa: E731  a stand-in for new_log_prob
    torch.manual_seed(21)
    loader = data.DataLoader(data.TensorDataset(X, old0), batch_size=batch, shuffle=True)
    want_rows, want_old = [], []
    for epoch in range(3):
        xs, olds, news = [], [], []
        for x, old in loader:
            xs.append(x)
            olds.append(old)
            news.append(new_of(x[:, :1], epoch, old))
        want_rows.append(torch.cat(xs)[:, 0].to(torch.int64))
        want_old.append(torch.cat(olds)[:, 0])
        loader = data.DataLoader(data.TensorDataset(torch.cat(xs), torch.cat(news)), batch_size=batch, shuffle=True)
    tail_want = torch.rand(3)
    torch.manual_seed(21)
    visited, old = None, old0.clone()
    for epoch in range(3):
        visited = compose_permutation(visited, epoch_permutation(N, batch))
        assert torch.equal(visited, want_rows[epoch])
        assert torch.equal(old[visited, 0], want_old[epoch])            # what the kernel reads: old_logp by dataset row
        old[visited] = new_of(visited[:, None].to(torch.float32), epoch, old[visited])      # ... and overwrites
    assert torch.equal(torch.rand(3), tail_want)
    assert sorted(visited.tolist()) == list(range(N))


@pytest.mark.parametrize("what,kw", [
    ("hidden width 65", dict(state_dim=9, action_dim=3, env="co", hidden=(64, 65, 32))),
    ("state width 129", dict(state_dim=129, action_dim=43, env="co")),
    ("action width 129", dict(state_dim=129, action_dim=129, env="msr")),
    ("CO state that is not 3 per node", dict(state_dim=8, action_dim=3, env="co")),
    ("NU without users", dict(state_dim=0, action_dim=2, env="nu")),
    ("unknown environment", dict(state_dim=9, action_dim=3, env=7)),
    ("no environment for a training call", dict(state_dim=9, action_dim=3, env=None)),
    ("nets larger than LDS", dict(state_dim=128, action_dim=128, env="msr", hidden=(64, 64, 64))),
])
def test_descriptor_limits_are_refused(what, kw):
    """Refused on the host, before any device call: runs without a GPU."""
    from diffsg_amd import _lib
    from diffsg_amd.ppo import ppo_desc
    d = ppo_desc(**kw)
    L = _lib.lib()
    one = ctypes.c_void_p(16)           # never dereferenced: the descriptor is refused first
    rc = L.dsg_ppo_train_epoch(ctypes.byref(d), one, one, one, one, one, one, one, one, 8, 4, 0.005, 0.9, 0.999, 1e-8, 0, one, 1, None)
    assert rc != 0, what
    msg = L.dsg_last_error().decode()
    assert "dsg_ppo_train_epoch" in msg and len(msg) > 24, msg
    assert L.dsg_ppo_loss_grad(ctypes.byref(d), one, one, one, one, one, 8, one, one, one, one, None) != 0, what
    if kw["env"] is not None:
        assert L.dsg_ppo_param_total(ctypes.byref(d)) == -1
        assert L.dsg_ppo_forward(ctypes.byref(d), one, one, one, one, 8, None) != 0


def test_param_total_of_the_shipped_sizes():
    from diffsg_amd import _lib
    from diffsg_amd.ppo import ppo_desc
    L = _lib.lib()
    for S, A, env, want in ((9, 3, "co", 4583), (6, 5, "nu", 4267), (80, 80, "msr", 16289), (3, 3, None, None)):
        got = L.dsg_ppo_param_total(ctypes.byref(ppo_desc(S, A, env)))
        assert got == sum(int(np.prod(s)) for _, s in PR.shapes(S, A)) and (want is None or got == want)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour without a GPU")
def test_compute_entry_points_raise_without_a_gpu():
    from diffsg_amd import PPOAgent
    from diffsg_amd import ppo
    agent = PPOAgent(9, 3)
    X, Y = np.zeros((4, 9), np.float32), np.zeros((4, 3), np.float32)
    cfg = dict(env="co", scaler_min=0.0, scaler_max=1.0)
    with pytest.raises(RuntimeError, match="HIP device"):
        ppo.fit(agent, X, Y, cfg, 1, log=None)
    with pytest.raises(RuntimeError, match="HIP device"):
        ppo.loss_grad(agent, X, Y, Y, Y, cfg)
    with pytest.raises(RuntimeError, match="HIP device"):
        ppo.device_forward(agent, torch.zeros(4, 9))
    with pytest.raises(RuntimeError):
        ppo.ppo_co(os.path.join(GOLD, "data", "3nodes_200samples_ood.csv"), epochs=1, log=None)
    with torch.no_grad():                           # the CPU forward is the torch module
        value, dist = agent(torch.zeros(4, 9))
    assert value.shape == (4, 1) and dist.mean.shape == (4, 3)


def test_fit_wants_the_agent_among_its_replicas():
    from diffsg_amd import PPOAgent
    from diffsg_amd.ppo import fit
    a, b = PPOAgent(9, 3), PPOAgent(9, 3)
    with pytest.raises(ValueError, match="must contain"):
        fit(a, np.zeros((4, 9), np.float32), np.zeros((4, 3), np.float32), dict(env="co"), 1, replicas=[b], log=None)
