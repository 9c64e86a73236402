"""The PPO baseline (reference: baselines/PPO.py): the actor-critic agent DiffSG is compared with, on the device.

`PPOAgent` is a plain torch module with the reference's names and registration order, so a seeded construction on the CPU gives the
reference's orthogonal initial weights and state dicts (the shipped checkpoints among them) load strictly both ways.  On a HIP device
under `torch.no_grad()` its `forward` takes value and mean from one `dsg_ppo_forward` launch (the flat parameter vector it reads is
rebuilt only after a parameter changed); on the CPU, or with autograd on, it is the torch module.  `loss_grad` is `dsg_ppo_loss_grad`,
`fit` the reference's training loop with ONE `dsg_ppo_train_epoch` launch per epoch (csrc/dsg_ppo.hpp).

Reference quirks kept and named: the advantage is not detached, so the critic is trained by the actor loss too; `log_std` is in
neither optimizer and stays at its initial zeros; `nu_env_step` builds its user positions with `zeros_like`, so every NU reward is
computed with all users at the origin; `ppo_co` SAMPLES an action at test time where `ppo_msr` / `ppo_nu` use the mean; and the
evaluation loader shuffles, so the drivers return `*_reference_order` and `*_aligned` figures as the MTFNN drivers do.

The Gaussian noise of the actions comes from torch's device generator (one `torch.randn` per epoch), not from the reference's
per-batch `Normal.sample()` on its own device: equality with a reference run from the same seed is not a goal.  Equality with the same
noise fed in is, and the tests hold `dsg_ppo_loss_grad` / `dsg_ppo_train_epoch` to it.
"""
import ctypes
from functools import partial

import numpy as np
import torch
import torch.nn as nn
from torch.distributions import Normal

from . import _lib
from . import _smallnet as _sn
from ._smallnet import epoch_lrs, epoch_permutation, flat_params  # noqa: F401  (part of this module's interface)

_cuda = partial(_sn.cuda, "ppo")
_call = _sn.call

ENVS = {"co": 0, "msr": 1, "nu": 2}
HIDDEN = (64, 16, 32)


# ---------------------------------------------------------------------------------------------------------------------
# module
# ---------------------------------------------------------------------------------------------------------------------
def layer_init(layer, std=np.sqrt(2), bias_const=0.0):
    torch.nn.init.orthogonal_(layer.weight, std)
    torch.nn.init.constant_(layer.bias, bias_const)
    return layer


class PPOAgent(nn.Module):
    """PPO.py:33-70: critic state -> 64 -> 16 -> 32 -> 1 and actor state -> 64 -> 16 -> 32 -> action, tanh between the layers, and a
    state-independent log_std."""

    def __init__(self, state_dim, action_dim):
        super().__init__()
        self.state_dim = state_dim
        self.action_dim = action_dim
        self.critic = nn.Sequential(
            layer_init(nn.Linear(state_dim, 64)), nn.Tanh(),
            layer_init(nn.Linear(64, 16)), nn.Tanh(),
            layer_init(nn.Linear(16, 32)), nn.Tanh(),
            layer_init(nn.Linear(32, 1), std=1.0),
        )
        self.actor = nn.Sequential(
            layer_init(nn.Linear(state_dim, 64)), nn.Tanh(),
            layer_init(nn.Linear(64, 16)), nn.Tanh(),
            layer_init(nn.Linear(16, 32)), nn.Tanh(),
            layer_init(nn.Linear(32, action_dim), std=0.01),
        )
        self.log_std = nn.Parameter(torch.zeros(1, action_dim))

    def forward(self, state):
        """(value [rows][1], Normal(mu, std))."""
        if state.is_cuda and not torch.is_grad_enabled() and self.log_std.device == state.device:
            mu, value = device_forward(self, state)
            value = value[:, None]
        else:
            value = self.critic(state)
            mu = self.actor(state)
        std = self.log_std.exp()
        return value, Normal(mu, std)


# ---------------------------------------------------------------------------------------------------------------------
# the library's view of an agent
# ---------------------------------------------------------------------------------------------------------------------
def ppo_desc(state_dim, action_dim, env=None, env_config=None, hidden=HIDDEN):
    """ctypes descriptor.  env: "co" | "msr" | "nu", or None for inference alone (dsg_ppo_forward); env_config: the data loaders'
    custom_config (scaler_min / scaler_max [/ W] or width / height / P_sum).  Not validated here: the library refuses."""
    d = _lib.PpoDesc()
    d.state_dim, d.action_dim = int(state_dim), int(action_dim)
    for i, w in enumerate(list(hidden)[:3]):
        d.hidden[i] = int(w)
    d.env = -1 if env is None else (ENVS[env] if env in ENVS else int(env))
    cfg = env_config or {}
    for k in ("scaler_min", "scaler_max", "W", "width", "height", "P_sum"):
        setattr(d, k, float(cfg.get(k, 0.0)))
    return d


def agent_desc(agent, env_config=None):
    hidden = [m.out_features for m in agent.actor if isinstance(m, nn.Linear)][:3]
    return ppo_desc(agent.state_dim, agent.action_dim, (env_config or {}).get("env"), env_config, hidden)


def forward_flat(desc, params, x):
    """dsg_ppo_forward on a flat parameter vector: (mu [rows][A], value [rows])."""
    mu = torch.empty((x.shape[0], desc.action_dim), device=x.device, dtype=torch.float32)
    value = torch.empty((x.shape[0],), device=x.device, dtype=torch.float32)
    _call("dsg_ppo_forward", x.device, ctypes.byref(desc), _lib.ptr(params), _lib.ptr(x), _lib.ptr(mu), _lib.ptr(value), x.shape[0])
    return mu, value


def device_forward(agent, x):
    x = _cuda(x, x.device, "forward")
    desc, flat = _sn.cached_flat(agent, agent_desc)
    if x.shape[1] != desc.state_dim:
        raise ValueError(f"forward: x has {x.shape[1]} columns, the agent {desc.state_dim} state inputs")
    return forward_flat(desc, flat, x)


def loss_grad_flat(desc, params, x, y, old_logp, noise):
    """dsg_ppo_loss_grad on a flat parameter vector: (out3 = [actor loss, critic loss, sum of rewards], new_logp [rows][A],
    reward [rows], flat gradient with zeros in the log_std slots)."""
    rows, A = x.shape[0], desc.action_dim
    out3 = torch.zeros(3, device=x.device, dtype=torch.float32)
    new_logp = torch.zeros((rows, A), device=x.device, dtype=torch.float32)
    reward = torch.zeros(rows, device=x.device, dtype=torch.float32)
    grad = torch.zeros_like(params)
    _call("dsg_ppo_loss_grad", x.device, ctypes.byref(desc), _lib.ptr(params), _lib.ptr(x), _lib.ptr(y), _lib.ptr(old_logp), _lib.ptr(noise),
          rows, _lib.ptr(out3), _lib.ptr(new_logp), _lib.ptr(reward), _lib.ptr(grad))
    return out3, new_logp, reward, grad


def loss_grad(agent, x, y, old_logp, noise, env_config):
    """(out3, new_logp, reward, {parameter name: gradient}) of one batch of PPO.py:140-154 with the given noise, from
    dsg_ppo_loss_grad.  The gradient is that of actor_loss + critic_loss; log_std's is not computed (zeros)."""
    dev = agent.log_std.device
    x, y, old_logp, noise = (_cuda(t, dev, "loss_grad") for t in (x, y, old_logp, noise))
    desc = agent_desc(agent, env_config)
    A = desc.action_dim
    if x.shape[1] != desc.state_dim or any(t.shape != (x.shape[0], A) for t in (y, old_logp, noise)):
        raise ValueError(f"loss_grad: x {tuple(x.shape)} / y {tuple(y.shape)} / old_logp {tuple(old_logp.shape)} / noise "
                         f"{tuple(noise.shape)} do not fit the agent")
    out3, new_logp, reward, flat = loss_grad_flat(desc, flat_params(agent), x, y, old_logp, noise)
    return out3, new_logp, reward, _sn.named_grads(agent, flat)


# ---------------------------------------------------------------------------------------------------------------------
# training
# ---------------------------------------------------------------------------------------------------------------------
def train_epoch_flat(desc, params, exp_avg, exp_avg_sq, X, Y, old_logp, noise, perm, batch, lr, step0, betas=(0.9, 0.999), eps=1e-8):
    """dsg_ppo_train_epoch on flat [R][P] tensors (updated in place); old_logp [R][N][A] by dataset row (overwritten with this epoch's
    new_logp), noise [R][N][A] by position, perm int32 [R][N].  Returns batch_out [R][ceil(N / batch)][3]."""
    R, N = perm.shape
    nb = (N + batch - 1) // batch
    batch_out = torch.zeros((R, nb, 3), device=X.device, dtype=torch.float32)
    _call("dsg_ppo_train_epoch", X.device, ctypes.byref(desc), _lib.ptr(params), _lib.ptr(exp_avg), _lib.ptr(exp_avg_sq), _lib.ptr(X),
          _lib.ptr(Y), _lib.ptr(old_logp), _lib.ptr(noise), _lib.ptr(perm), N, batch, float(lr), betas[0], betas[1], eps, step0,
          _lib.ptr(batch_out), R)
    return batch_out


def compose_permutation(visited, perm):
    """The reference re-wraps the rows it visited in a new DataLoader every epoch (PPO.py:166-175): the permutation of epoch e indexes
    the visiting order of epoch e - 1.  `visited`: that order in dataset rows (None before the first epoch); returns this epoch's."""
    return perm if visited is None else visited[perm]


def fit(agent, X, Y, env_config, epochs, batch_size=512, lr=0.005, milestones=(20,), replicas=None, log=print):
    """The reference's training loop (PPO.py:118-180) on the device: two Adam optimizers with identical hyper-parameters (here one
    sweep over the critic and actor range), MultiStepLR(gamma=0.1), one launch per epoch.  env_config: the data loader's custom_config
    plus "env": "co" | "msr" | "nu".  X, Y (arrays or tensors) are uploaded once.  `replicas`: the list of agents trained side by side
    in the same launches (`agent` among them), each with old log-probabilities, permutations and noise of its own.  Per epoch: the
    permutations (epoch_permutation, composed with the previous epoch's visiting order, so that `perm` and `old_logp` are in
    dataset-row terms), one torch.randn on the device, one launch, one read-back.  Returns the per-epoch log values,
    [epochs][R] of (actor loss, critic loss, reward): the reference's sums of batch means over the row count, and reward per row."""
    dev = agent.log_std.device
    agents = _sn.replica_list("ppo", "agent", agent, replicas, dev, partial(agent_desc, env_config=env_config))
    desc = agent_desc(agent, env_config)
    X, Y = _cuda(X, dev, "fit"), _cuda(Y, dev, "fit")
    N, A, R = X.shape[0], desc.action_dim, len(agents)
    if X.shape[1] != desc.state_dim or Y.shape != (N, A):
        raise ValueError(f"fit: X {tuple(X.shape)} / Y {tuple(Y.shape)} do not fit the agent")
    params = torch.stack([flat_params(a).to(dev) for a in agents]).contiguous()
    exp_avg, exp_avg_sq = torch.zeros_like(params), torch.zeros_like(params)
    with torch.no_grad():                           # PPO.py:126-130
        dist = Normal(0.5 * torch.ones((R, N, A), device=dev), 0.2 * torch.ones((R, N, A), device=dev))
        old_logp = dist.log_prob(dist.sample()).contiguous()
    nb = (N + batch_size - 1) // batch_size
    visited = [None] * R
    history = []
    for epoch, cur_lr in enumerate(epoch_lrs(lr, milestones, epochs)):
        visited = [compose_permutation(v, epoch_permutation(N, batch_size)) for v in visited]
        perm = torch.stack(visited).to(device=dev, dtype=torch.int32)
        noise = torch.randn((R, N, A), device=dev, dtype=torch.float32)
        bo = train_epoch_flat(desc, params, exp_avg, exp_avg_sq, X, Y, old_logp, noise, perm, batch_size, cur_lr, epoch * nb).cpu()
        # per replica the running sums of actor loss, critic loss and reward over the batches
        vals = [tuple(_sn.running_sum(col) / N for col in zip(*rows)) if N else (0.0, 0.0, 0.0) for rows in bo.tolist()]
        history.append(vals)
        if log is not None:
            log(f"Epoch: {epoch}, Actor loss: {vals[0][0]}, Critic loss: {vals[0][1]}.")
            log(f"Reward: {vals[0][2]}")
    for a, p in zip(agents, params):
        _sn.unflatten_into(a, p)
    return history


# ---------------------------------------------------------------------------------------------------------------------
# drivers
# ---------------------------------------------------------------------------------------------------------------------
def _actions(agent, X_test, sample):
    with torch.no_grad():
        _, dist = agent(X_test)
        return dist.sample() if sample else dist.mean


def _orders(n, batch_size, dev):
    """Row batches of the two evaluation orders: row for row, and as the reference's shuffling evaluation loader visits them."""
    perm = epoch_permutation(n, batch_size).to(dev)
    return torch.arange(n, device=dev).split(batch_size), perm.split(batch_size)


def _train(agent, X_train, Y_train, cfg, epochs, batch_size, lr, milestones, replicas, log):
    return {"history": fit(agent, X_train, Y_train, cfg, epochs, batch_size, lr, milestones, [agent] + list(replicas) if replicas else None, log)}


def ppo_co(dataset_path, epochs=200, batch_size=512, lr=0.005, milestones=(20, 100), replicas=None, save_path=None, log=print):
    """ppo_co, PPO.py:102-213; the test-time action is SAMPLED, as there.  Returns (agent, {"sum_ratio_*": the reference's "exceeded
    ratio", "mean_diff_*": its "avg cost diff"}); `replicas`: further agents to train beside it (fit)."""
    from . import decode
    from .classifier_free_CO import co_data_load
    X_train, Y_train, X_test, Y_test, custom_config = co_data_load(dataset_path)
    dev = _sn.device()
    node_num = Y_train.shape[1]
    agent = PPOAgent(node_num * 3, node_num).to(dev)
    out = _train(agent, X_train, Y_train, dict(custom_config, env="co"), epochs, batch_size, lr, milestones, replicas, log)
    X_t, Y_t = _cuda(X_test, dev, "ppo_co"), _cuda(Y_test, dev, "ppo_co")
    aligned = torch.softmax(_actions(agent, X_t, True), dim=1)
    _, ref_batches = _orders(X_t.shape[0], batch_size, dev)
    ref_order = aligned[torch.cat(ref_batches)]
    lo, hi = custom_config['scaler_min'], custom_config['scaler_max']
    X_raw = X_t * (hi - lo) + lo
    true_cost = decode.co_cost(X_raw, Y_t)
    _sn.figures(decode.co_cost(X_raw, ref_order), true_cost, "reference_order", out)
    _sn.figures(decode.co_cost(X_raw, aligned), true_cost, "aligned", out)
    return _sn.finish(agent, out, save_path, log)


def ppo_msr(dataset_path, epochs=100, batch_size=512, lr=0.005, milestones=(20,), replicas=None, save_path=None, log=print):
    """ppo_msr, PPO.py:230-344: trained on Y / W, the mean action softmaxed and scaled back by W.  Returns (agent, {"sum_ratio_*": the
    reference's "less ratio", "mean_diff_*": its "avg rate diff"})."""
    from . import decode
    from .classifier_free_MSR import msr_data_load
    X_train, Y_train, X_test, Y_test, custom_config = msr_data_load(dataset_path)
    M, W = custom_config['M'], custom_config['W']
    Y_train /= W
    dev = _sn.device()
    agent = PPOAgent(M, M).to(dev)
    out = _train(agent, X_train, Y_train, dict(custom_config, env="msr"), epochs, batch_size, lr, milestones, replicas, log)
    X_t, Y_t = _cuda(X_test, dev, "ppo_msr"), _cuda(Y_test, dev, "ppo_msr")
    aligned = torch.softmax(_actions(agent, X_t, False), dim=1) * W
    _, ref_batches = _orders(X_t.shape[0], batch_size, dev)
    ref_order = aligned[torch.cat(ref_batches)]
    lo, hi = custom_config['scaler_min'], custom_config['scaler_max']
    X_raw = X_t * (hi - lo) + lo
    true_rate = decode.msr_rate(Y_t, X_raw)
    _sn.figures(decode.msr_rate(ref_order, X_raw), true_rate, "reference_order", out)
    _sn.figures(decode.msr_rate(aligned, X_raw), true_rate, "aligned", out)
    return _sn.finish(agent, out, save_path, log)


def ppo_nu(dataset_path, epochs=50, width=400, height=400, batch_size=512, lr=0.005, milestones=(20,), replicas=None, save_path=None,
           log=print):
    """ppo_nu, PPO.py:363-484: targets scaled by (width, height, P_sum); the mean action goes through custom_decoder batch by batch
    (its min-max is per evaluation batch, as in the reference's loop).  Returns (agent, {"sum_ratio_*": the reference's "less
    ratio", "mean_diff_*": its "avg rate diff"})."""
    from . import decode
    from .classifier_free_NU import nu_data_load
    X_train, Y_train, X_test, Y_test, _, custom_config = nu_data_load(dataset_path, width, height)
    Y_train[:, 0] *= width
    Y_train[:, 1] *= height
    K, P_sum = custom_config['K'], custom_config['P_sum']
    Y_train[:, -K:] *= P_sum
    dev = _sn.device()
    agent = PPOAgent(K * 2, K + 2).to(dev)
    cfg = dict(custom_config, env="nu", width=width, height=height)
    out = _train(agent, X_train, Y_train, cfg, epochs, batch_size, lr, milestones, replicas, log)
    X_t, Y_t = _cuda(X_test, dev, "ppo_nu"), _cuda(Y_test, dev, "ppo_nu")
    mean = _actions(agent, X_t, False)
    xs = torch.tensor([width, height] * K, device=dev, dtype=torch.float32)
    ys = torch.tensor([width, height] + [P_sum] * K, device=dev, dtype=torch.float32)
    X_raw = X_t * xs
    true_rate = decode.nu_rate(Y_t * ys, X_raw)
    for tag, batches in zip(("aligned", "reference_order"), _orders(X_t.shape[0], batch_size, dev)):
        pred = torch.cat([decode.nu_decode(mean[idx].contiguous(), width, height, P_sum) for idx in batches])
        _sn.figures(decode.nu_rate(pred, X_raw), true_rate, tag, out)
    return _sn.finish(agent, out, save_path, log)
