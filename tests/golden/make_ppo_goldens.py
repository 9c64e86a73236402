#!/usr/bin/env python3
"""Generate tests/golden/g15_ppo.npz from torch on the CPU and the reference's PPO classes, and copy the two shipped checkpoints the
tests load (ppo_co.pt, ppo_nu.pt) beside it.

Runs ONLY where the reference checkout is present (REF below); the output is committed.  Nothing here is imported by the tests.

    python tests/golden/make_ppo_goldens.py

From the reference come PPOAgent, calc_advantage, clipped_surrogate_objective_loss and the three *_env_step (baselines/PPO.py); the
batch below is the body of its training loop (PPO.py:140-159) with the Gaussian noise injected: actions = noise * std + mu under
no_grad, which is what Normal(mu, std).sample() computes.  Cases and inputs: tests/ppo_ref.py.
Per case and weight state (`init`: torch.manual_seed(seed), construction, recorded as per-tensor checksums; `trained`:
ppo_ref.synth_state(case, seed), stored):
  <case>.<state>.seed ................... the first seed below 20 that meets the conditions below (it seeds the weights AND the
                                          inputs: ppo_ref.inputs(case, seed))
  <case>.<state>.old_logp ............... ppo_ref.make_old_logp of that state (an input)
  <case>.<state>.mu / value / new_logp / reward ... of the ROWS inputs as one batch
  <case>.<state>.cost / gt .............. the objectives of action and target (ppo_ref, float64; the reward test's kappa comes from them)
  <case>.<state>.actor_loss / critic_loss / grad.<key> ... after actor_loss.backward(retain_graph=True); critic_loss.backward()
  <case>.<state>.step_loss / adam.<key> . the three (actor, critic) losses and the parameters after three steps of two
                                          torch.optim.Adam(lr=0.005) over ppo_ref.STEP_BATCHES (see ppo_ref.adam_steps)
  <case>.<state>.step_kappa ............. the largest kappa of each step's batch
The generator asserts on its own cases, for the recorded batch and for each Adam step's batch: (a) no ratio within 1e-4 of 0.8 or 1.2,
(b) CO: no softmaxed action or target within 1e-4 of the 0.1 offload threshold, (c) kappa = (|c| + |gt|) / (|c - gt| + offset) <= 10 on
every row, (d) NU: the reference's argsort of the (equal) gains is the stable order 0, 1, 2 ...
"""
import os
import shutil
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
for p_ in (REF, HERE, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p_)
os.chdir(os.path.join(REF, "baselines"))

from baselines.PPO import (PPOAgent, calc_advantage, clipped_surrogate_objective_loss, co_env_step, msr_env_step,  # noqa: E402
                           nu_env_step)
from ddpm_opt.classifier_free_NU import custom_decoder  # noqa: E402
import ppo_ref as PR  # noqa: E402

torch.set_num_threads(4)
ENV_STEP = {"co": co_env_step, "msr": msr_env_step, "nu": nu_env_step}


def np_state(model):
    return {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}


def torch_batch(agent, case, x, y, old_logp, noise):
    """PPO.py:140-154 with the noise injected; returns (values, mu, new_log_prob, rewards, actor_loss, critic_loss), graph attached."""
    c = PR.CASES[case]
    cfg = c["cfg"]
    values, dist = agent(x)
    with torch.no_grad():
        actions = noise * dist.scale + dist.loc
    new_log_prob = dist.log_prob(actions)
    actions = torch.softmax(actions, dim=1)
    if c["env"] == "nu":
        actions = custom_decoder(actions, cfg["width"], cfg["height"], cfg["P_sum"])
    _, rewards = ENV_STEP[c["env"]](x, actions, y, cfg)
    advantages, returns = calc_advantage(rewards, values)
    ratio = (new_log_prob - old_logp).exp()
    actor_loss = clipped_surrogate_objective_loss(ratio, advantages)
    critic_loss = F.mse_loss(values, returns)
    return values, dist.loc, new_log_prob, rewards, actor_loss, critic_loss


def nu_order_ok(case, res):
    """(d): the reference sorts -h with torch.argsort; with every user at the origin the gains are equal."""
    if PR.CASES[case]["env"] != "nu":
        return True
    cfg = PR.CASES[case]["cfg"]
    act = torch.from_numpy(res["act"].astype(np.float32))
    dec = custom_decoder(act, cfg["width"], cfg["height"], cfg["P_sum"])
    K = act.shape[1] - 2
    for i in range(act.shape[0]):
        h = torch.sqrt(60 / (150 ** 2 + (0 - dec[i, 0]) ** 2 + (0 - dec[i, 1]) ** 2)) * torch.ones(K)
        if torch.argsort(-h).tolist() != list(range(K)):
            return False
    return True


def run_state(case, agent, out, tag, seed):
    """Forward, losses + gradients, three Adam steps; False if a condition is missed anywhere on the way."""
    X, Y, noise, noise2 = PR.inputs(case, seed)
    st = np_state(agent)
    old = PR.make_old_logp(case, st, X, noise, seed)
    ref = PR.batch(st, case, X, Y, old, noise)
    if PR.conditions(case, ref, Y) or not nu_order_ok(case, ref):
        return False
    rec = {"old_logp": old, "cost": ref["cost"], "gt": ref["gt"]}
    x, y, nz, nz2 = (torch.from_numpy(a) for a in (X, Y, noise, noise2))
    agent.zero_grad()
    values, mu, logp, rewards, a_loss, c_loss = torch_batch(agent, case, x, y, torch.from_numpy(old), nz)
    a_loss.backward(retain_graph=True)
    c_loss.backward()
    rec.update(mu=mu.detach().numpy(), value=values.detach().numpy()[:, 0], new_logp=logp.detach().numpy(), reward=rewards.numpy(),
               actor_loss=np.float32(a_loss.item()), critic_loss=np.float32(c_loss.item()))
    for k, p in agent.named_parameters():
        rec["grad." + k] = p.grad.detach().numpy().copy()
    agent.zero_grad()
    actor_opt = torch.optim.Adam(agent.actor.parameters(), lr=PR.LR)
    critic_opt = torch.optim.Adam(agent.critic.parameters(), lr=PR.LR)
    cur, nxt = torch.from_numpy(old).clone(), torch.from_numpy(old).clone()
    losses, kappas = [], []
    for t, (lo, hi) in enumerate(PR.STEP_BATCHES, start=1):
        if t == 3:
            cur = nxt
        n = (nz if t < 3 else nz2)[lo:hi]
        chk = PR.batch(np_state(agent), case, X[lo:hi], Y[lo:hi], cur[lo:hi].numpy(), n.numpy())
        if PR.conditions(case, chk, Y[lo:hi]) or not nu_order_ok(case, chk):
            return False
        kappas.append(chk["kappa"].max())
        _, _, logp, _, a_loss, c_loss = torch_batch(agent, case, x[lo:hi], y[lo:hi], cur[lo:hi], n)
        a_loss.backward(retain_graph=True)
        c_loss.backward()
        actor_opt.step()
        actor_opt.zero_grad()
        critic_opt.step()
        critic_opt.zero_grad()
        agent.zero_grad()                           # log_std collects a gradient that no optimizer owns
        nxt = nxt.clone()
        nxt[lo:hi] = logp.detach()
        losses.append((a_loss.item(), c_loss.item()))
    rec["step_loss"] = np.array(losses, dtype=np.float32)
    rec["step_kappa"] = np.array(kappas)
    for k, v in np_state(agent).items():
        rec["adam." + k] = v
    rec["seed"] = np.int64(seed)
    out.update({f"{case}.{tag}.{k}": v for k, v in rec.items()})
    return True


def report(case, tag, st, out):
    g = lambda k: out[f"{case}.{tag}.{k}"]      # noqa: E731
    X, Y, noise, noise2 = PR.inputs(case, int(g("seed")))
    ref = PR.batch(st, case, X, Y, g("old_logp"), noise)
    rel = lambda a, b: float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(np.abs(b).max(), 1e-30))      # noqa: E731
    gmax = max(np.abs(v).max() for v in ref["grads"].values())
    d_g = max(np.abs(ref["grads"][k] - g("grad." + k)).max() / max(np.abs(ref["grads"][k]).max(), 1e-3 * gmax) for k in ref["grads"] if k != "log_std")
    p3, losses = PR.adam_steps(st, case, X, Y, g("old_logp"), noise, noise2)
    d_p = max(rel(g("adam." + k), p3[k]) for k in p3)
    print(f"{case}.{tag}: seed {int(g('seed'))}, kappa max {ref['kappa'].max():.2f} (steps {g('step_kappa').max():.2f}), ppo_ref vs torch: "
          f"mu {rel(g('mu'), ref['mu']):.1e}, value {rel(g('value'), ref['value']):.1e}, new_logp {rel(g('new_logp'), ref['new_logp']):.1e}, "
          f"reward {rel(g('reward'), ref['reward']):.1e}, actor loss {abs(ref['actor_loss'] - g('actor_loss')) / abs(ref['actor_loss']):.1e}, "
          f"critic loss {abs(ref['critic_loss'] - g('critic_loss')) / ref['critic_loss']:.1e}, worst grad tensor {d_g:.1e}, "
          f"step losses {rel(g('step_loss'), np.array(losses)):.1e}, adam x3 {d_p:.1e}")


def main():
    out = {}
    for case, c in PR.CASES.items():
        out[f"{case}.layout"] = np.array([k for k, _ in PR.case_shapes(case)])
        states = {}
        for seed in range(20):
            torch.manual_seed(seed)
            agent = PPOAgent(c["S"], c["A"])
            sd = np_state(agent)
            assert [(k, tuple(v.shape)) for k, v in sd.items()] == PR.case_shapes(case), case
            if run_state(case, agent, out, "init", seed):
                out[f"{case}.init.sums"] = np.array([float(v.astype(np.float64).sum()) for v in sd.values()])
                out[f"{case}.init.abs"] = np.array([float(np.abs(v.astype(np.float64)).sum()) for v in sd.values()])
                states["init"] = sd
                break
        else:
            raise SystemExit(f"{case}: no init seed below 20 meets the conditions")
        for seed in range(20):
            w = PR.synth_state(case, seed)
            agent = PPOAgent(c["S"], c["A"])
            agent.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
            if run_state(case, agent, out, "trained", seed):
                for k, v in w.items():
                    out[f"{case}.trained.w.{k}"] = v
                states["trained"] = w
                break
        else:
            raise SystemExit(f"{case}: no trained-like seed below 20 meets the conditions")
        for tag in ("init", "trained"):
            report(case, tag, states[tag], out)
    path = os.path.join(HERE, "g15_ppo.npz")
    np.savez_compressed(path, **out)
    print(f"wrote g15_ppo.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")
    for name in ("ppo_co.pt", "ppo_nu.pt"):
        shutil.copyfile(os.path.join(REF, "ckpts", name), os.path.join(HERE, name))
        sd = torch.load(os.path.join(HERE, name), map_location="cpu")
        assert len(sd) == 17 and list(sd)[0] == "log_std", name
        print(f"copied {name}: {os.path.getsize(os.path.join(HERE, name)) / 1024:.1f} KiB, log_std {tuple(sd['log_std'].shape)}, "
              f"|log_std| max {float(sd['log_std'].abs().max())}")


if __name__ == "__main__":
    main()
