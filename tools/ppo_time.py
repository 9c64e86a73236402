#!/usr/bin/env python3
"""Time one training epoch of the PPO baseline (CO agent: state 9, action 3, two nets 9 -> 64 -> 16 -> 32 -> {1 | 3}; 40 000 rows, batch
512: 79 Adam steps) on the same GPU in the same process after warm-up:

  fit R=1 ....... diffsg_amd.ppo.fit, one epoch: host permutation + upload + one torch.randn + ONE dsg_ppo_train_epoch launch + the
                  read-back of batch_out
  fit R=32 ...... the same with 32 replicas in the launch
  launch R=1/32 . dsg_ppo_train_epoch alone between two synchronisations (permutation, noise, old_logp already on the device)
  torch eager ... the same loop with the module under autograd on the same device: data resident, the environment step in torch
                  (vectorised over the batch), two torch.optim.Adam, one read-back per epoch

Median of REPEATS calls each.  Writes the figures and the kernels' resource usage to --out (default profiles/ppo_time.txt).

    python tools/ppo_time.py [--out FILE] [--rows 40000] [--repeats 7]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def co_cost_torch(X, Y):
    """cost_calc of the CO problem, vectorised (X raw [B][3n], Y [B][n])."""
    D = Y > 0.1
    ysum, dsum = (Y * D).sum(dim=1), D.sum(dim=1)
    spread = (1 - ysum) / torch.where(dsum == 0, 0.00001, dsum.to(Y.dtype))
    share = torch.where(D, Y + spread[:, None], torch.ones_like(Y))
    return torch.where(D, X[:, 1::3] + X[:, 2::3] / share, X[:, 0::3]).sum(dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_time.txt"))
    ap.add_argument("--rows", type=int, default=40000)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    from diffsg_amd import PPOAgent, _lib
    from diffsg_amd import ppo as P

    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    X = rs.uniform(0, 1, (a.rows, 9)).astype(np.float32)
    Y = rs.uniform(0, 1, (a.rows, 3)).astype(np.float32)
    Y /= Y.sum(axis=1, keepdims=True)
    cfg = dict(env="co", scaler_min=0.5, scaler_max=10.0)
    Xd, Yd = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)

    torch.manual_seed(0)
    res = {}
    for R in (1, 32):
        agents = [PPOAgent(9, 3).to(dev) for _ in range(R)]
        res[f"fit R={R}"] = median_ms(lambda: P.fit(agents[0], Xd, Yd, cfg, 1, batch_size=a.batch, replicas=agents, log=None), a.repeats)
        desc = P.agent_desc(agents[0], cfg)
        p = torch.stack([P.flat_params(m) for m in agents]).contiguous()
        m1, m2 = torch.zeros_like(p), torch.zeros_like(p)
        perm = torch.stack([torch.randperm(a.rows) for _ in range(R)]).to(device=dev, dtype=torch.int32)
        noise = torch.randn(R, a.rows, 3, device=dev)
        old = torch.randn(R, a.rows, 3, device=dev) * 0.1 - 1.4
        res[f"launch R={R}"] = median_ms(lambda: P.train_epoch_flat(desc, p, m1, m2, Xd, Yd, old, noise, perm, a.batch, 0.005, 0), a.repeats)

    agent = PPOAgent(9, 3).to(dev)
    actor_opt = torch.optim.Adam(agent.actor.parameters(), lr=0.005)
    critic_opt = torch.optim.Adam(agent.critic.parameters(), lr=0.005)
    old_e = torch.randn(a.rows, 3, device=dev) * 0.1 - 1.4
    lo, hi = cfg["scaler_min"], cfg["scaler_max"]

    def eager_resident():
        perm = torch.randperm(a.rows, device=dev)
        outs = []
        for b0 in range(0, a.rows, a.batch):
            idx = perm[b0:b0 + a.batch]
            x, y = Xd[idx], Yd[idx]
            values, dist = agent(x)
            actions = dist.sample()
            new_logp = dist.log_prob(actions)
            with torch.no_grad():
                act = torch.softmax(actions, dim=1)
                xr = x * (hi - lo) + lo
                rewards = 1 / (torch.abs(co_cost_torch(xr, act) - co_cost_torch(xr, y)) + 0.1)
                returns = (rewards + 0.99 * 3.8)[:, None]
            adv = returns - values
            ratio = (new_logp - old_e[idx]).exp()
            actor_loss = -torch.min(ratio * adv, torch.clamp(ratio, 0.8, 1.2) * adv).mean()
            actor_loss.backward(retain_graph=True)
            critic_loss = F.mse_loss(values, returns)
            critic_loss.backward()
            actor_opt.step()
            actor_opt.zero_grad()
            critic_opt.step()
            critic_opt.zero_grad()
            agent.log_std.grad = None
            old_e[idx] = new_logp.detach()
            outs.append(torch.stack((actor_loss.detach(), critic_loss.detach(), rewards.sum())))
        return torch.stack(outs).sum(dim=0).tolist()

    res["torch eager (module under autograd, data resident, one read-back per epoch)"] = median_ms(eager_resident, a.repeats)

    nb = (a.rows + a.batch - 1) // a.batch
    lines = [f"PPO epoch time: CO agent (state 9, action 3, hidden 64-16-32, 4 583 parameters), {a.rows} rows, batch {a.batch} ({nb} Adam steps per epoch)",
             f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; median (min .. max) of {a.repeats} calls after 2 warm-up calls, "
             "wall clock between device synchronisations, one process"]
    for k, (med, lo_, hi_) in res.items():
        lines.append(f"  {k:80s} {med:9.3f} ms  ({lo_:.3f} .. {hi_:.3f})")
    e = res["torch eager (module under autograd, data resident, one read-back per epoch)"][0]
    lines.append(f"  resident eager / fit R=1: {e / res['fit R=1'][0]:.1f}x;  per agent at R=32: {res['fit R=32'][0] / 32:.3f} ms "
                 f"({e / (res['fit R=32'][0] / 32):.0f}x the eager loop)")
    lines.append(f"  launch alone per Adam step: R=1 {res['launch R=1'][0] / nb * 1e3:.1f} us, R=32 {res['launch R=32'][0] / nb * 1e3:.1f} us")
    kr = _lib.kernel_resources()
    for n in ("dsg::k_ppo_epoch", "dsg::k_ppo_loss_grad", "dsg::k_ppo_forward"):
        r = kr[n]
        lines.append(f"  {n}: {r['vgprs']} VGPRs, {r['agprs']} AGPRs, {r['sgprs']} SGPRs, scratch {r['scratch']} B/lane, occupancy {r['occupancy']} waves/SIMD "
                     "(256 threads; dynamic LDS by agent: parameters + one tile of both nets' activations [+ gradient and moments] [+ batch buffer])")
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt)
    print(txt, end="")


if __name__ == "__main__":
    main()
