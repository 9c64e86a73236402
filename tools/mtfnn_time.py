#!/usr/bin/env python3
"""Time one training epoch of the MTFNN baseline (CO net 9 -> 32 -> 64 -> 16 -> 3, 40 000 rows, batch 512: 79 Adam steps) three ways,
on the same GPU in the same process after warm-up:

  fit R=1 ....... diffsg_amd.mtfnn.fit, one epoch: host permutation + upload + ONE dsg_mlp_train_epoch launch + the loss read-back
  fit R=32 ...... the same with 32 replicas in the launch
  torch eager ... the reference's loop (MTFNN.py:57-73): DataLoader over CPU tensors, forward, mse_loss, backward, Adam.step per batch

and, beside them, the launch alone (dsg_mlp_train_epoch between two synchronisations, permutation already on the device) and the
eager loop on tensors that already live on the device.  Median of REPEATS calls each.  Writes the figures and the kernels' resource
usage to --out (default profiles/mtfnn_time.txt).

    python tools/mtfnn_time.py [--out FILE] [--rows 40000] [--repeats 7]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F
import torch.utils.data as data

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mtfnn_time.txt"))
    ap.add_argument("--rows", type=int, default=40000)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    from diffsg_amd import _lib, co_net, init_weights
    from diffsg_amd import mtfnn as M

    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    X = rs.uniform(0, 1, (a.rows, 9)).astype(np.float32)
    Y = (1.0 / (1.0 + np.exp(-(X @ rs.standard_normal((9, 3)))))).astype(np.float32)
    Xd, Yd = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)

    def make():
        m = co_net(9, 3)
        m.apply(init_weights)
        return m.to(dev)

    torch.manual_seed(0)
    lines = []
    res = {}
    for R in (1, 32):
        models = [make() for _ in range(R)]
        res[f"fit R={R}"] = median_ms(lambda: M.fit(models[0], Xd, Yd, 1, batch_size=a.batch, replicas=models, log=None), a.repeats)
        desc = M.model_desc(models[0])
        p = torch.stack([M.flat_params(m) for m in models]).contiguous()
        m1, m2 = torch.zeros_like(p), torch.zeros_like(p)
        perm = torch.stack([torch.randperm(a.rows) for _ in range(R)]).to(device=dev, dtype=torch.int32)
        res[f"launch R={R}"] = median_ms(lambda: M.train_epoch_flat(desc, p, m1, m2, Xd, Yd, perm, a.batch, 0.005, 0), a.repeats)

    model = make()
    opt = torch.optim.Adam(model.parameters(), lr=0.005)
    loader = data.DataLoader(data.TensorDataset(torch.from_numpy(X), torch.from_numpy(Y)), batch_size=a.batch, shuffle=True)

    def eager_reference():
        epoch_loss = 0
        for x, y in loader:
            x, y = x.to(dev), y.to(dev)
            loss = F.mse_loss(y, model(x))
            loss.backward()
            opt.step()
            opt.zero_grad()
            epoch_loss += loss.item()
        return epoch_loss

    def eager_resident():
        perm = torch.randperm(a.rows, device=dev)
        losses = []
        for lo in range(0, a.rows, a.batch):
            idx = perm[lo:lo + a.batch]
            loss = F.mse_loss(Yd[idx], model(Xd[idx]))
            loss.backward()
            opt.step()
            opt.zero_grad()
            losses.append(loss.detach())
        return float(torch.stack(losses).sum())

    res["torch eager (reference loop: CPU DataLoader, loss.item() per step)"] = median_ms(eager_reference, a.repeats)
    res["torch eager (data resident on the device, one read-back per epoch)"] = median_ms(eager_resident, a.repeats)

    nb = (a.rows + a.batch - 1) // a.batch
    lines.append(f"MTFNN epoch time: CO net 9-32-64-16-3, {a.rows} rows, batch {a.batch} ({nb} Adam steps per epoch)")
    lines.append(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; median (min .. max) of {a.repeats} calls after 2 warm-up calls, "
                 "wall clock between device synchronisations, one process")
    for k, (med, lo, hi) in res.items():
        lines.append(f"  {k:72s} {med:9.3f} ms  ({lo:.3f} .. {hi:.3f})")
    e = res["torch eager (reference loop: CPU DataLoader, loss.item() per step)"][0]
    e2 = res["torch eager (data resident on the device, one read-back per epoch)"][0]
    lines.append(f"  eager reference loop / fit R=1: {e / res['fit R=1'][0]:.1f}x;  resident eager / fit R=1: {e2 / res['fit R=1'][0]:.1f}x;  "
                 f"per model at R=32: {res['fit R=32'][0] / 32:.3f} ms ({e / (res['fit R=32'][0] / 32):.0f}x the reference loop)")
    lines.append(f"  launch alone per Adam step: R=1 {res['launch R=1'][0] / nb * 1e3:.1f} us, R=32 {res['launch R=32'][0] / nb * 1e3:.1f} us")
    kr = _lib.kernel_resources()
    for n in ("dsg::k_mlp_epoch", "dsg::k_mlp_loss_grad", "dsg::k_mlp_forward"):
        r = kr[n]
        lines.append(f"  {n}: {r['vgprs']} VGPRs, {r['agprs']} AGPRs, {r['sgprs']} SGPRs, scratch {r['scratch']} B/lane, occupancy {r['occupancy']} waves/SIMD "
                     "(256 threads; dynamic LDS by net: parameters + one 64-row tile of every layer's activations [+ gradient and moments])")
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt)
    print(txt, end="")


if __name__ == "__main__":
    main()
