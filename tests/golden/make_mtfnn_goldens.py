#!/usr/bin/env python3
"""Generate tests/golden/g14_mtfnn.npz from torch on the CPU and the reference's MTFNN class.

Runs ONLY where the reference checkout is present (REF below); the output is committed.  Nothing here is imported by the tests.

    python tests/golden/make_mtfnn_goldens.py

The NU net is the reference's imported class (baselines/MTFNN.py: MTFNN); the CO and MSR nets exist in the reference only inline
inside mtfnn_co / mtfnn_msr and are built here with torch.nn from the same layer list.  Cases and inputs: tests/mtfnn_ref.py.
Per case and weight state (`init`: torch.manual_seed(seed), construction, apply(init_weights), recorded as per-tensor checksums;
`trained`: mtfnn_ref.synth_state(widths, seed), std 0.3, stored):
  <case>.<state>.seed ................. the seed (the first one that meets the ReLU margin below)
  <case>.<state>.out .................. forward output on the ROWS inputs
  <case>.<state>.loss / .grad.<key> ... F.mse_loss(y, net(x)) and every gradient from autograd at batch = ROWS
  <case>.<state>.step_loss / .adam.<key>  the three losses and the parameters after three torch.optim.Adam(lr=0.005) steps over the
                                          batches mtfnn_ref.STEP_BATCHES
The generator asserts on its own inputs that in every hidden layer min|pre-activation| >= 2e-5 * max|pre-activation| (for the
recorded batch and for each Adam step's batch at that step's parameters): no ReLU sits where float32 rounding could flip it.
"""
import os
import sys
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
for p_ in (REF, HERE, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p_)
os.chdir(os.path.join(REF, "baselines"))

from ddpm_opt.diffusion import init_weights  # noqa: E402
from baselines.MTFNN import MTFNN  # noqa: E402
import mtfnn_ref as MR  # noqa: E402

torch.set_num_threads(4)


def build(case):
    widths, n_sig = MR.CASES[case]
    if case.startswith("nu"):
        return MTFNN(widths[0], widths[-1])
    layers = []
    for i in range(len(widths) - 1):
        layers.append((f"lin{i + 1}", nn.Linear(widths[i], widths[i + 1])))
        last = i + 2 == len(widths)
        layers.append((f"act{i + 1}", (nn.Sigmoid() if n_sig else nn.Softmax(dim=1)) if last else nn.ReLU()))
    return nn.Sequential(OrderedDict(layers))


def np_state(model):
    return {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}


def margin_ok(model, case, X):
    widths, n_sig = MR.CASES[case]
    return MR.relu_margin(np_state(model), widths, n_sig, X) >= MR.RELU_MARGIN


def run_state(case, model, X, Y, out, tag):
    """Forward, loss + gradients, three Adam steps; False if a ReLU margin is missed anywhere on the way."""
    widths, n_sig = MR.CASES[case]
    if not margin_ok(model, case, X):
        return False
    rec = {}
    x, y = torch.from_numpy(X), torch.from_numpy(Y)
    with torch.no_grad():
        rec["out"] = model(x.clone()).numpy()
    model.zero_grad()
    loss = F.mse_loss(y, model(x.clone()))
    loss.backward()
    rec["loss"] = np.float32(loss.item())
    for k, p in model.named_parameters():
        rec["grad." + k] = p.grad.detach().numpy().copy()
    model.zero_grad()
    opt = torch.optim.Adam(model.parameters(), lr=MR.LR)
    losses = []
    for lo, hi in MR.STEP_BATCHES:
        if not margin_ok(model, case, X[lo:hi]):
            return False
        loss = F.mse_loss(y[lo:hi], model(x[lo:hi].clone()))
        loss.backward()
        opt.step()
        opt.zero_grad()
        losses.append(loss.item())
    rec["step_loss"] = np.array(losses, dtype=np.float32)
    for k, v in np_state(model).items():
        rec["adam." + k] = v
    out.update({f"{case}.{tag}.{k}": v for k, v in rec.items()})
    return True


def main():
    out = {}
    for case, (widths, n_sig) in MR.CASES.items():
        X, Y = MR.inputs(case)
        out[f"{case}.layout"] = np.array([k for k, _ in MR.shapes(widths)])
        for seed in range(20):
            torch.manual_seed(seed)
            model = build(case)
            model.apply(init_weights)
            sd = np_state(model)
            assert [(k, tuple(v.shape)) for k, v in sd.items()] == MR.shapes(widths), case
            if run_state(case, model, X, Y, out, "init"):
                out[f"{case}.init.seed"] = np.int64(seed)
                out[f"{case}.init.sums"] = np.array([float(v.astype(np.float64).sum()) for v in sd.values()])
                out[f"{case}.init.abs"] = np.array([float(np.abs(v.astype(np.float64)).sum()) for v in sd.values()])
                break
        else:
            raise SystemExit(f"{case}: no init seed below 20 meets the ReLU margin")
        for seed in range(20):
            w = MR.synth_state(widths, seed)
            model = build(case)
            model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
            if run_state(case, model, X, Y, out, "trained"):
                out[f"{case}.trained.seed"] = np.int64(seed)
                for k, v in w.items():
                    out[f"{case}.trained.w.{k}"] = v
                break
        else:
            raise SystemExit(f"{case}: no trained-like seed below 20 meets the ReLU margin")
        for tag in ("init", "trained"):
            st = sd if tag == "init" else w
            ref_out = MR.forward(st, widths, n_sig, X)
            ref_loss, ref_g = MR.loss_grad(st, widths, n_sig, X, Y)
            d_o = np.abs(ref_out - out[f"{case}.{tag}.out"]).max()
            d_g = max(np.abs(ref_g[k] - out[f"{case}.{tag}.grad.{k}"]).max() / max(np.abs(ref_g[k]).max(), 1e-30) for k in ref_g)
            print(f"{case}.{tag}: seed {int(out[f'{case}.{tag}.seed'])}, mtfnn_ref vs torch: out {d_o:.2e}, "
                  f"loss {abs(ref_loss - float(out[f'{case}.{tag}.loss'])) / ref_loss:.2e}, worst grad tensor {d_g:.2e}")
    path = os.path.join(HERE, "g14_mtfnn.npz")
    np.savez_compressed(path, **out)
    print(f"wrote g14_mtfnn.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()
