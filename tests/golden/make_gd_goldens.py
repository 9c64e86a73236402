#!/usr/bin/env python3
"""Generate tests/golden/g16_gd.npz from the reference's gradient-descent baseline (baselines/GD.py) on the CPU.

Runs ONLY where the reference checkout is present (REF below); the output is committed.  Nothing here is imported by the tests.

    python tests/golden/make_gd_goldens.py

The gradients are the reference's imported co_gradient / msr_gradient / nu_gradient, the loaders and evaluators its co_data_load /
msr_data_load / nu_data_load / cost_calc / rate_calc; the loops around them are those of co_solve / msr_solve / nu_solve with the
dataset path and the iteration count as arguments (the reference hard-codes both).

Problems and inputs (x: the condition the gradient reads, y0: the reference's start state):
  co ..... every row of data/3nodes_200samples_ood.csv through co_data_load (train then test rows), de-normalised
  msr3 ... every row of data/3c_10w_200samples.csv through msr_data_load, de-normalised, W = 10
  msr80 .. 64 rows at M = 80, W = 20: the 48 rows of g8_sum_rate_gen.npz's m80_gs, then its first 16 rows with the channel order reversed
  nu ..... every row of data/3u_18mW_200samples.csv through nu_data_load(400, 400)
Per problem:
  <p>.x, <p>.y0 ........ float64 inputs
  <p>.y<k> ............. the float64 state after k iterations, k in gd_ref.STATES
Per driver (co, msr3, nu: the first test rows of the fixture, as the reference takes them) and iterations it in (20, 100):
  drv.<p>.<it>.Y ....... the final float64 state
  drv.<p>.<it>.pred / .true ............. per-row objectives after the reference's post-processing
  drv.<p>.<it>.sum_ratio / .mean_diff ... sum(pred) / sum(true), mean(pred - true)
  drv.co.<it>.norm ..... the min-max-normalised float32 allocations cost_calc scored (the tests leave out rows within 1e-4 of its
                         0.1 decision threshold; asserted here to be at most 2 % of the rows at 20 iterations)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
for p_ in (REF, HERE, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p_)
os.chdir(os.path.join(REF, "baselines"))

from baselines.GD import co_gradient, msr_gradient, nu_gradient  # noqa: E402
from ddpm_opt.classifier_free_CO import co_data_load, cost_calc  # noqa: E402
from ddpm_opt.classifier_free_MSR import msr_data_load  # noqa: E402
from ddpm_opt.classifier_free_NU import nu_data_load, rate_calc  # noqa: E402
import gd_ref as GR  # noqa: E402

torch.set_num_threads(4)
DATA = os.path.join(HERE, "data")
CO_CSV, MSR_CSV, NU_CSV = (os.path.join(DATA, f) for f in ("3nodes_200samples_ood.csv", "3c_10w_200samples.csv", "3u_18mW_200samples.csv"))
WIDTH = HEIGHT = 400


def descend(kind, x, y0, iters, keep=()):
    """The reference's loops: Y_pred -= grad * 0.1 (CO), += grad * 0.001 (MSR), += grad * 0.1 (NU)."""
    y, kept = y0.copy(), {}
    with np.errstate(all="ignore"):
        for k in range(1, iters + 1):
            if kind == "co":
                grad = co_gradient(x, y, y.shape[1] // 2, 1.0, 1.0)
                y -= grad * 0.1
            elif kind == "msr":
                y += msr_gradient(x, y) * 0.001
            else:
                grad = nu_gradient(y, x, y.shape[1] - 2)
                y += grad * 0.1
            if k in keep:
                kept[k] = y.copy()
    return y, kept


def states(out, name, kind, x, y0):
    out[f"{name}.x"], out[f"{name}.y0"] = x, y0
    _, kept = descend(kind, x, y0, max(GR.STATES), GR.STATES)
    for k, y in kept.items():
        out[f"{name}.y{k}"] = y


def main():
    out = {}
    # ---- CO
    X_train, Y_train, X_test, Y_test, cc = co_data_load(CO_CSV)
    lo, hi = cc['scaler_min'], cc['scaler_max']
    node_num = Y_train.shape[1]
    X_all = np.concatenate((X_train, X_test)) * (hi - lo) + lo
    assert X_all.shape == (200, 3 * node_num), X_all.shape
    y0 = np.ones((X_all.shape[0], 2 * node_num))
    y0[:, -node_num:] = 1 / node_num
    states(out, "co", "co", X_all, y0)
    X_te = X_test * (hi - lo) + lo
    for it in (20, 100):
        Y_pred = np.ones((X_te.shape[0], 2 * node_num))
        Y_pred[:, -node_num:] = 1 / node_num
        Y_pred, _ = descend("co", X_te, Y_pred, it)
        X_t = torch.tensor(X_te, dtype=torch.float32)
        Y_t = torch.tensor(Y_test, dtype=torch.float32)
        Y_p = torch.tensor(Y_pred[:, -node_num:], dtype=torch.float32)
        mn, _ = torch.min(Y_p, dim=1, keepdim=True)
        mx, _ = torch.max(Y_p, dim=1, keepdim=True)
        Y_p = (Y_p - mn) / (mx - mn)
        pred, true = cost_calc(X_t, Y_p), cost_calc(X_t, Y_t)
        tag = f"drv.co.{it}"
        out[f"{tag}.Y"], out[f"{tag}.norm"] = Y_pred, Y_p.numpy()
        out[f"{tag}.pred"], out[f"{tag}.true"] = pred.numpy(), true.numpy()
        out[f"{tag}.sum_ratio"] = np.float64(torch.sum(pred) / torch.sum(true))
        out[f"{tag}.mean_diff"] = np.float64(torch.mean(pred - true))
        near = ~GR.co_far_from_threshold(Y_p.numpy())
        print(f"{tag}: {int(near.sum())} of {near.size} rows within 1e-4 of the threshold or non-finite, ratio {out[f'{tag}.sum_ratio']:.6f}")
        if it == 20:
            assert near.mean() <= 0.02, near.mean()
    out["drv.co.x"], out["drv.co.y_test"] = X_te, Y_test

    # ---- MSR, 3 channels
    X_train, Y_train, X_test, Y_test, cc = msr_data_load(MSR_CSV)
    M, W = cc['M'], cc['W']
    lo, hi = cc['scaler_min'], cc['scaler_max']
    X_all = np.concatenate((X_train, X_test)) * (hi - lo) + lo
    assert X_all.shape == (200, M)
    states(out, "msr3", "msr", X_all, np.ones_like(X_all) / M * W)
    out["msr3.W"] = np.float64(W)
    X_te = X_test * (hi - lo) + lo
    for it in (20, 100):
        Y_pred, _ = descend("msr", X_te, np.ones_like(Y_test) / M * W, it)
        tag = f"drv.msr3.{it}"
        out[f"{tag}.Y"] = Y_pred.copy()
        Y_pred_sum = np.atleast_2d(np.sum(Y_pred, axis=1)).T
        Y_pred += (W - Y_pred_sum) / M
        pred = np.sum(np.log2(1.0 + Y_pred * X_te), axis=1)
        true = np.sum(np.log2(1.0 + Y_test * X_te), axis=1)
        out[f"{tag}.pred"], out[f"{tag}.true"] = pred, true
        out[f"{tag}.sum_ratio"], out[f"{tag}.mean_diff"] = np.float64(np.sum(pred) / np.sum(true)), np.float64(np.mean(pred - true))
        print(f"{tag}: ratio {out[f'{tag}.sum_ratio']:.6f}")

    # ---- MSR, 80 channels
    gs = np.load(os.path.join(HERE, "g8_sum_rate_gen.npz"))["m80_gs"].astype(np.float64)
    gs = np.concatenate((gs, gs[:16, ::-1]))
    assert gs.shape == (64, 80)
    states(out, "msr80", "msr", gs, np.ones_like(gs) / 80 * 20.0)
    out["msr80.W"] = np.float64(20.0)

    # ---- NU
    X_train, Y_train, X_test, Y_test, R_test, cc = nu_data_load(NU_CSV, WIDTH, HEIGHT)
    K, P_sum = cc['K'], cc['P_sum']
    X_all = np.concatenate((X_train, X_test))
    assert X_all.shape == (200, 2 * K)
    y0 = np.ones((200, 2 + K)) * P_sum / K - 0.01
    y0[:, 0], y0[:, 1] = WIDTH / 2, HEIGHT / 2
    states(out, "nu", "nu", X_all, y0)
    out["nu.P_sum"] = np.float64(P_sum)
    for it in (20, 100):
        Y_pred = np.ones_like(Y_test) * P_sum / K - 0.01
        Y_pred[:, 0], Y_pred[:, 1] = WIDTH / 2, HEIGHT / 2
        Y_pred, _ = descend("nu", X_test, Y_pred, it)
        X_t = torch.tensor(X_test, dtype=torch.float32)
        for i in range(K):
            X_t[:, 2 * i] *= WIDTH
            X_t[:, 2 * i + 1] *= HEIGHT
        Y_t = torch.tensor(Y_test, dtype=torch.float32)
        Y_t[:, 0] *= WIDTH
        Y_t[:, 1] *= HEIGHT
        Y_t[:, 2:] *= P_sum
        Y_p = torch.tensor(Y_pred, dtype=torch.float32)
        Y_p_sum = torch.sum(Y_p[:, -K:], dim=1).unsqueeze(dim=1)
        Y_p[:, -K:] = Y_p[:, -K:] / Y_p_sum * P_sum
        pred, true = rate_calc(Y_p, X_t), rate_calc(Y_t, X_t)
        tag = f"drv.nu.{it}"
        out[f"{tag}.Y"] = Y_pred
        out[f"{tag}.pred"], out[f"{tag}.true"] = pred.numpy(), true.numpy()
        out[f"{tag}.sum_ratio"] = np.float64(torch.sum(pred) / torch.sum(true))
        out[f"{tag}.mean_diff"] = np.float64(torch.mean(pred - true))
        print(f"{tag}: ratio {out[f'{tag}.sum_ratio']:.6f}")

    # the restatement against what was just written, and the conditioning figures the tests assert
    for name, kind in (("co", "co"), ("msr3", "msr"), ("msr80", "msr"), ("nu", "nu")):
        _, kept = GR.run(kind, out[f"{name}.x"], out[f"{name}.y0"], 100, GR.STATES)
        same = all(np.array_equal(kept[k], out[f"{name}.y{k}"], equal_nan=True) for k in GR.STATES)
        t20, t100 = (GR.twin_dev(kind, out[f"{name}.x"], out[f"{name}.y0"], it) for it in (20, 100))
        print(f"{name}: gd_ref reproduces every state: {same}; twin deviation max at 20: {t20.max():.2e}, at 100: max {t100.max():.2e}, "
              f"share <= 1e-9: {np.mean(t100 <= 1e-9):.3f}")
    path = os.path.join(HERE, "g16_gd.npz")
    np.savez_compressed(path, **out)
    print(f"wrote g16_gd.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()
