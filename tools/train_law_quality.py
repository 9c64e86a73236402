#!/usr/bin/env python3
"""The fine-tuning table of DESIGN.md 17 on the device: python tools/train_law_quality.py [out.txt]
Does training on the timesteps a K-step plan visits recover the quality K-step sampling loses?  The shipped NU
checkpoint (tests/golden/g4_sample_nu_ckpt.npz, T = 20) is fine-tuned for a few epochs on rows of `labelgen.noma_uav_gen` under four
timestep laws -- uniform (the reference's rule), on_plan(strided K = 5), on_plan(strided K = 7), min_snr(gamma = 5) -- every arm from
the same weights, with the same data, shuffling and device-draw seed, through the captured step graph (run_epochs(graph=True)).  Each
arm is scored by the less ratio of the checkpoint's 512 test rows under K = 5, K = 7 and all 20 steps (omega = 500, mean of four Philox
seeds), and by the loss per timestep (one uniform pass over the training rows, loss report on) before and after.  No pass mark: the table
is what it is.  Writes it to `out.txt` (default profiles/train_law_quality.txt) and prints it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

ROWS, BATCH, EPOCHS, LR, SEED = 4096, 512, 5, 2e-4, 7
OMEGA, SEEDS, KS = 500.0, (101, 102, 103, 104), (5, 7, 20)


def main():
    from oracle import ddpm_oracle as O
    from weights import CONFIGS
    from diffsg_amd import UNet1D, decode, labelgen, steps, timesteps as TS, train as tr
    from diffsg_amd import classifier_free_NU as NU
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "train_law_quality.txt")
    g = np.load(os.path.join(ROOT, "tests", "golden", "g4_sample_nu_ckpt.npz"))
    T, P = int(g["T"]), float(g["P_sum"])
    cfg = CONFIGS["nu3"]
    D = cfg["input_dim"]
    dev = torch.device("cuda:0")
    weights = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w.")}

    def fresh():
        m = UNet1D(**cfg, is_attn=(False,) * len(cfg["dims"]))
        m.load_state_dict(weights, strict=True)
        return NU.DDPM(T, m.to(dev), D - 2, P, 1.0 - O.cosine_betas(T), dev, (1, D), {"width": 400, "height": 400}).to(dev)

    # training rows: users (6) | UAV x, y | powers (3) | rate, scaled as nu_data_load scales them
    np.random.seed(SEED)
    data = labelgen.noma_uav_gen(ROWS, P, log=lambda *_: None)
    data = data[data.any(axis=1)]
    X, Y = data[:, :6].copy(), data[:, 6:11].copy()
    X /= 400.0
    Y[:, :2] /= 400.0
    Y[:, 2:] /= P
    X, Y = torch.tensor(X, dtype=torch.float32), torch.tensor(Y, dtype=torch.float32)

    cond = torch.from_numpy(g["cond"]).to(dev)
    Xs = cond.clone(); Xs[:, 0::2] *= 400; Xs[:, 1::2] *= 400
    Yt = torch.from_numpy(g["y_test"]).to(dev).clone(); Yt[:, 0] *= 400; Yt[:, 1] *= 400; Yt[:, 2:] *= P
    label = decode.nu_rate(Yt, Xs).sum()

    def less_ratio(d, K):
        plan = None if K == T else steps.strided(d, K)
        r = [float(decode.nu_rate(decode.nu_decode(d.sample(cond, OMEGA, seed=s, plan=plan), 400, 400, P), Xs).sum() / label) for s in SEEDS]
        return sum(r) / len(r)

    def loss_by_t(d):
        """One pass over the training rows under the uniform rule, fixed draws, no update: the mean squared error per timestep."""
        law, draws, calls = d.train_law, d.device_draws, d._draw_calls
        d.train_law, d.device_draws, d._draw_calls = None, 999, 0
        d.loss_report(True)
        d.read_loss_report()
        with torch.no_grad():
            for i in range(0, X.shape[0], BATCH):
                d(Y[i:i + BATCH].to(dev), X[i:i + BATCH].to(dev))
        mean, _ = d.read_loss_report()
        d.loss_report(False)
        d.train_law, d.device_draws, d._draw_calls = law, draws, calls
        return mean

    arms = {"uniform": lambda d: None, "on_plan K=5": lambda d: TS.on_plan(d, steps.strided(d, 5)),
            "on_plan K=7": lambda d: TS.on_plan(d, steps.strided(d, 7)), "min_snr g=5": lambda d: TS.min_snr(d, 5.0)}
    base = fresh()
    before_t = loss_by_t(base)
    before_q = {K: less_ratio(base, K) for K in KS}
    lines = [f"device: {torch.cuda.get_device_name(0)}",
             f"NU checkpoint, T = {T}; fine-tuning: {X.shape[0]} rows of noma_uav_gen (numpy seed {SEED}), batch {BATCH}, {EPOCHS} epochs, "
             f"FlatAdam lr {LR:g}, device draws seed {SEED}, graph=True; score: less ratio on the 512 test rows, omega = {OMEGA:g}, mean of seeds "
             f"{SEEDS[0]} .. {SEEDS[-1]}",
             f"{'arm':<14}" + "".join(f"{'K = ' + str(K):>10}" for K in KS) + "   epoch losses (weighted, as logged)",
             f"{'checkpoint':<14}" + "".join(f"{before_q[K]:>10.4f}" for K in KS)]
    by_t = {"checkpoint": before_t}
    for name, law_of in arms.items():
        d = fresh()
        d.train_law = law_of(d)
        d.device_draws = SEED
        opt = tr.FlatAdam(d, lr=LR)
        logged = []
        tr.run_epochs(d, None, opt, torch.optim.lr_scheduler.MultiStepLR(opt, [10 ** 9]), EPOCHS, False, 0, dev, logged.append, graph=True,
                      batches=tr.DeviceBatches(X, Y, BATCH, SEED, dev))
        q = {K: less_ratio(d, K) for K in KS}
        by_t[name] = loss_by_t(d)
        lines.append(f"{name:<14}" + "".join(f"{q[K]:>10.4f}" for K in KS) + "   " + " ".join(f"{float(ln.split('Loss:')[1]):.3e}" for ln in logged))
    lines.append("")
    lines.append("mean squared error per timestep (uniform pass over the training rows, draws seed 999), t = 0 .. T-1:")
    for name, v in by_t.items():
        lines.append(f"{name:<14}" + " ".join(f"{x:.3f}" for x in v.tolist()))
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(txt)
    print(txt)


if __name__ == "__main__":
    main()
