#!/usr/bin/env python3
"""The quality table of DESIGN.md 16 on the device: python tools/guidance_quality.py [out.txt]
The shipped NU checkpoint (tests/golden/g4_sample_nu_ckpt.npz) on its 512 rows, T = 20, omega = 500, under the guidance masks of
tests/golden/g19_guidance.json: every step guided, step indices 5 .. 14, the even indices, every third (j % 3 == 1).  Per mask the
less ratio of a single round (mean of seeds 101 .. 104, min and max), of best-of-8 (seeds 101 .. 108) with 4 renorm steps, and of
best-of-8 with the renorm count cycled 4, 0, 2, 1, 3 -- the CPU table's columns.  The draws are the device's Philox streams under those
seed NUMBERS, not the CPU table's torch draws: the two tables agree in distribution, not value by value.  Scored by the product's
decoder and evaluator on the device.  Writes the table to `out.txt` (default profiles/guidance_quality.txt) and prints it, with the CPU
column beside it."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

SEEDS = tuple(range(101, 109))
RENORM_CYCLE = (4, 0, 2, 1, 3)
OMEGA = 500.0


def main():
    from oracle import ddpm_oracle as O
    from weights import CONFIGS
    from diffsg_amd import UNet1D, decode, steps
    from diffsg_amd import classifier_free_NU as NU
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "guidance_quality.txt")
    gold = os.path.join(ROOT, "tests", "golden")
    g = np.load(os.path.join(gold, "g4_sample_nu_ckpt.npz"))
    with open(os.path.join(gold, "g19_guidance.json")) as f:
        cpu = json.load(f)["T20"]
    T, P = int(g["T"]), float(g["P_sum"])
    cfg = CONFIGS["nu3"]
    m = UNet1D(**cfg, is_attn=(False,) * len(cfg["dims"]))
    m.load_state_dict({k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w.")}, strict=True)
    D = cfg["input_dim"]
    d = NU.DDPM(T, m.to("cuda"), D - 2, P, 1.0 - O.cosine_betas(T), torch.device("cuda"), (1, D), {"width": 400, "height": 400}).to("cuda")
    cond = torch.from_numpy(g["cond"]).cuda()
    Xs = cond.clone(); Xs[:, 0::2] *= 400; Xs[:, 1::2] *= 400
    Yt = torch.from_numpy(g["y_test"]).cuda().clone(); Yt[:, 0] *= 400; Yt[:, 1] *= 400; Yt[:, 2:] *= P
    label = decode.nu_rate(Yt, Xs).sum()
    masks = {"all": torch.ones(T), "interval5_14": steps.guidance_interval(T, 5, 14), "even": steps.guidance_every(T, 2),
             "third": steps.guidance_every(T, 3, 1)}

    def rate(seed, mask, renorm):
        plan = steps.with_renorm(steps.with_guidance(d, mask), renorm)
        return decode.nu_rate(decode.nu_decode(d.sample(cond, OMEGA, seed=seed, plan=plan), 400, 400, P), Xs)

    lines = [f"device: {torch.cuda.get_device_name(0)}",
             f"NU checkpoint, 512 rows, T = {T}, omega = {OMEGA:g}, device Philox draws under seeds {SEEDS[0]} .. {SEEDS[-1]}; CPU value (torch draws) in brackets",
             f"{'mask':<14}{'passes':>7}  {'single round: mean [min, max]':<44}{'best-of-8, 4 renorm':<24}{'best-of-8, renorm cycled':<24}"]
    for name, mask in masks.items():
        same = [rate(s, mask, 4) for s in SEEDS]
        cyc = [rate(s, mask, RENORM_CYCLE[r % len(RENORM_CYCLE)]) for r, s in enumerate(SEEDS)]
        single = [float(x.sum() / label) for x in same[:4]]
        b_same = float(torch.stack(same).max(dim=0).values.sum() / label)
        b_cyc = float(torch.stack(cyc).max(dim=0).values.sum() / label)
        c = cpu[name]
        lines.append(f"{name:<14}{int(T + (mask != 0).sum()):>7}  "
                     + f"{sum(single) / 4:.4f} [{min(single):.4f}, {max(single):.4f}] ({c['single_mean']:.4f})".ljust(44)
                     + f"{b_same:.4f} ({c['best8_same']:.4f})".ljust(24) + f"{b_cyc:.4f} ({c['best8_renorm']:.4f})")
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(txt)
    print(txt)


if __name__ == "__main__":
    main()
