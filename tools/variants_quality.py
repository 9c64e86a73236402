#!/usr/bin/env python3
"""Best-of-n over sampler settings on the device: python tools/variants_quality.py [out.txt]
The NU checkpoint golden (tests/golden/g4_sample_nu_ckpt.npz), its 512 rows, T = 20: `DDPM.sample_best(cond, X, 16, variants=...)` with the
device's Philox draws (seeds 101 .. 116, and 11 .. 18), the rows of the CPU table tests/golden/g18_variants.json.  Printed per row:
sum over the conditions of the best rate of the first n rounds / sum of the stored labels' rate, n = 4, 8, 16.  The draws are not the
CPU table's (torch's generator there), so the two tables agree in what they show, not digit for digit."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch  # noqa: E402

RENORM, OMEGAS = (4, 0, 2, 1, 3), (500.0, 200.0, 2000.0, 50.0)


def main():
    import steps_ref as R
    from oracle import ddpm_oracle as O
    from weights import CONFIGS
    from diffsg_amd import UNet1D, decode, steps
    from diffsg_amd import classifier_free_NU as NU
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "variants_quality.txt")
    g = R.nu_golden()
    T, P = int(g["T"]), float(g["P_sum"])
    cfg = CONFIGS["nu3"]
    m = UNet1D(**cfg, is_attn=(False,) * len(cfg["dims"]))
    m.load_state_dict(R.net_params("nu3")[1])
    dev = torch.device("cuda")
    d = NU.DDPM(T, m.to(dev), 3, 18.0, 1.0 - O.cosine_betas(T), dev, (1, 5), {"width": 400, "height": 400}).to(dev)
    cond = torch.from_numpy(g["cond"]).cuda()
    Xs = cond.clone(); Xs[:, 0::2] *= 400; Xs[:, 1::2] *= 400
    Yt = torch.from_numpy(g["y_test"]).cuda().clone(); Yt[:, 0] *= 400; Yt[:, 1] *= 400; Yt[:, 2:] *= P
    label = decode.nu_rate(Yt, Xs).sum()
    ddim = steps.ddim(d, 10, 0.0)

    def variants(row, base):
        om = OMEGAS if "omega" in row else (500.0,)
        rn = RENORM if "renorm" in row else (4,)
        n = len(om) * len(rn)
        return [(om[r % len(om)], steps.with_renorm(base, rn[r % len(rn)])) for r in range(n)]

    lines = [f"device: {torch.cuda.get_device_name(0)}", "NU checkpoint, 512 rows, sample_best, Philox seeds; best-of-n ratio to the stored labels",
             f"{'rounds':<40}{'n = 4':>10}{'n = 8':>10}{'n = 16':>10}"]
    for tag, row, base, seeds in (("T20 same setting", "same", d, range(101, 117)), ("T20 renorm cycled", "renorm", d, range(101, 117)),
                                  ("T20 renorm and omega cycled", "renorm+omega", d, range(101, 117)),
                                  ("K10 DDIM0 same setting", "same", ddim, range(101, 117)), ("K10 DDIM0 renorm cycled", "renorm", ddim, range(101, 117)),
                                  ("T20 same setting, seeds 11..", "same", d, range(11, 19)), ("T20 omega cycled, seeds 11..", "omega", d, range(11, 19)),
                                  ("T20 renorm cycled, seeds 11..", "renorm", d, range(11, 19))):
        seeds = list(seeds)
        vs = variants(row, base)
        best = d.sample_best(cond, Xs, len(seeds), seeds=seeds, return_objectives=True, variants=vs)
        obj = best.objectives                                     # [rounds][512]
        cells = [f"{float(obj[:n].max(dim=0).values.sum() / label):>10.4f}" if n <= len(seeds) else f"{'':>10}" for n in (4, 8, 16)]
        single = [float(obj[r].sum() / label) for r in range(len(seeds))]
        wins = torch.bincount(best.round.clamp(min=0) % len(vs), minlength=len(vs)).tolist()
        lines.append(f"{tag:<40}" + "".join(cells) + f"   single rounds {min(single):.3f} .. {max(single):.3f}; wins per variant {wins}")
        print(lines[-1], flush=True)
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(txt)
    print(txt)


if __name__ == "__main__":
    main()
