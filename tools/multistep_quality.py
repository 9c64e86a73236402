#!/usr/bin/env python3
"""Less ratio of the shipped NU checkpoint on the device under DDIM eta = 0 and under the two-step rule:
python tools/multistep_quality.py [out.txt]
The checkpoint golden's 512 rows with its own y_T, T = 20, omega = 500; K in {10, 7, 5}, 4 and 0 early renormalised steps; scored by the
product's decoder and evaluator on the device, beside the CPU value of tests/golden/g18_multistep.json.  float32 itself is good to about
2.6e-3 against float64 at this omega (tests/test_gpu_parity.py), so device and CPU agree to that, not to the last digit.
Writes the table to `out.txt` (default profiles/multistep_quality.txt) and prints it."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch  # noqa: E402


def main():
    import steps_ref as R
    from test_gpu_guidance import make_ddpm
    from diffsg_amd import decode, steps
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", "multistep_quality.txt")
    with open(os.path.join(ROOT, "tests", "golden", "g18_multistep.json")) as f:
        cpu = json.load(f)["ratios"]
    g = R.nu_golden()
    d = make_ddpm("nu3")
    cond = torch.from_numpy(g["cond"]).cuda()
    y_T = torch.from_numpy(g["y_T"])
    P = float(g["P_sum"])
    Xs = cond.clone(); Xs[:, 0::2] *= 400; Xs[:, 1::2] *= 400
    Yt = torch.from_numpy(g["y_test"]).cuda().clone(); Yt[:, 0] *= 400; Yt[:, 1] *= 400; Yt[:, 2:] *= P
    label = decode.nu_rate(Yt, Xs).sum()
    lines = [f"device: {torch.cuda.get_device_name(0)}", "NU checkpoint, 512 rows, T = 20, omega = 500: less ratio, device (CPU reference)",
             f"{'K':>3}{'renorm':>8}{'DDIM eta = 0':>24}{'two-step':>24}"]
    for K in (10, 7, 5):
        for rn in (4, 0):
            cells = []
            for rule, plan in (("ddim0", steps.with_renorm(steps.ddim(d, K, 0.0), rn)), ("2m", steps.dpmpp_2m(d, K, renorm_steps=rn))):
                y0 = d.sample_checked(cond, 500.0, y_T=y_T, plan=plan)
                ratio = float(decode.nu_rate(decode.nu_decode(y0, 400, 400, P), Xs).sum() / label)
                cells.append(f"{ratio:.5f} ({cpu[f'K{K}_r{rn}_{rule}']:.5f})")
            lines.append(f"{K:>3}{rn:>8}{cells[0]:>24}{cells[1]:>24}")
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(txt)
    print(txt)


if __name__ == "__main__":
    main()
