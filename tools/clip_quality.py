#!/usr/bin/env python3
"""Less ratio of the shipped NU checkpoint on the device with and without the x0 clip:
python tools/clip_quality.py [out.txt]
The checkpoint golden's 512 rows with its own y_T and z, T = 20; the settings of tests/clip_ref.NU_CELLS (trained 20 steps at omega = 500,
`ddim` and `strided` K-step plans at small omega; bounds from the golden's own y_test); scored by the product's decoder and evaluator on the
device, beside the CPU value of tests/golden/g21_clip.json.  Per cell also whether the fp16 range guard repeated the call on the exact
kernels (`exact`: it did; `split`: the split-f16 result stood).  float32 itself is good to about 2.6e-3 against float64 at omega = 500
(tests/test_gpu_parity.py), so device and CPU agree to that there, not to the last digit.
Writes the table to `out.txt` (default profiles/clip_quality.txt) and prints it."""
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch  # noqa: E402


def main():
    import clip_ref as C
    import steps_ref as R
    from test_gpu_guidance import make_ddpm
    from diffsg_amd import decode, steps
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", "clip_quality.txt")
    with open(os.path.join(ROOT, "tests", "golden", "g21_clip.json")) as f:
        cpu = json.load(f)["cells"]
    g = R.nu_golden()
    d = make_ddpm("nu3")
    cond = torch.from_numpy(g["cond"]).cuda()
    y_T, z = torch.from_numpy(g["y_T"]), torch.from_numpy(g["z"])
    D = y_T.shape[1]
    P = float(g["P_sum"])
    Xs = cond.clone(); Xs[:, 0::2] *= 400; Xs[:, 1::2] *= 400
    Yt = torch.from_numpy(g["y_test"]).cuda().clone(); Yt[:, 0] *= 400; Yt[:, 1] *= 400; Yt[:, 2:] *= P
    label = decode.nu_rate(Yt, Xs).sum()
    lines = [f"device: {torch.cuda.get_device_name(0)}", "NU checkpoint, 512 rows, T = 20: less ratio, device (CPU reference), range guard",
             f"{'cell':<24}{'no clip':>32}{'clipped':>32}"]
    for key, kind, K, eta, omega, rn, spec in C.NU_CELLS:
        base = steps.strided(d, d.T) if kind == "identity" else steps.strided(d, K) if kind == "strided" else steps.ddim(d, K, eta)
        base = steps.with_renorm(base, rn)
        cells = []
        for tag, plan in (("plain", base), ("clip", steps.with_clip(base, *C.nu_bounds(spec, D)))):
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                y0 = d.sample(cond, omega, y_T=y_T, noise=z[:plan.K - 2], plan=plan)
            guard = "exact" if any("repeating the call" in str(x.message) for x in w) else "split"
            ratio = float(decode.nu_rate(decode.nu_decode(y0, 400, 400, P), Xs).sum() / label)
            cells.append(f"{ratio:.5f} ({cpu[key][tag]:.5f}) {guard}")
        lines.append(f"{key:<24}{cells[0]:>32}{cells[1]:>32}")
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(txt)
    print(txt)


if __name__ == "__main__":
    main()
