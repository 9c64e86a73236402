#!/usr/bin/env python3
"""Wall time of a sampling call on a sub-sequence of the trained steps: python tools/steps_speed.py [out.txt] [--no-plans]
One GPU, one process.  BASELINE config 2's shape (MSR-3c net, 8 192 rows, T = 1000, omega = 1, captured graphs): `sample()` and
`sample(plan=steps.strided(ddpm, K))` for K in 250, 100, 50; per call the median of 7 timed calls after 2 warm-up calls (host wall
time around call + synchronise, range check off: the call only enqueues), and the time per step = median / K.  The box probe
(dsg_box_calibrate) before and after.  `--no-plans` times the plan-less call only: that runs on a tree without step plans too, for the
per-step time of a parent commit on the same box.  Writes the table to `out.txt` (default profiles/steps_speed.txt) and prints it."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch  # noqa: E402

from bench import box_calibrate  # noqa: E402

B, T, OMEGA = 8192, 1000, 1.0


def build():
    from _util import synth_params
    from oracle import ddpm_oracle as O
    from weights import CONFIGS
    from diffsg_amd import UNet1D
    from diffsg_amd.classifier_free_MSR import DDPM
    cfg = CONFIGS["msr3"]
    _, p = synth_params("msr3", 7)
    m = UNet1D(**cfg, is_attn=(False,) * len(cfg["dims"]))
    m.load_state_dict(p)
    return DDPM(T, m.to("cuda"), 3, 10.0, 1.0 - O.cosine_betas(T), torch.device("cuda"), (1, 3), None).to("cuda")


def median_ms(fn, warmup=2, calls=7):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    plans = "--no-plans" not in sys.argv
    path = args[0] if args else os.path.join(ROOT, "profiles", "steps_speed.txt")
    ddpm = build()
    cond = torch.rand(B, 3, generator=torch.Generator().manual_seed(0)).cuda()
    lines = [f"device: {torch.cuda.get_device_name(0)}", f"box before: {box_calibrate()}",
             f"msr3, {B} rows, T = {T}, omega = {OMEGA:g}, graph; median (min .. max) ms of 7 calls after 2 warm-up calls",
             f"{'call':<28}{'steps':>6}{'ms per call':>34}{'us per step':>13}"]

    def row(tag, K, fn):
        med, lo, hi = median_ms(fn)
        lines.append(f"{tag:<28}{K:>6}{med:>14.3f} ({lo:.3f} .. {hi:.3f})".ljust(68) + f"{med / K * 1e3:>13.2f}")

    row("sample()", T, lambda: ddpm.sample(cond, OMEGA, seed=1, check_range=False))
    if plans:
        from diffsg_amd import steps
        for K in (250, 100, 50):
            plan = steps.strided(ddpm, K)
            row(f"sample(plan=strided({K}))", K, lambda: ddpm.sample(cond, OMEGA, seed=1, check_range=False, plan=plan))
        row("sample() again", T, lambda: ddpm.sample(cond, OMEGA, seed=1, check_range=False))
    ddpm.model.check_range()
    lines.append(f"box after: {box_calibrate()}")
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(txt)
    print(txt)


if __name__ == "__main__":
    main()
