#!/usr/bin/env python3
"""Wall time of a sampling call under an x0 clip: python tools/clip_speed.py [out.txt]
One GPU, one process.  Two shapes, captured graphs, range check off (a call only enqueues):
  msr80-65536   the bench shape: MSR-80c net, 65 536 rows, T = 20, K = 10 (throughput bound);
  msr3-8192     BASELINE config 2's shape: MSR-3c net, 8 192 rows, T = 1000, K = 50.
Per shape, on one grid and with the default min(K, 4) early renormalised steps in all four (so that only the update differs): `ddim(K)`
(k_update), the same plan with infinite bounds (k_update_clip, every select keeps eps), the same plan with binding bounds ([-0.5, 0.5]: a
good share of the predictions of an untrained net is clamped) and `ddim(K)` again; per call the median of 7 timed calls after 2 warm-up
calls (host wall time around call + synchronise) and the time per step = median / K.  The box probe (dsg_box_calibrate) before and
after.  The clip adds no per-element stream (the bounds are D floats): what shows is the extra arithmetic of a memory-bound kernel.
Writes the table to `out.txt` (default profiles/clip_speed.txt) and prints it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from bench import box_calibrate  # noqa: E402
from guidance_speed import build, median_ms  # noqa: E402

# name: (net, rows, T, K, omega)
SHAPES = {"msr80-65536": ("msr80", 65536, 20, 10, 1.0), "msr3-8192": ("msr3", 8192, 1000, 50, 1.0)}


def main():
    from diffsg_amd import steps
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", "clip_speed.txt")
    lines = [f"device: {torch.cuda.get_device_name(0)}", f"box before: {box_calibrate()}",
             "graph, check_range off, min(K, 4) renorm steps; median (min .. max) ms of 7 calls after 2 warm-up calls",
             f"{'shape':<14}{'call':<34}{'ms per call':>34}{'us per step':>13}"]
    inf = float("inf")
    for shape, (net, rows, T, K, omega) in SHAPES.items():
        ddpm, C = build(net, T)
        cond = torch.rand(rows, C, generator=torch.Generator().manual_seed(0)).cuda()
        one = steps.ddim(ddpm, K, 0.0)

        def row(tag, plan):
            med, lo, hi = median_ms(lambda: ddpm.sample(cond, omega, seed=1, check_range=False, plan=plan))
            lines.append(f"{shape:<14}{tag:<34}{med:>14.3f} ({lo:.3f} .. {hi:.3f})".ljust(82) + f"{med / K * 1e3:>13.2f}")

        row(f"ddim({K})", one)
        row(f"ddim({K}) + clip [-inf, inf]", steps.with_clip(one, -inf, inf))
        row(f"ddim({K}) + clip [-0.5, 0.5]", steps.with_clip(one, -0.5, 0.5))
        row(f"ddim({K}) again", one)
        ddpm.model.check_range()
        del ddpm
    lines.append(f"box after: {box_calibrate()}")
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(txt)
    print(txt)


if __name__ == "__main__":
    main()
