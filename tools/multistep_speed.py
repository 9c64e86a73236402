#!/usr/bin/env python3
"""Wall time of a sampling call under a two-step plan: python tools/multistep_speed.py [out.txt]
One GPU, one process.  Two shapes, captured graphs, range check off (a call only enqueues):
  msr80-65536   the bench shape: MSR-80c net, 65 536 rows, T = 20, K = 10 (throughput bound);
  msr3-8192     BASELINE config 2's shape: MSR-3c net, 8 192 rows, T = 1000, K = 50 on the log-SNR grid.
Per shape, on one grid and with the default min(K, 4) early renormalised steps in all three (so that only the update differs): `ddim(K)`
(k_update), the same table with an all-zero history (k_update_hist moving the bytes of k_update) and `dpmpp_2m(K)` (K - 6 second-order
steps, each one more read of the history, and as many steps that store it: one more write); per call the median of 7 timed calls
after 2 warm-up calls (host wall time around call + synchronise) and the time per step = median / K.  The box probe
(dsg_box_calibrate) before and after.
Writes the table to `out.txt` (default profiles/multistep_speed.txt) and prints it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from bench import box_calibrate  # noqa: E402
from guidance_speed import build, median_ms  # noqa: E402

# name: (net, rows, T, K, log-SNR grid, omega)
SHAPES = {"msr80-65536": ("msr80", 65536, 20, 10, False, 1.0), "msr3-8192": ("msr3", 8192, 1000, 50, True, 1.0)}


def main():
    from diffsg_amd import steps
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", "multistep_speed.txt")
    lines = [f"device: {torch.cuda.get_device_name(0)}", f"box before: {box_calibrate()}",
             "graph, check_range off, min(K, 4) renorm steps; median (min .. max) ms of 7 calls after 2 warm-up calls",
             f"{'shape':<14}{'call':<30}{'2nd-order':>10}{'ms per call':>34}{'us per step':>13}"]
    for shape, (net, rows, T, K, logsnr, omega) in SHAPES.items():
        ddpm, C = build(net, T)
        cond = torch.rand(rows, C, generator=torch.Generator().manual_seed(0)).cuda()
        taus = steps.logsnr_taus(ddpm, K) if logsnr else None
        two = steps.dpmpp_2m(ddpm, None if taus else K, taus=taus)
        one = steps.ddim(ddpm, None if taus else K, 0.0, taus=taus)
        n = two.K

        def row(tag, plan):
            second = 0 if plan.history is None else int((plan.history[:, 0] != 0).sum())
            med, lo, hi = median_ms(lambda: ddpm.sample(cond, omega, seed=1, check_range=False, plan=plan))
            lines.append(f"{shape:<14}{tag:<30}{second:>10}{med:>14.3f} ({lo:.3f} .. {hi:.3f})".ljust(88) + f"{med / n * 1e3:>13.2f}")

        row(f"ddim({n})", one)
        row(f"ddim({n}) + all-zero history", steps.with_history(one, torch.zeros(n, 3)))
        row(f"dpmpp_2m({n})", two)
        row(f"ddim({n}) again", one)
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
