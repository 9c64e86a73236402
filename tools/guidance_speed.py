#!/usr/bin/env python3
"""Wall time of a sampling call under a guidance schedule: python tools/guidance_speed.py [out.txt] [--plain]
One GPU, one process.  Three shapes, captured graphs, range check off (a call only enqueues):
  msr80-65536   MSR-80c net, 65 536 rows, T = 20 (throughput bound);
  msr3-8192     BASELINE config 2's shape: MSR-3c net, 8 192 rows, T = 1000;
  nu3-16x512    NU-3u net, 16 chunks of 512 rows in one chunked call, T = 20 (one tile's dependent chain per chunk).
Per shape: the plan-less call, then the identity plan under the schedules all ones (the scheduled two-pass step), even step indices,
the middle half of the indices, and all zeros (the one-pass step); per call the median of 7 timed calls after 2 warm-up calls (host
wall time around call + synchronise) and the time per step = median / T.  `--plain` times the plan-less calls only: that runs on a tree
without guidance schedules too, for the parent commit's numbers on the same box.  The box probe (dsg_box_calibrate) before and after.
Writes the table to `out.txt` (default profiles/guidance_speed.txt) and prints it."""
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

# name: (net, rows, chunk rows or None, T, omega)
SHAPES = {"msr80-65536": ("msr80", 65536, None, 20, 1.0), "msr3-8192": ("msr3", 8192, None, 1000, 1.0), "nu3-16x512": ("nu3", 16 * 512, 512, 20, 1.0)}


def build(net, T):
    from _util import synth_params
    from oracle import ddpm_oracle as O
    from weights import CONFIGS
    from diffsg_amd import UNet1D
    from diffsg_amd.classifier_free_MSR import DDPM
    cfg = CONFIGS[net]
    _, p = synth_params(net, 7)
    m = UNet1D(**cfg, is_attn=(False,) * len(cfg["dims"]))
    m.load_state_dict(p)
    D = cfg["input_dim"]
    return DDPM(T, m.to("cuda"), D, 10.0, 1.0 - O.cosine_betas(T), torch.device("cuda"), (1, D), None).to("cuda"), cfg["cond_dim"]


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
    plain_only = "--plain" in sys.argv
    path = args[0] if args else os.path.join(ROOT, "profiles", "guidance_speed.txt")
    lines = [f"device: {torch.cuda.get_device_name(0)}", f"box before: {box_calibrate()}",
             "graph, check_range off; median (min .. max) ms of 7 calls after 2 warm-up calls",
             f"{'shape':<14}{'call':<26}{'passes':>7}{'ms per call':>34}{'us per step':>13}"]
    for shape, (net, rows, chunk, T, omega) in SHAPES.items():
        ddpm, C = build(net, T)
        cond = torch.rand(rows, C, generator=torch.Generator().manual_seed(0)).cuda()
        seeds = list(range(1, 1 + (rows // chunk if chunk else 1)))

        def call(plan):
            if chunk:
                return ddpm.sample_chunked(cond, omega, chunk, seeds=seeds, check_range=False, plan=plan)
            return ddpm.sample(cond, omega, seed=1, check_range=False, plan=plan)

        def row(tag, passes, plan):
            med, lo, hi = median_ms(lambda: call(plan))
            lines.append(f"{shape:<14}{tag:<26}{passes:>7}{med:>14.3f} ({lo:.3f} .. {hi:.3f})".ljust(81) + f"{med / T * 1e3:>13.2f}")

        row("no plan", 2 * T, None)
        if not plain_only:
            from diffsg_amd import steps
            for tag, g in (("all ones", torch.ones(T)), ("even indices", steps.guidance_every(T, 2)),
                           ("middle half", steps.guidance_interval(T, T // 4, T // 4 + T // 2 - 1)), ("all zeros", torch.zeros(T))):
                row(tag, int(T + (g != 0).sum()), steps.with_guidance(ddpm, g))
            row("no plan again", 2 * T, None)
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
