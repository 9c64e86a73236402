#!/usr/bin/env python3
"""Time the gradient-descent baseline (100 iterations, the reference's rates) per problem:

  launch ........ one dsg_gd_* call through diffsg_amd.gd on data that lives on the device, at 10 000 rows (the reference's largest
                  workload) and at 1 000 000 rows, between two device synchronisations (the copy of the start state included)
  numpy ......... the float64 restatement tests/gd_ref.py at 10 000 rows on one core (what baselines/GD.py does)

Median of REPEATS calls each.  Nothing in the package rests on these figures.  Writes them and the kernels' resource usage to --out
(default profiles/gd_time.txt).

    python tools/gd_time.py [--out FILE] [--repeats 7]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p_)

CASES = (("CO n=3", "co", 3), ("MSR M=3", "msr", 3), ("MSR M=80", "msr", 80), ("NU K=3", "nu", 3))


def median_ms(fn, repeats, sync, warmup=2):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gd_time.txt"))
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    torch.set_num_threads(1)
    from diffsg_amd import _lib, gd
    import gd_ref as GR

    def launch(kind, x, y0):
        if kind == "co":
            return lambda: gd.co_descent(x, y0)
        if kind == "msr":
            return lambda: gd.msr_descent(x, 10.0, y0)
        return lambda: gd.nu_descent(x, 18.0, 400, 400, y0)

    lines = [f"GD baseline, 100 iterations; device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; median (min .. max) of "
             f"{a.repeats} calls after 2 warm-up calls, wall clock, one process"]
    for title, kind, size in CASES:
        for rows in (10000, 1000000):
            x, y0 = GR.synth(kind, rows, size)
            xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y0).cuda()
            med, lo, hi = median_ms(launch(kind, xd, yd), a.repeats, torch.cuda.synchronize)
            lines.append(f"  {title:10s} {rows:8d} rows  one launch      {med:10.3f} ms  ({lo:.3f} .. {hi:.3f})")
            if rows == 10000:
                med, lo, hi = median_ms(lambda: GR.run(kind, x, y0, 100), max(3, a.repeats // 2), lambda: None, warmup=1)
                lines.append(f"  {title:10s} {rows:8d} rows  numpy, one core {med:10.3f} ms  ({lo:.3f} .. {hi:.3f})")
            del xd, yd
    for n, r in sorted(_lib.kernel_resources().items()):
        if "k_gd_" in n:
            lines.append(f"  {n}: {r['vgprs']} VGPRs, {r['agprs']} AGPRs, {r['sgprs']} SGPRs, scratch {r['scratch']} B/lane, LDS {r['lds']} B, "
                         f"occupancy {r['occupancy']} waves/SIMD")
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt)
    print(txt, end="")


if __name__ == "__main__":
    main()
