#!/usr/bin/env python3
"""Repeated sampling's selection step against the torch composition of the existing calls: python tools/best_of_time.py [out.txt]
One GPU, one process.  Per shape: the fused `diffsg_amd.best_of` (one statistics pass + one selection launch) and the
composition it replaces (per round decode.*_decode, the objective, a strict-improvement torch.where update of the running
solution / objective / round).  Warm-up, then the median of 25 timed calls with HIP events around each call; the box
probe (dsg_box_calibrate) before and after.  Writes the table to `out.txt` (default profiles/best_of_time.txt) and prints it."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench import box_calibrate  # noqa: E402
from diffsg_amd import best_of, decode as Dc  # noqa: E402

NU = {"width": 400, "height": 400, "p_sum": 18.0}


def compose(problem, Y, X, **p):
    sol = obj = rnd = None
    for k in range(Y.shape[0]):
        if problem == "msr":
            s = p["W"] * Dc.msr_decode(Y[k]); o = Dc.msr_rate(s, X)
        else:
            s = Dc.nu_decode(Y[k], p["width"], p["height"], p["p_sum"]); o = Dc.nu_rate(s, X)
        fin = torch.isfinite(o)
        idx = torch.full_like(o, k, dtype=torch.int32)
        if sol is None:
            sol, obj, rnd = s, o, torch.where(fin, idx, torch.full_like(idx, -1))
            continue
        take = fin & ((rnd < 0) | (o > obj))
        sol, obj, rnd = torch.where(take[:, None], s, sol), torch.where(take, o, obj), torch.where(take, idx, rnd)
    return sol, obj, rnd


def median_ms(fn, warmup=5, calls=25):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "best_of_time.txt")
    g = torch.Generator().manual_seed(0)
    lines = [f"device: {torch.cuda.get_device_name(0)}", f"box before: {box_calibrate()}",
             "median (min .. max) ms of 25 calls after 5 warm-up calls, HIP events around each call",
             f"{'shape':<34}{'fused best_of':>26}{'torch composition':>28}{'ratio':>8}"]
    for problem, B, D, n in [("msr", 65536, 80, 1), ("msr", 65536, 80, 8), ("nu", 8192, 5, 64)]:
        Y = (torch.randn(n, B, D, generator=g) * (3.0 if problem == "msr" else 1.0)).cuda()
        if problem == "msr":
            X, p = (torch.rand(B, D, generator=g) * 2.0 + 0.5).cuda(), {"W": 20.0}
        else:
            X, p = (torch.rand(B, 2 * (D - 2), generator=g) * 400.0).cuda(), dict(NU)
        a, b = best_of(problem, Y, X, **p), compose(problem, Y, X, **p)
        assert all(torch.equal(x, y) for x, y in zip(a[:3], b)), "the fused call and the composition disagree"
        f = median_ms(lambda: best_of(problem, Y, X, **p))
        c = median_ms(lambda: compose(problem, Y, X, **p))
        lines.append(f"{problem.upper() + f' {B} x {D}, n = {n} ({B * n} rows)':<34}"
                     f"{f[0]:>10.4f} ({f[1]:.4f} .. {f[2]:.4f})" f"{c[0]:>12.4f} ({c[1]:.4f} .. {c[2]:.4f})" f"{c[0] / f[0]:>8.2f}")
    lines.append(f"box after: {box_calibrate()}")
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(txt)
    print(txt)


if __name__ == "__main__":
    main()
