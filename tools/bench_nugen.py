#!/usr/bin/env python3
"""NU label generator (datasets/noma_uav_gen.py): device time of noma_uav_gen for 2 500 and 10 000 samples at P_sum = 18 (the
reference's job and the size of its shipped set) and 100 samples at P_sum = 30, copies included, next to the CPU restatement
(tests/nu_gen_ref.py, one thread) on a bounded sample.  Work is counted as inside grid points x table rows (float64 rate
evaluations).  Prints one JSON line; with --out FILE also writes it there.

    python tools/bench_nugen.py [--out profiles/<tag>_nugen.json]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
from diffsg_amd.labelgen import coordinates_gen, feasible_solution, noma_uav_gen
import nu_gen_ref as N

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
args = ap.parse_args()


def evaluations(qs, nfs):
    """inside grid points x table rows; drawn triangles have integer corners, so only their bounding boxes are scanned
    (a degenerate one, whose whole line counts, goes through the full-grid scan of the restatement)"""
    from diffsg_amd.labelgen import is_point_inside_triangle
    pts = 0
    for q in qs:
        if (q[2] - q[0]) * (q[5] - q[1]) - (q[4] - q[0]) * (q[3] - q[1]) == 0:
            pts += int(N.inside_points(q).size)
            continue
        x, y = np.meshgrid(np.arange(q[0::2].min(), q[0::2].max() + 1), np.arange(q[1::2].min(), q[1::2].max() + 1))
        pts += int(np.count_nonzero(is_point_inside_triangle([x, y], q[0:2], q[2:4], q[4:6])))
    return pts * nfs


out = {"device": torch.cuda.get_device_name(0)}
quiet = lambda *_: None
for P, n, reps in ((18, 2500, 2), (18, 10000, 1), (30, 100, 2)):
    np.random.seed(1000 + n)
    qs = coordinates_gen(n)
    fs = feasible_solution(P)
    noma_uav_gen(min(n, 64), P, qs=qs[:min(n, 64)], log=quiet)           # warm-up (library load, first launch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        noma_uav_gen(n, P, qs=qs, log=quiet)
    s = (time.perf_counter() - t0) / reps
    ev = evaluations(qs, fs.shape[0])
    out[f"P{P}_{n}"] = {"s_per_call_incl_copies": s, "samples_per_s": n / s, "evaluations": ev, "gevals_per_s": ev / s / 1e9}
np.random.seed(7)
qs = coordinates_gen(2)
fs = feasible_solution(18)
t0 = time.perf_counter()
N.noma_uav_search(qs, fs)
cpu = time.perf_counter() - t0
out["cpu_restatement"] = {"samples": 2, "P_sum": 18, "seconds": cpu, "s_per_sample": cpu / 2,
                          "gevals_per_s": evaluations(qs, fs.shape[0]) / cpu / 1e9}
line = json.dumps(out)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
