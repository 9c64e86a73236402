#!/usr/bin/env python3
"""Fixed cost of a large launch as profiles/HISTORY.md defines it: dsg_time_op times of one operator at 2 048 / 3 072 / 4 096 / 6 144
row tiles (two passes of 32 768 ... 98 304 rows), least-squares line through the four points, the intercept at zero tiles.
    python tools/launch_fixed_cost.py [op ...]        (default: one up-128, one down-128, one up-64 launch)
Works in an older tree copied under ab_old/ as well (run it there): same-box comparisons only."""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch
import bench
from diffsg_amd import _lib

ops = sys.argv[1:] or ["up.17.res", "down.1.res", "up.13.res"]
ROWS = (32768, 49152, 65536, 98304)
dev = torch.device("cuda:0")
ddpm = bench.build_model(dev, 6)
ddpm.model.set_launch_policy(0, 0)
L, hd = _lib.lib(), ddpm.model.native_handle()
times = {o: [] for o in ops}
for B in ROWS:
    cond = torch.rand(B, 80, device=dev)
    ddpm.sample(cond, 1.0, seed=1)          # fills the workspace with real activations of this size
    names = []
    for i in range(L.dsg_op_count(hd)):
        nm = ctypes.create_string_buffer(64)
        L.dsg_op_info(hd, i, nm, None, None)
        names.append(nm.value.decode())
    for o in ops:
        ms = ctypes.c_float()
        best = None
        for rep in range(5):
            _lib.check(L.dsg_time_op(hd, names.index(o), B, 40, ctypes.byref(ms), _lib.stream_ptr()))
            torch.cuda.synchronize()
            best = ms.value if best is None else min(best, ms.value)
        times[o].append(best * 1e3)
tiles = [2 * B // 32 for B in ROWS]
print("tiles            " + " ".join(f"{t:8d}" for t in tiles) + "   us/1024 tiles  intercept us")
n = len(tiles)
mx = sum(tiles) / n
for o in ops:
    my = sum(times[o]) / n
    slope = sum((x - mx) * (y - my) for x, y in zip(tiles, times[o])) / sum((x - mx) ** 2 for x in tiles)
    print(f"{o:16s} " + " ".join(f"{v:8.1f}" for v in times[o]) + f"   {slope * 1024:13.2f}  {my - slope * mx:12.2f}")
