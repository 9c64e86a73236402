#!/usr/bin/env python3
"""Phase stamps of down.0 at the bench size in both forms (library built with DSG_EXTRA_CXXFLAGS="-DDSG_CYCLE_STAMPS -DDSG_STAMP_DOWN0=1",
run with the same variable set; full panels: the stamp area only fits beside the 8-wave form's LDS):
    python tools/duo_stamps.py [B]
cfg_share 0: k_panel128_h<false, 0, 1, 4>, a wave walks two tiles; 1: k_panel128_duo_h<4>, a wave walks one row tile.
Tags as tools/panel_stamps.py (01 group start; S0 row statistics done; S1 step 0 prepared; S4 panel begun; S2 panel's MFMA stream done;
13 / 23 stage epilogue; 33 condition embedding added; 43 stage 3 un-scaled and residual added; 50 stored; the launch preamble: 02 init
done, 05 prologue's requests issued, 03 per-feature vectors loaded and written to LDS, 04 staging barrier passed).  The last stamped launch of
the call is read: the final step's down.0.  The stamps write LDS: the stamped binary's RESULTS are not valid, only its timing."""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch, bench
from diffsg_amd import _lib
B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
T = 6
dev = torch.device("cuda:0")
ddpm = bench.build_model(dev, T)
ddpm.model.set_option("panel_half", 0)
cond = torch.rand(B, 80, device=dev)
L2 = ctypes.CDLL(os.path.join(ROOT, "diffsg_amd", "libdiffsg_hip.so"))
GROUP = {0x10: "stats", 0x11: "prep0", 0x14: "wait+barrier", 0x12: "mfma", 0x13: "epilogue", 0x20: "stats", 0x21: "prep0", 0x24: "wait+barrier",
         0x22: "mfma", 0x23: "epilogue", 0x33: "cond", 0x30: "stats", 0x31: "prep0", 0x34: "wait+barrier", 0x32: "mfma", 0x43: "epilogue",
         0x50: "store", 0x01: "seam"}
for val in (0, 1):
    ddpm.model.set_option("cfg_share", val)
    ddpm.sample(cond, 1.0, seed=1, check_range=False)
    ddpm.sample(cond, 1.0, seed=1, profile=True, check_range=False)
    torch.cuda.synchronize()
    us = {r[0]: r[3] / T * 1e3 for r in ddpm.op_profile()}["down.0.res"]
    buf = (ctypes.c_ulonglong * 8192)()
    n = L2.dsg_stamps_fetch(buf, 8192)
    print(f"cfg_share={val}: down.0.res {us:.1f} us per launch (stamped build, full panels); {n} stamp slots")
    if n >= 8 * 128 + 4:
        t0, r0, t1, r1 = (buf[8 * 128 + k] for k in range(4))
        if r1 > r0:
            print(f"  workgroup 0, whole launch: {t1 - t0} shader cycles in {(r1 - r0) * 10} ns = {(t1 - t0) / ((r1 - r0) * 10.0):.3f} GHz")
    for w in range(8):
        st = [(buf[w * 128 + k] >> 16, buf[w * 128 + k] & 0xffff) for k in range(128) if buf[w * 128 + k]]
        if not st:
            continue
        if w in (0, 4):
            print(f"  wave {w}: " + " ".join(f"{tag:02x}:{t - p}" for (t, tag), (p, _) in zip(st[1:], st[:-1])))
        tot = {}
        for (t, tag), (p, _) in zip(st[1:], st[:-1]):
            tot[GROUP.get(tag, hex(tag))] = tot.get(GROUP.get(tag, hex(tag)), 0) + t - p
        print(f"  wave {w}: first stamp {st[0][0] - t0 if n >= 8 * 128 + 4 else 0} cycles after the kernel's start, {st[-1][0] - st[0][0]} cycles first to last stamp; by kind: {tot}")
        if n >= 8 * 128 + 4:      # the launch preamble: every stamp up to the first stage-1 panel, cycles after the kernel's start
            k1 = next((k for k, (_, tag) in enumerate(st) if tag == 0x14), len(st) - 1)
            print(f"  wave {w}: preamble " + " ".join(f"{tag:02x}@{t - t0}" for t, tag in st[:k1 + 1]))
