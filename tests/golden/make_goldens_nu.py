#!/usr/bin/env python3
"""Generate tests/golden/g12_noma_uav_gen.npz (G12: the NU label generator) by importing the reference itself.

Runs ONLY where the reference tree is available; the output is committed and the tests read nothing else.

    python tests/golden/make_goldens_nu.py REFERENCE_ROOT      (or DIFFSG_REFERENCE=REFERENCE_ROOT in the environment)

Contents, per total power P in (18, 30, 6):
  P<P>_seed, P<P>_out      np.random.seed(seed); noma_uav_gen(n, P)  -> [n][12] float64 (qs | x, y | powers | rate)
  P<P>_fs_shape, _fs_sha256, _fs_first, _fs_last    feasible_solution(P): shape, sha256 of its bytes, first and last rows
and ext_seed / ext_out: np.random.seed(ext_seed); dataset_extension(tests/golden/data/3u_18mW_200samples.csv).
"""
import hashlib
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DIFFSG_REFERENCE", "")
if not os.path.isfile(os.path.join(REF, "datasets", "noma_uav_gen.py")):
    sys.exit("usage: make_goldens_nu.py REFERENCE_ROOT (the tree that holds datasets/noma_uav_gen.py)")
sys.path.insert(0, os.path.join(REF, "datasets"))

import noma_uav_gen as R  # noqa: E402

CASES = ((18.0, 1234, 12), (30.0, 4321, 3), (6.0, 99, 4))
EXT_SEED = 7


def main():
    out = {}
    for P, seed, n in CASES:
        tag = f"P{int(P)}"
        fs = R.feasible_solution(P)
        out[tag + "_fs_shape"] = np.array(fs.shape, dtype=np.int64)
        out[tag + "_fs_sha256"] = np.array(hashlib.sha256(np.ascontiguousarray(fs).tobytes()).hexdigest())
        out[tag + "_fs_first"], out[tag + "_fs_last"] = fs[0].copy(), fs[-1].copy()
        t0 = time.time()
        np.random.seed(seed)
        out[tag + "_seed"] = np.array(seed, dtype=np.int64)
        out[tag + "_out"] = R.noma_uav_gen(n, P)
        print(f"{tag}: {n} samples, {fs.shape[0]} solutions, {time.time() - t0:.1f} s", flush=True)
    np.random.seed(EXT_SEED)
    out["ext_seed"] = np.array(EXT_SEED, dtype=np.int64)
    out["ext_out"] = R.dataset_extension(os.path.join(HERE, "data", "3u_18mW_200samples.csv"))
    path = os.path.join(HERE, "g12_noma_uav_gen.npz")
    np.savez_compressed(path, **out)
    print(f"wrote g12_noma_uav_gen.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()
