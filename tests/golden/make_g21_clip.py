"""Writes tests/golden/g21_clip.json: the NU checkpoint's less ratio and the largest |y| along the path with and without the x0 clip, on
the CPU (tests/clip_ref.py: the oracle's denoiser, decoder and evaluator).  Run from the repository root:
python tests/golden/make_g21_clip.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _util  # noqa: E402,F401  (puts the repository root and tests/golden on sys.path)
import clip_ref as C  # noqa: E402


def main():
    cells = {k: {"plain": round(v["plain"], 6), "clip": round(v["clip"], 6), "max_plain": float(f"{v['max_plain']:.4g}"),
                 "max_clip": float(f"{v['max_clip']:.4g}")} for k, v in C.nu_cells().items()}
    out = {"what": "less ratio of the NU checkpoint (g4_sample_nu_ckpt.npz: 512 rows, T = 20, its own y_T and z) without (plain) and with "
                   "(clip) the x0 clip, and the largest |y| after any step of the path, computed on the CPU by tests/clip_ref.py (float32 "
                   "oracle).  `settings`: plan kind, K, eta, omega, early renormalised steps, bounds (unit [0, 1]; wide [-0.25, 1.25]; "
                   "pooled25: the pooled range of the golden's y_test +- 25 %; feature100: its per-feature range +- 100 %)",
           "rows": 512, "T": 20,
           "settings": {c[0]: list(c[1:]) for c in C.NU_CELLS},
           "cells": cells}
    with open(os.path.join(HERE, "g21_clip.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for k, v in cells.items():
        print(f"{k}: {v}")


if __name__ == "__main__":
    main()
