"""Writes tests/golden/g18_multistep.json: the NU checkpoint's less ratio under DDIM eta = 0 and under the two-step rule, on the CPU
(tests/multistep_ref.py: the oracle's denoiser, decoder and evaluator).  Run from the repository root:
python tests/golden/make_g18_multistep.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _util  # noqa: E402,F401  (puts the repository root and tests/golden on sys.path)
import multistep_ref as M  # noqa: E402


def main():
    out = {"what": "less ratio of the NU checkpoint (g4_sample_nu_ckpt.npz: 512 rows, T = 20, omega = 500, its own y_T; both rules are noise "
                   "free) on K-step plans of the default grid with `renorm` early renormalised steps: DDIM eta = 0 (ddim0) against "
                   "DPM-Solver++(2M) (2m), computed on the CPU by tests/multistep_ref.py (float32 oracle).  Key: K<K>_r<renorm>_<rule>",
           "omega": 500.0, "rows": 512, "T": 20,
           "ratios": {k: round(v, 6) for k, v in M.nu_cells().items()}}
    with open(os.path.join(HERE, "g18_multistep.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for k, v in out["ratios"].items():
        print(f"{k}: {v:.6f}")


if __name__ == "__main__":
    main()
