"""Writes tests/golden/g18_variants.json: best-of-n over sampler settings on the NU checkpoint, on the CPU (tests/variants_ref.py: the
oracle's denoiser, decoder and evaluator).  Run from the repository root: python tests/golden/make_g18_variants.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _util  # noqa: E402,F401  (puts the repository root and tests/golden on sys.path)
import variants_ref as VR  # noqa: E402

SEEDS_A, SEEDS_B = tuple(range(101, 117)), tuple(range(11, 19))


def main():
    table = {}
    for row in ("same", "renorm", "renorm+omega"):
        for n in (4, 8, 16):
            table[f"T20_{row}_n{n}"] = VR.best_of_ratio(row, SEEDS_A[:n], 20)
    for row in ("same", "renorm"):
        for n in (8, 16):
            table[f"K10ddim0_{row}_n{n}"] = VR.best_of_ratio(row, SEEDS_A[:n], 10)
    for row in ("same", "omega", "renorm"):
        table[f"T20_{row}_n8_seeds11"] = VR.best_of_ratio(row, SEEDS_B, 20)
    single = [float(VR.nu_round_rate(s, om, rn, 20, 512).sum() / VR.label_rate(512).sum())
              for s in SEEDS_A[:4] for om in VR.OMEGA_CYCLE for rn in VR.RENORM_CYCLE]
    pinned = {"rows": VR.PIN_ROWS, "seeds": list(VR.PIN_SEEDS),
              "same": VR.best_of_ratio("same", VR.PIN_SEEDS, 20, VR.PIN_ROWS), "renorm": VR.best_of_ratio("renorm", VR.PIN_SEEDS, 20, VR.PIN_ROWS)}
    out = {"what": "NU checkpoint (g4_sample_nu_ckpt.npz), T = 20: sum over the rows of the best round's rate / sum of the stored labels' rate; round r "
                   "draws y_T = randn(rows, 5) then z = randn(K-2, rows, 5) from torch.Generator().manual_seed(seeds[r]) and runs "
                   "variants_ref.round_setting(row, r); computed on the CPU by tests/variants_ref.py (float32 oracle)",
           "rows": 512, "T": 20, "seeds": list(SEEDS_A), "seeds11": list(SEEDS_B), "renorm_cycle": list(VR.RENORM_CYCLE),
           "omega_cycle": list(VR.OMEGA_CYCLE), "ratios": {k: round(v, 6) for k, v in table.items()},
           "single_round_min_max": [round(min(single), 6), round(max(single), 6)],
           "pinned": {k: (round(v, 6) if isinstance(v, float) else v) for k, v in pinned.items()}}
    with open(os.path.join(HERE, "g18_variants.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for k, v in out["ratios"].items():
        print(k, v)
    print(out["single_round_min_max"], out["pinned"])


if __name__ == "__main__":
    main()
