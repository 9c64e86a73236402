"""Writes tests/golden/g19_guidance.json: the NU checkpoint under guidance masks, on the CPU (tests/guidance_ref.py: the oracle's
denoiser, decoder and evaluator).  Run from the repository root: python tests/golden/make_g19_guidance.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _util  # noqa: E402,F401  (puts the repository root and tests/golden on sys.path)
import guidance_ref as GR  # noqa: E402
import variants_ref as VR  # noqa: E402

SEEDS = tuple(range(101, 109))
ROWS = 512


def ratio(rate):
    return float(rate.sum() / VR.label_rate(ROWS).sum())


def best(rates):
    import torch
    return float(torch.stack(rates).max(dim=0).values.sum() / VR.label_rate(ROWS).sum())


def cells(row, K, omega=500.0):
    """single rounds of the first four seeds, best-of-8 with 4 renorm steps, best-of-8 with the renorm count cycled"""
    same = [GR.nu_round_rate(s, omega, min(K, 4), K, ROWS, row) for s in SEEDS]
    cyc = [GR.nu_round_rate(s, omega, VR.RENORM_CYCLE[r % len(VR.RENORM_CYCLE)], K, ROWS, row) for r, s in enumerate(SEEDS)]
    single = [ratio(x) for x in same[:4]]
    return {"passes": GR.passes_of(row, K), "single_mean": round(sum(single) / 4, 6), "single_min": round(min(single), 6),
            "single_max": round(max(single), 6), "best8_same": round(best(same), 6), "best8_renorm": round(best(cyc), 6)}


def main():
    out = {"what": "NU checkpoint (g4_sample_nu_ckpt.npz) on its 512 rows, less ratio (sum of rates / sum of the stored labels' rates) under a "
                   "guidance mask: a step whose weight is 0 runs the conditional denoiser pass alone.  Rounds draw y_T = randn(rows, 5) then "
                   "z = randn(K-2, rows, 5) from torch.Generator().manual_seed(seed); computed on the CPU by tests/guidance_ref.py (float32 oracle)",
           "rows": ROWS, "T": 20, "omega": 500.0, "seeds": list(SEEDS), "renorm_cycle": list(VR.RENORM_CYCLE)}
    out["T20"] = {row: cells(row, 20) for row in GR.TABLE_MASKS}
    out["golden_inputs"] = {row: round(GR.nu_golden_cell(row), 6) for row in ("all", "interval5_14", "even", "odd", "none")}
    out["omega50_single_seed101"] = {row: round(ratio(GR.nu_round_rate(101, 50.0, 4, 20, ROWS, row)), 6)
                                     for row in ("all", "first_quarter_off", "interval5_14", "even", "third")}
    out["K10ddim0"] = {row: cells(row, 10) for row in ("all", "even")}
    out["pinned"] = {"rows": GR.PIN_ROWS, "all": round(GR.nu_golden_cell("all", GR.PIN_ROWS), 6), "even": round(GR.nu_golden_cell("even", GR.PIN_ROWS), 6)}
    with open(os.path.join(HERE, "g19_guidance.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
