#!/usr/bin/env python3
"""Wall time of chunked sampling with and without chunk variants: python tools/variants_speed.py [out.txt] [--no-variants]
One GPU, one process.  Two shapes, each a 16-chunk call of 512-row chunks (8 192 rows):
  nu3   the shipped NU checkpoint, T = 20, omega = 500: 16 rounds x 512 rows, the shape of `sample_best(cond, X, 16)`;
  msr3  BASELINE config 2's shape: MSR-3c net, T = 1000, omega = 1.
Per shape: the uniform `sample_chunked` call, the variants call of the same shape (renorm count cycled over five values and omega over four:
every chunk another setting), and on nu3 `sample_best` over 16 rounds without and with variants.  Median of 7 timed calls after
2 warm-up calls (host wall time around call + synchronise; range check off: the call only enqueues).  The box probe (dsg_box_calibrate)
before and after.  `--no-variants` times the variant-less calls only: that runs on a tree without chunk variants too, for the parent
commit's times on the same box.  Writes the table to `out.txt` (default profiles/variants_speed.txt) and prints it."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch  # noqa: E402

from bench import box_calibrate  # noqa: E402

ROUNDS, ROWS = 16, 512
RENORM = {"nu3": (4, 0, 2, 1, 3), "msr3": (4, 5, 6, 8, 16)}     # (synthetic msr3 weights leave the fp16 range with fewer than 4 renorm steps)


def build(net):
    import steps_ref as R
    from _util import synth_params
    from oracle import ddpm_oracle as O
    from weights import CONFIGS
    from diffsg_amd import UNet1D
    from diffsg_amd import classifier_free_MSR as MSR, classifier_free_NU as NU
    cfg = CONFIGS[net]
    p = R.net_params("nu3")[1] if net == "nu3" else synth_params("msr3", 7)[1]
    m = UNet1D(**cfg, is_attn=(False,) * len(cfg["dims"]))
    m.load_state_dict(p)
    dev = torch.device("cuda")
    if net == "nu3":
        T = 20
        return NU.DDPM(T, m.to(dev), 3, 18.0, 1.0 - O.cosine_betas(T), dev, (1, 5), {"width": 400, "height": 400}).to(dev)
    T = 1000
    return MSR.DDPM(T, m.to(dev), 3, 10.0, 1.0 - O.cosine_betas(T), dev, (1, 3), None).to(dev)


def median_ms(fn, warmup=2, calls=7):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    variants = "--no-variants" not in sys.argv
    path = args[0] if args else os.path.join(ROOT, "profiles", "variants_speed.txt")
    lines = [f"device: {torch.cuda.get_device_name(0)}", f"box before: {box_calibrate()}",
             f"{ROUNDS} chunks x {ROWS} rows, graph; median (min .. max) ms of 7 calls after 2 warm-up calls",
             f"{'call':<44}{'ms per call':>34}"]

    def row(tag, fn):
        try:
            med, lo, hi = median_ms(fn)
            lines.append(f"{tag:<44}{med:>14.3f} ({lo:.3f} .. {hi:.3f})")
        except RuntimeError as e:          # an unchecked call that left the fp16 range raises at the next entry point
            lines.append(f"{tag:<44} raised: {str(e)[:120]}")
        print(lines[-1], flush=True)

    seeds = list(range(101, 101 + ROUNDS))
    for net, omega, omegas in (("nu3", 500.0, (500.0, 200.0, 2000.0, 50.0)), ("msr3", 1.0, (1.0, 0.5, 0.75, 0.25))):
        ddpm = build(net)
        C = ddpm.model.cfg["cond_dim"]
        cond = torch.rand(ROWS, C, generator=torch.Generator().manual_seed(0)).cuda()
        big = cond.repeat(ROUNDS, 1)
        X = cond * 400.0
        vs = None
        if variants:
            from diffsg_amd import steps
            vs = [(omegas[r % len(omegas)], steps.with_renorm(ddpm, RENORM[net][r % 5])) for r in range(ROUNDS)]
        tag = f"{net} T={ddpm.T}"
        row(f"{tag} sample_chunked uniform", lambda: ddpm.sample_chunked(big, omega, ROWS, seeds=seeds, check_range=False))
        if variants:
            row(f"{tag} sample_chunked variants", lambda: ddpm.sample_chunked(big, omega, ROWS, seeds=seeds, check_range=False, variants=vs))
            row(f"{tag} sample_chunked uniform again", lambda: ddpm.sample_chunked(big, omega, ROWS, seeds=seeds, check_range=False))
        if net == "nu3":
            row(f"{tag} sample_best n=16 uniform", lambda: ddpm.sample_best(cond, X, ROUNDS, omega, seeds=seeds, check_range=False))
            if variants:
                row(f"{tag} sample_best n=16 variants", lambda: ddpm.sample_best(cond, X, ROUNDS, seeds=seeds, check_range=False, variants=vs[:5]))
                # plain and variants calls alternating on one handle: each form replays its own graphs
                def both():
                    ddpm.sample(cond, omega, seed=1, check_range=False)
                    ddpm.sample_best(cond, X, ROUNDS, seeds=seeds, check_range=False, variants=vs[:5])
                row(f"{tag} sample() + sample_best variants", both)
                row(f"{tag} sample() alone", lambda: ddpm.sample(cond, omega, seed=1, check_range=False))
        ddpm.model.range_exceeded()
    lines.append(f"box after: {box_calibrate()}")
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(txt)
    print(txt)


if __name__ == "__main__":
    main()
