#!/usr/bin/env python3
"""Wall time of one training epoch of the entry points' loop (`train.run_epochs`) in three forms:
    python tools/train_epoch_speed.py [out.txt] [--eager-only] [--limit SECONDS]
One GPU, one process.  `msr80`, `co3` and `nu3` as `train_ddpm_{msr,co,nu}` build them, at the reference's shapes: 7 000 rows (70 % of
10 000), batch 512 (13 full batches and one of 344 rows), T = 20, weights from `init_weights`, synthetic data.
  (a) eager, DataLoader   the loop as the entry points run it by default: `make_loader` (512 per-sample fetches and a collate per batch on
                          the host), torch's generator for the draws, `loss.item()` and the health check per step;
  (b) eager, device data  the same loop fed from `train.DeviceBatches` (two index_select per batch), device-side draws;
  (c) graph               `run_epochs(graph=True)`: one graph replay per full batch, the ragged batch eager, one synchronise per epoch.
Per form 9 epochs in ONE `run_epochs` call; an epoch's time is the host wall time between two of its log lines (each follows a
synchronise); the first 2 are warm-up (workspaces, the capture), the median (min .. max) of the other 7 is reported.  The box probe
(dsg_box_calibrate) before and after.  `--eager-only` times (a) alone: that runs on a tree without DeviceBatches too, for the PARENT
commit's time on the same box (copy this file into a checkout of the parent, or use it from tools/tree_ab.sh's ab_old/).  The run stops
at the first form that raises, and after `--limit` seconds (default 420) it starts no further form.  Writes the table to `out.txt`
(default profiles/train_epoch_speed.txt) and prints it."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench import box_calibrate  # noqa: E402

ROWS, BATCH, T, WARM, TIMED = 7000, 512, 20, 2, 7


def build(net, dev):
    from diffsg_amd import classifier_free_CO as CO, classifier_free_MSR as MSR, classifier_free_NU as NU
    from diffsg_amd.diffusion import init_weights
    torch.manual_seed(1)
    d = {"msr80": lambda: MSR.build_model(80, 80, dev, T, None, 20.0), "co3": lambda: CO.build_model(3, 9, dev, T, None),
         "nu3": lambda: NU.build_model(3, 18.0, dev, T, {"width": 400, "height": 400})}[net]()
    d.apply(init_weights)
    return d.to(dev)


def epoch_times(net, form, dev):
    """[ms] of the 9 epochs of one run_epochs call in `form`."""
    import torch.optim as optim
    import torch.utils.data as data
    from diffsg_amd import train as tr
    d = build(net, dev)
    cfg = d.model.cfg
    g = torch.Generator().manual_seed(7)
    X, Y = torch.rand(ROWS, cfg["cond_dim"], generator=g), torch.rand(ROWS, cfg["input_dim"], generator=g) * 0.25
    opt = tr.FlatAdam(d, lr=1e-4)              # (the reference's 5e-3 drives a fresh net on random targets out of the fp16 range in 2 epochs)
    sched = optim.lr_scheduler.MultiStepLR(opt, [100, 150])
    stamps = []
    log = lambda _line: stamps.append(time.perf_counter())
    args = (opt, sched, WARM + TIMED, False, 5, dev, log)
    torch.cuda.synchronize()
    stamps.append(time.perf_counter())
    if form == "a":
        tr.run_epochs(d, tr.make_loader(data.TensorDataset(X, Y), BATCH), *args)
    else:
        d.device_draws = 0
        tr.run_epochs(d, None, *args, graph=form == "c", batches=tr.DeviceBatches(X, Y, BATCH, 0, dev))
    torch.cuda.synchronize()
    return [(b - a) * 1e3 for a, b in zip(stamps, stamps[1:])]


def main():
    argv = sys.argv[1:]
    limit = float(argv[argv.index("--limit") + 1]) if "--limit" in argv else 420.0
    args = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--limit")]
    forms = [("a", "(a) eager, DataLoader")] + ([] if "--eager-only" in argv else [("b", "(b) eager, device data"), ("c", "(c) graph")])
    path = args[0] if args else os.path.join(ROOT, "profiles", "train_epoch_speed.txt")
    dev = torch.device("cuda:0")
    t_start = time.perf_counter()
    lines = [f"device: {torch.cuda.get_device_name(0)}", f"box before: {box_calibrate()}",
             f"{ROWS} rows, batch {BATCH} ({-(-ROWS // BATCH)} steps per epoch), T = {T}; ms per epoch: median (min .. max) of {TIMED} epochs "
             f"after {WARM} warm-up epochs; ms per step = median / steps",
             f"{'net':<8}{'form':<26}{'ms per epoch':>34}{'ms per step':>14}"]
    steps = -(-ROWS // BATCH)
    for net in ("msr80", "co3", "nu3"):
        for form, tag in forms:
            if time.perf_counter() - t_start > limit:
                lines.append(f"{net:<8}{tag:<26} not started: the time limit of {limit:g} s was reached")
                print(lines[-1], flush=True)
                continue
            ms = epoch_times(net, form, dev)[WARM:]          # an exception ends the run here: nothing further is started on the GPU
            med = statistics.median(ms)
            lines.append(f"{net:<8}{tag:<26}{med:>14.2f} ({min(ms):.2f} .. {max(ms):.2f}){med / steps:>14.3f}")
            print(lines[-1], flush=True)
    lines.append(f"box after: {box_calibrate()}")
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(txt)
    print(txt)


if __name__ == "__main__":
    main()
