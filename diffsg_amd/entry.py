"""What the entry points of the three problem modules (classifier_free_{MSR,CO,NU}.py) and of trajectory.py share: the device, the
checkpoint, the training set-up, the reference's evaluation loop and the refusal of sampler options.  A problem module keeps what is its
own: the data loader, `build_model`, unscaling, the decoder and the objective, the metrics and their log lines.

The sampler options of `load_test_msr`, `load_test_co` and `load_test_nu`, beyond the reference's arguments:
  repeats   > 1: that many draws per test row, the one with the best objective scored (DDPM.sample_best); 1 is the reference's single draw.
  steps     = K: sample on K of the T trained steps (`steps.strided`, or `steps.ddim` with `sampler="ddim"` and `eta`, or
            `steps.dpmpp_2m` with `sampler="dpmpp2m"`: the two-step rule of DESIGN.md 18); None: all T, as the reference.  A variant's
            plan must not carry a history table (a `dpmpp_2m` plan): the per-chunk form of the update has none.
  variants  a list of (omega, plan) sampler settings cycled over the `repeats` rounds (round r runs variants[r % len(variants)],
            DDPM.sample_best); `omega` and `steps` / `sampler` / `eta` stay the single-setting spelling and are not read then.
            A plan of a variant may carry a guidance schedule (`steps.with_guidance(plan_or_model, g)`, DESIGN.md 16: step j guided with
            omega * g_j, one denoiser pass where g_j == 0); the variants of one call share it.  The entry points have no keyword of their
            own for it: their signatures are pinned.
  clip      no keyword either: `with steps.clipping(lo, hi):` or `with steps.clipping(margin=m):` around the call.  Inside
            the context the single-setting plan (the identity plan for `steps=None`) and every variant plan without a clip of its own
            sample under the clip; with `margin` the bounds are `steps.clip_bounds` of the loader's own training labels.
"""
from __future__ import annotations

import torch

from .steps import clipping     # `entry.clipping` is `steps.clipping`: the context the entry points read through `clipped`


def device():
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device: this build of DiffSG has no CPU path")
    return torch.device("cuda:0")


def load_checkpoint(model, ckpt_path, device):
    """`model` with the state dict stored at `ckpt_path`, on `device`."""
    model.load_state_dict(torch.load(ckpt_path, map_location="cpu"))
    return model.to(device)


def check_variants(variants, repeats):
    if variants is not None and repeats < 2:
        raise ValueError("variants are settings of repeated sampling: pass repeats >= 2")


def clipped(model, plan, variants, Y_train):
    """`plan` and `variants` of a `load_test_*` call under the enclosing `steps.clipping()` context, unchanged outside one: the
    single-setting plan (the identity plan for None) with the context's clip, and every variant plan that carries none with it too.
    `Y_train`: the loader's training labels, read for `clipping(margin=...)` alone."""
    from . import steps
    bounds = steps.active_clip(Y_train)
    if bounds is None:
        return plan, variants
    ident = steps.with_clip(model, *bounds)        # built once: the variants without a plan share its tensors
    plan = ident if plan is None else steps.with_clip(plan, *bounds)
    if variants is not None:
        clip = plan.clip
        def one(p):
            if p is None:
                return ident
            return p if p.clip is not None else steps.StepPlan(p.taus, p.t, p.coef, p.renorm_steps, p.guidance, p.history, clip)
        variants = [(o, one(p)) for o, p in variants]
    return plan, variants


def sample_in_batches(model, X, omega, batch_size, plan=None):
    """The reference's loop of independent `batch_size`-row sample() calls over the rows of `X` (own noise, own early-step renorm per
    chunk; classifier_free_MSR.py:273-279), run as one set of launches; chunk sizes that are not a multiple of the 32-row tile keep the
    serial calls."""
    dev = next(model.model.parameters()).device
    if batch_size % 32 == 0:
        return model.sample_chunked(X.to(dev), omega, batch_size, plan=plan)
    return torch.cat([model.sample(X[i:i + batch_size].to(dev), omega, plan=plan) for i in range(0, len(X), batch_size)])


def train_ddpm(problem, *args, graph=False, seed=None, **kw):
    """`train_ddpm_msr` / `train_ddpm_co` / `train_ddpm_nu` (`problem` = "msr", "co", "nu") with their own arguments and defaults, plus the
    two options of `train`: `graph=True` trains from device-resident batches through the captured step graph, `seed` seeds its shuffling
    and device-side draws.  The three functions keep the reference's signatures (tests/test_entry_cpu.py pins them), so the options live
    here; `graph=False` is the function's own call."""
    import importlib
    import inspect
    if problem not in ("msr", "co", "nu"):
        raise ValueError(f"train_ddpm: problem must be 'msr', 'co' or 'nu', not {problem!r}")
    mod = importlib.import_module(f".classifier_free_{problem.upper()}", __package__)
    bound = inspect.signature(getattr(mod, f"train_ddpm_{problem}")).bind(*args, **kw)
    bound.apply_defaults()
    return mod._train(*bound.arguments.values(), graph=graph, seed=seed)


def train(build, X_train, Y_train, lr, milestones, epochs, use_ema, warmup_epoch, batch_size, log, graph=False, seed=None):
    """The training run of the three scripts (classifier_free_MSR.py:187-236, hot loop :217-234) on the model `build(device)` returns.

    `graph=True` (opt-in; `train.run_epochs(graph=True)`): the training set lives on the device (`train.DeviceBatches`, shuffled per epoch
    from `seed`), ts / noise / mask are drawn on the device (`device_draws = seed`, default 0 -- not torch's generator) and every step is a
    replay of the captured step graph; the epoch loss is read, and the step health checked, once per epoch.  Data-parallel runs keep the
    eager loop and say so."""
    import torch.optim as optim
    import torch.utils.data as data
    from .diffusion import init_weights
    from .train import DeviceBatches, FlatAdam, dp_context, make_loader, run_epochs, sync_replicas
    dataset = data.TensorDataset(torch.tensor(X_train, dtype=torch.float32), torch.tensor(Y_train, dtype=torch.float32))
    dev, rank, world = dp_context()         # one process per GPU when launched under torch.distributed.run; else cuda:0
    if graph and world > 1:
        if rank == 0:
            log(f"graph=True: {world} processes train data parallel, which keeps the eager loop (one all-reduce per step)")
        graph = False
    loader = None if graph else make_loader(dataset, batch_size, rank, world)
    if dev is None:
        dev = device()                      # raises: no CPU path
    diffusion_model = build(dev)
    from . import timesteps
    timesteps.apply_active(diffusion_model)     # the options of an enclosing timesteps.training(law=..., report=...); nothing outside one
    diffusion_model.apply(init_weights)
    diffusion_model.to(dev)
    sync_replicas(diffusion_model)          # data parallel: rank 0's initial weights everywhere (no-op for one process)
    optimizer = FlatAdam(diffusion_model, lr=lr)  # torch Adam, same update rule, over one flat tensor (one launch)
    scheduler = optim.lr_scheduler.MultiStepLR(optimizer, list(milestones))
    if graph:
        diffusion_model.device_draws = 0 if seed is None else int(seed)
        batches = DeviceBatches(*dataset.tensors, batch_size, diffusion_model.device_draws, dev)
        run_epochs(diffusion_model, None, optimizer, scheduler, epochs, use_ema, warmup_epoch, dev, log, graph=True, batches=batches)
        return diffusion_model
    run_epochs(diffusion_model, loader, optimizer, scheduler, epochs, use_ema, warmup_epoch, dev, log)
    return diffusion_model
