"""Host side of the training step (reference hot loop: classifier_free_MSR.py:217-234, = CO.py:233-250, NU.py:245-262).

`run_epochs` is the reference's epoch loop; the per-batch arithmetic (q_sample, denoiser forward and backward, MSE)
is DDPM.forward -> libdiffsg_hip.so.  Adam and MultiStepLR stay PyTorch objects (not part of the path).
With torch.distributed initialised, gradients of `model.*` are averaged over ranks with ONE all-reduce per step over a
flat float32 bucket (RCCL over xGMI on MI355X; gloo in the CPU tests); `ema.module.*` never receives gradients and is
not communicated.
"""
from __future__ import annotations

import torch


def flatten_parameters(unet):
    """Re-point every parameter of `unet` at a slice of ONE flat float32 tensor (state-dict order = the order of the
    gradient bucket, `DDPM.grad_bucket`) and return that tensor.  `state_dict()` / `load_state_dict()` are unchanged: the
    parameters are still separate `nn.Parameter`s, they only share storage."""
    params = list(unet.parameters())
    flat = torch.empty(sum(p.numel() for p in params), device=params[0].device, dtype=params[0].dtype)
    off = 0
    for p in params:
        n = p.numel()
        flat[off:off + n].copy_(p.data.reshape(-1))
        p.data = flat[off:off + n].view_as(p)
        off += n
    if hasattr(unet, "mark_weights_changed"):
        unet.mark_weights_changed(rebuild=True)    # new storage behind the same Parameter objects
    return flat


class FlatAdam(torch.optim.Adam):
    """torch.optim.Adam (the reference's optimizer, classifier_free_MSR.py:209) applied to the model's parameters as ONE
    flat tensor whose gradient is the flat bucket written by dsg_train_step: the update is elementwise, so it is the same
    arithmetic as Adam over the ~330 separate tensors, in one kernel launch instead of one multi-tensor launch per chunk
    of tensors.  A torch `Optimizer`, so MultiStepLR drives it as it drives the reference's."""

    native_step = True       # False: torch's own fused kernel (A/B measurements, tools/train_ab.py)

    def __init__(self, diffusion_model, lr=1e-3, **kw):
        self._ddpm = diffusion_model
        self._flat = torch.nn.Parameter(flatten_parameters(diffusion_model.model))
        kw.setdefault("fused", True)
        super().__init__([self._flat], lr=lr, **kw)

    @torch.no_grad()
    def step(self, closure=None):
        bucket = self._ddpm.grad_bucket
        if bucket is None or not getattr(self._ddpm, "_grads_ready", False) or self._ddpm.model.param_list()[0].grad is None:
            return None                    # no backward since the last zero_grad
        self._flat.grad = bucket
        group = self.param_groups[0]
        plain = (self.native_step and closure is None and len(self.param_groups) == 1 and not group.get("amsgrad") and not group.get("capturable")
                 and not group.get("differentiable") and not torch.is_tensor(group["lr"]) and self._flat.is_cuda)
        if not plain:
            st = self.state.get(self._flat)
            if st and group.get("fused") and not st["step"].is_cuda:
                st["step"] = st["step"].to(self._flat.device)       # torch's fused kernel counts on the device
            out = super().step(closure)    # torch's own kernels for the variants dsg_adam_step does not cover
        else:
            # torch's fused kernel hands a block 65 536 elements of a tensor: the one flat tensor runs on 26 workgroups (45 us for 6.6 MB);
            # dsg_adam_step is the same arithmetic element for element (bit-identical to torch.optim.Adam(fused=True)) as a grid-wide loop, and the
            # step count stays on the host (no `_foreach_add_` launch for it)
            from . import _lib
            st = self.state[self._flat]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(self._flat, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(self._flat, memory_format=torch.preserve_format)
            if st["step"].is_cuda:         # a state loaded from a fused-Adam checkpoint: keep counting on the host
                st["step"] = st["step"].detach().cpu()
            st["step"] += 1
            b1, b2 = group["betas"]
            dyn = getattr(self, "_dyn", None)          # StepGraph: learning rate and step count in device memory
            with torch.cuda.device(self._flat.device):
                if dyn is not None:
                    _lib.check(_lib.lib().dsg_adam_step_dyn(_lib.ptr(self._flat), _lib.ptr(bucket), _lib.ptr(st["exp_avg"]), _lib.ptr(st["exp_avg_sq"]),
                                                            self._flat.numel(), _lib.ptr(dyn["lr"]), float(b1), float(b2), float(group["eps"]),
                                                            float(group["weight_decay"]), int(bool(group.get("maximize"))), _lib.ptr(dyn["step"]),
                                                            _lib.stream_ptr()))
                else:
                    _lib.check(_lib.lib().dsg_adam_step(_lib.ptr(self._flat), _lib.ptr(bucket), _lib.ptr(st["exp_avg"]), _lib.ptr(st["exp_avg_sq"]),
                                                        self._flat.numel(), float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                                                        float(group["weight_decay"]), int(bool(group.get("maximize"))), int(st["step"].item()),
                                                        _lib.stream_ptr()))
            out = None
        self._ddpm.model.mark_weights_changed()   # in-place update through an alias: the per-parameter versions do not move
        return out

    def zero_grad(self, set_to_none=False):
        """Default: ONE fill of the flat bucket; the per-parameter `.grad` views stay installed and read zero (torch's
        `set_to_none=False` semantics) - re-creating ~500 views and `.grad` assignments per step costs more host time than
        the step's launch sequence at the reference's batch of 512.  `set_to_none=True` drops them as torch does."""
        self._flat.grad = None
        self._ddpm._grads_ready = False
        bucket = self._ddpm.grad_bucket
        if not set_to_none:
            if bucket is not None:
                bucket.zero_()
            return
        for p in self._ddpm.model.param_list():
            p.grad = None


class StepGraph:
    """One whole training step -- device-side draws, q_sample + denoiser forward + backward (dsg_train_step_seeded_dyn), Adam
    (dsg_adam_step_dyn), zero_grad, the re-pack of the updated weights -- captured ONCE as a HIP graph and replayed per step (reference
    loop body: classifier_free_MSR.py:220-232, the same shape every step).  Per step the host then issues one graph launch instead of ~70
    kernel launches, a dozen torch ops and the ctypes marshalling around them (0.87 ms of host time per 1.8 ms step before; VERDICT r5,
    next 4).  What changes from step to step lives in DEVICE memory and is moved on by the graph itself: the Philox call number of the
    draws and Adam's step count; the learning rate is a device scalar the host rewrites when a scheduler changes it.  The replayed
    kernels are the eager step's, on the same operands: weights after k replays == weights after k eager steps, bit for bit
    (tests/test_gpu_parity.py::test_graph_train_step_is_the_eager_step_bit_for_bit).

    Contract: `y` and `cond` are STATIC buffers -- copy each batch into them (`graph.y.copy_(batch)`); single process (a captured RCCL
    all-reduce is not used here: data-parallel runs keep the eager loop); requires `diffusion_model.device_draws` (the reference's torch
    generator cannot be replayed from a graph) and a FlatAdam on its native path; batches below `DDPM.train_split_min_rows`.  `loss` is the
    static loss tensor of the last replay.  The EMA update of the reference loop (ema.py, gated off in every shipped script) stays outside:
    call `ema.update_parameters` between replays if it is on.

    Other calls on the model may come between two `step()` calls -- sampling, an eager forward, a settings call, a host-side change of the
    weights -- and every `step()` is still ONE step of the same sequence: weights, Adam's state, `_draw_calls` and the device counters after N
    calls are those of N eager steps, bit for bit.
      * What invalidates the capture.  The captured launches hold addresses inside the handle's workspaces, the launch plan of capture time and
        the per-batch-size tables of the training step.  The handle counts every event that makes one of them stale (`dsg_generation`,
        include/diffsg.h): a workspace that grows (a `sample()` over more rows than the batch, another T), `set_precision`,
        `set_launch_policy`, `set_option` with another value, a training step of another batch size on the same handle.  The count (of the
        primary handle and of every twin handle alive at capture time) is recorded after the capture and compared in `step()`.
      * What re-captures.  When the count has moved the stale graph is dropped WITHOUT being replayed, the step runs eagerly on the dyn path
        (the same kernels on the same device counters: the sequence does not notice; it is also what re-creates the workspaces), and the graph
        is captured again behind it.  `recaptures` counts these; `eager_steps` the steps that did not come from a replay.
      * Host-side weight changes (`load_state_dict`, a broadcast, an EMA copy, `mark_weights_changed`): the captured re-pack sits at the END of
        the graph, so `step()` calls `model.native_handle()` before the replay -- nothing when the bound key is unchanged, an eager re-pack
        otherwise.  Replays and `close()` move the twin handles' epoch: a twin re-binds on its next use.
      * A capture that fails leaves nothing behind: `_draw_calls` and Adam's step count are put back, the counters return to the host
        (`optimizer._dyn = None`, `diffusion_model._call_dev = None`), and the exception is raised again.  The steps made before it stand.
      * `warmup=0` captures lazily: nothing runs in the constructor, the first `step()` is a real eager step on the caller's data and the
        capture follows it (with `warmup >= 1` the constructor makes that many real steps on whatever `y` / `cond` hold).
      * `step_on(y, cond)` is one eager step of the same sequence on ANOTHER batch (the ragged last batch of an epoch).  A batch of another
        size runs on a twin handle of the module -- its own workspace and tables, the same weights and kernels -- so the capture stays valid.
      * While the counters live on the device (between the capture and `close()`), `DDPM.forward` REFUSES a batch that would run as two
        halves (`DDPM.train_split_min_rows`): that path draws with a by-value call number and would leave the device counter behind its
        host mirror.  The call counter is checked against the 2^30 range of the Philox counter word on the host mirror."""

    def __init__(self, diffusion_model, optimizer, y, cond, warmup=3):
        if diffusion_model.device_draws is None:
            raise ValueError("StepGraph needs device-side draws: set diffusion_model.device_draws = <seed>")
        if not isinstance(optimizer, FlatAdam) or not FlatAdam.native_step:
            raise ValueError("StepGraph needs a FlatAdam on its native path")
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise ValueError("StepGraph is single-process: the data-parallel loop stays eager (one all-reduce per step)")
        if diffusion_model._splits(y.shape[0]):
            raise ValueError(f"StepGraph: a batch of {y.shape[0]} rows runs as two halves on two handles (DDPM.train_split_min_rows): "
                             "capture batches below that threshold")
        self.ddpm, self.opt, self.y, self.cond = diffusion_model, optimizer, y, cond
        self.graph, self.loss, self._held, self._lr_host = None, None, (), None
        self.replays = self.recaptures = self.eager_steps = 0
        if int(warmup) <= 0:
            return                             # lazy: the first step() is an eager step on the caller's data, the capture follows it
        dev = y.device
        # eager warm-up on a side stream (workspaces, descriptor tables, the side streams of the fused step, Adam's state), as torch's
        # capture rules ask; then the counters move to the device at their current values
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(int(warmup)):
                self._eager_step()
        torch.cuda.current_stream(dev).wait_stream(side)
        self._capture()

    def _capture(self):
        """Capture one step behind at least one eager step.  The counters move to the device at their current values the first time; a
        re-capture finds them there.  On failure everything is as before the attempt, on the host path."""
        d, opt, dev = self.ddpm, self.opt, self.y.device
        torch.cuda.synchronize(dev)
        st = opt.state[opt._flat]
        calls0, step0 = int(d._draw_calls), float(st["step"])
        self._lr_host = float(opt.param_groups[0]["lr"])
        if getattr(opt, "_dyn", None) is None or getattr(d, "_call_dev", None) is None:
            opt._dyn = {"lr": torch.tensor([self._lr_host], dtype=torch.float64, device=dev),
                        "step": torch.tensor([step0], dtype=torch.float32, device=dev)}
            d._call_dev = torch.tensor([calls0], dtype=torch.int64, device=dev)
        else:
            opt._dyn["lr"].fill_(self._lr_host)
        try:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                loss = self._eager_step()
        except BaseException:
            # the host ran the bookkeeping of a step the device never executed, and the dyn path's counters would disagree with nobody
            # watching: back to the host counters, at the values of the last executed step
            d._draw_calls = calls0
            st["step"].fill_(step0)
            opt._dyn = None
            d._call_dev = None
            opt._flat.grad = None
            d._grads_ready = False
            self.graph, self.loss, self._held = None, None, ()
            raise
        # the capture ran the bookkeeping of ONE step on the host (call number, step count) without executing it on the device: undo it
        d._draw_calls = calls0
        st["step"].fill_(step0)
        self.graph, self.loss = graph, loss
        self._held = self._generations()

    def _natives(self):
        m = self.ddpm.model
        return [m._native] + list(m.__dict__.get("_twins", {}).values())

    def _generations(self):
        from . import _lib
        L = _lib.lib()
        return tuple((n, n.handle, int(L.dsg_generation(n.handle))) for n in self._natives() if n.handle)

    def _stale(self):
        """Did anything the captured launches hold go away since the capture (dsg_generation of the handles alive then)?"""
        from . import _lib
        L = _lib.lib()
        return any(n.handle != hd or int(L.dsg_generation(hd)) != gen for n, hd, gen in self._held)

    def _touch_twins(self):
        for n in self._natives()[1:]:
            n.epoch += 1                       # the weights moved without the host seeing it: a twin re-binds (re-packs) on its next use

    def _before_step(self):
        if self.ddpm._draw_calls >> 30:
            raise RuntimeError("StepGraph: the call counter of the device-side draws is out of range (2^30)")
        # a replay does not pass through DDPM.forward: a law or a report set, changed or removed since the last step reaches the handles
        # here, and moves dsg_generation (the capture is then dropped and made again behind an eager step); nothing when unchanged
        self.ddpm._sync_train_settings()
        lr = float(self.opt.param_groups[0]["lr"])
        if getattr(self.opt, "_dyn", None) is not None and lr != self._lr_host:
            self.opt._dyn["lr"].fill_(lr)      # MultiStepLR moved it (once per milestone): a stream-ordered 8-byte write
            self._lr_host = lr

    def _eager_step(self, y=None, cond=None):
        loss = self.ddpm(self.y if y is None else y, self.cond if cond is None else cond)
        loss.backward()
        self.opt.step()
        self.opt.zero_grad()
        self.ddpm.model.native_handle()        # the re-pack of the updated weights belongs to the step (it would otherwise open the next one)
        return loss

    def step(self):
        """One training step on what `y` / `cond` hold; returns its loss tensor (the static one of the graph after a replay).  A replay where
        the capture is valid -- the host mirrors of the two counters then move with the device's --, else an eager step followed by a
        (re-)capture; see the class docstring."""
        self._before_step()
        if self.graph is not None and not self._stale():
            self.ddpm.model.native_handle()    # weights changed on the host since the last step: re-pack now (the graph's re-pack is at its end)
            self.graph.replay()
            self.ddpm._draw_calls += 1
            self.opt.state[self.opt._flat]["step"] += 1
            self.replays += 1
            self._touch_twins()
            return self.loss
        again = self.graph is not None
        self.graph, self.loss, self._held = None, None, ()      # never replayed again: its launches hold freed or rewritten memory
        loss = self._eager_step()              # a real step: the counters, on the device or not yet, move by themselves
        self.eager_steps += 1
        self._capture()
        self.recaptures += int(again)
        return loss

    __call__ = step

    def step_on(self, y, cond):
        """One EAGER step of the same sequence on another batch, e.g. the ragged last batch of an epoch; returns its loss.  With the
        counters on the device a batch of another size than the captured one runs on a twin handle of the module: the per-batch-size tables
        of the primary handle, which the captured launches read, stay as they are."""
        if self.ddpm._splits(y.shape[0]):
            raise ValueError(f"StepGraph.step_on: a batch of {y.shape[0]} rows runs as two halves (DDPM.train_split_min_rows)")
        self._before_step()
        twin = 1 if (self.graph is not None and y.shape[0] != self.y.shape[0]) else 0
        if twin:
            self._touch_twins()
        self.ddpm._step_twin = twin
        try:
            loss = self._eager_step(y, cond)
        finally:
            self.ddpm._step_twin = 0
        self.eager_steps += 1
        return loss

    def close(self):
        """Back to the eager loop: the counters continue on the host where the graph left them."""
        self.opt._dyn = None
        self.ddpm._call_dev = None
        self.graph, self.loss, self._held = None, None, ()
        self._touch_twins()


def dp_context(backend=None):
    """(device, rank, world) of this process for the train entry points.

    Single process: cuda:0 (the reference's `torch.device("cuda:0")`, classifier_free_MSR.py:196), rank 0 of 1.
    Launched one process per GPU (torch.distributed.run, or any launcher that sets RANK / LOCAL_RANK / WORLD_SIZE): the device
    is cuda:LOCAL_RANK and the process group is created here if the caller has not done it (backend "nccl" = RCCL over
    xGMI; tests pass "gloo").  Every rank then draws its own ts / noise / mask: the global generators are re-seeded with
    `initial_seed + rank` (torch's default seed is the same constant in every process)."""
    import os
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if dist.is_available() and dist.is_initialized():
        world = dist.get_world_size()
    if world > 1 and not dist.is_initialized():
        backend = backend or ("nccl" if torch.cuda.is_available() else "gloo")
        if backend == "nccl":
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        dist.init_process_group(backend)
    rank = dist.get_rank() if world > 1 else 0
    if torch.cuda.is_available():
        local = int(os.environ.get("LOCAL_RANK", "0")) if world > 1 else 0
        torch.cuda.set_device(local)
        device = torch.device("cuda", local)
    else:
        device = None                       # the caller raises: there is no CPU path for the compute
    if world > 1:
        torch.manual_seed(torch.initial_seed() + rank)
    return device, rank, world


def make_loader(dataset, batch_size, rank=0, world=1, seed=0):
    """The reference's `DataLoader(dataset, batch_size, shuffle=True)` (classifier_free_MSR.py:190-192); data parallel: every
    rank iterates its own 1/world of a per-epoch permutation (DistributedSampler pads so that all ranks make the same number
    of steps -- each step holds a collective)."""
    import torch.utils.data as data
    if world == 1:
        return data.DataLoader(dataset, batch_size=batch_size, shuffle=True)
    sampler = data.distributed.DistributedSampler(dataset, num_replicas=world, rank=rank, shuffle=True, seed=seed)
    return data.DataLoader(dataset, batch_size=batch_size, sampler=sampler)


def sync_replicas(diffusion_model):
    """Data parallel: every replica starts from rank 0's weights -- `apply(init_weights)` drew them from each rank's own
    generator -- for `model.*` and `ema.module.*` alike; then the library re-packs (the broadcast writes through `.data`)."""
    from . import parallel
    _, world = parallel.world()
    if world == 1:
        return
    parallel.broadcast_parameters(diffusion_model)
    for m in (diffusion_model.model, diffusion_model.ema.module):
        if hasattr(m, "mark_weights_changed"):
            m.mark_weights_changed()


def step_health(diffusion_model, loss_value, device, world, where=""):
    """Raise FloatingPointError on EVERY rank if ANY rank's step was invalid: its fp16 range flag is set (`UNet1D.range_exceeded`, the twin
    handle's included) or its loss is not finite.  world > 1: one all-reduce(MAX) of two scalars (gloo / RCCL), issued by every rank in
    every step -- the healthy path pays a 8-byte collective behind the gradient bucket's, a failing rank can no longer leave the job
    hanging in the next step's gradient all-reduce."""
    import math
    model = diffusion_model.model
    bad_range = bool(hasattr(model, "range_exceeded") and model.range_exceeded())
    bad_loss = not math.isfinite(loss_value)
    here = (bad_range, bad_loss)
    if world > 1:
        import torch.distributed as dist
        t = torch.tensor([float(bad_range), float(bad_loss)], dtype=torch.float32, device=device if device is not None else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        bad_range, bad_loss = bool(t[0].item() > 0), bool(t[1].item() > 0)
    if not (bad_range or bad_loss):
        return
    who = "this rank" if any(here) else "another rank"
    what = []
    if bad_range:
        what.append("an activation of the training step left the fp16 range of the split-f16 path (|x| > 6e4, or a whole raw row too small "
                    "for it: bound under 2^-9, a row of the network input under 2^-14; the float32 reference has no such limits): bring the "
                    "targets to order 1 -- scale them DOWN if an activation was too large, UP if the data is in small units -- or train "
                    "with model.set_precision('f32')")
    if bad_loss:
        what.append("the loss is not finite")
    raise FloatingPointError(f"{where}: invalid training step on {who} of {world}: " + "; ".join(what) +
                             ".  The gradients of this step and the update made from them are invalid on every rank")


class DeviceBatches:
    """The training set on the device, once, and the reference's shuffled batches (`DataLoader(dataset, batch_size, shuffle=True)`,
    classifier_free_MSR.py:190-192) as index tensors: no per-sample fetch and no collate on the host (3.4 ms per 512-row batch), one gather
    per tensor on the device.  `X` (conditions) and `Y` (targets) are held as float32 on `device`.

    The order of epoch `e` is `torch.randperm(n, generator=g)` drawn on the HOST from a private generator seeded with `seed` once and
    advanced once per epoch (epoch e is the (e+1)-th draw; the global generator is never touched); not the DataLoader's own order.
    `epoch(e)` uploads it once and yields per-batch index tensors, views of the uploaded permutation; the last batch is ragged, as
    `drop_last=False` gives it.  `host_order(e)` is the same permutation as a list of index lists, so that a plain eager loop can be fed
    the identical batches."""

    def __init__(self, X, Y, batch_size, seed=0, device=None):
        X, Y = torch.as_tensor(X, dtype=torch.float32), torch.as_tensor(Y, dtype=torch.float32)
        if X.shape[0] != Y.shape[0]:
            raise ValueError(f"DeviceBatches: {X.shape[0]} conditions and {Y.shape[0]} targets")
        if int(batch_size) < 1:
            raise ValueError("DeviceBatches: batch_size must be at least 1")
        self.device = torch.device(device) if device is not None else X.device
        self.X, self.Y = X.to(self.device).contiguous(), Y.to(self.device).contiguous()
        self.n, self.batch_size, self.seed = int(X.shape[0]), int(batch_size), int(0 if seed is None else seed)
        self._gen = torch.Generator()
        self._drawn, self._perm = -1, None     # the last epoch drawn and its permutation (host)

    def __len__(self):
        return (self.n + self.batch_size - 1) // self.batch_size

    def _order(self, e):
        e = int(e)
        if e < 0:
            raise ValueError("DeviceBatches: epochs count from 0")
        if self._perm is None or e < self._drawn:
            self._gen.manual_seed(self.seed)   # an earlier epoch again: the draws from the start
            self._drawn = -1
        while self._drawn < e:
            self._perm = torch.randperm(self.n, generator=self._gen)
            self._drawn += 1
        return self._perm

    def host_order(self, e):
        perm = self._order(e).tolist()
        return [perm[i:i + self.batch_size] for i in range(0, self.n, self.batch_size)]

    def epoch(self, e):
        perm = self._order(e).to(self.device)  # ONE upload per epoch
        for i in range(0, self.n, self.batch_size):
            yield perm[i:i + self.batch_size]

    def fill(self, idx, cond_out, y_out):
        """Gather the rows `idx` into the caller's buffers (`StepGraph`'s static `cond` and `y`), which must have `len(idx)` rows."""
        torch.index_select(self.X, 0, idx, out=cond_out)
        torch.index_select(self.Y, 0, idx, out=y_out)

    def take(self, idx):
        """(conditions, targets) of the rows `idx` as new tensors."""
        return self.X.index_select(0, idx), self.Y.index_select(0, idx)


class _BatchesAsLoader:
    """A `DeviceBatches` behind the two things `run_epochs`' eager loop asks of a loader: `sampler.set_epoch(e)` and iteration."""

    def __init__(self, batches):
        self.batches, self.sampler, self._epoch = batches, self, 0

    def set_epoch(self, e):
        self._epoch = e

    def __iter__(self):
        return (self.batches.take(idx) for idx in self.batches.epoch(self._epoch))


def _read_loss_by_t(diffusion_model, epoch):
    """With a loss report on (`DDPM.loss_report`): read and zero it right behind the epoch's own synchronise, keep the epoch's mean squared
    error per timestep in `diffusion_model.loss_by_t` (a list, one float64 [T] tensor per epoch, NaN where no row was drawn; the row counts
    in `loss_rows_by_t`) and return the second log line of the epoch, which goes out after the pinned `Epoch: e, Loss: ...` line.  None
    without a report."""
    if getattr(diffusion_model, "_report", None) is None:
        return None
    mean_sq, rows = diffusion_model.read_loss_report(reset=True)
    if not isinstance(getattr(diffusion_model, "loss_by_t", None), list):
        diffusion_model.loss_by_t = []
        diffusion_model.loss_rows_by_t = []
    diffusion_model.loss_by_t.append(mean_sq)
    diffusion_model.loss_rows_by_t.append(rows)
    return f"Epoch: {epoch}, Loss by timestep: " + " ".join(f"{v:.4g}" for v in mean_sq.tolist())


def _run_epochs_graph(diffusion_model, batches, optimizer, scheduler, epochs, use_ema, warmup_epoch, device, log):
    """`run_epochs(graph=True)`: every full batch is `DeviceBatches.fill` into static buffers and one `StepGraph.step()`; the ragged last
    batch one eager step of the same sequence (`StepGraph.step_on`)."""
    rows_full = batches.batch_size
    y_buf = torch.empty(rows_full, batches.Y.shape[1], device=batches.device, dtype=torch.float32)
    c_buf = torch.empty(rows_full, batches.X.shape[1], device=batches.device, dtype=torch.float32)
    sg = StepGraph(diffusion_model, optimizer, y_buf, c_buf, warmup=0)
    epoch_sum = torch.zeros((), device=batches.device, dtype=torch.float64)
    ema_step_cnt = 1
    try:
        for epoch in range(epochs):
            epoch_sum.zero_()
            epoch_rows = 0
            for idx in batches.epoch(epoch):
                if idx.numel() == rows_full:
                    batches.fill(idx, c_buf, y_buf)
                    loss = sg.step()
                else:
                    x, y_true = batches.take(idx)
                    loss = sg.step_on(y_true, x)
                if (use_ema and epoch > warmup_epoch and ema_step_cnt > diffusion_model.ema_start
                        and ema_step_cnt % diffusion_model.ema_update_rate == 0):
                    diffusion_model.ema.update_parameters(diffusion_model.model)
                # float64 additions of the float32 batch losses in step order: the sum the eager loop forms on the host, bit for bit
                epoch_sum.add_(loss.detach())
                epoch_rows += idx.numel()
                ema_step_cnt += 1
            epoch_loss = epoch_sum.item()       # the epoch's one synchronise
            by_t = _read_loss_by_t(diffusion_model, epoch)      # behind that synchronise; one small copy, no further wait
            # one health check per epoch, on the sum (a NaN or inf of any step stays in it) and on the sticky fp16 range flag: an invalid
            # step is reported at the END of its epoch, after the steps that followed it
            step_health(diffusion_model, epoch_loss, device, 1,
                        where=f"epoch {epoch} (graph=True: checked once, at the end of the epoch, over all its steps)")
            log(f"Epoch: {epoch}, Loss: {epoch_loss / epoch_rows}")
            if by_t is not None:
                log(by_t)
            scheduler.step()
    finally:
        sg.close()
    return diffusion_model


def run_epochs(diffusion_model, loader, optimizer, scheduler, epochs, use_ema, warmup_epoch, device, log=print, graph=False, batches=None):
    """The reference's epoch loop (classifier_free_MSR.py:217-234).  `batches`: a `DeviceBatches` in place of `loader` (which is then not
    read): the same loop fed from the device-resident set.

    `graph=True` (opt-in) runs every step through the captured step graph (`StepGraph`) from a `DeviceBatches`, with no host
    synchronisation inside an epoch: the epoch loss is accumulated on the device (float64, step order: the logged lines are the eager
    loop's) and read once per epoch, and `step_health` runs once per epoch on that sum and the sticky fp16 range flag, NOT per step -- an
    invalid step is reported at the end of its epoch, and the steps behind it have run.  (With the EMA gate open, `update_parameters` reads
    its `n_averaged` buffer: one synchronise per EMA update.)  Requirements, each refused with its own message: a single process
    (data-parallel runs keep the eager loop: pass graph=False), `diffusion_model.device_draws` set, a `FlatAdam` on its native path, a
    `DeviceBatches`, a batch below `DDPM.train_split_min_rows`.  The EMA gate, MultiStepLR and the log line are the eager loop's; weights,
    Adam's state and `_draw_calls` after the run equal those of the eager loop on the same batches and `device_draws` seed, bit for bit."""
    if graph:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise ValueError("run_epochs(graph=True) is single-process: data-parallel runs keep the eager loop (one all-reduce per step): "
                             "pass graph=False")
        if getattr(diffusion_model, "device_draws", None) is None:
            raise ValueError("run_epochs(graph=True) needs device-side draws: set diffusion_model.device_draws = <seed> (torch's generator "
                             "cannot be replayed from a graph)")
        if not isinstance(optimizer, FlatAdam) or not FlatAdam.native_step:
            raise ValueError("run_epochs(graph=True) needs a FlatAdam on its native path as the optimizer")
        if not isinstance(batches, DeviceBatches):
            raise ValueError("run_epochs(graph=True) needs batches=DeviceBatches(X, Y, batch_size, seed, device): the captured step reads "
                             "static device buffers, which a DataLoader cannot fill without the host")
        if diffusion_model._splits(batches.batch_size):
            raise ValueError(f"run_epochs(graph=True): a batch of {batches.batch_size} rows runs as two halves on two handles "
                             "(DDPM.train_split_min_rows): train with batches below that threshold, or graph=False")
        return _run_epochs_graph(diffusion_model, batches, optimizer, scheduler, epochs, use_ema, warmup_epoch, device, log)
    if batches is not None:
        loader = _BatchesAsLoader(batches)
    from . import parallel
    rank, world = parallel.world()
    if rank != 0:
        log = lambda *_a, **_k: None        # rank 0 reports (its local metric); every rank trains
    ema_step_cnt = 1
    for epoch in range(epochs):
        epoch_loss, epoch_rows = 0.0, 0
        if hasattr(getattr(loader, "sampler", None), "set_epoch"):
            loader.sampler.set_epoch(epoch)
        for x, y_true in loader:
            x = x.to(device)
            y_true = y_true.to(device)
            loss = diffusion_model(y_true, x)
            loss.backward()
            diffusion_model.allreduce_grads()   # no-op unless torch.distributed is initialised with world_size > 1
            optimizer.step()
            optimizer.zero_grad()
            if (use_ema and epoch > warmup_epoch and ema_step_cnt > diffusion_model.ema_start
                    and ema_step_cnt % diffusion_model.ema_update_rate == 0):
                diffusion_model.ema.update_parameters(diffusion_model.model)
            loss_value = loss.item()
            epoch_loss += loss_value
            # loss.item() has just synchronised: reading the fp16 range flag of the split-f16 path costs nothing more.  A step whose raw
            # operands left fp16's range saturated silently (the float32 reference is fine at |x| > 6e4): its gradients, and the update
            # just made from them, are wrong -- stop and say what to do.  Data parallel: EVERY rank takes part in step_health's
            # two-scalar all-reduce(MAX) and every rank raises in the same step; a rank that raised alone would leave the others
            # waiting in the next gradient all-reduce.  The gradient bucket stays the step's only large message.
            step_health(diffusion_model, loss_value, device, world, where=f"epoch {epoch}")
            epoch_rows += x.shape[0]
            ema_step_cnt += 1
        # the reference prints (sum of batch-mean losses) / (row count), MSR.py:233 -- reproduced as is
        log(f"Epoch: {epoch}, Loss: {epoch_loss / epoch_rows}")
        by_t = _read_loss_by_t(diffusion_model, epoch)
        if by_t is not None:
            log(by_t)
        scheduler.step()
    return diffusion_model
