"""Every stream-taking entry point of include/diffsg.h on a NON-default stream.

The header's contract: "`stream` is a hipStream_t passed as void*; all work is enqueued on it, the calls do not synchronise".  PyTorch's
default stream is the legacy null stream, which orders itself against every blocking stream, so on it a launch on stream 0 instead of `s`,
a library-owned stream that never waits on `s` (or is never joined back) and a blocking null-stream table upload all give correct
numbers.  `torch.cuda.Stream()` is a non-blocking stream: there they do not.

One protocol for every case `f() -> outputs` over input buffers on the device (reference_pass / deferred_pass below):

  1. reference pass on the default stream: real inputs, `f` once to warm up (workspace growth, table builds, graph capture), `f` again:
     its outputs are `want`, its host time the case's enqueue time;
  2. the input buffers are filled with DECOYS: another seeded draw of the same shape and dtype, valid for the operation (finite, ts in
     [0, T), gains in the generator's range), so that a wrongly ordered read gives wrong numbers and never a fault;
  3. deferred pass: on a fresh side stream a delay is enqueued, an event recorded behind it, the REAL inputs copied into the buffers
     behind that, and `f` called while the delay still runs (`ev.query()` is False before the call, or the case fails as "delay too
     short").  The outputs are cloned on the side stream, and again on the default stream after `wait_stream(side)`;
  4. both clones equal `want` bit for bit; `want` is within the bound the existing test of that entry point holds it to (CPU oracle,
     numpy restatement or bit-for-bit composition); and, unless the case is listed as synchronising, `ev.query()` is still False when
     `f` returns: "the calls do not synchronise" in the steady state.  A case listed as synchronising (with its reason, read from
     the host side under csrc/) must have waited for the delay instead: both lists are pinned.

The delay is 10 x the longest enqueue time of the table, at least 20 ms, at most 250 ms, calibrated once with a pair of events.  A control
case runs `torch.softmax` under the same protocol from the DEFAULT stream: it must see the decoys, or the whole module fails -- side
streams would then be ordered against the null stream and nothing here would mean anything.

CASES is importable data: tests/test_streams_cpu.py checks on the CPU that every function of the header that takes a stream is named in
it (or exempted with a reason).  All tests here need an MI355X: run with `-m gpu`.
"""
import ctypes
import functools
import os
import time
from collections import namedtuple

import numpy as np
import pytest
import torch

import attn_ref as AR
import shape_ref as S
from _util import GOLD, synth_params
from oracle import ddpm_oracle as O
from test_gpu_parity import GTOL, POLICIES, TOL, assert_grads, rel
from weights import CONFIGS

pytestmark = pytest.mark.gpu

B, T = S.B, S.T                 # 70 rows (three row tiles, the last one ragged), 5 steps
DELAY_MIN_MS, DELAY_MAX_MS, DELAY_FACTOR = 20.0, 250.0, 10.0

Case = namedtuple("Case", "id entries sync build args")
CASES = []


def case(cid, entries, build, *args, sync=None):
    """One row of the table: id, the header functions the case calls, why it synchronises (None: it must not), builder and arguments."""
    CASES.append(Case(cid, tuple(entries), sync, build, args))


# reasons of the synchronising cases, read from the host side: csrc/host_forward.hpp (prepare_fused, the driver of the forward tables, and
# run_cond_embed), csrc/host_sample.hpp (sample_impl, enqueue_step) and csrc/dsg_api.hip (the entry points)
SYNC_F32_COND = "exact-f32 mode: run_cond_embed uploads the <= 32-wide blocks' table from a reused host vector and synchronises `stream` first"
SYNC_CHUNK_SEEDS = "dsg_sample_chunked uploads the per-chunk seeds from pageable host memory and synchronises `stream` behind the copy"
SYNC_PROFILE = "DSG_SAMPLE_PROFILE reads its HIP events back: one hipStreamSynchronize per step"
SYNC_RANGE = "the range check of DDPM.sample reads the flag with dsg_range_status_stream: one hipStreamSynchronize per call"
SYNC_POINTERS = ("dsg_unet_forward keeps x and out in its fused-run table: a call with another x / out pointer (UNet1D.forward allocates its "
                 "output per call) rebuilds the table, and prepare_fused synchronises `stream` first")
SYNC_RESHAPE = "a call at another batch size rebuilds the fused-run tables: prepare_fused synchronises `stream` before it reuses the host tables"


class Built:
    """A built case: input buffers, their real and decoy contents, the call, the oracle check; `keep` holds what must stay alive."""

    def __init__(self, bufs, real, decoy, f, check=None, keep=None):
        assert len(bufs) == len(real) == len(decoy)
        for b, r, d in zip(bufs, real, decoy):
            assert b.shape == r.shape == d.shape and b.dtype == r.dtype == d.dtype, (b.shape, r.shape, d.shape, b.dtype, r.dtype, d.dtype)
            assert bool(torch.isfinite(d.double()).all())
        self.bufs, self.real, self.decoy, self.f, self.check, self.keep = bufs, real, decoy, f, check, keep
        self.want, self.enqueue_ms = None, None


def lib():
    from diffsg_amd import _lib
    return _lib


def call(name, *args):
    L = lib()
    L.check(getattr(L.lib(), name)(*args, L.stream_ptr()))


def ptr(t):
    return lib().ptr(t)


def dev(*ts):
    return [(torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t).cuda().contiguous() for t in ts]


def like(ts):
    return [torch.empty_like(t) for t in ts]


def load(bufs, src):
    with torch.no_grad():
        for b, s in zip(bufs, src):
            b.copy_(s)


def same_bits(a, b):
    """Bit-for-bit equality (NaNs included): the bytes."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


# ---------------------------------------------------------------------------------------------------------------------
# the protocol
# ---------------------------------------------------------------------------------------------------------------------
def _delay(units):
    """A harmless delay on the current stream: torch.cuda._sleep, or a fixed chain of matmuls where torch has none."""
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(int(units))
    else:
        a = _delay.__dict__.setdefault("a", torch.full((512, 512), 1.0 / 512, device="cuda"))
        for _ in range(max(int(units) // 100000, 1)):
            a = a @ a
        _delay.a = a


def _time_delay(units):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    _delay(units)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def calibrate_delay(target_ms):
    """(units, measured ms) of a delay of about target_ms: one pair of events per probe, at most four probes."""
    units = 1000000
    _time_delay(units)                                  # first launch: module load
    ms = _time_delay(units)
    for _ in range(3):
        if ms >= 2.0:
            break
        units *= 10
        ms = _time_delay(units)
    units = max(int(units * target_ms / max(ms, 1e-3)), 1)
    return units, _time_delay(units)


def reference_pass(bt):
    """Step 1, on the default stream."""
    load(bt.bufs, bt.real)
    bt.f()
    torch.cuda.synchronize()
    load(bt.bufs, bt.real)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    outs = bt.f()
    bt.enqueue_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    bt.want = [o.detach().clone() for o in outs]
    torch.cuda.synchronize()


N_SIDE_STREAMS = 2      # consecutive streams of torch's pool per case: see deferred_pass


def deferred_pass(bt, units, issue_on_default=False):
    """Steps 2 and 3, once on each of N_SIDE_STREAMS consecutive side streams.  Returns per stream (clones on the side stream, clones on
    the default stream or None, `ev.query()` was still False behind `f`); the default-stream clones are made for the first stream.
    issue_on_default: the control -- `f` is issued on the default stream although its inputs arrive on the side stream.

    Why two streams: HIP maps streams onto a few hardware queues in turn (four here), and a queue runs its packets in order.  Measured
    with one launch of the library redirected to stream 0: on one side stream in four -- the one that shares the null stream's queue --
    the misplaced kernel ran behind the delay anyway and the case stayed green.  Two streams created one after the other never share
    a queue, so a launch on any fixed wrong stream is out of order on at least one of them."""
    # the handle may have served another case since the reference pass: back to this case's steady state first
    load(bt.bufs, bt.real)
    bt.f()
    torch.cuda.synchronize()
    cur = torch.cuda.current_stream()
    sides = [torch.cuda.Stream() for _ in range(N_SIDE_STREAMS)]
    res = []
    for k, side in enumerate(sides):
        load(bt.bufs, bt.decoy)
        torch.cuda.synchronize()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            _delay(units)
            ev = torch.cuda.Event()
            ev.record()
            load(bt.bufs, bt.real)
            assert not ev.query(), "the delay was too short: it ended before the call was issued"
            if issue_on_default:
                with torch.cuda.stream(cur):
                    outs = bt.f()
                    got_side = [o.detach().clone() for o in outs]
            else:
                outs = bt.f()
                got_side = None
            pending = not ev.query()
            if got_side is None:
                got_side = [o.detach().clone() for o in outs]
        got_main = None
        if k == 0:
            cur.wait_stream(side)
            got_main = [o.detach().clone() for o in outs]
        side.synchronize()
        torch.cuda.synchronize()
        res.append((got_side, got_main, pending))
    return res


# ---------------------------------------------------------------------------------------------------------------------
# nets, seeded inputs and cached CPU references
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def net(name, seed=None):
    """(constructor arguments, plan, float32 weights, (forward, sample, loss_and_grads) of the oracle) of a shipped config or of an
    attention descriptor of tests/attn_ref.py ("attn_<name>")."""
    if name.startswith("attn_"):
        cfg = AR.ATTN_CONFIGS[name[5:]]
        plan, p = AR.attn_params(name[5:]) if seed is None else AR.attn_params(name[5:], seed)
        return cfg, plan, p, (AR.unet_forward, AR.sample, AR.loss_and_grads)
    plan, p = synth_params(name, 5 if seed is None else seed)
    return CONFIGS[name], plan, p, (O.unet_forward, O.ddpm_sample, O.ddpm_loss_and_grads)


def schedule(t=T):
    return O.schedule_buffers(1.0 - O.cosine_betas(t))


def make_ddpm(name, policy="default", mode="split_f16"):
    from diffsg_amd import UNet1D
    from diffsg_amd.classifier_free_MSR import DDPM
    cfg, _, p, _ = net(name)
    m = UNet1D(**cfg)
    m.load_state_dict(p, strict=True)
    D = cfg["input_dim"]
    d = DDPM(T, m.to("cuda"), D, 10.0, 1.0 - O.cosine_betas(T), torch.device("cuda"), (1, D), None).to("cuda")
    if mode != "split_f16":
        d.model.set_precision(mode)
    if policy == "large":
        d.model.set_launch_policy(0, 0)
    return d


@functools.lru_cache(maxsize=None)
def sampler(name, policy="default", mode="split_f16"):
    """One DDPM per (net, policy, mode), shared by the sampling cases (the graph / eager and omega variants change no table)."""
    return make_ddpm(name, policy, mode)


@functools.lru_cache(maxsize=None)
def sample_data(name, rows, seed):
    cfg = net(name)[0]
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(rows, cfg["cond_dim"], generator=g), torch.randn(rows, cfg["input_dim"], generator=g),
            torch.randn(T - 2, rows, cfg["input_dim"], generator=g))


@functools.lru_cache(maxsize=None)
def train_data(name, rows, seed):
    """y, cond, ts int32 [rows] in [0, T), noise, mask [rows]."""
    cfg = net(name)[0]
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(rows, cfg["input_dim"], generator=g) * 0.25, torch.rand(rows, cfg["cond_dim"], generator=g),
            torch.randint(0, T, (rows,), generator=g).to(torch.int32), torch.randn(rows, cfg["input_dim"], generator=g),
            (torch.rand(rows, generator=g) < 0.9).float())


@functools.lru_cache(maxsize=None)
def forward_data(name, rows, seed):
    cfg = net(name)[0]
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, cfg["input_dim"], generator=g), torch.randint(0, 50, (rows,), generator=g) / 50,
            torch.rand(rows, cfg["cond_dim"], generator=g), (torch.rand(rows, generator=g) < 0.8).float())


@functools.lru_cache(maxsize=None)
def sample_ref(name, rows, omega, lo=0, hi=None):
    """(float32 oracle samples of rows [lo, hi) of sample_data(name, rows, 9) as ONE call, rel(float32 oracle, float64 oracle))."""
    _, plan, p, fns = net(name)
    cond, y_T, z = (t[..., lo:hi, :] for t in sample_data(name, rows, 9))
    b = schedule()
    zd = {i: z[j] for j, i in enumerate(range(T - 1, 1, -1))}
    with torch.no_grad():
        ref = fns[1](p, plan, b, T, cond, omega, y_T, zd)
        ref64 = fns[1]({k: v.double() for k, v in p.items()}, plan, {k: v.double() for k, v in b.items()}, T, cond.double(), omega,
                       y_T.double(), {i: v.double() for i, v in zd.items()})
    return ref, rel(ref, ref64)


def check_sample(name, rows, omega, got, tag):
    """test_sample_large_launch_vs_oracle's bound on seeded inputs: TOL + 3 x the oracle's own float32 error."""
    ref, budget = sample_ref(name, rows, omega)
    e = rel(got, ref)
    print(f"{tag}: rel err vs oracle {e:.2e} (oracle float32 vs float64: {budget:.2e})")
    assert e <= TOL + 3.0 * budget, (tag, e, budget)


def check_train(name, model, y, cond, ts, noise, mask, grads_flat, loss, tag):
    """test_train_step_vs_oracle_ragged's bounds: loss 1e-5 relative, every gradient tensor within assert_grads."""
    _, plan, p, fns = net(name)
    args = (p, plan, schedule(), T, y.cpu(), cond.cpu(), ts.cpu().long()[None], noise.cpu(), mask.cpu()[:, None])
    ref_loss, g32 = fns[2](*args)
    _, g64 = fns[2](*args, f64=True)
    assert abs(float(loss) - float(ref_loss)) <= 1e-5 * abs(float(ref_loss)), (tag, float(loss), float(ref_loss))
    got, off = {}, 0
    for k, q in model.named_parameters():
        got[k] = grads_flat[off:off + q.numel()].view_as(q)
        off += q.numel()
    assert off == grads_flat.numel()
    assert_grads(got, g32, g64, tag)


# ---------------------------------------------------------------------------------------------------------------------
# builders: the UNet handle through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def b_bind_weights(name):
    """The weights are the inputs: changed on the side stream behind the delay, re-packed by dsg_bind_weights, seen by the next forward."""
    d = make_ddpm(name)
    _, plan, p, fns = net(name)
    params = d.model.param_list()
    hd = d.model.native_handle()
    bufs = [q.data for q in params]
    real = [q.detach().clone() for q in params]
    decoy = dev(*[net(name, 6 if not name.startswith("attn_") else AR.WEIGHT_SEED + 1)[2][k] for k, _ in d.model._named_param_list()])
    arr = (ctypes.c_void_p * len(params))(*[q.data_ptr() for q in params])
    x, t, cond, mask = dev(*forward_data(name, B, 9))
    out = torch.empty_like(x)       # one output buffer: the forward's table holds the caller's pointers (see SYNC_POINTERS)

    def f():
        call("dsg_bind_weights", hd, arr, len(params))
        call("dsg_unet_forward", hd, ptr(x), ptr(t), ptr(cond), ptr(mask), ptr(out), B)
        return [out]

    def check(want):
        xs, ts, cs, ms = forward_data(name, B, 9)
        with torch.no_grad():
            ref = fns[0](p, plan, xs, ts[None], cs, ms[:, None])
        assert rel(want[0], ref) <= TOL
    return Built(bufs, real, decoy, f, check, keep=(d, arr))


def b_forward(name, fresh_out=False):
    d = make_ddpm(name)
    _, plan, p, fns = net(name)
    hd = d.model.native_handle()
    real, decoy = dev(*forward_data(name, B, 9)), dev(*forward_data(name, B, 1009))
    bufs = like(real)
    x, t, cond, mask = bufs
    out = torch.empty_like(x)       # one output buffer: the forward's table holds the caller's pointers (see SYNC_POINTERS)

    def f():
        if fresh_out:               # UNet1D.forward: a new output tensor per call
            return [d.model(x, t[None], cond, mask[:, None])]
        call("dsg_unet_forward", hd, ptr(x), ptr(t), ptr(cond), ptr(mask), ptr(out), B)
        return [out]

    def check(want):
        xs, ts, cs, ms = forward_data(name, B, 9)
        with torch.no_grad():
            ref = fns[0](p, plan, xs, ts[None], cs, ms[:, None])
        assert rel(want[0], ref) <= TOL
    return Built(bufs, real, decoy, f, check, keep=d)


def b_sample(name, policy, mode, graph, omega, form="plain"):
    """dsg_sample / dsg_sample_rec with injected start state and noise; form: plain | rec | profile."""
    d = sampler(name, policy, mode)
    hd, coef, D = d.model.native_handle(), d._coef_table(), net(name)[0]["input_dim"]
    real, decoy = dev(*sample_data(name, B, 9)), dev(*sample_data(name, B, 1009))
    bufs = like(real)
    cond, y_T, z = bufs
    flags = 2 if form == "profile" else (0 if graph else 1)

    def f():
        out = torch.empty(B, D, device="cuda")
        if form == "rec":
            ry, re = torch.empty(T, B, D, device="cuda"), torch.empty(T, B, D, device="cuda")
            call("dsg_sample_rec", hd, ptr(cond), ptr(y_T), ptr(z), 0, omega, ptr(coef), T, ptr(out), B, flags, ptr(ry), ptr(re))
            return [out, ry, re]
        call("dsg_sample", hd, ptr(cond), ptr(y_T), ptr(z), 0, omega, ptr(coef), T, ptr(out), B, flags)
        return [out]

    def check(want):
        check_sample(name, B, omega, want[0], f"{name}/{policy}/{mode}/{'graph' if graph else 'eager'}/{omega:g}")
        if form == "rec":           # the last recorded state is the state the last step started from; the output follows from it
            assert bool(torch.isfinite(want[1]).all()) and bool(torch.isfinite(want[2]).all())
    return Built(bufs, real, decoy, f, check, keep=d)


def b_sample_chunked(name, rows, chunk):
    """Four independent 64-row calls (the last one 8 rows) in one set of launches: every chunk against the oracle's own call on its rows."""
    d = make_ddpm(name)
    hd, coef, D = d.model.native_handle(), d._coef_table(), net(name)[0]["input_dim"]
    real, decoy = dev(*sample_data(name, rows, 9)), dev(*sample_data(name, rows, 1009))
    bufs = like(real)
    cond, y_T, z = bufs
    nch = (rows + chunk - 1) // chunk
    seeds = (ctypes.c_ulonglong * nch)(*range(11, 11 + nch))

    def f():
        out = torch.empty(rows, D, device="cuda")
        call("dsg_sample_chunked", hd, ptr(cond), ptr(y_T), ptr(z), seeds, chunk, 2.0, ptr(coef), T, ptr(out), rows, 0)
        return [out]

    def check(want):
        for lo in range(0, rows, chunk):
            hi = min(lo + chunk, rows)
            ref, budget = sample_ref(name, rows, 2.0, lo, hi)
            e = rel(want[0][lo:hi], ref)
            print(f"chunk [{lo}, {hi}): rel err vs oracle {e:.2e} (budget {budget:.2e})")
            assert e <= TOL + 3.0 * budget, (lo, e, budget)
    return Built(bufs, real, decoy, f, check, keep=(d, seeds))


def b_train(name, rows, kind="explicit", beside=None, oracle=True):
    """dsg_train_step / _seeded / _seeded_dyn: flat gradients and the loss."""
    d = make_ddpm(name)
    if beside is not None:
        d.model.set_option("train_time_beside", beside)
    L = lib()
    hd = d.model.native_handle()
    total, D = L.lib().dsg_param_total(hd), net(name)[0]["input_dim"]
    sa, sb = d.sqrt_alphas_cumprod, d.sqrt_one_minus_alphas_cumprod
    seed, call_no, keep = 77, 3, 0.9
    if kind == "explicit":
        real, decoy = dev(*train_data(name, rows, 9)), dev(*train_data(name, rows, 1009))
    else:
        real, decoy = dev(*train_data(name, rows, 9)[:2]), dev(*train_data(name, rows, 1009)[:2])
        if kind == "seeded_dyn":        # the call number lives on the device: an input like the others
            real.append(torch.tensor([call_no], dtype=torch.int64, device="cuda"))
            decoy.append(torch.tensor([call_no + 8], dtype=torch.int64, device="cuda"))
    bufs = like(real)

    def f():
        grads, loss = torch.empty(total, device="cuda"), torch.empty(1, device="cuda")
        if kind == "explicit":
            y, cond, ts, noise, mask = bufs
            call("dsg_train_step", hd, ptr(y), ptr(cond), ptr(ts), ptr(noise), ptr(mask), ptr(sa), ptr(sb), T, ptr(grads), ptr(loss), rows)
            return [grads, loss]
        if kind == "seeded":
            y, cond = bufs
            call("dsg_train_step_seeded", hd, ptr(y), ptr(cond), seed, call_no, keep, ptr(sa), ptr(sb), T, ptr(grads), ptr(loss), rows)
            return [grads, loss]
        y, cond, cdev = bufs
        call("dsg_train_step_seeded_dyn", hd, ptr(y), ptr(cond), seed, ptr(cdev), keep, ptr(sa), ptr(sb), T, ptr(grads), ptr(loss), rows)
        return [grads, loss, cdev]

    def check(want):
        if not oracle:      # tests/test_gpu_parity.py holds the 32 768-row step to the oracle (test_train_step_large_launch_vs_oracle)
            assert bool(torch.isfinite(want[0]).all()) and bool(torch.isfinite(want[1]).all())
            return
        y, cond = real[0], real[1]
        if kind == "explicit":
            ts, noise, mask = real[2], real[3], real[4]
        else:               # the draws the seeded step makes are those of dsg_train_draws (test_seeded_train_step_is_the_explicit_step...)
            ts = torch.empty(rows, dtype=torch.int32, device="cuda")
            noise, mask = torch.empty(rows, D, device="cuda"), torch.empty(rows, device="cuda")
            L.check(L.lib().dsg_train_draws(seed, call_no, T, keep, rows, D, ptr(ts), ptr(noise), ptr(mask), L.stream_ptr()))
            torch.cuda.synchronize()
            if kind == "seeded_dyn":
                assert int(want[2]) == call_no + 1
        check_train(name, d.model, y, cond, ts, noise, mask, want[0].cpu(), want[1].cpu(), f"{name}/{kind}/{rows}")
    return Built(bufs, real, decoy, f, check, keep=d)


def b_train_draws():
    """dsg_train_draws has no device input: the case pins that it is enqueued on `stream` (the clone behind the delay sees the draws)
    and does not synchronise."""
    rows, D = B, 7

    def f():
        ts = torch.empty(rows, dtype=torch.int32, device="cuda")
        noise, mask = torch.empty(rows, D, device="cuda"), torch.empty(rows, device="cuda")
        call("dsg_train_draws", 77, 3, T, 0.9, rows, D, ptr(ts), ptr(noise), ptr(mask))
        return [ts, noise, mask]

    def check(want):
        ts, noise, mask = want
        assert 0 <= int(ts.min()) and int(ts.max()) < T and bool(torch.isfinite(noise).all()) and set(mask.unique().tolist()) <= {0.0, 1.0}
    return Built([], [], [], f, check)


def _adam_inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1, torch.randn(n, generator=g) * 0.01,
            torch.rand(n, generator=g) * 0.01)


def b_adam(dyn):
    """p, g, exp_avg, exp_avg_sq are inputs; bit-identical to torch.optim.Adam(fused=True), as the header states."""
    n, lr, step = 4099, 1e-3, 3
    real, decoy = dev(*_adam_inputs(n, 9)), dev(*_adam_inputs(n, 1009))
    if dyn:     # the learning rate and the step count live on the device
        real += [torch.tensor([lr], dtype=torch.float64, device="cuda"), torch.tensor([step - 1.0], device="cuda")]
        decoy += [torch.tensor([0.5], dtype=torch.float64, device="cuda"), torch.tensor([40.0], device="cuda")]
    bufs = like(real)

    def f():
        p, g, m, v = bufs[:4]
        if dyn:
            call("dsg_adam_step_dyn", ptr(p), ptr(g), ptr(m), ptr(v), n, ptr(bufs[4]), 0.9, 0.999, 1e-8, 0.0, 0, ptr(bufs[5]))
            return [p, m, v, bufs[5]]
        call("dsg_adam_step", ptr(p), ptr(g), ptr(m), ptr(v), n, lr, 0.9, 0.999, 1e-8, 0.0, 0, step)
        return [p, m, v]

    def check(want):
        q = real[0].clone().requires_grad_(True)
        q.grad = real[1].clone()
        opt = torch.optim.Adam([q], lr=lr, fused=True)
        opt.state[q] = {"step": torch.tensor(step - 1.0, device="cuda"), "exp_avg": real[2].clone(), "exp_avg_sq": real[3].clone()}
        opt.step()
        torch.cuda.synchronize()
        st = opt.state[q]
        assert torch.equal(want[0], q.detach()) and torch.equal(want[1], st["exp_avg"]) and torch.equal(want[2], st["exp_avg_sq"])
        if dyn:
            assert float(want[3]) == float(step)
    return Built(bufs, real, decoy, f, check)


def b_ema():
    n, decay = 4099, 0.9
    mk = lambda s: [torch.randn(n, generator=torch.Generator().manual_seed(s)), torch.randn(n, generator=torch.Generator().manual_seed(s + 1))]
    real, decoy = dev(*mk(9)), dev(*mk(1009))
    bufs = like(real)

    def f():
        call("dsg_ema_update", ptr(bufs[0]), ptr(bufs[1]), decay, 1.0 - decay, n)
        return [bufs[0]]

    def check(want):            # test_ema_update's bound
        ref = decay * real[0].double() + (1.0 - decay) * real[1].double()
        assert rel(want[0], ref.cpu()) <= 2e-7
    return Built(bufs, real, decoy, f, check)


# ---------------------------------------------------------------------------------------------------------------------
# builders: sequences on one handle, two streams, two handles
# ---------------------------------------------------------------------------------------------------------------------
def b_batch_sequence(name, sizes):
    """70 -> 513 -> 70 rows of dsg_sample back to back on one handle behind ONE delay, nothing synchronised by the caller in between:
    the table rebuild of every size change has to order itself against the calls still queued on `stream`."""
    d = make_ddpm(name)
    hd, coef, D = d.model.native_handle(), d._coef_table(), net(name)[0]["input_dim"]
    uniq = sorted(set(sizes))
    real = [t for r in uniq for t in dev(*sample_data(name, r, 9))]
    decoy = [t for r in uniq for t in dev(*sample_data(name, r, 1009))]
    bufs = like(real)
    by_rows = {r: bufs[3 * i:3 * i + 3] for i, r in enumerate(uniq)}

    def f():
        outs = []
        for r in sizes:
            cond, y_T, z = by_rows[r]
            out = torch.empty(r, D, device="cuda")
            call("dsg_sample", hd, ptr(cond), ptr(y_T), ptr(z), 0, 2.0, ptr(coef), T, ptr(out), r, 0)
            outs.append(out)
        return outs

    def check(want):
        for r, got in zip(sizes, want):
            check_sample(name, r, 2.0, got, f"{name} sequence {r} rows")
        assert torch.equal(want[0], want[2])
    return Built(bufs, real, decoy, f, check, keep=d)


def b_handover(name):
    """dsg_sample on stream A (the current one), stream B waits for A, dsg_train_step on B with the same handle: the caller orders the
    two streams, the library adds nothing."""
    d = make_ddpm(name)
    L = lib()
    hd, coef, D = d.model.native_handle(), d._coef_table(), net(name)[0]["input_dim"]
    total = L.lib().dsg_param_total(hd)
    sa, sb = d.sqrt_alphas_cumprod, d.sqrt_one_minus_alphas_cumprod
    real = dev(*sample_data(name, B, 9)) + dev(*train_data(name, B, 9))
    decoy = dev(*sample_data(name, B, 1009)) + dev(*train_data(name, B, 1009))
    bufs = like(real)
    other = torch.cuda.Stream()

    def f():
        cond, y_T, z, y, c2, ts, noise, mask = bufs
        a = torch.cuda.current_stream()
        out = torch.empty(B, D, device="cuda")
        call("dsg_sample", hd, ptr(cond), ptr(y_T), ptr(z), 0, 2.0, ptr(coef), T, ptr(out), B, 0)
        other.wait_stream(a)
        with torch.cuda.stream(other):
            grads, loss = torch.empty(total, device="cuda"), torch.empty(1, device="cuda")
            call("dsg_train_step", hd, ptr(y), ptr(c2), ptr(ts), ptr(noise), ptr(mask), ptr(sa), ptr(sb), T, ptr(grads), ptr(loss), B)
        a.wait_stream(other)
        return [out, grads, loss]

    def check(want):
        check_sample(name, B, 2.0, want[0], f"{name} hand-over, sample")
        check_train(name, d.model, *real[3:], want[1].cpu(), want[2].cpu(), f"{name} hand-over, train")
    return Built(bufs, real, decoy, f, check, keep=(d, other))


def b_two_handles(first, second):
    """Two handles sampling at once on two streams, each behind the delay."""
    ds = [make_ddpm(first), make_ddpm(second)]
    real = [t for n in (first, second) for t in dev(*sample_data(n, B, 9))]
    decoy = [t for n in (first, second) for t in dev(*sample_data(n, B, 1009))]
    bufs = like(real)
    other = torch.cuda.Stream()

    def one(d, name, cond, y_T, z):
        D = net(name)[0]["input_dim"]
        out = torch.empty(B, D, device="cuda")
        call("dsg_sample", d.model.native_handle(), ptr(cond), ptr(y_T), ptr(z), 0, 2.0, ptr(d._coef_table()), T, ptr(out), B, 0)
        return out

    def f():
        a = torch.cuda.current_stream()
        other.wait_stream(a)                 # behind the same delay and input copies
        with torch.cuda.stream(other):
            o2 = one(ds[1], second, *bufs[3:])
        o1 = one(ds[0], first, *bufs[:3])
        a.wait_stream(other)
        return [o1, o2]

    def check(want):
        check_sample(first, B, 2.0, want[0], f"two handles: {first}")
        check_sample(second, B, 2.0, want[1], f"two handles: {second}")
    return Built(bufs, real, decoy, f, check, keep=(ds, other))


# ---------------------------------------------------------------------------------------------------------------------
# builders: the Python layer with a side stream current
# ---------------------------------------------------------------------------------------------------------------------
def _backward(d, loss):
    loss.backward()
    return [loss.detach(), d.grad_bucket]


def _zero(d):
    for q in d.model.parameters():
        q.grad = None


def b_py_forward(name, rows, draws, oracle=True):
    """DDPM.forward + backward.  draws: "torch" (the generator, reseeded before every call; the draws run on DDPM's own _draw_stream),
    "device" (device_draws: dsg_train_step_seeded), "given" (explicit ts / noise / mask)."""
    d = make_ddpm(name)
    D = net(name)[0]["input_dim"]
    n_in = 5 if draws == "given" else 2
    real, decoy = dev(*train_data(name, rows, 9)[:n_in]), dev(*train_data(name, rows, 1009)[:n_in])
    bufs = like(real)
    if draws == "device":
        d.device_draws = 77

    def f():
        _zero(d)
        if draws == "torch":
            torch.manual_seed(1234)
            return _backward(d, d(bufs[0], bufs[1]))
        if draws == "device":
            d._draw_calls = 0
            return _backward(d, d(bufs[0], bufs[1]))
        y, cond, ts, noise, mask = bufs
        return _backward(d, d(y, cond, ts=ts[None], noise=noise, cond_mask=mask[:, None]))

    def check(want):
        if not oracle:      # 65 536 rows: test_train_step_large_launch_vs_oracle holds the split step to the oracle
            assert d._splits(rows) and bool(torch.isfinite(want[0]).all()) and bool(torch.isfinite(want[1]).all())
            return
        y, cond = real[0], real[1]
        if draws == "torch":        # the same three draws in the same order from the same seed (ddpm.py, MSR.py:101-107)
            torch.manual_seed(1234)
            ts = torch.randint(low=0, high=T, size=(1, rows), device="cuda")[0].to(torch.int32)
            noise = torch.randn_like(y)
            mask = torch.bernoulli(torch.fill(torch.zeros(rows, device="cuda"), 1 - d.uncond_prob))
        else:
            L = lib()
            ts = torch.empty(rows, dtype=torch.int32, device="cuda")
            noise, mask = torch.empty(rows, D, device="cuda"), torch.empty(rows, device="cuda")
            L.check(L.lib().dsg_train_draws(77, 0, T, float(1.0 - d.uncond_prob), rows, D, ptr(ts), ptr(noise), ptr(mask), L.stream_ptr()))
        torch.cuda.synchronize()
        check_train(name, d.model, y, cond, ts, noise, mask, want[1].cpu(), want[0].cpu(), f"DDPM.forward {name}/{draws}")
    return Built(bufs, real, decoy, f, check, keep=d)


def b_py_sample(name):
    d = make_ddpm(name)
    real, decoy = dev(*sample_data(name, B, 9)), dev(*sample_data(name, B, 1009))
    bufs = like(real)

    def f():
        return [d.sample(bufs[0], 2.0, y_T=bufs[1], noise=bufs[2])]

    def check(want):
        check_sample(name, B, 2.0, want[0], f"DDPM.sample {name}")
    return Built(bufs, real, decoy, f, check, keep=d)


def _msr_features(rows, seed):
    """test_gpu_repeated.features: the gains the objective reads (the generator's range 0.5 .. 2.5) and their min-max scaling."""
    X = torch.rand(rows, 3, generator=torch.Generator().manual_seed(seed)) * 2.0 + 0.5
    return (X - X.min()) / (X.max() - X.min()), X


def b_py_sample_best(n):
    """sample_best == best_of over the rounds' own sample() calls, bit for bit (test_sample_best_is_best_of_over_the_rounds_own_sample_calls)."""
    from test_gpu_repeated import make_problem_ddpm
    d = make_problem_ddpm("msr3", 31, T)
    real, decoy = dev(*_msr_features(96, 9)), dev(*_msr_features(96, 1009))
    bufs = like(real)
    seeds = [101, 202, 303][:n]

    def f():
        r = d.sample_best(bufs[0], bufs[1], n, 1.0, seeds=seeds, return_objectives=True)
        return [r.solution, r.objective, r.round, r.objectives]

    def check(want):
        from diffsg_amd import best_of
        problem, p = d._best_of_problem()
        rounds = torch.stack([d.sample(real[0], 1.0, seed=s) for s in seeds])
        ref = best_of(problem, rounds, real[1], return_objectives=True, **p)
        torch.cuda.synchronize()
        for a, b in zip(want, ref):
            assert torch.equal(a, b)
    return Built(bufs, real, decoy, f, check, keep=d)


# ---------------------------------------------------------------------------------------------------------------------
# builders: entry points without a handle
# ---------------------------------------------------------------------------------------------------------------------
def _decode_inputs(fn, rows, D, seed):
    g = torch.Generator().manual_seed(seed)
    if fn in ("row_softmax", "msr_decode"):
        return (torch.randn(rows, D, generator=g) * 4.0,)
    if fn == "co_decode":
        y = torch.randn(rows, D, generator=g)
        y[seed % 7::7] = -20.0                          # dead rows, elsewhere in the decoy
        return (y,)
    if fn == "msr_rate":
        return (10.0 * O.msr_decode(torch.randn(rows, D, generator=g) * 3.0), torch.rand(rows, D, generator=g) * 5.0)
    if fn == "co_cost":
        return (torch.rand(rows, 3 * D, generator=g) * 10.0, O.co_decode(torch.randn(rows, D, generator=g)))
    if fn == "nu_decode":
        return (torch.randn(rows, D, generator=g),)
    K = D - 2                                           # nu_rate
    return (O.nu_decode(torch.randn(rows, D, generator=g), 400, 400, 18.0), torch.rand(rows, 2 * K, generator=g) * 400.0)


def b_decode(fn, D, rows=63):
    """The seven decode.* functions, bounds of test_decoders_vs_oracle_random."""
    from diffsg_amd import decode as Dc
    cpu = _decode_inputs(fn, rows, D, 9)
    real, decoy = dev(*cpu), dev(*_decode_inputs(fn, rows, D, 1009))
    bufs = like(real)
    extra = (400, 400, 18.0) if fn == "nu_decode" else ()

    def f():
        return [getattr(Dc, fn)(*bufs, *extra)]

    def check(want):
        got = want[0].cpu()
        close = lambda ref, tol: float((got - ref).abs().max()) <= tol * max(float(ref.abs().max()), 1e-30)
        if fn == "row_softmax":
            assert close(torch.softmax(cpu[0], 1), 2e-6)
        elif fn == "msr_decode":
            assert close(O.msr_decode(cpu[0]), 3e-6)
        elif fn == "co_decode":
            assert close(O.co_decode(cpu[0]), 2e-6) and float(got[9 % 7::7].abs().max()) == 0.0
        elif fn == "msr_rate":
            assert close(O.msr_rate(*cpu), 5e-6)
        elif fn == "co_cost":
            assert close(O.co_cost(*cpu), 1e-5)
        elif fn == "nu_decode":
            assert close(O.nu_decode(cpu[0], 400, 400, 18.0), 2e-6)
        else:
            ref = O.nu_rate(*cpu)
            assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max()) + (D - 2) * 1.8e-7
    return Built(bufs, real, decoy, f, check)


def b_best_of(problem, D):
    """dsg_best_of == the composition of the decode.* calls per round, bit for bit (tests/test_gpu_repeated.py)."""
    from test_gpu_repeated import compose, inputs
    rows, n = 63, 5
    Yr, Xr, p = inputs(problem, rows, n, D=D, K=D)
    Yd, Xd, _ = inputs(problem, rows, n, D=D, seed=1, K=D)
    real, decoy = dev(Yr, Xr), dev(Yd, Xd)
    bufs = like(real)

    def f():
        from diffsg_amd import best_of
        r = best_of(problem, bufs[0], bufs[1], return_objectives=True, **p)
        return [r.solution, r.objective, r.round, r.objectives]

    def check(want):
        ref = compose(problem, real[0], real[1], **p)
        torch.cuda.synchronize()
        for a, b in zip(want, ref):
            assert same_bits(a, b)
    return Built(bufs, real, decoy, f, check)


def b_sum_rate_gen(rows, M):
    """dsg_sum_rate_gen through the C ABI (labelgen.SUM_RATE_GEN copies to the host itself); bounds of test_sum_rate_gen_vs_oracle."""
    gs = np.random.default_rng(rows + M).uniform(0.5, 2.5, size=(rows, M))
    real, decoy = dev(gs), dev(np.random.default_rng(rows + M + 1000).uniform(0.5, 2.5, size=(rows, M)))
    bufs = like(real)

    def f():
        schemes, rates = torch.empty_like(bufs[0]), torch.empty(rows, dtype=torch.float64, device="cuda")
        call("dsg_sum_rate_gen", ptr(bufs[0]), ptr(schemes), ptr(rates), rows, M, 20.0)
        return [schemes, rates]

    def check(want):
        from oracle import sumrate_oracle as SR
        ref_rates, ref_schemes = SR.sum_rate_gen(gs, 20.0)
        assert np.allclose(want[0].cpu().numpy(), ref_schemes, rtol=1e-10, atol=1e-12)
        assert np.allclose(want[1].cpu().numpy(), ref_rates, rtol=1e-12)
    return Built(bufs, real, decoy, f, check)


def _co_minlp_params(n, samples, seed):
    """(params [samples][7][n] as labelgen.CONV_CO_MINLP_GEN lays them out, the draws they come from), from the oracle's draw order."""
    from oracle import co_minlp_oracle as C
    np.random.seed(seed)
    P, draws = np.empty((samples, 7, n)), []
    for i in range(samples):
        s, f_local, alpha, h = C.draw_sample(n)
        c, beta, r_u, cost_local = C.derived(s, f_local, alpha, h)
        P[i] = (s, c, f_local, alpha, beta, r_u, cost_local)
        draws.append((s, f_local, alpha, h))
    return P, draws


def b_co_minlp(n, samples):
    """dsg_co_minlp_search through the C ABI; the labels equal the oracle's bit for bit (test_co_minlp_gen_vs_oracle)."""
    from oracle import co_minlp_oracle as C
    P, draws = _co_minlp_params(n, samples, 50 + n)
    real, decoy = dev(P), dev(_co_minlp_params(n, samples, 950 + n)[0])
    bufs = like(real)
    ch = dev(C.choices())[0]

    def f():
        Y, tol = torch.empty(samples, 2 * n + 1, dtype=torch.float64, device="cuda"), torch.empty(samples, dtype=torch.int32, device="cuda")
        call("dsg_co_minlp_search", ptr(bufs[0]), ptr(ch), ch.numel(), ptr(Y), ptr(tol), samples, n, C.F_T, C.P_T, C.P_I, C.THETA)
        return [Y, tol]

    def check(want):
        assert np.array_equal(want[0].cpu().numpy(), np.array([C.solve(*d)[1] for d in draws]))
    return Built(bufs, real, decoy, f, check, keep=ch)


def b_noma_uav(samples, P_sum):
    """dsg_noma_uav_search through the C ABI against the restatement, judged as tests/test_gpu_nu_gen.py judges it."""
    from diffsg_amd.labelgen import NU_H, NU_ROU_0, NU_SIGMA_SQ, coordinates_gen, feasible_solution
    np.random.seed(501)
    qs = coordinates_gen(samples)
    np.random.seed(1501)
    real, decoy = dev(qs), dev(coordinates_gen(samples))
    bufs = like(real)
    fs_host = np.ascontiguousarray(feasible_solution(P_sum))
    fs = dev(fs_host)[0]

    def f():
        out = torch.empty(samples, 6, dtype=torch.float64, device="cuda")
        call("dsg_noma_uav_search", ptr(bufs[0]), ptr(fs), fs.shape[0], ptr(out), samples, NU_SIGMA_SQ, NU_ROU_0, NU_H)
        return [out]

    def check(want):
        import nu_gen_ref as N
        from test_gpu_nu_gen import _judge
        _judge(qs, fs_host, want[0].cpu().numpy(), N.noma_uav_search(qs, fs_host, workers=1))
    return Built(bufs, real, decoy, f, check, keep=fs)


def _g(name):
    return np.load(os.path.join(GOLD, name))


def b_mlp(what):
    """dsg_mlp_forward / _loss_grad / _train_epoch on the NU net of tests/golden/g14_mtfnn.npz, bounds of tests/test_gpu_mtfnn.py."""
    import mtfnn_ref as MR
    import test_gpu_mtfnn as TM
    from diffsg_amd import mtfnn
    g14, case_ = _g("g14_mtfnn.npz"), "nu3"
    widths, n_sig = MR.CASES[case_]
    desc, p0, X, Y = TM.shaped_case(g14, case_)
    P = p0.numel()
    rs = np.random.RandomState(7)
    dp, dX, dY = dev(MR.flat(MR.synth_state(widths, 77), widths), rs.uniform(0, 1, X.shape).astype(np.float32), rs.uniform(0, 1, Y.shape).astype(np.float32))
    if what == "forward":
        real, decoy = [p0, X], [dp, dX]
    elif what == "loss_grad":
        real, decoy = [p0, X, Y], [dp, dX, dY]
    else:
        perm = lambda s: torch.randperm(MR.ROWS, generator=torch.Generator().manual_seed(s)).to(device="cuda", dtype=torch.int32)[None].contiguous()
        zeros = torch.zeros(1, P, device="cuda")
        real = [p0[None].contiguous(), zeros, zeros.clone(), X, Y, perm(64)]
        decoy = [dp[None].contiguous(), torch.full_like(zeros, 1e-3), torch.full_like(zeros, 1e-4), dX, dY, perm(65)]
    bufs = like(real)

    def f():
        if what == "forward":
            return [mtfnn.forward_flat(desc, bufs[0], bufs[1])]
        if what == "loss_grad":
            return list(mtfnn.loss_grad_flat(desc, *bufs))
        p, m, v, Xb, Yb, pm = bufs
        bl = mtfnn.train_epoch_flat(desc, p, m, v, Xb, Yb, pm, 64, MR.LR, 0)
        return [p, m, v, bl]

    def check(want):
        if what == "forward":
            assert rel(want[0], g14[f"{case_}.trained.out"]) < 1e-5
        elif what == "loss_grad":
            ref_loss = float(g14[f"{case_}.trained.loss"])
            assert abs(float(want[0]) - ref_loss) < 1e-5 * ref_loss
            ref = {k: g14[f"{case_}.trained.grad.{k}"].astype(np.float64) for k, _ in MR.shapes(widths)}
            assert max(TM.grad_errs(MR.unflat(want[1].cpu().numpy(), widths), ref).values()) < GTOL
        else:       # test_epoch_is_the_composition_bit_for_bit
            ref = TM.compose(desc, p0, X, Y, real[5][0], 64)
            torch.cuda.synchronize()
            for a, b in zip((want[0][0], want[1][0], want[2][0], want[3][0]), ref):
                assert torch.equal(a, b)
    return Built(bufs, real, decoy, f, check, keep=desc)


def b_ppo(what):
    """dsg_ppo_forward / _loss_grad / _train_epoch on the CO agent of tests/golden/g15_ppo.npz, bounds of tests/test_gpu_ppo.py."""
    import ppo_ref as PR
    import test_gpu_ppo as TP
    from diffsg_amd import ppo
    g15, case_, tag = _g("g15_ppo.npz"), "co3", "trained"
    p0, X, Y, old, noise, noise2 = TP.golden_inputs(g15, case_, tag)
    A = PR.CASES[case_]["A"]
    dX, dY, dnoise, _ = dev(*PR.inputs(case_, 5))
    dp = dev(PR.flat(PR.synth_state(case_, 77), case_))[0]
    dold = (old + 0.1).contiguous()
    desc = TP.desc_of(case_, env=(what != "forward"))
    if what == "forward":
        real, decoy = [p0, X], [dp, dX]
    elif what == "loss_grad":
        real, decoy = [p0, X, Y, old, noise], [dp, dX, dY, dold, dnoise]
    else:
        N = PR.ROWS
        perm = lambda s: torch.randperm(N, generator=torch.Generator().manual_seed(s)).to(device="cuda", dtype=torch.int32)[None].contiguous()
        zeros = torch.zeros(1, p0.numel(), device="cuda")
        real = [p0[None].contiguous(), zeros, zeros.clone(), X, Y, old[None].contiguous(), noise[None].contiguous(), perm(64)]
        decoy = [dp[None].contiguous(), torch.full_like(zeros, 1e-3), torch.full_like(zeros, 1e-4), dX, dY, dold[None].contiguous(),
                 dnoise[None].contiguous(), perm(65)]
    bufs = like(real)

    def f():
        if what == "forward":
            return list(ppo.forward_flat(desc, bufs[0], bufs[1]))
        if what == "loss_grad":
            return list(ppo.loss_grad_flat(desc, *bufs))
        p, m, v, Xb, Yb, o, nz, pm = bufs
        bo = ppo.train_epoch_flat(desc, p, m, v, Xb, Yb, o, nz, pm, 64, PR.LR, 0)
        return [p, m, v, bo, o]

    def check(want):
        g = lambda k: g15[f"{case_}.{tag}.{k}"]      # noqa: E731
        if what == "forward":
            assert rel(want[0], g("mu")) < 1e-5 and rel(want[1], g("value")) < 1e-5
        elif what == "loss_grad":       # test_one_batch_against_goldens
            out3, new_logp, reward, grad = want
            kappa = (np.abs(g("cost")) + np.abs(g("gt"))) / (np.abs(g("cost") - g("gt")) + PR.OFFSET[PR.CASES[case_]["env"]])
            want_r = g("reward").astype(np.float64)
            r_err = np.abs(reward.cpu().numpy().astype(np.float64) - want_r) / want_r
            assert rel(new_logp, g("new_logp")) < 1e-5 and np.all(r_err <= 1e-5 * kappa)
            assert abs(out3[0].item() - float(g("actor_loss"))) / abs(float(g("actor_loss"))) < 1e-5 * kappa.max()
            assert abs(out3[1].item() - float(g("critic_loss"))) / float(g("critic_loss")) < 1e-5 * kappa.max()
            got = PR.unflat(grad.cpu().numpy(), case_)
            ref = {k: g("grad." + k).astype(np.float64) for k in got if k != "log_std"}
            assert max(TP.grad_errs(got, ref).values()) < GTOL and not got["log_std"].any()
        else:       # test_epoch_is_the_composition_bit_for_bit
            ref = TP.compose(desc, p0, X, Y, old, noise, real[7][0], 64)
            torch.cuda.synchronize()
            for a, b in zip((want[0][0], want[1][0], want[2][0], want[3][0], want[4][0]), ref):
                assert torch.equal(a, b)
            assert not torch.equal(want[0][0], p0) and torch.equal(want[0][0][:A], p0[:A])
    return Built(bufs, real, decoy, f, check, keep=desc)


def b_gd(kind, size):
    """dsg_gd_* through the C ABI with `rec`: three iterations against the restatement on the last step's bound
    (test_ragged_batches_and_every_kernel_variant); the state buffer is input and output."""
    import gd_ref as GR
    rows, iters = 65, 3
    x, y0 = GR.synth(kind, rows, size)
    xd, yd = GR.synth(kind, rows, size, seed=1)
    real, decoy = dev(x, y0), dev(xd, yd * 1.01)
    bufs = like(real)
    D = y0.shape[1]

    def f():
        X, Y = bufs
        rec = torch.empty(iters, rows, D, dtype=torch.float64, device="cuda")
        if kind == "co":
            call("dsg_gd_co", ptr(X), ptr(Y), rows, size, iters, 0.1, 1.0, 1.0, ptr(rec), 1)
        elif kind == "msr":
            call("dsg_gd_msr", ptr(X), ptr(Y), rows, size, iters, 0.001, ptr(rec), 1)
        else:
            call("dsg_gd_nu", ptr(X), ptr(Y), rows, size, iters, 0.1, 18.0, ptr(rec), 1)
        return [Y, rec]

    def check(want):
        _, kept = GR.run(kind, x, y0, iters, (2, 3))
        ok, ratio = GR.step_ok(want[0].cpu().numpy(), kept[2], kept[3], 1e-13 if kind == "msr" and size > 8 else 1e-14)
        assert ok, (kind, size, ratio)
        assert same_bits(want[1][-1], want[0])
    return Built(bufs, real, decoy, f, check)


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
NETS = ("tiny", "msr80", "attn_wide")       # 128-wide panel kernels: msr80; AttentionBlocks (tests/attn_ref.py): attn_wide

for _n in NETS:
    case(f"bind_weights-{_n}", ["dsg_bind_weights", "dsg_unet_forward"], b_bind_weights, _n)
    case(f"unet_forward-{_n}", ["dsg_unet_forward"], b_forward, _n)
    for _pol in POLICIES:
        for _mode in ("split_f16", "f32"):
            for _graph in (True, False):
                for _om in S.OMEGAS:
                    case(f"sample-{_n}-{_pol}-{_mode}-{'graph' if _graph else 'eager'}-om{_om:g}", ["dsg_sample"], b_sample, _n, _pol, _mode,
                         _graph, _om, sync=SYNC_F32_COND if _mode == "f32" else None)
    case(f"sample_rec-{_n}", ["dsg_sample_rec"], b_sample, _n, "default", "split_f16", True, 2.0, "rec")
    case(f"train_step-{_n}-70", ["dsg_train_step"], b_train, _n, B)
    case(f"train_step_seeded-{_n}", ["dsg_train_step_seeded"], b_train, _n, B, "seeded")
    case(f"train_step_seeded_dyn-{_n}", ["dsg_train_step_seeded_dyn"], b_train, _n, B, "seeded_dyn")
case("py-unet_forward-tiny", ["dsg_unet_forward"], b_forward, "tiny", True, sync=SYNC_POINTERS)
case("sample-profile-tiny", ["dsg_sample"], b_sample, "tiny", "default", "split_f16", False, 2.0, "profile", sync=SYNC_PROFILE)
case("sample_chunked-msr3-200x64", ["dsg_sample_chunked"], b_sample_chunked, "msr3", 200, 64, sync=SYNC_CHUNK_SEEDS)
for _beside in (1, 0):      # the library's own side stream, its fork and its join
    case(f"train_step-msr80-32768-beside{_beside}", ["dsg_train_step"], b_train, "msr80", 32768, "explicit", _beside, False)
case("train_draws", ["dsg_train_draws"], b_train_draws)
case("adam_step", ["dsg_adam_step"], b_adam, False)
case("adam_step_dyn", ["dsg_adam_step_dyn"], b_adam, True)
case("ema_update", ["dsg_ema_update"], b_ema)
case("batch_sequence-msr80-70-513-70", ["dsg_sample"], b_batch_sequence, "msr80", (70, 513, 70), sync=SYNC_RESHAPE)
case("stream_handover-tiny", ["dsg_sample", "dsg_train_step"], b_handover, "tiny")
case("two_handles-tiny-co3", ["dsg_sample"], b_two_handles, "tiny", "co3")
case("py-forward-torch_draws-tiny", ["dsg_train_step"], b_py_forward, "tiny", B, "torch")
case("py-forward-device_draws-tiny", ["dsg_train_step_seeded"], b_py_forward, "tiny", B, "device")
case("py-forward-msr80-65536-twin", ["dsg_train_step"], b_py_forward, "msr80", 65536, "given", False)
case("py-sample-tiny", ["dsg_sample_rec"], b_py_sample, "tiny", sync=SYNC_RANGE)
case("py-sample_best-msr3-n3", ["dsg_sample_rec", "dsg_best_of"], b_py_sample_best, 3, sync=SYNC_RANGE)
for _fn, _Ds in (("row_softmax", (17, 1100)), ("msr_decode", (17, 1100)), ("co_decode", (3,)), ("msr_rate", (80,)), ("co_cost", (3,)),
                 ("nu_decode", (9,)), ("nu_rate", (9,))):
    for _D in _Ds:
        case(f"decode-{_fn}-D{_D}", ["dsg_" + _fn], b_decode, _fn, _D)
for _pb, _D in (("msr", 80), ("co", 3), ("nu", 3)):
    case(f"best_of-{_pb}", ["dsg_best_of"], b_best_of, _pb, _D)
for _rows, _M in ((5, 2), (300, 128)):
    case(f"sum_rate_gen-{_rows}x{_M}", ["dsg_sum_rate_gen"], b_sum_rate_gen, _rows, _M)
case("co_minlp_search-n3-5", ["dsg_co_minlp_search"], b_co_minlp, 3, 5)
case("noma_uav_search-4", ["dsg_noma_uav_search"], b_noma_uav, 4, 6)
for _w in ("forward", "loss_grad", "train_epoch"):
    case(f"mlp_{_w}", ["dsg_mlp_" + _w], b_mlp, _w)
    case(f"ppo_{_w}", ["dsg_ppo_" + _w], b_ppo, _w)
for _k, _sz in (("co", 3), ("msr", 3), ("msr", 80), ("nu", 3)):
    case(f"gd_{_k}-{_sz}", ["dsg_gd_" + _k], b_gd, _k, _sz)

IDS = [c.id for c in CASES]
assert len(set(IDS)) == len(IDS)


# ---------------------------------------------------------------------------------------------------------------------
# the session state: every case built and run on the default stream, the delay calibrated, the control run
# ---------------------------------------------------------------------------------------------------------------------
def _control():
    real, decoy = dev(torch.randn(B, 80, generator=torch.Generator().manual_seed(9))), dev(torch.randn(B, 80, generator=torch.Generator().manual_seed(1009)))
    bufs = like(real)
    return Built(bufs, real, decoy, lambda: [torch.softmax(bufs[0], 1)])


@pytest.fixture(scope="module")
def table():
    """{case id: Built or the exception its builder raised}, plus "delay" = (units, measured ms, longest enqueue ms)."""
    built = {}
    for c in CASES:
        try:
            bt = c.build(*c.args)
            reference_pass(bt)
            built[c.id] = bt
        except Exception as e:          # the case's own test reports it; the others still run
            built[c.id] = e
    ctl = _control()
    reference_pass(ctl)
    times = {cid: bt.enqueue_ms for cid, bt in built.items() if isinstance(bt, Built)}
    longest = max(times, key=times.get)
    target = min(max(DELAY_FACTOR * times[longest], DELAY_MIN_MS), DELAY_MAX_MS)
    units, measured = calibrate_delay(target)
    print(f"\nstream protocol: longest enqueue {times[longest]:.3f} ms ({longest}); delay target {target:.1f} ms, calibrated "
          f"{units} units = {measured:.1f} ms")
    built["delay"] = (units, measured, times[longest])
    # the control: the same protocol, the call issued on the DEFAULT stream.  It must read the decoys -- on every side stream but one
    # that shares the null stream's hardware queue (deferred_pass), so: on at least one of the consecutive streams
    runs = deferred_pass(ctl, units, issue_on_default=True)
    built["control"] = (ctl, runs)
    if all(same_bits(side[0], ctl.want[0]) for side, _, _ in runs):
        pytest.fail("control: a call on the default stream saw inputs written on a side stream behind the delay -- side streams are "
                    "ordered against the null stream here (or the delay does not defer): no case of this module means anything")
    yield built


def test_control_a_call_on_the_default_stream_reads_the_decoys(table):
    ctl, runs = table["control"]
    saw_decoys = 0
    for k, (side, _, pending) in enumerate(runs):
        assert pending, "the delay ended before the control's call was issued"
        if same_bits(side[0], ctl.want[0]):
            continue                                            # this side stream shares the null stream's hardware queue
        assert same_bits(side[0], torch.softmax(ctl.decoy[0], 1))      # exactly the decoy's result: the copy had not started
        saw_decoys += 1
    print(f"control: the default-stream call read the decoys on {saw_decoys} of {len(runs)} side streams; "
          f"max |softmax(decoy) - softmax(real)| = {float((torch.softmax(ctl.decoy[0], 1) - ctl.want[0]).abs().max()):.3e}")
    assert saw_decoys >= len(runs) - 1


@pytest.mark.parametrize("cid", IDS)
def test_entry_point_on_a_side_stream(table, cid):
    c = CASES[IDS.index(cid)]
    bt = table[cid]
    if isinstance(bt, Exception):
        raise bt
    units, measured, _ = table["delay"]
    print(f"{cid}: enqueue {bt.enqueue_ms:.3f} ms, delay {measured:.1f} ms")
    assert measured > bt.enqueue_ms or c.sync, "the calibrated delay does not cover this case's enqueue time"
    runs = deferred_pass(bt, units)
    for k, (side, main, _) in enumerate(runs):
        for i, w in enumerate(bt.want):
            assert same_bits(side[i], w), f"side stream {k}: output {i}, cloned on the side stream, differs from the default-stream run"
            if main is not None:
                assert same_bits(main[i], w), f"side stream {k}: output {i}, cloned on the default stream behind wait_stream(side), differs"
    if bt.check is not None:
        bt.check(bt.want)
    for k, (_, _, pending) in enumerate(runs):
        if c.sync is None:
            assert pending, f"side stream {k}: the call synchronised: the event behind the delay had completed when it returned"
        else:   # the list of synchronising calls is pinned too: a case that stops synchronising leaves it (and the header's list)
            assert not pending, f"side stream {k}: listed as synchronising ({c.sync}), but the delay was still running when the call returned"


def test_first_use_of_a_fresh_handle_on_a_side_stream():
    """Handle creation, the first dsg_bind_weights, workspace growth, table uploads and graph capture all happen inside the first calls.
    Here they happen with a non-blocking side stream current (as in train.StepGraph's warm-up): the first training step and the first
    sampling call of a fresh handle must give the bits a fresh handle gives on the default stream, within the oracle's bounds.  Not a
    steady state: these calls synchronise, and no delay is used."""
    name = "msr80"
    tr, sm = dev(*train_data(name, B, 9)), dev(*sample_data(name, B, 9))

    def first_calls():
        d = make_ddpm(name)
        y, cond, ts, noise, mask = tr
        _zero(d)
        out = _backward(d, d(y, cond, ts=ts[None], noise=noise, cond_mask=mask[:, None]))
        return d, [out[0].clone(), out[1].clone(), d.sample(sm[0], 2.0, y_T=sm[1], noise=sm[2])]

    d0, want = first_calls()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d1, got = first_calls()
    side.synchronize()
    for i, (a, b) in enumerate(zip(got, want)):
        assert same_bits(a, b), i
    check_train(name, d0.model, *tr, want[1].cpu(), want[0].cpu(), "first step of a fresh handle")
    check_sample(name, B, 2.0, want[2], "first sampling call of a fresh handle")
