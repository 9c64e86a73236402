"""Training on a timestep law, on the device: the law's draw against the stated integer rule, the weighted loss and its
gradients against the oracle, the loss by timestep, the captured step under a law and a report, the refusals at the C ABI, the
host-generator path and the no-split rule.  Nets `tiny` (T = 8) and `nu3` (T = 20), B = 70 unless a case says otherwise; references
and budgets from tests/timesteps_ref.py (tests/test_timesteps_cpu.py checks their caps)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import philox_ref as P
import timesteps_ref as R
from _util import GOLD
from oracle import ddpm_oracle as O
from test_gpu_parity import GTOL, _device_draws, assert_grads
from weights import CONFIGS

pytestmark = pytest.mark.gpu

MODES = ["split_f16", "f32"]
G24 = 1 << 24


def make_ddpm(name, mode="split_f16"):
    from diffsg_amd import UNet1D
    from diffsg_amd.classifier_free_MSR import DDPM
    cfg, T = CONFIGS[name], R.NETS[name]["T"]
    m = UNet1D(**cfg, is_attn=(False,) * len(cfg["dims"]))
    m.load_state_dict(R.net(name)[1], strict=True)
    D = cfg["input_dim"]
    d = DDPM(T, m.to("cuda"), D, 10.0, 1.0 - O.cosine_betas(T), torch.device("cuda"), (1, D), None, 0.1, 0.9999, 1, 2).to("cuda")
    d.model.set_precision(mode)
    return d


def step(d, y, cond, **kw):
    """(loss as a float, [gradient clones]) of one forward + backward."""
    for q in d.model.parameters():
        q.grad = None
    loss = d(y, cond, **kw)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), [q.grad.detach().clone() for q in d.model.parameters()]


def same(a, b):
    return a[0] == b[0] and all(torch.equal(x, z) for x, z in zip(a[1], b[1]))


def inputs(name, rows):
    cfg = CONFIGS[name]
    g = torch.Generator().manual_seed(rows)
    return (torch.rand(rows, cfg["input_dim"], generator=g) * 0.25).cuda(), torch.rand(rows, cfg["cond_dim"], generator=g).cuda()


def laws(d, kind):
    from diffsg_amd import steps, timesteps as TS
    T = d.T
    if kind == "two_point":
        p = np.zeros(T)
        p[2], p[T - 3] = 1.0, 3.0
        return TS.law(d, p)
    if kind == "on_plan":
        return TS.on_plan(d, steps.strided(d, 4))
    if kind == "zero_ends":
        p = np.minimum(np.arange(T), np.arange(T)[::-1]).astype(np.float64)
        return TS.law(d, p, w=R.weights("tiny" if T == 8 else "nu3"))
    assert kind == "weights_only"
    return TS.law(d, None, w=R.weights("tiny" if T == 8 else "nu3"))


# ------------------------------------------------------------------------------------------------ 1. the draw
@pytest.mark.parametrize("name,kind,B", [("tiny", "two_point", 70), ("tiny", "on_plan", 70), ("tiny", "zero_ends", 70), ("tiny", "weights_only", 70),
                                         ("tiny", "two_point", 1000), ("tiny", "on_plan", 1000), ("tiny", "zero_ends", 1000),
                                         ("tiny", "weights_only", 1000), ("nu3", "on_plan", 70), ("nu3", "zero_ends", 1000)])
def test_the_laws_draw_is_the_stated_integer_rule(name, kind, B):
    d = make_ddpm(name)
    T, D, keep, seed = d.T, CONFIGS[name]["input_dim"], 1.0 - d.uncond_prob, 4242
    lw = laws(d, kind)
    y, cond = inputs(name, B)
    d.train_law = lw
    d.loss_report(True)
    for call in range(2):
        # the 24-bit word of every row from the CPU restatement of the draws (tests/philox_ref.py), not from the library: T = 2^24 gives
        # ts == u24 exactly, and the device's own call with that T must agree
        u24 = P.train_draws(seed, call, G24, keep, B, D)[0].astype(np.int64)
        assert u24.min() >= 0 and u24.max() < G24
        assert np.array_equal(_device_draws(seed, call, G24, keep, B, D)[0].cpu().numpy(), u24)
        _, noise, mask = _device_draws(seed, call, T, keep, B, D)
        if lw.cdf24 is None:
            ts_want = P.train_draws(seed, call, T, keep, B, D)[0].astype(np.int64)                 # the uniform draw, as without a law
        else:
            ts_want = R.expected_ts(lw.cdf24, u24)
        d.device_draws, d._draw_calls = seed, call
        got = step(d, y, cond)
        _, rows = d.read_loss_report()
        assert rows.tolist() == np.bincount(ts_want, minlength=T).tolist(), (call, rows.tolist())
        if lw.p is not None:
            assert all(int(rows[t]) == 0 for t in range(T) if lw.p[t] == 0)
        d.device_draws = None
        ref = step(d, y, cond, ts=torch.from_numpy(ts_want)[None, :].cuda(), noise=noise, cond_mask=mask[:, None])
        d.read_loss_report()
        assert same(got, ref), (kind, B, call, got[0], ref[0])


# ------------------------------------------------------------------------------------------------ 2. the weights
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["tiny", "nu3"])
def test_unit_weights_give_the_bits_of_the_step_without_a_law(name, mode):
    from diffsg_amd import timesteps as TS
    d = make_ddpm(name, mode)
    y, cond, ts, noise, mask = (v.cuda() for v in R.train_inputs(name))
    kw = dict(ts=ts, noise=noise, cond_mask=mask)
    plain = step(d, y, cond, **kw)
    d.train_law = TS.law(d, None, w=np.ones(d.T))
    ones = step(d, y, cond, **kw)
    assert same(plain, ones)
    d.train_law = None
    assert same(plain, step(d, y, cond, **kw))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["tiny", "nu3"])
def test_weighted_loss_and_gradients_vs_the_reference(name, mode):
    from diffsg_amd import timesteps as TS
    d = make_ddpm(name, mode)
    y, cond, ts, noise, mask = (v.cuda() for v in R.train_inputs(name))
    d.train_law = TS.law(d, None, w=R.weights(name).numpy())
    loss, _ = step(d, y, cond, ts=ts, noise=noise, cond_mask=mask)
    l32, g32, l64, g64 = R.weighted_ref(name)
    print(f"{name}/{mode}: weighted loss {loss:.8g}, reference {float(l32):.8g}, rel err {abs(loss - float(l32)) / abs(float(l32)):.2e}")
    assert abs(loss - float(l32)) <= 1e-5 * abs(float(l32))
    assert_grads({k: q.grad for k, q in d.model.named_parameters()}, g32, g64, f"weighted {name}/{mode}")     # GTOL + 4 x budget, per tensor
    assert GTOL == 1e-4


@pytest.mark.parametrize("mode", MODES)
def test_a_batch_of_zero_weight_rows_gives_zero_loss_and_zero_gradients(mode):
    from diffsg_amd import timesteps as TS
    d = make_ddpm("tiny", mode)
    y, cond, _, noise, mask = (v.cuda() for v in R.train_inputs("tiny"))
    w = np.ones(d.T)
    w[2] = w[5] = 0.0
    ts = torch.where(torch.arange(R.B) % 2 == 0, 2, 5)[None, :].cuda()
    d.train_law = TS.law(d, None, w=w)
    loss, grads = step(d, y, cond, ts=ts, noise=noise, cond_mask=mask)
    assert loss == 0.0
    assert all(bool((g == 0).all()) for g in grads) and all(bool(torch.isfinite(g).all()) for g in grads)


# ------------------------------------------------------------------------------------------------ 3. the report
def test_report_sums_rows_determinism_and_removal():
    name = "nu3"
    d = make_ddpm(name)
    T, D = d.T, CONFIGS[name]["input_dim"]
    y, cond, ts0, noise0, mask = (v.cuda() for v in R.train_inputs(name))
    steps3 = [((ts0 + k) % T, noise0.roll(k, 0)) for k in range(3)]
    want_sq, want_rows = torch.zeros(T, dtype=torch.float64), torch.zeros(T, dtype=torch.int64)
    for ts, nz in steps3:
        t = ts.reshape(-1)
        y_t = d.sqrt_alphas_cumprod[t][:, None] * y + d.sqrt_one_minus_alphas_cumprod[t][:, None] * nz
        eps = d.model(y_t, ts / T, cond, mask)                          # the device's own eps_hat (dsg_unet_forward)
        sq, rows = R.per_timestep_sums(eps.cpu(), nz.cpu(), ts.cpu(), T)
        want_sq += sq
        want_rows += rows

    def run():
        for ts, nz in steps3:
            step(d, y, cond, ts=ts, noise=nz, cond_mask=mask)
        torch.cuda.synchronize()
        return d._report[0].clone(), d._report[1].clone()
    d.loss_report(True)
    sq1, rows1 = run()
    err = float(((sq1.cpu() - want_sq).abs() / want_sq.clamp(min=1e-300)).max())
    print(f"report: worst relative error of sq_dev {err:.2e}; rows {rows1.tolist()}")
    assert torch.equal(rows1.cpu(), want_rows) and int(want_rows.sum()) == 3 * R.B
    assert err <= 1e-6
    mean, rows = d.read_loss_report()                                       # reads and zeroes
    assert torch.equal(rows, want_rows) and bool(torch.isnan(mean[rows == 0]).all())
    seen = rows > 0
    assert float((mean[seen] - want_sq[seen] / (want_rows[seen] * D)).abs().max()) <= 1e-6 * float(mean[seen].max())
    assert not bool(d._report[0].any()) and not bool(d._report[1].any())
    sq2, rows2 = run()
    assert torch.equal(sq1, sq2) and torch.equal(rows1, rows2)              # bit-identical from zeroed buffers
    bufs = d._report
    d.loss_report(False)
    step(d, y, cond, ts=steps3[0][0], noise=steps3[0][1], cond_mask=mask)
    torch.cuda.synchronize()
    assert torch.equal(bufs[0], sq2) and torch.equal(bufs[1], rows2)        # removed: nothing is added


# ------------------------------------------------------------------------------------------------ 4. the captured step
def _graph_setup(name, law_of, report=True):
    from diffsg_amd.train import FlatAdam
    d = make_ddpm(name)
    d.device_draws = 321
    d.train_law = law_of(d)
    if report:
        d.loss_report(True)
    return d, FlatAdam(d, lr=5e-3)


def _snapshot(d, opt):
    """Clones of everything a step leaves behind, stream-ordered behind it.  No device-wide synchronise here: the clones need none, and
    the sequence replay -> torch.cuda.synchronize() -> replay of the same captured step leaves the eager sequence on this runtime with
    or without a law -- a defect of the captured step that is older than the law and is described in DESIGN.md 17 ("Open")."""
    st = opt.state[opt._flat]
    rep = getattr(d, "_report", None)
    return [opt._flat.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), torch.tensor(float(st["step"])),
            torch.tensor(d._draw_calls)] + ([rep[0].clone(), rep[1].clone()] if rep else [])


@pytest.mark.parametrize("name", ["tiny", "nu3"])
def test_step_graph_under_a_law_and_a_report_is_the_eager_loop(name):
    """Ten steps: six under a law with a CDF, weights and a report, two after a change of law, two after its removal; the captured step
    against the eager loop, bit for bit after every step: the loss, the weights, Adam's moments and step, `_draw_calls` and the two
    report buffers; 7 replays and 2 re-captures."""
    from diffsg_amd import timesteps as TS
    from diffsg_amd.train import StepGraph
    B = 70
    y, cond = inputs(name, B)
    law_a = lambda d: TS.law(d, np.arange(1, d.T + 1), w=R.weights(name).numpy())
    law_b = lambda d: TS.on_plan(d, (1, d.T - 2))
    sched = [None] * 6 + [law_b, law_b, "remove", "remove"]          # six steps under law_a, then a change, then none

    def eager(d, opt):
        loss = d(y, cond)
        loss.backward()
        opt.step()
        opt.zero_grad()
        return float(loss.detach())
    runs = []
    for graph in (False, True):
        d, opt = _graph_setup(name, law_a)
        sg = StepGraph(d, opt, y, cond, warmup=0) if graph else None
        losses, snaps = [], []
        for k, change in enumerate(sched):
            if change == "remove":
                d.train_law = None
            elif change is not None and (k == 0 or sched[k - 1] is not change):
                d.train_law = change(d)
            losses.append(float(sg.step().detach()) if graph else eager(d, opt))
            snaps.append(_snapshot(d, opt))
        if graph:
            assert sg.replays == 5 + 1 + 1 and sg.recaptures == 2, (sg.replays, sg.eager_steps, sg.recaptures)
            sg.close()
        runs.append((losses, snaps))
        print(f"{name} {'graph' if graph else 'eager'} losses: " + " ".join(f"{v:.9g}" for v in losses))
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    for k, (a, b) in enumerate(zip(runs[0][1], runs[1][1])):
        assert len(a) == len(b) == 7 and all(torch.equal(x, z) for x, z in zip(a, b)), k
    assert int(runs[1][1][-1][6].sum()) == len(sched) * B


def test_run_epochs_graph_under_the_training_context():
    """The 200-row NU fixture (140 training rows: two batches of 64 and one of 12), two epochs, through entry.train_ddpm inside
    timesteps.training(law=on_plan(K = 5), report=True); the eager run is entry.train's own sequence with graph=False."""
    from diffsg_amd import classifier_free_NU as NU, entry, steps, timesteps as TS, train as tr
    from diffsg_amd.diffusion import init_weights
    csv = os.path.join(GOLD, "data", "3u_18mW_200samples.csv")
    law_of = lambda d: TS.on_plan(d, steps.strided(d, 5))
    with TS.training(law=law_of, report=True):
        lines_g = []
        torch.manual_seed(4)
        mg = entry.train_ddpm("nu", csv, epochs=2, batch_size=64, log=lines_g.append, graph=True, seed=0)
        # the same run, eager
        X, Y, _, _, _, cc = NU.nu_data_load(csv, 400, 400)
        dev = torch.device("cuda:0")
        torch.manual_seed(4)
        me = NU.build_model(cc["K"], cc["P_sum"], dev, 20, cc)
        TS.apply_active(me)
        me.apply(init_weights)
        me.to(dev)
        opt = tr.FlatAdam(me, lr=0.004)
        me.device_draws = 0
        batch = []
        me.register_forward_hook(lambda m, inp, out: batch.append((out.detach(), inp[0].shape[0])))
        lines_e = []
        b = tr.DeviceBatches(torch.tensor(X, dtype=torch.float32), torch.tensor(Y, dtype=torch.float32), 64, 0, dev)
        tr.run_epochs(me, None, opt, torch.optim.lr_scheduler.MultiStepLR(opt, [80, 200]), 2, False, 5, dev, lines_e.append, batches=b)
    print("\n".join(lines_g))
    assert lines_g == lines_e and len(lines_g) == 4
    assert lines_g[0].startswith("Epoch: 0, Loss: ") and lines_g[1].startswith("Epoch: 0, Loss by timestep: ")
    assert torch.equal(torch.cat([p.detach().reshape(-1) for p in mg.model.parameters()]),
                       torch.cat([p.detach().reshape(-1) for p in me.model.parameters()]))
    T, D = 20, 5
    support = set(steps.strided(mg, 5).taus)
    for m in (mg, me):
        assert len(m.loss_by_t) == 2 and all(tuple(v.shape) == (T,) for v in m.loss_by_t)
    for e in range(2):
        assert torch.equal(mg.loss_by_t[e].nan_to_num(-1.0), me.loss_by_t[e].nan_to_num(-1.0))
        mean, rows = mg.loss_by_t[e], mg.loss_rows_by_t[e]
        assert int(rows.sum()) == 140 and set(torch.nonzero(rows).reshape(-1).tolist()) <= support
        assert bool(torch.isnan(mean[rows == 0]).all())
        got = float((mean.nan_to_num(0.0) * rows).sum() / rows.sum())
        want = sum(float(l.double()) * n for l, n in batch[3 * e:3 * e + 3]) / 140            # w == 1: the unweighted loss of the epoch's rows
        print(f"epoch {e}: row-weighted mean of mean_sq {got:.9g}, unweighted loss {want:.9g}")
        assert abs(got - want) <= 1e-6 * want
    assert D == mg.model.cfg["input_dim"]


# ------------------------------------------------------------------------------------------------ 5. refusals at the C ABI
def test_refusals_at_the_c_abi():
    from diffsg_amd import _lib
    L = _lib.lib()
    name = "tiny"
    d = make_ddpm(name)
    T, D = d.T, CONFIGS[name]["input_dim"]
    y, cond, ts, noise, mask = (v.cuda() for v in R.train_inputs(name))
    before = step(d, y, cond, ts=ts, noise=noise, cond_mask=mask)
    hd = d.model.native_handle()
    U, F = ctypes.c_uint * T, ctypes.c_float * T
    good = U(*[G24 * (k + 1) // T for k in range(T)])

    def refused(rc, *words):
        assert rc != 0
        msg = L.dsg_last_error().decode()
        assert all(w in msg for w in words), msg
    gen0 = int(L.dsg_generation(hd))
    refused(L.dsg_set_train_law(hd, good, None, -1), "dsg_set_train_law", "negative")
    dec = U(*good)
    dec[3] = dec[2] - 1
    refused(L.dsg_set_train_law(hd, dec, None, T), "dsg_set_train_law", "decreases at step 3")
    short = U(*good)
    short[T - 1] = G24 - 1
    refused(L.dsg_set_train_law(hd, short, None, T), "dsg_set_train_law", "last CDF entry", str(G24))
    for bad in (-1.0, float("nan"), float("inf")):
        w = F(*([1.0] * T))
        w[4] = bad
        refused(L.dsg_set_train_law(hd, None, w, T), "dsg_set_train_law", "weight 4", "finite and >= 0")
    sq, rows = torch.zeros(T + 1, dtype=torch.float64, device="cuda"), torch.zeros(T + 1, dtype=torch.int64, device="cuda")
    refused(L.dsg_set_train_report(hd, _lib.ptr(sq), _lib.ptr(rows), -2), "dsg_set_train_report", "negative")
    refused(L.dsg_set_train_report(hd, _lib.ptr(sq), None, T), "dsg_set_train_report", "rows_dev")
    assert int(L.dsg_generation(hd)) == gen0                             # a refused setter changes nothing
    assert L.dsg_set_train_law(hd, None, None, 0) == 0 and L.dsg_set_train_report(hd, None, None, 0) == 0
    assert int(L.dsg_generation(hd)) == gen0                             # removing what is not held moves nothing

    # T mismatch on the three training entry points, under a law and under a report of T + 1 entries
    good1 = (ctypes.c_uint * (T + 1))(*[G24 * (k + 1) // (T + 1) for k in range(T + 1)])
    bucket = torch.full((int(L.dsg_param_total(hd)),), 7.0, device="cuda")
    loss = torch.full((1,), -3.0, device="cuda")
    call_dev = torch.tensor([5], dtype=torch.int64, device="cuda")
    sa, sb = _lib.ptr(d.sqrt_alphas_cumprod), _lib.ptr(d.sqrt_one_minus_alphas_cumprod)
    ts32 = ts.reshape(-1).to(torch.int32).contiguous()
    mk = mask.reshape(-1).contiguous()
    keep = ctypes.c_float(0.9)
    for setting in ("law", "report"):
        if setting == "law":
            assert L.dsg_set_train_law(hd, good1, None, T + 1) == 0
        else:
            assert L.dsg_set_train_report(hd, _lib.ptr(sq), _lib.ptr(rows), T + 1) == 0
        words = ("dsg_set_train_" + setting, f"T = {T + 1}", f"T = {T}")
        refused(L.dsg_train_step(hd, _lib.ptr(y), _lib.ptr(cond), _lib.ptr(ts32), _lib.ptr(noise), _lib.ptr(mk), sa, sb, T, _lib.ptr(bucket),
                                 _lib.ptr(loss), R.B, _lib.stream_ptr()), "dsg_train_step:", *words)
        refused(L.dsg_train_step_seeded(hd, _lib.ptr(y), _lib.ptr(cond), 9, 0, keep, sa, sb, T, _lib.ptr(bucket), _lib.ptr(loss), R.B,
                                        _lib.stream_ptr()), "dsg_train_step_seeded:", *words)
        refused(L.dsg_train_step_seeded_dyn(hd, _lib.ptr(y), _lib.ptr(cond), 9, _lib.ptr(call_dev), keep, sa, sb, T, _lib.ptr(bucket),
                                            _lib.ptr(loss), R.B, _lib.stream_ptr()), "dsg_train_step_seeded_dyn:", *words)
        torch.cuda.synchronize()
        assert bool((bucket == 7.0).all()) and float(loss) == -3.0 and int(call_dev) == 5        # nothing was enqueued
        assert not bool(sq.any()) and not bool(rows.any())
        assert L.dsg_set_train_law(hd, None, None, 0) == 0 and L.dsg_set_train_report(hd, None, None, 0) == 0
    assert same(before, step(d, y, cond, ts=ts, noise=noise, cond_mask=mask))                      # the handle trains as before


# ------------------------------------------------------------------------------------------------ 6. the host-generator path
def test_host_generator_path_under_a_law(monkeypatch):
    from diffsg_amd import timesteps as TS
    name = "tiny"
    d = make_ddpm(name)
    d.draws_on_side_stream = False
    y, cond = inputs(name, R.B)
    lw = laws(d, "two_point")
    d.train_law = lw
    d.loss_report(True)
    assert d.device_draws is None
    order = []
    real = {n: getattr(torch, n) for n in ("randint", "randn_like", "bernoulli")}
    for n in real:
        monkeypatch.setattr(torch, n, lambda *a, _n=n, **k: (order.append((_n, k.get("high"))), real[_n](*a, **k))[1])
    torch.manual_seed(11)
    first = step(d, y, cond)
    rows = d.read_loss_report()[1]
    assert [o[0] for o in order] == ["randint", "randn_like", "bernoulli"] and order[0][1] == G24
    for n in real:
        monkeypatch.setattr(torch, n, real[n])
    torch.manual_seed(11)
    u24 = torch.randint(low=0, high=G24, size=(1, R.B), device="cuda")
    ts_want = R.expected_ts(lw.cdf24, u24.cpu().numpy().reshape(-1))
    assert rows.tolist() == np.bincount(ts_want, minlength=d.T).tolist() and set(ts_want.tolist()) <= {2, d.T - 3}
    torch.manual_seed(11)
    assert same(first, step(d, y, cond))                                  # reproducible under torch.manual_seed


# ------------------------------------------------------------------------------------------------ 7. no split
def test_a_law_keeps_a_batch_in_one_piece():
    from diffsg_amd import timesteps as TS
    name = "nu3"
    y, cond = inputs(name, 128)
    out = {}
    for thr in (64, None):
        d = make_ddpm(name)
        d.device_draws = 5
        d.train_split_min_rows = thr
        d.train_law = TS.law(d, np.arange(1, d.T + 1))
        assert not d._splits(128)
        out[thr] = step(d, y, cond)
        assert "_twins" not in d.model.__dict__ or not d.model.__dict__["_twins"]      # no second handle was made
    assert same(out[64], out[None])
    d = make_ddpm(name)
    d.device_draws = 5
    d.train_split_min_rows = 64
    assert d._splits(128)
    step(d, y, cond)
    assert d.model.__dict__.get("_twins")                                 # without a law the batch runs as two halves, as before
