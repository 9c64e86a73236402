"""Training from device-resident data through the captured step graph (`run_epochs(graph=True)`, `train.StepGraph`, `train.DeviceBatches`).

Every comparison is BIT FOR BIT: the reference of every case is the eager loop of this tree, fed the same batches (`host_order(e)`) with the
same `device_draws` seed.  Nets `tiny` (T = 8) and `nu3` (T = 20) with the synthetic weights of seed 3; 150 rows in batches
of 64: two full batches and a ragged one of 22 rows (five 32-row tiles, the last ragged)."""
import os

import numpy as np
import pytest
import torch

from _util import GOLD, synth_params
from oracle import ddpm_oracle as O
from weights import CONFIGS

pytestmark = pytest.mark.gpu

N, BS = 150, 64
NET_T = {"tiny": 8, "nu3": 20}
FORMS = [(p, m) for p in ("default", "large") for m in ("split_f16", "f32")]        # launch policy x precision mode
DRAWS = 321


def make_ddpm(name, policy="default", mode="split_f16"):
    from diffsg_amd import UNet1D
    from diffsg_amd.classifier_free_MSR import DDPM
    cfg, T = CONFIGS[name], NET_T[name]
    m = UNet1D(**cfg, is_attn=(False,) * len(cfg["dims"]))
    m.load_state_dict(synth_params(name, 3)[1], strict=True)
    D = cfg["input_dim"]
    d = DDPM(T, m.to("cuda"), D, 10.0, 1.0 - O.cosine_betas(T), torch.device("cuda"), (1, D), None, 0.1, 0.9999, 1, 2).to("cuda")
    if policy == "large":
        d.model.set_launch_policy(0, 0)
    d.model.set_precision(mode)
    d.device_draws = DRAWS
    return d


def setup(name, policy="default", mode="split_f16"):
    from diffsg_amd.train import FlatAdam
    d = make_ddpm(name, policy, mode)
    opt = FlatAdam(d, lr=5e-3)
    return d, opt, torch.optim.lr_scheduler.MultiStepLR(opt, [1])


def data(name, rows=N):
    cfg = CONFIGS[name]
    g = torch.Generator().manual_seed(rows)
    return torch.rand(rows, cfg["cond_dim"], generator=g), torch.rand(rows, cfg["input_dim"], generator=g) * 0.25


class HostOrderLoader:
    """The eager loop's loader: the batches of `DeviceBatches.host_order(e)` as host tensors, as a DataLoader hands them over."""

    def __init__(self, X, Y, batches):
        self.X, self.Y, self.batches, self.sampler, self.e = X, Y, batches, self, 0

    def set_epoch(self, e):
        self.e = e

    def __iter__(self):
        return iter([(self.X[i], self.Y[i]) for i in self.batches.host_order(self.e)])


def state(d, opt):
    torch.cuda.synchronize()
    st = opt.state[opt._flat]
    return {"model": opt._flat.detach().clone(), "ema": torch.cat([p.detach().reshape(-1) for p in d.ema.module.parameters()]),
            "n_averaged": int(d.ema.n_averaged), "exp_avg": st["exp_avg"].clone(), "exp_avg_sq": st["exp_avg_sq"].clone(),
            "step": float(st["step"]), "calls": int(d._draw_calls)}


def assert_same(a, b):
    for k in a:
        assert (torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k]), k


def counters_on_host(d, opt):
    return getattr(opt, "_dyn", None) is None and getattr(d, "_call_dev", None) is None


def generation(d):
    from diffsg_amd import _lib
    return int(_lib.lib().dsg_generation(d.model._native.handle))


def record_graphs(monkeypatch):
    """The StepGraph objects run_epochs makes."""
    from diffsg_amd import train as tr
    made = []

    class Recorded(tr.StepGraph):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    monkeypatch.setattr(tr, "StepGraph", Recorded)
    return made


def run_both(name, policy, mode, monkeypatch, between=None, epochs=3):
    """(eager state, eager log, graph state, graph log, the StepGraph) of `epochs` epochs, EMA on from epoch 1, lr milestone at 1;
    `between(d, epoch)` runs at the end of every epoch (from the log call) in both runs."""
    from diffsg_amd import train as tr
    X, Y = data(name)
    dev = torch.device("cuda")
    out = []
    made = record_graphs(monkeypatch)
    for graph in (False, True):
        d, opt, sched = setup(name, policy, mode)
        b = tr.DeviceBatches(X, Y, BS, 9, dev)
        lines = []

        def log(line, d=d, lines=lines):
            lines.append(line)
            if between is not None:
                between(d, len(lines) - 1, graph)
        if graph:
            tr.run_epochs(d, None, opt, sched, epochs, True, 0, dev, log, graph=True, batches=b)
        else:
            tr.run_epochs(d, HostOrderLoader(X, Y, b), opt, sched, epochs, True, 0, dev, log)
        out += [state(d, opt), lines]
        assert counters_on_host(d, opt)                                      # back on the host after the run
    assert len(made) == 1
    return out + [made[0]]


@pytest.mark.parametrize("policy,mode", FORMS)
@pytest.mark.parametrize("name", ["tiny", "nu3"])
def test_graph_epochs_are_the_eager_epochs_bit_for_bit(name, policy, mode, monkeypatch):
    """Case 1: three epochs, MultiStepLR milestone at 1, EMA on (ema_start 1, rate 2, warmup_epoch 0): weights, EMA weights and count,
    Adam's moments and step, `_draw_calls` and the logged lines.  The ragged batch runs on a twin handle: nothing is re-captured."""
    s0, log0, s1, log1, sg = run_both(name, policy, mode, monkeypatch)
    print(log1)
    assert log0 == log1 and len(log1) == 3
    assert_same(s0, s1)
    assert s1["calls"] == 9 and s1["step"] == 9.0 and s1["n_averaged"] == 3      # steps 4, 6, 8 passed the EMA gate
    assert (sg.replays, sg.eager_steps, sg.recaptures) == (5, 4, 0)              # 6 full batches (the first one eager), 3 ragged ones


@pytest.mark.parametrize("policy,mode", FORMS)
def test_interleaved_calls_that_reallocate_or_replan(policy, mode, monkeypatch):
    """Case 2: between the epochs, a sample() that fits the workspace (nothing moves), a sample() over 256 rows (the workspaces are freed and
    re-created), and set_precision to the other mode and back (the launch plan changes twice; setting the held mode changes nothing).
    Without the generation check the next replay would run on freed memory; with it the results are the eager loop's, which makes the same
    calls."""
    name = "nu3"
    other = "f32" if mode == "split_f16" else "split_f16"
    cond = torch.rand(256, CONFIGS[name]["cond_dim"], generator=torch.Generator().manual_seed(2)).cuda()
    moves = {False: [], True: []}

    def between(d, epoch, graph):
        g = [generation(d)]
        if epoch == 0:
            d.sample(cond[:32], 1.0, seed=4)
            g.append(generation(d))
            d.sample(cond, 1.0, seed=5)
            g.append(generation(d))
            moves[graph].append((g[1] == g[0], g[2] > g[1]))
        elif epoch == 1:
            for m in (mode, other, other, mode):
                d.model.set_precision(m)
                g.append(generation(d))
            moves[graph].append((g[1] == g[0], g[2] > g[1], g[3] == g[2], g[4] > g[3]))

    s0, log0, s1, log1, sg = run_both(name, policy, mode, monkeypatch, between)
    assert moves[False] == moves[True] == [(True, True), (True, True, True, True)], moves
    assert log0 == log1
    assert_same(s0, s1)
    assert sg.recaptures >= 2 and sg.replays + sg.eager_steps == 9, (sg.recaptures, sg.replays, sg.eager_steps)


def one_step(d, opt, y, cond):
    loss = d(y, cond)
    loss.backward()
    opt.step()
    opt.zero_grad()
    return float(loss.detach())


def fixed_batch(name, rows=BS):
    X, Y = data(name, rows)
    return Y.cuda(), X.cuda()


@pytest.mark.parametrize("policy,mode", FORMS)
def test_a_host_side_weight_change_between_replays(policy, mode):
    """Case 3, at StepGraph level: load_state_dict of a perturbed copy between two replays.  The captured re-pack sits at the end of the
    graph: without the refresh in step() the next replay runs forward and backward on the old packed weights -- one silently wrong step."""
    from diffsg_amd.train import StepGraph
    name = "tiny"
    y, cond = fixed_batch(name)
    (d0, o0, _), (d1, o1, _) = setup(name, policy, mode), setup(name, policy, mode)
    sg = StepGraph(d1, o1, y, cond, warmup=1)
    got = [float(sg.step().detach()) for _ in range(2)]
    ref = [one_step(d0, o0, y, cond) for _ in range(3)][1:]
    assert got == ref
    g = torch.Generator().manual_seed(8)
    pert = {k: v.cpu() + 0.05 * torch.randn(v.shape, generator=g) for k, v in d0.model.state_dict().items()}
    d0.model.load_state_dict(pert)
    d1.model.load_state_dict(pert)
    got = [float(sg.step().detach()) for _ in range(2)]
    ref = [one_step(d0, o0, y, cond) for _ in range(2)]
    assert got == ref, (got, ref)
    assert sg.recaptures == 0 and sg.replays == 4
    sg.close()
    assert_same(state(d0, o0), state(d1, o1))


@pytest.mark.parametrize("lazy", [False, True])
def test_a_capture_that_fails_leaves_nothing_behind(lazy, monkeypatch):
    """Case 4: torch.cuda.graph raises.  The counters are those of the steps that ran, on the host; the eager loop continued from there is
    the eager loop that never tried."""
    from diffsg_amd.train import StepGraph
    name = "tiny"
    y, cond = fixed_batch(name)
    (d0, o0, _), (d1, o1, _) = setup(name), setup(name)

    class Refused:
        def __init__(self, *a, **k):
            raise RuntimeError("capture refused")
    monkeypatch.setattr(torch.cuda, "graph", Refused)
    with pytest.raises(RuntimeError, match="capture refused"):
        if lazy:
            StepGraph(d1, o1, y, cond, warmup=0).step()                      # one eager step, then the capture
        else:
            StepGraph(d1, o1, y, cond, warmup=2)
    monkeypatch.undo()
    ran = 1 if lazy else 2
    assert d1._draw_calls == ran and float(o1.state[o1._flat]["step"]) == ran
    assert counters_on_host(d1, o1)
    got = [one_step(d1, o1, y, cond) for _ in range(2)]
    ref = [one_step(d0, o0, y, cond) for _ in range(ran + 2)]
    assert got == ref[ran:]
    assert_same(state(d0, o0), state(d1, o1))


def test_the_dyn_step_refuses_a_shape_before_it_enqueues():
    """Case 5: the net with 267 tracked gradient tensors (kMaxGmax = 256).  dsg_train_step_seeded_dyn returns the error and the device call
    counter, the bucket and the loss word are what they were."""
    import shape_ref as S
    from diffsg_amd import _lib
    from test_gpu_shapes import make_ddpm as shape_ddpm
    d = shape_ddpm("gmax267")
    L, hd = _lib.lib(), d.model.native_handle()
    y, c2 = (t.cuda() for t in S.train_inputs("gmax267")[:2])
    calls = torch.tensor([5], dtype=torch.int64, device="cuda")
    bucket = torch.full((L.dsg_param_total(hd),), 7.0, device="cuda")
    loss = torch.full((1,), 7.0, device="cuda")
    rc = L.dsg_train_step_seeded_dyn(hd, _lib.ptr(y), _lib.ptr(c2), 77, _lib.ptr(calls), 0.9, _lib.ptr(d.sqrt_alphas_cumprod),
                                     _lib.ptr(d.sqrt_one_minus_alphas_cumprod), S.T, _lib.ptr(bucket), _lib.ptr(loss), S.B, _lib.stream_ptr())
    msg = L.dsg_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0 and "gradient tensors" in msg and "267" in msg, msg
    assert int(calls) == 5
    assert bool((bucket == 7.0).all()) and float(loss) == 7.0


def test_train_ddpm_nu_with_the_graph(tmp_path):
    """Case 6: the entry point end to end on the 200-row fixture (140 training rows: two batches of 64 and one of 12): runs, saves, loads
    strictly and samples; the same seeds give the same weights."""
    from diffsg_amd import classifier_free_NU as NU, entry
    csv = os.path.join(GOLD, "data", "3u_18mW_200samples.csv")
    runs = []
    for _ in range(2):
        logs = []
        torch.manual_seed(4)                                                 # init_weights draws from the global generator
        m = entry.train_ddpm("nu", csv, epochs=2, batch_size=64, log=logs.append, graph=True, seed=0)    # train_ddpm_nu + the two options
        assert len(logs) == 2 and all(np.isfinite(float(ln.split("Loss:")[1])) for ln in logs), logs
        assert m.device_draws == 0 and m._draw_calls == 6 and getattr(m, "_call_dev", None) is None
        runs.append(torch.cat([p.detach().reshape(-1) for p in m.model.parameters()]).clone())
    assert torch.equal(runs[0], runs[1])
    ck = str(tmp_path / "ddpm_nu.pt")
    torch.save(m.state_dict(), ck)
    fresh = NU.build_model(3, 18.0, torch.device("cuda:0"), 20, {"width": 400, "height": 400})
    fresh.load_state_dict(torch.load(ck, map_location="cpu"), strict=True)
    out = NU.load_test_nu(ck, csv, omega=1.0, log=logs.append)
    assert np.isfinite(out["less_ratio"])


@pytest.mark.parametrize("policy,mode", FORMS)
def test_lazy_capture_makes_no_step_of_its_own(policy, mode):
    """Case 7: StepGraph(warmup=0) runs nothing in its constructor; N calls are N eager steps (the first one eager, then replays)."""
    from diffsg_amd.train import StepGraph
    name, n = "tiny", 5
    y, cond = fixed_batch(name)
    (d0, o0, _), (d1, o1, _) = setup(name, policy, mode), setup(name, policy, mode)
    sg = StepGraph(d1, o1, y, cond, warmup=0)
    assert d1._draw_calls == 0 and len(o1.state) == 0 and counters_on_host(d1, o1)
    got = [float(sg.step().detach()) for _ in range(n)]
    ref = [one_step(d0, o0, y, cond) for _ in range(n)]
    assert got == ref
    assert (sg.eager_steps, sg.replays, sg.recaptures) == (1, n - 1, 0)
    sg.close()
    assert_same(state(d0, o0), state(d1, o1))


@pytest.mark.parametrize("mode", ["split_f16", "f32"])
def test_an_eager_step_of_another_batch_size_on_the_same_handle_invalidates_the_capture(mode):
    """The per-batch-size tables of the training step are rewritten in place by a step of another size on the primary handle (a plain
    `ddpm(y, c)` between replays, not `step_on`, which goes to a twin): the generation moves, the next step() runs eagerly and re-captures,
    and the sequence is the eager one."""
    from diffsg_amd.train import StepGraph
    name = "tiny"
    y, cond = fixed_batch(name)
    y22, cond22 = fixed_batch(name, 22)
    (d0, o0, _), (d1, o1, _) = setup(name, "default", mode), setup(name, "default", mode)
    order = [(y, cond), (y, cond), (y22, cond22), (y, cond), (y, cond)]
    ref = [one_step(d0, o0, *b) for b in order]
    sg = StepGraph(d1, o1, y, cond, warmup=1)
    got = [float(sg.step().detach())]                                         # (the warm-up step's loss is compared through the state)
    g0 = generation(d1)
    got.append(one_step(d1, o1, y22, cond22))                                 # the dyn path on the primary handle, 22 rows
    assert generation(d1) > g0
    got += [float(sg.step().detach()) for _ in range(2)]
    assert got == ref[1:], (got, ref)
    assert (sg.recaptures, sg.replays, sg.eager_steps) == (1, 2, 1)
    sg.close()
    assert_same(state(d0, o0), state(d1, o1))


def test_a_split_size_batch_is_refused_while_the_counters_are_on_the_device():
    """An eager batch that would run as two halves draws with a by-value call number: with a StepGraph live it would leave the device
    counter behind the host mirror, so DDPM.forward refuses it and moves nothing."""
    from diffsg_amd.train import StepGraph
    name = "tiny"
    y, cond = fixed_batch(name)
    y2, cond2 = fixed_batch(name, 128)
    d, opt, _ = setup(name)
    d.train_split_min_rows = 128
    sg = StepGraph(d, opt, y, cond, warmup=1)
    sg.step()
    with pytest.raises(RuntimeError, match="two halves"):
        d(y2, cond2)
    torch.cuda.synchronize()
    assert d._draw_calls == 2 and int(d._call_dev) == 2
    sg.close()
    d(y2, cond2)                                                             # fine again on the host counters
    assert d._draw_calls == 3
