"""Training from device-resident data through the captured step graph, without a device: the C ABI declares `dsg_generation`, the
batch order of `train.DeviceBatches` (run on CPU tensors here), the `graph` / `seed` arguments of the entry points, the refusals of
`run_epochs(graph=True)` -- all raised before anything touches a device --, and the call sequence of the default path
(`graph=False`), which is the parent's."""
import inspect
import os
import re

import pytest
import torch

from _util import ROOT
from test_steps_cpu import make_ddpm


# ------------------------------------------------------------------------------------------------ C ABI
def test_header_and_binding_declare_the_generation_counter():
    from diffsg_amd import _lib
    with open(os.path.join(ROOT, "include", "diffsg.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    m = re.search(r"\bunsigned\s+long\s+long\s+dsg_generation\s*\(([^()]*)\)\s*;", hdr)
    assert m, "include/diffsg.h does not declare `unsigned long long dsg_generation(...)`"
    assert [a.strip() for a in m.group(1).split(",")] == ["const dsg_handle* h"]          # one handle, no stream
    import ctypes
    res, args = _lib._SIGS["dsg_generation"]
    assert res is ctypes.c_ulonglong and args == [ctypes.c_void_p]
    assert hasattr(_lib.lib(), "dsg_generation")
    assert _lib.lib().dsg_generation(None) == 0                                              # a null handle: 0, no crash
    import test_streams_cpu as S
    assert "dsg_generation" not in S.stream_functions()


# ------------------------------------------------------------------------------------------------ DeviceBatches
def batches(n=150, bs=64, seed=5):
    from diffsg_amd.train import DeviceBatches
    X = torch.arange(n, dtype=torch.float32)[:, None].repeat(1, 3)          # row r holds the value r
    return DeviceBatches(X, X[:, :2] + 0.5, bs, seed, "cpu")


@pytest.mark.parametrize("n,bs", [(150, 64), (128, 64), (7, 3), (5, 8), (1, 1)])
def test_device_batches_order(n, bs):
    state = torch.get_rng_state()
    a, b = batches(n, bs), batches(n, bs)
    assert len(a) == -(-n // bs)
    seen = []
    for e in range(3):
        idx = list(a.epoch(e))
        assert [i.numel() for i in idx] == [bs] * (n // bs) + ([n % bs] if n % bs else [])     # the ragged last batch, as drop_last=False
        flat = torch.cat(idx)
        assert flat.dtype == torch.int64 and sorted(flat.tolist()) == list(range(n))              # a permutation of range(n)
        assert all(i.untyped_storage().data_ptr() == idx[0].untyped_storage().data_ptr() for i in idx)   # views of ONE uploaded permutation
        assert a.host_order(e) == [i.tolist() for i in idx]
        assert b.host_order(e) == a.host_order(e)                                                  # two instances with one seed agree
        seen.append(flat.tolist())
    if n > 5:                                                                                      # (5 rows: two of 120 orders may coincide)
        assert seen[0] != seen[1] and seen[1] != seen[2]                                           # epochs differ
    assert a.host_order(0) == [seen[0][i:i + bs] for i in range(0, n, bs)]                        # an earlier epoch again: the same order
    assert batches(n, bs, seed=6).host_order(0) != a.host_order(0) or n <= 4
    assert torch.equal(torch.get_rng_state(), state)                                               # the global generator is untouched


def test_device_batches_fill_and_take():
    a = batches()
    idx = list(a.epoch(1))
    c, y = torch.empty(64, 3), torch.empty(64, 2)
    a.fill(idx[0], c, y)
    want = torch.tensor(a.host_order(1)[0], dtype=torch.float32)
    assert torch.equal(c[:, 0], want) and torch.equal(y[:, 1], want + 0.5)
    x22, y22 = a.take(idx[-1])
    assert x22.shape == (22, 3) and y22.shape == (22, 2) and x22[:, 0].tolist() == [float(v) for v in a.host_order(1)[-1]]
    from diffsg_amd.train import DeviceBatches
    with pytest.raises(ValueError, match="conditions and"):
        DeviceBatches(torch.zeros(3, 2), torch.zeros(4, 2), 2)
    with pytest.raises(ValueError, match="batch_size"):
        DeviceBatches(torch.zeros(3, 2), torch.zeros(3, 2), 0)


# ------------------------------------------------------------------------------------------------ entry points
def test_the_entry_points_take_graph_and_seed(monkeypatch):
    """`entry.train` and `entry.train_ddpm(problem, ...)` take `graph=False, seed=None`.  `train_ddpm_{msr,co,nu}` themselves keep the
    reference's signatures, which tests/test_entry_cpu.py pins: `entry.train_ddpm` is those calls, with their defaults, plus the options."""
    from diffsg_amd import classifier_free_CO, classifier_free_MSR, classifier_free_NU, entry, train
    p = inspect.signature(entry.train).parameters
    assert p["graph"].default is False and p["seed"].default is None and list(p)[-2:] == ["graph", "seed"]
    p = inspect.signature(entry.train_ddpm).parameters
    assert p["graph"].default is False and p["seed"].default is None
    assert p["graph"].kind is p["seed"].kind is inspect.Parameter.KEYWORD_ONLY
    for problem, mod in (("msr", classifier_free_MSR), ("co", classifier_free_CO), ("nu", classifier_free_NU)):
        public = getattr(mod, "train_ddpm_" + problem)
        names = list(inspect.signature(public).parameters)
        assert "graph" not in names and "seed" not in names
        assert list(inspect.signature(mod._train).parameters) == names + ["graph", "seed"]      # the public arguments, in order, then the two
        seen = []
        monkeypatch.setattr(mod, "_train", lambda *a, **k: seen.append((a, k)))
        public("some.csv", 7, batch_size=64)
        entry.train_ddpm(problem, "some.csv", 7, batch_size=64)
        entry.train_ddpm(problem, "some.csv", 7, batch_size=64, graph=True, seed=3)
        defaults = tuple(q.default for q in inspect.signature(public).parameters.values())
        want = ("some.csv", 7) + defaults[2:5] + (64,) + defaults[6:]
        assert seen == [(want, {}), (want, {"graph": False, "seed": None}), (want, {"graph": True, "seed": 3})], problem
    with pytest.raises(ValueError, match="problem"):
        entry.train_ddpm("uav")
    p = inspect.signature(train.run_epochs).parameters
    assert p["graph"].default is False and p["batches"].default is None and list(p)[-2:] == ["graph", "batches"]
    assert inspect.signature(train.StepGraph.__init__).parameters["warmup"].default == 3


# ------------------------------------------------------------------------------------------------ refusals of graph=True
def cpu_setup(plain_adam=False):
    from diffsg_amd import train as tr
    d = make_ddpm(8)
    d.device_draws = 7
    opt = torch.optim.Adam(d.model.parameters(), lr=1e-3) if plain_adam else tr.FlatAdam(d, lr=1e-3, fused=False)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, [5])
    b = tr.DeviceBatches(torch.zeros(10, 3), torch.zeros(10, 3), 4, 0, "cpu")
    return tr, d, opt, sched, b


def test_run_epochs_graph_refusals_need_no_device():
    tr, d, opt, sched, b = cpu_setup()
    run = lambda **kw: tr.run_epochs(d, None, kw.pop("opt", opt), sched, 1, False, 5, torch.device("cpu"), lambda *_: None, graph=True, **kw)
    d.device_draws = None
    with pytest.raises(ValueError, match="device-side draws"):
        run(batches=b)
    d.device_draws = 7
    with pytest.raises(ValueError, match="DeviceBatches"):
        run()
    with pytest.raises(ValueError, match="DeviceBatches"):
        run(batches=[(torch.zeros(4, 3), torch.zeros(4, 3))])
    tr2, d2, adam, sched2, b2 = cpu_setup(plain_adam=True)
    with pytest.raises(ValueError, match="FlatAdam"):
        tr2.run_epochs(d2, None, adam, sched2, 1, False, 5, torch.device("cpu"), lambda *_: None, graph=True, batches=b2)
    d.train_split_min_rows = 4                                               # the batch would run as two halves
    b128 = tr.DeviceBatches(torch.zeros(300, 3), torch.zeros(300, 3), 128, 0, "cpu")
    with pytest.raises(ValueError, match="two halves"):
        run(batches=b128)
    assert d._draw_calls == 0 and len(opt.state) == 0                        # nothing ran


def _world2_worker(rank, ws, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(ws))
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    try:
        tr, d, opt, sched, b = cpu_setup()
        try:
            tr.run_epochs(d, None, opt, sched, 1, False, 5, torch.device("cpu"), lambda *_: None, graph=True, batches=b)
            q.put((rank, "run_epochs(graph=True) returned in a process group of 2"))
        except ValueError as e:
            q.put((rank, "ok" if "single-process" in str(e) and "graph=False" in str(e) else str(e)))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_run_epochs_graph_refuses_a_process_group_of_two():
    import torch.multiprocessing as mp
    from test_distributed_cpu import _free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_world2_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=150) for _ in procs]
    for p in procs:
        p.join(30)
    assert sorted(r for r, _ in res) == [0, 1]
    for r, msg in res:
        assert msg == "ok", f"rank {r}:\n{msg}"


# ------------------------------------------------------------------------------------------------ the default path is the parent's
class _Recorder:
    """Stand-ins for the model, the optimizer and the scheduler that only record what `run_epochs` asks of them."""

    def __init__(self, monkeypatch, tr):
        self.calls = calls = []

        class Loss:
            def __init__(self, v):
                self.v = v

            def backward(self):
                calls.append("backward")

            def item(self):
                calls.append("item")
                return self.v

        class Ema:
            def update_parameters(self, model):
                calls.append("ema")

        class Model:
            ema_start, ema_update_rate, ema, model = 1, 2, Ema(), object()

            def __call__(self, y, x):
                calls.append(("forward", y[:, 0].tolist(), x[:, 0].tolist()))
                return Loss(float(len(calls)))

            def allreduce_grads(self):
                calls.append("allreduce")

        class Opt:
            def step(self):
                calls.append("opt.step")

            def zero_grad(self):
                calls.append("zero_grad")

        class Sched:
            def step(self):
                calls.append("sched.step")

        self.model, self.opt, self.sched = Model(), Opt(), Sched()
        monkeypatch.setattr(tr, "step_health", lambda m, v, dev, world, where="": calls.append(("health", v, world, where)))
        self.log = lambda s: calls.append(("log", s))


def expected_calls(order, use_ema, warmup_epoch, ema_start=1, ema_rate=2):
    """The parent's loop body, written out: classifier_free_MSR.py:217-234 with the all-reduce hook, loss.item() and step_health."""
    out, n, cnt = [], 0, 1
    for epoch, batches_ in enumerate(order):
        total, rows = 0.0, 0
        for idx in batches_:
            vals = [float(i) for i in idx]
            out += [("forward", [v + 0.5 for v in vals], vals), "backward", "allreduce", "opt.step", "zero_grad"]
            loss = float(len(out) - 4)
            if use_ema and epoch > warmup_epoch and cnt > ema_start and cnt % ema_rate == 0:
                out.append("ema")
            out += ["item", ("health", loss, 1, f"epoch {epoch}")]
            total += loss
            rows += len(idx)
            cnt += 1
        out += [("log", f"Epoch: {epoch}, Loss: {total / rows}"), "sched.step"]
    return out


@pytest.mark.parametrize("use_ema", [False, True])
def test_the_default_path_issues_the_parents_calls_in_the_parents_order(monkeypatch, use_ema):
    from diffsg_amd import train as tr
    b = batches(20, 8)
    order = [b.host_order(e) for e in range(2)]

    class Loader:                                                            # a loader with a per-epoch order, as DistributedSampler's
        def __init__(self):
            self.sampler, self.e = self, 0

        def set_epoch(self, e):
            self.e = e

        def __iter__(self):
            return iter([(b.X[i], b.Y[i]) for i in order[self.e]])

    r = _Recorder(monkeypatch, tr)
    tr.run_epochs(r.model, Loader(), r.opt, r.sched, 2, use_ema, 0, torch.device("cpu"), r.log)          # the parent's nine arguments
    want = expected_calls(order, use_ema, 0)
    assert r.calls == want
    assert ("ema" in want) == use_ema
    # the same loop fed from DeviceBatches (graph=False, batches=...): the same calls on the same batches
    r2 = _Recorder(monkeypatch, tr)
    tr.run_epochs(r2.model, None, r2.opt, r2.sched, 2, use_ema, 0, torch.device("cpu"), r2.log, graph=False, batches=b)
    assert r2.calls == want
