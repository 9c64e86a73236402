"""The entry points without a device: the public signatures of the problem modules, trajectory.py and the sampling methods are the ones
of the commit before the helpers were shared (diffsg_amd/entry.py), `entry.sample_in_batches` makes the calls the three evaluation loops
made, and `ddpm.best_calls` lists the calls of `sample_best` with their seeds in round-major order."""
import importlib
import inspect

import torch

from test_steps_cpu import make_ddpm

# str(inspect.signature(f)) of every public function, recorded from the commit before diffsg_amd/entry.py existed
SIGNATURES = {
    "classifier_free_MSR.build_model": "(M, cond_dim, device, T=20, custom_config=None, W=10.0)",
    "classifier_free_MSR.custom_decoder": "(Y_pred)",
    "classifier_free_MSR.load_test_msr": "(ckpt_path, dataset_path='../datasets/3c_10w_10000samples.csv', T=20, omega=500, batch_size=512, log=<built-in function print>, repeats=1, steps=None, sampler='strided', eta=0.0, variants=None)",
    "classifier_free_MSR.load_test_msr_debug": "(ckpt_path, dataset_path='../datasets/3c_10w_10000samples.csv', T=20, omega=150, want2look=(0, 1, 2, 3, 4, 5, 6, 7, 8, 9), log=<built-in function print>)",
    "classifier_free_MSR.msr_data_load": "(dataset_path)",
    "classifier_free_MSR.train_ddpm_msr": "(dataset_path='../datasets/3c_10w_10000samples.csv', epochs=200, T=20, use_ema=False, warmup_epoch=5, batch_size=512, lr=0.005, milestones=(100, 150), log=<built-in function print>)",
    "classifier_free_CO.build_model": "(node_num, cond_dim, device, T=20, custom_config=None)",
    "classifier_free_CO.co_data_load": "(dataset_path)",
    "classifier_free_CO.cost_calc": "(X, Y)",
    "classifier_free_CO.customized_real_decoder": "(Y_pred)",
    "classifier_free_CO.data_preprocess_co": "(X)",
    "classifier_free_CO.load_test_co": "(ckpt_path, dataset_path='../datasets/3nodes_50000samples_new.csv', T=20, omega=500.0, batch_size=512, log=<built-in function print>, repeats=1, steps=None, sampler='strided', eta=0.0, variants=None)",
    "classifier_free_CO.load_test_co_debug": "(ckpt_path, dataset_path='../datasets/3nodes_50000samples_new.csv', T=400, omega=150.0, batch_size=512, want2look=(0, 1, 2, 3, 4, 5, 6, 7, 8, 9), log=<built-in function print>)",
    "classifier_free_CO.test_ddpm": "(ckpt_path=None, T=500, omega=30.0, batch_size=512, diffusion_model=None, data_split=None, log=<built-in function print>)",
    "classifier_free_CO.train_ddpm_co": "(dataset_path='../datasets/3nodes_50000samples_new.csv', epochs=200, T=20, use_ema=False, warmup_epoch=5, batch_size=512, lr=0.005, milestones=(15, 80, 150), log=<built-in function print>)",
    "classifier_free_CO.validate_ddpm_co": "(epochs=500, T=500, use_ema=False, warmup_epoch=5, batch_size=512, lr=0.005, milestones=(30, 150, 350), data_split=None, log=<built-in function print>)",
    "classifier_free_CO.validation_data_gen": "()",
    "classifier_free_NU.build_model": "(K, P_sum, device, T=20, custom_config=None)",
    "classifier_free_NU.custom_decoder": "(Y_pred, width, height, P_sum)",
    "classifier_free_NU.load_test_nu": "(ckpt_path, dataset_path='../datasets/3u_18mW_10000samples.csv', T=20, omega=500, batch_size=512, width=400, height=400, log=<built-in function print>, repeats=1, steps=None, sampler='strided', eta=0.0, variants=None)",
    "classifier_free_NU.load_test_nu_debug": "(*args, **kw)",
    "classifier_free_NU.nu_data_load": "(dataset_path, width, height)",
    "classifier_free_NU.rate_calc": "(Y_pred_decoded, X)",
    "classifier_free_NU.train_ddpm_nu": "(dataset_path='../datasets/3u_18mW_10000samples.csv', epochs=200, T=20, use_ema=False, warmup_epoch=5, batch_size=512, lr=0.004, milestones=(80, 200), width=400, height=400, log=<built-in function print>)",
    "trajectory.co_trajectory_gen_store": "(ckpt_path='../ckpts/ddpm_co.pt', dataset_path='../datasets/3nodes_50000samples_new.csv', out_csv='../results/co_denoise_path.csv', T=20, omega=500, batch_size=512, diffusion_model=None, log=<built-in function print>)",
    "trajectory.msr_trajectory_gen_store": "(ckpt_path='../ckpts/ddpm_msr_3c.pt', dataset_path='../datasets/3c_10w_10000samples.csv', out_csv='../results/msr_denoise_path.csv', T=20, omega=500, diffusion_model=None, log=<built-in function print>)",
    "trajectory.nu_dataset_store": "(out_csv=None, sample_num=2500, P_sum=18, extend=False, ext_csv=None, qs=None, log=<built-in function print>)",
    "trajectory.nu_trajectory_gen_store": "(ckpt_path='../ckpts/ddpm_nu_3u.pt', dataset_path='../datasets/3u_18mW_10000samples.csv', out_csv='../results/nu_denoise_path.csv', T=20, omega=500, width=400, height=400, diffusion_model=None, log=<built-in function print>)",
    "trajectory.record_trajectories": "(diffusion_model, X_test, omega, batch_size=None, steps=None, sampler='strided', eta=0.0)",
    "trajectory.sum_rate_dataset_store": "(out_csv=None, sample_num=2000, M=80, W=20.0, g_range=(0.5, 2.5), gs=None, log=<built-in function print>)",
    "DDPMCore.sample": "(self, cond, omega=1.0, *, y_T=None, noise=None, seed=None, host_rng=False, use_graph=True, profile=False, check_range=True, plan=None)",
    "DDPMCore.sample_chunked": "(self, cond, omega=1.0, chunk_rows=512, *, seeds=None, y_T=None, noise=None, use_graph=True, check_range=True, plan=None, variants=None)",
    "DDPMCore.sample_best": "(self, cond, X, n, omega=1.0, *, seeds=None, chunk_rows=None, max_rows=65536, use_graph=True, check_range=True, return_objectives=False, plan=None, variants=None)",
    "DDPMCore.refine": "(self, cond, y_start, k, omega=1.0, *, q_noise=None, noise=None, seed=None, **kw)",
    "DDPMCore.sample_checked": "(self, cond, omega=1.0, **kw)",
    "DDPMCore.sample_chunked_checked": "(self, cond, omega=1.0, chunk_rows=512, **kw)",
}


def test_public_signatures_are_the_recorded_ones():
    """Every public function the four modules define (no more, no fewer) and the six sampling methods: names, order, defaults."""
    from diffsg_amd.ddpm import DDPMCore
    now = {}
    for mod in ("classifier_free_MSR", "classifier_free_CO", "classifier_free_NU", "trajectory"):
        m = importlib.import_module("diffsg_amd." + mod)
        for name, f in vars(m).items():
            if not name.startswith("_") and inspect.isfunction(f) and f.__module__ == m.__name__:
                now[f"{mod}.{name}"] = str(inspect.signature(f))
        assert mod == "trajectory" or callable(m._device)          # the modules' own name for entry.device stays importable
    for name in ("sample", "sample_chunked", "sample_best", "refine", "sample_checked", "sample_chunked_checked"):
        now["DDPMCore." + name] = str(inspect.signature(getattr(DDPMCore, name)))
    assert set(now) == set(SIGNATURES), sorted(set(now) ^ set(SIGNATURES))
    for k, v in SIGNATURES.items():
        assert now[k] == v, k


def recording_model(monkeypatch, D=3):
    """A DDPM on the CPU whose two device entry points record their calls -- (method, rows as (first value, count), omega, chunk_rows or
    None, keywords) -- and return zeros; row r of the inputs used with it holds the value r."""
    d = make_ddpm(8)
    calls = []

    def rows(cond):
        return (int(cond[0, 0]), cond.shape[0]) if cond.shape[0] else (0, 0)

    def fake_sample(self, cond, omega=1.0, **kw):
        calls.append(("sample", rows(cond), float(omega), None, kw))
        return torch.zeros(cond.shape[0], D)

    def fake_chunked(self, cond, omega=1.0, chunk_rows=512, **kw):
        calls.append(("sample_chunked", rows(cond), float(omega), chunk_rows, kw))
        return torch.zeros(cond.shape[0], D)

    for cls in (type(d).__mro__[1], type(d)):
        monkeypatch.setattr(cls, "sample", fake_sample)
        monkeypatch.setattr(cls, "sample_chunked", fake_chunked)
    return d, calls


def test_sample_in_batches_makes_the_calls_of_the_evaluation_loops(monkeypatch):
    from diffsg_amd.entry import sample_in_batches
    d, calls = recording_model(monkeypatch)
    X = torch.arange(60, dtype=torch.float32)[:, None].repeat(1, 3)
    plan = object()
    # on the 32-row tile: ONE chunked call over all rows
    assert sample_in_batches(d, X, 500, 32, plan).shape == (60, 3)
    assert calls == [("sample_chunked", (0, 60), 500.0, 32, {"plan": plan})]
    # off the tile: the serial calls, rows 0:48 and 48:60
    calls.clear()
    assert sample_in_batches(d, X, 2.0, 48, plan).shape == (60, 3)
    assert calls == [("sample", (0, 48), 2.0, None, {"plan": plan}), ("sample", (48, 12), 2.0, None, {"plan": plan})]
    # batch >= rows: what the loops did -- the chunked call on the tile (sample_chunked itself turns one chunk into a sample() call),
    # one serial call off it; no plan is plan=None
    calls.clear()
    sample_in_batches(d, X, 1.0, 64)
    sample_in_batches(d, X, 1.0, 60)
    sample_in_batches(d, X, 1.0, 100)
    assert calls == [("sample_chunked", (0, 60), 1.0, 64, {"plan": None}), ("sample", (0, 60), 1.0, None, {"plan": None}),
                     ("sample", (0, 60), 1.0, None, {"plan": None})]


def test_best_calls_pin_the_order_of_the_seed_slices():
    from diffsg_amd.ddpm import best_calls
    key = lambda calls: [(c.kind, c.round0, c.rounds, c.chunk, (c.seeds.start, c.seeds.stop)) for c in calls]
    # two 32-row chunks per round, two rounds fit into 128 rows: one group of two rounds, then one round
    calls = best_calls(3, 64, 32, 128, None, 7.0, "p")
    assert key(calls) == [("chunked", 0, 2, 32, (0, 4)), ("chunked", 2, 1, 32, (4, 6))]
    assert all((c.omega, c.plan, c.variants) == (7.0, "p", None) for c in calls)
    # chunks off the tile: the serial path, round by round, two seeds each
    assert key(best_calls(3, 64, 48, 128)) == [("serial", 0, 1, 48, (0, 2)), ("serial", 1, 1, 48, (2, 4)), ("serial", 2, 1, 48, (4, 6))]
    # no chunks: a round is one sample() call -- grouped into chunked calls of 64-row chunks while they fit, one seed per round
    assert key(best_calls(3, 64, None, 128)) == [("chunked", 0, 2, 64, (0, 2)), ("sample", 2, 1, 64, (2, 3))]
    assert key(best_calls(3, 64, None, 64)) == [("sample", r, 1, 64, (r, r + 1)) for r in range(3)]
    assert key(best_calls(2, 60, None, 65536)) == [("sample", r, 1, 60, (r, r + 1)) for r in range(2)]       # 60 rows are off the tile
    # variants: round r has variants[r % 2]; a group carries them per chunk and reads no omega / plan of its own
    va, vb = (2.0, "a"), (-1.0, "b")
    calls = best_calls(3, 64, 32, 128, [va, vb])
    assert key(calls) == [("chunked", 0, 2, 32, (0, 4)), ("chunked", 2, 1, 32, (4, 6))]
    assert (calls[0].omega, calls[0].plan, calls[0].variants) == (0.0, None, [va, va, vb, vb])
    assert (calls[1].omega, calls[1].plan, calls[1].variants) == (2.0, "a", None)


def test_sample_best_runs_its_call_list_through_sample_and_sample_chunked(monkeypatch):
    """The seeds reach the two entry points in the order of the list, for the three shapes above."""
    from diffsg_amd import repeated
    d, calls = recording_model(monkeypatch)
    monkeypatch.setattr(type(d), "_best_of_problem", lambda self: ("msr", {}))
    monkeypatch.setattr(repeated, "best_of", lambda problem, Y, X, out=None, round0=0, **kw: (out or []) + [(round0, tuple(Y.shape))])

    class FakeCond(torch.Tensor):
        is_cuda = True

    cond = torch.arange(64, dtype=torch.float32)[:, None].repeat(1, 3).as_subclass(FakeCond)
    seeds = list(range(100, 106))
    kw = {"use_graph": True, "check_range": True}
    assert d.sample_best(cond, cond, 3, 7.0, seeds=seeds, chunk_rows=32, max_rows=128) == [(0, (2, 64, 3)), (2, (1, 64, 3))]
    assert calls == [("sample_chunked", (0, 128), 7.0, 32, {"seeds": seeds[:4], "plan": None, "variants": None, **kw}),
                     ("sample_chunked", (0, 64), 7.0, 32, {"seeds": seeds[4:], "plan": None, "variants": None, **kw})]
    calls.clear()
    assert d.sample_best(cond, cond, 3, 7.0, seeds=seeds, chunk_rows=48) == [(r, (1, 64, 3)) for r in range(3)]
    assert [(c[0], c[1], c[4]["seed"]) for c in calls] == [("sample", (0, 48) if k % 2 == 0 else (48, 16), 100 + k) for k in range(6)]
    calls.clear()
    assert d.sample_best(cond, cond, 3, 7.0, seeds=seeds[:3], chunk_rows=None, max_rows=64) == [(r, (1, 64, 3)) for r in range(3)]
    assert [(c[0], c[1], c[4]["seed"]) for c in calls] == [("sample", (0, 64), 100 + r) for r in range(3)]
