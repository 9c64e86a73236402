"""The device's own random draws against their CPU restatement (tests/philox_ref.py): which Philox word belongs to which
element of which step of which call.

(a) `dsg_train_draws` against `philox_ref.train_draws`: ts and mask bit for bit, the noise within the draw bound
    |z_dev - z_ref| <= 8 x unit x max(1, |z_ref|), unit = what a float32 evaluation of Box-Muller is away from the float64 one on the
    same float32 uniforms (tests/test_philox_cpu.py measures it: 2.2e-7).
(b) Sampling with device draws -- the path of the benchmark, `sample_best` and the load tests -- against the oracle in float64 on the
    restated draws, on nets whose last Linear is zeroed (eps == 0: y_0 is a function of the draws, the table and the renorm alone, and
    every operator still runs in every launch form).  Cases and budgets: tests/philox_cases.py; tests/test_philox_cpu.py caps the budgets.

Measured on an MI355X: the draws are at most 1.08 units from the restatement (8 allowed), the sampling cases 3.3e-8 .. 5.4e-7 (budgets
1.0e-6 .. 4.3e-6); the docstrings of the tests that print the figures have the detail.  All tests need an MI355X: run with `-m gpu`."""
import numpy as np
import pytest
import torch

import philox_cases as C
import philox_ref as P
from test_gpu_parity import _device_draws
from oracle import ddpm_oracle as O
from weights import CONFIGS

pytestmark = pytest.mark.gpu


def make_ddpm(net):
    """The case's zeroed net under the plain DDPM class, on the device; the recorded trajectory is the raw states."""
    from diffsg_amd import UNet1D
    from diffsg_amd.classifier_free_MSR import DDPM
    from diffsg_amd.ddpm import DDPMCore
    name, T = C.NETS[net]
    cfg = CONFIGS[name]
    m = UNet1D(**cfg, is_attn=(False,) * len(cfg["dims"]))
    m.load_state_dict(C.zero_net(net)[1], strict=True)
    D = cfg["input_dim"]
    d = DDPM(T, m.to("cuda"), D, 10.0, 1.0 - O.cosine_betas(T), torch.device("cuda"), (1, D), None).to("cuda")
    d._decode_recorded = lambda i, y: DDPMCore._decode_recorded(d, i, y)
    return d


def device_plan(d, case, table=None):
    """The library's plan of a case (of one variant `table` = (kind, eta, renorm count))."""
    from diffsg_amd import steps
    K = C.K_OF.get(case.net)
    if case.kind == "dpmpp":
        return steps.dpmpp_2m(d, K, renorm_steps=case.arg)
    if case.kind == "guided":
        return steps.with_guidance(d, C.G.masks(d.T)[case.arg])
    kind, eta, rn = table if table is not None else (*case.arg, None)
    plan = steps.strided(d, K) if kind == "strided" else steps.ddim(d, K, eta)
    return plan if rn is None else steps.with_renorm(plan, rn)


def check(got, cid, tag=""):
    ref = C.reference(cid)
    e = C.rel(got, ref.y64)
    print(f"{cid} {tag}: rel err vs the oracle on the restated draws {e:.2e} (budget {ref.budget:.2e})")
    assert torch.isfinite(got).all() and e <= ref.budget, (cid, tag, e, ref.budget)
    return e


def run(d, case, **kw):
    cond = C.cond_of(case.net, case.B).cuda()
    g = C.given(case)
    if case.given:
        kw["y_T" if case.given == "y_T" else "noise"] = g
    if case.kind in ("plan", "dpmpp", "guided"):
        kw["plan"] = device_plan(d, case)
    return d.sample(cond, C.OMEGA, seed=case.seed, **kw)


# ------------------------------------------------------------------------------------------------ (a) the training draws
@pytest.mark.parametrize("B,D", [(1, 1), (33, 3), (70, 5), (257, 80)])
def test_training_draws_are_the_restated_draws(B, D):
    """ts and mask bit for bit, noise within the draw bound, over calls {0, 1, 5}, three seeds (two with a live high half), T in
    {1, 7, 1000, 2^24} and keep in {0, 0.5, 0.9, 1}.  Measured on an MI355X: the worst noise deviation is 0.48, 0.70, 0.76 and 0.93
    units at the four shapes (2.07e-7 relative to max(1, |z|) at the largest) and 1.08 units at 2^16 x 80 (the next test), against
    the 8 units allowed: the device's float32 Box-Muller is as close to the float64 one as numpy's float32 one is."""
    unit = C.box_muller_unit()[1]
    worst = 0.0
    for seed in (123, 2 ** 32 + 1, 77 ^ C.FOLD):
        for call in (0, 1, 5):
            for T in (1, 7, 1000, 1 << 24):
                for keep in (0.0, 0.5, 0.9, 1.0):
                    ts, noise, mask = _device_draws(seed, call, T, keep, B, D)
                    ts_ref, z_ref, mask_ref = P.train_draws(seed, call, T, keep, B, D)
                    tag = (hex(seed), call, T, keep)
                    assert ts.dtype == torch.int32 and np.array_equal(ts.cpu().numpy(), ts_ref), tag
                    assert np.array_equal(mask.cpu().numpy(), mask_ref), tag
                    z = noise.cpu().numpy().astype(np.float64)
                    dev = np.abs(z - z_ref) / np.maximum(1.0, np.abs(z_ref))
                    worst = max(worst, float(dev.max()))
                    assert np.isfinite(z).all() and bool((np.abs(z - z_ref) <= C.draw_bound(z_ref)).all()), (tag, float(dev.max()) / unit)
                    if keep in (0.0, 1.0):
                        assert set(mask.unique().tolist()) == {keep}
    print(f"B = {B}, D = {D}: worst noise deviation {worst:.2e} relative to max(1, |z|) = {worst / unit:.2f} units (bound: {C.FACTOR:g} units)")


def test_training_draws_through_the_grid_stride_loop():
    """2^16 x 80 elements: the grid-stride loop of k_train_draws (4096 blocks) -- ts and mask bit for bit, noise within the draw bound."""
    B, D, T, keep = 1 << 16, 80, 20, 0.9
    ts, noise, mask = _device_draws(2 ** 61 + 9, 3, T, keep, B, D)
    ts_ref, z_ref, mask_ref = P.train_draws(2 ** 61 + 9, 3, T, keep, B, D)
    assert np.array_equal(ts.cpu().numpy(), ts_ref) and np.array_equal(mask.cpu().numpy(), mask_ref)
    z = noise.cpu().numpy().astype(np.float64)
    dev = float((np.abs(z - z_ref) / np.maximum(1.0, np.abs(z_ref))).max())
    print(f"2^16 x 80: worst noise deviation {dev / C.box_muller_unit()[1]:.2f} units")
    assert bool((np.abs(z - z_ref) <= C.draw_bound(z_ref)).all())


# ------------------------------------------------------------------------------------------------ (b) sampling
@pytest.mark.parametrize("cid", [c.id for c in C.PLAIN])
def test_plain_calls_with_device_draws(cid):
    """Captured step graphs and eager launches (DSG_SAMPLE_NO_GRAPH), both precision modes on the graph form.  Measured on an MI355X:
    rel err 3.3e-8 (tiny, B = 1) .. 2.5e-7 against budgets of 1.0e-6 .. 2.2e-6, and 5.4e-7 of 4.3e-6 at T = 70; over all the sampling
    cases of this file 3.3e-8 .. 5.4e-7 against 1.0e-6 .. 4.3e-6."""
    case = C.CASE[cid]
    d = make_ddpm(case.net)
    a = run(d, case)
    check(a, cid, "graph")
    b = run(d, case, use_graph=False)
    check(b, cid, "eager")
    assert torch.equal(a, b)
    d.model.set_precision("f32")
    check(run(d, case), cid, "graph f32")
    d.model.set_precision("split_f16")


@pytest.mark.parametrize("cid", [c.id for c in C.MIXED])
def test_one_part_given_and_the_other_drawn_on_the_device(cid):
    case = C.CASE[cid]
    d = make_ddpm(case.net)
    check(run(d, case), cid, "graph")
    check(run(d, case, use_graph=False), cid, "eager")


@pytest.mark.parametrize("cid", [c.id for c in C.REC])
def test_recorded_trajectory_step_by_step(cid):
    """`dsg_sample_rec`: every recorded y against the oracle's state after that step, so that a failure names its step; the recorded eps
    is exactly zero (the zeroed last Linear, on the device)."""
    case = C.CASE[cid]
    d = make_ddpm(case.net)
    D, T = CONFIGS[C.NETS[case.net][0]]["input_dim"], d.T
    d.record_denoise_path = True
    y0 = run(d, case)
    ref = C.reference(cid)
    assert d.y_i_record.shape == (case.B, T * D) and len(ref.steps) == T
    assert not d.eps_i_record.any()
    for k, (step, y64, budget) in enumerate(ref.steps):
        e = C.rel(d.y_i_record[:, k * D:(k + 1) * D], y64)
        print(f"{cid}: step {step}: rel err {e:.2e} (budget {budget:.2e})")
        assert step == T - 1 - k and e <= budget, (step, e, budget)
    assert np.array_equal(d.y_i_record[:, -D:], y0.cpu().numpy())
    check(y0, cid)


@pytest.mark.parametrize("cid", [c.id for c in C.CHUNKED])
def test_chunked_call_draws_per_chunk_with_chunk_local_indices(cid):
    """B = 150 in 64-row chunks (the last of 22 rows), distinct seeds of which one is >= 2^32; then seeds[0] == seeds[1]: chunks 0 and 1
    bit-equal (eps == 0: the conditions do not matter), chunk 2 another draw."""
    case = C.CASE[cid]
    rows = case.arg[0]
    d = make_ddpm(case.net)
    cond = C.cond_of(case.net, case.B).cuda()
    for graph in (True, False):
        check(d.sample_chunked(cond, C.OMEGA, rows, seeds=list(case.seed), use_graph=graph), cid, "graph" if graph else "eager")
    s = list(case.seed)
    y = d.sample_chunked(cond, C.OMEGA, rows, seeds=[s[0], s[0], s[2]])
    tail = case.B - 2 * rows
    assert torch.equal(y[:rows], y[rows:2 * rows]) and not torch.equal(y[2 * rows:], y[:tail])
    assert C.rel(y[:rows], C.reference(cid).y64[:rows]) <= C.reference(cid).budget


@pytest.mark.parametrize("cid", [c.id for c in C.VARIANTS])
def test_chunk_variants_with_device_draws(cid):
    """Three tables (one of them noise free) and three renorm counts in one call, against variants_ref on the restated draws."""
    case = C.CASE[cid]
    rows, var = case.arg
    d = make_ddpm(case.net)
    cond = C.cond_of(case.net, case.B).cuda()
    variants = [(om, device_plan(d, case, (kind, eta, rn))) for om, kind, eta, rn in var]
    for graph in (True, False):
        y = d.sample_chunked(cond, 1.0, rows, seeds=list(case.seed), variants=variants, use_graph=graph)
        check(y, cid, "graph" if graph else "eager")
        ref = C.reference(cid)
        for c, lo in enumerate(range(0, case.B, rows)):                 # a chunk is a call: its error on its own scale
            e = C.rel(y[lo:lo + rows], ref.y64[lo:lo + rows])
            assert e <= ref.budget * float(ref.y64.abs().max() / ref.y64[lo:lo + rows].abs().max()), (c, e)


@pytest.mark.parametrize("cid", [c.id for c in C.PLANS + C.GUIDED])
def test_plans_and_guidance_with_device_draws(cid):
    case = C.CASE[cid]
    d = make_ddpm(case.net)
    check(run(d, case), cid, "graph")
    check(run(d, case, use_graph=False), cid, "eager")


def test_eta_zero_and_seed_changes():
    """ddim(K, 0): only y_T is random -- two seeds differ and each matches its own y_T.  Two seeds that differ only in the high 32 bits
    differ, and each matches its own reference."""
    d = make_ddpm("nu3")
    a, b = (run(d, C.CASE[cid]) for cid in ("nu3-ddim0-a", "nu3-ddim0-b"))
    assert not torch.equal(a, b) and C.rel(a, b) > 0.1
    d = make_ddpm("tiny")
    lo, hi = (run(d, c) for c in C.HIGH)
    check(lo, C.HIGH[0].id)
    check(hi, C.HIGH[1].id)
    assert not torch.equal(lo, hi) and C.rel(lo, hi) > 0.1


def test_folded_rank_seeds_give_uncorrelated_draws():
    """parallel.sample_sharded hands rank r the seed fold_rank(seed, r): two ranks' 70 x 80 results are each the oracle's on their own
    draws, and their sample correlation is below 5 / sqrt(n)."""
    from diffsg_amd import parallel as par
    c0, c1 = C.FOLDED
    assert c1.seed == par.fold_rank(c0.seed, 1) and c0.seed == par.fold_rank(c0.seed, 0)
    d = make_ddpm("msr80")
    y0, y1 = run(d, c0), run(d, c1)
    check(y0, c0.id)
    check(y1, c1.id)
    n = y0.numel()
    r = float(torch.corrcoef(torch.stack((y0.double().flatten(), y1.double().flatten())))[0, 1])
    print(f"sample correlation of two ranks' draws over {n} elements: {r:.4f} (bound {5 / n ** 0.5:.4f})")
    assert n == 70 * 80 and abs(r) < 5 / n ** 0.5
