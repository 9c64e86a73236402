"""Chunk variants without a device: the C ABI declares the setter (no stream), the Python layer refuses malformed variant
lists before any device is touched and maps rounds to variants as documented, `steps.with_renorm` keeps its bounds, the parity cases of
tests/test_gpu_variants.py have the error budgets their bound assumes, and one cell of the best-of-n quality table is pinned with the
CPU oracle."""
import json
import os
import re

import pytest
import torch

import steps_ref as R
import variants_ref as VR
from _util import GOLD, ROOT
from test_steps_cpu import make_ddpm


# ------------------------------------------------------------------------------------------------ C ABI
def test_header_and_binding_declare_the_setter():
    import ctypes
    from diffsg_amd import _lib
    with open(os.path.join(ROOT, "include", "diffsg.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    m = re.search(r"\bint\s+dsg_set_chunk_variants\s*\(([^()]*)\)\s*;", hdr)
    assert m, "include/diffsg.h does not declare dsg_set_chunk_variants"
    assert [a.strip() for a in m.group(1).split(",")] == ["dsg_handle* h", "const float* omega_host", "const int* renorm_host",
                                                          "const int* table_host", "int chunks", "int tables"]
    res, args = _lib._SIGS["dsg_set_chunk_variants"]
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                    ctypes.c_int, ctypes.c_int]
    assert hasattr(_lib.lib(), "dsg_set_chunk_variants")


def test_the_setter_takes_no_stream():
    """By design: a settings call like dsg_set_step_grid (it synchronises the handle's device before it overwrites its buffers)."""
    import test_streams_cpu as S
    assert "dsg_set_chunk_variants" not in S.stream_functions()
    assert "dsg_sample_chunked" in S.stream_functions()


# ------------------------------------------------------------------------------------------------ with_renorm
def test_with_renorm_bounds():
    from diffsg_amd import steps
    T = 8
    d = make_ddpm(T)
    base = steps.ddim(d, 5, 0.5)
    for n in range(0, 6):
        p = steps.with_renorm(base, n)
        assert p.renorm_steps == n and p.taus == base.taus and p.t is base.t and p.coef is base.coef
    ident = steps.with_renorm(d, 0)
    assert ident.taus == tuple(range(T)) and ident.renorm_steps == 0 and ident.coef is d._coef_table()
    assert torch.equal(ident.t, torch.arange(T) / T)
    assert steps.with_renorm(d, T).renorm_steps == T
    for bad in (lambda: steps.with_renorm(base, 6), lambda: steps.with_renorm(base, -1), lambda: steps.with_renorm(base, 1.5),
                lambda: steps.with_renorm(d, T + 1), lambda: steps.with_renorm(d, -1)):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_need_no_device():
    from diffsg_amd import steps
    from diffsg_amd.steps import StepPlan
    T = 8
    d = make_ddpm(T)
    cond = torch.zeros(96, 3)
    a, b = steps.strided(d, 5), steps.ddim(d, 5, 0.5)
    good = [(2.0, a), (-1.0, b), (500.0, steps.with_renorm(a, 0))]
    # wrong length: one variant per chunk
    for v in (good[:2], good + good[:1], []):
        with pytest.raises(ValueError, match="variants"):
            d.sample_chunked(cond, 1.0, 32, variants=v)
    # another grid: differing taus, and the same taus with another t
    other = steps.strided(d, taus=[0, 1, 3, 5, 7])
    assert other.taus != a.taus
    with pytest.raises(ValueError, match="variant 2"):
        d.sample_chunked(cond, 1.0, 32, variants=[good[0], good[1], (2.0, other)])
    shifted = StepPlan(a.taus, a.t + 0.01, a.coef, a.renorm_steps)
    with pytest.raises(ValueError, match="variant 1"):
        d.sample_chunked(cond, 1.0, 32, variants=[good[0], (2.0, shifted), good[2]])
    with pytest.raises(ValueError, match="variant 1"):
        d.sample_chunked(cond, 1.0, 32, variants=[good[0], (2.0, None), good[2]])       # None is all T steps: not the 5-step grid
    with pytest.raises(ValueError, match="variant 1"):
        d.sample_best(cond, cond, 4, variants=[good[0], (2.0, other)])
    # a noisy last step in one of the tables
    coef = b.coef.clone()
    coef[1, 3] = 1.0
    noisy = StepPlan(b.taus, b.t, coef, b.renorm_steps)
    with pytest.raises(ValueError, match="variant 2.*noise free"):
        d.sample_chunked(cond, 1.0, 32, variants=[good[0], good[1], (2.0, noisy)])
    with pytest.raises(ValueError, match="variant 0.*noise free"):
        d.sample_best(cond, cond, 2, variants=[(2.0, noisy)])
    # injected noise has the variants' step count
    with pytest.raises(ValueError, match="noise must have shape"):
        d.sample_chunked(cond, 1.0, 32, variants=good, noise=torch.zeros(T - 2, 96, 3))
    # a plan beside variants, something that is no pair, no rounds
    with pytest.raises(ValueError):
        d.sample_chunked(cond, 1.0, 32, variants=good, plan=a)
    with pytest.raises(ValueError):
        d.sample_best(cond, cond, 2, variants=good, plan=a)
    with pytest.raises(ValueError, match="variant 1"):
        d.sample_chunked(cond, 1.0, 32, variants=[good[0], 2.0, good[2]])
    for n in (0, -3):
        with pytest.raises(ValueError, match="n must be at least 1"):
            d.sample_best(cond, cond, n, variants=good)
    with pytest.raises(ValueError):
        d.sample_best(cond, cond, 2, variants=[])
    # the trajectory ring belongs to one call
    d.record_denoise_path = True
    with pytest.raises(RuntimeError, match="record_denoise_path"):
        d.sample_chunked(cond, 1.0, 32, variants=good)
    with pytest.raises(RuntimeError, match="record_denoise_path"):
        d.sample_best(cond, cond, 2, variants=good)
    d.record_denoise_path = False
    # a well-formed list gets as far as the device check
    with pytest.raises(RuntimeError, match="not on a HIP device"):
        d.sample_chunked(cond, 1.0, 32, variants=good)
    with pytest.raises(RuntimeError, match="not on a HIP device"):
        d.sample_best(cond, cond, 4, variants=good[:2])
    with pytest.raises(RuntimeError, match="not on a HIP device"):
        d.sample_chunked(cond, 1.0, 32, variants=[(1.0, None), (2.0, steps.with_renorm(d, 0)), (3.0, None)])


# ------------------------------------------------------------------------------------------------ round -> variant
def test_round_to_variant_mapping(monkeypatch):
    """Round r runs variants[r % len(variants)], every chunk of the round with it, whatever the grouping: recorded from the calls
    sample_best makes (the device entry points replaced by recorders; nothing is launched)."""
    from diffsg_amd import steps
    from diffsg_amd import repeated
    from diffsg_amd.ddpm import DDPMCore
    T = 8
    d = make_ddpm(T)
    a, b = steps.strided(d, 5), steps.ddim(d, 5, 0.5)
    variants = [(2.0, a), (-1.0, b), (500.0, steps.with_renorm(a, 0))]
    B, n = 64, 7
    seen = []          # (first seed of the call, omega, plan) per chunk, in call order

    class FakeCond(torch.Tensor):
        is_cuda = True

    cond = torch.zeros(B, 3).as_subclass(FakeCond)

    def fake_sample(self, cond, omega=1.0, *, seed=None, plan=None, **kw):
        seen.append((seed, float(omega), plan))
        return torch.zeros(cond.shape[0], 3)

    def fake_chunked(self, cond, omega=1.0, chunk_rows=512, *, seeds=None, plan=None, variants=None, **kw):
        nch = -(-cond.shape[0] // chunk_rows)
        assert len(seeds) == nch
        per = [(float(omega), plan)] * nch if variants is None else [(float(o), p) for o, p in variants]
        assert len(per) == nch
        seen.extend((s, o, p) for s, (o, p) in zip(seeds, per))
        return torch.zeros(cond.shape[0], 3)

    for cls in (DDPMCore, type(d)):
        monkeypatch.setattr(cls, "sample", fake_sample)
        monkeypatch.setattr(cls, "sample_chunked", fake_chunked)
        monkeypatch.setattr(cls, "_best_of_problem", lambda self: ("msr", {}))
    monkeypatch.setattr(repeated, "best_of", lambda problem, Y, X, out=None, round0=0, **kw: (out or []) + [(round0, Y.shape[0])])
    for chunk_rows, max_rows in ((None, 65536), (None, 64), (None, 3 * 64), (32, 65536), (32, 64), (32, 5 * 64), (16, 65536), (48, 65536)):
        seen.clear()
        per_round = 1 if chunk_rows is None else -(-B // chunk_rows)
        seeds = list(range(1000, 1000 + n * per_round))
        groups = d.sample_best(cond, cond, n, seeds=seeds, chunk_rows=chunk_rows, max_rows=max_rows, variants=variants)
        assert sum(g for _, g in groups) == n and [r0 for r0, _ in groups] == [sum(g for _, g in groups[:k]) for k in range(len(groups))]
        assert [s for s, _, _ in seen] == seeds                       # round-major, chunk by chunk
        for k, (s, om, plan) in enumerate(seen):
            want_om, want_plan = variants[(k // per_round) % len(variants)]
            assert om == want_om and plan is want_plan, (chunk_rows, max_rows, k)


# ------------------------------------------------------------------------------------------------ budgets of the GPU parity cases
@pytest.mark.parametrize("name", [c.name for c in VR.CASES])
def test_parity_case_budgets(name):
    """Every chunk of every parity case of tests/test_gpu_variants.py: the reference's own float32-against-float64 error is below
    steps_ref.CAP = 1e-5 (the bound there is TOL + 3 x budget per chunk), and on `tiny`, whose weights are chosen by the rule below, at
    most CAP / 2.  Measured: 2.3e-7 .. 1.7e-6; the omega = 500 chunks of `tiny` 8.5e-7 and 8.6e-7.  (omega = 500 with renorm steps, and on
    the NU checkpoint: see variants_ref.CASES -- bit-for-bit cases only.)"""
    b = VR.chunk_budgets(name)
    print(name, ["%.2e" % v for v in b])
    case = VR.CASE[name]
    assert len(b) == len(case.variants) == -(-case.B // case.chunk_rows)
    assert max(b) < (R.CAP if case.net == "nu3" else R.CAP / 2), b


def test_tiny_weight_seed_follows_the_rule():
    """Synthetic weights: the first seed from 3 upwards at which every chunk of every tiny case has a budget of at most CAP / 2
    (DESIGN.md 7.1): seed 3, the seed tests/steps_ref.py uses for the net (worst chunk 1.7e-6)."""
    tiny = [c.name for c in VR.CASES if c.net == "tiny"]
    assert tiny and VR.TINY_SEED >= 3
    for seed in range(3, VR.TINY_SEED):
        worst = max(max(VR.chunk_budgets(nm, seed)) for nm in tiny)
        assert worst > R.CAP / 2, f"seed {seed} already meets the cap: the rule picks it"
    assert max(max(VR.chunk_budgets(nm)) for nm in tiny) <= R.CAP / 2


def test_cases_cover_what_they_claim():
    every = VR.CASES + VR.BIT_ONLY
    for c in every:
        assert len(set(c.variants)) == len(c.variants), c.name                      # all chunks distinct
        assert c.chunk_rows % 32 == 0 and len(c.variants) == -(-c.B // c.chunk_rows) > 1
        K = VR.steps_of(c)
        assert all(0 <= v.renorm <= K for v in c.variants)
    D = {"nu3": 5, "tiny": 3}
    assert any(c.B * D[c.net] % 4 for c in every) and any(c.B * D[c.net] % 4 == 0 for c in every)    # scalar and quad path
    assert any(c.B % c.chunk_rows for c in every) and any(c.chunk_rows == 64 for c in every)
    for group in (VR.CASES, VR.BIT_ONLY):
        vs = [(c, v) for c in group for v in c.variants]
        assert {v.omega for _, v in vs} == {2.0, -1.0, 500.0}
        assert {0, 1, 4} <= {v.renorm for _, v in vs} and any(v.renorm == VR.steps_of(c) for c, v in vs)
        assert {"identity", "strided", "ddim0", "ddim0.5"} <= {v.table for _, v in vs}


# ------------------------------------------------------------------------------------------------ the quality table
def test_recorded_quality_table_is_well_formed():
    with open(os.path.join(GOLD, "g18_variants.json")) as f:
        rec = json.load(f)
    assert (rec["rows"], rec["T"]) == (512, 20) and rec["renorm_cycle"] == list(VR.RENORM_CYCLE) and rec["omega_cycle"] == list(VR.OMEGA_CYCLE)
    r = rec["ratios"]
    for n in (4, 8, 16):
        assert r[f"T20_renorm_n{n}"] > r[f"T20_same_n{n}"]
    assert r["T20_renorm_n8"] > r["T20_same_n16"]                  # eight rounds with the count cycled beat sixteen that differ in seed only
    assert r["K10ddim0_renorm_n8"] > r["K10ddim0_same_n16"]
    assert r["T20_renorm_n8_seeds11"] > r["T20_same_n8_seeds11"]
    assert (rec["pinned"]["rows"], rec["pinned"]["seeds"]) == (VR.PIN_ROWS, list(VR.PIN_SEEDS))


def test_renorm_cycle_beats_seeds_only_at_best_of_8():
    """One cell of the table, recomputed with the oracle: the NU checkpoint's first 128 rows, T = 20, omega = 500, seeds 101 .. 108 --
    best-of-8 with the renorm count cycled 4, 0, 2, 1, 3 over the rounds against best-of-8 with 4 renorm steps in every round, the same
    seeds.  Measured (tests/golden/g18_variants.json, "pinned"): 1.179317 seeds only, 1.285353 cycled, margin 0.106; on all 512 rows
    1.152785 against 1.268860.  Both values must be within 1e-4 of the record and the margin at least a third of the recorded one."""
    with open(os.path.join(GOLD, "g18_variants.json")) as f:
        pin = json.load(f)["pinned"]
    same = VR.best_of_ratio("same", VR.PIN_SEEDS, 20, VR.PIN_ROWS)
    cyc = VR.best_of_ratio("renorm", VR.PIN_SEEDS, 20, VR.PIN_ROWS)
    print(f"best-of-8 on {VR.PIN_ROWS} rows: seeds only {same:.6f}, renorm cycled {cyc:.6f}, margin {cyc - same:.6f} "
          f"(recorded {pin['same']:.6f} / {pin['renorm']:.6f})")
    assert abs(same - pin["same"]) <= 1e-4 and abs(cyc - pin["renorm"]) <= 1e-4
    assert cyc - same >= (pin["renorm"] - pin["same"]) / 3 > 0.01, (same, cyc, pin)
