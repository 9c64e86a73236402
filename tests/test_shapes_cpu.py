"""The shape catalogue of tests/shape_ref.py on the CPU: conditions that keep the bounds of tests/test_gpu_shapes.py meaningful.

The GPU tests bound sampling by `TOL + 3 x budget` and every gradient tensor by `GTOL + 4 x budget`, where the budgets are what the
float32 oracle itself is away from the float64 oracle on the same inputs.  A net on which float32 is badly conditioned would make those
bounds so wide that a wrong kernel passes; so each catalogue entry (descriptor AND weight seed) has to keep the sampling budget at most
1e-5 and the worst per-tensor gradient budget at most 2e-5, on exactly the inputs the GPU tests use.  No GPU, none of the library.
"""
import pytest
import torch

import shape_ref as S
from oracle import ddpm_oracle as O
from test_gpu_parity import grad_errs, rel


@pytest.mark.parametrize("name", S.NAMES)
def test_oracle_budgets_of_the_catalogue(name):
    ref, budget = S.sample_ref(name, 2.0)
    _, g32, g64 = S.train_ref(name)
    gb = grad_errs(g32, g64)
    worst = max(gb, key=gb.get)
    print(f"{name}: sampling budget {budget:.2e} (omega -1: {S.sample_ref(name, -1.0)[1]:.2e}), gradient budget {gb[worst]:.2e} at {worst}")
    assert torch.isfinite(ref).all()
    assert budget <= S.SAMPLE_CAP
    assert gb[worst] <= S.GRAD_CAP, worst


def test_the_catalogue_is_what_the_issue_lists():
    """13 descriptors, none with input_dim 1 (the reference's torch.squeeze in the loss collapses it; the oracle's loss raises there),
    every one inside what dsg_create accepts, and each with the property it exists for."""
    assert len(S.NAMES) == 13
    for name, e in S.SHAPES.items():
        c = e["cfg"]
        assert 2 <= c["input_dim"] <= 128 and 1 <= c["cond_dim"] <= 4096 and c["n_blocks"] >= 1 and 1 <= len(c["dims"]) <= 8, name
        assert c["proj_dim"] in (8, 16, 32, 64, 128) and all(d in (4, 8, 16, 32, 64, 128) for d in c["dims"]), name
    narrow = {n: [f for _, f in S.narrow_flags(n)] for n in S.NAMES}
    assert not any(narrow["allwide"]) and S.longest_narrow_run("allwide") == (0, 0)
    for n in ("hill", "jump"):          # narrow operators on both sides of wide ones: some lie outside the one fused run
        lo, hi = S.longest_narrow_run(n)
        assert hi - lo >= 2 and sum(narrow[n]) > hi - lo, n
    for n in ("flat32", "flat32x4"):    # everything between feature_proj and final is one narrow run
        assert S.longest_narrow_run(n) == (1, len(narrow[n]) - 1), n
    assert len(O.state_shapes(S.net("deep8")[0])) == 848


def test_inputs_are_the_documented_shapes():
    for name in ("one8", "io127"):
        c = S.SHAPES[name]["cfg"]
        cond, y_T, z = S.sample_inputs(name)
        assert cond.shape == (S.B, c["cond_dim"]) and y_T.shape == (S.B, c["input_dim"]) and z.shape == (S.T - 2, S.B, c["input_dim"])
        y, cond, ts, noise, mask = S.train_inputs(name)
        assert ts.shape == (1, S.B) and int(ts.max()) < S.T and 0.0 < float(mask.mean()) < 1.0
        x, t, cond, mask = S.forward_inputs(name, S.B)
        assert 0.0 < float(mask.mean()) < 1.0 and t.shape == (1, S.B)
    assert S.B == 70 and S.T == 5 and rel(S.forward_ref("one8", 1), S.forward_ref("one8", 1)) == 0.0
