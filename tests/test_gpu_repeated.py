"""Repeated sampling on the device: dsg_best_of / diffsg_amd.best_of / DDPM.sample_best / load_test_*(repeats=n).

1. bit for bit against a torch composition of the EXISTING decode.* calls per round (strict-improvement torch.where loop);
2. against the CPU restatement tests/best_ref.py, with the tolerances of test_decoders_vs_oracle_random;
3. sample_best end to end against best_of over the stacked per-round sample() calls;
4. load_test_nu(repeats=4) on the committed NU checkpoint.
All tests need an MI355X: run with `-m gpu`."""
import os

import numpy as np
import pytest
import torch

from _util import GOLD, synth_params
from best_ref import best_of_ref
from oracle import ddpm_oracle as O
from weights import CONFIGS

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (63, 5), (333, 7), (4096, 16), (65536, 4)]
NU_PARAMS = {"width": 400, "height": 400, "p_sum": 18.0}


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    """torch.equal, on the bit patterns where a NaN is in play (NaN != NaN)."""
    return torch.equal(a, b) or (a.dtype == torch.float32 and torch.equal(bits(a), bits(b)))


def compose(problem, Y, X, out=None, round0=0, **p):
    """best-of-n from the existing whole-tensor entry points, one round at a time."""
    from diffsg_amd import decode as Dc
    maximise = problem != "co"
    sol, obj, rnd = (None, None, None) if out is None else (out[0].clone(), out[1].clone(), out[2].clone())
    objs = []
    for k in range(Y.shape[0]):
        if problem == "msr":
            s = p["W"] * Dc.msr_decode(Y[k])
            o = Dc.msr_rate(s, X)
        elif problem == "co":
            s = Dc.co_decode(Y[k])
            o = Dc.co_cost(X, s)
        else:
            s = Dc.nu_decode(Y[k], p["width"], p["height"], p["p_sum"])
            o = Dc.nu_rate(s, X)
        objs.append(o)
        fin = torch.isfinite(o)
        idx = torch.full_like(o, round0 + k, dtype=torch.int32)
        if sol is None:
            sol, obj, rnd = s.clone(), o.clone(), torch.where(fin, idx, torch.full_like(idx, -1))
            continue
        take = fin & ((rnd < 0) | ((o > obj) if maximise else (o < obj)))
        sol = torch.where(take[:, None], s, sol)
        obj = torch.where(take, o, obj)
        rnd = torch.where(take, idx, rnd)
    return sol, obj, rnd, torch.stack(objs)


def inputs(problem, B, n, D=None, seed=0, K=3):
    """Inputs as test_decoders_vs_oracle_random builds them (CPU tensors)."""
    g = torch.Generator().manual_seed(1000 * seed + B + n)
    if problem == "msr":
        return torch.randn(n, B, D, generator=g) * 3.0, torch.rand(B, D, generator=g) * 2.0 + 0.5, {"W": 20.0}
    if problem == "co":
        Y = torch.randn(n, B, 3, generator=g)
        Y[:, ::7] = -20.0                                 # dead rows in every round: exact ties
        return Y, torch.rand(B, 9, generator=g) * 10.0, {}
    return torch.randn(n, B, K + 2, generator=g), torch.rand(B, 2 * K, generator=g) * 400.0, dict(NU_PARAMS)


CASES = [("msr", 3), ("msr", 80), ("msr", 200), ("co", 3), ("nu", 3), ("nu", 7)]


@pytest.mark.parametrize("B,n", SHAPES)
@pytest.mark.parametrize("problem,D", CASES)
def test_best_of_is_the_composition_of_the_existing_calls_bit_for_bit(problem, D, B, n):
    from diffsg_amd import best_of
    Y, X, p = inputs(problem, B, n, D=D, K=D)
    Y, X = Y.cuda(), X.cuda()
    got = best_of(problem, Y, X, return_objectives=True, **p)
    ref = compose(problem, Y, X, **p)
    assert got.round.dtype == torch.int32 and got.solution.shape == Y.shape[1:] and got.objectives.shape == Y.shape[:2]
    for name, a, b in zip(("solution", "objective", "round", "objectives"), got, ref):
        assert torch.equal(a, b), name
    if problem == "co" and B >= 7:
        assert int(got.round[::7].max()) == 0             # dead rows tie in every round: the first wins
    if n > 1:                                             # two groups with round0 == the one-shot call
        cut = n // 2
        first = best_of(problem, Y[:cut], X, return_objectives=True, **p)
        two = best_of(problem, Y[cut:], X, out=first, round0=cut, return_objectives=True, **p)
        assert two.solution is first.solution
        for name, a, b in zip(("solution", "objective", "round", "objectives"), two, got):
            assert torch.equal(a, b), name
    assert best_of(problem, Y, X, **p).objectives is None


@pytest.mark.parametrize("problem,D", [("msr", 12), ("msr", 40), ("msr", 300), ("msr", 1024), ("co", 16), ("nu", 32)])
def test_best_of_every_lane_layout(problem, D):
    """The row widths that take the remaining lanes-per-row pairings of (k_row_softmax, k_msr_rate), and the widest rows."""
    from diffsg_amd import best_of
    g = torch.Generator().manual_seed(D)
    n, B = 3, 257
    if problem == "msr":
        Y, X, p = torch.randn(n, B, D, generator=g) * 3.0, torch.rand(B, D, generator=g) * 2.0 + 0.5, {"W": 20.0}
    elif problem == "co":
        Y, X, p = torch.randn(n, B, D, generator=g) * 2.0, torch.rand(B, 3 * D, generator=g) * 10.0, {}
    else:
        Y, X, p = torch.randn(n, B, D + 2, generator=g), torch.rand(B, 2 * D, generator=g) * 400.0, dict(NU_PARAMS)
    Y, X = Y.cuda(), X.cuda()
    got = best_of(problem, Y, X, return_objectives=True, **p)
    for name, a, b in zip(("solution", "objective", "round", "objectives"), got, compose(problem, Y, X, **p)):
        assert torch.equal(a, b), name


def test_best_of_nan_rounds_and_refusals():
    from diffsg_amd import best_of
    Y, X, p = inputs("msr", 333, 7, D=80)
    Y[2, 5] = float("nan")          # one round of one condition
    Y[:, 9] = float("nan")          # a condition without a finite round
    Y[0, 11] = float("nan")         # round 0 of a condition
    X[20] = -100.0                  # negative gains: 1 + p * g < 0, every objective NaN
    Y, X = Y.cuda(), X.cuda()
    got = best_of("msr", Y, X, return_objectives=True, **p)
    ref = compose("msr", Y, X, **p)
    for name, a, b in zip(("solution", "objective", "round", "objectives"), got, ref):
        assert same(a, b), name
    assert int(got.round[9]) == -1 and int(got.round[20]) == -1 and int(got.round[5]) != 2 and int(got.round[11]) > 0
    assert bool(torch.isnan(got.objective[9])) and same(got.solution[20], 20.0 * __import__("diffsg_amd").decode.msr_decode(Y[0])[20])
    first = best_of("msr", Y[:3], X, **p)
    two = best_of("msr", Y[3:], X, out=first, round0=3, **p)
    for a, b in zip(two[:3], got[:3]):
        assert same(a, b)
    # refusals
    z = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(RuntimeError, match="NU with D = 2"):
        best_of("nu", z(2, 4, 2), z(4, 0), **NU_PARAMS)
    with pytest.raises(RuntimeError, match="K = 33"):
        best_of("nu", z(2, 4, 35), z(4, 66), **NU_PARAMS)
    with pytest.raises(RuntimeError, match="at most"):
        best_of("msr", z(1, 2, 1025), z(2, 1025), W=1.0)
    with pytest.raises(RuntimeError, match="at most"):
        best_of("co", z(1, 2, 17), z(2, 51))
    empty = best_of("co", z(3, 0, 3), z(0, 9))
    assert empty.solution.shape == (0, 3) and empty.round.shape == (0,)


EPS = {"msr": lambda o, K: 5e-6 * o, "co": lambda o, K: 1e-5 * o, "nu": lambda o, K: 1e-5 * o + K * 1.8e-7}


@pytest.mark.parametrize("problem,B,n", [(pb, B, n) for pb in ("msr", "co", "nu") for B, n in [(4096, 16), (333, 7), (65536, 4)]]
                         + [("msr", 1000, 64), ("nu", 1000, 64)])
def test_best_of_vs_cpu_restatement(problem, B, n):
    """Every condition: the device objective is within eps of the restatement's at the device's round; that one is within
    2 eps of the restatement's best; where the restatement's top two are more than 2 eps apart the rounds agree (at least
    75 % of the conditions are that clear); the solution row is within 2e-6 relative of the restatement's row of that round.
    eps: test_decoders_vs_oracle_random's own tolerances (MSR 5e-6, CO 1e-5 relative to max|obj|; NU 1e-5 relative + K * 1.8e-7)."""
    from diffsg_amd import best_of
    K = 3
    Y, X, p = inputs(problem, B, n, D=80, seed=1, K=K)
    got = best_of(problem, Y.cuda(), X.cuda(), return_objectives=True, **p)
    sign = 1.0 if problem != "co" else -1.0
    sols = []
    objs = []
    for k in range(n):
        if problem == "msr":
            s = p["W"] * O.msr_decode(Y[k]); o = O.msr_rate(s, X)
        elif problem == "co":
            s = O.co_decode(Y[k]); o = O.co_cost(X, s)
        else:
            s = O.nu_decode(Y[k], 400, 400, 18.0); o = O.nu_rate(s, X)
        sols.append(s); objs.append(o)
    sols, objs = torch.stack(sols), torch.stack(objs)                     # [n, B, D], [n, B]
    ref = best_of_ref(problem, Y, X, **p)
    assert torch.equal(ref[3], objs.float())
    eps = EPS[problem](float(objs.abs().max()), K)
    rnd = got.round.cpu().long()
    assert int(rnd.min()) >= 0 and int(rnd.max()) < n
    rows = torch.arange(B)
    at = objs[rnd, rows]
    dev_err = float((got.objective.cpu() - at).abs().max())
    best = (sign * objs).max(0).values
    regret = float((best - sign * at).max())
    top2 = torch.topk(sign * objs, 2, dim=0).values if n > 1 else None
    clear = (top2[0] - top2[1]) > 2 * eps if n > 1 else torch.ones(B, dtype=torch.bool)
    share = float(clear.float().mean())
    sol_err = float((got.solution.cpu() - sols[rnd, rows]).abs().max() / sols.abs().max())
    print(f"{problem} B={B} n={n}: eps {eps:.3e}, |dev - ref| {dev_err:.3e}, regret {regret:.3e}, clear share {share:.3f}, "
          f"solution rel err {sol_err:.2e}, objectives max err {float((got.objectives.cpu() - objs).abs().max()):.3e}")
    assert dev_err <= eps
    assert regret <= 2 * eps
    assert torch.equal(rnd[clear], ref[2].long()[clear])
    assert share >= 0.75
    assert sol_err <= 2e-6


# ---------------------------------------------------------------- end to end
def make_problem_ddpm(name, seed, T):
    """A small model of the named config (the builders of test_gpu_parity.py) under its problem's DDPM class."""
    from diffsg_amd import UNet1D
    from diffsg_amd import classifier_free_CO as CO, classifier_free_MSR as MSR, classifier_free_NU as NU
    cfg = CONFIGS[name]
    _, params = synth_params(name, seed)
    m = UNet1D(**cfg, is_attn=(False,) * len(cfg["dims"]))
    m.load_state_dict(params, strict=True)
    D, dev, alphas = cfg["input_dim"], torch.device("cuda"), 1.0 - O.cosine_betas(T)
    if name.startswith("msr"):
        d = MSR.DDPM(T, m.to("cuda"), D, 20.0, alphas, dev, (1, D), None)
    elif name.startswith("co"):
        d = CO.DDPM(T, m.to("cuda"), D, alphas, dev, (1, D), None)
    else:
        d = NU.DDPM(T, m.to("cuda"), D - 2, 18.0, alphas, dev, (1, D), {"width": 400, "height": 400})
    return d.to("cuda")


def features(name, B, g):
    """(cond, X): the scaled condition the sampler sees and the unscaled features the objective reads."""
    if name.startswith("msr"):
        X = torch.rand(B, CONFIGS[name]["input_dim"], generator=g) * 2.0 + 0.5
        return ((X - X.min()) / (X.max() - X.min())).cuda(), X.cuda()
    if name.startswith("co"):
        X = torch.rand(B, 3 * CONFIGS[name]["input_dim"], generator=g) * 9.0 + 0.1
        return (X / 10.0).cuda(), X.cuda()
    X = torch.rand(B, 2 * (CONFIGS[name]["input_dim"] - 2), generator=g) * 400.0
    return (X / 400.0).cuda(), X.cuda()


@pytest.mark.parametrize("name", ["msr3", "msr80", "co3", "nu3"])
def test_sample_best_is_best_of_over_the_rounds_own_sample_calls(name):
    from diffsg_amd import best_of
    g = torch.Generator().manual_seed(17)
    d = make_problem_ddpm(name, 31, 6)
    problem, p = d._best_of_problem()
    seeds = [101, 202, 303, 404, 505]
    for B, kw in [(96, {}), (100, {}), (96, {"chunk_rows": 32}), (96, {"max_rows": 200}), (96, {"chunk_rows": 32, "max_rows": 100})]:
        cond, X = features(name, B, g)
        if "chunk_rows" in kw:
            sd = [1000 * k + c for k in range(5) for c in range(3)]       # round-major, one per chunk
            rounds = [torch.cat([d.sample(cond[32 * c:32 * c + 32], 1.0, seed=sd[3 * k + c]) for c in range(3)]) for k in range(5)]
        else:
            sd = seeds
            rounds = [d.sample(cond, 1.0, seed=s) for s in sd]
        ref = best_of(problem, torch.stack(rounds), X, return_objectives=True, **p)
        got = d.sample_best(cond, X, 5, 1.0, seeds=sd, return_objectives=True, **kw)
        for fname, a, b in zip(("solution", "objective", "round", "objectives"), got, ref):
            assert torch.equal(a, b), (B, kw, fname)
        if not kw:
            one = d.sample_best(cond, X, 1, 1.0, seeds=sd[:1])
            assert int(one.round.abs().max()) == 0
            dec = compose(problem, rounds[0][None], X, **p)
            assert torch.equal(one.solution, dec[0]) and torch.equal(one.objective, dec[1])
            assert bool(((got.objective >= one.objective) if problem != "co" else (got.objective <= one.objective)).all())
    # seeds drawn from torch's global generator, round-major, in call order
    cond, X = features(name, 96, g)
    torch.manual_seed(5)
    drawn = [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in range(3)]
    torch.manual_seed(5)
    a = d.sample_best(cond, X, 3, 1.0)
    b = d.sample_best(cond, X, 3, 1.0, seeds=drawn)
    assert torch.equal(a.solution, b.solution) and torch.equal(a.round, b.round)
    with pytest.raises(ValueError, match="seeds"):
        d.sample_best(cond, X, 3, 1.0, seeds=[1, 2])


def test_load_test_nu_with_repeats_on_the_committed_checkpoint(tmp_path, monkeypatch):
    from diffsg_amd import classifier_free_NU as NU
    from diffsg_amd.ddpm import DDPMCore
    g = np.load(os.path.join(GOLD, "g4_sample_nu_ckpt.npz"))
    T, P = int(g["T"]), float(g["P_sum"])
    csv = os.path.join(GOLD, "data", "3u_18mW_200samples.csv")
    m = NU.build_model(3, P, torch.device("cuda"), T, {"width": 400, "height": 400})
    m.model.load_state_dict({k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w.")}, strict=True)
    ck = str(tmp_path / "ddpm_nu.pt")
    torch.save(m.state_dict(), ck)
    used = []
    plain = DDPMCore._sample_once

    def spy(self, cond, omega, y_T, noise, seed, *rest):
        if seed not in used:                              # (the float32 repeat of a saturated call passes the same seed again)
            used.append(seed)
        return plain(self, cond, omega, y_T, noise, seed, *rest)
    monkeypatch.setattr(DDPMCore, "_sample_once", spy)
    logs = []
    torch.manual_seed(7)
    one = NU.load_test_nu(ck, csv, T=T, omega=500, log=logs.append)
    seed1, used[:] = list(used), []
    torch.manual_seed(7)
    parent = NU.load_test_nu(ck, csv, T=T, omega=500, log=logs.append, repeats=1)
    assert parent == one and used == seed1 and sorted(one) == ["avg_rate_diff", "less_ratio"] and len(logs) == 4
    used[:] = []
    torch.manual_seed(7)
    four = NU.load_test_nu(ck, csv, T=T, omega=500, log=logs.append, repeats=4)
    assert sorted(four) == ["avg_rate_diff", "less_ratio", "repeats"] and four["repeats"] == 4
    # four seeds, the first of them the one the single draw uses (both come first out of torch's generator after the model is built)
    assert len(seed1) == 1 and seed1[0] is not None and len(used) == 4 and len(set(used)) == 4 and used[0] == seed1[0]
    print(f"less_ratio: repeats=1 {one['less_ratio']:.5f}, repeats=4 {four['less_ratio']:.5f}")
    assert four["less_ratio"] >= one["less_ratio"]
