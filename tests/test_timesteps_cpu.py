"""Timestep laws on the host: the CDF rule on known cases, every refusal of the constructors, the constructors'
definitions, the C ABI's declarations, the pinned signatures, and the float32-against-float64 budgets of the weighted reference that
tests/test_gpu_timesteps.py uses in its bounds.  No device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from _util import ROOT
import timesteps_ref as R
from diffsg_amd import _lib, timesteps as TS

G = 1 << 24


# ------------------------------------------------------------------------------------------------ the CDF rule
def test_cdf24_on_known_cases():
    lw = TS.law(4, p=[1, 1, 1, 1])
    assert lw.cdf24.tolist() == [G // 4, G // 2, 3 * G // 4, G] and all(v % (1 << 22) == 0 for v in lw.cdf24.tolist())
    lw = TS.law(5, p=[0, 1, 0, 1, 0])
    assert lw.cdf24.tolist() == [0, G // 2, G // 2, G, G] and lw.support == (1, 3)          # zeros give repeated entries
    p = [1, 1, 1]                                                                            # thirds need rounding
    lw = TS.law(3, p=p)
    assert lw.cdf24.tolist() == [5592405, 11184811, G] and lw.cdf24[-1] == G
    rng = np.random.default_rng(0)
    for T in (2, 7, 1000):
        p = rng.random(T)
        assert np.array_equal(TS.law(T, p=p).cdf24, R.cdf24(p))
        assert TS.law(T, p=p * 1e-30).cdf24[-1] == G                                         # a sum far from 1: the last entry is forced
    assert TS.law(6).cdf24 is None and TS.law(6).w is None and TS.law(6).T == 6              # the reference's rule: nothing to set


def test_expected_ts_is_the_upper_bound():
    cdf = TS.law(5, p=[0, 1, 0, 1, 0]).cdf24
    u = np.array([0, 1, G // 2 - 1, G // 2, G - 1])
    assert TS.expected_ts(cdf, u).tolist() == R.expected_ts(cdf, u).tolist() == [1, 1, 1, 3, 3]
    assert R.expected_ts(TS.law(4, p=[1, 1, 1, 1]).cdf24, [0, G // 4 - 1, G // 4, G - 1]).tolist() == [0, 0, 1, 3]


def test_a_law_is_immutable():
    lw = TS.law(4, p=[1, 2, 3, 4], w=[1, 1, 0, 2])
    with pytest.raises(Exception):
        lw.w = None
    for a in (lw.p, lw.w, lw.cdf24):
        with pytest.raises(ValueError):
            a[0] = 1
    assert lw.p.dtype == np.float64 and lw.w.dtype == np.float32 and lw.cdf24.dtype == np.int64


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_of_the_constructors():
    with pytest.raises(ValueError, match="3 probabilities for T = 4"):
        TS.law(4, p=[1, 1, 1])
    with pytest.raises(ValueError, match="probabilities must be >= 0"):
        TS.law(3, p=[1, -1, 1])
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="probabilities must be finite"):
            TS.law(3, p=[1, bad, 1])
    with pytest.raises(ValueError, match="sum to 0"):
        TS.law(3, p=[0, 0, 0])
    with pytest.raises(ValueError, match=r"timestep 1 has p = .* 2\^-24"):
        TS.law(3, p=[1, 1e-9, 1])
    with pytest.raises(ValueError, match="2 weights for T = 3"):
        TS.law(3, w=[1, 1])
    with pytest.raises(ValueError, match="weights must be >= 0"):
        TS.law(3, w=[1, -0.5, 1])
    for bad in (float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="weights must be finite"):
            TS.law(3, w=[1, bad, 1])
    with pytest.raises(ValueError, match="weights must be >= 0"):
        TS.with_weights(TS.law(3, p=[1, 1, 1]), [1, -1, 1])
    with pytest.raises(ValueError, match="taus must be distinct integers"):
        TS.on_plan(8, (1, 9))


# ------------------------------------------------------------------------------------------------ constructors
class _Sched:
    def __init__(self, T):
        from oracle import ddpm_oracle as O
        self.T = T
        self.alphas_cumprod = O.schedule_buffers(1.0 - O.cosine_betas(T))["alphas_cumprod"]

    def _coef_table(self):
        return torch.zeros(self.T, 4)


def test_on_plan_support_is_the_plans_taus():
    from diffsg_amd import steps
    d = _Sched(20)
    for K in (5, 7):
        plan = steps.strided(d, K)
        lw = TS.on_plan(d, plan)
        assert lw.support == tuple(plan.taus) and lw.w is None
        widths = np.diff(np.concatenate(([0], lw.cdf24)))
        assert set(np.nonzero(widths)[0].tolist()) == set(plan.taus) and widths[list(plan.taus)].max() - widths[list(plan.taus)].min() <= 1
    assert TS.on_plan(d, (3, 11)).support == (3, 11)
    assert TS.on_plan(8, (0, 7), w=np.ones(8)).w.tolist() == [1.0] * 8


@pytest.mark.parametrize("T", [8, 20, 1000])
def test_min_snr_is_the_float64_formula_within_one_ulp(T):
    d = _Sched(T)
    for gamma in (5.0, 1.0):
        lw = TS.min_snr(d, gamma)
        acp = d.alphas_cumprod.double().numpy()
        snr = acp / (1.0 - acp)
        want = np.minimum(snr, gamma) / snr
        got = lw.w.astype(np.float64)
        assert lw.cdf24 is None and lw.w.dtype == np.float32
        assert np.all(np.abs(got - want) <= np.spacing(want.astype(np.float32)).astype(np.float64)), np.abs(got - want).max()
        assert got.max() <= 1.0 and got.min() > 0.0
    assert TS.min_snr(d, 5.0, p=np.ones(T)).cdf24[-1] == G
    base = TS.on_plan(d, (1, 3))
    both = TS.with_weights(base, TS.min_snr(d).w)
    assert both.cdf24 is base.cdf24 and np.array_equal(both.w, TS.min_snr(d).w) and TS.with_weights(both, None).w is None


# ------------------------------------------------------------------------------------------------ C ABI
def _header():
    with open(os.path.join(ROOT, "include", "diffsg.h")) as f:
        return re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)


def test_header_sigs_and_binding_agree_and_neither_takes_a_stream():
    hdr = _header()
    want = {"dsg_set_train_law": ["dsg_handle* h", "const unsigned* cdf24_host", "const float* weight_host", "int T"],
            "dsg_set_train_report": ["dsg_handle* h", "double* sq_dev", "long long* rows_dev", "int T"]}
    import test_streams_cpu as S
    for name, params in want.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^()]*)\)\s*;", hdr)
        assert m, f"include/diffsg.h does not declare {name}"
        assert [a.strip() for a in m.group(1).split(",")] == params
        res, args = _lib._SIGS[name]
        assert res is ctypes.c_int and len(args) == 4 and args[0] is ctypes.c_void_p and args[3] is ctypes.c_int
        assert name not in S.stream_functions()
        assert hasattr(_lib.lib(), name)
    assert _lib._SIGS["dsg_set_train_law"][1][1:3] == [ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_float)]
    # the design chosen for captured steps is written where the issue asks for it
    with open(os.path.join(ROOT, "include", "diffsg.h")) as f:
        raw = f.read()
    comment = raw[:raw.index("unsigned long long dsg_generation")].rsplit("/*", 1)[1]
    assert "dsg_set_train_law" in comment and "dsg_set_train_report" in comment and "re-captures" in comment


def test_the_context_leaves_the_pinned_signatures_alone(monkeypatch):
    from diffsg_amd import entry, train
    before = (inspect.signature(entry.train), inspect.signature(entry.train_ddpm), inspect.signature(train.run_epochs))
    seen = []

    class M:
        T = 4

        def loss_report(self, on=True):
            seen.append(("report", on))
    lw = TS.law(4, p=[1, 1, 0, 0])
    m = M()
    TS.apply_active(m)
    assert seen == [] and "train_law" not in vars(m)                     # outside the context nothing is read
    with TS.training(law=lambda d: TS.on_plan(d, (1, 2)), report=True):
        TS.apply_active(m)
        assert m.train_law.support == (1, 2) and seen == [("report", True)]
        with TS.training(law=lw):
            m2 = M()
            TS.apply_active(m2)
            assert m2.train_law is lw and len(seen) == 1
        assert (inspect.signature(entry.train), inspect.signature(entry.train_ddpm), inspect.signature(train.run_epochs)) == before
    m3 = M()
    TS.apply_active(m3)
    assert "train_law" not in vars(m3)
    p = inspect.signature(entry.train).parameters
    assert list(p)[-2:] == ["graph", "seed"] and "law" not in p and "report" not in p
    assert list(inspect.signature(train.run_epochs).parameters)[-2:] == ["graph", "batches"]
    assert "timesteps.apply_active(diffusion_model)" in inspect.getsource(entry.train)


def test_no_split_while_a_law_or_a_report_is_held():
    from diffsg_amd.ddpm import DDPMCore
    d = DDPMCore.__new__(DDPMCore)
    torch.nn.Module.__init__(d)
    d.train_split_min_rows = 64
    assert d._splits(128) and not d._splits(32)
    d.train_law = TS.law(4, w=[1, 1, 1, 1])
    assert not d._splits(128)
    d.train_law = TS.law(4)                       # a law without arrays is the reference's rule
    assert d._splits(128)
    d._report = ()
    assert not d._splits(128)


# ------------------------------------------------------------------------------------------------ budgets of the GPU bounds
@pytest.mark.parametrize("name", list(R.NETS))
def test_budgets_of_the_weighted_reference(name):
    lb, gb = R.budgets(name)
    print(f"{name} (weight seed {R.NETS[name]['seed']}): weighted loss f32 vs f64 {lb:.2e} (cap {R.LOSS_CAP:g}), "
          f"worst per-tensor gradient budget {gb:.2e} (cap {R.GRAD_CAP:g})")
    assert lb <= R.LOSS_CAP and gb <= R.GRAD_CAP
    w = R.weights(name)
    ts = R.train_inputs(name)[2].reshape(-1)
    assert float(w.min()) == 0.0 and float(w.max()) <= 3.0 and int((w[ts] == 0).sum()) > 0 and int((w[ts] > 0).sum()) > 0


def test_the_per_timestep_sums_add_up_to_the_unweighted_loss():
    name = "tiny"
    plan, p = R.net(name)
    y, cond, ts, noise, mask = R.train_inputs(name)
    T = R.NETS[name]["T"]
    with torch.no_grad():
        eps = R.O.unet_forward(p, plan, R.O.q_sample(R.bufs(name), y, ts, noise), ts / T, cond, mask)
        loss = R.O.ddpm_loss(p, plan, R.bufs(name), T, y, cond, ts, noise, mask)
    sq, rows = R.per_timestep_sums(eps, noise, ts, T)
    assert int(rows.sum()) == R.B and torch.equal(rows, torch.bincount(ts.reshape(-1), minlength=T))
    assert abs(float(sq.sum()) / (R.B * y.shape[1]) - float(loss)) <= 1e-6 * float(loss)
