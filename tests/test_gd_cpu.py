"""Gradient-descent baseline, host side (no GPU): the float64 restatement against the reference's states, the argument checks of
diffsg_amd.gd, the kernels' resources, and the conditioning facts the GPU tests (tests/test_gpu_gd.py) rest their bounds on."""
import os

import numpy as np
import pytest
import torch

from _util import GOLD
import gd_ref as GR

PROBLEMS = {"co": "co", "msr3": "msr", "msr80": "msr", "nu": "nu"}


@pytest.fixture(scope="module")
def g16():
    return np.load(os.path.join(GOLD, "g16_gd.npz"))


@pytest.fixture(scope="module")
def twins(g16):
    """{(problem, iterations): per-row twin deviation}: computed once for the tests below."""
    return {(name, it): GR.twin_dev(kind, g16[f"{name}.x"], g16[f"{name}.y0"], it) for name, kind in PROBLEMS.items() for it in (20, 100)}


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_restatement_reproduces_every_golden_state(g16, name):
    _, kept = GR.run(PROBLEMS[name], g16[f"{name}.x"], g16[f"{name}.y0"], max(GR.STATES), GR.STATES)
    for k in GR.STATES:
        assert np.array_equal(kept[k], g16[f"{name}.y{k}"], equal_nan=True), k


def test_start_states_are_the_goldens(g16):
    assert np.array_equal(GR.co_init(200, 3), g16["co.y0"])
    assert np.array_equal(GR.msr_init(200, 3, float(g16["msr3.W"])), g16["msr3.y0"])
    assert np.array_equal(GR.msr_init(64, 80, float(g16["msr80.W"])), g16["msr80.y0"])
    assert np.array_equal(GR.nu_init(200, 3, float(g16["nu.P_sum"]), 400, 400), g16["nu.y0"])


def test_one_co_step_in_extended_precision_stays_inside_the_step_bound(g16):
    """(a) From every golden state the float64 step is within 1e-14 * (|Y_k| + |Y_k+1|) of the same step evaluated in np.longdouble:
    the bound of the GPU's step-by-step test is many float64 roundings wide (measured: 3.8e-16 on that scale)."""
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps, "np.longdouble is no wider than float64 on this platform"
    x = g16["co.x"]
    worst = 0.0
    for k in GR.TEACHER:
        yk = g16[f"co.y{k}"]
        y64 = GR.co_step(x, yk)
        with np.errstate(all="ignore"):
            yld = GR.co_step(x.astype(np.longdouble), yk.astype(np.longdouble))
        ok, ratio = GR.step_ok(y64, yk, yld.astype(np.float64))
        worst = max(worst, ratio * 1e-14)
        assert ok, (k, ratio)
    print(f"worst float64 vs longdouble CO step: {worst:.2e} of |Y_k| + |Y_k+1|")


def test_co_twin_runs_bound_the_conditioning(twins):
    """(b) One ulp on the start state: at most 1e-9 on every row after 20 iterations, on at least 80 % of the rows after 100."""
    t20, t100 = twins["co", 20], twins["co", 100]
    print(f"CO twin deviation: max at 20 = {t20.max():.2e}; share <= 1e-9 at 100 = {np.mean(t100 <= 1e-9):.3f}, max = {t100.max():.2e}")
    assert t20.max() <= 1e-9
    assert np.mean(t100 <= 1e-9) >= 0.8


@pytest.mark.parametrize("name", ["msr3", "msr80", "nu"])
def test_msr_and_nu_are_contractive(twins, name):
    """(c) The same perturbation stays below 1e-12 after 100 iterations (measured: MSR 2.0e-16 / 8.5e-17, NU 2.2e-13)."""
    t = twins[name, 100]
    print(f"{name} twin deviation at 100: {t.max():.2e}")
    assert t.max() <= 1e-12


def test_msr_sum_order_is_immaterial(g16):
    """The device adds an 80-entry row in its own order: left to right against numpy's pairwise sum over 100 iterations."""
    x, y0 = g16["msr80.x"], g16["msr80.y0"]
    a, _ = GR.run("msr", x, y0, 100)
    b, _ = GR.run("msr", x, y0, 100, sum_fn=GR.rowsum)
    assert GR.rel_dev(b, a).max() <= 1e-12


def test_driver_goldens_are_consistent(g16):
    """The stored figures are the stored per-row objectives', and few CO rows sit at cost_calc's decision threshold."""
    for p in ("co", "msr3", "nu"):
        for it in (20, 100):
            pred, true = g16[f"drv.{p}.{it}.pred"].astype(np.float64), g16[f"drv.{p}.{it}.true"].astype(np.float64)
            assert abs(pred.sum() / true.sum() - float(g16[f"drv.{p}.{it}.sum_ratio"])) <= 1e-5 * abs(float(g16[f"drv.{p}.{it}.sum_ratio"]))
    assert np.mean(~GR.co_far_from_threshold(g16["drv.co.20.norm"])) <= 0.02
    Y, rate = GR.msr_finish(g16["drv.msr3.20.Y"], g16["msr3.x"][-60:], float(g16["msr3.W"]))
    assert np.array_equal(rate, g16["drv.msr3.20.pred"])


def test_host_refusals_need_no_device():
    from diffsg_amd import gd
    x64 = torch.zeros(4, 9, dtype=torch.float64)
    for fn, args in ((gd.co_descent, (x64,)), (gd.msr_descent, (x64, 10.0)), (gd.nu_descent, (x64[:, :6], 18.0, 400, 400))):
        with pytest.raises(RuntimeError, match=rf"diffsg_amd\.gd\.{fn.__name__}: tensors are not on a HIP device"):
            fn(*args)
        with pytest.raises(TypeError, match=rf"diffsg_amd\.gd\.{fn.__name__}: tensors must be float64"):
            fn(args[0].float(), *args[1:])
        with pytest.raises(TypeError, match=rf"diffsg_amd\.gd\.{fn.__name__}: expected a torch tensor"):
            fn(args[0].numpy(), *args[1:])


def test_package_exports_and_signatures():
    import ctypes
    import inspect
    import diffsg_amd
    from diffsg_amd import _lib, gd
    for name in ("co_descent", "msr_descent", "nu_descent", "gd_co", "gd_msr", "gd_nu"):
        assert getattr(diffsg_amd, name) is getattr(gd, name) and name in diffsg_amd.__all__
    d = lambda f: {k: v.default for k, v in inspect.signature(f).parameters.items() if v.default is not inspect.Parameter.empty}
    assert d(gd.co_descent) == {"y0": None, "iters": 100, "lr": 0.1, "lambda1": 1.0, "lambda2": 1.0, "record_every": 0}
    assert d(gd.msr_descent) == {"y0": None, "iters": 100, "lr": 0.001, "record_every": 0}
    assert d(gd.nu_descent) == {"y0": None, "iters": 100, "lr": 0.1, "p_ref": 18.0, "record_every": 0}
    assert d(gd.gd_co) == {"used_sample_num": 10000, "iterations": 100, "log": print}
    assert d(gd.gd_msr) == {"used_sample_num": 1000, "iterations": 100, "log": print}
    assert d(gd.gd_nu) == {"width": 400, "height": 400, "used_sample_num": 3000, "iterations": 100, "log": print}
    for name, n_args in (("dsg_gd_co", 11), ("dsg_gd_msr", 9), ("dsg_gd_nu", 10)):
        res, args = _lib._SIGS[name]
        assert res is ctypes.c_int and len(args) == n_args and args[2] is ctypes.c_longlong
    with open(os.path.join(os.path.dirname(GOLD), "..", "include", "diffsg.h")) as f:
        header = f.read()
    assert all(f"int {name}(" in header for name in ("dsg_gd_co", "dsg_gd_msr", "dsg_gd_nu"))


def test_kernels_use_no_scratch_and_no_lds():
    import __graft_entry__ as g
    from diffsg_amd import _lib
    g.build()
    res = {k: v for k, v in _lib.kernel_resources().items() if "k_gd_" in k}
    for kernel in ("k_gd_co", "k_gd_msr", "k_gd_nu"):
        assert any(kernel + "<" in k for k in res), (kernel, sorted(res))
    for k, v in res.items():
        assert v["scratch"] == 0 and v["lds"] == 0, (k, v)
