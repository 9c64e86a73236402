"""Gradient-descent baseline on the device (csrc/dsg_gd.hpp through diffsg_amd.gd and the C ABI) against the reference's float64 states
(tests/golden/g16_gd.npz) and the numpy restatement (tests/gd_ref.py).

The CO iteration is chaotic, so nothing here compares a long CO run row for row: single steps are checked from the reference's own
states, long runs where the reference itself is well conditioned (tests/test_gd_cpu.py asserts that the inputs meet those caps)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from _util import GOLD
import gd_ref as GR

pytestmark = pytest.mark.gpu

PROBLEMS = {"co": "co", "msr3": "msr", "msr80": "msr", "nu": "nu"}
STEP_FACTOR = {"co": 1e-14, "msr3": 1e-14, "msr80": 1e-13, "nu": 1e-14}     # msr80: the row sum's order differs (M * ulp of a sum near 20)
DATA = os.path.join(GOLD, "data")
CO_CSV, MSR_CSV, NU_CSV = (os.path.join(DATA, f) for f in ("3nodes_200samples_ood.csv", "3c_10w_200samples.csv", "3u_18mW_200samples.csv"))


@pytest.fixture(scope="module")
def g16():
    return np.load(os.path.join(GOLD, "g16_gd.npz"))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def descend(kind, x, y0, iters, record_every=0):
    """Device run of `iters` steps from y0 (numpy in, numpy out) with the reference's constants."""
    from diffsg_amd import gd
    x, y0 = dev(x), dev(y0)
    if kind == "co":
        r = gd.co_descent(x, y0, iters=iters, record_every=record_every)
    elif kind == "msr":
        r = gd.msr_descent(x, 10.0, y0, iters=iters, record_every=record_every)     # W only shapes the default start state
    else:
        r = gd.nu_descent(x, 18.0, 400, 400, y0, iters=iters, record_every=record_every)
    return tuple(t.cpu().numpy() for t in r) if record_every else r.cpu().numpy()


def device_t(kind, x, y0, iters, record_every=0):
    from diffsg_amd import gd
    if kind == "co":
        return gd.co_descent(x, y0, iters=iters, record_every=record_every)
    if kind == "msr":
        return gd.msr_descent(x, 10.0, y0, iters=iters, record_every=record_every)
    return gd.nu_descent(x, 18.0, 400, 400, y0, iters=iters, record_every=record_every)


# ---------------------------------------------------------------------------------------------------------------------
# 1. step by step, from the reference's own states
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_single_steps_from_the_reference_states(g16, name):
    x = g16[f"{name}.x"]
    worst = 0.0
    for k in GR.TEACHER:
        yk, yk1 = g16[f"{name}.y{k}"], g16[f"{name}.y{k + 1}"]
        got = descend(PROBLEMS[name], x, yk, 1)
        ok, ratio = GR.step_ok(got, yk, yk1, STEP_FACTOR[name])
        worst = max(worst, ratio)
        print(f"{name}: step {k} -> {k + 1}: worst error {ratio:.3g} of the bound, bit-identical: {np.array_equal(got, yk1, equal_nan=True)}")
        assert ok, (name, k, ratio)


# ---------------------------------------------------------------------------------------------------------------------
# 2. composition
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_calls_compose_bit_for_bit(g16, name):
    kind = PROBLEMS[name]
    x, y0 = dev(g16[f"{name}.x"]), dev(g16[f"{name}.y0"])
    whole = device_t(kind, x, y0, 20)
    assert torch.isfinite(whole).all()
    parts = device_t(kind, x, device_t(kind, x, y0, 7), 13)
    assert torch.equal(parts, whole)
    final, rec = device_t(kind, x, y0, 20, record_every=5)
    assert rec.shape == (4,) + tuple(y0.shape) and torch.equal(final, whole) and torch.equal(rec[-1], whole)
    assert torch.equal(rec[0], device_t(kind, x, y0, 5)) and torch.equal(rec[2], device_t(kind, x, y0, 15))
    _, rec7 = device_t(kind, x, y0, 20, record_every=7)       # 20 is no multiple of 7: two entries, the final state is not one of them
    assert rec7.shape[0] == 2 and torch.equal(rec7[1], device_t(kind, x, y0, 14))
    same = device_t(kind, x, y0, 0)
    assert torch.equal(same, y0) and same.data_ptr() != y0.data_ptr()
    assert torch.equal(y0, dev(g16[f"{name}.y0"]))           # the caller's start state is never written


# ---------------------------------------------------------------------------------------------------------------------
# 3. full runs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["msr3", "msr80", "nu"])
def test_contractive_problems_after_100_iterations(g16, name):
    got = descend(PROBLEMS[name], g16[f"{name}.x"], g16[f"{name}.y0"], 100)
    err = GR.rel_dev(got, g16[f"{name}.y100"])
    print(f"{name}: 100 iterations, worst deviation {err.max():.3g}")
    assert err.max() <= 1e-11


def test_co_after_20_iterations_all_rows(g16):
    got = descend("co", g16["co.x"], g16["co.y0"], 20)
    err = GR.rel_dev(got, g16["co.y20"])
    print(f"co: 20 iterations, worst deviation {err.max():.3g}, bit-identical rows {np.mean((got == g16['co.y20']).all(axis=1)):.3f}")
    assert err.max() <= 1e-8


def test_co_after_100_iterations_on_well_conditioned_rows(g16):
    x, y0 = g16["co.x"], g16["co.y0"]
    well = GR.twin_dev("co", x, y0, 100) <= 1e-9
    assert well.mean() >= 0.8
    got = descend("co", x, y0, 100)
    err = GR.rel_dev(got, g16["co.y100"])
    print(f"co: 100 iterations, {well.mean():.3f} of the rows well conditioned, worst deviation on them {err[well].max():.3g}; "
          f"bit-identical rows overall {np.mean((got == g16['co.y100']).all(axis=1)):.3f}")
    assert err[well].max() <= 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# 4. shapes that break layouts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,size", [("co", 1), ("co", 3), ("co", 16), ("msr", 1), ("msr", 3), ("msr", 7), ("msr", 80), ("msr", 128),
                                       ("nu", 1), ("nu", 3), ("nu", 32)])
def test_ragged_batches_and_every_kernel_variant(kind, size):
    """Three iterations from the start state against the restatement, on the last step's bound (the wide MSR variant adds a row in its
    own order: 1e-13 there, as for the 80-channel goldens)."""
    factor = 1e-13 if kind == "msr" and size > 8 else 1e-14
    for B in (1, 63, 65, 200):
        x, y0 = GR.synth(kind, B, size)
        _, kept = GR.run(kind, x, y0, 3, (2, 3))
        got = descend(kind, x, y0, 3)
        ok, ratio = GR.step_ok(got, kept[2], kept[3], factor)
        assert got.shape == y0.shape and ok, (kind, size, B, ratio)


def test_mid_sizes_take_the_next_wider_variant():
    """n = 5 and 9, K = 5, 9 and 17, M = 8 and 9: the first size of each wider kernel variant and the last of the narrow MSR one."""
    for kind, size in (("co", 5), ("co", 9), ("nu", 5), ("nu", 9), ("nu", 17), ("msr", 8), ("msr", 9)):
        x, y0 = GR.synth(kind, 65, size)
        _, kept = GR.run(kind, x, y0, 3, (2, 3))
        ok, ratio = GR.step_ok(descend(kind, x, y0, 3), kept[2], kept[3], 1e-13 if kind == "msr" and size > 8 else 1e-14)
        assert ok, (kind, size, ratio)


def test_zero_denominators_propagate_as_in_numpy():
    """No clamps: a zero allocation (CO) and a power sum exactly at p_ref (NU) give the inf / NaN numpy gives, in the same places,
    and the other rows are untouched by it."""
    x, y0 = GR.synth("co", 65, 3)
    y0[7, 4] = 0.0
    y0[64, 3] = 0.0
    for iters in (1, 3):
        want, kept = GR.run("co", x, y0, iters, (iters - 1,))
        got = descend("co", x, y0, iters)
        assert not np.isfinite(want[7]).all() and not np.isfinite(want[64]).all()
        ok, ratio = GR.step_ok(got, kept.get(iters - 1, y0), want)
        assert ok, (iters, ratio)
    x, y0 = GR.synth("nu", 65, 3)
    y0[5, 2:] = 6.0
    want, kept = GR.run("nu", x, y0, 2, (1,))
    got = descend("nu", x, y0, 2)
    assert not np.isfinite(want[5]).all()
    ok, ratio = GR.step_ok(got, kept[1], want)
    assert ok, ratio


# ---------------------------------------------------------------------------------------------------------------------
# 5. refusals of the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_c_abi_refusals():
    from diffsg_amd import _lib
    L = _lib.lib()
    buf = torch.ones(1024, device="cuda", dtype=torch.float64)       # room for 4 rows of the widest problem
    X, Y, rec, null = _lib.ptr(buf), _lib.ptr(buf.clone()), _lib.ptr(buf.clone()), ctypes.c_void_p(0)
    st = _lib.stream_ptr()
    co = lambda X=X, Y=Y, B=4, n=3, iters=1, rec=null, every=0: L.dsg_gd_co(X, Y, B, n, iters, 0.1, 1.0, 1.0, rec, every, st)
    msr = lambda X=X, Y=Y, B=4, M=3, iters=1, rec=null, every=0: L.dsg_gd_msr(X, Y, B, M, iters, 0.001, rec, every, st)
    nu = lambda X=X, Y=Y, B=4, K=3, iters=1, rec=null, every=0: L.dsg_gd_nu(X, Y, B, K, iters, 0.1, 18.0, rec, every, st)

    def refused(rc, who):
        assert rc != 0 and who in L.dsg_last_error().decode()

    refused(co(n=17), "dsg_gd_co"); refused(co(n=0), "dsg_gd_co")
    refused(msr(M=129), "dsg_gd_msr"); refused(msr(M=0), "dsg_gd_msr")
    refused(nu(K=33), "dsg_gd_nu"); refused(nu(K=0), "dsg_gd_nu")
    for fn, who in ((co, "dsg_gd_co"), (msr, "dsg_gd_msr"), (nu, "dsg_gd_nu")):
        refused(fn(B=-1), who)
        refused(fn(iters=-1), who)
        refused(fn(every=-1), who)
        refused(fn(rec=rec, every=0), who)
        refused(fn(X=null), who)
        refused(fn(Y=null), who)
        assert fn(X=null, Y=null, B=0) == 0          # nothing to do: no launch, no pointer read
        assert fn(iters=0) == 0
    assert co(n=16) == 0 and msr(M=128) == 0 and nu(K=32) == 0      # the limits themselves are served
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# 6. drivers on the fixture files
# ---------------------------------------------------------------------------------------------------------------------
# Tolerances of the evaluators' own parity test (tests/test_gpu_parity.py::test_decoders_match_reference_goldens): max |a - b| <= tol *
# max |b| with 2e-6 for co_cost and msr_rate, 1e-5 for nu_rate.  A figure is formed from two such vectors (predicted and true): the
# ratio of their sums is held to 2 * tol relative, the mean of their difference to 2 * tol * max |objective|.
DRIVER_TOL = {"co": 2e-6, "msr3": 2e-6, "nu": 1e-5}


def run_driver(p, it):
    from diffsg_amd import gd
    if p == "co":
        return gd.gd_co(CO_CSV, iterations=it, log=None)
    if p == "msr3":
        return gd.gd_msr(MSR_CSV, iterations=it, log=None)
    return gd.gd_nu(NU_CSV, iterations=it, log=None)


def check_driver(g16, p, it, out, keep, figures):
    tol = DRIVER_TOL[p]
    gp, gt = g16[f"drv.{p}.{it}.pred"].astype(np.float64), g16[f"drv.{p}.{it}.true"].astype(np.float64)
    pred, true = out["pred"].double().cpu().numpy(), out["true"].double().cpu().numpy()
    assert pred.shape == gp.shape and keep.any()
    scale = max(np.abs(gp[keep]).max(), np.abs(gt[keep]).max())
    e_pred, e_true = np.abs(pred[keep] - gp[keep]).max() / np.abs(gp[keep]).max(), np.abs(true[keep] - gt[keep]).max() / np.abs(gt[keep]).max()
    print(f"driver {p} at {it}: {int(keep.sum())} of {keep.size} rows, per-row error pred {e_pred:.3g}, true {e_true:.3g} (bar {tol:g})")
    assert e_pred <= tol and e_true <= tol
    if not figures:
        return
    ratio, gratio = pred[keep].sum() / true[keep].sum(), gp[keep].sum() / gt[keep].sum()
    diff, gdiff = np.mean(pred[keep] - true[keep]), np.mean(gp[keep] - gt[keep])
    print(f"driver {p} at {it}: sum_ratio {ratio:.8f} (reference {gratio:.8f}), mean_diff {diff:.8g} (reference {gdiff:.8g})")
    assert abs(ratio - gratio) <= 2 * tol * abs(gratio) and abs(diff - gdiff) <= 2 * tol * scale
    if keep.all():      # nothing left out: the driver's own figures are the reference's
        assert abs(out["sum_ratio"] - float(g16[f"drv.{p}.{it}.sum_ratio"])) <= 2 * tol * abs(gratio)
        assert abs(out["mean_diff"] - float(g16[f"drv.{p}.{it}.mean_diff"])) <= 2 * tol * scale


@pytest.mark.parametrize("p", ["co", "msr3", "nu"])
def test_drivers_at_20_iterations(g16, p):
    Y, out = run_driver(p, 20)
    assert Y.shape == g16[f"drv.{p}.20.Y"].shape and set(out) >= {"sum_ratio", "mean_diff"}
    keep = GR.co_far_from_threshold(g16["drv.co.20.norm"]) if p == "co" else np.ones(Y.shape[0], dtype=bool)
    assert keep.mean() >= 0.98
    check_driver(g16, p, 20, out, keep, figures=True)


@pytest.mark.parametrize("p", ["co", "msr3", "nu"])
def test_drivers_at_100_iterations(g16, p):
    Y, out = run_driver(p, 100)
    if p == "co":       # per row, and only where the reference's own run is well conditioned and its decisions are off the threshold
        x = g16["drv.co.x"]
        keep = (GR.twin_dev("co", x, GR.co_init(x.shape[0], 3), 100) <= 1e-9) & GR.co_far_from_threshold(g16["drv.co.100.norm"])
        check_driver(g16, p, 100, out, keep, figures=False)
    else:
        check_driver(g16, p, 100, out, np.ones(Y.shape[0], dtype=bool), figures=True)


def test_driver_takes_fewer_rows_when_asked(g16):
    from diffsg_amd import gd
    Y, out = gd.gd_msr(MSR_CSV, used_sample_num=7, iterations=20, log=None)
    assert Y.shape == (7, 3) and out["pred"].shape == (7,)
    assert np.abs(out["pred"].cpu().numpy() - g16["drv.msr3.20.pred"][:7]).max() <= 2e-6 * np.abs(g16["drv.msr3.20.pred"]).max()
