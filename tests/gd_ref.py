"""float64 numpy restatement of the gradient-descent baseline (reference: baselines/GD.py), general in n, M and K.

Written from the formulas, in this project's words.  Every expression keeps the reference's left-to-right order, so on float64 inputs
the states are the reference's bit for bit (tests/test_gd_cpu.py checks that against tests/golden/g16_gd.npz); with
`dtype=np.longdouble` the same code is the higher-precision yardstick of the conditioning checks.  Row sums are added one column after
another: that is numpy's own order below 8 columns, and the order the device uses for CO and NU at any size.
"""
import numpy as np

LN2 = np.log(2)
TEACHER = (0, 1, 2, 3, 5, 10, 20, 50, 99)       # the states a single step is checked from
STATES = tuple(sorted({k for t in TEACHER for k in (t, t + 1)} - {0}))      # the iterations whose state the goldens keep: those and their successors


def rowsum(a):
    """Columns added left to right."""
    s = a[:, 0].copy()
    for j in range(1, a.shape[1]):
        s = s + a[:, j]
    return s


# ---------------------------------------------------------------------------------------------------------------------
# start states
# ---------------------------------------------------------------------------------------------------------------------
def co_init(rows, n):
    y = np.ones((rows, 2 * n))
    y[:, n:] = 1 / n
    return y


def msr_init(rows, M, W):
    return np.ones((rows, M)) / M * W


def nu_init(rows, K, P_sum, width, height):
    y = np.ones((rows, 2 + K)) * P_sum / K - 0.01
    y[:, 0], y[:, 1] = width / 2, height / 2
    return y


# ---------------------------------------------------------------------------------------------------------------------
# one step
# ---------------------------------------------------------------------------------------------------------------------
def co_step(x, y, lr=0.1, lambda1=1.0, lambda2=1.0):
    n = y.shape[1] // 2
    g = np.zeros_like(y)
    S = rowsum(y[:, n:])
    for i in range(n):
        a, d = y[:, n + i], y[:, i]
        g[:, i] = -x[:, 3 * i] + x[:, 3 * i + 1] + x[:, 3 * i + 2] / a + (1 - 2 * d) * lambda1
        g[:, n + i] = -x[:, 3 * i + 2] / (a * a) * d + (S * 2 - 1) * lambda2
    return y - g * lr


def msr_step(gs, s, lr=0.001, sum_fn=None):
    """sum_fn: the row sum (its order is free: the device's differs from numpy's at M > 8)."""
    tot = (sum_fn or (lambda a: np.sum(a, axis=1)))(s)
    g = gs / ((gs * s + 1.0) * LN2) - (1.0 / ((tot - 1) * (tot - 1)))[:, None]
    return s + g * lr


def nu_step(c, y, lr=0.1, p_ref=18.0):
    K = y.shape[1] - 2
    px, py = y[:, 0], y[:, 1]
    d = [(px - c[:, 2 * i]) * (px - c[:, 2 * i]) + (py - c[:, 2 * i + 1]) * (py - c[:, 2 * i + 1]) for i in range(K)]
    D = d[0]
    for i in range(1, K):
        D = D + d[i]
    P = rowsum(y[:, 2:])
    g = np.zeros_like(y)
    for i in range(K):
        p = y[:, 2 + i]
        tmp = 6 + 11 / 6 * (22500 + d[i])
        q = 1 + p / tmp
        # the second term of BOTH position components reads the user's Y coordinate (the reference's quirk)
        g[:, 0] = g[:, 0] + (-p * (px - c[:, 2 * i]) * 11 / 3 / (tmp * tmp) / q / LN2 + 2 * (c[:, 2 * i + 1] - px) / (D * D))
        g[:, 1] = g[:, 1] + (-p * (py - c[:, 2 * i + 1]) * 11 / 3 / (tmp * tmp) / q / LN2 + 2 * (c[:, 2 * i + 1] - py) / (D * D))
        g[:, 2 + i] = -1 / tmp / q / LN2 + 1 / ((P - p_ref) * (P - p_ref))
    return y + g * lr


STEP = {"co": co_step, "msr": msr_step, "nu": nu_step}


def run(kind, x, y0, iters, keep=(), **kw):
    """The state after `iters` steps, and {k: state after k steps} for k in keep."""
    step = STEP[kind]
    y, kept = np.array(y0, copy=True), {}
    with np.errstate(all="ignore"):
        for k in range(1, iters + 1):
            y = step(x, y, **kw)
            if k in keep:
                kept[k] = y.copy()
    return y, kept


# ---------------------------------------------------------------------------------------------------------------------
# conditioning
# ---------------------------------------------------------------------------------------------------------------------
def rel_dev(a, b):
    """Per row: max over the entries of |a - b| / (1 + |b|); a row with a non-finite entry on either side counts as inf unless the
    two rows are equal as such."""
    with np.errstate(all="ignore"):
        e = np.abs(a - b) / (1 + np.abs(b))
    bad = ~(np.isfinite(a) & np.isfinite(b))
    same = (np.isnan(a) & np.isnan(b)) | (a == b)
    e = np.where(bad, np.where(same, 0.0, np.inf), e)
    return e.max(axis=1)


def twin_dev(kind, x, y0, iters, **kw):
    """Per-row deviation after `iters` steps between the run from y0 and the run from y0 moved one ulp towards +inf."""
    a, _ = run(kind, x, y0, iters, **kw)
    b, _ = run(kind, x, np.nextafter(y0, np.inf), iters, **kw)
    return rel_dev(b, a)


def step_bound(yk, yk1, factor=1e-14):
    return factor * (np.abs(yk) + np.abs(yk1))


def step_ok(got, yk, yk1, factor=1e-14):
    """got == yk1 within factor * (|yk| + |yk1|) element-wise; non-finite entries equal as such.  Returns (ok, worst ratio)."""
    fin = np.isfinite(yk1)
    same_nonfinite = np.array_equal(np.isnan(got), np.isnan(yk1)) and np.array_equal(got[~fin & ~np.isnan(yk1)], yk1[~fin & ~np.isnan(yk1)])
    with np.errstate(all="ignore"):
        bound = step_bound(yk, yk1, factor)
        ratio = np.where(fin, np.abs(got - yk1) / np.where(bound > 0, bound, 1.0), 0.0)
        ok = np.where(fin, np.abs(got - yk1) <= bound, True)
    return bool(same_nonfinite and ok.all()), float(ratio.max()) if ratio.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the drivers' closing steps that are plain numpy (the evaluators are the package's / the reference's)
# ---------------------------------------------------------------------------------------------------------------------
def co_minmax(alloc32):
    """Per-row min-max of the float32 allocations (GD.py:43-45)."""
    lo, hi = alloc32.min(axis=1, keepdims=True), alloc32.max(axis=1, keepdims=True)
    with np.errstate(all="ignore"):
        return (alloc32 - lo) / (hi - lo)


def co_far_from_threshold(norm, margin=1e-4):
    """Rows whose min-max-normalised allocations all stay `margin` away from cost_calc's 0.1 decision threshold (and are finite)."""
    return np.isfinite(norm).all(axis=1) & (np.abs(norm - 0.1) > margin).all(axis=1)


def msr_finish(Y, X, W):
    """GD.py:85-87: spread the budget's remainder evenly, then the rate in float64."""
    M = Y.shape[1]
    Y = Y + (W - np.atleast_2d(np.sum(Y, axis=1)).T) / M
    return Y, np.sum(np.log2(1.0 + Y * X), axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# synthetic inputs of the shape tests
# ---------------------------------------------------------------------------------------------------------------------
def synth(kind, B, size, seed=0):
    """(x, y0) for B rows of problem size `size`: CO x in (0.03, 10) as the loader guarantees, MSR gains in (0.1, 5) with W = 10,
    NU coordinates in (0, 1) with P_sum = 18 on a 400 x 400 field."""
    r = np.random.default_rng(1000 * seed + 17 * size + B)
    if kind == "co":
        return 0.03 + 9.97 * r.random((B, 3 * size)), co_init(B, size)
    if kind == "msr":
        return 0.1 + 4.9 * r.random((B, size)), msr_init(B, size, 10.0)
    return r.random((B, 2 * size)), nu_init(B, size, 18.0, 400, 400)
