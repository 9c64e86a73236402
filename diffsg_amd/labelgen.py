"""Label generators on the device: SUM_RATE_GEN (MSR), CONV_CO_MINLP_GEN (CO) and noma_uav_gen (NU).

Reference: utils/dataset_generate.py:280-313 `SUM_RATE_GEN(sample_num, M, g_range, W)` ("LRH gradient descent", float64),
used by datasets/sum_rate_gen.py to write the `*c_*w_*samples.csv` training sets.  Same signature and return value
(gs, rates, schemes as numpy float64 arrays); the channel gains are drawn on the host with numpy's global generator exactly
as the reference draws them (or passed in), the 149 descent iterations run in libdiffsg_hip.so (csrc/dsg_labelgen.hpp).
"""
import numpy as np
import torch

from . import _lib


def SUM_RATE_GEN(sample_num=3, M=3, g_range=(0.5, 2.5), W=10.0, gs=None, device=None):
    if gs is None:
        gs = np.random.uniform(g_range[0], g_range[1], size=(sample_num, M))
    gs = np.ascontiguousarray(gs, dtype=np.float64)
    if gs.ndim != 2 or gs.shape[1] != M:
        raise ValueError(f"SUM_RATE_GEN: gs is {gs.shape}, expected (sample_num, {M})")
    if not torch.cuda.is_available():
        raise RuntimeError("SUM_RATE_GEN: no HIP device; libdiffsg_hip has no CPU path")
    dev = torch.device(device if device is not None else "cuda")
    g = torch.from_numpy(gs).to(dev)
    schemes = torch.empty_like(g)
    rates = torch.empty(g.shape[0], device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dsg_sum_rate_gen(_lib.ptr(g), _lib.ptr(schemes), _lib.ptr(rates), g.shape[0], M, float(W), _lib.stream_ptr()))
    return gs, rates.cpu().numpy(), schemes.cpu().numpy()


def range_random(mu, sigma, size, lower=None, upper=None):
    """utils/dataset_generate.py:5-24: normal draws, out-of-range entries re-drawn until none is left (numpy's global
    generator, same calls in the same order as the reference)."""
    arr = np.random.normal(mu, sigma, size)
    if lower is None or upper is None:
        return arr
    while np.any(arr < lower) or np.any(arr > upper):
        arr[arr < lower] = np.random.normal(mu, sigma, np.sum(arr < lower))
        arr[arr > upper] = np.random.normal(mu, sigma, np.sum(arr > upper))
    return arr


def CONV_CO_MINLP_GEN(node_num, sample_num, step=0.02, device=None, log=print):
    """utils/dataset_generate.py:147-245: labels of the conventional computation-offloading MINLP by exhaustive search
    (2^n decisions x the `step` allocation grid).  Same signature, draws and return value as the reference -- X
    [samples][6n + 7] features, Y [samples][2n + 1] = decision | allocation | cost -- and the same two report lines; the
    draws and the derived per-node quantities are numpy on the host (:169-184), the search runs in libdiffsg_hip.so
    (csrc/dsg_cogen.hpp, one workgroup per sample; the reference spends ~1 s per 3-node sample on it)."""
    import time
    if not torch.cuda.is_available():
        raise RuntimeError("CONV_CO_MINLP_GEN: no HIP device; libdiffsg_hip has no CPU path")
    F_t, kappa, P_t, P_I, theta, B, N0 = 2.5e9, 1e-28, 0.3, 0.1, 1.0, 10e5, 7.96159e-13
    n = int(node_num)
    params = np.empty((sample_num, 7, n), dtype=np.float64)
    X = np.empty((sample_num, 6 * n + 7), dtype=np.float64)
    for i in range(sample_num):
        s = range_random(2.5e5, 5e4, n, 0, 5e5).astype(int)
        c = s * 3e3
        f_local = range_random(5.0e8, 2.0e8, n, 0, 1e9).astype(int)
        alpha = np.random.rand(n)
        beta = 1 - alpha
        h = np.random.rand(n)
        sinr = P_t * (h ** 2) / (N0 + np.sum(P_t * (h ** 2)))
        r_u = B * np.log2(1 + sinr)
        cost_local = alpha * (c / f_local) + beta * (kappa * (f_local ** 2) * c)
        params[i] = (s, c, f_local, alpha, beta, r_u, cost_local)
        X[i, :6 * n] = np.stack((s, c, f_local, h, alpha, beta), axis=1).reshape(-1)
        X[i, 6 * n:] = (F_t, kappa, P_t, P_I, theta, B, N0)
    dev = torch.device(device if device is not None else "cuda")
    choices = np.arange(step, 1 + step, step)
    t0 = time.time()
    P = torch.from_numpy(params).to(dev)
    ch = torch.from_numpy(choices).to(dev)
    Y = torch.empty(sample_num, 2 * n + 1, device=dev, dtype=torch.float64)
    tol = torch.empty(sample_num, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dsg_co_minlp_search(_lib.ptr(P), _lib.ptr(ch), len(choices), _lib.ptr(Y), _lib.ptr(tol), sample_num, n,
                                                  F_t, P_t, P_I, theta, _lib.stream_ptr()))
    Yh, hits = Y.cpu().numpy(), int(tol.sum().item())
    log(f"{hits}/{sample_num} satisfy the tolerable delay.")
    log(f"{(time.time() - t0) * 1000 / max(sample_num, 1)} ms per sample.")
    return X, Yh


# ---------------------------------------------------------------------------------------------------------------------
# NU problem: datasets/noma_uav_gen.py (noma_uav_gen, dataset_extension).  K = 3 users in a 400 x 400 area, the UAV on the
# integer grid; the search over grid points x power splits runs in libdiffsg_hip.so (csrc/dsg_nugen.hpp), the draws, the
# power table and the augmentation are numpy on the host, in the reference's call order so that a seed gives its outputs.

NU_SIGMA_SQ, NU_ROU_0, NU_H = 110.0, 60.0, 150.0
NU_WIDTH = NU_HEIGHT = 400


def coordinates_gen(sample_num, K=3, width=400, height=400):
    """User positions [sample_num][2K] (integers stored as float64): every user lands in a quadrant no earlier user of the
    sample took (np.random.choice over the free ones), then x and y are drawn uniformly inside that quadrant, 1-based."""
    qs = np.zeros((sample_num, 2 * K))
    hw, hh = width // 2, height // 2
    for i in range(sample_num):
        taken = np.zeros(4, dtype=np.int64)
        for u in range(K):
            quad = np.random.choice(np.flatnonzero(taken == 0))
            taken[quad] = 1
            col, row = quad % 2, quad // 2
            qs[i, 2 * u] = np.random.randint(hw * col + 1, hw * (col + 1) + 1)
            qs[i, 2 * u + 1] = np.random.randint(hh * row + 1, hh * (row + 1) + 1)
    return qs


def feasible_solution(P_sum):
    """The power table [n][3] = (k, j, i) with k < j < i and k + j + i = P_sum on a 0.1 grid, rows ordered by i, then j.
    The grids are numpy's aranges with the reference's float bounds (their lengths depend on them), and k = (P - i) - j."""
    step = 0.1
    P = float(P_sum)
    rows = []
    for i in np.arange(P / 3 + step, P - 2 * step, step):
        j = np.arange((P - i) / 2 + step, P - i - step, step)
        if j.size:
            rows.append(np.stack(((P - i) - j, j, np.full_like(j, i)), axis=1))
    if not rows:
        raise ValueError(f"feasible_solution: no power split for P_sum = {P_sum}")
    return np.concatenate(rows)


def is_point_inside_triangle(a, b, c, d):
    """True if point a lies in the triangle (b, c, d), edges and corners included: the three edge cross products do not
    take both signs.  Works elementwise when a's coordinates are arrays."""
    def cross(p, q, r):
        return (p[0] - r[0]) * (q[1] - r[1]) - (q[0] - r[0]) * (p[1] - r[1])
    s1, s2, s3 = cross(a, b, c), cross(a, c, d), cross(a, d, b)
    neg = np.logical_or(np.logical_or(s1 < 0, s2 < 0), s3 < 0)
    pos = np.logical_or(np.logical_or(s1 > 0, s2 > 0), s3 > 0)
    return np.logical_not(np.logical_and(neg, pos))


def rotate_point(point, center, angle_degrees):
    """Rotation of `point` about `center` by `angle_degrees` counter-clockwise (the reference's expression order)."""
    t = np.radians(angle_degrees)
    x, y = point
    cx, cy = center
    dx, dy = x - cx, y - cy
    return np.cos(t) * dx - np.sin(t) * dy + cx, np.sin(t) * dx + np.cos(t) * dy + cy


def dataset_extension(src, times=3, width=400, height=400, rotation_angle_upper=10):
    """Augmented copies of an NU table (rows: 3 users | UAV x, y | powers | rate): `times` passes over the rows; per row one
    np.random.randint(2) picks a random translation that keeps the users inside the area (two more draws), or a point
    reflection through the area's centre followed by a rotation about the users' centroid by a whole number of degrees in
    [-upper, upper) (one more draw).  Powers and rate are copied.  `src` is a headerless CSV path or an array."""
    import pandas as pd
    if isinstance(src, (str, bytes)) or hasattr(src, "__fspath__"):
        src = np.array(pd.read_csv(src, header=None))
    src = np.asarray(src, dtype=np.float64)
    n = src.shape[0]
    xs, ys = [0, 2, 4, 6], [1, 3, 5, 7]
    ext = np.zeros((n * times, src.shape[1]))
    for t in range(times):
        for r in range(n):
            row, o = src[r], t * n + r
            ext[o] = row
            if np.random.randint(2) == 0:
                lo_x, hi_x = np.min(row[xs[:3]]), np.max(row[xs[:3]])
                lo_y, hi_y = np.min(row[ys[:3]]), np.max(row[ys[:3]])
                shift_x = (np.random.randint(width - hi_x) if width > hi_x else 0) - lo_x
                shift_y = (np.random.randint(height - hi_y) if height > hi_y else 0) - lo_y
                ext[o, xs] += shift_x
                ext[o, ys] += shift_y
                continue
            ext[o, xs] = width - row[xs]
            ext[o, ys] = height - row[ys]
            tri = ext[o, :6].reshape(3, 2).copy()
            centre = np.mean(tri, axis=0)
            angle = np.random.randint(low=-rotation_angle_upper, high=rotation_angle_upper)
            for u in range(3):
                ext[o, 2 * u], ext[o, 2 * u + 1] = rotate_point(tri[u], centre, angle)
            ext[o, 6], ext[o, 7] = rotate_point(ext[o, 6:8].copy(), centre, angle)
    return ext


def noma_uav_gen(sample_num, P_sum, qs=None, device=None, log=print):
    """datasets/noma_uav_gen.py: NU training rows [sample_num][12] float64 = users (6) | UAV x, y | powers (3, user order) |
    rate.  Per sample the UAV point of the 401 x 401 integer grid inside the users' triangle and the row of
    feasible_solution(P_sum) with the largest rate (first point in grid order, then first row, on ties).  The users are
    drawn with numpy's global generator as the reference draws them unless `qs` [sample_num][6] is given.  A sample whose
    triangle holds no grid point stays all zeros and its index is logged.

    The rate is the reference's generator formula, which differs from the evaluator rate_calc (dsg_nu_rate): the
    interference term of the user ranked r is the sum of ALL entries of table rows 0 .. r-1 picked by the stronger users'
    indices (one scalar per point), not the stronger users' powers."""
    fs = feasible_solution(P_sum)
    if qs is None:
        qs = coordinates_gen(sample_num)
    qs = np.ascontiguousarray(qs, dtype=np.float64)
    if qs.ndim != 2 or qs.shape[1] != 6:
        raise ValueError(f"noma_uav_gen: qs is {qs.shape}, expected (sample_num, 6)")
    if not np.all(np.isfinite(qs)):
        raise ValueError("noma_uav_gen: qs holds non-finite coordinates")
    if not torch.cuda.is_available():
        raise RuntimeError("noma_uav_gen: no HIP device; libdiffsg_hip has no CPU path")
    dev = torch.device(device if device is not None else "cuda")
    n = qs.shape[0]
    with torch.cuda.device(dev):
        q = torch.from_numpy(qs).to(dev)
        f = torch.from_numpy(np.ascontiguousarray(fs)).to(dev)
        out = torch.empty(n, 6, device=dev, dtype=torch.float64)
        _lib.check(_lib.lib().dsg_noma_uav_search(_lib.ptr(q), _lib.ptr(f), fs.shape[0], _lib.ptr(out), n, NU_SIGMA_SQ, NU_ROU_0,
                                                  NU_H, _lib.stream_ptr()))
        res = out.cpu().numpy()
    data = np.concatenate((qs, res), axis=1)
    for i in np.flatnonzero(~res.any(axis=1)):
        log(int(i))
    return data
