"""CPU restatement of the NU label search (datasets/noma_uav_gen.py, noma_uav_gen): numpy, vectorised over grid points and
power-table rows in bounded chunks, every float64 step in the reference's order.  Bit-identical to the reference's outputs
(tests/golden/g12_noma_uav_gen.npz); the device tests use it as the oracle on inputs the goldens do not cover.

Per grid point p = y * 401 + x inside the users' triangle (edges included):
    h[u]  = sqrt(rou_0 / ((H^2 + dx_u^2) + dy_u^2)),  ranks: h descending, equal h -> lower user index first
    F[s][u] = fs[s][rank(u)]
    sinr of the rank-0 user  = (F * h^2) / sigma^2
    sinr of the rank-r user  = F / (S_r + sigma^2 / h^2),  S_r = all 3r entries of table ROWS u_0 .. u_{r-1} of F (the
                               stronger users' indices used as row numbers), added one after another in memory order
    rate = (log2(1 + sinr_0) + log2(1 + sinr_1)) + log2(1 + sinr_2)   (user order)
The label is the first maximum over rows at each point and then the first maximum over points in grid order.
"""
import numpy as np

GRID = 401
SIGMA_SQ, ROU_0, H = 110.0, 60.0, 150.0


def inside_points(q):
    """Indices p (ascending) of the grid points inside the triangle q = (x0, y0, x1, y1, x2, y2)."""
    p = np.arange(GRID * GRID)
    x, y = (p % GRID).astype(np.float64), (p // GRID).astype(np.float64)

    def cross(ax, ay, b, c):
        return (ax - c[0]) * (b[1] - c[1]) - (b[0] - c[0]) * (ay - c[1])
    b, c, d = q[0:2], q[2:4], q[4:6]
    s1, s2, s3 = cross(x, y, b, c), cross(x, y, c, d), cross(x, y, d, b)
    neg = (s1 < 0) | (s2 < 0) | (s3 < 0)
    pos = (s1 > 0) | (s2 > 0) | (s3 > 0)
    return p[~(neg & pos)]


def point_constants(q, fs, pts, sigma_sq=SIGMA_SQ, rou_0=ROU_0, H=H):
    """Per point: rank [n][3] of every user, h^2 of the rank-0 user, and the denominators D1, D2 of ranks 1, 2."""
    x, y = (pts % GRID).astype(np.float64), (pts // GRID).astype(np.float64)
    h = np.empty((pts.size, 3))
    for u in range(3):
        dx, dy = x - q[2 * u], y - q[2 * u + 1]
        h[:, u] = np.sqrt(rou_0 / (H * H + dx * dx + dy * dy))
    order = np.argsort(-h, axis=1, kind="stable")           # order[:, r] = user of rank r
    rank = np.argsort(order, axis=1, kind="stable")
    hh = h * h
    ar = np.arange(pts.size)
    S = np.zeros(pts.size)
    D = []
    for r in (1, 2):
        row = fs[order[:, r - 1]]                           # table row numbered by the user of rank r - 1
        for u in range(3):
            S = S + row[ar, rank[:, u]]
        D.append(S + sigma_sq / hh[ar, order[:, r]])
    return rank, hh[ar, order[:, 0]], D[0], D[1]


def rates(q, fs, pts, sigma_sq=SIGMA_SQ, rou_0=ROU_0, H=H):
    """[len(pts)][len(fs)] rate of every table row at every point."""
    rank, a, D1, D2 = point_constants(q, fs, pts, sigma_sq, rou_0, H)
    L = np.stack((np.log2(1 + (fs[None, :, 0] * a[:, None]) / sigma_sq),
                  np.log2(1 + fs[None, :, 1] / D1[:, None]),
                  np.log2(1 + fs[None, :, 2] / D2[:, None])))   # [rank][point][row]
    ar = np.arange(pts.size)
    Lu = [L[rank[:, u], ar] for u in range(3)]
    return (Lu[0] + Lu[1]) + Lu[2]


def search_one(q, fs, chunk_elems=1 << 22, **kw):
    """[6] = x, y, powers (user order), rate of one sample; zeros if no grid point is inside."""
    q = np.asarray(q, dtype=np.float64)
    pts = inside_points(q)
    best = None
    step = max(1, chunk_elems // fs.shape[0])
    for lo in range(0, pts.size, step):
        sub = pts[lo:lo + step]
        R = rates(q, fs, sub, **kw)
        s = np.argmax(R, axis=1)
        r = R[np.arange(sub.size), s]
        k = int(np.argmax(r))
        if best is None or r[k] > best[0]:
            best = (r[k], int(sub[k]), int(s[k]))
    if best is None:
        return np.zeros(6)
    return label_row(q, fs, best[1], best[2], **kw)


def label_row(q, fs, p, s, **kw):
    """[6] output row for the choice (grid point p, table row s)."""
    pts = np.array([p])
    rank = point_constants(np.asarray(q, dtype=np.float64), fs, pts, **kw)[0][0]
    return np.concatenate(([p % GRID, p // GRID], fs[s, rank], rates(np.asarray(q, dtype=np.float64), fs, pts, **kw)[0, s:s + 1]))


def rate_at(q, fs, x, y, powers, **kw):
    """The restatement's rate at an output row's choice (x, y, powers in user order); NaN if the powers are no table row
    under that point's ranking."""
    q = np.asarray(q, dtype=np.float64)
    p = int(round(y)) * GRID + int(round(x))
    rank = point_constants(q, fs, np.array([p]), **kw)[0][0]
    hit = np.flatnonzero(np.all(fs[:, rank] == np.asarray(powers), axis=1))
    if hit.size == 0:
        return float("nan")
    return float(rates(q, fs, np.array([p]), **kw)[0, hit[0]])


def default_workers():
    """Threads for noma_uav_search: numpy's ufunc loops release the GIL; bounded by the job's thread budget, not the box."""
    import os
    return max(1, min(16, int(os.environ.get("OMP_NUM_THREADS", "8") or 8)))


def noma_uav_search(qs, fs, workers=1, **kw):
    """[n][6] labels of every sample in qs [n][6] (samples spread over `workers` threads)."""
    qs = np.atleast_2d(np.asarray(qs, dtype=np.float64))
    if workers <= 1 or qs.shape[0] <= 1:
        return np.stack([search_one(q, fs, **kw) for q in qs])
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=workers) as ex:
        return np.stack(list(ex.map(lambda q: search_one(q, fs, **kw), qs)))
