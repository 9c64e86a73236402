"""NU label generator on the device (dsg_noma_uav_search via diffsg_amd.labelgen.noma_uav_gen) against the reference's own
outputs (tests/golden/g12_noma_uav_gen.npz) and, on inputs the goldens do not cover, the CPU restatement (tests/nu_gen_ref.py).

The device's float64 arithmetic is the reference's step for step except log2 (numpy's and the device library's are each within
about an ulp, not identical), so a sample passes if its outputs are identical, or the choice is the same and the rate agrees
to 1e-13 relative, or the choices differ and the restatement's rate AT the device's choice is within 1e-13 relative of the
best rate: a near-tie.  Near-ties are counted and printed."""
import os

import numpy as np
import pytest
import torch

import nu_gen_ref as N

pytestmark = pytest.mark.gpu

TOL = 1e-13


def _judge(qs, fs, got, want):
    """Returns the number of near-ties; asserts the rule above for every sample."""
    ties = 0
    for i in range(qs.shape[0]):
        g, w = got[i], want[i]
        if np.array_equal(g, w):
            continue
        assert w[5] != 0.0 and g[5] != 0.0, (i, g, w)
        if np.array_equal(g[:5], w[:5]):
            assert abs(g[5] - w[5]) <= TOL * abs(w[5]), (i, g, w)
            continue
        r = N.rate_at(qs[i], fs, g[0], g[1], g[2:5])
        assert np.isfinite(r) and abs(r - w[5]) <= TOL * abs(w[5]), (i, g, w, r)
        assert abs(g[5] - r) <= TOL * abs(r), (i, g, r)
        ties += 1
    return ties


def _run(qs, P, **kw):
    from diffsg_amd.labelgen import noma_uav_gen
    out = noma_uav_gen(qs.shape[0], P, qs=qs, **kw)
    assert out.shape == (qs.shape[0], 12) and out.dtype == np.float64
    assert np.array_equal(out[:, :6], qs)
    return out[:, 6:]


@pytest.mark.parametrize("P", [18, 30, 6])
def test_noma_uav_gen_matches_reference_goldens(gold, P):
    from diffsg_amd.labelgen import feasible_solution, noma_uav_gen
    import hashlib
    g = gold("g12_noma_uav_gen.npz")
    ref = g[f"P{P}_out"]
    fs = feasible_solution(P)
    assert hashlib.sha256(fs.tobytes()).hexdigest() == str(g[f"P{P}_fs_sha256"])
    np.random.seed(int(g[f"P{P}_seed"]))
    logs = []
    out = noma_uav_gen(ref.shape[0], P, log=logs.append)
    assert np.array_equal(out[:, :6], ref[:, :6])                  # features: the reference's draws
    ties = _judge(ref[:, :6], fs, out[:, 6:], ref[:, 6:])
    exact = int(np.all(out == ref, axis=1).sum())
    print(f"\nP_sum = {P}: {exact}/{ref.shape[0]} rows bit-identical, {ties} near-ties")
    assert not logs


@pytest.mark.parametrize("P,n,seed", [(18, 200, 501), (30, 40, 502), (18, 1, 503)])
def test_noma_uav_gen_vs_restatement(P, n, seed):
    from diffsg_amd.labelgen import coordinates_gen, feasible_solution
    np.random.seed(seed)
    qs = coordinates_gen(n)
    fs = feasible_solution(P)
    got = _run(qs, P)
    want = N.noma_uav_search(qs, fs, workers=N.default_workers())
    ties = _judge(qs, fs, got, want)
    print(f"\nP_sum = {P}, {n} samples: {int(np.all(got == want, axis=1).sum())} bit-identical, {ties} near-ties")


def test_equidistant_users_rank_tie():
    """Users 0 and 2 mirror each other about x = 200, so on that column their h are equal and the lower index ranks first;
    users placed so that the best point sits on the mirror line."""
    from diffsg_amd.labelgen import feasible_solution
    qs = np.array([[150.0, 100.0, 200.0, 300.0, 250.0, 100.0],
                   [100.0, 200.0, 300.0, 200.0, 200.0, 200.0],     # degenerate: all three on y = 200 (the whole line counts)
                   [200.0, 120.0, 260.0, 180.0, 140.0, 180.0]])
    fs = feasible_solution(18)
    got = _run(qs, 18)
    want = N.noma_uav_search(qs, fs)
    _judge(qs, fs, got, want)
    # the tie rule is exercised: some inside point of sample 0 has two equal h
    pts = N.inside_points(qs[0])
    x = pts % 401
    assert np.any(x == 200)


def test_triangle_without_grid_points_gives_zero_row():
    from diffsg_amd.labelgen import noma_uav_gen
    qs = np.array([[10.2, 10.1, 10.8, 10.3, 10.5, 10.9],          # inside no integer point
                   [20.0, 30.0, 390.0, 40.0, 200.0, 380.0],
                   [-50.0, -50.0, -10.0, -40.0, -30.0, -5.0]])       # outside the area
    logs = []
    out = noma_uav_gen(3, 18, qs=qs, log=logs.append)
    assert np.all(out[0, 6:] == 0) and np.all(out[2, 6:] == 0) and out[1, 11] > 0
    assert logs == [0, 2]


def test_noma_uav_gen_is_deterministic():
    from diffsg_amd.labelgen import coordinates_gen
    np.random.seed(77)
    qs = coordinates_gen(96)
    a = _run(qs, 18)
    b = _run(qs, 18)
    assert np.array_equal(a, b)
    one = _run(qs[5:6], 18)                   # the small-call tiling gives the same label
    assert np.array_equal(one[0], a[5])


def test_nu_dataset_store_round_trip(tmp_path):
    from diffsg_amd.trajectory import nu_dataset_store
    from diffsg_amd.classifier_free_NU import nu_data_load
    np.random.seed(3)
    out_csv = str(tmp_path / "3u_18mW_20samples.csv")
    table, ext = nu_dataset_store(out_csv, sample_num=20, P_sum=18, extend=True, log=lambda *_: None)
    assert table.shape == (20, 12) and ext.shape == (60, 12)
    assert os.path.exists(str(tmp_path / "3u_18mW_extension.csv"))
    X_tr, Y_tr, X_te, Y_te, R_te, cfg = nu_data_load(out_csv, 400, 400)
    assert cfg["P_sum"] == 18.0 and cfg["K"] == 3
    assert X_tr.shape == (14, 6) and Y_tr.shape == (14, 5) and X_te.shape == (6, 6) and Y_te.shape == (6, 5)
    # pandas' default CSV float parser (what nu_data_load reads with) is not round-trip exact: ~1e-13 relative
    assert np.allclose(X_tr * 400, table[:14, :6], rtol=1e-12, atol=0)
    assert np.allclose(Y_te[:, :2] * 400, table[-6:, 6:8], rtol=1e-12, atol=0)
    assert np.allclose(Y_te[:, 2:] * 18, table[-6:, 8:11], rtol=1e-12, atol=0)
    assert np.allclose(R_te, table[-6:, 11], rtol=1e-12, atol=0)
    # default name carries P_sum and the row count
    cwd = os.getcwd()
    os.makedirs(tmp_path / "datasets")
    os.makedirs(tmp_path / "w")
    os.chdir(tmp_path / "w")
    try:
        nu_dataset_store(sample_num=3, P_sum=30, log=lambda *_: None)
    finally:
        os.chdir(cwd)
    assert os.path.exists(tmp_path / "datasets" / "3u_30mW_3samples.csv")


def test_abi_rejects_bad_arguments():
    from diffsg_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda")
    q = torch.zeros(2, 6, device=dev, dtype=torch.float64)
    f = torch.ones(16, 3, device=dev, dtype=torch.float64)
    o = torch.empty(2, 6, device=dev, dtype=torch.float64)
    P, Z, s = _lib.ptr, _lib.ptr(None), _lib.stream_ptr()
    for args in ((Z, P(f), 16, P(o), 2), (P(q), Z, 16, P(o), 2), (P(q), P(f), 16, Z, 2),
                 (P(q), P(f), 0, P(o), 2), (P(q), P(f), 2, P(o), 2), (P(q), P(f), 16385, P(o), 2),
                 (P(q), P(f), 16, P(o), -1)):
        assert L.dsg_noma_uav_search(*args, 110.0, 60.0, 150.0, s) != 0, args
    assert L.dsg_noma_uav_search(P(q), P(f), 16, P(o), 0, 110.0, 60.0, 150.0, s) == 0    # rows = 0: no-op
    torch.cuda.synchronize()


def test_nu_search_kernels_use_no_scratch():
    from diffsg_amd import _lib
    res = _lib.kernel_resources()
    names = [n for n in res if "k_nu_tiles" in n or "k_nu_pick" in n]
    assert len(names) == 2, names
    assert all(res[n]["scratch"] == 0 for n in names), {n: res[n] for n in names}
