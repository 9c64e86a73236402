"""NU label generator, host side (no GPU): the CPU restatement of the search (tests/nu_gen_ref.py) and the numpy parts of
diffsg_amd.labelgen (user draws, power table, augmentation) against the reference's own outputs
(tests/golden/g12_noma_uav_gen.npz, written by tests/golden/make_goldens_nu.py)."""
import hashlib
import os

import numpy as np
import pytest
import torch

from _util import GOLD
import nu_gen_ref as N

CASES = (18, 30, 6)


@pytest.mark.parametrize("P", CASES)
def test_feasible_solution_matches_reference(gold, P):
    from diffsg_amd.labelgen import feasible_solution
    g = gold("g12_noma_uav_gen.npz")
    t = f"P{P}"
    fs = feasible_solution(P)
    assert fs.dtype == np.float64 and fs.flags.c_contiguous
    assert tuple(fs.shape) == tuple(g[t + "_fs_shape"])
    assert np.array_equal(fs[0], g[t + "_fs_first"]) and np.array_equal(fs[-1], g[t + "_fs_last"])
    assert hashlib.sha256(fs.tobytes()).hexdigest() == str(g[t + "_fs_sha256"])


@pytest.mark.parametrize("P", CASES)
def test_coordinates_gen_reproduces_reference_draws(gold, P):
    from diffsg_amd.labelgen import coordinates_gen
    g = gold("g12_noma_uav_gen.npz")
    out = g[f"P{P}_out"]
    np.random.seed(int(g[f"P{P}_seed"]))
    qs = coordinates_gen(out.shape[0])
    assert np.array_equal(qs, out[:, :6])
    # the draw after them is the same too: both consumed exactly the reference's calls
    np.random.seed(int(g[f"P{P}_seed"]))
    coordinates_gen(out.shape[0])
    a = np.random.randint(1 << 30)
    np.random.seed(int(g[f"P{P}_seed"]))
    coordinates_gen(out.shape[0])
    assert np.random.randint(1 << 30) == a


@pytest.mark.parametrize("P", CASES)
def test_restatement_reproduces_reference_labels(gold, P):
    """The numpy restatement of the search gives the reference's labels bit for bit (x, y, powers, rate)."""
    from diffsg_amd.labelgen import feasible_solution
    g = gold("g12_noma_uav_gen.npz")
    out = g[f"P{P}_out"]
    got = N.noma_uav_search(out[:, :6], feasible_solution(P), workers=N.default_workers())
    assert np.array_equal(got, out[:, 6:]), np.argwhere(got != out[:, 6:])


def test_restatement_rate_at_a_choice(gold):
    from diffsg_amd.labelgen import feasible_solution
    g = gold("g12_noma_uav_gen.npz")
    out = g["P6_out"]
    fs = feasible_solution(6)
    for row in out:
        assert N.rate_at(row[:6], fs, row[6], row[7], row[8:11]) == row[11]


def test_dataset_extension_matches_reference(gold):
    from diffsg_amd.labelgen import dataset_extension
    g = gold("g12_noma_uav_gen.npz")
    path = os.path.join(GOLD, "data", "3u_18mW_200samples.csv")
    np.random.seed(int(g["ext_seed"]))
    ext = dataset_extension(path)
    assert ext.shape == g["ext_out"].shape and np.array_equal(ext, g["ext_out"])
    # an array source is the same as its CSV
    import pandas as pd
    np.random.seed(int(g["ext_seed"]))
    assert np.array_equal(dataset_extension(np.array(pd.read_csv(path, header=None))), g["ext_out"])


def test_inside_triangle_counts_edges_and_corners():
    from diffsg_amd.labelgen import is_point_inside_triangle
    b, c, d = [0.0, 0.0], [4.0, 0.0], [0.0, 4.0]
    for a, want in (([0, 0], True), ([2, 2], True), ([1, 1], True), ([2, 0], True), ([3, 2], False), ([-1, 0], False)):
        assert bool(is_point_inside_triangle(a, b, c, d)) == want, a
    # the restatement's grid scan agrees with the elementwise test over the whole grid
    q = np.array([3.0, 5.0, 170.0, 2.0, 90.0, 140.0])
    x, y = np.meshgrid(np.arange(401), np.arange(401))
    mask = is_point_inside_triangle([x.ravel(), y.ravel()], q[0:2], q[2:4], q[4:6])
    assert np.array_equal(N.inside_points(q), np.flatnonzero(mask))


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_noma_uav_gen_without_device_raises():
    from diffsg_amd.labelgen import noma_uav_gen
    with pytest.raises(RuntimeError, match="no CPU path"):
        noma_uav_gen(2, 18, qs=np.array([[10.0, 10, 300, 20, 100, 300]] * 2))


def test_noma_uav_gen_rejects_bad_qs():
    from diffsg_amd.labelgen import noma_uav_gen
    with pytest.raises(ValueError):
        noma_uav_gen(1, 18, qs=np.zeros((1, 5)))
    with pytest.raises(ValueError):
        noma_uav_gen(1, 18, qs=np.array([[np.nan, 0, 1, 1, 2, 0]]))
