"""The start-up chain of the persistent wide kernels: k_panel128_h / k_panel128_duo_h issue their first tile's requests
as their first memory operations, stage every per-feature vector from one batch of loads and receive the step's time-bias row by
LDS-DMA; k_res64_lds / k_res64_dual load the first tile's input together with the block's image.  No value changes: every comparison
here is `torch.equal`, against tests/golden/g20_launch_preamble.npz -- y_0 as the build of the commit BEFORE that change computed it
on an MI355X (tests/golden/make_g20_launch_preamble.py; never regenerated from the tree under test) -- and between runs.

MSR-80c net of bench.py, set_launch_policy(0, 0): the persistent forms at every size.  T = 6: four renorm steps run eagerly, two from
the graph, and every step reads its own time-bias row, so a stale or late row shows.  32 rows: one live wave, the idle ones still stage
their share of the vectors and meet every barrier; 100: a ragged last tile; 160 / 295: a second and a third group."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T = 6
SEED = 7
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g20_launch_preamble.npz")

_cache = {}


def golden():
    if "g" not in _cache:
        with np.load(GOLDEN) as z:
            _cache["g"] = {k: z[k] for k in z.files}
    return _cache["g"]


def parent_y0(B, omega, half):
    """Stored once as `..._h` where the parent gave the same bits under both panel_half settings, else per setting."""
    g = golden()
    base = f"y0_B{B}_w{int(round(omega * 10)):02d}_h"
    return torch.from_numpy(g[base] if base in g else g[base + str(half)])


def model():
    if "m" not in _cache:
        import bench
        ddpm = bench.build_model(torch.device("cuda:0"), T)
        ddpm.model.set_launch_policy(0, 0)
        _cache["m"] = ddpm
    return _cache["m"]


def cond_of(B, seed=4):
    return torch.rand(B, 80, generator=torch.Generator().manual_seed(seed)).cuda()


@pytest.mark.parametrize("half", [1, 0])
@pytest.mark.parametrize("omega", [1.0, 0.3])
@pytest.mark.parametrize("B", [32, 100, 160, 295])
def test_bit_for_bit_against_parent_and_between_runs(B, omega, half):
    """Three consecutive calls equal the parent commit's y_0 (hence each other); the eager path (profile=True) equals the graph path.
    (The first-panel race of round 5 showed only as run-to-run differences.)"""
    ddpm = model()
    ddpm.model.set_option("panel_half", half)
    cond = cond_of(B)
    ref = parent_y0(B, omega, half)
    runs = [ddpm.sample(cond, omega, seed=SEED).cpu() for _ in range(3)]
    for rep, y in enumerate(runs):
        assert torch.isfinite(y).all()
        assert torch.equal(y, runs[0]), (B, omega, half, rep, "run-to-run")
        assert torch.equal(y, ref), (B, omega, half, rep, float((y - ref).abs().max()))
    eager = ddpm.sample(cond, omega, seed=SEED, profile=True).cpu()
    assert torch.equal(eager, runs[0]), (B, omega, half, "eager vs graph")
    assert not ddpm.model.range_exceeded()


def test_wide_instances_of_the_step_fit():
    """Every k_panel128_* and k_res64_* instance: no scratch, two waves per SIMD or more; two workgroups' LDS fit the CU's 160 KiB
    wherever they did before the change (the half-panel forms and the down-64 block without a consuming Linear)."""
    from diffsg_amd import _lib
    res = _lib.kernel_resources()
    wide = {k: r for k, r in res.items() if k.startswith("dsg::k_panel128_") or k.startswith("dsg::k_res64_")}
    assert any("k_panel128_duo_h" in k for k in wide) and any("k_res64_dual" in k for k in wide) and any("k_res64_lds" in k for k in wide), sorted(wide)
    for k, r in sorted(wide.items()):
        print(k, r)
        assert r["scratch"] == 0, (k, r)
        assert r["occupancy"] >= 2, (k, r)
    # LDS of the parent commit's build, bytes per workgroup: instances with 2 x lds <= 160 KiB there
    two_per_cu = [k for k in wide if k in PARENT_TWO_PER_CU]
    assert sorted(two_per_cu) == sorted(PARENT_TWO_PER_CU), (sorted(two_per_cu), sorted(wide))
    for k in two_per_cu:
        assert 2 * wide[k]["lds"] <= 160 * 1024, (k, wide[k])


# the instances of the parent commit's build whose LDS let two workgroups share a CU (its libdiffsg_hip.resources.txt)
PARENT_TWO_PER_CU = (
    "dsg::k_panel128_duo_h<2>",
    "dsg::k_panel128_h<false, 0, 1, 2>", "dsg::k_panel128_h<false, 1, 1, 2>", "dsg::k_panel128_h<false, 1, 2, 2>",
    "dsg::k_panel128_h<true, 0, 1, 2>", "dsg::k_panel128_h<true, 2, 1, 2>", "dsg::k_panel128_h<true, 2, 3, 2>",
    "dsg::k_res64_lds<false, 0>", "dsg::k_res64_lds<false, 1>", "dsg::k_res64_lds<false, 2>",
)
