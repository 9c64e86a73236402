"""dsg_set_option(DSG_OPT_CFG_SHARE): down.0 of a two-pass reverse step runs its condition-free stages once per row tile
(csrc/dsg_panel.hpp, k_panel128_duo_h).

The ResidualBlock adds the condition embedding behind lin2 (UNetCF.py, ResidualBlock.forward) and down.0 reads the shared
feature_proj(y), so the LN1 statistics, lin1 and lin2 of the unconditional and of the conditional tile of a row tile are the same
bits.  The shared form computes them once and runs only `+ cond_emb`, lin3, the residual add and the store per pass, with the pieces
and the order of k_panel128_h: every comparison here is `torch.equal` against the form switched off.  The comparison with the CPU
oracle stays where it was (test_gpu_parity.py, test_gpu_shapes.py run with the form on by default).  All on the MSR-80c net of bench.py.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DUO = {2: "dsg::k_panel128_duo_h<2>", 4: "dsg::k_panel128_duo_h<4>"}
SOLO = {2: "dsg::k_panel128_h<false, 0, 1, 2>", 4: "dsg::k_panel128_h<false, 0, 1, 4>"}


def model(T, large=True):
    import bench
    ddpm = bench.build_model(torch.device("cuda:0"), T)
    if large:
        ddpm.model.set_launch_policy(0, 0)      # the persistent forms at every size
    return ddpm


def cond_of(B, seed=4):
    return torch.rand(B, 80, generator=torch.Generator().manual_seed(seed)).cuda()


@pytest.mark.parametrize("half", [1, 0])
@pytest.mark.parametrize("B", [32, 100, 160, 295])
def test_small_batches_bit_for_bit(B, half):
    """32 rows: one live wave and three (seven) idle ones that still meet every barrier; 100: a ragged last tile in exactly one half-panel
    group; 160: a second group with one live wave; 295.  omega 1.0 and 0.3 (omega 0 would hide a wrong unconditional pass).  Three runs
    of the shared form: the first-panel race of the half-panel form showed as run-to-run differences."""
    ddpm = model(3)
    ddpm.model.set_option("panel_half", half)
    cond = cond_of(B)
    for omega in (1.0, 0.3):
        ddpm.model.set_option("cfg_share", 0)
        ref = ddpm.sample(cond, omega, seed=7)
        assert torch.isfinite(ref).all()
        ddpm.model.set_option("cfg_share", 1)
        for rep in range(3):
            assert torch.equal(ddpm.sample(cond, omega, seed=7), ref), (B, half, omega, rep)
    assert not ddpm.model.range_exceeded()


def test_workgroup_walks_more_than_one_group():
    """65 536 + 96 rows: 2 051 row tiles = 513 half-panel groups on 512 workgroups, so one workgroup carries its private stream across
    a group seam."""
    ddpm = model(2, large=False)
    cond = cond_of(65536 + 96)
    ddpm.model.set_option("cfg_share", 0)
    ref = ddpm.sample(cond, 1.0, seed=7)
    ddpm.model.set_option("cfg_share", 1)
    for rep in range(2):
        assert torch.equal(ddpm.sample(cond, 1.0, seed=7), ref), rep


def test_graph_replay_equals_eager_launches():
    ddpm = model(3)
    cond = cond_of(295)
    graph = ddpm.sample(cond, 1.0, seed=7)
    assert torch.equal(ddpm.sample(cond, 1.0, seed=7, profile=True), graph)
    assert torch.equal(ddpm.sample(cond, 1.0, seed=7), graph)


def test_form_is_taken_and_fits():
    """Both instances are in the build, use no scratch, leave room for two workgroups per CU (half panels: 4-wave workgroups, so two
    waves per SIMD: at most 256 of the 512 registers each) and take no more LDS than the one-pass form; the step still has ONE
    down.0.res launch."""
    from diffsg_amd import _lib
    res = _lib.kernel_resources()
    for steps in (2, 4):
        assert DUO[steps] in res, sorted(k for k in res if "panel128" in k)
        r, solo = res[DUO[steps]], res[SOLO[steps]]
        print(DUO[steps], r)
        assert r["scratch"] == 0, r
        assert r["lds"] <= solo["lds"], (r, solo)
    r2 = res[DUO[2]]
    assert r2["vgprs"] + max(r2["agprs"], 0) <= 256 and r2["occupancy"] >= 2, r2
    assert 2 * r2["lds"] <= 160 * 1024, r2
    T = 3
    ddpm = model(T)
    out = ddpm.sample(cond_of(295), 1.0, seed=7, profile=True)
    assert torch.isfinite(out).all()
    down0 = [r for r in ddpm.op_profile() if r[0] == "down.0.res"]
    assert len(down0) == 1 and down0[0][3] > 0.0, down0


def test_fallbacks_are_unchanged():
    """A single-pass forward (one pass: nothing to share) and the exact-float32 path (no panel kernels) do not take the form: same
    bits with the switch on and off."""
    ddpm = model(3)
    B = 295
    g = torch.Generator().manual_seed(9)
    x, cond = torch.randn(B, 80, generator=g).cuda(), torch.rand(B, 80, generator=g).cuda()
    t = (torch.randint(1, 4, (1, B), generator=g).float() / 3.0).cuda()
    mask = (torch.rand(B, 1, generator=g) < 0.7).float().cuda()
    outs = {}
    for val in (0, 1):
        ddpm.model.set_option("cfg_share", val)
        outs[val] = ddpm.model(x, t, cond, mask)
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
    ddpm.model.set_precision("f32")
    for val in (0, 1):
        ddpm.model.set_option("cfg_share", val)
        outs[val] = ddpm.sample(cond, 1.0, seed=7)
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
