"""CPU self-check of the range-guard scenarios (tests/envelope_ref.py): completeness of the raw-read list against the plan, and isolation
of every scenario -- at A_OUT only the targeted tensor's reads are above kRawLimit, at A_IN none is, every other raw read stays below
3e4 and eps stays of order 1.  This is what lets tests/test_gpu_envelope.py conclude "flag up => a kernel that reads THIS tensor raised it".

Which launches read a tensor (msr80: proj 128, dims 64/32/16/8, two blocks per resolution; the other configs follow the same rule):

  y ............................. feature_proj: k_linear_h<IN_ROWMAJOR> (the open-coded max|x| compare), every form
  feature_proj, down.0, down.1 .. skip halves of up.18 / up.17 / up.16 (128-wide blocks with a Linear shortcut): k_unet_tile (tile),
                                  k_resblock_c<128,true> (coop), k_panel128_h<true,..> (large), k_wide128_h<true,..> (per-row t), the
                                  training forward; down.1 ALSO feeds down.2.lin (128 -> 64), fused behind down.1 in the large forms
                                  (the EPI = 1 site of dsg_panel.hpp / dsg_wide.hpp) -- two reads, covered JOINTLY, not apart
  down.2 .. down.4 .............. skip halves of the 64-wide up blocks: k_res64_lds<true,..> / k_res64_dual (large), k_resblock_c<64,true>,
                                  k_resblock_h<64,true> and the k_resblock_lin_h pairs; down.4 also feeds down.5.lin (the EPI site of
                                  dsg_res64.hpp), again jointly
  down.5 .. down.10 ............. 32- and 16-wide: the narrow run (k_fused_narrow_h / k_fused_narrow_lds: linear_reg_h,
                                  linear_reg_out_h, linear_pre_to_reg_h and the block bodies' Chan-merged shortcut check), k_unet_tile
  down.11 .. up.2, middle ....... 8-wide: read only inside the float32 vector section when narrow_valu8 is on (no flag by design), by the
                                  narrow run's matrix-core forms when it is off
  up.3 .. up.17 ................. running halves of the up blocks' shortcuts and the inputs of the Upsample Linears, by width as above
"""
import pytest
import torch

import envelope_ref as E
from oracle import ddpm_oracle as O
from weights import CONFIGS

CFGS = ["msr80", "co3", "nu3"]
B = 33


def _inputs(name):
    cfg = CONFIGS[name]
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, cfg["input_dim"], generator=g)
    cond = torch.rand(B, cfg["cond_dim"], generator=g)
    t = torch.full((1, B), 2.0 / 3.0)
    return x, t, cond


@pytest.mark.parametrize("name", CFGS)
def test_raw_read_list_is_complete_for_the_plan(name):
    """Every Linear of the plan that is not behind a LayerNorm reads raw: feature_proj, every Down/Upsample, every shortcut -- and each
    column of such a weight belongs to exactly one listed tensor."""
    cfg = CONFIGS[name]
    plan = O.unet_plan(cfg["input_dim"], cfg["proj_dim"], cfg["cond_dim"], cfg["dims"], cfg["n_blocks"])
    shapes = O.state_shapes(plan)
    want = {k[:-len(".weight")] for k in shapes if k.endswith((".shortcut.weight", ".lin.weight"))} | {"feature_proj"}
    reads = E.raw_reads(plan)
    assert {r.site for r in reads} == want and len(reads) == len(want)
    tensors = E.raw_tensors(plan)
    for r in reads:
        cols = shapes[r.site + ".weight"][1]
        covered = []
        for n, c0 in zip(r.tensors, r.col0):
            covered += list(range(c0, c0 + tensors[n].width))
        assert covered == list(range(cols)), r
    # every module output but the last one (it goes to the final LayerNorm) is read raw somewhere, and so is y
    taps = {}
    x, t, cond = _inputs(name)
    _, base, _ = E.scenarios(name, 3, E.A_IN, only=set())
    O.unet_forward(base, plan, x, t, cond, torch.ones(B, 1), taps=taps)
    last = f"up.{len(plan['up']) - 1}"
    assert set(tensors) == (set(taps) - {"time_emb", last}) | {"y"}
    # carried tensors are exactly those followed by an identity-shortcut block; their cancelling bias exists
    for tn in tensors.values():
        assert tn.carry is None or tn.carry in shapes
        assert tn.bias is None or tn.bias in shapes


@pytest.mark.parametrize("name", CFGS)
@pytest.mark.parametrize("A", [E.A_IN, E.A_OUT])
def test_every_scenario_is_isolated(name, A):
    plan, base, scns = E.scenarios(name, 3, A)
    assert [s.tensor for s in scns] == list(E.raw_tensors(plan))
    x, t, cond = _inputs(name)
    for s in scns:
        xs = E.apply_y(s, x)
        for m in (0.0, 1.0):
            taps = {}
            with torch.no_grad():
                eps = O.unet_forward({k: v.double() for k, v in s.params.items()}, plan, xs.double(), t.double(), cond.double(),
                                     torch.full((B, 1), m, dtype=torch.float64), taps=taps)
            bounds = E.raw_bounds(plan, taps, xs)
            for site, (bound, mx) in bounds.items():
                if site in s.sites:
                    if A == E.A_OUT:
                        assert mx > E.F16_MAX and bound > E.RAW_LIMIT, (s.name, site, bound, mx)
                    else:
                        assert mx > 0.9 * A and bound < E.RAW_LIMIT, (s.name, site, bound, mx)
                else:
                    assert bound < E.QUIET, (s.name, site, bound, mx)
            assert float(eps.abs().max()) < 100.0, (s.name, float(eps.abs().max()))
        if s.y_col is None and A == E.A_OUT:
            # "feature j is A in EVERY row": each row tile of a launch sees the outlier, not only the one that holds the worst row
            assert float(taps[s.tensor][:, s.j].min()) > E.F16_MAX, s.name


# The float32 section as csrc/dsg_narrow8.hpp describes it (its head comment and V8SecL: "Downsample 16 -> 8, n_blocks DownBlocks, the two
# MiddleBlocks, n_blocks + 1 UpBlocks 16 -> 8, Upsample 8 -> 16", NOPS = 2 * NB + 5 operators), written out by hand per config from the
# module list of UNetCF.py -- NOT through the rule `v8_section` uses: the tensors the section's operators read, less the Downsample's own
# 16-wide input (an up block outside the section reads that one too).
V8_BY_HAND = {
    "msr80": {"down.11", "down.12", "down.13", "middle", "up.0", "up.1", "up.2"},                       # 2 blocks, 4 resolutions
    "co3": {"down.15", "down.16", "down.17", "down.18", "middle", "up.0", "up.1", "up.2", "up.3"},       # 3 blocks, 4 resolutions
    "nu3": {"down.8", "down.9", "down.10", "middle", "up.0", "up.1", "up.2"},                            # 2 blocks, 3 resolutions
}


@pytest.mark.parametrize("name", CFGS)
def test_v8_section_is_the_one_the_kernel_header_describes(name):
    """The GPU test lets the flag stay down for these tensors under narrow_valu8 = 1, so the set must be the section's real extent."""
    import os
    import re
    from _util import ROOT
    cfg = CONFIGS[name]
    plan = O.unet_plan(cfg["input_dim"], cfg["proj_dim"], cfg["cond_dim"], cfg["dims"], cfg["n_blocks"])
    v8 = E.v8_section(plan)
    assert v8 == V8_BY_HAND[name]
    # the operator count the header states: every operator of the section but the first reads one of these tensors, and middle.res2 reads
    # middle.res1's output, which is no raw-read tensor
    src = open(os.path.join(ROOT, "diffsg_amd", "csrc", "dsg_narrow8.hpp")).read()
    m = re.search(r"NOPS\s*=\s*(\d+)\s*\*\s*NB\s*\+\s*(\d+)", src)
    assert m, "dsg_narrow8.hpp no longer states the section's operator count"
    nops = int(m.group(1)) * cfg["n_blocks"] + int(m.group(2))
    assert len(v8) == nops - 2
    tensors = E.raw_tensors(plan)
    for n in v8:                      # read by nothing outside the section: every read of them is an 8-wide operator's or the Upsample's
        for site, _ in tensors[n].reads:
            w = O.state_shapes(plan)[site + ".weight"]
            assert min(w) == 8, (n, site, w)
