"""CPU self-check of the range-guard scenarios (tests/envelope_ref.py): completeness of the raw-read list against the plan, and isolation
of every scenario -- at A_OUT only the targeted tensor's reads are above kRawLimit, at A_IN none is, every other raw read stays below
3e4 and eps stays of order 1.  This is what lets tests/test_gpu_envelope.py conclude "flag up => a kernel that reads THIS tensor raised it".
The second half does the same for the low side (whole stream segments at a small amplitude) and proves where the kernels' floors may sit:
what the accuracy contract asks for per tests/split_ref.py, and how far under it the shipped workloads push them.

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
import re

import numpy as np
import pytest
import torch

import envelope_ref as E
import split_ref as S
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


# ------------------------------------------------------------------------------------------------ the low side
# What tests/test_gpu_envelope.py relies on for its small-row cases, proved on the oracle's taps for the very rows it runs (B = 33, T = 3, all
# three kinds of call, every denoiser pass of each) plus a PADDING row -- y = 0, cond = 0: what the ragged last tile of a launch computes
# in its unused rows, which the kernels bound like any other.
T_GPU = 3
KINDS = ("sample", "forward", "train")
# Measured here, in units of s (float64; the asserts below hold them): a whole targeted row's |mean| + sqrt(M2) and a y row's max|y|.
BOUND_OVER_S, Y_OVER_S = E.BOUND_OVER_S, E.Y_OVER_S               # (1.2, 26.0) and (0.2, 3.9)
# every row of a targeted tensor has max|x| within [s / SPREAD, SPREAD * s] (the padding row and rows of the 3-wide y are the small ones)
SPREAD = 32.0
# the oracle's own float32-vs-float64 error on the low scenarios, all three configs, seed 3, every amplitude used: at most 1.9e-6 (forward)
BUDGET_CAP = 1e-5


def _floor(site):
    return E.RAW_FLOOR_IN if site == "feature_proj" else E.RAW_FLOOR


def _passes(name, scn, kind):
    d = E.data(name, B, T_GPU)
    calls = E.call_inputs(scn, d, T_GPU, kind)
    if scn.segment == "y" and kind == "sample":
        calls = calls[:2]                # the reverse loop renormalises y: only the first step reads the small start state
    pad = lambda a: torch.cat([a, torch.zeros(1, a.shape[1])])       # noqa: E731
    return [(pad(x), torch.cat([t, t[:, -1:]], dim=1), pad(c), torch.cat([m, m[-1:]])) for x, t, c, m in calls]


@pytest.mark.parametrize("name", CFGS)
def test_every_raw_read_is_targeted_by_a_low_scenario(name):
    plan, _, scns = E.low_scenarios(name, 3, E.S_IN)
    reads = E.raw_reads(plan)
    assert {st for s in scns for st in s.sites} == {r.site for r in reads}
    # every tensor belongs to exactly one segment, and every Down/Upsample Linear, feature_proj and the first up block's shortcut see a
    # WHOLE small row in some scenario: the sites at which the floor can be asserted
    owned = [t for s in scns for t in s.tensors]
    assert sorted(owned) == sorted(E.raw_tensors(plan))
    whole = {st for s in scns for st in s.whole}
    assert whole == {r.site for r in reads if r.site.endswith(".lin")} | {"feature_proj", "up.0.res.shortcut"}
    for s in scns:
        assert not s.v8_only or all(E.site_in_v8(plan, st) for st in s.whole), s.name


@pytest.mark.parametrize("name", CFGS)
@pytest.mark.parametrize("amp", [E.S_IN, E.S_OUT] + list(E.LOW_CURVE))
def test_low_scenarios_are_small_where_they_should_be_and_nowhere_else(name, amp):
    plan, _, scns = E.low_scenarios(name, 3, amp)
    seen = {"bound": [1e30, 0.0], "y": [1e30, 0.0], "rows": [1e30, 0.0]}
    for s in scns:
        for kind in KINDS:
            if s.segment == "y" and kind == "sample" and amp != E.S_IN:
                continue                 # not run (see _passes): beyond the first step feature_proj's output would be 1 / s times too large
            for x, t, cond, mask in _passes(name, s, kind):
                taps = {}
                with torch.no_grad():
                    eps = O.unet_forward(s.params, plan, x, t, cond, mask, taps=taps)
                assert float(eps.abs().max()) < 100.0
                for tn in s.tensors:     # every row of every tensor of the segment is of size s
                    mx = (x if tn == "y" else taps[tn]).abs().amax(dim=1)
                    mx = mx[mx > 0]
                    seen["rows"] = [min(seen["rows"][0], float(mx.min()) / amp), max(seen["rows"][1], float(mx.max()) / amp)]
                    assert float(mx.min()) >= amp / SPREAD and float(mx.max()) <= SPREAD * amp, (s.name, kind, tn, float(mx.min()) / amp, float(mx.max()) / amp)
                lo = E.raw_bounds_min(plan, taps, x)
                for r in E.raw_reads(plan):
                    bmin, bmax = lo[r.site]
                    if r.site in s.whole:
                        k = seen["y" if r.site == "feature_proj" else "bound"]
                        k[0], k[1] = min(k[0], bmin / amp), max(k[1], bmax / amp)
                        if amp == E.S_OUT:
                            assert bmax < 0.5 * _floor(r.site), (s.name, kind, r.site, bmax)
                        want = E.flag_at(s.segment, amp, True)       # the GPU tests assert the flag wherever this rule decides it
                        assert want is not True or bmax < 0.9 * _floor(r.site), (s.name, kind, r.site, bmax)
                    if r.site not in s.whole or E.flag_at(s.segment, amp, True) is False:
                        assert bmin > 2.0 * _floor(r.site), (s.name, kind, r.site, bmin)          # never a false report
                    assert lo[r.site][1] < E.QUIET                                                # ... from either side
                    if r.site not in s.sites:
                        rows = torch.cat([(x if n == "y" else taps[n]) for n in r.tensors], dim=1).abs().amax(dim=1)
                        assert float(rows[rows > 0].min()) >= 2.0 ** -4, (s.name, kind, r.site)
    print(f"{name} @ {amp:g}: whole-row bound / s in [{seen['bound'][0]:.2f}, {seen['bound'][1]:.1f}], max|y| / s in [{seen['y'][0]:.2f}, {seen['y'][1]:.2f}], row max|x| / s in [{seen['rows'][0]:.2f}, {seen['rows'][1]:.1f}]")
    assert BOUND_OVER_S[0] <= seen["bound"][0] and seen["bound"][1] <= BOUND_OVER_S[1]
    assert Y_OVER_S[0] <= seen["y"][0] and seen["y"][1] <= Y_OVER_S[1]


@pytest.mark.parametrize("name", CFGS)
def test_low_scenarios_keep_the_oracle_within_its_budget_cap(name):
    """rel(float32 oracle, float64 oracle) of the forward pass under every low scenario and amplitude the GPU tests use."""
    d = E.data(name, B, T_GPU)
    worst = 0.0
    for amp in E.LOW_CURVE + (E.S_IN, E.S_OUT):
        plan, _, scns = E.low_scenarios(name, 3, amp)
        for s in scns:
            x = E.apply_y(s, d["y_T"])
            r64 = E.oracle_forward(s.params, plan, x, d["t"], d["cond"], d["mask"], True)
            worst = max(worst, E.rel(E.oracle_forward(s.params, plan, x, d["t"], d["cond"], d["mask"], False), r64))
    print(f"{name}: largest oracle budget over the low scenarios {worst:.2e}")
    assert worst <= BUDGET_CAP


def test_the_amplitudes_follow_from_the_floors_and_the_measured_bounds():
    """S_IN is the smallest power of two at which no row can be under its floor, S_OUT the largest at which every whole row must be."""
    lo = min(BOUND_OVER_S[0] / E.RAW_FLOOR, Y_OVER_S[0] / E.RAW_FLOOR_IN)       # a row is safe when s * lo > 2 (the margin asserted above)
    hi = max(BOUND_OVER_S[1] / E.RAW_FLOOR, Y_OVER_S[1] / E.RAW_FLOOR_IN)
    assert E.S_IN * lo > 2.0 and E.S_IN / 2 * lo <= 2.0
    assert E.S_OUT * hi < 0.5 and E.S_OUT * 2 * hi >= 0.5
    # the flag's state at S_IN, S_OUT and the curve's points, per kind of segment (envelope_ref.flag_at)
    assert [E.flag_at("down.2", a, True) for a in (E.S_IN, E.S_OUT) + E.LOW_CURVE] == [False, True, False, None, True]
    assert [E.flag_at("y", a, True) for a in (E.S_IN, E.S_OUT) + E.LOW_CURVE] == [False, True, False, False, None]
    assert E.flag_at("down.2", E.S_OUT, False) is None


def test_the_kernels_floors_are_the_ones_the_scenarios_assume():
    import os
    from _util import ROOT
    src = open(os.path.join(ROOT, "diffsg_amd", "csrc", "dsg_split.hpp")).read()
    for cname, want in (("kRawFloor", E.RAW_FLOOR), ("kRawFloorIn", E.RAW_FLOOR_IN)):
        m = re.search(r"constexpr float " + cname + r"\s*=\s*([0-9.eE+-]+)f\s*/\s*kRawScale;", src)
        assert m, cname
        assert float(m.group(1)) == want, (cname, m.group(1), want)


# ------------------------------------------------------------------------------------------------ where the floors come from
def _floor_from_split_ref(name):
    """The floor the accuracy contract alone asks for, in the kernels' quantity: the smallest power of two above the bound of every whole read
    whose split_ref prediction (its own rows, its own weight columns) exceeds TOL / 2 -- over the low scenarios at s = 2^-4 ... 2^-12."""
    TOL = 1e-5
    d = E.data(name, B, T_GPU)
    worst = {"bound": 0.0, "y": 0.0}
    for k in range(4, 13):
        amp = 2.0 ** -k
        plan, _, scns = E.low_scenarios(name, 3, amp)
        raw = E.raw_tensors(plan)
        for s in scns:
            if not s.whole:
                continue
            x = E.apply_y(s, d["y_T"])
            taps = {}
            with torch.no_grad():
                O.unet_forward(s.params, plan, x, d["t"], d["cond"], d["mask"], taps=taps)
            lo = E.raw_bounds_min(plan, taps, x)
            for r in E.raw_reads(plan):
                if r.site in s.whole:
                    rows = torch.cat([(x if n == "y" else taps[n]) for n in r.tensors], dim=1).numpy()
                    pred = S.predicted_rel(rows, s.params[r.site + ".weight"].numpy())
                    if pred > TOL / 2:
                        key = "y" if r.site == "feature_proj" else "bound"
                        worst[key] = max(worst[key], lo[r.site][0])
    return {k: 2.0 ** np.floor(np.log2(v) + 1) for k, v in worst.items()}


def test_the_floor_the_accuracy_contract_alone_would_ask_for():
    """... is 2^-5 on the row bound and 2^-8 on max|y| (rows of rms 2^-8 to 2^-9, as the error-versus-amplitude table says).  The shipped
    workloads do not leave room for it (next test): the floors in the kernels are lower, and this is what that costs per split_ref --
    a Linear over rows AT the floor is predicted 2e-5 (8-wide) to 1.2e-4 (128-wide) off, over 80-wide rows of y at its floor 7e-4."""
    got = {n: _floor_from_split_ref(n) for n in CFGS}
    print(got)
    assert max(g["bound"] for g in got.values()) == 2.0 ** -5
    assert max(g["y"] for g in got.values()) == 2.0 ** -8
    assert E.RAW_FLOOR < 2.0 ** -5 and E.RAW_FLOOR_IN < 2.0 ** -8
    # the cost: rows of rms r -> bound about sqrt(N) r
    for n_in, lo, hi in ((8, 1e-5, 4e-5), (128, 6e-5, 2.4e-4)):
        rng = np.random.default_rng(n_in)
        x = (rng.standard_normal((70, n_in)) * E.RAW_FLOOR / np.sqrt(n_in)).astype(np.float32)
        W = (rng.uniform(-1, 1, (64, n_in)) / np.sqrt(n_in)).astype(np.float32)
        pred = S.predicted_rel(x, W)
        print(f"rows of {n_in} at the floor: predicted {pred:.1e}")
        assert lo <= pred <= hi, (n_in, pred)
    rng = np.random.default_rng(80)
    y = rng.standard_normal((70, 80))
    y = (y / np.abs(y).max(axis=1, keepdims=True) * E.RAW_FLOOR_IN).astype(np.float32)          # every row's max|y| AT the floor
    pred = S.predicted_rel(y, (rng.uniform(-1, 1, (128, 80)) / np.sqrt(80)).astype(np.float32))
    print(f"rows of y at the input floor: predicted {pred:.1e}")
    assert 3e-4 <= pred <= 1.5e-3, pred


MARGIN = 8.0


def test_no_shipped_workload_comes_near_the_floor():
    """The guard must never fire on what the project ships: the smallest row bound of every raw read (all-zero rows apart, which raise
    nothing) over the five catalogue nets in both flavours (a sampling call, and a T = 1000 training batch with all-zero y rows at ts = 0,
    where x_t = sqrt(1 - acp_0) * noise = 6.4e-3 * noise), the 13 descriptor-space nets, the NU checkpoint on its 512 rows at omega 1 and 500,
    and the benchmark's init-flavour MSR-80c inputs stays a factor 8 above the floors -- every pass with the padding row of a ragged last
    tile (y = 0, cond = 0), which the kernels bound too: 0.074 at its smallest (the NU checkpoint).  Measured: row bound >= 0.023 (the NU checkpoint's
    last Upsample input; everything synthetic >= 0.44), max|y| >= 1.2e-3 (CO-3n, a zero row at ts = 0; sampling >= 0.037).
    The input floor is NOT the largest power of two with that margin: the largest of three normal draws has no lower bound, so a longer
    survey finds smaller rows.  kRawFloorIn = 2^-14 is set by the chance of such a row (csrc/dsg_split.hpp) and merely checked here."""
    import shape_ref as SR
    from _util import GOLD, synth_params
    import os
    acc = {}

    def take(bounds, what):
        for site, (lo, _) in bounds.items():
            key = "y" if site == "feature_proj" else "bound"
            if lo < acc.get(key, (1e30, ""))[0]:
                acc[key] = (lo, f"{what}: {site}")

    g = torch.Generator().manual_seed(0)
    for name in CONFIGS:
        cfg = CONFIGS[name]
        for fl in ("trained", "init"):
            plan, p = synth_params(name, 3, fl)
            Bs, Ts = 64, 4
            cond, y_T = torch.rand(Bs, cfg["cond_dim"], generator=g), torch.randn(Bs, cfg["input_dim"], generator=g)
            z = torch.randn(Ts, Bs, cfg["input_dim"], generator=g)
            take(E.survey_sample(p, plan, Ts, cond, 1.0, y_T, z), f"{name}/{fl}/sample")
            y = torch.rand(Bs, cfg["input_dim"], generator=g)
            y[:16] = 0.0
            ts = torch.randint(0, 1000, (1, Bs), generator=g)
            ts[0, :32] = 0
            take(E.survey_train(p, plan, 1000, y, cond, ts, torch.randn(Bs, cfg["input_dim"], generator=g), torch.ones(Bs, 1)), f"{name}/{fl}/train")
    for name in SR.NAMES:
        plan, p = SR.net(name)
        cond, y_T, z = SR.sample_inputs(name)
        take(E.survey_sample(p, plan, SR.T, cond, 2.0, y_T, z), f"{name}/sample")
    gd = np.load(os.path.join(GOLD, "g4_sample_nu_ckpt.npz"))
    p = {k[2:]: torch.from_numpy(gd[k]) for k in gd.files if k.startswith("w.")}
    cfg = CONFIGS["nu3"]
    plan = O.unet_plan(cfg["input_dim"], cfg["proj_dim"], cfg["cond_dim"], cfg["dims"], cfg["n_blocks"])
    for om in (1.0, 500.0):
        take(E.survey_sample(p, plan, int(gd["T"]), torch.from_numpy(gd["cond"]), om, torch.from_numpy(gd["y_T"]), torch.from_numpy(gd["z"])), f"NU checkpoint/omega {om:g}")
    plan, p = synth_params("msr80", 0, "init")                                    # bench.py: init flavour, seed 0, cond ~ U[0, 1), y ~ N(0, 1)
    g = torch.Generator().manual_seed(0)
    cond, y_T, z = torch.rand(512, 80, generator=g), torch.randn(512, 80, generator=g), torch.randn(6, 512, 80, generator=g)
    take(E.survey_sample(p, plan, 6, cond, 1.0, y_T, z), "benchmark inputs")
    print(acc)
    assert acc["bound"][0] >= MARGIN * E.RAW_FLOOR, acc["bound"]
    assert acc["y"][0] >= MARGIN * E.RAW_FLOOR_IN, acc["y"]
    # and the floors are the largest powers of two with that margin
    assert acc["bound"][0] < MARGIN * 2 * E.RAW_FLOOR
    sigma0 = float(O.schedule_buffers(1.0 - O.cosine_betas(1000))["sqrt_one_minus_alphas_cumprod"][0])
    assert (0.8 * E.RAW_FLOOR_IN / sigma0) ** 3 < 1e-6, sigma0        # P(max of 3 |N(0, sigma0)| < floor) <= (sqrt(2 / pi) floor / sigma0)^3
