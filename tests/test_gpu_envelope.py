"""The fp16 range guard of the split-f16 path at every raw operand of every kernel form, the condition operand and the weight-side envelope.

Scenarios come from tests/envelope_ref.py (one raw-read tensor at amplitude A, everything else of order 1; tests/test_envelope_cpu.py
proves the isolation and lists which launches read which tensor), so "the flag came up" can only be the work of a kernel that reads the
targeted tensor.  A form is a way of reaching other kernels (csrc/host_dispatch.hpp is the map):

  tile      sample, default policy ................ k_linear_h, k_unet_tile
  coop      sample, tile_step off ................. k_resblock_c, stand-alone k_linear_h<IN_FRAG>, k_fused_narrow_h<true,*>
  large     sample, policy (0, 0) ................. k_panel128_h<..,2>, k_panel128_duo_h<2>, k_res64_lds, k_res64_dual, k_fused_narrow_lds
  full      large + panel_half off ................ k_panel128_h<..,4>, k_panel128_duo_h<4>
  rowt      model(x, t, cond, mask), policy (0, 0)  k_wide128_h, k_resblock_h<64,*>, k_resblock_lin_h pairs, k_fused_narrow_h<false,*>
  forward   model(x, t, cond, mask) ............... the small-launch forward
  onepass   sample, guidance 0 at every step ...... the second resident table set
  train     ddpm(y, cond, ts=, noise=, cond_mask=)  the training forward (the forms that save h1 / h2)

Per scenario and form:
  A_OUT = 7e4, split mode, enqueue-only call: `range_exceeded()` is True and a second query False.  Strict, except for a tensor read only
      inside the float32 vector section (the 8-wide tensors under narrow_valu8 = 1, envelope_ref.v8_section): there the flag may stay
      down, and then a non-cancel scenario must meet the accuracy bound below (a cancel scenario carries no accuracy claim: finite only).
  A_IN = 5e4, split mode: the flag stays down and, for non-cancel scenarios, rel(result, float64 oracle) <= TOL + 3 x the oracle's own
      float32-vs-float64 error (the rule of test_sample_large_launch_vs_oracle; the budget never comes from the code under test).
  A_OUT under set_precision("f32"), every scenario and form: the flag stays down and non-cancel results are within the same bound of the
      float64 oracle (the training form: the loss) -- the exact kernels are where every flagged call is sent.
  A_OUT, plain sample(), for the scenarios of PLAIN (one per kernel family): it warns, returns bit for bit what an f32-mode call returns
      and leaves the precision mode alone.
  The narrow-run scenarios (tensors at most 32 wide) run under narrow_valu8 1 and 0.
  Training: the flag at A_OUT; flag down and the loss within 1e-5 of the float64 oracle's at A_IN.  Gradients under these weights are out
      of scope (a cancel scenario's lin3 bias pair makes them ill-conditioned by construction).

Tensors with two raw reads (a skip tensor that also feeds a Downsample: down.1 -> down.2.lin and up.16's shortcut) are covered jointly.
Every launch here is a valid launch on finite data.  A case's time is mostly the CPU oracle's (float32 and float64, two amplitudes, one
reverse loop per scenario): each reference is computed once and shared by the forms that use it, so the first case of a config and call
kind pays for the others.
"""
import functools
import warnings

import pytest
import torch

import envelope_ref as E
from oracle import ddpm_oracle as O
from test_gpu_parity import TOL, make_ddpm, rel
from weights import CONFIGS

pytestmark = pytest.mark.gpu

T, OMEGA, SEED = 3, 1.0, 3
# one tensor per kernel family for the plain-sample / f32 checks: y (feature_proj), a 128-wide skip, a 64-wide skip that also feeds a
# Downsample, a narrow-run tensor, the running half of a 64-wide up block
PLAIN = {"msr80": ("y", "down.1", "down.4", "down.7", "up.13"), "co3": ("y", "down.2", "down.9"), "nu3": ("y", "down.1", "up.5")}

FORMS = {
    # name: (kind, launch policy or None, options, one-pass plan)
    "tile": ("sample", None, {}, False),
    "coop": ("sample", None, {"tile_step": 0}, False),
    "large": ("sample", (0, 0), {}, False),
    "full": ("sample", (0, 0), {"panel_half": 0}, False),
    "rowt": ("forward", (0, 0), {}, False),
    "forward": ("forward", None, {}, False),
    "onepass": ("sample", None, {}, True),
    "train": ("train", None, {}, False),
}
# every form on every config at B = 33 (two row tiles per pass, one ragged); the large-launch forms also at 289 rows on msr80, the one config
# with 128-wide blocks (10 tiles per pass: the pass boundary and the last group fall inside a workgroup's group of 8 or 4 tiles)
CASES = [(n, f, 33) for n in ("msr80", "co3", "nu3") for f in FORMS] + [("msr80", f, 289) for f in ("large", "full", "rowt")]


@functools.lru_cache(maxsize=None)
def _data(name, B):
    cfg = CONFIGS[name]
    D, C = cfg["input_dim"], cfg["cond_dim"]
    g = torch.Generator().manual_seed(100 + B)
    d = dict(cond=torch.rand(B, C, generator=g), y_T=torch.randn(B, D, generator=g), z=torch.randn(T - 2, B, D, generator=g),
             t=torch.rand(1, B, generator=g), mask=(torch.rand(B, 1, generator=g) < 0.7).float(),
             y=torch.rand(B, D, generator=g), ts=torch.randint(0, T, (1, B), generator=g), noise=torch.randn(B, D, generator=g))
    d["mask"][-1] = 1.0
    return d


@functools.lru_cache(maxsize=None)
def _scenario(name, tensor, A):
    plan, _, (s,) = E.scenarios(name, SEED, A, only={tensor})
    return plan, s


def _train_y(s, d):
    """The training form's `y`: q_sample scales it by sqrt(acp[ts]) before feature_proj reads it, so the `y` scenario sets A / that."""
    if s.y_col is None:
        return d["y"]
    bufs = O.schedule_buffers(1.0 - O.cosine_betas(T))
    y = d["y"].clone()
    y[-1, s.y_col] = s.A / float(bufs["sqrt_alphas_cumprod"][int(d["ts"][0, -1])])
    return y


@functools.lru_cache(maxsize=None)
def _oracle(name, tensor, A, B, kind, omega):
    """(float64 reference, the oracle's float32-vs-float64 relative error) of one scenario under one kind of call; shared by the forms."""
    plan, s = _scenario(name, tensor, A)
    d = _data(name, B)
    if kind == "sample":
        return E.in_range_budget(s.params, plan, T, d["cond"], omega, E.apply_y(s, d["y_T"]), d["z"])
    if kind == "forward":
        x = E.apply_y(s, d["y_T"])
        r64 = E.oracle_forward(s.params, plan, x, d["t"], d["cond"], d["mask"], True)
        return r64, rel(E.oracle_forward(s.params, plan, x, d["t"], d["cond"], d["mask"], False), r64)
    return E.oracle_loss64(s.params, plan, T, _train_y(s, d), d["cond"], d["ts"], d["noise"], d["mask"]), 0.0


class _Runner:
    """One model in one form; scenarios are loaded into it (load_state_dict re-binds the weights)."""

    def __init__(self, name, form, B):
        self.name, self.form, self.B = name, form, B
        self.kind, policy, options, onepass = FORMS[form]
        _, base = E.scenarios(name, SEED, E.A_IN, only=set())[:2]
        self.ddpm = make_ddpm(name, base, T)
        self.model = self.ddpm.model
        if policy is not None:
            self.model.set_launch_policy(*policy)
        for k, v in options.items():
            self.model.set_option(k, v)
        self.plan = None
        self.omega = OMEGA
        if onepass:
            from diffsg_amd import steps
            self.plan = steps.with_guidance(self.ddpm, torch.zeros(T))
        self.d = {k: (v.cuda() if k != "z" and k != "y_T" else v) for k, v in _data(name, B).items()}

    @property
    def oracle_omega(self):
        return 0.0 if self.plan is not None else OMEGA      # guidance 0 at every step: eps = the conditional pass alone

    def load(self, s):
        self.model.load_state_dict(s.params, strict=True)

    def run(self, s, check_range=False):
        """One enqueue-only call of the form on scenario `s` (its parameters are loaded); returns the result tensor / the loss."""
        d = self.d
        if self.kind == "sample":
            out = self.ddpm.sample(d["cond"], self.omega, y_T=E.apply_y(s, d["y_T"]), noise=d["z"], check_range=check_range, plan=self.plan)
            self.ddpm._range_unchecked = False          # this test reads the flag itself
            return out
        if self.kind == "forward":
            return self.model(E.apply_y(s, d["y_T"]).cuda(), d["t"], d["cond"], d["mask"])
        with torch.no_grad():
            return self.ddpm(_train_y(s, _data(self.name, self.B)).cuda(), d["cond"], ts=d["ts"], noise=d["noise"], cond_mask=d["mask"])

    def err(self, s, out):
        """(error of `out` against the float64 oracle, its bound) for scenario `s`."""
        ref, budget = _oracle(self.name, s.tensor, s.A, self.B, self.kind, self.oracle_omega)
        if self.kind == "train":
            return abs(float(out) - float(ref)) / abs(float(ref)), 1e-5
        return rel(out, ref), TOL + 3.0 * budget


def _tensors(name):
    cfg = CONFIGS[name]
    plan = O.unet_plan(cfg["input_dim"], cfg["proj_dim"], cfg["cond_dim"], cfg["dims"], cfg["n_blocks"])
    return plan, E.raw_tensors(plan)


@pytest.mark.parametrize("name,form,B", CASES)
def test_range_guard_at_every_raw_operand(name, form, B):
    plan, tensors = _tensors(name)
    r = _Runner(name, form, B)
    bad, worst = [], (0.0, 0.0, "")
    for v8 in (1, 0):
        r.model.set_option("narrow_valu8", v8)
        for tn in tensors.values():
            if v8 == 0 and not (tn.name != "y" and tn.width <= 32):
                continue                                   # the second setting re-runs the narrow run's scenarios only
            tag = f"{name}/{form}/B={B}/v8={v8}/{tn.name}"
            # ---- A_OUT: the flag
            _, s = _scenario(name, tn.name, E.A_OUT)
            r.load(s)
            out = r.run(s)
            up, again = r.model.range_exceeded(), r.model.range_exceeded()
            if again:
                bad.append(f"{tag}: the query did not clear the flag")
            if not up:
                if not (s.v8_only and v8 == 1):
                    bad.append(f"{tag}: flag DOWN at A_OUT (sites {s.sites})")
                elif s.cancel:
                    if not bool(torch.isfinite(out).all()):
                        bad.append(f"{tag}: float32 section, not finite")
                else:
                    e, bound = r.err(s, out)
                    print(f"{tag}: float32 section, flag down at A_OUT, err {e:.2e} (bound {bound:.2e})")
                    if not e <= bound:
                        bad.append(f"{tag}: float32 section, flag down and err {e:.2e} > {bound:.2e}")
            # ---- A_IN: flag down, accuracy
            _, s = _scenario(name, tn.name, E.A_IN)
            r.load(s)
            out = r.run(s)
            if r.model.range_exceeded():
                bad.append(f"{tag}: flag UP at A_IN")
            if not s.cancel:
                e, bound = r.err(s, out)
                if e > worst[0]:
                    worst = (e, bound, tag)
                if not e <= bound:
                    bad.append(f"{tag}: A_IN err {e:.2e} > bound {bound:.2e}")
    # ---- A_OUT on the exact kernels, where every flagged call is sent: nothing to flag, and right (narrow_valu8 is a split-path option)
    r.model.set_precision("f32")
    worst32 = (0.0, 0.0, "")
    for tn in tensors.values():
        tag = f"{name}/{form}/B={B}/f32/{tn.name}"
        _, s = _scenario(name, tn.name, E.A_OUT)
        r.load(s)
        out = r.run(s)
        if r.model.range_status() != 0:
            bad.append(f"{tag}: flag UP in f32 mode")
        if s.cancel:
            if not bool(torch.isfinite(out).all()):
                bad.append(f"{tag}: not finite")
        else:
            e, bound = r.err(s, out)
            if e > worst32[0]:
                worst32 = (e, bound, tag)
            if not e <= bound:
                bad.append(f"{tag}: f32 mode at A_OUT err {e:.2e} > bound {bound:.2e}")
    r.model.set_precision("split_f16")
    print(f"{name}/{form}/B={B}: largest f32-mode A_OUT error {worst32[0]:.2e}, its bound {worst32[1]:.2e} ({worst32[2]})")
    print(f"{name}/{form}/B={B}: largest A_IN error {worst[0]:.2e}, its bound {worst[1]:.2e} ({worst[2]})")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name,form", [("msr80", f) for f in ("tile", "coop", "large", "full", "onepass")] + [("co3", "large"), ("nu3", "tile")])
def test_plain_sample_falls_back_to_the_exact_kernels(name, form):
    B = 33
    r = _Runner(name, form, B)
    d = r.d
    bad = []
    for tensor in PLAIN[name]:
        tag = f"{name}/{form}/{tensor}"
        _, s = _scenario(name, tensor, E.A_OUT)
        r.load(s)
        y_T = E.apply_y(s, d["y_T"])
        with pytest.warns(UserWarning):
            got = r.ddpm.sample(d["cond"], r.omega, y_T=y_T, noise=d["z"], plan=r.plan)
        if r.model.precision != "split_f16":
            bad.append(f"{tag}: precision mode left as {r.model.precision}")
        r.model.set_precision("f32")
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            exact = r.ddpm.sample(d["cond"], r.omega, y_T=y_T, noise=d["z"], plan=r.plan, check_range=False)
        r.ddpm._range_unchecked = False
        if r.model.range_exceeded():
            bad.append(f"{tag}: flag UP in f32 mode")
        r.model.set_precision("split_f16")
        if not torch.equal(got, exact):
            bad.append(f"{tag}: the fallback differs from the f32-mode call (rel {rel(got, exact):.2e})")
        if not s.cancel:
            e, bound = r.err(s, exact)
            print(f"{tag}: f32 mode at A_OUT vs float64 oracle {e:.2e} (bound {bound:.2e})")
            if not e <= bound:
                bad.append(f"{tag}: f32 mode err {e:.2e} > {bound:.2e}")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ the condition operand
def _cond_case(name, B, entry):
    """Parameters, condition and the column: `cond[-1, c] = entry`, every block's cond_emb column c divided by it (embeddings stay of order 1)."""
    plan, base = E.scenarios(name, SEED, E.A_IN, only=set())[:2]
    c = 2
    p = {k: v.clone() for k, v in base.items()}
    for k in p:
        if k.endswith(".cond_emb.weight"):
            p[k][:, c] /= entry
    cond = _data(name, B)["cond"].clone()
    cond[-1, c] = entry
    return plan, p, cond


@pytest.mark.parametrize("form", ["tile", "large", "full", "rowt", "forward", "train"])
def test_condition_operand_is_guarded(form):
    """16 * silu(cond * mask) is split with no LayerNorm in front (k_cond_embed_h; the training weight gradients read the same fragments):
    an entry of 3 000 (48 000 at the activation scale) is in range and accurate, one of 5 000 (80 000) must raise the flag -- k_cond_frag,
    behind the handle's flag pointer, at each of its three launch sites: the sampling call (tile, large, full), `model(x, t, cond, mask)`
    (rowt, forward) and the training step.  In f32 mode the flag stays down (the exact path passes no pointer), the plain sample() falls
    back to the exact kernels, and where the call takes a mask a MASKED row holding the entry leaves the flag down: silu(5000 * 0) = 0."""
    name, B = "msr80", 33
    r = _Runner(name, form, B)
    d = _data(name, B)

    def call(cond, mask=None, **kw):
        mask = r.d["mask"] if mask is None else mask.cuda()
        if r.kind == "sample":
            out = r.ddpm.sample(cond.cuda(), OMEGA, y_T=d["y_T"], noise=d["z"], **kw)
            r.ddpm._range_unchecked = False
            return out
        if r.kind == "forward":
            return r.model(r.d["y_T"].cuda(), r.d["t"], cond.cuda(), mask)
        with torch.no_grad():
            return r.ddpm(r.d["y"], cond.cuda(), ts=r.d["ts"], noise=r.d["noise"], cond_mask=mask)

    def unchecked(cond, mask=None):
        return call(cond, check_range=False) if r.kind == "sample" else call(cond, mask)

    # in range
    plan, p, cond = _cond_case(name, B, 3000.0)
    r.model.load_state_dict(p)
    out = unchecked(cond)
    assert not r.model.range_exceeded()
    if r.kind == "sample":
        ref, budget = E.in_range_budget(p, plan, T, cond, OMEGA, d["y_T"], d["z"])
        e, bound = rel(out, ref), TOL + 3.0 * budget
    elif r.kind == "forward":
        ref = E.oracle_forward(p, plan, d["y_T"], d["t"], cond, d["mask"], True)
        budget = rel(E.oracle_forward(p, plan, d["y_T"], d["t"], cond, d["mask"], False), ref)
        e, bound = rel(out, ref), TOL + 3.0 * budget
    else:
        l64 = E.oracle_loss64(p, plan, T, d["y"], cond, d["ts"], d["noise"], d["mask"])
        e, bound = abs(float(out) - float(l64)) / abs(float(l64)), 1e-5
    print(f"cond entry 3000, {form}: err {e:.2e} (bound {bound:.2e})")
    assert e <= bound
    # out of range
    plan, p, cond = _cond_case(name, B, 5000.0)
    r.model.load_state_dict(p)
    unchecked(cond)
    assert r.model.range_exceeded(), "condition entry 5000: flag down"
    assert not r.model.range_exceeded()
    if r.kind != "sample":
        masked = d["mask"].clone()
        masked[-1] = 0.0                                   # the row that holds the entry contributes silu(0) = 0
        out = unchecked(cond, masked)
        assert not r.model.range_exceeded(), "condition entry 5000 in a masked row: flag up"
        assert bool(torch.isfinite(out).all())
    r.model.set_precision("f32")
    exact = unchecked(cond)
    assert r.model.range_status() == 0                     # the exact path passes no flag to the condition launch
    r.model.set_precision("split_f16")
    assert bool(torch.isfinite(exact).all())
    if r.kind == "sample":
        with pytest.warns(UserWarning):
            got = call(cond)
        assert r.model.precision == "split_f16"
        assert torch.equal(got, exact)


# ------------------------------------------------------------------------------------------------ the weight side
def _weights_case(kind):
    plan, base = E.scenarios("msr80", SEED, E.A_IN, only=set())[:2]
    p = {k: v.clone() for k, v in base.items()}
    if kind == "gamma64":            # every LayerNorm gamma of one wide block x 64: 16 * (64 * 1.4 * sqrt(128) + 0.4) = 16 000, in the envelope
        for n in ("norm1", "norm2", "norm3"):
            p[f"down.0.res.{n}.weight"] *= 64.0
    elif kind == "scale":            # one Linear x 2^12, another x 2^-12, biases alike; both feed a LayerNorm, so the net stays of order 1
        for k, f in (("down.0.res.lin1", 4096.0), ("up.18.res.lin2", 1.0 / 4096.0)):
            p[k + ".weight"] *= f
            p[k + ".bias"] *= f
    elif kind == "gamma1e3":         # 16 * 1e3 * sqrt(128) = 181 000
        p["down.1.res.norm2.weight"].fill_(1e3)
    elif kind == "w2p22":
        p["down.3.res.lin2.weight"][5, 7] = float(2 ** 22)
    return plan, p


@pytest.mark.parametrize("form", ["tile", "large"])
@pytest.mark.parametrize("kind", ["gamma64", "scale"])
def test_weights_at_the_edge_of_the_envelope_stay_accurate(kind, form):
    name, B = "msr80", 33
    r = _Runner(name, form, B)
    d = _data(name, B)
    plan, p = _weights_case(kind)
    r.model.load_state_dict(p)
    out = r.ddpm.sample(r.d["cond"], OMEGA, y_T=d["y_T"], noise=d["z"], check_range=False)
    r.ddpm._range_unchecked = False
    assert r.model.range_status() == 0
    ref, budget = E.in_range_budget(p, plan, T, d["cond"], OMEGA, d["y_T"], d["z"])
    e = rel(out, ref)
    print(f"{kind}/{form}: err {e:.2e} (bound {TOL + 3.0 * budget:.2e})")
    assert e <= TOL + 3.0 * budget


@pytest.mark.parametrize("kind", ["gamma1e3", "w2p22"])
def test_weights_outside_the_envelope_are_reported(kind):
    """A LayerNorm whose 16 * (max|gamma| sqrt(N) + max|beta|) exceeds 6e4, or a Linear with max|W| >= 2^21, is outside what the split path
    represents, and no activation statistic shows it: the bind computes the word, the range query reports it (bit 2, not cleared by the
    query), check_range names it, the plain sample() takes the exact path, and the next bind of good weights clears it."""
    name, B = "msr80", 33
    r = _Runner(name, "tile", B)
    d = _data(name, B)
    plan, base = E.scenarios(name, SEED, E.A_IN, only=set())[:2]
    r.run(E.Scenario("base", "", 0.0, 0, False, base, None, (), False))
    assert r.model.range_status() == 0
    _, p = _weights_case(kind)
    r.model.load_state_dict(p)
    assert not r.model.weights_known_outside_envelope()                      # nobody has asked since this bind
    with pytest.warns(UserWarning, match="weights"):                         # the first plain call finds out, says so and falls back
        got = r.ddpm.sample(r.d["cond"], OMEGA, y_T=d["y_T"], noise=d["z"])
    assert r.model.precision == "split_f16"
    assert r.model.range_status() & 2
    assert r.model.range_status() & 2 and r.model.range_exceeded()           # not cleared by the query
    with pytest.raises(RuntimeError, match="weights are outside the envelope"):
        r.model.check_range()
    # the word is a property of the bind: once a query has seen it, the plain call goes straight to the exact kernels -- no second
    # split-f16 attempt, no second warning -- until the weights change
    assert r.model.weights_known_outside_envelope()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        again = r.ddpm.sample(r.d["cond"], OMEGA, y_T=d["y_T"], noise=d["z"])
    assert torch.equal(again, got) and r.model.precision == "split_f16"
    r.model.set_precision("f32")
    assert r.model.range_status() == 0                                         # the exact path has no envelope to report
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        exact = r.ddpm.sample(r.d["cond"], OMEGA, y_T=d["y_T"], noise=d["z"])
    r.model.set_precision("split_f16")
    assert torch.equal(got, exact) and bool(torch.isfinite(got).all())
    # and what it fell back to is right: the exact kernels under these weights against the float64 oracle (gamma = 1e3 puts the SiLU
    # argument beyond +-88, where the exact path's exp(-u) used to overflow into NaN)
    ref, budget = E.in_range_budget(p, plan, T, d["cond"], OMEGA, d["y_T"], d["z"])
    e = rel(got, ref)
    print(f"{kind}: exact fallback vs float64 oracle {e:.2e} (bound {TOL + 3.0 * budget:.2e})")
    assert e <= TOL + 3.0 * budget
    r.model.load_state_dict(base)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r.ddpm.sample(r.d["cond"], OMEGA, y_T=d["y_T"], noise=d["z"])
    assert r.model.range_status() == 0 and not r.model.weights_known_outside_envelope()
