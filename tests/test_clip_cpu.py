"""The x0 clip without a device: the per-step scalars against float64, `with_clip` / `check_clip` / `clip_bounds` and every
refusal, the `with_*` helpers carry the clip, variants with differing clips are refused before any device call, the `clipping` context
leaves the pinned signatures alone, the C ABI declares the setter (no stream), the bounds of the parity cases of tests/test_gpu_clip.py
bind where they should, the cases have the error budgets their bound assumes, and the NU checkpoint's cells are the recorded ones."""
import json
import os
import re

import numpy as np
import pytest
import torch

import clip_ref as C
import steps_ref as R
from _util import GOLD, ROOT
from test_steps_cpu import make_ddpm

INF = float("inf")


# ------------------------------------------------------------------------------------------------ C ABI
def test_header_and_binding_declare_the_setter():
    import ctypes
    from diffsg_amd import _lib
    with open(os.path.join(ROOT, "include", "diffsg.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    m = re.search(r"\bint\s+dsg_set_xstart_clip\s*\(([^()]*)\)\s*;", hdr)
    assert m, "include/diffsg.h does not declare dsg_set_xstart_clip"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == ["dsg_handle* h", "const float* lo_host", "const float* hi_host", "int D",
                                                                   "const float* x0_host", "int n"]
    res, args = _lib._SIGS["dsg_set_xstart_clip"]
    fp = ctypes.POINTER(ctypes.c_float)
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p, fp, fp, ctypes.c_int, fp, ctypes.c_int]
    assert hasattr(_lib.lib(), "dsg_set_xstart_clip")


def test_the_setter_takes_no_stream():
    """By design: a settings call like dsg_set_step_history (it synchronises the handle's device before it replaces its buffers)."""
    import ctypes
    import test_streams_cpu as S
    from diffsg_amd import _lib
    with open(os.path.join(ROOT, "include", "diffsg.h")) as f:
        assert re.search(r"\bint\s+dsg_set_xstart_clip\s*\(", f.read()), "include/diffsg.h does not declare dsg_set_xstart_clip"
    assert ctypes.c_void_p not in _lib._SIGS["dsg_set_xstart_clip"][1][1:]      # bound, and no argument but the handle is a void*
    assert "dsg_set_xstart_clip" not in S.stream_functions()
    assert "dsg_sample" in S.stream_functions()


def test_the_clip_kernels_live_in_their_own_header_and_the_old_ones_keep_their_names():
    def names(header):
        with open(os.path.join(ROOT, "diffsg_amd", "csrc", header)) as f:
            return re.findall(r"__global__\s+__launch_bounds__\(256\)\s+void\s+(k_update\w*)\s*\(", f.read())
    assert names("dsg_clip.hpp") == ["k_update_clip", "k_update_clip_sched", "k_update_clip_var", "k_update_clip_var_sched", "k_update_clip_hist",
                                     "k_update_clip_hist_sched"]
    assert names("dsg_kernels.hpp") == ["k_update", "k_update_var", "k_update_sched", "k_update_var_sched"]
    assert names("dsg_multistep.hpp") == ["k_update_hist", "k_update_hist_sched"]


# ------------------------------------------------------------------------------------------------ the scalars
@pytest.mark.parametrize("name", list(C.NETS))
def test_x0_rows_are_within_one_ulp_of_float64(name):
    from diffsg_amd import steps
    T, K = C.NETS[name]
    d = make_ddpm(T)
    taus = R.default_taus(T, K)
    got = steps.x0_rows(d, taus)
    assert got.dtype == torch.float32 and tuple(got.shape) == (K, 4)
    want = C.x0_rows64(R.acp64(T), taus)
    g = got.numpy()
    err = np.abs(g.astype(np.float64) - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    print(f"{name}: worst {err.max():.3f} ulp")
    assert float(err.max()) <= 1.0
    assert bool(np.isfinite(g).all()) and bool((g > 0).all())
    assert torch.equal(steps.x0_rows(d, range(T)), C.x0_rows(T, range(T)))              # the identity plan's rows: the reference's, bit for bit


# ------------------------------------------------------------------------------------------------ with_clip, check_clip, clip_bounds
def bad_clips(D):
    """[((lo, hi), what the message names)]: every refusal of check_clip / dsg_set_xstart_clip on well-shaped bounds."""
    lo, hi = [0.0] * D, [1.0] * D
    nan_lo = list(lo); nan_lo[D - 1] = float("nan")
    nan_hi = list(hi); nan_hi[0] = float("nan")
    crossed = list(lo); crossed[D // 2] = 1.5
    inf_crossed = list(lo); inf_crossed[0] = INF
    return [((nan_lo, hi), "NaN"), ((lo, nan_hi), "NaN"), ((crossed, hi), "above hi"), ((inf_crossed, hi), "above hi")]


def bad_rows(rows):
    """Every refusal of dsg_set_xstart_clip on the rows {s, ia, a, is}: a scalar that is not finite and > 0."""
    out = []
    for at, v in ((0, 0.0), (1, -0.5), (2, float("nan")), (len(rows) - 1, INF), (len(rows) - 2, -INF)):
        r = list(rows); r[at] = v
        out.append(r)
    return out


def test_with_clip_values():
    from diffsg_amd import steps
    from diffsg_amd.steps import StepPlan
    T, K = 8, 5
    d = make_ddpm(T)
    base = steps.ddim(d, K)
    assert base.clip is None
    for n in (4, 5, 6):                                                       # four- to six-argument construction keeps working
        assert StepPlan(*(base.taus, base.t, base.coef, base.renorm_steps, None, None)[:n]).clip is None
    p = steps.with_clip(base, [0.0, -1.0, 0.25], [1.0, INF, 0.25])
    assert p.clip.dtype == torch.float32 and tuple(p.clip.shape) == (2, 3)
    assert p.clip.tolist() == [[0.0, -1.0, 0.25], [1.0, INF, 0.25]]           # lo == hi and an infinite bound are allowed
    assert p.coef is base.coef and p.t is base.t and p.taus is base.taus and p.renorm_steps == base.renorm_steps
    s = steps.with_clip(base, 0.0, 1.0)                                       # scalars: one pair, spread over the features by the call
    assert s.clip.tolist() == [[0.0], [1.0]]
    m = steps.with_clip(base, -0.5, [1.0, 2.0, 3.0])
    assert m.clip.tolist() == [[-0.5] * 3, [1.0, 2.0, 3.0]]
    assert steps.with_clip(base, np.float64(0.1), torch.tensor([0.5, 0.75, 1.0], dtype=torch.float64)).clip.dtype == torch.float32
    assert steps.with_clip(p, None).clip is None and steps.with_clip(p, None).coef is base.coef
    ident = steps.with_clip(d, -INF, INF)
    assert ident.taus == tuple(range(T)) and ident.coef is d._coef_table() and ident.renorm_steps == min(T, 4) and ident.clip.tolist() == [[-INF], [INF]]
    steps.check_clip(p.clip)
    steps.check_clip(p.clip, 3)
    steps.check_clip(s.clip, 3)


def test_clip_bounds_values():
    from diffsg_amd import steps
    Y = np.array([[0.0, 2.0, -1.0], [1.0, 2.0, 3.0], [0.5, 2.0, 1.0]])
    lo, hi = steps.clip_bounds(Y)
    assert lo.dtype == hi.dtype == torch.float32
    assert lo.tolist() == [-0.25, 2.0, -2.0] and hi.tolist() == [1.25, 2.0, 4.0]
    lo, hi = steps.clip_bounds(torch.tensor(Y), margin=0.0)
    assert lo.tolist() == [0.0, 2.0, -1.0] and hi.tolist() == [1.0, 2.0, 3.0]
    lo, hi = steps.clip_bounds(Y, 1.0)
    assert lo.tolist() == [-1.0, 2.0, -5.0] and hi.tolist() == [2.0, 2.0, 7.0]
    steps.check_clip(torch.stack(steps.clip_bounds(Y)), 3)
    for bad in (lambda: steps.clip_bounds(Y, -0.1), lambda: steps.clip_bounds(Y, float("nan")), lambda: steps.clip_bounds(Y[0]),
                lambda: steps.clip_bounds(np.zeros((0, 3))), lambda: steps.clip_bounds(np.array([[0.0, float("nan")]])),
                lambda: steps.clip_bounds(np.array([[0.0, INF]]))):
        with pytest.raises(ValueError, match="clip_bounds"):
            bad()


def test_refusals_need_no_device():
    from diffsg_amd import steps
    from diffsg_amd.steps import StepPlan
    T, K, D = 8, 5, 3
    d = make_ddpm(T)
    cond = torch.zeros(96, 3)
    a = steps.ddim(d, K)
    shaped = [(torch.zeros(3, D), "shape"), (torch.zeros(2 * D), "shape"), (torch.zeros(2, D, 1), "shape"), (torch.zeros(2, 0), "shape"),
              (torch.zeros(2, D, dtype=torch.float64), "float32"), ([[0.0] * D, [1.0] * D], "float32")]
    valued = [(torch.tensor([lo, hi], dtype=torch.float32), what) for (lo, hi), what in bad_clips(D)]
    for bad, what in shaped + valued:
        with pytest.raises(ValueError, match="clip.*" + re.escape(what)):
            steps.check_clip(bad)
        plan = StepPlan(a.taus, a.t, a.coef, a.renorm_steps, None, None, bad)
        for call in (lambda: d.sample(cond, 1.0, plan=plan), lambda: d.sample_chunked(cond, 1.0, 32, plan=plan),
                     lambda: d.sample_chunked(cond, 1.0, 32, variants=[(1.0, plan)] * 3), lambda: d.sample_best(cond, cond, 2, variants=[(1.0, plan)])):
            with pytest.raises(ValueError, match="clip.*" + re.escape(what)):
                call()
    for (lo, hi), what in bad_clips(D):
        with pytest.raises(ValueError, match="clip.*" + re.escape(what)):
            steps.with_clip(a, lo, hi)
    # another feature count than the model's: refused by the call, naming both
    wrong = steps.with_clip(a, [0.0] * (D + 1), [1.0] * (D + 1))
    with pytest.raises(ValueError, match=f"clip.*{D + 1} features.*D = {D}"):
        d.sample(cond, 1.0, plan=wrong)
    with pytest.raises(ValueError, match="clip.*3"):
        steps.check_clip(wrong.clip, D)
    for bad in (lambda: steps.with_clip(a, 0.0), lambda: steps.with_clip(a, [0.0, 0.0], [1.0, 1.0, 1.0])):
        with pytest.raises(ValueError, match="with_clip"):
            bad()
    # a well-formed plan gets as far as the device check
    good = steps.with_clip(a, [0.0, 0.1, 0.2], [1.0, 0.9, INF])
    for call in (lambda: d.sample(cond, 1.0, plan=good), lambda: d.sample_chunked(cond, 1.0, 32, plan=good),
                 lambda: d.sample(cond, 1.0, plan=steps.with_clip(steps.dpmpp_2m(d, K, renorm_steps=0), 0.0, 1.0)),
                 lambda: d.sample_chunked(cond, 1.0, 32, variants=[(1.0, good), (2.0, steps.with_renorm(good, 1)), (3.0, good)])):
        with pytest.raises(RuntimeError, match="not on a HIP device"):
            call()


def test_with_friends_carry_the_clip_and_share_tensors():
    from diffsg_amd import steps
    T, K = 8, 5
    d = make_ddpm(T)
    base = steps.with_clip(steps.ddim(d, K), [0.0, 0.1, 0.2], [1.0, 0.9, 0.8])
    r = steps.with_renorm(base, 2)
    assert r.clip is base.clip and r.coef is base.coef and r.renorm_steps == 2
    g = steps.with_guidance(base, [1.0, 0.0, 0.5, 0.0, 1.0])
    assert g.clip is base.clip and g.coef is base.coef and g.t is base.t
    assert steps.with_guidance(g, None).clip is base.clip
    two = steps.dpmpp_2m(d, K, renorm_steps=0)
    h = steps.with_history(base, two.history.tolist())
    assert h.clip is base.clip and h.coef is base.coef and h.history is not None
    assert steps.with_history(h, None).clip is base.clip
    c = steps.with_clip(steps.with_guidance(two, [1.0] * K), 0.0, 1.0)
    assert c.history is two.history and c.guidance is not None and c.coef is two.coef
    off = steps.with_clip(c, None)
    assert off.clip is None and off.history is two.history and off.guidance is c.guidance


def test_variants_with_differing_clips_are_refused_before_any_device_call():
    from diffsg_amd import steps
    T, K = 8, 5
    d = make_ddpm(T)
    cond = torch.zeros(96, 3)
    a = steps.ddim(d, K)
    one = steps.with_clip(a, [0.0] * 3, [1.0] * 3)
    same = steps.with_clip(steps.with_renorm(a, 1), [0.0] * 3, [1.0] * 3)      # another tensor, the same bounds
    other = steps.with_clip(a, [0.0] * 3, [1.0, 1.0, 1.5])
    ident = steps.with_clip(d, 0.0, 1.0)                                      # all T steps: a variant without a plan is that grid, no clip
    for bad in ([(1.0, one), (2.0, other), (1.0, one)], [(1.0, one), (2.0, a), (1.0, one)], [(1.0, a), (2.0, one), (1.0, a)],
                [(1.0, ident), (2.0, None), (1.0, ident)]):
        with pytest.raises(ValueError, match="variant 1.*clip"):
            d.sample_chunked(cond, 1.0, 32, variants=bad)
        with pytest.raises(ValueError, match="variant 1.*clip"):
            d.sample_best(cond, cond, 3, variants=bad)
    scalar = steps.with_clip(a, 0.0, 1.0)                                     # [2, 1]: the same bounds once spread over the features
    with pytest.raises(RuntimeError, match="not on a HIP device"):
        d.sample_chunked(cond, 1.0, 32, variants=[(1.0, one), (2.0, same), (1.0, scalar)])
    with pytest.raises(ValueError, match="variant 2.*clip"):
        d.sample_chunked(cond, 1.0, 32, variants=[(1.0, one), (2.0, same), (1.0, steps.with_clip(a, 0.0, 1.5))])


# ------------------------------------------------------------------------------------------------ the context of the pinned entry points
def test_clipping_context_and_entry_clipped():
    from diffsg_amd import entry, steps
    from test_entry_cpu import test_public_signatures_are_the_recorded_ones
    T, K = 8, 5
    d = make_ddpm(T)
    Y_train = np.array([[0.0, 2.0, -1.0], [1.0, 3.0, 3.0]])
    a, own = steps.ddim(d, K), steps.with_clip(steps.ddim(d, K), -9.0, 9.0)
    assert entry.clipping is steps.clipping
    assert entry.clipped(d, a, None, Y_train) == (a, None) and entry.clipped(d, None, [(1.0, a)], Y_train)[0] is None      # outside: nothing
    with steps.clipping([0.0, 0.125, 0.25], [1.0, 1.125, 1.25]):
        test_public_signatures_are_the_recorded_ones()
        plan, variants = entry.clipped(d, None, None, Y_train)
        assert variants is None and plan.taus == tuple(range(T)) and plan.coef is d._coef_table() and plan.clip.tolist() == [[0.0, 0.125, 0.25], [1.0, 1.125, 1.25]]
        plan, variants = entry.clipped(d, a, [(1.0, a), (2.0, own), (3.0, None)], Y_train)
        assert plan.coef is a.coef and plan.clip.tolist() == [[0.0, 0.125, 0.25], [1.0, 1.125, 1.25]]
        assert [o for o, _ in variants] == [1.0, 2.0, 3.0]
        assert variants[0][1].clip is plan.clip and variants[0][1].coef is a.coef
        assert variants[1][1] is own                                          # a clip of its own stays
        assert variants[2][1].taus == tuple(range(T)) and variants[2][1].clip.tolist() == plan.clip.tolist()
        with steps.clipping(margin=0.5):                                      # nested: the inner one holds, then the outer one again
            p2, _ = entry.clipped(d, a, None, lambda: Y_train)
            assert p2.clip.tolist() == [[-0.5, 1.5, -3.0], [1.5, 3.5, 5.0]]
        assert entry.clipped(d, a, None, Y_train)[0].clip.tolist() == plan.clip.tolist()
    assert entry.clipped(d, a, None, Y_train) == (a, None)
    with steps.clipping(margin=0.25):
        p3, _ = entry.clipped(d, None, None, Y_train)
        lo, hi = steps.clip_bounds(Y_train, 0.25)
        assert p3.clip.tolist() == [lo.tolist(), hi.tolist()]
    for bad in (lambda: steps.clipping(), lambda: steps.clipping(0.0), lambda: steps.clipping(0.0, 1.0, margin=0.1), lambda: steps.clipping(margin=-1.0),
                lambda: steps.clipping(1.0, 0.0), lambda: steps.clipping([0.0, float("nan")], [1.0, 1.0])):
        with pytest.raises(ValueError):
            with bad():
                pass
    assert steps.active_clip(Y_train) is None


def test_load_test_entry_points_read_the_context():
    """Each `load_test_*` passes its plan and variants through `entry.clipped` with its loader's training labels."""
    for mod, loader in (("classifier_free_MSR", "msr_data_load"), ("classifier_free_CO", "co_data_load"), ("classifier_free_NU", "nu_data_load")):
        with open(os.path.join(ROOT, "diffsg_amd", mod + ".py")) as f:
            src = f.read()
        body = src[src.index("def load_test_" + mod[-3:].lower().lstrip("_")):]
        body = body[:body.index("\ndef ", 1)]
        assert re.search(r"Y_train[^\n]*=\s*" + loader + r"\(", body), mod
        assert "plan, variants = entry.clipped(diffusion_model, plan, variants, Y_train)" in body, mod


# ------------------------------------------------------------------------------------------------ the reference, its bounds and budgets
def test_reference_without_a_clip_is_the_older_references():
    import multistep_ref as M
    name, omega = "tiny", 2.0
    T, K = C.NETS[name]
    net, p = R.net_params(name)
    cond, y_T, z = C.inputs(name, 70)
    for sampler in ("ddim0.5", "dpmpp2m"):
        plan = C.case_plan(name, sampler)
        want = (M.sample_multistep(p, net, plan, T, cond, omega, y_T, z[:K - 2]) if sampler == "dpmpp2m" else
                R.sample_plan(p, net, R.case_plan(name, sampler), T, cond, omega, y_T, z[:K - 2]))
        D = y_T.shape[1]
        inf = torch.full((D,), INF)
        assert torch.equal(C.sample_clip(p, net, plan, T, cond, omega, y_T, z[:K - 2]), want)
        assert torch.equal(C.sample_clip(p, net, plan, T, cond, omega, y_T, z[:K - 2], (-inf, inf)), want)
    # the rule keeps a NaN and touches nothing inside the bounds
    y, e = torch.tensor([[0.5, float("nan"), 3.0]]), torch.tensor([[0.25, 0.5, -1.0]])
    row = C.x0_rows(T, [3])[0]
    out, x0, moved = C.clip_eps(y, e, torch.zeros(3), torch.ones(3), row)
    assert moved.tolist() == [[False, False, True]] and out[0, 0] == e[0, 0] and torch.isnan(x0[0, 1]) and out[0, 1] == e[0, 1]
    assert abs(float((y[0, 2] - row[0] * out[0, 2]) * row[1]) - 1.0) <= 1e-6         # the new eps predicts the bound


@pytest.mark.parametrize("name", list(C.NETS))
def test_bounds_and_budgets_of_the_gpu_cases(name):
    """Bounds: per case the 0.2 / 0.8 quantiles of the unclipped float32 reference's x0 -- all different per feature; in every step of every
    case some elements are clipped and some are not; the mean clipped share of a case lies in [0.2, 0.6].
    Budgets: the reference's own float32-against-float64 error of every case tests/test_gpu_clip.py compares with it is at most
    CAP / 2 = 5e-6, all three nets.  Measured: worst `tiny` 1.6e-6 (weight seed 3), `nu3` 4.5e-7, `msr3` 3.6e-6 under weight seed
    19 -- the first from 3 upwards within CAP / 2: under the clip seed 3 has 2.4e-5 (ddim0, omega = 2, 72 rows) and each of
    the seeds 4 .. 18 has a case above 5e-6 (clip_ref.PASSED_OVER names one per seed; recomputed here).  Per-step clipped share
    0.005 ... 0.951, mean per case 0.265 ... 0.412."""
    D = None
    for case in C.CASES:
        lo, hi = C.bounds(name, *case)
        D = lo.numel()
        assert len(set(lo.tolist())) == D and len(set(hi.tolist())) == D and bool((lo < hi).all()), case
        share = C.reference(name, *case).share
        assert len(share) == C.NETS[name][1]
        print(f"{name} {case}: clipped share per step {min(share):.3f} ... {max(share):.3f}, mean {np.mean(share):.3f}")
        assert all(0.0 < s < 1.0 for s in share), (case, share)
        assert 0.2 <= float(np.mean(share)) <= 0.6, (case, share)
    b = C.budgets(name)
    for key, v in b.items():
        print(f"{name} {key}: budget {v:.2e}")
    assert max(b.values()) <= C.CAP / 2, b
    if name != "nu3":
        passed = C.PASSED_OVER.get(name, {})
        assert sorted(passed) == list(range(3, C.SEEDS[name]))
        for seed, case in passed.items():
            v = R.rel(*C.reference(name, *case, seed)[:2])
            print(f"{name} seed {seed} {case}: budget {v:.2e}")
            assert v > C.CAP / 2, f"seed {seed}: the named case meets the cap"


# ------------------------------------------------------------------------------------------------ the quality table
def test_nu_checkpoint_cells_are_the_recorded_ones():
    """The shipped NU checkpoint (512 rows, T = 20, its own y_T and z) with and without the clip: recomputed here, within 2e-5 of
    tests/golden/g21_clip.json."""
    with open(os.path.join(GOLD, "g21_clip.json")) as f:
        rec = json.load(f)
    assert (rec["rows"], rec["T"]) == (512, 20)
    got = C.nu_cells()
    assert sorted(got) == sorted(rec["cells"]) == sorted(c[0] for c in C.NU_CELLS)
    for k in got:
        print(f"{k}: plain {got[k]['plain']:.6f} (recorded {rec['cells'][k]['plain']:.6f}), clip {got[k]['clip']:.6f} "
              f"(recorded {rec['cells'][k]['clip']:.6f}); max |y| {got[k]['max_plain']:.3g} / {got[k]['max_clip']:.3g}")
    for k in got:
        for tag in ("plain", "clip"):
            assert abs(got[k][tag] - rec["cells"][k][tag]) <= 2e-5, (k, tag, got[k][tag], rec["cells"][k][tag])
    # the clip bounds the path where the unclipped one blows up (the noise of an ancestral step comes on top of the clamped prediction)
    for k in got:
        assert got[k]["max_clip"] <= 6.0 and abs(got[k]["max_clip"] - rec["cells"][k]["max_clip"]) <= 1e-3 * rec["cells"][k]["max_clip"], k
