"""Scenario builder for the fp16 range guard of the split-f16 path (csrc/dsg_split.hpp: kRawLimit), in the style of the other *_ref.py.

The split path feeds some tensors to the matrix cores RAW (scale 1, no LayerNorm in front): `y` into feature_proj, the input of every
Down/Upsample Linear, and both halves (running x, popped skip) of every up block's Linear shortcut.  A kernel that splits such an operand
bounds its rows by |mean| + sqrt(M2) and raises the handle's range flag above 6e4.  To test ONE such read at a time a scenario puts ONE
tensor out of range and keeps every other raw-read tensor, and eps, of order 1:

  * feature j of the tensor becomes A in every row: A is added to the producer's output bias (`....res.lin3.bias[j]`, `....lin.bias[j]`,
    `feature_proj.bias[j]`);
  * column j of every raw consumer's weight is divided by A (`....shortcut.weight[:, j]` for the running half, `[:, w + j]` for the skip
    half behind a w-wide running half, `....lin.weight[:, j]`), so the products stay of order 1;
  * where the tensor is carried on by an identity shortcut (out = x + h: the down and middle blocks) the next block's `lin3.bias[j]`
    takes A away again: `cancel=True`.  The sum (A + x) + (h - A) loses 16 bits of feature j in float32, so such scenarios are for the
    flag only, never for accuracy;
  * the `y` scenario sets one element of the LAST row of the start state to A and divides that column of feature_proj.weight by A.

Everything is derived from the oracle's `unet_plan`, so the list is complete for any config (tests/test_envelope_cpu.py checks that, and
that every scenario is isolated).  Amplitudes follow from the code, not from a measurement: a row with one entry A among N has
|mean| + sqrt(M2) <= A (sqrt(1 - 1/N) + 1/N) <= 1.15 A for N >= 3, so A_IN = 5e4 stays under the limit (<= 57 500) while A_OUT = 7e4 is above
the limit AND above fp16's largest finite value 65 504.

The guard has a low side too (kRawFloor, kRawFloorIn: rows whose entries are all small); its scenarios scale whole stream segments and are
described where they are built ("the low side", below).
"""
import functools
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from oracle import ddpm_oracle as O

A_IN = 5.0e4
A_OUT = 7.0e4
RAW_LIMIT = 6.0e4          # kRawLimit (csrc/dsg_split.hpp)
QUIET = 3.0e4              # every raw read a scenario does NOT target stays below this
F16_MAX = 65504.0

# one raw read: `site` = state-dict prefix of the Linear that reads, `tensors` = taps names of what it reads (two for a shortcut over a
# concat: the kernels bound the concatenated row, Chan-merged), `col0` = first weight column of each
Read = namedtuple("Read", "site tensors col0")
# one raw-read tensor: its taps name ("y": the network input), width, the bias that produces it, the bias of the identity-shortcut block
# that carries it on (or None), its reads [(site, first column)]
Tensor = namedtuple("Tensor", "name width bias carry reads")
Scenario = namedtuple("Scenario", "name tensor A j cancel params y_col sites v8_only")


def _out_bias(kind, prefix):
    return prefix + (".res.lin3.bias" if kind == "res" else ".lin.bias")


def raw_tensors(plan):
    """OrderedDict name -> Tensor of every tensor a split-path kernel reads raw, walking the plan as `unet_forward` does."""
    out = OrderedDict()
    width = {"y": plan["input_dim"], "feature_proj": plan["proj_dim"]}
    bias = {"y": None, "feature_proj": "feature_proj.bias"}
    carry = {}

    def read(name, site, col0):
        if name not in out:
            out[name] = Tensor(name, width[name], bias[name], None, [])
        out[name].reads.append((site, col0))

    read("y", "feature_proj", 0)
    cur, skips = "feature_proj", ["feature_proj"]
    for idx, (kind, i, o) in enumerate(plan["down"]):
        name = f"down.{idx}"
        width[name], bias[name] = o, _out_bias(kind, name)
        if kind == "lin":
            read(cur, name + ".lin", 0)
        elif i != o:
            read(cur, name + ".res.shortcut", 0)
        else:
            carry[cur] = name + ".res.lin3.bias"
        cur = name
        skips.append(name)
    carry[cur] = "middle.res1.lin3.bias"
    width["middle"], bias["middle"] = plan["mid_w"], "middle.res2.lin3.bias"
    cur = "middle"
    for idx, (kind, i, o) in enumerate(plan["up"]):
        name = f"up.{idx}"
        width[name], bias[name] = o, _out_bias(kind, name)
        if kind == "lin":
            read(cur, name + ".lin", 0)
        else:
            sk = skips.pop()
            assert width[cur] + width[sk] == i and i != o, (name, cur, sk)
            read(cur, name + ".res.shortcut", 0)
            read(sk, name + ".res.shortcut", width[cur])
        cur = name
    assert not skips
    return OrderedDict((k, t._replace(carry=carry.get(k))) for k, t in out.items())


def raw_reads(plan):
    """[Read] of every raw read site, in launch order: what each split-path Linear over a raw operand is given."""
    sites = OrderedDict()
    for t in raw_tensors(plan).values():
        for site, col0 in t.reads:
            sites.setdefault(site, []).append((col0, t.name))
    return [Read(site, tuple(n for _, n in sorted(v)), tuple(c for c, _ in sorted(v))) for site, v in sites.items()]


def v8_section(plan):
    """Names of the tensors that are read ONLY inside the float32 vector section of the narrow run (csrc/dsg_narrow8.hpp: Downsample 16 -> 8
    ... Upsample 8 -> 16, built for 2 or 3 blocks per resolution): every 8-wide tensor of such a net.  With `narrow_valu8` on their reads are
    exact float32 and raise no flag."""
    downs = [(i, o) for kind, i, o in plan["down"] if kind == "lin"]
    nb = sum(1 for kind, i, o in plan["down"] if kind == "res" and i == plan["mid_w"])
    if not downs or downs[-1] != (16, 8) or nb not in (2, 3):
        return frozenset()
    return frozenset(t.name for t in raw_tensors(plan).values() if t.name != "y" and t.width == 8)


def feature_of(t, k):
    """The feature a scenario raises: fixed per tensor, spread over the fragment groups."""
    return (3 + 5 * k) % t.width


@functools.lru_cache(maxsize=None)
def base_params(name, seed):
    """(plan, synth_params(name, seed)), made once: callers treat the tensors as read only."""
    from _util import synth_params
    return synth_params(name, seed)


def scenarios(name, seed, A, only=None):
    """(plan, base parameters, [Scenario]) for config `name`: one scenario per raw-read tensor at amplitude A (`only`: a set of tensor names)."""
    plan, base = base_params(name, seed)
    v8 = v8_section(plan)
    out = []
    for k, t in enumerate(raw_tensors(plan).values()):
        if only is not None and t.name not in only:
            continue
        j = feature_of(t, k)
        p = dict(base)                 # the tensors a scenario does not change are the base's own: read only

        def own(key):
            if p[key] is base[key]:
                p[key] = base[key].clone()
            return p[key]
        if t.bias is not None:
            own(t.bias)[j] += A
        for site, col0 in t.reads:
            own(site + ".weight")[:, col0 + j] /= A
        if t.carry is not None:
            own(t.carry)[j] -= A
        out.append(Scenario(f"{name}:{t.name}@{A:g}", t.name, A, j, t.carry is not None, p, j if t.name == "y" else None,
                            tuple(s for s, _ in t.reads), t.name in v8))
    return plan, base, out


# ------------------------------------------------------------------------------------------------ the low side
# The guard's other edge (csrc/dsg_split.hpp: kRawFloor, kRawFloorIn): a raw operand below 2^-4 has a subnormal lo part and carries an
# absolute error of 2^-25 (tests/split_ref.py), so a row whose entries are ALL small loses bits in proportion to its amplitude.  One outlier
# does not make a row small: a low scenario brings a whole STREAM SEGMENT to amplitude s -- a tensor with a scalable producer
# (feature_proj, a Down/Upsample Linear, an up block with its Linear shortcut) and the tensors identity shortcuts carry it into (out = x + h:
# the following down blocks, the two middle blocks), up to the next block that is no identity:
#   * the producing weight / bias pairs are multiplied by s: `feature_proj.*` or `....lin.*` or the head block's `....res.lin3.*` and
#     `....res.shortcut.*`, and `....res.lin3.*` of every identity-carried successor (so x + h stays of size s);
#   * the segment's columns of every raw consumer's weight are divided by s (`....shortcut.weight[:, col0:col0 + w]`, `....lin.weight`), so the
#     products stay of order 1.  Nothing cancels: every low scenario carries an accuracy claim;
#   * the `y` scenario multiplies the network input (the start state, the forward input, the training step's y AND noise) by s and divides
#     `feature_proj.weight` by s.  (A sampling call renormalises y after its first steps, so only its first step reads a small y.)
# A read is WHOLE in a scenario when every tensor of its row belongs to the segment: the kernels bound the concatenated row of a shortcut,
# so a small half beside a half of order 1 is, by construction of that bound, not a small row (DESIGN.md 7 says what that leaves open).
RAW_FLOOR = 2.0 ** -9      # kRawFloor: rows with 0 < |mean| + sqrt(M2) < this are reported
RAW_FLOOR_IN = 2.0 ** -14  # kRawFloorIn: feature_proj's rows with 0 < max|y| < this are reported
# Amplitudes, from the row bounds tests/test_envelope_cpu.py measures on the oracle's taps (float64): a whole row of a segment at amplitude s
# has |mean| + sqrt(M2) between 1.2 s (an 8-wide row) and 26 s (a 128-wide one, about sqrt(N) times its rms), a row of y has max|y| between
# 0.2 s and 3.9 s.  S_IN is the smallest power of two at which no such row can be within a factor 2 of its floor (1.2 * 2^-8 = 2.4 kRawFloor,
# 0.2 * 2^-8 = 13 kRawFloorIn), S_OUT the largest at which every one must be (26 * 2^-17 = 0.1 kRawFloor, 3.9 * 2^-17 = 0.49 kRawFloorIn).
BOUND_OVER_S = (1.2, 26.0)  # a whole targeted row's |mean| + sqrt(M2), in units of s (tests/test_envelope_cpu.py holds both pairs to the taps)
Y_OVER_S = (0.2, 3.9)       # a row of y: max|y| in units of s
S_IN = 2.0 ** -8
S_OUT = 2.0 ** -17
LOW_CURVE = (2.0 ** -6, 2.0 ** -10, 2.0 ** -14)     # the amplitudes of the accuracy curve


def flag_at(segment, s, must):
    """The state the flag MUST have after a call on segment `segment` at amplitude s, or None where the measured bounds leave it open.
    `must`: the scenario has a whole read outside the float32 section (flagging_sites); without one nothing is claimed.  Up when every
    whole row is under its floor (the largest bound, with a tenth to spare: the kernels' float32 statistics are within 1e-6 of these),
    down when none can be within a factor 2 of it.  S_IN and S_OUT are one floor's worth apart for BOTH floors at once, nine binades;
    this rule also decides the curve's points -- a row segment is down at 2^-6 and up at 2^-14, y is down at 2^-6 and 2^-10 -- which
    holds kRawFloor inside (the widest rows' smallest bound at 2^-14, the narrowest rows' at 2^-8] and kRawFloorIn inside
    (max|y| at 2^-17, at 2^-10] ON THE DEVICE; the source text is checked besides (tests/test_envelope_cpu.py)."""
    if not must:
        return None
    (lo, hi), floor = (Y_OVER_S, RAW_FLOOR_IN) if segment == "y" else (BOUND_OVER_S, RAW_FLOOR)
    if hi * s < 0.9 * floor:
        return True
    if lo * s > 2.0 * floor:
        return False
    return None
LowScenario = namedtuple("LowScenario", "name segment s params y_scale tensors sites whole v8_only")


def segments(plan):
    """[(head tensor name, [prefixes whose weight and bias are multiplied by s], [raw-read tensors of the segment])] in stream order."""
    raw = raw_tensors(plan)
    segs = [["feature_proj", ["feature_proj"], ["feature_proj"]]]
    for idx, (kind, i, o) in enumerate(plan["down"]):
        name = f"down.{idx}"
        if kind == "res" and i == o:
            segs[-1][1].append(name + ".res.lin3")
            segs[-1][2].append(name)
        elif kind == "lin":
            segs.append([name, [name + ".lin"], [name]])
        else:
            segs.append([name, [name + ".res.lin3", name + ".res.shortcut"], [name]])
    segs[-1][1] += ["middle.res1.lin3", "middle.res2.lin3"]
    segs[-1][2].append("middle")
    for idx, (kind, i, o) in enumerate(plan["up"]):
        name = f"up.{idx}"
        assert kind == "lin" or i != o
        segs.append([name, [name + ".lin"] if kind == "lin" else [name + ".res.lin3", name + ".res.shortcut"], [name]])
    # the last module's output goes to the final LayerNorm: no raw read, no scenario.  A carried tensor that nothing reads raw does not exist
    # (every module output but the last is a skip or the next Linear's input); keep the raw-read ones only
    return [(h, keys, [t for t in ts if t in raw]) for h, keys, ts in segs if any(t in raw for t in ts)]


def site_in_v8(plan, site):
    """Is the Linear at `site` an operator of the narrow run's float32 vector section (one side 8 wide, see v8_section)?"""
    return bool(v8_section(plan)) and min(O.state_shapes(plan)[site + ".weight"]) == 8


def low_scenarios(name, seed, s, only=None):
    """(plan, base parameters, [LowScenario]) for config `name` at amplitude s: `y`, then one per stream segment (`only`: a set of segment names)."""
    plan, base = base_params(name, seed)
    raw, v8, reads = raw_tensors(plan), v8_section(plan), raw_reads(plan)
    out = []

    def make(seg, keys, tensors, y_scale):
        p = dict(base)
        for k in keys:
            p[k + ".weight"], p[k + ".bias"] = base[k + ".weight"] * s, base[k + ".bias"] * s
        sites = []
        for t in tensors:
            for site, col0 in raw[t].reads:
                key = site + ".weight"
                if p[key] is base[key]:
                    p[key] = base[key].clone()
                p[key][:, col0:col0 + raw[t].width] /= s
                if site not in sites:
                    sites.append(site)
        whole = tuple(r.site for r in reads if r.site in sites and all(t in tensors for t in r.tensors))
        out.append(LowScenario(f"{name}:low:{seg}@{s:g}", seg, s, p, y_scale, tuple(tensors), tuple(sites), whole,
                               all(t in v8 for t in tensors)))

    if only is None or "y" in only:
        make("y", [], ["y"], s)
    for head, keys, tensors in segments(plan):
        if only is None or head in only:
            make(head, keys, tensors, None)
    return plan, base, out


def flagging_sites(plan, scn, v8):
    """The sites that must raise the flag when the segment is under the floor: its whole reads, less -- with narrow_valu8 on -- those inside
    the float32 vector section, which split nothing."""
    return tuple(st for st in scn.whole if not (v8 and site_in_v8(plan, st)))


@functools.lru_cache(maxsize=None)
def data(name, B, T):
    """The seeded inputs of tests/test_gpu_envelope.py for config `name` at B rows (read only): cond, start state, injected noise, per-row
    t, mask, and the training step's y / ts / noise.  Here so that tests/test_envelope_cpu.py can prove the scenarios on the very rows."""
    from weights import CONFIGS
    cfg = CONFIGS[name]
    D, C = cfg["input_dim"], cfg["cond_dim"]
    g = torch.Generator().manual_seed(100 + B)
    d = dict(cond=torch.rand(B, C, generator=g), y_T=torch.randn(B, D, generator=g), z=torch.randn(T - 2, B, D, generator=g),
             t=torch.rand(1, B, generator=g), mask=(torch.rand(B, 1, generator=g) < 0.7).float(),
             y=torch.rand(B, D, generator=g), ts=torch.randint(0, T, (1, B), generator=g), noise=torch.randn(B, D, generator=g))
    d["mask"][-1] = 1.0
    return d


def call_inputs(scn, d, T, kind, omega=1.0):
    """[(network input x [B, D], t [1, B], cond, mask [B, 1])] of every denoiser pass one call of `kind` makes under scenario `scn` on data
    `d`, from the float32 oracle: both passes of every reverse step, the one forward, or the training step's x_t."""
    cond, B = d["cond"], d["cond"].shape[0]
    if kind == "forward":
        return [(apply_y(scn, d["y_T"]), d["t"], cond, d["mask"])]
    bufs = O.schedule_buffers(1.0 - O.cosine_betas(T))
    if kind == "train":
        sc = scn.y_scale if isinstance(scn, LowScenario) and scn.y_scale is not None else 1.0
        return [(O.q_sample(bufs, d["y"] * sc, d["ts"], d["noise"] * sc).reshape(B, -1), d["ts"] / T, cond, d["mask"])]
    out, y = [], apply_y(scn, d["y_T"])
    with torch.no_grad():
        for k, i in enumerate(range(T - 1, -1, -1)):
            t = (torch.full((1, B), i, dtype=torch.int64) / T).to(y.dtype)
            out += [(y, t, cond, torch.zeros(B, 1)), (y, t, cond, torch.ones(B, 1))]
            y, _ = O.sample_step(scn.params, scn_plan(scn), bufs, T, i, y, cond, omega, d["z"][k] if i > 1 else 0)
    return out


def scn_plan(scn):
    from weights import CONFIGS
    cfg = CONFIGS[scn.name.split(":")[0]]
    return O.unet_plan(cfg["input_dim"], cfg["proj_dim"], cfg["cond_dim"], cfg["dims"], cfg["n_blocks"])


def apply_y(scn, y):
    """`y` with the scenario's element set (the `y` scenario: feature j of the last row becomes A); other scenarios leave it alone."""
    if isinstance(scn, LowScenario):
        return y if scn.y_scale is None else y * scn.y_scale
    if scn.y_col is None:
        return y
    y = y.clone()
    y[-1, scn.y_col] = scn.A
    return y


def raw_bounds(plan, taps, y):
    """{site: (max over rows of |mean| + sqrt(M2), max|x|)} in float64 for every raw read, from the taps of one `unet_forward` call on `y`:
    what the kernel at that site compares with kRawLimit (feature_proj compares max|x| itself), over the concatenated row for a shortcut."""
    out = OrderedDict()
    for r in raw_reads(plan):
        x = torch.cat([(y if n == "y" else taps[n]).double() for n in r.tensors], dim=1)
        mean = x.mean(dim=1, keepdim=True)
        m2 = ((x - mean) ** 2).sum(dim=1)
        out[r.site] = (float((mean[:, 0].abs() + m2.sqrt()).max()), float(x.abs().max()))
    return out


def raw_bounds_min(plan, taps, y, rows=None):
    """{site: (min over rows of the quantity the kernel at that site compares with kRawFloor, max over rows of it)} in float64: the row's
    max|x| for feature_proj, |mean| + sqrt(M2) over the concatenated row elsewhere.  All-zero rows are left out, as the kernels leave them
    out (a bound of exactly 0 raises nothing); `rows` restricts the survey to a subset of the batch."""
    out = OrderedDict()
    for r in raw_reads(plan):
        x = torch.cat([(y if n == "y" else taps[n]).double() for n in r.tensors], dim=1)
        if rows is not None:
            x = x[rows]
        if r.site == "feature_proj":
            b = x.abs().amax(dim=1)
        else:
            mean = x.mean(dim=1, keepdim=True)
            b = mean[:, 0].abs() + ((x - mean) ** 2).sum(dim=1).sqrt()
        b = b[b > 0]
        out[r.site] = (float(b.min()), float(b.max())) if b.numel() else (float("inf"), 0.0)
    return out


def _merge(acc, bounds):
    for k, (lo, hi) in bounds.items():
        a = acc.get(k, (float("inf"), 0.0))
        acc[k] = (min(a[0], lo), max(a[1], hi))
    return acc


def _padded(x, t, cond, mask):
    """The rows of one denoiser pass plus a PADDING row -- y = 0, cond = 0, the last row's t and mask: what the ragged last tile of a
    launch computes in its unused rows, which the kernels bound like any other row."""
    pad = lambda a: torch.cat([a, torch.zeros(1, a.shape[1], dtype=a.dtype)])       # noqa: E731
    return pad(x), torch.cat([t, t[:, -1:]], dim=1), pad(cond), torch.cat([mask, mask[-1:]])


def survey_sample(p, plan, T, cond, omega, y_T, z):
    """`raw_bounds_min` over both denoiser passes of every step of the float32 oracle's reverse loop (z: [>= T - 2, B, D]), each pass
    with a padding row."""
    bufs, acc, y, B = O.schedule_buffers(1.0 - O.cosine_betas(T)), {}, y_T, cond.shape[0]
    with torch.no_grad():
        for k, i in enumerate(range(T - 1, -1, -1)):
            t = (torch.full((1, B), i, dtype=torch.int64) / T).to(y.dtype)
            for m in (0.0, 1.0):
                taps = {}
                yp, tp, cp, mp = _padded(y, t, cond, torch.full((B, 1), m))
                O.unet_forward(p, plan, yp, tp, cp, mp, taps=taps)
                _merge(acc, raw_bounds_min(plan, taps, yp))
            y, _ = O.sample_step(p, plan, bufs, T, i, y, cond, omega, z[k] if i > 1 else 0)
    return acc


def survey_train(p, plan, T, y, cond, ts, noise, mask):
    """`raw_bounds_min` of one training forward of the float32 oracle, with a padding row."""
    bufs = O.schedule_buffers(1.0 - O.cosine_betas(T))
    x_t = O.q_sample(bufs, y, ts, noise).reshape(y.shape[0], -1)
    taps = {}
    xp, tp, cp, mp = _padded(x_t, ts / T, cond, mask)
    with torch.no_grad():
        O.unet_forward(p, plan, xp, tp, cp, mp, taps=taps)
    return raw_bounds_min(plan, taps, xp)


def rel(a, b):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64)
    b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _dbl(d):
    return {k: v.double() for k, v in d.items()}


def oracle_sample(p, plan, T, cond, omega, y_T, z, f64):
    """The oracle's reverse loop on injected noise z (T-2, B, D), in float32 or float64."""
    bufs = O.schedule_buffers(1.0 - O.cosine_betas(T))
    zd = {i: z[k] for k, i in enumerate(range(T - 1, 1, -1))}
    with torch.no_grad():
        if f64:
            return O.ddpm_sample(_dbl(p), plan, _dbl(bufs), T, cond.double(), omega, y_T.double(), _dbl(zd))
        return O.ddpm_sample(p, plan, bufs, T, cond, omega, y_T, zd)


def oracle_forward(p, plan, x, t, cond, mask, f64):
    with torch.no_grad():
        if f64:
            return O.unet_forward(_dbl(p), plan, x.double(), t.double(), cond.double(), mask.double())
        return O.unet_forward(p, plan, x, t, cond, mask)


def oracle_loss64(p, plan, T, y, cond, ts, noise, mask):
    """The oracle's training loss in float64 (float32-valued parameters, buffers and inputs), as `ddpm_loss_and_grads(f64=True)` forms it."""
    b64 = _dbl(O.schedule_buffers(1.0 - O.cosine_betas(T)))
    with torch.no_grad():
        y_t = O.q_sample(b64, y.double(), ts, noise.double())
        eps = O.unet_forward(_dbl(p), plan, y_t, (ts / T).double(), cond.double(), mask.double())
        return torch.nn.functional.mse_loss(noise.double(), eps)


def in_range_budget(p, plan, T, cond, omega, y_T, z):
    """(float64 result, the oracle's own float32-vs-float64 relative error) of a sampling call under parameters `p`: the budget an
    accuracy bound may add to TOL (x3, as test_sample_large_launch_vs_oracle does) -- computed by the oracle, never by the code under test."""
    ref64 = oracle_sample(p, plan, T, cond, omega, y_T, z, True)
    return ref64, rel(oracle_sample(p, plan, T, cond, omega, y_T, z, False), ref64)
