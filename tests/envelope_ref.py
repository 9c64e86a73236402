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


def apply_y(scn, y):
    """`y` with the scenario's element set (the `y` scenario: feature j of the last row becomes A); other scenarios leave it alone."""
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
