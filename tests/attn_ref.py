"""UNet1D with AttentionBlocks: configurations, deterministic weights and a torch-CPU restatement, shared by
tests/golden/make_attn_goldens.py and the attention tests.

`oracle/` has no attention, so the expected values of the attention tests come from the reference itself
(tests/golden/g13_attn_*.npz, written by make_attn_goldens.py).  The restatement below composes the oracle's
`residual_block`, `_lin` and `time_embedding` with the closed form of the reference's AttentionBlock on a sequence of
length 1 (UNetCF.py:98-157: the softmax over one key is identically 1, `norm` is never called):

    v   = Wv x + bv            Wv / bv = rows 2d:3d of `projection`
    out = output(v) + x

It is used as the reference at shapes the goldens do not cover, and only after test_attention_gpu has checked it
against the reference-generated golden at the golden's shape with max|diff| = 0.

Weights are never stored in the fixtures (config "wide" alone has ~1 M floats, a committed file holds 1 MiB): as for the
other goldens (tests/golden/weights.py) they are regenerated from numpy.random.RandomState(seed); the fixtures record the
seed and per-tensor float64 checksums of what the generator used.
"""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ddpm_oracle as O

ATTN_CONFIGS = {
    # NU-like: attention at 32 / 16 (down), 8 (extra down, middle), 8 / 16 (up); none at the first resolution and at proj_dim
    "nu": dict(input_dim=5, proj_dim=32, cond_dim=6, dims=(32, 16, 8), n_blocks=2, is_attn=(False, True, True), middle_attn=True),
    # wide: 128- and 64-wide attention (both precision modes of the >= 64-wide kernels), 32-wide at the bottom
    "wide": dict(input_dim=4, proj_dim=128, cond_dim=3, dims=(64, 32), n_blocks=1, is_attn=(True, True), middle_attn=False),
}
WEIGHT_SEED = 61


def attn_plan(cfg):
    """The oracle's plan plus, per down / up entry, whether the block carries an AttentionBlock (UNetCF.py:278-311: is_attn[i]
    for every block of resolution i; the extra blocks behind the loops use the loop's final i)."""
    plan = O.unet_plan(cfg["input_dim"], cfg["proj_dim"], cfg["cond_dim"], cfg["dims"], cfg["n_blocks"])
    ia, nb, nres = cfg["is_attn"], cfg["n_blocks"], len(cfg["dims"])
    down, up = [], []
    for i in range(nres):
        down += [ia[i]] * nb + [False]
        if i == nres - 1:
            down += [ia[i]] * nb
    for i in reversed(range(nres)):
        up += [ia[i]] * (nb + 1) + [False]
        if i == 0:
            up += [ia[i]] * (nb + 1)
    assert len(down) == len(plan["down"]) and len(up) == len(plan["up"])
    plan = dict(plan, down_attn=down, up_attn=up, middle_attn=bool(cfg["middle_attn"]))
    return plan


def attn_shapes(plan):
    """State-dict keys and shapes in registration order: the oracle's table with `<block>.attn.{norm,projection,output}`
    behind `<block>.res.*` (middle: between res1 and res2)."""
    base = O.state_shapes(plan)
    width = {}
    for idx, (kind, _, o) in enumerate(plan["down"]):
        if plan["down_attn"][idx]:
            width[f"down.{idx}"] = o
    for idx, (kind, _, o) in enumerate(plan["up"]):
        if plan["up_attn"][idx]:
            width[f"up.{idx}"] = o
    out = OrderedDict()

    def attn(prefix, d):
        out[prefix + ".norm.weight"] = (d,); out[prefix + ".norm.bias"] = (d,)
        out[prefix + ".projection.weight"] = (3 * d, d); out[prefix + ".projection.bias"] = (3 * d,)
        out[prefix + ".output.weight"] = (d, d); out[prefix + ".output.bias"] = (d,)

    keys = list(base)
    for n, k in enumerate(keys):
        if k == "middle.res2.norm1.weight" and plan["middle_attn"]:
            attn("middle.attn", plan["mid_w"])
        out[k] = base[k]
        nxt = keys[n + 1] if n + 1 < len(keys) else ""
        blk = k.split(".res.")[0]
        if ".res." in k and blk in width and not nxt.startswith(blk + ".res."):
            attn(blk + ".attn", width[blk])
    return out


def attn_weights(shapes, seed=WEIGHT_SEED):
    """The "trained" flavour of weights.synth_weights (activations stay O(1)); the attention Linears' weights ~ N(0, 0.1^2), so that
    Wo Wv is far from negligible beside the identity of the residual at every width."""
    from weights import synth_weights
    w = synth_weights(shapes, seed, "trained")
    rs = np.random.RandomState(seed + 1)
    for k, shape in shapes.items():
        if ".attn." in k and k.endswith(".weight") and ".norm." not in k:
            w[k] = np.ascontiguousarray(0.1 * rs.standard_normal(shape), dtype=np.float32)
    return w


def attn_params(name, seed=WEIGHT_SEED):
    cfg = ATTN_CONFIGS[name]
    plan = attn_plan(cfg)
    return plan, OrderedDict((k, torch.from_numpy(v)) for k, v in attn_weights(attn_shapes(plan), seed).items())


def checksums(p):
    return (np.array([float(torch.as_tensor(v).double().sum()) for v in p.values()]),
            np.array([float(torch.as_tensor(v).double().abs().sum()) for v in p.values()]))


def attention(p, prefix, x):
    """Two GEMMs, then the residual add."""
    d = x.shape[-1]
    v = F.linear(x, p[prefix + ".projection.weight"][2 * d:], p[prefix + ".projection.bias"][2 * d:])
    out = F.linear(v, p[prefix + ".output.weight"], p[prefix + ".output.bias"])
    out += x
    return out


def unet_forward(p, plan, x, t, cond, cond_mask):
    """oracle.ddpm_oracle.unet_forward with the attention operators in place (UNetCF.py:318-356)."""
    temb = O.time_embedding(p, t, plan["time_dim"])
    x = O._lin(p, "feature_proj", x)
    cond = cond * cond_mask
    skips = [x]
    for idx, (kind, _, _) in enumerate(plan["down"]):
        if kind == "res":
            x = O.residual_block(p, f"down.{idx}.res", x, temb, cond)
            if plan["down_attn"][idx]:
                x = attention(p, f"down.{idx}.attn", x)
        else:
            x = O._lin(p, f"down.{idx}.lin", x)
        skips.append(x)
    x = O.residual_block(p, "middle.res1", x, temb, cond)
    if plan["middle_attn"]:
        x = attention(p, "middle.attn", x)
    x = O.residual_block(p, "middle.res2", x, temb, cond)
    for idx, (kind, _, _) in enumerate(plan["up"]):
        if kind == "lin":
            x = O._lin(p, f"up.{idx}.lin", x)
        else:
            x = torch.cat((x, skips.pop()), dim=1)
            x = O.residual_block(p, f"up.{idx}.res", x, temb, cond)
            if plan["up_attn"][idx]:
                x = attention(p, f"up.{idx}.attn", x)
    return O._lin(p, "final", O.swish(O._ln(p, "norm", x)))


def loss_and_grads(p, plan, bufs, T, y, cond, ts, noise, cond_mask, f64=False):
    """oracle.ddpm_oracle.ddpm_loss_and_grads on this forward; unused tensors (attn.norm) get zeros."""
    dt = torch.float64 if f64 else torch.float32
    leaf = OrderedDict((k, v.detach().to(dt).clone().requires_grad_(True)) for k, v in p.items())
    b = {k: v.to(dt) for k, v in bufs.items()}
    y_t = O.q_sample(b, y.to(dt), ts, noise.to(dt))
    eps_hat = unet_forward(leaf, plan, y_t, (ts / T).to(dt), cond.to(dt), cond_mask.to(dt))
    loss = F.mse_loss(noise.to(dt), eps_hat)
    grads = torch.autograd.grad(loss, list(leaf.values()), allow_unused=True)
    return loss.detach(), OrderedDict((k, (g if g is not None else torch.zeros_like(v))) for (k, v), g in zip(leaf.items(), grads))


@torch.no_grad()
def sample(p, plan, bufs, T, cond, omega, y_T, noises):
    """oracle.ddpm_oracle.ddpm_sample on this forward (MSR.py:114-155)."""
    B = cond.shape[0]
    y_t = y_T
    acp = bufs["alphas_cumprod"]
    for i in range(T - 1, -1, -1):
        z = noises[i] if i > 1 else 0
        t = (torch.full((1, B), i, dtype=torch.int64) / T).to(y_t.dtype)
        eps0 = unet_forward(p, plan, y_t, t, cond, torch.zeros(B, 1, dtype=y_t.dtype))
        eps1 = unet_forward(p, plan, y_t, t, cond, torch.ones(B, 1, dtype=y_t.dtype))
        eps = (1 + omega) * eps1 - omega * eps0
        y_t = (y_t - bufs["betas"][i] / bufs["sqrt_one_minus_alphas_cumprod"][i] * eps) * bufs["reciprocal_sqrt_alphas"][i] \
            + (1.0 - acp[i - 1 if i - 1 >= 0 else 0]) / (1.0 - acp[i]) * z
        if i > T - 5:
            y_t = (y_t - torch.mean(y_t)) / torch.sqrt(torch.var(y_t))
    return y_t
