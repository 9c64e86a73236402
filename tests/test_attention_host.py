"""UNet1D(is_attn=..., middle_attn=...) on the host: module tree, state-dict layout and seeded construction against the
reference's own (tests/golden/g13_attn_*.npz, tests/golden/make_attn_goldens.py).  No GPU needed."""
import json

import numpy as np
import pytest
import torch

import attn_ref as AR
from oracle import ddpm_oracle as O
from weights import CONFIGS

NAMES = sorted(AR.ATTN_CONFIGS)


def layout_of(g):
    return [(k, tuple(s)) for k, s in json.loads(str(g["layout"]))]


@pytest.mark.parametrize("name", NAMES)
def test_seeded_construction_gives_the_reference_layout_and_initial_weights(gold, name):
    from diffsg_amd import UNet1D, init_weights
    g = gold(f"g13_attn_{name}.npz")
    torch.manual_seed(5)
    m = UNet1D(**AR.ATTN_CONFIGS[name])
    m.apply(init_weights)
    sd = m.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == layout_of(g)
    sums = np.array([float(v.double().sum()) for v in sd.values()])
    absum = np.array([float(v.double().abs().sum()) for v in sd.values()])
    assert np.array_equal(sums, g["seed_sums"]) and np.array_equal(absum, g["seed_abs"])


@pytest.mark.parametrize("name", NAMES)
def test_reference_state_loads_strict(gold, name):
    from diffsg_amd import UNet1D
    g = gold(f"g13_attn_{name}.npz")
    plan, p = AR.attn_params(name, int(g["w_seed"]))
    assert [(k, tuple(v.shape)) for k, v in p.items()] == layout_of(g)        # the reference's keys, order and shapes
    sums, absum = AR.checksums(p)
    assert np.array_equal(sums, g["w_sums"]) and np.array_equal(absum, g["w_abs"])   # ... and the weights the goldens were made with
    m = UNet1D(**AR.ATTN_CONFIGS[name])
    m.load_state_dict(p, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, p[k]), k


@pytest.mark.parametrize("name", NAMES)
def test_flag_to_block_placement(gold, name):
    """is_attn[i] reaches every Down / UpBlock of resolution i; the extra blocks at the last width (down) and at proj_dim (up)
    take the loop's final i; `attn` is registered behind `res` (middle: between res1 and res2)."""
    from diffsg_amd import UNet1D
    from diffsg_amd.UNetCF import DownBlock, UpBlock
    g = gold(f"g13_attn_{name}.npz")
    cfg = AR.ATTN_CONFIGS[name]
    m = UNet1D(**cfg)
    plan = AR.attn_plan(cfg)
    assert [hasattr(b, "attn") for b in m.down] == plan["down_attn"]
    assert [hasattr(b, "attn") for b in m.up] == plan["up_attn"]
    assert hasattr(m.middle, "attn") == cfg["middle_attn"]
    assert all(isinstance(b, DownBlock) == (k == "res") for b, (k, _, _) in zip(m.down, plan["down"]))
    assert all(isinstance(b, UpBlock) == (k == "res") for b, (k, _, _) in zip(m.up, plan["up"]))
    keys = [k for k, _ in layout_of(g)]
    assert list(m.state_dict()) == keys
    golden_blocks = sorted({k.split(".attn.")[0] for k in keys if ".attn." in k})
    want = sorted([f"down.{i}" for i, a in enumerate(plan["down_attn"]) if a] + [f"up.{i}" for i, a in enumerate(plan["up_attn"]) if a] +
                  (["middle"] if cfg["middle_attn"] else []))
    assert golden_blocks == want
    n = cfg["n_blocks"]
    nres = len(cfg["dims"])
    # the extra blocks: the last n down blocks and the last n + 1 up blocks
    assert plan["down_attn"][-n:] == [cfg["is_attn"][nres - 1]] * n and plan["up_attn"][-(n + 1):] == [cfg["is_attn"][0]] * (n + 1)
    assert m.cfg["is_attn"] == tuple(cfg["is_attn"]) and m.cfg["middle_attn"] == cfg["middle_attn"]
    for k in keys:
        if ".attn." in k:
            blk = k.split(".attn.")[0]
            first_attn = keys.index(blk + ".attn.norm.weight")
            res_keys = [i for i, q in enumerate(keys) if q.startswith(blk + (".res1." if blk == "middle" else ".res."))]
            assert first_attn == max(res_keys) + 1


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_without_flags_nothing_changes(name):
    """All flags false (explicitly, or by the default): the state dict is the one the oracle's table describes, no `attn` anywhere."""
    from diffsg_amd import UNet1D
    cfg = CONFIGS[name]
    plan = O.unet_plan(cfg["input_dim"], cfg["proj_dim"], cfg["cond_dim"], cfg["dims"], cfg["n_blocks"])
    want = [(k, tuple(s)) for k, s in O.state_shapes(plan).items()]
    for kw in (dict(is_attn=(False,) * len(cfg["dims"])), dict(is_attn=(False,) * len(cfg["dims"]), middle_attn=False), dict()):
        torch.manual_seed(3)
        m = UNet1D(**cfg, **kw)
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == want
        assert not any(".attn." in k for k in m.state_dict())
        assert not any(m.cfg["is_attn"]) and m.cfg["middle_attn"] is False
        assert {k: m.cfg[k] for k in cfg} == {k: (tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in cfg.items()}


def test_a_short_flag_list_with_a_flag_set_is_refused():
    from diffsg_amd import UNet1D
    with pytest.raises(ValueError):
        UNet1D(input_dim=3, proj_dim=16, cond_dim=3, dims=(16, 8, 8, 8), is_attn=(True, False, False))


@pytest.mark.parametrize("field,limit", [("input_dim", 128), ("cond_dim", 4096)])
def test_each_size_limit_of_the_descriptor_is_refused_under_its_own_name(field, limit):
    """dsg_create checks the descriptor before it looks for a device: input_dim > 128 and cond_dim > 4096 are refused, each with a message
    that names the field, the value and the limit (cond_dim used to be reported as "input_dim > 128")."""
    import ctypes
    from diffsg_amd import _lib
    L = _lib.lib()
    d = _lib.UNetDesc()
    d.input_dim, d.proj_dim, d.cond_dim, d.n_blocks, d.n_res = 3, 16, 3, 1, 1
    d.dims[0] = 8
    setattr(d, field, limit + 1)
    assert not L.dsg_create(ctypes.byref(d))
    msg = L.dsg_last_error().decode()
    other = "cond_dim" if field == "input_dim" else "input_dim"
    assert field in msg and str(limit + 1) in msg and str(limit) in msg and other not in msg, msg
    setattr(d, field, limit)                     # the limit itself passes the descriptor checks (what stops it without a GPU is the device)
    hd = L.dsg_create(ctypes.byref(d))
    if hd:
        L.dsg_destroy(hd)
    else:
        assert "no HIP device" in L.dsg_last_error().decode()


@pytest.mark.parametrize("name", NAMES)
def test_cpu_restatement_is_the_reference(gold, name):
    """attn_ref (the oracle's pieces + the two-GEMM closed form) IS the reference at the golden's shape, max|diff| = 0, for the forward,
    the sampling loop and the loss: only then do the GPU tests use it as the reference at other shapes."""
    g = gold(f"g13_attn_{name}.npz")
    plan, p = AR.attn_params(name, int(g["w_seed"]))
    t = lambda k: torch.from_numpy(g[k])
    B = g["x"].shape[0]
    t7 = torch.full((1, B), int(g["b_step"]), dtype=torch.int64) / 20
    with torch.no_grad():
        assert torch.equal(AR.unet_forward(p, plan, t("x"), t("a_ts") / int(g["a_T"]), t("cond"), t("a_mask")), t("a_eps"))
        assert torch.equal(AR.unet_forward(p, plan, t("x"), t7, t("cond"), torch.zeros(B, 1)), t("b_eps"))
        assert torch.equal(AR.unet_forward(p, plan, t("x"), t7, t("cond"), torch.ones(B, 1)), t("c_eps"))
    T = int(g["s_T"])
    bufs = O.schedule_buffers(1.0 - O.cosine_betas(T))
    z = t("s_z")
    for omega in (0.0, 1.0):
        y0 = AR.sample(p, plan, bufs, T, t("s_cond"), omega, t("s_y_T"), {i: z[j] for j, i in enumerate(range(T - 1, 1, -1))})
        assert torch.equal(y0, t(f"s_om{omega:g}_y0"))
    T = int(g["t_T"])
    loss, grads = AR.loss_and_grads(p, plan, O.schedule_buffers(1.0 - O.cosine_betas(T)), T, t("t_y"), t("t_cond"), t("t_ts"), t("t_noise"), t("t_mask"))
    assert float(loss) == float(g["t_loss"])
    none = json.loads(str(g["t_none"]))
    assert none and all(".attn.norm." in k for k in none)
    for k, v in grads.items():
        if k in none:
            assert not v.any(), k
        elif int(g["t_full"]):
            assert torch.equal(v, t("t_grad." + k)), k
        else:
            assert torch.equal(v.reshape(-1)[:16], t("t_gradhead." + k)), k
        if ".attn.projection." in k:
            assert not v[: 2 * v.shape[0] // 3].any(), k
