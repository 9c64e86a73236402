#!/usr/bin/env python3
"""Generate tests/golden/g13_attn_<config>.npz by importing the reference itself (UNet1D with is_attn / middle_attn).

Runs ONLY in the build container (needs /root/reference); the outputs are committed.  Nothing here is imported by the tests.

    python tests/golden/make_attn_goldens.py

Per configuration of tests/attn_ref.py (ATTN_CONFIGS):
  keys / shapes ......... the reference's state-dict layout (JSON in `layout`)
  seed_sums / seed_abs .. per-tensor float64 checksums of torch.manual_seed(5); UNet1D(...); apply(init_weights)
  w_seed, w_sums, w_abs . the weights of every run below are attn_ref.attn_weights(shapes, w_seed) -- a seeded state with the
                          attention Linears at 0.1 std, so that Wo Wv is not negligible -- and are NOT stored (1 MiB per committed
                          file; the tests regenerate them and compare these checksums)
  x, cond, a_*, b_*, c_*  UNet1D.forward inputs and outputs (as G2 of make_goldens.py)
  t_*  .................. DDPM.forward: draws, loss and every gradient (None recorded as zeros) -- in full for the small
                          configuration, as float64 norm + first 16 elements per tensor for the wide one (as G3)
  s_*  .................. DDPM.sample with injected y_T and noises, T = 6, omega in {0, 1}
"""
import json
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
for p_ in (REF, HERE, os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p_)
os.chdir(os.path.join(REF, "ddpm_opt"))

from ddpm_opt.diffusion import generate_cosine_schedule, init_weights  # noqa: E402
from ddpm_opt.UNetCF import UNet1D  # noqa: E402
import ddpm_opt.classifier_free_MSR as RMSR  # noqa: E402
import attn_ref as AR  # noqa: E402

torch.set_num_threads(8)


def ref_unet(cfg):
    return UNet1D(input_dim=cfg["input_dim"], proj_dim=cfg["proj_dim"], cond_dim=cfg["cond_dim"], dims=cfg["dims"],
                  is_attn=cfg["is_attn"], middle_attn=cfg["middle_attn"], n_blocks=cfg["n_blocks"])


def replay_sample_noise(seed, B, D, T):
    torch.manual_seed(seed)
    y_T = torch.randn(B, 1, D).squeeze()
    z = {}
    for i in range(T - 1, -1, -1):
        if i > 1:
            z[i] = torch.randn(B, 1, D).squeeze()
    return y_T, z


def main():
    for name, cfg in AR.ATTN_CONFIGS.items():
        out = {}
        D, C = cfg["input_dim"], cfg["cond_dim"]
        # ---- layout and seeded construction
        torch.manual_seed(5)
        m = ref_unet(cfg)
        m.apply(init_weights)
        sd = m.state_dict()
        out["layout"] = np.array(json.dumps([[k, list(v.shape)] for k, v in sd.items()]))
        out["seed_sums"] = np.array([float(v.double().sum()) for v in sd.values()])
        out["seed_abs"] = np.array([float(v.double().abs().sum()) for v in sd.values()])
        # ---- the weights of every run below
        shapes = {k: tuple(v.shape) for k, v in sd.items()}
        w = {k: torch.from_numpy(v) for k, v in AR.attn_weights(shapes, AR.WEIGHT_SEED).items()}
        out["w_seed"] = np.int64(AR.WEIGHT_SEED)
        out["w_sums"], out["w_abs"] = AR.checksums(w)
        model = ref_unet(cfg)
        model.load_state_dict(w, strict=True)
        # ---- UNet1D.forward
        B = 48
        rs = np.random.RandomState(1300)
        x = torch.from_numpy(rs.standard_normal((B, D)).astype(np.float32))
        cond = torch.from_numpy(rs.uniform(0, 1, (B, C)).astype(np.float32))
        ts = torch.from_numpy(rs.randint(0, 20, (1, B)).astype(np.int64))
        mask = torch.from_numpy((rs.uniform(0, 1, (B, 1)) < 0.7).astype(np.float32))
        t7 = torch.full((1, B), 7, dtype=torch.int64) / 20
        with torch.no_grad():
            out.update(x=x.numpy(), cond=cond.numpy(), a_ts=ts.numpy(), a_T=np.int64(20), a_mask=mask.numpy(), b_step=np.int64(7))
            out["a_eps"] = model(x, ts / 20, cond, mask).numpy()
            out["b_eps"] = model(x, t7, cond, torch.zeros(B, 1)).numpy()
            out["c_eps"] = model(x, t7, cond, torch.ones(B, 1)).numpy()
            # the restatement the tests use at other shapes, against the reference right here
            plan = AR.attn_plan(cfg)
            d_ = float((AR.unet_forward(w, plan, x, ts / 20, cond, mask) - torch.from_numpy(out["a_eps"])).abs().max())
            print(f"{name}: attn_ref.unet_forward vs the reference: max|diff| = {d_:.3e}")
        # ---- DDPM.forward
        T = 20
        alphas = 1.0 - generate_cosine_schedule(T)
        ddpm = RMSR.DDPM(T, ref_unet(cfg), D, 10.0, alphas, torch.device("cpu"), (1, D), None, 0.1, 0.9999, 10, 5, False)
        ddpm.model.load_state_dict(w, strict=True)
        y = torch.from_numpy(rs.uniform(0, 1, (B, D)).astype(np.float32))
        tc = torch.from_numpy(rs.uniform(0, 1, (B, C)).astype(np.float32))
        seed = 4321
        torch.manual_seed(seed)
        random.seed(0)   # keeps the debug print (MSR.py:110) quiet
        loss = ddpm(y, tc)
        loss.backward()
        torch.manual_seed(seed)        # the three draws, replayed in the reference's order (MSR.py:101,102,107)
        dts = torch.randint(low=0, high=T, size=(1, B))
        noise = torch.randn_like(y)
        dmask = torch.bernoulli(torch.fill(torch.zeros(B), 1 - 0.1))[:, None]
        out.update(t_y=y.numpy(), t_cond=tc.numpy(), t_ts=dts.numpy(), t_noise=noise.numpy(), t_mask=dmask.numpy(),
                   t_loss=loss.detach().numpy(), t_T=np.int64(T))
        none = []
        full = sum(v.numel() for v in sd.values()) * 4 < 600 * 1024
        out["t_full"] = np.int64(1 if full else 0)
        for k, p_ in ddpm.model.named_parameters():
            if p_.grad is None:
                none.append(k)
            g = (p_.grad if p_.grad is not None else torch.zeros_like(p_)).detach().numpy()
            if full:
                out["t_grad." + k] = g
            else:
                out["t_gradnorm." + k] = np.float64(np.sqrt((g.astype(np.float64) ** 2).sum()))
                out["t_gradhead." + k] = g.reshape(-1)[:16].copy()
                if ".attn.projection." in k:       # the q / k rows: recorded as what they are
                    out["t_gradqk_absmax." + k] = np.float64(np.abs(g[: 2 * g.shape[0] // 3]).max())
        out["t_none"] = np.array(json.dumps(none))
        # ---- DDPM.sample
        T = 6
        B = 40
        alphas = 1.0 - generate_cosine_schedule(T)
        ddpm = RMSR.DDPM(T, ref_unet(cfg), D, 10.0, alphas, torch.device("cpu"), (1, D), None)
        ddpm.model.load_state_dict(w, strict=True)
        scond = torch.from_numpy(rs.uniform(0, 1, (B, C)).astype(np.float32))
        seed = 77
        y_T, z = replay_sample_noise(seed, B, D, T)
        out.update(s_cond=scond.numpy(), s_y_T=y_T.numpy(), s_T=np.int64(T), s_z=np.stack([z[i].numpy() for i in range(T - 1, 1, -1)]))
        with torch.no_grad():
            for omega in (0.0, 1.0):
                torch.manual_seed(seed)
                out[f"s_om{omega:g}_y0"] = ddpm.sample(scond, omega).numpy()
        path = os.path.join(HERE, f"g13_attn_{name}.npz")
        np.savez_compressed(path, **out)
        print(f"wrote g13_attn_{name}.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays, "
              f"{sum(v.numel() for v in sd.values())} parameters, grads None: {len(none)}")


if __name__ == "__main__":
    main()
