"""Writes tests/golden/g20_launch_preamble.npz: y_0 of small MSR-80c sampling calls through the persistent wide kernels, as the build
of the commit BEFORE the launch-preamble change computes them on an MI355X.  tests/test_gpu_launch_preamble.py compares
the tree under test with these bits (`torch.equal`), so the file is generated ONCE, from a checkout and build of that parent commit:

    git archive <parent> | tar -x -C ab_old && cp tests/golden/make_g20_launch_preamble.py ab_old/tests/golden/
    (cd ab_old && python -c "import __graft_entry__ as g; g.build()" && python tests/golden/make_g20_launch_preamble.py OUT.npz)

Never regenerate it from the tree under test.  Cases: rows x omega x panel_half at T = 6 (four renorm steps run eagerly, two from the
graph; every step has its own time-bias row), net and inputs as tests/test_gpu_cfg_share.py.  Where both panel_half settings give the
same bits (they run the same arithmetic in the same order) the array is stored once, as `..._h`; otherwise as `..._h0` and `..._h1`."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

T = 6
ROWS = (32, 100, 160, 295)
OMEGAS = (1.0, 0.3)
HALVES = (1, 0)
SEED = 7


def cond_of(B, seed=4):
    import torch
    return torch.rand(B, 80, generator=torch.Generator().manual_seed(seed)).cuda()


def key(B, omega, half=None):
    return f"y0_B{B}_w{int(round(omega * 10)):02d}_h" + ("" if half is None else str(half))


def main():
    import numpy as np
    import torch
    import bench
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g20_launch_preamble.npz")
    ddpm = bench.build_model(torch.device("cuda:0"), T)
    ddpm.model.set_launch_policy(0, 0)          # the persistent forms at every size
    arrays = {}
    for B in ROWS:
        cond = cond_of(B)
        for omega in OMEGAS:
            got = {}
            for half in HALVES:
                ddpm.model.set_option("panel_half", half)
                y = ddpm.sample(cond, omega, seed=SEED)
                assert torch.isfinite(y).all()
                assert torch.equal(ddpm.sample(cond, omega, seed=SEED), y), (B, omega, half)     # the reference itself repeats
                got[half] = y.cpu().numpy()
            if np.array_equal(got[0], got[1]):
                arrays[key(B, omega)] = got[0]
            else:
                arrays[key(B, omega, 0)], arrays[key(B, omega, 1)] = got[0], got[1]
    assert not ddpm.model.range_exceeded()
    np.savez(out_path, **arrays)
    print(f"{out_path}: {len(arrays)} arrays, {os.path.getsize(out_path)} bytes: " + " ".join(sorted(arrays)))


if __name__ == "__main__":
    main()
