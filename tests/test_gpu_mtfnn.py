"""MTFNN baseline on the device: dsg_mlp_forward / dsg_mlp_loss_grad / dsg_mlp_train_epoch and diffsg_amd.mtfnn.

Goldens: tests/golden/g14_mtfnn.npz (torch on the CPU, the reference's class for the NU net; make_mtfnn_goldens.py asserts that no
ReLU of a golden case sits within float32 rounding of zero, so no tolerance below allows for a flipped mask).
All tests need an MI355X: run with `-m gpu`."""
import ctypes
import os

import numpy as np
import pytest
import torch

from _util import GOLD
import mtfnn_ref as MR

pytestmark = pytest.mark.gpu

TOL = 1e-5      # forward: max|a - b| / max|b|, the bar tests/test_gpu_parity.py holds the denoiser to
GTOL = 1e-4     # gradients, per tensor on the grad_errs scale
ATOL = 1e-3     # parameters after three Adam steps (rel), the bar of the project's three-step Adam test
NU32 = ((64, 64, 32, 16, 32, 34), 2)        # the NU net at K = 32: gradient and moments do not fit in LDS beside it (global-memory form)
# nets near the width limits, where the tile is lower than 64 rows (both keep gradient and moments in global memory)
WIDE = {"wide32": ((128, 64, 64, 128), 64),                 # P = 20 736, TR = 32
        "wide16": ((128, 64, 64, 64, 64, 128), 0)}          # P = 29 056, TR = 16


@pytest.fixture(scope="module")
def g14():
    return np.load(os.path.join(GOLD, "g14_mtfnn.npz"))


def rel(a, b):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64)
    b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def grad_errs(got, ref):
    """tests/test_gpu_parity.py's scale: max|got - ref| / max(max|ref_k|, 1e-3 * global max|ref|) per tensor."""
    gmax = max(float(np.abs(v).max()) for v in ref.values())
    return {k: float(np.abs(np.asarray(got[k], dtype=np.float64) - ref[k]).max()) / max(float(np.abs(ref[k]).max()), 1e-3 * gmax) for k in ref}


def build(case):
    from diffsg_amd import MTFNN, co_net, msr_net
    widths, _ = MR.CASES[case]
    ctor = MTFNN if case.startswith("nu") else (co_net if case.startswith("co") else msr_net)
    return ctor(widths[0], widths[-1])


def state(g14, case, tag):
    widths, _ = MR.CASES[case]
    if tag == "trained":
        return {k: g14[f"{case}.trained.w.{k}"] for k, _ in MR.shapes(widths)}
    from diffsg_amd import init_weights
    torch.manual_seed(int(g14[f"{case}.init.seed"]))
    m = build(case)
    m.apply(init_weights)
    return {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype).contiguous()


def desc_of(widths, n_sig):
    from diffsg_amd.mtfnn import mlp_desc
    return mlp_desc(widths, n_sig)


def adam_step(p, g, m, v, step, lr=MR.LR):
    from diffsg_amd import _lib
    _lib.check(_lib.lib().dsg_adam_step(_lib.ptr(p), _lib.ptr(g), _lib.ptr(m), _lib.ptr(v), p.numel(), lr, 0.9, 0.999, 1e-8, 0.0, 0, step,
                                        _lib.stream_ptr()))


FORWARD = [(c, t, MR.ROWS) for c in MR.CASES for t in ("init", "trained")] + [("nu3", "trained", r) for r in (1, 63, 257)]


@pytest.mark.parametrize("case,tag,rows", FORWARD)
def test_forward_against_goldens(g14, case, tag, rows):
    """Measured on an MI355X: 6.1e-08 .. 4.8e-07 over the eleven cases (worst: msr80.trained at 104 rows, 4.82e-07); the bar is 1e-5."""
    from diffsg_amd.mtfnn import forward_flat
    widths, n_sig = MR.CASES[case]
    X, _ = MR.inputs(case)
    idx = np.arange(rows) % MR.ROWS                 # 257 rows: the golden rows again (a fifth tile, short)
    got = forward_flat(desc_of(widths, n_sig), dev(MR.flat(state(g14, case, tag), widths)), dev(X[idx]))
    err = rel(got, g14[f"{case}.{tag}.out"][idx])
    print(f"forward {case}.{tag} rows {rows}: {err:.2e}")
    assert got.shape == (rows, widths[-1])
    assert err < TOL


@pytest.mark.parametrize("tag", ["init", "trained"])
@pytest.mark.parametrize("case", list(MR.CASES))
def test_loss_and_gradients_against_goldens(g14, case, tag):
    """Measured on an MI355X: loss 6.4e-08 .. 3.8e-07 relative (bar 1e-5); worst gradient tensor per case 2.4e-07 .. 4.6e-07, and 1.47e-06
    for msr3.init (bar 1e-4)."""
    from diffsg_amd.mtfnn import loss_grad
    m = build(case)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state(g14, case, tag).items()}, strict=True)
    m.to("cuda")
    X, Y = MR.inputs(case)
    loss, grads = loss_grad(m, dev(X), dev(Y))
    want = float(g14[f"{case}.{tag}.loss"])
    ref = {k: g14[f"{case}.{tag}.grad.{k}"].astype(np.float64) for k in grads}
    errs = grad_errs({k: v.cpu().numpy() for k, v in grads.items()}, ref)
    print(f"loss_grad {case}.{tag}: loss rel {abs(loss.item() - want) / want:.2e}, worst grad tensor {max(errs.values()):.2e}")
    assert [tuple(v.shape) for v in grads.values()] == [s for _, s in MR.shapes(MR.CASES[case][0])]
    assert abs(loss.item() - want) < 1e-5 * want
    assert max(errs.values()) < GTOL, errs


@pytest.mark.parametrize("case", list(WIDE))
def test_forward_of_the_low_tile_nets(case):
    """Tiles of 32 and of 16 rows against the float64 restatement; a float32 emulation of the two nets (k in order, no FMA) is
    1.5e-7 and 3.0e-7 away from it.  Measured on an MI355X: 1.19e-07 (wide32) and 5.12e-07 (wide16); the bar is 1e-5."""
    from diffsg_amd.mtfnn import forward_flat
    widths, n_sig = WIDE[case]
    w, X, _ = synth_case(widths, 42, 0.1)
    got = forward_flat(desc_of(widths, n_sig), dev(MR.flat(w, widths)), dev(X))
    err = rel(got, MR.forward(w, widths, n_sig, X))
    print(f"forward {case} rows {MR.ROWS}: {err:.2e}")
    assert got.shape == (MR.ROWS, widths[-1])
    assert err < TOL


def compose(desc, p0, X, Y, perm, batch, step0=0, lr=MR.LR):
    """The epoch from dsg_mlp_loss_grad + dsg_adam_step, one batch at a time, on the gathered rows."""
    from diffsg_amd.mtfnn import loss_grad_flat
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    N, losses = perm.numel(), []
    for k, lo in enumerate(range(0, N, batch)):
        idx = perm[lo:lo + batch].long()
        loss, g = loss_grad_flat(desc, p, X[idx].contiguous(), Y[idx].contiguous())
        adam_step(p, g, m, v, step0 + k + 1, lr)
        losses.append(loss)
    return p, m, v, torch.stack(losses)


def synth_case(widths, seed, std):
    """(weights, X, Y): N(0, std^2) weights and uniform inputs and targets, seeded."""
    rs = np.random.RandomState(seed)
    X, Y = rs.uniform(0, 1, (MR.ROWS, widths[0])).astype(np.float32), rs.uniform(0, 1, (MR.ROWS, widths[-1])).astype(np.float32)
    return MR.synth_state(widths, seed, std), X, Y


def shaped_case(g14, case):
    """(desc, flat trained-like parameters, X, Y) of a golden case, or of the K = 32 NU net / a wide net on seeded inputs."""
    if case == "nu32":
        widths, n_sig = NU32
        w, X, Y = synth_case(widths, 32, 0.3)
    elif case in WIDE:
        widths, n_sig = WIDE[case]
        w, X, Y = synth_case(widths, 42, 0.1)
    else:
        widths, n_sig = MR.CASES[case]
        X, Y = MR.inputs(case)
        w = state(g14, case, "trained")
    return desc_of(widths, n_sig), dev(MR.flat(w, widths)), dev(X), dev(Y)


@pytest.mark.parametrize("batch", [64, 104, 512])
@pytest.mark.parametrize("case", ["co3", "msr80", "nu3", "nu32", "wide32", "wide16"])
def test_epoch_is_the_composition_bit_for_bit(g14, case, batch):
    from diffsg_amd.mtfnn import train_epoch_flat
    desc, p0, X, Y = shaped_case(g14, case)
    perm = torch.randperm(MR.ROWS, generator=torch.Generator().manual_seed(batch)).to(device="cuda", dtype=torch.int32)
    want = compose(desc, p0, X, Y, perm, batch)
    p, m, v = p0.clone()[None], torch.zeros_like(p0)[None], torch.zeros_like(p0)[None]
    bl = train_epoch_flat(desc, p, m, v, X, Y, perm[None].contiguous(), batch, MR.LR, 0)
    assert bl.shape == (1, (MR.ROWS + batch - 1) // batch)
    diff = {name: (int((a != b).sum()), a.numel(), float((a - b).abs().max()))
            for name, a, b in zip(("params", "exp_avg", "exp_avg_sq", "batch_loss"), (p[0], m[0], v[0], bl[0]), want) if not torch.equal(a, b)}
    assert not diff, f"(elements that differ, of, max |difference|): {diff}"
    assert not torch.equal(p[0], p0)


@pytest.mark.parametrize("tag", ["init", "trained"])
@pytest.mark.parametrize("case", list(MR.CASES))
def test_three_adam_steps_against_goldens(g14, case, tag):
    """Batches [0:64], [64:104], [0:64]: one epoch of 104 rows at batch 64 (identity order), then one of the first 64 rows from step 2.
    Measured on an MI355X: worst tensor 7.2e-08 .. 4.6e-07 over the eight cases (bar 1e-3)."""
    from diffsg_amd.mtfnn import train_epoch_flat
    widths, n_sig = MR.CASES[case]
    desc = desc_of(widths, n_sig)
    X, Y = (dev(a) for a in MR.inputs(case))
    p = dev(MR.flat(state(g14, case, tag), widths))[None].contiguous()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    ident = torch.arange(MR.ROWS, device="cuda", dtype=torch.int32)[None]
    l1 = train_epoch_flat(desc, p, m, v, X, Y, ident.contiguous(), 64, MR.LR, 0)
    l2 = train_epoch_flat(desc, p, m, v, X[:64].contiguous(), Y[:64].contiguous(), ident[:, :64].contiguous(), 64, MR.LR, 2)
    assert rel(torch.cat((l1[0], l2[0])), g14[f"{case}.{tag}.step_loss"]) < 1e-5
    got = MR.unflat(p[0].cpu().numpy(), widths)
    errs = {k: rel(got[k], g14[f"{case}.{tag}.adam.{k}"]) for k in got}
    print(f"adam x3 {case}.{tag}: worst tensor {max(errs.values()):.2e}")
    assert max(errs.values()) < ATOL, errs


def test_replicas_are_independent_and_deterministic(g14):
    from diffsg_amd.mtfnn import train_epoch_flat
    widths, n_sig = MR.CASES["co3"]
    desc = desc_of(widths, n_sig)
    X, Y = (dev(a) for a in MR.inputs("co3"))
    R, batch = 3, 40
    p0 = torch.stack([dev(MR.flat(MR.synth_state(widths, 100 + r), widths)) for r in range(R)]).contiguous()
    perm = torch.stack([torch.randperm(MR.ROWS, generator=torch.Generator().manual_seed(r)) for r in range(R)]).to(device="cuda",
                                                                                                                  dtype=torch.int32)

    def run(ps, perms, step0=5):
        p, m, v = ps.clone(), torch.full_like(ps, 0.01), torch.full_like(ps, 1e-4)
        return p, m, v, train_epoch_flat(desc, p, m, v, X, Y, perms.contiguous(), batch, MR.LR, step0)

    both = run(p0, perm)
    again = run(p0, perm)
    assert all(torch.equal(a, b) for a, b in zip(both, again))
    for r in range(R):
        one = run(p0[r:r + 1], perm[r:r + 1])
        assert all(torch.equal(a[r:r + 1], b) for a, b in zip(both, one)), r
    assert not torch.equal(both[0][0], both[0][1])


@pytest.mark.parametrize("what,widths,n_sig,n_layers", [
    ("hidden width 65", (9, 32, 65, 16, 3), 3, 4),
    ("six layers", (9, 32, 64, 16, 8, 3), 3, 6),
    ("n_sig above the output width", (9, 32, 64, 16, 3), 4, 4),
])
def test_refusals(what, widths, n_sig, n_layers):
    from diffsg_amd import _lib
    d = desc_of(widths, n_sig)
    d.n_layers = n_layers
    L = _lib.lib()
    x, y = torch.rand(8, 9, device="cuda"), torch.rand(8, 3, device="cuda")
    par, out = torch.zeros(40000, device="cuda"), torch.full((8, 3), -7.0, device="cuda")
    grad, loss = torch.full((40000,), -7.0, device="cuda"), torch.full((1,), -7.0, device="cuda")
    perm = torch.arange(8, device="cuda", dtype=torch.int32)
    s = _lib.stream_ptr()
    calls = {
        "dsg_mlp_forward": lambda: L.dsg_mlp_forward(ctypes.byref(d), _lib.ptr(par), _lib.ptr(x), _lib.ptr(out), 8, s),
        "dsg_mlp_loss_grad": lambda: L.dsg_mlp_loss_grad(ctypes.byref(d), _lib.ptr(par), _lib.ptr(x), _lib.ptr(y), 8, _lib.ptr(loss),
                                                         _lib.ptr(grad), s),
        "dsg_mlp_train_epoch": lambda: L.dsg_mlp_train_epoch(ctypes.byref(d), _lib.ptr(par), _lib.ptr(grad), _lib.ptr(grad), _lib.ptr(x),
                                                             _lib.ptr(y), _lib.ptr(perm), 8, 4, 0.005, 0.9, 0.999, 1e-8, 0, _lib.ptr(loss), 1, s),
    }
    for name, call in calls.items():
        assert call() != 0, (what, name)
        msg = L.dsg_last_error().decode()
        assert name in msg and len(msg) > len(name) + 4, msg
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((grad == -7.0).all()) and bool((loss == -7.0).all()) and bool((par == 0).all())
    assert L.dsg_mlp_param_total(ctypes.byref(d)) == -1


def test_zero_rows_launch_nothing():
    from diffsg_amd import _lib
    widths, n_sig = MR.CASES["co3"]
    d = desc_of(widths, n_sig)
    L = _lib.lib()
    assert L.dsg_mlp_param_total(ctypes.byref(d)) == sum(int(np.prod(s)) for _, s in MR.shapes(widths))
    assert L.dsg_mlp_forward(ctypes.byref(d), None, None, None, 0, _lib.stream_ptr()) == 0
    assert L.dsg_mlp_loss_grad(ctypes.byref(d), None, None, None, 0, None, None, _lib.stream_ptr()) == 0
    assert L.dsg_mlp_train_epoch(ctypes.byref(d), None, None, None, None, None, None, 0, 512, 0.005, 0.9, 0.999, 1e-8, 0, None, 1,
                                 _lib.stream_ptr()) == 0


def test_fit_end_to_end():
    """fit on 2 048 rows of CO-shaped data, 3 epochs at batch 512, two replicas: the loss falls, the replica equals training it alone
    from the same generator state, and the no-grad forward of the trained module is dsg_mlp_forward (and the torch module's, to TOL)."""
    from diffsg_amd import co_net, init_weights
    from diffsg_amd.mtfnn import fit, flat_params, forward_flat, model_desc
    rs = np.random.RandomState(7)
    X = rs.uniform(0, 1, (2048, 9)).astype(np.float32)
    Y = (1.0 / (1.0 + np.exp(-(X @ rs.standard_normal((9, 3)))))).astype(np.float32)

    def make(seed):
        torch.manual_seed(seed)
        m = co_net(9, 3)
        m.apply(init_weights)
        return m.to("cuda")

    a, b = make(1), make(2)
    lines = []
    torch.manual_seed(3)
    hist = fit(a, X, Y, 3, batch_size=512, replicas=[a, b], log=lines.append)
    assert len(hist) == 3 and len(hist[0]) == 2 and len(lines) == 3 and lines[0].startswith("Epoch: 0, Loss: ")
    assert hist[-1][0] < hist[0][0] and hist[-1][1] < hist[0][1]
    # the first replica alone from the same generator state: epoch 0's first permutation is its own in both runs
    a1 = make(1)
    torch.manual_seed(3)
    h1 = fit(a1, X, Y, 1, batch_size=512, log=None)
    assert h1[0][0] == hist[0][0]
    xd = dev(X)
    with torch.no_grad():
        got = a(xd)
    assert torch.equal(got, forward_flat(model_desc(a), flat_params(a), xd))
    with torch.enable_grad():
        want = a(xd)
    assert want.requires_grad and rel(got, want) < TOL
    # the cached flat vector follows the parameters: an in-place change, then a model left on the CPU (torch's own error, no library call)
    with torch.no_grad():
        a.lin4.bias.add_(0.5)
        moved = a(xd)
    assert not torch.equal(moved, got) and torch.equal(moved, forward_flat(model_desc(a), flat_params(a), xd))
    with torch.no_grad(), pytest.raises(RuntimeError):
        co_net(9, 3)(xd)
