"""MTFNN baseline, host side (no GPU): the float64 restatement against the torch goldens, the modules' layout and seeded
initialisation, the per-epoch learning rates, and the permutations `fit` trains on."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.utils.data as data

from _util import GOLD
import mtfnn_ref as MR

TOL = 1e-5      # forward, max|a - b| / max|b|: the bar of tests/test_gpu_parity.py
GTOL = 1e-4     # gradients, per tensor on the grad_errs scale
ATOL = 1e-3     # parameters after three Adam steps (rel), the bar of the project's three-step Adam test


@pytest.fixture(scope="module")
def g14():
    return np.load(os.path.join(GOLD, "g14_mtfnn.npz"))


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def grad_errs(got, ref):
    gmax = max(float(np.abs(v).max()) for v in ref.values())
    return {k: float(np.abs(np.asarray(got[k], dtype=np.float64) - ref[k]).max()) / max(float(np.abs(ref[k]).max()), 1e-3 * gmax) for k in ref}


def build(case):
    from diffsg_amd import MTFNN, co_net, msr_net
    widths, _ = MR.CASES[case]
    ctor = MTFNN if case.startswith("nu") else (co_net if case.startswith("co") else msr_net)
    return ctor(widths[0], widths[-1])


def state(g14, case, tag):
    """The weight state of a golden case: `trained` is stored, `init` is the seeded construction of this package's module."""
    widths, _ = MR.CASES[case]
    if tag == "trained":
        return {k: g14[f"{case}.trained.w.{k}"] for k, _ in MR.shapes(widths)}
    from diffsg_amd import init_weights
    torch.manual_seed(int(g14[f"{case}.init.seed"]))
    m = build(case)
    m.apply(init_weights)
    return {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}


@pytest.mark.parametrize("tag", ["init", "trained"])
@pytest.mark.parametrize("case", list(MR.CASES))
def test_restatement_against_goldens(g14, case, tag):
    widths, n_sig = MR.CASES[case]
    w = state(g14, case, tag)
    X, Y = MR.inputs(case)
    assert MR.relu_margin(w, widths, n_sig, X) >= MR.RELU_MARGIN
    assert rel(MR.forward(w, widths, n_sig, X), g14[f"{case}.{tag}.out"]) < TOL
    loss, grads = MR.loss_grad(w, widths, n_sig, X, Y)
    assert abs(loss - float(g14[f"{case}.{tag}.loss"])) < 1e-5 * abs(loss)
    errs = grad_errs({k: g14[f"{case}.{tag}.grad.{k}"] for k in grads}, grads)
    assert max(errs.values()) < GTOL, errs
    p3, losses = MR.adam_steps(w, widths, n_sig, X, Y)
    assert rel(losses, g14[f"{case}.{tag}.step_loss"]) < 1e-5
    for k in p3:
        assert rel(g14[f"{case}.{tag}.adam.{k}"], p3[k]) < ATOL, k


@pytest.mark.parametrize("case", list(MR.CASES))
def test_module_layout_and_seeded_init(g14, case):
    widths, n_sig = MR.CASES[case]
    m = build(case)
    sd = m.state_dict()
    assert list(sd) == list(g14[f"{case}.layout"])
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == MR.shapes(widths)
    assert m.n_sig == n_sig
    names = [n for n, _ in m.named_children()]
    L = len(widths) - 1
    want = [x for i in range(1, L) for x in (f"lin{i}", f"act{i}")] + ([f"lin{L}", f"act{L}1", f"act{L}2"] if case.startswith("nu")
                                                                      else [f"lin{L}", f"act{L}"])
    assert names == want
    w = state(g14, case, "init")
    np.testing.assert_allclose([float(v.astype(np.float64).sum()) for v in w.values()], g14[f"{case}.init.sums"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose([float(np.abs(v.astype(np.float64)).sum()) for v in w.values()], g14[f"{case}.init.abs"], rtol=1e-9)
    # state dicts load strictly both ways, and the CPU forward of the module is the golden's
    m2 = build(case)
    m2.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    with torch.no_grad():
        assert rel(m2(torch.from_numpy(MR.inputs(case)[0])).numpy(), g14[f"{case}.init.out"]) < TOL


def test_module_autograd_path_matches_goldens(g14):
    """The torch fallback (autograd on): the NU module's out-of-place head gives the reference's loss and gradients."""
    case = "nu3"
    m = build(case)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state(g14, case, "trained").items()}, strict=True)
    X, Y = MR.inputs(case)
    loss = torch.nn.functional.mse_loss(torch.from_numpy(Y), m(torch.from_numpy(X)))
    loss.backward()
    assert abs(loss.item() - float(g14[f"{case}.trained.loss"])) < 1e-5 * loss.item()
    ref = {k: g14[f"{case}.trained.grad.{k}"].astype(np.float64) for k, _ in m.named_parameters()}
    errs = grad_errs({k: p.grad.numpy() for k, p in m.named_parameters()}, ref)
    assert max(errs.values()) < GTOL, errs


@pytest.mark.parametrize("milestones,epochs", [((20,), 50), ((20, 60), 100), ((), 5), ((0, 2, 2), 6)])
def test_epoch_lrs_are_the_schedulers(milestones, epochs):
    from diffsg_amd.mtfnn import epoch_lrs
    opt = torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=0.005)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, list(milestones))
    want = []
    for _ in range(epochs):
        want.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    assert epoch_lrs(0.005, milestones, epochs) == want          # the same doubles


@pytest.mark.parametrize("N,batch", [(104, 64), (1000, 512), (7, 512)])
def test_fit_permutations_are_the_dataloaders(N, batch):
    """Two epochs drawn as `fit` draws them equal the row order a shuffling DataLoader over the tensors yields from the same seed,
    and leave torch's global generator in the same state."""
    from diffsg_amd.mtfnn import epoch_permutation
    X = torch.arange(N, dtype=torch.float32)[:, None] * torch.ones(1, 3)
    Y = -torch.arange(N, dtype=torch.float32)[:, None]
    torch.manual_seed(11)
    loader = data.DataLoader(data.TensorDataset(X, Y), batch_size=batch, shuffle=True)
    want = []
    for _ in range(2):
        rows, sizes = [], []
        for x, y in loader:
            assert torch.equal(x[:, 0], -y[:, 0])
            rows.append(x[:, 0].to(torch.int64))
            sizes.append(x.shape[0])
        assert sizes == [min(batch, N - i) for i in range(0, N, batch)]
        want.append(torch.cat(rows))
    tail_want = torch.rand(3)
    torch.manual_seed(11)
    got = [epoch_permutation(N, batch) for _ in range(2)]
    tail_got = torch.rand(3)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert torch.equal(tail_got, tail_want)
    assert not torch.equal(got[0], got[1]) or N < 3


def test_fit_wants_the_model_among_its_replicas():
    from diffsg_amd import co_net
    from diffsg_amd.mtfnn import fit
    a, b = co_net(9, 3), co_net(9, 3)
    with pytest.raises(ValueError, match="must contain"):
        fit(a, np.zeros((4, 9), np.float32), np.zeros((4, 3), np.float32), 1, replicas=[b], log=None)


def test_param_total_of_the_listed_sizes():
    """The library's parameter count against the state-dict shapes: the golden cases, the sizes DESIGN.md section 11 lists, and the
    nets tests/test_gpu_mtfnn.py runs at tile heights 32 and 16."""
    from diffsg_amd import _lib
    from diffsg_amd.mtfnn import mlp_desc
    L = _lib.lib()
    nets = [(w, n, None) for w, n in MR.CASES.values()] + [
        ((9, 32, 64, 16, 3), 3, 3523), ((128, 8, 16, 8, 128), 0, 2464), ((6, 64, 32, 16, 32, 5), 2, 3765),
        ((64, 64, 32, 16, 32, 34), 2, 8434), ((128, 64, 64, 128), 64, 20736), ((128, 64, 64, 64, 64, 128), 0, 29056)]
    for widths, n_sig, want in nets:
        got = L.dsg_mlp_param_total(ctypes.byref(mlp_desc(widths, n_sig)))
        assert got == sum(int(np.prod(s)) for _, s in MR.shapes(widths)) and (want is None or got == want), widths


@pytest.mark.parametrize("what,widths,n_sig,n_layers", [
    ("one layer", (9, 3), 3, 1),
    ("six layers", (9, 32, 64, 16, 8, 3), 3, 6),
    ("hidden width 65", (9, 32, 65, 16, 3), 3, 4),
    ("input width 129", (129, 32, 64, 16, 3), 3, 4),
    ("output width 129", (9, 32, 64, 16, 129), 3, 4),
    ("n_sig above the output width", (9, 32, 64, 16, 3), 4, 4),
])
def test_descriptor_limits_are_refused(what, widths, n_sig, n_layers):
    """Refused on the host, before any device call: runs without a GPU."""
    from diffsg_amd import _lib
    from diffsg_amd.mtfnn import mlp_desc
    d = mlp_desc(widths, n_sig)
    d.n_layers = n_layers
    L = _lib.lib()
    one = ctypes.c_void_p(16)           # never dereferenced: the descriptor is refused first
    calls = {
        "dsg_mlp_forward": lambda: L.dsg_mlp_forward(ctypes.byref(d), one, one, one, 8, None),
        "dsg_mlp_loss_grad": lambda: L.dsg_mlp_loss_grad(ctypes.byref(d), one, one, one, 8, one, one, None),
        "dsg_mlp_train_epoch": lambda: L.dsg_mlp_train_epoch(ctypes.byref(d), one, one, one, one, one, one, 8, 4, 0.005, 0.9, 0.999, 1e-8, 0,
                                                             one, 1, None),
    }
    for name, call in calls.items():
        assert call() != 0, (what, name)
        msg = L.dsg_last_error().decode()
        assert name in msg and len(msg) > len(name) + 4, msg
    assert L.dsg_mlp_param_total(ctypes.byref(d)) == -1
    assert "dsg_mlp_param_total" in L.dsg_last_error().decode()
