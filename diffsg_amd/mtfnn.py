"""The MTFNN baseline (reference: baselines/MTFNN.py): the small regression MLPs DiffSG is compared with, on the device.

The three nets are plain torch modules with the reference's names and registration order, so seeded construction +
`.apply(init_weights)` gives the reference's weights and state dicts load strictly both ways.  On a HIP device under
`torch.no_grad()` their `forward` is one `dsg_mlp_forward` launch (the flat parameter vector it reads is rebuilt only after a
parameter changed); on the CPU, or with autograd on, it is the torch module
(host code: these three modules are the one place with a torch fallback).  `loss_grad` is `dsg_mlp_loss_grad`, `fit` the
reference's training loop with ONE `dsg_mlp_train_epoch` launch per epoch (csrc/dsg_mlp.hpp).

Reference quirk kept and named: the reference's evaluation loader shuffles too (MTFNN.py:77,156,253), so its predictions
are scored against inputs and labels in a different row order.  The drivers return both figures: `*_reference_order`
follows that loop (and consumes torch's global generator as it does), `*_aligned` scores row against row.
"""
from collections import OrderedDict
import ctypes
from functools import partial

import torch
import torch.nn as nn

from . import _lib
from . import _smallnet as _sn
from ._smallnet import epoch_lrs, epoch_permutation, flat_params  # noqa: F401  (part of this module's interface)
from .diffusion import init_weights

_cuda = partial(_sn.cuda, "mtfnn")
_call = _sn.call


# ---------------------------------------------------------------------------------------------------------------------
# modules
# ---------------------------------------------------------------------------------------------------------------------
def _use_device_path(model, x):
    """The library path: no autograd, and input and parameters on the same HIP device (anything else is the torch module, which
    raises torch's own device-mismatch error where the two differ)."""
    return x.is_cuda and not torch.is_grad_enabled() and next(model.parameters()).device == x.device


class MTFNN(nn.Module):
    """MTFNN.py:187-211 (the NU net): in -> 64 -> 32 -> 16 -> 32 -> out, sigmoid on columns 0, 1 and softmax on the rest."""
    n_sig = 2

    def __init__(self, in_dim, out_dim):
        super().__init__()
        self.lin1 = nn.Linear(in_dim, 64)
        self.act1 = nn.ReLU()
        self.lin2 = nn.Linear(64, 32)
        self.act2 = nn.ReLU()
        self.lin3 = nn.Linear(32, 16)
        self.act3 = nn.ReLU()
        self.lin4 = nn.Linear(16, 32)
        self.act4 = nn.ReLU()
        self.lin5 = nn.Linear(32, out_dim)
        self.act51 = nn.Sigmoid()
        self.act52 = nn.Softmax(dim=1)      # the reference's bare nn.Softmax() resolves to dim 1 on its 2-D input

    def forward(self, x):
        if _use_device_path(self, x):
            return device_forward(self, x)
        x = self.act1(self.lin1(x))
        x = self.act2(self.lin2(x))
        x = self.act3(self.lin3(x))
        x = self.act4(self.lin4(x))
        x = self.lin5(x)
        # the reference assigns the two slices in place; the same values and gradients without the in-place writes
        return torch.cat((self.act51(x[:, :2]), self.act52(x[:, 2:])), dim=1)


class _SequentialNet(nn.Sequential):
    """nn.Sequential whose no-grad forward on a HIP device is one library launch."""
    n_sig = 0

    def forward(self, x):
        if _use_device_path(self, x):
            return device_forward(self, x)
        return super().forward(x)


def co_net(in_dim, out_dim):
    """The inline net of mtfnn_co (MTFNN.py:44-53): 3n -> 32 -> 64 -> 16 -> n, sigmoid on every output."""
    net = _SequentialNet(OrderedDict([
        ('lin1', nn.Linear(in_dim, 32)), ('act1', nn.ReLU()),
        ('lin2', nn.Linear(32, 64)), ('act2', nn.ReLU()),
        ('lin3', nn.Linear(64, 16)), ('act3', nn.ReLU()),
        ('lin4', nn.Linear(16, out_dim)), ('act4', nn.Sigmoid())]))
    net.n_sig = out_dim
    return net


def msr_net(in_dim, out_dim):
    """The inline net of mtfnn_msr (MTFNN.py:123-132): M -> 8 -> 16 -> 8 -> M, softmax over the outputs."""
    net = _SequentialNet(OrderedDict([
        ('lin1', nn.Linear(in_dim, 8)), ('act1', nn.ReLU()),
        ('lin2', nn.Linear(8, 16)), ('act2', nn.ReLU()),
        ('lin3', nn.Linear(16, 8)), ('act3', nn.ReLU()),
        ('lin4', nn.Linear(8, out_dim)), ('act4', nn.Softmax(dim=1))]))
    net.n_sig = 0
    return net


# ---------------------------------------------------------------------------------------------------------------------
# the library's view of a module
# ---------------------------------------------------------------------------------------------------------------------
def linears(model):
    return [m for m in model.children() if isinstance(m, nn.Linear)]


def mlp_desc(widths, n_sig):
    """ctypes descriptor of a net with the given widths (inputs ... outputs).  Not validated here: the library refuses."""
    d = _lib.MlpDesc()
    d.n_layers = len(widths) - 1
    for i, w in enumerate(list(widths)[:6]):
        d.widths[i] = int(w)
    d.n_sig = int(n_sig)
    return d


def model_desc(model):
    lins = linears(model)
    return mlp_desc([lins[0].in_features] + [l.out_features for l in lins], model.n_sig)


def forward_flat(desc, params, x):
    """dsg_mlp_forward on a flat parameter vector."""
    out = torch.empty((x.shape[0], desc.widths[desc.n_layers]), device=x.device, dtype=torch.float32)
    _call("dsg_mlp_forward", x.device, ctypes.byref(desc), _lib.ptr(params), _lib.ptr(x), _lib.ptr(out), x.shape[0])
    return out


def device_forward(model, x):
    x = _cuda(x, x.device, "forward")
    desc, flat = _sn.cached_flat(model, model_desc)
    if x.shape[1] != desc.widths[0]:
        raise ValueError(f"forward: x has {x.shape[1]} columns, the net {desc.widths[0]} inputs")
    return forward_flat(desc, flat, x)


def loss_grad_flat(desc, params, x, y):
    """dsg_mlp_loss_grad on a flat parameter vector: (loss (0-d tensor), flat gradient)."""
    loss = torch.zeros((), device=x.device, dtype=torch.float32)
    grad = torch.zeros_like(params)
    _call("dsg_mlp_loss_grad", x.device, ctypes.byref(desc), _lib.ptr(params), _lib.ptr(x), _lib.ptr(y), x.shape[0], _lib.ptr(loss),
          _lib.ptr(grad))
    return loss, grad


def loss_grad(model, x, y):
    """(loss, {parameter name: gradient}) of F.mse_loss(y, model(x)), from dsg_mlp_loss_grad."""
    dev = next(model.parameters()).device
    x, y = _cuda(x, dev, "loss_grad"), _cuda(y, dev, "loss_grad")
    desc = model_desc(model)
    if x.shape[1] != desc.widths[0] or y.shape != (x.shape[0], desc.widths[desc.n_layers]):
        raise ValueError(f"loss_grad: x {tuple(x.shape)} / y {tuple(y.shape)} do not fit the net")
    loss, flat = loss_grad_flat(desc, flat_params(model), x, y)
    return loss, _sn.named_grads(model, flat)


# ---------------------------------------------------------------------------------------------------------------------
# training
# ---------------------------------------------------------------------------------------------------------------------
def train_epoch_flat(desc, params, exp_avg, exp_avg_sq, X, Y, perm, batch, lr, step0, betas=(0.9, 0.999), eps=1e-8):
    """dsg_mlp_train_epoch on flat [R][P] tensors (updated in place); perm int32 [R][N].  Returns batch_loss [R][ceil(N / batch)]."""
    R, N = perm.shape
    nb = (N + batch - 1) // batch
    batch_loss = torch.zeros((R, nb), device=X.device, dtype=torch.float32)
    _call("dsg_mlp_train_epoch", X.device, ctypes.byref(desc), _lib.ptr(params), _lib.ptr(exp_avg), _lib.ptr(exp_avg_sq), _lib.ptr(X),
          _lib.ptr(Y), _lib.ptr(perm), N, batch, float(lr), betas[0], betas[1], eps, step0, _lib.ptr(batch_loss), R)
    return batch_loss


def fit(model, X, Y, epochs, batch_size=512, lr=0.005, milestones=(20,), replicas=None, log=print):
    """The reference's training loop (MTFNN.py:57-73) on the device: Adam with torch's default betas / eps, MultiStepLR(gamma=0.1),
    one launch per epoch.  X, Y (arrays or tensors) are uploaded once.  `replicas`: the list of models trained side by side in the
    same launches (all of `model`'s architecture, `model` among them), each with permutations of its
    own, drawn replica by replica within each epoch.  Returns the per-epoch log values, [epochs][R] (the reference's
    `epoch_loss / epoch_sample_num`: the sum of the batch means over the row count)."""
    dev = next(model.parameters()).device
    models = _sn.replica_list("mtfnn", "model", model, replicas, dev, model_desc)
    desc = model_desc(model)
    X, Y = _cuda(X, dev, "fit"), _cuda(Y, dev, "fit")
    N = X.shape[0]
    if X.shape[1] != desc.widths[0] or Y.shape != (N, desc.widths[desc.n_layers]):
        raise ValueError(f"fit: X {tuple(X.shape)} / Y {tuple(Y.shape)} do not fit the net")
    params = torch.stack([flat_params(m).to(dev) for m in models]).contiguous()
    exp_avg, exp_avg_sq = torch.zeros_like(params), torch.zeros_like(params)
    nb = (N + batch_size - 1) // batch_size
    history = []
    for epoch, cur_lr in enumerate(epoch_lrs(lr, milestones, epochs)):
        perm = torch.stack([epoch_permutation(N, batch_size) for _ in models]).to(device=dev, dtype=torch.int32)
        bl = train_epoch_flat(desc, params, exp_avg, exp_avg_sq, X, Y, perm, batch_size, cur_lr, epoch * nb).cpu()
        vals = [_sn.running_sum(row) / N if N else 0.0 for row in bl.tolist()]
        history.append(vals)
        if log is not None:
            log(f"Epoch: {epoch}, Loss: {vals[0] if len(vals) == 1 else vals}")
    for m, p in zip(models, params):
        _sn.unflatten_into(m, p)
    return history


# ---------------------------------------------------------------------------------------------------------------------
# drivers
# ---------------------------------------------------------------------------------------------------------------------
def _predict(model, X_test, batch_size=512):
    """(predictions row for row, predictions in the reference's evaluation order).  The reference's evaluation loader shuffles
    (MTFNN.py:77): its Y_pred is model(X_test[perm]); the permutation is drawn as that loader draws it."""
    with torch.no_grad():
        aligned = model(X_test)
    perm = epoch_permutation(X_test.shape[0], batch_size).to(X_test.device)
    return aligned, aligned[perm]


def mtfnn_co(dataset_path, epochs=50, batch_size=512, lr=0.005, milestones=(20,), replicas=None, save_path=None, log=print):
    """mtfnn_co, MTFNN.py:29-104.  Returns (model, {"sum_ratio_*": the reference's "exceeded ratio", "mean_diff_*": its "avg cost
    diff"}); `replicas`: further co_net models to train beside it (fit)."""
    from . import decode
    from .classifier_free_CO import co_data_load
    X_train, Y_train, X_test, Y_test, custom_config = co_data_load(dataset_path)
    dev = _sn.device()
    node_num = Y_train.shape[1]
    model = co_net(node_num * 3, node_num)
    model.apply(init_weights)
    model.to(dev)
    out = {"history": fit(model, X_train, Y_train, epochs, batch_size, lr, milestones, [model] + list(replicas) if replicas else None, log)}
    X_t, Y_t = _cuda(X_test, dev, "mtfnn_co"), _cuda(Y_test, dev, "mtfnn_co")
    aligned, ref_order = _predict(model, X_t, batch_size)
    lo, hi = custom_config['scaler_min'], custom_config['scaler_max']
    X_raw = X_t * (hi - lo) + lo
    true_cost = decode.co_cost(X_raw, Y_t)
    _sn.figures(decode.co_cost(X_raw, ref_order), true_cost, "reference_order", out)
    _sn.figures(decode.co_cost(X_raw, aligned), true_cost, "aligned", out)
    return _sn.finish(model, out, save_path, log)


def mtfnn_msr(dataset_path, epochs=50, batch_size=512, lr=0.005, milestones=(20,), replicas=None, save_path=None, log=print):
    """mtfnn_msr, MTFNN.py:107-184: trained on Y / W (softmax targets), predictions scaled back by W.  Returns (model, {"sum_ratio_*":
    the reference's "less ratio", "mean_diff_*": its "avg rate diff"})."""
    from . import decode
    from .classifier_free_MSR import msr_data_load
    X_train, Y_train, X_test, Y_test, custom_config = msr_data_load(dataset_path)
    M, W = custom_config['M'], custom_config['W']
    Y_train /= W  # Softmax train (in place, as the reference)
    dev = _sn.device()
    model = msr_net(M, M)
    model.apply(init_weights)
    model.to(dev)
    out = {"history": fit(model, X_train, Y_train, epochs, batch_size, lr, milestones, [model] + list(replicas) if replicas else None, log)}
    X_t, Y_t = _cuda(X_test, dev, "mtfnn_msr"), _cuda(Y_test, dev, "mtfnn_msr")
    aligned, ref_order = _predict(model, X_t, batch_size)
    aligned, ref_order = aligned * W, ref_order * W
    lo, hi = custom_config['scaler_min'], custom_config['scaler_max']
    X_raw = X_t * (hi - lo) + lo
    true_rate = decode.msr_rate(Y_t, X_raw)
    _sn.figures(decode.msr_rate(ref_order, X_raw), true_rate, "reference_order", out)
    _sn.figures(decode.msr_rate(aligned, X_raw), true_rate, "aligned", out)
    return _sn.finish(model, out, save_path, log)


def mtfnn_nu(dataset_path, epochs=100, width=400, height=400, batch_size=512, lr=0.005, milestones=(20, 60), replicas=None,
             save_path=None, log=print):
    """mtfnn_nu, MTFNN.py:213-287: positions scaled by (width, height), powers by P_sum.  Returns (model, {"sum_ratio_*": the
    reference's "less ratio", "mean_diff_*": its "avg rate diff"})."""
    from . import decode
    from .classifier_free_NU import nu_data_load
    X_train, Y_train, X_test, Y_test, _, custom_config = nu_data_load(dataset_path, width, height)
    K, P_sum = custom_config['K'], custom_config['P_sum']
    dev = _sn.device()
    model = MTFNN(K * 2, 2 + K)
    model.apply(init_weights)
    model.to(dev)
    out = {"history": fit(model, X_train, Y_train, epochs, batch_size, lr, milestones, [model] + list(replicas) if replicas else None, log)}
    X_t, Y_t = _cuda(X_test, dev, "mtfnn_nu"), _cuda(Y_test, dev, "mtfnn_nu")
    aligned, ref_order = _predict(model, X_t, batch_size)
    xs = torch.tensor([width, height] * K, device=dev, dtype=torch.float32)
    ys = torch.tensor([width, height] + [P_sum] * K, device=dev, dtype=torch.float32)
    X_raw = X_t * xs
    true_rate = decode.nu_rate(Y_t * ys, X_raw)
    _sn.figures(decode.nu_rate(ref_order * ys, X_raw), true_rate, "reference_order", out)
    _sn.figures(decode.nu_rate(aligned * ys, X_raw), true_rate, "aligned", out)
    return _sn.finish(model, out, save_path, log)
