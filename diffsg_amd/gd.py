"""The gradient-descent baseline (reference: baselines/GD.py): plain gradient steps on each problem's penalised objective, on the device.

Everything is float64, like the reference's numpy.  One library call runs every iteration of every row in one launch
(csrc/dsg_gd.hpp): `co_descent`, `msr_descent` and `nu_descent` take the condition X and a start state and
return the state after `iters` steps, with `record_every` also the states on the way (the convergence curve).  The drivers `gd_co`,
`gd_msr` and `gd_nu` are the reference's co_solve / msr_solve / nu_solve with the dataset path and the counts as arguments.

Reference quirks kept and named: the MSR penalty is centred on 1, not on W; the NU x gradient reads the user's Y coordinate in its
second term; the NU coordinates arrive divided by width and height while the UAV position is in metres; the NU power penalty is
centred on 18 whatever the file's P_sum is (`p_ref`).  The CO iteration divides by allocations that cross zero: it is chaotic, and
the states of ill-conditioned rows after many iterations are the reference's only as long as the float64 trajectories coincide.
"""
import torch

from . import _lib
from . import _smallnet as _sn

_call = _sn.call


def _cuda64(t, what):
    """t, which must be a float64 (rows, columns) tensor on a HIP device, made contiguous.  Nothing is cast or moved: another dtype
    would silently change the trajectory."""
    if not torch.is_tensor(t):
        raise TypeError(f"diffsg_amd.gd.{what}: expected a torch tensor, got {type(t).__name__}")
    if t.dtype != torch.float64:
        raise TypeError(f"diffsg_amd.gd.{what}: tensors must be float64 (the reference iterates in float64), got {t.dtype}")
    if not t.is_cuda:
        raise RuntimeError(f"diffsg_amd.gd.{what}: tensors are not on a HIP device; libdiffsg_hip has no CPU path")
    if t.dim() != 2:
        raise ValueError(f"{what}: expected a (rows, columns) tensor, got {tuple(t.shape)}")
    return t.detach().contiguous()


def _counts(what, iters, record_every):
    iters, record_every = int(iters), int(record_every)
    if iters < 0 or record_every < 0:
        raise ValueError(f"{what}: iters = {iters}, record_every = {record_every}")
    return iters, record_every


def _state(what, X, y0, init, D):
    """The start state as a fresh tensor the launch may overwrite: a copy of y0, or the reference's start."""
    if y0 is None:
        return init()
    y0 = _cuda64(y0, what)
    if y0.device != X.device or y0.shape != (X.shape[0], D):
        raise ValueError(f"{what}: y0 is {tuple(y0.shape)} on {y0.device}, expected {(X.shape[0], D)} on {X.device}")
    return y0.clone()


def _descend(name, X, Y, iters, record_every, *scalars):
    rec = torch.empty((iters // record_every, Y.shape[0], Y.shape[1]), device=Y.device, dtype=torch.float64) if record_every else None
    _call(name, X.device, _lib.ptr(X), _lib.ptr(Y), X.shape[0], *scalars, _lib.ptr(rec), record_every)
    return (Y, rec) if record_every else Y


# ---------------------------------------------------------------------------------------------------------------------
# start states (GD.py:32-33, 80, 127-128)
# ---------------------------------------------------------------------------------------------------------------------
def co_init(rows, node_num, device=None):
    """Decisions 1, allocations 1 / node_num."""
    y = torch.ones((rows, 2 * node_num), device=device or _sn.device(), dtype=torch.float64)
    y[:, node_num:] = 1 / node_num
    return y


def msr_init(rows, M, W, device=None):
    """W / M on every channel."""
    return torch.ones((rows, M), device=device or _sn.device(), dtype=torch.float64) / M * W


def nu_init(rows, K, P_sum, width, height, device=None):
    """The UAV at the centre of the field, P_sum / K - 0.01 on every user."""
    y = torch.ones((rows, 2 + K), device=device or _sn.device(), dtype=torch.float64) * P_sum / K - 0.01
    y[:, 0], y[:, 1] = width / 2, height / 2
    return y


# ---------------------------------------------------------------------------------------------------------------------
# the descents
# ---------------------------------------------------------------------------------------------------------------------
def co_descent(X, y0=None, iters=100, lr=0.1, lambda1=1.0, lambda2=1.0, record_every=0):
    """`iters` steps Y -= grad * lr of co_gradient (GD.py:12-21) from y0 (default: co_init).  X (rows, 3n) de-normalised costs; the
    state is (rows, 2n) = decisions | allocations.  Returns the final state, with record_every > 0 also the (iters // record_every,
    rows, 2n) states after every record_every-th step."""
    X = _cuda64(X, "co_descent")
    iters, record_every = _counts("co_descent", iters, record_every)
    if X.shape[1] % 3 or not X.shape[1]:
        raise ValueError(f"co_descent: X has {X.shape[1]} columns, expected 3 per node")
    n = X.shape[1] // 3
    Y = _state("co_descent", X, y0, lambda: co_init(X.shape[0], n, X.device), 2 * n)
    return _descend("dsg_gd_co", X, Y, iters, record_every, n, iters, float(lr), float(lambda1), float(lambda2))


def msr_descent(X, W, y0=None, iters=100, lr=0.001, record_every=0):
    """`iters` steps Y += grad * lr of msr_gradient (GD.py:62-70) from y0 (default: msr_init(W)).  X (rows, M) de-normalised gains."""
    X = _cuda64(X, "msr_descent")
    iters, record_every = _counts("msr_descent", iters, record_every)
    M = X.shape[1]
    Y = _state("msr_descent", X, y0, lambda: msr_init(X.shape[0], M, W, X.device), M)
    return _descend("dsg_gd_msr", X, Y, iters, record_every, M, iters, float(lr))


def nu_descent(X, P_sum, width, height, y0=None, iters=100, lr=0.1, p_ref=18.0, record_every=0):
    """`iters` steps Y += grad * lr of nu_gradient (GD.py:100-117, generalised from 3 to K users) from y0 (default: nu_init).  X
    (rows, 2K) user coordinates as nu_data_load scales them; the state is (rows, 2 + K) = position in metres | powers."""
    X = _cuda64(X, "nu_descent")
    iters, record_every = _counts("nu_descent", iters, record_every)
    if X.shape[1] % 2 or not X.shape[1]:
        raise ValueError(f"nu_descent: X has {X.shape[1]} columns, expected 2 per user")
    K = X.shape[1] // 2
    Y = _state("nu_descent", X, y0, lambda: nu_init(X.shape[0], K, P_sum, width, height, X.device), 2 + K)
    return _descend("dsg_gd_nu", X, Y, iters, record_every, K, iters, float(lr), float(p_ref))


# ---------------------------------------------------------------------------------------------------------------------
# drivers
# ---------------------------------------------------------------------------------------------------------------------
def _finish(pred, true, out, log):
    """The two figures as _smallnet.figures forms them, and the per-row objectives they come from."""
    out["sum_ratio"] = float(torch.sum(pred) / torch.sum(true))
    out["mean_diff"] = float(torch.mean(pred - true))
    out["pred"], out["true"] = pred, true
    if log is not None:
        log(f"sum_ratio: {out['sum_ratio']}, mean_diff: {out['mean_diff']}")
    return out


def gd_co(dataset_path, used_sample_num=10000, iterations=100, log=print):
    """co_solve, GD.py:23-59, on the first `used_sample_num` test rows.  Returns (Y_pred (rows, 2n) float64, {"sum_ratio": the
    reference's "exceeded ratio", "mean_diff": its "avg cost diff", "pred", "true": the per-row costs})."""
    from . import decode
    from .classifier_free_CO import co_data_load
    _, Y_train, X_test, Y_test, custom_config = co_data_load(dataset_path)
    dev = _sn.device()
    lo, hi = custom_config['scaler_min'], custom_config['scaler_max']
    X_raw = torch.as_tensor(X_test * (hi - lo) + lo, dtype=torch.float64)[:used_sample_num].to(dev)
    node_num = Y_train.shape[1]
    Y_pred = co_descent(X_raw, iters=iterations)
    # the reference's normalisation "because the cost_calc cannot cope with the extremely invalid solutions": per-row min-max
    alloc = Y_pred[:, node_num:].to(torch.float32)
    lo_r, hi_r = alloc.min(dim=1, keepdim=True).values, alloc.max(dim=1, keepdim=True).values
    alloc = (alloc - lo_r) / (hi_r - lo_r)
    X32 = X_raw.to(torch.float32)
    Y_t = torch.as_tensor(Y_test, dtype=torch.float32)[:X_raw.shape[0]].to(dev)
    return Y_pred, _finish(decode.co_cost(X32, alloc), decode.co_cost(X32, Y_t), {}, log)


def gd_msr(dataset_path, used_sample_num=1000, iterations=100, log=print):
    """msr_solve, GD.py:72-97: the remainder of the budget is spread evenly after the descent, the rate is float64.  Returns (Y_pred
    after that shift, {"sum_ratio": the reference's "less ratio", "mean_diff": its "avg rate diff", "pred", "true"})."""
    from .classifier_free_MSR import msr_data_load
    _, _, X_test, Y_test, custom_config = msr_data_load(dataset_path)
    dev = _sn.device()
    M, W = custom_config['M'], custom_config['W']
    lo, hi = custom_config['scaler_min'], custom_config['scaler_max']
    X_raw = torch.as_tensor(X_test * (hi - lo) + lo, dtype=torch.float64)[:used_sample_num].to(dev)
    Y_t = torch.as_tensor(Y_test, dtype=torch.float64)[:X_raw.shape[0]].to(dev)
    Y_pred = msr_descent(X_raw, W, iters=iterations)
    Y_pred = Y_pred + (W - Y_pred.sum(dim=1, keepdim=True)) / M
    rate = lambda Y: torch.log2(1.0 + Y * X_raw).sum(dim=1)
    return Y_pred, _finish(rate(Y_pred), rate(Y_t), {}, log)


def gd_nu(dataset_path, width=400, height=400, used_sample_num=3000, iterations=100, log=print):
    """nu_solve, GD.py:120-157: the powers are rescaled to P_sum in float32 and scored by rate_calc.  Returns (Y_pred (rows, 2 + K)
    float32 after that rescaling, {"sum_ratio": the reference's "less ratio", "mean_diff": its "avg rate diff", "pred", "true"})."""
    from . import decode
    from .classifier_free_NU import nu_data_load
    _, _, X_test, Y_test, _, custom_config = nu_data_load(dataset_path, width, height)
    dev = _sn.device()
    K, P_sum = custom_config['K'], custom_config['P_sum']
    X = torch.as_tensor(X_test, dtype=torch.float64)[:used_sample_num].to(dev)
    Y_pred = nu_descent(X, P_sum, width, height, iters=iterations).to(torch.float32)     # p_ref stays the reference's 18
    xs = torch.tensor([width, height] * K, device=dev, dtype=torch.float32)
    ys = torch.tensor([width, height] + [P_sum] * K, device=dev, dtype=torch.float32)
    X32 = X.to(torch.float32) * xs
    Y_t = torch.as_tensor(Y_test, dtype=torch.float32)[:X.shape[0]].to(dev) * ys
    Y_pred[:, 2:] = Y_pred[:, 2:] / Y_pred[:, 2:].sum(dim=1, keepdim=True) * P_sum
    return Y_pred, _finish(decode.nu_rate(Y_pred, X32), decode.nu_rate(Y_t, X32), {}, log)
