"""Float64 numpy restatement of the MTFNN baseline's arithmetic, written for this project: forward (ReLU layers, sigmoid /
softmax head), F.mse_loss, its gradient for every parameter, and torch.optim.Adam.  tests/test_mtfnn_cpu.py holds it to the
goldens recorded from torch (tests/golden/make_mtfnn_goldens.py); the shapes and inputs of the golden cases live here so that
the generator and the tests share them."""
import numpy as np

# name: (widths inputs ... outputs, n_sig = sigmoid columns in front of the softmax)
CASES = {
    "co3": ((9, 32, 64, 16, 3), 3),
    "msr3": ((3, 8, 16, 8, 3), 0),
    "msr80": ((80, 8, 16, 8, 80), 0),
    "nu3": ((6, 64, 32, 16, 32, 5), 2),
}
ROWS = 104
STEP_BATCHES = ((0, 64), (64, 104), (0, 64))        # the three Adam steps of the goldens
LR = 0.005
RELU_MARGIN = 2e-5          # min |pre-activation| >= RELU_MARGIN * max |pre-activation| in every hidden layer (asserted by the generator)


def shapes(widths):
    out = []
    for i in range(len(widths) - 1):
        out.append((f"lin{i + 1}.weight", (widths[i + 1], widths[i])))
        out.append((f"lin{i + 1}.bias", (widths[i + 1],)))
    return out


def synth_state(widths, seed, std=0.3):
    """The "trained-like" state: every weight and bias ~ N(0, std^2), float32."""
    rs = np.random.RandomState(seed)
    return {k: (rs.standard_normal(s) * std).astype(np.float32) for k, s in shapes(widths)}


def inputs(case):
    """X [ROWS][in] uniform; Y [ROWS][out] shaped like the problem's labels (sigmoid columns uniform, softmax columns a distribution)."""
    widths, n_sig = CASES[case]
    rs = np.random.RandomState(1400 + sorted(CASES).index(case))
    X = rs.uniform(0, 1, (ROWS, widths[0])).astype(np.float32)
    Y = rs.uniform(0, 1, (ROWS, widths[-1]))
    if n_sig < widths[-1]:
        Y[:, n_sig:] /= Y[:, n_sig:].sum(axis=1, keepdims=True)
    return X, Y.astype(np.float32)


def flat(params, widths):
    return np.concatenate([np.asarray(params[k]).reshape(-1) for k, _ in shapes(widths)])


def unflat(vec, widths):
    out, off = {}, 0
    for k, s in shapes(widths):
        n = int(np.prod(s))
        out[k] = np.asarray(vec[off:off + n]).reshape(s)
        off += n
    return out


def forward(params, widths, n_sig, x, cache=None):
    L = len(widths) - 1
    a = np.asarray(x, dtype=np.float64)
    for i in range(L):
        z = a @ np.asarray(params[f"lin{i + 1}.weight"], dtype=np.float64).T + np.asarray(params[f"lin{i + 1}.bias"], dtype=np.float64)
        if cache is not None:
            cache.append((a, z))
        a = np.maximum(z, 0.0) if i + 1 < L else z
    out = np.empty_like(a)
    out[:, :n_sig] = 1.0 / (1.0 + np.exp(-a[:, :n_sig]))
    if n_sig < a.shape[1]:
        e = np.exp(a[:, n_sig:] - a[:, n_sig:].max(axis=1, keepdims=True))
        out[:, n_sig:] = e / e.sum(axis=1, keepdims=True)
    return out


def relu_margin(params, widths, n_sig, x):
    """min over the hidden layers of min|z| / max|z| (z = the pre-activations of the ReLU)."""
    cache = []
    forward(params, widths, n_sig, x, cache)
    return min(float(np.abs(z).min() / np.abs(z).max()) for _, z in cache[:-1])


def loss_grad(params, widths, n_sig, x, y):
    """(mean((y - net(x))^2), {key: gradient}) in float64."""
    L = len(widths) - 1
    cache = []
    out = forward(params, widths, n_sig, x, cache)
    y = np.asarray(y, dtype=np.float64)
    loss = float(np.mean((y - out) ** 2))
    g = 2.0 * (out - y) / out.size
    d = np.empty_like(g)
    s = out[:, :n_sig]
    d[:, :n_sig] = g[:, :n_sig] * s * (1.0 - s)
    if n_sig < out.shape[1]:
        p, gp = out[:, n_sig:], g[:, n_sig:]
        d[:, n_sig:] = p * (gp - (gp * p).sum(axis=1, keepdims=True))
    grads = {}
    for i in range(L - 1, -1, -1):
        a, z = cache[i]
        grads[f"lin{i + 1}.weight"] = d.T @ a
        grads[f"lin{i + 1}.bias"] = d.sum(axis=0)
        if i > 0:
            d = (d @ np.asarray(params[f"lin{i + 1}.weight"], dtype=np.float64)) * (cache[i - 1][1] > 0)
    return loss, grads


def adam_steps(params, widths, n_sig, X, Y, batches=STEP_BATCHES, lr=LR, beta1=0.9, beta2=0.999, eps=1e-8):
    """torch.optim.Adam (no weight decay, no amsgrad) over the given row ranges; returns (parameters after the last step, losses)."""
    p = {k: np.asarray(v, dtype=np.float64).copy() for k, v in params.items()}
    m = {k: np.zeros_like(v) for k, v in p.items()}
    v2 = {k: np.zeros_like(v) for k, v in p.items()}
    losses = []
    for t, (lo, hi) in enumerate(batches, start=1):
        loss, g = loss_grad(p, widths, n_sig, X[lo:hi], Y[lo:hi])
        losses.append(loss)
        for k in p:
            m[k] = beta1 * m[k] + (1 - beta1) * g[k]
            v2[k] = beta2 * v2[k] + (1 - beta2) * g[k] * g[k]
            denom = np.sqrt(v2[k]) / np.sqrt(1 - beta2 ** t) + eps
            p[k] = p[k] - (lr / (1 - beta1 ** t)) * m[k] / denom
    return p, losses
