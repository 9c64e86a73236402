"""Float64 numpy restatement of one PPO batch of the baseline (actor and critic forward, Gaussian action, log-probability, the
CO / MSR / NU environment step, clipped-surrogate and value losses, every gradient) and of torch.optim.Adam, written for this
project from the operator's description.  tests/test_ppo_cpu.py holds it to the goldens recorded from torch
and the reference's classes (tests/golden/make_ppo_goldens.py); the shapes and inputs of the golden cases live here so that the
generator and the tests share them."""
import numpy as np

HIDDEN = (64, 16, 32)
# name: state_dim, action_dim, environment, the environment's scalars
CASES = {
    "co3": dict(S=9, A=3, env="co", cfg=dict(scaler_min=0.0, scaler_max=10.0)),
    "msr3": dict(S=3, A=3, env="msr", cfg=dict(scaler_min=0.1, scaler_max=2.0, W=10.0)),
    "msr80": dict(S=80, A=80, env="msr", cfg=dict(scaler_min=0.1, scaler_max=2.0, W=10.0)),
    # P_sum is far above the shipped 18: with every user at the origin and 18 mW the rates are ~3e-4, the reward is 10 to three digits
    # whatever the action, and a wrong decoder or rate would not show in it.  At 1e5 the rates are of order 1 and the reward follows them.
    "nu3": dict(S=6, A=5, env="nu", cfg=dict(width=400.0, height=400.0, P_sum=1.0e5)),
}
ROWS = 70
STEP_BATCHES = ((0, 64), (64, 70), (0, 70))     # the three Adam steps of the goldens: an epoch of 70 rows at batch 64, then one batch of 70
LR = 0.005
OFFSET = {"co": 0.1, "msr": 0.01, "nu": 0.1}
RETURN_CONST = float(np.float32(0.99 * 3.8))    # calc_advantage's gamma * 3.8 as float32 arithmetic sees it
LOG_SQRT_2PI = float(np.log(np.sqrt(2 * np.pi)))
RATIO_MARGIN = 1e-4         # (a) no ratio within this of 0.8 / 1.2
CO_MARGIN = 1e-4            # (b) no softmaxed action or target within this of the 0.1 offload threshold
KAPPA_MAX = 10.0            # (c) (|c| + |gt|) / (|c - gt| + offset) on every row


def shapes(S, A, hidden=HIDDEN):
    """The reference's state-dict order: log_std, critic.{0,2,4,6}, actor.{0,2,4,6}."""
    out = [("log_std", (1, A))]
    for net, last in (("critic", 1), ("actor", A)):
        w = (S,) + tuple(hidden) + (last,)
        for i in range(4):
            out.append((f"{net}.{2 * i}.weight", (w[i + 1], w[i])))
            out.append((f"{net}.{2 * i}.bias", (w[i + 1],)))
    return out


def case_shapes(case):
    return shapes(CASES[case]["S"], CASES[case]["A"])


def synth_state(case, seed, std=0.3):
    """The "trained-like" state: every weight and bias ~ N(0, std^2), log_std ~ U(-0.5, 0.3), float32."""
    rs = np.random.RandomState(seed)
    out = {k: (rs.standard_normal(s) * std).astype(np.float32) for k, s in case_shapes(case)}
    out["log_std"] = rs.uniform(-0.5, 0.3, out["log_std"].shape).astype(np.float32)
    return out


def inputs(case, seed=0):
    """X [ROWS][S], Y [ROWS][A], noise, noise2 [ROWS][A] (float32).  The targets are made poor on purpose, so that the objective of
    the action and of the target stay apart and the reward does not amplify an objective's rounding (condition (c)):
    CO targets keep every node local, MSR and NU targets spend 5 % of the power budget."""
    c = CASES[case]
    S, A, env = c["S"], c["A"], c["env"]
    rs = np.random.RandomState(1500 + 100 * seed + sorted(CASES).index(case))
    X = rs.uniform(0, 1, (ROWS, S))
    if env == "co":
        X[:, 0::3] *= 0.1                           # local costs small, transfer and execution costs large
        X[:, 1::3] = 0.3 + 0.7 * X[:, 1::3]
        X[:, 2::3] = 0.3 + 0.7 * X[:, 2::3]
        Y = rs.uniform(0, 0.09, (ROWS, A))
    elif env == "msr":
        Y = rs.uniform(0, 1, (ROWS, A))
        Y = 0.05 * Y / Y.sum(axis=1, keepdims=True)
    else:
        Y = rs.uniform(0, 1, (ROWS, A))
        Y[:, 2:] /= Y[:, 2:].sum(axis=1, keepdims=True)
        Y[:, 0] *= c["cfg"]["width"]
        Y[:, 1] *= c["cfg"]["height"]
        Y[:, 2:] *= 0.05 * c["cfg"]["P_sum"]
    noise = rs.standard_normal((ROWS, A))
    # The log-probability of an action drawn with noise n is -n^2 / 2 - log_std - const whatever mu is, so the ratio of the golden's
    # third step (old_logp = the first epoch's new_logp) is exp(-(n2^2 - n^2) / 2): noise2 is built so that this is exp(-u), u gapped.
    u = rs.uniform(-0.4, 0.4, (ROWS, A))
    u = _gapped(np.where(noise ** 2 + 2 * u < 0.01, np.abs(u), u))       # keep n2^2 = n^2 + 2 u positive
    noise2 = -np.sign(noise) * np.sqrt(noise ** 2 + 2 * u)
    return tuple(a.astype(np.float32) for a in (X, Y, noise, noise2))


def _gapped(u):
    """u with the values within 0.01 of -log(0.8) / -log(1.2) moved up by 0.03: exp(-u) then keeps clear of the clip bounds by far more
    than RATIO_MARGIN, however many elements a batch has (a generator's property, not a margin of the tests)."""
    for b in (-np.log(0.8), -np.log(1.2)):
        u = np.where(np.abs(u - b) < 0.01, u + 0.03, u)
    return u


def make_old_logp(case, params, x, noise, seed=0):
    """An old log-probability near the new one: new_logp + u, u ~ U(-0.4, 0.4) gapped, so that the ratios exp(-u) fall on both
    sides of the clip range and inside it."""
    rs = np.random.RandomState(1700 + 100 * seed + sorted(CASES).index(case))
    mu, _ = forward(params, x)
    _, logp = action(params, mu, noise)
    return (logp + _gapped(rs.uniform(-0.4, 0.4, logp.shape))).astype(np.float32)


def flat(params, case):
    return np.concatenate([np.asarray(params[k]).reshape(-1) for k, _ in case_shapes(case)])


def unflat(vec, case):
    out, off = {}, 0
    for k, s in case_shapes(case):
        n = int(np.prod(s))
        out[k] = np.asarray(vec[off:off + n]).reshape(s)
        off += n
    return out


def _net(params, net, x, cache=None):
    a = np.asarray(x, dtype=np.float64)
    for i in range(4):
        z = a @ np.asarray(params[f"{net}.{2 * i}.weight"], dtype=np.float64).T + np.asarray(params[f"{net}.{2 * i}.bias"], dtype=np.float64)
        if cache is not None:
            cache.append(a)
        a = np.tanh(z) if i < 3 else z
    return a


def forward(params, x):
    """(mu [rows][A], value [rows])."""
    return _net(params, "actor", x), _net(params, "critic", x)[:, 0]


def action(params, mu, noise):
    """(a = noise * std + mu, Normal(mu, std).log_prob(a))."""
    ls = np.asarray(params["log_std"], dtype=np.float64)
    std = np.exp(ls)
    a = np.asarray(noise, dtype=np.float64) * std + mu
    d = a - mu
    return a, -(d ** 2) / (2 * std ** 2) - ls - LOG_SQRT_2PI


def softmax(a):
    e = np.exp(a - a.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def co_cost(xr, y):
    D = y > 0.1
    ysum, dsum = (y * D).sum(axis=1), D.sum(axis=1)
    spread = (1.0 - ysum) / np.where(dsum == 0, 0.00001, dsum)
    share = np.where(D, y + spread[:, None], 1.0)
    return np.where(D, xr[:, 1::3] + xr[:, 2::3] / share, xr[:, 0::3]).sum(axis=1)


def nu_rate_origin(yd):
    """rate_calc with every user at the origin: equal gains, so the stable order is 0, 1, 2 ..."""
    sigma_sq, rou_0, H = 110.0, 60.0, 150.0
    h2 = rou_0 / (H * H + yd[:, 0] ** 2 + yd[:, 1] ** 2)
    pw = yd[:, 2:]
    before = np.cumsum(pw, axis=1) - pw
    sinr = pw / (before + (sigma_sq / h2)[:, None])
    sinr[:, 0] = pw[:, 0] * h2 / sigma_sq
    return np.log2(1.0 + sinr).sum(axis=1)


def objectives(case, x, act, y):
    """(objective of the softmaxed action, objective of the target) per row."""
    c = CASES[case]
    cfg, x, y = c["cfg"], np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if c["env"] == "co":
        xr = x * float(np.float32(cfg["scaler_max"] - cfg["scaler_min"])) + cfg["scaler_min"]
        return co_cost(xr, act), co_cost(xr, y)
    if c["env"] == "msr":
        g = x * float(np.float32(cfg["scaler_max"] - cfg["scaler_min"])) + float(np.float32(cfg["scaler_min"]))
        return np.log2(1.0 + act * cfg["W"] * g).sum(axis=1), np.log2(1.0 + y * cfg["W"] * g).sum(axis=1)
    lo, hi = act[:, :2].min(), act[:, :2].max()                 # over the WHOLE batch
    dec = np.empty_like(act)
    dec[:, 0] = (act[:, 0] - lo) / (hi - lo) * cfg["width"]
    dec[:, 1] = (act[:, 1] - lo) / (hi - lo) * cfg["height"]
    dec[:, 2:] = softmax(act[:, 2:]) * cfg["P_sum"]
    return nu_rate_origin(dec), nu_rate_origin(y)


def batch(params, case, x, y, old_logp, noise):
    """One batch in float64: a dict with mu, value, new_logp, ratio, act, cost, gt, kappa, reward, actor_loss, critic_loss and
    grads {key: gradient of actor_loss + critic_loss} (log_std: zeros -- not differentiated here)."""
    env = CASES[case]["env"]
    ca, cc = [], []
    mu, value = _net(params, "actor", x, ca), _net(params, "critic", x, cc)[:, 0]
    B, A = mu.shape
    ls = np.asarray(params["log_std"], dtype=np.float64)
    var = np.exp(ls) ** 2
    a, logp = action(params, mu, noise)
    d = a - mu
    ratio = np.exp(logp - np.asarray(old_logp, dtype=np.float64))
    act = softmax(a)
    cost, gt = objectives(case, x, act, y)
    reward = 1.0 / (np.abs(cost - gt) + OFFSET[env])
    ret = reward + RETURN_CONST
    adv = (ret - value)[:, None]                    # NOT detached: the critic sees the actor loss too
    cr = np.clip(ratio, 0.8, 1.2)
    u, cl = ratio * adv, cr * adv
    actor_loss = -np.minimum(u, cl).mean()
    critic_loss = np.mean((value - ret) ** 2)
    wu = np.where(u < cl, 1.0, np.where(u == cl, 0.5, 0.0))       # torch.min's backward: ties half and half
    wc = 1.0 - wu
    inside = (ratio >= 0.8) & (ratio <= 1.2)                        # clamp passes the gradient at the bound itself
    dr = wu * adv + wc * adv * inside
    dadv = wu * ratio + wc * cr
    dmu = -dr * ratio * d / var / (B * A)
    dval = dadv.sum(axis=1) / (B * A) + 2.0 * (value - ret) / B
    grads = {"log_std": np.zeros_like(ls)}
    for net, cache, delta in (("actor", ca, dmu), ("critic", cc, dval[:, None])):
        for i in range(3, -1, -1):
            grads[f"{net}.{2 * i}.weight"] = delta.T @ cache[i]
            grads[f"{net}.{2 * i}.bias"] = delta.sum(axis=0)
            if i > 0:
                delta = (delta @ np.asarray(params[f"{net}.{2 * i}.weight"], dtype=np.float64)) * (1.0 - cache[i] ** 2)
    kappa = (np.abs(cost) + np.abs(gt)) / (np.abs(cost - gt) + OFFSET[env])
    return dict(mu=mu, value=value, new_logp=logp, ratio=ratio, act=act, cost=cost, gt=gt, kappa=kappa, reward=reward,
                actor_loss=float(actor_loss), critic_loss=float(critic_loss), grads=grads)


def conditions(case, res, y):
    """The golden generator's conditions (a) - (c) on one batch's result; (d) needs the reference's argsort and lives there."""
    bad = []
    if min(np.abs(res["ratio"] - 0.8).min(), np.abs(res["ratio"] - 1.2).min()) < RATIO_MARGIN:
        bad.append("ratio at a clip bound")
    if CASES[case]["env"] == "co" and min(np.abs(res["act"] - 0.1).min(), np.abs(np.asarray(y, dtype=np.float64) - 0.1).min()) < CO_MARGIN:
        bad.append("action or target at the offload threshold")
    if res["kappa"].max() > KAPPA_MAX:
        bad.append(f"kappa {res['kappa'].max():.1f}")
    return bad


def adam_steps(params, case, X, Y, old_logp, noise, noise2, lr=LR, beta1=0.9, beta2=0.999, eps=1e-8, on_batch=None):
    """torch.optim.Adam over STEP_BATCHES on every parameter but log_std.  The first two batches are one epoch (noise, old_logp);
    their new_logp is the third batch's old_logp, as the reference hands it from epoch to epoch; the third batch draws noise2.
    Returns (parameters, [(actor loss, critic loss)] per step)."""
    p = {k: np.asarray(v, dtype=np.float64).copy() for k, v in params.items()}
    m = {k: np.zeros_like(v) for k, v in p.items()}
    v2 = {k: np.zeros_like(v) for k, v in p.items()}
    old = np.asarray(old_logp, dtype=np.float64).copy()
    nxt = old.copy()
    losses = []
    for t, (lo, hi) in enumerate(STEP_BATCHES, start=1):
        if t == 3:
            old = nxt
        res = batch(p, case, X[lo:hi], Y[lo:hi], old[lo:hi], (noise if t < 3 else noise2)[lo:hi])
        if on_batch is not None:
            on_batch(t, res, Y[lo:hi])
        nxt[lo:hi] = res["new_logp"]
        losses.append((res["actor_loss"], res["critic_loss"]))
        for k in p:
            if k == "log_std":
                continue
            g = res["grads"][k]
            m[k] = beta1 * m[k] + (1 - beta1) * g
            v2[k] = beta2 * v2[k] + (1 - beta2) * g * g
            denom = np.sqrt(v2[k]) / np.sqrt(1 - beta2 ** t) + eps
            p[k] = p[k] - (lr / (1 - beta1 ** t)) * m[k] / denom
    return p, losses
