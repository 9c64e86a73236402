"""Timestep laws: training on a non-uniform draw of ts, with a loss weight per timestep, and the loss by timestep.

A `TrainLaw` is what the training step needs beyond the reference's rule `ts ~ U{0..T-1}`, unweighted mean:

  p      float64 [T] or None   the probability of every trained timestep, as given (not normalised);
  cdf24  int64 [T] or None     its integer CDF on the 24-bit grid -- what the library draws from:  u24 = (Philox word) >> 8 and
                               ts = #{k : cdf24[k] <= u24}, an upper bound in integers, which `np.searchsorted(cdf24, u24, "right")`
                               restates exactly.  None: the uniform draw, exactly the expression without a law;
  w      float32 [T] or None   the loss weight of every timestep: loss = sum_r w[ts_r] sum_f (eps_hat - eps)^2 / (B D).  None: all 1.

Constructors: `law(ddpm_or_T, p, w)`, `on_plan(ddpm, plan_or_taus, w)` (uniform on the steps a `steps.StepPlan` visits: the fine-tuning
law of K-step sampling), `min_snr(ddpm, gamma, p)` (Hang et al. 2023: w_t = min(SNR_t, gamma) / SNR_t) and `with_weights(law, w)`.
A law is set on a model as `ddpm.train_law = law`; `ddpm.loss_report(True)` turns the loss by timestep on.  The pinned entry points take
both through the context manager `training(law=..., report=...)`.
"""
from __future__ import annotations

import contextlib
from dataclasses import dataclass
from typing import Optional

import numpy as np

GRID = 1 << 24      # the draw's resolution: u24 has 24 bits


@dataclass(frozen=True, eq=False)
class TrainLaw:
    p: Optional[np.ndarray] = None        # float64 [T], read-only
    w: Optional[np.ndarray] = None        # float32 [T], read-only
    cdf24: Optional[np.ndarray] = None    # int64 [T], read-only
    T: Optional[int] = None               # taken from the arrays when not given; a law with no array at all (the reference's rule) has none

    def __post_init__(self):
        for a in (self.p, self.w, self.cdf24):
            if a is not None:
                a.setflags(write=False)
                if self.T is None:
                    object.__setattr__(self, "T", int(a.shape[0]))
                elif a.shape[0] != self.T:
                    raise ValueError(f"train law: an array of {a.shape[0]} entries for T = {self.T}")

    @property
    def support(self):
        """The timesteps the law can draw (all T without a CDF)."""
        if self.cdf24 is None:
            return tuple(range(self.T))
        prev = np.concatenate(([0], self.cdf24[:-1]))
        return tuple(int(k) for k in np.nonzero(self.cdf24 > prev)[0])


def _T_of(ddpm_or_T):
    return int(ddpm_or_T if isinstance(ddpm_or_T, (int, np.integer)) else ddpm_or_T.T)


def _weights(w, T):
    if w is None:
        return None
    if hasattr(w, "detach"):              # a torch tensor
        w = w.detach().cpu().numpy()
    w = np.array(w, dtype=np.float64).reshape(-1)
    if w.shape[0] != T:
        raise ValueError(f"train law: {w.shape[0]} weights for T = {T} timesteps")
    if not np.isfinite(w).all():
        raise ValueError("train law: the weights must be finite")
    if (w < 0).any():
        raise ValueError("train law: the weights must be >= 0")
    with np.errstate(over="ignore"):
        w32 = w.astype(np.float32)
    if not np.isfinite(w32).all():
        raise ValueError("train law: the weights must be finite in float32")
    return w32


def cdf24_of(p):
    """cdf24[k] = floor(2^24 cumsum(p)[k] / sum(p) + 0.5) in float64, the last entry forced to 2^24; refuses a step with p > 0 whose
    interval rounds to empty."""
    p = np.asarray(p, dtype=np.float64)
    total = p.sum()
    cdf = np.floor(GRID * np.cumsum(p) / total + 0.5).astype(np.int64)
    cdf = np.minimum(cdf, GRID)
    cdf[-1] = GRID
    cdf = np.maximum.accumulate(cdf)
    prev = np.concatenate(([0], cdf[:-1]))
    empty = np.nonzero((p > 0) & (cdf == prev))[0]
    if empty.size:
        k = int(empty[0])
        raise ValueError(f"train law: timestep {k} has p = {p[k]:g} > 0, but its interval of the CDF is empty at the draw's resolution "
                         f"of 2^-24 (p / sum(p) = {p[k] / total:.3g}): it would never be drawn")
    return cdf


def law(ddpm_or_T, p=None, w=None):
    """The law with probabilities `p` (any non-negative float64 [T] with a positive sum; None: uniform) and weights `w` ([T], finite,
    >= 0; None: all 1)."""
    T = _T_of(ddpm_or_T)
    if T < 1:
        raise ValueError(f"train law: T = {T}")
    cdf = None
    if p is not None:
        if hasattr(p, "detach"):
            p = p.detach().cpu().numpy()
        p = np.array(p, dtype=np.float64).reshape(-1)
        if p.shape[0] != T:
            raise ValueError(f"train law: {p.shape[0]} probabilities for T = {T} timesteps")
        if not np.isfinite(p).all():
            raise ValueError("train law: the probabilities must be finite")
        if (p < 0).any():
            raise ValueError("train law: the probabilities must be >= 0")
        if p.sum() == 0:
            raise ValueError("train law: the probabilities sum to 0")
        cdf = cdf24_of(p)
    return TrainLaw(p, _weights(w, T), cdf, T)


def on_plan(ddpm, plan_or_taus, w=None):
    """Uniform on the trained timesteps a step plan visits (`plan.taus`, or the taus themselves), 0 elsewhere."""
    T = _T_of(ddpm)
    taus = tuple(int(t) for t in getattr(plan_or_taus, "taus", plan_or_taus))
    if not taus or min(taus) < 0 or max(taus) > T - 1 or len(set(taus)) != len(taus):
        raise ValueError(f"on_plan: taus must be distinct integers in [0, {T - 1}]")
    p = np.zeros(T, dtype=np.float64)
    p[list(taus)] = 1.0
    return law(T, p, w)


def min_snr_weights(alphas_cumprod, gamma=5.0):
    """float32 [T]: min(SNR_t, gamma) / SNR_t with SNR = acp / (1 - acp), in float64 from the float32 `alphas_cumprod`, cast once."""
    acp = np.asarray(alphas_cumprod, dtype=np.float32).astype(np.float64)
    snr = acp / (1.0 - acp)
    return (np.minimum(snr, float(gamma)) / snr).astype(np.float32)


def min_snr(ddpm, gamma=5.0, p=None):
    """Min-SNR-gamma loss weights (for an eps-prediction loss) on the model's schedule; `p` as in `law`."""
    if not float(gamma) > 0:
        raise ValueError(f"min_snr: gamma must be > 0, got {gamma}")
    return law(ddpm, p, min_snr_weights(ddpm.alphas_cumprod.detach().cpu().numpy(), gamma))


def with_weights(base, w):
    """The law `base` with the weights `w` (None: all 1) and everything else shared."""
    T = base.T if base.T is not None or w is None else int(np.asarray(w).reshape(-1).shape[0])
    return TrainLaw(base.p, _weights(w, T), base.cdf24, T)


def expected_ts(cdf24, u24):
    """ts of the 24-bit draws `u24` under `cdf24`: the number of entries <= u24."""
    return np.searchsorted(np.asarray(cdf24, dtype=np.int64), np.asarray(u24, dtype=np.int64), side="right")


# ---------------------------------------------------------------- the options of the pinned entry points
_ACTIVE = None


@contextlib.contextmanager
def training(law=None, report=False):
    """Inside the context, `entry.train` (and so `train_ddpm_*` / `entry.train_ddpm`) sets `law` and the loss report on the model it
    builds, right after `build(device)`.  `law`: a `TrainLaw`, or a callable `ddpm -> TrainLaw` (`on_plan` and `min_snr` need the built
    model).  Outside the context nothing is read."""
    global _ACTIVE
    prev, _ACTIVE = _ACTIVE, (law, bool(report))
    try:
        yield
    finally:
        _ACTIVE = prev


def apply_active(ddpm):
    """What `entry.train` calls on the built model: the options of the enclosing `training()` context, if any."""
    if _ACTIVE is None:
        return
    lw, report = _ACTIVE
    if lw is not None:
        ddpm.train_law = lw(ddpm) if callable(lw) else lw
    if report:
        ddpm.loss_report(True)
