"""Repeated sampling: n candidate solutions per condition, the best one kept on the device.

DiffSG's method is to draw from the learned solution distribution many times and keep the best draw.  `best_of` decodes and
scores `n` rounds of raw sampler output and picks, per condition, the round with the strictly best finite objective (one
call into libdiffsg_hip.so, csrc/dsg_best.hpp); `DDPMCore.sample_best` (ddpm.py) samples the rounds in groups and feeds them
through it.  Like the rest of the package there is no CPU path (the CPU restatement used by the tests is tests/best_ref.py).

Per round the values are those of `decode.msr_decode` / `msr_rate`, `co_decode` / `co_cost`, `nu_decode` / `nu_rate` on that
round's `[B, D]` tensor, bit for bit:

    problem   solution row                            objective                   direction
    "msr"     W * msr_decode(Y[k])                    msr_rate(solution, X)       maximise
    "co"      co_decode(Y[k])                         co_cost(X, solution)        minimise
    "nu"      nu_decode(Y[k], width, height, p_sum)   nu_rate(solution, X)        maximise
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import torch

from . import _lib
from .decode import _dev

PROBLEMS = {"msr": 0, "co": 1, "nu": 2}          # DSG_PROBLEM_* of include/diffsg.h


class BestOf(NamedTuple):
    solution: torch.Tensor                # [B, D]  the winner's decoded row (round 0's where no round is finite)
    objective: torch.Tensor               # [B]     its objective
    round: torch.Tensor                   # [B]     int32 index of the winning round, -1 where no round is finite
    objectives: Optional[torch.Tensor]    # [n, B]  every round's objective (return_objectives=True), else None


def _problem_code(problem):
    if isinstance(problem, str):
        if problem.lower() not in PROBLEMS:
            raise ValueError(f"best_of: unknown problem {problem!r} (one of {sorted(PROBLEMS)})")
        return PROBLEMS[problem.lower()]
    if int(problem) not in PROBLEMS.values():
        raise ValueError(f"best_of: unknown problem code {problem!r}")
    return int(problem)


def best_of(problem, Y, X, *, W=None, width=None, height=None, p_sum=None, out=None, round0=0, return_objectives=False) -> BestOf:
    """The best of the `n` rounds `Y[n, B, D]` per condition; `X` holds the unscaled features the objective reads (MSR gains
    `[B, D]`, CO costs `[B, 3D]`, NU user positions `[B, 2(D-2)]`).  Ties keep the lowest round, a non-finite objective never
    wins, a condition without a finite round gets `round = -1` and round 0's row.

    `out` is an earlier `BestOf` of the same conditions to accumulate into (updated in place and returned): only strictly
    better candidates replace its entries, their indices are stored as `round0 + k`.  With `return_objectives` the rounds'
    objectives are appended to `out.objectives`."""
    code = _problem_code(problem)
    Y, X = _dev(Y, X)
    if Y.dim() != 3:
        raise ValueError(f"best_of: Y is {tuple(Y.shape)}, expected (rounds, conditions, columns)")
    n, B, D = Y.shape
    want = {0: (B, D), 1: (B, 3 * D), 2: (B, 2 * (D - 2))}[code]
    if tuple(X.shape) != want:
        raise ValueError(f"best_of: X is {tuple(X.shape)}, expected {want}")
    if code == 0:
        if W is None:
            raise ValueError("best_of: the MSR problem needs W")
        params = (ctypes.c_float * 1)(float(W))
    elif code == 2:
        if width is None or height is None or p_sum is None:
            raise ValueError("best_of: the NU problem needs width, height and p_sum")
        params = (ctypes.c_float * 3)(float(width), float(height), float(p_sum))
    else:
        params = None
    dev = Y.device
    if out is None:
        if n == 0:
            raise ValueError("best_of: no rounds and nothing to accumulate into")
        sol = torch.empty(B, D, device=dev, dtype=torch.float32)
        obj = torch.empty(B, device=dev, dtype=torch.float32)
        rnd = torch.empty(B, device=dev, dtype=torch.int32)
    else:
        sol, obj, rnd = out.solution, out.objective, out.round
        if (tuple(sol.shape) != (B, D) or tuple(obj.shape) != (B,) or tuple(rnd.shape) != (B,) or sol.dtype != torch.float32
                or obj.dtype != torch.float32 or rnd.dtype != torch.int32 or not (sol.is_contiguous() and obj.is_contiguous()
                                                                                  and rnd.is_contiguous())
                or any(t.device != dev for t in (sol, obj, rnd))):
            raise ValueError("best_of: `out` does not match Y (an earlier BestOf of the same conditions on the same device)")
    objs = torch.empty(n, B, device=dev, dtype=torch.float32) if return_objectives else None
    with torch.cuda.device(dev):       # (the library checks the arguments and launches nothing for B == 0 or n == 0)
        _lib.check(_lib.lib().dsg_best_of(code, _lib.ptr(Y), _lib.ptr(X), n, B, D, params, _lib.ptr(sol), _lib.ptr(obj), _lib.ptr(rnd),
                                          _lib.ptr(objs), 0 if out is None else 1, int(round0), _lib.stream_ptr()))
    if return_objectives and out is not None and out.objectives is not None:
        objs = torch.cat([out.objectives, objs])
    return BestOf(sol, obj, rnd, objs)
