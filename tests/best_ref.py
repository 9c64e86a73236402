"""CPU restatement of repeated sampling's selection rule (diffsg_amd/repeated.py, csrc/dsg_best.hpp), built from the
decoders and objectives of oracle/ddpm_oracle.py.

A round is one [B, D] tensor, decoded as the problem's decoder decodes it today (MSR / NU: min-max over that round only).
Per condition the round with the strictly best objective wins, the lowest round on equal objectives; a round whose objective
is not finite never wins; a condition without a finite round gets round -1 and round 0's row and objective."""
import torch

from oracle import ddpm_oracle as O

MAXIMISE = {"msr": True, "co": False, "nu": True}


def decode_and_score(problem, Yk, X, **p):
    """(decoded solution [B, D], objective [B]) of one round."""
    if problem == "msr":
        sol = p["W"] * O.msr_decode(Yk)
        return sol, O.msr_rate(sol, X)
    if problem == "co":
        sol = O.co_decode(Yk)
        return sol, O.co_cost(X, sol)
    if problem == "nu":
        sol = O.nu_decode(Yk, p["width"], p["height"], p["p_sum"])
        return sol, O.nu_rate(sol, X)
    raise ValueError(problem)


def best_of_ref(problem, Y, X, out=None, round0=0, **params):
    """(solution [B, D], objective [B], round [B] int32, objectives [n, B]) of the rounds Y [n, B, D].  `out` = an earlier
    (solution, objective, round, ...) to accumulate into (not modified): indices are then stored as round0 + k."""
    n = Y.shape[0]
    if out is None:
        sol = obj = None
        rnd = torch.full((Y.shape[1],), -1, dtype=torch.int32)
    else:
        sol, obj, rnd = out[0].clone(), out[1].clone(), out[2].clone()
    objs = []
    for k in range(n):
        s, o = decode_and_score(problem, Y[k], X, **params)
        s, o = s.to(torch.float32), o.to(torch.float32)
        objs.append(o)
        if sol is None:                                  # round 0 is the answer until a finite round shows up
            sol, obj = s.clone(), o.clone()
            rnd = torch.where(torch.isfinite(o), torch.tensor(round0, dtype=torch.int32), rnd)
            continue
        better = (o > obj) if MAXIMISE[problem] else (o < obj)
        take = torch.isfinite(o) & ((rnd < 0) | better)
        sol = torch.where(take[:, None], s, sol)
        obj = torch.where(take, o, obj)
        rnd = torch.where(take, torch.tensor(round0 + k, dtype=torch.int32), rnd)
    return sol, obj, rnd, torch.stack(objs) if objs else torch.zeros(0, Y.shape[1])
