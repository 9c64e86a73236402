"""Repeated sampling, host side: the selection rules of the CPU restatement (tests/best_ref.py) on hand-made cases, the
C-ABI surface of dsg_best_of, and the refusal to run without a device.  No compute call is made here."""
import os
import re

import pytest
import torch

from _util import ROOT
from best_ref import best_of_ref

NAN = float("nan")


def _msr_case():
    """3 rounds x 4 conditions x 2 columns, gains 1, W = 2.  Within a round the min-max maps every entry to 0 or 1, so a
    row is either flat (softmax 0.5 / 0.5) or one-sided; the flat row has the higher sum rate."""
    flat, skew = [0.0, 0.0], [0.0, 1.0]
    Y = torch.tensor([[flat, skew, skew, skew],
                      [flat, flat, skew, skew],
                      [skew, flat, flat, skew]], dtype=torch.float32)
    # every round holds a 0 and a 1 somewhere, so its min-max is (0, 1): add an anchor condition that is never compared
    anchor = torch.tensor([[[0.0, 1.0]]] * 3)
    return torch.cat([Y, anchor], dim=1), torch.ones(5, 2)


def test_equal_rounds_keep_the_lower_index():
    Y, G = _msr_case()
    sol, obj, rnd, objs = best_of_ref("msr", Y, G, W=2.0)
    assert objs.shape == (3, 5)
    assert float(objs[0, 0]) == float(objs[1, 0]) > float(objs[2, 0])      # condition 0: rounds 0 and 1 tie, both beat round 2
    assert rnd.dtype == torch.int32 and rnd[:4].tolist() == [0, 1, 2, 0]   # first of the equal rounds; condition 3: all equal
    assert torch.equal(obj, objs.max(0).values)
    assert torch.equal(sol[0], torch.tensor([1.0, 1.0]))                  # W * softmax of a flat row


def test_a_nan_round_never_wins_and_an_all_nan_condition_gives_minus_one():
    """Gains (-0.8, 1): the allocation W * softmax((1, 0)) = (1.46, 0.54) makes 1 + p * g negative, so its rate is NaN; the
    flat row scores -1.32 and the row (0, 1) scores 0.49."""
    flat, skew, bad = [0.0, 0.0], [0.0, 1.0], [1.0, 0.0]
    Y = torch.tensor([[bad, bad, bad],
                      [flat, skew, bad],
                      [skew, skew, bad]], dtype=torch.float32)
    G = torch.tensor([[-0.8, 1.0]] * 3)
    sol, obj, rnd, objs = best_of_ref("msr", Y, G, W=2.0)
    assert torch.isnan(objs[0]).all() and torch.isnan(objs[:, 2]).all() and torch.isfinite(objs[1:, :2]).all()
    assert rnd.tolist() == [2, 1, -1]                     # the NaN round 0 never wins; equal rounds 1, 2 keep 1; no finite round
    assert torch.equal(obj[:2], objs[1:, :2].max(0).values) and torch.isnan(obj[2])
    assert torch.equal(sol[2], 2.0 * torch.softmax(torch.tensor(bad), 0))   # round 0's row
    # the same rounds in the other order: a later NaN does not displace a finite best
    _, _, rnd, _ = best_of_ref("msr", Y.flip(0), G, W=2.0)
    assert rnd.tolist() == [0, 0, -1]
    # CO minimises, and a later equal cost does not displace the first
    Yc = torch.tensor([[[3.0, 0.0, 0.0]], [[0.0, 3.0, 0.0]], [[3.0, 0.0, 0.0]]])
    Xc = torch.tensor([[1.0, 5.0, 1.0, 1.0, 2.0, 1.0, 1.0, 1.0, 1.0]])
    _, objc, rndc, objsc = best_of_ref("co", Yc, Xc)
    assert float(objsc[0, 0]) == float(objsc[2, 0]) > float(objsc[1, 0]) and rndc.tolist() == [1] and float(objc[0]) == float(objsc[1, 0])
    assert best_of_ref("co", Yc[[0, 2]], Xc)[2].tolist() == [0]


@pytest.mark.parametrize("problem", ["msr", "co", "nu"])
def test_accumulating_in_two_groups_is_the_one_shot_result(problem):
    g = torch.Generator().manual_seed(3)
    n, B = 7, 50
    if problem == "msr":
        Y, X, p = torch.randn(n, B, 6, generator=g) * 3, torch.rand(B, 6, generator=g) * 2 + 0.5, {"W": 20.0}
        X[5, 0] = -0.3           # NaN whenever column 0 gets more than a sixth of the 20 units
        X[9] = -100.0            # never finite
    elif problem == "co":
        Y, X, p = torch.randn(n, B, 3, generator=g), torch.rand(B, 9, generator=g) * 10, {}
        Y[:, ::7] = -20.0        # dead rows: every round of these conditions costs the same -> ties
    else:
        Y, X, p = torch.randn(n, B, 5, generator=g), torch.rand(B, 6, generator=g) * 400, {"width": 400, "height": 400, "p_sum": 18.0}
        X[9] = NAN               # never finite
    one = best_of_ref(problem, Y, X, **p)
    for cut in (1, 3, 6):
        a = best_of_ref(problem, Y[:cut], X, **p)
        two = best_of_ref(problem, Y[cut:], X, out=a, round0=cut, **p)
        for x, y in zip(one[:3], two[:3]):
            assert torch.equal(torch.nan_to_num(x.float(), nan=-7.0), torch.nan_to_num(y.float(), nan=-7.0))
        assert torch.equal(torch.isnan(one[0]), torch.isnan(two[0]))
        assert torch.equal(torch.cat([a[3], two[3]]), one[3]) or problem != "co"
    if problem == "co":
        assert one[2][::7].tolist() == [0] * len(one[2][::7])             # ties keep round 0
    else:
        assert int(one[2][9]) == -1 and bool(torch.isnan(one[1][9]))
    if problem == "msr":
        nan5 = torch.isnan(one[3][:, 5])
        assert bool(nan5.any()) and not bool(nan5[int(one[2][5])])       # some rounds of condition 5 are NaN, the winner is not


def test_abi_surface_carries_best_of():
    from diffsg_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "diffsg.h")).read()
    assert re.search(r"\bint dsg_best_of\s*\(int problem, const float\* Y, const float\* X, int n, long long B, int D", hdr)
    for name, val in (("MSR", 0), ("CO", 1), ("NU", 2)):
        assert re.search(rf"#define DSG_PROBLEM_{name} {val}\b", hdr)
    assert "dsg_best_of" in _lib._SIGS and len(_lib._SIGS["dsg_best_of"][1]) == 14
    assert hasattr(_lib.lib(), "dsg_best_of")
    from diffsg_amd import repeated
    assert repeated.PROBLEMS == {"msr": 0, "co": 1, "nu": 2}
    assert "| `dsg_best_of` |" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_best_of_has_no_cpu_path():
    import diffsg_amd
    from diffsg_amd.ddpm import DDPMCore
    assert diffsg_amd.best_of is diffsg_amd.repeated.best_of and hasattr(DDPMCore, "sample_best")
    with pytest.raises(RuntimeError, match="no CPU path"):
        diffsg_amd.best_of("msr", torch.zeros(2, 4, 3), torch.ones(4, 3), W=1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        diffsg_amd.best_of("co", torch.zeros(2, 4, 3), torch.ones(4, 9))
