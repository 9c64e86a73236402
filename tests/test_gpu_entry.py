"""`load_test_msr` / `load_test_co` / `load_test_nu` against the same evaluation composed by hand from the public calls
(`DDPM.sample_chunked`, `DDPM.sample`, `DDPM.sample_best`, then the module's decoder and objective), under the same seed of torch's
generator: the metrics are the same Python floats.  That pins what the three entry points share (diffsg_amd/entry.py): the order in which
the Philox seeds are drawn -- after the model is built, one per call or per chunk, round-major -- the batching rule and the unscaling.

The committed 200-row CSV slices (60 test rows), T = 20, a seeded `build_model(...).apply(init_weights)` checkpoint: batch 32 (two chunks,
the second of 28 rows), batch 48 (off the tile: serial calls), three rounds at batch 32 (60 rows do not tile into 32-row chunks, so every
round is its own chunked call) and four rounds over two variants.  Needs an MI355X: run with `-m gpu`."""
import os

import pytest
import torch

from _util import GOLD

pytestmark = pytest.mark.gpu

T, SEED = 20, 11
DATA = os.path.join(GOLD, "data")


def _msr():
    from diffsg_amd import classifier_free_MSR as M
    from diffsg_amd.decode import msr_rate
    csv = os.path.join(DATA, "3c_10w_200samples.csv")
    _, _, X_test, Y_test, cc = M.msr_data_load(csv)
    build = lambda: M.build_model(cc['M'], cc['sfn'] * cc['M'], torch.device("cuda:0"), T, cc, cc['W'])

    def metrics(X, Yt, sampled, best):
        Xt = X * (cc['scaler_max'] - cc['scaler_min']) + cc['scaler_min']
        pred = best(Xt).objective if best else msr_rate(cc['W'] * M.custom_decoder(sampled), Xt)
        true = msr_rate(Yt, Xt)
        return {"less_ratio": float(torch.sum(pred) / torch.sum(true)), "avg_rate_diff": float(torch.mean(pred - true))}
    return M.load_test_msr, csv, {}, build, X_test, Y_test, metrics


def _co():
    from diffsg_amd import classifier_free_CO as C
    csv = os.path.join(DATA, "3nodes_200samples_ood.csv")
    _, Y_train, X_test, Y_test, cc = C.co_data_load(csv)
    n = Y_train.shape[1]
    build = lambda: C.build_model(n, cc['sfn'] * n, torch.device("cuda:0"), T, cc)

    def metrics(X, Yt, sampled, best):
        Xt = X * (cc['scaler_max'] - cc['scaler_min']) + cc['scaler_min']
        if best:
            b = best(Xt)
            Yd, pred = b.solution, b.objective
        else:
            Yd = C.customized_real_decoder(sampled)
            pred = C.cost_calc(Xt, Yd)
        true = C.cost_calc(Xt, Yt)
        w = 2 ** torch.arange(n - 1, -1, -1, device=X.device)
        hits = (((Yd > 0.1).long() * w).sum(dim=1) == ((Yt > 0.1).long() * w).sum(dim=1)).sum()
        return {"exceeded_ratio": float(torch.sum(pred) / torch.sum(true)), "avg_cost_diff": float(torch.mean(pred - true)),
                "terrible": int(((pred / true > 1.2) & (pred > 10.0)).sum()), "accuracy": int(hits), "n": int(X.shape[0])}
    return C.load_test_co, csv, {}, build, X_test, Y_test, metrics


def _nu():
    from diffsg_amd import classifier_free_NU as N
    csv = os.path.join(DATA, "3u_18mW_200samples.csv")
    W, H = 400, 300                                  # not the defaults, and not each other
    _, _, X_test, Y_test, _, cc = N.nu_data_load(csv, W, H)
    build = lambda: N.build_model(cc['K'], cc['P_sum'], torch.device("cuda:0"), T, cc)

    def metrics(X, Yt, sampled, best):
        Xt, Yt = X.clone(), Yt.clone()
        Xt[:, 0::2] *= W
        Xt[:, 1::2] *= H
        Yt[:, 0] *= W
        Yt[:, 1] *= H
        Yt[:, 2:] *= cc['P_sum']
        pred = best(Xt).objective if best else N.rate_calc(N.custom_decoder(sampled, W, H, cc['P_sum']), Xt)
        true = N.rate_calc(Yt, Xt)
        return {"less_ratio": float(torch.sum(pred) / torch.sum(true)), "avg_rate_diff": float(torch.mean(pred - true))}
    return N.load_test_nu, csv, {"width": W, "height": H}, build, X_test, Y_test, metrics


def _pin(out):
    return {k: v.hex() if isinstance(v, float) else v for k, v in out.items()}


@pytest.mark.parametrize("problem", [_msr, _co, _nu])
def test_load_test_is_the_hand_composition_of_the_public_calls(problem, tmp_path):
    from diffsg_amd import steps
    from diffsg_amd.diffusion import init_weights
    load_test, csv, extra, build, X_test, Y_test, metrics = problem()
    torch.manual_seed(3)
    first = build().apply(init_weights)
    ck = str(tmp_path / "ddpm.pt")
    torch.save(first.state_dict(), ck)
    first.to("cuda:0")
    variants = [(500, None), (500, steps.with_renorm(first, 2))]      # a plan holds tables, no model: any model of this schedule makes it
    assert len(X_test) == 60

    def by_hand(run, best=None):
        torch.manual_seed(SEED)
        m = build()                                  # consumes torch's generator, as the model load_test builds does
        m.load_state_dict(torch.load(ck, map_location="cpu"))
        m.to("cuda:0")
        X = torch.tensor(X_test, dtype=torch.float32).cuda()
        Yt = torch.tensor(Y_test, dtype=torch.float32).cuda()
        return metrics(X, Yt, run(m, X) if run else None, (lambda Xt: best(m, X, Xt)) if best else None)

    def entry(**kw):
        logs = []
        torch.manual_seed(SEED)
        out = load_test(ck, csv, T=T, omega=500, log=logs.append, **extra, **kw)
        assert len(logs) == (4 if "accuracy" in out else 2)
        return out

    cases = [
        ("batch 32", dict(batch_size=32), dict(run=lambda m, X: m.sample_chunked(X, 500, 32)), {}),
        ("batch 48", dict(batch_size=48), dict(run=lambda m, X: torch.cat([m.sample(X[:48], 500), m.sample(X[48:], 500)])), {}),
        ("3 rounds", dict(batch_size=32, repeats=3), dict(run=None, best=lambda m, X, Xt: m.sample_best(X, Xt, 3, 500, chunk_rows=32)),
         {"repeats": 3}),
        ("variants", dict(batch_size=32, repeats=4, variants=variants),
         dict(run=None, best=lambda m, X, Xt: m.sample_best(X, Xt, 4, 0.0, chunk_rows=32, variants=variants)), {"repeats": 4}),
    ]
    seen = []
    for name, kw, hand, more in cases:
        got, want = entry(**kw), {**by_hand(**hand), **more}
        print(problem.__name__, name, got)
        assert list(got) == list(want) and _pin(got) == _pin(want), (name, got, want)
        seen.append(_pin(got))
    assert seen[0] != seen[1] and seen[2] != seen[3]          # the cases do not collapse into one evaluation
