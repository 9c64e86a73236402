"""Chunk variants on the device (DDPM.sample_chunked(variants=...), DDPM.sample_best(variants=...), dsg_set_chunk_variants;
DESIGN.md 15): every chunk of a variants call is the chunk's own sample() call bit for bit, the call agrees with the CPU reference
tests/variants_ref.py, and every refusal leaves the handle sampling as before.

Shapes (variants_ref.CASES / BIT_ONLY): `nu3` with the shipped checkpoint (D = 5; T = 20 plan-less, K = 10 plans) and `tiny` (T = 8, K = 4);
chunk_rows = 32 with B = 150 (five chunks, the last 22 rows; the scalar path of the update) and B = 160 (the quad path), chunk_rows = 64
with B = 192 (two row tiles per chunk).  Bound of the comparison with the reference, per chunk: `rel <= TOL + 3 x budget`, TOL = 1e-5 as in
tests/test_gpu_steps.py, `budget` the reference's own float32-against-float64 error of that chunk (tests/test_variants_cpu.py caps it).
All tests need an MI355X: run with `-m gpu`."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import steps_ref as R
import variants_ref as VR
from oracle import ddpm_oracle as O
from weights import CONFIGS

pytestmark = pytest.mark.gpu

TOL = 1e-5
MODES = ("split_f16", "f32")


def make_ddpm(net, policy="default"):
    """The net under its problem's DDPM class (NU for nu3: decoder and objective of sample_best), on the device."""
    from diffsg_amd import UNet1D
    from diffsg_amd import classifier_free_MSR as MSR, classifier_free_NU as NU
    T, _ = R.NETS[net]
    cfg = CONFIGS[net]
    _, p = VR.net_params(net)
    m = UNet1D(**cfg, is_attn=(False,) * len(cfg["dims"]))
    m.load_state_dict(p, strict=True)
    D, dev, alphas = cfg["input_dim"], torch.device("cuda"), 1.0 - O.cosine_betas(T)
    if net == "nu3":
        d = NU.DDPM(T, m.to("cuda"), D - 2, 18.0, alphas, dev, (1, D), {"width": 400, "height": 400})
    else:
        d = MSR.DDPM(T, m.to("cuda"), D, 20.0, alphas, dev, (1, D), None)
    d = d.to("cuda")
    if policy == "large":
        d.model.set_launch_policy(0, 0)
    return d


def device_variants(d, case):
    """[(omega, plan)] of a case through the package's own constructors; the chunks that share a table share its `coef` tensor."""
    from diffsg_amd import steps
    _, K = R.NETS[case.net]
    base = {}

    def plan_of(v):
        if v.table == "identity":
            return steps.with_renorm(d, v.renorm)
        if v.table not in base:
            kind, eta = R.SAMPLERS[v.table]
            base[v.table] = steps.strided(d, K) if kind == "strided" else steps.ddim(d, K, eta)
        return steps.with_renorm(base[v.table], v.renorm)
    return [(v.omega, plan_of(v)) for v in case.variants]


def case_inputs(case):
    K = VR.steps_of(case)
    cond, y_T, z = VR.inputs(case.net, case.B)
    return cond.cuda(), y_T.cuda(), z[:K - 2].contiguous().cuda()


def own_calls(d, case, variants, cond, seeds, y_T=None, z=None, **kw):
    """The chunks' own sample() calls; also how many of them left the fp16 range of the split path and repeated themselves in float32."""
    out, repeats = [], 0
    for c, sl in enumerate(VR.chunk_slices(case.B, case.chunk_rows)):
        om, plan = variants[c]
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out.append(d.sample(cond[sl], om, seed=seeds[c], plan=plan, y_T=None if y_T is None else y_T[sl],
                                noise=None if z is None else z[:, sl].contiguous(), **kw))
        repeats += sum("fp16 range" in str(x.message) for x in w)
    return torch.cat(out), repeats


def chunked(d, case, variants, cond, seeds, **kw):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = d.sample_chunked(cond, 123.0, case.chunk_rows, seeds=seeds, variants=variants, **kw)     # `omega` is not read
    return got, sum("fp16 range" in str(x.message) for x in w)


SEEDS = [11, 2 ** 40 + 5, 77, 2 ** 63 + 9, 5]


# 1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["default", "large"])
@pytest.mark.parametrize("name", [c.name for c in VR.CASES + VR.BIT_ONLY])
def test_chunks_are_their_own_calls_bit_for_bit(name, policy):
    """Graph and eager, both launch policies, both precision modes, injected noise and the device's Philox draws.  A call that leaves the
    fp16 range of the split path repeats itself WHOLE on the exact-float32 kernels (DDPM.sample_chunked), a chunk's own call only
    itself: where that happens the split-mode call is compared with the chunks' float32 calls, as documented there."""
    case = VR.CASE[name]
    d = make_ddpm(case.net, policy)
    variants = device_variants(d, case)
    cond, y_T, z = case_inputs(case)
    seeds = SEEDS[:len(variants)]
    refs, last = {}, None
    for mode in reversed(MODES):                                    # float32 first: the fall-back of a saturated split-mode call
        d.model.set_precision(mode)
        for inject in (True, False):
            io = dict(y_T=y_T, z=z) if inject else {}
            ref, rep = own_calls(d, case, variants, cond, seeds, **io)
            refs[(mode, inject)] = ref
            assert torch.isfinite(ref).all()
            for graph in (True, False):
                got, rep_c = chunked(d, case, variants, cond, seeds, use_graph=graph, **({"y_T": y_T, "noise": z} if inject else {}))
                assert (rep_c > 0) == (rep > 0), (mode, inject, graph, rep, rep_c)
                want = refs[("f32", inject)] if rep_c else ref
                assert torch.equal(got, want), (name, policy, mode, inject, graph, rep)
                last = got
    assert d.model.precision == "split_f16"
    # and the call is not one setting for every chunk: chunk 0's setting everywhere gives other rows from chunk 1 on
    plain = d.sample_chunked(cond, variants[0][0], case.chunk_rows, seeds=seeds, plan=variants[0][1])
    assert not torch.equal(plain[case.chunk_rows:], last[case.chunk_rows:])


# 2 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,B,chunk", [("nu3", 150, 32), ("tiny", 160, 32)])
def test_equal_variants_are_the_plain_chunked_call(net, B, chunk):
    from diffsg_amd import steps
    _, K = R.NETS[net]
    d = make_ddpm(net)
    cond = VR.inputs(net, B)[0].cuda()
    nch = -(-B // chunk)
    seeds = SEEDS[:nch]
    for plan in (None, steps.ddim(d, K, 0.5), steps.with_renorm(steps.strided(d, K), 1)):
        for graph in (True, False):
            a = d.sample_chunked(cond, 2.0, chunk, seeds=seeds, plan=plan, use_graph=graph)
            b = d.sample_chunked(cond, -7.0, chunk, seeds=seeds, variants=[(2.0, plan)] * nch, use_graph=graph)
            assert torch.isfinite(a).all() and torch.equal(a, b), (plan is None, graph)


# 3 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in VR.CASES])
def test_against_the_reference(name):
    case = VR.CASE[name]
    d = make_ddpm(case.net)
    variants = device_variants(d, case)
    cond, y_T, z = case_inputs(case)
    y32, y64 = VR.reference(name)
    for mode in MODES:
        d.model.set_precision(mode)
        got = d.sample_chunked(cond, 0.0, case.chunk_rows, variants=variants, y_T=y_T, noise=z).cpu()
        worst = []
        for c, sl in enumerate(VR.chunk_slices(case.B, case.chunk_rows)):
            e, budget = R.rel(got[sl], y32[sl]), R.rel(y32[sl], y64[sl])
            print(f"{name} {mode} chunk {c} {case.variants[c]}: rel err vs reference {e:.2e} (reference float32 vs float64: {budget:.2e})")
            worst.append((e, budget))
        for c, (e, budget) in enumerate(worst):
            assert np.isfinite(e) and e <= TOL + 3.0 * budget, (name, mode, c, e, budget)
    d.model.set_precision("split_f16")


# 4 ------------------------------------------------------------------------------------------------
def test_plain_then_variants_then_plain_on_one_model():
    """The two forms of the step keep their own graphs and their own settings: a variants call between two plain ones changes neither
    the plain chunked call nor sample(), with and without a plan, and the variants call itself repeats bit for bit."""
    from diffsg_amd import steps
    case = VR.CASE["nu3-K10-b160-w500"]
    d = make_ddpm(case.net)
    variants = device_variants(d, case)
    cond, y_T, z = case_inputs(case)
    seeds = SEEDS[:len(variants)]
    plan = steps.strided(d, 10)

    def plains():
        return (d.sample_chunked(cond, 2.0, case.chunk_rows, seeds=seeds), d.sample(cond, 2.0, seed=3),
                d.sample_chunked(cond, 2.0, case.chunk_rows, seeds=seeds, plan=plan), d.sample(cond[:64], -1.0, seed=4, plan=plan))
    first = plains()
    assert getattr(d.model._native, "chunk_variants", None) is None
    v1 = d.sample_chunked(cond, 0.0, case.chunk_rows, seeds=seeds, variants=variants)
    assert d.model._native.chunk_variants is not None
    v2 = d.sample_chunked(cond, 0.0, case.chunk_rows, seeds=seeds, variants=variants)
    third = plains()
    assert d.model._native.chunk_variants is None
    v3 = d.sample_chunked(cond, 0.0, case.chunk_rows, seeds=seeds, variants=variants)
    # another set of the same chunk count: contents only
    v4 = d.sample_chunked(cond, 0.0, case.chunk_rows, seeds=seeds, variants=variants[::-1])
    v5 = d.sample_chunked(cond, 0.0, case.chunk_rows, seeds=seeds, variants=variants)
    for a, b in zip(first, third):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    assert torch.equal(v1, v2) and torch.equal(v1, v3) and torch.equal(v1, v5) and not torch.equal(v1, v4)
    assert not torch.equal(v1, first[2])


# 5, 6 ---------------------------------------------------------------------------------------------
class CAbi:
    """dsg_sample / dsg_sample_chunked on one tiny model with injected start state and noise; `out` is pre-filled so that a refused
    call can be seen to have enqueued nothing."""
    FILL = 123.0

    def __init__(self, B=96):
        from diffsg_amd import _lib
        self.lib, self.L = _lib, _lib.lib()
        self.d = make_ddpm("tiny")
        self.T = R.NETS["tiny"][0]
        cond, y_T, z = VR.inputs("tiny", 160)
        self.B = B
        self.cond, self.y_T, self.z = cond[:B].contiguous().cuda(), y_T[:B].contiguous().cuda(), z[:, :B].contiguous().cuda()
        self.coef = self.d._coef_table().contiguous()
        self.d.sample(self.cond, 1.0, seed=1)              # binds the weights
        self.hd = self.d.model.native_handle()
        self.out = torch.empty(B, 3, device="cuda")

    def err(self):
        return self.L.dsg_last_error().decode()

    def sample(self, omega, coef=None, T=None):
        self.out.fill_(self.FILL)
        torch.cuda.synchronize()
        p = self.lib.ptr
        rc = self.L.dsg_sample(self.hd, p(self.cond), p(self.y_T), p(self.z), 0, float(omega), p(self.coef if coef is None else coef),
                               self.T if T is None else T, p(self.out), self.B, 0, self.lib.stream_ptr())
        torch.cuda.synchronize()
        return rc, self.out.clone()

    def chunked(self, omega, chunk_rows, coef=None, flags=0):
        self.out.fill_(self.FILL)
        torch.cuda.synchronize()
        p = self.lib.ptr
        nch = -(-self.B // chunk_rows)
        sd = (ctypes.c_ulonglong * nch)(*range(1, nch + 1))
        rc = self.L.dsg_sample_chunked(self.hd, p(self.cond), p(self.y_T), p(self.z), sd, chunk_rows, float(omega),
                                       p(self.coef if coef is None else coef), self.T, p(self.out), self.B, flags, self.lib.stream_ptr())
        torch.cuda.synchronize()
        return rc, self.out.clone()

    def set(self, omega, renorm=None, table=None, chunks=None, tables=1):
        n = len(omega) if chunks is None else chunks
        om = (ctypes.c_float * max(len(omega), 1))(*omega)
        rn = None if renorm is None else (ctypes.c_int * len(renorm))(*renorm)
        tb = None if table is None else (ctypes.c_int * len(table))(*table)
        return self.L.dsg_set_chunk_variants(self.hd, om, rn, tb, n, tables)

    def unset(self):
        return self.L.dsg_set_chunk_variants(self.hd, None, None, None, 0, 1)

    def untouched(self, out):
        return bool((out == self.FILL).all())


def test_set_and_unset_at_the_c_abi():
    a = CAbi()
    T, B = a.T, a.B
    rc, plain2 = a.sample(2.0)
    assert rc == 0, a.err()
    rc, plain5 = a.sample(-5.0)
    assert rc == 0 and not torch.equal(plain2, plain5)
    # one chunk (chunk_rows >= B): legal, takes the variant kernels, reads omega from the setting; NULL renorm = the call's default count
    # (min(T, 4)), NULL table = table 0
    assert a.set([2.0]) == 0, a.err()
    for flags in (0, 1):
        rc, got = a.chunked(-5.0, 96, flags=flags)
        assert rc == 0, a.err()
        assert torch.equal(got, plain2), flags
    rc, got = a.chunked(-5.0, 128)
    assert rc == 0 and torch.equal(got, plain2)
    # the same count spelled out, then another count: 0 renorm steps is another result, and the step grid's count is its own call's
    assert a.set([2.0], renorm=[4]) == 0
    assert torch.equal(a.chunked(0.0, 96)[1], plain2)
    assert a.set([2.0], renorm=[0]) == 0
    rc, r0 = a.chunked(0.0, 96)
    assert rc == 0 and torch.isfinite(r0).all() and not torch.equal(r0, plain2)
    t = (ctypes.c_float * T)(*[i / T for i in range(T)])
    assert a.L.dsg_set_chunk_variants(a.hd, None, None, None, 0, 1) == 0
    assert a.L.dsg_set_step_grid(a.hd, t, T, 0) == 0
    rc, r0_own = a.sample(2.0)
    assert rc == 0 and torch.equal(r0_own, r0)
    assert a.L.dsg_set_step_grid(a.hd, None, 0, -1) == 0
    # two tables stacked: table 1 is read at rows T .. 2T-1
    other = a.coef.clone()
    other[:, 0] *= 0.5
    stacked = torch.stack((a.coef, other)).contiguous()
    assert a.set([2.0, 2.0, -5.0], renorm=[4, 4, 4], table=[1, 0, 0], tables=2) == 0, a.err()
    rc, got = a.chunked(0.0, 32, coef=stacked)
    assert rc == 0, a.err()
    # chunk statistics are per chunk, so compare with the chunk's own 32-row calls
    b = CAbi(B=32)
    for c, (om, cf) in enumerate(((2.0, other), (2.0, None), (-5.0, None))):
        b.cond, b.y_T, b.z = a.cond[32 * c:32 * c + 32].contiguous(), a.y_T[32 * c:32 * c + 32].contiguous(), a.z[:, 32 * c:32 * c + 32].contiguous()
        rc, own = b.sample(om, coef=cf)
        assert rc == 0 and torch.equal(got[32 * c:32 * c + 32], own), c
    # removed: the plain calls are back, and dsg_sample_chunked reads its omega argument again
    assert a.unset() == 0
    assert torch.equal(a.sample(2.0)[1], plain2) and torch.equal(a.sample(-5.0)[1], plain5)
    assert torch.equal(a.chunked(-5.0, 96)[1], plain5)
    # chunks == 0 with arrays given removes as well
    assert a.set([2.0]) == 0 and a.set([2.0], chunks=0) == 0
    assert torch.equal(a.sample(-5.0)[1], plain5)


def test_refusals_leave_the_handle_sampling_as_before():
    a = CAbi()
    T = a.T
    rc, plain = a.sample(2.0)
    assert rc == 0
    assert a.set([2.0, -1.0, 500.0], renorm=[4, 0, 1]) == 0, a.err()
    rc, held = a.chunked(0.0, 32)
    assert rc == 0 and torch.isfinite(held).all()

    def still_held():
        rc, again = a.chunked(0.0, 32)
        assert rc == 0 and torch.equal(again, held)

    # the setter's own refusals, under its name; the held setting stays
    for bad in (lambda: a.set([1.0, 1.0, 1.0], chunks=-1), lambda: a.set([1.0, 1.0, 1.0], tables=0),
                lambda: a.set([1.0, 1.0, 1.0], table=[0, 1, 0], tables=1), lambda: a.set([1.0, 1.0, 1.0], table=[0, -1, 0], tables=2),
                lambda: a.set([1.0, 1.0, 1.0], renorm=[0, -1, 0])):
        assert bad() != 0
        assert "dsg_set_chunk_variants" in a.err(), a.err()
        still_held()
    # a chunk-count mismatch: nothing is enqueued
    for rows in (64, 96):
        rc, out = a.chunked(0.0, rows)
        assert rc != 0 and a.untouched(out)
        msg = a.err()
        assert "3" in msg and str(-(-a.B // rows)) in msg and "dsg_set_chunk_variants" in msg, msg
    still_held()
    # dsg_sample while variants are held
    rc, out = a.sample(2.0)
    assert rc != 0 and a.untouched(out) and "dsg_set_chunk_variants" in a.err(), a.err()
    still_held()
    # a renorm count above T is refused by the call, naming both numbers
    assert a.set([2.0, -1.0, 500.0], renorm=[4, T + 3, 1]) == 0
    rc, out = a.chunked(0.0, 32)
    msg = a.err()
    assert rc != 0 and a.untouched(out) and str(T + 3) in msg and str(T) in msg.replace(str(T + 3), ""), msg
    assert a.set([2.0, -1.0, 500.0], renorm=[4, 0, 1]) == 0
    still_held()
    # a renorm hook together with variants
    stats = torch.zeros(3, device="cuda", dtype=torch.float64)
    cb = ctypes.CFUNCTYPE(None, ctypes.c_void_p)(lambda user: None)
    assert a.L.dsg_set_renorm_hook(a.hd, a.lib.ptr(stats), ctypes.cast(cb, ctypes.c_void_p), None) == 0
    rc, out = a.chunked(0.0, 32)
    assert rc != 0 and a.untouched(out) and "hook" in a.err(), a.err()
    assert a.L.dsg_set_renorm_hook(a.hd, None, None, None) == 0
    still_held()
    # and without the setting the handle samples what it sampled before
    assert a.unset() == 0
    rc, out = a.sample(2.0)
    assert rc == 0 and torch.equal(out, plain)


# 7 ------------------------------------------------------------------------------------------------
def test_variants_on_a_non_default_stream():
    case = VR.CASE["nu3-K10-b160-w500"]
    d = make_ddpm(case.net)
    variants = device_variants(d, case)
    cond, y_T, z = case_inputs(case)
    seeds = SEEDS[:len(variants)]
    ref = d.sample_chunked(cond, 0.0, case.chunk_rows, seeds=seeds, variants=variants)
    ref_inj = d.sample_chunked(cond, 0.0, case.chunk_rows, variants=variants, y_T=y_T, noise=z)
    d.sample(cond, 2.0, seed=1)                  # drop the setting: the next call sets it again, from inside the stream context
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = d.sample_chunked(cond, 0.0, case.chunk_rows, seeds=seeds, variants=variants)
        again = d.sample_chunked(cond, 0.0, case.chunk_rows, seeds=seeds, variants=variants)
        inj = d.sample_chunked(cond, 0.0, case.chunk_rows, variants=variants, y_T=y_T, noise=z)
    side.synchronize()
    assert torch.equal(got, ref) and torch.equal(again, ref) and torch.equal(inj, ref_inj)


# 8 ------------------------------------------------------------------------------------------------
def test_sample_best_with_variants():
    """Bit-identical across groupings and to repeated.best_of over the rounds' own calls; `round % len(variants)` names the winner's
    variant."""
    from diffsg_amd import best_of, steps
    d = make_ddpm("nu3")
    B, n = 64, 7
    cond = VR.inputs("nu3", B)[0].cuda()
    X = cond.clone() * 400.0
    problem, p = d._best_of_problem()
    ddim = steps.ddim(d, 10, 0.5)
    for variants in ([(500.0, None), (200.0, steps.with_renorm(d, 0)), (500.0, steps.with_renorm(d, 2))],
                     [(500.0, steps.strided(d, 10)), (50.0, steps.with_renorm(ddim, 0)), (500.0, steps.with_renorm(ddim, 10)), (2.0, steps.ddim(d, 10, 0.0))]):
        L = len(variants)
        # a round is one call
        seeds = list(range(40, 40 + n))
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            rounds = [d.sample(cond, variants[r % L][0], seed=seeds[r], plan=variants[r % L][1]) for r in range(n)]
        sat = [str(x.message) for x in w if "fp16 range" in str(x.message)]
        assert not sat, sat                                # (a saturated round would repeat alone, a saturated group whole)
        ref = best_of(problem, torch.stack(rounds), X, return_objectives=True, **p)
        for max_rows in (65536, B, 3 * B):
            got = d.sample_best(cond, X, n, seeds=seeds, max_rows=max_rows, return_objectives=True, variants=variants)
            for fname, x, y in zip(("solution", "objective", "round", "objectives"), got, ref):
                assert torch.equal(x, y), (fname, max_rows)
        # the winner's variant: its own call reproduces the kept solution's objective row by row
        win = (got.round % L).tolist()
        assert len(set(win)) > 1
        for v in sorted(set(win)):
            rows = torch.tensor([i for i, k in enumerate(win) if k == v], device="cuda")
            rs = sorted({int(r) for r in got.round[rows].tolist()})
            assert all(r % L == v for r in rs)
            for r in rs:
                sel = rows[(got.round[rows] == r)]
                assert torch.equal(got.objective[sel], ref.objectives[r][sel])
        # a round is two 32-row chunks; and chunks off the 32-row tile: the serial calls
        for chunk_rows in (32, 16):
            per = B // chunk_rows
            seeds = list(range(400, 400 + n * per))
            rounds = [torch.cat([d.sample(cond[c * chunk_rows:(c + 1) * chunk_rows], variants[r % L][0], seed=seeds[r * per + c],
                                          plan=variants[r % L][1]) for c in range(per)]) for r in range(n)]
            ref = best_of(problem, torch.stack(rounds), X, return_objectives=True, **p)
            for max_rows in (65536, B, 2 * B):
                got = d.sample_best(cond, X, n, seeds=seeds, chunk_rows=chunk_rows, max_rows=max_rows, return_objectives=True, variants=variants)
                for fname, x, y in zip(("solution", "objective", "round", "objectives"), got, ref):
                    assert torch.equal(x, y), (fname, chunk_rows, max_rows)
