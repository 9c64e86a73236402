"""The restatement of the library's random draws (tests/philox_ref.py) on the CPU: known answers of Philox4x32-10, the
edges of the uniform mapping, what the key and the counter keep of a 64-bit seed and index, the unit of the draw bound, and the
conditions that keep the bounds of tests/test_gpu_philox.py meaningful: eps is exactly 0 on every zeroed net, and every case's budget
is at most philox_cases.CAP.  No GPU, none of the library."""
import numpy as np
import pytest
import torch

import philox_cases as C
import philox_ref as P
from oracle import ddpm_oracle as O

# counter | key -> output, computed with the restatement; the first and the third are the Random123 known-answer vectors
KAT = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


def test_known_answer_vectors():
    for ctr, key, want in KAT:
        assert tuple(int(w) for w in P.philox4x32_10(*ctr, *key)) == want, [hex(v) for v in ctr]
    # vectorised: the three at once give the three
    cols = [np.array([k[0][i] for k in KAT], dtype=np.uint64) for i in range(4)] + [np.array([k[1][i] for k in KAT], dtype=np.uint64) for i in range(2)]
    got = np.stack(P.philox4x32_10(*cols), axis=1)
    assert got.tolist() == [list(k[2]) for k in KAT]
    # the draw contract's layout: counter (idx4 lo, idx4 hi, stream, 0x5eed), key (seed lo, seed hi)
    seed, stream, idx4 = 0x299f31d0a4093822, 0x13198a2e, 0x85a308d3243f6a88
    assert P.words(seed, stream, [idx4])[0].tolist() == [int(w) for w in P.philox4x32_10(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x5eed, 0xa4093822, 0x299f31d0)]


def test_edges_of_the_uniform_mapping():
    """Word 0xFFFFFFxx: (2^24 - 1) + 0.5 rounds to 2^24 in float32, u == 1.0, r == 0 and z == 0 (finite).  Word 0: u = 2^-25, the
    smallest, |z| <= sqrt(-2 ln 2^-25) = 5.887: the `< 7.0` of test_device_training_draws_have_the_reference_distributions holds for
    every word.  From 2^23 upwards the + 0.5 is lost (ties to even)."""
    top = P.uniform_of(np.array([0xFFFFFF00, 0xFFFFFFFF, 0xFFFFFE00], dtype=np.uint64))
    assert top.dtype == np.float32 and top[0] == 1.0 and top[1] == 1.0 and top[2] == np.float32(1.0 - 2.0 ** -23)
    low = P.uniform_of(np.array([0, 0xFF, 0x100], dtype=np.uint64))
    assert low[0] == np.float32(2.0 ** -25) and low[1] == low[0] and low[2] == np.float32(1.5 * 2.0 ** -24)
    mid = P.uniform_of(np.array([(1 << 31) | 0x100, ((1 << 23) - 1) << 8], dtype=np.uint64))
    assert mid[0] == np.float32((2 ** 23 + 2) * 2.0 ** -24)                 # 2^23 + 1 + 0.5 -> 2^23 + 2 (ties to even)
    assert mid[1] == np.float32((2 ** 23 - 0.5) * 2.0 ** -24)               # below 2^23 the half is kept
    zmax = float(np.sqrt(-2.0 * np.log(2.0 ** -25)))
    assert abs(zmax - 5.887) < 1e-3
    for f32 in (False, True):
        z = P.box_muller(np.array([[1.0, 0.3, 1.0, 1.0], [2.0 ** -25, 0.0, 2.0 ** -25, 0.25]], dtype=np.float32), f32)
        assert np.isfinite(z).all() and (z[0] == 0).all()
        assert abs(abs(z[1, 0]) - zmax) < 1e-5 and np.abs(z[1]).max() <= zmax + 1e-5 < 7.0


def test_the_high_halves_of_seed_and_index_are_live():
    idx = np.arange(8, dtype=np.uint64)
    for seed in (1 << 32, (1 << 32) + 1, 77 ^ C.FOLD, (1 << 62) - 1):
        assert not np.array_equal(P.words(seed, 3, idx), P.words(seed & 0xFFFFFFFF, 3, idx)), hex(seed)
    big = idx + np.uint64(1 << 32)
    assert not np.array_equal(P.words(5, 3, big), P.words(5, 3, idx))
    assert np.array_equal(P.words(5, 3, big), np.stack(P.philox4x32_10(idx, 1, 3, 0x5eed, 5, 0), axis=1))
    # streams: a step, the start state and the three kinds of a training call never share a counter
    seen = {tuple(P.words(5, s, [0])[0].tolist()) for s in (0, 1, 2, 4, 5, 6, P.Y_T_STREAM)}
    assert len(seen) == 7
    assert P.Y_T_STREAM == 0xFFFFFFFF and np.array_equal(P.words(5, 4 * (1 << 30) + 1, idx), P.words(5, 1, idx))     # the 32-bit wrap


def test_layout_of_the_draws():
    """Element 4 * idx4 + p, truncated; the noise layout of a sampling call; chunk-local indices; ts / mask by row."""
    z = P.normals(9, 2, 11)
    assert z.shape == (11,) and np.array_equal(z, P.normals(9, 2, 12)[:11]) and np.array_equal(z[8:], P.normals(9, 2, 3, idx4_base=2))
    y_T, nz = P.sample_draws(9, 5, 11)
    assert np.array_equal(y_T, P.normals(9, 0xFFFFFFFF, 11)) and nz.shape == (3, 11)
    assert all(np.array_equal(nz[r], P.normals(9, 4 - r, 11)) for r in range(3))                  # row r: step K-1-r = 4, 3, 2
    _, nz = P.sample_draws(9, 5, 11, noisy=[False, False, True, False, True])
    assert np.isnan(nz[1]).all() and np.array_equal(nz[0], P.normals(9, 4, 11)) and np.array_equal(nz[2], P.normals(9, 2, 11))
    yc, zc = P.sample_draws_chunked([4, 4, 6], 5, 150, 3, 64)
    assert yc.shape == (450,) and zc.shape == (3, 450)
    assert np.array_equal(yc[:192], yc[192:384]) and np.array_equal(yc[384:], P.normals(6, 0xFFFFFFFF, 66))
    assert not np.array_equal(yc[384:], yc[:66]) and np.array_equal(zc[1, 192:384], P.normals(4, 3, 192))
    ts, noise, mask = P.train_draws(123, 5, 1000, 0.9, 33, 3)
    assert ts.dtype == np.int32 and ts.shape == (33,) and noise.shape == (33, 3) and mask.dtype == np.float32
    assert np.array_equal(noise.reshape(-1), P.normals(123, 20, 99))
    w = P.words(123, 21, np.arange(9))[:, :].reshape(-1)[:33]
    u24 = (w >> np.uint64(8)).astype(np.int64)
    assert np.array_equal(P.train_draws(123, 5, 1 << 24, 0.9, 33, 3)[0], u24)                     # T = 2^24: ts is the 24-bit word itself
    assert np.all(np.abs(ts - u24 * 1000 / 2 ** 24) < 1.0) and ts.max() <= 999
    assert set(P.train_draws(1, 0, 7, 0.0, 70, 2)[2].tolist()) == {0.0} and set(P.train_draws(1, 0, 7, 1.0, 70, 2)[2].tolist()) == {1.0}
    assert set(P.train_draws(1, 0, 1, 0.5, 70, 2)[0].tolist()) == {0}
    # the clamp to T - 1 is a guard that the 24-bit grid never reaches: the largest word gives fl32((1 - 2^-24) * T) < T, because
    # T * 2^-24 lies between half an ulp and one ulp below T (at a power of two: exactly one ulp), so the product rounds to T - ulp
    for T in (1, 7, 20, 1000, 1023, 1 << 24, (1 << 24) - 1):
        assert int(np.float32(np.float32((2 ** 24 - 1) * 2.0 ** -24) * np.float32(T))) == T - 1, T


def test_float32_box_muller_against_float64_is_the_unit_of_the_draw_bound():
    """The largest deviation of the float32-evaluated Box-Muller from the float64 one on the same float32 uniforms (2^20 draws): about
    6e-7 absolute and 2.2e-7 relative to max(1, |z|).  The device may be philox_cases.FACTOR = 8 times that away from the restatement."""
    a, r = C.box_muller_unit()
    print(f"float32 Box-Muller vs float64 on the same uniforms: {a:.2e} absolute, {r:.2e} relative to max(1, |z|)")
    assert 5e-8 < r < 5e-7 and r <= a < 2e-6
    # and a float64 evaluation of u would be a different draw: up to 1.6e-5 away
    w = P.words(123, 0, np.arange(1 << 18))
    u64 = ((w >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    ang = 2.0 * np.pi * u64[:, 1::2]
    r64 = np.sqrt(-2.0 * np.log(u64[:, 0::2]))
    z64 = np.stack((r64[:, 0] * np.cos(ang[:, 0]), r64[:, 0] * np.sin(ang[:, 0]), r64[:, 1] * np.cos(ang[:, 1]), r64[:, 1] * np.sin(ang[:, 1])), axis=1)
    off = float(np.abs(z64.reshape(-1) - P.normals(123, 0, 1 << 20)).max())
    print(f"float64-evaluated uniforms move z by up to {off:.2e}")
    assert off > C.FACTOR * a                               # such a draw would miss the draw bound


@pytest.mark.parametrize("net", list(C.NETS))
def test_a_zeroed_last_linear_gives_eps_exactly_zero(net):
    name, T = C.NETS[net]
    plan, p = C.zero_net(net)
    base = C.G.net_params(name)[1]
    assert bool(base["final.weight"].any()) and set(k for k in p if not torch.equal(p[k], base[k])) <= {"final.weight", "final.bias"}
    B, D = 33, C.CONFIGS[name]["input_dim"]
    g = torch.Generator().manual_seed(T)
    y = 3.0 * torch.randn(B, D, generator=g)
    for mask in (0.0, 1.0):
        for i in (0, T - 1):
            t = torch.full((1, B), i, dtype=torch.int64) / T
            with torch.no_grad():
                eps = O.unet_forward(p, plan, y, t, C.cond_of(net, B), torch.full((B, 1), mask))
            assert eps.shape == (B, D) and bool((eps == 0).all())


@pytest.mark.parametrize("cid", list(C.CASE))
def test_budgets_of_the_sampling_cases(cid):
    ref = C.reference(cid)
    print(f"{cid}: budget {ref.budget:.2e} = {C.FACTOR:g} x (float32 oracle {ref.rel32:.2e} + response {ref.response:.2e}); "
          f"max|y_0| {float(ref.y64.abs().max()):.3g}")
    assert torch.isfinite(ref.y64).all() and ref.y64.dtype == torch.float64
    assert 0.0 < ref.budget <= C.CAP
    assert all(0.0 <= b <= C.CAP for _, _, b in ref.steps)
    case = C.CASE[cid]
    if case.kind != "chunks":
        assert len(ref.steps) == C.steps_of(case)


def test_the_cases_are_what_the_contract_lists():
    assert {(c.net, c.B) for c in C.PLAIN} == {(n, b) for n in ("tiny", "nu3", "msr80") for b in (1, 33, 70)} | {("tiny70", 70)}
    assert C.NETS["tiny70"][1] - 4 == 32 + 32 + 2
    assert any(s >= 1 << 32 for s in C.CHUNK_SEEDS) and len(set(C.CHUNK_SEEDS)) == 3 and 150 % 64 == 22
    lo, hi = (c.seed for c in C.HIGH)
    assert lo != hi and lo & 0xFFFFFFFF == hi & 0xFFFFFFFF
    assert C.FOLDED[0].seed ^ C.FOLDED[1].seed == C.FOLD and C.FOLDED[1].seed >> 32
    # ddim(eta = 0) and dpmpp_2m draw nothing but y_T; the two eta = 0 cases differ in the seed alone
    for cid in ("nu3-ddim0-a", "nu3-dpmpp"):
        assert np.isnan(C.draws(C.CASE[cid])[1]).all()
    a, b = C.reference("nu3-ddim0-a").y64, C.reference("nu3-ddim0-b").y64
    assert C.rel(a, b) > 0.1
    # the variants case: three tables, three renorm counts, one chunk without noise
    noisy = [bool(p.coef[:, 3].any()) for p in C.ref_plans(C.VARIANTS[0])]
    assert noisy == [True, False, True] and len({p.renorm_steps for p in C.ref_plans(C.VARIANTS[0])}) == 3
