"""Pins tests/split_ref.py, the CPU restatement of the split-f16 operand split: known-answer vectors worked out by hand at the binade edges,
the 22-bit claim and where it ends, and the error-versus-amplitude table of a raw Linear that the low side of the envelope
is derived from.  Everything the low-side tests expect comes from that module and the float64 oracle, so it is checked here against
arithmetic done on paper, not against the kernels."""
import numpy as np
import pytest

import split_ref as S

U = 2.0 ** -24            # fp16's subnormal spacing

# (v, hi, lo), all exact in float32.  hi rounds TOWARD ZERO, lo to NEAREST EVEN with subnormals kept.
VECTORS = [
    (2.0 ** -4, 2.0 ** -4, 0.0),
    # nearest-even would round hi up to 2^-4 (1 + 2^-10); toward zero keeps 2^-4.  The remainder 2^-15 + 2^-25 lies half way between the
    # subnormals 512 U and 513 U: the tie goes to the even one
    (2.0 ** -4 * (1 + 2.0 ** -11 + 2.0 ** -21), 2.0 ** -4, 512 * U),
    # just under 2^-4: hi = 2^-5 (2 - 2^-10), remainder 2^-16 + 2^-17 = 384 U, a subnormal, exact
    (2.0 ** -5 * (2 - 2.0 ** -10 + 2.0 ** -11 + 2.0 ** -12), 2.0 ** -5 * (2 - 2.0 ** -10), 384 * U),
    (2.0 ** -14, 2.0 ** -14, 0.0),                       # the smallest normal
    (1023 * U, 1023 * U, 0.0),                           # the largest subnormal
    (1023.5 * U, 1023 * U, 0.0),                         # nearest-even would give 2^-14; the remainder U / 2 ties to 0
    (1023.75 * U, 1023 * U, U),                          # remainder 0.75 U rounds UP: a truncating lo gives 0
    (U, U, 0.0),                                         # 2^-24
    (1.75 * U, U, U),                                    # rounds up; truncation gives 0
    (2.5 * U, 2 * U, 0.0),                               # tie to even (0)
    (0.5 * U, 0.0, 0.0),                                 # 2^-25: hi = 0 toward zero, the remainder ties to 0 -- the operand is lost whole
    (0.75 * U, 0.0, U),                                  # hi = 0, the remainder rounds up
    (2.0 ** -30, 0.0, 0.0),
    # normal range: hi = 1, remainder 2^-11 + 0.75 * 2^-21 rounds up to 2^-11 + 2^-21 (a truncating lo: 2^-11)
    (1 + 2.0 ** -11 + 2.0 ** -22 + 2.0 ** -23, 1.0, 2.0 ** -11 + 2.0 ** -21),
    (1 + 2.0 ** -11 + 2.0 ** -22, 1.0, 2.0 ** -11),      # tie: 2^-11 (even)
    (65504.0, 65504.0, 0.0),
    (65519.0, 65504.0, 15.0),                            # nearest-even would still give 65504 ...
    (65520.0, 65504.0, 16.0),                            # ... and inf from here on: toward zero saturates
    (70000.0, 65504.0, 4496.0),
    (0.0, 0.0, 0.0),
]


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_known_answer_vectors(sign):
    v = np.array([sign * t[0] for t in VECTORS], dtype=np.float32)
    assert np.array_equal(v.astype(np.float64), [sign * t[0] for t in VECTORS]), "a vector is not a float32 number"
    hi, lo = S.split(v)
    assert hi.dtype == np.float16 and lo.dtype == np.float16
    for (x, h, l), gh, gl in zip(VECTORS, hi.astype(np.float64), lo.astype(np.float64)):
        assert gh == sign * h and gl == sign * l, (sign * x, gh, gl, "expected", sign * h, sign * l)
    assert not np.signbit(S.split(np.zeros(3, np.float32))[0]).any()


def _sweep(lo, hi, n=200000, seed=1):
    rng = np.random.default_rng(seed)
    v = np.exp(rng.uniform(np.log(lo), np.log(hi), n)) * rng.choice([-1.0, 1.0], n)
    edges = 2.0 ** np.arange(np.ceil(np.log2(lo)), np.floor(np.log2(hi)) + 1)
    edges = edges[(edges >= lo) & (edges <= hi)]
    near = np.concatenate([edges, np.nextafter(edges.astype(np.float32), np.float32(0)), edges * (1 + 2.0 ** -11), edges * (1 + 2.0 ** -11 + 2.0 ** -22)])
    return np.concatenate([v, near, -near]).astype(np.float32)


def test_22_bits_from_one_eighth_up_to_the_raw_limit():
    """|hi + lo - v| <= 2^-22 |v| for |v| in [2^-3, 6e4]: 11 bits of hi, 11 of lo, lo's sign for free."""
    v = _sweep(S.FULL_BITS_FROM, 6.0e4)
    v = v[(np.abs(v) >= S.FULL_BITS_FROM) & (np.abs(v) <= 6.0e4)]
    err = S.operand_error(v)
    assert (err <= 2.0 ** -22 * np.abs(v.astype(np.float64))).all(), float((err / np.abs(v)).max())
    # and the bound is met somewhere: the reference is not accidentally better than the format
    assert float((err / np.abs(v)).max()) > 2.0 ** -23.1


def test_absolute_error_below_one_eighth():
    """Below 2^-3 the error is absolute, at most 2^-25: 21 bits in [2^-4, 2^-3), a bit less per binade below; reached below 2^-4."""
    v = _sweep(2.0 ** -40, S.FULL_BITS_FROM)
    v = v[np.abs(v) < S.FULL_BITS_FROM]
    err = S.operand_error(v)
    assert (err <= S.SUBNORMAL_ABS_ERR).all(), float(err.max())
    small = np.abs(v) < S.LO_SUBNORMAL_BELOW
    assert float(err[small].max()) == S.SUBNORMAL_ABS_ERR
    # in [2^-4, 2^-3): never worse than 2^-21 relative
    mid = ~small
    assert (err[mid] <= 2.0 ** -21 * np.abs(v[mid].astype(np.float64))).all()


def test_zero_is_exact_and_products_of_zero_rows_are_zero():
    z = np.zeros((3, 16), np.float32)
    assert not S.operand_error(z).any()
    _, W = S.table_case(0, n_in=16, n_out=8)
    assert not S.linear(z, W).any()


def test_weight_scale_rule_and_clamp():
    assert S.scale_exp(1.0) == 13 and S.scale_exp(0.99) == 13 and S.scale_exp(0.5) == 14 and S.scale_exp(0.49) == 14
    assert S.scale_exp(8192.0) == 0 and S.scale_exp(8193.0) == -1
    assert S.scale_exp(2.0 ** 21) == -8 and S.scale_exp(2.0 ** 30) == -8           # clamp below
    assert S.scale_exp(2.0 ** -11) == 24 and S.scale_exp(2.0 ** -20) == 24 and S.scale_exp(0.0) == 24      # clamp above
    assert S.scale_exp_lin3(1.0, 1.0) == 9 and S.scale_exp_lin3(2.0 ** -8, 1.0) == 9 and S.scale_exp_lin3(1.0, 2.0 ** -8) == 13
    for m in (0.3, 1.0, 77.0, 5000.0):
        W = np.array([[m, -m / 3, m * 2.0 ** -9]], np.float32)
        hi, lo, e = S.weight_planes(W)
        assert 4096.0 <= float(np.abs(hi.astype(np.float64)).max()) <= 8192.0
        got = (hi.astype(np.float64) + lo.astype(np.float64)) * 2.0 ** -e
        assert (np.abs(got - W) <= 2.0 ** -22 * np.abs(W)).all()       # both planes to nearest: 22 bits and better


# row rms 2^-k -> the relative error of an 80 -> 128 Linear over 70 rows that the issue's emulation predicted
TABLE = {8: 4.3e-6, 10: 1.7e-5, 12: 8.2e-5, 14: 2.8e-4}


def test_error_versus_amplitude_table():
    for k in (0, 2, 4):
        assert S.predicted_rel(*S.table_case(k)) < 4e-7, k
    for k, want in TABLE.items():
        got = S.predicted_rel(*S.table_case(k))
        print(f"row rms 2^-{k}: predicted {got:.2e} (table {want:.1e})")
        assert want / 2 <= got <= want * 2, (k, got, want)
    # the loss is the operand's, not the weights': the same rows scaled by 2^12 (an exact scaling) are back at 22 bits
    x, W = S.table_case(12)
    assert S.predicted_rel(x * np.float32(4096.0), W) < 4e-7


def test_low_side_of_the_weight_side_conditions():
    """Where the other operands of the split products reach 1e-5 on their low side: a LayerNorm + SiLU operand
    16 silu(gamma xhat + beta) with beta = 0 at gamma = 2^-12 (with an ordinary beta never: the operand is then of the size of 16 silu(beta)
    and what gamma xhat adds is carried as an absolute 2^-25 / 16 beside it), a weight at max|W| = 2^-32 -- 21 binades under the exponent
    clamp of scale_exp, where the planes' own lo parts turn subnormal.  x 2^-6 and x 2^-20, which the GPU tests run, are far inside both."""
    rng = np.random.default_rng(5)
    xh = rng.standard_normal((70, 128))
    W = (rng.uniform(-1, 1, (128, 128)) / np.sqrt(128)).astype(np.float32)
    silu = lambda u: u / (1 + np.exp(-u))                                        # noqa: E731
    g = {k: S.predicted_rel(silu(2.0 ** -k * xh).astype(np.float32), W, scale=S.ACT_SCALE) for k in (6, 10, 12, 14)}
    assert g[6] < 4e-7 and g[10] < 5e-6 < g[12] < 2e-5 < g[14], g
    beta = 0.1 * rng.standard_normal(128)
    assert S.predicted_rel(silu(2.0 ** -14 * xh + beta).astype(np.float32), W, scale=S.ACT_SCALE) < 4e-7
    x = silu(xh).astype(np.float32)
    w = {k: S.predicted_rel(x, W * np.float32(2.0 ** -k), scale=S.ACT_SCALE) for k in (20, 24, 28, 32)}
    assert w[20] < 4e-7 and w[24] < 1e-6 and 2e-6 < w[28] < 2e-5 < w[32], w
    assert S.scale_exp(np.abs(W).max() * 2.0 ** -20) == 24
