"""CPU restatement of the split-f16 operand split (csrc/dsg_split.hpp: split_pair, scale_exp, k_pack_h, mfma_step_h), in numpy alone:
nothing here comes from the package or its kernels.

  * an activation operand v (float32, already multiplied by its scale: kRawScale = 1 for raw operands, kActScale = 16 behind
    LayerNorm + SiLU) becomes hi + lo: hi = fp16(v) rounded TOWARD ZERO (v_cvt_pkrtz: never inf, beyond +-65504 it saturates there),
    lo = fp16(v - hi), the float32 remainder (exact in float32) rounded to NEAREST EVEN with fp16 subnormals kept (v_fma_mixlo_f16);
  * a weight W becomes the planes of W * 2^e: hi = fp16(.) and lo = fp16(. - hi), both to nearest even (k_pack_h), with
    e = floor(log2(8192 / max|W|)) clamped to [-8, 24] (scale_exp);
  * the product is hi*hi + hi*lo + lo*hi (the lo*lo term is dropped), accumulated here in float64 -- the device accumulates in float32,
    whose own error is the float32 oracle's business, not the split's -- and un-scaled by 2^-e / scale.

Where the split loses bits: fp16 has 11 significant bits down to 2^-14 and a fixed spacing of 2^-24 below.  For v in binade 2^E the
remainder v - hi is below 2^(E-10), where fp16's spacing is 2^(E-21) -- as long as that is not below the subnormal spacing 2^-24, i.e. for
E >= -3: there hi + lo carries 22 bits (|hi + lo - v| <= 2^(E-22) <= 2^-22 |v|).  In [2^-4, 2^-3) the remainder is below 2^-14, always a
subnormal, and one bit is gone (2^-21 |v|); below 2^-4 the operand carries an ABSOLUTE error of up to 2^-25 whatever its size: a bit per
binade.
"""
import numpy as np

F16_MAX = 65504.0
ACT_SCALE = 16.0           # kActScale
RAW_SCALE = 1.0            # kRawScale
FULL_BITS_FROM = 2.0 ** -3       # |v| from which hi + lo carries 22 bits
LO_SUBNORMAL_BELOW = 2.0 ** -4   # |v| below which the operand loses a bit per binade (in between: 21 bits)
SUBNORMAL_ABS_ERR = 2.0 ** -25   # half the fp16 subnormal spacing: the operand's absolute error wherever lo is a subnormal
_F = np.float32


def rtz16(v):
    """float32 -> fp16 rounded toward zero, subnormals kept, saturating at +-65504."""
    v = np.asarray(v, dtype=_F)
    with np.errstate(over="ignore"):
        h = v.astype(np.float16)                     # to nearest even; may overflow to inf
    bits = h.view(np.uint16).copy()
    away = np.abs(h.astype(np.float64)) > np.abs(v.astype(np.float64))     # rounded away from zero (inf included): one step back
    bits[away] -= 1                                  # sign-magnitude: the previous magnitude, same sign; inf -> 65504
    return bits.view(np.float16)


def rne16(v):
    """float32 -> fp16 to nearest even, subnormals kept."""
    with np.errstate(over="ignore"):
        return np.asarray(v, dtype=_F).astype(np.float16)


def split(v):
    """(hi, lo) fp16 arrays of the activation operand v (float32, scale applied)."""
    v = np.asarray(v, dtype=_F)
    hi = rtz16(v)
    lo = rne16(v - hi.astype(_F))                    # the float32 subtraction is exact for |v| <= 65504
    return hi, lo


def operand_error(v):
    """|hi + lo - v| in float64: the operand's own error."""
    v = np.asarray(v, dtype=_F)
    hi, lo = split(v)
    return np.abs(hi.astype(np.float64) + lo.astype(np.float64) - v.astype(np.float64))


def scale_exp(maxabs):
    """Weight scale exponent of one Linear: max|W| * 2^e in [4096, 8192), e clamped to [-8, 24] (float32 arithmetic as the kernel's)."""
    e = int(np.floor(np.log2(_F(8192.0) / max(_F(maxabs), _F(1e-30)))))
    return max(-8, min(24, e))


def scale_exp_lin3(m3, msc):
    """lin3 and the Linear shortcut share an accumulator: lin3 uses this exponent, the shortcut this + 4."""
    return min(scale_exp(m3), scale_exp(msc) - 4)


def weight_planes(W, e=None):
    """(hi, lo, e): fp16 planes of W * 2^e, both rounded to nearest even."""
    W = np.asarray(W, dtype=_F)
    if e is None:
        e = scale_exp(np.abs(W).max())
    ws = W * _F(2.0 ** e)                            # a power of two: exact
    hi = rne16(ws)
    lo = rne16(ws - hi.astype(_F))
    return hi, lo, e


def linear(x, W, scale=RAW_SCALE, e=None):
    """x @ W.T as the split path forms it (no bias): the three products in float64, un-scaled."""
    v = np.asarray(x, dtype=_F) * _F(scale)
    xh, xl = (a.astype(np.float64) for a in split(v))
    wh, wl, e = weight_planes(W, e)
    wh, wl = wh.astype(np.float64), wl.astype(np.float64)
    acc = xh @ wh.T + xl @ wh.T + xh @ wl.T
    return acc * (2.0 ** -e / scale)


def predicted_rel(x, W, scale=RAW_SCALE, e=None):
    """max|split - exact| / max|exact| of one Linear x @ W.T over the float64 product of the float32 operands: what the split alone costs."""
    ref = np.asarray(x, dtype=np.float64) @ np.asarray(W, dtype=np.float64).T
    return float(np.abs(linear(x, W, scale, e) - ref).max() / max(np.abs(ref).max(), 1e-300))


def table_case(k, rows=70, n_in=80, n_out=128, seed=0):
    """The operands of the error-versus-amplitude table (tests/test_split_cpu.py): `rows` normal rows of rms 2^-k into an n_in -> n_out
    Linear with uniform weights of the usual 1 / sqrt(n_in) size."""
    rng = np.random.default_rng([seed, k])
    W = (rng.uniform(-1.0, 1.0, (n_out, n_in)) / np.sqrt(n_in)).astype(_F)
    x = (rng.standard_normal((rows, n_in)) * 2.0 ** -k).astype(_F)
    return x, W
