"""CPU restatement of the library's random draws, in numpy alone: nothing here comes from the package or its kernels.

  * Philox4x32-10 (Salmon et al. 2011) on uint64 arrays that hold 32-bit words;
  * the draw contract: counter (idx4 & 0xffffffff, idx4 >> 32, stream, 0x5eed), key (seed & 0xffffffff, seed >> 32); one counter gives the
    four words of quad `idx4`, element 4 * idx4 + p takes word p;
  * the uniform mapping u = ((w >> 8) + 0.5f) * 2^-24f EVALUATED IN FLOAT32: from w >> 8 = 2^23 upwards the + 0.5 is lost to rounding
    (ties to even), and w >> 8 = 0xFFFFFF gives u == 1.0 -- a float64 evaluation of u would move z by up to 1.6e-5;
  * Box-Muller in float64 from those float32 uniforms and the float32 angle fl32(6.2831855f * u1) (`f32=True`: every operation in numpy
    float32, which is the measure of what float32 arithmetic alone does to a draw);
  * the streams: reverse step `step` draws z from stream `step`, the start state y_T from stream 0xFFFFFFFF, training call `call` draws
    noise / ts / mask from streams 4 * call + {0, 1, 2} (32-bit wrap);
  * ts and mask: exact integer / float32 rules, restated in numpy float32 so that they compare bit for bit.
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
_MUL0, _MUL1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)      # the two round multipliers
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)          # the key schedule (golden ratio, sqrt(3) - 1)
_S32, _S8 = np.uint64(32), np.uint64(8)
COUNTER3 = 0x5EED                                                 # the fourth counter word of every draw
Y_T_STREAM = 0xFFFFFFFF                                           # the stream of a sampling call's start state
_F = np.float32
_2M24 = _F(1.0 / 16777216.0)
_TWO_PI_F = _F(6.28318530717958647692)                            # 6.2831855f


def _words(x):
    return np.asarray(x, dtype=np.uint64) & M32


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """The ten rounds on (broadcastable) uint64 arrays of 32-bit words; returns the four output words."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(_words(v) for v in (c0, c1, c2, c3, k0, k1)))
    for _ in range(10):
        p0, p1 = _MUL0 * c0, _MUL1 * c2                          # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & M32, (p0 >> _S32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + _W0) & M32, (k1 + _W1) & M32
    return c0, c1, c2, c3


def words(seed, stream, idx4):
    """uint64 [len(idx4)][4]: the four words of every quad `idx4` of `stream` under `seed` (any Python ints; 64 and 32 bits are kept)."""
    seed, stream = int(seed) & (2 ** 64 - 1), int(stream) & 0xFFFFFFFF
    i = np.asarray(idx4, dtype=np.uint64).reshape(-1)
    return np.stack(philox4x32_10(i & M32, i >> _S32, np.uint64(stream), np.uint64(COUNTER3), np.uint64(seed & 0xFFFFFFFF),
                                  np.uint64(seed >> 32)), axis=1)


def uniform_of(w):
    """float32 u in (0, 1] of words `w`: ((w >> 8) + 0.5f) * 2^-24f, every operation rounded to float32."""
    return (((np.asarray(w, dtype=np.uint64) & M32) >> _S8).astype(_F) + _F(0.5)) * _2M24


def uniforms(seed, stream, idx4):
    """float32 [len(idx4)][4]."""
    return uniform_of(words(seed, stream, idx4))


def box_muller(u, f32=False):
    """[..., 4] normals of float32 uniforms [..., 4]: (u0, u1) -> r (cos, sin), (u2, u3) likewise.  float64 from the float32 u and the
    float32 angle; f32=True: all of it in float32."""
    u = np.asarray(u, dtype=_F)
    ang = _TWO_PI_F * u[..., 1::2]                                # float32 product, as the kernel's
    if f32:
        r = np.sqrt(_F(-2.0) * np.log(u[..., 0::2]))
        c, s = np.cos(ang), np.sin(ang)
    else:
        r = np.sqrt(-2.0 * np.log(u[..., 0::2].astype(np.float64)))
        c, s = np.cos(ang.astype(np.float64)), np.sin(ang.astype(np.float64))
    return np.stack((r[..., 0] * c[..., 0], r[..., 0] * s[..., 0], r[..., 1] * c[..., 1], r[..., 1] * s[..., 1]), axis=-1)


def normals(seed, stream, n, f32=False, idx4_base=0):
    """[n] normals: element 4 * idx4 + p is value p of quad idx4 (from `idx4_base` on), truncated to n."""
    n4 = (int(n) + 3) // 4
    idx4 = np.arange(n4, dtype=np.uint64) + np.uint64(idx4_base)
    return box_muller(uniforms(seed, stream, idx4), f32).reshape(-1)[:int(n)]


def train_draws(seed, call, T, keep, B, D, f32=False):
    """(ts int32 [B], noise [B][D], mask float32 [B]) of training call `call`.  Row r takes word r % 4 of quad r // 4."""
    base = 4 * int(call)
    noise = normals(seed, base, B * D, f32).reshape(B, D)
    idx4 = np.arange((B + 3) // 4, dtype=np.uint64)
    u24 = lambda kind: ((words(seed, base + kind, idx4) >> _S8).reshape(-1)[:B].astype(_F) * _2M24)     # exact: 24 bits
    t = (u24(1) * _F(T)).astype(np.int64)                        # float32 product, truncated
    ts = np.minimum(t, int(T) - 1).astype(np.int32)
    mask = (u24(2) < _F(keep)).astype(_F)
    return ts, noise, mask


def sample_draws(seed, K, n, noisy=None, f32=False):
    """(y_T [n], noise [max(K-2, 0)][n]) of a K-step sampling call over n = B * D elements, in the layout of the `noise` argument of
    DDPM.sample: row r belongs to step K-1-r.  `noisy` [K] (column 3 of the coefficient table): rows of steps it marks noise free are
    NaN -- the device draws nothing there and no reference may read them."""
    y_T = normals(seed, Y_T_STREAM, n, f32)
    rows = []
    for r in range(max(K - 2, 0)):
        step = K - 1 - r
        if noisy is not None and not bool(noisy[step]):
            rows.append(np.full(n, np.nan, dtype=y_T.dtype))
        else:
            rows.append(normals(seed, step, n, f32))
    return y_T, (np.stack(rows) if rows else np.zeros((0, n), dtype=y_T.dtype))


def sample_draws_chunked(seeds, K, B, D, chunk_rows, noisy=None, f32=False):
    """The same for a chunked call: chunk c = rows [c * chunk_rows, min(B, (c + 1) * chunk_rows)) draws under seeds[c] with chunk-local
    element indices (the last chunk may be shorter), exactly as its own sample() call.  `noisy`: [K], or one [K] per chunk."""
    ys, zs = [], []
    for c, lo in enumerate(range(0, B, chunk_rows)):
        rows = min(chunk_rows, B - lo)
        nz = noisy[c] if noisy is not None and np.ndim(noisy) == 2 else noisy
        y, z = sample_draws(seeds[c], K, rows * D, nz, f32)
        ys.append(y)
        zs.append(z)
    return np.concatenate(ys), np.concatenate(zs, axis=1)
