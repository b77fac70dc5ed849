"""Plain numpy fp32 restatement of the pool pyramid launch (pool_pyramid_kernel, ojf_pool_pyramid in include/ojf.h): the value
definition the kernel is held to bit for bit.  Not a test; tests/test_pool_pyramid_host.py pins it on float64, the GPU test uses it.

Planes are arrays [group, h, w, 4] of float32 (the kernel's [group][h*w] float4).

Pools: per level the sum starts at zero and adds the nine taps in row-major order, then one correctly rounded division by 9; every
level is zero outside the image; after the last level bias, the NaN-keeping ReLU (x < 0 ? 0 : x) and, for split planes, the split into
fp16 halves {4 high | 4 low}.

Fold: mean[c] = float(double(sum of the 16 shards) * 2^-20) / float(h*w) (NaN where the channel's flag is set), then two mat-vecs as
fmaf chains over ascending input channels, ONE rounding per step: the step is evaluated in exact rational arithmetic and rounded once to
fp32 (a float64 multiply-add rounds twice, and so does a float64 fma followed by the conversion to fp32)."""
from fractions import Fraction
import math

import numpy as np

F32 = np.float32
SHARDS, COL_MAX = 16, 256
COL_SCALE = 1048576.0


def pool_level(x):
    """One nn.AvgPool2d(3, 1, 1) (zero padding, always / 9) of planes [..., h, w, 4] in the kernel's order of operations."""
    h, w = x.shape[-3], x.shape[-2]
    p = np.zeros(x.shape[:-3] + (h + 2, w + 2, 4), F32)
    p[..., 1:-1, 1:-1, :] = x
    s = np.zeros(x.shape, F32)
    with np.errstate(over='ignore'):
        for dy in range(3):
            for dx in range(3):
                s = s + p[..., dy:dy + h, dx:dx + w, :]
    return s / F32(9.0)


def div9(x):
    """The kernel's division by nine as it is written (csrc/ojf_net.hip div9): q = x * RN(1/9), f = fma(fma(-9, q, x), RN(1/9), q), x itself
    where q == x (zeros, infinities).  Must equal x / 9 rounded once for every x: tests/test_pool_pyramid_host.py."""
    r = F32(1.0) / F32(9.0)
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        q = F32(x) * r
    if q == x:
        return F32(x)
    return fma32(fma32(F32(-9.0), q, x), r, q)


def relu_keep_nan(x):
    return np.where(x < 0, F32(0.0), x).astype(F32)


def split_pack(x):
    """float4 -> its split-fp16 form in the same 16 bytes: halves {h0 h1 h2 h3 | l0 l1 l2 l3}, h = fp16(x), l = fp16(x - h) (the
    difference is exact in fp32).  Returned as float32 bit patterns."""
    hi = x.astype(np.float16)
    lo = (x - hi.astype(F32)).astype(np.float16)
    return np.ascontiguousarray(np.concatenate([hi, lo], axis=-1)).view(F32)


def pyramid(z, biases, c4, z2=None, bias0=None, split_out=False):
    """z [4*c4, h, w, 4]; biases: three arrays [c4*4] (branches 1..3).  -> [q1, q2, q3] (+ [q0] with z2), each [c4, h, w, 4]."""
    zz = z if z2 is None else (z + z2).astype(F32)
    out = []
    for b in (1, 2, 3):
        x = zz[b * c4:(b + 1) * c4]
        for _ in range(b):
            x = pool_level(x)
        x = relu_keep_nan(x + biases[b - 1].astype(F32).reshape(c4, 1, 1, 4))
        out.append(split_pack(x) if split_out else x)
    if z2 is not None:
        x = relu_keep_nan((z[:c4] + z2[:c4]) + bias0.astype(F32).reshape(c4, 1, 1, 4))
        out.append(split_pack(x) if split_out else x)
    return out


def _round_f32(fr):
    """exact rational (non-zero) -> the nearest fp32, ties to even"""
    a = abs(fr)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    e = max(e, -126)  # subnormal results: the quantum stays 2^-149
    q = Fraction(2) ** (e - 23)
    n = a / q
    k = n.numerator // n.denominator
    rem = n - k
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (k & 1)):
        k += 1
    v = k * q
    if v >= Fraction(2) ** 128:
        return F32(math.copysign(math.inf, fr))
    return F32(math.copysign(float(v), fr))  # 24 significant bits: exact as a double


def fma32(a, b, c):
    """fmaf(a, b, c) of fp32 values: a * b + c rounded once"""
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        with np.errstate(invalid='ignore'):
            return F32(np.float64(a) * np.float64(b) + np.float64(c))  # NaN / infinity: no rounding involved
    fr = Fraction(a) * Fraction(b) + Fraction(c)
    if fr == 0:
        return F32(a * b + c)  # the product is exact in double and the sum is an exact zero: IEEE's sign of zero
    return _round_f32(fr)


def fold_mean(fix, bad, cphys, npix):
    """fix int64 [16, 256], bad uint32 [256] -> mean float32 [256] (zero from cphys on)"""
    q = fix.astype(np.int64).sum(axis=0)
    s = (q.astype(np.float64) * (1.0 / COL_SCALE)).astype(F32)
    with np.errstate(invalid='ignore'):
        mean = s / F32(npix)
    mean = np.where(bad != 0, F32(np.nan), mean).astype(F32)
    mean[cphys:] = 0
    return mean


def matvec_chain(w_t, x, bias):
    """out[t] = bias[t], then for c ascending: out[t] = fmaf(w_t[c][t], x[c], out[t])"""
    rows, n = w_t.shape
    out = np.empty(n, F32)
    for t in range(n):
        s = F32(bias[t])
        for c in range(rows):
            s = fma32(w_t[c, t], x[c], s)
        out[t] = s
    return out


def fold(fix, bad, npix, wg_t, bg, wfg_t, bf, bias_len):
    """-> bias_out float32 [bias_len]: the final convolution's bias with the global-average branch folded in"""
    cphys, c_out = wg_t.shape
    mean = fold_mean(fix, bad, cphys, npix)
    g = matvec_chain(wg_t, mean, bg)
    out = np.zeros(bias_len, F32)
    out[:c_out] = matvec_chain(wfg_t, g, bf)
    return out
