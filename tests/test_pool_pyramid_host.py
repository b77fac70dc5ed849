"""CPU: the numpy restatement of the pool pyramid launch (tests/pool_pyramid_ref.py) against float64 - the pools against three
cascaded torch.nn.AvgPool2d(3, 1, 1) + bias + ReLU, the fold against float64 mat-vecs - and its fmaf against cases whose single
rounding differs from a float64 multiply-add's two."""
import numpy as np
import torch

import pool_pyramid_ref as ref


def _planes_to_nchw(x):  # [g, h, w, 4] -> [1, 4g, h, w]
    g, h, w, _ = x.shape
    return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2)).reshape(1, 4 * g, h, w).astype(np.float64))


def test_pools_agree_with_cascaded_avgpool_in_float64():
    rng = np.random.default_rng(5)
    c4 = 2
    pool = torch.nn.AvgPool2d(3, 1, 1)
    for h, w in ((1, 40), (9, 33), (17, 70)):
        z = rng.standard_normal((4 * c4, h, w, 4)).astype(np.float32)
        z2 = rng.standard_normal((4 * c4, h, w, 4)).astype(np.float32)
        biases = [rng.standard_normal(c4 * 4).astype(np.float32) * 0.3 for _ in range(3)]
        bias0 = rng.standard_normal(c4 * 4).astype(np.float32) * 0.3
        for second in (None, z2):
            got = ref.pyramid(z, biases, c4, second, bias0 if second is not None else None)
            zz = _planes_to_nchw(z) if second is None else _planes_to_nchw(z) + _planes_to_nchw(second)
            for b in (1, 2, 3):
                x = zz[:, 4 * b * c4:4 * (b + 1) * c4]
                for _ in range(b):
                    x = pool(x)
                want = torch.relu(x + torch.from_numpy(biases[b - 1].astype(np.float64)).view(1, -1, 1, 1))
                err = (_planes_to_nchw(got[b - 1]) - want).abs().max().item()
                assert err <= 1e-6, (h, w, b, err)
            if second is not None:
                want = torch.relu(zz[:, :4 * c4] + torch.from_numpy(bias0.astype(np.float64)).view(1, -1, 1, 1))
                assert (_planes_to_nchw(got[3]) - want).abs().max().item() <= 1e-6


def test_split_planes_hold_the_value_to_22_bits():
    rng = np.random.default_rng(6)
    x = np.abs(rng.standard_normal((3, 5, 7, 4))).astype(np.float32)
    halves = ref.split_pack(x).view(np.float16).astype(np.float32)
    back = halves[..., :4] + halves[..., 4:]
    assert np.abs(back - x).max() <= 2.0 ** -21 * np.abs(x).max()


def test_fma_rounds_once():
    f = np.float32
    # a * b = 1 + 2^-22 + 2^-46: with c = 2^-24 the exact sum lies just above the tie between 1 + 2 ulp and 1 + 3 ulp, so one rounding
    # goes up; the fp32 product rounds to 1 + 2 ulp first and the tie then goes to even (down)
    a = b = f(1 + 2.0 ** -23)
    exact = ref.fma32(a, b, f(2.0 ** -24))
    twice = f(f(a * b) + f(2.0 ** -24))
    assert exact == f(1 + 3 * 2.0 ** -23) and twice == f(1 + 2 * 2.0 ** -23)
    # exact cancellation, signed zeros, non-finite operands, the subnormal range
    assert ref.fma32(f(3), f(-2), f(6)) == 0 and not np.signbit(ref.fma32(f(3), f(-2), f(6)))
    assert np.signbit(ref.fma32(f(-0.0), f(2), f(-0.0)))
    assert np.isnan(ref.fma32(f(0), f(np.nan), f(1))) and ref.fma32(f(np.inf), f(1), f(1)) == np.inf
    assert ref.fma32(f(2.0 ** -100), f(2.0 ** -49), f(0)) == f(2.0 ** -149)
    assert ref.fma32(f(2.0 ** -100), f(2.0 ** -50), f(0)) == 0  # the tie to even at half the smallest subnormal
    assert ref.fma32(f(3.0e38), f(2), f(0)) == np.inf


def test_fold_agrees_with_float64_matvecs():
    rng = np.random.default_rng(7)
    cphys, c_out, npix, bias_len = 36, 34, 8 * 224, 48
    fix = rng.integers(-2 ** 36, 2 ** 36, size=(ref.SHARDS, ref.COL_MAX), dtype=np.int64)
    fix[:, cphys:] = 0
    bad = np.zeros(ref.COL_MAX, np.uint32)
    wg_t = (rng.standard_normal((cphys, c_out)) * 0.2).astype(np.float32)
    wfg_t = (rng.standard_normal((c_out, c_out)) * 0.2).astype(np.float32)
    bg, bf = rng.standard_normal(c_out).astype(np.float32), rng.standard_normal(c_out).astype(np.float32)
    got = ref.fold(fix, bad, npix, wg_t, bg, wfg_t, bf, bias_len)
    mean = fix.sum(axis=0).astype(np.float64)[:cphys] / ref.COL_SCALE / npix
    g = bg.astype(np.float64) + wg_t.astype(np.float64).T @ mean
    want = bf.astype(np.float64) + wfg_t.astype(np.float64).T @ g
    # fp32 chains of n steps: each step rounds once, |error| <= n * 2^-24 * sum |terms| per mat-vec (first order), the first one's
    # error enters the second through |wfg_t|
    e1 = (cphys + 2) * 2.0 ** -24 * (np.abs(bg) + np.abs(wg_t.astype(np.float64)).T @ np.abs(mean))
    e2 = (c_out + 1) * 2.0 ** -24 * (np.abs(bf) + np.abs(wfg_t.astype(np.float64)).T @ np.abs(g)) + np.abs(wfg_t.astype(np.float64)).T @ e1
    assert (np.abs(got[:c_out] - want) <= e2).all(), float(np.abs(got[:c_out] - want).max())
    assert np.abs(got[:c_out] - want).max() > 0  # (fp32 it is)
    assert (got[c_out:] == 0).all() and got.shape == (bias_len,)
    # a flagged channel: NaN mean, NaN everywhere below; an all-zero channel contributes nothing
    bad[3] = 1
    assert np.isnan(ref.fold_mean(fix, bad, cphys, npix)[3])
    assert np.isnan(ref.fold(fix, bad, npix, wg_t, bg, wfg_t, bf, bias_len)[:c_out]).all()
    bad[3] = 0
    fix0 = fix.copy()
    fix0[:, 5] = 0
    w0 = wg_t.copy()
    w0[5] = 7.0
    assert (ref.fold(fix0, bad, npix, w0, bg, wfg_t, bf, bias_len) == ref.fold(fix0, bad, npix, wg_t, bg, wfg_t, bf, bias_len)).all()


def test_the_kernels_division_by_nine_is_the_correctly_rounded_one():
    """div9 (multiply, exact residual, correction: five instructions) against x / 9 in fp32 on every binade - the subnormals, the smallest
    and largest normals included - with the mantissas at the binade's ends, around the multiples of nine (exact quotients and their
    neighbours) and a seeded random sample; zeros with both signs, infinities, NaN.  (All 2^32 bit patterns were compared once on the
    host when the kernel got this form; this keeps a sample of every binade in the suite.)"""
    rng = np.random.default_rng(9)
    mant = np.concatenate([np.array([0, 1, 2, 8, 9, 10, 0x7ffffe, 0x7fffff, 0x400000, 0x100000, 0x638e38, 0x638e39, 0x638e3a]),
                           rng.integers(0, 1 << 23, size=40)]).astype(np.uint32)
    bits = (np.arange(0, 255, dtype=np.uint32)[:, None] << 23 | mant[None, :]).reshape(-1)
    bits = np.concatenate([bits, bits | np.uint32(0x80000000)])
    xs = bits.view(np.float32)
    for x in xs:
        want = x / np.float32(9.0)
        got = ref.div9(x)
        assert got.view(np.uint32) == want.view(np.uint32), (float(x), float(got), float(want))
    for x in (np.float32(0.0), np.float32(-0.0), np.float32(np.inf), np.float32(-np.inf)):
        assert ref.div9(x).view(np.uint32) == (x / np.float32(9.0)).view(np.uint32)
    assert np.isnan(ref.div9(np.float32(np.nan)))
