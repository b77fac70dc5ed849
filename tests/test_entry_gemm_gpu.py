"""GPU: the stand-alone branch-entry GEMM of a VortexPooling through ojf_entry_gemm - the persistent form the net launches (form 1: a
block walks several 64-pixel strips, the next strip's planes in flight while one computes) against the one-strip-per-block kernel (form
0) bit for bit, and both against a float64 restatement (tests/entry_gemm_ref.py).

"Bit for bit" covers every output plane, the `bad` flags and the channel sums as integers: the SUM of the 16 fix[] shards per channel.
Which shard a strip adds into differs between the forms (it is the block's index modulo 16, and the forms hand strips to different
blocks); the fold that reads ColSums adds the shards as integers, so their sum is the value.

Bound against float64: 1e-5 * sum_k |w_k x_k| per output element - fp32 accumulation over 128 terms, 128 * 2^-24 = 7.6e-6, dominates the
split's 3 * 2^-22 = 7.2e-7 - and the same factor on sum |x| for the channel sums (the 2^-20 fixed point adds at most 2^-21 per strip, far
below it: sum |x| is ~0.8 per pixel)."""
import functools

import numpy as np
import pytest
import torch

from online_joint_depthfusion_and_semantic_amd import _lib
import entry_gemm_ref as ref

pytestmark = pytest.mark.gpu

C_IN, C4_IN, CS, ACT_N = 120, 30, 20, 20  # 30 groups: the `G < c4_in` guard is live in the eighth input tile
C_OUT = 4 * CS

# (npix, caps on the persistent grid; 0 = the product rule)
SHAPES = [
    (9, (0,)),                 # one strip, three idle waves
    (480, (8, 3, 1)),          # eight strips, banded, the last strip half idle
    (1536, (24, 16, 8, 5)),    # 24 strips: banded walks of 1, 1-2 and 3 strips per block; a grid that is no multiple of 8: the plain stride
    (1961, (31, 8, 5, 1)),     # 31 strips, unbanded, npix % 64 == 41: the last strip first, in the middle and last in a block's walk
]
RUNS = [(npix, mb) for npix, caps in SHAPES for mb in caps]


@functools.lru_cache(maxsize=None)
def layer():
    rng = np.random.default_rng(5)
    w = (rng.standard_normal((C_OUT, C_IN)) * 0.1).astype(np.float32)
    b = (rng.standard_normal(C_OUT) * 0.3).astype(np.float32)
    w.setflags(write=False)
    b.setflags(write=False)
    return w, b


@functools.lru_cache(maxsize=None)
def inputs(npix, in_split, special=None):
    """-> (planes as the kernel gets them [C4_IN, npix, 4] float32 bit patterns, the values they mean [C_IN, npix]); shared, never modified"""
    rng = np.random.default_rng(100 + npix)
    x = rng.standard_normal((C_IN, npix)).astype(np.float32)
    if special == 'nan':
        x[37, npix // 2] = np.nan
    if special == 'inf':
        x[90, npix - 1] = np.inf
    if special == 'ones':
        x[0, :] = 1.0
    p = ref.to_planes(x)
    if in_split:
        p = ref.split_planes(p)
        x = ref.from_planes(ref.unsplit_planes(p))
    p.setflags(write=False)
    x.setflags(write=False)
    return p, x


def launch(cuda, planes, weight, bias, form, max_blocks, in_split, split_groups, og_store=CS):
    """One call -> (output planes [CS, npix, 4] as stored, fix [16, 256] int64, bad [256] uint32)"""
    npix = planes.shape[1]
    buf = torch.zeros((1 + C4_IN * npix) * 4, device=cuda)  # a zero float4 in front of the planes: what lanes outside the frame read
    buf[4:] = torch.from_numpy(planes.reshape(-1).copy()).to(cuda)
    out = torch.full((CS, npix, 4), -7.0, device=cuda)      # a pattern no result has: a pixel the launch misses shows
    colsums = torch.zeros(ref.SHARDS * ref.COL_MAX * 8 + ref.COL_MAX * 4, dtype=torch.uint8, device=cuda)
    lib = _lib.load()
    rc = lib.ojf_entry_gemm(_lib.ptr(weight), _lib.ptr(bias), C_IN, CS, _lib.ptr(buf) + 16, int(in_split), C4_IN, npix, _lib.ptr(out),
                            og_store, split_groups, ACT_N, _lib.ptr(colsums), form, max_blocks, _lib.stream_ptr(cuda))
    _lib.check(rc, 'ojf_entry_gemm')
    cs = colsums.cpu().numpy()
    fix = cs[:ref.SHARDS * ref.COL_MAX * 8].view(np.int64).reshape(ref.SHARDS, ref.COL_MAX)
    bad = cs[ref.SHARDS * ref.COL_MAX * 8:].view(np.uint32)
    return out.cpu().numpy(), fix, bad


@functools.lru_cache(maxsize=None)
def one_strip_form(npix, in_split, split_groups, special=None):
    """Form 0 on the shared case, once (the `cuda` fixture's device)"""
    w, b = layer()
    return launch(torch.device('cuda:0'), inputs(npix, in_split, special)[0], w, b, 0, 0, in_split, split_groups)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def values(out, split_groups):
    """stored planes -> [C_OUT, npix] fp32 values (the first split_groups groups are split planes)"""
    v = out.copy()
    if split_groups:
        v[:split_groups] = ref.unsplit_planes(out[:split_groups])
    return ref.from_planes(v)


def guard_fired(cuda):
    """ojf_net_check: nonzero when the process-wide range guard fired since the last check; re-arms it"""
    return _lib.load().ojf_net_check(_lib.stream_ptr(cuda)) != 0


@pytest.mark.parametrize('split_groups', [0, 5])
@pytest.mark.parametrize('in_split', [0, 1])
@pytest.mark.parametrize('npix,max_blocks', RUNS)
def test_persistent_form_equals_the_one_strip_form_bit_for_bit(cuda, npix, max_blocks, in_split, split_groups):
    w, b = layer()
    want, want_fix, want_bad = one_strip_form(npix, in_split, split_groups)
    got, fix, bad = launch(cuda, inputs(npix, in_split)[0], w, b, 1, max_blocks, in_split, split_groups)
    wrong = bits(got) != bits(want)
    assert not wrong.any(), (int(wrong.sum()), np.argwhere(wrong)[:4].tolist())
    assert np.array_equal(fix.sum(axis=0), want_fix.sum(axis=0))  # int64: exact
    assert np.array_equal(bad, want_bad) and not bad.any()
    assert not guard_fired(cuda)


@pytest.mark.parametrize('form', [0, 1])
@pytest.mark.parametrize('split_groups', [0, 5])
@pytest.mark.parametrize('in_split', [0, 1])
@pytest.mark.parametrize('npix', [n for n, _ in SHAPES])
def test_both_forms_against_float64(cuda, npix, in_split, split_groups, form):
    w, b = layer()
    planes, x = inputs(npix, in_split)
    got, fix, bad = one_strip_form(npix, in_split, split_groups) if form == 0 else launch(cuda, planes, w, b, 1, 0, in_split, split_groups)
    want, mag = ref.gemm(w, b, x, ACT_N)
    err = np.abs(values(got, split_groups).astype(np.float64) - want)
    print('npix %d in_split %d split_groups %d form %d: max err / (sum |w x|) = %.3g' % (npix, in_split, split_groups, form, (err / mag).max()))
    assert (err <= 1e-5 * mag).all(), float((err / mag).max())
    sums, mags = ref.column_sums(x)
    got_sums = fix.sum(axis=0)[:C_IN].astype(np.float64) / ref.COL_SCALE
    print('   channel sums: max err / (sum |x|) = %.3g' % (np.abs(got_sums - sums) / mags).max())
    assert (np.abs(got_sums - sums) <= 1e-5 * mags).all()
    assert not fix[:, C_IN:].any() and not bad.any()


@pytest.mark.parametrize('special,in_split', [('nan', 0), ('nan', 1), ('inf', 0)])
def test_nan_and_inf_pixels_flag_and_spread_alike(cuda, special, in_split):
    """One NaN / one Inf input value: the channel's `bad` flag and the NaN outputs of its pixel are the same in both forms (1961 pixels
    under 5 blocks: the pixel's strip comes late in a walk).  The range guard is read (and re-armed) after each form."""
    npix = 1961
    w, b = layer()
    want, want_fix, want_bad = one_strip_form(npix, in_split, 5, special)
    guard0 = guard_fired(cuda)
    got, fix, bad = launch(cuda, inputs(npix, in_split, special)[0], w, b, 1, 5, in_split, 5)
    guard1 = guard_fired(cuda)
    ch = 37 if special == 'nan' else 90
    assert want_bad[ch] == 1 and want_bad.sum() == 1 and np.array_equal(bad, want_bad)
    assert np.array_equal(fix.sum(axis=0), want_fix.sum(axis=0))
    nan_want, nan_got = np.isnan(values(want, 5)), np.isnan(values(got, 5))
    assert nan_want.any() and np.array_equal(nan_got, nan_want)
    assert set(np.argwhere(nan_want)[:, 1].tolist()) == {npix // 2 if special == 'nan' else npix - 1}  # that pixel's column only
    nan_planes = np.isnan(got)
    nan_planes[:5] = np.isnan(ref.unsplit_planes(got[:5]))  # the first five groups are stored as split planes
    assert ((bits(got) == bits(want)) | nan_planes).all()
    assert guard0 == guard1  # (NaN is no range violation; what an Inf does to the guard, it does in both forms)


@pytest.mark.parametrize('form', [0, 1])
def test_range_guard_sees_stored_elements_only(cuda, form):
    """A stored pre-activation beyond 65504 is reported by ojf_net_check after either form; the same magnitude in a channel group that is
    not stored (og_store), or in lanes past npix, is not."""
    npix = 1961  # 41 pixels in the last strip: 23 lanes past npix compute, and must not report
    w0, b0 = layer()
    planes, x = inputs(npix, 1)
    assert not guard_fired(cuda)
    # row 77 (group 19) times 1e6: |pre-activation| ~ 1e6
    w = w0.copy()
    w[77] *= 1e6
    launch(cuda, planes, w, b0, form, 5, 1, 5)
    assert guard_fired(cuda)
    launch(cuda, planes, w, b0, form, 5, 1, 5, og_store=19)  # group 19 is computed, not stored
    assert not guard_fired(cuda)
    # channel 0 is 1.0 at every pixel; row 30 = -1e5 on it, bias 1e5: exactly 0 inside the frame, 1e5 in the lanes past it (they read zeros)
    ones, _ = inputs(npix, 1, 'ones')
    w, b = w0.copy(), b0.copy()
    w[30] = 0.0
    w[30, 0] = -1e5
    b[30] = 1e5
    got, _, _ = launch(cuda, ones, w, b, form, 5, 1, 5)
    assert (values(got, 5)[30] == 0.0).all()
    assert not guard_fired(cuda)
    b[30] = 2e5  # now 1e5 inside the frame as well
    launch(cuda, ones, w, b, form, 5, 1, 5)
    assert guard_fired(cuda)
