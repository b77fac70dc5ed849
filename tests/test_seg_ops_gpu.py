"""-m gpu: the streaming operators of csrc/ojf_seg_ops.hip, called through the C ABI, against their float64 restatement
(seg_ops_ref.py, proven against torch on the CPU by test_stream_ops_host.py) at the shapes and edges where they take
another path.  Every destination is a guarded buffer: wider and longer than the operator's target and pre-filled with a
sentinel that must survive everywhere outside the target; the pad floats of every input row hold NaN, which must not leak
into a result.  Bit-exact operators are held to equality, sums to a bound counted from the kernel's roundings (each test
prints its worst error / bound as a ``RATIO`` line)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import seg_ops_ref as ref
import stream_ops_cases as cases
from stream_ops_cases import Guarded, Rows, same_bits

pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # unit roundoff of fp32
F32 = np.float32


def api(cuda):
    from online_joint_depthfusion_and_semantic_amd import _lib
    _lib.require_gpu()
    return _lib.load(), _lib.stream_ptr(cuda)


def up(x, m):
    return (x + m - 1) // m * m


def ratio_line(name, case, ratio):
    print('RATIO {} {} {:.3f}'.format(name, case, ratio))


# ---- bit-exact operators ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', [(1, 1), (37, 53)])
def test_pack_input_bits_and_bounds(cuda, h, w):
    """image / 255 and depth / 1 (a true division), three planes and the replicated depth plane, NaN and negative values,
    into rows of 8 and into a slice of rows of 12: equal to the reference, channels 3..7 zero, nothing else written."""
    L, st = api(cuda)
    img, depth = cases.pack_image(h, w)
    for src, chan_stride in ((img, h * w), (depth, 0)):
        d = torch.from_numpy(src).to(cuda)
        for div in (255.0, 1.0):
            want = ref.pack_input(src, div).astype(F32)
            for stride, off in ((8, 0), (12, 3)):
                out = Guarded(cuda, h * w, 8, stride, off)
                assert L.ojf_seg_pack_input(d.data_ptr(), chan_stride, div, h, w, out.ptr, stride, st) == 0
                assert same_bits(out.read(), want), (chan_stride, div, stride)


@pytest.mark.parametrize('sliced', [False, True], ids=['rows', 'slice'])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('shape', cases.MAXPOOL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_maxpool_bits_and_bounds(cuda, shape, B, sliced):
    """MaxPool2d(3, 2, 1) with -Inf padding on [B, H, W, C]: one pixel, one row, one column, C no multiple of the 4-channel
    group, several images (a window never crosses into the next image), NaN / +Inf / -Inf at a corner, on an edge and inside
    (a NaN in the window wins, a window of -Inf gives -Inf), input and output as channel slices at odd offsets."""
    L, st = api(cuda)
    C, H, W = shape
    x = cases.maxpool_input(C, H, W, B)
    want = ref.maxpool3s2p1(x)
    Ho, Wo = want.shape[1:3]
    inp = Rows(cuda, x.reshape(-1, C), C + 5, 3) if sliced else Rows(cuda, x.reshape(-1, C))
    out = Guarded(cuda, B * Ho * Wo, C, C + 3, 2) if sliced else Guarded(cuda, B * Ho * Wo, C)
    assert L.ojf_seg_maxpool_batch(B, inp.ptr, inp.stride, C, H, W, out.ptr, out.stride, st) == 0
    assert same_bits(out.read(), want.reshape(-1, C).astype(F32))
    if B == 1:
        out1 = Guarded(cuda, Ho * Wo, C, out.stride, out.off)
        assert L.ojf_seg_maxpool(inp.ptr, inp.stride, C, H, W, out1.ptr, out1.stride, st) == 0
        assert same_bits(out1.read(), want.reshape(-1, C).astype(F32))


@pytest.mark.parametrize('C', [1, 5, 64, 65])
@pytest.mark.parametrize('npix', [1, 33, 300])
def test_broadcast_bits_and_bounds(cuda, C, npix):
    """out[p][c] = vec[c] (* mul[p][c]): one fp32 product, so equal to the rounded float64 one; plain and into / from slices."""
    L, st = api(cuda)
    v = cases.positive((C,), [C, npix]) - F32(1.0)
    g = cases.positive((npix, C), [C, npix, 1]) - F32(0.75)
    vec = torch.from_numpy(v).to(cuda)
    for gate in (None, g):
        for sliced in (False, True):
            mul = None if gate is None else (Rows(cuda, gate, C + 7, 5) if sliced else Rows(cuda, gate))
            out = Guarded(cuda, npix, C, C + 3, 1) if sliced else Guarded(cuda, npix, C)
            rc = L.ojf_seg_broadcast(vec.data_ptr(), mul.ptr if mul else None, mul.stride if mul else 0, C, npix, out.ptr, out.stride, st)
            assert rc == 0 and same_bits(out.read(), ref.broadcast(v, npix, gate).astype(F32))


# ---- sums ------------------------------------------------------------------------------------------------------
def mean_roundings(npix, slices):
    """Roundings on the longest path of a two-stage mean: a phase of a slice adds ceil(ceil(npix / slices) / 4) =
    ceil(npix / (4 slices)) pixels one after the other, two additions join the four phases, ``slices`` additions join the
    slices, one division: ceil(npix / (4 slices)) + slices + 3, bounded by the + 4 of the stated count."""
    return math.ceil(npix / (4 * slices)) + slices + 4


@pytest.mark.parametrize('npix', cases.MEAN_PIXELS)
@pytest.mark.parametrize('C', cases.MEAN_CHANNELS)
def test_mean_within_its_rounding_count(cuda, C, npix):
    """ojf_seg_mean against the float64 mean: C across one, two and five blocks of 64 channels and a second block of the
    finishing launch (C = 300 > 256), pixel counts below, at and above its 32 slices (empty slices, ragged slices), 4800
    pixels; plain rows and a channel slice at an odd offset.
    Bound per channel: (ceil(npix / (4 * 32)) + 32 + 4) * 2^-24 * mean_p |x[p, c]| - every one of the k roundings on a path
    (``mean_roundings``) is relative 2^-24 of a partial sum of non-negative terms, hence of at most the full sum.  Inputs in
    [0.5, 1.5]: a dropped or doubled pixel moves the mean by >= 0.5 / npix, i.e. >= 0.33 / npix relative, against a bound of
    at most 74 * 2^-24 = 4.4e-6 (4800 pixels: 6.9e-5 against 4.4e-6)."""
    L, st = api(cuda)
    x = cases.positive((npix, C), [C, npix])
    want = ref.channel_mean(x)
    bound = mean_roundings(npix, 32) * U * np.abs(x).astype(np.float64).mean(axis=0)
    assert 0.5 / npix > 10 * bound.max()
    worst = 0.0
    for inp in (Rows(cuda, x), Rows(cuda, x, C + 5, 3)):
        partial, out = Guarded(cuda, 1, 32 * C), Guarded(cuda, 1, C)
        assert L.ojf_seg_mean(inp.ptr, inp.stride, C, npix, partial.ptr, out.ptr, st) == 0
        partial.read()  # (scratch: only its bounds matter)
        got = out.read()[0].astype(np.float64)
        worst = max(worst, float((np.abs(got - want) / bound).max()))
    ratio_line('mean', 'C{} npix{}'.format(C, npix), worst)
    assert worst <= 1.0


@pytest.mark.parametrize('idx', range(len(cases.POOL_FC_CASES)), ids=['x'.join(map(str, c[:5])) for c in cases.POOL_FC_CASES])
def test_pool_fc_within_its_rounding_count(cuda, idx):
    """ojf_seg_pool_fc (mean -> W @ mean + b -> ReLU -> broadcast x gate) against float64: the 8- and the 16-slice split
    (npix_in <= / > 1200), the eight-deep weight loop (c_in > 512), c_in = 100 (no multiple of 64), 1024 and 2048 channels
    (the 4-chunk cap of the pixel chunks), one chunk, several, the 64-chunk cap (9216 output pixels), 1, 2, 3 and 8 members,
    bias on all / none / some members, with and without gate, ReLU and none, npix_out != npix_in; odd cases use channel
    slices for inputs, outputs and gates.
    Bound per output: k * 2^-24 * (sum_k |W[c,k]| mean_p|x[p,k]| + |b_c|) * |gate[p,c]| with k = the mean's count
    (``mean_roundings`` with 8 or 16 slices) + ceil(c_in / 64) fused multiply-adds of a lane + 6 butterfly additions + 3
    (bias, gate, one spare); the ReLU is 1-Lipschitz.  Inputs in [0.5, 1.5], weights and biases signed."""
    L, st = api(cuda)
    case = cases.POOL_FC_CASES[idx]
    cin, cout, pin, pout, n, _, _, act = case
    members = cases.pool_fc_inputs(case)
    sliced = idx % 2 == 1
    ins = [Rows(cuda, x, cin + 5, 3) if sliced else Rows(cuda, x) for x, _, _, _ in members]
    ws = [torch.from_numpy(w).to(cuda) for _, w, _, _ in members]
    bs = [None if b is None else torch.from_numpy(b).to(cuda) for _, _, b, _ in members]
    gates = [None if g is None else (Rows(cuda, g, cout + 6, 5) if sliced else Rows(cuda, g)) for _, _, _, g in members]
    outs = [Guarded(cuda, pout, cout, cout + 3, 2) if sliced else Guarded(cuda, pout, cout) for _ in members]
    partial = Guarded(cuda, 1, n * 128 * cin)
    arr = lambda ptrs: (ctypes.c_void_p * n)(*ptrs)
    has_gate = gates[0] is not None
    rc = L.ojf_seg_pool_fc(n, arr([i.ptr for i in ins]), ins[0].stride, cin, pin, arr([w.data_ptr() for w in ws]),
                           arr([None if b is None else b.data_ptr() for b in bs]) if any(b is not None for b in bs) else None,
                           cout, {'none': 0, 'relu': 1}[act], arr([g.ptr for g in gates]) if has_gate else None,
                           gates[0].stride if has_gate else 0, arr([o.ptr for o in outs]), outs[0].stride, pout, partial.ptr, st)
    assert rc == 0
    partial.read()
    k = mean_roundings(pin, 16 if pin > 1200 else 8) + math.ceil(cin / 64) + 6 + 3
    worst = 0.0
    for (x, w, b, g), out in zip(members, outs):
        want = ref.pool_fc(x, w, b, act, pout, g)
        scale = np.abs(w).astype(np.float64) @ np.abs(x).astype(np.float64).mean(axis=0) + (0 if b is None else np.abs(b).astype(np.float64))
        bound = k * U * scale[None, :] * (1.0 if g is None else np.abs(g).astype(np.float64))
        got = out.read().astype(np.float64)
        worst = max(worst, float((np.abs(got - want) / bound).max()))
        if act == 'relu':
            assert (got == 0).any() and (got > 0).any()
    ratio_line('pool_fc', 'x'.join(map(str, case[:5])), worst)
    assert worst <= 1.0


def test_pool_fc_refuses_what_it_cannot_run(cuda):
    """act = sigmoid, c_in = 8193 and 9 members are errors, and nothing is launched: output and scratch keep their sentinels."""
    from online_joint_depthfusion_and_semantic_amd import segconv, _lib
    L, st = api(cuda)

    def call(n, cin, act):
        x = Rows(cuda, cases.positive((1, cin), 1))
        w = torch.zeros((2, cin), device=cuda)
        outs = [Guarded(cuda, 1, 2) for _ in range(n)]
        partial = Guarded(cuda, 1, n * 128 * cin)
        arr = lambda ptrs: (ctypes.c_void_p * n)(*ptrs)
        rc = L.ojf_seg_pool_fc(n, arr([x.ptr] * n), cin, cin, 1, arr([w.data_ptr()] * n), None, 2, act, None, 0, arr([o.ptr for o in outs]), 2,
                               1, partial.ptr, st)
        for g in outs + [partial]:
            assert (g.read() == g.sent).all()
        return rc
    assert call(1, 64, 2) != 0 and b'ojf_seg_pool_fc' in L.ojf_last_error()
    assert call(1, 8193, 1) != 0
    assert call(9, 64, 1) != 0
    fc = segconv.PoolFC(torch.nn.Conv2d(8, 16, 1).to(cuda))
    x, out = segconv.nhwc(8, 3, 3, cuda), segconv.nhwc(16, 3, 3, cuda)
    with pytest.raises(_lib.OjfError):
        segconv.pool_fc([fc], [x], [out], act='sigmoid')
    assert float(out.abs().max()) == 0.0


# ---- softmax + max ---------------------------------------------------------------------------------------------
LAYOUTS = {'pad8': lambda C: (up(C, 8), 0),          # rows padded to 8: the vector form up to 64 classes
           'tight': lambda C: (C, 0),                 # stride == C: scalar form unless C % 4 == 0
           'off2': lambda C: (up(C + 2, 4) + 4, 2),   # a slice 2 floats in: the pointer is off the 16-byte grid
           'off4': lambda C: (up(C + 4, 4) + 4, 4)}   # a slice 4 floats in: aligned, vector form with a wider stride


@pytest.mark.parametrize('layout', list(LAYOUTS))
@pytest.mark.parametrize('C', cases.SOFTMAX_CLASSES)
def test_softmax_max_ids_and_scores(cuda, C, layout):
    """torch.softmax(logits, 1).max(1) over 1 .. 256 classes - the vector form (<= 64 classes, 16-byte aligned rows) up to
    its boundary at 64 / 65, the scalar form behind it, for a stride that is no multiple of 4 and for a misaligned pointer -
    on a 19 x 23 image (two blocks) and on single pixels, with the planted rows of stream_ops_cases.PLANTED_ROWS: an exact tie
    (first maximum wins), NaN behind the maximum, NaN first, +Inf behind the maximum, two +Inf, only -Inf (all: score NaN,
    id 0, as the all-NaN softmax row of the reference gives), -Inf among finite values.  The pads of every row hold NaN.
    Ids: equal.  Scores: (C + 8) * 2^-24 relative - l - max is exact for these logits (multiples of 2^-9 below 8), expf is
    within 1 ulp = 2 * 2^-24, C - 1 additions of non-negative terms and one division round once each: C + 2, bounded by the
    stated C + 8.
    Left out: logits closer than about 2^-26 relative.  Their softmax values are EQUAL in fp32, so the reference's first
    maximum is then decided by torch's exp to the ulp, while the kernel takes the larger logit; the logits here are distinct
    multiples of 2^-9 (>= 1.9e-3 apart), planted ties aside, where both rules agree."""
    L, st = api(cuda)
    stride, off = LAYOUTS[layout](C)
    images = [('19x23', cases.softmax_image(C, 19 * 23, 0)), ('1x1', cases.softmax_logits(C, 1, 5))]
    images += [('1x1 ' + kind, row[None]) for k, kind in enumerate(cases.PLANTED_ROWS)
               for row in [cases.planted_row(kind, C, k)] if row is not None]
    worst = 0.0
    for name, logits in images:
        npix = logits.shape[0]
        want_s, want_i = ref.softmax_max(logits)
        inp = Rows(cuda, logits, stride, off)
        assert (inp.ptr % 16 == 0) == (off % 4 == 0)
        scores, ids = Guarded(cuda, 1, npix), Guarded(cuda, 1, npix, dtype=np.uint8)
        assert L.ojf_seg_softmax_max(inp.ptr, stride, C, npix, scores.ptr, ids.ptr, st) == 0
        got_s, got_i = scores.read()[0].astype(np.float64), ids.read()[0]
        assert np.array_equal(got_i, want_i.astype(np.uint8)), (name, np.flatnonzero(got_i != want_i)[:8])
        assert np.array_equal(np.isnan(got_s), np.isnan(want_s)), name
        ok = ~np.isnan(want_s)
        if ok.any():
            worst = max(worst, float((np.abs(got_s[ok] - want_s[ok]) / ((C + 8) * U * want_s[ok])).max()))
    ratio_line('softmax', 'C{} {}'.format(C, layout), worst)
    assert worst <= 1.0
