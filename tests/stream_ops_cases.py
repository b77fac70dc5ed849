"""The inputs of the streaming-operator tests (csrc/ojf_seg_ops.hip, csrc/ojf_volume.hip), shared by the host test that
proves the references (test_stream_ops_host.py) and the GPU tests that use them (test_seg_ops_gpu.py,
test_volume_gpu.py): both see the same ordinary and edge inputs."""
import numpy as np

F = np.float32
H16 = np.float16

def same_bits(a, b):
    """Equal element for element, NaN == NaN, and -0.0 != 0.0."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan = np.isnan(a) if a.dtype.kind == 'f' else np.zeros(a.shape, bool)
    nanb = np.isnan(b) if b.dtype.kind == 'f' else nan
    if not np.array_equal(nan, nanb):
        return False
    if a.dtype.kind == 'f':
        a, b = np.where(nan, 0, a), np.where(nan, 0, b)
        return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))
    return np.array_equal(a, b)


# ---- device buffers of the GPU tests ----------------------------------------------------------------------------
SENTINEL = {np.dtype(np.float32): -7.25e11, np.dtype(np.float64): -7.25e11, np.dtype(np.float16): -1234.0, np.dtype(np.uint8): 0xA5,
            np.dtype(np.int32): -77, np.dtype(np.int64): -77}


class Guarded:
    """A device buffer of sentinels around a target of ``npix`` rows of ``C`` elements, ``stride`` apart, that starts
    ``off`` elements into its row (a channel slice); ``ptr`` is the target's address."""

    def __init__(self, cuda, npix, C, stride=None, off=0, dtype=np.float32, lead=8, tail=8):
        stride = C if stride is None else stride
        assert off + C <= stride
        self.npix, self.C, self.stride, self.off, self.lead = npix, C, stride, off, lead
        self.sent = np.dtype(dtype).type(SENTINEL[np.dtype(dtype)])
        import torch
        self.buf = torch.from_numpy(np.full(lead + npix * stride + tail, self.sent, dtype)).to(cuda)
        self.ptr = self.buf.data_ptr() + (lead + off) * self.buf.element_size()

    def write(self, data):
        """Set the target (an operator that works in place)."""
        import torch
        rows = self.buf[self.lead:self.lead + self.npix * self.stride].view(self.npix, self.stride)
        rows[:, self.off:self.off + self.C] = torch.from_numpy(np.ascontiguousarray(data).reshape(self.npix, self.C)).to(self.buf.device)
        return self

    def read(self):
        """The target [npix, C]; fails if anything outside it has been written."""
        a = self.buf.cpu().numpy().copy()
        rows = a[self.lead:self.lead + self.npix * self.stride].reshape(self.npix, self.stride)
        got = rows[:, self.off:self.off + self.C].copy()
        rows[:, self.off:self.off + self.C] = self.sent
        assert (a == self.sent).all(), 'the operator wrote outside its target'
        return got


class Rows:
    """Input rows on the device: ``data`` [npix, C] as a channel slice ``off`` floats into rows of ``stride``; every other
    float of the buffer (pads, lead, tail) is NaN."""

    def __init__(self, cuda, data, stride=None, off=0):
        npix, C = data.shape
        stride = C if stride is None else stride
        assert off + C <= stride
        a = np.full(npix * stride + 16, np.nan, F)
        a[:npix * stride].reshape(npix, stride)[:, off:off + C] = data
        import torch
        self.buf = torch.from_numpy(a).to(cuda)
        self.ptr, self.stride = self.buf.data_ptr() + 4 * off, stride


# ---- softmax + max ---------------------------------------------------------------------------------------------
SOFTMAX_CLASSES = (1, 2, 5, 30, 64, 65, 100, 256)
PLANTED_ROWS = ('tie', 'nan_later', 'nan_first', 'inf_later', 'two_inf', 'all_ninf', 'ninf_among')


def softmax_logits(C, npix, seed):
    """[npix, C] f32 logits on a grid of 2^-9 in [-4, 4), distinct within a row: two classes differ by >= 1.9e-3, l - max is
    exact in fp32 and in float64, and no two softmax values of a row are equal in either."""
    rng = np.random.default_rng([seed, C, npix])
    k = rng.permuted(np.tile(np.arange(-2048, 2048), (npix, 1)), axis=1)[:, :C]
    return (k * 2.0 ** -9).astype(F)


def planted_row(kind, C, seed=0):
    """One row [C] of ``softmax_logits`` with the named edge planted (None where C is too small for it)."""
    row = softmax_logits(C, 1, 1000 + seed)[0]
    hi = int(np.argmax(row))
    if kind == 'nan_first':
        row[0] = np.nan
    elif kind == 'all_ninf':
        row[:] = -np.inf
    elif C < 2:
        if kind != 'inf_later':
            return None
        row[0] = np.inf  # (the only index there is)
    elif kind == 'tie':  # an exact tie of the maximum: the first wins
        a, b = (0, C - 1) if C < 3 else (1, C - 1)
        row[a] = row[b] = 5.0
    elif kind == 'nan_later':  # the maximum first, a NaN behind it
        row[0], row[hi] = row[hi], row[0]
        row[C - 1] = np.nan
        if C > 3:
            row[C // 2] = np.nan
    elif kind == 'inf_later':
        row[0], row[hi] = row[hi], row[0]
        row[C - 1] = np.inf
    elif kind == 'two_inf':
        row[C // 2] = row[C - 1] = np.inf
    elif kind == 'ninf_among':
        row[0] = -np.inf
        if C > 2:
            row[C - 1] = -np.inf
    return row


def softmax_image(C, npix, seed):
    """``softmax_logits`` with every planted row that C allows written over pixels 3, 3 + 5, ... (where npix allows)."""
    l = softmax_logits(C, npix, seed)
    p = 3
    for i, kind in enumerate(PLANTED_ROWS):
        row = planted_row(kind, C, i)
        if row is not None and p < npix:
            l[p] = row
            p += 5
    return l


# ---- max-pool --------------------------------------------------------------------------------------------------
MAXPOOL_SHAPES = ((1, 1, 1), (3, 2, 2), (4, 1, 9), (5, 9, 1), (64, 37, 53), (7, 8, 8))


def maxpool_input(C, H, W, B, seed=0):
    """[B, H, W, C] f32 with NaN, +Inf and -Inf at a corner, on an edge and in the interior; which of the three sits
    where rotates with the channel and the image, so every position sees every value."""
    rng = np.random.default_rng([seed, C, H, W, B])
    x = rng.standard_normal((B, H, W, C)).astype(F)
    spots = [(0, 0), (H - 1, W - 1), (0, W // 2), (H // 2, 0), (H // 2, W // 2), (H // 2, max(W // 2 - 1, 0))]
    vals = [np.nan, np.inf, -np.inf]
    for b in range(B):
        for c in range(C):
            for i, (y, xx) in enumerate(spots):
                if (i + c) % 2 == 0 or H * W == 1:  # leave some windows of every channel ordinary
                    x[b, y, xx, c] = vals[(i + c + b) % 3]
    if H > 2 and W > 2:  # a window of nothing but -Inf (its result is -Inf, not the padding's)
        x[:, :2, :2, 0] = -np.inf
    return x


# ---- sums ------------------------------------------------------------------------------------------------------
MEAN_CHANNELS = (1, 5, 64, 65, 300)
MEAN_PIXELS = (1, 7, 31, 32, 33, 129, 4800)
# (c_in, c_out, npix_in, npix_out, members, bias, gate, act); bias: 'all' / 'none' / 'some' members
POOL_FC_CASES = ((64, 24, 300, 300, 1, 'all', True, 'relu'),
                 (100, 5, 1, 1, 3, 'some', False, 'none'),
                 (576, 256, 1200, 1200, 2, 'none', True, 'relu'),
                 (576, 40, 1209, 130, 1, 'all', False, 'relu'),
                 (1024, 256, 300, 4800, 2, 'all', True, 'none'),
                 (2048, 256, 300, 300, 8, 'some', True, 'relu'),
                 (8, 16, 37, 9216, 1, 'none', True, 'relu'))


def positive(shape, seed):
    """f32 in [0.5, 1.5]: a dropped or doubled pixel moves a mean of npix of them by >= 0.5 / npix."""
    return np.random.default_rng(seed).uniform(0.5, 1.5, shape).astype(F)


def pool_fc_inputs(case):
    """Per member: x [npix_in, c_in] in [0.5, 1.5], signed W [c_out, c_in] and bias [c_out] (or None), gate [npix_out, c_out]
    in [0.5, 1.5] (or None)."""
    cin, cout, pin, pout, n, bias, gate, _ = case
    rng = np.random.default_rng([cin, cout, pin, pout, n])
    members = []
    for i in range(n):
        x = rng.uniform(0.5, 1.5, (pin, cin)).astype(F)
        w = (rng.standard_normal((cout, cin)) / np.sqrt(cin)).astype(F)
        has_b = bias == 'all' or (bias == 'some' and i % 2 == 1)
        b = (rng.standard_normal(cout) * 0.3).astype(F) if has_b else None
        g = rng.uniform(0.5, 1.5, (pout, cout)).astype(F) if gate else None
        members.append((x, w, b, g))
    return members


def pack_image(h, w, seed=0):
    """[3, h, w] f32 image values with negatives and a NaN, and an [h, w] depth plane."""
    rng = np.random.default_rng([seed, h, w])
    img = (rng.standard_normal((3, h, w)) * 60 + 100).astype(F)
    depth = (rng.random((h, w)) * 4).astype(F)
    img[1, h // 2, w // 2] = np.nan
    img[2, 0, 0] = -255.0
    depth[h - 1, w - 1] = np.nan
    depth[0, 0] = -1.5
    return img, depth


# ---- volumes ---------------------------------------------------------------------------------------------------
GRID_THREADS = 2048 * 256  # threads of the largest streaming grid: beyond it the kernels grid-stride
FILL_SIZES = (1, 3, 7, 8, 9, 819, GRID_THREADS * 8 + 8 * 3 + 5)
FILL_VALUES = (0.1, -0.0, 65504.0)
FILTER_THRESHOLDS = (2.0, 0.1, 2.3)
STREAM_SIZES = (819, GRID_THREADS + 777)


def filter_volume(n, thr, seed=0):
    """fp16 (tsdf, weights) [n]: weights in [0, 4] with float16(thr), its two fp16 neighbours, 0, -1, NaN and +Inf planted
    at the front and, where n allows, in the part of the volume that the grid-stride loop's second pass covers."""
    rng = np.random.default_rng([seed, n, int(thr * 1000)])
    tsdf = rng.uniform(-0.1, 0.1, n).astype(H16)
    w = (rng.random(n) * 4).astype(H16)
    t = H16(thr)
    plant = np.array([t, np.nextafter(t, H16(-np.inf)), np.nextafter(t, H16(np.inf)), 0, -1, np.nan, np.inf, t], H16)
    for start in (5, n // 2, GRID_THREADS + 100):
        if start + len(plant) <= n:
            w[start:start + len(plant)] = plant
    return tsdf, w


def evaluate_volume(n, seed=0):
    """fp16 (est, gt, weights) [n]: est / gt around the +-0.04 clip with NaN, +-Inf, -0.0, +-0.04 (as fp16 rounds it), the
    fp16 values on either side of the clip and sign disagreements planted against each other; weights 0, negative, NaN and
    positive."""
    rng = np.random.default_rng([seed, n])
    est = rng.uniform(-0.06, 0.06, n).astype(H16)
    gt = rng.uniform(-0.06, 0.06, n).astype(H16)
    w = np.where(rng.random(n) < 0.6, rng.random(n) * 5, 0).astype(H16)
    c = H16(0.04)
    edge = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, c, -c, np.nextafter(c, H16(1)), np.nextafter(c, H16(0)),
                     np.nextafter(-c, H16(-1)), np.nextafter(-c, H16(0)), 0.02, -0.02, 6.1e-5, -6e-8], H16)
    k = len(edge)
    if n >= k * k + 8:
        for start in (0, GRID_THREADS + 8):
            if start + k * k <= n:
                est[start:start + k * k] = np.repeat(edge, k)  # every edge value of est against every one of gt
                gt[start:start + k * k] = np.tile(edge, k)
                w[start:start + k * k] = H16(1.5)
        w[k * k:k * k + 8] = np.array([0, -0.0, -2, np.nan, np.inf, 6e-8, -np.inf, 3], H16)
    elif n == 1:
        est[0], gt[0], w[0] = H16(-0.02), H16(0.03), H16(1)
    return est, gt, w


def confusion_volume(n, C, spill, seed=0):
    """u8 (est, gt) and fp16 weights [n].  ``spill``: labels in [C, 256) in gt (the pair is in no cell), in est under a small
    gt (the flat index gt * C + est lands in a later row) and in est under gt = C - 1 (the index reaches C * C: dropped)."""
    rng = np.random.default_rng([seed, n, C])
    hi = min(C, 255)
    est = rng.integers(0, hi, n).astype(np.uint8)
    gt = np.where(rng.random(n) < 0.7, est, rng.integers(0, hi, n)).astype(np.uint8)
    w = np.where(rng.random(n) < 0.4, rng.random(n) * 5, 0).astype(H16)
    if spill:
        assert C < 256
        big = rng.integers(C, 256, n).astype(np.uint8)
        pick = rng.random(n)
        g_big = pick < 0.05
        gt[g_big] = big[g_big]
        e_big = (pick > 0.9) & (gt.astype(np.int64) * C + big < C * C)
        est[e_big] = big[e_big]
        both = pick > 0.97
        gt[both] = big[both]
        est[both] = big[::-1][both]
        over = (pick > 0.5) & (pick < 0.52)
        gt[over] = C - 1
        est[over] = big[over]
    return est, gt, w
