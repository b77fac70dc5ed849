"""CPU: the colour volume's definition (color_ref.py, the numpy restatement of csrc/ojf_color.hip) - the coverage of the GPU
parity cases, the refusals of ojf_fuse_color / ojf_color_sample / ojf_color_render without a device, the sampler on analytic
volumes, and the quality of the definition on the synthetic room."""
import numpy as np
import pytest

from online_joint_depthfusion_and_semantic_amd import _lib, synthetic
import color_ref as ref


# ---- the GPU parity cases are not vacuous ------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', ref.SHAPES)
@pytest.mark.parametrize('pose', ref.POSES)
def test_gpu_cases_update_voxels(shape, pose):
    for masked in (False, True):
        c = ref.tiny_color_case(shape, pose)
        before = c['colors'].copy()
        n = ref.fuse(c['colors'], c['origin'], c['res'], c['image'], c['depth'], c['K'], c['E'], c['mask'] if masked else None,
                     band=c['band'], max_weight=c['color_max_weight'])[0]
        changed = int((before.view(np.uint16) != c['colors'].view(np.uint16)).any(axis=-1).sum())
        if pose == 'looking_away':
            assert n == 0 and changed == 0
        else:
            assert n >= 20 and 0 < changed <= n, (n, changed)


def test_views_in_one_call_are_calls_of_one_view():
    cases = [ref.tiny_color_case((16, 16, 16), p) for p in ref.POSES]
    a, b = cases[0]['colors'].copy(), cases[0]['colors'].copy()
    o, res = cases[0]['origin'], cases[0]['res']
    ref.fuse(a, o, res, np.stack([c['image'] for c in cases]), np.stack([c['depth'] for c in cases]), cases[0]['K'],
             np.stack([c['E'] for c in cases]), band=ref.BAND, max_weight=ref.MAX_WEIGHT)
    for c in cases:
        ref.fuse(b, o, res, c['image'], c['depth'], c['K'], c['E'], band=ref.BAND, max_weight=ref.MAX_WEIGHT)
    assert np.array_equal(a.view(np.uint16), b.view(np.uint16))
    assert a[..., 3].max() == ref.MAX_WEIGHT  # the weight saturates, the colour still moves


# ---- the entry points refuse bad arguments before any HIP call ---------------------------------------------------------
K0 = np.array([[4.0, 0.0, 2.0], [0.0, 4.0, 2.0], [0.0, 0.0, 1.0]])
E0 = np.eye(4)[:3]


class _Args:
    """Complete, valid argument lists with fake (never dereferenced) device pointers; keyword overrides replace entries."""

    def __init__(self):
        self.origin = np.zeros(3)
        self.K = np.ascontiguousarray(np.stack([K0.reshape(9)] * 2))
        self.E = np.ascontiguousarray(np.stack([E0.reshape(12)] * 2))
        self.Ki = np.ascontiguousarray(np.stack([np.linalg.inv(K0).reshape(9)] * 2).astype(np.float32))
        self.Ef = self.E.astype(np.float32)
        self.p = 0x1000

    def _call(self, name, order, a, kw):
        a.update(kw)
        lib = _lib.load()
        rc = getattr(lib, name)(*[a[k] for k in order], None)
        return rc, lib.ojf_last_error().decode()

    def fuse(self, **kw):
        a = dict(color=self.p, X=8, Y=8, Z=8, origin=self.origin.ctypes.data, res=0.1, n=2, K=self.K.ctypes.data,
                 E=self.E.ctypes.data, depth=self.p, mask=None, image=self.p, h=4, w=4, band=0.1, max_weight=64.0, near=0.0)
        return self._call('ojf_fuse_color', list(a), a, kw)

    def sample(self, **kw):
        a = dict(color=self.p, X=8, Y=8, Z=8, points=self.p, n=10, rgba=self.p)
        return self._call('ojf_color_sample', list(a), a, kw)

    def render(self, **kw):
        a = dict(color=self.p, X=8, Y=8, Z=8, origin=self.origin.ctypes.data, res=0.1, n=2, Ki=self.Ki.ctypes.data,
                 E=self.Ef.ctypes.data, depth=self.p, h=4, w=4, rgba=self.p)
        return self._call('ojf_color_render', list(a), a, kw)


def _refused(result, prefix, word):
    rc, msg = result
    assert rc != 0 and msg.startswith(prefix + ':') and word in msg, (rc, msg)


def test_fuse_color_refuses_bad_arguments_without_a_device():
    a = _Args()
    who = 'ojf_fuse_color'
    for key in ('color', 'origin', 'K', 'E', 'depth', 'image'):
        _refused(a.fuse(**{key: None}), who, 'null')
    _refused(a.fuse(n=0), who, 'views')
    _refused(a.fuse(n=_lib.COLOR_MAX_VIEWS + 1), who, 'views')
    assert _lib.COLOR_MAX_VIEWS == 32
    for key in ('X', 'Y', 'Z'):
        _refused(a.fuse(**{key: 0}), who, 'volume size')
    _refused(a.fuse(X=2048, Y=2048, Z=2048), who, 'too large')
    _refused(a.fuse(h=0), who, 'image size')
    _refused(a.fuse(w=-3), who, 'image size')
    for v in (0.0, -0.1, float('inf'), float('nan')):
        _refused(a.fuse(band=v), who, 'band')
    for v in (0.0, 0.5, 4096.0, float('nan')):
        _refused(a.fuse(max_weight=v), who, 'max_weight')
    for v in (-0.01, float('nan'), float('inf')):
        _refused(a.fuse(near=v), who, 'near')
    for idx, v in ((1, 0.1), (3, 1e-3), (6, 1.0), (7, -2.0), (8, 2.0)):
        bad = _Args()
        bad.K[1, idx] = v  # (the second view's matrix: every view is checked)
        _refused(bad.fuse(), who, 'pinhole')
    for name, idx in (('K', 4), ('E', 7), ('origin', 2)):
        for v in (float('nan'), float('inf')):
            bad = _Args()
            getattr(bad, name).reshape(-1)[idx] = v
            _refused(bad.fuse(), who, 'non-finite')
    _refused(a.fuse(res=float('nan')), who, 'non-finite')
    _refused(a.fuse(res=0.0), who, 'resolution')
    _refused(a.fuse(image=a.p + 2), who, 'aligned')


def test_color_read_outs_refuse_bad_arguments_without_a_device():
    a = _Args()
    who = 'ojf_color_sample'
    for key in ('color', 'points', 'rgba'):
        _refused(a.sample(**{key: None}), who, 'null')
    _refused(a.sample(n=0), who, 'points')
    _refused(a.sample(n=1 << 31), who, 'points')
    for key in ('X', 'Y', 'Z'):
        _refused(a.sample(**{key: 0}), who, 'volume size')
    _refused(a.sample(X=2048, Y=2048, Z=2048), who, 'too large')
    _refused(a.sample(color=a.p + 1), who, 'aligned')
    who = 'ojf_color_render'
    for key in ('color', 'origin', 'Ki', 'E', 'depth', 'rgba'):
        _refused(a.render(**{key: None}), who, 'null')
    _refused(a.render(n=0), who, 'views')
    _refused(a.render(n=_lib.RENDER_MAX_VIEWS + 1), who, 'views')
    _refused(a.render(Y=-1), who, 'volume size')
    _refused(a.render(h=0), who, 'image size')
    _refused(a.render(res=0.0), who, 'resolution')
    _refused(a.render(res=float('inf')), who, 'non-finite')
    for name, idx in (('Ki', 9), ('Ef', 20), ('origin', 1)):
        bad = _Args()
        getattr(bad, name).reshape(-1)[idx] = float('nan')
        _refused(bad.render(), who, 'non-finite')


# ---- the sampler on volumes whose answer is known ----------------------------------------------------------------------
def test_sampler_returns_a_constant_colour_wherever_a_coloured_corner_exists():
    rng = np.random.default_rng(5)
    shape = (9, 6, 11)
    vol = np.zeros(shape + (4,), np.float16)
    vol[..., :3] = (200.0, 17.0, 96.0)
    w = rng.integers(1, 9, shape).astype(np.float16)
    w[rng.random(shape) < 0.5] = 0
    vol[..., 3] = w
    vol[w == 0] = 0
    N = np.array(shape, np.float64)
    g = rng.uniform(-1.5, N + 0.5, (4000, 3)).astype(np.float32)
    got = ref.sample(vol, g)
    # a coloured corner: inside the grid, W > 0 and a non-zero trilinear weight (an integer coordinate has weight 0 on its upper corner)
    i0 = np.floor(g).astype(np.int64)
    f = g - np.floor(g)
    in_range = ((g >= -1) & (g <= N.astype(np.float32))).all(axis=1)
    any_corner = np.zeros(len(g), bool)
    for c in range(8):
        bits = np.array([(c >> 2) & 1, (c >> 1) & 1, c & 1])
        idx = i0 + bits
        inside = ((idx >= 0) & (idx < np.array(shape))).all(axis=1)
        tw = np.where(bits, f, 1 - f).prod(axis=1)
        cl = np.clip(idx, 0, np.array(shape) - 1)
        any_corner |= in_range & inside & (w[cl[:, 0], cl[:, 1], cl[:, 2]] > 0) & (tw > 0)
    assert 0.5 < any_corner.mean() < 0.99
    assert (got[any_corner] == (200, 17, 96, 255)).all()
    assert not got[~any_corner].any()


def test_sampler_reproduces_a_linear_colour():
    shape = (12, 10, 14)
    i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing='ij')
    vol = np.ones(shape + (4,), np.float16)
    lin = [(10.0, 3.0, 5.0, 2.0), (240.0, -4.0, -6.0, -3.0), (20.0, 8.0, 0.5, 7.0)]  # (multiples of 1/2: exact in fp16 below 1024)
    for ch, (a0, a1, a2, a3) in enumerate(lin):
        vol[..., ch] = a0 + a1 * i + a2 * j + a3 * k
        assert np.array_equal(vol[..., ch].astype(np.float64), a0 + a1 * i + a2 * j + a3 * k)
    rng = np.random.default_rng(6)
    g = rng.uniform(0.0, np.array(shape) - 1.0, (4000, 3)).astype(np.float32)
    got = ref.sample(vol, g).astype(np.float64)
    want = np.stack([a0 + a1 * g[:, 0] + a2 * g[:, 1] + a3 * g[:, 2] for a0, a1, a2, a3 in lin], axis=1)
    assert (got[:, 3] == 255).all()
    assert np.abs(got[:, :3] - np.clip(want, 0, 255)).max() <= 1.0


# ---- quality of the definition on the synthetic room -------------------------------------------------------------------
ROOM_MEAN, ROOM_P99 = 1.468, 10.472  # measured once with this reference (levels of 0..255); see the docstring below


def test_fused_colour_of_the_synthetic_room_matches_the_analytic_colour():
    """20 frames of synthetic.SyntheticStream(48, 64, 64, 20) - depth_gt, mask, poses - with images of a smooth analytic
    colour of the world-space surface point (color_ref.analytic_color: sinusoids of wavelength >= 16 voxels inside 30..225),
    fused by color_ref.fuse with band = 0.24 m (3 voxels) and max_weight 64.  The colour sampled at the zero crossings of the
    ground-truth TSDF along the grid axes between two coloured voxels is compared with the analytic colour there.
    Measured with this reference: mean absolute error 1.468 levels, 99th percentile 10.472 levels over 5744 crossing points, all of
    them coloured (the tail sits at the furniture's edges, where the band of one surface reaches voxels next to another).  The assertion is 1.5x those values; the margin covers nothing but a change of the case."""
    h, w, grid, frames, band = 48, 64, 64, 20, 0.24
    st = synthetic.SyntheticStream(h, w, grid, frames)
    origin, res, _ = synthetic.grid_spec(grid)
    vol = np.zeros((grid,) * 3 + (4,), np.float16)
    for f in ref.room_frames(st, frames):
        ref.fuse(vol, origin, res, f['image'], f['depth_gt'], f['intrinsics'], f['extrinsics'], f['mask'], band=band)
    gt, _ = synthetic.gt_volumes(grid, band)
    t = gt.astype(np.float64)
    coloured = vol[..., 3] > 0
    pts = []
    for axis in range(3):
        n = grid - 1
        a, b = np.take(t, range(n), axis), np.take(t, range(1, n + 1), axis)
        cross = np.take(coloured, range(n), axis) & np.take(coloured, range(1, n + 1), axis) & ((a < 0) != (b < 0))
        idx = np.argwhere(cross).astype(np.float64)
        idx[:, axis] += a[cross] / (a[cross] - b[cross])
        pts.append(idx)
    g = np.concatenate(pts)
    assert len(g) > 5000
    got = ref.sample(vol, g.astype(np.float32))
    have = got[:, 3] == 255
    want = ref.analytic_color(origin + (g + 0.5) * res)
    err = np.abs(got[have, :3].astype(np.float64) - want[have])
    mean, p99 = err.mean(), np.percentile(err, 99)
    print('room colour: {} crossings, {:.4f} coloured, mean |err| {:.3f}, p99 {:.3f}'.format(len(g), have.mean(), mean, p99))
    assert have.mean() >= 0.90
    assert mean <= 1.5 * ROOM_MEAN and p99 <= 1.5 * ROOM_P99, (mean, p99)
