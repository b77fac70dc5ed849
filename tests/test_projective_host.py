"""CPU: the projective TSDF fusion definition (projective_ref.py, the numpy restatement of csrc/ojf_projective.hip) on
analytic cases, the refusals of ojf_fuse_projective without a device, and the coverage of the GPU parity cases."""
import numpy as np
import pytest

from online_joint_depthfusion_and_semantic_amd import _lib
import projective_ref as ref

# A fronto-parallel plane seen by an axis-aligned camera, in numbers fp16 holds exactly: 8x8x16 voxels of 1/8 m, camera at
# (0, 0, -0.9375) looking along +z, so that voxel (i,j,k) has camera depth zc = 1 + k/8; 64x64 pixels, f = 64: every voxel
# projects inside the image.
SHAPE, RES, TRUNC, INIT = (8, 8, 16), 0.125, 0.25, 0.5
ORIGIN = np.array([-0.5, -0.5, 0.0])
E0 = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, -0.9375]])
K0 = np.array([[64.0, 0.0, 31.5], [0.0, 64.0, 31.5], [0.0, 0.0, 1.0]])
ZC = 1.0 + np.arange(16) / 8.0


def _fresh():
    return np.full(SHAPE, INIT, np.float16), np.zeros(SHAPE, np.float16)


def _plane(d):
    return np.full((64, 64), d, np.float32)


def _rows(vol):
    """The volume as one value per k (asserting that every (i,j) column agrees)."""
    v = vol.astype(np.float32)
    assert (v == v[0, 0]).all()
    return v[0, 0]


def test_one_and_two_views_of_a_plane():
    t, w = _fresh()
    n = ref.fuse(t, w, ORIGIN, RES, _plane(1.5), K0, E0, trunc=TRUNC)
    s1 = 1.5 - ZC  # 0.5 - k/8: in the band for k = 2 (s = trunc) .. 6 (s = -trunc, still updated)
    band1 = (s1 >= -TRUNC) & (s1 <= TRUNC)
    assert list(np.flatnonzero(band1)) == [2, 3, 4, 5, 6] and n == [64 * 5]
    assert np.array_equal(_rows(t), np.where(band1, s1, INIT)) and np.array_equal(_rows(w), band1.astype(np.float32))
    ref.fuse(t, w, ORIGIN, RES, _plane(1.25), K0, E0, trunc=TRUNC)
    s2 = 1.25 - ZC  # band: k = 0 .. 4
    band2 = (s2 >= -TRUNC) & (s2 <= TRUNC)
    want = np.where(band1 & band2, (s1 + s2) / 2, np.where(band1, s1, np.where(band2, s2, INIT)))
    assert np.array_equal(_rows(t), want)
    assert np.array_equal(_rows(w), band1.astype(np.float32) + band2)
    # both views in one call: the same bits
    t2, w2 = _fresh()
    ref.fuse(t2, w2, ORIGIN, RES, np.stack([_plane(1.5), _plane(1.25)]), K0, E0, trunc=TRUNC)
    assert np.array_equal(t2.view(np.uint16), t.view(np.uint16)) and np.array_equal(w2.view(np.uint16), w.view(np.uint16))


def test_carve_pulls_free_space_to_the_truncation():
    t, w = _fresh()
    ref.fuse(t, w, ORIGIN, RES, _plane(1.5), K0, E0, trunc=TRUNC, carve=True)
    s1 = 1.5 - ZC
    seen = s1 >= -TRUNC  # k = 0, 1 lie in front of the band
    assert np.array_equal(_rows(t), np.where(seen, np.minimum(s1, TRUNC), INIT))
    assert np.array_equal(_rows(w), seen.astype(np.float32))
    off_t, off_w = _fresh()
    ref.fuse(off_t, off_w, ORIGIN, RES, _plane(1.5), K0, E0, trunc=TRUNC, carve=False)
    differ = _rows(w) != _rows(off_w)
    assert list(np.flatnonzero(differ)) == [0, 1]


def test_weight_clamps_and_value_still_averages():
    t, w = _fresh()
    ref.fuse(t, w, ORIGIN, RES, np.stack([_plane(1.5), _plane(1.5), _plane(1.25)]), K0, E0, trunc=TRUNC, max_weight=2.0)
    k = 3  # s = 0.125, 0.125, -0.125
    assert _rows(w)[k] == 2.0
    want = np.float16((np.float32(2.0) * np.float32(0.125) + np.float32(-0.125)) / np.float32(3.0))
    assert _rows(t)[k] == np.float32(want) and want != np.float16(0.125)


def test_near_and_depth_validity():
    t, w = _fresh()
    d = _plane(1.5)
    d[:, :32] = np.nan
    d[:16, 32:] = -1.0
    d[16:32, 32:] = np.inf
    mask = np.ones((64, 64), bool)
    mask[32:48, 32:] = False
    ref.fuse(t, w, ORIGIN, RES, d, K0, E0, mask=mask, trunc=TRUNC, near=1.5)
    touched = w.astype(np.float32) > 0
    # near = 1.5 leaves k <= 4 alone (zc > near is strict); only rows 48.., columns 32.. carry a depth
    assert not touched[:, :, :5].any() and touched[:, :, 5:7].any()
    x = ORIGIN[0] + (np.arange(8) + 0.5) * RES
    for i in range(8):
        for j in range(8):
            c = np.floor(64 * x[i] / ZC[5] + 31.5 + 0.5)
            r = np.floor(64 * x[j] / ZC[5] + 31.5 + 0.5)
            assert touched[i, j, 5] == (c >= 32 and r >= 48)


def test_pixel_ties_go_to_floor():
    # f = 8, cx = 4: voxel i of the k = 0 slab (zc = 1) projects to u = i + 0.5 exactly; u + 0.5 = i + 1 -> column i + 1
    K = np.array([[8.0, 0.0, 4.0], [0.0, 8.0, 3.5], [0.0, 0.0, 1.0]])
    d = np.empty((8, 9), np.float32)
    d[:] = 1.0 + 0.125 * (np.arange(9) % 2)
    t, w = _fresh()
    ref.fuse(t, w, ORIGIN, RES, d, K, E0, trunc=TRUNC)
    got = t.astype(np.float32)[:, :, 0]
    for i in range(8):
        assert (got[i] == 0.125 * ((i + 1) % 2)).all()


def test_semantic_rule():
    def run(label_scores):
        t, w = _fresh()
        ids, sc = np.zeros(SHAPE, np.uint8), np.zeros(SHAPE, np.float16)
        labels = np.stack([np.full((64, 64), l, np.uint8) for l in (3, 5, 7)])
        ref.fuse(t, w, ORIGIN, RES, np.stack([_plane(1.5)] * 3), K0, E0, ids=ids, scores=sc, labels=labels,
                 label_scores=label_scores, trunc=TRUNC, carve=True)
        return ids, sc
    ls = np.stack([np.full((64, 64), v, np.float32) for v in (0.5, 0.75, 0.75)])
    ids, sc = run(ls)
    # the higher score replaces the label, the equal one does not; only the band (k = 2..6) takes labels, carved voxels none
    assert (ids[:, :, 2:7] == 5).all() and (sc[:, :, 2:7] == np.float16(0.75)).all()
    assert (ids[:, :, :2] == 0).all() and (ids[:, :, 7:] == 0).all() and (sc[:, :, :2] == 0).all()
    ids, sc = run(None)  # every label scores 1: the first stays
    assert (ids[:, :, 2:7] == 3).all() and (sc[:, :, 2:7] == np.float16(1.0)).all()


def test_reference_refuses_a_non_pinhole_matrix():
    bad = K0.copy()
    bad[0, 1] = 0.5
    with pytest.raises(ValueError):
        ref.fuse(*_fresh(), ORIGIN, RES, _plane(1.5), bad, E0, trunc=TRUNC)


# ---- ojf_fuse_projective refuses bad arguments before any HIP call -----------------------------------------------------
class _Args:
    """A complete, valid argument list with fake (never dereferenced) device pointers; keyword overrides replace entries."""

    def __init__(self):
        self.origin = np.zeros(3)
        self.K = np.ascontiguousarray(np.stack([K0.reshape(9)] * 2))
        self.E = np.ascontiguousarray(np.stack([E0.reshape(12)] * 2))
        self.p = 0x1000

    def call(self, **kw):
        a = dict(tsdf=self.p, wgt=self.p, ids=None, scores=None, X=8, Y=8, Z=8, origin=self.origin.ctypes.data, res=0.1, n=2,
                 K=self.K.ctypes.data, E=self.E.ctypes.data, depth=self.p, mask=None, labels=None, lscores=None, h=4, w=4,
                 trunc=0.1, max_weight=128.0, near=0.0, carve=0)
        a.update(kw)
        lib = _lib.load()
        rc = lib.ojf_fuse_projective(a['tsdf'], a['wgt'], a['ids'], a['scores'], a['X'], a['Y'], a['Z'], a['origin'], a['res'],
                                     a['n'], a['K'], a['E'], a['depth'], a['mask'], a['labels'], a['lscores'], a['h'], a['w'],
                                     a['trunc'], a['max_weight'], a['near'], a['carve'], None)
        return rc, lib.ojf_last_error().decode()


def _refused(result, word):
    rc, msg = result
    assert rc != 0 and word in msg, (rc, msg)


def test_fuse_projective_refuses_bad_arguments_without_a_device():
    a = _Args()
    for key in ('tsdf', 'wgt', 'origin', 'K', 'E', 'depth'):
        _refused(a.call(**{key: None}), 'null')
    _refused(a.call(ids=a.p), 'all given or all null')
    _refused(a.call(ids=a.p, scores=a.p), 'all given or all null')
    _refused(a.call(labels=a.p), 'all given or all null')
    _refused(a.call(lscores=a.p), 'labels_dev')
    _refused(a.call(n=0), 'views')
    _refused(a.call(n=_lib.PROJECTIVE_MAX_VIEWS + 1), 'views')
    for key in ('X', 'Y', 'Z'):
        _refused(a.call(**{key: 0}), 'volume size')
    _refused(a.call(X=2048, Y=2048, Z=2048), 'too large')
    _refused(a.call(h=0), 'image size')
    _refused(a.call(w=-3), 'image size')
    for v in (0.0, -0.1, float('inf'), float('nan')):
        _refused(a.call(trunc=v), 'trunc')
    for v in (0.5, 4096.0, float('nan')):
        _refused(a.call(max_weight=v), 'max_weight')
    for v in (-0.01, float('nan'), float('inf')):
        _refused(a.call(near=v), 'near')
    for v in (-1, 2):
        _refused(a.call(carve=v), 'carve')
    for idx, v in ((1, 0.1), (3, 1e-3), (6, 1.0), (7, -2.0), (8, 2.0)):
        bad = _Args()
        bad.K[1, idx] = v  # (the second view's matrix: every view is checked)
        _refused(bad.call(), 'pinhole')
    for name, idx in (('K', 4), ('E', 7), ('origin', 2)):
        for v in (float('nan'), float('inf')):
            bad = _Args()
            getattr(bad, name).reshape(-1)[idx] = v
            _refused(bad.call(), 'non-finite')
    _refused(a.call(res=float('nan')), 'non-finite')
    _refused(a.call(res=float('inf')), 'non-finite')
    _refused(a.call(res=0.0), 'resolution')
    _refused(a.call(res=-0.1), 'resolution')


# ---- the GPU parity cases are not vacuous ------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', ref.SHAPES)
@pytest.mark.parametrize('pose', ref.POSES)
def test_gpu_cases_update_voxels(shape, pose):
    for carve in (False, True):
        c = ref.tiny_case(shape, pose)
        n = ref.fuse(c['tsdf'], c['weights'], c['origin'], c['res'], c['depth'], c['K'], c['E'], c['mask'], c['ids'], c['scores'],
                     c['labels'], c['label_scores'], trunc=c['trunc'], max_weight=c['max_weight'], carve=carve)[0]
        if pose == 'looking_away':
            assert n == 0
        else:
            assert n >= 25, n
