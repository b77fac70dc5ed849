"""-m gpu: the resample operator (ojf_resample_volumes / ojf_resample_records, resample.resample_scene, Database.resample /
recentre / merge) against its numpy restatement (resample_ref.py) bit for bit over the whole tensors, and against plain torch
indexing where the definition makes it an exact copy."""
import numpy as np
import pytest
import torch

from online_joint_depthfusion_and_semantic_amd import _lib, resample, synthetic
from online_joint_depthfusion_and_semantic_amd.config import default_config, database_config
from online_joint_depthfusion_and_semantic_amd.database import Database, Voxelgrid
from online_joint_depthfusion_and_semantic_amd.label_probs import record_size
import resample_ref as ref
from test_resample_host import shifted_copy, plane_case, plane_check

pytestmark = pytest.mark.gpu

H = np.float16
SRC, RES = (11, 15, 21), 0.05
O_S = np.array([-0.4, 0.3, 1.1])
SHIFT = (3, -2, 5)
QUARTER = np.array([[0.0, 1, 0, 0], [-1.0, 0, 0, 0], [0, 0, 1.0, 0]])  # about z; the translation goes on per case


def _dev(a, cuda, off=0):
    """A device copy of ``a``; off > 0: at a pointer ``off`` elements past a 256-byte boundary."""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not off:
        return t.to(cuda)
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=cuda)
    out = buf[off:].view(t.shape)
    out.copy_(t)
    return out


def _bits(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return a.view(np.uint16) if a.dtype == H else a


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    n_bad = int((g != w).sum())
    assert n_bad == 0, '{}: {} of {} values differ'.format(what, n_bad, g.size)


def shift_box(shift=SHIFT, res=RES):
    return dict(src_origin=O_S, src_resolution=res, dst_origin=O_S + res * np.array(shift, np.float64), dst_resolution=res)


def quarter_box():
    T = QUARTER.copy()
    T[:, 3] = O_S - QUARTER[:, :3] @ O_S + np.array([0.0, 15 * RES, 0.0])  # destination (i,j,k) reads source (j, 14 - i, k)
    return dict(src_origin=O_S, src_resolution=RES, dst_origin=O_S, dst_resolution=RES, transform=T)


def skew_box(src_shape=SRC):
    T = ref.about_centre(ref.rotation(ref.SKEW_AXIS, np.deg2rad(17.0)), O_S, RES, src_shape, shift=(0.01, -0.02, 0.015))
    return dict(src_origin=O_S, src_resolution=RES, dst_origin=O_S + np.array([-0.03, 0.05, 0.02]), dst_resolution=0.8 * RES, transform=T)


def run_scene(cuda, src, box, dst_shape, into=None, max_weight=None, off=0):
    """(device result, restatement) of one resample_scene call on the numpy scene ``src`` (records under 'colors' /
    'label_probs' with 'n_classes')."""
    M, c = resample.compose(**box)
    dsrc = {k: (v if k == 'n_classes' else _dev(v, cuda, off if k != 'label_probs' else 0)) for k, v in src.items()}
    dinto = None if into is None else {k: (v if k == 'n_classes' else _dev(v, cuda, off if k != 'label_probs' else 0))
                                       for k, v in into.items()}
    got = resample.resample_scene(dsrc, dst_shape=dst_shape, into=dinto, init_value=ref.INIT, max_weight=max_weight, **box)
    want = {}
    geo_max, rec_max = (65504.0, 64.0) if max_weight is None else (max_weight, max_weight)
    if 'tsdf' in src:
        geo = {k: src[k] for k in ('tsdf', 'weights', 'ids', 'scores') if k in src}
        gin = None if into is None else {k: into[k].copy() for k in geo}
        want.update(ref.resample_volumes(geo, M, c, dst_shape, init_value=ref.INIT, into=gin, max_weight=geo_max))
    for key, Cw in (('colors', 3), ('label_probs', src.get('n_classes'))):
        if key in src:
            want[key] = ref.resample_records(src[key], Cw, M, c, dst_shape, into=None if into is None else into[key].copy(), max_weight=rec_max)
    for k, v in dsrc.items():  # the source is read only
        if k != 'n_classes':
            _same(v, src[k], 'source ' + k)
    return got, want


def check(got, want, what):
    assert set(want) == set(got) - {'n_classes'}
    for k in want:
        _same(got[k], want[k], '{}: {}'.format(what, k))


# ---- 1. shape edges ------------------------------------------------------------------------------------------------------------
def test_whole_voxel_shift_against_the_restatement_and_torch_slicing(cuda):
    s = ref.random_scene(SRC)
    got, want = run_scene(cuda, s, shift_box(), (13, 9, 37))
    check(got, want, 'shift')
    obs = s['weights'] > 0
    for key, fill in (('tsdf', H(ref.INIT)), ('weights', 0), ('ids', 0), ('scores', 0)):
        _same(got[key], shifted_copy(s[key], obs, SHIFT, (13, 9, 37), fill), 'slicing: ' + key)
    # the same on the device: the overlap of the two boxes, sliced by torch
    t, w = _dev(s['tsdf'], cuda), _dev(s['weights'], cuda)
    inner = got['tsdf'][0:8, 2:9, 0:16]  # destination p reads source p + (3, -2, 5)
    assert torch.equal(inner.view(torch.int16), torch.where(w[3:11, 0:7, 5:21] > 0, t[3:11, 0:7, 5:21],
                                                            torch.full_like(inner, ref.INIT)).view(torch.int16))


def test_quarter_turn_against_the_restatement_and_rot90(cuda):
    s = ref.random_scene(SRC)
    got, want = run_scene(cuda, s, quarter_box(), (15, 11, 21))
    check(got, want, 'quarter turn')
    full = ref.random_scene(SRC, unobserved=0.0)
    got, _ = run_scene(cuda, full, quarter_box(), (15, 11, 21))
    for key in ('tsdf', 'weights', 'ids', 'scores'):
        assert torch.equal(got[key], torch.rot90(_dev(full[key], cuda), 1, (0, 1))), key


def test_skew_rotation_with_a_finer_destination(cuda):
    s = ref.random_scene(SRC)
    got, want = run_scene(cuda, s, skew_box(), (13, 9, 37))
    assert 0.1 < (want['weights'] > 0).mean() < 0.9
    check(got, want, '17 degrees, res x 0.8')


@pytest.mark.parametrize('dst_shape', [(1, 1, 1), (2, 3, 5), (4, 4, 64), (4, 4, 65), (5, 6, 67)])
def test_destination_shapes(cuda, dst_shape):
    """z-run tails (64, 65, 67) and brick edges on every axis, under the axis-aligned map (z-runs) and the rotation (bricks);
    (5, 6, 67) also from pointers 2 bytes past a 256-byte boundary."""
    s = ref.random_scene(SRC)
    s['colors'] = ref.random_records(SRC, 4, 3)
    for name, box in (('shift', shift_box((1, 2, 3))), ('skew', skew_box())):
        for off in (0, 1) if dst_shape == (5, 6, 67) else (0,):
            got, want = run_scene(cuda, s, box, dst_shape, off=off)
            check(got, want, '{} {} off {}'.format(name, dst_shape, off))
            into = ref.random_scene(dst_shape, seed=3)
            into['colors'] = ref.random_records(dst_shape, 4, 3, seed=3)
            got, want = run_scene(cuda, s, box, dst_shape, into=into, off=off)
            check(got, want, 'merge {} {} off {}'.format(name, dst_shape, off))


# ---- 2. thresholds and ties ----------------------------------------------------------------------------------------------------
def test_half_voxel_offsets(cuda):
    shape, res = (6, 6, 6), 0.5
    s = ref.random_scene(shape, unobserved=0.0)
    s['weights'][:, :, 1::2] = 0
    s['colors'] = ref.random_records(shape, 4, 3, unobserved=0.0)
    s['colors'][:, :, 1::2, 3] = 0
    s['colors'][:, :, 1::2, :3] = 0
    for axes in ((2,), (1, 2), (0, 1, 2)):
        off = np.zeros(3)
        off[list(axes)] = 0.5 * res
        got, want = run_scene(cuda, s, dict(src_origin=np.zeros(3), src_resolution=res, dst_origin=off, dst_resolution=res), shape)
        inner = tuple(slice(0, 5) if a in axes else slice(None) for a in range(3))
        assert (want['weights'][inner] > 0).all() and (want['colors'][inner][..., 3] > 0).all()  # ws == 0.5: covered
        check(got, want, 'half a voxel on {}'.format(axes))


def test_index_range_edges_and_a_destination_outside(cuda):
    s = ref.random_scene((4, 4, 8), unobserved=0.0)
    res = 0.25
    box = dict(src_origin=np.zeros(3), src_resolution=res, dst_origin=np.array([-res, -res, -res]), dst_resolution=res)
    got, want = run_scene(cuda, s, box, (6, 6, 10))  # g = -1 .. N on every axis
    check(got, want, 'g on -1, 0, N - 1, N')
    assert np.array_equal(_bits(got['tsdf'])[1:5, 1:5, 1:9], _bits(s['tsdf']))
    assert not got['weights'][0].any() and not got['weights'][5].any() and not got['weights'][:, :, 9].any()
    box = dict(box, dst_origin=np.array([40.0, 0, 0]))
    got, want = run_scene(cuda, s, box, (3, 3, 3))
    check(got, want, 'outside')
    assert (_bits(got['tsdf']) == _bits(np.array(ref.INIT, H))).all() and not got['weights'].any() and not got['ids'].any() and not got['scores'].any()
    # ... and a merge from there leaves everything alone
    into = ref.random_scene((3, 3, 3), seed=4)
    got, _ = run_scene(cuda, s, box, (3, 3, 3), into=into)
    check(got, into, 'merge from outside')


def test_the_smallest_weight(cuda):
    s = ref.random_scene((4, 4, 8), unobserved=0.0)
    s['weights'][...] = H(2.0 ** -24)
    s['weights'][:, :, 1::2] = 0
    for off in (0.0, 0.25, 0.5):
        box = dict(src_origin=np.zeros(3), src_resolution=0.25, dst_origin=np.array([0.075, 0, off * 0.25]), dst_resolution=0.25)
        got, want = run_scene(cuda, s, box, (3, 4, 7))
        check(got, want, '2^-24 at z offset {}'.format(off))
        assert (_bits(got['weights'])[:, :, 0::2] == 1).all()


# ---- 3. forms ------------------------------------------------------------------------------------------------------------------
def test_ground_truth_form_and_the_form_without_labels(cuda):
    s = ref.random_scene(SRC)
    for box, shape in ((shift_box(), (13, 9, 37)), (skew_box(), (13, 9, 37))):
        for keys in (('tsdf',), ('tsdf', 'ids', 'scores'), ('tsdf', 'weights')):
            got, want = run_scene(cuda, {k: s[k] for k in keys}, box, shape)
            check(got, want, 'form {}'.format(keys))
    gt, _ = run_scene(cuda, {'tsdf': s['tsdf']}, shift_box(), (13, 9, 37))
    _same(gt['tsdf'], shifted_copy(s['tsdf'], np.ones(SRC, bool), SHIFT, (13, 9, 37), H(ref.INIT)), 'every voxel of the overlap')


# ---- 4. records ------------------------------------------------------------------------------------------------------------------
def _records_direct(cuda, src, dst, Cw, M, c, mode, max_weight):
    lib = _lib.load()
    rc = lib.ojf_resample_records(_lib.ptr(src), *src.shape[:3], _lib.ptr(dst), *dst.shape[:3], src.shape[3], Cw, M.ctypes.data, c.ctypes.data,
                                  mode, max_weight, _lib.stream_ptr(cuda))
    _lib.check(rc, 'ojf_resample_records')


@pytest.mark.parametrize('S,Cw', [(4, 3), (8, 5), (8, 7), (32, 30), (264, 256)])
def test_records(cuda, S, Cw):
    """Colour; one chunk with padding and without; 30 classes (4 lanes a voxel, W in the last chunk); 256 classes (33 chunks, W
    alone in the last).  Padding poisoned with a NaN on both sides: it is in no mean and comes back as it went."""
    dst_shape = (13, 9, 37) if S < 264 else (5, 6, 19)
    src = ref.random_records(SRC, S, Cw)
    for name, box in (('shift', shift_box()), ('skew', skew_box())):
        M, c = resample.compose(**box)
        for mode, mw in ((_lib.RESAMPLE_REPLACE, 64.0), (_lib.RESAMPLE_MERGE, 64.0), (_lib.RESAMPLE_MERGE, 6.0)):
            start = ref.random_records(dst_shape, S, Cw, seed=5)
            if mode == _lib.RESAMPLE_REPLACE:
                want = ref.resample_records(src, Cw, M, c, dst_shape)
                want.view(np.uint16)[..., Cw + 1:] = ref.PAD_BITS
            else:
                want = ref.resample_records(src, Cw, M, c, dst_shape, into=start.copy(), max_weight=mw)
            assert not np.isnan(want[..., :Cw + 1]).any()
            dsrc, ddst = _dev(src, cuda), _dev(start, cuda)
            _records_direct(cuda, dsrc, ddst, Cw, M, c, mode, mw)
            _same(ddst, want, '{} S={} mode {} max_weight {}'.format(name, S, mode, mw))
            _same(dsrc, src, 'the source is read only')
            if mode == _lib.RESAMPLE_MERGE and mw == 6.0:
                assert (want[..., Cw] == H(6.0)).any()
    # through the public layer: n_classes gives S and Cw
    if S in (4, 32):
        key = 'colors' if S == 4 else 'label_probs'
        scene = {key: src, 'n_classes': Cw} if S == 32 else {key: src}
        got, want = run_scene(cuda, scene, skew_box(), dst_shape)
        check(got, want, 'resample_scene ' + key)
        assert record_size(30) == 32


def test_record_indexing_is_64_bit(cuda):
    """A zeroed 512^3 x 32 source (8.6 GB, 4.3e9 halves) with records set in its last x-slab; a 4 x 4 x 8 destination at the far
    corner, shifted by whole voxels, is torch indexing of the source."""
    free, _ = torch.cuda.mem_get_info(cuda)
    if free < 24 * 2 ** 30:
        pytest.skip('needs 24 GB of free device memory, {:.1f} GB are free'.format(free / 2 ** 30))
    N, S, Cw = 512, 32, 30
    src = torch.zeros((N, N, N, S), dtype=torch.float16, device=cuda)
    rng = np.random.default_rng(9)
    spots = [(511, 511, 511), (511, 510, 505), (510, 511, 507), (509, 509, 504), (511, 508, 510)]
    for p in spots:
        rec = rng.uniform(0.0, 1.0, S).astype(H)
        rec[Cw] = 3
        src[p] = torch.from_numpy(rec).to(cuda)
    shift = (508, 508, 504)
    got = resample.resample_scene({'label_probs': src, 'n_classes': Cw}, src_origin=np.zeros(3), src_resolution=0.25, dst_shape=(4, 4, 8),
                                  dst_origin=0.25 * np.array(shift, np.float64), dst_resolution=0.25, init_value=ref.INIT)['label_probs']
    want = src[508:512, 508:512, 504:512].clone()
    want[..., Cw + 1:] = 0
    assert int((want[..., Cw] > 0).sum()) == len(spots)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    del src


# ---- 5. merge, aliasing, determinism ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('max_weight', [None, 30.0])
def test_merge_is_replace_into_scratch_then_combine_in_torch(cuda, max_weight):
    dst_shape = (13, 9, 37)
    s, d = ref.random_scene(SRC, seed=1), ref.random_scene(dst_shape, seed=2)
    s['colors'], d['colors'] = ref.random_records(SRC, 4, 3, seed=1), ref.random_records(dst_shape, 4, 3, seed=2)
    box = skew_box()
    got, want = run_scene(cuda, s, box, dst_shape, into=d, max_weight=max_weight)
    check(got, want, 'merge against the restatement')
    scratch, _ = run_scene(cuda, s, box, dst_shape)
    geo_max, rec_max = (65504.0, 64.0) if max_weight is None else (max_weight, max_weight)
    dd = {k: _dev(v, cuda) for k, v in d.items()}
    f = lambda t: t.float()  # noqa: E731
    cov = scratch['weights'].view(torch.int16) != 0
    w0, w1 = f(dd['weights']), f(scratch['weights'])
    mean = ((w0 * f(dd['tsdf']) + w1 * f(scratch['tsdf'])) / (w0 + w1)).half()
    T = torch.where(cov, torch.where(w0 == 0, scratch['tsdf'], mean), dd['tsdf'])
    W = torch.where(cov, torch.clamp(w0 + w1, max=geo_max).half(), dd['weights'])
    beats = cov & (f(scratch['scores']) > f(dd['scores']))
    assert torch.equal(got['tsdf'].view(torch.int16), T.view(torch.int16)) and torch.equal(got['weights'].view(torch.int16), W.view(torch.int16))
    assert torch.equal(got['ids'], torch.where(beats, scratch['ids'], dd['ids']))
    assert torch.equal(got['scores'].view(torch.int16), torch.where(beats, scratch['scores'], dd['scores']).view(torch.int16))
    cc = scratch['colors'][..., 3].view(torch.int16) != 0
    c0, c1 = f(dd['colors'][..., 3]), f(scratch['colors'][..., 3])
    for k in range(3):
        m = ((c0 * f(dd['colors'][..., k]) + c1 * f(scratch['colors'][..., k])) / (c0 + c1)).half()
        ck = torch.where(cc, torch.where(c0 == 0, scratch['colors'][..., k], m), dd['colors'][..., k])
        assert torch.equal(got['colors'][..., k].view(torch.int16), ck.view(torch.int16)), k
    cw = torch.where(cc, torch.clamp(c0 + c1, max=rec_max).half(), dd['colors'][..., 3])
    assert torch.equal(got['colors'][..., 3].view(torch.int16), cw.view(torch.int16))
    reached = bool((got['weights'] == geo_max).any())
    assert reached == (max_weight is not None)


def test_an_aliased_call_is_refused_not_run(cuda):
    s = {k: _dev(v, cuda) for k, v in ref.random_scene((8, 8, 8)).items()}
    before = {k: v.clone() for k, v in s.items()}
    box = dict(src_origin=np.zeros(3), src_resolution=0.1, dst_origin=np.array([0.1, 0, 0]), dst_resolution=0.1)
    with pytest.raises(_lib.OjfError, match='overlap'):
        resample.resample_scene(s, dst_shape=(8, 8, 8), into=s, init_value=ref.INIT, **box)
    other = {k: v.clone() for k, v in s.items()}
    with pytest.raises(_lib.OjfError, match='overlap'):
        resample.resample_scene(s, dst_shape=(8, 8, 8), into=dict(other, weights=s['weights']), init_value=ref.INIT, **box)
    rec = _dev(ref.random_records((8, 8, 8), 4, 3), cuda)
    with pytest.raises(_lib.OjfError, match='overlap'):
        resample.resample_scene({'colors': rec}, dst_shape=(8, 8, 8), into={'colors': rec}, init_value=ref.INIT, **box)
    torch.cuda.synchronize()
    for k in s:
        assert torch.equal(s[k], before[k]), k


def test_two_calls_give_the_same_bits(cuda):
    s = ref.random_scene(SRC)
    s['label_probs'], s['n_classes'] = ref.random_records(SRC, 32, 30), 30
    d = ref.random_scene((13, 9, 37), seed=2)
    d['label_probs'], d['n_classes'] = ref.random_records((13, 9, 37), 32, 30, seed=2), 30
    for into in (None, d):
        a, _ = run_scene(cuda, s, skew_box(), (13, 9, 37), into=into)
        b, _ = run_scene(cuda, s, skew_box(), (13, 9, 37), into=into)
        for k in a:
            if k != 'n_classes':
                _same(a[k], b[k], k)


# ---- 6. linear precision ---------------------------------------------------------------------------------------------------------
def test_plane_within_two_half_ulps(cuda):
    """Half an ulp of fp16 on the inputs and half on the output, each <= 2^-11 max|F|, under a convex combination; the fp32 terms
    are three orders smaller.  Every voxel whose g lies in [0, N-1] on all axes is covered and in the set."""
    src, M, c, d_shape, want, fmax, s_shape = plane_case()
    lib = _lib.load()
    st, sw = _dev(src['tsdf'], cuda), _dev(src['weights'], cuda)
    dt, dw = torch.empty(d_shape, dtype=torch.float16, device=cuda), torch.empty(d_shape, dtype=torch.float16, device=cuda)
    rc = lib.ojf_resample_volumes(_lib.ptr(st), _lib.ptr(sw), None, None, *s_shape, _lib.ptr(dt), _lib.ptr(dw), None, None, *d_shape,
                                  M.ctypes.data, c.ctypes.data, ref.INIT, _lib.RESAMPLE_REPLACE, 65504.0, _lib.stream_ptr(cuda))
    _lib.check(rc, 'ojf_resample_volumes')
    out = {'tsdf': dt.cpu().numpy(), 'weights': dw.cpu().numpy()}
    err, bound = plane_check(out, M, c, d_shape, want, fmax, s_shape)
    print('plane on the device: max error {:.3e}, bound {:.3e}'.format(err, bound))
    assert err <= bound


# ---- 7. Database -------------------------------------------------------------------------------------------------------------------
# 1.92 x 2.56 x 3.2 m around the wall at x = 2.4 the first frames look at, at the 0.08 m of the 64^3 room grid
BOX_SHAPE, BOX_RES, BOX_ORIGIN = (24, 32, 40), 0.08, np.array([0.8, -1.28, -1.6])
FH, FW, FRAMES = 48, 64, 4


class TwoRooms:
    """Two scenes over one 24 x 32 x 40 box: the Database grids have the box's shape, origin and resolution."""

    def __init__(self):
        self.scenes = ['room_0', 'room_1']
        self.stream = synthetic.SyntheticStream(FH, FW, 64, 20)
        self.bbox = np.stack([BOX_ORIGIN, BOX_ORIGIN + np.array(BOX_SHAPE) * BOX_RES], axis=1)

    def get_grid(self, scene, truncation, semantic_grid=True):
        ax = [BOX_ORIGIN[i] + (np.arange(BOX_SHAPE[i]) + 0.5) * BOX_RES for i in range(3)]
        pts = np.stack(np.meshgrid(*ax, indexing='ij'), axis=-1)
        sd = synthetic.scene_sdf(pts)
        g, s = Voxelgrid(BOX_RES), Voxelgrid(BOX_RES)
        g.from_array(np.clip(sd, -truncation, truncation).astype(H), self.bbox)
        s.from_array(np.where(np.abs(sd) < truncation, 1 + (np.floor(pts[..., 0] + 2.4) % 7), 0).astype(np.uint8), self.bbox)
        return (g, s) if semantic_grid else (g,)


def _volumes_of(db, s):
    return {'tsdf': db.scenes_est[s].volume, 'weights': db.fusion_weights[s], 'ids': db.ids_est[s].volume, 'scores': db.scores[s].volume,
            'colors': db.colors.get(s), 'label_probs': db.label_probs.get(s), 'gt': db.scenes_gt[s].volume, 'ids_gt': db.ids_gt[s].volume}


@pytest.fixture
def fused(cuda):
    cfg = default_config(FH, FW, semantics=True, model='tsdf')
    cfg.SETTINGS.device = str(cuda)
    ds = TwoRooms()
    db = Database(ds, database_config(cfg))
    rng = np.random.default_rng(21)
    for i in range(FRAMES):
        f = ds.stream.frame(i)
        args = ('room_0', f['tof_depth'], f['intrinsics'], f['extrinsics'])
        db.integrate_depth(*args, mask=f['mask'], labels=f['semantic_gt'], label_scores=f['semantic_scores'])
        db.integrate_color('room_0', rng.integers(0, 256, (FH, FW, 3)).astype(np.uint8), *args[1:], mask=f['mask'])
        db.integrate_label_probs(*args, mask=f['mask'], labels=f['semantic_gt'])
    snap = {k: v.clone() for k, v in _volumes_of(db, 'room_0').items()}
    f = ds.stream.frame(0)
    snap['render'] = db.render('room_0', f['intrinsics'], f['extrinsics'], (FH, FW))['depth'].clone()
    assert int((snap['weights'] > 0).sum()) > 1000 and int((snap['colors'][..., 3] > 0).sum()) > 200
    assert int((snap['label_probs'][..., 30] > 0).sum()) > 200
    return db, snap


def _moved(snap, shift, observed_by):
    """What a whole-voxel shift of the box leaves of the snapshot: numpy slicing per volume."""
    host = {k: v.cpu().numpy() for k, v in snap.items() if k != 'render'}
    obs = {'est': host['weights'] > 0, 'colors': host['colors'][..., 3] > 0, 'label_probs': host['label_probs'][..., 30] > 0,
           'gt': np.ones(BOX_SHAPE, bool)}
    fills = {'tsdf': ('est', None), 'weights': ('est', 0), 'ids': ('est', 0), 'scores': ('est', 0), 'gt': ('gt', None), 'ids_gt': ('gt', 0)}
    out = {}
    for k, (who, fill) in fills.items():
        out[k] = shifted_copy(host[k], obs[who], shift, BOX_SHAPE, H(observed_by) if fill is None else fill)
    for k in ('colors', 'label_probs'):
        n = 4 if k == 'colors' else 31
        out[k] = np.zeros_like(host[k])
        for ch in range(n):
            out[k][..., ch] = shifted_copy(host[k][..., ch], obs[k], shift, BOX_SHAPE, 0)
    return out


def test_database_recentre_and_back(cuda, fused):
    db, snap = fused
    init = db.initial_value
    centre = BOX_ORIGIN + (np.array(BOX_SHAPE) // 2 + 0.5) * BOX_RES
    shift = db.recentre('room_0', centre + np.array(SHIFT) * BOX_RES)
    assert shift == SHIFT
    new_origin = BOX_ORIGIN + np.array(SHIFT) * BOX_RES
    assert np.allclose(np.asarray(db.origin['room_0']), new_origin, atol=1e-12) and db.resolution['room_0'] == BOX_RES
    for grid in (db.scenes_est['room_0'], db.scenes_gt['room_0'], db.ids_est['room_0'], db.scores['room_0'], db.ids_gt['room_0']):
        assert np.allclose(grid.origin, new_origin, atol=1e-12) and np.allclose(grid.bbox[:, 1], new_origin + np.array(BOX_SHAPE) * BOX_RES)
        assert grid.resolution == BOX_RES and tuple(grid.volume.shape) == BOX_SHAPE
    want = _moved(snap, SHIFT, init)
    for k, v in _volumes_of(db, 'room_0').items():
        _same(v, want[k], 'recentred ' + k)
    assert db.label_probs['room_0'].data_ptr() % 16 == 0
    # the public calls still run on the re-boxed scene
    assert db.state['room_0'] and set(db.evaluate()) >= {'mse', 'iou'}
    f = TwoRooms().stream.frame(0)
    img = db.render('room_0', f['intrinsics'], f['extrinsics'], (FH, FW), semantics=True, color=True)
    both = (img['depth'] > 0) & (snap['render'] > 0)  # the same surface where both boxes hold it
    assert int(both.sum()) > 100 and float((img['depth'] - snap['render'])[both].abs().median()) < 1e-3
    vertices, faces, _, _ = db.get_mesh('room_0')
    assert len(vertices) > 100 and len(faces) > 100
    # ... and back: what stayed inside both boxes has its bits again, the rest is init / 0
    back = db.recentre('room_0', new_origin + (np.array(BOX_SHAPE) // 2 - np.array(SHIFT) + 0.5) * BOX_RES)
    assert back == tuple(-s for s in SHIFT) and np.allclose(np.asarray(db.origin['room_0']), BOX_ORIGIN, atol=1e-12)
    stayed = shifted_copy(np.ones(BOX_SHAPE, bool), np.ones(BOX_SHAPE, bool), SHIFT, BOX_SHAPE, False)  # destination voxels with a source
    stayed = shifted_copy(stayed, stayed, tuple(-s for s in SHIFT), BOX_SHAPE, False)
    assert 0.3 < stayed.mean() < 0.9
    host = {k: v.cpu().numpy() for k, v in snap.items() if k != 'render'}
    empty = {k: np.full(BOX_SHAPE, H(init) if k in ('tsdf', 'gt') else 0, host[k].dtype) for k in host if host[k].ndim == 3}  # init / 0
    for k, v in _volumes_of(db, 'room_0').items():
        got = v.cpu().numpy()
        obs = host['weights'] > 0 if k in ('tsdf', 'weights', 'ids', 'scores') else (np.ones(BOX_SHAPE, bool) if k in ('gt', 'ids_gt') else
                                                                                     host[k][..., 3 if k == 'colors' else 30] > 0)
        keep = stayed & obs
        if got.ndim == 4:
            n = 4 if k == 'colors' else 31
            _same(got[keep][:, :n], host[k][keep][:, :n], 'restored ' + k)
            assert not got[~keep].any(), k
        else:
            _same(got[keep], host[k][keep], 'restored ' + k)
            _same(got[~keep], empty[k][~keep], 'emptied ' + k)
    assert db.recentre('room_0', centre) == (0, 0, 0)


def test_database_merge_into_an_empty_scene(cuda, fused):
    db, snap = fused
    assert 'room_1' not in db.colors and not db.state['room_1']
    src = {k: v.clone() for k, v in _volumes_of(db, 'room_0').items()}
    db.merge('room_1', 'room_0')
    got = _volumes_of(db, 'room_1')
    obs = src['weights'] > 0
    assert int(obs.sum()) > 1000
    for k in ('tsdf', 'weights', 'scores'):
        assert torch.equal(got[k][obs].view(torch.int16), src[k][obs].view(torch.int16)), k
    voted = obs & (src['scores'] > 0)
    assert torch.equal(got['ids'][voted], src['ids'][voted])
    assert (_bits(got['tsdf'][~obs]) == _bits(np.array(db.initial_value, H))).all() and not got['weights'][~obs].any() and not got['ids'][~obs].any()
    for k, cw in (('colors', 3), ('label_probs', 30)):
        o = src[k][..., cw] > 0
        assert int(o.sum()) > 100
        assert torch.equal(got[k][o][:, :cw + 1].view(torch.int16), src[k][o][:, :cw + 1].view(torch.int16)), k
        assert not got[k][~o].any()
    for k, v in _volumes_of(db, 'room_0').items():  # the source is read only
        assert torch.equal(v, src[k]), k
    with pytest.raises(ValueError):
        db.merge('room_0', 'room_0')
    # a second merge of the same scene: the weights add up, the values stay (the mean of two equal values, to an ulp)
    db.merge('room_1', 'room_0', max_weight=65504.0)
    w2 = db.fusion_weights['room_1']
    assert torch.equal(w2[obs], (src['weights'][obs].float() * 2).half())
    assert float((db.scenes_est['room_1'].volume[obs].float() - src['tsdf'][obs].float()).abs().max()) <= 2.0 ** -10 * 0.5


def test_host_resident_scenes_are_refused(cuda, fused):
    db, _ = fused
    db.to_numpy()
    try:
        for call in (lambda: db.resample('room_0', shape=(8, 8, 8)), lambda: db.recentre('room_0', np.zeros(3)),
                     lambda: db.merge('room_1', 'room_0')):
            with pytest.raises(ValueError, match='to_torch'):
                call()
    finally:
        db.to_torch()


def test_database_resample_to_another_resolution(cuda):
    """Database.resample with a shape, a resolution and a transform: the volumes are resample_scene's, the grids follow."""
    cfg = default_config(FH, FW, semantics=True, model='tsdf')
    cfg.SETTINGS.device = str(cuda)
    ds = TwoRooms()
    db = Database(ds, database_config(cfg))
    f = ds.stream.frame(0)
    db.integrate_depth('room_0', f['tof_depth'], f['intrinsics'], f['extrinsics'], mask=f['mask'], labels=f['semantic_gt'],
                       label_scores=f['semantic_scores'])
    src = {k: v.clone() for k, v in _volumes_of(db, 'room_0').items() if v is not None}
    T = ref.about_centre(ref.rotation(ref.SKEW_AXIS, 0.2), BOX_ORIGIN, BOX_RES, BOX_SHAPE)
    new_origin = BOX_ORIGIN + np.array([0.05, 0.03, 0.1])
    db.resample('room_0', origin=new_origin, shape=(12, 17, 21), resolution=0.16, transform=T)
    kw = dict(src_origin=BOX_ORIGIN, src_resolution=BOX_RES, dst_shape=(12, 17, 21), dst_origin=new_origin, dst_resolution=0.16, transform=T,
              init_value=db.initial_value)
    want = resample.resample_scene({k: src[k] for k in ('tsdf', 'weights', 'ids', 'scores')}, **kw)
    want_gt = resample.resample_scene({'tsdf': src['gt'], 'ids': src['ids_gt'], 'scores': torch.zeros_like(src['gt'])}, **kw)
    got = _volumes_of(db, 'room_0')
    for k in ('tsdf', 'weights', 'ids', 'scores'):
        _same(got[k], want[k], k)
    _same(got['gt'], want_gt['tsdf'], 'gt')
    _same(got['ids_gt'], want_gt['ids'], 'ids_gt')
    assert int((got['weights'] > 0).sum()) > 100 and db.resolution['room_0'] == 0.16
    assert np.allclose(db.scenes_est['room_0'].bbox, np.stack([new_origin, new_origin + 0.16 * np.array([12, 17, 21])], axis=1))
    assert tuple(db.scenes_gt['room_1'].volume.shape) == BOX_SHAPE and db.resolution['room_1'] == BOX_RES  # the other scene is untouched
