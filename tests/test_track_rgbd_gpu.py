"""-m gpu: joint geometric + photometric tracking (ojf_track_rgbd, ojf_track_rgbd_associate, tracking.track_frame_rgbd,
Database.track(image=...)) against its numpy restatement (track_rgbd_ref.py): both pyramids, the model maps, J, r and the
reason codes of both terms bit for bit, the fp64 sums and the solve to 1e-12, the whole call as the chain of its single
steps, and the textured plane that depth alone cannot track, end to end."""
import ctypes

import numpy as np
import pytest
import torch

from online_joint_depthfusion_and_semantic_amd import _lib, color, synthetic
from online_joint_depthfusion_and_semantic_amd.config import default_config, database_config
from online_joint_depthfusion_and_semantic_amd.database import Database
from online_joint_depthfusion_and_semantic_amd.ops import camera_arrays
from online_joint_depthfusion_and_semantic_amd.render import render_views
from online_joint_depthfusion_and_semantic_amd.tracking import level_intrinsics, pose12, track_frame, track_frame_rgbd
from render_ref import plane_case
from test_track_gpu import _associate
import color_ref
import track_ref
import track_rgbd_ref as ref

pytestmark = pytest.mark.gpu

# Measured once: the restatement run on the device's own model images (plane_case(64)'s volume, a colour volume fused from
# four 48x64 analytic-colour views, 3 levels, (10, 5, 4) iterations, defaults) from PLANE_STARTS[0] (3 cm / 2 deg in the
# plane), against the true pose: (translation m, rotation deg).  The bound absorbs the colour volume's own error.
PLANE_END_TO_END = (0.000439, 0.00540)


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint8).reshape(got.size, -1) != want.view(np.uint8).reshape(want.size, -1)
    n_bad = int(bad.any(axis=1).sum())
    assert n_bad == 0, '{}: {} of {} elements differ'.format(what, n_bad, got.size)


def _up(cuda, a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(cuda)


def _upload(cuda, case):
    """A case's frame and per-level model images on the device."""
    return dict(depth=_up(cuda, case['depth'], np.float32),
                mask=None if case.get('mask') is None else _up(cuda, case['mask'], np.uint8),
                image=color.pack_image(_up(cuda, case['image'], np.uint8), 1, case['depth'].shape[0], case['depth'].shape[1], cuda),
                mdepth=[_up(cuda, x, np.float32) for x in case['mdepth']],
                mnormal=[_up(cuda, x, np.float32) for x in case['mnormal']],
                mcolor=[_up(cuda, x, np.uint8) for x in case['mcolor']])


def _step(cuda, dev, case, level, pose, dist=0.1, angle=20.0, delta=0.03, frac=0.05, weight=ref.PHOTO_WEIGHT,
          thresh=ref.PHOTO_THRESH, grad=0.1):
    """One ojf_track_rgbd_associate call at ``level`` from ``pose``: everything it exports, on the host."""
    lib = _lib.load()
    h, w = case['depth'].shape
    hl, wl = h >> level, w >> level
    ws = torch.zeros(lib.ojf_track_rgbd_workspace_bytes(h, w, level + 1), dtype=torch.uint8, device=cuda)
    pose_d = torch.zeros(12, dtype=torch.float64, device=cuda)
    sums = torch.zeros(29, dtype=torch.float64, device=cuda)
    jr = torch.zeros((hl * wl, 7), dtype=torch.float32, device=cuda)
    pjr = torch.zeros((hl * wl, 7), dtype=torch.float32, device=cuda)
    reason = torch.full((hl * wl,), 255, dtype=torch.uint8, device=cuda)
    preason = torch.full((hl * wl,), 255, dtype=torch.uint8, device=cuda)
    status = torch.zeros(2, dtype=torch.int32, device=cuda)
    Kd = np.ascontiguousarray(np.asarray(case['K'], np.float64).reshape(9))
    Ki = np.ascontiguousarray(case['Kinv'][level], np.float32)
    Er, Ep = pose12(case['E_ref']), pose12(pose)
    rc = lib.ojf_track_rgbd_associate(
        _lib.ptr(dev['depth']), _lib.ptr(dev['mask']), _lib.ptr(dev['image']), h, w, level, Kd.ctypes.data, Ki.ctypes.data,
        _lib.ptr(dev['mdepth'][level]), _lib.ptr(dev['mnormal'][level]), _lib.ptr(dev['mcolor'][level]), Er.ctypes.data,
        Ep.ctypes.data, dist, angle, delta, frac, weight, thresh, grad, _lib.ptr(ws), ws.numel(), _lib.ptr(pose_d),
        _lib.ptr(sums), _lib.ptr(jr), _lib.ptr(reason), _lib.ptr(pjr), _lib.ptr(preason), _lib.ptr(status),
        _lib.stream_ptr(cuda))
    _lib.check(rc, 'ojf_track_rgbd_associate')
    n = sum((h >> l) * (w >> l) for l in range(level + 1))
    stride = (4 * n + 255) // 256 * 256
    raw = ws.cpu().numpy()
    dflat, iflat = raw[:4 * n].view(np.float32), raw[stride:stride + 4 * n].view(np.float32)
    mflat = raw[2 * stride:2 * stride + 16 * n].view(np.float32).reshape(n, 4)
    dpyr, ipyr, off = [], [], 0
    for l in range(level + 1):
        k = (h >> l) * (w >> l)
        dpyr.append(dflat[off:off + k].reshape(h >> l, w >> l))
        ipyr.append(iflat[off:off + k].reshape(h >> l, w >> l))
        off += k
    jr, pjr = jr.cpu().numpy().reshape(hl, wl, 7), pjr.cpu().numpy().reshape(hl, wl, 7)
    return dict(dpyr=dpyr, ipyr=ipyr, map=mflat[n - hl * wl:].reshape(hl, wl, 4), J=jr[..., :6], r=jr[..., 6],
                pJ=pjr[..., :6], pr=pjr[..., 6], reason=reason.cpu().numpy().reshape(hl, wl),
                preason=preason.cpu().numpy().reshape(hl, wl), sums=sums.cpu().numpy(),
                pose=pose_d.cpu().numpy().reshape(3, 4), status=status.cpu().numpy())


def _check_step(out, case, level, pose, what, dist=0.1, angle=20.0, delta=0.03, frac=0.05, weight=ref.PHOTO_WEIGHT,
                thresh=ref.PHOTO_THRESH, grad=0.1):
    """One ojf_track_rgbd_associate result against the restatement evaluated at ``pose``; returns its associate dict."""
    dpyr = track_ref.pyramid(case['depth'], case.get('mask'), level + 1, delta)
    ipyr = ref.intensity_pyramid(case['image'], level + 1)
    for l in range(level + 1):
        _same_bits(out['dpyr'][l], dpyr[l], '%s: depth pyramid level %d' % (what, l))
        _same_bits(out['ipyr'][l], ipyr[l], '%s: intensity pyramid level %d' % (what, l))
    mmap = ref.model_map(case['mcolor'][level], case['mdepth'][level], grad)
    _same_bits(out['map'], mmap, what + ': model map')
    a = ref.associate(dpyr[level], ipyr[level], case['Kinv'][level], case['K'], level, case['mdepth'][level],
                      case['mnormal'][level], mmap, case['E_ref'], pose, dist, angle, weight, thresh)
    for k in ('reason', 'preason', 'J', 'r', 'pJ', 'pr'):
        _same_bits(out[k], a[k], '%s: %s' % (what, k))
    terms = ref.term_matrix(a, weight)
    want = terms.sum(axis=0)
    bound = 1e-12 * np.abs(terms).sum(axis=0)
    assert (np.abs(out['sums'] - want) <= bound).all(), (what, np.abs(out['sums'] - want) / np.maximum(bound, 1e-300))
    assert out['sums'][28] == ((a['reason'] == 0) | (a['preason'] == 0)).sum(), what
    code, P = track_ref.step(out['sums'], pose, frac * a['reason'].size)
    assert int(out['status'][0]) == code, (what, out['status'], code)
    assert np.abs(out['pose'] - P).max() <= 1e-12, what
    a['map'] = mmap
    return a


@pytest.mark.parametrize('h,w,levels', [(32, 32, 1), (25, 41, 1), (64, 64, 4), (67, 93, 3)])
def test_one_step_is_the_restatement(cuda, h, w, levels):
    """1024 pixels (one block), 1025 (a block of one pixel), the smallest legal level, odd sizes with prepare tiles cut at
    the right and bottom edges - on inputs that take every photometric path (track_rgbd_ref.hostile_case)."""
    case = ref.hostile_case(h, w, levels)
    dev = _upload(cuda, case)
    for l in range(levels):
        what = '%dx%d level %d' % (h, w, l)
        # a threshold nothing exceeds, then the median |r_I| itself (its pixel stays) and the value below it (it is cut)
        out = _step(cuda, dev, case, l, case['pose'], thresh=1e9)
        a = _check_step(out, case, l, case['pose'], what, thresh=1e9)
        c = np.bincount(a['preason'].reshape(-1), minlength=11)
        print(what, 'geometric', np.bincount(a['reason'].reshape(-1), minlength=8).tolist(), 'photometric', c.tolist())
        if l > 0:
            continue
        assert all(c[k] > 0 for k in (0, 1, 3, 4, 5, 6, 8)) and c[9] == 0, (what, c)
        assert (a['reason'][a['preason'] == 0] == 2).any(), what  # a photometric row without a normal
        mag = np.abs(a['pr'][a['preason'] == 0])
        t0 = np.sort(mag)[mag.size // 2]
        at = a['preason'] == 0
        at &= np.abs(a['pr']) == t0
        assert at.any() and t0 > 0
        for thresh, kept in ((float(t0), 0), (float(np.nextafter(t0, np.float32(0))), 9)):
            out = _step(cuda, dev, case, l, case['pose'], thresh=thresh)
            b = _check_step(out, case, l, case['pose'], '%s, photo_thresh %r' % (what, thresh), thresh=thresh)
            assert (b['preason'][at] == kept).all() and (b['preason'] == 9).any() and (b['preason'] == 0).any(), (what, thresh)
        # the model map: pixels without colour inside the image, a depth step between coloured pixels, values 0 and 255
        mcol, mmap = case['mcolor'][0], a['map']
        has = mcol[..., 3] != 0
        inner = np.zeros_like(has)
        inner[1:-1, 1:-1] = has[1:-1, 1:-1] & has[:-2, 1:-1] & has[2:, 1:-1] & has[1:-1, :-2] & has[1:-1, 2:]
        assert (~has[1:-1, 1:-1]).any() and (inner & (mmap[..., 3] == 0)).any() and (mmap[..., 3] == 1).any(), what
        assert (mmap[..., 0] == 0).any() and (mmap[..., 0] == 255).any(), what
        I0 = ref.intensity(case['image'])
        assert (I0 == 0).any() and (I0 == 255).any(), what
        # live pixels that project into the outermost model rows and columns
        mr, mc = a['mrow'], a['mcol']
        rim = (mr == 0) | (mr == h - 1) | (mc == 0) | (mc == w - 1)
        assert (rim & (a['preason'] == 8)).any() and not (rim & (a['preason'] == 0)).any(), what
    # lambda = 0: no photometric rows, reason 10 everywhere
    out = _step(cuda, dev, case, 0, case['pose'], weight=0.0)
    a = _check_step(out, case, 0, case['pose'], '%dx%d, photo_weight 0' % (h, w), weight=0.0)
    assert (a['preason'] == 10).all() and out['sums'][28] == (a['reason'] == 0).sum()


@pytest.mark.parametrize('h,w,levels', [(25, 41, 1), (67, 93, 3)])
def test_one_step_at_photo_weight_0_is_ojf_track_associate(cuda, h, w, levels):
    """The front half the two trackers share (csrc/ojf_track_front.h), seen at step level: from the same pose,
    ojf_track_associate and ojf_track_rgbd_associate at photo_weight 0 leave the same bits in everything both export, at
    every level.  1025 pixels (a block of one pixel) and odd halves with cut tiles; at level 0 the inputs reach every
    geometric reason (track_ref.associate counts 26, 532, 395, 14, 46, 2, 2, 8 of reasons 0..7 at 25x41 and 238, 3027,
    2373, 88, 356, 9, 21, 119 at 67x93; the coarser levels of 67x93 lack some)."""
    case = ref.hostile_case(h, w, levels)
    dev = _upload(cuda, case)
    for l in range(levels):
        what = '%dx%d level %d' % (h, w, l)
        both = _step(cuda, dev, case, l, case['pose'], weight=0.0)
        depth_only = _associate(cuda, case['depth'], case['mask'], l, case['K'], case['Kinv'][l], dev['mdepth'][l],
                                dev['mnormal'][l], case['E_ref'], case['pose'])
        for k in range(l + 1):
            _same_bits(both['dpyr'][k], depth_only['pyr'][k], '%s: depth pyramid level %d' % (what, k))
        for k in ('J', 'r', 'reason', 'sums', 'pose', 'status'):
            _same_bits(both[k], depth_only[k], '%s: %s' % (what, k))
        assert (both['preason'] == 10).all(), what
        counts = np.bincount(depth_only['reason'].reshape(-1), minlength=8)
        print(what, 'geometric', counts.tolist())
        if l == 0:
            assert len(counts) == 8 and (counts > 0).all(), (what, counts)


# ---- the whole call
POISON = 0x7f


def _track(cuda, dev, case, iterations, rows, weight=ref.PHOTO_WEIGHT, rgbd=True):
    """One raw ojf_track_rgbd (or ojf_track) call into buffers filled with 0x7f bytes."""
    lib = _lib.load()
    h, w = case['depth'].shape
    levels = len(case['mdepth'])
    its = np.ascontiguousarray(list(iterations) + [0] * (4 - len(iterations)), dtype=np.int32)
    K = np.ascontiguousarray(np.asarray(case['K'], np.float64).reshape(9))
    Kinv = np.ascontiguousarray(np.stack(case['Kinv']), dtype=np.float32)
    md = np.array([_lib.ptr(m) for m in dev['mdepth']], dtype=np.uint64)
    mn = np.array([_lib.ptr(m) for m in dev['mnormal']], dtype=np.uint64)
    mc = np.array([_lib.ptr(m) for m in dev['mcolor']], dtype=np.uint64)
    E_ref, E_init = pose12(case['E_ref']), pose12(case['E_init'])
    size = lib.ojf_track_rgbd_workspace_bytes(h, w, levels) if rgbd else lib.ojf_track_workspace_bytes(h, w, levels)
    ws = torch.full((int(size),), POISON, dtype=torch.uint8, device=cuda)
    out = torch.full((96 + 32 * (rows + 1) + 8,), POISON, dtype=torch.uint8, device=cuda)
    stats_ptr = out.data_ptr() + 96
    status_ptr = stats_ptr + 32 * (rows + 1)
    if rgbd:
        rc = lib.ojf_track_rgbd(_lib.ptr(dev['depth']), _lib.ptr(dev['mask']), _lib.ptr(dev['image']), h, w, levels,
                                K.ctypes.data, Kinv.ctypes.data, md.ctypes.data, mn.ctypes.data, mc.ctypes.data,
                                E_ref.ctypes.data, E_init.ctypes.data, its.ctypes.data, 0.1, 20.0, 0.03, 0.05, weight,
                                ref.PHOTO_THRESH, 0.1, _lib.ptr(ws), ws.numel(), out.data_ptr(), stats_ptr, status_ptr,
                                _lib.stream_ptr(cuda))
    else:
        rc = lib.ojf_track(_lib.ptr(dev['depth']), _lib.ptr(dev['mask']), h, w, levels, K.ctypes.data, Kinv.ctypes.data,
                           md.ctypes.data, mn.ctypes.data, E_ref.ctypes.data, E_init.ctypes.data, its.ctypes.data, 0.1, 20.0,
                           0.03, 0.05, _lib.ptr(ws), ws.numel(), out.data_ptr(), stats_ptr, status_ptr, _lib.stream_ptr(cuda))
    _lib.check(rc, 'ojf_track_rgbd' if rgbd else 'ojf_track')
    host = out.cpu().numpy()
    raw = host[96:96 + 32 * (rows + 1)].reshape(rows + 1, 32)
    assert (raw[rows] == POISON).all(), 'a stats row past the last one was written'
    return dict(pose=host[:96].view(np.float64).reshape(3, 4).copy(), stats=raw[:rows].copy().view(np.float64).reshape(rows, 4),
                stats_bytes=raw[:rows].copy(), status=host[96 + 32 * (rows + 1):].view(np.int32).copy())


@pytest.fixture(scope='module')
def room64():
    """Frame pair (53, 54) of the 64x64 synthetic room with analytic colour, from a start 3 deg / 4 cm off."""
    st = synthetic.SyntheticStream(64, 64, 64, 400)
    frames = color_ref.room_frames(st, 55)
    return ref.room_tracking_case(st, frames, 53, (3.0, 0.04, (1, -1, 0.5), (-1, 0, 1)))


def test_the_call_is_the_chain_of_its_steps(cuda, room64):
    case = room64
    dev = _upload(cuda, case)
    iterations = (10, 5, 4)
    steps = track_ref.schedule(iterations, 3)
    n = len(steps)
    runs = [_track(cuda, dev, case, track_ref.prefix_iterations(iterations, 3, k), n) for k in range(n + 1)]
    _same_bits(runs[0]['pose'], case['E_init'][:3], 'pose of the call without iterations')
    for k, run in enumerate(runs):
        assert run['status'].tolist() == [0, -1], (k, run['status'])
        assert (run['stats_bytes'][k:] == POISON).all(), 'the call of %d steps wrote a later stats row' % k
    for k, l in enumerate(steps):
        what = 'step %d (level %d)' % (k, l)
        P = runs[k]['pose']
        out = _step(cuda, dev, case, l, P)
        _same_bits(out['pose'], runs[k + 1]['pose'], what + ': pose')
        sums = out['sums']
        _same_bits(runs[k + 1]['stats'][k][:2], np.array([sums[28], sums[27] / sums[28]]), what + ': stats')
        a = _check_step(out, case, l, P, what)
        # (at level 2, 16 x 16, neighbouring model depths of this room differ by more than grad_depth almost everywhere)
        assert (a['reason'] == 0).any() and (a['preason'] == 0).mean() > (0.3 if l < 2 else 0.0), what
    # the same bits twice
    again = _track(cuda, dev, case, iterations, n)
    _same_bits(again['pose'], runs[n]['pose'], 'pose of a second call')
    _same_bits(again['stats'], runs[n]['stats'], 'stats of a second call')
    print('64x64 room pair: %.3f mm, %.4f deg from the truth' % track_ref.pose_error(runs[n]['pose'], case['E_true']))
    # photo_weight 0: ojf_track's pose, stats and status
    a, b = _track(cuda, dev, case, iterations, n, weight=0.0), _track(cuda, dev, case, iterations, n, rgbd=False)
    assert a['status'].tolist() == b['status'].tolist()
    _same_bits(a['pose'], b['pose'], 'pose at photo_weight 0')
    _same_bits(a['stats'], b['stats'], 'stats at photo_weight 0')
    assert not np.array_equal(a['pose'], runs[n]['pose'])


# ---- the textured plane, end to end
@pytest.fixture(scope='module')
def plane(cuda):
    """plane_case(64)'s volume with unit weights and a colour volume fused from four 48x64 analytic-colour views."""
    tsdf, origin, res, K, E, want, _ = plane_case(64)
    tsdf = torch.from_numpy(tsdf).to(cuda)
    weights = torch.ones_like(tsdf)
    colors = color.new_volume(tsdf.shape, cuda)
    views = [E.copy() for _ in range(4)]
    for v, (dx, dy) in zip(views[1:], ((0.3, 0.1), (-0.3, -0.1), (0.05, 0.3))):
        v[0, 3] += dx
        v[1, 3] += dy
    shots = [ref.plane_view(v, K, 48, 64) for v in views]
    color.integrate_color(colors, origin=origin, resolution=res,
                          image=_up(cuda, np.stack([s[2] for s in shots]), np.uint8),
                          depth=_up(cuda, np.stack([s[0] for s in shots]), np.float32), intrinsics=K,
                          extrinsics=np.stack(views), band=3 * res)
    depth, _, image = ref.plane_view(E, K, 48, 64)
    return dict(tsdf=tsdf, weights=weights, colors=colors, origin=origin, res=res, K=K, E=E, depth=depth.astype(np.float32),
                image=image)


def test_the_textured_plane_is_tracked_end_to_end(cuda, plane):
    p = plane
    kw = dict(origin=p['origin'], resolution=p['res'], depth=p['depth'], intrinsics=p['K'])
    control = track_frame(p['tsdf'], p['weights'], extrinsics=p['E'], **kw)
    assert not control['ok'] and control['status'] == 2  # geometry alone: a singular system (test_track_gpu pins it)
    E0 = np.eye(4)
    E0[:3] = track_ref.perturb(p['E'], *ref.PLANE_STARTS[0])
    got = track_frame_rgbd(p['tsdf'], p['weights'], p['colors'], image=_up(cuda, p['image'], np.uint8), extrinsics=E0, **kw)
    assert got['ok'] and got['status'] == 0 and got['stats'].shape == (19, 4), got['status']
    # the restatement on the device's own model images
    Kinv, md, mn, mc = [], [], [], []
    for l in range(3):
        Kl = level_intrinsics(p['K'], l)
        r = render_views(p['tsdf'], p['weights'], None, origin=p['origin'], resolution=p['res'], intrinsics=Kl,
                         extrinsics=E0[:3], shape=(48 >> l, 64 >> l))
        c = color.render_color(p['colors'], origin=p['origin'], resolution=p['res'], intrinsics=Kl, extrinsics=E0[:3],
                               depth=r['depth'])
        Kinv.append(camera_arrays(Kl, E0[:3])[0])
        md.append(r['depth'][0].cpu().numpy())
        mn.append(r['normals'][0].cpu().numpy())
        mc.append(c[0].cpu().numpy())
    assert all((x[..., 3] != 0).mean() > 0.8 for x in mc)
    want, status, _ = ref.run(p['depth'], None, p['image'], p['K'], Kinv, md, mn, mc, E0[:3], E0[:3], (10, 5, 4))
    assert status == (0, -1)
    gap = np.abs(got['extrinsics'][:3] - want).max()
    e_ref = track_ref.pose_error(want, p['E'])
    e_gpu = track_ref.pose_error(got['extrinsics'], p['E'])
    print('textured plane: GPU vs restatement max |dP| %.3g; restatement %.4f mm %.5f deg, GPU %.4f mm %.5f deg from the truth'
          % (gap, 1e3 * e_ref[0], e_ref[1], 1e3 * e_gpu[0], e_gpu[1]))
    assert gap <= 1e-9, gap
    assert e_gpu[0] <= 1.5 * PLANE_END_TO_END[0] and e_gpu[1] <= 1.5 * PLANE_END_TO_END[1], e_gpu


# ---- Database.track(image=...)
H, W, GRID = 48, 64, 64


class _Room(synthetic.SyntheticDataset):
    def __init__(self):
        super().__init__(H, W, GRID, 400, scenes=['room_0'])

    def get_grid(self, scene, truncation, semantic_grid=True):
        from online_joint_depthfusion_and_semantic_amd.database import Voxelgrid
        st = self.streams[scene]
        g = Voxelgrid(st.resolution)
        g.from_array(synthetic.gt_volumes(GRID, truncation)[0].copy(), st.bbox)
        return (g,)


def test_database_track_with_an_image(cuda):
    cfg = default_config(H, W)
    cfg.SETTINGS.device = str(cuda)
    db = Database(_Room(), database_config(cfg))
    s = 'room_0'
    st = synthetic.SyntheticStream(H, W, GRID, 400)
    frames = color_ref.room_frames(st, 55)
    db.scenes_est[s].volume.copy_(torch.from_numpy(synthetic.gt_volumes(GRID)[0]).to(cuda))
    db.fusion_weights[s].fill_(1.0)
    f0, f1 = frames[53], frames[54]
    args = (s, f1['tof_depth'], st.K, f0['extrinsics'])
    with pytest.raises(ValueError, match='no colour volume'):
        db.track(*args, mask=f1['mask'], image=f1['image'])
    for f in frames[44:54:3]:
        db.integrate_color(s, _up(cuda, f['image'], np.uint8), f['depth_gt'], st.K, f['extrinsics'])
    a = db.track(*args, mask=f1['mask'], image=_up(cuda, f1['image'], np.uint8))
    direct = track_frame_rgbd(db.scenes_est[s].volume, db.fusion_weights[s], db.colors[s], origin=db.origin[s],
                              resolution=float(db.resolution[s]), image=_up(cuda, f1['image'], np.uint8), depth=f1['tof_depth'],
                              intrinsics=st.K, extrinsics=f0['extrinsics'], mask=f1['mask'])
    plain = db.track(*args, mask=f1['mask'])
    depth_only = track_frame(db.scenes_est[s].volume, db.fusion_weights[s], origin=db.origin[s],
                             resolution=float(db.resolution[s]), depth=f1['tof_depth'], intrinsics=st.K,
                             extrinsics=f0['extrinsics'], mask=f1['mask'])
    db.to_numpy()
    b = db.track(*args, mask=f1['mask'], image=f1['image'])
    assert a['ok'] and b['ok'] and direct['ok']
    for other, what in ((b, 'host state'), (direct, 'track_frame_rgbd')):
        _same_bits(a['extrinsics'], other['extrinsics'], 'pose, ' + what)
        _same_bits(a['stats'], other['stats'], 'stats, ' + what)
    assert plain['status'] == depth_only['status']
    _same_bits(plain['extrinsics'], depth_only['extrinsics'], 'pose with image=None')
    _same_bits(plain['stats'], depth_only['stats'], 'stats with image=None')
    assert not np.array_equal(a['extrinsics'], plain['extrinsics'])
    print('Database.track(image=...): %.4f m, %.4f deg from the truth' % track_ref.pose_error(a['extrinsics'], f1['extrinsics']))


# ---- argument checks: the failure code and its message, without a launch
def test_argument_checks():
    lib = _lib.load()
    host = ctypes.create_string_buffer(256)
    dev = ctypes.addressof(host)  # "device" addresses nothing reads: every call below is refused before any launch
    K = np.array([64.0, 0, 32, 0, 64, 32, 0, 0, 1])
    Ki = np.zeros((4, 9), np.float32)
    E = np.eye(4)[:3].reshape(12).copy()
    ptrs = np.full(4, dev, dtype=np.uint64)
    its = np.array([1, 1, 1, 1], np.int32)
    good = dict(depth=dev, image=dev, h=64, w=64, levels=3, K=K.ctypes.data, Ki=Ki.ctypes.data, md=ptrs.ctypes.data,
                mn=ptrs.ctypes.data, mc=ptrs.ctypes.data, E=E.ctypes.data, its=its.ctypes.data, dist=0.1, angle=20.0, delta=0.03,
                frac=0.05, weight=0.002, thresh=40.0, grad=0.1, ws=dev, ws_bytes=lib.ojf_track_rgbd_workspace_bytes(64, 64, 3),
                out=dev)
    assert good['ws_bytes'] > lib.ojf_track_workspace_bytes(64, 64, 3)
    assert lib.ojf_track_rgbd_workspace_bytes(64, 64, 0) == 0 and lib.ojf_track_rgbd_workspace_bytes(0, 64, 1) == 0

    def whole(d):
        return lib.ojf_track_rgbd(d['depth'], None, d['image'], d['h'], d['w'], d['levels'], d['K'], d['Ki'], d['md'], d['mn'],
                                  d['mc'], d['E'], d['E'], d['its'], d['dist'], d['angle'], d['delta'], d['frac'], d['weight'],
                                  d['thresh'], d['grad'], d['ws'], d['ws_bytes'], d['out'], d['out'], d['out'], None)

    def step(d):
        return lib.ojf_track_rgbd_associate(d['depth'], None, d['image'], d['h'], d['w'], d['levels'] - 1, d['K'], d['Ki'],
                                            dev if d['md'] else None, dev, dev if d['mc'] else None, d['E'], d['E'], d['dist'],
                                            d['angle'], d['delta'], d['frac'], d['weight'], d['thresh'], d['grad'], d['ws'],
                                            d['ws_bytes'], d['out'], d['out'], None, None, None, None, d['out'], None)

    null_level = np.array([dev, 0, dev, dev], dtype=np.uint64)
    cases = [(dict(depth=None), b'null'), (dict(image=None), b'null'), (dict(mc=None), b'null'), (dict(ws=None), b'null'),
             (dict(levels=5), b'levels'), (dict(levels=4, h=60), b'8 x 8'), (dict(h=0), b'image size'),
             (dict(dist=0.0), b'thresholds'), (dict(angle=181.0), b'thresholds'), (dict(frac=1.5), b'thresholds'),
             (dict(thresh=-1.0), b'thresholds'), (dict(thresh=float('nan')), b'thresholds'), (dict(grad=0.0), b'thresholds'),
             (dict(weight=-0.001), b'photo_weight'), (dict(weight=float('inf')), b'photo_weight'),
             (dict(weight=float('nan')), b'photo_weight'), (dict(ws_bytes=good['ws_bytes'] - 1), b'workspace too small')]
    for fault, word in cases:
        for call, prefix in ((whole, b'ojf_track_rgbd:'), (step, b'ojf_track_rgbd_associate:')):
            assert call(dict(good, **fault)) != 0, (fault, prefix)
            msg = lib.ojf_last_error()
            assert msg.startswith(prefix) and word in msg, (fault, prefix, msg)
    negative, many = np.array([1, -1, 1, 1], np.int32), np.array([100, 20, 9, 0], np.int32)
    for fault, word in ((dict(mc=null_level.ctypes.data), b'model maps'), (dict(its=negative.ctypes.data), b'negative'),
                        (dict(its=many.ctypes.data), b'OJF_TRACK_MAX_ITERATIONS')):
        assert whole(dict(good, **fault)) != 0, fault
        assert word in lib.ojf_last_error(), (fault, lib.ojf_last_error())
