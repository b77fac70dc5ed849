"""-m gpu: camera tracking (ojf_track, ojf_track_associate, tracking.track_frame, Database.track, drivers.test_fusion with
TESTING.track_invalid_poses) against its numpy restatement (track_ref.py: the pyramid, J, r and the reason codes bit for
bit, the fp64 sums and the solve to 1e-12) and against the ground-truth trajectory of the synthetic room."""
import ctypes

import numpy as np
import pytest
import torch

from online_joint_depthfusion_and_semantic_amd import _lib, synthetic
from online_joint_depthfusion_and_semantic_amd.config import default_config, database_config
from online_joint_depthfusion_and_semantic_amd.database import Database
from online_joint_depthfusion_and_semantic_amd.ops import camera_arrays
from online_joint_depthfusion_and_semantic_amd.pipeline import Pipeline
from online_joint_depthfusion_and_semantic_amd.render import render_views
from online_joint_depthfusion_and_semantic_amd.tracking import level_intrinsics, track_frame
from render_ref import plane_case
import track_ref

pytestmark = pytest.mark.gpu

H, W, GRID = 240, 320, 256


_GT = {}


def _gt(truncation=0.1):
    """synthetic.gt_volumes(256) once per module (5 s of numpy)."""
    if truncation not in _GT:
        _GT[truncation] = synthetic.gt_volumes(GRID, truncation)[0]
    return _GT[truncation]


@pytest.fixture(scope='module')
def room(cuda):
    """The GT room at 256^3 on the device and a 400-frame stream over it (1.4 cm and ~1 deg per frame, 5 mm noise)."""
    tsdf = _gt()
    origin, res, _ = synthetic.grid_spec(GRID)
    st = synthetic.SyntheticStream(H, W, GRID, 400)
    return dict(tsdf=torch.from_numpy(tsdf).to(cuda), origin=origin, res=res, st=st, K=st.K)


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint8).reshape(got.size, -1) != want.view(np.uint8).reshape(want.size, -1)
    n_bad = int(bad.any(axis=1).sum())
    assert n_bad == 0, '{}: {} of {} elements differ'.format(what, n_bad, got.size)


def _models(room, E_ref, levels):
    out = []
    for l in range(levels):
        Kl = level_intrinsics(room['K'], l)
        r = render_views(room['tsdf'], None, origin=room['origin'], resolution=room['res'], intrinsics=Kl, extrinsics=E_ref,
                         shape=(H >> l, W >> l))
        out.append((r['depth'][0].contiguous(), r['normals'][0].contiguous(), camera_arrays(Kl, E_ref)[0]))
    return out


def _associate(cuda, depth, mask, level, K, Ki, mdepth, mnormal, E_ref, E_pose, **kw):
    """One ojf_track_associate call: (pyramid levels 0..level, J, r, reason, sums, pose, status) on the host.  Keywords:
    dist (0.1), angle (20), delta (0.03), frac (the minimum inlier fraction, 0.05)."""
    lib = _lib.load()
    h, w = depth.shape
    hl, wl = h >> level, w >> level
    ws = torch.zeros(lib.ojf_track_workspace_bytes(h, w, level + 1), dtype=torch.uint8, device=cuda)
    pose = torch.zeros(12, dtype=torch.float64, device=cuda)
    sums = torch.zeros(29, dtype=torch.float64, device=cuda)
    jr = torch.zeros((hl * wl, 7), dtype=torch.float32, device=cuda)
    reason = torch.full((hl * wl,), 255, dtype=torch.uint8, device=cuda)
    status = torch.zeros(2, dtype=torch.int32, device=cuda)
    d = torch.from_numpy(np.ascontiguousarray(depth, np.float32)).to(cuda)
    m = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask).astype(np.uint8)).to(cuda)
    Kd = np.ascontiguousarray(np.asarray(K, np.float64).reshape(9))
    Ki = np.ascontiguousarray(Ki, np.float32)
    Er, Ep = track_ref_pose(E_ref), track_ref_pose(E_pose)
    rc = lib.ojf_track_associate(_lib.ptr(d), _lib.ptr(m), h, w, level, Kd.ctypes.data, Ki.ctypes.data, _lib.ptr(mdepth),
                                 _lib.ptr(mnormal), Er.ctypes.data, Ep.ctypes.data, kw.get('dist', 0.1), kw.get('angle', 20.0),
                                 kw.get('delta', 0.03), kw.get('frac', 0.05), _lib.ptr(ws), ws.numel(), _lib.ptr(pose),
                                 _lib.ptr(sums), _lib.ptr(jr),
                                 _lib.ptr(reason), _lib.ptr(status), _lib.stream_ptr(cuda))
    _lib.check(rc, 'ojf_track_associate')
    wsf = ws.cpu().numpy()[:4 * sum((h >> l) * (w >> l) for l in range(level + 1))].view(np.float32)
    pyr, off = [], 0
    for l in range(level + 1):
        n = (h >> l) * (w >> l)
        pyr.append(wsf[off:off + n].reshape(h >> l, w >> l))
        off += n
    jr = jr.cpu().numpy().reshape(hl, wl, 7)
    return dict(pyr=pyr, J=jr[..., :6], r=jr[..., 6], reason=reason.cpu().numpy().reshape(hl, wl),
                sums=sums.cpu().numpy(), pose=pose.cpu().numpy().reshape(3, 4), status=status.cpu().numpy())


def track_ref_pose(E):
    return np.ascontiguousarray(np.asarray(E, np.float64).reshape(-1, 4)[:3].reshape(12))


def _check_level(out, level, K, Ki, mdepth, mnormal, E_ref, E_pose, **kw):
    J, r, reason = track_ref.associate(out['pyr'][level], Ki, K, level, mdepth.cpu().numpy(), mnormal.cpu().numpy(), E_ref,
                                       E_pose, **kw)
    _same_bits(out['reason'], reason, 'reason codes, level %d' % level)
    _same_bits(out['J'], J, 'J, level %d' % level)
    _same_bits(out['r'], r, 'r, level %d' % level)
    return J, r, reason


def test_pyramid_is_the_restatement(room, cuda):
    f = room['st'].frame(7)
    depth, mask = f['tof_depth'], f['mask']
    assert (depth == 0).any() and (~mask).any()
    E = f['extrinsics']
    models = _models(room, E, 3)
    out = _associate(cuda, depth, mask, 2, room['K'], models[2][2], models[2][0], models[2][1], E, E)
    want = track_ref.pyramid(depth, mask, 3)
    for l in range(3):
        _same_bits(out['pyr'][l], want[l], 'pyramid level %d' % l)
    assert (want[2] > 0).mean() > 0.95


def test_association_is_the_restatement_on_every_level(room, cuda):
    st = room['st']
    f0, f1 = st.frame(20), st.frame(21)
    E_ref = f0['extrinsics']
    models = _models(room, E_ref, 3)
    for l in range(3):
        md, mn, Ki = models[l]
        out = _associate(cuda, f1['tof_depth'], f1['mask'], l, room['K'], Ki, md, mn, E_ref, E_ref)
        _same_bits(out['pyr'][l], track_ref.pyramid(f1['tof_depth'], f1['mask'], l + 1)[l], 'pyramid level %d' % l)
        _, _, reason = _check_level(out, l, room['K'], Ki, md, mn, E_ref, E_ref)
        # (at level 0 the 5-mm noise tilts most live normals beyond 20 degrees: code 7 rejects them)
        assert (reason == 0).mean() > (0.1 if l == 0 else 0.5), (l, np.bincount(reason.reshape(-1), minlength=8))


def test_every_reason_code_occurs_and_matches(room, cuda):
    """A crafted frame: the reference camera 0.5 m in front of the live one (near points behind it, border points outside
    its image), a live patch 0.3 m from the camera (behind the reference), a live patch pushed 0.3 m back (too far),
    a model patch with no depth and one with flipped normals."""
    st = room['st']
    f = st.frame(40)
    E_live = f['extrinsics']
    E_ref = E_live.copy()
    E_ref[:, 3] += 0.5 * E_live[:, 2]
    depth = f['tof_depth'].copy()
    depth[100:120, 150:170] = 0.3
    depth[60:80, 60:80] += 0.3
    md, mn, Ki = _models(room, E_ref, 1)[0]
    md, mn = md.clone(), mn.clone()
    md[150:170, 200:220] = 0
    mn[30:50, 200:220] *= -1
    out = _associate(cuda, depth, f['mask'], 0, room['K'], Ki, md, mn, E_ref, E_live)
    _, _, reason = _check_level(out, 0, room['K'], Ki, md, mn, E_ref, E_live)
    counts = np.bincount(reason.reshape(-1), minlength=8)
    assert (counts[:8] > 0).all(), dict(zip(track_ref.REASONS, counts.tolist()))


def test_sums_solve_and_determinism(room, cuda):
    st = room['st']
    f0, f1 = st.frame(60), st.frame(61)
    E_ref = f0['extrinsics']
    md, mn, Ki = _models(room, E_ref, 1)[0]
    out = _associate(cuda, f1['tof_depth'], f1['mask'], 0, room['K'], Ki, md, mn, E_ref, E_ref)
    J, r, reason = _check_level(out, 0, room['K'], Ki, md, mn, E_ref, E_ref)
    terms = track_ref.term_matrix(J, r, reason)
    want = terms.sum(axis=0)
    bound = 1e-12 * np.abs(terms).sum(axis=0)
    assert (np.abs(out['sums'] - want) <= bound).all(), np.abs(out['sums'] - want) / np.maximum(bound, 1e-300)
    assert out['sums'][28] == (reason == 0).sum()
    code, P = track_ref.step(out['sums'], E_ref, 0.05 * H * W)
    assert code == 0 and out['status'][0] == 0
    assert np.abs(out['pose'] - P).max() <= 1e-12
    # the whole call: the same bits twice
    kw = dict(origin=room['origin'], resolution=room['res'], depth=f1['tof_depth'], mask=f1['mask'], intrinsics=room['K'],
              extrinsics=E_ref)
    a, b = track_frame(room['tsdf'], None, **kw), track_frame(room['tsdf'], None, **kw)
    assert a['ok'] and b['ok']
    _same_bits(a['extrinsics'], b['extrinsics'], 'pose')
    _same_bits(a['stats'], b['stats'], 'stats')
    assert a['stats'].shape == (19, 4)


def _track(room, frame, E_init, E_ref):
    return track_frame(room['tsdf'], None, origin=room['origin'], resolution=room['res'], depth=frame['tof_depth'],
                       mask=frame['mask'], intrinsics=room['K'], extrinsics=E_init, reference_extrinsics=E_ref)


def test_convergence_on_the_gt_room(room):
    st = room['st']
    errs = []
    # (frames 0-5 and 390-399 look at one wall: a single plane, which ICP cannot pin down - see test_failure_is_reported)
    for i in (20, 60, 110, 150, 200, 230, 300, 340):  # frame pairs from the previous GT pose
        f = st.frame(i + 1)
        out = _track(room, f, st.frame(i)['extrinsics'], st.frame(i)['extrinsics'])
        assert out['ok'], (i, out['status'])
        errs.append(track_ref.pose_error(out['extrinsics'], f['extrinsics']))
    starts = [(3.0, 0.05, (1, 0, 0), (0, 1, 0)), (3.0, 0.0, (0, 1, 0), (1, 0, 0)), (0.0, 0.05, (0, 0, 1), (1, 1, 1)),
              (3.0, 0.05, (1, -1, 0.5), (-1, 0, 1))]
    for k, (deg, m, axis, direction) in enumerate(starts):  # perturbed starts: up to 5 cm / 3 deg from the truth
        i = 25 + 90 * k
        f = st.frame(i + 1)
        E0 = track_ref.perturb(f['extrinsics'], deg, m, axis, direction)
        out = _track(room, f, E0, st.frame(i)['extrinsics'])
        assert out['ok'], (i, out['status'])
        errs.append(track_ref.pose_error(out['extrinsics'], f['extrinsics']))
    errs = np.array(errs)
    print('pair / perturbed-start errors: max %.2f mm, %.4f deg' % (1e3 * errs[:, 0].max(), errs[:, 1].max()))
    assert errs[:, 0].max() <= 0.005 and errs[:, 1].max() <= 0.2, errs
    # a chain of 30 frames, each from the previous tracked pose
    E = st.frame(100)['extrinsics']
    for i in range(101, 131):
        out = _track(room, st.frame(i), E, E)
        assert out['ok'], (i, out['status'])
        E = out['extrinsics']
    dt, dr = track_ref.pose_error(E, st.frame(130)['extrinsics'])
    print('30-frame chain drift: %.2f mm, %.4f deg' % (1e3 * dt, dr))
    assert dt <= 0.01 and dr <= 0.5, (dt, dr)


def test_failure_is_reported(room, cuda):
    st = room['st']
    f = st.frame(5)
    E = f['extrinsics']
    out = track_frame(room['tsdf'], None, origin=room['origin'], resolution=room['res'], depth=np.zeros((H, W), np.float32),
                      intrinsics=room['K'], extrinsics=E)
    assert not out['ok'] and out['status'] == 1
    assert np.array_equal(out['extrinsics'][:3], E) and np.isfinite(out['stats']).all()
    # a single plane constrains 3 of the 6 DOF
    tsdf, origin, res, K, Ep, want, _ = plane_case(64)
    out = track_frame(torch.from_numpy(tsdf).to(cuda), None, origin=origin, resolution=res,
                      depth=want.astype(np.float32), intrinsics=K, extrinsics=Ep)
    assert not out['ok'] and out['status'] == 2, out['status']
    assert np.array_equal(out['extrinsics'][:3], Ep) and np.isfinite(out['stats']).all()


def test_database_track_resident_and_host_state(room, cuda):
    cfg = default_config(H, W)
    cfg.SETTINGS.device = str(cuda)
    st = room['st']
    db = Database(_Stream(), database_config(cfg))
    s = st.scene
    db.scenes_est[s].volume.copy_(room['tsdf'])
    db.fusion_weights[s].fill_(1.0)
    f0, f1 = st.frame(200), st.frame(201)
    kw = dict(mask=f1['mask'])
    a = db.track(s, f1['tof_depth'], st.K, f0['extrinsics'], **kw)
    db.to_numpy()
    b = db.track(s, f1['tof_depth'], st.K, f0['extrinsics'], **kw)
    assert a['ok'] and b['ok']
    _same_bits(a['extrinsics'], b['extrinsics'], 'pose')
    _same_bits(a['stats'], b['stats'], 'stats')
    assert track_ref.pose_error(a['extrinsics'], f1['extrinsics'])[0] <= 0.005
    # a solid slab in the free space in front of the camera: unobserved it is transparent, observed it is not
    db.to_torch()
    origin, res = room['origin'], room['res']
    ax = origin[0] + (np.arange(GRID) + 0.5) * res
    cam = f0['extrinsics'][:, 3]
    fwd = f0['extrinsics'][:, 2]
    centre = cam + 1.0 * fwd
    sel = [np.flatnonzero(np.abs(ax - centre[i]) < (0.04 if i == int(np.argmax(np.abs(fwd))) else 0.5)) for i in range(3)]
    ix = np.ix_(*sel)
    tsdf = db.scenes_est[s].volume
    tsdf_np = tsdf.cpu().numpy()
    tsdf_np[ix] = -0.1
    tsdf.copy_(torch.from_numpy(tsdf_np))
    wgt = db.fusion_weights[s].cpu().numpy()
    wgt[ix] = 0
    db.fusion_weights[s].copy_(torch.from_numpy(wgt))
    c = db.track(s, f1['tof_depth'], st.K, f0['extrinsics'], **kw)
    dt, dr = track_ref.pose_error(c['extrinsics'], a['extrinsics'])
    assert c['ok'] and dt <= 1e-4 and dr <= 0.01, (dt, dr)
    db.fusion_weights[s].fill_(1.0)
    d = db.track(s, f1['tof_depth'], st.K, f0['extrinsics'], **kw)
    assert d['stats'][-1, 0] < a['stats'][-1, 0] - 0.03 * H * W  # observed, the slab hides part of the room


class _Stream(synthetic.SyntheticDataset):
    """Frames 150..161 of a 400-frame trajectory; frames in ``invalid`` get extrinsics = inf, frames in ``drop`` are left
    out."""

    def __init__(self, invalid=(), drop=()):
        super().__init__(H, W, GRID, 400, scenes=['room_0'])
        self.items = [i for i in range(150, 162) if i not in drop]
        self.invalid = set(invalid)
        self.frames_per_scene = 400

    def __len__(self):
        return len(self.items)

    def __getitem__(self, item):
        i = self.items[item]
        out = super().__getitem__(i)
        if i in self.invalid:
            out['extrinsics'] = torch.full_like(out['extrinsics'], float('inf'))
        return out

    def get_grid(self, scene, truncation, semantic_grid=True):
        from online_joint_depthfusion_and_semantic_amd.database import Voxelgrid
        st = self.streams[scene]
        g = Voxelgrid(st.resolution)
        g.from_array(_gt(truncation).copy(), st.bbox)
        return (g,)


def test_test_fusion_tracks_frames_without_poses(cuda):
    from online_joint_depthfusion_and_semantic_amd.drivers import test_fusion as run_test_fusion
    _, res, _ = synthetic.grid_spec(GRID)
    cfg = default_config(H, W)
    cfg.SETTINGS.device = str(cuda)
    pipe = Pipeline(cfg)
    last = [m for m in pipe._fusion_network.pred.modules() if isinstance(m, torch.nn.Conv2d)][-1]
    with torch.no_grad():  # the head outputs the projective distances (4 - k)·res: classic TSDF averaging
        last.weight.zero_()
        last.bias.copy_(torch.atanh(torch.tensor([(4 - k) * res for k in range(9)], dtype=torch.float32)))
    state = pipe._fusion_network.state_dict()
    invalid = (156, 157, 158)

    def run(track, **kw):
        c = default_config(H, W)
        c.SETTINGS.device = str(cuda)
        c.TESTING.track_invalid_poses = track
        return run_test_fusion(c, _Stream(**kw), cuda, state_dict=state, log=lambda *a: None)[2]
    db_on = run(True, invalid=invalid)
    db_off = run(False, invalid=invalid)
    db_never = run(False, drop=invalid)
    st = synthetic.SyntheticStream(H, W, GRID, 400)
    assert sorted(db_on.tracked_poses) == ['room_0/0/%06d' % i for i in invalid]
    errs = [track_ref.pose_error(db_on.tracked_poses['room_0/0/%06d' % i], st.frame(i)['extrinsics']) for i in invalid]
    print('tracked poses (mm, deg):', [(round(1e3 * a, 2), round(b, 4)) for a, b in errs])
    assert max(e[0] for e in errs) <= 0.005 and max(e[1] for e in errs) <= 0.2, errs
    s = 'room_0'
    w_on, w_off = db_on.fusion_weights[s].float(), db_off.fusion_weights[s].float()
    assert float(w_on.sum()) > float(w_off.sum()) and int((w_on > w_off).sum()) > 1000
    assert torch.equal(db_off.scenes_est[s].volume.view(torch.int16), db_never.scenes_est[s].volume.view(torch.int16))
    assert torch.equal(db_off.fusion_weights[s].view(torch.int16), db_never.fusion_weights[s].view(torch.int16))
