"""CPU: the numpy restatement of joint geometric + photometric tracking (track_rgbd_ref.py) on its own: the textured plane
that depth alone cannot track, photo_weight 0 as the depth-only tracker bit for bit, and frame pairs of the synthetic room
with analytic colour.  The GPU tests (test_track_rgbd_gpu.py) pin the kernels to this restatement."""
import functools

import numpy as np

from online_joint_depthfusion_and_semantic_amd import synthetic
import color_ref
import track_ref
import track_rgbd_ref as ref

# Measured once with the restatement at the defaults (photo_weight 0.002, photo_thresh 40, levels 3, iterations (10, 5, 4)):
# render_ref.plane_case(64)'s plane at 48x64 painted with color_ref.analytic_color, live frame at the case's pose, analytic
# model images at the start; (translation m, rotation deg) after the call from PLANE_STARTS[0..2]
PLANE_ERRORS = ((0.000157, 0.00867), (0.000307, 0.00764), (0.000205, 0.00688))
# the smallest Cholesky pivot over the solve's threshold 1e-6 max diag, over all 19 steps, per start (>= 100 is the
# condition on the default weight)
PLANE_MARGIN = (673.0, 513.0, 914.0)
# SyntheticStream(48, 64, 64, 400) pairs (i, i+1) with color_ref.room_frames images, the model analytic at frame i, 5 mm
# ToF noise on the live depth; start = frame i's pose, perturbed as ROOM_STARTS; (rgbd m, deg, depth-only status, m, deg)
ROOM_PAIRS = (20, 35, 53, 47)
ROOM_STARTS = (None, (3.0, 0.05, (1, 0, 0), (0, 1, 0)), (3.0, 0.0, (0, 1, 0), (1, 0, 0)), (2.0, 0.04, (1, -1, 0.5), (-1, 0, 1)))
ROOM_ERRORS = ((0.000325, 0.0339, 2, None, None), (0.000537, 0.0167, 0, 0.000535, 0.0164),
               (0.000379, 0.0089, 0, 0.000373, 0.0128), (0.000822, 0.0347, 0, 0.000885, 0.0394))


@functools.lru_cache(maxsize=None)
def _room():
    st = synthetic.SyntheticStream(48, 64, 64, 400)
    return st, color_ref.room_frames(st, max(ROOM_PAIRS) + 2)


def test_the_textured_plane_is_tracked():
    for s in range(3):
        case = ref.plane_tracking_case(s)
        _, status, _ = ref.run_depth_only(case)
        assert status[0] == 2, (s, status)  # geometry alone: a singular system
        trace = []
        P, status, stats = ref.run_case(case, trace=trace)
        dt, dr = track_ref.pose_error(P, case['E_true'])
        margin = min(t['margin'] for t in trace)
        start = track_ref.pose_error(case['E_init'], case['E_true'])
        print('plane start %d (%.1f mm, %.2f deg): status %s, %.4f mm, %.5f deg, pivot margin %.0f' % (
            s, 1e3 * start[0], start[1], status, 1e3 * dt, dr, margin))
        assert status == (0, -1) and len(trace) == 19, (s, status)
        assert dt <= 1.5 * PLANE_ERRORS[s][0] and dr <= 1.5 * PLANE_ERRORS[s][1], (s, dt, dr)
        assert margin >= 100.0 and margin >= PLANE_MARGIN[s] / 1.5, (s, margin)
        # every photometric path the case is meant to take
        assert all((t['preason'] == 0).mean() > 0.5 for t in trace), s
        assert any((t['preason'] == 8).any() for t in trace), s


def test_weight_zero_is_the_depth_only_tracker():
    st, frames = _room()
    case = ref.room_tracking_case(st, frames, ROOM_PAIRS[2], ROOM_STARTS[2])
    a = ref.run_case(case, photo_weight=0.0)
    b = ref.run_depth_only(case)
    assert a[1] == b[1] == (0, -1)
    assert a[0].tobytes() == b[0].tobytes() and a[2].tobytes() == b[2].tobytes()
    assert not np.array_equal(ref.run_case(case)[0], b[0])


def test_room_pairs_with_colour():
    st, frames = _room()
    for k, (i, start) in enumerate(zip(ROOM_PAIRS, ROOM_STARTS)):
        case = ref.room_tracking_case(st, frames, i, start)
        P, status, _ = ref.run_case(case)
        Pd, status_d, _ = ref.run_depth_only(case)
        e, ed = track_ref.pose_error(P, case['E_true']), track_ref.pose_error(Pd, case['E_true'])
        print('room pair %d: rgbd status %s %.4f mm %.5f deg | depth only status %s %.4f mm %.5f deg' % (
            i, status, 1e3 * e[0], e[1], status_d, 1e3 * ed[0], ed[1]))
        if status_d[0] == 0:
            assert status[0] == 0, (i, status)
        assert status[0] == 0, (i, status)
        assert ROOM_ERRORS[k][2] == status_d[0], (i, status_d)
        assert e[0] <= 1.5 * ROOM_ERRORS[k][0] and e[1] <= 1.5 * ROOM_ERRORS[k][1], (i, e)


def test_hostile_cases_take_every_path():
    """What test_track_rgbd_gpu.py relies on, shown on the restatement: at level 0 of each of its shapes every photometric
    reason but the cut occurs (the cut is placed by the test itself), rows are added without a normal, and live pixels land on
    the outermost model rows and columns without getting a row."""
    for h, w, levels in ((32, 32, 1), (25, 41, 1), (64, 64, 4), (67, 93, 3)):
        case = ref.hostile_case(h, w, levels)
        D = track_ref.pyramid(case['depth'], case['mask'], 1)[0]
        I = ref.intensity_pyramid(case['image'], 1)[0]
        mmap = ref.model_map(case['mcolor'][0], case['mdepth'][0], 0.1)
        a = ref.associate(D, I, case['Kinv'][0], case['K'], 0, case['mdepth'][0], case['mnormal'][0], mmap, case['E_ref'],
                          case['pose'], photo_thresh=1e9)
        c = np.bincount(a['preason'].reshape(-1), minlength=11)
        assert all(c[k] > 0 for k in (0, 1, 3, 4, 5, 6, 8)) and c[9] == 0, (h, w, c)
        assert (a['reason'][a['preason'] == 0] == 2).any(), (h, w)
        rim = (a['mrow'] == 0) | (a['mrow'] == h - 1) | (a['mcol'] == 0) | (a['mcol'] == w - 1)
        assert (rim & (a['preason'] == 8)).any() and not (rim & (a['preason'] == 0)).any(), (h, w)
        assert (np.isnan(case['depth'])).any() and (case['mask'] == 0).any()


def test_the_driver_passes_the_image_only_when_asked():
    """drivers._tracked_batch hands the batch's image to Database.track with TESTING.track_with_color, and None without."""
    import torch
    from online_joint_depthfusion_and_semantic_amd.config import default_config
    from online_joint_depthfusion_and_semantic_amd.drivers import _tracked_batch

    class Db:
        tracked_poses = {}

        def track(self, scene, depth, K, E0, **kw):
            self.kw = kw
            return {'ok': True, 'status': 0, 'extrinsics': np.eye(4)}
    cfg = default_config(48, 64)
    assert cfg.TESTING.track_with_color is False
    batch = {'frame_id': ['room_0/0/000007'], cfg.DATA.input: torch.zeros(1, 48, 64), 'mask': torch.ones(1, 48, 64),
             'image': torch.full((1, 3, 48, 64), 7.0), 'intrinsics': torch.eye(3)[None], 'extrinsics': torch.full((1, 3, 4), float('inf'))}
    for on in (False, True):
        cfg.TESTING.track_with_color = on
        db = Db()
        out = _tracked_batch(batch, db, cfg, {'room_0': np.eye(4)}, lambda *a: None)
        assert out is not None and torch.isfinite(out['extrinsics']).all()
        assert (db.kw['image'] is batch['image'][0] or torch.equal(db.kw['image'], batch['image'][0])) if on else db.kw['image'] is None
