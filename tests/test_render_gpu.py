"""-m gpu: the ray caster (ojf_render, render.render_views, Database.render) against its fp32 numpy restatement
(render_ref.py: depth and labels bit for bit, normals within 1e-6) and against analytic scenes."""
import numpy as np
import pytest
import torch

from online_joint_depthfusion_and_semantic_amd import synthetic
from online_joint_depthfusion_and_semantic_amd.config import default_config, database_config
from online_joint_depthfusion_and_semantic_amd.database import Database
from online_joint_depthfusion_and_semantic_amd.pipeline import Pipeline
from online_joint_depthfusion_and_semantic_amd.render import render_views
from render_ref import plane_case, render_ref

pytestmark = pytest.mark.gpu


def _host(out):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint8).reshape(got.size, -1) != want.view(np.uint8).reshape(want.size, -1)
    n_bad = int(bad.any(axis=1).sum())
    if n_bad:
        diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
        pytest.fail('{}: {} of {} elements differ (max |diff| {:.3e})'.format(what, n_bad, got.size, diff.max()))


def _check_against_ref(out, tsdf, weights, ids, origin, res, K, E, shape, near=0.0):
    depth, normals, labels = render_ref(tsdf, weights, ids, origin, res, K, E, shape, near)
    got = _host(out)
    _same_bits(got['depth'], depth, 'depth')
    if ids is not None:
        _same_bits(got['labels'], labels, 'labels')
    if got['normals'] is not None:
        assert np.abs(got['normals'] - normals).max() <= 1e-6
    return depth, normals, labels


def _dev(a, cuda):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _orbit(ts):
    return np.stack([synthetic.camera_pose(t) for t in ts])


def _fused(cuda, h=48, w=64, grid=64, frames=6):
    """Pipeline.fuse of a SyntheticStream (semantics 'gt'): a volume with real holes."""
    cfg = default_config(h, w, semantics=True, use_semantics=True)
    cfg.SETTINGS.device = str(cuda)
    st = synthetic.SyntheticStream(h, w, grid, frames)
    db = Database(st, database_config(cfg))
    torch.manual_seed(3)
    pipe = Pipeline(cfg)
    for m in pipe._fusion_network.modules():
        if isinstance(m, torch.nn.Conv2d):
            torch.nn.init.xavier_normal_(m.weight)
    pipe = pipe.to(cuda).eval()
    with torch.no_grad():
        for i in range(frames):
            b = {k: (v.to(cuda) if torch.is_tensor(v) else v) for k, v in st.batch(i).items()}
            pipe.fuse(b, db, cuda)
    torch.cuda.synchronize()
    return st, db


def test_restatement_parity_on_gt_volume(cuda):
    h, w, grid = 48, 64, 64
    tsdf, ids = synthetic.gt_volumes(grid)
    origin, res, _ = synthetic.grid_spec(grid)
    K, E = synthetic.intrinsics(h, w), _orbit([0.3, 2.0, 4.1])
    out = render_views(_dev(tsdf, cuda), None, _dev(ids, cuda), origin=origin, resolution=res, intrinsics=K,
                       extrinsics=E, shape=(h, w))
    depth, _, labels = _check_against_ref(out, tsdf, None, ids, origin, res, K, E, (h, w))
    assert (depth > 0).mean() > 0.99 and (labels > 0).mean() > 0.9


def test_restatement_parity_on_fused_volume(cuda):
    h, w = 48, 64
    st, db = _fused(cuda, h, w)
    s = st.scene
    tsdf, wgt, ids = db.scenes_est[s].volume, db.fusion_weights[s], db.ids_est[s].volume
    K = st.frame(0)['intrinsics']
    hits = []
    # a fused pose (frames orbit t = 0 .. 0.79), an unseen one further along the orbit that sees part of the fused surface
    for E in (st.frame(3)['extrinsics'], synthetic.camera_pose(1.0)):
        out = render_views(tsdf, wgt, ids, origin=db.origin[s], resolution=db.resolution[s], intrinsics=K, extrinsics=E,
                           shape=(h, w))
        depth, _, _ = _check_against_ref(out, tsdf.cpu().numpy(), wgt.cpu().numpy(), ids.cpu().numpy(), db.origin[s],
                                         db.resolution[s], K, E, (h, w))
        hits.append((depth > 0).mean())
    assert hits[0] > 0.9 and 0.2 < hits[1] < 0.99, hits  # the unseen pose looks into holes


def test_analytic_room_256(cuda):
    h, w, grid = 240, 320, 256
    tsdf, ids = synthetic.gt_volumes(grid)
    origin, res, _ = synthetic.grid_spec(grid)
    K, E = synthetic.intrinsics(h, w), _orbit([0.4, 1.9, 3.3, 5.2])
    out = render_views(_dev(tsdf, cuda), None, _dev(ids, cuda), origin=origin, resolution=res, intrinsics=K,
                       extrinsics=E, shape=(h, w))
    depth = out['depth'].cpu().numpy().astype(np.float64)
    want = np.stack([synthetic._raycast(E[i], K, h, w)[0] for i in range(len(E))])
    hit = depth > 0
    err = np.abs(depth - want)
    assert hit.mean() >= 0.999, hit.mean()
    assert (hit & (err <= 0.5 * res)).mean() >= 0.99, (hit & (err <= 0.5 * res)).mean()
    assert np.median(err[hit]) <= 0.01 * res, np.median(err[hit])


def test_plane_depth_and_normals(cuda):
    tsdf, origin, res, K, E, want, normal = plane_case(128)
    h, w = want.shape
    out = render_views(_dev(tsdf, cuda), origin=origin, resolution=res, intrinsics=K, extrinsics=E, shape=(h, w))
    depth, _, _ = _check_against_ref(out, tsdf, None, None, origin, res, K, E, (h, w))
    assert out['labels'] is None
    assert np.abs(depth[0] - want).max() <= 1e-3 * res
    assert np.abs(out['normals'][0].cpu().numpy() - normal).max() <= 1e-3


def test_unobserved_voxels_are_transparent(cuda):
    """A sheet (solid between z = 2.2 and 2.5) above the tilted plane of plane_case: with the sheet's slab unobserved
    the rays pass it and hit the plane, without weights they hit the sheet's top at z-depth 1.0."""
    grid = 64
    tsdf_p, origin, res, K, E, want, _ = plane_case(grid)
    z = (np.arange(grid) + 0.5) * res
    sheet = np.maximum(z - 2.5, 2.2 - z)
    sdf = np.minimum(tsdf_p.astype(np.float64), np.clip(sheet, -4 * res, 4 * res)[None, None, :])
    tsdf = sdf.astype(np.float16)
    wgt = np.ones_like(tsdf)
    wgt[:, :, (z > 2.0) & (z < 2.7)] = 0
    h, w = want.shape
    t, wd = _dev(tsdf, cuda), _dev(wgt, cuda)
    seen = render_views(t, wd, origin=origin, resolution=res, intrinsics=K, extrinsics=E, shape=(h, w))
    depth, _, _ = _check_against_ref(seen, tsdf, wgt, None, origin, res, K, E, (h, w))
    assert (depth > 0).all() and np.abs(depth[0] - want).max() <= 0.5 * res
    raw = render_views(t, None, origin=origin, resolution=res, intrinsics=K, extrinsics=E, shape=(h, w))
    depth, _, _ = _check_against_ref(raw, tsdf, None, None, origin, res, K, E, (h, w))
    assert np.abs(depth - 1.0).max() <= 0.5 * res


def test_cameras_outside_the_volume(cuda):
    grid = 64
    tsdf, origin, res, K, _, _, _ = plane_case(grid)
    h, w = 48, 64
    K = K.copy()
    K[0, 0] = K[1, 1] = 2 * w  # narrow enough that every ray meets the plane inside the 4-m cube
    ids = np.full(tsdf.shape, 9, np.uint8)
    t, i = _dev(tsdf, cuda), _dev(ids, cuda)
    # above the cube (z = 5 > 4) looking down: the rays enter through the top face
    E_in = np.array([[1.0, 0.0, 0.0, 2.0], [0.0, -1.0, 0.0, 2.0], [0.0, 0.0, -1.0, 5.0]])
    out = render_views(t, None, i, origin=origin, resolution=res, intrinsics=K, extrinsics=E_in, shape=(h, w))
    depth, _, labels = _check_against_ref(out, tsdf, None, ids, origin, res, K, E_in, (h, w))
    r = np.arange(h, dtype=np.float64)[:, None] + np.zeros((1, w))
    want = 3.5 / (1.0 + 0.5 * (r - h / 2.0) / (2 * w))
    assert np.abs(depth[0] - want).max() <= 1e-3 * res and (labels == 9).all()
    # same place looking up, away from the cube: every pixel is a miss
    E_out = np.array([[1.0, 0.0, 0.0, 2.0], [0.0, 1.0, 0.0, 2.0], [0.0, 0.0, 1.0, 5.0]])
    out = render_views(t, None, i, origin=origin, resolution=res, intrinsics=K, extrinsics=E_out, shape=(h, w))
    for k, v in _host(out).items():
        assert not v.any(), k


def test_batched_views_equal_single_views_and_repeat(cuda):
    h, w, grid = 48, 64, 64
    tsdf, ids = synthetic.gt_volumes(grid)
    wgt = np.ones_like(tsdf)
    wgt[20:30] = 0
    origin, res, _ = synthetic.grid_spec(grid)
    K = torch.from_numpy(synthetic.intrinsics(h, w)).float()
    t, wd, i = _dev(tsdf, cuda), _dev(wgt, cuda), _dev(ids, cuda)
    for n in (8, 40):  # 40: more views than one launch carries
        E = torch.from_numpy(_orbit(np.linspace(0.0, 6.0, n)))
        kw = dict(origin=origin, resolution=res, intrinsics=K.expand(n, 3, 3), extrinsics=E, shape=(h, w))
        a = _host(render_views(t, wd, i, **kw))
        b = _host(render_views(t, wd, i, **kw))
        for k in a:
            _same_bits(a[k], b[k], 'repeat ' + k)
        for v in range(n):
            one = _host(render_views(t, wd, i, origin=origin, resolution=res, intrinsics=K, extrinsics=E[v], shape=(h, w)))
            for k in a:
                _same_bits(a[k][v], one[k][0], 'view {} of {}: {}'.format(v, n, k))
        assert (a['depth'] > 0).mean() > 0.5


def test_database_render(cuda):
    h, w = 48, 64
    st, db = _fused(cuda, h, w, frames=4)
    s = st.scene
    f = st.batch(2)
    K, E = f['intrinsics'], f['extrinsics']
    direct = _host(render_views(db.scenes_est[s].volume, db.fusion_weights[s], db.ids_est[s].volume, origin=db.origin[s],
                                resolution=db.resolution[s], intrinsics=K, extrinsics=E, shape=(h, w)))
    resident = _host(db.render(s, K, E, (h, w), semantics=True))
    plain = _host(db.render(s, K, E, (h, w)))
    assert plain['labels'] is None
    db.to_numpy()
    host = _host(db.render(s, K, E, (h, w), semantics=True))
    for k in ('depth', 'normals', 'labels'):
        _same_bits(resident[k], direct[k], 'resident ' + k)
        _same_bits(host[k], direct[k], 'to_numpy ' + k)
    _same_bits(plain['depth'], direct['depth'], 'no semantics depth')
    hit = direct['depth'] > 0
    assert hit.mean() > 0.5 and (direct['labels'][hit] > 0).any()
