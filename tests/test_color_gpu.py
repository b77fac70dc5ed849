"""-m gpu: the colour volume (ojf_fuse_color / ojf_color_sample / ojf_color_render, color.py, Database.integrate_color / render /
get_mesh / save, Pipeline with FUSION_MODEL.fuse_color) against its numpy restatement (color_ref.py) bit for bit, and the public
layers against direct calls."""
import os

import numpy as np
import pytest
import torch

from online_joint_depthfusion_and_semantic_amd import _lib, mesh, synthetic
from online_joint_depthfusion_and_semantic_amd.color import integrate_color, sample_color, render_color, new_volume
from online_joint_depthfusion_and_semantic_amd.config import default_config, database_config
from online_joint_depthfusion_and_semantic_amd.database import Database
from online_joint_depthfusion_and_semantic_amd.pipeline import Pipeline
from online_joint_depthfusion_and_semantic_amd.projective import integrate_depth
from online_joint_depthfusion_and_semantic_amd.render import render_views
import color_ref as ref

pytestmark = pytest.mark.gpu


def _dev(a, cuda):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _bits(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return a.view(np.uint16) if a.dtype == np.float16 else a


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    n_bad = int((g != w).sum())
    assert n_bad == 0, '{}: {} of {} values differ'.format(what, n_bad, g.size)


def _fuse_case(vol, c, cuda, mask=None, image=None, depth=None, E=None):
    integrate_color(vol, origin=c['origin'], resolution=c['res'], image=_dev(c['image'] if image is None else image, cuda),
                    depth=_dev(c['depth'] if depth is None else depth, cuda), intrinsics=c['K'],
                    extrinsics=c['E'] if E is None else E, mask=_dev(mask, cuda), band=c['band'], max_weight=c['color_max_weight'])


# ---- 1. bit parity of integrate_color ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', ref.SHAPES)  # (5,7,19): 665 voxels, no multiple of the group of 4
@pytest.mark.parametrize('pose', ref.POSES)
def test_bit_parity_on_tiny_volumes(cuda, shape, pose):
    for masked in (False, True):
        c = ref.tiny_color_case(shape, pose)
        mask = c['mask'] if masked else None
        want = c['colors'].copy()
        n = ref.fuse(want, c['origin'], c['res'], c['image'], c['depth'], c['K'], c['E'], mask, band=c['band'],
                     max_weight=c['color_max_weight'])
        got = _dev(c['colors'], cuda)
        _fuse_case(got, c, cuda, mask)
        _same(got, want, '{} {} mask={} ({} updates)'.format(shape, pose, masked, n))


def test_bit_parity_with_a_volume_off_the_16_byte_grid(cuda):
    """A view at voxel offset 1 of a larger buffer (8 B off the 16-byte grid: the element-wise path) and at offset 0."""
    c = ref.tiny_color_case((33, 20, 70), 'oblique')
    want = c['colors'].copy()
    n = ref.fuse(want, c['origin'], c['res'], c['image'], c['depth'], c['K'], c['E'], band=c['band'], max_weight=c['color_max_weight'])
    assert n[0] >= 20
    nv = want.size // 4
    for off in (0, 1):
        buf = torch.zeros((nv + 2, 4), dtype=torch.float16, device=cuda)
        got = buf[off:off + nv].view(c['shape'] + (4,))
        got.copy_(_dev(c['colors'], cuda))
        assert got.data_ptr() % 16 == 8 * off
        _fuse_case(got, c, cuda)
        _same(got, want, 'offset {}'.format(off))
        assert not buf[:off].any() and not buf[off + nv:].any()  # nothing outside the view was written


# ---- 2. views per call ---------------------------------------------------------------------------------------------------------
def test_views_per_call_do_not_change_the_bits(cuda):
    shape = (33, 20, 70)
    cases = [ref.tiny_color_case(shape, p) for p in ref.POSES]
    c = cases[0]

    def run(images, depths, Es, masks, per_call):
        vol = _dev(c['colors'], cuda)
        for v0 in range(0, len(images), per_call):
            s = slice(v0, v0 + per_call)
            _fuse_case(vol, c, cuda, mask=masks[s], image=images[s], depth=depths[s], E=Es[s])
        return vol

    def stacked(idx, images):
        return (images, np.stack([cases[i]['depth'] for i in idx]), np.stack([cases[i]['E'] for i in idx]),
                np.stack([cases[i]['mask'] for i in idx]))
    five = stacked(range(5), np.stack([k['image'] for k in cases]))
    single = run(*five, 1)
    want = c['colors'].copy()
    ref.fuse(want, c['origin'], c['res'], five[0], five[1], c['K'], five[2], five[3], band=c['band'], max_weight=c['color_max_weight'])
    _same(single, want, 'five single calls against the reference')
    _same(run(*five, 5), single, 'five views in one call')
    # 34 views: the poses cycled, each view with an image of its own; integrate_color cuts them into 32 + 2
    rng = np.random.default_rng(11)
    many = stacked([i % 5 for i in range(34)], rng.integers(0, 256, (34,) + c['image'].shape).astype(np.uint8))
    assert 34 > _lib.COLOR_MAX_VIEWS
    once = run(*many, 34)
    _same(once, run(*many, 1), '34 views in one call against 34 calls')
    _same(run(*many, 34), once, 'repeat')
    assert (once[..., 3] == ref.MAX_WEIGHT).sum() > (single[..., 3] == ref.MAX_WEIGHT).sum()


# ---- 3. sample_color -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', ref.SHAPES)
def test_sample_color_bit_parity(cuda, shape):
    vol, pts = ref.sample_case(shape)
    assert 0.4 < (vol[..., 3] == 0).mean() < 0.6 and len(pts) > 4096
    want = ref.sample(vol, pts)
    assert 0.3 < (want[:, 3] == 255).mean() < 0.99 and not want[~np.isfinite(pts).all(axis=1)].any()
    got = sample_color(_dev(vol, cuda), _dev(pts, cuda))
    _same(got, want, 'sample_color {}'.format(shape))
    _same(sample_color(_dev(vol, cuda), pts.astype(np.float64)), want, 'host f64 points')
    # a volume off the 8-byte grid: the 2-byte loads
    buf = torch.zeros(vol.size + 1, dtype=torch.float16, device=cuda)
    off = buf[1:].view(vol.shape)
    off.copy_(_dev(vol, cuda))
    assert off.data_ptr() % 8 == 2
    _same(sample_color(off, _dev(pts, cuda)), want, 'unaligned volume')
    assert sample_color(_dev(vol, cuda), np.zeros((0, 3), np.float32)).shape == (0, 4)


# ---- 4. render_color -----------------------------------------------------------------------------------------------------------
def test_render_color_of_a_fused_sphere(cuda):
    c = ref.sphere_case()
    shape = c['shape']
    tsdf = torch.full(shape, c['trunc'], dtype=torch.float16, device=cuda)
    wgt = torch.zeros(shape, dtype=torch.float16, device=cuda)
    vol = new_volume(shape, cuda)
    kw = dict(origin=c['origin'], resolution=c['res'], depth=_dev(c['depth'], cuda), intrinsics=c['K'], extrinsics=c['E'])
    integrate_depth(tsdf, wgt, truncation=c['trunc'], **kw)
    integrate_color(vol, image=_dev(c['image'], cuda), band=c['band'], **kw)
    h, w = c['depth'].shape[1:]
    E = c['E'][:2]
    depth = render_views(tsdf, wgt, origin=c['origin'], resolution=c['res'], intrinsics=c['K'], extrinsics=E, shape=(h, w))['depth']
    got = render_color(vol, origin=c['origin'], resolution=c['res'], intrinsics=c['K'], extrinsics=E, depth=depth)
    want = ref.render_color(vol.cpu().numpy(), c['origin'], c['res'], c['K'], E, depth.cpu().numpy())
    _same(got, want, 'render_color')
    hit = depth.cpu().numpy() > 0
    assert hit.sum() > 200 and (want[..., 3][hit] == 255).mean() > 0.5
    assert not want[~hit].any()
    # depth without a value anywhere writes zeros
    bad = torch.tensor([0.0, -1.0, float('nan'), float('inf')], device=cuda).repeat(h * w // 4).view(1, h, w)
    assert not render_color(vol, origin=c['origin'], resolution=c['res'], intrinsics=c['K'], extrinsics=E[0], depth=bad).any()


# ---- 5. the public layers ------------------------------------------------------------------------------------------------------
H, W, GRID, FRAMES = 48, 64, 64, 6


def _room(cuda, model, semantics=True, fuse_color=True):
    cfg = default_config(H, W, semantics=semantics, model=model)
    cfg.SETTINGS.device = str(cuda)
    cfg.FUSION_MODEL.fuse_color = fuse_color
    ds = synthetic.SyntheticDataset(H, W, GRID, FRAMES, scenes=['room_0', 'room_1'])
    frames = {s: ref.room_frames(ds.streams[s], FRAMES) for s in ds.scenes}
    return cfg, ds, frames


def _batch(stream, frame):
    b = stream.batch(frame['item_id'])
    b['image'] = torch.from_numpy(frame['image'].astype(np.float32)).permute(2, 0, 1).unsqueeze(0).contiguous()  # [1,3,h,w], 0..255
    return b


def _direct(frames, cuda, band):
    origin, res, _ = synthetic.grid_spec(GRID)
    vol = new_volume((GRID,) * 3, cuda)
    for f in frames:
        integrate_color(vol, origin=origin, resolution=res, image=_dev(f['image'], cuda), depth=_dev(f['tof_depth'], cuda),
                        intrinsics=f['intrinsics'], extrinsics=f['extrinsics'], mask=_dev(f['mask'], cuda), band=band)
    return vol


def test_database_layers(cuda, tmp_path):
    cfg, ds, frames = _room(cuda, 'tsdf', semantics=False)
    st, fr = ds.streams['room_0'], frames['room_0']
    origin, res, _ = synthetic.grid_spec(GRID)
    db = Database(ds, database_config(cfg))
    assert db.colors == {} and 'colors' not in db['room_0']
    with pytest.raises(ValueError):
        db.render('room_0', st.K, fr[0]['extrinsics'], (H, W), color=True)
    for f in fr:
        db.integrate_depth('room_0', f['tof_depth'], f['intrinsics'], f['extrinsics'], mask=f['mask'])
        db.integrate_color('room_0', f['image'], f['tof_depth'], f['intrinsics'], f['extrinsics'], mask=f['mask'])
    want = _direct(fr, cuda, cfg.DATA.init_value)
    assert int((want[..., 3] > 0).sum()) > 1000
    _same(db.colors['room_0'], want, 'Database.integrate_color')
    assert db['room_0']['colors'] is db.colors['room_0'] and 'colors' not in db['room_1'] and list(db.colors) == ['room_0']
    # the float [3,h,w] image of a batch dict gives the same volume as the u8 image
    other = Database(ds, database_config(cfg))
    for f in fr:
        b = _batch(st, f)
        other.integrate_color('room_0', b['image'][0], f['tof_depth'], f['intrinsics'], f['extrinsics'], mask=f['mask'])
    _same(other.colors['room_0'], want, 'float image')

    E = np.stack([fr[1]['extrinsics'], fr[4]['extrinsics']])
    out = db.render('room_0', st.K, E, (H, W), color=True)
    assert out['color'].shape == (2, H, W, 4) and out['color'].dtype == torch.uint8
    _same(out['color'], render_color(want, origin=origin, resolution=res, intrinsics=st.K, extrinsics=E, depth=out['depth']), 'render')
    hit = out['depth'] > 0
    assert hit.float().mean() > 0.5 and (out['color'][..., 3][hit] == 255).float().mean() > 0.9
    assert 'color' not in db.render('room_0', st.K, E, (H, W))

    verts, faces, normals, rgb = db.get_mesh('room_0', color=True)
    base = db.get_mesh('room_0')
    assert len(verts) > 100 and np.array_equal(verts, base[0]) and np.array_equal(faces, base[1]) and base[3] is None
    sampled = sample_color(want, verts.astype(np.float32) / np.float32(res)).cpu().numpy()
    assert np.array_equal(rgb, sampled[:, :3] / 255.0) and (sampled[:, 3] == 255).mean() > 0.9

    db.save(str(tmp_path), 'test', 'room_0')
    names = sorted(os.listdir(str(tmp_path)))
    assert 'room_0.ply' in names and 'room_0_color.ply' in names and any(n.startswith('room_0.color.') for n in names), names
    coloured, bare = mesh.load_ply(str(tmp_path / 'room_0_color.ply')), mesh.load_ply(str(tmp_path / 'room_0.ply'))
    assert len(coloured['vertices']) == len(bare['vertices']) == len(verts) and np.array_equal(coloured['rgba'], sampled)
    os.makedirs(str(tmp_path / 'tsdf'))
    db.save(str(tmp_path / 'tsdf'), 'tsdf', 'room_0')
    assert sorted(n.split('.')[1] for n in os.listdir(str(tmp_path / 'tsdf'))) == ['color', 'tsdf', 'weights']

    db.to_numpy()
    assert isinstance(db.colors['room_0'], np.ndarray) and db.colors['room_0'].dtype == np.float16
    db.to_torch()
    _same(db.colors['room_0'], want, 'to_numpy / to_torch')
    db.reset('room_0')
    assert db.colors['room_0'].is_cuda and not db.colors['room_0'].any() and not db.state['room_0']
    db.remove('room_0')
    assert 'room_0' not in db.colors


@pytest.mark.parametrize('model', ['tsdf', 'v3'])
def test_pipeline_fuses_colour_and_leaves_the_other_volumes_alone(cuda, model):
    """fuse, fuse_sequence and fuse_many (two scenes) with FUSION_MODEL.fuse_color: the colour volumes of direct calls, and the
    TSDF / weight / id / score volumes of a run without it."""
    vols = {}
    for fuse_color in (True, False):
        cfg, ds, frames = _room(cuda, model, fuse_color=fuse_color)
        assert default_config().FUSION_MODEL.fuse_color is False and cfg.FUSION_MODEL.color_band == cfg.DATA.init_value
        db = Database(ds, database_config(cfg))
        torch.manual_seed(3)
        pipe = Pipeline(cfg).to(cuda).eval()
        batches = {s: [_batch(ds.streams[s], f) for f in frames[s]] for s in ds.scenes}

        def snapshot(stage):
            for s in ds.scenes:
                vols[(fuse_color, stage, s)] = [v.clone() for v in (db.scenes_est[s].volume, db.fusion_weights[s], db.ids_est[s].volume,
                                                                    db.scores[s].volume)] + [db.colors[s].clone() if s in db.colors else None]
        with torch.no_grad():
            for b in batches['room_0']:
                pipe.fuse(b, db, cuda)
            snapshot('fuse')
            db.reset()
            pipe.fuse_sequence(batches['room_0'][:4] + batches['room_1'][:2] + batches['room_0'][4:], db, cuda)
            snapshot('fuse_sequence')
            db.reset()
            for a, b in zip(batches['room_0'], batches['room_1']):
                pipe.fuse_many([a, b], db, cuda)
            snapshot('fuse_many')
        pipe.check()
    band = default_config().DATA.init_value
    want = {s: _direct(frames[s], cuda, band) for s in ('room_0', 'room_1')}
    want_two = _direct(frames['room_1'][:2], cuda, band)
    assert int((want['room_0'][..., 3] > 0).sum()) > 1000
    for stage, scenes in (('fuse', {'room_0': want['room_0']}), ('fuse_sequence', {'room_0': want['room_0'], 'room_1': want_two}),
                          ('fuse_many', want)):
        for s in ('room_0', 'room_1'):
            on, off = vols[(True, stage, s)], vols[(False, stage, s)]
            if s in scenes:
                _same(on[4], scenes[s], '{} {}: colour volume'.format(stage, s))
            else:
                assert on[4] is None or not on[4].any()
            assert off[4] is None
            for name, a, b in zip(('tsdf', 'weights', 'ids', 'scores'), on, off):
                _same(a, b, '{} {}: {} with and without fuse_color'.format(stage, s, name))
        assert (vols[(True, stage, 'room_0')][1] > 0).sum() > 1000


# ---- 6. argument errors ----------------------------------------------------------------------------------------------------------
def test_argument_errors_are_value_errors(cuda):
    vol = new_volume((8, 8, 8), cuda)
    d = torch.full((4, 4), 0.5, device=cuda)  # (voxels k = 4, 5 of the 0.1-m grid lie within the band of it)
    img = torch.full((4, 4, 3), 200, dtype=torch.uint8, device=cuda)
    K, E = np.array([[4.0, 0, 2], [0, 4.0, 2], [0, 0, 1]]), np.eye(4)
    kw = dict(origin=np.zeros(3), resolution=0.1, image=img, depth=d, intrinsics=K, extrinsics=E, band=0.1)
    skew = K.copy()
    skew[0, 1] = 0.1
    bad = [dict(kw, depth=d.cpu()), dict(kw, image=img.cpu()), dict(kw, image=img[:3]), dict(kw, image=img.to(torch.int32)),
           dict(kw, image=torch.zeros((2, 4, 4), device=cuda)), dict(kw, image=torch.zeros((4, 4, 5), dtype=torch.uint8, device=cuda)),
           dict(kw, intrinsics=np.stack([K] * 3)), dict(kw, intrinsics=skew), dict(kw, extrinsics=np.full((3, 4), np.nan)),
           dict(kw, band=0.0), dict(kw, band=float('inf')), dict(kw, max_weight=0.5), dict(kw, max_weight=4096), dict(kw, near=-1.0),
           dict(kw, mask=torch.ones(5, dtype=torch.bool, device=cuda)), dict(kw, depth=torch.ones((0, 4, 4), device=cuda))]
    for case in bad:
        with pytest.raises(ValueError):
            integrate_color(vol, **case)
    for wrong in (vol.float(), vol[..., :3], vol[:, :, ::2], vol.cpu(), vol.view(8, 8, 32)):
        with pytest.raises(ValueError):
            integrate_color(wrong, **kw)
        with pytest.raises(ValueError):
            sample_color(wrong, np.zeros((4, 3), np.float32))
        with pytest.raises(ValueError):
            render_color(wrong, origin=np.zeros(3), resolution=0.1, intrinsics=K, extrinsics=E, depth=d)
    assert not vol.any()
    for pts in (np.zeros((4, 2), np.float32), np.zeros(3, np.float32), np.zeros((4, 3), np.int64)):
        with pytest.raises(ValueError):
            sample_color(vol, pts)
    rk = dict(origin=np.zeros(3), resolution=0.1, intrinsics=K, extrinsics=E, depth=d)
    for case in (dict(rk, depth=d.cpu()), dict(rk, depth=torch.ones((2, 4, 4), device=cuda)), dict(rk, extrinsics=np.zeros((3, 3))),
                 dict(rk, depth=torch.ones((4,), device=cuda))):
        with pytest.raises(ValueError):
            render_color(vol, **case)
    integrate_color(vol, **kw)  # the well-formed call is what works
    assert vol.any()
