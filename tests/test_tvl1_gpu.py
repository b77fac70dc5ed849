"""-m gpu: the TV-L1 fusion (ojf_fuse_depth_hist / ojf_tvl1_solve / ojf_tvl1_write, tvl1.py, Database.integrate_depth_hist /
regularize / save, Pipeline with FUSION_MODEL.name 'tvl1') against its numpy restatement (tvl1_ref.py) bit for bit - fp16 and
fp32 bit patterns over the whole tensors, padding and unobserved voxels included - and the public layers against direct
calls."""
import os

import numpy as np
import pytest
import torch

from online_joint_depthfusion_and_semantic_amd import _lib, synthetic, tvl1
from online_joint_depthfusion_and_semantic_amd.config import default_config, database_config
from online_joint_depthfusion_and_semantic_amd.database import Database
from online_joint_depthfusion_and_semantic_amd.pipeline import Pipeline
import tvl1_ref as ref

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = F(7.25)  # what u holds where nothing may write


def _dev(a, cuda):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _bits(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize]) if a.dtype.kind == 'f' else a


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    n_bad = int((g != w).sum())
    assert n_bad == 0, '{}: {} of {} values differ'.format(what, n_bad, g.size)


def _fuse(vol, B, c, cuda, views=slice(None), mask=False, **kw):
    tvl1.integrate_depth_hist(vol, B, origin=c['origin'], resolution=c['res'], depth=_dev(c['depth'][views], cuda), intrinsics=c['K'],
                              extrinsics=c['E'][views], mask=_dev(c['mask'][views], cuda) if mask else None, truncation=c['trunc'], **kw)


# ---- 1. fusion -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', ref.SHAPES)
@pytest.mark.parametrize('B', [2, 7, 8, 15])  # 7: W is the last half of the first chunk; 8: it moves to the second
def test_fusion_bit_parity(cuda, shape, B):
    c = ref.fuse_case(shape)
    for carve in (False, True):
        for masked in (False, True):
            for max_weight in (1.0, 128.0):
                want = ref.new_volume(shape, B)
                counts = ref.fuse(want, B, c['origin'], c['res'], c['depth'], c['K'], c['E'], c['mask'] if masked else None,
                                  trunc=c['trunc'], max_weight=max_weight, carve=carve)
                got = _dev(ref.new_volume(shape, B), cuda)
                _fuse(got, B, c, cuda, mask=masked, max_weight=max_weight, carve=carve)
                _same(got, want, 'hist {} B={} carve={} mask={} max_weight={}'.format(shape, B, carve, masked, max_weight))
                assert sum(counts) > 0 and counts[4] == 0


# ---- 2. views per call -----------------------------------------------------------------------------------------------------
def test_views_per_call_do_not_change_the_bits(cuda):
    c = ref.fuse_case((16, 16, 16))
    order = [i % 4 for i in range(33)]  # (the four cameras that see the box, in turn)
    c = dict(c, depth=c['depth'][order], E=c['E'][order], mask=c['mask'][order])
    B = 9
    vols = [tvl1.new_volume((16, 16, 16), B, cuda) for _ in range(3)]
    _fuse(vols[0], B, c, cuda, mask=True, max_weight=16.0)  # 32 + 1
    for v in range(33):
        _fuse(vols[1], B, c, cuda, views=slice(v, v + 1), mask=True, max_weight=16.0)
    _fuse(vols[2], B, c, cuda, views=slice(0, 2), mask=True, max_weight=16.0)
    _fuse(vols[2], B, c, cuda, views=slice(2, 33), mask=True, max_weight=16.0)
    want = ref.new_volume((16, 16, 16), B, pad=False)
    ref.fuse(want, B, c['origin'], c['res'], c['depth'], c['K'], c['E'], c['mask'], trunc=c['trunc'], max_weight=16.0)
    assert want[..., B].max() == 16
    for vol, what in zip(vols, ('32 + 1', '33 x 1', '2 + 31')):
        _same(vol, want, what)


# ---- 3., 4. the solver -------------------------------------------------------------------------------------------------------
def _solve_gpu(vol, B, cuda, iterations, lam=2.0, **kw):
    s = tvl1.Solver(vol.shape[:3], cuda)
    s.u.fill_(float(SENTINEL))
    s.solve(_dev(vol, cuda), B, lam, iterations, **kw)
    return s


# the issue's shapes, and one voxel below, at and above the brick extents 4 x 8 x 32 (tvl1_ref.BRICK <- kTvX, kTvY, kTvZ) and the
# z group 4 (tvl1_ref.GROUP) on each axis, and a box of 2 bricks + 1 voxel on every axis
@pytest.mark.parametrize('shape', ref.SHAPES + ref.EDGE_SHAPES)
def test_solver_bit_parity_over_shapes_and_iteration_counts(cuda, shape):
    assert ref.BRICK == (4, 8, 32) and ref.GROUP == 4
    B = 9 if sum(shape) % 2 else 15  # one chunk and two
    rng = np.random.default_rng(list(shape))
    vol = ref.random_hist(shape, B, rng, 'random' if min(shape) > 1 or max(shape) > 1 else 'all')
    st = ref.State(np.full(shape, SENTINEL, F))
    done = 0
    for n in (0, 1, 2, 3, 25):  # odd and even counts: both copies of ub / p end a call
        ref.solve(st, vol, B, 2.0, n - done, restart=done == 0 and n == 0)
        done = n
        got = _solve_gpu(vol, B, cuda, n)
        _same(got.u, st.u, 'u {} after {} iterations'.format(shape, n))
    obs = ref.observed(vol, B)
    assert (st.u[~obs] == SENTINEL).all() and (np.abs(st.u[obs]) <= 1).all()


@pytest.mark.parametrize('pattern', ['none', 'all', 'checker', 'sheet', 'views'])
def test_solver_bit_parity_over_observation_patterns(cuda, pattern):
    shape, B = (9, 17, 70), 9
    if pattern == 'views':
        c = ref.fuse_case(shape)
        vol = ref.new_volume(shape, B)
        ref.fuse(vol, B, c['origin'], c['res'], c['depth'], c['K'], c['E'], c['mask'], trunc=c['trunc'])
    else:
        vol = ref.random_hist(shape, B, np.random.default_rng(8), pattern)
    obs = ref.observed(vol, B)
    st = ref.State(np.full(shape, SENTINEL, F))
    ref.solve(st, vol, B, 4.0, 12)
    got = _solve_gpu(vol, B, cuda, 12, lam=4.0)
    _same(got.u, st.u, 'u, pattern ' + pattern)
    if pattern == 'none':
        assert not obs.any() and (st.u == SENTINEL).all()
    elif pattern == 'checker':
        assert not ref.edges(obs).any() and not st.p.any()  # no edge counts: the per-voxel medians
    else:
        assert ref.edges(obs).any() and st.p.any()


# ---- 5. restart, continue, refresh ---------------------------------------------------------------------------------------------
def test_split_calls_and_refresh(cuda):
    shape, B = (9, 17, 70), 8
    vol = ref.random_hist(shape, B, np.random.default_rng(2), 'random')
    hist = _dev(vol, cuda)
    one = _solve_gpu(vol, B, cuda, 25)
    two = _solve_gpu(vol, B, cuda, 12)
    two.solve(hist, B, 2.0, 13, restart=False)
    _same(two.u, one.u, '12 + 13')
    many = _solve_gpu(vol, B, cuda, 1)
    for _ in range(24):
        many.solve(hist, B, 2.0, 1, restart=False)
    _same(many.u, one.u, '25 x 1')
    everywhere = _solve_gpu(vol, B, cuda, 25, all_bricks=True)
    _same(everywhere.u, one.u, 'all bricks listed')
    # views arrive: the voxels observed for the first time join, the others go on
    more = ref.random_hist(shape, B, np.random.default_rng(2), 'all')
    st = ref.State(np.full(shape, SENTINEL, F))
    ref.solve(st, vol, B, 2.0, 25)
    ref.solve(st, more, B, 2.0, 5, restart=False, changed=True)
    one.solve(_dev(more, cuda), B, 2.0, 5, restart=False, changed=True)
    _same(one.u, st.u, 'refresh')


# ---- 6. write ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(5, 7, 19), (1, 1, 257)])
def test_write_leaves_unobserved_voxels_alone(cuda, shape):
    B = 7
    vol = ref.random_hist(shape, B, np.random.default_rng(6), 'random')
    s = _solve_gpu(vol, B, cuda, 4)
    tsdf, wgt = np.full(shape, 0.5, np.float16), np.full(shape, 9, np.float16)
    ref.write(vol, B, s.u.cpu().numpy(), 0.1, tsdf, wgt)
    t, w = _dev(np.full(shape, 0.5, np.float16), cuda), _dev(np.full(shape, 9, np.float16), cuda)
    s.write(t, w, 0.1)
    _same(t, tsdf, 'tsdf')
    _same(w, wgt, 'weights')
    obs = ref.observed(vol, B)
    assert obs.any() and (~obs).any() and (tsdf[~obs] == 0.5).all() and (wgt[~obs] == 9).all()


# ---- 7., 8. the public layers --------------------------------------------------------------------------------------------------
H, W, GRID, FRAMES = 48, 64, 64, 6


def _room(cuda, model, **fm):
    cfg = default_config(H, W, semantics=True, model='tsdf')
    cfg.FUSION_MODEL.name = model
    cfg.SETTINGS.device = str(cuda)
    cfg.FUSION_MODEL.update(fm)
    ds = synthetic.SyntheticDataset(H, W, GRID, FRAMES, scenes=['room_0', 'room_1'])
    frames = {s: [ds.streams[s].frame(i) for i in range(FRAMES)] for s in ds.scenes}
    return cfg, ds, frames


def _direct(frames, cuda, trunc, B=9, lam=2.0, iterations=25, every=None, init=None):
    """The direct tvl1.py calls: all frames then one solve (every=None), or a warm-started solve after every ``every`` frames."""
    origin, res, _ = synthetic.grid_spec(GRID)
    hist = tvl1.new_volume((GRID,) * 3, B, cuda)
    solver = tvl1.Solver((GRID,) * 3, cuda)
    tsdf = torch.full((GRID,) * 3, trunc if init is None else init, dtype=torch.float16, device=cuda)
    wgt = torch.zeros((GRID,) * 3, dtype=torch.float16, device=cuda)
    solved = False
    for i, f in enumerate(frames):
        tvl1.integrate_depth_hist(hist, B, origin=origin, resolution=res, depth=_dev(f['tof_depth'], cuda), intrinsics=f['intrinsics'],
                                  extrinsics=f['extrinsics'], mask=_dev(f['mask'], cuda), truncation=trunc)
        if every is not None and (i + 1) % every == 0:
            solver.solve(hist, B, lam, iterations, restart=not solved, changed=True)
            solver.write(tsdf, wgt, trunc)
            solved = True
    if every is None:
        solver.solve(hist, B, lam, iterations)
        solver.write(tsdf, wgt, trunc)
    return hist, tsdf, wgt


def test_database_layers(cuda, tmp_path):
    cfg, ds, frames = _room(cuda, 'tsdf')
    fr = frames['room_0']
    trunc = cfg.DATA.init_value
    db = Database(ds, database_config(cfg))
    assert db.depth_hists == {} and 'depth_hist' not in db['room_0']
    with pytest.raises(ValueError):
        db.regularize('room_0')
    for f in fr:
        db.integrate_depth_hist('room_0', f['tof_depth'], f['intrinsics'], f['extrinsics'], mask=f['mask'])
    assert not db.state['room_0'] and not db.fusion_weights['room_0'].any()  # the volumes wait for regularize
    db.regularize('room_0')
    hist, tsdf, wgt = _direct(fr, cuda, trunc)
    assert int((wgt > 0).sum()) > 10000 and int((wgt > 0).sum()) < GRID ** 3
    _same(db.depth_hists['room_0'][0], hist, 'Database.integrate_depth_hist')
    _same(db.scenes_est['room_0'].volume, tsdf, 'Database.regularize: tsdf')
    _same(db.fusion_weights['room_0'], wgt, 'Database.regularize: weights')
    assert db.state['room_0'] and db['room_0']['depth_hist'] is db.depth_hists['room_0'][0] and 'depth_hist' not in db['room_1']
    with pytest.raises(ValueError):
        db.integrate_depth_hist('room_0', fr[0]['tof_depth'], fr[0]['intrinsics'], fr[0]['extrinsics'], n_bins=7)  # 9 bins are fixed
    vertices, faces = db.get_mesh('room_0')[:2]
    assert len(vertices) > 1000 and len(faces) > 1000
    for call in (lambda: db.resample('room_0', shape=(32, 32, 32)), lambda: db.recentre('room_0', np.zeros(3)),
                 lambda: db.merge('room_1', 'room_0'), lambda: db.merge('room_0', 'room_1')):
        with pytest.raises(ValueError, match='depth histograms'):
            call()
    db.save(str(tmp_path), 'tsdf', 'room_0')
    assert sorted(n.split('.')[1] for n in os.listdir(str(tmp_path))) == ['depth_hist', 'semantics', 'tsdf', 'weights']
    db.to_numpy()
    assert isinstance(db.depth_hists['room_0'][0], np.ndarray) and db.depth_hists['room_0'][0].dtype == np.float16
    with pytest.raises(ValueError):
        db.regularize('room_0')  # host state
    db.to_torch()
    _same(db.depth_hists['room_0'][0], hist, 'to_numpy / to_torch')
    db.regularize('room_0', restart=False)  # (the solver's state did not survive the host: a restart)
    _same(db.scenes_est['room_0'].volume, tsdf, 'regularize after to_numpy / to_torch')
    db.reset('room_0')
    assert db.depth_hists['room_0'][0].is_cuda and not db.depth_hists['room_0'][0].any() and not db.state['room_0']
    db.remove('room_0')
    assert 'room_0' not in db.depth_hists


@pytest.mark.parametrize('every', [1, 3])
def test_pipeline_tvl1_mode(cuda, every):
    """Frames through Pipeline.fuse / fuse_sequence with FUSION_MODEL.name 'tvl1' give the bits of the direct calls; the colour
    and class-distribution volumes are those of the 'tsdf' mode."""
    side = {}
    for model in ('tvl1', 'tsdf'):
        cfg, ds, frames = _room(cuda, model, fuse_color=True, fuse_label_probs=True, tvl1_every=every, tvl1_iterations=5, tvl1_lambda=3.0,
                                hist_bins=7)
        db = Database(ds, database_config(cfg))
        pipe = Pipeline(cfg).to(cuda).eval()
        batches = [ds.streams['room_0'].batch(i) for i in range(FRAMES)]
        with torch.no_grad():
            for b in batches[:2]:
                pipe.fuse(b, db, cuda)
            pipe.fuse_sequence(batches[2:], db, cuda)
            if model == 'tvl1':
                with pytest.raises(ValueError, match='tvl1'):
                    pipe.fuse_many(batches[:1], db, cuda)
                with pytest.raises(ValueError, match='tvl1'):
                    pipe.fuse_sequence(batches[:1], db, cuda, prefetch=batches[1:2])
        side[model] = (db.colors['room_0'].clone(), db.label_probs['room_0'].clone())
        if model == 'tvl1':
            init = cfg.DATA.init_value
            hist, tsdf, wgt = _direct(frames['room_0'], cuda, init, B=7, lam=3.0, iterations=5, every=every)
            _same(db.depth_hists['room_0'][0], hist, 'histograms')
            _same(db.scenes_est['room_0'].volume, tsdf, 'tsdf')
            _same(db.fusion_weights['room_0'], wgt, 'weights')
            assert int((wgt > 0).sum()) > 10000 and db.state['room_0'] and not db.ids_est['room_0'].volume.any()
    _same(side['tvl1'][0], side['tsdf'][0], 'colour volume')
    _same(side['tvl1'][1], side['tsdf'][1], 'class-distribution volume')


# ---- 9. argument errors ------------------------------------------------------------------------------------------------------
def test_argument_errors_are_value_errors(cuda):
    c = ref.fuse_case((5, 7, 19))
    vol = tvl1.new_volume((5, 7, 19), 9, cuda)
    good = dict(origin=c['origin'], resolution=c['res'], depth=_dev(c['depth'], cuda), intrinsics=c['K'], extrinsics=c['E'],
                truncation=c['trunc'])
    tvl1.integrate_depth_hist(vol, 9, **good)
    for bad in (dict(truncation=0.0), dict(max_weight=0.5), dict(near=-1.0), dict(depth=_dev(c['depth'], cuda).cpu()),
                dict(mask=torch.ones(3, 3, device=cuda)), dict(extrinsics=c['E'][:2]), dict(intrinsics=np.ones((3, 3)))):
        with pytest.raises(ValueError):
            tvl1.integrate_depth_hist(vol, 9, **dict(good, **bad))
    for v, B in ((vol, 7), (vol[..., :8], 7), (vol.cpu(), 9), (vol.float(), 9)):
        with pytest.raises(ValueError):
            tvl1.integrate_depth_hist(v, B, **good)
    s = tvl1.Solver((5, 7, 19), cuda)
    with pytest.raises(ValueError):
        s.solve(vol, 9, 2.0, 1, restart=False)  # nothing to continue from
    for bad in (dict(lam=0.0), dict(iterations=-1), dict(tau=0.3, sigma=0.3), dict(sigma=0.0)):
        with pytest.raises(ValueError):
            s.solve(vol, 9, **dict(dict(lam=2.0, iterations=1), **bad))
    with pytest.raises(ValueError):
        s.solve(tvl1.new_volume((5, 7, 20), 9, cuda), 9, 2.0, 1)
    s.solve(vol, 9, 2.0, 1)
    with pytest.raises(ValueError):
        s.solve(vol, 9, 2.0, 1, restart=False, all_bricks=True)
    t, w = torch.zeros(5, 7, 19, dtype=torch.float16, device=cuda), torch.zeros(5, 7, 19, dtype=torch.float16, device=cuda)
    with pytest.raises(ValueError):
        tvl1.Solver((5, 7, 19), cuda).write(t, w, 0.1)  # nothing solved yet
    s.write(t, w, 0.1)
    for args in ((t.float(), w, 0.1), (t, w[:4], 0.1), (t, w, 0.0), (t.cpu(), w, 0.1)):
        with pytest.raises(ValueError):
            s.write(*args)
