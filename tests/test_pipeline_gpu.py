"""-m gpu: Pipeline.fuse / fuse_training (the drop-in boundary) on the HIP path against
 (a) golden volumes produced by the reference's own Pipeline.fuse (tests/golden/make_golden.py),
 (b) the CPU oracle frame step at config A, including the reference's volume metrics.
Stated tolerances: semantic ids/scores and (parity mode) weights bit-exact; against the reference's golden volumes
|dTSDF| <= 6.2e-5 (one fp16 ulp of the top binade of the +-0.1 band) on <= 1 % of the touched voxels (the HIP net
differs from the CPU net by < 1e-6 in tsdf_est, which can move the fp16 rounding of U/W by one step; FAST mode has its
own single-ulp budget); over a six-frame stream against the oracle <= 2 ulps; metrics within 1e-3 relative."""
import numpy as np
import pytest
import torch

from online_joint_depthfusion_and_semantic_amd.config import default_config, database_config
from online_joint_depthfusion_and_semantic_amd.database import Database
from online_joint_depthfusion_and_semantic_amd.pipeline import Pipeline
from online_joint_depthfusion_and_semantic_amd import metrics
from helpers import (n_mismatch, f16_ulp_distance, golden, net_from_golden, oracle_fuse, fresh_volumes, make_stream)

pytestmark = pytest.mark.gpu
# 2 fp16 ulps at the top of the +-0.1 truncation band (ulp(0.0625..0.125) = 6.1e-5)
TSDF_ABS_TOL = 1.25e-4
# against the reference's own volumes, frame by frame: one ulp of the band's top binade (measured max 6.1e-5) on at
# most 1 % of the touched voxels (measured <= 0.63 %)
GOLDEN_ABS_TOL = 6.2e-5
TSDF_MOVED_FRACTION = 0.01


def _setup(h, w, grid, sem, use_sem, mode, cuda, state=None):
    cfg = default_config(h, w, semantics=sem, use_semantics=use_sem, integrate_mode=mode)
    cfg.SETTINGS.device = str(cuda)
    st = make_stream(h, w, grid)
    db = Database(st, database_config(cfg))
    pipe = Pipeline(cfg)
    if state is not None:
        pipe._fusion_network.load_state_dict(state)
    pipe = pipe.to(cuda).eval()
    return cfg, st, db, pipe


def _batch(st, i, cuda, to_device=True):
    b = st.batch(i)
    if to_device:  # like utils/transform.to_device in the reference drivers
        b = {k: (v.to(cuda) if torch.is_tensor(v) else v) for k, v in b.items()}
    return b


@pytest.mark.parametrize('mode', ['fast', 'parity'])
@pytest.mark.parametrize('use_sem', [True, False])
def test_fuse_matches_reference_pipeline_golden(cuda, use_sem, mode):
    g = golden('pipeline_v3_%s_24x32_g32.npz' % ('sem' if use_sem else 'nosem'))
    h, w, grid = 24, 32, 32
    state = {k[len('state_'):]: torch.from_numpy(g[k]) for k in g.files if k.startswith('state_')}
    cfg, st, db, pipe = _setup(h, w, grid, True, use_sem, mode, cuda, state)
    with torch.no_grad():
        for i in range(3):
            pipe.fuse(_batch(st, i, cuda, to_device=(i % 2 == 0)), db, cuda)
            s = st.scene
            got = dict(tsdf=db.scenes_est[s].volume, wgt=db.fusion_weights[s], ids=db.ids_est[s].volume,
                       scores=db.scores[s].volume)
            got = {k: v.cpu().numpy() for k, v in got.items()}
            assert n_mismatch(got['ids'], g['f%d_ids' % i]) == 0, i
            assert n_mismatch(got['scores'], g['f%d_scores' % i]) == 0, i
            wd = f16_ulp_distance(got['wgt'], g['f%d_wgt' % i])
            touched = int((g['f%d_wgt' % i] > 0).sum())
            # the weight path never sees the net: PARITY reproduces the reference bit for bit on every frame; FAST
            # rounds the per-voxel sum once instead of after every add (<= 1 fp16 ulp on a few voxels)
            assert wd.max() <= (0 if mode == 'parity' else 1), (i, int(wd.max()))
            assert (wd > 0).sum() <= 0.002 * touched, (i, int((wd > 0).sum()), touched)
            nan_eq = np.isnan(got['tsdf']) == np.isnan(g['f%d_tsdf' % i])
            assert nan_eq.all()
            td = np.nan_to_num(np.abs(got['tsdf'].astype(np.float32) - g['f%d_tsdf' % i].astype(np.float32)))
            print('golden 24x32 sem=%s %s frame %d: max |dTSDF| %.2e, %d of %d touched voxels differ, %d weight ulps'
                  % (use_sem, mode, i, float(td.max()), int((td > 0).sum()), touched, int((wd > 0).sum())))
            assert td.max() <= GOLDEN_ABS_TOL, (i, float(td.max()))
            assert (td > 0).sum() <= TSDF_MOVED_FRACTION * touched, (i, int((td > 0).sum()), touched)
    assert db.state[st.scene] is True


def test_fuse_training_matches_reference_golden(cuda):
    g = golden('pipeline_v3_nosem_24x32_g32.npz')
    h, w, grid = 24, 32, 32
    state = {k[len('state_'):]: torch.from_numpy(g[k]) for k in g.files if k.startswith('state_')}
    cfg, st, db, pipe = _setup(h, w, grid, True, False, 'parity', cuda, state)
    s = st.scene
    # start from the reference's state after 3 frames, then one training frame (eval-mode BN like the fixture)
    db.scenes_est[s].volume.copy_(torch.from_numpy(g['f2_tsdf']))
    db.fusion_weights[s].copy_(torch.from_numpy(g['f2_wgt']))
    out = pipe.fuse_training(_batch(st, 3, cuda), db, cuda)
    assert out['tsdf_fused'].requires_grad
    for k in ('tsdf_est', 'tsdf_fused', 'tsdf_target'):
        a, b = out[k].detach()[0].cpu().numpy(), g['train_' + k]
        assert a.shape == b.shape, (k, a.shape, b.shape)
        assert np.abs(a - b).max() <= (0 if k == 'tsdf_target' else 2e-5), (k, float(np.abs(a - b).max()))
    wd = f16_ulp_distance(db.fusion_weights[s].cpu().numpy(), g['train_wgt'])
    assert wd.max() == 0
    got = db.scenes_est[s].volume.cpu().numpy()
    td = np.nan_to_num(np.abs(got.astype(np.float32) - g['train_tsdf'].astype(np.float32)))
    assert td.max() <= TSDF_ABS_TOL
    out['tsdf_fused'].sum().backward()  # gradients reach the net's parameters
    assert any(p.grad is not None and p.grad.abs().sum() > 0 for p in pipe._fusion_network.parameters())


@pytest.mark.parametrize('sem', [False, True])
def test_stream_config_A_against_oracle(cuda, sem):
    h, w, grid, frames = 120, 160, 64, 6
    cfg, st, db, pipe = _setup(h, w, grid, sem, sem, 'fast', cuda)
    torch.manual_seed(5)
    for m in pipe._fusion_network.modules():
        if isinstance(m, torch.nn.Conv2d):
            torch.nn.init.xavier_normal_(m.weight)
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    import copy
    cpu_net = copy.deepcopy(pipe._fusion_network).cpu().eval()
    vols = fresh_volumes(grid, True)
    with torch.no_grad():
        for i in range(frames):
            pipe.fuse(_batch(st, i, cuda), db, cuda)
            oracle_fuse(st, i, vols, cpu_net, sem)
    s = st.scene
    got_t, got_w = db.scenes_est[s].volume.cpu().numpy(), db.fusion_weights[s].cpu().numpy()
    wd = f16_ulp_distance(got_w, vols['wgt'])
    assert wd.max() <= 1
    nan = np.isnan(got_t) | np.isnan(vols['tsdf'])
    assert (np.isnan(got_t) == np.isnan(vols['tsdf'])).all()
    td = np.where(nan, 0, np.abs(got_t.astype(np.float32) - vols['tsdf'].astype(np.float32)))
    assert np.percentile(td[vols['wgt'] > 0], 99) <= 6.2e-5 and td.max() <= 2 * TSDF_ABS_TOL, float(td.max())
    if sem:
        assert n_mismatch(db.ids_est[s].volume.cpu().numpy(), vols['ids']) == 0
        assert n_mismatch(db.scores[s].volume.cpu().numpy(), vols['scores']) == 0
    # the on-device evaluate kernel == the reference's metric formulas (utils/metrics.py) on the same volumes
    gt = db.scenes_gt[s].volume.cpu().numpy()
    have = db.evaluate(mode='val')
    same = metrics.evaluation(got_t, gt, got_w > 0)
    for k in same:
        assert abs(same[k] - have[k]) <= 1e-6 * max(1.0, abs(same[k])), (k, same[k], have[k])
    # metric parity with the oracle's volumes: a handful of near-zero TSDF values may change sign
    want = metrics.evaluation(vols['tsdf'], gt, vols['wgt'] > 0)
    for k in want:
        assert abs(want[k] - have[k]) <= 1e-3 * max(1.0, abs(want[k])), (k, want[k], have[k])
    # reconstruction F-score (the engine's own definition, metrics.py) is equal on oracle and HIP volumes
    f_have = metrics.reconstruction_f_score(got_t, gt, got_w, st.origin, st.resolution)
    f_want = metrics.reconstruction_f_score(vols['tsdf'], gt, vols['wgt'], st.origin, st.resolution)
    assert abs(f_have['fscore'] - f_want['fscore']) <= 1e-3 and f_want['fscore'] > 0.05, (f_have, f_want)
    f_dev = metrics.reconstruction_f_score(db.scenes_est[s].volume, db.scenes_gt[s].volume, db.fusion_weights[s],
                                           st.origin, st.resolution)  # volumes on the device -> ojf_points_within
    assert f_dev == f_have, (f_dev, f_have)  # hit counts are integers: equal, ties at d == tau included
    # filter (outlier removal) on device == numpy semantics
    db.filter(value=2.0)
    low = vols['wgt'] < np.float16(2.0)
    vols['tsdf'][low] = np.float16(0.1)
    vols['wgt'][low] = 0
    assert f16_ulp_distance(db.fusion_weights[s].cpu().numpy(), vols['wgt']).max() <= 1
    db.reset(s)
    assert float(db.fusion_weights[s].float().abs().sum()) == 0 and db.state[s] is False
    assert torch.all(db.scenes_est[s].volume == torch.tensor(0.1, dtype=torch.float16))


@pytest.mark.parametrize('sem', [False, True])
def test_stream_on_a_box_against_oracle(cuda, sem):
    """test_stream_config_A_against_oracle on a NON-CUBIC volume whose origin components all differ (box_cases.py ``room``,
    66 x 62 x 37, 45x52 frames 0, 3, 7, 12): Database takes the shape from the dataset's grid, Pipeline.fuse, evaluate, the
    F-score, filter, reset and render run on it.  The bars are the cube test's."""
    import copy
    from box_cases import BOXES, BoxStream
    from online_joint_depthfusion_and_semantic_amd.render import render_views
    h, w = 45, 52
    cfg = default_config(h, w, semantics=sem, use_semantics=sem, integrate_mode='fast')
    cfg.SETTINGS.device = str(cuda)
    st = BoxStream('room', h, w)
    db = Database(st, database_config(cfg))
    s = st.scene
    assert tuple(db.scenes_est[s].volume.shape) == st.shape == tuple(db.scenes_gt[s].volume.shape)
    assert np.array_equal(np.asarray(db.origin[s]), st.origin) and db.resolution[s] == st.resolution
    pipe = Pipeline(cfg)
    torch.manual_seed(5)
    for m in pipe._fusion_network.modules():
        if isinstance(m, torch.nn.Conv2d):
            torch.nn.init.xavier_normal_(m.weight)
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    pipe = pipe.to(cuda).eval()
    cpu_net = copy.deepcopy(pipe._fusion_network).cpu().eval()
    vols = fresh_volumes(st.shape, True)
    with torch.no_grad():
        for i in BOXES['room']['frames']:
            pipe.fuse(_batch(st, i, cuda), db, cuda)
            oracle_fuse(st, i, vols, cpu_net, sem)
    got_t, got_w = db.scenes_est[s].volume.cpu().numpy(), db.fusion_weights[s].cpu().numpy()
    wd = f16_ulp_distance(got_w, vols['wgt'])
    assert wd.max() <= 1
    nan = np.isnan(got_t) | np.isnan(vols['tsdf'])
    assert (np.isnan(got_t) == np.isnan(vols['tsdf'])).all()
    td = np.where(nan, 0, np.abs(got_t.astype(np.float32) - vols['tsdf'].astype(np.float32)))
    touched = vols['wgt'] > 0
    print('box stream sem=%s: %d touched, %d weight ulps, TSDF p99 %.2e max %.2e' % (
        sem, int(touched.sum()), int((wd > 0).sum()), float(np.percentile(td[touched], 99)), float(td.max())))
    assert touched.sum() > 20000
    assert np.percentile(td[touched], 99) <= 6.2e-5 and td.max() <= 2 * TSDF_ABS_TOL, float(td.max())
    if sem:
        assert n_mismatch(db.ids_est[s].volume.cpu().numpy(), vols['ids']) == 0
        assert n_mismatch(db.scores[s].volume.cpu().numpy(), vols['scores']) == 0
    gt = db.scenes_gt[s].volume.cpu().numpy()
    have = db.evaluate(mode='val')
    same = metrics.evaluation(got_t, gt, got_w > 0)
    for k in same:
        assert abs(same[k] - have[k]) <= 1e-6 * max(1.0, abs(same[k])), (k, same[k], have[k])
    want = metrics.evaluation(vols['tsdf'], gt, vols['wgt'] > 0)
    for k in want:
        assert abs(want[k] - have[k]) <= 1e-3 * max(1.0, abs(want[k])), (k, want[k], have[k])
    f_have = metrics.reconstruction_f_score(got_t, gt, got_w, st.origin, st.resolution)
    f_want = metrics.reconstruction_f_score(vols['tsdf'], gt, vols['wgt'], st.origin, st.resolution)
    assert abs(f_have['fscore'] - f_want['fscore']) <= 1e-3 and f_want['fscore'] > 0.05, (f_have, f_want)
    f_dev = metrics.reconstruction_f_score(db.scenes_est[s].volume, db.scenes_gt[s].volume, db.fusion_weights[s],
                                           st.origin, st.resolution)  # volumes on the device -> ojf_points_within
    assert f_dev == f_have, (f_dev, f_have)
    # Database.render == render_views on the same volumes, from a fused pose
    f = st.batch(3)
    direct = render_views(db.scenes_est[s].volume, db.fusion_weights[s], db.ids_est[s].volume if sem else None,
                          origin=db.origin[s], resolution=db.resolution[s], intrinsics=f['intrinsics'],
                          extrinsics=f['extrinsics'], shape=(h, w))
    shown = db.render(s, f['intrinsics'], f['extrinsics'], (h, w), semantics=sem)
    for k in ('depth', 'normals') + (('labels',) if sem else ()):
        assert torch.equal(shown[k].view(torch.uint8), direct[k].view(torch.uint8)), k
    assert float((direct['depth'] > 0).float().mean()) > 0.3
    # filter (outlier removal) on device == numpy semantics
    db.filter(value=2.0)
    low = vols['wgt'] < np.float16(2.0)
    vols['tsdf'][low] = np.float16(0.1)
    vols['wgt'][low] = 0
    assert 0 < low.sum() < low.size and (vols['wgt'] > 0).any()
    assert f16_ulp_distance(db.fusion_weights[s].cpu().numpy(), vols['wgt']).max() <= 1
    assert (db.scenes_est[s].volume.cpu().numpy()[low] == np.float16(0.1)).all()
    db.reset(s)
    assert float(db.fusion_weights[s].float().abs().sum()) == 0 and db.state[s] is False
    assert torch.all(db.scenes_est[s].volume == torch.tensor(0.1, dtype=torch.float16))
    assert tuple(db.scenes_est[s].volume.shape) == st.shape


def test_fuse_with_predicted_semantics(cuda):
    """semantic_strategy 'predict': AdapNet++ (torch ops on the GPU) -> softmax -> (score, id) per pixel
    (pipeline.py:42-60,181-185) feeding the HIP semantic volume update."""
    h, w, grid = 64, 96, 32
    cfg = default_config(h, w, semantics=True, use_semantics=True, n_classes=12)
    cfg.SETTINGS.device = str(cuda)
    cfg.DATA.semantic_strategy = 'predict'
    st = make_stream(h, w, grid, n_classes=12)
    db = Database(st, database_config(cfg))
    torch.manual_seed(0)
    pipe = Pipeline(cfg).to(cuda).eval()
    assert pipe._semantic_2d_network is not None
    with torch.no_grad():
        for i in range(2):
            pipe.fuse(_batch(st, i, cuda), db, cuda)
    s = st.scene
    w_vol = db.fusion_weights[s].float()
    sc = db.scores[s].volume.float()
    touched = w_vol > 0
    assert int(touched.sum()) > 500
    assert float(sc[touched].min()) > 0 and float(sc[touched].max()) <= 1.0  # softmax confidences
    assert float(sc[~touched].abs().max()) == 0
    assert int(db.ids_est[s].volume.max()) < 12


def test_segmentation_graph_replay_equals_eager(cuda):
    """The device-graph replay of the AdapNet++ front end (labels2d.LabelFrontEnd.segmentation_graph) returns what the eager
    call returns (to rounding), frame after frame and after an in-place weight update."""
    h, w, grid = 64, 96, 32
    cfg = default_config(h, w, semantics=True, use_semantics=True, n_classes=12)
    cfg.SETTINGS.device = str(cuda)
    cfg.DATA.semantic_strategy = 'predict'
    st = make_stream(h, w, grid, n_classes=12)
    torch.manual_seed(0)
    pipe = Pipeline(cfg).to(cuda).eval()
    pipe.device = torch.device(cuda)
    pipe._semantic_2d_network.no_resn50_dropout()  # the reference's inference-time dropout would make both random
    with torch.no_grad():
        for i in range(3):
            b = _batch(st, i, cuda)
            b['image'] = torch.randn(1, 3, h, w, device=cuda) * 50 + 120
            want_s, want_i = pipe._labels2d.segmentation(b, cuda).max(dim=-1)
            got_s, got_i = pipe._labels2d.segmentation_graph(b, cuda)
            assert pipe._labels2d.seg_graph['graph'] is not None  # the capture worked: this is the replay path
            # same operators; the convolution library may pick another algorithm between calls, so scores agree to
            # rounding and an arg-max can flip only where two classes tie to that precision
            assert torch.allclose(got_s, want_s, atol=1e-5, rtol=0), i
            assert float((got_i == want_i).float().mean()) > 0.999, i
            if i == 1:  # parameters are read in place by the replay
                for p in pipe._semantic_2d_network.parameters():
                    p.mul_(1.01)


@pytest.mark.parametrize('engine', ['hip', 'torch'])
def test_fuse_predict_strategy_matches_reference_golden(cuda, engine):
    """semantic_strategy 'predict' against the REFERENCE's Pipeline.fuse with its own AdapNet in front
    (tests/golden/make_golden_adapnet.py::predict_pipeline: stand-in ResNet-50 backbone, seeded weights, dropout flags
    off): per-frame (score, id) images of `_segmentation(...).max(-1)` (pipeline.py:42-60,181-185) and the four
    volumes after every frame.  The near-uniform softmax of a randomly initialised 12-class net leaves 0.6 % of the
    pixels with a top-1 / top-2 margin below 1e-4, where an arg-max may legitimately flip; everywhere else ids are
    equal.  A flipped pixel changes the semantic input channel of the two-head fusion net, so TSDF is compared with
    the looser bound stated below; weights never see either net and stay bit-exact (PARITY mode)."""
    from adapnet_golden_util import randomise_net
    g = golden('pipeline_predict_64x96_g32.npz')
    small = golden('pipeline_v3_sem_24x32_g32.npz')
    h, w, grid, n_classes = 64, 96, 32, 12
    cfg = default_config(h, w, semantics=True, use_semantics=True, n_classes=n_classes, integrate_mode='parity')
    cfg.SETTINGS.device = str(cuda)
    cfg.DATA.semantic_strategy = 'predict'
    cfg.SEMANTIC_2D_MODEL.engine = engine
    st = make_stream(h, w, grid, n_classes=n_classes)
    db = Database(st, database_config(cfg))
    pipe = Pipeline(cfg)
    pipe._fusion_network.load_state_dict({k[len('state_'):]: torch.from_numpy(small[k]) for k in small.files if k.startswith('state_')})
    assert list(pipe._semantic_2d_network.state_dict().keys()) == list(g['keys'])
    randomise_net(pipe._semantic_2d_network, 31)
    pipe = pipe.to(cuda).eval()
    pipe.device = torch.device(cuda)
    s = st.scene
    with torch.no_grad():
        for i in range(2):
            b = _batch(st, i, cuda)
            ids, scores = pipe._labels2d.frame_semantics(b, cuda)
            scores, ids = scores.reshape(h, w).cpu().numpy(), ids.reshape(h, w).cpu().numpy()
            margin = g['f%d_seg_margin' % i]
            clear = margin > 1e-4
            flips = int((ids != g['f%d_seg_ids' % i]).sum())
            ds = float(np.abs(scores - g['f%d_seg_scores' % i]).max())
            print('predict %s frame %d: max |d score| %.2e, %d arg-max flips (%d pixels with margin < 1e-4)' % (engine, i, ds, flips, int((~clear).sum())))
            assert ds <= 1e-6  # measured 7e-8 .. 1.2e-7 (softmax probabilities of ~0.1)
            assert (ids[clear] == g['f%d_seg_ids' % i][clear]).all() and flips <= (~clear).sum()
            pipe.fuse(b, db, cuda)
            got = {k: v.cpu().numpy() for k, v in (('tsdf', db.scenes_est[s].volume), ('wgt', db.fusion_weights[s]),
                                                   ('ids', db.ids_est[s].volume), ('scores', db.scores[s].volume))}
            touched = g['f%d_wgt' % i] > 0
            assert n_mismatch(got['wgt'], g['f%d_wgt' % i]) == 0, i
            id_bad = int((got['ids'] != g['f%d_ids' % i]).sum())
            sc_ulp = f16_ulp_distance(got['scores'], g['f%d_scores' % i])
            td = np.nan_to_num(np.abs(got['tsdf'].astype(np.float32) - g['f%d_tsdf' % i].astype(np.float32)))
            print('   volumes: %d of %d touched voxels with another id, score ulps max %d (%d voxels > 1), max |dTSDF| %.2e, %d voxels > 6.2e-5'
                  % (id_bad, int(touched.sum()), int(sc_ulp.max()), int((sc_ulp > 1).sum()), float(td.max()), int((td > 6.2e-5).sum())))
            # measured: no flip, ids / scores identical, |dTSDF| 4.8e-7.  Bars: a flipped pixel may change the 56 entries it
            # writes; scores within one fp16 ulp; TSDF within one fp16 ulp of the band (as everywhere else) unless a flip
            # changed the semantic input channel of the two-head net
            assert id_bad <= 56 * flips and sc_ulp.max() <= 1
            assert (np.isnan(got['tsdf']) == np.isnan(g['f%d_tsdf' % i])).all()
            assert td.max() <= (6.2e-5 if flips == 0 else 2e-3)


def test_engine_follows_replaced_parameters(cuda):
    """weights swapped in with load_state_dict(assign=True) (new Parameter objects, version counters reset)
    or by rebinding ``param.data`` must reach the folded HIP engine on the very next frame."""
    h, w, grid = 24, 32, 32
    cfg, st, db, pipe = _setup(h, w, grid, False, False, 'fast', cuda)
    with torch.no_grad():
        pipe.fuse(_batch(st, 0, cuda), db, cuda)
        first = pipe._engine
        other = Pipeline(cfg)._fusion_network.to(cuda).state_dict()
        pipe._fusion_network.load_state_dict(other, assign=True)
        pipe.fuse(_batch(st, 1, cuda), db, cuda)
        second = pipe._engine
        assert second is not first
        for p in pipe._fusion_network.parameters():
            p.data = p.data.clone() * 1.0001
        pipe.fuse(_batch(st, 2, cuda), db, cuda)
        assert pipe._engine is not second


# ---- the range guard protects the scene -------------------------------------------------------------
def _tripping_pipeline(cuda, h, w, grid, policy, sem=False):
    """A pipeline whose net leaves the fp16 range: first convolution scaled by 1e9 (eval-mode BN with fresh running
    statistics does not normalise it away)."""
    cfg, st, db, pipe = _setup(h, w, grid, sem, False, 'fast', cuda)
    cfg.FUSION_MODEL.guard_policy = policy
    torch.manual_seed(5)
    for m in pipe._fusion_network.modules():
        if isinstance(m, torch.nn.Conv2d):
            torch.nn.init.xavier_normal_(m.weight)
    with torch.no_grad():
        pipe._fusion_network.block0[0].block[0].weight.mul_(1e9)
    return cfg, st, db, pipe


def _volumes(db, s):
    return [db.scenes_est[s].volume.clone(), db.fusion_weights[s].clone()]


@pytest.mark.parametrize('mode', ['fast', 'parity'])
def test_range_guard_leaves_the_volumes_untouched(cuda, mode):
    """A frame whose net trips the split-fp16 range guard must not be fused - nor any frame after it until the host has
    reported the event: volumes bit-identical to the pre-frame state, Pipeline.check() raises, and after the check the
    same scene fuses normally again with arithmetic f32."""
    from online_joint_depthfusion_and_semantic_amd import _lib
    h, w, grid = 48, 64, 64
    cfg, st, db, pipe = _tripping_pipeline(cuda, h, w, grid, 'raise')
    pipe._integrate_mode = _lib.MODE_PARITY if mode == 'parity' else _lib.MODE_FAST
    s = st.scene
    good = Pipeline(default_config(h, w, semantics=False, use_semantics=False, integrate_mode=mode)).to(cuda).eval()
    with torch.no_grad():
        good.fuse(_batch(st, 0, cuda), db, cuda)  # a healthy frame first: the pre-frame state is not the empty volume
        good.check()
        before = _volumes(db, s)
        assert float((before[1].float() > 0).sum()) > 1000
        fused = 0
        for i in range(1, 4):
            try:
                pipe.fuse(_batch(st, i, cuda), db, cuda)
                fused += 1
            except _lib.OjfError:  # (a later frame's forward may already see the flag: equally fine)
                break
        torch.cuda.synchronize()
        for a, b in zip(before, _volumes(db, s)):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16))
        with pytest.raises(_lib.OjfError, match='fp16 range'):
            pipe.check()
        pipe.check()  # cleared
        # the scene is alive: the same (un-normalised) net fuses on the fp32-input path
        cfg.FUSION_MODEL.arithmetic = 'f32'
        pipe.fuse(_batch(st, 1, cuda), db, cuda)
        pipe.check()
        after = _volumes(db, s)
        assert not torch.equal(before[1].view(torch.int16), after[1].view(torch.int16))


def test_range_guard_policy_f32_refuses_nothing_and_loses_nothing(cuda):
    """FUSION_MODEL.guard_policy = 'f32': the tripped frames are fused again on the fp32-input path, in order - the volumes
    equal those of a pipeline that ran arithmetic f32 from the first frame, bit for bit."""
    h, w, grid = 48, 64, 64
    n_frames = 6
    cfg, st, db, pipe = _tripping_pipeline(cuda, h, w, grid, 'f32')
    cfg2, st2, db2, ref = _tripping_pipeline(cuda, h, w, grid, 'raise')
    cfg2.FUSION_MODEL.arithmetic = 'f32'
    ref._fusion_network.load_state_dict(pipe._fusion_network.state_dict())
    with torch.no_grad(), pytest.warns(RuntimeWarning, match='switched to f32'):
        for i in range(n_frames):
            pipe.fuse(_batch(st, i, cuda), db, cuda)
        pipe.check()
    with torch.no_grad():
        for i in range(n_frames):
            ref.fuse(_batch(st2, i, cuda), db2, cuda)
        ref.check()
    assert pipe.guard_events == 1 and cfg.FUSION_MODEL.arithmetic == 'f32'
    for a, b in zip(_volumes(db, st.scene), _volumes(db2, st2.scene)):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert float((db.fusion_weights[st.scene].float() > 0).sum()) > 1000


# ---- the reference's own net in train() mode -------------------------------------------------------
@pytest.mark.parametrize('engine', ['hip', 'torch'])
def test_fuse_training_train_mode_matches_reference_golden(cuda, engine):
    """Fixture = ONE ``fuse_training`` frame + ``loss.backward()`` of the reference with /root/reference/modules/model.py's
    FusionNet_v3 in train() mode (batch statistics, running-statistics update; only the Dropout2d modules in eval), held
    twice from the same pre-frame state: as the reference runs (fp32) and with the same module tree in float64
    (tests/golden/make_golden.py::run_training_train_mode).  A batch-statistics net amplifies rounding (the reference's own
    fp32 gradients deviate by up to 6 % of a tensor's scale from its float64 ones here), so every tensor is judged against
    the float64 values: within 1e-4 of its scale, or no further away than 2.5x the reference's own fp32 run on that tensor
    (gradients also: than twice the reference's worst relative fp32 deviation over all gradients, the noise level of the net -
    the bar of tests/test_train_gpu.py; torch's own GPU autograd needs it on one tensor).  Checked:
    tsdf_target bit for bit, tsdf_est, tsdf_fused, loss, ALL parameter gradients, ALL BatchNorm buffers after the step
    (running_mean, running_var, num_batches_tracked), the post-frame weight volume bit for bit and the TSDF volume."""
    g = golden('train_mode_v3_nosem_48x64_g64.npz')
    h, w, grid = 48, 64, 64
    state = {k[len('state_'):]: torch.from_numpy(g[k]) for k in g.files if k.startswith('state_')}
    cfg, st, db, pipe = _setup(h, w, grid, False, False, 'parity', cuda, state)
    cfg.FUSION_MODEL.train_engine = engine
    s = st.scene
    db.scenes_est[s].volume.copy_(torch.from_numpy(g['pre_tsdf']))
    db.fusion_weights[s].copy_(torch.from_numpy(g['pre_wgt']))
    net = pipe._fusion_network
    net.train()
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.eval()
    out = pipe.fuse_training(_batch(st, 2, cuda), db, cuda)
    diff = out['tsdf_fused'] - out['tsdf_target']
    loss = diff.abs().mean() + 10 * (diff ** 2).mean()
    loss.backward()
    import hashlib
    tgt = np.ascontiguousarray(out['tsdf_target'].detach()[0].cpu().numpy())
    assert hashlib.sha256(tgt.tobytes()).hexdigest() == str(g['32_tsdf_target_sha256'])
    assert out['tsdf_fused'].shape[1] == int(g['32_n_valid'])

    worst = [0.0]

    gmax = max(float(np.abs(g[k]).max()) for k in g.files if k.startswith('64_grad_') and g[k].size)
    noise = max(float(np.abs(g['32_' + k[3:]].astype(np.float64) - g[k]).max()) / max(float(np.abs(g[k]).max()), 1e-3 * gmax)
                for k in g.files if k.startswith('64_grad_') and g[k].size)

    def bar(got, key, floor=None, what=None):
        got = np.asarray(got, np.float64)
        truth, fp32 = g['64_' + key].astype(np.float64), g['32_' + key].astype(np.float64)
        scale = max(float(np.abs(truth).max()), floor or 0.0)
        e, e32 = float(np.abs(got - truth).max()), float(np.abs(fp32 - truth).max())
        assert e <= max(1e-4 * scale, 2.5 * e32, (2.0 * noise * scale) if key.startswith('grad_') else 0.0), (what or key, e, e32, scale, noise)
        worst[0] = max(worst[0], e / max(e32, 1e-4 * scale))
    bar(out['tsdf_est'].detach()[0].cpu().numpy(), 'tsdf_est')
    bar(out['tsdf_fused'].detach()[0].cpu().numpy(), 'tsdf_fused')
    bar(float(loss.detach()), 'loss')
    for name, p in net.named_parameters():
        want = g['64_grad_' + name]
        assert (p.grad is None) == (want.size == 0), name
        if want.size:
            bar(p.grad.cpu().numpy(), 'grad_' + name, floor=1e-3 * gmax)
    for name, b in net.named_buffers():
        if b.dtype.is_floating_point:
            bar(b.cpu().numpy(), 'buf_' + name)
        else:
            assert int(b) == int(g['64_buf_' + name]) == 1, name
    print('train() mode vs the reference (%s engine): worst deviation = %.2f x the reference\'s own fp32 run' % (engine, worst[0]))
    # volumes: integrate(test=False) with the clamped est
    assert f16_ulp_distance(db.fusion_weights[s].cpu().numpy(), g['32_post_wgt']).max() == 0
    got = db.scenes_est[s].volume.cpu().numpy().astype(np.float32)
    td = np.nan_to_num(np.abs(got - g['32_post_tsdf'].astype(np.float32)))
    touched = g['32_post_wgt'] > 0
    assert td.max() <= 2 * TSDF_ABS_TOL and (td[touched] > 0).mean() <= 0.02, (float(td.max()), float((td[touched] > 0).mean()))


# ---- several scenes per call ---------------------------------------------------------------------------
@pytest.mark.parametrize('launches', ['joint', 'slots'])
@pytest.mark.parametrize('sem', [False, True])
def test_fuse_many_equals_separate_fuse_calls(cuda, sem, launches):
    """Pipeline.fuse_many runs one frame of each of S scenes side by side (slot i: own engine, est rows, workspace, stream):
    every volume of every scene must come out bit for bit as from S separate fuse() calls per step - FAST mode is
    deterministic and the scenes share nothing but the read-only weights."""
    from online_joint_depthfusion_and_semantic_amd.synthetic import SyntheticDataset
    h, w, grid, S, frames = 48, 64, 64, 3, 4
    scenes = tuple('room_%d' % k for k in range(S))

    def build():
        cfg = default_config(h, w, semantics=sem, use_semantics=sem, integrate_mode='fast')
        cfg.SETTINGS.device = str(cuda)
        cfg.SETTINGS.fuse_many_launches = launches  # (default 'auto': joint launches for two scenes, per-slot launches from three on)
        ds = SyntheticDataset(h, w, grid, 8, scenes=scenes)
        db = Database(ds, database_config(cfg))
        torch.manual_seed(3)
        pipe = Pipeline(cfg)
        for m in pipe._fusion_network.modules():
            if isinstance(m, torch.nn.Conv2d):
                torch.nn.init.xavier_normal_(m.weight)
        return ds, db, pipe.to(cuda).eval()
    ds_a, db_a, many = build()
    ds_b, db_b, one = build()
    one._fusion_network.load_state_dict(many._fusion_network.state_dict())

    def batch(ds, s, i):
        b = ds.streams[s].batch(i)
        return {k: (v.to(cuda) if torch.is_tensor(v) else v) for k, v in b.items()}
    with torch.no_grad():
        for i in range(frames):
            many.fuse_many([batch(ds_a, s, i) for s in scenes], db_a, cuda)
            for s in scenes:
                one.fuse(batch(ds_b, s, i), db_b, cuda)
        many.check()
        one.check()
        with pytest.raises(ValueError):
            many.fuse_many([batch(ds_a, scenes[0], 0), batch(ds_a, scenes[0], 1)], db_a, cuda)
    for s in scenes:
        assert float((db_a.fusion_weights[s].float() > 0).sum()) > 1000
        pairs = [(db_a.scenes_est[s].volume, db_b.scenes_est[s].volume), (db_a.fusion_weights[s], db_b.fusion_weights[s])]
        if sem:
            pairs += [(db_a.ids_est[s].volume, db_b.ids_est[s].volume), (db_a.scores[s].volume, db_b.scores[s].volume)]
        for a, b in pairs:
            assert torch.equal(a.view(torch.uint8) if a.dtype == torch.uint8 else a.view(torch.int16), b.view(torch.uint8) if b.dtype == torch.uint8 else b.view(torch.int16)), s
    assert not torch.equal(db_a.fusion_weights[scenes[0]], db_a.fusion_weights[scenes[1]])  # (the scenes differ)


def test_fuse_many_with_predicted_semantics(cuda):
    """fuse_many with ``semantic_strategy: predict``: the S frames go through AdapNet++ as ONE batched pass
    (SegEngine.predict_many).  Geometry (TSDF, weights: the geometry-only net never sees the labels) bit for bit as from
    separate fuse() calls; the per-frame (score, id) images equal the single-frame pass to 1e-6 / apart from near-ties, so
    the semantic volumes agree on >= 99.9 % of the touched voxels and the score volume to one fp16 ulp."""
    from adapnet_golden_util import randomise_net
    from online_joint_depthfusion_and_semantic_amd.synthetic import SyntheticDataset
    h, w, grid, S, n_classes = 64, 96, 32, 3, 12
    scenes = tuple('room_%d' % k for k in range(S))

    def build():
        cfg = default_config(h, w, semantics=True, use_semantics=False, n_classes=n_classes, integrate_mode='fast')
        cfg.SETTINGS.device = str(cuda)
        cfg.DATA.semantic_strategy = 'predict'
        ds = SyntheticDataset(h, w, grid, 8, scenes=scenes, n_classes=n_classes)
        db = Database(ds, database_config(cfg))
        torch.manual_seed(3)
        pipe = Pipeline(cfg)
        for m in pipe._fusion_network.modules():
            if isinstance(m, torch.nn.Conv2d):
                torch.nn.init.xavier_normal_(m.weight)
        randomise_net(pipe._semantic_2d_network, 31)
        for m in pipe._semantic_2d_network.modules():
            if hasattr(m, 'dropout') and isinstance(m.dropout, bool):
                m.dropout = False  # (the masks are a function of the frame counter: the two pipelines would draw differently)
        return ds, db, pipe.to(cuda).eval()
    ds_a, db_a, many = build()
    ds_b, db_b, one = build()
    one.load_state_dict(many.state_dict())

    def batch(ds, s, i):
        return {k: (v.to(cuda) if torch.is_tensor(v) else v) for k, v in ds.streams[s].batch(i).items()}
    with torch.no_grad():
        for i in range(3):
            many.fuse_many([batch(ds_a, s, i) for s in scenes], db_a, cuda)
            for s in scenes:
                one.fuse(batch(ds_b, s, i), db_b, cuda)
        many.check()
        one.check()
    assert many._labels2d.seg_graph_many['graph'] is not None  # the batched pass was captured and replayed
    for s in scenes:
        assert torch.equal(db_a.scenes_est[s].volume.view(torch.int16), db_b.scenes_est[s].volume.view(torch.int16))
        assert torch.equal(db_a.fusion_weights[s].view(torch.int16), db_b.fusion_weights[s].view(torch.int16))
        touched = db_b.fusion_weights[s] > 0
        same = (db_a.ids_est[s].volume[touched] == db_b.ids_est[s].volume[touched]).float().mean().item()
        assert same >= 0.999, (s, same)
        ulp = f16_ulp_distance(db_a.scores[s].volume.cpu().numpy(), db_b.scores[s].volume.cpu().numpy())
        assert ulp.max() <= 1, (s, int(ulp.max()))


def test_fuse_sequence_with_predicted_semantics(cuda):
    """Pipeline.fuse_sequence: consecutive frames of ONE scene, labels of the chunk predicted as one batched AdapNet++ pass,
    frame steps in order.  Geometry bit for bit as from frame-at-a-time fuse(); label volumes as in the fuse_many test."""
    from adapnet_golden_util import randomise_net
    h, w, grid, n_classes, frames = 64, 96, 32, 12, 6

    def build():
        cfg = default_config(h, w, semantics=True, use_semantics=False, n_classes=n_classes, integrate_mode='fast')
        cfg.SETTINGS.device = str(cuda)
        cfg.DATA.semantic_strategy = 'predict'
        st = make_stream(h, w, grid, n_classes=n_classes)
        db = Database(st, database_config(cfg))
        torch.manual_seed(3)
        pipe = Pipeline(cfg)
        for m in pipe._fusion_network.modules():
            if isinstance(m, torch.nn.Conv2d):
                torch.nn.init.xavier_normal_(m.weight)
        randomise_net(pipe._semantic_2d_network, 31)
        for m in pipe._semantic_2d_network.modules():
            if hasattr(m, 'dropout') and isinstance(m.dropout, bool):
                m.dropout = False
        return st, db, pipe.to(cuda).eval()
    st_a, db_a, seq = build()
    st_b, db_b, one = build()
    one.load_state_dict(seq.state_dict())
    with torch.no_grad():
        seq.fuse_sequence([_batch(st_a, i, cuda) for i in range(4)], db_a, cuda)
        seq.fuse_sequence([_batch(st_a, i, cuda) for i in range(4, frames)], db_a, cuda)  # a shorter chunk: another graph
        for i in range(frames):
            one.fuse(_batch(st_b, i, cuda), db_b, cuda)
        seq.check()
        one.check()
    s = st_a.scene
    assert torch.equal(db_a.scenes_est[s].volume.view(torch.int16), db_b.scenes_est[s].volume.view(torch.int16))
    assert torch.equal(db_a.fusion_weights[s].view(torch.int16), db_b.fusion_weights[s].view(torch.int16))
    touched = db_b.fusion_weights[s] > 0
    assert (db_a.ids_est[s].volume[touched] == db_b.ids_est[s].volume[touched]).float().mean().item() >= 0.999
    assert f16_ulp_distance(db_a.scores[s].volume.cpu().numpy(), db_b.scores[s].volume.cpu().numpy()).max() <= 1


@pytest.mark.gpu
def test_fuse_sequence_prefetch_changes_no_bit(cuda):
    """fuse_sequence(chunk, prefetch=next chunk): the next chunk's batched 2-D pass runs on a side stream beside this chunk's
    frame steps.  The same graph replays, on another stream: all four volumes bit for bit as without the prefetch, also when
    the announced chunk is NOT the one that comes (its labels are dropped) and across a change of chunk length."""
    from adapnet_golden_util import randomise_net
    h, w, grid, n_classes, frames = 64, 96, 32, 12, 14

    def build():
        cfg = default_config(h, w, semantics=True, use_semantics=False, n_classes=n_classes, integrate_mode='fast')
        cfg.SETTINGS.device = str(cuda)
        cfg.DATA.semantic_strategy = 'predict'
        st = make_stream(h, w, grid, n_classes=n_classes)
        db = Database(st, database_config(cfg))
        torch.manual_seed(3)
        pipe = Pipeline(cfg)
        for m in pipe._fusion_network.modules():
            if isinstance(m, torch.nn.Conv2d):
                torch.nn.init.xavier_normal_(m.weight)
        randomise_net(pipe._semantic_2d_network, 31)
        for m in pipe._semantic_2d_network.modules():
            if hasattr(m, 'dropout') and isinstance(m.dropout, bool):
                m.dropout = False
        return st, db, pipe.to(cuda).eval()
    st_a, db_a, pre = build()
    st_b, db_b, plain = build()
    plain.load_state_dict(pre.state_dict())
    chunks = [(0, 4), (4, 8), (8, 12), (12, 14)]
    with torch.no_grad():
        ba = [[_batch(st_a, i, cuda) for i in range(a, b)] for a, b in chunks]
        bb = [[_batch(st_b, i, cuda) for i in range(a, b)] for a, b in chunks]
        pre.fuse_sequence(ba[0], db_a, cuda, prefetch=ba[1])
        pre.fuse_sequence(ba[1], db_a, cuda, prefetch=ba[3])   # announces the wrong chunk: ba[2] comes
        pre.fuse_sequence(ba[2], db_a, cuda, prefetch=ba[3])   # ... and a shorter one next
        pre.fuse_sequence(ba[3], db_a, cuda)
        for c in bb:
            plain.fuse_sequence(c, db_b, cuda)
        pre.check()
        plain.check()
    s = st_a.scene
    assert torch.equal(db_a.scenes_est[s].volume.view(torch.int16), db_b.scenes_est[s].volume.view(torch.int16))
    assert torch.equal(db_a.fusion_weights[s].view(torch.int16), db_b.fusion_weights[s].view(torch.int16))
    assert torch.equal(db_a.ids_est[s].volume, db_b.ids_est[s].volume)
    assert torch.equal(db_a.scores[s].volume.view(torch.int16), db_b.scores[s].volume.view(torch.int16))


@pytest.mark.parametrize('sem', [False, True])
def test_fuse_sequence_without_a_2d_network(cuda, sem):
    """fuse_sequence on streams that need no 2-D pass (geometry only / gt labels): an empty chunk is a no-op, a chunk of one
    frame is fuse(), ``prefetch`` is ignored - all volumes bit for bit as from frame-at-a-time fuse()."""
    h, w, grid, frames = 48, 64, 32, 7

    def build():
        cfg = default_config(h, w, semantics=sem, use_semantics=sem, integrate_mode='fast')
        cfg.SETTINGS.device = str(cuda)
        st = make_stream(h, w, grid)
        db = Database(st, database_config(cfg))
        torch.manual_seed(3)
        pipe = Pipeline(cfg)
        for m in pipe._fusion_network.modules():
            if isinstance(m, torch.nn.Conv2d):
                torch.nn.init.xavier_normal_(m.weight)
        return st, db, pipe.to(cuda).eval()
    st_a, db_a, seq = build()
    st_b, db_b, one = build()
    one._fusion_network.load_state_dict(seq._fusion_network.state_dict())
    with torch.no_grad():
        ba = [_batch(st_a, i, cuda) for i in range(frames)]
        seq.fuse_sequence([], db_a, cuda)
        seq.fuse_sequence(ba[0:1], db_a, cuda, prefetch=ba[1:4])
        seq.fuse_sequence(ba[1:4], db_a, cuda, prefetch=ba[4:7])
        seq.fuse_sequence(ba[4:7], db_a, cuda, prefetch=[])
        for i in range(frames):
            one.fuse(_batch(st_b, i, cuda), db_b, cuda)
        seq.check()
        one.check()
    s = st_a.scene
    pairs = [(db_a.scenes_est[s].volume, db_b.scenes_est[s].volume), (db_a.fusion_weights[s], db_b.fusion_weights[s])]
    if sem:
        pairs += [(db_a.scores[s].volume, db_b.scores[s].volume)]
        assert torch.equal(db_a.ids_est[s].volume, db_b.ids_est[s].volume)
    for a, b in pairs:
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert float((db_a.fusion_weights[s].float() > 0).sum()) > 1000


def test_streams_overlap_probe(cuda):
    """ojf_streams_overlap (set-up helper behind labels2d.side_stream): a stream never runs beside itself; two streams give
    0 or 1 (the runtime's queue mapping decides); side_stream returns a stream that passed the probe when one of its eight
    candidates does."""
    from online_joint_depthfusion_and_semantic_amd import _lib
    from online_joint_depthfusion_and_semantic_amd.labels2d import side_stream
    lib = _lib.load()
    a, b = torch.cuda.Stream(device=cuda), torch.cuda.Stream(device=cuda)
    assert lib.ojf_streams_overlap(a.cuda_stream, a.cuda_stream) == 0
    assert lib.ojf_streams_overlap(a.cuda_stream, b.cuda_stream) in (0, 1)
    cfg = default_config(24, 32)
    cfg.SETTINGS.device = str(cuda)
    pipe = Pipeline(cfg).to(cuda).eval()
    pipe.device = torch.device(cuda)
    main = torch.cuda.current_stream(cuda)
    side = side_stream(cuda, [main])
    assert isinstance(side, torch.cuda.Stream) and side.cuda_stream != main.cuda_stream


# ---- round 6: the gaps the look-ahead / multi-scene entry points opened ---------------------
def _predict_pipeline(cuda, h, w, grid, n_classes, scenes=None, frames=16):
    from adapnet_golden_util import randomise_net
    from online_joint_depthfusion_and_semantic_amd.synthetic import SyntheticDataset
    cfg = default_config(h, w, semantics=True, use_semantics=False, n_classes=n_classes, integrate_mode='fast')
    cfg.SETTINGS.device = str(cuda)
    cfg.DATA.semantic_strategy = 'predict'
    if scenes:
        st = SyntheticDataset(h, w, grid, frames, scenes=scenes, n_classes=n_classes)
    else:
        st = make_stream(h, w, grid, n_classes=n_classes)
    db = Database(st, database_config(cfg))
    torch.manual_seed(3)
    pipe = Pipeline(cfg)
    for m in pipe._fusion_network.modules():
        if isinstance(m, torch.nn.Conv2d):
            torch.nn.init.xavier_normal_(m.weight)
    randomise_net(pipe._semantic_2d_network, 31)
    for m in pipe._semantic_2d_network.modules():
        if hasattr(m, 'dropout') and isinstance(m.dropout, bool):
            m.dropout = False
    return cfg, st, db, pipe.to(cuda).eval()


def _same_volumes(db_a, db_b, s):
    assert torch.equal(db_a.scenes_est[s].volume.view(torch.int16), db_b.scenes_est[s].volume.view(torch.int16))
    assert torch.equal(db_a.fusion_weights[s].view(torch.int16), db_b.fusion_weights[s].view(torch.int16))
    assert torch.equal(db_a.ids_est[s].volume, db_b.ids_est[s].volume)
    assert torch.equal(db_a.scores[s].volume.view(torch.int16), db_b.scores[s].volume.view(torch.int16))


def test_fuse_sequence_prefetch_of_a_dropped_chunk_is_never_taken(cuda):
    """The announced chunk is matched by OBJECT IDENTITY of batch dicts the pipeline keeps alive: a caller that announces a
    chunk, drops it and builds new dicts (which CPython may give the freed addresses - the old id()-keyed match could then
    fuse the stale labels of OTHER frames) must get its own labels.  The new dicts here carry different frames."""
    import gc
    h, w, grid, n_classes = 64, 96, 32, 12
    _, st_a, db_a, pre = _predict_pipeline(cuda, h, w, grid, n_classes)
    _, st_b, db_b, plain = _predict_pipeline(cuda, h, w, grid, n_classes)
    plain.load_state_dict(pre.state_dict())
    with torch.no_grad():
        first = [_batch(st_a, i, cuda) for i in range(0, 4)]
        for attempt in range(6):  # several rounds: address reuse needs luck, the assertion must hold every time
            announced = [_batch(st_a, i, cuda) for i in range(4, 8)]
            pre.fuse_sequence(first, db_a, cuda, prefetch=announced)
            del announced
            gc.collect()
            other = [_batch(st_a, i, cuda) for i in range(8, 12)]  # new dicts, other frames, maybe the old addresses
            pre.fuse_sequence(other, db_a, cuda)
            assert pre._labels2d.prefetch.get('hits', 0) == 0
            plain.fuse_sequence([_batch(st_b, i, cuda) for i in range(0, 4)], db_b, cuda)
            plain.fuse_sequence([_batch(st_b, i, cuda) for i in range(8, 12)], db_b, cuda)
        pre.check()
        plain.check()
    _same_volumes(db_a, db_b, st_a.scene)
    # ... and the same objects ARE taken
    with torch.no_grad():
        nxt = [_batch(st_a, i, cuda) for i in range(12, 16)]
        pre.fuse_sequence(first, db_a, cuda, prefetch=nxt)
        pre.fuse_sequence(nxt, db_a, cuda)
        pre.check()
    assert pre._labels2d.prefetch['hits'] == 1


@pytest.mark.parametrize('entry', ['fuse_sequence', 'fuse_many', 'fuse_many_joint'])
def test_range_guard_policy_f32_covers_fuse_sequence_and_fuse_many(cuda, entry):
    """guard_policy 'f32' through the chunked / multi-scene entry points: the tripped frames are fused again on the fp32-input
    path, in order - volumes bit for bit those of a pipeline that ran arithmetic f32 from the first frame through fuse()."""
    from online_joint_depthfusion_and_semantic_amd.synthetic import SyntheticDataset
    h, w, grid, S, steps = 48, 64, 64, 3, 3
    scenes = tuple('room_%d' % k for k in range(S))

    def build(policy, arithmetic):
        cfg = default_config(h, w, semantics=False, use_semantics=False, integrate_mode='fast')
        cfg.SETTINGS.device = str(cuda)
        cfg.FUSION_MODEL.guard_policy = policy
        cfg.FUSION_MODEL.arithmetic = arithmetic
        cfg.SETTINGS.fuse_many_launches = 'joint' if entry == 'fuse_many_joint' else 'slots'
        ds = SyntheticDataset(h, w, grid, 8, scenes=scenes)
        db = Database(ds, database_config(cfg))
        torch.manual_seed(5)
        pipe = Pipeline(cfg)
        for m in pipe._fusion_network.modules():
            if isinstance(m, torch.nn.Conv2d):
                torch.nn.init.xavier_normal_(m.weight)
        with torch.no_grad():
            pipe._fusion_network.block0[0].block[0].weight.mul_(1e9)  # trips the split-fp16 range guard
        return cfg, ds, db, pipe.to(cuda).eval()
    cfg, ds_a, db_a, pipe = build('f32', 'f16x3')
    _, ds_b, db_b, ref = build('raise', 'f32')
    ref._fusion_network.load_state_dict(pipe._fusion_network.state_dict())

    def batch(ds, s, i):
        return {k: (v.to(cuda) if torch.is_tensor(v) else v) for k, v in ds.streams[s].batch(i).items()}
    with torch.no_grad(), pytest.warns(RuntimeWarning, match='switched to f32'):
        for i in range(steps):
            if entry.startswith('fuse_many'):
                pipe.fuse_many([batch(ds_a, s, i) for s in scenes], db_a, cuda)
            else:  # a chunk = the step's frames of all scenes in stream order
                pipe.fuse_sequence([batch(ds_a, s, i) for s in scenes], db_a, cuda)
        pipe.check()
    with torch.no_grad():
        for i in range(steps):
            for s in scenes:
                ref.fuse(batch(ds_b, s, i), db_b, cuda)
        ref.check()
    assert pipe.guard_events == 1 and cfg.FUSION_MODEL.arithmetic == 'f32'
    for s in scenes:
        assert float((db_a.fusion_weights[s].float() > 0).sum()) > 1000
        for a, b in zip(_volumes(db_a, s), _volumes(db_b, s)):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), s


@pytest.mark.parametrize('launches,mode', [('slots', 'fast'), ('joint', 'fast'), ('slots', 'parity')])
def test_range_guard_recovery_fuses_exactly_the_skipped_frames(cuda, launches, mode):
    """guard_policy 'f32' in fuse_many when ONE scene's net trips: three scenes, three steps, and in step 1 the frame of the MIDDLE
    scene alone leaves the fp16 range (a 4 x 4 patch of masked-out pixels carries a depth of 3e4 and the first convolution is
    scaled by 100: ordinary frames reach a few hundred).  Whether the step-1 integrate calls of the two other scenes skip
    depends on where their streams stand when the flag goes up - every scene latches for itself - so the skipped frames need not
    be the last ones remembered.  The recovery must fuse again exactly the frames whose own record says "skipped":

        skipped in step 1                       f16x3, f32 (fused again), f32
        enqueued in step 1 and not skipped      f16x3, f16x3, f32
        refused by the host's poll in step 1    f16x3, f32, f32   (the event was noticed before the frame was enqueued: it is in
                                                                   no record and runs on the fp32 engine - the first history)

    (a step-2 frame is enqueued behind the event on every stream: it runs on the fp32 engine or is skipped and fused again on it).
    Both histories come from a 'raise' pipeline whose arithmetic is set by hand, frame by frame, through fuse().  The tripping
    scene equals the first, every other scene the one its record names: TSDF and weights, bit for bit.  With the earlier rule
    (the last n remembered frames) a recovery with only the middle scene skipped fused the last scene's frame twice and lost
    the middle one's (tests/test_guard_recover_host.py shows the rule itself)."""
    from online_joint_depthfusion_and_semantic_amd import _lib
    from online_joint_depthfusion_and_semantic_amd.synthetic import SyntheticDataset
    h, w, grid, S, steps = 48, 64, 64, 3, 3
    scenes = tuple('room_%d' % k for k in range(S))
    mid = scenes[1]

    def build(policy):
        cfg = default_config(h, w, semantics=False, use_semantics=False, integrate_mode=mode)
        cfg.SETTINGS.device = str(cuda)
        cfg.FUSION_MODEL.guard_policy = policy
        cfg.SETTINGS.fuse_many_launches = launches
        torch.manual_seed(5)
        pipe = Pipeline(cfg)
        for m in pipe._fusion_network.modules():
            if isinstance(m, torch.nn.Conv2d):
                torch.nn.init.xavier_normal_(m.weight)
        with torch.no_grad():
            pipe._fusion_network.block0[0].block[0].weight.mul_(100.0)
        return cfg, pipe.to(cuda).eval()

    ds = SyntheticDataset(h, w, grid, 8, scenes=scenes)

    def database(cfg):
        return Database(ds, database_config(cfg))

    def batch(s, i):
        b = ds.streams[s].batch(i)
        if (s, i) == (mid, 1):  # the trigger: in this frame's data, outside its mask (no volume ever sees these pixels)
            b['tof_depth'][0, 5:9, 7:11] = 3.0e4
            b['mask'][0, 5:9, 7:11] = False
        return {k: (v.to(cuda) if torch.is_tensor(v) else v) for k, v in b.items()}

    cfg, pipe = build('f32')
    cfg_r, ref = build('raise')
    ref._fusion_network.load_state_dict(pipe._fusion_network.state_dict())
    with torch.no_grad():
        # precondition: that frame alone trips the guard, every other frame of the test alone does not
        scratch = database(cfg_r)
        for i in range(steps):
            for s in scenes:
                ref.fuse(batch(s, i), scratch, cuda)
                if (s, i) == (mid, 1):
                    with pytest.raises(_lib.OjfError, match='fp16 range'):
                        ref.check()
                ref.check()
        # the two histories per scene (the middle scene has only the first: its step-1 frame cannot pass in f16x3)
        db_again, db_kept = database(cfg_r), database(cfg_r)
        for s in scenes:
            ref.fuse(batch(s, 0), db_again, cuda)
            ref.fuse(batch(s, 0), db_kept, cuda)
        for s in scenes:
            if s != mid:
                ref.fuse(batch(s, 1), db_kept, cuda)
        ref.check()
        cfg_r.FUSION_MODEL.arithmetic = 'f32'
        for s in scenes:
            ref.fuse(batch(s, 1), db_again, cuda)
        for s in scenes:
            ref.fuse(batch(s, 2), db_again, cuda)
            if s != mid:
                ref.fuse(batch(s, 2), db_kept, cuda)
        ref.check()

        db = database(cfg)
        with pytest.warns(RuntimeWarning, match='switched to f32'):
            for i in range(steps):
                pipe.fuse_many([batch(s, i) for s in scenes], db, cuda)
            pipe.check()
    assert pipe.guard_events == 1 and cfg.FUSION_MODEL.arithmetic == 'f32'
    records = dict(pipe.last_guard_skips)  # the frames remembered when the event was noticed: frame_id -> its call skipped
    skipped = {fid for fid, skip in records.items() if skip}
    print('range guard, %s / %s: skipped and fused again: %s; enqueued in front of the event: %s'
          % (launches, mode, sorted(skipped), sorted(set(records) - skipped)))
    assert all(int(fid.split('/')[-1]) >= 1 for fid in skipped)  # (step 0 was healthy)
    # a step-1 frame went through on f16x3 only if it was enqueued, remembered and its own record says "not skipped"; one whose
    # frame step the host's poll refused (the event was noticed inside step 1) was never enqueued on f16x3: it is in no
    # record and ran on the fp32 engine, like a skipped one
    step1 = {s: records.get(ds.streams[s].frame(1)['frame_id'], True) for s in scenes}
    assert step1[mid] and ds.streams[mid].frame(1)['frame_id'] in skipped
    for s in scenes:
        want = db_again if step1[s] else db_kept
        assert float((db.fusion_weights[s].float() > 0).sum()) > 1000
        for a, b in zip(_volumes(db, s), _volumes(want, s)):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (s, step1[s])
    # (a frame lost or fused twice moves thousands of voxels; the two histories themselves differ by the arithmetic of one frame)
    print('voxels that tell the two histories of %s apart: %d' % (scenes[0], int(
        (_volumes(db_again, scenes[0])[0].view(torch.int16) != _volumes(db_kept, scenes[0])[0].view(torch.int16)).sum())))


def test_single_frame_and_batched_2d_graphs_share_one_engine(cuda):
    """fuse() (B = 1 graph of the 2-D engine), fuse_many() (B = S graph), fuse() again on ONE pipeline: each captured graph
    addresses its own decoder concat buffers by raw pointer, so neither batch size may evict the other's (the
    second fuse() replayed into freed memory; the zero pad channels 280..287 could come back as NaN logits).  Volumes against
    pipelines that only ever ran one of the two paths, with the allocator's cache emptied in between."""
    h, w, grid, n_classes, S = 64, 96, 32, 12, 3
    scenes = tuple('room_%d' % k for k in range(S))
    _, ds_a, db_a, mixed = _predict_pipeline(cuda, h, w, grid, n_classes, scenes)
    _, ds_b, db_b, single = _predict_pipeline(cuda, h, w, grid, n_classes, scenes)
    single.load_state_dict(mixed.state_dict())

    def batch(ds, s, i):
        return {k: (v.to(cuda) if torch.is_tensor(v) else v) for k, v in ds.streams[s].batch(i).items()}
    with torch.no_grad():
        for rnd in range(2):
            i0 = 3 * rnd
            for s in scenes:
                mixed.fuse(batch(ds_a, s, i0), db_a, cuda)
            torch.cuda.synchronize(); torch.cuda.empty_cache()
            junk = torch.full((64 << 20,), float('nan'), device=cuda)  # whatever was freed is NaN now
            mixed.fuse_many([batch(ds_a, s, i0 + 1) for s in scenes], db_a, cuda)
            del junk
            torch.cuda.synchronize(); torch.cuda.empty_cache()
            junk = torch.full((64 << 20,), float('nan'), device=cuda)
            for s in scenes:
                mixed.fuse(batch(ds_a, s, i0 + 2), db_a, cuda)
            del junk
        mixed.check()
        # the label images of the mixed pipeline's LAST single-frame pass against a pipeline that never ran a batch
        for i in range(6):
            for s in scenes:
                single.fuse(batch(ds_b, s, i), db_b, cuda)
        single.check()
        b = batch(ds_a, scenes[0], 7)
        ids_m, sc_m = mixed._labels2d.frame_semantics(b, cuda)
        ids_s, sc_s = single._labels2d.frame_semantics(b, cuda)
        assert torch.isfinite(sc_m).all() and torch.equal(ids_m, ids_s) and torch.equal(sc_m, sc_s)
    for s in scenes:
        # geometry does not see the labels: bit for bit; labels: the batched pass's rounding at near-ties only
        assert torch.equal(db_a.scenes_est[s].volume.view(torch.int16), db_b.scenes_est[s].volume.view(torch.int16))
        assert torch.equal(db_a.fusion_weights[s].view(torch.int16), db_b.fusion_weights[s].view(torch.int16))
        touched = db_b.fusion_weights[s] > 0
        assert (db_a.ids_est[s].volume[touched] == db_b.ids_est[s].volume[touched]).float().mean().item() >= 0.999
        assert torch.isfinite(db_a.scores[s].volume.float()).all()


def test_a_tripped_2d_pass_is_loud_when_the_fusion_net_runs_fp32(cuda):
    """The 2-D engine's kernels are split-fp16 whatever FUSION_MODEL.arithmetic says, and they raise the same process-wide
    flag the integrate calls honour.  With arithmetic 'f32' the fusion net's forward does not poll it: the frame step itself
    must (every later frame was dropped silently until check()).  Volumes hold every frame before the event and
    nothing after it; the next fuse() raises; check() reports and clears."""
    from online_joint_depthfusion_and_semantic_amd import _lib
    h, w, grid, n_classes = 64, 96, 32, 12
    cfg, st, db, pipe = _predict_pipeline(cuda, h, w, grid, n_classes)
    cfg.FUSION_MODEL.arithmetic = 'f32'
    s = st.scene
    with torch.no_grad():
        pipe.fuse(_batch(st, 0, cuda), db, cuda)
        pipe.check()
        before = _volumes(db, s) + [db.ids_est[s].volume.clone(), db.scores[s].volume.clone()]
        pipe._semantic_2d_network.encoder_mod1.res_n50_enc.conv1.weight.mul_(1e12)  # the stem's output leaves the fp16 range
        raised = False
        for i in range(1, 4):
            try:
                pipe.fuse(_batch(st, i, cuda), db, cuda)
            except _lib.OjfError as err:
                assert 'fp16 range' in str(err)
                raised = True
                break
            torch.cuda.synchronize()  # (the flag is raised by the device: the NEXT frame step must see it)
        assert raised, 'three frames went by after the 2-D engine left the fp16 range and no fuse() raised'
        after = _volumes(db, s) + [db.ids_est[s].volume.clone(), db.scores[s].volume.clone()]
        for a, b in zip(before, after):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
        with pytest.raises(_lib.OjfError, match='fp16 range'):
            pipe.check()
        pipe.check()  # cleared


def test_segmentation_on_odd_frame_sizes_says_why(cuda):
    """AdapNet++ (modules/adapnet.py: three stride-2 stages up, x2 / x2 / x4 transposed convolutions down) only closes on frame
    sides that are multiples of 16 - the reference's module dies in a ``torch.cat`` of the decoder for anything else, and so
    does this package's module tree.  The HIP engine refuses such frames; the pipeline says so ONCE (a RuntimeWarning naming
    the constraint) before the module forward raises the reference's own error (the hand-over was silent)."""
    h, w, grid, n_classes = 40, 56, 32, 12
    cfg, st, db, pipe = _predict_pipeline(cuda, h, w, grid, n_classes)
    with torch.no_grad():
        with pytest.warns(RuntimeWarning, match='multiples of 16'), pytest.raises(RuntimeError):
            pipe.fuse(_batch(st, 0, cuda), db, cuda)
    assert pipe._labels2d.warned_seg_fallback is True


def test_announced_training_frames_change_no_bit(cuda):
    """Pipeline.announce_training_frame(next batch): the filtered frame and the valid-ray count of the next training frame are
    requested one frame ahead (the frame step's only host read; pipeline.py:125-131 reads it with a blocking ``nonzero``).  The same
    launches, earlier: outputs, gradients, BatchNorm buffers and volumes bit for bit those of the un-announced loop - in train()
    mode with Dropout2d active (the persistent mask buffer draws what the per-pass tensor drew) - also when the announced batch is
    NOT the one that comes, and across an optimizer step (the cached layer table must follow the weights)."""
    h, w, grid, frames = 48, 64, 64, 6

    def run(announce):
        torch.manual_seed(10)  # (the modules' default initialisation draws too)
        cfg, st, db, pipe = _setup(h, w, grid, False, False, 'fast', cuda)
        torch.manual_seed(11)
        for m in pipe._fusion_network.modules():
            if isinstance(m, torch.nn.Conv2d):
                torch.nn.init.xavier_normal_(m.weight)
        pipe.train()
        opt = torch.optim.RMSprop(pipe._fusion_network.parameters(), lr=1e-3)
        torch.manual_seed(12)  # the Dropout2d draws
        batches = [_batch(st, i, cuda) for i in range(frames + 1)]
        outs, hits = [], []
        stranger = _batch(st, 0, cuda)
        for i in range(frames):
            if announce:  # frame 3 is announced wrongly (another object): its own count is computed in the call
                pipe.announce_training_frame(batches[i + 1] if i != 2 else stranger, cuda)
            out = pipe.fuse_training(batches[i], db, cuda)
            hits.append(pipe.announce_hits)
            # the stranger waits through frame 2 (the documented order: announced one frame step ahead), then it is dropped unused
            assert any(a[0] is stranger for a in pipe._announcements.held) == (announce and i == 2)
            assert len(pipe._announcements.held) <= 1
            loss = (out['tsdf_fused'] - out['tsdf_target']).abs().mean()
            loss.backward()
            outs.append((out['tsdf_est'].detach().clone(), out['tsdf_fused'].detach().clone(), loss.detach().clone()))
            if i % 2 == 1:
                opt.step()
                opt.zero_grad(set_to_none=False)
        torch.cuda.synchronize()
        # frames 1, 2, 4 and 5 arrive announced; frame 0 never was, and frame 3's announcement was the stranger
        assert (pipe.announce_hits, pipe.announce_misses) == ((4, 2) if announce else (0, frames))
        assert hits == ([0, 1, 2, 2, 3, 4] if announce else [0] * frames)
        pipe.announce_training_frame(batches[frames], cuda)
        pipe.announce_training_frame(None)
        assert pipe._announcements.held == []
        net = pipe._fusion_network
        return (outs, [p.detach().clone() for p in net.parameters()], [b.detach().clone() for b in net.buffers()],
                [db.scenes_est[st.scene].volume.clone(), db.fusion_weights[st.scene].clone()])
    a, b = run(True), run(False)
    for (e1, f1, l1), (e2, f2, l2) in zip(a[0], b[0]):
        assert torch.equal(e1, e2) and torch.equal(f1, f2) and torch.equal(l1, l2)
    for x, y in zip(a[1] + a[2], b[1] + b[2]):
        assert torch.equal(x, y)
    for x, y in zip(a[3], b[3]):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16))
    assert float((a[3][1].float() > 0).sum()) > 1000


@pytest.mark.parametrize('replay,thread', [(False, False), (True, False), (False, True)])
def test_backward_beside_the_next_forward_stage_changes_no_bit(cuda, replay, thread):
    """FUSION_MODEL.train_overlap: the backward pass of frame k on the pipeline's gradient stream beside the forward stage of frame
    k + 1 (two executors take turns; gradient clipping, optimizer step and zero_grad inside ``with pipeline.gradients():``).  The
    reference's loop order (train_fusion.py:160-189) is kept by stream dependencies instead of by one queue: outputs, losses,
    parameters, BatchNorm buffers, accumulated gradients and volumes of ten train()-mode frames with Dropout2d and an RMSprop step
    every third frame are bit for bit those of the serial loop - also with the executor's passes replayed as device graphs, and with the
    backward pass's launches and the gradient work enqueued by the pipeline's gradient thread (``gradient_work``)."""
    h, w, grid, frames = 48, 64, 64, 10

    def run(overlap):
        torch.manual_seed(10)
        cfg, st, db, pipe = _setup(h, w, grid, False, False, 'fast', cuda)
        cfg.FUSION_MODEL.train_overlap = overlap
        cfg.FUSION_MODEL.train_replay = replay and overlap
        cfg.FUSION_MODEL.train_overlap_thread = thread
        torch.manual_seed(11)
        for m in pipe._fusion_network.modules():
            if isinstance(m, torch.nn.Conv2d):
                torch.nn.init.xavier_normal_(m.weight)
        pipe.train()
        net = pipe._fusion_network
        opt = torch.optim.RMSprop(net.parameters(), lr=1e-3)
        torch.manual_seed(12)  # the Dropout2d draws
        batches = [_batch(st, i, cuda) for i in range(frames)]
        outs = []
        for i in range(frames):
            out = pipe.fuse_training(batches[i], db, cuda)
            loss = (out['tsdf_fused'] - out['tsdf_target']).abs().mean()
            loss.backward()
            outs.append((out['tsdf_est'].detach().clone(), out['tsdf_fused'].detach().clone(), loss.detach().clone()))
            def gradient_step(i=i):
                torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0)
                if i % 3 == 2:
                    opt.step()
                    opt.zero_grad(set_to_none=False)
            if thread:  # the function form: enqueued by the pipeline's gradient thread, this thread waits only where the weights change
                pipe.gradient_work(gradient_step, join=i % 3 == 2)
            else:
                with pipe.gradients():
                    gradient_step()
        pipe.join_gradients()
        grads = [p.grad.detach().clone() for p in net.parameters() if p.grad is not None]
        torch.cuda.synchronize()
        tn = pipe.__dict__['_hip_train']
        assert tn.overlap == overlap and (len(tn._trainers) == (2 if overlap else 1))
        if replay and overlap:
            assert tn.replays >= 8
        return (outs, [p.detach().clone() for p in net.parameters()], [b.detach().clone() for b in net.buffers()], grads,
                [db.scenes_est[st.scene].volume.clone(), db.fusion_weights[st.scene].clone()])
    a, b = run(True), run(False)
    for (e1, f1, l1), (e2, f2, l2) in zip(a[0], b[0]):
        assert torch.equal(e1, e2) and torch.equal(f1, f2) and torch.equal(l1, l2)
    assert len(a[3]) == len(b[3]) > 100
    for x, y in zip(a[1] + a[2] + a[3], b[1] + b[2] + b[3]):
        assert torch.equal(x, y)
    for x, y in zip(a[4], b[4]):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16))


def test_optimizer_step_outside_the_gradient_context_is_loud(cuda):
    """train_overlap moves the backward pass to the gradient stream: an optimizer step on the caller's stream would run beside the
    backward pass it needs.  The next fuse_training sees the parameters' version counters move without a gradients() section (or a
    join) since that backward pass and raises instead of training on half-written gradients; behind join_gradients() the plain loop
    of train_fusion.py:182-189 is fine."""
    h, w, grid = 48, 64, 64
    torch.manual_seed(10)
    cfg, st, db, pipe = _setup(h, w, grid, False, False, 'fast', cuda)
    cfg.FUSION_MODEL.train_overlap = True
    pipe.train()
    net = pipe._fusion_network
    opt = torch.optim.RMSprop(net.parameters(), lr=1e-4)
    batches = [_batch(st, i, cuda) for i in range(4)]

    def frame(i):
        out = pipe.fuse_training(batches[i], db, cuda)
        (out['tsdf_fused'] - out['tsdf_target']).abs().mean().backward()
    frame(0)
    frame(1)  # (steady state: from the second pass on the backward pass runs on the gradient stream)
    pipe.join_gradients()
    opt.step()  # behind a join: allowed
    frame(2)
    opt.step()  # NOT behind anything
    with pytest.raises(Exception, match='outside `with pipeline.gradients'):
        frame(3)
    pipe.join_gradients()
    torch.cuda.synchronize()
