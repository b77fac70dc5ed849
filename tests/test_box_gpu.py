"""-m gpu: the volume kernels on NON-CUBIC boxes whose origin components all differ (box_cases.py; test_box_host.py shows
that these inputs tell the axes apart): extract / integrate against the CPU oracle with the bars of
test_extract_integrate_gpu.py, the ray caster against render_ref (depth and labels bit for bit, normals within 1e-6) with
odd image sizes, near > 0 and axis-parallel rays, and the tracker against track_ref on odd frame sizes."""
import numpy as np
import pytest
import torch

from oracle import oracle
from online_joint_depthfusion_and_semantic_amd import _lib, ops
from online_joint_depthfusion_and_semantic_amd.render import render_views
from online_joint_depthfusion_and_semantic_amd.tracking import track_frame
from helpers import n_mismatch, f16_ulp_distance, fresh_volumes, frame_inputs, to_cuda, make_stream
import box_cases
from box_cases import BOXES, FRAME_SIZES, box, oracle_run
from stream_ops_cases import Guarded
from test_extract_integrate_gpu import FAST_MOVED_FRACTION
import track_ref

pytestmark = pytest.mark.gpu

ROLL = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], dtype=np.float32)
BOX_SIZES = [(name, h, w) for name in sorted(BOXES) for h, w in FRAME_SIZES]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _stream(h, w, **kw):
    return make_stream(h, w, box_cases.STREAM_GRID, box_cases.STREAM_FRAMES, **kw)


def _random_volumes(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.1, 0.1, shape).astype(np.float16), rng.uniform(0, 6, shape).astype(np.float16)


# ---- extract -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rolled', [False, True])
@pytest.mark.parametrize('name,h,w', BOX_SIZES)
def test_extract_bit_exact_on_a_box(cuda, name, h, w, rolled):
    """Indices, corner weights, points, point cloud and sample rows of ops.extract(debug=True) on pre-filled random volumes
    of the box shape: zero mismatches against the oracle, upright (column tiles) and with the camera rolled by 90 degrees
    (row tiles; test_extract_bit_exact_for_a_rolled_camera)."""
    origin, res, shape = box(name)
    st = _stream(h, w)
    tsdf, wgt = _random_volumes(shape, 3)
    g_tsdf, g_wgt = _t(tsdf, cuda), _t(wgt, cuda)
    for i in BOXES[name]['frames']:
        fi = frame_inputs(st, i)
        E = fi['E']
        if rolled:
            E = E.reshape(3, 4).copy()
            assert abs(E[2, 1]) > abs(E[2, 0])  # upright: the camera's y axis carries the volume's z
            E[:, :3] = E[:, :3] @ ROLL
            assert abs(E[2, 0]) > abs(E[2, 1])
            E = np.ascontiguousarray(E.reshape(12))
        ref = oracle.extract(fi['depth'], fi['Ki'], E, origin, res, tsdf, wgt, debug=True)
        out = ops.extract(_t(fi['depth'], cuda), fi['Ki'], E, origin, res, g_tsdf, g_wgt, debug=True)
        bad = {key: n_mismatch(out[key].cpu().numpy(), ref[key]) for key in ref}
        print('extract %s %dx%d rolled=%s frame %d: mismatches %s' % (name, h, w, rolled, i, bad))
        assert not any(bad.values()), (i, bad)
        planes = ops.extract(_t(fi['depth'], cuda), fi['Ki'], E, origin, res, g_tsdf, g_wgt, planes=True)
        assert n_mismatch(planes['fusion_values'].t().contiguous().cpu().numpy(), ref['fusion_values']) == 0, i
        assert n_mismatch(planes['fusion_weights'].t().contiguous().cpu().numpy(), ref['fusion_weights']) == 0, i
    assert (ref['fusion_weights'] > 0).any() and (ref['fusion_weights'] == 0).any()  # (rays inside and outside the box)


def test_extract_to_net_on_a_box(cuda):
    """ojf_extract_to_net on ``room`` at 13x15: the same net output bits as planes=True extract + prepare_input."""
    from online_joint_depthfusion_and_semantic_amd import model
    from online_joint_depthfusion_and_semantic_amd.engine import FusionNetEngine
    from helpers import NS
    h, w = 13, 15
    origin, res, shape = box('room')
    fi = frame_inputs(_stream(h, w), 3)
    tsdf, wgt = _random_volumes(shape, 5)
    wgt[:, :, ::3] = 0
    tsdf, wgt, depth = _t(tsdf, cuda), _t(wgt, cuda), _t(fi['depth'], cuda)
    torch.manual_seed(0)
    net = model.FusionNet_v3(NS(n_points=9, growth_factor=6, use_semantics=False, output_scale=1.0, resx=w, resy=h))
    for m in net.modules():
        if isinstance(m, torch.nn.Conv2d):
            torch.nn.init.xavier_normal_(m.weight)
    eng = FusionNetEngine(net.eval(), h, w, cuda)
    assert eng.fused_input
    fv, fw = torch.empty((9, h * w), device=cuda), torch.empty((9, h * w), device=cuda)
    ops.extract(depth, fi['Ki'], fi['E'], origin, res, tsdf, wgt, out_values=fv, out_weights=fw, out_stride=h * w, planes=True)
    eng.prepare_input(fv, fw, depth, planes=True)
    a = eng.forward(torch.zeros((h * w, 9), device=cuda)).clone()
    eng.prepare_input(torch.zeros_like(fv), torch.zeros_like(fw), torch.zeros_like(depth), planes=True)  # wipe the slot
    ops.extract_to_net(depth, fi['Ki'], fi['E'], origin, res, tsdf, wgt, eng)
    b = eng.forward(torch.zeros((h * w, 9), device=cuda))
    assert torch.isfinite(a).all() and float(a.abs().max()) > 0
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    eng.close()


# ---- integrate -----------------------------------------------------------------------------------------------------------
def _integrate(name, fi, g, ws, mode, semantics, cuda, **kw):
    origin, res, _ = box(name)
    if semantics:
        kw.update(sem_ids=_t(fi['sem_ids'].reshape(-1), cuda), sem_scores=_t(fi['sem_scores'].reshape(-1), cuda),
                  id_vol=g['ids'], score_vol=g['scores'])
    ops.integrate(_t(fi['fd'], cuda), fi['Ki'], fi['E'], origin, res, _t(fi['est'], cuda), g['tsdf'], g['wgt'], ws,
                  mode=mode, stats=True, **kw)


def _keys(semantics):
    return ('tsdf', 'wgt', 'ids', 'scores') if semantics else ('tsdf', 'wgt')


@pytest.mark.parametrize('semantics', [False, True])
@pytest.mark.parametrize('name,h,w', BOX_SIZES)
def test_integrate_parity_mode_bit_exact_on_a_box(cuda, name, h, w, semantics):
    shape = box(name)[2]
    run = oracle_run(name, h, w)
    g = to_cuda({k: run[0]['pre'][k] for k in _keys(semantics)}, cuda)
    ws = ops.IntegrateWorkspace(shape, h, w, 7, ops.MODE_PARITY, cuda)
    for r in run:
        _integrate(name, r['fi'], g, ws, ops.MODE_PARITY, semantics, cuda)  # state carried on both sides
        bad = {key: n_mismatch(g[key].cpu().numpy(), r['post'][key]) for key in g}
        print('parity %s %dx%d sem=%s frame %d: mismatches %s, touched %d' % (name, h, w, semantics, r['i'], bad, r['touched']))
        assert not any(bad.values()), (r['i'], bad)
        assert int(ws.stats[0].item()) == r['touched']


@pytest.mark.parametrize('semantics', [False, True])
@pytest.mark.parametrize('name,h,w', BOX_SIZES)
def test_integrate_fast_mode_tolerance_on_a_box(cuda, name, h, w, semantics):
    """FAST from a common pre-frame state: the NaN pattern equal, <= 1 fp16 ulp, ids and scores bit for bit, the touched
    count the oracle's, the workspace left clean.  The moved-voxel share is held to the coarse-grid bar of
    test_extract_integrate_gpu.py on ``room`` at 45x52 over its four frames (~39 k touched); elsewhere the few thousand
    touched voxels make a 1e-3 share a coin toss and the count is printed only."""
    shape = box(name)[2]
    run = oracle_run(name, h, w)
    ws = ops.IntegrateWorkspace(shape, h, w, 7, ops.MODE_FAST, cuda)
    moved, touched = {'tsdf': 0, 'wgt': 0}, 0
    for r in run:
        g = to_cuda({k: r['pre'][k] for k in _keys(semantics)}, cuda)  # common pre-frame state
        _integrate(name, r['fi'], g, ws, ops.MODE_FAST, semantics, cuda)
        assert int(ws.stats[0].item()) == r['touched']
        touched += r['touched']
        for key in ('tsdf', 'wgt'):
            got, want = g[key].cpu().numpy(), r['post'][key]
            assert (np.isnan(got) == np.isnan(want)).all(), (key, r['i'])
            ulp = np.where(np.isnan(got), 0, f16_ulp_distance(got, want))
            assert ulp.max() <= 1, (key, r['i'], int(ulp.max()))
            moved[key] += int((ulp > 0).sum())
        if semantics:
            assert n_mismatch(g['ids'].cpu().numpy(), r['post']['ids']) == 0, r['i']
            assert n_mismatch(g['scores'].cpu().numpy(), r['post']['scores']) == 0, r['i']
    print('fast-mode %s %dx%d sem=%s: %s of %d touched voxels moved by one ulp' % (name, h, w, semantics, moved, touched))
    if (name, h, w) == ('room', 45, 52):
        for key in moved:
            assert moved[key] <= max(2, FAST_MOVED_FRACTION[64] * touched), (key, moved[key], touched)
    # the workspace must be left clean: an all-masked frame touches nothing
    fi = dict(run[0]['fi'])
    fi['fd'] = np.zeros_like(fi['fd'])
    last = {k: run[-1]['post'][k] for k in _keys(semantics)}
    g = to_cuda(last, cuda)
    _integrate(name, fi, g, ws, ops.MODE_FAST, semantics, cuda)
    assert int(ws.stats[0].item()) == 0
    for key in g:
        assert n_mismatch(g[key].cpu().numpy(), last[key]) == 0, key


@pytest.mark.parametrize('semantics', [False, True])
@pytest.mark.parametrize('name,h,w', [('room', 45, 52), ('slab', 13, 15)])
def test_many_scene_launches_on_a_box(cuda, name, h, w, semantics):
    """ojf_extract_many / ojf_integrate_many with two scenes of one box: bit for bit the separate calls."""
    origin, res, shape = box(name)
    S, n_tail = 2, 7
    streams = [_stream(h, w, scene='room_%d' % s, seed=1911 + 17 * s) for s in range(S)]
    one = [to_cuda(fresh_volumes(shape, semantics), cuda) for _ in range(S)]
    many = [to_cuda(fresh_volumes(shape, semantics), cuda) for _ in range(S)]
    ws_one = ops.IntegrateWorkspace(shape, h, w, n_tail, ops.MODE_FAST, cuda)
    ws_many = [ops.IntegrateWorkspace(shape, h, w, n_tail, ops.MODE_FAST, cuda) for _ in range(S)]
    frames = BOXES[name]['frames']
    for step in range(2):
        fis = [frame_inputs(st, frames[(step + s) % len(frames)]) for s, st in enumerate(streams)]
        depth = [_t(fi['depth'], cuda) for fi in fis]
        mask = [_t(fi['fd'] != 0, cuda) for fi in fis]
        est = [_t(fi['est'], cuda) for fi in fis]
        ids = [_t(fi['sem_ids'].reshape(-1), cuda) for fi in fis]
        sc = [_t(fi['sem_scores'].reshape(-1), cuda) for fi in fis]
        ref = [ops.extract(depth[s], fis[s]['Ki'], fis[s]['E'], origin, res, one[s]['tsdf'], one[s]['wgt'], planes=True)
               for s in range(S)]
        outs = [(torch.empty((9, h * w), device=cuda), torch.empty((9, h * w), device=cuda)) for _ in range(S)]
        ops.extract_many([dict(depth=depth[s], Ki=fis[s]['Ki'], E=fis[s]['E'], origin=origin, resolution=res, tsdf=many[s]['tsdf'],
                               weights=many[s]['wgt'], out_values=outs[s][0], out_weights=outs[s][1]) for s in range(S)])
        for s in range(S):
            assert torch.equal(ref[s]['fusion_values'].view(torch.int32), outs[s][0].view(torch.int32)), (step, s)
            assert torch.equal(ref[s]['fusion_weights'].view(torch.int32), outs[s][1].view(torch.int32)), (step, s)
        for s in range(S):
            kw = dict(sem_ids=ids[s], sem_scores=sc[s], id_vol=one[s]['ids'], score_vol=one[s]['scores']) if semantics else {}
            ops.integrate(depth[s], fis[s]['Ki'], fis[s]['E'], origin, res, est[s], one[s]['tsdf'], one[s]['wgt'], ws_one,
                          n_tail=n_tail, mask=mask[s], **kw)
        ops.integrate_many([dict(depth=depth[s], mask=mask[s], Ki=fis[s]['Ki'], E=fis[s]['E'], origin=origin, resolution=res,
                                 est=est[s], tsdf=many[s]['tsdf'], weights=many[s]['wgt'], workspace=ws_many[s],
                                 **(dict(sem_ids=ids[s], sem_scores=sc[s], id_vol=many[s]['ids'], score_vol=many[s]['scores'])
                                    if semantics else {})) for s in range(S)], n_tail=n_tail)
        for s in range(S):
            for k in one[s]:
                assert torch.equal(one[s][k].view(torch.uint8), many[s][k].view(torch.uint8)), (step, s, k)
    assert float((many[0]['wgt'].float() > 0).sum()) > 100
    assert not torch.equal(many[0]['wgt'], many[1]['wgt'])  # (the scenes differ)


@pytest.mark.parametrize('mode', [ops.MODE_FAST, ops.MODE_PARITY])
@pytest.mark.parametrize('name,h,w', [('room', 13, 15), ('slab', 45, 52)])
def test_masked_integrate_equals_filtered_frame_on_a_box(cuda, name, h, w, mode):
    origin, res, shape = box(name)
    st = _stream(h, w)
    vols = fresh_volumes(shape, True)
    a, b = to_cuda(vols, cuda), to_cuda(vols, cuda)
    ws = ops.IntegrateWorkspace(shape, h, w, 7, mode, cuda)
    rng = np.random.default_rng(4)
    for i in BOXES[name]['frames']:
        fi = frame_inputs(st, i)
        raw = fi['depth'].astype(np.float32).copy()
        mask = rng.random((h, w)) > 0.3
        raw[~mask & (rng.random((h, w)) > 0.5)] = np.nan  # what the mask hides may be anything
        filt = np.where(mask, raw, np.float32(0)).astype(np.float32)
        ids, sc, est = _t(fi['sem_ids'].reshape(-1), cuda), _t(fi['sem_scores'].reshape(-1), cuda), _t(fi['est'], cuda)
        ops.integrate(_t(filt, cuda), fi['Ki'], fi['E'], origin, res, est, a['tsdf'], a['wgt'], ws, mode=mode,
                      sem_ids=ids, sem_scores=sc, id_vol=a['ids'], score_vol=a['scores'])
        ops.integrate(_t(raw, cuda), fi['Ki'], fi['E'], origin, res, est, b['tsdf'], b['wgt'], ws, mode=mode,
                      mask=torch.from_numpy(mask).to(cuda), sem_ids=ids, sem_scores=sc, id_vol=b['ids'], score_vol=b['scores'])
    assert int((a['wgt'].float() > 0).sum()) > 200
    for key in a:
        assert torch.equal(a[key].view(torch.uint8), b[key].view(torch.uint8)), key


@pytest.mark.parametrize('semantics', [False, True])
def test_reference_style_modules_on_the_slab(cuda, semantics):
    """The drop-in Extractor / Integrator modules with the reference's call signatures, Integrator.forward through
    ojf_integrate_entries (the entry-list path of ops), on ``slab`` at 45x52."""
    from online_joint_depthfusion_and_semantic_amd.config import default_config
    from online_joint_depthfusion_and_semantic_amd.extractor import Extractor
    from online_joint_depthfusion_and_semantic_amd.integrator import Integrator
    name, h, w = 'slab', 45, 52
    origin, res, shape = box(name)
    cfg = default_config(h, w, semantics=semantics)
    cfg.SETTINGS.device = str(cuda)
    ex, ig = Extractor(cfg), Integrator(cfg)
    st = _stream(h, w)
    for r in oracle_run(name, h, w):
        b, fi = st.batch(r['i']), r['fi']
        g = to_cuda({k: r['pre'][k] for k in _keys(semantics)}, cuda)  # common pre-frame state
        out = ex.forward(b['tof_depth'].to(cuda), b['extrinsics'], b['intrinsics'], g['tsdf'], g['wgt'],
                         torch.from_numpy(origin), res)
        ref = oracle.extract(fi['depth'], fi['Ki'], fi['E'], origin, res, r['pre']['tsdf'], r['pre']['wgt'], debug=True)
        for key in ('fusion_values', 'indices', 'weights'):
            assert n_mismatch(out[key][0].cpu().numpy(), ref[key]) == 0, (key, r['i'])
        est = _t(fi['est'], cuda).view(1, h * w, 9)
        valid = (_t(fi['fd'], cuda).view(1, h * w, 1) != 0).nonzero()[:, 1]
        updates = dict(values=torch.clamp(est[:, valid, :7], -0.1, 0.1), indices=out['indices'][:, valid, :7],
                       weights=out['weights'][:, valid, :7])
        if semantics:
            rep = lambda t: t.view(1, h * w, 1).unsqueeze(-2).repeat(1, 1, 9, 1)[:, valid, :7]  # noqa: E731
            updates['semantics'] = rep(_t(fi['sem_ids'], cuda))
            updates['scores'] = rep(_t(fi['sem_scores'], cuda))
        ret = ig.forward(updates, g['tsdf'], g['wgt'], g.get('scores'), g.get('ids'))
        assert ret[0] is g['tsdf'] and ret[1] is g['wgt']
        assert int(ig._entry_ws.stats[0].item()) == r['touched']
        for key in ('tsdf', 'wgt'):
            got = g[key].cpu().numpy()
            ulp = np.where(np.isnan(got), 0, f16_ulp_distance(got, r['post'][key]))
            assert ulp.max() <= 1 and (np.isnan(got) == np.isnan(r['post'][key])).all(), (key, r['i'])
        if semantics:
            assert n_mismatch(g['ids'].cpu().numpy(), r['post']['ids']) == 0
            assert n_mismatch(g['scores'].cpu().numpy(), r['post']['scores']) == 0


# ---- ray caster ----------------------------------------------------------------------------------------------------------
def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = got.view(np.uint8).reshape(got.size, -1) != want.view(np.uint8).reshape(want.size, -1)
    n_bad = int(bad.any(axis=1).sum())
    assert n_bad == 0, '{}: {} of {} elements differ'.format(what, n_bad, got.size)


def _dev(a, cuda):
    return None if a is None else _t(a, cuda)


_RENDERED = {}


def _rendered(tag, cuda):
    """render_views of box_cases.render_cases()[tag], checked against render_ref: (depth, normals, labels) on the host."""
    if tag not in _RENDERED:
        c = box_cases.render_cases()[tag]
        out = render_views(_dev(c['tsdf'], cuda), _dev(c['weights'], cuda), _dev(c['ids'], cuda), origin=c['origin'],
                           resolution=c['res'], intrinsics=c['K'], extrinsics=c['E'], shape=c['shape'], near=c['near'])
        depth, normals, labels = box_cases.render_reference(tag)
        got_d, got_n = out['depth'].cpu().numpy(), out['normals'].cpu().numpy()
        got_l = labels if out['labels'] is None else out['labels'].cpu().numpy()
        print('render %s: %d depth, %d label mismatches, max |dn| %.1e' % (
            tag, n_mismatch(got_d, depth), n_mismatch(got_l, labels), float(np.abs(got_n - normals).max())))
        _same_bits(got_d, depth, tag + ' depth')
        if c['ids'] is not None:
            _same_bits(got_l, labels, tag + ' labels')
        assert np.abs(got_n - normals).max() <= 1e-6, tag
        _RENDERED[tag] = (got_d, got_n, got_l)
    return _RENDERED[tag]


@pytest.mark.parametrize('tag', ['gt-near0', 'gt-near1.5', 'holes-near0', 'holes-near1.5', 'axis', 'thin'])
def test_render_is_the_restatement_on_a_box(cuda, tag):
    """``room`` GT volume (66 x 62 x 37) at 37x53 - no multiple of the 8x8 tiles - from three orbit poses with near = 0
    and 1.5, with labels, without and with a weight volume that is zero on [:, 20:30]; four views with axis-parallel
    rays (the dv_i == 0 branch of the slab test); a volume two voxels thin."""
    _rendered(tag, cuda)


def test_render_cases_show_what_they_are_for(cuda):
    box_cases.check_render_conditions(lambda tag: _rendered(tag, cuda))


def test_render_writes_nothing_outside_its_images(cuda):
    """ojf_render on sentinel-guarded depth, normal and label buffers: the axis-parallel views at 37x53."""
    c = box_cases.render_cases()['axis']
    from render_ref import cameras
    Ki, E, _ = cameras(c['K'], c['E'], c['origin'], c['res'])
    n, (h, w) = len(E), c['shape']
    tsdf, ids = _t(c['tsdf'], cuda), _t(c['ids'], cuda)
    X, Y, Z = tsdf.shape
    depth = Guarded(cuda, n * h * w, 1, dtype=np.float32)
    normals = Guarded(cuda, n * h * w, 3, dtype=np.float32)
    labels = Guarded(cuda, n * h * w, 1, dtype=np.uint8)
    org = np.ascontiguousarray(c['origin'], dtype=np.float64)
    Ki, E = np.ascontiguousarray(Ki, np.float32), np.ascontiguousarray(E, np.float32)
    rc = _lib.load().ojf_render(_lib.ptr(tsdf), None, _lib.ptr(ids), X, Y, Z, org.ctypes.data, float(c['res']), n, Ki.ctypes.data,
                                E.ctypes.data, h, w, 0.0, depth.ptr, normals.ptr, labels.ptr, _lib.stream_ptr(cuda))
    _lib.check(rc, 'ojf_render')
    torch.cuda.synchronize()
    want_d, want_n, want_l = box_cases.render_reference('axis')
    _same_bits(depth.read().reshape(n, h, w), want_d, 'depth')
    _same_bits(labels.read().reshape(n, h, w), want_l, 'labels')
    assert np.abs(normals.read().reshape(n, h, w, 3) - want_n).max() <= 1e-6


# ---- tracker -------------------------------------------------------------------------------------------------------------
def _track_case(h, w, cuda):
    origin, res, _ = box('room')
    tsdf = _t(box_cases.room_gt(box_cases.RENDER_TRUNC)[0], cuda)

    def render(K, E, shape):
        r = render_views(tsdf, None, origin=origin, resolution=res, intrinsics=K, extrinsics=E, shape=shape)
        return r['depth'][0].cpu().numpy(), r['normals'][0].cpu().numpy()
    return tsdf, origin, res, box_cases.track_case(h, w, render)


@pytest.mark.parametrize('h,w', box_cases.TRACK_SIZES)
def test_tracker_is_the_restatement_on_odd_frames(cuda, h, w):
    """ojf_track_associate at 37x53 (levels 18x26 and 9x13: a row or a column is dropped at every level) and 45x77 (3465
    pixels: four associate blocks, the last with whole idle waves), model images of the ``room`` GT volume: pyramid, J, r
    and the reason codes bit for bit, the sums within 1e-12 of sum |terms|, status and pose track_ref.step's to 1e-12 - the
    degenerate level 2 (code 2) included."""
    from test_track_gpu import _associate
    _, _, _, case = _track_case(h, w, cuda)
    want = box_cases.track_restatement(case)
    assert [lv['code'] for lv in want] == [0, 0, 2]
    for l, (md, mn, Ki) in enumerate(case['models']):
        out = _associate(cuda, case['depth'], case['mask'], l, case['K'], Ki, _t(md, cuda), _t(mn, cuda), case['E_ref'],
                         case['E_ref'])
        lv = want[l]
        for k in range(l + 1):
            _same_bits(out['pyr'][k], want[k]['D'], 'pyramid level %d (call of level %d)' % (k, l))
        _same_bits(out['reason'], lv['reason'], 'reason codes, level %d' % l)
        _same_bits(out['J'], lv['J'], 'J, level %d' % l)
        _same_bits(out['r'], lv['r'], 'r, level %d' % l)
        bound = 1e-12 * np.abs(lv['terms']).sum(axis=0)
        err = np.abs(out['sums'] - lv['sums'])
        print('track %dx%d level %d: %d inliers, sums within %.2g of the bound, status %d' % (
            h, w, l, int(out['sums'][28]), float((err / np.maximum(bound, 1e-300)).max()), int(out['status'][0])))
        assert (err <= bound).all(), err / np.maximum(bound, 1e-300)
        assert out['sums'][28] == (lv['reason'] == 0).sum()
        code, P = track_ref.step(out['sums'], case['E_ref'], 0.05 * lv['D'].size)
        assert code == lv['code'] and int(out['status'][0]) == code
        assert np.abs(out['pose'] - P).max() <= 1e-12


@pytest.mark.parametrize('h,w', box_cases.TRACK_SIZES)
def test_track_frame_repeats_on_odd_frames(cuda, h, w):
    tsdf, origin, res, case = _track_case(h, w, cuda)
    kw = dict(origin=origin, resolution=res, depth=case['depth'], mask=case['mask'], intrinsics=case['K'],
              extrinsics=case['E_ref'], levels=box_cases.TRACK_LEVELS)
    a, b = track_frame(tsdf, None, **kw), track_frame(tsdf, None, **kw)
    assert a['status'] == b['status'] and a['stats'].shape == (19, 4)
    _same_bits(a['extrinsics'], b['extrinsics'], 'pose')
    _same_bits(a['stats'], b['stats'], 'stats')
