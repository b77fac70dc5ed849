"""-m gpu: the whole tracking call, step by step.  One iteration of ojf_track must be, bit for bit, what
ojf_track_associate produces from the pose the previous iteration left (the same kernels with the same argument fill), and
ojf_track_associate is pinned to the numpy restatement (track_ref.py: pyramid, J, r and the reason codes bit for bit, the
sums within 1e-12 of sum |terms|, the pose within 1e-12): the chain has no free number in it.  Covered: the host loop of
ojf_track (per-level arguments, the iteration counter, idle levels, one level, no iterations), level 3, the frozen path
after a failure that is not the first step (codes 1, 2 and 3), the pyramid kernel on inputs the synthetic stream never
makes, non-default thresholds and arbitrary model maps, the LDS chunk edges of the solve, and track_frame's marshalling.
The cases are analytic (track_cases.py); test_track_steps_host.py shows on the restatement what each relies on."""
import numpy as np
import pytest
import torch

from online_joint_depthfusion_and_semantic_amd import _lib, synthetic
from online_joint_depthfusion_and_semantic_amd.ops import camera_arrays
from online_joint_depthfusion_and_semantic_amd.render import render_views
from online_joint_depthfusion_and_semantic_amd.tracking import level_intrinsics, pose12, track_frame
from test_track_gpu import _associate, _same_bits
import track_cases
import track_ref

pytestmark = pytest.mark.gpu

POISON = 0x7f


def _upload(cuda, case):
    """The case's frame and model maps on the device: dict(depth, mask, models [(depth, normals, Kinv)])."""
    def up(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(cuda)
    return dict(depth=up(case['depth'], np.float32), mask=None if case['mask'] is None else up(case['mask'], np.uint8),
                models=[(up(md, np.float32), up(mn, np.float32), Ki) for md, mn, Ki, _ in case['models']])


def _track(cuda, dev, case, iterations, rows):
    """One raw ojf_track call into buffers filled with 0x7f bytes: dict(pose f64[3,4], stats f64[rows,4], status i32[2],
    stats_bytes u8[rows,32])."""
    lib = _lib.load()
    h, w, levels = case['h'], case['w'], case['levels']
    its = np.ascontiguousarray(list(iterations) + [0] * (4 - len(iterations)), dtype=np.int32)
    assert int(its.sum()) <= rows
    K = np.ascontiguousarray(np.asarray(case['K'], np.float64).reshape(9))
    Kinv = np.ascontiguousarray(np.stack([Ki for _, _, Ki in dev['models']]), dtype=np.float32)
    md = np.array([_lib.ptr(m[0]) for m in dev['models']], dtype=np.uint64)
    mn = np.array([_lib.ptr(m[1]) for m in dev['models']], dtype=np.uint64)
    E_ref, E_init = pose12(case['E_ref']), pose12(case['E_init'])
    ws = torch.full((int(lib.ojf_track_workspace_bytes(h, w, levels)),), POISON, dtype=torch.uint8, device=cuda)
    out = torch.full((96 + 32 * (rows + 1) + 8,), POISON, dtype=torch.uint8, device=cuda)
    stats_ptr = out.data_ptr() + 96
    status_ptr = stats_ptr + 32 * (rows + 1)
    rc = lib.ojf_track(_lib.ptr(dev['depth']), _lib.ptr(dev['mask']), h, w, levels, K.ctypes.data, Kinv.ctypes.data,
                       md.ctypes.data, mn.ctypes.data, E_ref.ctypes.data, E_init.ctypes.data, its.ctypes.data,
                       float(case['dist']), float(case['angle']), float(case['delta']), float(case['frac']), _lib.ptr(ws),
                       ws.numel(), out.data_ptr(), stats_ptr, status_ptr, _lib.stream_ptr(cuda))
    _lib.check(rc, 'ojf_track')
    host = out.cpu().numpy()
    raw = host[96:96 + 32 * (rows + 1)].reshape(rows + 1, 32)
    assert (raw[rows] == POISON).all(), 'a stats row past the last one was written'
    return dict(pose=host[:96].view(np.float64).reshape(3, 4).copy(), stats=raw[:rows].copy().view(np.float64).reshape(rows, 4),
                stats_bytes=raw[:rows].copy(), status=host[96 + 32 * (rows + 1):].view(np.int32).copy())


def _step_call(cuda, dev, case, level, pose, **kw):
    """ojf_track_associate at ``level`` of the case from ``pose``, with the case's thresholds."""
    md, mn, Ki = dev['models'][level]
    args = dict(dist=case['dist'], angle=case['angle'], delta=case['delta'], frac=case['frac'])
    args.update(kw)
    return _associate(cuda, case['depth'], case['mask'], level, case['K'], Ki, md, mn, case['E_ref'], pose, **args)


def _check_against_restatement(out, case, level, pose, what, dist=None, angle=None, pyr=None, nan_pixels=0):
    """The existing checks of one ojf_track_associate result against track_ref evaluated at ``pose``: pyramid, J, r and
    the reasons bit for bit, the sums within 1e-12 of sum |terms| and the count exact, the status and the pose
    track_ref.step's within 1e-12.  Returns (code, reason)."""
    md, mn, Ki, _ = case['models'][level]
    dist = case['dist'] if dist is None else dist
    angle = case['angle'] if angle is None else angle
    if pyr is None:
        pyr = track_ref.pyramid(case['depth'], case['mask'], level + 1, case['delta'])
    for l in range(level + 1):
        _same_bits(out['pyr'][l], pyr[l], '%s: pyramid level %d' % (what, l))
    J, r, reason = track_ref.associate(pyr[level], Ki, case['K'], level, md, mn, case['E_ref'], pose, dist, angle)
    _same_bits(out['reason'], reason, what + ': reason codes')
    _same_bits(out['J'], J, what + ': J')
    nan = np.isnan(r)
    assert int(nan.sum()) == nan_pixels and np.array_equal(np.isnan(out['r']), nan), what
    _same_bits(np.where(nan, np.float32(0), out['r']), np.where(nan, np.float32(0), r), what + ': r')
    with np.errstate(invalid='ignore'):
        terms = track_ref.term_matrix(J, r, reason)
        want = terms.sum(axis=0)
        bound = 1e-12 * np.abs(terms).sum(axis=0)
    finite = np.isfinite(want)
    assert np.array_equal(np.isnan(out['sums']), ~finite), (what, out['sums'])
    if nan_pixels:
        assert finite[:21].all() and finite[28] and not finite[21:28].any(), what
    err = np.abs(out['sums'] - want)[finite]
    assert (err <= bound[finite]).all(), (what, err / np.maximum(bound[finite], 1e-300))
    assert out['sums'][28] == (reason == 0).sum(), what
    code, P = track_ref.step(out['sums'], pose, case['frac'] * reason.size)
    assert int(out['status'][0]) == code, (what, out['status'], code)
    assert np.abs(out['pose'] - P).max() <= 1e-12, what
    return code, reason


@pytest.mark.parametrize('name', sorted(track_cases.STEP_CASES))
def test_every_step_of_the_call_is_one_associate_call(cuda, name):
    case = track_cases.step_case(name)
    dev = _upload(cuda, case)
    levels = case['levels']
    steps = track_ref.schedule(case['iterations'], levels)
    n = len(steps)
    assert track_ref.prefix_iterations(case['iterations'], levels, n) == list(case['iterations'])
    runs = [_track(cuda, dev, case, track_ref.prefix_iterations(case['iterations'], levels, k), n) for k in range(n + 1)]
    # no step: only the pyramid launch, which also writes the pose and the status
    _same_bits(runs[0]['pose'], case['E_init'][:3], 'pose of the call without iterations')
    for k, run in enumerate(runs):
        assert run['status'].tolist() == [0, -1], (name, k, run['status'])
        assert (run['stats_bytes'][k:] == POISON).all(), '%s: the call of %d steps wrote a later stats row' % (name, k)
        if k > 1:
            _same_bits(run['stats'][:k - 1], runs[k - 1]['stats'][:k - 1], 'stats rows before step %d' % (k - 1))
    pyr = track_ref.pyramid(case['depth'], case['mask'], levels, case['delta'])
    for k, l in enumerate(steps):
        what = 'case %s step %d (level %d)' % (name, k, l)
        P = runs[k]['pose']
        out = _step_call(cuda, dev, case, l, P)
        _same_bits(out['pose'], runs[k + 1]['pose'], what + ': pose')
        row = runs[k + 1]['stats'][k]
        sums = out['sums']
        _same_bits(row[:2], np.array([sums[28], sums[27] / sums[28]]), what + ': inlier count and mean squared residual')
        code, _, th, tau = track_ref.step(sums, P, case['frac'] * ((case['h'] >> l) * (case['w'] >> l)), moves=True)
        assert code == 0 and abs(row[2] - th) <= 1e-12 and abs(row[3] - tau) <= 1e-12, (what, row, th, tau)
        assert row[2] + row[3] > 1e-6, (what, row)
        # every pose the loop visits is checked against the restatement, not only E_ref
        code, reason = _check_against_restatement(out, case, l, P, what, pyr=pyr[:l + 1])
        assert code == 0 and (reason == 0).mean() >= 0.3, what
    free = track_cases.healthy_trace(name)[0]
    # a report, not an assertion: the fp32 rounding of the pose makes the free-running comparison discontinuous.  (The
    # angle from |Ra^T Rb - I|_F / sqrt 2: acos of the trace cannot resolve angles below 1e-6 deg.)
    dP = runs[n]['pose'] - free
    dr = np.degrees(np.linalg.norm(runs[n]['pose'][:, :3].T @ free[:, :3] - np.eye(3)) / np.sqrt(2.0))
    print('case %s: final pose of ojf_track vs the free-running restatement: %.3g m, %.3g deg (max |dP| %.3g)' % (
        name, np.linalg.norm(dP[:, 3]), dr, np.abs(dP).max()))


@pytest.fixture(scope='module')
def healthy_c(cuda):
    """Case C on the device, its whole healthy call and the poses before steps 2 and 4."""
    case = track_cases.step_case('C')
    dev = _upload(cuda, case)
    full = _track(cuda, dev, case, case['iterations'], 6)
    assert full['status'].tolist() == [0, -1]
    before = {k: _track(cuda, dev, case, track_ref.prefix_iterations(case['iterations'], 3, k), 6)['pose'] for k in (2, 4)}
    return dict(case=case, dev=dev, full=full, before=before)


@pytest.mark.parametrize('name', sorted(track_cases.failure_cases()))
def test_failure_after_the_first_step_freezes_the_call(cuda, healthy_c, name):
    case, code, index = track_cases.failure_cases()[name]
    dev = _upload(cuda, case)
    got = _track(cuda, dev, case, case['iterations'], 6)
    assert got['status'].tolist() == [code, index], (name, got['status'])
    _same_bits(got['pose'], case['E_init'][:3], name + ': the pose after a failure is E_init')
    assert not np.array_equal(healthy_c['before'][index], case['E_init'][:3])  # (the last good pose is another one)
    if code != 2:  # (the one-plane case runs with another min_inlier_fraction: its healthy prefix is its own)
        _same_bits(got['stats'][:index], healthy_c['full']['stats'][:index], name + ': stats rows before the failure')
    else:
        ok = dict(track_cases.step_case('C'), frac=case['frac'])
        _same_bits(got['stats'][:index], _track(cuda, healthy_c['dev'], ok, ok['iterations'], 6)['stats'][:index],
                   name + ': stats rows before the failure')
    assert (got['stats_bytes'][index + 1:] == 0).all(), name + ': a stats row after the failure is not 0'
    # the failing step itself, from the pose the healthy steps left
    level = track_ref.schedule(case['iterations'], 3)[index]
    P = healthy_c['before'][index]
    out = _step_call(cuda, dev, case, level, P)
    assert int(out['status'][0]) == code
    _same_bits(out['pose'], P, name + ': the failed step leaves its pose')
    s28, s27 = out['sums'][28], out['sums'][27]
    row = got['stats'][index]
    _same_bits(row[[0, 2, 3]], np.array([s28, 0.0, 0.0]), name + ': stats row of the failed step')
    if code == 3:
        assert np.isnan(s27) and np.isnan(row[1]) and s28 > 0
    else:
        _same_bits(row[1:2], np.array([s27 / s28 if s28 > 0 else 0.0]), name + ': mean squared residual of the failed step')
    got_code, reason = _check_against_restatement(out, case, level, P, name, nan_pixels=1 if code == 3 else 0)
    assert got_code == code
    if code == 3:  # the NaN changes no reason code: those of the healthy call's step
        healthy = _step_call(cuda, healthy_c['dev'], healthy_c['case'], level, P)
        _same_bits(out['reason'], healthy['reason'], name + ': reason codes with and without the NaN')


@pytest.mark.parametrize('name', sorted(track_cases.pyramid_inputs()))
def test_pyramid_on_inputs_the_stream_never_makes(cuda, name):
    depth, mask, delta = track_cases.pyramid_inputs()[name]
    h, w = depth.shape
    K = synthetic.intrinsics(h, w)
    E = synthetic.camera_pose(1.0)
    Ki = camera_arrays(level_intrinsics(K, 3), E)[0]
    md = torch.zeros((h >> 3, w >> 3), dtype=torch.float32, device=cuda)
    mn = torch.zeros((h >> 3, w >> 3, 3), dtype=torch.float32, device=cuda)
    out = _associate(cuda, depth, mask, 3, K, Ki, md, mn, E, E, delta=delta)
    want = track_ref.pyramid(depth, mask, 4, delta)
    assert want[3].shape == (8, w >> 3)
    for l in range(4):
        _same_bits(out['pyr'][l], want[l], '%s: pyramid level %d' % (name, l))
    assert int(out['status'][0]) != 0  # (no model: the solve's status is beside the point)


@pytest.mark.parametrize('level', (0, 2))
def test_association_with_other_thresholds_and_arbitrary_model_maps(cuda, level):
    case = track_cases.step_case('C')
    dev = _upload(cuda, case)
    for name, kw in track_cases.THRESHOLD_CASES.items():
        what = 'level %d, %s' % (level, name)
        out = _step_call(cuda, dev, case, level, case['E_init'], **kw)
        _, reason = _check_against_restatement(out, case, level, case['E_init'], what, **kw)
        c = np.bincount(reason.reshape(-1), minlength=8)
        print(what, c.tolist())
        if name == 'angle 180':
            assert c[7] == 0
    mask, fd, fn, pose = track_cases.fuzz_case(level)
    fuzz = track_cases.with_models(case, level, depth=fd, normals=fn, mask=mask)
    out = _step_call(cuda, _upload(cuda, fuzz), fuzz, level, pose)
    _, reason = _check_against_restatement(out, fuzz, level, pose, 'level %d, fuzz' % level)
    c = np.bincount(reason.reshape(-1), minlength=8)
    print('level %d, fuzz' % level, c.tolist())
    assert all(c[k] >= 10 for k in (0, 1, 2, 5, 6, 7)), c


@pytest.mark.parametrize('h,w', sorted(track_cases.CHUNK_CASES))
def test_solve_chunk_edges(cuda, h, w):
    """64, 65, 128 and 129 associate blocks: the solve adds their rows from LDS chunks of 64."""
    case = track_cases.chunk_case(h, w)
    dev = _upload(cuda, case)
    out = _step_call(cuda, dev, case, 0, case['E_init'])
    code, reason = _check_against_restatement(out, case, 0, case['E_init'], '%dx%d' % (h, w))
    assert code == 0 and (reason == 0).mean() >= 0.3
    # the whole call's one step is the same step
    got = _track(cuda, dev, case, (1,), 1)
    _same_bits(got['pose'], out['pose'], '%dx%d: pose of ojf_track' % (h, w))
    _same_bits(got['stats'][0, :2], np.array([out['sums'][28], out['sums'][27] / out['sums'][28]]), 'stats')


def test_track_frame_marshals_what_the_raw_call_takes(cuda):
    """track_frame at 4 levels equals, in pose, stats and status bits, a raw ojf_track call fed the maps track_frame
    renders: the Kinv rows, the two pointer arrays, the iteration list and the packed output buffer."""
    h, w, levels, its = 128, 176, 4, (2, 1, 2, 2)
    tsdf = torch.from_numpy(synthetic.gt_volumes(64)[0]).to(cuda)
    origin, res, _ = synthetic.grid_spec(64)
    st = synthetic.SyntheticStream(h, w, 64, 400)
    f0, f1 = st.frame(230), st.frame(231)
    E_ref = f0['extrinsics']
    kw = dict(origin=origin, resolution=res, depth=f1['tof_depth'], mask=f1['mask'], intrinsics=st.K, extrinsics=E_ref)
    a = track_frame(tsdf, None, levels=levels, iterations=its + (9,), **kw)  # (a count past `levels` is ignored)
    models = []
    for l in range(levels):
        Kl = level_intrinsics(st.K, l)
        r = render_views(tsdf, None, None, origin=origin, resolution=res, intrinsics=Kl, extrinsics=E_ref, shape=(h >> l, w >> l))
        models.append((r['depth'][0].contiguous(), r['normals'][0].contiguous(), camera_arrays(Kl, E_ref)[0]))
    case = dict(h=h, w=w, levels=levels, K=st.K, E_ref=E_ref, E_init=E_ref, dist=0.1, angle=20.0, delta=0.03, frac=0.05)
    dev = dict(depth=torch.from_numpy(f1['tof_depth']).to(cuda), mask=torch.from_numpy(f1['mask'].astype(np.uint8)).to(cuda),
               models=models)
    raw = _track(cuda, dev, case, its, 7)
    print('track_frame at 4 levels on the 64^3 room: status %d, inliers per step %s' % (a['status'], a['stats'][:, 0].tolist()))
    assert a['status'] == int(raw['status'][0]) and a['ok'] == (a['status'] == 0)
    assert a['stats'].shape == (7, 4) and a['extrinsics'].shape == (4, 4)
    _same_bits(a['extrinsics'][:3], raw['pose'], 'pose')
    _same_bits(a['stats'], raw['stats'], 'stats')
    assert a['extrinsics'][3].tolist() == [0.0, 0.0, 0.0, 1.0]
    assert (a['stats'][:, 0] > 0).all()  # every step ran
    # no iterations at all
    b = track_frame(tsdf, None, levels=3, iterations=(0, 0, 0), **kw)
    assert b['ok'] and b['status'] == 0 and b['stats'].shape == (0, 4)
    _same_bits(b['extrinsics'][:3], E_ref, 'pose of a call without iterations')
