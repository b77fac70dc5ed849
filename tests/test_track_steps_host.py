"""CPU: the conditions every case of test_track_steps_gpu.py relies on, shown on the numpy restatement (track_ref.py)
alone: the step cases are healthy and well conditioned and every step moves, the failure cases fail with the code and at
the iteration the GPU test names, the crafted pyramid inputs hold every kind of entry they are meant to hold, the
threshold and fuzz cases produce the reason codes they are for, the chunk-edge frames have the intended block counts, and
the restated loop is a pure function of its prefix."""
import numpy as np
import pytest

import track_cases
import track_ref

f32 = np.float32


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('name', sorted(track_cases.STEP_CASES))
def test_step_cases_are_healthy(name):
    case = track_cases.step_case(name)
    pose, status, stats, trace = track_cases.healthy_trace(name)
    steps = track_ref.schedule(case['iterations'], case['levels'])
    assert status == (0, -1) and len(trace) == len(steps) == stats.shape[0] <= 7
    assert [s['level'] for s in trace] == steps
    for k, s in enumerate(trace):
        assert s['code'] == 0, (name, k, s['code'])
        share = float((s['reason'] == 0).mean())
        cond = float(np.linalg.cond(track_ref.system(s['sums'])[0]))
        assert share >= 0.3 and cond <= 1e4, (name, k, share, cond)
        assert stats[k, 0] == (s['reason'] == 0).sum() and stats[k, 2] + stats[k, 3] > 1e-6, (name, k, stats[k])
    if name == 'A':  # all four levels take steps; level 3 is 16 x 22
        assert sorted(set(steps)) == [0, 1, 2, 3] and trace[0]['reason'].shape == (16, 22)
    if name == 'B':  # levels 0 and 1 (131x179, 65x89) lose a row and a column to the next level; level 1 takes no step
        assert all((case['h'] >> l) & 1 and (case['w'] >> l) & 1 for l in range(2)) and 1 not in steps
    if name == 'C':
        assert track_ref.pose_error(case['E_init'], case['E_ref'])[0] == pytest.approx(0.03)
    if name == 'D':
        assert case['mask'] is None and (case['depth'] > 0).all()


@pytest.mark.parametrize('name', sorted(track_cases.STEP_CASES))
def test_restated_loop_is_a_function_of_its_prefix(name):
    case = track_cases.step_case(name)
    pose, status, stats, trace = track_cases.healthy_trace(name)
    n = len(trace)
    for k in range(n + 1):
        its = track_ref.prefix_iterations(case['iterations'], case['levels'], k)
        assert sum(its) == k and track_ref.schedule(its, case['levels']) == [s['level'] for s in trace[:k]]
        P, st, rows = track_cases.run(case, iterations=its)
        assert st == (0, -1) and rows.shape == (k, 4)
        assert _same_bits(rows, stats[:k])
        assert _same_bits(P, trace[k]['pose'] if k < n else pose)
    assert _same_bits(track_cases.run(case, iterations=[0] * case['levels'])[0], case['E_init'][:3])


@pytest.mark.parametrize('name', sorted(track_cases.failure_cases()))
def test_failure_cases_fail_where_the_gpu_test_says(name):
    case, code, index = track_cases.failure_cases()[name]
    healthy = track_cases.healthy_trace('C')
    trace = []
    pose, status, stats = track_cases.run(case, trace=trace)
    assert status == (code, index) and index >= 2 and len(trace) == index + 1
    assert _same_bits(pose, case['E_init'][:3])
    assert not _same_bits(case['E_init'][:3], healthy[3][index]['pose'])  # the last good pose is another pose
    assert _same_bits(stats[:index], healthy[2][:index])
    assert not stats[index + 1:].any() and stats.shape == (6, 4)
    last = trace[-1]
    share = float((last['reason'] == 0).mean())
    if code == 1:
        assert share == 0 and not stats[index].any()
    if code == 2:  # one plane: plenty of inliers, a singular system
        assert 0.3 <= share <= 0.45 and stats[index, 0] >= case['frac'] * last['reason'].size
        assert stats[index, 1] > 0 and not stats[index, 2:].any()
    if code == 3:
        want = healthy[3][index]
        assert _same_bits(last['reason'], want['reason'])  # the NaN changes no reason code
        assert np.isnan(last['sums'][21:28]).all() and np.isfinite(last['sums'][:21]).all()
        assert last['sums'][28] == want['sums'][28] and stats[index, 0] == want['sums'][28]
        assert np.isnan(stats[index, 1]) and not stats[index, 2:].any()
        bad, target = track_cases._nan_pixel_case()
        md, mn, Ki, _ = bad['models'][1]
        assert int(np.isnan(md).sum()) == 1 and np.isnan(md.reshape(-1)[target])
        D1 = track_ref.pyramid(case['depth'], case['mask'], 2)[1]
        J, r, reason = track_ref.associate(D1, Ki, case['K'], 1, md, mn, case['E_ref'], last['pose'])
        assert int(np.isnan(r).sum()) == 1 and np.isfinite(J).all()


def test_pyramid_inputs_hold_what_they_are_for():
    inputs = track_cases.pyramid_inputs()
    assert len(inputs) == 2 * (1 + 2 * len(track_cases.PYRAMID_DELTAS) + 1)
    for name, (depth, mask, delta) in inputs.items():
        h, w = depth.shape
        assert (h, w) in track_cases.PYRAMID_SHAPES and depth.dtype == f32
        pyr = track_ref.pyramid(depth, mask, 4, delta)
        assert pyr[3].shape == (8, w >> 3) and all(np.isfinite(p).all() and (p >= 0).all() for p in pyr)
        if name.startswith('hostile'):
            counts = [np.isnan(depth).sum(), (depth == np.inf).sum(), (depth == -np.inf).sum(),
                      (np.isfinite(depth) & (depth < 0)).sum(), ((depth == 0) & np.signbit(depth)).sum(),
                      (depth == track_cases.SUBNORMAL).sum(), ((depth == 0) & ~np.signbit(depth)).sum()]
            assert min(counts) >= 0.03 * h * w, (name, counts)
            assert 0 < track_cases.SUBNORMAL < np.finfo(f32).tiny and (pyr[0] == track_cases.SUBNORMAL).any()
            if mask is None:
                assert 'no mask' in name
            else:
                assert mask.dtype == np.uint8 and sorted(np.unique(mask)) == [0, 1, 2, 255]
                assert min((mask == v).sum() for v in (0, 1, 2, 255)) >= 0.1 * h * w
                for v in (2, 255):  # a byte other than 1 lets a good depth through
                    assert ((mask == v) & (pyr[0] > 0)).sum() >= 0.03 * h * w
            assert (pyr[3] > 0).any()
        if name.startswith('blocks'):
            _, blocks = track_cases.block_frame(h, w, delta, 11 * h + w)
            kinds = {-1, 0, 1} - ({-1} if delta == 0 else set())
            seen = {(p, k) for p, k in blocks}
            assert seen == {(p, k) for p in range(16) for k in kinds}, (name, sorted(seen))
            # count the blocks by what the values in them really are: the occupancy and the largest spread
            D = depth[:h & ~1, :w & ~1].reshape(h >> 1, 2, w >> 1, 2).transpose(0, 2, 1, 3).reshape(-1, 4)
            got = {}
            for vals in D:
                occ = vals != 0
                pattern = int(sum(1 << k for k in range(4) if occ[k]))
                if occ.sum() >= 2:
                    key = (pattern, track_cases.spread(vals[occ].max(), vals[occ].min(), delta))
                    got[key] = got.get(key, 0) + 1
            pairs = [p for p in range(16) if bin(p).count('1') >= 2]
            assert set(got) == {(p, k) for p in pairs for k in kinds}, (name, sorted(got))
            assert min(got.values()) >= 3, (name, got)
            # the rule bites: at level 1 some blocks drop an entry and some keep all
            dropped = (pyr[1] != track_ref.pyramid(depth, mask, 2, 1e30)[1]).sum()
            assert (dropped > 0) == (delta < 1e30), (name, dropped)
    assert float(f32(0.1)) != 0.1  # rounded once to fp32 on the host


@pytest.mark.parametrize('level', (0, 2))
def test_threshold_and_fuzz_cases_produce_their_reasons(level):
    case = track_cases.step_case('C')
    md, mn, Ki, _ = case['models'][level]
    D = track_ref.pyramid(case['depth'], case['mask'], level + 1)[level]
    counts = {}
    for name, kw in track_cases.THRESHOLD_CASES.items():
        reason = track_ref.associate(D, Ki, case['K'], level, md, mn, case['E_ref'], case['E_init'],
                                     dist_thresh=kw.get('dist', 0.1), angle_thresh=kw.get('angle', 20.0))[2]
        counts[name] = np.bincount(reason.reshape(-1), minlength=8)
    n = D.size
    assert counts['angle 180'][7] == 0 and counts['angle 180'][0] > 0.3 * n
    assert counts['angle 0.5'][7] > 0.45 * n and counts['angle 0.5'][7] == counts['angle 0.5'].max()
    assert counts['dist 1e-3'][6] > 0.8 * n
    assert counts['dist 10'][6] == 0 and counts['dist 10'][0] > 0.5 * n
    mask, fd, fn, pose = track_cases.fuzz_case(level)
    Df = track_ref.pyramid(case['depth'], mask, level + 1)[level]
    reason = track_ref.associate(Df, Ki, case['K'], level, fd, fn, case['E_ref'], pose)[2]
    c = np.bincount(reason.reshape(-1), minlength=8)
    assert all(c[k] >= 10 for k in (0, 1, 2, 5, 6, 7)), c
    if level == 0:
        assert c[4] > 0, c
    lengths = np.linalg.norm(fn, axis=-1)
    assert lengths.min() < 0.5 and lengths.max() > 1.5 and (fn < 0).any() and (fn > 0).any()
    assert 0.05 < (fd == 0).mean() < 0.15


@pytest.mark.parametrize('h,w', sorted(track_cases.CHUNK_CASES))
def test_chunk_cases_have_the_intended_blocks(h, w):
    blocks = track_cases.CHUNK_CASES[(h, w)][0]
    assert -(-h * w // 1024) == blocks and blocks in (64, 65, 128, 129)
    if (h, w) == (256, 257):
        assert h * w - 1024 * (blocks - 1) == 256  # the last block is a quarter full: one wave of four
    trace = []
    pose, status, stats = track_cases.run(track_cases.chunk_case(h, w), trace=trace)
    assert status == (0, -1) and trace[0]['code'] == 0
    assert float((trace[0]['reason'] == 0).mean()) >= 0.3
    assert np.linalg.cond(track_ref.system(trace[0]['sums'])[0]) <= 1e4


def test_step_reports_its_moves_without_changing_its_result():
    sums = track_cases.healthy_trace('E')[3][0]['sums']
    P = track_cases.step_case('E')['E_init']
    code, Q = track_ref.step(sums, P, 10.0)
    code2, Q2, th, tau = track_ref.step(sums, P, 10.0, moves=True)
    assert code == code2 == 0 and _same_bits(Q, Q2) and th > 0 and tau > 0
    x = track_ref.cholesky_solve(*track_ref.system(sums))
    assert th == pytest.approx(np.linalg.norm(x[:3]), rel=1e-15) and tau == pytest.approx(np.linalg.norm(x[3:]), rel=1e-15)
    assert track_ref.step(sums, P, 1e9, moves=True)[2:] == (0.0, 0.0)
