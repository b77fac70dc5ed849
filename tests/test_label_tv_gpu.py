"""-m gpu: the multi-label TV solver (ojf_label_tv_setup / _solve / _write, label_tv.Solver, Database.regularize_labels,
FUSION_MODEL.label_tv in drivers.test_fusion) against its numpy restatement (label_tv_ref.py) bit for bit - u of every class,
ids, scores and the second record volume over the whole tensors, padding and unobserved voxels included."""
import numpy as np
import pytest
import torch

from online_joint_depthfusion_and_semantic_amd import _lib, label_tv, synthetic
from online_joint_depthfusion_and_semantic_amd.config import default_config, database_config
from online_joint_depthfusion_and_semantic_amd.database import Database
import label_ref
import label_tv_ref as ref

pytestmark = pytest.mark.gpu


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _bits(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize]) if a.dtype.kind == 'f' else a


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    n_bad = int((g != w).sum())
    assert n_bad == 0, '{}: {} of {} values differ'.format(what, n_bad, g.size)


def _field(solver):
    return torch.stack([solver.class_field(k) for k in range(solver.n_classes)])


def _outputs(shape, vol, C, cuda):
    ids, scores = ref.sentinels(shape)
    return _dev(ids, cuda), _dev(scores, cuda), _dev(ref.fresh_probs_out(vol, C), cuda)


def _check(solver, vol, got_vol, want, cuda, what):
    """The state and the three outputs of ``solver`` against ``want`` = (u, ids, scores, probs_out) of the restatement; the input
    volume is left as it was."""
    C, shape = solver.n_classes, solver.shape
    _same(_field(solver), want[0], what + ': u')
    ids, scores, probs_out = _outputs(shape, vol, C, cuda)
    solver.write(ids, scores, probs_out)
    _same(ids, want[1], what + ': ids')
    _same(scores, want[2], what + ': scores')
    _same(probs_out, want[3], what + ': probs_out')
    _same(got_vol, vol, what + ': the input volume')


# ---- 1. bit parity -------------------------------------------------------------------------------------------------------------
CASES = [  # every C on (5, 9, 33): two bricks per axis with a one-voxel remainder
    ((5, 9, 33), 2, 'all'), ((5, 9, 33), 7, 'other_bricks'), ((5, 9, 33), 8, 'faces'), ((5, 9, 33), 9, 'zero_sum'),
    ((5, 9, 33), 16, 'random'), ((5, 9, 33), 30, 'all'), ((5, 9, 33), 32, 'random'), ((5, 9, 33), 30, 'other_bricks'),
    ((5, 9, 33), 2, 'corner'), ((5, 9, 33), 16, 'none'),
    ((4, 8, 32), 7, 'all'), ((4, 8, 32), 32, 'all'), ((4, 8, 32), 16, 'corner'),  # one brick
    ((3, 5, 6), 9, 'all'), ((3, 5, 6), 30, 'random'), ((3, 5, 6), 8, 'none'),  # less than a brick, Z no multiple of 4
    ((9, 17, 70), 30, 'random'), ((9, 17, 70), 16, 'other_bricks'), ((9, 17, 70), 7, 'faces'), ((9, 17, 70), 32, 'zero_sum'),
]


@pytest.mark.parametrize('shape,C,pattern', CASES, ids=['{}x{}x{}-C{}-{}'.format(*s, C, p) for s, C, p in CASES])
def test_bit_parity_with_the_restatement(cuda, shape, C, pattern):
    """0, 1 and 7 iterations from a restart each, default options (lam 4, w_sat 4, tau = sigma = default_step)."""
    vol, want = ref.solved_case(shape, C, pattern)
    got_vol = _dev(vol, cuda)
    solver = label_tv.Solver(shape, C, cuda)
    observed = vol[..., C].astype(np.float32) > 0
    for n in (0, 1, 7):
        solver.solve(got_vol, iterations=n)
        assert int(solver.status.item()) == 0
        _check(solver, vol, got_vol, want[n], cuda, '{} C={} {} after {} iterations'.format(shape, C, pattern, n))
    x, y, z = np.nonzero(observed)
    bricks = len(set(zip(x // 4, y // 8, z // 32)))
    assert solver.count == bricks == solver.capacity  # (the state is sized by the listed bricks, not by the box)
    if pattern == 'none':
        assert solver.count == 0 and solver.workspace.numel() == solver.layout['u']


def test_other_options_than_the_defaults(cuda):
    shape, C = (5, 9, 33), 9
    vol = ref.case_volume(shape, C, 'random', seed=5)
    opts = dict(lam=1.5, w_sat=2.5, tau=0.2, sigma=0.4)
    s = ref.Solver(vol, C).iterate(4, **opts)
    ids, scores = ref.sentinels(shape)
    probs_out = ref.fresh_probs_out(vol, C)
    s.write(ids, scores, probs_out)
    got_vol = _dev(vol, cuda)
    solver = label_tv.Solver(shape, C, cuda)
    solver.solve(got_vol, iterations=4, **opts)
    _check(solver, vol, got_vol, (s.u, ids, scores, probs_out), cuda, 'lam 1.5, w_sat 2.5, tau 0.2, sigma 0.4')


def test_split_calls_restarts_and_continue_errors(cuda):
    """7 iterations in one call are 3 + 4 over two calls; a second restart gives the first one's bits (on a workspace that is
    already large enough, and after a solve on a volume with more bricks); restart=False needs a restart on the same object."""
    shape, C = (5, 9, 33), 16
    vol, want = ref.solved_case(shape, C, 'random')
    got_vol = _dev(vol, cuda)
    solver = label_tv.Solver(shape, C, cuda)
    with pytest.raises(ValueError, match='before any restart'):
        solver.solve(got_vol, iterations=1, restart=False)
    with pytest.raises(ValueError, match='nothing was solved'):
        solver.write(*_outputs(shape, vol, C, cuda)[:2])
    solver.solve(got_vol, iterations=3)
    solver.solve(got_vol, iterations=4, restart=False)
    _check(solver, vol, got_vol, want[7], cuda, '3 + 4 iterations')
    solver.solve(got_vol, iterations=0, restart=False)
    _same(_field(solver), want[7][0], 'a continue of 0 iterations')
    with pytest.raises(ValueError, match='another volume'):
        solver.solve(got_vol.clone(), iterations=1, restart=False)
    with pytest.raises(ValueError):
        solver.solve(_dev(ref.case_volume(shape, 7, 'all'), cuda), iterations=1)  # another class count
    with pytest.raises(ValueError):
        solver.class_field(C)
    solver.solve(got_vol, iterations=7)
    _check(solver, vol, got_vol, want[7], cuda, 'the second restart')
    few, few_want = ref.solved_case(shape, C, 'corner')
    few_vol = _dev(few, cuda)
    solver.solve(few_vol, iterations=7)  # (one listed brick in a workspace for eight)
    assert solver.count == 1 and solver.capacity == 8
    _check(solver, few, few_vol, few_want[7], cuda, 'a smaller list in the same workspace')
    solver.solve(got_vol, iterations=7)
    _check(solver, vol, got_vol, want[7], cuda, 'the third restart')


def test_capacity_one_brick_too_small(cuda):
    """ojf_label_tv_solve with capacity_bricks = count - 1: the status says so (1), the state is not touched, and the write
    that follows writes nothing."""
    shape, C = (5, 9, 33), 8
    vol, want = ref.solved_case(shape, C, 'all')
    got_vol = _dev(vol, cuda)
    solver = label_tv.Solver(shape, C, cuda)
    solver.solve(got_vol, iterations=7)
    assert solver.count == 8
    lib, L = _lib.load(), solver.layout
    state = solver.workspace[L['u']:].clone()
    status = torch.full((1,), -1, dtype=torch.int32, device=cuda)
    for mode in (_lib.LABEL_TV_RESTART, _lib.LABEL_TV_CONTINUE):
        rc = lib.ojf_label_tv_solve(_lib.ptr(got_vol), C, *shape, 4.0, 4.0, float(ref.STEP), float(ref.STEP), 3, mode, solver.count - 1,
                                    _lib.ptr(solver.workspace), solver.workspace.numel(), _lib.ptr(status), _lib.stream_ptr(cuda))
        _lib.check(rc, 'ojf_label_tv_solve')
        assert int(status.item()) == 1
        assert torch.equal(solver.workspace[L['u']:], state)
    ids, scores, probs_out = _outputs(shape, vol, C, cuda)
    solver.write(ids, scores, probs_out)
    sent_ids, sent_scores = ref.sentinels(shape)
    _same(ids, sent_ids, 'ids after a refused solve')
    _same(scores, sent_scores, 'scores after a refused solve')
    _same(probs_out, ref.fresh_probs_out(vol, C), 'probs_out after a refused solve')
    # a continue with the right capacity does not revive a state the header calls refused; a restart does
    rc = lib.ojf_label_tv_solve(_lib.ptr(got_vol), C, *shape, 4.0, 4.0, float(ref.STEP), float(ref.STEP), 3, _lib.LABEL_TV_CONTINUE, solver.count,
                                _lib.ptr(solver.workspace), solver.workspace.numel(), _lib.ptr(status), _lib.stream_ptr(cuda))
    _lib.check(rc, 'ojf_label_tv_solve')
    assert int(status.item()) != 0 and torch.equal(solver.workspace[L['u']:], state)
    solver.solve(got_vol, iterations=7)
    _check(solver, vol, got_vol, want[7], cuda, 'a restart after the refusals')


def test_write_in_place_into_the_solved_volume(cuda):
    """probs_out = the solved volume itself: the class channels take u, W and the padding stay."""
    shape, C = (5, 9, 33), 30
    vol, want = ref.solved_case(shape, C, 'other_bricks')
    got_vol = _dev(vol, cuda)
    solver = label_tv.Solver(shape, C, cuda)
    solver.solve(got_vol, iterations=7)
    ids, scores, _ = _outputs(shape, vol, C, cuda)
    solver.write(ids, scores, got_vol)
    expect = vol.copy()
    obs = vol[..., C].astype(np.float32) > 0
    expect[obs, :C] = want[7][3][obs, :C]
    _same(got_vol, expect, 'the volume after an in-place write')
    _same(ids, want[7][1], 'ids')


# ---- 2. Database and driver ----------------------------------------------------------------------------------------------------
H, W, GRID, FRAMES = 48, 64, 64, 6


def _room(cuda, **fm):
    cfg = default_config(H, W, semantics=True, model='tsdf')
    cfg.SETTINGS.device = str(cuda)
    cfg.FUSION_MODEL.update(fm)
    ds = synthetic.SyntheticDataset(H, W, GRID, FRAMES, scenes=['room_0'])
    return cfg, ds, [ds.streams['room_0'].frame(i) for i in range(FRAMES)]


def test_database_regularize_labels(cuda):
    cfg, ds, frames = _room(cuda)
    C = cfg.SEMANTIC_2D_MODEL.n_classes
    db = Database(ds, database_config(cfg))
    with pytest.raises(ValueError, match='class-distribution'):
        db.regularize_labels('room_0')
    for f in frames:
        db.integrate_label_probs('room_0', f['tof_depth'], f['intrinsics'], f['extrinsics'], mask=f['mask'], labels=f['semantic_gt'])
    vol = db.label_probs['room_0'].cpu().numpy().copy()
    assert int((vol[..., C].astype(np.float32) > 0).sum()) > 1000
    opts = dict(lam=2.0, w_sat=3.0)
    s = ref.Solver(vol, C).iterate(3, **opts)
    ids, scores = db.ids_est['room_0'].volume.cpu().numpy().copy(), db.scores['room_0'].volume.cpu().numpy().copy()
    probs_out = vol.copy()
    s.write(ids, scores, probs_out)
    db.regularize_labels(iterations=3, **opts)
    _same(db.ids_est['room_0'].volume, ids, 'Database.regularize_labels: ids')
    _same(db.scores['room_0'].volume, scores, 'Database.regularize_labels: scores')
    _same(db.label_probs['room_0'], vol, 'the distribution without keep_distribution')
    solver = db._label_tv_solvers['room_0']
    assert 0 < solver.count < solver.layout['n_bricks']  # the state covers the observed bricks only
    db.regularize_labels('room_0', iterations=3, keep_distribution=True, **opts)
    assert db._label_tv_solvers['room_0'] is solver
    _same(db.label_probs['room_0'], probs_out, 'the distribution with keep_distribution')
    _same(db.ids_est['room_0'].volume, ids, 'ids of the second call')
    db.to_numpy()
    assert db._label_tv_solvers == {}
    db.to_torch()
    db.regularize_labels('room_0', iterations=0)
    assert 'room_0' in db._label_tv_solvers
    db.reset('room_0')
    assert db._label_tv_solvers == {}
    db.regularize_labels('room_0', iterations=1)  # (an empty volume: nothing listed, nothing written)
    assert db._label_tv_solvers['room_0'].count == 0 and not db.ids_est['room_0'].volume.any()
    db.remove('room_0')
    assert db._label_tv_solvers == {}


def test_regularised_labels_beat_the_vote_on_noisy_labels(cuda):
    """The experiment of test_label_tv_host.py on the device: Database.integrate_label_probs of the clean and of the noisy
    label images, decide_labels on both, regularize_labels (lam 4, 30 iterations, w_sat 4) on the noisy one.  The same two
    conditions.  Measured on an MI355X: 16 089 observed voxels, vote 0.9218, regularised 0.9931; 8 890 with W >= 3: vote
    0.9874, regularised 0.9957 - the host figures."""
    st, frames = label_ref.noisy_frames(q=0.2, seed=7)
    C = label_ref.NOISE_CLASSES
    cfg = default_config(label_ref.NOISE_H, label_ref.NOISE_W, semantics=True, model='tsdf', n_classes=C)
    cfg.SETTINGS.device = str(cuda)
    out = {}
    for kind in ('labels_clean', 'labels_noisy'):
        db = Database(st, database_config(cfg))
        for f in frames:
            db.integrate_label_probs('room_0', f['depth_gt'], f['intrinsics'], f['extrinsics'], mask=f['mask'], labels=f[kind],
                                     band=label_ref.NOISE_BAND)
        db.decide_labels()
        vote = db.ids_est['room_0'].volume.cpu().numpy().copy()
        db.regularize_labels(**ref.NOISE_OPTIONS)
        out[kind] = (vote, db.ids_est['room_0'].volume.cpu().numpy(), db.label_probs['room_0'][..., C].float().cpu().numpy())
    figures = ref.noisy_figures(out['labels_clean'][0], out['labels_clean'][2], out['labels_noisy'][0], out['labels_noisy'][1])
    ref.assert_noisy_figures('on the device', figures)
    assert tuple(round(x, 4) for x in figures[2:]) == ref.NOISE_FIGURES, figures  # the figures of the host run


def test_driver_decides_as_before_without_label_tv(cuda, monkeypatch):
    """drivers.test_fusion with fuse_label_probs: without the key label_tv and with label_tv None it calls decide_labels, never
    regularize_labels, and leaves the same bits in every volume; with a dict it calls regularize_labels with those options,
    and only the labels change."""
    from online_joint_depthfusion_and_semantic_amd.drivers import test_fusion as run_test_fusion
    calls = []
    decide, regularize = Database.decide_labels, Database.regularize_labels
    monkeypatch.setattr(Database, 'decide_labels', lambda self, *a, **kw: (calls.append(('decide', kw)), decide(self, *a, **kw))[1])
    monkeypatch.setattr(Database, 'regularize_labels', lambda self, *a, **kw: (calls.append(('regularize', kw)), regularize(self, *a, **kw))[1])
    vols = {}
    for name in ('absent', 'none', 'dict'):
        cfg, ds, _ = _room(cuda, fuse_label_probs=True)
        assert cfg.FUSION_MODEL.label_tv is None
        if name == 'absent':
            del cfg.FUSION_MODEL['label_tv']
        elif name == 'dict':
            cfg.FUSION_MODEL.label_tv = dict(lam=2.0, iterations=5, w_sat=3.0)
        del calls[:]
        db = run_test_fusion(cfg, ds, cuda, log=lambda *a: None)[2]
        assert calls == ([('regularize', dict(lam=2.0, iterations=5, w_sat=3.0))] if name == 'dict' else [('decide', {})]), (name, calls)
        vols[name] = [v.clone() for v in (db.scenes_est['room_0'].volume, db.fusion_weights['room_0'], db.label_probs['room_0'],
                                          db.ids_est['room_0'].volume, db.scores['room_0'].volume)]
    for i, what in enumerate(('tsdf', 'weights', 'label volume', 'ids', 'scores')):
        _same(vols['none'][i], vols['absent'][i], what + ': label_tv None and absent')
        if i < 3:
            _same(vols['dict'][i], vols['absent'][i], what + ': label_tv given and absent')
    assert int((vols['absent'][2][..., 30] > 0).sum()) > 1000
    assert not torch.equal(vols['dict'][4].view(torch.int16), vols['absent'][4].view(torch.int16))  # the scores are u, not the mean
