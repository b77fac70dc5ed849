"""CPU: the multi-label TV solver's definition (label_tv_ref.py, the numpy restatement of csrc/ojf_label_tv.hip) - its simplex
projection against the float64 sort-based one, the energy it lowers, the GPU cases' coverage, the noisy-label experiment, and
the refusals of ojf_label_tv_* and of the Python layers without a device."""
import ctypes

import numpy as np
import pytest

from online_joint_depthfusion_and_semantic_amd import _lib, label_tv, tvl1
from online_joint_depthfusion_and_semantic_amd.config import default_config, database_config
import label_ref
import label_tv_ref as ref

F = np.float32


# ---- (a) the projection --------------------------------------------------------------------------------------------------------
def _projection_inputs(C):
    """4000 seeded rows: normal values at scales 0.01, 0.3, 1 and 3 (what the primal step hands the projection: a distribution
    plus a step of the order of tau · (6 + lam)), every third row rounded to quarters (ties, whole runs of equal values), 50
    rows of one repeated quarter and 50 distributions that are already on the simplex."""
    rng = np.random.default_rng([11, C])
    v = (rng.standard_normal((4000, C)) * rng.choice([0.01, 0.3, 1.0, 3.0], (4000, 1))).astype(F)
    v[::3] = np.round(v[::3] * 4) / 4
    v[1:200:4] = np.round(v[1:200:4, :1] * 4) / 4
    p = rng.random((50, C)) ** 4
    v[200:400:4] = (p / p.sum(axis=1, keepdims=True)).astype(F)
    return v


PROJECTION_ERROR = 4.768372e-07  # measured: the largest |Pi(v) - Pi_f64(v)| over the inputs above is 2.384e-7, 3.179e-7, 3.179e-7 and 4.768e-7 for C = 2, 7, 16, 32
PROJECTION_BOUND = 4 * PROJECTION_ERROR  # 1.907e-6 asserted


@pytest.mark.parametrize('C', [2, 7, 16, 32])
def test_projection_is_the_euclidean_projection_onto_the_simplex(C):
    """Pi of the definition (no sort: the largest of the C candidate thresholds) against the float64 sort-based projection
    (label_tv_ref.project_f64), which is the yardstick here - not the kernel.  Measured and asserted: see PROJECTION_ERROR."""
    v = _projection_inputs(C)
    got = ref.project(v)
    assert got.dtype == F
    want = ref.project_f64(v)
    assert np.abs(want.sum(axis=1) - 1).max() < 1e-12 and want.min() >= 0  # (the yardstick is a projection)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print('C = {}: largest |Pi - Pi_f64| = {:.3e}'.format(C, err))
    assert err <= PROJECTION_BOUND, err
    ties = v[1:200:4]
    assert (ties == ties[:, :1]).all() and np.abs(ref.project(ties) - F(1) / F(C)).max() <= PROJECTION_BOUND  # equal values: uniform
    one = np.zeros((1, C), F)
    assert (ref.project(one) == F(1) / F(C)).all()  # P = 0: theta = -1/C, the uniform start value


# ---- (b) the energy ------------------------------------------------------------------------------------------------------------
def test_iterations_lower_the_energy():
    """sum_k TV(u_k) - lam · sum omega <u, P> in float64 on a (9, 10, 11) box with 60 % observed voxels, C = 7: not higher
    after 30 iterations than at the start, with the simplex constraint kept to rounding."""
    vol = ref.case_volume((9, 10, 11), 7, 'random', seed=3)
    s = ref.Solver(vol, 7)
    e0 = s.energy()
    s.iterate(30)
    e1 = s.energy()
    print('energy: {:.4f} at the start, {:.4f} after 30 iterations'.format(e0, e1))
    assert e1 <= e0, (e0, e1)
    u = s.u[:, s.obs]
    assert np.abs(u.astype(np.float64).sum(axis=0) - 1).max() < 1e-5 and u.min() >= 0
    assert not s.u[:, ~s.obs].any() and not s.p[:, :, ~s.obs].any()  # unobserved voxels take no part


def test_split_calls_and_restarts_in_the_restatement():
    vol = ref.case_volume((5, 9, 33), 9, 'random')
    a, b = ref.Solver(vol, 9).iterate(7), ref.Solver(vol, 9).iterate(3).iterate(4)
    assert np.array_equal(a.u.view(np.uint32), b.u.view(np.uint32)) and np.array_equal(a.p.view(np.uint32), b.p.view(np.uint32))
    b.restart()
    b.iterate(7)
    assert np.array_equal(a.u.view(np.uint32), b.u.view(np.uint32))


# ---- the GPU cases are not vacuous -------------------------------------------------------------------------------------------
def test_gpu_cases_cover_what_they_claim():
    B = ref.BRICK
    for pattern, C in (('all', 30), ('other_bricks', 7), ('faces', 8), ('zero_sum', 9), ('corner', 2), ('none', 16)):
        shape = (5, 9, 33)
        vol = ref.case_volume(shape, C, pattern)
        assert vol.shape == shape + (ref.record_size(C),)
        assert (vol.view(np.uint16)[..., C + 1:] == ref.PAD_BITS).all()
        obs = vol[..., C].astype(F) > 0
        x, y, z = np.meshgrid(*[np.arange(n) for n in shape], indexing='ij')
        brick = (x // B[0] * 2 + y // B[1]) * 2 + z // B[2]
        listed = np.unique(brick[obs])
        if pattern == 'all':
            assert obs.all() and len(listed) == 8
        elif pattern == 'other_bricks':
            assert len(listed) == 4 and 0 < obs.sum() < obs.size
        elif pattern == 'faces':
            assert len(listed) == 8 and not obs[0, 0, 0] and obs[3, 0, 0] and obs[4, 0, 0] and obs[0, 0, 31] and obs[0, 0, 32]
        elif pattern == 'zero_sum':
            zero = ~vol[..., :C].any(axis=-1)
            assert obs.all() and 100 < zero.sum() < obs.sum()
        elif pattern == 'corner':
            assert obs.sum() == 1 and obs[-1, -1, -1] and len(listed) == 1
        else:
            assert not obs.any()
    vol, out = ref.solved_case((5, 9, 33), 7, 'other_bricks')
    u0, u1, u7 = (out[n][0] for n in (0, 1, 7))
    assert (u0 != u1).any() and (u1 != u7).any()  # the iterations move the field
    assert (out[0][1] != out[7][1]).any()  # ... and the decision
    obs = vol[..., 7].astype(F) > 0
    ids, scores, probs_out = out[7][1:]
    assert (ids[~obs] == 0xee).all() and (scores.view(np.uint16)[~obs] == 0x7e01).all() and (ids[obs] < 7).all()
    assert (probs_out.view(np.uint16)[~obs] == ref.PAD_BITS).all() and (probs_out.view(np.uint16)[..., 8:] == ref.PAD_BITS).all()
    assert np.array_equal(probs_out.view(np.uint16)[..., 7][obs], vol.view(np.uint16)[..., 7][obs])


# ---- (c) the noisy-label experiment ------------------------------------------------------------------------------------------
def test_regularised_labels_beat_the_vote_on_noisy_labels():
    """The experiment of test_label_probs_host.py (20 frames at 48 x 64 into 64^3, 16 classes, 20 % of the label pixels wrong,
    seed 7, band 0.1 m), fused by label_ref.fuse; the noisy volume decided by the per-voxel vote (label_ref.decide) and by the
    solver at lam = 4, iterations = 30, w_sat = 4; both against the per-voxel vote of the clean volume, on the clean volume's
    observed voxels and on those with W >= 3.
    Measured with this restatement: 16 089 observed voxels, vote 0.9218, regularised 0.9931; 8 890 with W >= 3: vote 0.9874,
    regularised 0.9957.  Asserted: regularised >= vote + 0.04 on the observed voxels, regularised >= vote on W >= 3."""
    vols = ref.noisy_volumes()
    C, G = label_ref.NOISE_CLASSES, (label_ref.NOISE_GRID,) * 3
    votes = {}
    for kind, vol in vols.items():
        ids, scores = np.zeros(G, np.uint8), np.zeros(G, np.float16)
        label_ref.decide(vol, C, ids, scores)
        votes[kind] = ids
    o = ref.NOISE_OPTIONS
    s = ref.Solver(vols['labels_noisy'], C).iterate(o['iterations'], lam=o['lam'], w_sat=o['w_sat'])
    reg, scores = votes['labels_noisy'].copy(), np.zeros(G, np.float16)
    s.write(reg, scores)
    figures = ref.noisy_figures(votes['labels_clean'], vols['labels_clean'][..., C].astype(F), votes['labels_noisy'], reg)
    ref.assert_noisy_figures('in the restatement', figures)
    assert tuple(round(x, 4) for x in figures[2:]) == ref.NOISE_FIGURES, figures  # (what the documents quote and the device run repeats)


# ---- (d) refusals --------------------------------------------------------------------------------------------------------------
class _Args:
    """A well-formed description of the three calls on host bytes nothing reads (every refusal comes before any HIP call)."""

    def __init__(self):
        self.buf = ctypes.create_string_buffer(1024)
        self.p = (ctypes.addressof(self.buf) + 255) & ~255
        self.good = dict(vol=self.p, C=16, X=8, Y=8, Z=8, lam=4.0, w_sat=4.0, tau=float(ref.STEP), sigma=float(ref.STEP), iterations=3,
                         mode=_lib.LABEL_TV_RESTART, capacity=1, ws=self.p + 256, ws_bytes=None, count=self.p + 16, status=self.p + 32,
                         ids=self.p + 48, scores=self.p + 64, out=None)

    def _d(self, kw):
        d = dict(self.good, **kw)
        if d['ws_bytes'] is None:
            d['ws_bytes'] = _lib.load().ojf_label_tv_workspace_bytes(8, 8, 8, 16, d['capacity'])
        return d

    def setup(self, **kw):
        d = self._d(dict(kw, capacity=0))
        return _lib.load().ojf_label_tv_setup(d['vol'], d['C'], d['X'], d['Y'], d['Z'], d['ws'], d['ws_bytes'], d['count'], None)

    def solve(self, **kw):
        d = self._d(kw)
        return _lib.load().ojf_label_tv_solve(d['vol'], d['C'], d['X'], d['Y'], d['Z'], d['lam'], d['w_sat'], d['tau'], d['sigma'],
                                              d['iterations'], d['mode'], d['capacity'], d['ws'], d['ws_bytes'], d['status'], None)

    def write(self, **kw):
        d = self._d(dict(kw, capacity=0))
        return _lib.load().ojf_label_tv_write(d['vol'], d['C'], d['X'], d['Y'], d['Z'], d['ws'], d['ws_bytes'], d['ids'], d['scores'],
                                              d['out'], None)


def _refused(rc, who, word):
    msg = _lib.load().ojf_last_error().decode()
    assert rc != 0 and msg.startswith(who + ':') and word in msg, (rc, msg)


def test_entry_points_refuse_bad_arguments_without_a_device():
    a, lib = _Args(), _lib.load()
    assert _lib.LABEL_TV_MAX_CLASSES == ref.MAX_CLASSES == 32 and (_lib.LABEL_TV_CONTINUE, _lib.LABEL_TV_RESTART) == (0, 1)
    wb = lib.ojf_label_tv_workspace_bytes
    assert wb(0, 8, 8, 16, 0) == 0 and wb(2048, 2048, 2048, 16, 0) == 0 and wb(8, 8, 8, 1, 0) == 0 and wb(8, 8, 8, 33, 0) == 0
    # two bricks: header, three tables of two words, 2 x 1024 flag bytes; then 5 · C · 1024 floats per slot
    assert wb(8, 8, 8, 16, 0) == 256 + 3 * 256 + 2 * 1024 and wb(8, 8, 8, 16, 3) == wb(8, 8, 8, 16, 0) + 3 * 20 * 16 * 1024
    assert wb(5, 9, 33, 30, 8) == label_tv.workspace_layout((5, 9, 33), 30, 8)['bytes'] == 256 + 3 * 256 + 8 * 1024 + 8 * 20 * 30 * 1024
    for call, who, keys in ((a.setup, 'ojf_label_tv_setup', ('vol', 'ws', 'count')), (a.solve, 'ojf_label_tv_solve', ('vol', 'ws', 'status')),
                            (a.write, 'ojf_label_tv_write', ('vol', 'ws', 'ids', 'scores'))):
        for key in keys:
            _refused(call(**{key: None}), who, 'null')
        for C in (1, 33, 256):
            _refused(call(C=C), who, 'n_classes')
        _refused(call(vol=a.p + 8), who, '16-byte')
        for key in ('X', 'Y', 'Z'):
            _refused(call(**{key: 0}), who, 'volume size')
        _refused(call(X=2048, Y=2048, Z=2048), who, 'too large')
        _refused(call(ws=a.p + 16), who, 'aligned')
        _refused(call(ws_bytes=lib.ojf_label_tv_workspace_bytes(8, 8, 8, 16, 0) - 1), who, 'workspace too small')
    who = 'ojf_label_tv_solve'
    _refused(a.solve(ws_bytes=lib.ojf_label_tv_workspace_bytes(8, 8, 8, 16, 1) - 1), who, 'workspace too small')
    for v in (0.0, -1.0, float('nan'), float('inf')):
        _refused(a.solve(lam=v), who, 'lambda')
        _refused(a.solve(w_sat=v), who, 'w_sat')
    for key in ('tau', 'sigma'):
        for v in (0.0, -0.1, float('nan'), float('inf')):
            _refused(a.solve(**{key: v}), who, 'tau and sigma')
    _refused(a.solve(tau=0.3, sigma=0.3), who, '1/12')
    _refused(a.solve(tau=float(np.nextafter(ref.STEP, F(1))), sigma=float(ref.STEP)), who, '1/12')
    _refused(a.solve(iterations=-1), who, 'iterations')
    for v in (-1, 2, 3):
        _refused(a.solve(mode=v), who, 'mode')
    _refused(a.solve(status=a.p + 33), who, 'misaligned')
    _refused(a.setup(count=a.p + 18), 'ojf_label_tv_setup', 'misaligned')
    _refused(a.write(scores=a.p + 65), 'ojf_label_tv_write', 'misaligned')
    _refused(a.write(out=a.p + 8), 'ojf_label_tv_write', 'misaligned')
    assert float(ref.STEP) == tvl1.default_step()


def test_python_layer_refuses_bad_arguments_without_a_device():
    for bad in (dict(shape=(4, 4, 4), n_classes=16, device='cpu'), dict(shape=(4, 4), n_classes=16, device='cuda'),
                dict(shape=(4, 0, 4), n_classes=16, device='cuda'), dict(shape=(4, 4, 4), n_classes=1, device='cuda'),
                dict(shape=(4, 4, 4), n_classes=33, device='cuda')):
        with pytest.raises(ValueError):
            label_tv.Solver(**bad)
    good = dict(lam=4.0, iterations=30, w_sat=4.0, tau=None, sigma=None)
    assert label_tv.solver_options('t', **good) == (4.0, 30, 4.0, tvl1.default_step(), tvl1.default_step())
    for bad in (dict(lam=0.0), dict(lam=float('nan')), dict(w_sat=0.0), dict(w_sat=float('inf')), dict(iterations=-1),
                dict(tau=0.3, sigma=0.3), dict(tau=-1.0)):
        with pytest.raises(ValueError):
            label_tv.solver_options('t', **dict(good, **bad))
    L = label_tv.workspace_layout((9, 17, 70), 30, 5)
    assert L['bricks'] == (3, 3, 3) and L['n_bricks'] == 27 and L['plane'] == 5 * 30 * 1024 and L['u'] % 256 == 0


def test_database_and_config_without_a_device():
    """regularize_labels on a scene without a class-distribution volume is a ValueError (raised in front of any device work);
    FUSION_MODEL.label_tv is None - off - by default."""
    from online_joint_depthfusion_and_semantic_amd import synthetic
    from online_joint_depthfusion_and_semantic_amd.database import Database
    cfg = default_config(48, 64, semantics=True, model='tsdf')
    assert 'label_tv' in cfg.FUSION_MODEL and cfg.FUSION_MODEL.label_tv is None
    cfg.SETTINGS.device = 'cpu'
    ds = synthetic.SyntheticDataset(48, 64, 16, 2, scenes=['room_0'])
    db = Database(ds, database_config(cfg))
    with pytest.raises(ValueError, match='class-distribution'):
        db.regularize_labels('room_0')
    db.regularize_labels()  # (no scene has a volume: nothing to do)
    db.label_probs['room_0'] = np.zeros((16, 16, 16, 32), np.float16)  # host state
    with pytest.raises(ValueError, match='resident'):
        db.regularize_labels('room_0')
    assert db._label_tv_solvers == {}
