"""CPU: the label volume's definition (label_ref.py, the numpy restatement of csrc/ojf_labels.hip) - the coverage of the GPU
parity cases, views per call, the decision's rules, the refusals of ojf_fuse_label_probs / ojf_label_decide / ojf_seg_softmax
and of the Python wrappers without a device, and the quality of the per-voxel vote against the one-slot rule on noisy labels."""
import numpy as np
import pytest
import torch

from online_joint_depthfusion_and_semantic_amd import _lib, label_probs, synthetic
import label_ref as ref
import projective_ref as pref


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


# ---- the GPU parity cases are not vacuous ------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', ref.SHAPES)
@pytest.mark.parametrize('pose', ref.POSES)
def test_gpu_cases_update_voxels_and_skip_what_they_claim(shape, pose):
    c = ref.tiny_label_case(shape, pose)
    C = c['n_classes']
    assert (c['labels'] >= C).sum() >= 5 and (c['labels'] < C).sum() >= 100
    bad = ~((c['probs'][..., :C] >= 0) & (c['probs'][..., :C] <= 1))
    assert np.isnan(c['probs'][..., :C]).sum() >= 20 and (c['probs'][..., :C] < 0).sum() >= 20 and (c['probs'][..., :C] > 1).sum() >= 20
    assert bad.any(axis=-1).mean() > 0.5
    for form in ('labels', 'probs'):
        for masked in (False, True):
            vol = c['volume'].copy()
            n = ref.fuse(vol, C, c['origin'], c['res'], c['depth'], c['K'], c['E'], c['mask'] if masked else None,
                         band=c['band'], max_weight=c['label_max_weight'], **{form: c[form]})[0]
            changed = int((_bits(vol) != _bits(c['volume'])).any(axis=-1).sum())
            assert (_bits(vol)[..., C + 1:] == ref.PAD_BITS).all()  # the padding is never written
            if pose == 'looking_away':
                assert n['updates'] == 0 and changed == 0
                continue
            assert n['updates'] >= 20 and 0 < changed <= n['updates'], (n, changed)
            if form == 'labels':
                assert n['label_skips'] >= 1, n  # a label >= C inside the band leaves its voxel alone
            else:
                assert n['bad_probs'] >= 20, n  # NaN / negative / > 1 entries reach voxels and count as 0
            assert not np.isnan(vol[..., :C + 1].astype(np.float32)).any()


@pytest.mark.parametrize('C', [2, 7, 8, 256])
def test_record_sizes_and_edge_class_counts(C):
    """C = 7: W is the last element of the only chunk; 8: the first of a second chunk, then 7 padding elements; 256: S = 264."""
    assert ref.record_size(C) == label_probs.record_size(C) == {2: 8, 7: 8, 8: 16, 256: 264}[C]
    for stride in (C, C + 3):
        c = ref.tiny_label_case((5, 7, 19), 'oblique', C=C, prob_stride=stride)
        assert c['probs'].shape[-1] == stride and c['volume'].shape[-1] == ref.record_size(C)
        for form in ('labels', 'probs'):
            vol = c['volume'].copy()
            n = ref.fuse(vol, C, c['origin'], c['res'], c['depth'], c['K'], c['E'], band=c['band'],
                         max_weight=c['label_max_weight'], **{form: c[form]})[0]
            assert n['updates'] >= 20
            assert (_bits(vol)[..., C + 1:] == ref.PAD_BITS).all()


def test_views_in_one_call_are_calls_of_one_view():
    cases = [ref.tiny_label_case((16, 16, 16), p) for p in ref.POSES]
    C = cases[0]['n_classes']
    o, res = cases[0]['origin'], cases[0]['res']
    for form in ('labels', 'probs'):
        a, b = cases[0]['volume'].copy(), cases[0]['volume'].copy()
        ref.fuse(a, C, o, res, np.stack([c['depth'] for c in cases]), cases[0]['K'], np.stack([c['E'] for c in cases]),
                 band=ref.BAND, max_weight=ref.MAX_WEIGHT, **{form: np.stack([c[form] for c in cases])})
        for c in cases:
            ref.fuse(b, C, o, res, c['depth'], c['K'], c['E'], band=ref.BAND, max_weight=ref.MAX_WEIGHT, **{form: c[form]})
        assert np.array_equal(_bits(a), _bits(b))
        assert a[..., C].max() == ref.MAX_WEIGHT  # the weight saturates, the means still move


def test_one_hot_votes_keep_a_distribution():
    """From an empty volume, one-hot votes keep every record a distribution: the class means sum to 1 within the fp16
    rounding of C values, and W counts the votes."""
    cases = [ref.tiny_label_case((16, 16, 16), p) for p in ref.POSES[:4]]
    C = cases[0]['n_classes']
    vol = np.zeros((16, 16, 16, ref.record_size(C)), np.float16)
    for c in cases:
        ref.fuse(vol, C, c['origin'], c['res'], c['depth'], c['K'], c['E'], labels=c['labels'], band=ref.BAND)
    seen = vol[..., C] > 0
    assert seen.sum() > 100 and vol[..., C].max() >= 2
    total = vol[..., :C].astype(np.float64).sum(axis=-1)
    assert np.abs(total[seen] - 1.0).max() <= C * 2.0 ** -11 and not vol[~seen].any()


# ---- the decision ----------------------------------------------------------------------------------------------------------
def test_decide_rules():
    C = 5
    S = ref.record_size(C)
    vol = np.zeros((2, 2, 2, S), np.float16)
    r = vol.reshape(8, S)
    r[0, :C + 1] = (0.5, 0.5, 0, 0, 0, 3)          # two classes tie: the lower index
    r[1, :C + 1] = (0.2, 0.2, 0.2, 0.2, 0.2, 1)    # all equal: class 0
    r[2, :C + 1] = (0.6, 0.1, 0.1, 0.1, 0.1, 2)    # class 0 wins
    r[3, :C + 1] = (0.1, 0.1, 0.1, 0.1, 0.6, 2)    # the last class wins
    for i, wv in ((4, 0.0), (5, -0.0), (6, -1.0), (7, np.nan)):
        r[i, :C + 1] = (0, 0.9, 0, 0, 0.1, wv)
    ids = np.full((2, 2, 2), 77, np.uint8)
    scores = np.full((2, 2, 2), 0.25, np.float16)
    assert ref.decide(vol, C, ids, scores) == 4
    assert ids.reshape(8).tolist() == [0, 0, 0, 4, 77, 77, 77, 77]
    assert scores.reshape(8).tolist() == [0.5, np.float16(0.2), np.float16(0.6), np.float16(0.6), 0.25, 0.25, 0.25, 0.25]
    r[4, C] = np.float16(2.0 ** -24)  # the smallest positive weight decides
    assert ref.decide(vol, C, ids, scores) == 5 and ids.reshape(8)[4] == 1


def test_softmax_restatement_matches_torch():
    rng = np.random.default_rng(3)
    l = rng.normal(0.0, 3.0, (500, 19)).astype(np.float32)
    l[7, 3] = np.nan
    l[8, 0] = np.inf
    l[9, :] = -np.inf
    l[10, 5] = -np.inf
    got, bad = ref.softmax(l)
    want = torch.softmax(torch.from_numpy(l).double(), dim=1).numpy()
    assert bad.tolist() == [i in (7, 8, 9) for i in range(500)]
    assert np.isnan(got[bad]).all() and np.isnan(want[bad]).all()
    assert np.abs(got[~bad] - want[~bad]).max() <= 1e-6 and got[10, 5] == 0


# ---- the entry points refuse bad arguments before any HIP call ---------------------------------------------------------
K0 = np.array([[4.0, 0.0, 2.0], [0.0, 4.0, 2.0], [0.0, 0.0, 1.0]])
E0 = np.eye(4)[:3]


class _Args:
    """Complete, valid argument lists with fake (never dereferenced) device pointers; keyword overrides replace entries."""

    def __init__(self):
        self.origin = np.zeros(3)
        self.K = np.ascontiguousarray(np.stack([K0.reshape(9)] * 2))
        self.E = np.ascontiguousarray(np.stack([E0.reshape(12)] * 2))
        self.p = 0x1000

    def _call(self, name, a, kw):
        a.update(kw)
        lib = _lib.load()
        rc = getattr(lib, name)(*list(a.values()), None)
        return rc, lib.ojf_last_error().decode()

    def fuse(self, **kw):
        a = dict(vol=self.p, C=30, X=8, Y=8, Z=8, origin=self.origin.ctypes.data, res=0.1, n=2, K=self.K.ctypes.data,
                 E=self.E.ctypes.data, depth=self.p, mask=None, probs=None, prob_stride=0, labels=self.p, h=4, w=4, band=0.1,
                 max_weight=64.0, near=0.0)
        return self._call('ojf_fuse_label_probs', a, kw)

    def decide(self, **kw):
        a = dict(vol=self.p, C=30, X=8, Y=8, Z=8, ids=self.p, scores=self.p)
        return self._call('ojf_label_decide', a, kw)


def _refused(result, prefix, word):
    rc, msg = result
    assert rc != 0 and msg.startswith(prefix + ':') and word in msg, (rc, msg)


def test_fuse_label_probs_refuses_bad_arguments_without_a_device():
    a = _Args()
    who = 'ojf_fuse_label_probs'
    assert _lib.LABEL_MAX_VIEWS == 32
    for key in ('vol', 'origin', 'K', 'E', 'depth'):
        _refused(a.fuse(**{key: None}), who, 'null')
    _refused(a.fuse(labels=None), who, 'exactly one')                              # neither form
    _refused(a.fuse(probs=a.p, prob_stride=30), who, 'exactly one')                # both
    _refused(a.fuse(labels=None, probs=a.p, prob_stride=29), who, 'prob_stride')   # rows shorter than the classes
    _refused(a.fuse(labels=None, probs=a.p + 2, prob_stride=30), who, 'aligned')
    for off in (2, 8):
        _refused(a.fuse(vol=a.p + off), who, '16-byte')
    for C in (-1, 0, 1, 257):
        _refused(a.fuse(C=C), who, 'n_classes')
    _refused(a.fuse(n=0), who, 'views')
    _refused(a.fuse(n=_lib.LABEL_MAX_VIEWS + 1), who, 'views')
    for key in ('X', 'Y', 'Z'):
        _refused(a.fuse(**{key: 0}), who, 'volume size')
    _refused(a.fuse(X=2048, Y=2048, Z=2048), who, 'too large')
    _refused(a.fuse(h=0), who, 'image size')
    _refused(a.fuse(w=-3), who, 'image size')
    for v in (0.0, -0.1, float('inf'), float('nan')):
        _refused(a.fuse(band=v), who, 'band')
    for v in (0.0, 0.5, 4096.0, float('nan')):
        _refused(a.fuse(max_weight=v), who, 'max_weight')
    for v in (-0.01, float('nan'), float('inf')):
        _refused(a.fuse(near=v), who, 'near')
    for idx, v in ((1, 0.1), (3, 1e-3), (6, 1.0), (7, -2.0), (8, 2.0)):
        bad = _Args()
        bad.K[1, idx] = v  # (the second view's matrix: every view is checked)
        _refused(bad.fuse(), who, 'pinhole')
    for name, idx in (('K', 4), ('E', 7), ('origin', 2)):
        for v in (float('nan'), float('inf')):
            bad = _Args()
            getattr(bad, name).reshape(-1)[idx] = v
            _refused(bad.fuse(), who, 'non-finite')
    _refused(a.fuse(res=float('nan')), who, 'non-finite')
    _refused(a.fuse(res=0.0), who, 'resolution')


def test_label_decide_and_softmax_refuse_bad_arguments_without_a_device():
    a = _Args()
    who = 'ojf_label_decide'
    for key in ('vol', 'ids', 'scores'):
        _refused(a.decide(**{key: None}), who, 'null')
    for C in (1, 257):
        _refused(a.decide(C=C), who, 'n_classes')
    _refused(a.decide(vol=a.p + 8), who, '16-byte')
    for key in ('X', 'Y', 'Z'):
        _refused(a.decide(**{key: 0}), who, 'volume size')
    _refused(a.decide(X=2048, Y=2048, Z=2048), who, 'too large')
    _refused(a.decide(scores=a.p + 1), who, 'aligned')
    lib = _lib.load()
    good = dict(logits=a.p, stride=32, C=30, npix=10, probs=a.p, out_stride=32)
    for fault in (dict(logits=None), dict(probs=None), dict(C=0), dict(C=257), dict(npix=0), dict(stride=29), dict(out_stride=29),
                  dict(probs=a.p + 2)):
        assert lib.ojf_seg_softmax(*list(dict(good, **fault).values()), None) != 0, fault
        assert lib.ojf_last_error().decode().startswith('ojf_seg_softmax:')


def test_python_wrappers_refuse_bad_arguments_without_a_device():
    """What the wrappers can refuse on a machine without a GPU: the class count and a volume that is not a device tensor of
    the record's shape - ValueError, in front of the device check (the rest of their checks run in the GPU tests)."""
    for C in (1, 257, 0):
        with pytest.raises(ValueError):
            label_probs.new_volume((4, 4, 4), C, 'cpu')
    vol = label_probs.new_volume((4, 4, 4), 30, 'cpu')
    assert vol.shape == (4, 4, 4, 32) and vol.dtype == torch.float16 and not vol.any()
    kw = dict(origin=np.zeros(3), resolution=0.1, depth=torch.ones(4, 4), intrinsics=K0, extrinsics=E0, labels=torch.zeros(4, 4, dtype=torch.uint8),
              band=0.1)
    with pytest.raises(ValueError):
        label_probs.integrate_label_probs(vol, 30, **kw)  # a host tensor
    with pytest.raises(ValueError):
        label_probs.integrate_label_probs(vol, 1, **kw)
    with pytest.raises(ValueError):
        label_probs.decide_labels(vol, 30, torch.zeros(4, 4, 4, dtype=torch.uint8), torch.zeros(4, 4, 4, dtype=torch.float16))
    with pytest.raises(ValueError):
        label_probs.decide_labels(vol.numpy(), 30, None, None)


def test_pipeline_and_database_refuse_label_fusion_without_classes():
    from online_joint_depthfusion_and_semantic_amd.config import default_config
    from online_joint_depthfusion_and_semantic_amd.pipeline import Pipeline
    cfg = default_config(48, 64, semantics=True, model='tsdf')
    assert cfg.FUSION_MODEL.fuse_label_probs is False and cfg.FUSION_MODEL.label_band == cfg.DATA.init_value
    assert Pipeline(cfg)._label_options() is None
    cfg.FUSION_MODEL.fuse_label_probs = True
    assert Pipeline(cfg)._label_options() == dict(band=cfg.DATA.init_value)
    del cfg.FUSION_MODEL['fuse_label_probs'], cfg.FUSION_MODEL['label_band']  # (configs written before the option: read with .get)
    assert Pipeline(cfg)._label_options() is None
    bare = default_config(48, 64, semantics=False, model='tsdf')
    bare.FUSION_MODEL.fuse_label_probs = True
    with pytest.raises(ValueError):
        Pipeline(bare)._label_options()


# ---- quality of the definition: noisy labels on the synthetic room -----------------------------------------------------
def test_vote_beats_the_one_slot_rule_on_noisy_labels():
    """20 frames of synthetic.SyntheticStream(48, 64, 64, 20, n_classes=16) - depth_gt, mask, poses - whose label pixels are
    replaced with probability q = 0.2 (seed 7) by a uniform class of 1..15 while keeping the frame's semantic_scores (a wrong
    pixel is as confident as a right one), fused with a band of 0.1 m by the one-slot rule (projective_ref.fuse: the highest
    score owns the voxel) and by the per-voxel vote (label_ref.fuse + decide).  Each rule's labels are compared with the labels
    the same rule fuses from the clean label images, over the 16 089 voxels the frames observe.
    Measured with this reference: one-slot 0.8177, vote 0.9218; over the 8 890 voxels with W >= 3: one-slot 0.8197, vote
    0.9874.  (q = 0.35: 0.676 / 0.846; q = 0.5: 0.535 / 0.747.)  The assertions are conditions set at about half the gap: the
    vote is at least 0.05 ahead over the observed voxels, and at least 0.95 right where a voxel was seen three times."""
    st, frames = ref.noisy_frames(q=0.2, seed=7)
    origin, res, _ = synthetic.grid_spec(ref.NOISE_GRID)
    C, G = ref.NOISE_CLASSES, (ref.NOISE_GRID,) * 3
    out = {}
    for kind in ('labels_clean', 'labels_noisy'):
        tsdf, wgt = np.full(G, 0.1, np.float16), np.zeros(G, np.float16)
        ids, scores = np.zeros(G, np.uint8), np.zeros(G, np.float16)
        vol = np.zeros(G + (ref.record_size(C),), np.float16)
        for f in frames:
            pref.fuse(tsdf, wgt, origin, res, f['depth_gt'], f['intrinsics'], f['extrinsics'], f['mask'], ids, scores, f[kind],
                      f['label_scores'], trunc=ref.NOISE_BAND)
            ref.fuse(vol, C, origin, res, f['depth_gt'], f['intrinsics'], f['extrinsics'], f['mask'], labels=f[kind], band=ref.NOISE_BAND)
        vote_ids, vote_scores = np.zeros(G, np.uint8), np.zeros(G, np.float16)
        ref.decide(vol, C, vote_ids, vote_scores)
        out[kind] = (ids, vote_ids, vol[..., C].astype(np.float32))
    observed, thrice = out['labels_clean'][2] > 0, out['labels_clean'][2] >= 3
    slot = ref.agreement(out['labels_noisy'][0], out['labels_clean'][0], observed)
    vote = ref.agreement(out['labels_noisy'][1], out['labels_clean'][1], observed)
    slot3 = ref.agreement(out['labels_noisy'][0], out['labels_clean'][0], thrice)
    vote3 = ref.agreement(out['labels_noisy'][1], out['labels_clean'][1], thrice)
    print('noisy labels q=0.2: {} observed, one-slot {:.4f}, vote {:.4f}; {} with W >= 3: one-slot {:.4f}, vote {:.4f}'.format(
        int(observed.sum()), slot, vote, int(thrice.sum()), slot3, vote3))
    assert observed.sum() > 15000 and thrice.sum() > 8000
    assert vote >= slot + 0.05, (vote, slot)
    assert vote3 >= 0.95, vote3
