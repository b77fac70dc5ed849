"""-m gpu: the label volume (ojf_fuse_label_probs / ojf_label_decide / ojf_seg_softmax, label_probs.py, segconv.softmax,
SegEngine.predict_probs, Database.integrate_label_probs / decide_labels / save, Pipeline with FUSION_MODEL.fuse_label_probs)
against its numpy restatement (label_ref.py) bit for bit over the whole tensors, padding included, and the public layers
against direct calls."""
import os

import numpy as np
import pytest
import torch

from online_joint_depthfusion_and_semantic_amd import _lib, segconv, synthetic
from online_joint_depthfusion_and_semantic_amd.label_probs import integrate_label_probs, decide_labels, new_volume, record_size
from online_joint_depthfusion_and_semantic_amd.config import default_config, database_config
from online_joint_depthfusion_and_semantic_amd.database import Database
from online_joint_depthfusion_and_semantic_amd.pipeline import Pipeline
import label_ref as ref
import stream_ops_cases as cases
from stream_ops_cases import Guarded, Rows

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


def _fuse_case(vol, c, cuda, form, mask=None, obs=None, depth=None, E=None):
    obs = c[form] if obs is None else obs
    integrate_label_probs(vol, c['n_classes'], origin=c['origin'], resolution=c['res'], depth=_dev(c['depth'] if depth is None else depth, cuda),
                          intrinsics=c['K'], extrinsics=c['E'] if E is None else E, mask=_dev(mask, cuda), band=c['band'],
                          max_weight=c['label_max_weight'], **{form: _dev(obs, cuda)})


def _ref_case(vol, c, form, mask=None):
    return ref.fuse(vol, c['n_classes'], c['origin'], c['res'], c['depth'], c['K'], c['E'], mask, band=c['band'],
                    max_weight=c['label_max_weight'], **{form: c[form]})


# ---- 1. bit parity of integrate_label_probs ----------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', ref.SHAPES)  # (5,7,19): 665 voxels, no multiple of 64
@pytest.mark.parametrize('pose', ref.POSES)
def test_bit_parity_on_tiny_volumes(cuda, shape, pose):
    """C = 30 (S = 32: three whole chunks, six classes and W in the last one), both observation forms, with and without mask."""
    c = ref.tiny_label_case(shape, pose)
    for form in ('labels', 'probs'):
        for masked in (False, True):
            mask = c['mask'] if masked else None
            want = c['volume'].copy()
            n = _ref_case(want, c, form, mask)
            got = _dev(c['volume'], cuda)
            _fuse_case(got, c, cuda, form, mask)
            _same(got, want, '{} {} {} mask={} ({})'.format(shape, pose, form, masked, n))


@pytest.mark.parametrize('shape', [(5, 7, 19), (16, 16, 16)])
@pytest.mark.parametrize('C', [2, 7, 8, 256])
def test_bit_parity_at_the_edges_of_the_record(cuda, shape, C):
    """C = 2; 7 (W is the last element of the only chunk); 8 (W is the first element of a second chunk, seven padding elements
    behind it); 256 (S = 264, the limit) - with probability rows of C and of C + 3 floats (NaN behind the classes).  The
    padding holds 0x7e00 and must come back as it went."""
    for pose in ('oblique', 'outside_z'):
        for stride in (C, C + 3):
            c = ref.tiny_label_case(shape, pose, C=C, prob_stride=stride)
            assert c['volume'].shape[-1] == record_size(C) and c['probs'].shape[-1] == stride
            for form in ('labels', 'probs') if stride == C else ('probs',):
                want = c['volume'].copy()
                n = _ref_case(want, c, form)
                assert n[0]['updates'] >= 20
                got = _dev(c['volume'], cuda)
                _fuse_case(got, c, cuda, form)
                _same(got, want, '{} C={} {} stride {} {}'.format(shape, C, pose, stride, form))
                assert (_bits(got)[..., C + 1:] == ref.PAD_BITS).all()


# ---- 2. views per call -------------------------------------------------------------------------------------------------------
def test_views_per_call_do_not_change_the_bits(cuda):
    shape = (16, 16, 16)
    poses = ref.POSES[:4]
    cs = [ref.tiny_label_case(shape, p) for p in poses]
    c = cs[0]
    assert 33 > _lib.LABEL_MAX_VIEWS
    rng = np.random.default_rng(12)
    for form in ('labels', 'probs'):
        def run(obs, depths, Es, per_call):
            vol = _dev(c['volume'], cuda)
            for v0 in range(0, len(obs), per_call):
                s = slice(v0, v0 + per_call)
                _fuse_case(vol, c, cuda, form, obs=obs[s], depth=depths[s], E=Es[s])
            return vol
        three = (np.stack([k[form] for k in cs[:3]]), np.stack([k['depth'] for k in cs[:3]]), np.stack([k['E'] for k in cs[:3]]))
        single = run(*three, 1)
        want = c['volume'].copy()
        ref.fuse(want, c['n_classes'], c['origin'], c['res'], three[1], c['K'], three[2], band=c['band'], max_weight=c['label_max_weight'],
                 **{form: three[0]})
        _same(single, want, 'three single calls against the reference')
        _same(run(*three, 3), single, 'three views in one call')
        # 33 views: the poses cycled, each view with an observation of its own; the wrapper cuts them into 32 + 1
        idx = [i % len(cs) for i in range(33)]
        obs = np.stack([cs[i][form] for i in idx])
        if form == 'labels':
            obs = rng.integers(0, 40, obs.shape).astype(np.uint8)
        else:
            obs = np.where(np.isfinite(obs), rng.random(obs.shape).astype(np.float32), obs)
        many = (obs, np.stack([cs[i]['depth'] for i in idx]), np.stack([cs[i]['E'] for i in idx]))
        _same(run(*many, 33), run(*many, 1), '33 views through the wrapper against 33 calls ({})'.format(form))


# ---- 3. decide_labels --------------------------------------------------------------------------------------------------------
def _decide_volume(shape, C, rot, seed=0):
    """A seeded start volume with the special records planted at voxels 0..8 (rotated by ``rot``, so that the eight voxels of
    (2,2,2) see all of them in two cases): two classes at 0.5, all classes equal, class 0 ahead, the last class ahead, and a
    clear winner under W = 0, -0, -1, NaN (all left alone) and 2^-24 (decided)."""
    rng = np.random.default_rng([seed, 92, C] + list(shape))
    vol = ref.start_volume(shape, C, rng)
    S = ref.record_size(C)
    flat = vol.reshape(-1, S)
    a, b = (0, 1) if C < 3 else (1, C - 1)
    specials = []
    for kind in range(9):
        r = np.zeros(C + 1, np.float16)
        if kind == 0:
            r[a] = r[b] = 0.5
            r[C] = 3
        elif kind == 1:
            r[:C] = np.float16(1.0 / C)
            r[C] = 1
        elif kind == 2:
            r[:C] = np.float16(0.3 / C)
            r[0], r[C] = 0.7, 2
        elif kind == 3:
            r[:C] = np.float16(0.3 / C)
            r[C - 1], r[C] = 0.7, 2
        else:
            r[C - 1], r[0] = 0.9, 0.1
            r[C] = (0.0, -0.0, -1.0, np.nan, 2.0 ** -24)[kind - 4]
        specials.append(r)
    planted = {}
    for i in range(min(len(flat), 9)):
        kind = (i + rot) % 9
        flat[i, :C + 1] = specials[kind]
        planted[i] = kind
    return vol, planted, (a, C - 1)


@pytest.mark.parametrize('shape,rot', [((2, 2, 2), 0), ((2, 2, 2), 4), ((5, 7, 19), 0), ((1, 5, 13), 0), ((1, 1, 257), 2)])
@pytest.mark.parametrize('C', [7, 30, 256])
def test_decide_labels(cuda, shape, rot, C):
    """(2,2,2); (5,7,19); 65 = 64 + 1 and 257 = 4 * 64 + 1 voxels (a second wave / a second block of one lane)."""
    vol, planted, (tie, last) = _decide_volume(shape, C, rot)
    ids = np.full(shape, 0xA5, np.uint8)
    scores = np.full(shape, -1234.0, np.float16)
    want_ids, want_scores = ids.copy(), scores.copy()
    n = ref.decide(vol, C, want_ids, want_scores)
    assert 0 < n < vol[..., 0].size or vol[..., 0].size == 8
    expect = {0: tie, 1: 0, 2: 0, 3: last, 4: 0xA5, 5: 0xA5, 6: 0xA5, 7: 0xA5, 8: last}
    for i, kind in planted.items():  # the restatement follows the stated rules
        assert want_ids.reshape(-1)[i] == expect[kind], (i, kind)
        assert (want_scores.reshape(-1)[i] == np.float16(-1234.0)) == (kind in (4, 5, 6, 7))
    got_ids, got_scores = _dev(ids, cuda), _dev(scores, cuda)
    dvol = _dev(vol, cuda)
    decide_labels(dvol, C, got_ids, got_scores)
    _same(got_ids, want_ids, 'ids')
    _same(got_scores, want_scores, 'scores')
    _same(dvol, vol, 'the volume is read only')


# ---- 4. softmax ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [2, 19, 30, 65])  # 65: past the 64 classes the vector form holds in registers
def test_softmax_rows(cuda, C):
    """1, 63, 64, 65 and 12 x 16 pixels, rows padded to 8 floats (the vector form up to 64 classes) and tight rows (stride C:
    off the 16-byte grid for these C), with the planted rows of stream_ops_cases (NaN, +Inf, only -Inf, a tie, -Inf among finite
    values); the output rows are C + 3 floats apart inside a guarded buffer.  Row maximum and first arg max: the bits of
    ojf_seg_softmax_max on the same input.  Every probability within 1e-6 of the float64 softmax (the bound the scores are held
    to), bad rows all NaN."""
    _lib.require_gpu()
    L, st = _lib.load(), _lib.stream_ptr(cuda)
    images = [(npix, cases.softmax_image(C, npix, npix)) for npix in (1, 63, 64, 65, 12 * 16)]
    images += [(1, row[None]) for k, kind in enumerate(('nan_later', 'inf_later', 'all_ninf', 'tie'))
               for row in [cases.planted_row(kind, C, k)] if row is not None]
    worst = 0.0
    for npix, logits in images:
        _, bad = ref.softmax(logits)
        with np.errstate(all='ignore'):
            l64 = logits.astype(np.float64)
            e = np.exp(l64 - l64.max(axis=1, keepdims=True))
            want = e / e.sum(axis=1, keepdims=True)
        if npix >= 63:
            assert bad.sum() >= 3 and not bad.all()
        for stride in ((C + 7) // 8 * 8, C):
            inp = Rows(cuda, logits, stride)
            out = Guarded(cuda, npix, C, stride=C + 3)
            assert L.ojf_seg_softmax(inp.ptr, stride, C, npix, out.ptr, C + 3, st) == 0
            scores, ids = Guarded(cuda, 1, npix), Guarded(cuda, 1, npix, dtype=np.uint8)
            assert L.ojf_seg_softmax_max(inp.ptr, stride, C, npix, scores.ptr, ids.ptr, st) == 0
            got, s, i = out.read(), scores.read()[0], ids.read()[0]
            assert np.array_equal(np.isnan(got), np.repeat(bad[:, None], C, axis=1)), (npix, stride)
            with np.errstate(all='ignore'):
                top = got.max(axis=1)  # (NaN for a bad row)
            assert cases.same_bits(top, s), (npix, stride)
            assert np.array_equal(np.where(bad, 0, np.argmax(np.where(np.isnan(got), -1.0, got), axis=1)).astype(np.uint8), i), (npix, stride)
            if (~bad).any():
                worst = max(worst, float(np.abs(got[~bad].astype(np.float64) - want[~bad]).max()))
    print('softmax C={}: worst |p - float64 softmax| {:.3e}'.format(C, worst))
    assert worst <= 1e-6


def test_segconv_softmax_and_predict_probs(cuda):
    """segconv.softmax on an NHWC view, and SegEngine.predict_probs against predict on the same frame (the engine's dropout
    counter set back in between: the same forward pass): the maximum over the classes and its first index are predict's."""
    from online_joint_depthfusion_and_semantic_amd.adapnet import AdapNet
    from online_joint_depthfusion_and_semantic_amd.adapnet_engine import SegEngine
    from online_joint_depthfusion_and_semantic_amd.config import AttrDict
    C, h, w = 19, 12, 16
    logits = cases.softmax_logits(C, h * w, 3)
    x = _dev(logits, cuda).view(1, h, w, C).permute(0, 3, 1, 2)  # an NHWC view [1, C, h, w]
    probs = segconv.softmax(x)
    s, i = segconv.softmax_max(x)
    assert probs.shape == (h * w, 20) and not probs[:, C:].any()
    assert torch.equal(probs[:, :C].max(dim=1).values, s) and torch.equal(probs[:, :C].argmax(dim=1).to(torch.uint8), i)
    torch.manual_seed(5)
    net = AdapNet(AttrDict({'stage': 2, 'n_classes': 12})).cuda().eval()
    g = torch.Generator().manual_seed(6)
    image, depth = (torch.rand((1, 3, 32, 48), generator=g) * 255).cuda(), (torch.rand((1, 32, 48), generator=g) * 3).cuda()
    with torch.no_grad():
        eng = SegEngine(net)
        state = eng.rng.clone()
        scores, ids = eng.predict(image, depth)
        eng.rng.copy_(state)
        p = eng.predict_probs(image, depth)
    assert p.shape == (32, 48, 12) and p.dtype == torch.float32
    assert float((p.sum(dim=-1) - 1.0).abs().max()) <= 1e-5
    assert torch.equal(p.max(dim=-1).values.reshape(-1), scores) and torch.equal(p.argmax(dim=-1).reshape(-1).to(torch.uint8), ids)


# ---- 5. the public layers ------------------------------------------------------------------------------------------------------
H, W, GRID, FRAMES = 48, 64, 64, 6


def _room(cuda, model, fuse_label_probs=True):
    cfg = default_config(H, W, semantics=True, model=model)
    cfg.SETTINGS.device = str(cuda)
    cfg.FUSION_MODEL.fuse_label_probs = fuse_label_probs
    ds = synthetic.SyntheticDataset(H, W, GRID, FRAMES, scenes=['room_0', 'room_1'])
    frames = {s: [ds.streams[s].frame(i) for i in range(FRAMES)] for s in ds.scenes}
    return cfg, ds, frames


def _direct(frames, cuda, band, C=30):
    origin, res, _ = synthetic.grid_spec(GRID)
    vol = new_volume((GRID,) * 3, C, cuda)
    for f in frames:
        integrate_label_probs(vol, C, origin=origin, resolution=res, depth=_dev(f['tof_depth'], cuda), intrinsics=f['intrinsics'],
                              extrinsics=f['extrinsics'], mask=_dev(f['mask'], cuda), labels=_dev(f['semantic_gt'], cuda), band=band)
    return vol


def test_database_layers(cuda, tmp_path):
    cfg, ds, frames = _room(cuda, 'tsdf')
    fr = frames['room_0']
    C = cfg.SEMANTIC_2D_MODEL.n_classes
    db = Database(ds, database_config(cfg))
    assert db.label_probs == {} and 'label_probs' not in db['room_0']
    with pytest.raises(ValueError):
        db.decide_labels('room_0')
    db.decide_labels()  # (no scene has a volume: nothing to do)
    for f in fr:
        db.integrate_depth('room_0', f['tof_depth'], f['intrinsics'], f['extrinsics'], mask=f['mask'], labels=f['semantic_gt'],
                           label_scores=f['semantic_scores'])
        db.integrate_label_probs('room_0', f['tof_depth'], f['intrinsics'], f['extrinsics'], mask=f['mask'], labels=f['semantic_gt'])
    want = _direct(fr, cuda, cfg.DATA.init_value)
    assert want.shape == (GRID,) * 3 + (32,) and int((want[..., C] > 0).sum()) > 1000
    _same(db.label_probs['room_0'], want, 'Database.integrate_label_probs')
    assert db['room_0']['label_probs'] is db.label_probs['room_0'] and 'label_probs' not in db['room_1'] and list(db.label_probs) == ['room_0']
    # the probability form: one-hot rows are the label votes
    other = Database(ds, database_config(cfg))
    for f in fr:
        onehot = np.zeros((H, W, 32), np.float32)
        np.put_along_axis(onehot, f['semantic_gt'][..., None].astype(np.int64), 1.0, axis=-1)
        other.integrate_label_probs('room_0', f['tof_depth'], f['intrinsics'], f['extrinsics'], mask=f['mask'], probs=onehot)
    _same(other.label_probs['room_0'], want, 'one-hot probabilities')
    with pytest.raises(ValueError):
        other.integrate_label_probs('room_0', fr[0]['tof_depth'], fr[0]['intrinsics'], fr[0]['extrinsics'])  # neither form
    bare = default_config(H, W, semantics=False, model='tsdf')
    bare.SETTINGS.device = str(cuda)
    with pytest.raises(ValueError):
        Database(ds, database_config(bare)).integrate_label_probs('room_0', fr[0]['tof_depth'], fr[0]['intrinsics'], fr[0]['extrinsics'],
                                                                  labels=fr[0]['semantic_gt'])

    ids, scores = db.ids_est['room_0'].volume.cpu().numpy().copy(), db.scores['room_0'].volume.cpu().numpy().copy()
    n = ref.decide(want.cpu().numpy(), C, ids, scores)
    assert n > 1000
    db.decide_labels()
    _same(db.ids_est['room_0'].volume, ids, 'Database.decide_labels: ids')
    _same(db.scores['room_0'].volume, scores, 'Database.decide_labels: scores')
    results, per_scene = db.evaluate_semantics(mode='test')
    assert 'room_0' in per_scene and results  # (evaluate_semantics runs on the decided ids)

    db.save(str(tmp_path), 'tsdf', 'room_0')
    assert sorted(n.split('.')[1] for n in os.listdir(str(tmp_path))) == ['label_probs', 'semantics', 'tsdf', 'weights']
    db.to_numpy()
    assert isinstance(db.label_probs['room_0'], np.ndarray) and db.label_probs['room_0'].dtype == np.float16
    with pytest.raises(ValueError):
        db.decide_labels('room_0')  # host state
    db.to_torch()
    _same(db.label_probs['room_0'], want, 'to_numpy / to_torch')
    assert db.label_probs['room_0'].data_ptr() % 16 == 0
    db.reset('room_0')
    assert db.label_probs['room_0'].is_cuda and not db.label_probs['room_0'].any() and not db.state['room_0']
    db.remove('room_0')
    assert 'room_0' not in db.label_probs


@pytest.mark.parametrize('model', ['tsdf', 'v3'])
def test_pipeline_votes_and_leaves_the_other_volumes_alone(cuda, model):
    """fuse, fuse_sequence and fuse_many (two scenes) with FUSION_MODEL.fuse_label_probs (semantic_strategy gt): the label volumes
    of direct calls with the same frames, and the TSDF / weight / id / score volumes of a run without it."""
    vols = {}
    for on in (True, False):
        cfg, ds, frames = _room(cuda, model, fuse_label_probs=on)
        assert default_config().FUSION_MODEL.fuse_label_probs is False and cfg.FUSION_MODEL.label_band == cfg.DATA.init_value
        db = Database(ds, database_config(cfg))
        torch.manual_seed(3)
        pipe = Pipeline(cfg).to(cuda).eval()
        batches = {s: [ds.streams[s].batch(i) for i in range(FRAMES)] for s in ds.scenes}

        def snapshot(stage):
            for s in ds.scenes:
                vols[(on, stage, s)] = [v.clone() for v in (db.scenes_est[s].volume, db.fusion_weights[s], db.ids_est[s].volume,
                                                            db.scores[s].volume)] + [db.label_probs[s].clone() if s in db.label_probs else None]
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
        if not on:
            assert db.label_probs == {}
    band = default_config().DATA.init_value
    want = {s: _direct(frames[s], cuda, band) for s in ('room_0', 'room_1')}
    want_two = _direct(frames['room_1'][:2], cuda, band)
    assert int((want['room_0'][..., 30] > 0).sum()) > 1000
    for stage, scenes in (('fuse', {'room_0': want['room_0']}), ('fuse_sequence', {'room_0': want['room_0'], 'room_1': want_two}),
                          ('fuse_many', want)):
        for s in ('room_0', 'room_1'):
            with_, without = vols[(True, stage, s)], vols[(False, stage, s)]
            if s in scenes:
                _same(with_[4], scenes[s], '{} {}: label volume'.format(stage, s))
            else:
                assert with_[4] is None or not with_[4].any()
            assert without[4] is None
            for name, a, b in zip(('tsdf', 'weights', 'ids', 'scores'), with_, without):
                _same(a, b, '{} {}: {} with and without fuse_label_probs'.format(stage, s, name))
        assert (vols[(True, stage, 'room_0')][1] > 0).sum() > 1000


def test_pipeline_predict_strategy_in_fuse_many_is_refused(cuda):
    cfg, ds, _ = _room(cuda, 'v3')
    cfg.DATA.semantic_strategy = 'predict'
    pipe = Pipeline(cfg)  # (refused in front of any device work)
    db = Database(ds, database_config(cfg))
    with pytest.raises(ValueError, match='fuse_many'):
        pipe.fuse_many([ds.streams['room_0'].batch(0), ds.streams['room_1'].batch(0)], db, cuda)
    assert db.label_probs == {} and not db.state['room_0']


# ---- 6. noisy labels: the vote against the one-slot rule, end to end ---------------------------------------------------------
def test_vote_beats_the_one_slot_rule_on_noisy_labels(cuda):
    """The experiment of test_label_probs_host.py (20 frames at 48 x 64 into 64^3, 16 classes, q = 0.2, seed 7, band 0.1 m) on the
    device: the one-slot rule through Database.integrate_depth(labels=, label_scores=), the vote through integrate_label_probs +
    decide_labels; each against what the same rule fuses from the clean label images.  The same two conditions.
    Measured on an MI355X: 16 089 observed voxels, one-slot 0.8177, vote 0.9218; 8 890 with W >= 3: vote 0.9874 - the host figures."""
    st, frames = ref.noisy_frames(q=0.2, seed=7)
    C = ref.NOISE_CLASSES
    cfg = default_config(ref.NOISE_H, ref.NOISE_W, semantics=True, model='tsdf', n_classes=C)
    cfg.SETTINGS.device = str(cuda)
    out = {}
    for kind in ('labels_clean', 'labels_noisy'):
        slot, vote = Database(st, database_config(cfg)), Database(st, database_config(cfg))
        for f in frames:
            args = ('room_0', f['depth_gt'], f['intrinsics'], f['extrinsics'])
            slot.integrate_depth(*args, mask=f['mask'], labels=f[kind], label_scores=f['label_scores'], truncation=ref.NOISE_BAND)
            vote.integrate_label_probs(*args, mask=f['mask'], labels=f[kind], band=ref.NOISE_BAND)
        vote.decide_labels()
        out[kind] = (slot.ids_est['room_0'].volume.cpu().numpy(), vote.ids_est['room_0'].volume.cpu().numpy(),
                     vote.label_probs['room_0'][..., C].float().cpu().numpy())
    observed, thrice = out['labels_clean'][2] > 0, out['labels_clean'][2] >= 3
    slot_a = ref.agreement(out['labels_noisy'][0], out['labels_clean'][0], observed)
    vote_a = ref.agreement(out['labels_noisy'][1], out['labels_clean'][1], observed)
    vote3 = ref.agreement(out['labels_noisy'][1], out['labels_clean'][1], thrice)
    print('noisy labels on the device: {} observed, one-slot {:.4f}, vote {:.4f}; {} with W >= 3: vote {:.4f}'.format(
        int(observed.sum()), slot_a, vote_a, int(thrice.sum()), vote3))
    assert observed.sum() > 15000 and thrice.sum() > 8000
    assert vote_a >= slot_a + 0.05, (vote_a, slot_a)
    assert vote3 >= 0.95, vote3


# ---- 7. argument errors ------------------------------------------------------------------------------------------------------
def test_argument_errors_are_value_errors(cuda):
    C = 5
    vol = new_volume((8, 8, 8), C, cuda)
    d = torch.full((4, 4), 0.5, device=cuda)  # (voxels k = 4, 5 of the 0.1-m grid lie within the band of it)
    lab = torch.full((4, 4), 3, dtype=torch.uint8, device=cuda)
    pr = torch.full((4, 4, C), 0.2, device=cuda)
    K, E = np.array([[4.0, 0, 2], [0, 4.0, 2], [0, 0, 1]]), np.eye(4)
    kw = dict(origin=np.zeros(3), resolution=0.1, depth=d, intrinsics=K, extrinsics=E, labels=lab, band=0.1)
    skew = K.copy()
    skew[0, 1] = 0.1
    bad = [dict(kw, depth=d.cpu()), dict(kw, labels=lab.cpu()), dict(kw, labels=lab[:3]), dict(kw, labels=lab.to(torch.int32)),
           dict(kw, labels=None), dict(kw, probs=pr), dict(kw, labels=None, probs=pr[..., :4]), dict(kw, labels=None, probs=pr.cpu()),
           dict(kw, labels=None, probs=pr[:3]), dict(kw, labels=None, probs=pr.to(torch.int32)),
           dict(kw, intrinsics=np.stack([K] * 3)), dict(kw, intrinsics=skew), dict(kw, extrinsics=np.full((3, 4), np.nan)),
           dict(kw, band=0.0), dict(kw, band=float('inf')), dict(kw, max_weight=0.5), dict(kw, max_weight=4096), dict(kw, near=-1.0),
           dict(kw, mask=torch.ones(5, dtype=torch.bool, device=cuda)), dict(kw, depth=torch.ones((0, 4, 4), device=cuda))]
    for case in bad:
        with pytest.raises(ValueError):
            integrate_label_probs(vol, C, **case)
    ids, scores = torch.zeros((8, 8, 8), dtype=torch.uint8, device=cuda), torch.zeros((8, 8, 8), dtype=torch.float16, device=cuda)
    buf = torch.zeros(8 * 8 * 8 * 8 + 4, dtype=torch.float16, device=cuda)
    for wrong in (vol.float(), vol[..., :7], vol[:, :, ::2], vol.cpu(), vol.view(8, 8, 64), buf[4:].view(8, 8, 8, 8)):  # (the last: 8 B off the grid)
        with pytest.raises(ValueError):
            integrate_label_probs(wrong, C, **kw)
        with pytest.raises(ValueError):
            decide_labels(wrong, C, ids, scores)
    for n_classes in (1, 257, 9):  # (9 classes want S = 16)
        with pytest.raises(ValueError):
            integrate_label_probs(vol, n_classes, **kw)
    for i, s in ((ids.cpu(), scores), (ids, scores.float()), (ids[:4], scores), (ids, scores[:, :, ::2])):
        with pytest.raises(ValueError):
            decide_labels(vol, C, i, s)
    assert not vol.any()
    integrate_label_probs(vol, C, **kw)  # the well-formed calls are what works
    integrate_label_probs(vol, C, **dict(kw, labels=None, probs=pr))
    decide_labels(vol, C, ids, scores)
    assert vol.any() and set(ids.unique().tolist()) == {0, 3} and float(scores.max()) == float(np.float16(0.6))
