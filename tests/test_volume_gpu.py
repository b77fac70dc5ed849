"""-m gpu: full-grid Database passes on device against their host definitions (bit-exact for u8/fp16 work).  The tests
from ``test_fill_f16_...`` on call the C ABI on guarded buffers (stream_ops_cases.Guarded: sentinels before and behind the
target, which must survive) and compare with volume_ref.py, which test_stream_ops_host.py proves against numpy / torch."""
import numpy as np
import pytest
import torch
from scipy.ndimage import median_filter

import stream_ops_cases as cases
import volume_ref
from stream_ops_cases import Guarded, same_bits
from online_joint_depthfusion_and_semantic_amd import ops

H16 = np.float16

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('shape', [(32, 32, 32), (17, 9, 30), (64, 40, 8), (5, 5, 5), (3, 2, 1)])
def test_median5_matches_scipy(cuda, shape):
    rng = np.random.default_rng(sum(shape))
    # blobs of labels plus salt noise: the regime filter_semantics is used in
    vol = (rng.integers(0, 40, size=[(s + 3) // 4 for s in shape]).repeat(4, 0).repeat(4, 1).repeat(4, 2))[:shape[0], :shape[1], :shape[2]]
    vol = np.where(rng.random(shape) < 0.2, rng.integers(0, 256, size=shape), vol).astype(np.uint8)
    vol = np.ascontiguousarray(vol)
    want = median_filter(vol, size=5)  # modules/database.py:116
    got = ops.volume_median5(torch.from_numpy(vol).to(cuda)).cpu().numpy()
    assert np.array_equal(got, want)


def test_fill_filter_known_answers(cuda):
    t = torch.empty((9, 7, 13), dtype=torch.float16, device=cuda)
    ops.volume_fill(t, 0.1)
    assert torch.all(t == torch.tensor(0.1, dtype=torch.float16))
    w = torch.tensor(np.linspace(0, 4, 9 * 7 * 13).reshape(9, 7, 13).astype(np.float16)).to(cuda)
    w0 = w.clone()
    t.fill_(-0.02)
    ops.volume_filter(t, w, 2.0, 0.1)
    low = w0 < 2.0
    assert torch.all(t[low] == torch.tensor(0.1, dtype=torch.float16)) and torch.all(w[low] == 0)
    assert torch.all(t[~low] == torch.tensor(-0.02, dtype=torch.float16)) and torch.equal(w[~low], w0[~low])
    u = torch.ones((5, 5, 5), dtype=torch.uint8, device=cuda)
    ops.volume_fill(u, 0)
    assert int(u.sum()) == 0


@pytest.mark.parametrize('shape,n_classes,offset', [((32, 32, 32), 30, 0), ((17, 9, 31), 40, 0), ((64, 40, 9), 30, 3),
                                                    ((5, 5, 5), 12, 1), ((33, 20, 16), 100, 0), ((16, 16, 16), 256, 0)])
def test_confusion_counts_and_semantic_metrics(cuda, shape, n_classes, offset):
    """ojf_volume_confusion == the counts inside utils/metrics.py:69-108 (np.bincount of target * C + est on masked
    volumes, np.unique presence); the metrics computed from them are then the same floats.  ``offset`` misaligns the
    device pointers (scalar path), C > 64 takes the global-atomics path."""
    from online_joint_depthfusion_and_semantic_amd import metrics
    rng = np.random.default_rng(sum(shape) + n_classes)
    n = int(np.prod(shape))
    hi = min(n_classes, 255)
    est = rng.integers(0, hi, size=n).astype(np.uint8)
    gt = np.where(rng.random(n) < 0.7, est, rng.integers(0, hi, size=n)).astype(np.uint8)
    wgt = np.where(rng.random(n) < 0.4, rng.random(n) * 5, 0).astype(np.float16)

    def dev(a):
        buf = torch.zeros(n + 8, dtype=torch.from_numpy(a).dtype, device=cuda)
        view = buf[offset:offset + n]
        view.copy_(torch.from_numpy(a))
        return view.view(shape)
    hist, e_ids, g_ids = ops.volume_confusion(dev(est), dev(gt), dev(wgt), n_classes)
    m = wgt > 0
    e, g = est * m, gt * m
    want = np.bincount(n_classes * g.astype(np.uint16).astype(np.int64) + e, minlength=n_classes * n_classes).reshape(n_classes, n_classes)
    assert np.array_equal(hist, want) and hist.sum() == n
    assert np.array_equal(np.flatnonzero(e_ids), np.unique(e)) and np.array_equal(np.flatnonzero(g_ids), np.unique(g))
    want_m, want_iou = metrics.semantic_evaluation(est.reshape(shape), gt.reshape(shape), m.reshape(shape), n_classes)
    got_m, got_iou = metrics.semantic_metrics_from_counts(hist, e_ids[:n_classes], g_ids[:n_classes])
    assert got_m == want_m and got_iou.keys() == want_iou.keys() and all(got_iou[k] == want_iou[k] for k in want_iou)


@pytest.mark.parametrize('offset', [0, 3])
def test_confusion_reproduces_the_reference_fixture(cuda, offset):
    """tests/golden/semantic_evaluation_12.npz: the reference's own utils/metrics.py on a 12^3 case with classes on one
    side only, a class hidden by the mask and classes that occur nowhere.  The metrics from ojf_volume_confusion's counts
    are the reference's two returned values, exactly; the counts are volume_ref.confusion's."""
    from helpers import golden
    from online_joint_depthfusion_and_semantic_amd import metrics
    g = golden('semantic_evaluation_12.npz')
    C = int(g['n_class'])
    est, gt, w = g['est'].ravel(), g['target'].ravel(), g['mask'].ravel().astype(H16)
    hist, pe, pg = raw_confusion(cuda, est, gt, w, C, offset)
    want, want_pe, want_pg, dropped = volume_ref.confusion(est, gt, w, C)
    assert dropped == 0 and np.array_equal(hist, want) and np.array_equal(pe, want_pe) and np.array_equal(pg, want_pg)
    m, iou = metrics.semantic_metrics_from_counts(hist, pe[:C], pg[:C])
    assert m == {'Mean Acc': float(g['mean_acc']), 'Mean IoU': float(g['mean_iou'])}
    assert {int(k): float(v) for k, v in iou.items()} == dict(zip(g['cls_ids'].tolist(), g['cls_iou'].tolist()))


def test_database_evaluate_semantics_on_device(cuda):
    """Database.evaluate_semantics (modules/database.py:311-349) with device-resident volumes == the host path."""
    from online_joint_depthfusion_and_semantic_amd.config import default_config, database_config
    from online_joint_depthfusion_and_semantic_amd.database import Database
    from online_joint_depthfusion_and_semantic_amd.synthetic import SyntheticStream
    cfg = default_config(24, 32, semantics=True)
    cfg.SETTINGS.device = str(cuda)
    st = SyntheticStream(24, 32, 32, 5)
    db = Database(st, database_config(cfg))
    s = st.scene
    rng = np.random.default_rng(2)
    gt = db.ids_gt[s].volume.cpu().numpy()
    est = np.where(rng.random(gt.shape) < 0.8, gt, rng.integers(0, 30, size=gt.shape)).astype(np.uint8)
    db.ids_est[s].volume = torch.from_numpy(est).to(cuda)
    db.fusion_weights[s] = torch.from_numpy((rng.random(gt.shape) < 0.3).astype(np.float16) * 2).to(cuda)
    db.state[s] = True
    quiet = type('W', (), {'log': staticmethod(lambda *a: None)})
    on_dev, iou_dev = db.evaluate_semantics(mode='test', workspace=quiet)
    db.to_numpy()
    on_host, iou_host = db.evaluate_semantics(mode='test', workspace=quiet)
    assert on_dev == on_host and on_dev['Mean IoU'] > 0.3
    assert iou_dev[s].keys() == iou_host[s].keys() and all(iou_dev[s][k] == iou_host[s][k] for k in iou_host[s])


# ---- ojf_volume_* at their edges: heads, tails, grid-stride loops, non-finite values -------------------------------
def api(cuda):
    from online_joint_depthfusion_and_semantic_amd import _lib
    _lib.require_gpu()
    return _lib.load(), _lib.stream_ptr(cuda)


def volume16(cuda, data, off=0):
    """A guarded fp16 volume [n] that starts ``off`` elements behind a 16-byte boundary."""
    g = Guarded(cuda, 1, len(data), dtype=H16, lead=8 + off, tail=16).write(data)
    assert g.ptr % 16 == 2 * off
    return g


@pytest.mark.parametrize('n', cases.FILL_SIZES)
def test_fill_f16_heads_tails_and_bounds(cuda, n):
    """ojf_volume_fill_f16 on a view 0 .. 7 elements behind a 16-byte boundary: the scalar head (up to 7 elements), n
    smaller than the head, the 16-byte body, the tail, and for 2048 * 256 * 8 + 29 elements the grid-stride loop; 0.1
    (rounded to fp16), -0.0 (its sign bit) and 65504.  Every element equals the reference, the sentinels on both sides stay."""
    L, st = api(cuda)
    for off in range(8):
        for v in cases.FILL_VALUES:
            g = volume16(cuda, np.full(n, -1234.0, H16), off)
            assert L.ojf_volume_fill_f16(g.ptr, n, v, st) == 0
            assert same_bits(g.read()[0], volume_ref.fill(n, v)), (off, v)


@pytest.mark.parametrize('thr', cases.FILTER_THRESHOLDS)
@pytest.mark.parametrize('n', cases.STREAM_SIZES)
def test_filter_is_the_fp16_comparison_of_the_reference(cuda, n, thr):
    """ojf_volume_filter == volume_ref.filter (``weights < float16(thr)``) bit for bit at 2.0, 0.1 and 2.3, with
    float16(thr), its two fp16 neighbours, 0, -1, NaN and +Inf among the weights - float16(0.1) = 0.0999755859375 is below
    0.1f, so an fp32 comparison would reset the voxels that weigh exactly that - on 819 voxels and on more than the 2048 x 256
    threads of the grid (the planted weights sit in both passes of its loop); volumes at an odd offset, sentinels around."""
    L, st = api(cuda)
    tsdf, w = cases.filter_volume(n, thr)
    want_t, want_w = volume_ref.filter(tsdf, w, thr, 0.1)
    gt_, gw = volume16(cuda, tsdf, 3), volume16(cuda, w, 5)
    assert L.ojf_volume_filter(gt_.ptr, gw.ptr, n, thr, 0.1, st) == 0
    got_t, got_w = gt_.read()[0], gw.read()[0]
    at = w == H16(thr)
    assert at.sum() >= 2 and same_bits(got_w[at], w[at]) and same_bits(got_t[at], tsdf[at])  # float16(thr) itself is kept
    assert same_bits(got_w, want_w) and same_bits(got_t, want_t)


def test_database_filter_device_path_equals_host_path(cuda):
    """Database.filter(0.1) on device-resident volumes == on numpy volumes, bit for bit, float16(0.1) weights included."""
    from online_joint_depthfusion_and_semantic_amd.config import default_config, database_config
    from online_joint_depthfusion_and_semantic_amd.database import Database
    from online_joint_depthfusion_and_semantic_amd.synthetic import SyntheticStream
    cfg = default_config(24, 32, semantics=True)
    cfg.SETTINGS.device = str(cuda)
    st = SyntheticStream(24, 32, 32, 5)
    db = Database(st, database_config(cfg))
    s = st.scene
    shape = tuple(db.scenes_est[s].volume.shape)
    tsdf, w = cases.filter_volume(int(np.prod(shape)), 0.1)
    tsdf, w = tsdf.reshape(shape), w.reshape(shape)
    db.scenes_est[s].volume, db.fusion_weights[s] = torch.from_numpy(tsdf.copy()).to(cuda), torch.from_numpy(w.copy()).to(cuda)
    db.filter(0.1)
    dev_t, dev_w = db.scenes_est[s].volume.cpu().numpy(), db.fusion_weights[s].cpu().numpy()
    db.to_numpy()
    db.scenes_est[s].volume, db.fusion_weights[s] = tsdf.copy(), w.copy()
    db.filter(0.1)
    host_t, host_w = db.scenes_est[s].volume, db.fusion_weights[s]
    at = w == H16(0.1)
    assert at.sum() >= 2 and (host_w[at] == H16(0.1)).all() and (host_w == 0).sum() > (w == 0).sum()
    assert same_bits(dev_w, host_w) and same_bits(dev_t, host_t)


def raw_sums(cuda, est, gt, w):
    """The eight doubles ojf_volume_evaluate writes (n, sum d^2, sum |d|, intersection, union, sign-equal, 0, 0)."""
    L, st = api(cuda)
    sums = Guarded(cuda, 1, 8, dtype=np.float64)
    vols = [volume16(cuda, a, o) for a, o in ((est, 1), (gt, 0), (w, 6))]
    assert L.ojf_volume_evaluate(vols[0].ptr, vols[1].ptr, vols[2].ptr, len(est), sums.ptr, st) == 0
    return sums.read()[0]


@pytest.mark.parametrize('n', (1, 665) + cases.STREAM_SIZES[1:])
def test_evaluate_counts_and_sums(cuda, n):
    """ojf_volume_evaluate on one voxel, on 665 and past the 2048 x 256 threads of its grid, est / gt holding NaN, +-Inf, -0.0,
    float16(+-0.04) and its fp16 neighbours on either side of the clip, sign disagreements (every edge value against every
    other), weights 0, -0.0, negative, NaN, +-Inf, subnormal and positive.  n, intersection, union and sign-equal: equal to
    the reference.  Sums of d^2 and |d|: d = e - g and |d| are exact in double, d * d rounds once, and the n additions of
    non-negative terms (threads, shuffles, atomics, in any order) round once each: (n + 1) * 2^-53 <= n * 2^-52 relative.  iou
    and acc of ops.volume_evaluate equal metrics.evaluation exactly (ratios of the same counts)."""
    from online_joint_depthfusion_and_semantic_amd import metrics
    est, gt, w = cases.evaluate_volume(n)
    want = volume_ref.evaluate(est, gt, w)
    got = raw_sums(cuda, est, gt, w)
    assert [got[0], got[3], got[4], got[5]] == [want['sums'][0], want['sums'][3], want['sums'][4], want['sums'][5]]
    assert got[6] == 0 and got[7] == 0
    tol = n * 2.0 ** -52
    assert abs(got[1] - want['sums'][1]) <= tol * want['sums'][1] and abs(got[2] - want['sums'][2]) <= tol * want['sums'][2]
    shape = (n, 1, 1)
    r = ops.volume_evaluate(*[torch.from_numpy(a.reshape(shape)).to(cuda) for a in (est, gt, w)])
    assert abs(r['mse'] - want['mse']) <= tol * want['mse'] and abs(r['mad'] - want['mad']) <= tol * want['mad']
    with np.errstate(invalid='ignore'):
        host = metrics.evaluation(est, gt, w > 0)
    assert r['iou'] == host['iou'] == want['iou'] and r['acc'] == host['acc'] == want['acc']


def test_evaluate_of_an_all_masked_volume_is_zero(cuda):
    est, gt, w = cases.evaluate_volume(665)
    for masked in (np.zeros_like(w), np.full_like(w, np.nan), np.full_like(w, -1)):
        assert list(raw_sums(cuda, est, gt, masked)) == [0.0] * 8
        r = ops.volume_evaluate(*[torch.from_numpy(a.reshape(665, 1, 1)).to(cuda) for a in (est, gt, masked)])
        assert r == {'mse': 0.0, 'mad': 0.0, 'iou': 0.0, 'acc': 0.0}


def raw_confusion(cuda, est, gt, w, C, offset):
    """(hist [C, C], est_present [256], gt_present [256]) of ojf_volume_confusion on guarded buffers; ``offset`` elements
    misalign the three volumes (the scalar path)."""
    L, st = api(cuda)
    n = len(est)
    ge = Guarded(cuda, 1, n, dtype=np.uint8, lead=16 + offset, tail=16).write(est)
    gg = Guarded(cuda, 1, n, dtype=np.uint8, lead=16 + offset, tail=16).write(gt)
    gw = volume16(cuda, w, offset)
    hist, present = Guarded(cuda, 1, C * C, dtype=np.int64), Guarded(cuda, 1, 512, dtype=np.int32)
    assert L.ojf_volume_confusion(ge.ptr, gg.ptr, gw.ptr, n, C, hist.ptr, present.ptr, st) == 0
    for g in (ge, gg, gw):
        g.read()  # (inputs: untouched around and, below, inside)
    assert np.array_equal(ge.read()[0], est) and np.array_equal(gg.read()[0], gt)
    p = present.read()[0]
    assert set(np.unique(p)) <= {0, 1}
    return hist.read()[0].reshape(C, C), p[:256] != 0, p[256:] != 0


def test_confusion_past_the_vector_grid(cuda):
    """2048 * 256 * 8 + 29 voxels: the 8-voxel vector loop of ojf_volume_confusion grid-strides (and leaves a scalar tail).
    Counts and presence equal volume_ref.confusion; the metrics from them equal metrics.semantic_evaluation on the host."""
    from online_joint_depthfusion_and_semantic_amd import metrics
    n, C = cases.FILL_SIZES[-1], 30
    est, gt, w = cases.confusion_volume(n, C, False)
    hist, pe, pg = raw_confusion(cuda, est, gt, w, C, 0)
    want, want_pe, want_pg, dropped = volume_ref.confusion(est, gt, w, C)
    assert dropped == 0 and hist.sum() == n
    assert np.array_equal(hist, want) and np.array_equal(pe, want_pe) and np.array_equal(pg, want_pg)
    want_m, want_iou = metrics.semantic_evaluation(est, gt, w > 0, C)
    got_m, got_iou = metrics.semantic_metrics_from_counts(hist, pe[:C], pg[:C])
    assert got_m == want_m and got_iou.keys() == want_iou.keys() and all(got_iou[k] == want_iou[k] for k in want_iou)


@pytest.mark.parametrize('offset', [0, 3])
@pytest.mark.parametrize('C', [30, 100])
def test_confusion_with_labels_beyond_the_classes(cuda, C, offset):
    """est and gt labels in [C, 256), for the LDS histogram (C = 30) and the global one (C = 100): a pair with gt >= C is
    in no cell, an est >= C spills into a later row as the reference's flat index gt * C + est does, an index >= C * C is
    dropped; the presence vectors cover all 256 labels.  hist.sum() == n - dropped.  (The reference's own host path,
    metrics.semantic_evaluation, raises for any label >= C - test_stream_ops_host.py shows it - so volume_ref.confusion is
    the only yardstick here.)"""
    n = 40 * 33 * 17
    est, gt, w = cases.confusion_volume(n, C, True)
    hist, pe, pg = raw_confusion(cuda, est, gt, w, C, offset)
    want, want_pe, want_pg, dropped = volume_ref.confusion(est, gt, w, C)
    m = w > 0
    e, g = (est * m).astype(np.int64), (gt * m).astype(np.int64)
    assert dropped == int(((g >= C) | (g * C + e >= C * C)).sum()) > 0 and ((g < C) & (g * C + e >= C * C)).sum() > 0
    assert hist.sum() == n - dropped
    assert np.array_equal(hist, want) and np.array_equal(pe, want_pe) and np.array_equal(pg, want_pg)
    assert pe[C:].any() and pg[C:].any()
