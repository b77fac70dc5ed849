"""Plain numpy restatement, in float64, of the full-grid Database passes in csrc/ojf_volume.hip (modules/database.py:108-112,
311-370; utils/metrics.py:69-127).  Nothing here imports the package: the host test (test_stream_ops_host.py) shows that
every function equals the numpy / torch expression of the reference, the GPU test (test_volume_gpu.py) holds the kernels
to them.  Volumes are flat arrays; fp16 volumes are np.float16."""
import math

import numpy as np


def fill(n, value):
    """Database.reset: n fp16 elements of float16(value)."""
    return np.full(n, np.float16(value), np.float16)


def filter(tsdf, weights, value, init_value):
    """Database.filter (database.py:108-112): ``weights < value`` on an fp16 array is evaluated in fp16 by numpy and torch,
    i.e. against float16(value) (0.1 -> 0.0999755859375: a weight of exactly that is KEPT).  Returns new (tsdf, weights)."""
    tsdf, weights = np.array(tsdf, np.float16), np.array(weights, np.float16)
    with np.errstate(over='ignore'):
        thr = np.float64(np.float16(value))
    low = weights.astype(np.float64) < thr  # NaN weights compare false: kept
    tsdf[low] = np.float16(init_value)
    weights[low] = np.float16(0)
    return tsdf, weights


def evaluate(est, gt, weights):
    """utils/metrics.py:111-127 with mask = weights > 0: nan_to_num (NaN -> 0, the infinities end at the clip), clip to
    +-float32(0.04), then over the masked voxels n, sum d^2, sum |d|, and the occupancy (value < 0) counts.  Returns mse,
    mad, iou, acc and the six raw sums in the order of ojf_volume_evaluate; the float sums are exact (math.fsum of
    float64 terms) up to the one rounding of each d * d."""
    clip = np.float64(np.float32(0.04))

    def prep(a):
        a = np.asarray(a, np.float16).astype(np.float64).ravel()
        a = np.where(np.isnan(a), 0.0, a)
        return np.minimum(np.maximum(a, -clip), clip)
    e, g = prep(est), prep(gt)
    m = np.asarray(weights, np.float16).astype(np.float64).ravel() > 0  # NaN, 0, negative: masked out
    d = e[m] - g[m]
    eo, go = e[m] < 0, g[m] < 0  # (-0.0 is not occupied)
    sums = [float(m.sum()), math.fsum(d * d), math.fsum(np.abs(d)), float((eo & go).sum()), float((eo | go).sum()),
            float((eo == go).sum())]
    n, sq, ab, inter, union, same = sums
    eps = 1.e-10
    return {'mse': sq / (n + eps), 'mad': ab / (n + eps), 'iou': inter / (union + eps), 'acc': same / (n + eps), 'sums': sums}


def confusion(est, gt, weights, n_classes):
    """Database.evaluate_semantics -> utils/metrics.py:69-108: with mask = weights > 0, est' = est * mask, gt' = gt * mask,
    hist.flat[gt' * C + est'] += 1 for gt' < C, as the reference's bincount of the flat index does: an est' >= C lands in a
    later row, and an index >= C * C (where the reference's reshape raises) is dropped.  Returns (hist int64 [C, C],
    est_present bool [256], gt_present bool [256], dropped): the presence vectors cover all 256 labels, ``dropped`` counts
    the voxels that are in no cell."""
    C = int(n_classes)
    m = np.asarray(weights, np.float16).astype(np.float64).ravel() > 0
    e = np.where(m, np.asarray(est, np.uint8).ravel(), 0).astype(np.int64)
    g = np.where(m, np.asarray(gt, np.uint8).ravel(), 0).astype(np.int64)
    hist = np.zeros(C * C, np.int64)
    idx = g * C + e
    keep = (g < C) & (idx < C * C)
    np.add.at(hist, idx[keep], 1)
    pe, pg = np.zeros(256, bool), np.zeros(256, bool)
    pe[e] = True
    pg[g] = True
    return hist.reshape(C, C), pe, pg, int((~keep).sum())
