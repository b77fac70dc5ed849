"""numpy restatement of the label volume's definition in csrc/ojf_labels.hip (ojf_fuse_label_probs, ojf_label_decide) and of
ojf_seg_softmax in csrc/ojf_seg_ops.hip: every fp32 operation is one numpy ufunc on float32 arrays (rounded on its own), the
host part of the projection comes from projective_ref.view_constants.  Also the cases the CPU and GPU tests share and the
noisy-label experiment both measure.  Test helper, not a test."""
import numpy as np

import projective_ref as pref
from projective_ref import view_constants, tiny_case, SHAPES, POSES, RES  # noqa: F401  (re-exported for the tests)

F = np.float32
MAX_WEIGHT = 8.0
BAND = 2.5 * RES
PAD_BITS = 0x7e00  # what the padding channels of the start volumes hold (a NaN: arithmetic on it would show)


def record_size(C):
    return 8 * ((C + 8) // 8)


def _views(depth, K, E):
    depth = np.asarray(depth, F)
    if depth.ndim == 2:
        depth = depth[None]
    n = depth.shape[0]
    K = np.broadcast_to(np.asarray(K, np.float64).reshape(-1, 3, 3), (n, 3, 3))
    E = np.asarray(E, np.float64)
    E = np.broadcast_to(E.reshape((-1,) + E.shape[-2:]), (n,) + E.shape[-2:])
    return depth, K, E


def fuse(vol, C, origin, res, depth, K, E, mask=None, probs=None, labels=None, *, band, max_weight=64.0, near=0.0):
    """In place on fp16 ``vol`` [X,Y,Z,S] for the views of ``depth`` f32 [n,h,w] (a single view may come without the leading
    axis) and exactly one of ``probs`` f32 [n,h,w,>=C] and ``labels`` u8 [n,h,w]; K [n,3,3] or [3,3], E [n,3,4] (or 4x4).
    Channels behind C are never read or written.  Returns per view a dict of counts: 'updates' (voxels that reach step 4)
    and, of the voxels inside the band, 'label_skips' (label >= C) and 'bad_probs' (class values replaced by 0)."""
    assert (probs is None) != (labels is None) and vol.shape[3] == record_size(C)
    depth, K, E = _views(depth, K, E)
    n, h, w = depth.shape
    mask = None if mask is None else np.asarray(mask).reshape(n, h, w)
    if probs is not None:
        probs = np.asarray(probs, F).reshape(n, h, w, -1)
    else:
        labels = np.asarray(labels, np.uint8).reshape(n, h, w)
    X, Y, Z = vol.shape[:3]
    x = np.arange(X, dtype=F)[:, None, None]
    y = np.arange(Y, dtype=F)[None, :, None]
    z = np.arange(Z, dtype=F)[None, None, :]
    band, max_weight, near = F(band), F(max_weight), F(near)
    counts = []
    with np.errstate(all='ignore'):
        for v in range(n):
            # steps 1-3 of ojf_fuse_projective
            A, b, fx, fy, cx, cy = view_constants(K[v], E[v][:3], origin, res)
            p = [((A[a, 0] * x + A[a, 1] * y) + A[a, 2] * z) + b[a] for a in range(3)]
            zc = p[2]
            ok = zc > near
            u = fx * (p[0] / zc) + cx
            q = fy * (p[1] / zc) + cy
            c = np.floor(u + F(0.5))
            r = np.floor(q + F(0.5))
            ok &= (c >= 0) & (c <= F(w - 1)) & (r >= 0) & (r <= F(h - 1))
            ci = np.where(ok, c, 0).astype(np.int64)
            ri = np.where(ok, r, 0).astype(np.int64)
            d = depth[v][ri, ci]
            ok &= np.isfinite(d) & (d > 0)
            if mask is not None:
                ok &= mask[v][ri, ci] != 0
            # 2. the band
            s = d - zc
            ok &= (s >= -band) & (s <= band)
            count = dict(updates=0, label_skips=0, bad_probs=0)
            # 3. the observation
            if labels is not None:
                lab = labels[v][ri, ci]
                count['label_skips'] = int((ok & (lab >= C)).sum())
                ok &= lab < C
            # 4., 5.
            w0 = vol[..., C].astype(F)
            w1 = w0 + F(1)
            for k in range(C):
                if labels is not None:
                    pk = np.where(lab == k, F(1), F(0))
                else:
                    xk = probs[v][ri, ci, k]
                    good = (xk >= 0) & (xk <= 1)
                    count['bad_probs'] += int((ok & ~good).sum())
                    pk = np.where(good, xk, F(0))
                Pk = (w0 * vol[..., k].astype(F) + pk) / w1
                vol[..., k][ok] = Pk.astype(np.float16)[ok]
            vol[..., C][ok] = np.minimum(w1, max_weight).astype(np.float16)[ok]
            count['updates'] = int(ok.sum())
            counts.append(count)
    return counts


def decide(vol, C, ids, scores):
    """In place on ``ids`` u8 [X,Y,Z] and ``scores`` fp16 [X,Y,Z]; returns the number of voxels decided."""
    with np.errstate(all='ignore'):
        seen = vol[..., C].astype(F) > 0  # (a NaN fails)
        best = vol[..., 0].astype(F)
        bits = vol[..., 0].view(np.uint16).copy()
        idx = np.zeros(vol.shape[:3], np.uint8)
        for k in range(1, C):
            xk = vol[..., k].astype(F)
            win = xk > best
            best = np.where(win, xk, best)
            bits = np.where(win, vol[..., k].view(np.uint16), bits)
            idx = np.where(win, np.uint8(k), idx)
    ids[seen] = idx[seen]
    scores.view(np.uint16)[seen] = bits[seen]
    return int(seen.sum())


def _expf(x):
    """fp32 exp as a correctly rounded float64 exp: the device's expf is within 1 ulp of it, which is why the softmax test
    holds probabilities to a tolerance and only maxima / arg maxima to bits."""
    return np.exp(x.astype(np.float64)).astype(F)


def softmax(logits):
    """ojf_seg_softmax of f32 [npix, C] in the kernel's operation order: m = the first maximum, s = the sum of exp(l_j - m)
    in class order from 0, p_c = exp(l_c - m) / s; a row that holds a NaN or a +Inf, or only -Inf, is NaN in every class.
    Returns (probs f32 [npix, C], bad rows)."""
    l = np.asarray(logits, F)
    with np.errstate(all='ignore'):
        m = l[:, 0].copy()
        bad = np.isnan(m)
        for c in range(1, l.shape[1]):
            xc = l[:, c]
            bad |= np.isnan(xc)
            m = np.where(xc > m, xc, m)
        bad |= np.isinf(m)
        s = np.zeros(l.shape[0], F)
        for c in range(l.shape[1]):
            s = s + _expf(l[:, c] - m)
        out = np.stack([_expf(l[:, c] - m) / s for c in range(l.shape[1])], axis=1)
    out[bad] = np.nan
    return out, bad


# ---- cases ---------------------------------------------------------------------------------------------------------------
def start_volume(shape, C, rng, max_weight=MAX_WEIGHT):
    """A seeded non-empty label volume: W 0..5, 10 % at max_weight, a normalised distribution where W > 0, an all-zero record
    where W == 0, and PAD_BITS in every padding channel."""
    shape = tuple(shape)
    S = record_size(C)
    w = rng.integers(0, 6, shape).astype(np.float16)
    w[rng.random(shape) < 0.10] = max_weight
    p = rng.random(shape + (C,)) ** 4
    p /= p.sum(axis=-1, keepdims=True)
    vol = np.zeros(shape + (S,), np.float16)
    vol[..., :C] = p.astype(np.float16)
    vol[..., C] = w
    vol[w == 0] = 0
    vol.view(np.uint16)[..., C + 1:] = PAD_BITS
    return vol


def tiny_label_case(shape, pose, C=30, seed=0, prob_stride=None):
    """projective_ref.tiny_case (its label image holds 1..29) plus: label pixels >= C planted over 20 % of the image (for
    C < 256), a seeded f32 [h,w,prob_stride] probability image (a normalised distribution per pixel; 3 % of the entries NaN, 3 %
    negative, 3 % > 1; NaN in the floats behind the classes, which the kernel must ignore), a seeded start volume, band =
    2.5 RES and max_weight = 8."""
    c = tiny_case(shape, pose, seed)
    rng = np.random.default_rng([seed, 91, SHAPES.index(tuple(shape)), POSES.index(pose), C])
    h, w = c['depth'].shape
    stride = C if prob_stride is None else prob_stride
    labels = rng.integers(0, C, (h, w)).astype(np.uint8)
    if C < 256:
        over = rng.random((h, w)) < 0.20
        labels[over] = rng.integers(C, 256, (h, w)).astype(np.uint8)[over]
    p = rng.random((h, w, C)) ** 4
    p /= p.sum(axis=-1, keepdims=True)
    probs = np.full((h, w, stride), np.nan, F)
    probs[..., :C] = p
    u = rng.random((h, w, C))
    probs[..., :C][u < 0.03] = np.nan
    probs[..., :C][(u >= 0.03) & (u < 0.06)] = -0.25
    probs[..., :C][(u >= 0.06) & (u < 0.09)] = 1.5
    c['labels'] = labels
    c['probs'] = probs
    c['n_classes'] = C
    c['volume'] = start_volume(shape, C, rng)
    c['band'] = BAND
    c['label_max_weight'] = MAX_WEIGHT
    return c


# ---- the noisy-label experiment: one-slot rule against the per-voxel vote -------------------------------------
NOISE_H, NOISE_W, NOISE_GRID, NOISE_FRAMES, NOISE_CLASSES, NOISE_BAND = 48, 64, 64, 20, 16, 0.1


def noisy_frames(q=0.2, seed=7):
    """(stream, frames): frames 0..19 of synthetic.SyntheticStream(48, 64, 64, 20, n_classes=16), each with 'labels_clean'
    (its semantic_gt as u8), 'labels_noisy' (every pixel replaced with probability q by a uniform class of 1..15) and
    'label_scores' (the frame's own semantic_scores: a wrong pixel is as confident as a right one)."""
    from online_joint_depthfusion_and_semantic_amd import synthetic
    st = synthetic.SyntheticStream(NOISE_H, NOISE_W, NOISE_GRID, NOISE_FRAMES, n_classes=NOISE_CLASSES)
    rng = np.random.default_rng(seed)
    frames = []
    for i in range(NOISE_FRAMES):
        f = st.frame(i)
        clean = np.asarray(f['semantic_gt']).astype(np.uint8)
        noisy = clean.copy()
        flip = rng.random(clean.shape) < q
        noisy[flip] = rng.integers(1, NOISE_CLASSES, clean.shape).astype(np.uint8)[flip]
        f['labels_clean'], f['labels_noisy'] = clean, noisy
        f['label_scores'] = np.asarray(f['semantic_scores'], F)
        frames.append(f)
    return st, frames


def agreement(ids_noisy, ids_clean, where):
    return float((ids_noisy[where] == ids_clean[where]).mean())
