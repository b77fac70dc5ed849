"""numpy restatement of the projective TSDF fusion definition in csrc/ojf_projective.hip (ojf_fuse_projective), vectorised
over the volume: every fp32 operation is one numpy ufunc on float32 arrays (rounded on its own), the host part is written
out in f64 sums (no ``@``).  Also the tiny-shape cases the GPU parity test runs, so that a CPU test can show they are not
vacuous."""
import numpy as np

F = np.float32


def view_constants(K, E, origin, res):
    """(A f32[3,3] with A[a][m], b f32[3], fx, fy, cx, cy) of one view; refuses a non-pinhole K."""
    K = np.asarray(K, np.float64).reshape(9)
    E = np.asarray(E, np.float64).reshape(-1)[:12]
    origin = np.asarray(origin, np.float64).reshape(3)
    res = np.float64(res)
    if not (K[1] == 0 and K[3] == 0 and K[6] == 0 and K[7] == 0 and K[8] == 1):
        raise ValueError('pinhole K expected')
    g = [(origin[m] + np.float64(0.5) * res) - E[4 * m + 3] for m in range(3)]
    A = np.empty((3, 3), F)
    b = np.empty(3, F)
    for a in range(3):
        for m in range(3):
            A[a, m] = F(E[4 * m + a] * res)
        b[a] = F((E[a] * g[0] + E[4 + a] * g[1]) + E[8 + a] * g[2])
    return A, b, F(K[0]), F(K[4]), F(K[2]), F(K[5])


def fuse(tsdf, weights, origin, res, depth, K, E, mask=None, ids=None, scores=None, labels=None, label_scores=None, *,
         trunc, max_weight=128.0, near=0.0, carve=False):
    """In place on fp16 ``tsdf`` / ``weights`` [X,Y,Z] (and u8 ``ids`` / fp16 ``scores``) for the views of ``depth``
    f32 [n,h,w]; K [n,3,3] or [3,3], E [n,3,4] (or 4x4).  Returns the number of voxel updates (step 5) per view."""
    depth = np.asarray(depth, F)
    if depth.ndim == 2:
        depth = depth[None]
    n, h, w = depth.shape
    K = np.broadcast_to(np.asarray(K, np.float64).reshape(-1, 3, 3), (n, 3, 3))
    E = np.asarray(E, np.float64)
    E = np.broadcast_to(E.reshape((-1,) + E.shape[-2:]), (n,) + E.shape[-2:])
    mask = None if mask is None else np.asarray(mask).reshape(n, h, w)
    sem = labels is not None
    if sem:
        labels = np.asarray(labels, np.uint8).reshape(n, h, w)
        label_scores = None if label_scores is None else np.asarray(label_scores, F).reshape(n, h, w)
    X, Y, Z = tsdf.shape
    x = np.arange(X, dtype=F)[:, None, None]
    y = np.arange(Y, dtype=F)[None, :, None]
    z = np.arange(Z, dtype=F)[None, None, :]
    trunc, max_weight, near = F(trunc), F(max_weight), F(near)
    counts = []
    with np.errstate(all='ignore'):
        for v in range(n):
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
            s = d - zc
            ok &= ~(s < -trunc)
            band = s <= trunc
            if not carve:
                ok &= band
            band &= ok
            o = np.minimum(s, trunc)
            w0 = weights.astype(F)
            t0 = tsdf.astype(F)
            w1 = w0 + F(1)
            t1 = (w0 * t0 + o) / w1
            tsdf[ok] = t1.astype(np.float16)[ok]
            weights[ok] = np.minimum(w1, max_weight).astype(np.float16)[ok]
            counts.append(int(ok.sum()))
            if sem:
                sc = (label_scores[v][ri, ci] if label_scores is not None else np.ones(ok.shape, F)).astype(np.float16)
                win = band & (sc.astype(F) > scores.astype(F))
                ids[win] = labels[v][ri, ci][win]
                scores[win] = sc[win]
    return counts


# ---- the tiny-shape cases of the GPU parity test ------------------------------------------------------------------------
SHAPES = ((5, 7, 19), (16, 16, 16), (33, 20, 70))
POSES = ('outside_z', 'outside_x_rolled', 'inside', 'oblique', 'looking_away')
RES = 0.04
IMG_H, IMG_W = 12, 16
MAX_WEIGHT = 8.0


def _look_at(eye, target, roll=0.0):
    """Camera-to-world [3,4] f64: z forward to the target, x right, y down, rolled about z."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = target - eye
    fwd /= np.linalg.norm(fwd)
    up = np.array([0.0, 0.0, 1.0]) if abs(fwd[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    cr, sr = np.cos(roll), np.sin(roll)
    right, down = cr * right + sr * down, -sr * right + cr * down
    return np.concatenate([np.stack([right, down, fwd], axis=1), eye[:, None]], axis=1)


def tiny_case(shape, pose, seed=0):
    """Inputs of one parity case: volume centred on the origin at RES, a 12x16 image (f = 0.6 w, cx = w/2 - 0.5), depth =
    distance to the centre + 1.5 RES of Gaussian noise with 5 % zeros, 2 % NaN, 2 % +inf, 2 % -1, a mask that drops 10 %,
    label / score images, and seeded non-empty start volumes (weights 0..5, 10 % at max_weight, weight 0 -> init)."""
    rng = np.random.default_rng([seed, SHAPES.index(tuple(shape)), POSES.index(pose)])
    shape = tuple(shape)
    ext = np.array(shape, np.float64) * RES
    origin = -0.5 * ext
    long_, short = ext.max(), ext.min()
    zero = np.zeros(3)
    if pose == 'outside_z':
        E = _look_at([0.0, 0.0, 1.2 * long_], zero)
    elif pose == 'outside_x_rolled':
        E = _look_at([-1.2 * long_, 0.0, 0.0], zero, roll=np.pi / 2)
    elif pose == 'inside':
        E = _look_at([0.0, 0.0, 0.2 * short], zero)
    elif pose == 'oblique':
        E = _look_at(np.array([1.0, 1.0, 1.0]) * 0.8 * long_, zero)
    elif pose == 'looking_away':
        E = _look_at([0.0, 0.0, 1.2 * long_], [0.0, 0.0, 3.0 * long_])
    else:
        raise ValueError(pose)
    h, w = IMG_H, IMG_W
    f = 0.6 * w
    K = np.array([[f, 0.0, w / 2 - 0.5], [0.0, f, h / 2 - 0.5], [0.0, 0.0, 1.0]])
    dist = np.linalg.norm(E[:, 3])
    depth = (dist + rng.normal(0.0, 1.5 * RES, (h, w))).astype(F)
    u = rng.random((h, w))
    depth[u < 0.05] = 0.0
    depth[(u >= 0.05) & (u < 0.07)] = np.nan
    depth[(u >= 0.07) & (u < 0.09)] = np.inf
    depth[(u >= 0.09) & (u < 0.11)] = -1.0
    mask = rng.random((h, w)) >= 0.10
    labels = rng.integers(1, 30, (h, w)).astype(np.uint8)
    label_scores = rng.uniform(0.2, 1.0, (h, w)).astype(F)
    init = 0.1
    wgt = rng.integers(0, 6, shape).astype(np.float16)
    wgt[rng.random(shape) < 0.10] = MAX_WEIGHT
    tsdf = rng.uniform(-0.1, 0.1, shape).astype(np.float16)
    tsdf[wgt == 0] = init
    ids = rng.integers(0, 30, shape).astype(np.uint8)
    scores = rng.uniform(0.0, 0.9, shape).astype(np.float16)
    return dict(shape=shape, origin=origin, res=RES, K=K, E=E, depth=depth, mask=mask, labels=labels,
                label_scores=label_scores, tsdf=tsdf, weights=wgt, ids=ids, scores=scores, trunc=2.5 * RES,
                max_weight=MAX_WEIGHT)
