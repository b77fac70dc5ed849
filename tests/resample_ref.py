"""numpy restatement of the definition in csrc/ojf_resample.hip (ojf_resample_volumes, ojf_resample_records): every fp32
operation is one numpy ufunc on float32 arrays (rounded on its own); M and c are the f64 values resample.compose hands to the
C ABI, rounded once to fp32 here as there.  Also the cases the CPU and GPU tests share.  Test helper, not a test."""
import numpy as np

F = np.float32
H = np.float16
CORNERS = [((c >> 2) & 1, (c >> 1) & 1, c & 1) for c in range(8)]  # bits x, y, z


def index_coordinates(M, c, dst_shape):
    """Step 1: g_a f32 [dX,dY,dZ] for a = 0..2."""
    M = np.asarray(M, np.float64).reshape(3, 3).astype(F)
    c = np.asarray(c, np.float64).reshape(3).astype(F)
    i = np.arange(dst_shape[0], dtype=F)[:, None, None]
    j = np.arange(dst_shape[1], dtype=F)[None, :, None]
    k = np.arange(dst_shape[2], dtype=F)[None, None, :]
    with np.errstate(all='ignore'):
        return [np.broadcast_to(((M[a, 0] * i + M[a, 1] * j) + M[a, 2] * k) + c[a], dst_shape) for a in range(3)]


def corners(M, c, src_shape, dst_shape):
    """Steps 1-3 and the geometric half of 4: per corner (tw f32, in-grid-and-tw>0 bool, flat source voxel i64)."""
    g = index_coordinates(M, c, dst_shape)
    N = src_shape
    with np.errstate(all='ignore'):
        ok = np.ones(dst_shape, bool)
        for a in range(3):
            ok &= (g[a] >= F(-1)) & (g[a] <= F(N[a]))  # (a NaN or inf fails)
        gs = [np.where(ok, g[a], F(0)) for a in range(3)]
        fl = [np.floor(x) for x in gs]
        f = [gs[a] - fl[a] for a in range(3)]
        i0 = [x.astype(np.int64) for x in fl]
        out = []
        one = F(1)
        for bits in CORNERS:
            idx = [i0[a] + bits[a] for a in range(3)]
            w = [f[a] if bits[a] else one - f[a] for a in range(3)]
            tw = (w[0] * w[1]) * w[2]
            inside = ok & (tw > 0)
            for a in range(3):
                inside &= (idx[a] >= 0) & (idx[a] < N[a])
            flat = np.where(inside, (idx[0] * N[1] + idx[1]) * N[2] + idx[2], 0)
            out.append((tw, inside, flat))
    return out


def _gather(cs, values, weight, dst_shape):
    """Steps 4-6 for the channels ``values`` (list of flat f16 source arrays) under the flat f16 source weight (None: every
    in-grid corner is observed): (covered, [half(acc_k/ws)], half(accW/ws) or None, counted masks per corner)."""
    ws = np.zeros(dst_shape, F)
    accW = np.zeros(dst_shape, F)
    acc = [np.full(dst_shape, F(-0.0)) for _ in values]  # (-0: the first term enters unchanged, a copied -0 stays -0)
    counted = []
    with np.errstate(all='ignore'):
        for tw, inside, flat in cs:
            if weight is None:
                cnt = inside
                wv = None
            else:
                wv = weight[flat].astype(F)
                cnt = inside & (wv > 0)
            counted.append(cnt)
            ws = np.where(cnt, ws + tw, ws)
            for n, v in enumerate(values):
                acc[n] = np.where(cnt, acc[n] + tw * v[flat].astype(F), acc[n])
            if wv is not None:
                accW = np.where(cnt, accW + tw * wv, accW)
        covered = ws >= F(0.5)
        means = [(a / ws).astype(H) for a in acc]
        W = None
        if weight is not None:
            W = (accW / ws).astype(H)
            covered = covered & (W.view(np.uint16) != 0)
    return covered, means, W, counted


def _nearest(cs, counted, dst_shape):
    """Step 7: the flat source voxel of the counting corner with the largest tw, the first in corner order on a tie."""
    best = np.zeros(dst_shape, F)
    bestv = np.zeros(dst_shape, np.int64)
    for (tw, _, flat), cnt in zip(cs, counted):
        take = cnt & (tw > best)
        best = np.where(take, tw, best)
        bestv = np.where(take, flat, bestv)
    return bestv


def _merge_mean(w0, old, w1, fresh):
    with np.errstate(all='ignore'):
        m = ((w0 * old.astype(F) + w1 * fresh.astype(F)) / (w0 + w1)).astype(H)
    return np.where(w0 == 0, fresh, m)


def _merge_weight(w0, w1, max_weight):
    with np.errstate(all='ignore'):
        return np.fmin(w0 + w1, F(max_weight)).astype(H)


def _put(dst, mask, new):
    """dst[mask] = new[mask] by bits."""
    d = dst.view(np.uint16) if dst.dtype == H else dst
    n = new.view(np.uint16) if new.dtype == H else new
    d[mask] = n[mask]


def resample_volumes(src, M, c, dst_shape, *, init_value, into=None, max_weight=65504.0):
    """src: dict with 'tsdf' and optionally 'weights', 'ids' + 'scores' (numpy, [X,Y,Z]).  into None: replace mode, returns the
    new dict; else merge mode in place on the arrays of ``into`` (returned)."""
    dst_shape = tuple(dst_shape)
    s_shape = src['tsdf'].shape
    cs = corners(M, c, s_shape, dst_shape)
    wsrc = src['weights'].reshape(-1) if src.get('weights') is not None else None
    covered, (T,), W, counted = _gather(cs, [src['tsdf'].reshape(-1)], wsrc, dst_shape)
    labels = src.get('ids') is not None
    if labels:
        bestv = _nearest(cs, counted, dst_shape)
        ids, scores = src['ids'].reshape(-1)[bestv], src['scores'].reshape(-1)[bestv]
    if into is None:
        out = {'tsdf': np.full(dst_shape, init_value, H)}
        _put(out['tsdf'], covered, T)
        if W is not None:
            out['weights'] = np.zeros(dst_shape, H)
            _put(out['weights'], covered, W)
        if labels:
            out['ids'], out['scores'] = np.zeros(dst_shape, np.uint8), np.zeros(dst_shape, H)
            _put(out['ids'], covered, ids)
            _put(out['scores'], covered, scores)
        return out
    assert W is not None, 'a merge needs the weight volumes'
    w0, w1 = into['weights'].astype(F), W.astype(F)
    _put(into['tsdf'], covered, _merge_mean(w0, into['tsdf'], w1, T))
    _put(into['weights'], covered, _merge_weight(w0, w1, max_weight))
    if labels:
        with np.errstate(all='ignore'):
            beats = covered & (scores.astype(F) > into['scores'].astype(F))
        _put(into['ids'], beats, ids)
        _put(into['scores'], beats, scores)
    return into


def resample_records(src, Cw, M, c, dst_shape, *, into=None, max_weight=64.0):
    """src f16 [X,Y,Z,S] with the weight in channel Cw.  into None: replace mode - returns a zeroed [dX,dY,dZ,S] volume with
    channels 0..Cw written (the caller's padding, if it wants one, goes on top); else merge mode in place on ``into``."""
    dst_shape = tuple(dst_shape)
    S = src.shape[3]
    flat = src.reshape(-1, S)
    cs = corners(M, c, src.shape[:3], dst_shape)
    covered, means, W, _ = _gather(cs, [flat[:, k] for k in range(Cw)], flat[:, Cw], dst_shape)
    if into is None:
        out = np.zeros(dst_shape + (S,), H)
        for k in range(Cw):
            _put(out[..., k], covered, means[k])
        _put(out[..., Cw], covered, W)
        return out
    w0, w1 = into[..., Cw].astype(F), W.astype(F)
    for k in range(Cw):
        _put(into[..., k], covered, _merge_mean(w0, into[..., k], w1, means[k]))
    _put(into[..., Cw], covered, _merge_weight(w0, w1, max_weight))
    return into


# ---- the per-voxel combine: merge == combine(dst, replace into scratch) ------------------------------------------------------
def combine_volumes(dst, scratch, max_weight=65504.0):
    """In place on ``dst``: the merge rule with the replace-mode result ``scratch`` as (T', W', id', score'); a scratch voxel is
    covered iff the bits of its weight are not +0."""
    covered = scratch['weights'].view(np.uint16) != 0
    w0, w1 = dst['weights'].astype(F), scratch['weights'].astype(F)
    _put(dst['tsdf'], covered, _merge_mean(w0, dst['tsdf'], w1, scratch['tsdf']))
    _put(dst['weights'], covered, _merge_weight(w0, w1, max_weight))
    if dst.get('ids') is not None:
        with np.errstate(all='ignore'):
            beats = covered & (scratch['scores'].astype(F) > dst['scores'].astype(F))
        _put(dst['ids'], beats, scratch['ids'])
        _put(dst['scores'], beats, scratch['scores'])
    return dst


def combine_records(dst, scratch, Cw, max_weight=64.0):
    covered = scratch[..., Cw].view(np.uint16) != 0
    w0, w1 = dst[..., Cw].astype(F), scratch[..., Cw].astype(F)
    for k in range(Cw):
        _put(dst[..., k], covered, _merge_mean(w0, dst[..., k], w1, scratch[..., k]))
    _put(dst[..., Cw], covered, _merge_weight(w0, w1, max_weight))
    return dst


# ---- cases -------------------------------------------------------------------------------------------------------------------
INIT = 0.1
PAD_BITS = 0x7e00  # a NaN in the padding of a record: read into a mean it would show


def random_scene(shape, seed=0, unobserved=1.0 / 3.0, labels=True, weights=True):
    """Random fp16 values (2 % of the TSDF -0), about a third of the voxels unobserved (weight 0, with a TSDF that must not
    leak), random ids / scores."""
    shape = tuple(shape)
    rng = np.random.default_rng([seed, 151] + list(shape))
    s = {'tsdf': rng.uniform(-0.1, 0.1, shape).astype(H)}
    s['tsdf'][rng.random(shape) < 0.02] = H(-0.0)  # (a copy keeps the sign of a zero)
    if weights:
        w = rng.uniform(0.5, 40.0, shape).astype(H)
        w[rng.random(shape) < unobserved] = 0
        s['weights'] = w
    if labels:
        s['ids'] = rng.integers(0, 40, shape).astype(np.uint8)
        s['scores'] = rng.uniform(0.0, 1.0, shape).astype(H)
    return s


def random_records(shape, S, Cw, seed=0, unobserved=1.0 / 3.0):
    """A record volume with random channels 0..Cw-1, a weight in Cw (a third 0) and PAD_BITS behind it."""
    shape = tuple(shape)
    rng = np.random.default_rng([seed, 152, S, Cw] + list(shape))
    v = np.empty(shape + (S,), H)
    v[..., :Cw] = rng.uniform(0.0, 255.0 if S == 4 else 1.0, shape + (Cw,)).astype(H)
    v[..., :Cw][rng.random(shape + (Cw,)) < 0.02] = H(-0.0)
    w = rng.integers(1, 9, shape).astype(H)
    w[rng.random(shape) < unobserved] = 0
    v[..., Cw] = w
    v.view(np.uint16)[..., Cw + 1:] = PAD_BITS
    return v


def rotation(axis, angle):
    """Rodrigues: f64 [3,3]."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def about_centre(R, origin, res, shape, shift=(0.0, 0.0, 0.0)):
    """[3,4]: the rotation R about the centre of the box (origin, res, shape), then a translation."""
    centre = np.asarray(origin, np.float64) + 0.5 * res * np.asarray(shape, np.float64)
    return np.concatenate([R, (centre - R @ centre + np.asarray(shift, np.float64))[:, None]], axis=1)


SKEW_AXIS = (1.0, 2.0, 3.0)
