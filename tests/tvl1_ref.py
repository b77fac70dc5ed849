"""numpy restatement of the TV-L1 fusion definition in csrc/ojf_tvl1.hip (ojf_fuse_depth_hist, ojf_tvl1_solve, ojf_tvl1_write),
vectorised over the volume: every fp32 operation is one numpy ufunc on float32 arrays (rounded on its own), the host part of
the projection comes from projective_ref.view_constants.  Also the cases the CPU and GPU tests share.  Test helper, not a
test."""
import numpy as np

import projective_ref as pref
from projective_ref import view_constants, tiny_case, RES  # noqa: F401  (re-exported for the tests)

F = np.float32
MAX_BINS, MAX_VIEWS = 15, 32
PAD_BITS = 0x7e00  # what the padding channels of the test volumes hold (a NaN: arithmetic on it would show)
BRICK = (4, 8, 32)  # csrc/ojf_tvl1.hip kTvX, kTvY, kTvZ
GROUP = 4           # the z voxels of one lane; Zp = Z rounded up to it
STEP = F(0.28867513)  # tvl1.default_step(): the largest fp32 whose square is <= 1/12


def record_size(B):
    return 8 * ((B + 8) // 8)


def centres(B):
    """l_b = float(2b) / float(B-1) - 1, fp32."""
    return (np.arange(0, 2 * B, 2).astype(F) / F(B - 1) - F(1)).astype(F)


def new_volume(shape, B, pad=True):
    vol = np.zeros(tuple(shape) + (record_size(B),), np.float16)
    if pad:
        vol.view(np.uint16)[..., B + 1:] = PAD_BITS
    return vol


# ---- fusion ----------------------------------------------------------------------------------------------------------------
def fuse(vol, B, origin, res, depth, K, E, mask=None, *, trunc, max_weight=128.0, near=0.0, carve=True):
    """In place on fp16 ``vol`` [X,Y,Z,S] for the views of ``depth`` f32 [n,h,w] (or [h,w]); K [n,3,3] or [3,3], E [n,3,4] (or
    4x4).  Channels behind B are never read or written.  Returns the number of voting voxels per view."""
    assert vol.shape[3] == record_size(B) and 2 <= B <= MAX_BINS
    depth = np.asarray(depth, F)
    if depth.ndim == 2:
        depth = depth[None]
    n, h, w = depth.shape
    K = np.broadcast_to(np.asarray(K, np.float64).reshape(-1, 3, 3), (n, 3, 3))
    E = np.asarray(E, np.float64)
    E = np.broadcast_to(E.reshape((-1,) + E.shape[-2:]), (n,) + E.shape[-2:])
    mask = None if mask is None else np.asarray(mask).reshape(n, h, w)
    X, Y, Z = vol.shape[:3]
    x = np.arange(X, dtype=F)[:, None, None]
    y = np.arange(Y, dtype=F)[None, :, None]
    z = np.arange(Z, dtype=F)[None, None, :]
    trunc, max_weight, near = F(trunc), F(max_weight), F(near)
    hb = F(B - 1) * F(0.5)
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
            s = d - zc
            # 2. who votes
            ok &= s >= -trunc
            if not carve:
                ok &= s <= trunc
            # 3. the vote
            t = np.fmin(s, trunc) / trunc
            g = (t + F(1)) * hb
            b0 = np.minimum(np.floor(np.where(ok, g, 0)).astype(np.int64), B - 2)
            f = g - b0.astype(F)
            f0 = F(1) - f
            # 4. the running mean
            w0 = vol[..., B].astype(F)
            w1 = w0 + F(1)
            for k in range(B):
                vote = np.where(b0 == k, f0, np.where(b0 + 1 == k, f, F(0))).astype(F)
                hk = (w0 * vol[..., k].astype(F) + vote) / w1
                vol[..., k][ok] = hk.astype(np.float16)[ok]
            vol[..., B][ok] = np.fmin(w1, max_weight).astype(np.float16)[ok]
            counts.append(int(ok.sum()))
    return counts


# ---- the solver ------------------------------------------------------------------------------------------------------------
def observed(vol, B):
    with np.errstate(invalid='ignore'):
        return vol[..., B].astype(F) > 0


def edges(obs):
    """bool [3,X,Y,Z]: edge a of a voxel counts when it and its upper neighbour along a are observed and inside the box."""
    e = np.zeros((3,) + obs.shape, bool)
    e[0, :-1] = obs[:-1] & obs[1:]
    e[1, :, :-1] = obs[:, :-1] & obs[:, 1:]
    e[2, :, :, :-1] = obs[:, :, :-1] & obs[:, :, 1:]
    return e


def _canon_clamp(x):
    return (np.fmin(np.fmax(x, F(-1)), F(1)) + F(0)).astype(F)


def prefix_weights(vol, B):
    """(P f32 [B+1,X,Y,Z], T): P_0 = 0, P_(i+1) = P_i + h_i; T = P_B.  W_i = (T - P_i) - P_i."""
    P = [np.zeros(vol.shape[:3], F)]
    for i in range(B):
        P.append(P[-1] + vol[..., i].astype(F))
    return P, P[B]


def start_value(vol, B):
    l = centres(B)
    N = np.zeros(vol.shape[:3], F)
    T = np.zeros(vol.shape[:3], F)
    with np.errstate(all='ignore'):
        for b in range(B):
            h = vol[..., b].astype(F)
            N = N + h * l[b]
            T = T + h
        return _canon_clamp(N / T)


def prox(vol, B, v, tl):
    """The primal step of every voxel from ``v`` f32 [X,Y,Z]: canon(clamp(max_i min(c_i, l_i))), and the unclamped m."""
    l = centres(B)
    P, T = prefix_weights(vol, B)
    tl = F(tl)
    with np.errstate(all='ignore'):
        m = v + tl * ((T - P[B]) - P[B])
        for i in range(B):
            m = np.fmax(m, np.fmin(v + tl * ((T - P[i]) - P[i]), l[i]))
        return _canon_clamp(m), m


class State:
    """The solver's state on the host: u (the caller's; only observed voxels are ever written), ub and p."""

    def __init__(self, u):
        self.u = u
        self.ub = np.zeros(u.shape, F)
        self.p = np.zeros((3,) + u.shape, F)
        self.obs = np.zeros(u.shape, bool)


def setup(state, vol, B, restart):
    """The set-up pass: restart (mode 1) or refresh (mode 2: the histogram changed)."""
    obs = observed(vol, B)
    fresh = obs if restart else obs & ~state.obs
    u0 = start_value(vol, B)
    if restart:
        state.p[:] = 0
        state.ub[:] = 0
    state.u[fresh] = u0[fresh]
    state.ub[fresh] = u0[fresh]
    state.obs = obs


def _shift_up(a, axis):
    """a at x + e_axis (0 past the box)."""
    out = np.zeros_like(a)
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    src[axis], dst[axis] = slice(1, None), slice(0, -1)
    out[tuple(dst)] = a[tuple(src)]
    return out


def _shift_down(a, axis):
    """a at x - e_axis (0 past the box)."""
    out = np.zeros_like(a)
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    src[axis], dst[axis] = slice(0, -1), slice(1, None)
    out[tuple(dst)] = a[tuple(src)]
    return out


def iterate(state, vol, B, lam, tau, sigma):
    """One iteration, in place."""
    tau, sigma = F(tau), F(sigma)
    tl = F(tau * F(lam))
    e = edges(state.obs)
    with np.errstate(all='ignore'):
        q = [np.where(e[a], state.p[a] + sigma * (_shift_up(state.ub, a) - state.ub), F(0)).astype(F) for a in range(3)]
        d = np.fmax(F(1), np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]))
        p = [q[a] / d for a in range(3)]
        div = ((p[0] - _shift_down(p[0], 0)) + (p[1] - _shift_down(p[1], 1))) + (p[2] - _shift_down(p[2], 2))
        v = state.u + tau * div
        un, _ = prox(vol, B, v, tl)
        ubn = F(2) * un - state.u
    for a in range(3):
        state.p[a] = p[a]
    o = state.obs
    state.ub[o] = ubn[o]
    state.u[o] = un[o]


def solve(state, vol, B, lam, iterations, tau=STEP, sigma=STEP, restart=True, changed=False):
    if restart or changed:
        setup(state, vol, B, restart)
    for _ in range(iterations):
        iterate(state, vol, B, lam, tau, sigma)
    return state.u


def write(vol, B, u, trunc, tsdf, weights):
    obs = observed(vol, B)
    tsdf[obs] = (F(trunc) * u).astype(np.float16)[obs]
    weights.view(np.uint16)[obs] = vol[..., B].view(np.uint16)[obs]


def energy(vol, B, u, lam):
    """float64: sum over the counted edges of |grad u| (isotropic, per voxel) + lam · sum h_b |u - l_b| over the observed voxels."""
    obs = observed(vol, B)
    e = edges(obs)
    u = u.astype(np.float64)
    g2 = np.zeros(u.shape)
    for a in range(3):
        g = np.where(e[a], _shift_up(u, a) - u, 0.0)
        g2 += g * g
    l = centres(B).astype(np.float64)
    data = sum(vol[..., b].astype(np.float64) * np.abs(u - l[b]) for b in range(B))
    return float(np.sqrt(g2).sum() + lam * data[obs].sum())


def hist_median(vol, B):
    """The per-voxel histogram median bin centre: the smallest l_i with sum_(b<=i) h_b >= sum_(b>i) h_b (float64)."""
    h = vol[..., :B].astype(np.float64)
    c = np.cumsum(h, axis=-1)
    idx = np.argmax(c >= (c[..., -1:] - c), axis=-1)
    return centres(B)[idx]


# ---- cases -----------------------------------------------------------------------------------------------------------------
# the shapes the issue names, and on every axis one voxel below, at and above the brick extent (BRICK) and, in z, the group
# (GROUP) the kernels use
SHAPES = ((1, 1, 1), (5, 7, 19), (1, 1, 257), (9, 17, 70), (16, 16, 16))
EDGE_SHAPES = tuple((BRICK[0] + dx, 3, 5) for dx in (-1, 0, 1)) + tuple((2, BRICK[1] + dy, 6) for dy in (-1, 0, 1)) \
    + tuple((2, 3, BRICK[2] + dz) for dz in (-1, 0, 1)) + tuple((3, 2, GROUP + dz) for dz in (-1, 0, 1)) \
    + ((2 * BRICK[0] + 1, 2 * BRICK[1] + 1, 2 * BRICK[2] + 1),)
POSES = pref.POSES


def fuse_case(shape, seed=0):
    """Origin, resolution, K, and per pose of projective_ref.POSES a depth map, mask and pose for a box of ``shape`` centred
    on the origin (projective_ref.tiny_case's recipe, for any shape)."""
    shape = tuple(shape)
    rng = np.random.default_rng([seed, 77] + list(shape))
    ext = np.array(shape, np.float64) * RES
    origin = -0.5 * ext
    long_, short = ext.max(), ext.min()
    zero = np.zeros(3)
    poses = [pref._look_at([0.0, 0.0, 1.2 * long_], zero), pref._look_at([-1.2 * long_, 0.0, 0.0], zero, roll=np.pi / 2),
             pref._look_at([0.0, 0.0, 0.2 * short], zero), pref._look_at(np.array([1.0, 1.0, 1.0]) * 0.8 * long_, zero),
             pref._look_at([0.0, 0.0, 1.2 * long_], [0.0, 0.0, 3.0 * long_])]
    h, w = pref.IMG_H, pref.IMG_W
    f = 0.6 * w
    K = np.array([[f, 0.0, w / 2 - 0.5], [0.0, f, h / 2 - 0.5], [0.0, 0.0, 1.0]])
    depths, masks = [], []
    for E in poses:
        dist = np.linalg.norm(E[:, 3])
        depth = (dist + rng.normal(0.0, 1.5 * RES, (h, w))).astype(F)
        u = rng.random((h, w))
        depth[u < 0.05] = 0.0
        depth[(u >= 0.05) & (u < 0.07)] = np.nan
        depth[(u >= 0.07) & (u < 0.09)] = np.inf
        depth[(u >= 0.09) & (u < 0.11)] = -1.0
        depths.append(depth)
        masks.append(rng.random((h, w)) >= 0.10)
    return dict(shape=shape, origin=origin, res=RES, K=K, E=np.stack(poses), depth=np.stack(depths), mask=np.stack(masks),
                trunc=2.5 * RES)


def random_hist(shape, B, rng, pattern='random', max_weight=8.0):
    """A seeded histogram volume: normalised records with a weight where the pattern says "observed", all-zero records
    elsewhere, PAD_BITS in the padding.  Patterns: random (60 % observed), none, all, checker (a 3-D checkerboard: no edge
    counts), sheet (the plane x = X // 2)."""
    shape = tuple(shape)
    X, Y, Z = shape
    i, j, k = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing='ij')
    if pattern == 'random':
        obs = rng.random(shape) < 0.6
    elif pattern == 'none':
        obs = np.zeros(shape, bool)
    elif pattern == 'all':
        obs = np.ones(shape, bool)
    elif pattern == 'checker':
        obs = (i + j + k) % 2 == 0
    elif pattern == 'sheet':
        obs = i == X // 2
    else:
        raise ValueError(pattern)
    vol = new_volume(shape, B)
    # a noisy two-mode histogram per voxel: the modes move smoothly through the box so that neighbours pull on each other
    l = centres(B).astype(np.float64)
    mode = 0.6 * np.sin(0.7 * i + 0.4 * j + 0.3 * k) + rng.normal(0.0, 0.25, shape)
    h = np.exp(-0.5 * ((l[None, None, None, :] - mode[..., None]) / 0.3) ** 2) + 0.3 * rng.random(shape + (B,)) ** 3
    h /= h.sum(axis=-1, keepdims=True)
    vol[..., :B] = h.astype(np.float16)
    w = rng.integers(1, 6, shape).astype(np.float16)
    w[rng.random(shape) < 0.1] = max_weight
    vol[..., B] = w
    vol[~obs, :B + 1] = 0
    return vol
