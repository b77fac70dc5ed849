"""numpy restatement of the colour volume's definition in csrc/ojf_color.hip (ojf_fuse_color, ojf_color_sample,
ojf_color_render): every fp32 operation is one numpy ufunc on float32 arrays (rounded on its own), the host part comes from
projective_ref.view_constants / render_ref.cameras.  Also the cases the CPU and GPU tests share.  Test helper, not a test."""
import numpy as np

import projective_ref as pref
import render_ref
from projective_ref import view_constants, tiny_case, SHAPES, POSES, RES  # noqa: F401  (re-exported for the tests)

F = np.float32
MAX_WEIGHT = 8.0
BAND = 2.5 * RES


def _views(depth, K, E):
    depth = np.asarray(depth, F)
    if depth.ndim == 2:
        depth = depth[None]
    n = depth.shape[0]
    K = np.broadcast_to(np.asarray(K, np.float64).reshape(-1, 3, 3), (n, 3, 3))
    E = np.asarray(E, np.float64)
    E = np.broadcast_to(E.reshape((-1,) + E.shape[-2:]), (n,) + E.shape[-2:])
    return depth, K, E


def fuse(colors, origin, res, image, depth, K, E, mask=None, *, band, max_weight=64.0, near=0.0):
    """In place on fp16 ``colors`` [X,Y,Z,4] for the views of ``image`` u8 [n,h,w,3|4] and ``depth`` f32 [n,h,w] (a single
    view may come without the leading axis); K [n,3,3] or [3,3], E [n,3,4] (or 4x4).  Returns the number of voxel updates
    (step 3) per view."""
    depth, K, E = _views(depth, K, E)
    n, h, w = depth.shape
    image = np.asarray(image, np.uint8).reshape(n, h, w, -1)
    mask = None if mask is None else np.asarray(mask).reshape(n, h, w)
    X, Y, Z = colors.shape[:3]
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
            # 3., 4.
            w0 = colors[..., 3].astype(F)
            w1 = w0 + F(1)
            for k in range(3):
                ck = (w0 * colors[..., k].astype(F) + image[v][ri, ci, k].astype(F)) / w1
                colors[..., k][ok] = ck.astype(np.float16)[ok]
            colors[..., 3][ok] = np.minimum(w1, max_weight).astype(np.float16)[ok]
            counts.append(int(ok.sum()))
    return counts


def sample(colors, g):
    """S(g): u8 [M,4] for g f32 [M,3] in voxel index coordinates."""
    colors = np.asarray(colors, np.float16)
    g = np.asarray(g, F).reshape(-1, 3)
    N = colors.shape[:3]
    vol = colors.reshape(-1, 4).astype(F)
    with np.errstate(all='ignore'):
        ok = np.ones(g.shape[0], bool)
        for a in range(3):
            ok &= (g[:, a] >= F(-1)) & (g[:, a] <= F(N[a]))  # (a NaN or inf fails)
        gs = np.where(ok[:, None], g, F(0))
        fl = np.floor(gs)
        f = gs - fl
        i0 = fl.astype(np.int64)
        acc = np.zeros((g.shape[0], 3), F)
        ws = np.zeros(g.shape[0], F)
        one = F(1)
        for c in range(8):
            bits = ((c >> 2) & 1, (c >> 1) & 1, c & 1)
            idx = [i0[:, a] + bits[a] for a in range(3)]
            inside = ok.copy()
            for a in range(3):
                inside &= (idx[a] >= 0) & (idx[a] < N[a])
            flat = np.where(inside, (idx[0] * N[1] + idx[1]) * N[2] + idx[2], 0)
            vox = vol[flat]
            counted = inside & (vox[:, 3] > 0)
            wa = [f[:, a] if bits[a] else one - f[:, a] for a in range(3)]
            tw = (wa[0] * wa[1]) * wa[2]
            for k in range(3):
                acc[:, k] = np.where(counted, acc[:, k] + tw * vox[:, k], acc[:, k])
            ws = np.where(counted, ws + tw, ws)
        have = ws > 0
        out = np.zeros((g.shape[0], 4), np.uint8)
        for k in range(3):
            m = np.floor(np.fmin(np.fmax(acc[:, k] / ws, F(0)), F(255)) + F(0.5))
            out[:, k] = np.where(have, m, 0).astype(np.uint8)
        out[:, 3] = np.where(have, 255, 0)
    return out


def render_color(colors, origin, resolution, intrinsics, extrinsics, depth):
    """u8 [n,h,w,4] as ojf_color_render defines it, for depth f32 [n,h,w]."""
    depth = np.asarray(depth, F)
    n, h, w = depth.shape
    Ki, E, O = render_ref.cameras(intrinsics, extrinsics, origin, resolution)
    resf = F(resolution)
    rr, cc = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    rf, cf = rr.reshape(-1).astype(F), cc.reshape(-1).astype(F)
    out = np.zeros((n, h * w, 4), np.uint8)
    with np.errstate(all='ignore'):
        for v in range(n):
            K, R, o = Ki[v], E[v].reshape(3, 4)[:, :3], O[v]
            dc = [(K[3 * i] * cf + K[3 * i + 1] * rf) + K[3 * i + 2] for i in range(3)]
            t = depth[v].reshape(-1)
            g = np.empty((h * w, 3), F)
            for i in range(3):
                d = (R[i, 0] * dc[0] + R[i, 1] * dc[1]) + R[i, 2] * dc[2]
                dv = d / resf
                g[:, i] = (o[i] + t * dv) - F(0.5)
            valid = np.isfinite(t) & (t > 0)
            out[v] = np.where(valid[:, None], sample(colors, np.where(valid[:, None], g, F(0))), 0)
    return out.reshape(n, h, w, 4)


# ---- cases ---------------------------------------------------------------------------------------------------------------
def start_volume(shape, rng, max_weight=MAX_WEIGHT):
    """A seeded non-empty colour volume: W 0..5, 10 % at max_weight, colour 0 where W == 0."""
    shape = tuple(shape)
    w = rng.integers(0, 6, shape).astype(np.float16)
    w[rng.random(shape) < 0.10] = max_weight
    vol = np.empty(shape + (4,), np.float16)
    vol[..., :3] = rng.uniform(0.0, 255.0, shape + (3,)).astype(np.float16)
    vol[..., 3] = w
    vol[w == 0] = 0
    return vol


def tiny_color_case(shape, pose, seed=0):
    """projective_ref.tiny_case plus a seeded u8 [h,w,4] image (the 4th byte is noise the kernel must ignore), a seeded
    start colour volume and band = 2.5 RES, max_weight = 8."""
    c = tiny_case(shape, pose, seed)
    rng = np.random.default_rng([seed, 77, SHAPES.index(tuple(shape)), POSES.index(pose)])
    c['image'] = rng.integers(0, 256, c['depth'].shape + (4,)).astype(np.uint8)
    c['colors'] = start_volume(shape, rng)
    c['band'] = BAND
    c['color_max_weight'] = MAX_WEIGHT
    return c


def sample_case(shape, seed=0, m=4096):
    """(colors with half its W at 0, points f32 [M,3]): ``m`` points uniform in [-2, N+1] plus points on integer
    coordinates, at exactly -1 and N, NaN and +-inf."""
    shape = tuple(shape)
    rng = np.random.default_rng([seed, 78, SHAPES.index(shape)])
    vol = start_volume(shape, rng)
    vol[..., 3] = np.where(vol[..., 3] == 0, 1, vol[..., 3])
    vol[..., :3] = rng.uniform(0.0, 255.0, shape + (3,)).astype(np.float16)
    vol[rng.random(shape) < 0.5] = 0
    N = np.array(shape, np.float64)
    pts = rng.uniform(-2.0, N + 1.0, (m, 3))
    ints = np.floor(rng.uniform(-1.0, N + 1.0, (256, 3)))
    edge = rng.uniform(0.0, N, (64, 3))
    for i in range(64):
        edge[i, i % 3] = -1.0 if (i // 3) % 2 else N[i % 3]
    bad = rng.uniform(0.0, N, (12, 3))
    for i, v in enumerate((np.nan, np.inf, -np.inf, np.nan)):
        bad[3 * i + np.arange(3), np.arange(3)] = v
    return vol, np.concatenate([pts, ints, edge, bad]).astype(F)


def analytic_color(p):
    """A smooth colour of world points p [...,3] (m): every channel one sinusoid inside 30..225 whose wavelength (1.6, 2.0
    and 1.28 m) is at least 16 voxels of the 64^3 room grid (0.08 m)."""
    p = np.asarray(p, np.float64)
    dirs = np.array([[1.0, 0.5, 0.25], [-0.5, 1.0, 0.5], [0.25, -0.5, 1.0]])
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    lam, phase = np.array([1.6, 2.0, 1.28]), np.array([0.0, 1.0, 2.0])
    return 127.5 + 97.5 * np.sin(2.0 * np.pi * (p @ dirs.T) / lam + phase)


def room_frames(stream, frames):
    """Frames 0..frames-1 of a synthetic.SyntheticStream with 'image' replaced by the u8 [h,w,3] analytic colour of the
    world-space surface point eye + depth_gt·ray of every pixel."""
    out = []
    for i in range(frames):
        f = stream.frame(i)
        K, E = f['intrinsics'], f['extrinsics']
        u, v = np.meshgrid(np.arange(stream.w, dtype=np.float64), np.arange(stream.h, dtype=np.float64))
        dc = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], axis=-1)
        pw = E[:, 3] + f['depth_gt'].astype(np.float64)[..., None] * (dc @ E[:, :3].T)
        f['image'] = np.round(analytic_color(pw)).astype(np.uint8)
        out.append(f)
    return out


def look_at(eye, target):
    """Camera-to-world [3,4] f64: z forward to the target, x right, y down."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    up = np.array([0.0, 0.0, 1.0]) if abs(fwd[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    return np.concatenate([np.stack([right, np.cross(fwd, right), fwd], axis=1), eye[:, None]], axis=1)


def sphere_case(n_views=4, h=24, w=32, grid=32, radius_voxels=10.0, seed=0):
    """A sphere of radius 10 voxels in the middle of a 32^3 volume (res 0.05 m, centred on the origin) seen by ``n_views``
    cameras on a ring around it: analytic z-depth (0 where the ray misses), seeded u8 images."""
    res = 0.05
    origin = np.full(3, -0.5 * grid * res)
    rad = radius_voxels * res
    K = np.array([[0.9 * w, 0.0, w / 2 - 0.5], [0.0, 0.9 * w, h / 2 - 0.5], [0.0, 0.0, 1.0]])
    rng = np.random.default_rng([seed, 79])
    E, depth = [], []
    for i in range(n_views):
        a = 2.0 * np.pi * i / n_views + 0.3
        e = look_at([1.6 * np.cos(a), 1.6 * np.sin(a), 0.4 * np.sin(2.0 * a)], np.zeros(3))
        u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
        dw = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], axis=-1) @ e[:, :3].T
        qa, qb, qc = (dw * dw).sum(-1), 2.0 * (dw @ e[:, 3]), e[:, 3] @ e[:, 3] - rad * rad
        disc = qb * qb - 4.0 * qa * qc
        t = np.where(disc > 0, (-qb - np.sqrt(np.maximum(disc, 0.0))) / (2.0 * qa), 0.0)
        E.append(e)
        depth.append(t.astype(F))
    image = rng.integers(0, 256, (n_views, h, w, 3)).astype(np.uint8)
    return dict(shape=(grid,) * 3, origin=origin, res=res, K=K, E=np.stack(E), depth=np.stack(depth), image=image,
                trunc=3 * res, band=3 * res)
