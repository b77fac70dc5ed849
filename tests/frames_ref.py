"""numpy restatement of csrc/ojf_frames.hip (ojf_depth_prepare) - one numpy ufunc on float32 per device operation, in the
order the kernel's header fixes - and the cases the host and GPU tests of frames.py share.  Nothing here needs a device."""
import numpy as np

F = np.float32
TILE_W, TILE_H = 32, 8  # csrc/ojf_frames.hip kTileW, kTileH


def spatial_table(radius, sigma_space):
    """f32 [(2R+1)^2]: exp(-(dr^2 + dc^2) / (2 sigma^2)) in f64, rounded once."""
    out = []
    for dr in range(-radius, radius + 1):
        for dc in range(-radius, radius + 1):
            out.append(np.exp(-np.float64(dr * dr + dc * dc) / (2.0 * np.float64(sigma_space) ** 2)))
    return np.asarray(out, dtype=np.float64).astype(F)


def frame_intrinsics(K, n):
    """f32 [n,4] (1/fx, 1/fy, cx, cy) of [3,3] or [n,3,3] intrinsics."""
    K = np.broadcast_to(np.asarray(K, dtype=np.float64).reshape(-1, 3, 3), (n, 3, 3))
    return np.stack([1.0 / K[:, 0, 0], 1.0 / K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], axis=1).astype(F)


def cos_min_of(max_angle):
    """The kernel's cos_min of a largest accepted angle in degrees (None: 0, the stage is off)."""
    if max_angle is None:
        return 0.0
    return max(float(F(np.cos(np.radians(np.float64(max_angle))))), float(np.finfo(F).tiny))


def _shift(a, dy, dx, fill):
    """b[r, c] = a[r + dy, c + dx], ``fill`` outside the image; a is [n,h,w]."""
    n, h, w = a.shape
    p = max(abs(dy), abs(dx))
    if p == 0:
        return a
    pad = np.full((n, h + 2 * p, w + 2 * p), fill, dtype=a.dtype)
    pad[:, p:p + h, p:p + w] = a
    return pad[:, p + dy:p + dy + h, p + dx:p + dx + w]


def prepare(depth, mask=None, K4=None, radius=2, spatial=None, range0=0.05, range2=0.0, edge_abs=0.0, edge_rel=0.0, near=0.0,
            far=np.inf, cos_min=0.0, normals=False):
    """ojf_depth_prepare on the host with the kernel's arguments: depth f32 [n,h,w], mask [n,h,w] or None, K4 f32 [n,4],
    ``spatial`` the f32 table.  Returns {'depth' f32, 'valid' bool, 'normals' f32 [n,h,w,3] or None}."""
    d = np.ascontiguousarray(depth, dtype=F)
    assert d.ndim == 3
    n, h, w = d.shape
    R = int(radius)
    range0, range2, edge_abs, edge_rel, near, far, cos_min = (F(x) for x in (range0, range2, edge_abs, edge_rel, near, far, cos_min))
    need_normals = normals or cos_min != 0
    with np.errstate(all='ignore'):
        # 1. validity
        v0 = np.isfinite(d) & (near <= d) & (d <= far)
        if mask is not None:
            v0 &= np.asarray(mask).reshape(n, h, w) != 0
        d = np.where(v0, d, F(0))
        # 2. edge rejection
        v1 = v0
        if edge_abs != 0 or edge_rel != 0:
            t = edge_abs + edge_rel * d
            drop = np.zeros_like(v0)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    dn, vn = _shift(d, dy, dx, F(0)), _shift(v0, dy, dx, False)
                    drop |= vn & (np.abs(dn - d) > t)
            v1 = v0 & ~drop
        # 3. bilateral filter
        if R == 0:
            f = np.where(v1, d, F(0))
        else:
            S = np.asarray(spatial, dtype=F).reshape(-1)
            assert S.size == (2 * R + 1) ** 2
            rho = range0 + range2 * (d * d)
            q = F(1) / rho
            num, den = np.zeros_like(d), np.zeros_like(d)
            k = 0
            for dy in range(-R, R + 1):
                for dx in range(-R, R + 1):
                    dn, vn = _shift(d, dy, dx, F(0)), _shift(v1, dy, dx, False)
                    diff = dn - d
                    t = diff * q
                    u = F(1) - t * t
                    take = v1 & vn & (np.abs(t) < F(1))
                    wgt = S[k] * (u * u)
                    num = np.where(take, num + wgt * diff, num)
                    den = np.where(take, den + wgt, den)
                    k += 1
            f = np.where(v1, d + num / np.where(v1, den, F(1)), F(0))
        valid = v1
        nrm = None
        if need_normals:
            # 4. vertex and normal map
            K4 = np.asarray(K4, dtype=F).reshape(n, 4)
            ifx, ify, cx, cy = (K4[:, i][:, None, None] for i in range(4))
            rr = np.arange(h, dtype=F)[None, :, None]
            cc = np.arange(w, dtype=F)[None, None, :]
            V = [((cc - cx) * ifx) * f, ((rr - cy) * ify) * f, f + np.zeros_like(f)]

            def difference(dy, dx):
                vp, vm = _shift(v1, dy, dx, False), _shift(v1, -dy, -dx, False)
                out = []
                for k in range(3):
                    P = np.where(vp, _shift(V[k], dy, dx, F(0)), V[k])
                    M = np.where(vm, _shift(V[k], -dy, -dx, F(0)), V[k])
                    out.append(P - M)
                return out, vp | vm

            a, oka = difference(0, 1)
            b, okb = difference(1, 0)
            m = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
            ln = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
            has = v1 & oka & okb & (ln > 0) & np.isfinite(ln)
            lns = np.where(has, ln, F(1))
            nv = [m[k] / lns for k in range(3)]
            dot = (nv[0] * V[0] + nv[1] * V[1]) + nv[2] * V[2]
            flip = dot > 0
            nv = [np.where(flip, -x, x) for x in nv]
            dot = np.where(flip, -dot, dot)
            # 5. incidence test
            if cos_min != 0:
                cs = (-dot) / np.sqrt((V[0] * V[0] + V[1] * V[1]) + V[2] * V[2])
                valid = v1 & has & (cs >= cos_min)
            if normals:
                keep = valid & has
                nrm = np.stack([np.where(keep, x, F(0)) for x in nv], axis=-1).astype(F)
        # 6. outputs
        out = np.where(valid, f, F(0)).astype(F)
    return {'depth': out, 'valid': valid.copy(), 'normals': nrm}


def prepare_depth(depth, intrinsics=None, mask=None, radius=2, sigma_space=1.5, range0=0.05, range2=0.0, edge_abs=0.0, edge_rel=0.0,
                  near=0.0, far=np.inf, max_angle=None, normals=False):
    """``prepare`` with the arguments of frames.prepare_depth (numpy [h,w] or [n,h,w] in, [n,h,w] out)."""
    d = np.asarray(depth, dtype=F)
    d = d[None] if d.ndim == 2 else d
    n = d.shape[0]
    K4 = None if intrinsics is None else frame_intrinsics(intrinsics, n)
    return prepare(d, None if mask is None else np.asarray(mask).reshape(d.shape), K4, radius, spatial_table(radius, sigma_space) if radius
                   else None, range0, range2, edge_abs, edge_rel, near, far, cos_min_of(max_angle), normals)


# ---- shared cases ------------------------------------------------------------------------------------------------------------
SMALL_SIZES = [(1, 1), (1, 7), (5, 3)]  # smaller than the halo
TILE_SIZES = [(hh, ww) for hh in (TILE_H - 1, TILE_H, TILE_H + 1) for ww in (TILE_W - 1, TILE_W, TILE_W + 1)]
TWO_TILES = (2 * TILE_H + 1, 2 * TILE_W + 1)
INTRINSICS = np.array([[41.5, 0.0, 17.25], [0.0, 39.0, 6.5], [0.0, 0.0, 1.0]])

# the stages on and off, every combination of edge test and normals (the two that change the halo) at a radius each
OPTION_SETS = {
    'all off': dict(radius=0, range0=0.05),
    'filter only r1': dict(radius=1, sigma_space=0.8, range0=0.05),
    'filter only r4': dict(radius=4, sigma_space=2.5, range0=0.08, range2=0.004),
    'edge only': dict(radius=0, range0=0.05, edge_abs=0.1, edge_rel=0.01),
    'normals only': dict(radius=0, range0=0.05, normals=True),
    'angle only': dict(radius=0, range0=0.05, max_angle=60.0),
    'edge + filter r1': dict(radius=1, sigma_space=1.0, range0=0.06, edge_abs=0.12),
    'filter r4 + normals': dict(radius=4, sigma_space=2.0, range0=0.06, normals=True, near=0.3, far=4.0),
    'all on r1': dict(radius=1, sigma_space=1.0, range0=0.06, range2=0.002, edge_abs=0.05, edge_rel=0.02, near=0.3, far=4.0,
                      max_angle=70.0, normals=True),
    'all on r4': dict(radius=4, sigma_space=1.5, range0=0.06, edge_abs=0.12, max_angle=75.0, normals=True),
}


def surface(n, h, w, seed, noise=0.01):
    """f32 [n,h,w]: a slanted, gently curved surface between about 1 and 3 m with a depth step along a slanted line and
    Gaussian noise; different in every frame."""
    rng = np.random.default_rng([77, seed, n, h, w])
    r, c = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    out = np.empty((n, h, w), dtype=np.float64)
    for i in range(n):
        gx, gy = rng.uniform(-0.01, 0.01, 2)
        z = 1.5 + 0.3 * (i % 5) + gx * c + gy * r + 0.05 * np.sin(0.4 * c + i) * np.cos(0.3 * r)
        z = z + np.where(c + 0.5 * r > rng.uniform(0.3, 0.7) * (w + 0.5 * h), 0.6, 0.0)
        out[i] = z + rng.normal(0.0, noise, size=z.shape)
    return out.astype(F)


def with_bad_pixels(depth, seed):
    """(depth, mask): about a tenth of the pixels replaced by NaN, +inf, -inf, negative values, zeros and values off the
    [0.3, 4] range in turn, and a mask that clears about another tenth."""
    rng = np.random.default_rng([78, seed])
    d = depth.copy()
    bad = np.array([np.nan, np.inf, -np.inf, -1.25, 0.0, 0.1, 7.5], dtype=F)
    pick = rng.random(d.shape) < 0.1
    d[pick] = bad[rng.integers(0, bad.size, size=int(pick.sum()))]
    mask = rng.random(d.shape) >= 0.1
    return d, mask


def with_border_holes(depth):
    """Holes (0) on the image border - corners, a run along the first row and last column - and on the borders of the
    kernel's tiles: the last row / column of a tile and the first of the next, where the image has them."""
    d = depth.copy()
    n, h, w = d.shape
    d[:, 0, 0] = 0
    d[:, h - 1, w - 1] = 0
    d[:, 0, w // 3:w // 3 + 3] = 0
    d[:, h // 2:h // 2 + 2, w - 1] = 0
    for r in range(TILE_H, h, TILE_H):
        d[:, r - 1, 1::5] = 0
        d[:, r, 3::5] = 0
    for c in range(TILE_W, w, TILE_W):
        d[:, 0::3, c - 1] = 0
        d[:, 1::3, c] = 0
    return d


def tile_border_steps(h=3 * TILE_H, w=2 * TILE_W + 5):
    """f32 [3,h,w]: a depth step along the horizontal tile border r = TILE_H, one along the vertical tile border c = TILE_W,
    and one that crosses both diagonally; a little noise everywhere."""
    rng = np.random.default_rng(79)
    r, c = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    d = np.stack([np.where(r >= TILE_H, 2.0, 1.4), np.where(c >= TILE_W, 1.2, 2.1), np.where(c - TILE_W >= 2 * (r - TILE_H), 1.0, 1.7)])
    return (d + rng.normal(0.0, 0.004, size=d.shape)).astype(F)
