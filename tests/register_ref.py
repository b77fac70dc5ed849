"""numpy restatement of the registration's definition (csrc/ojf_register.hip header, include/ojf.h ojf_register): the
selection, the association in fp32 with every operation rounded on its own (one ufunc per operation: the kernel's bits), the
29 terms as exact fp64 products, and - through track_ref - the fp64 Cholesky solve and pose update in the kernel's order; the
signed distance field of the coarse stage from distance_ref; the host's conditioning and the loop over the stages.  Test
helper, not a test."""
import numpy as np

import distance_ref
import track_ref

f32 = np.float32
REASONS = ('inlier', 'outside the fixed grid', 'a corner without a value', 'field saturated', 'residual too large', 'no gradient')
POINTS_PER_BLOCK = 1024  # csrc/ojf_gauss_newton.h kTrackPixPerBlock


def observed(tsdf, weights):
    """ojf_blocks.h voxel_observed: weight > 0 and the TSDF a number."""
    t, w = np.asarray(tsdf, np.float16).astype(f32), np.asarray(weights, np.float16).astype(f32)
    with np.errstate(invalid='ignore'):
        return (w > 0) & ~np.isnan(t)


def select(tsdf, weights, band, stride):
    """u32 [n]: the linear indices of the points, increasing."""
    t = np.asarray(tsdf, np.float16).astype(f32)
    ok = observed(tsdf, weights)
    with np.errstate(invalid='ignore'):
        ok &= np.abs(t) < f32(band)
    on = np.zeros(t.shape, bool)
    on[::stride, ::stride, ::stride] = True
    return np.flatnonzero(ok & on).astype(np.uint32)


def _lerp(a, b, f):
    return (a + (f * (b - a).astype(f32)).astype(f32)).astype(f32)


def interpolate(v, fx, fy, fz):
    """(F, Gx, Gy, Gz) f32 of the corner values v[..., bx, by, bz] f32 at the fractions fx, fy, fz, in the definition's order
    (G is the gradient per voxel: not yet divided by the resolution)."""
    v = np.asarray(v, f32)
    dz = [[(v[..., bx, by, 1] - v[..., bx, by, 0]).astype(f32) for by in range(2)] for bx in range(2)]
    e2 = [[_lerp(v[..., bx, by, 0], v[..., bx, by, 1], fz) for by in range(2)] for bx in range(2)]
    e1 = [_lerp(e2[bx][0], e2[bx][1], fy) for bx in range(2)]
    F = _lerp(e1[0], e1[1], fx)
    Gx = (e1[1] - e1[0]).astype(f32)
    Gy = _lerp((e2[0][1] - e2[0][0]).astype(f32), (e2[1][1] - e2[1][0]).astype(f32), fx)
    Gz = _lerp(_lerp(dz[0][0], dz[0][1], fy), _lerp(dz[1][0], dz[1][1], fy), fx)
    return F, Gx, Gy, Gz


def associate(moving_tsdf, moving_origin, moving_resolution, points, fixed, fixed_origin, fixed_resolution, pose, field_band,
              dist):
    """(J f32[n,6], r f32[n], reason u8[n]) of the points (u32 linear indices of the moving volume).  ``fixed``: the pair
    (tsdf f16, weights f16) - the TSDF form - or an f32 [X,Y,Z] field; origins f64[3] and resolutions are rounded to fp32 as
    the entry points do; pose the current f64 pose [3,4]."""
    mt = np.asarray(moving_tsdf, np.float16)
    n = np.asarray(points, np.uint32).astype(np.int64)
    count = len(n)
    reason = np.zeros(count, np.uint8)
    open_ = np.ones(count, bool)

    def mark(cond, code):
        nonlocal open_
        reason[open_ & cond] = code
        open_ = open_ & ~cond

    mark(n >= mt.size, 1)
    n = np.where(open_, n, 0)
    Y, Z = mt.shape[1], mt.shape[2]
    idx = [n // Z // Y, n // Z % Y, n % Z]
    aT = mt.reshape(-1)[n].astype(f32)
    mres, fres = f32(moving_resolution), f32(fixed_resolution)
    mo, fo = np.asarray(moving_origin, np.float64).astype(f32), np.asarray(fixed_origin, np.float64).astype(f32)
    P = np.asarray(pose, np.float64).reshape(-1, 4)[:3].astype(f32)
    R, t = P[:, :3], P[:, 3]
    tsdf_form = isinstance(fixed, tuple)
    if tsdf_form:
        ft = np.asarray(fixed[0], np.float16)
        counts = observed(fixed[0], fixed[1])
        values = ft.astype(f32)
    else:
        values = np.asarray(fixed, f32)
        counts = np.isfinite(values)
    N = values.shape
    with np.errstate(all='ignore'):
        x = [(((idx[a].astype(f32) + f32(0.5)).astype(f32) * mres).astype(f32) + mo[a]).astype(f32) for a in range(3)]
        q = [((((R[i, 0] * x[0]).astype(f32) + (R[i, 1] * x[1]).astype(f32)).astype(f32) + (R[i, 2] * x[2]).astype(f32)).astype(f32)
              + t[i]).astype(f32) for i in range(3)]
        g = [(((q[a] - fo[a]).astype(f32) / fres).astype(f32) - f32(0.5)).astype(f32) for a in range(3)]
        fl = [np.floor(g[a]) for a in range(3)]
        mark(~(np.isfinite(g[0]) & np.isfinite(g[1]) & np.isfinite(g[2])), 1)
        for a in range(3):
            inside = (fl[a] >= 0) & (fl[a] < f32(2147483648.0))
            i0 = np.where(inside, fl[a], 0).astype(np.int64)
            mark(~inside | (i0 + 1 > N[a] - 1), 1)
        i0 = [np.where(open_, fl[a], 0).astype(np.int64) for a in range(3)]
        f = [(g[a] - fl[a]).astype(f32) for a in range(3)]
        v = np.zeros((count, 2, 2, 2), f32)
        every = np.ones(count, bool)
        for bx in range(2):
            for by in range(2):
                for bz in range(2):
                    at = (np.where(open_, i0[0] + bx, 0), np.where(open_, i0[1] + by, 0), np.where(open_, i0[2] + bz, 0))
                    every &= counts[at]
                    v[:, bx, by, bz] = np.where(counts[at], values[at], f32(0))
        mark(~every, 2)
        F, Gx, Gy, Gz = interpolate(v, f[0], f[1], f[2])
        grad = [(G / fres).astype(f32) for G in (Gx, Gy, Gz)]
        mark(~(np.abs(F) < f32(field_band)), 3)
        r = (F - aT).astype(f32)
        mark(~(np.abs(r) <= f32(dist)), 4)
        gg = (((grad[0] * grad[0]).astype(f32) + (grad[1] * grad[1]).astype(f32)).astype(f32) + (grad[2] * grad[2]).astype(f32)).astype(f32)
        mark(~(gg > 0) | ~np.isfinite(gg), 5)
        Jv = [((q[1] * grad[2]).astype(f32) - (q[2] * grad[1]).astype(f32)).astype(f32),
              ((q[2] * grad[0]).astype(f32) - (q[0] * grad[2]).astype(f32)).astype(f32),
              ((q[0] * grad[1]).astype(f32) - (q[1] * grad[0]).astype(f32)).astype(f32), grad[0], grad[1], grad[2]]
    ok = open_
    J = np.zeros((count, 6), f32)
    for i in range(6):
        J[:, i] = np.where(ok, Jv[i], f32(0))
    return J, np.where(ok, r, f32(0)).astype(f32), reason


def kernel_sums(terms_of_points):
    """f64[29] of the per-point terms [n, 29] (zero rows for outliers) in the kernels' order: per block of 1024 points lane t
    adds its points t, t+256, t+512, t+768 in order, the wave's 64 lanes by a shift-down tree, the four waves in order; the
    solve adds the blocks in order."""
    T = np.asarray(terms_of_points, np.float64)
    n = len(T)
    blocks = (n + POINTS_PER_BLOCK - 1) // POINTS_PER_BLOCK
    pad = np.zeros((blocks * POINTS_PER_BLOCK, T.shape[1]))
    pad[:n] = T
    pad = pad.reshape(blocks, 4, 256, T.shape[1])
    lane = np.zeros((blocks, 256, T.shape[1]))
    for k in range(4):
        lane = lane + pad[:, k]
    lane = lane.reshape(blocks, 4, 64, T.shape[1])
    off = 32
    while off:
        shifted = np.zeros_like(lane)
        shifted[:, :, :64 - off] = lane[:, :, off:]
        lane = lane + shifted  # (lanes past 64 - off add what the shuffle hands them: their own sums never reach lane 0)
        off >>= 1
    wave = lane[:, :, 0]
    rows = np.zeros((blocks, T.shape[1]))
    for w in range(4):
        rows = rows + wave[:, w]
    total = np.zeros(T.shape[1])
    for b in range(blocks):
        total = total + rows[b]
    return total


def point_terms(J, r, reason):
    """f64 [n, 29]: the terms of every point, zero rows for outliers."""
    ok = reason == 0
    Jd, rd = J.astype(np.float64), r.astype(np.float64)
    cols = [Jd[:, i] * Jd[:, j] for i in range(6) for j in range(i, 6)]
    cols += [Jd[:, i] * rd for i in range(6)]
    cols += [rd * rd, np.ones_like(rd)]
    return np.where(ok[:, None], np.stack(cols, axis=1), 0.0)


def signed_distance_field(tsdf, weights, resolution, reach=None, edt=distance_ref.edt):
    """f32 [X,Y,Z]: fp32(resolution)·sqrt(fp32(dist2)) to the nearest surface voxel, the sign of that seed for every voxel
    (negative iff fp32(T[nearest]) < 0), NaN with no seed in reach (metres).  ``edt(seeds, max_dist2)`` -> (dist2, nearest):
    distance_ref.edt, the definition; ``scipy_edt`` is the same function but for which of equally near seeds it names."""
    limit = -1 if reach is None else int(min(np.floor((float(reach) / float(resolution)) ** 2), 2 ** 24))
    dist2, nearest = edt(distance_ref.surface_mask(tsdf, weights), limit)
    none = nearest < 0
    with np.errstate(invalid='ignore'):
        mag = (np.sqrt(np.where(none, 0, dist2).astype(f32)) * f32(resolution)).astype(f32)
    t = np.asarray(tsdf, np.float16).astype(f32).reshape(-1)[np.where(none, 0, nearest).reshape(-1)].reshape(mag.shape)
    with np.errstate(invalid='ignore'):
        field = np.where(t < 0, -mag, mag)
    return np.where(none, f32(np.nan), field).astype(f32)


def scipy_edt(seeds, max_dist2=-1):
    """(dist2 i32, nearest i32) from scipy.ndimage.distance_transform_edt: exact like distance_ref.edt and much faster; of
    equally near seeds it may name another one."""
    from scipy import ndimage
    seeds = np.asarray(seeds) != 0
    if not seeds.any():
        return np.full(seeds.shape, distance_ref.NONE, np.int32), np.full(seeds.shape, -1, np.int32)
    at = ndimage.distance_transform_edt(~seeds, return_distances=False, return_indices=True).astype(np.int64)
    own = np.indices(seeds.shape)
    dist2 = ((at - own) ** 2).sum(axis=0)
    nearest = (at[0] * seeds.shape[1] + at[1]) * seeds.shape[2] + at[2]
    gone = dist2 > max_dist2 if max_dist2 >= 0 else np.zeros(seeds.shape, bool)
    return np.where(gone, distance_ref.NONE, dist2).astype(np.int32), np.where(gone, -1, nearest).astype(np.int32)


def coarse_reach(stages, band, fixed_resolution):
    """The reach (metres) of the 'sdf' stages' field: their largest dist + band + 4 voxels."""
    return max(float(s['dist']) for s in stages if s['field'] == 'sdf') + float(band) + 4.0 * float(fixed_resolution)


def condition(moving_shape, moving_origin, moving_resolution, R0, t0):
    """(c_m, c_f) f64: the centre of the moving box and its image under the initial transform, the origins of the shifted
    worlds."""
    c_m = np.asarray(moving_origin, np.float64) + 0.5 * float(moving_resolution) * np.asarray(moving_shape, np.float64)
    return c_m, np.asarray(R0, np.float64) @ c_m + np.asarray(t0, np.float64)


def run(moving, fixed, stages, transform=None, band=None, min_inlier_fraction=0.05, field=None, trace=None):
    """The whole call (registration.register_volumes): dict(transform f64[3,4], status (code, iteration), stats f64[n,4],
    n_points per stage).  moving / fixed: dicts of numpy tsdf / weights (f16), origin, resolution; stages: dicts with field
    ('sdf' | 'tsdf'), stride, iterations, dist, field_band; ``field``: the signed distance field of the 'sdf' stages (default:
    signed_distance_field of fixed up to coarse_reach).  The sums are numpy's (not the kernels' summation order).  ``trace``: a list that
    receives, per step that ran, dict(stage, pose (before the step, in the shifted worlds), sums, code)."""
    T = np.eye(4)[:3] if transform is None else np.asarray(transform, np.float64).reshape(-1, 4)[:3]
    R0, t0 = T[:, :3], T[:, 3]
    c_m, c_f = condition(moving['tsdf'].shape, moving['origin'], moving['resolution'], R0, t0)
    o_m, o_f = np.asarray(moving['origin'], np.float64) - c_m, np.asarray(fixed['origin'], np.float64) - c_f
    E0 = np.concatenate([R0, np.zeros((3, 1))], axis=1)
    band = 3.0 * float(moving['resolution']) if band is None else band
    n_it = sum(int(s['iterations']) for s in stages)
    stats = np.zeros((n_it, 4))
    P, status, it, n_points = E0.copy(), (0, -1), 0, []
    for k, s in enumerate(stages):
        pts = select(moving['tsdf'], moving['weights'], band, int(s['stride']))
        n_points.append(len(pts))
        if len(pts) == 0:
            raise ValueError('register_ref.run: no points')
        if s['field'] == 'sdf':
            if field is None:
                field = signed_distance_field(fixed['tsdf'], fixed['weights'], fixed['resolution'],
                                              reach=coarse_reach(stages, band, fixed['resolution']))
            target, fband = field, s.get('field_band') or np.inf
        else:
            target, fband = (fixed['tsdf'], fixed['weights']), s.get('field_band')
            if fband is None:
                t = np.asarray(fixed['tsdf'], np.float16).astype(f32)
                fband = np.nextafter(np.where(observed(fixed['tsdf'], fixed['weights']), np.abs(t), f32(0)).max(), f32(0))
        for _ in range(int(s['iterations'])):
            if not status[0]:
                J, r, reason = associate(moving['tsdf'], o_m, moving['resolution'], pts, target, o_f, fixed['resolution'], P, fband,
                                         s['dist'])
                sums = point_terms(J, r, reason).sum(axis=0)
                code, Q, th, tau = track_ref.step(sums, P, float(min_inlier_fraction) * len(pts), moves=True)
                if trace is not None:
                    trace.append(dict(stage=k, pose=P.copy(), sums=sums, code=code, reason=reason))
                stats[it] = (sums[28], sums[27] / sums[28] if sums[28] > 0 else 0.0, th, tau)
                if code:
                    status, P = (code, it), E0.copy()
                else:
                    P = Q
            it += 1
    out = P.copy()
    out[:, 3] = out[:, 3] + c_f - out[:, :3] @ c_m
    if status[0]:
        out = T.copy()
    return dict(transform=out, status=status, stats=stats, n_points=n_points)


def transform_error(P, truth, points):
    """The largest distance (metres) between the images of ``points`` [n,3] under two transforms [3,4]."""
    P, G = np.asarray(P, np.float64).reshape(-1, 4)[:3], np.asarray(truth, np.float64).reshape(-1, 4)[:3]
    d = points @ (P[:, :3] - G[:, :3]).T + (P[:, 3] - G[:, 3])
    return float(np.linalg.norm(d, axis=1).max())


def axis_angle(axis, degrees):
    a = np.asarray(axis, np.float64)
    return track_ref.rodrigues(a / np.linalg.norm(a) * np.radians(degrees))


# ---- the scenes of the tests: the synthetic room sampled analytically in two worlds ----------------------------------------
def sampled_scene(shape, origin, resolution, truncation, world_from_room=None, observed_if=None):
    """dict(tsdf f16, weights f16, origin, resolution) of synthetic.scene_sdf sampled at the voxel centres of a box whose world
    is the room's moved by ``world_from_room`` [3,4] (default: the room's own).  Voxels more than the truncation behind the
    surface are unobserved (weight 0), and so are those where ``observed_if(world points [...,3])`` is false."""
    from online_joint_depthfusion_and_semantic_amd import synthetic
    origin = np.asarray(origin, np.float64)
    ax = [origin[a] + (np.arange(shape[a]) + 0.5) * resolution for a in range(3)]
    pts = np.stack(np.meshgrid(*ax, indexing='ij'), axis=-1)
    room = pts
    if world_from_room is not None:
        W = np.asarray(world_from_room, np.float64)
        room = (pts - W[:, 3]) @ W[:, :3]  # R^T (x - t)
    sd = synthetic.scene_sdf(room)
    seen = sd > -truncation
    if observed_if is not None:
        seen &= observed_if(pts)
    return dict(tsdf=np.clip(sd, -truncation, truncation).astype(np.float16), weights=seen.astype(np.float16),
                origin=origin, resolution=float(resolution))
