"""numpy restatement of joint geometric + photometric tracking (csrc/ojf_track_rgbd.hip header, include/ojf.h
ojf_track_rgbd): the geometry is track_ref's (imported, not copied), the intensity pyramid, the model maps, the bilinear
fetch and the photometric row are restated here in fp32 with every operation rounded on its own, the terms as exact fp64
products and the solve as track_ref's.  Also the analytic cases the CPU and GPU tests share.  Test helper, not a test."""
import math

import numpy as np

import color_ref
import track_ref
from track_ref import _dc, _dot3, f32

PHOTO_REASONS = {0: 'row added', 1: 'no depth', 3: 'behind the reference camera', 4: 'outside the model image',
                 5: 'no model depth', 6: 'too far', 8: 'a bilinear corner is not valid', 9: 'residual beyond photo_thresh',
                 10: 'photometric term off'}
# the defaults of tracking.track_frame_rgbd (DESIGN.md section 25 has the sweep they come from)
PHOTO_WEIGHT, PHOTO_THRESH = 0.002, 40.0


def intensity(image):
    """f32 [h,w]: (77 R + 150 G + 29 B) / 256 of a u8 [h,w,3|4] image (integer arithmetic, one conversion, one exact
    division)."""
    im = np.asarray(image, np.uint8).astype(np.int32)
    return ((77 * im[..., 0] + 150 * im[..., 1] + 29 * im[..., 2]).astype(f32) / f32(256)).astype(f32)


def intensity_pyramid(image, levels):
    """[I_0, .., I_{levels-1}]: level l+1 is (((a + b) + c) + d) * 0.25 of the block (2r,2c), (2r,2c+1), (2r+1,2c),
    (2r+1,2c+1)."""
    out = [intensity(image)]
    for _ in range(1, levels):
        I = out[-1]
        h, w = I.shape[0] >> 1, I.shape[1] >> 1
        a, b, c, d = I[0:2 * h:2, 0:2 * w:2], I[0:2 * h:2, 1:2 * w:2], I[1:2 * h:2, 0:2 * w:2], I[1:2 * h:2, 1:2 * w:2]
        out.append(((((a + b).astype(f32) + c).astype(f32) + d).astype(f32) * f32(0.25)).astype(f32))
    return out


def model_map(mcolor, mdepth, grad_depth):
    """f32 [h,w,4] records (I_m, gx, gy, valid) of one level's model colour u8 [h,w,4] and model depth f32 [h,w]."""
    mcolor = np.asarray(mcolor, np.uint8)
    h, w = mcolor.shape[:2]
    d = np.asarray(mdepth, f32).reshape(h, w)
    has = mcolor[..., 3] != 0
    I = np.where(has, intensity(mcolor), f32(0)).astype(f32)
    lim = f32(grad_depth)
    out = np.zeros((h, w, 4), f32)
    out[..., 0] = I
    if h < 3 or w < 3:
        return out
    c = (slice(1, h - 1), slice(1, w - 1))
    nb = {'l': (slice(1, h - 1), slice(0, w - 2)), 'r': (slice(1, h - 1), slice(2, w)),
          'u': (slice(0, h - 2), slice(1, w - 1)), 'd': (slice(2, h), slice(1, w - 1))}
    ok = has[c].copy()
    with np.errstate(invalid='ignore'):
        for s in nb.values():
            ok &= has[s] & (np.abs((d[s] - d[c]).astype(f32)) <= lim)
    gx = ((I[nb['r']] - I[nb['l']]).astype(f32) * f32(0.5)).astype(f32)
    gy = ((I[nb['d']] - I[nb['u']]).astype(f32) * f32(0.5)).astype(f32)
    out[..., 1][c] = np.where(ok, gx, f32(0))
    out[..., 2][c] = np.where(ok, gy, f32(0))
    out[..., 3][c] = np.where(ok, f32(1), f32(0))
    return out


def _lerp2(v00, v01, v10, v11, ax, ay):
    top = (v00 + (ax * (v01 - v00).astype(f32)).astype(f32)).astype(f32)
    bot = (v10 + (ax * (v11 - v10).astype(f32)).astype(f32)).astype(f32)
    return (top + (ay * (bot - top).astype(f32)).astype(f32)).astype(f32)


def associate(D, I_live, Ki, K, level, mdepth, mnormal, mmap, E_ref, pose, dist_thresh=0.1, angle_thresh=20.0,
              photo_weight=PHOTO_WEIGHT, photo_thresh=PHOTO_THRESH):
    """dict(J, r, reason: track_ref.associate's; pJ f32[h,w,6], pr f32[h,w]: the unscaled photometric row (0 unless
    preason == 0); preason u8[h,w]; mrow, mcol i64[h,w]: the model pixel of every live pixel that passed the checks of the
    geometry other than those on normals, else -1 (absent at photo_weight 0)) of one level."""
    D = np.asarray(D, f32)
    h, w = D.shape
    J, r, reason, mr, mc = track_ref.associate(D, Ki, K, level, mdepth, mnormal, E_ref, pose, dist_thresh, angle_thresh,
                                               pixels=True)
    pJ, pr = np.zeros((h, w, 6), f32), np.zeros((h, w), f32)
    if f32(photo_weight) == 0:
        return dict(J=J, r=r, reason=reason, pJ=pJ, pr=pr, preason=np.full((h, w), 10, np.uint8))
    Ki = np.asarray(Ki, f32).reshape(9)
    fx, fy, cx, cy = (f32(v) for v in track_ref.level_intrinsics(K, level))
    P = np.asarray(pose, np.float64).reshape(-1, 4)[:3].astype(f32)
    Er = np.asarray(E_ref, np.float64).reshape(-1, 4)[:3].astype(f32)
    R, t, Rr, tr = P[:, :3], P[:, 3], Er[:, :3], Er[:, 3]
    dist2 = f32(float(dist_thresh) * float(dist_thresh))
    mdepth = np.asarray(mdepth, f32).reshape(h, w)
    mmap = np.asarray(mmap, f32).reshape(h, w, 4)
    rr, cc = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    preason = np.zeros((h, w), np.uint8)
    open_ = np.ones((h, w), bool)

    def mark(cond, code):
        nonlocal open_
        hit = open_ & cond
        preason[hit] = code
        open_ = open_ & ~cond

    mark(D == 0, 1)
    dc = _dc(Ki, rr, cc)
    v = [(D * dc[i]).astype(f32) for i in range(3)]
    with np.errstate(all='ignore'):
        p = [(_dot3(R[i], v) + t[i]).astype(f32) for i in range(3)]
        e = [(p[i] - tr[i]).astype(f32) for i in range(3)]
        q = [_dot3(Rr[:, i], e) for i in range(3)]
        mark(~(q[2] > 0), 3)
        ux = ((fx * (q[0] / q[2]).astype(f32)).astype(f32) + cx).astype(f32)
        uy = ((fy * (q[1] / q[2]).astype(f32)).astype(f32) + cy).astype(f32)
        fc = np.floor((ux + f32(0.5)).astype(f32))
        fr = np.floor((uy + f32(0.5)).astype(f32))
        mark(~((fc >= 0) & (fc < f32(w)) & (fr >= 0) & (fr < f32(h))), 4)
        pr_, pc_ = np.where(open_, fr, 0).astype(np.int64), np.where(open_, fc, 0).astype(np.int64)
        dm = mdepth[pr_, pc_]
        mark(dm == 0, 5)
        dcm = _dc(Ki, pr_, pc_)
        mv = [(dm * dcm[i]).astype(f32) for i in range(3)]
        m = [(_dot3(Rr[i], mv) + tr[i]).astype(f32) for i in range(3)]
        g = [(p[i] - m[i]).astype(f32) for i in range(3)]
        mark(_dot3(g, g) > dist2, 6)
        # what is open now passed every check of the geometry but the two on normals
        assert np.isin(reason[open_], (0, 2, 7)).all() and not np.isin(reason[~open_], (0, 7)).any()
        mrow, mcol = np.where(open_, pr_, -1), np.where(open_, pc_, -1)
        x0f, y0f = np.floor(ux), np.floor(uy)
        inside = (x0f >= 0) & (x0f <= f32(w - 2)) & (y0f >= 0) & (y0f <= f32(h - 2))
        x0 = np.where(open_ & inside, x0f, 0).astype(np.int64)
        y0 = np.where(open_ & inside, y0f, 0).astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
        c00, c01, c10, c11 = mmap[y0, x0], mmap[y0, x1], mmap[y1, x0], mmap[y1, x1]
        valid = inside & (c00[..., 3] != 0) & (c01[..., 3] != 0) & (c10[..., 3] != 0) & (c11[..., 3] != 0)
        mark(~valid, 8)
        ax, ay = (ux - x0f).astype(f32), (uy - y0f).astype(f32)
        Im, gx, gy = (_lerp2(c00[..., k], c01[..., k], c10[..., k], c11[..., k], ax, ay) for k in range(3))
        rI = (Im - np.asarray(I_live, f32)).astype(f32)
        mark(~(np.abs(rI) <= f32(photo_thresh)), 9)
        a0, a1 = (fx * gx).astype(f32), (fy * gy).astype(f32)
        gc = [(a0 / q[2]).astype(f32), (a1 / q[2]).astype(f32),
              -(((a0 * q[0]).astype(f32) + (a1 * q[1]).astype(f32)).astype(f32) / (q[2] * q[2]).astype(f32)).astype(f32)]
        a = [_dot3(Rr[i], gc) for i in range(3)]
        Jv = [((p[1] * a[2]).astype(f32) - (p[2] * a[1]).astype(f32)).astype(f32),
              ((p[2] * a[0]).astype(f32) - (p[0] * a[2]).astype(f32)).astype(f32),
              ((p[0] * a[1]).astype(f32) - (p[1] * a[0]).astype(f32)).astype(f32), a[0], a[1], a[2]]
    ok = open_
    for i in range(6):
        pJ[..., i] = np.where(ok, Jv[i], f32(0))
    pr[:] = np.where(ok, rI, f32(0))
    return dict(J=J, r=r, reason=reason, pJ=pJ, pr=pr, preason=preason, mrow=mrow, mcol=mcol)


def _rows(J, r):
    Jd, rd = J.astype(np.float64), r.astype(np.float64)
    cols = [Jd[:, i] * Jd[:, j] for i in range(6) for j in range(i, 6)]
    cols += [Jd[:, i] * rd for i in range(6)]
    cols += [rd * rd]
    return np.stack(cols, axis=1)


def term_matrix(a, photo_weight=PHOTO_WEIGHT):
    """fp64 terms [n_pixels, 29] of an ``associate`` result: a pixel's geometric row (reason 0) plus its photometric row
    (preason 0, scaled in fp32 by fp32(photo_weight)); term 28 is 1 for a pixel with at least one row."""
    lam = f32(photo_weight)
    geo = (a['reason'] == 0).reshape(-1)
    pho = (a['preason'] == 0).reshape(-1)
    with np.errstate(invalid='ignore'):
        G = _rows(a['J'].reshape(-1, 6), a['r'].reshape(-1))
        Pm = _rows((lam * a['pJ'].reshape(-1, 6)).astype(f32), (lam * a['pr'].reshape(-1)).astype(f32))
        T = np.where(geo[:, None], G, 0.0) + np.where(pho[:, None], Pm, 0.0)
    T = np.concatenate([T, (geo | pho).astype(np.float64)[:, None]], axis=1)
    return T[geo | pho]


def pivot_margin(sums):
    """The smallest Cholesky pivot d_j of the solve over its acceptance threshold 1e-6 * max diag (the solve fails at
    <= 1; inf when it has no system)."""
    A, _ = track_ref.system(sums)
    thr = 1e-6 * max(A[j, j] for j in range(6))
    L = np.zeros((6, 6))
    worst = math.inf
    for j in range(6):
        d = A[j, j] - float(L[j, :j] @ L[j, :j])
        worst = min(worst, d / thr if thr > 0 else -math.inf)
        if not d > thr:
            return worst
        L[j, j] = math.sqrt(d)
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - float(L[i, :j] @ L[j, :j])) / L[j, j]
    return worst


def run(depth, mask, image, K, Kinv, mdepth, mnormal, mcolor, E_ref, E_init, iterations, dist_thresh=0.1, angle_thresh=20.0,
        delta=0.03, min_inlier_fraction=0.05, photo_weight=PHOTO_WEIGHT, photo_thresh=PHOTO_THRESH, grad_depth=None,
        trace=None):
    """The whole call (ojf_track_rgbd): (pose f64[3,4], (code, iteration), stats f64[n,4]), as track_ref.run with the live
    image u8 [h,w,3|4] and per-level model colour images u8 [h_l,w_l,4].  ``trace`` receives per step dict(level, pose,
    reason, preason, sums, code, margin)."""
    levels = len(mdepth)
    grad_depth = dist_thresh if grad_depth is None else grad_depth
    E0 = np.asarray(E_init, np.float64).reshape(-1, 4)[:3].copy()
    pyr = track_ref.pyramid(depth, mask, levels, delta)
    ipyr = intensity_pyramid(image, levels)
    maps = [model_map(mcolor[l], mdepth[l], grad_depth) for l in range(levels)]
    steps = track_ref.schedule(iterations, levels)
    stats = np.zeros((len(steps), 4))
    P, status = E0.copy(), (0, -1)
    for it, l in enumerate(steps):
        if status[0]:
            continue
        a = associate(pyr[l], ipyr[l], Kinv[l], K, l, mdepth[l], mnormal[l], maps[l], E_ref, P, dist_thresh, angle_thresh,
                      photo_weight, photo_thresh)
        with np.errstate(invalid='ignore'):
            sums = term_matrix(a, photo_weight).sum(axis=0)
        code, Q, th, tau = track_ref._step(sums, P, float(min_inlier_fraction) * float(pyr[l].size))
        if trace is not None:
            trace.append(dict(level=l, pose=P.copy(), reason=a['reason'], preason=a['preason'], sums=sums, code=code,
                              margin=pivot_margin(sums) if sums[28] > 0 else math.inf))
        stats[it] = (sums[28], sums[27] / sums[28] if sums[28] > 0 else 0.0, th, tau)
        if code:
            status, P = (code, it), E0.copy()
        else:
            P = Q
    return P, status, stats


# ---- cases ---------------------------------------------------------------------------------------------------------------
PLANE_N = np.array([0.0, 0.5, 1.0])  # gradient of render_ref.plane_case's T = 0.5 (y - 2) + (z - 1.5)
# (rotation in degrees, translation in m, axis, direction) of track_ref.perturb: 3 cm / 2 deg in the plane's own freedoms
# (rotation about its normal, a slide along x), 5 cm / 2.4 deg general, 8 cm / 4 deg in-plane
PLANE_STARTS = ((2.0, 0.03, (0.0, 0.5, 1.0), (1.0, 0.0, 0.0)),
                (2.4, 0.05, (1.0, -1.0, 0.5), (1.0, 0.5, -0.4)),
                (4.0, 0.08, (0.0, 0.5, 1.0), (1.0, 2.0, -1.0)))


def plane_view(E, K, h, w):
    """(depth f64[h,w], points f64[h,w,3], image u8[h,w,4]) of plane_case's plane painted with color_ref.analytic_color,
    seen from the camera-to-world pose E with intrinsics K (alpha 255 everywhere: the plane fills every view used)."""
    E = np.asarray(E, np.float64).reshape(-1, 4)[:3]
    K = np.asarray(K, np.float64).reshape(3, 3)
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    dc = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], axis=-1)
    dw = dc @ E[:, :3].T
    eye = E[:, 3]
    T0 = 0.5 * (eye[1] - 2.0) + (eye[2] - 1.5)
    t = -T0 / (dw @ PLANE_N)
    assert (t > 0).all()
    pts = eye + t[..., None] * dw
    img = np.full((h, w, 4), 255, np.uint8)
    img[..., :3] = np.round(color_ref.analytic_color(pts)).astype(np.uint8)
    return t, pts, img


def plane_tracking_case(start, h=48, w=64, levels=3):
    """The textured plane: the live frame at plane_case's pose (the truth), the model images analytic at the perturbed
    start PLANE_STARTS[start] (reference pose = start).  dict(depth, image, K, Kinv, mdepth, mnormal, mcolor, E_ref,
    E_init, E_true)."""
    from online_joint_depthfusion_and_semantic_amd.ops import camera_arrays
    from render_ref import plane_case
    _, _, _, K, E_true, want, normal = plane_case(64, h, w)
    depth, _, image = plane_view(E_true, K, h, w)
    assert np.abs(depth - want).max() < 1e-12
    E0 = track_ref.perturb(E_true, *PLANE_STARTS[start])
    Kinv, md, mn, mcol = [], [], [], []
    for l in range(levels):
        Kl = np.eye(3)
        Kl[0, 0], Kl[1, 1], Kl[0, 2], Kl[1, 2] = track_ref.level_intrinsics(K, l)
        hl, wl = h >> l, w >> l
        t, _, img = plane_view(E0, Kl, hl, wl)
        Kinv.append(camera_arrays(Kl, E0)[0])
        md.append(t.astype(f32))
        mn.append(np.broadcast_to(normal.astype(f32), (hl, wl, 3)).copy())
        mcol.append(img)
    return dict(depth=depth.astype(f32), image=image, K=K, Kinv=Kinv, mdepth=md, mnormal=mn, mcolor=mcol, E_ref=E0,
                E_init=E0, E_true=E_true)


def _level_K(K, l):
    Kl = np.eye(3)
    Kl[0, 0], Kl[1, 1], Kl[0, 2], Kl[1, 2] = track_ref.level_intrinsics(K, l)
    return Kl


def paint_models(models, E_ref, K):
    """Per level u8 [h_l,w_l,4]: analytic_color at the hit points of track_cases.model_maps' depth images at E_ref, alpha
    255; all 0 where the model has no depth."""
    E_ref = np.asarray(E_ref, np.float64).reshape(-1, 4)[:3]
    out = []
    for l, m in enumerate(models):
        md = m[0]
        Kl = _level_K(K, l)
        hl, wl = md.shape
        u, v = np.meshgrid(np.arange(wl, dtype=np.float64), np.arange(hl, dtype=np.float64))
        dc = np.stack([(u - Kl[0, 2]) / Kl[0, 0], (v - Kl[1, 2]) / Kl[1, 1], np.ones_like(u)], axis=-1)
        pw = E_ref[:, 3] + md.astype(np.float64)[..., None] * (dc @ E_ref[:, :3].T)
        img = np.full((hl, wl, 4), 255, np.uint8)
        img[..., :3] = np.round(color_ref.analytic_color(pw)).astype(np.uint8)
        img[md == 0] = 0
        out.append(img)
    return out


def hostile_case(h, w, levels, seed=0):
    """Inputs that take every path of the associate and prepare kernels at h x w: track_cases.hostile_frame as the live
    depth and mask (NaN, inf, negative, masked pixels), the reference camera 0.5 m in front of the live one (near points
    behind it, border points outside its image or on its outermost rows and columns), a live patch 0.3 m from the camera, one
    pushed 0.3 m back; per level a model patch without depth, one without colour (alpha 0), a depth step of 0.25 m; live and
    model image patches of 0 and 255; the fourth byte of the live image is noise.  Patches are fractions of the frame."""
    from online_joint_depthfusion_and_semantic_amd import synthetic
    import track_cases
    st = synthetic.SyntheticStream(h, w, 64, 400)
    f = st.frame(120)
    depth, mask = track_cases.hostile_frame(h, w, seed)
    E_live = f['extrinsics']
    E_ref = E_live.copy()
    E_ref[:, 3] += 0.5 * E_live[:, 2]

    def box(hl, wl, r0, r1, c0, c1):
        a, b = int(r0 * hl), int(c0 * wl)
        return slice(a, max(int(r1 * hl), a + 1)), slice(b, max(int(c1 * wl), b + 1))

    depth = depth.copy()
    depth[box(h, w, .40, .50, .45, .55)] = 0.3
    depth[box(h, w, .25, .33, .18, .26)] += f32(0.3)
    K = st.K
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    dc = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], axis=-1)
    pw = E_live[:, 3] + f['depth_gt'].astype(np.float64)[..., None] * (dc @ E_live[:, :3].T)
    rng = np.random.default_rng([seed, h, w])
    image = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    image[..., :3] = np.round(color_ref.analytic_color(pw)).astype(np.uint8)
    image[box(h, w, .70, .80, .10, .20)] = 0
    image[box(h, w, .70, .80, .25, .35)] = 255
    models = track_cases.model_maps(E_ref, K, h, w, levels)
    mcol = paint_models(models, E_ref, K)
    md = [m[0].copy() for m in models]
    for l in range(levels):
        hl, wl = h >> l, w >> l
        md[l][box(hl, wl, .50, .62, .20, .38)] += f32(0.25)
        md[l][box(hl, wl, .40, .56, .42, .56)] = 0
        mcol[l][box(hl, wl, .30, .40, .60, .72)] = 0
        mcol[l][box(hl, wl, .12, .24, .40, .50)][..., :3] = 0
        mcol[l][box(hl, wl, .12, .24, .55, .65)][..., :3] = 255
    pose = track_ref.perturb(E_live, 1.5, 0.02, (0.2, 1.0, -0.3), (1.0, -0.5, 0.4))
    return dict(h=h, w=w, levels=levels, depth=depth, mask=mask, image=image, K=K, Kinv=[m[2] for m in models], mdepth=md,
                mnormal=[m[1] for m in models], mcolor=mcol, E_ref=E_ref, pose=pose)


def room_tracking_case(stream, frames, i, start=None, levels=3):
    """Frame pair (i, i+1) of a synthetic stream with color_ref.room_frames images: the model analytic at frame i's pose
    (track_cases.model_maps, painted with analytic_color at its hit points), the live frame i+1 with its ToF depth, the
    start frame i's pose, perturbed by ``start`` when given."""
    import track_cases
    f0, f1 = frames[i], frames[i + 1]
    E_ref = f0['extrinsics']
    h, w = stream.h, stream.w
    models = track_cases.model_maps(E_ref, stream.K, h, w, levels)
    mcol = paint_models(models, E_ref, stream.K)
    E_init = E_ref if start is None else track_ref.perturb(E_ref, *start)
    return dict(depth=f1['tof_depth'], mask=f1['mask'], image=f1['image'], K=stream.K, Kinv=[m[2] for m in models],
                mdepth=[m[0] for m in models], mnormal=[m[1] for m in models], mcolor=mcol, E_ref=E_ref, E_init=E_init,
                E_true=f1['extrinsics'])


def run_case(case, iterations=(10, 5, 4), trace=None, **kw):
    return run(case['depth'], case.get('mask'), case['image'], case['K'], case['Kinv'], case['mdepth'], case['mnormal'],
               case['mcolor'], case['E_ref'], case['E_init'], iterations, trace=trace, **kw)


def run_depth_only(case, iterations=(10, 5, 4), **kw):
    return track_ref.run(case['depth'], case.get('mask'), case['K'], case['Kinv'], case['mdepth'], case['mnormal'],
                         case['E_ref'], case['E_init'], iterations, **kw)
