"""numpy restatement of the tracker's definition (csrc/ojf_track.hip header, include/ojf.h ojf_track): the depth pyramid
and the association in fp32 with every operation rounded on its own (the kernels' bits), the 29 terms as exact fp64
products, and the fp64 Cholesky solve and pose update in the kernel's order.  Test helper, not a test."""
import math

import numpy as np

f32 = np.float32
TERMS = 29
REASONS = ('inlier', 'no depth', 'no normal', 'behind the reference camera', 'outside the model image', 'no model depth',
           'too far', 'normals disagree')


def level_intrinsics(K, level):
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    s = float(1 << level)
    return K[0, 0] / s, K[1, 1] / s, (K[0, 2] + 0.5) / s - 0.5, (K[1, 2] + 0.5) / s - 0.5


def pyramid(depth, mask, levels, delta=0.03):
    """[D_0, .., D_{levels-1}] f32 as the pyramid kernel writes them."""
    d = np.asarray(depth, dtype=f32)
    with np.errstate(invalid='ignore'):
        ok = np.isfinite(d) & (d > f32(0))
    if mask is not None:
        ok &= np.asarray(mask).reshape(d.shape) != 0
    out = [np.where(ok, d, f32(0)).astype(f32)]
    dl = f32(delta)
    for _ in range(1, levels):
        D = out[-1]
        h, w = D.shape[0] >> 1, D.shape[1] >> 1
        blk = [D[0:2 * h:2, 0:2 * w:2], D[0:2 * h:2, 1:2 * w:2], D[1:2 * h:2, 0:2 * w:2], D[1:2 * h:2, 1:2 * w:2]]
        dmin = np.full((h, w), np.inf, f32)
        for v in blk:
            dmin = np.where(v != 0, np.fmin(dmin, v), dmin).astype(f32)
        s = np.zeros((h, w), f32)
        n = np.zeros((h, w), np.int32)
        with np.errstate(invalid='ignore'):
            for v in blk:
                sel = (v != 0) & ((v - dmin).astype(f32) <= dl)
                s = np.where(sel, (s + v).astype(f32), s)
                n += sel
            out.append(np.where(n > 0, (s / n.astype(f32)).astype(f32), f32(0)).astype(f32))
    return out


def _dc(Ki, r, c):
    rf, cf = r.astype(f32), c.astype(f32)
    return [((Ki[3 * i] * cf).astype(f32) + (Ki[3 * i + 1] * rf).astype(f32) + Ki[3 * i + 2]).astype(f32)
            for i in range(3)]


def _dot3(a, b):
    return ((a[0] * b[0]).astype(f32) + (a[1] * b[1]).astype(f32) + (a[2] * b[2]).astype(f32)).astype(f32)


def associate(D, Ki, K, level, mdepth, mnormal, E_ref, pose, dist_thresh=0.1, angle_thresh=20.0, pixels=False):
    """(J f32[h,w,6], r f32[h,w], reason u8[h,w]) of level ``level`` (D its pyramid level, Ki f32[9] the level's Kinv,
    K the level-0 intrinsics, mdepth [h,w] / mnormal [h,w,3] the model images at E_ref, pose the current f64 pose).
    ``pixels``: also the model pixel (row i64[h,w], col i64[h,w]) each live pixel projects to (0 for reasons 1..4)."""
    D = np.asarray(D, f32)
    h, w = D.shape
    Ki = np.asarray(Ki, f32).reshape(9)
    fx, fy, cx, cy = (f32(v) for v in level_intrinsics(K, level))
    P = np.asarray(pose, np.float64).reshape(-1, 4)[:3].astype(f32)
    Er = np.asarray(E_ref, np.float64).reshape(-1, 4)[:3].astype(f32)
    R, t, Rr, tr = P[:, :3], P[:, 3], Er[:, :3], Er[:, 3]
    dist2 = f32(float(dist_thresh) * float(dist_thresh))
    cos_thr = f32(math.cos(float(angle_thresh) * math.pi / 180.0))
    mdepth = np.asarray(mdepth, f32).reshape(h, w)
    mnormal = np.asarray(mnormal, f32).reshape(h, w, 3)

    rr, cc = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    reason = np.zeros((h, w), np.uint8)
    J = np.zeros((h, w, 6), f32)
    res = np.zeros((h, w), f32)
    open_ = np.ones((h, w), bool)

    def mark(cond, code):
        nonlocal open_
        hit = open_ & cond
        reason[hit] = code
        open_ = open_ & ~cond

    mark(D == 0, 1)
    Dd = np.zeros_like(D)
    Dd[:-1] = D[1:]
    Dr = np.zeros_like(D)
    Dr[:, :-1] = D[:, 1:]
    mark((rr + 1 >= h) | (cc + 1 >= w) | (Dd == 0) | (Dr == 0), 2)
    dc, dcd, dcr = _dc(Ki, rr, cc), _dc(Ki, rr + 1, cc), _dc(Ki, rr, cc + 1)
    v = [(D * dc[i]).astype(f32) for i in range(3)]
    vd = [(Dd * dcd[i]).astype(f32) for i in range(3)]
    vr = [(Dr * dcr[i]).astype(f32) for i in range(3)]
    a = [(vd[i] - v[i]).astype(f32) for i in range(3)]
    b = [(vr[i] - v[i]).astype(f32) for i in range(3)]
    x = [((a[1] * b[2]).astype(f32) - (a[2] * b[1]).astype(f32)).astype(f32),
         ((a[2] * b[0]).astype(f32) - (a[0] * b[2]).astype(f32)).astype(f32),
         ((a[0] * b[1]).astype(f32) - (a[1] * b[0]).astype(f32)).astype(f32)]
    with np.errstate(all='ignore'):
        xx = _dot3(x, x)
        mark(~(xx > 0) | ~np.isfinite(xx), 2)
        xl = np.sqrt(xx).astype(f32)
        n = [(x[i] / xl).astype(f32) for i in range(3)]
        p = [(_dot3(R[i], v) + t[i]).astype(f32) for i in range(3)]
        nw = [_dot3(R[i], n) for i in range(3)]
        e = [(p[i] - tr[i]).astype(f32) for i in range(3)]
        q = [_dot3(Rr[:, i], e) for i in range(3)]
        mark(~(q[2] > 0), 3)
        ux = ((fx * (q[0] / q[2]).astype(f32)).astype(f32) + cx).astype(f32)
        uy = ((fy * (q[1] / q[2]).astype(f32)).astype(f32) + cy).astype(f32)
        fc = np.floor((ux + f32(0.5)).astype(f32))
        fr = np.floor((uy + f32(0.5)).astype(f32))
        mark(~((fc >= 0) & (fc < f32(w)) & (fr >= 0) & (fr < f32(h))), 4)
    mc = np.where(open_, fc, 0).astype(np.int64)
    mr = np.where(open_, fr, 0).astype(np.int64)
    dm = mdepth[mr, mc]
    mark(dm == 0, 5)
    dcm = _dc(Ki, mr, mc)
    mv = [(dm * dcm[i]).astype(f32) for i in range(3)]
    m = [(_dot3(Rr[i], mv) + tr[i]).astype(f32) for i in range(3)]
    g = [(p[i] - m[i]).astype(f32) for i in range(3)]
    with np.errstate(all='ignore'):
        mark(_dot3(g, g) > dist2, 6)
        nm = [mnormal[mr, mc, i] for i in range(3)]
        mark(_dot3(nw, nm) < cos_thr, 7)
    ok = open_
    rv = _dot3(nm, g)
    Jv = [((p[1] * nm[2]).astype(f32) - (p[2] * nm[1]).astype(f32)).astype(f32),
          ((p[2] * nm[0]).astype(f32) - (p[0] * nm[2]).astype(f32)).astype(f32),
          ((p[0] * nm[1]).astype(f32) - (p[1] * nm[0]).astype(f32)).astype(f32), nm[0], nm[1], nm[2]]
    for i in range(6):
        J[..., i] = np.where(ok, Jv[i], f32(0))
    res[:] = np.where(ok, rv, f32(0))
    if pixels:
        return J, res, reason, mr, mc
    return J, res, reason


def term_matrix(J, r, reason):
    """fp64 terms [n_inliers, 29] (exact products of the fp32 values) in the kernel's term order."""
    ok = reason.reshape(-1) == 0
    Jd = J.reshape(-1, 6)[ok].astype(np.float64)
    rd = r.reshape(-1)[ok].astype(np.float64)
    cols = [Jd[:, i] * Jd[:, j] for i in range(6) for j in range(i, 6)]
    cols += [Jd[:, i] * rd for i in range(6)]
    cols += [rd * rd, np.ones_like(rd)]
    return np.stack(cols, axis=1)


def rodrigues(w):
    """R_inc f64[3,3] of the rotation vector w, in the kernel's operation order."""
    w = [float(v) for v in w]
    th = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    if th < 1e-12:
        return np.array([[1.0, -w[2], w[1]], [w[2], 1.0, -w[0]], [-w[1], w[0], 1.0]])
    k = [w[0] / th, w[1] / th, w[2] / th]
    s, c = math.sin(th), 1.0 - math.cos(th)
    Kx = [[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]]
    R = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            dl = 1.0 if i == j else 0.0
            R[i, j] = (dl + s * Kx[i][j]) + c * (k[i] * k[j] - dl)
    return R


def cholesky_solve(A, b):
    """xi f64[6] of A·xi = b, or None when a pivot fails (d <= 1e-6·max diag) - the kernel's loop order."""
    A = [[float(A[i][j]) for j in range(6)] for i in range(6)]
    dmax = A[0][0]
    for j in range(1, 6):
        dmax = max(dmax, A[j][j])
    thr = 1e-6 * dmax
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        d = A[j][j]
        for k in range(j):
            d = d - L[j][k] * L[j][k]
        if not d > thr:
            return None
        L[j][j] = math.sqrt(d)
        for i in range(j + 1, 6):
            s = A[i][j]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            L[i][j] = s / L[j][j]
    y = [0.0] * 6
    for i in range(6):
        s = float(b[i])
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s / L[i][i]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * x[k]
        x[i] = s / L[i][i]
    return np.array(x)


def system(sums):
    """(A f64[6,6], b f64[6]) from the 29 sums."""
    A = np.empty((6, 6))
    e = 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = sums[e]
            e += 1
    return A, -np.asarray(sums[21:27], dtype=np.float64)


def step(sums, pose, min_count, moves=False):
    """(status code, new pose f64[3,4]) of one solve: the kernel's checks, Cholesky and left update.  ``moves``: also
    th = |omega| and |tau| as the stats row holds them (0 after a failed step)."""
    code, out, th, tau = _step(sums, pose, min_count)
    return (code, out, th, tau) if moves else (code, out)


def _step(sums, pose, min_count):
    sums = np.asarray(sums, dtype=np.float64)
    P = np.asarray(pose, dtype=np.float64).reshape(-1, 4)[:3]
    if sums[28] < min_count:
        return 1, P.copy(), 0.0, 0.0
    A, b = system(sums)
    x = cholesky_solve(A, b)
    if x is None:
        return 2, P.copy(), 0.0, 0.0
    if not np.isfinite(x).all():
        return 3, P.copy(), 0.0, 0.0
    Ri = rodrigues(x[:3])
    out = np.empty((3, 4))
    for i in range(3):
        for j in range(3):
            out[i, j] = Ri[i, 0] * P[0, j] + Ri[i, 1] * P[1, j] + Ri[i, 2] * P[2, j]
        out[i, 3] = (Ri[i, 0] * P[0, 3] + Ri[i, 1] * P[1, 3] + Ri[i, 2] * P[2, 3]) + x[3 + i]
    th = math.sqrt(float(x[0]) * float(x[0]) + float(x[1]) * float(x[1]) + float(x[2]) * float(x[2]))
    tau = math.sqrt(float(x[3]) * float(x[3]) + float(x[4]) * float(x[4]) + float(x[5]) * float(x[5]))
    return 0, out, th, tau


def schedule(iterations, levels):
    """The level of every step of a call, in launch order: levels - 1 down to 0, iterations[l] times each."""
    return [l for l in range(levels - 1, -1, -1) for _ in range(int(iterations[l]))]


def prefix_iterations(iterations, levels, k):
    """iterations_host of the call that runs only the first k steps of ``schedule(iterations, levels)``."""
    steps = schedule(iterations, levels)[:k]
    return [steps.count(l) for l in range(levels)]


def run(depth, mask, K, Kinv, mdepth, mnormal, E_ref, E_init, iterations, dist_thresh=0.1, angle_thresh=20.0, delta=0.03,
        min_inlier_fraction=0.05, trace=None):
    """The whole call (ojf_track): (pose f64[3,4], (code, iteration), stats f64[n,4]).  Kinv[l], mdepth[l], mnormal[l] per
    level, len(mdepth) levels; the pyramid once, then levels L-1 down to 0 and iterations[l] times associate -> sums ->
    step with min_count = min_inlier_fraction * h_l * w_l.  A failed step writes (s28, s27/s28 or 0, 0, 0), sets the
    status and puts the pose back to E_init; every later step is skipped and its stats row is 0.  The sums are numpy's
    (not the kernels' summation order).  ``trace``: a list that receives, per step that ran, dict(level, pose (before the
    step), reason, sums, code)."""
    levels = len(mdepth)
    E0 = np.asarray(E_init, np.float64).reshape(-1, 4)[:3].copy()
    pyr = pyramid(depth, mask, levels, delta)
    steps = schedule(iterations, levels)
    stats = np.zeros((len(steps), 4))
    P, status = E0.copy(), (0, -1)
    for it, l in enumerate(steps):
        if status[0]:
            continue
        J, r, reason = associate(pyr[l], Kinv[l], K, l, mdepth[l], mnormal[l], E_ref, P, dist_thresh, angle_thresh)
        with np.errstate(invalid='ignore'):
            sums = term_matrix(J, r, reason).sum(axis=0)
        code, Q, th, tau = _step(sums, P, float(min_inlier_fraction) * float(pyr[l].size))
        if trace is not None:
            trace.append(dict(level=l, pose=P.copy(), reason=reason, sums=sums, code=code))
        stats[it] = (sums[28], sums[27] / sums[28] if sums[28] > 0 else 0.0, th, tau)
        if code:
            status, P = (code, it), E0.copy()
        else:
            P = Q
    return P, status, stats


def pose_error(E, E_gt):
    """(translation error in m, rotation error in degrees) between two camera-to-world poses."""
    E = np.asarray(E, np.float64).reshape(-1, 4)[:3]
    G = np.asarray(E_gt, np.float64).reshape(-1, 4)[:3]
    dt = float(np.linalg.norm(E[:, 3] - G[:, 3]))
    c = (np.trace(E[:, :3].T @ G[:, :3]) - 1.0) / 2.0
    return dt, math.degrees(math.acos(min(1.0, max(-1.0, c))))


def perturb(E, rot_deg, trans_m, axis=(1.0, 0.0, 0.0), direction=(0.0, 1.0, 0.0)):
    """E with a left rotation of rot_deg about ``axis`` (about the camera centre) and a translation of trans_m."""
    E = np.asarray(E, np.float64).reshape(-1, 4)[:3]
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    R = rodrigues(a * math.radians(rot_deg))
    d = np.asarray(direction, np.float64) / np.linalg.norm(direction)
    out = E.copy()
    out[:, :3] = R @ E[:, :3]
    out[:, 3] = E[:, 3] + trans_m * d
    return out
