"""numpy restatement of the mesh distance field's definition in csrc/ojf_mesh_distance.hip (ojf_mesh_distance,
ojf_mesh_distance_sign): every fp32 operation is one numpy ufunc on float32 arrays (rounded on its own), every voxel is
tested against every triangle - no bricks, no bins, no lists.  Also a float64 brute-force distance by another route
(barycentric coordinates from the Gram matrix) that serves only as a yardstick, and the meshes of the tests."""
import numpy as np

from online_joint_depthfusion_and_semantic_amd.mesh_distance import pseudonormals
import raster_ref

F = np.float32
NO_KEY = np.uint64(0xffffffffffffffff)


def voxel_centres(origin, res, shape):
    """Three f32 arrays: the centres of the voxels on each axis, (float)(origin_m + (i + 0.5)·res) with the f64 product and sum."""
    origin = np.asarray(origin, np.float64).reshape(3)
    return [(origin[m] + (np.arange(shape[m]).astype(np.float64) + 0.5) * np.float64(res)).astype(F) for m in range(3)]


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _cross(u, v):
    return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]


def _sub(u, v):
    return [u[m] - v[m] for m in range(3)]


def prepare(vertices, faces):
    """Per face: ok (not skipped) and the header's a, b, c, e_0, e_1, e_2, n (lists of three f32[nf]), nn, ee (three f32[nf])."""
    vertices = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    ok = ((faces >= 0) & (faces < len(vertices))).all(axis=1)
    P = vertices[np.where(ok[:, None], faces, 0)]  # [nf, corner, xyz]
    ok &= np.isfinite(P).all(axis=(1, 2))
    P = np.where(ok[:, None, None], P, F(0))
    a, b, c = ([np.ascontiguousarray(P[:, i, m]) for m in range(3)] for i in range(3))
    with np.errstate(all='ignore'):
        e0, e1, e2, ac = _sub(b, a), _sub(c, b), _sub(a, c), _sub(c, a)
        n = _cross(e0, ac)
        T = dict(ok=ok, a=a, b=b, c=c, e0=e0, e1=e1, e2=e2, n=n, nn=_dot(n, n), ee=[_dot(e0, e0), _dot(e1, e1), _dot(e2, e2)])
    return T, faces


def _segment(w, e, ee):
    t = np.where(ee > 0, _dot(w, e) / ee, F(0))
    t = np.where(t < 0, F(0), t)
    t = np.where(t > 1, F(1), t)
    r = [w[m] - t * e[m] for m in range(3)]
    return _dot(r, r), t, r


def candidates(p, T, full=False):
    """The header's candidate order for points p (three broadcastable f32 arrays) against triangles T (dict of broadcastable
    arrays): d²; with ``full`` also (feature 0..3, t, r, h) of the winner."""
    w = [_sub(p, T['a']), _sub(p, T['b']), _sub(p, T['c'])]
    e = [T['e0'], T['e1'], T['e2']]
    best, t, r = _segment(w[0], e[0], T['ee'][0])
    feat = np.zeros(np.shape(best), np.int8) if full else None
    for k in (1, 2):
        s, tk, rk = _segment(w[k], e[k], T['ee'][k])
        m = s < best
        best = np.where(m, s, best)
        if full:
            feat = np.where(m, np.int8(k), feat)
            t = np.where(m, tk, t)
            r = [np.where(m, rk[i], r[i]) for i in range(3)]
    h = _dot(w[0], T['n'])
    f = [_dot(_cross(e[k], w[k]), T['n']) for k in range(3)]
    s3 = (h * h) / T['nn']
    m = (T['nn'] > 0) & (f[0] >= 0) & (f[1] >= 0) & (f[2] >= 0) & (s3 <= best)
    best = np.where(m, s3, best)
    if not full:
        return best
    return best, np.where(m, np.int8(3), feat), t, r, h


def distance_field(vertices, faces, origin, res, shape, band, elements=1 << 20):
    """(distance f32 [X,Y,Z], face i32 [X,Y,Z]) of the definition."""
    T, faces = prepare(vertices, faces)
    px, py, pz = voxel_centres(origin, res, shape)
    p = [px[None, :, None, None], py[None, None, :, None], pz[None, None, None, :]]
    band2 = F(band) * F(band)
    best = np.full(tuple(shape), NO_KEY, np.uint64)
    chunk = max(1, elements // int(np.prod(shape)))
    col = lambda v, s: v[s, None, None, None]  # noqa: E731
    with np.errstate(all='ignore'):
        for f0 in range(0, len(faces), chunk):
            s = slice(f0, f0 + chunk)
            Ts = {k: ([col(x, s) for x in v] if isinstance(v, list) else col(v, s)) for k, v in T.items()}
            d2 = np.ascontiguousarray(np.broadcast_to(candidates(p, Ts), (len(T['ok'][s]),) + tuple(shape)))
            reach = Ts['ok'] & (d2 <= band2)
            idx = np.arange(f0, f0 + d2.shape[0], dtype=np.uint64)[:, None, None, None]
            key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx
            best = np.minimum(best, np.where(reach, key, NO_KEY).min(axis=0))
        hit = best != NO_KEY
        d2 = (best >> np.uint64(32)).astype(np.uint32).view(F)
        distance = np.where(hit, np.sqrt(d2), F(np.inf)).astype(F)
    face = np.where(hit, (best & np.uint64(0xffffffff)).astype(np.int64), -1).astype(np.int32)
    return distance, face


def signed_distance(vertices, faces, origin, res, shape, distance, face):
    """signed f32 [X,Y,Z] of ojf_mesh_distance_sign's definition, from the outputs of ``distance_field``."""
    T, faces = prepare(vertices, faces)
    vn, en, fe = pseudonormals(vertices, faces)
    px, py, pz = voxel_centres(origin, res, shape)
    p = [np.broadcast_to(px[:, None, None], shape).ravel(), np.broadcast_to(py[None, :, None], shape).ravel(),
         np.broadcast_to(pz[None, None, :], shape).ravel()]
    f = face.ravel().astype(np.int64)
    inside = (f >= 0) & (f < len(faces))
    g = np.where(inside, f, 0)
    valid = inside & T['ok'][g]
    Tg = {k: ([x[g] for x in v] if isinstance(v, list) else v[g]) for k, v in T.items()}
    with np.errstate(all='ignore'):
        _, feat, t, r, h = candidates(p, Tg, full=True)
        k = np.where(feat < 3, feat, 0).astype(np.int64)
        corner = np.where(valid[:, None], faces[g], 0)
        at0, at1 = t == 0, t == 1
        vert = np.where(at0, corner[np.arange(len(g)), k], corner[np.arange(len(g)), (k + 1) % 3])
        N = np.where((at0 | at1)[:, None], vn[vert], en[fe[g, k]])
        s = np.where(feat == 3, h, _dot(r, [N[:, 0], N[:, 1], N[:, 2]]))
        d = distance.ravel()
        out = np.where(valid, np.where(s >= 0, d, -d), F(np.inf)).astype(F)
    return out.reshape(shape)


# ---- the float64 yardstick ------------------------------------------------------------------------------------------------
def distance_f64(points, vertices, faces, chunk=64):
    """min over the valid faces of the Euclidean distance from ``points`` f64 [n,3] to the triangle, in float64: the closest
    point from the barycentric coordinates of the projection (Gram matrix), else the nearest of the three edges."""
    vertices = np.asarray(vertices, np.float64).reshape(-1, 3)
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    ok = ((faces >= 0) & (faces < len(vertices))).all(axis=1)
    faces = faces[ok]
    faces = faces[np.isfinite(vertices[faces]).all(axis=(1, 2))]
    P = np.asarray(points, np.float64).reshape(-1, 3)
    best = np.full(len(P), np.inf)

    def seg(p, a, b):
        ab = b - a
        L = (ab * ab).sum(-1)
        t = np.clip(np.where(L > 0, ((p - a) * ab).sum(-1) / np.where(L > 0, L, 1.0), 0.0), 0.0, 1.0)
        return np.linalg.norm(p - (a + t[..., None] * ab), axis=-1)
    for f0 in range(0, len(faces), chunk):
        tri = vertices[faces[f0:f0 + chunk]]  # [c,3,3]
        a, b, c = tri[:, None, 0], tri[:, None, 1], tri[:, None, 2]
        p = P[None]
        d = np.minimum(np.minimum(seg(p, a, b), seg(p, b, c)), seg(p, c, a))
        u, v, w = b - a, c - a, p - a
        uu, uv, vv = (u * u).sum(-1), (u * v).sum(-1), (v * v).sum(-1)
        det = uu * vv - uv * uv
        with np.errstate(all='ignore'):
            wu, wv = (w * u).sum(-1), (w * v).sum(-1)
            s = (vv * wu - uv * wv) / det
            t = (uu * wv - uv * wu) / det
            inside = (det > 0) & (s >= 0) & (t >= 0) & (s + t <= 1)
            q = a + np.where(inside, s, 0.0)[..., None] * u + np.where(inside, t, 0.0)[..., None] * v
            d = np.where(inside, np.minimum(d, np.linalg.norm(p - q, axis=-1)), d)
        best = np.minimum(best, d.min(axis=0))
    return best


def centres_f64(origin, res, shape):
    """The voxel centres as the kernels see them (the fp32 values), as f64 [X·Y·Z, 3]."""
    px, py, pz = voxel_centres(origin, res, shape)
    g = np.meshgrid(px.astype(np.float64), py.astype(np.float64), pz.astype(np.float64), indexing='ij')
    return np.stack(g, axis=-1).reshape(-1, 3)


# ---- the meshes and boxes of the tests -------------------------------------------------------------------------------------
BOX_LO, BOX_HI = (-1.03, -0.77, -0.51), (0.93, 1.21, 0.67)


def closed_box(lo=BOX_LO, hi=BOX_HI):
    """A closed box with corners that are no round numbers, outward wound: 8 vertices, 12 triangles."""
    v, t = raster_ref._box(lo, hi)
    return dict(vertices=v.astype(F), faces=t.astype(np.int32), face_labels=np.arange(1, 13).astype(np.uint8))


def box_sdf(points, lo=BOX_LO, hi=BOX_HI):
    """Analytic signed distance to the box (positive outside) whose corners are the fp32 roundings of lo, hi."""
    lo, hi = np.asarray(lo, F).astype(np.float64), np.asarray(hi, F).astype(np.float64)
    q = np.abs(np.asarray(points, np.float64) - 0.5 * (lo + hi)) - 0.5 * (hi - lo)
    return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(axis=-1), 0.0)


def icosphere(level=2, radius=0.83, centre=(0.11, -0.07, 0.05)):
    """An icosahedron subdivided ``level`` times onto the sphere, outward wound: 20·4^level triangles."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                x = v[i] + v[j]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    verts = (np.array(v) * radius + np.asarray(centre)).astype(F)
    return dict(vertices=verts, faces=np.array(f, np.int32), face_labels=(1 + np.arange(len(f)) % 200).astype(np.uint8))


def fan(n=300, seed=5):
    """``n`` small triangles around the point (0.31, 0.27, 0.22), all inside one brick of a box at the origin with 0.1 m
    voxels, with random windings."""
    rng = np.random.default_rng(seed)
    c = np.array([0.31, 0.27, 0.22])
    verts = c + rng.uniform(-0.12, 0.12, (3 * n, 3))
    return dict(vertices=verts.astype(F), faces=np.arange(3 * n, dtype=np.int32).reshape(n, 3),
                face_labels=rng.integers(1, 255, n).astype(np.uint8))


BRICK = 8  # csrc/ojf_mesh_distance.hip: kBrick


def brick_counts(vertices, faces, origin, res, shape, band):
    """u32 [bricks] in the kernel's brick order: the (triangle, brick) pairs mesh_bin_kernel counts per brick - every brick of
    the box of voxels whose centres lie in the triangle's bounding box dilated by R (the header's f64 arithmetic).  Only for
    meshes whose brick boxes hold at most 8 bricks each: the larger ones go through a plane test that is not restated here."""
    origin, res, band = np.asarray(origin, np.float64).reshape(3), float(res), float(F(band))
    nb = [(s + BRICK - 1) // BRICK for s in shape]
    counts = np.zeros(nb, np.uint32)
    gmax = max(max(abs(origin[m]), abs(origin[m] + float(shape[m]) * res)) for m in range(3))
    T, faces = prepare(vertices, faces)
    for f in np.flatnonzero(T['ok']):
        P = np.asarray(vertices, F).reshape(-1, 3)[faces[f]].astype(np.float64)
        lo, hi = P.min(axis=0), P.max(axis=0)
        D, G = 0.0, gmax
        for m in range(3):
            D += hi[m] - lo[m]
            G = max(G, abs(lo[m]), abs(hi[m]))
        R = band + (1.0 / 262144.0) * ((G + D) + band)
        b = []
        for m in range(3):
            i0 = max(np.ceil(((lo[m] - R) - origin[m]) / res - 0.5), 0.0)
            i1 = min(np.floor(((hi[m] + R) - origin[m]) / res - 0.5), float(shape[m] - 1))
            if not i0 <= i1:
                break
            b.append(slice(int(i0) // BRICK, int(i1) // BRICK + 1))
        else:
            assert counts[tuple(b)].size <= 8, 'face {}: a brick box of the wave-wide tier'.format(f)
            counts[tuple(b)] += 1
    return counts.ravel()


SCAN_BRICKS = (1, 1023, 1024, 1025, 2049)  # chunks of 1, 1, 1, 2 and 3 counters per lane of the one-block scan (1024 lanes)
SCAN_BOX = dict(origin=np.zeros(3), res=0.1, band=0.15)


def scan_bricks(B):
    """The bricks of a (8·B, 8, 8) box that hold triangles in ``scan_mesh``: the first and the last, and the last counter of a
    scan lane's chunk with the first of the next lane's - behind lane 0, in the middle, and in front of the last lane with work."""
    chunk = (B + 1023) // 1024
    mid, last = (B // chunk // 2) * chunk, (B - 1) // chunk * chunk
    return sorted({b for b in (0, chunk - 1, chunk, mid - 1, mid, last - 1, last, B - 1) if 0 <= b < B})


def scan_mesh(B):
    """Small triangles about the centres of ``scan_bricks(B)`` of a box of (8·B, 8, 8) voxels of 0.1 m at the origin, 2, 3, 4, 2,
    ... to a brick, each within 0.1 m of the centre: with SCAN_BOX's band every one of them is binned to its own brick alone."""
    verts = []
    for i, b in enumerate(scan_bricks(B)):
        for j in range(2 + i % 3):
            c = np.array([0.8 * b + 0.4, 0.4, 0.4 + 0.06 * (j - 1.5)])  # (0.06 apart: each is the nearest of some voxel)
            verts += [c + (-0.05, -0.04, 0.0), c + (0.05, -0.03, 0.01), c + (0.0, 0.05, -0.01)]
    n = len(verts) // 3
    return dict(vertices=np.array(verts).astype(F), faces=np.arange(3 * n, dtype=np.int32).reshape(n, 3),
                face_labels=(1 + np.arange(n) % 200).astype(np.uint8))


ROOM32 = dict(shape=(32, 32, 32), band=0.24)


def room32_spec():
    """(origin, res) of the 32^3 grid over the room."""
    from online_joint_depthfusion_and_semantic_amd import synthetic
    origin, res, _ = synthetic.grid_spec(32)
    return origin, res


_CACHE = {}


def cached_field(name, mesh, origin, res, shape, band):
    """``distance_field`` of a named case, computed once per process; read-only."""
    if name not in _CACHE:
        out = distance_field(mesh['vertices'], mesh['faces'], origin, res, shape, band)
        for a in out:
            a.setflags(write=False)
        _CACHE[name] = out
    return _CACHE[name]
