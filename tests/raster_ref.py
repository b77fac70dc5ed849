"""numpy restatement of the mesh rasteriser's definition in csrc/ojf_raster.hip (ojf_rasterize, ojf_rasterize_attributes):
every fp32 operation is one numpy ufunc on float32 arrays (rounded on its own), every pixel is tested against every
triangle - no bounding boxes, no tiers.  Also the meshes and views of the GPU parity tests, so that a CPU test can show
they are not vacuous, and the CPU ground-truth composition (this file into projective_ref with carving)."""
import numpy as np

from online_joint_depthfusion_and_semantic_amd import synthetic
import projective_ref

F = np.float32
NO_KEY = np.uint64(0xffffffffffffffff)


def view_constants(K, E):
    """(R f32[3,3] with R[m][a] = E[4m+a], t f32[3], fx, fy, cx, cy) of one view."""
    K = np.asarray(K, np.float64).reshape(9)
    E = np.asarray(E, np.float64).reshape(-1)[:12]
    if not (K[1] == 0 and K[3] == 0 and K[6] == 0 and K[7] == 0 and K[8] == 1):
        raise ValueError('pinhole K expected')
    R = np.array([[E[4 * m + a] for a in range(3)] for m in range(3)]).astype(F)
    t = np.array([E[4 * m + 3] for m in range(3)]).astype(F)
    return R, t, F(K[0]), F(K[4]), F(K[2]), F(K[5])


def _cross(u, v):
    return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]


def _triangles(vertices, faces, R, t):
    """Per face: ok (not skipped), n0, n1, n2 (lists of three f32[nf]) and det f32[nf]."""
    nv = len(vertices)
    ok = ((faces >= 0) & (faces < nv)).all(axis=1)
    P = vertices[np.where(ok[:, None], faces, 0)]  # [nf, corner, xyz]
    ok &= np.isfinite(P).all(axis=(1, 2))
    d = [P[..., m] - t[m] for m in range(3)]
    cam = [(R[0, k] * d[0] + R[1, k] * d[1]) + R[2, k] * d[2] for k in range(3)]  # cam[k][face, corner]
    a, b, c = ([cam[k][:, i] for k in range(3)] for i in range(3))
    n0, n1, n2 = _cross(b, c), _cross(c, a), _cross(a, b)
    det = (a[0] * n0[0] + a[1] * n0[1]) + a[2] * n0[2]
    return ok, (n0, n1, n2), det


def _mesh_arrays(vertices, faces):
    vertices = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    return vertices, faces


def _views(K, E, n=None):
    E = np.asarray(E, np.float64)
    E = E.reshape((-1,) + E.shape[-2:])
    n = len(E) if n is None else n
    K = np.broadcast_to(np.asarray(K, np.float64).reshape(-1, 3, 3), (n, 3, 3))
    return K, np.broadcast_to(E, (n,) + E.shape[-2:])


def rasterize(vertices, faces, K, E, shape, near=0.0, chunk=512):
    """(depth f32 [n,h,w], face i32 [n,h,w]) of the definition; K [3,3] or [n,3,3], E [n,3|4,4] or one matrix."""
    vertices, faces = _mesh_arrays(vertices, faces)
    K, E = _views(K, E)
    h, w = shape
    near = F(near)
    depth = np.zeros((len(E), h, w), F)
    face = np.full((len(E), h, w), -1, np.int32)
    with np.errstate(all='ignore'):
        for v in range(len(E)):
            R, t, fx, fy, cx, cy = view_constants(K[v], E[v][:3])
            ok, n, det = _triangles(vertices, faces, R, t)
            rx = ((np.arange(w).astype(F) - cx) / fx)[None, None, :]
            ry = ((np.arange(h).astype(F) - cy) / fy)[None, :, None]
            best = np.full((h, w), NO_KEY, np.uint64)
            for f0 in range(0, len(faces), chunk):
                s = slice(f0, f0 + chunk)
                e = [(ni[0][s, None, None] * rx + ni[1][s, None, None] * ry) + ni[2][s, None, None] for ni in n]
                S = (e[0] + e[1]) + e[2]
                z = det[s, None, None] / S
                acc = ((e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0)) | ((e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0))
                acc &= (S != 0) & np.isfinite(z) & (z > near) & ok[s, None, None]
                idx = np.arange(f0, f0 + z.shape[0], dtype=np.uint64)[:, None, None]
                key = (np.ascontiguousarray(z).view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx
                best = np.minimum(best, np.where(acc, key, NO_KEY).min(axis=0))
            hit = best != NO_KEY
            depth[v] = np.where(hit, (best >> np.uint64(32)).astype(np.uint32).view(F), F(0))
            face[v] = np.where(hit, (best & np.uint64(0xffffffff)).astype(np.int64), -1).astype(np.int32)
    return depth, face


def attributes(vertices, faces, K, E, face, face_labels=None, vertex_colors=None):
    """(labels u8 [n,h,w] or None, rgba u8 [n,h,w,4] or None) of the definition's second pass over ``face`` i32 [n,h,w]."""
    vertices, faces = _mesh_arrays(vertices, faces)
    face = np.asarray(face, np.int32)
    nviews, h, w = face.shape
    K, E = _views(K, E, nviews)
    labels = None if face_labels is None else np.zeros((nviews, h, w), np.uint8)
    rgba = None if vertex_colors is None else np.zeros((nviews, h, w, 4), np.uint8)
    with np.errstate(all='ignore'):
        for v in range(nviews):
            R, t, fx, fy, cx, cy = view_constants(K[v], E[v][:3])
            ok, n, det = _triangles(vertices, faces, R, t)
            inside = (face[v] >= 0) & (face[v] < len(faces))
            f = np.where(inside, face[v], 0)
            hit = inside & ok[f]
            if labels is not None:
                labels[v] = np.where(hit, np.asarray(face_labels, np.uint8)[f], 0)
            if rgba is None:
                continue
            rx = np.broadcast_to(((np.arange(w).astype(F) - cx) / fx)[None, :], (h, w))
            ry = np.broadcast_to(((np.arange(h).astype(F) - cy) / fy)[:, None], (h, w))
            e = [(ni[0][f] * rx + ni[1][f] * ry) + ni[2][f] for ni in n]
            S = (e[0] + e[1]) + e[2]
            lam = [ei / S for ei in e]
            col = np.asarray(vertex_colors, np.uint8)[np.where(ok[:, None], faces, 0)][f]  # [h, w, corner, channel]
            for k in range(3):
                ck = (lam[0] * col[..., 0, k].astype(F) + lam[1] * col[..., 1, k].astype(F)) + lam[2] * col[..., 2, k].astype(F)
                byte = np.fmin(np.fmax(np.floor(ck + F(0.5)), F(0)), F(255))  # (fmax / fmin: a NaN gives 0)
                rgba[v, ..., k] = np.where(hit, byte, 0).astype(np.uint8)
            rgba[v, ..., 3] = np.where(hit, 255, 0)
    return labels, rgba


# ---- the meshes and views of the parity tests ----------------------------------------------------------------------------
def _box(lo, hi):
    """8 corners (index = 4·ix + 2·iy + iz) and 12 triangles, two per side, listed side by side: (axis, low | high)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    verts = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]  # x-, x+, y-, y+, z-, z+
    tris = [t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))]
    return verts, np.array(tris, np.int64)


def room_mesh():
    """The box room of synthetic.py and its three solids, one closed box each: 32 vertices, 48 triangles (room first).
    ``face_labels`` are the surface ids of synthetic._raycast: 1 + 2·axis + (the high side) for the room's walls, 7 + s for
    solid s.  (The sides of a solid that lie in a wall are part of its box; no ray from inside the room reaches them
    before it reaches the solid.)  Vertex colours: a seeded random colour per vertex."""
    verts, faces, labels = [], [], []
    boxes = [(synthetic.ROOM_MIN, synthetic.ROOM_MAX)] + list(synthetic._SOLIDS)
    for s, (lo, hi) in enumerate(boxes):
        v, t = _box(lo, hi)
        faces.append(t + 8 * s)
        verts.append(v)
        labels += [1 + 2 * (q // 2) + (q % 2) for q in range(6) for _ in (0, 1)] if s == 0 else [6 + s] * 12
    colors = np.random.default_rng(11).integers(0, 256, (8 * len(boxes), 4)).astype(np.uint8)
    return dict(vertices=np.concatenate(verts).astype(F), faces=np.concatenate(faces).astype(np.int32),
                face_labels=np.array(labels, np.uint8), vertex_colors=colors)


def orbit_poses(n, frames=40):
    """The poses of synthetic.SyntheticStream(.., n_frames <= 40): camera-to-world f64 [n,3,4]."""
    return np.stack([synthetic.camera_pose(2.0 * np.pi * i / frames) for i in range(n)])


PATCH_SHAPE = (48, 64)
PATCH_K = np.array([[40.0, 0.0, 31.5], [0.0, 40.0, 23.5], [0.0, 0.0, 1.0]])
PATCH_E = np.array([[1.0, 0.0, 0.0, 0.1], [0.0, 1.0, 0.0, -0.05], [0.0, 0.0, 1.0, -2.0]])


def bumpy_patch(quads=60, seed=7):
    """A quads x quads height field over [-1.4, 1.4] x [-1.05, 1.05] around the plane z = 0, seen from PATCH_E at 48 x 64
    with PATCH_K: a quad covers less than a pixel (0.93 x 0.7), the patch about 56 x 42 pixels inside the image.  Every
    quad is cut along one of its two diagonals and every triangle wound one of the two ways, both at random (seeded)."""
    rng = np.random.default_rng(seed)
    x = np.linspace(-1.4, 1.4, quads + 1)
    y = np.linspace(-1.05, 1.05, quads + 1)
    X, Y = np.meshgrid(x, y, indexing='ij')
    Z = 0.06 * np.sin(5.0 * X) * np.cos(4.0 * Y) + 0.01 * rng.standard_normal(X.shape)
    verts = np.stack([X, Y, Z], axis=-1).reshape(-1, 3)
    vid = lambda i, j: i * (quads + 1) + j  # noqa: E731
    tris = []
    for i in range(quads):
        for j in range(quads):
            q = (vid(i, j), vid(i + 1, j), vid(i + 1, j + 1), vid(i, j + 1))
            pair = ((q[0], q[1], q[2]), (q[0], q[2], q[3])) if rng.random() < 0.5 else ((q[0], q[1], q[3]), (q[1], q[2], q[3]))
            for t in pair:
                tris.append(t if rng.random() < 0.5 else (t[0], t[2], t[1]))
    labels = rng.integers(1, 30, len(tris)).astype(np.uint8)
    colors = rng.integers(0, 256, (len(verts), 4)).astype(np.uint8)
    return dict(vertices=verts.astype(F), faces=np.array(tris, np.int32), face_labels=labels, vertex_colors=colors, quads=quads)


def patch_footprint(mesh):
    """Pixels (bool [48,64]) that lie inside the patch's outline by more than a pixel: between the innermost projections
    of its four border rows of vertices (f64)."""
    q = mesh['quads'] + 1
    cam = mesh['vertices'].astype(np.float64).reshape(q, q, 3) - PATCH_E[:, 3]
    u = PATCH_K[0, 0] * cam[..., 0] / cam[..., 2] + PATCH_K[0, 2]
    v = PATCH_K[1, 1] * cam[..., 1] / cam[..., 2] + PATCH_K[1, 2]
    c = np.arange(PATCH_SHAPE[1])[None, :]
    r = np.arange(PATCH_SHAPE[0])[:, None]
    return (c >= u[0].max() + 1) & (c <= u[-1].min() - 1) & (r >= v[:, 0].max() + 1) & (r <= v[:, -1].min() - 1)


EDGE_SHAPE = (37, 53)
EDGE_K = np.array([[32.0, 0.0, -3.5], [0.0, 32.0, 18.0], [0.0, 0.0, 1.0]])  # the principal point lies left of the image
EDGE_E = np.array([[1.0, 0.0, 0.0, 0.5], [0.0, 1.0, 0.0, -0.25], [0.0, 0.0, 1.0, 0.0]])  # d = P - t and a = d are exact
EDGE_FACES = {'background': (0, 1), 'crossing': (2,), 'behind': (3,), 'zero_area': (4,), 'edge_on': (5,), 'pixel_centres': (6,),
              'duplicate': (7, 8), 'out_of_range': (9, 10), 'nan_vertex': (11,)}


def edge_cases():
    """One mesh with a triangle (or two) for each case of EDGE_FACES, given in camera coordinates of EDGE_E (identity
    rotation, a translation that fp32 subtracts exactly); ray directions of the image: rx 0.11..1.73, ry -0.56..0.56."""
    ray = lambda c, r, z: (z * (c + 3.5) / 32.0, z * (r - 18.0) / 32.0, z)  # noqa: E731  (exact in fp32 for z a power of two)
    cam, faces = [], []

    def tri(*pts):
        faces.append(tuple(range(len(cam), len(cam) + 3)))
        cam.extend(pts)
    cam.extend([(0.0, -3.0, 4.0), (6.0, -3.0, 4.0), (6.0, 1.0, 4.0), (0.0, 1.0, 4.0)])  # background: rows up to 26 at z = 4
    faces.extend([(0, 1, 2), (0, 2, 3)])
    tri((0.2, -0.5, 3.0), (2.5, -0.5, 3.0), (1.0, 0.4, -1.0))  # 2: one vertex behind the camera plane
    tri((0.2, -1.0, -2.0), (2.0, -1.0, -2.0), (1.0, 1.0, -2.0))  # 3: wholly behind
    cam.extend([(0.3, -0.2, 0.5), (0.8, 0.2, 0.5)])  # 4: zero area, a repeated vertex, in front of everything
    faces.append((len(cam) - 2, len(cam) - 2, len(cam) - 1))
    tri((0.2, 0.1, 1.0), (0.9, -0.2, 2.0), (1.1, -0.1, 3.0))  # 5: c = a + b, its plane holds the camera centre
    tri(ray(10, 5, 2.0), ray(20, 5, 2.0), ray(10, 12, 2.0))  # 6: vertices on the centres of pixels (5,10), (5,20), (12,10)
    tri(ray(30, 20, 1.0), ray(45, 22, 1.0), ray(33, 33, 1.0))  # 7, 8: the same three vertices twice
    faces.append(faces[-1])
    faces.extend([(0, 1, len(cam) + 40), (-1, 0, 1)])  # 9, 10: an index past the end, a negative index
    tri((0.2, -0.3, 0.25), (1.5, -0.3, 0.25), (np.nan, 0.3, 0.25))  # 11: a NaN vertex, nearer than everything
    verts = (np.array(cam, np.float64) + EDGE_E[:, 3]).astype(F)
    on_centres = np.array(faces[6])
    assert np.array_equal(verts[on_centres].astype(np.float64) - EDGE_E[:, 3], np.array(cam)[on_centres])  # (no rounding there)
    rng = np.random.default_rng(3)
    return dict(vertices=verts, faces=np.array(faces, np.int32), face_labels=np.arange(1, len(faces) + 1).astype(np.uint8),
                vertex_colors=rng.integers(0, 256, (len(verts), 4)).astype(np.uint8))


# ---- the ground-truth composition on the CPU -------------------------------------------------------------------------------
def fuse_ground_truth(depth, labels, K, E, origin, res, shape, trunc, max_weight=128.0):
    """What rasterize.ground_truth_grid does with rasterised views, in numpy: projective_ref.fuse with carve from fresh
    volumes, then -trunc / label 0 where no view reached.  Returns (tsdf f16, labels u8, weights f16)."""
    tsdf = np.full(shape, trunc, np.float16)
    weights = np.zeros(shape, np.float16)
    ids = np.zeros(shape, np.uint8)
    scores = np.zeros(shape, np.float16)
    projective_ref.fuse(tsdf, weights, origin, res, depth, K, E, None, ids, scores, labels, None, trunc=trunc,
                        max_weight=max_weight, carve=True)
    unseen = weights == 0
    tsdf[unseen] = -trunc
    ids[unseen] = 0
    return tsdf, ids, weights


ROOM_H, ROOM_W, ROOM_GRID, ROOM_FRAMES, ROOM_TRUNC = 48, 64, 64, 20, 0.24
_ROOM = {}


def room_views():
    """The room mesh rasterised at the 20 orbit poses at 48 x 64, once: dict(mesh, K, E, depth, face, labels)."""
    if 'views' not in _ROOM:
        mesh = room_mesh()
        K, E = synthetic.intrinsics(ROOM_H, ROOM_W), orbit_poses(ROOM_FRAMES)
        depth, face = rasterize(mesh['vertices'], mesh['faces'], K, E, (ROOM_H, ROOM_W))
        labels, _ = attributes(mesh['vertices'], mesh['faces'], K, E, face, mesh['face_labels'])
        for a in (depth, face, labels):
            a.setflags(write=False)
        _ROOM['views'] = dict(mesh=mesh, K=K, E=E, depth=depth, face=face, labels=labels)
    return _ROOM['views']


def room_ground_truth():
    """The CPU ground-truth composition of the room into 64^3 (once): (tsdf, labels, weights), read-only."""
    if 'gt' not in _ROOM:
        v = room_views()
        origin, res, _ = synthetic.grid_spec(ROOM_GRID)
        out = fuse_ground_truth(v['depth'], v['labels'], v['K'], v['E'], origin, res, (ROOM_GRID,) * 3, ROOM_TRUNC)
        for a in out:
            a.setflags(write=False)
        _ROOM['gt'] = out
    return _ROOM['gt']
