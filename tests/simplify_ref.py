"""Normative restatement of csrc/ojf_simplify.hip in numpy: vertex clustering of a triangle mesh with quadric
error metrics.  The GPU tests hold the kernels to this module bit for bit; the host tests prove this module right from
properties that do not depend on the kernels.

Definition (vertices f32[nv,3], faces i32[nf,3], lo f32[3], cell f32 > 0, G = (GX, GY, GZ); fp32 unless stated, every operation
rounded on its own):

1. CELL.  Per axis t = (v - lo) / cell, g = floor(t).  A vertex is VALID when all three t are finite and 0 <= g < G; its cell
   index is (gx GY + gy) GZ + gz, -1 when invalid.
2. CLUSTERS.  The occupied cells in ascending cell index are the output vertices 0..nc-1; cluster[v] = that rank, or -1.
3. LOCAL POSITION.  p = clamp(rint(((t - g) - 0.5) 256), -128, 128) per axis: integers, 1/256 cell around the cell centre.
   Per cluster the exact integer sums S (3) and cnt over its valid vertices.
4. FACE QUADRIC.  A face COUNTS when its three indices are in [0, nv), its three vertices are valid and, with the world
   positions q0, q1, q2 of its corners as listed, e1 = q1 - q0, e2 = q2 - q0,
   N = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), L2 = (Nx Nx + Ny Ny) + Nz Nz is finite and > 0.  Then
   L = sqrt(L2), n_i = (int)clamp(rint(N_i / L 512), -512, 512), w = (int)clamp(rint(((0.5 L) / (cell cell)) 1024), 1, 1024)
   (the clamps in fp32, before the conversion).  For each corner k, into cluster[v_k], with that corner's local p:
   d = -(n . p), A += w n n^T (00 01 02 11 12 22), b += w d n - integers, once per corner, not once per distinct cluster.
5. REPRESENTATIVE, in f64, every operation rounded, integers converted to f64 first (to nearest even):
   lam = ((A00 + A11 + A22) >> 10) + 1 (integer), m_a = S_a / cnt, M = A with lam added on the diagonal,
   r_a = lam m_a - b_a; cofactors c00 = M11 M22 - M12 M12, c01 = M02 M12 - M01 M22, c02 = M01 M12 - M02 M11,
   c11 = M00 M22 - M02 M02, c12 = M01 M02 - M00 M12, c22 = M00 M11 - M01 M01; det = (M00 c00 + M01 c01) + M02 c02;
   x0 = ((c00 r0 + c01 r1) + c02 r2) / det, x1 = ((c01 r0 + c11 r1) + c12 r2) / det, x2 = ((c02 r0 + c12 r1) + c22 r2) / det.
   Unless det is finite and > 0 and every |x_a| <= 256: x = m.
   position_a = (float)(lo_a + ((g_a + 0.5) + x_a / 256) cell).
6. SOURCE.  source[c] = low word of the minimum over the members v of c of (bits(d2) << 32) | v,
   d2 = (dx dx + dy dy) + dz dz in fp32, dx = v_x - position_x etc.
7. FACES.  Face f becomes (cluster[v0], cluster[v1], cluster[v2]), kept when it counts and the three clusters differ; kept faces
   in input order; face_source[j] = the input face.

unique_faces (the Python layer's option): every kept face rotated to start at its smallest index (orientation kept), the distinct
triples in ascending lexicographic order, face_source = the smallest input face among the repeats.

default_grid: lo_a = floor(min_a / cell) cell in fp32, minus cell if that is still above min_a; G_a = floor((max_a - lo_a) / cell) + 1.
"""
import collections

import numpy as np

f32 = np.float32
POS_MAX, NORMAL_MAX, WEIGHT_MAX = 128, 512, 1024
MAX_FACES = 1 << 24

Simplified = collections.namedtuple('Simplified', 'vertices faces source face_source cluster cell A b S cnt x')
Simplified.__doc__ = """vertices f32[nc,3], faces i32[nk,3], source i32[nc], face_source i32[nk]; for the tests: cluster i32[nv],
cell i64[nc] (cell index of every cluster), the integer sums A i64[nc,6], b i64[nc,3], S i64[nc,3], cnt i64[nc] and x f64[nc,3],
the representative in 1/256 cell around the cell centre."""


def default_grid(vmin, vmax, cell):
    """(lo f32[3], G) the Python layer uses when none is given: finite vmin <= vmax."""
    cell = f32(cell)
    vmin, vmax = np.asarray(vmin, f32), np.asarray(vmax, f32)
    lo = np.floor(vmin / cell) * cell
    lo = np.where(lo > vmin, lo - cell, lo).astype(f32)
    G = tuple(int(v) + 1 for v in np.floor((vmax - lo) / cell))
    return lo, G


def locate(vertices, lo, cell, G):
    """Steps 1 and 3: (cell index i64[nv] or -1, p i64[nv,3])."""
    v = np.asarray(vertices, f32).reshape(-1, 3)
    lo, cell = np.asarray(lo, f32).reshape(1, 3), f32(cell)
    with np.errstate(all='ignore'):
        t = (v - lo) / cell
        g = np.floor(t)
        valid = (np.isfinite(t) & (g >= 0) & (g < np.asarray(G, np.float64)[None])).all(axis=1)
        p = np.clip(np.rint(((t - g) - f32(0.5)) * f32(256.0)), f32(-POS_MAX), f32(POS_MAX))
    assert t.dtype == f32 and p.dtype == f32
    gi = np.where(valid[:, None], g, 0).astype(np.int64)
    idx = (gi[:, 0] * G[1] + gi[:, 1]) * G[2] + gi[:, 2]
    idx[~valid] = -1
    return idx, np.where(valid[:, None], p, 0).astype(np.int64)


def face_terms(vertices, faces, valid, cell):
    """Step 4 without the corners: (counts bool[nf], n i64[nf,3], w i64[nf])."""
    v = np.asarray(vertices, f32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    cell = f32(cell)
    nv = v.shape[0]
    inside = ((faces >= 0) & (faces < nv)).all(axis=1)
    safe = np.where(inside[:, None], faces, 0)
    counts = inside & valid[safe].all(axis=1)
    q = v[safe]
    with np.errstate(all='ignore'):
        e1, e2 = q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]
        N = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        L2 = (N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2]
        counts &= np.isfinite(L2) & (L2 > 0)
        L = np.sqrt(np.where(counts, L2, f32(1.0)))
        n = np.clip(np.rint(N / L[:, None] * f32(512.0)), f32(-NORMAL_MAX), f32(NORMAL_MAX))
        w = np.clip(np.rint(f32(0.5) * L / (cell * cell) * f32(1024.0)), f32(1.0), f32(WEIGHT_MAX))
    assert N.dtype == f32 and L.dtype == f32 and n.dtype == f32 and w.dtype == f32
    n = np.where(counts[:, None], n, 0).astype(np.int64)
    w = np.where(counts, w, 0).astype(np.int64)
    return counts, n, w


def solve(A, b, S, cnt):
    """Step 5 up to x: f64[nc,3] in 1/256 cell around the cell centre."""
    A, b, S, cnt = (np.asarray(a, np.int64) for a in (A, b, S, cnt))
    lam = (((A[:, 0] + A[:, 3] + A[:, 5]) >> 10) + 1).astype(np.float64)
    Af, bf = A.astype(np.float64), b.astype(np.float64)
    with np.errstate(all='ignore'):
        m = S.astype(np.float64) / cnt.astype(np.float64)[:, None]
        M00, M01, M02, M11, M12, M22 = Af[:, 0] + lam, Af[:, 1], Af[:, 2], Af[:, 3] + lam, Af[:, 4], Af[:, 5] + lam
        r0, r1, r2 = lam * m[:, 0] - bf[:, 0], lam * m[:, 1] - bf[:, 1], lam * m[:, 2] - bf[:, 2]
        c00, c01, c02 = M11 * M22 - M12 * M12, M02 * M12 - M01 * M22, M01 * M12 - M02 * M11
        c11, c12, c22 = M00 * M22 - M02 * M02, M01 * M02 - M00 * M12, M00 * M11 - M01 * M01
        det = (M00 * c00 + M01 * c01) + M02 * c02
        x = np.stack([((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det,
                      ((c02 * r0 + c12 * r1) + c22 * r2) / det], axis=1)
        ok = np.isfinite(det) & (det > 0) & (np.abs(x) <= 256.0).all(axis=1)
    return np.where(ok[:, None], x, m)


def cluster(vertices, faces, lo, cell, G):
    """The whole definition: a ``Simplified``."""
    v = np.ascontiguousarray(np.asarray(vertices, f32).reshape(-1, 3))
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    lo, cell = np.asarray(lo, f32).reshape(3), f32(cell)
    G = tuple(int(g) for g in G)
    nv, nf = v.shape[0], faces.shape[0]
    assert nf <= MAX_FACES and min(G) >= 1 and G[0] * G[1] * G[2] < 2 ** 31 and cell > 0 and np.isfinite(cell)
    idx, p = locate(v, lo, cell, G)
    valid = idx >= 0
    cells = np.unique(idx[valid])
    nc = cells.shape[0]
    clus = np.where(valid, np.searchsorted(cells, idx), -1).astype(np.int64)
    S, cnt = np.zeros((nc, 3), np.int64), np.zeros(nc, np.int64)
    np.add.at(S, clus[valid], p[valid])
    np.add.at(cnt, clus[valid], 1)
    counts, n, w = face_terms(v, faces, valid, cell)
    A, b = np.zeros((nc, 6), np.int64), np.zeros((nc, 3), np.int64)
    rows = np.flatnonzero(counts)
    fn, fw = n[rows], w[rows]
    quad = fw[:, None] * np.stack([fn[:, 0] * fn[:, 0], fn[:, 0] * fn[:, 1], fn[:, 0] * fn[:, 2], fn[:, 1] * fn[:, 1],
                                   fn[:, 1] * fn[:, 2], fn[:, 2] * fn[:, 2]], axis=1)
    for k in range(3):
        corner = faces[rows, k]
        d = -(fn * p[corner]).sum(axis=1)
        np.add.at(A, clus[corner], quad)
        np.add.at(b, clus[corner], (fw * d)[:, None] * fn)
    x = solve(A, b, S, cnt)
    g = np.stack([cells // (G[1] * G[2]), (cells // G[2]) % G[1], cells % G[2]], axis=1).astype(np.float64)
    pos = (lo.astype(np.float64)[None] + ((g + 0.5) + x / 256.0) * np.float64(cell)).astype(f32)
    with np.errstate(all='ignore'):
        dlt = v[valid] - pos[clus[valid]]
        d2 = (dlt[:, 0] * dlt[:, 0] + dlt[:, 1] * dlt[:, 1]) + dlt[:, 2] * dlt[:, 2]
    assert d2.dtype == f32
    key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.flatnonzero(valid).astype(np.uint64)
    best = np.full(nc, np.iinfo(np.uint64).max, np.uint64)
    np.minimum.at(best, clus[valid], key)
    source = (best & np.uint64(0xffffffff)).astype(np.int64).astype(np.int32)
    fc = np.where(counts[:, None], clus[np.where(counts[:, None], faces, 0)], -1)
    kept = counts & (fc[:, 0] != fc[:, 1]) & (fc[:, 1] != fc[:, 2]) & (fc[:, 0] != fc[:, 2])
    return Simplified(pos, fc[kept].astype(np.int32), source, np.flatnonzero(kept).astype(np.int32), clus.astype(np.int32), cells, A, b,
                      S, cnt, x)


def unique_faces(faces, face_source):
    """The Python layer's ``unique_faces``: (faces, face_source)."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    if faces.shape[0] == 0:
        return faces.astype(np.int32), np.asarray(face_source, np.int32).reshape(0)
    first = faces.argmin(axis=1)
    rot = np.stack([faces[np.arange(len(faces)), (first + k) % 3] for k in range(3)], axis=1)
    uniq, inverse = np.unique(rot, axis=0, return_inverse=True)
    src = np.full(uniq.shape[0], np.iinfo(np.int64).max, np.int64)
    np.minimum.at(src, inverse.reshape(-1), np.asarray(face_source, np.int64))
    return uniq.astype(np.int32), src.astype(np.int32)


# ---- meshes for the tests --------------------------------------------------------------------------------------------
def weld(tri):
    """Indexed mesh of a triangle list f32[T,3,3]: bit-equal vertices merge (sorted), collapsed faces go."""
    verts, inverse = np.unique(np.asarray(tri, f32).reshape(-1, 3), axis=0, return_inverse=True)
    faces = inverse.reshape(-1, 3)
    keep = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
    return verts, faces[keep].astype(np.int32)


def tessellated_cube(step_inv=32):
    """The unit cube [0,1]^3 with every face cut into step_inv^2 squares of two triangles, outward normals, welded; every
    coordinate is a multiple of 1 / step_inv (exact in fp32)."""
    n = step_inv
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    i, j = i.ravel().astype(np.float64), j.ravel().astype(np.float64)
    tris = []
    for axis in range(3):
        for side in (0, 1):
            u, w = (axis + 1) % 3, (axis + 2) % 3

            def pt(a, b):
                q = np.zeros((len(i), 3))
                q[:, axis], q[:, u], q[:, w] = side, a / n, b / n
                return q
            q00, q10, q11, q01 = pt(i, j), pt(i + 1, j), pt(i + 1, j + 1), pt(i, j + 1)
            quads = [(q00, q10, q11), (q00, q11, q01)] if side else [(q00, q11, q10), (q00, q01, q11)]
            tris += [np.stack(t, axis=1) for t in quads]
    return weld(np.concatenate(tris, axis=0).astype(f32))


def random_mesh(seed, nv, nf, span=4.0):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0, span, (nv, 3)).astype(f32)), rng.integers(0, nv, (nf, 3)).astype(np.int32)


def signed_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float((a * np.cross(b, c)).sum() / 6.0)


def directed_edge_balance(faces):
    """Number of directed edges a->b that do not occur as often as b->a (0 for a closed oriented surface)."""
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], axis=0)
    n = int(e.max()) + 1 if len(e) else 1
    fwd = collections.Counter((e[:, 0] * n + e[:, 1]).tolist())
    return sum(1 for k, c in fwd.items() if fwd.get((k % n) * n + k // n, 0) != c)


def weld_keys(tri, keys, labels=None):
    """mesh.weld with the extractor's edge keys, restated: vertices in ascending key order, faces in list order."""
    uniq, first, inverse = np.unique(np.asarray(keys).reshape(-1), return_index=True, return_inverse=True)
    verts = np.asarray(tri, f32).reshape(-1, 3)[first]
    vlab = None if labels is None else np.asarray(labels).reshape(-1)[first]
    return verts, inverse.reshape(-1, 3).astype(np.int32), vlab


def closed_cases(n=32):
    """(name, fp16 volume) of the closed surfaces the host tests simplify: a sphere and the analytic fixture's torus at n^3 = 32^3."""
    import json
    import os
    g = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing='ij'), axis=-1).astype(np.float64)
    yield 'sphere', np.clip(np.linalg.norm(g - (15.5 + 0.137), axis=-1) - 10.3, -4, 4).astype(np.float16)
    cases = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'mesh_analytic_cases.json')))['cases']
    torus = [k for k in cases if k['name'] == 'torus'][0]  # the fixture is stated for 64^3: half of every length
    q = g - np.asarray(torus['centre']) / 2
    ring = np.sqrt(q[..., 0] ** 2 + q[..., 1] ** 2) - torus['R'] / 2
    yield 'torus', np.clip(np.sqrt(ring ** 2 + q[..., 2] ** 2) - torus['r'] / 2, -4, 4).astype(np.float16)
