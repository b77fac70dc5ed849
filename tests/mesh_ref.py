"""Normative restatement of csrc/ojf_mesh.hip in numpy: the ordered triangle list of ``ojf_mesh_extract`` and the
brute-force statement of ``ojf_points_within``.  The GPU tests hold the kernels to this module bit for bit; the host
tests prove this module right from properties that do not depend on the kernel.

Definition of the triangle list (volume ``v`` fp16[X,Y,Z], optional weights fp16, optional ids u8, iso fp32, origin f64[3],
res f64):

* CELL (i,j,k), 0 <= i < X-1 etc., has the corners c = 0..7 at (i,j,k) + CORNER[c].  It is VALID when every corner value is
  non-NaN and, with weights, fp32(weight) > 0 at every corner (NaN, negative and -0 weights are unobserved; the smallest
  subnormal is observed).  Invalid cells emit nothing.
* INSIDE: corner c is inside when fp32(v) < iso in fp32.  A value equal to iso is outside; so is -0 at iso 0.
* ORDER of the list: x index i, then y tile j // 4, then z tile k // 64 (these three number the BLOCK,
  (i * gy + j // 4) * gz + k // 64 with (gz, gy, gx) = blocks(shape)), then j % 4, then k % 64, then the tetrahedron
  0..5 of TETS, then the triangle 0..1 of the tetrahedron.
* TETRAHEDRON with the local corners 0..3 = TETS[t]: n_in inside corners.  0 or 4: nothing.  The MINORITY side is the inside
  corners when n_in <= 2, else the outside ones; a = minority corners, b = the others, both in local order.
  one corner (|a| = 1): one triangle on the edges (a0,b0), (a0,b1), (a0,b2).
  two against two: the quad q0..q3 on the edges (a0,b0), (a0,b1), (a1,b1), (a1,b0), split along q0-q2 into (q0,q1,q2) and
  (q0,q2,q3).
* CROSSING of an edge, in voxel-index coordinates, taken from the lower-valued end (p0, v0) towards (p1, v1):
  t = (iso - v0) / (v1 - v0), p = p0 + t * (p1 - p0), every operation rounded to fp32 (no contraction, correctly rounded
  division).  The same edge therefore gives the same bits in every tetrahedron and cell that shares it.
* WINDING: dir = (last outside local corner) - (last inside local corner), n = (B - A) x (C - A) as
  nx = u1*w2 - u2*w1, ny = u2*w0 - u0*w2, nz = u0*w1 - u1*w0, dot = (nx*dir0 + ny*dir1) + nz*dir2, all fp32 with every
  operation rounded.  Vertices 1 and 2 swap when dot < 0 and only then (a dot of +-0 keeps the order).
* WORLD position: fp32(origin + f64(p) * res), product and sum rounded to f64 one after the other.
* LABEL: ids[rint(p)], ties to even on the fp32 index coordinates.
* KEY: 8 * lin(lower corner of the edge) + direction bits (bit a set: the edge advances on axis a), lin = (x*Y + y)*Z + z.
* +-inf voxels are outside this definition: the kernel treats them as observed and the crossing parameter becomes NaN.

The scan turns the per-block counts into their exclusive prefix; the workspace holds it after the call.
"""
import collections

import numpy as np

KUHN_DIRS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]
CORNER = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]])
TETS = [(0, 5, 1, 6), (0, 1, 2, 6), (0, 2, 3, 6), (0, 3, 7, 6), (0, 7, 4, 6), (0, 4, 5, 6)]
TILE_Y, TILE_Z = 4, 64


# ---- the helpers test_mesh_gpu.py has always used (count and vertex SET of the same level set) -------------------------
def np_triangle_count(vol, iso, valid):
    """Triangles marching tetrahedra emit: per tetrahedron 1 (one corner apart) or 2 (two against two)."""
    X, Y, Z = vol.shape
    inside = vol < iso
    corner = [inside[c[0]:X - 1 + c[0], c[1]:Y - 1 + c[1], c[2]:Z - 1 + c[2]].astype(np.int64) for c in CORNER]
    total = 0
    for t in TETS:
        k = sum(corner[c] for c in t)
        total += int(((((k == 1) | (k == 3)) * 1 + (k == 2) * 2) * valid).sum())
    return total


def np_cell_valid(vol, weights):
    X, Y, Z = vol.shape
    ok = ~np.isnan(vol)
    if weights is not None:
        ok &= weights > 0
    valid = np.ones((X - 1, Y - 1, Z - 1), dtype=bool)
    for c in CORNER:
        valid &= ok[c[0]:X - 1 + c[0], c[1]:Y - 1 + c[1], c[2]:Z - 1 + c[2]]
    return valid


def np_vertex_set(vol, iso, valid, origin, res):
    """Unique surface vertices: crossings on every Kuhn edge that belongs to at least one valid cell."""
    X, Y, Z = vol.shape
    vol = vol.astype(np.float32)
    iso = np.float32(iso)
    out = []
    pad = np.zeros((X + 1, Y + 1, Z + 1), dtype=bool)  # pad[i+1,j+1,k+1] = valid[i,j,k]
    pad[1:X, 1:Y, 1:Z] = valid
    for d in KUHN_DIRS:
        d = np.array(d)
        n = np.array([X, Y, Z]) - d
        a = vol[:n[0], :n[1], :n[2]]
        b = vol[d[0]:, d[1]:, d[2]:]
        cross = (a < iso) != (b < iso)
        # cells sharing the edge p..p+d: lower corners p - e with e in {0,1} on the axes where d is 0
        used = np.zeros(cross.shape, dtype=bool)
        free = [ax for ax in range(3) if d[ax] == 0]
        for m in range(1 << len(free)):
            e = np.zeros(3, dtype=int)
            for q, ax in enumerate(free):
                e[ax] = (m >> q) & 1
            sl = tuple(slice(1 - e[ax], 1 - e[ax] + n[ax]) for ax in range(3))
            used |= pad[sl]
        with np.errstate(invalid='ignore'):
            cross &= used
        idx = np.argwhere(cross)
        if idx.shape[0] == 0:
            continue
        va, vb = a[cross], b[cross]
        pa, pb = idx.astype(np.float32), (idx + d).astype(np.float32)
        swap = va > vb
        p0, p1 = np.where(swap[:, None], pb, pa), np.where(swap[:, None], pa, pb)
        v0, v1 = np.where(swap, vb, va), np.where(swap, va, vb)
        t = ((iso - v0) / (v1 - v0)).astype(np.float32)
        p = (p0 + (t[:, None] * (p1 - p0)).astype(np.float32)).astype(np.float32)
        out.append((np.asarray(origin, dtype=np.float64)[None] + p.astype(np.float64) * float(res)).astype(np.float32))
    return np.unique(np.concatenate(out, axis=0), axis=0) if out else np.zeros((0, 3), np.float32)


# ---- the ordered list --------------------------------------------------------------------------------------------------
def blocks(shape):
    """(gz, gy, gx) of the kernel's launch grid: z tiles of 64 cells, y tiles of 4 cells, one x index per block."""
    X, Y, Z = shape
    return ((Z - 1 + TILE_Z - 1) // TILE_Z, (Y - 1 + TILE_Y - 1) // TILE_Y, X - 1)


def block_of(cell, shape):
    """Block number of the cells [n,3] (the index of their count in the workspace)."""
    gz, gy, _ = blocks(shape)
    cell = np.asarray(cell)
    return (cell[:, 0] * gy + cell[:, 1] // TILE_Y) * gz + cell[:, 2] // TILE_Z


def tet_case(m):
    """Sign case m (bit q set: local corner q inside) of a tetrahedron -> (triangles as local-corner edge pairs, neg, pos)."""
    inside = [(m >> q) & 1 for q in range(4)]
    minority = 1 if sum(inside) <= 2 else 0
    a = [q for q in range(4) if inside[q] == minority]
    b = [q for q in range(4) if inside[q] != minority]
    if len(a) == 1:
        tris = [[(a[0], b[0]), (a[0], b[1]), (a[0], b[2])]]
    else:
        quad = [(a[0], b[0]), (a[0], b[1]), (a[1], b[1]), (a[1], b[0])]
        tris = [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    neg = max(q for q in range(4) if inside[q])
    pos = max(q for q in range(4) if not inside[q])
    return tris, neg, pos


Triangles = collections.namedtuple('Triangles', 'tri labels keys counts index cell tet dot')
Triangles.__doc__ = """tri f32[T,3,3] world positions, labels u8[T,3] or None, keys u64[T,3], counts i64[n_blocks] triangles
per block; for the tests: index f32[T,3,3] the voxel-index coordinates, cell i64[T,3] and tet i64[T] where each triangle
comes from, dot f32[T] the winding dot before the swap."""


def triangles(vol, iso, weights=None, ids=None, origin=(0., 0., 0.), res=1.):
    """The triangle list of ojf_mesh_extract, in order (definition: the module docstring)."""
    f32 = np.float32
    X, Y, Z = vol.shape
    v32 = vol.astype(f32)
    iso = f32(iso)
    valid = np_cell_valid(vol, weights)
    with np.errstate(invalid='ignore'):
        inside = v32 < iso
    bits = np.zeros((X - 1, Y - 1, Z - 1), dtype=np.int64)
    for c, o in enumerate(CORNER):
        bits |= inside[o[0]:X - 1 + o[0], o[1]:Y - 1 + o[1], o[2]:Z - 1 + o[2]].astype(np.int64) << c
    cell = np.argwhere(valid & (bits != 0) & (bits != 255))
    ci, cj, ck = cell[:, 0], cell[:, 1], cell[:, 2]
    cell = cell[np.lexsort((ck % TILE_Z, cj % TILE_Y, ck // TILE_Z, cj // TILE_Y, ci))]  # the last key is the primary one
    N = cell.shape[0]
    cv = np.stack([v32[cell[:, 0] + o[0], cell[:, 1] + o[1], cell[:, 2] + o[2]] for o in CORNER], axis=1).reshape(N, 8)
    cin = cv < iso
    P = np.zeros((N, 6, 2, 3, 3), dtype=f32)          # voxel-index coordinates
    E = np.zeros((N, 6, 2, 3, 2), dtype=np.int8)      # cube corners of the edge under each vertex
    DOT = np.zeros((N, 6, 2), dtype=f32)
    present = np.zeros((N, 6, 2), dtype=bool)
    for t, tet in enumerate(TETS):
        case = sum(cin[:, tet[q]].astype(np.int64) << q for q in range(4))
        for m in range(1, 15):
            rows = np.nonzero(case == m)[0]
            if rows.size == 0:
                continue
            tris, neg, pos = tet_case(m)
            p = [(cell[rows] + CORNER[tet[q]]).astype(f32) for q in range(4)]
            tv = [cv[rows, tet[q]] for q in range(4)]
            d = (CORNER[tet[pos]] - CORNER[tet[neg]]).astype(f32)

            def crossing(e):
                va, vb = tv[e[0]], tv[e[1]]
                swap = va > vb
                p0, p1 = np.where(swap[:, None], p[e[1]], p[e[0]]), np.where(swap[:, None], p[e[0]], p[e[1]])
                v0, v1 = np.where(swap, vb, va), np.where(swap, va, vb)
                tt = (iso - v0) / (v1 - v0)
                return p0 + tt[:, None] * (p1 - p0)
            for q, edges in enumerate(tris):
                A, B, C = crossing(edges[0]), crossing(edges[1]), crossing(edges[2])
                assert A.dtype == f32
                u, w = B - A, C - A
                nx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
                ny = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
                nz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
                dot = (nx * d[0] + ny * d[1]) + nz * d[2]
                assert dot.dtype == f32
                swap = dot < 0
                e = np.array([[tet[x[0]], tet[x[1]]] for x in edges], dtype=np.int64)  # [3,2] cube corners
                P[rows, t, q, 0] = A
                P[rows, t, q, 1] = np.where(swap[:, None], C, B)
                P[rows, t, q, 2] = np.where(swap[:, None], B, C)
                E[rows, t, q, 0] = e[0]
                E[rows, t, q, 1] = np.where(swap[:, None], e[2][None], e[1][None])
                E[rows, t, q, 2] = np.where(swap[:, None], e[1][None], e[2][None])
                DOT[rows, t, q] = dot
                present[rows, t, q] = True
    sel = present.reshape(-1)
    index = P.reshape(-1, 3, 3)[sel]
    edge = E.reshape(-1, 3, 2)[sel]
    dot = DOT.reshape(-1)[sel]
    src = np.repeat(np.arange(N), 12)[sel]
    tet_of = np.tile(np.repeat(np.arange(6), 2), N)[sel]
    tri_cell = cell[src]
    c0, c1 = CORNER[edge[..., 0]], CORNER[edge[..., 1]]                       # [T,3,3]
    lower = tri_cell[:, None, :] + np.minimum(c0, c1)
    code = ((c0 != c1).astype(np.uint64) << np.arange(3, dtype=np.uint64)).sum(axis=-1).astype(np.uint64)
    lin = ((lower[..., 0] * Y + lower[..., 1]) * Z + lower[..., 2]).astype(np.uint64)
    keys = lin * np.uint64(8) + code
    tri = (np.asarray(origin, dtype=np.float64).reshape(1, 1, 3) + index.astype(np.float64) * float(res)).astype(f32)
    labels = None
    if ids is not None:
        r = np.rint(index).astype(np.int64)
        labels = ids[r[..., 0], r[..., 1], r[..., 2]].astype(np.uint8)
    gz, gy, gx = blocks(vol.shape)
    per_cell = present.reshape(N, 12).sum(axis=1)
    counts = np.bincount(block_of(cell, vol.shape), weights=per_cell, minlength=gz * gy * gx).astype(np.int64)
    return Triangles(tri, labels, keys, counts, index, tri_cell, tet_of, dot)


# ---- F-score support ---------------------------------------------------------------------------------------------------
def within(query, points, tau, chunk=256):
    """Brute-force f64 statement of ojf_points_within: hit[i] = some point with sqrt(ex*ex + ey*ey + ez*ez) <= tau, products
    and sums rounded one after the other.  A query with a non-finite coordinate is no hit."""
    q = np.asarray(query, dtype=np.float64).reshape(-1, 3)
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    hit = np.zeros(q.shape[0], dtype=bool)
    if p.shape[0] == 0:
        return hit
    finite = np.isfinite(q).all(axis=1)
    for lo in range(0, q.shape[0], chunk):
        rows = np.nonzero(finite[lo:lo + chunk])[0] + lo
        if rows.size == 0:
            continue
        ex = p[None, :, 0] - q[rows, None, 0]
        ey = p[None, :, 1] - q[rows, None, 1]
        ez = p[None, :, 2] - q[rows, None, 2]
        hit[rows] = (np.sqrt(ex * ex + ey * ey + ez * ez) <= float(tau)).any(axis=1)
    return hit
