"""Exact mesh-to-voxel distance fields: for every voxel centre of a box the Euclidean distance to a triangle mesh within a
band, the nearest face, its label and - for closed meshes - a sign (csrc/ojf_mesh_distance.hip, ``ojf_mesh_distance`` /
``ojf_mesh_distance_sign``; the fp32 definition is in that file's header and restated in numpy by
tests/mesh_distance_ref.py).  The reference gets its ground-truth TSDFs from a distance transform over a voxelised mesh
(deps/distance-transform, deps/graphics compute_tsdf); this is the same quantity, computed against the triangles themselves.

The box is the volume of extract / integrate / render: voxel (i, j, k) has its centre at origin + (index + 0.5)·resolution."""
import numpy as np
import torch

from . import _lib
from .ops import _origin_array


def pseudonormals(vertices, faces):
    """Angle-weighted pseudonormals (Baerentzen & Aanaes 2005) of a mesh, in float64 numpy, rounded to fp32 at the end.

    vertices [nv,3], faces int [nf,3] (numpy).  Returns (vertex_normals f32 [nv,3], edge_normals f32 [ne,3], face_edges i32
    [nf,3]): a vertex's normal is the sum over its faces of (the face's angle at the vertex)·(the unit face normal); an
    edge's the sum of the unit normals of the faces that share the unordered vertex pair; ``face_edges[f][k]`` is the edge
    from vertex k to vertex k + 1 of face f.  Faces with an index outside [0, nv), a non-finite vertex or no area add
    nothing.  The sums run corner by corner, each in face order (``np.add.at``).  None of the normals is normalised: only
    the sign of a dot product with them is ever used."""
    V = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    Fc = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    nv, nf = len(V), len(Fc)
    ok = ((Fc >= 0) & (Fc < nv)).all(axis=1)
    ok &= np.isfinite(V[np.where(ok[:, None], Fc, 0)]).all(axis=(1, 2))
    G = Fc[ok]
    P = V[G]  # [m, corner, xyz]
    n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    length = np.linalg.norm(n, axis=1)
    with np.errstate(all='ignore'):
        unit = np.where((length > 0)[:, None], n / length[:, None], 0.0)
    vn = np.zeros((nv, 3))
    pair = np.sort(np.stack([G, np.roll(G, -1, axis=1)], axis=-1), axis=-1)  # [m, k, 2]: (v_k, v_k+1), unordered
    face_edges = np.zeros((nf, 3), np.int32)
    if len(G):
        uniq, inverse = np.unique(pair.reshape(-1, 2), axis=0, return_inverse=True)
        inverse = inverse.reshape(-1, 3)
        face_edges[ok] = inverse
        en = np.zeros((len(uniq), 3))
    else:
        inverse = np.zeros((0, 3), np.int64)
        en = np.zeros((1, 3))
    for k in range(3):
        u, w = P[:, (k + 1) % 3] - P[:, k], P[:, (k + 2) % 3] - P[:, k]
        angle = np.arctan2(np.linalg.norm(np.cross(u, w), axis=1), (u * w).sum(axis=1))
        np.add.at(vn, G[:, k], angle[:, None] * unit)
        np.add.at(en, inverse[:, k], unit)
    return vn.astype(np.float32), en.astype(np.float32), face_edges


def _box(origin, resolution, shape, who):
    origin = _origin_array(origin)
    resolution = float(resolution)
    try:
        X, Y, Z = (int(s) for s in shape)
    except (TypeError, ValueError):
        raise ValueError('{}: shape must be (X, Y, Z)'.format(who))
    if min(X, Y, Z) < 1 or X * Y * Z >= 2 ** 31:
        raise ValueError('{}: shape must be (X, Y, Z) with positive sizes and X·Y·Z < 2^31'.format(who))
    if not (np.isfinite(origin).all() and np.isfinite(resolution) and resolution > 0):
        raise ValueError('{}: finite origin and a finite resolution > 0 expected'.format(who))
    return origin, resolution, (X, Y, Z)


def distance_field(vertices, faces, *, origin, resolution, shape, band, face_labels=None, sign=None):
    """The distance from every voxel centre of the box to the mesh where it is at most ``band`` (metres), on the current
    stream of the vertices' device.

    vertices: cuda float [nv,3]; faces: integer [nf,3] (tensor or numpy); origin f64[3], resolution, shape (X, Y, Z): the
    box; face_labels: u8 [nf]; sign: None or 'normals'.  Returns a dict of device tensors [X,Y,Z]:
      'distance' f32 - the Euclidean distance to the nearest triangle, +inf where that is more than ``band``;
      'face' i32 - the nearest face (ties to the lower index), -1 there;
      'labels' u8 (with face_labels) - face_labels[face], 0 where face < 0;
      'signed' f32 (with sign='normals') - distance with the sign of (voxel - closest point)·N, N the angle-weighted
        pseudonormal of the closest feature (face, edge or vertex), +inf where face < 0.  Positive outside a CLOSED,
        consistently outward-wound, non-self-intersecting mesh, and meaningful only for such a mesh: a union of overlapping
        closed pieces (a room with solids that share faces with its walls) is not one - take the sign from views there
        (``rasterize.ground_truth_grid(distance='euclidean')``);
    and 'pairs', a Python int: the number of (triangle, brick) pairs the call binned (0: the mesh is nowhere near the box).
    Faces with an index out of range or a non-finite vertex are skipped; zero-area faces count as their edges.  The
    outputs are the same bits on every run and for every order of the faces.  Waits once, to read the number of
    (triangle, brick) pairs that sizes the lists."""
    who = 'distance_field'
    from .rasterize import _attribute, _mesh
    _lib.require_gpu()
    lib = _lib.load()
    vertices, faces = _mesh(vertices, faces, who)
    dev = vertices.device
    nv, nf = vertices.shape[0], faces.shape[0]
    origin, resolution, (X, Y, Z) = _box(origin, resolution, shape, who)
    band = float(band)
    if not (0.0 < band < float('inf')) or not np.isfinite(np.float32(band)) or np.float32(band) <= 0:
        raise ValueError('{}: band > 0 and finite expected, got {}'.format(who, band))
    if sign not in (None, 'normals'):
        raise ValueError("{}: sign must be None or 'normals'".format(who))
    face_labels = _attribute(face_labels, nf, None, 'face_labels', who, dev)
    stream = _lib.stream_ptr(dev)
    ws_bytes = lib.ojf_mesh_distance_workspace_bytes(X, Y, Z)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    args = (_lib.ptr(vertices), nv, _lib.ptr(faces), nf, origin.ctypes.data, resolution, X, Y, Z, band)
    rc = lib.ojf_mesh_distance(*args, _lib.MESH_DISTANCE_ALL, _lib.ptr(ws), ws_bytes, None, 0, _lib.ptr(count), None, None, stream)
    _lib.check(rc, 'ojf_mesh_distance')
    n_pairs = int(count.item())
    if n_pairs >= 2 ** 31:
        raise ValueError('{}: {} (triangle, brick) pairs: too many for one call - a smaller band or box'.format(who, n_pairs))
    pairs = torch.empty(max(n_pairs, 1), dtype=torch.int32, device=dev)
    out = {'distance': torch.empty((X, Y, Z), dtype=torch.float32, device=dev),
           'face': torch.empty((X, Y, Z), dtype=torch.int32, device=dev)}
    # (the counts and offsets of the first call are still in the workspace)
    rc = lib.ojf_mesh_distance(*args, _lib.MESH_DISTANCE_FILL | _lib.MESH_DISTANCE_GATHER, _lib.ptr(ws), ws_bytes, _lib.ptr(pairs),
                               pairs.numel(), None, _lib.ptr(out['distance']), _lib.ptr(out['face']), stream)
    _lib.check(rc, 'ojf_mesh_distance')
    out['pairs'] = n_pairs
    if face_labels is not None:
        out['labels'] = torch.where(out['face'] >= 0, face_labels[out['face'].clamp(min=0).long()], torch.zeros((), dtype=torch.uint8, device=dev))
    if sign == 'normals':
        vn, en, fe = pseudonormals(vertices.cpu().numpy(), faces.cpu().numpy())
        vn, en, fe = (torch.from_numpy(a).to(dev) for a in (vn, en, fe))
        out['signed'] = torch.empty((X, Y, Z), dtype=torch.float32, device=dev)
        rc = lib.ojf_mesh_distance_sign(*args[:9], _lib.ptr(out['distance']), _lib.ptr(out['face']), _lib.ptr(vn), _lib.ptr(en),
                                        en.shape[0], _lib.ptr(fe), _lib.ptr(out['signed']), stream)
        _lib.check(rc, 'ojf_mesh_distance_sign')
    return out


def tsdf_from_mesh(vertices, faces, *, origin, resolution, shape, truncation, face_labels=None):
    """Cameraless ground-truth volumes of a CLOSED mesh (see ``distance_field`` for what that has to mean): returns device
    (tsdf fp16 [X,Y,Z] = clip(signed distance, -truncation, truncation), positive outside; labels u8 [X,Y,Z] = the nearest
    face's label where |signed| < truncation, else 0) - the shapes and dtypes ``rasterize.save_ground_truth`` takes.

    A voxel deep inside the mesh needs its nearest face for its sign as much as one near the surface, so the band here is
    the diagonal of the box and the mesh together: every voxel meets every triangle that reaches its brick - voxels x
    triangles work at worst.  Meant for object-sized meshes; a scene-sized mesh takes its sign from views."""
    who = 'tsdf_from_mesh'
    truncation = float(truncation)
    if not (0.0 < truncation < float('inf')):
        raise ValueError('{}: truncation > 0 and finite expected'.format(who))
    org, res, (X, Y, Z) = _box(origin, resolution, shape, who)
    if not (torch.is_tensor(vertices) and vertices.is_cuda):
        raise ValueError('{}: vertices must be a cuda tensor [nv,3]'.format(who))
    finite = vertices[torch.isfinite(vertices).all(dim=1)].double()
    lo = np.minimum(org, finite.min(dim=0).values.cpu().numpy() if len(finite) else org)
    hi = np.maximum(org + res * np.array([X, Y, Z]), finite.max(dim=0).values.cpu().numpy() if len(finite) else org)
    band = float(np.linalg.norm(hi - lo)) * 1.001 + truncation
    f = distance_field(vertices, faces, origin=org, resolution=res, shape=(X, Y, Z), band=band, face_labels=face_labels, sign='normals')
    tsdf = f['signed'].clamp(-truncation, truncation).to(torch.float16)
    labels = torch.zeros((X, Y, Z), dtype=torch.uint8, device=tsdf.device)
    if face_labels is not None:
        labels = torch.where(f['distance'] < truncation, f['labels'], labels)
    return tsdf, labels
