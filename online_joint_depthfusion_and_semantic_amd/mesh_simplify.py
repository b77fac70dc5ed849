"""Mesh simplification on the device: vertex clustering with quadric error metrics (csrc/ojf_simplify.hip, ``ojf_mesh_simplify``;
the definition is in DESIGN.md §19 and restated in numpy by tests/simplify_ref.py).  The third stage of the reference's
deps/mesh-fusion (scale, fuse, simplify), which shells out to meshlabserver on the host.

A uniform grid of cells cuts the mesh; all vertices of a cell become one vertex, placed where the summed plane quadric of the
incident faces is smallest (so planes stay planes and room corners stay sharp); faces that lose a corner disappear.  The cell
size is the only knob.  The same bits on every run and for every order of the faces.  Clustering can pinch a surface: there is no
manifoldness guarantee, and no face-count target."""
import math

import numpy as np
import torch

from . import _lib

MAX_FACES = 1 << 24  # csrc/ojf_simplify.hip: kSMaxFaces (the exact integer sums are proved for that many faces)


def default_grid(vmin, vmax, cell):
    """(lo f32[3], (GX, GY, GZ)) of the grid ``cluster`` uses when none is given (host arithmetic only): per axis lo is the
    vertex minimum rounded down to a multiple of ``cell`` in fp32 and the grid reaches the cell of the vertex maximum."""
    cell = np.float32(cell)
    vmin, vmax = np.asarray(vmin, np.float32).reshape(3), np.asarray(vmax, np.float32).reshape(3)
    if not (np.isfinite(vmin).all() and np.isfinite(vmax).all()):
        raise ValueError('cluster: without lo and grid every vertex must be finite')
    with np.errstate(over='ignore', invalid='ignore'):
        lo = np.floor(vmin / cell) * cell
        lo = np.where(lo > vmin, lo - cell, lo).astype(np.float32)
        top = np.floor((vmax - lo) / cell)
    if not (np.isfinite(lo).all() and np.isfinite(top).all() and (top < 2 ** 31 - 1).all()):
        raise ValueError('cluster: cell {!r} is too small for the extent of the mesh'.format(float(cell)))
    return lo, tuple(int(v) + 1 for v in top)


def voxel_cell(simplify, resolution):
    """The cell size of ``extract_mesh(..., simplify=)``: ``simplify`` voxels of ``resolution`` (the f64 product)."""
    if isinstance(simplify, bool) or not isinstance(simplify, (int, float)) or not math.isfinite(simplify) or not simplify > 0:
        raise ValueError('simplify must be None or a finite cell size in voxels > 0, got {!r}'.format(simplify))
    return float(simplify) * float(resolution)


def _check(who, vertices, faces, cell, lo, grid):
    """Argument errors, before a device is touched.  Returns (cell, lo or None, grid or None)."""
    for name, t, dt in (('vertices', vertices, torch.float32), ('faces', faces, torch.int32)):
        if not torch.is_tensor(t) or t.dtype != dt or t.dim() != 2 or t.shape[1] != 3:
            raise ValueError('{}: {} must be a {} tensor of shape [n,3]'.format(who, name, dt))
    if vertices.shape[0] >= 2 ** 31:
        raise ValueError('{}: fewer than 2^31 vertices expected'.format(who))
    if faces.shape[0] > MAX_FACES:
        raise ValueError('{}: at most 2^24 faces expected, got {}'.format(who, faces.shape[0]))
    if isinstance(cell, bool) or not isinstance(cell, (int, float)) or not math.isfinite(cell):
        raise ValueError('{}: cell must be a finite number > 0, got {!r}'.format(who, cell))
    with np.errstate(over='ignore'):
        cell32 = np.float32(cell)
    if not (cell32 > 0 and np.isfinite(cell32)):
        raise ValueError('{}: cell must be > 0 and finite in fp32, got {!r}'.format(who, cell))
    if (lo is None) != (grid is None):
        raise ValueError('{}: lo and grid go together'.format(who))
    if lo is not None:
        lo = np.ascontiguousarray(np.asarray(lo, dtype=np.float32).reshape(-1))
        if lo.shape != (3,) or not np.isfinite(lo).all():
            raise ValueError('{}: lo must be three finite numbers'.format(who))
        grid = tuple(grid)
        if len(grid) != 3 or any(isinstance(g, bool) or not isinstance(g, (int, np.integer)) or g < 1 for g in grid) or \
                int(grid[0]) * int(grid[1]) * int(grid[2]) >= 2 ** 31:
            raise ValueError('{}: grid must be three integers >= 1 with a product below 2^31, got {!r}'.format(who, grid))
        grid = tuple(int(g) for g in grid)
    if not vertices.is_cuda or faces.device != vertices.device:
        raise ValueError('{}: vertices and faces must be cuda tensors on one device'.format(who))
    return float(cell32), lo, grid


def cluster(vertices, faces, cell, lo=None, grid=None):
    """Cluster an indexed mesh on the current stream of its device.

    vertices f32 [nv,3], faces i32 [nf,3] (cuda, nf <= 2^24); ``cell``: the cell size; ``lo`` (three numbers) and ``grid``
    (GX, GY, GZ): the grid - omitted, lo is the vertex minimum rounded down to a multiple of ``cell`` and the grid covers the
    maximum (``default_grid``; every vertex must then be finite).  Vertices outside the grid or not finite are invalid: they and
    their faces are left out.  Returns device tensors (vertices f32 [nc,3], faces i32 [nk,3], source i32 [nc], face_source i32
    [nk]): one vertex per occupied cell in ascending cell order, the kept faces in input order, and for attributes
    ``attr[source]`` - the input vertex nearest to each output vertex - and the input face of each output face.  Repeated
    output faces are kept (``simplify(..., unique_faces=True)`` drops them).  Waits once, for the two counts."""
    who = 'cluster'
    cell, lo, grid = _check(who, vertices, faces, cell, lo, grid)
    dev = vertices.device
    nv, nf = vertices.shape[0], faces.shape[0]

    def empty():
        return (torch.zeros((0, 3), dtype=torch.float32, device=dev), torch.zeros((0, 3), dtype=torch.int32, device=dev),
                torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev))
    if nv == 0:
        return empty()
    _lib.require_gpu()
    lib = _lib.load()
    vertices, faces = vertices.contiguous(), faces.contiguous()
    if lo is None:
        lo, grid = default_grid(vertices.min(dim=0).values.tolist(), vertices.max(dim=0).values.tolist(), cell)
        if grid[0] * grid[1] * grid[2] >= 2 ** 31:
            raise ValueError('{}: cell {!r} gives a grid of {} cells, 2^31 or more'.format(who, cell, grid))
    ws_bytes = lib.ojf_mesh_simplify_workspace_bytes(nv, nf, *grid)
    if ws_bytes == 0:
        raise ValueError('{}: sizes out of range (nv {}, nf {}, grid {})'.format(who, nv, nf, grid))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    st = _lib.stream_ptr(dev)

    def run(phases, rows, out_v, src, out_f, fsrc):
        rc = lib.ojf_mesh_simplify(_lib.ptr(vertices), nv, _lib.ptr(faces), nf, lo.ctypes.data, cell, grid[0], grid[1], grid[2], phases,
                                   _lib.ptr(ws), ws_bytes, _lib.ptr(rows), 0 if rows is None else rows.numel(), _lib.ptr(out_v),
                                   _lib.ptr(src), 0 if out_v is None else out_v.shape[0], _lib.ptr(out_f), _lib.ptr(fsrc),
                                   0 if out_f is None else out_f.shape[0], _lib.ptr(counts), st)
        _lib.check(rc, 'ojf_mesh_simplify')

    run(_lib.SIMPLIFY_MARK | _lib.SIMPLIFY_SCAN | _lib.SIMPLIFY_COUNT, None, None, None, None, None)
    nc, nk = counts.tolist()
    if nc == 0:
        return empty()
    rows = torch.empty(lib.ojf_mesh_simplify_cluster_bytes(nc), dtype=torch.uint8, device=dev)
    out_v = torch.empty((nc, 3), dtype=torch.float32, device=dev)
    src = torch.empty(nc, dtype=torch.int32, device=dev)
    out_f = torch.empty((nk, 3), dtype=torch.int32, device=dev)
    fsrc = torch.empty(nk, dtype=torch.int32, device=dev)
    run(_lib.SIMPLIFY_ACCUMULATE | _lib.SIMPLIFY_SOLVE | _lib.SIMPLIFY_NEAREST | _lib.SIMPLIFY_FACES, rows, out_v, src,
        out_f if nk else None, fsrc if nk else None)
    return out_v, out_f, src, fsrc


def unique_faces(faces, face_source):
    """Drop repeated faces: every triple rotated to start at its smallest index (the orientation is kept), the distinct triples
    in ascending lexicographic order, each with the smallest input face among its repeats.  Device tensors in and out."""
    if faces.shape[0] == 0:
        return faces, face_source
    f = faces.to(torch.int64)
    first = f.argmin(dim=1, keepdim=True)
    rot = torch.gather(f, 1, (first + torch.arange(3, device=f.device)[None]) % 3)
    uniq, inverse = torch.unique(rot, dim=0, return_inverse=True)
    src = torch.full((uniq.shape[0],), 2 ** 31 - 1, dtype=torch.int32, device=f.device)
    src.scatter_reduce_(0, inverse.reshape(-1), face_source.to(torch.int32), 'amin')
    return uniq.to(torch.int32), src


def simplify_tensors(vertices, faces, cell, labels=None, unique=False):
    """``cluster`` on device tensors with the vertex labels carried along: (vertices, faces i32, labels or None, source,
    face_source)."""
    verts, out_f, source, fsrc = cluster(vertices, faces.to(torch.int32), cell)
    if unique:
        out_f, fsrc = unique_faces(out_f, fsrc)
    vlab = None if labels is None else labels[source.to(torch.int64)]
    return verts, out_f, vlab, source, fsrc


def simplify(mesh, cell, unique_faces=False, device=None):
    """Simplify a mesh: ``mesh`` is the dict ``mesh.extract_mesh`` returns (vertices, faces, and optionally normals, labels,
    rgb; numpy arrays or tensors) or a (vertices, faces) pair.  Returns a dict of numpy arrays like extract_mesh's: vertices,
    faces (i32), normals (recomputed with ``mesh.vertex_normals``), labels and rgb (``attr[source]``, None where the input has
    none), and source / face_source.  ``unique_faces`` drops repeated output faces."""
    from . import mesh as mesh_
    if not isinstance(mesh, dict):
        vertices, faces = mesh
        mesh = {'vertices': vertices, 'faces': faces}
    dev = torch.device(device) if device is not None else (mesh['vertices'].device if torch.is_tensor(mesh['vertices']) else
                                                          torch.device('cuda'))

    def to_dev(a, dt):
        return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(device=dev, dtype=dt)
    verts, faces, _, source, fsrc = simplify_tensors(to_dev(mesh['vertices'], torch.float32), to_dev(mesh['faces'], torch.int32), cell,
                                                     unique=unique_faces)
    f64 = faces.to(torch.int64)
    normals = mesh_.vertex_normals(verts, f64) if faces.shape[0] else torch.zeros_like(verts)
    src = source.cpu().numpy()
    out = {'vertices': verts.cpu().numpy(), 'faces': faces.cpu().numpy(), 'normals': normals.cpu().numpy(), 'labels': None, 'rgb': None,
           'source': src, 'face_source': fsrc.cpu().numpy()}
    for name in ('labels', 'rgb'):
        attr = mesh.get(name)
        if attr is not None:
            out[name] = (attr.cpu().numpy() if torch.is_tensor(attr) else np.asarray(attr))[src]
    return out
