"""Triangle meshes to frames and to ground-truth volumes: depth, face, label and colour images of a mesh at pinhole views
(csrc/ojf_raster.hip, ``ojf_rasterize`` / ``ojf_rasterize_attributes``; the fp32 definition is in that file's header and
restated in numpy by tests/raster_ref.py), a frame stream over a mesh with the dict schema of synthetic.SyntheticStream,
and the ground-truth TSDF / label grids datasets.py reads - the rasterised views fused by projective.integrate_depth with
carving.  The reference makes its grids with an OpenGL off-screen renderer feeding a CUDA fusion (deps/mesh-fusion);
neither runs here.

Views are camera-to-world poses with pinhole intrinsics, pixel centres at integer coordinates: the conventions of
projective.integrate_depth, so that a rasterised depth map goes straight back into a volume."""
import os

import numpy as np
import torch

from . import _lib, views
from .ops import _origin_array
from .projective import integrate_depth


def _mesh(vertices, faces, who):
    if not (torch.is_tensor(vertices) and vertices.is_cuda and vertices.dim() == 2 and vertices.shape[1] == 3 and vertices.shape[0] > 0):
        raise ValueError('{}: vertices must be a cuda tensor [nv,3]'.format(who))
    dev = vertices.device
    vertices = vertices.to(torch.float32).contiguous()
    faces = torch.as_tensor(faces)
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] == 0 or faces.is_floating_point():
        raise ValueError('{}: faces must be an integer array [nf,3]'.format(who))
    if faces.dtype != torch.int32:  # (an index that does not fit is out of range either way: the kernel skips the face)
        faces = faces.to(torch.int64).clamp(-1, 2 ** 31 - 1)
    return vertices, faces.to(device=dev, dtype=torch.int32).contiguous()


def _attribute(x, rows, cols, name, who, dev):
    if x is None:
        return None
    x = torch.as_tensor(x)
    shape = (rows,) if cols is None else (rows, cols)
    if cols == 4 and tuple(x.shape) == (rows, 3):
        x = torch.cat([x, torch.full((rows, 1), 255, dtype=x.dtype, device=x.device)], dim=1)
    if tuple(x.shape) != shape or x.dtype != torch.uint8:
        raise ValueError('{}: {} must be u8 {}'.format(who, name, list(shape)))
    return x.to(dev).contiguous()


def rasterize(vertices, faces, intrinsics, extrinsics, shape, near=0., face_labels=None, vertex_colors=None):
    """Depth, face and, where asked for, label and colour images of a triangle mesh at ``n`` views, on the current stream
    of the vertices' device.

    vertices: cuda float [nv,3] in the world frame; faces: integer [nf,3] (tensor or numpy); intrinsics [3,3] or [n,3,3]
    pinhole, extrinsics (camera-to-world) [3,4] / [4,4] or [n,...]; the number of views is that of the extrinsics;
    shape: (h, w); near: hits with a camera depth <= near are dropped; face_labels: u8 [nf]; vertex_colors: u8 [nv,3|4].
    Returns {'depth' f32 [n,h,w] (camera z-depth, 0 where nothing is hit), 'face' i32 [n,h,w] (-1 where nothing is hit),
    'labels' u8 [n,h,w] (with face_labels; 0 where nothing is hit), 'color' u8 [n,h,w,4] (with vertex_colors; barycentric,
    alpha 255, all 0 where nothing is hit)} of device tensors.  Two-sided, no culling; triangles that cross the camera
    plane come out right; faces with an out-of-range index or a non-finite vertex are skipped.  More than
    ``_lib.RASTER_MAX_VIEWS`` views go in several kernel calls, with the same bits as one view per call."""
    who = 'rasterize'
    _lib.require_gpu()
    lib = _lib.load()
    vertices, faces = _mesh(vertices, faces, who)
    dev = vertices.device
    nv, nf = vertices.shape[0], faces.shape[0]
    h, w = int(shape[0]), int(shape[1])
    if h < 1 or w < 1:
        raise ValueError('{}: shape must be (h, w) with h, w >= 1'.format(who))
    near = float(near)
    if not (0.0 <= near < float('inf')):
        raise ValueError('{}: near >= 0 and finite expected, got {}'.format(who, near))
    n, K, E = views.cameras(who, intrinsics, extrinsics, nonzero_focal=True)
    face_labels = _attribute(face_labels, nf, None, 'face_labels', who, dev)
    vertex_colors = _attribute(vertex_colors, nv, 4, 'vertex_colors', who, dev)
    out = {'depth': torch.empty((n, h, w), dtype=torch.float32, device=dev),
           'face': torch.empty((n, h, w), dtype=torch.int32, device=dev)}
    if face_labels is not None:
        out['labels'] = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    if vertex_colors is not None:
        out['color'] = torch.empty((n, h, w, 4), dtype=torch.uint8, device=dev)
    step = _lib.RASTER_MAX_VIEWS
    keys = torch.empty((min(n, step), h, w), dtype=torch.int64, device=dev)
    stream = _lib.stream_ptr(dev)
    for v0, v1, Kc, Ec in views.chunks(n, step, K, E):
        rc = lib.ojf_rasterize(_lib.ptr(vertices), nv, _lib.ptr(faces), nf, v1 - v0, Kc.ctypes.data, Ec.ctypes.data, h, w, near,
                               _lib.ptr(keys), _lib.ptr(out['depth'][v0:v1]), _lib.ptr(out['face'][v0:v1]), stream)
        _lib.check(rc, 'ojf_rasterize')
        if face_labels is not None or vertex_colors is not None:
            rc = lib.ojf_rasterize_attributes(_lib.ptr(vertices), nv, _lib.ptr(faces), nf, v1 - v0, Kc.ctypes.data, Ec.ctypes.data,
                                              h, w, _lib.ptr(out['face'][v0:v1]), _lib.ptr(face_labels), _lib.ptr(vertex_colors),
                                              _lib.ptr(out['labels'][v0:v1]) if face_labels is not None else None,
                                              _lib.ptr(out['color'][v0:v1]) if vertex_colors is not None else None, stream)
            _lib.check(rc, 'ojf_rasterize_attributes')
    return out


class MeshStream:
    """Frame stream over a triangle mesh with the dict schema of synthetic.SyntheticStream: ``frame(i)`` returns the
    un-batched sample (numpy), ``batch(i)`` the batched torch dict ``Pipeline.fuse`` takes.  Keys: ``image [3,h,w] f32``
    (the rasterised vertex colours on the 0..255 scale, zeros without vertex_colors), ``<input_key> [h,w] f32`` camera
    z-depth, ``mask = depth > 0``, ``extrinsics [3,4] f64``, ``intrinsics [3,3] f64``, ``semantic_gt [h,w] u8`` (the
    rasterised face labels, zeros without face_labels), ``frame_id 'scene/0/frame'``, ``item_id``.

    vertices: cuda float [nv,3]; poses: camera-to-world [n,3,4] or [n,4,4]; intrinsics [3,3] or [n,3,3]; shape (h, w).
    Frames are rendered in batches of up to ``_lib.RASTER_MAX_VIEWS`` (the batch a requested frame lies in) and cached on
    the host."""

    def __init__(self, vertices, faces, poses, intrinsics, shape, face_labels=None, vertex_colors=None, scene='mesh_0',
                 input_key='tof_depth', near=0.):
        self.vertices, self.faces = _mesh(vertices, faces, 'MeshStream')
        self.face_labels, self.vertex_colors = face_labels, vertex_colors
        self.h, self.w = int(shape[0]), int(shape[1])
        P = np.asarray(torch.as_tensor(poses).detach().cpu().to(torch.float64).numpy())
        if P.ndim != 3 or P.shape[1] not in (3, 4) or P.shape[2] != 4 or P.shape[0] < 1:
            raise ValueError('MeshStream: poses [n,3,4] or [n,4,4] expected, got {}'.format(P.shape))
        self.poses = np.ascontiguousarray(P[:, :3, :])
        K = np.asarray(torch.as_tensor(intrinsics).detach().cpu().to(torch.float64).numpy())
        if K.shape not in ((3, 3), (len(P), 3, 3)):
            raise ValueError('MeshStream: intrinsics [3,3] or [n,3,3] expected, got {}'.format(K.shape))
        self.K = np.ascontiguousarray(np.broadcast_to(K, (len(P), 3, 3)))
        self.scene, self.scenes = scene, [scene]
        self.input_key = input_key
        self.near = near
        self._batches = list(views.chunks(len(P), _lib.RASTER_MAX_VIEWS, self.K, self.poses))  # (v0, v1, K, poses) per batch
        self._cache = {}  # first frame of a batch -> host images of the batch

    def __len__(self):
        return len(self.poses)

    def _images(self, i):
        v0, _, K, poses = self._batches[i // _lib.RASTER_MAX_VIEWS]
        if v0 not in self._cache:
            out = rasterize(self.vertices, self.faces, K, poses, (self.h, self.w), self.near, self.face_labels, self.vertex_colors)
            self._cache[v0] = {k: v.cpu().numpy() for k, v in out.items()}
        return {k: v[i - v0] for k, v in self._cache[v0].items()}

    def frame(self, i):
        if not 0 <= i < len(self):
            raise IndexError(i)
        im = self._images(i)
        depth = im['depth']
        image = np.zeros((3, self.h, self.w), np.float32)
        if 'color' in im:
            image = np.ascontiguousarray(im['color'][..., :3].transpose(2, 0, 1)).astype(np.float32)
        return {
            'item_id': i,
            'frame_id': '{}/0/{:06d}'.format(self.scene, i),
            'image': image,
            self.input_key: depth.copy(),
            'mask': depth > 0,
            'extrinsics': self.poses[i].copy(),
            'intrinsics': self.K[i].copy(),
            'semantic_gt': im['labels'].copy() if 'labels' in im else np.zeros((self.h, self.w), np.uint8),
        }

    def batch(self, i):
        out = {}
        for k, v in self.frame(i).items():
            if isinstance(v, np.ndarray):
                out[k] = torch.from_numpy(v).unsqueeze(0)
            elif isinstance(v, str):
                out[k] = [v]
            else:
                out[k] = torch.tensor([v])
        return out


def ground_truth_grid(vertices, faces, *, origin, resolution, shape, truncation, intrinsics, extrinsics, image_shape,
                      face_labels=None, max_weight=128.0, near=0.0, distance='projective'):
    """Ground-truth volumes of a mesh: the views are rasterised and fused by ``projective.integrate_depth(carve=True)``,
    with the face labels where given.  origin / resolution / shape (X, Y, Z): the volume, in the frame of extract /
    integrate / render; intrinsics / extrinsics / image_shape (h, w): the views, as for ``rasterize`` - they should see
    every surface from the free side.  Returns device (tsdf fp16 [X,Y,Z], labels u8 [X,Y,Z]); voxels no view reached
    (weight 0) hold -truncation and label 0: the "solid" value datasets.py pads ground-truth grids with.

    distance='projective' (the default): the fused values as they are - distances along the optical axes.
    distance='euclidean': the views give only the sign - positive where a view reached the voxel and the fused value is
    > 0, negative everywhere else; the value is sign·min(d, truncation) with d the exact distance to the mesh
    (``mesh_distance.distance_field(band=truncation)``), and the label that of the nearest face where d < truncation, 0
    elsewhere: a Euclidean TSDF, and labels that do not depend on the list of poses."""
    if not (torch.is_tensor(vertices) and vertices.is_cuda):
        raise ValueError('ground_truth_grid: vertices must be a cuda tensor [nv,3]')
    if distance not in ('projective', 'euclidean'):
        raise ValueError("ground_truth_grid: distance must be 'projective' or 'euclidean'")
    dev = vertices.device
    truncation = float(truncation)
    X, Y, Z = (int(s) for s in shape)
    frames = rasterize(vertices, faces, intrinsics, extrinsics, image_shape, near, face_labels)
    tsdf = torch.full((X, Y, Z), truncation, dtype=torch.float16, device=dev)
    weights = torch.zeros((X, Y, Z), dtype=torch.float16, device=dev)
    sem = face_labels is not None
    ids = torch.zeros((X, Y, Z), dtype=torch.uint8, device=dev)
    scores = torch.zeros((X, Y, Z), dtype=torch.float16, device=dev) if sem else None
    integrate_depth(tsdf, weights, origin=_origin_array(origin), resolution=float(resolution), depth=frames['depth'],
                    intrinsics=intrinsics, extrinsics=extrinsics, ids=ids if sem else None, scores=scores,
                    labels=frames['labels'] if sem else None, truncation=truncation, max_weight=max_weight, near=near, carve=True)
    unseen = weights == 0
    tsdf.masked_fill_(unseen, -truncation)
    ids.masked_fill_(unseen, 0)
    if distance == 'euclidean':
        from .mesh_distance import distance_field
        field = distance_field(vertices, faces, origin=origin, resolution=resolution, shape=(X, Y, Z), band=truncation,
                               face_labels=face_labels)
        d = field['distance'].clamp(max=float(np.float32(truncation)))
        tsdf = torch.where(tsdf > 0, d, -d).to(torch.float16)  # (unseen voxels hold -truncation: negative)
        ids = torch.where(field['distance'] < truncation, field['labels'], torch.zeros_like(ids)) if sem else torch.zeros_like(ids)
    return tsdf, ids


def save_ground_truth(path, tsdf, labels, origin, resolution):
    """Writes the volumes of ``ground_truth_grid`` as the npz sibling of ``path`` (an ``*.hdf`` name) through
    ``datasets.export_grid_npz``: what ``datasets.load_sdf_file`` and the adapters' ``get_grid`` read.  Returns the file
    written."""
    from .datasets import export_grid_npz
    host = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)  # noqa: E731
    tsdf = host(tsdf)
    org = _origin_array(origin)
    bbox = np.stack([org, org + float(resolution) * np.array(tsdf.shape, np.float64)], axis=1)
    return export_grid_npz(os.path.abspath(path), tsdf, bbox, float(resolution), None if labels is None else host(labels))
