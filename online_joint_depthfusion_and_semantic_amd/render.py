"""Ray casting of a fused volume: depth, normal and label images of the model as a camera would see it (KinectFusion
style).  The kernel is csrc/ojf_render.hip (``ojf_render``); its fp32 definition is written in that file's header and
restated in numpy by tests/render_ref.py.  The reference has no counterpart on its hot path.

The volume frame is the one extract and integrate use (voxel (i,j,k) centred at origin + (i+0.5, j+0.5, k+0.5)·res),
not the mesh frame of ``Database.get_mesh``.  The returned depth is the camera z-depth, 0 where the ray hits nothing -
the same convention as the input depth maps.
"""
import torch

from . import _lib, views
from .ops import _origin_array


def _poses(intrinsics, extrinsics):
    """``views.inverse_cameras`` under the name the test helpers of earlier revisions import (their render_ref.cameras)."""
    return views.inverse_cameras('render', intrinsics, extrinsics)


def render_views(tsdf, weights=None, ids=None, *, origin, resolution, intrinsics, extrinsics, shape, near=0.0,
                 normals=True):
    """Ray-cast ``n`` views of a device volume in one kernel call on the current stream of the volume's device.

    tsdf: cuda fp16 [X,Y,Z]; weights: cuda fp16 [X,Y,Z] or None (every voxel observed; with weights, a crossing between
    samples that touch an unobserved voxel is not a surface); ids: cuda u8 [X,Y,Z] or None.  origin f64[3] and
    resolution of the volume; intrinsics [3,3] or [n,3,3], extrinsics (camera-to-world) [3,4] or [n,3,4] (or 4x4) - the
    batch dict's entries will do; shape (h, w); near: the smallest z-depth a hit may have.
    Returns {'depth': f32 [n,h,w], 'normals': f32 [n,h,w,3] or None, 'labels': u8 [n,h,w] or None} on the device, with
    the leading n kept for a single view too."""
    _lib.require_gpu()
    lib = _lib.load()
    who = 'render_views'
    tsdf = views.volume3(who, tsdf, 'tsdf', torch.float16, copy=True)
    if weights is not None:
        weights = views.volume3(who, weights, 'weights', torch.float16, tsdf.shape, tsdf.device, copy=True)
    if ids is not None:
        ids = views.volume3(who, ids, 'ids', torch.uint8, tsdf.shape, tsdf.device, copy=True)
    n, Ki, E = views.inverse_cameras(who, intrinsics, extrinsics)
    if n > _lib.RENDER_MAX_VIEWS:
        raise ValueError('render_views: at most {} views per call'.format(_lib.RENDER_MAX_VIEWS))
    h, w = int(shape[0]), int(shape[1])
    org = _origin_array(origin)
    dev = tsdf.device
    depth = torch.empty((n, h, w), dtype=torch.float32, device=dev)
    nrm = torch.empty((n, h, w, 3), dtype=torch.float32, device=dev) if normals else None
    labels = torch.empty((n, h, w), dtype=torch.uint8, device=dev) if ids is not None else None
    X, Y, Z = tsdf.shape
    rc = lib.ojf_render(_lib.ptr(tsdf), _lib.ptr(weights), _lib.ptr(ids), X, Y, Z, org.ctypes.data, float(resolution), n,
                        Ki.ctypes.data, E.ctypes.data, h, w, float(near), _lib.ptr(depth), _lib.ptr(nrm), _lib.ptr(labels),
                        _lib.stream_ptr(dev))
    _lib.check(rc, 'ojf_render')
    return {'depth': depth, 'normals': nrm, 'labels': labels}
