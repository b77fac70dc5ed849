"""Ray casting of a fused volume: depth, normal and label images of the model as a camera would see it (KinectFusion
style).  The kernel is csrc/ojf_render.hip (``ojf_render``); its fp32 definition is written in that file's header and
restated in numpy by tests/render_ref.py.  The reference has no counterpart on its hot path.

The volume frame is the one extract and integrate use (voxel (i,j,k) centred at origin + (i+0.5, j+0.5, k+0.5)·res),
not the mesh frame of ``Database.get_mesh``.  The returned depth is the camera z-depth, 0 where the ray hits nothing -
the same convention as the input depth maps.
"""
import numpy as np
import torch

from . import _lib
from .ops import camera_arrays, _origin_array


def _poses(intrinsics, extrinsics):
    """(n, Kinv f32[n,9], E f32[n,12]) from [3,3] / [n,3,3] intrinsics and [3,4] / [4,4] / [n,3,4] / [n,4,4]
    extrinsics (numpy or torch, any float type); a single intrinsics matrix serves every pose."""
    K = torch.as_tensor(intrinsics).detach().cpu()
    E = torch.as_tensor(extrinsics).detach().cpu()
    if K.dim() == 2:
        K = K.unsqueeze(0)
    if E.dim() == 2:
        E = E.unsqueeze(0)
    if K.shape[-2:] != (3, 3) or E.shape[-1] != 4 or E.shape[-2] not in (3, 4):
        raise ValueError('render: intrinsics [n,]3x3 and extrinsics [n,]3x4 or 4x4 expected, got {} and {}'.format(
            tuple(K.shape), tuple(E.shape)))
    n = max(K.shape[0], E.shape[0])
    if K.shape[0] not in (1, n) or E.shape[0] not in (1, n):
        raise ValueError('render: {} intrinsics for {} poses'.format(K.shape[0], E.shape[0]))
    Ki, Ew = np.empty((n, 9), np.float32), np.empty((n, 12), np.float32)
    for i in range(n):
        Ki[i], Ew[i] = camera_arrays(K[i if K.shape[0] > 1 else 0], E[i if E.shape[0] > 1 else 0])
    return n, Ki, Ew


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
    if not (torch.is_tensor(tsdf) and tsdf.is_cuda and tsdf.dtype == torch.float16 and tsdf.dim() == 3):
        raise ValueError('render_views: tsdf must be a cuda fp16 [X,Y,Z] tensor')
    tsdf = tsdf.contiguous()
    for vol, dt, name in ((weights, torch.float16, 'weights'), (ids, torch.uint8, 'ids')):
        if vol is not None and not (torch.is_tensor(vol) and vol.device == tsdf.device and vol.dtype == dt
                                    and vol.shape == tsdf.shape):
            raise ValueError('render_views: {} must be a {} tensor of the volume\'s shape and device'.format(name, dt))
    weights = None if weights is None else weights.contiguous()
    ids = None if ids is None else ids.contiguous()
    n, Ki, E = _poses(intrinsics, extrinsics)
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
