"""Classical projective TSDF fusion (Curless-Levoy / KinectFusion style): depth maps go into the fp16 volumes by a running
weighted mean of the projective distance, without a network.  The kernel is csrc/ojf_projective.hip
(``ojf_fuse_projective``); its fp32 definition is written in that file's header and restated in numpy by
tests/projective_ref.py.  The reference has no counterpart: every path of its into a volume runs through FusionNet.

The volume frame is the one extract, integrate and render use (voxel (i,j,k) centred at origin + (i+0.5, j+0.5,
k+0.5)·res).  Depth is the camera z-depth; 0, negative and non-finite pixels carry no depth.
"""
import numpy as np
import torch

from . import _lib
from .ops import _origin_array


def _cameras(intrinsics, extrinsics, n):
    """(K f64[n,9], E f64[n,12]) from [3,3] / [n,3,3] intrinsics and [3,4] / [4,4] / [n,3,4] / [n,4,4] extrinsics (numpy or
    torch, any float type); a single matrix serves every view."""
    K = torch.as_tensor(intrinsics).detach().cpu().to(torch.float64)
    E = torch.as_tensor(extrinsics).detach().cpu().to(torch.float64)
    if K.dim() == 2:
        K = K.unsqueeze(0)
    if E.dim() == 2:
        E = E.unsqueeze(0)
    if K.dim() != 3 or E.dim() != 3 or K.shape[-2:] != (3, 3) or E.shape[-1] != 4 or E.shape[-2] not in (3, 4):
        raise ValueError('integrate_depth: intrinsics [n,]3x3 and extrinsics [n,]3x4 or 4x4 expected, got {} and {}'.format(
            tuple(K.shape), tuple(E.shape)))
    if K.shape[0] not in (1, n) or E.shape[0] not in (1, n):
        raise ValueError('integrate_depth: {} intrinsics and {} extrinsics for {} depth maps'.format(K.shape[0], E.shape[0], n))
    K = K.expand(n, 3, 3).reshape(n, 9)
    E = E[:, :3, :].expand(n, 3, 4).reshape(n, 12)
    return np.ascontiguousarray(K.numpy()), np.ascontiguousarray(E.numpy())


def _images(x, name, dtype, n, h, w, dev):
    if x is None:
        return None
    if not (torch.is_tensor(x) and x.device == dev):
        raise ValueError('integrate_depth: {} must be a tensor on the volume\'s device'.format(name))
    if x.numel() != n * h * w:
        raise ValueError('integrate_depth: {} has {} elements for {} depth maps of {}x{}'.format(name, x.numel(), n, h, w))
    if dtype == torch.uint8 and x.dtype == torch.bool:
        x = x.contiguous().view(torch.uint8)
    return x.to(dtype).reshape(n, h, w).contiguous()


def integrate_depth(tsdf, weights, *, origin, resolution, depth, intrinsics, extrinsics, mask=None, ids=None, scores=None,
                    labels=None, label_scores=None, truncation, max_weight=128.0, near=0.0, carve=False):
    """Fuse ``n`` depth views into device volumes in place, on the current stream of the volumes' device.

    tsdf, weights: cuda fp16 [X,Y,Z], contiguous; ids (u8) / scores (fp16) [X,Y,Z] and labels u8 [n,h,w]: all given or all
    None; label_scores f32 [n,h,w] or None (every label scores 1).  depth: cuda f32 [h,w] or [n,h,w]; mask: bool / u8 of
    the same shape or None; intrinsics [3,3] or [n,3,3], extrinsics (camera-to-world) [3,4] / [4,4] or [n,...] - the batch
    dict's entries will do.  truncation: width of the band behind and in front of the surface (m); max_weight: where the
    running mean's weight saturates (1..2048); near: smallest camera depth of a voxel that is updated; carve: also pull
    the free space in front of the surface to +truncation.  The views are fused in order; more than
    ``_lib.PROJECTIVE_MAX_VIEWS`` go in several kernel calls, with the same bits as one view per call."""
    _lib.require_gpu()
    lib = _lib.load()
    if not (torch.is_tensor(tsdf) and tsdf.is_cuda and tsdf.dtype == torch.float16 and tsdf.dim() == 3 and tsdf.is_contiguous()):
        raise ValueError('integrate_depth: tsdf must be a contiguous cuda fp16 [X,Y,Z] tensor (it is updated in place)')
    dev = tsdf.device
    for vol, dt, name in ((weights, torch.float16, 'weights'), (ids, torch.uint8, 'ids'), (scores, torch.float16, 'scores')):
        if vol is None and name != 'weights':
            continue
        if not (torch.is_tensor(vol) and vol.device == dev and vol.dtype == dt and vol.shape == tsdf.shape and vol.is_contiguous()):
            raise ValueError('integrate_depth: {} must be a contiguous {} tensor of the volume\'s shape and device'.format(name, dt))
    if (ids is None) != (scores is None) or (ids is None) != (labels is None):
        raise ValueError('integrate_depth: ids, scores and labels are all given or all None')
    if label_scores is not None and labels is None:
        raise ValueError('integrate_depth: label_scores without labels')
    if not (torch.is_tensor(depth) and depth.device == dev and depth.dim() in (2, 3)):
        raise ValueError('integrate_depth: depth must be a [h,w] or [n,h,w] tensor on the volume\'s device')
    depth = depth.to(torch.float32)
    if depth.dim() == 2:
        depth = depth.unsqueeze(0)
    depth = depth.contiguous()
    n, h, w = depth.shape
    if n < 1:
        raise ValueError('integrate_depth: no depth map')
    truncation, max_weight, near = float(truncation), float(max_weight), float(near)
    if not (0.0 < truncation < float('inf')) or not (1.0 <= max_weight <= 2048.0) or not (0.0 <= near < float('inf')):
        raise ValueError('integrate_depth: truncation > 0, 1 <= max_weight <= 2048 and near >= 0 expected, got {}, {}, {}'.format(
            truncation, max_weight, near))
    K, E = _cameras(intrinsics, extrinsics, n)
    if not (np.isfinite(K).all() and np.isfinite(E).all()):
        raise ValueError('integrate_depth: non-finite intrinsics or extrinsics')
    if np.any(K[:, [1, 3, 6, 7]] != 0.0) or np.any(K[:, 8] != 1.0):
        raise ValueError('integrate_depth: pinhole intrinsics [fx 0 cx; 0 fy cy; 0 0 1] expected')
    mask = _images(mask, 'mask', torch.uint8, n, h, w, dev)
    labels = _images(labels, 'labels', torch.uint8, n, h, w, dev)
    label_scores = _images(label_scores, 'label_scores', torch.float32, n, h, w, dev)
    org = _origin_array(origin)
    X, Y, Z = tsdf.shape
    stream = _lib.stream_ptr(dev)
    step = _lib.PROJECTIVE_MAX_VIEWS
    for v0 in range(0, n, step):
        v1 = min(n, v0 + step)
        Kc, Ec = np.ascontiguousarray(K[v0:v1]), np.ascontiguousarray(E[v0:v1])
        part = lambda t: None if t is None else t[v0:v1]  # noqa: E731  (leading-axis slices of contiguous images are contiguous)
        rc = lib.ojf_fuse_projective(_lib.ptr(tsdf), _lib.ptr(weights), _lib.ptr(ids), _lib.ptr(scores), X, Y, Z,
                                     org.ctypes.data, float(resolution), v1 - v0, Kc.ctypes.data, Ec.ctypes.data,
                                     _lib.ptr(part(depth)), _lib.ptr(part(mask)), _lib.ptr(part(labels)),
                                     _lib.ptr(part(label_scores)), h, w, float(truncation), float(max_weight), float(near),
                                     int(bool(carve)), stream)
        _lib.check(rc, 'ojf_fuse_projective')
