"""Classical projective TSDF fusion (Curless-Levoy / KinectFusion style): depth maps go into the fp16 volumes by a running
weighted mean of the projective distance, without a network.  The kernel is csrc/ojf_projective.hip
(``ojf_fuse_projective``); its fp32 definition is written in that file's header and restated in numpy by
tests/projective_ref.py.  The reference has no counterpart: every path of its into a volume runs through FusionNet.

The volume frame is the one extract, integrate and render use (voxel (i,j,k) centred at origin + (i+0.5, j+0.5,
k+0.5)·res).  Depth is the camera z-depth; 0, negative and non-finite pixels carry no depth.
"""
import torch

from . import _lib, views
from .ops import _origin_array


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
    who = 'integrate_depth'
    _lib.require_gpu()
    lib = _lib.load()
    tsdf = views.volume3(who, tsdf, 'tsdf', torch.float16)  # (updated in place: never a copy)
    dev = tsdf.device
    for vol, dt, name in ((weights, torch.float16, 'weights'), (ids, torch.uint8, 'ids'), (scores, torch.float16, 'scores')):
        if vol is not None or name == 'weights':
            views.volume3(who, vol, name, dt, tsdf.shape, dev)
    if (ids is None) != (scores is None) or (ids is None) != (labels is None):
        raise ValueError('integrate_depth: ids, scores and labels are all given or all None')
    if label_scores is not None and labels is None:
        raise ValueError('integrate_depth: label_scores without labels')
    depth = views.depth_frames(who, depth, dev)
    n, h, w = depth.shape
    truncation, max_weight, near = views.running_mean_options(who, 'truncation', truncation, max_weight, near)
    n, K, E = views.cameras(who, intrinsics, extrinsics, n)
    mask = views.images(who, mask, 'mask', torch.uint8, n, h, w, dev)
    labels = views.images(who, labels, 'labels', torch.uint8, n, h, w, dev)
    label_scores = views.images(who, label_scores, 'label_scores', torch.float32, n, h, w, dev)
    org = _origin_array(origin)
    X, Y, Z = tsdf.shape
    stream = _lib.stream_ptr(dev)
    for v0, v1, Kc, Ec in views.chunks(n, _lib.PROJECTIVE_MAX_VIEWS, K, E):
        rc = lib.ojf_fuse_projective(_lib.ptr(tsdf), _lib.ptr(weights), _lib.ptr(ids), _lib.ptr(scores), X, Y, Z,
                                     org.ctypes.data, float(resolution), v1 - v0, Kc.ctypes.data, Ec.ctypes.data,
                                     _lib.ptr(depth[v0:v1]), _lib.ptr(views.part(mask, v0, v1)),
                                     _lib.ptr(views.part(labels, v0, v1)), _lib.ptr(views.part(label_scores, v0, v1)), h, w,
                                     truncation, max_weight, near, int(bool(carve)), stream)
        _lib.check(rc, 'ojf_fuse_projective')
