"""The live depth frame made ready for tracking and fusion (KinectFusion's first stage): validity, rejection of the mixed
pixels at depth edges, a bilateral filter, the camera-space normal map and an incidence-angle test, for ``n`` frames in one
kernel launch.  The kernel is csrc/ojf_frames.hip (``ojf_depth_prepare``); its fp32 definition is written in that file's
header and restated in numpy by tests/frames_ref.py.  The reference only erodes its depth maps (deps/mesh-fusion/2_fusion.py).

A pixel that a stage drops comes out as depth 0, which every operator that takes a depth frame reads as "no depth": the
result goes into ``integrate_depth``, ``integrate_depth_hist``, ``integrate_color``, ``integrate_label_probs`` and
``track_frame`` as it is (their ``filter=`` keyword on ``Database`` does exactly that).
"""
import math

import numpy as np
import torch

from . import views

MAX_RADIUS = 4  # csrc/ojf_frames.hip kMaxRadius
OPTIONS = ('radius', 'sigma_space', 'range0', 'range2', 'edge_abs', 'edge_rel', 'near', 'far', 'max_angle')  # of a ``filter=`` dict


def spatial_table(radius, sigma_space):
    """The f32 [(2·radius+1)²] spatial weights of the bilateral window, row-major: exp(-(dr² + dc²) / (2 sigma²)) evaluated
    in f64 and rounded once (the centre is exactly 1)."""
    ax = np.arange(-radius, radius + 1, dtype=np.float64)
    d2 = ax[:, None] ** 2 + ax[None, :] ** 2
    return np.ascontiguousarray(np.exp(-d2 / (2.0 * float(sigma_space) ** 2)).astype(np.float32).reshape(-1))


def frame_intrinsics(K):
    """f32 [n,4] (1/fx, 1/fy, cx, cy) of the f64 [n,9] intrinsics ``views.cameras`` returns: the reciprocals are formed in
    f64 and rounded once."""
    return np.ascontiguousarray(np.stack([1.0 / K[:, 0], 1.0 / K[:, 4], K[:, 2], K[:, 5]], axis=1).astype(np.float32))


def options(radius=2, sigma_space=1.5, *, range0, range2=0.0, edge_abs=0.0, edge_rel=0.0, near=0.0, far=float('inf'), max_angle=None):
    """The checked scalar options of ``prepare_depth`` as the kernel takes them: dict(radius, spatial f32 table or None,
    range0, range2, edge_abs, edge_rel, near, far, cos_min).  Needs no device."""
    who = 'prepare_depth'
    if isinstance(radius, bool) or int(radius) != radius or not 0 <= int(radius) <= MAX_RADIUS:
        raise ValueError('{}: radius must be an integer in 0..{}, got {!r}'.format(who, MAX_RADIUS, radius))
    radius = int(radius)
    sigma_space, range0, range2, edge_abs, edge_rel, near, far = (float(x) for x in (sigma_space, range0, range2, edge_abs, edge_rel,
                                                                                        near, far))
    if not 0.0 < sigma_space < float('inf'):
        raise ValueError('{}: sigma_space must be > 0 and finite, got {}'.format(who, sigma_space))
    if not (0.0 < range0 < float('inf') and 0.0 <= range2 < float('inf')):
        raise ValueError('{}: range0 > 0 and range2 >= 0, both finite, expected, got {} and {}'.format(who, range0, range2))
    if not (0.0 <= edge_abs < float('inf') and 0.0 <= edge_rel < float('inf')):
        raise ValueError('{}: edge_abs >= 0 and edge_rel >= 0, both finite, expected, got {} and {}'.format(who, edge_abs, edge_rel))
    if not (0.0 <= near < float('inf') and near <= far):
        raise ValueError('{}: 0 <= near <= far and a finite near expected, got {} and {}'.format(who, near, far))
    cos_min = 0.0
    if max_angle is not None:
        max_angle = float(max_angle)
        if not 0.0 < max_angle <= 90.0:
            raise ValueError('{}: max_angle must be in (0, 90] degrees or None, got {}'.format(who, max_angle))
        cos_min = max(float(np.float32(math.cos(math.radians(max_angle)))), float(np.finfo(np.float32).tiny))  # never 0: 0 is "off"
    return dict(radius=radius, spatial=spatial_table(radius, sigma_space) if radius else None, range0=range0, range2=range2,
                edge_abs=edge_abs, edge_rel=edge_rel, near=near, far=far, cos_min=cos_min)


def prepare_depth(depth, *, intrinsics=None, mask=None, radius=2, sigma_space=1.5, range0, range2=0.0, edge_abs=0.0, edge_rel=0.0,
                  near=0.0, far=float('inf'), max_angle=None, normals=False):
    """Filter ``n`` depth frames on the current stream of their device, in one launch and without synchronising.

    depth: cuda [h,w] or [n,h,w] metric z-depth; mask: bool / u8 of the depth's shape or None; intrinsics [3,3] or [n,3,3]
    (needed for ``normals`` and ``max_angle`` only).  In this order: a pixel is valid if it is finite, near <= d <= far and
    the mask is set (with near = 0 a depth of exactly 0 counts as a measurement: give the frame's mask or a near > 0);
    a valid pixel with a valid 8-neighbour further than ``edge_abs + edge_rel·d`` metres in depth is dropped (the mixed pixels
    of a depth edge; off when both are 0); the rest goes through a bilateral filter of ``radius`` 0..4 pixels (0 copies),
    spatial Gaussian ``sigma_space`` pixels and range kernel (1 - t²)² for |t| < 1, t = (d_n - d) / (range0 + range2·d²) - the
    range width in metres, range2 for a sensor whose noise grows with d²; camera-space unit normals of the filtered frame
    that face the camera; a pixel seen under more than ``max_angle`` degrees from its normal, or without a normal, is dropped
    (None: off).  Returns {'depth' f32 [n,h,w] (0 where not valid), 'valid' bool [n,h,w], 'normals' f32 [n,h,w,3] or None
    (0 where not valid)}; the input is not touched."""
    who = 'prepare_depth'
    o = options(radius, sigma_space, range0=range0, range2=range2, edge_abs=edge_abs, edge_rel=edge_rel, near=near, far=far,
                max_angle=max_angle)
    if not torch.is_tensor(depth) or not depth.is_cuda:
        raise ValueError('{}: depth must be a [h,w] or [n,h,w] cuda tensor'.format(who))
    dev = depth.device
    depth = views.depth_frames(who, depth, dev)
    n, h, w = depth.shape
    if h < 1 or w < 1 or depth.numel() >= 2 ** 31:
        raise ValueError('{}: 1 <= n·h·w < 2^31 expected, got shape {}'.format(who, tuple(depth.shape)))
    mask = views.images(who, mask, 'mask', torch.uint8, n, h, w, dev)
    K = None
    if normals or o['cos_min'] != 0.0:
        if intrinsics is None:
            raise ValueError('{}: normals and max_angle need intrinsics'.format(who))
        K = frame_intrinsics(views.cameras(who, intrinsics, np.eye(4), n, nonzero_focal=True)[1])
    from . import _lib
    _lib.require_gpu()
    lib = _lib.load()
    out = torch.empty_like(depth)
    valid = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    nrm = torch.empty((n, h, w, 3), dtype=torch.float32, device=dev) if normals else None
    rc = lib.ojf_depth_prepare(_lib.ptr(depth), _lib.ptr(mask), n, h, w, _lib.ptr(K), o['radius'], _lib.ptr(o['spatial']), o['range0'],
                               o['range2'], o['edge_abs'], o['edge_rel'], o['near'], o['far'], o['cos_min'], _lib.ptr(out),
                               _lib.ptr(valid), _lib.ptr(nrm), _lib.stream_ptr(dev))
    _lib.check(rc, 'ojf_depth_prepare')
    return {'depth': out, 'valid': valid.view(torch.bool), 'normals': nrm}


def check_filter(filter):
    """Refuse what is no ``filter=`` dict: keys among ``OPTIONS``, range0 given, values ``options`` accepts.  Needs no device."""
    if not isinstance(filter, dict) or not set(filter) <= set(OPTIONS) or 'range0' not in filter:
        raise ValueError('prepare_depth: filter must be a dict with range0 and keys among {}, got {!r}'.format(', '.join(OPTIONS), filter))
    options(**filter)


def filtered(depth, mask, intrinsics, filter):
    """(depth, mask) of an operator's ``filter=`` keyword: the frames and their mask through ``prepare_depth`` with the
    options of the dict ``filter`` (``OPTIONS``) and the call's own intrinsics; the mask that comes back is the validity.  A
    single [h,w] frame comes back as [h,w]."""
    check_filter(filter)
    out = prepare_depth(depth, intrinsics=intrinsics if filter.get('max_angle') is not None else None, mask=mask, **filter)
    if depth.dim() == 2:
        return out['depth'][0], out['valid'][0]
    return out['depth'], out['valid']
