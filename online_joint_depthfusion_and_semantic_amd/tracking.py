"""Camera tracking against the fused volume: the pose of a depth frame by frame-to-model projective point-to-plane ICP
(KinectFusion style).  The model is ray-cast once per pyramid level at a reference pose (render.py), then ``ojf_track``
(csrc/ojf_track.hip) builds the depth pyramid of the live frame and runs every Gauss-Newton iteration on the device; its
fp32 / fp64 definition is written in that file's header and restated in numpy by tests/track_ref.py.  The reference has
no counterpart: it takes every pose from its dataset.

``track_frame_rgbd`` adds a photometric term against colour images of the model (``color.render_color`` at the depths of the
same ray casts; ``ojf_track_rgbd``, csrc/ojf_track_rgbd.hip, restated by tests/track_rgbd_ref.py): it pins the freedoms
geometry leaves open, a view of a single plane first of all.
"""
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from .ops import camera_arrays
from .render import render_views


def level_intrinsics(intrinsics, level):
    """K_l f64[3,3] of pyramid level ``level``: fx/2^l, fy/2^l, (cx + 0.5)/2^l - 0.5, (cy + 0.5)/2^l - 0.5 (pixel centres
    of a 2x2 block average onto the centre of the coarse pixel)."""
    K = np.asarray(torch.as_tensor(intrinsics).detach().cpu().numpy(), dtype=np.float64).reshape(3, 3)
    s = float(1 << level)
    return np.array([[K[0, 0] / s, 0.0, (K[0, 2] + 0.5) / s - 0.5],
                     [0.0, K[1, 1] / s, (K[1, 2] + 0.5) / s - 0.5],
                     [0.0, 0.0, 1.0]], dtype=np.float64)


def pose12(extrinsics):
    """First three rows of a [3,4] / [4,4] camera-to-world pose (numpy or torch) as f64[12]."""
    E = torch.as_tensor(extrinsics).detach().cpu().to(torch.float64).reshape(-1, 4)[:3]
    return np.ascontiguousarray(E.numpy().reshape(12))


# defaults of the photometric term: lambda in metres per intensity level and the hard cut in intensity levels (DESIGN.md
# section 25 has the sweep they come from)
PHOTO_WEIGHT, PHOTO_THRESH = 0.002, 40.0


def _frame_and_model(who, tsdf, weights, origin, resolution, depth, intrinsics, extrinsics, reference_extrinsics, mask,
                     levels, iterations, more=None):
    """What both trackers do before their library call (``who`` names the caller in messages): the checked levels and
    iteration counts, depth and mask on the volume's device, the poses, K0 and Kinv_l, the model's ray casts per level -
    ``more(K_l, E_ref [3,4], model depth)``, if given, adds one more model image per level - and the output buffer.
    ``maps[k]`` holds the device addresses of the k-th model image of every level (depth, normals, then ``more``'s)."""
    _lib.require_gpu()
    a = SimpleNamespace(levels=int(levels))
    if not 1 <= a.levels <= _lib.TRACK_MAX_LEVELS:
        raise ValueError('{}: levels must be 1..{}'.format(who, _lib.TRACK_MAX_LEVELS))
    its = [int(i) for i in iterations]
    if len(its) < a.levels:
        raise ValueError('{}: {} iteration counts for {} levels'.format(who, len(its), a.levels))
    a.its = np.ascontiguousarray(its[:a.levels], dtype=np.int32)
    if not (torch.is_tensor(tsdf) and tsdf.is_cuda):
        raise ValueError('{}: tsdf must be a cuda fp16 [X,Y,Z] tensor'.format(who))
    a.dev = tsdf.device
    d = torch.as_tensor(depth)
    a.depth = d.to(device=a.dev, dtype=torch.float32).reshape(d.shape[-2:]).contiguous()
    a.h, a.w = int(a.depth.shape[0]), int(a.depth.shape[1])
    a.mask = None
    if mask is not None:
        m = torch.as_tensor(mask).to(device=a.dev).reshape(a.h, a.w)
        a.mask = (m != 0).to(torch.uint8).contiguous()
    a.E_init = pose12(extrinsics)
    a.E_ref = a.E_init if reference_extrinsics is None else pose12(reference_extrinsics)
    if not (np.isfinite(a.E_init).all() and np.isfinite(a.E_ref).all()):
        raise ValueError('{}: the initial and reference poses must be finite'.format(who))
    a.K0 = np.ascontiguousarray(np.asarray(torch.as_tensor(intrinsics).detach().cpu().numpy(), dtype=np.float64).reshape(9))
    a.Kinv = np.empty((a.levels, 9), np.float32)
    E = a.E_ref.reshape(3, 4)
    a.model = []  # the images themselves, alive until the call is enqueued
    for l in range(a.levels):
        Kl = level_intrinsics(a.K0.reshape(3, 3), l)
        a.Kinv[l] = camera_arrays(Kl, E)[0]
        out = render_views(tsdf, weights, None, origin=origin, resolution=resolution, intrinsics=Kl, extrinsics=E,
                           shape=(a.h >> l, a.w >> l))
        a.model.append((out['depth'], out['normals']) + (() if more is None else (more(Kl, E, out['depth']),)))
    a.maps = [np.array([_lib.ptr(x) for x in images], dtype=np.uint64) for images in zip(*a.model)]
    a.n_it = int(a.its.sum())
    # pose f64[12] | stats f64[n_it, 4] | status int32[2]: one buffer, one copy back
    a.out = torch.empty(12 + 4 * a.n_it + 1, dtype=torch.float64, device=a.dev)
    a.out_ptrs = (a.out.data_ptr(), a.out.data_ptr() + 8 * 12, a.out.data_ptr() + 8 * (12 + 4 * a.n_it))
    return a


def _result(a):
    """The result dictionary of both trackers from the output buffer of ``_frame_and_model``: the call's one copy back."""
    host = a.out.cpu().numpy()
    status = int(host[12 + 4 * a.n_it:].view(np.int32)[0])
    E = np.eye(4)
    E[:3] = host[:12].reshape(3, 4)
    return {'extrinsics': E, 'ok': status == 0, 'status': status,
            'stats': host[12:12 + 4 * a.n_it].reshape(a.n_it, 4).copy()}


def track_frame(tsdf, weights, *, origin, resolution, depth, intrinsics, extrinsics, reference_extrinsics=None, mask=None,
                levels=3, iterations=(10, 5, 4), dist_thresh=0.1, angle_thresh=20.0, pyramid_delta=0.03,
                min_inlier_fraction=0.05):
    """Track one depth frame against a device volume on the current stream of the volume's device.

    tsdf / weights: cuda fp16 [X,Y,Z] (weights None: every voxel observed; with weights, unobserved voxels are
    transparent to the ray casts); depth [h,w] metric z-depth (0 or non-finite: none), mask [h,w] or None;
    intrinsics [3,3]; extrinsics: the camera-to-world pose tracking starts from ([3,4] or [4,4]); reference_extrinsics:
    the pose the model is rendered at (default ``extrinsics``); iterations[l]: Gauss-Newton steps at level l (level 0 is
    the input resolution; levels run coarsest first).
    Returns {'extrinsics': f64 [4,4] numpy camera-to-world, 'ok': bool, 'status': int (0 ok, 1 too few inliers, 2 singular
    system, 3 non-finite step), 'stats': f64 [sum(iterations), 4] numpy (inlier count, mean squared residual, |omega|,
    |tau|)}.  On failure the pose is ``extrinsics`` unchanged.  Copying these back is the call's only synchronisation."""
    a = _frame_and_model('track_frame', tsdf, weights, origin, resolution, depth, intrinsics, extrinsics,
                         reference_extrinsics, mask, levels, iterations)
    lib = _lib.load()
    ws = torch.empty(int(lib.ojf_track_workspace_bytes(a.h, a.w, a.levels)), dtype=torch.uint8, device=a.dev)
    rc = lib.ojf_track(_lib.ptr(a.depth), _lib.ptr(a.mask), a.h, a.w, a.levels, a.K0.ctypes.data, a.Kinv.ctypes.data,
                       a.maps[0].ctypes.data, a.maps[1].ctypes.data, a.E_ref.ctypes.data, a.E_init.ctypes.data,
                       a.its.ctypes.data, float(dist_thresh), float(angle_thresh), float(pyramid_delta),
                       float(min_inlier_fraction), _lib.ptr(ws), ws.numel(), *a.out_ptrs, _lib.stream_ptr(a.dev))
    _lib.check(rc, 'ojf_track')
    return _result(a)


def track_frame_rgbd(tsdf, weights, colors, *, origin, resolution, image, depth, intrinsics, extrinsics,
                     reference_extrinsics=None, mask=None, levels=3, iterations=(10, 5, 4), dist_thresh=0.1, angle_thresh=20.0,
                     pyramid_delta=0.03, min_inlier_fraction=0.05, photo_weight=PHOTO_WEIGHT, photo_thresh=PHOTO_THRESH,
                     grad_depth_limit=None):
    """``track_frame`` with a photometric term: one depth + colour frame against a device volume and its colour volume.

    colors: cuda fp16 [X,Y,Z,4] (color.py); image: u8 [h,w,3|4] or float [3,h,w] on the 0..255 scale, on the volume's device
    or on the host; photo_weight: metres per intensity level (0: no photometric rows, ``track_frame``'s bits); photo_thresh:
    a photometric residual beyond it (intensity levels) is cut; grad_depth_limit: a model intensity gradient counts only
    where the model depth of the neighbours is within it of the centre's (default ``dist_thresh``).  Everything else, the
    result included, as ``track_frame``: the inlier count of 'stats' counts pixels with a geometric or a photometric row."""
    from . import color

    def model_color(Kl, E, mdepth):
        return color.render_color(colors, origin=origin, resolution=resolution, intrinsics=Kl, extrinsics=E, depth=mdepth)
    a = _frame_and_model('track_frame_rgbd', tsdf, weights, origin, resolution, depth, intrinsics, extrinsics,
                         reference_extrinsics, mask, levels, iterations, model_color)
    lib = _lib.load()
    img = torch.as_tensor(image)
    if img.dim() == 4 and img.shape[0] == 1:
        img = img[0]
    img = color.pack_image(img.to(a.dev), 1, a.h, a.w, a.dev)
    ws = torch.empty(int(lib.ojf_track_rgbd_workspace_bytes(a.h, a.w, a.levels)), dtype=torch.uint8, device=a.dev)
    grad = float(dist_thresh if grad_depth_limit is None else grad_depth_limit)
    rc = lib.ojf_track_rgbd(_lib.ptr(a.depth), _lib.ptr(a.mask), _lib.ptr(img), a.h, a.w, a.levels, a.K0.ctypes.data,
                            a.Kinv.ctypes.data, a.maps[0].ctypes.data, a.maps[1].ctypes.data, a.maps[2].ctypes.data,
                            a.E_ref.ctypes.data, a.E_init.ctypes.data, a.its.ctypes.data, float(dist_thresh),
                            float(angle_thresh), float(pyramid_delta), float(min_inlier_fraction), float(photo_weight),
                            float(photo_thresh), grad, _lib.ptr(ws), ws.numel(), *a.out_ptrs, _lib.stream_ptr(a.dev))
    _lib.check(rc, 'ojf_track_rgbd')
    return _result(a)
