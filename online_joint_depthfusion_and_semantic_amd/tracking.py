"""Camera tracking against the fused volume: the pose of a depth frame by frame-to-model projective point-to-plane ICP
(KinectFusion style).  The model is ray-cast once per pyramid level at a reference pose (render.py), then ``ojf_track``
(csrc/ojf_track.hip) builds the depth pyramid of the live frame and runs every Gauss-Newton iteration on the device; its
fp32 / fp64 definition is written in that file's header and restated in numpy by tests/track_ref.py.  The reference has
no counterpart: it takes every pose from its dataset.

``track_frame_rgbd`` adds a photometric term against colour images of the model (``color.render_color`` at the depths of the
same ray casts; ``ojf_track_rgbd``, csrc/ojf_track_rgbd.hip, restated by tests/track_rgbd_ref.py): it pins the freedoms
geometry leaves open, a view of a single plane first of all.
"""
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
    _lib.require_gpu()
    lib = _lib.load()
    levels = int(levels)
    if not 1 <= levels <= _lib.TRACK_MAX_LEVELS:
        raise ValueError('track_frame: levels must be 1..{}'.format(_lib.TRACK_MAX_LEVELS))
    its = [int(i) for i in iterations]
    if len(its) < levels:
        raise ValueError('track_frame: {} iteration counts for {} levels'.format(len(its), levels))
    its = np.ascontiguousarray(its[:levels], dtype=np.int32)
    if not (torch.is_tensor(tsdf) and tsdf.is_cuda):
        raise ValueError('track_frame: tsdf must be a cuda fp16 [X,Y,Z] tensor')
    dev = tsdf.device
    d = torch.as_tensor(depth)
    d = d.to(device=dev, dtype=torch.float32).reshape(d.shape[-2:]).contiguous()
    h, w = int(d.shape[0]), int(d.shape[1])
    m = None
    if mask is not None:
        m = torch.as_tensor(mask).to(device=dev).reshape(h, w)
        m = (m != 0).to(torch.uint8).contiguous()
    E_init = pose12(extrinsics)
    E_ref = E_init if reference_extrinsics is None else pose12(reference_extrinsics)
    if not (np.isfinite(E_init).all() and np.isfinite(E_ref).all()):
        raise ValueError('track_frame: the initial and reference poses must be finite')
    K0 = np.ascontiguousarray(np.asarray(torch.as_tensor(intrinsics).detach().cpu().numpy(), dtype=np.float64).reshape(9))
    Kinv = np.empty((levels, 9), np.float32)
    model = []
    for l in range(levels):
        Kl = level_intrinsics(K0.reshape(3, 3), l)
        Kinv[l] = camera_arrays(Kl, E_ref.reshape(3, 4))[0]
        out = render_views(tsdf, weights, None, origin=origin, resolution=resolution, intrinsics=Kl,
                           extrinsics=E_ref.reshape(3, 4), shape=(h >> l, w >> l))
        model.append((out['depth'], out['normals']))
    mdepth = np.array([_lib.ptr(md) for md, _ in model], dtype=np.uint64)
    mnorm = np.array([_lib.ptr(mn) for _, mn in model], dtype=np.uint64)
    n_it = int(its.sum())
    ws = torch.empty(int(lib.ojf_track_workspace_bytes(h, w, levels)), dtype=torch.uint8, device=dev)
    # pose f64[12] | stats f64[n_it, 4] | status int32[2]: one buffer, one copy back
    out = torch.empty(12 + 4 * n_it + 1, dtype=torch.float64, device=dev)
    status_ptr = out.data_ptr() + 8 * (12 + 4 * n_it)
    rc = lib.ojf_track(_lib.ptr(d), _lib.ptr(m), h, w, levels, K0.ctypes.data, Kinv.ctypes.data, mdepth.ctypes.data,
                       mnorm.ctypes.data, E_ref.ctypes.data, E_init.ctypes.data, its.ctypes.data, float(dist_thresh),
                       float(angle_thresh), float(pyramid_delta), float(min_inlier_fraction), _lib.ptr(ws), ws.numel(),
                       out.data_ptr(), out.data_ptr() + 8 * 12, status_ptr, _lib.stream_ptr(dev))
    _lib.check(rc, 'ojf_track')
    host = out.cpu().numpy()
    status = int(host[12 + 4 * n_it:].view(np.int32)[0])
    E = np.eye(4)
    E[:3] = host[:12].reshape(3, 4)
    return {'extrinsics': E, 'ok': status == 0, 'status': status, 'stats': host[12:12 + 4 * n_it].reshape(n_it, 4).copy()}


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
    _lib.require_gpu()
    lib = _lib.load()
    levels = int(levels)
    if not 1 <= levels <= _lib.TRACK_MAX_LEVELS:
        raise ValueError('track_frame_rgbd: levels must be 1..{}'.format(_lib.TRACK_MAX_LEVELS))
    its = [int(i) for i in iterations]
    if len(its) < levels:
        raise ValueError('track_frame_rgbd: {} iteration counts for {} levels'.format(len(its), levels))
    its = np.ascontiguousarray(its[:levels], dtype=np.int32)
    if not (torch.is_tensor(tsdf) and tsdf.is_cuda):
        raise ValueError('track_frame_rgbd: tsdf must be a cuda fp16 [X,Y,Z] tensor')
    dev = tsdf.device
    d = torch.as_tensor(depth)
    d = d.to(device=dev, dtype=torch.float32).reshape(d.shape[-2:]).contiguous()
    h, w = int(d.shape[0]), int(d.shape[1])
    m = None
    if mask is not None:
        m = torch.as_tensor(mask).to(device=dev).reshape(h, w)
        m = (m != 0).to(torch.uint8).contiguous()
    img = torch.as_tensor(image)
    if img.dim() == 4 and img.shape[0] == 1:
        img = img[0]
    img = color.pack_image(img.to(dev), 1, h, w, dev)
    E_init = pose12(extrinsics)
    E_ref = E_init if reference_extrinsics is None else pose12(reference_extrinsics)
    if not (np.isfinite(E_init).all() and np.isfinite(E_ref).all()):
        raise ValueError('track_frame_rgbd: the initial and reference poses must be finite')
    K0 = np.ascontiguousarray(np.asarray(torch.as_tensor(intrinsics).detach().cpu().numpy(), dtype=np.float64).reshape(9))
    Kinv = np.empty((levels, 9), np.float32)
    model = []
    for l in range(levels):
        Kl = level_intrinsics(K0.reshape(3, 3), l)
        Kinv[l] = camera_arrays(Kl, E_ref.reshape(3, 4))[0]
        out = render_views(tsdf, weights, None, origin=origin, resolution=resolution, intrinsics=Kl,
                           extrinsics=E_ref.reshape(3, 4), shape=(h >> l, w >> l))
        mc = color.render_color(colors, origin=origin, resolution=resolution, intrinsics=Kl, extrinsics=E_ref.reshape(3, 4),
                                depth=out['depth'])
        model.append((out['depth'], out['normals'], mc))
    mdepth = np.array([_lib.ptr(x[0]) for x in model], dtype=np.uint64)
    mnorm = np.array([_lib.ptr(x[1]) for x in model], dtype=np.uint64)
    mcol = np.array([_lib.ptr(x[2]) for x in model], dtype=np.uint64)
    n_it = int(its.sum())
    ws = torch.empty(int(lib.ojf_track_rgbd_workspace_bytes(h, w, levels)), dtype=torch.uint8, device=dev)
    # pose f64[12] | stats f64[n_it, 4] | status int32[2]: one buffer, one copy back
    out = torch.empty(12 + 4 * n_it + 1, dtype=torch.float64, device=dev)
    status_ptr = out.data_ptr() + 8 * (12 + 4 * n_it)
    grad = float(dist_thresh if grad_depth_limit is None else grad_depth_limit)
    rc = lib.ojf_track_rgbd(_lib.ptr(d), _lib.ptr(m), _lib.ptr(img), h, w, levels, K0.ctypes.data, Kinv.ctypes.data,
                            mdepth.ctypes.data, mnorm.ctypes.data, mcol.ctypes.data, E_ref.ctypes.data, E_init.ctypes.data,
                            its.ctypes.data, float(dist_thresh), float(angle_thresh), float(pyramid_delta),
                            float(min_inlier_fraction), float(photo_weight), float(photo_thresh), grad, _lib.ptr(ws),
                            ws.numel(), out.data_ptr(), out.data_ptr() + 8 * 12, status_ptr, _lib.stream_ptr(dev))
    _lib.check(rc, 'ojf_track_rgbd')
    host = out.cpu().numpy()
    status = int(host[12 + 4 * n_it:].view(np.int32)[0])
    E = np.eye(4)
    E[:3] = host[:12].reshape(3, 4)
    return {'extrinsics': E, 'ok': status == 0, 'status': status, 'stats': host[12:12 + 4 * n_it].reshape(n_it, 4).copy()}
