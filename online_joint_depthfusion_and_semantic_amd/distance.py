"""Exact Euclidean distance transform of volumes (csrc/ojf_distance.hip, ``ojf_volume_edt`` / ``ojf_volume_surface_mask`` /
``ojf_volume_esdf``; the definition is in that file's header and restated in numpy by tests/distance_ref.py): for every voxel
the squared distance to the nearest seed voxel and which seed that is, and from the two - the ESDF of a fused TSDF (how much
room there is at a point of the map, beyond the truncation), dilation and erosion of masks by a metric radius, and the label
or colour of the nearest labelled voxel.

Volumes are [X,Y,Z] device tensors with z contiguous, 1 <= X, Y, Z <= 2048; the linear index of voxel (x, y, z) is
(x·Y + y)·Z + z.  Distances are between voxel centres."""
import math

import torch

from . import _lib, views

MAX_DIM = 2048  # csrc/ojf_distance.hip: kDMaxDim
NONE = _lib.EDT_NONE


def _radius2(who, name, radius, unit=1.0):
    """floor((radius / unit)²) as the library takes it (None: -1, unlimited); the arithmetic is f64."""
    if radius is None:
        return -1
    if isinstance(radius, bool) or not isinstance(radius, (int, float)) or not (radius >= 0) or math.isinf(radius):
        raise ValueError('{}: {} must be a finite number >= 0, got {!r}'.format(who, name, radius))
    r = float(radius) / unit
    return int(min(math.floor(r * r), 2 ** 24))  # (d² < 2^24 in every volume: 2^24 is as good as unlimited)


def _edt(who, seeds, max_dist2):
    seeds = views.mask_volume(who, seeds, 'seeds', torch.uint8)
    lib = views.on_device(who, seeds, MAX_DIM)
    dev, (X, Y, Z) = seeds.device, seeds.shape
    ws_bytes = lib.ojf_volume_edt_workspace_bytes(X, Y, Z)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    dist2 = torch.empty((X, Y, Z), dtype=torch.int32, device=dev)
    nearest = torch.empty((X, Y, Z), dtype=torch.int32, device=dev)
    rc = lib.ojf_volume_edt(_lib.ptr(seeds), X, Y, Z, max_dist2, _lib.EDT_ALL, _lib.ptr(ws), ws_bytes, _lib.ptr(dist2), _lib.ptr(nearest),
                            _lib.stream_ptr(dev))
    _lib.check(rc, 'ojf_volume_edt')
    return dist2, nearest


def edt(seeds, max_distance=None, *, max_dist2=None):
    """The distance transform of a seed volume, on the current stream of its device.

    seeds: u8 (or bool) [X,Y,Z], a seed where non-zero.  Returns (dist2, nearest), i32 [X,Y,Z] on the device: the squared
    distance in voxels to the nearest seed and that seed's linear index - of equally near seeds the one with the smallest
    index; ``NONE`` (2^31 - 1) and -1 with no seed in reach.  ``max_distance`` (voxels; None: unlimited) - or ``max_dist2``,
    the integer floor(max_distance²) itself - limits the reach: voxels further than that get NONE / -1, the others are what
    they are without a limit, and the passes look no further.  The same bits on every run.  Does not wait."""
    who = 'edt'
    if max_dist2 is not None:
        if max_distance is not None:
            raise ValueError('{}: at most one of max_distance and max_dist2 expected'.format(who))
        if isinstance(max_dist2, bool) or not isinstance(max_dist2, int) or max_dist2 < 0:
            raise ValueError('{}: max_dist2 must be an integer >= 0, got {!r}'.format(who, max_dist2))
        limit = min(max_dist2, 2 ** 24)
    else:
        limit = _radius2(who, 'max_distance', max_distance)
    return _edt(who, seeds, limit)


def surface_mask(tsdf, weights):
    """u8 [X,Y,Z] on the device: 1 where a voxel is observed (``components.observed_mask`` without a band) and has an observed
    face neighbour on the other side of the surface - inside is fp32(tsdf) < 0, so both zeros are outside.  The voxels on
    either side of every observed zero crossing: the seeds of the ESDF."""
    who = 'surface_mask'
    tsdf, weights = views.tsdf_pair(who, tsdf, weights)
    lib = views.on_device(who, tsdf, MAX_DIM)
    X, Y, Z = tsdf.shape
    mask = torch.empty(tsdf.shape, dtype=torch.uint8, device=tsdf.device)
    rc = lib.ojf_volume_surface_mask(_lib.ptr(tsdf.view(torch.int16)), _lib.ptr(weights.view(torch.int16)), X, Y, Z, _lib.ptr(mask),
                                     _lib.stream_ptr(tsdf.device))
    _lib.check(rc, 'ojf_volume_surface_mask')
    return mask


def esdf(tsdf, weights, resolution, max_distance=None):
    """The Euclidean signed distance field of a fused TSDF, f32 [X,Y,Z] on the device, in metres: resolution · sqrt(dist2) to
    the nearest surface voxel (``surface_mask``), negative where the voxel is observed and inside; an unobserved voxel gets the
    unsigned distance (``components.observed_mask`` tells which those are).  ``max_distance`` (metres; None: unlimited):
    voxels further than floor((max_distance / resolution)²) squared voxels from the surface get ±max_distance (±inf when
    unlimited and there is no surface at all).  The accuracy is that of voxel centres: within [-1, sqrt 3] voxels of the
    distance to the surface itself."""
    who = 'esdf'
    if isinstance(resolution, bool) or not isinstance(resolution, (int, float)) or not (resolution > 0) or math.isinf(resolution):
        raise ValueError('{}: resolution must be a finite number > 0, got {!r}'.format(who, resolution))
    limit = _radius2(who, 'max_distance', max_distance, float(resolution))
    tsdf, weights = views.tsdf_pair(who, tsdf, weights)
    lib = views.on_device(who, tsdf, MAX_DIM)
    dist2, _ = _edt(who, surface_mask(tsdf, weights), limit)
    out = torch.empty(tsdf.shape, dtype=torch.float32, device=tsdf.device)
    rc = lib.ojf_volume_esdf(_lib.ptr(dist2), _lib.ptr(tsdf.view(torch.int16)), _lib.ptr(weights.view(torch.int16)), tsdf.numel(),
                             float(resolution), float('inf') if max_distance is None else float(max_distance), _lib.ptr(out),
                             _lib.stream_ptr(tsdf.device))
    _lib.check(rc, 'ojf_volume_esdf')
    return out


def dilate(mask, radius):
    """u8 [X,Y,Z] on the device: 1 where a voxel is within ``radius`` voxels (d² <= floor(radius²)) of a non-zero voxel of
    ``mask`` - dilation by the Euclidean ball."""
    who = 'dilate'
    if radius is None:
        raise ValueError('{}: a radius is needed'.format(who))
    limit = _radius2(who, 'radius', radius)
    dist2, _ = _edt(who, mask, limit)
    return (dist2 != NONE).to(torch.uint8)


def erode(mask, radius):
    """u8 [X,Y,Z] on the device: 1 where every voxel of the box within ``radius`` voxels is non-zero in ``mask`` - erosion by
    the Euclidean ball, ``~dilate(~mask)``; what lies outside the box counts as foreground."""
    who = 'erode'
    if radius is None:
        raise ValueError('{}: a radius is needed'.format(who))
    limit = _radius2(who, 'radius', radius)
    mask = views.mask_volume(who, mask, 'mask', torch.uint8)
    views.on_device(who, mask, MAX_DIM)
    dist2, _ = _edt(who, (mask == 0).view(torch.uint8), limit)
    return (dist2 == NONE).to(torch.uint8)


def nearest_values(values, nearest, fill=0):
    """``values`` [X,Y,Z] or [X,Y,Z,C] at the nearest seed of every voxel (``nearest`` of ``edt``): the label, colour or TSDF
    value of the nearest labelled voxel; ``fill`` where there is none (-1)."""
    who = 'nearest_values'
    if not (torch.is_tensor(nearest) and nearest.dtype == torch.int32 and nearest.dim() == 3):
        raise ValueError('{}: nearest must be an i32 [X,Y,Z] tensor'.format(who))
    if not (torch.is_tensor(values) and values.dim() in (3, 4) and values.shape[:3] == nearest.shape and values.device == nearest.device):
        raise ValueError('{}: values must be an [X,Y,Z] or [X,Y,Z,C] tensor of the shape and device of nearest'.format(who))
    flat = values.reshape((nearest.numel(),) + tuple(values.shape[3:]))
    out = flat[nearest.reshape(-1).clamp(min=0).long()]
    out[nearest.reshape(-1) < 0] = fill
    return out.reshape(values.shape)
