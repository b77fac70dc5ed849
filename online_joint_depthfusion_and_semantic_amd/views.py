"""The host front end the view operators share (render, projective, color, label_probs, rasterize): ``n`` pinhole cameras,
their [n,h,w] frames, the running-mean options and the [X,Y,Z] volumes, checked and brought into the form the kernels take,
and the one loop that cuts ``n`` views into kernel calls - and the volume half, which the volume operators share (components,
distance): ``mask_volume``, ``tsdf_pair``, ``on_device``.  Nothing here loads the library or needs a device before a device
check is due: every helper but the last, ``on_device``, works on CPU tensors (tests/test_views_host.py).  ``who`` is the
public function's name; every refusal is a ValueError that starts with it.  ``dev`` is the torch.device the tensors of a call
must live on.
"""
import numpy as np
import torch

from .ops import camera_arrays


def _matrices(who, intrinsics, extrinsics):
    """The [k,3,3] / [m,3|4,4] host tensors of [3,3] / [n,3,3] intrinsics and [3,4] / [4,4] / [n,3,4] / [n,4,4] extrinsics
    (numpy or torch, any float type)."""
    K = torch.as_tensor(intrinsics).detach().cpu()
    E = torch.as_tensor(extrinsics).detach().cpu()
    if K.dim() == 2:
        K = K.unsqueeze(0)
    if E.dim() == 2:
        E = E.unsqueeze(0)
    if K.dim() != 3 or E.dim() != 3 or K.shape[-2:] != (3, 3) or E.shape[-1] != 4 or E.shape[-2] not in (3, 4):
        raise ValueError('{}: intrinsics [n,]3x3 and extrinsics [n,]3x4 or 4x4 expected, got {} and {}'.format(
            who, tuple(K.shape), tuple(E.shape)))
    return K, E


def cameras(who, intrinsics, extrinsics, n=None, nonzero_focal=False):
    """(n, K f64[n,9], E f64[n,12]) of ``n`` camera-to-world views (default: as many as there are extrinsics); a single
    matrix serves every view and a 4x4 pose gives its first three rows.  Finite entries and pinhole intrinsics
    [fx 0 cx; 0 fy cy; 0 0 1] only; ``nonzero_focal``: fx, fy != 0 as well."""
    K, E = _matrices(who, intrinsics, extrinsics)
    if n is None:
        n = E.shape[0]
        if n < 1:
            raise ValueError('{}: no view'.format(who))
    if K.shape[0] not in (1, n) or E.shape[0] not in (1, n):
        raise ValueError('{}: {} intrinsics and {} extrinsics for {} views'.format(who, K.shape[0], E.shape[0], n))
    K = np.ascontiguousarray(K.to(torch.float64).expand(n, 3, 3).reshape(n, 9).numpy())
    E = np.ascontiguousarray(E.to(torch.float64)[:, :3, :].expand(n, 3, 4).reshape(n, 12).numpy())
    if not (np.isfinite(K).all() and np.isfinite(E).all()):
        raise ValueError('{}: non-finite intrinsics or extrinsics'.format(who))
    if (K[:, [1, 3, 6, 7]] != 0.0).any() or (K[:, 8] != 1.0).any() or (nonzero_focal and (K[:, [0, 4]] == 0.0).any()):
        raise ValueError('{}: pinhole intrinsics [fx 0 cx; 0 fy cy; 0 0 1] expected'.format(who))
    return n, K, E


def inverse_cameras(who, intrinsics, extrinsics):
    """(n, Kinv f32[n,9], E f32[n,12]) for the ray casts, view by view through ``ops.camera_arrays`` (the reference's
    ``K.float().inverse()``); n is the larger of the two counts and a single matrix serves every view."""
    K, E = _matrices(who, intrinsics, extrinsics)
    n = max(K.shape[0], E.shape[0])
    if K.shape[0] not in (1, n) or E.shape[0] not in (1, n):
        raise ValueError('{}: {} intrinsics for {} poses'.format(who, K.shape[0], E.shape[0]))
    Ki, Ew = np.empty((n, 9), np.float32), np.empty((n, 12), np.float32)
    for i in range(n):
        Ki[i], Ew[i] = camera_arrays(K[i if K.shape[0] > 1 else 0], E[i if E.shape[0] > 1 else 0])
    return n, Ki, Ew


def depth_frames(who, depth, dev):
    """Contiguous f32 [n,h,w] of a [h,w] or [n,h,w] tensor on ``dev``, n >= 1."""
    if not (torch.is_tensor(depth) and depth.device == dev and depth.dim() in (2, 3)):
        raise ValueError('{}: depth must be a [h,w] or [n,h,w] tensor on the volume\'s device'.format(who))
    depth = depth.to(torch.float32)
    if depth.dim() == 2:
        depth = depth.unsqueeze(0)
    if depth.shape[0] < 1:
        raise ValueError('{}: no depth map'.format(who))
    return depth.contiguous()


def images(who, x, name, dtype, n, h, w, dev):
    """None, or the contiguous ``dtype`` [n,h,w] of a tensor of n·h·w elements on ``dev``; a bool image asked for as u8 is
    reinterpreted, not converted."""
    if x is None:
        return None
    if not (torch.is_tensor(x) and x.device == dev):
        raise ValueError('{}: {} must be a tensor on the volume\'s device'.format(who, name))
    if x.numel() != n * h * w:
        raise ValueError('{}: {} has {} elements for {} depth maps of {}x{}'.format(who, name, x.numel(), n, h, w))
    if dtype == torch.uint8 and x.dtype == torch.bool:
        x = x.contiguous().view(torch.uint8)
    return x.to(dtype).reshape(n, h, w).contiguous()


def running_mean_options(who, width_name, width, max_weight, near):
    """(width, max_weight, near) as floats: 0 < width < inf (the truncation or band, named ``width_name``),
    1 <= max_weight <= 2048, 0 <= near < inf."""
    width, max_weight, near = float(width), float(max_weight), float(near)
    if not (0.0 < width < float('inf')) or not (1.0 <= max_weight <= 2048.0) or not (0.0 <= near < float('inf')):
        raise ValueError('{}: {} > 0, 1 <= max_weight <= 2048 and near >= 0 expected, got {}, {}, {}'.format(
            who, width_name, width, max_weight, near))
    return width, max_weight, near


def volume3(who, vol, name, dtype, shape=None, dev=None, copy=False):
    """``vol`` if it is a contiguous ``dtype`` [X,Y,Z] tensor - on a cuda device, or on ``dev`` and of ``shape`` where those
    are given (a volume beside another).  ``copy``: a strided tensor is made contiguous instead of refused."""
    if not (torch.is_tensor(vol) and vol.dtype == dtype and vol.dim() == 3 and (copy or vol.is_contiguous())
            and (vol.is_cuda if dev is None else vol.device == dev) and (shape is None or vol.shape == tuple(shape))):
        raise ValueError('{}: {} must be a {}cuda {} [X,Y,Z] tensor{}'.format(
            who, name, '' if copy else 'contiguous ', dtype, '' if shape is None and dev is None else ' of the volume\'s shape and device'))
    return vol.contiguous() if copy else vol


def chunks(n, step, K, E):
    """(v0, v1, K[v0:v1], E[v0:v1]) for the kernel calls of at most ``step`` views that ``n`` views go in, in order; the
    slices are C-contiguous."""
    for v0 in range(0, n, step):
        v1 = min(n, v0 + step)
        yield v0, v1, np.ascontiguousarray(K[v0:v1]), np.ascontiguousarray(E[v0:v1])


def part(x, v0, v1):
    """The views v0..v1 of an [n,...] image stack or None (leading-axis slices of contiguous images are contiguous)."""
    return None if x is None else x[v0:v1]


def mask_volume(who, vol, name, dtype, like=None):
    """``vol`` as ``volume3`` takes it, on whatever device it lives: beside ``like`` (its shape and device) when that is given.
    A contiguous bool volume asked for as u8 is reinterpreted, not converted."""
    if not torch.is_tensor(vol):
        raise ValueError('{}: {} must be a {} [X,Y,Z] tensor'.format(who, name, dtype))
    if dtype == torch.uint8 and vol.dtype == torch.bool and vol.is_contiguous():
        vol = vol.view(torch.uint8)
    return volume3(who, vol, name, dtype, shape=None if like is None else like.shape, dev=vol.device if like is None else like.device)


def tsdf_pair(who, tsdf, weights):
    """The f16 [X,Y,Z] TSDF and, beside it, its weights."""
    tsdf = mask_volume(who, tsdf, 'tsdf', torch.float16)
    return tsdf, mask_volume(who, weights, 'weights', torch.float16, like=tsdf)


def on_device(who, vol, max_dim=None):
    """The loaded library, for a checked volume that is on a cuda device and of a size the kernels index: 1 <= X·Y·Z < 2^31,
    and with ``max_dim`` no side above it.  The one helper here that needs a GPU and loads the library - the device check is
    due where an operator calls it - hence last, with its import inside."""
    from . import _lib
    if not vol.is_cuda:
        raise ValueError('{}: the volumes must be cuda tensors'.format(who))
    if max_dim is None:
        if vol.numel() < 1 or vol.numel() >= 2 ** 31:
            raise ValueError('{}: 1 <= X·Y·Z < 2^31 expected, got shape {}'.format(who, tuple(vol.shape)))
    elif min(vol.shape) < 1 or max(vol.shape) > max_dim or vol.numel() >= 2 ** 31:
        raise ValueError('{}: 1 <= X, Y, Z <= {} and X·Y·Z < 2^31 expected, got shape {}'.format(who, max_dim, tuple(vol.shape)))
    _lib.require_gpu()
    return _lib.load()
