"""A colour volume beside the fused geometry (KinectFusion's colour volume, InfiniTAM, Open3D): colour images go into an
fp16 [X,Y,Z,4] volume (c0, c1, c2, W per voxel: the running mean of the image's three channels on its 0..255 scale, in the
image's channel order, and the colour weight) by the voxel-projective sweep of projective.py, and come out at points and at
the hit points of a rendered depth image.  The kernels are csrc/ojf_color.hip (``ojf_fuse_color``, ``ojf_color_sample``,
``ojf_color_render``); their fp32 definition is written in that file's header and restated in numpy by tests/color_ref.py.
The reference has no counterpart.

The volume frame is the one extract, integrate, render and projective use (voxel (i,j,k) centred at origin + (i+0.5, j+0.5,
k+0.5)·res).  Packing a float image into bytes is host-side plumbing and not part of the definition.
"""
import torch

from . import _lib, views
from .ops import _origin_array


def new_volume(shape, device):
    """The zeroed colour volume of a [X,Y,Z] grid: fp16 [X,Y,Z,4]."""
    return torch.zeros(tuple(shape) + (4,), dtype=torch.float16, device=device)


def _volume(colors, who):
    if not (torch.is_tensor(colors) and colors.is_cuda and colors.dtype == torch.float16 and colors.dim() == 4
            and colors.shape[3] == 4 and colors.is_contiguous()):
        raise ValueError('{}: colors must be a contiguous cuda fp16 [X,Y,Z,4] tensor'.format(who))
    return colors.shape[:3]


def pack_image(image, n, h, w, dev):
    """u8 [n,h,w,4] on ``dev`` from u8 [n,]h,w,3|4 or float [n,]3,h,w on the 0..255 scale (the batch dict's ``image``:
    clamp(0, 255), round, u8); the fourth byte is padding the kernel ignores."""
    if not (torch.is_tensor(image) and image.device == dev):
        raise ValueError('integrate_color: image must be a tensor on the volume\'s device')
    if image.dtype == torch.uint8:
        if image.dim() == 3:
            image = image.unsqueeze(0)
        if image.dim() != 4 or tuple(image.shape[:3]) != (n, h, w) or image.shape[3] not in (3, 4):
            raise ValueError('integrate_color: u8 image [n,]h,w,3|4 expected for {} depth maps of {}x{}, got {}'.format(
                n, h, w, tuple(image.shape)))
        if image.shape[3] == 4:
            return image.contiguous()
        px = image
    elif image.is_floating_point():
        if image.dim() == 3:
            image = image.unsqueeze(0)
        if image.dim() != 4 or tuple(image.shape) != (n, 3, h, w):
            raise ValueError('integrate_color: float image [n,]3,h,w expected for {} depth maps of {}x{}, got {}'.format(
                n, h, w, tuple(image.shape)))
        px = torch.round(image.float().clamp(0.0, 255.0)).to(torch.uint8).permute(0, 2, 3, 1)
    else:
        raise ValueError('integrate_color: image must be u8 [n,]h,w,3|4 or float [n,]3,h,w, got {}'.format(image.dtype))
    out = torch.zeros((n, h, w, 4), dtype=torch.uint8, device=dev)
    out[..., :3] = px
    return out


def integrate_color(colors, *, origin, resolution, image, depth, intrinsics, extrinsics, mask=None, band, max_weight=64.0,
                    near=0.0):
    """Fuse ``n`` colour views into a device colour volume in place, on the current stream of the volume's device.

    colors: cuda fp16 [X,Y,Z,4], contiguous.  image: u8 [n,]h,w,3|4 or float [n,]3,h,w on the 0..255 scale; depth: cuda f32
    [h,w] or [n,h,w] of the same frames (it decides which voxels a pixel colours: those within ``band`` metres of the
    observed surface along the optical axis); mask: bool / u8 of the depth's shape or None; intrinsics [3,3] or [n,3,3],
    extrinsics (camera-to-world) [3,4] / [4,4] or [n,...].  max_weight: where the running mean's weight saturates
    (1..2048); near: smallest camera depth of a voxel that is coloured.  The views are fused in order; more than
    ``_lib.COLOR_MAX_VIEWS`` go in several kernel calls, with the same bits as one view per call."""
    _lib.require_gpu()
    lib = _lib.load()
    who = 'integrate_color'
    X, Y, Z = _volume(colors, who)
    dev = colors.device
    depth = views.depth_frames(who, depth, dev)
    n, h, w = depth.shape
    band, max_weight, near = views.running_mean_options(who, 'band', band, max_weight, near)
    n, K, E = views.cameras(who, intrinsics, extrinsics, n)
    mask = views.images(who, mask, 'mask', torch.uint8, n, h, w, dev)
    image = pack_image(image, n, h, w, dev)
    org = _origin_array(origin)
    stream = _lib.stream_ptr(dev)
    for v0, v1, Kc, Ec in views.chunks(n, _lib.COLOR_MAX_VIEWS, K, E):
        rc = lib.ojf_fuse_color(_lib.ptr(colors), X, Y, Z, org.ctypes.data, float(resolution), v1 - v0, Kc.ctypes.data,
                                Ec.ctypes.data, _lib.ptr(depth[v0:v1]), _lib.ptr(views.part(mask, v0, v1)),
                                _lib.ptr(image[v0:v1]), h, w, band, max_weight, near, stream)
        _lib.check(rc, 'ojf_fuse_color')


def sample_color(colors, points_index):
    """u8 [N,4] colours (alpha 255, or all 0 where nothing coloured is near) of a colour volume at ``points_index``
    [N,3] in voxel index coordinates (voxel (i,j,k) sits at (i,j,k); a world point x is at (x - origin) / res - 0.5, a
    vertex v of ``Database.get_mesh`` at v / res): trilinear over the coloured corners only.  Points: numpy or a tensor,
    any float type; the result lives on the volume's device."""
    _lib.require_gpu()
    lib = _lib.load()
    X, Y, Z = _volume(colors, 'sample_color')
    pts = torch.as_tensor(points_index)
    if not (pts.dim() == 2 and pts.shape[1] == 3 and pts.is_floating_point()):
        raise ValueError('sample_color: points [N,3] of a float type expected, got {} {}'.format(tuple(pts.shape), pts.dtype))
    pts = pts.to(device=colors.device, dtype=torch.float32).contiguous()
    out = torch.empty((pts.shape[0], 4), dtype=torch.uint8, device=colors.device)
    if pts.shape[0]:
        rc = lib.ojf_color_sample(_lib.ptr(colors), X, Y, Z, _lib.ptr(pts), pts.shape[0], _lib.ptr(out),
                                  _lib.stream_ptr(colors.device))
        _lib.check(rc, 'ojf_color_sample')
    return out


def render_color(colors, *, origin, resolution, intrinsics, extrinsics, depth):
    """u8 [n,h,w,4] colour images of a colour volume at the points a depth image [n,h,w] (or [h,w]) marks on the rays of
    its pixels - ``render.render_views(...)['depth']`` of the same cameras gives what the camera sees of the model.  Pixels
    without depth (0, negative, non-finite) and points with nothing coloured near them are 0, alpha included."""
    _lib.require_gpu()
    lib = _lib.load()
    who = 'render_color'
    X, Y, Z = _volume(colors, who)
    dev = colors.device
    depth = views.depth_frames(who, depth, dev)
    n, Ki, E = views.inverse_cameras(who, intrinsics, extrinsics)
    if n != depth.shape[0]:
        raise ValueError('render_color: {} poses for {} depth images'.format(n, depth.shape[0]))
    h, w = depth.shape[1:]
    org = _origin_array(origin)
    out = torch.empty((n, h, w, 4), dtype=torch.uint8, device=dev)
    for v0, v1, Kc, Ec in views.chunks(n, _lib.RENDER_MAX_VIEWS, Ki, E):
        rc = lib.ojf_color_render(_lib.ptr(colors), X, Y, Z, org.ctypes.data, float(resolution), v1 - v0, Kc.ctypes.data,
                                  Ec.ctypes.data, _lib.ptr(depth[v0:v1]), h, w, _lib.ptr(out[v0:v1]), _lib.stream_ptr(dev))
        _lib.check(rc, 'ojf_color_render')
    return out
