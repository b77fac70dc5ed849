"""A per-voxel class distribution beside the fused geometry (SemanticFusion, Kimera-Semantics): the label observations of
the frames go into an fp16 [X,Y,Z,S] volume (per voxel the running mean of the class probabilities and a weight) by the
voxel-projective sweep of projective.py, and ``decide_labels`` writes the arg max of every observed voxel into the id / score
volumes everything downstream reads - in place of the reference's one-slot rule, under which a voxel keeps the single most
confident observation it ever saw.  The kernels are csrc/ojf_labels.hip (``ojf_fuse_label_probs``, ``ojf_label_decide``);
their fp32 definition is written in that file's header and restated in numpy by tests/label_ref.py.  The reference has no
counterpart.

The volume frame is the one extract, integrate, render, projective and color use.  A record is S = 8·ceil((C+1)/8) halves:
the C class means, the weight W (channel C; 0: nothing fused), and padding that no kernel touches.
"""
import torch

from . import _lib, views
from .ops import _origin_array


def record_size(n_classes):
    """S: the fp16 elements of a voxel's record for ``n_classes`` classes (2..256)."""
    n_classes = int(n_classes)
    if not 2 <= n_classes <= 256:
        raise ValueError('label_probs: n_classes must be in 2..256, got {}'.format(n_classes))
    return 8 * ((n_classes + 8) // 8)


def new_volume(shape, n_classes, device):
    """The zeroed label volume of a [X,Y,Z] grid: fp16 [X,Y,Z,S]."""
    return torch.zeros(tuple(shape) + (record_size(n_classes),), dtype=torch.float16, device=device)


def _volume(volume, n_classes, who):
    S = record_size(n_classes)
    if not (torch.is_tensor(volume) and volume.is_cuda and volume.dtype == torch.float16 and volume.dim() == 4
            and volume.shape[3] == S and volume.is_contiguous() and volume.data_ptr() % 16 == 0):
        raise ValueError('{}: volume must be a contiguous, 16-byte aligned cuda fp16 [X,Y,Z,{}] tensor for {} classes'.format(
            who, S, n_classes))
    return volume.shape[:3]


def integrate_label_probs(volume, n_classes, *, origin, resolution, depth, intrinsics, extrinsics, mask=None, probs=None,
                          labels=None, band, max_weight=64.0, near=0.0):
    """Fuse the label observations of ``n`` views into a device label volume in place, on the current stream of the volume's
    device.

    volume: cuda fp16 [X,Y,Z,S] (``new_volume``).  Exactly one of ``probs`` - float [n,]h,w,stride with stride >= n_classes,
    a distribution per pixel (values outside [0, 1] and NaN count as 0; the floats behind the classes are ignored) - and
    ``labels`` - u8 [n,]h,w, a one-hot vote per pixel (a label >= n_classes votes for nothing).  depth: cuda f32 [h,w] or
    [n,h,w] of the same frames (it decides which voxels a pixel votes in: those within ``band`` metres of the observed
    surface along the optical axis); mask, intrinsics, extrinsics as for ``projective.integrate_depth``.  max_weight: where
    the running mean's weight saturates (1..2048); near: smallest camera depth of a voxel that is updated.  The views are
    fused in order; more than ``_lib.LABEL_MAX_VIEWS`` go in several kernel calls, with the same bits as one view per call."""
    who = 'integrate_label_probs'
    X, Y, Z = _volume(volume, n_classes, who)  # (first: a host tensor or a bad class count is a ValueError on any machine)
    _lib.require_gpu()
    lib = _lib.load()
    C = int(n_classes)
    dev = volume.device
    if (probs is None) == (labels is None):
        raise ValueError('{}: exactly one of probs and labels must be given'.format(who))
    depth = views.depth_frames(who, depth, dev)
    n, h, w = depth.shape
    band, max_weight, near = views.running_mean_options(who, 'band', band, max_weight, near)
    n, K, E = views.cameras(who, intrinsics, extrinsics, n)
    mask = views.images(who, mask, 'mask', torch.uint8, n, h, w, dev)
    if labels is not None and torch.is_tensor(labels) and labels.dtype != torch.uint8:
        raise ValueError('{}: labels must be u8, got {}'.format(who, labels.dtype))
    labels = views.images(who, labels, 'labels', torch.uint8, n, h, w, dev)
    stride = 0
    if probs is not None:
        if not (torch.is_tensor(probs) and probs.device == dev and probs.is_floating_point() and probs.dim() in (3, 4)):
            raise ValueError('{}: probs must be a float [n,]h,w,stride tensor on the volume\'s device'.format(who))
        if probs.dim() == 3:
            probs = probs.unsqueeze(0)
        if tuple(probs.shape[:3]) != (n, h, w) or probs.shape[3] < C:
            raise ValueError('{}: probs [n,]h,w,>={} expected for {} depth maps of {}x{}, got {}'.format(
                who, C, n, h, w, tuple(probs.shape)))
        probs = probs.to(torch.float32).contiguous()
        stride = probs.shape[3]
    org = _origin_array(origin)
    stream = _lib.stream_ptr(dev)
    for v0, v1, Kc, Ec in views.chunks(n, _lib.LABEL_MAX_VIEWS, K, E):
        rc = lib.ojf_fuse_label_probs(_lib.ptr(volume), C, X, Y, Z, org.ctypes.data, float(resolution), v1 - v0, Kc.ctypes.data,
                                      Ec.ctypes.data, _lib.ptr(depth[v0:v1]), _lib.ptr(views.part(mask, v0, v1)),
                                      _lib.ptr(views.part(probs, v0, v1)), stride, _lib.ptr(views.part(labels, v0, v1)), h, w,
                                      band, max_weight, near, stream)
        _lib.check(rc, 'ojf_fuse_label_probs')


def decide_labels(volume, n_classes, ids, scores):
    """Write the decision of a label volume into ``ids`` (cuda u8 [X,Y,Z]) and ``scores`` (cuda fp16 [X,Y,Z]) in place: every
    voxel with a weight > 0 takes the first class of the largest mean and that mean; the other voxels keep what they hold."""
    who = 'decide_labels'
    X, Y, Z = _volume(volume, n_classes, who)
    _lib.require_gpu()
    lib = _lib.load()
    views.volume3(who, ids, 'ids', torch.uint8, (X, Y, Z), volume.device)
    views.volume3(who, scores, 'scores', torch.float16, (X, Y, Z), volume.device)
    rc = lib.ojf_label_decide(_lib.ptr(volume), int(n_classes), X, Y, Z, _lib.ptr(ids), _lib.ptr(scores),
                              _lib.stream_ptr(volume.device))
    _lib.check(rc, 'ojf_label_decide')
