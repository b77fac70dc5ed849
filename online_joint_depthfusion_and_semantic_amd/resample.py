"""Re-box, resample and merge fused scenes: every voxel of a destination box reads the volumes of a source box through a
rigid transform - the trilinear mean of the observed source voxels around the point its centre maps to, the label of the
nearest of them.  One operator with three uses: the box follows the camera (a whole-voxel shift is an exact copy of the
overlap), a scene is handed on at another resolution, and two fused sessions of one room, aligned by a tracked pose, are
combined by their weights.  The kernels are csrc/ojf_resample.hip (``ojf_resample_volumes``, ``ojf_resample_records``); their
fp32 definition is written in that file's header and restated in numpy by tests/resample_ref.py.  The reference has no
counterpart.

The volume frame is the one extract, integrate, render, projective, color and label_probs use: voxel (i,j,k) has its centre at
origin + (i+0.5, j+0.5, k+0.5)·resolution.
"""
import numpy as np
import torch

from . import _lib
from .label_probs import record_size

SCALAR_KEYS = ('tsdf', 'weights', 'ids', 'scores')
RECORD_KEYS = ('colors', 'label_probs')
GEOMETRY_MAX_WEIGHT = 65504.0  # the largest finite fp16: the fusion weights of the learned integrator are not capped
RECORD_MAX_WEIGHT = 64.0  # the default of integrate_color / integrate_label_probs


def _vec3(x, name):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    x = np.asarray(x, dtype=np.float64)
    if x.size != 3:
        raise ValueError('resample: {} must have 3 entries, got shape {}'.format(name, x.shape))
    return x.reshape(3)


def _res(x, name):
    x = float(x)
    if not (np.isfinite(x) and x > 0.0):
        raise ValueError('resample: {} must be finite and > 0, got {}'.format(name, x))
    return x


def compose(src_origin, src_resolution, dst_origin, dst_resolution, transform=None):
    """(M f64[9], c f64[3]) of the definition: destination voxel (i,j,k) reads the source at index coordinates M·(i,j,k) + c.
    ``transform`` ([3,4] or [4,4], default identity) maps destination-world points to source-world points, x_s = R·x_d + t;
    M = R·res_d/res_s, c = (R·(origin_d + 0.5·res_d·1) + t - origin_s)/res_s - 0.5.  ValueError: a resolution <= 0, an R with
    |RᵀR - I| > 1e-6, a non-finite M or c."""
    o_s, o_d = _vec3(src_origin, 'src_origin'), _vec3(dst_origin, 'dst_origin')
    r_s, r_d = _res(src_resolution, 'src_resolution'), _res(dst_resolution, 'dst_resolution')
    if transform is None:
        R, t = np.eye(3), np.zeros(3)
    else:
        if torch.is_tensor(transform):
            transform = transform.detach().cpu().numpy()
        T = np.asarray(transform, dtype=np.float64)
        if T.shape not in ((3, 4), (4, 4)):
            raise ValueError('resample: transform must be [3,4] or [4,4], got {}'.format(T.shape))
        R, t = T[:3, :3], T[:3, 3]
        if not np.isfinite(T[:3]).all():
            raise ValueError('resample: non-finite transform')
        if np.abs(R.T @ R - np.eye(3)).max() > 1e-6:
            raise ValueError('resample: the transform\'s rotation is not orthonormal (|RᵀR - I| > 1e-6)')
    with np.errstate(all='ignore'):
        M = R * r_d / r_s
        c = (R @ (o_d + 0.5 * r_d * np.ones(3)) + t - o_s) / r_s - 0.5
    if not (np.isfinite(M).all() and np.isfinite(c).all()):
        raise ValueError('resample: non-finite M or c (origins, resolutions, transform)')
    return np.ascontiguousarray(M.reshape(9)), np.ascontiguousarray(c)


def _shape3(shape, name):
    try:
        shape = tuple(int(n) for n in shape)
    except TypeError:
        raise ValueError('resample: {} must be three sizes'.format(name)) from None
    if len(shape) != 3 or min(shape) <= 0:
        raise ValueError('resample: {} must be three positive sizes, got {}'.format(name, shape))
    return shape


def _volumes(d, who, shape=None):
    """The volumes of a scene dict, checked: ({key: tensor}, [X,Y,Z], record channel counts {key: (S, Cw)}, device)."""
    if not isinstance(d, dict):
        raise ValueError('resample: {} must be a dict of volumes'.format(who))
    unknown = set(d) - set(SCALAR_KEYS) - set(RECORD_KEYS) - {'n_classes'}
    if unknown:
        raise ValueError('resample: {} has unknown keys {}'.format(who, sorted(unknown)))
    vols = {k: d[k] for k in SCALAR_KEYS + RECORD_KEYS if d.get(k) is not None}
    if not vols:
        raise ValueError('resample: {} holds no volume'.format(who))
    for k, v in vols.items():
        if isinstance(v, np.ndarray) or (torch.is_tensor(v) and not v.is_cuda):
            raise ValueError('resample: {}[{!r}] is host-resident; the volumes must be on the device (to_torch()) - there is no '
                             'CPU path'.format(who, k))
        if not torch.is_tensor(v):
            raise ValueError('resample: {}[{!r}] must be a device tensor'.format(who, k))
    if ('weights' in vols or 'ids' in vols or 'scores' in vols) and 'tsdf' not in vols:
        raise ValueError('resample: {} has weights / ids / scores without tsdf'.format(who))
    if ('ids' in vols) != ('scores' in vols):
        raise ValueError('resample: {} must hold ids and scores together'.format(who))
    chans = {}
    if 'colors' in vols:
        chans['colors'] = (4, 3)
    if 'label_probs' in vols:
        if d.get('n_classes') is None:
            raise ValueError('resample: {} has label_probs without n_classes'.format(who))
        chans['label_probs'] = (record_size(d['n_classes']), int(d['n_classes']))
    dev = next(iter(vols.values())).device
    for k, v in vols.items():
        want = torch.uint8 if k == 'ids' else torch.float16
        dims = 3 if k in SCALAR_KEYS else 4
        if v.device != dev or v.dtype != want or v.dim() != dims or not v.is_contiguous():
            raise ValueError('resample: {}[{!r}] must be a contiguous {} tensor of {} dimensions on one device'.format(who, k, want, dims))
        if shape is None:
            shape = tuple(v.shape[:3])
        if tuple(v.shape[:3]) != tuple(shape) or min(shape) <= 0:
            raise ValueError('resample: {}[{!r}] has the grid {}, expected {}'.format(who, k, tuple(v.shape[:3]), tuple(shape)))
        if k in chans and v.shape[3] != chans[k][0]:
            raise ValueError('resample: {}[{!r}] must have {} channels, got {}'.format(who, k, chans[k][0], v.shape[3]))
        if k == 'label_probs' and v.data_ptr() % 16:
            raise ValueError('resample: {}[\'label_probs\'] must be 16-byte aligned'.format(who))
    return vols, tuple(shape), chans, dev


def _max_weights(max_weight):
    if max_weight is None:
        return GEOMETRY_MAX_WEIGHT, RECORD_MAX_WEIGHT
    m = float(max_weight)
    if not (np.isfinite(m) and 1.0 <= m <= 65504.0):
        raise ValueError('resample: max_weight must be finite and in 1..65504, got {}'.format(m))
    return m, m


def resample_scene(src, *, src_origin, src_resolution, dst_shape, dst_origin, dst_resolution, transform=None, into=None,
                   init_value, max_weight=None):
    """Read the volumes of a source box into a destination box, on the current stream of the volumes' device, without ever
    synchronising.

    src: a dict of device tensors under the keys ``tsdf`` / ``weights`` (fp16 [X,Y,Z]; tsdf alone is the ground-truth form:
    every voxel observed), ``ids`` (u8) / ``scores`` (fp16) (both or neither, beside tsdf), ``colors`` (fp16 [X,Y,Z,4]) and
    ``label_probs`` (fp16 [X,Y,Z,S], with ``n_classes``); any consistent subset.  src_origin / src_resolution and dst_shape /
    dst_origin / dst_resolution describe the two boxes; ``transform`` ([3,4] or [4,4], default identity) maps
    destination-world points to source-world points.

    into=None: replace mode - fresh volumes of dst_shape are returned (a dict with the keys of ``src``); a voxel no observed
    source voxel covers holds init_value / weight 0 / id 0 / score 0 / a zero record.  into=dict: merge mode - the volumes of
    ``into`` (the keys of ``src``, grid dst_shape, with weights) are updated in place by their weights and returned; max_weight:
    where the merged weight saturates (default: 65504 for the geometry, 64 for colour and class distributions)."""
    vols, s_shape, chans, dev = _volumes(src, 'src')
    d_shape = _shape3(dst_shape, 'dst_shape')
    M, c = compose(src_origin, src_resolution, dst_origin, dst_resolution, transform)
    init_value = float(init_value)
    if not np.isfinite(init_value):
        raise ValueError('resample: init_value must be finite')
    geo_max, rec_max = _max_weights(max_weight)
    merge = into is not None
    if merge:
        dst, _, d_chans, d_dev = _volumes(into, 'into', d_shape)
        if set(dst) != set(vols) or d_chans != chans or d_dev != dev:
            raise ValueError('resample: into must hold the volumes of src ({}) on its device, got {}'.format(sorted(vols), sorted(dst)))
        if 'tsdf' in vols and 'weights' not in vols:
            raise ValueError('resample: a merge needs the weight volumes')
    _lib.require_gpu()
    lib = _lib.load()
    if not merge:
        dst = {}
        for k, v in vols.items():
            # (a record's padding is never written: zeros; every scalar voxel is written once)
            dst[k] = (torch.zeros if k in RECORD_KEYS else torch.empty)(d_shape + tuple(v.shape[3:]), dtype=v.dtype, device=dev)
    mode = _lib.RESAMPLE_MERGE if merge else _lib.RESAMPLE_REPLACE
    stream = _lib.stream_ptr(dev)
    if 'tsdf' in vols:
        p = lambda side, k: _lib.ptr(side.get(k))  # noqa: E731
        rc = lib.ojf_resample_volumes(p(vols, 'tsdf'), p(vols, 'weights'), p(vols, 'ids'), p(vols, 'scores'), *s_shape,
                                      p(dst, 'tsdf'), p(dst, 'weights'), p(dst, 'ids'), p(dst, 'scores'), *d_shape,
                                      M.ctypes.data, c.ctypes.data, init_value, mode, geo_max, stream)
        _lib.check(rc, 'ojf_resample_volumes')
    for k, (S, Cw) in chans.items():
        rc = lib.ojf_resample_records(_lib.ptr(vols[k]), *s_shape, _lib.ptr(dst[k]), *d_shape, S, Cw, M.ctypes.data, c.ctypes.data,
                                      mode, rec_max, stream)
        _lib.check(rc, 'ojf_resample_records')
    out = dict(dst)
    if 'label_probs' in chans:
        out['n_classes'] = chans['label_probs'][1]
    return out
