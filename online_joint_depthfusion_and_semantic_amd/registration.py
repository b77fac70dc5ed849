"""Register two fused scenes of one room: the rigid transform that ``Database.merge`` and ``resample.compose`` take, by
Gauss-Newton on signed distance fields (csrc/ojf_register.hip, ``ojf_register_select`` / ``ojf_register``; the definition is in
that file's header and restated in numpy by tests/register_ref.py).  The voxels of the MOVING volume near its surface are
points that carry their own distance; the pose is sought under which the FIXED scene's field, read trilinearly at the mapped
points, shows the same distances.  A coarse stage reads a signed distance field of the fixed scene (``signed_distance_field``,
from the exact distance transform), whose basin is the whole box; a fine stage reads the fixed TSDF itself.  The reference
has no counterpart.

A scene is a dict {'tsdf': cuda fp16 [X,Y,Z] in metres, 'weights': cuda fp16 [X,Y,Z], 'origin': 3 numbers,
'resolution': metres per voxel} in the volume frame of resample.py.
"""
import math

import numpy as np
import torch

from . import _lib, distance, views

STATUS = ('ok', 'too few inliers', 'singular system', 'non-finite step')


def signed_distance_field(tsdf, weights, resolution, reach=None):
    """f32 [X,Y,Z] on the device, metres: fp32(resolution)·sqrt(dist2) to the nearest surface voxel (``distance.edt`` over
    ``distance.surface_mask``), and EVERY voxel, observed or not, takes the sign of that seed: negative iff fp32(T[nearest]) < 0.
    NaN where no seed is in reach (``reach`` metres; None: unlimited).  Unlike ``distance.esdf``, whose unobserved voxels are
    unsigned: behind a wall an unsigned distance grows where a signed one falls, and its gradient points the wrong way.
    Plain torch on the two outputs of ``edt``; does not wait."""
    who = 'signed_distance_field'
    if isinstance(resolution, bool) or not isinstance(resolution, (int, float)) or not (resolution > 0) or math.isinf(resolution):
        raise ValueError('{}: resolution must be a finite number > 0, got {!r}'.format(who, resolution))
    tsdf, weights = views.tsdf_pair(who, tsdf, weights)
    views.on_device(who, tsdf, distance.MAX_DIM)
    dist2, nearest = distance.edt(distance.surface_mask(tsdf, weights),
                                  None if reach is None else float(reach) / float(resolution))
    none = nearest < 0
    mag = torch.sqrt(dist2.to(torch.float32)) * torch.tensor(float(resolution), dtype=torch.float32, device=tsdf.device)
    inside = tsdf.reshape(-1)[nearest.reshape(-1).clamp(min=0).long()].to(torch.float32).reshape(tsdf.shape) < 0
    field = torch.where(inside, -mag, mag)
    return torch.where(none, torch.full_like(field, float('nan')), field)


def _band(who, name, x, inf_ok=False):
    x = float(x)
    if not (x > 0.0) or (math.isinf(x) and not inf_ok):
        raise ValueError('{}: {} must be > 0{}, got {}'.format(who, name, '' if inf_ok else ' and finite', x))
    return x


def _select(who, lib, tsdf, weights, band, stride, ws, list_=None):
    """One ojf_register_select call: the count tensor (u32 as i32 [1]) of a count-only or filling pass."""
    X, Y, Z = tsdf.shape
    count = torch.empty(1, dtype=torch.int32, device=tsdf.device)
    rc = lib.ojf_register_select(_lib.ptr(tsdf.view(torch.int16)), _lib.ptr(weights.view(torch.int16)), X, Y, Z, band, stride,
                                 _lib.ptr(ws), ws.numel(), _lib.ptr(list_), 0 if list_ is None else list_.numel(), _lib.ptr(count),
                                 _lib.stream_ptr(tsdf.device))
    _lib.check(rc, 'ojf_register_select')
    return count


def _select_workspace(lib, tsdf):
    return torch.empty(int(lib.ojf_register_workspace_bytes(tsdf.numel())), dtype=torch.uint8, device=tsdf.device)


def select_points(tsdf, weights, band, stride=1):
    """The points of a volume as the registration takes them: i32 [n] on the device (u32 linear indices (i·Y + j)·Z + k, increasing)
    of the voxels whose three indices are multiples of ``stride``, that are observed and have |tsdf| < ``band``.  Reads the
    count back once."""
    who = 'select_points'
    band = _band(who, 'band', band)
    if isinstance(stride, bool) or not isinstance(stride, int) or stride < 1:
        raise ValueError('{}: stride must be an integer >= 1, got {!r}'.format(who, stride))
    tsdf, weights = views.tsdf_pair(who, tsdf, weights)
    lib = views.on_device(who, tsdf)
    ws = _select_workspace(lib, tsdf)
    n = int(_select(who, lib, tsdf, weights, band, stride, ws).cpu()[0])
    out = torch.empty(n, dtype=torch.int32, device=tsdf.device)
    if n:
        _select(who, lib, tsdf, weights, band, stride, ws, out)
    return out


def _scene(who, d, name):
    if not isinstance(d, dict) or any(k not in d for k in ('tsdf', 'weights', 'origin', 'resolution')):
        raise ValueError('{}: {} must be a dict with tsdf, weights, origin and resolution'.format(who, name))
    for k in ('tsdf', 'weights'):
        v = d[k]
        if isinstance(v, np.ndarray) or (torch.is_tensor(v) and not v.is_cuda):
            raise ValueError('{}: {}[{!r}] is host-resident; the volumes must be on the device (to_torch()) - there is no CPU '
                             'path'.format(who, name, k))
    tsdf, weights = views.tsdf_pair('{}: {}'.format(who, name), d['tsdf'], d['weights'])
    o = d['origin']
    o = np.asarray(o.detach().cpu().numpy() if torch.is_tensor(o) else o, dtype=np.float64)
    res = float(d['resolution'])
    if o.size != 3 or not np.isfinite(o).all() or not (np.isfinite(res) and res > 0.0):
        raise ValueError('{}: {} needs a finite origin of 3 entries and a finite resolution > 0'.format(who, name))
    return tsdf, weights, o.reshape(3), res


def _transform(who, transform):
    if transform is None:
        return np.eye(3), np.zeros(3)
    if torch.is_tensor(transform):
        transform = transform.detach().cpu().numpy()
    T = np.asarray(transform, dtype=np.float64)
    if T.shape not in ((3, 4), (4, 4)) or not np.isfinite(T[:3]).all():
        raise ValueError('{}: transform must be a finite [3,4] or [4,4] matrix'.format(who))
    return T[:3, :3].copy(), T[:3, 3].copy()


def default_stages(band):
    """The two stages of the default: coarse on the signed distance field (the basin is the box), fine on the TSDF."""
    return [dict(field='sdf', stride=2, iterations=10, dist=0.5, field_band=float('inf')),
            dict(field='tsdf', stride=1, iterations=10, dist=band, field_band=None)]


def coarse_reach(stages, band, fixed_resolution):
    """How far from the surface (metres) the signed distance field of the 'sdf' stages is computed: the largest ``dist`` of those
    stages + band + 4 voxels; beyond it the field has no value.  Where the nearest surface is further than dist + band a point
    is no inlier (|F| > dist + band gives |r| > dist); distances are 1-Lipschitz and a cell's corners lie within sqrt(3) voxels of
    each other, so every cell that can hold such an inlier is complete - and the transform costs what the reach is, not what the
    box is.  What the limit does drop are cells far from every surface whose corners take opposite signs from
    seeds on two sides: their interpolated zero is no surface."""
    return max(s['dist'] for s in stages if s['field'] == 'sdf') + band + 4.0 * fixed_resolution


def condition(moving_shape, moving_origin, moving_resolution, R0, t0):
    """(c_m, c_f): the shift of both worlds that makes the centre of the moving box, and its image under the initial
    transform, the origins - x' = x - c_m, y' = y - c_f (f64); the conjugated initial pose is [R0 | 0], and a pose [R | t'] of
    the shifted worlds is [R | t' + c_f - R·c_m] of the callers'.  Without it q × grad grows with the distance of the scene
    from the world origin, and the solve's pivot rule would refuse a well-posed problem."""
    c_m = moving_origin + 0.5 * moving_resolution * np.asarray(moving_shape, dtype=np.float64)
    return c_m, R0 @ c_m + t0


def register_volumes(moving, fixed, *, transform=None, band=None, stages=None, min_inlier_fraction=0.05):
    """The rigid transform between two fused scenes, on the current stream of the volumes' device.

    moving / fixed: scene dicts (module docstring).  transform ([3,4] or [4,4], default identity): the initial guess; like the
    result it maps points of the moving scene's world to the fixed scene's - with moving = ``Database.merge``'s dst and fixed =
    its src it is what merge and ``resample.compose`` take.  band (metres, default 3 moving voxels): the moving voxels with
    |tsdf| < band are the points; it must lie below the truncation.  stages: a list of dicts {'field': 'sdf' | 'tsdf',
    'stride', 'iterations', 'dist', 'field_band'} (``default_stages(band)``: 'sdf', stride 2, 10 iterations, dist 0.5 m, then
    'tsdf', stride 1, 10 iterations, dist = band); the 'sdf' stages read ``signed_distance_field`` of fixed up to
    ``coarse_reach``; a 'tsdf' stage without a field_band takes the value just under the largest
    observed |tsdf| of the fixed volume.  min_inlier_fraction of a stage's points.
    Returns {'transform': f64 [3,4] numpy, 'ok', 'status' (0 ok, 1 too few inliers, 2 singular system, 3 non-finite step),
    'failed_iteration' (or -1), 'stats': f64 [sum(iterations), 4] (inlier count, mean squared residual, |omega|, |tau|),
    'n_points': per stage}.  After a failure the transform is the initial one.  The point counts (and the default
    field_band) are read back once, before the first stage; the stages then run back to back, and copying the result back is the
    call's only other synchronisation."""
    who = 'register_volumes'
    m_tsdf, m_w, m_o, m_res = _scene(who, moving, 'moving')
    f_tsdf, f_w, f_o, f_res = _scene(who, fixed, 'fixed')
    if f_tsdf.device != m_tsdf.device:
        raise ValueError('{}: moving and fixed must be on one device'.format(who))
    R0, t0 = _transform(who, transform)
    band = 3.0 * m_res if band is None else _band(who, 'band', band)
    stages = default_stages(band) if stages is None else [dict(s) for s in stages]
    if not stages:
        raise ValueError('{}: no stage'.format(who))
    for s in stages:
        if s.get('field') not in ('sdf', 'tsdf'):
            raise ValueError('{}: a stage\'s field must be \'sdf\' or \'tsdf\', got {!r}'.format(who, s.get('field')))
        s['stride'], s['iterations'] = int(s.get('stride', 1)), int(s.get('iterations', 10))
        if s['stride'] < 1 or s['iterations'] < 0:
            raise ValueError('{}: stride >= 1 and iterations >= 0 expected'.format(who))
        s['dist'] = _band(who, 'dist', s.get('dist', band))
        if s.get('field_band') is not None or s['field'] == 'sdf':
            s['field_band'] = _band(who, 'field_band', s.get('field_band') or float('inf'), inf_ok=True)
    n_it = sum(s['iterations'] for s in stages)
    if n_it > _lib.REGISTER_MAX_ITERATIONS:
        raise ValueError('{}: more than {} iterations'.format(who, _lib.REGISTER_MAX_ITERATIONS))
    frac = float(min_inlier_fraction)
    if not 0.0 <= frac <= 1.0:
        raise ValueError('{}: min_inlier_fraction must be in 0..1'.format(who))
    lib = views.on_device(who, m_tsdf)
    views.on_device(who, f_tsdf)
    dev = m_tsdf.device

    # the one read-back: the points of every stride, and the fixed volume's truncation where a stage asks for it
    ws_sel = _select_workspace(lib, m_tsdf)
    strides = sorted({s['stride'] for s in stages})
    heads = [_select(who, lib, m_tsdf, m_w, band, st, ws_sel).to(torch.float64) for st in strides]
    if any(s.get('field_band') is None for s in stages):
        ft = f_tsdf.to(torch.float32)
        seen = (f_w.to(torch.float32) > 0) & ~torch.isnan(ft)
        heads.append(torch.where(seen, ft.abs(), torch.zeros_like(ft)).max().to(torch.float64).reshape(1))
    host = torch.cat(heads).cpu().numpy()
    counts = {st: int(host[i]) for i, st in enumerate(strides)}
    for s in stages:
        if s.get('field_band') is None:
            s['field_band'] = _band(who, 'field_band (the largest observed |tsdf| of fixed)',
                                    np.nextafter(np.float32(host[-1]), np.float32(0)))
    for st in strides:
        if counts[st] == 0:
            raise ValueError('{}: the moving volume has no observed voxel with |tsdf| < {} at stride {}'.format(who, band, st))
    lists = {}
    for st in strides:
        lists[st] = torch.empty(counts[st], dtype=torch.int32, device=dev)
        _select(who, lib, m_tsdf, m_w, band, st, ws_sel, lists[st])
    field = None
    if any(s['field'] == 'sdf' for s in stages):
        field = signed_distance_field(f_tsdf, f_w, f_res, reach=coarse_reach(stages, band, f_res))

    c_m, c_f = condition(m_tsdf.shape, m_o, m_res, R0, t0)
    o_m, o_f = np.ascontiguousarray(m_o - c_m), np.ascontiguousarray(f_o - c_f)
    E0 = np.ascontiguousarray(np.concatenate([R0, np.zeros((3, 1))], axis=1).reshape(12))
    ws = torch.empty(int(lib.ojf_register_workspace_bytes(max(counts.values()))), dtype=torch.uint8, device=dev)
    # pose f64[12] | stats f64[MAX, 4] | status int32[2]: one buffer, one copy back
    rows = _lib.REGISTER_MAX_ITERATIONS
    out = torch.zeros(12 + 4 * rows + 1, dtype=torch.float64, device=dev)
    pose_ptr, stats_ptr, status_ptr = out.data_ptr(), out.data_ptr() + 8 * 12, out.data_ptr() + 8 * (12 + 4 * rows)
    first = 0
    for k, s in enumerate(stages):
        lst = lists[s['stride']]
        sdf = s['field'] == 'sdf'
        rc = lib.ojf_register(_lib.ptr(m_tsdf.view(torch.int16)), *m_tsdf.shape, o_m.ctypes.data, m_res, _lib.ptr(lst), lst.numel(),
                              None if sdf else _lib.ptr(f_tsdf.view(torch.int16)), None if sdf else _lib.ptr(f_w.view(torch.int16)),
                              _lib.ptr(field) if sdf else None, *f_tsdf.shape, o_f.ctypes.data, f_res, s['field_band'], s['dist'],
                              s['iterations'], first, frac, E0.ctypes.data, int(k > 0), _lib.ptr(ws), ws.numel(), pose_ptr,
                              stats_ptr, status_ptr, _lib.stream_ptr(dev))
        _lib.check(rc, 'ojf_register')
        first += s['iterations']
    host = out.cpu().numpy()
    status = host[12 + 4 * rows:].view(np.int32)
    P = host[:12].reshape(3, 4).copy()
    P[:, 3] = P[:, 3] + c_f - P[:, :3] @ c_m  # undo the shift: y = R (x - c_m) + t' + c_f
    code = int(status[0])
    if code:
        P = np.concatenate([R0, t0.reshape(3, 1)], axis=1)
    return {'transform': P, 'ok': code == 0, 'status': code, 'failed_iteration': int(status[1]),
            'stats': host[12:12 + 4 * n_it].reshape(n_it, 4).copy(), 'n_points': [counts[s['stride']] for s in stages]}
