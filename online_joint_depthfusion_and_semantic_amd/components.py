"""Connected components of fused volumes (csrc/ojf_components.hip, ``ojf_volume_components`` / ``ojf_volume_observed_mask`` /
``ojf_volume_components_apply``; the definition is in that file's header and restated in numpy by tests/components_ref.py):
labels every foreground voxel with the smallest linear index of its component, lists the components with their sizes, keys and
boxes, and removes the small ones from a TSDF - the floaters an outlier depth streak leaves in mid-air, which the per-voxel
weight filter cannot see.  With the label volume as keys the components are 3-D instances.

Volumes are [X,Y,Z] device tensors with z contiguous; the linear index of voxel (x, y, z) is (x·Y + y)·Z + z."""
import numpy as np
import torch

from . import _lib, views


def _connectivity(who, connectivity):
    if connectivity not in (6, 26):
        raise ValueError('{}: connectivity must be 6 or 26, got {!r}'.format(who, connectivity))
    return int(connectivity)


def label_components(mask=None, keys=None, *, connectivity=6):
    """The connected components of the foreground of a volume, on the current stream of its device.

    mask: u8 (or bool) [X,Y,Z], foreground where non-zero (None: every voxel); keys: u8 [X,Y,Z], neighbouring foreground voxels
    are joined only where their keys are equal (None: always); at least one of the two; connectivity 6 (faces) or 26.
    Returns a dict: 'labels' i32 [X,Y,Z] on the device (-1 background, else the smallest linear index of the component),
    'ids' i32 [X,Y,Z] on the device (-1 background, else the rank of the component in the list), and the list in ascending
    order of root as numpy arrays - 'n', 'roots' i32 [n], 'sizes' i32 [n] (voxels), 'keys' u8 [n] (the key at the root, 0
    without keys), 'boxes' i32 [n,6] = (x0, y0, z0, x1, y1, z1), inclusive.  A function of the input alone: the same bits on
    every run.  Waits once, to read n, which sizes the list."""
    who = 'label_components'
    connectivity = _connectivity(who, connectivity)
    if mask is None and keys is None:
        raise ValueError('{}: a mask or a key volume is needed'.format(who))
    first = views.mask_volume(who, mask if mask is not None else keys, 'mask' if mask is not None else 'keys', torch.uint8)
    if mask is not None:
        mask, keys = first, (None if keys is None else views.mask_volume(who, keys, 'keys', torch.uint8, like=first))
    else:
        keys = first
    lib = views.on_device(who, first)
    dev, (X, Y, Z) = first.device, first.shape
    stream = _lib.stream_ptr(dev)
    ws_bytes = lib.ojf_volume_components_workspace_bytes(X, Y, Z)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    labels = torch.empty((X, Y, Z), dtype=torch.int32, device=dev)
    ids = torch.empty((X, Y, Z), dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    head = (_lib.ptr(mask), _lib.ptr(keys), X, Y, Z, connectivity)
    rc = lib.ojf_volume_components(*head, _lib.COMPONENTS_ALL, _lib.ptr(ws), ws_bytes, _lib.ptr(labels), _lib.ptr(ids), None, None, None,
                                   None, 0, _lib.ptr(count), stream)
    _lib.check(rc, 'ojf_volume_components')
    n = int(count.item())
    out = {'labels': labels, 'ids': ids, 'n': n}
    roots = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    sizes = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    list_keys = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    boxes = torch.empty((max(n, 1), 6), dtype=torch.int32, device=dev)
    if n:  # (the labels, the ranks and the brick-local figures of the first call are still where it left them)
        rc = lib.ojf_volume_components(*head, _lib.COMPONENTS_LIST, _lib.ptr(ws), ws_bytes, _lib.ptr(labels), _lib.ptr(ids), _lib.ptr(roots),
                                       _lib.ptr(sizes), _lib.ptr(list_keys), _lib.ptr(boxes), n, None, stream)
        _lib.check(rc, 'ojf_volume_components')
    out.update(roots=roots[:n].cpu().numpy(), sizes=sizes[:n].cpu().numpy(), keys=list_keys[:n].cpu().numpy(), boxes=boxes[:n].cpu().numpy())
    return out


def _band(who, band):
    if band is None:
        return 0, 0.0
    band = float(band)
    if not (band > 0.0) or not (np.float32(band) > 0):
        raise ValueError('{}: band > 0 expected, got {}'.format(who, band))
    return 1, band


def observed_mask(tsdf, weights, band=None):
    """u8 [X,Y,Z] on the device: 1 where a voxel is observed - fp32(weight) > 0 and a TSDF value that is no NaN, the mesh
    extractor's rule (a NaN, negative or -0 weight is unobserved, the smallest subnormal observed) - and, with ``band``,
    |tsdf| < band.  The learned fusion writes only the samples around the surface, so its observed set is a band already;
    carving projective fusion observes free space as well and needs one (its truncation)."""
    who = 'observed_mask'
    use_band, band = _band(who, band)
    tsdf, weights = views.tsdf_pair(who, tsdf, weights)
    lib = views.on_device(who, tsdf)
    mask = torch.empty(tsdf.shape, dtype=torch.uint8, device=tsdf.device)
    rc = lib.ojf_volume_observed_mask(_lib.ptr(tsdf.view(torch.int16)), _lib.ptr(weights.view(torch.int16)), tsdf.numel(), use_band, band,
                                      _lib.ptr(mask), _lib.stream_ptr(tsdf.device))
    _lib.check(rc, 'ojf_volume_observed_mask')
    return mask


def keep_flags(sizes, roots, min_voxels=None, keep_largest=None, who='remove_small_components'):
    """The u8 keep flag of every component of a list (numpy; no device): exactly one of ``min_voxels`` (keep the components
    of at least that many voxels) and ``keep_largest`` = k (keep the k largest; of equal sizes the smaller root first)."""
    if (min_voxels is None) == (keep_largest is None):
        raise ValueError('{}: exactly one of min_voxels and keep_largest expected'.format(who))
    value = min_voxels if keep_largest is None else keep_largest
    if isinstance(value, bool) or int(value) != value or value < 1:
        raise ValueError('{}: {} must be an integer >= 1, got {!r}'.format(who, 'min_voxels' if keep_largest is None else 'keep_largest', value))
    sizes, roots = np.asarray(sizes, dtype=np.int64), np.asarray(roots, dtype=np.int64)
    if min_voxels is not None:
        return (sizes >= int(min_voxels)).astype(np.uint8)
    keep = np.zeros(len(sizes), dtype=np.uint8)
    keep[np.lexsort((roots, -sizes))[:int(keep_largest)]] = 1
    return keep


def remove_small_components(tsdf, weights, *, init_value, min_voxels=None, keep_largest=None, connectivity=26, band=None):
    """Remove the small connected components of the observed voxels (``observed_mask(tsdf, weights, band)``) from fp16 volumes
    in place: their voxels go back to ``init_value`` and weight 0, as ``Database.filter`` leaves a voxel; kept components and
    unobserved voxels are not written.  Exactly one of ``min_voxels`` and ``keep_largest`` (see ``keep_flags``; decided on the
    host from the list).  Returns the list of ``label_components`` (with 'labels' and 'ids' on the device) plus 'keep', the
    u8 [n] flags."""
    who = 'remove_small_components'
    keep_flags([], [], min_voxels, keep_largest, who)  # (the criteria, before anything is computed)
    connectivity = _connectivity(who, connectivity)
    _band(who, band)
    tsdf, weights = views.tsdf_pair(who, tsdf, weights)
    lib = views.on_device(who, tsdf)
    out = label_components(observed_mask(tsdf, weights, band), connectivity=connectivity)
    keep = keep_flags(out['sizes'], out['roots'], min_voxels, keep_largest, who)
    out['keep'] = keep
    if out['n'] and not keep.all():
        flags = torch.from_numpy(keep).to(tsdf.device)
        rc = lib.ojf_volume_components_apply(_lib.ptr(out['ids']), _lib.ptr(flags), out['n'], _lib.ptr(tsdf.view(torch.int16)),
                                             _lib.ptr(weights.view(torch.int16)), tsdf.numel(), float(init_value), _lib.stream_ptr(tsdf.device))
        _lib.check(rc, 'ojf_volume_components_apply')
    return out


def instances(ids_volume, tsdf, weights, *, connectivity=6, min_voxels=1, band=None):
    """3-D instances: the connected components of equal labels of a u8 label volume among the observed voxels.  Returns a dict:
    'ids' i32 [X,Y,Z] on the device (-1: unobserved or dropped, else the instance's rank) and, in ascending order of root,
    'n', 'roots', 'sizes', 'classes' u8 [n] (the label of the instance) and 'boxes' i32 [n,6].  Components of fewer than
    ``min_voxels`` voxels are dropped from the list; the others are renumbered densely in root order."""
    who = 'instances'
    connectivity = _connectivity(who, connectivity)
    if isinstance(min_voxels, bool) or int(min_voxels) != min_voxels or min_voxels < 1:
        raise ValueError('{}: min_voxels must be an integer >= 1, got {!r}'.format(who, min_voxels))
    tsdf, weights = views.tsdf_pair(who, tsdf, weights)
    ids_volume = views.mask_volume(who, ids_volume, 'ids', torch.uint8, like=tsdf)
    c = label_components(observed_mask(tsdf, weights, band), ids_volume, connectivity=connectivity)
    keep = c['sizes'] >= int(min_voxels)
    ids = c['ids']
    if not keep.all():
        new_rank = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
        table = torch.from_numpy(new_rank).to(ids.device)
        ids = torch.where(ids >= 0, table[ids.clamp(min=0).long()], ids)
    return {'ids': ids, 'n': int(keep.sum()), 'roots': c['roots'][keep], 'sizes': c['sizes'][keep], 'classes': c['keys'][keep],
            'boxes': c['boxes'][keep]}
