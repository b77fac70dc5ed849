"""Normative restatement of csrc/ojf_components.hip in numpy: connected components of an [X,Y,Z] volume by min-propagation
over the shifted neighbour arrays with pointer jumping, run to a fixed point - no bricks, no union-find, no atomics.

Definition (the kernel file's header): the linear index of a voxel is v = (x·Y + y)·Z + z.  A voxel is foreground when its
mask byte is non-zero (no mask: every voxel); two neighbouring foreground voxels - face neighbours for connectivity 6, the
3x3x3 neighbourhood for 26 - are joined when their key bytes are equal (no keys: always).  labels: -1 on the background,
else the smallest linear index of the voxel's component.  The list, in ascending order of root: roots, sizes, keys (the key
at the root, 0 without keys), boxes (x0, y0, z0, x1, y1, z1), inclusive.  ids: -1 on the background, else the component's rank.

Also here: the observed mask and the removal, and the hand-made volumes the host and GPU tests share."""
import itertools

import numpy as np


def neighbour_offsets(connectivity):
    assert connectivity in (6, 26)
    offs = [d for d in itertools.product((-1, 0, 1), repeat=3) if any(d)]
    return [d for d in offs if connectivity == 26 or sum(abs(c) for c in d) == 1]


def _shifted(shape, d):
    """(dst, src) slices with dst + d = src inside the volume."""
    dst, src = [], []
    for n, c in zip(shape, d):
        dst.append(slice(max(0, -c), n - max(0, c)))
        src.append(slice(max(0, c), n - max(0, -c)))
    return tuple(dst), tuple(src)


def label_components(mask=None, keys=None, connectivity=6):
    """dict(labels i32 [X,Y,Z], ids i32 [X,Y,Z], n, roots i32 [n], sizes i32 [n], keys u8 [n], boxes i32 [n,6])."""
    first = mask if mask is not None else keys
    shape = first.shape
    assert len(shape) == 3 and first.size < 2 ** 31
    fg = np.ones(shape, bool) if mask is None else np.asarray(mask) != 0
    key = np.zeros(shape, np.uint8) if keys is None else np.asarray(keys, np.uint8)
    index = np.arange(first.size, dtype=np.int64).reshape(shape)
    lab = np.where(fg, index, -1)
    pairs = []
    for d in neighbour_offsets(connectivity):
        dst, src = _shifted(shape, d)
        pairs.append((dst, src, fg[dst] & fg[src] & (key[dst] == key[src])))
    f = fg.ravel()
    while True:
        new = lab.copy()
        for dst, src, joined in pairs:
            new[dst] = np.where(joined, np.minimum(new[dst], lab[src]), new[dst])
        flat = new.ravel()
        while True:  # pointer jumping: a label is a voxel of the same component, whose label is no larger
            jump = flat[flat[f]]
            if (jump == flat[f]).all():
                break
            flat[f] = jump
        if (new == lab).all():
            break
        lab = new
    flat = lab.ravel()
    roots = np.unique(flat[f])
    n = len(roots)
    rank = np.searchsorted(roots, flat[f])
    ids = np.full(first.size, -1, np.int32)
    ids[f] = rank
    sizes = np.bincount(rank, minlength=n).astype(np.int32)
    boxes = np.zeros((n, 6), np.int32)
    coords = np.stack(np.unravel_index(np.flatnonzero(f), shape), axis=1)
    lo = np.full((n, 3), np.iinfo(np.int64).max)
    hi = np.full((n, 3), -1)
    np.minimum.at(lo, rank, coords)
    np.maximum.at(hi, rank, coords)
    boxes[:, :3], boxes[:, 3:] = lo, hi
    return {'labels': lab.astype(np.int32), 'ids': ids.reshape(shape), 'n': n, 'roots': roots.astype(np.int32), 'sizes': sizes,
            'keys': key.ravel()[roots].astype(np.uint8), 'boxes': boxes}


def observed_mask(tsdf, weights, band=None):
    """u8: fp32(weight) > 0 and a TSDF value that is no NaN and, with a band, |fp32(tsdf)| < fp32(band)."""
    t, w = np.asarray(tsdf, np.float16).astype(np.float32), np.asarray(weights, np.float16).astype(np.float32)
    with np.errstate(invalid='ignore'):
        m = (w > 0) & ~np.isnan(t)
        if band is not None:
            m &= np.abs(t) < np.float32(band)
    return m.astype(np.uint8)


def keep_flags(sizes, roots, min_voxels=None, keep_largest=None):
    assert (min_voxels is None) != (keep_largest is None)
    if min_voxels is not None:
        return (np.asarray(sizes) >= min_voxels).astype(np.uint8)
    order = sorted(range(len(sizes)), key=lambda i: (-int(sizes[i]), int(roots[i])))
    keep = np.zeros(len(sizes), np.uint8)
    keep[order[:keep_largest]] = 1
    return keep


def apply_removal(tsdf, weights, ids, keep, init_value):
    """In place: voxels of components that are not kept go to float16(init_value) and weight 0; nothing else is written."""
    gone = (ids >= 0) & (np.asarray(keep)[np.maximum(ids, 0)] == 0) if len(keep) else np.zeros(ids.shape, bool)
    tsdf[gone] = np.float16(np.float32(init_value))
    weights[gone] = 0


# ---- hand-made volumes ---------------------------------------------------------------------------------------------------
def serpentine(shape):
    """(mask, size): a path one voxel wide through every 2 x 2 x Z column of the volume - in every even x-layer the even
    y-rows run the whole z-axis and neighbouring rows are bridged at alternating ends, the layers are bridged at alternating
    ends of that layer path.  One component at either connectivity; the box is (0, 0, 0, 2(nL-1), 2(nR-1), Z-1)."""
    X, Y, Z = shape
    m = np.zeros(shape, np.uint8)
    nL, nR = (X + 1) // 2, (Y + 1) // 2
    m[0::2, 0::2, :] = 1
    for r in range(nR - 1):
        m[0::2, 2 * r + 1, Z - 1 if r % 2 == 0 else 0] = 1
    end = (2 * (nR - 1), Z - 1 if nR % 2 == 1 else 0)  # where a layer's path ends; it starts at (0, 0)
    for k in range(nL - 1):
        y, z = end if k % 2 == 0 else (0, 0)
        m[2 * k + 1, y, z] = 1
    return m, nL * (nR * Z + nR - 1) + (nL - 1)


def checkerboard(shape):
    x, y, z = np.indices(shape)
    return ((x + y + z) % 2 == 0).astype(np.uint8)


def corner_cubes(shape, corner, side=2):
    """Two cubes of ``side`` voxels that touch only at the lattice corner ``corner`` (the first ends before it on every axis,
    the second starts at it): two components under 6, one under 26."""
    m = np.zeros(shape, np.uint8)
    cx, cy, cz = corner
    m[cx - side:cx, cy - side:cy, cz - side:cz] = 1
    m[cx:cx + side, cy:cy + side, cz:cz + side] = 1
    return m
