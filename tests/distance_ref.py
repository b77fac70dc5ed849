"""Normative restatement of csrc/ojf_distance.hip in numpy: the exact Euclidean distance transform with the nearest seed, in
its separable form - no chunks, no runs, no ballots, no walk.

Definition (the kernel file's header): the linear index of a voxel is v = (x·Y + y)·Z + z.  A voxel is a seed where its byte
is non-zero.  dist2: the minimum over the seeds q of |p - q|²; nearest: the smallest linear index among the seeds that attain
it - together the minimum of the 64-bit key (d² << 32) | index(q), which ``brute_force`` computes as it stands.  NONE
(2^31 - 1) and -1 with no seed in reach; with max_dist2 >= 0 also where d² > max_dist2.  ``edt`` is the separable form:
g'[c] = min over c' of g[c'] + (c - c')² along z, then y, then x, ties to the smaller c' (numpy's argmin takes the first).

Also here: the surface mask and the ESDF in fp32, and the shapes and volumes the host and GPU tests share."""
import numpy as np

NONE = 2 ** 31 - 1

# csrc/ojf_distance.hip: the z pass works in chunks of CHUNK voxels; the y and x passes own lines of L voxels for runs of
# line_run(L, Z) consecutive z
CHUNK, MAX_RUN, LDS_INTS, MAX_DIM = 64, 64, 20480, 2048


def line_run(L, Z):
    return min(MAX_RUN, LDS_INTS // L, Z)


FIXED_SHAPES = [(1, 1, 1), (1, 1, 130), (1, 130, 1), (130, 1, 1), (2, 3, 65), (5, 67, 9), (67, 5, 9), (17, 13, 130), (33, 65, 129)]
T = CHUNK  # the chunk of the z pass, and the run of the y and x passes for lines of up to 320 voxels
TILE_SHAPES = [tuple(n if a == axis else m for a, m in enumerate((3, 2, 5))) for axis in range(3) for n in (T - 1, T, T + 1, 2 * T + 1)]
# where the run is no longer 64: lines of 321 voxels (runs of 63: 63 + 2 of Z = 65), of 700 (29: 29 + 29 + 12) and of 2048
# (10: 10 + 10 + 1), along y and along x
RUN_SHAPES = [(2, 321, 65), (321, 2, 65), (1, 700, 70), (2048, 1, 21), (1, 2048, 11)]
SHAPES = FIXED_SHAPES + TILE_SHAPES + RUN_SHAPES
assert [line_run(L, Z) for L, Z in ((320, 65), (321, 65), (700, 70), (2048, 21), (130, 9))] == [64, 63, 29, 10, 9]


def random_seeds(shape, density, seed=0):
    """u8 seeds of any non-zero byte; at least one."""
    rng = np.random.default_rng([seed, int(1000 * density)] + list(shape))
    s = (rng.random(shape) < density).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)
    if not s.any():
        s.ravel()[rng.integers(0, s.size)] = 1
    return s


def _limit(dist2, nearest, max_dist2):
    gone = dist2 >= NONE if max_dist2 < 0 else dist2 > max_dist2
    return np.where(gone, NONE, dist2), np.where(gone, -1, nearest)


def brute_force(seeds, max_dist2=-1):
    """(dist2 i32, nearest i32) as the minimum of the 64-bit keys over all seeds; for small volumes."""
    shape = seeds.shape
    q = np.argwhere(np.asarray(seeds) != 0).astype(np.int64)
    if len(q) == 0:
        return np.full(shape, NONE, np.int32), np.full(shape, -1, np.int32)
    p = np.stack(np.indices(shape), axis=-1).reshape(-1, 1, 3).astype(np.int64)
    d2 = ((p - q[None]) ** 2).sum(axis=2)
    index = (q[:, 0] * shape[1] + q[:, 1]) * shape[2] + q[:, 2]
    key = ((d2 << 32) | index[None]).min(axis=1)
    dist2, nearest = _limit(key >> 32, key & 0xffffffff, max_dist2)
    return dist2.reshape(shape).astype(np.int32), nearest.reshape(shape).astype(np.int32)


def _pass(g, idx, axis, max_dist2):
    """One 1-D pass: (g', idx') with g'[c] = min over c' of g[c'] + (c - c')², the first c' of equals, idx' = idx at it."""
    g, idx = np.moveaxis(g, axis, 0), np.moveaxis(idx, axis, 0)
    L = g.shape[0]
    out_g, out_i = np.empty_like(g), np.empty_like(idx)
    at = np.arange(L, dtype=np.int64).reshape((L,) + (1,) * (g.ndim - 1))
    for c in range(L):
        cand = g + (at - c) ** 2
        win = cand.argmin(axis=0)[None]
        out_g[c] = np.take_along_axis(cand, win, axis=0)[0]
        out_i[c] = np.take_along_axis(idx, win, axis=0)[0]
    out_g, out_i = _limit(out_g, out_i, max_dist2)
    return np.moveaxis(out_g, 0, axis), np.moveaxis(out_i, 0, axis)


def edt(seeds, max_dist2=-1, phases=('z', 'y', 'x'), start=None):
    """(dist2 i32 [X,Y,Z], nearest i32 [X,Y,Z]): the separable form.  ``phases``/``start``: a subset of the passes, from the
    pair an earlier subset left."""
    seeds = np.asarray(seeds)
    assert seeds.ndim == 3 and seeds.size < 2 ** 31 and max(seeds.shape) <= MAX_DIM
    if start is None:  # a seed is at distance 0 from itself: the z pass is a pass like the others
        is_seed = seeds != 0
        g = np.where(is_seed, 0, NONE).astype(np.int64)
        idx = np.where(is_seed, np.arange(seeds.size, dtype=np.int64).reshape(seeds.shape), -1)
    else:
        g, idx = start[0].astype(np.int64), start[1].astype(np.int64)
    for name in phases:
        g, idx = _pass(g, idx, 'xyz'.index(name), max_dist2)
    return g.astype(np.int32), idx.astype(np.int32)


def dilate(mask, max_dist2):
    return (edt(mask, max_dist2)[0] != NONE).astype(np.uint8)


def _state(tsdf, weights):
    """0: unobserved, 1: observed and outside, 2: observed and inside (fp32(tsdf) < 0)."""
    t, w = np.asarray(tsdf, np.float16).astype(np.float32), np.asarray(weights, np.float16).astype(np.float32)
    with np.errstate(invalid='ignore'):
        observed = (w > 0) & ~np.isnan(t)
        return np.where(observed, np.where(t < 0, 2, 1), 0)


def surface_mask(tsdf, weights):
    """u8: observed, with an observed face neighbour on the other side of the surface."""
    s = _state(tsdf, weights)
    hit = np.zeros(s.shape, bool)
    for axis in range(3):
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[axis], b[axis] = slice(0, -1), slice(1, None)
        a, b = tuple(a), tuple(b)
        across = (s[a] ^ s[b]) == 3
        hit[a] |= across
        hit[b] |= across
    return hit.astype(np.uint8)


def esdf(dist2, tsdf, weights, resolution, far):
    """f32: s · (fp32(resolution) · sqrt(fp32(dist2))), s · far where dist2 is NONE; s = -1 where observed and inside."""
    with np.errstate(invalid='ignore'):
        mag = np.float32(resolution) * np.sqrt(np.where(dist2 == NONE, 0, dist2).astype(np.float32))
    mag = np.where(dist2 == NONE, np.float32(far), mag).astype(np.float32)
    return np.where(_state(tsdf, weights) == 2, -mag, mag).astype(np.float32)


def scene_esdf(tsdf, weights, resolution, max_distance=None):
    """What distance.esdf computes, from the restatements."""
    r = None if max_distance is None else float(max_distance) / float(resolution)
    limit = -1 if r is None else int(min(np.floor(r * r), 2 ** 24))
    dist2, _ = edt(surface_mask(tsdf, weights), limit)
    return esdf(dist2, tsdf, weights, resolution, np.inf if max_distance is None else max_distance)
