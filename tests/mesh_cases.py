"""Small volumes and point sets that reach each edge of csrc/ojf_mesh.hip, with the property that justifies every case next
to it.  test_mesh_edges_host.py asserts those properties from the reference (mesh_ref.py) alone; test_mesh_edges_gpu.py
holds the kernels to the reference on the same cases.  Everything is seeded; a case and its reference are built once per
process and handed out read-only."""
import collections
import functools

import numpy as np

import mesh_ref

Case = collections.namedtuple('Case', 'name vol weights ids iso origin res')

# name -> (shape, iso, origin, res).  iso, origin and res differ from case to case; 'tile_131' has the negative iso and
# 'scan_1025' the origin of magnitude 1e3 at res 0.0125, where fp32(origin + f64(p) * res) differs from an fp32 transform.
TILE = {
    'tile_65':    ((3, 5, 65),   0.03,  (-1.25, 0.5, 3.0),    0.0125),   # Z-1 = 64: one exactly full wave, one z tile
    'tile_66':    ((3, 6, 66),   0.05,  (0.75, -2.5, 1.0),    0.02),     # second z tile with one cell; y tile with one row
    'tile_66_row': ((2, 2, 66),  0.01,  (4.0, 4.5, -6.0),     0.5),      # one cell row: three idle waves per block
    'tile_131':   ((5, 7, 131),  -0.07, (-3.5, 2.25, 0.125),  0.04),     # third z tile with two cells; 3*2*4 = 24 blocks
    'tile_min':   ((2, 2, 2),    0.02,  (10.0, -20.0, 30.0),  0.1),      # the axis minimum: one cell
    'tile_y33':   ((9, 33, 5),   0.04,  (0.1, 0.2, 0.3),      0.025),    # Y-1 = 32: 8 y tiles, 1*8*8 = 64 blocks
}
# name -> (shape, n_blocks, iso, origin, res, share of blocks observed, first block observed, last block observed)
SCAN = {
    'scan_1':    ((2, 3, 3),      1,    0.06,  (1.0, 2.0, 3.0),           0.3,    1.0,  True,  True),
    'scan_1023': ((32, 44, 131),  1023, 0.08,  (-0.5, -0.25, -0.125),     0.01,   0.2,  False, True),   # first block empty
    'scan_1024': ((129, 33, 10),  1024, 0.09,  (2.0, 0.0, -1.0),          0.05,   0.5,  True,  False),  # last block empty
    'scan_1025': ((42, 98, 5),    1025, 0.11,  (1000.3, -999.7, 1001.1),  0.0125, 0.5,  True,  True),
    'scan_2049': ((684, 4, 131),  2049, 0.12,  (-7.0, 8.0, -9.0),         0.015,  0.15, True,  True),   # chunk = 3
}
VALUE_SHAPE = (17, 13, 19)
VALUE = {
    'ties':     (0.0,               (0.5, 0.25, -0.75),   1.0),
    'on_iso':   (0.0,               (-2.0, 3.0, 0.0),     0.0625),
    'extremes': (np.float32(1.7e-7), (0.0, -1.0, 5.5),    0.2),   # 1.7e-7 lies between the fp16 subnormals 2 and 3 * 2^-24
    'masked':   (0.025,             (6.0, 6.5, 7.25),     0.03),
}
TILE_NAMES, SCAN_NAMES, VALUE_NAMES = list(TILE), list(SCAN), list(VALUE)
ALL_NAMES = TILE_NAMES + SCAN_NAMES + VALUE_NAMES
SUBNORMAL = np.float16(2.0 ** -24)  # the smallest positive fp16: observed


def noise(shape, rng):
    """Normal noise, averaged once with the neighbour along each axis so that the surface is not pure salt, kept fp16.
    Drawn one voxel larger and cropped: the cyclic neighbour would make an axis of two voxels constant."""
    vol = rng.normal(size=tuple(s + 1 for s in shape)).astype(np.float16)
    for ax in range(3):
        vol = ((vol.astype(np.float32) + np.roll(vol, 1, axis=ax).astype(np.float32)) / 2).astype(np.float16)
    return np.ascontiguousarray(vol[1:, 1:, 1:])


def _seed(name):
    return 1000 + ALL_NAMES.index(name)


def _tile_case(name):
    shape, iso, origin, res = TILE[name]
    rng = np.random.default_rng(_seed(name))
    vol = noise(shape, rng)
    weights = np.full(shape, 3.0, dtype=np.float16)
    if min(shape) > 2:  # a few unobserved voxels; a one-cell-thick volume would lose most of its cells to them
        weights[rng.random(shape) < 0.03] = 0
    ids = rng.integers(0, 256, size=shape).astype(np.uint8)
    return Case(name, vol, weights, ids, iso, origin, res)


def _scan_case(name):
    """Noise under a weight mask that observes whole blocks: a block (i, y tile, z tile) that is drawn has every voxel its
    cells touch at weight 3.  A block that is not drawn stays empty unless both of its x neighbours are drawn (its voxels at
    x = i come from the one, those at x = i + 1 from the other), so the first and the last block are empty exactly when
    they are not drawn."""
    shape, n_blocks, iso, origin, res, share, first, last = SCAN[name]
    rng = np.random.default_rng(_seed(name))
    vol = noise(shape, rng)
    gz, gy, gx = mesh_ref.blocks(shape)
    drawn = rng.random((gx, gy, gz)) < share
    drawn.reshape(-1)[0], drawn.reshape(-1)[-1] = first, last
    weights = np.zeros(shape, dtype=np.float16)
    for i, yt, zt in np.argwhere(drawn):
        weights[i:i + 2, 4 * yt:4 * yt + 5, 64 * zt:64 * zt + 65] = 3
    ids = rng.integers(0, 256, size=shape).astype(np.uint8)
    return Case(name, vol, weights, ids, iso, origin, res)


def _value_case(name):
    iso, origin, res = VALUE[name]
    rng = np.random.default_rng(_seed(name))
    shape = VALUE_SHAPE
    weights = np.full(shape, 3.0, dtype=np.float16)
    weights[rng.random(shape) < 0.02] = 0
    if name == 'ties':
        # +-1 at iso 0: every crossing has t = 0.5 exactly, every off-grid coordinate is x.5, every label a to-even decision
        vol = rng.choice(np.array([-1.0, 1.0], dtype=np.float16), size=shape)
    elif name == 'on_iso':
        # an outside end that holds +-0 puts the crossing at t = 1 exactly, on that grid point (t = 0 cannot happen: the
        # inside end is < iso); edges that meet there give the same vertex: zero-area triangles, winding dots of exactly 0
        vol = rng.choice(np.array([-0.5, -0.25, -0.0, 0.0, 0.25, 0.5], dtype=np.float16), size=shape)
    elif name == 'extremes':
        sub = 2.0 ** -24
        pool = np.array([sub, -sub, 2 * sub, 3 * sub, -3 * sub, 1023 * sub, 2.0 ** -14, -2.0 ** -14, 65504.0, -65504.0, 1.0, -1.0],
                        dtype=np.float16)
        vol = rng.choice(pool, size=shape)
    elif name == 'masked':
        vol = noise(shape, rng)
        vol[rng.random(shape) < 0.02] = np.nan
        pool = np.array([0.0, -0.0, -1.0, np.nan, SUBNORMAL, 3.0], dtype=np.float16)
        weights = rng.choice(pool, size=shape, p=[0.02, 0.02, 0.02, 0.02, 0.12, 0.8])
    ids = rng.integers(0, 256, size=shape).astype(np.uint8)
    return Case(name, vol, weights, ids, iso, origin, res)


@functools.lru_cache(maxsize=None)
def case(name):
    c = (_tile_case if name in TILE else _scan_case if name in SCAN else _value_case)(name)
    for a in (c.vol, c.weights, c.ids):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(name, weights=True, ids=True):
    """mesh_ref.triangles of a case, computed once (optionally without its weights or ids)."""
    c = case(name)
    ref = mesh_ref.triangles(c.vol, c.iso, c.weights if weights else None, c.ids if ids else None, c.origin, c.res)
    for a in ref:
        if a is not None:
            a.setflags(write=False)
    return ref


# ---- point sets for ojf_points_within -----------------------------------------------------------------------------------
PointSet = collections.namedtuple('PointSet', 'name query points tau group expect')
PointSet.__doc__ = """expect: None (whatever mesh_ref.within says), True (every query must hit) or False (none may)."""
BOX_PARAMS = [(5000, 7000, 0.05), (3000, 100, 0.3), (1, 1, 0.01), (4000, 4000, 1e-4), (2000, 3000, 2.5), (3000, 3000, 1e-7),
              (500, 800, 0.0)]
FLAT_TAUS = [0.0, 1e-7, 1e-4, 0.05]
LATTICE_TAU = 2.0 ** -4


def _box(n_q, n_p, rng):
    p = rng.random((n_p, 3)) * [2.0, 1.0, 3.0] + [-1.0, 5.0, 0.25]
    q = rng.random((n_q, 3)) * [2.4, 1.4, 3.4] + [-1.2, 4.8, 0.05]  # some queries leave the cell grid
    q[: n_q // 10] = p[rng.integers(0, n_p, n_q // 10)]  # exact hits at distance 0
    return q, p


def _near(p, n_q, tau, rng):
    """Queries around a set: a third exact copies, a third at about tau from a point, a third well away."""
    pick = p[rng.integers(0, p.shape[0], n_q)].copy()
    step = rng.normal(size=(n_q, 3))
    step /= np.linalg.norm(step, axis=1, keepdims=True)
    third = n_q // 3
    pick[third:2 * third] += step[third:2 * third] * (tau * rng.uniform(0.5, 1.5, size=(third, 1)))
    pick[2 * third:] += step[2 * third:] * rng.uniform(0.1, 0.6, size=(n_q - 2 * third, 1))
    return pick


@functools.lru_cache(maxsize=None)
def point_sets():
    out = []
    # (a) the box-shaped sets of test_points_within_matches_kdtree
    for n_q, n_p, tau in BOX_PARAMS:
        q, p = _box(n_q, n_p, np.random.default_rng(n_q + n_p))
        out.append(PointSet('box_%d_%d_%g' % (n_q, n_p, tau), q, p, tau, 'a', None))
    # (b) flat and degenerate sets: what surface_points returns for an axis-aligned wall
    rng = np.random.default_rng(77)
    plane = np.concatenate([rng.random((3000, 2)) * [2.0, 1.0] + [-1.0, 5.0], np.full((3000, 1), 0.25)], axis=1)
    line = np.stack([rng.random(2000) * 3.0 - 1.0, np.full(2000, 5.5), np.full(2000, -0.75)], axis=1)
    dot = np.tile(np.array([[0.3, -1.7, 2.9]]), (500, 1))
    for name, p in (('plane', plane), ('line', line), ('dot', dot)):
        for tau in FLAT_TAUS:
            out.append(PointSet('%s_%g' % (name, tau), _near(p, 600, tau, rng), p, tau, 'b', None))
    # (c) dyadic lattice: points at lo + k * tau for even k, queries = the points moved by exactly +-tau along one axis (at
    # distance tau, computed without rounding, on the border of the neighbouring cell: must hit), two axes (sqrt 2 tau: must
    # miss) and three axes (sqrt 3 tau: must miss)
    tau = LATTICE_TAU
    k = np.stack(np.meshgrid(np.arange(0, 12, 2), np.arange(0, 10, 2), np.arange(0, 8, 2), indexing='ij'), axis=-1).reshape(-1, 3)
    lattice = np.array([-1.0, 5.0, 0.25]) + k * tau
    for n_axes in (1, 2, 3):
        shifts = [s for s in np.stack(np.meshgrid(*[[-1, 0, 1]] * 3, indexing='ij'), axis=-1).reshape(-1, 3)
                  if np.count_nonzero(s) == n_axes]
        q = np.concatenate([lattice + np.array(s) * tau for s in shifts], axis=0)
        out.append(PointSet('lattice_%d' % n_axes, q, lattice, tau, 'c', n_axes == 1))
    # a voxel-aligned set, as the surface points of a wall are: 22 sites per axis at res 0.0125 and tau = 1.5 res, where the
    # extent over the cell is 13.999999999999998 but the extent times the reciprocal of the cell is 14: the binning has to
    # divide the way bin_grid and the kernel do, or the last layer leaves the grid
    res = 0.0125
    k = np.stack(np.meshgrid(*[np.arange(22)] * 3, indexing='ij'), axis=-1).reshape(-1, 3)
    wall = -0.3 + (k + 0.5) * res
    out.append(PointSet('voxel_sites', _near(wall, 900, 1.5 * res, rng), wall, 1.5 * res, 'c', None))
    # (d) queries that are not finite, absurdly far, or far outside the grid on one axis only
    q, p = _box(400, 900, np.random.default_rng(5))
    q[0], q[1], q[2] = [np.nan, 5.5, 1.0], [0.0, np.inf, 1.0], [0.0, 5.5, -np.inf]
    q[3], q[4], q[5] = [1e30, 5.5, 1.0], [0.0, -1e30, 1.0], p[0] + [0.0, 0.0, np.nan]
    q[6:40] = p[6:40] + np.eye(3)[np.arange(34) % 3] * np.where(np.arange(34) % 2, 1e6, -1e6)[:, None]
    q[40:60] = p[40:60]
    out.append(PointSet('odd_queries', q, p, 0.05, 'd', None))
    # (e) every query a hit, at query counts around the wave (64) and block (256) sizes: the ballot / popcount sum over
    # partly filled waves and blocks must give n_query
    p = np.random.default_rng(6).random((700, 3)) * [2.0, 1.0, 3.0] + [-1.0, 5.0, 0.25]
    for n_q in (1, 63, 64, 65, 255, 256, 257):
        out.append(PointSet('all_hit_%d' % n_q, p[:n_q] + 1e-3, p, 0.01, 'e', True))
    for s in out:
        s.query.setflags(write=False)
        s.points.setflags(write=False)
    return tuple(out)
