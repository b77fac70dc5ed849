"""No GPU: proves the reference (mesh_ref.py) and the cases (mesh_cases.py) that test_mesh_edges_gpu.py holds the mesh
kernels to.  The reference is checked against the older, independent count / vertex-set statements, against geometry
(closed oriented manifolds), and against its own definition where that can be read back (keys, labels, order); every
property that justifies a case is asserted here from the reference alone; the bin grid of mesh.points_within is checked
through mesh.bin_grid."""
import json
import math
import os

import numpy as np
import pytest

import mesh_cases
import mesh_ref
from online_joint_depthfusion_and_semantic_amd import mesh

CORNER = mesh_ref.CORNER


@pytest.mark.parametrize('name', mesh_cases.ALL_NAMES)
def test_reference_agrees_with_count_and_vertex_set(name):
    c, ref = mesh_cases.case(name), mesh_cases.reference(name)
    valid = mesh_ref.np_cell_valid(c.vol, c.weights)
    T = ref.tri.shape[0]
    assert T == mesh_ref.np_triangle_count(c.vol, np.float32(c.iso), valid)
    assert T > 0 and int(ref.counts.sum()) == T and ref.counts.shape[0] == int(np.prod(mesh_ref.blocks(c.vol.shape)))
    assert T <= 330000  # the GPU test stays quick
    got = np.unique(ref.tri.reshape(-1, 3), axis=0)
    want = mesh_ref.np_vertex_set(c.vol, c.iso, valid, c.origin, c.res)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert np.isfinite(ref.tri).all()
    # without weights: the same statement on the larger list
    if name not in mesh_cases.SCAN:
        free = mesh_cases.reference(name, weights=False)
        assert free.tri.shape[0] == mesh_ref.np_triangle_count(c.vol, np.float32(c.iso), mesh_ref.np_cell_valid(c.vol, None)) >= T


@pytest.mark.parametrize('name', mesh_cases.ALL_NAMES)
def test_reference_order_keys_and_labels(name):
    c, ref = mesh_cases.case(name), mesh_cases.reference(name)
    X, Y, Z = c.vol.shape
    # order: block, row in the block, lane, tetrahedron; at most two triangles share all four
    rank = (((mesh_ref.block_of(ref.cell, c.vol.shape) * 4 + ref.cell[:, 1] % 4) * 64 + ref.cell[:, 2] % 64) * 6 + ref.tet)
    assert (np.diff(rank) >= 0).all() and np.bincount(np.unique(rank, return_counts=True)[1]).shape[0] <= 3
    assert np.array_equal(np.bincount(mesh_ref.block_of(ref.cell, c.vol.shape), minlength=ref.counts.shape[0]), ref.counts)
    # every key decodes to a Kuhn edge of the triangle's own cell that contains the vertex
    key = ref.keys.astype(np.int64)
    lin, code = key // 8, key % 8
    lo = np.stack([lin // (Y * Z), (lin // Z) % Y, lin % Z], axis=-1)
    d = np.stack([code & 1, (code >> 1) & 1, (code >> 2) & 1], axis=-1)
    assert (code > 0).all() and ((lo >= ref.cell[:, None]) & (lo + d <= ref.cell[:, None] + 1)).all()
    p = ref.index.astype(np.float64)
    assert ((p >= lo) & (p <= lo + d)).all()
    on_line = (p - lo) * (1 - d)  # no offset on the axes the edge does not advance on
    assert (on_line == 0).all()
    t = np.where(d == 1, p - lo, np.nan)  # one parameter along the edge on every axis it advances on
    assert (np.nanmax(t, axis=-1) - np.nanmin(t, axis=-1) <= 2.0 ** -13).all()  # each rounded to fp32 at its own index < 1024
    # equal keys <=> the same edge: bit-equal positions
    flat_key, flat_pos = key.reshape(-1), ref.tri.reshape(-1, 3)
    order = np.argsort(flat_key, kind='stable')
    same = flat_key[order][1:] == flat_key[order][:-1]
    assert np.array_equal(flat_pos[order][1:][same].view(np.uint32), flat_pos[order][:-1][same].view(np.uint32))
    # labels: the id of the voxel np.rint names
    r = np.rint(ref.index).astype(np.int64)
    assert np.array_equal(ref.labels, c.ids[r[..., 0], r[..., 1], r[..., 2]])
    assert mesh_cases.reference(name, ids=False).labels is None
    # world position
    world = (np.asarray(c.origin)[None, None] + ref.index.astype(np.float64) * c.res).astype(np.float32)
    assert np.array_equal(world, ref.tri)


def test_world_transform_case_differs_from_fp32():
    """The origin of magnitude 1e3 at res 0.0125 is there so that an fp32 transform would be caught."""
    c, ref = mesh_cases.case('scan_1025'), mesh_cases.reference('scan_1025')
    fp32 = np.asarray(c.origin, dtype=np.float32)[None, None] + ref.index * np.float32(c.res)
    assert (fp32 != ref.tri).mean() > 0.05
    isos = [mesh_cases.case(n).iso for n in mesh_cases.ALL_NAMES if n not in ('ties', 'on_iso')]
    assert len(set(float(i) for i in isos)) == len(isos) and min(isos) < 0
    frames = [(mesh_cases.case(n).origin, mesh_cases.case(n).res) for n in mesh_cases.ALL_NAMES]
    assert len(set(frames)) == len(frames)


def test_block_counts():
    want = {(3, 5, 65): (1, 1, 2), (3, 6, 66): (2, 2, 2), (2, 2, 66): (2, 1, 1), (5, 7, 131): (3, 2, 4), (2, 2, 2): (1, 1, 1),
            (9, 33, 5): (1, 8, 8), (2, 3, 3): (1, 1, 1), (32, 44, 131): (3, 11, 31), (129, 33, 10): (1, 8, 128),
            (42, 98, 5): (1, 25, 41), (684, 4, 131): (3, 1, 683), (64, 64, 64): (1, 16, 63), (256, 256, 256): (4, 64, 255)}
    for shape, grid in want.items():
        assert mesh_ref.blocks(shape) == grid
    for name, row in mesh_cases.SCAN.items():
        assert int(np.prod(mesh_ref.blocks(row[0]))) == row[1]
    assert sorted(row[1] for row in mesh_cases.SCAN.values()) == [1, 1023, 1024, 1025, 2049]
    assert [mesh_cases.TILE[n][0] for n in mesh_cases.TILE_NAMES] == [(3, 5, 65), (3, 6, 66), (2, 2, 66), (5, 7, 131), (2, 2, 2), (9, 33, 5)]


# ---- the property behind every case ------------------------------------------------------------------------------------
def test_tile_cases_reach_their_tiles():
    for name in mesh_cases.TILE_NAMES:
        c, ref = mesh_cases.case(name), mesh_cases.reference(name)
        X, Y, Z = c.vol.shape
        assert (ref.cell[:, 1] == Y - 2).any(), name  # the last cell row: the last row of a partly filled y tile where there is one
        assert (ref.cell[:, 0] == X - 2).any() and (ref.cell[:, 0] == 0).any(), name
    k = mesh_cases.reference('tile_65').cell[:, 2]
    assert k.max() == 63  # lane 63 of the one full wave
    for name in ('tile_66', 'tile_66_row'):
        assert mesh_cases.reference(name).cell[:, 2].max() == 64, name  # the single cell of the second z tile
    cell = mesh_cases.reference('tile_66').cell
    assert (cell[:, 1] == 4).any() and (6 - 1) % 4 == 1  # the y tile with one row
    assert (mesh_cases.reference('tile_131').cell[:, 2] >= 128).any()
    assert ((mesh_cases.reference('tile_131').cell[:, 2] >= 64) & (mesh_cases.reference('tile_131').cell[:, 2] < 128)).any()
    partly = mesh_cases.reference('tile_131').cell
    assert (partly[:, 1] == 5).any() and (7 - 1) % 4 != 0  # rows 4, 5 of a y tile of 4
    assert mesh_cases.reference('tile_min').cell.max() == 0
    assert (mesh_cases.reference('tile_y33').cell[:, 1] // 4 == 7).any()


def test_scan_cases_reach_their_chunks():
    for name in mesh_cases.SCAN_NAMES:
        ref = mesh_cases.reference(name)
        n = mesh_cases.SCAN[name][1]
        assert ref.counts.shape[0] == n
        if n > 1:
            full = np.nonzero(ref.counts)[0]
            assert (ref.counts[full[0]:full[-1]] == 0).any(), name  # an empty block strictly between two non-empty ones
    assert mesh_cases.reference('scan_1023').counts[0] == 0 and mesh_cases.reference('scan_1023').counts[-1] > 0
    assert mesh_cases.reference('scan_1024').counts[-1] == 0 and mesh_cases.reference('scan_1024').counts[0] > 0
    for name, chunk in (('scan_1', 1), ('scan_1023', 1), ('scan_1024', 1), ('scan_1025', 2), ('scan_2049', 3)):
        assert (mesh_cases.SCAN[name][1] + 1023) // 1024 == chunk
    counts = mesh_cases.reference('scan_2049').counts
    # chunk 3: thread t owns blocks [3t, 3t + 3).  Thread 682 is the last with work, thread 683 starts exactly at n (an empty
    # range that must read and write nothing), the threads above start past n.
    assert 683 * 3 == counts.shape[0] and 684 * 3 > counts.shape[0]
    assert counts[0:3].any() and counts[3 * 682:3 * 683].any() and counts[3 * 341:3 * 342 + 30].any()
    half = mesh_cases.reference('scan_1025').counts
    assert half[0:2].any() and half[1024] > 0  # chunk 2: thread 512 owns the single block 1024


def test_value_cases_hold_their_properties():
    # ties: every vertex has a coordinate at x.5, and the to-even rule goes both ways
    ref = mesh_cases.reference('ties')
    p = ref.index.reshape(-1, 3).astype(np.float64)
    tie = (p - np.floor(p)) == 0.5
    assert tie.any(axis=1).all()
    lower = np.floor(p)[tie].astype(np.int64)
    assert (lower % 2 == 0).any() and (lower % 2 == 1).any()
    # on_iso: collapsed triangles and winding dots of exactly zero
    ref = mesh_cases.reference('on_iso')
    t = ref.index.astype(np.float64)
    area2 = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    flat = (area2 == 0).all(axis=1)
    assert flat.mean() >= 0.01 and (ref.dot == 0).any()
    assert (ref.dot < 0).any() and (ref.dot > 0).any()
    c = mesh_cases.case('on_iso')
    assert (np.signbit(c.vol) & (c.vol == 0)).any() and (~np.signbit(c.vol) & (c.vol == 0)).any()
    # extremes: an iso no fp16 holds, subnormals and the largest finite values at the two ends of crossing edges
    c, ref = mesh_cases.case('extremes'), mesh_cases.reference('extremes')
    assert np.float32(np.float16(c.iso)) != np.float32(c.iso) and np.isfinite(c.vol).all()
    a, b = np.abs(c.vol[:, :, :-1].astype(np.float32)), np.abs(c.vol[:, :, 1:].astype(np.float32))
    assert ((a < 2.0 ** -14) & (a > 0) & (b == 65504)).any() and np.isfinite(ref.tri).all() and np.isfinite(ref.dot).all()


def test_masked_case_kills_and_keeps():
    c, ref = mesh_cases.case('masked'), mesh_cases.reference('masked')
    X, Y, Z = c.vol.shape
    w = c.weights
    kind = np.zeros(c.vol.shape, dtype=np.int64)  # 0: fine; one bit per way of being unobserved
    kind |= np.isnan(c.vol) * 1
    kind |= ((w == 0) & ~np.signbit(w)) * 2
    kind |= ((w == 0) & np.signbit(w)) * 4
    kind |= (w < 0) * 8
    kind |= np.isnan(w) * 16
    v = c.vol.astype(np.float32)
    cell_kind = np.zeros((X - 1, Y - 1, Z - 1), dtype=np.int64)
    n_in = np.zeros(cell_kind.shape, dtype=np.int64)
    n_out = np.zeros(cell_kind.shape, dtype=np.int64)
    sub = np.zeros(cell_kind.shape, dtype=bool)
    for o in CORNER:
        sl = (slice(o[0], X - 1 + o[0]), slice(o[1], Y - 1 + o[1]), slice(o[2], Z - 1 + o[2]))
        cell_kind |= kind[sl]
        with np.errstate(invalid='ignore'):
            n_in += v[sl] < np.float32(c.iso)
            n_out += v[sl] >= np.float32(c.iso)
        sub |= w[sl] == mesh_cases.SUBNORMAL
    crossing = (n_in > 0) & (n_out > 0)  # the corners that hold a value lie on both sides
    emitted = np.zeros(cell_kind.shape, dtype=bool)
    emitted[ref.cell[:, 0], ref.cell[:, 1], ref.cell[:, 2]] = True
    assert np.array_equal(emitted, crossing & (cell_kind == 0))
    for bit in (1, 2, 4, 8, 16):
        assert (crossing & (cell_kind == bit)).any(), bit  # this kind alone kills a cell that would emit
    assert (emitted & sub).any()  # the smallest subnormal weight is observed


# ---- closed surfaces: the reference list alone is a consistently oriented 2-manifold ------------------------------------
def _closed_cases():
    n = 32
    g = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing='ij'), axis=-1).astype(np.float64)
    yield 'sphere', np.clip(np.linalg.norm(g - (15.5 + 0.137), axis=-1) - 10.3, -4, 4).astype(np.float16)
    cases = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'mesh_analytic_cases.json')))['cases']
    torus = [k for k in cases if k['name'] == 'torus'][0]  # the fixture is stated for 64^3: half of every length
    q = g - np.asarray(torus['centre']) / 2
    ring = np.sqrt(q[..., 0] ** 2 + q[..., 1] ** 2) - torus['R'] / 2
    yield 'torus', np.clip(np.sqrt(ring ** 2 + q[..., 2] ** 2) - torus['r'] / 2, -4, 4).astype(np.float16)


def test_reference_list_is_a_closed_oriented_manifold():
    for name, vol in _closed_cases():
        ref = mesh_ref.triangles(vol, 0.0)
        key = ref.keys.astype(np.int64)
        assert key.shape[0] > 1000, name
        assert (key[:, 0] != key[:, 1]).all() and (key[:, 1] != key[:, 2]).all() and (key[:, 0] != key[:, 2]).all(), name
        e = np.concatenate([key[:, [0, 1]], key[:, [1, 2]], key[:, [2, 0]]], axis=0)
        fwd = np.unique(e, axis=0)
        assert fwd.shape[0] == e.shape[0], name  # every directed edge once
        assert np.array_equal(fwd, np.unique(e[:, ::-1], axis=0)), name  # and its reverse once
        t = ref.tri.astype(np.float64)
        assert ((t[:, 0] * np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])).sum() / 6.0) > 100.0, name  # outward: volume > 0
        flat_key, flat_pos = key.reshape(-1), ref.tri.reshape(-1, 3)
        order = np.argsort(flat_key, kind='stable')
        same = flat_key[order][1:] == flat_key[order][:-1]
        assert np.array_equal(flat_pos[order][1:][same], flat_pos[order][:-1][same]), name
        n_vert, n_edge, n_face = np.unique(flat_key).size, e.shape[0] // 2, key.shape[0]
        assert n_vert - n_edge + n_face == (2 if name == 'sphere' else 0), name


# ---- points_within: the brute-force statement and the bin grid ----------------------------------------------------------
@pytest.mark.parametrize('group', ['a', 'c', 'e'])
def test_within_agrees_with_kdtree(group):
    from scipy.spatial import cKDTree
    for s in mesh_cases.point_sets():
        if s.group != group:
            continue
        want = cKDTree(s.points).query(s.query)[0] <= s.tau
        got = mesh_ref.within(s.query, s.points, s.tau)
        assert np.array_equal(got, want), s.name
        if s.expect is not None:
            assert (got == s.expect).all(), s.name


def test_point_sets_cover_what_they_claim():
    sets = {s.name: s for s in mesh_cases.point_sets()}
    assert sorted(set(s.group for s in sets.values())) == ['a', 'b', 'c', 'd', 'e']
    for name in ('plane', 'line', 'dot'):
        for tau in mesh_cases.FLAT_TAUS:
            s = sets['%s_%g' % (name, tau)]
            flat = np.ptp(s.points, axis=0) == 0
            assert flat.sum() == {'plane': 1, 'line': 2, 'dot': 3}[name]
            hit = mesh_ref.within(s.query, s.points, tau)
            assert hit.any() and not hit.all(), s.name
    s = sets['lattice_1']
    cell, G = mesh.bin_grid(s.points.min(axis=0), np.ptp(s.points, axis=0), s.tau)
    assert cell == s.tau  # so the single shift lands exactly on a cell border, in the neighbouring cell
    f = (s.query - s.points.min(axis=0)) / cell
    assert (f == np.floor(f)).all() and (f.min() == -1) and (f.max(axis=0) == G).all()
    d = np.sqrt(((s.query[:, None] - s.points[None]) ** 2).sum(-1)).min(axis=1)
    assert (d == s.tau).all()
    s = sets['voxel_sites']
    span, (cell, G) = np.ptp(s.points, axis=0), mesh.bin_grid(s.points.min(axis=0), np.ptp(s.points, axis=0), s.tau)
    assert cell == s.tau and (np.floor(span / cell) + 1 == G).all() and (np.floor(span * (1.0 / cell)) + 1 > G).all()
    top = s.points.max(axis=0)
    assert mesh_ref.within(s.query, s.points[(s.points == top).any(axis=1)], s.tau).any()  # hits that need the last layer
    q = sets['odd_queries'].query
    assert np.isnan(q).any() and np.isposinf(q).any() and np.isneginf(q).any() and (np.abs(q[np.isfinite(q)]) == 1e30).sum() == 2
    hit = mesh_ref.within(q, sets['odd_queries'].points, 0.05)
    assert not hit[:40].any() and hit[40:60].all()
    assert [sets['all_hit_%d' % n].query.shape[0] for n in (1, 63, 64, 65, 255, 256, 257)] == [1, 63, 64, 65, 255, 256, 257]


def _check_grid(lo, span, tau, points=None):
    cell, G = mesh.bin_grid(lo, span, tau)
    assert isinstance(cell, float) and math.isfinite(cell) and cell > 0 and cell >= tau
    assert all(isinstance(g, int) and g >= 1 for g in G)
    assert G[0] * G[1] * G[2] <= mesh.MAX_BINS == 1 << 24  # the exact bound: no slack
    for a in range(3):
        assert G[a] == int(math.floor(max(float(span[a]), 0.0) / cell)) + 1
        if span[a] < cell:
            assert G[a] == 1
    if points is not None:  # the sort key of points_within stays inside the grid
        c = np.floor((points - np.asarray(lo)) / cell).astype(np.int64)
        assert (c >= 0).all() and (c.max(axis=0) == np.asarray(G) - 1).all()
    return cell, G


def test_bin_grid_is_bounded_on_every_set():
    """Fails on the parent's sizing, which took the cube root over all three extents: the plane set at tau = 1e-7 got
    87556 x 43763 x 1 = 3.8e9 bins, and at tau = 0 about 4e12 per axis."""
    for s in mesh_cases.point_sets():
        if s.group in 'abc':
            lo = s.points.min(axis=0)
            _check_grid(lo.tolist(), (s.points.max(axis=0) - lo).tolist(), s.tau, s.points)
    sets = {s.name: s for s in mesh_cases.point_sets()}
    for tau in (0.0, 1e-7):
        p = sets['plane_%g' % tau].points
        cell, G = _check_grid(p.min(axis=0).tolist(), np.ptp(p, axis=0).tolist(), tau, p)
        assert G[2] == 1 and G[0] * G[1] > (1 << 23)  # the cap is shared between the two axes that have an extent
    p = sets['dot_0'].points
    assert _check_grid(p[0].tolist(), [0.0, 0.0, 0.0], 0.0, p)[1] == [1, 1, 1]
    # a set that never needed coarsening keeps cell = tau
    assert _check_grid([0.0, 0.0, 0.0], [2.0, 1.0, 3.0], 0.05)[0] == 0.05


def test_bin_grid_never_overflows():
    big, tiny = 1e300, 1e-300
    for span in ([big, big, big], [big, 1.0, tiny], [tiny, tiny, tiny], [5e-324, 0.0, 1.0], [big, 0.0, 0.0], [1.0, 1.0, big],
                 [3.0, 3.0 * 2.0 ** -24, 0.0], [1.0, 1.0, 1.0]):
        for tau in (0.0, 5e-324, 1e-30, 1e-7, 1.0, 1e300):
            _check_grid([-1.0, 2.0, 3.0], span, tau)
    for bad in (float('nan'), -1.0):
        with pytest.raises(ValueError):
            mesh.bin_grid([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], bad)
    with pytest.raises(ValueError):
        mesh.bin_grid([0.0, 0.0, 0.0], [1.0, float('inf'), 1.0], 0.1)
