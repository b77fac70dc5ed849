"""CPU: the numpy restatement of the mesh simplification (simplify_ref.py) held to its own definition - exact
integer sums, independence of the order of faces and vertices, the overflow bound on a worst-case fan, closed surfaces that stay
closed, and the quality the quadric buys over the cell mean - and the Python layer's argument checks, which need no device."""
import functools

import numpy as np
import pytest
import torch

from online_joint_depthfusion_and_semantic_amd import _lib, mesh_simplify
import mesh_ref
import simplify_ref as ref

f32 = np.float32


def _grid(v, cell):
    return ref.default_grid(v.min(axis=0), v.max(axis=0), cell)


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_exact_sums_equal_python_integers(seed):
    """A, b, S and cnt of every cluster against sums of Python ints formed face by face from the definition."""
    v, f = ref.random_mesh(seed, 300, 900, span=3.0)
    cell = f32(0.75)
    lo, G = _grid(v, cell)
    r = ref.cluster(v, f, lo, cell, G)
    idx, p = ref.locate(v, lo, cell, G)
    counts, n, w = ref.face_terms(v, f, idx >= 0, cell)
    assert counts.sum() > 500 and len(r.vertices) > 20
    A = [[0] * 6 for _ in r.vertices]
    b = [[0] * 3 for _ in r.vertices]
    S = [[0] * 3 for _ in r.vertices]
    cnt = [0] * len(r.vertices)
    for i in range(len(v)):
        c = int(r.cluster[i])
        cnt[c] += 1
        for a in range(3):
            S[c][a] += int(p[i, a])
    for j in np.flatnonzero(counts):
        nn, ww = [int(x) for x in n[j]], int(w[j])
        assert 1 <= ww <= ref.WEIGHT_MAX and max(abs(x) for x in nn) <= ref.NORMAL_MAX
        for k in range(3):
            i = int(f[j, k])
            c = int(r.cluster[i])
            d = -sum(nn[a] * int(p[i, a]) for a in range(3))
            for q, (x, y) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                A[c][q] += ww * nn[x] * nn[y]
            for a in range(3):
                b[c][a] += ww * d * nn[a]
    assert r.A.tolist() == A and r.b.tolist() == b and r.S.tolist() == S and r.cnt.tolist() == cnt
    assert np.abs(p).max() <= ref.POS_MAX


def test_order_independence():
    """Permuting the faces and the vertices changes no output position and no face set (source follows the vertices)."""
    v, f = ref.random_mesh(5, 400, 1500, span=3.0)
    cell = f32(0.6)
    lo, G = _grid(v, cell)
    base = ref.cluster(v, f, lo, cell, G)
    rng = np.random.default_rng(11)
    fperm = rng.permutation(len(f))
    r = ref.cluster(v, f[fperm], lo, cell, G)
    assert np.array_equal(r.vertices.view(np.uint32), base.vertices.view(np.uint32))
    assert np.array_equal(r.source, base.source)
    assert sorted(map(tuple, r.faces.tolist())) == sorted(map(tuple, base.faces.tolist()))
    assert np.array_equal(np.sort(fperm[r.face_source]), base.face_source)
    vperm = rng.permutation(len(v))  # new vertex i is old vertex vperm[i]
    inv = np.argsort(vperm)
    r = ref.cluster(v[vperm], inv[f].astype(np.int32), lo, cell, G)
    assert np.array_equal(r.vertices.view(np.uint32), base.vertices.view(np.uint32))
    assert np.array_equal(r.faces, base.faces) and np.array_equal(r.face_source, base.face_source)
    assert np.array_equal(r.cluster[inv], base.cluster)


def test_overflow_bound_on_a_worst_case_fan():
    """The terms of step 4 at their limits: a fan of faces with the normal (512, 512, 512)-ish clamp, weight 1024 and the corners
    in the far corner of their cell.  One incidence adds at most 3 2^35 to b and 2^28 to A; 3 2^24 incidences stay below 2^63."""
    # normal along an axis gives |n| = 512 exactly; a large face gives w = 1024; p = (-128, -128, -128) at the cell's low corner
    cell = f32(1.0)
    lo, G = np.zeros(3, f32), (4, 4, 4)
    v = np.array([[1, 1, 1], [3, 1, 1], [1, 3, 1]], f32)  # every corner on a cell's low corner: p = -128 on every axis
    fan = 64
    f = np.tile(np.array([[0, 1, 2]], np.int32), (fan, 1))
    r = ref.cluster(v, f, lo, cell, G)
    idx, p = ref.locate(v, lo, cell, G)
    counts, n, w = ref.face_terms(v, f, idx >= 0, cell)
    assert (p == -128).all() and (w == ref.WEIGHT_MAX).all() and (n == [0, 0, ref.NORMAL_MAX]).all()
    term_A, term_b = ref.WEIGHT_MAX * ref.NORMAL_MAX ** 2, ref.WEIGHT_MAX * (ref.NORMAL_MAX * ref.POS_MAX) * ref.NORMAL_MAX
    assert (r.A[:, 5] == fan * term_A).all() and (r.b[:, 2] == fan * term_b).all()
    # the bound of the definition: every |n_i| and |p_i| at its limit at once (no real normal reaches it: |n| <= 512 sqrt(3) / sqrt(3))
    d_max = 3 * ref.NORMAL_MAX * ref.POS_MAX
    b_max, A_max = ref.WEIGHT_MAX * d_max * ref.NORMAL_MAX, ref.WEIGHT_MAX * ref.NORMAL_MAX ** 2
    assert d_max == 3 * 2 ** 16 and b_max == 3 * 2 ** 35 and A_max == 2 ** 28
    incidences = 3 * ref.MAX_FACES
    assert incidences * b_max < 2 ** 63 and 3 * incidences * A_max < 2 ** 63  # (3 x: the trace that gives lam)
    assert ref.POS_MAX * (2 ** 31 - 1) < 2 ** 63
    assert term_b <= b_max and term_A <= A_max
    # the same column of faces scaled to 2^24 incidences still fits an int64 exactly as Python ints
    assert int(r.b[0, 2]) // fan * incidences == term_b * incidences < 2 ** 63


@functools.lru_cache(maxsize=None)
def _closed(name):
    vol = dict(ref.closed_cases())[name]
    t = mesh_ref.triangles(vol, 0.0)
    v, f, _ = ref.weld_keys(t.tri, t.keys)
    return v, f


# measured on this restatement with cells of 2 voxels: the signed volume shrinks by 0.63 % (sphere) and 1.80 % (torus)
VOLUME_CHANGE = {'sphere': 7e-3, 'torus': 2e-2}


@pytest.mark.parametrize('name', ['sphere', 'torus'])
def test_closed_stays_closed(name):
    v, f = _closed(name)
    assert ref.directed_edge_balance(f) == 0 and len(f) > 10000
    before = ref.signed_volume(v, f)
    for cell in (1.0, 2.0, 4.0):
        lo, G = _grid(v, cell)
        r = ref.cluster(v, f, lo, cell, G)
        assert len(r.faces) < len(f) / 2
        assert ref.directed_edge_balance(r.faces) == 0, (name, cell)  # dropped faces cancel their own edges: exact
        uf, _ = ref.unique_faces(r.faces, r.face_source)
        assert len(uf) <= len(r.faces)
        if cell == 2.0:
            change = abs(ref.signed_volume(r.vertices, r.faces) - before) / before
            print(name, 'relative volume change at 2 voxels per cell: %.4e' % change)
            assert change < VOLUME_CHANGE[name], (name, change)


def _cube_quality(cell):
    """Per cluster of the tessellated unit cube: how many cube planes its members lie on, and the distance (in cells) of the
    quadric representative and of the cell mean to that plane / edge line / corner; and the distance to the cube's surface."""
    v, f = ref.tessellated_cube(32)
    lo = np.array([-0.013, -0.027, -0.031], f32)  # no cube face on a cell border
    G = tuple(int(np.floor((1.0 - l) / cell)) + 2 for l in lo)
    r = ref.cluster(v, f, lo, cell, G)
    on = (v == 0) | (v == 1)
    planes = np.zeros((len(r.vertices), 3), bool)
    np.logical_or.at(planes, r.cluster, on)
    coord = np.zeros((len(r.vertices), 3))
    for a in range(3):
        coord[r.cluster[on[:, a]], a] = v[on[:, a], a]
    g = np.stack([r.cell // (G[1] * G[2]), (r.cell // G[2]) % G[1], r.cell % G[2]], axis=1)
    mean = lo.astype(np.float64) + (g + 0.5 + (r.S / r.cnt[:, None]) / 256.0) * np.float64(f32(cell))
    P = r.vertices.astype(np.float64)
    dist = np.sqrt((np.where(planes, P - coord, 0) ** 2).sum(axis=1)) / cell
    dist_mean = np.sqrt((np.where(planes, mean - coord, 0) ** 2).sum(axis=1)) / cell
    inside = ((P >= 0) & (P <= 1)).all(axis=1)
    surface = np.where(inside, np.minimum(P, 1 - P).min(axis=1), np.sqrt((np.maximum(0, np.maximum(-P, P - 1)) ** 2).sum(axis=1))) / cell
    return planes.sum(axis=1), dist, dist_mean, surface


# measured on this restatement, in cells, the larger of the two cell sizes: the representatives are 2.3e-3 off the
# surface and the edge clusters' 3.6e-3 off their edge line (the 2^-9 cell quantisation of the local positions); asserted at 4 x
SURFACE_BAR, EDGE_BAR = 4 * 2.3e-3, 4 * 3.6e-3


@pytest.mark.parametrize('cell', [0.1, 0.23])
def test_quality_on_the_tessellated_cube(cell):
    kind, dist, dist_mean, surface = _cube_quality(cell)
    edge = kind == 2
    assert (kind >= 1).all() and edge.sum() >= 36 and (kind == 3).sum() == 8
    print('cell %.2f: surface %.3e, edge line %.3e, corner %.3e; cell mean of the edge clusters %.3f' % (
        cell, surface.max(), dist[edge].max(), dist[kind == 3].max(), dist_mean[edge].max()))
    assert surface.max() < SURFACE_BAR
    assert dist[edge].max() < EDGE_BAR
    assert dist_mean[edge].max() > 0.1  # the cheap alternative rounds the cube's edges


def test_unique_faces_keeps_orientation():
    faces = np.array([[5, 2, 7], [2, 7, 5], [7, 5, 2], [2, 5, 7], [9, 8, 1], [1, 9, 8]], np.int32)
    uf, src = ref.unique_faces(faces, np.array([10, 11, 12, 13, 14, 15], np.int32))
    assert uf.tolist() == [[1, 9, 8], [2, 5, 7], [2, 7, 5]] and src.tolist() == [14, 13, 10]


def test_default_grid_covers_every_vertex():
    rng = np.random.default_rng(3)
    for cell in (0.02, 0.1, 0.37, 3.0):
        v = rng.uniform(-5, 9, (200, 3)).astype(f32)
        lo, G = ref.default_grid(v.min(axis=0), v.max(axis=0), cell)
        lo2, G2 = mesh_simplify.default_grid(v.min(axis=0), v.max(axis=0), cell)
        assert np.array_equal(lo, lo2) and tuple(G) == tuple(G2)
        idx, _ = ref.locate(v, lo, cell, G)
        assert (idx >= 0).all() and (lo <= v.min(axis=0)).all()


def test_argument_errors_need_no_device():
    """cluster refuses bad arguments before it touches a device (host tensors reach the last check only)."""
    v, f = torch.zeros((4, 3)), torch.zeros((2, 3), dtype=torch.int32)
    bad = [dict(cell=0.0), dict(cell=-1.0), dict(cell=float('nan')), dict(cell=float('inf')), dict(cell=1e-60), dict(cell=True),
           dict(cell=1.0, lo=(0, 0, 0)), dict(cell=1.0, grid=(1, 1, 1)), dict(cell=1.0, lo=(0, float('nan'), 0), grid=(1, 1, 1)),
           dict(cell=1.0, lo=(0, 0, 0), grid=(0, 1, 1)), dict(cell=1.0, lo=(0, 0, 0), grid=(2048, 1024, 1024)),
           dict(cell=1.0, lo=(0, 0), grid=(1, 1, 1)), dict(cell=1.0)]  # (the last: host tensors)
    for kw in bad:
        with pytest.raises(ValueError):
            mesh_simplify.cluster(v, f, **kw)
    with pytest.raises(ValueError):
        mesh_simplify.cluster(v.double(), f, 1.0)
    with pytest.raises(ValueError):
        mesh_simplify.cluster(v, f.long(), 1.0)
    with pytest.raises(ValueError):
        mesh_simplify.cluster(v.reshape(3, 4), f, 1.0)
    for s in (0, -2, float('nan'), True, 'two'):
        with pytest.raises(ValueError):
            mesh_simplify.voxel_cell(s, 0.01)
    assert mesh_simplify.voxel_cell(2, 0.01) == 0.02


def test_library_refuses_before_any_device_call():
    """ojf_mesh_simplify on a host without a device: every malformed description is refused under the entry point's name."""
    import ctypes
    lib = _lib.load()
    host = ctypes.create_string_buffer(4096)
    dev = (ctypes.addressof(host) + 127) & ~127
    lo = np.zeros(3, f32)
    ws = lib.ojf_mesh_simplify_workspace_bytes(4, 2, 2, 2, 2)
    assert ws == (3 * 4 + 2 * 1 + 1) * 4
    assert lib.ojf_mesh_simplify_workspace_bytes(0, 2, 2, 2, 2) == 0 and lib.ojf_mesh_simplify_workspace_bytes(4, 2 ** 24 + 1, 2, 2, 2) == 0
    assert lib.ojf_mesh_simplify_workspace_bytes(4, 2, 2048, 1024, 1024) == 0 and lib.ojf_mesh_simplify_workspace_bytes(4, 2, 2, 0, 2) == 0
    assert lib.ojf_mesh_simplify_cluster_bytes(0) == 128 and lib.ojf_mesh_simplify_cluster_bytes(7) == 7 * 128
    good = dict(v=dev, nv=4, f=dev + 128, nf=2, lo=lo.ctypes.data, cell=1.0, G=(2, 2, 2), phases=_lib.SIMPLIFY_ALL, ws=dev + 256, ws_bytes=ws,
                rows=dev + 512, rows_bytes=1024, ov=dev + 1536, src=dev + 1664, vcap=4, of=dev + 1792, fsrc=dev + 1920, fcap=2, counts=dev + 2048)
    nan_lo = np.array([0, np.nan, 0], f32)
    cases = [(dict(nv=0), b'nv'), (dict(nf=-1), b'nf'), (dict(nf=2 ** 24 + 1), b'nf'), (dict(G=(0, 2, 2)), b'grid'),
             (dict(G=(2048, 1024, 1024)), b'grid'), (dict(phases=0), b'phases'), (dict(phases=128), b'phases'), (dict(v=None), b'null'),
             (dict(f=None), b'null'), (dict(lo=None), b'null'), (dict(ws=None), b'null'), (dict(counts=None), b'null'),
             (dict(cell=0.0), b'cell'), (dict(cell=float('nan')), b'cell'), (dict(cell=float('inf')), b'cell'), (dict(cell=-1.0), b'cell'),
             (dict(lo=nan_lo.ctypes.data), b'lo'), (dict(ws_bytes=ws - 1), b'workspace too small'), (dict(rows=None), b'clusters_dev'),
             (dict(rows_bytes=127), b'clusters_dev'), (dict(ov=None), b'null'), (dict(src=None), b'null'), (dict(of=None), b'null'),
             (dict(fsrc=None), b'null'), (dict(v=dev + 2), b'aligned'), (dict(ws=dev + 260), b'aligned'), (dict(rows=dev + 576), b'aligned'),
             (dict(counts=dev + 2049), b'aligned')]
    for fault, word in cases:
        d = dict(good, **fault)
        rc = lib.ojf_mesh_simplify(d['v'], d['nv'], d['f'], d['nf'], d['lo'], d['cell'], *d['G'], d['phases'], d['ws'], d['ws_bytes'], d['rows'],
                                   d['rows_bytes'], d['ov'], d['src'], d['vcap'], d['of'], d['fsrc'], d['fcap'], d['counts'], None)
        msg = lib.ojf_last_error()
        assert rc != 0 and msg.startswith(b'ojf_mesh_simplify:') and word in msg, (fault, msg)
