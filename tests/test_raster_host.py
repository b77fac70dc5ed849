"""CPU: the mesh rasteriser's definition (raster_ref.py, the numpy restatement of csrc/ojf_raster.hip) - the coverage of the
GPU parity cases, its accuracy against the analytic ray caster of the synthetic room, the refusals of ojf_rasterize /
ojf_rasterize_attributes without a device, the per-face label property of the PLY writer, and the quality of ground-truth
volumes made from rasterised views."""
import numpy as np

from online_joint_depthfusion_and_semantic_amd import _lib, mesh, metrics, synthetic
import raster_ref as ref


# ---- the GPU parity cases are not vacuous ----------------------------------------------------------------------------------
def test_room_covers_every_pixel_and_matches_the_analytic_ray_caster():
    """20 orbit poses at 48 x 64.  Depth within 5e-6 m of synthetic._raycast (f64, analytic): about 10 ulp of fp32 at the
    room's 5 m; measured 9.3e-7.  Surface ids match exactly."""
    v = ref.room_views()
    assert v['mesh']['vertices'].shape == (32, 3) and v['mesh']['faces'].shape == (48, 3)
    assert v['depth'].shape == (20, 48, 64)
    assert int((v['face'] < 0).sum()) == 0 and (v['depth'] > 0).all()
    worst = 0.0
    for i in range(len(v['E'])):
        d, ids = synthetic._raycast(v['E'][i], v['K'], ref.ROOM_H, ref.ROOM_W)
        worst = max(worst, float(np.abs(v['depth'][i].astype(np.float64) - d).max()))
        assert np.array_equal(v['labels'][i], ids.astype(np.uint8))
    print('room: max |z - raycast| = {:.3e} m'.format(worst))
    assert worst <= 5e-6
    assert len(np.unique(v['labels'])) >= 6 and (v['labels'] >= 7).any()  # (half an orbit: most walls and some solids are seen)


def test_patch_has_no_hole_inside_its_footprint():
    m = ref.bumpy_patch()
    assert m['faces'].shape == (7200, 3)
    depth, face = ref.rasterize(m['vertices'], m['faces'], ref.PATCH_K, ref.PATCH_E, ref.PATCH_SHAPE)
    inside = ref.patch_footprint(m)
    assert inside.sum() > 2000
    assert int((face[0][inside] < 0).sum()) == 0
    assert 0 < (face[0] < 0).sum() < face[0].size - inside.sum() + 1  # the image's border stays empty
    assert len(np.unique(face[0])) > 1500  # sub-pixel triangles: most pixels see a face of their own
    # both windings and both diagonals are among the winners
    f = m['faces'][face[0][face[0] >= 0]].astype(np.int64)
    q = m['quads'] + 1
    spans = np.sort(f, axis=1)
    assert ((spans[:, 2] - spans[:, 0]) == q + 1).any() and ((spans[:, 2] - spans[:, 0]) == q).any()


def test_edge_cases_resolve_as_the_definition_says():
    m = ref.edge_cases()
    depth, face = ref.rasterize(m['vertices'], m['faces'], ref.EDGE_K, ref.EDGE_E, ref.EDGE_SHAPE)
    won = set(np.unique(face[0]).tolist())
    E = ref.EDGE_FACES
    for name in ('background', 'crossing', 'pixel_centres'):
        assert set(E[name]) <= won, name
    for name in ('behind', 'zero_area', 'out_of_range', 'nan_vertex'):
        assert not (set(E[name]) & won), name
    assert E['duplicate'][0] in won and E['duplicate'][1] not in won  # a tie in z goes to the lower face index
    for r, c in ((5, 10), (5, 20), (12, 10)):  # a pixel centre exactly on a vertex is hit, at the vertex's depth
        assert face[0, r, c] == E['pixel_centres'][0] and depth[0, r, c] == 2.0
    # the crossing triangle is seen from the camera plane on: depths from (nearly) 0 up
    z = depth[0][face[0] == E['crossing'][0]]
    assert z.min() < 0.5 and z.max() > 1.5
    # with near = 1 everything nearer disappears, here too
    d1, f1 = ref.rasterize(m['vertices'], m['faces'], ref.EDGE_K, ref.EDGE_E, ref.EDGE_SHAPE, near=1.0)
    assert (d1[f1 >= 0] > 1.0).all() and E['duplicate'][0] not in set(np.unique(f1).tolist())
    labels, rgba = ref.attributes(m['vertices'], m['faces'], ref.EDGE_K, ref.EDGE_E, face, m['face_labels'], m['vertex_colors'])
    assert np.array_equal(labels[0], np.where(face[0] >= 0, face[0] + 1, 0))
    assert np.array_equal(rgba[0, ..., 3], np.where(face[0] >= 0, 255, 0)) and not rgba[0][face[0] < 0].any()
    for r, c, corner in ((5, 10, 0), (5, 20, 1), (12, 10, 2)):  # at a vertex the colour is the vertex's
        assert np.array_equal(rgba[0, r, c, :3], m['vertex_colors'][m['faces'][6][corner], :3])
    # a face image with entries no face answers to counts as "nothing hit"
    bad = face.copy()
    bad[0, 0], bad[0, 1] = len(m['faces']), E['nan_vertex'][0]
    l2, c2 = ref.attributes(m['vertices'], m['faces'], ref.EDGE_K, ref.EDGE_E, bad, m['face_labels'], m['vertex_colors'])
    assert not l2[0, :2].any() and not c2[0, :2].any() and np.array_equal(l2[0, 2:], labels[0, 2:])


# ---- order and colour ------------------------------------------------------------------------------------------------------
def test_face_order_does_not_change_the_depth():
    v = ref.room_views()
    m = v['mesh']
    perm = np.random.default_rng(2).permutation(len(m['faces']))
    depth, face = ref.rasterize(m['vertices'], m['faces'][perm], v['K'], v['E'][:4], (ref.ROOM_H, ref.ROOM_W))
    assert np.array_equal(depth.view(np.uint32), v['depth'][:4].view(np.uint32))
    assert np.array_equal(m['face_labels'][perm][face], v['labels'][:4])


def test_a_constant_colour_per_triangle_comes_back_exact():
    v = ref.room_views()
    m = v['mesh']
    verts = m['vertices'][m['faces']].reshape(-1, 3)  # every triangle gets vertices of its own
    faces = np.arange(len(verts)).reshape(-1, 3)
    per_face = np.random.default_rng(4).integers(0, 256, (len(faces), 4)).astype(np.uint8)
    per_face[:3] = ((0, 255, 1, 9), (255, 0, 254, 9), (128, 127, 129, 9))
    depth, face = ref.rasterize(verts, faces, v['K'], v['E'][:3], (ref.ROOM_H, ref.ROOM_W))
    assert np.array_equal(depth.view(np.uint32), v['depth'][:3].view(np.uint32)) and np.array_equal(face, v['face'][:3])
    _, rgba = ref.attributes(verts, faces, v['K'], v['E'][:3], face, None, np.repeat(per_face, 3, axis=0))
    assert np.array_equal(rgba[..., :3], per_face[face][..., :3]) and (rgba[..., 3] == 255).all()


# ---- the entry points refuse bad arguments before any HIP call -------------------------------------------------------------
K0 = np.array([[4.0, 0.0, 2.0], [0.0, 4.0, 2.0], [0.0, 0.0, 1.0]])
E0 = np.eye(4)[:3]


class _Args:
    """Complete, valid argument lists with fake (never dereferenced) device pointers; keyword overrides replace entries."""

    def __init__(self):
        self.K = np.ascontiguousarray(np.stack([K0.reshape(9)] * 2))
        self.E = np.ascontiguousarray(np.stack([E0.reshape(12)] * 2))
        self.p = 0x1000

    def _call(self, name, a, kw):
        assert set(kw) <= set(a), kw
        a.update(kw)
        lib = _lib.load()
        rc = getattr(lib, name)(*a.values(), None)
        return rc, lib.ojf_last_error().decode()

    def raster(self, **kw):
        a = dict(vertices=self.p, nv=10, faces=self.p, nf=6, n=2, K=self.K.ctypes.data, E=self.E.ctypes.data, h=4, w=4, near=0.0,
                 keys=self.p, depth=self.p, face=self.p)
        return self._call('ojf_rasterize', a, kw)

    def attr(self, **kw):
        a = dict(vertices=self.p, nv=10, faces=self.p, nf=6, n=2, K=self.K.ctypes.data, E=self.E.ctypes.data, h=4, w=4, face=self.p,
                 face_labels=self.p, vertex_rgba=self.p, labels=self.p, rgba=self.p)
        return self._call('ojf_rasterize_attributes', a, kw)


def _refused(result, prefix, word):
    rc, msg = result
    assert rc != 0 and msg.startswith(prefix + ':') and word in msg, (rc, msg)


def _refuses_what_both_take(call, who):
    for key in ('vertices', 'faces', 'K', 'E'):
        _refused(call(**{key: None}), who, 'null')
    _refused(call(n=0), who, 'views')
    _refused(call(n=_lib.RASTER_MAX_VIEWS + 1), who, 'views')
    for key in ('nv', 'nf'):
        _refused(call(**{key: 0}), who, 'mesh size')
        _refused(call(**{key: -4}), who, 'mesh size')
    _refused(call(nf=(1 << 31) // 3 + 1), who, 'too large')
    _refused(call(h=0), who, 'image size')
    _refused(call(w=-3), who, 'image size')
    _refused(call(h=1 << 15, w=1 << 15), who, 'too large')  # n·h·w = 2^31
    for idx, v in ((1, 0.1), (3, 1e-3), (6, 1.0), (7, -2.0), (8, 2.0)):
        bad = _Args()
        bad.K[1, idx] = v  # (the second view's matrix: every view is checked)
        _refused(getattr(bad, call.__name__)(), who, 'pinhole')
    for idx in (0, 4):
        bad = _Args()
        bad.K[1, idx] = 0.0
        _refused(getattr(bad, call.__name__)(), who, 'fx and fy')
    for name, idx in (('K', 4), ('E', 19)):
        for v in (float('nan'), float('inf')):
            bad = _Args()
            getattr(bad, name).reshape(-1)[idx] = v
            _refused(getattr(bad, call.__name__)(), who, 'non-finite')
    _refused(call(vertices=0x1002), who, 'aligned')


def test_rasterize_refuses_bad_arguments_without_a_device():
    a = _Args()
    who = 'ojf_rasterize'
    assert _lib.RASTER_MAX_VIEWS == 32
    _refuses_what_both_take(a.raster, who)
    for key in ('keys', 'depth', 'face'):
        _refused(a.raster(**{key: None}), who, 'null')
    for v in (-0.01, float('nan'), float('inf')):
        _refused(a.raster(near=v), who, 'near')
    _refused(a.raster(keys=a.p + 4), who, 'aligned')
    _refused(a.raster(depth=a.p + 2), who, 'aligned')


def test_rasterize_attributes_refuses_bad_arguments_without_a_device():
    a = _Args()
    who = 'ojf_rasterize_attributes'
    _refuses_what_both_take(a.attr, who)
    _refused(a.attr(face=None), who, 'null')
    _refused(a.attr(face_labels=None, vertex_rgba=None, labels=None, rgba=None), who, 'nothing to do')
    _refused(a.attr(face_labels=None), who, 'both set or both NULL')
    _refused(a.attr(labels=None), who, 'both set or both NULL')
    _refused(a.attr(vertex_rgba=None), who, 'both set or both NULL')
    _refused(a.attr(rgba=None), who, 'both set or both NULL')
    _refused(a.attr(rgba=a.p + 1), who, 'aligned')
    _refused(a.attr(face=a.p + 2), who, 'aligned')


# ---- PLY: an optional per-face label -----------------------------------------------------------------------------------------
def test_ply_round_trip_with_face_labels(tmp_path):
    m = ref.room_mesh()
    path = str(tmp_path / 'room.ply')
    mesh.save_ply(path, m['vertices'], m['faces'], rgba=m['vertex_colors'], face_labels=m['face_labels'])
    got = mesh.load_ply(path)
    assert np.array_equal(got['vertices'], m['vertices']) and np.array_equal(got['faces'], m['faces'])
    assert np.array_equal(got['rgba'], m['vertex_colors']) and got['normals'] is None
    assert got['face_labels'].dtype == np.uint8 and np.array_equal(got['face_labels'], m['face_labels'])
    assert b'property uchar label\nend_header\n' in open(path, 'rb').read()


def test_ply_without_face_labels_is_unchanged(tmp_path):
    """The bytes of a file without labels, written out here the way the writer always made them."""
    m = ref.room_mesh()
    normals = np.random.default_rng(1).standard_normal(m['vertices'].shape).astype(np.float32)
    for with_normals, with_rgba in ((False, False), (True, False), (True, True)):
        path = str(tmp_path / 'plain.ply')
        mesh.save_ply(path, m['vertices'], m['faces'], normals if with_normals else None, m['vertex_colors'] if with_rgba else None)
        header = ['ply', 'format binary_little_endian 1.0', 'comment ojf_mesh (marching tetrahedra)', 'element vertex 32',
                  'property float x', 'property float y', 'property float z']
        header += ['property float nx', 'property float ny', 'property float nz'] if with_normals else []
        header += ['property uchar red', 'property uchar green', 'property uchar blue', 'property uchar alpha'] if with_rgba else []
        header += ['element face 48', 'property list uchar int vertex_indices', 'end_header']
        body = b''
        for i in range(32):
            body += m['vertices'][i].astype('<f4').tobytes() + (normals[i].astype('<f4').tobytes() if with_normals else b'')
            body += m['vertex_colors'][i].tobytes() if with_rgba else b''
        for f in m['faces']:
            body += b'\x03' + f.astype('<i4').tobytes()
        assert open(path, 'rb').read() == ('\n'.join(header) + '\n').encode('ascii') + body
        got = mesh.load_ply(path)
        assert sorted(got) == ['faces', 'normals', 'rgba', 'vertices']  # no new key for a file without labels
        assert np.array_equal(got['faces'], m['faces']) and np.array_equal(got['vertices'], m['vertices'])


# ---- quality of ground-truth volumes made from rasterised views --------------------------------------------------------------
def test_ground_truth_from_the_mesh_is_as_good_as_from_the_analytic_depth():
    """The CPU ground-truth composition (raster_ref into projective_ref with carve, -trunc where no view reached) of the
    room, 20 orbit poses at 48 x 64 into 64^3, against synthetic.gt_volumes: iou and acc within 0.002 of the same fusion fed
    the analytic depth and ids of synthetic._raycast.  (The two inputs differ by at most 5e-6 m: only voxels that sit on a
    threshold can flip.)  Measured: iou 0.63736 and acc 0.69442 on both paths, 108 of 262144 voxels differ - half an orbit
    leaves much of the room unseen, and unseen voxels count as solid."""
    v = ref.room_views()
    origin, res, _ = synthetic.grid_spec(ref.ROOM_GRID)
    shape = (ref.ROOM_GRID,) * 3
    tsdf, labels, weights = ref.room_ground_truth()
    cast = [synthetic._raycast(E, v['K'], ref.ROOM_H, ref.ROOM_W) for E in v['E']]
    a_tsdf, a_labels, _ = ref.fuse_ground_truth(np.stack([c[0] for c in cast]).astype(np.float32),
                                                np.stack([c[1] for c in cast]).astype(np.uint8), v['K'], v['E'], origin, res, shape,
                                                ref.ROOM_TRUNC)
    gt, _ = synthetic.gt_volumes(ref.ROOM_GRID, ref.ROOM_TRUNC)
    ours, theirs = metrics.evaluation(tsdf, gt), metrics.evaluation(a_tsdf, gt)
    print('ground truth from the mesh: iou {:.5f} acc {:.5f}; from the analytic depth: iou {:.5f} acc {:.5f}; {} voxels differ'.format(
        ours['iou'], ours['acc'], theirs['iou'], theirs['acc'], int((tsdf != a_tsdf).sum())))
    assert abs(ours['iou'] - theirs['iou']) <= 0.002 and abs(ours['acc'] - theirs['acc']) <= 0.002
    assert (weights > 0).mean() > 0.15 and (labels[weights > 0] > 0).mean() > 0.05
    assert (np.asarray(labels) != a_labels).mean() < 0.001
