"""csrc/ojf_mesh.hip held to its restatement (mesh_ref.py) on the cases of mesh_cases.py: the ordered triangle list with
labels and keys bit for bit, the capacity cut, the block offsets the scan leaves in the workspace, welding of a list with
collapsed triangles, and ojf_points_within on flat, degenerate, lattice and odd query sets.  test_mesh_edges_host.py proves
the reference and the cases; nothing here is a tolerance."""
import numpy as np
import pytest
import torch

import mesh_cases
import mesh_ref

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the cases are read-only


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.astype(np.uint64) if a.dtype == np.int64 else a


def assert_same_list(name, what, got, want, ref):
    """got == want entry for entry; on failure name the first differing slot and the (cell, tetrahedron) it belongs to."""
    shown = (got, want)
    got, want = bits(got), bits(want)
    if got.shape == want.shape and np.array_equal(got, want):
        return
    n = min(got.shape[0], want.shape[0])
    bad = np.nonzero((got[:n] != want[:n]).reshape(n, int(np.prod(want.shape[1:]))).any(axis=1))[0]
    slot = int(bad[0]) if bad.size else n
    where = 'past the shorter list' if slot >= ref.cell.shape[0] else 'cell %s, tetrahedron %d' % (tuple(int(v) for v in ref.cell[slot]), ref.tet[slot])
    pytest.fail('%s: %s has %d entries, the reference %d; %d slots differ, the first is %d (%s): got %s, want %s' % (
        name, what, got.shape[0], want.shape[0], bad.size, slot, where,
        shown[0][slot].tolist() if slot < got.shape[0] else None, shown[1][slot].tolist() if slot < want.shape[0] else None))


def extract(c, weights=True, ids=True, keys=True):
    from online_joint_depthfusion_and_semantic_amd import mesh
    out = mesh.extract_triangles(dev(c.vol), dev(c.weights) if weights else None, dev(c.ids) if ids else None, iso=c.iso,
                                 origin=c.origin, resolution=c.res, keys=keys)
    return [None if t is None else t.cpu().numpy() for t in out]


@pytest.mark.parametrize('name', mesh_cases.ALL_NAMES)
def test_triangle_list_equals_reference(name):
    from online_joint_depthfusion_and_semantic_amd import _lib
    c, ref = mesh_cases.case(name), mesh_cases.reference(name)
    gz, gy, gx = mesh_ref.blocks(c.vol.shape)
    assert _lib.load().ojf_mesh_workspace_bytes(*c.vol.shape) == 4 * gz * gy * gx
    tri, labels, keys = extract(c)
    assert_same_list(name, 'tri', tri, ref.tri, ref)
    assert_same_list(name, 'labels', labels, ref.labels, ref)
    assert_same_list(name, 'keys', keys, ref.keys, ref)
    tri, labels, keys = extract(c, ids=False)
    assert labels is None
    assert_same_list(name, 'tri without ids', tri, ref.tri, ref)
    assert_same_list(name, 'keys without ids', keys, ref.keys, ref)
    tri, labels = extract(c, keys=False)
    assert_same_list(name, 'tri without keys', tri, ref.tri, ref)
    assert_same_list(name, 'labels without keys', labels, ref.labels, ref)


@pytest.mark.parametrize('name', mesh_cases.ALL_NAMES)
def test_triangle_list_without_weights_equals_reference(name):
    c, ref = mesh_cases.case(name), mesh_cases.reference(name, weights=False)
    tri, labels, keys = extract(c, weights=False)
    assert_same_list(name, 'tri', tri, ref.tri, ref)
    assert_same_list(name, 'labels', labels, ref.labels, ref)
    assert_same_list(name, 'keys', keys, ref.keys, ref)


class Abi:
    """ojf_mesh_extract through the C ABI on one case, with buffers of the caller's choosing."""

    def __init__(self, c):
        from online_joint_depthfusion_and_semantic_amd import _lib
        self.lib, self.c = _lib.load(), c
        self.vol, self.wgt, self.ids = dev(c.vol), dev(c.weights), dev(c.ids)
        self.org = np.ascontiguousarray(np.asarray(c.origin, dtype=np.float64))
        self.wsb = self.lib.ojf_mesh_workspace_bytes(*c.vol.shape)
        self.ws = torch.full((self.wsb // 4,), -1, dtype=torch.int32, device='cuda')
        self.count = torch.zeros(1, dtype=torch.int32, device='cuda')
        self.stream = _lib.stream_ptr(self.vol.device)

    def run(self, tri, labels, keys, cap):
        X, Y, Z = self.c.vol.shape
        ptr = lambda t: None if t is None else t.data_ptr()
        rc = self.lib.ojf_mesh_extract(self.vol.data_ptr(), self.wgt.data_ptr(), self.ids.data_ptr(), X, Y, Z, float(self.c.iso),
                                       self.org.ctypes.data, float(self.c.res), self.ws.data_ptr(), self.wsb, ptr(tri), ptr(labels),
                                       ptr(keys), cap, self.count.data_ptr(), self.stream)
        assert rc == 0, self.lib.ojf_last_error()
        return int(self.count.item())


@pytest.mark.parametrize('name', ['tile_66', 'scan_1025'])
def test_capacity_cuts_the_list_anywhere(name):
    c, ref = mesh_cases.case(name), mesh_cases.reference(name)
    T = ref.tri.shape[0]
    second = np.nonzero((ref.cell[1:] == ref.cell[:-1]).all(axis=1) & (ref.tet[1:] == ref.tet[:-1]))[0] + 1
    in_quad = int(second[second.size // 2])            # the slot of the second triangle of a two-against-two tetrahedron
    offsets = np.concatenate([[0], np.cumsum(ref.counts)[:-1]])
    full = np.nonzero((ref.counts > 0) & (offsets > 0))[0]
    block_start = int(offsets[full[full.size // 2]])   # the first slot of a block in the middle of the list
    assert 0 < in_quad < T and 0 < block_start < T and ref.tet[in_quad] == ref.tet[in_quad - 1]
    abi = Abi(c)
    for cap in (in_quad, block_start, T - 1, T, T + 7):
        tri = torch.full((cap + 64, 3, 3), -777.0, device='cuda')
        labels = torch.full((cap + 64, 3), 9, dtype=torch.uint8, device='cuda')
        keys = torch.full((cap + 64, 3), -5, dtype=torch.int64, device='cuda')
        assert abi.run(tri, labels, keys, cap) == T, cap
        n = min(cap, T)
        assert_same_list('%s capacity %d' % (name, cap), 'tri', tri[:n].cpu().numpy(), ref.tri[:n], ref)
        assert_same_list('%s capacity %d' % (name, cap), 'labels', labels[:n].cpu().numpy(), ref.labels[:n], ref)
        assert_same_list('%s capacity %d' % (name, cap), 'keys', keys[:n].cpu().numpy(), ref.keys[:n], ref)
        assert (tri[n:] == -777.0).all() and (labels[n:] == 9).all() and (keys[n:] == -5).all(), cap  # nothing past the cut


@pytest.mark.parametrize('name', ['scan_1023', 'scan_1024', 'scan_1025', 'scan_2049'])
def test_workspace_holds_the_block_offsets(name):
    """The scan on its own: after a capacity-0 call the workspace is the exclusive prefix of the per-block counts."""
    c, ref = mesh_cases.case(name), mesh_cases.reference(name)
    abi = Abi(c)
    assert abi.run(None, None, None, 0) == ref.tri.shape[0]
    want = np.concatenate([[0], np.cumsum(ref.counts)[:-1]])
    got = abi.ws.cpu().numpy().astype(np.int64)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, '%s: %d block offsets differ, the first at block %d: got %d, want %d' % (
        name, bad.size, bad[0], got[bad[0]], want[bad[0]])


def test_weld_of_a_list_with_collapsed_triangles():
    from online_joint_depthfusion_and_semantic_amd import mesh
    c, ref = mesh_cases.case('on_iso'), mesh_cases.reference('on_iso')
    tri, labels, keys = mesh.extract_triangles(dev(c.vol), dev(c.weights), dev(c.ids), c.iso, c.origin, c.res, keys=True)
    assert_same_list('on_iso', 'tri', tri.cpu().numpy(), ref.tri, ref)
    va, fa, la = mesh.weld(tri, labels, keys)
    vb, fb, lb = mesh.weld(tri, labels, keys, n_voxels=c.vol.size)
    assert torch.equal(va, vb) and torch.equal(fa, fb) and torch.equal(la, lb)  # the two key paths: one mesh
    assert va.shape[0] == np.unique(ref.keys).size and fa.shape[0] == ref.tri.shape[0]
    assert np.array_equal(va[fa].cpu().numpy(), ref.tri) and np.array_equal(la[fa].cpu().numpy(), ref.labels)
    # by position: vertices that coincide on a grid point merge across keys, and exactly the faces with two equal corners go
    t = ref.tri
    collapsed = (t[:, 0] == t[:, 1]).all(axis=1) | (t[:, 1] == t[:, 2]).all(axis=1) | (t[:, 0] == t[:, 2]).all(axis=1)
    assert 0 < collapsed.sum() < collapsed.size
    vp, fp, _ = mesh.weld(tri)
    assert vp.shape[0] == np.unique(t.reshape(-1, 3), axis=0).shape[0] < va.shape[0]
    assert fp.shape[0] == int((~collapsed).sum()) and np.array_equal(vp[fp].cpu().numpy(), t[~collapsed])
    m = mesh.extract_mesh(dev(c.vol), dev(c.weights), dev(c.ids), c.iso, c.origin, c.res)
    assert np.array_equal(m['vertices'], va.cpu().numpy()) and np.isfinite(m['normals']).all()


@pytest.mark.parametrize('group', ['a', 'b', 'c', 'd', 'e'])
def test_points_within_equals_brute_force(group):
    from online_joint_depthfusion_and_semantic_amd import mesh
    for s in mesh_cases.point_sets():
        if s.group != group:
            continue
        lo = s.points.min(axis=0)
        cell, G = mesh.bin_grid(lo.tolist(), (s.points.max(axis=0) - lo).tolist(), s.tau)
        assert G[0] * G[1] * G[2] <= mesh.MAX_BINS, s.name
        count, hit = mesh.points_within(dev(s.query), dev(s.points), s.tau)
        want = mesh_ref.within(s.query, s.points, s.tau)
        if s.expect is not None:
            assert (want == s.expect).all(), s.name
        got = hit.cpu().numpy().astype(bool)
        assert np.array_equal(got, want), '%s: %d queries differ, the first is %d' % (
            s.name, (got != want).sum(), np.nonzero(got != want)[0][0])
        assert count == int(want.sum()), s.name
