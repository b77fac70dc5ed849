"""-m gpu: the registration (ojf_register_select / ojf_register / ojf_register_associate, registration.py,
Database.register) against its numpy restatement (register_ref.py): the selected list, J, r and the reason codes bit for bit,
the fp64 sums to 1e-12·sum|terms| and the solved pose to 1e-12 (ojf_track's rule), the chain of steps and stages, the whole
call on the synthetic room, and Database.register followed by Database.merge."""
import numpy as np
import pytest
import torch

from online_joint_depthfusion_and_semantic_amd import _lib, registration, resample
from online_joint_depthfusion_and_semantic_amd.config import default_config, database_config
from online_joint_depthfusion_and_semantic_amd.database import Database, Voxelgrid
import register_ref as rr
import track_ref

pytestmark = pytest.mark.gpu
f32, H = np.float32, np.float16


def _put(a, dev):
    """A device copy of ``a`` one element past the start of its buffer: naturally aligned, off the 256-byte grid."""
    a = np.ascontiguousarray(a).reshape(-1)
    flat = torch.from_numpy(a.view({H: np.int16, np.uint32: np.int32}.get(a.dtype.type, a.dtype)))
    buf = torch.empty(flat.numel() + 1, dtype=flat.dtype, device=dev)
    buf[1:].copy_(flat)
    return buf[1:]


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    view = {4: np.uint32, 1: np.uint8, 8: np.uint64, 2: np.uint16}[got.dtype.itemsize]
    bad = np.flatnonzero(got.reshape(-1).view(view) != want.reshape(-1).view(view))
    assert len(bad) == 0, '%s: %d of %d differ, first at %d: %r != %r' % (what, len(bad), got.size, bad[0], got.reshape(-1)[bad[0]],
                                                                         want.reshape(-1)[bad[0]])


class Scene:
    """The arguments of ojf_register / ojf_register_associate that describe the two volumes, with their device copies."""

    def __init__(self, dev, moving, fixed):
        self.dev, self.moving, self.fixed = dev, moving, fixed
        self.mt = _put(moving['tsdf'], dev)
        self.mo, self.fo = np.ascontiguousarray(moving['origin'], np.float64), np.ascontiguousarray(fixed['origin'], np.float64)
        self.tsdf_form = 'field' not in fixed
        if self.tsdf_form:
            self.ft, self.fw, self.field = _put(fixed['tsdf'], dev), _put(fixed['weights'], dev), None
            self.target, self.fshape = (fixed['tsdf'], fixed['weights']), fixed['tsdf'].shape
        else:
            self.ft, self.fw, self.field = None, None, _put(fixed['field'], dev)
            self.target, self.fshape = fixed['field'], fixed['field'].shape

    def args(self, lst, n):
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        return (p(self.mt), *self.moving['tsdf'].shape, self.mo.ctypes.data, float(self.moving['resolution']), p(lst), n, p(self.ft),
                p(self.fw), p(self.field), *self.fshape, self.fo.ctypes.data, float(self.fixed['resolution']))

    def ref(self, pts, pose, field_band, dist):
        return rr.associate(self.moving['tsdf'], self.mo, self.moving['resolution'], pts, self.target, self.fo, self.fixed['resolution'],
                            pose, field_band, dist)


def _workspace(n, dev):
    nbytes = int(_lib.load().ojf_register_workspace_bytes(n))
    assert nbytes > 0
    buf = torch.empty(nbytes + 8, dtype=torch.uint8, device=dev)
    return buf[8:], nbytes


def gpu_associate(sc, pts, pose, field_band, dist, frac=0.05):
    lib, dev, n = _lib.load(), sc.dev, len(pts)
    lst = _put(np.asarray(pts, np.uint32), dev)
    ws, nbytes = _workspace(n, dev)
    out = torch.zeros(1 + 12 + 29, dtype=torch.float64, device=dev)[1:]
    jr = torch.full((n * 7 + 1,), 7.0, dtype=torch.float32, device=dev)[1:]
    reason = torch.full((n + 1,), 99, dtype=torch.uint8, device=dev)[1:]
    status = torch.full((3,), 77, dtype=torch.int32, device=dev)[1:]
    E = np.ascontiguousarray(np.asarray(pose, np.float64).reshape(12))
    rc = lib.ojf_register_associate(*sc.args(lst, n), float(field_band), float(dist), frac, E.ctypes.data, ws.data_ptr(), nbytes,
                                    out.data_ptr(), out.data_ptr() + 96, jr.data_ptr(), reason.data_ptr(), status.data_ptr(),
                                    _lib.stream_ptr(dev))
    _lib.check(rc, 'ojf_register_associate')
    host = out.cpu().numpy()
    jrh = jr.cpu().numpy().reshape(n, 7)
    return dict(pose=host[:12].reshape(3, 4), sums=host[12:], J=jrh[:, :6], r=jrh[:, 6], reason=reason.cpu().numpy(),
                status=tuple(status.cpu().numpy().tolist()))


def check_associate(sc, pts, pose, field_band, dist, frac=0.05):
    """One device step against the restatement: bits of J, r, reason; sums and pose by track's rule.  Returns the device's."""
    got = gpu_associate(sc, pts, pose, field_band, dist, frac)
    J, r, reason = sc.ref(pts, pose, field_band, dist)
    _same_bits(got['reason'], reason, 'reason')
    _same_bits(got['J'], J, 'J')
    _same_bits(got['r'], r, 'r')
    terms = rr.point_terms(J, r, reason)
    want = rr.kernel_sums(terms)
    assert (np.abs(got['sums'] - want) <= 1e-12 * np.abs(terms).sum(axis=0)).all(), (got['sums'], want)
    code, P = track_ref.step(got['sums'], pose, frac * len(pts))
    assert got['status'] == ((code, 0) if code else (0, -1))
    assert np.abs(got['pose'] - P).max() <= 1e-12
    if code:
        _same_bits(got['pose'], np.asarray(pose, np.float64).reshape(3, 4), 'the pose after a failed step')
    got['code'] = code
    return got


def gpu_select(t, w, band, stride, dev, capacity=None):
    lib = _lib.load()
    td, wd = _put(t, dev), _put(w, dev)
    ws, nbytes = _workspace(t.size, dev)
    cap = t.size if capacity is None else capacity
    lst = torch.full((cap + 2,), -5, dtype=torch.int32, device=dev)
    count = torch.zeros(2, dtype=torch.int32, device=dev)
    for out in (None, lst[1:]):  # count only, then fill
        rc = lib.ojf_register_select(td.data_ptr(), wd.data_ptr(), *t.shape, float(band), stride, ws.data_ptr(), nbytes,
                                     None if out is None else out.data_ptr(), 0 if out is None else cap, count[1:].data_ptr(),
                                     _lib.stream_ptr(dev))
        _lib.check(rc, 'ojf_register_select')
        if out is None:
            first = int(count.cpu()[1])
    n = int(count.cpu()[1])
    assert n == first
    host = lst.cpu().numpy()
    assert host[0] == -5 and (host[1 + min(n, cap):] == -5).all()  # nothing outside the list, nothing past the capacity
    return n, host[1:1 + min(n, cap)].view(np.uint32)


# ---- the edge scene: moving (11,15,21), fixed (13,9,17), distinct origins and resolutions ------------------------------------
def edge_volume(shape, seed, unobserved=0.1):
    rng = np.random.default_rng(seed)
    t = rng.uniform(-0.3, 0.3, shape).astype(H)
    w = (rng.random(shape) >= unobserved).astype(H) * rng.integers(1, 9, shape).astype(H)
    ft, fw = t.reshape(-1), w.reshape(-1)
    at = rng.choice(t.size, 40, replace=False)
    ft[at[0:5]], ft[at[5:10]], ft[at[10:15]], ft[at[15:20]] = np.nan, np.inf, -np.inf, H(-0.0)
    fw[at[0:20]] = 1
    fw[at[20:25]] = H(6e-8)   # the smallest subnormal: observed
    fw[at[25:30]] = H(-1.0)
    fw[at[30:35]] = np.nan    # NaN > 0 is false: unobserved
    ft[at[35:40]], fw[at[35:40]] = H(0.1), 1  # |T| == band of the selection tests
    return t, w


def edge_scene(dev, form):
    mt, mw = edge_volume((11, 15, 21), 1)
    moving = dict(tsdf=mt, weights=mw, origin=np.array([-0.31, 0.07, -0.52]), resolution=0.043)
    fixed = dict(origin=np.array([-0.35, -0.02, -0.50]), resolution=0.051)
    if form == 'tsdf':
        fixed['tsdf'], fixed['weights'] = edge_volume((13, 9, 17), 2, unobserved=0.03)
    else:
        rng = np.random.default_rng(3)
        f = rng.uniform(-0.3, 0.3, (13, 9, 17)).astype(f32)
        flat = f.reshape(-1)
        at = rng.choice(f.size, 40, replace=False)
        flat[at[:10]], flat[at[10:20]], flat[at[20:30]], flat[at[30:40]] = np.nan, np.inf, -np.inf, f32(-0.0)
        fixed['field'] = f
    return Scene(dev, moving, fixed)


EDGE_POSE = np.concatenate([rr.axis_angle((1, -1, 2), 7.0), np.array([[0.012], [-0.021], [0.017]])], axis=1)


@pytest.mark.parametrize('stride', [1, 2, 3])
def test_selection_is_the_restatement(cuda, stride):
    t, w = edge_volume((11, 15, 21), 1)
    band = float(H(0.1))
    want = rr.select(t, w, band, stride)
    n, got = gpu_select(t, w, band, stride, cuda)
    assert n == len(want) > 0
    _same_bits(got, want, 'list')
    n2, head = gpu_select(t, w, band, stride, cuda, capacity=5)  # a short list: the count is the whole count
    assert n2 == n
    _same_bits(head, want[:5], 'list head')
    pts = registration.select_points(torch.from_numpy(t).to(cuda), torch.from_numpy(w).to(cuda), band, stride)
    assert pts.dtype == torch.int32 and pts.is_cuda
    _same_bits(pts.cpu().numpy().view(np.uint32), want, 'select_points')


def test_selection_across_blocks_and_an_empty_selection(cuda):
    rng = np.random.default_rng(8)
    shape = (9, 17, 29)  # 4437 voxels: five blocks of 1024, the last one short
    t = rng.uniform(-0.2, 0.2, shape).astype(H)
    w = (rng.random(shape) < 0.7).astype(H)
    for band, stride in ((0.15, 1), (0.15, 2)):
        want = rr.select(t, w, band, stride)
        n, got = gpu_select(t, w, band, stride, cuda)
        assert n == len(want)
        _same_bits(got, want, 'list')
    n, got = gpu_select(t, np.zeros(shape, H), 0.15, 1, cuda)
    assert n == 0 and len(got) == 0


@pytest.mark.parametrize('form', ['tsdf', 'field'])
def test_association_is_the_restatement(cuda, form):
    sc = edge_scene(cuda, form)
    pts = rr.select(sc.moving['tsdf'], sc.moving['weights'], 0.29, 1)
    assert len(pts) > 2048
    band = 0.25 if form == 'tsdf' else np.inf
    got = check_associate(sc, pts, EDGE_POSE, band, 0.2)
    counts = np.bincount(got['reason'], minlength=6)
    want = [0, 1, 2, 4] + ([3] if form == 'tsdf' else [])
    assert all(counts[c] > 0 for c in want), dict(zip(rr.REASONS, counts.tolist()))
    # an index that is no voxel of the moving volume is reason 1, not a read
    odd = np.concatenate([pts[:10], np.array([sc.moving['tsdf'].size, 2 ** 32 - 1], np.uint32)])
    got = check_associate(sc, odd, EDGE_POSE, band, 0.2)
    assert got['reason'][-2:].tolist() == [1, 1]


@pytest.mark.parametrize('form', ['tsdf', 'field'])
@pytest.mark.parametrize('n', [1, 255, 256, 257, 1023, 1024, 1025])
def test_list_sizes_around_the_wave_and_block_edges(cuda, form, n):
    sc = edge_scene(cuda, form)
    pts = rr.select(sc.moving['tsdf'], sc.moving['weights'], 0.29, 1)[100:100 + n]
    check_associate(sc, pts, EDGE_POSE, 0.25 if form == 'tsdf' else np.inf, 0.2)


@pytest.mark.parametrize('form', ['tsdf', 'field'])
def test_points_on_the_faces_of_the_fixed_grid(cuda, form):
    """Dyadic origins and resolutions make g exact: under the identity moving voxel i sits at g = i/2, so that whole moving
    voxels land on g = 0 and on g = N - 1 exactly; a translation of one fp32 ulp puts the first ones just outside."""
    rng = np.random.default_rng(4)
    mshape, fshape = (12, 10, 16), (6, 5, 8)
    mt = rng.uniform(-0.1, 0.1, mshape).astype(H)
    moving = dict(tsdf=mt, weights=np.ones(mshape, H), origin=np.array([0.0625, 0.0625, 0.0625]), resolution=0.125)
    fixed = dict(origin=np.zeros(3), resolution=0.25)
    if form == 'tsdf':
        fixed['tsdf'], fixed['weights'] = rng.uniform(-0.1, 0.1, fshape).astype(H), np.ones(fshape, H)
    else:
        fixed['field'] = rng.uniform(-0.1, 0.1, fshape).astype(f32)
    sc = Scene(cuda, moving, fixed)
    pts = np.arange(mt.size, dtype=np.uint32)
    # x = (i + 0.5)/8 + 1/16, g = 4x - 0.5 = i/2: even i on whole g, i = 0 on g = 0, i = 2(N-1) on g = N - 1
    I = np.eye(4)[:3]
    got = check_associate(sc, pts, I, np.inf, 1.0)
    reason = got['reason'].reshape(mshape)
    assert reason[0, 0, 0] != 1 and reason[9, 7, 13] != 1  # g = 0, and the last whole cell
    assert (reason[10:, :, :] == 1).all() and (reason[:, 8:, :] == 1).all() and (reason[:, :, 14:] == 1).all()  # g >= N - 1
    assert (reason[:10, :8, :14] != 1).all()
    for axis in range(3):
        P = I.copy()
        P[axis, 3] = -2.0 ** -27  # q = 0.125 - 2^-27 is the float just below 0.125 at i = 0: g = -2^-25
        r2 = check_associate(sc, pts, P, np.inf, 1.0)['reason'].reshape(mshape)
        assert (np.take(r2, 0, axis=axis) == 1).all() and (np.take(r2, 1, axis=axis)[:4, :4] != 1).all()
    bad = I.copy()
    bad[0, 3] = 1e38  # q is finite, g = 4e38 is not
    assert (check_associate(sc, pts, bad, np.inf, 1.0)['reason'] == 1).all()


@pytest.mark.parametrize('form', ['tsdf', 'field'])
def test_thresholds_met_exactly_and_a_constant_field(cuda, form):
    """A constant field: F = c exactly and the gradient is 0, so a point that passes the two thresholds ends as reason 5.
    |F| == field_band is saturated (3); |r| == dist is still an inlier of the threshold (<=)."""
    shape = (6, 7, 9)
    c = float(H(0.0625))
    rng = np.random.default_rng(6)
    mt = rng.choice(np.array([0.0, 0.03125, -0.03125, 0.09375, 0.1875], H), shape)
    moving = dict(tsdf=mt, weights=np.ones(shape, H), origin=np.array([0.01, 0.02, 0.03]), resolution=0.05)
    fixed = dict(origin=np.array([-0.05, -0.05, -0.05]), resolution=0.05)
    if form == 'tsdf':
        fixed['tsdf'], fixed['weights'] = np.full((9, 9, 12), c, H), np.ones((9, 9, 12), H)
    else:
        fixed['field'] = np.full((9, 9, 12), c, f32)
    sc = Scene(cuda, moving, fixed)
    pts = np.arange(mt.size, dtype=np.uint32)
    I = np.eye(4)[:3]
    got = check_associate(sc, pts, I, c, 1.0)
    assert (got['reason'] == 3).all()  # |F| == field_band
    above = float(np.nextafter(f32(c), f32(1)))
    # r = c - a_T in {0.0625, 0.03125, 0.09375, -0.03125, -0.125}; dist = 0.09375 is met exactly by a_T = -0.03125
    got = check_associate(sc, pts, I, above, 0.09375)
    flat = mt.reshape(-1).astype(f32)
    assert (got['reason'][flat == f32(0.1875)] == 4).all() and (got['reason'][flat != f32(0.1875)] == 5).all()
    assert (flat == f32(-0.03125)).any() and got['code'] == 1 and got['sums'][28] == 0.0
    got = check_associate(sc, pts, I, above, float(np.nextafter(f32(0.09375), f32(0))))
    assert (got['reason'][flat == f32(-0.03125)] == 4).all()


def ball_scene(dev, form, mshape=(41, 41, 41)):
    """A moving volume wholly inside the band (a shallow ball field) over a fixed one that holds the same ball: every voxel is a
    point and nearly every point an inlier."""
    def ball(shape, origin, res, centre):
        ax = [origin[a] + (np.arange(shape[a]) + 0.5) * res for a in range(3)]
        p = np.stack(np.meshgrid(*ax, indexing='ij'), axis=-1)
        return (0.05 * (np.linalg.norm((p - centre) * np.array([1.0, 1.3, 0.8]), axis=-1) - 0.9)).astype(f32)
    res = 0.05
    mo = -0.5 * res * np.array(mshape)
    fshape = tuple(n + 6 for n in mshape)
    fo = -0.5 * res * np.array(fshape) + np.array([0.004, -0.003, 0.002])
    centre = np.array([0.07, -0.05, 0.03])
    mt = ball(mshape, mo, res, centre).astype(H)
    assert np.abs(mt.astype(f32)).max() < 0.09
    moving = dict(tsdf=mt, weights=np.ones(mshape, H), origin=mo, resolution=res)
    fixed = dict(origin=fo, resolution=res)
    if form == 'tsdf':
        fixed['tsdf'], fixed['weights'] = ball(fshape, fo, res, centre).astype(H), np.ones(fshape, H)
    else:
        fixed['field'] = ball(fshape, fo, res, centre)
    return Scene(dev, moving, fixed)


BALL_POSE = np.concatenate([rr.axis_angle((2, 1, -1), 1.5), np.array([[0.004], [0.003], [-0.005]])], axis=1)


@pytest.mark.parametrize('form', ['tsdf', 'field'])
def test_64_and_65_block_rows(cuda, form):
    """The solve reads the block rows in chunks of 64: 65536 points are 64 rows, 65537 are 65."""
    sc = ball_scene(cuda, form)
    n, pts = gpu_select(sc.moving['tsdf'], sc.moving['weights'], 0.09, 1, cuda)
    assert n == 41 ** 3 and (pts == np.arange(n, dtype=np.uint32)).all()
    for count in (65536, 65537):
        got = check_associate(sc, pts[:count], BALL_POSE, 0.09 if form == 'tsdf' else np.inf, 0.05)
        assert got['code'] == 0 and got['sums'][28] > 0.9 * count


def gpu_register(sc, lst, n, iterations, E_init, field_band, dist, frac=0.05, first=0, cont=False, state=None, rows=None):
    """One ojf_register call; ``state``: the (pose | stats | status) buffer an earlier call left (a fresh one otherwise)."""
    lib, dev = _lib.load(), sc.dev
    rows = _lib.REGISTER_MAX_ITERATIONS if rows is None else rows
    if state is None:
        state = torch.full((12 + 4 * rows + 1,), -3.0, dtype=torch.float64, device=dev)
    ws, nbytes = _workspace(n, dev)
    E = np.ascontiguousarray(np.asarray(E_init, np.float64).reshape(12))
    rc = lib.ojf_register(*sc.args(lst, n), float(field_band), float(dist), iterations, first, frac, E.ctypes.data, int(cont),
                          ws.data_ptr(), nbytes, state.data_ptr(), state.data_ptr() + 96, state.data_ptr() + 8 * (12 + 4 * rows),
                          _lib.stream_ptr(dev))
    _lib.check(rc, 'ojf_register')
    return state


def _state(state, rows=None):
    rows = _lib.REGISTER_MAX_ITERATIONS if rows is None else rows
    host = state.cpu().numpy()
    return host[:12].reshape(3, 4).copy(), host[12:12 + 4 * rows].reshape(rows, 4).copy(), tuple(host[12 + 4 * rows:].view(np.int32).tolist())


@pytest.mark.parametrize('form', ['tsdf', 'field'])
def test_failures_freeze_the_call(cuda, form):
    sc = edge_scene(cuda, form)
    pts = rr.select(sc.moving['tsdf'], sc.moving['weights'], 0.29, 1)
    lst = _put(pts, cuda)
    band = 0.25 if form == 'tsdf' else np.inf
    # fewer inliers than the minimum: status 1 at iteration 2 of a call whose rows start at 2
    state = gpu_register(sc, lst, len(pts), 3, EDGE_POSE, band, 0.2, frac=1.0, first=2)
    P, stats, status = _state(state)
    assert status == (1, 2)
    _same_bits(P, EDGE_POSE, 'the pose after status 1')
    J, r, reason = sc.ref(pts, EDGE_POSE, band, 0.2)
    assert stats[2, 0] == (reason == 0).sum() > 0 and stats[2, 1] > 0 and (stats[2, 2:] == 0).all() and (stats[3:5] == 0).all()
    assert (stats[:2] == -3.0).all() and (stats[5:] == -3.0).all()  # only the call's own rows are written
    # a single plane: the gradient is (1, 0, 0) everywhere, the system has rank 3: status 2
    shape = (8, 8, 8)
    moving = dict(tsdf=np.zeros(shape, H), weights=np.ones(shape, H), origin=np.array([0.25, 0.25, 0.25]), resolution=0.125)
    x = (np.arange(12) * 0.125 - 0.5).astype(f32)
    fixed = dict(origin=np.zeros(3), resolution=0.125)
    if form == 'tsdf':
        fixed['tsdf'], fixed['weights'] = np.broadcast_to(x.astype(H)[:, None, None], (12, 12, 12)).copy(), np.ones((12, 12, 12), H)
    else:
        fixed['field'] = np.broadcast_to(x[:, None, None], (12, 12, 12)).copy()
    plane = Scene(cuda, moving, fixed)
    pts = np.arange(512, dtype=np.uint32)
    E0 = np.concatenate([np.eye(3), np.array([[0.03125], [0.0], [0.0]])], axis=1)
    got = check_associate(plane, pts, E0, np.inf, 1.0)
    assert got['code'] == 2 and got['sums'][28] == 512
    state = gpu_register(plane, _put(pts, cuda), 512, 3, E0, np.inf, 1.0)
    P, stats, status = _state(state)
    assert status == (2, 0)
    _same_bits(P, E0, 'the pose after status 2')
    assert stats[0, 0] == 512 and (stats[0, 2:] == 0).all() and (stats[1:3] == 0).all()
    # a later stage that continues from the frozen state does nothing but zero its rows, and restores nothing else
    state = gpu_register(plane, _put(pts, cuda), 512, 2, E0, np.inf, 1.0, first=3, cont=True, state=state)
    P2, stats2, status2 = _state(state)
    assert status2 == (2, 0) and (stats2[3:5] == 0).all()
    _same_bits(P2, E0, 'the pose of a frozen call')


# ---- a small room in two worlds: chain, whole call, Database ---------------------------------------------------------------
def small_room(dev, shape_m=(32, 32, 32), deg=8.0, half=True):
    """The 32^3 room (16 cm voxels, truncation 0.64 m) in its own world and in one turned by ``deg`` about (1,2,3); ``half``: the
    fixed scene is observed only for x < 0.8 m of its world."""
    res, trunc = 0.16, 0.64
    W = np.concatenate([rr.axis_angle((1, 2, 3), deg), np.array([[0.25], [-0.15], [0.10]])], axis=1)
    moving = rr.sampled_scene(shape_m, np.array([-2.56, -2.56, -2.56]), res, trunc)
    fshape = (38, 36, 30)
    fo = W[:, 3] - 0.5 * res * np.array(fshape) + np.array([0.03, -0.05, 0.02])
    fixed = rr.sampled_scene(fshape, fo, res, trunc, world_from_room=W, observed_if=(lambda p: p[..., 0] < 0.8) if half else None)
    return moving, fixed, W, res


def _on(scene, dev):
    return dict(tsdf=torch.from_numpy(scene['tsdf']).to(dev), weights=torch.from_numpy(scene['weights']).to(dev),
                origin=scene['origin'], resolution=scene['resolution'])


@pytest.fixture(scope='module')
def chain_case(cuda):
    moving, fixed, W, res = small_room(cuda, deg=4.0, half=False)
    field = registration.signed_distance_field(torch.from_numpy(fixed['tsdf']).to(cuda), torch.from_numpy(fixed['weights']).to(cuda),
                                               res).cpu().numpy()
    c_m, c_f = rr.condition(moving['tsdf'].shape, moving['origin'], res, np.eye(3), np.zeros(3))
    m = dict(moving, origin=moving['origin'] - c_m)
    coarse = Scene(cuda, m, dict(field=field, origin=fixed['origin'] - c_f, resolution=res))
    fine = Scene(cuda, m, dict(tsdf=fixed['tsdf'], weights=fixed['weights'], origin=fixed['origin'] - c_f, resolution=res))
    return coarse, fine, rr.select(moving['tsdf'], moving['weights'], 0.48, 1)


def test_signed_field_is_the_restatement(cuda, chain_case):
    coarse, fine, pts = chain_case
    want = rr.signed_distance_field(fine.fixed['tsdf'], fine.fixed['weights'], 0.16, edt=rr.scipy_edt)
    got = coarse.fixed['field']
    assert np.isfinite(got).all()
    _same_bits(np.abs(got), np.abs(want), '|field|')  # (the sign may differ where equally near seeds disagree: the definition names the smallest index)
    small = rr.sampled_scene((9, 8, 10), np.array([1.6, 1.5, -1.0]), 0.16, 0.64)
    got = registration.signed_distance_field(torch.from_numpy(small['tsdf']).to(cuda), torch.from_numpy(small['weights']).to(cuda), 0.16,
                                             reach=0.5).cpu().numpy()
    want = rr.signed_distance_field(small['tsdf'], small['weights'], 0.16, reach=0.5)
    assert np.isnan(want).any() and (~np.isnan(want)).any()
    _same_bits(got, want, 'field with a reach')


def test_chain_of_steps_and_stages(cuda, chain_case):
    coarse, fine, pts = chain_case
    n = len(pts)
    lst = _put(pts, cuda)
    E0 = np.eye(4)[:3]
    poses = []
    for k in range(4):  # P_k: the call cut after k steps
        P, stats, status = _state(gpu_register(coarse, lst, n, k, E0, np.inf, 0.5))
        assert status == (0, -1)
        poses.append(P)
    _same_bits(poses[0], E0, 'P_0')
    assert np.abs(poses[3] - poses[0]).max() > 1e-3
    for k in range(3):  # step k is ojf_register_associate from P_k, bit for bit, and that is the restatement's step
        got = check_associate(coarse, pts, poses[k], np.inf, 0.5)
        _same_bits(got['pose'], poses[k + 1], 'P_%d' % (k + 1))
        assert stats[k, 0] == got['sums'][28] and stats[k, 1] == got['sums'][27] / got['sums'][28]
    # a second stage continued from pose_dev equals one started from the copied-back pose
    a = gpu_register(coarse, lst, n, 3, E0, np.inf, 0.5)
    a = gpu_register(fine, lst, n, 2, E0, 0.6, 0.48, first=3, cont=True, state=a)
    Pa, sa, sta = _state(a)
    b = gpu_register(fine, lst, n, 2, poses[3], 0.6, 0.48, first=3)
    Pb, sb, stb = _state(b)
    assert sta == stb == (0, -1)
    _same_bits(Pa, Pb, 'the continued stage')
    _same_bits(sa[3:5], sb[3:5], 'its stats')
    got = check_associate(fine, pts, poses[3], 0.6, 0.48)  # and its first step is the TSDF form's restatement
    assert sa[3, 0] == got['sums'][28]
    # two identical calls give identical bits
    c = gpu_register(coarse, lst, n, 3, E0, np.inf, 0.5)
    c = gpu_register(fine, lst, n, 2, E0, 0.6, 0.48, first=3, cont=True, state=c)
    _same_bits(c.cpu().numpy(), a.cpu().numpy(), 'a repeated call')


CORNERS = np.array([[x, y, z] for x in (-2.4, 2.4) for y in (-2.4, 2.4) for z in (-1.4, 1.4)])


def _whole_call(cuda, moving, fixed, truth, band, res):
    out = registration.register_volumes(_on(moving, cuda), _on(fixed, cuda), band=band)
    reach = rr.coarse_reach(registration.default_stages(band), band, res)
    assert reach == registration.coarse_reach(registration.default_stages(band), band, res)
    field = registration.signed_distance_field(torch.from_numpy(fixed['tsdf']).to(cuda), torch.from_numpy(fixed['weights']).to(cuda),
                                               float(res), reach=reach).cpu().numpy()
    ref = rr.run(moving, fixed, registration.default_stages(band), band=band, field=field)
    e_dev = rr.transform_error(out['transform'], truth, CORNERS) / res
    e_ref = rr.transform_error(ref['transform'], truth, CORNERS) / res
    start = rr.transform_error(np.eye(4)[:3], truth, CORNERS) / res
    print('start %.3f voxels; device %.5f voxels, restatement %.5f voxels; points %s' % (start, e_dev, e_ref, out['n_points']))
    assert out['ok'] and out['status'] == 0 and ref['status'] == (0, -1)
    assert out['n_points'] == ref['n_points'] and out['stats'].shape == (20, 4)
    assert (out['stats'][:, 0] > 0).all()
    return e_dev, e_ref


def test_whole_call_on_the_half_observed_32_room(cuda):
    """Measured on the MI355X: see DESIGN.md §21."""
    moving, fixed, W, res = small_room(cuda)
    e_dev, e_ref = _whole_call(cuda, moving, fixed, W, 0.48, res)
    assert e_ref < 0.25 and e_dev <= 2.0 * e_ref


def test_whole_call_on_the_128_room(cuda):
    """The 128^3 case of test_register_host.py.  Measured on the MI355X: see DESIGN.md §21."""
    import test_register_host as host
    moving, fixed, truth = host.room_pair()
    e_dev, e_ref = _whole_call(cuda, moving, fixed, truth, host.BAND, host.RES)
    assert e_ref < 0.25 and e_dev <= 2.0 * e_ref


class TwoBoxes:
    """Two scenes of 32^3 voxels with boxes of their own."""

    def __init__(self, boxes):
        self.scenes = list(boxes)
        self.boxes = boxes

    def get_grid(self, scene, truncation, semantic_grid=True):
        b = self.boxes[scene]
        g = Voxelgrid(b['resolution'])
        shape = np.array(b['tsdf'].shape)
        g.from_array(b['tsdf'].copy(), np.stack([b['origin'], b['origin'] + shape * b['resolution']], axis=1))
        return (g,)


def test_database_register_then_merge(cuda):
    moving, fixed, W, res = small_room(cuda, half=False)
    fixed = rr.sampled_scene((32, 32, 32), W[:, 3] - 0.5 * res * 32 + np.array([0.03, -0.05, 0.02]), res, 0.64, world_from_room=W)
    cfg = default_config(48, 64, semantics=False, model='tsdf', init_value=0.64)
    cfg.SETTINGS.device = str(cuda)
    db = Database(TwoBoxes({'dst': moving, 'src': fixed}), database_config(cfg))
    for s, scene in (('dst', moving), ('src', fixed)):
        db.scenes_est[s].volume = torch.from_numpy(scene['tsdf']).to(cuda)
        db.fusion_weights[s] = torch.from_numpy(scene['weights']).to(cuda)
        db.state[s] = True
    before = db.scenes_est['dst'].volume.clone(), db.fusion_weights['dst'].clone()
    out = db.register('dst', 'src', band=0.48)
    assert out['ok'] and out['transform'].shape == (3, 4) and out['transform'].dtype == np.float64
    assert torch.equal(db.scenes_est['dst'].volume, before[0]) and torch.equal(db.fusion_weights['dst'], before[1])  # writes no volume
    e = rr.transform_error(out['transform'], W, CORNERS) / res
    assert e < 0.25
    R = out['transform'][:, :3]
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-6
    resample.compose(fixed['origin'], res, moving['origin'], res, out['transform'])  # passes compose's orthonormality check
    with pytest.raises(ValueError, match='itself'):
        db.register('dst', 'dst')

    def changed_by(transform):
        db.scenes_est['dst'].volume, db.fusion_weights['dst'] = before[0].clone(), before[1].clone()
        db.merge('dst', 'src', transform=transform)
        return ((db.fusion_weights['dst'] != before[1]) | (db.scenes_est['dst'].volume != before[0])).cpu().numpy()

    got, want = changed_by(out['transform']), changed_by(W)
    # only voxels whose image lies within the registration error of the boundary of what the source covers can differ: a layer
    # e < 0.25 voxels thick over that boundary, whose area is at most the voxels of `want` with a face neighbour outside it
    pad = np.pad(want, 1)
    inner = np.ones_like(want)
    for axis in range(3):
        for shift in (-1, 1):
            inner &= np.roll(pad, shift, axis)[1:-1, 1:-1, 1:-1]
    shell = int((want & ~inner).sum())
    differ = int((got != want).sum())
    print('register error %.5f voxels; merge changes %d voxels, %d differ from the true-transform merge (boundary %d)'
          % (e, int(want.sum()), differ, shell))
    assert want.sum() > 5000 and differ <= 0.25 * shell

    db.to_numpy()
    with pytest.raises(ValueError, match=r'to_torch\(\)'):
        db.register('dst', 'src')
