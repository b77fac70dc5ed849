"""-m gpu: the distance transform on the device (ojf_volume_edt / ojf_volume_surface_mask / ojf_volume_esdf, distance.py,
Database.esdf) against the numpy restatement (distance_ref.py).  Every comparison with the restatement is bit equality of dist2
and nearest (of the mask, of the fp32 ESDF) unless stated otherwise.  Shapes are the smallest that reach every edge of the z
pass's 64-voxel chunk and of the y and x passes' run of z (64 for lines of up to 320 voxels, shorter for longer lines)."""
import functools

import numpy as np
import pytest
import torch

from online_joint_depthfusion_and_semantic_amd import _lib, distance, synthetic
from online_joint_depthfusion_and_semantic_amd.config import default_config, database_config
from online_joint_depthfusion_and_semantic_amd.database import Database
import distance_ref as ref

pytestmark = pytest.mark.gpu

NONE = ref.NONE
T = ref.T


def _same(got, want, what):
    for name, g, w in zip(('dist2', 'nearest'), got, want):
        g, w = (a.cpu().numpy() if torch.is_tensor(a) else a for a in (g, w))
        assert g.dtype == np.int32 and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero((g != w).ravel())
        assert len(bad) == 0, (what, name, len(bad), bad[:5], g.ravel()[bad[:5]], w.ravel()[bad[:5]])


def _run(seeds, cuda, **kw):
    return distance.edt(torch.from_numpy(seeds).to(cuda), **kw)


@functools.lru_cache(maxsize=None)
def _random_case(shape, density):
    seeds = ref.random_seeds(shape, density)
    return seeds, ref.edt(seeds)


@pytest.mark.parametrize('density', [0.02, 0.3])
@pytest.mark.parametrize('shape', ref.SHAPES)
def test_shapes_and_densities(cuda, shape, density):
    seeds, want = _random_case(shape, density)
    _same(_run(seeds, cuda), want, (shape, density))


def test_corner_seeds(cuda):
    """One seed in each of the eight corners in turn, two chunks and two runs and a bit wide: the closed form."""
    shape = (2 * T + 1, 2 * T + 2, 2 * T + 3)
    x, y, z = np.indices(shape)
    for corner in range(8):
        c = [(n - 1) * ((corner >> (2 - a)) & 1) for a, n in enumerate(shape)]
        seeds = np.zeros(shape, np.uint8)
        seeds[tuple(c)] = 255
        d2, near = _run(seeds, cuda)
        want = (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2
        assert (d2.cpu().numpy() == want).all(), corner
        assert (near == (c[0] * shape[1] + c[1]) * shape[2] + c[2]).all(), corner


def test_empty_and_full(cuda):
    shape = (17, 13, 130)
    d2, near = _run(np.zeros(shape, np.uint8), cuda)
    assert (d2 == NONE).all() and (near == -1).all()
    d2, near = _run(np.zeros(shape, np.uint8), cuda, max_dist2=9)
    assert (d2 == NONE).all() and (near == -1).all()
    d2, near = _run(np.full(shape, 7, np.uint8), cuda)
    assert (d2 == 0).all() and (near.cpu().numpy().ravel() == np.arange(17 * 13 * 130)).all()


@pytest.mark.parametrize('axis', [0, 1, 2])
def test_tie_rule(cuda, axis):
    """Two seeds mirror-symmetric about a plane - along z across the chunk boundary, along y and x with the plane running over
    a boundary between two runs of z: the plane's voxels, and the whole half in front of it, name the smaller index."""
    shape = (10, 12, 2 * T + 12)
    for half in (1, 4):
        plane = T if axis == 2 else 5
        a, b = [3, 4, T - 2], [3, 4, T - 2]
        a[axis], b[axis] = plane - half, plane + half
        seeds = np.zeros(shape, np.uint8)
        seeds[tuple(a)] = seeds[tuple(b)] = 1
        d2, near = _run(seeds, cuda)
        near = near.cpu().numpy()
        ia = (a[0] * shape[1] + a[1]) * shape[2] + a[2]
        ib = (b[0] * shape[1] + b[1]) * shape[2] + b[2]
        assert ia < ib
        coord = np.indices(shape)[axis]
        assert (near[coord <= plane] == ia).all() and (near[coord > plane] == ib).all(), (axis, half)
        _same((d2, near), ref.edt(seeds), ('tie', axis, half))


def test_distance_limit(cuda):
    """Sparse seeds, so that every limit but the last masks something: each limited result is the unlimited one masked."""
    shape = (33, 65, 129)
    seeds = ref.random_seeds(shape, 0.0005)
    want = ref.edt(seeds)
    free = _run(seeds, cuda)
    _same(free, want, 'unlimited')
    assert want[0].max() > 50
    for limit in (0, 1, 2, 3, 9, 50, 2 ** 24):
        far = want[0] > limit
        assert far.any() == (limit < 2 ** 24)
        got = _run(seeds, cuda, max_dist2=limit)
        _same(got, (np.where(far, NONE, want[0]).astype(np.int32), np.where(far, -1, want[1]).astype(np.int32)), ('limit', limit))
    # in voxels: floor(R²)
    _same(_run(seeds, cuda, max_distance=1.8), _run(seeds, cuda, max_dist2=3), 'max_distance=1.8')
    _same(_run(seeds, cuda, max_distance=None), want, 'max_distance=None')


def _call(lib, seeds, shape, limit, phases, ws, d2, near, cuda, ws_bytes=None):
    return lib.ojf_volume_edt(seeds.data_ptr(), *shape, limit, phases, ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes,
                              d2.data_ptr(), near.data_ptr(), _lib.stream_ptr(cuda))


def test_phases_run_one_by_one(cuda):
    """The three phase bits as three calls equal one call, and each equals the restatement's pass."""
    lib = _lib.load()
    shape = (17, 13, 130)
    seeds_h, want = _random_case(shape, 0.02)
    seeds = torch.from_numpy(seeds_h).to(cuda)
    for limit in (-1, 9):
        ws = torch.empty(lib.ojf_volume_edt_workspace_bytes(*shape), dtype=torch.uint8, device=cuda)
        d2 = torch.full(shape, -7, dtype=torch.int32, device=cuda)
        near = torch.full(shape, -7, dtype=torch.int32, device=cuda)
        step = None
        for bit, name in ((_lib.EDT_Z, 'z'), (_lib.EDT_Y, 'y'), (_lib.EDT_X, 'x')):
            assert _call(lib, seeds, shape, limit, bit, ws, d2, near, cuda) == 0, lib.ojf_last_error()
            step = ref.edt(seeds_h, limit, phases=(name,), start=step)
            # (the index the y pass leaves is in the workspace)
            index = ws[:4 * seeds.numel()].view(torch.int32).view(shape) if name == 'y' else near
            _same((d2, index), step, ('phase', name, limit))
        once = _run(seeds_h, cuda, max_dist2=limit) if limit >= 0 else _run(seeds_h, cuda)
        _same((d2, near), (once[0].cpu().numpy(), once[1].cpu().numpy()), ('three calls', limit))
        # two bits in one call
        d2b, nearb = torch.empty_like(d2), torch.empty_like(near)
        assert _call(lib, seeds, shape, limit, _lib.EDT_Z | _lib.EDT_Y, ws, d2b, nearb, cuda) == 0
        assert _call(lib, seeds, shape, limit, _lib.EDT_X, ws, d2b, nearb, cuda) == 0
        _same((d2b, nearb), ref.edt(seeds_h, limit), ('two calls', limit))


def test_refusals_leave_the_outputs_untouched(cuda):
    lib = _lib.load()
    shape = (5, 6, 70)
    n = 5 * 6 * 70
    seeds = torch.ones(shape, dtype=torch.uint8, device=cuda)
    ws = torch.full((lib.ojf_volume_edt_workspace_bytes(*shape),), 0x5a, dtype=torch.uint8, device=cuda)
    d2 = torch.full(shape, -7, dtype=torch.int32, device=cuda)
    near = torch.full(shape, -7, dtype=torch.int32, device=cuda)
    st = _lib.stream_ptr(cuda)
    p = dict(seeds=seeds.data_ptr(), dims=shape, limit=-1, phases=_lib.EDT_ALL, ws=ws.data_ptr(), ws_bytes=ws.numel(), d2=d2.data_ptr(),
             near=near.data_ptr())
    faults = [dict(seeds=None), dict(ws=None), dict(d2=None), dict(near=None), dict(dims=(0, 6, 70)), dict(dims=(5, 6, 2049)),
              dict(dims=(2048, 2048, 2048)), dict(phases=0), dict(phases=8), dict(ws_bytes=ws.numel() - 8), dict(ws_bytes=0),
              dict(d2=d2.data_ptr() + 2)]
    for fault in faults:
        a = dict(p, **fault)
        rc = lib.ojf_volume_edt(a['seeds'], *a['dims'], a['limit'], a['phases'], a['ws'], a['ws_bytes'], a['d2'], a['near'], st)
        assert rc != 0 and lib.ojf_last_error().startswith(b'ojf_volume_edt:'), fault
    t = torch.full(shape, 0.5, dtype=torch.float16, device=cuda)
    mask = torch.full(shape, 0x5a, dtype=torch.uint8, device=cuda)
    out = torch.full(shape, -7.0, dtype=torch.float32, device=cuda)
    assert lib.ojf_volume_surface_mask(t.data_ptr(), None, *shape, mask.data_ptr(), st) != 0
    assert lib.ojf_volume_surface_mask(t.data_ptr(), t.data_ptr(), 5, 6, 4096, mask.data_ptr(), st) != 0
    assert lib.ojf_volume_surface_mask(t.data_ptr(), t.data_ptr(), 5, 0, 70, mask.data_ptr(), st) != 0
    assert lib.ojf_volume_esdf(d2.data_ptr(), t.data_ptr(), None, n, 0.02, 1.0, out.data_ptr(), st) != 0
    assert lib.ojf_volume_esdf(d2.data_ptr(), t.data_ptr(), t.data_ptr(), 0, 0.02, 1.0, out.data_ptr(), st) != 0
    assert lib.ojf_volume_esdf(d2.data_ptr(), t.data_ptr(), t.data_ptr(), n, 0.0, 1.0, out.data_ptr(), st) != 0
    assert lib.ojf_volume_esdf(d2.data_ptr(), t.data_ptr(), t.data_ptr(), n, 0.02, float('nan'), out.data_ptr(), st) != 0
    torch.cuda.synchronize(cuda)
    assert (d2 == -7).all() and (near == -7).all() and (ws == 0x5a).all() and (mask == 0x5a).all() and (out == -7.0).all()
    with pytest.raises(ValueError, match='2048'):
        distance.edt(torch.ones((1, 2049, 1), dtype=torch.uint8, device=cuda))


def test_transposed_input_gives_transposed_distances(cuda):
    """x <-> y changes every linear index and swaps the roles of the y and the x pass: the distances stay (the named seed may
    be another of the equally near ones)."""
    seeds, want = _random_case((17, 13, 130), 0.02)
    d2, near = _run(np.ascontiguousarray(seeds.transpose(1, 0, 2)), cuda)
    assert (d2.cpu().numpy().transpose(1, 0, 2) == want[0]).all()
    near = near.cpu().numpy().transpose(1, 0, 2)  # indices of the [Y,X,Z] volume
    qy, qx, qz = np.unravel_index(near.ravel(), (13, 17, 130))
    px, py, pz = (a.ravel() for a in np.indices((17, 13, 130)))
    assert (seeds[qx, qy, qz] != 0).all() and ((px - qx) ** 2 + (py - qy) ** 2 + (pz - qz) ** 2 == want[0].ravel()).all()


SPECIAL_W = np.array([1, -0.0, 0.0, np.nan, -1, np.array([1], np.uint16).view(np.float16)[0], np.inf, 2], np.float16)
SPECIAL_T = np.array([0.01, -0.03, np.nan, -np.array([1], np.uint16).view(np.float16)[0], np.array([1], np.uint16).view(np.float16)[0], -0.04, 0.0,
                      -0.0], np.float16)


@pytest.mark.parametrize('shape', [(5, 7, 40), (5, 7, 37), (1, 1, 8), (3, 1, 16), (1, 3, 16)])
def test_special_values(cuda, shape):
    """NaN, ±0, subnormal and negative weights and values: the surface mask and the ESDF against their restatements, with z rows
    of whole 16-byte groups and not, at offset 0 and at an offset that defeats the wide-load path."""
    rng = np.random.default_rng(list(shape))
    n = shape[0] * shape[1] * shape[2]
    for off in (0, 1):
        t = torch.from_numpy(SPECIAL_T[rng.integers(0, 8, n + off)]).to(cuda)[off:].view(shape)
        w = torch.from_numpy(SPECIAL_W[rng.integers(0, 8, n + off)]).to(cuda)[off:].view(shape)
        assert off == 0 or t.data_ptr() % 16 != 0
        th, wh = t.cpu().numpy(), w.cpu().numpy()
        got = distance.surface_mask(t, w).cpu().numpy()
        want = ref.surface_mask(th, wh)
        assert got.dtype == np.uint8 and (got == want).all(), (shape, off)
        assert shape[2] < 37 or 0 < want.sum() < n
        for max_distance, res in ((None, 0.02), (0.05, 0.02), (0.0, 0.5)):
            got = distance.esdf(t, w, res, max_distance).cpu().numpy()
            want_e = ref.scene_esdf(th, wh, res, max_distance)
            assert got.dtype == np.float32 and (got.view(np.uint32) == want_e.view(np.uint32)).all(), (shape, off, max_distance)


def test_morphology_and_nearest_values(cuda):
    shape = (17, 13, 130)
    mask_h, _ = _random_case(shape, 0.02)
    mask = torch.from_numpy(mask_h).to(cuda)
    for radius, r2 in ((1, 1), (1.5, 2), (1.8, 3), (3, 9), (0, 0)):
        grown = distance.dilate(mask, radius)
        assert grown.dtype == torch.uint8 and (grown.cpu().numpy() == ref.dilate(mask_h, r2)).all(), radius
        assert (distance.dilate(mask != 0, radius) == grown).all()  # a bool mask is taken as it is
        back = distance.erode(grown, radius)
        assert (back.cpu().numpy() == 1 - ref.dilate(1 - grown.cpu().numpy(), r2)).all(), radius
        assert (back.cpu().numpy() >= (mask_h != 0)).all()  # closing is extensive
    d2, near = distance.edt(mask, max_dist2=9)
    labels = torch.from_numpy(np.arange(mask_h.size, dtype=np.int64).reshape(shape) % 251).to(cuda).to(torch.uint8)
    got = distance.nearest_values(labels, near, fill=255).cpu().numpy()
    want_d2, want_near = ref.edt(mask_h, 9)
    want = np.where(want_near >= 0, (np.maximum(want_near, 0) % 251), 255).astype(np.uint8)
    assert (got == want).all() and (want == 255).any() and (want != 255).any()


# ---- fused room ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def room(cuda):
    h, w, grid, frames = 48, 64, 64, 10
    cfg = default_config(h, w, semantics=False, model='tsdf')
    cfg.SETTINGS.device = str(cuda)
    st = synthetic.SyntheticStream(h, w, grid, frames)
    db = Database(st, database_config(cfg))
    for i in range(frames):
        f = st.frame(i)
        db.integrate_depth(st.scene, f['tof_depth'], f['intrinsics'], f['extrinsics'], mask=f['mask'])
    return db, st.scene


def test_fused_room(room):
    """The synthetic room fused from 10 frames into 64³: surface mask, transform and ESDF bit for bit, unlimited and limited."""
    db, s = room
    tsdf, wgt = db.scenes_est[s].volume, db.fusion_weights[s]
    th, wh = tsdf.cpu().numpy(), wgt.cpu().numpy()
    res = float(db.resolution[s])
    surface = ref.surface_mask(th, wh)
    assert 1000 < surface.sum() < surface.size // 4
    assert (distance.surface_mask(tsdf, wgt).cpu().numpy() == surface).all()
    _same(distance.edt(torch.from_numpy(surface).to(tsdf.device)), ref.edt(surface), 'room')
    for max_distance in (None, 12 * res, 2.5 * res):
        got = distance.esdf(tsdf, wgt, res, max_distance).cpu().numpy()
        want = ref.scene_esdf(th, wh, res, max_distance)
        assert got.dtype == np.float32 and (got.view(np.uint32) == want.view(np.uint32)).all(), max_distance
        assert (got < 0).any() and (got > 0).any()
        if max_distance is not None:
            assert np.abs(got).max() == np.float32(max_distance) and (np.abs(got) == np.float32(max_distance)).sum() > 100


def test_database_esdf(room):
    """Database.esdf equals the module call, leaves every volume of the scene as it was and refuses host-resident state."""
    db, s = room

    def volumes():
        return {'tsdf': db.scenes_est[s].volume, 'weights': db.fusion_weights[s], 'gt': db.scenes_gt[s].volume}
    before = {k: v.cpu().numpy().tobytes() for k, v in volumes().items()}
    res = float(db.resolution[s])
    for max_distance in (None, 0.24):
        got = db.esdf(s, max_distance)
        want = distance.esdf(db.scenes_est[s].volume, db.fusion_weights[s], res, max_distance)
        assert got.dtype == torch.float32 and got.is_cuda and (got.view(torch.int32) == want.view(torch.int32)).all()
    for k, v in volumes().items():
        assert v.cpu().numpy().tobytes() == before[k], k
    with pytest.raises(ValueError, match='max_distance'):
        db.esdf(s, -1.0)
    db.to_numpy()
    try:
        with pytest.raises(ValueError, match='not resident'):
            db.esdf(s)
    finally:
        db.to_torch()
    assert db.scenes_est[s].volume.is_cuda and db.scenes_est[s].volume.cpu().numpy().tobytes() == before['tsdf']


# ---- analytic accuracy -----------------------------------------------------------------------------------------------------------
TRUNC = 0.06
# the written TSDF is rounded to fp16: where it sits on the wrong side of a voxel's true value the surface the kernels see has
# moved by at most the fp16 spacing at the truncation value, 2^-15 for values in [2^-5, 2^-4) (fp32 rounding of the ESDF itself,
# 2^-23 relative, is far below it)
SLACK = float(np.spacing(np.float16(TRUNC)))
assert SLACK == 2.0 ** -15


def _analytic(surface, shape, res):
    """(signed distance f64 [X,Y,Z] of the voxel centres to the surface, the surface point nearest to each [X,Y,Z,3])."""
    p = (np.stack(np.indices(shape), axis=-1).astype(np.float64) + 0.5) * res
    if surface == 'sphere':
        centre, radius = np.array([0.4731, 0.4127, 0.5519]), 0.3173
        d = np.linalg.norm(p - centre, axis=-1)
        return d - radius, centre + (p - centre) * (radius / d)[..., None]
    normal = np.array([0.3, -0.5, 0.81])
    normal /= np.linalg.norm(normal)
    true = p @ normal - 0.4312
    return true, p - true[..., None] * normal


@pytest.mark.parametrize('surface', ['sphere', 'plane'])
def test_analytic_accuracy(cuda, surface):
    """A fully observed fp16 TSDF of an analytic surface: -res <= |esdf| - true <= sqrt(3) res.  A seed has the surface within
    one voxel edge along an axis (esdf >= true - res) and the cell of the surface point nearest to a voxel has a seed at one
    of its corners (esdf <= true + sqrt(3) res) - where the volume holds that cell: a voxel whose nearest point of the plane
    lies outside the box has its nearest seed further along the plane, and only the lower bound is asked of it; the whole
    sphere is inside.  The sign is that of the written value."""
    shape, res = (48, 40, 56), 0.02
    true, foot = _analytic(surface, shape, res)
    written = np.clip(true, -TRUNC, TRUNC).astype(np.float16)
    tsdf = torch.from_numpy(written).to(cuda)
    wgt = torch.ones(shape, dtype=torch.float16, device=cuda)
    got = distance.esdf(tsdf, wgt, res).cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    err = np.abs(got) - np.abs(true)
    # the upper bound speaks of the cell of the nearest surface point: it holds where the volume has that cell
    inside = ((foot >= 0.5 * res) & (foot <= (np.array(shape) - 0.5) * res)).all(axis=-1)
    assert inside.all() if surface == 'sphere' else inside.mean() > 0.6
    print('analytic', surface, 'min', err.min() / res, 'max', err[inside].max() / res, 'voxels;', inside.mean(), 'of the voxels under the upper bound')
    assert err.min() >= -res - SLACK and err[inside].max() <= np.sqrt(3.0) * res + SLACK, (err.min() / res, err[inside].max() / res)
    assert (np.signbit(got) == (written.astype(np.float32) < 0)).all()
    assert (got < 0).any() and (got > 0).any()
