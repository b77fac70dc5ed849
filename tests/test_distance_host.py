"""CPU: the numpy restatement of the distance transform (distance_ref.py) against the brute-force minimum of the 64-bit keys
and against scipy.ndimage; the surface mask and the ESDF in fp32 on hand-made values; dilation against scipy's with the
Euclidean ball; the refusals of the Python layer and of the C ABI, none of which needs a device."""
import numpy as np
import pytest
import torch

from online_joint_depthfusion_and_semantic_amd import _lib, distance
import distance_ref as ref

NONE = ref.NONE


@pytest.mark.parametrize('density', [0.01, 0.05, 0.3])
def test_restatement_equals_brute_force_keys(density):
    """Both fields, on integer lattices where ties are abundant: the separable passes with ties towards the smaller source
    coordinate give the smallest linear index among the nearest seeds."""
    rng = np.random.default_rng(int(100 * density))
    ties = 0
    for trial in range(27):
        shape = tuple(int(n) for n in rng.integers(1, (10, 9, 12)))
        seeds = ref.random_seeds(shape, density, seed=trial)
        limit = (-1, -1, 0, 1, 2, 5, 9, 50, 2 ** 24)[trial % 9]
        got, want = ref.edt(seeds, limit), ref.brute_force(seeds, limit)
        assert got[0].dtype == np.int32 and got[1].dtype == np.int32
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all(), (shape, limit)
        if limit < 0:  # the limited result is the unlimited one masked
            for m in (0, 3, 9):
                lim = ref.edt(seeds, m)
                far = got[0] > m
                assert (lim[0] == np.where(far, NONE, got[0])).all() and (lim[1] == np.where(far, -1, got[1])).all()
        q = np.argwhere(seeds != 0)
        p = np.stack(np.indices(shape), axis=-1).reshape(-1, 1, 3)
        ties += int((((p - q[None]) ** 2).sum(axis=2) == want[0].reshape(-1, 1)).sum(axis=1).max() > 1)
    assert ties >= (5 if density >= 0.05 else 1)  # (the rule was exercised; at 0.01 most volumes hold a single seed)


def test_restatement_hand_cases():
    shape = (4, 5, 6)
    d2, near = ref.edt(np.zeros(shape, np.uint8))
    assert (d2 == NONE).all() and (near == -1).all()
    d2, near = ref.edt(np.full(shape, 200, np.uint8))
    assert (d2 == 0).all() and (near.ravel() == np.arange(4 * 5 * 6)).all()
    # two seeds mirror-symmetric about the plane z = 2: the plane names the smaller index
    s = np.zeros(shape, np.uint8)
    s[1, 2, 0] = s[1, 2, 4] = 1
    d2, near = ref.edt(s)
    lo, hi = (1 * 5 + 2) * 6 + 0, (1 * 5 + 2) * 6 + 4
    assert (near[:, :, 2] == lo).all() and (near[:, :, 3:] == hi).all() and (near[:, :, :2] == lo).all()
    assert d2[3, 0, 2] == 4 + 4 + 4
    # the passes one by one are the passes at once
    seeds = ref.random_seeds((7, 6, 9), 0.05)
    step = ref.edt(seeds, 9, phases=('z',))
    step = ref.edt(seeds, 9, phases=('y',), start=step)
    step = ref.edt(seeds, 9, phases=('x',), start=step)
    once = ref.edt(seeds, 9)
    assert (step[0] == once[0]).all() and (step[1] == once[1]).all()


@pytest.mark.parametrize('shape', ref.SHAPES)
def test_restatement_equals_scipy_on_the_gpu_shapes(shape):
    from scipy import ndimage
    for density in (0.02, 0.3):
        seeds = ref.random_seeds(shape, density)
        d2, near = ref.edt(seeds)
        want = np.rint(ndimage.distance_transform_edt(seeds == 0) ** 2).astype(np.int64)
        assert (d2 == want).all(), (shape, density)
        # the named seed is a seed at that distance
        q = np.stack(np.unravel_index(near.ravel(), shape), axis=1)
        p = np.stack(np.indices(shape), axis=-1).reshape(-1, 3)
        assert (seeds.ravel()[near.ravel()] != 0).all() and (((p - q) ** 2).sum(axis=1) == d2.ravel()).all()


@pytest.mark.parametrize('radius,r2', [(1, 1), (1.5, 2), (1.8, 3), (3, 9)])
def test_dilation_equals_scipy_with_the_euclidean_ball(radius, r2):
    from scipy import ndimage
    assert distance._radius2('dilate', 'radius', radius) == r2
    k = int(np.floor(np.sqrt(r2)))
    ax = np.arange(-k, k + 1)
    ball = (ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2) <= r2
    for shape, density in (((17, 13, 30), 0.02), ((5, 67, 9), 0.01), ((1, 1, 130), 0.05)):
        mask = ref.random_seeds(shape, density)
        want = ndimage.binary_dilation(mask != 0, structure=ball, border_value=0)
        assert (ref.dilate(mask, r2) == want).all(), (shape, r2)
        # erosion, with the outside of the box as foreground: ~dilate(~mask)
        solid = ndimage.binary_dilation(mask != 0, structure=np.ones((5, 5, 5), bool))
        eroded = 1 - ref.dilate((~solid).astype(np.uint8), r2)
        assert (eroded == ndimage.binary_erosion(solid, structure=ball, border_value=1)).all(), (shape, r2)


def test_surface_mask_and_esdf_semantics():
    h = np.float16
    sub = np.array([1], np.uint16).view(np.float16)[0]  # the smallest subnormal
    # a z row of 12 voxels: (tsdf, weight) - a crossing counts only between two observed voxels of opposite sides
    t = np.array([0.5, -0.5, -0.5, np.nan, 0.5, -0.0, 0.0, -sub, 0.5, -0.5, 0.5, -0.5], h).reshape(1, 1, 12)
    w = np.array([1, 1, 1, 1, 1, 1, 1, sub, 1, 0, -1, -0.0], h).reshape(1, 1, 12)
    # voxel:        0  1  2  3    4  5     6    7     8  9   10  11
    # state:        o  i  i  un   o  o(-0) o(0) i     o  un  un  un
    assert ref.surface_mask(t, w).ravel().tolist() == [1, 1, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0]
    # across x and across y
    t3 = np.full((3, 3, 3), 0.5, h)
    w3 = np.ones((3, 3, 3), h)
    t3[1, 1, 1] = -0.5
    want = np.zeros((3, 3, 3), np.uint8)
    want[1, 1, :] = want[1, :, 1] = want[:, 1, 1] = 1
    assert (ref.surface_mask(t3, w3) == want).all()
    w3[0, 1, 1] = 0  # an unobserved neighbour is no neighbour
    want[0, 1, 1] = 0
    assert (ref.surface_mask(t3, w3) == want).all()

    d2 = np.array([0, 1, 2, 3, NONE, 4, 0, 9, NONE, 16, 3 * 2047 ** 2, 1], np.int32).reshape(1, 1, 12)
    res = 0.02
    e = ref.esdf(d2, t, w, res, 0.24).ravel()
    assert e.dtype == np.float32
    r32 = np.float32(res)
    assert e[0] == 0 and not np.signbit(e[0]) and e[1] == -r32 and e[2] == -(r32 * np.sqrt(np.float32(2)))
    assert e[3] == r32 * np.sqrt(np.float32(3))  # unobserved: unsigned
    assert e[4] == np.float32(0.24) and e[5] == r32 * 2 and e[6] == 0 and e[7] == -(r32 * 3)
    assert e[8] == np.float32(0.24) and e[9] == r32 * 4 and e[11] == r32
    assert e[10] == r32 * np.sqrt(np.float32(3 * 2047 ** 2))  # (exact in fp32: d² < 2^24)
    e = ref.esdf(d2, -np.abs(t), np.ones_like(w), res, np.inf).ravel()
    assert e[4] == -np.inf and e[8] == -np.inf and np.signbit(e[0]) and e[0] == 0  # -0.0 at an inside seed


def test_python_layer_refusals():
    t = torch.zeros((4, 4, 4), dtype=torch.float16)
    w = torch.zeros((4, 4, 4), dtype=torch.float16)
    m = torch.ones((4, 4, 4), dtype=torch.uint8)
    for bad in (-1, float('nan'), float('inf'), 'far', True):
        with pytest.raises(ValueError, match='max_distance'):
            distance.edt(m, bad)
        with pytest.raises(ValueError, match='max_distance'):
            distance.esdf(t, w, 0.02, bad)
        with pytest.raises(ValueError, match='radius'):
            distance.dilate(m, bad)
        with pytest.raises(ValueError, match='radius'):
            distance.erode(m, bad)
    with pytest.raises(ValueError, match='radius'):
        distance.dilate(m, None)
    with pytest.raises(ValueError, match='radius'):
        distance.erode(m, None)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match='max_dist2'):
            distance.edt(m, max_dist2=bad)
    with pytest.raises(ValueError, match='at most one'):
        distance.edt(m, 2.0, max_dist2=4)
    for bad in (0, -0.02, float('nan'), float('inf'), None):
        with pytest.raises(ValueError, match='resolution'):
            distance.esdf(t, w, bad)
    with pytest.raises(ValueError, match='seeds'):
        distance.edt(m.int())
    with pytest.raises(ValueError, match='seeds'):
        distance.edt(m[:, :, ::2])  # strided
    with pytest.raises(ValueError, match='seeds'):
        distance.edt(m.numpy())
    with pytest.raises(ValueError, match='weights'):  # mismatched shapes
        distance.surface_mask(t, w[:3])
    with pytest.raises(ValueError, match='weights'):
        distance.esdf(t, w.float(), 0.02)
    with pytest.raises(ValueError, match='tsdf'):
        distance.surface_mask(t.float(), w)
    with pytest.raises(ValueError, match='nearest'):
        distance.nearest_values(m, m)
    with pytest.raises(ValueError, match='values'):
        distance.nearest_values(m[:2], m.int())
    # well-formed host tensors: refused for where they live, by name, before the library is asked for a device
    for call in (lambda: distance.edt(m), lambda: distance.edt(m, 3), lambda: distance.surface_mask(t, w), lambda: distance.esdf(t, w, 0.02),
                 lambda: distance.dilate(m, 2), lambda: distance.erode(m.bool(), 2)):
        with pytest.raises(ValueError, match='cuda'):
            call()
    # nearest_values is plain indexing: host tensors will do
    near = torch.tensor([[[1, -1, 1, 3]]], dtype=torch.int32)
    vals = torch.tensor([[[5, 6, 7, 8]]], dtype=torch.uint8)
    assert distance.nearest_values(vals, near, fill=9).tolist() == [[[6, 9, 6, 8]]]
    rgb = torch.arange(12, dtype=torch.uint8).reshape(1, 1, 4, 3)
    assert distance.nearest_values(rgb, near, fill=0).tolist() == [[[[3, 4, 5], [0, 0, 0], [3, 4, 5], [9, 10, 11]]]]


def test_database_refuses_host_state():
    from online_joint_depthfusion_and_semantic_amd.database import Database

    class Grid:
        volume = None

    db = Database.__new__(Database)
    db.scenes, db.initial_value, db.resolution = ['s'], 0.1, {'s': 0.02}
    host = np.zeros((4, 4, 4), np.float16)
    db.scenes_est, db.fusion_weights = {'s': Grid()}, {'s': host}
    db.scenes_est['s'].volume = host.copy()
    with pytest.raises(ValueError, match='not resident'):
        db.esdf('s')
    db.scenes_est['s'].volume, db.fusion_weights['s'] = torch.from_numpy(host.copy()), torch.from_numpy(host.copy())  # host tensors
    with pytest.raises(ValueError, match='not resident'):
        db.esdf('s', max_distance=0.24)


def test_abi_refusals_without_a_device():
    import ctypes
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15  # host bytes nothing reads: every call below is refused before any HIP call
    wsb = lib.ojf_volume_edt_workspace_bytes
    assert wsb(4, 4, 4) == 256 and wsb(3, 5, 65) == (975 * 4 + 7) // 8 * 8 and wsb(2048, 1, 2048) == 4 * 2048 * 2048
    assert wsb(0, 4, 4) == 0 and wsb(4, -1, 4) == 0 and wsb(2049, 1, 1) == 0 and wsb(2048, 1024, 1024) == 0 and wsb(2047, 1024, 1024) > 0
    assert (_lib.EDT_Z, _lib.EDT_Y, _lib.EDT_X, _lib.EDT_ALL, _lib.EDT_NONE) == (1, 2, 4, 7, NONE)

    def edt(seeds=p, dims=(4, 4, 4), limit=-1, phases=_lib.EDT_ALL, ws=p + 1024, ws_bytes=None, dist2=p + 2048, nearest=p + 3072):
        ws_bytes = wsb(4, 4, 4) if ws_bytes is None else ws_bytes
        return lib.ojf_volume_edt(seeds, *dims, limit, phases, ws, ws_bytes, dist2, nearest, None)

    cases = [(dict(seeds=None), b'null'), (dict(ws=None), b'null'), (dict(dist2=None), b'null'), (dict(nearest=None), b'null'),
             (dict(dims=(0, 4, 4)), b'1..2048'), (dict(dims=(4, 4, -4)), b'1..2048'), (dict(dims=(4, 2049, 1)), b'1..2048'),
             (dict(dims=(2048, 1024, 1024)), b'too large'), (dict(phases=0), b'phases'), (dict(phases=8), b'phases'),
             (dict(ws_bytes=wsb(4, 4, 4) - 1), b'workspace too small'), (dict(ws=p + 1028), b'aligned'), (dict(dist2=p + 2050), b'aligned')]
    for fault, word in cases:
        assert edt(**fault) != 0, fault
        msg = lib.ojf_last_error()
        assert msg.startswith(b'ojf_volume_edt:') and word in msg, (fault, msg)

    sm = lib.ojf_volume_surface_mask
    assert sm(None, p, 4, 4, 4, p + 512, None) != 0 and b'null' in lib.ojf_last_error()
    assert sm(p, None, 4, 4, 4, p + 512, None) != 0 and b'null' in lib.ojf_last_error()
    assert sm(p, p + 128, 4, 4, 4, None, None) != 0 and b'null' in lib.ojf_last_error()
    assert sm(p, p + 128, 4, 0, 4, p + 512, None) != 0 and b'1..2048' in lib.ojf_last_error()
    assert sm(p, p + 128, 4, 4, 4096, p + 512, None) != 0 and b'1..2048' in lib.ojf_last_error()
    assert sm(p + 1, p + 128, 4, 4, 4, p + 512, None) != 0 and b'aligned' in lib.ojf_last_error()
    es = lib.ojf_volume_esdf
    assert es(None, p, p + 128, 8, 0.02, 1.0, p + 512, None) != 0 and b'null' in lib.ojf_last_error()
    assert es(p, p + 128, p + 256, 8, 0.02, 1.0, None, None) != 0 and b'null' in lib.ojf_last_error()
    assert es(p, p + 128, p + 256, 0, 0.02, 1.0, p + 512, None) != 0 and b'voxel count' in lib.ojf_last_error()
    assert es(p, p + 128, p + 256, 2 ** 31, 0.02, 1.0, p + 512, None) != 0 and b'voxel count' in lib.ojf_last_error()
    for res in (0.0, -1.0, float('nan'), float('inf')):
        assert es(p, p + 128, p + 256, 8, res, 1.0, p + 512, None) != 0 and b'resolution' in lib.ojf_last_error()
    for far in (-1.0, float('nan')):
        assert es(p, p + 128, p + 256, 8, 0.02, far, p + 512, None) != 0 and b'far' in lib.ojf_last_error()
    assert es(p + 2, p + 128, p + 256, 8, 0.02, 1.0, p + 512, None) != 0 and b'aligned' in lib.ojf_last_error()
    assert bytes(buf) == bytes(4096)  # nothing was written
