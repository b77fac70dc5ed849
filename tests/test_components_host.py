"""CPU: the numpy restatement of the connected-components definition (components_ref.py) against scipy.ndimage.label and
against hand-made volumes whose sizes and boxes follow from their construction; the observed-mask rule; the refusals of the
Python layer and of the C ABI, none of which needs a device."""
import numpy as np
import pytest
import torch

from online_joint_depthfusion_and_semantic_amd import _lib, components
import components_ref as ref

SHAPE = (24, 20, 28)


def _scipy_labels(fg, connectivity):
    """labels by scipy: the partition of ndimage.label, every component named by its smallest linear index."""
    from scipy import ndimage
    structure = ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3)
    lab, n = ndimage.label(fg, structure=structure)
    out = np.full(fg.shape, -1, np.int64)
    if n:
        index = np.arange(fg.size).reshape(fg.shape)
        smallest = ndimage.minimum(index, lab, np.arange(1, n + 1)).astype(np.int64)
        out[lab > 0] = smallest[lab[lab > 0] - 1]
    return out


def _check_list(r, labels):
    """The list and ids of a result follow from its labels."""
    fg = labels >= 0
    roots, sizes = np.unique(labels[fg], return_counts=True)
    assert r['n'] == len(roots) and (r['roots'] == roots).all() and (r['sizes'] == sizes).all()
    assert r['roots'].dtype == np.int32 and r['sizes'].dtype == np.int32 and r['boxes'].dtype == np.int32 and r['keys'].dtype == np.uint8
    assert (r['ids'][fg] == np.searchsorted(roots, labels[fg])).all() and (r['ids'][~fg] == -1).all()
    for i, root in enumerate(roots):
        where = np.argwhere(labels == root)
        assert (r['boxes'][i] == np.concatenate([where.min(axis=0), where.max(axis=0)])).all()


@pytest.mark.parametrize('connectivity,density', [(6, 0.2), (6, 0.31), (6, 0.42), (26, 0.05), (26, 0.10), (26, 0.16)])
def test_restatement_equals_scipy_label(connectivity, density):
    """Densities on both sides of the site-percolation thresholds (0.31 for faces, 0.10 for the 3x3x3 neighbourhood): many
    small components below, one that spans the volume above."""
    rng = np.random.default_rng(int(1000 * density) + connectivity)
    mask = (rng.random(SHAPE) < density).astype(np.uint8) * rng.integers(1, 256, SHAPE).astype(np.uint8)  # any non-zero byte
    r = ref.label_components(mask, None, connectivity)
    want = _scipy_labels(mask != 0, connectivity)
    assert (r['labels'] == want).all()
    _check_list(r, want)
    assert (r['keys'] == 0).all()
    # with keys: one label call per key value
    keys = rng.integers(0, 4, SHAPE).astype(np.uint8)
    rk = ref.label_components(mask, keys, connectivity)
    want = np.full(SHAPE, -1, np.int64)
    for k in range(4):
        part = _scipy_labels((mask != 0) & (keys == k), connectivity)
        want[part >= 0] = part[part >= 0]
    assert (rk['labels'] == want).all()
    _check_list(rk, want)
    assert (rk['keys'] == keys.ravel()[rk['roots']]).all()
    # no mask: every voxel is foreground
    rn = ref.label_components(None, keys, connectivity)
    want = np.full(SHAPE, -1, np.int64)
    for k in range(4):
        part = _scipy_labels(keys == k, connectivity)
        want[part >= 0] = part[part >= 0]
    assert (rn['labels'] == want).all()


@pytest.mark.parametrize('connectivity', [6, 26])
def test_hand_cases(connectivity):
    shape = (5, 6, 7)
    V = 5 * 6 * 7
    r = ref.label_components(np.zeros(shape, np.uint8), None, connectivity)  # empty
    assert r['n'] == 0 and (r['labels'] == -1).all() and (r['ids'] == -1).all() and r['boxes'].shape == (0, 6)
    r = ref.label_components(np.ones(shape, np.uint8), None, connectivity)  # full
    assert r['n'] == 1 and (r['labels'] == 0).all() and (r['ids'] == 0).all()
    assert r['sizes'].tolist() == [V] and r['boxes'].tolist() == [[0, 0, 0, 4, 5, 6]] and r['roots'].tolist() == [0]
    one = np.zeros(shape, np.uint8)  # a single voxel at the last index
    one[4, 5, 6] = 9
    r = ref.label_components(one, None, connectivity)
    assert r['n'] == 1 and r['roots'].tolist() == [V - 1] and r['sizes'].tolist() == [1] and r['boxes'].tolist() == [[4, 5, 6, 4, 5, 6]]
    assert r['labels'][4, 5, 6] == V - 1 and (r['labels'] >= 0).sum() == 1

    board = ref.checkerboard(shape)
    r = ref.label_components(board, None, connectivity)
    if connectivity == 6:  # all singletons
        assert r['n'] == board.sum() and (r['sizes'] == 1).all() and (r['roots'] == np.flatnonzero(board)).all()
        assert (r['boxes'][:, :3] == r['boxes'][:, 3:]).all() and (r['boxes'][:, :3] == np.argwhere(board)).all()
    else:  # held together by edge diagonals
        assert r['n'] == 1 and r['sizes'].tolist() == [board.sum()] and r['boxes'].tolist() == [[0, 0, 0, 4, 5, 6]]

    cubes = ref.corner_cubes((6, 6, 6), (3, 3, 3))
    r = ref.label_components(cubes, None, connectivity)
    if connectivity == 6:
        assert r['n'] == 2 and r['sizes'].tolist() == [8, 8] and r['boxes'].tolist() == [[1, 1, 1, 2, 2, 2], [3, 3, 3, 4, 4, 4]]
        assert r['roots'].tolist() == [(1 * 6 + 1) * 6 + 1, (3 * 6 + 3) * 6 + 3]
    else:
        assert r['n'] == 1 and r['sizes'].tolist() == [16] and r['boxes'].tolist() == [[1, 1, 1, 4, 4, 4]]

    # two cubes of key 5 with a one-voxel wall of key 2 between them: three components whatever the connectivity
    keys = np.zeros((3, 3, 7), np.uint8)
    keys[:, :, :3], keys[:, :, 3], keys[:, :, 4:] = 5, 2, 5
    r = ref.label_components(None, keys, connectivity)
    assert r['n'] == 3 and r['roots'].tolist() == [0, 3, 4] and r['keys'].tolist() == [5, 2, 5] and r['sizes'].tolist() == [27, 9, 27]
    assert r['boxes'].tolist() == [[0, 0, 0, 2, 2, 2], [0, 0, 3, 2, 2, 3], [0, 0, 4, 2, 2, 6]]
    assert (r['ids'][:, :, :3] == 0).all() and (r['ids'][:, :, 3] == 1).all() and (r['ids'][:, :, 4:] == 2).all()

    snake, size = ref.serpentine((7, 6, 9))
    assert snake.sum() == size
    r = ref.label_components(snake, None, connectivity)
    assert r['n'] == 1 and r['sizes'].tolist() == [size] and r['boxes'].tolist() == [[0, 0, 0, 6, 4, 8]] and r['roots'].tolist() == [0]


def test_serpentine_is_a_path():
    """One voxel wide: under face connectivity every voxel has two neighbours but the two ends."""
    from scipy import ndimage
    snake, _ = ref.serpentine((7, 6, 9))
    degree = ndimage.convolve(snake.astype(np.int32), ndimage.generate_binary_structure(3, 1).astype(np.int32), mode='constant') - 1
    assert sorted(np.bincount(degree[snake > 0]).tolist()) == [0, 2, snake.sum() - 2]


def test_observed_mask_semantics():
    h = np.float16
    sub = np.array([1], np.uint16).view(np.float16)[0]  # the smallest subnormal
    weights = np.array([1, -0.0, 0.0, np.nan, -1, sub, 1, 1, 1, 1], h)
    tsdf = np.array([0.01, 0.01, 0.01, 0.01, 0.01, 0.01, np.nan, 0.0400390625, -0.0400390625, -0.03], h)
    assert ref.observed_mask(tsdf, weights).tolist() == [1, 0, 0, 0, 0, 1, 0, 1, 1, 1]
    band = float(np.float16(0.0400390625))  # |v| == band is outside
    assert ref.observed_mask(tsdf, weights, band).tolist() == [1, 0, 0, 0, 0, 1, 0, 0, 0, 1]
    assert ref.observed_mask(tsdf, weights, np.inf).tolist() == [1, 0, 0, 0, 0, 1, 0, 1, 1, 1]


def test_keep_flags():
    sizes, roots = np.array([5, 9, 5, 1, 9]), np.array([0, 7, 20, 31, 40])
    assert components.keep_flags(sizes, roots, min_voxels=5).tolist() == [1, 1, 1, 0, 1]
    assert components.keep_flags(sizes, roots, keep_largest=1).tolist() == [0, 1, 0, 0, 0]  # of equal sizes the smaller root
    assert components.keep_flags(sizes, roots, keep_largest=3).tolist() == [1, 1, 0, 0, 1]
    assert components.keep_flags(sizes, roots, keep_largest=9).tolist() == [1, 1, 1, 1, 1]
    for kw in (dict(min_voxels=5), dict(keep_largest=1), dict(keep_largest=3)):
        assert (components.keep_flags(sizes, roots, **kw) == ref.keep_flags(sizes, roots, **kw)).all()


def test_python_layer_refusals():
    t = torch.zeros((4, 4, 4), dtype=torch.float16)
    w = torch.zeros((4, 4, 4), dtype=torch.float16)
    m = torch.ones((4, 4, 4), dtype=torch.uint8)
    rm = components.remove_small_components
    for kw in (dict(), dict(min_voxels=2, keep_largest=1), dict(min_voxels=0), dict(keep_largest=0), dict(min_voxels=1.5)):
        with pytest.raises(ValueError, match='min_voxels|keep_largest'):
            rm(t, w, init_value=0.1, **kw)
    with pytest.raises(ValueError, match='connectivity'):
        rm(t, w, init_value=0.1, min_voxels=2, connectivity=18)
    with pytest.raises(ValueError, match='connectivity'):
        components.label_components(m, connectivity=18)
    with pytest.raises(ValueError, match='band'):
        rm(t, w, init_value=0.1, min_voxels=2, band=0.0)
    with pytest.raises(ValueError, match='band'):
        components.observed_mask(t, w, band=float('nan'))
    with pytest.raises(ValueError, match='weights'):  # mismatched shapes
        rm(t, w[:3], init_value=0.1, min_voxels=2)
    with pytest.raises(ValueError, match='weights'):  # mismatched dtypes
        components.observed_mask(t, w.float())
    with pytest.raises(ValueError, match='tsdf'):
        components.observed_mask(t.float(), w)
    with pytest.raises(ValueError, match='tsdf'):
        components.observed_mask(t.numpy(), w)
    with pytest.raises(ValueError, match='keys'):
        components.label_components(m, m[:, :2])
    with pytest.raises(ValueError, match='mask'):
        components.label_components(m.int())
    with pytest.raises(ValueError, match='mask'):
        components.label_components(m[:, :, ::2])  # strided
    with pytest.raises(ValueError, match='needed'):
        components.label_components()
    with pytest.raises(ValueError, match='ids'):
        components.instances(m.float(), t, w)
    with pytest.raises(ValueError, match='min_voxels'):
        components.instances(m, t, w, min_voxels=0)
    # well-formed host tensors: refused for where they live, by name, before the library is asked for a device
    for call in (lambda: components.label_components(m), lambda: components.observed_mask(t, w),
                 lambda: rm(t, w, init_value=0.1, min_voxels=2), lambda: components.instances(m, t, w)):
        with pytest.raises(ValueError, match='cuda'):
            call()


def test_database_refuses_host_state():
    """filter_components and instances ask for resident volumes (after to_numpy there are none), whatever the device; the
    criteria are checked first."""
    from online_joint_depthfusion_and_semantic_amd.database import Database

    class Grid:
        volume = None

    db = Database.__new__(Database)
    db.scenes, db.initial_value, db.semantics = ['s'], 0.1, True
    host = np.zeros((4, 4, 4), np.float16)
    db.scenes_est, db.fusion_weights, db.ids_est = {'s': Grid()}, {'s': host}, {'s': Grid()}
    db.scenes_est['s'].volume, db.ids_est['s'].volume = host.copy(), np.zeros((4, 4, 4), np.uint8)
    with pytest.raises(ValueError, match='not resident'):
        db.filter_components(min_voxels=3)
    db.scenes_est['s'].volume, db.fusion_weights['s'] = torch.from_numpy(host.copy()), torch.from_numpy(host.copy())  # host tensors
    with pytest.raises(ValueError, match='not resident'):
        db.filter_components(keep_largest=1)
    with pytest.raises(ValueError, match='min_voxels'):
        db.filter_components()
    with pytest.raises(ValueError, match='min_voxels'):
        db.filter_components(min_voxels=3, keep_largest=1)
    with pytest.raises(ValueError, match='not resident'):
        db.instances('s')
    db.semantics = False
    with pytest.raises(ValueError, match='semantics'):
        db.instances('s')


def test_abi_refusals_without_a_device():
    import ctypes
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15  # host bytes nothing reads: every call below is refused before any HIP call
    wsb = lib.ojf_volume_components_workspace_bytes
    assert wsb(4, 4, 4) == ((64 + 1 + 1) * 4 + 7) // 8 * 8 and wsb(3, 5, 65) == ((975 + 1 + 1) * 4 + 7) // 8 * 8
    assert wsb(8, 16, 16) == (2048 + 2 + 1) * 4 + 4
    assert wsb(0, 4, 4) == 0 and wsb(4, -1, 4) == 0 and wsb(2048, 1024, 1024) == 0 and wsb(2047, 1024, 1024) > 0

    def label(mask=p, keys=p + 64, dims=(4, 4, 4), conn=6, phases=_lib.COMPONENTS_ALL, ws=p + 128, ws_bytes=None, labels=p + 1024,
              ids=p + 2048, lists=(p + 3072, p + 3200, p + 3328, p + 3456), cap=0, count=p + 3900):
        ws_bytes = wsb(4, 4, 4) if ws_bytes is None else ws_bytes
        return lib.ojf_volume_components(mask, keys, *dims, conn, phases, ws, ws_bytes, labels, ids, *lists, cap, count, None)

    cases = [(dict(labels=None), b'null'), (dict(ids=None), b'null'), (dict(ws=None), b'null'), (dict(count=None), b'count_dev'),
             (dict(cap=4, lists=(None, p, p, p)), b'list arrays'), (dict(cap=4, lists=(p, p, p, None)), b'list arrays'),
             (dict(dims=(0, 4, 4)), b'non-positive'), (dict(dims=(4, 4, -4)), b'non-positive'),
             (dict(dims=(2048, 1024, 1024)), b'too large'), (dict(dims=(65536, 65536, 1)), b'too large'),
             (dict(conn=18), b'connectivity'), (dict(conn=0), b'connectivity'), (dict(phases=0), b'phases'), (dict(phases=32), b'phases'),
             (dict(phases=_lib.COMPONENTS_LIST), b'capacity 0'), (dict(ws_bytes=wsb(4, 4, 4) - 1), b'workspace too small'),
             (dict(ws=p + 132), b'aligned'), (dict(labels=p + 1026), b'aligned')]
    for fault, word in cases:
        assert label(**fault) != 0, fault
        msg = lib.ojf_last_error()
        assert msg.startswith(b'ojf_volume_components:') and word in msg, (fault, msg)

    assert lib.ojf_volume_observed_mask(None, p, 8, 0, 0.0, p + 64, None) != 0 and b'null' in lib.ojf_last_error()
    assert lib.ojf_volume_observed_mask(p, p + 32, 8, 0, 0.0, None, None) != 0 and b'null' in lib.ojf_last_error()
    assert lib.ojf_volume_observed_mask(p, p + 32, 0, 0, 0.0, p + 64, None) != 0 and b'voxel count' in lib.ojf_last_error()
    assert lib.ojf_volume_observed_mask(p, p + 32, 2 ** 31, 0, 0.0, p + 64, None) != 0 and b'voxel count' in lib.ojf_last_error()
    for band in (0.0, -1.0, float('nan')):
        assert lib.ojf_volume_observed_mask(p, p + 32, 8, 1, band, p + 64, None) != 0 and b'band' in lib.ojf_last_error()
    assert lib.ojf_volume_components_apply(None, p, 1, p + 64, p + 128, 8, 0.1, None) != 0 and b'null' in lib.ojf_last_error()
    assert lib.ojf_volume_components_apply(p, None, 1, p + 64, p + 128, 8, 0.1, None) != 0 and b'null' in lib.ojf_last_error()
    assert lib.ojf_volume_components_apply(p, p + 32, 1, None, p + 128, 8, 0.1, None) != 0 and b'null' in lib.ojf_last_error()
    assert lib.ojf_volume_components_apply(p, p + 32, 1, p + 64, p + 128, 2 ** 31, 0.1, None) != 0 and b'voxel count' in lib.ojf_last_error()
    assert lib.ojf_volume_components_apply(p + 2, p + 32, 1, p + 64, p + 128, 8, 0.1, None) != 0 and b'aligned' in lib.ojf_last_error()
    assert lib.ojf_volume_components_apply(p, None, 0, p + 64, p + 128, 8, 0.1, None) == 0  # no component: nothing to do, no launch
