"""-m gpu: connected components on the device (ojf_volume_components, components.py, Database.filter_components /
Database.instances) against the numpy restatement (components_ref.py).  Every comparison is bit equality of labels, ids, n,
roots, sizes, keys and boxes.  Shapes are the smallest that reach every edge of the 4 x 4 x 64 brick and every kind of seam."""
import functools

import numpy as np
import pytest
import torch

from online_joint_depthfusion_and_semantic_amd import _lib, components, synthetic
from online_joint_depthfusion_and_semantic_amd.config import default_config, database_config
from online_joint_depthfusion_and_semantic_amd.database import Database
import components_ref as ref

pytestmark = pytest.mark.gpu

BX, BY, BZ = 4, 4, 64  # csrc/ojf_components.hip: kCBx, kCBy, kCBz
FIELDS = ('labels', 'ids', 'n', 'roots', 'sizes', 'keys', 'boxes')


def _same(got, want, what):
    for k in FIELDS:
        g = got[k].cpu().numpy() if torch.is_tensor(got[k]) else got[k]
        if k == 'n':
            assert g == want[k], (what, k, g, want[k])
            continue
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (what, k, g.dtype, g.shape, want[k].dtype, want[k].shape)
        bad = np.flatnonzero((g != want[k]).ravel())
        assert len(bad) == 0, (what, k, len(bad), bad[:5], g.ravel()[bad[:5]], want[k].ravel()[bad[:5]])


def _run(mask, keys, connectivity, cuda):
    dev = lambda a: None if a is None else torch.from_numpy(a).to(cuda)  # noqa: E731
    return components.label_components(dev(mask), dev(keys), connectivity=connectivity)


@functools.lru_cache(maxsize=None)
def _random_case(shape, connectivity, with_keys):
    rng = np.random.default_rng(hash((shape, connectivity, with_keys)) % 2 ** 32)
    mask = (rng.random(shape) < (0.3 if connectivity == 6 else 0.1)).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)
    keys = rng.integers(0, 4, shape).astype(np.uint8) if with_keys else None
    return mask, keys, ref.label_components(mask, keys, connectivity)


EDGE_SHAPES = [(1, 1, 1), (2, 2, 2), (BX - 1, BY - 1, BZ - 1), (BX, BY, BZ), (BX + 1, BY + 1, BZ + 1), (2 * BX + 1, 3, 2 * BZ + 3),
               (3, 5, 65), (9, 33, 5), (17, 13, 130)]


@pytest.mark.parametrize('with_keys', [False, True])
@pytest.mark.parametrize('connectivity', [6, 26])
@pytest.mark.parametrize('shape', EDGE_SHAPES)
def test_brick_edges(cuda, shape, connectivity, with_keys):
    mask, keys, want = _random_case(shape, connectivity, with_keys)
    _same(_run(mask, keys, connectivity, cuda), want, (shape, connectivity, with_keys))
    if with_keys and shape == (17, 13, 130):  # no mask: every voxel is foreground, the keys alone cut the volume
        _same(_run(None, keys, connectivity, cuda), ref.label_components(None, keys, connectivity), 'keys alone')


@pytest.mark.parametrize('connectivity', [6, 26])
def test_seam_serpentine(cuda, connectivity):
    """One path through every brick of (4Bx, 3By, 2Bz): the longest chain of unions the seam pass can be given."""
    shape = (4 * BX, 3 * BY, 2 * BZ)
    mask, size = ref.serpentine(shape)
    got = _run(mask, None, connectivity, cuda)
    assert got['n'] == 1 and got['sizes'].tolist() == [size] and got['roots'].tolist() == [0]
    assert got['boxes'].tolist() == [[0, 0, 0, shape[0] - 2, shape[1] - 2, shape[2] - 1]]
    labels = got['labels'].cpu().numpy()
    assert (labels[mask > 0] == 0).all() and (labels[mask == 0] == -1).all()
    _same(got, ref.label_components(mask, None, connectivity), 'serpentine')


@pytest.mark.parametrize('connectivity', [6, 26])
def test_seam_full_and_checkerboard(cuda, connectivity):
    shape = (2 * BX + 1, 2 * BY + 1, 2 * BZ + 2)
    got = _run(np.ones(shape, np.uint8), None, connectivity, cuda)
    assert got['n'] == 1 and got['sizes'].tolist() == [shape[0] * shape[1] * shape[2]] and (got['labels'] == 0).all()
    assert got['boxes'].tolist() == [[0, 0, 0, shape[0] - 1, shape[1] - 1, shape[2] - 1]]
    board = ref.checkerboard(shape)
    got = _run(board, None, connectivity, cuda)
    if connectivity == 6:
        assert got['n'] == board.sum() and (got['sizes'] == 1).all()
    else:  # one component, held together only across diagonals - across brick edges and brick corners too
        assert got['n'] == 1 and got['sizes'].tolist() == [board.sum()]
    _same(got, ref.label_components(board, None, connectivity), 'checkerboard')


@pytest.mark.parametrize('connectivity', [6, 26])
def test_components_that_meet_at_a_brick_corner(cuda, connectivity):
    shape = (2 * BX, 2 * BY, 2 * BZ)
    for side in (1, 2):
        mask = ref.corner_cubes(shape, (BX, BY, BZ), side)
        got = _run(mask, None, connectivity, cuda)
        assert got['n'] == (2 if connectivity == 6 else 1)
        assert got['sizes'].tolist() == ([side ** 3] * 2 if connectivity == 6 else [2 * side ** 3])
        _same(got, ref.label_components(mask, None, connectivity), ('corner', side))
    # the other diagonal of the corner: (-, +, +) against (+, -, -)
    mask = np.zeros(shape, np.uint8)
    mask[BX - 1, BY, BZ] = mask[BX, BY - 1, BZ - 1] = 1
    got = _run(mask, None, connectivity, cuda)
    assert got['n'] == (2 if connectivity == 6 else 1)
    _same(got, ref.label_components(mask, None, connectivity), 'corner, other diagonal')


def test_statistics_of_a_component_over_many_bricks(cuda):
    """A frame of thickness 1 around a (20, 20, 130) volume plus a rod through it: one component over all 75 bricks, and an
    island; sizes and boxes from the construction."""
    shape = (5 * BX, 5 * BY, 2 * BZ + 2)
    X, Y, Z = shape
    mask = np.ones(shape, np.uint8)
    mask[1:-1, 1:-1, 1:-1] = 0
    mask[X // 2, Y // 2, :] = 1
    mask[3:6, 3:5, 70:77] = 1
    shell = X * Y * Z - (X - 2) * (Y - 2) * (Z - 2) + (Z - 2)
    got = _run(mask, None, 6, cuda)
    assert got['n'] == 2 and got['sizes'].tolist() == [shell, 3 * 2 * 7] and got['roots'].tolist() == [0, (3 * Y + 3) * Z + 70]
    assert got['boxes'].tolist() == [[0, 0, 0, X - 1, Y - 1, Z - 1], [3, 3, 70, 5, 4, 76]]
    _same(got, ref.label_components(mask, None, 6), 'frame')


RUN_Y, RUN_Z = 16, 64  # one x slice = one run of 1024 voxels of the root count (csrc/ojf_components.hip: kCRun)


def _isolated_voxels(R):
    """u8 (R, 16, 64): foreground voxels of which no two are 26-adjacent, for the scan of the R root counts (one block of 1024
    lanes, lane t owns the counts [chunk·t, chunk·t + chunk)).  Run x holds 7x mod 5 voxels in its middle - 0 to 4, rows y that
    alternate with the parity of x.  Around a seam r between two lanes' chunks (behind lane 0, in the middle, in front of the
    last lane with work) the runs r - 2 and r hold their first voxel as well and the runs r - 1 and r + 1 their last.  The
    first and the last run are empty, but for R = 1, which holds its first, its last and 3 voxels between."""
    mask = np.zeros((R, RUN_Y, RUN_Z), np.uint8)
    if R == 1:
        mask[0, 0, 0] = mask[0, RUN_Y - 1, RUN_Z - 1] = 1
        mask[0, 4:9:2, 10] = 1
        return mask, []
    for x in range(1, R - 1):
        for k in range(7 * x % 5):
            mask[x, 4 + 2 * (x % 2) + 4 * (k % 2), 10 + 20 * (k // 2)] = 1
    chunk = (R + 1023) // 1024
    seams = sorted({chunk, (R // chunk // 2) * chunk, (R - 1) // chunk * chunk})
    for r in seams:
        for x, y, z in ((r - 2, 0, 0), (r, 0, 0), (r - 1, RUN_Y - 1, RUN_Z - 1), (r + 1, RUN_Y - 1, RUN_Z - 1)):
            if 0 < x < R - 1:
                mask[x, y, z] = 1
    return mask, seams


@pytest.mark.parametrize('R', [1, 1023, 1024, 1025, 2049])  # chunks of 1, 1, 1, 2 and 3 counts per lane of the scan
def test_rank_scan_at_its_chunk_edges(cuda, R):
    """Every foreground voxel is a component of its own, so the result is closed form: labels[v] = v, ids = the rank of v among
    the foreground voxels - the exclusive scan of the runs' root counts plus the rank inside the run -, sizes 1, boxes the
    voxel.  A wrong offset of one run shifts the ids of every voxel of the run."""
    mask, seams = _isolated_voxels(R)
    P = np.argwhere(mask)  # index order
    taken = set(map(tuple, P.tolist()))
    offsets = [d for d in np.ndindex(3, 3, 3) if d != (1, 1, 1)]
    assert not any((x + dx - 1, y + dy - 1, z + dz - 1) in taken for x, y, z in taken for dx, dy, dz in offsets)  # no two 26-adjacent
    per_run = mask.reshape(R, -1).sum(axis=1)
    if R > 1:
        assert per_run[0] == 0 and per_run[-1] == 0 and set(per_run[1:-1].tolist()) >= {0, 1, 2, 3, 4} and len(seams) == 3
        chunk = (R + 1023) // 1024
        for r in seams:  # the last voxel of a chunk's last run, the first voxel of the next chunk's first run
            assert r % chunk == 0 and 0 < r < R and (mask[r - 1, -1, -1] or r == 1) and (mask[r, 0, 0] or r == R - 1), r
        r = seams[1]  # the one in the middle has all four
        assert mask[r - 2, 0, 0] and mask[r - 1, -1, -1] and mask[r, 0, 0] and mask[r + 1, -1, -1]
    roots = np.flatnonzero(mask.ravel()).astype(np.int32)
    n = len(roots)
    want = {'labels': np.where(mask.ravel() > 0, np.arange(mask.size), -1).astype(np.int32).reshape(mask.shape),
            'ids': np.full(mask.size, -1, np.int32), 'n': n, 'roots': roots, 'sizes': np.ones(n, np.int32),
            'keys': np.zeros(n, np.uint8), 'boxes': np.concatenate([P, P], axis=1).astype(np.int32)}
    want['ids'][roots] = np.arange(n, dtype=np.int32)
    want['ids'] = want['ids'].reshape(mask.shape)
    _same(_run(mask, None, 26, cuda), want, ('isolated voxels', R))


def test_capacity_contract(cuda):
    """Capacity 0 returns n and writes nothing to the list; a list phase of its own fills it from what the first call left; one
    call with enough capacity does both; a smaller capacity drops the entries beyond it."""
    lib = _lib.load()
    shape = (17, 13, 130)
    mask, keys, want = _random_case(shape, 26, True)
    n = want['n']
    assert n > 8
    m, k = torch.from_numpy(mask).to(cuda), torch.from_numpy(keys).to(cuda)
    ws_bytes = lib.ojf_volume_components_workspace_bytes(*shape)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=cuda)
    st = _lib.stream_ptr(cuda)

    def call(phases, cap, lists, count=None):
        labels, ids = out['labels'], out['ids']
        rc = lib.ojf_volume_components(m.data_ptr(), k.data_ptr(), *shape, 26, phases, ws.data_ptr(), ws_bytes, labels.data_ptr(), ids.data_ptr(),
                                       *(None if a is None else a.data_ptr() for a in lists), cap, None if count is None else count.data_ptr(), st)
        assert rc == 0, lib.ojf_last_error()

    def fresh(cap):
        return [torch.full((cap,), -7, dtype=torch.int32, device=cuda), torch.full((cap,), -7, dtype=torch.int32, device=cuda),
                torch.full((cap,), 77, dtype=torch.uint8, device=cuda), torch.full((cap, 6), -7, dtype=torch.int32, device=cuda)]

    def result(lists, count, upto):
        return dict(labels=out['labels'], ids=out['ids'], n=int(count.item()), roots=lists[0][:upto].cpu().numpy(), sizes=lists[1][:upto].cpu().numpy(),
                    keys=lists[2][:upto].cpu().numpy(), boxes=lists[3][:upto].cpu().numpy())

    out = {'labels': torch.empty(shape, dtype=torch.int32, device=cuda), 'ids': torch.empty(shape, dtype=torch.int32, device=cuda)}
    count = torch.zeros(1, dtype=torch.int32, device=cuda)
    lists = fresh(n + 3)
    call(_lib.COMPONENTS_ALL, 0, lists, count)  # (the list arrays are given, and must stay untouched)
    assert int(count.item()) == n
    assert all((a == (77 if a.dtype == torch.uint8 else -7)).all() for a in lists)
    call(_lib.COMPONENTS_ALL, 0, [None] * 4, count)
    call(_lib.COMPONENTS_LIST, n + 3, lists)
    _same(result(lists, count, n), want, 'list phase')
    assert all((a[n:] == (77 if a.dtype == torch.uint8 else -7)).all() for a in lists)  # nothing behind entry n - 1

    out = {'labels': torch.empty(shape, dtype=torch.int32, device=cuda), 'ids': torch.empty(shape, dtype=torch.int32, device=cuda)}
    lists, count = fresh(n), torch.zeros(1, dtype=torch.int32, device=cuda)
    call(_lib.COMPONENTS_ALL, n, lists, count)
    _same(result(lists, count, n), want, 'one call')

    lists, count = fresh(8), torch.zeros(1, dtype=torch.int32, device=cuda)
    call(_lib.COMPONENTS_ALL, 5, lists, count)  # capacity 5 of arrays of 8
    cut = {f: (want[f][:5] if f in ('roots', 'sizes', 'keys', 'boxes') else want[f]) for f in FIELDS}
    _same(result(lists, count, 5), cut, 'capacity 5')
    assert all((a[5:] == (77 if a.dtype == torch.uint8 else -7)).all() for a in lists)


@pytest.mark.parametrize('connectivity', [6, 26])
def test_transposed_input_gives_the_same_partition(cuda, connectivity):
    """x <-> y changes every linear index, the brick every voxel falls in and the order of all unions: the partition stays."""
    mask, keys, want = _random_case((17, 13, 130), connectivity, True)
    got = _run(np.ascontiguousarray(mask.transpose(1, 0, 2)), np.ascontiguousarray(keys.transpose(1, 0, 2)), connectivity, cuda)
    a = got['labels'].cpu().numpy().transpose(1, 0, 2).ravel().astype(np.int64)
    b = want['labels'].ravel().astype(np.int64)
    assert ((a < 0) == (b < 0)).all() and got['n'] == want['n']
    fg = b >= 0
    pairs = np.unique(np.stack([a[fg], b[fg]]), axis=1)
    assert pairs.shape[1] == want['n']  # a bijection between the two sets of labels
    assert sorted(got['sizes'].tolist()) == sorted(want['sizes'].tolist())


def test_observed_mask_and_apply(cuda):
    """The observed mask against its restatement on special values at vector and tail positions, at an offset that defeats
    the 16-byte path; the removal writes float16(init) / 0 into the components that are not kept and nothing else."""
    rng = np.random.default_rng(5)
    n = 5 * 7 * 37
    sub = np.array([1], np.uint16).view(np.float16)[0]
    special_w = np.array([1, -0.0, 0.0, np.nan, -1, sub, np.inf, 2], np.float16)
    special_t = np.array([0.01, -0.03, np.nan, 0.0400390625, -0.0400390625, 0.04, 0.0, -0.0], np.float16)
    for off in (0, 1):
        t = torch.from_numpy(special_t[rng.integers(0, 8, n + off)]).to(cuda)[off:].view(5, 7, 37)
        w = torch.from_numpy(special_w[rng.integers(0, 8, n + off)]).to(cuda)[off:].view(5, 7, 37)
        assert off == 0 or t.data_ptr() % 16 != 0
        for band in (None, float(np.float16(0.0400390625)), 0.02):
            got = components.observed_mask(t, w, band).cpu().numpy()
            assert got.dtype == np.uint8 and (got == ref.observed_mask(t.cpu().numpy(), w.cpu().numpy(), band)).all(), (off, band)
    th, wh = t.cpu().numpy().copy(), w.cpu().numpy().copy()
    out = components.remove_small_components(t, w, init_value=0.1, min_voxels=3, connectivity=6)
    want = ref.label_components(ref.observed_mask(th, wh), None, 6)
    _same(out, want, 'remove_small_components')
    keep = ref.keep_flags(want['sizes'], want['roots'], min_voxels=3)
    assert (out['keep'] == keep).all() and 0 < keep.sum() < len(keep)
    ref.apply_removal(th, wh, want['ids'], keep, 0.1)
    assert (t.cpu().numpy().view(np.uint16) == th.view(np.uint16)).all() and (w.cpu().numpy().view(np.uint16) == wh.view(np.uint16)).all()


# ---- floaters ----------------------------------------------------------------------------------------------------------------
def _room_database(cuda, semantics=False):
    h, w, grid, frames = 48, 64, 64, 10
    cfg = default_config(h, w, semantics=semantics, model='tsdf')
    cfg.SETTINGS.device = str(cuda)
    st = synthetic.SyntheticStream(h, w, grid, frames)
    db = Database(st, database_config(cfg))
    for i in range(frames):
        f = st.frame(i)
        db.integrate_depth(st.scene, f['tof_depth'], f['intrinsics'], f['extrinsics'], mask=f['mask'])
    return db, st.scene


def _bits(db, s):
    return db.scenes_est[s].volume.cpu().numpy().view(np.uint16).copy(), db.fusion_weights[s].cpu().numpy().view(np.uint16).copy()


def test_floaters(cuda):
    """Three blobs of 1, 8 and 27 observed voxels, each with at least two unobserved voxels between it and anything observed,
    in a room fused from 10 frames (one component under 26): filter_components(min_voxels=28) takes exactly them back to the
    initial value and weight 0."""
    from scipy import ndimage
    db, s = _room_database(cuda)
    tsdf, wgt = db.scenes_est[s].volume, db.fusion_weights[s]
    before_t, before_w = _bits(db, s)
    taken = ref.observed_mask(before_t.view(np.float16), before_w.view(np.float16)) > 0
    room = ref.label_components(taken.astype(np.uint8), None, 26)
    assert room['n'] == 1 and room['sizes'][0] > 1000
    blobs = []
    for side in (1, 2, 3):
        far = ndimage.distance_transform_cdt(~taken, metric='chessboard') >= side + 3  # every voxel of the blob then has >= 4
        far[:2], far[:, :2], far[:, :, :2] = False, False, False
        far[64 - side - 2:], far[:, 64 - side - 2:], far[:, :, 64 - side - 2:] = False, False, False
        cand = np.argwhere(far)
        c = cand[len(cand) // 2]
        sl = tuple(slice(int(c[m]), int(c[m]) + side) for m in range(3))
        assert not taken[tuple(slice(int(c[m]) - 2, int(c[m]) + side + 2) for m in range(3))].any(), (side, c)
        taken[sl] = True
        blobs.append(sl)
        tsdf[sl] = 0.01
        wgt[sl] = 3.0
    planted_t, planted_w = _bits(db, s)
    want = ref.label_components(taken.astype(np.uint8), None, 26)
    assert want['n'] == 4 and sorted(want['sizes'].tolist()) == [1, 8, 27, int(room['sizes'][0])]
    init_bits = np.array([db.initial_value], np.float32).astype(np.float16).view(np.uint16)[0]
    for sl in blobs:
        assert (before_t[sl] == init_bits).all() and (before_w[sl] == 0).all() and (planted_w[sl] != 0).all()

    out = db.filter_components(min_voxels=1)  # every component has a voxel: nothing changes
    got_t, got_w = _bits(db, s)
    assert (got_t == planted_t).all() and (got_w == planted_w).all() and out[s]['keep'].all()
    _same(out[s], want, 'filter_components(min_voxels=1)')

    out = db.filter_components(min_voxels=28)
    _same(out[s], want, 'filter_components(min_voxels=28)')
    assert (out[s]['keep'] == (want['sizes'] >= 28)).all() and out[s]['keep'].sum() == 1
    got_t, got_w = _bits(db, s)
    for sl in blobs:  # back at the initial value and weight 0
        assert (got_t[sl] == init_bits).all() and (got_w[sl] == 0).all()
    assert (got_t == before_t).all() and (got_w == before_w).all()  # and every other voxel keeps its bits

    tsdf.copy_(torch.from_numpy(planted_t.view(np.float16)).to(cuda))
    wgt.copy_(torch.from_numpy(planted_w.view(np.float16)).to(cuda))
    out = db.filter_components(keep_largest=1)  # the same volumes
    assert (out[s]['keep'] == (want['sizes'] >= 28)).all()
    got_t, got_w = _bits(db, s)
    assert (got_t == before_t).all() and (got_w == before_w).all()
    with pytest.raises(ValueError):
        db.filter_components()


def test_instances(cuda):
    """Two separated boxes of class 7 and one of class 3 that touches one of them: three instances with their classes, sizes
    and boxes; min_voxels drops the smallest and renumbers the rest."""
    db, s = _room_database(cuda, semantics=True)
    shape = tuple(db.scenes_est[s].volume.shape)
    Y, Z = shape[1], shape[2]
    tsdf = torch.full(shape, db.initial_value, dtype=torch.float16, device=cuda)
    wgt = torch.zeros(shape, dtype=torch.float16, device=cuda)
    ids = torch.zeros(shape, dtype=torch.uint8, device=cuda)
    boxes = [((2, 3, 50), (6, 9, 60), 7), ((6, 3, 50), (9, 6, 54), 3), ((20, 20, 5), (23, 22, 8), 7)]  # [lo, hi), class; the second touches the first
    for lo, hi, cls in boxes:
        sl = tuple(slice(a, b) for a, b in zip(lo, hi))
        wgt[sl] = 1.0
        tsdf[sl] = 0.0
        ids[sl] = cls
    db.scenes_est[s].volume, db.fusion_weights[s], db.ids_est[s].volume = tsdf, wgt, ids
    sizes = [int(np.prod(np.subtract(hi, lo))) for lo, hi, _ in boxes]
    roots = [(lo[0] * Y + lo[1]) * Z + lo[2] for lo, _, _ in boxes]
    want_boxes = [list(lo) + [h - 1 for h in hi] for lo, hi, _ in boxes]
    for connectivity in (6, 26):
        r = db.instances(s, connectivity=connectivity)
        assert r['n'] == 3 and r['roots'].tolist() == roots and r['sizes'].tolist() == sizes
        assert r['classes'].tolist() == [7, 3, 7] and r['boxes'].tolist() == want_boxes
        got = r['ids'].cpu().numpy()
        want = np.full(shape, -1, np.int32)
        for i, (lo, hi, _) in enumerate(boxes):
            want[tuple(slice(a, b) for a, b in zip(lo, hi))] = i
        assert got.dtype == np.int32 and (got == want).all()
    smallest = int(np.argmin(sizes))
    assert smallest == 2
    r = db.instances(s, min_voxels=sizes[smallest] + 1)
    left = [i for i in range(3) if i != smallest]
    assert r['n'] == 2 and r['roots'].tolist() == [roots[i] for i in left] and r['sizes'].tolist() == [sizes[i] for i in left]
    assert r['classes'].tolist() == [7, 3] and r['boxes'].tolist() == [want_boxes[i] for i in left]
    want[want == smallest] = -1
    assert (r['ids'].cpu().numpy() == want).all()
    # dropping the first renumbers the ones behind it
    r = db.instances(s, min_voxels=sizes[1] + 1)
    assert r['n'] == 1 and r['classes'].tolist() == [7] and r['roots'].tolist() == [roots[0]]
    got = r['ids'].cpu().numpy()
    assert (got[want == 0] == 0).all() and (got[want != 0] == -1).all()
