"""CPU: the relocalisation definition as tests/reloc_ref.py restates it - the packed nibble count, the half-valid rule, strict
thresholds, the order of insert - and, as a condition on the definition itself, that the fern codes retrieve the right
keyframes on the synthetic orbit."""
import numpy as np
import pytest

from online_joint_depthfusion_and_semantic_amd import synthetic
from online_joint_depthfusion_and_semantic_amd.relocalize import fern_table
import reloc_ref


def test_packed_count_is_the_per_fern_count():
    rng = np.random.default_rng(5)
    for M in (8, 512, 1000, 4096):
        a = rng.integers(0, 16, (20, M)).astype(np.uint8)
        b = np.where(rng.random((20, M)) < 0.7, a, rng.integers(0, 16, (20, M))).astype(np.uint8)
        pa, pb = np.stack([reloc_ref.pack(x) for x in a]), np.stack([reloc_ref.pack(x) for x in b])
        assert pa.shape == (20, M // 8) and pa.dtype == np.uint32
        for i in range(20):
            assert np.array_equal(reloc_ref.unpack(pa[i]), a[i])
            assert reloc_ref.differ(pa[i], pb[i]) == int((a[i] != b[i]).sum()) == int(reloc_ref.differ_packed(pa[i], pb[i]))
            assert reloc_ref.differ(pa[i], pa[i]) == 0 == int(reloc_ref.differ_packed(pa[i], pa[i]))
        assert np.array_equal(reloc_ref.differ_packed(pa[0], pb), [(a[0] != b[i]).sum() for i in range(20)])
    # fern m sits in word m / 8 at bits 4 * (m % 8)
    nib = np.zeros(16, np.uint8)
    nib[9] = 0xb
    assert reloc_ref.pack(nib).tolist() == [0, 0xb0]


def test_fern_table_is_reproducible_and_the_depth_draws_come_first():
    a, b = fern_table(1911, 512, 192), fern_table(1911, 512, 192)
    for key in ('cell', 'channel', 'threshold'):
        assert np.array_equal(a[key], b[key])
    assert a['cell'].dtype == np.int32 and a['channel'].dtype == np.uint8 and a['threshold'].dtype == np.float32
    assert a['cell'].shape == a['channel'].shape == a['threshold'].shape == (512, 4)
    assert a['cell'].min() >= 0 and a['cell'].max() < 192 and a['cell'].max() > 150 and not a['channel'].any()
    assert a['threshold'].min() >= 0.2 and a['threshold'].max() <= 4.0
    c = fern_table(1911, 512, 192, color=True)
    assert np.array_equal(c['cell'], a['cell'])
    depth_rows = c['channel'] == 0
    assert 0.15 < depth_rows.mean() < 0.35 and c['channel'].max() == 3
    assert np.array_equal(c['threshold'][depth_rows], a['threshold'][depth_rows])
    assert c['threshold'][~depth_rows].max() > 200 and c['threshold'][~depth_rows].min() >= 0.0
    assert not np.array_equal(fern_table(1912, 512, 192)['cell'], a['cell'])
    r = np.random.default_rng(1911)  # the draws of the definition, in order
    assert np.array_equal(r.integers(0, 192, (512, 4)), a['cell'])
    assert np.array_equal(r.uniform(0.2, 4.0, (512, 4)).astype(np.float32), a['threshold'])
    for bad in (dict(n_ferns=12), dict(n_ferns=0), dict(n_ferns=4104), dict(cells=0)):
        with pytest.raises(ValueError):
            fern_table(**dict(dict(seed=1, n_ferns=8, cells=4), **bad))


def test_half_valid_rule_and_pixel_validity():
    c = 4
    depth = np.full((4, 8), 1.5, np.float32)
    depth[:2, :4] = 0.0  # 8 of 16 valid: 2n == c^2
    depth[:2, 4:] = 0.0
    depth[2, 4] = np.nan  # 7 of 16
    values, ok = reloc_ref.code_image(depth, None, None, c)
    assert ok.tolist() == [[True, False]] and values[0, 0, 0] == np.float32(1.5) and values[0, 0, 1] == 0.0
    assert not values[1:].any()
    # what counts as a valid pixel
    d = np.array([[np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0, 1e-42, 64.0, np.nextafter(np.float32(64), np.float32(0)), 2.0]], np.float32)
    valid, q = reloc_ref.quantise(d)
    assert valid.tolist() == [[False] * 6 + [True, False, True, True]]
    assert q.tolist() == [[0] * 6 + [0, 0, 65536, 2048]]
    valid, _ = reloc_ref.quantise(d, np.array([[1] * 8 + [0, 7]], np.uint8))
    assert valid.tolist() == [[False] * 6 + [True, False, False, True]]
    # trailing rows and columns are ignored; the mean is of the quantised depths
    depth = np.full((7, 9), 100.0, np.float32)
    depth[:6, :8] = np.float32(1.00049)  # q = 1025 (1024.50...)
    values, ok = reloc_ref.code_image(depth, None, None, 2)
    assert values.shape == (4, 3, 4) and ok.all() and (values[0] == np.float32(1025 / 1024)).all()


def test_threshold_is_strict_and_channel_zero_needs_a_valid_cell():
    values = np.zeros((4, 1, 2), np.float32)
    values[0, 0, 0], values[2, 0, 1] = 1.5, 100.0
    ok = np.array([[True, False]])
    table = {'cell': np.array([[0, 0, 0, 1]] * 8, np.int32), 'channel': np.array([[0, 0, 0, 2]] * 8, np.uint8),
             'threshold': np.array([[1.5, np.nextafter(np.float32(1.5), np.float32(0)), np.nan, 100.0]] * 8, np.float32)}
    assert reloc_ref.fern_bits(values, ok, table).tolist() == [0b0010] * 8
    # an invalid cell: channel 0 gives 0 even below the value, a colour channel does not ask
    table = {'cell': np.array([[1, 1, 0, 5]] * 8, np.int32), 'channel': np.array([[0, 2, 0, 0]] * 8, np.uint8),
             'threshold': np.array([[-1.0, 99.0, -1.0, -1.0]] * 8, np.float32)}
    assert reloc_ref.fern_bits(values, ok, table).tolist() == [0b0110] * 8


def test_insert_order_force_and_capacity():
    rng = np.random.default_rng(3)
    code = rng.integers(0, 2 ** 32, (1, 64), dtype=np.uint32)
    two = np.concatenate([code, code])
    poses = rng.standard_normal((2, 12))
    s = reloc_ref.Store(4, 64)
    best, flags = s.insert(two, poses, min_differ=51)
    assert flags.tolist() == [1, 0] and s.count == 1
    assert best[0] == reloc_ref.NO_KEY and best[1] == 0  # the second meets the first: 0 ferns differ, keyframe 0
    s = reloc_ref.Store(4, 64)
    best, flags = s.insert(two, poses, min_differ=51, force=True)
    assert flags.tolist() == [1, 1] and s.count == 2 and np.array_equal(s.poses[:2], poses)
    other = rng.integers(0, 2 ** 32, (3, 64), dtype=np.uint32)
    best, flags = s.insert(other, rng.standard_normal((3, 12)), min_differ=51)
    assert flags.tolist() == [1, 1, 2] and s.count == 4
    before = (s.codes.copy(), s.poses.copy())
    best, flags = s.insert(np.concatenate([other[2:], code]), rng.standard_normal((2, 12)), min_differ=51)
    assert flags.tolist() == [2, 0] and s.count == 4 and np.array_equal(before[0], s.codes) and np.array_equal(before[1], s.poses)
    assert best[1] == 0  # equal codes: the smallest index
    # query: ascending, ties smallest index first, all-ones beyond the count
    keys = reloc_ref.query(code[0], s.codes, s.count, 6)
    assert keys[0] == 0 and keys[1] == 1 and (keys[4:] == reloc_ref.NO_KEY).all() and (np.diff(keys[:4].astype(np.float64)) > 0).all()
    assert (reloc_ref.query(code[0], s.codes, 0, 2) == reloc_ref.NO_KEY).all()


@pytest.mark.parametrize('h,w,cell', [(48, 64, 4), (240, 320, 20)])
def test_retrieval_on_the_synthetic_orbit(h, w, cell):
    """Frames 0..79 of the 400-frame orbit (1.4 cm / 1 degree apart), keyframes every 4th, 512 depth-only ferns."""
    st = synthetic.SyntheticStream(h, w, 64, 400)
    table = fern_table(1911, 512, (h // cell) * (w // cell))
    codes = []
    for i in range(80):
        f = st.frame(i)
        codes.append(reloc_ref.encode(f['tof_depth'], f['mask'], None, cell, table)[0])
    codes = np.stack(codes)
    key_frames = np.arange(0, 80, 4)
    held_out = [i for i in range(80) if i % 4]
    off, margins = [], []
    for i in held_out:
        d = reloc_ref.differ_packed(codes[i], codes[key_frames])
        top = int(np.argmin(d))  # (the first of equal counts: the smallest index, as the key orders them)
        off.append(abs(int(key_frames[top]) - i))
        far = np.abs(key_frames - i) > 8
        margins.append(int(d[far].min() - d[top]))
    off = np.array(off)
    print('{}x{}: worst top-1 {} frames away, {} of {} within 2, margin >= {}'.format(h, w, off.max(), int((off <= 2).sum()), len(off),
                                                                                       min(margins)))
    assert off.max() <= 3
    assert int((off > 2).sum()) <= 1
    assert min(margins) >= 20
    # harvesting: fewer keyframes as the threshold rises; every frame is a keyframe or within the threshold of one
    counts = []
    for share in (0.05, 0.1):
        min_differ = int(np.floor(share * 512))
        s = reloc_ref.Store(128, 64)
        _, flags = s.insert(codes, np.zeros((80, 12)), min_differ)
        assert set(flags.tolist()) == {0, 1} and flags[0] == 1 and s.count == int(flags.sum())
        for i in range(80):
            assert flags[i] == 1 or reloc_ref.differ_packed(codes[i], s.codes[:s.count]).min() <= min_differ
        counts.append(s.count)
    print('harvested keyframes at 0.05 / 0.1: {}'.format(counts))
    assert counts[0] > counts[1] >= 1
