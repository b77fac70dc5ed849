"""GPU: the pool pyramid launch of the fusion net (ojf_pool_pyramid: the product kernel under the product grid rule, on caller-supplied
buffers) equals its numpy restatement (tests/pool_pyramid_ref.py) bit for bit - the pools at the smallest frames that reach each edge
of the 32x8 tiling, the fold of the global-average branch (one block of the same launch) at the two channel counts the nets run it at."""
import functools

import numpy as np
import pytest
import torch

from online_joint_depthfusion_and_semantic_amd import _lib
import pool_pyramid_ref as ref

pytestmark = pytest.mark.gpu

C4 = 2  # channel groups per branch: block rows [0, C4) run three levels, [C4, 2 C4) two, [2 C4, 3 C4) one, [3 C4, 4 C4) none (Z2)
BIAS_LEN = 128

# (h, w, with Z2): the smallest frames that reach each edge
FRAMES = [
    (1, 40, False), (40, 1, False),  # the halo is wider than the frame
    (8, 32, False),                  # exactly one tile
    (9, 33, False),                  # four ragged tiles, every tile edge beside a frame border
    (17, 70, False),                 # an interior tile whose halo lies wholly in other tiles
    (8, 224, False),                 # 7 tiles: with the fold, its block is the last block of the row
    (8, 256, False),                 # 8 tiles: the fold block is followed by seven padding blocks
    (9, 33, True),                   # the lv == 4 row on a ragged frame
]


@functools.lru_cache(maxsize=None)
def fold_case(name):
    """-> dict of host arrays: fix, bad, wg_t, bg, wfg_t, bf (seeded; shared, never modified)"""
    rng = np.random.default_rng(11)
    cphys, c_out = (232, 114) if name == 'c232' else (116, 114)
    fix = np.zeros((ref.SHARDS, ref.COL_MAX), np.int64)
    fix[:, :cphys] = rng.integers(-2 ** 38, 2 ** 38, size=(ref.SHARDS, cphys), dtype=np.int64)  # |channel sum| up to ~4e6
    bad = np.zeros(ref.COL_MAX, np.uint32)
    if name == 'bad':
        bad[57] = 1
    if name == 'zero':
        fix[:, 20] = 0
    wg_t = (rng.standard_normal((cphys, c_out)) * 0.1).astype(np.float32)
    wfg_t = (rng.standard_normal((c_out, c_out)) * 0.1).astype(np.float32)
    bg, bf = rng.standard_normal(c_out).astype(np.float32), rng.standard_normal(c_out).astype(np.float32)
    for a in (fix, bad, wg_t, bg, wfg_t, bf):
        a.setflags(write=False)
    return dict(fix=fix, bad=bad, wg_t=wg_t, bg=bg, wfg_t=wfg_t, bf=bf)


@functools.lru_cache(maxsize=None)
def fold_reference(name, npix):
    c = fold_case(name)
    return ref.fold(c['fix'], c['bad'], npix, c['wg_t'], c['bg'], c['wfg_t'], c['bf'], BIAS_LEN)


def run_launch(cuda, h, w, with_z2, split_out, fold=None, seed=0):
    """One launch on seeded inputs -> (outputs [q1, q2, q3 (, q0)] as host arrays [C4, h, w, 4], the restatement's, bias_out or None,
    the ColSums words after the launch or None)"""
    rng = np.random.default_rng(1000 * h + w + seed)
    z = rng.standard_normal((4 * C4, h, w, 4)).astype(np.float32)
    z2 = rng.standard_normal((4 * C4, h, w, 4)).astype(np.float32) if with_z2 else None
    if not split_out and h * w >= 8:
        # values at the ends of the range in every group: subnormals, -0, sums that overflow to +inf (no -inf: inf - inf would be a NaN,
        # whose payload nothing defines)
        flat, at = z.reshape(4 * C4, h * w, 4), rng.choice(h * w, size=8, replace=False)
        for g in range(4 * C4):
            flat[g, at, g % 4] = np.array([1e-40, -1e-39, 3e38, 2e38, -0.0, 1e-45, 1.5e-38, 65504.0], np.float32)
    biases = [(rng.standard_normal(C4 * 4) * 0.3).astype(np.float32) for _ in range(3)]
    bias0 = (rng.standard_normal(C4 * 4) * 0.3).astype(np.float32) if with_z2 else None
    want = ref.pyramid(z, biases, C4, z2, bias0, bool(split_out))

    def dev(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)

    dz, dz2, db, db0 = dev(z), dev(z2), [dev(b) for b in biases], dev(bias0)
    # outputs start as a pattern no result has: a pixel the launch misses shows
    q = [torch.full((C4, h, w, 4), -7.0, device=cuda) for _ in range(4 if with_z2 else 3)]
    colsums = wg = bg = wfg = bf = bias_out = None
    cphys = c_out = 0
    if fold is not None:
        c = fold_case(fold)
        cphys, c_out = c['wg_t'].shape
        colsums = dev(np.concatenate([c['fix'].reshape(-1).view(np.uint8), c['bad'].view(np.uint8)]))
        wg, bg, wfg, bf = dev(c['wg_t']), dev(c['bg']), dev(c['wfg_t']), dev(c['bf'])
        bias_out = torch.full((BIAS_LEN,), -7.0, device=cuda)
    lib = _lib.load()
    rc = lib.ojf_pool_pyramid(_lib.ptr(dz), _lib.ptr(dz2), _lib.ptr(q[0]), _lib.ptr(q[1]), _lib.ptr(q[2]),
                              _lib.ptr(q[3]) if with_z2 else None, _lib.ptr(db[0]), _lib.ptr(db[1]), _lib.ptr(db[2]), _lib.ptr(db0),
                              h, w, C4, int(split_out), _lib.ptr(colsums), _lib.ptr(wg), _lib.ptr(bg), _lib.ptr(wfg), _lib.ptr(bf),
                              cphys, c_out, _lib.ptr(bias_out), BIAS_LEN if fold is not None else 0, _lib.stream_ptr(cuda))
    _lib.check(rc, 'ojf_pool_pyramid')
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in q]
    return (got, want, None if bias_out is None else bias_out.cpu().numpy(), None if colsums is None else colsums.cpu().numpy())


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize('split_out', [0, 1])
@pytest.mark.parametrize('h,w,with_z2', FRAMES)
def test_pools_equal_the_restatement_bit_for_bit(cuda, h, w, with_z2, split_out):
    """Every frame twice: as plain planes under the general flow's grid (no fold block) and as split planes under the chain flow's grid
    (tiles + 1 block columns, the extra one folding the 116-channel case)."""
    fold = 'c116' if split_out else None
    got, want, bias_out, colsums = run_launch(cuda, h, w, with_z2, split_out, fold)
    for name, g, x in zip(('q1', 'q2', 'q3', 'q0'), got, want):
        wrong = bits(g) != bits(x)
        assert not wrong.any(), (name, int(wrong.sum()), np.argwhere(wrong)[:4].tolist())
    if fold:
        assert (bits(bias_out) == bits(fold_reference(fold, h * w))).all()
        assert not colsums.any()


@pytest.mark.parametrize('name', ['c116', 'c232', 'bad', 'zero'])
def test_fold_equals_the_restatement_bit_for_bit(cuda, name):
    """cphys 116 with c_out 114, cphys 232, one flagged channel (NaN mean: NaN entries exactly where the restatement has them), one
    all-zero channel; the shards and flags read back as zero afterwards.  Frame 8x224: the fold block is the last block of its row."""
    h, w = 8, 224
    _, _, bias_out, colsums = run_launch(cuda, h, w, False, 1, name)
    want = fold_reference(name, h * w)
    assert (np.isnan(bias_out) == np.isnan(want)).all()
    if name == 'bad':
        assert np.isnan(want[:114]).all() and (want[114:] == 0).all()
    else:
        assert not np.isnan(want).any()
    ok = np.isnan(want) | (bits(bias_out) == bits(want))
    assert ok.all(), np.argwhere(~ok)[:8].tolist()
    assert not colsums.any()
