"""CPU: the definition of the resample operator (csrc/ojf_resample.hip) as tests/resample_ref.py restates it - its exact cases
against plain numpy, the plane bound, the host composition of M and c, every ValueError of resample.py, and the two entry
points refusing malformed arguments without a device."""
import ctypes

import numpy as np
import pytest

from online_joint_depthfusion_and_semantic_amd import _lib, resample
import resample_ref as ref

H, F = np.float16, np.float32


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16) if a.dtype == H else a


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    n_bad = int((g != w).sum())
    assert n_bad == 0, '{}: {} of {} values differ'.format(what, n_bad, g.size)


def shifted_copy(vol, observed, shift, dst_shape, fill):
    """dst[p] = vol[p + shift] where that voxel exists and is observed, else fill: plain numpy slicing."""
    out = np.full(dst_shape, fill, vol.dtype)
    lo = [max(0, -s) for s in shift]
    hi = [min(d, n - s) for d, n, s in zip(dst_shape, vol.shape, shift)]
    if all(h > l for l, h in zip(lo, hi)):
        d = tuple(slice(l, h) for l, h in zip(lo, hi))
        s = tuple(slice(l + sh, h + sh) for l, h, sh in zip(lo, hi, shift))
        out[d] = np.where(observed[s], vol[s], out[d])
    return out


# ---- 1. the exact cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('res', [0.25, 0.05])  # (0.05: the f64 composition is off an integer by rounding, its fp32 value is not)
def test_whole_voxel_shift_is_a_copy_of_the_observed_overlap(res):
    src_shape, dst_shape, shift = (11, 15, 21), (13, 9, 37), (3, -2, 5)
    s = ref.random_scene(src_shape)
    o_s = np.array([-0.4, 0.3, 1.1])
    M, c = resample.compose(o_s, res, o_s + res * np.array(shift), res)
    assert np.array_equal(M.astype(F).reshape(3, 3), np.eye(3, dtype=F)) and np.array_equal(c.astype(F), np.array(shift, F))
    out = ref.resample_volumes(s, M, c, dst_shape, init_value=ref.INIT)
    obs = s['weights'] > 0
    assert 0.25 < 1 - obs.mean() < 0.42
    for key, fill in (('tsdf', H(ref.INIT)), ('weights', 0), ('ids', 0), ('scores', 0)):
        _same(out[key], shifted_copy(s[key], obs, shift, dst_shape, fill), key)
    # the ground-truth form: every voxel of the overlap
    gt = ref.resample_volumes({'tsdf': s['tsdf']}, M, c, dst_shape, init_value=ref.INIT)
    _same(gt['tsdf'], shifted_copy(s['tsdf'], np.ones(src_shape, bool), shift, dst_shape, H(ref.INIT)), 'gt tsdf')
    rec = ref.random_records(src_shape, 8, 5)
    got = ref.resample_records(rec, 5, M, c, dst_shape)
    for k in range(6):
        _same(got[..., k], shifted_copy(rec[..., k], rec[..., 5] > 0, shift, dst_shape, 0), 'record channel {}'.format(k))
    assert not got[..., 6:].any()


def test_quarter_turn_is_rot90():
    src_shape, res = (11, 15, 21), 0.25
    s = ref.random_scene(src_shape, unobserved=0.0)
    T = np.array([[0.0, 1, 0, 0], [-1.0, 0, 0, 15 * res], [0, 0, 1.0, 0]])  # destination (i,j,k) reads source (j, 14 - i, k)
    M, c = resample.compose(np.zeros(3), res, np.zeros(3), res, T)
    assert np.array_equal(c, [0.0, 14.0, 0.0])
    out = ref.resample_volumes(s, M, c, (15, 11, 21), init_value=ref.INIT)
    for key in ('tsdf', 'weights', 'ids', 'scores'):
        _same(out[key], np.rot90(s[key], 1, axes=(0, 1)), key)


def test_half_resolution_is_the_mean_of_the_eight_children():
    s = ref.random_scene((12, 10, 14), unobserved=0.0, labels=False)
    res = 0.125
    M, c = resample.compose(np.zeros(3), res, np.zeros(3), 2 * res)
    assert np.array_equal(M.reshape(3, 3), 2 * np.eye(3)) and np.array_equal(c, [0.5, 0.5, 0.5])
    out = ref.resample_volumes(s, M, c, (6, 5, 7), init_value=ref.INIT)
    for key in ('tsdf', 'weights'):
        v = s[key].astype(F)
        acc, ws = np.zeros((6, 5, 7), F), np.zeros((6, 5, 7), F)
        for bx, by, bz in ref.CORNERS:
            acc = acc + F(0.125) * v[bx::2, by::2, bz::2]
            ws = ws + F(0.125)
        _same(out[key], (acc / ws).astype(H), key)


def test_half_voxel_offsets_tie_and_sit_on_the_threshold():
    """An offset of exactly half a voxel on 1, 2 and 3 axes: the 2, 4, 8 corners with tw > 0 tie - the label is the first of them
    that is observed - and with half of the weight unobserved ws is exactly 0.5: covered."""
    shape, res = (6, 6, 6), 0.5
    s = ref.random_scene(shape, unobserved=0.0)
    s['weights'][:, :, 1::2] = 0  # odd z unobserved
    for axes in ((2,), (1, 2), (0, 1, 2)):
        off = np.zeros(3)
        off[list(axes)] = 0.5 * res
        M, c = resample.compose(np.zeros(3), res, off, res)
        out = ref.resample_volumes(s, M, c, shape, init_value=ref.INIT)
        inner = tuple(slice(0, 5) if a in axes else slice(None) for a in range(3))
        assert (out['weights'][inner] > 0).all()  # ws == 0.5 exactly on every voxel with all its corners in the grid
        # the winner: corner 000 where its z is even, else the corner one step along z (odd z + 1 is even)
        i, j, k = np.meshgrid(*[np.arange(5 if a in axes else 6) for a in range(3)], indexing='ij')
        kk = np.where(k % 2 == 0, k, k + 1)
        _same(out['ids'][inner], s['ids'][i, j, kk], 'ids {}'.format(axes))
        _same(out['scores'][inner], s['scores'][i, j, kk], 'scores {}'.format(axes))


def test_edges_of_the_index_range():
    """g exactly on -1, 0, N-1 and N along z: -1 and N have a corner weight of 0 on the only in-grid side: uncovered; 0 and N-1
    copy the edge voxels; past them nothing is covered.  A destination entirely outside is all init_value / 0."""
    s = ref.random_scene((4, 4, 8), unobserved=0.0)
    res = 0.25
    M, c = resample.compose(np.zeros(3), res, np.array([0, 0, -1.0 * res]), res)
    out = ref.resample_volumes(s, M, c, (4, 4, 10), init_value=ref.INIT)  # g_z = -1 .. 8
    _same(out['tsdf'][:, :, 1:9], s['tsdf'], 'inside')
    for k in (0, 9):
        assert (out['weights'][:, :, k] == 0).all() and (out['tsdf'][:, :, k] == H(ref.INIT)).all()
    M, c = resample.compose(np.zeros(3), res, np.array([40.0, 0, 0]), res)
    out = ref.resample_volumes(s, M, c, (3, 3, 3), init_value=ref.INIT)
    assert (out['tsdf'] == H(ref.INIT)).all() and not out['weights'].any() and not out['ids'].any() and not out['scores'].any()


def test_the_smallest_weight_survives():
    """The source weight that could round to +0: 2^-24, the smallest fp16.  W' is a convex combination of the counting corners'
    weights, all >= 2^-24, so it rounds to 2^-24 again (the next fp16 down is 0, the halfway point 2^-25): the voxel stays
    covered with its weight bits 1, under an identity and under fractional offsets.  (The "+0 is uncovered" clause of step 6 is
    the guard that makes merge == combine(replace) hold by construction; no source reaches it.)"""
    s = ref.random_scene((4, 4, 8), unobserved=0.0)
    s['weights'][...] = H(2.0 ** -24)
    s['weights'][:, :, 1::2] = 0
    res = 0.25
    for off, covered_odd in ((0.0, False), (0.25, False), (0.5, True)):  # ws on odd z: 0, 0.25, 0.5
        M, c = resample.compose(np.zeros(3), res, np.array([0.3 * res, 0, off * res]), res)
        out = ref.resample_volumes(s, M, c, (3, 4, 7), init_value=ref.INIT)
        assert (out['weights'][:, :, 0::2].view(np.uint16) == 1).all()
        assert (out['weights'][:, :, 1::2].view(np.uint16) == (1 if covered_odd else 0)).all()
        assert ((out['tsdf'] == H(ref.INIT)) | (out['weights'] > 0)).all()


# ---- 2. linear precision -------------------------------------------------------------------------------------------------------
def plane_case():
    n, d = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8]), 0.35
    s_shape, s_origin, s_res = (24, 20, 28), np.array([-1.0, -0.8, -0.2]), 0.08
    d_shape, d_res = (19, 23, 17), 0.1
    idx = np.stack(np.meshgrid(*[np.arange(m) for m in s_shape], indexing='ij'), axis=-1)
    Fs = ((s_origin + (idx + 0.5) * s_res) @ n - d)
    src = {'tsdf': Fs.astype(H), 'weights': np.ones(s_shape, H)}
    T = ref.about_centre(ref.rotation(ref.SKEW_AXIS, 0.3), s_origin, s_res, s_shape, shift=(0.05, -0.03, 0.02))
    d_origin = s_origin + np.array([0.1, -0.15, 0.3])
    M, c = resample.compose(s_origin, s_res, d_origin, d_res, T)
    didx = np.stack(np.meshgrid(*[np.arange(m) for m in d_shape], indexing='ij'), axis=-1)
    xs = (d_origin + (didx + 0.5) * d_res) @ T[:, :3].T + T[:, 3]  # destination centres in the source world
    return src, M, c, d_shape, xs @ n - d, float(np.abs(Fs).max()), s_shape


def plane_check(out, M, c, d_shape, want, fmax, s_shape):
    g = ref.index_coordinates(M, c, d_shape)
    inner = np.ones(d_shape, bool)
    for a in range(3):
        inner &= (g[a] >= 0) & (g[a] <= F(s_shape[a] - 1))
    assert inner.sum() > 1000
    assert (out['weights'][inner] > 0).all(), 'a voxel with all corners in the grid is not covered'
    err = float(np.abs(out['tsdf'].astype(np.float64) - want)[inner].max())
    return err, 2.0 ** -10 * fmax


def test_plane_is_reproduced_within_two_half_ulps():
    """Half an ulp of fp16 on the inputs and half on the output, each <= 2^-11 max|F|, under a convex combination; the fp32 terms
    are three orders smaller.  Every voxel with g in [0, N-1] on all axes is in the set."""
    src, M, c, d_shape, want, fmax, s_shape = plane_case()
    out = ref.resample_volumes(src, M, c, d_shape, init_value=ref.INIT)
    err, bound = plane_check(out, M, c, d_shape, want, fmax, s_shape)
    print('plane: max error {:.3e}, bound {:.3e}'.format(err, bound))
    assert err <= bound


# ---- 3. the host composition -------------------------------------------------------------------------------------------------
def test_compose_against_direct_evaluation():
    o_s, r_s, o_d, r_d = np.array([0.3, -1.2, 2.0]), 0.04, np.array([-0.5, 0.25, 1.5]), 0.07
    R = ref.rotation(ref.SKEW_AXIS, np.deg2rad(17.0))
    t = np.array([0.2, -0.1, 0.05])
    for T in (np.concatenate([R, t[:, None]], axis=1), np.vstack([np.concatenate([R, t[:, None]], axis=1), [0, 0, 0, 1.0]])):
        M, c = resample.compose(o_s, r_s, o_d, r_d, T)
        assert M.dtype == np.float64 and M.shape == (9,) and c.shape == (3,)
        for v in ((0, 0, 0), (5, 1, 9), (100, 37, 2), (511, 511, 511)):
            x_d = o_d + (np.array(v) + 0.5) * r_d
            g = (R @ x_d + t - o_s) / r_s - 0.5
            assert np.abs(M.reshape(3, 3) @ np.array(v, np.float64) + c - g).max() <= 1e-9 * (1 + np.abs(g).max())
    M, c = resample.compose(o_s, r_s, o_s, r_s)
    assert np.array_equal(M.reshape(3, 3), np.eye(3)) and np.abs(c).max() < 1e-12
    import torch
    M2, c2 = resample.compose(torch.tensor(o_s), r_s, torch.tensor(o_d), r_d, torch.tensor(T))
    assert np.array_equal(M2, M2) and np.array_equal(resample.compose(o_s, r_s, o_d, r_d, T)[1], c2)


# ---- 4. ValueErrors ----------------------------------------------------------------------------------------------------------
def test_value_errors():
    import torch
    ok = dict(src_origin=np.zeros(3), src_resolution=0.1, dst_origin=np.zeros(3), dst_resolution=0.1)
    R = ref.rotation(ref.SKEW_AXIS, 0.3)
    bad_R = R.copy()
    bad_R[0, 0] += 1e-4
    nan_T = np.concatenate([R, [[np.nan], [0], [0]]], axis=1)
    for kw in (dict(ok, src_resolution=0.0), dict(ok, dst_resolution=-1.0), dict(ok, dst_resolution=np.inf), dict(ok, src_resolution=np.nan),
               dict(ok, dst_origin=np.array([np.inf, 0, 0])), dict(ok, src_origin=np.array([0, np.nan, 0])),
               dict(ok, src_origin=np.zeros(2)), dict(ok, transform=np.concatenate([bad_R, np.zeros((3, 1))], axis=1)),
               dict(ok, transform=np.concatenate([2 * R, np.zeros((3, 1))], axis=1)), dict(ok, transform=nan_T),
               dict(ok, transform=np.eye(3)), dict(ok, src_resolution=1e-320, dst_resolution=1e300)):
        with pytest.raises(ValueError):
            resample.compose(**kw)
    resample.compose(**dict(ok, transform=np.concatenate([R, np.ones((3, 1))], axis=1)))

    # resample_scene: everything below is refused before a device is asked for
    host = {'tsdf': np.zeros((4, 4, 4), H), 'weights': np.zeros((4, 4, 4), H)}
    kw = dict(ok, dst_shape=(4, 4, 4), init_value=0.1)
    with pytest.raises(ValueError, match='to_torch'):
        resample.resample_scene(host, **kw)
    with pytest.raises(ValueError, match='to_torch'):
        resample.resample_scene({k: torch.from_numpy(v) for k, v in host.items()}, **kw)
    for src in ({}, {'n_classes': 5}, {'weights': host['weights']}, {'tsdf': host['tsdf'], 'bogus': 1}, [host['tsdf']]):
        with pytest.raises(ValueError):
            resample.resample_scene(src, **kw)


def test_value_errors_of_the_box(monkeypatch):
    """dst_shape, init_value, max_weight and the consistency of the dicts, with meta tensors standing in for device volumes."""
    import torch

    class FakeCuda(torch.Tensor):  # a host tensor that says it is on the device: nothing below may reach a kernel
        is_cuda = True

    def vol(*shape, dtype=torch.float16):
        return torch.zeros(shape, dtype=dtype).as_subclass(FakeCuda)
    monkeypatch.setattr(_lib, 'require_gpu', lambda: (_ for _ in ()).throw(AssertionError('reached the device')))
    ok = dict(src_origin=np.zeros(3), src_resolution=0.1, dst_origin=np.zeros(3), dst_resolution=0.1, dst_shape=(4, 4, 4), init_value=0.1)
    geo = {'tsdf': vol(4, 4, 4), 'weights': vol(4, 4, 4)}
    for kw in (dict(ok, dst_shape=(4, 0, 4)), dict(ok, dst_shape=(4, 4)), dict(ok, dst_shape=(4, -1, 4)), dict(ok, dst_shape=5),
               dict(ok, init_value=np.nan), dict(ok, max_weight=0.5), dict(ok, max_weight=1e6), dict(ok, max_weight=np.nan)):
        with pytest.raises(ValueError):
            resample.resample_scene(geo, **kw)
    for src in (dict(geo, ids=vol(4, 4, 4, dtype=torch.uint8)), dict(geo, scores=vol(4, 4, 4)), dict(geo, weights=vol(4, 4, 5)),
                dict(geo, tsdf=vol(4, 4, 4, dtype=torch.float32)), dict(geo, colors=vol(4, 4, 4, 3)), dict(geo, label_probs=vol(4, 4, 4, 8)),
                dict(geo, label_probs=vol(4, 4, 4, 8), n_classes=9), dict(geo, label_probs=vol(4, 4, 4, 8), n_classes=1),
                dict(geo, tsdf=vol(4, 4, 8)[:, :, ::2]), dict(geo, colors=vol(4, 4, 4))):
        with pytest.raises(ValueError):
            resample.resample_scene(src, **ok)
    # merge: the destination must mirror the source
    for into in ({'tsdf': vol(4, 4, 4)}, dict(geo, colors=vol(4, 4, 4, 4)), {'tsdf': vol(4, 4, 5), 'weights': vol(4, 4, 5)}):
        with pytest.raises(ValueError):
            resample.resample_scene(geo, into=into, **ok)
    with pytest.raises(ValueError, match='weight'):
        resample.resample_scene({'tsdf': vol(4, 4, 4)}, into={'tsdf': vol(4, 4, 4)}, **ok)
    with pytest.raises(AssertionError, match='reached the device'):  # the well-formed call is what gets that far
        resample.resample_scene(geo, **ok)


# ---- 5. the entry points without a device ------------------------------------------------------------------------------------
def test_entry_points_refuse_malformed_arguments_without_a_device():
    lib = _lib.load()
    host = ctypes.create_string_buffer(1 << 16)  # "device" addresses nothing reads
    base = (ctypes.addressof(host) + 63) & ~63
    n = 8 * 8 * 8
    M, c = np.eye(3).reshape(9).copy(), np.zeros(3)
    good = dict(st=base, sw=base + 2 * n, si=base + 4 * n, ss=base + 5 * n, s=(8, 8, 8), dt=base + 8 * n, dw=base + 10 * n, di=base + 12 * n,
                ds=base + 13 * n, d=(8, 8, 8), M=M.ctypes.data, c=c.ctypes.data, init=0.1, mode=_lib.RESAMPLE_REPLACE, mw=64.0)

    def volumes(a):
        return lib.ojf_resample_volumes(a['st'], a['sw'], a['si'], a['ss'], *a['s'], a['dt'], a['dw'], a['di'], a['ds'], *a['d'], a['M'], a['c'],
                                        a['init'], a['mode'], a['mw'], None)
    nanM, infc, hugeM = M.copy(), c.copy(), M.copy()
    nanM[4], infc[1], hugeM[0] = np.nan, np.inf, 1e300  # (1e300 is finite as f64 and +inf as fp32)
    cases = [(dict(st=None), b'null'), (dict(dt=None), b'null'), (dict(M=None), b'null'), (dict(c=None), b'null'),
             (dict(dw=None), b'weights'), (dict(sw=None), b'weights'), (dict(si=None), b'all set or all NULL'),
             (dict(ds=None), b'all set or all NULL'), (dict(s=(8, 0, 8)), b'non-positive'), (dict(d=(8, 8, -1)), b'non-positive'),
             (dict(s=(2048, 2048, 2048)), b'too large'), (dict(dt=base + 2), b'overlap'), (dict(dw=base + 4 * n - 2), b'overlap'),
             (dict(di=base + n), b'overlap'), (dict(M=nanM.ctypes.data), b'non-finite'), (dict(c=infc.ctypes.data), b'non-finite'),
             (dict(M=hugeM.ctypes.data), b'non-finite'), (dict(mode=2), b'mode'), (dict(mode=-1), b'mode'), (dict(mw=0.5), b'max_weight'),
             (dict(mw=float('inf')), b'max_weight'), (dict(mw=float('nan')), b'max_weight'), (dict(init=float('nan')), b'init_value'),
             (dict(st=base + 1), b'aligned'), (dict(mode=_lib.RESAMPLE_MERGE, sw=None, dw=None), b'merge')]
    for fault, word in cases:
        assert volumes(dict(good, **fault)) != 0, fault
        msg = lib.ojf_last_error()
        assert msg.startswith(b'ojf_resample_volumes:') and word in msg, (fault, msg)

    rgood = dict(src=base, s=(4, 4, 4), dst=base + (1 << 15), d=(4, 4, 4), S=32, Cw=30, M=M.ctypes.data, c=c.ctypes.data,
                 mode=_lib.RESAMPLE_REPLACE, mw=64.0)

    def records(a):
        return lib.ojf_resample_records(a['src'], *a['s'], a['dst'], *a['d'], a['S'], a['Cw'], a['M'], a['c'], a['mode'], a['mw'], None)
    rcases = [(dict(src=None), b'null'), (dict(dst=None), b'null'), (dict(M=None), b'null'), (dict(s=(0, 4, 4)), b'non-positive'),
              (dict(S=12), b'S must'), (dict(S=0), b'S must'), (dict(S=272), b'S must'), (dict(Cw=0), b'Cw'), (dict(Cw=32), b'Cw'),
              (dict(src=base + 8), b'aligned'), (dict(dst=base + (1 << 15) + 2), b'aligned'), (dict(S=4, Cw=3, src=base + 1), b'aligned'),
              (dict(dst=base + 64), b'overlap'), (dict(M=nanM.ctypes.data), b'non-finite'), (dict(c=infc.ctypes.data), b'non-finite'),
              (dict(mode=7), b'mode'), (dict(mw=70000.0), b'max_weight')]
    for fault, word in rcases:
        assert records(dict(rgood, **fault)) != 0, fault
        msg = lib.ojf_last_error()
        assert msg.startswith(b'ojf_resample_records:') and word in msg, (fault, msg)


# ---- 6. merge == combine(dst, replace) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('max_weight', [65504.0, 30.0])  # 30: reached by most sums of two weights up to 40
def test_merge_is_replace_then_combine(max_weight):
    src_shape, dst_shape, res = (11, 15, 21), (13, 9, 17), 0.05
    s, d = ref.random_scene(src_shape, seed=1), ref.random_scene(dst_shape, seed=2)
    T = ref.about_centre(ref.rotation(ref.SKEW_AXIS, np.deg2rad(17.0)), np.zeros(3), res, src_shape)
    M, c = resample.compose(np.zeros(3), res, np.array([-0.05, 0.1, 0.02]), 0.8 * res, T)
    scratch = ref.resample_volumes(s, M, c, dst_shape, init_value=ref.INIT)
    covered = scratch['weights'] > 0
    assert 0.2 < covered.mean() < 0.95
    want = ref.combine_volumes({k: v.copy() for k, v in d.items()}, scratch, max_weight)
    got = ref.resample_volumes(s, M, c, dst_shape, init_value=ref.INIT, into={k: v.copy() for k, v in d.items()}, max_weight=max_weight)
    for k in want:
        _same(got[k], want[k], k)
        _same(got[k][~covered], d[k][~covered], k + ' where nothing is covered')
    assert (got['weights'] == H(max_weight)).any() == (max_weight == 30.0)
    assert (got['ids'] != d['ids']).any() and (got['ids'][covered] == d['ids'][covered]).any()  # some scores beat, some do not
    for S, Cw in ((4, 3), (8, 5)):
        rs, rd = ref.random_records(src_shape, S, Cw, seed=1), ref.random_records(dst_shape, S, Cw, seed=2)
        scratch = ref.resample_records(rs, Cw, M, c, dst_shape)
        want = ref.combine_records(rd.copy(), scratch, Cw, 6.0)
        got = ref.resample_records(rs, Cw, M, c, dst_shape, into=rd.copy(), max_weight=6.0)
        _same(got, want, 'records S={}'.format(S))
        assert (got.view(np.uint16)[..., Cw + 1:] == ref.PAD_BITS).all() and (got[..., Cw] == H(6.0)).any()
