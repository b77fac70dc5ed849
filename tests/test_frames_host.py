"""CPU: the definition of the depth-frame preparation (csrc/ojf_frames.hip) as tests/frames_ref.py restates it - against an
independent float64 brute force, against its limiting cases and analytic surfaces, and for its effect on the noisy synthetic
room - and the refusals of frames.prepare_depth / Pipeline that need no device."""
import math

import numpy as np
import pytest
import torch

from online_joint_depthfusion_and_semantic_amd import frames
from online_joint_depthfusion_and_semantic_amd.config import default_config
from online_joint_depthfusion_and_semantic_amd.pipeline import Pipeline
from online_joint_depthfusion_and_semantic_amd.synthetic import SyntheticStream
import frames_ref as ref

EPS = 2.0 ** -24  # half the spacing of fp32 numbers in [1, 2): the relative error of one rounded fp32 operation


def ulp(x):
    return float(np.spacing(np.float32(x)))


def brute(d, mask, K, radius, sigma, range0, range2, edge_abs, edge_rel, near, far, cos_min):
    """One frame [h,w] in float64 with plain loops over pixels and taps, written from the prose of the definition.  Returns
    (depth, valid, margin): margin is the smallest distance of any compared quantity from its threshold (near, far, the edge
    threshold, cos_min) - validity can only differ from an fp32 evaluation where that distance is within rounding."""
    h, w = d.shape
    margin = [np.inf]

    def cmp_gt(a, b):  # a > b, recording how close the call was (equal fp32 inputs compare the same way in any precision)
        if a != b:
            margin[0] = min(margin[0], abs(a - b))
        return a > b

    v0 = np.zeros((h, w), bool)
    for r in range(h):
        for c in range(w):
            x = float(d[r, c])
            if not math.isfinite(x) or (mask is not None and not mask[r, c]):
                continue
            v0[r, c] = not cmp_gt(near, x) and not cmp_gt(x, far)
    v1 = v0.copy()
    if edge_abs != 0 or edge_rel != 0:
        for r in range(h):
            for c in range(w):
                if not v0[r, c]:
                    continue
                t = edge_abs + edge_rel * float(d[r, c])
                for rr in range(max(r - 1, 0), min(r + 2, h)):
                    for cc in range(max(c - 1, 0), min(c + 2, w)):
                        if (rr, cc) != (r, c) and v0[rr, cc] and cmp_gt(abs(float(d[rr, cc]) - float(d[r, c])), t):
                            v1[r, c] = False
    f = np.zeros((h, w))
    for r in range(h):
        for c in range(w):
            if not v1[r, c]:
                continue
            x = float(d[r, c])
            rho = range0 + range2 * x * x
            num = den = 0.0
            for dr in range(-radius, radius + 1):
                for dc in range(-radius, radius + 1):
                    rr, cc = r + dr, c + dc
                    if not (0 <= rr < h and 0 <= cc < w) or not v1[rr, cc]:
                        continue
                    t = (float(d[rr, cc]) - x) / rho
                    if abs(t) < 1.0:
                        wgt = math.exp(-(dr * dr + dc * dc) / (2.0 * sigma * sigma)) * (1.0 - t * t) ** 2
                        num += wgt * (float(d[rr, cc]) - x)
                        den += wgt
            f[r, c] = x + num / den
    valid = v1.copy()
    if cos_min != 0:
        fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]

        def V(r, c):
            return np.array([(c - cx) / fx * f[r, c], (r - cy) / fy * f[r, c], f[r, c]])

        def diff(r, c, dr, dc):
            p = 0 <= r + dr < h and 0 <= c + dc < w and v1[r + dr, c + dc]
            m = 0 <= r - dr < h and 0 <= c - dc < w and v1[r - dr, c - dc]
            if not p and not m:
                return None
            return (V(r + dr, c + dc) if p else V(r, c)) - (V(r - dr, c - dc) if m else V(r, c))

        for r in range(h):
            for c in range(w):
                if not v1[r, c]:
                    continue
                a, b = diff(r, c, 0, 1), diff(r, c, 1, 0)
                nrm = None if a is None or b is None else np.cross(a, b)
                if nrm is None or not np.linalg.norm(nrm) > 0:
                    valid[r, c] = False
                    continue
                nrm = nrm / np.linalg.norm(nrm)
                cs = abs(float(nrm @ V(r, c))) / float(np.linalg.norm(V(r, c)))  # the flipped normal: -(n.V) = |n.V|
                valid[r, c] = not cmp_gt(cos_min, cs)
    return np.where(valid, f, 0.0), valid, margin[0]


BRUTE_CASES = [
    dict(radius=2, sigma=1.5, range0=0.06, range2=0.0, edge_abs=0.12, edge_rel=0.0, near=0.0, far=np.inf, max_angle=None),
    dict(radius=4, sigma=2.5, range0=0.08, range2=0.004, edge_abs=0.05, edge_rel=0.02, near=0.3, far=4.0, max_angle=None),
    dict(radius=1, sigma=1.0, range0=0.05, range2=0.0, edge_abs=0.0, edge_rel=0.0, near=0.3, far=4.0, max_angle=65.0),
    dict(radius=3, sigma=1.2, range0=0.07, range2=0.001, edge_abs=0.09, edge_rel=0.0, near=0.0, far=np.inf, max_angle=75.0),
]


@pytest.mark.parametrize('case', range(len(BRUTE_CASES)))
def test_restatement_against_float64_brute_force(case):
    """Tolerance.  Inputs are fp32 numbers, so both sides start from the same values.  With depths below 4 m the fp32 result
    f = d + num / den carries: half a spacing of f for the final sum and half a spacing of d for each difference d_n - d
    (together at most ulp(4)); and a relative error of the quotient num / den, a weighted mean of differences |diff| < rho:
    each weight S[k] * (u * u) is the product of a rounded table entry and five rounded operations (t, t * t, u, u * u, the
    product) - at most 8 EPS with the cancellation in u bounded by the weight's own size where it matters - and each of the
    two sums over T taps adds at most T EPS, so the mean moves by at most 2 * (T + 8) * EPS * rho_max.  Validity can differ
    only where a compared quantity lies within rounding of its threshold: the case is built (and checked) to keep every
    comparison at least 1e-5 - forty spacings of a 4 m depth - away from it."""
    o = BRUTE_CASES[case]
    d = ref.surface(1, 13, 19, 5 + case, noise=0.012)
    d, mask = ref.with_bad_pixels(d, case)
    cos_min = ref.cos_min_of(o['max_angle'])
    got = ref.prepare(d, mask, ref.frame_intrinsics(ref.INTRINSICS, 1), o['radius'], ref.spatial_table(o['radius'], o['sigma']), o['range0'],
                      o['range2'], o['edge_abs'], o['edge_rel'], o['near'], o['far'], cos_min, normals=False)
    want, valid, margin = brute(d[0], mask[0], ref.INTRINSICS, o['radius'], o['sigma'], o['range0'], o['range2'], o['edge_abs'],
                                o['edge_rel'], o['near'], o['far'], cos_min)
    assert margin > 1e-5, margin
    assert 0.3 < valid.mean() < 0.95 and (mask[0] & ~valid).any()
    assert np.array_equal(got['valid'][0], valid)
    dmax = float(want.max())
    assert dmax < 4.0
    taps = (2 * o['radius'] + 1) ** 2
    tol = ulp(4.0) + 2 * (taps + 8) * EPS * (o['range0'] + o['range2'] * dmax * dmax)
    err = np.abs(got['depth'][0].astype(np.float64) - want).max()
    print('case {}: max error {:.3e}, tolerance {:.3e}, comparison margin {:.3e}'.format(case, err, tol, margin))
    assert err <= tol


def test_wide_range_kernel_is_the_normalised_spatial_convolution_and_radius_0_the_identity():
    """range0 = 1e6: t = diff / 1e6 is below 1e-6, t * t below 2^-24 / 2, so u = 1 - t * t rounds to 1 and every weight is
    S[k]: f = d + sum S (d_n - d) / sum S over the valid neighbours, the normalised convolution - compared in float64 with
    the tolerance of the brute-force test (rho_max there bounds |diff|; here the largest difference in the image does)."""
    d = ref.surface(2, 11, 17, 3)
    d, mask = ref.with_bad_pixels(d, 3)
    R, sigma = 2, 1.3
    S = ref.spatial_table(R, sigma)
    got = ref.prepare(d, mask, None, R, S, range0=1e6, near=0.3, far=4.0)
    valid = np.isfinite(d) & (d >= 0.3) & (d <= 4.0) & mask
    assert np.array_equal(got['valid'], valid)
    dz = np.where(valid, d, 0).astype(np.float64)
    num, den = np.zeros_like(dz), np.zeros_like(dz)
    k = 0
    for dr in range(-R, R + 1):
        for dc in range(-R, R + 1):
            num += np.float64(S[k]) * ref._shift(dz, dr, dc, 0.0)
            den += np.float64(S[k]) * ref._shift(valid, dr, dc, False)
            k += 1
    want = np.where(valid, num / np.where(valid, den, 1.0), 0.0)
    spread = float(dz[valid].max() - dz[valid].min())
    tol = ulp(4.0) + 2 * (25 + 8) * EPS * spread
    assert np.abs(got['depth'] - want).max() <= tol
    # radius 0: the identity on valid pixels, 0 elsewhere - exactly
    same = ref.prepare(d, mask, None, 0, None, range0=0.05, near=0.3, far=4.0)
    assert np.array_equal(same['valid'], valid) and np.array_equal(same['depth'], np.where(valid, d, np.float32(0)))
    # and with every stage off and no mask, whatever is finite and in range passes unchanged
    raw = ref.prepare(d, None, None, 0, None, range0=0.05)
    ok = np.isfinite(d) & (d >= 0)
    assert np.array_equal(raw['valid'], ok) and np.array_equal(raw['depth'][ok], d[ok]) and not raw['depth'][~ok].any()


def test_normals_of_planes_are_analytic_and_face_the_camera():
    """A fronto-parallel plane z = 2 gives (0, 0, -1) exactly: the differences are (x, 0, 0) and (0, y, 0).  A tilted plane
    n.X = p has depth z = p / (n . ((c - cx) / fx, (r - cy) / fy, 1)) along the pixel's ray, rounded to fp32.  Bound on the
    angle: a vertex coordinate carries at most 4 spacings of the largest depth (half for the rounded depth, two rounded
    products and a rounded intrinsic on |x| <= z, half for the difference that follows, with margin), a difference of two
    vertices 8, over a baseline of at least zmin / fmax metres (one pixel: the one-sided differences at the border); two axes
    enter the cross product, so the angle is below 16 * ulp(zmax) / (zmin / fmax) radians."""
    h, w = 9, 12
    K = ref.INTRINSICS
    K4 = ref.frame_intrinsics(K, 1)
    flat = ref.prepare(np.full((1, h, w), 2.0, np.float32), None, K4, 0, None, range0=0.05, normals=True)
    assert flat['valid'].all() and np.array_equal(flat['normals'], np.broadcast_to(np.float32([0, 0, -1]), (1, h, w, 3)))
    n = np.array([0.35, -0.25, -0.9])
    n /= np.linalg.norm(n)
    r, c = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    ray = np.stack([(c - K[0, 2]) / K[0, 0], (r - K[1, 2]) / K[1, 1], np.ones_like(c)], axis=-1)
    z = (-2.0 / (ray @ n)).astype(np.float32)  # the plane n.X = -2: two metres in front of the camera, n towards it
    assert z.min() > 1.0 and z.max() < 4.0
    out = ref.prepare(z[None], None, K4, 0, None, range0=0.05, normals=True, cos_min=ref.cos_min_of(89.0))
    assert out['valid'].all()
    got = out['normals'][0].astype(np.float64)
    assert np.abs(np.linalg.norm(got, axis=-1) - 1.0).max() <= 4 * EPS
    V = ray * z[..., None].astype(np.float64)
    assert ((got * V).sum(-1) < 0).all()  # faces the camera
    assert (got @ n > 0.99).all()
    angle = np.arcsin(np.linalg.norm(np.cross(got, n), axis=-1)).max()  # (arccos of a dot product near 1 resolves no angle below 3e-4)
    bound = 16 * ulp(z.max()) / (float(z.min()) / max(K[0, 0], K[1, 1]))
    print('largest angle to the analytic normal {:.3e} rad, bound {:.3e}'.format(angle, bound))
    assert angle <= bound
    # the incidence test: this plane is seen under at most ~45 degrees; 20 degrees keeps only the pixels that look along n
    cs = -(ray @ n) / np.linalg.norm(ray, axis=-1)
    cut = ref.prepare(z[None], None, K4, 0, None, range0=0.05, cos_min=ref.cos_min_of(20.0))
    sure = np.abs(cs - math.cos(math.radians(20.0))) > 1e-4
    assert np.array_equal(cut['valid'][0][sure], (cs >= math.cos(math.radians(20.0)))[sure]) and 0 < cut['valid'].mean() < 1


def test_step_image_loses_exactly_the_two_columns_at_the_step():
    h, w, step = 12, 21, 9
    rng = np.random.default_rng(5)
    level = np.where(np.arange(w) >= step, 1.5, 1.0)[None, :].repeat(h, 0)
    d = (level + np.clip(rng.normal(0.0, 0.006, (h, w)), -0.02, 0.02)).astype(np.float32)[None]
    range0 = 0.06
    out = ref.prepare(d, None, None, 2, ref.spatial_table(2, 1.5), range0=range0, edge_abs=0.12)
    want = np.ones((1, h, w), bool)
    want[:, :, step - 1:step + 1] = False
    assert np.array_equal(out['valid'], want)
    assert (np.abs(out['depth'][0] - level)[want[0]] < range0).all() and not out['depth'][~want].any()
    # the filter moved the survivors towards their level, never across the step
    assert np.abs(out['depth'][0] - level)[want[0]].mean() < np.abs(d[0] - level)[want[0]].mean()
    # no cascade: the test reads the validity of the first step, so the columns next to the dropped ones stay
    assert out['valid'][0, :, step - 2].all() and out['valid'][0, :, step + 1].all()


def test_effect_on_the_noisy_synthetic_room():
    """Frames 0, 7 and 13 of the 48 x 64 room with 2 cm depth noise, radius 2, sigma 1.5 px, range width 0.06 m, edge
    threshold 0.12 m; the valid pixels are those of the frame's mask.  Measured with this restatement: mean absolute error
    over the kept pixels 0.01563 m raw, 0.01131 m filtered (ratio 0.724); 95.43 % of the valid pixels kept."""
    st = SyntheticStream(48, 64, 64, 40, noise_sigma=0.02)
    raw = fil = kept = valid = 0.0
    for i in (0, 7, 13):
        fr = st.frame(i)
        d, gt, m = fr['tof_depth'], fr['depth_gt'], fr['mask']
        out = ref.prepare_depth(d, st.K, m, radius=2, sigma_space=1.5, range0=0.06, edge_abs=0.12)
        k = out['valid'][0]
        assert not (k & ~m).any()
        raw += np.abs(d[k] - gt[k]).sum()
        fil += np.abs(out['depth'][0][k] - gt[k]).sum()
        kept += k.sum()
        valid += m.sum()
    print('raw {:.5f} m, filtered {:.5f} m, ratio {:.3f}, kept {:.4f}'.format(raw / kept, fil / kept, fil / raw, kept / valid))
    assert fil / raw < 0.85
    assert kept / valid >= 0.90


def test_front_end_tables_match_the_restatement():
    """frames.py forms the kernel's host arguments - spatial table, (1/fx, 1/fy, cx, cy), cos_min - as the restatement does."""
    for R, s in ((1, 0.8), (2, 1.5), (4, 2.5)):
        assert np.array_equal(frames.spatial_table(R, s), ref.spatial_table(R, s)) and frames.spatial_table(R, s)[(2 * R + 1) ** 2 // 2] == 1
    from online_joint_depthfusion_and_semantic_amd import views
    K = views.cameras('t', ref.INTRINSICS, np.eye(4), 3)[1]
    assert np.array_equal(frames.frame_intrinsics(K), ref.frame_intrinsics(ref.INTRINSICS, 3))
    for a in (None, 20.0, 70.0, 90.0):
        assert frames.options(range0=0.05, max_angle=a)['cos_min'] == ref.cos_min_of(a)
    assert frames.options(range0=0.05, max_angle=90.0)['cos_min'] > 0  # 90 degrees still asks for a normal


def test_prepare_depth_refusals_that_need_no_device():
    d = torch.ones(4, 5)
    bad = [dict(radius=5), dict(radius=-1), dict(radius=1.5), dict(sigma_space=0.0), dict(range0=0.0), dict(range0=float('inf')),
           dict(range0=float('nan')), dict(range2=-1.0), dict(edge_abs=-0.1), dict(edge_rel=float('nan')), dict(near=-0.1),
           dict(near=2.0, far=1.0), dict(max_angle=0.0), dict(max_angle=91.0)]
    for kw in bad:
        with pytest.raises(ValueError, match='^prepare_depth: '):
            frames.prepare_depth(d, **dict(dict(range0=0.05), **kw))
    with pytest.raises(TypeError):
        frames.prepare_depth(d)  # range0 has no default: the range width is the sensor's
    with pytest.raises(ValueError, match='^prepare_depth: depth must be'):
        frames.prepare_depth(d, range0=0.05)  # a host tensor
    with pytest.raises(ValueError, match='^prepare_depth: depth must be'):
        frames.prepare_depth(d.numpy(), range0=0.05)
    for f in (None, [], dict(radius=1), dict(range0=0.05, normals=True), dict(range0=0.05, mask=None), dict(range0=-1.0)):
        with pytest.raises(ValueError, match='^prepare_depth: '):
            frames.check_filter(f)
    frames.check_filter(dict(range0=0.05, radius=3, edge_abs=0.1, max_angle=70.0))


def test_library_refuses_bad_arguments_before_any_device_call():
    """ojf_depth_prepare on a machine without a device: every malformed description is refused under the entry point's name
    (the "device" addresses are host bytes nothing reads)."""
    import ctypes
    from online_joint_depthfusion_and_semantic_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    a = ctypes.addressof(buf)
    a += (-a) % 16
    S = frames.spatial_table(1, 1.0)
    K = np.array([[0.02, 0.02, 2.0, 2.0]], dtype=np.float32)
    good = dict(depth=a, mask=None, n=1, h=4, w=5, K=K.ctypes.data, radius=1, spatial=S.ctypes.data, range0=0.05, range2=0.0, edge_abs=0.0,
                edge_rel=0.0, near=0.0, far=float('inf'), cos_min=0.0, out=a + 256, valid=a + 512, normals=a + 1024)
    order = list(good)
    half = S.copy()
    half[4] = 0.5
    nanK = K.copy()
    nanK[0, 1] = np.nan
    cases = [(dict(depth=None), b'null'), (dict(out=None), b'null'), (dict(n=0), b'>= 1'), (dict(h=70000, w=70000), b'too large'),
             (dict(radius=5), b'radius'), (dict(radius=-1), b'radius'), (dict(spatial=None), b'spatial_host'), (dict(spatial=half.ctypes.data), b'centre'),
             (dict(range0=0.0), b'range0'), (dict(range2=float('nan')), b'range0'), (dict(edge_abs=-1.0), b'edge_abs'), (dict(near=-1.0), b'near'),
             (dict(near=2.0, far=1.0), b'near'), (dict(cos_min=1.5), b'cos_min'), (dict(K=None), b'K_host'),
             (dict(K=None, normals=None, cos_min=0.5), b'K_host'), (dict(K=nanK.ctypes.data), b'non-finite'), (dict(out=a + 258), b'aligned'),
             (dict(out=a), b'in-place'), (dict(out=a + 40), b'overlaps'), (dict(valid=a + 256 + 8), b'overlap'), (dict(mask=a + 512 + 3), b'overlaps')]
    for fault, word in cases:
        args = dict(good, **fault)
        assert lib.ojf_depth_prepare(*[args[k] for k in order], None) != 0, fault
        msg = lib.ojf_last_error()
        assert msg.startswith(b'ojf_depth_prepare: ') and word in msg, (fault, msg)


def test_pipeline_refuses_depth_filter_in_a_network_mode():
    for name in ('v2', 'v3'):
        cfg = default_config(24, 32, model=name)
        cfg.FUSION_MODEL.depth_filter = dict(range0=0.05)
        with pytest.raises(ValueError, match='depth_filter'):
            Pipeline(cfg)
    cfg = default_config(24, 32, model='tsdf')
    assert cfg.FUSION_MODEL.depth_filter is None
    cfg.FUSION_MODEL.depth_filter = dict(range0=0.05, radius=7)
    with pytest.raises(ValueError, match='^prepare_depth: radius'):
        Pipeline(cfg)
    cfg.FUSION_MODEL.depth_filter = dict(range0=0.05, radius=2, edge_abs=0.1)
    Pipeline(cfg)
