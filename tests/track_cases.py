"""Analytic tracker cases that need no device to build: live frames of the synthetic stream, model depth images ray-cast
analytically at the reference pose and model normals from the gradient of the room's signed distance.  The GPU tests
upload these maps and call ojf_track / ojf_track_associate through the raw ABI; test_track_steps_host.py shows on the
numpy restatement (track_ref.py) that every case meets the conditions its GPU test relies on.  Test helper, not a test."""
import functools

import numpy as np

from online_joint_depthfusion_and_semantic_amd import synthetic
from online_joint_depthfusion_and_semantic_amd.ops import camera_arrays
from online_joint_depthfusion_and_semantic_amd.tracking import level_intrinsics
import track_ref

f32 = np.float32

# name: (h, w, levels, iterations of level 0.., reference frame i (the live frame is i + 1), noise-free live depth,
#        perturbation of the start (deg, m, axis, direction) or None)
STEP_CASES = {
    'A': (128, 176, 4, (2, 1, 2, 2), 230, False, None),   # level 3 is 16 x 22
    'B': (131, 179, 4, (1, 0, 2, 1), 50, False, None),    # a row and a column dropped at every level; level 1 idle
    'C': (64, 88, 3, (2, 2, 2), 230, False, (2.0, 0.03, (1, 0, 0), (0, 1, 0))),
    'D': (67, 93, 3, (2, 0, 1), 310, True, None),
    'E': (32, 40, 1, (3,), 300, False, None),             # levels == 1
}

# frame size: (associate blocks at level 0, reference frame) - the solve reads the block rows in LDS chunks of 64
CHUNK_CASES = {
    (256, 256): (64, 230),    # one full chunk
    (256, 260): (65, 230),    # a chunk of one row
    (256, 257): (65, 230),    # the same, the last block a quarter full
    (256, 512): (128, 230),   # two full chunks
    (256, 513): (129, 230),
}


def model_maps(E_ref, K, h, w, levels):
    """Per level (depth f32[h_l,w_l], normals f32[h_l,w_l,3], Kinv f32[9], surface ids i64[h_l,w_l]) of the analytic room
    seen from E_ref: synthetic._raycast for the depth, the normalised central-difference gradient of scene_sdf at the hit
    points for the normals (it points into free space, as the definition wants), Kinv as tracking.py forms it."""
    E_ref = np.asarray(E_ref, np.float64).reshape(-1, 4)[:3]
    out = []
    for l in range(levels):
        Kl = level_intrinsics(K, l)
        hl, wl = h >> l, w >> l
        t, ids = synthetic._raycast(E_ref, Kl, hl, wl)
        u, v = np.meshgrid(np.arange(wl, dtype=np.float64), np.arange(hl, dtype=np.float64))
        dc = np.stack([(u - Kl[0, 2]) / Kl[0, 0], (v - Kl[1, 2]) / Kl[1, 1], np.ones_like(u)], axis=-1)
        p = (dc * t[..., None]) @ E_ref[:, :3].T + E_ref[:, 3]
        e = 1e-4
        g = np.stack([synthetic.scene_sdf(p + e * ax) - synthetic.scene_sdf(p - e * ax) for ax in np.eye(3)], axis=-1)
        n = np.linalg.norm(g, axis=-1, keepdims=True)
        g = np.where(n > 0, g / np.where(n > 0, n, 1.0), 0.0)
        out.append((np.ascontiguousarray(t, f32), np.ascontiguousarray(g, f32), camera_arrays(Kl, E_ref)[0], ids))
    return out


def build_case(h, w, levels, iterations, ref_frame, noise_free=False, start=None):
    st = synthetic.SyntheticStream(h, w, 64, 400)
    f0, f1 = st.frame(ref_frame), st.frame(ref_frame + 1)
    E_ref = f0['extrinsics']
    E_init = E_ref if start is None else track_ref.perturb(E_ref, *start)
    depth = f1['depth_gt'] if noise_free else f1['tof_depth']
    mask = None if noise_free else f1['mask']
    return dict(h=h, w=w, levels=levels, iterations=tuple(iterations), K=st.K, E_ref=E_ref, E_init=E_init, depth=depth,
                mask=mask, models=model_maps(E_ref, st.K, h, w, levels), dist=0.1, angle=20.0, delta=0.03, frac=0.05)


@functools.lru_cache(maxsize=None)
def step_case(name):
    h, w, levels, its, i, noise_free, start = STEP_CASES[name]
    return build_case(h, w, levels, its, i, noise_free, start)


@functools.lru_cache(maxsize=None)
def chunk_case(h, w):
    """One level, one step, noise-free live depth: with the stream's 5 mm noise the live normals of a 256-pixel-wide
    frame tilt past the 20 degree gate (the best frame pair of a scan of 10..390 has an inlier share of 0.257 at 256x256
    and 0.127 at 256x512), and the solve's chunk edges deserve a well-posed system."""
    return build_case(h, w, 1, (1,), CHUNK_CASES[(h, w)][1], noise_free=True)


def with_models(case, level, depth=None, normals=None, **kw):
    """A copy of ``case`` with level ``level``'s model depth / normals replaced (and further entries overridden)."""
    out = dict(case)
    models = list(case['models'])
    md, mn, Ki, ids = models[level]
    models[level] = (md if depth is None else np.ascontiguousarray(depth, f32),
                     mn if normals is None else np.ascontiguousarray(normals, f32), Ki, ids)
    out['models'] = models
    out.update(kw)
    return out


def run(case, iterations=None, trace=None):
    """track_ref.run on a case: (pose, (code, iteration), stats)."""
    m = case['models']
    return track_ref.run(case['depth'], case['mask'], case['K'], [x[2] for x in m], [x[0] for x in m], [x[1] for x in m],
                         case['E_ref'], case['E_init'], case['iterations'] if iterations is None else iterations,
                         case['dist'], case['angle'], case['delta'], case['frac'], trace=trace)


@functools.lru_cache(maxsize=None)
def healthy_trace(name):
    """(pose, status, stats, trace) of the restated whole call on step case ``name``."""
    trace = []
    pose, status, stats = run(step_case(name), trace=trace)
    return pose, status, stats, trace


# ---- failures after the first iteration (case C: 64x88, 3 levels, (2, 2, 2): steps 0-1 level 2, 2-3 level 1, 4-5 level 0)
def _nan_pixel_case():
    """Case C with one NaN in level 1's model depth, at a model pixel that exactly one inlier of the healthy run's step 2
    projects to: that pixel stays an inlier (dm == 0 is false, the NaN comparisons of reasons 6 and 7 are false) with a
    NaN residual, so b is NaN and the step is not finite."""
    case = step_case('C')
    step2 = healthy_trace('C')[3][2]
    assert step2['level'] == 1
    md, mn, Ki, _ = case['models'][1]
    D1 = track_ref.pyramid(case['depth'], case['mask'], 2, case['delta'])[1]
    _, _, reason, mr, mc = track_ref.associate(D1, Ki, case['K'], 1, md, mn, case['E_ref'], step2['pose'], case['dist'],
                                               case['angle'], pixels=True)
    flat = (mr * md.shape[1] + mc)[reason == 0]
    hits = np.bincount(flat, minlength=md.size)
    target = int(np.flatnonzero(hits == 1)[0])
    bad = md.copy()
    bad.reshape(-1)[target] = np.nan
    return with_models(case, 1, depth=bad), target


@functools.lru_cache(maxsize=None)
def failure_cases():
    """name -> (case, status code, iteration index it fails at)."""
    case = step_case('C')
    md1, _, _, ids1 = case['models'][1]
    main = int(np.bincount(ids1.reshape(-1)).argmax())
    return {
        'no inliers at level 1': (with_models(case, 1, depth=np.zeros_like(md1)), 1, 2),
        'no inliers at level 0': (with_models(case, 0, depth=np.zeros_like(case['models'][0][0])), 1, 4),
        'one plane at level 1': (with_models(case, 1, depth=np.where(ids1 == main, md1, f32(0)), frac=0.01), 2, 2),
        'NaN residual at level 1': (_nan_pixel_case()[0], 3, 2),
    }


# ---- pyramid inputs the synthetic stream never makes
PYRAMID_SHAPES = ((64, 64), (67, 93))  # level 3: 8 x 8 (the smallest legal level, one wave) and 8 x 11
PYRAMID_DELTAS = (0.03, 0.0, 0.1, 1e30)
SUBNORMAL = f32(1e-41)


def hostile_frame(h, w, seed, with_mask=True):
    """(depth f32[h,w], mask u8[h,w] or None): a stream frame with shares of NaN, +inf, -inf, negative values, -0.0, a
    subnormal and exact 0, and mask bytes drawn from {0, 1, 2, 255}."""
    rng = np.random.default_rng(seed)
    depth = synthetic.SyntheticStream(h, w, 64, 400).frame(120)['tof_depth'].copy()
    kind = rng.choice(8, size=(h, w), p=[0.58, 0.06, 0.06, 0.06, 0.06, 0.06, 0.06, 0.06])
    for k, v in enumerate((np.nan, np.inf, -np.inf, None, -0.0, SUBNORMAL, 0.0), start=1):
        sel = kind == k
        depth[sel] = -depth[sel] - f32(0.5) if v is None else f32(v)
    mask = rng.choice(np.array([0, 1, 2, 255], np.uint8), size=(h, w), p=[0.2, 0.4, 0.2, 0.2]) if with_mask else None
    return depth, mask


def spread(v, b, delta):
    """-1 / 0 / +1: fp32(v - b) below, exactly at or above fp32(delta)."""
    d = f32(f32(v) - f32(b))
    dl = f32(delta)
    return -1 if d < dl else (0 if d == dl else 1)


def _spread_values(delta, kind, rng):
    """(b, v) f32 with v >= b > 0 and fp32(v - b) below (-1), exactly (0) or above (+1) fp32(delta); None when fp32 has
    no such pair (nothing is below a spread of 0)."""
    dl = f32(delta)
    if kind < 0 and dl == 0:
        return None
    for _ in range(10000):
        if dl == 0:
            b = f32(rng.uniform(0.5, 3.0))
            v = b if kind == 0 else f32(b * f32(rng.uniform(1.01, 1.5)))
        elif kind == 0:
            # b below delta, so that b + delta is a value of fp32 (about one draw in four) and v - b is delta again
            b = f32(dl * f32(rng.uniform(0.3, 1.0)))
            v = f32(b + dl)
        else:
            b = f32(rng.uniform(0.5, 3.0)) if dl < 1e20 else f32(rng.uniform(0.5, 3.0) * 1e29)
            near = np.nextafter(f32(b + dl), f32(0 if kind < 0 else np.inf), dtype=f32)
            far = f32(b + dl * f32(rng.uniform(0.1, 0.9) if kind < 0 else rng.uniform(1.1, 3.0)))
            v = near if rng.random() < 0.5 else far
        if v >= b and np.isfinite(v) and spread(v, b, delta) == kind:
            return b, v
    raise AssertionError('no fp32 pair with spread kind %d for delta %r' % (kind, delta))


def block_frame(h, w, delta, seed):
    """(depth f32[h,w], blocks): every 2x2 block holds one of the 16 occupancy patterns; one occupied entry is the
    block's minimum b, each other one is b or a value v whose spread v - b is below, exactly or above fp32(delta).
    blocks: list of (pattern 0..15, spread kind) in raster order of the whole blocks."""
    rng = np.random.default_rng(seed)
    depth = np.zeros((h, w), f32)
    blocks = []
    n = 0
    for r in range(h >> 1):
        for c in range(w >> 1):
            pattern, kind = n % 16, (n // 16) % 3 - 1
            n += 1
            pair = _spread_values(delta, kind, rng)
            if pair is None:
                kind = 0
                pair = _spread_values(delta, 0, rng)
            b, v = pair
            occupied = [k for k in range(4) if pattern >> k & 1]
            vals = np.zeros(4, f32)
            if occupied:
                lowest = occupied[int(rng.integers(len(occupied)))]
                others = [k for k in occupied if k != lowest]
                vals[lowest] = b
                for j, k in enumerate(others):
                    vals[k] = v if j == 0 or rng.random() < 0.5 else b
            depth[2 * r:2 * r + 2, 2 * c:2 * c + 2] = vals.reshape(2, 2)
            blocks.append((pattern, kind))
    if h & 1:
        depth[-1] = f32(1.5)
    if w & 1:
        depth[:, -1] = f32(1.5)
    return depth, blocks


@functools.lru_cache(maxsize=None)
def pyramid_inputs():
    """name -> (depth, mask, delta): what test_track_steps_gpu.py feeds the pyramid kernel with 4 levels."""
    out = {}
    for h, w in PYRAMID_SHAPES:
        f = synthetic.SyntheticStream(h, w, 64, 400).frame(120)
        out['stream %dx%d' % (h, w)] = (f['tof_depth'], f['mask'], 0.03)
        for delta in PYRAMID_DELTAS:
            out['hostile %dx%d delta %g' % (h, w, delta)] = hostile_frame(h, w, 7 * h + w) + (delta,)
            out['blocks %dx%d delta %g' % (h, w, delta)] = (block_frame(h, w, delta, 11 * h + w)[0], None, delta)
        out['hostile %dx%d no mask' % (h, w)] = hostile_frame(h, w, 3 * h + w, with_mask=False) + (0.03,)
    return out


# ---- association with non-default thresholds and arbitrary model maps (case C, levels 0 and 2)
THRESHOLD_CASES = {'angle 180': dict(angle=180.0), 'angle 0.5': dict(angle=0.5), 'dist 1e-3': dict(dist=1e-3),
                   'dist 10': dict(dist=10.0)}


@functools.lru_cache(maxsize=None)
def fuzz_case(level):
    """(live mask, model depth, model normals, pose) at ``level`` of case C: the model depth times a random factor in
    [0.9, 1.1] with 10 % zeros, random normals (not unit, both signs), the pose 3 deg / 5 cm from the reference.  The
    live mask drops whole 8x8 blocks (a tenth of them), so that "no depth" also occurs at level 2."""
    case = step_case('C')
    md, mn, _, _ = case['models'][level]
    rng = np.random.default_rng(1000 + level)
    depth = (md * rng.uniform(0.9, 1.1, size=md.shape).astype(f32)).astype(f32)
    depth[rng.random(md.shape) < 0.1] = 0
    normals = (rng.normal(size=mn.shape) * rng.uniform(0.2, 3.0, size=md.shape + (1,))).astype(f32)
    pose = track_ref.perturb(case['E_ref'], 3.0, 0.05, (0.2, 1.0, -0.3), (1.0, -0.5, 0.4))
    keep = rng.random((case['h'] // 8, case['w'] // 8)) >= 0.1
    mask = case['mask'] & np.kron(keep, np.ones((8, 8), bool))
    return mask, depth, normals, pose
