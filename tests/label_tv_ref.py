"""numpy restatement of the multi-label TV solver's definition in csrc/ojf_label_tv.hip (ojf_label_tv_setup / _solve / _write):
every fp32 operation is one numpy ufunc on float32 arrays (rounded on its own), the ascending-k sums are loops over k, min / max
are np.fmin / np.fmax (IEEE minNum / maxNum).  Also the float64 yardsticks of the host tests (the sort-based simplex projection,
the energy), the cases the CPU and GPU tests share and the noisy-label experiment both measure.  Test helper, not a test."""
import functools
import math

import numpy as np

import label_ref

F = np.float32
MAX_CLASSES = 32
PAD_BITS = label_ref.PAD_BITS
record_size = label_ref.record_size


def default_step():
    """tau = sigma: the largest fp32 value whose square is <= 1/12 (tvl1.default_step)."""
    s = F(1.0 / math.sqrt(12.0))
    while float(s) * float(s) > 1.0 / 12.0:
        s = np.nextafter(s, F(0.0))
    return s


STEP = default_step()


def project(v):
    """Pi(v) of f32 [N, C], row by row: for every j the sum s_j (ascending k, from 0.0f) and the count n_j of the v_k >= v_j,
    theta_j = (s_j - 1) / float(n_j); theta = max_j theta_j; max(v_k - theta, 0)."""
    v = np.asarray(v, F)
    N, C = v.shape
    theta = np.full(N, -np.inf, F)
    with np.errstate(all='ignore'):
        for j in range(C):
            s, n = np.zeros(N, F), np.zeros(N, F)
            for k in range(C):
                ge = v[:, k] >= v[:, j]
                s = np.where(ge, s + v[:, k], s)
                n = n + ge.astype(F)  # (a count up to 32: exact)
            theta = np.fmax(theta, (s - F(1)) / n)
        return np.fmax(v - theta[:, None], F(0))


def project_f64(v):
    """The sort-based Euclidean projection onto the simplex (Held, Wolfe, Crowder 1974) in float64: the yardstick of
    ``project``."""
    v = np.asarray(v, np.float64)
    N, C = v.shape
    srt = -np.sort(-v, axis=1)
    css = np.cumsum(srt, axis=1) - 1.0
    ks = np.arange(1, C + 1, dtype=np.float64)
    rho = (srt - css / ks > 0).sum(axis=1)  # (the condition holds for a prefix)
    theta = css[np.arange(N), rho - 1] / rho
    return np.maximum(v - theta[:, None], 0.0)


def _up(a, axis):
    """a(x + e_axis), 0 outside the box"""
    o = np.zeros_like(a)
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    src[axis], dst[axis] = slice(1, None), slice(None, -1)
    o[tuple(dst)] = a[tuple(src)]
    return o


def _down(a, axis):
    """a(x - e_axis), 0 outside the box"""
    o = np.zeros_like(a)
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    src[axis], dst[axis] = slice(None, -1), slice(1, None)
    o[tuple(dst)] = a[tuple(src)]
    return o


class Solver:
    """The state of the definition on dense arrays: u, ub f32 [C,X,Y,Z] and p f32 [C,3,X,Y,Z], all 0 at unobserved voxels (a p
    whose edge does not count is 0 at every step, which is what makes the shifted read of the primal step the definition's
    m_a)."""

    def __init__(self, vol, C):
        assert 2 <= C <= MAX_CLASSES and vol.shape[3] == record_size(C) and vol.dtype == np.float16
        self.vol, self.C = vol, C
        self.W = vol[..., C].astype(F)
        with np.errstate(all='ignore'):
            self.obs = self.W > 0
        self.P = np.ascontiguousarray(np.moveaxis(vol[..., :C].astype(F), -1, 0))
        self.edge = [self.obs & _up(self.obs, a) for a in range(3)]
        self.restart()

    def restart(self):
        C = self.C
        self.u = np.zeros((C,) + self.obs.shape, F)
        self.u[:, self.obs] = project(self.P[:, self.obs].T).T
        self.ub = self.u.copy()
        self.p = np.zeros((C, 3) + self.obs.shape, F)

    def iterate(self, n, lam=4.0, w_sat=4.0, tau=None, sigma=None):
        tau = STEP if tau is None else F(tau)
        sigma = STEP if sigma is None else F(sigma)
        w_sat = F(w_sat)
        tl = F(tau * F(lam))
        omega = np.fmin(self.W, w_sat) / w_sat
        tlo = tl * omega
        obs, C = self.obs, self.C
        for _ in range(n):
            v = np.zeros((C,) + obs.shape, F)
            for k in range(C):
                ub = self.ub[k]
                q = [np.where(self.edge[a], self.p[k, a] + sigma * (_up(ub, a) - ub), F(0)) for a in range(3)]
                d = np.fmax(F(1), np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]))
                for a in range(3):
                    self.p[k, a] = q[a] / d
                t = [self.p[k, a] - _down(self.p[k, a], a) for a in range(3)]
                div = (t[0] + t[1]) + t[2]
                v[k] = (self.u[k] + tau * div) + tlo * self.P[k]
            new = project(v[:, obs].T).T
            old = self.u[:, obs]
            self.ub[:, obs] = F(2) * new - old
            self.u[:, obs] = new
        return self

    def write(self, ids, scores, probs_out=None):
        """In place on ids u8 [X,Y,Z], scores fp16 [X,Y,Z] and, if given, the record volume probs_out."""
        obs, C = self.obs, self.C
        best = self.u[0].copy()
        idx = np.zeros(obs.shape, np.uint8)
        for k in range(1, C):
            win = self.u[k] > best
            best = np.where(win, self.u[k], best)
            idx = np.where(win, np.uint8(k), idx)
        ids[obs] = idx[obs]
        scores[obs] = best.astype(np.float16)[obs]
        if probs_out is not None:
            for k in range(C):
                probs_out[..., k][obs] = self.u[k].astype(np.float16)[obs]
            probs_out.view(np.uint16)[..., C][obs] = self.vol.view(np.uint16)[..., C][obs]

    def energy(self, lam=4.0, w_sat=4.0):
        """sum_k sum_x |grad u_k| over the counted edges minus lam · sum_x omega <u, P>, in float64."""
        u = self.u.astype(np.float64)
        tv = 0.0
        for k in range(self.C):
            g2 = sum(np.where(self.edge[a], _up(u[k], a) - u[k], 0.0) ** 2 for a in range(3))
            tv += float(np.sqrt(g2)[self.obs].sum())
        omega = np.minimum(self.W.astype(np.float64), w_sat) / w_sat
        data = float((omega * (u * self.P.astype(np.float64)).sum(axis=0))[self.obs].sum())
        return tv - lam * data


# ---- cases -------------------------------------------------------------------------------------------------------------------
BRICK = (4, 8, 32)
PATTERNS = ('all', 'random', 'other_bricks', 'corner', 'faces', 'none', 'zero_sum')


def case_volume(shape, C, pattern, seed=0):
    """A seeded label volume fp16 [X,Y,Z,S]: a normalised distribution and W in 1..5 (10 %: 8) at the observed voxels, an
    all-zero record at the others, PAD_BITS in every padding channel.  pattern: 'all' voxels observed; 'random' (60 %);
    'other_bricks' (every other 4 x 8 x 32 brick unobserved: neighbours in bricks that are not listed); 'corner' (one voxel,
    the last of the box); 'faces' (only the voxels on either side of the first brick boundary of every axis); 'none';
    'zero_sum' (all observed, a third of the records with P = 0: the start value is uniform)."""
    shape = tuple(shape)
    rng = np.random.default_rng([seed, 23, C, PATTERNS.index(pattern)] + list(shape))
    x, y, z = np.meshgrid(*[np.arange(s) for s in shape], indexing='ij')
    if pattern in ('all', 'zero_sum'):
        obs = np.ones(shape, bool)
    elif pattern == 'random':
        obs = rng.random(shape) < 0.6
    elif pattern == 'other_bricks':
        obs = (x // BRICK[0] + y // BRICK[1] + z // BRICK[2]) % 2 == 0
    elif pattern == 'corner':
        obs = (x == shape[0] - 1) & (y == shape[1] - 1) & (z == shape[2] - 1)
    elif pattern == 'faces':
        obs = np.isin(x, (BRICK[0] - 1, BRICK[0])) | np.isin(y, (BRICK[1] - 1, BRICK[1])) | np.isin(z, (BRICK[2] - 1, BRICK[2]))
    else:
        obs = np.zeros(shape, bool)
    w = rng.integers(1, 6, shape).astype(np.float16)
    w[rng.random(shape) < 0.10] = 8
    p = rng.random(shape + (C,)) ** 4
    p /= p.sum(axis=-1, keepdims=True)
    if pattern == 'zero_sum':
        p[rng.random(shape) < 1 / 3] = 0
    vol = np.zeros(shape + (record_size(C),), np.float16)
    vol[..., :C] = p.astype(np.float16)
    vol[..., C] = w
    vol[~obs] = 0
    vol.view(np.uint16)[..., C + 1:] = PAD_BITS
    return vol


def sentinels(shape):
    """ids / scores no solver writes: 0xee and the bits 0x7e01 (a NaN)"""
    return np.full(shape, 0xee, np.uint8), np.full(shape, 0x7e01, np.uint16).view(np.float16)


@functools.lru_cache(maxsize=None)
def solved_case(shape, C, pattern, iterations=(0, 1, 7)):
    """(volume, {n: (u f32 [C,X,Y,Z], ids, scores, probs_out)}) for n of ``iterations`` (ascending) with the default options,
    the outputs written over sentinels / a copy of the volume with its class channels set to PAD_BITS at every voxel.
    Computed once and shared: nobody writes into it."""
    vol = case_volume(shape, C, pattern)
    s = Solver(vol, C)
    out, done = {}, 0
    for n in iterations:
        s.iterate(n - done)
        done = n
        ids, scores = sentinels(shape)
        probs_out = fresh_probs_out(vol, C)
        s.write(ids, scores, probs_out)
        out[n] = (s.u.copy(), ids, scores, probs_out)
    return vol, out


def fresh_probs_out(vol, C):
    """The second record volume of a write test: every channel PAD_BITS, so that what the write leaves alone shows."""
    return np.full(vol.shape, PAD_BITS, np.uint16).view(np.float16)


# ---- the noisy-label experiment: the regularised decision against the per-voxel vote ---------------------------
NOISE_OPTIONS = dict(lam=4.0, iterations=30, w_sat=4.0)
NOISE_FIGURES = (0.9218, 0.9931, 0.9874, 0.9957)  # measured with this restatement: vote, regularised; on W >= 3: vote, regularised


@functools.lru_cache(maxsize=None)
def noisy_volumes():
    """label_ref.noisy_frames (q = 0.2, seed 7) fused on the host by label_ref.fuse: {'labels_clean': vol, 'labels_noisy': vol}
    (fp16 [64,64,64,24])."""
    from online_joint_depthfusion_and_semantic_amd import synthetic
    st, frames = label_ref.noisy_frames(q=0.2, seed=7)
    origin, res, _ = synthetic.grid_spec(label_ref.NOISE_GRID)
    C, G = label_ref.NOISE_CLASSES, (label_ref.NOISE_GRID,) * 3
    out = {}
    for kind in ('labels_clean', 'labels_noisy'):
        vol = np.zeros(G + (record_size(C),), np.float16)
        for f in frames:
            label_ref.fuse(vol, C, origin, res, f['depth_gt'], f['intrinsics'], f['extrinsics'], f['mask'], labels=f[kind],
                           band=label_ref.NOISE_BAND)
        out[kind] = vol
    return out


def noisy_figures(clean_vote, clean_w, noisy_vote, noisy_reg):
    """(observed, thrice, vote, reg, vote3, reg3): the voxel counts of the two masks (the clean volume's W > 0 and W >= 3) and
    the agreement of the noisy volume's per-voxel vote and of its regularised decision with the clean per-voxel vote on them."""
    observed, thrice = clean_w > 0, clean_w >= 3
    return (int(observed.sum()), int(thrice.sum()),
            label_ref.agreement(noisy_vote, clean_vote, observed), label_ref.agreement(noisy_reg, clean_vote, observed),
            label_ref.agreement(noisy_vote, clean_vote, thrice), label_ref.agreement(noisy_reg, clean_vote, thrice))


def assert_noisy_figures(where, figures):
    """Print the figures and assert the two conditions of the experiment: on the observed voxels the regularised decision is at
    least 0.04 ahead of the vote; on W >= 3 it is not below it."""
    n, n3, vote, reg, vote3, reg3 = figures
    print('noisy labels {}: {} observed, vote {:.4f}, regularised {:.4f}; {} with W >= 3: vote {:.4f}, regularised {:.4f}'.format(
        where, n, vote, reg, n3, vote3, reg3))
    assert n > 15000 and n3 > 8000
    assert reg >= vote + 0.04, (reg, vote)
    assert reg3 >= vote3, (reg3, vote3)
