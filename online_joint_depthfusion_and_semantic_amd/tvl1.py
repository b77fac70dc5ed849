"""Robust TV-L1 fusion of depth views (Zach et al., ICCV 2007): every voxel keeps a histogram of the truncated distances the
views proposed for it - an fp16 [X,Y,Z,S] record volume like the class distributions of label_probs.py - and the fused field is
the minimiser of total variation plus an L1 distance to those samples over the observed voxels: a regularised median, where
projective.py and FusionNet's integrate keep a running mean that one grossly wrong frame bends for good.  The kernels are
csrc/ojf_tvl1.hip (``ojf_fuse_depth_hist``, ``ojf_tvl1_solve``, ``ojf_tvl1_write``); their fp32 definition is written in that
file's header and restated in numpy by tests/tvl1_ref.py.

The volume frame is the one extract, integrate, render and projective use.  A record is S = 8·ceil((B+1)/8) halves: the B bin
means, the weight W (channel B; 0: never observed), and padding that no kernel touches.  Bin b sits at the normalised distance
2b/(B-1) - 1; the solver's field ``u`` is in the same units (-1: -truncation, +1: +truncation).
"""
import math

import numpy as np
import torch

from . import _lib, views
from .ops import _origin_array


def record_size(n_bins):
    """S: the fp16 elements of a voxel's record for ``n_bins`` bins (2.._lib.HIST_MAX_BINS)."""
    n_bins = int(n_bins)
    if not 2 <= n_bins <= _lib.HIST_MAX_BINS:
        raise ValueError('tvl1: n_bins must be in 2..{}, got {}'.format(_lib.HIST_MAX_BINS, n_bins))
    return 8 * ((n_bins + 8) // 8)


def new_volume(shape, n_bins, device):
    """The zeroed histogram volume of a [X,Y,Z] grid: fp16 [X,Y,Z,S]."""
    return torch.zeros(tuple(shape) + (record_size(n_bins),), dtype=torch.float16, device=device)


def _volume(volume, n_bins, who):
    S = record_size(n_bins)
    if not (torch.is_tensor(volume) and volume.is_cuda and volume.dtype == torch.float16 and volume.dim() == 4
            and volume.shape[3] == S and volume.is_contiguous() and volume.data_ptr() % 16 == 0):
        raise ValueError('{}: hist must be a contiguous, 16-byte aligned cuda fp16 [X,Y,Z,{}] tensor for {} bins'.format(who, S, n_bins))
    return tuple(volume.shape[:3])


def integrate_depth_hist(hist, n_bins, *, origin, resolution, depth, intrinsics, extrinsics, mask=None, truncation, max_weight=128.0,
                         near=0.0, carve=True):
    """Fuse ``n`` depth views into a device histogram volume in place, on the current stream of the volume's device.

    hist: cuda fp16 [X,Y,Z,S] (``new_volume``); depth, mask, intrinsics, extrinsics, truncation, max_weight and near as for
    ``projective.integrate_depth``.  carve (the default): a voxel in the free space in front of a view's surface votes for the
    last bin, which is what lets good views outvote a wrong surface hanging in the air; without it a view votes only within
    ``truncation`` of its surface.  The views are fused in order; more than ``_lib.HIST_MAX_VIEWS`` go in several kernel calls,
    with the same bits as one view per call."""
    who = 'integrate_depth_hist'
    X, Y, Z = _volume(hist, n_bins, who)  # (first: a host tensor or a bad bin count is a ValueError on any machine)
    _lib.require_gpu()
    lib = _lib.load()
    dev = hist.device
    depth = views.depth_frames(who, depth, dev)
    n, h, w = depth.shape
    truncation, max_weight, near = views.running_mean_options(who, 'truncation', truncation, max_weight, near)
    n, K, E = views.cameras(who, intrinsics, extrinsics, n)
    mask = views.images(who, mask, 'mask', torch.uint8, n, h, w, dev)
    org = _origin_array(origin)
    stream = _lib.stream_ptr(dev)
    for v0, v1, Kc, Ec in views.chunks(n, _lib.HIST_MAX_VIEWS, K, E):
        rc = lib.ojf_fuse_depth_hist(_lib.ptr(hist), int(n_bins), X, Y, Z, org.ctypes.data, float(resolution), v1 - v0,
                                     Kc.ctypes.data, Ec.ctypes.data, _lib.ptr(depth[v0:v1]), _lib.ptr(views.part(mask, v0, v1)), h, w,
                                     truncation, max_weight, near, int(bool(carve)), stream)
        _lib.check(rc, 'ojf_fuse_depth_hist')


def default_step():
    """tau = sigma: the largest fp32 value whose square is <= 1/12 (the bound ||grad||^2 <= 12 of a 3-D grid gives)."""
    s = np.float32(1.0 / math.sqrt(12.0))
    while float(s) * float(s) > 1.0 / 12.0:
        s = np.nextafter(s, np.float32(0.0))
    return float(s)


def solver_options(who, lam, iterations, tau, sigma):
    """(lam, iterations, tau, sigma) as the kernel takes them; ValueError for what it would refuse."""
    lam, iterations = float(lam), int(iterations)
    tau = default_step() if tau is None else float(np.float32(tau))
    sigma = default_step() if sigma is None else float(np.float32(sigma))
    if not (0.0 < lam < float('inf')) or iterations < 0:
        raise ValueError('{}: lam > 0 and iterations >= 0 expected, got {}, {}'.format(who, lam, iterations))
    if not (tau > 0.0 and sigma > 0.0 and tau * sigma <= 1.0 / 12.0):
        raise ValueError('{}: tau, sigma > 0 with tau * sigma <= 1/12 expected, got {}, {}'.format(who, tau, sigma))
    return lam, iterations, tau, sigma


class Solver:
    """The TV-L1 solver's state for one box shape on one device: ``u`` (f32 [X,Y,Z], normalised distance; meaningful at the
    observed voxels of the histogram it was solved for) and the workspace.  One Solver serves one histogram volume at a time:
    ``restart=False`` continues from what the previous ``solve`` left."""

    def __init__(self, shape, device):
        shape = tuple(int(s) for s in shape)
        if len(shape) != 3 or min(shape) < 1:
            raise ValueError('tvl1.Solver: a [X,Y,Z] shape expected, got {}'.format(shape))
        device = torch.device(device)
        if device.type != 'cuda':
            raise ValueError('tvl1.Solver: a cuda device expected, got {}'.format(device))
        _lib.require_gpu()
        nbytes = _lib.load().ojf_tvl1_workspace_bytes(*shape)
        if nbytes == 0:
            raise ValueError('tvl1.Solver: the box {} is too large'.format(shape))
        self.shape, self.device = shape, device
        self.u = torch.zeros(shape, dtype=torch.float32, device=device)
        self.workspace = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
        self._ws_ptr = (self.workspace.data_ptr() + 255) & ~255
        self._ws_bytes = nbytes
        self._started = False
        self._hist, self._n_bins = None, None  # what the last solve ran on: what write reads the weights of

    def solve(self, hist, n_bins, lam, iterations, tau=None, sigma=None, restart=True, changed=False, all_bricks=False):
        """``iterations`` Chambolle-Pock iterations on the observed voxels of ``hist``, on the current stream.  restart: start
        from the per-voxel histogram mean with a zero dual; else continue (N iterations in one call give the bits of any split
        over consecutive calls) - with ``changed`` when views were fused into ``hist`` since the previous call: voxels
        observed for the first time join at their histogram mean.  tau, sigma default to ``default_step()``.  all_bricks
        (measurements): the iterations visit every brick of the box, not only those that hold an observed voxel."""
        who = 'tvl1.Solver.solve'
        if _volume(hist, n_bins, who) != self.shape or hist.device != self.device:
            raise ValueError('{}: hist must be a {} volume on {}'.format(who, self.shape, self.device))
        lam, iterations, tau, sigma = solver_options(who, lam, iterations, tau, sigma)
        if not restart and not self._started:
            raise ValueError('{}: restart=False before any restart'.format(who))
        mode = _lib.TVL1_RESTART if restart else (_lib.TVL1_REFRESH if changed else _lib.TVL1_CONTINUE)
        if all_bricks:
            if mode == _lib.TVL1_CONTINUE:
                raise ValueError('{}: all_bricks needs restart or changed (it is the set-up pass that lists the bricks)'.format(who))
            mode |= _lib.TVL1_ALL_BRICKS
        rc = _lib.load().ojf_tvl1_solve(_lib.ptr(hist), int(n_bins), *self.shape, lam, tau, sigma, iterations, mode, _lib.ptr(self.u),
                                        self._ws_ptr, self._ws_bytes, _lib.stream_ptr(self.device))
        _lib.check(rc, 'ojf_tvl1_solve')
        self._started = True
        self._hist, self._n_bins = hist, int(n_bins)
        return self.u

    def write(self, tsdf, weights, truncation):
        """tsdf = truncation · u and weights = W at the observed voxels of the histogram volume the last ``solve`` ran on (cuda
        fp16 [X,Y,Z] volumes, in place); the other voxels keep what they hold."""
        who = 'tvl1.Solver.write'
        if self._hist is None:
            raise ValueError('{}: nothing was solved yet'.format(who))
        hist, n_bins = self._hist, self._n_bins
        views.volume3(who, tsdf, 'tsdf', torch.float16, self.shape, self.device)
        views.volume3(who, weights, 'weights', torch.float16, self.shape, self.device)
        truncation = float(truncation)
        if not 0.0 < truncation < float('inf'):
            raise ValueError('{}: truncation > 0 expected, got {}'.format(who, truncation))
        rc = _lib.load().ojf_tvl1_write(_lib.ptr(hist), int(n_bins), *self.shape, _lib.ptr(self.u), truncation, _lib.ptr(tsdf),
                                        _lib.ptr(weights), _lib.stream_ptr(self.device))
        _lib.check(rc, 'ojf_tvl1_write')
