"""The fused class distributions regularised in space (Zach et al., multi-label TV; Häne et al., joint reconstruction and
class segmentation): where ``label_probs.decide_labels`` lets every voxel of the label volume decide alone, here the
neighbours have a say - the convex relaxation of the Potts model, total variation of every class field minus ``lam`` times the
confidence-weighted agreement with the fused distribution, over fields that are a distribution at every observed voxel; what
tvl1.py does for geometry, done for labels.  The kernels are csrc/ojf_label_tv.hip (``ojf_label_tv_setup``,
``ojf_label_tv_solve``, ``ojf_label_tv_write``); their fp32 definition is written in that file's header and restated in numpy by
tests/label_tv_ref.py.  The reference has no counterpart.

The input is a label volume of label_probs.py with at most ``_lib.LABEL_TV_MAX_CLASSES`` classes.  The solver's state is 5·C
floats per voxel, so it is kept only for the 4 x 8 x 32 bricks of the box that hold an observed voxel: a set-up pass lists them,
the Solver reads their count (its one synchronisation) and sizes the workspace by it.
"""
import numpy as np
import torch

from . import _lib, label_probs, views
from .tvl1 import default_step

BRICK = (4, 8, 32)  # csrc/ojf_label_tv.hip kLtvX, kLtvY, kLtvZ
BRICK_VOXELS = 1024
OBSERVED = 8  # the "observed" bit of a voxel's flag byte


def solver_options(who, lam, iterations, w_sat, tau, sigma):
    """(lam, iterations, w_sat, tau, sigma) as the kernel takes them; ValueError for what it would refuse."""
    lam, iterations, w_sat = float(lam), int(iterations), float(w_sat)
    tau = default_step() if tau is None else float(np.float32(tau))
    sigma = default_step() if sigma is None else float(np.float32(sigma))
    if not (0.0 < lam < float('inf')) or not (0.0 < w_sat < float('inf')) or iterations < 0:
        raise ValueError('{}: lam > 0, w_sat > 0 and iterations >= 0 expected, got {}, {}, {}'.format(who, lam, w_sat, iterations))
    if not (tau > 0.0 and sigma > 0.0 and tau * sigma <= 1.0 / 12.0):
        raise ValueError('{}: tau, sigma > 0 with tau * sigma <= 1/12 expected, got {}, {}'.format(who, tau, sigma))
    return lam, iterations, w_sat, tau, sigma


def workspace_layout(shape, n_classes, capacity):
    """The workspace of include/ojf.h for ``capacity`` listed bricks: a dict of the brick grid ('bricks': per axis), their number
    'n_bricks', the byte offsets 'slot', 'list', 'flags' and 'u', the floats of one state array 'plane' and the size 'bytes'."""
    grid = tuple((s + b - 1) // b for s, b in zip(shape, BRICK))
    nb = grid[0] * grid[1] * grid[2]

    def up(v):
        return (v + 255) & ~255
    off_any = 256
    off_slot = up(off_any + 4 * nb)
    off_list = up(off_slot + 4 * nb)
    off_flags = up(off_list + 4 * nb)
    off_u = up(off_flags + BRICK_VOXELS * nb)
    plane = int(capacity) * int(n_classes) * BRICK_VOXELS
    return dict(bricks=grid, n_bricks=nb, slot=off_slot, list=off_list, flags=off_flags, u=off_u, plane=plane, bytes=off_u + 20 * plane)


class Solver:
    """The multi-label TV solver's state for one box shape and class count on one device.  One Solver serves one label volume at
    a time: ``restart=False`` continues from what the previous ``solve`` on the same volume left."""

    def __init__(self, shape, n_classes, device):
        shape = tuple(int(s) for s in shape)
        if len(shape) != 3 or min(shape) < 1:
            raise ValueError('label_tv.Solver: a [X,Y,Z] shape expected, got {}'.format(shape))
        n_classes = int(n_classes)
        if not 2 <= n_classes <= _lib.LABEL_TV_MAX_CLASSES:
            raise ValueError('label_tv.Solver: n_classes must be in 2..{}, got {}'.format(_lib.LABEL_TV_MAX_CLASSES, n_classes))
        device = torch.device(device)
        if device.type != 'cuda':
            raise ValueError('label_tv.Solver: a cuda device expected, got {}'.format(device))
        _lib.require_gpu()
        self.shape, self.n_classes, self.device = shape, n_classes, device
        self.count = 0  # listed bricks of the last restart
        self.capacity = 0
        self._allocate(0)
        self._count_dev = torch.zeros(1, dtype=torch.int32, device=device)
        self.status = torch.zeros(1, dtype=torch.int32, device=device)  # include/ojf.h: 0 solved, 1 capacity, 2 no state
        self._volume = None  # what the last restart ran on: what a continue must get, and what write reads W of

    def _allocate(self, capacity):
        nbytes = _lib.load().ojf_label_tv_workspace_bytes(*self.shape, self.n_classes, capacity)
        if nbytes == 0:
            raise ValueError('label_tv.Solver: the box {} is too large'.format(self.shape))
        self.layout = workspace_layout(self.shape, self.n_classes, capacity)
        assert self.layout['bytes'] == nbytes, (self.layout, nbytes)
        raw = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        pad = (-raw.data_ptr()) % 256
        self.workspace = raw[pad:pad + nbytes]  # 256-byte aligned
        self.capacity = capacity

    def solve(self, volume, lam=4.0, iterations=30, w_sat=4.0, tau=None, sigma=None, restart=True):
        """``iterations`` Chambolle-Pock iterations on the observed voxels of the label ``volume`` (cuda fp16 [X,Y,Z,S] of this
        Solver's shape and class count), on the current stream.  lam: the weight of the fused distribution against the
        smoothness; w_sat: the fusion weight W at which a voxel's distribution counts in full.  restart: list the observed
        bricks, size the state by their count (one synchronisation) and start from the fused distribution with a zero dual;
        else continue on the same volume object (N iterations in one call give the bits of any split over consecutive
        calls).  There is no warm start across a changed volume: when it took views, restart.  tau, sigma default to
        ``tvl1.default_step()``."""
        who = 'label_tv.Solver.solve'
        if tuple(label_probs._volume(volume, self.n_classes, who)) != self.shape or volume.device != self.device:
            raise ValueError('{}: volume must be a {} volume on {}'.format(who, self.shape, self.device))
        lam, iterations, w_sat, tau, sigma = solver_options(who, lam, iterations, w_sat, tau, sigma)
        if not restart and self._volume is None:
            raise ValueError('{}: restart=False before any restart'.format(who))
        if not restart and volume is not self._volume:
            raise ValueError('{}: restart=False on another volume than the one the state was made for'.format(who))
        lib, stream = _lib.load(), _lib.stream_ptr(self.device)
        if restart:
            self._volume = None  # (a refusal below leaves no state to continue from)
            rc = lib.ojf_label_tv_setup(_lib.ptr(volume), self.n_classes, *self.shape, _lib.ptr(self.workspace), self.workspace.numel(),
                                        _lib.ptr(self._count_dev), stream)
            _lib.check(rc, 'ojf_label_tv_setup')
            self.count = int(self._count_dev.item())
            if self.count > self.capacity:
                setup = self.workspace[:self.layout['u']]
                self._allocate(self.count)
                self.workspace[:self.layout['u']].copy_(setup)  # (the set-up pass's part is the head of every workspace)
        rc = lib.ojf_label_tv_solve(_lib.ptr(volume), self.n_classes, *self.shape, lam, w_sat, tau, sigma, iterations,
                                    _lib.LABEL_TV_RESTART if restart else _lib.LABEL_TV_CONTINUE, self.capacity, _lib.ptr(self.workspace),
                                    self.workspace.numel(), _lib.ptr(self.status), stream)
        _lib.check(rc, 'ojf_label_tv_solve')
        self._volume = volume

    def write(self, ids, scores, probs_out=None):
        """ids (cuda u8 [X,Y,Z]) = the first class of the largest u_k and scores (cuda fp16 [X,Y,Z]) = that u_k at the observed
        voxels of the volume the last ``solve`` ran on, in place; with ``probs_out`` (a label volume of the same class count;
        the solved volume itself is allowed) its class channels = u, W copied.  The other voxels keep what they hold."""
        who = 'label_tv.Solver.write'
        if self._volume is None:
            raise ValueError('{}: nothing was solved yet'.format(who))
        views.volume3(who, ids, 'ids', torch.uint8, self.shape, self.device)
        views.volume3(who, scores, 'scores', torch.float16, self.shape, self.device)
        if probs_out is not None and (tuple(label_probs._volume(probs_out, self.n_classes, who)) != self.shape
                                      or probs_out.device != self.device):
            raise ValueError('{}: probs_out must be a {} volume on {}'.format(who, self.shape, self.device))
        rc = _lib.load().ojf_label_tv_write(_lib.ptr(self._volume), self.n_classes, *self.shape, _lib.ptr(self.workspace),
                                            self.workspace.numel(), _lib.ptr(ids), _lib.ptr(scores), _lib.ptr(probs_out),
                                            _lib.stream_ptr(self.device))
        _lib.check(rc, 'ojf_label_tv_write')

    def _part(self, name, dtype, count):
        size = torch.empty(0, dtype=dtype).element_size()
        return self.workspace[self.layout[name]:self.layout[name] + size * count].view(dtype)

    def class_field(self, k):
        """u_k scattered into a dense f32 [X,Y,Z] (0 at unobserved voxels): for tests and inspection, by torch indexing from the
        brick list."""
        k = int(k)
        if self._volume is None or not 0 <= k < self.n_classes:
            raise ValueError('label_tv.Solver.class_field: a solved state and 0 <= k < {} expected'.format(self.n_classes))
        L, (bx, by, bz) = self.layout, self.layout['bricks']
        dense = torch.zeros((L['n_bricks'],) + BRICK, dtype=torch.float32, device=self.device)
        if self.count:
            bricks = self._part('list', torch.int32, L['n_bricks'])[:self.count].long()
            flags = self._part('flags', torch.uint8, L['n_bricks'] * BRICK_VOXELS).view((L['n_bricks'],) + BRICK)[bricks]
            u = self._part('u', torch.float32, L['plane']).view((self.capacity, self.n_classes) + BRICK)[:self.count, k]
            dense[bricks] = torch.where((flags & OBSERVED) != 0, u, torch.zeros_like(u))
        dense = dense.view(bx, by, bz, *BRICK).permute(0, 3, 1, 4, 2, 5).reshape(bx * BRICK[0], by * BRICK[1], bz * BRICK[2])
        X, Y, Z = self.shape
        return dense[:X, :Y, :Z].contiguous()
