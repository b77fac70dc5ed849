"""Relocalise a lost camera: keyframes coded by randomised ferns beside the tracker (Glocker et al. 2013, as InfiniTAM and
ElasticFusion use them).  A frame's code is M four-bit ferns over a coarse code image of the frame (cell means of depth,
and of colour where asked for); a ``Relocalizer`` keeps the codes and poses of harvested keyframes on the device, finds
the keyframes nearest to a frame in code space, and ``relocalize_frame`` hands their poses to ``tracking.track_frame`` as
starts.  The kernels are csrc/ojf_reloc.hip (``ojf_reloc_encode``, ``ojf_reloc_query``, ``ojf_reloc_insert``); their
definition is written in that file's header and restated in numpy by tests/reloc_ref.py.  The reference has no counterpart:
it takes every pose from its dataset.
"""
import math

import numpy as np
import torch

from . import views

MAX_CELLS, MAX_FERNS, MAX_K = 1024, 4096, 16  # csrc/ojf_reloc.hip kRelocMaxCells / kRelocMaxFerns / kRelocMaxK
STATUS_NO_CANDIDATE = 4  # beside tracking's 0..3: no keyframe gave a pose


def fern_table(seed, n_ferns, cells, color=False, depth_range=(0.2, 4.0)):
    """The host table of ``n_ferns`` ferns over ``cells`` cells: {'cell' i32 [M,4], 'channel' u8 [M,4], 'threshold' f32
    [M,4]}.  One ``np.random.default_rng(seed)``: cell indices, then depth thresholds uniform in ``depth_range``; with
    ``color`` two further draws follow - the channel 0..3 of every decision and a threshold in 0..255 for the decisions that
    fell on a colour channel - so the depth-only table is what the colour table is drawn on top of."""
    M, cells = int(n_ferns), int(cells)
    if not (8 <= M <= MAX_FERNS and M % 8 == 0):
        raise ValueError('fern_table: n_ferns must be a multiple of 8 in 8..{}, got {}'.format(MAX_FERNS, n_ferns))
    if not 1 <= cells <= MAX_CELLS:
        raise ValueError('fern_table: cells must be 1..{}, got {}'.format(MAX_CELLS, cells))
    lo, hi = (float(x) for x in depth_range)
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
        raise ValueError('fern_table: a finite depth_range (lo <= hi) expected, got {!r}'.format(depth_range))
    r = np.random.default_rng(seed)
    pos = r.integers(0, cells, (M, 4))
    thr = r.uniform(lo, hi, (M, 4)).astype(np.float32)
    ch = np.zeros((M, 4), dtype=np.uint8)
    if color:
        ch = r.integers(0, 4, (M, 4)).astype(np.uint8)
        thr = np.where(ch == 0, thr, r.uniform(0.0, 255.0, (M, 4)).astype(np.float32))
    return {'cell': np.ascontiguousarray(pos, dtype=np.int32), 'channel': np.ascontiguousarray(ch),
            'threshold': np.ascontiguousarray(thr, dtype=np.float32)}


def _poses12(who, extrinsics, n):
    """f64 [n,12] of [3,4] / [4,4] / [n,3,4] / [n,4,4] camera-to-world poses (numpy or torch); finite."""
    E = torch.as_tensor(extrinsics).detach().cpu().to(torch.float64)
    if E.dim() == 2:
        E = E.unsqueeze(0)
    if E.dim() != 3 or E.shape[0] != n or E.shape[-1] != 4 or E.shape[-2] not in (3, 4):
        raise ValueError('{}: extrinsics [n,]3x4 or 4x4 for {} frames expected, got {}'.format(who, n, tuple(E.shape)))
    E = np.ascontiguousarray(E[:, :3, :].reshape(n, 12).numpy())
    if not np.isfinite(E).all():
        raise ValueError('{}: non-finite extrinsics'.format(who))
    return E


class Relocalizer:
    """The fern table of one frame size and a keyframe store on ``device``: ``codes`` i32 [capacity, M/8] (the u32 words),
    ``poses`` f64 [capacity, 12], ``count`` i32 [1].  The count lives on the device: ``add`` never reads it back."""

    def __init__(self, h, w, *, device, cell=None, n_ferns=512, seed=1911, color=False, capacity=4096, min_dissimilarity=0.1,
                 depth_range=(0.2, 4.0)):
        who = 'Relocalizer'
        self.h, self.w = int(h), int(w)
        self.cell = max(1, self.w // 16) if cell is None else int(cell)
        if self.h < 1 or self.w < 1 or not 1 <= self.cell <= 64 or self.h < self.cell or self.w < self.cell:
            raise ValueError('{}: a cell of 1..64 pixels no larger than the {}x{} frame expected, got {}'.format(who, self.h, self.w, self.cell))
        self.CH, self.CW = self.h // self.cell, self.w // self.cell
        if self.CH * self.CW > MAX_CELLS:
            raise ValueError('{}: {} cells, at most {}: choose a larger cell'.format(who, self.CH * self.CW, MAX_CELLS))
        self.n_ferns, self.seed, self.color = int(n_ferns), int(seed), bool(color)
        self.capacity = int(capacity)
        if not 1 <= self.capacity <= 2 ** 24:
            raise ValueError('{}: capacity must be 1..2^24, got {}'.format(who, capacity))
        self.min_dissimilarity = float(min_dissimilarity)
        if not 0.0 <= self.min_dissimilarity <= 1.0:
            raise ValueError('{}: min_dissimilarity must be in 0..1, got {}'.format(who, min_dissimilarity))
        self.depth_range = tuple(float(x) for x in depth_range)
        self.table = fern_table(self.seed, self.n_ferns, self.CH * self.CW, self.color, self.depth_range)
        self.min_differ = int(math.floor(self.min_dissimilarity * self.n_ferns))
        self.words = self.n_ferns // 8
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise ValueError('{}: a cuda device expected, got {}'.format(who, device))
        from . import _lib
        _lib.require_gpu()
        self._lib = _lib
        self.device = torch.empty(0, device=self.device).device  # ('cuda' -> the indexed device its tensors report)
        self._table_dev = {k: torch.from_numpy(v).to(self.device) for k, v in self.table.items()}
        self.codes = torch.zeros((self.capacity, self.words), dtype=torch.int32, device=self.device)
        self.poses = torch.zeros((self.capacity, 12), dtype=torch.float64, device=self.device)
        self.count = torch.zeros(1, dtype=torch.int32, device=self.device)

    def __len__(self):
        return int(self.count.item())

    def _frames(self, who, depth, mask, image):
        depth = views.depth_frames(who, depth, self.device)
        n, h, w = depth.shape
        if (h, w) != (self.h, self.w):
            raise ValueError('{}: frames of {}x{} expected, got {}x{}'.format(who, self.h, self.w, h, w))
        mask = views.images(who, mask, 'mask', torch.uint8, n, h, w, self.device)
        if self.color:
            if image is None:
                raise ValueError('{}: a colour table needs the frames\' images'.format(who))
            from . import color
            image = color.pack_image(image, n, h, w, self.device)
        else:
            image = None
        return depth, mask, image, n

    def encode(self, depth, mask=None, image=None, code_image=False):
        """The codes i32 [n, M/8] (u32 words) of ``n`` frames, on the device and without synchronising: depth [h,w] or
        [n,h,w], mask bool / u8 or None, image as ``color.pack_image`` takes it (read only by a colour table).
        ``code_image``: return (codes, f32 [n,4,CH,CW]) instead."""
        _lib = self._lib
        depth, mask, image, n = self._frames('Relocalizer.encode', depth, mask, image)
        codes = torch.empty((n, self.words), dtype=torch.int32, device=self.device)
        ci = torch.empty((n, 4, self.CH, self.CW), dtype=torch.float32, device=self.device) if code_image else None
        t = self._table_dev
        rc = _lib.load().ojf_reloc_encode(_lib.ptr(depth), _lib.ptr(mask), _lib.ptr(image), n, self.h, self.w, self.cell, self.n_ferns,
                                          _lib.ptr(t['cell']), _lib.ptr(t['channel']), _lib.ptr(t['threshold']), _lib.ptr(codes),
                                          _lib.ptr(ci), _lib.stream_ptr(self.device))
        _lib.check(rc, 'ojf_reloc_encode')
        return (codes, ci) if code_image else codes

    def add(self, depth, extrinsics, mask=None, image=None, force=False):
        """Offer ``n`` frames with their camera-to-world poses to the store, in order: a frame becomes a keyframe when
        ``force``, or the store is empty, or its nearest keyframe differs in more than ``min_dissimilarity`` of the ferns.
        Returns device tensors {'added' i32 [n] (1 added, 0 too similar, 2 the store is full), 'best' i64 [n] (the nearest
        keyframe's key differ << 32 | index as the frame met the store; -1: it was empty)} without synchronising."""
        _lib = self._lib
        codes = self.encode(depth, mask, image)
        n = codes.shape[0]
        poses = torch.from_numpy(_poses12('Relocalizer.add', extrinsics, n)).to(self.device)
        best = torch.empty(n, dtype=torch.int64, device=self.device)
        added = torch.empty(n, dtype=torch.int32, device=self.device)
        rc = _lib.load().ojf_reloc_insert(_lib.ptr(codes), _lib.ptr(poses), n, self.n_ferns, self.min_differ, int(bool(force)),
                                          _lib.ptr(self.codes), _lib.ptr(self.poses), _lib.ptr(self.count), self.capacity,
                                          _lib.ptr(best), _lib.ptr(added), _lib.stream_ptr(self.device))
        _lib.check(rc, 'ojf_reloc_insert')
        return {'added': added, 'best': best}

    def query(self, depth, mask=None, image=None, k=4):
        """The ``k`` nearest keyframes of ``n`` frames: {'index' i64 [n,k] (-1: none), 'dissimilarity' f64 [n,k] (the share
        of ferns that differ; inf where none), 'extrinsics' f64 [n,k,4,4] (identity where none), 'keys' i64 [n,k] (the
        kernel's keys; -1 where none)}, nearest first, equal codes smallest index first.  One copy back."""
        _lib = self._lib
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError('Relocalizer.query: k must be 1..{}, got {}'.format(MAX_K, k))
        codes = self.encode(depth, mask, image)
        n = codes.shape[0]
        keys = torch.empty((n, k), dtype=torch.int64, device=self.device)
        rc = _lib.load().ojf_reloc_query(_lib.ptr(codes), n, self.n_ferns, _lib.ptr(self.codes), _lib.ptr(self.count), self.capacity, k,
                                         _lib.ptr(keys), _lib.stream_ptr(self.device))
        _lib.check(rc, 'ojf_reloc_query')
        index = torch.where(keys < 0, torch.full_like(keys, -1), keys & 0xffffffff)
        poses = self.poses[index.clamp(min=0)]  # [n,k,12]
        # keys and poses in one f64 buffer: one copy back
        host = torch.cat([keys.view(torch.float64).reshape(n, k, 1), poses], dim=2).cpu()
        keys_h = host[:, :, 0].contiguous().view(torch.int64).numpy()
        none = keys_h < 0
        idx = np.where(none, -1, keys_h & 0xffffffff)
        E = np.zeros((n, k, 4, 4), dtype=np.float64)
        E[..., :3, :] = host[:, :, 1:].numpy().reshape(n, k, 3, 4)
        E[..., 3, 3] = 1.0
        E[none] = np.eye(4)
        return {'index': idx, 'dissimilarity': np.where(none, np.inf, (keys_h >> 32) / float(self.n_ferns)), 'extrinsics': E,
                'keys': keys_h}

    def state(self):
        """The store and the constructor's arguments as numpy arrays (``np.savez(path, **state)``)."""
        n = len(self)
        return {'codes': self.codes[:n].cpu().numpy().view(np.uint32), 'poses': self.poses[:n].cpu().numpy(),
                'count': np.array([n], dtype=np.int32), 'h': np.array(self.h), 'w': np.array(self.w), 'cell': np.array(self.cell),
                'n_ferns': np.array(self.n_ferns), 'seed': np.array(self.seed), 'color': np.array(self.color),
                'capacity': np.array(self.capacity), 'min_dissimilarity': np.array(self.min_dissimilarity),
                'depth_range': np.array(self.depth_range, dtype=np.float64)}

    @classmethod
    def from_state(cls, state, device):
        """The ``Relocalizer`` a ``state()`` was taken from, on ``device``: a saved scene can be relocalised in."""
        r = cls(int(state['h']), int(state['w']), device=device, cell=int(state['cell']), n_ferns=int(state['n_ferns']),
                seed=int(state['seed']), color=bool(state['color']), capacity=int(state['capacity']),
                min_dissimilarity=float(state['min_dissimilarity']), depth_range=tuple(np.asarray(state['depth_range']).tolist()))
        n = int(np.asarray(state['count']).reshape(-1)[0])
        codes = np.ascontiguousarray(state['codes']).view(np.int32).reshape(-1, r.words)
        poses = np.ascontiguousarray(state['poses'], dtype=np.float64).reshape(-1, 12)
        if not (0 <= n <= r.capacity and codes.shape[0] == n and poses.shape[0] == n):
            raise ValueError('Relocalizer.from_state: {} keyframes, {} codes and {} poses for a capacity of {}'.format(
                n, codes.shape[0], poses.shape[0], r.capacity))
        if n:
            r.codes[:n] = torch.from_numpy(codes).to(r.device)
            r.poses[:n] = torch.from_numpy(poses).to(r.device)
        r.count.fill_(n)
        return r


def relocalize_frame(tsdf, weights, reloc, *, origin, resolution, depth, intrinsics, mask=None, image=None, colors=None, k=4,
                     max_dissimilarity=None, **track_kw):
    """The pose of a frame that has none: the ``k`` keyframes of ``reloc`` nearest to the frame, those beyond
    ``max_dissimilarity`` (a share of the ferns; None: no cut) dropped, each tried as the start and the reference pose of
    ``tracking.track_frame`` - of ``track_frame_rgbd`` with ``colors`` and ``image`` - which ``track_kw`` goes to.  The winner
    is the ``ok`` candidate with the most inliers in the last row of its 'stats' (ties: the smaller mean squared residual,
    then candidate order).  Returns its dict plus 'candidate' (the keyframe's index; -1: none) and 'candidates' (a list of
    {'index', 'dissimilarity', 'result'}); with no ``ok`` candidate {'ok': False, 'status': 4, 'extrinsics': identity,
    'stats': f64 [0,4]}."""
    from . import tracking
    dev = tsdf.device
    d = torch.as_tensor(depth).to(device=dev, dtype=torch.float32)
    d = d.reshape(d.shape[-2:])
    m = None if mask is None else torch.as_tensor(mask).to(dev).reshape(d.shape)
    img = None if image is None else torch.as_tensor(image).to(dev)
    if img is not None and img.dim() == 4 and img.shape[0] == 1:
        img = img[0]
    near = reloc.query(d, mask=m, image=img, k=k)
    rgbd = colors is not None and img is not None
    candidates, best = [], None
    for j in range(near['index'].shape[1]):
        index, dis = int(near['index'][0, j]), float(near['dissimilarity'][0, j])
        if index < 0 or (max_dissimilarity is not None and dis > float(max_dissimilarity)):
            continue
        E = near['extrinsics'][0, j]
        kw = dict(origin=origin, resolution=resolution, depth=d, intrinsics=intrinsics, extrinsics=E, reference_extrinsics=E, mask=m,
                  **track_kw)
        res = tracking.track_frame_rgbd(tsdf, weights, colors, image=img, **kw) if rgbd else tracking.track_frame(tsdf, weights, **kw)
        candidates.append({'index': index, 'dissimilarity': dis, 'result': res})
        if res['ok'] and len(res['stats']):
            score = (-res['stats'][-1, 0], res['stats'][-1, 1])
            if best is None or score < best[0]:
                best = (score, index, res)
    if best is None:
        return {'extrinsics': np.eye(4), 'ok': False, 'status': STATUS_NO_CANDIDATE, 'stats': np.zeros((0, 4)), 'candidate': -1,
                'candidates': candidates}
    return dict(best[2], candidate=best[1], candidates=candidates)
