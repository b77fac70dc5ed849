"""Per-scene volume store: counterpart of the reference's ``modules/database.py`` Database.

Same constructor, attributes and methods, with one deliberate difference in
*where* the state lives: the four volumes of every scene (TSDF fp16, weights fp16, semantic ids
u8, semantic scores fp16) are HIP device tensors resident in HBM for the whole stream, the GT
volumes included (the reference re-uploads the GT grid every training frame, extractor.py:47).
Pipeline mutates them in place.  ``to_numpy()`` moves the state to the host exactly like the
reference's (database.py:383-393), after which ``filter`` / ``evaluate`` run on numpy arrays;
while the state is on the device they run as HIP kernels (ojf_volume_*).
"""
import contextlib
import os

import numpy as np
import torch

from . import ops
from .metrics import evaluation, semantic_evaluation, semantic_metrics_from_counts


class Voxelgrid:
    """The 30 lines of deps/graphics' Voxelgrid the hot path uses (voxelgrid.py:157-161)."""

    def __init__(self, resolution):
        self.resolution = resolution
        self.volume = None
        self.bbox = None
        self.origin = None

    def from_array(self, array, bbox):
        self.volume = array
        self.bbox = np.asarray(bbox, dtype=np.float64)
        self.origin = self.bbox[:, 0].copy()

    @property
    def shape(self):
        return self.volume.shape


def _is_dev(v):
    return torch.is_tensor(v) and v.is_cuda


def _to_dev(x, device):
    return None if x is None else torch.as_tensor(x).to(device)


def _filtered(depth, mask, intrinsics, filter):
    """(depth, mask) of a call's ``filter=`` dict: the device frames through frames.prepare_depth, the validity as the mask."""
    from . import frames
    return frames.filtered(depth, mask, intrinsics, filter)


class Database(torch.utils.data.Dataset):

    def __init__(self, dataset, config):
        super().__init__()
        self.device = torch.device(config.device)
        self.implementation = config.implementation
        self.transform = config.transform
        self.initial_value = config.init_value
        self.semantics = config.semantics
        self.semantic_grid = config.semantic_grid
        self.pad = config.pad
        if self.semantics:
            self.n_classes = config.n_classes

        self.scenes = []
        self.state = {}  # True once a scene's grid holds integrated frames
        self.origin, self.resolution = {}, {}
        self.scenes_gt, self.scenes_est, self.fusion_weights = {}, {}, {}
        self.ids_gt, self.ids_est, self.scores = {}, {}, {}
        self.colors = {}  # scene -> fp16 [X,Y,Z,4] colour volume (color.py), only for scenes integrate_color was called on
        self.label_probs = {}  # scene -> fp16 [X,Y,Z,S] class distribution (label_probs.py), only for scenes integrate_label_probs was called on
        self.depth_hists = {}  # scene -> (fp16 [X,Y,Z,S] depth histograms, n_bins) (tvl1.py), only for scenes integrate_depth_hist was called on
        self._tvl1_solvers = {}  # scene -> tvl1.Solver: u and the workspace of regularize, kept for warm starts
        self._tvl1_changed = set()  # scenes whose histograms took views since their solver last ran
        self._label_tv_solvers = {}  # scene -> label_tv.Solver: the workspace of regularize_labels, kept for the next call
        self.tracked_poses = {}  # frame_id -> f64 [4,4] camera-to-world: frames fused with a tracked pose (drivers.test_fusion)
        self.relocalizers = {}  # scene -> relocalize.Relocalizer: the keyframes of add_keyframe, made on first use
        self.relocalizer_options = dict(config.get('relocalizer', None) or {})  # Relocalizer keywords (TESTING.relocalizer)
        self.relocalized = []  # frame ids fused with a pose that came from a keyframe (drivers.test_fusion)

        for s in dataset.scenes:
            self.scenes.append(s)
            try:
                grid = dataset.get_grid(s, self.initial_value, self.semantic_grid)
            except Exception:  # no ground truth available (database.py:52-53)
                grid = dataset.create_grid(s, self.initial_value)
            self.state[s] = False
            self.scenes_gt[s] = grid[0]
            self.origin[s] = np.asarray(grid[0].origin, dtype=np.float64)
            self.resolution[s] = grid[0].resolution
            shape = tuple(grid[0].volume.shape)
            self.scenes_est[s] = Voxelgrid(grid[0].resolution)
            self.scenes_est[s].from_array(np.full(shape, self.initial_value, dtype=np.float16), grid[0].bbox)
            self.fusion_weights[s] = np.zeros(shape, dtype=np.float16)
            if self.semantics:
                if self.semantic_grid:
                    self.ids_gt[s] = grid[1]
                self.ids_est[s] = Voxelgrid(grid[0].resolution)
                self.ids_est[s].from_array(np.zeros(shape, dtype=np.uint8), grid[0].bbox)
                self.scores[s] = Voxelgrid(grid[0].resolution)
                self.scores[s].from_array(np.zeros(shape, dtype=np.float16), grid[0].bbox)
        self.to_torch()

    # ---- access ---------------------------------------------------------------------------
    def __getitem__(self, item):
        sample = {'origin': self.origin[item], 'resolution': self.resolution[item],
                  'gt': self.scenes_gt[item].volume, 'current': self.scenes_est[item].volume,
                  'weights': self.fusion_weights[item]}
        if self.semantics:
            sample['ids_est'] = self.ids_est[item].volume
            sample['scores'] = self.scores[item].volume
            if self.semantic_grid:
                sample['ids_gt'] = self.ids_gt[item].volume
        else:
            sample.update(histograms=None, ids_est=None, ids_gt=None, scores=None)
        if self.colors.get(item) is not None:
            sample['colors'] = self.colors[item]
        if self.label_probs.get(item) is not None:
            sample['label_probs'] = self.label_probs[item]
        if self.depth_hists.get(item) is not None:
            sample['depth_hist'] = self.depth_hists[item][0]
        return sample

    def __len__(self):
        return len(self.scenes_gt)

    # ---- residency ------------------------------------------------------------------------
    def _dev(self, a):
        if torch.is_tensor(a):
            return a.to(self.device).contiguous()
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def to_torch(self, gt=True, scenes=None):
        scenes = self.scenes if scenes is None else [scenes]
        for s in scenes:
            self.scenes_est[s].volume = self._dev(self.scenes_est[s].volume)
            self.fusion_weights[s] = self._dev(self.fusion_weights[s])
            if self.colors.get(s) is not None:
                self.colors[s] = self._dev(self.colors[s])
            if self.label_probs.get(s) is not None:
                self.label_probs[s] = self._dev(self.label_probs[s])
            if self.depth_hists.get(s) is not None:
                self.depth_hists[s] = (self._dev(self.depth_hists[s][0]), self.depth_hists[s][1])
            if gt:
                o = self.origin[s]
                self.origin[s] = o.double().cpu() if torch.is_tensor(o) else torch.from_numpy(np.asarray(o, np.float64))
                self.scenes_gt[s].volume = self._dev(self.scenes_gt[s].volume)
            if self.semantics:
                self.ids_est[s].volume = self._dev(self.ids_est[s].volume)
                self.scores[s].volume = self._dev(self.scores[s].volume)
                if gt and self.semantic_grid:
                    self.ids_gt[s].volume = self._dev(self.ids_gt[s].volume)

    def to_numpy(self):
        def host(a):
            return a.detach().cpu().numpy() if torch.is_tensor(a) else a
        for s in self.scenes:
            self.origin[s] = host(self.origin[s])
            self.scenes_est[s].volume = host(self.scenes_est[s].volume)
            self.scenes_gt[s].volume = host(self.scenes_gt[s].volume)
            self.fusion_weights[s] = host(self.fusion_weights[s])
            if self.colors.get(s) is not None:
                self.colors[s] = host(self.colors[s])
            if self.label_probs.get(s) is not None:
                self.label_probs[s] = host(self.label_probs[s])
                self._label_tv_solvers.pop(s, None)
            if self.depth_hists.get(s) is not None:
                self.depth_hists[s] = (host(self.depth_hists[s][0]), self.depth_hists[s][1])
                self._tvl1_solvers.pop(s, None)  # (the solver's state is not carried to the host: the next regularize restarts)
            if self.semantics:
                self.ids_est[s].volume = host(self.ids_est[s].volume)
                self.scores[s].volume = host(self.scores[s].volume)
                if self.semantic_grid:
                    self.ids_gt[s].volume = host(self.ids_gt[s].volume)

    def reset(self, scene_id=None):
        """database.py:351-370; device volumes are re-filled in place by a HIP kernel instead of
        being re-allocated on the host and uploaded."""
        for s in ([scene_id] if scene_id else self.scenes):
            self.state[s] = False
            self.relocalizers.pop(s, None)  # (keyframes of a volume that is gone)
            c = self.colors.get(s)
            if _is_dev(c):
                ops.volume_fill(c, 0.0)
            elif c is not None:
                self.colors[s] = np.zeros(c.shape, dtype=np.float16)  # (a host volume; goes up with the rest below)
            p = self.label_probs.get(s)
            if _is_dev(p):
                ops.volume_fill(p, 0.0)
            elif p is not None:
                self.label_probs[s] = np.zeros(p.shape, dtype=np.float16)
            self._label_tv_solvers.pop(s, None)
            if self.depth_hists.get(s) is not None:
                hist, n_bins = self.depth_hists[s]
                if _is_dev(hist):
                    ops.volume_fill(hist, 0.0)
                else:
                    self.depth_hists[s] = (np.zeros(hist.shape, dtype=np.float16), n_bins)
                self._tvl1_solvers.pop(s, None)
            if _is_dev(self.scenes_est[s].volume):
                ops.volume_fill(self.scenes_est[s].volume, self.initial_value)
                ops.volume_fill(self.fusion_weights[s], 0.0)
                if self.semantics:
                    ops.volume_fill(self.ids_est[s].volume, 0)
                    ops.volume_fill(self.scores[s].volume, 0.0)
            else:
                shape = self.scenes_est[s].volume.shape
                self.scenes_est[s].volume = np.full(shape, self.initial_value, dtype=np.float16)
                self.fusion_weights[s] = np.zeros(shape, dtype=np.float16)
                if self.semantics:
                    self.ids_est[s].volume = np.zeros(shape, dtype=np.uint8)
                    self.scores[s].volume = np.zeros(shape, dtype=np.float16)
                self.to_torch(gt=False, scenes=s)

    def remove(self, scene_id):
        self.state[scene_id] = False
        self.scenes_est[scene_id] = None
        self.scenes_gt[scene_id] = None
        self.fusion_weights[scene_id] = None
        self.colors.pop(scene_id, None)
        self.label_probs.pop(scene_id, None)
        self.depth_hists.pop(scene_id, None)
        self._tvl1_solvers.pop(scene_id, None)
        self._label_tv_solvers.pop(scene_id, None)
        self.relocalizers.pop(scene_id, None)
        if self.semantics:
            self.ids_est[scene_id] = None
            self.scores[scene_id] = None
            if self.semantic_grid:
                self.ids_gt[scene_id] = None

    # ---- post-processing ------------------------------------------------------------------
    def filter(self, value=2.):
        """Outlier filter (database.py:108-112): where weights < value: tsdf = init, weights = 0."""
        for s in self.scenes:
            w = self.fusion_weights[s]
            if _is_dev(w):
                ops.volume_filter(self.scenes_est[s].volume, w, value, self.initial_value)
            else:
                low = w < value
                self.scenes_est[s].volume[low] = self.initial_value
                self.fusion_weights[s][low] = 0

    def filter_semantics(self, value=5):
        """database.py:114-116: median filter of the label volume (on device for the reference's size 5)."""
        for s in self.scenes:
            v = self.ids_est[s].volume
            if _is_dev(v) and value == 5:
                self.ids_est[s].volume = ops.volume_median5(v)
            else:
                from scipy.ndimage import median_filter
                host = v.cpu().numpy() if torch.is_tensor(v) else v
                res = median_filter(host, size=value)
                self.ids_est[s].volume = torch.from_numpy(res).to(v.device) if torch.is_tensor(v) else res

    def filter_components(self, min_voxels=None, keep_largest=None, connectivity=26, band=None):
        """Floater filter (components.remove_small_components; no counterpart in the reference): in every scene, the connected
        components of the observed voxels (within ``band`` of the surface, if given) that are smaller than ``min_voxels`` - or
        all but the ``keep_largest`` largest - go back to the initial value and weight 0, as ``filter`` leaves a voxel.  Touches
        the same two volumes as ``filter``; host state is refused.  Returns {scene: the component list with the keep flags}."""
        from . import components
        components.keep_flags([], [], min_voxels, keep_largest, 'Database.filter_components')
        for s in self.scenes:
            self._resident(s, 'filter_components', self.scenes_est[s].volume, self.fusion_weights[s])
        return {s: components.remove_small_components(self.scenes_est[s].volume, self.fusion_weights[s], init_value=self.initial_value,
                                                      min_voxels=min_voxels, keep_largest=keep_largest, connectivity=connectivity, band=band)
                for s in self.scenes}

    def instances(self, scene_id, connectivity=6, min_voxels=1):
        """3-D instances of a scene (components.instances): the connected components of equal labels of ids_est among the
        observed voxels.  Returns {'ids' i32 [X,Y,Z] on the device (-1: no instance), 'n', 'roots', 'sizes', 'classes',
        'boxes'}; components of fewer than ``min_voxels`` voxels are dropped and the rest renumbered densely in root order."""
        from . import components
        if not self.semantics:
            raise ValueError('Database.instances: the database has no semantics (ids_est)')
        tsdf, w, ids = self.scenes_est[scene_id].volume, self.fusion_weights[scene_id], self.ids_est[scene_id].volume
        self._resident(scene_id, 'instances', tsdf, w, ids)
        return components.instances(ids, tsdf, w, connectivity=connectivity, min_voxels=min_voxels)

    def esdf(self, scene_id, max_distance=None):
        """Euclidean signed distance field of a scene (distance.esdf; f32 [X,Y,Z] on the device, metres): the distance of every
        voxel to the nearest surface voxel of the estimated volume, negative inside, capped at ``max_distance``.  Reads the
        TSDF and the weights and writes no volume of the scene; host state is refused."""
        from . import distance
        tsdf, w = self.scenes_est[scene_id].volume, self.fusion_weights[scene_id]
        self._resident(scene_id, 'esdf', tsdf, w)
        return distance.esdf(tsdf, w, float(self.resolution[scene_id]), max_distance)

    def evaluate(self, mode='train', workspace=None):
        """database.py:265-309 (note: averages over ALL scenes, untouched ones included, :304)."""
        results, per_scene = {}, {}
        for s in self.scenes:
            if not self.state[s]:
                continue
            est, gt, w = self.scenes_est[s].volume, self.scenes_gt[s].volume, self.fusion_weights[s]
            if _is_dev(est):
                r = ops.volume_evaluate(est, gt, w)
            else:
                r = evaluation(est, gt, w > 0)
            per_scene[s] = r
            for k, v in r.items():
                msg = '{} {}'.format(k, v)
                workspace.log(msg, mode) if workspace is not None else print(msg)
                results[k] = results.get(k, 0) + v
        for k in results:
            results[k] /= len(self.scenes_est.keys())
        return (results, per_scene) if mode == 'test' else results

    def evaluate_semantics(self, mode='train', workspace=None):
        """database.py:311-349.  Device-resident volumes are reduced to the C x C confusion counts by one HIP pass
        (ojf_volume_confusion, 5 B/voxel); only those counts come to the host."""
        results, per_scene = {}, {}

        def host(a):
            return a.detach().cpu().numpy() if torch.is_tensor(a) else a
        for s in self.scenes:
            if not self.state[s]:
                continue
            est, gt, w = self.ids_est[s].volume, self.ids_gt[s].volume, self.fusion_weights[s]
            if _is_dev(est) and _is_dev(w):
                gt_dev = gt if _is_dev(gt) else self._device_volume(gt, torch.uint8)
                hist, e_ids, g_ids = ops.volume_confusion(est, gt_dev, w, self.n_classes)
                n = self.n_classes  # np.bincount(np.unique(x), minlength=n): at least n entries, more if a label >= n occurs
                e_ids = e_ids[:max(n, int(np.flatnonzero(e_ids).max(initial=0)) + 1)]
                g_ids = g_ids[:max(n, int(np.flatnonzero(g_ids).max(initial=0)) + 1)]
                k = max(len(e_ids), len(g_ids))
                e_ids, g_ids = np.pad(e_ids, (0, k - len(e_ids))), np.pad(g_ids, (0, k - len(g_ids)))
                r, cls_iou = semantic_metrics_from_counts(hist, e_ids, g_ids)
            else:
                r, cls_iou = semantic_evaluation(host(est), host(gt), host(w) > 0, self.n_classes)
            per_scene[s] = cls_iou
            for k, v in r.items():
                msg = '{} {}'.format(k, v)
                workspace.log(msg, mode) if workspace is not None else print(msg)
                results[k] = results.get(k, 0) + v
        for k in results:
            results[k] /= len(self.scenes_est.keys())
        return results, per_scene

    # ---- IO: volumes as hdf (or npy), meshes as ply from the HIP marching-tetrahedra kernel (mesh.py) ---
    def _device_volume(self, vol, dtype):
        if not torch.is_tensor(vol):
            vol = torch.from_numpy(np.ascontiguousarray(vol))
        return vol.to(device='cuda', dtype=dtype).contiguous()

    def _resident(self, scene_id, who, *volumes, optional=()):
        """Refuse host state: ``volumes``, and those of ``optional`` that exist, must be on the device."""
        if not all(_is_dev(v) for v in volumes + tuple(v for v in optional if v is not None)):
            raise ValueError('Database.{}: the volumes of {!r} are not resident on the device (to_torch())'.format(who, scene_id))

    @staticmethod
    @contextlib.contextmanager
    def _side_volume(store, scene_id, make):
        """A scene's side volume in ``store`` (colors, label_probs) for the call in the ``with`` body: the stored one, or
        ``make()`` on first use, which is kept only if the body went through - a refused call leaves a scene without a side
        volume without one."""
        vol = store.get(scene_id)
        if vol is None:
            vol = make()
        yield vol  # (a refusal in the body leaves from here)
        store[scene_id] = vol

    def _color_volume(self, scene_id, who):
        if self.colors.get(scene_id) is None:
            raise ValueError('Database.{}: scene {!r} has no colour volume (integrate_color)'.format(who, scene_id))
        return self._device_volume(self.colors[scene_id], torch.float16)

    def _vertex_colors(self, scene_id, vertices, who):
        """u8 [V,4] colours (alpha 255 where coloured) of mesh-frame vertices: a vertex at v sits at voxel index v / resolution."""
        from . import color
        if len(vertices) == 0:
            return np.zeros((0, 4), dtype=np.uint8)
        g = np.asarray(vertices, dtype=np.float32) / np.float32(self.resolution[scene_id])  # (one fp32 division per coordinate)
        return color.sample_color(self._color_volume(scene_id, who), g).cpu().numpy()

    def get_mesh(self, scene_id, semantics=False, palette=None, color=False, simplify=None):
        """database.py:118-139: (vertices, faces, normals, rgb) of the zero level set of the estimated volume in
        the reference's mesh frame (voxel index * voxel size, no origin).  Marching tetrahedra instead of skimage's
        marching cubes: same surface, different triangulation (mesh.py).  color=True: rgb is what the scene's colour
        volume holds at the vertices (color.sample_color), in [0,1] and the images' channel order, 0 where nothing is
        coloured.  simplify: None, or the cell size in voxels of the quadric vertex clustering (mesh_simplify.py) the mesh
        goes through before it leaves the device."""
        from . import mesh
        ids = self._device_volume(self.ids_est[scene_id].volume, torch.uint8) if semantics else None
        m = mesh.extract_mesh(self._device_volume(self.scenes_est[scene_id].volume, torch.float16), ids=ids,
                              resolution=float(self.resolution[scene_id]), palette=palette, simplify=simplify)
        if color:
            return m['vertices'], m['faces'], m['normals'], self._vertex_colors(scene_id, m['vertices'], 'get_mesh')[:, :3] / 255.0
        return m['vertices'], m['faces'], m['normals'], m['rgb']

    def render(self, scene_id, intrinsics, extrinsics, shape, semantics=False, normals=True, color=False):
        """Ray-cast the estimated volume of a scene at one or more camera poses (render.py): {'depth', 'normals',
        'labels'} device tensors of [n,h,w](,3), 0 where a ray hits nothing.  Unobserved voxels (fusion weight 0) are
        transparent; semantics=True labels every hit with ids_est; color=True adds 'color', u8 [n,h,w,4]: the scene's
        colour volume at the hit points (color.render_color; alpha 255 where coloured).  Works on resident and on host
        (to_numpy) state."""
        from . import render
        tsdf = self._device_volume(self.scenes_est[scene_id].volume, torch.float16)
        w = self._device_volume(self.fusion_weights[scene_id], torch.float16)
        ids = self._device_volume(self.ids_est[scene_id].volume, torch.uint8) if semantics else None
        cvol = self._color_volume(scene_id, 'render') if color else None
        out = render.render_views(tsdf, w, ids, origin=self.origin[scene_id], resolution=float(self.resolution[scene_id]),
                                  intrinsics=intrinsics, extrinsics=extrinsics, shape=shape, normals=normals)
        if color:
            from . import color as color_
            out['color'] = color_.render_color(cvol, origin=self.origin[scene_id], resolution=float(self.resolution[scene_id]),
                                               intrinsics=intrinsics, extrinsics=extrinsics, depth=out['depth'])
        return out

    def track(self, scene_id, depth, intrinsics, extrinsics, reference_extrinsics=None, filter=None, image=None, **kw):
        """Camera pose of a depth frame against the estimated volume of a scene (tracking.py, frame-to-model ICP):
        tracking starts at ``extrinsics`` and the model is ray-cast at ``reference_extrinsics`` (default: the same pose);
        ``kw`` goes to ``tracking.track_frame`` (mask, levels, iterations, thresholds).  Unobserved voxels are transparent.
        ``filter``: a dict of ``frames.prepare_depth`` options - the frame and its mask go through it first (None: as they are).
        ``image``: the frame's colour image (u8 [h,w,3|4] or float [3,h,w] on the 0..255 scale) - tracking then also compares
        it with the scene's colour volume (``tracking.track_frame_rgbd``, which ``kw`` goes to: photo_weight, photo_thresh,
        grad_depth_limit); a scene without a colour volume (``integrate_color``) is a ValueError.
        Returns {'extrinsics' f64 [4,4], 'ok', 'status', 'stats'}.  Works on resident and on host (to_numpy) state."""
        from . import tracking
        tsdf = self._device_volume(self.scenes_est[scene_id].volume, torch.float16)
        w = self._device_volume(self.fusion_weights[scene_id], torch.float16)
        cvol = self._color_volume(scene_id, 'track') if image is not None else None
        if filter is not None:
            depth, kw['mask'] = _filtered(_to_dev(depth, tsdf.device), _to_dev(kw.get('mask'), tsdf.device), intrinsics, filter)
        if image is not None:
            return tracking.track_frame_rgbd(tsdf, w, cvol, origin=self.origin[scene_id], resolution=float(self.resolution[scene_id]),
                                             image=image, depth=depth, intrinsics=intrinsics, extrinsics=extrinsics,
                                             reference_extrinsics=reference_extrinsics, **kw)
        return tracking.track_frame(tsdf, w, origin=self.origin[scene_id], resolution=float(self.resolution[scene_id]),
                                    depth=depth, intrinsics=intrinsics, extrinsics=extrinsics,
                                    reference_extrinsics=reference_extrinsics, **kw)

    def _relocalizer(self, scene_id, depth):
        """The scene's ``relocalize.Relocalizer``, made on first use for the size of ``depth`` [..,h,w] from
        ``relocalizer_options``."""
        from . import relocalize
        r = self.relocalizers.get(scene_id)
        if r is None:
            h, w = (int(x) for x in depth.shape[-2:])
            r = relocalize.Relocalizer(h, w, device=self.device, **self.relocalizer_options)
            self.relocalizers[scene_id] = r
        return r

    def add_keyframe(self, scene_id, depth, extrinsics, mask=None, image=None, filter=None, force=False):
        """Offer one or more frames with their camera-to-world poses to the scene's keyframe store (relocalize.py): a
        frame is kept when it differs enough from every keyframe (``relocalizer_options['min_dissimilarity']``), or when
        ``force``.  depth [h,w] / [n,h,w], mask and image (read only by a colour table) of the same frames; ``filter`` as
        for ``track`` (a filter with max_angle needs intrinsics and is refused here).  Returns device tensors {'added',
        'best'} without synchronising; the volumes are not touched."""
        dev = lambda x: _to_dev(x, self.device)  # noqa: E731
        depth, mask = dev(depth), dev(mask)
        if filter is not None:
            depth, mask = _filtered(depth, mask, None, filter)
        return self._relocalizer(scene_id, depth).add(depth, extrinsics, mask=mask, image=dev(image), force=force)

    def relocalize(self, scene_id, depth, intrinsics, mask=None, image=None, filter=None, k=4, **kw):
        """The pose of a frame without one, against the estimated volume of a scene: the ``k`` nearest keyframes of the
        scene's store are the starts of ``track`` (relocalize.relocalize_frame, which ``kw`` goes to: max_dissimilarity and
        the tracker's keywords).  ``image`` joins the tracking when the scene has a colour volume, and the code when the
        store's table is a colour table.  Returns ``track``'s dict plus 'candidate' and 'candidates'; {'ok': False, 'status':
        4} when no keyframe gave a pose - a scene without keyframes included.  Works on resident and on host state."""
        from . import relocalize
        tsdf = self._device_volume(self.scenes_est[scene_id].volume, torch.float16)
        w = self._device_volume(self.fusion_weights[scene_id], torch.float16)
        depth, mask = _to_dev(depth, tsdf.device), _to_dev(mask, tsdf.device)
        if filter is not None:
            depth, mask = _filtered(depth, mask, intrinsics, filter)
        cvol = self._color_volume(scene_id, 'relocalize') if image is not None and self.colors.get(scene_id) is not None else None
        return relocalize.relocalize_frame(tsdf, w, self._relocalizer(scene_id, depth), origin=self.origin[scene_id],
                                           resolution=float(self.resolution[scene_id]), depth=depth, intrinsics=intrinsics, mask=mask,
                                           image=image, colors=cvol, k=k, **kw)

    def integrate_depth(self, scene_id, depth, intrinsics, extrinsics, mask=None, labels=None, label_scores=None, filter=None, **kw):
        """Fuse one or more depth maps into the resident volumes of a scene by classical projective TSDF averaging
        (projective.py, no network): depth [h,w] / [n,h,w], poses as for ``render``; ``labels`` (u8, with optional
        ``label_scores``) also update ids_est / scores when the database has semantics; ``kw`` goes to
        ``projective.integrate_depth`` (truncation - default: the initial value -, max_weight, near, carve).  ``filter``: a dict of
        ``frames.prepare_depth`` options (radius, sigma_space, range0, range2, edge_abs, edge_rel, near, far, max_angle) - the
        depth maps and their mask go through it first, with these intrinsics (None: they are fused as they are); the same
        keyword on ``integrate_color``, ``integrate_label_probs``, ``integrate_depth_hist`` and ``track``."""
        from . import projective
        tsdf, w = self.scenes_est[scene_id].volume, self.fusion_weights[scene_id]
        self._resident(scene_id, 'integrate_depth', tsdf, w)
        kw.setdefault('truncation', self.initial_value)
        sem = bool(self.semantics) and labels is not None
        dev = lambda x: _to_dev(x, tsdf.device)  # noqa: E731
        if filter is not None:
            depth, mask = _filtered(dev(depth), dev(mask), intrinsics, filter)
        projective.integrate_depth(tsdf, w, origin=self.origin[scene_id], resolution=float(self.resolution[scene_id]),
                                   depth=dev(depth), intrinsics=intrinsics, extrinsics=extrinsics, mask=dev(mask),
                                   ids=self.ids_est[scene_id].volume if sem else None,
                                   scores=self.scores[scene_id].volume if sem else None,
                                   labels=dev(labels) if sem else None, label_scores=dev(label_scores) if sem else None, **kw)
        self.state[scene_id] = True

    def integrate_color(self, scene_id, image, depth, intrinsics, extrinsics, mask=None, filter=None, **kw):
        """Fuse the colour images of one or more frames into the scene's colour volume (color.py; allocated, zeroed, on first
        use): image u8 [n,]h,w,3|4 or float [n,]3,h,w on the 0..255 scale (the batch dict's), depth / mask / poses of the
        same frames as for ``integrate_depth``; ``kw`` goes to ``color.integrate_color`` (band - default: the initial value -,
        max_weight, near); ``filter`` as for ``integrate_depth``.  Geometry and labels are not touched."""
        from . import color
        tsdf = self.scenes_est[scene_id].volume
        self._resident(scene_id, 'integrate_color', tsdf, optional=(self.colors.get(scene_id),))
        kw.setdefault('band', self.initial_value)
        dev = lambda x: _to_dev(x, tsdf.device)  # noqa: E731
        if filter is not None:
            depth, mask = _filtered(dev(depth), dev(mask), intrinsics, filter)
        with self._side_volume(self.colors, scene_id, lambda: color.new_volume(tsdf.shape, tsdf.device)) as vol:
            color.integrate_color(vol, origin=self.origin[scene_id], resolution=float(self.resolution[scene_id]), image=dev(image),
                                  depth=dev(depth), intrinsics=intrinsics, extrinsics=extrinsics, mask=dev(mask), **kw)

    def integrate_label_probs(self, scene_id, depth, intrinsics, extrinsics, mask=None, probs=None, labels=None, filter=None, **kw):
        """Fuse the label observations of one or more frames into the scene's class-distribution volume (label_probs.py;
        allocated, zeroed, on first use): exactly one of ``probs`` (float [n,]h,w,>=n_classes, a distribution per pixel -
        ``SegEngine.predict_probs``) and ``labels`` (u8 [n,]h,w, a one-hot vote per pixel); depth / mask / poses of the same
        frames as for ``integrate_depth``; ``kw`` goes to ``label_probs.integrate_label_probs`` (band - default: the initial
        value -, max_weight, near); ``filter`` as for ``integrate_depth``.  Geometry, ids_est and scores are not touched:
        ``decide_labels`` writes the labels."""
        from . import label_probs
        if not self.semantics:
            raise ValueError('Database.integrate_label_probs: the database has no semantics (n_classes)')
        tsdf = self.scenes_est[scene_id].volume
        self._resident(scene_id, 'integrate_label_probs', tsdf, optional=(self.label_probs.get(scene_id),))
        kw.setdefault('band', self.initial_value)
        dev = lambda x: _to_dev(x, tsdf.device)  # noqa: E731
        if filter is not None:
            depth, mask = _filtered(dev(depth), dev(mask), intrinsics, filter)
        with self._side_volume(self.label_probs, scene_id, lambda: label_probs.new_volume(tsdf.shape, self.n_classes, tsdf.device)) as vol:
            label_probs.integrate_label_probs(vol, self.n_classes, origin=self.origin[scene_id], resolution=float(self.resolution[scene_id]),
                                              depth=dev(depth), intrinsics=intrinsics, extrinsics=extrinsics, mask=dev(mask),
                                              probs=dev(probs), labels=dev(labels), **kw)

    def integrate_depth_hist(self, scene_id, depth, intrinsics, extrinsics, mask=None, n_bins=9, filter=None, **kw):
        """Fuse one or more depth maps into the scene's depth-histogram volume (tvl1.py; allocated, zeroed, on first use; the bin
        count is fixed then): depth / mask / poses as for ``integrate_depth``; ``kw`` goes to ``tvl1.integrate_depth_hist``
        (truncation - default: the initial value -, max_weight, near, carve); ``filter`` as for ``integrate_depth``.  The estimated
        TSDF and the fusion weights are not touched: ``regularize`` writes them."""
        from . import tvl1
        tsdf = self.scenes_est[scene_id].volume
        have = self.depth_hists.get(scene_id)
        self._resident(scene_id, 'integrate_depth_hist', tsdf, optional=(None if have is None else have[0],))
        if have is not None and have[1] != int(n_bins):
            raise ValueError('Database.integrate_depth_hist: scene {!r} has histograms of {} bins, not {}'.format(scene_id, have[1], n_bins))
        kw.setdefault('truncation', self.initial_value)
        dev = lambda x: _to_dev(x, tsdf.device)  # noqa: E731
        if filter is not None:
            depth, mask = _filtered(dev(depth), dev(mask), intrinsics, filter)
        with self._side_volume(self.depth_hists, scene_id, lambda: (tvl1.new_volume(tsdf.shape, n_bins, tsdf.device), int(n_bins))) as (vol, B):
            tvl1.integrate_depth_hist(vol, B, origin=self.origin[scene_id], resolution=float(self.resolution[scene_id]), depth=dev(depth),
                                      intrinsics=intrinsics, extrinsics=extrinsics, mask=dev(mask), **kw)
        self._tvl1_changed.add(scene_id)

    def regularize(self, scene_id, lam=2.0, iterations=25, restart=True, truncation=None, **kw):
        """Solve the TV-L1 problem of the scene's depth histograms (tvl1.Solver: ``iterations`` Chambolle-Pock iterations with
        data weight ``lam``) and write the result into the estimated TSDF (``truncation`` - default: the initial value - times the
        normalised field) and the fusion weights (the histograms' weights) at the observed voxels.  restart=False continues from
        the previous call's state, taking in the views fused since; ``kw`` goes to ``Solver.solve`` (tau, sigma)."""
        from . import tvl1
        have = self.depth_hists.get(scene_id)
        if have is None:
            raise ValueError('Database.regularize: scene {!r} has no depth histograms (integrate_depth_hist)'.format(scene_id))
        hist, B = have
        tsdf, w = self.scenes_est[scene_id].volume, self.fusion_weights[scene_id]
        self._resident(scene_id, 'regularize', hist, tsdf, w)
        solver = self._tvl1_solvers.get(scene_id)
        if solver is None or solver.shape != tuple(tsdf.shape) or solver.device != tsdf.device:
            solver, restart = tvl1.Solver(tsdf.shape, tsdf.device), True
        solver.solve(hist, B, lam, iterations, restart=restart, changed=scene_id in self._tvl1_changed, **kw)
        solver.write(tsdf, w, self.initial_value if truncation is None else truncation)
        self._tvl1_solvers[scene_id] = solver
        self._tvl1_changed.discard(scene_id)
        self.state[scene_id] = True

    def _refuse_depth_hist(self, scene_id, who):
        if self.depth_hists.get(scene_id) is not None:
            raise ValueError('Database.{}: scene {!r} has depth histograms (integrate_depth_hist), which are not carried through '
                             '{}: remove them first (depth_hists.pop) or fuse into the new box'.format(who, scene_id, who))

    def decide_labels(self, scene_id=None):
        """Write the decision of the class-distribution volumes - of one scene, or of every scene that has one - into ids_est /
        scores (label_probs.decide_labels): a voxel with a vote takes the first class of its largest mean and that mean, the
        others keep what they hold.  Everything that reads ids_est (evaluate_semantics, filter_semantics, render, get_mesh, save)
        sees the decided labels from then on."""
        from . import label_probs
        for s in ([scene_id] if scene_id is not None else list(self.label_probs)):
            vol = self.label_probs.get(s)
            if vol is None:
                raise ValueError('Database.decide_labels: scene {!r} has no class-distribution volume (integrate_label_probs)'.format(s))
            ids, scores = self.ids_est[s].volume, self.scores[s].volume
            self._resident(s, 'decide_labels', vol, ids, scores)
            label_probs.decide_labels(vol, self.n_classes, ids, scores)

    def regularize_labels(self, scene_id=None, lam=4.0, iterations=30, w_sat=4.0, keep_distribution=False):
        """``decide_labels`` with the neighbours having a say (label_tv.py): solve the multi-label TV problem of the
        class-distribution volumes - of one scene, or of every scene that has one - from a restart (``iterations``
        Chambolle-Pock iterations, data weight ``lam``, a voxel's distribution counting in full from the fusion weight
        ``w_sat``) and write the decision into ids_est / scores, the volumes ``decide_labels`` writes; the voxels without a vote
        keep what they hold.  keep_distribution: the scene's class-distribution volume takes the regularised distribution
        (its weights stay)."""
        from . import label_tv
        for s in ([scene_id] if scene_id is not None else list(self.label_probs)):
            vol = self.label_probs.get(s)
            if vol is None:
                raise ValueError('Database.regularize_labels: scene {!r} has no class-distribution volume (integrate_label_probs)'.format(s))
            ids, scores = self.ids_est[s].volume, self.scores[s].volume
            self._resident(s, 'regularize_labels', vol, ids, scores)
            solver = self._label_tv_solvers.get(s)
            if solver is None or solver.shape != tuple(vol.shape[:3]) or solver.device != vol.device or solver.n_classes != self.n_classes:
                solver = label_tv.Solver(vol.shape[:3], self.n_classes, vol.device)
            solver.solve(vol, lam=lam, iterations=iterations, w_sat=w_sat)
            solver.write(ids, scores, vol if keep_distribution else None)
            self._label_tv_solvers[s] = solver

    # ---- the box: re-box, resample, merge (resample.py) ------------------------------------------------------
    def _estimated_volumes(self, scene_id, who):
        """The estimated volumes of a scene as resample.resample_scene takes them; host state is refused."""
        vols = {'tsdf': self.scenes_est[scene_id].volume, 'weights': self.fusion_weights[scene_id]}
        if self.semantics:
            vols.update(ids=self.ids_est[scene_id].volume, scores=self.scores[scene_id].volume)
        if self.colors.get(scene_id) is not None:
            vols['colors'] = self.colors[scene_id]
        if self.label_probs.get(scene_id) is not None:
            vols.update(label_probs=self.label_probs[scene_id], n_classes=self.n_classes)
        self._resident(scene_id, who, *(v for k, v in vols.items() if k != 'n_classes'))
        return vols

    def _origin64(self, scene_id):
        o = self.origin[scene_id]
        return (o.detach().cpu().numpy() if torch.is_tensor(o) else np.asarray(o)).astype(np.float64).reshape(3)

    def resample(self, scene_id, origin=None, shape=None, resolution=None, transform=None):
        """Re-box every volume of a scene (resample.resample_scene, replace mode): the new box has ``origin``, ``shape`` and
        ``resolution`` (each defaults to what the scene has); ``transform`` ([3,4] or [4,4], default identity) maps points of
        the new box's world to the old one's.  The estimated TSDF / weights / ids / scores, the colour and class-distribution
        volumes read the observed voxels of the old box (trilinear, labels from the nearest observed voxel); the ground-truth
        volumes read every voxel of it.  What the old box does not cover holds the initial value / weight 0 / label 0.
        ``origin``, ``resolution`` and the bbox / origin of every Voxelgrid of the scene follow."""
        from . import resample as rs
        self._refuse_depth_hist(scene_id, 'resample')
        est = self._estimated_volumes(scene_id, 'resample')
        gt = self.scenes_gt[scene_id].volume
        ids_gt = self.ids_gt[scene_id].volume if self.semantics and self.semantic_grid else None
        self._resident(scene_id, 'resample', gt, optional=(ids_gt,))
        if gt.dtype != torch.float16:
            raise ValueError('Database.resample: the ground-truth volume of {!r} must be fp16, got {}'.format(scene_id, gt.dtype))
        old_origin, old_res = self._origin64(scene_id), float(self.resolution[scene_id])
        new_origin = old_origin if origin is None else np.asarray(ops._origin_array(origin))
        new_res = old_res if resolution is None else float(resolution)
        new_shape = tuple(gt.shape) if shape is None else tuple(shape)
        kw = dict(src_origin=old_origin, src_resolution=old_res, dst_shape=new_shape, dst_origin=new_origin, dst_resolution=new_res,
                  transform=transform, init_value=self.initial_value)
        new = rs.resample_scene(est, **kw)
        truth = {'tsdf': gt}
        if ids_gt is not None:  # (the nearest rule needs a score volume beside the ids: zeros)
            truth.update(ids=ids_gt, scores=torch.zeros_like(gt))
        new_gt = rs.resample_scene(truth, **kw)
        new_shape = tuple(new['tsdf'].shape)

        bbox = np.stack([new_origin, new_origin + np.array(new_shape, dtype=np.float64) * new_res], axis=1)
        self.origin[scene_id] = torch.from_numpy(new_origin.copy())
        self.resolution[scene_id] = new_res
        grids = [(self.scenes_est[scene_id], new['tsdf']), (self.scenes_gt[scene_id], new_gt['tsdf'])]
        self.fusion_weights[scene_id] = new['weights']
        if self.semantics:
            grids += [(self.ids_est[scene_id], new['ids']), (self.scores[scene_id], new['scores'])]
            if ids_gt is not None:
                grids.append((self.ids_gt[scene_id], new_gt['ids']))
        for grid, volume in grids:
            grid.resolution = new_res
            grid.from_array(volume, bbox)
        if 'colors' in new:
            self.colors[scene_id] = new['colors']
        if 'label_probs' in new:
            self.label_probs[scene_id] = new['label_probs']

    def recentre(self, scene_id, point):
        """Shift the box of a scene by whole voxels so that the voxel holding the world point ``point`` becomes the centre voxel
        (index N // 2 on every axis); returns the integer shift (i, j, k) in voxels.  A whole-voxel shift is exact: every voxel
        that stays inside the box keeps its bits, the voxels that come in hold the initial value / weight 0 / label 0.  The call
        a live driver makes when the tracked camera nears a face of the box."""
        self._refuse_depth_hist(scene_id, 'recentre')
        o, res = self._origin64(scene_id), float(self.resolution[scene_id])
        shape = np.array(self.scenes_est[scene_id].volume.shape, dtype=np.int64)
        p = np.asarray(ops._origin_array(point))
        if not np.isfinite(p).all():
            raise ValueError('Database.recentre: non-finite point')
        shift = np.floor((p - o) / res).astype(np.int64) - shape // 2
        if shift.any():
            self.resample(scene_id, origin=o + shift.astype(np.float64) * res)
        else:
            self._estimated_volumes(scene_id, 'recentre')  # (host state is refused all the same)
        return tuple(int(s) for s in shift)

    def merge(self, dst_scene, src_scene, transform=None, max_weight=None):
        """Merge the estimated volumes of ``src_scene`` into those of ``dst_scene`` in place (resample.resample_scene, merge
        mode): where the source is observed the destination takes the running mean of both by their weights, the label of the
        higher score, and the sum of the weights up to ``max_weight`` (default: 65504 for the geometry, 64 for colour and class
        distributions); elsewhere it is left alone.  ``transform`` maps points of the destination's world to the source's (the
        tracked pose between two sessions; default: one world).  A colour or class-distribution volume only the source has is
        created in the destination; ``decide_labels`` is left to the caller."""
        from . import color, label_probs, resample as rs
        if dst_scene == src_scene:
            raise ValueError('Database.merge: a scene cannot be merged into itself')
        self._refuse_depth_hist(dst_scene, 'merge')
        self._refuse_depth_hist(src_scene, 'merge')
        src = self._estimated_volumes(src_scene, 'merge')
        dst = self._estimated_volumes(dst_scene, 'merge')
        shape, dev = tuple(dst['tsdf'].shape), dst['tsdf'].device
        fresh = {}
        if 'colors' in src and 'colors' not in dst:
            fresh['colors'] = dst['colors'] = color.new_volume(shape, dev)
        if 'label_probs' in src and 'label_probs' not in dst:
            fresh['label_probs'] = dst['label_probs'] = label_probs.new_volume(shape, self.n_classes, dev)
            dst['n_classes'] = self.n_classes
        into = {k: v for k, v in dst.items() if k in src}
        rs.resample_scene(src, src_origin=self._origin64(src_scene), src_resolution=float(self.resolution[src_scene]), dst_shape=shape,
                          dst_origin=self._origin64(dst_scene), dst_resolution=float(self.resolution[dst_scene]), transform=transform,
                          into=into, init_value=self.initial_value, max_weight=max_weight)
        if 'colors' in fresh:  # (a refused call leaves a scene without a volume without one)
            self.colors[dst_scene] = fresh['colors']
        if 'label_probs' in fresh:
            self.label_probs[dst_scene] = fresh['label_probs']
        self.state[dst_scene] = self.state[dst_scene] or self.state[src_scene]

    def register(self, dst_scene, src_scene, transform=None, **kw):
        """The rigid transform between the estimated volumes of two scenes (registration.register_volumes, Gauss-Newton on
        signed distance fields): it maps points of ``dst_scene``'s world to ``src_scene``'s - what ``merge(dst_scene, src_scene,
        transform=...)`` takes.  ``transform`` is the initial guess (default: one world); ``kw`` goes to ``register_volumes``
        (band, stages, min_inlier_fraction).  Returns its dict {'transform' f64 [3,4], 'ok', 'status', 'failed_iteration',
        'stats', 'n_points'}.  Reads the TSDF and the weights of both scenes and writes no volume; host state is refused."""
        from . import registration
        if dst_scene == src_scene:
            raise ValueError('Database.register: a scene cannot be registered to itself')
        scenes = []
        for s in (dst_scene, src_scene):
            tsdf, w = self.scenes_est[s].volume, self.fusion_weights[s]
            self._resident(s, 'register', tsdf, w)
            scenes.append({'tsdf': tsdf, 'weights': w, 'origin': self._origin64(s), 'resolution': float(self.resolution[s])})
        return registration.register_volumes(scenes[0], scenes[1], transform=transform, **kw)

    def save_to_workspace(self, workspace, mode, save_mode='ply', simplify=None):
        """database.py:141-177: every scene that holds integrated frames goes to the workspace's output directory as
        ``<scene>.tsdf_<mode>.hf5`` / ``.weights_<mode>.hf5`` / ``.semantic_<mode>.hf5`` ('tsdf'), ``<scene>_<mode>.ply``
        ('ply'), or all of them ('test').  ``workspace`` offers save_tsdf_data / save_weights_data /
        save_semantic_data / save_ply_data(file, volume) (utils/setup.py:253-267; drivers.Workspace).  simplify (cell size in
        voxels, SETTINGS.simplify; default off) goes to save_ply_data as a keyword when it is set."""
        if save_mode not in ('tsdf', 'ply', 'test'):
            return  # the reference's if / elif chain falls through silently
        for s in self.scenes:
            if not self.state[s]:
                continue
            base = s.replace('/', '.')
            if save_mode in ('tsdf', 'test'):
                workspace.save_tsdf_data('{}.tsdf_{}.hf5'.format(base, mode), self.scenes_est[s].volume)
                workspace.save_weights_data('{}.weights_{}.hf5'.format(base, mode), self.fusion_weights[s])
                if self.semantics:
                    workspace.save_semantic_data('{}.semantic_{}.hf5'.format(base, mode), self.ids_est[s].volume)
            if save_mode in ('ply', 'test'):
                workspace.save_ply_data('{}_{}.ply'.format(base, mode), self.scenes_est[s].volume,
                                        **({} if simplify is None else {'simplify': simplify}))

    def save(self, path, save_mode='ply', scene_id=None, palette=None, simplify=None):
        """database.py:172-261: 'tsdf' (volumes), 'ply' (mesh), 'test' (volumes + mesh + label-coloured mesh whose
        alpha channel carries the label id).  A scene with a colour volume also gets ``<scene>_color.ply`` (the mesh with
        its sampled vertex colours, alpha 255 where coloured) beside every mesh and ``<scene>.color.hf5`` beside the volumes; a scene
        with a class-distribution volume gets ``<scene>.label_probs.hf5`` there, one with depth histograms ``<scene>.depth_hist.hf5``.  simplify (cell size in voxels; default off):
        the meshes go through the quadric vertex clustering of mesh_simplify.py first."""
        if scene_id is None:
            raise NotImplementedError
        if save_mode not in ('tsdf', 'ply', 'test'):
            raise ValueError('unknown save_mode {!r}'.format(save_mode))
        base = scene_id.replace('/', '.')
        if save_mode in ('ply', 'test'):
            from . import mesh
            sem = self.semantics and save_mode == 'test'
            ids = self._device_volume(self.ids_est[scene_id].volume, torch.uint8) if sem else None
            m = mesh.extract_mesh(self._device_volume(self.scenes_est[scene_id].volume, torch.float16), ids=ids,
                                  resolution=float(self.resolution[scene_id]), palette=palette, simplify=simplify)
            mesh.save_ply(os.path.join(path, base + '.ply'), m['vertices'], m['faces'], m['normals'])
            if sem:
                table = np.array(mesh.default_palette() if palette is None else palette, dtype=np.uint8)
                rgba = np.concatenate([table[m['labels']], m['labels'][:, None]], axis=1)
                mesh.save_ply(os.path.join(path, base + '_semantic.ply'), m['vertices'], m['faces'], m['normals'], rgba)
            if self.colors.get(scene_id) is not None:
                mesh.save_ply(os.path.join(path, base + '_color.ply'), m['vertices'], m['faces'], m['normals'],
                              self._vertex_colors(scene_id, m['vertices'], 'save'))
            if save_mode == 'ply':
                return

        def host(a):
            return a.detach().cpu().numpy() if torch.is_tensor(a) else a
        arrays = {'tsdf': ('TSDF', host(self.scenes_est[scene_id].volume)),
                  'weights': ('weights', host(self.fusion_weights[scene_id]))}
        if self.semantics:
            arrays['semantics'] = ('semantics', host(self.ids_est[scene_id].volume))
        if self.colors.get(scene_id) is not None:
            arrays['color'] = ('color', host(self.colors[scene_id]))
        if self.label_probs.get(scene_id) is not None:
            arrays['label_probs'] = ('label_probs', host(self.label_probs[scene_id]))
        if self.depth_hists.get(scene_id) is not None:
            arrays['depth_hist'] = ('depth_hist', host(self.depth_hists[scene_id][0]))
        from .datasets import save_volume_hdf
        for name, (key, arr) in arrays.items():  # same file / dataset names as database.py:184-201 (npz without h5py)
            save_volume_hdf(os.path.join(path, '{}.{}.hf5'.format(base, name)), key, arr)
