"""Pipeline: per-frame orchestration with the reference's API (modules/pipeline.py:12-363).

``fuse`` / ``fuse_training`` keep the reference's signatures, batch-dict keys and side effects on
``Database``; the work is done by three HIP stages on the current stream with no host round trip
in between:

    ojf_extract  -> fusion_values / fusion_weights rows [N,9] (kept: they are part of the API)
    ojf_net_*    -> fp32-MFMA FusionNet (eval mode, BN folded)            [inference]
                    torch autograd on the same device                     [training, needs grads]
    ojf_integrate-> recomputes indices/weights, resolves colliding voxel writes, updates the
                    fp16 volumes in place (and the semantic ids/scores in test mode)

The reference's intermediate tensors (int64 indices [N,9,8,3], fp64 weights, NCHW permutes,
fancy-index slices of valid pixels: pipeline.py:74-171) never exist here.

The class keeps the frame steps.  Three plain objects, created with it, own the state around them: labels2d.LabelFrontEnd (a
frame's 2-D labels: engine cache, graph captures, look-ahead prefetch), guard_records.GuardRecords (the frames a range-guard
recovery may have to fuse again) and announce.TrainingAnnouncements (training frames announced ahead, their valid-ray counts).
"""
import torch

from . import ops
from . import _lib
from ._lib import MODE_FAST, MODE_PARITY
from .announce import TrainingAnnouncements
from .engine import FusionNetEngine
from .extractor import Extractor
from .guard_records import GuardRecords, guard_frames_to_fuse_again, guard_policy  # noqa: F401 (the rule stays importable from here)
from .integrator import Integrator
from .labels2d import LabelFrontEnd, side_stream
from .model import FusionNet_v2, FusionNet_v3


class Pipeline(torch.nn.Module):

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.n_points = config.FUSION_MODEL.n_points
        if config.DATA.semantics:
            self.n_classes = config.SEMANTIC_2D_MODEL.n_classes
        config.FUSION_MODEL.resx = config.DATA.resx  # pipeline.py:24-25
        config.FUSION_MODEL.resy = config.DATA.resy

        name = config.FUSION_MODEL.name
        # FUSION_MODEL.depth_filter: None, or the frames.prepare_depth options every frame and its mask go through in front of the
        # classical modes' fusion calls
        self._depth_filter = config.FUSION_MODEL.get('depth_filter', None)
        if self._depth_filter is not None:
            if name not in ('tsdf', 'tvl1'):
                raise ValueError('Pipeline: FUSION_MODEL.depth_filter is supported by FUSION_MODEL.name "tsdf" and "tvl1" only (the '
                                 'fusion net\'s parity with the reference depends on the raw frame)')
            from . import frames
            frames.check_filter(dict(self._depth_filter))
        if name == 'v2':
            self._fusion_network = FusionNet_v2(config.FUSION_MODEL)
        elif name == 'v3':
            self._fusion_network = FusionNet_v3(config.FUSION_MODEL)
        elif name in ('tsdf', 'tvl1'):
            # classical projective TSDF averaging (projective.py) or robust TV-L1 fusion of depth histograms (tvl1.py): no network -
            # an empty module with an empty state_dict, so that .to() / .eval() / checkpoint code written for the learned modes
            # keeps working
            self._fusion_network = torch.nn.Module()
        else:  # the reference's v1 cannot even be constructed (model.py:58)
            raise ValueError('FUSION_MODEL.name must be "v2", "v3", "tsdf" or "tvl1"')
        self._classical = name in ('tsdf', 'tvl1')
        self._tvl1 = name == 'tvl1'
        self._tvl1_frames = {}  # scene -> frames fused into its histograms (the solver runs after every tvl1_every of them)

        if config.DATA.semantics and config.DATA.semantic_strategy == 'predict':
            from .adapnet import AdapNet
            self._semantic_2d_network = AdapNet(config.SEMANTIC_2D_MODEL)
        else:
            self._semantic_2d_network = None

        self._extractor = Extractor(config)
        self._integrator = Integrator(config)
        # a load_state_dict into the fusion net (any flavour, assign=True included) drops the cached tensor list of the
        # engine-staleness check at once
        def _drop_fingerprint(module, incompatible):
            self._fp_cache = None  # (a post hook must return None)
        self._fusion_network.register_load_state_dict_post_hook(_drop_fingerprint)
        mode = getattr(config.SETTINGS, 'integrate_mode', 'fast')
        self._integrate_mode = MODE_PARITY if mode == 'parity' else MODE_FAST
        # per-slot device state (engine with its activation buffers, est rows, sample planes, integrate workspaces): slot 0
        # is the frame step of fuse() / fuse_training(); fuse_many() runs scene i of a call on slot i and its own stream
        self._slots = {}
        self._workspaces = {}
        self.profile = False  # True / N: fuse() brackets its three stages with HIP events on every (N-th) frame
        self._frames_fused = 0
        self._marks = []
        self.device = torch.device('cpu')  # the device of the last frame step (every one sets it)
        self._fp_cache = None  # [id(net), its parameters and buffers, age in frames] of _weights_fingerprint
        self._zero = None  # a device scalar 0.0 for the filtered frame of _frames
        self._seg_marks = []  # (event in front of the 2-D pass, the frame's first stage event) per profiled frame
        self._slot_streams = []  # fuse_many: the stream of slot i + 1
        self._shape = None  # image shape of the last prepared frame (_prepare_frame)
        self._hip_train = None  # train.HipTrainNet of the fusion net, made by the first fuse_training on a GPU
        self.guard_events = 0  # range-guard recoveries so far (_guard_recover)
        self.last_guard_skips = []  # per frame remembered at the last recovery: (frame_id, did its integrate call skip)
        # plain objects, not sub-modules: the state_dict and children() are the two networks'
        # (no closure over self: a deep copy of the pipeline gets owners that read the copy's networks and config)
        self._labels2d = LabelFrontEnd(config, self._modules)
        self._guard = GuardRecords(config)
        self._announcements = TrainingAnnouncements()

    # fuse_training calls that found / did not find their batch announced (announce_training_frame)
    announce_hits = property(lambda self: self._announcements.hits)
    announce_misses = property(lambda self: self._announcements.misses)

    # ---- live stage timing (HIP events on the launch stream; bench.py) ---------------------------
    def _mark(self, first=False):
        """Even a fence-free event record is a marker packet in the queue (~4.5 us of idle queue each, four per frame):
        ``profile = N`` samples every N-th frame so that the timing does not change what it times."""
        if first:
            self._frames_fused += 1
        if self.profile and (self.profile is True or self._frames_fused % int(self.profile) == 0):
            e = _lib.TimingEvent()  # no system-scope fence: a default event costs ~5 us of idle queue per record
            e.record(torch.cuda.current_stream(self.device).cuda_stream)
            self._marks.append(e)

    def _mark_segmentation(self):
        """Event in front of the 2-D segmentation of a frame the stage sampling will pick (predict strategy only)."""
        if not self.profile or not self.config.DATA.semantics or self.config.DATA.semantic_strategy != 'predict':
            return None
        if self.profile is not True and (self._frames_fused + 1) % int(self.profile) != 0:
            return None
        e = _lib.TimingEvent()
        e.record(torch.cuda.current_stream(self.device).cuda_stream)
        return e

    def reset_profile(self):
        self._marks = []
        self._seg_marks = []

    def stage_times_ms(self):
        """Mean milliseconds per frame of extract / net / integrate over the frames fused since
        reset_profile() (4 events per frame)."""
        torch.cuda.synchronize(self.device)
        ev = self._marks
        n = len(ev) // 4
        if n == 0:
            return {}
        acc = [0.0, 0.0, 0.0]
        for f in range(n):
            for j in range(3):
                acc[j] += ev[4 * f + j].elapsed_time(ev[4 * f + j + 1])
        out = {'extract': acc[0] / n, 'net': acc[1] / n, 'integrate': acc[2] / n}
        seg = self._seg_marks
        if seg:  # AdapNet++ prediction of the frame's labels (+ the host work between it and the extract launch)
            out['segmentation'] = sum(a.elapsed_time(b) for a, b in seg) / len(seg)
        return out

    def check(self):
        """Synchronise and raise OjfError if the split-fp16 range guard fired since the last check (the frames
        fused in between are invalid then; set FUSION_MODEL.arithmetic = 'f32').  Cheap: call per scene / epoch."""
        if self._engine is not None:
            if self._guard_policy() == 'f32':
                self._guard_recover()  # (a tripped frame at the end of a scene: nothing after it polled the flag)
            torch.cuda.synchronize(self.device)  # (every slot's stream)
            self._engine.check()
        elif self.device.type == 'cuda':
            # no inference engine yet (training only, or only the 2-D engine ran): the executors share the one flag
            torch.cuda.synchronize(self.device)
            _lib.check(_lib.load().ojf_net_check(_lib.stream_ptr(self.device)), 'ojf_net_check')

    # ---- cached device objects ----------------------------------------------------------------
    def _weights_fingerprint(self):
        """In-place weight updates (optimizer steps, load_state_dict) bump the tensors' version counters.  Walking
        the module tree costs ~0.3 ms, so the tensor list is cached and re-collected every 64 frames."""
        net = self._fusion_network
        cache = self._fp_cache
        if cache is None or cache[0] != id(net) or cache[2] >= 64:
            cache = self._fp_cache = [id(net), list(net.parameters()) + list(net.buffers()), 0]
        cache[2] += 1
        # version counters see in-place updates (optimizer steps, load_state_dict); storage addresses see
        # ``p.data = ...``; replaced Parameter objects (load_state_dict(assign=True), swapped sub-modules) are seen by
        # the load_state_dict hook below at once and by the re-collection within 64 frames otherwise
        return (len(cache[1]), sum(t._version for t in cache[1]), sum(t.data_ptr() for t in cache[1]) & 0xffffffffffff)

    class _Slot:
        engine = key = est = fv = fw = None

    # slot 0 under the names the rest of the package (and bench.py) knows
    _engine = property(lambda self: self._slots[0].engine if 0 in self._slots else None)
    _est = property(lambda self: self._slots[0].est if 0 in self._slots else None)
    _fv = property(lambda self: self._slots[0].fv if 0 in self._slots else None)
    _fw = property(lambda self: self._slots[0].fw if 0 in self._slots else None)

    def _get_slot(self, h, w, device, slot=0, fingerprint=None):
        arith = self.config.FUSION_MODEL.get('arithmetic', 'f16x3')
        key = (h, w, str(device), arith, fingerprint if fingerprint is not None else self._weights_fingerprint())
        sl = self._slots.get(slot)
        if sl is None:
            sl = self._slots[slot] = Pipeline._Slot()
        if sl.engine is None or sl.key != key:
            if sl.engine is not None:
                sl.engine.close()
            sl.engine = FusionNetEngine(self._fusion_network, h, w, device, arithmetic=arith)
            sl.key = key
            sl.est = torch.empty((h * w, self.n_points), dtype=torch.float32, device=device)
            sl.fv = torch.empty((self.n_points, h * w), dtype=torch.float32, device=device)  # sample planes
            sl.fw = torch.empty((self.n_points, h * w), dtype=torch.float32, device=device)
        return sl

    def _get_engine(self, h, w, device):
        return self._get_slot(h, w, device).engine

    def _get_workspace(self, shape, h, w, device, slot=0):
        key = (tuple(shape), h, w, self._integrate_mode, slot)
        if key not in self._workspaces:
            self._workspaces[key] = ops.IntegrateWorkspace(shape, h, w, self.config.FUSION_MODEL.n_tail_points,
                                                           self._integrate_mode, device)
        return self._workspaces[key]

    def fuse_sequence(self, batches, database, device, prefetch=None):
        """``for b in batches: fuse(b, database, device)`` for CONSECUTIVE frames (of one scene, or any mix of scenes in stream
        order).  The frame steps stay strictly in order - frame t+1 is extracted from the volume frame t was integrated into -
        but the 2-D network does not depend on the volumes: with ``semantic_strategy: predict`` the labels of all the frames
        are predicted first, as ONE batched AdapNet++ pass (SegEngine.predict_many: 0.62 / 0.48 ms per frame at four / eight
        frames per pass against 1.20 ms one at a time).  Same volumes as the separate calls, with the batched
        pass's rounding of the scores (include/ojf.h, ojf_segconv_forward_batch).  With FUSION_MODEL.fuse_label_probs every frame's
        label image - the ids of that pass, or semantic_gt - also votes in its scene's class-distribution volume, right after its
        frame step.  The reference predicts and fuses one frame
        at a time (test_fusion.py:68-80); a driver that reads a recorded stream can hand over chunks (drivers.test_fusion does).

        ``prefetch``: the chunk the NEXT call will bring (the same batch objects).  Its batched 2-D pass is enqueued on a
        side stream before this chunk's frame steps and runs beside them; the next call finds the labels ready.  Bits do not
        depend on it (the same graph replay, another stream)."""
        if self._tvl1 and prefetch:
            raise ValueError('Pipeline.fuse_sequence: FUSION_MODEL.name "tvl1" does not support the look-ahead (prefetch)')
        self.device = torch.device(device)
        labels = self._labels2d
        sems = labels.take_prefetched(batches, self.device)
        if sems is None:
            sems = labels.frame_semantics_many(batches, self.device)
        if prefetch and labels.batched_pass_applies(prefetch):
            if sems and sems[0][0] is not None and not (labels.prefetch or {}).get('taken'):
                sems = [(i.clone(), sc.clone()) for i, sc in sems]  # (this chunk's labels sit in the graph's output buffers, which the prefetched pass overwrites)
            eng, est = self._engine, self._est
            labels.prefetch_semantics(prefetch, self.device, eng, (lambda: eng.forward(est)) if eng is not None else None)
        if self._classical:
            return self._fuse_classical(batches, sems, database)
        fp = self._weights_fingerprint()
        recover = self._guard_policy() == 'f32'
        for b, sem in zip(batches, sems):
            self._fuse_guarded(b, database, sem, fp, recover)
            self._fuse_colors([b], database)
            self._fuse_labels([b], [sem[0]], database)

    def _fuse_guarded(self, batch, database, sem=None, fingerprint=None, recover=False):
        """One frame step of fuse_sequence / fuse_many's sequential paths under FUSION_MODEL.guard_policy (what ``fuse`` does
        for its one frame): with 'f32' a fired range guard switches the arithmetic, fuses the skipped frames again and goes
        on with this one; the frame joins the ring of remembered batches.  ``sem`` (the frame's labels from a batched 2-D
        pass) does not depend on the fusion net's arithmetic and is used either way; the re-fused frames predict theirs
        again, one frame at a time.  Returns the frame's label image (``_fuse_frame``)."""
        if not recover:
            return self._fuse_frame(batch, database, 0, sem, fingerprint)
        try:
            sem_ids = self._fuse_frame(batch, database, 0, sem, fingerprint)
        except _lib.OjfError as err:
            if 'fp16 range' not in str(err):
                raise
            self._guard_recover(err)
            return self._fuse_frame(batch, database, 0, sem)  # (fp32 engine: a new fingerprint)
        self._guard.remember(batch, database)
        return sem_ids

    def _frames(self, batch, filtered=True):
        """(frame, filtered frame) of pipeline.py:194-199; with ``filtered=False`` the second item is the bool mask
        instead and the integrate kernels apply it themselves (ojf_integrate_masked)."""
        frame = batch[self.config.DATA.input]
        frame = frame.reshape(frame.shape[0], frame.shape[-2], frame.shape[-1])  # squeeze_(1) of [b,1,h,w]
        if frame.shape[0] != 1:
            raise ValueError('Pipeline: batch size 1 only (one scene per frame, pipeline.py:199)')
        frame = frame.to(self.device).float().contiguous()
        mask = batch['mask'].to(self.device).reshape(frame.shape)
        if not filtered:
            if mask.dtype != torch.bool:
                mask = mask != 0
            return frame[0], mask[0].contiguous()
        zero = self._zero
        if zero is None or zero.device != frame.device:
            zero = self._zero = torch.zeros((), dtype=torch.float32, device=frame.device)
        filtered = torch.where(mask, frame, zero)  # pipeline.py:196; one launch (a python scalar costs a fill kernel)
        return frame[0], filtered[0]

    def _prepare_frame(self, batch, database, filtered=False, frames=None):
        """What every frame step needs of its batch: (scene id, the scene's volume dict, frame, mask, Ki, E, h, w).  ``filtered``: the
        filtered frame instead of the mask (``_frames``; fuse_training); ``frames``: that pair where the caller holds it already (an
        announced frame).  ``database=None`` (classical mode: one volume look-up per run, fp64 poses of its own): no volume, Ki, E."""
        self._shape = batch['image'].shape
        frame, mask = frames or self._frames(batch, filtered)
        scene_id = batch['frame_id'][0].split('/')[0]
        if database is None:
            return (scene_id, None, frame, mask, None, None) + tuple(frame.shape)
        Ki, E = ops.camera_arrays(batch['intrinsics'][0], batch['extrinsics'][0])
        return (scene_id, database[scene_id], frame, mask, Ki, E) + tuple(frame.shape)

    @staticmethod
    def _commit_frame(database, scene_id, volume):
        database.state[scene_id] = True  # volumes were updated in place (pipeline.py:239-244)
        database.scenes_est[scene_id].volume = volume['current']
        database.fusion_weights[scene_id] = volume['weights']

    def _refuse_tripped_guard(self, who):
        """The range-guard flag is process-wide and raised by EVERY split-fp16 executor (the 2-D engine's kernels always are, whatever
        FUSION_MODEL.arithmetic says), while the integrate calls skip as long as it is set: a host read of the mapped word in front of
        anything a frame enqueues keeps a tripped 2-D pass from dropping frames (or handing its labels to a volume) silently when the
        fusion net itself runs fp32, whose forward call does not poll - or when there is no net."""
        if self.device.type == 'cuda' and _lib.load().ojf_guard_poll():
            raise _lib.OjfError(who + ': the split-fp16 range guard is set (fp16 range exceeded in a network pass since the last '
                                'check()): the integrate calls skip until check() has reported it')

    # ---- range guard of the split-fp16 net: no frame of a tripped net reaches a volume --------------
    # (include/ojf.h ojf_net_check: while the flag is set the integrate calls skip, so nothing is corrupted; what is left
    # to decide is what happens to the skipped frames.)  FUSION_MODEL.guard_policy:
    #   'raise' (default)  the next fuse() / check() raises OjfError; the volumes hold every frame in front of the event
    #                      and nothing after it;
    #   'f32'              the pipeline switches this network to the fp32-input MFMA arithmetic for good (a warning says
    #                      so) and fuses the skipped frames again, in order: the stream comes out as if the net had run in
    #                      fp32 from the event on.  The batches of the last <= 48 frames stay alive for that (an event
    #                      every 16 frames bounds how far the host may run ahead of the device).
    def _guard_policy(self):
        return guard_policy(self.config)

    def _guard_recover(self, err=None):
        """guard_policy 'f32': if the guard fired - report + clear the event, switch the arithmetic, fuse the skipped frames
        again.  Synchronises.  Returns True when it did."""
        import ctypes
        import warnings
        lib = _lib.load()
        flag, skipped = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(lib.ojf_guard_status(_lib.stream_ptr(self.device), ctypes.byref(flag), ctypes.byref(skipped)), 'ojf_guard_status')
        if flag.value != 1:  # nothing pending, or an internal error: not this policy's to absorb
            if err is not None:
                raise err
            return False
        lib.ojf_net_check(_lib.stream_ptr(self.device))  # (reports what `flag` said and clears it)
        n = skipped.value
        # per remembered frame, in order: (frame_id, did its integrate call skip) - which frames the recovery below fuses again
        redo, self.last_guard_skips = self._guard.take(n)
        self.config.FUSION_MODEL.arithmetic = 'f32'
        self.guard_events += 1
        warnings.warn('split-fp16 range guard fired: FUSION_MODEL.arithmetic switched to f32 for this network, '
                      '%d skipped frame(s) fused again' % n, RuntimeWarning)
        for b, db in redo:
            self._fuse_frame(b, db)
        return True

    def fuse(self, batch, database, device):
        self.device = torch.device(device)
        if self._classical:
            return self._fuse_classical([batch], [None], database)
        # (a frame the forward call's poll refuses was raised BEFORE its net / integrate were enqueued: it is not among the
        # skipped ones, it follows them - _fuse_guarded)
        sem_ids = self._fuse_guarded(batch, database, recover=self._guard_policy() == 'f32')
        self._fuse_colors([batch], database)
        self._fuse_labels([batch], [sem_ids], database)

    # ---- FUSION_MODEL.fuse_color: the frames' colour images into the scenes' colour volumes (color.py) -----------------------
    def _color_options(self):
        """None (FUSION_MODEL.fuse_color off, the default) or the keywords of Database.integrate_color: color_band (default
        DATA.init_value)."""
        fm = self.config.FUSION_MODEL
        if not fm.get('fuse_color', False):
            return None
        return dict(band=fm.get('color_band', None) or self.config.DATA.init_value)

    def _fuse_colors(self, batches, database):
        """The learned modes' colour step: ``batch['image']`` of every frame, in order, into its scene's colour volume with the
        depth frame, mask and pose its frame step used, on the current stream.  Called once per frame the caller has fused
        (a frame the range guard made the pipeline fuse again is not coloured again).  Geometry and labels are not touched."""
        kw = self._color_options()
        if kw is None:
            return
        for b in batches:
            frame, mask = self._frames(b, filtered=False)
            database.integrate_color(b['frame_id'][0].split('/')[0], b['image'].to(self.device), frame.unsqueeze(0),
                                     b['intrinsics'][0], b['extrinsics'][0], mask=mask.unsqueeze(0), **kw)

    # ---- FUSION_MODEL.fuse_label_probs: the frames' label images as one-hot votes into the scenes' class distributions ---------
    def _label_options(self):
        """None (FUSION_MODEL.fuse_label_probs off, the default) or the keywords of Database.integrate_label_probs: label_band
        (default DATA.init_value)."""
        fm = self.config.FUSION_MODEL
        if not fm.get('fuse_label_probs', False):
            return None
        if not self.config.DATA.semantics:
            raise ValueError('Pipeline: FUSION_MODEL.fuse_label_probs needs DATA.semantics (label images and a class count)')
        return dict(band=fm.get('label_band', None) or self.config.DATA.init_value)

    def _fuse_labels(self, batches, label_images, database):
        """The learned modes' label-vote step: the label image of every frame, in order, as a one-hot vote
        (label_probs.integrate_label_probs(labels=...)) into its scene's class-distribution volume with the depth frame, mask
        and pose its frame step used, on the current stream.  ``label_images[i]``: the ids the frame step of batch i fused
        (u8, h*w; ``_fuse_frame`` returns them - with ``semantic_strategy: predict`` the 2-D network is not run a second time),
        or None: ``batch['semantic_gt']``, the label image of strategy 'gt'.  ids_est / scores are not touched here:
        Database.decide_labels() writes them."""
        kw = self._label_options()
        if kw is None:
            return
        for b, ids in zip(batches, label_images):
            frame, mask = self._frames(b, filtered=False)
            if ids is None:
                if self.config.DATA.semantic_strategy != 'gt':
                    raise ValueError('Pipeline: fuse_label_probs has no label image for this frame (semantic_strategy predict)')
                ids = b['semantic_gt']
            labels = ids.to(self.device).to(torch.uint8).reshape((1,) + tuple(frame.shape))
            database.integrate_label_probs(b['frame_id'][0].split('/')[0], frame.unsqueeze(0), b['intrinsics'][0], b['extrinsics'][0],
                                           mask=mask.unsqueeze(0), labels=labels, **kw)

    def _fuse_frame(self, batch, database, slot=0, semantics=None, fingerprint=None):
        """One frame step on the current stream with the device state of ``slot``; ``semantics`` = (sem_ids, scores) computed
        by the caller (fuse_many) instead of here.  Returns the frame's label image sem_ids (u8 [h*w], None without semantics)."""
        self._refuse_tripped_guard('Pipeline.fuse')
        profiled = slot == 0 and semantics is None
        seg0 = self._mark_segmentation() if profiled else None
        sem_ids, scores = self._labels2d.frame_semantics(batch, self.device) if semantics is None else semantics
        scene_id, volume, frame, mask, Ki, E, h, w = self._prepare_frame(batch, database)
        tsdf, weights = volume['current'], volume['weights']

        sl = self._get_slot(h, w, self.device, slot, fingerprint)
        eng = sl.engine
        P = self.n_points
        mark = self._mark if profiled else (lambda first=False: None)
        mark(first=True)
        if seg0 is not None and self._marks:
            self._seg_marks.append((seg0, self._marks[-1]))
        use_sem = self.config.FUSION_MODEL.use_semantics
        if eng.fused_input:
            # geometry-only net: the extractor writes the net's input planes itself (one launch less, no sample planes)
            ops.extract_to_net(frame, Ki, E, volume['origin'], volume['resolution'], tsdf, weights, eng)
            mark()
        else:
            ops.extract(frame, Ki, E, volume['origin'], volume['resolution'], tsdf, weights, n_points=P,
                        out_values=sl.fv, out_weights=sl.fw, out_stride=h * w, planes=True)
            mark()
            eng.prepare_input(sl.fv, sl.fw, frame, sem_ids if use_sem else None, self.n_classes if use_sem else 0,
                              planes=True)
        eng.forward(sl.est)
        mark()

        sem = bool(self.config.DATA.semantics)
        ws = self._get_workspace(tsdf.shape, h, w, self.device, slot)
        ops.integrate(frame, Ki, E, volume['origin'], volume['resolution'], sl.est, tsdf, weights, ws,
                      n_points=P, n_tail=self.config.FUSION_MODEL.n_tail_points,
                      trunc=self.config.DATA.init_value,
                      sem_ids=sem_ids if sem else None, sem_scores=scores if sem else None,
                      id_vol=volume['ids_est'] if sem else None, score_vol=volume['scores'] if sem else None,
                      mode=self._integrate_mode, mask=mask)  # filtered frame of pipeline.py:196 formed in the kernels
        self._guard.note(slot, ws)
        mark()
        self._commit_frame(database, scene_id, volume)
        return sem_ids

    # ---- FUSION_MODEL.name 'tvl1': depth histograms and their TV-L1 minimiser in place of the running mean (tvl1.py) -----------
    def _tvl1_options(self):
        """None (any other mode) or {n_bins, lam, iterations, every}: FUSION_MODEL hist_bins (default 9), tvl1_lambda (2.0),
        tvl1_iterations (25; warm-started, after every tvl1_every (1) frames of a scene)."""
        if not self._tvl1:
            return None
        fm = self.config.FUSION_MODEL
        o = dict(n_bins=int(fm.get('hist_bins', 9)), lam=float(fm.get('tvl1_lambda', 2.0)), iterations=int(fm.get('tvl1_iterations', 25)),
                 every=int(fm.get('tvl1_every', 1)))
        if not 2 <= o['n_bins'] <= _lib.HIST_MAX_BINS or not 0.0 < o['lam'] < float('inf') or o['iterations'] < 0 or o['every'] < 1:
            raise ValueError('Pipeline: FUSION_MODEL hist_bins in 2..{}, tvl1_lambda > 0, tvl1_iterations >= 0 and tvl1_every >= 1 '
                             'expected, got {}'.format(_lib.HIST_MAX_BINS, o))
        return o

    # ---- FUSION_MODEL.name 'tsdf': classical projective TSDF averaging, no network (projective.py) -------------------------
    def _fuse_classical(self, batches, sems, database):
        """The frame steps of ``batches`` (in order) as projective.integrate_depth calls: the frame, mask, pose and labels that
        ``_fuse_frame`` takes, runs of consecutive frames of one scene and one image shape as ONE kernel call of up to
        ``_lib.PROJECTIVE_MAX_VIEWS`` views (the same bits as a call per frame), and the same side effects on ``database``.
        ``sems[i]``: the frame's (sem_ids, scores) from a batched 2-D pass, or None.  FUSION_MODEL keys: truncation
        (default DATA.init_value), max_weight (128), carve (False); with fuse_color, the images of a run go into the scene's
        colour volume as one call as well, and with fuse_label_probs its label images (the sem_ids the depth call fuses) into
        the scene's class-distribution volume.  With FUSION_MODEL.name 'tvl1' the depth call is Database.integrate_depth_hist
        (carve defaults to True; ids_est / scores are left alone), a run also ends where a scene's frame count reaches a
        multiple of tvl1_every, and Database.regularize(restart=False) follows it there."""
        from . import projective
        fm = self.config.FUSION_MODEL
        kw = dict(truncation=fm.get('truncation', None) or self.config.DATA.init_value,
                  max_weight=fm.get('max_weight', 128.0), carve=bool(fm.get('carve', False)))
        self._refuse_tripped_guard('Pipeline.fuse')  # (the labels of a 2-D pass that tripped the guard must not reach a volume)
        sem = bool(self.config.DATA.semantics)
        color_kw = self._color_options()
        label_kw = self._label_options()
        tv = self._tvl1_options()
        if tv is not None:
            kw['carve'] = bool(fm.get('carve', True))
        run, run_key = [], None

        def flush():
            if not run:
                return
            scene_id = run_key[0]
            volume = database[scene_id]
            # (frame, mask, K, E, sem_ids, scores, image) per frame: every stack of the run is made once and serves all three calls
            depth, mask, K, E = (torch.stack([r[i] for r in run]) for i in range(4))
            labels, label_scores = (torch.stack([r[i] for r in run]) for i in (4, 5)) if sem else (None, None)
            if self._depth_filter is not None:
                # once per run, for the depth, colour and label calls alike: what ``filter=`` on each of them would compute
                from . import frames
                depth, mask = frames.filtered(depth, mask, K, dict(self._depth_filter))
            if tv is not None:
                database.integrate_depth_hist(scene_id, depth, K, E, mask=mask, n_bins=tv['n_bins'], **kw)
                if self._tvl1_frames[scene_id] % tv['every'] == 0:
                    database.regularize(scene_id, lam=tv['lam'], iterations=tv['iterations'], restart=False, truncation=kw['truncation'])
            else:
                projective.integrate_depth(
                    volume['current'], volume['weights'], origin=volume['origin'], resolution=float(volume['resolution']),
                    depth=depth, mask=mask, intrinsics=K, extrinsics=E, ids=volume['ids_est'] if sem else None,
                    scores=volume['scores'] if sem else None, labels=labels, label_scores=label_scores, **kw)
                self._commit_frame(database, scene_id, volume)
            if color_kw is not None:
                database.integrate_color(scene_id, torch.cat([r[6] for r in run]), depth, K, E, mask=mask, **color_kw)
            if label_kw is not None:
                database.integrate_label_probs(scene_id, depth, K, E, mask=mask, labels=labels, **label_kw)
            del run[:]

        for b, s in zip(batches, sems):
            sem_ids, scores = self._labels2d.frame_semantics(b, self.device) if s is None else s
            scene_id, _, frame, mask = self._prepare_frame(b, None)[:4]
            key = (scene_id, tuple(frame.shape))
            if key != run_key or len(run) == _lib.PROJECTIVE_MAX_VIEWS:
                flush()
                run_key = key
            E = torch.as_tensor(b['extrinsics'][0]).detach().cpu().to(torch.float64)
            run.append((frame, mask, torch.as_tensor(b['intrinsics'][0]).detach().cpu().to(torch.float64), E[:3], sem_ids, scores,
                        b['image'].to(self.device) if color_kw is not None else None))
            self._frames_fused += 1
            if tv is not None:
                self._tvl1_frames[scene_id] = self._tvl1_frames.get(scene_id, 0) + 1
                if self._tvl1_frames[scene_id] % tv['every'] == 0:
                    flush()
                    run_key = None
        flush()

    # ---- several scenes per call (SURVEY.md §7 "hard parts") ------------------------------------------
    def fuse_many(self, batches, database, device):
        """``for b in batches: fuse(b, database, device)`` for frames of DISTINCT scenes (one frame each, one frame size),
        with the frame steps running side by side on the device: scene i of the call uses slot i - its own engine
        (activation buffers), est rows and integrate workspace - on its own stream, forked from and joined to the current
        stream.  The scenes' volumes do not overlap, every slot runs the kernels ``fuse`` runs with the same arguments, so the
        volumes come out bit for bit as from the separate calls; what changes is the schedule - the launches of one frame are
        latency-bound chains of 600-block kernels, and several of them fill the chip better (the two heads of a semantic net
        already run this way).  With ``semantic_strategy: predict`` the 2-D network of the S frames runs first, on the current
        stream (one engine).  The reference has no counterpart: its drivers fuse one frame at a time
        (test_fusion.py:68-80).  With FUSION_MODEL.fuse_color the frames' colour calls follow on the current stream, after the
        join, and with FUSION_MODEL.fuse_label_probs their label votes - for ``semantic_strategy: gt``; the learned modes refuse
        'predict' here (the ids of the batched 2-D pass stay inside the side-by-side frame steps; ``fuse`` and ``fuse_sequence``
        take it, and so does the classical mode)."""
        if self._tvl1:
            raise ValueError('Pipeline.fuse_many: FUSION_MODEL.name "tvl1" is supported by fuse and fuse_sequence only')
        if not self._classical and self._label_options() is not None and self.config.DATA.semantic_strategy == 'predict':
            raise ValueError('Pipeline.fuse_many: FUSION_MODEL.fuse_label_probs with semantic_strategy "predict" is supported by '
                             'fuse and fuse_sequence only (and by FUSION_MODEL.name "tsdf")')
        self._fuse_many_frames(batches, database, device)
        if not self._classical:  # (the classical frame steps bring their colour and label calls along)
            self._fuse_colors(batches, database)
            self._fuse_labels(batches, [None] * len(batches), database)

    def _fuse_many_frames(self, batches, database, device):
        self.device = torch.device(device)
        ids = [b['frame_id'][0].split('/')[0] for b in batches]
        if len(set(ids)) != len(ids):
            raise ValueError('Pipeline.fuse_many: one frame per scene (the frames of ONE scene depend on each other)')
        if self._classical:  # (one kernel per frame, each a sweep of its scene's own volume: nothing to run side by side)
            for b in batches:
                self._fuse_classical([b], [None], database)
            return
        recover = self._guard_policy() == 'f32'
        if len(batches) == 1 or self.device.type != 'cuda':
            for b in batches:
                self._fuse_guarded(b, database, recover=recover)
            return
        if len(batches) > _lib.MAX_SCENES:  # (the launches take up to MAX_SCENES scenes: larger calls go in groups)
            for i in range(0, len(batches), _lib.MAX_SCENES):
                self._fuse_many_frames(batches[i:i + _lib.MAX_SCENES], database, device)
            return
        main = torch.cuda.current_stream(self.device)
        sems = self._labels2d.frame_semantics_many(batches, self.device)  # (None, None) without semantics; predict: ONE batched pass, this stream
        fp = self._weights_fingerprint()
        streams = self._slot_streams
        while len(streams) < len(batches) - 1:
            streams.append(side_stream(self.device, [main] + streams))  # (a stream that runs beside the caller's and the other slots')
        enqueued = 0
        try:
            # 'auto' (default): the joint launches for two scenes, per-slot launches from three on - measured on one box (round 6,
            # profiles/r06_many_scene_launches.txt): joint 2246 against 2220 frames/s at S = 2, 2650 against 2747 at S = 4 (the two joins -
            # every net waits for the gather of ALL scenes, the scatter for ALL nets - cost more than the shared launches save)
            how = self.config.SETTINGS.get('fuse_many_launches', 'auto')
            if how == 'auto':
                how = 'joint' if len(batches) <= 2 else 'slots'
            if self._integrate_mode == MODE_FAST and how == 'joint':
                self._fuse_many_joint(batches, database, sems, fp, main, streams)
                enqueued = len(batches)
            else:  # PARITY integrate (its sort is per scene) / A-B switch: every slot runs fuse()'s own launches on its stream
                for i, (b, sem) in enumerate(zip(batches, sems)):
                    if i == 0:
                        self._fuse_frame(b, database, 0, sem, fp)
                    else:
                        st = streams[i - 1]
                        st.wait_stream(main)  # (the frame tensors and the labels were produced on the current stream)
                        with torch.cuda.stream(st):
                            self._fuse_frame(b, database, i, sem, fp)
                    enqueued = i + 1
        except _lib.OjfError as err:
            for st in streams[:len(batches) - 1]:
                main.wait_stream(st)
            if not recover or 'fp16 range' not in str(err):
                raise
            # guard_policy 'f32': the frames of this call that were enqueued behind the event are among the skipped ones
            # (remember them first); the one the poll refused and those after it follow, one at a time on the fp32 engine
            for i, b in enumerate(batches[:enqueued]):
                self._guard.remember(b, database, i)
            self._guard_recover(err)
            for b, sem in zip(batches[enqueued:], sems[enqueued:]):
                self._fuse_guarded(b, database, sem, None, True)
            return
        for st in streams[:len(batches) - 1]:
            main.wait_stream(st)
        if recover:
            for i, b in enumerate(batches):
                self._guard.remember(b, database, i)  # (scene i ran on slot i: its own record)

    def _fuse_many_joint(self, batches, database, sems, fp, main, streams):
        """fuse_many's frame steps with the gather and the scatter of ALL scenes as single launches (round 6):

            ops.extract_many     one launch, blockIdx.y = scene       caller's stream
            S fusion nets        slot i on its own stream, forked from / joined to the caller's (as before)
            ops.integrate_many   accumulate + finalize of all scenes  caller's stream

        extract / accumulate / finalize are one round of blocks that each walk a chain of dependent steps (DESIGN.md 5.0c:
        0.017 of the HBM roofline, 70 % parked): S scenes in ONE launch share the ramp and keep the CUs busy while other
        blocks wait, which S launches on S streams do not.  Per scene the same blocks run the same code as in ``fuse``: the
        volumes come out bit for bit the same.  Raises (the poll below, a net's forward call) before ANY integrate launch of
        the call has been enqueued: none of the call's frames is among the skipped ones."""
        self._refuse_tripped_guard('Pipeline.fuse_many')
        P, n_tail = self.n_points, self.config.FUSION_MODEL.n_tail_points
        use_sem, sem = self.config.FUSION_MODEL.use_semantics, bool(self.config.DATA.semantics)
        prep = []
        for i, (b, (sem_ids, scores)) in enumerate(zip(batches, sems)):
            scene_id, volume, frame, mask, Ki, E, h, w = self._prepare_frame(b, database)
            sl = self._get_slot(h, w, self.device, i, fp)
            ws = self._get_workspace(volume['current'].shape, h, w, self.device, i)
            job = dict(depth=frame, Ki=Ki, E=E, origin=volume['origin'], resolution=volume['resolution'], tsdf=volume['current'], weights=volume['weights'])
            if sem:
                job.update(sem_ids=sem_ids, sem_scores=scores, id_vol=volume['ids_est'], score_vol=volume['scores'])  # (the gather ignores them)
            prep.append(dict(scene=scene_id, frame=frame, volume=volume, slot=sl, sem_ids=sem_ids, job=job, scatter=dict(job, mask=mask, est=sl.est, workspace=ws)))
        if len({(p['frame'].shape, p['volume']['current'].shape) for p in prep}) != 1:
            raise ValueError('Pipeline.fuse_many: one frame size and one grid size per call')
        fused = prep[0]['slot'].engine.fused_input
        self._mark(first=True)  # (profile: four events per CALL - gather of all scenes | nets | scatter of all scenes)
        ops.extract_many([dict(p['job'], **(dict(engine=p['slot'].engine) if fused else dict(out_values=p['slot'].fv, out_weights=p['slot'].fw)))
                          for p in prep], n_points=P)
        self._mark()
        for i, p in enumerate(prep):
            sl = p['slot']
            if i:
                streams[i - 1].wait_stream(main)
            with torch.cuda.stream(streams[i - 1] if i else main):
                if not fused:
                    sl.engine.prepare_input(sl.fv, sl.fw, p['frame'], p['sem_ids'] if use_sem else None, self.n_classes if use_sem else 0, planes=True)
                sl.engine.forward(sl.est)
        for st in streams[:len(prep) - 1]:
            main.wait_stream(st)
        self._mark()
        ops.integrate_many([p['scatter'] for p in prep], n_points=P, n_tail=n_tail, trunc=self.config.DATA.init_value)
        for i, p in enumerate(prep):  # (every scene of the launch latches for itself)
            self._guard.note(i, p['scatter']['workspace'])
        self._mark()
        self._frames_fused += len(prep) - 1  # (the first mark counted one)
        for p in prep:
            self._commit_frame(database, p['scene'], p['volume'])

    def _training_forward(self, inputs):
        """The net forward of pipeline.py:322 with a graph for ``loss.backward()``: on the libojf training kernels
        (train.HipTrainNet: ``FUSION_MODEL.train_engine: hip``, default on a GPU) or on torch autograd (``torch``)."""
        if self.config.FUSION_MODEL.get('train_engine', 'hip') == 'hip' and self.device.type == 'cuda':
            tn = self._hip_train
            if tn is None or tn.net is not self._fusion_network:
                from .train import HipTrainNet
                tn = self._hip_train = HipTrainNet(self._fusion_network, graph=self.config.FUSION_MODEL.get('train_graph', False),
                                                               inplace_grads=True, arithmetic=self.config.FUSION_MODEL.get('train_arithmetic', 'f16x3'),
                                                               backward_arithmetic=self.config.FUSION_MODEL.get('train_arithmetic_bwd', None),
                                                               replay=self.config.FUSION_MODEL.get('train_replay', None),
                                                               overlap=self.config.FUSION_MODEL.get('train_overlap', False),
                                                               overlap_thread=self.config.FUSION_MODEL.get('train_overlap_thread', False))
            return tn(inputs)
        return self._fusion_network.forward(inputs)

    def gradients(self):
        """``with pipeline.gradients():`` around everything between ``loss.backward()`` and the next ``fuse_training`` that touches the
        fusion net's gradients or writes its parameters (train_fusion.py:182-189: clip_grad_norm_, optimizer.step(), zero_grad()).  With
        ``FUSION_MODEL.train_overlap`` the backward pass of a frame runs on a stream of its own beside the next frame's forward stage and
        this context puts its body on that stream; without it (the default) the context does nothing."""
        tn = self._hip_train
        if tn is not None:
            return tn.gradients()
        import contextlib
        return contextlib.nullcontext()

    def gradient_work(self, fn, join=True):
        """``fn()`` behind the backward passes enqueued so far - the function form of ``with pipeline.gradients(): ...`` that a host thread
        of the pipeline's own can run (``FUSION_MODEL.train_overlap_thread``, default off: measured neutral): the caller does not wait
        for the backward pass's launch loop.  ``join=False`` only for an ``fn`` that writes no parameter (train.HipTrainNet.gradient_work)."""
        tn = self._hip_train
        if tn is not None:
            return tn.gradient_work(fn, join=join)
        fn()

    def join_gradients(self):
        """The current stream waits for the gradient stream (before checkpoints, validation, host reads of gradients or freshly stepped
        weights); a no-op without ``FUSION_MODEL.train_overlap``.  The next ``fuse_training`` joins by itself when a weight changed."""
        tn = self._hip_train
        if tn is not None:
            tn.join_gradients()

    # ---- training frame step (pipeline.py:251-363) -----------------------------------------------
    def announce_training_frame(self, batch, device=None):
        """Tells the pipeline which batch the ``fuse_training`` call AFTER the coming one will bring (the same object; call order
        announce(i + 1), fuse_training(i) - announcing the very next call's batch works too).  Up to two announcements are held,
        matched by object identity and consumed by the first ``fuse_training`` that brings the object; ``None`` clears them
        (announce.TrainingAnnouncements).  The part of that frame
        step that depends on the batch alone - the filtered frame of pipeline.py:196 and the number of valid rays, the one value
        the host must read to shape ``tsdf_fused`` / ``tsdf_target`` [1, Nv, 9] - is enqueued NOW, in front of the current
        frame's work, so that its answer is on the host long before the next call asks for it.  Without the announcement the count
        is requested at the start of its own frame: the read then waits until the device has drained the previous frame, which
        ties the host to the device once per frame - on a host that needs longer to enqueue a backward pass than the device
        needs for the forward pass, the device starves (round 6: 3.2 ms of host work and 4.25 ms of device work per frame took
        4.8-5.5 ms).  With it the host may run up to one frame ahead.  Optional and bit-neutral: the same launches, earlier.  The
        reference has no counterpart (its ``nonzero`` drains the queue in the middle of every frame, pipeline.py:125-131)."""
        if batch is None:
            return self._announcements.announce(None)
        if device is not None:
            self.device = torch.device(device)
        self._announcements.announce(batch, *self._frames(batch))

    def fuse_training(self, batch, database, device):
        if self._classical:
            raise RuntimeError('Pipeline.fuse_training: FUSION_MODEL.name "tsdf" is classical TSDF averaging - there is no '
                               'network to train (use "v2" or "v3")')
        self.device = torch.device(device)
        sem_ids, scores = self._labels2d.frame_semantics(batch, self.device)
        ann = self._announcements.take(batch, self.device)
        if ann is not None:
            frames, valid_mask, count = tuple(ann[1:3]), ann[3], ann[4]  # (enqueued a frame ago: the count is on the host by now)
        else:
            frames = valid_mask = count = None
        scene_id, volume, frame, filtered, Ki, E, h, w = self._prepare_frame(batch, database, filtered=True, frames=frames)
        n, P = h * w, self.n_points
        tsdf, weights = volume['current'], volume['weights']

        # The shapes [1, Nv, P] of the masked outputs (pipeline.py:125-131) need the number of valid rays on the host: the one
        # device -> host read of the frame step.  The count is REQUESTED here (one reduction + an asynchronous copy into
        # pinned memory, behind an event) and awaited only after extract and the net's forward pass have been enqueued: by
        # then the copy is long done, the host never drains the queue, and it runs ahead of the device through loss and
        # backward.  (Read with a blocking ``nonzero`` after the net forward - the reference's order - the queue drained in
        # the middle of every frame and the device idled while Python enqueued the loss: 2.7 of 10.4 ms per 320x240 frame.)
        if valid_mask is None:
            valid_mask = filtered.reshape(n) != 0
            count = self._announcements.async_count(valid_mask)

        # sample planes [P, n] are NCHW [1, P, h, w] as they stand: no permute / contiguous copies in front of the net
        cur = ops.extract(frame, Ki, E, volume['origin'], volume['resolution'], tsdf, weights, n_points=P, planes=True)
        gt = ops.extract(frame, Ki, E, volume['origin'], volume['resolution'], volume['gt'], weights, n_points=P)
        fv, fw = cur['fusion_values'], cur['fusion_weights']
        inputs = {'tsdf_values': fv.view(1, P, h, w), 'tsdf_weights': fw.view(1, P, h, w), 'tsdf_frame': frame.view(1, 1, h, w)}
        if self.config.FUSION_MODEL.use_semantics:
            inputs['semantic_frame'] = ((1 + sem_ids.float()) / self.n_classes).view(1, 1, h, w)
        try:
            est_pn = self._training_forward(inputs)[:, :P].reshape(1, P, n)  # differentiable; BN / dropout follow the modules' modes
        except _lib.OjfError as err:
            # the executor's forward refuses to run while the shared range-guard flag is set and leaves it set (include/ojf.h):
            # report + clear it here, so that a training loop that catches the error and carries on (another arithmetic, the
            # next scene) does not have every later integrate call skip silently
            if 'fp16 range' in str(err) and self.device.type == 'cuda':
                _lib.load().ojf_net_check(_lib.stream_ptr(self.device))
            raise
        valid = self._announcements.valid_index(valid_mask, count)

        # pipeline.py:104-135 in the plane layout, one launch each way; the [1, n, P] tensor of the API is a transposed view
        init = self.config.DATA.init_value
        from .train import FuseOutput
        tsdf_fused = FuseOutput.apply(est_pn, fv.view(1, P, n), fw.view(1, P, n), valid, init)
        output = {'tsdf_est': est_pn.transpose(1, 2), 'tsdf_fused': tsdf_fused,
                  'tsdf_target': gt['fusion_values'].view(1, n, P)[:, valid, :]}

        ws = self._get_workspace(tsdf.shape, h, w, self.device)
        est_rows = est_pn.detach()[0].t().contiguous()
        ops.integrate(filtered, Ki, E, volume['origin'], volume['resolution'], est_rows, tsdf, weights, ws,
                      n_points=P, n_tail=self.config.FUSION_MODEL.n_tail_points, trunc=init,
                      mode=self._integrate_mode)  # test=False: no semantic update (pipeline.py:357)
        self._commit_frame(database, scene_id, volume)
        return output
