"""The 2-D label front end of the pipeline (modules/pipeline.py:42-60, 181-193): a frame's (label ids, scores) from semantic_gt or
from the AdapNet++ network - the SEGCONV engine cache, the device-graph captures of the one-frame and the batched pass, and
fuse_sequence's look-ahead prefetch with its side-stream selection.  Not an nn.Module: the network stays Pipeline's child and is
read through ``network()``, from the pipeline's sub-module dict, at call time (drivers and tests replace and retrain it; the
caches key on id(net) and the version counters)."""
import torch

from . import _lib


def side_stream(device, others):
    """A torch stream whose kernels really run beside those of ``others``: the runtime backs all streams by a small
    round-robin pool of hardware queues, and two streams on one queue take turns (measured: the look-ahead pass beside
    the frame steps 933 frames/s on two queues, 775 on one).  Up to eight candidates are tried (ojf_streams_overlap, a
    set-up cost of ~0.5 ms each); the rejected ones stay referenced until the choice is made, so that the next candidate
    is another pool member."""
    lib = _lib.load()
    rejected, best = [], None
    for _ in range(8):
        cand = torch.cuda.Stream(device=device)
        if all(lib.ojf_streams_overlap(o if isinstance(o, int) else o.cuda_stream, cand.cuda_stream) == 1 for o in others):
            return cand
        best = best or cand
        rejected.append(cand)
    return best


class LabelFrontEnd:

    def __init__(self, config, modules):
        self.config = config
        self._modules = modules  # the pipeline's own sub-module dict, read at call time
        self.seg_cache = None  # the SegEngine with the tensor list and version key it was built from
        self.seg_graph = None  # device graph of the one-frame pass: {'key', 'graph', in/out buffers}
        self.seg_graph_many = None  # device graph of the batched pass, per (S, frame shape)
        self.prefetch = None  # look-ahead record: side stream, two result slots, the chunk that is ready, 'hits'
        self.warned_seg_fallback = False  # the frame-size warning of seg_engine is given once

    def network(self):
        """The pipeline's current _semantic_2d_network (None without the predict strategy)."""
        return self._modules.get('_semantic_2d_network')

    def segmentation(self, data, device):
        inputs = {'image': (data['image'] / 255.0).to(device).float()}
        in_ = self.config.DATA.input
        if in_ != 'image':
            inputs[in_] = data[in_].repeat(1, 3, 1, 1).to(device).float()
        net = self.seg_engine(inputs['image'].shape, device) or self.network()
        if self.config.SEMANTIC_2D_MODEL.stage == 1:
            output = net(inputs[in_])
        else:
            output = net(inputs['image'], inputs[in_])
        logits = output if torch.is_tensor(output) else output[0]  # the engine returns the main head only
        return torch.softmax(logits, dim=1).permute(0, 2, 3, 1)

    def segment_max(self, data, device):
        """``segmentation(data).max(dim=-1)`` -> (scores, ids).  With the HIP engine the whole chain - image / 255,
        depth x 3, AdapNet++, softmax, max - is libojf launches (SegEngine.predict); ids come back as uint8."""
        image = data['image']
        engine = self.seg_engine(image.shape, device)
        if engine is None:
            return self.segmentation(data, device).max(dim=-1)
        in_ = self.config.DATA.input
        depth = data[in_].to(device).float() if in_ != 'image' else None
        h, w = image.shape[-2:]
        scores, ids = engine.predict(image.to(device).float(), depth)
        return scores.view(1, h, w), ids.view(1, h, w)

    def seg_engine(self, shape, device):
        """The AdapNet++ convolutions on the SEGCONV HIP kernels (adapnet_engine.SegEngine) when the front-end runs
        inference on the GPU: ``SEMANTIC_2D_MODEL.engine: hip`` (default) | ``torch`` (module forward, MIOpen).
        Rebuilt when the parameters change (version counters, checked like the fusion net's)."""
        net = self.network()
        if (self.config.SEMANTIC_2D_MODEL.get('engine', 'hip') != 'hip' or net.training or torch.is_grad_enabled()
                or torch.device(device).type != 'cuda' or shape[0] != 1):
            return None
        if shape[-2] % 16 or shape[-1] % 16:
            if not self.warned_seg_fallback:
                import warnings
                self.warned_seg_fallback = True
                warnings.warn('SEMANTIC_2D_MODEL.engine = hip needs frame sides that are multiples of 16 (the 1/16-resolution '
                              'stage of AdapNet++): %dx%d frames run on the torch module forward instead' % (shape[-2], shape[-1]),
                              RuntimeWarning)
            return None
        cache = self.seg_cache
        if cache is None or cache['net'] != id(net) or cache['age'] >= 64:
            tensors = list(net.parameters()) + list(net.buffers())
            cache = {'net': id(net), 'tensors': tensors, 'age': 0, 'key': None, 'engine': None} if cache is None or cache['net'] != id(net) \
                else dict(cache, tensors=tensors, age=0)
            self.seg_cache = cache
        cache['age'] += 1
        key = (len(cache['tensors']), sum(t._version for t in cache['tensors']), str(device))
        if cache['engine'] is None or cache['key'] != key:
            from .adapnet_engine import SegEngine
            cache['engine'], cache['key'] = SegEngine(net), key
        return cache['engine']

    def segmentation_graph(self, data, device):
        """Inference-time replay of ``segmentation(...).max(-1)``: captured once per frame shape (and engine) into a
        device graph.  320x240: torch module 772 launches, 9.1 ms eager / 4.5 ms replayed; SEGCONV engine 215 launches,
        2.6 ms eager / 2.3 ms replayed.  Parameters are read in place, so ``load_state_dict`` /
        optimizer steps are seen; ``SEMANTIC_2D_MODEL.graph: False`` or a failed capture falls back to eager."""
        image = data['image']
        in_ = self.config.DATA.input
        depth = data[in_] if in_ != 'image' else None
        with torch.no_grad():
            engine = self.seg_engine(image.shape, device)  # a rebuilt engine owns new weight buffers: recapture
        key = (tuple(image.shape), str(device), id(self.network()), id(engine))
        st = self.seg_graph
        if st is None or st['key'] != key:
            st = self.seg_graph = {'key': key, 'graph': None}
            try:
                st['image'] = torch.zeros(image.shape, dtype=image.dtype, device=device)
                st['depth'] = torch.zeros(depth.shape, dtype=depth.dtype, device=device) if depth is not None else None
                batch = {'image': st['image']}
                if depth is not None:
                    batch[in_] = st['depth']
                side = torch.cuda.Stream(device=device)
                side.wait_stream(torch.cuda.current_stream(device))
                with torch.cuda.stream(side):  # library workspaces and autotuning must be settled before the capture
                    for _ in range(3):
                        self.segment_max(batch, device)
                torch.cuda.current_stream(device).wait_stream(side)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    st['scores'], st['ids'] = self.segment_max(batch, device)
                st['graph'] = graph
            except Exception:  # capture is an optimisation only
                st['graph'] = None
        if st['graph'] is None:
            return self.segment_max(data, device)
        st['image'].copy_(image, non_blocking=True)
        if depth is not None:
            st['depth'].copy_(depth.reshape(st['depth'].shape), non_blocking=True)
        st['graph'].replay()
        return st['scores'], st['ids']

    def frame_semantics(self, batch, device):
        if not self.config.DATA.semantics:
            return None, None
        strategy = self.config.DATA.semantic_strategy
        if strategy == 'predict':
            with torch.no_grad():
                use_graph = (self.config.SEMANTIC_2D_MODEL.get('graph', True) and not self.network().training
                             and torch.device(device).type == 'cuda')
                if use_graph:
                    scores, sem_ids = self.segmentation_graph(batch, device)
                else:
                    scores, sem_ids = self.segment_max(batch, device)
        elif strategy == 'gt':
            sem_ids = batch['semantic_gt']
            scores = torch.ones_like(sem_ids, dtype=torch.float32)
        else:
            raise ValueError('Valid values for DATA.semantic_strategy are "gt" or "predict".')
        h, w = sem_ids.shape[-2:]
        sem_ids = sem_ids.to(device).to(torch.uint8).reshape(h * w).contiguous()
        scores = scores.to(device).float().reshape(h * w).contiguous()
        return sem_ids, scores

    def batched_pass_applies(self, batches):
        cfg = self.config
        return bool(cfg.DATA.semantics and cfg.DATA.semantic_strategy == 'predict' and len(batches) > 1
                    and not self.network().training and cfg.SEMANTIC_2D_MODEL.get('stage', 2) != 1)

    def _measured_side_stream(self, cur, frames, device, replay_net):
        """The look-ahead stream by measurement: which hardware queue a new stream gets, and whose packets it then waits
        behind, is the runtime's business (a stream that passes ojf_streams_overlap against every stream we know of still ran
        the pass 20 % slower than its neighbour in the pool: 780 against 940 frames/s at four frames per chunk).  Six candidate
        streams each replay the batched 2-D pass beside ``frames`` forward passes of the fusion net on the caller's stream
        (``replay_net()``: the executor recomputes its last frame's estimate, no volume is touched); the fastest is kept.
        ~30 ms, once."""
        st = self.seg_graph_many
        if not st or st.get('graph') is None or replay_net is None:
            return None
        best, best_ms, cands = None, None, []
        with torch.no_grad():
            for _ in range(6):
                cand = torch.cuda.Stream(device=device)
                cands.append(cand)  # (kept alive: the next candidate is another member of the pool)
                ms = []
                for _rep in range(3):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(cur)
                    cand.wait_stream(cur)
                    with torch.cuda.stream(cand):
                        st['graph'].replay()
                    for _f in range(frames):
                        replay_net()
                    cur.wait_stream(cand)
                    e1.record(cur)
                    e1.synchronize()
                    ms.append(e0.elapsed_time(e1))
                t = min(ms[1:])
                if best is None or t < best_ms:
                    best, best_ms = cand, t
        return best

    @staticmethod
    def _net_side_streams(net_engine):
        """Raw handles of the fusion net's own side streams (the second head of the two-head net runs on one): the look-ahead
        pass must not share a hardware queue with them either (measured: 775 frames/s when it does, 930-1070 when not)."""
        try:
            return net_engine.side_streams() if net_engine is not None and hasattr(net_engine, 'side_streams') else []
        except Exception:
            return []

    def prefetch_semantics(self, batches, device, net_engine=None, replay_net=None):
        """The batched 2-D pass of ``batches`` on the side stream; the labels land in one of two persistent result slots
        (the graph's own output buffers belong to the next replay).  Slot k % 2 was last read by the frame steps of the
        chunk two calls ago: they are in front of the side stream's wait on the caller's stream.  ``net_engine``: the fusion
        net's executor, ``replay_net``: a callable that runs its last forward pass again - both None while no executor exists."""
        if not self.batched_pass_applies(batches):
            return
        cur = torch.cuda.current_stream(device)
        pf = self.prefetch
        # 'measured' (_measured_side_stream, round 5) | 'priority' (below) | 'probe': the first stream that passes ojf_streams_overlap
        how = self.config.SETTINGS.get('lookahead_stream', 'measured')
        if pf is None:
            net_streams = self._net_side_streams(net_engine)
            if how == 'priority':
                # a stream of ANOTHER priority class: the runtime keeps one pool of hardware queues per priority, so this stream never
                # shares a queue with the caller's (normal-priority) stream or the net's side streams - by construction, not by probing
                side = torch.cuda.Stream(device=device, priority=-1)
            else:
                side = side_stream(device, [cur] + net_streams)
            pf = self.prefetch = {'stream': side, 'n': 0, 'slots': [None, None], 'ready': None, 'taken': False, 'measured': how != 'measured',
                                  'net_seen': bool(net_streams) or net_engine is not None}
        elif not pf.get('measured') and replay_net is not None and (self.seg_graph_many or {}).get('graph') is not None:
            # (once, when both networks' launch sequences exist: the stream is chosen by what it does to the real work)
            old = pf['stream']
            pf['stream'] = self._measured_side_stream(cur, len(batches), device, replay_net) or old
            pf['stream'].wait_stream(old)
            pf['measured'] = True
        side = pf['stream']
        side.wait_stream(cur)
        with torch.cuda.stream(side), torch.no_grad():
            sems = self.frame_semantics_many(batches, device)
            if sems[0][0] is None:
                return
            k = pf['n'] % 2
            slot = pf['slots'][k]
            if slot is None or len(slot) != len(sems) or slot[0][0].shape != sems[0][0].shape:
                side.synchronize(); cur.synchronize()  # (first use / another chunk shape: allocate the slot once, outside any overlap)
                slot = pf['slots'][k] = [(torch.empty_like(i), torch.empty_like(sc)) for i, sc in sems]
            for (di, dsc), (i, sc) in zip(slot, sems):
                di.copy_(i, non_blocking=True)
                dsc.copy_(sc, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(side)
        pf['n'] += 1
        # the announced batch OBJECTS are held (and compared with `is`): an id() of a dict the caller has dropped can be handed to a
        # new dict, and the stale labels of other frames would be fused silently
        pf['ready'] = {'batches': list(batches), 'sems': slot, 'event': ev}

    def take_prefetched(self, batches, device):
        pf = self.prefetch
        if pf:
            pf['taken'] = False
        if not pf or not pf['ready']:
            return None
        ready, pf['ready'] = pf['ready'], None
        cur = torch.cuda.current_stream(device)
        cur.wait_event(ready['event'])  # (also orders this call's own 2-D pass, if the chunk is another one, behind the side stream's use of the graph buffers)
        pf['taken'] = len(ready['batches']) == len(batches) and all(a is b for a, b in zip(ready['batches'], batches))
        pf['hits'] = pf.get('hits', 0) + int(pf['taken'])
        return ready['sems'] if pf['taken'] else None

    def frame_semantics_many(self, batches, device):
        """``[frame_semantics(b) for b in batches]``; with ``semantic_strategy: predict`` on the HIP engine the S frames go
        through the 2-D network as ONE batched pass (SegEngine.predict_many: every layer's weights fetched once for all
        frames), replayed from a device graph per (S, frame shape)."""
        cfg = self.config
        if (not cfg.DATA.semantics or cfg.DATA.semantic_strategy != 'predict' or len(batches) == 1
                or self.network().training or cfg.SEMANTIC_2D_MODEL.get('stage', 2) == 1):
            return [self.frame_semantics(b, device) for b in batches]
        with torch.no_grad():
            engine = self.seg_engine(batches[0]['image'].shape, device)
            if engine is None:
                return [self.frame_semantics(b, device) for b in batches]
            in_ = cfg.DATA.input
            images = [b['image'].to(device).float() for b in batches]
            depths = [b[in_].to(device).float() for b in batches] if in_ != 'image' else None
            S = len(batches)
            h, w = images[0].shape[-2:]
            key = (S, tuple(images[0].shape), None if depths is None else tuple(depths[0].shape), str(device), id(engine))
            st = self.seg_graph_many
            if st is None or st['key'] != key:
                st = self.seg_graph_many = {'key': key, 'graph': None}
                if cfg.SEMANTIC_2D_MODEL.get('graph', True):
                    try:
                        st['images'] = [torch.zeros_like(im) for im in images]
                        st['depths'] = [torch.zeros_like(d) for d in depths] if depths is not None else None
                        side = torch.cuda.Stream(device=device)
                        side.wait_stream(torch.cuda.current_stream(device))
                        with torch.cuda.stream(side):
                            for _ in range(2):
                                engine.predict_many(st['images'], st['depths'])
                        torch.cuda.current_stream(device).wait_stream(side)
                        graph = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(graph):
                            st['scores'], st['ids'] = engine.predict_many(st['images'], st['depths'])
                        st['graph'] = graph
                    except Exception:  # capture is an optimisation only
                        st['graph'] = None
            if st['graph'] is None:
                scores, ids = engine.predict_many(images, depths)
            else:
                for dst, src in zip(st['images'], images):
                    dst.copy_(src, non_blocking=True)
                if depths is not None:
                    for dst, src in zip(st['depths'], depths):
                        dst.copy_(src.reshape(dst.shape), non_blocking=True)
                st['graph'].replay()
                scores, ids = st['scores'], st['ids']
            return [(ids[i].contiguous(), scores[i].contiguous()) for i in range(S)]
