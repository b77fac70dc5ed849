"""What a range-guard recovery (FUSION_MODEL.guard_policy 'f32', pipeline.Pipeline._guard_recover) needs to know of the frames
fused so far: the ring of remembered (batch, database) pairs, each with the latched decision of ITS integrate call, and the
event marks that bound how many of them are kept."""
import torch

from . import _lib


def guard_frames_to_fuse_again(ring, records, device_count):
    """Which remembered frames a range-guard recovery fuses again (FUSION_MODEL.guard_policy 'f32').  ``ring``: the remembered
    frames in the order they were fused; ``records``: per frame, whether ITS integrate call skipped (the call's own latched
    decision, GuardRecords.note); ``device_count``: the number of skipped integrate calls the device counted since the last
    report.  Returns the skipped frames, in ring order - they need not be the last ones: with a stream per scene a later slot may
    have latched "not set" before an earlier slot's net raised the flag.  Raises OjfError when the records and the device
    disagree (a frame was skipped that nobody remembers, or the other way round): nothing can be fused again reliably then."""
    if len(records) != len(ring):
        raise _lib.OjfError('range guard: %d frames are remembered but %d records of their integrate calls' % (len(ring), len(records)))
    again = [frame for frame, skipped in zip(ring, records) if skipped]
    if len(again) != int(device_count):
        raise _lib.OjfError('range guard: the device counted %d skipped frames, the records of the %d remembered frames say %d'
                            % (int(device_count), len(ring), len(again)))
    return again


def guard_policy(config):
    """FUSION_MODEL.guard_policy as it holds now: 'raise' unless the net runs the split-fp16 arithmetic (nothing to switch to)."""
    if config.FUSION_MODEL.get('arithmetic', 'f16x3') != 'f16x3':
        return 'raise'
    return config.FUSION_MODEL.get('guard_policy', 'raise')


def _record_event(device):
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(device))
    return ev


def _guard_is_set():
    return _lib.load().ojf_guard_poll()


class GuardRecords:
    # The batches of the last <= KEEP frames stay alive for a recovery; an event every EVERY frames bounds how far the host may
    # run ahead of the device.
    EVERY, KEEP = 16, 48

    def __init__(self, config, record_event=_record_event, guard_is_set=_guard_is_set):
        """``config``: the pipeline's (nothing is kept unless guard_policy(config) says 'f32').  ``record_event(device)`` makes
        an event and records it on the current stream of ``device`` (the result needs ``synchronize()``); ``guard_is_set()``
        is the host read of the guard flag: the two ties to a device, replaceable by stand-ins on a host."""
        self.config, self.record_event, self.guard_is_set = config, record_event, guard_is_set
        self.ring = []  # (batch, database, latch) per remembered frame, in the order they were fused
        self.marks = []  # [ring length when recorded, event], oldest first
        self.latches = {}  # slot -> latch copy of the slot's last integrate call, until remember() hands it to its frame

    def note(self, slot, workspace):
        """Keeps, per slot, a copy of the decision the integrate call just enqueued on this stream will have taken
        (ops.IntegrateWorkspace.guard_latch: the slot's workspace is reused by the slot's next call).  The healthy path's
        whole cost: 4 bytes, device to device, per frame; nothing is read before a recovery."""
        if guard_policy(self.config) == 'f32':
            self.latches[slot] = workspace.guard_latch()

    def remember(self, batch, database, slot=0):
        if guard_policy(self.config) != 'f32':  # (a frame fused behind a recovery, on the fp32 engine: there is nothing to recover to)
            return
        ring, marks = self.ring, self.marks
        latch = self.latches.pop(slot, None)
        ring.append((batch, database, latch))
        if len(ring) % self.EVERY == 0:  # (on the caller's stream of the device the frame was fused on: its latch's)
            marks.append([len(ring), self.record_event(None if latch is None else latch.device)])
        if len(ring) > self.KEEP:
            upto, ev = marks.pop(0)
            ev.synchronize()  # (long done unless the host is > 32 frames ahead of the device)
            if not self.guard_is_set():  # the frames in front of that event were fused with the guard silent
                del ring[:upto]
                for m in marks:
                    m[0] -= upto

    def take(self, device_count):
        """For a recovery, after the device has been drained: (the frames to fuse again as (batch, database), in ring order;
        per remembered frame, in order, (frame_id, did its integrate call skip)).  One host read of all latches.  Raises
        OjfError on a frame without a record, or when the records and ``device_count`` disagree.  Leaves nothing remembered."""
        ring = self.ring
        # (every stream that fused a remembered frame has been joined to the caller's, which ojf_guard_status has drained: one read)
        latches = [r[2] for r in ring]
        if any(l is None for l in latches):
            raise _lib.OjfError('range guard: a remembered frame has no record of its integrate call')
        records = torch.stack(latches).cpu().ne(0).any(dim=1).tolist() if latches else []
        redo = guard_frames_to_fuse_again([r[:2] for r in ring], records, device_count)
        skips = [(r[0]['frame_id'][0], s) for r, s in zip(ring, records)]
        self.ring, self.marks, self.latches = [], [], {}
        return redo, skips
