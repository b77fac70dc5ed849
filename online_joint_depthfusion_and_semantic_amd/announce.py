"""Training frames announced ahead of their ``fuse_training`` call (pipeline.Pipeline.announce_training_frame): the held
announcements with the valid-ray count each one requested early, and the pinned buffers those counts travel in."""
import torch


class TrainingAnnouncements:

    def __init__(self):
        # [batch, frame, filtered, valid_mask, count, fuse_training calls of OTHER batches it has seen]; at most two
        self.held = []
        self.hits = self.misses = 0  # take() calls that found / did not find their batch announced
        self._count_slots = []  # (pinned int32 buffer, event) of async_count, a ring of four
        self._count_at = 0  # async_count requests so far

    def async_count(self, mask_flat):
        """Number of set elements of a device bool vector, on its way to the host: (pinned int32 buffer, event)."""
        if not mask_flat.is_cuda:
            return int(mask_flat.sum())
        slots = self._count_slots
        # A ring of four.  A frame step that was not announced reads its slot inside the same call.  An announcement's slot is read
        # by the fuse_training call after next at the latest (take drops it then); with an announcement and a miss in
        # every frame the requests in between are: the miss of the frame step in front of it, the next announcement, and - when
        # it is dropped instead of read - the miss of its own frame step.  That is at most three newer requests while a value is
        # still wanted, so the slot that the fourth reuses has been read or given up.
        if len(slots) < 4:
            slots.append((torch.empty(1, dtype=torch.int32).pin_memory(), torch.cuda.Event()))
        buf, ev = slots[self._count_at % len(slots)]
        self._count_at += 1
        buf.copy_(mask_flat.sum(dtype=torch.int32).reshape(1), non_blocking=True)
        ev.record(torch.cuda.current_stream(mask_flat.device))
        return buf, ev

    @staticmethod
    def valid_index(mask_flat, count):
        """``mask.nonzero()[:, 0]`` without draining the stream: the size comes from async_count."""
        if isinstance(count, int):
            return mask_flat.nonzero()[:, 0]
        buf, ev = count
        ev.synchronize()
        nv = int(buf[0])
        try:
            return torch.nonzero_static(mask_flat, size=nv)[:, 0]
        except (RuntimeError, NotImplementedError):  # builds without the device kernel: the blocking form
            return mask_flat.nonzero()[:, 0]

    def announce(self, batch, frame=None, filtered=None):
        """Holds ``batch`` with its (frame, filtered frame) pair (Pipeline._frames) and requests its valid-ray count now;
        ``None`` clears the held announcements.  Up to two are held: the one waiting for the frame step in between, and this one."""
        if batch is None:
            self.held = []
            return
        valid_mask = filtered.reshape(frame.numel()) != 0
        self.held.append([batch, frame, filtered, valid_mask, self.async_count(valid_mask), 0])
        del self.held[:-2]

    def take(self, batch, device):
        """The announcement of ``batch`` (the same object, on this call's device) or None, for ``fuse_training``.  The documented
        order is announce(i + 1), fuse_training(i): an announcement outlives ONE frame step of another batch and is dropped by the
        second, as is one made for another device.  ``hits`` / ``misses`` count the calls either way."""
        hit, keep = None, []
        # ('cuda' and 'cuda:<current>' are one device: a frame tensor's device always carries its index)
        dev = torch.empty(0, device=device).device
        for a in self.held:
            if a[1].device != dev:
                continue
            if hit is None and a[0] is batch:
                hit = a
            elif a[5] == 0:
                a[5] = 1
                keep.append(a)
        self.held = keep
        if hit is None:
            self.misses += 1
        else:
            self.hits += 1
        return hit
