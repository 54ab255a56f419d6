"""Decoded frames kept on the device across clips.

The reference's clips are index lists (dataset_helper.get_sequence) and the clips of a bank-construction pass overlap
heavily: Charades centres lie 12 frames apart and a 32-frame clip at rate 4 spans 128, so 29 of its 32 frames were in the
previous clip; the three spatial shifts of a test segment are the same frames; a sequence clamped at a video's end repeats
one.  Test-mode preprocessing is deterministic, so these are the same bytes.  A `FrameStore` holds the last `capacity`
frames of one size in device memory; a clip is handed to the loader as `(store, video, frame_numbers)`
(datasets.clip_loader.FrameLoader), `slots` uploads only the frames that are not resident, and the preprocess kernels read
the clip through a table of slot numbers (vlfb_clip_batch_preprocess_indexed).

    store = FrameStore(256, 340, capacity=64, device=loader.device, stream=loader.stream)
    store.fetch = decode                                   # decode(video, frame_number) -> (H, W, 3) uint8 BGR
    frames_list = [(store, video, seq) for video, seq in clips]

Stream contract: uploads and the launches that read the store are on ONE stream (the loader's), so a slot is overwritten
only behind every launch that read its previous frame and eviction needs no event.  The pinned staging is a ring of
buffers, each rewritten only after the event behind its last host-to-device copy (the rule of the loader's own slots).
Frames the minibatch being filled refers to are not evictable until `release` (the loader calls it once the launch is
enqueued); a minibatch of more distinct frames than `capacity` raises and never overwrites.
"""
import collections

import numpy as np
import torch

from vlfb import hip


class StoreIndex(object):
    """which (video, frame number) lives in which of `capacity` slots: plain bookkeeping, no device.  FIFO: the frame
    resident longest goes first (a hit does not renew it), frames of the open minibatch never."""

    def __init__(self, capacity):
        self.capacity = int(capacity)
        assert self.capacity >= 1
        self.slot_of = collections.OrderedDict()       # (video, frame number) -> slot, in order of arrival
        self.free = list(range(self.capacity - 1, -1, -1))
        self.open = set()                              # keys the minibatch being filled refers to
        self.fetched = 0                               # frames that had to be fetched and uploaded
        self.requested = 0                             # frames asked for

    def assign(self, video, frame_numbers):
        """-> (slot of every requested frame, [(frame number, slot)] of those that must be uploaded, in request order).
        A request the store cannot hold is refused whole: VlfbError, and the bookkeeping is what it was before the call."""
        self._before = (self.slot_of.copy(), list(self.free), set(self.open), self.fetched, self.requested)
        slots, missing = [], []
        try:
            for f in frame_numbers:
                key = (video, int(f))
                slot = self.slot_of.get(key)
                if slot is None:
                    slot = self._take()
                    self.slot_of[key] = slot
                    missing.append((int(f), slot))
                self.open.add(key)
                slots.append(slot)
        except hip.VlfbError:
            self.undo()
            raise
        self.requested += len(slots)
        self.fetched += len(missing)
        return slots, missing

    def undo(self):
        """take the last `assign` back (it was refused, or a frame it asked for could not be fetched) before anything was
        uploaded: what it evicted is resident again -- the device still holds those bytes --, what it opened is not open,
        and nothing of it is counted"""
        self.slot_of, self.free, self.open, self.fetched, self.requested = self._before
        self._before = None

    def _take(self):
        if self.free:
            return self.free.pop()
        for key in self.slot_of:                       # oldest first
            if key not in self.open:
                return self.slot_of.pop(key)
        raise hip.VlfbError("frame store: the minibatch refers to more than the %d frames the store holds" % self.capacity)

    def release(self):
        """the launch that reads the open minibatch's frames has been enqueued: they may be evicted again"""
        self.open.clear()

    def resident(self):
        return list(self.slot_of)


class FrameStore(object):
    def __init__(self, height, width, capacity, device, stream, staging_buffers=2):
        """a ring of `capacity` uint8 BGR frames (height, width, 3) on `device`; `stream` is the stream of the loader
        whose launches read it"""
        self.height, self.width, self.capacity = int(height), int(width), int(capacity)
        self.device, self.stream = torch.device(device), stream
        self.fetch = None                              # the default `fetch` of `slots`: set it before clips name this store
        self.index = StoreIndex(capacity)
        self.frames = torch.zeros(self.capacity, self.height, self.width, 3, dtype=torch.uint8, device=self.device)
        self.staging = []
        for _ in range(int(staging_buffers)):
            pin = torch.empty(self.capacity, self.height, self.width, 3, dtype=torch.uint8).pin_memory()
            self.staging.append(dict(pin=pin, np=pin.numpy(), done=torch.cuda.Event(), used=0, in_flight=False))
        self._cur = 0

    fetched = property(lambda self: self.index.fetched)
    requested = property(lambda self: self.index.requested)
    frame_bytes = property(lambda self: self.height * self.width * 3)

    def data_ptr(self):
        return self.frames.data_ptr()

    def _staging_for(self, n):
        st = self.staging[self._cur]
        if st["used"] + n > self.capacity:
            self._cur = (self._cur + 1) % len(self.staging)
            st = self.staging[self._cur]
            if st["in_flight"]:
                st["done"].synchronize()               # the only host wait: this buffer's own last copy
            st["used"], st["in_flight"] = 0, False
        return st

    def slots(self, video, frame_numbers, fetch=None):
        """the slot of every frame of `frame_numbers` of `video`; `fetch(video, frame_number)` (default: self.fetch) is
        called for the frames that are not resident, and those are uploaded on the store's stream (runs of adjacent slots
        in one copy)"""
        fetch = fetch if fetch is not None else self.fetch
        slots, missing = self.index.assign(video, frame_numbers)
        if missing:
            st = self._staging_for(len(missing))
            base = st["used"]
            try:
                for k, (f, _) in enumerate(missing):
                    a = np.asarray(fetch(video, f))
                    assert a.dtype == np.uint8 and a.shape == (self.height, self.width, 3), \
                        "fetch must return (%d, %d, 3) uint8" % (self.height, self.width)
                    np.copyto(st["np"][base + k], a)
            except BaseException:
                self.index.undo()                      # nothing was uploaded yet: the store is what it was
                raise
            with torch.cuda.stream(self.stream):
                k = 0
                while k < len(missing):
                    run = 1
                    while k + run < len(missing) and missing[k + run][1] == missing[k][1] + run:
                        run += 1
                    s0 = missing[k][1]
                    self.frames[s0:s0 + run].copy_(st["pin"][base + k:base + k + run], non_blocking=True)
                    k += run
                st["done"].record(self.stream)
            st["used"], st["in_flight"] = base + len(missing), True
        return slots

    def release(self):
        self.index.release()
