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

Compressed frames: with `store.fetch_jpeg = read` (read(video, frame_number) -> the bytes of a baseline JPEG file) the
store parses each missing file on the host (datasets.jpeg), uploads the scan bytes and one record per frame in ONE copy and
decodes them on its stream into their slots (vlfb_jpeg_decode_batch_par: bit for bit what cv2.imread returns); `slots_many`
does this once for all the clips of a minibatch.  A file the
decoder does not take (datasets.jpeg.JpegUnsupported: progressive, CMYK, ...) goes through `fetch` when that is set as
well; a file of another size than the store's is refused like a failing `fetch`.  What the device finds in a damaged
stream comes back through `check_decoded()`, to be called where the caller synchronises anyway.

Stream contract: uploads and the launches that read the store are on ONE stream (the loader's), so a slot is overwritten
only behind every launch that read its previous frame and eviction needs no event.  The pinned staging is a ring of
buffers, each rewritten only after the event behind its last host-to-device copy (the rule of the loader's own slots).
Frames the minibatch being filled refers to are not evictable until `release` (the loader calls it once the launch is
enqueued); a minibatch of more distinct frames than `capacity` raises and never overwrites.
"""
import collections
import ctypes as C
import threading

import numpy as np
import torch

from datasets import jpeg
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
        return self.assign_many([(video, frame_numbers)])[0]

    def assign_many(self, requests):
        """`assign` for the requests [(video, frame_numbers), ...] of one minibatch -> [(slots, missing)] per request; a
        frame several requests name is missing in the first of them only.  ONE snapshot, taken before the first request:
        a refusal of any request, and `undo`, take all of them back."""
        self._before = (self.slot_of.copy(), list(self.free), set(self.open), self.fetched, self.requested)
        out = []
        try:
            for video, frame_numbers in requests:
                slots, missing = [], []
                for f in frame_numbers:
                    key = (video, int(f))
                    slot = self.slot_of.get(key)
                    if slot is None:
                        slot = self._take()
                        self.slot_of[key] = slot
                        missing.append((int(f), slot))
                    self.open.add(key)
                    slots.append(slot)
                self.requested += len(slots)
                self.fetched += len(missing)
                out.append((slots, missing))
        except hip.VlfbError:
            self.undo()
            raise
        return out

    def undo(self):
        """take the last `assign` / `assign_many` back (it was refused, or a frame it asked for could not be fetched) before
        anything was uploaded: what it evicted is resident again -- the device still holds those bytes --, what it opened
        is not open, and nothing of it is counted"""
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
    def __init__(self, height, width, capacity, device, stream, staging_buffers=2, jpeg_subseq_bytes=None):
        """a ring of `capacity` uint8 BGR frames (height, width, 3) on `device`; `stream` is the stream of the loader
        whose launches read it.  jpeg_subseq_bytes: the subsequence size of the lane-parallel JPEG decode
        (vlfb_jpeg_decode_batch_par; None: the library's default), -1: the serial vlfb_jpeg_decode_batch"""
        self.height, self.width, self.capacity = int(height), int(width), int(capacity)
        self.device, self.stream = torch.device(device), stream
        self.fetch = None                              # the default `fetch` of `slots`: set it before clips name this store
        self.fetch_jpeg = None                         # f(video, frame_number) -> JPEG bytes, decoded on the device
        self._jpeg = None                              # rings, workspace and status log of the JPEG path: on its first use
        self._jpeg_staging_buffers = int(staging_buffers)
        self.jpeg_subseq_bytes = None if jpeg_subseq_bytes is None else int(jpeg_subseq_bytes)
        self.uploaded_bytes = 0                        # bytes copied host-to-device so far, either way
        self.decode_calls = 0                          # JPEG decode calls enqueued so far: one per minibatch that missed a file
        self.decoded_frames = 0                        # frames they decoded
        self.index = StoreIndex(capacity)
        self.frames = torch.zeros(self.capacity, self.height, self.width, 3, dtype=torch.uint8, device=self.device)
        # the fill runs on the constructing thread's current stream, which `stream` does not follow by itself: without this
        # edge a fill that runs late (a backlog of parameter uploads in front of it) wipes the first frames uploaded
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
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

    # ---- compressed frames ------------------------------------------------------------------------
    JPEG_STATUS_LOG = 1 << 16                          # status words kept between two check_decoded()

    def _jpeg_state(self):
        """allocated once: a ring of pinned byte buffers (records, segment tables, scan bytes; a buffer is rewritten only
        behind the event of its last copy) with one device buffer they are copied to, the coefficient workspace of
        `capacity` frames of this size at the densest sampling, and the status log"""
        if self._jpeg is None:
            j = self._jpeg = dict(lock=threading.Lock(), pending=[], logged=0, cur=0, bufs=[])
            # per frame: its record, and a file never larger than the decoded frame plus its tables
            j["bytes"] = self.capacity * (hip.JPEG_ITEM_BYTES + self.frame_bytes + 4096)
            for _ in range(self._jpeg_staging_buffers):
                pin = torch.zeros(j["bytes"], dtype=torch.uint8).pin_memory()
                j["bufs"].append(dict(pin=pin, np=pin.numpy(), done=torch.cuda.Event(), used=0, in_flight=False))
            j["dev"] = torch.zeros(j["bytes"], dtype=torch.uint8, device=self.device)
            blocks = 3 * (2 * -(-self.height // 16)) * (2 * -(-self.width // 16))
            j["workspace"] = torch.zeros(self.capacity * 192 * blocks, dtype=torch.uint8, device=self.device)
            j["status"] = torch.zeros(self.JPEG_STATUS_LOG, dtype=torch.int32, device=self.device)
            self.stream.wait_stream(torch.cuda.current_stream(self.device))      # behind these fills, as for `frames`
        return self._jpeg

    def _jpeg_buffer_for(self, nbytes):
        j = self._jpeg
        if nbytes > j["bytes"]:
            raise hip.VlfbError("frame store: %d bytes of compressed frames do not fit the %d-byte ring buffer" % (nbytes, j["bytes"]))
        st = j["bufs"][j["cur"]]
        if st["used"] + nbytes > j["bytes"]:
            j["cur"] = (j["cur"] + 1) % len(j["bufs"])
            st = j["bufs"][j["cur"]]
            if st["in_flight"]:
                st["done"].synchronize()               # the only host wait: this buffer's own last copy
            st["used"], st["in_flight"] = 0, False
        return st

    def _stage_jpeg(self, parsed):
        """records, segment tables and scan bytes of `parsed` [(video, frame number, slot, file bytes, JpegInfo)] into the ring;
        -> (buffer, first byte, bytes, item array) of the chunk to upload"""
        j, n = self._jpeg, len(parsed)
        if j["logged"] + n > self.JPEG_STATUS_LOG:
            self.check_decoded()                       # the log is full: one wait per JPEG_STATUS_LOG decoded frames
        rec = -(-n * hip.JPEG_ITEM_BYTES // 16) * 16
        seg_at, scan_at, at = [], [], rec
        for _, _, _, _, info in parsed:
            seg_at.append(at)
            at += -(-4 * len(info.segment_offsets) // 16) * 16
        for _, _, _, _, info in parsed:
            scan_at.append(at)
            at += -(-max(info.scan_bytes, 1) // 16) * 16
        st = self._jpeg_buffer_for(at)
        base = st["used"]
        dev = j["dev"].data_ptr() + base
        items = (hip.JpegItem * n).from_buffer(st["np"], base)
        ws = 0
        for k, (_, _, slot, data, info) in enumerate(parsed):
            it = info.fill(items[k])
            it.scan, it.seg_offsets = dev + scan_at[k], dev + seg_at[k]
            it.dst = self.frames.data_ptr() + slot * self.frame_bytes
            it.ws_offset = ws
            ws += info.workspace_bytes
            seg = np.asarray(info.segment_offsets, dtype=np.uint32)
            st["np"][base + seg_at[k]:base + seg_at[k] + 4 * seg.size] = seg.view(np.uint8)
            st["np"][base + scan_at[k]:base + scan_at[k] + info.scan_bytes] = \
                np.frombuffer(data, dtype=np.uint8)[info.scan_start:info.scan_end]
        return st, base, at, items

    def check_decoded(self):
        """the status words of the frames decoded since the last check, read behind the store's stream (it waits for it:
        call it where the caller synchronises anyway); VlfbError naming every (video, frame number) the device could not
        decode.  Those slots hold what the damaged stream gave, zeros from where it stopped."""
        j = self._jpeg
        if j is None:
            return
        with j["lock"]:
            pending, logged = j["pending"], j["logged"]
            j["pending"], j["logged"] = [], 0
        if not logged:
            return
        with torch.cuda.stream(self.stream):
            status = j["status"][:logged].cpu().numpy()
        names = {hip.JPEG_TRUNCATED: "truncated", hip.JPEG_BAD_CODE: "bad code", hip.JPEG_BAD_RESTART: "bad restart marker"}
        bad = []
        for first, keys in pending:
            for k, key in enumerate(keys):
                word = int(status[first + k])
                if word:
                    bad.append("%r (%s)" % (key, ", ".join(t for bit, t in sorted(names.items()) if word & bit) or word))
        if bad:
            raise hip.VlfbError("frame store: %d frame(s) could not be decoded: %s" % (len(bad), "; ".join(bad)))

    def slots(self, video, frame_numbers, fetch=None):
        """the slot of every frame of `frame_numbers` of `video`; the frames that are not resident are fetched and uploaded
        on the store's stream: decoded by `fetch(video, frame_number)` (default: self.fetch; runs of adjacent slots in one
        copy), or, when `fetch` is not given and self.fetch_jpeg is set, as JPEG bytes decoded on the device"""
        return self.slots_many([(video, frame_numbers)], fetch=fetch)[0]

    def slots_many(self, requests, fetch=None):
        """`slots` for the requests [(video, frame_numbers), ...] of one minibatch -> one slot list per request.  A frame
        several requests share is fetched once; all missing JPEG files of all requests are ONE chunk of the ring (one copy,
        one decode call), all frames that go through `fetch` one staging pass.  All or nothing: a request the store
        cannot hold, a file of another size, a failing `fetch` or an unsupported file without `fetch` raises, enqueues
        nothing and leaves the index as it was before the call."""
        as_jpeg = fetch is None and self.fetch_jpeg is not None
        fetch = fetch if fetch is not None else self.fetch
        assigned = self.index.assign_many(requests)
        missing = [(video, f, slot) for (video, _), (_, miss) in zip(requests, assigned) for f, slot in miss]
        if missing:
            parsed, chunk = [], None
            try:
                if as_jpeg:
                    self._jpeg_state()
                    decoded = []
                    for video, f, slot in missing:
                        data = self.fetch_jpeg(video, f)
                        try:
                            info = jpeg.parse(data)
                        except jpeg.JpegUnsupported:
                            if fetch is None:
                                raise
                            decoded.append((video, f, slot))  # a file the device does not take: decoded by `fetch`
                            continue
                        if (info.height, info.width) != (self.height, self.width):
                            raise hip.VlfbError("frame store: frame %r of %r is %d x %d, the store holds %d x %d"
                                                % (f, video, info.height, info.width, self.height, self.width))
                        parsed.append((video, f, slot, data, info))
                    missing = decoded
                    if parsed:
                        chunk = self._stage_jpeg(parsed)
                if missing:
                    st = self._staging_for(len(missing))
                    base = st["used"]
                    for k, (video, f, _) in enumerate(missing):
                        a = np.asarray(fetch(video, f))
                        assert a.dtype == np.uint8 and a.shape == (self.height, self.width, 3), \
                            "fetch must return (%d, %d, 3) uint8" % (self.height, self.width)
                        np.copyto(st["np"][base + k], a)
                if chunk is not None:
                    self._enqueue_jpeg(parsed, *chunk)
            except BaseException:
                self.index.undo()                      # nothing was uploaded yet: the store is what it was
                raise
            if missing:
                with torch.cuda.stream(self.stream):
                    k = 0
                    while k < len(missing):
                        run = 1
                        while k + run < len(missing) and missing[k + run][2] == missing[k][2] + run:
                            run += 1
                        s0 = missing[k][2]
                        self.frames[s0:s0 + run].copy_(st["pin"][base + k:base + k + run], non_blocking=True)
                        k += run
                    st["done"].record(self.stream)
                st["used"], st["in_flight"] = base + len(missing), True
                self.uploaded_bytes += len(missing) * self.frame_bytes
        return [slots for slots, _ in assigned]

    def _enqueue_jpeg(self, parsed, st, base, nbytes, items):
        """one copy of the chunk and one decode of its frames into their slots, on the store's stream.  A batch the entry
        point refuses is refused before it launches anything: no slot has changed."""
        j, n = self._jpeg, len(parsed)
        with j["lock"]:
            first = j["logged"]
        with torch.cuda.stream(self.stream):
            j["dev"][base:base + nbytes].copy_(st["pin"][base:base + nbytes], non_blocking=True)
            st["done"].record(self.stream)
            st["used"], st["in_flight"] = base + nbytes, True
            head = (C.cast(items, C.c_void_p), j["dev"].data_ptr() + base, n, j["workspace"].data_ptr(), j["workspace"].numel(),
                    j["status"].data_ptr() + 4 * first)
            if self.jpeg_subseq_bytes == -1:
                hip.call("vlfb_jpeg_decode_batch", *head)
            else:
                hip.call("vlfb_jpeg_decode_batch_par", *(head + (self.jpeg_subseq_bytes or 0, None)))
        with j["lock"]:
            j["pending"].append((first, [(video, f) for video, f, _, _, _ in parsed]))
            j["logged"] = first + n
        self.uploaded_bytes += nbytes
        self.decode_calls += 1
        self.decoded_frames += n

    def release(self):
        self.index.release()
