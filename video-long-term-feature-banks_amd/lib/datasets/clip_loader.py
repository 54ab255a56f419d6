"""The next minibatch is assembled while the current one trains.

Counterpart of the reference's lib/datasets/dataloader.py and the *_data_input.py assemblers: those run a pool of worker
processes per GPU that preprocess one clip each on the host and push fp32 blobs through a queue.  Here the pixel work is
one launch for the whole minibatch (`vlfb_clip_batch_preprocess`, after `vlfb_clip_batch_channel_sums` when a colour plan
has a contrast op) on a stream of the loader's own, fed from pinned memory, so ONE background thread is enough and the
training thread never waits for a copy or a launch of the loader.

    loader = MinibatchLoader(engine, "_train", 1, max_src_hw=(256, 340), bank=bank)
    loader.start(source)                 # source yields (frames_list, boxes_list, labels_list, meta, rng)
    for it in range(iters):
        mb = loader.next()               # blocks until a minibatch has been SUBMITTED (not until the device is done)
        loader.deliver(mb)               # BETWEEN steps: stream-ordered copies into the engine's input blobs
        engine.train_step(lr)
    loader.stop()

Thread and stream contract
  * `submit` runs on any ONE thread at a time (the background thread after `start`); `deliver` runs on the training thread,
    between steps and never inside `train_step`: a recorded step (Engine.STEP_TRACE) must not contain it, and does not --
    the recorder only sees the recording thread, and `deliver` issues no `vlfb_*` call at all.
  * Everything is allocated in the constructor (a training thread may be recording or capturing while the loader runs);
    resize tables are the exception the first time a source size is met, so pass `src_sizes` to build them up front.
  * One HIP stream, the process's fourth after the engine's main, side and solver streams.
  * A slot's pinned staging and item array are rewritten only after the event behind its last host-to-device copy has
    completed (`submit` waits for it on the host); its device buffers only after the loader stream has waited for the event
    `deliver` recorded behind the copies into the engine.  `submit` RAISES when every slot is submitted and not yet
    delivered: it never overwrites a minibatch nobody has consumed.

Below `submit` nothing knows AVA: the kernels and the slot machinery (`ClipSlots`) take clips, rows and a bank query.
`FrameLoader` is the same machinery for the frame-level datasets (Charades, EPIC-Kitchens), whose engines take data /
labels (/ lfb) and no proposals:

    loader = FrameLoader(engine, "_train", 1, max_src_hw=(256, 340), bank=bank, bank_kind="charades")
    loader.start(source)                 # source yields (frames_list, labels_list, meta, rng[, spatial_shift_pos])

Both loaders also take a clip as `(store, video, frame_numbers)` -- a frame list into a datasets.frame_store.FrameStore
built on the loader's stream -- instead of stacked frames: only the frames that are not resident in the store are fetched
and uploaded, and the kernels read the clip through a table of store slots (vlfb_clip_batch_*_indexed).
"""
import ctypes as C
import queue
import threading

import numpy as np
import torch

from core.config import config as cfg
from datasets import charades
from datasets import data_input_helper as dh
from datasets.frame_store import FrameStore
from vlfb import hip


class Slot(object):
    """the buffers of one minibatch in flight: device buffers in the layout of the engine's input blobs and their staging"""

    def __init__(self, index):
        self.index = index
        self.state = "free"            # free -> filling -> submitted -> free (deliver)
        self.serial = 0                # counts the minibatches the slot has held
        self.used_h2d = False
        self.used_consumed = False
        self.keep = None               # device frames of the caller, alive until the slot is submitted again
        self.stores = []               # frame stores the minibatch being filled reads


class Minibatch(object):
    """what `submit` returns: the slot that holds the minibatch on the device, and what the host keeps of it -- `boxes` per
    clip as transformed, `proposals` (rows, 5) / `labels` (rows, classes) as uploaded (padded to the plan; `used` rows are
    real), `original_boxes` (used, 5) and `metadata` (used, 4) = [video, sec, height, width] as ava_data_input.py:180-189
    builds them for the AVA meter; `meta`, the dict that was submitted with it.  Stays valid after the slot has moved on."""

    def __init__(self, slot):
        self.slot, self.index, self.serial = slot, slot.index, slot.serial


class ClipSlots(object):
    """what the loaders share: the slots with the clip staging of a minibatch, the stream, `submit`'s slot bookkeeping,
    the preprocess launches, `deliver` and the background thread.  A subclass's constructor calls `_init_clips`, gives
    every slot its other buffers and its `pairs`, and implements `_fill(slot, *what submit was given)`."""

    def _init_clips(self, engine, suffix, split, n_slots, max_src_hw, device, src_sizes):
        hip.lib()
        self.engine, self.split = engine, split
        self.device = torch.device(device if device is not None else engine.device)
        data, (self.w_pad, self.c_pad) = engine.blob_padded("data" + suffix)
        self.N, self.T, self.crop = int(data.shape[0]), int(data.shape[1]), int(data.shape[2])
        assert int(data.shape[3]) == self.crop + 2 * self.w_pad, "the loader crops squares"
        self.dst = {"data": engine.input_tensor("data" + suffix)[:data.numel()]}
        self.code = hip.dtype_code(data.dtype)
        dev = self.device
        self.frame_bytes = self.N * self.T * int(max_src_hw[0]) * int(max_src_hw[1]) * 3
        self.clip_elems = self.T * self.crop * (self.crop + 2 * self.w_pad) * self.c_pad
        self.slots = []
        for i in range(int(n_slots)):
            s = Slot(i)
            s.pin_frames = torch.empty(self.frame_bytes, dtype=torch.uint8).pin_memory()
            s.pin_frames_np = s.pin_frames.numpy()
            s.dev_frames = torch.empty(self.frame_bytes, dtype=torch.uint8, device=dev)
            s.pin_items = torch.zeros(self.N * hip.CLIP_ITEM_BYTES, dtype=torch.uint8).pin_memory()
            s.items = (hip.ClipItem * self.N).from_buffer(s.pin_items.numpy())
            s.dev_items = torch.zeros(self.N * hip.CLIP_ITEM_BYTES, dtype=torch.uint8, device=dev)
            s.pin_index = torch.zeros(self.N * self.T, dtype=torch.int32).pin_memory()     # store slots of (store, video, frames) clips
            s.dev_index = torch.zeros(self.N * self.T, dtype=torch.int32, device=dev)
            s.store_frames = np.zeros(self.N, dtype=np.int32)
            s.clip = torch.zeros(self.N * self.clip_elems, dtype=data.dtype, device=dev)  # padding is zero and stays zero
            s.sums = torch.zeros(self.N * self.T * hip.CLIP_SUM_BANDS * 3, dtype=torch.int64, device=dev)
            s.pairs = [("data", s.clip)]
            s.h2d_done = torch.cuda.Event()
            s.ready = torch.cuda.Event()
            s.consumed = torch.cuda.Event()
            self.slots.append(s)
        self.stream = torch.cuda.Stream(device=dev)
        self._ordered = False          # the stream has not yet been put behind the fills that zeroed the slots' buffers
        self._next_slot = 0
        self._lock = threading.Lock()
        self._thread = None
        dh.warm_tables(src_sizes, split, dev)

    # ---- one minibatch ---------------------------------------------------------------------------
    def _submit(self, *args):
        with self._lock:
            s = self.slots[self._next_slot]
            if s.state != "free":
                raise hip.VlfbError("clip loader: slot %d was submitted and not delivered (%d slots)" % (s.index, len(self.slots)))
            s.state = "filling"
            self._next_slot = (self._next_slot + 1) % len(self.slots)
        try:
            if not self._ordered:
                # the slots' device buffers (this class's and the subclass's) were zeroed by fills on the device's default
                # stream, which this stream does not follow by itself: a fill that runs late would wipe the first minibatch
                self.stream.wait_stream(torch.cuda.default_stream(self.device))
                self._ordered = True
            s.serial += 1
            s.stores = []
            if s.used_h2d:
                s.h2d_done.synchronize()               # the pinned staging, the item array and the index table are free again
            mb = self._fill(s, *args)
        except BaseException:
            for store in s.stores:                     # an abandoned minibatch holds no frame in a store
                store.release()
            s.state = "free"
            raise
        s.state = "submitted"
        return mb

    def _stage(self, s, frames_list):
        """the clips' frames into the slot's pinned staging (or, for clips given as (store, video, frame_numbers), their
        store slots into its index table; the store uploads what it misses on this loader's stream).
        -> (sizes, device addresses, bytes staged, stores): `stores` is empty unless the clips are frame lists."""
        T = self.T
        forms = [isinstance(f, tuple) and len(f) == 3 and isinstance(f[0], FrameStore) for f in frames_list]
        if any(forms) and not all(forms):
            raise hip.VlfbError("clip loader: a minibatch is either stacked clips or (store, video, frame_numbers) clips")
        sizes, ptrs, keep, used, stores, staged = [], [], [], 0, [], {}
        s.keep, s.stores = keep, stores
        index = s.pin_index.numpy().reshape(self.N, T)
        for i, f in enumerate(frames_list):            # the frame-list clips of one store: ONE slots_many, so one upload and
            if forms[i]:                               # one decode call per store and minibatch
                store, video, numbers = f
                assert store.stream is self.stream and store.device == self.device, \
                    "the frame store must be built on this loader's stream and device"
                assert len(numbers) == T, "clips of %d frames" % T
                if not any(store is x for x in stores):
                    stores.append(store)
        for store in list(stores):
            mine = [i for i, f in enumerate(frames_list) if forms[i] and f[0] is store]
            for i, slots in zip(mine, store.slots_many([(frames_list[i][1], frames_list[i][2]) for i in mine])):
                index[i] = slots
        for i, f in enumerate(frames_list):
            if forms[i]:
                store = f[0]
                s.store_frames[i] = store.capacity
                sizes.append((store.height, store.width))
                ptrs.append(store.data_ptr())
                continue
            if torch.is_tensor(f) and f.is_cuda:
                assert f.dtype == torch.uint8 and f.dim() == 4 and f.shape[3] == 3 and f.is_contiguous()
                assert int(f.shape[0]) == T, "clips of %d frames" % T
                sizes.append((int(f.shape[1]), int(f.shape[2])))
                ptrs.append(f.data_ptr())
                keep.append(f)
                continue
            if id(f) in staged:                        # the same array for several clips (the shifts of a test segment): once
                size, ptr = staged[id(f)]
                sizes.append(size)
                ptrs.append(ptr)
                continue
            a = f.numpy() if torch.is_tensor(f) else (f if isinstance(f, np.ndarray) else np.stack(list(f)))
            assert a.dtype == np.uint8 and a.ndim == 4 and a.shape[3] == 3, "frames must be (T, H, W, 3) uint8"
            assert a.shape[0] == T, "clips of %d frames" % T
            nbytes = a.size
            if used + nbytes > self.frame_bytes:
                raise hip.VlfbError("clip loader: the frames of this minibatch exceed max_src_hw")
            np.copyto(s.pin_frames_np[used:used + nbytes].reshape(a.shape), a)
            sizes.append((int(a.shape[1]), int(a.shape[2])))
            ptrs.append(s.dev_frames.data_ptr() + used)
            if isinstance(f, np.ndarray):
                staged[id(f)] = (sizes[-1], ptrs[-1])
            used += nbytes
        return sizes, ptrs, used, stores

    def _pack(self, s, plans, colors, sizes, ptrs):
        es = s.clip.element_size()
        return dh.pack_items(s.items, plans, colors, [self.T] * self.N, sizes, self.crop, ptrs,
                             [s.clip.data_ptr() + i * self.clip_elems * es for i in range(self.N)],
                             [s.sums.data_ptr() + i * self.T * hip.CLIP_SUM_BANDS * 3 * 8 for i in range(self.N)],
                             self.w_pad, self.c_pad, self.device)

    def _enqueue_clips(self, s, need_sums, used, stores):
        """on the loader stream: the slot's frames, items (and index table) to the device, then the one or two launches"""
        N = self.N
        if s.used_consumed:
            self.stream.wait_event(s.consumed)          # the engine has copied the slot's previous minibatch out
        if used:
            s.dev_frames[:used].copy_(s.pin_frames[:used], non_blocking=True)
        s.dev_items.copy_(s.pin_items, non_blocking=True)
        items = C.cast(s.items, C.c_void_p)
        if stores:
            s.dev_index.copy_(s.pin_index, non_blocking=True)
            table = (s.pin_index.data_ptr(), hip.ptr(s.dev_index), self.T, s.store_frames.ctypes.data)
            if need_sums:
                hip.call("vlfb_clip_batch_channel_sums_indexed", items, hip.ptr(s.dev_items), N, *table)
            hip.call("vlfb_clip_batch_preprocess_indexed", items, hip.ptr(s.dev_items), N, *(table + (self.code,)))
            for store in stores:
                store.release()                         # enqueued: the store may evict these frames for the next minibatch
        else:
            if need_sums:
                hip.call("vlfb_clip_batch_channel_sums", items, hip.ptr(s.dev_items), N)
            hip.call("vlfb_clip_batch_preprocess", items, hip.ptr(s.dev_items), N, self.code)

    def deliver(self, minibatch):
        """on the CURRENT stream of the calling (training) thread, between steps: wait for the minibatch, copy it
        device-to-device into the engine's input blobs, and hand its slot back.  No host synchronisation."""
        slot = minibatch.slot
        if slot.state != "submitted" or slot.serial != minibatch.serial:
            raise hip.VlfbError("clip loader: slot %d holds no submitted minibatch of this handle" % slot.index)
        cur = torch.cuda.current_stream()
        cur.wait_event(slot.ready)
        for name, src in slot.pairs:
            self.dst[name].copy_(src, non_blocking=True)
        slot.consumed.record(cur)
        slot.used_consumed = True
        slot.state = "free"
        if self._thread is not None:
            self._free.release()

    # ---- the background thread -------------------------------------------------------------------
    def start(self, source):
        """run `submit` over `source` -- an iterator of the argument tuples of `submit` -- in one background thread, at
        most n_slots minibatches ahead of `deliver`"""
        assert self._thread is None, "the loader is already running"
        self._free = threading.Semaphore(len(self.slots))
        self._out = queue.Queue()
        self._stop = False
        self._thread = threading.Thread(target=self._run, args=(iter(source),), name="vlfb-clip-loader", daemon=True)
        self._thread.start()

    def _run(self, source):
        try:
            torch.cuda.set_device(self.device)
            while True:
                self._free.acquire()
                if self._stop:
                    return
                try:
                    args = next(source)
                except StopIteration:
                    self._out.put(("end", None))
                    return
                self._out.put(("slot", self.submit(*args)))
        except BaseException as e:                      # re-raised in next()
            self._out.put(("error", e))

    def next(self):
        """the next submitted Minibatch, in submission order; raises what the thread raised, StopIteration at the end of the source"""
        assert self._thread is not None, "start() first"
        kind, val = self._out.get()
        if kind == "slot":
            return val
        self._out.put((kind, val))                      # (sticky: every later call ends the same way)
        if kind == "error":
            raise val
        raise StopIteration

    def stop(self):
        """end the background thread and wait for it, and for what it enqueued on the loader stream"""
        if self._thread is None:
            return
        self._stop = True
        self._free.release()
        self._thread.join()
        self._thread = None
        self.stream.synchronize()
        for s in self.slots:
            s.state = "free"
        self._next_slot = 0


class MinibatchLoader(ClipSlots):
    def __init__(self, engine, suffix, split, n_slots=2, max_src_hw=(256, 340), bank=None, device=None, src_sizes=(),
                 bank_window=None, bank_max_per_step=None, bank_seed=None):
        """engine: a planned Engine whose inputs are data / labels / proposals (/ lfb with `bank`) + suffix; split 1 is
        train.  max_src_hw bounds height * width of a source frame (the staging holds N * T such frames)."""
        self._init_clips(engine, suffix, split, n_slots, max_src_hw, device, src_sizes)
        self.bank = bank
        self.dst["proposals"] = engine.input_tensor("proposals" + suffix)
        self.dst["labels"] = engine.input_tensor("labels" + suffix)
        self.rows = self.dst["proposals"].numel() // 5
        self.num_classes = self.dst["labels"].numel() // self.rows
        if bank is not None:
            self.dst["lfb"] = engine.input_tensor("lfb" + suffix)
            self.bank_window = int(bank_window if bank_window is not None else cfg.LFB.WINDOW_SIZE)
            self.bank_max = int(bank_max_per_step if bank_max_per_step is not None else cfg.AVA.LFB_MAX_NUM_FEAT_PER_STEP)
            self.bank_seed = int(bank_seed if bank_seed is not None else cfg.RNG_SEED)
            assert self.dst["lfb"].numel() == self.rows * self.bank_window * self.bank_max * bank.dim, "lfb blob and bank window differ"
        dev = self.device
        for s in self.slots:
            s.pin_props = torch.zeros(self.rows * 5, dtype=torch.float32).pin_memory()
            s.pin_labels = torch.zeros(self.rows * self.num_classes, dtype=torch.int32).pin_memory()
            s.dev_props = torch.zeros(self.rows * 5, dtype=torch.float32, device=dev)
            s.dev_labels = torch.zeros(self.rows * self.num_classes, dtype=torch.int32, device=dev)
            s.pairs += [("proposals", s.dev_props), ("labels", s.dev_labels)]
            if bank is not None:
                s.pin_query = torch.zeros(self.rows * 3, dtype=torch.int32).pin_memory()
                s.dev_query = torch.zeros(self.rows * 3, dtype=torch.int32, device=dev)
                s.lfb = torch.zeros_like(self.dst["lfb"])
                s.pairs.append(("lfb", s.lfb))

    def submit(self, frames_list, boxes_list, labels_list, meta, rng=np.random, spatial_shift_pos=1):
        """frames_list: per clip (T, H, W, 3) uint8 BGR frames (NumPy array, list of frames, or a device tensor, which skips
        the staging copy and must stay untouched until the slot is delivered); boxes_list: per clip (k, 4+) normalised boxes;
        labels_list: per clip (k, classes) int32; meta: dict(iteration=..., videos=[per clip], secs=[per clip]) -- the bank
        draw of clip n is named iteration * N + n.  Returns a Minibatch without waiting for the device.  Raises VlfbError when
        the slot in turn has not been delivered."""
        n = len(frames_list)
        assert n == self.N and len(boxes_list) == n and len(labels_list) == n, "a minibatch is %d clips" % self.N
        return self._submit(frames_list, boxes_list, labels_list, meta, rng, spatial_shift_pos)

    def _fill(self, s, frames_list, boxes_list, labels_list, meta, rng, spatial_shift_pos):
        N = self.N
        sizes, ptrs, used, stores = self._stage(s, frames_list)
        norm = [None if b is None or len(b) == 0 else np.asarray(b, dtype=np.float64)[:, :4] for b in boxes_list]
        plans, colors, boxes = dh.plan_minibatch(sizes, self.split, self.crop, spatial_shift_pos, norm, rng)
        need_sums = self._pack(s, plans, colors, sizes, ptrs)
        props, labels, rows = dh.minibatch_rows(boxes, labels_list, self.rows, self.num_classes)
        s.pin_props.numpy()[:] = props.reshape(-1)
        s.pin_labels.numpy()[:] = labels.reshape(-1)
        clip_of = props[:rows, 0].astype(np.int64)
        videos, secs = np.asarray(meta["videos"]), np.asarray(meta["secs"])
        if self.bank is not None and rows:
            q = self.bank.window_query(videos[clip_of], secs[clip_of], int(meta["iteration"]) * N + clip_of)
            s.pin_query.numpy()[:3 * rows] = q.reshape(-1)
        # what the host keeps (ava_data_input.py:172-204)
        mb = Minibatch(s)
        mb.meta = meta
        mb.boxes, mb.proposals, mb.labels, mb.used = boxes, props, labels, rows
        mb.original_boxes = np.concatenate(
            [np.concatenate([np.full((len(b), 1), i, dtype=np.float64), b], axis=1) for i, b in enumerate(norm) if b is not None]
            + [np.zeros((0, 5))]).astype(np.float32)
        mb.metadata = np.array([[videos[c], secs[c], sizes[c][0], sizes[c][1]] for c in clip_of], dtype=np.float32).reshape(rows, 4)

        with torch.cuda.stream(self.stream):
            self._enqueue_clips(s, need_sums, used, stores)
            s.dev_props.copy_(s.pin_props, non_blocking=True)
            s.dev_labels.copy_(s.pin_labels, non_blocking=True)
            if self.bank is not None:
                per_row = self.bank_window * self.bank_max * self.bank.dim
                if rows < self.rows:
                    s.lfb[rows * per_row:].zero_()           # padding rows: an empty bank window
                if rows:
                    s.dev_query.copy_(s.pin_query, non_blocking=True)
            s.h2d_done.record(self.stream)                   # behind the last copy out of the slot's pinned memory
            if self.bank is not None and rows:
                self.bank.sample_window_enqueue(s.dev_query, rows, self.bank_window, self.bank_max, self.bank_seed, s.lfb)
            s.ready.record(self.stream)
        s.used_h2d = True
        return mb


BANK_KINDS = ("charades", "epic_verb", "epic_noun")


class FrameLoader(ClipSlots):
    """The loader of the frame-level datasets: engines whose inputs are data / labels (/ lfb with `bank`) + suffix and no
    proposals.  Counterpart of charades_data_input.py / epic_data_input.py; the clips' frame numbers, labels and shifts
    come from datasets.charades.CharadesIndex / datasets.epic.EpicIndex.  Thread and stream contract: the module's."""

    def __init__(self, engine, suffix, split, n_slots=2, max_src_hw=(256, 340), bank=None, bank_kind=None, device=None,
                 src_sizes=(), bank_window=None):
        """split 1 is train.  With `bank` (a DeviceBank), bank_kind in BANK_KINDS names the window that is sampled into the
        `lfb` input: Charades frames (CHARADES.LFB_CLIPS_PER_SECOND), EPIC verb clips (EPIC.VERB_LFB_CLIPS_PER_SECOND) or
        EPIC noun detections (EPIC.MAX_NUM_FEATS_PER_NOUN_LFB_FRAME, EPIC.NOUN_LFB_FRAMES_PER_SECOND)."""
        self._init_clips(engine, suffix, split, n_slots, max_src_hw, device, src_sizes)
        self.bank, self.bank_kind = bank, bank_kind
        self.dst["labels"] = engine.input_tensor("labels" + suffix)
        # labels as planned: (N, classes) multi-hot rows (Charades) or (N,) class ids (EPIC)
        self.label_shape = tuple(int(d) for d in engine.env["labels" + suffix].root.shape)
        assert self.label_shape[0] == self.N and int(np.prod(self.label_shape)) == self.dst["labels"].numel()
        self.multi_hot = len(self.label_shape) == 2
        if bank is not None:
            assert bank_kind in BANK_KINDS, "bank_kind must be one of %r" % (BANK_KINDS,)
            self.dst["lfb"] = engine.input_tensor("lfb" + suffix)
            self.bank_window = int(bank_window if bank_window is not None else cfg.LFB.WINDOW_SIZE)
            assert self.dst["lfb"].numel() == self.N * self.bank_window * bank.dim, "lfb blob and bank window differ"
        dev = self.device
        for s in self.slots:
            s.pin_labels = torch.zeros(self.dst["labels"].numel(), dtype=torch.int32).pin_memory()
            s.dev_labels = torch.zeros(self.dst["labels"].numel(), dtype=torch.int32, device=dev)
            s.pairs.append(("labels", s.dev_labels))
            if bank is not None:
                s.pin_query = torch.zeros(self.N * 3, dtype=torch.int32).pin_memory()
                s.dev_query = torch.zeros(self.N * 3, dtype=torch.int32, device=dev)
                s.lfb = torch.zeros_like(self.dst["lfb"])
                s.pairs.append(("lfb", s.lfb))

    def submit(self, frames_list, labels_list, meta, rng=np.random, spatial_shift_pos=1):
        """frames_list: per clip what MinibatchLoader.submit takes, or (store, video, frame_numbers); the same array object
        for several clips (the three shifts of a test segment) is staged once.  labels_list: per clip a list of class ids
        (multi-hot labels: the row of charades.construct_label_array) or one class id (EPIC).  meta: dict(iteration=...,
        videos=[per clip, the bank's video keys], centers=[per clip, the clip's centre frame]).  spatial_shift_pos: one
        position or one per clip (ignored in train).  Returns a Minibatch without waiting for the device; raises VlfbError
        when the slot in turn has not been delivered."""
        n = len(frames_list)
        assert n == self.N and len(labels_list) == n, "a minibatch is %d clips" % self.N
        return self._submit(frames_list, labels_list, meta, rng, spatial_shift_pos)

    def _query(self, videos, centers):
        if self.bank_kind == "charades":
            return self.bank.frames_query(videos, centers, self.bank_window, cfg.CHARADES.LFB_CLIPS_PER_SECOND)
        if self.bank_kind == "epic_verb":
            return self.bank.epic_verb_query(videos, centers, self.bank_window, cfg.EPIC.VERB_LFB_CLIPS_PER_SECOND)
        return self.bank.epic_noun_query(videos, centers, self.bank_window, cfg.EPIC.MAX_NUM_FEATS_PER_NOUN_LFB_FRAME,
                                         cfg.EPIC.NOUN_LFB_FRAMES_PER_SECOND)

    def _fill(self, s, frames_list, labels_list, meta, rng, spatial_shift_pos):
        N = self.N
        sizes, ptrs, used, stores = self._stage(s, frames_list)
        plans, colors, _ = dh.plan_minibatch(sizes, self.split, self.crop, spatial_shift_pos, None, rng)
        need_sums = self._pack(s, plans, colors, sizes, ptrs)
        if self.multi_hot:
            labels = np.stack([charades.construct_label_array(l, self.label_shape[1]) for l in labels_list])
        else:
            labels = np.asarray(labels_list, dtype=np.int32).reshape(N)
        s.pin_labels.numpy()[:] = labels.reshape(-1)
        videos, centers = list(meta["videos"]), [int(c) for c in meta["centers"]]
        assert len(videos) == N and len(centers) == N, "meta names a video and a centre per clip"
        if self.bank is not None:
            s.pin_query.numpy()[:] = self._query(videos, centers).reshape(-1)
        mb = Minibatch(s)
        mb.meta = meta
        mb.labels, mb.videos, mb.centers, mb.iteration = labels, videos, centers, meta.get("iteration")

        with torch.cuda.stream(self.stream):
            self._enqueue_clips(s, need_sums, used, stores)
            s.dev_labels.copy_(s.pin_labels, non_blocking=True)
            if self.bank is not None:
                s.dev_query.copy_(s.pin_query, non_blocking=True)
            s.h2d_done.record(self.stream)                   # behind the last copy out of the slot's pinned memory
            if self.bank is not None:
                if self.bank_kind == "charades":
                    self.bank.sample_compact_enqueue(s.dev_query, N, self.bank_window, s.lfb)
                else:
                    per = 1 if self.bank_kind == "epic_verb" else cfg.EPIC.MAX_NUM_FEATS_PER_NOUN_LFB_FRAME
                    self.bank.sample_packed_enqueue(s.dev_query, N, self.bank_window, per, s.lfb)
            s.ready.record(self.stream)
        s.used_h2d = True
        return mb
