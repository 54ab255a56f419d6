"""The long-term feature bank as a device tensor.

Reference: tools/lfb_loader.py builds `{video: {sec: [feat, ...]}}` (AVA, :79-112) or
`{video: {frame: feat}}` (Charades/EPIC, :49-76) on the host from `box_pooled` / `pool5` fetched
after every inference iteration, pickles it, and the dataset classes sample a window per clip in
NumPy (lib/datasets/ava.py:300-323, charades.py:251-276) -- 2.46 MB per RoI through the blob queue
every training iteration.

Here the bank lives in HBM for the whole job (AVA train: 235 videos x 900 s x 16 slots x 2048 bf16
= 13.9 GB of the 288 GB), `box_pooled` is appended to it by a kernel without leaving the device,
and the sampled (R, K, 2048) block is written by a kernel straight into the model's `lfb` input.
`from_reference` / `to_reference` convert to and from the reference's pickled dictionaries.  Whatever leaves the bank
(`to_reference`, `save`, `merge_from`, `all_gather_ranks`) reads it through `packed_chunks`: the occupied rows only, in cell
order, one staging chunk at a time (vlfb_lfb_pack_offsets / vlfb_lfb_pack), never a dense copy.

All compute goes through libvlfb_hip.so (vlfb_lfb_*); there is no host fallback.
"""
import ctypes as C

import numpy as np
import torch

from vlfb import hip

FPS = 24   # cfg.CHARADES.FPS (lib/datasets/charades.py:43)


def frame_window_steps(center_frames, window, clips_per_second):
    """first / last bank step (inclusive) of the frame window the reference searches around each clip
    centre (charades.py:259-261: begin = round(centre - secs/2 * FPS), end = begin + secs * FPS).
    Bank step t holds frame sample_freq * (t + 1) - 1, so frames in [begin, end] <=> t in [lo, hi]."""
    sample_freq = FPS // int(clips_per_second)
    secs = int(window) // int(clips_per_second)
    c = np.asarray(center_frames, dtype=np.float64).reshape(-1)
    begin = np.round(c - (float(secs) / 2.0 * FPS)).astype(np.int64)
    end = begin + secs * FPS
    lo = -((-(begin + 1)) // sample_freq) - 1
    hi = (end + 1) // sample_freq - 1
    return lo, hi


EPIC_FPS = 30   # lib/datasets/epic.py:46 / cfg.EPIC.FPS


def _ceil_div(a, b):
    return -((-a) // b)


def epic_verb_window_steps(center_frames, window, clips_per_second=1, fps=EPIC_FPS):
    """first / last bank step of sample_verb_lfb (epic.py:310-318): frames [centre - half, centre + half] with
    half = (window * FPS) // 2.  Verb banks hold the frames f with f % sample_freq == 0
    (epic.py:286-303), bank step t = frame t * sample_freq."""
    sf = int(fps) // int(clips_per_second)
    c = np.asarray(center_frames, dtype=np.int64).reshape(-1)
    half = (int(window) * int(fps)) // 2
    lo = _ceil_div(c - half, sf)
    hi = (c + half) // sf
    return lo, hi


def epic_noun_window_steps(center_frames, window, max_per_frame=10, frames_per_second=1, fps=EPIC_FPS):
    """first / last bank step of sample_noun_lfb (epic.py:338-350): secs = window / (max_per_frame * fps_lfb),
    lower = int(centre - secs / 2 * FPS)  (Python int(): truncation toward zero), upper = int(lower + secs * FPS).
    Noun banks hold one detector frame per 1 / frames_per_second seconds: step t = frame t * (FPS // fps_lfb)."""
    sf = int(fps) // int(frames_per_second)
    secs = float(window) / (int(max_per_frame) * int(frames_per_second))
    c = np.asarray(center_frames, dtype=np.float64).reshape(-1)
    lower = np.trunc(c - (secs / 2.0) * fps).astype(np.int64)
    upper = np.trunc(lower + secs * fps).astype(np.int64)
    return _ceil_div(lower, sf), upper // sf


def reference_draw_clip(counts, video, centre, window, K, rng):
    """the slot table of ONE `sample_lfb` call (lib/datasets/ava.py:300-323): the occupied seconds of the window around
    `centre` (a bank step: keyframe second minus the bank's first second) in ascending order, one
    `rng.choice(range(num_feat), min(num_feat, K), replace=False)` each -> int32 [window][K], -1 = empty slot"""
    t = np.full((int(window), int(K)), -1, dtype=np.int32)
    lower = int(centre) - int(window) // 2
    for j in range(int(window)):
        si = lower + j
        n = int(counts[video, si]) if (0 <= video < counts.shape[0] and 0 <= si < counts.shape[1]) else 0
        if n > 0:                                    # `if si in in_video_lfb`
            used = min(n, int(K))
            t[j, :used] = rng.choice(range(n), used, replace=False)
    return t


def reference_draw_table(counts, vid, centre, clip_index, window, K, rng):
    """The slot table of `sample_lfb` (lib/datasets/ava.py:300-323) for the rows of a minibatch, drawn from `rng` in the
    reference's call order: clips in minibatch order (ava.py:205-230 appends one sampled bank per clip; rows of one clip --
    its boxes, ava_data_input.py:191-192 -- share that bank), per clip the occupied seconds of its window in ascending
    order, one `rng.choice(range(num_feat), min(num_feat, K), replace=False)` each.  counts[video][step] = features stored
    for that second (0 = `si not in in_video_lfb`); centre = keyframe second minus the bank's first second.
    -> int32 [rows][window][K], -1 = empty slot.  Pure host code (tests/test_lfb_oracle.py replays the reference loop)."""
    rows = len(vid)
    ids = np.asarray(clip_index).astype(np.int64).reshape(-1)
    if ids.size != rows or (rows and (ids[0] != 0 or np.any(np.diff(ids) < 0) or np.any(np.diff(ids) > 1))):
        raise ValueError("clip_index must be the minibatch position of every row's clip: 0, 0, 1, 1, 1, ... (got %r)" % (ids[:8],))
    table = np.full((rows, int(window), int(K)), -1, dtype=np.int32)
    prev = None
    for r in range(rows):
        if prev is None or ids[r] != ids[prev]:              # a new clip of the minibatch: its own draw
            # (even when it names the same keyframe as the clip before it: still a NEW draw, as in the reference)
            cur = reference_draw_clip(counts, vid[r], centre[r], window, K, rng)
        elif vid[r] != vid[prev] or centre[r] != centre[prev]:
            raise ValueError("rows %d and %d belong to one clip but name different keyframes" % (prev, r))
        table[r] = cur
        prev = r
    return table


class DeviceBank(object):
    """bank[video][step][slot][dim] + count[video][step] on one GPU.

    `step_base` is subtracted from the reference's time keys (AVA seconds start at 902);
    `video_ids` optionally maps the reference's video keys to dense rows."""

    def __init__(self, n_videos, n_steps, capacity, dim=2048, dtype="bf16", device="cuda:0", step_base=0,
                 video_ids=None):
        hip.lib()
        self.device = torch.device(device)
        self.code = (hip.BF16 if dtype in ("bf16", torch.bfloat16) else
                     hip.F16 if dtype in ("fp16", "f16", torch.float16) else hip.F32)
        self.desc = hip.LfbDesc(int(n_videos), int(n_steps), int(capacity), int(dim), self.code, int(step_base))
        nbytes = hip.lib().vlfb_lfb_bank_bytes(C.byref(self.desc))
        if nbytes <= 0:
            raise hip.VlfbError("lfb bank: bad geometry %r" % ((n_videos, n_steps, capacity, dim),))
        self.bank = torch.zeros(int(n_videos) * int(n_steps) * int(capacity) * int(dim), device=self.device,
                                dtype=hip.TORCH_DTYPE[self.code])
        self.count = torch.zeros(int(n_videos) * int(n_steps), device=self.device, dtype=torch.int32)
        self.dropped = torch.zeros(1, device=self.device, dtype=torch.int32)
        self.step_base = int(step_base)
        self.video_row = None if video_ids is None else {v: i for i, v in enumerate(video_ids)}
        self.video_ids = None if video_ids is None else list(video_ids)

    # ---- geometry --------------------------------------------------------------------------------
    n_videos = property(lambda self: self.desc.n_videos)
    n_steps = property(lambda self: self.desc.n_steps)
    capacity = property(lambda self: self.desc.capacity)
    dim = property(lambda self: self.desc.dim)

    def _rows_of(self, videos):
        if self.video_row is None:
            return np.asarray(videos).astype(np.int64).reshape(-1)
        if any(isinstance(x, str) for x in videos):          # names (EPIC verb banks); a negative number is a padding row
            return np.array([self.video_row.get(x, -1) if isinstance(x, str) else -1 for x in videos], dtype=np.int64)
        v = np.asarray(videos).astype(np.int64).reshape(-1)
        return np.array([self.video_row.get(int(x), -1) if x >= 0 else -1 for x in v], dtype=np.int64)

    def _dev_i32(self, arr):
        return torch.as_tensor(np.ascontiguousarray(arr, dtype=np.int32)).to(self.device)

    # ---- construction ----------------------------------------------------------------------------
    def append(self, feats, videos, steps):
        """feats: (R, dim[,1,1,1]) device tensor (fp32 / bf16) or host array; videos/steps: (R,) reference
        keys (a negative video marks a padding row)."""
        self._append_sync(feats, self.append_keys(videos, steps))

    def _append_sync(self, feats, keys):
        if not torch.is_tensor(feats):
            feats = torch.as_tensor(np.asarray(feats, dtype=np.float32))
        feats = feats.to(self.device).reshape(feats.shape[0], -1).contiguous()
        assert feats.shape[1] == self.dim, "append: feature width %d, bank dim %d" % (feats.shape[1], self.dim)
        rows = feats.shape[0]
        assert keys.shape == (rows, 2)
        self.append_enqueue(feats, self._dev_i32(keys), rows)
        torch.cuda.current_stream().synchronize()     # the keys / feats may be temporaries

    def append_keys(self, videos, steps):
        """the (rows, 2) int32 keys `append` uploads: [bank row of the video (negative: a padding row), step]"""
        return np.stack([self._rows_of(videos), np.asarray(steps).astype(np.int64).reshape(-1) - self.step_base],
                        axis=1).astype(np.int32)

    def frame_keys(self, rows, frame_keys, sample_freq):
        """`append_keys` of `append_frames`: (video, frame) pairs with (frame + 1) % sample_freq == 0 -> keys of `rows`
        rows, those beyond len(frame_keys) marked as padding"""
        fk = np.asarray(frame_keys, dtype=np.int64).reshape(-1, 2)
        vids = np.full(rows, -1, dtype=np.int64)
        steps = np.zeros(rows, dtype=np.int64)
        n = min(rows, fk.shape[0])
        assert np.all((fk[:n, 1] + 1) % sample_freq == 0), "frame keys must be LFB frames"
        vids[:n] = fk[:n, 0]
        steps[:n] = (fk[:n, 1] + 1) // sample_freq - 1
        return self.append_keys(vids, steps + self.step_base)

    def epic_frame_keys(self, rows, frame_keys, sample_freq):
        """`frame_keys` for an EPIC verb bank: (video, frame) pairs with frame % sample_freq == 0, step = frame //
        sample_freq (epic.py get_annotations_for_lfb_frames; the step rule of `from_epic`) -> keys of `rows` rows, those
        beyond len(frame_keys) marked as padding"""
        n = min(int(rows), len(frame_keys))
        vids = [k[0] for k in frame_keys[:n]] + [-1] * (int(rows) - n)
        frames = np.array([int(k[1]) for k in frame_keys[:n]], dtype=np.int64)
        assert np.all(frames % sample_freq == 0), "frame keys must be LFB frames"
        steps = np.zeros(int(rows), dtype=np.int64)
        steps[:n] = frames // sample_freq
        return self.append_keys(vids, steps + self.step_base)

    def append_enqueue(self, feats, keys_dev, rows):
        """`append` for a caller that owns every buffer (a bank-construction pass): feats a contiguous (>= rows, dim) DEVICE
        tensor (fp32 / bf16), keys_dev the `append_keys` / `frame_keys` it uploaded in stream order.  One launch on the
        current stream, nothing allocated, no synchronisation."""
        assert feats.is_cuda and feats.is_contiguous() and feats.numel() >= int(rows) * self.dim
        hip.call("vlfb_lfb_append", C.byref(self.desc), hip.ptr(self.bank), hip.ptr(self.count), hip.ptr(feats),
                 hip.dtype_code(feats.dtype), hip.ptr(keys_dev), int(rows), hip.ptr(self.dropped))

    def append_ava(self, box_pooled, metadata):
        """one inference iteration of construct_ava_lfb (lfb_loader.py:79-112): metadata rows are
        [video_id, sec, ...] as floats"""
        md = np.asarray(metadata, dtype=np.float64)
        self.append(box_pooled, np.round(md[:, 0]).astype(np.int64), np.round(md[:, 1]).astype(np.int64))

    def append_frames(self, pool5, frame_keys, sample_freq):
        """one inference iteration of construct_frame_level_lfb (lfb_loader.py:49-76): frame_keys are
        (video, frame) pairs with (frame + 1) % sample_freq == 0 (charades.py:233-248); rows of
        `pool5` beyond len(frame_keys) are padding"""
        self._append_sync(pool5, self.frame_keys(pool5.shape[0], frame_keys, sample_freq))

    def check_no_drops(self):
        n = int(self.dropped.item())
        if n:
            raise hip.VlfbError("lfb bank: %d features did not fit (capacity %d per step, or key out of range)"
                                % (n, self.capacity))

    def counts(self):
        return self.count.view(self.n_videos, self.n_steps).cpu().numpy()

    def count_nonfinite(self):
        """(bad_rows, occupied_rows): the occupied rows that hold a NaN or +-Inf element and the occupied rows examined,
        counted on the device (vlfb_lfb_count_nonfinite); 16 bytes come back.  Synchronises."""
        out = torch.zeros(2, device=self.device, dtype=torch.int64)
        hip.call("vlfb_lfb_count_nonfinite", C.byref(self.desc), hip.ptr(self.bank), hip.ptr(self.count), hip.ptr(out))
        bad, occupied = out.cpu().tolist()
        return int(bad), int(occupied)

    def check_finite(self):
        """a finished bank holds no NaN / Inf row: on the 16-bit paths an activation above the format's range turns into one
        silently, and an inference pass has no loss to notice it"""
        bad, occupied = self.count_nonfinite()
        if bad:
            raise hip.VlfbError("lfb bank: %d of %d occupied rows hold a NaN or Inf element" % (bad, occupied))

    # ---- sampling --------------------------------------------------------------------------------
    def _out(self, out, shape, dtype):
        if out is None:
            return torch.empty(shape, device=self.device, dtype=dtype or hip.TORCH_DTYPE[self.code])
        assert out.is_contiguous() and out.numel() == int(np.prod(shape)), "sample: output tensor has the wrong size"
        return out

    def sample_window(self, videos, secs, sample_ids, window, max_per_step, seed, out=None, out_dtype=None):
        """AVA (ava.py:300-323): -> (R, window*max_per_step, dim).  `sample_ids` name the random draw
        (e.g. iteration * batch + clip); RoIs of one clip pass the same id and get the same sample."""
        rows = len(videos)
        q = np.stack([self._rows_of(videos), np.asarray(secs).astype(np.int64).reshape(-1) - self.step_base,
                      np.asarray(sample_ids).astype(np.int64).reshape(-1) & 0x7FFFFFFF], axis=1)
        qd = self._dev_i32(q)
        out = self._out(out, (rows, window * max_per_step, self.dim), out_dtype)
        hip.call("vlfb_lfb_sample_window", C.byref(self.desc), hip.ptr(self.bank), hip.ptr(self.count), hip.ptr(qd),
                 rows, int(window), int(max_per_step), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), hip.ptr(out),
                 hip.dtype_code(out.dtype))
        torch.cuda.current_stream().synchronize()
        return out

    def window_query(self, videos, secs, sample_ids):
        """the (rows, 3) int32 query `sample_window` uploads: [bank row of the video, step, sample id]"""
        return np.stack([self._rows_of(videos), np.asarray(secs).astype(np.int64).reshape(-1) - self.step_base,
                         np.asarray(sample_ids).astype(np.int64).reshape(-1) & 0x7FFFFFFF], axis=1).astype(np.int32)

    def sample_window_enqueue(self, query_dev, rows, window, max_per_step, seed, out):
        """`sample_window` for a caller that owns every buffer (a `window_query` it uploaded to `query_dev` in stream order,
        the output rows): one launch on the current stream, nothing allocated, no synchronisation"""
        assert out.is_contiguous() and out.numel() >= int(rows) * int(window) * int(max_per_step) * self.dim
        hip.call("vlfb_lfb_sample_window", C.byref(self.desc), hip.ptr(self.bank), hip.ptr(self.count), hip.ptr(query_dev),
                 int(rows), int(window), int(max_per_step), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), hip.ptr(out),
                 hip.dtype_code(out.dtype))

    def sample_window_reference_draw(self, videos, secs, clip_index, window, max_per_step, rng=None, out=None, out_dtype=None):
        """AVA (ava.py:300-323) with the reference's OWN random stream: the host makes exactly the calls `sample_lfb` makes
        (reference_draw_table below) and the device gathers (vlfb_lfb_gather_slots).  `clip_index[r]` = the position of row r's
        CLIP inside the minibatch (0, 0, 1, 1, 1, ...: the batch-index column the data layer writes into `proposals`,
        ava_data_input.py:175-192) -- NOT a keyframe id: the reference calls sample_lfb once per clip of the minibatch
        (ava.py:230), so a keyframe that was drawn twice into one minibatch makes two draws.  With `rng = np.random` seeded as
        the reference seeds it (np.random.seed(cfg.RNG_SEED)) and the caller's other np.random calls interleaved as the
        reference interleaves them, the sampled banks are the reference's, element for element.  `sample_window` (a
        counter-based key per draw, no host work, no sync) has the same DISTRIBUTION but another stream.  Needs the step
        counts on the host: one small D2H copy per call."""
        rng = np.random if rng is None else rng
        rows = len(videos)
        vid = self._rows_of(videos)
        centre = np.asarray(secs).astype(np.int64).reshape(-1) - self.step_base
        K = int(max_per_step)
        table = reference_draw_table(self.counts(), vid, centre, clip_index, int(window), K, rng)
        qd = self._dev_i32(np.stack([vid, centre], axis=1))
        td = self._dev_i32(table.reshape(-1))
        out = self._out(out, (rows, int(window) * K, self.dim), out_dtype)
        hip.call("vlfb_lfb_gather_slots", C.byref(self.desc), hip.ptr(self.bank), hip.ptr(self.count), hip.ptr(qd), hip.ptr(td),
                 rows, int(window), K, hip.ptr(out), hip.dtype_code(out.dtype))
        torch.cuda.current_stream().synchronize()
        return out

    def sample_frames(self, videos, center_frames, window, clips_per_second, out=None, out_dtype=None):
        """Charades (charades.py:251-276): -> (N, window, dim), the first `window` bank frames inside
        [begin, end] around each clip centre, packed to the front"""
        rows = len(videos)
        qd = self._dev_i32(self.frames_query(videos, center_frames, window, clips_per_second))
        out = self._out(out, (rows, int(window), self.dim), out_dtype)
        self.sample_compact_enqueue(qd, rows, window, out)
        torch.cuda.current_stream().synchronize()
        return out

    def _sample_packed(self, query, window, max_per_step, out, out_dtype):
        rows = len(query)
        qd = self._dev_i32(query)
        out = self._out(out, (rows, int(window), self.dim), out_dtype)
        self.sample_packed_enqueue(qd, rows, window, max_per_step, out)
        torch.cuda.current_stream().synchronize()
        return out

    # the (rows, 3) int32 queries [bank row of the video, first step, last step] the three samplers above and below upload
    def _steps_query(self, videos, lo, hi):
        return np.stack([self._rows_of(videos), lo, hi], axis=1).astype(np.int32)

    def frames_query(self, videos, center_frames, window, clips_per_second):
        """the query of `sample_frames`"""
        return self._steps_query(videos, *frame_window_steps(center_frames, window, clips_per_second))

    def epic_verb_query(self, videos, center_frames, window, clips_per_second=1):
        """the query of `sample_epic_verb`"""
        return self._steps_query(videos, *epic_verb_window_steps(center_frames, window, clips_per_second))

    def epic_noun_query(self, videos, center_frames, window, max_per_frame=10, frames_per_second=1):
        """the query of `sample_epic_noun`"""
        return self._steps_query(videos, *epic_noun_window_steps(center_frames, window, max_per_frame, frames_per_second))

    def sample_compact_enqueue(self, query_dev, rows, window, out):
        """`sample_frames` for a caller that owns every buffer (a `frames_query` it uploaded to `query_dev` in stream order,
        the (rows, window, dim) output): one launch on the current stream, nothing allocated, no synchronisation"""
        assert out.is_contiguous() and out.numel() >= int(rows) * int(window) * self.dim
        hip.call("vlfb_lfb_sample_compact", C.byref(self.desc), hip.ptr(self.bank), hip.ptr(self.count), hip.ptr(query_dev),
                 int(rows), int(window), hip.ptr(out), hip.dtype_code(out.dtype))

    def sample_packed_enqueue(self, query_dev, rows, window, max_per_step, out):
        """`sample_epic_verb` (max_per_step 1) / `sample_epic_noun` for a caller that owns every buffer, as
        `sample_compact_enqueue`"""
        assert out.is_contiguous() and out.numel() >= int(rows) * int(window) * self.dim
        hip.call("vlfb_lfb_sample_packed", C.byref(self.desc), hip.ptr(self.bank), hip.ptr(self.count), hip.ptr(query_dev),
                 int(rows), int(window), int(max_per_step), hip.ptr(out), hip.dtype_code(out.dtype))

    def sample_epic_verb(self, videos, center_frames, window, clips_per_second=1, out=None, out_dtype=None):
        """EPIC-Kitchens verb model (epic.py:310-331): -> (N, window, dim), the first `window` bank clips whose
        centre frame lies within +-(window * FPS) // 2 frames of the clip centre, zero padded"""
        return self._sample_packed(self.epic_verb_query(videos, center_frames, window, clips_per_second), window, 1, out, out_dtype)

    def sample_epic_noun(self, videos, center_frames, window, max_per_frame=10, frames_per_second=1, out=None,
                         out_dtype=None):
        """EPIC-Kitchens noun model (epic.py:338-374): detector features, at most `max_per_frame` per bank frame
        in stored order, frames in time order, truncated to `window` rows, zero padded"""
        query = self.epic_noun_query(videos, center_frames, window, max_per_frame, frames_per_second)
        return self._sample_packed(query, window, max_per_frame, out, out_dtype)

    @classmethod
    def from_epic(cls, lfb, noun, sample_freq=EPIC_FPS, capacity=None, dtype="bf16", device="cuda:0"):
        """`lfb` as the EPIC datasets hold it: verb {video: {frame: feat}} (frames % sample_freq == 0), noun
        {video: {frame: (n, dim) array or []}} (epic.py:191-199)"""
        vids = sorted(lfb)
        frames = [f for v in lfb.values() for f in v]
        assert all(f % sample_freq == 0 for f in frames), "EPIC bank frames must be multiples of the sampling period"
        n_steps = max(frames) // sample_freq + 1 if frames else 1
        feats = [np.asarray(x, dtype=np.float32).reshape(-1, np.shape(x)[-1]) for v in lfb.values() for x in v.values()
                 if np.size(x)]
        dim = feats[0].shape[1]
        cap = capacity or (max(f.shape[0] for f in feats) if noun else 1)
        bank = cls(len(vids), n_steps, cap, dim, dtype, device, 0, vids)
        for v in vids:
            rows, ks = [], []
            for f in sorted(lfb[v]):
                x = lfb[v][f]
                if not np.size(x):
                    continue
                x = np.asarray(x, dtype=np.float32).reshape(-1, dim)
                rows.append(x[:cap])
                ks += [f // sample_freq] * min(cap, x.shape[0])
            if rows:
                bank.append(torch.as_tensor(np.concatenate(rows)), [v] * len(ks), ks)
        bank.check_no_drops()
        return bank

    # ---- interchange with the reference's pickles -----------------------------------------------
    @classmethod
    def from_reference(cls, lfb, capacity=None, dtype="bf16", device="cuda:0", frame_level=False, sample_freq=None):
        """`lfb` as tools/lfb_loader.py writes it: {video: {sec: [feat, ...]}} or, frame_level,
        {video: {frame: feat}}"""
        vids = sorted(lfb)
        if frame_level:
            assert sample_freq, "frame-level banks need sample_freq (FPS // LFB_CLIPS_PER_SECOND)"
            n_steps = max([(max(f) + 1) // sample_freq for f in lfb.values() if len(f)] + [1])
            first = next(iter(next(v for v in lfb.values() if len(v)).values()))
            bank = cls(len(vids), n_steps, 1, int(np.size(first)), dtype, device, 0, vids)
            for v in vids:
                frames = sorted(lfb[v])
                if frames:
                    bank.append_frames(torch.as_tensor(np.stack([np.ravel(lfb[v][f]) for f in frames]).astype(np.float32)),
                                       [(v, f) for f in frames], sample_freq)
            return bank
        secs = [s for v in lfb.values() for s in v]
        base, n_steps = (min(secs), max(secs) - min(secs) + 1) if secs else (0, 1)
        cap = capacity or max([len(l) for v in lfb.values() for l in v.values()] + [1])
        first = next(l[0] for v in lfb.values() for l in v.values() if len(l))
        bank = cls(len(vids), n_steps, cap, int(np.size(first)), dtype, device, base, vids)
        for v in vids:
            feats, ks = [], []
            for s in sorted(lfb[v]):
                for f in lfb[v][s]:
                    feats.append(np.ravel(f))
                    ks.append(s)
            if feats:
                bank.append(torch.as_tensor(np.stack(feats).astype(np.float32)), [v] * len(ks), ks)
        bank.check_no_drops()
        return bank

    def to_reference(self, frame_level=False, sample_freq=None, chunk_rows=65536, epic=False):
        """the reference's dictionaries, fp32: {video: {sec: [feat, ...]}} or, frame_level, {video: {frame: feat}} with the
        frame of step s = sample_freq * (s + 1) - 1 (Charades) or, `epic`, sample_freq * s (EPIC verb).  Reads the
        bank through `packed_chunks`: the device memory it takes is one staging chunk plus the offsets, whatever the bank's size."""
        out = {(self.video_ids[vi] if self.video_ids is not None else vi): {} for vi in range(self.n_videos)}
        names = list(out)
        for feats, keys, n in self.packed_chunks(chunk_rows, torch.float32):
            f = feats[:n].cpu().numpy()
            k = keys[:n].cpu().numpy()
            for r in range(n):
                steps = out[names[k[r, 0]]]
                s = int(k[r, 1])
                if frame_level:
                    steps.setdefault(int(sample_freq * s if epic else sample_freq * (s + 1) - 1), f[r].copy())
                else:
                    steps.setdefault(s + self.step_base, []).append(f[r].copy())
        return out

    # ---- packed export: only occupied rows move ---------------------------------------------------
    MERGE_ROWS = 4096   # rows of one append in merge_from / load: lfb_commit_kernel is quadratic in the rows of a call

    def pack_offsets(self, count=None):
        """int64 (cells + 1,) device tensor of vlfb_lfb_pack_offsets: the packed row at which every cell starts; the last
        entry is the number of features the bank holds.  `count`: another int32 (cells,) device count array of this geometry
        (another rank's) instead of the bank's own."""
        count = self.count if count is None else count
        assert count.is_cuda and count.dtype == torch.int32 and count.is_contiguous() and count.numel() == self.count.numel()
        off = torch.empty(self.n_videos * self.n_steps + 1, device=self.device, dtype=torch.int64)
        hip.call("vlfb_lfb_pack_offsets", C.byref(self.desc), hip.ptr(count), hip.ptr(off))
        return off

    def packed_chunks(self, chunk_rows=65536, out_dtype=None):
        """yields (feats_dev, keys_dev, n): the bank's features in packed order (cell order, then append order), `n` rows at a
        time in ONE staging buffer that the next step overwrites (work enqueued on the current stream before that is safe),
        with the keys `append_enqueue` takes.  One scan, one synchronisation (the total), then one launch per chunk."""
        chunk_rows = int(chunk_rows)
        assert 0 < chunk_rows < (1 << 20), "packed_chunks: chunk_rows must be in (0, 2^20)"
        off = self.pack_offsets()
        total = int(off[-1].item())
        dt = out_dtype or hip.TORCH_DTYPE[self.code]
        rows = min(chunk_rows, total)
        if rows == 0:
            return
        feats = torch.empty((rows, self.dim), device=self.device, dtype=dt)
        keys = torch.empty((rows, 2), device=self.device, dtype=torch.int32)
        for first in range(0, total, chunk_rows):
            n = min(chunk_rows, total - first)
            self._pack_enqueue(off, first, n, feats, keys)
            yield feats, keys, n

    def _pack_enqueue(self, off, first, n, feats, keys):
        hip.call("vlfb_lfb_pack", C.byref(self.desc), hip.ptr(self.bank), hip.ptr(self.count), hip.ptr(off), int(first), int(n),
                 hip.ptr(feats), hip.dtype_code(feats.dtype), hip.ptr(keys))

    # ---- packed import: rows of another bank's packed order, placed without keys -------------------------------------------
    def unpack_enqueue(self, feats, src_count, src_offsets, first_row, n, src_capacity=None, base=None):
        """rows [first_row, first_row + n) of ANOTHER bank's packed order (vlfb_lfb_unpack): `feats` a contiguous (>= n, dim)
        device tensor of any bank element type, `src_count` / `src_offsets` that bank's int32 count and its `pack_offsets`
        (device tensors, same n_videos / n_steps / dim), `src_capacity` its capacity (default this bank's).  Row s of a cell
        goes to slot base[cell] + s, `base` = this bank's count by default; a row past the capacity is counted in `dropped`.
        The launch only READS the count: every chunk of one source is placed against the same base, and `unpack_commit`
        publishes the source once, after its last chunk.  One launch on the current stream, nothing allocated, no
        synchronisation."""
        assert feats.is_cuda and feats.is_contiguous() and feats.numel() >= int(n) * self.dim
        base = self.count if base is None else base
        hip.call("vlfb_lfb_unpack", C.byref(self.desc), hip.ptr(self.bank), hip.ptr(base), hip.ptr(feats),
                 hip.dtype_code(feats.dtype), hip.ptr(src_count), int(src_capacity or self.capacity), hip.ptr(src_offsets),
                 int(first_row), int(n), hip.ptr(self.dropped))

    def unpack_commit(self, src_count, src_capacity=None, count=None):
        """after the last `unpack_enqueue` of one source, ONCE: count = min(count + min(src_count, src_capacity), capacity)
        (vlfb_lfb_unpack_commit); `count` another int32 count array of this geometry instead of the bank's own"""
        count = self.count if count is None else count
        hip.call("vlfb_lfb_unpack_commit", C.byref(self.desc), hip.ptr(count), hip.ptr(src_count),
                 int(src_capacity or self.capacity))

    def _geometry(self):
        return (self.n_videos, self.n_steps, self.capacity, self.dim, self.code, self.step_base, self.video_ids)

    def all_gather_ranks(self, chunk_rows=65536):
        """Every rank's bank becomes the merge of all ranks' banks in rank order -- what rank 0's bank is after merge_from(rank
        1's), merge_from(rank 2's), ...: in every cell rank 0's rows, then rank 1's, ..., at most `capacity`.  A no-op without
        a process group.  Collective: every rank calls it, with the same geometry (n_videos, n_steps, capacity, dim, element
        type, step_base, video_ids; else every rank raises).

        The `count` arrays travel first (cells x 4 bytes per rank); every rank's offsets, totals and the base each rank's rows
        are placed on (the count after the ranks before it) follow from them, so no keys travel.  Then the packed rows, in
        rounds of at most `chunk_rows` rows per rank (the staging memory: world x chunk_rows rows); every rank runs the same
        number of rounds (the largest bank's), a rank with fewer rows sends padding.  The other ranks' chunks are placed with
        vlfb_lfb_unpack against their bases, and this rank's own rows stay where they are -- unless a rank before it holds
        rows of the same cells: then all ranks' rows are placed into a bank of the same geometry (one more bank of memory)
        that is copied back at the end.  Backend nccl: everything stays on the device; gloo: rows go through the host.
        Ends with check_no_drops: a merge that overflows a cell drops the same rows on every rank, so every rank raises."""
        import hashlib
        from vlfb import dist
        assert 0 < int(chunk_rows) < (1 << 20), "all_gather_ranks: chunk_rows must be in (0, 2^20)"
        if not dist.initialized():
            return self
        world, me = dist.world_size(), dist.rank()
        digest = np.frombuffer(hashlib.sha256(repr(self._geometry()).encode()).digest(), dtype=np.int64).copy()
        seen = dist.gather_rows(torch.as_tensor(digest).view(1, -1).to(self.device)).cpu().numpy()
        if not dist.all_ok(bool((seen == seen[0]).all())):
            raise hip.VlfbError("all_gather_ranks: the ranks' banks differ in geometry (n_videos, n_steps, capacity, dim, "
                                "dtype, step_base, video_ids); this rank's: %r" % (self._geometry()[:6],))
        if world == 1:
            self.check_no_drops()
            return self
        cells = self.n_videos * self.n_steps
        counts = dist.gather_rows(self.count.view(1, cells)).contiguous()          # [rank][cell]
        offsets = [self.pack_offsets(counts[k]) for k in range(world)]
        totals = [int(x) for x in torch.stack([o[-1] for o in offsets]).cpu().tolist()]
        bases = torch.zeros((world, cells), device=self.device, dtype=torch.int32)
        merged = torch.zeros(cells, device=self.device, dtype=torch.int32)
        for k in range(world):                                                     # base of rank k = ranks 0 .. k-1 committed
            bases[k].copy_(merged)
            self.unpack_commit(counts[k], count=merged)
        chunk = min(int(chunk_rows), max(totals))
        # this rank's rows stay in place where no rank before it holds rows of their cell (base 0: always so when the ranks'
        # cells are disjoint, as in a sharded pass); otherwise every rank's rows, this one's too, go to a bank of their own
        # first, since the rows of ranks before this one would land on own rows still to be sent
        shared = bool(((bases[me] > 0) & (counts[me] > 0)).any().item())
        dest = self
        if shared:
            dest = DeviceBank(self.n_videos, self.n_steps, self.capacity, self.dim, self.bank.dtype, self.device, self.step_base)
            dest.dropped = self.dropped
        if chunk:
            stage = torch.empty((chunk, self.dim), device=self.device, dtype=self.bank.dtype)
            keys = torch.empty((chunk, 2), device=self.device, dtype=torch.int32)
            for first in range(0, max(totals), chunk):
                rows = [max(0, min(chunk, t - first)) for t in totals]
                if rows[me]:
                    self._pack_enqueue(offsets[me], first, rows[me], stage, keys)
                parts = dist.gather_ragged(stage, rows)
                for k in range(world):
                    if rows[k] and (k != me or shared):
                        dest.unpack_enqueue(parts[k], counts[k], offsets[k], first, rows[k], base=bases[k])
        if shared:
            self.bank.copy_(dest.bank)
        self.count.copy_(merged)
        torch.cuda.current_stream().synchronize()
        self.check_no_drops()
        return self

    def merge_from(self, other):
        """append every feature of `other` behind what this bank holds, in `other`'s order (the partial banks of two runs; the
        ranks of a job merge theirs with `all_gather_ranks`).  n_steps, dim and step_base must agree, the element type need not; banks that both carry `video_ids`
        are matched through them, otherwise row by row.  Raises if a feature did not fit."""
        assert (self.n_steps, self.dim, self.step_base) == (other.n_steps, other.dim, other.step_base), \
            "merge_from: banks differ in n_steps / dim / step_base"
        lut = None
        if self.video_ids is not None and other.video_ids is not None:
            missing = [v for v in other.video_ids if v not in self.video_row]
            if missing:
                raise hip.VlfbError("merge_from: videos %r are not in this bank" % (missing[:8],))
            lut = self._dev_i32([self.video_row[v] for v in other.video_ids])
        else:
            assert self.n_videos == other.n_videos, "merge_from: banks without video_ids must have the same rows"
        for feats, keys, n in other.packed_chunks(self.MERGE_ROWS):
            if lut is not None:
                keys[:n, 0] = lut[keys[:n, 0].long()]
            self.append_enqueue(feats, keys, n)
        self.check_no_drops()

    def save(self, path):
        """native file (.npz): the descriptor, `video_ids`, `count` and the packed rows in the bank's own element type
        (16-bit types as uint16 bit patterns)"""
        host =np.dtype(np.float32) if self.code == hip.F32 else np.dtype(np.uint16)
        parts = []
        for feats, _, n in self.packed_chunks():
            x = feats[:n] if self.code == hip.F32 else feats[:n].view(torch.int16)
            parts.append(x.cpu().numpy().view(host))
        rows = np.concatenate(parts) if parts else np.zeros((0, self.dim), dtype=host)
        fields = dict(n_videos=self.n_videos, n_steps=self.n_steps, capacity=self.capacity, dim=self.dim, dtype=self.code,
                      step_base=self.step_base, has_video_ids=self.video_ids is not None,
                      video_ids=np.asarray(self.video_ids if self.video_ids is not None else []),
                      count=self.counts().astype(np.int32), rows=rows)
        with open(path, "wb") as f:
            np.savez(f, **fields)

    @classmethod
    def load(cls, path, device="cuda:0"):
        """a bank `save` wrote: equal in `count` and, for occupied slots, in bits"""
        with np.load(path, allow_pickle=False) as z:
            code = int(z["dtype"])
            ids = z["video_ids"].tolist() if bool(z["has_video_ids"]) else None
            bank = cls(int(z["n_videos"]), int(z["n_steps"]), int(z["capacity"]), int(z["dim"]), hip.TORCH_DTYPE[code], device,
                       int(z["step_base"]), ids)
            count, rows = z["count"].reshape(-1), z["rows"]
        cells = np.repeat(np.arange(count.size, dtype=np.int64), np.minimum(count, bank.capacity))
        assert cells.size == rows.shape[0], "lfb bank file: %d rows for counts that sum to %d" % (rows.shape[0], cells.size)
        keys = np.stack([cells // bank.n_steps, cells % bank.n_steps], axis=1).astype(np.int32)
        held = []                                              # uploads stay alive until the appends have run
        for first in range(0, cells.size, cls.MERGE_ROWS):
            x = np.ascontiguousarray(rows[first:first + cls.MERGE_ROWS])
            x = torch.from_numpy(x if code == hip.F32 else x.view(np.int16)).to(bank.device)
            x = x if code == hip.F32 else x.view(hip.TORCH_DTYPE[code])
            k = bank._dev_i32(keys[first:first + cls.MERGE_ROWS])
            bank.append_enqueue(x, k, x.shape[0])
            held.append((x, k))
        bank.check_no_drops()
        return bank
