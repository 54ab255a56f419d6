"""The device JPEG decoder (vlfb_jpeg_decode_batch) against PIL's pixels on every element, through the C ABI and through
FrameStore.fetch_jpeg; the files and the expected pixels come from tests/golden/jpeg_cases.npz only."""
import ctypes as C

import numpy as np
import pytest
import torch

import jpeg_cases as jc
from datasets import jpeg
from vlfb import hip

pytestmark = pytest.mark.gpu
GUARD = jc.GUARD


def decode_batch(datas):
    """one vlfb_jpeg_decode_batch over the files `datas`, destinations GUARD bytes apart in one buffer filled with 0xA5
    -> ([(H, W, 3) arrays], [guard strips], status words)"""
    dev = torch.device("cuda:0")
    n = len(datas)
    infos = [jpeg.parse(d) for d in datas]
    items = (hip.JpegItem * n)()
    blob, at = [], n * hip.JPEG_ITEM_BYTES                     # items, then per file its segment table and its scan
    place = []
    for d, info in zip(datas, infos):
        seg = np.asarray(info.segment_offsets, dtype=np.uint32).view(np.uint8)
        scan = np.frombuffer(d, dtype=np.uint8)[info.scan_start:info.scan_end]
        seg_at = at
        at += -(-seg.size // 16) * 16
        scan_at = at + 3                                        # scans need no alignment: start them off a 16-byte line
        at = scan_at + -(-max(scan.size, 1) // 16) * 16
        place.append((seg_at, seg, scan_at, scan))
    blob = np.zeros(at, dtype=np.uint8)
    dst_at, total = [], GUARD
    for info in infos:
        dst_at.append(total)
        total += info.height * info.width * 3 + GUARD
    out = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
    dev_blob = torch.zeros(at, dtype=torch.uint8, device=dev)
    ws = 0
    for k, (info, (seg_at, seg, scan_at, scan)) in enumerate(zip(infos, place)):
        it = info.fill(items[k])
        it.seg_offsets, it.scan = dev_blob.data_ptr() + seg_at, dev_blob.data_ptr() + scan_at
        it.dst, it.ws_offset = out.data_ptr() + dst_at[k], ws
        ws += info.workspace_bytes
        blob[seg_at:seg_at + seg.size] = seg
        blob[scan_at:scan_at + scan.size] = scan
    blob[:n * hip.JPEG_ITEM_BYTES] = np.frombuffer(items, dtype=np.uint8)
    assert hip.lib().vlfb_jpeg_workspace_bytes(C.cast(items, C.c_void_p), n) == ws
    dev_blob.copy_(torch.from_numpy(blob))
    workspace = torch.full((ws + 256,), 0x5A, dtype=torch.uint8, device=dev)      # stale bytes, and a guard behind it
    status = torch.full((n,), -7, dtype=torch.int32, device=dev)
    hip.call("vlfb_jpeg_decode_batch", C.cast(items, C.c_void_p), dev_blob.data_ptr(), n, workspace.data_ptr(), ws, status.data_ptr())
    torch.cuda.synchronize()
    assert (workspace[ws:] == 0x5A).all()
    host = out.cpu().numpy()
    pictures = [host[a:a + i.height * i.width * 3].reshape(i.height, i.width, 3) for a, i in zip(dst_at, infos)]
    guards = [host[a - GUARD:a] for a in dst_at] + [host[-GUARD:]]
    return pictures, guards, status.cpu().numpy()


@pytest.fixture(scope="module")
def mixed():
    """every good case in one batch, decoded once and shared"""
    _, files, _ = jc.fixture()
    names = jc.names("good")
    return names, decode_batch([files[n] for n in names])


def test_mixed_batch_equals_pil_on_every_pixel(mixed):
    _, _, want = jc.fixture()
    names, (pictures, guards, status) = mixed
    assert len(names) == 17 and (status == 0).all(), status
    for name, got in zip(names, pictures):
        diff = np.flatnonzero(got.ravel() != want[name].ravel())
        assert diff.size == 0, "%s: %d of %d bytes differ, first at %d" % (name, diff.size, got.size, diff[0])
    assert all((g == 0xA5).all() for g in guards)


def test_result_does_not_depend_on_the_batch(mixed):
    _, files, _ = jc.fixture()
    names, (pictures, _, _) = mixed
    back, guards, status = decode_batch([files[n] for n in reversed(names)])
    assert (status == 0).all() and all((g == 0xA5).all() for g in guards)
    for a, b in zip(pictures, reversed(back)):
        assert a.tobytes() == b.tobytes()
    half = len(names) // 2
    for part, ref in ((names[:half], pictures[:half]), (names[half:], pictures[half:])):
        got, guards, status = decode_batch([files[n] for n in part])
        assert (status == 0).all() and all((g == 0xA5).all() for g in guards)
        for a, b in zip(ref, got):
            assert a.tobytes() == b.tobytes()


def test_damaged_files_between_good_ones():
    _, files, want = jc.fixture()
    order = ["420_33x47_opt", "420_40x56_cut_middle", "420_24x40_rst1", "420_40x56_stray_rst", "422_31x33",
             "420_40x56_minus40", "420_32x340"]
    pictures, guards, status = decode_batch([files[n] for n in order])
    assert all((g == 0xA5).all() for g in guards)
    for name, got, word in zip(order, pictures, status):
        if name in want:
            assert word == 0 and got.tobytes() == want[name].tobytes(), name
        else:
            assert word != 0, name
    assert status[1] & hip.JPEG_TRUNCATED and status[5] & hip.JPEG_TRUNCATED and status[3] & hip.JPEG_BAD_RESTART
    # the host checker and the device agree on what a damaged stream gives, pixel for pixel
    for k in (1, 3, 5):
        _, host, host_status = jc.decode_host(files[order[k]])
        assert host_status == status[k] and host.tobytes() == pictures[k].tobytes(), order[k]


# ---- FrameStore.fetch_jpeg ---------------------------------------------------------------------------------------------
H, W = 40, 56


def stores(capacity=8):
    from datasets.frame_store import FrameStore
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    return FrameStore(H, W, capacity, dev, stream), FrameStore(H, W, capacity, dev, stream), stream


def test_store_decodes_what_fetch_would_upload():
    _, files, want = jc.fixture()
    a, b, stream = stores()
    a.fetch_jpeg = lambda video, f: files["420_40x56"]
    b.fetch = lambda video, f: want["420_40x56"]
    numbers = [3, 4, 4, 7, 9, 3]
    sa, sb = a.slots("v", numbers), b.slots("v", numbers)
    assert sa == sb and (a.fetched, a.requested) == (b.fetched, b.requested) == (4, 6)
    a.release()
    b.release()
    sa, sb = a.slots("v", [9, 10, 11]), b.slots("v", [9, 10, 11])
    assert sa == sb and (a.fetched, a.requested) == (b.fetched, b.requested) == (6, 9)
    stream.synchronize()
    a.check_decoded()
    assert torch.equal(a.frames, b.frames)
    assert (a.frames[sa[0]].cpu().numpy() == want["420_40x56"]).all() and not a.frames[6:].any()


def test_frame_loader_clip_is_identical_from_jpeg_bytes():
    """a (store, video, frame_numbers) minibatch of the FrameLoader: the `data` blob from a store fed JPEG bytes is the blob
    from a store whose `fetch` returns the fixture's pixels (40 x 56 frames scaled up to the 64 x 64 crop, as in
    tests/test_frame_loader_gpu.py)"""
    import collections
    import clip_loader_cases as cases
    from datasets.clip_loader import FrameLoader
    from datasets.frame_store import FrameStore
    from models.model_builder_video import ModelBuilder
    from vlfb import synth
    from vlfb.engine import Engine
    _, files, want = jc.fixture()
    N, T = 2, 4
    with cases.loader_cfg("charades_r50_baseline", clips=N, frames=T, extra=["NONLOCAL.CONV3_NONLOCAL", False]) as cfg:
        model = ModelBuilder(train=False, split="test", name="test")
        model.build_model(suffix="_test", lfb_infer_only=True)
        eng = Engine(model, "bf16", device="cuda:0", base_seed=2)
        shapes = {"data_test": (N, 3, T, cases.CROP, cases.CROP), "labels_test": (N, cfg.MODEL.NUM_CLASSES)}
        eng.plan(collections.OrderedDict((name, shapes[name]) for name in model.input_blob_names))
        eng.feed_params({k: v for k, v in synth.params(model, seed=2).items() if k in eng.param_views})
        data, _ = eng.blob_padded("data_test")
        loader = FrameLoader(eng, "_test", 0, n_slots=2, max_src_hw=(H, W), src_sizes=[(H, W)])
        numbers = [[5, 9, 13, 17], [13, 17, 21, 21]]
        blobs, counts = [], []
        for use_jpeg in (True, False):
            store = FrameStore(H, W, 8, loader.device, loader.stream)
            if use_jpeg:
                store.fetch_jpeg = lambda v, f: files["420_40x56"]
            else:
                store.fetch = lambda v, f: want["420_40x56"]
            mb = loader.submit([(store, 0, seq) for seq in numbers], [[1], [2]], dict(iteration=0, videos=[0, 0], centers=[9, 17]),
                               None, [0, 2])
            loader.deliver(mb)
            torch.cuda.synchronize()
            store.check_decoded()
            blobs.append(data.clone())
            counts.append((store.fetched, store.requested))
            data.zero_()
        assert counts[0] == counts[1] == (5, 8)
        assert torch.equal(blobs[0], blobs[1]) and float(blobs[0].float().abs().max()) > 0


def test_store_refuses_another_size_and_unsupported_files():
    _, files, want = jc.fixture()
    a, _, stream = stores()
    by_frame = {1: "420_40x56", 2: "420_40x56", 3: "420_33x47_opt", 4: "progressive_24x24"}
    a.fetch_jpeg = lambda video, f: files[by_frame[f]]
    assert a.slots("v", [1, 2]) == [0, 1]
    a.release()
    before = (a.index.resident(), list(a.index.free), a.fetched, a.requested)
    with pytest.raises(hip.VlfbError, match="33 x 47"):
        a.slots("v", [2, 3])
    assert (a.index.resident(), list(a.index.free), a.fetched, a.requested) == before and not a.index.open
    with pytest.raises(jpeg.JpegUnsupported, match="progressive"):
        a.slots("v", [1, 4])
    assert (a.index.resident(), list(a.index.free), a.fetched, a.requested) == before and not a.index.open
    asked = []
    a.fetch = lambda video, f: (asked.append(f), want["420_16x16_q100"][:1, :1].repeat(H, 0).repeat(W, 1))[1]
    slots = a.slots("v", [1, 4, 2])                     # the refused file goes through `fetch`, the others stay JPEG
    assert asked == [4] and a.fetched == 3
    stream.synchronize()
    a.check_decoded()
    assert (a.frames[slots[1]].cpu().numpy() == want["420_16x16_q100"][0, 0]).all()
    assert (a.frames[slots[0]].cpu().numpy() == want["420_40x56"]).all()


def test_check_decoded_names_the_damaged_frame():
    _, files, want = jc.fixture()
    a, _, stream = stores()
    a.check_decoded()                                   # nothing decoded yet: clean
    a.fetch_jpeg = lambda video, f: files["420_40x56_cut_middle" if f == 12 else "420_40x56"]
    slots = a.slots("vid", [11, 12, 13])
    with pytest.raises(hip.VlfbError, match=r"1 frame\(s\) could not be decoded: \('vid', 12\) \(truncated\)"):
        a.check_decoded()
    a.check_decoded()                                   # reported once
    assert (a.frames[slots[0]].cpu().numpy() == want["420_40x56"]).all() and (a.frames[slots[2]].cpu().numpy() == want["420_40x56"]).all()
    a.release()
    a.slots("vid", [14])
    a.check_decoded()
