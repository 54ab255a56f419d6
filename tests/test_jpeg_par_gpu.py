"""The lane-parallel JPEG decode on the device (vlfb_jpeg_decode_batch_par) against PIL's pixels on every element, against the
serial entry point on good, damaged and corrupted streams, and against the host checker's synchronisation counts; then
FrameStore.slots_many and the FrameLoader on top of it.  Files and expected pixels come from tests/golden/jpeg_cases.npz."""
import ctypes as C

import numpy as np
import pytest
import torch

import jpeg_cases as jc
import jpeg_par_cases as pc
from datasets import jpeg
from vlfb import hip

pytestmark = pytest.mark.gpu
GUARD = jc.GUARD
SUBSEQ = (8, 32, 256, 0)                                  # 0: the library's default


def entry(data):
    info = jpeg.parse(data)
    return info, np.frombuffer(data, dtype=np.uint8)[info.scan_start:info.scan_end]


def variant_entry(v):
    item, info, (scan, seg) = pc.variant_item(v)
    return info, scan


def decode_batch(entries, subseq=0, par=True, fill=0x5A):
    """one decode call over `entries` [(JpegInfo, scan bytes)], destinations GUARD bytes apart in one buffer filled with 0xA5,
    the workspace prefilled with `fill` -> ([(H, W, 3) arrays], [guard strips], status words, stats [n][4] or None)"""
    dev = torch.device("cuda:0")
    n = len(entries)
    items = (hip.JpegItem * n)()
    at, place = n * hip.JPEG_ITEM_BYTES, []
    for info, scan in entries:
        seg = np.asarray(info.segment_offsets, dtype=np.uint32).view(np.uint8)
        seg_at = at
        at += -(-seg.size // 16) * 16
        scan_at = at + 3                                        # scans need no alignment: start them off a 16-byte line
        at = scan_at + -(-max(scan.size, 1) // 16) * 16
        place.append((seg_at, seg, scan_at))
    blob = np.zeros(at, dtype=np.uint8)
    dst_at, total = [], GUARD
    for info, _ in entries:
        dst_at.append(total)
        total += info.height * info.width * 3 + GUARD
    out = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
    dev_blob = torch.zeros(at, dtype=torch.uint8, device=dev)
    ws = 0
    for k, ((info, scan), (seg_at, seg, scan_at)) in enumerate(zip(entries, place)):
        it = info.fill(items[k])
        it.seg_offsets, it.scan = dev_blob.data_ptr() + seg_at, dev_blob.data_ptr() + scan_at
        it.dst, it.ws_offset = out.data_ptr() + dst_at[k], ws
        ws += info.workspace_bytes
        blob[seg_at:seg_at + seg.size] = seg
        blob[scan_at:scan_at + scan.size] = scan
    blob[:n * hip.JPEG_ITEM_BYTES] = np.frombuffer(items, dtype=np.uint8)
    dev_blob.copy_(torch.from_numpy(blob))
    workspace = torch.full((ws + 256,), fill, dtype=torch.uint8, device=dev)      # stale bytes, and a guard behind it
    status = torch.full((n,), -7, dtype=torch.int32, device=dev)
    stats = torch.full((n + 1, 4), -7, dtype=torch.int32, device=dev) if par else None
    head = (C.cast(items, C.c_void_p), dev_blob.data_ptr(), n, workspace.data_ptr(), ws, status.data_ptr())
    if par:
        hip.call("vlfb_jpeg_decode_batch_par", *(head + (subseq, stats.data_ptr())))
    else:
        hip.call("vlfb_jpeg_decode_batch", *head)
    torch.cuda.synchronize()
    assert (workspace[ws:] == fill).all()
    if par:
        assert (stats[n] == -7).all()
        stats = stats[:n].cpu().numpy()
    host = out.cpu().numpy()
    pictures = [host[a:a + i.height * i.width * 3].reshape(i.height, i.width, 3) for a, (i, _) in zip(dst_at, entries)]
    guards = [host[a - GUARD:a] for a in dst_at] + [host[-GUARD:]]
    return pictures, guards, status.cpu().numpy(), stats


@pytest.fixture(scope="module")
def good():
    """every good case in one batch through the serial entry point, decoded once and shared"""
    _, files, _ = jc.fixture()
    names = jc.names("good")
    entries = [entry(files[n]) for n in names]
    return names, entries, decode_batch(entries, par=False)


@pytest.mark.parametrize("subseq", SUBSEQ)
def test_good_batch_equals_pil_the_serial_entry_and_the_host_checkers_counts(good, subseq):
    _, files, want = jc.fixture()
    names, entries, (serial, _, serial_status, _) = good
    pictures, guards, status, stats = decode_batch(entries, subseq)
    assert len(names) == 17 and (status == 0).all() and (serial_status == 0).all(), status
    assert all((g == 0xA5).all() for g in guards)
    n_par = 0
    for k, (name, got) in enumerate(zip(names, pictures)):
        diff = np.flatnonzero(got.ravel() != want[name].ravel())
        assert diff.size == 0, "%s: %d of %d bytes differ, first at %d" % (name, diff.size, got.size, diff[0])
        assert got.tobytes() == serial[k].tobytes(), name
        item, info, keep = jc.host_item(files[name])
        host = pc.decode(item, info, 256, subseq)[3]
        assert list(stats[k]) == host, (name, subseq, list(stats[k]), host)   # rounds and chunks are functions of the data
        if pc.is_parallel(info, subseq):
            n_par += 1
            assert stats[k][0] == 1 and stats[k][1] == pc.chunks(info, 256, subseq) and 1 <= stats[k][3] <= 256, (name, list(stats[k]))
        else:
            assert list(stats[k]) == [0, 0, 0, 0], name
    assert n_par >= (4 if subseq in (0, 256) else 10)


def test_workspace_prefill_does_not_show(good):
    names, entries, (serial, _, _, _) = good
    pictures, guards, status, stats = decode_batch(entries, 32, fill=0xFF)
    assert (status == 0).all() and all((g == 0xA5).all() for g in guards)
    for name, a, b in zip(names, serial, pictures):
        assert a.tobytes() == b.tobytes(), name               # the coefficient area really is cleared


def picked_variants():
    """8 of the host test's corruptions, each already through the host checker: redone ones, silently different ones, and the
    first of the rest"""
    _, _, want = jc.fixture()
    redone, silent, other = [], [], []
    for v, ((name, _), (ref, ref_status, par)) in enumerate(zip(pc.variants(), pc.variant_results())):
        if any(stats[0] == 2 for _, _, stats in par):
            redone.append(v)
        elif ref_status == 0 and (ref != want[name]).any():
            silent.append(v)
        else:
            other.append(v)
    assert redone and silent
    pick = redone[:3] + silent[:3]
    return (pick + redone[3:] + silent[3:] + other)[:8], redone, silent


def test_damaged_and_corrupted_streams_between_good_ones_equal_the_serial_entry():
    _, files, want = jc.fixture()
    pick, redone, silent = picked_variants()
    assert len(pick) == 8 and set(pick) & set(redone) and set(pick) & set(silent)
    order = ["420_33x47_opt", "420_40x56_cut_middle", "420_24x40_rst1", "420_40x56_stray_rst", "422_31x33",
             "420_40x56_minus40", "420_32x340"]
    entries = [entry(files[n]) for n in order]
    for v in pick:
        entries.append(variant_entry(v))
        entries.append(entry(files["420_40x56"]))
    serial, guards, serial_status, _ = decode_batch(entries, par=False)
    assert all((g == 0xA5).all() for g in guards)
    results = pc.variant_results()
    for subseq in (16, 64):
        pictures, guards, status, stats = decode_batch(entries, subseq)
        assert all((g == 0xA5).all() for g in guards)
        assert (status & ~pc.STATUS_BITS == 0).all(), status          # no private bit is left
        assert (status == serial_status).all(), (status, serial_status)
        for k, (a, b) in enumerate(zip(serial, pictures)):
            assert a.tobytes() == b.tobytes(), (k, subseq, list(stats[k]))
        assert status[1] & hip.JPEG_TRUNCATED and status[5] & hip.JPEG_TRUNCATED and status[3] & hip.JPEG_BAD_RESTART
        assert stats[1][0] == 2 and stats[5][0] == 2 and stats[3][0] == 0 and stats[2][0] == 0
        for j, v in enumerate(pick):                              # and what the host checker gave for the same variant
            k = len(order) + 2 * j
            ref, ref_status, par = results[v]
            assert status[k] == ref_status and pictures[k].tobytes() == ref.tobytes(), (v, subseq)
            if subseq == 64:
                assert list(stats[k]) == par[1][2], (v, list(stats[k]), par[1][2])
            assert status[k + 1] == 0 and pictures[k + 1].tobytes() == want["420_40x56"].tobytes()
        assert any(stats[len(order) + 2 * j][0] == 2 for j in range(8))


# ---- FrameStore.slots_many -------------------------------------------------------------------------------------------------
H, W = 40, 56


def stores(capacity=12, **kw):
    from datasets.frame_store import FrameStore
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    return FrameStore(H, W, capacity, dev, stream, **kw), FrameStore(H, W, capacity, dev, stream, **kw), stream


REQUESTS = [("v", [3, 4, 4, 7]), ("v", [4, 7, 9]), ("w", [3, 9]), ("v", [9, 3, 11])]


def test_slots_many_is_four_slots_calls_in_one_decode():
    _, files, want = jc.fixture()
    a, b, stream = stores()
    a.fetch_jpeg = b.fetch_jpeg = lambda video, f: files["420_40x56"]
    sa = a.slots_many(REQUESTS)
    sb = [b.slots(video, numbers) for video, numbers in REQUESTS]
    distinct = len({(video, f) for video, numbers in REQUESTS for f in numbers})
    assert sa == sb and distinct == 7
    assert (a.fetched, a.requested) == (b.fetched, b.requested) == (distinct, 12)
    assert (a.decode_calls, a.decoded_frames) == (1, distinct) and (b.decode_calls, b.decoded_frames) == (4, distinct)
    stream.synchronize()
    a.check_decoded()
    b.check_decoded()
    assert torch.equal(a.frames, b.frames)
    assert (a.frames[sa[2][1]].cpu().numpy() == want["420_40x56"]).all() and not a.frames[distinct:].any()
    a.release()
    assert a.slots_many(REQUESTS[:2]) == sa[:2] and a.decode_calls == 1 and a.decoded_frames == distinct      # all resident
    a.release()
    # the serial entry on request, and one store's default subsequence size against another's
    c, d, stream = stores(jpeg_subseq_bytes=-1)
    d.jpeg_subseq_bytes = 16
    c.fetch_jpeg = d.fetch_jpeg = a.fetch_jpeg
    assert c.slots_many(REQUESTS) == d.slots_many(REQUESTS) == sa
    stream.synchronize()
    assert torch.equal(c.frames, a.frames) and torch.equal(d.frames, a.frames) and c.decode_calls == d.decode_calls == 1


def test_slots_many_refuses_a_minibatch_whole():
    _, files, want = jc.fixture()
    a, _, stream = stores()
    by_frame = {33: "420_33x47_opt", 44: "progressive_24x24"}
    a.fetch_jpeg = lambda video, f: files[by_frame.get(f, "420_40x56")]
    first = a.slots_many([("v", [1, 2]), ("v", [2, 5])])
    a.release()
    stream.synchronize()
    state = lambda: (list(a.index.slot_of.items()), list(a.index.free), set(a.index.open), a.fetched, a.requested, a.decode_calls,
                     a.decoded_frames, a.uploaded_bytes)
    before, frames = state(), a.frames.clone()
    with pytest.raises(hip.VlfbError, match="33 x 47"):
        a.slots_many([("v", [5, 6]), ("v", [7]), ("v", [8, 33]), ("v", [9])])
    with pytest.raises(jpeg.JpegUnsupported, match="progressive"):
        a.slots_many([("v", [5, 6]), ("v", [44, 7])])
    with pytest.raises(hip.VlfbError, match="more than the 12 frames"):
        a.slots_many([("v", list(range(10, 17))), ("v", list(range(17, 24)))])
    stream.synchronize()
    assert state() == before and torch.equal(a.frames, frames)             # nothing was enqueued
    asked = []
    a.fetch = lambda video, f: (asked.append(f), want["420_16x16_q100"][:1, :1].repeat(H, 0).repeat(W, 1))[1]
    slots = a.slots_many([("v", [5, 44]), ("v", [44, 6])])          # the refused file goes through `fetch`, the others stay JPEG
    assert asked == [44] and a.decode_calls == 2 and a.decoded_frames == 3 + 1 and first == [[0, 1], [1, 2]]
    stream.synchronize()
    a.check_decoded()
    assert (a.frames[slots[0][1]].cpu().numpy() == want["420_16x16_q100"][0, 0]).all() and slots[0][1] == slots[1][0]
    assert (a.frames[slots[1][1]].cpu().numpy() == want["420_40x56"]).all()


def test_check_decoded_names_the_damaged_frame_of_a_minibatch():
    _, files, want = jc.fixture()
    a, _, stream = stores()
    a.fetch_jpeg = lambda video, f: files["420_40x56_cut_middle" if (video, f) == ("w", 12) else "420_40x56"]
    slots = a.slots_many([("v", [11, 12]), ("w", [12, 13])])
    with pytest.raises(hip.VlfbError, match=r"1 frame\(s\) could not be decoded: \('w', 12\) \(truncated\)"):
        a.check_decoded()
    a.check_decoded()                                   # reported once
    assert (a.frames[slots[0][1]].cpu().numpy() == want["420_40x56"]).all() and (a.frames[slots[1][1]].cpu().numpy() == want["420_40x56"]).all()
    _, ref, _ = jc.decode_host(files["420_40x56_cut_middle"])
    assert (a.frames[slots[1][0]].cpu().numpy() == ref).all()


def test_frame_loader_minibatch_is_one_decode_call():
    """a (store, video, frame_numbers) minibatch of the FrameLoader from a store fed JPEG bytes: the `data` blob is the one
    from a store whose `fetch` returns the fixture's pixels, and the store was asked to decode once for the minibatch"""
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
            counts.append((store.fetched, store.requested, store.decode_calls, store.decoded_frames))
            data.zero_()
        assert counts == [(5, 8, 1, 5), (5, 8, 0, 0)]
        assert torch.equal(blobs[0], blobs[1]) and float(blobs[0].float().abs().max()) > 0
