"""The lane-parallel JPEG entropy decode without a GPU: vlfb_jpeg_decode_host_par (csrc/vlfb_jpeg_core.h compiled for the
host, the text the parallel kernel is compiled from, its lanes run one after another) against PIL's pixels on every element
and against the serial checker vlfb_jpeg_decode_host on damaged and corrupted streams; the argument checks of both new
entry points; and the multi-request bookkeeping of the frame store's index."""
import ctypes as C
import os

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_par_cases as pc
from vlfb import hip

pytestmark = pytest.mark.skipif(not os.path.exists(hip.LIB_PATH), reason="libvlfb_hip.so not built")

LANES = (1, 3, 64, 256)
SUBSEQ = (8, 12, 32, 256)


@pytest.mark.parametrize("name", jc.names("good"))
def test_host_par_equals_pil_and_reports_its_route(name):
    _, files, want = jc.fixture()
    item, info, keep = jc.host_item(files[name])
    for lanes in LANES:
        for subseq in SUBSEQ:
            buf, got, status, stats = pc.decode(item, info, lanes, subseq)
            where = (name, lanes, subseq, stats)
            assert status == 0, where
            diff = np.flatnonzero(got.ravel() != want[name].ravel())
            assert diff.size == 0, "%r: %d of %d bytes differ, first at %d" % (where, diff.size, got.size, diff[0])
            assert (buf[:jc.GUARD] == 0xA5).all() and (buf[-jc.GUARD:] == 0xA5).all(), where
            if pc.is_parallel(info, subseq):
                assert stats[0] == 1, where                        # never 2: the serial decoder takes every good file
                assert stats[1] == pc.chunks(info, lanes, subseq), where
                assert stats[1] <= stats[2] and 1 <= stats[3] <= lanes and stats[3] <= stats[2] <= stats[1] * stats[3], where
                if lanes == 1:
                    assert stats[2] == stats[1] and stats[3] == 1, where
            else:
                assert stats == [0, 0, 0, 0], where


def test_the_rule_routes_restart_files_and_tiny_files_to_the_serial_decoder():
    _, files, _ = jc.fixture()
    routed = {}
    for name in jc.names("good"):
        item, info, keep = jc.host_item(files[name])
        routed[name] = [pc.decode(item, info, 64, s)[3][0] for s in SUBSEQ]
        assert routed[name] == [1 if pc.is_parallel(info, s) else 0 for s in SUBSEQ], name
        if info.restart_interval:
            assert routed[name] == [0, 0, 0, 0]
        elif info.scan_bytes < 16:
            assert routed[name] == [0, 0, 0, 0]
    assert sum(1 for r in routed.values() if r == [0, 0, 0, 0]) >= 3          # two restart files and the 1 x 1 file
    assert sum(1 for r in routed.values() if r == [1, 1, 1, 1]) >= 4
    assert any(r == [1, 1, 1, 0] for r in routed.values())                    # shorter than two subsequences of 256
    # the default: subseq_bytes 0
    item, info, keep = jc.host_item(files["420_32x340"])
    assert pc.decode(item, info, 256, 0)[3] == pc.decode(item, info, 256, pc.DEFAULT_SUBSEQ)[3]


def test_damaged_files_are_the_serial_decoders():
    _, files, _ = jc.fixture()
    assert len(jc.names("damaged")) == 3
    for name in jc.names("damaged"):
        item, info, keep = jc.host_item(files[name])
        _, ref, ref_status, _ = pc.decode(item, info)
        assert ref_status != 0
        for lanes, subseq in ((1, 8), (64, 16), (256, 64), (256, 256)):
            buf, got, status, stats = pc.decode(item, info, lanes, subseq)
            assert status == ref_status and (got == ref).all(), (name, lanes, subseq, status, ref_status)
            assert (buf[:jc.GUARD] == 0xA5).all() and (buf[-jc.GUARD:] == 0xA5).all()
            assert stats[0] == (2 if pc.is_parallel(info, subseq) else 0), (name, lanes, subseq, stats)


def test_seeded_corruptions_are_the_serial_decoders():
    _, files, want = jc.fixture()
    variants, results = pc.variants(), pc.variant_results()
    assert len(variants) == pc.N_VARIANTS == len(results)
    assert any(b == 0xFF for _, e in variants for _, b in e) and any(b == 0x00 for _, e in variants for _, b in e)
    redone = silent = 0
    for (name, edits), (ref, ref_status, par) in zip(variants, results):
        for got, status, stats in par:
            assert status == ref_status, (name, edits, status, ref_status, stats)
            assert (got == ref).all(), (name, edits, stats)
            assert stats[0] in (1, 2)
            assert status & ~pc.STATUS_BITS == 0
        redone += any(stats[0] == 2 for _, _, stats in par)
        silent += ref_status == 0 and bool((ref != want[name]).any())
    assert redone >= 1 and silent >= 1, (redone, silent)      # otherwise the seed exercises nothing


def test_argument_checks_need_no_gpu():
    _, files, _ = jc.fixture()
    lib = hip.lib()

    def batch(*datas):
        items = (hip.JpegItem * len(datas))()
        keep, ws = [], 0
        for k, d in enumerate(datas):
            it, info, arrays = jc.host_item(d)
            C.memmove(C.byref(items[k]), C.byref(it), hip.JPEG_ITEM_BYTES)
            items[k].dst, items[k].ws_offset = 0x1000, ws      # never dereferenced: every call returns before a launch
            ws += info.workspace_bytes
            keep.append(arrays)
        return items, keep, ws

    def refused(items, n, text, workspace=0x2000, ws_bytes=1 << 40, status=0x3000, items_dev=0x4000, subseq=0):
        rc = lib.vlfb_jpeg_decode_batch_par(C.cast(items, C.c_void_p), items_dev, n, workspace, ws_bytes, status, subseq, None, None)
        msg = lib.vlfb_last_error().decode()
        assert rc == -1 and text in msg, (rc, msg)             # VLFB_ERR_ARG
        if subseq == 0 and n != 65536 and items is not None:   # the serial entry refuses the same way, in the same words
            rc = lib.vlfb_jpeg_decode_batch(C.cast(items, C.c_void_p), items_dev, n, workspace, ws_bytes, status, None)
            assert rc == -1 and lib.vlfb_last_error().decode().replace("jpeg_decode_batch", "jpeg_decode_batch_par") == msg

    items, keep, ws = batch(files["420_40x56"], files["422_31x33"], files["grey_19x21"])
    refused(items, 0, "n_items")
    refused(items, 65536, "n_items")
    refused(None, 3, "NULL item array")
    refused(items, 3, "NULL buffer", items_dev=None)
    refused(items, 3, "NULL buffer", workspace=None)
    refused(items, 3, "NULL buffer", status=None)
    refused(items, 3, "16-byte aligned", workspace=0x2008)
    refused(items, 3, "the batch needs %d" % ws, ws_bytes=ws - 1)
    for bad in (4, 6, 10, 4100, -8):
        refused(items, 3, "subseq_bytes %d" % bad, subseq=bad)
    for field, value, text in (("width", 0, "item 1 has size"), ("height", 65536, "item 1 has size"), ("n_comp", 4, "item 1 has 4 components"),
                               ("dst", 0, "item 1 has a NULL address"), ("scan", 0, "item 1 has a NULL address"),
                               ("seg_offsets", 0, "item 1 has a NULL address"), ("n_segments", 0, "item 1 has no segment"),
                               ("scan_bytes", 1 << 30, "item 1 has a scan of"), ("restart_interval", -1, "item 1 has restart interval"),
                               ("ws_offset", 16, "item 1 has ws_offset 16")):
        items, keep, ws = batch(files["420_40x56"], files["422_31x33"], files["grey_19x21"])
        setattr(items[1], field, value)
        refused(items, 3, text)
    items, keep, ws = batch(files["420_40x56"], files["422_31x33"])
    items[1].h[0], items[1].v[0] = 1, 2
    refused(items, 2, "item 1 has unsupported sampling 1x2")
    items, keep, ws = batch(files["420_40x56"], files["422_31x33"])
    items[0].ta[2] = 2
    refused(items, 2, "item 0 component 2 selects tables")
    items, keep, ws = batch(files["420_40x56"])
    items[0].huff[3][0] = 3                                     # three codes of one bit
    refused(items, 1, "item 0 Huffman table 3 is not a prefix code")

    # the host checker: the same record refused the same way, its own two arguments, and a NULL stats
    status = C.c_int32(0)
    dst = np.zeros(40 * 56 * 3, dtype=np.uint8)

    def host(item, lanes, subseq, stats=None, dst_ptr=dst.ctypes.data):
        return lib.vlfb_jpeg_decode_host_par(item, dst_ptr, C.byref(status), lanes, subseq, stats)

    assert host(C.byref(items[0]), 64, 32) == -1 and "not a prefix code" in lib.vlfb_last_error().decode()
    assert host(None, 64, 32) == -1 and "NULL buffer" in lib.vlfb_last_error().decode()
    item, info, keep = jc.host_item(files["420_40x56"])
    assert host(C.byref(item), 64, 32, dst_ptr=None) == -1
    for lanes in (0, 1025, -1):
        assert host(C.byref(item), lanes, 32) == -1 and "lanes %d" % lanes in lib.vlfb_last_error().decode()
    for bad in (4, 6, 10, 4100):
        assert host(C.byref(item), 64, bad) == -1 and "subseq_bytes %d" % bad in lib.vlfb_last_error().decode()
    for lanes in (1, 1024):
        assert host(C.byref(item), lanes, 8) == 0 and status.value == 0           # NULL stats
    _, ref, _ = jc.decode_host(files["420_40x56"])
    assert (dst.reshape(ref.shape) == ref).all()


def test_store_index_takes_a_minibatch_back_whole():
    from datasets.frame_store import StoreIndex
    ix = StoreIndex(6)
    first = ix.assign_many([("a", [0, 1, 2]), ("a", [2, 3])])
    assert first == [([0, 1, 2], [(0, 0), (1, 1), (2, 2)]), ([2, 3], [(3, 3)])]        # a shared frame is missing once
    ix.release()
    assert ix.assign("a", [1, 4]) == ([1, 4], [(4, 4)])
    ix.release()
    state = lambda: (list(ix.slot_of.items()), list(ix.free), set(ix.open), ix.fetched, ix.requested)
    before = state()
    assert before[3:] == (5, 7)
    # four requests, the third of which cannot be held: the first two evicted frames and opened theirs -- all taken back
    with pytest.raises(hip.VlfbError, match="more than the 6 frames"):
        ix.assign_many([("b", [0, 1]), ("a", [4, 9]), ("b", [2, 3, 4, 5]), ("a", [0])])
    assert state() == before
    # undo after a whole multi-request assign (a frame of it could not be fetched) does the same
    out = ix.assign_many([("b", [0, 1]), ("a", [4, 9]), ("b", [1, 2]), ("a", [3])])
    assert [len(m) for _, m in out] == [2, 1, 1, 0] and state() != before
    assert out[1][0][0] == 4 and out[3][0] == [3]                                         # resident frames keep their slots
    ix.undo()
    assert state() == before
    # and the one-request form is the same code
    one = ix.assign("b", [7, 7, 8])
    assert one[0][0] == one[0][1] and len(one[1]) == 2 and ix.requested == 10 and ix.fetched == 7
