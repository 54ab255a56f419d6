"""The JPEG path without a GPU: the marker walk of datasets.jpeg on every case of the fixture, the host-compiled format
arithmetic (vlfb_jpeg_decode_host: csrc/vlfb_jpeg_core.h, the text the kernels are compiled from) against PIL's pixels on
every element, the damaged files, and the argument checks of the batch entry points."""
import ctypes as C
import os

import numpy as np
import pytest

import jpeg_cases as jc
from datasets import jpeg
from vlfb import hip

pytestmark = pytest.mark.skipif(not os.path.exists(hip.LIB_PATH), reason="libvlfb_hip.so not built")


def test_fixture_holds_the_cases_and_names_its_decoder():
    meta = jc.fixture()[0]
    assert meta["pil"] and meta["libjpeg_turbo"]
    assert len(jc.cases("good")) == 17 and len(jc.cases("refused")) == 3 and len(jc.cases("damaged")) == 3
    assert os.path.getsize(jc.PATH) < 300 * 1024
    sizes = {(c["height"], c["width"]) for c in jc.cases("good")}
    assert {(1, 1), (9, 3), (9, 5), (2, 40), (32, 340), (8, 2), (7, 4), (13, 17), (33, 47)} <= sizes


@pytest.mark.parametrize("name", jc.names("good"))
def test_parser_reads_size_sampling_tables_and_segments(name):
    _, files, _ = jc.fixture()
    case = [c for c in jc.cases("good") if c["name"] == name][0]
    data = files[name]
    info = jpeg.parse(data)
    assert (info.height, info.width) == (case["height"], case["width"])
    assert [list(hv) for hv in info.sampling] == case["sampling"] and info.n_comp == len(case["sampling"])
    assert len(info.quant) == case["n_quant"] and len(info.huff) == case["n_huff"]
    assert all(len(q) == 64 for q in info.quant.values())
    assert info.restart_interval == case["restart_interval"]
    assert info.scan_start == case["scan_start"] and info.scan_end == len(data) - 2 and data[info.scan_end:] == b"\xff\xd9"
    seg = info.segment_offsets
    assert len(seg) == case["n_segments"] and seg[0] == 0 and seg == sorted(seg)
    for k, off in enumerate(seg[1:]):                  # every later interval follows its RSTn marker, numbered modulo 8
        assert data[info.scan_start + off - 2:info.scan_start + off] == bytes([0xFF, 0xD0 + k % 8])
    # a memoryview parses alike, and nothing of the scan is copied: the offsets index the caller's buffer
    again = jpeg.parse(memoryview(bytearray(data)))
    assert (again.scan_start, again.scan_end, again.segment_offsets) == (info.scan_start, info.scan_end, seg)
    hmax, vmax = info.sampling[0]
    blocks = sum(h * v for h, v in info.sampling) * -(-info.width // (8 * hmax)) * -(-info.height // (8 * vmax))
    item = info.fill(hip.JpegItem())
    assert info.workspace_bytes == 192 * blocks == hip.lib().vlfb_jpeg_workspace_bytes(C.byref(item), 1)


def test_parser_refuses_with_a_reason():
    _, files, _ = jc.fixture()
    reasons = {"progressive": "progressive", "4 components": "4 components", "sampling factors": "sampling factors 1x2"}
    for c in jc.cases("refused"):
        with pytest.raises(jpeg.JpegUnsupported, match=reasons[c["reason"]]):
            jpeg.parse(files[c["name"]])
    good = files["420_40x56"]
    with pytest.raises(jpeg.JpegError, match="not a JPEG"):
        jpeg.parse(b"\x89PNG\r\n\x1a\n" + good[8:])
    for cut in (3, 20, 200, jpeg.parse(good).scan_start - 1):       # inside the header: no scan to hand over
        with pytest.raises(jpeg.JpegError, match="cut short") as e:
            jpeg.parse(good[:cut])
        assert not isinstance(e.value, jpeg.JpegUnsupported)
    assert issubclass(jpeg.JpegUnsupported, jpeg.JpegError)


@pytest.mark.parametrize("name", jc.names("good"))
def test_host_decode_equals_pil_on_every_element(name):
    _, files, want = jc.fixture()
    buf, got, status = jc.decode_host(files[name])
    assert status == 0
    assert got.shape == want[name].shape
    diff = np.flatnonzero(got.ravel() != want[name].ravel())
    assert diff.size == 0, "%d of %d bytes differ, first at %d" % (diff.size, got.size, diff[0])
    assert (buf[:jc.GUARD] == 0xA5).all() and (buf[-jc.GUARD:] == 0xA5).all()


def test_damaged_files_report_a_status_and_stay_inside_the_destination():
    _, files, want = jc.fixture()
    expect = {"420_40x56_cut_middle": hip.JPEG_TRUNCATED, "420_40x56_minus40": hip.JPEG_TRUNCATED,
              "420_40x56_stray_rst": hip.JPEG_BAD_RESTART}
    assert sorted(expect) == sorted(jc.names("damaged"))
    for name, bit in expect.items():
        buf, got, status = jc.decode_host(files[name])
        assert status != 0 and status & bit, (name, status)
        assert (buf[:jc.GUARD] == 0xA5).all() and (buf[-jc.GUARD:] == 0xA5).all()
    # what was decoded before the stream stopped is the good file's: the first MCU row of the file cut in the middle
    _, got, _ = jc.decode_host(files["420_40x56_cut_middle"])
    assert (got[:8] == want["420_40x56"][:8]).all()


def test_batch_argument_checks_need_no_gpu():
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

    def refused(items, n, text, workspace=0x2000, ws_bytes=1 << 40, status=0x3000, items_dev=0x4000):
        rc = lib.vlfb_jpeg_decode_batch(C.cast(items, C.c_void_p), items_dev, n, workspace, ws_bytes, status, None)
        msg = lib.vlfb_last_error().decode()
        assert rc == -1 and text in msg, (rc, msg)             # VLFB_ERR_ARG

    items, keep, ws = batch(files["420_40x56"], files["422_31x33"], files["grey_19x21"])
    assert lib.vlfb_jpeg_workspace_bytes(C.cast(items, C.c_void_p), 3) == ws
    assert lib.vlfb_jpeg_workspace_bytes(C.cast(items, C.c_void_p), 2) == ws - 192 * 9
    refused(items, 0, "n_items")
    refused(items, 65536, "n_items")
    refused(None, 3, "NULL item array")
    refused(items, 3, "NULL buffer", items_dev=None)
    refused(items, 3, "NULL buffer", workspace=None)
    refused(items, 3, "NULL buffer", status=None)
    refused(items, 3, "16-byte aligned", workspace=0x2008)
    refused(items, 3, "the batch needs %d" % ws, ws_bytes=ws - 1)
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
    assert lib.vlfb_jpeg_workspace_bytes(C.cast(items, C.c_void_p), 2) == -1 and "unsupported sampling" in lib.vlfb_last_error().decode()
    items, keep, ws = batch(files["420_40x56"], files["422_31x33"])
    items[0].ta[2] = 2
    refused(items, 2, "item 0 component 2 selects tables")
    items, keep, ws = batch(files["420_40x56"])
    items[0].huff[3][0] = 3                                     # three codes of one bit
    refused(items, 1, "item 0 Huffman table 3 is not a prefix code")
    # the host checker takes the same record and refuses the same way
    status = C.c_int32(0)
    dst = np.zeros(16, dtype=np.uint8)
    assert lib.vlfb_jpeg_decode_host(C.byref(items[0]), dst.ctypes.data, C.byref(status)) == -1
    assert lib.vlfb_jpeg_decode_host(None, dst.ctypes.data, C.byref(status)) == -1
