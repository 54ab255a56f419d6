"""Baseline JPEG files as the device decoder takes them (include/vlfb.h, vlfb_jpeg_item).

The reference reads every frame with cv2.imread (lib/datasets/data_input_helper.py:51-53); the frames are baseline 4:2:0
JPEGs written by ffmpeg -q:v 1 (dataset_tools/ava/extract_ava_frames.sh:43).  `parse` walks the markers of one file and
returns what the kernels need -- size, sampling, table selectors, the raw DQT / DHT content, the restart interval, where the
scan's bytes lie and where each restart interval begins.  It decodes nothing and copies no pixel data; the scan stays a
slice of the caller's buffer.

    info = parse(data)                  # JpegUnsupported: not baseline / sampling the kernels do not take; JpegError: not a JPEG
    info.fill(item)                     # everything of a vlfb.hip.JpegItem but its addresses
"""
import numpy as np


class JpegError(ValueError):
    """not a JPEG file, or its header is cut short"""


class JpegUnsupported(JpegError):
    """a JPEG file outside what the device decoder takes; the message says why"""


_SOF_NAMES = {0xC1: "extended sequential", 0xC2: "progressive", 0xC3: "lossless", 0xC5: "differential sequential",
              0xC6: "differential progressive", 0xC7: "differential lossless", 0xC9: "arithmetic-coded sequential",
              0xCA: "arithmetic-coded progressive", 0xCB: "arithmetic-coded lossless", 0xCD: "arithmetic-coded differential",
              0xCE: "arithmetic-coded differential progressive", 0xCF: "arithmetic-coded differential lossless"}
SAMPLINGS = {((1, 1),): "grey", ((1, 1), (1, 1), (1, 1)): "4:4:4", ((2, 1), (1, 1), (1, 1)): "4:2:2",
             ((2, 2), (1, 1), (1, 1)): "4:2:0"}


class JpegInfo(object):
    """width, height, n_comp; sampling [(h, v)] and selectors tq / td / ta per component; quant {id: 64 bytes, zigzag order},
    huff {(class, id): 16 counts + symbols} with class 0 = DC, 1 = AC; restart_interval (0 = none); scan_start / scan_end:
    the entropy-coded bytes data[scan_start:scan_end]; segment_offsets: where each restart interval begins, relative to
    scan_start (the first is 0, the others follow a RSTn marker -- every one found, in or out of sequence: the decoder
    checks them)"""

    def __init__(self):
        self.width = self.height = self.n_comp = 0
        self.sampling, self.tq, self.td, self.ta = [], [], [], []
        self.quant, self.huff = {}, {}
        self.restart_interval = 0
        self.scan_start = self.scan_end = 0
        self.segment_offsets = [0]

    subsampling = property(lambda self: SAMPLINGS[tuple(self.sampling)])
    scan_bytes = property(lambda self: self.scan_end - self.scan_start)

    @property
    def workspace_bytes(self):
        """this frame's part of the decoder's workspace (vlfb_jpeg_workspace_bytes): 192 bytes per 8x8 block of every
        component, each component in whole MCUs"""
        hmax, vmax = self.sampling[0]
        mcus = -(-self.width // (8 * hmax)) * -(-self.height // (8 * vmax))
        return 192 * mcus * sum(h * v for h, v in self.sampling)

    def fill(self, item):
        """the format fields of a vlfb.hip.JpegItem; scan, dst, seg_offsets and ws_offset are the caller's"""
        item.scan_bytes, item.n_segments = self.scan_bytes, len(self.segment_offsets)
        item.width, item.height, item.n_comp = self.width, self.height, self.n_comp
        item.restart_interval = self.restart_interval
        for c in range(4):
            on = c < self.n_comp
            item.h[c], item.v[c] = self.sampling[c] if on else (0, 0)
            item.tq[c], item.td[c], item.ta[c] = (self.tq[c], self.td[c], self.ta[c]) if on else (0, 0, 0)
        quant = np.frombuffer(item, dtype=np.uint8, count=256, offset=type(item).quant.offset).reshape(4, 64)
        huff = np.frombuffer(item, dtype=np.uint8, count=4 * 272, offset=type(item).huff.offset).reshape(4, 272)
        quant[:] = 0
        huff[:] = 0
        for t, q in self.quant.items():
            quant[t] = np.frombuffer(q, dtype=np.uint8)
        for (cls, t), h in self.huff.items():
            huff[2 * cls + t, :len(h)] = np.frombuffer(h, dtype=np.uint8)
        return item


def _u16(data, i):
    return (data[i] << 8) | data[i + 1]


def parse(data):
    """-> JpegInfo of the JPEG file in `data` (bytes / bytearray / memoryview)"""
    data = memoryview(data).cast("B") if not isinstance(data, (bytes, bytearray)) else data
    n = len(data)
    if n < 2 or data[0] != 0xFF or data[1] != 0xD8:
        raise JpegError("not a JPEG file: no SOI marker")
    info = JpegInfo()
    comp_ids, frames, i = [], 0, 2
    while True:
        if i + 4 > n:
            raise JpegError("the header is cut short (no SOS marker in %d bytes)" % n)
        if data[i] != 0xFF:
            raise JpegError("no marker at byte %d" % i)
        m = data[i + 1]
        if m == 0xFF:                                   # fill byte
            i += 1
            continue
        if m == 0xD8 or 0xD0 <= m <= 0xD7 or m == 0x01:
            i += 2
            continue
        if m == 0xD9:
            raise JpegError("EOI before any scan")
        length = _u16(data, i + 2)
        seg, end = i + 4, i + 2 + length
        if length < 2 or end > n:
            raise JpegError("the header is cut short (marker %02X at byte %d runs past the end)" % (m, i))
        if m == 0xDB:
            while seg < end:
                pq, t = data[seg] >> 4, data[seg] & 15
                if pq != 0:
                    raise JpegUnsupported("16-bit quantisation table")
                if t > 3 or seg + 65 > end:
                    raise JpegError("bad DQT segment")
                info.quant[t] = bytes(data[seg + 1:seg + 65])
                seg += 65
        elif m == 0xC4:
            while seg < end:
                cls, t = data[seg] >> 4, data[seg] & 15
                if seg + 17 > end:
                    raise JpegError("bad DHT segment")
                count = sum(data[seg + 1:seg + 17])
                if cls > 1 or count > 256 or seg + 17 + count > end:
                    raise JpegError("bad DHT segment")
                if t > 1:
                    raise JpegUnsupported("Huffman table id %d (baseline has 0 and 1)" % t)
                info.huff[(cls, t)] = bytes(data[seg + 1:seg + 17 + count])
                seg += 17 + count
        elif m == 0xC0:
            frames += 1
            if frames > 1:
                raise JpegUnsupported("more than one frame")
            if length < 8:
                raise JpegError("bad SOF segment")
            precision, info.height, info.width, info.n_comp = data[seg], _u16(data, seg + 1), _u16(data, seg + 3), data[seg + 5]
            if precision != 8:
                raise JpegUnsupported("%d-bit samples" % precision)
            if info.n_comp not in (1, 3):
                raise JpegUnsupported("%d components (1 or 3 are supported)" % info.n_comp)
            if length != 8 + 3 * info.n_comp:
                raise JpegError("bad SOF segment")
            if info.width == 0 or info.height == 0:
                raise JpegUnsupported("size %d x %d (a height given by a DNL marker is not supported)" % (info.height, info.width))
            for c in range(info.n_comp):
                cid, hv, tq = data[seg + 6 + 3 * c], data[seg + 7 + 3 * c], data[seg + 8 + 3 * c]
                comp_ids.append(cid)
                info.sampling.append((hv >> 4, hv & 15))
                info.tq.append(tq)
            if info.n_comp == 1:
                info.sampling = [(1, 1)]                # a single component is not interleaved: its factors do not matter
            if tuple(info.sampling) not in SAMPLINGS:
                raise JpegUnsupported("sampling factors %s (supported: luma 1x1, 2x1 or 2x2 with chroma 1x1)"
                                      % " ".join("%dx%d" % hv for hv in info.sampling))
        elif m in _SOF_NAMES:
            raise JpegUnsupported("%s JPEG (SOF%d); only baseline (SOF0) is supported" % (_SOF_NAMES[m], m - 0xC0))
        elif m == 0xCC:
            raise JpegUnsupported("arithmetic coding (DAC)")
        elif m == 0xDD:
            if length != 4:
                raise JpegError("bad DRI segment")
            info.restart_interval = _u16(data, seg)
        elif m == 0xDA:
            if not frames:
                raise JpegError("SOS before SOF")
            ns = data[seg]
            if length != 6 + 2 * ns:
                raise JpegError("bad SOS segment")
            if ns != info.n_comp:
                raise JpegUnsupported("a scan of %d of the %d components (one scan must hold all)" % (ns, info.n_comp))
            for c in range(ns):
                cid, tables = data[seg + 1 + 2 * c], data[seg + 2 + 2 * c]
                if cid != comp_ids[c]:
                    raise JpegUnsupported("scan components out of frame order")
                info.td.append(tables >> 4)
                info.ta.append(tables & 15)
            for c in range(ns):
                if info.tq[c] not in info.quant:
                    raise JpegError("component %d uses quantisation table %d, which the file does not define" % (c, info.tq[c]))
                if (0, info.td[c]) not in info.huff or (1, info.ta[c]) not in info.huff:
                    raise JpegError("component %d uses Huffman tables %d / %d, which the file does not define"
                                    % (c, info.td[c], info.ta[c]))
            info.scan_start = end
            break
        # APPn, COM and everything else with a length: skipped
        i = end
    # the scan: up to the first marker that is neither a stuffed zero, a fill byte nor RSTn (or the end of a truncated file)
    a = np.frombuffer(data, dtype=np.uint8)
    info.scan_end = n
    ff = np.flatnonzero(a[info.scan_start:n - 1] == 0xFF) + info.scan_start
    nxt = a[ff + 1]
    marks = ff[(nxt != 0) & (nxt != 0xFF)]
    for j in marks.tolist():
        if 0xD0 <= a[j + 1] <= 0xD7:
            info.segment_offsets.append(j + 2 - info.scan_start)
        else:
            info.scan_end = j
            break
    return info
