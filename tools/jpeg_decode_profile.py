#!/usr/bin/env python
"""What decoding a minibatch of JPEG frames on the device costs: 256 distinct 256 x 340 4:2:0 baseline files (8 clips of 32
frames), generated here with PIL at the quality whose mean file size is nearest --target-bytes (ffmpeg -q:v 1 frames of this
size are 30-90 KB), against the decoded-frame feed (`fetch` returning prepared arrays, as tools/frame_store_pass.py).

  device time   vlfb_jpeg_decode_batch of the 256 frames, device events on an otherwise idle device
  host time     FrameStore.slots() for 256 missing frames: parse + copy into the pinned ring + enqueue (no device wait)
  bytes         what slots() copies host-to-device
  PIL           single-thread decode of one file (libjpeg-turbo, the library behind cv2.imread), where PIL is importable

With --par the lane-parallel entry point is measured beside the serial one: vlfb_jpeg_decode_batch_par alone at every
--subseq size (with its synchronisation counts: chunks, rounds per chunk, items redone serially), and the host time of ONE
FrameStore.slots_many() for the same 256 missing frames as 8 clips of 32.

Medians of --repeats after --warmup, one process.  With --overlap, tools/loader_overlap.py --jpeg runs afterwards in a
process of its own (the training step beside a loader whose store is fed these bytes) and its table is appended.

    python tools/jpeg_decode_profile.py --overlap > profiles/jpeg_decode.txt
"""
import argparse
import io
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "video-long-term-feature-banks_amd", "lib"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def make_frames(n, h, w, target_bytes, seed=0):
    """-> (n JPEG files, n decoded (h, w, 3) BGR arrays, quality): smooth shapes under texture noise, 4:2:0 baseline"""
    from PIL import Image
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]

    def picture(k):
        a = np.stack([128 + 90 * np.sin(x / (9.0 + k % 7) + y / 23.0 + k), 128 + 90 * np.cos(x / 31.0 - y / (11.0 + k % 5)),
                      (x * 3 + y * 5 + 17 * k) % 256], -1)
        return np.clip(a + rng.randn(h, w, 3) * 18, 0, 255).astype(np.uint8)

    def encode(a, q):
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, "JPEG", quality=q, subsampling="4:2:0")
        return buf.getvalue()

    probe = [picture(k) for k in range(4)]
    quality = min(range(50, 101), key=lambda q: abs(np.mean([len(encode(a, q)) for a in probe]) - target_bytes))
    files = [encode(picture(k), quality) for k in range(n)]
    pixels = [np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(f)))[:, :, ::-1]) for f in files]
    return files, pixels, quality


def median_ms(v):
    return float(np.median(v)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--src", type=int, nargs=2, default=[256, 340])
    ap.add_argument("--target-bytes", type=int, default=55000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--overlap", action="store_true", help="append tools/loader_overlap.py --jpeg")
    ap.add_argument("--par", action="store_true", help="measure vlfb_jpeg_decode_batch_par and FrameStore.slots_many as well")
    ap.add_argument("--subseq", type=int, nargs="+", default=[32, 64, 128, 256, 512, 1024],
                    help="subsequence sizes of the --par sweep (0: the library's default)")
    args = ap.parse_args()

    import torch
    from datasets.frame_store import FrameStore
    from vlfb import hip
    try:
        import PIL
    except ImportError:
        sys.exit("PIL is not importable here: the frames cannot be generated")
    assert torch.cuda.is_available(), "needs the GPU: nothing here is measured on a CPU"
    n, (H, W) = args.frames, args.src
    files, pixels, quality = make_frames(n, H, W, args.target_bytes)
    sizes = [len(f) for f in files]
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    numbers = list(range(n))

    def feed(jpeg_fed, many=False):
        store = FrameStore(H, W, n, dev, stream)
        if jpeg_fed:
            store.fetch_jpeg = lambda v, f: files[f]
        else:
            store.fetch = lambda v, f: pixels[f]
        host, device, moved = [], [], []
        for rep in range(args.warmup + args.repeats):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            before = store.uploaded_bytes
            ev[0].record(stream)
            t0 = time.perf_counter()
            if many:                                    # the minibatch as the loader hands it over: 8 clips of 32 frames
                store.slots_many([(rep, numbers[c:c + 32]) for c in range(0, n, 32)])
            else:
                store.slots(rep, numbers)               # a new video every time: all frames are missing
            host.append(time.perf_counter() - t0)
            ev[1].record(stream)
            store.release()
            torch.cuda.synchronize()
            device.append(ev[0].elapsed_time(ev[1]) * 1e-3)
            moved.append(store.uploaded_bytes - before)
        store.check_decoded()
        w = args.warmup
        return store, median_ms(host[w:]), median_ms(device[w:]), moved[-1]

    store_j, host_j, span_j, bytes_j = feed(True)
    store_d, host_d, span_d, bytes_d = feed(False)
    assert torch.equal(store_j.frames, store_d.frames), "the device decode differs from PIL's pixels"

    # the decode batch alone: the last chunk's records are still in the ring and on the device
    parsed = [(0, f, f, files[f], __import__("datasets.jpeg", fromlist=["parse"]).parse(files[f])) for f in numbers]
    torch.cuda.synchronize()
    st, base, nbytes, items = store_j._stage_jpeg(parsed)
    j = store_j._jpeg
    import ctypes as C
    with torch.cuda.stream(stream):
        j["dev"][base:base + nbytes].copy_(st["pin"][base:base + nbytes])
        decode = []
        for rep in range(args.warmup + args.repeats):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record(stream)
            hip.call("vlfb_jpeg_decode_batch", C.cast(items, C.c_void_p), j["dev"].data_ptr() + base, n, j["workspace"].data_ptr(),
                     j["workspace"].numel(), j["status"].data_ptr())
            ev[1].record(stream)
            torch.cuda.synchronize()
            decode.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    assert not j["status"][:n].any() and (store_j.frames[5].cpu().numpy() == pixels[5]).all()      # (frame f went to slot f)

    sweep = []
    if args.par:
        want = store_j.frames.clone()
        stats = torch.zeros(n, 4, dtype=torch.int32, device=dev)
        with torch.cuda.stream(stream):
            for subseq in args.subseq:
                times = []
                for rep in range(args.warmup + args.repeats):
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    store_j.frames.zero_()
                    torch.cuda.synchronize()
                    ev[0].record(stream)
                    hip.call("vlfb_jpeg_decode_batch_par", C.cast(items, C.c_void_p), j["dev"].data_ptr() + base, n,
                             j["workspace"].data_ptr(), j["workspace"].numel(), j["status"].data_ptr(), subseq, stats.data_ptr())
                    ev[1].record(stream)
                    torch.cuda.synchronize()
                    times.append(ev[0].elapsed_time(ev[1]) * 1e-3)
                assert not j["status"][:n].any() and torch.equal(store_j.frames, want), "the parallel decode differs (subseq %d)" % subseq
                t = stats.cpu().numpy().astype(np.int64)
                par = t[t[:, 0] > 0]
                sweep.append((subseq, median_ms(times[args.warmup:]), int((t[:, 0] == 1).sum()), int((t[:, 0] == 2).sum()),
                              int((t[:, 0] == 0).sum()), float(par[:, 1].mean()) if len(par) else 0.0,
                              float(par[:, 2].sum()) / max(1, int(par[:, 1].sum())), int(par[:, 3].max()) if len(par) else 0))
        store_m, host_m, span_m, bytes_m = feed(True, many=True)
        assert torch.equal(store_m.frames, store_d.frames) and store_m.decode_calls == args.warmup + args.repeats

    from PIL import Image
    pil = []
    for f in files[:64]:
        t0 = time.perf_counter()
        np.asarray(Image.open(io.BytesIO(f)))
        pil.append(time.perf_counter() - t0)

    print("%d frames of %d x %d, 4:2:0 baseline, PIL %s quality %d: files of %d..%d bytes, mean %d (target %d); %s; medians of %d after %d warm-up"
          % (n, H, W, PIL.__version__, quality, min(sizes), max(sizes), int(np.mean(sizes)), args.target_bytes,
             torch.cuda.get_device_name(0), args.repeats, args.warmup))
    print("%-34s %12s %12s" % ("", "JPEG bytes", "decoded feed"))
    print("%-34s %12.3f %12.3f   ms" % ("host time of slots(), 256 missing", host_j, host_d))
    print("%-34s %12.3f %12.3f   ms (events around slots() on the store's stream, idle device)" % ("device span: copy (+ decode)", span_j, span_d))
    print("%-34s %12.3f %12s   ms (three launches; events, idle device)" % ("vlfb_jpeg_decode_batch alone", median_ms(decode[args.warmup:]), "-"))
    print("%-34s %12.2f %12.2f   MB per batch" % ("bytes uploaded", bytes_j / 1e6, bytes_d / 1e6))
    if args.par:
        print("%-34s %12.3f %12s   ms (8 requests of 32 frames: one copy, one decode call)" % ("host time of ONE slots_many()", host_m, "-"))
        print("%-34s %12.3f %12s   ms (events around slots_many() on the store's stream, idle device)" % ("device span of it", span_m, "-"))
        print("vlfb_jpeg_decode_batch_par alone (four launches; events, idle device), per subseq_bytes:")
        print("  %8s %10s %9s %7s %7s %8s %13s %11s" % ("subseq", "ms", "parallel", "redone", "serial", "chunks", "rounds/chunk", "most rounds"))
        for row in sweep:
            print("  %8d %10.3f %9d %7d %7d %8.2f %13.2f %11d" % row)
    print("PIL (libjpeg-turbo) on this host, one thread: %.3f ms per frame (median of 64) = %.0f ms of core time per batch"
          % (median_ms(pil), median_ms(pil) * n))
    print("the device's pixels equal PIL's on all %d frames" % n)
    sys.stdout.flush()
    if args.overlap:
        del store_j, store_d
        torch.cuda.empty_cache()
        cmd = [sys.executable, os.path.join(ROOT, "tools", "loader_overlap.py"), "--jpeg", "--target-bytes", str(args.target_bytes)]
        print("\n$ python tools/loader_overlap.py --jpeg   (the `loader` row: a store fed these JPEG bytes, every frame new every step)")
        sys.stdout.flush()
        subprocess.run(cmd, check=True)


if __name__ == "__main__":
    main()
