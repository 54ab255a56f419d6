"""Wall time and peak device memory of the bank's export paths on one GPU:

    python tools/lfb_pack_profile.py profiles/lfb_pack.txt

A bf16 bank of 16 videos x 900 steps x 16 slots x 2048 at about 30 % occupancy (binomial counts).  Measured: `to_reference`
(packed chunks), the dense loop it replaced (restated below: an fp32 copy of the whole bank on the device and on the host),
`save` and `merge_from` into an empty bank of the same geometry.  Medians of three runs after one warm-up, all in one process.
"""
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "video-long-term-feature-banks_amd", "lib"), ROOT]

GEOMETRY = (16, 900, 16, 2048)


def dense_to_reference(bank):
    """DeviceBank.to_reference before it read packed chunks"""
    cnt = bank.counts()
    data = bank.bank.view(bank.n_videos, bank.n_steps, bank.capacity, bank.dim).float().cpu().numpy()
    out = {}
    for vi in range(bank.n_videos):
        out[vi] = {}
        for s in np.nonzero(cnt[vi])[0]:
            out[vi][int(s + bank.step_base)] = [data[vi, s, k].copy() for k in range(cnt[vi, s])]
    return out


def measure(fn, repeats=3):
    """(median seconds, median rise of the peak of allocated device memory in bytes) after one warm-up"""
    times, peaks = [], []
    for r in range(repeats + 1):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        del out
        if r:
            times.append(dt)
            peaks.append(torch.cuda.max_memory_allocated() - before)
    return float(np.median(times)), int(np.median(peaks)), times


def main():
    from vlfb.lfb_bank import DeviceBank
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    n_videos, n_steps, capacity, dim = GEOMETRY
    bank = DeviceBank(n_videos, n_steps, capacity, dim, "bf16", step_base=902)
    bank.bank.normal_()
    rng = np.random.default_rng(0)
    counts = rng.binomial(capacity, 0.3, n_videos * n_steps).astype(np.int32)
    bank.count.copy_(torch.as_tensor(counts))
    rows = int(counts.sum())
    other = DeviceBank(n_videos, n_steps, capacity, dim, "bf16", step_base=902)
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "bank.npz")

    def merge():
        other.count.zero_()
        other.merge_from(bank)

    lines = ["bf16 bank %d videos x %d steps x %d slots x %d = %.1f MB, %d features held (%.1f %% of the slots); %s; "
             "medians of 3 runs after 1 warm-up, one process"
             % (n_videos, n_steps, capacity, dim, bank.bank.numel() * 2 / 1e6, rows, 100.0 * rows / (counts.size * capacity),
                torch.cuda.get_device_name(0)),
             "%-34s %10s %16s   %s" % ("path", "seconds", "peak device MB", "runs (s)")]
    for name, fn in (("to_reference (packed chunks)", bank.to_reference), ("to_reference (dense loop, before)", lambda: dense_to_reference(bank)),
                     ("save (.npz, packed bf16 rows)", lambda: bank.save(path)), ("merge_from (into an empty bank)", merge)):
        sec, peak, runs = measure(fn)
        lines.append("%-34s %10.3f %16.2f   %s" % (name, sec, peak / 1e6, " ".join("%.3f" % t for t in runs)))
    lines.append("file written by save: %.1f MB" % (os.path.getsize(path) / 1e6))
    os.remove(path)
    os.rmdir(tmp)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
