"""Wall time of placing one bank's rows into another on one GPU, keyed (merge_from) against keyless (packed import):

    python tools/lfb_unpack_profile.py profiles/lfb_unpack.txt

A bf16 bank of the AVA train geometry (235 videos x 900 steps x 16 slots x 2048) with binomial counts, placed into an empty
bank of the same geometry: `merge_from` (packed chunks of DeviceBank.MERGE_ROWS rows through vlfb_lfb_append, whose commit
is quadratic in the rows of a call) and the path of DeviceBank.all_gather_ranks without the exchange (packed chunks of 65536
rows through vlfb_lfb_unpack, one vlfb_lfb_unpack_commit).  merge_from is the code of the parent commit, unchanged.  Both
include the packing of the source.  Medians of three runs after one warm-up, one process; a record, not a gate.
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "video-long-term-feature-banks_amd", "lib"), ROOT]

GEOMETRY = (235, 900, 16, 2048)
OCCUPANCY = 0.15


def measure(fn, repeats=3):
    times = []
    for r in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r:
            times.append(time.perf_counter() - t0)
    return float(np.median(times)), times


def main():
    from vlfb.lfb_bank import DeviceBank
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    n_videos, n_steps, capacity, dim = GEOMETRY
    src = DeviceBank(n_videos, n_steps, capacity, dim, "bf16", step_base=902)
    src.bank.normal_()
    counts = np.random.default_rng(0).binomial(capacity, OCCUPANCY, n_videos * n_steps).astype(np.int32)
    src.count.copy_(torch.as_tensor(counts))
    rows = int(counts.sum())
    dst = DeviceBank(n_videos, n_steps, capacity, dim, "bf16", step_base=902)

    def merge():
        dst.count.zero_()
        dst.merge_from(src)

    def unpack():
        dst.count.zero_()
        off = src.pack_offsets()
        first = 0
        for feats, _, n in src.packed_chunks(65536):
            dst.unpack_enqueue(feats, src.count, off, first, n)
            first += n
        dst.unpack_commit(src.count)
        dst.check_no_drops()

    lines = ["bf16 bank %d videos x %d steps x %d slots x %d = %.2f GB, %d features held (%.1f %% of the slots, %.2f GB of rows); "
             "into an empty bank of the same geometry; %s; medians of 3 runs after 1 warm-up, one process"
             % (n_videos, n_steps, capacity, dim, src.bank.numel() * 2 / 1e9, rows, 100.0 * rows / (counts.size * capacity),
                rows * dim * 2 / 1e9, torch.cuda.get_device_name(0)),
             "%-52s %10s   %s" % ("path", "seconds", "runs (s)")]
    for name, fn in (("merge_from (pack 4096 + vlfb_lfb_append)", merge),
                     ("pack 65536 + vlfb_lfb_unpack + one commit", unpack)):
        sec, runs = measure(fn)
        lines.append("%-52s %10.3f   %s" % (name, sec, " ".join("%.3f" % t for t in runs)))
    same = np.array_equal(dst.counts().reshape(-1), counts)
    lines.append("counts after the last run equal the source's: %s" % same)
    text = "\n".join(lines) + "\n"
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write("$ python tools/lfb_unpack_profile.py profiles/lfb_unpack.txt\n" + text)


if __name__ == "__main__":
    main()
