"""vlfb_lfb_count_nonfinite (csrc/vlfb_lfb.hip) through the C ABI: the occupied rows of a bank that hold a NaN or +-Inf
element, counted on the device.  Counts are integers: exact.

The descriptor admits every dim >= 1, so the dims are not multiples of 64 and cover both load widths: a row whose byte
length is a multiple of 16 is read with 16-byte loads (100 fp32, 72 of every type), any other element by element
(100 of a 16-bit type, 3); 2048 is the real feature width."""
import ctypes as C

import numpy as np
import pytest
import torch

from vlfb import hip
from vlfb.lfb_bank import DeviceBank

pytestmark = pytest.mark.gpu
TYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
NAN, INF = float("nan"), float("inf")


def count_into(bank, out):
    hip.call("vlfb_lfb_count_nonfinite", C.byref(bank.desc), hip.ptr(bank.bank), hip.ptr(bank.count), hip.ptr(out))
    return out.cpu().tolist()


@pytest.mark.parametrize("dim", [3, 72, 100, 2048])
@pytest.mark.parametrize("dtype", sorted(TYPES))
def test_planted_rows_are_counted_and_unoccupied_slots_are_not(dtype, dim):
    bank = DeviceBank(2, 3, 2, dim, dtype)                    # 2 videos x 3 steps x capacity 2
    g = torch.Generator().manual_seed(dim)
    rows = bank.bank.view(6, 2, dim)                          # [cell][slot][dim]
    rows.copy_((torch.rand((6, 2, dim), generator=g) * 8 - 4).to(TYPES[dtype]))
    bank.count.copy_(torch.tensor([2, 1, 0, 1, 2, 5], dtype=torch.int32))        # (5 > capacity: the cell holds 2)
    occupied = 2 + 1 + 0 + 1 + 2 + 2
    out = torch.zeros(2, dtype=torch.int64, device=bank.device)
    assert count_into(bank, out) == [0, occupied]
    assert bank.count_nonfinite() == (0, occupied)
    bank.check_finite()
    rows[2, 0, dim // 2] = NAN                                # an unoccupied slot (count 0)
    rows[1, 1, 0] = NAN                                       # a slot beyond count (count 1)
    rows[3, 1, dim - 1] = INF                                 # ... and another
    assert bank.count_nonfinite() == (0, occupied)
    rows[0, 0, 0] = NAN
    rows[0, 0, dim // 2] = NAN                                # a second element of the same row: still one row
    rows[3, 0, dim - 1] = INF                                 # the last element of a row
    rows[5, 1, dim // 3] = -INF
    assert count_into(bank, out) == [3, 2 * occupied]         # a second call ADDS
    assert bank.count_nonfinite() == (3, occupied)
    with pytest.raises(hip.VlfbError, match="3 of %d occupied rows" % occupied):
        bank.check_finite()
    # the largest finite values of the type are finite
    rows[4, 0, :] = torch.finfo(TYPES[dtype]).max
    rows[4, 1, :] = torch.finfo(TYPES[dtype]).min
    assert bank.count_nonfinite() == (3, occupied)


@pytest.mark.parametrize("dtype", sorted(TYPES))
def test_more_rows_than_the_grid_holds(dtype):
    """20000 slots: more rows than one pass of the largest grid covers, so the count cannot depend on who walks which row"""
    n_videos, n_steps, cap, dim = 40, 50, 10, 8
    bank = DeviceBank(n_videos, n_steps, cap, dim, dtype)
    rng = np.random.RandomState(11)
    feats = rng.rand(n_videos * n_steps, cap, dim).astype(np.float32)
    sick = rng.rand(n_videos * n_steps, cap) < 0.05
    kind = rng.randint(0, 3, size=sick.shape)
    at = rng.randint(0, dim, size=sick.shape)
    for c, s in zip(*np.nonzero(sick)):
        feats[c, s, at[c, s]] = (np.nan, np.inf, -np.inf)[kind[c, s]]
    count = rng.randint(0, cap + 3, size=n_videos * n_steps).astype(np.int32)
    bank.bank.view(-1, cap, dim).copy_(torch.from_numpy(feats).to(TYPES[dtype]))
    bank.count.copy_(torch.from_numpy(count))
    live = np.arange(cap)[None, :] < np.minimum(count, cap)[:, None]
    assert bank.count_nonfinite() == (int(np.sum(sick & live)), int(np.sum(live)))
