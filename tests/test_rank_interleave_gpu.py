"""vlfb_rows_interleave (csrc/vlfb_metrics.hip) against a numpy restatement of its row formula: destination row g is row
(g / (b * world)) * b + g % b of part (g / b) % world.  Bytes are compared, so every case is exact.

Row sizes: 4 B (int32 labels), 157 B (multi-hot label rows: the byte path), 320 B (AVA scores: the 16-byte path), 628 B
(Charades scores: the 4-byte path); a 320-byte row from a part whose base is offset by 4 bytes takes the 4-byte path."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
WORLDS, BS, ROW_BYTES = (1, 2, 3), (1, 3), (4, 157, 320, 628)


def totals(b, world):
    """a multiple of b * world; one that ends mid-slice (mid-row-group when b > 1, else after rank 0's slice of the last
    global iteration); one that leaves the last global iteration without a slice for the higher ranks"""
    per = b * world
    return sorted({3 * per, 2 * per + (b // 2 if b > 1 else 1) + (b if world > 2 else 0), 2 * per + b})


def need(total, b, world):
    full, rem = divmod(total, b * world)
    return [full * b + min(max(rem - r * b, 0), b) for r in range(world)]


def expected(parts, b, total, rows_out, row_bytes):
    world = len(parts)
    out = np.full((rows_out, row_bytes), SENTINEL, np.uint8)
    for g in range(total):
        out[g] = parts[(g // b) % world][(g // (b * world)) * b + g % b]
    return out


def device_parts(host, offset=0):
    """each part in a buffer of its own, its base `offset` bytes behind an allocation's (256-byte aligned) start"""
    out = []
    for h in host:
        buf = torch.zeros(h.size + offset + 16, dtype=torch.uint8, device="cuda")
        view = buf[offset:offset + h.size]
        view.copy_(torch.from_numpy(h.reshape(-1)))
        out.append((buf, view))
    return out


def run(host, b, row_bytes, total, rows_out, offset=0, part_rows=None):
    from vlfb import hip
    dev = device_parts(host, offset)
    dst = torch.full((rows_out * row_bytes,), SENTINEL, dtype=torch.uint8, device="cuda")
    addr = (ctypes.c_void_p * len(host))(*[v.data_ptr() for _, v in dev])
    rows = (ctypes.c_int64 * len(host))(*(part_rows if part_rows is not None else [h.shape[0] for h in host]))
    hip.call("vlfb_rows_interleave", addr, rows, len(host), b, row_bytes, total, dst.data_ptr())
    torch.cuda.synchronize()
    return dst.cpu().numpy().reshape(rows_out, row_bytes)


@pytest.mark.parametrize("row_bytes", ROW_BYTES)
@pytest.mark.parametrize("b", BS)
@pytest.mark.parametrize("world", WORLDS)
def test_interleave_equals_the_row_formula(world, b, row_bytes):
    rng = np.random.default_rng(world * 100 + b * 10 + row_bytes)
    for total in totals(b, world):
        rows = need(total, b, world)
        if world > 1:
            assert total % (b * world) == 0 or rows[-1] < rows[0]
        host = [rng.integers(0, 256, (r + 1, row_bytes)).astype(np.uint8) for r in rows]     # (one row more than is asked)
        rows_out = total + 2
        got = run(host, b, row_bytes, total, rows_out)
        want = expected(host, b, total, rows_out, row_bytes)
        assert np.array_equal(got[:total], want[:total]), (world, b, row_bytes, total)
        assert (got[total:] == SENTINEL).all(), "rows at or after total were written"


def test_a_mid_slice_total_and_a_last_iteration_without_the_higher_ranks():
    """the two shapes of an unfinished last global iteration, spelled out for world 3, b 3"""
    assert need(3 * 9 - 9 + 4, 3, 3) == [9, 7, 6]          # ends inside rank 1's slice
    assert need(2 * 9 + 3, 3, 3) == [9, 6, 6]              # rank 0 alone has a slice in the last global iteration
    assert 2 * 9 + 3 in totals(3, 3)


@pytest.mark.parametrize("offset", [4, 1])
def test_part_bases_off_the_16_byte_grid_take_the_narrow_paths(offset):
    """320-byte rows would go 16 bytes at a time; from bases 4 (1) bytes off they go 4 bytes (1 byte) at a time"""
    rng = np.random.default_rng(offset)
    world, b, row_bytes, total = 2, 3, 320, 15
    host = [rng.integers(0, 256, (r, row_bytes)).astype(np.uint8) for r in need(total, b, world)]
    got = run(host, b, row_bytes, total, total + 1, offset=offset)
    assert np.array_equal(got, expected(host, b, total, total + 1, row_bytes))


def test_total_zero_launches_nothing_and_the_binding_wrapper_agrees():
    from vlfb import hip
    from vlfb.metrics import interleave_rows
    host = [np.arange(12, dtype=np.uint8).reshape(3, 4)]
    got = run(host, 1, 4, 0, 2)
    assert (got == SENTINEL).all()
    # vlfb.metrics.interleave_rows: typed tensors, 2-D and 1-D, the total implied by the parts
    rng = np.random.default_rng(3)
    parts = [rng.standard_normal((r, 5)).astype(np.float32) for r in need(11, 2, 3)]
    out = interleave_rows([torch.from_numpy(p).cuda() for p in parts], 2)
    want = expected([p.view(np.uint8) for p in parts], 2, 11, 11, 20)
    assert np.array_equal(out.cpu().numpy().view(np.uint8), want)
    labels = [np.arange(r, dtype=np.int32) + 100 * i for i, r in enumerate(need(11, 2, 3))]
    out = interleave_rows([torch.from_numpy(p).cuda() for p in labels], 2, 9)
    assert np.array_equal(out.cpu().numpy(), expected([p.view(np.uint8).reshape(-1, 4) for p in labels], 2, 9, 9, 4).view(np.int32).reshape(-1))
    with pytest.raises(hip.VlfbError, match="shares"):
        interleave_rows([torch.zeros(2, 5, device="cuda"), torch.zeros(3, 5, device="cuda")], 2)


BAD = {
    "world 0": dict(world=0),
    "world above the limit": dict(world=65),
    "b 0": dict(b=0),
    "row_bytes 0": dict(row_bytes=0),
    "negative total": dict(total=-1),
    "part 0 one row short": dict(part_rows=[5, 6]),
    "part 1 one row short": dict(part_rows=[6, 2]),
    "a NULL part that is read": dict(null_part=1),
    "a NULL destination": dict(null_dst=True),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments_are_refused_before_anything_is_launched(case):
    """world 2, b 3, total 9 asks 6 rows of part 0 and 3 of part 1.  Every refusal is VLFB_ERR_ARG (-1), and the
    destination keeps its sentinel: nothing ran."""
    from vlfb import hip
    kw = BAD[case]
    world, b, row_bytes, total = 2, 3, 16, 9
    parts = [torch.zeros(6 * row_bytes, dtype=torch.uint8, device="cuda"), torch.zeros(3 * row_bytes, dtype=torch.uint8, device="cuda")]
    dst = torch.full((total * row_bytes,), SENTINEL, dtype=torch.uint8, device="cuda")
    n = kw.get("world", world)
    addr = (ctypes.c_void_p * 65)(*[None if kw.get("null_part") == i else p.data_ptr() for i, p in enumerate(parts)])
    rows = (ctypes.c_int64 * 65)(*kw.get("part_rows", [6, 3]))
    rc = hip.lib().vlfb_rows_interleave(addr, rows, n, kw.get("b", b), kw.get("row_bytes", row_bytes), kw.get("total", total),
                                        None if kw.get("null_dst") else dst.data_ptr(), hip.stream())
    assert rc == -1, (case, rc)                                           # VLFB_ERR_ARG
    assert b"rows_interleave" in hip.lib().vlfb_last_error()
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == SENTINEL).all()
    with pytest.raises(hip.VlfbError, match="rows_interleave"):
        hip.call("vlfb_rows_interleave", addr, rows, n, kw.get("b", b), kw.get("row_bytes", row_bytes), kw.get("total", total),
                 None if kw.get("null_dst") else dst.data_ptr())


def test_the_largest_world_is_accepted():
    """64 ranks, one row each: no cap below 64"""
    rng = np.random.default_rng(64)
    host = [rng.integers(0, 256, (1, 8)).astype(np.uint8) for _ in range(64)]
    got = run(host, 1, 8, 64, 64)
    assert np.array_equal(got, np.concatenate(host))
