"""vlfb_conv_run_maxpool (csrc/vlfb_gemm_nt.h POOL2): a two-plane conv and the temporal max-pool behind it as ONE launch,
against the two launches it replaces -- vlfb_conv_run_args into the un-pooled planes, then vlfb_maxpool_fwd -- on the same
operands.  The pooled hi plane, the pooled lo plane and the arg-max bytes must be EQUAL, byte for byte: the fused epilogue
selects on the reconstructed hi + lo of the planes a row would have stored, in tap order with a strict >, as the pool kernel
does.  Every case carries what the real launch (res2_2_branch2c + pool2) carries: column bias, two-plane residual, ReLU.
The fused outputs are NaN / 0xFF filled where they must be written and sit between guard bands that must survive.

Descriptor pairs the library does not implement are REFUSED by vlfb_conv_maxpool_fusable and, with VLFB_ERR_UNSUPPORTED,
by the entry point itself; every case of the table below must be accepted."""
import math

import pytest
import torch

from gpu_util import dev, to_nthwc, w_to_kernel

pytestmark = pytest.mark.gpu

hip = None
GUARD = 512
SENT16 = -7.0            # sentinel of the fp16 guard bands
SENT8 = 0xAB             # ... of the arg-max guard bands


def setup_module(module):
    from vlfb import hip as h
    module.hip = h
    h.lib()


def teardown_module(module):
    # hand the cached blocks back: later test files measure peaks of the caching allocator, which depend on the free blocks
    # earlier files leave behind
    torch.cuda.empty_cache()


def gpu(t):
    return t.to(dev())


def pair_of(x):
    xg = gpu(x.contiguous().float())
    out = torch.empty(2 * xg.numel(), device=dev(), dtype=torch.float16)
    hip.call("vlfb_pair_split", hip.ptr(xg), hip.ptr(out), xg.numel())
    return out


# name -> (N, T, H, W, Cs, Cn, integer operands)
CASES = {
    "a_one_chunk_two_clips": (2, 4, 8, 8, 32, 128, False),      # one 64-position chunk per frame pair, tiles next to a clip boundary, ONE k-tile (two-pass staging)
    "b_ragged_chunk_and_columns": (1, 2, 9, 9, 64, 136, False),  # 81 = 64 + 17 positions, 136 = 128 + 8 columns
    "c_odd_t": (1, 3, 8, 8, 64, 256, False),                    # the last frame has no window
    "d_several_chunks": (1, 4, 16, 16, 64, 256, False),         # four chunks per frame, two k-tiles (one-pass staging)
    "ties": (2, 4, 8, 8, 32, 128, True),                        # small integers: exact sums, frequent positive ties
}


def operands(case):
    N, T, H, W, Cs, Cn, integer = CASES[case]
    gen = torch.Generator().manual_seed(sum(map(ord, case)))
    if integer:
        x = torch.randint(-1, 2, (N, Cs, T, H, W), generator=gen).float()
        w = torch.randint(-1, 2, (Cn, Cs, 1, 1, 1), generator=gen).float()
        bias = torch.zeros(Cn)
        res = torch.zeros(N, Cn, T, H, W)
    else:
        x = torch.randn(N, Cs, T, H, W, generator=gen)
        w = torch.randn(Cn, Cs, 1, 1, 1, generator=gen) * (1.0 / math.sqrt(Cs))
        bias = torch.randn(Cn, generator=gen)
        res = torch.randn(N, Cn, T, H, W, generator=gen)
    A = pair_of(to_nthwc(x))
    Wf = torch.empty(2, Cn, 1, Cs, device=dev(), dtype=torch.float16)
    hip.call("vlfb_weight_prep", hip.ptr(gpu(w_to_kernel(w).contiguous())), None, hip.ptr(Wf), None, hip.MIXH, Cn, 1, Cs)
    R = pair_of(to_nthwc(res))
    d = hip.conv_desc(mode=hip.FPROP, dtype=hip.F16, out_dtype=hip.F16, N=N, Tr=T, Hr=H, Wr=W, Ts=T, Hs=H, Ws=W, Cs=Cs, Cn=Cn,
                      relu=1, bias_mode=hip.BIAS_COL, math=hip.MATH_F16X3, a_pstride=x.numel(), b_pstride=Cn * Cs,
                      alpha=1.0 / hip.MIX_W2_SCALE)
    To = T // 2
    pd = hip.pool_desc(hip.F16PAIR, N, T, H, W, Cn, To, H, W, (2, 1, 1), (2, 1, 1), (0, 0, 0))
    return d, pd, A, Wf, gpu(bias), R


def unfused(d, pd, A, Wf, bias, R):
    """(un-pooled planes, pooled planes [2][n], arg-max bytes) of the two separate launches"""
    n_in = d.N * d.Tr * d.Hr * d.Wr * d.Cn
    n_out = pd.N * pd.To * pd.Ho * pd.Wo * pd.C
    O = torch.full((2 * n_in,), float("nan"), device=dev(), dtype=torch.float16)
    hip.conv_run(d, A, Wf, None, O, bias=bias, R=R, R_lo=R[n_in:], O_lo=O[n_in:])
    Y = torch.full((2 * n_out,), float("nan"), device=dev(), dtype=torch.float16)
    am = torch.full((n_out,), 0xFF, device=dev(), dtype=torch.uint8)
    hip.call("vlfb_maxpool_fwd", pd, hip.ptr(O), hip.ptr(Y), hip.ptr(am))
    return O, Y, am


def guarded(n, dtype, sentinel, fill):
    buf = torch.full((n + 2 * GUARD,), sentinel, device=dev(), dtype=dtype)
    buf[GUARD:GUARD + n] = fill
    return buf


def guards_intact(buf, n, sentinel):
    b = buf.cpu()
    return bool((b[:GUARD] == sentinel).all()) and bool((b[GUARD + n:] == sentinel).all())


@pytest.mark.parametrize("case", sorted(CASES))
def test_fused_conv_pool2_equals_conv_then_pool(case):
    d, pd, A, Wf, bias, R = operands(case)
    assert hip.conv_plan(d).startswith("nt_pair f16x3 128x128"), hip.conv_plan(d)
    assert hip.conv_maxpool_fusable(d, pd), "case %s must be accepted" % case
    assert hip.lib().vlfb_conv_maxpool_fusable(d, pd) == 1
    n_in = d.N * d.Tr * d.Hr * d.Wr * d.Cn
    n_out = pd.N * pd.To * pd.Ho * pd.Wo * pd.C
    O, Y, am = unfused(d, pd, A, Wf, bias, R)
    assert not torch.isnan(Y.float()).any()
    if CASES[case][6]:
        # a condition on the INPUTS, not a tolerance: windows whose maximum is positive and attained by both taps are frequent
        v = (O[:n_in].float() + O[n_in:].float()).cpu().view(d.N, d.Tr, -1)[:, :2 * pd.To].reshape(d.N, pd.To, 2, -1)
        share = float(((v[:, :, 0] == v[:, :, 1]) & (v[:, :, 0] > 0)).float().mean())
        print("\n[%s] share of windows with a positive maximum on both taps: %.4f" % (case, share))
        assert share >= 0.01, share
    for with_argmax in (True, False):
        hi = guarded(n_out, torch.float16, SENT16, float("nan"))
        lo = guarded(n_out, torch.float16, SENT16, float("nan"))
        fam = guarded(n_out, torch.uint8, SENT8, 0xFF)
        hip.conv_run_maxpool(d, pd, A, Wf, hi[GUARD:], lo[GUARD:], argmax=fam[GUARD:] if with_argmax else None, bias=bias,
                             R=R, R_lo=R[n_in:])
        torch.cuda.synchronize()
        # bit patterns, not values: -0.0 and +0.0 are different outputs
        assert torch.equal(hi[GUARD:GUARD + n_out].view(torch.int16).cpu(), Y[:n_out].view(torch.int16).cpu()), "pooled hi plane"
        assert torch.equal(lo[GUARD:GUARD + n_out].view(torch.int16).cpu(), Y[n_out:].view(torch.int16).cpu()), "pooled lo plane"
        assert guards_intact(hi, n_out, SENT16) and guards_intact(lo, n_out, SENT16)
        if with_argmax:
            assert torch.equal(fam[GUARD:GUARD + n_out].cpu(), am.cpu()), "arg-max bytes"
        else:
            assert bool((fam.cpu()[GUARD:GUARD + n_out] == 0xFF).all()), "arg-max written without a pointer"
        assert guards_intact(fam, n_out, SENT8)


def test_pairs_the_library_does_not_fuse_are_refused():
    d, pd, A, Wf, bias, R = operands("a_one_chunk_two_clips")
    n_in = d.N * d.Tr * d.Hr * d.Wr * d.Cn
    n_out = pd.N * pd.To * pd.Ho * pd.Wo * pd.C
    hi = torch.zeros(n_out, device=dev(), dtype=torch.float16)
    lo = torch.zeros(n_out, device=dev(), dtype=torch.float16)
    refused = []
    # the spatial pool (pool1's window) behind the same conv
    refused.append((d, hip.pool_desc(hip.F16PAIR, d.N, d.Tr, d.Hr, d.Wr, d.Cn, d.Tr, d.Hr // 2, d.Wr // 2, (1, 3, 3), (1, 2, 2), (0, 1, 1))))
    # a pool over another tensor than the conv's output
    refused.append((d, hip.pool_desc(hip.F16PAIR, d.N, d.Tr, d.Hr, d.Wr, d.Cn // 2, pd.To, d.Hr, d.Wr, (2, 1, 1), (2, 1, 1), (0, 0, 0))))
    # a conv with 64-column tiles
    d64 = hip.ConvDesc.from_buffer_copy(bytes(d))
    d64.Cn = 64
    refused.append((d64, hip.pool_desc(hip.F16PAIR, d.N, d.Tr, d.Hr, d.Wr, 64, pd.To, d.Hr, d.Wr, (2, 1, 1), (2, 1, 1), (0, 0, 0))))
    # an fp32 output
    d32 = hip.ConvDesc.from_buffer_copy(bytes(d))
    d32.out_dtype = hip.F32
    refused.append((d32, pd))
    for dd, pp in refused:
        assert not hip.conv_maxpool_fusable(dd, pp)
        with pytest.raises(hip.VlfbError, match="conv_run_maxpool"):
            hip.conv_run_maxpool(dd, pp, A, Wf, hi, lo, bias=bias, R=R, R_lo=R[n_in:])
    # operands the fused launch needs
    with pytest.raises(hip.VlfbError, match="pooled planes"):
        hip.call("vlfb_conv_run_maxpool", d, pd, hip.ConvArgs(hip.ptr(A), hip.ptr(Wf), None, hip.ptr(hi)), None)
