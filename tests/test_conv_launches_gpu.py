"""Every conv launch the engine issues, replayed against the fp64 descriptor model (tests/conv_desc_ref.py), plus the edges
where tile kernels go wrong.

Replay: hip.conv_run is wrapped around the first training step and one test-mode forward of the engine; only descriptors
and which operands were passed are recorded.  The records reduce to signatures -- the plan string with the split count
bucketed to 1 / >1, plus the operand and epilogue features present -- and each signature's descriptor is shrunk (N, T,
then H / W) to the smallest one with the same plan, run through the library and compared with the model: NaN-filled outputs
that must be written in full, sentinel guard bands that must survive, relative L2 at the kernel tests' bars and an
elementwise bound tight enough to catch one dropped k-tile (conv_desc_ref.Case.check).
"""
import collections

import pytest
import torch

import conv_desc_ref as cr

pytestmark = pytest.mark.gpu

hip = None


def setup_module(module):
    from vlfb import hip as h
    module.hip = h
    h.lib()


def replay(d, ops=(), seed=0, scale=1.0):
    c = cr.Case(d, ops, seed=seed, scale=scale)
    c.run(hip)
    return c, c.check()


def desc(**kw):
    d = cr.desc_dict(hip.conv_desc(**kw))
    return d


# ------------------------------------------------------------------------------------------------ launch capture
def _op_set(args, O):
    ops = set()
    for k in ("bias", "rowscale", "R", "mask", "O_planes", "dbias", "R_lo", "O_lo"):
        if args.get(k) is not None:
            ops.add(k)
    return ops


def capture(run):
    """(desc dict, operand set) of every hip.conv_run that `run()` issues"""
    rec = []
    orig = hip.conv_run

    def wrapped(d, A, B, P, O, **kw):
        ops = _op_set(kw, O)
        if d.algo == cr.ALGO_CLASS0 and kw.get("R") is not None and hip.ptr(kw["R"]) == hip.ptr(O):
            ops.add("class0_inplace")
        rec.append((cr.desc_dict(d), frozenset(ops)))
        return orig(d, A, B, P, O, **kw)

    hip.conv_run = wrapped
    try:
        run()
    finally:
        hip.conv_run = orig
    torch.cuda.synchronize()
    return rec


def signature(dtype, d, ops):
    flags = [k for k in ("relu", "accumulate", "wgrad_bias") if d[k]]
    flags += ["%s=%d" % (k, d[k]) for k in ("bias_mode", "a_planes", "p_planes", "o_planes", "out_dtype") if d[k]]
    if max(d["batch"], 1) > 1:
        flags.append("batched")
    if d["mode"] == cr.DGRAD and d["dt"] == 0:
        flags.append("dt0")
    return "%s|%s|%s" % (dtype, cr.plan_key(hip.conv_plan(hip.conv_desc(**d))), ",".join(sorted(flags) + sorted(ops)))


def engine_launches(preset, dtype, overrides):
    import test_model_gpu as tm
    recs = []
    cfg, model, eng, inputs, params, seed_fn = tm.build(preset, dtype, overrides=overrides)

    def step():
        eng.forward()
        eng.backward()
    recs += capture(step)
    del eng
    cfg, model, eng, inputs, params, seed_fn = tm.build(preset, dtype, overrides=overrides, train=False)
    recs += capture(eng.forward)
    del eng
    torch.cuda.empty_cache()
    return recs


def replay_all(dtype, recs):
    sigs = collections.OrderedDict()
    for d, ops in recs:
        sigs.setdefault(signature(dtype, d, ops), (d, ops))
    pf = lambda e: hip.conv_plan(hip.conv_desc(**e))
    failures = []
    for i, (sig, (d, ops)) in enumerate(sigs.items()):
        e = cr.shrink(d, pf)
        try:
            replay(e, ops, seed=i)
        except (AssertionError, cr.Unmodelled, hip.VlfbError) as ex:
            failures.append("%s: %s %s" % (sig, type(ex).__name__, (str(ex).splitlines() or [""])[0]))
    print("\n[%s] %d launches, %d signatures replayed" % (dtype, len(recs), len(sigs)))
    return sigs, failures


BASELINE_PRESETS = ("charades_r50_baseline", "charades_r50_lfb_nl", "ava_r50_lfb_nl", "ava_r101_lfb_nl_3l")
def sizes(clips, frames, crop):
    """the same clip shape for the training step and the test-mode forward"""
    return ["NUM_GPUS", 1] + [x for split in ("TRAIN", "TEST") for x in (split + ".BATCH_SIZE", clips, split + ".VIDEO_LENGTH",
                                                                        frames, split + ".CROP_SIZE", crop)]


SMALL = sizes(2, 16, 64)        # test_model_gpu.SMALL
BENCH = sizes(8, 32, 224)       # the benchmarked plan (bench.py defaults)


@pytest.mark.parametrize("dtype", ["mix", "fp16", "bf16", "split", "fp32"])
@pytest.mark.parametrize("preset", BASELINE_PRESETS)
def test_small_engine_launches_match_the_model(preset, dtype):
    sigs, failures = replay_all(dtype, engine_launches(preset, dtype, SMALL))
    assert sigs and not failures, "\n".join(failures)


@pytest.mark.parametrize("dtype", ["mix", "fp16", "bf16", "split", "fp32"])
def test_benchmarked_launches_match_the_model(dtype):
    sigs, failures = replay_all(dtype, engine_launches("ava_r50_lfb_nl", dtype, BENCH))
    assert sigs and not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ edge cases
def plain(dtype, M, K, Cn, **kw):
    return desc(mode=cr.FPROP, dtype=dtype, out_dtype=kw.pop("out_dtype", dtype), N=1, Tr=1, Hr=1, Wr=M, Ts=1, Hs=1, Ws=M,
                Cs=K, Cn=Cn, **kw)


# (M, K, Cn, kernel of the 16-bit launch, kernel of the two-plane launch): ragged M one row past a tile and below one tile,
# Cn = tile + 8, K of one k-tile, K on either side of the 512 at which the two-plane forward moves to the 256-row kernel and
# of the K >= 1024 at which a 512-column 16-bit launch does.  The kernel is asserted (family and tile), so that a change of
# the planner's rules that moves a case shows up here instead of quietly testing another kernel.
EDGE_16 = {
    "M129": (129, 256, 128, "nt 128x128", "nt_pair 128x128"),
    "M257": (257, 640, 256, "nt 128x128", "nt_pair 128x128"),
    "M5": (5, 128, 64, "nt_skinny 128x64", "nt_pair 128x64"),
    "M197": (197, 1024, 256, "nt 128x128", "nt_pair 128x128"),
    "Cn136": (300, 256, 136, "nt 128x128", "nt_pair 128x128"),
    "Cn264": (1000, 1024, 264, "nt 128x128", "nt_pair 128x128"),
    "K64": (300, 64, 128, "nt 128x128", "nt_pair 128x128"),
    "K448": (4000, 448, 256, "nt 128x128", "nt_pair 128x128"),
    "K512": (4000, 512, 256, "nt 128x128", "nt8_pair 196x128"),
    "K576": (4000, 576, 256, "nt 128x128", "nt8_pair 196x128"),
    "K512_M3000": (3000, 512, 512, "nt 128x128", "nt8_pair 196x128"),
    "K960_Cn512": (3000, 960, 512, "nt 128x128", "nt8_pair 196x128"),
    "K1024_Cn512": (3000, 1024, 512, "nt8 196x128", "nt8_pair 196x128"),
}


def kernel_of(d):
    """family and tile of the plan of `d` ("nt8 196x128" of "nt8 f16 196x128 pre")"""
    words = hip.conv_plan(hip.conv_desc(**d)).split()
    return "%s %s" % (words[0], words[2])


@pytest.mark.parametrize("dt", [cr.BF16, cr.F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("case", sorted(EDGE_16))
def test_plain_16bit_edges(case, dt):
    M, K, Cn, kern, _ = EDGE_16[case]
    d = plain(dt, M, K, Cn, relu=1, bias_mode=cr.BIAS_COL, alpha=0.75)
    assert kernel_of(d) == kern, hip.conv_plan(hip.conv_desc(**d))
    replay(d, ("bias", "R"), seed=M + K)


@pytest.mark.parametrize("case", sorted(EDGE_16))
def test_plain_f16x3_edges(case):
    M, K, Cn, _, kern = EDGE_16[case]
    d = plain(cr.F16, M, K, Cn, out_dtype=cr.F16, math=cr.MATH_F16X3, a_pstride=M * K, alpha=1.0 / 1024)
    assert kernel_of(d) == kern, hip.conv_plan(hip.conv_desc(**d))
    replay(d, ("O_lo",), seed=K)
    d = plain(cr.F16, M, K, Cn, out_dtype=cr.F16, math=cr.MATH_F16X3, a_pstride=M * K, alpha=1.0 / 1024, relu=1,
              bias_mode=cr.BIAS_COL)
    assert kernel_of(d) == kern, hip.conv_plan(hip.conv_desc(**d))
    replay(d, ("bias", "R", "R_lo", "O_lo"), seed=K + 1)


def f16x3_gather(T, H, W, Cs, Cn, k, p, s=(1, 1, 1)):
    To = (T + 2 * p[0] - k[0]) // s[0] + 1
    Ho = (H + 2 * p[1] - k[1]) // s[1] + 1
    Wo = (W + 2 * p[2] - k[2]) // s[2] + 1
    return desc(mode=cr.FPROP, dtype=cr.F16, out_dtype=cr.F16, N=1, Tr=To, Hr=Ho, Wr=Wo, Ts=T, Hs=H, Ws=W, Cs=Cs, Cn=Cn,
                kt=k[0], kh=k[1], kw=k[2], pt=p[0], ph=p[1], pw=p[2], st=s[0], sh=s[1], sw=s[2], dt=1, dh=1, dw=1,
                math=cr.MATH_F16X3, a_pstride=T * H * W * Cs, alpha=1.0 / 1024, relu=1, bias_mode=cr.BIAS_COL)


# two-plane (F16X3) launches whose planes hold exactly 32 elements, and their neighbours of 8 and 64
PLANE_CASES = {
    "p32_row1_c32": lambda: plain(cr.F16, 1, 32, 64, out_dtype=cr.F16, math=cr.MATH_F16X3, a_pstride=32),
    "p32_rows4_c8": lambda: plain(cr.F16, 4, 8, 64, out_dtype=cr.F16, math=cr.MATH_F16X3, a_pstride=32),
    "p32_tap333_c32": lambda: f16x3_gather(1, 1, 1, 32, 64, (3, 3, 3), (1, 1, 1)),
    "p32_tap311_c32": lambda: f16x3_gather(1, 1, 1, 32, 64, (3, 1, 1), (1, 0, 0)),
    "p8_row1_c8": lambda: plain(cr.F16, 1, 8, 64, out_dtype=cr.F16, math=cr.MATH_F16X3, a_pstride=8),
    "p64_row2_c32": lambda: plain(cr.F16, 2, 32, 64, out_dtype=cr.F16, math=cr.MATH_F16X3, a_pstride=64),
    "p64_tap333_c64": lambda: f16x3_gather(1, 1, 1, 64, 64, (3, 3, 3), (1, 1, 1)),
    "p64_tap311_t2_c32": lambda: f16x3_gather(2, 1, 1, 32, 64, (3, 1, 1), (1, 0, 0)),
}


@pytest.mark.parametrize("case", sorted(PLANE_CASES))
def test_f16x3_small_planes(case):
    d = PLANE_CASES[case]()
    assert hip.conv_plan(hip.conv_desc(**d)).startswith("nt_pair f16x3"), hip.conv_plan(hip.conv_desc(**d))
    ops = ("O_lo", "bias") if d["bias_mode"] else ("O_lo",)
    replay(d, ops, seed=len(case))


def test_dgrad_doubled_tap_and_w2i_and_class0():
    # the two-term DGRAD of `mix` as the doubled-tap form (kt = 2, dt = 0) and as F16W2, with residual + mask
    base = dict(mode=cr.DGRAD, dtype=cr.F16, out_dtype=cr.F16, N=1, Tr=4, Hr=9, Wr=9, Ts=4, Hs=9, Ws=9, Cs=128, Cn=64,
                kh=3, kw=3, ph=1, pw=1, dh=1, dw=1, alpha=1.0 / 1024)
    replay(desc(kt=2, dt=0, **base), ("R", "mask", "R_lo", "O_lo"), seed=1)
    replay(desc(kt=1, dt=1, math=cr.MATH_F16W2, **base), ("R", "mask"), seed=2)
    # the 16-bit DGRAD of a (1, 2, 2)-strided 1x1x1 conv as an in-place accumulate over the rows it touches
    d = desc(mode=cr.DGRAD, dtype=cr.F16, out_dtype=cr.F16, N=1, Tr=2, Hr=10, Wr=10, Ts=2, Hs=5, Ws=5, Cs=128, Cn=64,
             sh=2, sw=2, algo=cr.ALGO_CLASS0)
    replay(d, ("R", "class0_inplace"), seed=3)


@pytest.mark.parametrize("dt", [cr.F32, cr.BF16, cr.F16], ids=["f32", "bf16", "f16"])
def test_wgrad_epilogues(dt):
    base = dict(mode=cr.WGRAD, dtype=dt, out_dtype=cr.F32, N=2, Tr=4, Hr=14, Wr=14, Ts=4, Hs=14, Ws=14, Cs=64, Cn=128,
                kt=3, kh=1, kw=1, pt=1, dt=1, dh=1, dw=1, alpha=0.5)
    replay(desc(accumulate=1, **base), ("rowscale",), seed=4)
    replay(desc(splits=8, **base), ("rowscale",), seed=5)
    replay(desc(**dict(base, kt=1, pt=0), wgrad_bias=1), ("rowscale", "dbias"), seed=6)


def test_model_weight_planes_are_what_weight_prep_writes():
    """the model builds its weight operands in Python (every descriptor shape, no weight tensor behind it); pin those
    builders to vlfb_weight_prep bit for bit: the three bf16 planes of VLFB_SPLIT, the two fp16 planes of VLFB_MIXH and the
    interleaved two-term rows of VLFB_MIX_W2I ([Cin][taps][Cout / 64][term][64] of (w * s) * 2^10)"""
    gen = torch.Generator().manual_seed(21)
    cout, taps, cin = 128, 3, 96
    w = torch.randn(cout, taps, cin, generator=gen) * 0.05
    s = torch.rand(cout, generator=gen) + 0.5
    ws = w * s.view(-1, 1, 1)
    wg, sg = w.cuda(), s.cuda()
    f3 = torch.empty(3, cout, taps, cin, device="cuda", dtype=torch.bfloat16)
    hip.call("vlfb_weight_prep", hip.ptr(wg), hip.ptr(sg), hip.ptr(f3), None, hip.SPLIT, cout, taps, cin)
    f2 = torch.empty(2, cout, taps, cin, device="cuda", dtype=torch.float16)
    hip.call("vlfb_weight_prep", hip.ptr(wg), hip.ptr(sg), hip.ptr(f2), None, hip.MIXH, cout, taps, cin)
    wi = torch.empty(cin, taps * cout * 2, device="cuda", dtype=torch.float16)
    hip.call("vlfb_weight_prep", hip.ptr(wg), hip.ptr(sg), None, hip.ptr(wi), hip.MIX_W2I, cout, taps, cin)
    torch.cuda.synchronize()
    assert torch.equal(f3.cpu(), torch.stack(cr.bf16_terms(ws, 3)))
    assert torch.equal(f2.cpu(), torch.stack(cr.f16_pair(ws * hip.MIX_W2_SCALE)))
    rows, _ = cr.w2i_rows((ws * hip.MIX_W2_SCALE).permute(2, 1, 0).reshape(cin, taps * cout), torch.float16)
    assert torch.equal(wi.cpu(), rows)


# ------------------------------------------------------------------------------------------------ what the operands change
# The plan of a descriptor is corrected by the operands of a call in three ways (resolve_for_operands, vlfb_conv_plan.hip).
# Each case asserts the family the descriptor plans, so that a case which has moved to another kernel fails instead of
# quietly testing nothing.
def family_of(d):
    return hip.conv_plan(hip.conv_desc(**d)).split()[0]


def run_raw(d, ops, seed):
    """run `d`, check it against the model, and return the raw bytes of O and O_lo (guard bands included)"""
    c, _ = replay(d, ops, seed=seed)
    return [t.cpu().view(torch.uint8) for t in (c.O, c.Olo) if t is not None]


def assert_runs_the_tiled_kernel(d, ops, family, seed):
    """`d` plans `family`; with these operands the launch must be, bit for bit, the one of algo = TILE128"""
    assert family_of(d) == family, hip.conv_plan(hip.conv_desc(**d))
    tiled = dict(d, algo=hip.ALGO_TILE128)
    assert family_of(tiled) in ("nt", "nt_pair"), hip.conv_plan(hip.conv_desc(**tiled))
    got, ref = run_raw(d, ops, seed), run_raw(tiled, ops, seed)
    assert len(got) == len(ref) and all(torch.equal(a, b) for a, b in zip(got, ref)), "not the launch of algo = TILE128"


def engine_desc(dtype, overrides, pick):
    """first descriptor the dry-run engine of ava_r50_lfb_nl stores for which pick(dict) holds"""
    from test_lowering import plan
    from test_conv_launch_shrink import stored_descs
    _, _, eng = plan("ava_r50_lfb_nl", overrides=overrides, dtype=dtype)
    for _, d in stored_descs(eng):
        dd = cr.desc_dict(d)
        if pick(dd):
            return dd
    raise AssertionError("no such descriptor in the %s engine" % dtype)


def epilogue_ops(d, *ops):
    return tuple(ops) + (("bias",) if d["bias_mode"] else ())


def test_two_term_operands_move_a_streaming_launch_to_the_tiled_kernel():
    d = plain(cr.F16, 256, 64, 256, algo=hip.ALGO_STREAM)
    assert_runs_the_tiled_kernel(d, ("R", "R_lo", "O_lo"), "nt_stream", seed=31)


def test_two_term_operands_move_a_direct_conv_launch_to_the_tiled_kernel():
    from test_conv_launch_shrink import FULL
    d = engine_desc("fp16", FULL, lambda e: e["mode"] == cr.FPROP and (e["kt"], e["kh"], e["kw"]) == (1, 3, 3) and
                    (e["Cs"], e["Cn"]) == (64, 64))
    d = cr.shrink(d, lambda e: hip.conv_plan(hip.conv_desc(**e)))
    assert_runs_the_tiled_kernel(d, epilogue_ops(d, "R", "R_lo", "O_lo"), "conv_rows64", seed=32)


def test_a_rounded_copy_moves_a_skinny_launch_to_the_tiled_kernel():
    d = plain(cr.F16, 33, 512, 512, out_dtype=cr.F32)
    assert_runs_the_tiled_kernel(d, ("O_lo",), "nt_skinny", seed=33)


@pytest.mark.parametrize("dtype,family,ops", [("fp16", "stem_fprop", ("R",)), ("mix", "stem_fprop_pair", ("R", "R_lo", "O_lo"))],
                         ids=["fp16", "two_plane"])
def test_a_residual_moves_the_direct_stem_to_the_tiled_kernel(dtype, family, ops):
    # (the direct stem kernels exist for rows of 112 positions only, i.e. 224-pixel crops: the engine's descriptor at that
    # crop, shrunk in N, T and H as far as it keeps its plan)
    from test_conv_launch_shrink import FULL
    d = engine_desc(dtype, FULL, lambda e: e["mode"] == cr.FPROP and e["pack_w"])
    d = cr.shrink(d, lambda e: hip.conv_plan(hip.conv_desc(**e)))
    assert_runs_the_tiled_kernel(d, epilogue_ops(d, *ops), family, seed=34)


def test_thin_k_prefetch_with_and_without_a_residual():
    d = plain(cr.F16, 300, 64, 128, relu=1)
    words = hip.conv_plan(hip.conv_desc(**d)).split()
    assert words[0] == "nt" and words[-1] == "pre", words
    replay(d, ("R",), seed=35)          # the residual rows are prefetched before the k-loop
    replay(d, (), seed=35)              # nothing to prefetch: the launch must not read R


# ------------------------------------------------------------------------------------------------ two-plane range contract
FP16_MAX = 65504.0


def test_pair_split_range_contract():
    """vlfb_pair_split: values up to the fp16 limit keep 2^-22 relative (2^-24 absolute floor); past it, non-finite"""
    gen = torch.Generator().manual_seed(9)
    x = torch.cat([torch.rand(4096, generator=gen) * FP16_MAX, torch.tensor([FP16_MAX, 65519.0, -65519.0, 1e-9, 3e-7]),
                   torch.tensor([65520.0, -65520.0, 7e4, 1e6, float("inf")]),
                   torch.tensor([2.0 ** -24, 2.0 ** -14, -2.0 ** -15, 1.0 + 2.0 ** -20, -3.0, 0.0])]).float()
    xg = x.cuda()
    out = torch.empty(2 * x.numel(), device="cuda", dtype=torch.float16)
    hip.call("vlfb_pair_split", hip.ptr(xg), hip.ptr(out), x.numel())
    hi, lo = out.cpu().view(2, -1).double()
    v = hi + lo
    ok = x.double().abs() < 65520.0
    err = (v - x.double()).abs()
    assert bool((err[ok] <= torch.clamp(x.double().abs()[ok] * 2.0 ** -22, min=2.0 ** -24)).all())
    assert not bool(torch.isfinite(v[~ok]).any()), "a value past the fp16 limit came back finite"


@pytest.mark.parametrize("form", ["nt_pair", "nt8_pair", "stem_fprop_pair", "split_pair_io"])
def test_two_plane_epilogue_range_contract(form):
    """the epilogues that store two fp16 planes: outputs up to the fp16 limit within the two-plane bound, outputs past it
    non-finite (never a wrong finite number)"""
    if form == "nt_pair":
        d = plain(cr.F16, 300, 256, 136, out_dtype=cr.F16, math=cr.MATH_F16X3, a_pstride=300 * 256, bias_mode=cr.BIAS_COL)
    elif form == "nt8_pair":
        d = plain(cr.F16, 8000, 1024, 256, out_dtype=cr.F16, math=cr.MATH_F16X3, a_pstride=8000 * 1024, bias_mode=cr.BIAS_COL)
    elif form == "split_pair_io":
        d = plain(cr.F32, 300, 256, 136, out_dtype=cr.F16, math=cr.MATH_BF16X3, bias_mode=cr.BIAS_COL)
    else:
        W, wpad = 224, 4
        d = desc(mode=cr.FPROP, dtype=cr.F16, out_dtype=cr.F16, N=1, Tr=2, Hr=4, Wr=112, Ts=2, Hs=8, Ws=W + 2 * wpad, Cs=4,
                 Cn=64, pack_w=8, bias_mode=cr.BIAS_COL, math=cr.MATH_F16X3, a_pstride=2 * 8 * (W + 2 * wpad) * 4,
                 b_pstride=64 * 35 * 32, alpha=1.0 / 1024, kt=5, kh=7, kw=7, st=1, sh=2, sw=2, pt=2, ph=3, pw=3 - wpad,
                 dt=1, dh=1, dw=1)
    plan = hip.conv_plan(hip.conv_desc(**d))
    assert plan.startswith({"nt_pair": "nt_pair", "nt8_pair": "nt8_pair", "stem_fprop_pair": "stem_fprop_pair",
                            "split_pair_io": "nt_split"}[form]), plan
    c = cr.Case(d, ("bias", "O_lo"), seed=11)
    # column biases that put the outputs just under, at and past the fp16 limit
    n = d["Cn"]
    b = torch.linspace(-FP16_MAX * 0.999, FP16_MAX * 0.999, n)
    b[:4] = torch.tensor([7e4, -7e4, 1e6, -1e6])
    c.bias = b.float()
    c._expect()
    c.run(hip)
    got = (c._live_values(c.O.cpu().double(), c.o_live) + c._live_values(c.Olo.cpu().double(), c.lo_live))
    past = c.ref.abs() > 65536.0
    inside = c.ref.abs() < FP16_MAX
    assert bool(past.any()) and bool(inside.any())
    assert not bool(torch.isfinite(got[past]).any()), "%s: an output past the fp16 limit came back finite" % form
    err = (got - c.ref).abs()[inside]
    assert bool((err <= c.bound()[inside]).all()), "%s: worst %.3g" % (form, float((err / c.bound()[inside]).max()))
