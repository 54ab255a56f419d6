"""The WGRAD edge table: descriptors for conv_desc_ref.Case that pin, per entry, the kernel family, the tile, the split
count and the size of the last split, over every WGRAD family of the library (no GPU, no torch.cuda, no library: plain
dicts and integer arithmetic; tests/test_wgrad_cases_host.py proves the conditions below with the built library on the
CPU, tests/test_wgrad_gpu.py runs the table).

An entry is (fields, plan, ops, last, types):
  fields  the descriptor fields that differ from the defaults of vlfb_conv_desc_init (DEFAULTS; "same" for out_dtype =
          the operand type), without the element type;
  plan    the exact string vlfb_conv_plan_describe must give, written for bf16 ("bf16" becomes "f16" in the fp16 run);
  ops     the optional operands of the launch ("rowscale", "dbias");
  last    for a launch with more than one split: the number of units the last split holds -- row positions for the tiled
          families, output rows (n, t, h) for the whole-row families -- else None;
  types   the element types the entry runs in: both 16-bit types, "f32" (exact fp32 `tn`), or "f32x3" (fp32 storage with
          MATH_BF16X3: `tn_split`, and with two bf16 term planes per operand `tn_tr_planes`).
Operands are uniform(-1, 1), as Case generates them.

What the table pins (test_table_covers_*):
  * every family name of {tn, tn_tr, tn8, tn_split, tn_tr_planes, wgrad_rows, wgrad_rows_fat, stem_wgrad};
  * every tile shape launch_tn (128x128, 64x256, 64x128, 128x64, 64x64) and launch_tn_tr_as (128x128, 64x128, 128x64, 64x64)
    instantiate, with Cn and K one 16-byte chunk past a tile (136, 72), below one tile (8, 40), and not a multiple of it;
  * the split decode in both grid forms: blockIdx.y (splits % 8 != 0) and the 1-D XCD-interleaved grid (splits % 8 == 0),
    with a last split of one position (M = 64 s - 63) and of a whole k-tile (M = 64 s);
  * wgrad_reduce_kernel in its three instances (G = 1 below 8 splits, 4 from 8, 16 from 32), with split counts below G,
    on both sides of the 4 G of its unrolled loop, and with a tail behind it;
  * one, two and three output rows per workgroup of each whole-row kernel (`whole_row_splits`: more than 256 rows), with
    a ragged last workgroup and the h -> t and t -> n wraps inside one workgroup's rows;
  * both bias-gradient routes: fused into tn_tr (direct, and with splits through the extra blocks of the reduce) and the
    column-sum pass behind every other family, behind an accumulate and behind a batched launch;
  * scalar-store output rows (ldo & 3 != 0), strided lda / ldp / ldo, gaps between batch elements, 16-bit outputs.

Not covered, on purpose: the 32-bit extents `kend * ldp * 2` of the buffer descriptors (an index past 2^31 needs operands
of GiB; no small shape reaches it).

Teeth (test_one_dropped_position_is_past_the_bound): for every entry with splits > 1, the fp64 reference minus ONE
position's contribution alpha * rowscale * P[m]^T A[src(m)] -- m the last position of the last split, and the first
position of split 1 -- must fail Case._compare, with at least half of the outputs that position contributes to past
Case.bound().  On plain rows a position contributes to every output.  On a gathered launch a tap that reads padding at m
contributes exactly zero to its columns (the corner of a 3x3 window keeps 4 taps of 9), so the share is taken over the
columns whose tap reads data at m; there must be some.  This is a condition on the inputs, not a tolerance.
Two entries cannot meet it with one position and drop one output ROW instead (ROW_TEETH): the two sides of the planner's
row-width rule at (N, T, H) = (1, 1, 257), W = 56 and W = 64, sum M = 14392 / 16448 positions, where the accumulation term
of the bound, 2 * 2^-24 * (M / 16 + 64) * sum |p| |a| ~ 0.4 - 0.5, is above what one position of uniform(-1, 1) operands
contributes (|p| |a| rowscale: median 0.19).  A row of W positions is the unit the whole-row kernel loops over and one
k-tile of the tiled kernel; the same loop is held to one position by the W = 8 entries.
"""
import collections
import zlib

F32, BF16, F16 = 0, 1, 2
WGRAD = 2
MATH_BF16X3 = 3
ALGO_PIPE256 = 2
SAME = "same"

DEFAULTS = dict(mode=0, dtype=BF16, out_dtype=BF16, N=1, Tr=1, Hr=1, Wr=1, Ts=1, Hs=1, Ws=1, Cs=0, kt=1, kh=1, kw=1, st=1,
                sh=1, sw=1, pt=0, ph=0, pw=0, dt=1, dh=1, dw=1, pack_w=0, Cn=0, lda=0, ldb=0, ldo=0, ldr=0, ldp=0, batch=1,
                a_bstride=0, b_bstride=0, o_bstride=0, r_bstride=0, p_bstride=0, alpha=1.0, relu=0, bias_mode=0,
                accumulate=0, splits=0, algo=0, math=0, b_pstride=0, a_planes=0, p_planes=0, o_planes=0, wgrad_bias=0,
                a_pstride=0, p_pstride=0, o_pstride=0)

T16 = ("bf16", "f16")
TYPES = {"bf16": BF16, "f16": F16, "f32": F32, "f32x3": F32}
WHOLE_ROW = ("wgrad_rows", "wgrad_rows_fat", "stem_wgrad")
FAMILIES = ("tn", "tn_tr", "tn8", "tn_split", "tn_tr_planes") + WHOLE_ROW

Entry = collections.namedtuple("Entry", "fields plan ops last types")
CASES = collections.OrderedDict()


def add(name, fields, plan, ops=(), last=None, types=T16):
    assert name not in CASES, name
    CASES[name] = Entry(dict(fields), plan, tuple(ops), last, tuple(types))


def rows(Cs, Cn, M, **kw):
    """plain rows: N = Tr = Hr = 1, Wr = Ws = M, fp32 output"""
    return dict(dict(mode=WGRAD, out_dtype=F32, Wr=M, Ws=M, Cs=Cs, Cn=Cn), **kw)


def conv(N, T, H, W, Cs, Cn, k, p, s=(1, 1, 1), dil=(1, 1, 1), **kw):
    """gathered: rows = the conv's output positions, source = its input [N, T, H, W, Cs]"""
    o = [(e + 2 * pp - dd * (kk - 1) - 1) // ss + 1 for e, pp, dd, kk, ss in zip((T, H, W), p, dil, k, s)]
    return dict(dict(mode=WGRAD, out_dtype=F32, N=N, Tr=o[0], Hr=o[1], Wr=o[2], Ts=T, Hs=H, Ws=W, Cs=Cs, Cn=Cn, kt=k[0],
                     kh=k[1], kw=k[2], pt=p[0], ph=p[1], pw=p[2], st=s[0], sh=s[1], sw=s[2], dt=dil[0], dh=dil[1],
                     dw=dil[2]), **kw)


def stem(N, T, H, W, **kw):
    """the packed stem: 5x7x7, stride (1, 2, 2), 4 channels per pixel, kw padded to 8, source W-padded by 4 on each side"""
    return dict(dict(mode=WGRAD, out_dtype=F32, N=N, Tr=T, Hr=H // 2, Wr=W // 2, Ts=T, Hs=H, Ws=W + 8, Cs=4, Cn=64, kt=5,
                     kh=7, kw=7, st=1, sh=2, sw=2, pt=2, ph=3, pw=3 - 4, pack_w=8), **kw)


RS = ("rowscale",)
RS_DB = ("rowscale", "dbias")

# ------------------------------------------------------------------------------------------------ tn_tr, plain rows
for Cs, Cn, tile in ((128, 128, "128x128"), (64, 64, "64x64"), (128, 64, "64x128"), (64, 128, "128x64"), (72, 136, "128x128"),
                     (200, 40, "64x128"), (8, 8, "64x64")):
    add("tr_tile_%dx%d" % (Cs, Cn), rows(Cs, Cn, 321), "tn_tr bf16 %s splits=1" % tile)
for M in (1, 5, 63, 64, 65):
    add("tr_M%d" % M, rows(72, 136, M), "tn_tr bf16 128x128 splits=1", RS)
for s in (2, 3, 7, 8, 9, 16, 31, 32, 33, 40, 72):
    add("tr_split%d_last1" % s, rows(128, 128, 64 * s - 63, splits=s), "tn_tr bf16 128x128 splits=%d" % s, (), 1)
    add("tr_split%d_full" % s, rows(72, 136, 64 * s, splits=s), "tn_tr bf16 128x128 splits=%d" % s, RS, 64)
add("tr_split8_lowered", rows(72, 136, 321, splits=8), "tn_tr bf16 128x128 splits=6", RS, 1)
add("tr_alpha_rowscale", rows(72, 136, 321, alpha=0.5), "tn_tr bf16 128x128 splits=1", RS)
add("tr_accumulate", rows(72, 136, 321, accumulate=1, alpha=0.5), "tn_tr bf16 128x128 splits=1", RS)
add("tr_accumulate_split3", rows(72, 136, 321, accumulate=1, alpha=0.5, splits=3), "tn_tr bf16 128x128 splits=3", RS, 65)
add("tr_out16", rows(72, 136, 321, out_dtype=SAME), "tn_tr bf16 128x128 splits=1", RS)
add("tr_out16_split2_accumulate", rows(72, 136, 321, out_dtype=SAME, splits=2, accumulate=1), "tn_tr bf16 128x128 splits=2",
    RS, 129)
add("tr_strided", rows(72, 136, 200, lda=80, ldp=144, ldo=80), "tn_tr bf16 128x128 splits=1", RS)
add("tr_scalar_rows", rows(72, 136, 200, ldo=74), "tn_tr bf16 128x128 splits=1", RS)
add("tr_batch3_gaps", rows(72, 136, 200, batch=3, a_bstride=200 * 72 + 64, p_bstride=200 * 136 + 64, o_bstride=136 * 72 + 16),
    "tn_tr bf16 128x128 splits=1", RS)
add("tr_bias_fused", rows(128, 136, 321, wgrad_bias=1), "tn_tr bf16 128x128 splits=1", RS_DB)
add("tr_bias_fused_split3", rows(128, 136, 321, wgrad_bias=1, splits=3), "tn_tr bf16 128x128 splits=3", RS_DB, 65)
add("tr_bias_fused_split8_lowered", rows(128, 136, 321, wgrad_bias=1, splits=8), "tn_tr bf16 128x128 splits=6", RS_DB, 1)
add("tr_bias_accumulate", rows(128, 136, 321, wgrad_bias=1, accumulate=1), "tn_tr bf16 128x128 splits=1", RS_DB)
add("tr_bias_batch2", rows(128, 136, 321, wgrad_bias=1, batch=2, a_bstride=321 * 128, p_bstride=321 * 136,
                           o_bstride=136 * 128), "tn_tr bf16 128x128 splits=1", RS_DB)

# ------------------------------------------------------------------------------------------------ tn_tr, gathered
add("tr_conv333", conv(1, 3, 7, 9, 64, 128, (3, 3, 3), (1, 1, 1)), "tn_tr bf16 128x128 splits=1", RS)
add("tr_conv133_stride2", conv(1, 3, 9, 11, 64, 136, (1, 3, 3), (0, 1, 1), s=(1, 2, 2)), "tn_tr bf16 128x128 splits=1", RS)
add("tr_conv133_dil2", conv(1, 2, 9, 9, 64, 64, (1, 3, 3), (0, 2, 2), dil=(1, 2, 2)), "tn_tr bf16 64x128 splits=1", RS)
add("tr_conv311_split", conv(2, 4, 5, 5, 128, 64, (3, 1, 1), (1, 0, 0), splits=5), "tn_tr bf16 64x128 splits=4", RS, 8)

# ------------------------------------------------------------------------------------------------ tn, 16-bit (Cn % 8 != 0)
for Cn, ldp in ((12, 16), (20, 24), (60, 64)):
    for Cs, tile in ((64, "64x64"), (256, "64x256"), (320, "64x256")):
        add("tn16_%dx%d" % (Cs, Cn), rows(Cs, Cn, 321, ldp=ldp), "tn bf16 %s splits=1" % tile)
add("tn16_256x20_split3", rows(256, 20, 321, ldp=24, splits=3), "tn bf16 64x256 splits=3", RS, 65)

# ------------------------------------------------------------------------------------------------ tn, fp32
for Cs, Cn, tile in ((128, 128, "128x128"), (64, 64, "64x64"), (68, 132, "128x128"), (256, 64, "64x128"), (4, 4, "64x64"),
                     (36, 100, "128x64")):
    add("tn32_%dx%d" % (Cs, Cn), rows(Cs, Cn, 321), "tn f32 %s splits=1" % tile, RS, types=("f32",))
    add("tn32_%dx%d_split3" % (Cs, Cn), rows(Cs, Cn, 321, splits=3), "tn f32 %s splits=3" % tile, RS, 65, types=("f32",))
add("tn32_bias", rows(68, 132, 321, wgrad_bias=1), "tn f32 128x128 splits=1", RS_DB, types=("f32",))
add("tn32_bias_split3", rows(68, 132, 321, wgrad_bias=1, splits=3), "tn f32 128x128 splits=3", RS_DB, 65, types=("f32",))


# ------------------------------------------------------------------------------------------------ tn_split, tn_tr_planes
def planes(Cs, Cn, M, **kw):
    r8 = lambda n: -(-n // 8) * 8
    return rows(Cs, Cn, M, math=MATH_BF16X3, a_planes=2, p_planes=2, a_pstride=r8(M * Cs), p_pstride=r8(M * Cn), **kw)


for fam, make in (("tn_split", lambda Cs, Cn, M, **kw: rows(Cs, Cn, M, math=MATH_BF16X3, **kw)), ("tn_tr_planes", planes)):
    for Cs, Cn, tile in ((128, 128, "128x128"), (64, 64, "64x64"), (72, 136, "128x128"), (256, 40, "64x128")):
        add("%s_%dx%d" % (fam, Cs, Cn), make(Cs, Cn, 321), "%s f32x3 %s splits=1" % (fam, tile), RS, types=("f32x3",))
        add("%s_%dx%d_split3" % (fam, Cs, Cn), make(Cs, Cn, 321, splits=3), "%s f32x3 %s splits=3" % (fam, tile), RS, 65,
            types=("f32x3",))
    for M in (31, 32, 33):          # the k-tile of these kernels is 32 positions
        add("%s_M%d" % (fam, M), make(72, 136, M), "%s f32x3 128x128 splits=1" % fam, RS, types=("f32x3",))
add("tn_split_bias", rows(72, 136, 321, math=MATH_BF16X3, wgrad_bias=1), "tn_split f32x3 128x128 splits=1", RS_DB,
    types=("f32x3",))

# ------------------------------------------------------------------------------------------------ tn8 (256 x 256)
for Cs, Cn in ((128, 128), (136, 200), (264, 520)):
    add("tn8_%dx%d" % (Cs, Cn), rows(Cs, Cn, 700, algo=ALGO_PIPE256), "tn8 bf16 256x256 splits=1", RS)
    add("tn8_%dx%d_split3" % (Cs, Cn), rows(Cs, Cn, 700, algo=ALGO_PIPE256, splits=3), "tn8 bf16 256x256 splits=3", RS, 188)
add("tn8_M1", rows(128, 128, 1, algo=ALGO_PIPE256), "tn8 bf16 256x256 splits=1", RS, types=("f16",))
add("tn8_bias", rows(256, 256, 700, algo=ALGO_PIPE256, wgrad_bias=1), "tn8 bf16 256x256 splits=1", RS_DB)
add("tn8_auto", rows(2048, 512, 300), "tn8 bf16 256x256 splits=1", RS)

# ------------------------------------------------------------------------------------------------ whole-row kernels
# (N, T, H) -> (splits, rows of the last workgroup): two rows per workgroup with a last one of one; the h -> t wrap inside a
# workgroup's pair; three rows each; the t -> n wrap inside a workgroup; and one row per workgroup
ROW_SHAPES = (((1, 1, 257), 129, 1), ((1, 2, 129), 129, 2), ((1, 3, 171), 171, 3), ((2, 2, 160), 214, 1), ((1, 2, 5), 10, 1))
for (N, T, H), sp, last in ROW_SHAPES:
    tag = "%d_%d_%d" % (N, T, H)
    add("rows_133_" + tag, conv(N, T, H, 8, 64, 64, (1, 3, 3), (0, 1, 1)), "wgrad_rows bf16 64x128 splits=%d" % sp, RS, last)
    add("rows_311_" + tag, conv(N, T, H, 8, 64, 64, (3, 1, 1), (1, 0, 0)), "wgrad_rows bf16 64x128 splits=%d" % sp, RS, last)
    add("fat_311_" + tag, conv(N, T, H, 8, 256, 64, (3, 1, 1), (1, 0, 0)), "wgrad_rows_fat bf16 64x128 splits=%d" % sp, RS,
        last)
add("rows_133_W56", conv(1, 1, 257, 56, 64, 64, (1, 3, 3), (0, 1, 1)), "wgrad_rows bf16 64x128 splits=129", RS, 1)
add("rows_133_W64_is_tn_tr", conv(1, 1, 257, 64, 64, 64, (1, 3, 3), (0, 1, 1)), "tn_tr bf16 64x128 splits=29", RS, 320)
add("rows_133_bias_W16", conv(1, 1, 257, 16, 64, 64, (1, 3, 3), (0, 1, 1), wgrad_bias=1), "wgrad_rows bf16 64x128 splits=129",
    RS_DB, 1)
ROW_TEETH = ("rows_133_W56", "rows_133_W64_is_tn_tr")       # see "Teeth" above
for (N, T, H, W), sp, last in (((1, 1, 4, 16), 2, 1), ((1, 3, 172, 16), 129, 2), ((1, 2, 260, 32), 130, 2),
                               ((1, 2, 514, 16), 172, 1)):
    add("stem_%d_%d_%d_%d" % (N, T, H, W), stem(N, T, H, W), "stem_wgrad bf16 64x128 splits=%d" % sp, RS, last)

# ------------------------------------------------------------------------------------------------ refusals
# (fields, text the library's error must contain); each leaves the output untouched
REFUSALS = collections.OrderedDict([
    ("split_batched", (rows(128, 136, 321, batch=2, splits=2, a_bstride=321 * 128, p_bstride=321 * 136, o_bstride=136 * 128),
                       "split WGRAD cannot be batched")),
    ("split_strided_output", (rows(128, 136, 321, splits=2, ldo=136), "split WGRAD needs a dense output (ldo == K)")),
    ("Cn12_default_ldp", (rows(64, 12, 321), "leading dimensions must keep 16-byte alignment")),
    ("gathered_Cs72", (conv(1, 3, 7, 9, 72, 128, (3, 3, 3), (1, 1, 1)), "power-of-two chunk count")),
    ("pipe256_Cn64", (rows(128, 64, 321, algo=ALGO_PIPE256), "algo = PIPE256 WGRAD needs")),
])


# ------------------------------------------------------------------------------------------------ access
def full(fields, tname):
    """every field of the descriptor, for element type `tname`"""
    d = dict(DEFAULTS)
    d.update(fields)
    d["dtype"] = TYPES[tname]
    if d["out_dtype"] == SAME:
        d["out_dtype"] = d["dtype"]
    return d


def plan_of(entry, tname):
    return entry.plan.replace(" bf16 ", " %s " % tname) if tname in T16 else entry.plan


def case_ids():
    """[(name, type)] of the table"""
    return [(n, t) for n, e in CASES.items() for t in e.types]


def seed_of(name, tname):
    return zlib.crc32(("%s/%s" % (name, tname)).encode()) & 0x7fffffff


def family_of(plan):
    return plan.split()[0]


def splits_of(plan):
    return int(plan.rsplit("splits=", 1)[1])


def split_layout(d, family, planned=0):
    """(splits, units per split, units of the last split, row positions per unit) of descriptor `d` run by `family`
    (`planned`: the split count of the plan, for a descriptor that leaves the count to the library), from the planner's rule: tiled families cut the M row positions into pieces of whole k-tiles (64 positions of 16-bit
    operands, 32 of fp32 operands and of term planes); whole-row families give each of up to 256 workgroups the same number
    of consecutive output rows"""
    M = d["N"] * d["Tr"] * d["Hr"] * d["Wr"]
    if family in WHOLE_ROW:
        tiles = d["N"] * d["Tr"] * d["Hr"]
        tpw = -(-tiles // min(tiles, 256))
        sp = -(-tiles // tpw)
        return sp, tpw, tiles - (sp - 1) * tpw, d["Wr"]
    req = d["splits"] if d["splits"] > 0 else planned
    assert req >= 1, "a tiled entry states its split count, or the caller passes the planned one"
    bk = 64 if d["dtype"] != F32 else 32
    kper = -(-(-(-M // req)) // bk) * bk
    sp = -(-M // kper)
    return sp, kper, M - (sp - 1) * kper, 1


def grid_form(splits):
    """"1d": the XCD-interleaved split decode of the tiled kernels; "2d": blockIdx.y"""
    return "1d" if splits > 1 and splits % 8 == 0 else "2d"


def reduce_group(splits):
    """G of the wgrad_reduce_kernel instance that folds `splits` slabs"""
    return 16 if splits >= 32 else 4 if splits >= 8 else 1
