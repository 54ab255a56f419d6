"""Conditions on the attention case tables of tests/attn_cases.py, checked on the CPU: an fp32 emulation of the kernels'
formulas stays inside every bound, the tables reach every branch they claim to, the generators produce the rows the GPU
tests rely on, and vlfb_attn_scores_supported agrees with the restated predicate on its boundaries."""
import os
import re

import pytest
import torch

import attn_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ratio(got, want, bound):
    r, _ = ac.worst((got.double() - want).abs(), bound)
    return r


@pytest.mark.parametrize("case", ac.FUSED_CASES, ids=lambda c: c[0] + "-" + ac.case_id(c[1:]))
def test_fp32_emulation_is_within_the_fused_bounds(case):
    kernel, shape = case[0], case[1:]
    for gen in ac.FUSED_GENERATORS:
        for name in ac.FUSED_DTYPES:
            pref, pbound = ac.fused_forward_ref(shape, gen, name)
            p, ds = ac.fused_emulation(shape, gen, name)
            rf = _ratio(p, pref, pbound)
            want, dbound = ac.fused_backward_ref(shape, gen, name, p, shape[3] ** -0.5)
            rb = _ratio(ds, want, dbound)
            print("%s %s %s %s: fp32 emulation at %.3f of the forward bound, %.3f of the backward bound" % (
                kernel, ac.case_id(shape), gen, name, rf, rb))
            assert rf <= 1 and rb <= 1
            assert torch.isfinite(p).all() and torch.isfinite(ds).all()


@pytest.mark.parametrize("shape", ac.ENGINE_SCALE_SHAPES, ids=ac.case_id)
def test_fp32_emulation_is_within_the_backward_bound_at_the_engine_scale(shape):
    scale = shape[3] ** -0.5 * ac.engine_ds_scale(shape[2])
    for gen in ("randn", "hot"):
        p, ds = ac.fused_emulation(shape, gen, "fp16", scale)
        assert torch.isfinite(ds).all(), "fp16 dS overflows at the engine's scale"
        want, bound = ac.fused_backward_ref(shape, gen, "fp16", p, scale)
        r = _ratio(ds, want, bound)
        print("%s %s fp16 x %g: fp32 emulation at %.3f of the backward bound, max |dS| = %.1f" % (
            ac.case_id(shape), gen, ac.engine_ds_scale(shape[2]), r, float(ds.abs().max())))
        assert r <= 1


def test_engine_scale_restatement_matches_the_engine():
    text = open(os.path.join(ROOT, "video-long-term-feature-banks_amd", "lib", "vlfb", "engine.py")).read()
    m = re.search(r"self\.ds_scale = float\((.+?)\) if eng\.btdtype == torch\.float16 else 1\.0", text)
    assert m, "the engine's ds_scale expression moved"
    for L2 in (512, 513, 784, 1024, 1025, 1568):
        assert float(eval(m.group(1), {"L2": L2, "max": max})) == ac.engine_ds_scale(L2)
    assert ac.engine_ds_scale(784) == 16384.0 and ac.engine_ds_scale(1024) == 16384.0


def test_fused_table_reaches_every_branch():
    by = {}
    for kernel, B, L1, L2, Ci in ac.FUSED_CASES:
        assert ac.fused_supported("bf16", L1, L2, Ci) and ac.fused_supported("fp16", L1, L2, Ci)
        assert B * L1 * L2 <= 2 * 200 * 1024 and Ci <= 1024
        by.setdefault(kernel, []).append((B, L1, L2, Ci))
    assert set(by) == {"qrows", "rows7", "rows8"}
    for kernel, shapes in by.items():
        assert any(s[1] % 64 != 0 for s in shapes), kernel
        assert any(s[0] > 1 for s in shapes), kernel
        if kernel != "qrows":
            assert any(s[2] % 16 == 8 for s in shapes), kernel
            assert any(s[3] == 1024 for s in shapes), kernel
        else:
            assert all(s[2:] == (784, 256) for s in shapes)
            assert {64, 72} <= {s[1] for s in shapes} and any(s[1] > 128 and s[1] % 128 == 1 for s in shapes)
    # the dispatch edges: both sides of FN = 7 / 8, the model's key count on the rows kernel, both ends of L2 and Ci
    assert {s[2] for s in by["rows7"]} >= {512, 784, 896} and {s[2] for s in by["rows8"]} >= {904, 1016, 1024}
    assert {s[3] for s in ac.FUSED_SHAPES} >= {64, 128, 1024}
    assert any(s[3] // 32 == 6 for s in by["rows7"]), "an even number of k-steps that is no multiple of 4"
    # Ci = 1024: the query tile is larger than the FN = 7 probability tile, and 1 KiB smaller than the FN = 8 one
    q7, t7 = ac.fused_lds(784, 1024)
    q8, t8 = ac.fused_lds(1024, 1024)
    assert (q7, t7) == (131072, 115712) and (q8, t8) == (131072, 132096) and t8 - q8 == 1024
    for shape in ac.ENGINE_SCALE_SHAPES + ac.COMPOSED_SHAPES:
        assert shape in ac.FUSED_SHAPES
    assert {ac.fused_kernel(s[2], s[3]) for s in ac.COMPOSED_SHAPES} == {"qrows", "rows7", "rows8"}


def test_fbo_table_reaches_every_branch():
    for name in ac.DTYPES:
        mine = [c for c in ac.FBO_CASES if c[1] == name]
        assert {c[0] for c in mine} == {"chip", "row"}, name
        for path in ("chip", "row"):
            assert any(c[0] == path and c[5] > c[4] for c in mine), (name, path, "ld > D")
        assert any(c[0] == "chip" and c[3] % 8 != 0 for c in mine), name
        assert any(c[0] == "chip" and c[3] < 32 for c in mine) and any(c[3] == 1 for c in mine)
        assert any(c[2] == 1 for c in mine)
        for path, _, R, K, D, ld in mine:
            v = ac.FBO_VEC[name]
            assert D % v == 0 and ld % v == 0 and ld >= D and R * K * ld <= 7 * 300 * 576     # what the backward requires
    own = ac.SHARED_OWNER
    assert list(own) != sorted(own) and set(own) == set(range(ac.SHARED_NB)) and min(own.count(b) for b in set(own)) == 1
    for name in ac.DTYPES:
        assert {ac.fbo_path(name, s[2], s[3]) for s in ac.SHARED_SHAPES} == {"chip", "row"}
    assert all(s[3] > s[2] and s[0] == len(own) for s in ac.SHARED_SHAPES)


@pytest.mark.parametrize("case", ac.FUSED_CASES, ids=lambda c: c[0] + "-" + ac.case_id(c[1:]))
def test_generators_give_the_rows_they_claim(case):
    shape = case[1:]
    B, L1, L2, Ci = shape
    for name in ac.FUSED_DTYPES:
        p, _ = ac.fused_forward_ref(shape, "hot", name)
        assert float(p.max()) > 0.99 and float(p.min()) < 2.0 ** -24
        p, _ = ac.fused_forward_ref(shape, "flat", name)
        assert torch.equal(p, torch.full_like(p, 1.0 / L2))
        p, _ = ac.fused_forward_ref(shape, "edge_peak", name)
        keys = torch.tensor([ac.edge_key_of_row(r, L2, Ci) for r in range(L1)])
        mass = p[:, torch.arange(L1), keys]
        assert float(mass.min()) >= 0.9
        assert set(keys.tolist()) == set(ac.edge_keys(L2, Ci)), "every listed key is some row's peak"
        theta, phi, _, _ = ac.fused_inputs(shape, "edge_peak", name)
        logits = Ci ** -0.5 * torch.bmm(theta.double(), phi.double().transpose(1, 2))
        assert float(logits.abs().max()) >= 30
    fn = 8 if L2 > 896 else 7
    assert ac.edge_keys(L2, Ci)[:5] == [0, 15, 16, 16 * fn - 1, 16 * fn] and ac.edge_keys(L2, Ci)[-1] == L2 - 1


@pytest.mark.parametrize("case", ac.FBO_CASES, ids=lambda c: "%s-%s-%s" % (c[0], c[1], ac.case_id(c[2:])))
def test_fp32_emulation_is_within_the_fbo_bounds(case):
    path, name, shape = case[0], case[1], case[2:]
    for gen in ac.FBO_GENERATORS:
        p, pb, t, tb = ac.fbo_forward_ref(shape, gen, name)
        emu = ac.fbo_emulation(shape, gen, name)
        ratios = {"p": _ratio(emu["p"], p, pb), "t": _ratio(emu["t"], t, tb)}
        for key, (want, bound) in ac.fbo_backward_ref(shape, gen, name, emu["p"]).items():
            ratios[key] = _ratio(emu[key], want, bound)
        print("%s %s %s %s: fp32 emulation at %s of the bounds" % (
            path, name, ac.case_id(shape), gen, " ".join("%s %.3f" % kv for kv in ratios.items())))
        assert max(ratios.values()) <= 1, ratios


def test_supported_predicate_on_its_boundaries():
    from vlfb import hip
    if not os.path.exists(hip.LIB_PATH):
        pytest.skip("libvlfb_hip.so not built (run __graft_entry__.build())")
    sup = hip.lib().vlfb_attn_scores_supported
    codes = {"bf16": hip.BF16, "fp16": hip.F16, "fp32": hip.F32}
    for l2 in (504, 1032, 516):
        assert sup(hip.BF16, 64, l2, 256) == 0
    for ci in (0, 32, 96, 1088):
        assert sup(hip.F16, 64, 784, ci) == 0
    assert sup(hip.BF16, 63, 784, 256) == 0 and sup(hip.BF16, 64, 784, 256) != 0
    assert sup(hip.BF16, 1 << 20, 784, 1024) == 0 and sup(hip.BF16, (1 << 20) - 1, 784, 1024) != 0     # l1 * ci = 2^30
    assert sup(hip.BF16, 1 << 20, 1024, 64) == 0 and sup(hip.BF16, (1 << 20) - 1, 1024, 64) != 0      # l1 * l2 = 2^30
    assert sup(hip.F32, 3136, 784, 256) == 0
    for l2 in (512, 520, 1024):
        for ci in (64, 1024):
            assert sup(hip.F16, 64, l2, ci) & hip.ATTN_CAN_RUN
    for kernel, B, L1, L2, Ci in ac.FUSED_CASES:
        for name in ac.FUSED_DTYPES:
            assert sup(codes[name], L1, L2, Ci) & hip.ATTN_CAN_RUN
    # the restated predicate and the library agree on a grid around every limit
    for name, code in codes.items():
        for l1 in (1, 63, 64, 65, 3136):
            for l2 in (496, 504, 512, 516, 520, 784, 896, 904, 1016, 1024, 1028, 1032):
                for ci in (0, 32, 64, 96, 128, 256, 960, 1024, 1088):
                    assert bool(sup(code, l1, l2, ci)) == ac.fused_supported(name, l1, l2, ci), (name, l1, l2, ci)
    # measured-faster flags: forward at (784, 256) and (1024, 256), backward at (1024, 256) only
    for code in (hip.BF16, hip.F16):
        for l2 in range(512, 1025, 8):
            for ci in range(64, 1025, 64):
                r = sup(code, 3136, l2, ci)
                assert bool(r & hip.ATTN_FWD_FASTER) == ((l2, ci) in ((784, 256), (1024, 256))), (l2, ci)
                assert bool(r & hip.ATTN_BWD_FASTER) == ((l2, ci) == (1024, 256)), (l2, ci)
