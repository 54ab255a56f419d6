"""SpatialBN on the `mix` dtype: vlfb_bn_fwd_mix / vlfb_bn_bwd_mix against fp64 torch (two-plane and fp32 values, fp16 /
two-term fp16 / fp32 gradients, the fused residual + ReLU, canonical pairs, bit-identical reruns), the whole BN graph of
ava_r50_lfb_nl on `mix` against the fp64 oracle, and the driver level (recorded-step replay, shared test net, PreciseBN)."""
import collections

import numpy as np
import pytest
import torch

from gpu_util import dev, rel_err

pytestmark = pytest.mark.gpu

BN = ["MODEL.USE_AFFINE", False, "NONLOCAL.USE_BN", True, "NONLOCAL.USE_AFFINE", False, "MODEL.DILATIONS_AFTER_CONV5", False]


def _pair(t):
    """fp32 [rows][C] -> the two fp16 planes [2][rows * C] (hi = fp16(v), lo = fp16(v - hi)), as vlfb_pair_split writes them"""
    hi = t.half()
    lo = (t - hi.float()).half()
    return torch.cat([hi.reshape(-1), lo.reshape(-1)])


class _Values(object):
    """a value tensor in one of the two formats of the entry points"""

    def __init__(self, hip, pair, rows, C):
        self.pair, self.rows, self.C, self.n = pair, rows, C, rows * C
        self.xf = hip.F16PAIR if pair else hip.F32

    def put(self, t):
        return (_pair(t) if self.pair else t.reshape(-1).clone()).to(dev())

    def empty(self):
        return torch.full((2 * self.n if self.pair else self.n,), float("nan"), device=dev(), dtype=torch.float16 if self.pair else torch.float32)

    def value(self, T):
        """fp64 [rows][C] of what the tensor holds"""
        T = T.cpu()
        v = T[:self.n].double() + T[self.n:].double() if self.pair else T.double()
        return v.reshape(self.rows, self.C)

    def check_canonical(self, T, relu):
        if not self.pair:
            return
        hi, lo = T[:self.n], T[self.n:]
        assert torch.equal((hi.float() + lo.float()).half(), hi)
        if relu:
            assert bool((hi >= 0).all()) and bool((lo[hi == 0] == 0).all())


@pytest.mark.parametrize("gname", ["g16", "g32"])
@pytest.mark.parametrize("pair", [True, False], ids=["pair", "f32"])
@pytest.mark.parametrize("rows,C,shift", [(4097, 64, 0.0), (300, 256, 0.0), (20000, 8, 50.0), (1, 16, 0.0)])
def test_bn_mix_kernels_against_fp64(pair, gname, rows, C, shift):
    """the cases of test_bn_kernels_against_fp64 (a ragged last slab, several channel blocks, a mean 100x the spread on one
    chunk lane, a single row) and its bars: forward and fp32 dx at fp32's 3e-6, fp16 dx at fp16's 8e-4 (x40 where the bar of
    that test carries the factor for the shifted case), the statistics and parameter gradients at their bars"""
    from vlfb import hip
    lib = hip.lib()
    V = _Values(hip, pair, rows, C)
    gt = hip.F16 if gname == "g16" else hip.F32
    gen = torch.Generator().manual_seed(rows + C)
    x = torch.randn(rows, C, generator=gen) * 0.5 + shift
    res = torch.randn(rows, C, generator=gen)
    dy32 = torch.randn(rows, C, generator=gen)
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.1
    rm0, rv0 = torch.randn(C, generator=gen) * 0.1, torch.rand(C, generator=gen) + 0.5
    eps, mom = 1e-5, 0.9
    X, R = V.put(x), V.put(res)
    G, Bt = gamma.to(dev()), beta.to(dev())
    nbytes = lib.vlfb_bn_mix_workspace_bytes(V.xf, rows, C)
    assert nbytes > 0 and nbytes % 4 == 0
    ws = torch.empty(nbytes // 4, device=dev())
    tail = lambda: (hip.ptr(ws), ws.numel() * 4, V.xf, rows, C, eps, mom)

    def forward(residual, relu, is_test, rm, rv):
        Y = V.empty()
        save = torch.full((2 * C,), float("nan"), device=dev())
        hip.call("vlfb_bn_fwd_mix", hip.ptr(X), hip.ptr(Y), hip.ptr(residual), hip.ptr(G), hip.ptr(Bt), hip.ptr(rm), hip.ptr(rv),
                 None if is_test else hip.ptr(save), None if is_test else hip.ptr(save) + 4 * C, *tail(), int(is_test), int(relu))
        return Y, save

    # ---- training forward: moments, saved and running statistics, y
    RM, RV = rm0.clone().to(dev()), rv0.clone().to(dev())
    Y, save = forward(None, False, False, RM, RV)
    xd = V.value(X).requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    mu = xd.mean(0)
    var = ((xd - mu) ** 2).mean(0)
    yd = (xd - mu) / torch.sqrt(var + eps) * gd + bd
    f32tol = 3e-6 * (40 if shift else 1)
    V.check_canonical(Y, False)
    if rows > 1:
        assert rel_err(V.value(Y) - beta.double(), yd - bd) < f32tol
    spread = float(torch.sqrt(var + eps).detach().norm()) + 0.2 * float(mu.detach().norm())
    assert float((save[:C].cpu().double() - mu).norm()) < 1e-6 * spread
    assert rel_err(save[C:], 1.0 / torch.sqrt(var + eps)) < (2e-5 if shift else 2e-6)
    assert float((RM.cpu().double() - (mom * rm0.double() + (1 - mom) * mu)).norm()) < 1e-6 * (spread + float(rm0.norm()))
    assert rel_err(RV, mom * rv0.double() + (1 - mom) * var * (rows / max(rows - 1, 1))) < 1e-5
    # ... the same launch again: the same bits
    RMb, RVb = rm0.clone().to(dev()), rv0.clone().to(dev())
    Yb, saveb = forward(None, False, False, RMb, RVb)
    assert torch.equal(Y, Yb) and torch.equal(save, saveb) and torch.equal(RM, RMb) and torch.equal(RV, RVb)

    # ---- residual + ReLU in the apply pass
    RM2, RV2 = rm0.clone().to(dev()), rv0.clone().to(dev())
    Y2, save2 = forward(R, True, False, RM2, RV2)
    want2 = torch.relu(yd.detach() + V.value(R))
    V.check_canonical(Y2, True)
    assert torch.equal(save2, save) and torch.equal(RM2, RM) and torch.equal(RV2, RV)
    if rows > 1:
        assert rel_err(V.value(Y2), want2) < f32tol
        assert bool((V.value(Y2) == 0).any()) and bool((V.value(Y2) > 0).any())
    Y2b, _ = forward(R, True, False, rm0.clone().to(dev()), rv0.clone().to(dev()))
    assert torch.equal(Y2, Y2b)
    Y3, _ = forward(R, False, False, rm0.clone().to(dev()), rv0.clone().to(dev()))          # (a Sum without a ReLU)
    V.check_canonical(Y3, False)
    if rows > 1:
        assert rel_err(V.value(Y3), yd.detach() + V.value(R)) < f32tol

    # ---- backward
    gdt = torch.float16 if gt == hip.F16 else torch.float32
    dy = dy32.to(gdt)
    DY = dy.reshape(-1).to(dev())
    btail = lambda: (hip.ptr(ws), ws.numel() * 4, V.xf, gt, rows, C)

    def backward(dy_lo, want_dx, scale):
        DX = torch.full((rows * C,), float("nan"), device=dev(), dtype=gdt) if want_dx else None
        dG, dB = torch.full((C,), float("nan"), device=dev()), torch.full((C,), float("nan"), device=dev())
        hip.call("vlfb_bn_bwd_mix", hip.ptr(DY), hip.ptr(dy_lo), hip.ptr(X), hip.ptr(G), hip.ptr(save), hip.ptr(save) + 4 * C,
                 hip.ptr(DX), hip.ptr(dG), hip.ptr(dB), *btail(), scale)
        return DX, dG, dB

    dxtol = (8e-4 * (40 if shift else 1)) if gt == hip.F16 else 3e-6
    DX, dG, dB = backward(None, True, 1.0)
    gx, gg, gb = torch.autograd.grad(yd, (xd, gd, bd), dy.double(), retain_graph=True)
    err_dx = rel_err(DX.float().reshape(rows, C), gx) if rows > 1 else 0.0
    print("\n[bn_mix %s %s rows %d C %d] dx %.2e dgamma %.2e dbeta %.2e" % ("pair" if pair else "f32", gname, rows, C, err_dx,
                                                                          rel_err(dG, gg), rel_err(dB, gb)))
    assert rel_err(dB, gb) < 1e-5 and rel_err(dG, gg) < (5e-4 if shift else 2e-5)
    assert err_dx < dxtol
    DXb, dGb, dBb = backward(None, True, 1.0)
    assert torch.equal(DX, DXb) and torch.equal(dG, dGb) and torch.equal(dB, dBb)
    # parameter gradients only, scaled: exactly half
    _, dG2, dB2 = backward(None, False, 0.5)
    assert torch.equal(dG2, dG * 0.5) and torch.equal(dB2, dB * 0.5)
    if gt == hip.F16:
        # a two-term gradient: g = dy + dy_lo
        lo = (dy32 - dy.float()).half()
        LO = lo.reshape(-1).to(dev())
        DXl, dGl, dBl = backward(LO, True, 1.0)
        gx2, gg2, gb2 = torch.autograd.grad(yd, (xd, gd, bd), dy.double() + lo.double(), retain_graph=True)
        assert rel_err(dBl, gb2) < 1e-5 and rel_err(dGl, gg2) < (5e-4 if shift else 2e-5)
        if rows > 1:
            assert rel_err(DXl.float().reshape(rows, C), gx2) < dxtol
        # (one row: xhat = 0, dgamma is zero with or without the low term)
        assert not torch.equal(dBl, dB) and (rows == 1 or not torch.equal(dGl, dG))
        DXl2, dGl2, dBl2 = backward(LO, True, 1.0)
        assert torch.equal(DXl, DXl2) and torch.equal(dGl, dGl2) and torch.equal(dBl, dBl2)
    else:
        with pytest.raises(hip.VlfbError, match="dy_lo"):
            backward(DY, True, 1.0)

    # ---- test nets: the running statistics, nothing written but y
    rm1, rv1 = RM.clone(), RV.clone()
    Yt, savet = forward(None, False, True, RM, RV)
    want = (V.value(X) - rm1.cpu().double()) / torch.sqrt(rv1.cpu().double() + eps) * gamma.double() + beta.double()
    V.check_canonical(Yt, False)
    assert rel_err(V.value(Yt), want) < 3e-6 and torch.equal(RM, rm1) and torch.equal(RV, rv1) and bool(torch.isnan(savet).all())
    Ytb, _ = forward(None, False, True, RM, RV)
    assert torch.equal(Yt, Ytb)
    with pytest.raises(hip.VlfbError, match="workspace"):
        hip.call("vlfb_bn_fwd_mix", hip.ptr(X), hip.ptr(Y), None, hip.ptr(G), hip.ptr(Bt), hip.ptr(RM), hip.ptr(RV), None, None,
                 hip.ptr(ws), 16, V.xf, rows, C, eps, mom, 1, 0)


def test_pair_built_by_the_library_is_what_the_kernels_read():
    """vlfb_pair_split makes the input planes the engine's stem conv and these tests hand to the BN kernels"""
    from vlfb import hip
    hip.lib()
    x = torch.randn(64, 16, generator=torch.Generator().manual_seed(5)) * 3
    dst = torch.empty(2 * x.numel(), device=dev(), dtype=torch.float16)
    hip.call("vlfb_pair_split", hip.ptr(x.to(dev())), hip.ptr(dst), x.numel())
    assert torch.equal(dst.cpu(), _pair(x))


# Measured on an MI355X (profiles/bn_mix.txt), relative L2 per parameter gradient against the fp64 oracle evaluated on the
# engine's own ReLU / max-pool / RoI-bin decisions, ava_r50_lfb_nl with the BN overrides at 2 clips of 16 x 64^2:
#   mix   worst 4.56e-3 (res_conv1_bn_b)  median 1.88e-3  p90 2.09e-3   (raw, decisions not pinned: median 1.59e-2)
#   mix, long_rows softmax backward: worst 5.85e-3 (nonlocal_conv4_1_theta_b)  median 2.82e-3  p90 3.44e-3
#   split worst 2.88e-2 (nonlocal_conv4_1_theta_b)  median 2.12e-2   (the measurement of test_bn_model_matches_oracle[split],
#         same session; raw median 1.54e-1)       fp32 worst 3.67e-3  median 2.58e-3
# mix is 0.16x split here, not the ~19x of the affine graph at full size: the batch statistics of this test's few hundred rows
# amplify the FORWARD error (split's three-term products 2.6e-3 at res5, the two-plane forward 1.7e-4, fp32 2.4e-4), and that
# is what the gradients of a BN graph follow.  Nothing pointed at the BN backward, so nothing was changed before the bar was set.
# The bar is the measured mix worst value times 2, rounded up to one digit (9.1e-3 -> 1e-2): the kernels are deterministic,
# the factor covers the differences between boxes.  The long_rows variant is held to the same bar.
MIX_BN_GRAD_BAR = 1e-2


@pytest.mark.parametrize("softmax_bwd", ["p32", "long_rows"])
def test_bn_model_on_mix_matches_oracle(softmax_bwd, monkeypatch):
    """ava_r50_lfb_nl built with Conv3dBN / SpatialBN on `mix`: the blobs that survive the fold, the running statistics, the
    gradient set, and every parameter gradient on identical decisions.  long_rows: the softmax backward of the non-local
    blocks as it runs where the key axis is longer than vlfb_softmax_bwd_p32 takes (the ungrouped res3 block of this graph
    at 224^2 has 3136 keys): fp32 dP, the fp16 copy of P -- held to the same bars"""
    from test_model_gpu import build, rel, SMALL
    from oracle import model as om
    from vlfb.engine import AttentionStep
    if softmax_bwd == "long_rows":
        monkeypatch.setattr(AttentionStep, "P32_MAX_COLS", 0)
    cfg, model, eng, inputs, params, seed_fn = build("ava_r50_lfb_nl", "mix", SMALL + BN)
    nl = [st for st in eng.steps if isinstance(st, AttentionStep) and not st.single]
    assert len(nl) == 5 and all(st.precise and st.p32 == (softmax_bwd == "p32") for st in nl)
    eng.forward()
    eng.backward()
    torch.cuda.synchronize()
    blobs, grads = om.run(cfg, params, inputs, "train", torch.float64, True, seed_fn)
    # (the fused outputs keep the names of the ReLU / Sum they absorbed, which write in place in these graphs)
    for name in ("res_conv1_bn", "res2_2_branch2c_bn", "nonlocal_conv3_1_sum", "res4_5_branch2c_bn", "res5_2_branch2c_bn", "prob"):
        got = eng.fetch(name)
        deep = name.startswith(("res4", "res5", "prob"))
        err = rel(got, blobs[name].detach().numpy().reshape(got.shape))
        print("\n[bn mix] %s %.2e" % (name, err))
        assert err < (1e-2 if deep else 1e-3), name
    for name in ("res_conv1_bn", "res3_0_branch2b_bn", "nonlocal_conv4_1_bn", "res5_2_branch2c_bn"):
        for k in ("_rm", "_riv"):
            assert rel(eng.fetch_param(name + k), blobs[name + k].numpy()) < 1e-3, name + k
    assert set(grads) == set(eng.trainable)
    bn = [n for n in eng.trainable if n.endswith(("_bn_s", "_bn_b"))]
    assert len(bn) == 2 * 58
    for n in eng.trainable:
        g = eng.fetch_grad(n)
        assert np.isfinite(g).all() and float(np.abs(g).sum()) > 0, n
    dec = eng.discrete_decisions()
    _, g2 = om.run(cfg, params, inputs, "train", torch.float64, True, seed_fn, decisions=dec)
    assert not dec["_missing"], sorted(dec["_missing"])
    gmax = max(float(g.norm()) for g in grads.values())
    names = [n for n in eng.trainable if float(grads[n].norm()) > 1e-9 * gmax]
    raw = np.array(sorted(rel(eng.fetch_grad(n), grads[n].numpy()) for n in names))
    cond = sorted((rel(eng.fetch_grad(n), g2[n].numpy()), n) for n in names)
    e = np.array([x for x, _ in cond])
    print("[bn mix %s] %d gradients raw: median %.2e worst %.2e" % (softmax_bwd, len(raw), np.median(raw), raw[-1]))
    print("[bn mix %s] on identical decisions: median %.2e p90 %.2e worst %s" % (softmax_bwd, np.median(e), e[int(0.9 * (len(e) - 1))], cond[-4:]))
    assert MIX_BN_GRAD_BAR is not None and cond[-1][0] < MIX_BN_GRAD_BAR, cond[-5:]


def test_bn_model_on_mix_with_fp32_values(monkeypatch):
    """the fallback: no two-plane storage (VLFB_MIX_PAIR=0), so every SpatialBN runs the VLFB_F32 value form -- fp32 in and out,
    fp16 gradients, the ReLU mask and the WGRAD operands from the half copies a copy pass makes behind the step.  The forward
    is then split's (three-term bf16 products on fp32 storage), so the bars are the ones test_bn_model_matches_oracle sets for
    split: 1e-3 shallow, 1e-2 deep, 6e-2 for the worst gradient on identical decisions."""
    from test_model_gpu import build, rel, SMALL
    from oracle import model as om
    from vlfb.engine import Engine, BNStep
    monkeypatch.setattr(Engine, "MIX_PAIR", False)
    cfg, model, eng, inputs, params, seed_fn = build("ava_r50_lfb_nl", "mix", SMALL + BN)
    bns = [st for st in eng.steps if isinstance(st, BNStep)]
    assert len(bns) == 58 and all(st.xf == 0 and st.gt == 2 for st in bns) and any(st._half_post for st in bns)
    eng.forward()
    eng.backward()
    torch.cuda.synchronize()
    blobs, _ = om.run(cfg, params, inputs, "train", torch.float64, False, seed_fn)
    dec = eng.discrete_decisions()
    _, g2 = om.run(cfg, params, inputs, "train", torch.float64, True, seed_fn, decisions=dec)
    assert not dec["_missing"], sorted(dec["_missing"])
    for name in ("res_conv1_bn", "res2_2_branch2c_bn", "nonlocal_conv3_1_sum"):
        got = eng.fetch(name)
        assert rel(got, blobs[name].detach().numpy().reshape(got.shape)) < 1e-3, name
    for name in ("res4_5_branch2c_bn", "res5_2_branch2c_bn", "prob"):
        got = eng.fetch(name)
        assert rel(got, blobs[name].detach().numpy().reshape(got.shape)) < 1e-2, name
    assert set(g2) == set(eng.trainable)
    gmax = max(float(g.norm()) for g in g2.values())
    cond = sorted((rel(eng.fetch_grad(n), g2[n].numpy()), n) for n in eng.trainable if float(g2[n].norm()) > 1e-9 * gmax)
    e = np.array([x for x, _ in cond])
    print("\n[bn mix fp32 values] on identical decisions: median %.2e worst %s" % (np.median(e), cond[-3:]))
    assert all(np.isfinite(eng.fetch_grad(n)).all() and float(np.abs(eng.fetch_grad(n)).sum()) > 0 for n in eng.trainable)
    assert cond[-1][0] < 6e-2, cond[-5:]


SHAPES = ["NUM_GPUS", 1, "TRAIN.BATCH_SIZE", 2, "TRAIN.VIDEO_LENGTH", 8, "TRAIN.CROP_SIZE", 64,
          "TEST.BATCH_SIZE", 2, "TEST.VIDEO_LENGTH", 8, "TEST.CROP_SIZE", 64]


class ListLoader(object):
    """the loader interface PreciseBN uses, over a fixed list of synthetic batches (as tests/test_precise_bn_gpu.py)"""

    def __init__(self, engine, suffix, batches):
        self.engine, self.suffix, self.batches, self.at = engine, suffix, batches, 0

    def next(self):
        b = self.batches[self.at % len(self.batches)]
        self.at += 1
        return b

    def deliver(self, batch):
        for k, v in batch.items():
            if (k + self.suffix) in self.engine.model.input_blob_names:
                self.engine.feed(k + self.suffix, v)

    def stop(self):
        pass


def test_bn_training_steps_test_net_and_precise_bn_on_mix():
    """charades_r50_baseline with SpatialBN on `mix`: solver steps through the recorded-step replay, a `mix` test net on the
    shared parameters, and a PreciseBN pass whose aux engine is a `mix` engine as well"""
    from test_model_gpu import build
    from oracle import model as om
    from models.model_builder_video import ModelBuilder
    from vlfb.engine import Engine, BNStep
    from vlfb.precise_bn import PreciseBN
    ITERS = 2
    cfg, model, eng, inputs, params, _ = build("charades_r50_baseline", "mix", SHAPES + BN + [
        "TRAIN.COMPUTE_PRECISE_BN", True, "TRAIN.ITER_COMPUTE_PRECISE_BN", ITERS])
    assert any(isinstance(st, BNStep) and st.relu and st.xf == 8 for st in eng.steps)
    tmodel = ModelBuilder(train=False, split="test", name="bn_test")
    tmodel.build_model(suffix="_test")
    teng = Engine(tmodel, "mix", base_seed=cfg.RNG_SEED, share_params_with=eng)
    teng.plan(collections.OrderedDict((k + "_test", v.shape) for k, v in inputs.items() if (k + "_test") in tmodel.input_blob_names))
    for k, v in inputs.items():
        if (k + "_test") in tmodel.input_blob_names:
            teng.feed(k + "_test", v)
    teng.forward()
    torch.cuda.synchronize()
    before = teng.fetch("prob").copy()
    assert np.isfinite(before).all()
    s0, b0 = eng.fetch_param("res4_1_branch2a_bn_s").copy(), eng.fetch_param("res4_1_branch2a_bn_b").copy()
    rm0 = eng.fetch_param("res4_1_branch2a_bn_rm").copy()
    for it in range(4):
        eng.train_step(0.01)
    torch.cuda.synchronize()
    assert eng._trace is not None
    losses = eng.recent_losses()
    assert len(losses) == 4 and all(np.isfinite(losses))
    assert not np.allclose(eng.fetch_param("res4_1_branch2a_bn_s"), s0) and not np.allclose(eng.fetch_param("res4_1_branch2a_bn_b"), b0)
    assert not np.allclose(eng.fetch_param("res4_1_branch2a_bn_rm"), rm0)
    assert "res4_1_branch2a_bn_rm" in teng.shared_params
    teng.forward()
    torch.cuda.synchronize()
    after = teng.fetch("prob")
    assert np.isfinite(after).all() and not np.allclose(after, before)
    # precise BN: the aux engine takes the dtype of the train engine
    batches = [om.synth_inputs(cfg, 2, "train", seed=100 + i, crop=64, frames=8) for i in range(ITERS)]
    pbn = PreciseBN(eng, lambda e, sfx: ListLoader(e, sfx, batches))
    assert pbn.engine.mix and pbn.layers >= 53
    rm1 = eng.fetch_param("res4_1_branch2a_bn_rm").copy()
    pbn.compute_and_update_bn_stats(3)
    torch.cuda.synchronize()
    assert pbn.forwards == ITERS
    for st in pbn.steps:
        rm, rv = eng.param_tensor(st.rmname), eng.param_tensor(st.rvname)
        assert bool(torch.isfinite(rm).all()) and bool(torch.isfinite(rv).all()) and bool((rv > 0).all()), st.rmname
    assert not np.allclose(eng.fetch_param("res4_1_branch2a_bn_rm"), rm1)
