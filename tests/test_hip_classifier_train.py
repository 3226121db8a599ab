"""The launchers of csrc/metric_train.hip called directly, then siss_amd.classifier_train.ResNet18Trainer and
tools/train_classifier.py, against torch on the CPU in f64 (tests/classifier_train_ref.py, held to autograd by
tests/test_classifier_train_host.py).

What is held to what:
* data gradient, weight gradient, fc bias gradient: per element |got - ref64| <= (K + 4) 2^-24 sum |a_i b_i| (K the reduction
  length, the right-hand side formed in f64); the pad slots of a weight gradient exactly zero; the split path bitwise repeatable;
* BatchNorm forward / backward, whole steps, the hand-over, the tool: 4 x the error torch's own f32 CPU result shows against f64 on the
  same inputs (printed beside the kernels' error) -- f32 torch is what f32 can do, the factor covers another summation order;
* max-pool backward: bitwise autograd's;
* cross-entropy: the kernel forms the loss and the gradient in f64 and rounds once, so 2^-23 |ref| (+ the smallest f32 subnormal).
"""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import classifier_train_ref as T
from classifier_ref import ResNet18Ref
from test_hip_small_kernels import Buf, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
MARGIN = 4.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from siss_amd import lib
    lib.load()
    return torch.device("cuda:0")


def call(name, *args):
    from siss_amd import lib
    lib.call(name, *args)
    torch.cuda.synchronize()


def refused(name, *args):
    with pytest.raises(RuntimeError, match="bad argument"):
        call(name, *args)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def packed(case, w, dev):
    from siss_amd import metric_net as mn
    _, cin, cout, k, s, p, *_ = case
    return mn.pack_conv(w, torch.zeros(cout), s, p, dev)


def carried(dy, dev):
    """dy NCHW -> the device's NHWC with the channel stride padded to 32, NaN on the carried channels (never read as values)."""
    from siss_amd import metric_net as mn
    N, cout, Ho, Wo = dy.shape
    ld = mn.padded(cout)
    out = torch.full((N, Ho, Wo, ld), float("nan"))
    out[..., :cout] = nhwc(dy)
    return out.to(dev)


def within(got, ref, bound, what):
    err = (got.double() - ref).abs()
    bad = err > bound
    print(f"{what}: max error {float(err.max()):.3e}, max bound {float(bound.max()):.3e}, worst ratio "
          f"{float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements beyond the bound, worst {float((err - bound).max()):.3e}"


def margin(got, ref32, ref64, what, norm=None):
    """got within MARGIN x the error of torch's f32 result against f64 (max abs, or relative L2 with norm='l2'); both printed."""
    if norm == "l2":
        e_got, e_t = T.rel_l2(got, ref64), T.rel_l2(ref32, ref64)
    else:
        e_got, e_t = float((got.double() - ref64.double()).abs().max()), float((ref32.double() - ref64.double()).abs().max())
    print(f"{what}: kernel error {e_got:.3e}, f32 torch error {e_t:.3e}, ratio {e_got / e_t if e_t > 0 else float('inf'):.3f}")
    assert e_got <= MARGIN * e_t, f"{what}: error {e_got:.3e} > {MARGIN} x {e_t:.3e} (f32 torch against f64)"


# ================================================================ convolution gradients
@pytest.mark.parametrize("case", T.CONV_CASES, ids=lambda c: c[0])
def test_data_gradient(dev, case):
    _, cin, cout, k, s, p, N, H, W = case
    x, w, dy = T.conv_inputs(case)
    L = packed(case, w, dev)
    dyd = carried(dy, dev)
    Ho, Wo, ld = dyd.shape[1], dyd.shape[2], dyd.shape[3]
    from siss_amd import classifier_train as ct
    splits = ct.dgrad_splits(N * H * W, cin, k * k * (ld // 32))
    assert (splits > 1) == (k == 3), (case[0], splits)                        # both paths: the 3 x 3 cases split, the 1 x 1 and fc do not

    def run(add=None, splits=splits):
        out = Buf((N, H, W, cin), F32, dev)
        ct.conv_dgrad(L, dyd, (N, H, W, cin), add=add, splits=splits, out=out.t)
        torch.cuda.synchronize()
        return out
    out = run()
    out.guards("dx")
    ref, _ = T.autograd_conv(x, w, dy, s, p)
    bound = T.product_bound(k * k * cout, T.dgrad_gather(dy.abs(), w.abs(), H, W, s, p))
    got = out.t.cpu()
    within(nchw(got), ref, bound, "dx")
    # + add: one f32 addition on the same sum
    add = torch.randn(N, H, W, cin, generator=torch.Generator().manual_seed(5))
    run(add.to(dev)).check(got + add, "dx + add")
    if splits > 1:
        run().check(got, "the split data gradient, called twice")
        one = run(splits=1)
        one.guards("dx unsplit")
        within(nchw(one.t.cpu()), ref, bound, "dx unsplit")


def run_wgrad(dev, case, splits=None):
    from siss_amd import classifier_train as ct
    _, cin, cout, k, s, p, N, H, W = case
    x, w, dy = T.conv_inputs(case)
    L = packed(case, w, dev)
    dyd = carried(dy, dev)
    image = cin <= 4
    xd = x.to(dev) if image else nhwc(x).to(dev)
    M = N * dyd.shape[1] * dyd.shape[2]
    splits = ct.wgrad_splits(M, cout, L["Kp"]) if splits is None else splits
    out = Buf((cout, L["Kp"]), F32, dev)
    ct.conv_wgrad(L, xd, dyd, out.t, nchw_in=image, splits=splits)
    torch.cuda.synchronize()
    out.guards("dw")
    return out.t.cpu(), (x, w, dy), M, splits


@pytest.mark.parametrize("case", T.CONV_CASES + [T.STEM_CASE, T.SPLIT_CASE], ids=lambda c: c[0])
def test_weight_gradient(dev, case):
    from siss_amd import metric_net as mn
    _, cin, cout, k, s, p, N, H, W = case
    got, (x, w, dy), M, splits = run_wgrad(dev, case)
    assert (splits > 1) == (case in (T.STEM_CASE, T.SPLIT_CASE)), splits      # (the stem's 392 pixels are cut in 3, the split case in 8)
    cp = mn.padded(cin)
    K = k * k * cp
    assert bool((got[:, K:] == 0).all()), "pad slots of the packed weight gradient"
    if case is T.STEM_CASE:
        assert got.shape[1] == 64 and K == 49
    dw = got[:, :K].view(cout, k, k, cp)[..., :cin].permute(0, 3, 1, 2)
    _, ref = T.autograd_conv(x, w, dy, s, p)
    within(dw, ref, T.product_bound(M, T.wgrad_gather(x.abs(), dy.abs(), k, s, p)), "dw")
    if splits > 1:
        again, *_ = run_wgrad(dev, case)
        same(again, got, "the split weight gradient, called twice")
        one, *_ = run_wgrad(dev, case, splits=1)
        within(one[:, :K].view(cout, k, k, cp)[..., :cin].permute(0, 3, 1, 2), ref,
               T.product_bound(M, T.wgrad_gather(x.abs(), dy.abs(), k, s, p)), "dw unsplit")


def test_fc_bias_gradient(dev):
    dy = torch.randn(5, 10, generator=torch.Generator().manual_seed(2))
    dyd = carried(dy.view(5, 10, 1, 1), dev).view(5, 32)
    out = Buf((10,), F32, dev)
    call("siss_cls_bias_grad", dyd, out.t, 5, 10, 32)
    out.guards("db")
    within(out.t.cpu(), dy.double().sum(0), T.product_bound(5, dy.double().abs().sum(0)), "db")


# ================================================================ BatchNorm
class BN:
    """The device buffers of one BatchNorm2d(64) around the launchers."""

    def __init__(self, dev, gamma, beta, C=64):
        from siss_amd import classifier_train as ct
        self.gamma, self.beta = gamma.to(dev), beta.to(dev)
        self.rm, self.rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        self.nbt = torch.zeros(1, device=dev, dtype=torch.int64)
        self.mean, self.invstd = Buf((C,), F64, dev), Buf((C,), F64, dev)
        self.dgamma, self.dbeta = Buf((C,), F32, dev), Buf((C,), F32, dev)
        self.partials = ct.bn_partials(C, dev)

    def fwd(self, x, res, relu, training=True):
        from siss_amd import classifier_train as ct
        y = ct.bn_forward(x, self.gamma, self.beta, self.rm, self.rv, self.nbt, self.mean.t, self.invstd.t, self.partials, res=res,
                          relu=relu, training=training)
        torch.cuda.synchronize()
        return y

    def bwd(self, dy, y, x, dres):
        from siss_amd import classifier_train as ct
        dx = ct.bn_backward(dy, y, x, self.gamma, self.mean.t, self.invstd.t, self.dgamma.t, self.dbeta.t, self.partials, dres=dres)
        torch.cuda.synchronize()
        return dx


def bn_inputs(shape, shifted, seed):
    N, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x, dy, r = (torch.randn(N, 64, H, W, generator=g) for _ in range(3))
    if shifted:
        x = 100.0 + 0.01 * x
    return x, dy, r, torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g)


BN_CASES = [(s, res, relu, False) for s in T.BN_COUNTS for res in (False, True) for relu in (False, True)] + [((2, 7, 7), True, True, True)]


@pytest.mark.parametrize("shape,res,relu,shifted", BN_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_batchnorm_forward_and_backward(dev, shape, res, relu, shifted):
    x, dy, r, gamma, beta = bn_inputs(shape, shifted, 11 * shape[0] + shape[1])
    r64 = T.autograd_bn(x, gamma, beta, r if res else None, relu, dy, F64)
    r32 = T.autograd_bn(x, gamma, beta, r if res else None, relu, dy, F32)
    bn = BN(dev, gamma, beta)
    xd, dyd = nhwc(x).to(dev), Buf(nhwc(dy).shape, F32, dev, body=nhwc(dy))
    y = bn.fwd(xd, nhwc(r).to(dev) if res else None, relu)
    margin(nchw(y.cpu()), r32[0], r64[0], "y")
    dres = Buf(xd.shape, F32, dev) if res else None
    dx = bn.bwd(dyd.t, y if relu else None, xd, None if dres is None else dres.t)
    dyd.check(nhwc(dy), "dy after the backward")
    for b, what in ((bn.mean, "mean"), (bn.invstd, "invstd"), (bn.dgamma, "dgamma"), (bn.dbeta, "dbeta")):
        b.guards(what)
    margin(nchw(dx.cpu()), r32[1], r64[1], "dx")
    margin(bn.dgamma.t.cpu(), r32[2], r64[2], "dgamma")
    margin(bn.dbeta.t.cpu(), r32[3], r64[3], "dbeta")
    if res:                                                   # the residual branch's gradient: dy under the mask of the kernel's own output
        g = torch.where(y.cpu() > 0, nhwc(dy), torch.zeros(())) if relu else nhwc(dy)     # (+0 where masked, as threshold_backward)
        dres.check(g, "dres")
        # in place over dy
        bn.bwd(dyd.t, y if relu else None, xd, dyd.t)
        dyd.check(g, "dres written over dy")


def test_batchnorm_running_statistics_after_two_calls(dev):
    g = torch.Generator().manual_seed(3)
    xs = [torch.randn(3, 64, 5, 5, generator=g) * 2 + 1, torch.randn(3, 64, 5, 5, generator=g) - 0.5]
    refs = {}
    for dt in (F32, F64):
        m = torch.nn.BatchNorm2d(64).to(dt).train()
        for x in xs:
            m(x.to(dt))
        refs[dt] = m
    bn = BN(dev, torch.ones(64), torch.zeros(64))
    for x in xs:
        bn.fwd(nhwc(x).to(dev), None, False)
    assert int(bn.nbt.cpu()) == 2 == int(refs[F64].num_batches_tracked)
    margin(bn.rm.cpu(), refs[F32].running_mean, refs[F64].running_mean, "running_mean")
    margin(bn.rv.cpu(), refs[F32].running_var, refs[F64].running_var, "running_var")
    # eval mode: the running statistics are used and nothing is updated
    before = (bn.rm.clone(), bn.rv.clone())
    y = bn.fwd(nhwc(xs[0]).to(dev), None, True, training=False)
    assert torch.equal(bn.rm, before[0]) and torch.equal(bn.rv, before[1]) and int(bn.nbt.cpu()) == 2
    ev = {dt: torch.relu(refs[dt].eval()(xs[0].to(dt))).detach() for dt in (F32, F64)}
    margin(nchw(y.cpu()), ev[F32], ev[F64], "eval y")


# ================================================================ max pool, cross-entropy
def test_maxpool_backward_is_autograd_s_bitwise(dev):
    from siss_amd import classifier_train as ct
    x, dy = T.pool_inputs()
    xx = x.clone().requires_grad_(True)
    F.max_pool2d(xx, 3, 2, 1).backward(dy)
    got = ct.max_pool3_backward(nhwc(x).to(dev), nhwc(dy).to(dev))
    torch.cuda.synchronize()
    same(nchw(got.cpu()), xx.grad, "max-pool dx")


@pytest.mark.parametrize("B", [1, 5, 128])
def test_cross_entropy(dev, B):
    g = torch.Generator().manual_seed(B)
    logits = torch.randn(B, 10, generator=g)
    logits = logits * (80.0 / float(logits.abs().max()))
    labels = torch.randint(0, 10, (B,), generator=g)
    lg = logits.double().requires_grad_(True)
    ref = F.cross_entropy(lg, labels)
    ref.backward()
    loss, dl = Buf((1,), F32, dev), Buf((B, 32), F32, dev)
    call("siss_cls_softmax_ce", logits.to(dev), labels.to(dev), loss.t, dl.t, B, 10, 10, 32)
    loss.guards("loss"); dl.guards("dlogits")
    got = dl.t.cpu()
    assert bool((got[:, 10:] == 0).all())
    # the kernel works in f64 and rounds once to f32: 2^-24 |ref|, doubled, + the smallest f32 subnormal; and the f64 reference forms
    # softmax - onehot from values <= 1, so near a confident label it carries an absolute error of a few 2^-53 itself (8 of them here,
    # for the reference's and the kernel's own f64 arithmetic together), divided by B like the gradient
    tiny, own = 2.0 ** -149, 8 * 2.0 ** -53
    within(loss.t.cpu(), ref.detach().view(1), 2.0 ** -23 * ref.detach().abs().view(1) + tiny + 160 * own, "loss")     # (logits up to +-80 are subtracted in f64)
    within(got[:, :10], lg.grad, 2.0 ** -23 * lg.grad.abs() + tiny + own / B, "dlogits")


# ================================================================ refusals
def test_refusals_write_nothing(dev):
    from siss_amd import classifier_train as ct
    case = T.CONV_CASES[0]
    _, cin, cout, k, s, p, N, H, W = case
    x, w, dy = T.conv_inputs(case)
    L, dyd, xd = packed(case, w, dev), carried(dy, dev), nhwc(x).to(dev)
    dx, dw, ws = Buf((N, H, W, cin), F32, dev), Buf((cout, L["Kp"]), F32, dev), Buf((4 * cout * L["Kp"],), F32, dev)
    off = lambda t: t.reshape(-1)[1:]                          # 4 bytes off a 16-byte boundary
    dg = lambda dy_=dyd, w_=L["w"], add=None, out=dx.t, n=N, kp=L["Kp"], ld=64, ws_=None, words=0, splits=1: \
        ("siss_cls_conv_dgrad", dy_, w_, add, out, ws_, words, n, H, W, cin, H, W, cout, ld, k, k, s, p, p, kp, splits)
    wg = lambda x_=xd, dy_=dyd, out=dw.t, ws_=None, words=0, n=N, splits=1, ho=H: \
        ("siss_cls_conv_wgrad", x_, 0, dy_, out, ws_, words, n, H, W, cin, ho, W, cout, 64, k, k, s, p, p, L["Kp"], splits)
    C, M = 64, N * H * W
    gamma, rm, rv = torch.ones(C, device=dev), Buf((C,), F32, dev), Buf((C,), F32, dev)
    nbt = torch.full((1,), 7, device=dev, dtype=torch.int64)
    sm, si, y, dgm, dbt = Buf((C,), F64, dev), Buf((C,), F64, dev), Buf((M, C), F32, dev), Buf((C,), F32, dev), Buf((C,), F32, dev)
    part = ct.bn_partials(C, dev)
    part.fill_(-5.0)
    stat64 = torch.ones(C, device=dev, dtype=F64)
    x2 = xd.view(M, C)
    bf = lambda x_=x2, g_=gamma, y_=y.t, rm_=rm.t, nb=nbt, sm_=sm.t, pt=part, words=None, m=M, c=C, tr=1: \
        ("siss_cls_bn_fwd", x_, g_, gamma, None, y_, rm_, rv.t, nb, sm_, si.t, pt, (0 if pt is None else pt.numel()) if words is None else words, m, c, 1, tr)
    bb = lambda dy_=x2, x_=x2, out=y.t, dres=None, dg_=dgm.t, pt=part, m=M, c=C: \
        ("siss_cls_bn_bwd", dy_, None, x_, gamma, stat64, stat64, out, dres, dg_, dbt.t, pt, 0 if pt is None else pt.numel(), m, c)
    pool_x, pool_dy, pool_dx = torch.zeros(2, 14, 14, 64, device=dev), torch.zeros(2, 7, 7, 64, device=dev), Buf((2, 14, 14, 64), F32, dev)
    mp = lambda x_=pool_x, dy_=pool_dy, out=pool_dx.t, n=2, c=64, ho=7: ("siss_cls_maxpool3_bwd", x_, dy_, out, n, 14, 14, c, ho, 7)
    logits, labels = torch.zeros(5, 10, device=dev), torch.zeros(5, device=dev, dtype=torch.int64)
    loss, dl = Buf((1,), F32, dev), Buf((5, 32), F32, dev)
    ce = lambda lg=logits, lb=labels, ls=loss.t, d=dl.t, b=5, c=10, ldd=32: ("siss_cls_softmax_ce", lg, lb, ls, d, b, c, 10, ldd)
    db = Buf((10,), F32, dev)
    for args in (dg(dy_=None), dg(w_=None), dg(out=None), dg(dy_=off(dyd)[:-3]), dg(out=off(dx.t)), dg(add=off(xd)), dg(n=0), dg(kp=L["Kp"] + 32),
                 dg(ld=48), dg(ld=128), dg(splits=0), dg(splits=19), dg(splits=4), dg(splits=4, ws_=ws.t, words=4 * N * H * W * cin - 1),
                 dg(splits=4, ws_=off(ws.t), words=4 * N * H * W * cin),
                 wg(x_=None), wg(dy_=None), wg(out=None), wg(x_=off(xd)), wg(out=off(dw.t)), wg(n=0), wg(splits=0), wg(splits=4),
                 wg(splits=4, ws_=ws.t, words=4 * cout * L["Kp"] - 1), wg(splits=4, ws_=off(ws.t), words=4 * cout * L["Kp"]), wg(ho=H - 1),
                 ("siss_cls_bias_grad", None, db.t, 5, 10, 32), ("siss_cls_bias_grad", dl.t, None, 5, 10, 32),
                 ("siss_cls_bias_grad", dl.t, db.t, 0, 10, 32), ("siss_cls_bias_grad", dl.t, db.t, 5, 0, 32), ("siss_cls_bias_grad", dl.t, db.t, 5, 10, 8),
                 bf(x_=None), bf(g_=None), bf(y_=None), bf(rm_=None), bf(nb=None), bf(sm_=None), bf(pt=None), bf(words=63), bf(x_=off(x2)),
                 bf(y_=off(y.t)), bf(m=0), bf(m=1), bf(c=0), bf(c=62), bf(tr=0, sm_=off(sm.t)),
                 bb(dy_=None), bb(x_=None), bb(out=None), bb(dg_=None), bb(pt=None), bb(dy_=off(x2)), bb(out=off(y.t)), bb(dres=off(y.t)),
                 bb(m=0), bb(c=0), bb(c=62),
                 mp(x_=None), mp(dy_=None), mp(out=None), mp(x_=off(pool_x)), mp(out=off(pool_dx.t)), mp(n=0), mp(c=0), mp(c=62), mp(ho=6),
                 ce(lg=None), ce(lb=None), ce(ls=None), ce(d=None), ce(b=0), ce(c=0), ce(c=11), ce(ldd=8), ce(lb=labels.view(torch.int32)[1:])):
        refused(*args)
    for b, what in ((dx, "dx"), (dw, "dw"), (ws, "ws"), (rm, "running_mean"), (rv, "running_var"), (sm, "save_mean"), (si, "save_invstd"),
                    (y, "y"), (dgm, "dgamma"), (dbt, "dbeta"), (pool_dx, "pool dx"), (loss, "loss"), (dl, "dlogits"), (db, "db")):
        b.check(torch.full(b.shape, 77.0), what + " after the refusals")
    assert int(nbt.cpu()) == 7 and bool((part == -5.0).all())


# ================================================================ whole steps
def trainer_and_ref(dev, seed=1):
    from siss_amd.classifier_train import ResNet18Trainer
    tr = ResNet18Trainer(device=dev, seed=seed)
    return tr, tr.state_dict()


def batches_for(B, hw, n, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(B, 1, hw, hw, generator=g), torch.randint(0, 10, (B,), generator=g)) for _ in range(n)]


@pytest.mark.parametrize("B,hw", [(8, 28), (5, 20)])
def test_two_steps_against_the_f64_reference(dev, B, hw):
    """After each of two steps: the loss, every gradient tensor (relative L2 per tensor), the updated parameters and the running
    statistics, each within MARGIN x what f32 torch shows against f64.  The updated parameters and the running statistics are each
    held as ONE vector over all their tensors: Adam's first steps move a weight by lr g / (|g| + eps), so an element whose gradient
    is near zero gets a full +-lr with the sign its rounding errors leave it -- per tensor, one such element decides the ratio for
    either f32 implementation (measured at B = 8, step 1, layer3.0.conv2.weight: g = -1.2e-7 in f64, -2.3e-7 in f32 torch, +1.6e-7
    here, among gradients of median 9e-3: 8.2e-5 here against 1.9e-6; at B = 5 the same tensor 1.2e-4 here against 5.2e-4 for f32
    torch), while over the 11 M parameters those elements number enough for the sum to mean something (3.4e-5 against 3.5e-5).

    The loss of step 2 is the one check here that depends on WHICH of those elements a given f32 summation order flips: it is a single
    scalar evaluated at parameters that step 1 moved.  Measured at B = 8: 4.8e-6 off the f64 run's, f32 torch 4.8e-6 (bound 4 x that);
    with the data gradient's K loop unsplit -- another summation order, the same accuracy per gradient tensor -- it was 3.1e-5 and
    missed the bound.  The bound is the issue's and stays."""
    tr, sd0 = trainer_and_ref(dev)
    assert list(sd0) == list(ResNet18Ref().state_dict())
    batches = batches_for(B, hw, 2, 100 + B)
    r64, r32 = T.ref_steps(sd0, batches, F64), T.ref_steps(sd0, batches, F32)
    cat = lambda d, keys: torch.cat([d[k].double().reshape(-1) for k in keys])
    failures = []
    for i, (x, y) in enumerate(batches):
        loss = tr.step(x, y)
        torch.cuda.synchronize()
        grads, sd = tr.gradients(), tr.state_dict()
        params, stats = list(grads), [k for k in sd if "running_" in k]
        assert sorted(params + stats + [k for k in sd if k.endswith("num_batches_tracked")]) == sorted(sd)
        checks = [("loss", torch.tensor(float(loss)), torch.tensor(r32[i][0]), torch.tensor(r64[i][0]), None)]
        checks += [("grad " + k, grads[k], r32[i][1][k], r64[i][1][k], "l2") for k in grads]
        checks += [("updated parameters", cat(sd, params), cat(r32[i][2], params), cat(r64[i][2], params), "l2"),
                   ("running statistics", cat(sd, stats), cat(r32[i][2], stats), cat(r64[i][2], stats), "l2")]
        for what, got, a, b, norm in checks:
            try:
                margin(got, a, b, f"step {i + 1} {what}", norm)
            except AssertionError as e:
                failures.append(str(e).splitlines()[0])
        for k in sd:
            if k.endswith("num_batches_tracked"):
                assert int(sd[k]) == i + 1 == int(r64[i][2][k])
    assert not failures, "\n".join(failures)


def test_same_seed_and_batches_end_bitwise_equal(dev):
    batches = batches_for(6, 28, 2, 7) + batches_for(3, 28, 1, 8)            # (the batch size changes between calls)
    ends = []
    for _ in range(2):
        tr, _ = trainer_and_ref(dev, seed=4)
        losses = [tr.step(x, y) for x, y in batches]
        torch.cuda.synchronize()
        ends.append([t.cpu() for t in (tr.flat, tr.grad, tr.stats, tr.opt.m, tr.opt.v, torch.stack(losses))] + [tr.tracked.cpu()])
    for a, b in zip(*ends):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(ends[0][0]).all()) and int(ends[0][-1][0]) == 3
    with pytest.raises(ValueError):
        tr.step(batches[0][0][:1], batches[0][1][:1])


def test_saved_file_loads_into_the_metric_classifier(dev, tmp_path):
    from siss_amd.classifier import Classifier, resnet18
    tr, _ = trainer_and_ref(dev)
    for x, y in batches_for(8, 28, 2, 21):
        tr.step(x, y)
    path = tmp_path / "mnist.pt"
    tr.save(path)
    sd = torch.load(path, map_location="cpu")
    net = resnet18(10, True)
    assert net.load_state_dict(sd) is None and list(sd) == list(net.state_dict())
    ref32, ref64 = ResNet18Ref(), ResNet18Ref().double()
    ref32.load_state_dict(sd)
    ref64.load_state_dict({k: v if v.dtype == torch.int64 else v.double() for k, v in sd.items()})
    x = torch.rand(16, 1, 28, 28, generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        l32, l64 = ref32.eval()(x), ref64.eval()(x.double())
    clf = Classifier(resnet18, str(path), {"num_classes": 10, "grayscale": True}, None, dev)
    got_c, got_t = clf.compute_logits(x.to(dev)).cpu(), tr.eval_logits(x).cpu()
    margin(got_t, l32, l64, "trainer eval logits")
    margin(got_c, l32, l64, "Classifier logits")
    e_t = float((l32.double() - l64).abs().max())
    print(f"Classifier against trainer: {float((got_c - got_t).abs().max()):.3e}, margin {MARGIN * e_t:.3e}")
    assert float((got_c.double() - got_t.double()).abs().max()) <= MARGIN * e_t


# ================================================================ the tool
def test_tool_trains_on_synthetic_images_and_repeats_bitwise(dev, tmp_path):
    spec = importlib.util.spec_from_file_location("train_classifier_tool", os.path.join(ROOT, "tools", "train_classifier.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    from siss_amd.classifier_train import ResNet18Trainer
    from siss_amd.data import EpochSampler
    outs = []
    for d in ("a", "b"):
        out = tmp_path / d / "mnist.pt"
        rec = tool.main(["--allow-synthetic", "--epochs", "2", "--batch-size", "64", "--out", str(out)])
        assert out.is_file() and (tmp_path / d / "metrics.json").is_file()
        outs.append((torch.load(out, map_location="cpu"), json.load(open(tmp_path / d / "metrics.json"))))
        assert outs[-1][1]["step_losses"] == rec["step_losses"]
    (sd_a, m_a), (sd_b, m_b) = outs
    assert m_a["seed"] == 1 and m_a["args"]["epochs"] == 2 and m_a["args"]["batch_size"] == 64 and m_a["images"] == 640
    assert len(m_a["epochs"]) == 2 and len(m_a["step_losses"]) == 20 and all(0 <= e["train_acc"] <= 1 for e in m_a["epochs"])
    m_a["args"].pop("out"), m_b["args"].pop("out")
    assert m_a == m_b and list(sd_a) == list(sd_b) and all(torch.equal(sd_a[k], sd_b[k]) for k in sd_a)
    # the first 10 steps on the CPU: the same initial state (the trainer's constructor at that seed), the same batches
    ds = tool.Synthetic(640, 1, "train")
    sd0 = ResNet18Trainer(device=dev, seed=1).state_dict()
    batches = [tool.batch_of(ds, idx) for _, _, idx in EpochSampler(640, 64, 1, 1)]
    assert len(batches) == 10
    l32 = [l for l, _, _ in T.ref_steps(sd0, batches, F32)]
    l64 = [l for l, _, _ in T.ref_steps(sd0, batches, F64)]
    e_t = max(abs(a - b) for a, b in zip(l32, l64))
    errs = [abs(a - b) for a, b in zip(m_a["step_losses"][:10], l32)]
    print("tool losses", m_a["step_losses"][:10], "\nf32 torch  ", l32, "\nf64 torch  ", l64)
    print(f"tool against f32 torch: {max(errs):.3e}; f32 torch against f64 over the 10 steps: {e_t:.3e}")
    assert max(errs) <= MARGIN * e_t
