"""Optimizer scalars in device memory (include/dana_hip.h: the control block of dana_sgd_momentum_ctl / dana_adam_ctl):
the gradient-norm pass and the clipping coefficient against float64, the *_ctl updates against the launch-parameter kernels
bit for bit, Trainer(clip_norm=...) against the reference's loop (train.py:125-143 with net_utils.clip_gradient between
backward and step), and what the control block buys the replayed iteration: Adam, a learning-rate change and clipping
under program.ProgramTrainer and graphs.GraphedTrainer without re-recording."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ZERO_GRAD_BIASES = ("unary_layer.bias", "adapt_q_layer.bias", "adapt_k_layer.bias", "channel_k_layer.bias")


def _ops():
    import dana_amd
    return dana_amd.ops


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _f32(x):
    return float(np.float32(x))


def _check(got, ref, mag, what):
    """the rule of test_gpu_backward_ops.py: |got - ref| <= 1e-6 * mag per element; prints the worst err / bound"""
    got = got.detach().double().cpu().reshape(ref.shape)
    assert torch.isfinite(got).all(), "%s: non-finite result" % what
    err = (got - ref).abs()
    bound = 1e-6 * mag.expand_as(ref)
    inexact = torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err))
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), inexact)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print("ERR/BOUND %-44s %.4f" % (what, worst))
    assert worst <= 1.0, "%s: worst err / bound = %.3f (max err %.3e)" % (what, worst, float(err.max()))


def _model(dev, name="DAnA", ba=True, seed=5):
    import dana_amd
    from dana_amd import synthetic as S
    kw = dict(use_BA_block=ba) if name == "DAnA" else {}
    m = dana_amd.get_model(name, pretrained=False, way=2, shot=2, classes=["fg", "bg"], **kw)
    m.load_state_dict(S.fill_state_dict(m.state_dict(), seed=seed, profile="test"))
    return m.to(dev).train()


def _params(m):
    return np.concatenate([p.detach().float().cpu().numpy().ravel() for _, p in sorted(m.named_parameters())])


def _hyper(dev, lrs, grad_scale=1.0, clip_norm=0.0, betas=(0.0, 0.0), step=1):
    ops = _ops()
    return ops.optim_pack_hyper(torch.zeros(ops.OPTIM_HYPER_FLOATS), lrs, grad_scale, clip_norm, betas, step).to(dev)


def _state(dev, coef=1.0, grad_scale=1.0):
    """the device-written half as dana_optim_prepare leaves it: (sqnorm, total_norm, coef, gs_eff = grad_scale * coef)"""
    return torch.tensor([0.0, 0.0, _f32(coef), float(np.float32(grad_scale) * np.float32(coef))], dtype=torch.float32, device=dev)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the norm kernel
# ---------------------------------------------------------------------------------------------------------------------
def _sqnorm(x):
    """-> (float64 sum of the partials in index order, the partials)"""
    ops = _ops()
    k = ops.grad_sqnorm_workspace(x.numel())
    part = torch.full((k,), float("nan"), dtype=torch.float64, device=x.device)
    ops.grad_sqnorm_(x, part)
    host = part.cpu().numpy()
    total = 0.0
    for v in host:  # index order, in double
        total += float(v)
    return total, part


def _geometry():
    """(floats one workgroup covers per pass of its grid-stride loop, the grid's cap) derived from the workspace query: one
    double per workgroup, the workgroup count grows by one per span until the cap"""
    L = _ops().lib()
    q = lambda n: L.query("dana_grad_sqnorm_workspace_bytes", n) // 8
    assert q(4) == 1
    span = 4
    while q(span + 4) == 1:
        span += 4
        assert span <= 1 << 16
    cap = q(1 << 40)
    assert q(span * cap) == cap and q(span * (cap - 1)) == cap - 1
    return span, cap


@pytest.fixture(scope="module")
def dana_trainer(dev):
    from dana_amd.trainer import Trainer
    return Trainer(_model(dev), 0.01)


def test_grad_sqnorm_vs_fp64(dev, dana_trainer):
    """sum g^2 within 1e-6 relative of float64 (all terms are non-negative; the bar of test_gpu_backward_ops.py's sums) on
    the two flat sizes of a real DAnA trainer, the smallest segment, and one float4 below / at / above one workgroup pass
    and one full grid pass; N(0, 1) data and data spread over four decades; bit-identical between two calls and on a side
    stream"""
    ops = _ops()
    span, cap = _geometry()
    sizes = [dana_trainer.weights.numel, dana_trainer.biases.numel, 4, span - 4, span, span + 4,
             span * cap - 4, span * cap, span * cap + 4]
    assert dana_trainer.weights.numel > span * cap, "the production size must exercise the grid-stride loop"
    side = torch.cuda.Stream(device=dev)
    for n in sizes:
        assert n % 4 == 0 and n > 0
        for kind in ("normal", "decades"):
            g = _gen(n % 1009 + (7 if kind == "normal" else 8))
            x = torch.randn(n, generator=g)
            if kind == "decades":
                x = x * torch.pow(10.0, 4.0 * torch.rand(n, generator=g))
            ref = float(x.double().pow(2).sum())
            xd = x.to(dev)
            got, part = _sqnorm(xd)
            rel = abs(got - ref) / ref
            print("SQNORM n=%-9d %-8s rel err %.3e (%d partials)" % (n, kind, rel, part.numel()))
            assert rel <= 1e-6, (n, kind, got, ref)
            got2, part2 = _sqnorm(xd)
            assert torch.equal(part, part2) and got2 == got
            torch.cuda.synchronize(dev)
            with torch.cuda.stream(side):
                got3, part3 = _sqnorm(xd)
            side.synchronize()
            assert torch.equal(part, part3) and got3 == got


def test_grad_sqnorm_ignores_the_zero_padding_of_flat_buckets(dev):
    """FlatBuckets starts every parameter 16-byte aligned: the padding floats are zero and add nothing to the norm"""
    from dana_amd.trainer import FlatBuckets
    g = _gen(3)
    shapes = [(5,), (3, 7), (1,), (129,), (2, 3, 1, 1), (1026,), (4,), (31, 33)]
    named = [("p%d" % i, torch.nn.Parameter(torch.randn(*s, generator=g).to(dev))) for i, s in enumerate(shapes)]
    fb = FlatBuckets(named)
    assert fb.numel > sum(p.numel() for _, p in named) and fb.numel % 4 == 0
    ref = 0.0
    for _, p in named:
        gr = torch.randn(p.shape, generator=g)
        p.grad.copy_(gr.to(dev))  # (the views into the flat gradient buffer)
        ref += float(gr.double().pow(2).sum())
    got, _ = _sqnorm(fb.grads)
    assert abs(got - ref) <= 1e-6 * ref, (got, ref)
    assert abs(float(fb.grads.double().pow(2).sum()) - ref) <= 1e-12 * ref  # the padding really is zero


# ---------------------------------------------------------------------------------------------------------------------
# 2. the prepare kernel
# ---------------------------------------------------------------------------------------------------------------------
def _prepare(dev, partials, grad_scale, clip):
    ops = _ops()
    state = torch.full((ops.OPTIM_STATE_FLOATS,), float("nan"), dtype=torch.float32, device=dev)
    ops.optim_prepare_(partials, _hyper(dev, [0.01, 0.02], grad_scale, clip), state)
    return state.cpu().numpy()


def test_optim_prepare_coefficient(dev):
    """totals below, exactly at and above clip_norm, and clip_norm = 0: coef is exactly 1 and gs_eff the bits of grad_scale
    unless the norm exceeds the threshold; then coef = clip / total within 1e-6 of float64"""
    gs = 0.25
    part = torch.tensor([144.0, 0.0, 112.0, 144.0], dtype=torch.float64, device=dev)  # sum 400 -> total = 0.25 * 20 = 5
    for clip, clipped in ((6.0, False), (5.0, False), (3.0, True), (0.0, False)):
        st = _prepare(dev, part, gs, clip)
        assert st[0] == np.float32(400.0) and st[1] == np.float32(5.0)
        if clipped:
            assert abs(float(st[2]) - clip / 5.0) <= 1e-6 * (clip / 5.0)
            assert st[3] == np.float32(gs) * st[2]
        else:
            assert st[2] == np.float32(1.0) and st[3].tobytes() == np.float32(gs).tobytes()
    # more partials than the workgroup has threads, an inexact grad_scale, an irrational norm
    g = _gen(17)
    big = torch.rand(777, generator=g, dtype=torch.float64) * 1e3
    gs = 1.0 / 3.0
    total = _f32(gs) * math.sqrt(float(big.sum()))
    for clip in (0.0, 2.0 * total, 0.37 * total):
        st = _prepare(dev, big.to(dev), gs, clip)
        assert abs(float(st[0]) - float(big.sum())) <= 1e-6 * float(big.sum())
        assert abs(float(st[1]) - total) <= 1e-6 * total
        if 0 < clip < total:
            want = _f32(clip) / total
            assert abs(float(st[2]) - want) <= 1e-6 * want
            assert st[3] == np.float32(gs) * st[2]
        else:
            assert st[2] == np.float32(1.0) and st[3].tobytes() == np.float32(gs).tobytes()
    # no partials at all (every group empty): norm 0, nothing to clip
    st = _prepare(dev, torch.zeros(0, dtype=torch.float64, device=dev), 0.5, 1.0)
    assert st[0] == 0 and st[1] == 0 and st[2] == 1 and st[3] == np.float32(0.5)


def test_optim_prepare_over_two_groups_does_not_depend_on_the_split(dev):
    """the partials of two groups lie one behind the other and the kernel sums the concatenated sequence: the same
    gradients cut into two groups at different places give the same norm (within the norm kernel's 1e-6 of float64; where
    one group ends is not even an argument of dana_optim_prepare), and one fixed partial sequence gives the same bits
    wherever the boundary between its groups is taken to be"""
    ops = _ops()
    g = _gen(23)
    n = 3 * 1024 * 50 + 8
    x = torch.randn(n, generator=g)
    ref = math.sqrt(float(x.double().pow(2).sum()))
    xd = x.to(dev)
    states = []
    for cut in (4, 1024 * 7 + 4, n // 2 // 4 * 4, n - 4):
        ka, kb = ops.grad_sqnorm_workspace(cut), ops.grad_sqnorm_workspace(n - cut)
        part = torch.full((ka + kb,), float("nan"), dtype=torch.float64, device=dev)
        ops.grad_sqnorm_(xd[:cut], part[:ka])
        ops.grad_sqnorm_(xd[cut:], part[ka:])
        st = _prepare(dev, part, 1.0, 0.5 * ref)
        assert abs(float(st[1]) - ref) <= 1e-6 * ref, (cut, st, ref)
        assert abs(float(st[2]) - 0.5) <= 1e-6
        states.append((part, st))
    part = states[1][0]
    again = _prepare(dev, torch.cat([part[:3].clone(), part[3:].clone()]), 1.0, 0.5 * ref)
    assert again.tobytes() == states[1][1].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the *_ctl updates
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 1028, 1 << 20])
@pytest.mark.parametrize("wd,gs", [(0.0, 1.0), (1e-4, 0.125)])
def test_sgd_momentum_ctl_equals_the_launch_parameter_kernel_bit_for_bit(dev, n, wd, gs):
    """coef = 1: the same bits in params and buf as dana_sgd_momentum, for first_step 0 and 1 and both group slots"""
    ops = _ops()
    g = _gen(n % 97 + 5)
    lr, mom = 1e-3, 0.9
    hyper, state = _hyper(dev, [lr, 2 * lr], gs), _state(dev, 1.0, gs)
    for group in (0, 1):
        for first in (True, False):
            p0, g0, b0 = (torch.randn(n, generator=g).to(dev) for _ in range(3))
            pa, ba, pb, bb = p0.clone(), b0.clone(), p0.clone(), b0.clone()
            ops.sgd_momentum_(pa, g0, ba, lr * (group + 1), mom, wd, grad_scale=gs, first_step=first)
            ops.sgd_momentum_ctl_(pb, g0, bb, hyper, state, group, mom, wd, first_step=first)
            assert torch.equal(pa, pb) and torch.equal(ba, bb), (group, first)
            assert not torch.equal(pa, p0)


@pytest.mark.parametrize("n", [4, 1028, 1 << 20])
@pytest.mark.parametrize("wd,gs", [(0.0, 1.0), (1e-4, 0.125)])
def test_adam_ctl_equals_the_launch_parameter_kernel_bit_for_bit(dev, n, wd, gs):
    """coef = 1: the same bits in params and both moments as dana_adam at steps 1, 2, 10 and 1000 (the bias corrections
    come from the host-packed block), both group slots"""
    ops = _ops()
    g = _gen(n % 97 + 6)
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    state = _state(dev, 1.0, gs)
    for step in (1, 2, 10, 1000):
        hyper = _hyper(dev, [lr, 2 * lr], gs, betas=(b1, b2), step=step)
        for group in (0, 1):
            p0, g0, m0 = (torch.randn(n, generator=g).to(dev) for _ in range(3))
            v0 = torch.rand(n, generator=g).to(dev)
            a, b = [t.clone() for t in (p0, m0, v0)], [t.clone() for t in (p0, m0, v0)]
            ops.adam_(a[0], g0, a[1], a[2], lr * (group + 1), step, beta1=b1, beta2=b2, eps=eps, weight_decay=wd, grad_scale=gs)
            ops.adam_ctl_(b[0], g0, b[1], b[2], hyper, state, group, beta1=b1, beta2=b2, eps=eps, weight_decay=wd)
            for x, y, what in zip(a, b, ("p", "exp_avg", "exp_avg_sq")):
                assert torch.equal(x, y), (what, step, group)
            assert not torch.equal(a[0], p0)


@pytest.mark.parametrize("n", [4, 1028, 1 << 20])
@pytest.mark.parametrize("wd,gs", [(0.0, 1.0), (1e-4, 0.125)])
def test_sgd_momentum_ctl_with_a_clipping_coefficient_vs_torch_fp64(dev, n, wd, gs):
    """coef != 1: torch.optim.SGD in float64 on the gradient pre-multiplied by coef, three steps, with the rule and the
    magnitudes of test_sgd_momentum_vs_torch_fp64"""
    ops = _ops()
    g = _gen(n % 97 + 62)
    lr, mom, coef = 1e-3, 0.9, 0.37
    lrf, momf, wdf, gsf, cf = _f32(lr), _f32(mom), _f32(wd), _f32(gs), _f32(coef)
    hyper, state = _hyper(dev, [0.5, lr], gs, clip_norm=1.0), _state(dev, coef, gs)
    p0 = torch.randn(n, generator=g)
    pr = p0.double().requires_grad_(True)
    opt = torch.optim.SGD([pr], lr=lrf, momentum=momf, weight_decay=wdf)
    p, buf = p0.clone().to(dev), torch.full((n,), float("nan"), device=dev)
    for step in range(3):
        grad = torch.randn(n, generator=g)
        p_before = pr.detach().clone()
        b_before = opt.state[pr]["momentum_buffer"].clone() if step else torch.zeros(n, dtype=torch.float64)
        pr.grad = grad.double() * gsf * cf
        opt.step()
        ops.sgd_momentum_ctl_(p, grad.to(dev), buf, hyper, state, 1, mom, wd, first_step=(step == 0))
        b_ref = opt.state[pr]["momentum_buffer"]
        mag_b = (momf * b_before).abs() + (grad.double() * gsf * cf).abs() + (wdf * p_before).abs()
        _check(buf, b_ref, mag_b, "sgd_momentum_ctl_ buf (step %d)" % (step + 1))
        _check(p, pr.detach(), p_before.abs() + (lrf * b_ref).abs(), "sgd_momentum_ctl_ p (step %d)" % (step + 1))
        with torch.no_grad():
            pr.copy_(p.double().cpu())
            opt.state[pr]["momentum_buffer"].copy_(buf.double().cpu())


@pytest.mark.parametrize("n", [4, 1028, 1 << 20])
@pytest.mark.parametrize("wd,gs", [(0.0, 1.0), (1e-4, 0.125)])
def test_adam_ctl_with_a_clipping_coefficient_vs_torch_fp64(dev, n, wd, gs):
    """coef != 1: torch.optim.Adam in float64 on the gradient pre-multiplied by coef, steps 1, 2 and 10 with the state
    carried over, with the rule and the magnitudes of test_adam_vs_torch_fp64"""
    ops = _ops()
    g = _gen(n % 97 + 72)
    lr, b1, b2, eps, coef = 1e-3, 0.9, 0.999, 1e-8, 0.37
    lrf, b1f, b2f, epsf, wdf, gsf, cf = _f32(lr), _f32(b1), _f32(b2), _f32(eps), _f32(wd), _f32(gs), _f32(coef)
    state = _state(dev, coef, gs)
    p0 = torch.randn(n, generator=g)
    p0[:2] = torch.tensor([1e-3, -2e-4])
    pr = p0.double().requires_grad_(True)
    opt = torch.optim.Adam([pr], lr=lrf, betas=(b1f, b2f), eps=epsf, weight_decay=wdf)
    p, m, v = p0.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    for step in range(1, 11):
        grad = torch.randn(n, generator=g) * (10.0 if step % 2 else 0.1)
        p_before = pr.detach().clone()
        st = opt.state[pr]
        m_before = st["exp_avg"].clone() if st else torch.zeros(n, dtype=torch.float64)
        v_before = st["exp_avg_sq"].clone() if st else torch.zeros(n, dtype=torch.float64)
        pr.grad = grad.double() * gsf * cf
        opt.step()
        hyper = _hyper(dev, [lr, 0.5], gs, clip_norm=1.0, betas=(b1, b2), step=step)
        ops.adam_ctl_(p, grad.to(dev), m, v, hyper, state, 0, beta1=b1, beta2=b2, eps=eps, weight_decay=wd)
        if step in (1, 2, 10):
            st = opt.state[pr]
            gp_abs = (grad.double() * gsf * cf).abs() + (wdf * p_before).abs()
            _check(m, st["exp_avg"], (b1f * m_before).abs() + (1 - b1f) * gp_abs, "adam_ctl_ exp_avg (step %d)" % step)
            _check(v, st["exp_avg_sq"], (b2f * v_before).abs() + (1 - b2f) * gp_abs * gp_abs, "adam_ctl_ exp_avg_sq (step %d)" % step)
            _check(p, pr.detach(), p_before.abs() + (pr.detach() - p_before).abs(), "adam_ctl_ p (step %d)" % step)
        with torch.no_grad():
            pr.copy_(p.double().cpu())
            opt.state[pr]["exp_avg"].copy_(m.double().cpu())
            opt.state[pr]["exp_avg_sq"].copy_(v.double().cpu())


# ---------------------------------------------------------------------------------------------------------------------
# 4. Trainer(clip_norm=c) against the reference's loop
# ---------------------------------------------------------------------------------------------------------------------
def _grad_total(model):
    """float64: sqrt of the summed squared gradient norms of the trainable parameters"""
    return math.sqrt(sum(float(p.grad.double().pow(2).sum()) for p in model.parameters()
                         if p.requires_grad and p.grad is not None))


def _clip_gradients(model, c):
    """net_utils.clip_gradient restated: scale every trainable parameter's gradient by c / max(total, c)"""
    total = _grad_total(model)
    scale = c / max(total, c)
    for p in model.parameters():
        if p.requires_grad and p.grad is not None:
            p.grad.mul_(scale)
    return total


@pytest.mark.parametrize("name", ["DAnA", "frcnn"])
def test_trainer_with_clip_norm_matches_the_reference_loop(dev, name):
    """two iterations of train.py:125-143 with the gradients clipped between backward and step (autograd bridge,
    torch.optim.SGD with train.py:76-87's groups) against Trainer(clip_norm=c).step, c = half the first iteration's
    unclipped norm. Compared are the parameter UPDATES of each iteration: at lr = 0.01 the parameters themselves barely
    tell a clipped trajectory from an unclipped one. The first iteration always clips (by a factor 2). Measured norms:
    frcnn 47.3 then 29.7 against c = 23.6, so its second iteration clips too; DAnA 129.8 then 31.5 against c = 64.9 -- the
    synthetic model's first update takes most of the gradient away, and DAnA's second iteration runs through the
    not-clipped branch (coef exactly 1) on a trajectory that still differs from the unclipped one through the momentum."""
    from dana_amd import synthetic as S
    from dana_amd.config import cfg
    from dana_amd.trainer import Trainer
    lr = 0.01
    if name == "DAnA":
        inputs = [t.to(dev) for t in S.episode_inputs(2, 2, 2, 160, 224, seed=6)]
    else:
        inputs = [t.to(dev) for t in S.episode_inputs(2, 2, 2, 192, 256, seed=23)[:4]]
    ma, mb, mc = (_model(dev, name, seed=5 if name == "DAnA" else 21) for _ in range(3))
    groups = []
    for key, value in dict(ma.named_parameters()).items():
        if value.requires_grad:
            if "bias" in key:
                groups.append({"params": [value], "lr": lr * (cfg.TRAIN.DOUBLE_BIAS + 1),
                               "weight_decay": cfg.TRAIN.BIAS_DECAY and cfg.TRAIN.WEIGHT_DECAY or 0})
            else:
                groups.append({"params": [value], "lr": lr, "weight_decay": cfg.TRAIN.WEIGHT_DECAY})
    opt = torch.optim.SGD(groups, momentum=cfg.TRAIN.MOMENTUM)
    names = [k for k, v in ma.named_parameters() if v.requires_grad]

    def snapshot(m):
        return {k: v.detach().clone() for k, v in m.named_parameters() if v.requires_grad}

    tr = None
    tc = Trainer(mc, lr)  # the unclipped trajectory
    c = None
    for it in range(2):
        before_a, before_c = snapshot(ma), snapshot(mc)
        np.random.seed(40 + it)
        ma.zero_grad()
        out = ma(*inputs)
        loss = out[3].mean() + out[4].mean() + out[5].mean() + out[6].mean()
        opt.zero_grad()
        loss.backward()
        if c is None:
            c = 0.5 * _grad_total(ma)
            tr = Trainer(mb, lr, clip_norm=c)
        total = _clip_gradients(ma, c)
        assert it > 0 or total > c, "the first iteration must clip (%g vs %g)" % (total, c)
        opt.step()
        before_b = snapshot(mb)
        np.random.seed(40 + it)
        tr.step(*inputs)
        np.random.seed(40 + it)
        tc.step(*inputs)
        torch.cuda.synchronize()
        after_a, after_b, after_c = snapshot(ma), snapshot(mb), snapshot(mc)
        upd_a = {k: after_a[k] - before_a[k] for k in names}
        tol = {k: 1e-6 + 1e-5 * upd_a[k].abs().max().item() for k in names}
        # first: the check can tell the two trajectories apart -- on every tensor listed here the comparison below would
        # fail for an unclipped trainer (tensors whose whole update is below 100x the 1e-6 floor cannot show it)
        apart = [k for k in names
                 if (upd_a[k] - (after_c[k] - before_c[k])).abs().max().item() >= 100 * tol[k]]
        print("CLIP %s it %d: total %.6g, c %.6g, %d of %d tensors tell clipped from unclipped" % (name, it, total, c,
                                                                                                len(apart), len(names)))
        biggest = max(names, key=lambda k: upd_a[k].abs().max().item())
        assert biggest in apart, (len(apart), len(names), biggest)
        for k in names:
            d = (upd_a[k] - (after_b[k] - before_b[k])).abs().max().item()
            assert d <= tol[k], (it, k, d, tol[k])
        got = float(tr.grad_norm().item())
        assert tr.grad_norm().numel() == 1 and tr.grad_norm().is_cuda
        assert abs(got - total) <= 1e-5 * total, (it, got, total)
    assert tr.steps == 2 and "clip_norm" not in tr.state_dict()


def test_upload_hyper_is_stream_ordered_across_many_iterations(dev, dana_trainer):
    """every upload takes fresh pinned staging memory: a burst of uploads without any synchronisation delivers each
    iteration's values to the work queued behind it, none overwritten by a later one"""
    tr = dana_trainer
    lr0 = tr.lr
    seen = torch.zeros(200, dtype=torch.float32, device=dev)
    try:
        for k in range(200):
            tr.lr = float(k + 1)
            tr.upload_hyper()
            seen[k:k + 1].copy_(tr._hyper[0:1], non_blocking=True)  # the weight group's rate
    finally:
        tr.lr = lr0
    torch.cuda.synchronize()
    assert torch.equal(seen.cpu(), torch.arange(1, 201, dtype=torch.float32))


# ---------------------------------------------------------------------------------------------------------------------
# 5.-7. replayed iterations: Adam, a learning-rate change, clipping
# ---------------------------------------------------------------------------------------------------------------------
def _runner(kind, trainer, inputs, **kw):
    if kind == "program":
        from dana_amd.program import ProgramTrainer
        return ProgramTrainer(trainer, *inputs, **kw)
    from dana_amd.graphs import GraphedTrainer
    return GraphedTrainer(trainer, *inputs, **kw)


def _replay_objects(kind, r):
    return [r.p1, r.p2] if kind == "program" else [r.graphs] + [g for g, _ in r.graphs]


def _adam_close(ma, mb, lr, what):
    pa, pb = dict(ma.named_parameters()), dict(mb.named_parameters())
    for k in pa:
        if k.endswith(ZERO_GRAD_BIASES) or not pa[k].requires_grad:
            continue
        diff = (pa[k].detach() - pb[k].detach()).abs()
        frac = (diff > 0.05 * lr).float().mean().item()
        assert frac <= 2e-3 and diff.mean().item() <= 2e-3 * lr, (what, k, frac, diff.max().item(), diff.mean().item())


@pytest.mark.parametrize("kind", ["program", "graph"])
def test_adam_in_replayed_iterations(dev, kind):
    """Trainer(optimizer='adam') under ProgramTrainer / GraphedTrainer: three replayed iterations against three eager ones
    from the same weights and np.random seeds (the rule of test_trainer_adam_matches_torch_adam), the step count advances,
    an eager step continues the trajectory, and constructing the runner (two eager warm-up iterations + the recording, which
    is one more) leaves parameters, both moments, the step count and the host RNG exactly where they were"""
    from dana_amd import synthetic as S
    from dana_amd.trainer import Trainer
    lr = 1e-3
    inputs = [t.to(dev) for t in S.episode_inputs(1, 2, 2, 160, 224, seed=6)]
    m0, m1 = _model(dev, ba=False), _model(dev, ba=False)
    t0, t1 = Trainer(m0, lr, optimizer="adam"), Trainer(m1, lr, optimizer="adam")
    before = _params(m1)
    np.random.seed(123)
    rng = np.random.get_state()[1].copy()
    r = _runner(kind, t1, inputs)
    torch.cuda.synchronize()
    assert np.array_equal(_params(m1), before) and t1.steps == 0
    assert np.array_equal(np.random.get_state()[1], rng)
    for b in t1.bufs + t1.bufs2:
        assert not b.any().item(), "the warm-up / recording left Adam state behind"
    for it in range(3):
        np.random.seed(40 + it)
        t0.step(*inputs)
        np.random.seed(40 + it)
        r.step(*inputs)
    torch.cuda.synchronize()
    assert t1.steps == 3 and t0.steps == 3
    assert all(b.any().item() for b in t1.bufs2)
    _adam_close(m0, m1, lr, "after three replays")
    np.random.seed(43)
    t0.step(*inputs)
    np.random.seed(43)
    t1.step(*inputs)
    torch.cuda.synchronize()
    assert t1.steps == 4
    _adam_close(m0, m1, lr, "after an eager step behind the replays")


@pytest.mark.parametrize("kind", ["program", "graph"])
def test_learning_rate_change_needs_no_rerecording(dev, kind):
    """two replays, trainer.adjust_learning_rate(0.1), two more replays with the SAME programs / graphs == the eager trainer
    on the same schedule. That the new rate was used: the last two updates of the largest weight tensor are 0.1x the first
    two within 20 %, each update measured against the step it came from, |dw| / |buf| with buf = g / world + wd * p
    (momentum = 0 here). The raw update norms cannot show it: the gradient of this synthetic model falls 15x from the first
    iteration to the second (measured |dw| = 1.19, 0.0785, 0.0033, 0.0032)."""
    from dana_amd import synthetic as S
    from dana_amd.trainer import Trainer
    inputs = [t.to(dev) for t in S.episode_inputs(1, 2, 2, 160, 224, seed=6)]
    m0, m1 = _model(dev), _model(dev)
    t0, t1 = Trainer(m0, 0.01, momentum=0.0), Trainer(m1, 0.01, momentum=0.0)
    r = _runner(kind, t1, inputs, warmup=1)
    objs = _replay_objects(kind, r)
    big = max((k for k, p in m1.named_parameters() if p.requires_grad and "bias" not in k),
              key=lambda k: dict(m1.named_parameters())[k].numel())
    w = dict(m1.named_parameters())[big]
    upd, rate = [], []
    for it in range(4):
        if it == 2:
            t0.adjust_learning_rate(0.1)
            t1.adjust_learning_rate(0.1)
        np.random.seed(40)
        t0.step(*inputs)
        w_before = w.detach().clone()
        np.random.seed(40)
        r.step(*inputs)
        upd.append((w.detach() - w_before).double().norm().item())
        rate.append(upd[-1] / t1._views(t1.bufs)[big].double().norm().item())
    torch.cuda.synchronize()
    now = _replay_objects(kind, r)
    assert len(now) == len(objs) and all(a is b for a, b in zip(now, objs)), "the runner re-recorded"
    ref, got = _params(m0), _params(m1)
    d = np.abs(got - ref).max()
    assert d <= 1e-6 + 1e-4 * np.abs(ref).max(), d
    ratio = (rate[2] + rate[3]) / (rate[0] + rate[1])
    print("LR %s: %s |dw| %s, |dw| / |buf| %s -> ratio %.4f" % (kind, big, ["%.4e" % u for u in upd],
                                                               ["%.4e" % u for u in rate], ratio))
    assert abs(ratio - 0.1) <= 0.2 * 0.1, (ratio, upd, rate)
    assert abs(t1.lr - 0.001) < 1e-12 and t1.steps == 4


_CLIP = {}


def _clip_threshold(dev, inputs):
    """a twentieth of the unclipped gradient norm of the first iteration (seed 40), measured once on a trainer of its own:
    the norm falls from 67 to 23 within two iterations on this synthetic model, and all five iterations shall clip"""
    from dana_amd.trainer import Trainer
    if "c" not in _CLIP:
        tp = Trainer(_model(dev), 0.01)
        np.random.seed(40)
        tp.step(*inputs)
        torch.cuda.synchronize()
        _CLIP["c"] = 0.05 * math.sqrt(sum(float(fb.grads.double().pow(2).sum()) for fb, _, _ in tp.groups))
    return _CLIP["c"]


@pytest.mark.parametrize("rccl", [False, True], ids=["single", "rccl1rank"])
@pytest.mark.parametrize("kind", ["program", "graph"])
def test_clipping_in_replayed_iterations(dev, kind, rccl):
    """Trainer(clip_norm=c) under ProgramTrainer / GraphedTrainer == the eager clipped trainer, grad_norm() included.
    rccl1rank: a 1-rank RCCL group with always_reduce: the norm launches sit behind every bucket's sum (program: behind
    the host callback that waits for the buckets; graphs: in the last graph, replayed behind the waits)"""
    import torch.distributed as dist
    from dana_amd import _lib, program, synthetic as S
    from dana_amd.trainer import Trainer
    if rccl:
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", "29677" if kind == "program" else "29679"
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        inputs = [t.to(dev) for t in S.episode_inputs(1, 2, 2, 160, 224, seed=6)]
        c = _clip_threshold(dev, inputs)
        m0, m1 = _model(dev), _model(dev)
        t0 = Trainer(m0, 0.01, bucket_bytes=8 << 20, clip_norm=c)
        t1 = Trainer(m1, 0.01, bucket_bytes=8 << 20, clip_norm=c, always_reduce=rccl)
        for it in range(2):  # eager clipped iterations first, as the replay tests of the unclipped trainer do
            np.random.seed(40 + it)
            t0.step(*inputs)
            np.random.seed(40 + it)
            t1.step(*inputs)
        r = _runner(kind, t1, inputs, warmup=0)
        assert t1.steps == 2
        if kind == "program":
            L = _lib.lib()
            prog = r.p2 if r.p2 is not None else r.p1
            waits = [i for i, e in enumerate(prog.entries) if e[0] == program._HOST and e[1] == r._wait_buckets]
            norms = [i for i, e in enumerate(prog.entries) if e[0] == program._CALL and e[1] is L.fn["dana_grad_sqnorm"]]
            prep = [i for i, e in enumerate(prog.entries) if e[0] == program._CALL and e[1] is L.fn["dana_optim_prepare"]]
            upd = [i for i, e in enumerate(prog.entries) if e[0] == program._CALL and e[1] is L.fn["dana_sgd_momentum_ctl"]]
            assert len(waits) == 1 and len(norms) == 2 and len(prep) == 1 and len(upd) == 2
            assert waits[0] < norms[0] < norms[1] < prep[0] < upd[0] < upd[1]
            if rccl:
                assert prog.stats["host_callbacks"] == 1 + len(t1.weights.buckets) + len(t1.biases.buckets)
        elif rccl:
            assert len(r.graphs) == 4 and sum(len(b) for _, b in r.graphs) >= 3
        for it in range(2, 5):
            np.random.seed(40 + it)
            t0.step(*inputs)
            n0 = float(t0.grad_norm().item())
            np.random.seed(40 + it)
            r.step(*inputs)
            n1 = float(r.trainer.grad_norm().item())
            assert n0 > c and abs(n1 - n0) <= 1e-5 * n0, (it, n0, n1, c)  # (RoIAlign-backward atomics are unordered)
        torch.cuda.synchronize()
        assert t1.steps == 5
        ref, got = _params(m0), _params(m1)
        d = np.abs(got - ref).max()
        assert d <= 1e-6 + 1e-4 * np.abs(ref).max(), d
    finally:
        if rccl:
            dist.destroy_process_group()
