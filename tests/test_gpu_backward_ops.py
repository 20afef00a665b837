"""Operator-level tests of the backward-side kernels (element-wise / reduction / pooling / optimizer glue of the training
step, include/dana_hip.h) that only the end-to-end gradient tests of test_gpu_backward.py reached before.

Every reference is a plain torch statement of the FORWARD operation in float64 on the CPU (and autograd through it for an
adjoint), on the float32 inputs converted to float64. Two kinds of assertion:
  * bit equality with torch float32 on the CPU where the operation is a move or ONE IEEE operation per element;
  * everywhere else a per-element bound  |got - ref| <= 1e-6 * mag + tiny,  mag = the float64 sum of the absolute values of
    the terms that make up that output element. Where an element is built from a difference that can cancel (x - mean in a
    BatchNorm, a / out_scale - ugamma * u in the attention adjoint) the terms are the operands of that difference, not its
    result. 1e-6: float32 sums of n <= 16384 products emulated in the kernels' orders stay below 2.2e-7 * mag against
    float64, while one dropped / doubled / misplaced term moves an element by about mag / n >= 6e-5 * mag -- so every
    reduction here has at most 16384 terms per output element. `tiny` (the smallest normal float32) only covers float64
    results below the float32 normal range.
Each bound check prints its worst err / bound; the figures measured on the MI355X are in EXPERIMENTS.md."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TINY = float(np.finfo(np.float32).tiny)
ROWS = [1, 2, 3, 5, 255, 256, 257, 1023]     # 256-row chunks, 4 row lanes
CHANS = [4, 36, 64, 68, 1024]                # 64-channel slabs (float4 kernels: channels % 4 == 0)
CHANS_ANY = [4, 36, 64, 68, 100, 1024]       # ... and 100 where % 4 is not required
LENGTHS = [1, 49, 63, 64, 65, 147, 400]      # one wave per row


def _ops():
    import dana_amd
    return dana_amd.ops


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _f32(x):
    return float(np.float32(x))


def _check(got, ref, mag, what, tiny=0.0):
    """|got - ref| <= 1e-6 * mag + tiny per element; prints and reports the worst err / bound"""
    got = got.detach().double().cpu().reshape(ref.shape)
    assert torch.isfinite(got).all(), "%s: non-finite result" % what
    err = (got - ref).abs()
    bound = 1e-6 * mag.expand_as(ref) + tiny
    inexact = torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err))  # (a zero bound asks for equality)
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), inexact)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print("ERR/BOUND %-44s %.4f" % (what, worst))
    assert worst <= 1.0, "%s: worst err / bound = %.3f (max err %.3e)" % (what, worst, float(err.max()))
    return worst


def _wide(t, ld, fill):
    """t [rows][c] placed in the first c columns of a [rows][ld] buffer filled with a sentinel"""
    buf = torch.full((t.size(0), ld), fill, dtype=t.dtype)
    buf[:, :t.size(1)] = t
    return buf


# ---------------------------------------------------------------------------------------------------------------------
# moves and single IEEE operations: the bits of torch float32 on the CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_relu_mask_bits(dev):
    """adjoint of F.relu (resnet.py:100) by autograd; activations exactly 0.0 and -0.0 give gradient 0 as torch does;
    ld_grad != ld_act, nothing outside the written columns changes"""
    ops = _ops()
    g = _gen(11)
    cases = [(r, c, c + 8, c + 4) for r in ROWS for c in (4, 68)] + [(5, c, c, c + 12) for c in CHANS] + \
            [(384, 1024, 1024, 2048), (1176, 512, 512, 512)]  # rpn_x [B*hw][512], an o3 inside a concat buffer
    for rows, c, ldg, lda in cases:
        act = torch.randn(rows, c, generator=g)
        act.view(-1)[::3] = 0.0
        act.view(-1)[1::7] = -0.0
        grad = torch.randn(rows, c, generator=g)
        a = act.clone().requires_grad_(True)
        F.relu(a).backward(grad)
        gb, ab = _wide(grad, ldg, 9.0).to(dev), _wide(act, lda, -3.0).to(dev)
        ops.relu_mask_(gb, ab, rows, c, ld_grad=ldg, ld_act=lda)
        assert torch.equal(gb[:, :c].cpu(), a.grad), (rows, c)
        assert (gb[:, c:] == 9.0).all() and torch.equal(ab.cpu(), _wide(act, lda, -3.0))
    # zero rows: dana_relu_mask returns OK before it looks at the pointers
    ops.lib().call("dana_relu_mask", None, None, 0, 64, 0, 0, ops._stream())


def test_mul_rows_bits_and_zero_rows_refused(dev):
    """y *= x (dana.py:155-156) over strided rows: one multiply per element"""
    from dana_amd._lib import DanaError
    ops = _ops()
    g = _gen(12)
    for rows, c, ldy, ldx in [(r, 68, 72, 80) for r in ROWS] + [(3, c, c + 4, c) for c in CHANS] + [(384, 1024, 2048, 1024)]:
        y, x = torch.randn(rows, c, generator=g), torch.randn(rows, c, generator=g)
        yb, xb = _wide(y, ldy, 9.0).to(dev), _wide(x, ldx, 2.0).to(dev)
        ops.mul_rows_(yb, xb, rows, c, ld_y=ldy, ld_x=ldx)
        assert torch.equal(yb[:, :c].cpu(), y * x) and (yb[:, c:] == 9.0).all(), (rows, c)
    y = torch.zeros(4, 64, device=dev)
    with pytest.raises(DanaError):  # dana_mul_rows checks rows > 0 before any launch
        ops.mul_rows_(y, y, 0, 64)


def test_axpy_rows(dev):
    """y (+)= alpha * x: alpha = 1 is one add (accumulate) or a copy (overwrite) -> torch's bits; alpha = 1 / shot
    (backward.shot_mean_backward) against float64, mag = |y| + |alpha x|"""
    ops = _ops()
    g = _gen(13)
    for rows, c, ldy, ldx in [(r, 36, 40, 44) for r in ROWS] + [(5, c, c, c + 4) for c in CHANS] + [(400, 1024, 1024, 1024)]:
        y, x = torch.randn(rows, c, generator=g), torch.randn(rows, c, generator=g)
        xb = _wide(x, ldx, 2.0).to(dev)
        for acc in (True, False):
            yb = _wide(y, ldy, 9.0).to(dev)
            ops.axpy_rows_(yb, xb, rows, c, ld_y=ldy, ld_x=ldx, alpha=1.0, accumulate=acc)
            assert torch.equal(yb[:, :c].cpu(), y + x if acc else x) and (yb[:, c:] == 9.0).all(), (rows, c, acc)
            yb = _wide(y, ldy, 9.0).to(dev)
            al = _f32(1.0 / 3.0)
            ops.axpy_rows_(yb, xb, rows, c, ld_y=ldy, ld_x=ldx, alpha=1.0 / 3.0, accumulate=acc)
            ref = (y.double() if acc else 0) + al * x.double()
            _check(yb[:, :c], ref, (y.double().abs() if acc else 0) + (al * x.double()).abs(), "axpy_rows_")
            assert (yb[:, c:] == 9.0).all()


def test_rowscale_scale_rows_add_pe_broadcast_bits(dev):
    """dW rows times the frozen-BN scale; RoI rows times their group's vector (meta.py:136-140); x + pe over row groups
    that sit apart (dana.py:103,126-130); the adjoint of a mean over positions (broadcast) -- one operation per element"""
    ops = _ops()
    g = _gen(14)
    for rows, cols in [(1, 7), (3, 100), (64, 9 * 64), (257, 36), (512, 2304)]:
        dw, sc = torch.randn(rows, cols, generator=g), torch.rand(rows, generator=g) + 0.5
        got = ops.rowscale_(dw.clone().to(dev), sc.to(dev), rows, cols)
        assert torch.equal(got.cpu(), dw * sc.view(-1, 1)), (rows, cols)
    for rows, rpg, c in [(1, 1, 4), (5, 2, 36), (255, 128, 68), (257, 64, 64), (256, 128, 2048)]:
        x, vec = torch.randn(rows, c, generator=g), torch.randn((rows + rpg - 1) // rpg, c, generator=g)
        got = ops.scale_rows_by_group(x.to(dev), vec.to(dev), rows, rpg, c)
        assert torch.equal(got.cpu(), x * vec.repeat_interleave(rpg, 0)[:rows]), (rows, rpg, c)
    for groups, rpg, L, c, gstride in [(1, 5, 5, 4, 20), (3, 49, 49, 36, 2 * 49 * 36), (2, 1200, 400, 1024, 2 * 1200 * 1024),
                                       (5, 3, 2, 68, 3 * 68 + 8)]:
        buf = torch.randn(groups * gstride, generator=g)
        pe = torch.randn(L, c, generator=g)
        out = torch.full((groups * rpg + 2, c), 9.0, device=dev)
        ops.add_pe_groups(buf.to(dev), pe.to(dev), groups, rpg, L, c, gstride, out)
        x = torch.stack([buf[i * gstride:i * gstride + rpg * c].view(rpg, c) for i in range(groups)])
        ref = x + pe.repeat((rpg + L - 1) // L, 1)[:rpg]
        assert torch.equal(out[:groups * rpg].cpu().view(groups, rpg, c), ref) and (out[groups * rpg:] == 9.0).all()
    for groups, pos, c in [(1, 1, 4), (3, 5, 36), (256, 16, 2048), (2, 400, 1024), (7, 49, 68)]:
        go = torch.randn(groups, c, generator=g)
        full = torch.zeros(groups, pos, c, requires_grad=True)
        full.sum(1).backward(go)  # alpha = 1: the adjoint of a sum over the positions, a copy per position
        fresh = ops.broadcast_rows(go.to(dev), groups, pos, c)
        assert torch.equal(fresh.cpu().view(groups, pos, c), full.grad)
        init = torch.randn(groups * pos, c, generator=g)
        acc = ops.broadcast_rows(go.to(dev), groups, pos, c, out=init.clone().to(dev))
        assert torch.equal(acc.cpu(), init + full.grad.view(-1, c))
        full = torch.zeros(groups, pos, c, dtype=torch.float64, requires_grad=True)
        full.mean(1).backward(go.double())  # alpha = 1 / positions: the adjoint of spatial_mean (dana.py:387-389)
        ref = full.grad.view(-1, c)
        got = ops.broadcast_rows(go.to(dev), groups, pos, c, alpha=1.0 / pos)
        _check(got, ref, ref.abs(), "broadcast_rows(alpha)")
        acc = ops.broadcast_rows(go.to(dev), groups, pos, c, alpha=1.0 / pos, out=init.clone().to(dev))
        _check(acc, init.double() + ref, init.double().abs() + ref.abs(), "broadcast_rows(alpha, accumulate)")


def test_scale_by_device_scalar_bits(dev):
    ops = _ops()
    g = _gen(15)
    for n in (1, 3, 255, 257, 70001):
        x, s = torch.randn(n, generator=g), torch.randn(1, generator=g)
        got = ops.scale_by_device_scalar_(x.clone().to(dev), s.to(dev))
        assert torch.equal(got.cpu(), x * s), n


def test_unpack_conv_weight_grad_and_dgrad_weight_bits(dev):
    """packed [O][KH][KW][I] -> OIHW (the .grad layout), overwrite and accumulate (one add); the data-gradient weights
    [I][KH][KW][O] = the spatially flipped, transposed filter -- what F.conv_transpose2d applies -- without a scale a pure
    permutation, with the frozen-BN scale one multiply"""
    ops = _ops()
    g = _gen(16)
    for O, I, k in [(1, 1, 1), (5, 3, 3), (72, 100, 3), (64, 256, 1), (33, 31, 7), (512, 1024, 3)]:
        w = torch.randn(O, I, k, k, generator=g)
        packed = w.permute(0, 2, 3, 1).reshape(O, k * k * I).contiguous()
        got = torch.full((O + 1, I, k, k), 9.0, device=dev)
        ops.unpack_conv_weight_grad(packed.to(dev), got, O, I, k, k, accumulate=False)
        assert torch.equal(got[:O].cpu(), w) and (got[O:] == 9.0).all(), (O, I, k)
        init = torch.randn(O, I, k, k, generator=g)
        got = ops.unpack_conv_weight_grad(packed.to(dev), init.clone().to(dev), O, I, k, k, accumulate=True)
        assert torch.equal(got.cpu(), init + w), (O, I, k)
        ref = w.flip(2, 3).permute(1, 2, 3, 0).reshape(I, k * k * O)
        wd = ops.conv2d_dgrad_weight(packed.to(dev), O, I, k, k)
        assert torch.equal(wd.cpu(), ref), (O, I, k)
        sc = torch.rand(O, generator=g) + 0.5
        wds = ops.conv2d_dgrad_weight(packed.to(dev), O, I, k, k, scale=sc.to(dev))
        assert torch.equal(wds.cpu(), (w * sc.view(-1, 1, 1, 1)).flip(2, 3).permute(1, 2, 3, 0).reshape(I, k * k * O))
        if O * I <= 7200:  # ... and it IS the adjoint's filter: conv on it == autograd of the forward conv (float64)
            x = torch.randn(1, I, 6, 5, generator=g, dtype=torch.float64, requires_grad=True)
            y = F.conv2d(x, w.double(), padding=k // 2)
            gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
            y.backward(gy)
            wt = ref.double().view(I, k, k, O).permute(0, 3, 1, 2)
            assert torch.allclose(F.conv2d(gy, wt, padding=k - 1 - k // 2), x.grad, rtol=1e-12, atol=1e-12)


def test_upsample_scatter_bits(dev):
    """data gradient of a strided 1x1 conv (resnet.py:71): autograd of x[:, ::s, ::s] in float32, then the ReLU adjoint
    of mask_act; odd input sizes leave rows / columns behind the last sample (zero)"""
    ops = _ops()
    g = _gen(17)
    for B, ih, iw, c, s in [(1, 1, 1, 4, 2), (2, 8, 7, 36, 2), (3, 7, 7, 1024, 2), (2, 38, 63, 512, 2), (1, 10, 11, 68, 3)]:
        oh, ow = (ih - 1) // s + 1, (iw - 1) // s + 1
        compact = torch.randn(B, oh, ow, c, generator=g)
        act = torch.randn(B, ih, iw, c, generator=g)
        act.view(-1)[::5] = 0.0
        x = torch.zeros(B, ih, iw, c, requires_grad=True)
        x[:, ::s, ::s].backward(compact)
        for mask in (None, act):
            out = torch.full((B * ih * iw + 3, c), 9.0, device=dev)
            cd, md = compact.to(dev), mask.to(dev) if mask is not None else None
            ops.lib().call("dana_upsample_scatter_nhwc", cd.data_ptr(), out.data_ptr(), md.data_ptr() if md is not None else None,
                           B, oh, ow, ih, iw, c, s, ops._stream())
            ref = x.grad if mask is None else torch.where(mask > 0, x.grad, torch.zeros(()))
            assert torch.equal(out[:B * ih * iw].cpu().view(B, ih, iw, c), ref), (B, ih, iw, c, s, mask is not None)
            assert (out[B * ih * iw:] == 9.0).all()


@pytest.mark.parametrize("case", [(1, 2, 2, 4, "randn"), (2, 7, 9, 36, "ties"), (3, 20, 20, 1024, "randn"), (2, 5, 4, 68, "ties"),
                                  (1, 21, 20, 64, "ties"), (2, 2, 3, 100, "randn")])
def test_maxpool2x2s2_and_adjoint_bits(dev, case):
    """nn.MaxPool2d(2) (meta.py:203,246) and its adjoint against F.max_pool2d + autograd in float32 on the CPU. Odd heights
    / widths: the last row / column is never read and gets gradient 0. Built ties (2 and 4 equal maxima per window, from
    small integers): the gradient goes to the FIRST maximum in row-major window order, as torch's CPU backward gives it"""
    ops = _ops()
    B, H, W, C, kind = case
    g = _gen(sum(case[:4]))
    if kind == "ties":
        x = torch.randint(0, 3, (B, C, H, W), generator=g).float()
        x[:, :, 0:2, 0:2] = 2.0     # four equal maxima
        x[:, :, 0:2, 2:4] = torch.tensor([[1.0, 2.0], [2.0, 0.0]])  # two, the first is the window's second element
    else:
        x = torch.randn(B, C, H, W, generator=g)
    xr = x.clone().requires_grad_(True)
    y = F.max_pool2d(xr, 2)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy)
    x_nhwc = x.permute(0, 2, 3, 1).reshape(-1, C).contiguous().to(dev)
    gy_nhwc = gy.permute(0, 2, 3, 1).reshape(-1, C).contiguous().to(dev)
    if C % 4 == 0:  # (the forward reads float4; the adjoint takes any channel count)
        out, oh, ow = ops.maxpool2x2s2(x_nhwc, B, H, W, C)
        assert (oh, ow) == tuple(y.shape[2:])
        assert torch.equal(out.cpu().view(B, oh, ow, C).permute(0, 3, 1, 2), y.detach())
    gin = ops.maxpool2x2s2_backward(x_nhwc, gy_nhwc, B, H, W, C)
    assert torch.equal(gin.cpu().view(B, H, W, C).permute(0, 3, 1, 2), xr.grad)
    if kind == "ties":
        assert (xr.grad[:, :, 0, 0] == gy[:, :, 0, 0]).all() and (xr.grad[:, :, 0, 3] == gy[:, :, 0, 1]).all()


def test_labels_posneg_bits(dev):
    """rois_label of dana.py:191-194: cat(labels.long(), zeros)"""
    ops = _ops()
    g = _gen(19)
    for n in (1, 3, 128, 257, 1024):
        lab = torch.randint(0, 3, (n,), generator=g).float()
        got = ops.labels_posneg(lab.to(dev))
        assert got.dtype == torch.int64 and torch.equal(got.cpu(), torch.cat([lab.long(), torch.zeros(n, dtype=torch.int64)]))


# ---------------------------------------------------------------------------------------------------------------------
# reductions over rows: 256-row chunks, 4 row lanes, 64-channel slabs
# ---------------------------------------------------------------------------------------------------------------------
def test_colsum_vs_fp64(dev):
    """bias gradients: out (+)= alpha * x.sum(0); row stride wider than the channels; accumulation from a non-zero buffer"""
    ops = _ops()
    g = _gen(21)
    for rows, c in [(r, c) for r in ROWS for c in (36, 64, 100)] + [(5, c) for c in CHANS_ANY] + \
                   [(256, 2), (2400, 1), (1176, 512), (16384, 4)]:  # d scores [n_roi][2], d unary [B*K1][1], rpn d_x
        ld = c + 3
        x = torch.randn(rows, c, generator=g)
        xb = _wide(x, ld, 1e3).to(dev)
        al = _f32(0.37)
        got = ops.colsum(xb, rows, c, ld=ld, alpha=0.37)
        _check(got, al * x.double().sum(0), abs(al) * x.double().abs().sum(0), "colsum")
        init = torch.randn(c, generator=g)
        got = ops.colsum(xb, rows, c, ld=ld, out=init.clone().to(dev))
        _check(got, init.double() + x.double().sum(0), init.double().abs() + x.double().abs().sum(0), "colsum(accumulate)")


def test_colsum_batched_vs_fp64(dev):
    """one matrix per image in one launch pair (the unary-term adjoint, backward.py _attention_backward)"""
    ops = _ops()
    g = _gen(22)
    for batch, rows, c, ld in [(2, 192, 1200, 1200), (3, 257, 147, 160), (1, 5, 36, 40), (5, 1023, 68, 72)]:
        x = torch.randn(batch, rows, ld, generator=g)
        init = torch.randn(batch, c + 4, generator=g)
        out = init.clone().to(dev)
        al = _f32(0.1 / 3)
        ops.colsum_batched(x.to(dev), batch, rows, c, out, ld=ld, x_batch=rows * ld, out_batch=c + 4, alpha=0.1 / 3)
        xs = x[:, :, :c].double()
        _check(out[:, :c], init[:, :c].double() + al * xs.sum(1), init[:, :c].double().abs() + abs(al) * xs.abs().sum(1),
               "colsum_batched")
        assert torch.equal(out[:, c:].cpu(), init[:, c:])


def test_batch_stats_vs_fp64(dev):
    """what nn.BatchNorm2d normalises with in train mode (fgn.py:147-153): x.mean(0), x.var(0, unbiased=False). Rows whose
    mean is large against their spread (mean 100, std 0.1): the two-pass variance holds the bound, E[x^2] - E[x]^2 (error
    ~ 6e-8 * 1e4 against a variance of 1e-2) could not. mag: sum |x| / R for the mean, the variance itself (a sum of
    squares) for the variance"""
    ops = _ops()
    g = _gen(23)
    for rows, c, shifted in [(r, c, False) for r in ROWS for c in (36, 64, 100)] + [(5, c, False) for c in CHANS_ANY] + \
                            [(6400, 512, False), (2304, 128, False), (1023, 68, True), (257, 100, True), (6400, 512, True)]:
        ld = c + 5
        x = torch.randn(rows, c, generator=g)
        if shifted:
            x = 100.0 + 0.1 * x
        mean, var = ops.batch_stats(_wide(x, ld, 1e3).to(dev), rows, c, ld=ld)
        xd = x.double()
        _check(mean, xd.mean(0), xd.abs().mean(0), "batch_stats mean" + (" (mean 100)" if shifted else ""))
        _check(var, xd.var(0, unbiased=False), xd.var(0, unbiased=False), "batch_stats var" + (" (mean 100)" if shifted else ""))


def test_bn_train_backward_vs_fp64_autograd(dev):
    """adjoint of F.batch_norm(x, None, None, gamma, beta, training=True) (fgn.py:147-153) by float64 autograd; the kernel gets
    the float32 rounding of the float64 batch statistics; grad_gamma / grad_beta are accumulated onto non-zero buffers.
    (Rows start at 2: torch refuses a train-mode BatchNorm over one value per channel.)
    mag, with xhat = (x - mean) * istd and its terms xh_abs = (|x| + |mean|) * istd (the difference cancels when the mean
    is large against the spread): dbeta: |init| + sum |g|; dgamma: |init| + sum |g| xh_abs;
    dx: gamma istd (|g| + sum|g| / R + xh_abs * sum(|g| xh_abs) / R)"""
    ops = _ops()
    g = _gen(24)
    eps = 1e-5
    for rows, c, shifted in [(r, c, False) for r in ROWS[1:] for c in (36, 64, 100)] + [(5, c, False) for c in CHANS_ANY] + \
                            [(6400, 512, False), (2304, 128, False), (1023, 68, True), (6400, 512, True)]:
        x = torch.randn(rows, c, generator=g)
        if shifted:
            x = 100.0 + 0.1 * x
        gy = torch.randn(rows, c, generator=g)
        gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
        gg0, gb0 = torch.randn(c, generator=g), torch.randn(c, generator=g)
        xd = x.double().requires_grad_(True)
        gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        F.batch_norm(xd, None, None, gd, bd, True, 0.1, eps).backward(gy.double())
        mean, var = x.double().mean(0), x.double().var(0, unbiased=False)
        gg, gb = gg0.clone().to(dev), gb0.clone().to(dev)
        gx = ops.bn_train_backward(gy.to(dev), x.to(dev), mean.float().to(dev), var.float().to(dev), gamma.to(dev), eps, rows, c,
                                   gg, gb)
        istd = 1.0 / torch.sqrt(var + _f32(eps))
        ga = gy.double().abs()
        xh_abs = (x.double().abs() + mean.abs()) * istd
        tag = " (mean 100)" if shifted else ""
        _check(gb, gb0.double() + bd.grad, gb0.double().abs() + ga.sum(0), "bn_train_backward dbeta" + tag)
        _check(gg, gg0.double() + gd.grad, gg0.double().abs() + (ga * xh_abs).sum(0), "bn_train_backward dgamma" + tag)
        mag = gamma.double() * istd * (ga + ga.sum(0) / rows + xh_abs * (ga * xh_abs).sum(0) / rows)
        _check(gx, xd.grad, mag, "bn_train_backward dx" + tag)


def test_scale_shift_relu_vs_fp64(dev):
    """relu?(x * scale + shift): a BatchNorm applied after the residual sum; mag |x scale| + |shift|"""
    ops = _ops()
    g = _gen(25)
    for rows, c in [(r, 68) for r in ROWS] + [(5, c) for c in CHANS] + [(6400, 512)]:
        x, sc, sh = torch.randn(rows, c, generator=g), torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
        for relu in (True, False):
            got = ops.scale_shift_relu_(x.clone().to(dev), sc.to(dev), sh.to(dev), rows, c, relu=relu)
            ref = x.double() * sc.double() + sh.double()
            _check(got, F.relu(ref) if relu else ref, (x.double() * sc.double()).abs() + sh.double().abs(), "scale_shift_relu_")
    ops.lib().call("dana_scale_shift_relu", None, None, None, 0, 64, 1, ops._stream())  # zero rows: OK, nothing launched


def test_rowdot_backward_vs_fp64_autograd(dev):
    """adjoint of nn.Linear(dim, 1) (rpn_unary_layer, dana.py:131): grad_w (+)= d^T x, grad_x += d (x) w, by autograd of
    F.linear; ld_x and ld_grad_x wider than the row, grad_x left out, grad_w accumulated"""
    ops = _ops()
    g = _gen(26)
    for rows, dim in [(r, d) for r in ROWS for d in (64, 100)] + [(5, d) for d in CHANS_ANY] + [(2400, 1024)]:
        ldx, ldg = dim + 4, dim + 8
        x, w, d = torch.randn(rows, dim, generator=g), torch.randn(1, dim, generator=g) * 0.03, torch.randn(rows, generator=g)
        gx0, gw0 = torch.randn(rows, dim, generator=g), torch.randn(dim, generator=g)
        xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
        F.linear(xd, wd).squeeze(1).backward(d.double())
        xb = _wide(x, ldx, 1e3).to(dev)
        gxb = _wide(gx0, ldg, 9.0).to(dev)
        gw = ops.rowdot_backward(xb, d.to(dev), w.to(dev), rows, dim, grad_x=gxb, ld_x=ldx, ld_grad_x=ldg)
        mag_w = (d.double().abs().view(-1, 1) * x.double().abs()).sum(0)
        _check(gw, wd.grad.view(-1), mag_w, "rowdot_backward dw")
        _check(gxb[:, :dim], gx0.double() + xd.grad, gx0.double().abs() + xd.grad.abs(), "rowdot_backward dx")
        assert (gxb[:, dim:] == 9.0).all()
        gw = ops.rowdot_backward(xb, d.to(dev), w.to(dev), rows, dim, grad_w=gw0.clone().to(dev), ld_x=ldx)  # no grad_x
        _check(gw, gw0.double() + wd.grad.view(-1), gw0.double().abs() + mag_w, "rowdot_backward dw(accumulate)")


# ---------------------------------------------------------------------------------------------------------------------
# one wave per row, 4 rows per block
# ---------------------------------------------------------------------------------------------------------------------
def test_softmax_rows_to_vs_fp64(dev):
    """cls_prob next to the untouched cls_score (dana.py:290-292): F.softmax(x, 1). mag = p * (1 + |x - max|): the
    exponential turns the rounding of its argument x - max (half an ulp of |x - max|) into that relative error"""
    ops = _ops()
    g = _gen(31)
    for rows, L in [(r, 2) for r in (1, 3, 5, 257)] + [(7, L) for L in LENGTHS] + [(256, 2), (6, 400)]:
        ldi, ldo = L + 3, L + 2
        x = torch.randn(rows, L, generator=g) * 2
        xb = _wide(x, ldi, 50.0).to(dev)
        out = torch.full((rows, ldo), 9.0, device=dev)
        ops.softmax_rows_to(xb, out, rows, L, ld_in=ldi, ld_out=ldo)
        p = F.softmax(x.double(), 1)
        _check(out[:, :L], p, p * (1 + (x.double() - x.double().max(1, keepdim=True)[0]).abs()), "softmax_rows_to", TINY)
        assert (out[:, L:] == 9.0).all() and torch.equal(xb.cpu(), _wide(x, ldi, 50.0))


def test_softmax_rows_backward_vs_fp64_autograd(dev):
    """adjoint of F.softmax over the last dim, in place on grad; prob = the float32 rounding of the float64 forward;
    ld_grad != ld_prob. mag = p (|g| + sum |p g|)"""
    ops = _ops()
    g = _gen(32)
    for rows, L in [(r, 49) for r in (1, 2, 3, 5, 257)] + [(7, L) for L in LENGTHS] + [(6, 400), (768, 49)]:
        ldg, ldp = L + 3, L + 1
        z = (torch.randn(rows, L, generator=g) * 2).double().requires_grad_(True)
        p = F.softmax(z, 1)
        gr = torch.randn(rows, L, generator=g)
        p.backward(gr.double())
        pf = p.detach().float()
        gb = _wide(gr, ldg, 9.0).to(dev)
        ops.softmax_rows_backward_(gb, _wide(pf, ldp, 7.0).to(dev), rows, L, ld_grad=ldg, ld_prob=ldp)
        pd = p.detach()
        mag = pd * (gr.double().abs() + (pd * gr.double().abs()).sum(1, keepdim=True))
        _check(gb[:, :L], z.grad, mag, "softmax_rows_backward_", TINY)
        assert (gb[:, L:] == 9.0).all()
    ops.lib().call("dana_softmax_rows_backward", None, None, 0, 49, 0, 0, ops._stream())  # zero rows: OK


def test_ba_block_adjoint_vs_fp64_autograd(dev):
    """adjoint of the BA block S' = S + gamma * F.leaky_relu(w^T S) (dana.py:133-137, w = the softmaxed channel weights, a
    saved forward result) by float64 autograd w.r.t. S and w: ba_backward_prep (w^T S and the column sums of dS' per
    group, 4 row lanes x 64-channel slabs) then ba_backward_ (one wave per row). One channel of S is all zero: the pooled
    value is exactly 0 there and the adjoint takes leaky_relu's slope, as torch does."""
    ops = _ops()
    g = _gen(33)
    gamma, slope = 0.1, 0.01
    for G, L, D in [(6, 400, 1024), (1, 1, 4), (3, 5, 36), (2, 255, 68), (2, 257, 100), (5, 49, 64), (1, 1023, 64), (3, 2, 1024)]:
        s = torch.randn(G, L, D, generator=g)
        s[:, :, D // 2] = 0.0
        w = F.softmax(torch.randn(G, L, generator=g).double(), 1).float()
        gs = torch.randn(G, L, D, generator=g)
        sd, wd = s.double().requires_grad_(True), w.double().requires_grad_(True)
        pooled = torch.bmm(wd.unsqueeze(1), sd)  # [G][1][D]
        (sd + _f32(gamma) * F.leaky_relu(pooled, _f32(slope))).backward(gs.double())
        sdev, wdev, gdev = s.to(dev), w.to(dev), gs.clone().to(dev)
        gvec, gsum = ops.ba_backward_prep(sdev, wdev, gdev, G, L, D)
        mag_v = torch.bmm(w.double().abs().unsqueeze(1), s.double().abs()).squeeze(1)
        _check(gvec, pooled.detach().squeeze(1), mag_v, "ba_backward_prep gvec")
        _check(gsum, gs.double().sum(1), gs.double().abs().sum(1), "ba_backward_prep gsum")
        assert (gvec[:, D // 2] == 0).all()
        dw = ops.ba_backward_(gdev, sdev, wdev, gvec, gsum, G, L, D, gamma=gamma, slope=slope)
        lk = torch.where(pooled.detach().squeeze(1) > 0, torch.ones(()).double(), torch.full((), _f32(slope)).double())
        dg_abs = (_f32(gamma) * lk * gs.double().abs().sum(1)).unsqueeze(1)  # [G][1][D]
        _check(gdev, sd.grad, gs.double().abs() + w.double().abs().unsqueeze(2) * dg_abs, "ba_backward_ dS")
        _check(dw.view(G, L), wd.grad, (s.double().abs() * dg_abs).sum(2), "ba_backward_ dw")


def test_attn_softmax_unary_backward_vs_fp64_autograd(dev):
    """adjoint of A = (softmax_seg(alpha * S) + ugamma * u) * out_scale (dana.py:143-146 / 274-278) w.r.t. S by float64
    autograd; the kernel gets a = the float32 rounding of the float64 forward, in place on dA [rows][ld]: pad columns
    nseg*length..kpad-1 come back zero, columns kpad..ld-1 stay. unary in the way-2 layout of
    test_attention_small_kernels_vs_torch (unary_batch_stride = 2 * nseg * length, second block used).
    mag: the kernel rebuilds p = a / out_scale - ugamma * u, a difference: p_abs = |a / out_scale| + |ugamma u|, then
    |alpha| p_abs (|dA| out_scale + sum_seg p_abs |dA| out_scale)"""
    ops = _ops()
    g = _gen(34)
    ug = 0.1
    for Bn, rows_b, nseg, L, kpad, ld in [(2, 192, 3, 400, 1200, 1200), (2, 49, 3, 49, 160, 160), (1, 5, 1, 1, 1, 4), (3, 7, 1, 63, 64, 72),
                                          (2, 3, 3, 64, 192, 200), (1, 6, 3, 65, 208, 208), (2, 5, 1, 147, 160, 176), (1, 2, 3, 49, 147, 147)]:
        rows, K = Bn * rows_b, nseg * L
        osc, alpha = _f32(1.0 / nseg), _f32(1.0 / math.sqrt(256))
        S = torch.randn(Bn, rows_b, K, generator=g) * 8  # (alpha * S has a spread of 0.5: a soft attention)
        un = F.softmax(torch.randn(Bn, 2 * nseg, L, generator=g), 2)
        u = un[:, nseg:].reshape(Bn, 1, K).double()
        Sd = S.double().requires_grad_(True)
        sm = torch.cat([F.softmax(alpha * Sd[:, :, i * L:(i + 1) * L], 2) for i in range(nseg)], 2)
        A = (sm + _f32(ug) * u) * osc
        dA = torch.randn(Bn, rows_b, K, generator=g)
        A.backward(dA.double())
        af = A.detach().float()
        gb = torch.full((rows, ld), 9.0)
        gb[:, :K] = dA.view(rows, K)
        ab = torch.zeros(rows, ld)
        ab[:, :K] = af.view(rows, K)
        gb, ab = gb.to(dev), ab.to(dev)
        ops.attn_softmax_unary_backward_(gb, ab, un.to(dev).view(-1)[nseg * L:], rows, rows_b, nseg, L, ld, kpad, ug, 1.0 / nseg,
                                         1.0 / math.sqrt(256), unary_batch_stride=2 * nseg * L)
        p_abs = (af.double() / osc).abs() + (_f32(ug) * u).abs()
        gabs = dA.double().abs() * osc
        dots = torch.cat([(p_abs[:, :, i * L:(i + 1) * L] * gabs[:, :, i * L:(i + 1) * L]).sum(2, keepdim=True).expand(-1, -1, L)
                          for i in range(nseg)], 2)
        _check(gb[:, :K], Sd.grad.view(rows, K), (alpha * p_abs * (gabs + dots)).view(rows, K), "attn_softmax_unary_backward_", TINY)
        assert (gb[:, K:kpad] == 0).all() and (gb[:, kpad:] == 9.0).all()


# ---------------------------------------------------------------------------------------------------------------------
# skinny GEMMs
# ---------------------------------------------------------------------------------------------------------------------
def _gemm_small_case(ops, dev, g, m, n, k, ta, tb, tc, accumulate, alpha):
    a, b = torch.randn(m, k, generator=g), torch.randn(k, n, generator=g)
    a_store, a_str = (a.t().contiguous(), (1, m)) if ta else (a, (k, 1))
    b_store, b_str = (b.t().contiguous(), (1, k)) if tb else (b, (n, 1))
    c0 = torch.randn(m, n, generator=g)
    al = _f32(alpha)
    ref = al * (a.double() @ b.double())
    mag = abs(al) * (a.double().abs() @ b.double().abs())
    if accumulate or tc:  # (the wrapper accumulates into a given buffer)
        ref, mag = ref + c0.double(), mag + c0.double().abs()
        c_store = (c0.t() if tc else c0).clone(memory_format=torch.contiguous_format).to(dev)
        got = ops.gemm_small(a_store.to(dev), a_str, b_store.to(dev), b_str, m, n, k, out=c_store,
                             c_strides=(1, m) if tc else (n, 1), alpha=alpha)
        got = got.t() if tc else got
    else:
        got = ops.gemm_small(a_store.to(dev), a_str, b_store.to(dev), b_str, m, n, k, alpha=alpha)
    return _check(got, ref, mag, "gemm_small" + ("(ksplit)" if k >= 64 and m <= 65535 else ""))


def test_gemm_small_vs_fp64(dev):
    """c (+)= alpha * a . b with element strides: the skinny heads' weight and data gradients. k walks the switch to the
    K-split kernel at 64 and every tail of its 8-step loop; m = 65536 with k = 64 falls back to one lane per element"""
    ops = _ops()
    g = _gen(41)
    # production (backward.seed_linear_grads / seed_linear_dx): d scores^T . hid  ((1, 2) / (nhid, 1)),  d bbox . W  ((4, 1) / (2048, 1))
    _gemm_small_case(ops, dev, g, 2, 1024, 256, True, False, False, False, 0.5)
    _gemm_small_case(ops, dev, g, 256, 2048, 4, False, False, False, False, 0.25)
    _gemm_small_case(ops, dev, g, 4, 2048, 256, True, False, False, False, 1.0)
    _gemm_small_case(ops, dev, g, 256, 1152, 2, False, False, False, False, 1.0)
    for k in (1, 2, 4, 63, 64, 65, 71, 72, 512):
        for n in (1, 2, 63, 65):
            for m, ta, tb, tc, acc in ((5, False, False, False, False), (3, True, True, True, True), (1, False, True, False, True)):
                _gemm_small_case(ops, dev, g, m, n, k, ta, tb, tc, acc, 0.7)
        _gemm_small_case(ops, dev, g, 2, 2048, k, True, False, False, k % 2 == 0, 1.0)
    _gemm_small_case(ops, dev, g, 65536, 2, 64, False, False, False, True, 1.0)
    _gemm_small_case(ops, dev, g, 65535, 2, 64, False, True, False, False, 1.0)
    ops.lib().call("dana_gemm_small", None, 1, 1, None, 1, 1, None, 1, 1, 0, 4, 4, 1.0, 0, ops._stream())  # m = 0: OK


# ---------------------------------------------------------------------------------------------------------------------
# pooling / correlation adjoints
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(2, 20, 20, 1024, 14, 1), (128, 7, 7, 256, 3, 1), (256, 3, 3, 1024, 3, 1), (2, 10, 10, 36, 3, 2),
                                  (3, 5, 7, 4, 2, 2), (1, 3, 3, 68, 1, 1)])
def test_avgpool_backward_vs_fp64_autograd(dev, case):
    """adjoint of F.avg_pool2d(x, k, stride) (dana.py:42 AvgPool2d(14, 1); fsod's 3x3 pools); 10x10 k3 s2: the last input
    row and column no window covers get 0. mag = the same adjoint applied to |grad| (its weights 1 / k^2 are positive)"""
    ops = _ops()
    B, H, W, C, k, s = case
    g = _gen(sum(case))
    x = torch.zeros(B, C, H, W, dtype=torch.float64, requires_grad=True)
    y = F.avg_pool2d(x, k, s)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy.double())
    ref = x.grad.clone()
    x.grad = None
    F.avg_pool2d(x, k, s).backward(gy.double().abs())
    got = ops.avgpool_backward(gy.permute(0, 2, 3, 1).contiguous().to(dev), B, H, W, C, k, s)
    _check(got.view(B, H, W, C).permute(0, 3, 1, 2), ref, x.grad, "avgpool_backward")
    if (H - k) % s:
        assert (got.view(B, H, W, C)[:, -1] == 0).all() and (got.view(B, H, W, C)[:, :, -1] == 0).all()


@pytest.mark.parametrize("case", [(256, 7, 7, 1024, 7, 7, 128, 0), (2, 12, 16, 1024, 7, 7, 1, 0), (7, 9, 8, 36, 3, 2, 3, 44),
                                  (5, 4, 4, 4, 1, 1, 2, 0), (3, 6, 5, 68, 6, 5, 1, 72)])
def test_depthwise_corr_and_adjoints_vs_fp64(dev, case):
    """F.conv2d(feat, kern.view(C, 1, kh, kw), groups=C) (fsod.py:109-116, 207-214) per kernel group and both adjoints by
    float64 autograd: n_roi 7x7 maps on 7x7 kernels (one kernel per image), B trunk maps on a 7x7 kernel; maps_per_kernel
    that does not divide n_maps; a feature row stride wider than the channels; need_feat=False; accumulation into a given
    grad_kernels. (The kernel gradient is ONE chain of maps_per_kernel * OH * OW terms: at most 16384 here.)"""
    ops = _ops()
    n, H, W, C, kh, kw, per, fs = case
    g = _gen(sum(case))
    nk = (n + per - 1) // per
    oh, ow = H - kh + 1, W - kw + 1
    assert per * oh * ow <= 16384
    feat = torch.randn(n, H, W, C, generator=g)
    kern = torch.randn(nk, kh, kw, C, generator=g)
    gy = torch.randn(n, oh, ow, C, generator=g)
    fd, kd = feat.double().requires_grad_(True), kern.double().requires_grad_(True)

    def fwd(f, kk):
        outs = [F.conv2d(f[i * per:(i + 1) * per].permute(0, 3, 1, 2), kk[i].permute(2, 0, 1).unsqueeze(1), groups=C) for i in range(nk)]
        return torch.cat(outs).permute(0, 2, 3, 1)

    ref = fwd(fd, kd)
    ref.backward(gy.double())
    fb = (_wide(feat.view(-1, C), fs, 1e3) if fs else feat.view(-1, C)).to(dev)
    kb = kern.view(nk, kh * kw, C).to(dev)
    out, oh2, ow2 = ops.depthwise_corr(fb, kb, n, H, W, C, kh, kw, maps_per_kernel=per, feat_stride=fs)
    assert (oh2, ow2) == (oh, ow)
    with torch.no_grad():
        _check(out.view(n, oh, ow, C), ref.detach(), fwd(feat.double().abs(), kern.double().abs()), "depthwise_corr")
    fa, ka = feat.double().abs().requires_grad_(True), kern.double().abs().requires_grad_(True)
    fwd(fa, ka).backward(gy.double().abs())  # (the adjoints are bilinear: their |.| sums are the adjoints of the |.| inputs)
    gf, gk = ops.depthwise_corr_backward(gy.view(-1, C).to(dev), fb, kb, n, H, W, C, kh, kw, maps_per_kernel=per, feat_stride=fs)
    _check(gf.view(n, H, W, C), fd.grad, fa.grad, "depthwise_corr_backward d feat")
    _check(gk.view(nk, kh, kw, C), kd.grad, ka.grad, "depthwise_corr_backward d kernels")
    init = torch.randn(nk, kh * kw, C, generator=g)
    gf2, gk2 = ops.depthwise_corr_backward(gy.view(-1, C).to(dev), fb, kb, n, H, W, C, kh, kw, maps_per_kernel=per, feat_stride=fs,
                                           need_feat=False, grad_kernels=init.clone().to(dev))
    assert gf2 is None
    _check(gk2.view(nk, kh, kw, C), init.double().view(nk, kh, kw, C) + kd.grad, init.double().abs().view(nk, kh, kw, C) + ka.grad,
           "depthwise_corr_backward d kernels(accumulate)")


def test_sigmoid_vs_fp64(dev):
    """nn.Sigmoid (meta.py:202,250), in place; mag = the result, `tiny` for results below the float32 normal range"""
    ops = _ops()
    g = _gen(51)
    for n in (1, 3, 255, 257, 2048 * 6, 100003):
        x = torch.randn(n, generator=g) * 4
        x[::11] = torch.linspace(-110.0, 110.0, x[::11].numel())
        x[:1] = 0.0
        got = ops.sigmoid_(x.clone().to(dev))
        ref = torch.sigmoid(x.double())
        _check(got, ref, ref, "sigmoid_", TINY)


# ---------------------------------------------------------------------------------------------------------------------
# optimizers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 1028, 1 << 20])
@pytest.mark.parametrize("wd,gs", [(0.0, 1.0), (1e-4, 0.125)])
def test_sgd_momentum_vs_torch_fp64(dev, n, wd, gs):
    """torch.optim.SGD(momentum, weight_decay) in float64 (train.py:76-87) for three consecutive steps on the float32
    hyper-parameters; first_step=True with the momentum buffer pre-filled with NaN: it must be ignored, as torch ignores an
    absent buffer. mag: |p| + |lr buf| for the parameter, |momentum buf| + |grad_scale g| + |wd p| for the buffer"""
    ops = _ops()
    g = _gen(n % 97 + 61)
    lr, mom = 1e-3, 0.9
    lrf, momf, wdf, gsf = _f32(lr), _f32(mom), _f32(wd), _f32(gs)
    p0 = torch.randn(n, generator=g)
    pr = p0.double().requires_grad_(True)
    opt = torch.optim.SGD([pr], lr=lrf, momentum=momf, weight_decay=wdf)
    p, buf = p0.clone().to(dev), torch.full((n,), float("nan"), device=dev)
    for step in range(3):
        grad = torch.randn(n, generator=g)
        p_before = pr.detach().clone()
        b_before = opt.state[pr]["momentum_buffer"].clone() if step else torch.zeros(n, dtype=torch.float64)
        pr.grad = grad.double() * gsf
        opt.step()
        ops.sgd_momentum_(p, grad.to(dev), buf, lr, mom, wd, grad_scale=gs, first_step=(step == 0))
        b_ref = opt.state[pr]["momentum_buffer"]
        mag_b = (momf * b_before).abs() + (grad.double() * gsf).abs() + (wdf * p_before).abs()
        _check(buf, b_ref, mag_b, "sgd_momentum_ buf (step %d)" % (step + 1))
        _check(p, pr.detach(), p_before.abs() + (lrf * b_ref).abs(), "sgd_momentum_ p (step %d)" % (step + 1))
        # the next step starts from the kernel's own float32 state on both sides
        with torch.no_grad():
            pr.copy_(p.double().cpu())
            opt.state[pr]["momentum_buffer"].copy_(buf.double().cpu())


@pytest.mark.parametrize("n", [4, 1028, 1 << 20])
@pytest.mark.parametrize("wd,gs", [(0.0, 1.0), (1e-4, 0.125)])
def test_adam_vs_torch_fp64(dev, n, wd, gs):
    """torch.optim.Adam in float64 (train.py:84-85) on the float32 hyper-parameters, steps 1, 2 and 10 with the state
    carried over (both sides continue from the kernel's float32 state, so every step is checked on its own).
    mag: |beta1 m| + |(1 - beta1) g'| and |beta2 v| + |(1 - beta2) g'^2| for the moments, |p| + |update| for the parameter"""
    ops = _ops()
    g = _gen(n % 97 + 71)
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    lrf, b1f, b2f, epsf, wdf, gsf = _f32(lr), _f32(b1), _f32(b2), _f32(eps), _f32(wd), _f32(gs)
    p0 = torch.randn(n, generator=g)
    p0[:2] = torch.tensor([1e-3, -2e-4])  # parameters of the size of one update
    pr = p0.double().requires_grad_(True)
    opt = torch.optim.Adam([pr], lr=lrf, betas=(b1f, b2f), eps=epsf, weight_decay=wdf)
    p, m, v = p0.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    for step in range(1, 11):
        grad = torch.randn(n, generator=g) * (10.0 if step % 2 else 0.1)
        p_before = pr.detach().clone()
        st = opt.state[pr]
        m_before = st["exp_avg"].clone() if st else torch.zeros(n, dtype=torch.float64)
        v_before = st["exp_avg_sq"].clone() if st else torch.zeros(n, dtype=torch.float64)
        pr.grad = grad.double() * gsf
        opt.step()
        ops.adam_(p, grad.to(dev), m, v, lr, step, beta1=b1, beta2=b2, eps=eps, weight_decay=wd, grad_scale=gs)
        if step in (1, 2, 10):
            st = opt.state[pr]
            assert int(st["step"]) == step
            gp_abs = (grad.double() * gsf).abs() + (wdf * p_before).abs()
            _check(m, st["exp_avg"], (b1f * m_before).abs() + (1 - b1f) * gp_abs, "adam_ exp_avg (step %d)" % step)
            _check(v, st["exp_avg_sq"], (b2f * v_before).abs() + (1 - b2f) * gp_abs * gp_abs, "adam_ exp_avg_sq (step %d)" % step)
            _check(p, pr.detach(), p_before.abs() + (pr.detach() - p_before).abs(), "adam_ p (step %d)" % step)
        with torch.no_grad():
            pr.copy_(p.double().cpu())
            opt.state[pr]["exp_avg"].copy_(m.double().cpu())
            opt.state[pr]["exp_avg_sq"].copy_(v.double().cpu())


def test_optimizers_refuse_misaligned_segments(dev):
    """both kernels cast to float4*: a view that starts 4 bytes into an allocation is refused by the host-side check,
    before any launch; so is a length that is not a multiple of 4"""
    from dana_amd._lib import DanaError
    ops = _ops()
    base = [torch.zeros(64, device=dev) for _ in range(4)]
    ok = [b[4:12] for b in base]
    ops.adam_(ok[0], ok[1], ok[2], ok[3], 1e-3, 1)          # 16 bytes in: fine
    ops.sgd_momentum_(ok[0], ok[1], ok[2], 1e-3, 0.9, 0.0)
    for i in range(4):
        args = [b[4:12] for b in base]
        args[i] = base[i][1:9]
        with pytest.raises(DanaError):
            ops.adam_(args[0], args[1], args[2], args[3], 1e-3, 1)
        if i < 3:
            with pytest.raises(DanaError):
                ops.sgd_momentum_(args[0], args[1], args[2], 1e-3, 0.9, 0.0)
    with pytest.raises(DanaError):
        ops.adam_(base[0][:6], base[1][:6], base[2][:6], base[3][:6], 1e-3, 1)
    with pytest.raises(DanaError):
        ops.adam_(ok[0], ok[1], ok[2], ok[3], 1e-3, 0)       # steps count from 1
    assert all(float(b.abs().max()) == 0 for b in base[2:])
