"""Operator-level tests of the forward-side light kernels (csrc/attention.hip, csrc/elementwise.hip, csrc/class_sweep.hip)
and of the fused proposal layer (csrc/proposal.hip), at the edges of their launch geometry and on every kernel their entry
points can dispatch to. The conventions are those of test_gpu_backward_ops.py, whose `_check` and `_wide` are used here:
  * every reference is a plain float64 torch / numpy statement of the operation, computed on the CPU from the float32 inputs;
  * bit equality with torch float32 where the operation is a move or ONE IEEE operation per element;
  * everywhere else  |got - ref| <= 1e-6 * mag + tiny  per element, mag = the float64 sum of the absolute values of the
    terms of that element (the operands of a difference that can cancel; p * (1 + |x - max|) for a softmax); every
    reduction has at most 16384 terms per output element, so that file's reasoning for 1e-6 holds here as well;
  * wide row strides carry a sentinel, and everything outside the written columns must come back unchanged.
Where an entry point chooses between kernels, the parametrisation names the kernel and the test derives it again from
the dispatch conditions of the source (restated in the `_*_path` helpers below).
The proposal layer is exact: its result must equal, bit for bit, numpy's stable sort + a float64 greedy NMS on the
device-decoded boxes. Each bound check prints its worst err / bound; the figures measured on the MI355X are in
EXPERIMENTS.md."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_backward_ops import TINY, _check, _f32, _gen, _ops, _wide  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS = [1, 2, 3, 5, 255, 257]  # one wave per row, 4 rows per block


def _softmax_mag(x, p, dim):
    return p * (1 + (x - x.max(dim, keepdim=True)[0]).abs())


# ---------------------------------------------------------------------------------------------------------------------
# one wave per row: rowdot, softmax_rows_, attn_softmax_unary_
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [4, 36, 256, 260, 1024])  # float4 counts 1, 9, 64, 65, 256: below / at / above 64 lanes
def test_rowdot_vs_fp64(dev, dim):
    """nn.Linear(dim, 1) (dana.py:131): x . w + b over rows ld = dim + 8 apart, with and without the bias"""
    ops = _ops()
    g = _gen(100 + dim)
    ld = dim + 8
    for rows in ROWS + ([2400] if dim == 1024 else []):  # (production: 6 * 400 support positions)
        x, w, b = torch.randn(rows, dim, generator=g), torch.randn(dim, generator=g), torch.randn(1, generator=g)
        xb = _wide(x, ld, 1e3).to(dev)
        dot, mag = x.double() @ w.double(), x.double().abs() @ w.double().abs()
        got = ops.rowdot(xb, w.to(dev), b.to(dev), rows, dim, ld=ld)
        _check(got, dot + b.double(), mag + b.double().abs(), "rowdot(bias) dim %d" % dim)
        got = ops.rowdot(xb, w.to(dev), None, rows, dim, ld=ld)
        _check(got, dot, mag, "rowdot(no bias) dim %d" % dim)
        assert torch.equal(xb.cpu(), _wide(x, ld, 1e3))


@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 400, 2394])
def test_softmax_rows_vs_fp64(dev, L):
    """F.softmax(x, 1) in place (dana.py:134,144; 2394 = the 38 x 63 query positions), ld = L + 3"""
    ops = _ops()
    g = _gen(200 + L)
    ld = L + 3
    for rows in ROWS:
        for scale in (2.0, 20.0) if rows == 5 else (2.0,):  # x 20: |x - max| up to ~100, the bound's second term matters
            x = torch.randn(rows, L, generator=g) * scale
            xb = _wide(x, ld, 50.0).to(dev)
            ops.softmax_rows_(xb, rows, L, ld=ld)
            p = F.softmax(x.double(), 1)
            _check(xb[:, :L], p, _softmax_mag(x.double(), p, 1), "softmax_rows_ L %d%s" % (L, " (x20)" if scale > 2 else ""), TINY)
            assert (xb[:, L:] == 50.0).all()


def _attn_path(L):
    """attn_softmax_unary_kernel: `if (L <= 64 * RV)`, RV = 8, keeps a segment in registers; otherwise the loops"""
    return "registers" if L <= 64 * 8 else "loop"


@pytest.mark.parametrize("nseg", [1, 3])
@pytest.mark.parametrize("L,path", [(1, "registers"), (49, "registers"), (64, "registers"), (65, "registers"), (400, "registers"),
                                    (512, "registers"), (513, "loop"), (600, "loop")])
def test_attn_softmax_unary_vs_fp64(dev, L, path, nseg):
    """A = (softmax_seg(S) + ugamma * u) * out_scale (dana.py:143-146, 274-278) in place on rows ld apart. 10 rows in
    batches of 5: the block of rows 4..7 spans both batches' unary terms, which sit unary_batch_stride > nseg * L apart.
    Columns nseg*L .. kpad-1 come back zero, columns kpad .. ld-1 untouched. L = 512 and 513 sit on either side of the
    switch between the two paths: both meet the float64 reference under the same bound.
    mag = (p (1 + |x - max|) + |ugamma u|) * out_scale"""
    assert _attn_path(L) == path
    ops = _ops()
    g = _gen(300 + 7 * L + nseg)
    rows, rpb = 10, 5
    K = nseg * L
    kpad = (K + 7) // 8 * 8
    ld, ubs = kpad + 8, K + 5
    ug, osc = _f32(0.1), _f32(1.0 / nseg)
    x = torch.randn(rows, nseg, L, generator=g) * 2
    u = torch.rand(rows // rpb, ubs, generator=g)
    xb = _wide(x.view(rows, K), ld, 9.0).to(dev)
    ops.attn_softmax_unary_(xb, u.to(dev), rows, rpb, nseg, L, ld, kpad, 0.1, 1.0 / nseg, unary_batch_stride=ubs)
    xd = x.double()
    p = F.softmax(xd, 2)
    ud = u[:, :K].double().reshape(rows // rpb, 1, nseg, L).expand(-1, rpb, -1, -1).reshape(rows, nseg, L)
    ref = (p + ug * ud) * osc
    mag = (_softmax_mag(xd, p, 2) + (ug * ud).abs()) * osc
    _check(xb[:, :K], ref.view(rows, K), mag.view(rows, K), "attn_softmax_unary_ (%s) L %d nseg %d" % (path, L, nseg), TINY)
    assert (xb[:, K:kpad] == 0).all() and (xb[:, kpad:] == 9.0).all()


# ---------------------------------------------------------------------------------------------------------------------
# BA block: 64-channel slabs x 16 row groups
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("D", [4, 36, 64, 68, 1024])  # 36, 68: the last slab's float4 lanes with d + 3 >= D do nothing
@pytest.mark.parametrize("L", [1, 15, 16, 17, 49, 400])  # below 16: row groups without a row
def test_ba_apply_vs_fp64(dev, L, D, G):
    """S += gamma * leaky_relu(w^T S) (dana.py:133-137) on rows ld = D + 4 apart. Channel 0 is positive and channel 1
    negative in every row (w > 0), so both branches of the leaky ReLU occur in every case.
    mag = |S| + gamma * sum_l |w S|"""
    ops = _ops()
    g = _gen(400 + 31 * L + D + G)
    gamma, slope = _f32(0.1), _f32(0.01)
    ld = D + 4
    s = torch.randn(G, L, D, generator=g)
    s[:, :, 0] = s[:, :, 0].abs() + 0.5
    s[:, :, 1] = -s[:, :, 1].abs() - 0.5
    w = F.softmax(torch.randn(G, L, generator=g).double(), 1).float()
    sd, wd = s.double(), w.double()
    pooled = torch.bmm(wd.unsqueeze(1), sd)  # [G][1][D]
    assert (pooled > 0).any() and (pooled < 0).any()
    ref = sd + gamma * F.leaky_relu(pooled, slope)
    mag = sd.abs() + gamma * torch.bmm(wd.unsqueeze(1), sd.abs())
    sb = _wide(s.view(G * L, D), ld, 9.0).to(dev)
    ops.ba_apply_(sb, w.to(dev), G, L, D, ld=ld, gamma=0.1, slope=0.01)
    got = sb[:, :D].cpu().view(G, L, D)
    _check(got, ref, mag, "ba_apply_ L %d D %d" % (L, D))
    neg = (pooled < 0).expand_as(ref)
    _check(got[neg], ref[neg], mag[neg], "ba_apply_ (negative total) L %d D %d" % (L, D))
    assert (sb[:, D:] == 9.0).all()


# ---------------------------------------------------------------------------------------------------------------------
# pooling and means
# ---------------------------------------------------------------------------------------------------------------------
def _avgpool_path(H, W, C, k, stride):
    """the dispatch of dana_avgpool_nhwc (AP_CH4 = 4 float4s per workgroup, 16 bytes per float4)"""
    ow = (W - k) // stride + 1
    tile_lds = (H * W + H * ow) * 4 * 16
    if stride == 1 and (C // 4) % 4 == 0 and tile_lds <= 48 * 1024 and H * W >= 64:
        return "tile"
    if stride == 1 and ow <= 8:
        return "rows"
    return "generic"


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("path,H,W,k,stride,C", [
    ("tile", 20, 20, 14, 1, 16), ("tile", 20, 20, 14, 1, 1024), ("tile", 8, 8, 3, 1, 16),
    ("rows", 7, 7, 3, 1, 256), ("rows", 3, 3, 3, 1, 1024), ("rows", 10, 10, 3, 1, 4),  # 10x10: OW = 8, the rows kernel's last
    ("generic", 11, 11, 3, 1, 4), ("generic", 9, 9, 3, 2, 16), ("generic", 24, 24, 3, 1, 16)])  # OW 9; stride 2; LDS 70 656 B
def test_avgpool_vs_fp64(dev, path, H, W, k, stride, C, B):
    """F.avg_pool2d(x, k, stride) (dana.py:42 AvgPool2d(14, 1); fsod.py:157-160's 3x3 pools) on each of the three kernels.
    Inputs of mean 10: one dropped or doubled tap moves an element by 10 / k^2 >= 5e-3 * mag. mag = avgpool of |x|"""
    assert _avgpool_path(H, W, C, k, stride) == path
    ops = _ops()
    g = _gen(500 + H + W + C + B)
    x = 10.0 + torch.randn(B, C, H, W, generator=g)
    got = ops.avgpool(x.permute(0, 2, 3, 1).contiguous().to(dev), B, H, W, C, k, stride)
    ref = F.avg_pool2d(x.double(), k, stride)
    oh, ow = ref.shape[2:]
    _check(got.view(B, oh, ow, C).permute(0, 3, 1, 2), ref, F.avg_pool2d(x.double().abs(), k, stride), "avgpool (%s)" % path)


def _colmean_path(L, G):
    """dana_colmean_sub: `length <= 1024 && groups <= 65535` takes colmean_fused_kernel, else partial + apply"""
    return "fused" if L <= 1024 and G <= 65535 else "two-pass"


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("L,path", [(1, "fused"), (63, "fused"), (64, "fused"), (65, "fused"), (1024, "fused"), (1025, "two-pass"),
                                    (2394, "two-pass")])  # 64-row chunks; 2394 = the query side of dana.py:1265
def test_colmean_sub_vs_fp64(dev, L, path, G):
    """q - q.mean(1, keepdim=True) (dana.py:125,141,267,272) in place, ld = D + 5; D not a multiple of the 64-column slab.
    mag = |x| + mean |x|: the operands of the difference"""
    assert _colmean_path(L, G) == path
    ops = _ops()
    g = _gen(600 + L + G)
    for D, shifted in [(d, False) for d in (4, 36, 64, 68, 100, 256)] + [(68, True)]:  # (mean 100, std 0.1: the difference cancels)
        ld = D + 5
        x = torch.randn(G, L, D, generator=g)
        if shifted:
            x = 100.0 + 0.1 * x
        xb = _wide(x.view(G * L, D), ld, 1e3).to(dev)
        ops.colmean_sub_(xb, G, L, D, ld=ld)
        xd = x.double()
        _check(xb[:, :D].cpu().view(G, L, D), xd - xd.mean(1, keepdim=True), xd.abs() + xd.abs().mean(1, keepdim=True),
               "colmean_sub_ (%s)%s" % (path, " (mean 100)" if shifted else ""))
        assert (xb[:, D:] == 1e3).all()


@pytest.mark.parametrize("C", [4, 68, 2048])
@pytest.mark.parametrize("P", [1, 16, 49, 2394])
def test_spatial_mean_vs_fp64(dev, P, C):
    """.mean(3).mean(2) (dana.py:387-389) over pixels in_stride = C + 4 apart; mag = mean |x|"""
    ops = _ops()
    g = _gen(700 + P + C)
    groups = 3
    x = torch.randn(groups * P, C, generator=g)
    got = ops.spatial_mean(_wide(x, C + 4, 1e3).to(dev), groups, P, C, in_stride=C + 4)
    xd = x.double().view(groups, P, C)
    _check(got, xd.mean(1), xd.abs().mean(1), "spatial_mean P %d" % P)


@pytest.mark.parametrize("case", [(2, 3, 3, 4), (1, 4, 4, 68), (3, 5, 6, 36), (2, 7, 8, 64), (2, 8, 7, 4), (1, 75, 125, 64)])
def test_maxpool3x3s2_ceil_bits(dev, case):
    """nn.MaxPool2d(3, 2, ceil_mode=True) (resnet.py:113) against F.max_pool2d: windows clipped at the bottom / right
    edge. All-negative inputs: a maximum started from zero, or a window padded with zeros, would win every comparison"""
    ops = _ops()
    B, H, W, C = case
    g = _gen(800 + sum(case))
    x = -torch.rand(B, C, H, W, generator=g) - 0.5
    ref = F.max_pool2d(x, 3, 2, ceil_mode=True)
    out, oh, ow = ops.maxpool3x3s2_ceil(x.permute(0, 2, 3, 1).contiguous().to(dev), B, H, W, C)
    assert (oh, ow) == tuple(ref.shape[2:])
    assert torch.equal(out.cpu().view(B, oh, ow, C).permute(0, 3, 1, 2), ref)


# ---------------------------------------------------------------------------------------------------------------------
# moves and single IEEE operations: the bits of torch float32 on the CPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 49, 400])
def test_add_pe_strided_bits(dev, L):
    """x + pe over rows = 3 * L (PositionalEncoding.forward, dana.py:322-324), strided input and strided output"""
    ops = _ops()
    g = _gen(900 + L)
    for C in (4, 68, 1024):
        rows, ldi, ldo = 3 * L, C + 4, C + 8
        x, pe = torch.randn(rows, C, generator=g), torch.randn(L, C, generator=g)
        xb = _wide(x, ldi, 1e3).to(dev)
        out = torch.full((rows, ldo), 9.0, device=dev)
        ops.add_pe(xb, pe.to(dev), rows, L, C, in_stride=ldi, out=out, out_stride=ldo)
        assert torch.equal(out.cpu(), _wide(x + pe.repeat(3, 1), ldo, 9.0)), (L, C)
        assert torch.equal(xb.cpu(), _wide(x, ldi, 1e3))


def _nchw_to_nhwc_path(B, C, HW, cpad, out_stride):
    """dana_nchw_to_nhwc: the 3 -> 4 channel kernel needs C = 3, cpad = 4 and a pixel stride of exactly 4"""
    return "fast" if C == 3 and cpad == 4 and (out_stride or cpad) == 4 and B * HW < (1 << 31) else "generic"


@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (97, 131)])  # 1, 35 and 12 707 pixels
@pytest.mark.parametrize("path,C,cpad,out_stride", [("fast", 3, 4, 0), ("generic", 3, 8, 0), ("generic", 5, 8, 0), ("generic", 64, 64, 0),
                                                    ("generic", 3, 4, 8), ("generic", 5, 8, 12)])
def test_nchw_to_nhwc_bits(dev, path, C, cpad, out_stride, H, W):
    """[B][C][H][W] -> pixels of out_stride floats: channels C .. cpad-1 zero, everything from cpad on untouched"""
    assert _nchw_to_nhwc_path(2, C, H * W, cpad, out_stride) == path
    ops = _ops()
    g = _gen(1000 + C + cpad + H)
    B, ldo = 2, out_stride or cpad
    x = torch.randn(B, C, H, W, generator=g)
    out = torch.full((B * H * W, ldo), 9.0, device=dev)  # (torch allocations are 16-byte aligned: the fast path's store)
    assert out.data_ptr() % 16 == 0
    ops.nchw_to_nhwc(x.to(dev), cpad=cpad, out=out, out_stride=out_stride)
    ref = torch.full((B * H * W, ldo), 9.0)
    ref[:, :cpad] = 0.0
    ref[:, :C] = x.permute(0, 2, 3, 1).reshape(-1, C)
    assert torch.equal(out.cpu(), ref)


@pytest.mark.parametrize("case", [(2, 5, 3, 7), (1, 64, 5, 7), (3, 1, 1, 1), (2, 1024, 7, 9)])
def test_nhwc_to_nchw_bits(dev, case):
    """pixels in_stride = C and C + 4 floats apart -> [B][C][H][W]"""
    ops = _ops()
    B, C, H, W = case
    g = _gen(1100 + sum(case))
    x = torch.randn(B, C, H, W, generator=g)
    rows = x.permute(0, 2, 3, 1).reshape(-1, C)
    for ldi in (C, C + 4):
        xb = _wide(rows, ldi, 1e3).to(dev)
        got = ops.nhwc_to_nchw(xb, B, C, H, W, in_stride=0 if ldi == C else ldi)
        assert torch.equal(got.cpu(), x), (case, ldi)
        got = ops.nhwc_to_nchw(xb, B, C, H, W, in_stride=ldi)
        assert torch.equal(got.cpu(), x), (case, ldi)


@pytest.mark.parametrize("R", [1, 31, 32, 33, 49, 400])
def test_transpose_batched_bits(dev, R):
    """in[g][R][C] -> out[g][C][ldo] through 32 x 32 tiles, 3 groups whose blocks sit further apart than a dense block
    (dana.py:1486-1495 passes in_batch = way * shot * P2 * dim). ldo = R writes no zero tail; ldo > R writes zeros in
    exactly columns R .. ldo-1; the input rows are ldi = C + 4 apart. Nothing else of the output buffer changes."""
    ops = _ops()
    g = _gen(1200 + R)
    groups = 3
    for C in (1, 31, 32, 33, 49, 400):
        for ldo in (R, R + 1, (R // 8 + 1) * 8):
            ldi = C + 4
            in_batch, out_batch = R * ldi + 8, C * ldo + 12
            x = torch.randn(groups, R, C, generator=g)
            xb = torch.full((groups * in_batch,), 1e3)
            ref = torch.full((groups * out_batch,), 9.0)
            for i in range(groups):
                xb[i * in_batch:i * in_batch + R * ldi].view(R, ldi)[:, :C] = x[i]
                blk = ref[i * out_batch:i * out_batch + C * ldo].view(C, ldo)
                blk[:] = 0.0
                blk[:, :R] = x[i].t()
            out = torch.full((groups * out_batch,), 9.0, device=dev)
            ops.transpose_batched(xb.to(dev), groups, R, C, ldi=ldi, out=out, ldo=ldo, in_batch=in_batch, out_batch=out_batch)
            assert torch.equal(out.cpu(), ref), (R, C, ldo)
    x = torch.randn(2, R, 1024, generator=g)  # the wrapper's defaults: dense blocks, its own output
    got = ops.transpose_batched(x.to(dev), 2, R, 1024, ldo=(R + 7) // 8 * 8)
    assert torch.equal(got[:, :, :R].cpu(), x.transpose(1, 2)) and (got[:, :, R:] == 0).all()


@pytest.mark.parametrize("group,n_blocks", [(1, 1), (1, 4), (3, 3), (3, 5), (3, 7)])  # 5, 7: the last group is not full
def test_mul_and_repeat_rows_grouped_bits(dev, group, n_blocks):
    """class sweep (dana.SupportCache.sweep): problem p = image p // group. y rows p * rows + i *= x rows (p // group) *
    rows + i; dst rows p * rows + i = src rows (p // group) * rows + i. One multiply / one copy per element"""
    ops = _ops()
    g = _gen(1300 + 10 * group + n_blocks)
    n_img = (n_blocks + group - 1) // group
    img = torch.arange(n_blocks) // group
    for rows, c in [(1, 4), (5, 36), (49, 68), (257, 64), (400, 1024)]:
        ldy, ldx = c + 4, c + 8
        y, x = torch.randn(n_blocks * rows, c, generator=g), torch.randn(n_img, rows, c, generator=g)
        rep = x[img].reshape(n_blocks * rows, c)  # the replicated statement
        yb, xb = _wide(y, ldy, 9.0).to(dev), _wide(x.view(-1, c), ldx, 1e3).to(dev)
        ops.mul_rows_grouped_(yb, xb, rows, c, group, n_blocks, ld_y=ldy, ld_x=ldx)
        assert torch.equal(yb.cpu(), _wide(y * rep, ldy, 9.0)), (rows, c)
        assert torch.equal(xb.cpu(), _wide(x.view(-1, c), ldx, 1e3))
        for cols in (c, c - 1):  # (the copy has one lane per float: any column count)
            out = torch.full((n_blocks * rows + 1, cols + 3), 9.0, device=dev)
            ops.repeat_rows_grouped(xb, rows, cols, group, n_blocks, ld_src=ldx, out=out, ld_out=cols + 3)
            ref = torch.full((n_blocks * rows + 1, cols + 3), 9.0)
            ref[:-1, :cols] = rep[:, :cols]
            assert torch.equal(out.cpu(), ref), (rows, cols)
        got = ops.repeat_rows_grouped(x.view(-1, c).contiguous().to(dev), rows, c, group, n_blocks)  # dense defaults
        assert torch.equal(got.cpu(), rep)


def test_bn_fold_vs_fp64(dev):
    """frozen BatchNorm2d folded to scale / shift (dana.py:362-385): scale = gamma / sqrt(var + eps), shift = beta - mean *
    scale. mag: |scale|; |beta| + |mean scale|"""
    ops = _ops()
    g = _gen(1400)
    eps = 1e-5
    for n in (1, 3, 64, 255, 257, 2048):
        gam, bet = torch.randn(n, generator=g), torch.randn(n, generator=g)
        mu, var = torch.randn(n, generator=g) * 3, torch.rand(n, generator=g) * 2 + 1e-3
        sc, sh = ops.bn_fold(gam.to(dev), bet.to(dev), mu.to(dev), var.to(dev), eps)
        sc_ref = gam.double() / torch.sqrt(var.double() + _f32(eps))
        _check(sc, sc_ref, sc_ref.abs(), "bn_fold scale")
        _check(sh, bet.double() - mu.double() * sc_ref, bet.double().abs() + (mu.double() * sc_ref).abs(), "bn_fold shift")


# ---------------------------------------------------------------------------------------------------------------------
# RPN decode and the fused proposal layer
# ---------------------------------------------------------------------------------------------------------------------
def _anchors(A):
    from dana_amd import targets as T
    a = T.generate_anchors(scales=np.array({9: [8, 16, 32], 12: [4, 8, 16, 32]}[A]), ratios=np.array([0.5, 1, 2]))
    assert a.shape == (A, 4) and np.array_equal(a, np.round(a))  # integer corners: exact in float32
    return a


def _rpn_layout(layout, bg, fg, deltas):
    """bg, fg [B][K][A], deltas [B][K][A][4] -> (cls buffer, cls strides, bbox buffer or None, bbox strides, bbox offset)
    in the two layouts the model passes: 'rows' = the head GEMM's [B*K][2A | 4A] rows (dana.py:982), 'nchw' = the
    reference's [B][2A][H][W] / [B][4A][H][W] maps (stride of a channel K, of a cell 1)"""
    B, K, A = bg.shape
    if layout == "rows":
        heads = torch.cat([bg, fg, deltas.reshape(B, K, 4 * A)], 2).contiguous()
        return heads, (K * 6 * A, 1, 6 * A), None, (K * 6 * A, 1, 6 * A), 2 * A
    cls = torch.cat([bg, fg], 2).permute(0, 2, 1).contiguous()
    bbox = deltas.reshape(B, K, 4 * A).permute(0, 2, 1).contiguous()
    return cls, (2 * A * K, K, 1), bbox, (4 * A * K, K, 1), 0


def _decode_ref(anchors, deltas, im_info, H, W, feat_stride):
    """bbox_transform_inv + clip_boxes (bbox_transform.py:77-103, 125-133) in float64 -> (boxes [B][K*A][4] clipped, the
    same before clipping, mag = the sum of the absolute values of each coordinate's terms)"""
    B, K, A, _ = deltas.shape
    d = deltas.double()
    a = torch.from_numpy(anchors).double().view(1, 1, A, 4)
    k = torch.arange(K)
    shift = torch.stack([k % W, k // W, k % W, k // W], 1).double().view(1, K, 1, 4) * feat_stride
    a = a + shift
    wh = a[..., 2:] - a[..., :2] + 1.0
    ctr = a[..., :2] + 0.5 * wh
    pc = d[..., :2] * wh + ctr
    half = 0.5 * torch.exp(d[..., 2:]) * wh
    raw = torch.cat([pc - half, pc + half], 3)
    mag = ((d[..., :2] * wh).abs() + ctr.abs() + half).repeat(1, 1, 1, 2)
    hi = torch.stack([im_info[:, 1], im_info[:, 0], im_info[:, 1], im_info[:, 0]], 1).double().view(B, 1, 1, 4) - 1.0
    boxes = torch.minimum(raw.clamp_min(0.0), hi.expand_as(raw))
    return boxes.view(B, K * A, 4), raw.view(B, K * A, 4), mag.view(B, K * A, 4), hi.expand_as(raw).reshape(B, K * A, 4)


def _rpn_inputs(g, B, A, H, W, logit_step=0.0, delta_scale=(0.5, 3.0), size_bias=0.0):
    K = H * W
    bg, fg = torch.randn(B, K, A, generator=g) * 2, torch.randn(B, K, A, generator=g) * 2
    if logit_step:  # logits on a grid: many equal scores
        bg, fg = torch.round(bg / logit_step) * logit_step, torch.round(fg / logit_step) * logit_step
    deltas = torch.randn(B, K, A, 4, generator=g)
    deltas[..., :2] *= delta_scale[0]
    deltas[..., 2:] = (torch.rand(B, K, A, 2, generator=g) * 2 - 1) * delta_scale[1] + size_bias
    return bg, fg, deltas


@pytest.mark.parametrize("cls_is_prob", [0, 1])
@pytest.mark.parametrize("layout", ["rows", "nchw"])
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (19, 20)])  # n = H W A below, across and well above one 256-lane block
@pytest.mark.parametrize("A", [9, 12])
def test_rpn_decode_vs_fp64(dev, A, H, W, layout, cls_is_prob):
    """anchor grid + bbox_transform_inv + clip_boxes + the fg probability (proposal_layer.py:67-130, rpn.py:67-69), three
    images of different sizes, size deltas over the whole of +-3. The first anchors of every image are pushed wholly
    past the left / the right / the bottom border: they must come back as the border, exactly.
    Coordinates: mag = |dx w| + |ctr| + exp(dw) w / 2 before clipping; scores: the softmax bound, or a copy"""
    ops = _ops()
    g = _gen(1500 + 100 * A + H + 7 * cls_is_prob + (3 if layout == "nchw" else 0))
    B, K, fs = 3, H * W, 16
    anchors = _anchors(A)
    im_info = torch.tensor([[80.0, 100.0, 1.0], [600.0, 1000.0, 1.6], [37.0, 53.0, 0.5]])
    bg, fg, deltas = _rpn_inputs(g, B, A, H, W)
    deltas[:, 0, 0] = torch.tensor([-30.0, 0.0, -2.0, 0.0])  # 30 widths to the left, narrow
    deltas[:, 0, 1] = torch.tensor([40.0, 0.0, -2.0, 0.0])   # ... to the right
    deltas[:, 0, 2] = torch.tensor([0.0, 40.0, 0.0, -2.0])   # ... below
    if cls_is_prob:
        p2 = F.softmax(torch.stack([bg, fg], 3), 3)
        bg, fg = p2[..., 0].contiguous(), p2[..., 1].contiguous()
    cls, cs, bbox, bs, off = _rpn_layout(layout, bg, fg, deltas)
    cls_d = cls.to(dev)
    bbox_d = bbox.to(dev) if bbox is not None else cls_d.view(-1)[off:]
    props, scores = ops.rpn_decode(cls_d, cs, cls_is_prob, bbox_d, bs, im_info.to(dev), torch.from_numpy(anchors).float().to(dev),
                                   B, A, H, W, fs)
    ref, raw, mag, hi = _decode_ref(anchors, deltas, im_info, H, W, fs)
    tag = "%s A %d %dx%d" % (layout, A, H, W)
    _check(props, ref, mag, "rpn_decode boxes " + tag)
    got = props.double().cpu()
    low, high = raw < -1.0, raw > hi + 1.0  # a whole pixel outside: no rounding can bring it back in
    assert (got[low] == 0).all() and (got[high] == hi[high]).all()
    outside = (high[..., 0] & high[..., 2]) | (low[..., 0] & low[..., 2]) | (high[..., 1] & high[..., 3])
    assert outside[:, :3].all(), "the three displaced anchors are not wholly outside"
    assert (got[..., 0] <= got[..., 2]).all() and (got[..., 1] <= got[..., 3]).all()
    if cls_is_prob:
        assert torch.equal(scores.cpu(), fg.reshape(B, K * A))
    else:
        x2 = torch.stack([bg, fg], 3).double()
        p = F.softmax(x2, 3)
        _check(scores, p[..., 1].reshape(B, K * A), _softmax_mag(x2, p, 3)[..., 1].reshape(B, K * A), "rpn_decode scores " + tag, TINY)


def _proposal_ref(props, scores, pre, post, thr, inclusive):
    """_ProposalLayer.forward after the decode (proposal_layer.py:135-188) on float32 boxes / scores [B][n]: numpy's stable
    descending sort, cut by the reference's rule -- `pre < scores_keep.numel()` looks at the WHOLE batch's count, and the
    slice [:pre] of an image's n entries stops at n --, a greedy NMS with the legacy +1 widths in float64, the first
    `post` kept boxes behind the image index, zero rows after them.
    -> (rois [B][post][5] float32, the smallest |IoU - thr| over the pairs the greedy pass compared, kept per image,
    suppressed boxes the pass stepped over per image)"""
    B, n = scores.shape
    rois = np.zeros((B, post, 5), np.float32)
    margin, kept, skipped = math.inf, [], []
    for b in range(B):
        order = np.argsort(-scores[b], kind="stable")
        if 0 < pre < B * n:
            order = order[:pre]
        bx = props[b][order].astype(np.float64)
        area = (bx[:, 2] - bx[:, 0] + 1) * (bx[:, 3] - bx[:, 1] + 1)
        alive = np.ones(len(order), bool)
        keep, skip = [], 0
        for i in range(len(order)):
            if not alive[i]:
                skip += 1
                continue
            keep.append(i)
            if len(keep) == post:
                break
            j = np.nonzero(alive[i + 1:])[0] + i + 1
            if j.size == 0:
                continue
            iw = np.maximum(0.0, np.minimum(bx[i, 2], bx[j, 2]) - np.maximum(bx[i, 0], bx[j, 0]) + 1)
            ih = np.maximum(0.0, np.minimum(bx[i, 3], bx[j, 3]) - np.maximum(bx[i, 1], bx[j, 1]) + 1)
            iou = iw * ih / (area[i] + area[j] - iw * ih)
            margin = min(margin, float(np.abs(iou - thr).min()))
            alive[j[(iou >= thr) if inclusive else (iou > thr)]] = False
        rois[b, :, 0] = b
        rois[b, :len(keep), 1:] = props[b][order][keep]
        kept.append(len(keep))
        skipped.append(skip)
    return rois, margin, kept, skipped


# (H, W, pre, post, what the case reaches, zero rows expected, seed, size bias): B = 2, A = 12, n = 12 H W. The seeds are those for which a
# float32 restatement of the decode on the CPU (the float64 reference above, rounded; numpy's float32 softmax) leaves every
# compared pair >= 1e-3 from the threshold with both comparisons. 300 kept boxes of 2000 compare ~10^5 pairs: with boxes of
# the anchors' size none of 400 seeds keeps them all 1e-3 away, so that case shrinks its boxes (dw, dh around -2)
PROPOSAL_CASES = [
    (5, 7, 6000, 300, "pre > B n: top-N = n, fewer than post kept", True, 22, 0.0),
    (5, 7, 500, 300, "n < pre < B n: the whole-batch rule still cuts at n", True, 40, 0.0),
    (5, 7, 100, 20, "top-N = pre, truncated at post", False, 1, 0.0),
    # (with post = 20 the kept boxes all come from the first 42 of the order: only this case depends on WHERE the cut is)
    (5, 7, 100, 300, "top-N = pre: the cut decides what is kept, fewer than post", True, 10, 0.0),
    (19, 20, 2000, 300, "n = 4560: the long-row sort", False, 12, -2.0),
]


def _proposal_inputs(seed, H, W, size_bias=0.0):
    g = _gen(seed)
    B, A = 2, 12
    bg, fg, deltas = _rpn_inputs(g, B, A, H, W, logit_step=0.125, delta_scale=(0.3, 0.6), size_bias=size_bias)
    im_info = torch.tensor([[16.0 * H - 4, 16.0 * W + 10, 1.0], [16.0 * H - 24, 16.0 * W - 10, 1.0]])
    return B, A, bg, fg, deltas, im_info


@pytest.mark.parametrize("inclusive", [False, True])
@pytest.mark.parametrize("H,W,pre,post,what,padded,seed,size_bias", PROPOSAL_CASES,
                         ids=["%dx%d-pre%d-post%d" % c[:4] for c in PROPOSAL_CASES])
def test_proposal_layer_exact(dev, H, W, pre, post, what, padded, seed, size_bias, inclusive):
    """ops.proposal_layer (the fused _ProposalLayer.forward) == decode, numpy's stable sort cut at the reference's top-N,
    float64 greedy NMS, zero-padded assembly -- bit for bit. The logits are multiples of 1/8, so the cut and the NMS
    order run through runs of equal scores. The comparison is only meaningful where no NMS decision is a near tie:
    the inputs must leave every compared pair's IoU at least 1e-4 from the threshold (asserted, not skipped)"""
    ops = _ops()
    thr = 0.7
    B, A, bg, fg, deltas, im_info = _proposal_inputs(seed, H, W, size_bias)
    n = H * W * A
    cls, cs, _, bs, off = _rpn_layout("rows", bg, fg, deltas)
    cls_d = cls.to(dev)
    anchors = torch.from_numpy(_anchors(A)).float().to(dev)
    args = (cls_d, cs, False, cls_d.view(-1)[off:], bs, im_info.to(dev), anchors, B, A, H, W, 16)
    props, scores = ops.rpn_decode(*args)
    sc = scores.cpu().numpy()
    assert max(np.unique(s, return_counts=True)[1].max() for s in sc) > 1, "no equal scores"
    ref, margin, kept, skipped = _proposal_ref(props.cpu().numpy(), sc, pre, post, _f32(thr), inclusive)
    print("PROPOSAL %dx%d pre %d post %d inclusive %d: kept %s, stepped over %s, min |IoU - thr| %.3e" % (
        H, W, pre, post, inclusive, kept, skipped, margin))
    assert margin >= 1e-4, "an NMS decision of this input is a near tie (%.3e): choose another seed" % margin
    assert min(skipped) > 0, "the NMS suppressed nothing in front of the last kept box"
    if pre < n:  # the cut takes effect, and in some image it falls inside a run of equal scores
        srt = -np.sort(-sc, axis=1)
        assert (srt[:, pre - 1] == srt[:, pre]).any(), what
    assert (max(kept) < post) if padded else (min(kept) == post), what  # zero rows reached / the output cut at post
    rois = ops.proposal_layer(*args, pre, post, thr, nms_inclusive=inclusive)
    assert rois.shape == (B, post, 5)
    assert torch.equal(rois.cpu(), torch.from_numpy(ref)), what


def test_proposal_layer_arguments(dev):
    """a workspace one byte short is refused with the workspace error before any launch; B = 0 is OK without buffers"""
    ops = _ops()
    L = ops.lib()
    B, A, H, W, pre, post = 2, 12, 5, 7, 500, 300
    _, _, bg, fg, deltas, im_info = _proposal_inputs(1, H, W)
    cls, cs, _, bs, off = _rpn_layout("rows", bg, fg, deltas)
    cls_d, im_d = cls.to(dev), im_info.to(dev)
    anchors = torch.from_numpy(_anchors(A)).float().to(dev)
    need = L.query("dana_proposal_layer_workspace_bytes", B, A, H, W, pre, post)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rois = torch.full((B, post, 5), 9.0, device=dev)

    def call(batch, nbytes):
        return L.fn["dana_proposal_layer"](cls_d.data_ptr(), cs[0], cs[1], cs[2], 0, cls_d.view(-1)[off:].data_ptr(), bs[0], bs[1], bs[2],
                                           im_d.data_ptr(), anchors.data_ptr(), batch, A, H, W, 16, pre, post, 0.7, 0, rois.data_ptr(),
                                           ws.data_ptr(), nbytes, ops._stream())

    assert call(B, need - 1) == -3  # DANA_ERR_WORKSPACE
    assert b"workspace" in L.cdll.dana_last_error()
    torch.cuda.synchronize()
    assert (rois == 9.0).all()
    assert call(B, need) == 0
    torch.cuda.synchronize()
    assert (rois[:, :, 0] == torch.arange(B, device=dev).view(B, 1)).all()
    assert L.fn["dana_proposal_layer"](None, 0, 0, 0, 0, None, 0, 0, 0, None, None, 0, A, H, W, 16, pre, post, 0.7, 0, None, None, 0,
                                       ops._stream()) == 0
    assert L.query("dana_proposal_layer_workspace_bytes", 0, A, H, W, pre, post) == 0
