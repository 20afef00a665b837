"""Trimmed stage seams: a stage's last Bottleneck computes only the pixels that the next stage's stride-2 1x1 convs read
(resnet.py:71,136). Every check here is BIT equality (torch.equal) against the untrimmed form of the same kernels taken at
the even pixels: the strided fused tail, the 1x1 conv with a sampled residual, the sub-sampled F(4x4,3x3) output
transform, and the model with `trim_strided_seams` on and off.
The kernels run in both MFMA modes where they exist: the fused tail and the sampled residual are forms of the split
kernel (bf16x6) only and must REFUSE the f32-MFMA mode; the Winograd output transform is the same kernel in both."""
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _ops():
    import dana_amd
    return dana_amd.ops


@pytest.fixture(params=[1, 0], ids=["bf16x6", "f32mfma"])
def mfma_mode(request):
    ops = _ops()
    prev = ops.set_mfma_mode(request.param)
    yield request.param
    ops.set_mfma_mode(prev)


def _even(t, n, h, w, ld):
    """rows of the even pixels of a flat [n*h*w][ld] map, dense"""
    return t.view(n, h, w, ld)[:, ::2, ::2].reshape(-1, ld).contiguous()


# (n, h, w, in_stride, out_stride, res_stride, residual): odd sizes with ONE partial tile of 70 rows; 420 rows = tiles that
# straddle image rows and images + a partial last tile; even sizes; row strides larger than the channel counts; no residual
TAIL_CASES = [(2, 9, 13, 64, 256, 256, True), (3, 19, 27, 64, 256, 256, True), (1, 8, 12, 64, 256, 256, True),
              (2, 9, 13, 96, 320, 384, True), (3, 19, 27, 64, 256, 256, False)]


@pytest.mark.parametrize("case", TAIL_CASES, ids=lambda c: "n%d_%dx%d_ld%d_%d_%d_res%d" % c)
def test_strided_tail_equals_the_full_tail_at_even_pixels(dev, mfma_mode, case):
    ops = _ops()
    n, h, w, ldx, ldo, ldr, res = case
    ci, co = 64, 256
    g = torch.Generator().manual_seed(7)
    m = n * h * w
    x = torch.randn(m, ldx, generator=g).to(dev)
    w2 = (torch.randn(64, 9 * ci, generator=g) / np.sqrt(9 * ci)).to(dev)
    w3 = (torch.randn(co, 64, generator=g) / 8).to(dev)
    s2, b2 = (torch.rand(64, generator=g) + 0.5).to(dev), torch.randn(64, generator=g).to(dev)
    s3, b3 = (torch.rand(co, generator=g) + 0.5).to(dev), torch.randn(co, generator=g).to(dev)
    r = torch.randn(m, ldr, generator=g).to(dev) if res else None
    if mfma_mode == 0:
        assert ops.split_weight(w2, 64, 9 * ci) is None  # (split kernel only: there are no planes to hand it)
        return
    w2s, w3s = ops.split_weight(w2, 64, 9 * ci), ops.split_weight(w3, co, 64)
    full = torch.zeros(m, ldo, device=dev)
    ops.bottleneck_tail(x, n, h, w, ci, w2s, s2, b2, w3s, s3, b3, co, residual=r, in_stride=ldx, out=full, out_stride=ldo,
                        res_stride=ldr if res else 0)
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    mo = n * oh * ow
    got = torch.full((mo + 136, ldo), -7.0, device=dev)  # guard rows behind the last (partial) row tile
    got[:mo].zero_()
    _, gh, gw = ops.bottleneck_tail(x, n, h, w, ci, w2s, s2, b2, w3s, s3, b3, co, residual=r, in_stride=ldx, out=got,
                                    out_stride=ldo, res_stride=ldr if res else 0, stride=2)
    assert (gh, gw) == (oh, ow)
    ref = _even(full, n, h, w, ldo)
    assert torch.equal(ref, got[:mo]), float((ref - got[:mo]).abs().max())
    assert bool((got[mo:] == -7.0).all()), "rows past M were written"
    # stride 1 through the new entry is the old entry
    one = torch.zeros(m, ldo, device=dev)
    ops.lib().call("dana_bottleneck_tail_strided_nhwc", ops._p(x), ops._p(w2s.t), ops._p(s2), ops._p(b2), ops._p(w3s.t),
                   ops._p(s3), ops._p(b3), ops._p(r), ops._p(one), n, h, w, ci, 64, co, ldx, ldo, ldr if res else 0, 1,
                   ops.EPI_RELU, ops._stream())
    assert torch.equal(one, full)


def _expand_operands(dev, n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    K, N = 128, 512
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    o2 = torch.randn(n * h * w, K, generator=g).to(dev)                 # conv2's full output
    wt = (torch.randn(N, K, generator=g) / np.sqrt(K)).to(dev)
    sc, sh = (torch.rand(N, generator=g) + 0.5).to(dev), torch.randn(N, generator=g).to(dev)
    x = torch.randn(n * h * w, N, generator=g).to(dev)                  # the block's input: the residual map
    return K, N, oh, ow, o2, wt, sc, sh, x


@pytest.mark.parametrize("shape", [(2, 9, 13), (3, 19, 27)], ids=lambda s: "n%d_%dx%d" % s)
@pytest.mark.parametrize("tile", [0, 4], ids=["dispatch", "tile128x128"])
@pytest.mark.parametrize("presplit", [False, True], ids=["fp32w", "w3"])
def test_expand_with_sampled_residual(dev, mfma_mode, shape, tile, presplit):
    """K = 128 -> N = 512 over the even pixels' rows, residual = x at the even pixels: against the existing entry over a
    residual gathered by torch indexing (same M, same dispatch) and against the full-size launch taken at the even
    pixels -- both torch.equal (the row's K walk does not depend on the tile shape). The dispatcher's own choice at these
    sizes is the 64 x 64 tile; the forced 128 x 128 tile is the form the trunk's launch takes."""
    ops = _ops()
    n, h, w = shape
    K, N, oh, ow, o2, wt, sc, sh, x = _expand_operands(dev, n, h, w, 11 + n)
    rows = _even(o2, n, h, w, K)
    if mfma_mode == 0:
        if tile or presplit:
            return
        # the f32-MFMA kernel has no sampled form: the launch is refused, nothing is written
        out = torch.full((n * oh * ow, N), -3.0, device=dev)
        with pytest.raises(Exception, match="sampled residual"):
            ops.conv2d_nhwc(rows, n, oh, ow, K, wt, N, 1, 1, 1, 0, scale=sc, shift=sh, residual=x, relu=True, out=out,
                            out_stride=N, res_stride=N, res_hw=(h, w), res_sample=2)
        assert bool((out == -3.0).all())
        return
    wb = ops.split_weight(wt, N, K) if presplit else wt
    if tile:
        ops.force_tile(tile)
    try:
        gathered, _, _ = ops.conv2d_nhwc(rows, n, oh, ow, K, wb, N, 1, 1, 1, 0, scale=sc, shift=sh,
                                         residual=_even(x, n, h, w, N), relu=True)
        full, _, _ = ops.conv2d_nhwc(o2, n, h, w, K, wb, N, 1, 1, 1, 0, scale=sc, shift=sh, residual=x, relu=True)
        mo = n * oh * ow
        got = torch.full((mo + 136, N), -7.0, device=dev)
        got[:mo].zero_()
        ops.conv2d_nhwc(rows, n, oh, ow, K, wb, N, 1, 1, 1, 0, scale=sc, shift=sh, residual=x, relu=True, out=got,
                        out_stride=N, res_stride=N, res_hw=(h, w), res_sample=2)
    finally:
        if tile:
            ops.force_tile(0)
    assert torch.equal(gathered, got[:mo]), float((gathered - got[:mo]).abs().max())
    assert torch.equal(_even(full, n, h, w, N), got[:mo])
    assert bool((got[mo:] == -7.0).all()), "rows past M were written"


def test_sampled_residual_is_refused_where_no_kernel_implements_it(dev):
    """the LDS-epilogue mode, N <= 64 (128 x 64 tiles), a map that is not the output's: an error, never a wrong answer"""
    ops = _ops()
    n, h, w = 2, 9, 13
    K, N, oh, ow, o2, wt, sc, sh, x = _expand_operands(dev, n, h, w, 5)
    rows = _even(o2, n, h, w, K)

    def run(cout=N, res_hw=(h, w), **kw):
        out = torch.full((n * oh * ow, cout), -3.0, device=dev)
        with pytest.raises(Exception, match="sampled residual"):
            ops.conv2d_nhwc(rows, n, oh, ow, K, wt[:cout].contiguous(), cout, 1, 1, 1, 0, scale=sc, shift=sh, residual=x,
                            relu=True, out=out, out_stride=cout, res_stride=N, res_hw=res_hw, res_sample=2)
        assert bool((out == -3.0).all())

    prev = ops.set_epilogue_mode(1)
    try:
        run()
    finally:
        ops.set_epilogue_mode(prev)
    run(cout=64)
    run(res_hw=(h + 2, w))


# (n, h, w): odd sizes; even sizes; a single partial tile row and column
@pytest.mark.parametrize("shape", [(2, 9, 13), (1, 8, 12), (1, 5, 7)], ids=lambda s: "n%d_%dx%d" % s)
@pytest.mark.parametrize("epi", [False, True], ids=["plain", "scale_shift_relu"])
def test_winograd_sub2_equals_the_full_output_at_even_pixels(dev, mfma_mode, shape, epi):
    ops = _ops()
    n, h, w = shape
    C = 128
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n * h * w, C, generator=g).to(dev)
    wt = (torch.randn(C, 9 * C, generator=g) / np.sqrt(9 * C)).to(dev)
    sc = (torch.rand(C, generator=g) + 0.5).to(dev) if epi else None
    sh = torch.randn(C, generator=g).to(dev) if epi else None
    u = ops.winograd_filter_transform(wt, C, C, tile=4)
    for ub in ([u, ops.split_weight(u, C, C, batch=36)] if mfma_mode else [u]):
        full, _, _ = ops.conv3x3_winograd(x, n, h, w, C, ub, C, scale=sc, shift=sh, relu=epi)
        oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        mo = n * oh * ow
        got = torch.full((mo + 8, C), -7.0, device=dev)
        _, gh, gw = ops.conv3x3_winograd(x, n, h, w, C, ub, C, scale=sc, shift=sh, relu=epi, out=got, out_stride=C, sub=2)
        assert (gh, gw) == (oh, ow)
        assert torch.equal(_even(full, n, h, w, C), got[:mo])
        assert bool((got[mo:] == -7.0).all()), "rows past the sampled map were written"
    with pytest.raises(ValueError):
        ops.conv3x3_winograd(x, n, h, w, C, ops.winograd_filter_transform(wt, C, C, tile=2), C, sub=2)


# ---- the model ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dana_model(dev):
    import dana_amd
    from dana_amd import synthetic as S
    m = dana_amd.get_model("DAnA", pretrained=False, use_BA_block=True, way=2, shot=2, classes=["fg", "bg"])
    m.load_state_dict(S.fill_state_dict(m.state_dict(), seed=5, profile="test"))
    return m.to(dev)


def _both_walks(m, run):
    """-> outputs of the full-size walk and of the model as it comes (the trim is the default)"""
    assert m.trim_strided_seams is True
    on = [o.detach().clone() if torch.is_tensor(o) else o for o in run()]
    m.trim_strided_seams = False
    try:
        off = [o.detach().clone() if torch.is_tensor(o) else o for o in run()]
    finally:
        del m.trim_strided_seams  # (back to the class default)
    assert m.trim_strided_seams is True
    torch.cuda.synchronize()
    return off, on


def _same(a, b):
    assert len(a) == len(b)
    for i, (p, q) in enumerate(zip(a, b)):
        if torch.is_tensor(p):
            assert torch.equal(p, q), "output %d differs by %g" % (i, float((p.float() - q.float()).abs().max()))
        else:
            assert p == q, i


# the default query size, and one whose layer-1 grid is odd both ways (172 x 236 -> 43 x 59)
@pytest.mark.parametrize("size", [(160, 224), (172, 236)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("training", [False, True], ids=["eval", "train_no_grad"])
def test_model_outputs_are_bit_identical_with_and_without_the_trim(dev, dana_model, size, training):
    from dana_amd import synthetic as S
    ops = _ops()
    H, W = size
    if size == (172, 236):
        assert ops.maxpool_out_size((H - 1) // 2 + 1, (W - 1) // 2 + 1) == (43, 59)
    m = dana_model
    m.train() if training else m.eval()
    inputs = [t.to(dev) for t in S.episode_inputs(2, 2 if training else 1, 2, H, W, seed=9)]

    def run():
        np.random.seed(3)
        with torch.no_grad():
            return m(*inputs)

    off, on = _both_walks(m, run)
    _same(off, on)


def test_frcnn_sibling_is_bit_identical_with_and_without_the_trim(dev):
    import dana_amd
    from dana_amd import synthetic as S
    m = dana_amd.get_model("frcnn", pretrained=False, classes=["fg", "bg"])
    m.load_state_dict(S.fill_state_dict(m.state_dict(), seed=5, profile="test"))
    m.to(dev).eval()
    im_data, im_info, gt, nb, _ = S.episode_inputs(2, 1, 1, 172, 236, seed=4)
    args = [t.to(dev) for t in (im_data, im_info, gt, nb)]

    def run():
        with torch.no_grad():
            return m(*args)

    off, on = _both_walks(m, run)
    _same(off, on)


def test_trim_keeps_the_launch_count_and_quarters_the_trimmed_rows(dev, dana_model):
    """ops.PROFILE on one stream: the same number of contraction launches; layer1's fused tail and layer2's last expand
    conv run over (about) a quarter of the rows -- exactly the even-pixel count of their grids"""
    from dana_amd import synthetic as S
    ops = _ops()
    m = dana_model
    m.eval()
    H, W = 160, 224
    inputs = [t.to(dev) for t in S.episode_inputs(2, 1, 2, H, W, seed=9)]
    names = []
    m._single_stream = True
    try:
        for trim in (False, True):
            m.trim_strided_seams = trim
            ops.PROFILE = []
            try:
                with torch.no_grad():
                    m(*inputs)
                torch.cuda.synchronize()
                names.append([e[0] for e in ops.PROFILE])
            finally:
                ops.PROFILE = None
    finally:
        del m.trim_strided_seams  # (back to the class default)
        m._single_stream = False
    off, on = names
    assert len(off) == len(on)
    changed = [(a, b) for a, b in zip(off, on) if a != b]
    rows = lambda s: int(re.search(r"M=(\d+)", s).group(1))
    kind = lambda s: s.split(" M=")[0]
    tails = [(a, b) for a, b in changed if kind(a) == "conv3x3+1x1"]
    expands = [(a, b) for a, b in changed if kind(a) == "conv1x1" and " N=512 " in a and " K=128 " in a]
    assert len(tails) == 2 and len(expands) == 2, changed  # (query trunk and support trunk)
    h1, w1 = ops.maxpool_out_size((H - 1) // 2 + 1, (W - 1) // 2 + 1)  # layer1's grid of the query images
    assert any(rows(a) == 2 * h1 * w1 and rows(b) == 2 * ((h1 + 1) // 2) * ((w1 + 1) // 2) and b.endswith("s2") for a, b in tails), tails
    for a, b in tails + expands:
        assert rows(a) / 4.0 <= rows(b) <= rows(a) / 3.0, (a, b)  # a quarter, up to the odd row / column
    # every other changed launch is the next block reading dense rows: same M, stride 1 instead of 2
    for a, b in changed:
        if (a, b) not in tails and (a, b) not in expands:
            assert rows(a) == rows(b) and a.endswith("s2") and b.endswith("s1"), (a, b)
