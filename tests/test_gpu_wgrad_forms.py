"""Every kernel behind csrc/wgrad.hip's cost model, SELECTED in-process (ops.force_wgrad / ops.wgrad_forms), PROVEN through the
recorded launch (ops.last_wgrad_form: kernel, slice count S, planes) and compared with a float64 contraction of the same fp32
operands -- at the smallest shapes at which a tile, a pipeline prologue, the incremental geometry or the reducer can go wrong:
  * wgrad_f32_kernel (tile 64, under either MFMA mode), wgrad_f32_128_kernel (tile 128, set_mfma_mode(0)),
    wgrad_split_128p_kernel (tile 128, mode 1, 1x1 / stride 1 / pad 0) and wgrad_split_128_kernel (tile 128, mode 1, the rest);
  * wgrad_reduce_kernel with S = 1, 2, 5 (S = 5: slice lane 0 sums slices 0 and 4), with and without accumulate + row_scale;
  * dana_gemm_tn_batched (three planes, n_valid < n, strided rows, gaps between the planes' results) and the Winograd-domain
    weight gradient (36 planes; S = 1: the kernel writes dU itself, S = 2: through the reducer).
Bound (tests/test_gpu_contraction_forms.py's rule): with mag = |row_scale| (|gy|^T . |im2col x|) + |init| per element,
max |got - ref| / mag <= 2 e_ref + 2e-7, where e_ref is the same ratio of torch's own fp32 matmul of the unfolded operands on the
device -- never one of the forms. The Winograd path is held to the bar of test_winograd_weight_gradient_vs_direct_and_autograd
(2e-4 of max |ref|): its transforms are not a contraction of the same operands.
Every result lies in a buffer of sentinels: NaN where the launch must write when it does not accumulate, guards in front and
behind, checked bit for bit; the operands' guard columns (in_stride > cin, grad_stride > cout) hold NaN.

Conv geometries (batch, H, W, cin, cout, k, stride, pad), each fresh and with out= accumulate + row_scale (the latter with
in_stride = cin + 16 and grad_stride = cout + 8 whatever the geometry), each under forced S in {1, 2, 5} as far as the clamp
(ceil(M / 32), no empty slice) allows:
  (1,1,1,64,4,1,1,0)      M = 1, N = 4
  (1,h,w,64,132,1,1,0)    M = 15, 16, 17, 31, 33, 35, 47, 49: the pipelined kernel's one- to four-step prologues and its odd
                          all-zero step, the f32 kernels' 32-pixel slab tail; the second 128-row n tile holds four rows, K = 64
                          leaves half of the 128 k-tile dead
  (2,5,3,64,72,3,1,1)     a 128-column tile straddles two taps, OW = 3 < 16 (carries), every pixel touches padding
  (5,2,3,128,64,3,1,1)    OH * OW = 6 < 16: d_img = 2
  (2,9,7,64,68,1,2,0)     strided 1x1 (general X path, plain dY path), in_stride 80, grad_stride 72
  (1,7,9,192,64,3,2,1)    stride 2 with padding, three 64-channel groups per tap
  (1,19,23,64,64,3,1,1)   M = 437: S = 2 -> chunks of 224 (the tail slice shorter), S = 5 -> chunks of 96

Worst max |got - ref| / mag per kernel over every case of this file with the e_ref of that very case, as measured on an MI355X
(`pytest -s` prints the table again at the end of the module):
  f32_64       2.541e-07  (e_ref 2.541e-07)  gemm_tn_batched (49, 132, 129, 192), S = 1, accumulate
  f32_128      2.541e-07  (e_ref 2.541e-07)  gemm_tn_batched (49, 132, 129, 192), S = 1, accumulate
  split_128    3.499e-07  (e_ref 2.447e-07)  conv (5,2,3,128,64,3,1,1), S = 1, fresh
  split_128p   3.886e-07  (e_ref 1.843e-07)  conv (1,1,17,64,132,1,1,0), S = 1, accumulate + row_scale
Every recorded kernel and S was the expected one, the four rows of the unforced dispatcher included (S = 4, 10, 1, 28), and the
Winograd path's worst error was 1.72e-4 / 69.4 = 2.5e-6 of max |ref| (bar 2e-4).

What this file found: with the split kernels' operands cut into bf16 pieces by TRUNCATION (hi = x & 0xffff0000, twice: mid up to
2^-7 |x|, lo up to 2^-14 |x|) the three dropped products mid * lo, lo * mid, lo * lo reach 2^-20 of one product, and
gemm_tn_batched (1, 132, 129, 64 / 192) on wgrad_split_128p_kernel -- M = 1: an output element IS one product, nothing averages,
e_ref is one fp32 rounding -- measured 4.073e-07 (e_ref 5.921e-08) and 4.482e-07 (e_ref 5.931e-08) against bounds of 3.18e-07 /
3.19e-07. Both split kernels now round each level to the nearest bf16 (wsplit_hi in csrc/wgrad.hip): the dropped products stay
at 2^-24, and the two cases, kept as they were, measure 2.608e-07 and 2.422e-07 -- what a CPU restatement of the six products
accumulated in fp32 gives for those operands.
"""
import collections

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SENT = -77.25
NAN = float("nan")
GUARD = 256  # sentinel floats in front of and behind a result

FORMS = [(0, 64), (0, 128), (1, 128), (1, 64)]  # (MFMA mode, forced tile)
SLICES = (1, 2, 5)
ONE_BY_ONE = [(1, 3, 5), (1, 4, 4), (1, 1, 17), (1, 1, 31), (1, 3, 11), (1, 5, 7), (1, 1, 47), (1, 7, 7)]  # M = 15 .. 49
GEOMS = ([(1, 1, 1, 64, 4, 1, 1, 0)] + [(b, h, w, 64, 132, 1, 1, 0) for b, h, w in ONE_BY_ONE] +
         [(2, 5, 3, 64, 72, 3, 1, 1), (5, 2, 3, 128, 64, 3, 1, 1), (2, 9, 7, 64, 68, 1, 2, 0), (1, 7, 9, 192, 64, 3, 2, 1),
          (1, 19, 23, 64, 64, 3, 1, 1)])
STRIDES = {(2, 9, 7, 64, 68, 1, 2, 0): (80, 72)}  # (in_stride, grad_stride) of the fresh launch


def _ops():
    import dana_amd
    return dana_amd.ops


@pytest.fixture(autouse=True)
def _restore_forms():
    """force_wgrad(0, 0) and the previous MFMA mode after every test"""
    ops = _ops()
    prev = ops.get_mfma_mode()
    yield
    ops.force_wgrad(0, 0)
    ops.set_mfma_mode(prev)


_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _WORST:
        print("\nworst max |got - ref| / mag per kernel (its e_ref, the case):")
        for kern in sorted(_WORST):
            print("  %-12s %.3e  (e_ref %.3e)  %s" % ((kern,) + _WORST[kern]))


def _check(got, ref, mag, e_ref, form, what):
    ratio = float(((got.double() - ref).abs() / mag).max())
    print("%s %s: ratio %.3e e_ref %.3e" % (what, tuple(form), ratio, e_ref))
    if ratio > _WORST.get(form.kernel, (-1.0,))[0]:
        _WORST[form.kernel] = (ratio, e_ref, what)
    assert ratio <= 2.0 * e_ref + 2e-7, "%s %s: max |err| / mag %.3e, torch fp32 %.3e" % (what, tuple(form), ratio, e_ref)


def _chunk(m, s):
    return ((m + s - 1) // s + 31) // 32 * 32


def _clamped(s, m, planes=1):
    """the slice count a forced `s` becomes: at most ceil(M / 32), planes * S <= 65535, no empty slice"""
    s = max(1, min(s, (m + 31) // 32, 65535 // planes))
    while s > 1 and (s - 1) * _chunk(m, s) >= m:
        s -= 1
    return s


def _kernel(mode, tile, plain):
    if tile == 64:
        return "f32_64"
    if mode == 0:
        return "f32_128"
    return "split_128p" if plain else "split_128"


def test_the_clamp_of_a_forced_slice_count_by_hand():
    """what the cases below expect of the clamp, spelled out (437 pixels take 2 and 5 slices as they are, 35 and 49 at most two,
    up to 32 one; 300 pixels in 9 slices of 64 would leave four of them empty)"""
    assert [_clamped(s, 437) for s in SLICES] == [1, 2, 5] and (_chunk(437, 2), _chunk(437, 5)) == (224, 96)
    assert [_clamped(5, m) for m in (1, 15, 16, 17, 31, 32, 33, 35, 47, 49, 60, 70)] == [1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 3]
    assert _clamped(9, 300) == 5 and _clamped(64, 300) == 10 and _clamped(5, 437, planes=30000) == 2


class _Out:
    """`planes` results of `count` floats (plane stride `stride` >= count) between GUARD sentinels: NaN (or `init`) where the
    launch writes, SENT everywhere else"""

    def __init__(self, dev, count, planes=1, stride=None, init=None):
        self.stride = stride or count
        self.buf = torch.full((2 * GUARD + planes * self.stride,), SENT, device=dev)
        self.region = torch.as_strided(self.buf, (planes, count), (self.stride, 1), GUARD)
        if init is None:
            self.region.fill_(NAN)
        else:
            self.region.copy_(init.view(planes, count))
        self.pre = self.buf.clone()

    def ptr(self):
        return self.buf.data_ptr() + 4 * GUARD

    def take(self, what):
        got = self.region.clone()
        self.region.copy_(torch.as_strided(self.pre, self.region.shape, self.region.stride(), GUARD))
        assert torch.equal(self.buf.view(torch.int32), self.pre.view(torch.int32)), "%s: a sentinel was overwritten" % (what,)
        assert bool(torch.isfinite(got).all()), "%s: an output element was not written (or is not finite)" % (what,)
        return got


# ---- conv cases: operands, float64 reference, mag and e_ref, computed once per geometry and left unchanged ------------------------
ConvCase = collections.namedtuple("ConvCase", "gy cols x scale init ref mag e_ref ref_acc mag_acc e_ref_acc m")
_CONV = {}


def _im2col(x, k, stride, pad):
    """NCHW -> [batch * OH * OW][k * k * cin], columns in the packed weight's (kh, kw, cin) order"""
    b, cin = x.shape[:2]
    u = F.unfold(x, k, padding=pad, stride=stride)  # [b][cin * k * k][L], rows in (cin, kh, kw) order
    return u.view(b, cin, k * k, -1).permute(0, 3, 2, 1).reshape(-1, k * k * cin).contiguous()


def _conv_case(dev, geom):
    if geom in _CONV:
        return _CONV[geom]
    b, h, w, cin, cout, k, stride, pad = geom
    g = torch.Generator().manual_seed(sum(p * q for p, q in zip(geom, (1, 3, 5, 7, 11, 13, 17, 19))))
    x = torch.randn(b, cin, h, w, generator=g)
    cols = _im2col(x, k, stride, pad)
    m = cols.shape[0]
    gy = torch.randn(m, cout, generator=g)
    scale = (torch.rand(cout, generator=g) + 0.5) * (1 - 2 * (torch.arange(cout) % 2)).float()  # both signs
    init = torch.randn(cout, k * k * cin, generator=g)
    ref = gy.double().t() @ cols.double()
    mag = gy.double().abs().t() @ cols.double().abs()
    ref_acc = scale.double().view(-1, 1) * ref + init.double()
    mag_acc = scale.double().abs().view(-1, 1) * mag + init.double().abs()
    gyd, cd, scd, ind = gy.to(dev), cols.to(dev), scale.to(dev), init.to(dev)
    t32 = gyd.t() @ cd
    t32_acc = t32 * scd.view(-1, 1) + ind
    ref, mag, ref_acc, mag_acc = ref.to(dev), mag.to(dev), ref_acc.to(dev), mag_acc.to(dev)
    e_ref = float(((t32.double() - ref).abs() / mag).max())
    e_ref_acc = float(((t32_acc.double() - ref_acc).abs() / mag_acc).max())
    rows = x.permute(0, 2, 3, 1).reshape(-1, cin).contiguous().to(dev)  # NHWC pixel rows
    _CONV[geom] = ConvCase(gyd, cd, rows, scd, ind, ref, mag, e_ref, ref_acc, mag_acc, e_ref_acc, m)
    return _CONV[geom]


def _strided(rows, ld):
    """the rows inside a [rows + 1][ld] buffer whose other columns hold NaN (what lies around the channels must not be read)"""
    if ld == rows.shape[1]:
        return rows
    buf = torch.full((rows.shape[0] + 1, ld), NAN, device=rows.device)
    buf[:rows.shape[0], :rows.shape[1]] = rows
    return buf


def _conv_wgrad(ops, dev, geom, c, in_stride, grad_stride, out, row_scale, accumulate):
    b, h, w, cin, cout, k, stride, pad = geom
    x, gy = _strided(c.x, in_stride or cin), _strided(c.gy, grad_stride or cout)
    ws = ops._ws(ops.lib().query("dana_conv2d_wgrad_workspace_bytes", b, h, w, cin, cout, k, k, stride, pad), dev)
    ws.fill_(255)  # (all-ones words are NaN: the partial tiles are written before they are read)
    ops.lib().call("dana_conv2d_wgrad_nhwc", gy.data_ptr(), x.data_ptr(), out.ptr(), b, h, w, cin, cout, k, k, stride, pad,
                   in_stride, grad_stride, None if row_scale is None else row_scale.data_ptr(), int(accumulate), ws.data_ptr(),
                   ws.numel(), ops._stream())
    return ops.last_wgrad_form()


@pytest.mark.parametrize("mode,tile", FORMS, ids=["mode%d-tile%d" % f for f in FORMS])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g_: "b%d-%dx%d-c%d-%d-k%ds%dp%d" % g_)
def test_conv_wgrad_form_vs_fp64(dev, geom, mode, tile):
    """one kernel on one geometry under forced S = 1, 2, 5: fresh into NaN, then accumulated with a row scale from strided
    operands; the recorded kernel and S are the forced ones"""
    ops = _ops()
    ops.set_mfma_mode(mode)
    b, h, w, cin, cout, k, stride, pad = geom
    c = _conv_case(dev, geom)
    kern = _kernel(mode, tile, k == 1 and stride == 1 and pad == 0)
    in_stride, grad_stride = STRIDES.get(geom, (0, 0))
    done = set()
    for s in SLICES:
        expect = ops.WgradForm(kern, _clamped(s, c.m), 1)
        if expect.slices in done:  # (the clamp made it a launch this test has run already)
            continue
        done.add(expect.slices)
        what = "wgrad %s S=%d" % (geom, expect.slices)
        with ops.wgrad_forms(tile=tile, slices=s):
            out = _Out(dev, cout * k * k * cin)
            f = _conv_wgrad(ops, dev, geom, c, in_stride, grad_stride, out, None, False)
            assert f == expect, (f, expect)
            _check(out.take(what).view_as(c.ref), c.ref, c.mag, c.e_ref, f, what)
            out = _Out(dev, cout * k * k * cin, init=c.init)
            f = _conv_wgrad(ops, dev, geom, c, cin + 16, cout + 8, out, c.scale, True)
            assert f == expect, (f, expect)
            _check(out.take(what).view_as(c.ref), c.ref_acc, c.mag_acc, c.e_ref_acc, f, what + " accumulate + row_scale")
    assert 1 in done and (c.m <= 32 or 2 in done) and (c.m < 437 or 5 in done)


# ---- dana_gemm_tn_batched ----------------------------------------------------------------------------------------------------
TN_PLANES = 3
TN_SHAPES = [(m, n, nv, k) for m in (1, 17, 49) for n, nv in ((8, 5), (132, 129)) for k in (64, 192)]
TnCase = collections.namedtuple("TnCase", "y x init ldy ldx bo ref mag e_ref ref_acc mag_acc e_ref_acc")
_TN = {}


def _tn_case(dev, shape):
    if shape in _TN:
        return _TN[shape]
    m, n, nv, k = shape
    g = torch.Generator().manual_seed(1000 * m + 10 * n + k)
    ldy, ldx, bo = n + 8, k + 12, nv * k + 20
    y = torch.randn(TN_PLANES, m, n, generator=g)
    y[:, :, nv:] = 0  # (zero-padded columns behind n_valid: computed, never stored)
    x = torch.randn(TN_PLANES, m, k, generator=g)
    init = torch.randn(TN_PLANES, nv * k, generator=g)
    ref = (y[:, :, :nv].double().transpose(1, 2) @ x.double()).reshape(TN_PLANES, -1)
    mag = (y[:, :, :nv].double().abs().transpose(1, 2) @ x.double().abs()).reshape(TN_PLANES, -1)
    ref_acc, mag_acc = ref + init.double(), mag + init.double().abs()
    yd, xd, ind = y.to(dev), x.to(dev), init.to(dev)
    t32 = (yd[:, :, :nv].transpose(1, 2) @ xd).reshape(TN_PLANES, -1)
    t32_acc = t32 + ind
    ref, mag, ref_acc, mag_acc = ref.to(dev), mag.to(dev), ref_acc.to(dev), mag_acc.to(dev)
    e_ref = float(((t32.double() - ref).abs() / mag).max())
    e_ref_acc = float(((t32_acc.double() - ref_acc).abs() / mag_acc).max())
    yb = torch.full((TN_PLANES, m, ldy), NAN, device=dev)
    yb[:, :, :n] = yd
    xb = torch.full((TN_PLANES, m, ldx), NAN, device=dev)
    xb[:, :, :k] = xd
    _TN[shape] = TnCase(yb, xb, ind, ldy, ldx, bo, ref, mag, e_ref, ref_acc, mag_acc, e_ref_acc)
    return _TN[shape]


TN_FORMS = [(1, 64), (1, 128), (0, 128)]


@pytest.mark.parametrize("mode,tile", TN_FORMS, ids=["mode%d-tile%d" % f for f in TN_FORMS])
@pytest.mark.parametrize("shape", TN_SHAPES, ids=lambda s_: "m%d-n%d-nv%d-k%d" % s_)
def test_gemm_tn_batched_form_vs_fp64(dev, shape, mode, tile):
    """three planes, ldy > n, ldx > k (NaN behind the columns), results batch_out apart with a gap, n_valid < n, accumulate on
    and off, under tile 64 / 128 and S = 1 / 2: the gaps and the tail keep their bits"""
    ops = _ops()
    ops.set_mfma_mode(mode)
    m, n, nv, k = shape
    c = _tn_case(dev, shape)
    kern = _kernel(mode, tile, True)
    for s in (1, 2):
        expect = ops.WgradForm(kern, _clamped(s, m, TN_PLANES), TN_PLANES)
        if s == 2 and expect.slices == 1:
            continue
        for accumulate in (False, True):
            what = "gemm_tn_batched %s S=%d acc=%d" % (shape, expect.slices, accumulate)
            out = _Out(dev, nv * k, TN_PLANES, c.bo, init=c.init if accumulate else None)
            with ops.wgrad_forms(tile=tile, slices=s):
                ws = ops._ws(ops.lib().query("dana_gemm_tn_batched_workspace_bytes", TN_PLANES, m, n, k), dev)
                ws.fill_(255)
                ops.lib().call("dana_gemm_tn_batched", c.y.data_ptr(), c.x.data_ptr(), out.ptr(), TN_PLANES, m, n, k, c.ldy, c.ldx,
                               m * c.ldy, m * c.ldx, c.bo, nv, int(accumulate), ws.data_ptr(), ws.numel(), ops._stream())
                f = ops.last_wgrad_form()
            assert f == expect, (f, expect)
            got = out.take(what)
            if accumulate:
                _check(got, c.ref_acc, c.mag_acc, c.e_ref_acc, f, what)
            else:
                _check(got, c.ref, c.mag, c.e_ref, f, what)


# ---- the Winograd-domain weight gradient -------------------------------------------------------------------------------------
# (the third geometry has 50 tiles of 4x4 outputs: the first two have 4 and 12, which the clamp to ceil(M / 32) keeps at S = 1)
WINO_GEOMS = [(1, 5, 6, 64, 8), (2, 9, 7, 128, 132), (2, 17, 20, 64, 8)]
_WINO = {}


def _wino_case(dev, geom):
    if geom not in _WINO:
        ops = _ops()
        b, h, w, cin, cout = geom
        g = torch.Generator().manual_seed(sum(geom))
        x = torch.randn(b, cin, h, w, generator=g)
        gy = torch.randn(b, cout, h, w, generator=g)
        scale = torch.rand(cout, generator=g) + 0.5
        init = torch.randn(cout, 9 * cin, generator=g)
        wd = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
        F.conv2d(x.double(), wd, padding=1).backward(gy.double())
        ref = wd.grad.permute(0, 2, 3, 1).reshape(cout, 9 * cin)
        ref_acc = ref * scale.double().view(-1, 1) + init.double()
        _WINO[geom] = (ops.nchw_to_nhwc(x.to(dev)), ops.nchw_to_nhwc(gy.to(dev)), scale.to(dev), init.to(dev), ref.to(dev),
                       ref_acc.to(dev))
    return _WINO[geom]


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("geom", WINO_GEOMS, ids=lambda g_: "b%d-%dx%d-c%d-%d" % g_)
def test_winograd_wgrad_under_each_tile_and_slice_count(dev, geom, tile):
    """conv3x3_wgrad_winograd's 36-plane batched launch under tile 64 / 128 with S = 1 (partial = out: the kernel writes dU
    itself) and S = 2 (through the reducer), fresh and accumulated with a row scale, against float64 autograd"""
    ops = _ops()
    ops.set_mfma_mode(1)
    b, h, w, cin, cout = geom
    xd, gd, scale, init, ref, ref_acc = _wino_case(dev, geom)
    tiles = b * ((h + 3) // 4) * ((w + 3) // 4)
    ran = set()
    for s in (1, 2):
        expect = ops.WgradForm(_kernel(1, tile, True), _clamped(s, tiles, 36), 36)
        ran.add(expect.slices)
        with ops.wgrad_forms(tile=tile, slices=s):
            fresh = ops.conv3x3_wgrad_winograd(gd, xd, b, h, w, cin, cout)
            f = ops.last_wgrad_form()
            out = init.clone()
            ops.conv3x3_wgrad_winograd(gd, xd, b, h, w, cin, cout, out=out, row_scale=scale)
            assert f == expect == ops.last_wgrad_form(), (f, expect)
        for got, want in ((fresh, ref), (out, ref_acc)):
            err, top = float((got.double() - want).abs().max()), float(want.abs().max())
            print("winograd wgrad %s tile %d S=%d: max err %.3e of max |ref| %.3e" % (geom, tile, expect.slices, err, top))
            assert err <= 2e-4 * top, (geom, tile, s, err, top)
    assert ran == ({1, 2} if tiles > 32 else {1})


# ---- the unforced dispatcher --------------------------------------------------------------------------------------------------
DISPATCH = [  # (MFMA mode, conv geometry) -> (N, K, M), kernel, S
    (1, (2, 19, 23, 64, 64, 3, 1, 1), (64, 576, 874), "split_128", 4),
    (1, (1, 38, 63, 256, 256, 3, 1, 1), (256, 2304, 2394), "split_128", 10),
    (1, (1, 6, 8, 1024, 512, 1, 1, 0), (512, 1024, 48), "split_128p", 1),
    (0, (4, 38, 63, 256, 128, 3, 1, 1), (128, 2304, 9576), "f32_128", 28),
]


@pytest.mark.parametrize("mode,geom,nkm,kern,slices", DISPATCH, ids=["mode%d-N%d-K%d-M%d" % ((d[0],) + d[2]) for d in DISPATCH])
def test_default_cost_model_reaches_the_production_forms(dev, mode, geom, nkm, kern, slices):
    """nothing forced: the kernel and S the cost model picks for production-like shapes are the ones recorded here, and the
    result meets the bound (float64 reference and torch's fp32 matmul both on the device: these operands are large)"""
    ops = _ops()
    ops.set_mfma_mode(mode)
    ops.force_wgrad(0, 0)
    b, h, w, cin, cout, k, stride, pad = geom
    g = torch.Generator().manual_seed(sum(geom))
    x = torch.randn(b, cin, h, w, generator=g).to(dev)
    cols = _im2col(x, k, stride, pad)
    assert (cout, cols.shape[1], cols.shape[0]) == nkm
    gy = torch.randn(cols.shape[0], cout, generator=g).to(dev)
    rows = x.permute(0, 2, 3, 1).reshape(-1, cin).contiguous()
    got = ops.conv2d_wgrad(gy, rows, b, h, w, cin, cout, k, k, stride, pad)
    f = ops.last_wgrad_form()
    assert f == ops.WgradForm(kern, slices, 1), f
    ref = gy.double().t() @ cols.double()
    mag = gy.double().abs().t() @ cols.double().abs()
    e_ref = float((((gy.t() @ cols).double() - ref).abs() / mag).max())
    _check(got, ref, mag, e_ref, f, "default dispatch %s" % (nkm,))
