"""Every kernel form behind csrc/igemm.hip's dispatch(), SELECTED in-process, PROVEN through the recorded form
(ops.last_igemm_form) and compared with a float64 contraction of the same fp32 operands -- at the smallest shapes at which a
tile, the staging pipeline, the XCD tile remap or an epilogue path can go wrong (the product reaches most of these forms at
workload size only):
  * the f32-MFMA kernel (set_mfma_mode(0));
  * the split kernel's four tiles (force_tile 2 / 3 / 4 / 5 = 128x64 / 64x64 / 128x128 / 64x128), fp32 weight rows and
    split_weight planes, register epilogue and LDS epilogue;
  * igemm_dma_kernel on fp32 activation rows (dma kernel 2: <128,2,0>, <64,2,0> for N <= 64);
  * planes x planes with 2 / 3 / 4 / 6 / 13 / 14 stages.
Bound (test_contraction_error_vs_fp64_is_at_the_fp32_level's rule): with mag = |alpha| |scale| (|a| . |b|) + |shift| +
|residual| per output element (ReLU is 1-Lipschitz and does not enter), max |got - ref| / mag <= 2 e_ref + 2e-7, where e_ref
is the same ratio of torch's own fp32 matmul / conv2d (+ the epilogue in fp32) on the device -- never one of the forms.
Bit identity is asserted only where igemm.hip claims it: the dma kernel and every planes x planes stage count against the
split kernel the dispatcher would pick, the LDS epilogue against the register epilogue of every forced tile.
Every output lies in a buffer of sentinels: guard columns [n, ldc), two rows in front, 130 rows behind (more than a
128-row tile can overshoot), NaN where the kernel must write.

GEMM shapes: m in {1, 63, 65, 127, 129, 257}, n in {9, 33, 64, 65, 72, 128, 130, 147, 257}, k in {16, 32, 48} (one to three
K-steps: fewer than the 2..6 pipeline stages), {80, 100, 208, 272} (100: the K padding of the planes), {4, 36} (fp32 weights
only), batch 1 / 3 with batch_c > m * ldc; plus n = 33, k = 32 with m = 64 g - 1 and 128 g - 1 rows for grids of g = 7, 8,
9, 17 tiles of 64 and of 128 rows (xcd_remap: 7 = one partial round of the eight XCDs, 8 = exactly one, 9 and 17 = one past
one and two rounds; a single tile is (63, 33, 32)).

Worst max |got - ref| / mag per form family over every case of this file, with the e_ref of that very case, as measured on
an MI355X (`pytest -s` prints the table again at the end of the module):
  f32-MFMA 64x64                         2.945e-07   (e_ref 2.945e-07)   gemm (511, 33, 32, 1), no epilogue
  split 128x64 / 64x64 / 128x128 / 64x128,
  dma on fp32 rows, planes x planes      3.794e-07   (e_ref 2.714e-07)   gemm (1087, 33, 32, 1), no epilogue
The six split-family rows are one number because they are one result: on all 140 (shape, epilogue) GEMM cases with weight
planes the four forced tiles returned each other's bits (measured once, not asserted: igemm.hip does not claim it).
"""
import collections

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SENT = -77.25
NAN = float("nan")
TILES = {2: (128, 64), 3: (64, 64), 4: (128, 128), 5: (64, 128)}
PP_FORMS = {2: (2, 0), 3: (3, 0), 4: (4, 0), 6: (6, 0), 13: (3, 1), 14: (4, 1)}  # stage value -> (NST, DF) for N > 64
STAGES = (2, 3, 4, 6, 13, 14)

GEMM_SHAPES = [  # (m, n, k, batch)
    (1, 9, 16, 1), (63, 33, 32, 1), (65, 64, 48, 1), (127, 65, 80, 1), (129, 72, 100, 1), (257, 128, 208, 1),
    (63, 130, 272, 1), (65, 147, 16, 3), (127, 257, 32, 1), (129, 9, 48, 3), (257, 33, 80, 1), (1, 64, 100, 3),
    (63, 65, 208, 3), (65, 72, 272, 1), (127, 128, 16, 1), (129, 130, 32, 3), (257, 147, 48, 1), (1, 257, 80, 1),
    (129, 64, 272, 1), (257, 257, 100, 1), (127, 147, 208, 3),
    (65, 33, 4, 1), (129, 130, 36, 1), (63, 64, 36, 3),                       # k = 4 / 36: fp32 weights only
    (447, 33, 32, 1), (511, 33, 32, 1), (575, 33, 32, 1), (1087, 33, 32, 1),  # 7 / 8 / 9 / 17 tiles of 64 rows (1087: 9 of 128)
    (895, 33, 32, 1), (1023, 33, 32, 1), (2175, 33, 32, 1),                   # 7 / 8 / 17 tiles of 128 rows
]
EPILOGUES = ("plain", "alpha_shift", "bn_res_relu", "unaligned_c", "unaligned_ss")
GROUPS = ("f32", "tile2", "tile3", "tile4", "tile5", "dma_pp")


def _ops():
    import dana_amd
    return dana_amd.ops


@pytest.fixture(autouse=True)
def _restore_forms():
    """tile 0, dma -1, pp -1, epilogue 0 and the previous mfma mode after every test"""
    ops = _ops()
    prev = ops.get_mfma_mode()
    yield
    ops.set_mfma_mode(1)
    ops.force_tile(0)
    ops.set_dma_kernel(-1)
    ops.set_pp_stages(-1)
    ops.set_epilogue_mode(0)
    ops.set_mfma_mode(prev)


_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _WORST:
        print("\nworst max |got - ref| / mag per family (its e_ref, the case):")
        for fam in sorted(_WORST):
            print("  %-12s %.3e  (e_ref %.3e)  %s" % ((fam,) + _WORST[fam]))


def _family(f):
    if f.family == "dma":
        return "dma_pp" if f.apre else "dma_a0"
    return "f32" if f.family == "f32" else "split%dx%d" % (f.bm, f.bn)


def _check(got, ref, mag, e_ref, form, what):
    ratio = float(((got.double() - ref).abs() / mag).max())
    fam = _family(form)
    if ratio > _WORST.get(fam, (-1.0,))[0]:
        _WORST[fam] = (ratio, e_ref, what)
    assert ratio <= 2.0 * e_ref + 2e-7, "%s %s: max |err| / mag %.3e, torch fp32 %.3e" % (what, form, ratio, e_ref)


class _Out:
    """`rows` x n outputs per batch slice (row stride ldc, slice stride batch_c > rows * ldc) inside a buffer of sentinels:
    NaN where the kernel must write, SENT in the guard columns, two rows in front, 130 rows behind, `off` floats in front"""

    def __init__(self, dev, rows, n, ldc, batch=1, off=0):
        self.rows, self.n, self.ldc, self.batch = rows, n, ldc, batch
        self.batch_c = (rows + 132) * ldc
        self.c_off = off + 2 * ldc
        self.buf = torch.full((off + batch * self.batch_c + 4,), SENT, device=dev)
        self.region = torch.as_strided(self.buf, (batch, rows, n), (self.batch_c, ldc, 1), self.c_off)
        self.region.fill_(NAN)
        self.pre = self.buf.clone()

    def ptr(self):
        return self.buf.data_ptr() + 4 * self.c_off

    def tensor(self):
        return self.buf[self.c_off:]

    def take(self, what):
        got = self.region.clone()
        self.region.fill_(NAN)
        assert torch.equal(self.buf.view(torch.int32), self.pre.view(torch.int32)), "%s: a sentinel was overwritten" % (what,)
        assert bool(torch.isfinite(got).all()), "%s: an output element was not written (or is not finite)" % (what,)
        return got[0] if self.batch == 1 else got


def _up4(n):
    return (n + 3) // 4 * 4


# ---- GEMM cases: operands, float64 reference, mag and e_ref, computed once per (shape, epilogue) and left unchanged --------------
GemmCase = collections.namedtuple("GemmCase", "a b scale shift res alpha relu ldc ldr off ref mag e_ref")
_GEMM = {}
_PLANES = {}


def _gemm_case(dev, shape, epi):
    key = (shape, epi)
    if key in _GEMM:
        return _GEMM[key]
    m, n, k, batch = shape
    g = torch.Generator().manual_seed(1000 * m + 10 * n + k + batch)
    a = torch.randn(batch, m, k, generator=g)
    b = torch.randn(batch, n, k, generator=g) / np.sqrt(k)
    scale = shift = res = sbase = hbase = None
    alpha, relu, ldc, ldr, off = 1.0, False, n, 0, 0
    if epi == "alpha_shift":
        alpha, shift = -0.37, torch.randn(n, generator=g)
    elif epi == "bn_res_relu":  # (a residual needs batch == 1: dana_gemm_nt)
        scale, shift, relu = torch.rand(n, generator=g) + 0.5, torch.randn(n, generator=g), True
        ldc = _up4(n) + 4
        if batch == 1:
            ldr = ldc + 4
            res = torch.randn(m, ldr, generator=g)
    elif epi == "unaligned_c":  # rows of n + 1 floats from a pointer 4 bytes past a 16-byte boundary: vec_io = 0
        scale, shift, relu = torch.rand(n, generator=g) + 0.5, torch.randn(n, generator=g), True
        ldc = n + 1
        off = (1 - 2 * ldc) % 4
    elif epi == "unaligned_ss":  # scale / shift start one float into their buffers: vec_ss = 0
        sbase, hbase = torch.rand(n + 1, generator=g) + 0.5, torch.randn(n + 1, generator=g)
        scale, shift = sbase[1:], hbase[1:]
        ldc = _up4(n) + 4
    a64, b64 = a.double(), b.double()
    sc64 = scale.double() if scale is not None else torch.ones(n, dtype=torch.float64)
    ref = alpha * sc64 * (a64 @ b64.transpose(1, 2))
    mag = abs(alpha) * sc64.abs() * (a64.abs() @ b64.abs().transpose(1, 2))
    if shift is not None:
        ref, mag = ref + shift.double(), mag + shift.double().abs()
    if res is not None:
        ref, mag = ref + res[:, :n].double(), mag + res[:, :n].double().abs()
    if relu:
        ref = torch.relu(ref)
    d = lambda t: None if t is None else t.to(dev)  # noqa: E731
    ad, bd, scd, shd, resd = d(a), d(b), d(scale), d(shift), d(res)
    if sbase is not None:
        scd, shd = sbase.to(dev)[1:], hbase.to(dev)[1:]
        assert scd.data_ptr() % 16 == 4 and shd.data_ptr() % 16 == 4
    t32 = torch.matmul(ad, bd.transpose(1, 2)) * alpha
    if scd is not None:
        t32 = t32 * scd
    if shd is not None:
        t32 = t32 + shd
    if resd is not None:
        t32 = t32 + resd[:, :n]
    if relu:
        t32 = torch.relu(t32)
    ref, mag = ref.to(dev), mag.to(dev)
    if batch == 1:
        ref, mag, t32 = ref[0], mag[0], t32[0]
    e_ref = float(((t32.double() - ref).abs() / mag).max())
    _GEMM[key] = GemmCase(ad, bd, scd, shd, resd, alpha, relu, ldc, ldr, off, ref, mag, e_ref)
    return _GEMM[key]


def _planes(ops, dev, shape):
    """(weight planes, activation planes) of a shape's operands (the operands do not depend on the epilogue)"""
    if shape not in _PLANES:
        m, n, k, batch = shape
        c = _gemm_case(dev, shape, "plain")
        _PLANES[shape] = (ops.split_weight(c.b.view(-1), n, k, batch=batch), ops.split_weight(c.a.view(-1), m, k, batch=batch))
    return _PLANES[shape]


def _gemm(ops, dev, shape, c, a_planes=None, b_planes=None, what=""):
    m, n, k, batch = shape
    out = _Out(dev, m, n, c.ldc, batch, c.off)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    flags = ops.EPI_RELU if c.relu else 0
    pa, lda, batch_a = c.a.data_ptr(), k, m * k
    pb, ldb, batch_b = c.b.data_ptr(), k, n * k
    if b_planes is not None:
        pb, ldb, batch_b, flags = b_planes.t.data_ptr(), b_planes.kp, 3 * n * b_planes.kp, flags | ops.W_SPLIT3
    if a_planes is not None:
        pa, lda, batch_a, flags = a_planes.t.data_ptr(), a_planes.kp, 3 * m * a_planes.kp, flags | ops.A_SPLIT3
    ops.lib().call("dana_gemm_nt", pa, pb, out.ptr(), p(c.scale), p(c.shift), p(c.res), m, n, k, lda, ldb, c.ldc, c.ldr, batch,
                   batch_a, batch_b, out.batch_c, c.alpha, flags, ops._stream())
    return out.take(what), ops.last_igemm_form()


def _split_form(ops, tile, bpre, elds):
    bm, bn = TILES[tile]
    return ops.IgemmForm("split_128" if tile == 4 else "split", bm, bn, 0, bpre, 0, elds, 0, 0, 0)


def _picked_form(ops, n):
    """the split kernel dispatch() picks for a launch of fewer than 100 128x128 tiles on split weights"""
    return _split_form(ops, 2 if n <= 64 else 3, 1, 0)


def _dma_form(ops, n, apre=0, stages=2):
    if n <= 64:
        return ops.IgemmForm("dma", 128, 64, 0, 1, 0, 0, (2 if stages == 2 else 3) if apre else 2, apre, 0)
    nst, df = PP_FORMS[stages] if apre else (2, 0)
    return ops.IgemmForm("dma", 128, 128, 0, 1, 0, 0, nst, apre, df)


# (k = 4 / 36 come with fp32 weights only: no planes, so no dma / planes x planes group)
GEMM_PARAMS = [(s, g) for s in GEMM_SHAPES for g in GROUPS if not (g == "dma_pp" and s[2] in (4, 36))]


@pytest.mark.parametrize("shape,group", GEMM_PARAMS, ids=["m%d-n%d-k%d-b%d-" % s + g for s, g in GEMM_PARAMS])
def test_gemm_form_vs_fp64(dev, shape, group):
    """one group of forms on one shape under all five epilogues: f32 | a forced tile (fp32 weights and planes, register and
    LDS epilogue, the two bit for bit) | the dispatcher's split kernel, the dma kernel and every planes x planes stage count
    (all bit for bit)"""
    ops = _ops()
    m, n, k, batch = shape
    fp32_only = k in (4, 36)
    for epi in EPILOGUES:
        c = _gemm_case(dev, shape, epi)
        what = "gemm %s %s" % (shape, epi)
        if group == "f32":
            ops.set_mfma_mode(0)
            got, f = _gemm(ops, dev, shape, c, what=what)
            assert f == ops.IgemmForm("f32", 64, 64, 0, 0, 0, 0, 0, 0, 0), f
            _check(got, c.ref, c.mag, c.e_ref, f, what)
            continue
        ops.set_mfma_mode(1)
        w3, a3 = (None, None) if fp32_only else _planes(ops, dev, shape)
        if group.startswith("tile"):
            tile = int(group[4:])
            for planes in ((None,) if fp32_only else (None, w3)):
                bits = []
                for elds in (0, 1):
                    with ops.igemm_forms(tile=tile, epilogue=elds):
                        got, f = _gemm(ops, dev, shape, c, b_planes=planes, what=what)
                    assert f == _split_form(ops, tile, int(planes is not None), elds), f
                    _check(got, c.ref, c.mag, c.e_ref, f, what)
                    bits.append(got)
                assert torch.equal(bits[0], bits[1]), "%s tile %d: the LDS epilogue's bits differ from the register epilogue's" % (what, tile)
            continue
        with ops.igemm_forms(dma=0):
            base, f = _gemm(ops, dev, shape, c, b_planes=w3, what=what)
        assert f == _picked_form(ops, n), f
        _check(base, c.ref, c.mag, c.e_ref, f, what)
        with ops.igemm_forms(dma=2):
            got, f = _gemm(ops, dev, shape, c, b_planes=w3, what=what)
        assert f == _dma_form(ops, n), f
        _check(got, c.ref, c.mag, c.e_ref, f, what)
        assert torch.equal(got, base), "%s: %s differs from %s" % (what, f, _picked_form(ops, n))
        for st in STAGES:
            with ops.igemm_forms(pp=st):
                got, f = _gemm(ops, dev, shape, c, a_planes=a3, b_planes=w3, what=what)
            assert f == _dma_form(ops, n, 1, st), (st, f)
            _check(got, c.ref, c.mag, c.e_ref, f, what)
            assert torch.equal(got, base), "%s: planes x planes, %d stages: %s differs from %s" % (what, st, f, _picked_form(ops, n))


# ---- default dispatch reaches the production forms ----------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,k,expect", [(76800, 128, 64, ("dma", 128, 128, 2, 0)), (49, 147, 256, ("split", 64, 64, 0, 0)),
                                          (300, 64, 64, ("split", 128, 64, 0, 0))],
                         ids=["layer1-expand-dma", "narrow-last-column-64x64", "n64-128x64"])
def test_default_dispatch_reaches_the_production_form(dev, m, n, k, expect):
    """nothing forced: 600 128x128 tiles, K <= 192, N > 64 on split weights -> igemm_dma_kernel<128,2,0> (what the layer1 /
    layer2 expand convs run); a narrow last column tile -> 64x64; N <= 64 -> 128x64. Each against float64."""
    ops = _ops()
    ops.set_mfma_mode(1)
    assert (ops.get_dma_kernel(), ops.get_pp_stages()) in ((-1, -1), (1, -1)), "DANA_DMA_KERNEL / DANA_PP_STAGES are set"
    g = torch.Generator().manual_seed(m + n + k)
    a, b = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g) / np.sqrt(k)
    sc, sh = torch.rand(n, generator=g) + 0.5, torch.randn(n, generator=g)
    ad, bd, scd, shd = a.to(dev), b.to(dev), sc.to(dev), sh.to(dev)
    got = ops.gemm_nt(ad, ops.split_weight(bd, n, k), m, n, k, scale=scd, shift=shd, relu=True, force_slices=1)
    f = ops.last_igemm_form()
    assert (f.family, f.bm, f.bn, f.nst, f.apre) == expect and f.bpre == 1 and f.elds == 0, f
    ref = torch.relu(sc.double() * (a.double() @ b.double().t()) + sh.double()).to(dev)
    mag = (sc.double() * (a.double().abs() @ b.double().abs().t()) + sh.double().abs()).to(dev)
    t32 = torch.relu((ad @ bd.t()) * scd + shd)
    e_ref = float(((t32.double() - ref).abs() / mag).max())
    _check(got, ref, mag, e_ref, f, "default dispatch %s" % ((m, n, k),))


# ---- conv geometry under each forced form --------------------------------------------------------------------------------------
CONV_GEOMS = [(32, 96, 3, 1, 1), (64, 160, 3, 2, 1), (64, 96, 1, 2, 0), (32, 160, 1, 1, 0)]  # (cin, cout, k, stride, pad)
IMAGES = [(9, 11), (5, 7)]
NB = 2
CONV_FORMS = [("tile%d" % t, w) for t in (2, 3, 4, 5) for w in ("fp32", "planes")] + [("dma", "planes")]


def _rows(t):
    """NCHW -> [N*H*W][C] pixel rows"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.size(1)).contiguous()


def _oihw(w, cout, k, cin):
    """packed [cout][kh][kw][cin] -> OIHW"""
    return w.view(cout, k, k, cin).permute(0, 3, 1, 2).contiguous()


ConvCase = collections.namedtuple("ConvCase", "xbuf lda w scale shift res ldr ref mag e_ref oh ow")
_CONV = {}


def _conv_case(dev, geom, hw):
    """one image group: x inside a wider buffer (in_stride = cin + 8, first channel at column 4), bn + residual + ReLU"""
    key = (geom, hw)
    if key in _CONV:
        return _CONV[key]
    cin, cout, k, stride, pad = geom
    h, w_ = hw
    gw = torch.Generator().manual_seed(cin + 3 * cout + 7 * k + 11 * stride)  # one filter per geometry: the dual launch
    w = torch.randn(cout, k * k * cin, generator=gw) / np.sqrt(k * k * cin)
    scale, shift = torch.rand(cout, generator=gw) + 0.5, torch.randn(cout, generator=gw)
    g = torch.Generator().manual_seed(cin + 3 * cout + 7 * k + 11 * stride + h)
    x = torch.randn(NB, cin, h, w_, generator=g)
    wo = _oihw(w, cout, k, cin)
    y = F.conv2d(x.double(), wo.double(), stride=stride, padding=pad)
    ymag = F.conv2d(x.double().abs(), wo.double().abs(), stride=stride, padding=pad)
    oh, ow = y.shape[2:]
    ldr = cout + 8
    res = torch.randn(NB * oh * ow, ldr, generator=g)
    r64 = res[:, :cout].double()
    ref = torch.relu(_rows(y) * scale.double() + shift.double() + r64)
    mag = _rows(ymag) * scale.double() + shift.double().abs() + r64.abs()
    lda = cin + 8
    xbuf = torch.full((NB * h * w_ + 1, lda), 1e30)  # (what lies around the channels must not be read)
    xbuf[:NB * h * w_, 4:4 + cin] = _rows(x)
    xd, wd, scd, shd, resd = x.to(dev), wo.to(dev), scale.to(dev), shift.to(dev), res.to(dev)
    t32 = torch.relu(_rows(F.conv2d(xd, wd, stride=stride, padding=pad)) * scd + shd + resd[:, :cout])
    ref, mag = ref.to(dev), mag.to(dev)
    e_ref = float(((t32.double() - ref).abs() / mag).max())
    _CONV[key] = ConvCase(xbuf.to(dev), lda, w.to(dev), scd, shd, resd, ldr, ref, mag, e_ref, oh, ow)
    return _CONV[key]


def _conv_form(ops, form, weights, cout):
    """(igemm_forms arguments, the form that must be recorded)"""
    if form == "dma":
        return dict(dma=2), _dma_form(ops, cout)
    tile = int(form[4:])
    return dict(tile=tile), _split_form(ops, tile, int(weights == "planes"), 0)


@pytest.mark.parametrize("form,weights", CONV_FORMS, ids=["%s-%s" % fw for fw in CONV_FORMS])
@pytest.mark.parametrize("geom", CONV_GEOMS, ids=lambda g_: "c%d-%d-k%ds%dp%d" % g_)
def test_conv_geometry_under_each_form_vs_fp64(dev, geom, form, weights):
    """3x3 / 1x1, stride 1 / 2, padding, in_stride > cin, frozen-BN + residual (row stride > cout) + ReLU into guarded rows,
    images 9x11 and 5x7 one by one and together as the two geometry segments of conv2d_nhwc_dual (a tile straddles M0)"""
    ops = _ops()
    ops.set_mfma_mode(1)
    cin, cout, k, stride, pad = geom
    sel, expect = _conv_form(ops, form, weights, cout)
    cases = [_conv_case(dev, geom, hw) for hw in IMAGES]
    wt = cases[0].w
    wt = ops.split_weight(wt, cout, k * k * cin) if weights == "planes" else wt
    ldc = cout + 4
    single = []
    for (h, w_), c in zip(IMAGES, cases):
        what = "conv %s %dx%d %s %s" % (geom, h, w_, form, weights)
        out = _Out(dev, NB * c.oh * c.ow, cout, ldc)
        with ops.igemm_forms(**sel):
            ops.conv2d_nhwc(c.xbuf.view(-1)[4:], NB, h, w_, cin, wt, cout, k, k, stride, pad, scale=c.scale, shift=c.shift,
                            residual=c.res, relu=True, in_stride=c.lda, out=out.tensor(), out_stride=ldc, res_stride=c.ldr)
            f = ops.last_igemm_form()
        assert f == expect, f
        got = out.take(what)
        _check(got, c.ref, c.mag, c.e_ref, f, what)
        if form == "dma":
            base = _Out(dev, NB * c.oh * c.ow, cout, ldc)
            with ops.igemm_forms(dma=0):
                ops.conv2d_nhwc(c.xbuf.view(-1)[4:], NB, h, w_, cin, wt, cout, k, k, stride, pad, scale=c.scale, shift=c.shift,
                                residual=c.res, relu=True, in_stride=c.lda, out=base.tensor(), out_stride=ldc, res_stride=c.ldr)
                assert ops.last_igemm_form() == _picked_form(ops, cout)
            assert torch.equal(got, base.take(what)), "%s: differs from the split kernel" % what
        single.append(got)
    # both image groups in one launch: group 0's pixels, then group 1's (contiguous rows here: one pixel stride for both)
    c0, c1 = cases
    (h0, w0), (h1, w1) = IMAGES
    x2 = torch.cat([c0.xbuf[:NB * h0 * w0], c1.xbuf])
    o0, o1 = _Out(dev, NB * c0.oh * c0.ow, cout, ldc), _Out(dev, NB * c1.oh * c1.ow, cout, ldc + 4)
    what = "conv dual %s %s %s" % (geom, form, weights)
    with ops.igemm_forms(**sel):
        ops.conv2d_nhwc_dual(x2.view(-1)[4:], NB, h0, w0, NB, h1, w1, cin, wt, cout, k, k, stride, pad, scale=c0.scale,
                             shift=c0.shift, res0=c0.res, res1=c1.res, relu=True, in_stride=c0.lda, out0=o0.tensor(),
                             out1=o1.tensor(), out0_stride=ldc, out1_stride=ldc + 4, res0_stride=c0.ldr, res1_stride=c1.ldr)
        f = ops.last_igemm_form()
    assert f == expect, f
    for o, c in ((o0, c0), (o1, c1)):
        _check(o.take(what), c.ref, c.mag, c.e_ref, f, what)


@pytest.mark.parametrize("weights", ["fp32", "planes"])
@pytest.mark.parametrize("tile", [2, 3, 4, 5])
@pytest.mark.parametrize("geom", CONV_GEOMS[:2], ids=lambda g_: "c%d-%d-k%ds%dp%d" % g_)
def test_masked_conv_stays_on_the_split_tiles_vs_fp64(dev, geom, tile, weights):
    """dana_conv2d_nhwc_masked (the data-gradient form: out = mask > 0 ? out : 0) under each forced tile; without a forced
    tile and with the dma kernel asked for wherever it can run, a mask still keeps the launch on the split kernel"""
    ops = _ops()
    ops.set_mfma_mode(1)
    cin, cout, k, stride, pad = geom
    h, w_ = IMAGES[0]
    c = _conv_case(dev, geom, IMAGES[0])
    rows = NB * c.oh * c.ow
    g = torch.Generator().manual_seed(tile + cout)
    mask = torch.randn(rows, cout + 4, generator=g).to(dev)
    keep = mask[:, :cout] > 0
    wt = ops.split_weight(c.w, cout, k * k * cin) if weights == "planes" else c.w
    ldc = cout + 4
    for sel, expect in ((dict(tile=tile), _split_form(ops, tile, int(weights == "planes"), 0)),
                        (dict(dma=2), _split_form(ops, 2 if cout <= 64 else 3, int(weights == "planes"), 0))):
        what = "masked conv %s %s %s" % (geom, sel, weights)
        out = _Out(dev, rows, cout, ldc)
        with ops.igemm_forms(**sel):
            ops.lib().call("dana_conv2d_nhwc_masked", c.xbuf.data_ptr() + 16, wt.t.data_ptr() if weights == "planes" else wt.data_ptr(),
                           out.ptr(), c.scale.data_ptr(), c.shift.data_ptr(), c.res.data_ptr(), mask.data_ptr(), NB, h, w_, cin, cout,
                           k, k, stride, pad, c.lda, ldc, c.ldr, cout + 4,
                           ops.EPI_RELU | (ops.W_SPLIT3 if weights == "planes" else 0), ops._stream())
            f = ops.last_igemm_form()
        assert f == expect, f
        got = out.take(what)
        assert bool((got[~keep] == 0).all()), "%s: an element behind mask <= 0 is not zero" % what
        _check(torch.where(keep, got, c.ref.float()), c.ref, c.mag, c.e_ref, f, what)


# ---- the two-segment K walk (expand conv + strided downsample conv as one contraction) ---------------------------------------
CAT2 = [(16, 48, 1), (16, 48, 2), (64, 32, 1), (64, 32, 2)]  # (k0, k1, stride)
CAT2_COUT = 96
Cat2Case = collections.namedtuple("Cat2Case", "a0 a1 w shift ref mag e_ref m")
_CAT2 = {}


def _cat2_case(dev, k0, k1, stride, hw):
    key = (k0, k1, stride, hw)
    if key in _CAT2:
        return _CAT2[key]
    h, w_ = hw
    oh, ow = (h - 1) // stride + 1, (w_ - 1) // stride + 1
    g = torch.Generator().manual_seed(k0 + 3 * k1 + 5 * stride + h)
    t = torch.randn(NB, k0, oh, ow, generator=g)
    x = torch.randn(NB, k1, h, w_, generator=g)
    # (one weight and one shift per (k0, k1): both image sizes go through one dual launch)
    gw = torch.Generator().manual_seed(k0 + 3 * k1)
    w = torch.randn(CAT2_COUT, k0 + k1, generator=gw) / np.sqrt(k0 + k1)
    shift = torch.randn(CAT2_COUT, generator=gw)
    w0, w1 = w[:, :k0].reshape(CAT2_COUT, k0, 1, 1).contiguous(), w[:, k0:].reshape(CAT2_COUT, k1, 1, 1).contiguous()
    y = F.conv2d(t.double(), w0.double()) + F.conv2d(x.double(), w1.double(), stride=stride)
    ymag = F.conv2d(t.double().abs(), w0.double().abs()) + F.conv2d(x.double().abs(), w1.double().abs(), stride=stride)
    ref = torch.relu(_rows(y) + shift.double()).to(dev)
    mag = (_rows(ymag) + shift.double().abs()).to(dev)
    td, xd, shd = t.to(dev), x.to(dev), shift.to(dev)
    t32 = torch.relu(_rows(F.conv2d(td, w0.to(dev)) + F.conv2d(xd, w1.to(dev), stride=stride)) + shd)
    e_ref = float(((t32.double() - ref).abs() / mag).max())
    _CAT2[key] = Cat2Case(_rows(td), _rows(xd), w.to(dev), shd, ref, mag, e_ref, NB * oh * ow)
    return _CAT2[key]


@pytest.mark.parametrize("form,weights", CONV_FORMS, ids=["%s-%s" % fw for fw in CONV_FORMS])
@pytest.mark.parametrize("k0,k1,stride", CAT2, ids=lambda v: str(v))
def test_two_segment_k_walk_under_each_form_vs_fp64(dev, k0, k1, stride, form, weights):
    """conv1x1_cat2 on 9x11 and 5x7 images and conv1x1_cat2_dual over both, under each forced tile and the dma kernel"""
    ops = _ops()
    ops.set_mfma_mode(1)
    cout = CAT2_COUT
    sel, expect = _conv_form(ops, form, weights, cout)
    cases = [_cat2_case(dev, k0, k1, stride, hw) for hw in IMAGES]
    wt = cases[0].w
    wt = ops.split_weight(wt, cout, k0 + k1) if weights == "planes" else wt
    ldc = cout + 4
    for (h, w_), c in zip(IMAGES, cases):
        what = "cat2 %s %dx%d %s %s" % ((k0, k1, stride), h, w_, form, weights)
        out = _Out(dev, c.m, cout, ldc)
        with ops.igemm_forms(**sel):
            ops.conv1x1_cat2(c.a0, k0, c.a1, k1, NB, h, w_, stride, wt, c.shift, cout, relu=True, out=out.tensor(), out_stride=ldc)
            f = ops.last_igemm_form()
        assert f == expect, f
        got = out.take(what)
        _check(got, c.ref, c.mag, c.e_ref, f, what)
        if form == "dma":
            base = _Out(dev, c.m, cout, ldc)
            with ops.igemm_forms(dma=0):
                ops.conv1x1_cat2(c.a0, k0, c.a1, k1, NB, h, w_, stride, wt, c.shift, cout, relu=True, out=base.tensor(), out_stride=ldc)
                assert ops.last_igemm_form() == _picked_form(ops, cout)
            assert torch.equal(got, base.take(what)), "%s: differs from the split kernel" % what
    c0, c1 = cases
    (h0, w0), (h1, w1) = IMAGES
    o0, o1 = _Out(dev, c0.m, cout, ldc), _Out(dev, c1.m, cout, ldc + 4)
    what = "cat2 dual %s %s %s" % ((k0, k1, stride), form, weights)
    with ops.igemm_forms(**sel):
        ops.conv1x1_cat2_dual(torch.cat([c0.a0, c1.a0]), k0, torch.cat([c0.a1, c1.a1]), k1, NB, h0, w0, NB, h1, w1, stride, wt,
                              c0.shift, cout, relu=True, out0=o0.tensor(), out1=o1.tensor(), out0_stride=ldc, out1_stride=ldc + 4)
        f = ops.last_igemm_form()
    assert f == expect, f
    for o, c in ((o0, c0), (o1, c1)):
        _check(o.take(what), c.ref, c.mag, c.e_ref, f, what)
