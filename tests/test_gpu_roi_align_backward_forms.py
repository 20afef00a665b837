"""The four forms of dana_roi_align_backward (csrc/roi_ops.hip), each REACHED by shape, PROVEN through the recorded form
(ops.last_roi_align_backward_form) and compared with oracle.native.roi_align_backward -- the reference's fp32 per-sample
contributions, summed in float64:
  * roi_align_bwd_gather_nhwc (NHWC, P <= 8, C % 4 == 0: the form the training step uses) on maps (C, H, W) = (4,1,1), (8,1,9),
    (260,7,5), (1028,6,7), (2052,3,4) -- masked lanes, the second pass of the channel loop, odd sides, H or W of 1 -- with
    P in {1, 7, 8}, sampling_ratio in {0, 2}, R in {1, 64, 65, 130} (one to three ballot rounds; R in {1, 20} where C > 1000:
    the oracle stays under a second), B = 3 with an image no roi names;
  * roi_align_bwd_nhwc_bins (NHWC, P in {9, 14}) on (8,12,20) and (260,128,5);
  * roi_align_bwd<true> (the NHWC atomic scatter) on (8,129,4) with P = 9, on (6,10,12) (C % 4 != 0) and on (8,5,129) with P = 9;
  * roi_align_bwd<false> (NCHW) on (6,10,12) with P = 7;
  * R = 0 in both layouts: zeros, form "memset".
Bound per element (derived, not measured): |got - ref| <= (T + 8) 2^-24 mag, where mag is the same oracle call on |g| (the
weights are non-negative: the sum of |contributions| of that cell), T = (rois of that image) x P^2 is the longest fp32 sum a
cell can receive and 8 covers the roundings of one contribution. Where mag == 0 the result must be exactly +0.0 in every form;
the output is prefilled with NaN (the gather claims to write every cell and runs without a memset). The gather runs twice and
returns the same bits. One case per form is also checked as an adjoint in float64, <g, fwd(x)> == <bwd(g), x> to 1e-5 relative,
against roi_align_forward(_nhwc), independently of the oracle's backward.

Besides random rois every case with R >= 20 holds hand-written ones (spatial scale 1/16): edges on exact multiples of 16, a
roi narrower than one cell (forced size 1), zero-size rois, a roi ending exactly one cell before the tile of cells 2..3 and
one starting exactly one cell behind it (the hit box's boundary), rois wholly outside (left by more than 16 px, above, beyond
W * 16 and H * 16), one covering the map many times over (adaptive grid 5) and rois whose samples fall into (-1, 0) and
(H - 1, H), the clamped band.

Worst |got - ref| / ((T + 8) 2^-24 mag) per form over every case of this file (1 = the bound), with the same error in units of
2^-24 mag, as measured on an MI355X (`pytest -s` prints the table again at the end of the module):
  gather        0.371  (3.34 x 2^-24 mag, T = 1)      C=260 7x5 P=1 sr=0 R=1
  bins          0.006  (4.23 x 2^-24 mag, T = 648)    C=260 128x5 P=9 sr=2 R=20
  scatter_nhwc  0.011  (18.66 x 2^-24 mag, T = 1617)  C=6 10x12 P=7 sr=2 R=65
  scatter_nchw  0.013  (21.52 x 2^-24 mag, T = 1617)  C=6 10x12 P=7 sr=2 R=65
(the adjoint products agreed to 4e-8 relative or better in all ten cases)
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SCALE = 1.0 / 16
B = 3  # image 1 is named by no roi
NAN = float("nan")
EPS = 2.0 ** -24


def _ops():
    import dana_amd
    return dana_amd.ops


def _oracle():
    from oracle import native
    return native


_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _WORST:
        print("\nworst |got - ref| / ((T + 8) 2^-24 mag) per form (the same error / (2^-24 mag), its T, the case):")
        for form in sorted(_WORST):
            print("  %-13s %.3f  (%.2f, T = %d)  %s" % ((form,) + _WORST[form]))


def _hand_rois(H, W, P):
    """[x1, y1, x2, y2] in pixels"""
    big = 16.0 * (5 * P - 0.5)  # 5 P - 0.5 cells: ceil(size / P) = 5 samples per bin and axis
    cx, cy = 8.0 * W, 8.0 * H
    return [
        [0, 0, 16 * min(W, 3), 16 * min(H, 2)],              # edges on exact multiples of 16
        [16, 16, 48, 32],
        [5, 5, 9, 30],                                       # narrower than one cell: forced size 1
        [8, 8, 8, 8], [0, 0, 0, 0],                          # zero size
        [0, 0, 16, 16],                                      # ends exactly one cell before the tile of cells 2..3 (both axes)
        [64, 64, 96, 90],                                    # starts exactly one cell behind it
        [-60, 0, -20, 30], [0, -80, 30, -20],                # wholly outside: left by more than 16 px, above
        [W * 16 + 20, 0, W * 16 + 60, 20], [0, H * 16 + 20, 20, H * 16 + 70],  # beyond W * 16, beyond H * 16
        [cx - big / 2, cy - big / 2, cx + big / 2, cy + big / 2],             # covers the map many times over
        [-12, -12, 12, 12],                                  # samples in (-1, 0)
        [W * 16 - 20, H * 16 - 20, W * 16 - 2, H * 16 - 2],  # samples in (W - 1, W) and (H - 1, H)
    ]


def _rois(H, W, P, R, seed):
    rng = np.random.default_rng(seed)
    rois = np.zeros((R, 5), np.float32)
    x1, y1 = rng.uniform(-20, W * 16, R), rng.uniform(-20, H * 16, R)
    rois[:, 1], rois[:, 2] = x1, y1
    rois[:, 3] = x1 + rng.uniform(0, min(2 * W * 16, 80 * P), R)  # at most 5 P cells: adaptive grids <= 5
    rois[:, 4] = y1 + rng.uniform(0, min(2 * H * 16, 80 * P), R)
    if R >= 20:
        hand = np.asarray(_hand_rois(H, W, P), np.float32)
        rois[:len(hand), 1:] = hand
    rois[:, 0] = 2 * rng.integers(0, 2, R)  # images 0 and 2
    return rois


def _backward(ops, dev, g_dev, rois_dev, R, C, H, W, PH, PW, sr, layout, batch=B):
    shape = (batch, C, H, W) if layout == ops.NCHW else (batch, H, W, C)
    gin = torch.full(shape, NAN, device=dev)
    ops.lib().call("dana_roi_align_backward", None if g_dev is None else g_dev.data_ptr(),
                   None if rois_dev is None else rois_dev.data_ptr(), gin.data_ptr(), batch, C, H, W, R, SCALE, PH, PW, sr, layout,
                   ops._stream())
    return gin, ops.last_roi_align_backward_form()


def _case(dev, C, H, W, P, sr, R, layout, expect, seed, adjoint=False):
    """one launch against the oracle; returns the gradient as [B][C][H][W]"""
    ops, orc = _ops(), _oracle()
    nhwc = layout == "nhwc"
    rois = _rois(H, W, P, R, seed)
    rng = np.random.default_rng(seed + 1)
    g = rng.normal(size=(R, C, P, P)).astype(np.float32)
    if adjoint:
        g = np.abs(g) + 0.5
    ref = orc.roi_align_backward(g, rois, SCALE, P, P, B, C, H, W, sr)
    mag = orc.roi_align_backward(np.abs(g), rois, SCALE, P, P, B, C, H, W, sr)
    g_dev = torch.from_numpy(g).to(dev)
    if nhwc:
        g_dev = g_dev.permute(0, 2, 3, 1).contiguous()
    rois_dev = torch.from_numpy(rois).to(dev)
    what = "%s C=%d %dx%d P=%d sr=%d R=%d" % (expect, C, H, W, P, sr, R)
    gin, form = _backward(ops, dev, g_dev, rois_dev, R, C, H, W, P, P, sr, ops.NHWC if nhwc else ops.NCHW)
    assert form == expect, (what, form)
    if expect == "gather":  # fixed summation order, every cell written once: the same bits again, into NaN again
        again, form = _backward(ops, dev, g_dev, rois_dev, R, C, H, W, P, P, sr, ops.NHWC)
        assert form == "gather" and torch.equal(gin.view(torch.int32), again.view(torch.int32)), what
    got_t = gin.permute(0, 3, 1, 2) if nhwc else gin
    got = got_t.cpu().numpy()
    assert np.isfinite(got).all(), "%s: a cell was not written (or is not finite)" % what
    zero = mag == 0
    assert not got[zero].view(np.int32).any(), "%s: a cell no sample touches is not +0.0" % what
    assert zero[1].all(), "image 1 has a roi"
    T = np.array([(rois[:, 0] == b).sum() * P * P for b in range(B)], np.float64).reshape(B, 1, 1, 1)
    err = np.abs(got.astype(np.float64) - ref)
    units = np.where(zero, 0.0, err / np.where(zero, 1.0, EPS * mag))  # error in units of 2^-24 mag
    ratio = units / (T + 8)
    i = np.unravel_index(np.argmax(ratio), ratio.shape)
    print("%s: worst ratio %.3f (%.2f x 2^-24 mag, T = %d)" % (what, ratio[i], units[i], T[i[0], 0, 0, 0]))
    if ratio[i] > _WORST.get(expect, (-1.0,))[0]:
        _WORST[expect] = (float(ratio[i]), float(units[i]), int(T[i[0], 0, 0, 0]), what)
    assert ratio[i] <= 1.0, "%s: |got - ref| = %.2f x 2^-24 mag at %s, bound T + 8 = %d" % (what, units[i], i, T[i[0], 0, 0, 0] + 8)
    if adjoint:
        x = np.random.default_rng(seed + 2).uniform(0.5, 1.5, size=(B, C, H, W)).astype(np.float32)
        x_dev = torch.from_numpy(x).to(dev)
        if nhwc and C % 4 == 0:
            feat = x_dev.permute(0, 2, 3, 1).contiguous()
            y, _ = ops.roi_align_forward_nhwc(feat, B, H, W, C, C, rois_dev, SCALE, P, sr)
            lhs = float((y.double() * g_dev.view(R, P * P, C).double()).sum())
        else:  # (the NHWC forward needs C % 4 == 0: the NCHW forward is the same operator, bit for bit)
            y = ops.roi_align_forward(x_dev, rois_dev, SCALE, P, P, sr)
            lhs = float((y.double() * torch.from_numpy(g).to(dev).double()).sum())
        rhs = float((got_t.double() * x_dev.double()).sum())
        print("%s: adjoint <g, fwd x> = %.9e, <bwd g, x> = %.9e" % (what, lhs, rhs))
        assert lhs > 0 and abs(lhs - rhs) <= 1e-5 * abs(lhs), (what, lhs, rhs)
    return got


GATHER_MAPS = [(4, 1, 1), (8, 1, 9), (260, 7, 5), (1028, 6, 7), (2052, 3, 4)]


@pytest.mark.parametrize("sr", [0, 2])
@pytest.mark.parametrize("P", [1, 7, 8])
@pytest.mark.parametrize("chw", GATHER_MAPS, ids=lambda m_: "c%d-%dx%d" % m_)
def test_gather_vs_oracle(dev, chw, P, sr):
    """the NHWC gather: every map x pooled size x sampling ratio with one to three ballot rounds of rois"""
    C, H, W = chw
    for R in ((1, 20) if C > 1000 else (1, 64, 65, 130)):
        _case(dev, C, H, W, P, sr, R, "nhwc", "gather", seed=C + 10 * H + 100 * P + sr + R)


@pytest.mark.parametrize("P", [9, 14])
@pytest.mark.parametrize("chw", [(8, 12, 20), (260, 128, 5)], ids=lambda m_: "c%d-%dx%d" % m_)
def test_bins_kernel_vs_oracle(dev, chw, P):
    """NHWC with P > 8 on a map of at most 128 x 128: one workgroup per (roi, bin), one atomic per touched cell"""
    C, H, W = chw
    for sr in (0, 2):
        _case(dev, C, H, W, P, sr, 20 if C > 100 else 65, "nhwc", "bins", seed=C + H + P + sr)


@pytest.mark.parametrize("C,H,W,P", [(8, 129, 4, 9), (6, 10, 12, 7), (8, 5, 129, 9)], ids=["h129", "c6", "w129"])
def test_nhwc_scatter_vs_oracle(dev, C, H, W, P):
    """NHWC where neither the gather nor the bins kernel can run: a map side above 128 with P > 8, C % 4 != 0"""
    for sr in (0, 2):
        _case(dev, C, H, W, P, sr, 65, "nhwc", "scatter_nhwc", seed=C + H + W + sr)


def test_nchw_scatter_vs_oracle(dev):
    for sr in (0, 2):
        _case(dev, 6, 10, 12, 7, sr, 65, "nchw", "scatter_nchw", seed=77 + sr)


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_no_rois_is_a_zero_fill(dev, layout):
    """R = 0: all +0.0 in both layouts, recorded as the zero fill alone"""
    ops = _ops()
    gin, form = _backward(ops, dev, None, None, 0, 8, 5, 7, 7, 7, 2, ops.NCHW if layout == "nchw" else ops.NHWC)
    assert form == "memset" and not gin.view(torch.int32).any()


@pytest.mark.parametrize("C,H,W,P,layout,expect", [(260, 7, 5, 7, "nhwc", "gather"), (8, 12, 20, 9, "nhwc", "bins"),
                                                   (8, 129, 4, 9, "nhwc", "scatter_nhwc"), (6, 10, 12, 7, "nhwc", "scatter_nhwc"),
                                                   (6, 10, 12, 7, "nchw", "scatter_nchw")],
                         ids=["gather", "bins", "scatter_nhwc", "scatter_nhwc_c6", "scatter_nchw"])
def test_backward_is_the_adjoint_of_the_forward(dev, C, H, W, P, layout, expect):
    """<g, fwd(x)> == <bwd(g), x> in float64 to 1e-5 relative, with positive g and x (no cancellation in either product):
    independent of the oracle's backward (the forward is bit-exact against the oracle's forward elsewhere)"""
    for sr in (0, 2):
        _case(dev, C, H, W, P, sr, 65, layout, expect, seed=1000 + C + H + sr, adjoint=True)
