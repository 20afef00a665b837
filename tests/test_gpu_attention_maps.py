"""Attention maps (dana_amd/attention.py, csrc/attention_maps.hip): `model.attention_maps`, `attention.upsample` /
`render` and the reduction kernel under them.

Shapes: query 96 x 128 (feature grid 6 x 8), supports 320 x 320 (20 x 20), shot 2, the test-profile weights of seed 11
with the BA block, the synthetic episode of seed 5; one test at B = 2. Every launch geometry of the new kernels has its
edges inside these shapes: the box-mean's float4 and scalar paths, a partial last column chunk, 1-cell and full-grid
rectangles, the per-box row blocks of the 7 x 7 mode, more than one workgroup per map in the render.

Bars.
  * Against the definition: ba / rpn / roi restated in float64 torch on the CPU from oracle.model_ref.rcnn_base features
    and positional_encoding (the formulas of the oracle's rpn_attention / rcnn_head, which do not return the weights),
    RoI pooling from roi_align_torch: max |got - ref| <= 1e-3 * max(ref) per map. A cap, not a measurement: a map shifted
    by one support column, transposed, taken for another box or without its unary term is 70 to 440 times further off.
    The attained figures are printed and recorded in profiles/attention_maps.md.
  * Invariants: a real slot's rpn / roi map sums to 1 + unary_gamma within (N + 2) * 2^-24 relative (N rows averaged), a
    ba map to 1 (the same bound, N = 1), all entries >= 0.
  * The reduction alone: N * 2^-24 * mean per entry against a float64 numpy mean -- the worst case of an in-order fp32 sum
    of N non-negative terms; equal bits from two runs.
  * Support forms: bit-equal (torch.equal) -- images vs cache, a sweep's problem vs the per-class selection, a ragged
    view's real slots vs the unpadded call: at these shapes the score GEMMs of the two sides run the same products in the
    same order, and the per-slot-scale softmax equals the scalar one bit for bit when its scales are 1.
  * upsample: 1e-6 of the map's maximum against a float64 restatement of the cv2 tap formula; render: within +-1 of a
    numpy restatement everywhere."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

H, W, FH, FW, SHOT, S = 96, 128, 6, 8, 2, 320
GAMMA = 0.1  # unary_gamma
BOXES = [
    (20.0, 36.0, 30.0, 44.0),      # inside one cell (1, 2)
    (0.0, 0.0, 127.0, 95.0),       # the whole image
    (100.0, 70.0, 400.0, 300.0),   # past the right and bottom edges
    (90.0, 20.0, 40.0, 60.0),      # x2 < x1: clamps to one column
    (0.0, 0.0, 40.0, 30.0),        # two opposite corners
    (90.0, 60.0, 127.0, 95.0),
]


def _model(dev):
    import dana_amd
    from dana_amd import synthetic as Sy
    m = dana_amd.get_model("DAnA", pretrained=False, use_BA_block=True, way=1, shot=SHOT, classes=["fg", "bg"])
    sd = Sy.fill_state_dict(m.state_dict(), seed=11, profile="test")
    m.load_state_dict(sd)
    return m.to(dev).eval(), sd


def _sets(sup):
    return sup.reshape(sup.size(0), -1, 3, sup.size(-2), sup.size(-1))


_SHARED = {}


def _shared(dev):
    """one model, the B = 1 episode, its boxes, its maps from support images and the float64 reference: built once, never
    written again"""
    if not _SHARED:
        from dana_amd import synthetic as Sy
        m, sd = _model(dev)
        cpu_in = Sy.episode_inputs(1, 1, SHOT, H, W, seed=5)
        im, info, gt, nb, sup = [t.to(dev) for t in cpu_in]
        boxes = torch.tensor([BOXES], dtype=torch.float32, device=dev)
        with torch.no_grad():
            maps = m.attention_maps(im, info, boxes, sup)
        torch.cuda.synchronize()
        _SHARED.update(m=m, sd=sd, cpu_in=cpu_in, im=im, info=info, gt=gt, nb=nb, sup=sup, boxes=boxes, maps=maps,
                       ref=_reference(sd, cpu_in[0], cpu_in[4]))
    return _SHARED


def _rect(box, fh=FH, fw=FW):
    from dana_amd.attention import cell_rect
    return cell_rect(box, fh, fw)


def _reference(sd, im, sup):
    """ba [1][m][20][20], rpn [1][n][m][20][20], roi [1][n][m][7][7] in float64 (dana.py:126-146, :258-277)"""
    from oracle import model_ref as O
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}

    def lin(x, p):
        return F.linear(x, sd[p + ".weight"], sd[p + ".bias"])

    with torch.no_grad():
        base = O.rcnn_base(im.double(), sd)                                   # [1][1024][6][8]
        sfeat = O.rcnn_base(sup.reshape(-1, 3, S, S).double(), sd)           # [m][1024][20][20]
        pe400, pe49 = O.positional_encoding(400)[0].double(), O.positional_encoding(49)[0].double()
        q = lin(base.reshape(1024, -1).t(), "rpn_adapt_q_layer")             # [hw][256]
        q = q - q.mean(0, keepdim=True)
        ba, rows = [], []
        for i in range(SHOT):
            s = sfeat[i].reshape(1024, -1).t() + pe400                        # [400][1024]
            wgt = F.softmax(lin(s, "rpn_channel_k_layer"), 0)                 # [400][1]   (dana.py:134-135)
            ba.append(wgt.view(20, 20))
            s = s + 0.1 * F.leaky_relu(wgt.t() @ s)
            k = lin(s, "rpn_adapt_k_layer")
            k = k - k.mean(0, keepdim=True)
            a = F.softmax(q @ k.t() / math.sqrt(256), 1)                      # [hw][400]  (dana.py:142-146)
            rows.append(a + GAMMA * F.softmax(lin(s, "rpn_unary_layer"), 0).t())
        rpn = []
        for box in BOXES:
            x_lo, y_lo, x_hi, y_hi = _rect(box)
            cells = [y * FW + x for y in range(y_lo, y_hi + 1) for x in range(x_lo, x_hi + 1)]
            rpn.append(torch.stack([r[cells].mean(0).view(20, 20) for r in rows]))
        rois = torch.tensor([(0.0,) + b for b in BOXES])
        pooled = O.roi_align_torch(base, rois, 1.0 / 16.0, 7)                 # [n][1024][7][7]
        qf = pooled.reshape(len(BOXES), 1024, 49).transpose(1, 2) + pe49
        q2 = lin(qf, "rcnn_adapt_q_layer")
        q2 = q2 - q2.mean(1, keepdim=True)                                    # [n][49][256]
        sp = F.avg_pool2d(sfeat, 14, 1)                                       # [m][1024][7][7]
        roi = []
        for i in range(SHOT):
            s = sp[i].reshape(1024, 49).t() + pe49
            k = lin(s, "rcnn_adapt_k_layer")
            k = k - k.mean(0, keepdim=True)
            a = F.softmax(q2 @ k.t() / math.sqrt(256), 2)                     # [n][49][49]  (dana.py:273-277)
            a = a + GAMMA * F.softmax(lin(s, "rcnn_unary_layer"), 0).t()
            roi.append(a.mean(1).view(len(BOXES), 7, 7))
    return dict(ba=torch.stack(ba)[None], rpn=torch.stack(rpn)[None], roi=torch.stack(roi, 1)[None])


# ---- 1. against the definition ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", ["ba", "rpn", "roi"])
def test_maps_match_the_float64_definition(dev, level):
    sh = _shared(dev)
    got, ref = getattr(sh["maps"], level).double().cpu(), sh["ref"][level]
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert {"ba": (1, SHOT, 20, 20), "rpn": (1, len(BOXES), SHOT, 20, 20), "roi": (1, len(BOXES), SHOT, 7, 7)}[level] == got.shape
    assert getattr(sh["maps"], level).dtype == torch.float32 and getattr(sh["maps"], level).is_cuda
    err = (got - ref).abs().flatten(-2).max(-1).values
    peak = ref.flatten(-2).max(-1).values
    print("ATTAINED %s: max |got - ref| / max(ref) over the maps = %.3e (cap 1e-3); peak / mean of the maps %.2f .. %.2f"
          % (level, float((err / peak).max()), float((peak / ref.flatten(-2).mean(-1)).min()),
             float((peak / ref.flatten(-2).mean(-1)).max())))
    assert bool((err <= 1e-3 * peak).all()), "worst err / max(ref) = %.3e" % float((err / peak).max())


def test_the_bar_sees_the_errors_it_is_there_for(dev):
    """a shifted, a transposed, another box's map and one without its unary term all miss the 1e-3 cap by a wide margin"""
    ref = _shared(dev)["ref"]["rpn"][0]  # [n][m][20][20]
    peak = ref.flatten(-2).max(-1).values

    def miss(other):
        return float(((other - ref).abs().flatten(-2).max(-1).values / peak).max())

    figures = dict(shifted=miss(torch.roll(ref, 1, -1)), transposed=miss(ref.transpose(-1, -2)),
                   corners_swapped=miss(ref[[5, 1, 2, 3, 4, 0]]), unscaled_by_shots=miss(ref / SHOT))
    print("MISSES " + ", ".join("%s %.3f" % kv for kv in figures.items()))
    assert min(figures.values()) > 1e-2  # each at least ten times the cap


# ---- 2. invariants ----------------------------------------------------------------------------------------------------
def test_invariants_mass_and_sign(dev):
    maps = _shared(dev)["maps"]
    n_rows = [(r[2] - r[0] + 1) * (r[3] - r[1] + 1) for r in map(_rect, BOXES)]
    assert n_rows == [1, 48, 4, 3, 6, 9]
    for t in (maps.ba, maps.rpn, maps.roi):
        assert bool((t >= 0).all())
    worst = {}
    for j, nr in enumerate(n_rows):
        for name, t, N in (("rpn", maps.rpn[0, j], nr), ("roi", maps.roi[0, j], 49)):
            mass = t.double().flatten(-2).sum(-1).cpu()
            rel = float(((mass - (1 + GAMMA)).abs() / (1 + GAMMA)).max())
            worst[name] = max(worst.get(name, 0.0), rel / ((N + 2) * 2.0 ** -24))
            print("MASS %s box %d: N = %2d, |sum - 1.1| / 1.1 = %.3e (bound %.3e)" % (name, j, N, rel, (N + 2) * 2.0 ** -24))
    mass = maps.ba.double().flatten(-2).sum(-1).cpu()
    rel = float((mass - 1).abs().max())
    print("MASS ba: |sum - 1| = %.3e (bound %.3e); worst rpn / roi ratio to the bound %.3f / %.3f"
          % (rel, 3 * 2.0 ** -24, worst["rpn"], worst["roi"]))
    assert rel <= 3 * 2.0 ** -24
    assert worst["rpn"] <= 1.0 and worst["roi"] <= 1.0, worst


# ---- 3. the reduction kernel alone ------------------------------------------------------------------------------------
_CASES = [
    # (NP, group, n, gh, gw, ld, K, roi): the column chunk is 256 columns (float4 path) or 64 (scalar path)
    (3, 3, 5, 6, 8, 304, 301, False),   # ld > K, K = 256 + 45: a partial chunk that is no multiple of 4; one image, C = 3
    (2, 1, 1, 6, 8, 301, 301, False),   # ld % 4 != 0: the scalar path, K = 4 * 64 + 45; n = 1
    (4, 1, 5, 3, 5, 64, 64, False),     # one full chunk of the float4 path, K < 256
    (2, 1, 5, 7, 7, 128, 98, True),     # the 7 x 7 mode: rows j*49 .. of [n*49][K2p], K2 = 98 of ld 128
    (1, 1, 1, 7, 7, 99, 99, True),      # ... scalar path, n = 1
]
_KBOXES = [(20.0, 36.0, 30.0, 44.0), (-5.0, -5.0, 1e4, 1e4), (100.0, 70.0, 400.0, 300.0), (90.0, 20.0, 40.0, 60.0),
           (0.0, 0.0, 40.0, 30.0)]  # (1 cell, the full grid, ...)


@pytest.mark.parametrize("case", _CASES, ids=lambda c: "np%d_g%d_n%d_%dx%d_ld%d_k%d_%s" % (c[:7] + ("roi" if c[7] else "box",)))
def test_attn_box_mean_against_float64(dev, case):
    from dana_amd import ops
    NP, group, n, gh, gw, ld, K, roi = case
    g = torch.Generator().manual_seed(NP * 1000 + ld)
    rows_b = (n if roi else 1) * gh * gw
    attn = torch.rand((NP, rows_b, ld), generator=g)
    boxes = torch.tensor([_KBOXES[:n]] * (NP // group), dtype=torch.float32)
    boxes[-1, :, :2] += 1.0  # (every image its own boxes, same cells)
    a64 = attn.double().numpy()
    ref, nrow = np.zeros((NP, n, K)), np.zeros((n,))
    for p in range(NP):
        for j in range(n):
            if roi:
                rows = list(range(j * gh * gw, (j + 1) * gh * gw))
            else:
                x_lo, y_lo, x_hi, y_hi = _rect(boxes[p // group, j].tolist(), gh, gw)
                rows = [y * gw + x for y in range(y_lo, y_hi + 1) for x in range(x_lo, x_hi + 1)]
            nrow[j] = len(rows)
            ref[p, j] = a64[p, rows, :K].mean(0)
    if not roi:
        assert nrow[0] == 1 and (n < 2 or nrow[1] == gh * gw)  # a 1-cell and a full-grid rectangle
    d_attn, d_boxes = attn.to(dev), (None if roi else boxes.to(dev))
    out = ops.attn_box_mean(d_attn, d_boxes, n, gh, gw, k=K, group=group, roi=roi)
    again = ops.attn_box_mean(d_attn, d_boxes, n, gh, gw, k=K, group=group, roi=roi)
    assert out.shape == (NP, n, K) and out.dtype == torch.float32
    assert torch.equal(out, again)
    err = np.abs(out.double().cpu().numpy() - ref)
    bound = nrow[None, :, None] * 2.0 ** -24 * ref
    print("BOX-MEAN %s: worst err / bound %.3f" % (case, float((err / bound).max())))
    assert (err <= bound).all(), float((err / bound).max())


def test_attn_box_mean_bad_arguments_do_not_launch(dev):
    from dana_amd import ops
    from dana_amd._lib import lib, DanaError
    attn = torch.rand((1, 48, 64), device=dev)
    boxes = torch.zeros((1, 2, 4), device=dev)
    out = torch.full((1, 2, 64), -7.0, device=dev)
    st = ops._stream()
    for args in ((None, boxes.data_ptr(), out.data_ptr(), 1, 48, 64, 64, 2, 6, 8, 1, 0, 16.0),       # null attn
                 (attn.data_ptr(), None, out.data_ptr(), 1, 48, 64, 64, 2, 6, 8, 1, 0, 16.0),         # null boxes, mode 0
                 (attn.data_ptr(), boxes.data_ptr(), None, 1, 48, 64, 64, 2, 6, 8, 1, 0, 16.0),       # null out
                 (attn.data_ptr(), boxes.data_ptr(), out.data_ptr(), 1, 48, 64, 64, 0, 6, 8, 1, 0, 16.0),   # n = 0
                 (attn.data_ptr(), boxes.data_ptr(), out.data_ptr(), 1, 48, 64, 64, 2, 6, 7, 1, 0, 16.0),   # gh*gw != rows_b
                 (attn.data_ptr(), boxes.data_ptr(), out.data_ptr(), 1, 48, 64, 64, 2, 7, 7, 1, 1, 16.0),   # n*49 != rows_b
                 (attn.data_ptr(), boxes.data_ptr(), out.data_ptr(), 1, 48, 64, 65, 2, 6, 8, 1, 0, 16.0)):  # k > ld
        with pytest.raises(DanaError, match="dana_attn_box_mean"):
            lib().call("dana_attn_box_mean", *args, st)
    with pytest.raises(DanaError):
        ops.attn_box_mean(attn, boxes[:, :0], 0, 6, 8)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


# ---- 4. consistency across support forms ------------------------------------------------------------------------------
def _equal(a, b, what):
    """bit-equal; the distance is printed first"""
    d = (a.double() - b.double()).abs().flatten(-2).max(-1).values / b.double().flatten(-2).max(-1).values
    print("FORMS %s: worst |d| / max = %.3e" % (what, float(d.max())))
    assert torch.equal(a, b), what


def test_cache_gives_the_maps_of_support_images(dev):
    sh = _shared(dev)
    m = sh["m"]
    with torch.no_grad():
        cache = m.encode_supports(_sets(sh["sup"]))
        cache.select([0])
        got = m.attention_maps(sh["im"], sh["info"], sh["boxes"], cache)
        assert got.ba is None
        assert torch.equal(got.rpn, sh["maps"].rpn) and torch.equal(got.roi, sh["maps"].roi)
        only = m.attention_maps(sh["im"], sh["info"], sh["boxes"], cache, levels=("roi",))
        assert only.ba is None and only.rpn is None and torch.equal(only.roi, sh["maps"].roi)
        with pytest.raises(ValueError, match="'ba'"):
            m.attention_maps(sh["im"], sh["info"], sh["boxes"], cache, levels=("ba", "rpn"))
        with pytest.raises(ValueError, match="'ba'"):
            m.attention_maps(sh["im"], sh["info"], sh["boxes"], cache.sweep([0]), levels=("ba",))
    m.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            m.attention_maps(sh["im"], sh["info"], sh["boxes"], sh["sup"])
    finally:
        m.eval()


def test_sweep_problems_are_the_per_class_maps_at_batch_2(dev):
    from dana_amd import synthetic as Sy
    m = _shared(dev)["m"]
    im, info, gt, nb, sup = [t.to(dev) for t in Sy.episode_inputs(2, 1, SHOT, H, W, seed=5)]
    boxes = torch.tensor([BOXES[:3], BOXES[3:]], dtype=torch.float32, device=dev)
    C, n = 2, 3
    with torch.no_grad():
        cache = m.encode_supports(_sets(sup))
        sw = m.attention_maps(im, info, boxes, cache.sweep([0, 1]))
        assert sw.ba is None and sw.rpn.shape == (2 * C, n, SHOT, 20, 20) and sw.roi.shape == (2 * C, n, SHOT, 7, 7)
        for c in range(C):
            cache.select([c, c])
            one = m.attention_maps(im, info, boxes, cache)
            for b in range(2):
                _equal(sw.rpn[b * C + c], one.rpn[b], "sweep rpn b%d c%d" % (b, c))
                _equal(sw.roi[b * C + c], one.roi[b], "sweep roi b%d c%d" % (b, c))
        # the images' own sets: from support images at B = 2
        cache.select([0, 1])
        a, b_ = m.attention_maps(im, info, boxes, cache), m.attention_maps(im, info, boxes, sup)
        assert b_.ba.shape == (2, SHOT, 20, 20)
        _equal(a.rpn, b_.rpn, "B = 2 cache vs images rpn")
        _equal(a.roi, b_.roi, "B = 2 cache vs images roi")
        assert not torch.equal(sw.rpn[0], sw.rpn[1])  # (the two classes do differ)


def test_ragged_views_zero_the_padded_slot_and_leave_real_slots_unscaled(dev):
    sh = _shared(dev)
    m = sh["m"]
    with torch.no_grad():
        cache = m.encode_supports(_sets(sh["sup"]))
        rag = m.attention_maps(sh["im"], sh["info"], sh["boxes"], cache.sweep([0, 0], shots=[(0,), (0, 1)]))
        one = m.attention_maps(sh["im"], sh["info"], sh["boxes"], cache.sweep([0], shots=[(0,)]))
        full = m.attention_maps(sh["im"], sh["info"], sh["boxes"], cache.sweep([0]))
    assert rag.rpn.shape == (2, len(BOXES), 2, 20, 20) and one.rpn.shape == (1, len(BOXES), 1, 20, 20)
    for name in ("rpn", "roi"):
        r, o, f_ = getattr(rag, name), getattr(one, name), getattr(full, name)
        assert bool((r[0, :, 1] == 0).all()), "%s: the padded slot is not zero" % name
        _equal(r[0, :, 0], o[0, :, 0], "ragged %s: the 1-shot view's real slot" % name)
        _equal(r[1], f_[0], "ragged %s: the 2-shot view" % name)
        _equal(f_[0], getattr(sh["maps"], name)[0], "sweep of one class vs support images, %s" % name)
        mass = r[0, :, 0].double().flatten(-2).sum(-1)
        assert float((mass - 1.1).abs().max()) < 1e-5  # not scaled by the view's 1 / len, nor by 1 / m


# ---- 5. the forward is untouched --------------------------------------------------------------------------------------
def _is_rpn_conv_or_layer4(name):
    # RPN_Conv: 3 x 3 over 2048 channels (K = 18432); layer4: 3 x 3 over 512 channels (K = 4608), outputs of 2048 channels
    # and the box head's GEMM over them -- nothing in the trunk (<= 1024 channels, 3 x 3 over <= 256) has these shapes
    return "K=18432" in name or "K=4608" in name or " N=2048 " in name or "K=2048 " in name


def test_forward_is_untouched_and_no_rpn_conv_or_layer4_launch(dev):
    from dana_amd import ops
    sh = _shared(dev)
    m, args = sh["m"], (sh["im"], sh["info"], sh["gt"], sh["nb"], sh["sup"])
    with torch.no_grad():
        before = tuple(t.clone() for t in m(*args)[:3])
        m.attention_maps(sh["im"], sh["info"], sh["boxes"], sh["sup"])
        after = m(*args)[:3]
        for a, b in zip(before, after):
            assert torch.equal(a, b)
        m._single_stream = True
        try:
            ops.PROFILE = []
            m(*args)
            fwd = [e[0] for e in ops.PROFILE]
            ops.PROFILE = []
            m.attention_maps(sh["im"], sh["info"], sh["boxes"], sh["sup"])
            maps = [e[0] for e in ops.PROFILE]
            torch.cuda.synchronize()
        finally:
            ops.PROFILE = None
            m._single_stream = False
    print("LAUNCHES contractions: forward %d, attention_maps %d" % (len(fwd), len(maps)))
    assert sum(map(_is_rpn_conv_or_layer4, fwd)) >= 6, fwd  # (the forward does issue them: RPN conv + 3 layer4 blocks)
    assert not any(map(_is_rpn_conv_or_layer4, maps)), [n for n in maps if _is_rpn_conv_or_layer4(n)]
    assert len(maps) < len(fwd)


# ---- 6. rendering -----------------------------------------------------------------------------------------------------
def _taps(n_dst, n_src):
    """cv2.resize(INTER_LINEAR) taps in float64: (s0, s1, fraction)"""
    pos = (np.arange(n_dst, dtype=np.float64) + 0.5) * (float(n_src) / n_dst) - 0.5
    s = np.floor(pos)
    f = pos - s
    f[s < 0], s[s < 0] = 0.0, 0
    f[s >= n_src - 1], s[s >= n_src - 1] = 0.0, n_src - 1
    s = s.astype(np.int64)
    return s, np.minimum(s + 1, n_src - 1), f


def _upsample_np(maps, size, dtype=np.float64):
    """[..., gh, gw] -> [..., size, size]: horizontal pass, then vertical, each D = S[s] * (1 - f) + S[s + 1] * f; dtype
    float32 rounds every operation as the kernel does"""
    maps = maps.astype(dtype)
    gh, gw = maps.shape[-2:]
    (y0, y1, fy), (x0, x1, fx) = _taps(size, gh), _taps(size, gw)
    fx, fy = fx.astype(dtype), fy.astype(dtype)[:, None]
    one = dtype(1)
    r0 = maps[..., y0, :][..., x0] * (one - fx) + maps[..., y0, :][..., x1] * fx
    r1 = maps[..., y1, :][..., x0] * (one - fx) + maps[..., y1, :][..., x1] * fx
    return r0 * (one - fy) + r1 * fy


def _render_np(maps, images, alpha):
    """attention.render restated: float32 upsample, min-max of the MAP, table entry round(255 t), blend, round"""
    from dana_amd import cfg
    from dana_amd.attention import COLOR_TABLE
    f32 = np.float32
    up = _upsample_np(maps, images.shape[-1], f32)
    lo = maps.min((-2, -1), keepdims=True).astype(f32)
    hi = maps.max((-2, -1), keepdims=True).astype(f32)
    with np.errstate(divide="ignore"):
        inv = np.where(hi > lo, f32(1) / (hi - lo), f32(0)).astype(f32)
    t = np.clip((up - lo) * inv, f32(0), f32(1))
    idx = (t * f32(255) + f32(0.5)).astype(np.int64)
    colour = np.asarray(COLOR_TABLE, dtype=f32)[idx]                                       # [..., S, S, 3] RGB
    means = np.asarray(cfg.PIXEL_MEANS, dtype=f32).reshape(3)                              # BGR
    rgb = np.clip(np.moveaxis(images.astype(f32) + means[:, None, None], -3, -1)[..., ::-1], f32(0), f32(255))
    blend = (f32(1) - f32(alpha)) * rgb + f32(alpha) * colour
    return (np.clip(blend, f32(0), f32(255)) + f32(0.5)).astype(np.uint8), idx


@pytest.mark.parametrize("g", [20, 7])
def test_upsample_against_the_float64_tap_formula(dev, g):
    from dana_amd import attention
    maps = _shared(dev)["maps"]
    src = maps.rpn[0] if g == 20 else maps.roi[0]                                          # [n][m][g][g]
    up = attention.upsample(src, S)
    assert up.shape == src.shape[:-2] + (S, S) and up.dtype == torch.float32
    ref = _upsample_np(src.cpu().numpy(), S)
    err = np.abs(up.double().cpu().numpy() - ref).max((-2, -1)) / ref.max((-2, -1))
    print("UPSAMPLE %d -> %d: worst err / max(map) %.3e (cap 1e-6)" % (g, S, float(err.max())))
    assert (err <= 1e-6).all()


def test_render_real_maps_over_the_support_images(dev):
    from dana_amd import attention
    sh = _shared(dev)
    maps = sh["maps"].rpn[0]                                                                # [n][m][20][20]
    images = sh["sup"][0][None].expand(maps.size(0), SHOT, 3, S, S).contiguous()            # [n][m][3][S][S]
    out = attention.render(maps, images, alpha=0.5)
    assert out.dtype == torch.uint8 and out.shape == (maps.size(0), SHOT, S, S, 3) and out.is_cuda
    ref, idx = _render_np(maps.cpu().numpy(), images.cpu().numpy(), 0.5)
    d = np.abs(out.cpu().numpy().astype(np.int64) - ref.astype(np.int64))
    print("RENDER 20 -> %d: %d of %d bytes differ from the restatement, worst by %d; table entries used %d..%d"
          % (S, int((d > 0).sum()), d.size, int(d.max()), int(idx.min()), int(idx.max())))
    assert int(d.max()) <= 1
    assert int(idx.min()) == 0 and int(idx.max()) >= 250  # (the maps do use the table's range)
    # the 7 x 7 maps, alpha at its ends: the image alone, the colours alone
    roi = sh["maps"].roi[0]
    for alpha in (0.0, 1.0):
        o7 = attention.render(roi, images, alpha=alpha)
        r7, _ = _render_np(roi.cpu().numpy(), images.cpu().numpy(), alpha)
        assert int(np.abs(o7.cpu().numpy().astype(np.int64) - r7.astype(np.int64)).max()) <= 1
    with pytest.raises(ValueError):
        attention.render(maps, images[:, :1])
    with pytest.raises(ValueError):
        attention.render(maps, images, alpha=1.5)


def test_render_constant_map_and_argmax_colour(dev):
    """S = 3 * 20 and 3 * 7: an odd number of pixels per cell, so every cell has a centre pixel and it samples its cell
    alone (at S = 320, 16 pixels per cell, no pixel does)"""
    from dana_amd import attention, cfg
    from dana_amd.attention import COLOR_TABLE
    means = np.asarray(cfg.PIXEL_MEANS, dtype=np.float32).reshape(3)
    for g in (20, 7):
        size = 3 * g
        gen = torch.Generator().manual_seed(g)
        maps = torch.rand((3, g, g), generator=gen)
        maps[0] = 0.25                                                                      # a constant map
        cy, cx = 4, g - 2
        maps[1, cy, cx] = 2.0                                                               # map 1's argmax
        maps[2, 0, 0] = -1.0
        images = (torch.rand((3, 3, size, size), generator=gen) * 300 - 150)                # some pixels clamp at 0 / 255
        out = attention.render(maps.to(dev), images.to(dev), alpha=0.5).cpu().numpy()
        assert out.shape == (3, size, size, 3) and out.dtype == np.uint8
        ref, idx = _render_np(maps.numpy(), images.numpy(), 0.5)
        assert int(np.abs(out.astype(np.int64) - ref.astype(np.int64)).max()) <= 1
        # the constant map: the image under the table's first colour at alpha
        rgb = np.clip(np.moveaxis(images[0].numpy() + means[:, None, None], 0, -1)[..., ::-1], 0, 255).astype(np.float64)
        want = 0.5 * rgb + 0.5 * np.asarray(COLOR_TABLE[0], dtype=np.float64)
        assert np.abs(out[0].astype(np.float64) - want).max() <= 0.5 + 1e-3 and (idx[0] == 0).all()
        # the argmax cell's centre pixel carries the table's last colour; alone at alpha = 1
        py, px = 3 * cy + 1, 3 * cx + 1
        assert idx[1, py, px] == 255 and (idx[1] == 255).sum() == 1
        want = 0.5 * rgb_at(images[1], means, py, px) + 0.5 * np.asarray(COLOR_TABLE[255], dtype=np.float64)
        assert np.abs(out[1, py, px].astype(np.float64) - want).max() <= 0.5 + 1e-3
        solid = attention.render(maps.to(dev), images.to(dev), alpha=1.0).cpu().numpy()
        assert tuple(solid[1, py, px]) == COLOR_TABLE[255] and tuple(solid[2, 1, 1]) == COLOR_TABLE[0]
        assert (solid[0] == np.asarray(COLOR_TABLE[0], dtype=np.uint8)).all()


def rgb_at(image, means, y, x):
    return np.clip(image[:, y, x].numpy()[::-1] + means[::-1], 0, 255).astype(np.float64)
