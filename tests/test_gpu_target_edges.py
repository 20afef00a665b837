"""Target assignment (csrc/targets.hip), the device sampler (csrc/sampling.hip) and the loss kernels at their edges:
the compaction seams of the ordered fg / bg lists, every sampling branch of both target layers, the grid-stride loops of
the RPN losses, the global-memory rank loop and the tie rule of the RCNN loss. References: oracle.model_ref wherever an
IoU threshold decides (labels and picks must be equal), float64 torch written here for losses and gradients, and
tests/sampling_ref.py -- the plain restatement of the Philox sampler -- for the device-RNG picks, which are predicted
exactly. Every input that is meant to reach a branch is checked to reach it on the REFERENCE's numbers first."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sampling_ref as SR

pytestmark = pytest.mark.gpu

A, STRIDE = 12, 16
SEEDS = ((7, 0), ((1 << 40) + 3, (1 << 33) + 5))  # the second pair: a 64-bit value truncated anywhere shows


def _gt(B, n_gt, boxes):
    g = torch.zeros(B, n_gt, 5)
    for b, lst in enumerate(boxes):
        for k, bx in enumerate(lst):
            g[b, k] = torch.tensor(bx, dtype=torch.float32)
    return g


def _ii(h, w, B):
    return torch.tensor([[float(h), float(w), 1.0]] * B)


def _base():
    from dana_amd import targets as T
    from dana_amd.config import cfg
    return torch.from_numpy(T.generate_anchors(scales=np.array(cfg.ANCHOR_SCALES), ratios=np.array(cfg.ANCHOR_RATIOS))).float()


def _big_gt(B, seed):
    """3-4 boxes per image on 1200 x 1200; the LAST image also holds a box equal to the 64 x 64 anchor of cell (71, 50):
    a positive whose flat index lies in the tail that only the grid-stride loops reach"""
    rng = np.random.default_rng(seed)
    boxes = []
    for b in range(B):
        lst = []
        for _ in range(3):
            x1, y1 = rng.uniform(0, 900), rng.uniform(0, 900)
            lst.append((x1, y1, x1 + rng.uniform(60, 290), y1 + rng.uniform(60, 290), 1 + b % 3))
        lst.append((776, 1112, 839, 1175, 2) if b == B - 1 else None)
        boxes.append([x for x in lst if x is not None])
    return _gt(B, 5, boxes)


_GT_9x19 = [[(30, 30, 130, 130, 1), (160, 20, 290, 140, 2), (0, 0, 63, 63, 1)], [(100, 40, 227, 103, 4)]]
# H, W, im_info, gt [, inside anchors, fg / image, bg / image as the oracle reports them without subsampling]
ANCHOR_CASES = {
    # below one 1024-anchor chunk; one box equal to an anchor (IoU exactly 1), given twice
    "8x8": dict(H=8, W=8, im_info=_ii(128, 128, 1), gt=_gt(1, 3, [[(8, 8, 71, 71, 1), (8, 8, 71, 71, 2)]]),
                inside=40, fg=[1], bg=[26]),
    # just under one chunk; identical boxes with classes 1 and 3 (first argmax); the LAST image has no box at all
    "5x17": dict(H=5, W=17, im_info=_ii(80, 272, 3),
                 gt=_gt(3, 4, [[(20, 10, 110, 70, 1), (150, 5, 240, 75, 2)], [(20, 10, 110, 70, 1), (20, 10, 110, 70, 3)], []]),
                 inside=46, fg=[3, 1, 0], bg=[14, 31, 46]),
    # just over one chunk: the second chunk holds 8 anchors
    "2x43": dict(H=2, W=43, im_info=_ii(96, 700, 2),
                 gt=_gt(2, 3, [[(100, 0, 191, 47, 1)], [(300, 8, 420, 70, 1), (10, 0, 60, 40, 2)]]),
                 inside=38, fg=[2, 2], bg=[32, 32]),
    # just under two chunks
    "10x17": dict(H=10, W=17, im_info=_ii(160, 272, 2),
                  gt=_gt(2, 3, [[(20, 10, 110, 70, 1), (150, 40, 240, 130, 2)], [(60, 60, 187, 123, 3)]])),
    # third chunk: the unrolled "in front of my chunk" loop runs once, the last chunk holds 4 anchors
    "9x19": dict(H=9, W=19, im_info=_ii(144, 304, 2), gt=_gt(2, 5, _GT_9x19), inside=249, fg=[5, 2], bg=[173, 186]),
    # image 0's im_info decides "inside" for image 1 as well (anchor_target_layer.py:85-86)
    "9x19 image 0 rules": dict(H=9, W=19, im_info=torch.tensor([[144., 304., 1.], [100., 200., 1.]]), gt=_gt(2, 5, _GT_9x19),
                               inside=249, fg=[5, 2], bg=[173, 186]),
    # B * total = 135 000 > 131 072: rpn_loss_kernel's 512 blocks take a second trip
    "75x75 B2": dict(H=75, W=75, im_info=_ii(1200, 1200, 2), gt=_big_gt(2, 3)),
    # B * total = 540 000 > 524 288: rpn_loss_bwd_kernel's 2048 blocks take a second trip
    "75x75 B8": dict(H=75, W=75, im_info=_ii(1200, 1200, 8), gt=_big_gt(8, 4)),
}
SEAM_CASES = ["8x8", "5x17", "2x43", "10x17", "9x19", "9x19 image 0 rules"]
SUBSAMPLE_CASES = [("5x17", 4), ("9x19", 4), ("8x8", 256), ("9x19 image 0 rules", 256)]
DRAW_SEED = 13

_REF = {}  # oracle results, computed once and shared (read-only) among the tests


def _total(name):
    c = ANCHOR_CASES[name]
    return c["H"] * c["W"] * A


def _anchor_ref(monkeypatch, name, batchsize, seed=None):
    """oracle.model_ref.anchor_target_layer at RPN_BATCHSIZE = batchsize (under np.random.seed(seed)) -> its four outputs
    and the labels mapped back to the (h, w, a) order of the kernels' rows"""
    key = (name, batchsize, seed)
    if key not in _REF:
        from oracle import model_ref as O
        c = ANCHOR_CASES[name]
        B, H, W = c["gt"].shape[0], c["H"], c["W"]
        monkeypatch.setitem(O.CFG["TRAIN"], "RPN_BATCHSIZE", batchsize)
        if seed is not None:
            np.random.seed(seed)
        out = O.anchor_target_layer((H, W), c["gt"], c["im_info"])
        lab = out[0].view(B, A, H, W).permute(0, 2, 3, 1).reshape(B, -1).contiguous()
        _REF[key] = dict(out=out, lab=lab)
    return _REF[key]


def _presample(monkeypatch, name):
    """the oracle's labels before any subsampling ((h, w, a) order), and its fg / bg counts per image"""
    pre = _anchor_ref(monkeypatch, name, 2 * _total(name))["lab"]
    return pre, (pre == 1).sum(1).tolist(), (pre == 0).sum(1).tolist()


def _assign(dev, name, batchsize, device_rng=None):
    from dana_amd import ops
    from dana_amd.config import cfg
    c, tr = ANCHOR_CASES[name], cfg.TRAIN
    return ops.anchor_target_assign(c["gt"].to(dev), c["im_info"].to(dev), _base().to(dev), c["H"], c["W"], STRIDE,
                                    tr.RPN_NEGATIVE_OVERLAP, tr.RPN_POSITIVE_OVERLAP, batchsize, tr.RPN_FG_FRACTION,
                                    device_rng=device_rng)


def _same_outputs(got, ref):
    assert torch.equal(got[0].cpu(), ref[0])                # labels
    assert torch.allclose(got[1].cpu(), ref[1], atol=2e-6)  # targets (logf vs torch.log)
    assert torch.equal(got[2].cpu(), ref[2])                # inside weights
    assert torch.equal(got[3].cpu(), ref[3])                # outside weights: 1 / num_examples of the LAST image


# ---- a. labels and ordered lists at the compaction seams ---------------------------------------------------------------
@pytest.mark.parametrize("name", SEAM_CASES)
def test_anchor_labels_and_ordered_lists_at_the_compaction_seams(dev, monkeypatch, name):
    """anchor_target_{iou,label,lists}_kernel vs the oracle with nothing subsampled: below one 1024-anchor chunk, 4 under
    and 8 over one chunk, 8 under and 4 over two (the first size whose last chunk runs the unrolled front loop)"""
    from dana_amd import ops
    from oracle import model_ref as O
    c, total = ANCHOR_CASES[name], _total(name)
    ref = _anchor_ref(monkeypatch, name, 2 * total)
    pre, nf, nb = _presample(monkeypatch, name)
    B = pre.shape[0]
    assert sum(nf) > 0 and sum(nb) > 0
    if "inside" in c:  # the case is what it was chosen for, on the oracle's own numbers
        allA = O.anchor_grid(O.generate_anchors(scales=O.CFG["ANCHOR_SCALES"], ratios=O.CFG["ANCHOR_RATIOS"]), c["H"], c["W"], STRIDE)
        keep = ((allA[:, 0] >= 0) & (allA[:, 1] >= 0) & (allA[:, 2] < int(c["im_info"][0][1])) &
                (allA[:, 3] < int(c["im_info"][0][0])))
        assert (int(keep.sum()), nf, nb) == (c["inside"], c["fg"], c["bg"])
    h = _assign(dev, name, 2 * total)
    _same_outputs(ops.anchor_target_outputs(h), ref["out"])
    assert h["counts"].cpu().tolist() == [[nf[b], nb[b]] for b in range(B)]
    fl, bl = h["ibuf"][1].cpu().long(), h["ibuf"][2].cpu().long()
    for b in range(B):  # ascending indices of the PRE-subsample labels, derived from the oracle's labels
        assert torch.equal(fl[b, :nf[b]], torch.nonzero(pre[b] == 1).view(-1))
        assert torch.equal(bl[b, :nb[b]], torch.nonzero(pre[b] == 0).view(-1))


@pytest.mark.parametrize("H,W,side", [(1, 1, 16), (2, 2, 32)])
def test_no_anchor_inside_the_image(dev, H, W, side):
    """the smallest anchor is 64 px wide: nothing is inside, every label is -1, both lists are empty, the box loss is 0
    and the classification loss is NaN like F.cross_entropy over an empty selection"""
    from dana_amd import ops
    from dana_amd.config import cfg
    tr = cfg.TRAIN
    gt = _gt(2, 3, [[(2, 2, 12, 12, 1)], [(0, 0, side - 1, side - 1, 2)]]).to(dev)
    h = ops.anchor_target_assign(gt, _ii(side, side, 2).to(dev), _base().to(dev), H, W, STRIDE, tr.RPN_NEGATIVE_OVERLAP,
                                 tr.RPN_POSITIVE_OVERLAP, tr.RPN_BATCHSIZE, tr.RPN_FG_FRACTION)
    assert h["counts"].cpu().tolist() == [[0, 0], [0, 0]]
    lab, tgt, w_in, w_out = [t.cpu() for t in ops.anchor_target_outputs(h)]
    assert torch.all(lab == -1) and not tgt.any() and not w_in.any() and not w_out.any()
    heads = torch.randn(2 * H * W, 6 * A, generator=torch.Generator().manual_seed(1)).to(dev)
    l3 = ops.rpn_losses(heads, 6 * A, h, sigma=3.0).cpu()
    assert torch.isnan(l3[0]) and float(l3[1]) == 0.0 and float(l3[2]) == 0.0
    # the documented departure max(ne, 1): the reference divides by its zero examples (anchor_target_layer.py:156,176),
    # ops.anchor_target_draw returns "max(num_examples, 1)"
    assert h["num_examples"] == 1


def test_more_gt_boxes_than_anchors_is_an_argument_error_and_launches_nothing(dev):
    from dana_amd._lib import DanaError, lib
    B, n_gt, total = 1, 13, 12
    gt = torch.zeros(B, n_gt, 5, device=dev)
    labels = torch.full((B, total), 7.0, device=dev)
    max_ov = torch.full((B, total), 7.0, device=dev)
    ibuf = torch.full((3, B, total), -9, dtype=torch.int32, device=dev)
    counts = torch.full((B, 2), -9, dtype=torch.int32, device=dev)
    with pytest.raises(DanaError, match="more gt boxes than anchors"):
        lib().call("dana_anchor_target_prepare", gt.data_ptr(), _ii(16, 16, 1).to(dev).data_ptr(), _base().to(dev).data_ptr(),
                   B, A, 1, 1, STRIDE, n_gt, 0.3, 0.7, labels.data_ptr(), max_ov.data_ptr(), ibuf[0].data_ptr(),
                   ibuf[1].data_ptr(), ibuf[2].data_ptr(), counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.all(labels == 7) and torch.all(max_ov == 7) and torch.all(ibuf == -9) and torch.all(counts == -9)


# ---- b. subsampling branches, host RNG -----------------------------------------------------------------------------------
def _assert_subsample_branch(name, bs, nf, nb, ref_lab):
    """the branch the case is meant for is really taken, on the oracle's counts"""
    num_fg = bs // 2
    kept_f, kept_b = (ref_lab == 1).sum(1).tolist(), (ref_lab == 0).sum(1).tolist()
    if bs == 4:
        assert any(f > num_fg for f in nf)                              # positives dropped
        assert all(b_ > bs - min(f, num_fg) for f, b_ in zip(nf, nb))   # negatives dropped in every image
        assert (kept_f, kept_b) == {"5x17": ([2, 1, 0], [2, 3, 4]), "9x19": ([2, 2], [2, 2])}[name]
    else:
        assert all(f <= num_fg and b_ <= bs - f for f, b_ in zip(nf, nb))  # fewer negatives than the quota: nothing dropped
        assert (kept_f, kept_b) == (nf, nb)


@pytest.mark.parametrize("name,bs", SUBSAMPLE_CASES)
def test_anchor_subsampling_branches_host_rng_vs_oracle(dev, monkeypatch, name, bs):
    """positives dropped / negatives dropped (RPN_BATCHSIZE 4), nothing dropped (256), image 0's im_info for every image;
    the outside weight is 1 / num_examples of the LAST image (in 5x17 an image without positives). Same np.random stream
    as the oracle, through anchor_target_assign and through the draw buffer the model uses"""
    from dana_amd import ops
    from dana_amd.config import cfg
    c, total, tr = ANCHOR_CASES[name], _total(name), cfg.TRAIN
    pre, nf, nb = _presample(monkeypatch, name)
    B = pre.shape[0]
    ref = _anchor_ref(monkeypatch, name, bs, seed=DRAW_SEED)
    _assert_subsample_branch(name, bs, nf, nb, ref["lab"])
    if name == "9x19 image 0 rules":  # image 1 has labeled anchors that its own 100 x 200 would put outside
        from oracle import model_ref as O
        allA = O.anchor_grid(O.generate_anchors(scales=O.CFG["ANCHOR_SCALES"], ratios=O.CFG["ANCHOR_RATIOS"]), c["H"], c["W"], STRIDE)
        assert bool(((ref["lab"][1] >= 0) & ((allA[:, 2] >= 200) | (allA[:, 3] >= 100))).any())
    np.random.seed(DRAW_SEED)
    h = _assign(dev, name, bs)
    assert torch.equal(h["labels"].cpu(), ref["lab"])
    _same_outputs(ops.anchor_target_outputs(h), ref["out"])
    ne_last = int((ref["lab"][B - 1] >= 0).sum())
    assert h["num_examples"] == ne_last and ne_last > 0
    # the same draws through draw_layout / draw_and_upload / anchor_target_apply_draws (the dana_anchor_target_disable_dev path)
    h2 = ops.anchor_target_prepare(c["gt"].to(dev), c["im_info"].to(dev), _base().to(dev), c["H"], c["W"], STRIDE,
                                   tr.RPN_NEGATIVE_OVERLAP, tr.RPN_POSITIVE_OVERLAP)
    R = 4
    req = dict(anchor_counts=h2["counts"], anchor_stream=ops.cur_stream(), B=B, R=R, fg_per=1, rpn_batchsize=bs,
               num_fg=int(tr.RPN_FG_FRACTION * bs), total=total,
               proposal_counts=torch.tensor([[1, 1]] * B, dtype=torch.int32, device=dev))
    np.random.seed(DRAW_SEED)  # the anchor layer draws first (dana.py:166-185)
    drawn = ops.draw_and_upload(req, dev)
    ops.anchor_target_apply_draws(h2, drawn, ops.draw_layout(B, R, total))
    assert torch.equal(h2["labels"].cpu(), ref["lab"])
    assert float(h2["inv_ne_dev"].cpu()) == float(np.float32(1.0 / ne_last))
    _same_outputs(ops.anchor_target_outputs(h2), ref["out"])


# ---- c. RPN losses and their backward ------------------------------------------------------------------------------------
def _rpn_loss_ref(heads, ref_out, B, H, W):
    """rpn.py:97-115 in float64 from the oracle's labels / targets / weights; heads [B*H*W, >= 6A] float64 leaf"""
    lab, tgt, w_in, w_out = ref_out
    cls = heads[:, :2 * A].view(B, H, W, 2 * A).permute(0, 3, 1, 2)
    bbox = heads[:, 2 * A:6 * A].view(B, H, W, 4 * A).permute(0, 3, 1, 2)
    sc = cls.reshape(B, 2, A * H, W).permute(0, 2, 3, 1).reshape(-1, 2)
    lv = lab.view(-1)
    keep = lv.ne(-1).nonzero().view(-1)
    l_cls = F.cross_entropy(sc[keep], lv[keep].long())
    s2 = 9.0  # sigma 3 (net_utils.py:71-85)
    d = w_in.double() * (bbox - tgt.double())
    ad = d.abs()
    l_box = (w_out.double() * torch.where(ad < 1.0 / s2, d * d * (s2 / 2.0), ad - 0.5 / s2)).sum((1, 2, 3)).mean()
    return l_cls, l_box, keep.numel()


def _check_rpn_losses(dev, name, ref, h, pad):
    from dana_amd import ops
    c = ANCHOR_CASES[name]
    B, H, W = c["gt"].shape[0], c["H"], c["W"]
    nh = 6 * A + pad
    heads = torch.randn(B * H * W, nh, generator=torch.Generator().manual_seed(B * H + pad)) * 0.5
    hd = heads.double().requires_grad_(True)
    l_cls, l_box, n_lab = _rpn_loss_ref(hd, ref["out"], B, H, W)
    (0.7 * l_cls + 1.3 * l_box).backward()
    l_cls, l_box = l_cls.item(), l_box.item()
    hg = heads.to(dev)
    l3 = ops.rpn_losses(hg, nh, h, sigma=3.0)
    out = l3.cpu()
    print("%s pad %d: cls %.9g (ref %.9g)  box %.9g (ref %.9g)  labeled %d" % (name, pad, out[0], l_cls, out[1], l_box, n_lab))
    assert float(out[2]) == n_lab
    assert abs(float(out[0]) - l_cls) <= 1e-5 * max(1.0, abs(l_cls))
    assert abs(float(out[1]) - l_box) <= 1e-5 * max(1.0, abs(l_box))
    g = ops.rpn_loss_backward(hg, nh, h, l3, 0.7, 1.3, sigma=3.0).cpu()
    g2 = ops.rpn_loss_backward(hg, nh, h, l3, sigma=3.0, grad_dev=torch.tensor([0.7, 1.3], device=dev)).cpu()
    for got in (g, g2):  # scalar seeds and device seeds, each against autograd
        err = (got.double() - hd.grad).abs().max().item()
        assert err <= 1e-5 * (hd.grad.abs().max().item() + 1e-12), err  # as test_rpn_loss_backward_vs_autograd
        assert not got[:, 6 * A:].any()  # padding columns beyond 6A stay zero
    return l_box


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("name,bs", SUBSAMPLE_CASES)
def test_rpn_losses_and_backward_on_the_subsampled_handles(dev, monkeypatch, name, bs, pad):
    """rpn_loss_kernel / rpn_loss_bwd_kernel vs float64 autograd with head_row_stride 6A and 6A + 8; 5x17 ends with an
    image without positives whose example count nevertheless weights every image's box loss"""
    ref = _anchor_ref(monkeypatch, name, bs, seed=DRAW_SEED)
    np.random.seed(DRAW_SEED)
    h = _assign(dev, name, bs)
    assert torch.equal(h["labels"].cpu(), ref["lab"])
    if name == "5x17":
        assert int((ref["lab"][2] == 1).sum()) == 0 and int((ref["lab"][:2] == 1).sum()) > 0
    l_box = _check_rpn_losses(dev, name, ref, h, pad)
    assert l_box > 0


@pytest.mark.parametrize("name,cap", [("75x75 B2", 512 * 256), ("75x75 B8", 2048 * 256)])
def test_rpn_losses_grid_stride_loops(dev, monkeypatch, name, cap):
    """more anchors than 512 x 256 (the loss) and than 2048 x 256 (its backward): labeled anchors, a positive among them,
    lie in the tail that only the second trip of the grid-stride loop reaches"""
    bs = 2 * _total(name)  # nothing is subsampled: every inside anchor below 0.3 or above 0.7 is labeled
    ref = _anchor_ref(monkeypatch, name, bs)
    flat = ref["lab"].reshape(-1)
    assert flat.numel() > cap and bool((flat[cap:] == 1).any()) and bool((flat[cap:] == 0).any())
    h = _assign(dev, name, bs)
    assert torch.equal(h["labels"].cpu(), ref["lab"])
    _check_rpn_losses(dev, name, ref, h, 0)


# ---- d. proposal targets: every branch, host RNG ---------------------------------------------------------------------------
_GT3 = _gt(3, 4, [[(40, 30, 160, 150, 3), (200, 60, 300, 200, 1)], [(40, 30, 160, 150, 2)], []])
# identical boxes with classes 3 and 5: the label of a foreground roi is the FIRST maximum's class
_GT1 = _gt(1, 4, [[(40, 30, 160, 150, 3), (40, 30, 160, 150, 5), (200, 60, 300, 200, 1)]])


def _rois(seed, n, gt, near, pad):
    """n rois per image: near[b] of them jittered +-3 px around the image's first box, the rest uniform, the last `pad` zero"""
    rng = np.random.default_rng(seed)
    B = gt.shape[0]
    r = torch.zeros(B, n, 5)
    for b in range(B):
        r[b, :, 0] = b
        xy, wh = rng.uniform(0, 280, (n, 2)), rng.uniform(8, 120, (n, 2))
        r[b, :, 1:3] = torch.from_numpy(xy).float()
        r[b, :, 3:5] = torch.from_numpy(xy + wh).float()
        if near[b]:
            r[b, :near[b], 1:] = gt[b, :1, :4] + torch.from_numpy(rng.uniform(-3, 3, (near[b], 4))).float()
        if pad:
            r[b, n - pad:] = 0
    return r


def _inverted_rois():
    r = _rois(3, 30, _GT1, [4], 0)
    r[0, 10, 1:] = torch.tensor([100., 100., 99., 180.])
    r[0, 11, 1:] = torch.tensor([50., 50., 20., 20.])
    return r


# name -> (rois, gt, R)
PROPOSAL_CASES = {
    "three branches, n_all 64": (_rois(0, 60, _GT3, [20, 60, 0], 0), _GT3, 16),
    "n_all 1024": (_rois(1, 1020, _GT3, [3, 5, 0], 7), _GT3, 128),
    "n_all 1025": (_rois(2, 1021, _GT3, [40, 2, 0], 0), _GT3, 128),
    "inverted rois": (_inverted_rois(), _GT1, 256),
}


def _proposal_ref(monkeypatch, name):
    """oracle.model_ref.proposal_target_layer under np.random.seed(DRAW_SEED), and its fg / bg masks before the draws"""
    if ("prop", name) not in _REF:
        from oracle import model_ref as O
        rois, gt, R = PROPOSAL_CASES[name]
        t = O.CFG["TRAIN"]
        monkeypatch.setitem(t, "BATCH_SIZE", R)
        ga = torch.zeros_like(gt)
        ga[:, :, 1:5] = gt[:, :, :4]
        mo, _ = O.bbox_overlaps_batch(torch.cat([rois, ga], 1), gt).max(2)
        fg, bg = mo >= t["FG_THRESH"], (mo < t["BG_THRESH_HI"]) & (mo >= t["BG_THRESH_LO"])
        np.random.seed(DRAW_SEED)
        out = O.proposal_target_layer(rois, gt)
        _REF[("prop", name)] = dict(out=out, fg=fg, bg=bg, max_ov=mo, fg_per=int(np.round(t["FG_FRACTION"] * R)) or 1)
    return _REF[("prop", name)]


def _proposal_args(dev, rois, gt, R, fg_per):
    from dana_amd.config import cfg
    tr = cfg.TRAIN
    return (rois.to(dev), gt.to(dev), R, fg_per, tr.FG_THRESH, tr.BG_THRESH_HI, tr.BG_THRESH_LO, tr.BBOX_NORMALIZE_MEANS,
            tr.BBOX_NORMALIZE_STDS, tr.BBOX_INSIDE_WEIGHTS, True)


@pytest.mark.parametrize("name", list(PROPOSAL_CASES))
def test_proposal_targets_every_branch_host_rng_vs_oracle(dev, monkeypatch, name):
    """proposal_target_prepare_kernel's lists at 64, exactly 1024 and 1025 candidates, and the three sampling branches
    (both lists; foreground only; background only) in ONE batch, under the oracle's np.random stream"""
    from dana_amd import ops
    from dana_amd.config import cfg
    rois, gt, R = PROPOSAL_CASES[name]
    ref = _proposal_ref(monkeypatch, name)
    fg_per, tr = ref["fg_per"], cfg.TRAIN
    nf, nb = ref["fg"].sum(1).tolist(), ref["bg"].sum(1).tolist()
    pos = (ref["out"][1] > 0).sum(1).tolist()
    classes = set(ref["out"][1].view(-1).tolist())
    want = ref["out"]
    print(name, "n_all", rois.shape[1] + gt.shape[1], "nf", nf, "nb", nb, "fg_per", fg_per, "positive labels", pos)
    if name == "three branches, n_all 64":
        assert rois.shape[1] + gt.shape[1] == 64 and fg_per == 4
        assert nf[0] > fg_per and nb[0] > 0    # permutation branch, positives over the quota
        assert nf[1] > 0 and nb[1] == 0        # foreground only: R picks with replacement from the fg list
        assert nf[2] == 0 and nb[2] > 0        # background only
        assert pos == [4, 16, 0] and {2.0, 3.0} <= classes
    elif name == "n_all 1024":
        assert rois.shape[1] + gt.shape[1] == 1024 and not rois[:, -7:].any()
        assert 0 < nf[0] < fg_per and 0 < nf[1] < fg_per and nf[2] == 0  # fewer positives than the quota: all are taken
        assert pos[:2] == nf[:2]
    elif name == "n_all 1025":
        assert rois.shape[1] + gt.shape[1] == 1025
        assert nf[0] > fg_per and 0 < nf[1] < fg_per and nf[2] == 0
    else:
        n_all = rois.shape[1] + gt.shape[1]
        assert ref["bg"][0, 10] and ref["bg"][0, 11] and ref["max_ov"][0, 10] == 0 and ref["max_ov"][0, 11] == 0
        assert nf[0] > 0 and nf[0] + nb[0] < n_all  # (the padded gt row is neither)
        # the second of the identical boxes is itself a foreground candidate, and it is labeled 3, never 5: first maximum
        assert bool(ref["fg"][0, rois.shape[1] + 1]) and pos[0] == nf[0] and 3.0 in classes and 5.0 not in classes
        inv = want[0][0, :, 3] < want[0][0, :, 1]  # the inverted rois are among the sampled background rows ...
        assert bool(inv.any()) and not want[2][0][inv].any()  # ... and the oracle's targets for them are zeros
    h = ops.proposal_target_prepare(rois.to(dev), gt.to(dev), tr.FG_THRESH, tr.BG_THRESH_HI, tr.BG_THRESH_LO)
    assert h["counts"].cpu().tolist() == [[f, b_] for f, b_ in zip(nf, nb)]
    fl, bl = h["ibuf"][1].cpu().long(), h["ibuf"][2].cpu().long()
    for b in range(rois.shape[0]):
        assert torch.equal(fl[b, :nf[b]], torch.nonzero(ref["fg"][b]).view(-1))
        assert torch.equal(bl[b, :nb[b]], torch.nonzero(ref["bg"][b]).view(-1))
    np.random.seed(DRAW_SEED)
    got = [t.cpu() for t in ops.proposal_target_layer(*_proposal_args(dev, rois, gt, R, fg_per))]
    assert all(bool(torch.isfinite(t).all()) for t in got)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.allclose(got[2], want[2], atol=2e-6)
    assert torch.equal(got[3], want[3]) and torch.equal(got[4], want[4])
    if name == "inverted rois":  # background rows whose raw regression target is inf / nan come out as the oracle's zeros
        assert not got[2][0][inv].any()


def test_proposal_targets_when_neither_list_has_an_entry(dev):
    """all-zero rois and gt: the host path refuses like the reference (proposal_target_layer_cascade.py:186-187); the
    device-RNG path cannot raise and documents its departure in proposal_target_gather_kernel: "(clamped: a pick into an
    EMPTY list -- fg and bg both empty, which the reference refuses with a ValueError ... -- must not turn an uninitialised
    list entry into a wild read)". Its labels, targets and weights are 0; which roi it returns is unspecified"""
    from dana_amd import ops
    from oracle import model_ref as O
    rois, gt = torch.zeros(1, 30, 5), torch.zeros(1, 2, 5)
    with pytest.raises(ValueError, match="this should not happen"):
        O.proposal_target_layer(rois, gt)
    with pytest.raises(ValueError, match="this should not happen"):
        ops.proposal_target_layer(*_proposal_args(dev, rois, gt, 8, 2))
    got = [t.cpu() for t in ops.proposal_target_layer(*_proposal_args(dev, rois, gt, 8, 2), device_rng=(7, 0))]
    assert all(bool(torch.isfinite(t).all()) for t in got)
    assert not got[1].any() and not got[2].any() and not got[3].any() and not got[4].any()


# ---- e. the device sampler, exactly ----------------------------------------------------------------------------------------
SAMPLER_COUNTS = [(0, 0), (0, 1), (1, 0), (1, 1), (5, 0), (0, 7), (3, 40), (32, 40), (33, 1), (200, 1800), (2048, 0)]


def _device_picks(dev, counts, n_cand, R, fg_per, seed, offset, counter=None):
    from dana_amd._lib import lib
    B = len(counts)
    cnt = torch.tensor(counts, dtype=torch.int32, device=dev)
    picks = torch.full((B, R), -1, dtype=torch.int32, device=dev)
    taken = torch.full((B,), -1, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    if counter is None:
        lib().call("dana_proposal_target_sample", cnt.data_ptr(), B, n_cand, R, fg_per, seed, offset, picks.data_ptr(),
                   taken.data_ptr(), st)
    else:
        ctr = torch.tensor([counter], dtype=torch.int64, device=dev)
        lib().call("dana_proposal_target_sample_ctr", cnt.data_ptr(), B, n_cand, R, fg_per, seed, offset, ctr.data_ptr(),
                   picks.data_ptr(), taken.data_ptr(), st)
    return picks.cpu().numpy(), taken.cpu().numpy()


@pytest.mark.parametrize("seed,offset", SEEDS)
@pytest.mark.parametrize("n_cand,R", [(2048, 128), (2048, 300), (33, 128)])
def test_device_sampler_picks_are_exactly_the_restated_philox_draws(dev, n_cand, R, seed, offset):
    """proposal_target_sample_kernel, one (fg, bg) count per image, against tests/sampling_ref.py: the stream index, both
    64-bit words of seed and offset, Floyd's loop bounds and the with-replacement picks by absolute slot are all pinned"""
    counts = [c for c in SAMPLER_COUNTS if c[0] + c[1] <= n_cand]
    assert len(counts) == (len(SAMPLER_COUNTS) if n_cand == 2048 else 6)
    fg_per = 32
    want_p, want_t = SR.proposal_picks(counts, R, fg_per, seed, offset)
    got_p, got_t = _device_picks(dev, counts, n_cand, R, fg_per, seed, offset)
    assert np.array_equal(got_t, want_t)
    assert np.array_equal(got_p, want_p)
    for (nf, nb), p, t in zip(counts, want_p, want_t):  # the prediction itself is a valid sample
        assert len(set(p[:t])) == t or not (nf and nb)
        assert np.all(p[:t] < max(nf, 1)) and np.all(p[t:] < max(nb, 1)) and p.min() >= 0
    if R == 128:  # a call counter of 11 in device memory plus offset 4 is the plain call at offset 15
        want_p, want_t = SR.proposal_picks(counts, R, fg_per, seed, offset + 15)
        plain = _device_picks(dev, counts, n_cand, R, fg_per, seed, offset + 15)
        ctr = _device_picks(dev, counts, n_cand, R, fg_per, seed, offset + 4, counter=11)
        for got in (plain, ctr):
            assert np.array_equal(got[0], want_p) and np.array_equal(got[1], want_t)


def _expected_subsample(pre, nf, nb, bs, num_fg, seed, offset):
    """the pre-subsample rows with exactly the list positions dropped that the restated sampler does not keep"""
    keeps, inv_ne = SR.anchor_keep_masks(list(zip(nf, nb)), bs, num_fg, seed, offset)
    want = pre.clone()
    for b, (kf, kb) in enumerate(keeps):
        for kept, lab in ((kf, 1), (kb, 0)):
            if kept is not None:
                lst = torch.nonzero(pre[b] == lab).view(-1)
                drop = torch.ones(lst.numel(), dtype=torch.bool)
                drop[torch.tensor(kept, dtype=torch.long)] = False
                want[b, lst[drop]] = -1
    return want, inv_ne, keeps


@pytest.mark.parametrize("seed,offset", SEEDS)
@pytest.mark.parametrize("name,bs", [(n, None) for n in SEAM_CASES] + [("5x17", 4), ("9x19", 4)])
def test_device_anchor_subsample_drops_exactly_the_predicted_positions(dev, monkeypatch, name, bs, seed, offset):
    """anchor_target_subsample_kernel (streams 4b + 2 and 4b + 3) on the oracle's pre-subsample rows and lists"""
    from dana_amd import ops
    from dana_amd.config import cfg
    total = _total(name)
    bs = bs or 2 * total
    num_fg = int(cfg.TRAIN.RPN_FG_FRACTION * bs)
    pre, nf, nb = _presample(monkeypatch, name)
    want, inv_ne, keeps = _expected_subsample(pre, nf, nb, bs, num_fg, seed, offset)
    if bs == 4:  # both of Floyd's calls run
        assert any(kf is not None for kf, _ in keeps) and all(kb is not None for _, kb in keeps)
        assert not torch.equal(want, pre)
    else:
        assert torch.equal(want, pre)
    h = _assign(dev, name, bs, device_rng=(seed, offset))
    assert torch.equal(h["labels"].cpu(), want)
    assert h["inv_ne_dev"].cpu().numpy()[0] == inv_ne
    if bs == 4:  # the counter variant: 11 in device memory + offset 4 = offset 15
        want15, inv15, _ = _expected_subsample(pre, nf, nb, bs, num_fg, seed, offset + 15)
        c = ANCHOR_CASES[name]
        tr = cfg.TRAIN
        h2 = ops.anchor_target_prepare(c["gt"].to(dev), c["im_info"].to(dev), _base().to(dev), c["H"], c["W"], STRIDE,
                                       tr.RPN_NEGATIVE_OVERLAP, tr.RPN_POSITIVE_OVERLAP)
        ops.anchor_target_subsample_device(h2, bs, num_fg, seed, offset + 4,
                                           counter=torch.tensor([11], dtype=torch.int64, device=dev))
        assert torch.equal(h2["labels"].cpu(), want15) and h2["inv_ne_dev"].cpu().numpy()[0] == inv15
        # the float64 losses of the predicted row, through the device-side 1 / num_examples
        B, H, W = c["gt"].shape[0], c["H"], c["W"]
        lab_ref = want.view(B, H, W, A).permute(0, 3, 1, 2).reshape(B, 1, A * H, W)
        got = ops.anchor_target_outputs(h)
        assert torch.equal(got[0].cpu(), lab_ref)
        w_out = got[3].cpu()
        assert set(w_out.unique().tolist()) == {0.0, float(inv_ne)}


# ---- f. RCNN losses --------------------------------------------------------------------------------------------------------
def _smooth_l1(pred, tgt, w_in, w_out, sigma=1.0):
    """net_utils.py:71-85: sum over the 4 coordinates, mean over the rois"""
    s2 = sigma ** 2
    d = w_in * (pred - tgt)
    ad = d.abs()
    return (w_out * torch.where(ad < 1.0 / s2, d * d * (s2 / 2.0), ad - 0.5 / s2)).sum(1).mean()


def _rcnn_ref(sp, sn, lab, pred, tgt, w_in, w_out):
    """dana.py:199-217 (as in test_rcnn_losses_fused_vs_reference_formulation): -> losses, kept rows, the three seeds,
    and the background probabilities in their stable descending order per half"""
    n = lab.numel()
    sp, sn, pred = [t.double().requires_grad_(True) for t in (sp, sn, pred)]
    score = torch.cat([sp, sn], 0)
    label = torch.cat([lab, torch.zeros(n)], 0).long()
    fg = (label == 1).nonzero().squeeze(-1)
    bg = (label == 0).nonzero().squeeze(-1)
    soft = F.softmax(score, 1)[bg, :]
    n_all = label.shape[0]
    b0 = max(1, min(fg.shape[0] * 2, int(n_all * 0.25)))
    b1 = max(1, min(fg.shape[0], b0))
    p_sorted, order = torch.sort(soft[:, 1], descending=True, stable=True)
    real = bg[order]
    half0, half1 = real < int(n_all * 0.5), real >= int(n_all * 0.5)
    idx = torch.cat([fg, real[half0][:b0], real[half1][:b1]], 0)
    l_cls = F.cross_entropy(score[idx], label[idx])
    l_box = _smooth_l1(pred, tgt.double(), w_in.double(), w_out.double())
    (l_cls + l_box).backward()
    return dict(cls=float(l_cls.detach()), box=float(l_box.detach()), kept=idx.numel(), seeds=(sp.grad, sn.grad, pred.grad),
                b0=b0, b1=b1, p0=p_sorted[half0].detach(), p1=p_sorted[half1].detach())


def _check_rcnn(dev, sp, sn, lab, pred, tgt):
    from dana_amd import ops
    w_in = (lab.view(-1, 1) * torch.ones(1, 4)).contiguous()
    w_out = w_in.clone()
    ref = _rcnn_ref(sp, sn, lab, pred, tgt, w_in, w_out)
    out, seeds = ops.rcnn_losses(sp.to(dev), sn.to(dev), lab.to(dev), pred.to(dev), tgt.to(dev), w_in.to(dev), w_out.to(dev),
                                 with_grad=True)
    o = out.cpu()
    errs = [(s.cpu().double() - r).abs().max().item() for s, r in zip(seeds, ref["seeds"])]
    print("n %d fg %d: kept %d (ref %d) cls %.9g (ref %.9g) box %.9g (ref %.9g) seed errors %s" % (
        lab.numel(), int(lab.sum()), int(o[2]), ref["kept"], o[0], ref["cls"], o[1], ref["box"], errs))
    assert int(o[2]) == ref["kept"]
    assert abs(float(o[0]) - ref["cls"]) <= 2e-6 * max(1.0, abs(ref["cls"]))
    assert abs(float(o[1]) - ref["box"]) <= 2e-6 * max(1.0, abs(ref["box"]))
    # (a float32 torch CPU evaluation of the same formulation stays within 1e-7 of the float64 one on every case of this
    # file -- 3e-8 at the most here -- so the existing tests' absolute bound needs no scaling)
    assert max(errs) <= 1e-7
    return ref


@pytest.mark.parametrize("n,nfg", [(1, 0), (1, 1), (37, 5), (100, 100), (300, 0), (300, 17), (6200, 40)])
def test_rcnn_losses_row_counts_and_the_global_memory_rank_loop(dev, n, nfg):
    """rcnn_loss_{a,b,c}_kernel vs the float64 formulation: one row, rows that are no multiple of 64 or 256, a first half
    without any background row, no foreground at all, and 2n * 4 B > 48 KiB (ranks read from global memory)"""
    g = torch.Generator().manual_seed(1000 * n + nfg)
    sp, sn = torch.randn(n, 2, generator=g) * 2, torch.randn(n, 2, generator=g) * 2
    lab = torch.zeros(n)
    lab[torch.randperm(n, generator=g)[:nfg]] = 1
    pred, tgt = torch.randn(n, 4, generator=g), torch.randn(n, 4, generator=g) * 0.5
    ref = _check_rcnn(dev, sp, sn, lab, pred, tgt)
    if n == 6200:
        assert 2 * n * 4 > 48 * 1024
    if nfg == n:
        assert ref["p0"].numel() == 0 and ref["kept"] == n + ref["b1"]
    for p, q in ((ref["p0"], ref["b0"]), (ref["p1"], ref["b1"])):  # the quota does not cut between two float32 neighbours
        if q < p.numel():
            assert float(p[q - 1] - p[q]) > 1e-6 * float(p[q - 1])


TIE_POOLS = {
    # foreground probabilities 0.88, 0.73, 0.56, 0.38, 0.22, 0.08: at least 0.05 apart, so no rank between distinct values
    # can flip between float32 and float64
    "distinct": [(0.0, 2.0), (0.5, 1.5), (1.0, 1.25), (1.0, 0.5), (0.25, -1.0), (1.5, -1.0)],
    # saturated: the first three give exactly 1.0 in float32 AND in float64 (exp(-40) is below half an ulp of 1) with
    # cross-entropies 80, 60 and 40, so the order among them is the row index alone; (100, -100) gives exactly 0.0f
    "saturated": [(-40.0, 40.0), (-20.0, 40.0), (0.0, 40.0), (100.0, -100.0), (40.0, -40.0), (1.0, -1.0)],
}


@pytest.mark.parametrize("pool", list(TIE_POOLS))
def test_rcnn_losses_break_ties_in_the_foreground_probability_by_row_index(dev, pool):
    """both quotas cut INSIDE a run of rows with identical foreground probability: the kernel's "ties by row index" must
    keep what the reference's stable descending sort keeps"""
    n, nfg = 300, 17
    g = torch.Generator().manual_seed(5)
    pairs = torch.tensor(TIE_POOLS[pool])
    sp = pairs[torch.randint(0, 6, (n,), generator=g)].contiguous()
    sn = pairs[torch.randint(0, 6, (n,), generator=g)].contiguous()
    lab = torch.zeros(n)
    lab[torch.randperm(n, generator=g)[:nfg]] = 1
    pred, tgt = torch.randn(n, 4, generator=g), torch.randn(n, 4, generator=g) * 0.5
    ref = _check_rcnn(dev, sp, sn, lab, pred, tgt)
    assert (ref["b0"], ref["b1"]) == (34, 17)
    for p, q in ((ref["p0"], ref["b0"]), (ref["p1"], ref["b1"])):
        assert p.numel() > q and p[q - 1] == p[q]  # the last kept and the first dropped row tie exactly
    if pool == "saturated":
        assert float(ref["p0"][0]) == 1.0 and float(ref["p1"][0]) == 1.0
        assert float(F.softmax(torch.tensor([[100.0, -100.0]]), 1)[0, 1]) == 0.0  # exactly 0.0f in float32


@pytest.mark.parametrize("C", [1, 2, 21])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 300])
def test_plain_rcnn_losses_row_and_class_counts(dev, n, C):
    """plain_rcnn_loss_kernel (one 256-thread workgroup striding over the rows) around n = 256 and with 1, 2 and 21
    classes -- labels other than 1 for the sibling detectors -- vs float64 F.cross_entropy / smooth-L1 and autograd"""
    from dana_amd import ops
    g = torch.Generator().manual_seed(10 * n + C)
    sc, lab = torch.randn(n, C, generator=g), torch.randint(0, C, (n,), generator=g)
    bp, tg = torch.randn(n, 4, generator=g), torch.randn(n, 4, generator=g)
    win = (torch.rand(n, 4, generator=g) > 0.5).float()
    wout = win * torch.rand(n, 4, generator=g)
    s64, b64 = sc.double().requires_grad_(True), bp.double().requires_grad_(True)
    l_cls, l_box = F.cross_entropy(s64, lab), _smooth_l1(b64, tg.double(), win.double(), wout.double())
    (l_cls + l_box).backward()
    l_cls, l_box, grads = l_cls.item(), l_box.item(), (s64.grad, b64.grad)
    l2, seeds = ops.plain_rcnn_losses(sc.to(dev), lab.to(dev), bp.to(dev), tg.to(dev), win.to(dev), wout.to(dev), with_grad=True)
    errs = [(s.cpu().double() - r).abs().max().item() for s, r in zip(seeds, grads)]
    print("n %d C %d: cls %.9g (ref %.9g) box %.9g (ref %.9g) seed errors %s" % (n, C, l2[0], l_cls, l2[1], l_box, errs))
    if C > 2:
        assert int(lab.max()) > 1
    assert abs(float(l2[0]) - l_cls) <= 2e-6 * max(1.0, abs(l_cls))
    assert abs(float(l2[1]) - l_box) <= 2e-6 * max(1.0, abs(l_box))
    assert max(errs) <= 1e-7  # (as in _check_rcnn: a float32 CPU evaluation of this reference meets the bound itself)
