"""Attention maps: where each box looks in its support shots (the reference's README, "Attention Visualization").

`attention_maps` (also `DAnARCNN.attention_maps`) runs the staged eval forward as far as the attention weights -- query
trunk, support side or cache gather, RPN-level softmax, RoIAlign of the given boxes, RoI-level Q projection and softmax
-- and reduces them per box on the device (dana_attn_box_mean). No RPN conv, no proposals, no layer4, no FFN.
`upsample` / `render` turn any [..., gh, gw] map into S x S numbers or into the README's colour overlay
(dana_heatmap_upsample / dana_heatmap_render).

The three levels, for NP problems (B images, or B*C under a class sweep, image b's C classes contiguous), n boxes,
m shots and the (sh, sw) = 20 x 20 support map:
  ba   [NP][m][sh][sw]     the BA block's support_spatial_weight (dana.py:134-135): softmax over a shot's positions.
                           Only from support images with semantic_enhance on (a SupportCache keeps the BA-enhanced rows,
                           not the weights).
  rpn  [NP][n][m][sh][sw]  support_adaptive_attention_weight (dana.py:142-146): per query feature cell and shot,
                           softmax over the shot's sh*sw keys + unary_gamma * unary -- NOT divided by the number of
                           shots -- averaged over the cells the box covers (`cell_rect`).
  roi  [NP][n][m][7][7]    the same weights at the RoI level (dana.py:273-277): the box RoI-pooled from base_feat by
                           the forward's operator, PE added, Q-projected; averaged over the 49 query bins.
Every rpn / roi map of a real shot sums to 1 + unary_gamma, every ba map to 1. A padded slot of a ragged shot view is
all zero; real slots are not scaled by the view's 1 / len."""
import math
from collections import namedtuple

import torch

from . import ops
from .cached_inputs import read_inputs
from .config import cfg
from .dana import ATTENTION_LEVELS, DAnARCNN

AttentionMaps = namedtuple("AttentionMaps", ATTENTION_LEVELS)

# value -> colour, blue -> cyan -> green -> yellow -> red in 256 steps (R, G, B): entry round(255 t) for a map
# normalised to t in [0, 1]. Written out: no plotting library is involved.
COLOR_TABLE = (
    (0, 0, 255), (0, 4, 255), (0, 8, 255), (0, 12, 255), (0, 16, 255), (0, 20, 255), (0, 24, 255), (0, 28, 255),
    (0, 32, 255), (0, 36, 255), (0, 40, 255), (0, 44, 255), (0, 48, 255), (0, 52, 255), (0, 56, 255), (0, 60, 255),
    (0, 64, 255), (0, 68, 255), (0, 72, 255), (0, 76, 255), (0, 80, 255), (0, 84, 255), (0, 88, 255), (0, 92, 255),
    (0, 96, 255), (0, 100, 255), (0, 104, 255), (0, 108, 255), (0, 112, 255), (0, 116, 255), (0, 120, 255), (0, 124, 255),
    (0, 128, 255), (0, 132, 255), (0, 136, 255), (0, 140, 255), (0, 144, 255), (0, 148, 255), (0, 152, 255), (0, 156, 255),
    (0, 160, 255), (0, 164, 255), (0, 168, 255), (0, 172, 255), (0, 176, 255), (0, 180, 255), (0, 184, 255), (0, 188, 255),
    (0, 192, 255), (0, 196, 255), (0, 200, 255), (0, 204, 255), (0, 208, 255), (0, 212, 255), (0, 216, 255), (0, 220, 255),
    (0, 224, 255), (0, 228, 255), (0, 232, 255), (0, 236, 255), (0, 240, 255), (0, 244, 255), (0, 248, 255), (0, 252, 255),
    (0, 255, 254), (0, 255, 250), (0, 255, 246), (0, 255, 242), (0, 255, 238), (0, 255, 234), (0, 255, 230), (0, 255, 226),
    (0, 255, 222), (0, 255, 218), (0, 255, 214), (0, 255, 210), (0, 255, 206), (0, 255, 202), (0, 255, 198), (0, 255, 194),
    (0, 255, 190), (0, 255, 186), (0, 255, 182), (0, 255, 178), (0, 255, 174), (0, 255, 170), (0, 255, 166), (0, 255, 162),
    (0, 255, 158), (0, 255, 154), (0, 255, 150), (0, 255, 146), (0, 255, 142), (0, 255, 138), (0, 255, 134), (0, 255, 130),
    (0, 255, 126), (0, 255, 122), (0, 255, 118), (0, 255, 114), (0, 255, 110), (0, 255, 106), (0, 255, 102), (0, 255, 98),
    (0, 255, 94), (0, 255, 90), (0, 255, 86), (0, 255, 82), (0, 255, 78), (0, 255, 74), (0, 255, 70), (0, 255, 66),
    (0, 255, 62), (0, 255, 58), (0, 255, 54), (0, 255, 50), (0, 255, 46), (0, 255, 42), (0, 255, 38), (0, 255, 34),
    (0, 255, 30), (0, 255, 26), (0, 255, 22), (0, 255, 18), (0, 255, 14), (0, 255, 10), (0, 255, 6), (0, 255, 2),
    (2, 255, 0), (6, 255, 0), (10, 255, 0), (14, 255, 0), (18, 255, 0), (22, 255, 0), (26, 255, 0), (30, 255, 0),
    (34, 255, 0), (38, 255, 0), (42, 255, 0), (46, 255, 0), (50, 255, 0), (54, 255, 0), (58, 255, 0), (62, 255, 0),
    (66, 255, 0), (70, 255, 0), (74, 255, 0), (78, 255, 0), (82, 255, 0), (86, 255, 0), (90, 255, 0), (94, 255, 0),
    (98, 255, 0), (102, 255, 0), (106, 255, 0), (110, 255, 0), (114, 255, 0), (118, 255, 0), (122, 255, 0), (126, 255, 0),
    (130, 255, 0), (134, 255, 0), (138, 255, 0), (142, 255, 0), (146, 255, 0), (150, 255, 0), (154, 255, 0), (158, 255, 0),
    (162, 255, 0), (166, 255, 0), (170, 255, 0), (174, 255, 0), (178, 255, 0), (182, 255, 0), (186, 255, 0), (190, 255, 0),
    (194, 255, 0), (198, 255, 0), (202, 255, 0), (206, 255, 0), (210, 255, 0), (214, 255, 0), (218, 255, 0), (222, 255, 0),
    (226, 255, 0), (230, 255, 0), (234, 255, 0), (238, 255, 0), (242, 255, 0), (246, 255, 0), (250, 255, 0), (254, 255, 0),
    (255, 252, 0), (255, 248, 0), (255, 244, 0), (255, 240, 0), (255, 236, 0), (255, 232, 0), (255, 228, 0), (255, 224, 0),
    (255, 220, 0), (255, 216, 0), (255, 212, 0), (255, 208, 0), (255, 204, 0), (255, 200, 0), (255, 196, 0), (255, 192, 0),
    (255, 188, 0), (255, 184, 0), (255, 180, 0), (255, 176, 0), (255, 172, 0), (255, 168, 0), (255, 164, 0), (255, 160, 0),
    (255, 156, 0), (255, 152, 0), (255, 148, 0), (255, 144, 0), (255, 140, 0), (255, 136, 0), (255, 132, 0), (255, 128, 0),
    (255, 124, 0), (255, 120, 0), (255, 116, 0), (255, 112, 0), (255, 108, 0), (255, 104, 0), (255, 100, 0), (255, 96, 0),
    (255, 92, 0), (255, 88, 0), (255, 84, 0), (255, 80, 0), (255, 76, 0), (255, 72, 0), (255, 68, 0), (255, 64, 0),
    (255, 60, 0), (255, 56, 0), (255, 52, 0), (255, 48, 0), (255, 44, 0), (255, 40, 0), (255, 36, 0), (255, 32, 0),
    (255, 28, 0), (255, 24, 0), (255, 20, 0), (255, 16, 0), (255, 12, 0), (255, 8, 0), (255, 4, 0), (255, 0, 0),
)

_TABLES = {}  # device -> COLOR_TABLE as a uint8 [256][3] tensor there


def cell_rect(box, fh, fw, stride=16):
    """The feature cells a box covers, (x_lo, y_lo, x_hi, y_hi) inclusive, on an (fh, fw) grid of `stride`-pixel cells:
    x_lo = clamp(floor(x1 / stride), 0, fw - 1), x_hi = clamp(floor(x2 / stride), x_lo, fw - 1), the same for y with fh.
    Never empty: a box with x2 < x1, or one outside the image, covers one cell. The rule dana_attn_box_mean applies in
    its kernel (csrc/attention_maps.hip), here in Python for hand-worked checks."""
    x1, y1, x2, y2 = (float(v) for v in box)

    def clamp(v, lo, hi):
        return int(min(max(math.floor(v / stride), lo), hi))

    x_lo, y_lo = clamp(x1, 0, fw - 1), clamp(y1, 0, fh - 1)
    return x_lo, y_lo, clamp(x2, x_lo, fw - 1), clamp(y2, y_lo, fh - 1)


def check_levels(levels):
    """-> the requested levels as a tuple; ValueError for anything but names out of ("ba", "rpn", "roi")"""
    if isinstance(levels, str):
        levels = (levels,)
    levels = tuple(levels)
    bad = [lv for lv in levels if lv not in ATTENTION_LEVELS]
    if bad or not levels:
        raise ValueError("attention_maps: levels must name some of %s, got %s" % (list(ATTENTION_LEVELS), list(levels)))
    return levels


def check_boxes(boxes, im_data):
    """host-side checks of `boxes` [B][n][4] (no device read) -> n"""
    if not torch.is_tensor(boxes) or boxes.dim() != 3 or boxes.size(2) != 4:
        raise ValueError("attention_maps: boxes must be a [B][n][4] tensor of (x1, y1, x2, y2) in network-input pixels, "
                         "got %s" % (tuple(boxes.shape) if torch.is_tensor(boxes) else type(boxes),))
    if boxes.dtype != torch.float32:
        raise ValueError("attention_maps: boxes must be float32, got %s" % boxes.dtype)
    if boxes.size(1) < 1:
        raise ValueError("attention_maps: no boxes (n >= 1)")
    if boxes.size(0) != im_data.size(0):
        raise ValueError("attention_maps: boxes for %d images, im_data holds %d" % (boxes.size(0), im_data.size(0)))
    if not boxes.is_cuda:
        raise ValueError("attention_maps: boxes must be a CUDA (HIP) tensor: this build has no CPU path")
    return boxes.size(1)


def attention_maps(model, im_data, im_info, boxes, support, levels=ATTENTION_LEVELS):
    """model.eval(), under torch.no_grad(): im_data / im_info as for an eval forward, boxes float32 [B][n][4] on the device
    (the coordinates of rois[:, :, 1:5]; under a sweep image b's boxes apply to each of its C problems), support whatever
    the eval forward takes as its 5th argument (support images, a SupportCache selection, a ClassSweep)
    -> AttentionMaps(ba, rpn, roi) of float32 device tensors (module docstring); a level not in `levels` is None. `ba`
    needs support images and the BA block: without them it is None, or a ValueError when `levels` names it explicitly."""
    qbatch, cache, _, _ = read_inputs(im_data, support)
    if qbatch is not None:
        raise TypeError("attention_maps takes the query images themselves (im_data [B, 3, H, W]), not a QueryBatch: the maps "
                        "are an inspection tool and run the trunk")
    explicit = levels is not ATTENTION_LEVELS
    levels = check_levels(levels)
    if type(model)._forward_gen is not DAnARCNN._forward_gen:
        raise NotImplementedError("attention maps are defined for DAnARCNN (the sibling detectors have no such weights)")
    if model.training:
        raise RuntimeError("attention_maps runs in eval mode (model.eval()): it reads the weights of an eval forward")
    want_ba = "ba" in levels
    if want_ba and (cache is not None or not model.semantic_enhance):
        if explicit:
            raise ValueError("attention_maps: level 'ba' needs support images and a model with the BA block "
                             "(semantic_enhance): a SupportCache stores the BA-enhanced rows, not the weights")
        want_ba = False
    n = check_boxes(boxes, im_data)
    P = cfg.POOLING_SIZE
    with torch.no_grad():
        boxes = boxes.contiguous()
        f = model._forward_setup(im_data, im_info, boxes, support)
        f.maps = {}
        corr, (fh, fw), sup = model._trunks(f, im_data, support)
        model._rpn_attention(f, corr, fh, fw, sup)  # (joins the support stream; leaves the weights in f.maps["rpn_w"])
        NP, m, (sh, sw) = f.NP, f.shot, sup["map"]
        ba = rpn = roi = None
        if want_ba:
            ba = f.maps["ba_w"].view(f.B, m, sh, sw)
        if "rpn" in levels:
            rpn = ops.attn_box_mean(f.maps["rpn_w"], boxes, n, fh, fw, group=f.Cs,
                                    cell=float(model.RCNN_rpn.feat_stride)).view(NP, n, m, sh, sw)
        if "roi" in levels:
            model._roi_support(f, sup)
            # rois of the NP problems: column 0 the problem (RoIAlign reads image p / C), then image p / C's boxes
            rois = torch.cat([torch.arange(NP, dtype=torch.float32, device=f.dev).view(NP, 1, 1).expand(NP, n, 1),
                              boxes.view(f.B, 1, n, 4).expand(f.B, f.Cs, n, 4).reshape(NP, n, 4)], 2).contiguous()
            fold_pe = cfg.POOLING_MODE == "align" and getattr(model, "fold_roi_pe", True) and not f.product
            pooled, q_pe = model._roi_pool(f.plan, corr, f.B, fh, fw, 2048, rois, pe=not fold_pe, group=f.Cs)
            if sup["roi_done"] is not None:
                f.main.wait_event(sup["roi_done"])
            q2, qld, _ = model._roi_query(f, pooled, q_pe, fold_pe, NP * n)
            sc2 = model._roi_scores(f, q2, qld, sup["k2"].view(-1), sup["un2"].view(-1), n)
            roi = ops.attn_box_mean(sc2, None, n, P, P, k=m * P * P, roi=True).view(NP, n, m, P, P)
    return AttentionMaps(ba=ba, rpn=rpn, roi=roi)


def _maps_2d(maps_2d):
    if not torch.is_tensor(maps_2d) or maps_2d.dim() < 2 or maps_2d.dtype != torch.float32:
        raise ValueError("maps must be a float32 [..., gh, gw] tensor, got %s"
                         % ((tuple(maps_2d.shape), maps_2d.dtype) if torch.is_tensor(maps_2d) else type(maps_2d),))
    if not maps_2d.is_cuda:
        raise ValueError("maps must be a CUDA (HIP) tensor: this build has no CPU path")
    return maps_2d.contiguous()


def upsample(maps_2d, size):
    """[..., gh, gw] float32 maps -> [..., size, size] float32, bilinear with the cv2.resize convention"""
    if int(size) < 1:
        raise ValueError("upsample: size must be >= 1, got %s" % (size,))
    return ops.heatmap_upsample(_maps_2d(maps_2d), int(size))


def render(maps_2d, images, alpha=0.5):
    """maps [..., gh, gw] float32 and the matching prepared support images [..., 3, S, S] (BGR, mean-subtracted, as the
    model is fed) -> uint8 [..., S, S, 3] RGB: each map upsampled to S x S, min-max normalised (a constant map goes to
    0), coloured by COLOR_TABLE and blended, (1 - alpha) * image + alpha * colour, over the image restored to RGB
    0..255 with cfg.PIXEL_MEANS. One launch."""
    maps_2d = _maps_2d(maps_2d)
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError("render: alpha must be in [0, 1], got %s" % (alpha,))
    if (not torch.is_tensor(images) or images.dim() != maps_2d.dim() + 1 or images.dtype != torch.float32
            or tuple(images.shape[:-3]) != tuple(maps_2d.shape[:-2]) or images.size(-3) != 3 or images.size(-1) != images.size(-2)):
        raise ValueError("render: images must be float32 [..., 3, S, S] with the maps' leading dimensions %s, got %s"
                         % (tuple(maps_2d.shape[:-2]), tuple(images.shape) if torch.is_tensor(images) else type(images)))
    if not images.is_cuda:
        raise ValueError("render: images must be a CUDA (HIP) tensor: this build has no CPU path")
    key = str(maps_2d.device)
    table = _TABLES.get(key)
    if table is None:
        table = _TABLES[key] = torch.tensor(COLOR_TABLE, dtype=torch.uint8).to(maps_2d.device)
    means = [float(v) for v in torch.as_tensor(cfg.PIXEL_MEANS).reshape(-1).tolist()]  # (B, G, R)
    return ops.heatmap_render(maps_2d, images.contiguous(), table, float(alpha), means)
