"""Sibling model `frcnn` of the reference's factory (utils.py:109-110): the plain class-agnostic Faster R-CNN of
lib/model/framework/faster_rcnn.py:17-203 on the SAME HIP operators as the DAnA path --
Caffe ResNet-50 trunk -> RPN -> proposal layer -> (train) anchor / proposal targets -> RoIAlign or RoIPool ->
layer4 -> RCNN_cls_score / RCNN_bbox_pred -> losses. Same parameter tree and state_dict keys as the reference class.
`frcnn` and `meta` are trainable on the HIP kernels too: a training forward saves its context and hands the four losses
to autograd (`_LossBridge`), `loss.backward()` runs the class's own `_backward` (POOLING_MODE 'align'), composed of the
shared pieces of backward.py."""
import numpy as np
import torch
import torch.nn as nn

from . import backward as BW
from . import ops
from .cached_inputs import ClassSweep, SupportCache, check_cached_forward, read_inputs
from .config import cfg
from .dana import DAnARCNN, _RPNParams


class FasterRCNN(DAnARCNN):
    def __init__(self, classes, num_layers=50, pretrained=False):
        nn.Module.__init__(self)
        self.model_path = "data/pretrained_model/resnet50_caffe.pth"
        self.dout_base_model = 1024
        self.pretrained = pretrained
        self.classes = classes
        self.n_classes = len(classes)
        self.class_agnostic = True
        self.semantic_enhance = False
        self.use_winograd = True
        self.winograd_tile = 4
        self.winograd_min_cin = 128
        self.merge_trunk = False
        self.presplit_weights = True
        self.nms_inclusive = False
        self.device_rng, self.rng_seed, self._rng_calls = False, 1996, 0
        self.RCNN_rpn = _RPNParams(self.dout_base_model)
        self._plan, self._consts, self._conv_cache, self._epoch = None, {}, {}, 0
        self._ctx = self._grad_anchor = None
        self._init_modules()
        self._init_weights()

    def _init_modules(self):
        DAnARCNN._init_modules(self)  # trunk, RCNN_top, RCNN_bbox_pred, the freezing rules (faster_rcnn.py:129-160)
        self.RCNN_cls_score = nn.Linear(2048, self.n_classes)

    def _init_weights(self):
        DAnARCNN._init_weights(self)
        self.RCNN_cls_score.weight.data.normal_(0, 0.01)
        self.RCNN_cls_score.bias.data.zero_()

    # ---- cached support sets of the support-conditioned siblings (meta, fsod, fgn) ---------------------------------
    _support_set = None  # (model, sup_ims [shot, 3, 320, 320], plan, dev) -> {name: tensor} of _cache_layout; None: frcnn

    def _cache_state(self, dev):
        """what a sibling's SupportCache depends on besides the support images (every state_dict tensor is in _sig)"""
        return (self._sig(), str(dev), type(self).__name__, int(self.n_shot))

    # meta, fsod and fgn average over the shots WHILE encoding (one class vector / kernel per set), so a set's cached
    # tensors are not per-shot blocks: no shot views, no ragged sets
    _no_shot_views = ("this detector averages over a set's shots while it encodes them (one vector per set), so its "
                      "cached tensors have no per-shot blocks to pick from: encode the shots you want as their own sets")

    def _cache_shot_blocks(self, sup_map):
        return None

    # a SupportBank holds what DAnA's support side reads in front of its first trained weight (trunk map + PE, its average
    # pool + PE); the siblings encode their supports their own way (class vectors through layer4, correlation kernels ...)
    _no_support_bank = ("the sibling detectors own their support encoders (meta's class vectors go through layer4, which "
                        "trains; fsod and fgn pool their own kernels; the plain Faster R-CNN has no support branch), so "
                        "DAnA's bank rows are not what their forwards read: train them from support images")

    # a QueryBank replaces the query trunk call of DAnA's `_trunks`, which writes into corr; the siblings' forwards own their
    # trunk calls and their own query-map buffers
    _no_query_bank = ("the sibling detectors run their own trunk calls into their own query-map buffers (DAnA's bank rows "
                      "are gathered into corr, which they do not have): run them from query images")

    def encode_supports(self, support_ims, num_shots=None):
        """support_ims [C, shot, 3, 320, 320] -> SupportCache of the model's per-set support tensors (`_cache_layout`),
        each set built by `_support_set` with the launches an uncached B = 1 eval forward issues for it. The forward takes
        the cache (or cache.select / cache.sweep) in place of support images, as DAnARCNN's does."""
        if self._support_set is None:
            raise TypeError("%s is the plain Faster R-CNN (faster_rcnn.py): it has no support branch, so there are no "
                            "support sets to encode" % type(self).__name__)
        if num_shots is not None:
            raise NotImplementedError("encode_supports(num_shots=): " + self._no_shot_views)
        C, shot, dev = self._check_support_sets(support_ims)
        if tuple(support_ims.shape[-2:]) != (320, 320):
            raise RuntimeError("support images must be 320x320 (a 20x20 stride-16 map) for a cached support set, got %dx%d"
                               % tuple(support_ims.shape[-2:]))
        plan = self._get_plan()
        with torch.no_grad():
            per_set = [self._support_set(support_ims[c].float().contiguous(), plan, dev) for c in range(C)]
            tensors = {k: torch.stack([p_[k].reshape(-1) for p_ in per_set]) for k in self._cache_layout(shot, (20, 20))}
        return SupportCache(self, tensors, shot, (20, 20), None, self._cache_state(dev), dev)

    def _cached_supports(self, support_ims, B, dev):
        """-> (the gathered per-problem support tensors, problems per image) when support_ims is a SupportCache or a
        ClassSweep (problems p = b*C + c), else (None, 1). One dana_gather_blocks launch, none for one set and one image"""
        _, cache, sweep, _ = read_inputs(None, support_ims)
        if cache is None:
            return None, 1
        check_cached_forward(self, dev, cache, sweep)
        if sweep is None:
            return cache._gather(B), 1
        return cache._gather(B * len(sweep), sweep._index(B)), len(sweep)

    # ---- shared stages of the sibling detectors (frcnn, meta): trunk -> RPN -> targets -> RoI features -> layer4 ----
    def _stages(self, im_data, im_info, gt_boxes, anchor_gt_boxes=None, rpn_input=None, ctx=None, group=1):
        """-> dict(B, NP, R, n_roi, rois, rpn losses, rois_label / targets (train), pooled, fc7 [n_roi][2048]).
        anchor_gt_boxes: boxes the anchor-target layer sees (meta.py:65 passes ALL classes' boxes); default gt_boxes.
        rpn_input(base, B, fh, fw, plan) -> (feature [B*group*h*w][1024], h, w): what the RPN runs on instead of base_feat
        (fsod.py:109-119: the attention RPN's correlation map, which is smaller than base_feat).
        group: a class sweep's problems per image (eval): the RPN, the proposals (im_info of image p / group), RoI pooling
        (rois' column 0 = p, base_feat of image p / group) and layer4 run over NP = B*group problems p = b*group + c"""
        plan = self._get_plan()
        dev = im_data.device
        training = self.training
        B = im_data.size(0)
        NP = B * group
        if group > 1 and training:
            raise RuntimeError("a class sweep runs in eval mode")
        im_info = im_info.data.float().contiguous()
        gt_boxes = gt_boxes.data
        anchor_gt = gt_boxes if anchor_gt_boxes is None else anchor_gt_boxes.data
        inputs_ready = ops.record_event()
        main = ops.cur_stream()
        # ctx (training): everything the model's `_backward` needs is saved into it
        base, fh, fw = self._rcnn_base(im_data, plan, save=ctx["q_saved"] if ctx is not None else None,
                                       save_from=ctx["t"] if ctx is not None else 3)  # faster_rcnn.py:43
        # -- RPN (rpn.py:58-115) on base_feat (or on the model's own RPN input) --
        rfeat, rh, rw = (base, fh, fw) if rpn_input is None else rpn_input(base, B, fh, fw, plan)
        base_hw = (fh, fw)
        fh, fw = rh, rw  # the RPN / anchor / proposal geometry below is the RPN input's
        x = self._rpn_conv(plan, rfeat, NP, fh, fw)
        heads, nh = self._rpn_head(plan, x, NP * fh * fw)
        if group > 1:  # problem p clips and filters with the im_info row of image p / group (one launch)
            im_info = ops.repeat_rows_grouped(im_info, 1, 3, group, NP, ld_src=im_info.size(1))
        rois = self._proposals(plan, heads, nh, im_info, NP, fh, fw)
        st = dict(B=B, NP=NP, rpn_loss_cls=0, rpn_loss_bbox=0, rois_label=None, labels_f=None)
        if training:
            tr_ = cfg.TRAIN
            side = self._stream("targets", dev)
            side.wait_event(inputs_ready)
            with ops.on_stream(side):
                at = ops.anchor_target_assign(anchor_gt.float(), im_info, plan["anchors"], fh, fw, self.RCNN_rpn.feat_stride,
                                              tr_.RPN_NEGATIVE_OVERLAP, tr_.RPN_POSITIVE_OVERLAP, tr_.RPN_BATCHSIZE,
                                              tr_.RPN_FG_FRACTION)
            at["ibuf"].record_stream(main)
            at["labels"].record_stream(main)
            main.wait_stream(side)
            rpn_l = ops.rpn_losses(heads, nh, at, sigma=3.0, inside_weight=tr_.RPN_BBOX_INSIDE_WEIGHTS[0])
            st["rpn_loss_cls"], st["rpn_loss_bbox"] = rpn_l[0], rpn_l[1]
            if ctx is not None:
                ctx.update(rpn_x=x, rpn_heads=heads, at=at, rpn_l=rpn_l, nh=nh, rpn_feat=rfeat, rfh=fh, rfw=fw)
            fg_per = int(np.round(tr_.FG_FRACTION * tr_.BATCH_SIZE)) or 1
            rois, rois_label, rois_target, rois_inside_ws, rois_outside_ws = ops.proposal_target_layer(
                rois, gt_boxes.float(), int(tr_.BATCH_SIZE), fg_per, tr_.FG_THRESH, tr_.BG_THRESH_HI, tr_.BG_THRESH_LO,
                tr_.BBOX_NORMALIZE_MEANS, tr_.BBOX_NORMALIZE_STDS, tr_.BBOX_INSIDE_WEIGHTS,
                tr_.BBOX_NORMALIZE_TARGETS_PRECOMPUTED)
            st["labels_f"] = rois_label.reshape(-1).contiguous()
            st["rois_label"] = st["labels_f"].long()
            st["rois_target"] = rois_target.view(-1, 4)
            st["rois_inside_ws"] = rois_inside_ws.view(-1, 4)
            st["rois_outside_ws"] = rois_outside_ws.view(-1, 4)
        R = rois.size(1)
        n_roi = NP * R
        P = cfg.POOLING_SIZE
        fh, fw = base_hw
        pooled, _ = self._roi_pool(plan, base, B, fh, fw, 1024, rois, group=group)  # (faster_rcnn.py:70-73) on base_feat
        st.update(rois=rois, R=R, n_roi=n_roi, pooled=pooled, plan=plan,
                  fc7=self._head_to_tail(pooled, n_roi, P, P, plan, save=ctx["l4_saved"] if ctx is not None else None))
        if ctx is not None:
            ctx.update(plan=plan, B=B, R=R, rois=rois, fh=fh, fw=fw, fc7=st["fc7"])
        return st

    def forward(self, im_data, im_info, gt_boxes, num_boxes):
        bridge, ctx = self._saving_ctx(("q_saved", "l4_saved"), align_only_for="frcnn")
        self._ctx = None
        st = self._stages(im_data, im_info, gt_boxes, ctx=ctx)
        B, R, n_roi, fc7 = st["B"], st["R"], st["n_roi"], st["fc7"]
        wb, bb = self._w(self.RCNN_bbox_pred)
        wc, bc = self._w(self.RCNN_cls_score)
        bbox_pred = ops.gemm_nt(fc7, wb, n_roi, 4, 2048, shift=bb)
        cls_score = ops.gemm_nt(fc7, wc, n_roi, self.n_classes, 2048, shift=bc)
        cls_prob = ops.softmax_rows_(cls_score.clone(), n_roi, self.n_classes)
        RCNN_loss_cls = RCNN_loss_bbox = 0
        rpn_loss_cls, rpn_loss_bbox = st["rpn_loss_cls"], st["rpn_loss_bbox"]
        if self.training:  # faster_rcnn.py:93-98
            if ctx is None:  # the same fused launch, without the gradient seeds
                l2, _ = ops.plain_rcnn_losses(cls_score, st["rois_label"], bbox_pred, st["rois_target"],
                                              st["rois_inside_ws"], st["rois_outside_ws"], with_grad=False)
                RCNN_loss_cls, RCNN_loss_bbox = l2[0], l2[1]
            else:
                # the two loss tails ([n_roi][2], [n_roi][4]) and their gradient seeds: one HIP launch (dana_plain_rcnn_loss)
                l2, (d_cls, d_bbox) = ops.plain_rcnn_losses(cls_score, st["rois_label"], bbox_pred, st["rois_target"],
                                                           st["rois_inside_ws"], st["rois_outside_ws"], with_grad=True)
                RCNN_loss_cls, RCNN_loss_bbox = l2[0], l2[1]
                ctx.update(loss_seeds=(d_cls, d_bbox))
                self._ctx = ctx
                if bridge:  # loss.backward() (train.py:141-143) runs self._backward on the HIP kernels
                    rpn_loss_cls, rpn_loss_bbox, RCNN_loss_cls, RCNN_loss_bbox = self._loss_bridge(
                        im_data.device, (rpn_loss_cls, rpn_loss_bbox, RCNN_loss_cls, RCNN_loss_bbox))
        return (st["rois"], cls_prob.view(B, R, -1), bbox_pred.view(B, R, -1), rpn_loss_cls, rpn_loss_bbox,
                RCNN_loss_cls, RCNN_loss_bbox, st["rois_label"])


    # ---- training backward: backward.model_backward_gen / grad_stages dispatch to these through the class --------------
    _head_params = BW.lin("RCNN_cls_score")  # the RoI head's own trainable parameters (every sibling names its own)

    def _grad_stages(self, plan, t=None):
        """t None: read off the parameters (backward.first_trainable_stage); the backward passes its context's"""
        return BW.sibling_grad_stages(plan, self._head_params, BW.first_trainable_stage(self) if t is None else t)

    def _backward_gen(self, grad_losses, ctx=None):
        """(DAnARCNN._backward_gen's generator contract; a sibling's backward, `_backward`, never pauses.) g = (g1, g2, g3, g4,
        g_dev) of backward.begin; the loss seeds are scaled by the device-resident ones here"""
        ctx, g, grads = BW.begin(self, grad_losses, ctx)
        BW.scale_seeds(ctx["loss_seeds"], g[4])
        self._backward(ctx, g, grads)
        yield from ()

    def _backward(self, ctx, g, grads):
        """d(sum_i grad_losses[i] * loss_i)/d(parameters) of the last training forward (faster_rcnn.py:31-105): RCNN_cls_score
        and RCNN_bbox_pred into fc7, then everything below it"""
        d_cls, d_bbox = ctx["loss_seeds"]  # d(loss_cls + loss_bbox) / d(cls_score, bbox_pred)
        BW.seed_linear_grads(self.RCNN_cls_score, d_cls, ctx["fc7"], g[2])
        d_fc7 = BW.seed_linear_dx(self.RCNN_bbox_pred, d_bbox, g[3])
        d_fc7.add_(BW.seed_linear_dx(self.RCNN_cls_score, d_cls, g[2]))
        self._backward_below_fc7(ctx, g, grads, d_bbox, d_fc7)

    def _backward_below_fc7(self, ctx, g, grads, d_bbox, d_fc7, gs=None):
        """what frcnn and meta share below the RoI head: mean <- layer4 <- RoIAlign, RPN losses <- heads <- 3x3 conv, both into
        base_feat, then the trainable stages of the trunk (ctx["t"]) for the query batch and (meta: gs) the support batch.
        Over a frozen trunk (t = 3) neither layer4's input gradient, the RoIAlign adjoint nor the RPN conv's data gradient
        is run: nothing would read them"""
        g1, g2, _, g4, g_dev = g
        trunk = ctx["t"] < 3
        BW.seed_linear_grads(self.RCNN_bbox_pred, d_bbox, ctx["fc7"], g4)
        d_pooled = BW.layer4_backward(d_fc7, ctx["B"] * ctx["R"], ctx["l4_saved"], grads, need_dx=trunk)
        grads.finish_all(self, "RCNN_top")
        BW.ready(self, self._grad_stages(ctx["plan"], ctx["t"])[0][1])
        d_bf = BW.roi_features_backward(ctx, d_pooled) if trunk else None
        gq = BW.sibling_rpn_backward(self, ctx, g1, g2, g_dev, grads, residual=d_bf)  # d base_feat = RPN + RoIAlign paths
        grads.finish_all(self, "RCNN_rpn")
        BW.ready(self, BW.RPN_PARAMS)
        BW.trunk_backward(self, ctx, grads, gq, gs)


class MetaRCNN(FasterRCNN):
    """Sibling model `meta` (utils.py:113-114): Meta R-CNN, lib/model/framework/meta.py:18-251. The Predictor-head
    Remodeling Network turns every support image into a class-attentive vector, sigmoid(mean(layer4(maxpool2(trunk)))),
    the shots' mean multiplies the RoI features channel-wise in front of a 2-way Linear; positive + negative supports
    and the 1:2:1 hard-negative-mined loss as in DAnA. Trainable: `_backward` below."""

    def __init__(self, classes, num_layers=50, pretrained=False, num_way=2, num_shot=5):
        self.n_way, self.n_shot = num_way, num_shot
        FasterRCNN.__init__(self, classes, num_layers, pretrained)

    def _init_modules(self):
        FasterRCNN._init_modules(self)
        self.RCNN_cls_score = nn.Sequential(nn.Linear(2048, 2))  # meta.py:199-201 (state_dict key RCNN_cls_score.0.*)

    def _init_weights(self):  # meta.py:144-159: RCNN_cls_score keeps its default init
        DAnARCNN._init_weights(self)

    def _cache_layout(self, shot, sup_map):
        """a set's class-attentive vector: the mean over its shots of sigmoid(mean(layer4(maxpool2(trunk))))"""
        return dict(vec=(2048,))

    def _support_set(self, sup_ims, plan, dev):
        """the PRN (meta.py:58-62,241-251) of one support set, as the uncached eval forward runs it for one image"""
        shot = sup_ims.size(0)
        sup, sh_, sw_ = self._rcnn_base(sup_ims, plan)
        mp, mh, mw = ops.maxpool2x2s2(sup, shot, sh_, sw_, 1024)
        att = ops.sigmoid_(self._head_to_tail(mp, shot, mh, mw, plan))
        return dict(vec=ops.spatial_mean(att, 1, shot, 2048))

    def _cached_forward(self, im_data, im_info, gt_boxes, all_cls_gt_boxes, vec, Cs, sweep):
        """the eval forward on cached class-attentive vectors vec [B*Cs][2048]. The RPN runs on base_feat alone
        (meta.py:65), so proposals, RoIAlign and layer4 run once per image; a sweep's 2-way heads of all Cs classes are one
        launch (dana_meta_class_head) that writes the problems' rois / cls_prob / bbox_pred in ClassSweep's layout"""
        st = self._stages(im_data, im_info, gt_boxes, anchor_gt_boxes=all_cls_gt_boxes)
        B, R, n_roi, fc7 = st["B"], st["R"], st["n_roi"], st["fc7"]
        wb, bb = self._w(self.RCNN_bbox_pred)
        wc, bc = self._w(self.RCNN_cls_score[0])
        bbox_pred = ops.gemm_nt(fc7, wb, n_roi, 4, 2048, shift=bb)
        if sweep:
            rois, cls_prob, bbox_pred = ops.meta_class_head(fc7, vec, wc, bc, st["rois"], bbox_pred, B, Cs, R)
            return (rois, cls_prob, bbox_pred, 0, 0, 0, 0, None)
        comb = ops.scale_rows_by_group(fc7, vec, n_roi, R, 2048)
        score = ops.gemm_nt(comb, wc, n_roi, 2, 2048, shift=bc)
        return (st["rois"], ops.softmax_rows_(score.clone(), n_roi, 2), bbox_pred, 0, 0, 0, 0, None)

    def forward(self, im_data, im_info, gt_boxes, num_boxes, support_ims, all_cls_gt_boxes=None):
        if all_cls_gt_boxes is None:
            raise RuntimeError("meta: all_cls_gt_boxes is required (meta.py:48,65)")
        cached, Cs = self._cached_supports(support_ims, im_data.size(0), im_data.device)
        if cached is not None:
            return self._cached_forward(im_data, im_info, gt_boxes, all_cls_gt_boxes, cached["vec"], Cs,
                                        isinstance(support_ims, ClassSweep))
        training = self.training
        shot = self.n_shot
        way = self.n_way if training else 1
        bridge, ctx = self._saving_ctx(("q_saved", "l4_saved", "s_saved", "sl4_saved", "heads"), align_only_for="meta")
        self._ctx = None
        st = self._stages(im_data, im_info, gt_boxes, anchor_gt_boxes=all_cls_gt_boxes, ctx=ctx)
        B, R, n_roi, fc7, plan = st["B"], st["R"], st["n_roi"], st["fc7"], st["plan"]
        # PRN (meta.py:241-251) on every support image
        sup_ims = self._support_batch(support_ims, B, way, shot)
        Ns = sup_ims.size(0)
        sup, sh_, sw_ = self._rcnn_base(sup_ims, plan, save=ctx["s_saved"] if ctx is not None else None,
                                        save_from=ctx["t"] if ctx is not None else 3)
        mp, mh, mw = ops.maxpool2x2s2(sup, Ns, sh_, sw_, 1024)
        att = ops.sigmoid_(self._head_to_tail(mp, Ns, mh, mw, plan, save=ctx["sl4_saved"] if ctx is not None else None))
        wb, bb = self._w(self.RCNN_bbox_pred)
        wc, bc = self._w(self.RCNN_cls_score[0])
        bbox_pred = ops.gemm_nt(fc7, wb, n_roi, 4, 2048, shift=bb)

        def head(offset):  # supports [offset, offset + shot) of every episode: their mean vector x the RoI features
            vec = torch.empty((B, 2048), dtype=torch.float32, device=fc7.device)
            for b in range(B):
                vec[b:b + 1] = ops.spatial_mean(att.view(-1)[(b * way * shot + offset) * 2048:], 1, shot, 2048)
            comb = ops.scale_rows_by_group(fc7, vec, n_roi, R, 2048)
            score = ops.gemm_nt(comb, wc, n_roi, 2, 2048, shift=bc)
            if ctx is not None:
                ctx["heads"].append(dict(offset=offset, vec=vec, comb=comb))
            return ops.softmax_rows_(score.clone(), n_roi, 2), score

        cls_prob, cls_score = head(0)
        RCNN_loss_cls = RCNN_loss_bbox = 0
        rois_label = st["rois_label"]
        rpn_loss_cls, rpn_loss_bbox = st["rpn_loss_cls"], st["rpn_loss_bbox"]
        if training:
            neg_prob, neg_score = head(shot)
            cls_prob = torch.cat([cls_prob, neg_prob], 0)
            rois_label = torch.cat([rois_label, torch.zeros_like(rois_label)], 0)
            rl, seeds = ops.rcnn_losses(cls_score, neg_score, st["labels_f"], bbox_pred, st["rois_target"].contiguous(),
                                        st["rois_inside_ws"].contiguous(), st["rois_outside_ws"].contiguous(),
                                        with_grad=ctx is not None)
            RCNN_loss_cls, RCNN_loss_bbox = rl[0], rl[1]
            if ctx is not None:
                ctx.update(loss_seeds=seeds, att=att, sup=sup, sup_hw=(sh_, sw_), mp_hw=(mh, mw), Ns=Ns, shot=shot, way=way)
                self._ctx = ctx
                if bridge:  # loss.backward() (train.py:141-143) runs self._backward on the HIP kernels
                    rpn_loss_cls, rpn_loss_bbox, RCNN_loss_cls, RCNN_loss_bbox = self._loss_bridge(
                        im_data.device, (rpn_loss_cls, rpn_loss_bbox, RCNN_loss_cls, RCNN_loss_bbox))
        return (st["rois"], cls_prob, bbox_pred, rpn_loss_cls, rpn_loss_bbox, RCNN_loss_cls, RCNN_loss_bbox, rois_label)

    _head_params = BW.lin("RCNN_cls_score.0")  # meta.py:199-201: a Sequential

    def _backward(self, ctx, g, grads):
        """frcnn's adjoint (meta.py:39-142) plus the class-attentive vectors: score = Linear(fc7 * mean_shots(sigmoid(mean(
        layer4(maxpool2(trunk(support))))))) for the positive and the negative supports, so the support batch is
        differentiated through layer4 and the trunk too"""
        d_pos, d_neg, d_bbox = ctx["loss_seeds"]  # written by the fused mined-loss kernel (dana_rcnn_loss)
        B, R, Ns, shot, way, fc7, att = ctx["B"], ctx["R"], ctx["Ns"], ctx["shot"], ctx["way"], ctx["fc7"], ctx["att"]
        d_fc7 = BW.seed_linear_dx(self.RCNN_bbox_pred, d_bbox, g[3])
        d_att = torch.zeros((B, way * shot, 2048), dtype=torch.float32, device=fc7.device)
        for hc in ctx["heads"]:
            ds = d_pos if hc["offset"] == 0 else d_neg
            BW.seed_linear_grads(self.RCNN_cls_score[0], ds, hc["comb"], g[2])
            d_comb = BW.seed_linear_dx(self.RCNN_cls_score[0], ds, g[2])
            d_fc7.add_(ops.scale_rows_by_group(d_comb, hc["vec"], B * R, R, 2048))
            # the shots' mean of the attentive vectors: d vec[b] = sum over the image's rois of d_comb * fc7
            d_vec = (d_comb * fc7).view(B, R, 2048).sum(1) / shot
            d_att[:, hc["offset"]:hc["offset"] + shot] += d_vec.unsqueeze(1)
        d_pre = (d_att.view(Ns, 2048) * att * (1.0 - att)).contiguous()  # sigmoid adjoint (meta.py:250)
        d_mp = BW.layer4_backward(d_pre, Ns, ctx["sl4_saved"], grads, need_dx=ctx["t"] < 3)
        gs = None
        if d_mp is not None:  # (None: the trunk is frozen, the support maps' gradient has no reader)
            # 2x2 / 2 max pool (meta.py:247) back onto the support maps: the window's (first) maximum takes the gradient
            (sh_, sw_), (mh, mw) = ctx["sup_hw"], ctx["mp_hw"]
            gs = ops.maxpool2x2s2_backward(ctx["sup"].view(Ns * sh_ * sw_, 1024), d_mp.contiguous().view(Ns * mh * mw, 1024),
                                           Ns, sh_, sw_, 1024)
        self._backward_below_fc7(ctx, g, grads, d_bbox, d_fc7, gs)
