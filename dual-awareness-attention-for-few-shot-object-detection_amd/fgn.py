"""Sibling model `fgn` of the reference's factory (utils.py:115-116): lib/model/framework/fgn.py:18-259 on the same HIP
operators.

* attention RPN (fgn.py:63-82): base_feat is re-weighted channel-wise by the global mean of the positive supports'
  mean map (`dana_scale_rows_by_group`), the RPN runs on that;
* head (fgn.py:145-165): [support 7x7 | roi 7x7] -> 3x3 conv (2048->512, no padding) -> BatchNorm -> ReLU -> 3x3 conv
  (512->128) -> BatchNorm -> ReLU -> Linear(1152, 2). The concatenation never exists (the support half of the first conv
  is computed once per image and added as a residual). bn1 / bn2 are ORDINARY BatchNorm layers, unlike the trunk's:
  batch statistics and running-statistics updates in train mode (`dana_batch_stats`), running statistics in eval mode.
Same parameter tree as the reference class. Trainable: `FGN._backward` (train-mode BatchNorm adjoints, the split first
conv, the channel re-weighting of the RPN input, the support trunk)."""
import torch
import torch.nn as nn

from . import backward as BW
from . import ops
from .cached_inputs import ClassSweep
from .dana import DAnARCNN
from .frcnn import FasterRCNN


class FGN(FasterRCNN):
    def __init__(self, classes, num_layers=50, pretrained=False, num_way=2, num_shot=5):
        self.n_way, self.n_shot = num_way, num_shot
        FasterRCNN.__init__(self, classes, num_layers, pretrained)

    def _init_modules(self):
        FasterRCNN._init_modules(self)
        self.cls_conv1 = nn.Conv2d(2048, 512, 3, padding=0, bias=False)
        self.bn1 = nn.BatchNorm2d(512)
        self.cls_conv2 = nn.Conv2d(512, 128, 3, padding=0, bias=False)
        self.bn2 = nn.BatchNorm2d(128)
        self.RCNN_cls_score = nn.Linear(1152, 2)
        mods = self._modules  # the reference's registration order (fgn.py:29-41 then :207-219)
        for k in ("RCNN_rpn", "cls_conv1", "bn1", "cls_conv2", "bn2", "RCNN_base", "RCNN_top", "RCNN_cls_score",
                  "RCNN_bbox_pred"):
            mods[k] = mods.pop(k)

    def _init_weights(self):  # fgn.py:167-183: RCNN_cls_score keeps its default init
        DAnARCNN._init_weights(self)

    def _bn(self, x, rows, bn, save=None):
        """nn.BatchNorm2d on NHWC rows, in place, followed by ReLU: batch statistics + running update when bn.training.
        save: list that receives (pre-BN copy of x, batch mean, batch var) for the backward"""
        C = bn.num_features
        if bn.training:
            mean, var = ops.batch_stats(x, rows, C)
            if save is not None:
                save.append((x.clone(), mean, var))
            with torch.no_grad():  # F.batch_norm's running update: momentum 0.1, UNBIASED variance
                bn.running_mean.mul_(1 - bn.momentum).add_(mean, alpha=bn.momentum)
                bn.running_var.mul_(1 - bn.momentum).add_(var, alpha=bn.momentum * rows / max(rows - 1, 1))
                bn.num_batches_tracked += 1
        else:
            mean, var = bn.running_mean, bn.running_var
        scale, shift = ops.bn_fold(bn.weight, bn.bias, mean, var, bn.eps)
        return ops.scale_shift_relu_(x, scale, shift, rows, C, relu=True)

    # ---- cached support sets (encode_supports) ---------------------------------------------------------------------
    def _cache_layout(self, shot, sup_map):
        """pos_rpn: AvgPool2d(20) of the shots' mean map (fgn.py:71-73); s_half: the support half of cls_conv1 (3x3 valid)
        on its AvgPool2d(14, 1) (fgn.py:148-152)"""
        return dict(pos_rpn=(1024,), s_half=(25, 512))

    def _support_set(self, sup_ims, plan, dev):
        """one support set's cache tensors, with the launches of the uncached eval forward at B = 1"""
        shot = sup_ims.size(0)
        sup, sh_, sw_ = self._rcnn_base(sup_ims, plan)
        L = sh_ * sw_
        pos_map = ops.spatial_mean(sup, 1, shot, L * 1024)
        pos_rpn = ops.spatial_mean(pos_map, 1, L, 1024)
        pos_rcnn = ops.avgpool(pos_map, 1, sh_, sw_, 1024, 14, 1)
        w1_sup = ops.pack_conv_weight(self.cls_conv1.weight.detach()[:, :1024].contiguous())
        s_half, _, _ = ops.conv2d_nhwc(pos_rcnn, 1, 7, 7, 1024, w1_sup, 512, 3, 3, 1, 0)
        return dict(pos_rpn=pos_rpn, s_half=s_half)

    def forward(self, im_data, im_info, gt_boxes, num_boxes, support_ims, all_cls_gt_boxes=None):
        training = self.training
        shot = self.n_shot
        way = self.n_way if training else 1
        B = im_data.size(0)
        dev = im_data.device
        plan = self._get_plan()
        # cached: the support sets' tensors gathered per problem (a class sweep: B*Cs problems p = b*Cs + c)
        cached, Cs = self._cached_supports(support_ims, B, dev)
        sweep = isinstance(support_ims, ClassSweep)
        NP = B * Cs
        if cached is None:
            sup_ims = self._support_batch(support_ims, B, way, shot)
            Ns = sup_ims.size(0)
        bridge, ctx = self._saving_ctx(("q_saved", "l4_saved", "s_saved", "heads"), align_only_for="fgn")
        self._ctx = None
        if cached is None:
            sup, sh_, sw_ = self._rcnn_base(sup_ims, plan, save=ctx["s_saved"] if ctx is not None else None,
                                            save_from=ctx["t"] if ctx is not None else 3)  # [Ns*400][1024]
            if (sh_, sw_) != (20, 20):
                raise RuntimeError("support images must be 320x320 (fgn.py:34-35: AvgPool2d(20) / AvgPool2d(14, 1) of a 20x20 map)")
            L = sh_ * sw_

        def mean_map(offset):  # mean over the shots [offset, offset + shot): [B][400*1024]
            m = torch.empty((B, L * 1024), dtype=torch.float32, device=dev)
            for b in range(B):
                m[b:b + 1] = ops.spatial_mean(sup.view(-1)[(b * way * shot + offset) * L * 1024:], 1, shot, L * 1024)
            return m

        if cached is None:
            pos_map = mean_map(0)
            pos_rpn = ops.spatial_mean(pos_map, B, L, 1024)            # AvgPool2d(20): [B][1024]
            pos_rcnn = ops.avgpool(pos_map, B, sh_, sw_, 1024, 14, 1)  # AvgPool2d(14, 1): [B][49][1024]
        else:
            pos_rpn, pos_rcnn = cached["pos_rpn"], None

        def attention_rpn_input(base, B_, fh, fw, plan_):
            if ctx is not None:
                ctx["base"] = base
            if sweep:  # problem p: image p / Cs's map times set p's vector (the map is never replicated)
                return ops.scale_rows_grouped(base, pos_rpn, fh * fw, 1024, Cs, NP), fh, fw
            return ops.scale_rows_by_group(base, pos_rpn, B_ * fh * fw, fh * fw, 1024), fh, fw

        st = self._stages(im_data, im_info, gt_boxes, rpn_input=attention_rpn_input, ctx=ctx, group=Cs)
        R, n_roi, pooled, fc7 = st["R"], st["n_roi"], st["pooled"], st["fc7"]
        wb, bb = self._w(self.RCNN_bbox_pred)
        bbox_pred = ops.gemm_nt(fc7, wb, n_roi, 4, 2048, shift=bb)
        w1 = self.cls_conv1.weight.detach()
        # torch.cat([support, roi], 1): support channels first (a cache holds the support half's output)
        w1_sup = ops.pack_conv_weight(w1[:, :1024].contiguous()) if cached is None else None
        w1_roi = ops.pack_conv_weight(w1[:, 1024:].contiguous())
        w2 = ops.pack_conv_weight(self.cls_conv2.weight)
        # Linear(1152, 2) reads the NCHW flatten (c, h, w); the activations here are (h, w, c)
        wl = self.RCNN_cls_score.weight.detach().view(2, 128, 9).permute(0, 2, 1).reshape(2, 1152).contiguous()
        bl = self.RCNN_cls_score.bias.detach().contiguous()
        roi_half, _, _ = ops.conv2d_nhwc(pooled, n_roi, 7, 7, 1024, w1_roi, 512, 3, 3, 1, 0)  # [n*25][512], shared

        def head(support, offset):  # support [B][49][1024]; cached: s_half [NP*25][512] from the cache
            saved = [] if ctx is not None else None
            if cached is None:
                s_half, _, _ = ops.conv2d_nhwc(support, B, 7, 7, 1024, w1_sup, 512, 3, 3, 1, 0)  # [B*25][512]
            else:
                s_half = cached["s_half"]
            x = ops.broadcast_rows(s_half, NP, R, 25 * 512)                                     # [n*25][512]
            ops.axpy_rows_(x, roi_half, n_roi * 25, 512)
            x1 = self._bn(x, n_roi * 25, self.bn1, save=saved)
            x, _, _ = ops.conv2d_nhwc(x1, n_roi, 5, 5, 512, w2, 128, 3, 3, 1, 0)                # [n*9][128]
            x2 = self._bn(x, n_roi * 9, self.bn2, save=saved)
            score = ops.gemm_nt(x2, wl, n_roi, 2, 1152, shift=bl)
            if ctx is not None:
                ctx["heads"].append(dict(offset=offset, support=support, x1=x1, x2=x2, bn1=saved[0], bn2=saved[1]))
            return ops.softmax_rows_(score.clone(), n_roi, 2), score

        cls_prob, cls_score = head(pos_rcnn, 0)
        RCNN_loss_cls = RCNN_loss_bbox = 0
        rois_label = st["rois_label"]
        if training:
            neg_prob, neg_score = head(ops.avgpool(mean_map(shot), B, sh_, sw_, 1024, 14, 1), shot)
            cls_prob = torch.cat([cls_prob, neg_prob], 0)
            rois_label = torch.cat([rois_label, torch.zeros_like(rois_label)], 0)
            rl, seeds = ops.rcnn_losses(cls_score, neg_score, st["labels_f"], bbox_pred, st["rois_target"].contiguous(),
                                        st["rois_inside_ws"].contiguous(), st["rois_outside_ws"].contiguous(),
                                        with_grad=ctx is not None)
            RCNN_loss_cls, RCNN_loss_bbox = rl[0], rl[1]
        rpn_loss_cls, rpn_loss_bbox = st["rpn_loss_cls"], st["rpn_loss_bbox"]
        if ctx is not None:
            ctx.update(loss_seeds=seeds, sup=sup, Ns=Ns, shot=shot, way=way, L=L, pos_rpn=pos_rpn, pooled=pooled,
                       w1_sup=w1_sup, w1_roi=w1_roi, w2=w2, wl=wl)
            self._ctx = ctx
            if bridge:  # loss.backward() (train.py:141-143) runs self._backward on the HIP kernels
                rpn_loss_cls, rpn_loss_bbox, RCNN_loss_cls, RCNN_loss_bbox = self._loss_bridge(
                    dev, (rpn_loss_cls, rpn_loss_bbox, RCNN_loss_cls, RCNN_loss_bbox))
        return (st["rois"], cls_prob, bbox_pred, rpn_loss_cls, rpn_loss_bbox, RCNN_loss_cls, RCNN_loss_bbox, rois_label)

    # ---- training backward ---------------------------------------------------------------------------------------------
    # fgn.py:29-41: the relation head's two convs and their (trainable) BatchNorms
    _head_params = BW.lin("RCNN_cls_score") + ["cls_conv2.weight", "cls_conv1.weight"] + BW.lin("bn2") + BW.lin("bn1")

    def _relation_head_backward(self, ctx, grads, g3, gs):
        """Adjoint of both `head` calls of the forward (fgn.py:145-165): Linear <- ReLU/BN2 <- conv2 <- ReLU/BN1 <- (support
        half + roi half) of conv1; bn1 / bn2 are ORDINARY BatchNorms in train mode: their adjoint goes through the batch
        statistics. The support halves go into gs (d support trunk output); -> d pooled [n_roi*49][1024] through the roi half.
        gs None (a frozen trunk, ctx["t"] == 3): the data gradients of conv1's two halves have no reader and are not run -> None"""
        d_pos, d_neg, _ = ctx["loss_seeds"]
        B, R, lin_c, wl = ctx["B"], ctx["R"], self.RCNN_cls_score, ctx["wl"]
        n_roi, dev = B * R, ctx["pooled"].device
        for bn_ in (self.bn1, self.bn2):
            for p_ in (bn_.weight, bn_.bias):
                if p_.grad is None:
                    p_.grad = torch.zeros_like(p_)
        c2 = dict(cin=512, cout=128, k=3, stride=1, pad=0, w=ctx["w2"], scale=None, u=None)
        d_roi_half = torch.zeros((n_roi * 25, 512), dtype=torch.float32, device=dev)
        w1g = self.cls_conv1.weight

        def acc_w1_half(packed, lo):  # packed [512][3*3*1024] -> cls_conv1.weight.grad[:, lo:lo+1024] (OIHW)
            tmp = torch.empty((512, 1024, 3, 3), dtype=torch.float32, device=dev)
            ops.unpack_conv_weight_grad(packed, tmp, 512, 1024, 3, 3, accumulate=False)
            if w1g.grad is None:
                w1g.grad = torch.zeros_like(w1g)
            w1g.grad[:, lo:lo + 1024].add_(tmp)

        for hc in ctx["heads"]:
            ds = d_pos if hc["offset"] == 0 else d_neg
            dwl = ops.gemm_small(ds, (1, 2), hc["x2"], (1152, 1), 2, 1152, n_roi, alpha=g3)   # [2][(h,w,c)]
            BW.acc(lin_c.weight, dwl.view(2, 9, 128).permute(0, 2, 1).reshape(2, 1152))          # -> the NCHW flatten (c,h,w)
            BW.acc(lin_c.bias, ops.colsum(ds, n_roi, 2, alpha=g3))
            d_x2 = ops.gemm_small(ds, (2, 1), wl, (1152, 1), n_roi, 1152, 2, alpha=g3).view(n_roi * 9, 128)
            ops.relu_mask_(d_x2, hc["x2"], n_roi * 9, 128)
            x2_pre, m2, v2 = hc["bn2"]
            d_x2pre = ops.bn_train_backward(d_x2, x2_pre, m2, v2, self.bn2.weight, self.bn2.eps, n_roi * 9, 128,
                                            self.bn2.weight.grad, self.bn2.bias.grad)
            grads.add_conv("cls_conv2", d_x2pre, hc["x1"], n_roi, 5, 5, c2)
            d_x1 = BW.conv_dgrad(d_x2pre, n_roi, 5, 5, c2, mask=hc["x1"])  # (+ the ReLU adjoint of bn1's output)
            x1_pre, m1, v1 = hc["bn1"]
            d_x1pre = ops.bn_train_backward(d_x1, x1_pre, m1, v1, self.bn1.weight, self.bn1.eps, n_roi * 25, 512,
                                            self.bn1.weight.grad, self.bn1.bias.grad)
            ops.axpy_rows_(d_roi_half, d_x1pre, n_roi * 25, 512)
            d_s_half = ops.spatial_mean(d_x1pre, B, R, 25 * 512)  # broadcast over the image's R rois: sum = R * mean
            d_s_half.mul_(float(R))
            acc_w1_half(ops.conv2d_wgrad(d_s_half, hc["support"], B, 7, 7, 1024, 512, 3, 3, 1, 0), 0)
            if gs is not None:
                d_support = ops.conv2d_dgrad(d_s_half, ctx["w1_sup"], B, 7, 7, 1024, 512, 3, 3, 1, 0)  # [B*49][1024]
                BW.shot_mean_backward(gs, ops.avgpool_backward(d_support, B, 20, 20, 1024, 14, 1), ctx, hc["offset"])  # 14, 1
        acc_w1_half(ops.conv2d_wgrad(d_roi_half, ctx["pooled"], n_roi, 7, 7, 1024, 512, 3, 3, 1, 0), 1024)
        if gs is None:
            return None
        return ops.conv2d_dgrad(d_roi_half, ctx["w1_roi"], n_roi, 7, 7, 1024, 512, 3, 3, 1, 0)

    def _backward(self, ctx, g, grads):
        """frcnn's adjoint with the relation head in place of the plain RCNN_cls_score and the channel re-weighting in front
        of the RPN; the supports are differentiated through the trunk (where it trains: ctx["t"] < 3)"""
        g1, g2, g3, g4, g_dev = g
        B, n_roi, hw, L, d_bbox = ctx["B"], ctx["B"] * ctx["R"], ctx["fh"] * ctx["fw"], ctx["L"], ctx["loss_seeds"][2]
        d_fc7 = BW.seed_linear_dx(self.RCNN_bbox_pred, d_bbox, g4)
        trunk = ctx["t"] < 3
        gs = None
        if trunk:
            gs = torch.zeros((ctx["Ns"] * L, 1024), dtype=torch.float32, device=d_fc7.device)  # d(support trunk output)
        d_pooled_head = self._relation_head_backward(ctx, grads, g3, gs)
        BW.seed_linear_grads(self.RCNN_bbox_pred, d_bbox, ctx["fc7"], g4)
        d_pooled = BW.layer4_backward(d_fc7, n_roi, ctx["l4_saved"], grads, need_dx=trunk)
        grads.finish_all(self, "RCNN_top")
        grads.finish_all(self, "cls_conv2")
        if trunk:
            ops.axpy_rows_(d_pooled, d_pooled_head, n_roi * 49, 1024)  # the pooled features also feed the head's roi half
        BW.ready(self, self._grad_stages(ctx["plan"], ctx["t"])[0][1])
        d_bf = BW.roi_features_backward(ctx, d_pooled) if trunk else None
        d_rfeat = BW.sibling_rpn_backward(self, ctx, g1, g2, g_dev, grads)
        if not trunk:  # frozen trunk: base_feat, the channel weights and the support maps have no trainable producer
            grads.finish_all(self, "RCNN_rpn")
            BW.ready(self, BW.RPN_PARAMS)
            BW.trunk_backward(self, ctx, grads, None)
            return
        # the RPN ran on base_feat * pos_rpn[image] (fgn.py:75-82): d base = d rfeat * pos_rpn + RoIAlign path, and
        # d pos_rpn[image] = sum over the pixels of d rfeat * base -> AvgPool2d(20) -> the positive supports' mean map
        gq = ops.scale_rows_by_group(d_rfeat, ctx["pos_rpn"], B * hw, hw, 1024)
        ops.axpy_rows_(gq, d_bf, B * hw, 1024)
        d_pos_rpn = (d_rfeat * ctx["base"]).view(B, hw, 1024).sum(1).contiguous()
        BW.shot_mean_backward(gs, ops.broadcast_rows(d_pos_rpn, B, L, 1024, alpha=1.0 / L).view(B, L, 1024), ctx, 0)
        grads.finish_all(self, "RCNN_rpn")
        BW.ready(self, BW.RPN_PARAMS)
        BW.trunk_backward(self, ctx, grads, gq, gs)
