"""Attention maps of a synthetic episode, written out; or (--time) what they cost.

    python tools/attention_maps.py [--out DIR] [--height 192 --width 256 --shot 2]
        runs `model.attention_maps` on a seeded synthetic episode (test-profile weights, BA block on; the boxes are the
        episode's three ground-truth boxes) and writes ba.npy, rpn.npy, roi.npy and the overlays of `attention.render` as
        binary PPM files (P6): ba_s<shot>.ppm, rpn_box<j>_s<shot>.ppm, roi_box<j>_s<shot>.ppm. No image library needed.

    python tools/attention_maps.py --time [--json result.json]
        600 x 1000 query, shot 3, 20 boxes, B = 1: one `attention_maps` call against (a) an eval forward of the same inputs
        and (b) the host-side way to the same maps -- the same staged forward, then the attention tensors pulled to the host
        and reduced per box with numpy. All three in one process, alternating, each call bracketed by a device synchronise
        (host clock); 10 warm-up calls of each, then blocks of alternating rounds; a block's figure is the median of its
        calls, the spread that of the block medians (the method of profiles/merge_detections.md). Also: the C-ABI
        launches of a call and of a forward, and the box-mean launch alone (device events around back-to-back launches).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import dana_amd  # noqa: E402
from dana_amd import attention, ops, synthetic as S  # noqa: E402
from dana_amd._lib import lib  # noqa: E402
from dana_amd.config import cfg  # noqa: E402


def build(dev, shot):
    m = dana_amd.get_model("DAnA", pretrained=False, use_BA_block=True, way=1, shot=shot, classes=["fg", "bg"])
    m.load_state_dict(S.fill_state_dict(m.state_dict(), seed=11, profile="test"))
    return m.to(dev).eval()


def write_ppm(path, rgb):
    """rgb: uint8 [h][w][3] numpy array -> binary PPM"""
    h, w, _ = rgb.shape
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h))
        f.write(np.ascontiguousarray(rgb).tobytes())


def write_maps(a, dev):
    m = build(dev, a.shot)
    im, info, gt, nb, sup = [t.to(dev) for t in S.episode_inputs(1, 1, a.shot, a.height, a.width, seed=5)]
    boxes = gt[:, :3, :4].contiguous()
    with torch.no_grad():
        maps = m.attention_maps(im, info, boxes, sup)
        n = boxes.size(1)
        per_box = sup[0][None].expand(n, a.shot, 3, sup.size(-2), sup.size(-1)).contiguous()
        over = dict(ba=attention.render(maps.ba[0], sup[0], a.alpha), rpn=attention.render(maps.rpn[0], per_box, a.alpha),
                    roi=attention.render(maps.roi[0], per_box, a.alpha))
    os.makedirs(a.out, exist_ok=True)
    for name in ("ba", "rpn", "roi"):
        np.save(os.path.join(a.out, name + ".npy"), getattr(maps, name).cpu().numpy())
    for s in range(a.shot):
        write_ppm(os.path.join(a.out, "ba_s%d.ppm" % s), over["ba"][s].cpu().numpy())
        for j in range(n):
            write_ppm(os.path.join(a.out, "rpn_box%d_s%d.ppm" % (j, s)), over["rpn"][j, s].cpu().numpy())
            write_ppm(os.path.join(a.out, "roi_box%d_s%d.ppm" % (j, s)), over["roi"][j, s].cpu().numpy())
    print("wrote ba.npy %s, rpn.npy %s, roi.npy %s and %d overlays to %s"
          % (tuple(maps.ba.shape), tuple(maps.rpn.shape), tuple(maps.roi.shape), a.shot * (1 + 2 * n), a.out))


def host_pull(m, im, info, boxes, sup):
    """the maps without the box-mean kernel: the same staged forward up to the attention tensors, then both pulled to the
    host and reduced there (rpn: numpy mean over the box's cell rows; roi: over each box's 49 rows)"""
    with torch.no_grad():
        f = m._forward_setup(im, info, boxes, sup)
        f.maps = {}
        corr, (fh, fw), s = m._trunks(f, im, sup)
        m._rpn_attention(f, corr, fh, fw, s)
        m._roi_support(f, s)
        n, NP, P = boxes.size(1), f.NP, cfg.POOLING_SIZE
        rois = torch.cat([torch.zeros((NP, n, 1), device=f.dev), boxes], 2).contiguous()
        pooled, q_pe = m._roi_pool(f.plan, corr, f.B, fh, fw, 2048, rois, pe=False, group=1)
        f.main.wait_event(s["roi_done"])
        q2, qld, _ = m._roi_query(f, pooled, q_pe, True, NP * n)
        sc2 = m._roi_scores(f, q2, qld, s["k2"].view(-1), s["un2"].view(-1), n)
        w_rpn, w_roi, bx = f.maps["rpn_w"].cpu().numpy(), sc2.cpu().numpy(), boxes.cpu().numpy()
    L, K2 = s["map"][0] * s["map"][1], f.shot * P * P
    rpn = np.empty((NP, n, f.shot * L), dtype=np.float32)
    for j in range(n):
        x_lo, y_lo, x_hi, y_hi = attention.cell_rect(bx[0, j], fh, fw)
        rows = (np.arange(y_lo, y_hi + 1)[:, None] * fw + np.arange(x_lo, x_hi + 1)[None, :]).reshape(-1)
        rpn[:, j] = w_rpn[:, rows].mean(1, dtype=np.float64)
    roi = w_roi[:, :, :K2].reshape(NP, n, P * P, K2).mean(2, dtype=np.float64).astype(np.float32)
    return rpn, roi


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def count_launches(fn):
    """entry-point calls of libdana_hip.so during fn() (torch's own few small launches are not in it)"""
    L, n = lib(), [0]
    orig = L.call

    def counting(name, *args):
        n[0] += 1
        return orig(name, *args)

    L.call = counting
    try:
        fn()
    finally:
        del L.call
    return n[0]


def time_maps(a, dev):
    shot, n = 3, 20
    m = build(dev, shot)
    im, info, gt, nb, sup = [t.to(dev) for t in S.episode_inputs(1, 1, shot, 600, 1000, seed=5)]
    rng = np.random.RandomState(7)
    wh = rng.uniform(64, 400, size=(n, 2))
    xy = rng.uniform(0, 1, size=(n, 2)) * (np.array([999.0, 599.0]) - wh)
    boxes = torch.from_numpy(np.concatenate((xy, xy + wh), 1).astype(np.float32))[None].to(dev)
    ways = dict(attention_maps=lambda: m.attention_maps(im, info, boxes, sup),
                eval_forward=lambda: m(im, info, gt, nb, sup),
                host_pull=lambda: host_pull(m, im, info, boxes, sup))
    with torch.no_grad():
        maps = ways["attention_maps"]()
        rpn_h, roi_h = ways["host_pull"]()
        agree = (float(np.abs(maps.rpn.cpu().numpy().reshape(rpn_h.shape) - rpn_h).max() / rpn_h.max()),
                 float(np.abs(maps.roi.cpu().numpy().reshape(roi_h.shape) - roi_h).max() / roi_h.max()))
        for _ in range(10):
            for fn in ways.values():
                fn()
        blocks = []
        for _ in range(a.blocks):
            t = {k: [] for k in ways}
            for _ in range(a.rounds):
                for k, fn in ways.items():
                    t[k].append(timed(fn))
            blocks.append({k: dict(median=float(np.median(v)), min=float(np.min(v)), p90=float(np.percentile(v, 90)))
                           for k, v in t.items()})
        launches = {k: count_launches(ways[k]) for k in ("attention_maps", "eval_forward")}
        # the box-mean launch alone, on the weights of one more staged pass
        f = m._forward_setup(im, info, boxes, sup)
        f.maps = {}
        corr, (fh, fw), s = m._trunks(f, im, sup)
        m._rpn_attention(f, corr, fh, fw, s)
        w = f.maps["rpn_w"]
        reps = 200
        for _ in range(10):
            ops.attn_box_mean(w, boxes, n, fh, fw)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            ops.attn_box_mean(w, boxes, n, fh, fw)
        e1.record()
        torch.cuda.synchronize()
        box_us = e0.elapsed_time(e1) * 1e3 / reps
    rects = [attention.cell_rect(b, fh, fw) for b in boxes[0].cpu().tolist()]
    rows = [(r[2] - r[0] + 1) * (r[3] - r[1] + 1) for r in rects]
    read_bytes = 4.0 * w.size(2) * sum(rows)
    summary = {k: dict(median=float(np.median([b[k]["median"] for b in blocks])),
                       lo=float(np.min([b[k]["median"] for b in blocks])), hi=float(np.max([b[k]["median"] for b in blocks])))
               for k in ways}
    res = dict(shape=dict(query=[600, 1000], grid=[fh, fw], shot=shot, boxes=n, rows_per_box=rows, K=int(w.size(2)),
                          attention_tensor_bytes=int(w.numel() * 4)),
               host_pull_agrees=dict(rpn=agree[0], roi=agree[1]), ms=summary, blocks=blocks, rounds_per_block=a.rounds,
               c_abi_launches=launches,
               box_mean=dict(us_per_launch=box_us, rows_read=int(sum(rows)), bytes_read=read_bytes,
                             gb_per_s=read_bytes / (box_us * 1e-6) / 1e9,
                             workgroups=n * ((int(w.size(2)) + 255) // 256), longest_row_walk=int(max(rows))),
               device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fjson:
            fjson.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="attention_maps_out")
    ap.add_argument("--height", type=int, default=192)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--shot", type=int, default=2)
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=20, help="alternating rounds of the three ways per block")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool runs on the device only")
    dev = torch.device("cuda:0")
    if a.time:
        time_maps(a, dev)
    else:
        write_maps(a, dev)


if __name__ == "__main__":
    main()
