"""Flip and multi-scale testing of a synthetic image pool, as prediction sheets; or (--time) what the view ensemble costs.

    python tools/view_ensemble.py [--out DIR] [--images 2 --height 192 --width 256 --scales 160,192,224 --shot 2 --classes 2]
        builds a seeded pool of random frames with their flipped twins, plans the views (`pipeline.plan_views`), assembles
        them (`EpisodeAssembler`), sweeps every view against every cached class, and merges the views on the device
        (`postprocess.ensemble_views`, linear Soft-NMS with box voting). Writes views_<i>.png per image: the merged boxes on
        the image's first view (unmirrored, first scale), the classes' shots beside it; and single_<i>.png, the same sheet
        from that one view alone. No image library is involved.

    python tools/view_ensemble.py --time [--json result.json]
        (a) the fold alone and the whole `ensemble_views` on synthetic lists (4 images x 6 views x 3 classes, 300 rows per
            list), each the median of 50 calls between a pair of device events after 10 warm-up calls, against the host
            route it replaces: one D2H read of the lists, `fold_views_numpy`, one upload, `merge_detections` (median of 5,
            host clock around a device synchronise);
        (b) one 375 x 500 frame through assemble + sweep + detections_by_class + ensemble_views with V = 1, 2, 6 views
            (scales 600 | 600 with flip | 480, 600, 720 with flip) in ONE batch of V view images, against V separate B = 1
            batches of the same views, each merged the same way (median of 7 after 2 warm-up runs, host clock around a
            device synchronise). Every view of a batch is a holder of the LARGEST view's size, so the batched form runs
            the trunk over padding the separate form does not see.
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
from dana_amd import pipeline as PL, postprocess as PP, render, synthetic as S  # noqa: E402


def make_pool(dev, n, h, w, seed=3):
    """n random frames, each followed by nothing; then their n flipped twins -> (pool, [(row, twin)])"""
    rng = np.random.RandomState(seed)
    pool = PL.ImagePool(dev)
    for _ in range(n):
        pool.add(rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8), [])
    pairs = [(r, pool.add_flipped(r, [])) for r in range(n)]
    return pool.freeze(), pairs


def model_and_cache(dev, shot, classes):
    m = dana_amd.get_model("DAnA", pretrained=False, use_BA_block=True, way=1, shot=shot, classes=["fg", "bg"])
    m.load_state_dict(S.fill_state_dict(m.state_dict(), seed=11, profile="test"))
    m.to(dev).eval()
    sup = S.episode_inputs(classes, 1, shot, 128, 160, seed=7)[4].to(dev)  # [classes, shot, 3, 320, 320]
    sets = sup.reshape(classes, -1, 3, sup.size(-2), sup.size(-1))
    with torch.no_grad():
        cache = m.encode_supports(sets)
    return m, cache, sets


def holders_for(plan, dev):
    return PL.EpisodeHolders(plan.batch, 1, 0, plan.holder_hw[0], plan.holder_hw[1], dev, max_num_box=4)


def detect_views(m, cache, asm, plan, views, **kw):
    im_data, im_info, gt, nb = asm.assemble(plan)[:4]
    with torch.no_grad():
        rois, cls_prob, bbox_pred = m(im_data, im_info, gt, nb, cache.sweep())[:3]
    cd = PP.detections_by_class(rois, cls_prob, bbox_pred, im_info, len(cache), with_layout=True, nms_thresh=None)
    return PP.ensemble_views(cd, views, **kw), im_data, im_info


def write_sheets(a, dev):
    scales = tuple(int(s) for s in a.scales.split(","))
    pool, pairs = make_pool(dev, a.images, a.height, a.width)
    m, cache, sets = model_and_cache(dev, a.shot, a.classes)
    shots = sets.reshape(1, -1, 3, sets.size(-2), sets.size(-1)).expand(a.images, -1, -1, -1, -1).contiguous()
    kw = dict(method="linear", vote_thresh=0.8)
    os.makedirs(a.out, exist_ok=True)
    totals = {}
    for name, sc, flip, rows in (("views", scales, True, pairs), ("single", scales[:1], False, [r for r, _ in pairs])):
        plan, views = PL.plan_views(pool, rows, scales=sc, flip=flip)
        asm = PL.EpisodeAssembler(pool, holders_for(plan, dev))
        dets, im_data, im_info = detect_views(m, cache, asm, plan, views, **kw)
        first = torch.arange(a.images, device=dev) * views.views  # view 0 of every image: as stored, the first scale
        sheet = render.prediction_sheet(im_data[first].contiguous(), im_info[first].contiguous(), dets, shots,
                                        thickness=a.thickness, side=min(a.side, plan.holder_hw[0]))
        for i in range(a.images):
            render.write_png(os.path.join(a.out, "%s_%d.png" % (name, i)), sheet[i])
        totals[name] = (views.views, dets.counts.tolist())
    print("wrote %d x 2 sheets to %s: %d views per image -> %s boxes per (image, class); one view -> %s"
          % (a.images, a.out, totals["views"][0], totals["views"][1], totals["single"][1]))


def event_median(fn, reps=50, warm=10):
    """median over `reps` calls of the device time between two events around one call, in microseconds"""
    for _ in range(warm):
        fn()
    pairs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    t = [e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs]
    return dict(median_us=float(np.median(t)), min_us=float(np.min(t)), p90_us=float(np.percentile(t, 90)))


def host_median(fn, reps=5, warm=1):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(t)), min_ms=float(np.min(t)), max_ms=float(np.max(t)))


def synthetic_lists(B, V, Cn, R, fw, fh, seed=5):
    """B * V * Cn lists of R rows around 8 objects per (image, class), odd views mirrored beforehand; a tenth of the rows
    lies outside the frame -> (ClassDetections-like, table)"""
    rng = np.random.RandomState(seed)
    lists, table = [], np.zeros((B * V, 5), np.float32)
    for i in range(B):
        centres = rng.uniform(0.15, 0.85, size=(Cn, 8, 2)) * (fw, fh)
        for v in range(V):
            table[i * V + v] = (fw, fh, v % 2, -np.inf, np.inf)
            for c in range(Cn):
                k = rng.randint(0, 8, R)
                wh = rng.uniform(30, 120, size=(R, 2))
                xy = centres[c, k] + rng.normal(0, 6, size=(R, 2)) - wh / 2
                xy[rng.uniform(size=R) < 0.1] += (fw, 0)
                d = np.concatenate((xy, xy + wh, np.sort(rng.uniform(0.05, 1, (R, 1)), 0)[::-1]), 1).astype(np.float32)
                if v % 2:
                    d[:, 0], d[:, 2] = np.float32(fw - 1) - d[:, 2], np.float32(fw - 1) - d[:, 0]
                lists.append(d)
    return lists, table


def time_fold(dev):
    B, V, Cn, R, fw, fh = 4, 6, 3, 300, 1000.0, 600.0
    lists, table = synthetic_lists(B, V, Cn, R, fw, fh)
    counts = np.full(B * V * Cn, R, np.int32)
    offsets = (np.arange(B * V * Cn + 1) * R).astype(np.int32)
    cd = PP.ClassDetections([[None] * Cn for _ in range(B * V)])
    cd.packed = torch.from_numpy(np.concatenate(lists, 0)).to(dev)
    cd.counts, cd.offsets, cd.num_classes = torch.from_numpy(counts), torch.from_numpy(offsets), Cn
    cd.layout_dev = torch.from_numpy(np.concatenate((counts, offsets))).to(dev)
    views = PL.ViewSet(B, V, table, np.ones(B * V), np.zeros(B * V))
    kw = dict(method="linear", vote_thresh=0.8)

    def host_route():
        host = cd.packed.cpu().numpy()
        f = PP.fold_views_numpy([host[offsets[p]:offsets[p + 1]] for p in range(len(counts))], table, V, Cn)
        c = f["counts"]
        o = np.concatenate(([0], np.cumsum(c))).astype(np.int32)
        packed = torch.from_numpy(np.concatenate(f["dets"], 0)).to(dev)
        return PP.merge_detections((packed, torch.from_numpy(c), torch.from_numpy(o)), V, with_layout=True, **kw)

    dev_m, host_m = PP.ensemble_views(cd, views, **kw), host_route()
    same = bool(torch.equal(dev_m.counts, host_m.counts) and torch.equal(dev_m.packed[:dev_m.total], host_m.packed[:host_m.total]))
    kept = int(PP.fold_views(cd, views).counts.sum())
    return dict(shape=dict(images=B, views=V, classes=Cn, rows_per_list=R, rows=int(counts.sum()), rows_kept_by_fold=kept,
                           rows_out=dev_m.total),
                fold_views_us=event_median(lambda: PP.fold_views(cd, views)),
                merge_after_fold_us=event_median(lambda f=PP.fold_views(cd, views): PP.merge_detections(
                    f, V, with_layout=True, capacity=f.capacity, **kw), reps=20, warm=3),
                ensemble_views_ms=host_median(lambda: PP.ensemble_views(cd, views, **kw), reps=20, warm=3),
                host_route_ms=host_median(host_route),
                host_fold_only_ms=host_median(lambda: PP.fold_views_numpy(lists, table, V, Cn)),
                device_equals_host_route=same)


def time_end_to_end(dev, shot=2, classes=3):
    pool, pairs = make_pool(dev, 1, 375, 500)
    m, cache, _ = model_and_cache(dev, shot, classes)
    kw = dict(method="linear", vote_thresh=0.8)
    out = {}
    for name, scales, flip in (("V1", (600,), False), ("V2", (600,), True), ("V6", (480, 600, 720), True)):
        rows = pairs if flip else [pairs[0][0]]
        plan, views = PL.plan_views(pool, rows, scales=scales, flip=flip)
        asm = PL.EpisodeAssembler(pool, holders_for(plan, dev))
        # the same views one by one: a B = 1 batch each, in a holder of its own size, folded and merged together afterwards
        singles = []
        for q, t in zip(plan.queries, views.table):
            row = q["row"]
            p1, v1 = PL.plan_views(pool, [row], scales=(q["im_scale"] * min(pool.meta[row, 0], pool.meta[row, 1]),))
            singles.append((p1, PL.EpisodeAssembler(pool, holders_for(p1, dev))))

        def batched():
            return detect_views(m, cache, asm, plan, views, **kw)[0]

        def separate():
            cds = []
            for p1, a1 in singles:
                im_data, im_info, gt, nb = a1.assemble(p1)[:4]
                with torch.no_grad():
                    rois, cls_prob, bbox_pred = m(im_data, im_info, gt, nb, cache.sweep())[:3]
                cds.append(PP.detections_by_class(rois, cls_prob, bbox_pred, im_info, classes, with_layout=True, nms_thresh=None))
            packed = torch.cat([c.packed[:int(c.offsets[-1])] for c in cds], 0)
            counts = torch.cat([c.counts for c in cds])
            offsets = torch.cat((torch.zeros(1, dtype=torch.int32), torch.cumsum(counts, 0).to(torch.int32)))
            cd = PP.ClassDetections([c[0] for c in cds])
            cd.packed, cd.counts, cd.offsets, cd.num_classes = packed, counts, offsets, classes
            return PP.ensemble_views(cd, views, **kw)

        out[name] = dict(views=views.views, holder_hw=list(plan.holder_hw),
                         view_sizes=[[q["oh"], q["ow"]] for q in plan.queries],
                         batched_ms=host_median(batched, reps=7, warm=2), separate_ms=host_median(separate, reps=7, warm=2),
                         boxes_batched=batched().counts.tolist(), boxes_separate=separate().counts.tolist())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="view_ensemble_out")
    ap.add_argument("--images", type=int, default=2)
    ap.add_argument("--height", type=int, default=192)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--scales", default="160,192,224", help="comma-separated target sizes of the shorter side")
    ap.add_argument("--shot", type=int, default=2)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--side", type=int, default=96, help="side of a support shot on the sheet")
    ap.add_argument("--thickness", type=int, default=2)
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool runs on the device only")
    dev = torch.device("cuda:0")
    if not a.time:
        return write_sheets(a, dev)
    res = dict(fold=time_fold(dev), end_to_end=time_end_to_end(dev), device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
