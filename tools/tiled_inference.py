"""Tiled inference of a synthetic image pool, as prediction sheets with per-stage times; or (--time) what the tile fold costs.

    python tools/tiled_inference.py [--out DIR] [--images 1 --height 384 --width 512 --grid 2,2 --scale 384 --full 192
                                     --overlap 32 --margin 4 --shot 2 --classes 2]
        builds a seeded pool of random frames with their flipped twins, plans the tiles (`pipeline.plan_tiles`: a full-frame
        view, then grid tiles of the frame prepared at --scale, each also mirrored), assembles them (`EpisodeAssembler`),
        sweeps every view against every cached class, and merges on the device (`postprocess.ensemble_views`, linear
        Soft-NMS with box voting). Writes tiles_<i>.png per image: the merged boxes on the image's full-frame view, the
        classes' shots beside it. Prints one JSON line with, per stage, the GPU-side stretch between two device events and
        the host clock around the stage with a device synchronise after it (median of --reps runs after 2 warm-up runs).
        One sweep runs the RoI head over images x views x classes x 300 rois and its operands must stay below 2 GiB (about
        10 000 rois): with more frames, sweep them in batches of their own.

    python tools/tiled_inference.py --time [--json result.json] [--fold-only]
        `fold_tiles` next to `fold_views` on the SAME lists and layout (B = 2 frames of 1500 x 2000, a 2 x 2 grid at scale
        1200 with flipped twins and a full-frame view: V = 10; C = 20 classes, 300 rows per list), alternating in blocks in
        one process: the median of 50 calls between a pair of device events per block, 5 blocks each; then the whole
        `ensemble_views` (method="hard") with the TileSet and with a plain ViewSet of the same table's first five columns
        (host clock around a device synchronise). The view fold is unchanged code and serves as the yardstick.
        --fold-only stops after the folds: the form to run under a kernel tracer.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dana_amd import pipeline as PL, postprocess as PP, render  # noqa: E402
from view_ensemble import event_median, holders_for, host_median, make_pool, model_and_cache  # noqa: E402


def staged(stages, reps, warm=2):
    """run the chain of (name, key, fn(state) -> state[key]) `warm + reps` times -> per stage the median GPU-side stretch
    (device events around the stage) and host time (clock around the stage, a device synchronise after it), and the last
    state"""
    gpu, host = {n: [] for n, _, _ in stages}, {n: [] for n, _, _ in stages}
    state = {}
    for it in range(warm + reps):
        state = {}
        for name, key, fn in stages:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            state[key] = fn(state)
            e1.record()
            torch.cuda.synchronize()
            if it >= warm:
                host[name].append((time.perf_counter() - t0) * 1e3)
                gpu[name].append(e0.elapsed_time(e1))
    return {n: dict(gpu_ms=float(np.median(gpu[n])), host_ms=float(np.median(host[n]))) for n, _, _ in stages}, state


def write_sheets(a, dev):
    grid = tuple(int(g) for g in a.grid.split(","))
    pool, pairs = make_pool(dev, a.images, a.height, a.width)
    m, cache, sets = model_and_cache(dev, a.shot, a.classes)
    shots = sets.reshape(1, -1, 3, sets.size(-2), sets.size(-1)).expand(a.images, -1, -1, -1, -1).contiguous()
    kw = dict(grid=grid, scale=a.scale, overlap=a.overlap, margin=a.margin, flip=True, full_frame=a.full)
    plan, tiles = PL.plan_tiles(pool, pairs, **kw)
    asm = PL.EpisodeAssembler(pool, holders_for(plan, dev))
    if tiles.views * 300 > 3072:
        print("note: %d views of up to 300 rois: a class may exceed the soft merge's 3072 rows" % tiles.views, file=sys.stderr)
    if plan.batch * a.classes * 300 > 10000:
        raise SystemExit("%d view images x %d classes x 300 rois in one sweep: the RoI head's operands would pass 2 GiB; use fewer "
                         "--images per run" % (plan.batch, a.classes))

    first = torch.arange(a.images, device=dev) * tiles.views  # view 0 of every image: the full frame, as stored

    def forward(s):
        with torch.no_grad():
            return m(*s["inputs"], cache.sweep())[:3]

    stages = [  # (name, key of the state it fills, function of the state)
        ("plan_tiles (host only)", "plan", lambda s: PL.plan_tiles(pool, pairs, **kw)),
        ("assemble", "inputs", lambda s: asm.assemble(s["plan"][0])[:4]),
        ("sweep forward", "outputs", forward),
        ("detections_by_class", "cd", lambda s: PP.detections_by_class(*s["outputs"], s["inputs"][1], len(cache), with_layout=True,
                                                                       nms_thresh=None)),
        ("ensemble_views", "dets", lambda s: PP.ensemble_views(s["cd"], s["plan"][1], method="linear", vote_thresh=0.8)),
        ("prediction_sheet", "sheet", lambda s: render.prediction_sheet(
            s["inputs"][0][first].contiguous(), s["inputs"][1][first].contiguous(), s["dets"], shots, thickness=a.thickness,
            side=min(a.side, plan.holder_hw[0]))),
    ]
    times, state = staged(stages, a.reps)
    dets, sheet = state["dets"], state["sheet"]
    os.makedirs(a.out, exist_ok=True)
    for i in range(a.images):
        render.write_png(os.path.join(a.out, "tiles_%d.png" % i), sheet[i])
    folded = dets.folded.counts.cpu().numpy().reshape(a.images * a.classes, tiles.views)
    print(json.dumps(dict(
        frames=[a.height, a.width], views_per_image=tiles.views, holder_hw=list(plan.holder_hw),
        view_sizes=tiles.windows[:tiles.views, 2:].tolist(), rows_in=int(state["cd"].counts.sum()),
        rows_kept_by_fold_per_view=folded.sum(0).tolist(), rows_out_per_list=dets.counts.tolist(), stages=times,
        sheets=a.out, device=torch.cuda.get_device_name(0))))


def tile_lists(tiles, Cn, R, seed=5):
    """per view of `tiles` and class, R rows around 8 objects per (image, class) of the frame, expressed in the VIEW's own
    coordinates (mirrored first when the view is, then shifted by its offset), wherever they fall: most lie beyond a tile,
    some are cut by its seams -> host lists in problem order"""
    rng = np.random.RandomState(seed)
    lists, V = [], tiles.views
    for i in range(tiles.n_images):
        fw, fh = float(tiles.table[i * V, 0]), float(tiles.table[i * V, 1])
        centres = rng.uniform(0.1, 0.9, size=(Cn, 8, 2)) * (fw, fh)
        for v in range(V):
            t = tiles.table[i * V + v]
            for c in range(Cn):
                k = rng.randint(0, 8, R)
                wh = rng.uniform(30, 120, size=(R, 2))
                xy = centres[c, k] + rng.normal(0, 6, size=(R, 2)) - wh / 2
                d = np.concatenate((xy, xy + wh, np.sort(rng.uniform(0.05, 1, (R, 1)), 0)[::-1]), 1).astype(np.float32)
                if t[2]:
                    d[:, 0], d[:, 2] = np.float32(fw - 1) - d[:, 2], np.float32(fw - 1) - d[:, 0]
                d[:, [0, 2]] -= t[5]
                d[:, [1, 3]] -= t[6]
                lists.append(d)
    return lists


def time_folds(dev, fold_only):
    B, Cn, R = 2, 20, 300
    pool = PL.ImagePool()
    for _ in range(B):
        pool.add(np.zeros((1500, 2000, 3), np.uint8), [])
    pairs = [(r, pool.add_flipped(r, [])) for r in range(B)]
    _, tiles = PL.plan_tiles(pool.freeze(), pairs, grid=(2, 2), scale=1200, overlap=64, margin=4, flip=True, full_frame=600)
    V = tiles.views
    views = PL.ViewSet(B, V, tiles.table[:, :5], tiles.scales, tiles.rows)  # the same lists read as plain views
    lists = tile_lists(tiles, Cn, R)
    counts = np.full(B * V * Cn, R, np.int32)
    offsets = (np.arange(B * V * Cn + 1) * R).astype(np.int32)
    cd = PP.ClassDetections([[None] * Cn for _ in range(B * V)])
    cd.packed = torch.from_numpy(np.concatenate(lists, 0)).to(dev)
    cd.counts, cd.offsets, cd.num_classes = torch.from_numpy(counts), torch.from_numpy(offsets), Cn
    cd.layout_dev = torch.from_numpy(np.concatenate((counts, offsets))).to(dev)
    ref = PP.fold_tiles_numpy(lists, tiles.table, V, Cn)
    got = PP.fold_tiles(cd, tiles)
    same = got.counts.cpu().tolist() == ref["counts"].tolist()
    blocks = {"fold_tiles": [], "fold_views": []}
    for _ in range(5):  # alternating blocks: the two share whatever else the machine is doing
        blocks["fold_tiles"].append(event_median(lambda: PP.fold_tiles(cd, tiles))["median_us"])
        blocks["fold_views"].append(event_median(lambda: PP.fold_views(cd, views))["median_us"])
    res = dict(shape=dict(images=B, views=V, classes=Cn, rows_per_list=R, lists=B * V * Cn, rows=int(counts.sum()),
                          rows_kept_by_fold_tiles=int(ref["counts"].sum()), rows_kept_by_fold_views=int(PP.fold_views(cd, views).counts.sum())),
               fold_tiles_counts_equal_restatement=bool(same),
               fold_us={k: dict(block_medians=v, median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))
                        for k, v in blocks.items()})
    res["fold_us"]["ratio_tiles_over_views"] = res["fold_us"]["fold_tiles"]["median"] / res["fold_us"]["fold_views"]["median"]
    if not fold_only:
        ens = {"tiles": [], "views": []}
        for _ in range(3):
            ens["tiles"].append(host_median(lambda: PP.ensemble_views(cd, tiles, method="hard"), reps=7, warm=2)["median_ms"])
            ens["views"].append(host_median(lambda: PP.ensemble_views(cd, views, method="hard"), reps=7, warm=2)["median_ms"])
        res["ensemble_views_hard_ms"] = {k: dict(block_medians=v, median=float(np.median(v))) for k, v in ens.items()}
        res["rows_out"] = dict(tiles=PP.ensemble_views(cd, tiles, method="hard").total, views=PP.ensemble_views(cd, views, method="hard").total)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="tiled_inference_out")
    ap.add_argument("--images", type=int, default=1)
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--grid", default="2,2", help="ny,nx tiles per frame")
    ap.add_argument("--scale", type=float, default=384, help="shorter side of the whole frame as the tiles see it")
    ap.add_argument("--full", type=float, default=192, help="shorter side of the full-frame view")
    ap.add_argument("--overlap", type=int, default=32)
    ap.add_argument("--margin", type=int, default=4)
    ap.add_argument("--shot", type=int, default=2)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--side", type=int, default=96, help="side of a support shot on the sheet")
    ap.add_argument("--thickness", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--fold-only", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool runs on the device only")
    dev = torch.device("cuda:0")
    if not a.time:
        return write_sheets(a, dev)
    res = dict(time_folds(dev, a.fold_only), device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
