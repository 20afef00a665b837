"""What composed queries cost in the episode assembler: one batch at bs 4, way 2, shot 3 into 600 x 1000 holders (the pool
and the supports of tools/episode_augment_bench.py), assembled in one process by
  plain      the plain launches (one `ratio` query per item)
  augmented  the augmented launches (a drawn colour map on every record, min_visible 0.3)
  mosaic     the composed launches: a four-part mosaic per query (centre (290, 470), the four rows in rotating order)
  paste      the composed launches: per query a base part, four pasted objects (`paste_part` at target 300) and one erase

    python tools/episode_compose_bench.py [--reps 200] [--block 20]

All paths are warmed and checked (one part at (0, 0) through the composed launches must give the bits of the plain launches
on the same `crop` query), then timed in alternating blocks of `--block` batches until each has `--reps`. Per path, as in
tools/episode_augment_bench.py:
  gpu_ms     the interval between two device events around one batch (plan upload + three launches), device drained first
  host_ms    a host clock around the same calls, `plan_episode` included, no synchronise inside the window
  device_ms  the same interval with the batch enqueued behind a ~10 ms matrix product: the device time of the copy and the
             three kernels, not the enqueue
Prints one JSON line. profiles/episode_compose.md was made with it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from episode_augment_bench import B, BOXES, H, MEANS, QUERIES, S, SPECS, W, WS, _Count  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    from dana_amd import _lib, pipeline as PL
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(8)
    pool = PL.ImagePool(dev)
    for spec in SPECS:
        if spec[0] == "flip":
            pool.add_flipped(spec[1], spec[2])
        else:
            pool.add(rng.randint(0, 256, size=(spec[0], spec[1], 3)).astype(np.uint8), spec[2])
    pool.freeze()
    sups = [BOXES[(b + k) % 6] for b in range(B) for k in range(WS)]
    draw = np.random.default_rng(5)
    maps = [PL.draw_color_matrix(draw, p=1.0) for _ in range(B + B * WS)]
    queries = {"plain": QUERIES,
               "augmented": [dict(q, color=maps[b], min_visible=0.3) for b, q in enumerate(QUERIES)],
               "mosaic": [PL.mosaic_query(pool, [(b + k) % 4 for k in range(4)], (290, 470), (H, W), pos_cls=q["pos_cls"],
                                          min_visible=0.3) for b, q in enumerate(QUERIES)],
               "paste": []}
    for b, q in enumerate(QUERIES):
        ow = PL.plan_episode(pool, [q], holder_hw=(H, W)).queries[0]["ow"]
        parts = [dict(row=q["row"], crop=(0, 0, H, min(ow, W)), at=(0, 0))]
        for k, (row, _) in enumerate(BOXES[b:b + 4]):
            part = PL.paste_part(pool, row, 0, (0, 0), target_size=300, margin=4)
            part["at"] = (20 + 90 * k, 40 + 150 * k)
            parts.append(part)
        parts.append(dict(erase=(100, 200, 120, 160)))
        queries["paste"].append(dict(parts=parts, pos_cls=q["pos_cls"], min_visible=0.3))
    supports = {k: sups for k in queries}
    supports["augmented"] = [s + (maps[B + n],) for n, s in enumerate(sups)]
    holders = {k: PL.EpisodeHolders(B, 2, 3, H, W, dev) for k in queries}
    asm = {k: PL.EpisodeAssembler(pool, h, pixel_means=MEANS) for k, h in holders.items()}
    paths = {k: (lambda k=k: asm[k].assemble(PL.plan_episode(pool, queries[k], supports[k], holder_hw=(H, W)))) for k in queries}
    # one part at (0, 0) through the composed launches gives the plain bits (the tests compare this at edge shapes)
    crops = [dict(row=q["row"], pos_cls=q["pos_cls"], crop=p["crop"]) for q, p in zip(QUERIES, [c["parts"][0] for c in queries["paste"]])]
    want = [t.clone() for t in asm["plain"].assemble(PL.plan_episode(pool, crops, sups, holder_hw=(H, W)))]
    got = asm["mosaic"].assemble(PL.plan_episode(pool, [dict(q, at=(0, 0)) for q in crops], sups, holder_hw=(H, W)))
    for a, b in zip(want, got):
        assert torch.equal(a, b), "one part at (0, 0) through the composed launches differs from the plain launches"
    launches, words, kept = {}, {}, {}
    for name, fn in paths.items():  # warm-up and the launch counts
        fn()
        _lib.RECORDER = rec = _Count()
        try:
            fn()
        finally:
            _lib.RECORDER = None
        launches[name] = rec.n
        words[name] = int(PL.plan_episode(pool, queries[name], supports[name], holder_hw=(H, W)).words.nbytes)
        torch.cuda.synchronize()
        kept[name] = asm[name].all_cls_num_boxes.tolist()
    gpu, host, device = ({k: [] for k in paths} for _ in range(3))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    blocker = torch.randn((8192, 8192), device=dev)
    sink = torch.empty_like(blocker)
    torch.mm(blocker, blocker, out=sink)
    torch.cuda.synchronize()
    done = 0
    while done < args.reps:
        n = min(args.block, args.reps - done)
        for name, fn in paths.items():  # alternating blocks
            for _ in range(n):
                torch.cuda.synchronize()
                e0.record()
                t0 = time.perf_counter()
                fn()
                host[name].append((time.perf_counter() - t0) * 1e3)
                e1.record()
                e1.synchronize()
                gpu[name].append(e0.elapsed_time(e1))
            for _ in range(max(n // 4, 1)):
                torch.cuda.synchronize()
                torch.mm(blocker, blocker, out=sink)
                e0.record()  # completes when the product does; the batch is enqueued while it runs
                fn()
                e1.record()
                e1.synchronize()
                device[name].append(e0.elapsed_time(e1))
        done += n
    out = {"label": args.label, "reps": args.reps, "block": args.block,
           "shape": "B %d, way 2, shot 3, holders %dx%d, supports %d" % (B, H, W, S), "pool_bytes": pool.nbytes}
    for name in paths:
        g, h, d = np.array(gpu[name]), np.array(host[name]), np.array(device[name])
        out[name] = {"gpu_ms_median": round(float(np.median(g)), 4), "gpu_ms_min": round(float(g.min()), 4),
                     "host_ms_median": round(float(np.median(h)), 4), "host_ms_min": round(float(h.min()), 4),
                     "device_ms_median": round(float(np.median(d)), 4), "device_ms_min": round(float(d.min()), 4),
                     "c_abi_launches": launches[name], "plan_bytes": words[name], "boxes_kept": kept[name]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
