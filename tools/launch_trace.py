"""The launch sequence of one forward (+ backward) as text, for `diff` between two commits: one line per C-ABI launch
(entry point, every non-pointer argument, pointers as 0 / p, the stream as an ordinal by first appearance) and per event
operation (rec / wait, event ordinal, stream ordinal). A host-side refactor must leave every line as it was.

usage: launch_trace.py OUT.txt CASE [--mfma 0|1] [--shape B,way,shot,H,W]
CASE = model[,train][,attr=value ...][,+bwd | +trainer | +cached | +sweep | +bank | +qbank], e.g.
  DAnA                                            eval forward (eval cases run way 1, as the reference's eval)
  DAnA,train,merge_trunk=True,merge_from=1,+bwd   saving forward + model_backward
  DAnA,train,+trainer                             one Trainer.step
  DAnA,+cached  /  DAnA,+sweep                    encode_supports + one cached forward / one class sweep
  DAnA,train,+bank  /  DAnA,train,+qbank          one forward from a SupportBank episode / a QueryBank batch: the model is
                                                  built under cfg.RESNET.FIXED_BLOCKS = 3; the bank and its episode / batch
                                                  are made once, untraced (an index write under a recorder is refused)
  fsod,train,+bwd                                 a sibling (frcnn, meta, fgn, fsod)
The case runs once untraced (weight plan, allocator) and once traced. The other commit's package is traced by this same
file: put its directory in front on PYTHONPATH (and DANA_LIB_PATH on the library to use)."""
import ast
import ctypes
import os
import re
import sys


class Trace:
    """`_lib.RECORDER` stand-in: formats what `_Lib.call` hands to `add_call` and the event operations"""

    def __init__(self, protos):
        self.protos, self.lines, self.streams, self.events = protos, [], {}, {}

    def _stream(self, raw):
        return "s%d" % self.streams.setdefault(raw or 0, len(self.streams))

    def add_call(self, fn, name, args):
        out = [name]
        for (ty, _), a in zip(self.protos[name][1], args):
            v = a.value if isinstance(a, ctypes._SimpleCData) else a
            if ty == "dana_stream_t":
                out.append(self._stream(v))
            elif ty.endswith("*"):
                out.append("p" if v else "0")
            else:
                out.append(repr(v))
        self.lines.append(" ".join(out))

    def event(self, kind, ev, stream):
        n = self.events.setdefault(id(ev), (len(self.events), ev))[0]  # (holds the event: its id is not reused)
        self.lines.append("%s e%d %s" % (kind, n, self._stream(stream.cuda_stream)))


def main(out_path, case, mfma=1, shape=(2, 2, 2, 160, 224)):
    import numpy as np
    import torch
    sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # (behind PYTHONPATH: see the docstring)
    import dana_amd
    from dana_amd import _lib, ops, synthetic as S, backward as BW
    name, *opts = re.split(r",(?![^(]*\))", case)  # (commas inside a tuple value stay)
    kind = ([o for o in opts if o.startswith("+")] or ["+fwd"])[0]
    attrs = {k: ast.literal_eval(v) for k, v in (o.split("=") for o in opts if "=" in o)}
    B, way, shot, H, W = shape
    if "train" not in opts:
        way = 1  # (eval takes the positive supports only, dana.py:111)
    if "trunk_layers" in attrs:  # (read by create_architecture)
        dana_amd.DAnARCNN.trunk_layers = attrs.pop("trunk_layers")
    dev = torch.device("cuda:0")
    ops.set_mfma_mode(mfma)
    cfg = dana_amd.cfg
    prev_fixed = cfg.RESNET.FIXED_BLOCKS
    if kind in ("+bank", "+qbank"):
        cfg.RESNET.FIXED_BLOCKS = 3  # (read by the constructor: a bank row is a constant only over a frozen trunk)
    m = dana_amd.get_model(name, pretrained=False, way=way, shot=shot, classes=["fg", "bg"])
    cfg.RESNET.FIXED_BLOCKS = prev_fixed
    sd = S.fill_state_dict(m.state_dict(), seed=21, profile="test")
    m.load_state_dict(S.tame_fsod_weights(sd) if name == "fsod" else sd)
    m.to(dev).train("train" in opts)
    for k, v in attrs.items():
        setattr(m, k, v)
    m.save_for_backward = kind == "+bwd"
    e = [t.to(dev) for t in S.episode_inputs(B, way, shot, H, W, seed=4)]
    inputs = e[:4] if name == "frcnn" else e + [e[2].clone()] if name == "meta" else e
    if kind == "+trainer":
        from dana_amd.trainer import Trainer
        tr = Trainer(m, lr=1e-3)
    if kind == "+bank":  # (every support image of the episode is a bank row, in episode order)
        bank = m.encode_support_bank(e[4].reshape(-1, 3, e[4].size(-2), e[4].size(-1)))
        inputs = e[:4] + [bank.episode(np.arange(len(bank)).reshape(B, -1))]
    if kind == "+qbank":
        inputs = [m.encode_query_bank(e[0]).batch(np.arange(B))] + e[1:]

    def run():
        np.random.seed(7)
        if kind == "+trainer":
            return tr.step(*inputs)
        with torch.no_grad():
            if kind in ("+cached", "+sweep"):
                cache = m.encode_supports(e[4].reshape(B, -1, 3, e[4].size(-2), e[4].size(-1)))
                sup = cache.sweep() if kind == "+sweep" else cache
                on, _lib.RECORDER = _lib.RECORDER, None  # (a cache's first forward of a batch size runs outside a recording)
                m(*e[:4], sup, *inputs[5:])  # (meta's 6th argument, all_cls_gt_boxes, goes along)
                _lib.RECORDER = on
                return m(*e[:4], sup, *inputs[5:])
            m(*inputs)
        if kind == "+bwd":
            BW.model_backward(m, (1.0, 1.0, 1.0, 1.0))

    run()
    torch.cuda.synchronize()
    L = _lib.lib()
    tr_ = Trace(dict(L.protos, **L.debug_protos))
    ev = torch.cuda.Event
    rec, wait = ev.record, ev.wait
    def hooked(orig, kind):  # (as program.LaunchProgram.recording: Stream.wait_event and ops.record_event go through these)
        def op(e_, stream=None):
            stream = stream if stream is not None else ops.cur_stream()
            orig(e_, stream)
            if _lib.RECORDER is tr_:
                tr_.event(kind, e_, stream)
        return op

    ev.record, ev.wait = hooked(rec, "rec"), hooked(wait, "wait")
    _lib.RECORDER = tr_
    try:
        run()
    finally:
        _lib.RECORDER, ev.record, ev.wait = None, rec, wait
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(tr_.lines) + "\n")
    print("%s: %d lines, %d streams, %d events -> %s" % (case, len(tr_.lines), len(tr_.streams), len(tr_.events), out_path))


if __name__ == "__main__":
    a = sys.argv[1:]
    kw = {}
    if "--mfma" in a:
        kw["mfma"] = int(a[a.index("--mfma") + 1])
    if "--shape" in a:
        kw["shape"] = tuple(int(v) for v in a[a.index("--shape") + 1].split(","))
    main(a[0], a[1], **kw)
