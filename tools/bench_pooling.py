"""Time the native EcapaTdnn-1024 and TDNN forwards with each pooling head (ASP, SAP, TAP, TSP) on one device in one process: 256 utterances
x 298 frames (3 s of Fbank frames) of seeded features and seeded weights.  The heads ALTERNATE -- round r times `--iters` back-to-back forwards
of every head in turn, with HIP events -- so clock drift and warm-up land on all of them alike; the median round is reported, and the ratio
to ASP.  The backbone in front of the head is the same in all four; SAP, TAP and TSP replace ASP's hidden conv, context layer and attentive
statistics kernel with one conv + the mean-only pooling kernel (SAP) or one reduction pass (TAP, TSP).

    python tools/bench_pooling.py [--iters 20] [--rounds 5] [--json out.json]

(EcapaTdnn + TSP is built through the C ABI here: the library runs it, the module's Python gate does not offer it yet.)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'voiceprintrecognition-pytorch_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from mvector import _hip  # noqa: E402
from mvector.models import EcapaTdnn, TDNN  # noqa: E402
from oracle import weights  # noqa: E402

HEADS = ('ASP', 'SAP', 'TAP', 'TSP')
MODELS = {
    'ecapa1024': ('ecapa', lambda pt: EcapaTdnn(input_size=80, channels=[1024, 1024, 1024, 1024, 3072], pooling_type=pt)),
    'tdnn': ('tdnn', lambda pt: TDNN(input_size=80, pooling_type=pt)),
}


def handle(kind, module, pt, dev):
    sd = weights.make_state_dict(weights.shapes_of(module.state_dict()), 3)
    return _hip.Model(kind, module._native_cfg(), {k: v.to(dev) for k, v in sd.items()}, pooling_type=pt)


def time_once(m, x, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        m.forward(x)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--frames', type=int, default=298)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    B, T = a.batch, a.frames
    x = (torch.randn(B, T, 80, generator=torch.Generator().manual_seed(80)) * 2).to(dev)
    results = {}
    for name, (kind, make) in MODELS.items():
        hs = {pt: handle(kind, make(pt), pt, dev) for pt in HEADS}
        for m in hs.values():
            for _ in range(a.warmup):
                m.forward(x)
        torch.cuda.synchronize()
        rounds = {pt: [] for pt in HEADS}
        for _ in range(a.rounds):
            for pt in HEADS:
                rounds[pt].append(time_once(hs[pt], x, a.iters))
        asp = statistics.median(rounds['ASP'])
        for pt in HEADS:
            med = statistics.median(rounds[pt])
            results[f'{name}_{pt}'] = dict(us=round(med, 1), min=round(min(rounds[pt]), 1), max=round(max(rounds[pt]), 1),
                                           vs_asp=round(med / asp, 3))
        del hs
    for key, r in results.items():
        print(f"{key:16s} {r['us']:9.1f} us/forward  (rounds {r['min']:.1f} .. {r['max']:.1f})  x{r['vs_asp']:.3f} of ASP")
    line = json.dumps(dict(batch=B, frames=T, iters=a.iters, rounds=a.rounds, us_per_forward=results))
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
