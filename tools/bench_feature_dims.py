"""Time the native EcapaTdnn-1024 forward at feature widths F = 200, 201 and 208, and the TDNN at 23 vs 24, on one device in one process:
256 utterances x 298 frames (3 s of Fbank frames) of seeded features and seeded weights, warm-up first, then HIP events around `--iters`
back-to-back forwards.  A width that is not a multiple of 8 is zero-padded to the next one on the device (the pad pass replaces the cast
pass of the aligned widths), so 201 is expected to cost about what 208 costs.

    python tools/bench_feature_dims.py [--iters 20] [--json out.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'voiceprintrecognition-pytorch_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from mvector import _hip  # noqa: E402
from mvector.models import EcapaTdnn, TDNN  # noqa: E402
from oracle import weights  # noqa: E402


def time_model(kind, module, B, T, F, iters, warmup, dev):
    sd = weights.make_state_dict(weights.shapes_of(module.state_dict()), 3)
    m = _hip.Model(kind, module._native_cfg(), {k: v.to(dev) for k, v in sd.items()})
    x = (torch.randn(B, T, F, generator=torch.Generator().manual_seed(F)) * 2).to(dev)
    for _ in range(warmup):
        m.forward(x)
    torch.cuda.synchronize()
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
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    B, T = a.batch, a.frames
    results = {}
    for F in (200, 201, 208):
        mod = EcapaTdnn(input_size=F, channels=[1024, 1024, 1024, 1024, 3072])
        results[f'ecapa1024_F{F}'] = round(time_model('ecapa', mod, B, T, F, a.iters, a.warmup, dev), 1)
    for F in (23, 24):
        mod = TDNN(input_size=F)
        results[f'tdnn_F{F}'] = round(time_model('tdnn', mod, B, T, F, a.iters, a.warmup, dev), 1)
    for name, us in results.items():
        print(f'{name:18s} {us:9.1f} us/forward')
    print(f"ecapa1024 201 / 208: x{results['ecapa1024_F201'] / results['ecapa1024_F208']:.3f}   "
          f"201 / 200: x{results['ecapa1024_F201'] / results['ecapa1024_F200']:.3f}   "
          f"tdnn 23 / 24: x{results['tdnn_F23'] / results['tdnn_F24']:.3f}")
    line = json.dumps(dict(batch=B, frames=T, iters=a.iters, us_per_forward=results))
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
