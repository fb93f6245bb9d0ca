"""Time the MelSpectrogram, Spectrogram and MFCC front-ends (default arguments) on one device, in one process:
256 x 3 s / 16 kHz with ragged length ratios, warm-up first, then HIP events around `--iters` back-to-back forwards.

Reports microseconds per forward and the compulsory HBM traffic over that time against 8 TB/s: the waveforms in (49.2 MB), the
features out, and for MFCC the mel power the mel stage writes and the dB / DCT launches read back (it is not fused).

    python tools/bench_frontends.py [--iters 50] [--json out.json]
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
from oracle import frontend  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--samples', type=int, default=48000)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    B, L = a.batch, a.samples
    wav = frontend.synth_waveforms(B, L, seed=1).to(dev)
    ratio = torch.linspace(0.5, 1.0, B).to(dev)
    handles = {'MelSpectrogram': _hip.MelSpec({}), 'Spectrogram': _hip.Spectrogram({}), 'MFCC': _hip.Mfcc({})}
    results = {}
    for name, h in handles.items():
        for _ in range(a.warmup):
            out = h(wav, ratio)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.iters):
            out = h(wav, ratio)
        t1.record()
        torch.cuda.synchronize()
        us = t0.elapsed_time(t1) * 1e3 / a.iters
        T = out.shape[1]
        nbytes = 4.0 * B * L + 4.0 * out.numel()
        if name == 'MFCC':
            nbytes += 2 * 4.0 * B * T * 128 + 4.0 * B * T * 128   # mel power written, read by the dB max and by the DCT
        results[name] = dict(us_per_forward=round(us, 1), T=T, feature_dim=out.shape[2], mbytes=round(nbytes / 1e6, 1),
                             tb_per_s=round(nbytes / (us * 1e-6) / 1e12, 3), frac_of_8tbs=round(nbytes / (us * 1e-6) / HBM_BYTES_PER_S, 3))
    base = results['MelSpectrogram']['us_per_forward']
    for name in results:
        results[name]['vs_melspectrogram'] = round(results[name]['us_per_forward'] / base, 2)
    for name, r in results.items():
        print(f"{name:15s} {r['us_per_forward']:9.1f} us  {r['mbytes']:6.1f} MB  {r['tb_per_s']:.2f} TB/s ({100 * r['frac_of_8tbs']:.1f} % of 8)  "
              f"x{r['vs_melspectrogram']:.2f} of MelSpectrogram")
    line = json.dumps(dict(batch=B, samples=L, iters=a.iters, results=results))
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
