"""Time the MelSpectrogram, Spectrogram and MFCC front-ends (default arguments) on one device, in one process:
256 x 3 s / 16 kHz with ragged length ratios, warm-up first, then HIP events around `--iters` back-to-back forwards.

Reports microseconds per forward and the compulsory HBM traffic over that time against 8 TB/s: the waveforms in (49.2 MB), the
features out, and for MFCC the mel power the mel stage writes and the dB / DCT launches read back (it is not fused).

    python tools/bench_frontends.py [--iters 50] [--json out.json]

`--varlen`: the variable-length leg instead.  64 rows of 1 ... 10 s (seeded lengths), each featurised on its own length: ONE native call
(`mv_*_forward_varlen`) against the per-row loop `AudioFeaturizer.forward_varlen` ran before those entry points existed -- one forward, one
device-to-host read of the row's length and one copy per row.  Both in this process, alternating A B B A, `--repeats` rounds; wall-clock
times around a device synchronisation (the loop's cost IS its host synchronisations), median and spread of the rounds for either side.
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


def _loop_forward_varlen(h, wav, num_samples, dim):
    """what AudioFeaturizer.forward_varlen did on CUDA tensors for these three methods: a forward, a host sync and a copy per row"""
    out = torch.zeros((wav.size(0), h.num_frames(wav.size(1)), dim), dtype=torch.float32, device=wav.device)
    for i in range(wav.size(0)):
        n = int(num_samples[i])
        f = h(wav[i:i + 1, :n])
        out[i, :f.size(1)] = f[0]
    return out


def varlen_leg(a):
    import statistics
    import time
    dev = torch.device('cuda:0')
    B, rate = 64, 16000
    g = torch.Generator().manual_seed(a.seed)
    lens = torch.randint(1 * rate, 10 * rate + 1, (B,), generator=g)
    L = int(lens.max())
    wav = frontend.synth_waveforms(B, L, seed=2)
    for b in range(B):
        wav[b, int(lens[b]):] = 0.0
    wav, n = wav.to(dev), lens.to(dev)
    handles = {'MelSpectrogram': (_hip.MelSpec({}), 128), 'Spectrogram': (_hip.Spectrogram({}), 201), 'MFCC': (_hip.Mfcc({}), 40)}
    results = {}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6, out

    for name, (h, dim) in handles.items():
        one = lambda: h(wav, None, n)                             # noqa: E731
        loop = lambda: _loop_forward_varlen(h, wav, n, dim)       # noqa: E731
        same = torch.equal(one(), loop())
        for _ in range(a.warmup):
            one()
            loop()
        t_one, t_loop = [], []
        for _ in range(a.repeats):                                # A B B A
            t_one.append(timed(one)[0])
            t_loop.append(timed(loop)[0])
            t_loop.append(timed(loop)[0])
            t_one.append(timed(one)[0])
        r = dict(rows=B, seconds_total=round(float(lens.sum()) / rate, 1), same_bits=bool(same),
                 one_call_us=dict(median=round(statistics.median(t_one), 1), min=round(min(t_one), 1), max=round(max(t_one), 1)),
                 row_loop_us=dict(median=round(statistics.median(t_loop), 1), min=round(min(t_loop), 1), max=round(max(t_loop), 1)))
        r['loop_over_one_call'] = round(r['row_loop_us']['median'] / r['one_call_us']['median'], 2)
        r['one_call_faster_beyond_spread'] = bool(r['one_call_us']['max'] < r['row_loop_us']['min'])
        results[name] = r
        print(f"{name:15s} one call {r['one_call_us']['median']:9.1f} us [{r['one_call_us']['min']:.1f} .. {r['one_call_us']['max']:.1f}]   "
              f"row loop {r['row_loop_us']['median']:9.1f} us [{r['row_loop_us']['min']:.1f} .. {r['row_loop_us']['max']:.1f}]   "
              f"x{r['loop_over_one_call']:.2f}  same bits: {same}")
    line = json.dumps(dict(leg='varlen', rows=B, max_samples=L, repeats=a.repeats, results=results))
    print(line)
    bad = [k for k, r in results.items() if not (r['same_bits'] and r['one_call_faster_beyond_spread'])]
    if bad:   # the single call must give the loop's bits and beat it by more than the spread of the repeats
        raise SystemExit(f'variable-length leg: {bad} -- one call is not faster than the row loop beyond the spread, or the bits differ')
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--samples', type=int, default=48000)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--json', default=None)
    ap.add_argument('--varlen', action='store_true', help='the variable-length leg: one native call against the per-row loop')
    ap.add_argument('--repeats', type=int, default=10, help='--varlen: A B B A rounds')
    ap.add_argument('--seed', type=int, default=0, help='--varlen: seed of the row lengths')
    a = ap.parse_args()
    if a.varlen:
        line = varlen_leg(a)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, 'w') as f:
                f.write(line + '\n')
        return
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
