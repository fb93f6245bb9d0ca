"""Side measurement of the Wav2Vec2-BERT front-end (mv_w2vbert_forward): 256 utterances of 3 s of seeded bursts (tests/w2vbert_cases.py), HIP
events, 3 warm-ups, median (best) of 10.  The `box` block of bench.py comes first.  Recorded: the whole call with its features left on the device;
the plain Fbank-80 handle alone on the same batch (no time mean, no mask), so the difference is what the new passes -- per-bin statistics, the
normalise / stack / LayerNorm row pass, time mean and mask -- add; and the host yard-stick, one run on the same box: the HF
SeamlessM4TFeatureExtractor on the numpy rows plus the LayerNorm in torch on the CPU, which is what the reference runs.  The one condition on
time: the device call is faster than the host yard-stick (PASS / FAIL line).  Nothing else is promised.

    python tools/bench_w2vbert_frontend.py [--batch 256] [--seconds 3] [--iters 10]

--varlen: 256 rows of seeded uniform 1 - 3 s lengths: one mv_w2vbert_forward_varlen call on the padded batch against the per-row loop (the
lengths read back once, then the handle on wav[b:b+1, :n_b] row by row into a zeroed output); the same bits from both.

    python tools/bench_w2vbert_frontend.py --varlen [--iters 10]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'voiceprintrecognition-pytorch_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    ev[0].record()
    for i in range(iters):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(iters))
    return ms[len(ms) // 2], ms[0]


def per_row_loop(h, wav, num_samples):
    T2 = h.num_frames(wav.size(1))
    out = torch.zeros((wav.size(0), T2, h.dim), dtype=torch.float32, device=wav.device)
    lens = [int(n) for n in num_samples.tolist()]
    for i in range(wav.size(0)):
        n = min(max(lens[i], 0), wav.size(1))
        if n < 560:
            continue
        f = h(wav[i:i + 1, :n])
        out[i, :f.size(1)] = f[0]
    return out


def host_yardstick(wav, ln_w, ln_b, eps):
    """the reference's host path for this model: the HF processor on the numpy rows, then feature_projection.layer_norm; seconds of one run"""
    from transformers import SeamlessM4TFeatureExtractor
    processor = SeamlessM4TFeatureExtractor()
    x = wav.numpy()
    t0 = time.perf_counter()
    inputs = processor(x, sampling_rate=16000, return_tensors='pt')
    with torch.no_grad():
        out = torch.nn.functional.layer_norm(inputs['input_features'].float(), (160,), ln_w, ln_b, eps)
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--varlen', action='store_true')
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--seconds', type=float, default=3.0)
    ap.add_argument('--iters', type=int, default=10)
    a = ap.parse_args()
    import bench
    import w2vbert_cases as wc
    from mvector import _hip
    dev = torch.device('cuda:0')
    print(json.dumps(dict(box=bench.box_probe(dev))))
    B, L = a.batch, int(a.seconds * 16000)
    h = wc.handle(None, True, dev)
    ln_w, ln_b = wc.layer_norm_tensors()
    if a.varlen:
        g = torch.Generator().manual_seed(B)
        lens = torch.randint(16000, 48001, (B,), generator=g)
        L = int(lens.max())
        wav = wc.burst_waveforms(B, L, seed=2)
        for b in range(B):
            wav[b, int(lens[b]):] = 0.0
        wav, n = wav.to(dev), lens.to(dev)
        print(f'# {torch.cuda.get_device_name(0)}; B = {B}, seeded uniform lengths of 1-3 s, L = {L} (padding {1 - float(lens.sum()) / (B * L):.1%} of the '
              f'batch); medians (best) of {a.iters} runs, HIP events')
        assert torch.equal(h(wav, None, n), per_row_loop(h, wav, n)), 'the one call and the per-row loop differ'
        one_med, one_best = timed(lambda: h(wav, None, n), a.iters)
        loop_med, loop_best = timed(lambda: per_row_loop(h, wav, n), a.iters)
        print(f'one mv_w2vbert_forward_varlen call {one_med:8.3f} ms ({one_best:.3f}), per-row loop {loop_med:8.3f} ms ({loop_best:.3f}), '
              f'loop / one call = {loop_med / one_med:.2f}; same bits')
        return
    wav_cpu = wc.burst_waveforms(B, L, seed=1)
    wav = wav_cpu.to(dev)
    T2 = h.num_frames(L)
    print(f'# {torch.cuda.get_device_name(0)}; B = {B}, L = {L} ({a.seconds} s), {1 + (L - 400) // 160} frames -> {T2} stacked '
          f'frames of 160; medians (best) of {a.iters} runs after 3 warm-ups, HIP events')
    got = h(wav)
    whole_med, whole_best = timed(lambda: h(wav), a.iters)
    fb = _hip.Fbank(dict(sample_frequency=16000, num_mel_bins=80), subtract_time_mean=False)
    fb_med, fb_best = timed(lambda: fb(wav), a.iters)
    print(f'mv_w2vbert_forward, features left on the device: {whole_med:.3f} ms ({whole_best:.3f}) = {B / whole_med * 1e3:.0f} utterances/s')
    print(f'Fbank-80 handle alone on the same batch (no time mean, no mask): {fb_med:.3f} ms ({fb_best:.3f})')
    print(f'the new passes (statistics, row pass, time mean and mask) add {whole_med - fb_med:.3f} ms = {(whole_med - fb_med) / whole_med:.0%} of the call')
    host_s, host_out = host_yardstick(wav_cpu, ln_w, ln_b, wc.CFG['layer_norm_eps'])
    host_out = host_out - host_out.mean(1, keepdim=True)
    d = (got.cpu() - host_out).abs()
    print(f'host yard-stick, one run: SeamlessM4TFeatureExtractor + layer_norm on the CPU ({torch.get_num_threads()} torch threads): {host_s * 1e3:.1f} ms; '
          f'device - host features: max-abs {d.max().item():.2e}')
    print(f'{"PASS" if whole_med < host_s * 1e3 else "FAIL"}: device call {whole_med:.3f} ms against the host\'s {host_s * 1e3:.1f} ms ({host_s * 1e3 / whole_med:.0f} x)')


if __name__ == '__main__':
    main()
