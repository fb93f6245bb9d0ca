"""Side measurement of the HuggingFace front-end (mv_hfenc_forward): the wav2vec2-base geometry (7 layers of 512 channels, GroupNorm on layer 0,
no conv bias) on 256 utterances of 3 s, in total and per layer, with HIP events.  The per-layer times come from mv_hfenc_forward_timed: events recorded
between the stages of the real launch sequence (layer 0 with the z-score, every further conv with its GELU / LayerNorm pass, the tail).  Beside it, in the
same run, one dense 1x1 layer of the FLOPs of encoder layer 1 (K = 3 * 512, N = 512, the same rows) on the ring GEMM: what the matrix pipes give
on this box for that much work.  Reported, not promised: no threshold.

    python tools/bench_hf_frontend.py [--batch 256] [--seconds 3] [--iters 10] [--norm group|layer]

--varlen: the variable-length form instead.  64 rows and 256 rows of seeded uniform 1-3 s lengths, width 512, both norms: one
mv_hfenc_forward_varlen call on the padded batch against the per-row loop it replaced in AudioFeaturizer.forward_varlen (the lengths read back
once, then h(wav[b:b+1, :n_b]) row by row into a zeroed output), timed the same way; beside them the stages of the fixed-length forward on the
padded batch (what the one call computes: every row at the padded length).  Reported, not promised.

    python tools/bench_hf_frontend.py --varlen [--iters 10]
"""
import argparse
import ctypes
import os
import sys

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


def per_row_loop(h, wav, num_samples, min_len):
    """AudioFeaturizer.forward_varlen's device path before mv_hfenc_forward_varlen: one read-back, then every row alone"""
    T = h(wav[:1]).size(1)
    out = torch.zeros((wav.size(0), T, h.dim), dtype=torch.float32, device=wav.device)
    lens = [int(n) for n in num_samples.tolist()]
    for i in range(wav.size(0)):
        n = min(max(lens[i], 0), wav.size(1))
        if n < min_len:
            continue
        f = h(wav[i:i + 1, :n])
        out[i, :f.size(1)] = f[0]
    return out


def varlen(iters):
    import hf_cases as hc
    import hf_ref
    from mvector import _hip
    from oracle import frontend
    dev = torch.device('cuda:0')
    print(f'# {torch.cuda.get_device_name(0)}; wav2vec2-base geometry, width 512, seeded uniform lengths of 1-3 s; medians (best) of {iters} runs, HIP events')
    for norm in ('group', 'layer'):
        cfg, sd = hc.seeded_model(norm)
        h = _hip.HfEncoder(cfg, {k: v.to(dev) for k, v in sd.items()})
        min_len = hf_ref.receptive_field(cfg)
        for B in (64, 256):
            g = torch.Generator().manual_seed(B)
            lens = torch.randint(16000, 48001, (B,), generator=g)
            L = int(lens.max())
            wav = frontend.synth_waveforms(B, L, seed=2)
            for b in range(B):
                wav[b, int(lens[b]):] = 0.0
            wav, n = wav.to(dev), lens.to(dev)
            one = h(wav, None, n)
            assert torch.equal(one, per_row_loop(h, wav, n, min_len)), 'the one call and the per-row loop differ'
            one_med, one_best = timed(lambda: h(wav, None, n), iters)
            loop_med, loop_best = timed(lambda: per_row_loop(h, wav, n, min_len), iters)
            stages = []
            for _ in range(iters + 3):
                ms = []
                h(wav, stage_ms=ms)
                stages.append(ms)
            stages = stages[3:]
            med = [sorted(r[i] for r in stages)[len(stages) // 2] for i in range(len(stages[0]))]
            print(f'{norm:5s} B = {B:3d}, L = {L} (mean length {float(lens.float().mean()):.0f}, padding {1 - float(lens.sum()) / (B * L):.1%} of the batch): '
                  f'one call {one_med:8.3f} ms ({one_best:.3f}), per-row loop {loop_med:8.3f} ms ({loop_best:.3f}), loop / one call = {loop_med / one_med:.2f}; same bits')
            print(f'      fixed-length forward on the padded batch, per stage (layers 0-6, tail): ' + ' '.join(f'{m:.3f}' for m in med) + f' = {sum(med):.3f} ms')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--varlen', action='store_true')
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--seconds', type=float, default=3.0)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--norm', default='group', choices=['group', 'layer'])
    a = ap.parse_args()
    if a.varlen:
        return varlen(a.iters)
    import hf_cases as hc
    from mvector import _hip
    from oracle import frontend
    dev = torch.device('cuda:0')
    B, L = a.batch, int(a.seconds * 16000)
    cfg, sd = hc.seeded_model(a.norm, conv_bias=False)
    sd = {k: v.to(dev) for k, v in sd.items()}
    wav = frontend.synth_waveforms(B, L, seed=1).to(dev)
    frames = hc.frames_of(L)
    print(f'# {torch.cuda.get_device_name(0)}; wav2vec2-base geometry, feat_extract_norm={a.norm}, B = {B}, L = {L} ({a.seconds} s), frames per layer {frames}')
    print(f'# medians of {a.iters} forwards, HIP events; per layer: events between the stages of one forward (mv_hfenc_forward_timed)')
    h = _hip.HfEncoder(cfg, sd)
    total_med, total_best = timed(lambda: h(wav), a.iters)
    stages = []
    for _ in range(a.iters + 3):
        ms = []
        h(wav, stage_ms=ms)
        stages.append(ms)
    stages = stages[3:]
    med = [sorted(r[i] for r in stages)[len(stages) // 2] for i in range(8)]
    cin, total_flop = 1, 0.0
    for i in range(7):
        passes = 2 if i == 0 and a.norm == 'group' else 1
        flop = 2.0 * B * frames[i] * cin * cfg['conv_kernel'][i] * 512 * passes
        total_flop += flop
        print(f'layer {i} (k = {cfg["conv_kernel"][i]}, {frames[i]} frames{", conv evaluated twice, with the z-score" if passes == 2 else ""}): {med[i]:7.3f} ms, '
              f'{flop / 1e9:8.1f} GFLOP, {flop / med[i] / 1e9:7.1f} TFLOP/s')
        cin = 512
    print(f'tail (feature_projection.layer_norm + time mean + mask, {frames[6]} frames): {med[7]:7.3f} ms')
    print(f'sum of the stages: {sum(med):.3f} ms')
    print(f'total (untimed forward, events around the call): {total_med:.3f} ms ({total_best:.3f}) for {B} utterances = {B / total_med * 1e3:.0f} utterances/s, '
          f'{total_flop / 1e9:.0f} GFLOP evaluated, {total_flop / total_med / 1e9:.1f} TFLOP/s over the whole forward')

    # yard-stick: a dense 1x1 layer of encoder layer 1's FLOPs on the ring GEMM
    cdll = _hip.lib()
    T, K, N = frames[1], 3 * 512, 512
    x = torch.randn(B, T, K, device=dev).half()
    w = torch.randn(N, K, 1, device=dev) * K ** -0.5
    wp = torch.empty(cdll.mv_conv1d_packed_elems(N, K, 1), dtype=torch.float16, device=dev)
    _hip.check(cdll.mv_conv1d_pack_weight(w.data_ptr(), N, K, 1, wp.data_ptr(), None))
    y = torch.empty(B, T, N, dtype=torch.float16, device=dev)
    d = _hip.MvConv1dDesc()
    d.x, d.x_dtype, d.ldx, d.w_packed, d.y, d.y_dtype, d.ldy = x.data_ptr(), _hip.MV_DT_F16, K, wp.data_ptr(), y.data_ptr(), _hip.MV_DT_F16, N
    d.B, d.T_in, d.T_out, d.cin, d.cout, d.k, d.dilation, d.stride = B, T, T, K, N, 1, 1, 1
    stream = torch.cuda.current_stream().cuda_stream
    med, best = timed(lambda: _hip.check(cdll.mv_conv1d_forward(ctypes.byref(d), stream)), a.iters)
    flop = 2.0 * B * T * K * N
    print(f'yard-stick: dense 1x1 ring GEMM [{B * T} x {K}] x [{K} x {N}] ({flop / 1e9:.1f} GFLOP, the FLOPs of layer 1): {med:.3f} ms ({best:.3f}), '
          f'{flop / med / 1e9:.1f} TFLOP/s')
    del x, y
    # encoder layer 1's convolution alone, as the handle launches it (k = 3, stride 2, no padding: the generic tap loader): layer 1's stage minus
    # this is its GELU pass; this against the yard-stick is what the dense-row ring route could gain at most
    T0, T1 = frames[0], frames[1]
    x = torch.randn(B, T0, 512, device=dev).half()
    w = torch.randn(512, 512, 3, device=dev) * K ** -0.5
    wp = torch.empty(cdll.mv_conv1d_packed_elems(512, 512, 3), dtype=torch.float16, device=dev)
    _hip.check(cdll.mv_conv1d_pack_weight(w.data_ptr(), 512, 512, 3, wp.data_ptr(), None))
    y = torch.empty(B, T1, 512, dtype=torch.float16, device=dev)
    d = _hip.MvConv1dDesc()
    d.x, d.x_dtype, d.ldx, d.w_packed, d.y, d.y_dtype, d.ldy = x.data_ptr(), _hip.MV_DT_F16, 512, wp.data_ptr(), y.data_ptr(), _hip.MV_DT_F16, 512
    d.B, d.T_in, d.T_out, d.cin, d.cout, d.k, d.dilation, d.stride = B, T0, T1, 512, 512, 3, 1, 2
    med, best = timed(lambda: _hip.check(cdll.mv_conv1d_forward(ctypes.byref(d), stream)), a.iters)
    print(f'layer 1 conv alone (strided taps, k = 3, s = 2, {flop / 1e9:.1f} GFLOP): {med:.3f} ms ({best:.3f}), {flop / med / 1e9:.1f} TFLOP/s')


if __name__ == '__main__':
    main()
