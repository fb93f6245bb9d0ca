"""Time EcapaTdnn-1024 with grouped TDNN convolutions and one grouped 1x1 layer against its block-diagonal expansion, on one device in one
process.

  * the model: groups=[1, g, g, g, g] for g in 1, 2, 4, 8 (tdnn1 / tdnn2 of the three SE-Res2Net blocks and the MFA grouped; blocks.0 dense) at
    256 utterances x 298 frames (3 s of Fbank frames), seeded features and weights.  The group counts ALTERNATE -- round r times `--iters`
    back-to-back forwards of every g in turn, with HIP events -- and the median round is reported with its ratio to g = 1;
  * the layer: a 1024 -> 1024 1x1 TDNNBlock layer over the same 76 288 rows, grouped by g = 2, 4, 8: the grouped GEMM
    (mv_conv1d_forward_grouped) against the dense layer of its block-diagonal weight (what an expansion at create would run), alternating too.

    python tools/bench_ecapa_groups.py [--iters 20] [--rounds 5] [--json out.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'voiceprintrecognition-pytorch_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from mvector import _hip  # noqa: E402
from mvector.models import EcapaTdnn  # noqa: E402
from oracle import weights  # noqa: E402

GROUPS = (1, 2, 4, 8)


def model_handle(g, dev):
    m = EcapaTdnn(input_size=80, channels=[1024, 1024, 1024, 1024, 3072], groups=[1, g, g, g, g])
    sd = weights.make_state_dict(weights.shapes_of(m.state_dict()), 3)
    h = _hip.Model('ecapa', m._native_cfg(), {k: v.to(dev) for k, v in sd.items()})
    return h, [int(h.info(k)) for k in (_hip.MV_INFO_ECAPA_GROUPED_NATIVE, _hip.MV_INFO_ECAPA_GROUPED_EXPANDED)]


def time_once(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def layer_runners(g, rows, C, dev, lib):
    """(grouped GEMM, dense block-diagonal expansion) of a C -> C 1x1 layer grouped by g over `rows` rows"""
    import ecapa_variant_checks as ev
    gen = torch.Generator().manual_seed(g)
    x = (torch.randn(rows, C, generator=gen)).half().to(dev)
    w = (torch.randn(C, C // g, 1, generator=gen) * (2.0 / (C // g)) ** 0.5).to(dev)
    dense = torch.zeros(C, C, 1, device=dev)
    for gi in range(g):
        s = slice(gi * (C // g), (gi + 1) * (C // g))
        dense[s, s] = w[s]
    bias, scale, shift = (torch.rand(C, generator=gen).to(dev) for _ in range(3))
    y = torch.empty(rows, C, dtype=torch.float16, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    dg = ev.desc(x, C, ev.pack_grouped(lib, w, g), bias, scale, shift, y, C, 1, rows, C, C)
    pd = ev.pack_grouped(lib, dense, 1)
    dd = ev.desc(x, C, pd, bias, scale, shift, y, C, 1, rows, C, C)
    keep = (x, w, dense, bias, scale, shift, y, pd, dg, dd)
    assert lib.mv_conv1d_grouped_native(C, C, 1, g) == 1

    def grouped():
        _hip.check(lib.mv_conv1d_forward_grouped(ctypes.byref(dg), g, st), lib)

    def expanded():
        _hip.check(lib.mv_conv1d_forward(ctypes.byref(dd), st), lib)
    grouped.keep = expanded.keep = keep
    return grouped, expanded


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
    lib = _hip.lib()
    B, T = a.batch, a.frames
    x = (torch.randn(B, T, 80, generator=torch.Generator().manual_seed(80)) * 2).to(dev)
    out = dict(batch=B, frames=T, iters=a.iters, rounds=a.rounds, model={}, layer={})

    hs = {g: model_handle(g, dev) for g in GROUPS}
    for h, _ in hs.values():
        for _ in range(a.warmup):
            h.forward(x)
    torch.cuda.synchronize()
    rounds = {g: [] for g in GROUPS}
    for _ in range(a.rounds):
        for g in GROUPS:
            rounds[g].append(time_once(lambda: hs[g][0].forward(x), a.iters))
    base = statistics.median(rounds[1])
    for g in GROUPS:
        med = statistics.median(rounds[g])
        out['model'][f'g{g}'] = dict(us=round(med, 1), min=round(min(rounds[g]), 1), max=round(max(rounds[g]), 1), vs_g1=round(med / base, 3),
                                     native=hs[g][1][0], expanded=hs[g][1][1])
        print(f"EcapaTdnn-1024 groups=[1,{g},{g},{g},{g}]  {med:9.1f} us/forward  (rounds {min(rounds[g]):.1f} .. {max(rounds[g]):.1f})  "
              f"x{med / base:.3f} of g=1  (grouped layers native {hs[g][1][0]}, expanded {hs[g][1][1]})")
    del hs

    C = 1024
    for g in GROUPS[1:]:
        fg, fe = layer_runners(g, B * T, C, dev, lib)
        for _ in range(a.warmup):
            fg()
            fe()
        torch.cuda.synchronize()
        rg, re_ = [], []
        for _ in range(a.rounds):
            rg.append(time_once(fg, a.iters))
            re_.append(time_once(fe, a.iters))
        mg, me = statistics.median(rg), statistics.median(re_)
        flop = 2.0 * B * T * C * C / g
        out['layer'][f'g{g}'] = dict(grouped_us=round(mg, 1), expanded_us=round(me, 1), grouped_vs_expanded=round(mg / me, 3),
                                     grouped_tflops=round(flop / mg / 1e6, 1))
        print(f'1x1 layer {C}->{C} g={g} over {B * T} rows: grouped {mg:8.1f} us  expanded {me:8.1f} us  grouped/expanded x{mg / me:.3f} '
              f'(1/g = {1 / g:.3f}); grouped {flop / mg / 1e6:.0f} TFLOP/s of useful work')
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
