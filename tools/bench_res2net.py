"""Time the native Res2Net forward against the same module's torch graph (PyTorch-ROCm eager, fp32) on one device in one process.

  * the model: the default Res2Net (m_channels 32, layers [3, 4, 6, 3], base_width 32, scale 2, ASP; 5.61 M parameters) at 256 utterances x 298
    frames x 80 bins (3 s of Fbank frames), seeded features and weights (bn_gain 0.7, as the res2net_default fixture);
  * HIP events around every forward, 3 warm-ups, the median of 10;
  * the native forward twice: the serving handle (every map-storing launch reports to the handle's peak word: the TRACK instantiation of the
    conv kernel) and, with --no-peak-too (the default), a handle built with MV_RES2NET_NO_PEAK -- what the saturation word costs;
  * the `box` block of bench.py (tools/boxprobe) of the box the run landed on, first, so that the times can be told from the box.

    python tools/bench_res2net.py [--batch 256] [--frames 298] [--skip-torch] [--json out.json]

There is no pass bar: the parent of this tool could not run the model on the device at all.
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
from mvector.models.res2net import Res2Net  # noqa: E402
from oracle import weights  # noqa: E402


def timed(fn, warmup, reps):
    """median / min / max milliseconds of `reps` calls, each between two HIP events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return dict(ms=round(statistics.median(ts), 3), min=round(min(ts), 3), max=round(max(ts), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--frames', type=int, default=298)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--skip-torch', action='store_true', help='native forwards only')
    ap.add_argument('--no-peak-too', type=int, default=1, help='1: also time a handle without the peak word (MV_RES2NET_NO_PEAK)')
    ap.add_argument('--skip-box', action='store_true')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    _hip.lib()
    B, T = a.batch, a.frames
    model = Res2Net(input_size=80)
    sd = weights.make_state_dict(weights.shapes_of(model.state_dict()), 0, 0.7)
    model.load_state_dict(sd, strict=True)
    model.eval().to(dev)
    x = torch.randn(B, T, 80, generator=torch.Generator().manual_seed(80)).to(dev)
    out = dict(model='Res2Net default + ASP', batch=B, frames=T, warmup=a.warmup, reps=a.reps)
    if not a.skip_box:
        import bench
        out['box'] = bench.box_probe(dev)
        print('box', json.dumps(out['box']))

    dsd = {k: v.to(dev) for k, v in sd.items()}
    cfg = model._native_cfg()
    h = _hip.Model('res2net', cfg, dsd)
    out['workspace_gib'] = round(h.workspace_bytes(B, T) / 2 ** 30, 2)
    out['native'] = timed(lambda: h.forward(x), a.warmup, a.reps)
    out['native']['utt_per_s'] = round(B / out['native']['ms'] * 1e3, 1)
    out['range'] = h.s16_range()
    emb = h.forward(x)
    print(f"native (peak word)     {out['native']['ms']:9.3f} ms / forward  ({out['native']['min']:.3f} .. {out['native']['max']:.3f})  "
          f"{out['native']['utt_per_s']:.0f} utt/s  workspace {out['workspace_gib']} GiB  peak {out['range']['peak']:.1f} saturated {out['range']['saturated']}")
    if a.no_peak_too:
        cfg.pooling_type |= _hip.MV_RES2NET_NO_PEAK
        h2 = _hip.Model('res2net', cfg, dsd)
        out['native_no_peak'] = timed(lambda: h2.forward(x), a.warmup, a.reps)
        out['peak_word_cost'] = round(out['native']['ms'] / out['native_no_peak']['ms'], 4)
        assert torch.equal(h2.forward(x), emb)   # the word changes no bit of the result
        print(f"native (no peak word)  {out['native_no_peak']['ms']:9.3f} ms / forward  ({out['native_no_peak']['min']:.3f} .. "
              f"{out['native_no_peak']['max']:.3f})  with / without x{out['peak_word_cost']:.4f}")
        del h2
    if not a.skip_torch:
        def torch_forward():
            with torch.no_grad():
                return model(x)
        # the module's forward routes eval CUDA inputs to the native handle: the gate is held shut for the torch graph's timing
        model._use_native = lambda _x: False
        out['torch_eager_fp32'] = timed(torch_forward, a.warmup, a.reps)
        ref = torch_forward()
        del model._use_native
        out['speedup_vs_torch'] = round(out['torch_eager_fp32']['ms'] / out['native']['ms'], 2)
        out['one_minus_cos_vs_torch'] = float((1 - torch.nn.functional.cosine_similarity(emb.double(), ref.double(), dim=1)).max())
        print(f"torch eager fp32       {out['torch_eager_fp32']['ms']:9.3f} ms / forward  ({out['torch_eager_fp32']['min']:.3f} .. "
              f"{out['torch_eager_fp32']['max']:.3f})  native x{out['speedup_vs_torch']:.2f} faster  1 - cos native vs torch {out['one_minus_cos_vs_torch']:.2e}")
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
