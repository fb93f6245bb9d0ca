"""Time the native SphereFace2 and triplet losses (csrc/sphereface2.hip, csrc/triplet.hip) against what the parent commit ran for the two
classes: the package's own torch expression (``SphereFace2.torch_expression`` / ``TripletAngularMarginLoss.torch_expression``, PyTorch-ROCm
eager with autograd) on the same fp32 tensors and the same device.  One visit: HIP events around forward + backward, 3 warm-ups, the median
of 10.

Sizes: SphereFace2 type C and type A at (B, N) = (256, 5 994) and (512, 100 000); the triplet loss with its cross-entropy at
(B, D, N) = (256, 192, 5 994) and (1 024, 512, 5 994), 32 utterances per speaker.  Per size:
  * `native` / `torch`: forward + backward in ms (native: the `_hip` calls the modules make, the backward into a second buffer as autograd uses
    it; for the triplet loss mv_triplet_* plus mv_margin_ce_* of kind CE); `native_forward` / `native_backward` alone; `torch_over_native`;
  * SphereFace2 `bytes_over_copy`: the bytes the native path has to move (one read in the forward, a read and a write in the backward) divided by
    its time, as a share of the box's streaming-copy rate (the `box` block, first line); `peak_mb`: torch.cuda.max_memory_allocated of either path
    beyond the logits themselves, the native one with the in-place backward;
  * `max_abs_grad_diff`: the two gradients against each other (both fp32; information), and the two losses.

    python tools/bench_pairwise_losses.py [--log profiles/pairwise_losses_bench.log]

The one condition: the native forward + backward is faster than the torch expression at every size; the exit status and the last line say so.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'voiceprintrecognition-pytorch_amd'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_margin_loss import peak_mb, timed   # noqa: E402  (the same clock as the margin-loss table)

SF2_SIZES = (('C', 256, 5994), ('C', 512, 100000), ('A', 256, 5994), ('A', 512, 100000))
TRIPLET_SIZES = ((256, 192, 5994), (1024, 512, 5994))
SF2 = dict(margin=0.2, scale=32.0, lanbuda=0.7, t=3)
PER_SPEAKER = 32


def run_sphereface2(torch, margin_type, B, N, warmup, reps, copy_gbs):
    from mvector import _hip
    from mvector.loss import SphereFace2
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(B + N)
    logits = torch.rand((B, N), generator=gen, device=dev) * 1.9 - 0.95
    labels = torch.randint(0, N, (B,), generator=gen, device=dev)
    p = dict(SF2, margin_type=margin_type)
    module = SphereFace2(**p).to(dev)
    bias = module.bias
    one = torch.ones((), device=dev)
    out = torch.empty_like(logits)
    state = {}

    def native_forward():
        state['fwd'] = _hip.sphereface2_forward(logits, labels, bias, **p)

    def native_backward():
        state['bias_grad'] = _hip.sphereface2_backward(logits, labels, bias, state['fwd'][3], one, out=out, **p)[1]

    def native():
        native_forward()
        native_backward()

    def native_in_place(x):
        fwd = _hip.sphereface2_forward(x, labels, bias, **p)
        _hip.sphereface2_backward(x, labels, bias, fwd[3], one, out=x, **p)

    def eager():
        x = logits.detach().requires_grad_(True)
        bias.grad = None
        loss = module.torch_expression({'features': None, 'logits': x}, labels)
        loss.backward()
        state['eager'] = (loss.detach(), x.grad, bias.grad)

    rec = dict(loss='sphereface2_' + margin_type, B=B, N=N, logits_mb=round(B * N * 4 / 1e6, 1))
    rec['native'] = timed(torch, native, warmup, reps)
    rec['native_forward'] = timed(torch, native_forward, warmup, reps)
    rec['native_backward'] = timed(torch, native_backward, warmup, reps)
    rec['torch'] = timed(torch, eager, warmup, reps)
    moved = 3 * B * N * 4
    rec['bytes_gb_per_s'] = round(moved / (rec['native']['ms'] * 1e-3) / 1e9, 1)
    rec['bytes_over_copy'] = round(rec['bytes_gb_per_s'] / copy_gbs, 3) if copy_gbs else None
    native()
    eager()
    rec['loss_value'] = dict(native=float(state['fwd'][0]), torch=float(state['eager'][0]))
    rec['bias_grad'] = dict(native=float(state['bias_grad']), torch=float(state['eager'][2]))
    rec['max_abs_grad_diff'] = float((out - state['eager'][1]).abs().max())
    scratch = logits.clone()
    rec['peak_mb'] = dict(native_in_place=peak_mb(torch, lambda: native_in_place(scratch)), torch=peak_mb(torch, eager))
    rec['torch_over_native'] = round(rec['torch']['ms'] / rec['native']['ms'], 2)
    return rec


def run_triplet(torch, B, D, N, warmup, reps):
    from mvector import _hip
    from mvector.loss import TripletAngularMarginLoss
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(B + D)
    features = torch.randn((B, D), generator=gen, device=dev)
    logits = torch.rand((B, N), generator=gen, device=dev) * 1.9 - 0.95
    labels = torch.arange(B, device=dev) // PER_SPEAKER
    module = TripletAngularMarginLoss()
    p = dict(margin=module.margin, normalize=True, add_absolute=True, absolute_loss_weight=1.0, ap_value=0.8, an_value=0.4)
    ce_p = dict(kind='ce', margin=0.0, scale=1.0, label_smoothing=0.0)
    one = torch.ones((), device=dev)
    out_f, out_x = torch.empty_like(features), torch.empty_like(logits)
    state = {}

    def native_forward():
        state['tp'] = _hip.triplet_forward(features, labels, **p)
        state['ce'] = _hip.margin_ce_forward(logits, labels, **ce_p)
        state['loss'] = state['tp'][0] + state['ce'][0]

    def native_backward():
        _hip.triplet_backward(features, labels, state['tp'][1], state['tp'][2], one, out=out_f, **p)
        _hip.margin_ce_backward(logits, labels, state['ce'][3], one, out=out_x, **ce_p)

    def native():
        native_forward()
        native_backward()

    def eager():
        f, x = features.detach().requires_grad_(True), logits.detach().requires_grad_(True)
        loss = module.torch_expression({'features': f, 'logits': x}, labels)
        loss.backward()
        state['eager'] = (loss.detach(), f.grad, x.grad)

    rec = dict(loss='triplet+ce', B=B, D=D, N=N, fp64_madds_m=round(B * B * D / 1e6, 1))
    rec['native'] = timed(torch, native, warmup, reps)
    rec['native_forward'] = timed(torch, native_forward, warmup, reps)
    rec['native_backward'] = timed(torch, native_backward, warmup, reps)
    rec['native_triplet_forward'] = timed(torch, lambda: _hip.triplet_forward(features, labels, **p), warmup, reps)
    rec['torch'] = timed(torch, eager, warmup, reps)
    native()
    eager()
    rec['loss_value'] = dict(native=float(state['loss']), torch=float(state['eager'][0]))
    rec['max_abs_grad_diff'] = dict(features=float((out_f - state['eager'][1]).abs().max()), logits=float((out_x - state['eager'][2]).abs().max()))
    rec['torch_over_native'] = round(rec['torch']['ms'] / rec['native']['ms'], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--log', default=None)
    a = ap.parse_args()
    import torch
    import bench
    lines = [json.dumps(dict(box=bench.box_probe(torch.device('cuda:0'))))]
    print(lines[0], flush=True)
    copy_gbs = float(json.loads(lines[0])['box'].get('copy_gbs') or 0.0)
    ok = True
    jobs = [lambda mt=mt, B=B, N=N: run_sphereface2(torch, mt, B, N, a.warmup, a.reps, copy_gbs) for mt, B, N in SF2_SIZES]
    jobs += [lambda B=B, D=D, N=N: run_triplet(torch, B, D, N, a.warmup, a.reps) for B, D, N in TRIPLET_SIZES]
    for job in jobs:
        rec = job()
        ok = ok and rec['torch_over_native'] > 1.0
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    lines.append(json.dumps(dict(condition='the native forward + backward is faster than the torch expression at every size', met=ok)))
    print(lines[-1])
    if a.log:
        with open(a.log, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
