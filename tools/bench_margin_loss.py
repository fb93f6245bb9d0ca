"""Time the fused margin-softmax losses (csrc/marginloss.hip: _hip.margin_ce_forward + _hip.margin_ce_backward) against the package's own
restated torch expression (mvector.loss.softmax_family.margin_logits + F.cross_entropy, PyTorch-ROCm eager with autograd) on the same fp32
logits and the same device.  One visit: HIP events around forward + backward, 3 warm-ups, the median of 10.

Sizes (B, N, K): AAM at (256, 5 994, 1) and (512, 100 000, 1), SubCenter at (256, 5 994, 3).  Per size:
  * `native` / `torch`: forward + backward in ms (native: backward into a second buffer, as autograd uses it); `torch_over_native`;
  * `native_forward` / `native_backward` alone, and `second_read`: margin_seg_kernel<.., 1> alone through the library's profiling hook
    (MV_PROF_MARGIN_SUMS) -- the pass that reads the logits a second time;
  * `bytes_over_copy`: the bytes the native path has to move (two reads in the forward, a read and a write in the backward) divided by its
    time, as a share of the box's streaming-copy rate (the `box` block, first line);
  * `peak_mb`: torch.cuda.max_memory_allocated of either path beyond the logits themselves, the native one with the in-place backward;
  * `max_abs_grad_diff`: the two gradients against each other (both fp32; information).

    python tools/bench_margin_loss.py [--log profiles/margin_loss_bench.log]

The one condition: the native forward + backward is faster than the torch expression at every size; the exit status and the last line say so.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'voiceprintrecognition-pytorch_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

SIZES = (('aam', 256, 5994, 1), ('aam', 512, 100000, 1), ('subcenter', 256, 5994, 3))
MARGIN, SCALE = 0.2, 32.0


def med(ts):
    return dict(ms=round(statistics.median(ts), 4), min=round(min(ts), 4), max=round(max(ts), 4))


def timed(torch, fn, n_warm, n_reps):
    for _ in range(n_warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n_reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return med(ts)


def peak_mb(torch, fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 1e6, 1)


def run_size(torch, lib, kind, B, N, K, warmup, reps, copy_gbs):
    import torch.nn.functional as F
    from mvector import _hip
    from mvector.loss.softmax_family import margin_logits
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(B + N)
    logits = torch.rand((B, N * K), generator=gen, device=dev) * 1.9 - 0.95
    labels = torch.randint(0, N, (B,), generator=gen, device=dev)
    p = dict(kind=kind, margin=MARGIN, scale=SCALE, K=K)
    one = torch.ones((), device=dev)
    out = torch.empty_like(logits)
    state = {}

    def native_forward():
        state['fwd'] = _hip.margin_ce_forward(logits, labels, **p)

    def native_backward():
        _hip.margin_ce_backward(logits, labels, state['fwd'][3], one, out=out, **p)

    def native():
        native_forward()
        native_backward()

    def native_in_place(x):
        fwd = _hip.margin_ce_forward(x, labels, **p)
        _hip.margin_ce_backward(x, labels, fwd[3], one, out=x, **p)

    def eager():
        x = logits.detach().requires_grad_(True)
        loss = F.cross_entropy(margin_logits(x, labels, kind, MARGIN, SCALE, False, K), labels)
        loss.backward()
        state['eager'] = (loss.detach(), x.grad)

    rec = dict(kind=kind, B=B, N=N, K=K, logits_mb=round(B * N * K * 4 / 1e6, 1))
    rec['native'] = timed(torch, native, warmup, reps)
    rec['native_forward'] = timed(torch, native_forward, warmup, reps)
    rec['native_backward'] = timed(torch, native_backward, warmup, reps)
    rec['torch'] = timed(torch, eager, warmup, reps)
    # the second read alone
    calls, ms, work = ctypes.c_int32(), ctypes.c_double(), ctypes.c_double()
    _hip.check(lib.mv_profile_enable(1))
    for _ in range(reps):
        native_forward()
    _hip.check(lib.mv_profile_read(4, ctypes.byref(calls), ctypes.byref(ms), ctypes.byref(work), 1))
    _hip.check(lib.mv_profile_enable(0))
    rec['second_read'] = dict(mean_ms=round(ms.value / max(calls.value, 1), 4), calls=calls.value,
                              gb_per_s=round(work.value / max(ms.value, 1e-9) / 1e6, 1))
    moved = 4 * B * N * K * 4
    rec['bytes_gb_per_s'] = round(moved / (rec['native']['ms'] * 1e-3) / 1e9, 1)
    rec['bytes_over_copy'] = round(rec['bytes_gb_per_s'] / copy_gbs, 3) if copy_gbs else None
    native()
    eager()
    rec['loss'] = dict(native=float(state['fwd'][0]), torch=float(state['eager'][0]))
    rec['max_abs_grad_diff'] = float((out - state['eager'][1]).abs().max())
    scratch = logits.clone()
    rec['peak_mb'] = dict(native_in_place=peak_mb(torch, lambda: native_in_place(scratch)), torch=peak_mb(torch, eager))
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
    from mvector import _hip
    lib = _hip.lib()
    lines = [json.dumps(dict(box=bench.box_probe(torch.device('cuda:0'))))]
    print(lines[0], flush=True)
    copy_gbs = float(json.loads(lines[0])['box'].get('copy_gbs') or 0.0)
    ok = True
    for kind, B, N, K in SIZES:
        rec = run_size(torch, lib, kind, B, N, K, a.warmup, a.reps, copy_gbs)
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
