"""Time the device verification metrics (csrc/verif.hip: radix sort of the trial scores + metric scan) against the host code that
MVectorTrainer.evaluate(use_gpu=True) ran before them, on the same box.

  * scores: seeded uniform fp32 on the device, N = 2^20 (1024 x 1024), 2^24 (4096 x 4096) and 10^8 (10000 x 10000) trials; labels drawn from 100
    speakers on either side, so 1 % of the trials are targets;
  * device: HIP events and wall time, 3 warm-ups, the median of 10, of
      - the sort alone (mv_sort_scores_f32 on buffers allocated once),
      - the whole native call (mv_verif_metrics_f32 on a workspace allocated once; it synchronises) -- the scan is not an entry point of its own, its
        time is reported as the difference of the two event medians,
      - the whole Python call metrics.verification_metrics on the device tensors (allocates its workspace per call), which is what evaluate runs;
  * host yard-stick: the code of the parent commit's evaluate on the same scores -- download of the score matrix, the int32 label matrix,
    compute_fnr_fpr + compute_eer + compute_dcf -- wall time, the median of --host-reps runs (one run from 5 * 10^7 trials on: it takes tens of seconds);
  * the bytes the sort moves per second as a fraction of the box's streaming-copy rate (the `box` block of bench.py, tools/boxprobe, which comes
    first).  Bytes: per pass the count kernel reads the keys (4 N), the scatter kernel reads keys and indices (8 N; the first pass reads the
    scores only, 4 N) and writes both (8 N), and the [digit][tile] table is written once, read twice and rewritten once;
  * every size runs in a child process of its own under a time limit; the first failure ends the run.

    python tools/bench_verif_metrics.py [--sizes 1024x1024,4096x4096,10000x10000] [--log profiles/verif_metrics_bench.log]

The one condition: the whole device call is faster than the host yard-stick at every size (`host_over_device` > 1); the exit status says so.
Uniform scores at these sizes hold equal target and impostor scores, where numpy's default argsort and the device's flat-index rule may order them
differently: `same_floats_as_host` is reported, not asserted.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'voiceprintrecognition-pytorch_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

DIGITS, SCAN_TABLE_ACCESSES = 256, 4   # the pass structure of csrc/verif.hip, restated for the byte count


def sort_bytes(n, tile):
    tiles = -(-n // tile)
    return 4 * (4 * n + 8 * n + 8 * n) - 4 * n + 4 * SCAN_TABLE_ACCESSES * DIGITS * tiles * 4


def med(ts):
    return dict(ms=round(statistics.median(ts), 3), min=round(min(ts), 3), max=round(max(ts), 3))


def run_one(shape, warmup, reps, host_reps, copy_gbs):
    import numpy as np
    import torch
    from mvector import _hip
    from mvector.metric import metrics
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dev = torch.device('cuda:0')
    lib = _hip.lib()
    n_trials, n_enroll = shape
    n = n_trials * n_enroll
    gen = torch.Generator(device=dev)
    gen.manual_seed(n)
    scores = torch.rand((n_trials, n_enroll), generator=gen, device=dev, dtype=torch.float32)
    rng = np.random.default_rng(n)
    tl_host = rng.integers(100, size=n_trials).astype(np.int32)
    el_host = rng.integers(100, size=n_enroll).astype(np.int32)
    tl, el = torch.from_numpy(tl_host).to(dev), torch.from_numpy(el_host).to(dev)
    stream = _hip.current_stream(scores)
    tile = int(lib.mv_sort_scores_tile())
    out = dict(N=n, n_trials=n_trials, n_enroll=n_enroll, tile=tile, tiles=-(-n // tile))

    def timed(fn):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ev, wl = [], []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            wl.append((time.perf_counter() - t0) * 1e3)
            ev.append(e0.elapsed_time(e1))
        return dict(events=med(ev), wall=med(wl))

    sorted_scores = torch.empty((n,), dtype=torch.float32, device=dev)
    index = torch.empty((n,), dtype=torch.int32, device=dev)
    sort_ws = torch.empty((int(lib.mv_sort_scores_workspace_bytes(n)),), dtype=torch.uint8, device=dev)
    do_sort = lambda: _hip.check(lib.mv_sort_scores_f32(scores.data_ptr(), n, sorted_scores.data_ptr(), index.data_ptr(), sort_ws.data_ptr(),
                                                        sort_ws.numel(), stream))
    out['sort'] = timed(do_sort)
    moved = sort_bytes(n, tile)
    rate = moved / (out['sort']['events']['ms'] * 1e-3) / 1e9
    out['sort'].update(bytes_moved=moved, gb_per_s=round(rate, 1), of_streaming_copy=round(rate / copy_gbs, 3) if copy_gbs else None)
    del sort_ws, index, sorted_scores

    ws = torch.empty((int(lib.mv_verif_metrics_workspace_bytes(n_trials, n_enroll)),), dtype=torch.uint8, device=dev)
    cfg, res = _hip.MvVerifCfg(0.01, 1.0, 1.0), _hip.MvVerifResult()
    do_native = lambda: _hip.check(lib.mv_verif_metrics_f32(scores.data_ptr(), n_trials, n_enroll, tl.data_ptr(), el.data_ptr(), ctypes.byref(cfg),
                                                            ctypes.byref(res), None, None, ws.data_ptr(), ws.numel(), stream))
    out['native_call'] = timed(do_native)
    out['scan_ms_by_difference'] = round(out['native_call']['events']['ms'] - out['sort']['events']['ms'], 3)
    out['workspace_bytes'] = ws.numel()
    del ws

    got = []
    out['python_call'] = timed(lambda: got.append(metrics.verification_metrics(scores, tl, el)))
    out['result'] = got[-1]
    out['same_on_every_call'] = all(g == got[0] for g in got)

    def host():   # the host half of the parent commit's evaluate(use_gpu=True)
        s = scores.cpu().numpy()
        all_score = s.astype(np.float32).reshape(-1)
        all_labels = (tl_host[:, None] == el_host[None, :]).astype(np.int32).reshape(-1)
        fnr, fpr, _ = metrics.compute_fnr_fpr(all_score, all_labels)
        eer, threshold = metrics.compute_eer(fnr, fpr, all_score)
        return float(eer), float(metrics.compute_dcf(fnr, fpr)), float(threshold)

    runs = host_reps if n < 50_000_000 else 1
    ts, want = [], None
    for _ in range(runs):
        t0 = time.perf_counter()
        want = host()
        ts.append((time.perf_counter() - t0) * 1e3)
    out['host'] = dict(wall=med(ts), runs=runs, result=want)
    out['same_floats_as_host'] = got[-1] == want
    out['host_over_device'] = round(out['host']['wall']['ms'] / out['python_call']['wall']['ms'], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='1024x1024,4096x4096,10000x10000')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--limit', type=int, default=400, help='seconds per size')
    ap.add_argument('--log', default=None)
    ap.add_argument('--one', default=None, help='(child) run one size and print its JSON line')
    ap.add_argument('--copy-gbs', type=float, default=0.0, help='(child) the box\'s streaming-copy rate')
    ap.add_argument('--box-only', action='store_true', help='(child) print the box block')
    a = ap.parse_args()
    if a.one is not None:
        shape = tuple(int(v) for v in a.one.split('x'))
        print('RESULT ' + json.dumps(run_one(shape, a.warmup, a.reps, a.host_reps, a.copy_gbs)))
        return
    if a.box_only:
        import torch
        import bench
        print('RESULT ' + json.dumps(dict(box=bench.box_probe(torch.device('cuda:0')))))
        return
    lines, copy_gbs, ok = [], 0.0, True
    steps = [['--box-only']] + [['--one', s] for s in a.sizes.split(',')]
    for extra in steps:
        cmd = [sys.executable, os.path.abspath(__file__), '--warmup', str(a.warmup), '--reps', str(a.reps), '--host-reps', str(a.host_reps),
               '--copy-gbs', str(copy_gbs)] + extra
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            lines.append(json.dumps(dict(step=extra, error=f'time limit of {a.limit} s')))
            ok = False
            break
        got = [l[7:] for l in r.stdout.splitlines() if l.startswith('RESULT ')]
        if r.returncode != 0 or not got:
            lines.append(json.dumps(dict(step=extra, returncode=r.returncode, stderr=r.stderr[-2000:])))
            ok = False
            break   # nothing more is started on the device after a failure
        lines.append(got[0])
        print(got[0], flush=True)
        rec = json.loads(got[0])
        if 'box' in rec:
            copy_gbs = float(rec['box'].get('copy_gbs') or 0.0)
        elif rec['host_over_device'] <= 1.0:
            ok = False
    text = '\n'.join(lines) + '\n'
    if not ok:
        print(lines[-1])
    if a.log:
        with open(a.log, 'w') as f:
            f.write(text)
    sys.exit(0 if ok and len(lines) == len(steps) else 1)


if __name__ == '__main__':
    main()
