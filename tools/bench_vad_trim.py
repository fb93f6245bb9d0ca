"""Time the speech-only preparation of a batch on the device (EnergyVad.trim: csrc/vad.hip, mv_vad_energy_f32 -> mv_vad_regions_i32 ->
mv_wave_gather_f32) against what the tree offered for the same result before: the device VAD with its run-list download, then the host.

  * one seeded batch of 256 rows of 3 s and of 10 s at 16 kHz, resident on the device: bursts of amplitude-modulated noise (0.3 to 1.2 s) over
    a noise floor, the gaps drawn so that about 40 % of a row is silence; compute-vad's default settings and smoothing;
  * `native`: the three calls (outputs and workspaces from torch's allocator per call) -- HIP events around them;
    `gather`: HIP events around _hip.wave_gather alone; its bytes by the shapes (4 bytes read per kept sample, 4 written per output sample, the
    region table) over its time, as a share of the box's streaming-copy rate (the `box` block of bench.py, which comes first);
    `wall`: EnergyVad.trim on the CUDA tensor and the download of the [B] kept counts, which is the synchronisation the predictor adds;
    3 warm-ups, the median of 10;
  * `host`: the yard-stick on the same box -- EnergyVad.__call__ on the device tensor (device VAD, run-list download, numpy smoothing), the download
    of the waveform, slicing and concatenation in numpy, the upload of the padded result -- wall time, the median of 3 runs;
  * `equal`: both give the same kept counts (the yard-stick's regions are rounded to seconds and back, so its samples are compared only where the
    counts agree);
  * --bench: bench.py --gpus 1 on the same visit, its value against the spread of the committed runs: no existing kernel changes;
  * every size runs in a child process of its own under a time limit; the first failure ends the run.

    python tools/bench_vad_trim.py [--bench] [--log profiles/vad_trim_bench.log]

The one condition: the device path with its download is faster than the yard-stick at both sizes (`host_over_device` > 1, wall against wall); the
exit status and the last line of the log say so.
"""
import argparse
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

SECONDS = (3, 10)
ROWS = 256
SPREAD = (77.3e3, 81.4e3)   # utt/s of the committed bench.py runs (profiles/README.md)


def med(ts):
    return dict(ms=round(statistics.median(ts), 4), min=round(min(ts), 4), max=round(max(ts), 4))


def batch(np, seconds, rows=ROWS, sr=16000, seed=5):
    """[rows, seconds * sr] fp32: a 3e-4 noise floor with bursts of 0.1 amplitude, about 40 % of a row left silent"""
    rng = np.random.default_rng(seed + seconds)
    n = seconds * sr
    x = (3e-4 * rng.standard_normal((rows, n))).astype(np.float32)
    for b in range(rows):
        t = int(rng.uniform(0.1, 0.5) * sr)
        while t < n:
            d = min(int(rng.uniform(0.3, 1.2) * sr), n - t)
            tt = np.arange(d, dtype=np.float32) / sr
            x[b, t:t + d] += (0.1 * (1.0 + 0.3 * np.sin(2 * np.pi * 3.0 * tt)) * rng.standard_normal(d)).astype(np.float32)
            t += d + int(rng.uniform(0.4, 0.75) * sr)
    return x


def yardstick(np, torch, vad, wav):
    """what the parent commit offers: device VAD + run-list download + numpy smoothing, waveform download, numpy slicing, upload"""
    segs = vad(wav)
    host = wav.cpu().numpy()
    out = np.zeros(host.shape, dtype=np.float32)
    kept = []
    for b, row in enumerate(segs):
        parts = [host[b, int(round(s['start'] * vad.sample_rate)):int(round(s['end'] * vad.sample_rate))] for s in row]
        cat = np.concatenate(parts) if parts else np.zeros(0, dtype=np.float32)
        out[b, :cat.shape[0]] = cat
        kept.append(cat.shape[0])
    dev = torch.from_numpy(out).to(wav.device)
    torch.cuda.synchronize()
    return dev, kept


def run_size(seconds, warmup, reps, host_reps, copy_gbs):
    import numpy as np
    import torch
    from mvector import _hip
    from mvector.infer_utils.vad import EnergyVad
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dev = torch.device('cuda:0')
    _hip.lib()
    x = batch(np, seconds)
    wav = torch.from_numpy(x).to(dev)
    vad = EnergyVad()
    for _ in range(warmup):
        vad.trim(wav)[1].cpu()
    torch.cuda.synchronize()
    ev, gv, wl = [], [], []
    for _ in range(reps):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        num_regions, regions, kept, _ = vad._device_regions(wav, None)
        e1.record()
        out, _ = _hip.wave_gather(wav, None, num_regions, regions)
        e2.record()
        torch.cuda.synchronize()
        ev.append(e0.elapsed_time(e2))
        gv.append(e1.elapsed_time(e2))
        t0 = time.perf_counter()
        trimmed, k = vad.trim(wav)
        k_host = k.cpu()
        wl.append((time.perf_counter() - t0) * 1e3)
    ts = []
    for _ in range(host_reps):
        t0 = time.perf_counter()
        ref, ref_kept = yardstick(np, torch, vad, wav)
        ts.append((time.perf_counter() - t0) * 1e3)
    k_list = k_host.tolist()
    same = [b for b in range(ROWS) if k_list[b] == ref_kept[b]]
    samples_equal = bool(torch.equal(trimmed[same], ref[same]))
    moved = 4 * sum(k_list) + 4 * x.size + 8 * int(num_regions.sum().item())
    rec = dict(seconds=seconds, rows=ROWS, samples=int(x.size), kept_share=round(sum(k_list) / x.size, 3), regions=int(num_regions.sum().item()),
               native=med(ev), gather=med(gv), wall=med(wl), host=dict(wall=med(ts), runs=host_reps), rows_with_equal_counts=len(same),
               samples_equal_there=samples_equal, gather_moved_mb=round(moved / 1e6, 2), gather_gb_per_s=round(moved / (statistics.median(gv) * 1e-3) / 1e9, 1))
    rec['gather_share_of_copy_rate'] = round(moved / (statistics.median(gv) * 1e-3) / (copy_gbs * 1e9), 4) if copy_gbs else None
    rec['host_over_device'] = round(rec['host']['wall']['ms'] / rec['wall']['ms'], 1)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--limit', type=int, default=400, help='seconds per step')
    ap.add_argument('--log', default=None)
    ap.add_argument('--bench', action='store_true', help='also run bench.py --gpus 1 and hold its value against the committed spread')
    ap.add_argument('--one', type=int, default=None, help='(child) run one row length (seconds) and print its JSON line')
    ap.add_argument('--copy-gbs', type=float, default=0.0, help='(child) the box\'s streaming-copy rate')
    ap.add_argument('--box-only', action='store_true', help='(child) print the box block')
    a = ap.parse_args()
    if a.one is not None:
        print('RESULT ' + json.dumps(run_size(a.one, a.warmup, a.reps, a.host_reps, a.copy_gbs)))
        return
    if a.box_only:
        import torch
        import bench
        print('RESULT ' + json.dumps(dict(box=bench.box_probe(torch.device('cuda:0')))))
        return
    lines, copy_gbs, ok = [], 0.0, True
    me = [sys.executable, os.path.abspath(__file__), '--warmup', str(a.warmup), '--reps', str(a.reps), '--host-reps', str(a.host_reps)]
    steps = [me + ['--box-only']] + [me + ['--one', str(s)] for s in SECONDS]
    if a.bench:
        steps.append([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1'])
    done = 0
    for cmd in steps:
        is_bench = cmd[1].endswith('bench.py')
        try:
            r = subprocess.run(cmd + ([] if is_bench else ['--copy-gbs', str(copy_gbs)]), capture_output=True, text=True, timeout=a.limit, cwd=ROOT)
        except subprocess.TimeoutExpired:
            lines.append(json.dumps(dict(step=cmd[1:], error=f'time limit of {a.limit} s')))
            ok = False
            break
        if is_bench:
            got = [json.dumps(dict(bench_py={k: v for k, v in json.loads(l).items() if k in ('metric', 'value', 'unit', 'n_gpus', 'model', 'batch', 'steps')},
                                   committed_spread=list(SPREAD), inside_committed_spread=SPREAD[0] <= float(json.loads(l).get('value', 0.0)) <= SPREAD[1]))
                   for l in r.stdout.splitlines() if l.startswith('{') and '"value"' in l][-1:]
        else:
            got = [l[7:] for l in r.stdout.splitlines() if l.startswith('RESULT ')]
        if r.returncode != 0 or not got:
            lines.append(json.dumps(dict(step=cmd[1:], returncode=r.returncode, stderr=r.stderr[-2000:])))
            ok = False
            break   # nothing more is started on the device after a failure
        done += 1
        for line in got:
            lines.append(line)
            print(line, flush=True)
            rec = json.loads(line)
            if 'box' in rec:
                copy_gbs = float(rec['box'].get('copy_gbs') or 0.0)
            if 'host_over_device' in rec and rec['host_over_device'] <= 1.0:
                ok = False
    ok = ok and done == len(steps)
    lines.append(json.dumps(dict(condition='the device path with its download is faster than the yard-stick at both sizes', met=ok)))
    print(lines[-1])
    if a.log:
        with open(a.log, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
