"""Time the energy VAD (csrc/vad.hip: _hip.vad_energy, mvector.infer_utils.vad.EnergyVad) against its own numpy path on the same box.

  * one seeded recording of 1, 10 and 60 minutes at 16 kHz: bursts of amplitude-modulated noise (1 to 4 s, 0.4 to 1.5 s apart) over a noise
    floor, resident on the device; compute-vad's default settings and the VoxCeleb recipe's (5.5 / 0.5 / context 2 / 0.12);
  * `native`: _hip.vad_energy (outputs and workspace from torch's allocator per call) -- HIP events around the call;
    `wall`: EnergyVad on the CUDA tensor -- the native call, the download of the run list and the smoothing on the host, ended by the
    synchronisation the download is; 3 warm-ups, the median of 10;
  * `bytes_over_copy`: the bytes the five launches move by the shapes (4 L of samples read; per frame logE written and read, the decision
    written and read twice, 8 + 8 + 3 bytes) / the box's streaming-copy rate (the `box` block of bench.py, which comes first), as a share
    of `native`;
  * `host`: the yard-stick on the same box's CPUs -- EnergyVad on the numpy array -- wall time, the median of 3 runs;
  * `segments_equal`: the two paths return the same segments;
  * --bench: bench.py --gpus 1 on the same visit, its value against the spread of the committed runs (77.3 k .. 81.4 k utt/s): no existing
    kernel changes with the VAD;
  * every size runs in a child process of its own under a time limit; the first failure ends the run.

    python tools/bench_vad.py [--bench] [--log profiles/vad_bench.log]

The one condition: the device path with its download is faster than the host yard-stick at every length (`host_over_device` > 1, wall against
wall); the exit status and the last line of the log say so.
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

MINUTES = (1, 10, 60)
SETTINGS = {'default': dict(), 'recipe': dict(energy_threshold=5.5, frames_context=2, proportion_threshold=0.12)}
SPREAD = (77.3e3, 81.4e3)   # utt/s of the committed bench.py runs (profiles/README.md)


def med(ts):
    return dict(ms=round(statistics.median(ts), 4), min=round(min(ts), 4), max=round(max(ts), 4))


def recording(np, minutes, sr=16000, seed=3):
    rng = np.random.default_rng(seed + minutes)
    n = minutes * 60 * sr
    x = (3e-4 * rng.standard_normal(n)).astype(np.float32)
    t = int(rng.uniform(0.2, 1.0) * sr)
    while t < n:
        d = min(int(rng.uniform(1.0, 4.0) * sr), n - t)
        tt = np.arange(d, dtype=np.float32) / sr
        x[t:t + d] += (0.1 * (1.0 + 0.3 * np.sin(2 * np.pi * 3.0 * tt)) * rng.standard_normal(d)).astype(np.float32)
        t += d + int(rng.uniform(0.4, 1.5) * sr)
    return x


def run_size(minutes, warmup, reps, host_reps, copy_gbs):
    import numpy as np
    import torch
    from mvector import _hip
    from mvector.infer_utils.vad import EnergyVad
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dev = torch.device('cuda:0')
    _hip.lib()
    x = recording(np, minutes)
    wav = torch.from_numpy(x).to(dev)
    rec = dict(minutes=minutes, samples=int(x.shape[0]))
    for name, kw in SETTINGS.items():
        vad = EnergyVad(**kw)
        T = vad.num_frames(x.shape[0])
        for _ in range(warmup):
            vad(wav)
        torch.cuda.synchronize()
        ev, wl = [], []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _hip.vad_energy(wav, **vad.cfg)
            e1.record()
            torch.cuda.synchronize()
            ev.append(e0.elapsed_time(e1))
            t0 = time.perf_counter()
            segs = vad(wav)
            wl.append((time.perf_counter() - t0) * 1e3)
        ts = []
        for _ in range(host_reps):
            t0 = time.perf_counter()
            host = vad(x)
            ts.append((time.perf_counter() - t0) * 1e3)
        moved = 4 * x.shape[0] + 19 * T
        one = dict(frames=T, segments=len(segs), native=med(ev), wall=med(wl), host=dict(wall=med(ts), runs=host_reps), segments_equal=segs == host,
                   moved_mb=round(moved / 1e6, 2), gb_per_s=round(moved / (statistics.median(ev) * 1e-3) / 1e9, 1))
        one['bytes_over_copy'] = round(moved / (copy_gbs * 1e9) * 1e3 / statistics.median(ev), 4) if copy_gbs else None
        one['host_over_device'] = round(one['host']['wall']['ms'] / one['wall']['ms'], 1)
        rec[name] = one
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--limit', type=int, default=400, help='seconds per step')
    ap.add_argument('--log', default=None)
    ap.add_argument('--bench', action='store_true', help='also run bench.py --gpus 1 and hold its value against the committed spread')
    ap.add_argument('--one', type=int, default=None, help='(child) run one length (minutes) and print its JSON line')
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
    steps = [me + ['--box-only']] + [me + ['--one', str(m)] for m in MINUTES]
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
            for name in SETTINGS:
                if name in rec and (rec[name]['host_over_device'] <= 1.0 or not rec[name]['segments_equal']):
                    ok = False
    ok = ok and done == len(steps)
    lines.append(json.dumps(dict(condition='the device path with its download is faster than the host yard-stick at every length', met=ok)))
    print(lines[-1])
    if a.log:
        with open(a.log, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
