"""Time the device down-mix + resampler (csrc/resample.hip) against the host code that predict_batch ran for such files before it, on the same box.

  * batch: 256 x 3 s of seeded int16 noise as 44.1 kHz stereo, 48 kHz mono and 8 kHz mono, to 16 kHz with dB normalisation to -20 dB.  Both sides start
    from the decoded int16 frames in memory: parsing the WAV container is the same work on either path;
  * device: HIP events and wall time, 3 warm-ups, the median of 10, of
      - the resampler call alone (mv_resampler_forward_i16 through _hip.Resampler on PCM that is already on the device; both launches), with its
        algorithmic bytes (2 C n_in + 4 n_out per row) per second as a fraction of the box's streaming-copy rate (the `box` block of bench.py,
        tools/boxprobe, which comes first),
      - staging + upload + call: the rows copied into one pinned int16 buffer, one upload, the call -- what predict_batch's 'pcm16_resampled' path
        does per (rate, channels) group -- until the device has finished;
  * host yard-stick: what the parent commit does for the same files -- per file the float conversion and channel mean (AudioSegment), resample
    (scipy.signal.resample_poly), normalize, then the zero-padded float32 batch and its upload -- wall time, the median of --host-reps runs;
  * every format runs in a child process of its own under a time limit; the first failure ends the run.

    python tools/bench_resample.py [--formats 44100x2,48000x1,8000x1] [--log profiles/resample_bench.log]

The one condition: staging + upload + call is faster than the host yard-stick at every format (`host_over_device` > 1); the exit status says so.
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

TARGET_RATE, TARGET_DB = 16000, -20.0


def med(ts):
    return dict(ms=round(statistics.median(ts), 3), min=round(min(ts), 3), max=round(max(ts), 3))


def run_one(rate, channels, batch, seconds, warmup, reps, host_reps, copy_gbs):
    import numpy as np
    import torch
    from mvector import _hip
    from mvector.data_utils.audio import AudioSegment
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dev = torch.device('cuda:0')
    rs = _hip.Resampler(rate, TARGET_RATE)
    n_in = int(rate * seconds)
    n_out = rs.out_len(n_in)
    rng = np.random.default_rng(rate + channels)
    files = [np.round(3000.0 * rng.standard_normal((n_in, channels))).clip(-32768, 32767).astype(np.int16) for _ in range(batch)]
    out = dict(src_rate=rate, channels=channels, batch=batch, n_in=n_in, n_out=n_out, up=rs.up, down=rs.down, K=rs.K, tile=rs.tile,
               table_in_lds=rs.table_in_lds)

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

    resident = torch.from_numpy(np.stack(files)).to(dev)
    out['call'] = timed(lambda: rs(resident, target_db=TARGET_DB))
    moved = batch * (2 * channels * n_in + 4 * n_out)
    rate_gbs = moved / (out['call']['events']['ms'] * 1e-3) / 1e9
    out['call'].update(algorithmic_bytes=moved, gb_per_s=round(rate_gbs, 1), of_streaming_copy=round(rate_gbs / copy_gbs, 3) if copy_gbs else None)
    out['call_unnormalised'] = timed(lambda: rs(resident))
    del resident

    staging = torch.zeros((batch, n_in, channels), dtype=torch.int16).pin_memory()
    got = []

    def device_path():
        host = staging.numpy()
        for i, f in enumerate(files):
            host[i] = f
        wav, _, quiet = rs(staging.to(dev, non_blocking=True), target_db=TARGET_DB)
        got[:] = [wav, quiet]
    out['staging_upload_call'] = timed(device_path)

    def host_path():   # the parent commit's predict_batch for these files, from the decoded frames on
        rows = []
        for f in files:
            seg = AudioSegment(f, rate)
            seg.resample(TARGET_RATE)
            seg.normalize(target_db=TARGET_DB)
            rows.append(seg.samples)
        longest = max(r.shape[0] for r in rows)
        inputs = np.zeros((len(rows), longest), dtype=np.float32)
        for i, r in enumerate(rows):
            inputs[i, :r.shape[0]] = r
        wav = torch.from_numpy(inputs).to(dev)
        torch.cuda.synchronize()
        return wav

    ts, want = [], None
    for _ in range(host_reps):
        t0 = time.perf_counter()
        want = host_path()
        ts.append((time.perf_counter() - t0) * 1e3)
    out['host'] = dict(wall=med(ts), runs=host_reps)
    out['max_abs_diff_to_host'] = float((got[0] - want).abs().max().item())
    out['host_over_device'] = round(out['host']['wall']['ms'] / out['staging_upload_call']['wall']['ms'], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--formats', default='44100x2,48000x1,8000x1')
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--seconds', type=float, default=3.0)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--limit', type=int, default=300, help='seconds per format')
    ap.add_argument('--log', default=None)
    ap.add_argument('--one', default=None, help='(child) run one format and print its JSON line')
    ap.add_argument('--copy-gbs', type=float, default=0.0, help='(child) the box\'s streaming-copy rate')
    ap.add_argument('--box-only', action='store_true', help='(child) print the box block')
    a = ap.parse_args()
    if a.one is not None:
        rate, channels = (int(v) for v in a.one.split('x'))
        print('RESULT ' + json.dumps(run_one(rate, channels, a.batch, a.seconds, a.warmup, a.reps, a.host_reps, a.copy_gbs)))
        return
    if a.box_only:
        import torch
        import bench
        print('RESULT ' + json.dumps(dict(box=bench.box_probe(torch.device('cuda:0')))))
        return
    lines, copy_gbs, ok = [], 0.0, True
    steps = [['--box-only']] + [['--one', s] for s in a.formats.split(',')]
    for extra in steps:
        cmd = [sys.executable, os.path.abspath(__file__), '--batch', str(a.batch), '--seconds', str(a.seconds), '--warmup', str(a.warmup),
               '--reps', str(a.reps), '--host-reps', str(a.host_reps), '--copy-gbs', str(copy_gbs)] + extra
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
