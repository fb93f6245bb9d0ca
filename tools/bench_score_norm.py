"""Time the cohort score normalisation (csrc/scorenorm.hip: _hip.cohort_stats, _hip.score_norm) against the host recipe it replaces, on the
same box.

  * seeded normal embeddings at D = 192 on the device; sizes (rows, M, top_n) = (5 000, 6 000, 300), (20 000, 20 000, 300) and
    (100 000, 32 768, 400), rows being the enrolment and test embeddings together; and a 4 096 x 4 096 S-normalisation;
  * `stats`: _hip.cohort_stats (workspace from torch's allocator per call) -- HIP events around the call, and wall time of the call with the
    download of mean and std; 3 warm-ups, the median of 10;
  * `cosine_chunks`: the same chunks of rows through _hip.cosine alone, into one buffer of a chunk's size (events); `select` = stats - cosine_chunks,
    the time of cohort_topn_stats_kernel by difference (the library has no entry point that runs it alone); `select_bytes_over_copy`: the
    rows x M x 4 bytes the kernel reads / the box's streaming-copy rate (the `box` block of bench.py, which comes first), as a share of `select`;
  * `matrix_topk`, for information: _hip.cosine + torch.topk + mean / std (population) on the device (events; 3 runs, 1 at the largest size);
  * `host`: the yard-stick on the same box's CPUs -- numpy L2-normalise, one fp32 matmul, np.partition for the top N, mean / std -- wall time,
    the median of 3 runs (1 run at the largest size, where the matrix is walked in blocks of 16 384 rows: 13 GB at once help nobody);
  * `norm`: _hip.score_norm on 4 096 x 4 096 (events and wall with nothing to download: the matrix stays for the metrics) against the numpy
    float32 expression on the host;
  * every size runs in a child process of its own under a time limit; the first failure ends the run.

    python tools/bench_score_norm.py [--log profiles/score_norm_bench.log]

The one condition: the device path is faster than the host yard-stick at every size (`host_over_device` > 1, wall against wall); the exit status
and the last line of the log say so.
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

DIM = 192
SIZES = ((5000, 6000, 300), (20000, 20000, 300), (100000, 32768, 400))
NORM = 4096
HOST_BLOCK = 16384


def med(ts):
    return dict(ms=round(statistics.median(ts), 4), min=round(min(ts), 4), max=round(max(ts), 4))


def timed(torch, fn, wall_fn, n_warm, n_reps):
    """events around fn(); wall of wall_fn() (the call with whatever comes down)"""
    for _ in range(n_warm):
        wall_fn()
    torch.cuda.synchronize()
    ev, wl = [], []
    for _ in range(n_reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ev.append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        wall_fn()
        torch.cuda.synchronize()
        wl.append((time.perf_counter() - t0) * 1e3)
    return dict(events=med(ev), wall=med(wl))


def host_stats(np, x, cohort, top_n):
    xn = x / np.linalg.norm(x, axis=1, keepdims=True)
    cn = cohort / np.linalg.norm(cohort, axis=1, keepdims=True)
    block = HOST_BLOCK if x.shape[0] * cohort.shape[0] > (1 << 30) else x.shape[0]
    mean, std = np.empty(x.shape[0], dtype=np.float32), np.empty(x.shape[0], dtype=np.float32)
    for r0 in range(0, x.shape[0], block):
        scores = xn[r0:r0 + block] @ cn.T
        top = np.partition(scores, scores.shape[1] - top_n, axis=1)[:, -top_n:]
        mean[r0:r0 + block], std[r0:r0 + block] = top.mean(axis=1), top.std(axis=1)
    return mean, std


def run_size(index, warmup, reps, host_reps, copy_gbs):
    import numpy as np
    import torch
    from mvector import _hip
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dev = torch.device('cuda:0')
    lib = _hip.lib()
    rows, m, top_n = SIZES[index]
    largest = index == len(SIZES) - 1
    gen = torch.Generator(device=dev)
    gen.manual_seed(rows + m)
    x = torch.randn((rows, DIM), generator=gen, device=dev, dtype=torch.float32)
    cohort = torch.randn((m, DIM), generator=gen, device=dev, dtype=torch.float32)
    chunk = int(lib.mv_cohort_stats_workspace_bytes(rows, m, DIM, 0)) // (m * 4)
    rec = dict(rows=rows, cohort=m, top_n=top_n, chunk_rows=chunk, scores_mb=round(rows * m * 4 / 1e6, 1))

    def download():
        mean, std = _hip.cohort_stats(x, cohort, top_n)
        return mean.cpu().numpy(), std.cpu().numpy()
    rec['stats'] = timed(torch, lambda: _hip.cohort_stats(x, cohort, top_n), download, warmup, reps)
    buf = torch.empty((chunk, m), dtype=torch.float32, device=dev)

    def cosine_chunks():
        for r0 in range(0, rows, chunk):
            n = min(chunk, rows - r0)
            _hip.check(lib.mv_cosine_f32(x[r0:r0 + n].data_ptr(), n, cohort.data_ptr(), m, DIM, buf.data_ptr(), _hip.current_stream(x)))
    rec['cosine_chunks'] = timed(torch, cosine_chunks, cosine_chunks, warmup, reps)['events']
    select_ms = rec['stats']['events']['ms'] - rec['cosine_chunks']['ms']
    ideal_ms = rows * m * 4 / (copy_gbs * 1e9) * 1e3 if copy_gbs else None
    rec['select'] = dict(ms=round(select_ms, 4), select_bytes_over_copy=round(ideal_ms / select_ms, 3) if ideal_ms and select_ms > 0 else None)

    def matrix_topk():
        top = torch.topk(_hip.cosine(x, cohort), top_n, dim=1)[0]
        return top.mean(dim=1), top.std(dim=1, unbiased=False)
    rec['matrix_topk'] = timed(torch, matrix_topk, matrix_topk, 1, 1 if largest else 3)['events']
    del buf
    torch.cuda.empty_cache()
    xh, ch = x.cpu().numpy(), cohort.cpu().numpy()
    runs = 1 if largest else host_reps
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        hm, hs = host_stats(np, xh, ch, top_n)
        ts.append((time.perf_counter() - t0) * 1e3)
    rec['host'] = dict(wall=med(ts), runs=runs)
    dm, ds = download()
    rec['max_abs_diff_to_host'] = dict(mean=float(np.abs(dm - hm).max()), std=float(np.abs(ds - hs).max()))
    rec['host_over_device'] = round(rec['host']['wall']['ms'] / rec['stats']['wall']['ms'], 1)
    return rec


def run_norm(warmup, reps, host_reps):
    import numpy as np
    import torch
    from mvector import _hip
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dev = torch.device('cuda:0')
    _hip.lib()
    gen = torch.Generator(device=dev)
    gen.manual_seed(NORM)
    s = torch.randn((NORM, NORM), generator=gen, device=dev) * 0.2
    tm, em = torch.randn(NORM, generator=gen, device=dev) * 0.1, torch.randn(NORM, generator=gen, device=dev) * 0.1
    ts_, es = torch.rand(NORM, generator=gen, device=dev) * 0.1 + 0.01, torch.rand(NORM, generator=gen, device=dev) * 0.1 + 0.01
    out = torch.empty_like(s)
    call = lambda: _hip.score_norm(s, (tm, ts_), (em, es), 's', out=out)
    rec = dict(norm=f'{NORM} x {NORM}', mode='s', device=timed(torch, call, call, warmup, reps))
    h = [v.cpu().numpy() for v in (s, tm, ts_, em, es)]
    ts = []
    for _ in range(host_reps):
        t0 = time.perf_counter()
        want = np.float32(0.5) * ((h[0] - h[1][:, None]) / h[2][:, None] + (h[0] - h[3][None, :]) / h[4][None, :])
        ts.append((time.perf_counter() - t0) * 1e3)
    rec['host'] = dict(wall=med(ts), runs=host_reps)
    rec['equal_bits'] = bool(np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)))
    rec['bytes_gb_per_s'] = round(2 * NORM * NORM * 4 / (rec['device']['events']['ms'] * 1e-3) / 1e9, 1)
    rec['host_over_device'] = round(rec['host']['wall']['ms'] / rec['device']['wall']['ms'], 1)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--limit', type=int, default=400, help='seconds per step')
    ap.add_argument('--log', default=None)
    ap.add_argument('--one', type=int, default=None, help='(child) run one size and print its JSON line')
    ap.add_argument('--norm-only', action='store_true', help='(child) time the normalisation')
    ap.add_argument('--copy-gbs', type=float, default=0.0, help='(child) the box\'s streaming-copy rate')
    ap.add_argument('--box-only', action='store_true', help='(child) print the box block')
    a = ap.parse_args()
    if a.one is not None:
        print('RESULT ' + json.dumps(run_size(a.one, a.warmup, a.reps, a.host_reps, a.copy_gbs)))
        return
    if a.norm_only:
        print('RESULT ' + json.dumps(run_norm(a.warmup, a.reps, a.host_reps)))
        return
    if a.box_only:
        import torch
        import bench
        print('RESULT ' + json.dumps(dict(box=bench.box_probe(torch.device('cuda:0')))))
        return
    lines, copy_gbs, ok = [], 0.0, True
    steps = [['--box-only']] + [['--one', str(i)] for i in range(len(SIZES))] + [['--norm-only']]
    done = 0
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
        done += 1
        for line in got:
            lines.append(line)
            print(line, flush=True)
            rec = json.loads(line)
            if 'box' in rec:
                copy_gbs = float(rec['box'].get('copy_gbs') or 0.0)
            elif rec.get('host_over_device', 0.0) <= 1.0 or rec.get('equal_bits') is False:
                ok = False
    ok = ok and done == len(steps)
    lines.append(json.dumps(dict(condition='the device path is faster than the host yard-stick at every size', met=ok)))
    print(lines[-1])
    if a.log:
        with open(a.log, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
