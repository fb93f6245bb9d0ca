"""Time the fused cosine + top-k search (csrc/search.hip, _hip.cosine_topk) against the path MVectorPredictor._best_matches ran before it, on
the same box.

  * seeded normal embeddings at D = 192 on the device: users in {10^4, 10^5, 10^6} x queries in {1, 16, 256}, k = 1 and k = 16;
  * `fused`: _hip.cosine_topk (workspace from torch's allocator per call, as the predictor calls it) -- HIP events around the call, and wall
    time of the call with the download of its [n, k] scores and indices (to_host=True: one transfer for both); 3 warm-ups, the median of 10;
  * `of_streaming_copy`: gallery bytes / event time as a share of the box's streaming-copy rate (the `box` block of bench.py, tools/boxprobe,
    which comes first) -- the gallery is the one thing the call has to stream;
  * `parent` (k = 1): the parent commit's path -- _hip.cosine, `.cpu().numpy()` of the [n, users] matrix, np.argmax per row -- wall time, the
    median of 3 runs (one run at 10^6 x 256, where the matrix is 1 GB);
  * `matrix_topk`, for information: _hip.cosine + torch.topk on the device (events; wall with the download of the [n, k] results);
  * every gallery size runs in a child process of its own under a time limit; the first failure ends the run.

    python tools/bench_search.py [--users 10000,100000,1000000] [--log profiles/search_bench.log]

The one condition: the fused call (wall, with its download) is faster than the parent path at every size (`parent_over_fused` > 1); the exit
status says so.  The top-1 of the fused call is compared with the parent path's answer (`same_as_parent`): it must be the same rows and scores.
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
QUERIES = (1, 16, 256)
KS = (1, 16)


def med(ts):
    return dict(ms=round(statistics.median(ts), 4), min=round(min(ts), 4), max=round(max(ts), 4))


def run_one(users, warmup, reps, parent_reps, copy_gbs):
    import numpy as np
    import torch
    from mvector import _hip
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dev = torch.device('cuda:0')
    _hip.lib()
    gen = torch.Generator(device=dev)
    gen.manual_seed(users)
    gallery = torch.randn((users, DIM), generator=gen, device=dev, dtype=torch.float32)
    all_queries = torch.randn((max(QUERIES), DIM), generator=gen, device=dev, dtype=torch.float32)
    gallery_bytes = users * DIM * 4

    def timed(fn, download, wall_fn=None, n_warm=warmup, n_reps=reps):
        """events around fn(); wall of fn() + download(result) (or of wall_fn(), which does both)"""
        wall_fn = wall_fn or (lambda: download(fn()))
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
            got = wall_fn()
            wl.append((time.perf_counter() - t0) * 1e3)
        return dict(events=med(ev), wall=med(wl)), got

    rows = []
    for n in QUERIES:
        q = all_queries[:n].contiguous()
        parent_answer = None
        for k in KS:
            rec = dict(users=users, queries=n, k=k, gallery_mb=round(gallery_bytes / 1e6, 1))
            rec['fused'], fused = timed(lambda: _hip.cosine_topk(q, gallery, k), lambda r: r,
                                        wall_fn=lambda: _hip.cosine_topk(q, gallery, k, to_host=True))
            rate = gallery_bytes / (rec['fused']['events']['ms'] * 1e-3) / 1e9
            rec['fused'].update(gallery_gb_per_s=round(rate, 1), of_streaming_copy=round(rate / copy_gbs, 3) if copy_gbs else None)
            rec['matrix_topk'], via_matrix = timed(lambda: torch.topk(_hip.cosine(q, gallery), k, dim=1),
                                                   lambda r: (r[0].cpu().numpy(), r[1].cpu().numpy()))
            rec['fused_over_matrix_topk_events'] = round(rec['fused']['events']['ms'] / rec['matrix_topk']['events']['ms'], 2)
            rec['same_scores_as_matrix_topk'] = bool(np.array_equal(fused[0], via_matrix[0]))   # (the index order among equal scores is torch's own)
            if k == 1:
                def parent():   # MVectorPredictor._best_matches of the parent commit, without the names
                    scores = _hip.cosine(q, gallery).cpu().numpy()
                    out = []
                    for row in scores:
                        best = int(np.argmax(row))
                        out.append((best, float(row[best])))
                    return out
                runs = 1 if n * users >= 200_000_000 else parent_reps
                parent()   # one warm-up: the allocator's first [n, users] block
                ts = []
                for _ in range(runs):
                    t0 = time.perf_counter()
                    parent_answer = parent()
                    ts.append((time.perf_counter() - t0) * 1e3)
                rec['parent'] = dict(wall=med(ts), runs=runs, matrix_mb=round(n * users * 4 / 1e6, 1))
                rec['same_as_parent'] = [(int(i), float(s)) for s, i in zip(fused[0][:, 0], fused[1][:, 0])] == parent_answer
                rec['parent_over_fused'] = round(rec['parent']['wall']['ms'] / rec['fused']['wall']['ms'], 1)
            rows.append(rec)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', default='10000,100000,1000000')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--parent-reps', type=int, default=3)
    ap.add_argument('--limit', type=int, default=300, help='seconds per gallery size')
    ap.add_argument('--log', default=None)
    ap.add_argument('--one', type=int, default=None, help='(child) run one gallery size and print its JSON lines')
    ap.add_argument('--copy-gbs', type=float, default=0.0, help='(child) the box\'s streaming-copy rate')
    ap.add_argument('--box-only', action='store_true', help='(child) print the box block')
    a = ap.parse_args()
    if a.one is not None:
        for rec in run_one(a.one, a.warmup, a.reps, a.parent_reps, a.copy_gbs):
            print('RESULT ' + json.dumps(rec))
        return
    if a.box_only:
        import torch
        import bench
        print('RESULT ' + json.dumps(dict(box=bench.box_probe(torch.device('cuda:0')))))
        return
    lines, copy_gbs, ok = [], 0.0, True
    steps = [['--box-only']] + [['--one', s] for s in a.users.split(',')]
    done = 0
    for extra in steps:
        cmd = [sys.executable, os.path.abspath(__file__), '--warmup', str(a.warmup), '--reps', str(a.reps), '--parent-reps', str(a.parent_reps),
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
            elif 'parent_over_fused' in rec and (rec['parent_over_fused'] <= 1.0 or not rec['same_as_parent']):
                ok = False
    text = '\n'.join(lines) + '\n'
    if not ok:
        print(lines[-1])
    if a.log:
        with open(a.log, 'w') as f:
            f.write(text)
    sys.exit(0 if ok and done == len(steps) else 1)


if __name__ == '__main__':
    main()
