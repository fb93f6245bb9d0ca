"""Time the device clustering of speaker diarization (cosine -> pruned affinity / Laplacian -> lowest eigenpairs, csrc/diarize.hip) against the host
classes of mvector/infer_utils/speaker_diarization.py (numpy / scipy, the reference's arithmetic) on the same box.

  * synthetic embeddings: seeded 192-d speaker centres plus Gaussian noise in contiguous turns, N = 600 / 2400 / 4800 chunks (an hour of speech at a
    0.75 s shift is about 4800);
  * device: HIP events around each stage and wall time around the whole SpectralCluster call on a device tensor (k_means on the host included),
    3 warm-ups, the median of 10;
  * host: wall time of the same SpectralCluster call on the numpy embeddings and of its stages (similarity, pruning loop, scipy.linalg.eigh in fp32);
    the median of 3 runs without warm-up (eigh alone takes seconds at N = 4800);
  * the product L X is not an entry point of its own: its time is reported as an upper bound, eigen-solver wall time / products with L (the b x b host
    work and the stream synchronisations of the call are inside it), with the launch plan (row tile, K slices) beside it;
  * every N runs in a child process of its own under a time limit; the first failure ends the run;
  * the `box` block of bench.py (tools/boxprobe) of the box the run landed on comes first.

    python tools/bench_diarization.py [--sizes 600,2400,4800] [--log profiles/diarization_bench.log]

There is no pass bar: the parent of this tool could not run the clustering on the device at all.
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

PT_ROWS, PT_K, PT_TARGET_WGS, PT_MAX_SLICES = 128, 32, 512, 16   # the launch plan of csrc/diarize.hip (eig_plan), restated for the log


def launch_plan(n):
    row_tiles = -(-n // PT_ROWS)
    want = min(max(-(-PT_TARGET_WGS // row_tiles), 1), PT_MAX_SLICES)
    k_per_slice = -(-(-(-n // want)) // PT_K) * PT_K   # ceil(ceil(n / want) / PT_K) * PT_K
    return dict(row_tile=PT_ROWS, k_tile=PT_K, row_tiles=row_tiles, k_slices=-(-n // k_per_slice), k_per_slice=k_per_slice)


def synth(n, speakers, sigma=0.8, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed + n)
    centres = rng.standard_normal((speakers, 192))
    who = []
    while len(who) < n:
        who += [int(rng.integers(speakers))] * int(rng.integers(3, 31))
    who = np.array(who[:n])
    return (centres[who] + sigma * rng.standard_normal((n, 192))).astype(np.float32)


def wall(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(ms=round(statistics.median(ts), 3), min=round(min(ts), 3), max=round(max(ts), 3))


def run_one(n, warmup, reps, host_reps):
    import numpy as np
    import scipy.linalg
    import torch
    from mvector import _hip
    from mvector.infer_utils.speaker_diarization import SpeakerDiarization, SpectralCluster
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dev = torch.device('cuda:0')
    _hip.lib()
    speakers = 4 if n < 1000 else 8
    X = synth(n, speakers)
    Xd = torch.from_numpy(X).to(dev)
    sc = SpectralCluster()
    n_prune = sc.n_prune(n)
    out = dict(N=n, speakers=speakers, n_prune=n_prune, product_plan=launch_plan(n))

    def events(fn):
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

    sim = _hip.cosine(Xd, Xd)
    M, degree = _hip.affinity_laplacian(sim, n_prune)
    lam, vecs, info = _hip.laplacian_eig_lowest(M, degree, m=16)
    out['device'] = dict(cosine=events(lambda: _hip.cosine(Xd, Xd)), affinity_laplacian=events(lambda: _hip.affinity_laplacian(sim, n_prune)),
                         eig_events=events(lambda: _hip.laplacian_eig_lowest(M, degree, m=16)),
                         eig_wall=wall(lambda: _hip.laplacian_eig_lowest(M, degree, m=16), 1, reps), eig_info=info)
    out['device']['ms_per_product_upper_bound'] = round(out['device']['eig_wall']['ms'] / info['products'], 4)
    labels_dev = []
    out['device']['spectral_cluster_call_wall'] = wall(lambda: labels_dev.append(SpeakerDiarization._correct_labels(sc(Xd))), warmup, reps)

    host = {}
    t0 = time.perf_counter()
    S = sc.get_sim_mat(X)
    host['similarity_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
    t0 = time.perf_counter()
    P = sc.p_pruning(S.copy())
    L = sc.get_laplacian(0.5 * (P + P.T))
    host['pruning_laplacian_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
    t0 = time.perf_counter()
    lam_host = scipy.linalg.eigh(L)[0]
    host['eigh_fp32_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
    labels_host = []
    host['spectral_cluster_call_wall'] = wall(lambda: labels_host.append(SpeakerDiarization._correct_labels(sc(X.copy()))), 0, host_reps)
    out['host'] = host
    ub = info['ub']
    out['agreement'] = dict(labels_equal=bool(np.array_equal(labels_dev[-1], labels_host[-1])), speakers_found=int(labels_dev[-1].max() + 1),
                            eigenvalues_vs_host_fp32_eigh_of_ub=float(np.abs(lam - lam_host[:16]).max() / ub))
    out['speedup_whole_call'] = round(host['spectral_cluster_call_wall']['ms'] / out['device']['spectral_cluster_call_wall']['ms'], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='600,2400,4800')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--limit', type=int, default=240, help='seconds per size')
    ap.add_argument('--log', default=None)
    ap.add_argument('--one', type=int, default=None, help='(child) run one size and print its JSON line')
    ap.add_argument('--box-only', action='store_true', help='(child) print the box block')
    a = ap.parse_args()
    if a.one is not None:
        print('RESULT ' + json.dumps(run_one(a.one, a.warmup, a.reps, a.host_reps)))
        return
    if a.box_only:
        import torch
        import bench
        print('RESULT ' + json.dumps(dict(box=bench.box_probe(torch.device('cuda:0')))))
        return
    lines = []
    steps = [['--box-only']] + [['--one', s] for s in a.sizes.split(',')]
    for extra in steps:
        cmd = [sys.executable, os.path.abspath(__file__), '--warmup', str(a.warmup), '--reps', str(a.reps), '--host-reps', str(a.host_reps)] + extra
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            lines.append(json.dumps(dict(step=extra, error=f'time limit of {a.limit} s')))
            break
        got = [l[7:] for l in r.stdout.splitlines() if l.startswith('RESULT ')]
        if r.returncode != 0 or not got:
            lines.append(json.dumps(dict(step=extra, returncode=r.returncode, stderr=r.stderr[-2000:])))
            break   # nothing more is started on the device after a failure
        lines.append(got[0])
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.log:
        with open(a.log, 'w') as f:
            f.write(text)
    sys.exit(0 if len(lines) == len(steps) else 1)


if __name__ == '__main__':
    main()
