"""Generate the golden fixtures of the speaker-diarization host layer (tests/golden/diarization_*.npz, diarization_misc.json) by running the
REFERENCE's own SpectralCluster and SpeakerDiarization (mvector/infer_utils/speaker_diarization.py of the reference checkout) on seeded inputs.

Run where the reference checkout exists (oracle/make_golden.py: REF), with scipy and scikit-learn installed:

    python tools/make_diarization_golden.py

The reference file imports yeaudio for one type annotation only; a stub module stands in for it.  Only data is written.

Inputs: seeded 192-d speaker centres plus Gaussian noise, contiguous turns of 3-30 chunks.  Before anything is written the tool asserts what
keeps a test on these inputs from hiding a failure:
  * the reference's labels are identical over 5 runs of its unseeded k_means,
  * the largest eigen-gap is at least 4 x the second largest (so fp32 eigh, fp64 eigh and the device solver agree on the speaker count),
  * no row has equal values on the two sides of the pruning cut (numpy's argsort leaves the order of ties open).
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'voiceprintrecognition-pytorch_amd')]
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

# (N, speakers, noise sigma, first seed tried: the first of seed, seed + 1000, ... whose input meets the conditions is used and stored); the similarity matrix is stored up to SIM_MAX_N (it is dense: 4 N^2 bytes)
CASES = [(33, 2, 0.6, 33), (40, 3, 0.6, 40), (300, 3, 0.8, 300), (301, 5, 0.7, 301), (700, 4, 1.0, 700), (1200, 8, 0.8, 1200)]
SIM_MAX_N = 301
DIM = 192


def import_reference():
    from oracle.make_golden import REF
    stub = types.ModuleType('yeaudio.audio')
    stub.AudioSegment = object
    pkg = types.ModuleType('yeaudio')
    pkg.audio = stub
    sys.modules.setdefault('yeaudio', pkg)
    sys.modules.setdefault('yeaudio.audio', stub)
    spec = importlib.util.spec_from_file_location('ref_speaker_diarization', os.path.join(REF, 'mvector', 'infer_utils', 'speaker_diarization.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def synth_embeddings(n, speakers, sigma, seed):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((speakers, DIM))
    who = []
    while len(who) < n:
        spk = int(rng.integers(speakers))
        if who and who[-1] == spk:
            continue
        who += [spk] * int(rng.integers(3, 31))
    who = np.array(who[:n])
    # rounded to fp16 values: the fixture stores them as fp16 (half the bytes; the N = 1200 file stays below the size limit), every user widens them exactly
    return (centres[who] + sigma * rng.standard_normal((n, DIM))).astype(np.float16).astype(np.float32), who


def cluster_case(ref, n, speakers, sigma, seed):
    X, who = synth_embeddings(n, speakers, sigma, seed)
    sc = ref.SpectralCluster()
    sim = sc.get_sim_mat(X)
    assert sim.dtype == np.float32
    pval = 6. / n if n * sc.pval < 6 else sc.pval
    n_prune = int((1 - pval) * n)
    srt = np.sort(sim, axis=1)
    assert n_prune == 0 or not np.any(srt[:, n_prune - 1] == srt[:, n_prune]), f'N={n}: a row has equal values across the pruning cut'
    pruned = sc.p_pruning(sim.copy())
    sym = 0.5 * (pruned + pruned.T)
    lap = sc.get_laplacian(sym)          # zeroes the diagonal of `sym` in place
    import scipy.linalg
    lambdas = scipy.linalg.eigh(lap)[0]
    gaps = np.sort(np.array(sc.get_eigen_gaps(lambdas[sc.min_num_spks - 1:sc.max_num_spks + 1])))[::-1]
    assert gaps[0] >= 4 * gaps[1], f'N={n}: eigen-gap ratio {gaps[0] / gaps[1]:.2f} < 4'
    sd = ref.SpeakerDiarization()
    runs = []
    for _ in range(5):
        labels = sd._correct_labels(sc(X.copy()))
        runs.append(labels)
        assert np.array_equal(labels, runs[0]), f'N={n}: the reference\'s own labels differ between runs of k_means'
    assert runs[0].max() + 1 == speakers, (n, runs[0].max() + 1)
    merged, centres = sd.clustering(X.copy())
    segments = [[0.75 * i, 0.75 * i + 1.5, None] for i in range(n)]
    post = sd.postprocess(segments, merged.copy())
    post = [dict(speaker=int(p['speaker']), start=float(p['start']), end=float(p['end'])) for p in post]
    out = dict(X=X.astype(np.float16), who=who, n_prune=np.int64(n_prune), M=sym, L=lap, lambdas16=lambdas[:16].astype(np.float64), labels=runs[0].astype(np.int64),
               centres=centres.astype(np.float32), merged=np.asarray(merged).astype(np.int64), gap_ratio=np.float64(gaps[0] / gaps[1]),
               postprocess=np.array(json.dumps(post)))
    if n <= SIM_MAX_N:
        out['sim'] = sim
    from mvector.infer_utils.speaker_diarization import SpectralCluster
    same = np.array_equal(SpectralCluster.get_sim_mat(X), sim)
    print(f'N={n}: speakers {speakers}, n_prune {n_prune}, gap ratio {gaps[0] / gaps[1]:.1f}, merged speakers {merged.max() + 1}, turns {len(post)}, '
          f'this package\'s similarity bit-equal to sklearn\'s here: {same}')
    return out


def chunk_cases(ref):
    """_chunk on regions below, at and above one chunk and at a non-multiple of the shift (1 kHz keeps the rows small)"""
    sd = ref.SpeakerDiarization(sample_rate=1000)
    out = {}
    for name, n in (('below', 900), ('exact', 1500), ('above', 3000), ('ragged', 4100), ('one_over', 1501)):
        data = np.arange(1, n + 1, dtype=np.float32)
        segs = sd._chunk([[2.5, 2.5 + n / 1000, data]])
        out[f'{name}_n'] = np.int64(n)
        out[f'{name}_times'] = np.array([[s[0], s[1]] for s in segs], dtype=np.float64)
        out[f'{name}_rows'] = np.stack([s[2] for s in segs]).astype(np.float32)
    return out


def misc_cases(ref):
    sd = ref.SpeakerDiarization()
    rng = np.random.default_rng(7)
    base = rng.standard_normal((3, 16))
    merge = []
    # pair_above: centres 1 and 2 are close (above 0.78) and far from centre 0 (below): one merge.  (The reference does not re-index the centres after
    # a merge: a close pair (0, 1) would be compared again under the new labels and swallow speaker 2 as well -- all_merge shows a chain.)
    for name, centres in (('pair_above', np.stack([base[2], base[0], base[0] + 0.3 * base[1]])),
                          ('pair_below', np.stack([base[0], base[0] + 1.2 * base[1], base[2]])),
                          ('all_merge', np.stack([base[0], base[0] + 0.1 * base[1], base[0] + 0.1 * base[2]]))):
        labels = np.array([0, 0, 1, 1, 2, 2, 1, 0, 2])
        unit = centres / np.linalg.norm(centres, axis=1, keepdims=True)
        out = sd._merge_by_cos(labels.copy(), list(centres), 0.78)
        merge.append(dict(name=name, labels=labels.tolist(), centres=centres.tolist(), cos=np.triu(unit @ unit.T, 1).tolist(), threshold=0.78,
                          out=np.asarray(out).tolist()))
    assert merge[0]['cos'][1][2] >= 0.78 > max(merge[0]['cos'][0][1], merge[0]['cos'][0][2])
    assert max(max(r) for r in merge[1]['cos']) < 0.78
    smooth = []
    for name, res in (('first_short', [[0.0, 0.5, 0], [0.5, 3.0, 1], [3.0, 6.0, 0]]),
                      ('middle_short_left', [[0.0, 3.0, 0], [3.0, 3.6, 1], [4.0, 7.0, 2]]),
                      ('middle_short_right', [[0.0, 3.0, 0], [3.4, 3.9, 1], [4.0, 7.0, 2]]),
                      ('last_short', [[0.0, 3.0, 0], [3.0, 6.0, 1], [6.0, 6.4, 0]]),
                      ('nothing_short', [[0.0, 3.004, 0], [3.004, 6.0, 1]])):
        out = sd._smooth([list(r) for r in res])
        smooth.append(dict(name=name, res=res, out=[[float(r[0]), float(r[1]), int(r[2])] for r in out]))
    post = []
    for name, segs, labels in (('overlap_split', [[0.0, 1.5], [0.75, 2.25], [1.5, 3.0], [2.25, 3.75], [3.0, 4.5], [3.75, 5.25]], [0, 0, 0, 1, 1, 1]),
                               ('gap_kept', [[0.0, 1.5], [0.75, 2.25], [5.0, 6.5], [5.75, 7.25]], [0, 0, 0, 0])):
        out = sd.postprocess([s + [None] for s in segs], np.array(labels))
        post.append(dict(name=name, segments=segs, labels=labels, out=[dict(speaker=int(o['speaker']), start=float(o['start']), end=float(o['end'])) for o in out]))
    return dict(merge=merge, smooth=smooth, postprocess=post)


def main():
    ref = import_reference()
    for n, speakers, sigma, seed in CASES:
        path = os.path.join(GOLDEN, f'diarization_{n}.npz')
        for attempt in range(20):
            try:
                case = cluster_case(ref, n, speakers, sigma, seed + 1000 * attempt)
                break
            except AssertionError as e:
                print(f'  seed {seed + 1000 * attempt} not used: {e}')
        else:
            raise SystemExit(f'N={n}: no seed met the conditions')
        np.savez_compressed(path, seed=np.int64(seed + 1000 * attempt), **case)
        assert os.path.getsize(path) < 1 << 20, (path, os.path.getsize(path))
    np.savez_compressed(os.path.join(GOLDEN, 'diarization_chunks.npz'), **chunk_cases(ref))
    with open(os.path.join(GOLDEN, 'diarization_misc.json'), 'w') as f:
        json.dump(misc_cases(ref), f, indent=0)
    print('done ->', GOLDEN)


if __name__ == '__main__':
    main()
