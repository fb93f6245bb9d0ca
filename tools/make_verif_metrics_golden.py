"""Generate tests/golden/verif_metrics.npz by running the REFERENCE's own mvector/metric/metrics.py (compute_fnr_fpr, compute_eer, compute_dcf of
the reference checkout, loaded by path) on seeded score matrices.

Run where the reference checkout exists (oracle/make_golden.py: REF):

    python tools/make_verif_metrics_golden.py

Only data is written.  Per case <name>: <name>_scores (fp32, flat, trial-major), <name>_trial_labels / <name>_enroll_labels (int32),
<name>_costs (p_target, c_miss, c_fa), <name>_eer / <name>_min_dcf (fp64), <name>_threshold (fp32) and, for the smaller cases, <name>_fnr / <name>_fpr
(fp64) and <name>_thresholds (fp32).

Scores: seeded 192-d speaker centres plus Gaussian noise, cast to fp32 and normalised in fp32, scores = a @ b.T in fp32.  Before a case is written the
tool asserts what keeps a test on it from hiding a failure:
  * no target score equals an impostor score (numpy's default argsort leaves the order of equal scores open: with such a tie the reference's own
    arrays are one of several valid answers and no yardstick),
  * 0 < eer < 0.5 (a separable list never exercises the interpolation),
  * the stable-sort restatement of this package (metrics.verification_metrics on numpy input) is bit-equal to the reference in everything stored.
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'voiceprintrecognition-pytorch_amd')]
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
DIM = 192

# name: (seed, speakers, trials, enrolments, noise sigma, (p_target, c_miss, c_fa), store the curves)
CASES = {
    'main': (2, 12, 300, 97, 2.5, (0.01, 1, 1), False),       # 29 100 scores: several tiles of the sort, the crossing far from the first one
    'tiny': (1, 3, 7, 5, 3.0, (0.01, 1, 1), True),            # a few dozen scores
    'costs': (5, 8, 120, 41, 2.5, (0.05, 10, 1), True),       # non-default costs; 4920 scores = more than one tile, with the curves
}


def import_reference():
    from oracle.make_golden import REF
    spec = importlib.util.spec_from_file_location('ref_metrics', os.path.join(REF, 'mvector', 'metric', 'metrics.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def synth_scores(seed, speakers, n_trials, n_enroll, sigma):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((speakers, DIM))
    tl = rng.integers(speakers, size=n_trials)
    el = rng.integers(speakers, size=n_enroll)

    def embed(labels):
        x = (centres[labels] + sigma * rng.standard_normal((labels.shape[0], DIM))).astype(np.float32)
        return x / np.linalg.norm(x, axis=1, keepdims=True).astype(np.float32)

    a, b = embed(tl), embed(el)
    scores = a @ b.T
    assert scores.dtype == np.float32
    return scores, tl.astype(np.int32), el.astype(np.int32)


def make_case(ref, name, seed, speakers, n_trials, n_enroll, sigma, costs, curves):
    from mvector.metric.metrics import verification_metrics
    scores, tl, el = synth_scores(seed, speakers, n_trials, n_enroll, sigma)
    flat = scores.reshape(-1)
    labels = (tl[:, None] == el[None, :]).astype(np.int32).reshape(-1)
    tgt, imp = flat[labels == 1], flat[labels == 0]
    cross = np.intersect1d(tgt, imp).size
    same = flat.size - np.unique(flat).size
    assert cross == 0, f'{name}: {cross} target scores equal an impostor score'
    p_target, c_miss, c_fa = costs
    fnr, fpr, thresholds = ref.compute_fnr_fpr(flat, labels)
    eer, threshold = ref.compute_eer(fnr, fpr, flat)
    min_dcf = ref.compute_dcf(fnr, fpr, p_target=p_target, c_miss=c_miss, c_fa=c_fa)
    assert 0 < eer < 0.5, f'{name}: eer {eer}'
    mine = verification_metrics(scores, tl, el, p_target=p_target, c_miss=c_miss, c_fa=c_fa, return_curve=True)
    assert mine[:3] == (float(eer), float(min_dcf), float(threshold)), (name, mine[:3], eer, min_dcf, threshold)
    assert np.array_equal(mine[3], fnr) and np.array_equal(mine[4], fpr) and np.array_equal(mine[5], thresholds), name
    i1 = int(np.flatnonzero(fnr - fpr >= 0)[0])
    print(f'{name}: N = {flat.size}, {int(labels.sum())} targets, {same} equal scores of one label, 0 across labels, crossing at sorted position {i1}, '
          f'EER {eer:.5f}, minDCF {min_dcf:.5f}, threshold {threshold:.5f}')
    out = {f'{name}_scores': flat, f'{name}_trial_labels': tl, f'{name}_enroll_labels': el, f'{name}_costs': np.array(costs, dtype=np.float64),
           f'{name}_eer': np.float64(eer), f'{name}_min_dcf': np.float64(min_dcf), f'{name}_threshold': np.float32(threshold)}
    if curves:
        out.update({f'{name}_fnr': fnr, f'{name}_fpr': fpr, f'{name}_thresholds': thresholds})
    return out


def main():
    ref = import_reference()
    out = {}
    for name, (seed, speakers, n_trials, n_enroll, sigma, costs, curves) in CASES.items():
        for attempt in range(20):   # the first of seed, seed + 1000, ... whose scores meet the conditions is used and stored
            try:
                out.update(make_case(ref, name, seed + 1000 * attempt, speakers, n_trials, n_enroll, sigma, costs, curves))
                out[f'{name}_seed'] = np.int64(seed + 1000 * attempt)
                break
            except AssertionError as e:
                print(f'  seed {seed + 1000 * attempt} not used: {e}')
        else:
            raise SystemExit(f'{name}: no seed met the conditions')
    path = os.path.join(GOLDEN, 'verif_metrics.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20, os.path.getsize(path)
    print('done ->', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
