"""Checks of the verification-metric kernels (csrc/verif.hip) shared by tests/test_verif_metrics.py (the emulator build, CPU tensors) and
tests/test_gpu_verif_metrics.py (the product library on the device).  Each takes the bound library (None = the product library) and a device.

Every bar here is equality.  The sort is a permutation fixed by numpy.argsort(kind='stable'); the metrics are integer counts and single
correctly rounded fp64 operations in the reference's order, so the reference's own floats (tests/golden/verif_metrics.npz, written by
tools/make_verif_metrics_golden.py from the reference's metrics.py) are the expected values, not something near them."""
import ctypes
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN

CASES = ('main', 'tiny', 'costs')
SORT_KINDS = ('normal', 'ties17', 'special', 'sorted', 'reversed')


def sort_tile(cdll):
    from mvector import _hip
    return int((cdll or _hip.lib()).mv_sort_scores_tile())


def sort_sizes(tile):
    return [1, 2, 63, 64, 65, 255, 256, 257, tile - 1, tile, tile + 1, 3 * tile + 5]


_GOLDEN = {}


def golden():
    if not _GOLDEN:
        z = np.load(os.path.join(GOLDEN, 'verif_metrics.npz'))
        for k in z.files:
            _GOLDEN[k] = z[k]
            _GOLDEN[k].setflags(write=False)
    return _GOLDEN


def case(name):
    g = golden()
    tl, el = g[f'{name}_trial_labels'], g[f'{name}_enroll_labels']
    p_target, c_miss, c_fa = g[f'{name}_costs'].tolist()
    c_miss, c_fa = (int(c) if c == int(c) else c for c in (c_miss, c_fa))   # the reference was called with integer costs
    return g[f'{name}_scores'].reshape(tl.shape[0], el.shape[0]), tl, el, dict(p_target=p_target, c_miss=c_miss, c_fa=c_fa)


def sort_input(kind, n):
    rng = np.random.default_rng(100 + n)
    if kind == 'normal':
        return rng.standard_normal(n).astype(np.float32)
    if kind == 'ties17':   # heavy ties: the carried index shows whether every pass is stable
        return rng.standard_normal(17).astype(np.float32)[rng.integers(17, size=n)]
    if kind == 'special':
        bits = lambda u: np.array(u, dtype=np.uint32).view(np.float32)
        pool = np.concatenate([
            np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-40, -1e-40, 1.17549435e-38], dtype=np.float32),
            bits([0x3F800000 + i for i in range(6)]), bits([0xBF800000 + i for i in range(6)]),          # only the lowest byte differs
            bits([(h << 24) | 0x00345678 for h in (0x01, 0x3F, 0x40, 0x7E, 0x81, 0xBF, 0xC0, 0xFE)]),    # only the highest byte differs
            bits([0x7FC00000, 0xFFC00000, 0x7F800001])])                                                 # three NaNs, one negative, one signalling
        x = pool[rng.integers(pool.shape[0], size=n)]
        x[:min(n, pool.shape[0])] = pool[rng.permutation(pool.shape[0])[:min(n, pool.shape[0])]]          # every value at least once when n allows
        return x
    x = np.sort(rng.standard_normal(n).astype(np.float32))
    return x if kind == 'sorted' else x[::-1].copy()


def check_sort(cdll, device, n, kinds=SORT_KINDS):
    from mvector import _hip
    for kind in kinds:
        x = sort_input(kind, n)
        got, idx = _hip.sort_scores(torch.from_numpy(x.copy()).to(device), cdll=cdll)
        order = np.argsort(x, kind='stable')
        assert idx.dtype == torch.int32 and np.array_equal(idx.cpu().numpy(), order), f'{kind} N={n}: the carried index is not the stable argsort'
        assert np.array_equal(got.cpu().numpy(), x[order], equal_nan=True), f'{kind} N={n}: sorted scores differ'


def check_golden(cdll, device, name):
    """the raw counts, the EER / minDCF / threshold made of them and the curve against the reference's floats"""
    from mvector import _hip
    from mvector.metric import metrics
    g = golden()
    scores, tl, el, costs = case(name)
    t = lambda a: torch.from_numpy(np.array(a)).to(device)
    r = _hip.verification_metrics(t(scores), t(tl), t(el), curve=True, cdll=cdll, **costs)
    n = scores.size
    labels = (tl[:, None] == el[None, :]).reshape(-1)
    order = np.argsort(scores.reshape(-1), kind='stable')
    tgt_cum = np.cumsum(labels[order])
    assert r['n_target'] == labels.sum() and r['n_impostor'] == n - labels.sum()
    assert np.array_equal(r['tgt_cum'].cpu().numpy(), tgt_cum) and np.array_equal(r['sorted_scores'].cpu().numpy(), scores.reshape(-1)[order])
    eer = metrics._eer_from_counts(r['n_target'], r['n_impostor'], r['i1'], r['tgt_i1'], r['i2'], r['tgt_i2'])
    min_dcf = r['min_cost'] / min(costs['c_miss'] * costs['p_target'], costs['c_fa'] * (1 - costs['p_target']))
    print(f'{name}: N={n} i1={r["i1"]} i2={r["i2"]} eer={eer!r} (golden {float(g[name + "_eer"])!r}) min_dcf={min_dcf!r} '
          f'(golden {float(g[name + "_min_dcf"])!r}) threshold={r["score_i1"]!r} (golden {float(g[name + "_threshold"])!r})')
    assert eer == g[f'{name}_eer'] and min_dcf == g[f'{name}_min_dcf'] and np.float32(r['score_i1']) == g[f'{name}_threshold']
    if name == 'main':
        assert r['i1'] >= sort_tile(cdll), 'the crossing of this case is meant to lie outside the first tile'
    return r


def check_golden_public(device, name, cdll=None):
    """metrics.verification_metrics on numpy input (device None: the host restatement) or on tensors of `device`"""
    from mvector import _hip
    from mvector.metric import metrics
    g = golden()
    scores, tl, el, costs = case(name)
    if device is None:
        args = (scores, tl, el)
    else:
        args = tuple(torch.from_numpy(np.array(a)).to(device) for a in (scores, tl, el))
    out = metrics.verification_metrics(*args, return_curve=True, **costs)
    assert all(type(v) is float for v in out[:3])
    assert out[0] == g[f'{name}_eer'] and out[1] == g[f'{name}_min_dcf'] and np.float32(out[2]) == g[f'{name}_threshold'], (name, out[:3])
    assert metrics.verification_metrics(*args, **costs) == out[:3]
    fnr, fpr, thresholds = out[3:]
    assert fnr.dtype == fpr.dtype == np.float64 and thresholds.dtype == np.float32
    if f'{name}_fnr' in g:
        assert np.array_equal(fnr, g[f'{name}_fnr']) and np.array_equal(fpr, g[f'{name}_fpr']) and np.array_equal(thresholds, g[f'{name}_thresholds'])
    else:   # no curve stored for this case: the host restatement, itself bit-equal to the reference when the fixture was made
        want = metrics.verification_metrics(scores, tl, el, return_curve=True, **costs)
        assert np.array_equal(fnr, want[3]) and np.array_equal(fpr, want[4]) and np.array_equal(thresholds, want[5])


TIE_SCORES = np.array([[0.1, 0.5, 0.3, 0.5],
                       [0.5, 0.2, 0.5, 0.9],
                       [0.4, 0.5, 0.6, 0.5]], dtype=np.float32)
TIE_TRIALS = np.array([7, 8, 9], dtype=np.int32)
TIE_ENROLL = np.array([7, 8, 9, 7], dtype=np.int32)


def check_cross_label_ties(cdll, device, second_stream=False):
    """six scores of 0.5 astride the crossing, one of them a target (flat index 3) among five impostors (flat 1, 4, 6, 9, 11): the order is the
    flat index, so the target is the second of the six; the result is that of the kind='stable' host restatement, and the same on a second call /
    a second stream"""
    from mvector import _hip
    from mvector.metric import metrics
    labels = (TIE_TRIALS[:, None] == TIE_ENROLL[None, :]).reshape(-1)
    flat = TIE_SCORES.reshape(-1)
    tied = flat == np.float32(0.5)
    assert labels[tied].any() and not labels[tied].all()                     # a target and an impostor share the score ...
    t = lambda a: torch.from_numpy(a.copy()).to(device)
    r = _hip.verification_metrics(t(TIE_SCORES), t(TIE_TRIALS), t(TIE_ENROLL), curve=True, cdll=cdll)
    order = np.argsort(flat, kind='stable')
    assert flat[order][r['i1']] == np.float32(0.5) or flat[order][r['i2']] == np.float32(0.5)   # ... across the crossing
    assert np.array_equal(r['tgt_cum'].cpu().numpy(), np.cumsum(labels[order]))
    want = metrics.verification_metrics(TIE_SCORES, TIE_TRIALS, TIE_ENROLL)
    eer = metrics._eer_from_counts(r['n_target'], r['n_impostor'], r['i1'], r['tgt_i1'], r['i2'], r['tgt_i2'])
    assert (float(eer), float(r['min_cost'] / 0.01), float(r['score_i1'])) == want, (eer, r, want)
    strip = lambda d: {k: (v.cpu().numpy().tolist() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    if second_stream:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            r2 = _hip.verification_metrics(t(TIE_SCORES), t(TIE_TRIALS), t(TIE_ENROLL), curve=True, cdll=cdll)
        torch.cuda.current_stream().wait_stream(side)
        assert strip(r2) == strip(r)
    assert strip(_hip.verification_metrics(t(TIE_SCORES), t(TIE_TRIALS), t(TIE_ENROLL), curve=True, cdll=cdll)) == strip(r)
    if device != 'cpu':
        assert metrics.verification_metrics(t(TIE_SCORES), t(TIE_TRIALS), t(TIE_ENROLL)) == want


def _public(device, scores, tl, el, **kw):
    from mvector.metric import metrics
    if device is None:
        return metrics.verification_metrics(scores, tl, el, **kw)
    t = lambda a: torch.from_numpy(np.array(a)).to(device)
    return metrics.verification_metrics(t(scores), t(tl), t(el), **kw)


def check_edges_public(device):
    """the documented exceptions of metrics.verification_metrics, on numpy input (device None) or tensors of `device`"""
    s = np.array([[0.1, 0.9]], dtype=np.float32)
    with pytest.raises(ValueError, match='no impostor'):
        _public(device, s, np.array([3], dtype=np.int32), np.array([3, 3], dtype=np.int32))
    with pytest.raises(ValueError, match='no target'):
        _public(device, s, np.array([3], dtype=np.int32), np.array([4, 5], dtype=np.int32))
    with pytest.raises(IndexError):   # [0.1 (target), 0.9 (impostor)]: fnr >= fpr everywhere, the reference fails at flatnonzero(...)[-1]
        _public(device, s, np.array([3], dtype=np.int32), np.array([3, 4], dtype=np.int32))
    with pytest.raises(ValueError):   # N = 1: one class is empty
        _public(device, s[:, :1], np.array([3], dtype=np.int32), np.array([3], dtype=np.int32))
    # negative and large int32 labels: only equality matters
    scores, tl, el, costs = case('tiny')
    remap = np.array([-2147483648, 2147483647, -1], dtype=np.int32)
    assert _public(device, scores, remap[tl], remap[el], **costs) == _public(device, scores, tl, el, **costs)
    # non-default costs against the reference's own expressions on the reference-equal curve
    from mvector.metric import metrics
    eer, dcf, thr, fnr, fpr, _ = _public(device, scores, tl, el, p_target=0.2, c_miss=3, c_fa=0.5, return_curve=True)
    assert dcf == float(metrics.compute_dcf(fnr, fpr, p_target=0.2, c_miss=3, c_fa=0.5))


def check_edges_raw(cdll, device):
    """N = 1, one-class inputs reported rather than refused, and the refusals by message; nothing here launches out of bounds"""
    from mvector import _hip
    lib = cdll or _hip.lib()
    t = lambda a: torch.from_numpy(np.array(a)).to(device)
    one = np.array([[0.25]], dtype=np.float32)
    r = _hip.verification_metrics(t(one), t(np.array([5], dtype=np.int32)), t(np.array([5], dtype=np.int32)), curve=True, cdll=cdll)
    assert (r['n_target'], r['n_impostor']) == (1, 0) and r['tgt_cum'].tolist() == [1] and r['sorted_scores'].tolist() == [0.25]
    r = _hip.verification_metrics(t(one), t(np.array([5], dtype=np.int32)), t(np.array([-5], dtype=np.int32)), cdll=cdll)
    assert (r['n_target'], r['n_impostor']) == (0, 1)
    got, idx = _hip.sort_scores(t(one), cdll=cdll)
    assert got.tolist() == [0.25] and idx.tolist() == [0]

    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=device)
    p = buf.data_ptr()
    msg = lambda: lib.mv_last_error().decode()
    big = 1 << 31
    assert lib.mv_sort_scores_workspace_bytes(0) == 0 and lib.mv_sort_scores_workspace_bytes(big) == 0 and lib.mv_sort_scores_workspace_bytes(big - 1) > 0
    need = lib.mv_sort_scores_workspace_bytes(8)
    assert 0 < need < 32768
    assert lib.mv_sort_scores_f32(p, 0, p + 4096, p + 8192, p + 32768, need, None) == -1 and 'N outside 1 .. 2^31 - 1' in msg()
    assert lib.mv_sort_scores_f32(p, big, p + 4096, p + 8192, p + 32768, need, None) == -1 and 'N outside 1 .. 2^31 - 1' in msg()
    assert lib.mv_sort_scores_f32(None, 8, p + 4096, p + 8192, p + 32768, need, None) == -1 and 'null or aliased buffer' in msg()
    assert lib.mv_sort_scores_f32(p, 8, p + 4096, None, p + 32768, need, None) == -1 and 'null or aliased buffer' in msg()
    assert lib.mv_sort_scores_f32(p, 8, p + 4096, p + 8192, None, need, None) == -1 and 'null workspace' in msg()
    assert lib.mv_sort_scores_f32(p, 8, p + 4096, p + 8192, p + 32768, need - 1, None) == -4 and 'workspace smaller' in msg()

    cfg = _hip.MvVerifCfg(0.01, 1.0, 1.0)
    res = _hip.MvVerifResult()
    need = lib.mv_verif_metrics_workspace_bytes(2, 4)
    assert 0 < need < 32768
    assert lib.mv_verif_metrics_workspace_bytes(0, 4) == 0 and lib.mv_verif_metrics_workspace_bytes(1 << 16, 1 << 15) == 0
    assert lib.mv_verif_metrics_workspace_bytes((1 << 31) - 1, 1) > 0
    call = lambda nt, ne, ws=p + 32768, nbytes=need, c=cfg, s=p, tl=p + 1024, r=res: lib.mv_verif_metrics_f32(
        s, nt, ne, tl, p + 2048, ctypes.byref(c) if c is not None else None, ctypes.byref(r) if r is not None else None, None, None, ws, nbytes, None)
    assert call(0, 4) == -1 and 'N = 0' in msg()
    assert call(2, 0) == -1 and 'N = 0' in msg()
    assert call(1 << 16, 1 << 15) == -1 and 'outside 1 .. 2^31 - 1' in msg()
    assert call(2, 4, s=None) == -1 and 'null or aliased buffer' in msg()
    assert call(2, 4, tl=None) == -1 and 'null or aliased buffer' in msg()
    assert call(2, 4, r=None) == -1 and 'null or aliased buffer' in msg()
    assert call(2, 4, c=None) == -1 and 'null cfg' in msg()
    assert call(2, 4, ws=None) == -1 and 'null workspace' in msg()
    assert call(2, 4, nbytes=need - 1) == -4 and 'workspace smaller' in msg()
    for bad in (0.0, 1.0, -0.5, float('nan')):
        assert call(2, 4, c=_hip.MvVerifCfg(bad, 1.0, 1.0)) == -1 and 'p_target outside (0, 1)' in msg()
    assert call(2, 4, c=_hip.MvVerifCfg(0.01, -1.0, 1.0)) == -1 and 'negative cost' in msg()
    assert call(2, 4, c=_hip.MvVerifCfg(0.01, 1.0, -1e-9)) == -1 and 'negative cost' in msg()
    assert call(2, 4) == 0   # the same arguments, nothing bad: it runs (all-zero scores and labels)
    with pytest.raises(RuntimeError, match='N outside'):
        _hip.sort_scores(torch.zeros((0,), dtype=torch.float32, device=device), cdll=cdll)
    with pytest.raises(RuntimeError, match='p_target outside'):
        _hip.verification_metrics(t(one), t(np.array([5], dtype=np.int32)), t(np.array([5], dtype=np.int32)), p_target=1.5, cdll=cdll)


def check_transpose_invariance(cdll, device):
    """300 x 97 and 97 x 300 with swapped label vectors hold the same multiset of (score, label) pairs, and the golden has no cross-label tie"""
    from mvector import _hip
    from mvector.metric import metrics
    scores, tl, el, costs = case('main')
    t = lambda a: torch.from_numpy(np.array(a)).to(device)
    a = _hip.verification_metrics(t(scores), t(tl), t(el), cdll=cdll, **costs)
    b = _hip.verification_metrics(t(scores.T), t(el), t(tl), cdll=cdll, **costs)
    g = golden()
    for r in (a, b):
        eer = metrics._eer_from_counts(r['n_target'], r['n_impostor'], r['i1'], r['tgt_i1'], r['i2'], r['tgt_i2'])
        assert eer == g['main_eer'] and r['min_cost'] / 0.01 == g['main_min_dcf']
    assert a == b   # the positions and counts too: ties within one label do not move T
