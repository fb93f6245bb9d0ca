"""Verification metrics with the reference's signatures (mvector/metric/metrics.py:5-49).

``compute_fnr_fpr`` / ``compute_eer`` / ``compute_dcf`` are host-side numpy: one sort of the trial scores and two cumulative sums, the end of
``MVectorTrainer.evaluate(use_gpu=False)`` (trainer.py:463-468).  ``verification_metrics`` is the whole of it in one call from the score
matrix and the two label vectors; on CUDA tensors it runs in the native library (csrc/verif.hip) and is the end of ``evaluate(use_gpu=True)``.
"""
import numpy as np
import torch


def compute_fnr_fpr(scores, labels, weights=None):
    """Miss / false-alarm rates at every threshold = sorted score (ascending).

    fnr[i]: weighted fraction of target trials with score <= thresholds[i];
    fpr[i]: weighted fraction of impostor trials with score > thresholds[i].
    """
    scores = np.asarray(scores)
    labels = np.asarray(labels)
    order = np.argsort(scores)
    thresholds = scores[order]
    labels = labels[order]
    w = np.ones(labels.shape, dtype='f8') if weights is None else np.asarray(weights)[order]
    tgt = w * (labels == 1)
    imp = w * (labels == 0)
    fnr = np.cumsum(tgt) / np.sum(tgt)
    fpr = 1 - np.cumsum(imp) / np.sum(imp)
    return fnr, fpr, thresholds


def compute_eer(fnr, fpr, scores=None):
    """Equal error rate by linear interpolation between the two operating points around fnr == fpr; with ``scores``
    also the score at the first point where fnr >= fpr (the decision threshold the reference reports)."""
    gap = fnr - fpr
    i1 = np.flatnonzero(gap >= 0)[0]
    i2 = np.flatnonzero(gap < 0)[-1]
    a = (fnr[i1] - fpr[i1]) / (fpr[i2] - fpr[i1] - (fnr[i2] - fnr[i1]))
    eer = fnr[i1] + a * (fnr[i2] - fnr[i1])
    if scores is not None:
        return eer, np.sort(scores)[i1]
    return eer


def compute_dcf(fnr, fpr, p_target=0.01, c_miss=1, c_fa=1):
    """Minimum normalised detection cost."""
    c_det = np.min(c_miss * fnr * p_target + c_fa * fpr * (1 - p_target))
    c_def = min(c_miss * p_target, c_fa * (1 - p_target))
    return c_det / c_def


def _eer_from_counts(n_target, n_impostor, i1, tgt_i1, i2, tgt_i2):
    """compute_eer's interpolation from the cumulative target counts at its two operating points, with the reference's own fp64 expressions"""
    nt, ni = np.float64(n_target), np.float64(n_impostor)
    fnr1, fnr2 = np.float64(tgt_i1) / nt, np.float64(tgt_i2) / nt
    fpr1, fpr2 = 1 - np.float64(i1 + 1 - tgt_i1) / ni, 1 - np.float64(i2 + 1 - tgt_i2) / ni
    a = (fnr1 - fpr1) / (fpr2 - fpr1 - (fnr2 - fnr1))
    return fnr1 + a * (fnr2 - fnr1)


def _check_classes(n_target, n_impostor):
    if n_target == 0:
        raise ValueError('verification_metrics: no target trials (no trial label equals an enrolment label)')
    if n_impostor == 0:
        raise ValueError('verification_metrics: no impostor trials (every trial label equals every enrolment label)')


def verification_metrics(scores, trial_labels, enroll_labels, p_target=0.01, c_miss=1, c_fa=1, return_curve=False):
    """EER, minDCF and threshold of a whole evaluation from its score matrix ``scores`` [n_trials, n_enroll] and the two label vectors
    (trial (i, j) is a target when ``trial_labels[i] == enroll_labels[j]``) -> ``(eer, min_dcf, threshold)`` as floats, plus
    ``(fnr, fpr, thresholds)`` (fp64, fp64, fp32 numpy arrays over the sorted scores) with ``return_curve``.

    The numbers are those of ``compute_fnr_fpr`` / ``compute_eer`` / ``compute_dcf`` on the flattened, trial-major scores and labels, with ONE
    difference: equal scores are ordered by their flat index (``argsort(kind='stable')``).  numpy's default argsort leaves that order open, so
    when a target score equals an impostor score the three functions above may give another, equally valid, result; without such a tie the
    floats are identical.

    CUDA tensors run on the device (``_hip.verification_metrics``: a radix sort and one scan, nothing N-sized crosses to the host unless the
    curve is asked for); numpy arrays and CPU tensors run the same arithmetic in numpy.  Raises ``ValueError`` when there is no target or no
    impostor trial and ``IndexError`` when no threshold has fnr < fpr, where the reference's functions divide by zero or fail."""
    if isinstance(scores, torch.Tensor) and scores.is_cuda:
        from mvector import _hip
        as_t = lambda x: x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))
        r = _hip.verification_metrics(scores.to(torch.float32), as_t(trial_labels), as_t(enroll_labels), p_target, c_miss, c_fa, curve=return_curve)
        _check_classes(r['n_target'], r['n_impostor'])
        if r['i2'] < 0 or r['i1'] < 0:
            raise IndexError('verification_metrics: no threshold with fnr < fpr' if r['i2'] < 0 else 'verification_metrics: no threshold with fnr >= fpr')
        eer = _eer_from_counts(r['n_target'], r['n_impostor'], r['i1'], r['tgt_i1'], r['i2'], r['tgt_i2'])
        min_dcf = np.float64(r['min_cost']) / min(c_miss * p_target, c_fa * (1 - p_target))
        out = float(eer), float(min_dcf), float(r['score_i1'])
        if not return_curve:
            return out
        thresholds = r['sorted_scores'].cpu().numpy()
        tgt = r['tgt_cum'].cpu().numpy().astype('f8')
        imp = np.arange(1, tgt.shape[0] + 1, dtype='f8') - tgt
        return out + (tgt / np.float64(r['n_target']), 1 - imp / np.float64(r['n_impostor']), thresholds)

    to_np = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    scores = to_np(scores).astype(np.float32, copy=False)
    trial_labels, enroll_labels = to_np(trial_labels), to_np(enroll_labels)
    assert scores.ndim == 2 and trial_labels.shape == (scores.shape[0],) and enroll_labels.shape == (scores.shape[1],)
    if scores.size == 0:
        raise ValueError('verification_metrics: no trials')
    flat = scores.reshape(-1)
    order = np.argsort(flat, kind='stable')
    thresholds = flat[order]
    labels = (trial_labels[:, None] == enroll_labels[None, :]).reshape(-1)[order]
    tgt = labels.astype('f8')
    imp = (~labels).astype('f8')
    _check_classes(int(labels.sum()), int(labels.size - labels.sum()))
    fnr = np.cumsum(tgt) / np.sum(tgt)
    fpr = 1 - np.cumsum(imp) / np.sum(imp)
    gap = fnr - fpr
    i1 = np.flatnonzero(gap >= 0)[0]
    i2 = np.flatnonzero(gap < 0)[-1]          # IndexError when there is none, as in the reference
    a = (fnr[i1] - fpr[i1]) / (fpr[i2] - fpr[i1] - (fnr[i2] - fnr[i1]))
    eer = fnr[i1] + a * (fnr[i2] - fnr[i1])
    min_dcf = np.min(c_miss * fnr * p_target + c_fa * fpr * (1 - p_target)) / min(c_miss * p_target, c_fa * (1 - p_target))
    out = float(eer), float(min_dcf), float(thresholds[i1])
    return out + (fnr, fpr, thresholds) if return_curve else out


def accuracy(output, label):
    """Top-1 accuracy of classifier logits (training-time metric; kept for API completeness)."""
    pred = torch.argmax(torch.nn.functional.softmax(output, dim=-1), dim=1).cpu().numpy()
    return np.mean((pred == label.data.cpu().numpy()).astype(int))
