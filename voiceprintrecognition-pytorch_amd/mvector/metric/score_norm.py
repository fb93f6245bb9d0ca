"""Cohort score normalisation of verification scores: Z-, T-, S-norm and adaptive S-norm (AS-norm, the top-N cohort scores).

For an embedding ``x`` and a cohort ``C`` [M, D] the cohort scores are the cosines of ``x`` with every cohort row; the statistics of ``x`` are
the mean and the population standard deviation (two passes, fp64, rounded once to fp32) of its ``N' = min(top_n, M)`` largest cohort scores --
largest by the order key of ``gallery.sort_keys`` (-0 and +0 one value, NaN above +inf), equal keys by the lower cohort row.  A raw score
``s`` of trial ``t`` against enrolment ``e`` becomes, in float32 and in exactly this order of operations,

    'z': (s - mean_e) / std_e        't': (s - mean_t) / std_t        's': 0.5 * ((s - mean_t) / std_t + (s - mean_e) / std_e)

``top_n < M`` is the adaptive form, ``top_n >= M`` plain S-norm.  ``std == 0`` is not guarded: the IEEE result comes out.

CUDA tensors run the two native calls (``_hip.cohort_stats``: the cohort scores of a chunk of rows written by the kernel behind
``_hip.cosine`` and reduced per row by a radix select in LDS while they are cache-resident; ``_hip.score_norm``: one element-wise launch).
Numpy arrays and CPU tensors run the same definition in numpy; the scores there follow the row-by-row rule of ``DeviceGallery.search``.
"""
import numpy as np
import torch

from mvector.infer_utils.gallery import top_k_of_scores

MODES = ('s', 'z', 't')
_TINY = np.float32(1.17549435e-38)


def _is_cuda(x):
    return isinstance(x, torch.Tensor) and x.is_cuda


def _host(x):
    """array or CPU tensor -> float32 numpy array [n, D] (a vector becomes one row)"""
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(x.reshape(-1, x.shape[-1]), dtype=np.float32)


def cosine_scores(a, b):
    """[N, D] x [M, D] -> [N, M] float32 cosine scores where ``a`` lives: ``_hip.cosine`` for a CUDA tensor (a tensor comes back), else numpy
    row by row -- dot / (max(|a|, tiny) max(|b|, tiny)), every dot product summed on its own so that a score depends on its own pair of rows
    alone (an array comes back)."""
    if _is_cuda(a):
        from mvector import _hip
        return _hip.cosine(a.reshape(-1, a.shape[-1]), torch.as_tensor(b).reshape(-1, a.shape[-1]))
    a, b = _host(a), _host(b)
    with np.errstate(invalid='ignore', over='ignore'):
        dots = np.stack([(b * row).sum(axis=1) for row in a]) if len(a) else np.zeros((0, len(b)), dtype=np.float32)
        return dots / (np.maximum(np.linalg.norm(a, axis=1), _TINY)[:, None] * np.maximum(np.linalg.norm(b, axis=1), _TINY)[None, :])


def top_n_stats(scores, top_n):
    """[n, M] float32 cohort scores -> (mean, std) float32 [n] of each row's min(top_n, M) largest entries, as the module docstring defines"""
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    n, m = scores.shape
    assert m >= 1 and top_n >= 1
    kept = top_k_of_scores(scores, min(int(top_n), m))[0].astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        mean = kept.sum(axis=1) / kept.shape[1]
        std = np.sqrt(((kept - mean[:, None]) ** 2).sum(axis=1) / kept.shape[1])
        return mean.astype(np.float32), std.astype(np.float32)


def normalize_scores(scores, trial_stats, enroll_stats, mode='s'):
    """the float32 expression of the module docstring on numpy arrays: scores [T, E], statistics (mean, std) per side (None for the side
    the mode does not use)"""
    s = np.asarray(scores, dtype=np.float32)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        if mode != 'z':
            tm, ts = (np.asarray(v, dtype=np.float32)[:, None] for v in trial_stats)
            t = (s - tm) / ts
        if mode != 't':
            em, es = (np.asarray(v, dtype=np.float32)[None, :] for v in enroll_stats)
            z = (s - em) / es
        return z if mode == 'z' else t if mode == 't' else np.float32(0.5) * (t + z)


def cohort_means(embeddings, labels):
    """per-speaker mean embeddings [S, D] float32 in order of first appearance: fp64 sums on the host, divided and rounded once (the rule of
    ``SpeakerGallery.user_means``)"""
    rows = _host(embeddings)
    labels = (labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)).tolist()
    assert len(labels) == len(rows)
    order, sums, counts = [], {}, {}
    for label, row in zip(labels, rows):
        if label not in sums:
            order.append(label)
            sums[label], counts[label] = np.zeros(row.shape, dtype=np.float64), 0
        sums[label] += row
        counts[label] += 1
    if not order:
        return np.zeros((0, rows.shape[1]), dtype=np.float32)
    return np.stack([(sums[l] / counts[l]).astype(np.float32) for l in order])


class ScoreNormalizer:
    """Holds a cohort [M, D] where it is handed in (a CUDA tensor stays on the device, arrays and CPU tensors on the host) and normalises score
    matrices with it."""

    def __init__(self, cohort, top_n=300, mode='s'):
        if int(top_n) < 2:
            raise ValueError(f'ScoreNormalizer: top_n {top_n} is below 2 (the standard deviation of one score is 0)')
        if mode not in MODES:
            raise ValueError(f"ScoreNormalizer: mode {mode!r} is not one of 's', 'z', 't'")
        if _is_cuda(cohort):
            self.cohort = cohort.detach().to(torch.float32).contiguous()
        else:
            self.cohort = _host(cohort)
        if self.cohort.ndim != 2 or self.cohort.shape[0] < 1:
            raise ValueError('ScoreNormalizer: the cohort is not a matrix of at least one row')
        self.top_n, self.mode = int(top_n), mode

    def _cohort_for(self, x):
        """the cohort beside ``x``: kept where it was handed in, moved (and the copy kept) when the other side is asked for"""
        if _is_cuda(x) != _is_cuda(self.cohort):
            other = getattr(self, '_other', None)
            if other is None or (_is_cuda(x) and other.device != x.device):
                other = torch.from_numpy(self.cohort).to(x.device) if _is_cuda(x) else self.cohort.cpu().numpy()
                self._other = other
            return other
        return self.cohort

    def stats(self, embeddings):
        """embeddings [n, D] -> (mean, std), float32 [n]: tensors on the device for a CUDA tensor, numpy arrays otherwise"""
        if _is_cuda(embeddings):
            from mvector import _hip
            return _hip.cohort_stats(embeddings.reshape(-1, embeddings.shape[-1]), self._cohort_for(embeddings), self.top_n)
        return top_n_stats(cosine_scores(embeddings, self._cohort_for(embeddings)), self.top_n)

    def normalize(self, scores, trial_embeddings=None, enroll_embeddings=None, trial_stats=None, enroll_stats=None, out=None):
        """scores [T, E] float32 -> the normalised matrix on the same device (a tensor for a tensor, an array for an array).  Per side either the
        embeddings or precomputed ``stats``; the side the mode does not use needs neither.  ``out=scores`` normalises a CUDA matrix in place."""
        def side(stats, embeddings, used, what):
            if not used:
                return None
            if stats is None:
                if embeddings is None:
                    raise ValueError(f'ScoreNormalizer.normalize: mode {self.mode!r} needs {what}_embeddings or {what}_stats')
                if _is_cuda(scores) and not _is_cuda(embeddings):
                    embeddings = torch.as_tensor(embeddings).to(scores.device)
                stats = self.stats(embeddings)
            return stats
        trial_stats = side(trial_stats, trial_embeddings, self.mode != 'z', 'trial')
        enroll_stats = side(enroll_stats, enroll_embeddings, self.mode != 't', 'enroll')
        if _is_cuda(scores):
            from mvector import _hip
            return _hip.score_norm(scores.to(torch.float32).contiguous(), trial_stats, enroll_stats, self.mode, out=out)
        to_np = lambda st: None if st is None else tuple(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v for v in st)
        host = scores.detach().numpy() if isinstance(scores, torch.Tensor) else scores
        result = normalize_scores(host, to_np(trial_stats), to_np(enroll_stats), self.mode)
        return torch.from_numpy(result) if isinstance(scores, torch.Tensor) else result
