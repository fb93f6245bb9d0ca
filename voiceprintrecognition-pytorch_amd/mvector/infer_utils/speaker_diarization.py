"""Speaker diarization around the embeddings: ``SpeakerDiarization`` and ``SpectralCluster`` with the reference's constructor
arguments and method names (mvector/infer_utils/speaker_diarization.py there), restated in this project's own words.

Two paths share this file.  With numpy embeddings everything runs on the host in numpy / scipy and reproduces the reference's
arithmetic (fp32 similarity, pruning, symmetrisation, Laplacian, ``scipy.linalg.eigh``, the eigen-gap rule, ``k_means``): this is
the ``use_gpu=False`` path and the arbiter of the device path.  With a torch tensor of embeddings the cosine matrix, the pruned
affinity / Laplacian and the lowest eigenpairs come from the HIP library (``_hip.cosine`` -> ``_hip.affinity_laplacian`` ->
``_hip.laplacian_eig_lowest``); the gap rule, ``k_means`` on the N x k spectral embedding and the merging stay on the host.
There is no fallback between the two: a failure of the device path raises.

Ties in the pruning: the reference's ``np.argsort`` (introsort) leaves the order of equal values open.  Here, on both paths, the
entry with the LOWER column index is dropped first.

VAD is yeaudio's model in the reference (``audio_segment.vad(return_seconds=True)``); it is not part of this package.  Pass the
speech regions as ``vad_segments=[{'start': s, 'end': s}, ...]`` (seconds, the shape yeaudio returns) or hand in a segment object
that has a ``vad`` method.
"""
import numpy as np

MAX_DEVICE_EIGENPAIRS = 16   # mv_laplacian_eig_lowest iterates for at most 16 eigenpairs


class SpeakerDiarization(object):

    def __init__(self, seg_duration=1.5, seg_shift=0.75, sample_rate=16000, merge_threshold=0.78):
        """说话人日志工具

        :param seg_duration: 每个分割片段的持续时间（秒）
        :param seg_shift: 分割片段之间的时间间隔（秒）
        :param sample_rate: 音频采样率
        :param merge_threshold: 两个说话人中心的余弦相似度大于此阈值时合并
        """
        self.seg_duration = seg_duration
        self.seg_shift = seg_shift
        self.sample_rate = sample_rate
        self.merge_threshold = merge_threshold
        self.spectral_cluster = SpectralCluster()

    # ------------------------------------------------------------------ segmentation
    def _vad_list(self, audio_segment, vad_segments=None):
        """[[start s, end s, samples]] of the speech regions, times rounded to milliseconds as the reference rounds them"""
        self.sample_rate = audio_segment.sample_rate
        if vad_segments is None:
            if not hasattr(audio_segment, 'vad'):
                raise NotImplementedError(
                    'speaker diarization needs the speech regions: this package ships no VAD (the reference uses yeaudio\'s '
                    'AudioSegment.vad). Pass vad_segments=[{"start": seconds, "end": seconds}, ...] or an audio segment object with a '
                    'vad() method (yeaudio)')
            vad_segments = audio_segment.vad(return_seconds=True)
        samples = audio_segment.samples
        out = []
        for t in vad_segments:
            st, ed = round(t['start'], 3), round(t['end'], 3)
            out.append([st, ed, samples[int(st * self.sample_rate):int(ed * self.sample_rate)]])
        self._check_audio_list(out)
        return out

    def segments_audio(self, audio_segment, vad_segments=None) -> list:
        """Speech regions cut into fixed-length chunks: [[start s, end s, samples of one chunk]]."""
        return self._chunk(self._vad_list(audio_segment, vad_segments))

    def chunk_table(self, audio_segment, vad_segments=None):
        """The same chunks without their samples, for the device path: ([[start s, end s, None]], first sample of every chunk in the whole
        recording (int64), number of samples it holds before the zero padding (int64), chunk length in samples)."""
        vad = self._vad_list(audio_segment, vad_segments)
        times, starts, lens = [], [], []
        for seg_st, _, data in vad:
            base = int(seg_st * self.sample_rate)
            for lo, hi in self._chunk_spans(data.shape[0]):
                times.append([lo / self.sample_rate + seg_st, hi / self.sample_rate + seg_st, None])
                starts.append(base + lo)
                lens.append(hi - lo)
        return times, np.asarray(starts, dtype=np.int64), np.asarray(lens, dtype=np.int64), int(self.seg_duration * self.sample_rate)

    def _check_audio_list(self, audio: list):
        total = 0
        for i, (st, ed, data) in enumerate(audio):
            assert ed >= st, '分割的时间戳错误'
            assert isinstance(data, np.ndarray), '数据的类型不正确'
            assert int(ed * self.sample_rate) - int(st * self.sample_rate) == data.shape[0], '时间长度和数据长度不匹配'
            if i > 0:
                assert st >= audio[i - 1][1], 'wrong time stamps: speech regions overlap or are out of order'
            total += ed - st
        assert total > 5, f'音频时间过段，应当大于5秒，当前长度是{total}秒'

    def _chunk_spans(self, n):
        """(first, one past last) sample of every chunk of a region of n samples: a chunk per shift, the last one moved back so that it ends
        with the region; a region shorter than a chunk is one (short) chunk"""
        chunk_len = int(self.seg_duration * self.sample_rate)
        chunk_shift = int(self.seg_shift * self.sample_rate)
        spans, last_end = [], 0
        for lo in range(0, n, chunk_shift):
            hi = min(lo + chunk_len, n)
            if hi <= last_end:
                break
            last_end = hi
            spans.append((max(0, hi - chunk_len), hi))
        return spans

    def _chunk(self, vad_segments: list) -> list:
        chunk_len = int(self.seg_duration * self.sample_rate)
        out = []
        for seg_st, _, data in vad_segments:
            for lo, hi in self._chunk_spans(data.shape[0]):
                piece = data[lo:hi]
                if piece.shape[0] < chunk_len:
                    piece = np.pad(piece, (0, chunk_len - piece.shape[0]), 'constant')
                out.append([lo / self.sample_rate + seg_st, hi / self.sample_rate + seg_st, piece])
        return out

    # ------------------------------------------------------------------ clustering
    def clustering(self, embeddings, speaker_num=None):
        """Embeddings [n, dim] (numpy: host path; torch tensor: device path) -> (labels [n], centre embedding per speaker found BEFORE
        similar speakers are merged, as the reference returns them)."""
        labels = self.spectral_cluster(embeddings, oracle_num=speaker_num)
        labels = self._correct_labels(labels)
        if not isinstance(embeddings, np.ndarray):
            embeddings = embeddings.detach().cpu().numpy()
        centres = [embeddings[labels == i].mean(0) for i in range(labels.max() + 1)]
        assert len(centres) > 0
        centre_embeddings = np.stack(centres, axis=0)
        labels = self._merge_by_cos(labels, centres, self.merge_threshold)
        return labels, centre_embeddings

    @staticmethod
    def _merge_by_cos(labels, spk_center_emb, cos_thr):
        """While the two most similar centres reach cos_thr, the later speaker takes the earlier one's label and the labels above close the gap.
        The centres are not recomputed (nor re-indexed) after a merge: the reference's behaviour, kept."""
        assert 0 < cos_thr <= 1
        while True:
            spk_num = labels.max() + 1
            if spk_num == 1:
                break
            centres = np.stack([spk_center_emb[i] for i in range(spk_num)], axis=0)
            unit = centres / np.linalg.norm(centres, axis=1, keepdims=True)
            affinity = np.triu(np.matmul(unit, unit.T), 1)
            a, b = np.unravel_index(np.argmax(affinity), affinity.shape)
            if affinity[a, b] < cos_thr:
                break
            for i in range(len(labels)):
                if labels[i] == b:
                    labels[i] = a
                elif labels[i] > b:
                    labels[i] -= 1
        return labels

    # ------------------------------------------------------------------ post-processing
    def postprocess(self, segments: list, labels: np.ndarray) -> list:
        """Chunks + labels -> [{'speaker', 'start', 'end'}]: consecutive chunks of one speaker joined, overlaps split in the middle, turns
        shorter than a second given to a neighbour."""
        assert len(segments) == len(labels)
        turns = self._merge_seque([[seg[0], seg[1], lab] for seg, lab in zip(segments, labels)])
        for i in range(1, len(turns)):
            if turns[i - 1][1] > turns[i][0] + 1e-4:
                mid = (turns[i][0] + turns[i - 1][1]) / 2
                turns[i][0] = mid
                turns[i - 1][1] = mid
        turns = self._smooth(turns)
        return [dict(speaker=t[2], start=round(t[0], 3), end=round(t[1], 3)) for t in turns]

    @staticmethod
    def _correct_labels(labels):
        """labels renumbered in order of first appearance"""
        seen = {}
        out = []
        for lab in labels:
            if lab not in seen:
                seen[lab] = len(seen)
            out.append(seen[lab])
        return np.array(out)

    @staticmethod
    def _merge_seque(distribute_res):
        res = [distribute_res[0]]
        for item in distribute_res[1:]:
            if item[2] != res[-1][2] or item[0] > res[-1][1]:
                res.append(item)
            else:
                res[-1][1] = item[1]
        return res

    def _smooth(self, res, min_duration=1):
        last = len(res) - 1
        for i in range(len(res)):
            res[i][0] = round(res[i][0], 2)
            res[i][1] = round(res[i][1], 2)
            if res[i][1] - res[i][0] < min_duration:
                if i == 0:
                    res[i][2] = res[i + 1][2]
                elif i == last:
                    res[i][2] = res[i - 1][2]
                elif res[i][0] - res[i - 1][1] <= res[i + 1][0] - res[i][1]:
                    res[i][2] = res[i - 1][2]
                else:
                    res[i][2] = res[i + 1][2]
        return self._merge_seque(res)


class SpectralCluster:
    def __init__(self, min_num_spks=1, max_num_spks=15, pval=0.022, cdll=None):
        """Spectral clustering on the unnormalised Laplacian of the pruned cosine affinity.

        :param min_num_spks: 聚类的最小数量
        :param max_num_spks: 聚类的最大数量
        :param pval: 每行保留的相似度比例
        :param cdll: the bound native library of the device path (default: the product library; the test-suite passes its emulator build)
        """
        self.min_num_spks = min_num_spks
        self.max_num_spks = max_num_spks
        self.pval = pval
        self._cdll = cdll
        self.last_info = None   # device path: the eigen solver's info block of the last call

    def __call__(self, X, oracle_num=None):
        """X [n, dim] -> labels [n]; numpy runs the host path, a torch tensor the device path."""
        if not isinstance(X, np.ndarray):
            return self._call_device(X, oracle_num)
        sim_mat = self.get_sim_mat(X)
        pruned = self.p_pruning(sim_mat)
        sym = 0.5 * (pruned + pruned.T)
        laplacian = self.get_laplacian(sym)
        emb, num_of_spk = self.get_spec_embs(laplacian, oracle_num)
        return self.cluster_embs(emb, num_of_spk)

    def _call_device(self, X, oracle_num=None):
        from mvector import _hip
        n = X.shape[0]
        wanted = max(self.max_num_spks + 1, 0 if oracle_num is None else int(oracle_num))
        if wanted > MAX_DEVICE_EIGENPAIRS:
            raise ValueError(f'the device path computes at most {MAX_DEVICE_EIGENPAIRS} eigenpairs: speaker_num / max_num_spks + 1 = {wanted} '
                             f'is refused (the reference\'s own max_num_spks is 15)')
        n_prune = self.n_prune(n)
        if n_prune < 0:   # n < 6: the reference's expression goes negative and its slice [0:n_prune] then counts from the end
            n_prune = max(0, n + n_prune)
        sim = _hip.cosine(X, X, cdll=self._cdll)
        M, degree = _hip.affinity_laplacian(sim, n_prune, cdll=self._cdll)
        lambdas, vecs, self.last_info = _hip.laplacian_eig_lowest(M, degree, m=min(wanted, n), cdll=self._cdll)
        num_of_spk = self.num_speakers(lambdas, oracle_num)
        return self.cluster_embs(vecs[:, :num_of_spk].cpu().numpy(), num_of_spk)

    @staticmethod
    def get_sim_mat(X):
        """cosine similarities in X's own precision (fp32 embeddings give an fp32 matrix): rows scaled to unit length, then one product"""
        X = np.asarray(X)
        norms = np.sqrt(np.einsum('ij,ij->i', X, X))
        norms[norms == 0.0] = 1.0
        unit = X / norms[:, np.newaxis]
        return np.dot(unit, unit.T)

    def n_prune(self, n):
        """entries dropped per row: the reference's expression (negative below six rows, where it is used as a slice bound all the same)"""
        pval = 6. / n if n * self.pval < 6 else self.pval
        return int((1 - pval) * n)

    def p_pruning(self, A):
        """the n_prune smallest entries of every row become zero (in place); of equal values the lower column goes first"""
        n_elems = self.n_prune(A.shape[0])
        for i in range(A.shape[0]):
            A[i, np.argsort(A[i, :], kind='stable')[:n_elems]] = 0
        return A

    @staticmethod
    def get_laplacian(M):
        M[np.diag_indices(M.shape[0])] = 0
        D = np.diag(np.sum(np.abs(M), axis=1))
        return D - M

    def num_speakers(self, lambdas, k_oracle=None):
        if k_oracle is not None:
            return k_oracle
        gaps = self.get_eigen_gaps(lambdas[self.min_num_spks - 1:self.max_num_spks + 1])
        return int(np.argmax(gaps)) + self.min_num_spks

    def get_spec_embs(self, L, k_oracle=None):
        import scipy.linalg
        lambdas, eig_vecs = scipy.linalg.eigh(L)
        num_of_spk = self.num_speakers(lambdas, k_oracle)
        return eig_vecs[:, :num_of_spk], num_of_spk

    @staticmethod
    def cluster_embs(emb, k):
        try:
            from sklearn.cluster import k_means
        except ImportError as e:
            raise ImportError('speaker diarization clusters the spectral embedding with sklearn.cluster.k_means: '
                              'scikit-learn (sklearn) is not installed') from e
        _, labels, _ = k_means(emb, k, n_init="auto")
        return labels

    @staticmethod
    def get_eigen_gaps(eig_vals):
        return [float(eig_vals[i + 1]) - float(eig_vals[i]) for i in range(len(eig_vals) - 1)]
