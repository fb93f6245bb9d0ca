"""Energy voice activity detection: ``EnergyVad`` turns a waveform into the speech regions ``speaker_diarization`` asks for
(``vad_segments=[{'start': s, 'end': s}, ...]``, the shape yeaudio's VAD returns).

The frame decisions are Kaldi's ``compute-vad`` restated (the tool every x-vector recipe runs): frames of ``frame_length`` samples every
``frame_shift``, snip-edges; per frame the log of the centred energy of the samples scaled to the int16 range (no dither, no pre-emphasis,
no window; floored at 2^-23); a threshold ``energy_threshold + energy_mean_scale * mean(logE)`` per recording; a frame is speech when at
least ``proportion_threshold`` of the frames within ``frames_context`` of it lie above the threshold.  The defaults are compute-vad's own
(5.0 / 0.5 / context 0 / 0.6); the VoxCeleb recipe runs 5.5 / 0.5 / context 2 / 0.12.

Two paths share this file.  A CUDA tensor runs the HIP library (``_hip.vad_energy``: mv_vad_energy_f32): energies, threshold, decisions and
the compaction of the decisions into runs of speech frames stay on the device, the run list is the one thing that comes down -- that
download is the call's only synchronisation.  A numpy array or a CPU tensor runs the same definition in numpy: the ``use_gpu=False`` path
and the arbiter of the device path.  There is no fallback between the two.  Both then smooth the runs on the host, in integer samples:

1. the run of frames [a, b) covers the samples [a * shift, b * shift); a run that reaches the last frame ends with the recording;
2. regions closer than ``min_silence`` are joined;
3. regions shorter than ``min_speech`` are dropped;
4. every region grows by ``speech_pad`` on both sides, but not beyond the recording and not beyond the middle of the gap to its neighbour.

``regions`` and ``trim`` go on without the host in between: on CUDA tensors the same four steps run on the device (``_hip.vad_regions``:
mv_vad_regions_i32) and the kept regions of every row are moved together there (``_hip.wave_gather``: mv_wave_gather_f32) -- nothing comes
down; on arrays and CPU tensors they are ``smooth`` and a concatenation.  ``MVectorPredictor.predict`` / ``predict_batch`` use ``trim`` for
their ``vad=`` argument.

Out of scope: int16 input (convert, or let ``MVectorPredictor.vad`` load the audio), selecting voiced frames at the feature level, a neural
VAD, and any change to what ``speaker_diarization`` does without ``vad_segments``.
"""
import numpy as np

EPS = 2.0 ** -23
_BLOCK = 4096   # frames per numpy block of the host path: the [block, frame_length] fp64 matrices stay in the cache


class EnergyVad(object):

    def __init__(self, sample_rate=16000, frame_length_ms=25, frame_shift_ms=10, frames_context=0, energy_threshold=5.0, energy_mean_scale=0.5,
                 proportion_threshold=0.6, scale=32768.0, min_silence=0.3, min_speech=0.25, speech_pad=0.03, cdll=None):
        """:param sample_rate: samples per second of the waveforms this object is called with
        :param frame_length_ms, frame_shift_ms: the frames, in milliseconds (25 / 10: 400 / 160 samples at 16 kHz)
        :param frames_context, energy_threshold, energy_mean_scale, proportion_threshold: compute-vad's options of the same names
        :param scale: what a sample is multiplied with before the energy (32768: [-1, 1) samples in the int16 range the thresholds assume)
        :param min_silence, min_speech, speech_pad: the smoothing, in seconds
        :param cdll: the bound native library of the device path (default: the product library; the test-suite passes its emulator build)
        """
        self.sample_rate = int(sample_rate)
        self.cfg = dict(frame_length=int(round(self.sample_rate * frame_length_ms / 1000.0)),
                        frame_shift=int(round(self.sample_rate * frame_shift_ms / 1000.0)), frames_context=int(frames_context),
                        energy_threshold=float(energy_threshold), energy_mean_scale=float(energy_mean_scale),
                        proportion_threshold=float(proportion_threshold), scale=float(scale))
        if not 1 <= self.cfg['frame_shift'] <= self.cfg['frame_length'] <= 4096:
            raise ValueError(f'EnergyVad: frames of {self.cfg["frame_length"]} samples every {self.cfg["frame_shift"]} are outside '
                             f'1 <= frame_shift <= frame_length <= 4096')
        if not 0 <= self.cfg['frames_context'] <= 64:
            raise ValueError('EnergyVad: frames_context outside 0 .. 64')
        if not all(np.isfinite(self.cfg[k]) for k in ('energy_threshold', 'energy_mean_scale', 'proportion_threshold', 'scale')):
            raise ValueError('EnergyVad: non-finite energy_threshold, energy_mean_scale, proportion_threshold or scale')
        self.min_silence = int(round(min_silence * self.sample_rate))
        self.min_speech = int(round(min_speech * self.sample_rate))
        self.speech_pad = int(round(speech_pad * self.sample_rate))
        self._cdll = cdll

    # ------------------------------------------------------------------ frames
    def num_frames(self, n):
        length, shift = self.cfg['frame_length'], self.cfg['frame_shift']
        return 0 if n < length else 1 + (n - length) // shift

    @staticmethod
    def _is_device(wav):
        return not isinstance(wav, np.ndarray) and getattr(wav, 'is_cuda', False)

    def _host_rows(self, wav, lengths):
        x = wav if isinstance(wav, np.ndarray) else wav.detach().numpy()
        x = np.asarray(x, dtype=np.float32)
        assert x.ndim in (1, 2), 'EnergyVad: a waveform [L] or a batch [B, L]'
        rows = x[None, :] if x.ndim == 1 else x
        if lengths is None:
            n = [rows.shape[1]] * rows.shape[0]
        else:
            n = [min(max(int(v), 0), rows.shape[1]) for v in np.asarray(lengths).reshape(-1)]
            assert len(n) == rows.shape[0], f'EnergyVad: lengths must have {rows.shape[0]} entries'
        return rows, n

    def _host_frames(self, x):
        """one row of n samples -> (decisions uint8 [T], logE fp64 [T], thr fp64) by the definition, in numpy"""
        c = self.cfg
        length, shift, ctx = c['frame_length'], c['frame_shift'], c['frames_context']
        T = self.num_frames(x.shape[0])
        log_e = np.empty(T, dtype=np.float64)
        with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
            for t0 in range(0, T, _BLOCK):
                t1 = min(T, t0 + _BLOCK)
                v = x[t0 * shift:(t1 - 1) * shift + length].astype(np.float64) * c['scale']
                frames = np.lib.stride_tricks.as_strided(v, shape=(t1 - t0, length), strides=(shift * v.strides[0], v.strides[0]), writeable=False)
                d = frames - (frames.sum(axis=1) / length)[:, None]
                e = np.einsum('ij,ij->i', d, d)
                log_e[t0:t1] = np.log(np.where(e < EPS, EPS, e))
            thr = c['energy_threshold'] + c['energy_mean_scale'] * (log_e.sum() / T if T else np.float64('nan'))
            above = np.concatenate([[0], np.cumsum(log_e > thr)])
        t = np.arange(T)
        lo, hi = np.maximum(t - ctx, 0), np.minimum(t + ctx, T - 1)
        dec = (above[hi + 1] - above[lo]).astype(np.float64) >= (hi - lo + 1).astype(np.float64) * c['proportion_threshold']
        return dec.astype(np.uint8), log_e, np.float64(thr)

    def frames(self, wav, lengths=None):
        """-> (decisions uint8, log_energy fp64, threshold fp64) per frame: [T] / [T] / scalar for a 1-D waveform, [B, T(L)] / [B, T(L)] /
        [B] for a batch (zeros behind a row's own frames).  CUDA tensors give device tensors, the host path numpy arrays."""
        if self._is_device(wav):
            from mvector import _hip
            out = _hip.vad_energy(wav, lengths=None if lengths is None else _as_tensor(lengths), cdll=self._cdll, **self.cfg)
            got = out['decisions'], out['log_energy'], out['threshold']
            return tuple(g[0] for g in got) if wav.dim() == 1 else got
        rows, n = self._host_rows(wav, lengths)
        T = self.num_frames(rows.shape[1])
        dec, log_e = np.zeros((len(n), T), dtype=np.uint8), np.zeros((len(n), T), dtype=np.float64)
        thr = np.empty(len(n), dtype=np.float64)
        for b, nb in enumerate(n):
            d, l, thr[b] = self._host_frames(rows[b, :nb])
            dec[b, :d.shape[0]], log_e[b, :l.shape[0]] = d, l
        return (dec[0], log_e[0], thr[0]) if np.ndim(wav) == 1 else (dec, log_e, thr)

    @staticmethod
    def runs_of(decisions):
        """uint8 [T] -> int64 [R, 2]: the maximal stretches [a, b) of ones"""
        edge = np.flatnonzero(np.diff(np.concatenate([[0], np.asarray(decisions, dtype=np.int8), [0]])))
        return edge.reshape(-1, 2).astype(np.int64)

    # ------------------------------------------------------------------ segments
    def smooth(self, runs, num_frames, n):
        """runs [R, 2] of speech frames of a recording of n samples and num_frames frames -> int64 [S, 2]: the regions in samples"""
        runs = np.asarray(runs, dtype=np.int64).reshape(-1, 2)
        if runs.shape[0] == 0:
            return runs
        shift = self.cfg['frame_shift']
        start = runs[:, 0] * shift
        end = np.where(runs[:, 1] >= num_frames, n, runs[:, 1] * shift)
        keep = start[1:] - end[:-1] >= self.min_silence              # the gaps that stay
        start, end = start[np.concatenate([[True], keep])], end[np.concatenate([keep, [True]])]
        long_enough = end - start >= self.min_speech
        start, end = start[long_enough], end[long_enough]
        if start.shape[0] == 0:
            return np.zeros((0, 2), dtype=np.int64)
        gap = start[1:] - end[:-1]
        new_end = np.minimum(end + self.speech_pad, np.concatenate([end[:-1] + gap // 2, [n]]))
        new_start = np.maximum(start - self.speech_pad, np.concatenate([[0], end[:-1] + gap // 2]))
        return np.stack([new_start, new_end], axis=1)

    # ------------------------------------------------------------------ regions and trimming, without the host in between
    def _device_regions(self, wav, lengths):
        """CUDA rows [B, L] -> (num_regions, regions, kept, lengths tensor or None) on the device; nothing comes down"""
        from mvector import _hip
        lengths = None if lengths is None else _as_tensor(lengths)
        out = _hip.vad_energy(wav, lengths=lengths, cdll=self._cdll, **self.cfg)   # max_runs = (T(L) + 1) // 2: no row can be truncated
        got = _hip.vad_regions(out, lengths, self.cfg['frame_shift'], self.min_silence, self.min_speech, self.speech_pad, L=wav.shape[-1], cdll=self._cdll)
        return got + (lengths,)

    def regions(self, wav, lengths=None):
        """-> (num_regions int32 [B], regions int32 [B, (T(L) + 1) // 2, 2], kept int64 [B]): per row its speech regions [start, end) in samples
        (``smooth`` of its runs; the first num_regions pairs count) and the sum of their lengths; without the leading B for a 1-D waveform.
        CUDA tensors give device tensors and download nothing (mv_vad_energy_f32, mv_vad_regions_i32); the host path gives numpy arrays, zeros
        behind a row's regions."""
        if self._is_device(wav):
            got = self._device_regions(wav if wav.dim() == 2 else wav.unsqueeze(0), lengths)[:3]
            return tuple(g[0] for g in got) if wav.dim() == 1 else got
        rows, n = self._host_rows(wav, lengths)
        max_runs = (self.num_frames(rows.shape[1]) + 1) // 2
        num, reg, kept = np.zeros(len(n), dtype=np.int32), np.zeros((len(n), max_runs, 2), dtype=np.int32), np.zeros(len(n), dtype=np.int64)
        for b, nb in enumerate(n):
            dec = self._host_frames(rows[b, :nb])[0]
            r = self.smooth(self.runs_of(dec), dec.shape[0], nb)
            num[b], reg[b, :r.shape[0]], kept[b] = r.shape[0], r, (r[:, 1] - r[:, 0]).sum()
        return (num[0], reg[0], kept[0]) if np.ndim(wav) == 1 else (num, reg, kept)

    def trim(self, wav, lengths=None):
        """-> (trimmed fp32 [B, L], kept int64 [B]): every row's speech regions one behind the other, zeros behind its kept samples; [L] and a
        scalar for a 1-D waveform.  CUDA tensors run VAD -> regions -> gather on the current stream (mv_wave_gather_f32 last) and synchronise
        nowhere: both results are device tensors.  Arrays and CPU tensors run the same definition in numpy.  There is no fallback between the two."""
        if self._is_device(wav):
            from mvector import _hip
            rows = wav if wav.dim() == 2 else wav.unsqueeze(0)
            num_regions, regions, kept, lengths = self._device_regions(rows, lengths)
            out, _ = _hip.wave_gather(rows, lengths, num_regions, regions, cdll=self._cdll)
            return (out[0], kept[0]) if wav.dim() == 1 else (out, kept)
        rows, n = self._host_rows(wav, lengths)
        num, reg, kept = self.regions(rows, n)
        out = np.zeros(rows.shape, dtype=np.float32)
        for b in range(rows.shape[0]):
            if num[b]:
                out[b, :kept[b]] = np.concatenate([rows[b, s:e] for s, e in reg[b, :num[b]]])
        return (out[0], kept[0]) if np.ndim(wav) == 1 else (out, kept)

    def to_seconds(self, regions, n):
        """int64 [S, 2] samples -> [{'start': s, 'end': s}].  An end is lowered to the recording's last whole millisecond where its own
        millisecond rounding (speaker_diarization rounds so) would point behind the last sample."""
        sr = float(self.sample_rate)
        start, end = regions[:, 0] / sr, regions[:, 1] / sr
        beyond = np.floor(np.round(end, 3) * sr) > n
        end = np.where(beyond, np.floor(n / sr * 1000.0) / 1000.0, end)
        return [dict(start=float(s), end=float(e)) for s, e in zip(start, end)]

    def __call__(self, wav, lengths=None):
        """waveform [L] -> [{'start': seconds, 'end': seconds}], disjoint and in order; a batch [B, L] (``lengths``: the rows' own sample
        counts, host values) -> one such list per row"""
        if self._is_device(wav):
            from mvector import _hip
            B = 1 if wav.dim() == 1 else wav.shape[0]
            L = wav.shape[-1]
            n = [L] * B if lengths is None else [min(max(int(v), 0), L) for v in np.asarray(_as_host(lengths)).reshape(-1)]
            out = _hip.vad_energy(wav, lengths=None if lengths is None else _as_tensor(n), cdll=self._cdll, **self.cfg)
            packed = out['packed'].cpu().numpy()                       # the one download, the one synchronisation
            num_frames, num_runs, runs = packed[:B], packed[B:2 * B], packed[2 * B:].reshape(B, -1, 2)
            result = [self.to_seconds(self.smooth(runs[b, :num_runs[b]], int(num_frames[b]), n[b]), n[b]) for b in range(B)]
            return result[0] if wav.dim() == 1 else result
        rows, n = self._host_rows(wav, lengths)
        result = []
        for b, nb in enumerate(n):
            dec = self._host_frames(rows[b, :nb])[0]
            result.append(self.to_seconds(self.smooth(self.runs_of(dec), dec.shape[0], nb), nb))
        return result[0] if np.ndim(wav) == 1 else result


def _as_host(lengths):
    return lengths.detach().cpu().numpy() if hasattr(lengths, 'detach') else lengths


def _as_tensor(lengths):
    import torch
    return lengths if torch.is_tensor(lengths) else torch.as_tensor(np.asarray(lengths, dtype=np.int64))
