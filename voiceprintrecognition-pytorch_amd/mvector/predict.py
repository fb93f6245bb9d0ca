"""MVectorPredictor with the reference's public API (mvector/predict.py:22-396) on the MI355X-native path.

What changed underneath (not in the signatures): waveforms are padded on the host exactly as the reference
does (predict.py:244-255), moved to the GPU once, featurised there by the fused HIP front-end
(``AudioFeaturizer`` no longer runs on the CPU), embedded by the native backbone, and scored by the HIP cosine
kernel.  With ``use_gpu=False`` everything runs through the torch CPU graphs, as in the reference.
"""
import math
import os
from io import BufferedReader

import numpy as np
import torch
import torch.nn as nn
import yaml

from mvector.data_utils.audio import AudioSegment
from mvector.data_utils.featurizer import AudioFeaturizer
from mvector.models import build_model
from mvector.utils.checkpoint import load_pretrained
from mvector.utils.logger import logger
from mvector.utils.utils import dict_to_object, print_arguments


class MVectorPredictor:
    def __init__(self, configs, threshold=0.6, audio_db_path=None, model_path='models/CAMPPlus_Fbank/best_model/',
                 use_gpu=True):
        """声纹识别预测工具

        :param configs: 配置参数 (YAML path or dict)
        :param threshold: 判断是否为同一个人的阈值
        :param audio_db_path: 声纹库路径
        :param model_path: 导出的预测模型文件夹路径
        :param use_gpu: 是否使用GPU预测
        """
        if use_gpu:
            assert (torch.cuda.is_available()), 'GPU不可用'
            self.device = torch.device("cuda")
        else:
            os.environ['CUDA_VISIBLE_DEVICES'] = '-1'
            self.device = torch.device("cpu")
        self.threshold = threshold
        if isinstance(configs, str):
            with open(configs, 'r', encoding='utf-8') as f:
                configs = yaml.load(f.read(), Loader=yaml.FullLoader)
            print_arguments(configs=configs)
        self.configs = dict_to_object(configs)
        self._audio_featurizer = AudioFeaturizer(feature_method=self.configs.preprocess_conf.feature_method,
                                                 use_hf_model=self.configs.preprocess_conf.get('use_hf_model', False),
                                                 method_args=self.configs.preprocess_conf.get('method_args', {}))
        backbone = build_model(input_size=self._audio_featurizer.feature_dim, configs=self.configs)
        self.predictor = nn.Sequential(backbone)
        self.predictor.to(self.device)
        if os.path.isdir(model_path):
            model_path = os.path.join(model_path, 'model.pth')
        assert os.path.exists(model_path), f"{model_path} 模型不存在！"
        self.predictor = load_pretrained(self.predictor, model_path, use_gpu=use_gpu)
        logger.info(f"成功加载模型参数：{model_path}")
        self.predictor.eval()

        self.audio_db_path = audio_db_path
        self._gallery = None
        if audio_db_path is not None:
            self._open_gallery(audio_db_path)

    # ------------------------------------------------------------------ enrolment gallery (host side)
    def _open_gallery(self, audio_db_path):
        """Load ``audio_indexes.bin`` and embed (in eval-batch-sized batches) every audio file the index does not list yet."""
        from mvector.infer_utils.gallery import SpeakerGallery
        self._gallery = SpeakerGallery(audio_db_path)
        todo = self._gallery.unindexed_audio()
        if todo:
            logger.info('正在加载声纹库数据...')
            step = self.configs.dataset_conf.eval_conf.batch_size
            for lo in range(0, len(todo), step):
                chunk = todo[lo:lo + step]
                if self.device.type == 'cuda' and self._pcm16_frames_batch(chunk) is not None:
                    rows = self.predict_batch(chunk)   # 16-bit files of another rate / channel count: resampled on the device
                else:
                    rows = self.predict_batch([self._load_audio(p).samples for p in chunk])
                for path, row in zip(chunk, rows):
                    self._gallery.add(os.path.basename(os.path.dirname(path)), path, row)
            self._gallery.save()
        users, _ = self._gallery.user_means()
        if users:
            logger.info(f'声纹库数据加载完成，一共有{len(users)}个用户，分别是：{users}')
        self._device_gallery = None
        if self.device.type == 'cuda':
            # GPU-resident enrolment matrix (per-user sums): recognition scores against it without re-uploading anything
            from mvector.infer_utils.gallery import DeviceGallery
            self._device_gallery = DeviceGallery.from_gallery(self._gallery, self.device, self.predictor[0].embd_dim)

    # ------------------------------------------------------------------ scoring
    @staticmethod
    def normalize_features(features):
        return features / np.linalg.norm(features, axis=1, keepdims=True)

    def _cosine(self, queries, gallery):
        """[N, D] x [M, D] -> [N, M]; HIP kernel on the GPU predictor, numpy otherwise."""
        queries = np.asarray(queries, dtype=np.float32)
        gallery = np.asarray(gallery, dtype=np.float32)
        if self.device.type == 'cuda':
            from mvector import _hip
            return _hip.cosine(torch.from_numpy(queries).to(self.device), torch.from_numpy(gallery).to(self.device)).cpu().numpy()
        return self.normalize_features(queries) @ self.normalize_features(gallery).T

    def _best_matches(self, embeddings):
        """[name, score] of the best enrolled user per query row, or [None, None] below the threshold.  ``embeddings``: array
        or (GPU predictor) a device tensor, which is searched against the device-resident gallery by mv_cosine_topk_f32: the scores are
        those of mv_cosine_f32 and the first maximum wins, as np.argmax picks it, but only one score and one index per query come down."""
        if getattr(self, '_device_gallery', None) is not None:
            users = self._device_gallery.users
            q = embeddings if torch.is_tensor(embeddings) else torch.as_tensor(np.atleast_2d(np.asarray(embeddings, dtype=np.float32)))
            scores, index = self._device_gallery.search(q.to(self.device), 1, to_host=True)
            return [[users[i], round(float(s), 5)] if i >= 0 and s >= self.threshold else [None, None] for s, i in zip(scores[:, 0], index[:, 0])]
        users, means = self._gallery.user_means()
        scores = self._cosine(np.atleast_2d(np.asarray(embeddings, dtype=np.float32)), means)
        out = []
        for row in scores:
            best = int(np.argmax(row))
            out.append([users[best], round(float(row[best]), 5)] if row[best] >= self.threshold else [None, None])
        return out

    def _top_matches(self, embeddings, top_k):
        """per query row [[name, score], ...] of the min(top_k, users) best enrolled users, best first (equal scores: the user enrolled first),
        scores rounded as ``_best_matches`` rounds them, no threshold"""
        if getattr(self, '_device_gallery', None) is not None:
            users = self._device_gallery.users
            k = min(int(top_k), len(users))
            if k < 1:
                return [[] for _ in range(embeddings.reshape(-1, embeddings.shape[-1]).shape[0])]
            q = embeddings if torch.is_tensor(embeddings) else torch.as_tensor(np.atleast_2d(np.asarray(embeddings, dtype=np.float32)))
            scores, index = self._device_gallery.search(q.to(self.device), k, to_host=True)
        else:
            from mvector.infer_utils.gallery import top_k_of_scores
            users, means = self._gallery.user_means()
            queries = np.atleast_2d(np.asarray(embeddings, dtype=np.float32))
            k = min(int(top_k), len(users))
            if k < 1:
                return [[] for _ in range(queries.shape[0])]
            scores, index = top_k_of_scores(self._cosine(queries, means), k)
        return [[[users[i], round(float(s), 5)] for s, i in zip(srow, irow)] for srow, irow in zip(scores, index)]

    # ------------------------------------------------------------------ audio in
    def _load_audio(self, audio_data, sample_rate=16000):
        """支持文件路径，文件对象，字节，numpy，AudioSegment对象"""
        if isinstance(audio_data, (str, BufferedReader)):
            audio_segment = AudioSegment.from_file(audio_data)
        elif isinstance(audio_data, np.ndarray):
            audio_segment = AudioSegment.from_ndarray(audio_data, sample_rate)
        elif isinstance(audio_data, bytes):
            audio_segment = AudioSegment.from_bytes(audio_data)
        elif isinstance(audio_data, AudioSegment):
            audio_segment = audio_data
        else:
            raise Exception(f'不支持该数据类型，当前数据类型为：{type(audio_data)}')
        dataset = self.configs.dataset_conf.dataset
        assert audio_segment.duration >= dataset.min_duration, \
            f'音频太短，最小应该为{dataset.min_duration}s，当前音频为{audio_segment.duration}s'
        if audio_segment.sample_rate != dataset.sample_rate:
            audio_segment.resample(dataset.sample_rate)
        if dataset.use_dB_normalization:
            audio_segment.normalize(target_db=dataset.target_dB)
        return audio_segment

    # ------------------------------------------------------------------ embedding extraction (the hot path)
    @torch.no_grad()
    def _embed(self, audio_data, sample_rate=16000):
        """one utterance -> embedding tensor [1, embd_dim] on the predictor's device"""
        input_data = self._load_audio(audio_data=audio_data, sample_rate=sample_rate)
        wav = torch.tensor(input_data.samples, dtype=torch.float32).unsqueeze(0).to(self.device)
        return self.predictor(self._audio_featurizer(wav)).data

    def predict(self, audio_data, sample_rate=16000, vad=None):
        """预测一个音频的特征 -> np.ndarray [embd_dim]

        :param vad: None = the whole audio, as always; True or an ``EnergyVad`` = embed the speech only (``predict_batch`` says how)"""
        if vad is None:
            return self._embed(audio_data, sample_rate).cpu().numpy()[0]
        return self._embed_speech(audio_data, sample_rate, vad).cpu().numpy()[0]

    # ------------------------------------------------------------------ speech only: VAD -> regions -> gather in front of the front-end
    def _embedding_vad(self, vad):
        """``vad=`` of predict / predict_batch -> the EnergyVad to trim with (True: compute-vad's defaults at the configured rate)"""
        from mvector.infer_utils.vad import EnergyVad
        rate = self.configs.dataset_conf.dataset.sample_rate
        if vad is True:
            if getattr(self, '_trim_vad', None) is None or self._trim_vad.sample_rate != rate:
                self._trim_vad = EnergyVad(sample_rate=rate)
            return self._trim_vad
        assert isinstance(vad, EnergyVad), f'vad: None, True or an EnergyVad, not {type(vad)}'
        assert vad.sample_rate == rate, f'the VAD is set up for {vad.sample_rate} Hz, the audio has {rate} Hz'
        return vad

    def _trim_batch(self, wav, lens, vad):
        """the prepared batch ``wav`` [B, L] (a tensor on the predictor's device) with the rows' sample counts ``lens`` -> (the rows' speech
        regions one behind the other, cut to the longest kept row; the kept sample counts as a list).  GPU predictor: EnergyVad.trim on the
        device, the [B] kept counts are the one thing that comes down; ``use_gpu=False``: the same definition in numpy.  A row that keeps less
        than min_duration is refused as _load_audio refuses a short file."""
        dataset = self.configs.dataset_conf.dataset
        vad = self._embedding_vad(vad)
        if wav.is_cuda:
            trimmed, kept = vad.trim(wav, lengths=torch.as_tensor(lens, dtype=torch.int64))
            kept = kept.cpu().tolist()
        else:
            trimmed, kept = vad.trim(wav.numpy(), lengths=lens)
            trimmed, kept = torch.from_numpy(trimmed), kept.tolist()
        min_samples = int(math.ceil(round(dataset.min_duration * dataset.sample_rate, 6)))
        for i, k in enumerate(kept):
            assert k >= min_samples, (f'音频太短，最小应该为{dataset.min_duration}s，当前音频为{k / dataset.sample_rate}s '
                                      f'(item {i}: {k} samples of speech are left by the VAD, {min_samples} are needed)')
        return trimmed[:, :max(kept)], kept

    @torch.no_grad()
    def _embed_speech(self, audio_data, sample_rate, vad):
        """``_embed`` of the speech regions of one utterance"""
        input_data = self._load_audio(audio_data=audio_data, sample_rate=sample_rate)
        wav = torch.tensor(input_data.samples, dtype=torch.float32).unsqueeze(0).to(self.device)
        wav, _ = self._trim_batch(wav, [wav.shape[1]], vad)
        return self.predictor(self._audio_featurizer(wav)).data

    def _pcm16_batch(self, audios_data):
        """Raw int16 mono PCM at the configured rate for EVERY item (paths / bytes of 16-bit mono WAVs), else None.
        Such batches travel to the GPU as int16 (half the PCIe bytes) and are scaled / dB-normalised there."""
        from mvector.data_utils.audio import read_pcm16
        dataset = self.configs.dataset_conf.dataset
        out = []
        for a in audios_data:
            if not isinstance(a, (str, bytes)):
                return None
            got = read_pcm16(a)
            if got is None or got[1] != dataset.sample_rate:
                return None
            duration = got[0].shape[0] / float(got[1])
            assert duration >= dataset.min_duration, f'音频太短，最小应该为{dataset.min_duration}s，当前音频为{duration}s'
            out.append(got[0])
        return out

    @torch.no_grad()
    def _predict_batch_pcm16(self, pcms, batch_size, vad=None):
        """GPU fast path of predict_batch: same padding / length-ratio semantics (predict.py:244-255), int16 upload from
        pinned memory, int16 -> float + dB normalisation + front-end + CMN + mask + backbone on the device."""
        from mvector import _hip
        dataset = self.configs.dataset_conf.dataset
        lens = [p.shape[0] for p in pcms]
        max_len = max(lens)
        staging = torch.zeros((len(pcms), max_len), dtype=torch.int16)
        if torch.cuda.is_available():
            staging = staging.pin_memory()
        for i, p in enumerate(pcms):
            staging[i, :lens[i]] = torch.from_numpy(np.ascontiguousarray(p))
        pcm = staging.to(self.device, non_blocking=True)
        n = torch.tensor(lens, dtype=torch.int64, device=self.device)
        wav, too_quiet = _hip.wave_prepare(pcm, n, dataset.target_dB if dataset.use_dB_normalization else None)
        if vad is not None:
            wav, lens = self._trim_batch(wav, lens, vad)
            max_len = wav.shape[1]
        ratio = torch.tensor([l / max_len for l in lens], dtype=torch.float32, device=self.device)
        audio_feature = self._audio_featurizer(wav, ratio)
        step = max(int(batch_size), 256)  # 288 GB of HBM: the reference's 32-row chunks only multiply launches
        features = [self.predictor(audio_feature[i:i + step]).data for i in range(0, len(pcms), step)]
        out = torch.cat(features, dim=0).cpu().numpy()
        if bool(too_quiet.any().item()):
            raise ValueError(f'无法将段规范化到{dataset.target_dB}dB，音频增益已经超过max_gain_db (300.0dB)')
        return out

    # ---- 16-bit PCM of other rates / channel counts: down-mix, resampling and normalisation on the device (mv_resampler_*)
    def _resample_ratio(self, rate):
        dataset = self.configs.dataset_conf.dataset
        g = math.gcd(int(dataset.sample_rate), int(rate))
        return int(dataset.sample_rate) // g, int(rate) // g

    def _pcm16_frames_batch(self, audios_data):
        """[(int16 frames [n, channels], rate)] for EVERY item when all are paths / bytes of 16-bit PCM WAVs the device resampler takes (1 .. 8
        channels, max(up, down) <= 1024) and at least one is not mono at the configured rate, else None."""
        from mvector.data_utils.audio import read_pcm16_frames
        dataset = self.configs.dataset_conf.dataset
        out, foreign = [], False
        for a in audios_data:
            if not isinstance(a, (str, bytes)):
                return None
            got = read_pcm16_frames(a)
            if got is None or got[1] <= 0 or not 1 <= got[0].shape[1] <= 8 or max(self._resample_ratio(got[1])) > 1024:
                return None
            duration = got[0].shape[0] / float(got[1])   # of the source, as _load_audio asserts it before it resamples
            assert duration >= dataset.min_duration, f'音频太短，最小应该为{dataset.min_duration}s，当前音频为{duration}s'
            foreign = foreign or got[1] != dataset.sample_rate or got[0].shape[1] != 1
            out.append(got)
        return out if foreign else None

    @staticmethod
    def _resample_groups(frames):
        """{(rate, channels): [(batch index, frames), ...]} in first-seen order"""
        groups = {}
        for i, (f, rate) in enumerate(frames):
            groups.setdefault((rate, f.shape[1]), []).append((i, f))
        return groups

    def _resampled_lengths(self, frames):
        """samples of every item at the configured rate: ceil(n * up / down), from the frame counts alone"""
        out = []
        for f, rate in frames:
            up, down = self._resample_ratio(rate)
            out.append(-(-f.shape[0] * up // down))
        return out

    def _resampler(self, rate):
        from mvector import _hip
        cache = self.__dict__.setdefault('_resamplers', {})
        if rate not in cache:
            cache[rate] = _hip.Resampler(rate, self.configs.dataset_conf.dataset.sample_rate)
        return cache[rate]

    @torch.no_grad()
    def _predict_batch_resampled(self, frames, batch_size, vad=None):
        """GPU path of predict_batch for 16-bit files that are not all mono at the configured rate: per (rate, channels) group one pinned int16
        staging buffer, one upload and one call of the group's Resampler (target-rate mono rows: wave_prepare, as the pcm16 path), written into
        one [B, max n_out] batch; the length ratios come from the frame counts on the host -- nothing waits for the device."""
        from mvector import _hip
        dataset = self.configs.dataset_conf.dataset
        target_db = dataset.target_dB if dataset.use_dB_normalization else None
        lens = self._resampled_lengths(frames)
        max_len = max(lens)
        wav = torch.zeros((len(frames), max_len), dtype=torch.float32, device=self.device)
        flags = []
        for (rate, channels), members in self._resample_groups(frames).items():
            n_in = [f.shape[0] for _, f in members]
            staging = torch.zeros((len(members), max(n_in), channels), dtype=torch.int16)
            if torch.cuda.is_available():
                staging = staging.pin_memory()
            host = staging.numpy()   # (a view of the pinned buffer: the decoded frames may be read-only arrays)
            for r, (_, f) in enumerate(members):
                host[r, :n_in[r]] = f
            pcm = staging.to(self.device, non_blocking=True)
            n = torch.tensor(n_in, dtype=torch.int64, device=self.device)
            if rate == dataset.sample_rate and channels == 1:
                rows, quiet = _hip.wave_prepare(pcm[:, :, 0], n, target_db)
            else:
                rows, _, quiet = self._resampler(rate)(pcm, n, target_db)
            index = torch.tensor([i for i, _ in members], dtype=torch.int64, device=self.device)
            wav[index, :rows.shape[1]] = rows
            flags.append(quiet)
        if vad is not None:
            wav, lens = self._trim_batch(wav, lens, vad)
            max_len = wav.shape[1]
        ratio = torch.tensor([l / max_len for l in lens], dtype=torch.float32, device=self.device)
        audio_feature = self._audio_featurizer(wav, ratio)
        step = max(int(batch_size), 256)
        features = [self.predictor(audio_feature[i:i + step]).data for i in range(0, len(frames), step)]
        out = torch.cat(features, dim=0).cpu().numpy()
        if bool(torch.cat(flags).any().item()):
            raise ValueError(f'无法将段规范化到{dataset.target_dB}dB，音频增益已经超过max_gain_db (300.0dB)')
        return out

    @torch.no_grad()
    def predict_batch(self, audios_data, sample_rate=16000, batch_size=32, vad=None):
        """预测一批音频的特征 -> np.ndarray [B, embd_dim] (row order = input order)

        :param vad: None = the whole audio, as always.  True (compute-vad's defaults at the configured rate) or an ``EnergyVad`` = embed the
                    speech only: the batch is prepared exactly as without it (int16 upload, resampling, dB normalisation, on whichever of the
                    three batch paths applies), then every row's speech regions are moved together on the device (``EnergyVad.trim``:
                    mv_vad_energy_f32, mv_vad_regions_i32, mv_wave_gather_f32), the [B] kept sample counts come down -- the one added
                    synchronisation --, the batch is cut to the longest kept row and the length ratios are those of the kept counts.
                    ``use_gpu=False``: the same in numpy.  The VAD sees the dB-normalised waveform, as ``vad`` does, and the gain is NOT
                    recomputed from the speech that is left.  A row that keeps less than min_duration of speech (a row of silence, say)
                    raises the assertion a short file raises, with the item's index."""
        self._last_batch_path = 'host'
        if self.device.type == 'cuda':   # every feature method: wave_prepare and the ratio form of the front-end serve all four
            pcms = self._pcm16_batch(audios_data)
            if pcms is not None:
                self._last_batch_path = 'pcm16'
                return self._predict_batch_pcm16(pcms, batch_size, vad)
            frames = self._pcm16_frames_batch(audios_data)
            if frames is not None:
                self._last_batch_path = 'pcm16_resampled'
                return self._predict_batch_resampled(frames, batch_size, vad)
        samples = [self._load_audio(audio_data=a, sample_rate=sample_rate).samples for a in audios_data]
        max_len = max(s.shape[0] for s in samples)
        inputs = np.zeros((len(samples), max_len), dtype=np.float32)
        ratios = []
        for i, s in enumerate(samples):
            inputs[i, :s.shape[0]] = s
            ratios.append(s.shape[0] / max_len)
        wav = torch.from_numpy(inputs).to(self.device)
        if vad is not None:
            wav, kept = self._trim_batch(wav, [s.shape[0] for s in samples], vad)
            ratios = [k / wav.shape[1] for k in kept]
        ratio = torch.tensor(ratios, dtype=torch.float32, device=self.device)
        audio_feature = self._audio_featurizer(wav, ratio)
        features = []
        for i in range(0, len(samples), batch_size):
            features.append(self.predictor(audio_feature[i:i + batch_size]).data)
        return torch.cat(features, dim=0).cpu().numpy()

    def contrast(self, audio_data1, audio_data2):
        """声纹对比 -> 两个音频的相似度"""
        feature1 = self.predict(audio_data1)
        feature2 = self.predict(audio_data2)
        return np.dot(feature1, feature2) / (np.linalg.norm(feature1) * np.linalg.norm(feature2))

    def contrast_normalized(self, audio_data1, audio_data2, normalizer):
        """``contrast`` with cohort score normalisation -> float: the cosine of the two embeddings, normalised by ``normalizer`` (a
        ``metric.score_norm.ScoreNormalizer``; mode 's' with the first audio as the trial, the second as the enrolment).  On the GPU predictor
        the embeddings stay on the device: mv_cosine_f32, mv_cohort_stats_f32 per side and mv_score_norm_f32, one float comes down."""
        from mvector.metric.score_norm import cosine_scores
        e1, e2 = self._embed(audio_data1), self._embed(audio_data2)
        if self.device.type != 'cuda':
            e1, e2 = e1.numpy(), e2.numpy()
        score = normalizer.normalize(cosine_scores(e1, e2), trial_embeddings=e1, enroll_embeddings=e2)
        return float(score[0, 0])

    def register(self, audio_data, user_name: str, sample_rate=16000):
        """声纹注册"""
        audio_segment = self._load_audio(audio_data=audio_data, sample_rate=sample_rate)
        emb = self._embed(audio_segment)
        audio_path = self._gallery.next_audio_path(user_name)
        audio_segment.to_wav_file(audio_path)
        self._gallery.add(user_name, audio_path, emb.cpu().numpy()[0])
        self._gallery.save()
        if getattr(self, '_device_gallery', None) is not None:
            self._device_gallery.add(user_name, emb[0])  # the embedding never leaves the device for the resident matrix
        return True, "注册成功"

    def recognition(self, audio_data, threshold=None, sample_rate=16000):
        """声纹识别 -> [user name or None, score or None]"""
        if threshold:
            self.threshold = threshold
        return self._best_matches(self._embed(audio_data, sample_rate=sample_rate))[0]

    def recognition_batch(self, audios_data, threshold=None, sample_rate=16000, batch_size=32):
        """一批音频的声纹识别 -> one [user name or None, score or None] per item, exactly what ``recognition`` answers for each.
        Every item is embedded as ``recognition`` embeds it (one at a time: the padded batches of ``predict_batch`` prepare the audio by other
        arithmetic -- on the device from int16, with length ratios -- and their scores differ from ``recognition``'s in the last rounded digit,
        which near the threshold is another answer); the embeddings stay on the predictor's device, where one search takes them all, so a
        batch costs one synchronisation and one download of B scores and indices instead of one of each per item.  ``batch_size`` is accepted
        for the call shape of ``predict_batch`` and not used."""
        if threshold:
            self.threshold = threshold
        if len(audios_data) == 0:
            return []
        return self._best_matches(torch.cat([self._embed(a, sample_rate=sample_rate) for a in audios_data], dim=0))

    def search(self, audio_data, top_k=5, sample_rate=16000):
        """声纹检索 -> [[user name, score], ...]: the min(top_k, users) most similar enrolled users, best first, no threshold applied
        (GPU predictor: top_k <= 64, the limit of mv_cosine_topk_f32)"""
        return self._top_matches(self._embed(audio_data, sample_rate=sample_rate), top_k)[0]

    def get_users(self):
        """One entry per enrolled audio, as the reference returns its ``users_name`` list."""
        return list(self._gallery.names)

    def remove_user(self, user_name):
        ok = self._gallery.remove(user_name)
        if ok and getattr(self, '_device_gallery', None) is not None:
            self._device_gallery.remove(user_name)
        return ok

    @torch.no_grad()
    def _embed_chunks_device(self, samples, starts, lens, chunk_len, batch_size=256):
        """GPU path of speaker_diarization: the recording goes up ONCE, mv_wave_chunks_f32 cuts (and dB-normalises) the chunk rows there, the
        front-end and the backbone run in steps of at least 256 rows -> embeddings [n, embd_dim] that stay on the device."""
        from mvector import _hip
        dataset = self.configs.dataset_conf.dataset
        wav = torch.from_numpy(np.ascontiguousarray(samples, dtype=np.float32)).to(self.device)
        rows, too_quiet = _hip.wave_chunks(wav, torch.from_numpy(starts), torch.from_numpy(lens), chunk_len,
                                           dataset.target_dB if dataset.use_dB_normalization else None)
        step = max(int(batch_size), 256)
        features = []
        for i in range(0, rows.shape[0], step):
            part = rows[i:i + step]
            ratio = torch.ones((part.shape[0],), dtype=torch.float32, device=self.device)   # every row is chunk_len long, as in predict_batch
            features.append(self.predictor(self._audio_featurizer(part, ratio)).data)
        if bool(too_quiet.any().item()):
            raise ValueError(f'无法将段规范化到{dataset.target_dB}dB，音频增益已经超过max_gain_db (300.0dB)')
        return torch.cat(features, dim=0)

    def vad(self, audio_data, sample_rate=16000, vad=None):
        """语音活动检测 -> [{'start': seconds, 'end': seconds}]: the speech regions of a recording by the energy VAD
        (mvector/infer_utils/vad.py), in the shape ``speaker_diarization`` takes as ``vad_segments``.

        :param audio_data: 需要识别的数据，支持文件路径，文件对象，字节，numpy，AudioSegment对象
        :param sample_rate: 如果传入的是numpy数据，需要指定采样率
        :param vad: an ``EnergyVad`` with other settings (its sample_rate must be the configured one); None = compute-vad's defaults

        The audio is loaded as ``speaker_diarization`` loads it (resampling, dB normalisation), so the times line up.  GPU predictor: the
        samples go up once and mv_vad_energy_f32 runs there, the list of runs comes down; ``use_gpu=False``: the same definition in numpy."""
        from mvector.infer_utils.vad import EnergyVad
        input_data = self._load_audio(audio_data=audio_data, sample_rate=sample_rate)
        if vad is None:
            if getattr(self, 'energy_vad', None) is None or self.energy_vad.sample_rate != input_data.sample_rate:
                self.energy_vad = EnergyVad(sample_rate=input_data.sample_rate)
            vad = self.energy_vad
        assert vad.sample_rate == input_data.sample_rate, f'the VAD is set up for {vad.sample_rate} Hz, the audio has {input_data.sample_rate} Hz'
        samples = np.ascontiguousarray(input_data.samples, dtype=np.float32)
        if self.device.type == 'cuda':
            return vad(torch.from_numpy(samples).to(self.device))
        return vad(samples)

    def speaker_diarization(self, audio_data, sample_rate=16000, speaker_num=None, search_audio_db=False, vad_segments=None):
        """说话人日志识别 -> [{'speaker', 'start', 'end'}]

        :param audio_data: 需要识别的数据，支持文件路径，文件对象，字节，numpy，AudioSegment对象
        :param sample_rate: 如果传入的是numpy数据，需要指定采样率
        :param speaker_num: 预期的说话人数量，提供说话人数量可以提高准确率 (at most 16 on the GPU predictor)
        :param search_audio_db: 是否在声纹库中搜索说话人的名字
        :param vad_segments: speech regions [{'start': seconds, 'end': seconds}, ...] (the shape yeaudio's VAD returns); needed unless
                             ``audio_data`` is a segment object with a ``vad`` method -- this package ships no VAD

        GPU predictor: one upload of the recording, chunk rows / front-end / backbone / cosine / pruned Laplacian / lowest eigenpairs on
        the device (mvector/infer_utils/speaker_diarization.py), k_means and the merging on the host.  ``use_gpu=False``: predict_batch
        and the host classes, as the reference."""
        from mvector.infer_utils.speaker_diarization import SpeakerDiarization
        if getattr(self, 'speaker_diarize', None) is None:
            self.speaker_diarize = SpeakerDiarization()
        input_data = self._load_audio(audio_data=audio_data, sample_rate=sample_rate)
        if self.device.type == 'cuda':
            dataset = self.configs.dataset_conf.dataset
            segments, starts, lens, chunk_len = self.speaker_diarize.chunk_table(input_data, vad_segments=vad_segments)
            duration = chunk_len / float(input_data.sample_rate)   # the reference loads every (padded) chunk through _load_audio
            assert duration >= dataset.min_duration, f'音频太短，最小应该为{dataset.min_duration}s，当前音频为{duration}s'
            features = self._embed_chunks_device(input_data.samples, starts, lens, chunk_len)
        else:
            segments = self.speaker_diarize.segments_audio(input_data, vad_segments=vad_segments)
            features = self.predict_batch([segment[2] for segment in segments], sample_rate=input_data.sample_rate)
        labels, spk_center_embeddings = self.speaker_diarize.clustering(features, speaker_num=speaker_num)
        outputs = self.speaker_diarize.postprocess(segments, labels)
        if search_audio_db:
            assert self._gallery is not None and len(self._gallery.names) > 0, "数据库中没有音频数据，请先指定说话人特征数据库或者注册说话人"
            names = self._best_matches(spk_center_embeddings)
            outputs = [{'speaker': names[o['speaker']][0] if names[o['speaker']][0] else f"陌生人{o['speaker']}", 'start': o['start'],
                        'end': o['end']} for o in outputs]
        return outputs
