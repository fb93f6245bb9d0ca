"""``MVectorTrainer.evaluate`` with the reference's constructor and return values (mvector/trainer.py:38-86,399-482).

Only the evaluation of a trained model is on the MI355X embedding path; ``train`` / ``export`` / ``extract_features``
raise.  What changed underneath ``evaluate`` (not in its contract):

* GPU: utterances travel as zero-padded waveform batches; one variable-length front-end call per batch featurises every
  row on its own length (``mv_fbank_forward_varlen`` / ``mv_melspec_`` / ``mv_spectrogram_`` / ``mv_mfcc_forward_varlen`` =
  per-utterance featurisation + ``collate_fn`` zero padding of the reference), the native backbone embeds the batch, and
  the trials x enrolment score matrix is one HIP cosine launch instead of a Python loop over sklearn calls
  (trainer.py:452-461).
* CPU (``use_gpu=False``): the reference's flow -- per-item featurisation in the dataset, padded feature batches, torch
  graphs.
* GPU: the metrics (EER, minDCF, threshold) come from the device score matrix and the two label vectors
  (``metrics.verification_metrics``: a radix sort and one scan in the native library); the scores are not downloaded and no
  N-sized label matrix is built.  Equal scores are ordered by their flat (trial-major) index; numpy's default argsort on the
  CPU path leaves that order open, so the two paths return the same floats whenever no target score equals an impostor score.
* CPU: the metrics are computed on the host from the flattened score / label arrays.
"""
import os

import numpy as np
import torch
import yaml
from torch.utils.data import DataLoader

from mvector.data_utils.collate_fn import collate_fn, collate_waveforms
from mvector.data_utils.featurizer import AudioFeaturizer
from mvector.data_utils.reader import MVectorDataset
from mvector.metric.metrics import compute_fnr_fpr, compute_eer, compute_dcf, verification_metrics
from mvector.models import build_model
from mvector.utils.checkpoint import load_pretrained
from mvector.utils.logger import logger
from mvector.utils.utils import dict_to_object, print_arguments


class MVectorTrainer(object):
    def __init__(self, configs, use_gpu=True, data_augment_configs=None):
        """:param configs: YAML path or dict (reference config files work unchanged)
        :param use_gpu: embed on the MI355X (HIP path) or on the CPU (torch graphs)
        :param data_augment_configs: training-only; ignored by ``evaluate``"""
        if use_gpu:
            assert (torch.cuda.is_available()), 'GPU不可用'
            self.device = torch.device('cuda')
        else:
            self.device = torch.device('cpu')
        self.use_gpu = use_gpu
        if isinstance(configs, str):
            with open(configs, 'r', encoding='utf-8') as f:
                configs = yaml.load(f.read(), Loader=yaml.FullLoader)
            print_arguments(configs=configs)
        self.configs = dict_to_object(configs)
        self.model = None
        self.stop_eval = False
        self.audio_featurizer = AudioFeaturizer(feature_method=self.configs.preprocess_conf.feature_method,
                                                use_hf_model=self.configs.preprocess_conf.get('use_hf_model', False),
                                                method_args=self.configs.preprocess_conf.get('method_args', {}))
        # the GPU path batches raw waveforms (every feature method has a variable-length native call); that is implemented for audio
        # lists (not pre-extracted .npy features)
        self._waveform_batches = bool(use_gpu)

    # ---- out of scope -------------------------------------------------------------------------------------------
    def train(self, *args, **kwargs):
        raise NotImplementedError('training is outside the MI355X embedding path (SURVEY.md section 8: out of scope)')

    def export(self, *args, **kwargs):
        raise NotImplementedError('model export is outside the MI355X embedding path; model.pth files of the reference load as is')

    def extract_features(self, *args, **kwargs):
        raise NotImplementedError('offline feature extraction is outside the MI355X embedding path')

    # ---- evaluation ---------------------------------------------------------------------------------------------
    def _loaders(self):
        ds_conf = self.configs.dataset_conf
        args = dict(ds_conf.get('dataset', {}))
        args['max_duration'] = ds_conf.eval_conf.max_duration
        # DataLoader workers as configured (dataLoader.num_workers), also for the GPU path: there the workers only decode and
        # dB-normalise audio (waveform items; featurisation happens on the GPU in the main process), so forked workers never
        # touch the HIP runtime
        loader_args = dict(ds_conf.get('dataLoader', {}))
        lists = [ds_conf.enroll_list, ds_conf.trials_list]
        use_wave = self._waveform_batches and not any(self._has_npy(p) for p in lists)
        out = []
        for path in lists:
            ds = MVectorDataset(data_list_path=path, audio_featurizer=self.audio_featurizer, mode='eval',
                                return_waveform=use_wave, **args)
            out.append(DataLoader(dataset=ds, collate_fn=collate_waveforms if use_wave else collate_fn, shuffle=False,
                                  batch_size=ds_conf.eval_conf.batch_size, **loader_args))
        self.enroll_loader, self.trials_loader = out
        return use_wave

    @staticmethod
    def _has_npy(list_path):
        with open(list_path, 'r', encoding='utf-8') as f:
            return any(line.split('\t')[0].endswith('.npy') for line in f if line.strip())

    def _embed(self, loader, eval_model, use_wave):
        feats, labels = [], []
        with torch.no_grad():
            for data, label, lens in loader:
                if self.stop_eval:
                    break
                data = data.to(self.device)
                if use_wave:
                    data = self.audio_featurizer.forward_varlen(data, lens.to(self.device))
                feats.append(eval_model(data).float())
                labels.append(label)
        return torch.cat(feats), torch.cat(labels).numpy().astype(np.int32)

    def evaluate(self, resume_model=None, save_image_path=None):
        """:return: (eer, min_dcf, threshold) -- floats, as the reference.  With ``use_gpu`` they are computed on the device, equal scores
        ordered by their flat index: identical to the host path unless a target score equals an impostor score (module docstring)."""
        use_wave = self._loaders()
        if self.model is None:
            backbone = build_model(input_size=self.audio_featurizer.feature_dim, configs=self.configs)
            self.model = torch.nn.Sequential(backbone)
        self.model.to(self.device)
        if resume_model is not None:
            if os.path.isdir(resume_model):
                resume_model = os.path.join(resume_model, 'model.pth')
            assert os.path.exists(resume_model), f'{resume_model} 模型不存在！'
            self.model = load_pretrained(self.model, resume_model, use_gpu=self.use_gpu)
        self.model.eval()
        eval_model = self.model if len(self.model) == 1 else self.model[0]

        enroll_features, enroll_labels = self._embed(self.enroll_loader, eval_model, use_wave)
        trials_features, trials_labels = self._embed(self.trials_loader, eval_model, use_wave)
        if self.stop_eval:
            return -1, -1, -1
        logger.info('开始对比音频特征...')
        if self.use_gpu:
            # the score matrix stays on the device; the labels go up as two vectors (flat index = trial-major, the order of the reference's loop)
            from mvector import _hip
            scores = _hip.cosine(trials_features, enroll_features)
            out = verification_metrics(scores, torch.from_numpy(trials_labels), torch.from_numpy(enroll_labels),
                                       return_curve=bool(save_image_path))
            eer, min_dcf, threshold = out[:3]
            fnr, fpr, thresholds = out[3:] if save_image_path else (None, None, None)
        else:
            a = torch.nn.functional.normalize(trials_features, dim=1)
            b = torch.nn.functional.normalize(enroll_features, dim=1)
            scores = (a @ b.t()).numpy()
            # flattened trial-major, exactly the order of the reference's loop (trainer.py:452-461)
            all_score = scores.astype(np.float32).reshape(-1)
            all_labels = (trials_labels[:, None] == enroll_labels[None, :]).astype(np.int32).reshape(-1)
            fnr, fpr, thresholds = compute_fnr_fpr(all_score, all_labels)
            eer, threshold = compute_eer(fnr, fpr, all_score)
            min_dcf = compute_dcf(fnr, fpr)
            eer, min_dcf, threshold = float(eer), float(min_dcf), float(threshold)
        if save_image_path:
            self._save_curve(save_image_path, thresholds, fnr, fpr, eer, threshold)
        return eer, min_dcf, threshold

    def evaluate_normalized(self, cohort_list, top_n=300, mode='s', resume_model=None, save_image_path=None, per_speaker=True):
        """``evaluate`` with cohort score normalisation (``metric.score_norm``: Z-, T-, S-norm, adaptive with ``top_n`` below the cohort size)
        in front of the metrics -> (eer, min_dcf, threshold).  ``cohort_list`` is a data list in the format of ``enroll_list``; its utterances
        are embedded as the other two lists are and, with ``per_speaker``, reduced to one mean embedding per speaker.  With ``use_gpu`` the
        cohort stays on the device, the raw score matrix of ``evaluate`` is normalised in place there (``mv_cohort_stats_f32`` per side, then
        ``mv_score_norm_f32``) and goes to ``verification_metrics`` as it is; on the CPU the same definition runs in numpy."""
        from mvector.metric.score_norm import ScoreNormalizer, cohort_means, cosine_scores
        ds_conf = self.configs.dataset_conf
        use_wave = self._loaders()
        if use_wave and self._has_npy(cohort_list):
            raise ValueError('evaluate_normalized: the cohort list holds .npy features while the enrolment and trial lists hold audio')
        args = dict(ds_conf.get('dataset', {}))
        args['max_duration'] = ds_conf.eval_conf.max_duration
        cohort_set = MVectorDataset(data_list_path=cohort_list, audio_featurizer=self.audio_featurizer, mode='eval', return_waveform=use_wave, **args)
        cohort_loader = DataLoader(dataset=cohort_set, collate_fn=collate_waveforms if use_wave else collate_fn, shuffle=False,
                                   batch_size=ds_conf.eval_conf.batch_size, **dict(ds_conf.get('dataLoader', {})))
        eval_model = self._eval_model(resume_model)
        enroll_features, enroll_labels = self._embed(self.enroll_loader, eval_model, use_wave)
        trials_features, trials_labels = self._embed(self.trials_loader, eval_model, use_wave)
        cohort_features, cohort_labels = self._embed(cohort_loader, eval_model, use_wave)
        if self.stop_eval:
            return -1, -1, -1
        if per_speaker:
            cohort_features = torch.from_numpy(cohort_means(cohort_features, cohort_labels)).to(self.device)
        normalizer = ScoreNormalizer(cohort_features if self.use_gpu else cohort_features.numpy(), top_n=top_n, mode=mode)
        if self.use_gpu:
            scores = cosine_scores(trials_features, enroll_features)
            scores = normalizer.normalize(scores, trial_embeddings=trials_features, enroll_embeddings=enroll_features, out=scores)
        else:
            a = torch.nn.functional.normalize(trials_features, dim=1)
            b = torch.nn.functional.normalize(enroll_features, dim=1)
            scores = normalizer.normalize((a @ b.t()).numpy().astype(np.float32), trial_embeddings=trials_features, enroll_embeddings=enroll_features)
        out = verification_metrics(scores, trials_labels, enroll_labels, return_curve=bool(save_image_path))
        eer, min_dcf, threshold = out[:3]
        if save_image_path:
            self._save_curve(save_image_path, out[5], out[3], out[4], eer, threshold)
        return eer, min_dcf, threshold

    def _eval_model(self, resume_model):
        """the backbone in eval mode on the trainer's device, weights from ``resume_model`` (a file or a folder with model.pth), as
        ``evaluate`` prepares it"""
        if self.model is None:
            backbone = build_model(input_size=self.audio_featurizer.feature_dim, configs=self.configs)
            self.model = torch.nn.Sequential(backbone)
        self.model.to(self.device)
        if resume_model is not None:
            if os.path.isdir(resume_model):
                resume_model = os.path.join(resume_model, 'model.pth')
            assert os.path.exists(resume_model), f'{resume_model} 模型不存在！'
            self.model = load_pretrained(self.model, resume_model, use_gpu=self.use_gpu)
        self.model.eval()
        return self.model if len(self.model) == 1 else self.model[0]

    @staticmethod
    def _save_curve(save_image_path, thresholds, fnr, fpr, eer, threshold):
        """the reference plots FNR / FPR over the threshold (trainer.py:470-481); matplotlib is optional here"""
        try:
            import matplotlib
            matplotlib.use('Agg')
            import matplotlib.pyplot as plt
        except ImportError:
            logger.warning('matplotlib is not installed: evaluation curve not saved')
            return
        os.makedirs(save_image_path, exist_ok=True)
        plt.plot(thresholds, fnr, color='blue', linestyle='-', label='fnr')
        plt.plot(thresholds, fpr, color='red', linestyle='-', label='fpr')
        plt.plot(threshold, eer, 'ro-')
        plt.text(threshold, eer, f'({threshold:.3f}, {eer:.5f})', color='red')
        plt.xlabel('threshold')
        plt.title('fnr and fpr')
        plt.grid(True)
        plt.savefig(os.path.join(save_image_path, 'result.png'))
        plt.close()
