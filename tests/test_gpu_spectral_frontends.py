"""Spectrogram and MFCC front-ends on the MI355X: device against the restatement (tests/spectral_ref.py), batch coupling of the MFCC
dB floor, bit-identity across batch sizes / streams / graph replay, and end-to-end embeddings."""
import numpy as np
import pytest
import torch

import layer_checks as lc
import spectral_ref as sr
from helpers import cos_dist, load_case
from oracle import frontend, models as omodels, weights

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _batch(B=256, L=48000, seed=21):
    wav = frontend.synth_waveforms(B, L, seed=seed)
    ratio = torch.linspace(0.35, 1.0, B)[torch.randperm(B, generator=torch.Generator().manual_seed(seed))]
    return wav, ratio


def _spec_check(out, wav, ratio, args):
    ref = sr.featurize(wav, ratio, 'Spectrogram', args, torch.float64)
    ref32 = sr.featurize(wav, ratio, 'Spectrogram', args)
    bound = 1e-4 * ref.abs().amax(dim=(1, 2), keepdim=True) + 1e-6
    err = (out.cpu().double() - ref).abs()
    print(f'Spectrogram {args}: device max|err|/bound {float((err / bound).max()):.3f}, '
          f'fp32 restatement {float(((ref32.double() - ref).abs() / bound).max()):.3f}')
    assert bool((err <= bound).all())


def _mfcc_check(out, wav, ratio, args, tol=1e-2):
    ref = sr.featurize(wav, ratio, 'MFCC', args, torch.float64)
    ref32 = sr.featurize(wav, ratio, 'MFCC', args)
    err = (out.cpu().double() - ref).abs().max().item()
    print(f'MFCC {args}: device max-abs {err:.2e}, fp32 restatement {(ref32.double() - ref).abs().max().item():.2e}, '
          f'max|ref| {ref.abs().max().item():.1f}')
    assert err <= tol


@pytest.mark.parametrize('args', [{}, dict(n_fft=512), dict(n_fft=600), dict(hop_length=160), dict(normalized=True, pad=11),
                                  dict(pad_mode='constant', power=1.0)], ids=str)
def test_gpu_spectrogram_matches_restatement(args):
    from mvector.data_utils.featurizer import AudioFeaturizer
    wav, ratio = _batch()
    if args:
        wav, ratio = wav[:32], ratio[:32]
    _spec_check(AudioFeaturizer('Spectrogram', method_args=args)(wav.to(DEV), ratio.to(DEV)), wav, ratio, args)


@pytest.mark.parametrize('method,args', [('MelSpectrogram', dict(n_fft=600, n_mels=80)), ('Spectrogram', dict(n_fft=600))], ids=str)
def test_gpu_dense_path_time_mean_and_mask(method, args):
    """the device twin of test_emu_dense_path_time_mean_and_mask: cmn_mask_kernel in place (80 mel columns) and from the padded bin rows
    (301 of 304), two rows, the second one masked"""
    from mvector import _hip
    wav, ratio = frontend.synth_waveforms(2, 6000, seed=12), torch.tensor([1.0, 0.55])
    h = {'MelSpectrogram': _hip.MelSpec, 'Spectrogram': _hip.Spectrogram}[method](args)
    assert h.info()['kernel'] == 'stft_power_kernel (dense DFT)'
    out = h(wav.to(DEV), ratio.to(DEV))
    if method == 'Spectrogram':
        _spec_check(out, wav, ratio, args)
    else:
        lc.melspec_case(_hip.lib(), DEV, wav, ratio, args)
    assert bool((out[1, int(torch.round(ratio[1] * out.shape[1])):] == 0).all()) and bool((out[0] != 0).any())


@pytest.mark.parametrize('args', [{}, dict(n_mfcc=13), dict(n_mfcc=80), dict(norm=None), dict(log_mels=True),
                                  dict(melkwargs=dict(n_mels=40), n_mfcc=13), dict(melkwargs=dict(n_mels=80, n_fft=512, hop_length=160)),
                                  dict(melkwargs=dict(n_fft=600))], ids=str)
def test_gpu_mfcc_matches_restatement(args):
    from mvector.data_utils.featurizer import AudioFeaturizer
    wav, ratio = _batch()
    if args:
        wav, ratio = wav[:32], ratio[:32]
    _mfcc_check(AudioFeaturizer('MFCC', method_args=args)(wav.to(DEV), ratio.to(DEV)), wav, ratio, args)


def test_gpu_mfcc_floor_couples_rows_of_a_call():
    from mvector import _hip
    wav = frontend.synth_waveforms(2, 8000, seed=6)
    wav[0] *= 100.0
    wav[1] *= 1e-3
    h = _hip.Mfcc({})
    both = h(wav.to(DEV))
    _mfcc_check(both, wav, None, {})
    alone = h(wav[1:].to(DEV))
    _mfcc_check(alone, wav[1:], None, {})
    assert (alone[0] - both[1]).abs().max().item() > 1.0


@pytest.mark.parametrize('method,args', [('Spectrogram', {}), ('Spectrogram', dict(n_fft=512)), ('MFCC', dict(log_mels=True))], ids=str)
def test_gpu_row_bits_do_not_depend_on_the_batch_size(method, args):
    """where the semantics are batch-independent, row i carries the same bits at B = 1 / 8 / 256"""
    from mvector import _hip
    h = {'Spectrogram': _hip.Spectrogram, 'MFCC': _hip.Mfcc}[method](args)
    wav, ratio = _batch()
    wav, ratio = wav.to(DEV), ratio.to(DEV)
    full = h(wav, ratio)
    for nb in (1, 8):
        assert torch.equal(h(wav[:nb], ratio[:nb]), full[:nb]), nb
        assert torch.equal(h(wav[256 - nb:], ratio[256 - nb:]), full[256 - nb:]), nb


@pytest.mark.parametrize('method', ['Spectrogram', 'MFCC'])
def test_gpu_one_handle_two_streams_and_graph_replay(method):
    from mvector import _hip
    h = {'Spectrogram': _hip.Spectrogram, 'MFCC': _hip.Mfcc}[method]({})
    wa, ra = _batch(32, 48000, 11)
    wb, rb = _batch(48, 48000 + 160 * 300, 12)
    wa, ra, wb, rb = wa.to(DEV), ra.to(DEV), wb.to(DEV), rb.to(DEV)
    ea, eb = h(wa, ra).clone(), h(wb, rb).clone()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    bad = 0
    for _ in range(20):
        with torch.cuda.stream(s1):
            oa = h(wa, ra)
        with torch.cuda.stream(s2):
            ob = h(wb, rb)
        s1.synchronize()
        s2.synchronize()
        bad += int(not torch.equal(oa, ea)) + int(not torch.equal(ob, eb))
    assert bad == 0, bad
    # captured in a graph (no host synchronisation inside forward) and replayed on new inputs
    static_w, static_r = wa.clone(), ra.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        h(static_w, static_r)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static_out = h(static_w, static_r)
    wc, rc = _batch(32, 48000, 13)
    wc, rc = wc.to(DEV), rc.to(DEV)
    ec = h(wc, rc).clone()
    for w, r, e in ((wc, rc, ec), (wa, ra, ea)):
        static_w.copy_(w)
        static_r.copy_(r)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out, e)


def _tiny_ecapa(input_size, seed):
    from mvector.models import EcapaTdnn
    kw = dict(input_size=input_size, channels=[64, 64, 64, 64, 192])
    model = EcapaTdnn(**kw)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = weights.make_state_dict(shapes, seed)
    model.load_state_dict(sd)
    return model.eval().to(DEV), sd


# (Spectrogram: n_fft 398 = 200 bins.  The native EcapaTdnn takes input sizes that are multiples of 8 -- its first conv refuses the 201 bins of
# the default n_fft 400, which is a limit of the model, not of the front-end.)
@pytest.mark.parametrize('method,args,dim', [('MFCC', {}, 40), ('Spectrogram', dict(n_fft=398), 200)], ids=str)
def test_gpu_ecapa_on_spectral_features_matches_oracle(method, args, dim):
    from mvector.data_utils.featurizer import AudioFeaturizer
    wav, ratio = _batch(16, 48000, 31)
    fz = AudioFeaturizer(method, method_args=args)
    assert fz.feature_dim == dim
    model, sd = _tiny_ecapa(dim, 5)
    with torch.no_grad():
        emb = model(fz(wav.to(DEV), ratio.to(DEV)))
    ref = omodels.ecapa_tdnn(sd, sr.featurize(wav, ratio, method, args))
    d = cos_dist(emb.cpu().numpy(), ref.numpy()).max()
    print(f'{method}: EcapaTdnn(input_size={dim}) 1 - cos {d:.2e}')
    assert d <= 1e-4


def test_gpu_predictor_predict_batch_with_mfcc_config(tmp_path):
    """MVectorPredictor on a `feature_method: MFCC` config: the ragged batch is zero-padded and featurised in one call (the reference's
    predict_batch), so the dB floor is the batch's; compared with the restatement + oracle TDNN"""
    from mvector.predict import MVectorPredictor
    man, sd, _, _, _ = load_case('tdnn')
    model_dir = tmp_path / 'model'
    model_dir.mkdir()
    torch.save({'0.' + k: v for k, v in sd.items()}, str(model_dir / 'model.pth'))
    args = dict(n_mfcc=80)
    cfg = dict(dataset_conf=dict(dataset=dict(min_duration=0.3, sample_rate=16000, use_dB_normalization=True, target_dB=-20),
                                 eval_conf=dict(batch_size=2)),
               preprocess_conf=dict(feature_method='MFCC', method_args=args),
               model_conf=dict(model='TDNN', model_args=dict(embd_dim=192)))
    gpu = MVectorPredictor(cfg, model_path=str(model_dir), use_gpu=True)
    rng = np.random.default_rng(3)
    pcms = [(rng.standard_normal(n) * 3000 * (1 + i)).astype(np.int16) for i, n in enumerate((16000, 12000, 9000, 14500))]
    floats = [p.astype(np.float32) / 32768.0 for p in pcms]
    got = gpu.predict_batch(floats)
    n = torch.tensor([len(p) for p in pcms])
    staged = torch.zeros(len(pcms), int(n.max()), dtype=torch.int16)
    for i, p in enumerate(pcms):
        staged[i, :len(p)] = torch.from_numpy(p)
    wav, _ = frontend.wave_prepare(staged, n, -20.0)
    want = omodels.tdnn(sd, sr.featurize(wav, n.float() / int(n.max()), 'MFCC', args)).numpy()
    d = cos_dist(got, want).max()
    print(f'MFCC predictor: 1 - cos {d:.2e}')
    assert got.shape == (4, 192) and d < 1e-4
