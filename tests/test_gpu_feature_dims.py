"""Feature widths that are not multiples of 8 on the MI355X: EcapaTdnn / TDNN / CAM++ on the front-ends that produce them (the default
Spectrogram's 201 bins, Fbank's default 23, MFCC 13) against the oracle, the batch / stream / graph invariants at F = 201, the padding
contract (F = 201 gives the bits of F = 208 with zero-padded features and first-layer weights) and a Spectrogram predictor."""
import numpy as np
import pytest
import torch

import spectral_ref as sr
from helpers import cos_dist
from oracle import frontend, models as omodels, weights

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _batch(B=16, L=48000, seed=31):
    wav = frontend.synth_waveforms(B, L, seed=seed)
    ratio = torch.linspace(0.35, 1.0, B)[torch.randperm(B, generator=torch.Generator().manual_seed(seed))]
    return wav, ratio


def _model(cls, kw, seed=5):
    import mvector.models as M
    m = getattr(M, cls)(**kw)
    sd = weights.make_state_dict(weights.shapes_of(m.state_dict()), seed)
    m.load_state_dict(sd)
    return m.eval().to(DEV), sd


def _tiny_ecapa(F, dil0=1):
    return _model('EcapaTdnn', dict(input_size=F, channels=[64, 64, 64, 64, 192], dilations=[dil0, 2, 3, 4, 1]))


# MFCC features (c0 up to ~44 after the time mean) cost the native backbones' fp16 operands more than Fbank / Spectrogram features do, at ANY width:
# on this batch the aligned n_mfcc 40, where nothing is padded, measures 1 - cos 6e-5 (EcapaTdnn) and 2.3e-4 (CAM++, fp32 head 2.3e-4 as well), the
# device features themselves are within 1.5e-4 of the fp64 arbiter and move the oracle's embedding by < 1e-10.  The MFCC rows therefore hold the
# bar the aligned width meets, 5e-4; what the padding adds is checked bitwise (test_gpu_mfcc13_gives_the_bits_of_the_zero_padded_16).
MFCC_BAR = 5e-4


@pytest.mark.parametrize('method,args,dim,bar', [('Spectrogram', {}, 201, 1e-4), ('MFCC', dict(n_mfcc=13), 13, MFCC_BAR)], ids=str)
def test_gpu_ecapa_on_ragged_spectral_features_matches_oracle(method, args, dim, bar):
    from mvector.data_utils.featurizer import AudioFeaturizer
    wav, ratio = _batch()
    fz = AudioFeaturizer(method, method_args=args)
    assert fz.feature_dim == dim
    model, sd = _tiny_ecapa(dim)
    with torch.no_grad():
        emb = model(fz(wav.to(DEV), ratio.to(DEV)))
    ref = omodels.ecapa_tdnn(sd, sr.featurize(wav, ratio, method, args))
    d = cos_dist(emb.cpu().numpy(), ref.numpy()).max()
    print(f'{method} {args}: EcapaTdnn(input_size={dim}) 1 - cos {d:.2e}')
    assert d <= bar


def test_gpu_mfcc13_gives_the_bits_of_the_zero_padded_16():
    """EcapaTdnn on the device's MFCC-13 features: the bits of the same model at 16 with zero-padded features and block-0 weights"""
    from mvector import _hip
    from mvector.data_utils.featurizer import AudioFeaturizer
    wav, ratio = _batch()
    x = AudioFeaturizer('MFCC', method_args=dict(n_mfcc=13))(wav.to(DEV), ratio.to(DEV))
    m13, sd = _tiny_ecapa(13)
    m16, _ = _tiny_ecapa(16)
    sd16 = dict(sd)
    w = sd['blocks.0.conv.conv.weight']
    sd16['blocks.0.conv.conv.weight'] = torch.cat([w, torch.zeros(w.shape[0], 3, w.shape[2])], dim=1)
    a = _hip.Model('ecapa', m13._native_cfg(), {k: v.to(DEV) for k, v in sd.items()}).forward(x)
    b = _hip.Model('ecapa', m16._native_cfg(), {k: v.to(DEV) for k, v in sd16.items()}).forward(
        torch.cat([x, torch.zeros(*x.shape[:2], 3, device=DEV)], dim=2))
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_gpu_tdnn_on_default_fbank_matches_oracle():
    """Fbank without num_mel_bins: torchaudio's default 23 bins"""
    from mvector.data_utils.featurizer import AudioFeaturizer
    wav, ratio = _batch()
    args = dict(sample_frequency=16000)
    fz = AudioFeaturizer('Fbank', method_args=args)
    assert fz.feature_dim == 23
    model, sd = _model('TDNN', dict(input_size=23, embd_dim=192))
    with torch.no_grad():
        emb = model(fz(wav.to(DEV), ratio.to(DEV)))
    ref = omodels.tdnn(sd, frontend.audio_featurizer(wav, ratio, 'Fbank', args))
    d = cos_dist(emb.cpu().numpy(), ref.numpy()).max()
    print(f'Fbank default: TDNN(input_size=23) 1 - cos {d:.2e}')
    assert d <= 1e-4


@pytest.mark.parametrize('method,args,dim,bar', [('Spectrogram', {}, 201, 1e-4), ('Fbank', dict(sample_frequency=16000), 23, 1e-4),
                                              ('MFCC', dict(n_mfcc=13), 13, MFCC_BAR)], ids=str)
def test_gpu_campp_at_ragged_feature_width_matches_oracle(method, args, dim, bar):
    """CAM++ rounds the frequency axis up itself (F8 = ceil(F / 8) rows of 32 after the FCM head): odd heights through the strided head"""
    from mvector.data_utils.featurizer import AudioFeaturizer
    wav, ratio = _batch(8)
    fz = AudioFeaturizer(method, method_args=args)
    assert fz.feature_dim == dim
    model, sd = _model('CAMPPlus', dict(input_size=dim, embd_dim=192))
    with torch.no_grad():
        emb = model(fz(wav.to(DEV), ratio.to(DEV)))
    feats = frontend.audio_featurizer(wav, ratio, method, args) if method == 'Fbank' else sr.featurize(wav, ratio, method, args)
    ref = omodels.campplus(sd, feats)
    d = cos_dist(emb.cpu().numpy(), ref.numpy()).max()
    print(f'{method} {args}: CAMPPlus(input_size={dim}) 1 - cos {d:.2e}')
    assert d <= bar


def _feats(B, T, F, seed):
    return (torch.randn(B, T, F, generator=torch.Generator().manual_seed(seed)) * 2).to(DEV)


@pytest.mark.parametrize('cls,dil0', [('EcapaTdnn', 1), ('EcapaTdnn', 2), ('TDNN', 1)], ids=['ecapa-window', 'ecapa-per-tap', 'tdnn'])
def test_gpu_row_bits_at_201_do_not_depend_on_the_batch_size(cls, dil0):
    model, _ = _tiny_ecapa(201, dil0) if cls == 'EcapaTdnn' else _model('TDNN', dict(input_size=201, embd_dim=192))
    x = _feats(130, 300, 201, 3)
    with torch.no_grad():
        full = model(x)
        for nb in (1, 8, 40):
            assert torch.equal(model(x[:nb]), full[:nb]), nb
            assert torch.equal(model(x[130 - nb:]), full[130 - nb:]), nb


def test_gpu_201_one_handle_two_streams_and_graph_replay():
    model, _ = _tiny_ecapa(201)
    xa, xb = _feats(32, 300, 201, 11), _feats(48, 360, 201, 12)
    with torch.no_grad():
        ea, eb = model(xa).clone(), model(xb).clone()
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        bad = 0
        for _ in range(20):
            with torch.cuda.stream(s1):
                oa = model(xa)
            with torch.cuda.stream(s2):
                ob = model(xb)
            s1.synchronize()
            s2.synchronize()
            bad += int(not torch.equal(oa, ea)) + int(not torch.equal(ob, eb))
        assert bad == 0, bad
        static_x = xa.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model(static_x)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            static_out = model(static_x)
        xc = _feats(32, 300, 201, 13)
        ec = model(xc).clone()
        for x, e in ((xc, ec), (xa, ea)):
            static_x.copy_(x)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_out, e)


@pytest.mark.parametrize('cls,dil0', [('EcapaTdnn', 1), ('EcapaTdnn', 2), ('TDNN', 1)], ids=['ecapa-window', 'ecapa-per-tap', 'tdnn'])
def test_gpu_201_gives_the_bits_of_the_zero_padded_208(cls, dil0):
    from mvector import _hip
    if cls == 'EcapaTdnn':
        kw = lambda F: dict(input_size=F, channels=[64, 64, 64, 64, 192], dilations=[dil0, 2, 3, 4, 1])
        kind, wname = 'ecapa', 'blocks.0.conv.conv.weight'
    else:
        kw = lambda F: dict(input_size=F, embd_dim=192)
        kind, wname = 'tdnn', 'td_layer1.weight'
    m201, sd = _model(cls, kw(201))
    m208, _ = _model(cls, kw(208))
    sd208 = dict(sd)
    w = sd[wname]
    sd208[wname] = torch.cat([w, torch.zeros(w.shape[0], 7, w.shape[2])], dim=1)
    x = _feats(64, 300, 201, 7)
    x208 = torch.cat([x, torch.zeros(64, 300, 7, device=DEV)], dim=2)
    a = _hip.Model(kind, m201._native_cfg(), {k: v.to(DEV) for k, v in sd.items()}).forward(x)
    b = _hip.Model(kind, m208._native_cfg(), {k: v.to(DEV) for k, v in sd208.items()}).forward(x208)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_gpu_predictor_with_default_spectrogram(tmp_path):
    """MVectorPredictor on `feature_method: Spectrogram` with no method_args (201 bins) and the default EcapaTdnn, embedding on the GPU"""
    from mvector.models import EcapaTdnn
    from mvector.predict import MVectorPredictor
    shapes = weights.shapes_of(EcapaTdnn(input_size=201, embd_dim=192).state_dict())
    sd = weights.make_state_dict(shapes, 8)
    model_dir = tmp_path / 'model'
    model_dir.mkdir()
    torch.save({'0.' + k: v for k, v in sd.items()}, str(model_dir / 'model.pth'))
    cfg = dict(dataset_conf=dict(dataset=dict(min_duration=0.3, sample_rate=16000, use_dB_normalization=True, target_dB=-20),
                                 eval_conf=dict(batch_size=2)),
               preprocess_conf=dict(feature_method='Spectrogram'),
               model_conf=dict(model='EcapaTdnn', model_args=dict(embd_dim=192)))
    gpu = MVectorPredictor(cfg, model_path=str(model_dir), use_gpu=True)
    rng = np.random.default_rng(4)
    pcms = [(rng.standard_normal(n) * 3000 * (1 + i)).astype(np.int16) for i, n in enumerate((16000, 12000, 9000, 14500))]
    got = gpu.predict_batch([p.astype(np.float32) / 32768.0 for p in pcms])
    n = torch.tensor([len(p) for p in pcms])
    staged = torch.zeros(len(pcms), int(n.max()), dtype=torch.int16)
    for i, p in enumerate(pcms):
        staged[i, :len(p)] = torch.from_numpy(p)
    wav, _ = frontend.wave_prepare(staged, n, -20.0)
    want = omodels.ecapa_tdnn(sd, sr.featurize(wav, n.float() / int(n.max()), 'Spectrogram', {})).numpy()
    d = cos_dist(got, want).max()
    print(f'Spectrogram predictor: 1 - cos {d:.2e}')
    assert got.shape == (4, 192) and d < 1e-4
