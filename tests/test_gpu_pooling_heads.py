"""The SAP / TAP / TSP pooling heads on the MI355X: every golden of tools/make_pooling_golden.py (the reference's own modules) through the
pooled handles, bit-identical rows whatever the batch size, stream or graph replay, and MVectorPredictor / MVectorTrainer.evaluate on TDNN-TAP
and EcapaTdnn-SAP configs against the CPU path."""
import os

import numpy as np
import pytest
import torch

import pooling_ref as pr
from helpers import cos_dist, load_case
from oracle import frontend, weights

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')

HEADS = ['sap', 'tap', 'tsp']
GOLDENS = [f'tdnn_{p}' for p in HEADS] + [f'ecapa_{p}_tiny' for p in HEADS] + [f'ecapa_{p}_c1024' for p in HEADS]
KIND = {'TDNN': 'tdnn', 'EcapaTdnn': 'ecapa'}


def _module(man, sd):
    import mvector.models as M
    m = getattr(M, man['model'])(**man['kwargs'])
    m.load_state_dict(sd)
    return m.eval()


def _handle(man, sd):
    from mvector import _hip
    return _hip.Model(KIND[man['model']], _module(man, sd)._native_cfg(), {k: v.to(DEV) for k, v in sd.items()},
                      pooling_type=man['kwargs']['pooling_type'])


@pytest.mark.parametrize('case', GOLDENS)
def test_gpu_pooled_handle_matches_reference_golden(case):
    man, sd, x, emb, _ = load_case(case)
    got = _handle(man, sd).forward(x.to(DEV)).cpu()
    d = cos_dist(got, emb).max().item()
    print(f'{case}: 1 - cos {d:.2e}')
    assert d <= 1e-4, d


@pytest.mark.parametrize('pool', ['SAP', 'TAP'])
@pytest.mark.parametrize('cls', ['TDNN', 'EcapaTdnn'])
def test_gpu_module_forward_takes_the_native_head(cls, pool):
    """the module's own CUDA eval forward (no torch fallback there) on the newly enabled pairs, against the fp64 arbiter"""
    import mvector.models as M
    kw = dict(input_size=80) if cls == 'TDNN' else dict(input_size=80, channels=[512, 512, 512, 512, 1536])
    m = getattr(M, cls)(pooling_type=pool, **kw)
    sd = weights.make_state_dict(weights.shapes_of(m.state_dict()), 6)
    m.load_state_dict(sd)
    m.eval()
    x = torch.randn(4, 200, 80, generator=torch.Generator().manual_seed(2)) * 2
    want = pr.embed(m, sd, x)
    with torch.no_grad():
        got = m.to(DEV)(x.to(DEV)).cpu()
    d = cos_dist(got, want).max().item()
    print(f'{cls}-{pool} module forward: 1 - cos {d:.2e}')
    assert d <= 1e-4, d


def _feats(B, T, F, seed):
    return (torch.randn(B, T, F, generator=torch.Generator().manual_seed(seed)) * 2).to(DEV)


@pytest.mark.parametrize('case', ['tdnn_sap', 'tdnn_tap', 'tdnn_tsp', 'ecapa_sap_c1024', 'ecapa_tap_c1024', 'ecapa_tsp_c1024'])
def test_gpu_pooled_rows_do_not_depend_on_the_batch_size(case):
    man, sd, _, _, _ = load_case(case)
    h = _handle(man, sd)
    x = _feats(256, 298, 80, 4)
    full = h.forward(x)
    for nb in (1, 8, 40, 130):
        assert torch.equal(h.forward(x[:nb]), full[:nb]), nb
        assert torch.equal(h.forward(x[256 - nb:]), full[256 - nb:]), nb


@pytest.mark.parametrize('case', ['tdnn_sap', 'ecapa_tsp_tiny', 'ecapa_sap_tiny', 'tdnn_tsp'])
def test_gpu_pooled_handle_two_streams_and_graph_replay(case):
    man, sd, _, _, _ = load_case(case)
    h = _handle(man, sd)
    xa, xb = _feats(32, 300, 80, 11), _feats(48, 360, 80, 12)
    ea, eb = h.forward(xa).clone(), h.forward(xb).clone()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    bad = 0
    for _ in range(20):
        with torch.cuda.stream(s1):
            oa = h.forward(xa)
        with torch.cuda.stream(s2):
            ob = h.forward(xb)
        s1.synchronize()
        s2.synchronize()
        bad += int(not torch.equal(oa, ea)) + int(not torch.equal(ob, eb))
    assert bad == 0, bad
    static_x = xa.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        h.forward(static_x)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static_out = h.forward(static_x)
    xc = _feats(32, 300, 80, 13)
    ec = h.forward(xc).clone()
    for x, e in ((xc, ec), (xa, ea)):
        static_x.copy_(x)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out, e)


def test_gpu_tsp_at_one_frame_is_nan_like_torch_var():
    """TSP's unbiased variance of a single frame is 0 / 0 -- the device gives NaN where torch.var does"""
    from mvector import _hip
    x = torch.randn(3, 1, 512, generator=torch.Generator().manual_seed(1)).half().to(DEV)
    out = torch.empty(3, 1024, device=DEV)
    lib = _hip.lib()
    _hip.check(lib.mv_time_mean_var_f16(x.data_ptr(), 512, 3, 1, 512, out.data_ptr(), 1024, _hip.current_stream(x)), lib)
    torch.cuda.synchronize()
    assert torch.isnan(out[:, 512:]).all() and torch.equal(out[:, :512], x[:, 0].float())
    assert torch.isnan(torch.var(x[:, 0:1].float().transpose(1, 2), dim=2)).all()


# ------------------------------------------------------------------------------------------------ predictor / trainer

def _write_set(tmp_path, model, model_args, seed):
    """a checkpoint of `model` with seeded weights, 16-bit WAVs of three speakers, enrol / trial lists; -> (cfg, model_dir, wav paths)"""
    import scipy.io.wavfile as wavfile
    import mvector.models as M
    m = getattr(M, model)(input_size=80, **model_args)
    sd = weights.make_state_dict(weights.shapes_of(m.state_dict()), seed)
    model_dir = tmp_path / 'model'
    model_dir.mkdir()
    torch.save({'0.' + k: v for k, v in sd.items()}, str(model_dir / 'model.pth'))
    rng = np.random.default_rng(seed)
    lines = {'enroll': [], 'trials': []}
    paths = []
    for spk in range(3):
        base = frontend.synth_waveforms(1, 16000, seed=200 + spk)[0].numpy()
        for u in range(3):
            n = int(rng.integers(9000, 16000))
            xw = base[:n] + 0.02 * rng.standard_normal(n).astype(np.float32)
            pcm = np.clip(xw * 20000, -32768, 32767).astype(np.int16)
            path = str(tmp_path / f's{spk}_u{u}.wav')
            wavfile.write(path, 16000, pcm)
            paths.append(path)
            lines['enroll' if u == 0 else 'trials'].append(f'{path}\t{spk}\n')
    for k, v in lines.items():
        with open(str(tmp_path / f'{k}.txt'), 'w') as f:
            f.writelines(v)
    cfg = dict(dataset_conf=dict(dataset=dict(min_duration=0.3, sample_rate=16000, use_dB_normalization=True, target_dB=-20),
                                 eval_conf=dict(batch_size=4, max_duration=20), dataLoader=dict(num_workers=0),
                                 enroll_list=str(tmp_path / 'enroll.txt'), trials_list=str(tmp_path / 'trials.txt')),
               preprocess_conf=dict(feature_method='Fbank', method_args=dict(sample_frequency=16000, num_mel_bins=80)),
               model_conf=dict(model=model, model_args=dict(embd_dim=192, **model_args)))
    return cfg, str(model_dir), paths


PREDICTOR_CASES = [('TDNN', dict(pooling_type='TAP')), ('EcapaTdnn', dict(pooling_type='SAP'))]


@pytest.mark.parametrize('model,args', PREDICTOR_CASES, ids=['tdnn-tap', 'ecapa-sap'])
def test_gpu_predictor_and_evaluate_with_a_pooling_config(tmp_path, model, args):
    from mvector.predict import MVectorPredictor
    from mvector.trainer import MVectorTrainer
    cfg, model_dir, paths = _write_set(tmp_path, model, args, seed=7)
    gpu = MVectorPredictor(cfg, model_path=model_dir, use_gpu=True)
    e_gpu = gpu.predict_batch(paths)
    assert gpu._last_batch_path == 'pcm16'     # 16-bit mono WAVs at the target rate: int16 upload, scaled / normalised on the device
    cpu = MVectorPredictor(cfg, model_path=model_dir, use_gpu=False)
    e_cpu = cpu.predict_batch(paths)
    d = cos_dist(e_gpu, e_cpu).max().item()
    print(f'{model}-{args["pooling_type"]} predictor: GPU vs CPU 1 - cos {d:.2e}')
    assert e_gpu.shape == (len(paths), 192) and d < 1e-4, d
    eer_g, _, _ = MVectorTrainer(cfg, use_gpu=True).evaluate(resume_model=model_dir)
    eer_c, _, _ = MVectorTrainer(cfg, use_gpu=False).evaluate(resume_model=model_dir)
    print(f'{model}-{args["pooling_type"]} evaluate: EER GPU {eer_g:.4f} CPU {eer_c:.4f}')
    assert abs(eer_g - eer_c) < 1e-6, (eer_g, eer_c)
