"""EcapaTdnn with grouped TDNN convolutions and other SE-Res2Net block counts on the MI355X: every golden of tools/make_ecapa_variant_golden.py
(the reference's own module) through mv_ecapa_create_ex, the full-size grouped model on the grouped GEMM (no expanded 1x1 layer), rows
bit-identical whatever the batch size and under graph replay, the module's own CUDA forward, a predictor whose config sets `groups`, and the
grouped conv1d layer at full size on its native and expanded forms."""
import pytest
import torch

import ecapa_variant_checks as ev
from helpers import cos_dist, load_case

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _lib():
    from mvector import _hip
    return _hip.lib()


def _golden_handle(case):
    man, sd, x, emb, _ = load_case(case)
    return ev.handle(ev.golden_module(man, sd), sd, device=DEV), x, emb


@pytest.mark.parametrize('case', ev.GOLDENS)
def test_gpu_variant_golden(case):
    h, x, emb = _golden_handle(case)
    got = h.forward(x.to(DEV)).cpu()
    d = cos_dist(got, emb).max().item()
    print(f'{case}: 1 - cos {d:.2e}, info {ev.info(h)}')
    assert d <= 1e-4, d


def test_gpu_full_size_grouped_model_runs_no_expanded_1x1_layer():
    h, _, _ = _golden_handle('ecapa_grouped_c1024')
    native, expanded, expanded_1x1, blocks = ev.info(h)
    assert (native, expanded, expanded_1x1, blocks) == (7, 0, 0, 3)


def _feats(B, T, F, seed):
    return (torch.randn(B, T, F, generator=torch.Generator().manual_seed(seed)) * 2).to(DEV)


@pytest.mark.parametrize('case', ['ecapa_grouped_c1024', 'ecapa_blocks4_tiny', 'ecapa_grouped_tiny'])
def test_gpu_variant_rows_do_not_depend_on_the_batch_size(case):
    h, _, _ = _golden_handle(case)
    x = _feats(256, 298, 80, 4)
    full = h.forward(x)
    for nb in (1, 8, 40, 130):
        assert torch.equal(h.forward(x[:nb]), full[:nb]), nb
        assert torch.equal(h.forward(x[256 - nb:]), full[256 - nb:]), nb


@pytest.mark.parametrize('case', ['ecapa_grouped_c1024', 'ecapa_blocks1_tiny', 'ecapa_grouped_sap_tiny'])
def test_gpu_variant_graph_replay_is_bit_identical_to_eager(case):
    h, _, _ = _golden_handle(case)
    xa = _feats(32, 300, 80, 11)
    ea = h.forward(xa).clone()
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


@pytest.mark.parametrize('case', ['ecapa_grouped_c1024', 'ecapa_grouped_tiny', 'ecapa_blocks4_tiny'])
def test_gpu_module_cuda_eval_forward_gives_the_golden(case):
    """EcapaTdnn(groups=..., channels=...).cuda().eval() -- the module's own forward, which raised NotImplementedError before"""
    man, sd, x, emb, _ = load_case(case)
    m = ev.golden_module(man, sd).to(DEV)
    with torch.no_grad():
        got = m(x.to(DEV)).cpu()
    d = cos_dist(got, emb).max().item()
    assert d <= 1e-4, d


def test_gpu_predictor_with_groups_in_model_args(tmp_path):
    from mvector.predict import MVectorPredictor
    from test_gpu_pooling_heads import _write_set
    args = dict(channels=[256, 256, 256, 256, 768], groups=[1, 2, 2, 2, 2])
    cfg, model_dir, paths = _write_set(tmp_path, 'EcapaTdnn', args, seed=9)
    e_gpu = MVectorPredictor(cfg, model_path=model_dir, use_gpu=True).predict_batch(paths)
    e_cpu = MVectorPredictor(cfg, model_path=model_dir, use_gpu=False).predict_batch(paths)
    d = cos_dist(e_gpu, e_cpu).max().item()
    print(f'EcapaTdnn groups={args["groups"]} predictor: GPU vs CPU 1 - cos {d:.2e}')
    assert e_gpu.shape == (len(paths), 192) and d < 1e-4, d


GROUPED_CONV = [
    # B, T, cin, cout, g, k, dil, tile
    (64, 298, 1024, 1024, 2, 1, 1, 0),     # ring kernel, 512 per group
    (64, 298, 1024, 1024, 4, 1, 1, 0),     # ring kernel, 256 per group
    (64, 298, 1024, 1024, 8, 1, 1, 0),     # 128 per group: one-shot 128-channel tiles
    (32, 298, 3072, 3072, 4, 1, 1, 0),     # the MFA of [1, 4, 4, 4, 4]
    (64, 280, 1024, 1024, 2, 1, 1, 0),     # 280 tiles on 256 workgroups: the ring walk's last 24 tiles as 128 x 128 quarters
    (64, 298, 512, 512, 4, 1, 1, 0),       # EcapaTdnn-512 at g = 4
    (3, 298, 1024, 1024, 4, 1, 1, 0),      # a small batch (64 x 64 tiles)
    (16, 298, 1024, 1024, 16, 1, 1, 0),    # expanded (64 per group)
    (16, 298, 1024, 1024, 4, 3, 2, 0),     # expanded (k = 3)
]


@pytest.mark.parametrize('case', GROUPED_CONV, ids=[f'B{c[0]}T{c[1]}_{c[2]}to{c[3]}_g{c[4]}_k{c[5]}' for c in GROUPED_CONV])
def test_gpu_grouped_conv1d_matches_torch(case):
    B, T, cin, cout, g, k, dil, tile = case
    native = ev.grouped_conv_case(_lib(), DEV, B, T, cin, cout, g, k, dil, tile, seed=sum(case), bound=k == 1 and cin // g <= 1024, log=print)
    assert native == (k == 1 and (cin // g) % 64 == 0 and (cout // g) % 128 == 0)
