"""EcapaTdnn with grouped TDNN convolutions and other SE-Res2Net block counts (mv_ecapa_create_ex) and the grouped conv1d layer
(mv_conv1d_forward_grouped) under the SIMT emulator: the reference's goldens (tools/make_ecapa_variant_golden.py), other group / block
combinations against the package's torch forward, the grouped layer against F.conv1d(groups=g) on its native and its expanded shapes, the
refusals, and the Python gate."""
import ctypes
import os

import pytest
import torch

import ecapa_variant_checks as ev
from emu_lib import emu_cdll
from helpers import cos_dist, load_case
from mvector import _hip

SLOW = pytest.mark.skipif(os.environ.get('MV_SLOW_EMU') != '1', reason='minutes under the emulator; set MV_SLOW_EMU=1 (covered on the GPU by '
                          'test_gpu_variant_golden)')


@pytest.mark.parametrize('case', [c for c in ev.GOLDENS if 'c1024' not in c] + [pytest.param(c, marks=SLOW) for c in ev.GOLDENS if 'c1024' in c])
def test_emu_variant_golden(case):
    man, sd, x, emb, _ = load_case(case)
    got = ev.handle(ev.golden_module(man, sd), sd, cdll=emu_cdll()).forward(x)
    d = cos_dist(got, emb).max().item()
    print(f'{case}: 1 - cos {d:.2e}')
    assert d < 1e-5, d


# (grouped layers on the grouped GEMM, expanded grouped layers, expanded 1x1 ones, SE-Res2Net blocks)
INFO = {'ecapa_grouped_tiny': (0, 8, 7, 3), 'ecapa_blocks4_tiny': (0, 0, 0, 4), 'ecapa_blocks1_tiny': (0, 0, 0, 1),
        'ecapa_grouped_sap_tiny': (0, 7, 7, 3), 'ecapa_grouped_c1024': (7, 0, 0, 3)}


@pytest.mark.parametrize('case', ev.GOLDENS)
def test_emu_variant_info_keys(case):
    """blocks.0 (k = 5) and the narrow groups of the tiny models are expanded; the full-size [1, 4, 4, 4, 4] model runs all seven grouped layers
    (tdnn1 / tdnn2 of three blocks, the MFA) on the grouped GEMM; MV_INFO_CAMPP_HEAD_F32 (key 1) stays an error on EcapaTdnn"""
    man, sd, _, _, _ = load_case(case)
    h = ev.handle(ev.golden_module(man, sd), sd, cdll=emu_cdll())
    assert ev.info(h) == INFO[case]
    with pytest.raises(RuntimeError, match='no such key'):
        h.info(1)


OTHER = [
    # groups of 128 channels: tdnn1 / tdnn2 on the grouped GEMM's 128-channel tiles, the MFA (384 per group) as well
    (dict(input_size=40, channels=[256, 256, 256, 256, 768], groups=[1, 2, 2, 2, 2], embd_dim=64), 30, (7, 0, 0, 3)),
    # groups of 256 channels: the ring kernel (the emulated chip has 8 CUs, so 256-wide tiles are chosen)
    (dict(input_size=40, channels=[512, 512, 512, 512, 1536], groups=[1, 2, 2, 2, 2], embd_dim=64, attention_channels=64), 40, (7, 0, 0, 3)),
    # one block, a grouped MFA with k = 3 (expanded) and a grouped blocks.0
    (dict(input_size=48, channels=[128, 128, 128], kernel_sizes=[3, 3, 3], dilations=[1, 2, 2], groups=[4, 2, 4, 1, 4]), 30, (0, 4, 2, 1)),
    # widths that change from block to block (shortcut convs), every layer grouped by 2
    (dict(input_size=48, channels=[64, 128, 64, 192], kernel_sizes=[5, 3, 3, 1], dilations=[1, 2, 3, 1], groups=[2, 4, 2, 2]), 30, (0, 6, 5, 2)),
    # seven blocks and a head other than ASP
    (dict(input_size=40, channels=[64] * 8 + [448], kernel_sizes=[5] + [3] * 7 + [1], dilations=[1] + [2] * 7 + [1], groups=[1] * 9,
          pooling_type='TAP'), 24, (0, 0, 0, 7)),
]


@pytest.mark.parametrize('idx', range(len(OTHER)))
def test_emu_other_groups_and_block_counts_match_torch(idx):
    kw, T, want_info = OTHER[idx]
    m, sd = ev.module_and_weights(kw, 30 + idx)
    ok, why = m._native_supported()
    assert ok, why
    x = torch.randn(3, T, kw['input_size'], generator=torch.Generator().manual_seed(idx)) * 2
    with torch.no_grad():
        ref = m(x)
    h = ev.handle(m, sd, cdll=emu_cdll())
    assert ev.info(h) == want_info
    got = h.forward(x)
    d = cos_dist(got, ref).max().item()
    assert d < 1e-5, d


GROUPED_CONV = [
    # B, T, cin, cout, g, k, dil, tile, persist_blocks                   native form
    (2, 37, 256, 256, 2, 1, 1, 0, 0),       # 128-channel groups: one-shot glds tiles
    (1, 50, 128, 256, 2, 1, 1, 0, 0),       # 64-wide K per group
    (2, 70, 512, 512, 2, 1, 1, 256, 0),     # 256-channel groups on the ring kernel (conv1d_ring_grouped_kernel)
    (2, 45, 1024, 1024, 4, 1, 1, 0, 0),     # g = 4 on the ring kernel, auto tile
    (5, 256, 1024, 512, 2, 1, 1, 256, 8),   # ring walk + its tail as 128 x 128 quarters (10 tiles on 8 workgroups)
    (2, 40, 1024, 1024, 8, 1, 1, 128, 0),   # g = 8 (128 per group) forced onto the 128-channel tiles
    # expanded: narrow groups, k > 1
    (2, 33, 64, 64, 2, 1, 1, 0, 0),
    (2, 33, 256, 256, 4, 1, 1, 0, 0),
    (2, 33, 128, 128, 2, 3, 2, 0, 0),
    (2, 33, 80, 64, 2, 5, 1, 0, 0),
]


@pytest.mark.parametrize('case', GROUPED_CONV, ids=[f'B{c[0]}T{c[1]}_{c[2]}to{c[3]}_g{c[4]}_k{c[5]}_tile{c[7]}' for c in GROUPED_CONV])
def test_emu_grouped_conv1d_matches_torch(case):
    B, T, cin, cout, g, k, dil, tile, pb = case
    native = ev.grouped_conv_case(emu_cdll(), 'cpu', B, T, cin, cout, g, k, dil, tile, pb, seed=sum(case), bound=k == 1 and cin // g <= 1024)
    assert native == (k == 1 and (cin // g) % 64 == 0 and (cout // g) % 128 == 0)


def test_grouped_conv1d_refusals():
    cdll = emu_cdll()
    assert cdll.mv_conv1d_grouped_packed_elems(256, 250, 1, 4) == -1
    assert cdll.mv_conv1d_grouped_packed_elems(256, 256, 1, 2) == cdll.mv_conv1d_packed_elems(256, 128, 1)   # per group
    assert cdll.mv_conv1d_grouped_packed_elems(64, 64, 1, 2) == cdll.mv_conv1d_packed_elems(64, 64, 1)       # block-diagonal
    x = torch.zeros(2, 10, 256, dtype=torch.float16)
    y = torch.zeros(2, 10, 256, dtype=torch.float16)
    p = torch.zeros(4, 256)
    w = torch.zeros(int(cdll.mv_conv1d_packed_elems(256, 128, 1)), dtype=torch.float16)
    d = ev.desc(x, 256, w, p[0], p[1], p[2], y, 256, 2, 10, 256, 256)
    with pytest.raises(RuntimeError, match='divisible by groups'):
        _hip.check(cdll.mv_conv1d_forward_grouped(ctypes.byref(d), 3, None), cdll)
    with pytest.raises(RuntimeError, match='groups must be positive'):
        _hip.check(cdll.mv_conv1d_forward_grouped(ctypes.byref(d), 0, None), cdll)
    d.x2, d.ldx2 = x.data_ptr(), 256
    with pytest.raises(RuntimeError, match='grouped layer takes fp16 x without a second input'):
        _hip.check(cdll.mv_conv1d_forward_grouped(ctypes.byref(d), 2, None), cdll)
    d.x2, d.ldx, d.cin = None, 128, 256
    with pytest.raises(RuntimeError, match='ldx >= cin'):
        _hip.check(cdll.mv_conv1d_forward_grouped(ctypes.byref(d), 2, None), cdll)
    with pytest.raises(RuntimeError, match='divisible by groups'):
        _hip.check(cdll.mv_conv1d_pack_weight_grouped(p.data_ptr(), 256, 250, 1, 4, w.data_ptr(), None), cdll)
    assert torch.count_nonzero(y) == 0


def _cfg_ex(m):
    cfg = m._native_cfg()
    assert isinstance(cfg, _hip.MvEcapaCfgEx)
    return cfg


def _create(cfg, sd):
    cdll = emu_cdll()
    refs = (_hip.MvTensorRef * len(sd))()
    keep = []
    for i, (k, v) in enumerate(sd.items()):
        t = v.float().contiguous()
        keep.append((k.encode(), t))
        refs[i].name, refs[i].data, refs[i].numel = keep[-1][0], t.data_ptr(), t.numel()
    h = ctypes.c_void_p()
    rc = cdll.mv_ecapa_create_ex(ctypes.byref(cfg), _hip.MV_POOL_ASP, refs, len(sd), ctypes.byref(h))
    if rc == 0:
        cdll.mv_model_destroy(h)
    return rc, cdll.mv_last_error().decode()


def test_ecapa_ex_refusals_name_the_reason():
    m, sd = ev.module_and_weights(dict(input_size=80, channels=[64, 64, 64, 64, 192], groups=[2, 2, 2, 2, 2]), 1)
    cases = [
        (dict(nblocks=0), 'nblocks must be 1 .. 16'),
        (dict(nblocks=17), 'nblocks must be 1 .. 16'),
        (dict(channels={4: 200}), r'channels\[-1\] must equal the sum of the SE-Res2Net block widths \(200 != 192\)'),
        (dict(groups={2: 3}), r'block 2: channels\[1\] and channels\[2\] must be divisible by groups\[2\]'),
        (dict(groups={0: 3}), r'blocks.0: input_size and channels\[0\] must be divisible by groups\[0\]'),
        (dict(groups={4: 5}), r'mfa: channels\[-1\] must be divisible by groups\[-1\]'),
        (dict(groups={1: 0}), 'groups must be positive'),
    ]
    import re
    for change, msg in cases:
        cfg = _cfg_ex(m)
        for field, v in change.items():
            if isinstance(v, dict):
                for i, val in v.items():
                    getattr(cfg, field)[i] = val
            else:
                setattr(cfg, field, v)
        rc, err = _create(cfg, sd)
        assert rc != 0 and re.search(msg, err), (change, err)
    assert _create(_cfg_ex(m), sd)[0] == 0


def test_module_whose_mfa_width_is_not_the_block_sum_is_refused_by_the_library():
    """the reference itself cannot run it (torch.cat of the block outputs does not fit the MFA): the gate lets it through, the create call names it"""
    m, sd = ev.module_and_weights(dict(input_size=80, channels=[64, 64, 64, 64, 100]), 2)
    assert m._native_supported()[0]
    with pytest.raises(RuntimeError, match=r'channels\[-1\] must equal the sum'):
        ev.handle(m, sd, cdll=emu_cdll())


@pytest.mark.parametrize('kw', [dict(groups=[2, 2, 2, 2, 2]), dict(groups=[1, 4, 4, 4, 4], channels=[256, 256, 256, 256, 768]),
                                dict(channels=[64] * 6 + [320], kernel_sizes=[5, 3, 3, 3, 3, 3, 1], dilations=[1, 2, 3, 4, 5, 6, 1],
                                     groups=[1] * 7),
                                dict(channels=[64, 64, 64], kernel_sizes=[5, 3, 1], dilations=[1, 2, 1]),
                                dict(groups=[1, 2, 2, 2, 2], pooling_type='SAP')],
                         ids=['grouped', 'grouped-256', 'five-blocks', 'one-block', 'grouped-sap'])
def test_native_supported_for_groups_and_block_counts(kw):
    import mvector.models as M
    kw = dict(dict(input_size=80, channels=[64, 64, 64, 64, 192]), **kw)
    m = M.EcapaTdnn(**kw)
    ok, why = m._native_supported()
    assert ok, why
    cfg = m._native_cfg()
    n = len(kw['channels']) - 2
    assert isinstance(cfg, _hip.MvEcapaCfgEx) and cfg.nblocks == n
    g = kw.get('groups', [1] * 5)
    assert list(cfg.groups[:n + 2]) == [g[i] for i in range(n + 1)] + [g[-1]]   # by position, the MFA takes groups[-1]


def test_native_cfg_of_the_block_default_model_is_unchanged():
    import mvector.models as M
    assert type(M.EcapaTdnn(input_size=80, channels=[64, 64, 64, 64, 192])._native_cfg()) is _hip.MvEcapaCfg


def test_gates_that_stay_closed_keep_their_text():
    import mvector.models as M
    ok, why = M.EcapaTdnn(input_size=80, channels=[64, 64, 64, 64, 192], groups=[2, 2, 2, 2, 2], pooling_type='TSP')._native_supported()
    assert not ok and 'pooling_type' in why and 'TSP' in why
    ok, why = M.EcapaTdnn(input_size=80, channels=[64, 64, 64, 64, 192], groups=[2, 2, 2, 2, 2], activation=torch.nn.Tanh)._native_supported()
    assert not ok and why == 'a non-ReLU activation'
