"""Cases, seeded inputs and bars of the CAM++ dense-layer checks: tests/test_cam_dense.py (CPU: the bars can see the bugs they are for; emulator)
and tests/test_gpu_cam_dense.py (device).  One case = one launch of mv_cam_dense_block_f16 with the launch form pinned (or form 0 and the
expected choice), compared LAYER BY LAYER with tests/cam_ref.py in fp64 on the device's own input channels (teacher forcing).

Bars -- the convention of tests/hf_cases.py: cam_ref.py carries the rounding model of each form (fp32 with a round to fp16 exactly where the kernels
store or feed fp16).  Its distance from the fp64 arbiter is measured on the CPU on the case's own seeded input, with the model's own chain as the
layer inputs, max-abs and mean-abs over all layers' new channels (`python tests/cam_cases.py` reprints the table); the bar of a case is TWICE that:
the summation order inside the MFMA, `expf` and the DPP sums differ from torch's.  Nothing here comes from device output.

Inputs are drawn at test time from the case's name (never committed): x is O(1); BatchNorm gains around 1 with shifts that leave about half of the
ReLU inputs negative; the context FCs are scaled so that the gates spread over (0.1, 0.9) and differ between segments (asserted on the reference:
a gate near 0.5 everywhere hides gate bugs)."""
import os
import re
import zlib

import torch

import cam_ref

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'voiceprintrecognition-pytorch_amd', 'csrc')
G, BN = 32, 128


def source_constant(name, path='camdense.hip'):
    """an integer `constexpr int NAME = value;` of the kernel source: the cases sit ON the limits the predicates test"""
    with open(os.path.join(CSRC, path)) as f:
        return int(re.search(r'constexpr int %s = (\d+);' % name, f.read()).group(1))


CD_MAX_CIN = source_constant('CD_MAX_CIN')
CD_PAD = source_constant('CD_PAD')
LAYER_MAX_CIN = CD_MAX_CIN - 64     # cam_dense_layer_supported: cin <= CD_MAX_CIN - 64


def _case(form, T2, c_in, nlayers, dil=1, seg_len=100, B=3, pad=0, expect=None):
    return dict(form=form, T2=T2, c_in=c_in, nlayers=nlayers, dil=dil, seg_len=seg_len, B=B, pad=pad, expect=expect)


CASES = {}
# ---- block kernel (form 1): T2 on the 16-row tile edge, the 100-frame segment edge, the 160-frame limit; every other case with 8 pitch columns ----
for _i, (_dil, _T2) in enumerate((d, t) for d in (1, 2) for t in (1, 2, 3, 15, 16, 17, 100, 101, 159, 160)):
    CASES[f'block_T{_T2}_d{_dil}'] = _case(1, _T2, 128, 2, _dil, pad=8 * ((_i + _i // 10) % 2))
CASES.update({
    'block_T33_seg20': _case(1, 33, 128, 2, 1, seg_len=20, pad=8),         # ragged second segment of 13 frames
    'block_1layer': _case(1, 37, 128, 1, 2),                               # nothing is prefetched
    'block_24layers_c224': _case(1, 37, 224, 24, 2, pad=8),                # cin not a multiple of 64 on every other layer, last cin 960; waves with 1 / 0 stores at the counted entry
    'block_c960_3layers': _case(1, 101, 960, 3, 2),                        # cin reaches CB_MAX_CIN = 1024, c_out = 1056; two segments
    'block_c128_12layers': _case(1, 150, 128, 12, 1, pad=8),               # block 1 of the default model; waves with 3 / 2 stores at the counted entry
    'block_B1': _case(1, 45, 128, 2, 1, B=1, pad=8),
    'block_B300': _case(1, 40, 128, 2, 2, B=300),                          # more workgroups than compute units
})
# ---- per-layer kernel (form 2) ----
for _cin in (32, 64, 96, 448, LAYER_MAX_CIN):
    CASES[f'layer_c{_cin}'] = _case(2, 37, _cin, 1, 1, pad=8 if _cin in (64, 448) else 0)
for _T2 in (1, 17, 101, 160):
    CASES[f'layer_T{_T2}'] = _case(2, _T2, 96, 2, 2, pad=8 if _T2 in (17, 160) else 0)
for _dil in range(1, CD_PAD + 1):
    for _T2 in (3, 160):
        CASES[f'layer_d{_dil}_T{_T2}'] = _case(2, _T2, 64, 2, _dil, pad=8 if _T2 == 3 else 0)
# ---- two-launch long form (form 3): T2 on the chunk edge (161, 320, 321), seg_len at the predicate's limit (a chunk touches three segments) ----
CASES.update({
    'long_T161_c32_d1_s100_B1': _case(3, 161, 32, 2, 1, 100, B=1),
    'long_T161_c480_d2_s80_B5': _case(3, 161, 480, 1, 2, 80, B=5, pad=8),
    'long_T200_c480_d2_s80_B5': _case(3, 200, 480, 2, 2, 80, B=5),
    'long_T200_c32_d1_s100_B1': _case(3, 200, 32, 1, 1, 100, B=1, pad=8),
    'long_T320_c32_d2_s100_B5': _case(3, 320, 32, 2, 2, 100, B=5, pad=8),
    'long_T321_c480_d1_s80_B1': _case(3, 321, 480, 1, 1, 80, B=1),
    'long_T372_c32_d1_s80_B5': _case(3, 372, 32, 2, 1, 80, B=5),
    'long_T372_c480_d2_s100_B1': _case(3, 372, 480, 1, 2, 100, B=1, pad=8),
    'long_T401_c480_d2_s100_B1': _case(3, 401, 480, 2, 2, 100, B=1, pad=8),
    'long_T401_c32_d1_s80_B5': _case(3, 401, 32, 1, 1, 80, B=5),
})
# ---- form 0: one geometry per branch of the forward's choice, with the branch it has to take ----
CASES.update({
    'auto_block': _case(0, 50, 128, 2, 1, expect=1, pad=8),
    'auto_layer': _case(0, 50, 64, 3, 2, expect=2),                        # c_in < 128: block 1 of init_channels = 64
    'auto_long': _case(0, 170, 128, 2, 2, expect=3, pad=8),
})
# ---- emulator (every lane runs as a fiber: B = 1) ----
CASES.update({
    'emu_block_T17': _case(1, 17, 128, 2, 1, B=1, pad=8),
    'emu_block_T33_seg20': _case(1, 33, 128, 2, 2, seg_len=20, B=1),
    'emu_layer_c96_T17': _case(2, 17, 96, 1, 2, B=1, pad=8),
    'emu_long_T161_c32': _case(3, 161, 32, 1, 1, B=1),
})
EMU_CASES = tuple(n for n in CASES if n.startswith('emu_'))
GPU_CASES = tuple(n for n in CASES if not n.startswith('emu_'))

# a pinned form just outside its predicate: (form, T2, c_in, nlayers, dil, seg_len)
REFUSALS = {
    'block_T161': (1, 161, 128, 2, 1, 100),
    'block_c96': (1, 40, 96, 2, 1, 100),
    'layer_T161': (2, 161, 96, 1, 1, 100),
    'long_T160': (3, 160, 32, 1, 1, 100),
    'long_seg79': (3, 200, 32, 1, 1, 79),
}


def run_form(case):
    """the form a case's layers run (a form-0 case: the branch it expects)"""
    return case['form'] or case['expect']


def build(name):
    """(x0 [B, T2, c_in] fp16, layers: list of dicts of fp32 tensors with w1 / wl holding fp16 values)"""
    c = CASES[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    rn = lambda *s: torch.randn(*s, generator=g)
    x0 = rn(c['B'], c['T2'], c['c_in']).half()
    layers = []
    for l in range(c['nlayers']):
        cin = c['c_in'] + G * l
        layers.append(dict(
            w1=(rn(BN, cin) * (2.0 / cin) ** 0.5).half().float(),
            bn1_s=1.0 + 0.1 * rn(cin), bn1_t=0.3 * rn(cin),
            bn2_s=1.0 + 0.1 * rn(BN), bn2_t=0.3 * rn(BN),
            wl=(rn(G, BN, 3) * (2.0 / (3 * BN)) ** 0.5).half().float(),
            # context FCs: a wide first layer (its input, a sum of two means of ReLU outputs, moves little between segments), zero-sum rows so that
            # the common level of the context does not drive every unit the same way
            wa=_zero_sum_rows(rn(BN // 2, BN)) * 0.5, ba=0.2 * rn(BN // 2),
            wb=rn(G, BN // 2) * 0.04, bb=0.3 * rn(G)))
    return x0, layers


def _zero_sum_rows(w):
    return w - w.mean(1, keepdim=True)


def model_chain(name):
    c = CASES[name]
    x0, layers = build(name)
    return cam_ref.block_chain(x0, layers, c['dil'], c['seg_len'], cam_ref.CTX_FROM[run_form(c)]), layers


def new_channels(xfull, c):
    return xfull[..., c['c_in']:c['c_in'] + G * c['nlayers']]


def distances(got, ref64):
    d = (got.double() - ref64).abs()
    return d.max().item(), d.mean().item()


def model_distance(name):
    """the rounding model's chain against the fp64 arbiter applied to that chain's own layer inputs"""
    c = CASES[name]
    chain, layers = model_chain(name)
    ref = cam_ref.teacher_forced(chain, c['c_in'], layers, c['dil'], c['seg_len'])
    return distances(new_channels(chain, c), ref), ref.abs().max().item()


def check_gate_spread(gates, name):
    """the reference's gates spread over (0.1, 0.9) and differ between the segments"""
    g = torch.stack([t.reshape(-1, t.shape[1], G) for t in gates])     # [layers, B, nseg, 32]
    inside = ((g > 0.1) & (g < 0.9)).float().mean().item()
    assert g.min().item() < 0.3 and g.max().item() > 0.7 and inside > 0.6, (name, g.min().item(), g.max().item(), inside)
    if g.shape[2] > 1:
        gap = (g[:, :, 0] - g[:, :, -1]).abs()
        assert gap.mean().item() > 0.01 and gap.max().item() > 0.04, (name, gap.mean().item(), gap.max().item())


def bars(name):
    mx, mean = MODEL_DISTANCE[name]
    return 2.0 * mx, 2.0 * mean


def edges(name):
    """the deliberately wrong references (cam_ref.WRONG + 'stale_tile') that differ from the true layer at this case's shape -- every one of them must
    lie outside the case's bars (tests/test_cam_dense.py)"""
    c = CASES[name]
    T2, seg = c['T2'], c['seg_len']
    out = ['tap_plus', 'tap_minus']
    if T2 % seg:
        out.append('last_seg_len')
    if T2 > seg:
        out.append('gate_seg0')
    if abs(T2 - 160) >= 32:          # (a time mean over 160 rows instead of 159 or 161 is within a layer's rounding: no bar sees it)
        out.append('time_mean_160')
    if c['nlayers'] >= 2:
        out.append('stale_tile')
    return out


def wrong_reference(name, chain, layers, which):
    c = CASES[name]
    if which == 'stale_tile':   # the last layer reads the tile that holds the utterance's last row before its predecessor wrote it
        return cam_ref.teacher_forced(chain, c['c_in'], layers, c['dil'], c['seg_len'], stale=(c['nlayers'] - 1, (c['T2'] - 1) // 16 * 16))
    return cam_ref.teacher_forced(chain, c['c_in'], layers, c['dil'], c['seg_len'], wrong=which)


# measured on the CPU: rounding model (fp32 + fp16 sites) vs the fp64 arbiter, (max-abs, mean-abs) over all layers' new channels of the case
MODEL_DISTANCE = {
    'block_T1_d1': (5.461e-04, 8.256e-05),   # |ref| max 1.14
    'block_T2_d1': (7.075e-04, 1.170e-04),   # |ref| max 1.80
    'block_T3_d1': (1.023e-03, 1.240e-04),   # |ref| max 2.15
    'block_T15_d1': (1.151e-03, 1.521e-04),   # |ref| max 2.78
    'block_T16_d1': (1.250e-03, 1.375e-04),   # |ref| max 2.42
    'block_T17_d1': (1.012e-03, 1.337e-04),   # |ref| max 2.10
    'block_T100_d1': (1.392e-03, 1.500e-04),   # |ref| max 3.14
    'block_T101_d1': (1.586e-03, 1.462e-04),   # |ref| max 3.45
    'block_T159_d1': (1.256e-03, 1.418e-04),   # |ref| max 3.13
    'block_T160_d1': (1.620e-03, 1.394e-04),   # |ref| max 3.01
    'block_T1_d2': (9.189e-04, 1.082e-04),   # |ref| max 1.73
    'block_T2_d2': (5.291e-04, 8.630e-05),   # |ref| max 1.29
    'block_T3_d2': (1.172e-03, 1.233e-04),   # |ref| max 2.29
    'block_T15_d2': (1.145e-03, 1.427e-04),   # |ref| max 2.82
    'block_T16_d2': (1.392e-03, 1.678e-04),   # |ref| max 3.08
    'block_T17_d2': (1.273e-03, 1.396e-04),   # |ref| max 3.51
    'block_T100_d2': (1.356e-03, 1.550e-04),   # |ref| max 3.20
    'block_T101_d2': (1.295e-03, 1.412e-04),   # |ref| max 3.18
    'block_T159_d2': (1.462e-03, 1.464e-04),   # |ref| max 3.26
    'block_T160_d2': (1.723e-03, 1.542e-04),   # |ref| max 3.39
    'block_T33_seg20': (1.196e-03, 1.429e-04),   # |ref| max 2.61
    'block_1layer': (1.121e-03, 1.472e-04),   # |ref| max 2.35
    'block_24layers_c224': (1.348e-03, 1.203e-04),   # |ref| max 2.56
    'block_c960_3layers': (1.781e-03, 1.620e-04),   # |ref| max 3.66
    'block_c128_12layers': (1.564e-03, 1.254e-04),   # |ref| max 2.67
    'block_B1': (9.562e-04, 1.486e-04),   # |ref| max 2.26
    'block_B300': (1.692e-03, 1.410e-04),   # |ref| max 3.75
    'layer_c32': (1.702e-03, 1.333e-04),   # |ref| max 2.46
    'layer_c64': (1.091e-03, 1.391e-04),   # |ref| max 2.12
    'layer_c96': (1.420e-03, 1.595e-04),   # |ref| max 2.72
    'layer_c448': (9.249e-04, 1.195e-04),   # |ref| max 2.30
    'layer_c1984': (1.229e-03, 1.547e-04),   # |ref| max 2.59
    'layer_T1': (3.394e-04, 8.412e-05),   # |ref| max 1.37
    'layer_T17': (1.017e-03, 1.318e-04),   # |ref| max 2.12
    'layer_T101': (1.490e-03, 1.525e-04),   # |ref| max 3.08
    'layer_T160': (1.349e-03, 1.359e-04),   # |ref| max 2.78
    'layer_d1_T3': (6.880e-04, 1.297e-04),   # |ref| max 2.18
    'layer_d1_T160': (1.470e-03, 1.393e-04),   # |ref| max 3.57
    'layer_d2_T3': (1.020e-03, 1.303e-04),   # |ref| max 3.08
    'layer_d2_T160': (1.187e-03, 1.306e-04),   # |ref| max 2.66
    'long_T161_c32_d1_s100_B1': (1.346e-03, 1.501e-04),   # |ref| max 3.40
    'long_T161_c480_d2_s80_B5': (1.224e-03, 1.503e-04),   # |ref| max 3.17
    'long_T200_c480_d2_s80_B5': (1.493e-03, 1.609e-04),   # |ref| max 3.37
    'long_T200_c32_d1_s100_B1': (1.334e-03, 1.456e-04),   # |ref| max 3.80
    'long_T320_c32_d2_s100_B5': (1.795e-03, 1.362e-04),   # |ref| max 3.81
    'long_T321_c480_d1_s80_B1': (1.231e-03, 1.517e-04),   # |ref| max 2.83
    'long_T372_c32_d1_s80_B5': (1.944e-03, 1.369e-04),   # |ref| max 3.70
    'long_T372_c480_d2_s100_B1': (1.084e-03, 1.365e-04),   # |ref| max 2.50
    'long_T401_c480_d2_s100_B1': (1.342e-03, 1.377e-04),   # |ref| max 2.96
    'long_T401_c32_d1_s80_B5': (1.298e-03, 1.335e-04),   # |ref| max 3.20
    'auto_block': (1.404e-03, 1.393e-04),   # |ref| max 3.63
    'auto_layer': (1.429e-03, 1.489e-04),   # |ref| max 3.38
    'auto_long': (1.425e-03, 1.345e-04),   # |ref| max 2.70
    'emu_block_T17': (7.663e-04, 1.362e-04),   # |ref| max 2.18
    'emu_block_T33_seg20': (9.896e-04, 1.374e-04),   # |ref| max 2.25
    'emu_layer_c96_T17': (8.431e-04, 1.361e-04),   # |ref| max 2.27
    'emu_long_T161_c32': (1.381e-03, 1.468e-04),   # |ref| max 3.47
}


if __name__ == '__main__':
    for name in CASES:
        (mx, mean), top = model_distance(name)
        print(f"    '{name}': ({mx:.3e}, {mean:.3e}),   # |ref| max {top:.2f}")
