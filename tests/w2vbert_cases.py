"""Cases and bars shared by tests/test_w2vbert_frontend.py (CPU / emulator) and tests/test_gpu_w2vbert_frontend.py (device).

Tolerance on the feature tensor -- not invented: tests/w2vbert_ref.py in fp32 is the rounding model of the device path (the same rounding sites:
fp32 log-mel, fp32 normalisation, fp32 LayerNorm; other summation orders -- the kernels even sum the statistics and the time mean in fp64).  Its
distance from the fp64 arbiter was measured on every case's own input on the CPU (`python tests/w2vbert_cases.py` prints the tables); the bar of
a case is TWICE that, max-abs and mean-abs -- the rule and the headroom of tests/hf_cases.py, for the same reason.  MODEL_DISTANCE holds the
measured (max-abs, mean-abs); bars() doubles it.  The kernel-level cases use the same rule on the stage alone (STAGE_DISTANCE: the fp32 torch
evaluation of the stage on the same fp32 input against fp64).  The per-bin statistics are held tighter: within 1 ulp of the fp64 numpy value.

Inputs: seeded noise under a burst envelope (amplitude steps of >= 20 dB every 0.1 - 0.3 s; a row of at most 0.3 s steps down twice by 40 dB, L / 3 apart).
The per-bin standard deviation of the log-mel is then of order 1, so the normalisation does not amplify the log-mel stage's rounding:
check_bin_std() asserts >= 0.5 for every bin of every row that is not silent, on the length the row is featurised on."""
import math
import os

import numpy as np
import torch

import w2vbert_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIXTURES = ('hf_w2vbert_even', 'hf_w2vbert_odd')
CFG = dict(num_mel_bins=80, stride=2, sampling_rate=16000, layer_norm_eps=1e-5, feature_projection_input_dim=160, padding_value=0.0,
           padding_side='right', model_type='wav2vec2-bert')
VARLEN_LENS = [8000, 559, 560, 720, 5000, 8000]


def load_fixture(name):
    """(cfg dict, ln_weight, ln_bias, wav, the HF model's extract_features)"""
    import json
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    cfg = json.loads(bytes(z['config']).decode())
    return (cfg, torch.from_numpy(z['sd/feature_projection.layer_norm.weight']), torch.from_numpy(z['sd/feature_projection.layer_norm.bias']),
            torch.from_numpy(z['wav']), torch.from_numpy(z['extract_features']))


def burst_waveforms(B, L, seed):
    """[B, L] fp32: unit noise times an envelope that jumps by 20 or 40 dB between the levels 0.3 / 0.03 / 0.003 every 1600 .. 4800 samples"""
    g = torch.Generator().manual_seed(seed)
    wav = torch.randn(B, L, generator=g)
    for b in range(B):
        if L <= 4800:   # no longer than one segment can be: three steps down, L / 3 apart, so that the frames differ whatever the draw
            for k in range(3):
                wav[b, k * (L // 3):L if k == 2 else (k + 1) * (L // 3)] *= 0.3 * 100.0 ** -k   # (40 dB: a frame sees its louder neighbour through the window edge)
            continue
        level, pos = int(torch.randint(0, 3, (1,), generator=g)), 0
        while pos < L:
            n = int(torch.randint(1600, 4801, (1,), generator=g))
            wav[b, pos:pos + n] *= 0.3 * 10.0 ** -level
            level = (level + 1 + int(torch.randint(0, 2, (1,), generator=g))) % 3   # never the same level twice
            pos += n
    return wav.clamp(-1, 1).contiguous()


def layer_norm_tensors(seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(160, generator=g) + 0.5, torch.rand(160, generator=g) * 0.6 - 0.3


# name -> (B, L, lens_ratio, subtract_time_mean)
CASES = {
    'L560': (2, 560, None, True),            # 2 frames, 1 stacked row: minus its own time mean it is exactly 0
    'L560_nocmn': (2, 560, None, False),
    'L720': (2, 720, None, True),            # 3 frames: the zero half-frame
    'L8000_B3': (3, 8000, [1.0, 0.5, 0.8], True),   # 48 frames; row 2 zero-padded behind sample 5000
    'L16160_B2': (2, 16160, None, True),     # 99 frames, 50 stacked
    'L4000_B130': (130, 4000, None, True),   # more rows than one round of a small grid
    'silent_row': (2, 4000, None, True),     # row 1 all zeros
    'silent_row_nocmn': (2, 4000, None, False),
    'offset_view': (2, 2401, [1.0, 0.6], True),   # rows 2404 floats apart in a buffer, the view starts one float into it
}
SILENT = {'silent_row': (1,), 'silent_row_nocmn': (1,)}


def build(name):
    """(ln_w, ln_b, wav [B, L] fp32, lens_ratio tensor or None, subtract_time_mean)"""
    B, L, ratio, cmn = CASES[name]
    wav = burst_waveforms(B, L, seed=17 + L % 97)
    if name == 'L8000_B3':
        wav[2, 5000:] = 0.0
    for b in SILENT.get(name, ()):
        wav[b] = 0.0
    if name == 'offset_view':
        buf = torch.full((B * (L + 3) + 1,), float('nan'))
        view = buf[1:].view(B, L + 3)[:, :L]
        view.copy_(wav)
        wav = view
        assert wav.stride(0) == L + 3 and wav.storage_offset() == 1
    ln_w, ln_b = layer_norm_tensors()
    return ln_w, ln_b, wav, None if ratio is None else torch.tensor(ratio, dtype=torch.float32), cmn


def varlen_input():
    wav = torch.full((len(VARLEN_LENS), 8000), float('nan'))   # samples behind n_b are never read
    for b, n in enumerate(VARLEN_LENS):
        wav[b, :n] = burst_waveforms(1, n, seed=29 + b)[0]   # (the envelope of a row is drawn for the row's own length)
    return wav


def reference(name, dtype=torch.float64):
    ln_w, ln_b, wav, ratio, cmn = build(name)
    return ref.featurize(ln_w, ln_b, CFG, wav, ratio, dtype, cmn)


def varlen_reference(dtype=torch.float64):
    ln_w, ln_b = layer_norm_tensors()
    wav = torch.nan_to_num(varlen_input(), nan=0.0)   # (the per-row restatement slices the rows anyway)
    return ref.featurize_varlen(ln_w, ln_b, CFG, wav, VARLEN_LENS, dtype, True)


def check_bin_std(name):
    """every bin's standard deviation over the frames the row is normalised over, >= 0.5 on every row that is not silent; returns the smallest"""
    if name == 'varlen':
        wav, rows = torch.nan_to_num(varlen_input(), nan=0.0), [(b, n) for b, n in enumerate(VARLEN_LENS) if n >= ref.MIN_SAMPLES]
    else:
        wav = build(name)[2]
        rows = [(b, wav.shape[1]) for b in range(wav.shape[0]) if b not in SILENT.get(name, ())]
    worst = math.inf
    for b, n in rows[:8]:   # (the rows of the B = 130 case are drawn alike: eight stand for them)
        mel = ref.log_mel(wav[b:b + 1, :n], torch.float64)
        worst = min(worst, ref.bin_stats(mel)[1].sqrt().min().item())
    assert worst >= 0.5, f'{name}: a log-mel bin with std {worst:.3f} over time'
    return worst


# ---- the kernel-level inputs: the stage's own fp32 input, the same for the fp32 evaluation, the arbiter and the kernel

STAGE_L = 32000   # 198 frames: thirteen 16-frame tiles, a second round for the eight thread groups of the statistics kernel
STAGE_LENS = [32000, 16160, 559]   # the variable-length form of the stage: 198 / 99 / 0 frames


def stage_input():
    """fp32 log-mel [3, 198, 80] of burst rows (the fp32 restatement's: the kernels' stand-in)"""
    return ref.log_mel(burst_waveforms(3, STAGE_L, seed=41), torch.float32).contiguous()


def stage_stats_f64(mel, lens=None):
    """fp64 numpy mean and var(ddof = 1) over the row's frames, [B, 80] each; (0, 0) for a row without frames"""
    x = mel.numpy().astype(np.float64)
    mean, var = np.zeros((x.shape[0], 80)), np.zeros((x.shape[0], 80))
    for b in range(x.shape[0]):
        t = x.shape[1] if lens is None else ref.num_frames(lens[b]) if lens[b] >= ref.MIN_SAMPLES else 0
        if t >= 2:
            mean[b], var[b] = x[b, :t].mean(0), x[b, :t].var(0, ddof=1)
    return mean, var


def stage_rows(mel, mean, var, dtype, lens=None):
    """the row pass alone in `dtype` on fp32 inputs: [B, ceil(T / 2), 160]; a row of the variable-length form keeps its own frames, zeros behind"""
    ln_w, ln_b = layer_norm_tensors()
    B, T, _ = mel.shape
    out = torch.zeros(B, (T + 1) // 2, 160, dtype=dtype)
    for b in range(B):
        t = T if lens is None else ref.num_frames(lens[b]) if lens[b] >= ref.MIN_SAMPLES else 0
        if t:
            r = ref.rows(mel[b:b + 1, :t].to(dtype), mean[b:b + 1].to(dtype), var[b:b + 1].to(dtype), ln_w, ln_b, CFG['layer_norm_eps'])
            out[b, :r.shape[1]] = r[0]
    return out


# measured on the CPU: fp32 restatement vs the fp64 arbiter, (max-abs, mean-abs) over the featurizer output of the case
MODEL_DISTANCE = {
    'L560': (0.000e+00, 0.000e+00),   # smallest bin std 3.20; |ref| max 0.00 (one stacked row minus its own mean)
    'L560_nocmn': (5.076e-07, 1.208e-07),   # smallest bin std 3.20; |ref| max 1.75
    'L720': (5.383e-06, 4.717e-07),   # smallest bin std 3.53; |ref| max 1.94
    'L8000_B3': (1.937e-04, 3.233e-06),   # smallest bin std 3.72; |ref| max 7.61
    'L16160_B2': (1.939e-04, 3.414e-06),   # smallest bin std 3.46; |ref| max 6.46
    'L4000_B130': (3.398e-04, 3.035e-06),   # smallest bin std 6.67; |ref| max 9.28
    'silent_row': (3.025e-05, 2.969e-06),   # smallest bin std 6.83; |ref| max 4.36 (row 0 alone; the silent row is held to exact values)
    'silent_row_nocmn': (3.140e-05, 3.054e-06),   # smallest bin std 6.83; |ref| max 5.03 (row 0 alone)
    'offset_view': (3.333e-05, 2.122e-06),   # smallest bin std 6.70; |ref| max 4.58
    'varlen': (1.419e-04, 1.495e-06),   # smallest bin std 1.60; |ref| max 6.43
}

# the row pass alone (fp32 torch vs fp64 on the same fp32 log-mel and statistics): batch form, variable-length form
STAGE_DISTANCE = {
    'rows': (2.097e-06, 2.002e-07),
    'rows_varlen': (1.676e-06, 9.487e-08),
}


def bars(name):
    mx, mean = MODEL_DISTANCE[name]
    return 2.0 * mx, 2.0 * mean


def stage_bars(name):
    mx, mean = STAGE_DISTANCE[name]
    return 2.0 * mx, 2.0 * mean


def distances(got, ref64, name=None):
    """(max-abs, mean-abs); over the rows that are not silent when the case has a silent row (that one is held to exact values instead: the fp32
    restatement's own noise on a constant log-mel -- x - mean of order 1e-7 against sqrt(1e-7) -- would make its bar meaningless)"""
    keep = [b for b in range(ref64.shape[0]) if b not in SILENT.get(name, ())]
    d = (got.double().cpu() - ref64).abs()[keep]
    return d.max().item(), d.mean().item()


# ---- running a case on a library (the emulator build on the CPU, the product on the device)

def handle(cdll=None, cmn=True, device=None):
    from mvector import _hip
    ln_w, ln_b = layer_norm_tensors()
    sd = {'feature_projection.layer_norm.weight': ln_w, 'feature_projection.layer_norm.bias': ln_b}
    return _hip.W2vBert(CFG, sd, device=device, subtract_time_mean=cmn, cdll=cdll)


def forward_prefilled(h, wav, lens_ratio=None, num_samples=None):
    """the handle's forward on an output and a workspace that hold 0xFF bytes (NaNs): what they held must not reach a result"""
    import ctypes
    from mvector import _hip
    B, L = wav.shape
    out = torch.full((B, h.num_frames(L), 160), float('nan'), device=wav.device).view(torch.uint8).fill_(0xFF).view(torch.float32)
    need = ctypes.c_size_t()
    _hip.check(h._cdll.mv_w2vbert_workspace_bytes(h._h, B, L, ctypes.byref(need)), h._cdll)
    ws = torch.full((max(need.value, 16),), 0xFF, dtype=torch.uint8, device=wav.device)
    lens = lens_ratio if num_samples is None else torch.as_tensor(num_samples, dtype=torch.int64).to(wav.device)
    if lens is not None:
        lens = lens.to(wav.device).contiguous()
    fn = h._cdll.mv_w2vbert_forward if num_samples is None else h._cdll.mv_w2vbert_forward_varlen
    _hip.check(fn(h._h, wav.data_ptr(), B, L, wav.stride(0), None if lens is None else lens.data_ptr(), out.data_ptr(), ws.data_ptr(), need.value,
                  _hip.current_stream(wav)), h._cdll)
    return out


def run(name, cdll=None, device=None):
    """(features of the case from the library, fp64 reference)"""
    ln_w, ln_b, wav, ratio, cmn = build(name)
    h = handle(cdll, cmn, device)
    if device is not None:
        if name == 'offset_view':   # the same view on the device: one float into its buffer, rows L + 3 apart
            B, L = wav.shape
            buf = torch.full((B * (L + 3) + 1,), float('nan'), device=device)
            dview = buf[1:].view(B, L + 3)[:, :L]
            dview.copy_(wav)
            wav = dview
        else:
            wav = wav.to(device)
    return forward_prefilled(h, wav, ratio), ref.featurize(ln_w, ln_b, CFG, build(name)[2], ratio, torch.float64, cmn)


def check_case(name, got, ref64):
    """the assertions every case makes on a result, on either machine; returns the line to print"""
    assert got.shape == ref64.shape and torch.isfinite(got).all()
    mx, mean = distances(got, ref64, name)
    bmx, bmean = bars(name)
    line = f'{name}: max-abs {mx:.3e} (bar {bmx:.3e}) mean-abs {mean:.3e} (bar {bmean:.3e})'
    assert mx <= bmx and mean <= bmean, line
    got = got.cpu()
    ratio, cmn = CASES[name][2], CASES[name][3]
    if ratio is not None:   # zero behind round(ratio * T2), exactly
        T2 = got.shape[1]
        for b, r in enumerate(ratio):
            n = int(torch.round(torch.tensor(r, dtype=torch.float32) * T2))
            assert n == T2 or got[b, n:].abs().max().item() == 0.0
            assert got[b, :n].abs().max().item() > 0.0
    for b in SILENT.get(name, ()):   # constant log-mel: z = 0, so LayerNorm gives its bias exactly -- and minus its own time mean exactly 0
        want = torch.zeros(160) if cmn else layer_norm_tensors()[1]
        assert torch.equal(got[b], want.expand_as(got[b]))
    if name == 'L560':
        assert got.abs().max().item() == 0.0
    return line


if __name__ == '__main__':
    print('MODEL_DISTANCE = {')
    for name in list(CASES) + ['varlen']:
        r64 = varlen_reference() if name == 'varlen' else reference(name)
        r32 = varlen_reference(torch.float32) if name == 'varlen' else reference(name, torch.float32)
        mx, mean = distances(r32, r64, name)
        print(f"    '{name}': ({mx:.3e}, {mean:.3e}),   # smallest bin std {check_bin_std(name):.2f}; |ref| max {r64.abs().max():.2f}")
    print('}\nSTAGE_DISTANCE = {')
    mel = stage_input()
    for name, lens in (('rows', None), ('rows_varlen', STAGE_LENS)):
        mean, var = (torch.from_numpy(a).float() for a in stage_stats_f64(mel, lens))
        mx, mn = distances(stage_rows(mel, mean, var, torch.float32, lens), stage_rows(mel, mean, var, torch.float64, lens))
        print(f"    '{name}': ({mx:.3e}, {mn:.3e}),")
    print('}')
