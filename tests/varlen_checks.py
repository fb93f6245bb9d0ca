"""Variable-length form of the MelSpectrogram / Spectrogram / MFCC front-ends (mv_*_forward_varlen): the checks shared by the emulator
suite (tests/test_varlen_frontends.py) and the device suite (tests/test_gpu_varlen_frontends.py).

Row b of a variable-length call must be what the same handle makes of wav[b:b+1, :n_b] alone -- to the bar the batch form of the same
front-end is held to against the second implementation, and bit for bit against the handle's own [1, n_b] forward.  The second
implementations are evaluated once per geometry (on the CPU) and shared by every check that needs them."""
import functools

import torch

import spectral_ref as sr
from mvector import _hip
from oracle import frontend

L = 8000
# the full length; an odd length; a multiple of both hop lengths (200, 160: the last frame exists only through the padding); a length in the
# middle; one sample more than n_fft; n_fft / 2 + 1, the shortest row reflect padding allows at n_fft = 400
LENS = (8000, 7999, 6000, 5000, 401, 201)
LENS_SHORT = LENS + (200, 0)   # + a row reflect padding refuses at n_fft = 400, and an empty row
FILL = 0.37                    # behind every row's length: must never reach a result

# (method, arguments): one per code path
CASES = [
    ('MelSpectrogram', {}),                                       # melspec_tile_kernel, n_fft 400
    ('MelSpectrogram', dict(n_fft=512, hop_length=160)),          # melspec_pow2_kernel
    ('MelSpectrogram', dict(n_fft=600)),                          # dense DFT + GEMM + cmn_mask_kernel
    ('MelSpectrogram', dict(center=False)),                       # the row's own n_b without centre padding
    ('MelSpectrogram', dict(pad=11, pad_mode='constant')),        # melspec_extend_kernel in front
    ('MelSpectrogram', dict(pad=7, pad_mode='replicate')),        # the extension pass repeating the edge value at n_b
    ('Spectrogram', dict(pad_mode='circular', hop_length=160)),   # the extension pass wrapping round at n_b
    ('Spectrogram', {}),                                          # melspec_tile_kernel<spectrogram>
    ('Spectrogram', dict(n_fft=512)),                             # dense DFT + cmn_mask_kernel from the padded bin rows
    ('MFCC', {}),                                                 # per-row dB floor
    ('MFCC', dict(log_mels=True)),
    ('MFCC', dict(melkwargs=dict(n_fft=600))),
]
CASE_IDS = [f'{m}-{a}' for m, a in CASES]
HANDLES = {'MelSpectrogram': _hip.MelSpec, 'Spectrogram': _hip.Spectrogram, 'MFCC': _hip.Mfcc}


def make_handle(cdll, method, args):
    return HANDLES[method](args, cdll=cdll)


@functools.lru_cache(maxsize=None)
def batch(lens=LENS, seed=41):
    """(padded waveforms [B, L] with FILL behind every row's length, the clean waveforms, the lengths)"""
    wav = frontend.synth_waveforms(len(lens), L, seed=seed)
    padded = wav.clone()
    for b, n in enumerate(lens):
        padded[b, n:] = FILL
    return padded, wav, torch.tensor(lens, dtype=torch.int64)


def _stft_args(method, args):
    return dict(args.get('melkwargs') or {}) if method == 'MFCC' else args


def featurisable(method, args, n):
    """what the header promises: torch.stft takes the row (reflect: more than n_fft / 2 samples, circular: at least n_fft / 2, pad counted)
    and at least one frame fits"""
    a = _stft_args(method, args)
    n_fft, pad = a.get('n_fft', 400), a.get('pad', 0)
    lp = n + 2 * pad
    if n == 0:
        return False   # (nothing to featurise: whatever padding surrounds an empty row, its features are zero)
    if not a.get('center', True):
        return lp >= n_fft
    mode = a.get('pad_mode', 'reflect')
    return lp > n_fft // 2 if mode == 'reflect' else (lp >= n_fft // 2 if mode == 'circular' else lp > 0)


@functools.lru_cache(maxsize=None)
def _reference_rows(case_idx, lens):
    """per row: (second implementation on wav[b:b+1, :n_b] alone, its tolerance as an absolute bound), None for rows that cannot be featurised"""
    method, args = CASES[case_idx]
    _, wav, _ = batch(lens)
    out = []
    for b, n in enumerate(lens):
        if not featurisable(method, args, n):
            out.append(None)
            continue
        row = wav[b:b + 1, :n]
        if method == 'MelSpectrogram':      # layer_checks.melspec_case's bar
            ref = frontend.audio_featurizer(row, None, 'MelSpectrogram', args)[0]
            bound = 2e-4 * ref.abs().max().item() + 1e-6
        elif method == 'Spectrogram':       # test_spectral_frontends' / test_gpu_spectral_frontends' bar
            ref = sr.featurize(row, None, 'Spectrogram', args, torch.float64)[0]
            bound = 1e-4 * ref.abs().max().item() + 1e-6
        else:                               # test_gpu_spectral_frontends._mfcc_check's bar
            ref = sr.featurize(row, None, 'MFCC', args, torch.float64)[0]
            bound = 1e-2
        out.append((ref, bound))
    return out


def oracle_rows_case(cdll, device, case_idx, lens=LENS):
    """check 1: row b's first T_b frames against the second implementation on the row alone; frames t >= T_b exactly zero"""
    method, args = CASES[case_idx]
    h = make_handle(cdll, method, args)
    padded, _, n = batch(lens)
    out = h(padded.to(device), None, n.to(device)).cpu()
    assert out.shape[:2] == (len(lens), h.num_frames(L))
    worst = 0.0
    for b, ref in enumerate(_reference_rows(case_idx, lens)):
        if ref is None:
            assert bool((out[b] == 0).all()), (method, args, b)     # a row the reference cannot featurise: all zero, no fault
            continue
        ref, bound = ref
        Tb = h.num_frames(lens[b])
        assert ref.shape == (Tb, out.shape[2]), (ref.shape, Tb)
        err = (out[b, :Tb].double() - ref.double()).abs().max().item()
        print(f'{method} {args} row {b} (n = {lens[b]}, T_b = {Tb}): max|err| {err:.3e}, bound {bound:.3e}')
        assert err <= bound, (method, args, b, err, bound)
        assert bool((out[b, Tb:] == 0).all()), (method, args, b)
        worst = max(worst, err / bound)
    return worst


def bit_identity_case(cdll, device, case_idx, lens=LENS):
    """check 3: a row's bits are those of the handle's own [1, n_b] forward, whatever batch the row sits in; check 4: the ratio form gives
    equal bits before and after a variable-length call on the same handle"""
    method, args = CASES[case_idx]
    h = make_handle(cdll, method, args)
    padded, _, n = batch(lens)
    padded, n = padded.to(device), n.to(device)
    ratio = torch.tensor([1.0, 0.83, 0.6, 0.5, 0.71, 0.9, 1.0, 0.4][:len(lens)], device=device)
    before = h(padded, ratio).clone()
    out = h(padded, None, n)
    assert torch.equal(h(padded, ratio), before), (method, args)            # handles own no mutable state
    for b, nb in enumerate(lens):
        if not featurisable(method, args, nb) or nb == 0:
            assert bool((out[b] == 0).all())
            continue
        alone = h(padded[b:b + 1, :nb])
        Tb = alone.shape[1]
        assert Tb == h.num_frames(nb)
        assert torch.equal(out[b, :Tb], alone[0]), (method, args, b, (out[b, :Tb] - alone[0]).abs().max().item())
        assert torch.equal(h(padded[b:b + 1], None, n[b:b + 1])[0], out[b]), (method, args, b)      # B = 1, same L
    for b in range(0, len(lens), 2):
        assert torch.equal(h(padded[b:b + 2], None, n[b:b + 2]), out[b:b + 2]), (method, args, b)   # B = 2


def mfcc_floor_case(cdll, device):
    """check 2: with log_mels=False the floor is (the row's own loudest value) - top_db"""
    lens = (8000, 6000)
    wav = frontend.synth_waveforms(2, L, seed=6)
    wav[0] *= 100.0    # loud row: its max dB is > 80 dB above much of the quiet row
    wav[1] *= 1e-3
    for b, nb in enumerate(lens):
        wav[b, nb:] = FILL * (100.0 if b == 0 else 1e-3)
    wav = wav.to(device)
    n = torch.tensor(lens, dtype=torch.int64, device=device)
    h = make_handle(cdll, 'MFCC', {})
    var = h(wav, None, n)
    alone = h(wav[1:, :lens[1]])
    Tb = alone.shape[1]
    assert torch.equal(var[1, :Tb], alone[0]) and bool((var[1, Tb:] == 0).all())
    ref = sr.featurize(wav[1:, :lens[1]].cpu(), None, 'MFCC', {}, torch.float64)[0]
    assert (var[1, :Tb].cpu().double() - ref).abs().max().item() <= 1e-2
    both = h(wav, n.float() / L)                      # the ratio form couples the rows: the quiet row sits on the loud row's floor
    diff = (var[1, :Tb] - both[1, :Tb]).abs().max().item()
    print(f'MFCC quiet row: variable-length vs ratio form max|diff| {diff:.2f}')
    assert diff > 1.0
