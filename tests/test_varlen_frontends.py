"""Variable-length batches of the MelSpectrogram / Spectrogram / MFCC front-ends (mv_melspec_ / mv_spectrogram_ / mv_mfcc_forward_varlen)
on the emulator build of the kernels: every row against the second implementation on the row alone, bit identity with the handle's own
[1, n_b] forward, the per-row MFCC floor, the untouched ratio form, plumbing and refused arguments.  The checks themselves are in
tests/varlen_checks.py, shared with the device suite."""
import os
import re

import pytest
import torch

import varlen_checks as vc
from conftest import ROOT
from emu_lib import emu_cdll
from mvector import _hip

NEW_SYMBOLS = ('mv_melspec_forward_varlen', 'mv_spectrogram_forward_varlen', 'mv_mfcc_forward_varlen')


@pytest.mark.parametrize('idx', range(len(vc.CASES)), ids=vc.CASE_IDS)
def test_emu_rows_match_the_second_implementation(idx):
    vc.oracle_rows_case(emu_cdll(), 'cpu', idx)


@pytest.mark.parametrize('idx', range(len(vc.CASES)), ids=vc.CASE_IDS)
def test_emu_rows_the_reference_cannot_featurise_are_zero(idx):
    """+ a row of n_fft / 2 samples (torch.stft's reflect padding raises) and an empty row: all zero, the other rows as before"""
    vc.oracle_rows_case(emu_cdll(), 'cpu', idx, vc.LENS_SHORT)


@pytest.mark.parametrize('idx', range(len(vc.CASES)), ids=vc.CASE_IDS)
def test_emu_row_bits_are_those_of_the_row_alone(idx):
    vc.bit_identity_case(emu_cdll(), 'cpu', idx)


def test_emu_mfcc_floor_is_the_rows_own():
    vc.mfcc_floor_case(emu_cdll(), 'cpu')


# ---- plumbing ----

@pytest.mark.parametrize('method', sorted(vc.HANDLES))
def test_handles_take_num_samples(method):
    h = vc.make_handle(emu_cdll(), method, {})
    padded, _, n = vc.batch()
    out = h(padded, None, n)
    assert out.shape == h(padded).shape
    assert torch.equal(h(padded, num_samples=n), out)
    with pytest.raises(ValueError):
        h(padded, torch.ones(len(vc.LENS)), n)
    with pytest.raises(ValueError):
        h(padded, None, n[:3])


def test_symbols_declared_bound_and_exported():
    import shutil
    import subprocess
    import __graft_entry__
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mvector_hip.h')).read(), flags=re.S)
    lib = __graft_entry__.build()
    nm = shutil.which('nm') or '/opt/rocm/lib/llvm/bin/llvm-nm'
    exported = {line.split()[-1] for line in subprocess.run([nm, '-D', '--defined-only', lib], capture_output=True, text=True,
                                                             check=True).stdout.splitlines() if line.strip()}
    for s in NEW_SYMBOLS:
        assert re.search(r'\b' + s + r'\s*\(', text), s
        assert s in _hip.EXPORTED_SYMBOLS and s in exported, s
        assert hasattr(emu_cdll(), s), s


def test_cpu_featurizer_forward_varlen_keeps_the_per_row_loop():
    """CPU tensors: per-utterance featurisation, as before"""
    from mvector.data_utils.featurizer import AudioFeaturizer
    padded, wav, n = vc.batch()
    for method in ('MelSpectrogram', 'MFCC'):
        fz = AudioFeaturizer(method)
        out = fz.forward_varlen(padded, n)
        for b, nb in enumerate(vc.LENS):
            ref = fz(wav[b, :nb])[0]
            assert torch.equal(out[b, :ref.shape[0]], ref) and bool((out[b, ref.shape[0]:] == 0).all())


# ---- refused arguments ----

@pytest.mark.parametrize('method', sorted(vc.HANDLES))
def test_varlen_entry_points_refuse_bad_arguments(method):
    cd = emu_cdll()
    h = vc.make_handle(cd, method, dict(melkwargs=dict(n_fft=600)) if method == 'MFCC' else dict(n_fft=600))   # the dense DFT: needs its workspace
    prefix = {'MelSpectrogram': 'mv_melspec_', 'Spectrogram': 'mv_spectrogram_', 'MFCC': 'mv_mfcc_'}[method]
    fwd = getattr(cd, prefix + 'forward_varlen')
    padded, _, n = vc.batch()
    B = padded.shape[0]
    out = torch.zeros(B, h.num_frames(vc.L), 301)   # (wide enough for every method's rows)
    need = getattr(cd, prefix + 'workspace_bytes')(h._h, B, vc.L)
    assert need > 16
    ws = torch.zeros(need, dtype=torch.uint8)
    assert fwd(h._h, padded.data_ptr(), B, vc.L, vc.L, None, out.data_ptr(), ws.data_ptr(), need, None) != 0
    assert 'null length array' in cd.mv_last_error().decode()
    assert fwd(h._h, padded.data_ptr(), B, vc.L, vc.L, n.data_ptr(), out.data_ptr(), ws.data_ptr(), 16, None) != 0
    assert 'workspace' in cd.mv_last_error().decode()
    assert fwd(h._h, padded.data_ptr(), B, vc.L, vc.L - 1, n.data_ptr(), out.data_ptr(), ws.data_ptr(), need, None) != 0
    assert 'geometry' in cd.mv_last_error().decode()
    assert fwd(h._h, padded.data_ptr(), B, vc.L, vc.L, n.data_ptr(), None, ws.data_ptr(), need, None) != 0
    assert 'null buffer' in cd.mv_last_error().decode()
    assert fwd(h._h, padded.data_ptr(), B, vc.L, vc.L, n.data_ptr(), out.data_ptr(), ws.data_ptr(), need, None) == 0


@pytest.mark.parametrize('args,min_len,msg', [
    (dict(n_fft=64), 33, 'reflect padding needs more than n_fft/2 samples'),                 # the transform kernels reflect themselves
    (dict(n_fft=64, pad=3), 33, 'reflect padding needs more than n_fft/2 samples'),          # the extension pass; the 2 x 3 zeros count
    (dict(n_fft=64, pad_mode='circular'), 32, 'circular padding needs at least n_fft/2 samples'),
    (dict(n_fft=64, pad_mode='replicate'), 1, None), (dict(n_fft=64, pad_mode='constant'), 1, None)], ids=str)
def test_shortest_row_is_the_same_for_the_batch_form_and_the_variable_length_form(args, min_len, msg):
    """one frame rule on the host and on the device: the batch form refuses a call of min_len - 1 samples (pad counted) under reflect and
    circular padding and takes min_len; a row of the variable-length form has no frames below min_len and its own frames from there on"""
    h = _hip.Spectrogram(args, subtract_time_mean=False, cdll=emu_cdll())   # (no mean: the two frames of a wrapped-round row are equal)
    n = min_len - 2 * args.get('pad', 0)
    wav = vc.batch()[1][:2, :n + 5].contiguous()
    if msg is not None:
        with pytest.raises(RuntimeError, match=msg):
            h(wav[:, :n - 1])
    alone = h(wav[1:, :n])
    assert alone.shape[1] == h.num_frames(n) and bool((alone != 0).any())
    out = h(wav, None, torch.tensor([n - 1, n]))
    assert bool((out[0] == 0).all())
    assert torch.equal(out[1, :alone.shape[1]], alone[0]) and bool((out[1, alone.shape[1]:] == 0).all())
