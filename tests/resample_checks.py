"""Checks of the down-mix + polyphase resampler (csrc/resample.hip) shared by tests/test_resample.py (the emulator build, CPU tensors) and
tests/test_gpu_resample.py (the product library on the device).  Each takes the bound library (None = the product library) and a device.

The bars are rounding bounds, not measured tolerances: the table within one fp32 ulp of scipy's, the down-mix bit-equal to the host mean, every
resampled sample within (K + 3) 2^-24 sum_j |x_j| |h| of scipy.signal.resample_poly in fp64 (K products and adds, the fp32 table, one ulp of
table slack)."""
import ctypes
import math

import numpy as np
import pytest
import torch

FILTER_RATES = ((44100, 16000), (48000, 16000), (8000, 16000), (22050, 16000), (11025, 16000), (16000, 8000))
RESAMPLE_CASES = ((44100, 16000, 2), (8000, 16000, 1), (48000, 16000, 1), (22050, 16000, 3), (11025, 16000, 1), (16000, 8000, 1), (32000, 16000, 2))


def formulas(src, dst):
    g = math.gcd(dst, src)
    up, down = dst // g, src // g
    half = 10 * max(up, down)
    return dict(up=up, down=down, half=half, K=-(-(2 * half + 1) // up))


def out_len(n, up, down):
    return -(-n * up // down)


_TAPS = {}


def scipy_taps(src, dst):
    """firwin(2 half + 1, 1 / max_rate, window=('kaiser', 5.0)) * up in fp64, computed once per ratio"""
    if (src, dst) not in _TAPS:
        from scipy.signal import firwin
        f = formulas(src, dst)
        h = firwin(2 * f['half'] + 1, 1.0 / max(f['up'], f['down']), window=('kaiser', 5.0)) * f['up']
        h.setflags(write=False)
        _TAPS[(src, dst)] = h
    return _TAPS[(src, dst)]


def host_downmix(pcm):
    """[n, C] int16 -> what AudioSegment makes of it: float32 / 32768, channel mean"""
    x = pcm.astype(np.float32) / 32768.0
    return x.mean(axis=1) if pcm.shape[1] > 1 else x[:, 0]


def check_filter_table(cdll, src, dst):
    from mvector import _hip
    rs = _hip.Resampler(src, dst, cdll=cdll)
    f = formulas(src, dst)
    assert (rs.up, rs.down, rs.half, rs.K) == (f['up'], f['down'], f['half'], f['K'])
    assert 1 <= rs.tile <= 1024
    for n in (0, 1, 7, f['down'], f['down'] + 1, 12345, 3 * src):
        assert rs.out_len(n) == out_len(n, f['up'], f['down']), n
    want = scipy_taps(src, dst).astype(np.float32)
    got = rs.taps()
    assert got.shape == want.shape == (2 * f['half'] + 1,) and got.dtype == np.float32
    ulp = np.spacing(np.abs(want))
    differ = int((got != want).sum())
    worst = float((np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp).max())
    print(f'taps {src} -> {dst}: {differ} of {want.size} taps differ from scipy\'s fp32 table, worst {worst:.2f} ulp')
    assert worst <= 1.0


def check_refusals(cdll, device):
    """a refusal is a returned status with a message that names the limit; nothing is launched"""
    from mvector import _hip
    lib = cdll or _hip.lib()
    msg = lambda: lib.mv_last_error().decode()
    h = ctypes.c_void_p()
    assert lib.mv_resampler_create(16001, 16000, ctypes.byref(h)) == -1 and 'max(up, down) above 1024' in msg() and not h.value
    assert lib.mv_resampler_create(0, 16000, ctypes.byref(h)) == -1 and 'rates must be positive' in msg() and not h.value
    assert lib.mv_resampler_create(16000, -1, ctypes.byref(h)) == -1 and 'rates must be positive' in msg() and not h.value
    with pytest.raises(RuntimeError, match=r'max\(up, down\) above 1024'):
        _hip.Resampler(16001, 16000, cdll=cdll)
    with pytest.raises(RuntimeError, match='rates must be positive'):
        _hip.Resampler(0, 16000, cdll=cdll)
    rs = _hip.Resampler(44100, 16000, cdll=cdll)
    B, L = 2, 3000
    L_out = rs.out_len(L)
    pcm = torch.zeros((B, L, 2), dtype=torch.int16, device=device)
    wav = torch.full((B, L_out), 7.0, device=device)
    need = lib.mv_resampler_workspace_bytes(rs._h, B, L)
    assert need >= 8 * B
    ws = torch.zeros(need + 16, dtype=torch.uint8, device=device)
    call = lambda channels=2, l_out=L_out, ws_ptr=ws.data_ptr(), nbytes=need, stride=L * 2: lib.mv_resampler_forward_i16(
        rs._h, pcm.data_ptr(), stride, channels, None, B, L, 0, 0.0, 300.0, wav.data_ptr(), L_out, l_out, None, None, ws_ptr, nbytes,
        _hip.current_stream(pcm))
    assert call(channels=9) == -1 and 'channels outside 1 .. 8' in msg()
    assert call(channels=0) == -1 and 'channels outside 1 .. 8' in msg()
    assert call(l_out=L_out - 1) == -1 and 'L_out smaller than mv_resampler_out_len' in msg()
    assert call(nbytes=need - 1) == -4 and 'workspace smaller' in msg()
    assert call(ws_ptr=None) == -1 and 'null workspace' in msg()
    assert call(stride=L * 2 - 1) == -1 and 'bad geometry' in msg()
    assert bool((wav == 7.0).all()), 'a refused call wrote to its output'
    assert call() == 0 and not bool(wav.any())
    with pytest.raises(RuntimeError, match='channels outside'):
        rs(torch.zeros((1, 10, 9), dtype=torch.int16, device=device))


def check_downmix(cdll, device, channels):
    """16000 -> 16000: the channel mean alone, bit for bit the host's"""
    from mvector import _hip
    rng = np.random.default_rng(40 + channels)
    B, L = 3, 1500                                              # more than one tile of the copy, a ragged last one
    pcm = rng.integers(-32768, 32768, size=(B, L, channels), dtype=np.int64).astype(np.int16)
    pcm[0, :4] = [[32767] * channels, [-32768] * channels, [32767] + [-32768] * (channels - 1), [1] * channels]   # the extremes of the integer sum
    rs = _hip.Resampler(16000, 16000, cdll=cdll)
    assert (rs.up, rs.down) == (1, 1) and rs.out_len(L) == L
    lens = torch.tensor([L, 1025, 0])
    wav, num_out, quiet = rs(torch.from_numpy(pcm).to(device), lens.to(device))
    want = np.zeros((B, L), dtype=np.float32)
    for b in range(B):
        want[b, :lens[b]] = host_downmix(pcm[b, :lens[b]])
    assert torch.equal(wav.cpu(), torch.from_numpy(want))
    assert num_out.tolist() == lens.tolist() and quiet.tolist() == [0, 0, 0]


_REF = {}


def reference(src, dst, channels):
    """the case's PCM, row lengths and fp64 reference, computed once: (pcm [B, L_in, C] int16, lens, ref rows, bound rows, L_in, tile)"""
    key = (src, dst, channels)
    if key not in _REF:
        from scipy.signal import resample_poly
        f = formulas(src, dst)
        up, down, K = f['up'], f['down'], f['K']
        tile = 1024                                            # (every ratio of the cases keeps the full tile: asserted against the handle below)
        # about one output tile plus 1000 frames, a multiple of `down` (so n up is divisible by down)
        L_in = -(-(tile * down // up + 1000) // down) * down
        # the shortest row that ends past the tile edge: one output past it wherever up < down
        n_edge = next(n for n in range(tile * down // up - 2, L_in) if out_len(n, up, down) > tile)
        lens = [L_in, 1, 7, K - 1, K + 1, n_edge]
        assert (L_in * up) % down == 0 and (down == 1 or any((n * up) % down for n in lens))
        rng = np.random.default_rng(src + dst + channels)
        pcm = np.round(6000.0 * rng.standard_normal((len(lens), L_in, channels))).clip(-32768, 32767).astype(np.int16)
        h64 = scipy_taps(src, dst)
        refs, bounds = [], []
        for b, n in enumerate(lens):
            x = host_downmix(pcm[b, :n])
            ref = resample_poly(x.astype(np.float64), up, down)
            mag = resample_poly(np.abs(x).astype(np.float64), up, down, window=np.abs(h64) / up)
            assert ref.shape == mag.shape == (out_len(n, up, down),)
            refs.append(ref)
            bounds.append((K + 3) * 2.0 ** -24 * mag)
        pcm.setflags(write=False)
        _REF[key] = (pcm, lens, refs, bounds, L_in, tile)
    return _REF[key]


def _strided(pcm, device, pad=5):
    """the PCM in rows `pad` elements longer than L_in * C (odd: every other row starts off a 4-byte boundary)"""
    B, L, C = pcm.shape
    buf = torch.zeros((B, L * C + pad), dtype=torch.int16)
    buf[:, :L * C] = torch.from_numpy(np.array(pcm).reshape(B, L * C))
    view = buf.to(device)[:, :L * C].unflatten(1, (L, C))
    assert view.stride() == (L * C + pad, C, 1)
    return view


def check_resample(cdll, device, src, dst, channels, second_stream=False):
    from mvector import _hip
    pcm, lens, refs, bounds, L_in, tile = reference(src, dst, channels)
    f = formulas(src, dst)
    rs = _hip.Resampler(src, dst, cdll=cdll)
    assert rs.tile == tile
    dev_pcm = _strided(pcm, device)
    n_dev = torch.tensor(lens, dtype=torch.int64, device=device)
    wav, num_out, quiet = rs(dev_pcm, n_dev)
    L_out = out_len(L_in, f['up'], f['down'])
    assert wav.shape == (len(lens), L_out) and wav.dtype == torch.float32
    assert num_out.tolist() == [out_len(n, f['up'], f['down']) for n in lens] and quiet.tolist() == [0] * len(lens)
    y = wav.cpu().numpy()
    worst = 0.0
    for b, n in enumerate(lens):
        n_out = refs[b].shape[0]
        err = np.abs(y[b, :n_out].astype(np.float64) - refs[b])
        nz = bounds[b] > 0
        if nz.any():
            worst = max(worst, float((err[nz] / bounds[b][nz]).max()))
        assert bool((err <= bounds[b]).all()), f'row {b} (n = {n}): {int((err > bounds[b]).sum())} samples beyond the rounding bound'
        assert not y[b, n_out:].any(), f'row {b}: samples behind n_out'
    print(f'resample {src} -> {dst} C={channels}: worst |y - ref| = {worst:.3f} of the bound (K + 3) 2^-24 sum |x||h|, K = {f["K"]}')

    # a row alone, and a row beside an empty one, give the bits they have in the batch; the empty row is all zero
    for b in (0, 5):
        alone, n1, _ = rs(dev_pcm[b:b + 1], n_dev[b:b + 1])
        assert torch.equal(alone[0], wav[b]) and n1.tolist() == [num_out[b].item()], f'row {b} alone differs from the row in the batch'
    pair, n2, _ = rs(torch.stack([dev_pcm[4], dev_pcm[2]]).contiguous(), torch.tensor([lens[4], 0], device=device))
    assert torch.equal(pair[0], wav[4]) and n2.tolist() == [num_out[4].item(), 0] and not bool(pair[1].any())
    if second_stream:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            wav2, num_out2, _ = rs(dev_pcm, n_dev)
        torch.cuda.current_stream().wait_stream(side)
    else:
        wav2, num_out2, _ = rs(dev_pcm, n_dev)
    assert torch.equal(wav2, wav) and torch.equal(num_out2, num_out), 'not bit-identical on a second call / stream'


def check_normalize(cdll, device, src=44100, dst=16000, channels=2, target_db=-20.0):
    from mvector import _hip
    pcm, lens, refs, _, L_in, _ = reference(src, dst, channels)
    pcm = pcm.copy()
    pcm[2] = 0                                                  # digital silence: flagged, left finite
    lens = list(lens)
    lens[3] = 0                                                 # an empty row: flagged as mv_wave_prepare_i16 flags it
    rs = _hip.Resampler(src, dst, cdll=cdll)
    dev_pcm = _strided(pcm, device)
    n_dev = torch.tensor(lens, dtype=torch.int64, device=device)
    plain, num_out, quiet0 = rs(dev_pcm, n_dev, target_db=None)
    assert quiet0.tolist() == [0] * len(lens)                   # target_db=None: gain 1, no flags ...
    for b in (0, 1, 4, 5):
        err = np.abs(plain[b, :refs[b].shape[0]].cpu().numpy() - refs[b]).max()
        assert err < 2e-6 * max(1.0, np.abs(refs[b]).max())     # ... and the plain rows
    wav, num_out2, quiet = rs(dev_pcm, n_dev, target_db=target_db)
    assert torch.equal(num_out2, num_out)
    assert quiet.tolist() == [0, 0, 1, 1, 0, 0]
    y = wav.cpu().numpy()
    assert np.isfinite(y).all() and not y[2].any() and not y[3].any()
    for b in (0, 1, 4, 5):
        ref = refs[b]
        gain = 10.0 ** ((target_db - 10.0 * np.log10(np.mean(ref ** 2))) / 20.0)
        want = ref * gain
        err = np.abs(y[b, :ref.shape[0]] - want).max()
        print(f'normalize row {b} (n = {lens[b]}): gain {gain:.4f}, max abs err {err:.2e} against {2e-6 * max(1.0, np.abs(want).max()):.2e}')
        assert err < 2e-6 * max(1.0, np.abs(want).max()), err
        assert not y[b, ref.shape[0]:].any()
    again, _, _ = rs(dev_pcm, n_dev, target_db=target_db)
    assert torch.equal(again, wav)
    alone, _, q1 = rs(dev_pcm[5:6], n_dev[5:6], target_db=target_db)
    assert torch.equal(alone[0], wav[5]) and q1.tolist() == [0], 'a normalised row alone differs from the row in the batch'


def check_extreme_ratio(cdll, device):
    """1000 : 1 -- the table and a tile's source span do not fit into LDS together: the table is read from global memory, tiles are short"""
    from mvector import _hip
    from scipy.signal import resample_poly
    src, dst = 16000000, 16000
    rs = _hip.Resampler(src, dst, cdll=cdll)
    f = formulas(src, dst)
    assert (rs.up, rs.down, rs.K) == (1, 1000, 20001) and not rs.table_in_lds and rs.tile < 64
    n = (rs.tile + 2) * 1000 + 123                              # two tiles and a bit
    rng = np.random.default_rng(5)
    pcm = np.round(6000.0 * rng.standard_normal((2, n, 1))).clip(-32768, 32767).astype(np.int16)
    lens = [n, 1500]
    wav, num_out, _ = rs(torch.from_numpy(pcm).to(device), torch.tensor(lens, device=device))
    assert num_out.tolist() == [out_len(m, 1, 1000) for m in lens]
    h64 = scipy_taps(src, dst)
    for b, m in enumerate(lens):
        x = host_downmix(pcm[b, :m])
        ref = resample_poly(x.astype(np.float64), 1, 1000)
        mag = resample_poly(np.abs(x).astype(np.float64), 1, 1000, window=np.abs(h64))
        y = wav[b].cpu().numpy()
        assert bool((np.abs(y[:ref.shape[0]] - ref) <= (f['K'] + 3) * 2.0 ** -24 * mag).all()) and not y[ref.shape[0]:].any()
