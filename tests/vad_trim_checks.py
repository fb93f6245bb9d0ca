"""Checks of what follows the energy VAD on the device (csrc/vad.hip: mv_vad_regions_i32, mv_wave_gather_f32) shared by tests/test_vad_trim.py (the
emulator build, CPU tensors) and tests/test_gpu_vad_trim.py (the product library on the device).  Each takes the bound library (None = the product
library) and a device.

Everything here is integer or copy work, so every comparison is for equality:
  * regions: `==` against EnergyVad.smooth (numpy, mvector/infer_utils/vad.py) of the same run list, for the count, every pair and the kept sum.  The
    run lists are synthetic -- the entry point takes runs, not waveforms --, drawn around the three thresholds so that joining, dropping and the stop
    at the middle of a gap all fire, with 0, 1, 2, R - 1, R, R + 1 and 2 R + 3 runs per row (R = MV_VAD_REGION_TILE, the runs one tile holds);
  * gather: the int32 view of the output against the numpy concatenation of the int32 view of the input, whose words are random bits (NaNs of every
    payload, -0.0, denormals: a copy that computes with a sample would show);
  * the chain: EnergyVad.trim on the device against EnergyVad.trim in numpy, on the signals of vad_checks whose frames all lie more than 1e-6 from
    the threshold (so the decisions are the oracle's)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import vad_checks as vc

TIGHT = dict(min_silence=0.02, min_speech=0.01, speech_pad=0.03)   # tests/test_vad.py's: 320 / 160 / 480 samples
SMOOTHINGS = {'default': dict(), 'tight': TIGHT}


def tiles():
    from mvector import _hip
    return _hip.MV_VAD_REGION_TILE, _hip.MV_WAVE_GATHER_TILE


def energy_vad(smoothing='default', cdll=None, **kw):
    from mvector.infer_utils.vad import EnergyVad
    return EnergyVad(cdll=cdll, **dict(SMOOTHINGS[smoothing], **kw))


def smooth_cfg(vad, **over):
    from mvector import _hip
    values = dict(frame_shift=vad.cfg['frame_shift'], min_silence=vad.min_silence, min_speech=vad.min_speech, speech_pad=vad.speech_pad)
    values.update(over)
    return _hip.MvVadSmoothCfg(**values)


# ------------------------------------------------------------------------------------------------ regions
def draw_runs(count, vad, rng, from_zero, to_the_end):
    """-> (runs int32 [count, 2], T, n): gaps of min_silence -1 / +0 / +1 frame, of 1 .. 3 frames and long ones; runs of min_speech -1 / +0 / +1
    frame, single frames and long ones.  to_the_end: the last run reaches the last frame and n is not T * shift"""
    shift, length = vad.cfg['frame_shift'], vad.cfg['frame_length']
    sil, sp = vad.min_silence // shift, vad.min_speech // shift
    gaps = [max(1, sil - 1), max(1, sil), sil + 1, 1, 2, 3, 2 * sil + 5]
    lens = [max(1, sp - 1), max(1, sp), sp + 1, 1, 3 * sp + 2]
    runs, t = [], 0
    for i in range(count):
        if i or not from_zero:
            t += int(rng.choice(gaps))
        d = int(rng.choice(lens))
        runs.append([t, t + d])
        t += d
    T = t if to_the_end and count else t + 5
    n = max(T - 1, 0) * shift + length + (7 if to_the_end else 3)
    assert n != T * shift
    return np.array(runs, dtype=np.int32).reshape(-1, 2), T, n


@functools.lru_cache(maxsize=None)
def run_batch(smoothing):
    """-> (vad, runs per row, T per row, n per row, the oracle's regions per row): rows of 0, 1, 2, R - 1, R, R + 1, 2 R + 3 runs"""
    R, _ = tiles()
    vad = energy_vad(smoothing)
    rng = np.random.default_rng(41 + len(smoothing))
    rows = [draw_runs(c, vad, rng, from_zero=k % 2 == 1, to_the_end=k % 3 != 0) for k, c in enumerate((0, 1, 2, R - 1, R, R + 1, 2 * R + 3))]
    want = [vad.smooth(r, T, n) for r, T, n in rows]
    assert any(r[0].shape[0] and r[0][0, 0] == 0 for r in rows) and any(r[0].shape[0] and r[0][-1, 1] == r[1] for r in rows)
    big, w = rows[-1][0].astype(np.int64) * vad.cfg['frame_shift'], want[-1]
    gap = big[1:, 0] - big[:-1, 1]
    assert (gap < vad.min_silence).any() and (gap >= vad.min_silence).any(), 'no gap is joined, or none stays'
    if smoothing == 'default':   # (the tight min_speech is one frame: no run is shorter)
        assert 0 < w.shape[0] < (gap >= vad.min_silence).sum() + 1, 'no joined region is dropped'
    else:
        assert (w[1:, 0] == w[:-1, 1]).any() and (w[1:, 0] > w[:-1, 1]).any(), 'no padding stops at the middle of a gap, or every one does'
    return vad, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], want


def raw_regions(cdll, device, vad, runs, T, n, fill, max_runs=None, num_runs=None, stream=None, lengths=True):
    """the C entry point over outputs and a workspace pre-filled with ``fill`` bytes, guard bytes behind each -> (num_regions, regions, kept) on the
    host, the pairs behind every row's count checked to be untouched and cleared"""
    from mvector import _hip
    lib = cdll or _hip.lib()
    B = len(runs)
    max_runs = max([r.shape[0] for r in runs] + [1]) if max_runs is None else max_runs
    host = np.zeros((B, max_runs, 2), dtype=np.int32)
    for b, r in enumerate(runs):
        host[b, :min(r.shape[0], max_runs)] = r[:max_runs]
    d_runs = torch.from_numpy(host).to(device)
    d_nr = torch.tensor([r.shape[0] for r in runs] if num_runs is None else num_runs, dtype=torch.int32, device=device)
    d_T = torch.tensor(T, dtype=torch.int32, device=device)
    d_n = torch.tensor(n, dtype=torch.int64, device=device) if lengths else None
    L = max(n)
    need = int(lib.mv_vad_regions_workspace_bytes(B, max_runs))
    sizes = dict(num_regions=4 * B, regions=8 * B * max_runs, kept=8 * B, ws=need)
    buf = {k: torch.full((v + 16,), fill, dtype=torch.uint8, device=device) for k, v in sizes.items()}
    c = smooth_cfg(vad)
    _hip.check(lib.mv_vad_regions_i32(ctypes.byref(c), d_T.data_ptr(), d_nr.data_ptr(), d_runs.data_ptr(), max_runs, _hip._ptr(d_n), B, L,
                                      buf['num_regions'].data_ptr(), buf['regions'].data_ptr(), buf['kept'].data_ptr(), buf['ws'].data_ptr(), need,
                                      stream if stream is not None else _hip.current_stream(d_runs)), lib)
    got = {k: v.cpu() for k, v in buf.items()}
    for k, v in sizes.items():
        assert bool((got[k][v:] == fill).all()), f'wrote past {k}'
    num = got['num_regions'][:4 * B].view(torch.int32)
    reg = got['regions'][:8 * B * max_runs].view(torch.int32).view(B, max_runs, 2)
    kept = got['kept'][:8 * B].view(torch.int64)
    for b, k in enumerate(num.tolist()):
        assert bool((reg[b, max(k, 0):].contiguous().view(torch.uint8) == fill).all()), f'row {b}: pairs behind the region count were written'
        reg[b, max(k, 0):] = 0
    return num, reg, kept


def assert_regions(got, want, what):
    num, reg, kept = (g.cpu().numpy() for g in got)
    for b, w in enumerate(want):
        assert num[b] == w.shape[0], f'{what} row {b}: {num[b]} regions, smooth has {w.shape[0]}'
        assert np.array_equal(reg[b, :w.shape[0]], w), f'{what} row {b}: regions differ first at {np.flatnonzero((reg[b, :w.shape[0]] != w).any(axis=1))[:3].tolist()}'
        assert kept[b] == (w[:, 1] - w[:, 0]).sum(), f'{what} row {b}: kept {kept[b]}'


def check_regions_equal_smooth(cdll, device, smoothing):
    """the batch of synthetic run lists through _hip.vad_regions (device tensors in, device tensors out) and through the raw entry point"""
    from mvector import _hip
    vad, runs, T, n, want = run_batch(smoothing)
    B, max_runs = len(runs), max(r.shape[0] for r in runs)
    host = np.zeros((B, max_runs, 2), dtype=np.int32)
    for b, r in enumerate(runs):
        host[b, :r.shape[0]] = r
    vad_out = dict(num_frames=torch.tensor(T, dtype=torch.int32, device=device), num_runs=torch.tensor([r.shape[0] for r in runs], dtype=torch.int32, device=device),
                   runs=torch.from_numpy(host).to(device))
    got = _hip.vad_regions(vad_out, torch.tensor(n), vad.cfg['frame_shift'], vad.min_silence, vad.min_speech, vad.speech_pad, L=max(n), cdll=cdll)
    assert all(g.device == vad_out['runs'].device for g in got) and got[0].dtype == torch.int32 and got[2].dtype == torch.int64
    assert_regions(got, want, f'{smoothing}')
    assert_regions(raw_regions(cdll, device, vad, runs, T, n, 0xFF), want, f'{smoothing} (raw)')
    return [w.shape[0] for w in want]


HAND_T, HAND_N = 200, 199 * 160 + 400
HAND_CASES = (   # tests/test_vad.py, test_segment_smoothing_against_hand_written_cases: (smoothing, runs, regions)
    ('default', [[10, 50], [79, 120]], [[1600 - 480, 19200 + 480]]),                      # a gap of 29 frames (4640 samples) is joined
    ('default', [[10, 50], [80, 120]], [[1600 - 480, 8000 + 480], [12800 - 480, 19200 + 480]]),   # one of 30 frames (4800) stays
    ('default', [[10, 34]], []), ('default', [[10, 35]], [[1600 - 480, 5600 + 480]]),     # 24 frames are dropped, 25 stay
    ('default', [[10, 22], [32, 44]], [[1600 - 480, 7040 + 480]]),                        # the joining comes first
    ('default', [[1, 40]], [[0, 6400 + 480]]),                                            # the padding stops at 0 ...
    ('default', [[150, 199]], [[24000 - 480, HAND_N]]),                                   # ... and at n
    ('default', [[150, 200]], [[24000 - 480, HAND_N]]),                                   # a run to the last frame ends with the recording
    ('default', [], []), ('default', [[3, 5]], []),
    ('tight', [[10, 20], [23, 40]], [[1600 - 480, 3200 + 240], [3680 - 240, 6400 + 480]]),   # ... and at the middle of a gap
    ('tight', [[10, 20], [22, 40]], [[1600 - 480, 3200 + 160], [3520 - 160, 6400 + 480]]),
)


def check_hand_written_cases(cdll, device):
    for smoothing in SMOOTHINGS:
        vad = energy_vad(smoothing)
        cases = [c for c in HAND_CASES if c[0] == smoothing]
        runs = [np.array(c[1], dtype=np.int32).reshape(-1, 2) for c in cases]
        want = [np.array(c[2], dtype=np.int64).reshape(-1, 2) for c in cases]
        for r, w in zip(runs, want):
            assert vad.smooth(r, HAND_T, HAND_N).tolist() == w.tolist()
        assert_regions(raw_regions(cdll, device, vad, runs, [HAND_T] * len(runs), [HAND_N] * len(runs), 0xFF, lengths=False), want, f'hand-written ({smoothing})')


def check_truncated_row(cdll, device):
    """max_runs below one row's num_runs: that row reports -1 / -1 and nothing of it is written, its neighbours are what they are alone"""
    vad = energy_vad('tight')
    rng = np.random.default_rng(5)
    rows = [draw_runs(c, vad, rng, False, True) for c in (3, 9, 4)]
    runs, T, n = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
    num, reg, kept = raw_regions(cdll, device, vad, runs, T, n, 0xFF, max_runs=4)
    assert num.tolist()[1] == -1 and kept.tolist()[1] == -1 and not reg[1].any()
    for b in (0, 2):
        w = vad.smooth(runs[b], T[b], n[b])
        assert num[b] == w.shape[0] > 0 and reg[b, :w.shape[0]].tolist() == w.tolist() and kept[b] == (w[:, 1] - w[:, 0]).sum()


# ------------------------------------------------------------------------------------------------ gather
@functools.lru_cache(maxsize=None)
def gather_case():
    """-> (words int32 [B, L] of random bits, n per row, regions per row (None: a skipped row)); see check_gather for what each row is there for"""
    R, G = tiles()
    L = 2 * G + 38
    rng = np.random.default_rng(77)
    words = rng.integers(-2 ** 31, 2 ** 31, size=(9, L), dtype=np.int64).astype(np.int32)
    words[0, 16:20] = [0x7FC12345, -0x5FFFFF, -2 ** 31, 0x7F800001]   # quiet and signalling NaNs with payloads, -0.0: in the 16-byte path of row 0 ...
    words[0, 41:45] = [0x7FC12345, -0x5FFFFF, -2 ** 31, 0x7F800001]   # ... and in its scalar path
    n = [L, L, L, L, L, L, L - 101, L, L]
    small = np.cumsum(rng.integers(0, 7, size=2 * R + 3)) * 2
    rows = [
        # starts = 0, 1, 2, 3 (mod 4); a region of one sample; an empty one (e = s) and one with e < s; an overlap out of order; one that ends at n
        [[16, 40], [41, 77], [102, 131], [203, 260], [300, 301], [500, 500], [640, 600], [20, 36], [L - 9, L]],
        [],                                                            # no regions
        [[3, 3 + G + 1]],                                              # ends one sample behind a tile edge
        [[5, 5 + G - 1]],                                              # ends one sample before a tile edge
        [[int(s), int(s) + int(d)] for s, d in zip(small, rng.integers(0, 6, size=2 * R + 3))],   # more regions than the search table holds, in one tile
        None,                                                          # skipped by mv_vad_regions_i32
        [[-7, 30], [L - 150, L + 9], [L - 101, L]],                    # clamped to [0, n]: the last one is empty
        [[1, 2 * G + 30]],                                             # nearly the whole row from an odd start: every trip of two tiles
        [[2, 9], [11, 12], [13, 16], [18, 19], [22, 29]],              # threads whose four outputs span several regions
    ]
    return words, n, rows


def gather_reference(words, n, rows, L_out):
    out, total = np.zeros((len(rows), L_out), dtype=np.int32), []
    for b, regs in enumerate(rows):
        if regs is None:
            total.append(-1)
            continue
        parts = [words[b, min(max(s, 0), n[b]):min(max(e, 0), n[b])] for s, e in regs]
        row = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)
        total.append(row.shape[0])
        out[b, :min(row.shape[0], L_out)] = row[:L_out]
    return out, total


def region_table(rows, device):
    max_regions = max(len(r) for r in rows if r is not None)
    host = np.full((len(rows), max_regions, 2), 12345, dtype=np.int32)   # what lies behind a row's count is never looked at
    for b, r in enumerate(rows):
        if r:
            host[b, :len(r)] = r
    return torch.tensor([-1 if r is None else len(r) for r in rows], dtype=torch.int32, device=device), torch.from_numpy(host).to(device)


def device_words(words, device, pitch):
    """[B, L] int32 -> fp32 view on the device with row stride ``pitch``"""
    host = np.zeros((words.shape[0], pitch), dtype=np.int32)
    host[:, :words.shape[1]] = words
    wav = torch.from_numpy(host).to(device).view(torch.float32)[:, :words.shape[1]]
    assert wav.stride(0) == pitch
    return wav


def raw_gather(cdll, wav, n, num_regions, regions, L_out, out_pitch, fill, stream=None, out_offset=0):
    """the C entry point over an output (row stride out_pitch, ``out_offset`` floats behind a 16-byte boundary) and a workspace pre-filled with
    ``fill`` bytes -> (out int32 [B, L_out], out_samples) on the host; the pitch gaps, the guard bytes and what lies behind them are checked"""
    from mvector import _hip
    lib = cdll or _hip.lib()
    B, L = wav.shape
    max_regions = regions.shape[1]
    need = int(lib.mv_wave_gather_workspace_bytes(B, max_regions))
    assert need > 0
    flat = torch.full((4 * (out_offset + B * out_pitch) + 16,), fill, dtype=torch.uint8, device=wav.device)
    outs = torch.full((8 * B + 16,), fill, dtype=torch.uint8, device=wav.device)
    ws = torch.full((need + 16,), fill, dtype=torch.uint8, device=wav.device)
    d_n = None if n is None else torch.tensor(n, dtype=torch.int64, device=wav.device)
    assert flat.data_ptr() % 16 == 0
    _hip.check(lib.mv_wave_gather_f32(wav.data_ptr(), wav.stride(0), _hip._ptr(d_n), num_regions.data_ptr(), regions.data_ptr(), max_regions, B, L,
                                      flat.data_ptr() + 4 * out_offset, out_pitch, L_out, outs.data_ptr(), ws.data_ptr(), need,
                                      stream if stream is not None else _hip.current_stream(wav)), lib)
    host, houts, hws = flat.cpu(), outs.cpu(), ws.cpu()
    assert bool((host[:4 * out_offset] == fill).all()) and bool((host[4 * (out_offset + B * out_pitch):] == fill).all()) and bool((houts[8 * B:] == fill).all()) \
        and bool((hws[need:] == fill).all()), 'wrote outside a buffer'
    grid = host[4 * out_offset:4 * (out_offset + B * out_pitch)].view(torch.int32).view(B, out_pitch)
    assert bool((grid[:, L_out:].contiguous().view(torch.uint8) == fill).all()), 'wrote between the rows'
    return grid[:, :L_out].contiguous(), houts[:8 * B].view(torch.int64)


def check_gather(cdll, device):
    """every row of gather_case through _hip.wave_gather (the source rows 4-byte aligned only, wav_stride > L; the output rows alternately 16- and
    8-byte aligned), then through the raw entry point with an output that is one float off a 16-byte boundary, and with L_out below a row's total"""
    from mvector import _hip
    R, G = tiles()
    words, n, rows = gather_case()
    B, L = words.shape
    wav = device_words(words, device, L + 3)
    assert (L + 3) % 4 == 1 and {(wav.data_ptr() + 4 * b * wav.stride(0)) % 16 for b in range(B)} == {0, 4, 8, 12}
    num_regions, regions = region_table(rows, device)
    want, total = gather_reference(words, n, rows, L)
    assert total[2] == G + 1 and total[3] == G - 1 and len(rows[4]) == 2 * R + 3 and total[4] < G and total[7] > 2 * G
    out, out_samples = _hip.wave_gather(wav, torch.tensor(n), num_regions, regions, cdll=cdll)
    assert out.shape == (B, L) and out.dtype == torch.float32 and out.device == wav.device and out_samples.dtype == torch.int64
    assert out_samples.cpu().tolist() == total
    assert torch.equal(out.cpu().view(torch.int32), torch.from_numpy(want)), f'rows {np.flatnonzero((out.cpu().view(torch.int32).numpy() != want).any(axis=1)).tolist()} differ'
    for offset, L_out in ((1, L), (0, G + 5), (3, 100), (0, 0)):
        got, samples = raw_gather(cdll, wav, n, num_regions, regions, L_out, L_out + 6, 0xFF, out_offset=offset)
        w, _ = gather_reference(words, n, rows, L_out)
        assert samples.tolist() == total, 'the true total is reported whatever L_out'
        assert torch.equal(got, torch.from_numpy(w)), (offset, L_out)
    lone, _ = raw_gather(cdll, wav, None, num_regions, regions, L, L, 0xFF)   # num_samples = NULL: every row has L samples
    assert torch.equal(lone, torch.from_numpy(gather_reference(words, [L] * B, rows, L)[0]))


# ------------------------------------------------------------------------------------------------ the chain
CHAIN = {'default': ('bursts/default', 'batch/default', 'silence/default', 'edge0/default', 'speech/default'),
         'recipe': ('bursts/recipe', 'batch/recipe', 'silence/recipe', 'edge1/recipe', 'speech/recipe')}


def device_trim(vad, wav, lengths):
    """EnergyVad.trim of a CUDA tensor; for CPU tensors (the emulator build behind vad._cdll) the calls its device path is made of"""
    if wav.is_cuda:
        return vad.trim(wav, lengths=lengths)
    from mvector import _hip
    num_regions, regions, kept, lens = vad._device_regions(wav, lengths)
    return _hip.wave_gather(wav, lens, num_regions, regions, cdll=vad._cdll)[0], kept


def check_trim_chain(cdll, device, setting, smoothing):
    """VAD -> regions -> gather on the device against EnergyVad.trim on the same array in numpy: kept and every sample, rows with their own lengths"""
    rows = []
    for name in CHAIN[setting]:
        vc.reference(name)   # (asserts that every frame lies more than 1e-6 from its row's threshold)
        rows += vc.case(name)[0]
    cfg = vc.SETTINGS[setting]
    vad = energy_vad(smoothing, cdll=cdll, frames_context=cfg['frames_context'], energy_threshold=cfg['energy_threshold'],
                     proportion_threshold=cfg['proportion_threshold'])
    assert vad.cfg == {k: cfg[k] for k in vad.cfg}
    L = max(r.shape[0] for r in rows)
    host = np.zeros((len(rows), L), dtype=np.float32)
    for b, r in enumerate(rows):
        host[b, :r.shape[0]] = r
    lengths = [r.shape[0] for r in rows]
    want, want_kept = vad.trim(host, lengths=lengths)
    assert want.shape == host.shape and want_kept.dtype == np.int64
    assert min(lengths) < cfg['frame_length'] and (want_kept == 0).sum() >= 3 and (want_kept > 0).sum() >= 4   # shorter than a frame, silence; speech
    got, kept = device_trim(vad, torch.from_numpy(host).to(device), lengths)
    assert got.device.type == torch.device(device).type and kept.dtype == torch.int64
    assert kept.cpu().tolist() == want_kept.tolist()
    assert torch.equal(got.cpu().view(torch.int32), torch.from_numpy(want).view(torch.int32))
    if got.is_cuda:   # the public methods on CUDA tensors: regions, and a 1-D waveform ([L] and a scalar on both paths)
        num, reg, k2 = vad.regions(torch.from_numpy(host).to(device), lengths=lengths)
        hnum, hreg, hk2 = vad.regions(host, lengths=lengths)
        assert num.is_cuda and num.cpu().tolist() == hnum.tolist() and k2.cpu().tolist() == hk2.tolist() == want_kept.tolist() and reg.shape == hreg.shape
        for b, c in enumerate(hnum.tolist()):
            assert reg[b, :c].cpu().tolist() == hreg[b, :c].tolist()
        b = int(np.argmax(want_kept))
        one, one_kept = vad.trim(torch.from_numpy(rows[b]).to(device))
        h_one, h_kept = vad.trim(rows[b])
        assert one.shape == h_one.shape == rows[b].shape and int(one_kept) == int(h_kept) == want_kept[b] and np.array_equal(one.cpu().numpy(), h_one)
    return want_kept.tolist()


# ------------------------------------------------------------------------------------------------ no hidden state
def check_no_hidden_state(cdll, device, second_stream=False):
    vad, runs, T, n, want = run_batch('tight')
    ff = raw_regions(cdll, device, vad, runs, T, n, 0xFF)
    zz = raw_regions(cdll, device, vad, runs, T, n, 0x00)
    assert all(torch.equal(a, b) for a, b in zip(ff, zz)), 'regions: the result depends on what the buffers held'
    assert_regions(ff, want, '0xFF-filled buffers')
    for b in (1, 4, 6):   # a row alone: its bits do not depend on the batch it sits in
        one = raw_regions(cdll, device, vad, [runs[b]], [T[b]], [n[b]], 0xFF)
        c = want[b].shape[0]
        assert one[0].tolist() == [c] and torch.equal(one[1][0, :c], ff[1][b, :c]) and one[2][0] == ff[2][b]
    words, gn, rows = gather_case()
    B, L = words.shape
    wav = device_words(words, device, L + 3)
    num_regions, regions = region_table(rows, device)
    g_ff = raw_gather(cdll, wav, gn, num_regions, regions, L, L + 2, 0xFF)
    g_zz = raw_gather(cdll, wav, gn, num_regions, regions, L, L + 2, 0x00)
    assert all(torch.equal(a, b) for a, b in zip(g_ff, g_zz)), 'gather: the result depends on what the buffers held'
    assert torch.equal(g_ff[0], torch.from_numpy(gather_reference(words, gn, rows, L)[0]))
    for b in (0, 4, 6):
        nr, rg = region_table([rows[b]], device)
        one = raw_gather(cdll, device_words(words[b:b + 1], device, L + 3), [gn[b]], nr, rg, L, L + 2, 0xFF)
        assert torch.equal(one[0][0], g_ff[0][b]) and one[1][0] == g_ff[1][b]
    if second_stream:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            other = raw_regions(cdll, device, vad, runs, T, n, 0xFF, stream=side.cuda_stream)
            g_other = raw_gather(cdll, wav, gn, num_regions, regions, L, L + 2, 0xFF, stream=side.cuda_stream)
        side.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(other, ff)) and all(torch.equal(a, b) for a, b in zip(g_other, g_ff)), 'another stream gives other bits'


# ------------------------------------------------------------------------------------------------ refusals
def check_refusals(cdll, device):
    """a refusal is a returned status with a message that names the argument; nothing is launched, nothing is written"""
    from mvector import _hip
    lib = cdll or _hip.lib()
    msg = lambda: lib.mv_last_error().decode()
    vad = energy_vad()
    B, max_runs, L = 2, 6, 40000
    stream = _hip.current_stream(torch.zeros(1, device=device))
    ints = torch.zeros((64,), dtype=torch.int32, device=device)          # num_frames, num_runs, runs: zeros (no runs)
    out = torch.full((4096,), 0x5A, dtype=torch.uint8, device=device)
    need = int(lib.mv_vad_regions_workspace_bytes(B, max_runs))
    assert need >= B * max_runs * 8 and int(lib.mv_vad_regions_workspace_bytes(-1, max_runs)) == 0 and int(lib.mv_vad_regions_workspace_bytes(B, -1)) == 0
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=device)
    p, q = ints.data_ptr(), out.data_ptr()

    def regions(cfg=smooth_cfg(vad), nf=p, nr=p + 16, runs=p + 32, max_runs=max_runs, B=B, L=L, num=q, reg=q + 64, kept=q + 1024, ws_ptr=ws.data_ptr(), nbytes=need):
        return lib.mv_vad_regions_i32(None if cfg is None else ctypes.byref(cfg), nf, nr, runs, max_runs, None, B, L, num, reg, kept, ws_ptr, nbytes, stream)
    assert regions(cfg=None) == -1 and 'null cfg' in msg()
    for null in ('nf', 'nr', 'runs', 'num', 'reg', 'kept'):
        assert regions(**{null: None}) == -1 and 'null tensor' in msg(), null
    assert regions(ws_ptr=None) == -1 and 'null workspace' in msg()
    for neg in ('B', 'L', 'max_runs'):
        assert regions(**{neg: -1}) == -1 and 'negative B, L or max_runs' in msg(), neg
    assert regions(cfg=smooth_cfg(vad, frame_shift=0)) == -1 and 'frame_shift below 1' in msg()
    for field in ('min_silence', 'min_speech', 'speech_pad'):
        assert regions(cfg=smooth_cfg(vad, **{field: -1})) == -1 and 'negative min_silence, min_speech or speech_pad' in msg(), field
    assert regions(L=2 ** 31) == -1 and 'L above 2^31 - 1' in msg()
    assert regions(reg=p + 32) == -1 and 'regions aliases runs' in msg()
    assert regions(reg=p + 32 + 8 * B * max_runs - 4) == -1 and 'regions aliases runs' in msg()   # the last word of runs
    assert regions(nbytes=need - 1) == -4 and 'workspace smaller' in msg()
    assert bool((out == 0x5A).all()) and bool((ws == 0x5A).all()), 'a refused call wrote to its buffers'
    assert regions(B=0) == 0 and regions(B=0, nf=None, nr=None, runs=None, num=None, reg=None, kept=None, ws_ptr=None, nbytes=0) == 0
    assert bool((out == 0x5A).all()) and bool((ws == 0x5A).all()), 'B = 0 wrote to its buffers'
    assert regions(L=2 ** 31 - 1) == 0 and bool((out[:8] == 0).all()) and bool((out[1024:1040] == 0).all())   # the same arguments unrefused: no regions, kept 0

    out.fill_(0x5A)
    Lw = 300
    wav = torch.zeros((B, Lw + 4), dtype=torch.float32, device=device)
    dst = torch.full((B * (Lw + 4) * 4 + 64,), 0x5A, dtype=torch.uint8, device=device)
    gneed = int(lib.mv_wave_gather_workspace_bytes(B, max_runs))
    assert gneed >= B * (max_runs + 1) * 8 and int(lib.mv_wave_gather_workspace_bytes(-1, 3)) == 0 and int(lib.mv_wave_gather_workspace_bytes(B, -1)) == 0
    gws = torch.full((gneed,), 0x5A, dtype=torch.uint8, device=device)
    w, d = wav.data_ptr(), dst.data_ptr()

    def gather(wav_ptr=w, stride=Lw + 4, num=p, reg=p + 32, max_regions=max_runs, B=B, L=Lw, out_ptr=d, out_stride=Lw + 4, L_out=Lw, samples=q + 2048, ws_ptr=gws.data_ptr(),
               nbytes=gneed):
        return lib.mv_wave_gather_f32(wav_ptr, stride, None, num, reg, max_regions, B, L, out_ptr, out_stride, L_out, samples, ws_ptr, nbytes, stream)
    for null in ('wav_ptr', 'num', 'reg', 'out_ptr', 'samples'):
        assert gather(**{null: None}) == -1 and 'null tensor' in msg(), null
    assert gather(ws_ptr=None) == -1 and 'null workspace' in msg()
    for neg in ('B', 'L', 'L_out', 'max_regions'):
        assert gather(**{neg: -1}) == -1 and 'negative B, L, L_out or max_regions' in msg(), neg
    assert gather(stride=Lw - 1) == -1 and 'wav_stride below L' in msg()
    assert gather(out_stride=Lw - 1) == -1 and 'out_stride below L_out' in msg()
    assert gather(wav_ptr=w + 2) == -1 and 'not 4-byte aligned' in msg() and gather(out_ptr=d + 1) == -1 and 'not 4-byte aligned' in msg()
    assert gather(out_ptr=w) == -1 and 'out aliases wav' in msg()
    assert gather(out_ptr=w + 4 * ((B - 1) * (Lw + 4) + Lw - 1)) == -1 and 'out aliases wav' in msg()   # the last sample of wav
    assert gather(nbytes=gneed - 1) == -4 and 'workspace smaller' in msg()
    assert bool((out == 0x5A).all()) and bool((dst == 0x5A).all()) and bool((gws == 0x5A).all()), 'a refused call wrote to its buffers'
    assert gather(B=0) == 0 and gather(B=0, wav_ptr=None, num=None, reg=None, out_ptr=None, samples=None, ws_ptr=None, nbytes=0) == 0
    assert bool((out == 0x5A).all()) and bool((dst == 0x5A).all()), 'B = 0 wrote to its buffers'
    assert gather() == 0 and bool((out[2048:2064] == 0).all()) and bool((dst[:4 * Lw] == 0).all())   # unrefused: no regions, rows of zeros
    with pytest.raises(ValueError, match='lengths must have shape'):
        _hip.vad_regions(dict(num_frames=ints[:2], num_runs=ints[2:4], runs=ints[4:28].view(2, 6, 2)), torch.tensor([5]), 160, 0, 0, 0, cdll=cdll)
    with pytest.raises(ValueError, match='lengths or L'):
        _hip.vad_regions(dict(num_frames=ints[:2], num_runs=ints[2:4], runs=ints[4:28].view(2, 6, 2)), None, 160, 0, 0, 0, cdll=cdll)
    with pytest.raises(RuntimeError, match='frame_shift below 1'):
        _hip.vad_regions(dict(num_frames=ints[:2], num_runs=ints[2:4], runs=ints[4:28].view(2, 6, 2)), None, 0, 0, 0, 0, L=100, cdll=cdll)
    assert lib.mv_abi_version() == 5
