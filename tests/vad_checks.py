"""Checks of the energy VAD (csrc/vad.hip, mv_vad_energy_f32) shared by tests/test_vad.py (the emulator build, CPU tensors) and
tests/test_gpu_vad.py (the product library on the device).  Each takes the bound library (None = the product library) and a device.

The oracle below is the definition of include/mvector_hip.h written out frame by frame in numpy fp64, independently of
mvector/infer_utils/vad.py.  The bars are derived, not measured:
  * log energy: |logE_dev - logE_ref| <= 4 L 2^-53 max(1, |logE_ref|), L = frame_length: two fp64 sums of L terms (each within (L - 1) 2^-53
    relative of the exact one in ANY order) and one log, with slack.  Frames the oracle floors at eps = 2^-23 are equal exactly.
  * threshold: thr = et + ems * (S / T).  The device's S is a sum of T values, each within the bar above (d_t) of the oracle's, in another order:
    |S_dev - S_ref| <= sum d_t + 2 T 2^-53 sum |logE_t|; the division, the product and the sum add three roundings on either side:
    |thr_dev - thr_ref| <= |ems| (mean d_t + 2 T 2^-53 mean |logE_t|) + 8 2^-53 max(|thr|, |et|).
  * decisions, runs, counts: equal exactly.  The condition: every frame's |logE - thr| exceeds 1e-6 in the oracle, asserted on the inputs before
    anything is compared -- the rounding of either side (1e-12 at most) then cannot move a frame across the threshold.  It leaves out no frame.
    (A row with a NaN sample has a NaN threshold on both sides: every comparison with it is false whatever the rounding.)"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

EPS = 2.0 ** -23
U = 2.0 ** -53
DEFAULT = dict(frame_length=400, frame_shift=160, frames_context=0, energy_threshold=5.0, energy_mean_scale=0.5, proportion_threshold=0.6, scale=32768.0)
RECIPE = dict(DEFAULT, energy_threshold=5.5, frames_context=2, proportion_threshold=0.12)   # the VoxCeleb recipe's conf/vad.conf
SETTINGS = {'default': DEFAULT, 'recipe': RECIPE, 'context64': dict(DEFAULT, frames_context=64, proportion_threshold=0.3),
            'frames512': dict(RECIPE, frame_length=512, frame_shift=128), 'square': dict(DEFAULT, frame_length=160, frame_shift=160)}
FLOOR, LOUD = 3e-4, 0.1    # the noise floor and the bursts' amplitude: logE about 10.6 and 22.2 at the default frames


def tile_frames():
    from mvector import _hip
    return _hip.MV_VAD_TILE_FRAMES


def samples_for(T, cfg):
    """the fewest samples with T frames"""
    return (T - 1) * cfg['frame_shift'] + cfg['frame_length'] if T > 0 else cfg['frame_length'] - 1


# ------------------------------------------------------------------------------------------------ oracle
def num_frames_of(n, cfg):
    return 0 if n < cfg['frame_length'] else 1 + (n - cfg['frame_length']) // cfg['frame_shift']


def oracle_row(x, cfg):
    """x fp32 [n] -> dict(T, log_e [T], floored [T], thr, dec [T], runs [[a, b)], margin): one frame after the other"""
    length, shift, ctx = cfg['frame_length'], cfg['frame_shift'], cfg['frames_context']
    T = num_frames_of(x.shape[0], cfg)
    log_e, floored = np.zeros(T), np.zeros(T, dtype=bool)
    with np.errstate(invalid='ignore'):
        for t in range(T):
            v = x[t * shift:t * shift + length].astype(np.float64) * np.float64(cfg['scale'])
            m = v.sum() / length
            e = ((v - m) ** 2).sum()
            floored[t] = e < EPS
            log_e[t] = math.log(EPS) if e < EPS else (math.log(e) if e == e and e != math.inf else e)
        thr = cfg['energy_threshold'] + cfg['energy_mean_scale'] * (log_e.sum() / T) if T else math.nan
        above = [bool(v > thr) for v in log_e]
        margin = float(np.abs(log_e - thr).min()) if T and thr == thr else math.inf
    dec = np.zeros(T, dtype=np.uint8)
    for t in range(T):
        lo, hi = max(0, t - ctx), min(T - 1, t + ctx)
        num, den = sum(above[lo:hi + 1]), hi - lo + 1
        dec[t] = 1 if float(num) >= float(den) * cfg['proportion_threshold'] else 0
    runs, t = [], 0
    while t < T:
        if dec[t]:
            a = t
            while t < T and dec[t]:
                t += 1
            runs.append([a, t])
        else:
            t += 1
    return dict(T=T, log_e=log_e, floored=floored, thr=thr, dec=dec, runs=runs, margin=margin)


# ------------------------------------------------------------------------------------------------ inputs
def noise(n, seed, amp=1.0):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def burst_signal(n, bursts, seed, shift=160):
    """a FLOOR noise floor with bursts [(first frame, one past the last frame)] of amplitude-modulated LOUD noise; burst edges sit on multiples of
    the frame shift"""
    rng = np.random.default_rng(seed)
    x = FLOOR * rng.standard_normal(n)
    for a, b in bursts:
        lo, hi = a * shift, min(b * shift, n)
        tt = np.arange(hi - lo) / 16000.0
        x[lo:hi] = LOUD * (1.0 + 0.3 * np.sin(2 * np.pi * 3.0 * tt)) * rng.standard_normal(hi - lo)
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (rows: list of fp32 arrays (each row's own samples), cfg, expectation or None) of the named case"""
    F = tile_frames()
    if name == 'energy':   # kernel 1: seeded noise, a DC-dominated row, zeros, one NaN -- as one batch
        n = samples_for(F + 1, DEFAULT)
        nan_row = noise(n, 3, 0.05)
        nan_row[n // 2] = np.nan
        return [noise(n, 1, 0.05), (0.5 + 1e-5 * np.random.default_rng(2).standard_normal(n)).astype(np.float32), np.zeros(n, dtype=np.float32), nan_row], DEFAULT, None
    kind, _, setting = name.partition('/')
    cfg = SETTINGS[setting or 'default']
    shift = cfg['frame_shift']
    if kind == 'bursts':   # a run from frame 0, a run across the tile edge at F, a run to the last frame; context windows cross every tile edge
        T = 2 * F + 1
        n = samples_for(T, cfg)
        return [burst_signal(n, [(0, 30), (F - 12, F + 9), (2 * F - 40, 2 * F - 30), (T - 20, T + 99)], 7, shift)], cfg, None
    if kind.startswith('edge'):   # T = F - 1, F, F + 1: a run that lasts to the end -- its closing boundary is position T, in the next tile when T = F
        T = F + int(kind[4:])
        return [burst_signal(samples_for(T, cfg), [(5, 20), (T - 30, T + 99)], 11 + T, shift)], cfg, None
    if kind == 'short':   # n = frame_length - 1 and n = frame_length
        return [noise(cfg['frame_length'] - 1, 4, LOUD), noise(cfg['frame_length'], 5, LOUD)], cfg, dict(T=[0, 1])
    if kind == 'speech':
        return [noise(samples_for(F + 7, cfg), 6, LOUD)], cfg, dict(runs=[[[0, F + 7]]])
    if kind == 'silence':
        return [np.zeros(samples_for(F + 7, cfg), dtype=np.float32), noise(samples_for(F + 7, cfg), 8, 1e-4)], cfg, dict(runs=[[], []])
    if kind == 'square':   # the decision alternates every frame: loud even frames, floor odd frames (frames do not overlap in this setting)
        T = 2 * F + 1
        x = burst_signal(samples_for(T, cfg), [(t, t + 1) for t in range(0, T, 2)], 9, shift)
        return [x], cfg, dict(runs=[[[t, t + 1] for t in range(0, T, 2)]])
    if kind == 'batch':   # B = 3: lengths L, frame_length - 1, about L / 2
        T = F + 40
        n = samples_for(T, cfg)
        x = burst_signal(n, [(0, 12), (60, 130), (F - 5, F + 20)], 13, shift)
        return [x, x[:cfg['frame_length'] - 1], burst_signal(n // 2 + 3, [(20, 70), (100, 999)], 14, shift)], cfg, None
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    rows, cfg, expect = case(name)
    refs = [oracle_row(x, cfg) for x in rows]
    for r, ref in enumerate(refs):
        assert ref['margin'] > 1e-6, f'{name} row {r}: a frame within 1e-6 of the threshold ({ref["margin"]}): the input does not serve the exact comparison'
        if expect and 'T' in expect:
            assert ref['T'] == expect['T'][r]
        if expect and 'runs' in expect:
            assert ref['runs'] == expect['runs'][r], (name, r, ref['runs'][:4])
    return refs


def device_rows(rows, device, layout='dense'):
    """-> (wav [B, L] on the device, lengths int64 [B] or None).  layout: 'dense', 'strided' (row stride L + 5), 'offset' (one row, its pointer one
    float behind a 16-byte boundary)"""
    L = max(r.shape[0] for r in rows)
    pitch = L + 5 if layout == 'strided' else L
    host = np.zeros((len(rows), pitch), dtype=np.float32)
    for b, r in enumerate(rows):
        host[b, :r.shape[0]] = r
    if layout == 'offset':
        assert len(rows) == 1
        flat = torch.zeros(L + 1, dtype=torch.float32, device=device)
        wav = flat[1:].unsqueeze(0)
        wav.copy_(torch.from_numpy(host))
        assert wav.data_ptr() % 16 == 4
    else:
        wav = torch.from_numpy(host).to(device)[:, :L]
        assert wav.stride(0) == pitch
    same = all(r.shape[0] == L for r in rows)
    return wav, None if same else torch.tensor([r.shape[0] for r in rows], dtype=torch.int64)


def run(cdll, wav, lengths, cfg, **kw):
    from mvector import _hip
    out = _hip.vad_energy(wav, lengths=lengths, cdll=cdll, **kw, **cfg)
    assert all(v.device == wav.device for v in out.values())
    return out


def assert_against(out, refs, cfg, what):
    """the outputs of one call against the oracle's rows; returns the largest log-energy and threshold errors relative to their bars"""
    num_frames, num_runs = out['num_frames'].cpu().numpy(), out['num_runs'].cpu().numpy()
    log_e, thr = out['log_energy'].cpu().numpy(), out['threshold'].cpu().numpy()
    dec, runs = out['decisions'].cpu().numpy(), out['runs'].cpu().numpy()
    worst_e = worst_t = 0.0
    for b, ref in enumerate(refs):
        T = ref['T']
        assert num_frames[b] == T, f'{what} row {b}: {num_frames[b]} frames, the oracle has {T}'
        assert not log_e[b, T:].any() and not dec[b, T:].any(), f'{what} row {b}: entries behind the row\'s frames are not zero'
        got, want = log_e[b, :T], ref['log_e']
        assert np.array_equal(np.isnan(got), np.isnan(want)), f'{what} row {b}: NaN frames differ'
        ok = ~np.isnan(want)
        bar = 4 * cfg['frame_length'] * U * np.maximum(1.0, np.abs(want))
        err = np.abs(got - want)
        assert (err[ok] <= bar[ok]).all(), f'{what} row {b}: logE off at frames {np.flatnonzero(ok & ~(err <= bar))[:4].tolist()}: {err[ok].max()} (bar {bar[ok].min()})'
        assert np.array_equal(got[ref['floored']], want[ref['floored']]), f'{what} row {b}: a floored frame is not log(eps) exactly'
        if ok.any():
            worst_e = max(worst_e, float((err[ok] / bar[ok]).max()))
        if T == 0 or math.isnan(ref['thr']):
            assert math.isnan(thr[b]), f'{what} row {b}: threshold {thr[b]}, the oracle has NaN'
        else:
            bar_t = abs(cfg['energy_mean_scale']) * (bar.mean() + 2 * T * U * np.abs(want).mean()) + 8 * U * max(abs(ref['thr']), abs(cfg['energy_threshold']))
            assert abs(thr[b] - ref['thr']) <= bar_t, f'{what} row {b}: threshold off by {abs(thr[b] - ref["thr"])} (bar {bar_t})'
            worst_t = max(worst_t, abs(thr[b] - ref['thr']) / bar_t)
        assert np.array_equal(dec[b, :T], ref['dec']), f'{what} row {b}: decisions differ at frames {np.flatnonzero(dec[b, :T] != ref["dec"])[:6].tolist()}'
        assert num_runs[b] == len(ref['runs']), f'{what} row {b}: {num_runs[b]} runs, the oracle has {len(ref["runs"])}'
        k = min(len(ref['runs']), runs.shape[1])
        assert runs[b, :k].tolist() == ref['runs'][:k], f'{what} row {b}: runs differ: {runs[b, :k].tolist()[:4]} != {ref["runs"][:4]}'
    return worst_e, worst_t


# ------------------------------------------------------------------------------------------------ the checks
ENERGY_CASES = ('energy',)
RUN_CASES = ('bursts/default', 'bursts/recipe', 'bursts/context64', 'bursts/frames512', 'edge-1/default', 'edge0/default', 'edge0/recipe', 'edge1/recipe',
             'short/default', 'speech/default', 'speech/recipe', 'silence/default', 'silence/recipe', 'square/square', 'batch/default', 'batch/recipe')


def check_case(cdll, device, name, layout='dense'):
    rows, cfg, _ = case(name)
    refs = reference(name)
    wav, lengths = device_rows(rows, device, layout)
    out = run(cdll, wav, lengths, cfg)
    L = wav.shape[1]
    assert out['log_energy'].shape == (len(rows), num_frames_of(L, cfg)) and out['runs'].shape[1] == (num_frames_of(L, cfg) + 1) // 2
    worst = assert_against(out, refs, cfg, f'{name} ({layout})')
    return out, refs, worst


def check_log_energy(cdll, device):
    """kernel 1 alone: noise, DC-dominated, zeros, a NaN -- and the one-pass form sum v^2 - (sum v)^2 / L is NOT this definition on the DC row"""
    out, refs, worst = check_case(cdll, device, 'energy')
    rows, cfg, _ = case('energy')
    assert refs[2]['floored'].all() and not refs[0]['floored'].any()
    assert np.isnan(refs[3]['log_e']).sum() == 3 and math.isnan(refs[3]['thr']) and refs[3]['runs'] == []   # a sample lies in 2 or 3 frames of 400 / 160
    assert out['num_runs'].cpu().tolist()[3] == 0
    v = rows[1][:cfg['frame_length']].astype(np.float64) * cfg['scale']
    one_pass = (v * v).sum() - v.sum() ** 2 / cfg['frame_length']
    centred = math.exp(refs[1]['log_e'][0])
    assert abs(one_pass - centred) > 1e4 * 4 * cfg['frame_length'] * U * centred, 'the DC row does not separate the one-pass form from the centred one'
    return worst


def check_layouts(cdll, device):
    """a row stride above L; a row pointer one float behind a 16-byte boundary; both against the dense call's bits"""
    for name, layout in (('batch/recipe', 'strided'), ('edge1/recipe', 'offset'), ('bursts/frames512', 'offset')):
        out, _, _ = check_case(cdll, device, name, layout)
        rows, cfg, _ = case(name)
        dense = run(cdll, *device_rows(rows, device), cfg)
        assert same(host_view(out), host_view(dense)), f'{name} ({layout}): other bits than the dense layout'


def host_view(out):
    """the outputs of _hip.vad_energy on the host, the pairs behind every row's run count cleared (nothing is written there)"""
    host = {k: out[k].cpu().clone() for k in ('num_frames', 'num_runs', 'runs', 'log_energy', 'threshold', 'decisions')}
    for b, k in enumerate(host['num_runs'].tolist()):
        host['runs'][b, k:] = 0
    return host


def check_truncated_runs(cdll, device):
    """max_runs = 3 on the alternating input: the true count is reported, three pairs are written and nothing behind them"""
    rows, cfg, _ = case('square/square')
    ref = reference('square/square')[0]
    wav, lengths = device_rows(rows, device)
    assert len(ref['runs']) == (ref['T'] + 1) // 2 == tile_frames() + 1
    raw = raw_call(cdll, wav, lengths, cfg, 0xFF, max_runs=3)
    assert raw['num_runs'].tolist() == [len(ref['runs'])] and raw['runs'].tolist() == [ref['runs'][:3]]
    none = raw_call(cdll, wav, lengths, cfg, 0xFF, max_runs=0)
    assert none['num_runs'].tolist() == [len(ref['runs'])] and none['runs'].numel() == 0


def raw_call(cdll, wav, lengths, cfg, fill, max_runs=None, stream=None, optional=True):
    """the C entry point with outputs and workspace pre-filled with ``fill`` bytes and guard bytes behind each -> dict of CPU tensors"""
    from mvector import _hip
    lib = cdll or _hip.lib()
    B, L = wav.shape
    T = num_frames_of(L, cfg)
    max_runs = (T + 1) // 2 if max_runs is None else max_runs
    c = _hip.vad_cfg(**cfg)
    need = int(lib.mv_vad_energy_workspace_bytes(ctypes.byref(c), B, L))
    assert need > 0
    sizes = dict(num_frames=4 * B, num_runs=4 * B, runs=8 * B * max_runs, log_energy=8 * B * T, threshold=8 * B, decisions=B * T, ws=need)
    buf = {k: torch.full((v + 16,), fill, dtype=torch.uint8, device=wav.device) for k, v in sizes.items()}
    if lengths is not None:
        lengths = lengths.to(wav.device)
    opt = lambda k: buf[k].data_ptr() if optional else None
    _hip.check(lib.mv_vad_energy_f32(ctypes.byref(c), wav.data_ptr(), wav.stride(0), _hip._ptr(lengths), B, L, buf['num_frames'].data_ptr(), buf['num_runs'].data_ptr(),
                                     buf['runs'].data_ptr(), max_runs, opt('log_energy'), opt('threshold'), opt('decisions'), buf['ws'].data_ptr(), need,
                                     stream if stream is not None else _hip.current_stream(wav)), lib)
    host = {k: v.cpu() for k, v in buf.items()}
    for k, v in sizes.items():
        assert bool((host[k][v:] == fill).all()), f'wrote past {k}'
    out = dict(num_frames=host['num_frames'][:4 * B].view(torch.int32), num_runs=host['num_runs'][:4 * B].view(torch.int32),
               runs=host['runs'][:8 * B * max_runs].view(torch.int32).view(B, max_runs, 2), log_energy=host['log_energy'][:8 * B * T].view(torch.float64).view(B, T),
               threshold=host['threshold'][:8 * B].view(torch.float64), decisions=host['decisions'][:B * T].view(B, T))
    for b, k in enumerate(out['num_runs'].tolist()):
        assert bool((out['runs'][b, min(k, max_runs):].view(torch.uint8) == fill).all()), 'pairs behind the run count were written'
        out['runs'][b, min(k, max_runs):] = 0
    return out


def same(a, b, keys=('num_frames', 'num_runs', 'runs', 'log_energy', 'threshold', 'decisions')):
    return all(torch.equal(a[k].contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8)) for k in keys)


def check_no_hidden_state(cdll, device, second_stream=False):
    name = 'batch/recipe'
    rows, cfg, _ = case(name)
    refs = reference(name)
    wav, lengths = device_rows(rows, device)
    ff = raw_call(cdll, wav, lengths, cfg, 0xFF)
    zz = raw_call(cdll, wav, lengths, cfg, 0x00)
    assert same(ff, zz), 'the result depends on what the buffers held'
    assert_against(ff, refs, cfg, '0xFF-filled buffers')
    bare = raw_call(cdll, wav, lengths, cfg, 0xFF, optional=False)   # without the optional outputs: the same runs
    assert same(ff, bare, keys=('num_frames', 'num_runs', 'runs'))
    assert same(raw_call(cdll, wav, lengths, cfg, 0xFF), ff), 'a repeated call gives other bits'
    for b, row in enumerate(rows):   # a row's bits do not depend on the batch it sits in
        T = refs[b]['T']
        one = raw_call(cdll, *device_rows([row], device), cfg, 0xFF)
        assert one['num_frames'].tolist() == [T] and one['num_runs'][0] == ff['num_runs'][b]
        assert torch.equal(one['log_energy'][0, :T].view(torch.int64), ff['log_energy'][b, :T].view(torch.int64)), b
        assert torch.equal(one['threshold'].view(torch.int64), ff['threshold'][b:b + 1].view(torch.int64)), b
        assert torch.equal(one['decisions'][0, :T], ff['decisions'][b, :T]) and torch.equal(one['runs'][0, :len(refs[b]['runs'])], ff['runs'][b, :len(refs[b]['runs'])])
    if second_stream:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            other = raw_call(cdll, wav, lengths, cfg, 0xFF, stream=side.cuda_stream)
        side.synchronize()
        assert same(other, ff), 'another stream gives other bits'


def check_refusals(cdll, device):
    """a refusal is a returned status with a message that names the limit; nothing is launched, nothing is written"""
    from mvector import _hip
    lib = cdll or _hip.lib()
    msg = lambda: lib.mv_last_error().decode()
    B, L = 2, 2000
    wav = torch.zeros((B, L), dtype=torch.float32, device=device)
    T = num_frames_of(L, DEFAULT)
    out = torch.full((4096,), 0x5A, dtype=torch.uint8, device=device)
    good = _hip.vad_cfg()
    need = int(lib.mv_vad_energy_workspace_bytes(ctypes.byref(good), B, L))
    assert need > 0
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=device)
    p = out.data_ptr()

    def call(cfg=good, wav_ptr=wav.data_ptr(), stride=L, B=B, L=L, nf=p, nr=p + 64, runs=p + 128, max_runs=(T + 1) // 2, ws_ptr=ws.data_ptr(), nbytes=need):
        return lib.mv_vad_energy_f32(None if cfg is None else ctypes.byref(cfg), wav_ptr, stride, None, B, L, nf, nr, runs, max_runs, None, None, None, ws_ptr, nbytes,
                                     _hip.current_stream(wav))
    assert call(cfg=None) == -1 and 'null cfg' in msg()
    for null in ('wav_ptr', 'nf', 'nr', 'runs'):
        assert call(**{null: None}) == -1 and 'null tensor' in msg(), null
    assert call(ws_ptr=None) == -1 and 'null workspace' in msg()
    assert call(B=-1) == -1 and 'negative B or L' in msg()
    assert call(L=-1) == -1 and 'negative B or L' in msg()
    assert call(max_runs=-1) == -1 and 'negative max_runs' in msg()
    assert call(stride=L - 1) == -1 and 'wav_stride below L' in msg()
    assert call(nbytes=need - 1) == -4 and 'workspace smaller' in msg()
    bad_cfgs = [(dict(frame_shift=0), 'frame sizes outside'), (dict(frame_shift=401), 'frame sizes outside'), (dict(frame_length=4097, frame_shift=160), 'frame sizes outside'),
                (dict(frames_context=-1), 'frames_context outside 0 .. 64'), (dict(frames_context=65), 'frames_context outside 0 .. 64')]
    bad_cfgs += [({field: value}, 'non-finite') for field in ('energy_threshold', 'energy_mean_scale', 'proportion_threshold', 'scale')
                 for value in (math.nan, math.inf, -math.inf)]
    for fields, fragment in bad_cfgs:
        c = _hip.vad_cfg(**fields)
        assert call(cfg=c) == -1 and fragment in msg(), fields
        assert int(lib.mv_vad_energy_workspace_bytes(ctypes.byref(c), B, L)) == 0, fields
    assert call(B=1 << 20, L=1 << 40) == -1 and 'above 2^31 - 1' in msg()
    assert int(lib.mv_vad_energy_workspace_bytes(None, B, L)) == 0 and int(lib.mv_vad_energy_workspace_bytes(ctypes.byref(good), -1, L)) == 0
    assert bool((out == 0x5A).all()) and bool((ws == 0x5A).all()), 'a refused call wrote to its buffers'
    # B = 0: MV_OK, nothing is touched (not even looked at: every pointer may be null)
    assert call(B=0) == 0 and call(B=0, wav_ptr=None, nf=None, nr=None, runs=None, ws_ptr=None, nbytes=0) == 0
    assert bool((out == 0x5A).all()) and bool((ws == 0x5A).all()), 'B = 0 wrote to its buffers'
    empty = _hip.vad_energy(wav[:0], cdll=cdll)
    assert empty['num_frames'].shape == (0,) and empty['runs'].shape == (0, (T + 1) // 2, 2)
    assert call() == 0 and bool((out[:8] != 0x5A).any())   # the same arguments unrefused
    with pytest.raises(RuntimeError, match='frames_context outside'):
        _hip.vad_energy(wav, frames_context=65, cdll=cdll)
    with pytest.raises(TypeError, match='unknown configuration field'):
        _hip.vad_energy(wav, frame_len=400, cdll=cdll)
    with pytest.raises(ValueError, match='lengths must have shape'):
        _hip.vad_energy(wav, lengths=torch.tensor([5]), cdll=cdll)
    assert lib.mv_abi_version() == 5


# ------------------------------------------------------------------------------------------------ recordings for the host layers
RAMP = 0.16   # seconds of raised-cosine onset and decay of a burst


def soft_edges(count, sr=16000, ramp=RAMP):
    """envelope of a burst of ``count`` samples: raised-cosine ramps at both ends, as an utterance sets in and dies away.  The frame that holds the
    burst's first samples starts up to frame_length - 1 samples in front of it: with an abrupt edge of full amplitude that frame is speech already
    and a region starts frame_length - frame_shift samples earlier than one frame shift accounts for; under a ramp the first frames over the
    threshold are the ones that lie well inside the burst."""
    k = min(int(ramp * sr), count // 2)
    env = np.ones(count)
    up = 0.5 * (1.0 - np.cos(np.pi * (np.arange(k) + 0.5) / k))
    env[:k], env[count - k:] = up, up[::-1]
    return env


def synthetic_recording(seconds=12.0, sr=16000, seed=7, bursts=((0.8, 2.9), (3.6, 5.2), (6.4, 9.0), (9.7, 11.4))):
    """bursts (start s, end s) of amplitude-modulated noise (3 Hz tremolo, soft edges) over the FLOOR noise floor -> (samples fp32, the bursts)"""
    n = int(seconds * sr)
    rng = np.random.default_rng(seed)
    x = FLOOR * rng.standard_normal(n)
    for st, ed in bursts:
        lo, hi = int(st * sr), int(ed * sr)
        tt = np.arange(hi - lo) / sr
        x[lo:hi] += LOUD * soft_edges(hi - lo, sr) * (1.0 + 0.3 * np.sin(2 * np.pi * 3.0 * tt)) * rng.standard_normal(hi - lo)
    return x.astype(np.float32), list(bursts)


def assert_brackets(segments, bursts, vad):
    """one segment per burst that holds it, each edge within (frames_context + 1) * frame_shift + speech_pad of the burst's"""
    slack = ((vad.cfg['frames_context'] + 1) * vad.cfg['frame_shift'] + vad.speech_pad) / vad.sample_rate + 1e-9
    assert len(segments) == len(bursts), (segments, bursts)
    for seg, (st, ed) in zip(segments, bursts):
        assert seg['start'] <= st and seg['end'] >= ed, (seg, (st, ed))
        assert st - seg['start'] <= slack and seg['end'] - ed <= slack, (seg, (st, ed), slack)
