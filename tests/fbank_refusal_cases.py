"""What mv_fbank_create and the four mv_fbank_forward* entry points refuse, shared by tests/test_fbank_refusals.py (emulator) and
tests/test_gpu_fbank_refusals.py (device).  Every refusal is a host check that returns before any launch; each case names the fields or the call
that are wrong, the error code and a fragment of the message (include/mvector_hip.h: MV_ERR_*; csrc/fbank.hip: check_cfg, mv_fbank_create,
fbank_forward).  The fields are those of MvFbankCfg on top of mv_fbank_default_cfg with 80 bins."""
import ctypes

import torch

from mvector import _hip

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -3, -4

BAND = 'bad band'
ENERGY = 'use_energy / raw_energy / htk_compat are 0 or 1'
VTLN = 'bad VTLN options'
WINDOW = 'only frame lengths of 2 .. 512 samples'

# (id, MvFbankCfg fields -- or which argument is null --, code, message fragment)
CREATE_CASES = [
    ('null_cfg', 'cfg', INVALID, 'mv_fbank_create: null argument'),
    ('null_out', 'out', INVALID, 'mv_fbank_create: null argument'),
    ('shift_below_one_sample', dict(frame_shift_ms=0.05), INVALID, 'frame shift must be at least one sample'),
    ('bins_3', dict(num_mel_bins=3), INVALID, 'num_mel_bins must be in [4, 128]'),
    ('bins_129', dict(num_mel_bins=129), INVALID, 'num_mel_bins must be in [4, 128]'),
    ('band_low_negative', dict(low_freq=-1.0), INVALID, BAND),
    ('band_low_at_nyquist', dict(low_freq=8000.0), INVALID, BAND),
    ('band_high_zero_from_nyquist', dict(high_freq=-8000.0), INVALID, BAND),
    ('band_high_above_nyquist', dict(high_freq=8100.0), INVALID, BAND),
    ('band_low_above_high', dict(low_freq=7700.0, high_freq=-400.0), INVALID, BAND),
    ('window_1_sample', dict(frame_length_ms=0.1), UNSUPPORTED, WINDOW),
    ('window_513_samples', dict(sample_frequency=1000.0, frame_length_ms=513.0, frame_shift_ms=100.0), UNSUPPORTED, WINDOW),
    ('window_type_5', dict(window_type=5), INVALID, 'unknown window_type'),
    ('window_type_negative', dict(window_type=-1), INVALID, 'unknown window_type'),
    ('kernel_3', dict(kernel=3), INVALID, 'unknown kernel selector'),
    ('min_duration_negative', dict(min_duration=-0.1), INVALID, 'negative min_duration'),
    ('preemphasis_above_1', dict(preemphasis_coefficient=1.5), INVALID, 'preemphasis_coefficient must be in [0, 1]'),
    ('preemphasis_negative', dict(preemphasis_coefficient=-0.1), INVALID, 'preemphasis_coefficient must be in [0, 1]'),
    ('vtln_warp_zero', dict(vtln_warp=0.0), INVALID, 'vtln_warp must be positive'),
    ('vtln_warp_negative', dict(vtln_warp=-1.0), INVALID, 'vtln_warp must be positive'),
    ('use_energy_2', dict(use_energy=2), INVALID, ENERGY),
    ('raw_energy_negative', dict(raw_energy=-1), INVALID, ENERGY),
    ('htk_compat_2', dict(htk_compat=2), INVALID, ENERGY),
    ('energy_floor_negative', dict(energy_floor=-1.0), INVALID, ENERGY),
    ('min_samples_negative', dict(min_samples=-1), INVALID, 'negative min_samples'),
    ('vtln_low_below_the_band', dict(vtln_warp=1.1, vtln_low=10.0), INVALID, VTLN),
    ('vtln_high_below_vtln_low', dict(vtln_warp=0.9, vtln_high=-7950.0), INVALID, VTLN),
    ('vtln_high_at_the_band_edge', dict(vtln_warp=1.1, vtln_high=8000.0), INVALID, VTLN),
    ('tile_kernel_on_40_bins', dict(num_mel_bins=40, kernel=2), UNSUPPORTED, 'fbank_tile_kernel is instantiated'),
    # two wrong fields: the check that comes first wins
    ('bins_before_window_type', dict(num_mel_bins=3, window_type=9), INVALID, 'num_mel_bins must be in [4, 128]'),
    ('window_before_kernel', dict(frame_length_ms=40.0, kernel=7), UNSUPPORTED, WINDOW),
    ('min_duration_before_preemphasis', dict(min_duration=-1.0, preemphasis_coefficient=1.5), INVALID, 'negative min_duration'),
    ('energy_flags_before_min_samples', dict(use_energy=2, min_samples=-1), INVALID, ENERGY),
    ('min_samples_before_vtln_cutoffs', dict(min_samples=-1, vtln_warp=1.1, vtln_low=10.0), INVALID, 'negative min_samples'),
]

ENERGY_WS = 'use_energy writes the mel columns to the caller workspace first'
MIRROR_WS = 'snip_edges=False writes the mirrored signal to the caller workspace'

# (id, MvFbankCfg fields of the handle, the call, code, message fragment).  The call: entry = the exported forward; B, L; null = the argument
# passed as a null pointer; stride = wav_stride - L; ws = 'full' (mv_fbank_workspace_bytes), 'short' (one byte less), 'misaligned' (4 bytes off a
# 16-byte boundary).  A returned MV_OK must have left the output untouched.
FORWARD_CASES = [
    ('null_handle', {}, dict(entry='forward_ws', null='handle'), INVALID, 'mv_fbank_forward: null handle'),
    ('null_handle_varlen', {}, dict(entry='forward_varlen', null='handle'), INVALID, 'mv_fbank_forward: null handle'),
    ('stride_below_L', {}, dict(entry='forward', stride=-1), INVALID, 'bad batch geometry'),
    ('negative_B', {}, dict(entry='forward', B=-1), INVALID, 'bad batch geometry'),
    ('null_wav', {}, dict(entry='forward', null='wav'), INVALID, 'mv_fbank_forward: null buffer'),
    ('null_out', {}, dict(entry='forward_ws', null='out', ws='full'), INVALID, 'mv_fbank_forward: null buffer'),
    ('null_lengths', {}, dict(entry='forward_varlen', null='lens'), INVALID, 'mv_fbank_forward_varlen: null length array'),
    ('null_lengths_ws', {}, dict(entry='forward_varlen_ws', null='lens', ws='full'), INVALID, 'mv_fbank_forward_varlen_ws: null length array'),
    ('use_energy_without_workspace', dict(use_energy=1), dict(entry='forward'), WORKSPACE, ENERGY_WS),
    ('use_energy_varlen_without_workspace', dict(use_energy=1), dict(entry='forward_varlen'), WORKSPACE, ENERGY_WS),
    ('use_energy_workspace_one_byte_short', dict(use_energy=1), dict(entry='forward_ws', ws='short'), WORKSPACE, ENERGY_WS),
    ('use_energy_workspace_misaligned', dict(use_energy=1), dict(entry='forward_ws', ws='misaligned'), WORKSPACE, ENERGY_WS),
    ('mirror_without_workspace', dict(snip_edges=0), dict(entry='forward'), WORKSPACE, MIRROR_WS),
    ('mirror_workspace_one_byte_short', dict(snip_edges=0), dict(entry='forward_varlen_ws', ws='short'), WORKSPACE, MIRROR_WS),
    ('mirror_workspace_misaligned', dict(snip_edges=0), dict(entry='forward_ws', ws='misaligned'), WORKSPACE, MIRROR_WS),
    ('use_energy_wins_over_mirror', dict(use_energy=1, snip_edges=0), dict(entry='forward'), WORKSPACE, ENERGY_WS),
    ('too_short_to_mirror', dict(snip_edges=0), dict(entry='forward_ws', L=100, ws='full'), INVALID, 'the signal is too short to be mirrored over its frames'),
    # returns that are not refusals
    ('no_rows', {}, dict(entry='forward', B=0), OK, ''),
    ('no_rows_null_buffers', dict(use_energy=1, snip_edges=0), dict(entry='forward', B=0, null='wav'), OK, ''),
    ('no_frames', {}, dict(entry='forward_ws', L=399, ws='full'), OK, ''),
    ('no_frames_without_workspace', dict(use_energy=1, snip_edges=0), dict(entry='forward_varlen', L=79), OK, ''),
]


def default_cfg(cdll, fields):
    cfg = _hip.MvFbankCfg()
    cdll.mv_fbank_default_cfg(ctypes.byref(cfg))
    cfg.num_mel_bins = 80
    for k, v in fields.items():
        setattr(cfg, k, v)
    return cfg


def last_error(cdll):
    return cdll.mv_last_error().decode(errors='replace')


def create(cdll, fields):
    """(code, message, handle): mv_fbank_create on the case's fields or null argument"""
    h = _hip.c_vp()
    if fields == 'cfg':
        rc = cdll.mv_fbank_create(None, ctypes.byref(h))
    elif fields == 'out':
        rc = cdll.mv_fbank_create(ctypes.byref(default_cfg(cdll, {})), None)
    else:
        rc = cdll.mv_fbank_create(ctypes.byref(default_cfg(cdll, fields)), ctypes.byref(h))
    return rc, last_error(cdll) if rc != OK else '', h


def forward(cdll, device, fields, call):
    """(code, message, output untouched): one forward of a handle created from `fields`.  The buffers are real (a sentinel fills the output), so a
    call that did launch would be seen."""
    rc, msg, h = create(cdll, fields)
    assert rc == OK, msg
    try:
        B, L = call.get('B', 2), call.get('L', 2000)
        rows = max(B, 1)
        wav = torch.zeros(rows, L, device=device)
        T = _hip.c_i64()
        assert cdll.mv_fbank_num_frames(h, L, ctypes.byref(T)) == OK
        out = torch.full((rows, max(T.value, 1), 81), 7.0, device=device)
        lens = torch.full((rows,), L, dtype=torch.int64, device=device)
        ratio = torch.ones(rows, device=device)
        need = ctypes.c_size_t()
        assert cdll.mv_fbank_workspace_bytes(h, B, L, ctypes.byref(need)) == OK
        buf = torch.zeros(need.value + 32, dtype=torch.uint8, device=device)
        assert buf.data_ptr() % 16 == 0
        ws = {None: (None, 0), 'full': (buf.data_ptr(), need.value), 'short': (buf.data_ptr(), need.value - 1),
              'misaligned': (buf.data_ptr() + 4, need.value)}[call.get('ws')]
        if call.get('ws') == 'short':
            assert need.value > 0
        null = call.get('null')
        varlen = 'varlen' in call['entry']
        third = lens if varlen else ratio
        args = [None if null == 'handle' else h, None if null == 'wav' else wav.data_ptr(), B, L, L + call.get('stride', 0),
                None if null == 'lens' else third.data_ptr(), None if null == 'out' else out.data_ptr()]
        if call['entry'].endswith('_ws'):
            args += [ws[0], ws[1]]
        rc = getattr(cdll, 'mv_fbank_' + call['entry'])(*args, None)
        return rc, last_error(cdll) if rc != OK else '', bool((out == 7.0).all())
    finally:
        cdll.mv_fbank_destroy(h)


def check_create(cdll, idx):
    name, fields, code, fragment = CREATE_CASES[idx]
    rc, msg, h = create(cdll, fields)
    assert (rc, h.value) == (code, None) and fragment in msg, (name, rc, msg)


def check_forward(cdll, device, idx):
    name, fields, call, code, fragment = FORWARD_CASES[idx]
    rc, msg, untouched = forward(cdll, device, fields, call)
    assert rc == code and fragment in msg and untouched, (name, rc, msg, untouched)
