"""The down-mix + polyphase resampler without a GPU: the kernels of csrc/resample.hip on the emulator build against scipy in fp64 and the host's
channel mean, the filter table against scipy.signal.firwin, and the host pieces (read_pcm16_frames, the predictor's grouping).  The same kernel
checks run on the device in tests/test_gpu_resample.py (tests/resample_checks.py holds them)."""
import io

import numpy as np
import pytest

import resample_checks as rc


@pytest.fixture(scope='module')
def emu():
    import emu_lib
    return emu_lib.emu_cdll()


@pytest.mark.parametrize('src,dst', rc.FILTER_RATES)
def test_emu_filter_table_is_scipys(emu, src, dst):
    rc.check_filter_table(emu, src, dst)


def test_emu_refusals_by_name(emu):
    rc.check_refusals(emu, 'cpu')


@pytest.mark.parametrize('channels', [2, 3, 8])
def test_emu_downmix_is_the_host_mean_bit_for_bit(emu, channels):
    rc.check_downmix(emu, 'cpu', channels)


@pytest.mark.parametrize('src,dst,channels', rc.RESAMPLE_CASES)
def test_emu_resample_within_the_rounding_bound_of_fp64(emu, src, dst, channels):
    rc.check_resample(emu, 'cpu', src, dst, channels)


def test_emu_normalize(emu):
    rc.check_normalize(emu, 'cpu')


def test_emu_table_in_global_memory_at_an_extreme_ratio(emu):
    rc.check_extreme_ratio(emu, 'cpu')


def test_the_library_exports_the_resampler():
    import ctypes
    import __graft_entry__
    from mvector import _hip
    cdll = ctypes.CDLL(__graft_entry__.build())
    for name in ('mv_resampler_create', 'mv_resampler_destroy', 'mv_resampler_info', 'mv_resampler_taps', 'mv_resampler_out_len',
                 'mv_resampler_workspace_bytes', 'mv_resampler_forward_i16'):
        assert hasattr(cdll, name) and name in _hip.EXPORTED_SYMBOLS, name


# ------------------------------------------------------------------ host pieces
def _wav_bytes(rate, data):
    from scipy.io import wavfile
    buf = io.BytesIO()
    wavfile.write(buf, rate, data)
    return buf.getvalue()


def test_read_pcm16_frames(tmp_path):
    from mvector.data_utils.audio import read_pcm16, read_pcm16_frames
    rng = np.random.default_rng(0)
    stereo = rng.integers(-3000, 3000, size=(500, 2)).astype(np.int16)
    mono = rng.integers(-3000, 3000, size=(300,)).astype(np.int16)
    got, rate = read_pcm16_frames(_wav_bytes(44100, stereo))
    assert rate == 44100 and got.dtype == np.int16 and np.array_equal(got, stereo)
    got, rate = read_pcm16_frames(_wav_bytes(8000, mono))
    assert rate == 8000 and got.shape == (300, 1) and np.array_equal(got[:, 0], mono)
    path = tmp_path / 'a.wav'
    path.write_bytes(_wav_bytes(48000, stereo))
    got, rate = read_pcm16_frames(str(path))
    assert rate == 48000 and np.array_equal(got, stereo)
    assert read_pcm16_frames(_wav_bytes(16000, mono.astype(np.float32) / 32768)) is None      # float WAV
    assert read_pcm16_frames(_wav_bytes(16000, mono.astype(np.int32))) is None                # 32-bit PCM
    assert read_pcm16_frames(b'not a wav file') is None
    assert read_pcm16(_wav_bytes(44100, stereo)) is None and read_pcm16(_wav_bytes(8000, mono))[1] == 8000   # read_pcm16 is what it was


def test_predictor_groups_items_by_rate_and_channels():
    """the host side of predict_batch's resampled path, without a device: which batches take it, the groups, the lengths and the ratios"""
    import types
    from mvector.predict import MVectorPredictor
    p = object.__new__(MVectorPredictor)
    p.configs = types.SimpleNamespace(dataset_conf=types.SimpleNamespace(dataset=types.SimpleNamespace(sample_rate=16000, min_duration=0.3)))
    rng = np.random.default_rng(1)
    mk = lambda rate, n, c: _wav_bytes(rate, rng.integers(-3000, 3000, size=(n, c) if c > 1 else (n,)).astype(np.int16))
    items = [mk(44100, 22050, 2), mk(16000, 9000, 1), mk(8000, 4000, 1), mk(44100, 30000, 2)]
    frames = p._pcm16_frames_batch(items)
    assert [(f.shape, r) for f, r in frames] == [((22050, 2), 44100), ((9000, 1), 16000), ((4000, 1), 8000), ((30000, 2), 44100)]
    groups = p._resample_groups(frames)
    assert {k: [i for i, _ in v] for k, v in groups.items()} == {(44100, 2): [0, 3], (16000, 1): [1], (8000, 1): [2]}
    assert p._resampled_lengths(frames) == [8000, 9000, 8000, 10885]     # ceil(n * up / down)
    assert p._pcm16_frames_batch([mk(16000, 9000, 1), mk(16000, 8000, 1)]) is None                  # all target-rate mono: the pcm16 path, as before
    assert p._pcm16_frames_batch([mk(44100, 22050, 2), np.zeros(16000, dtype=np.float32)]) is None  # an ndarray: the host path
    assert p._pcm16_frames_batch([mk(44100, 22050, 2), _wav_bytes(16000, np.zeros(9000, dtype=np.float32))]) is None   # a float WAV: the host path
    assert p._pcm16_frames_batch([mk(16001, 9000, 1)]) is None                                      # a ratio the library refuses: the host path
    assert p._pcm16_frames_batch([mk(8000, 9000, 9)]) is None                                       # more than 8 channels: the host path
    with pytest.raises(AssertionError, match='音频太短'):
        p._pcm16_frames_batch([mk(44100, 4410, 2)])                                                  # 0.1 s of source audio
