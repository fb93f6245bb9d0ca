"""Cases, checks and bars shared by tests/test_hf_varlen.py (emulator) and tests/test_gpu_hf_varlen.py (device): the variable-length form of the
HuggingFace front-end, mv_hfenc_forward_varlen.

The yardstick of the bit-identity checks is the unchanged fixed-length forward of the same handle on the row alone (its distance to the fp64
arbiter is the subject of tests/test_hf_frontend.py / tests/test_gpu_hf_frontend.py).  The lengths sit where the per-row code can go wrong, on
the base geometry (kernels 10, 3, 3, 3, 3, 2, 2, strides 5, 2, 2, 2, 2, 2, 2; frame counts by hf_cases.frames_of):

    n       frames                  what it exercises
    0       none                    no sample, no division
    399     T0 = 78, T' = 0         an all-zero row although layer 0 has frames
    400     T0 = 79, T' = 1         one frame (minus its own mean it is zero: compared without the time mean as well)
    404/405 T0 = 79 / 80            frame boundary of layer 0
    645/650 T0 = 128 / 129          exactly one GroupNorm chunk / one frame into the second
    720     T' = 2                  time mean over two frames, fewer than its four phases
    1300    T0 = 259, T' = 3        the full row (= L), three chunks
    1400/-5                         clamped to L and to 0

Arbiter bars -- as in hf_cases.py: MODEL_DISTANCE holds the distance of the rounding model (hf_ref, fp32 with the fp16 sites of the device path)
from the fp64 arbiter, measured on the CPU on exactly the row the test compares (`python tests/hf_varlen_cases.py` prints the table); the bar is
TWICE that, max-abs and mean-abs."""
import torch

import hf_cases as hc
import hf_ref
from oracle import frontend

# ---- emulator: width 64 (the fixtures' weights), L = 1300 ----
EMU_L = 1300
EMU_LENS = [0, 399, 400, 404, 405, 645, 650, 720, 1300, 1400, -5]
EMU_T0 = {399: 78, 400: 79, 404: 79, 405: 80, 645: 128, 650: 129, 1300: 259}   # frames behind layer 0
EMU_TL = {399: 0, 400: 1, 720: 2, 1300: 3}                                     # frames of the output
BATCH_ROWS = (2, 6, 8)    # n = 400, 650, 1300: the rows of the B = 1 against whole-batch comparison

# ---- emulator, width 512: B = 2, L = 800 (the C == 512 form of hf_rows_kernel) ----
W512_L = 800
W512_LENS = [800, 405]

# ---- device: width 512, L = 4000; 2565 -> T0 = 512, exactly four chunks; 2570 -> T0 = 513, one frame into the fifth ----
GPU_L = 4000
GPU_LENS = [4000, 400, 399, 0, 2565, 2570, 404, 405]
GPU_ARBITER_ROWS = (0, 4)
MANY_B = 130


def emu_batch(name):
    """(cfg, sd, wav [11, 1300]) of a fixture: the first 1300 samples of its three waveforms, tiled to one row per length"""
    cfg, sd, wav, _ = hc.load_fixture(name)
    rows = [wav[b % wav.shape[0], :EMU_L] for b in range(len(EMU_LENS))]
    return cfg, sd, torch.stack(rows).float().contiguous()


def w512_batch(norm):
    cfg, sd = hc.seeded_model(norm)
    return cfg, sd, frontend.synth_waveforms(len(W512_LENS), W512_L, seed=11).float().contiguous()


def gpu_batch(norm):
    cfg, sd = hc.seeded_model(norm)
    return cfg, sd, frontend.synth_waveforms(len(GPU_LENS), GPU_L, seed=21).float().contiguous()


def many_batch():
    """(wav [130, 4000], lengths): seeded uniform lengths in [0, 4000]"""
    g = torch.Generator().manual_seed(17)
    lens = torch.randint(0, GPU_L + 1, (MANY_B,), generator=g).tolist()
    return frontend.synth_waveforms(MANY_B, GPU_L, seed=23).float().contiguous(), lens


def many_rows(lens):
    """the rows of the many-row case that are compared with the row alone: the shortest non-zero row, the longest and ten seeded rows"""
    field = hf_ref.receptive_field(hc.BASE)
    live = [b for b, n in enumerate(lens) if n >= field]
    g = torch.Generator().manual_seed(19)
    picks = [live[i] for i in torch.randperm(len(live), generator=g)[:10].tolist()]
    return sorted({min(live, key=lambda b: lens[b]), max(live, key=lambda b: lens[b]), *picks})


def clamp(n, L):
    return min(max(int(n), 0), L)


def with_tail(wav, lens, value):
    """a copy of wav with wav[b, n_b:] = value"""
    out = wav.clone()
    for b, n in enumerate(lens):
        out[b, clamp(n, wav.shape[1]):] = value
    return out


def check_rows(h, wav, lens, rows=None, out=None):
    """h(wav, None, lens)[b, :T_b] has the bits of h(wav[b:b+1, :n_b])[0] and is zero behind T_b, for every row of `rows` (default: all).
    Returns the whole-batch output."""
    B, L = wav.shape
    if out is None:
        out = h(wav, None, torch.tensor(lens, dtype=torch.int64, device=wav.device))
    assert out.shape == (B, h.num_frames(L), h.dim) and out.dtype == torch.float32 and out.device == wav.device
    for b in (range(B) if rows is None else rows):
        nb = clamp(lens[b], L)
        Tb = max(h.num_frames(nb), 0)
        if Tb > 0:
            alone = h(wav[b:b + 1, :nb])[0]
            assert alone.shape[0] == Tb
            assert torch.equal(out[b, :Tb], alone), f'row {b} (n = {lens[b]}): {(out[b, :Tb] - alone).abs().max().item():.3e} off the row alone'
        assert bool((out[b, Tb:] == 0).all()), f'row {b} (n = {lens[b]}): not zero behind frame {Tb}'
    return out


def arbiter_row(cfg, sd, wav, lens, b, dtype=torch.float64, fp16_sites=False):
    """hf_ref.featurize on row b alone, cut to its own samples: [T_b, C]"""
    return hf_ref.featurize(sd, cfg, wav[b:b + 1, :clamp(lens[b], wav.shape[1])], None, dtype, fp16_sites)[0]


# measured on the CPU: rounding model vs the fp64 arbiter on the row alone, (max-abs, mean-abs)
# (w512_*_L800_row0 is the input of hf_cases' w512_*_L800: the same max-abs; the mean-abs is twice that case's, whose ratio of 0.5 masks one of
# the two frames to an exact zero on both sides)
MODEL_DISTANCE = {
    'w512_group_L800_row0': (3.505e-03, 5.344e-04),    # fp32 restatement: 3.4e-06 max-abs; n = 800, 2 frames; |ref| max 2.50
    'w512_group_L4000_row0': (6.034e-03, 7.241e-04),   # fp32 restatement: 4.4e-06 max-abs; n = 4000, 12 frames; |ref| max 4.05
    'w512_group_L4000_row4': (6.721e-03, 6.806e-04),   # fp32 restatement: 3.6e-06 max-abs; n = 2565, 7 frames; |ref| max 3.73
    'w512_layer_L800_row0': (3.080e-03, 5.265e-04),    # fp32 restatement: 2.9e-06 max-abs; n = 800, 2 frames; |ref| max 1.76
    'w512_layer_L4000_row0': (6.674e-03, 7.057e-04),   # fp32 restatement: 4.4e-06 max-abs; n = 4000, 12 frames; |ref| max 4.06
    'w512_layer_L4000_row4': (6.501e-03, 7.030e-04),   # fp32 restatement: 3.8e-06 max-abs; n = 2565, 7 frames; |ref| max 3.73
}


def bars(key):
    mx, mean = MODEL_DISTANCE[key]
    return 2.0 * mx, 2.0 * mean


def check_arbiter(key, got_row, cfg, sd, wav, lens, b):
    ref = arbiter_row(cfg, sd, wav, lens, b)
    got_row = got_row[:ref.shape[0]]
    assert got_row.shape == ref.shape and bool(torch.isfinite(got_row).all())
    mx, mean = hc.distances(got_row, ref)
    bmx, bmean = bars(key)
    print(f'{key}: max-abs {mx:.3e} (bar {bmx:.3e}) mean-abs {mean:.3e} (bar {bmean:.3e})')
    assert mx <= bmx and mean <= bmean


def _arbiter_cases():
    for norm in ('group', 'layer'):
        cfg, sd, wav = w512_batch(norm)
        yield f'w512_{norm}_L800_row0', cfg, sd, wav, W512_LENS, 0
        cfg, sd, wav = gpu_batch(norm)
        for b in GPU_ARBITER_ROWS:
            yield f'w512_{norm}_L4000_row{b}', cfg, sd, wav, GPU_LENS, b


if __name__ == '__main__':
    for n, t in EMU_T0.items():
        assert hc.frames_of(n)[0] == t, n
    for n, t in EMU_TL.items():
        assert max(hf_ref.num_frames(hc.BASE, n), 0) == t, n
    assert hc.frames_of(2565)[0] == 512 and hc.frames_of(2570)[0] == 513
    for key, cfg, sd, wav, lens, b in _arbiter_cases():
        ref = arbiter_row(cfg, sd, wav, lens, b)
        model = arbiter_row(cfg, sd, wav, lens, b, torch.float32, True)
        f32 = arbiter_row(cfg, sd, wav, lens, b, torch.float32)
        mx, mean = hc.distances(model, ref)
        print(f"    '{key}': ({mx:.3e}, {mean:.3e}),   # fp32 restatement: {hc.distances(f32, ref)[0]:.1e} max-abs; n = {lens[b]}, "
              f'{ref.shape[0]} frames; |ref| max {ref.abs().max():.2f}')
