"""Checks of the Res2Net kernels (csrc/res2net2d.hip) and handle that the emulator suite (tests/test_res2net.py) and the device suite
(tests/test_gpu_res2net.py) share: each takes the bound library `cdll` and the torch device `dev` its buffers live on.  Maps come from
resnet_se_checks.make_map (both signs).

Bars (none comes from what the kernels give):
  max-pool   the merged output equals torch's max_pool2d of the merged input exactly, and every output (hi, lo) pair is an input pair of its window;
  avg-pool   the gate's bar of resnet_se_checks (rtol 2^-20 + atol 2^-29) against the S16 round trip of torch's fp32 avg_pool2d of the merged input:
             the kernel makes the same single rounding into S16 after an fp32 sum of nine terms.  The error against avg_pool2d in fp64 is printed
             next to that of torch's fp32 result and held to four times it plus the S16 format term;
  stem       max-abs error against fp64 at most 4 x that of torch's fp32 evaluation of the same layer (the factor of check_squeeze / check_excite:
             it covers another summation order) plus the S16 format term 2^-22 |v| + 2^-31.
"""
import ctypes
import functools

import torch
import torch.nn.functional as F

import resnet_se_checks as se
from helpers import cos_dist, load_case
from mvector import _hip

GOLDENS = ['res2net_tiny_asp', 'res2net_tiny_sap', 'res2net_tiny_tap', 'res2net_tiny_tsp', 'res2net_tiny_s4', 'res2net_tiny_s1', 'res2net_default']
# (B, H, W, C, ld): one pixel; odd sizes; even H, odd W and a padded unit; padding inside a unit; the default stem's map
POOL_SHAPES = [(2, 1, 1, 16, 16), (2, 5, 9, 16, 32), (3, 8, 41, 32, 48), (2, 6, 10, 40, 64), (1, 26, 98, 32, 32)]
# (B, T, F, C): one output pixel; two by one; padded channels; the default stem
STEM_SHAPES = [(2, 5, 5, 16), (2, 7, 8, 16), (3, 41, 16, 24), (1, 98, 80, 32)]
S16_RTOL, S16_ATOL = 2.0 ** -22, 2.0 ** -31   # the format's own round trip (split -> merge of an fp32 value)
np_bits, merge, split, make_map, _st = se.np_bits, se.merge, se.split, se.make_map, se._st


def pool_out(n, stride):
    return (n - 1) // stride + 1


def stem_out(n):
    return (n - 5) // 3 + 1


def maxpool(cdll, m, C, y=None):
    B, H, W, ld = m.shape
    if y is None:
        y = torch.full((B, pool_out(H, 2), pool_out(W, 2), ld), float('nan'), device=m.device)
    _hip.check(cdll.mv_maxpool3s2_s16(m.data_ptr(), ld, y.data_ptr(), y.shape[-1], B, H, W, C, _st(m)), cdll)
    return y


def avgpool(cdll, m, C, stride, y=None, unit=0):
    """unit: x and y are the slices at 16-channel unit `unit` of the maps m and y"""
    B, H, W, ld = m.shape
    if y is None:
        y = torch.full((B, pool_out(H, stride), pool_out(W, stride), ld), float('nan'), device=m.device)
    _hip.check(cdll.mv_avgpool3_s16(m.data_ptr() + unit * 64, ld, y.data_ptr() + unit * 64, y.shape[-1], B, H, W, C, stride, _st(m)), cdll)
    return y


def stem(cdll, x, w, b, peak=None):
    B, T, Fq = x.shape
    C = w.shape[0]
    y = torch.full((B, stem_out(Fq), stem_out(T), (C + 15) // 16 * 16), float('nan'), device=x.device)
    w = w.reshape(C, 49).contiguous()
    if peak is None:
        _hip.check(cdll.mv_conv2d_stem7_s16(x.data_ptr(), y.data_ptr(), w.data_ptr(), b.data_ptr(), B, T, Fq, C, _st(x)), cdll)
    else:
        _hip.check(cdll.mv_conv2d_stem7_peak_s16(x.data_ptr(), y.data_ptr(), w.data_ptr(), b.data_ptr(), B, T, Fq, C, peak.data_ptr(), _st(x)), cdll)
    return y


def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def check_padding(raw, C, ld, untouched_nan=True):
    """the kernel owns the channels 0 .. round_up(C, 16): zero bits (both halves) in C .. round_up(C, 16), and nothing beyond"""
    C16 = (C + 15) // 16 * 16
    lead = raw.shape[:-1]
    for u in range(C // 16, C16 // 16):
        halves = raw[..., 16 * u:16 * u + 16].contiguous().view(torch.int16).reshape(*lead, 2, 16)
        assert torch.count_nonzero(halves[..., C - 16 * u:]) == 0
    if ld > C16 and untouched_nan:
        assert torch.isnan(raw[..., C16:]).all()


# ------------------------------------------------------------------------------------------------ per kernel

def check_maxpool(cdll, dev, shape):
    B, H, W, C, ld = shape
    m, x = make_map(cdll, dev, B, H, W, C, ld, seed=sum(shape))
    y = maxpool(cdll, m, C)
    C16 = (C + 15) // 16 * 16
    got = merge(cdll, y).cpu()[..., :C16]
    expected = _nhwc(F.max_pool2d(_nchw(x[..., :C16]), 3, 2, 1))
    assert got.shape == expected.shape
    err = (got - expected).abs().max().item()
    print(f'maxpool {shape}: max-abs {err}')
    assert err == 0.0
    assert (expected < 0).any() or H * W == 1   # a window of negatives only: the padding took no part
    check_padding(y.cpu(), C, ld)
    # the output bits are input bits: pixel (ho, wo) holds, per channel, the 32-bit (hi, lo) pair of one of its window's pixels
    raw_in = m.cpu().contiguous().view(torch.int16).reshape(B, H, W, ld // 16, 2, 16)
    raw_out = y.cpu().contiguous().view(torch.int16).reshape(B, got.shape[1], got.shape[2], ld // 16, 2, 16)[:, :, :, :C16 // 16]
    found = torch.zeros(raw_out.shape[:4] + (16,), dtype=torch.bool)
    for dh in range(3):
        for dw in range(3):
            for ho in range(got.shape[1]):
                h = 2 * ho - 1 + dh
                if not 0 <= h < H:
                    continue
                for wo in range(got.shape[2]):
                    w = 2 * wo - 1 + dw
                    if 0 <= w < W:
                        found[:, ho, wo] |= (raw_in[:, h, w, :C16 // 16] == raw_out[:, ho, wo]).all(dim=-2)
    assert found.all()
    return err


def check_avgpool(cdll, dev, shape, stride):
    B, H, W, C, ld = shape
    m, x = make_map(cdll, dev, B, H, W, C, ld, seed=sum(shape) + stride)
    y = avgpool(cdll, m, C, stride)
    C16 = (C + 15) // 16 * 16
    got = merge(cdll, y).cpu()[..., :C16]
    ref64 = _nhwc(F.avg_pool2d(_nchw(x[..., :C16]).double(), 3, stride, 1))
    t32 = _nhwc(F.avg_pool2d(_nchw(x[..., :C16]), 3, stride, 1))
    assert got.shape == t32.shape
    full = torch.zeros(t32.shape[:3] + (ld,))
    full[..., :C16] = t32
    expected = merge(cdll, split(cdll, full.to(dev))).cpu()[..., :C16]
    diff = (got.double() - expected.double()).abs()
    bound = se.GATE_RTOL * expected.double().abs() + se.GATE_ATOL
    err, err_torch = (got.double() - ref64).abs().max().item(), (t32.double() - ref64).abs().max().item()
    print(f'avgpool {shape} stride {stride}: largest error / bound {(diff / bound).max().item():.3f}  against fp64: kernel {err:.2e}  torch fp32 {err_torch:.2e}')
    assert (diff <= bound).all(), (diff / bound).max().item()
    assert err <= 4.0 * err_torch + (S16_RTOL * ref64.abs().max().item() + S16_ATOL), (err, err_torch)
    check_padding(y.cpu(), C, ld)
    return err, err_torch


def check_avgpool_slice(cdll, dev, stride):
    """x = unit 1 of a map of 48 channels, y = unit 1 of a map of 64: 12 channels averaged, the other units of y keep their NaN fill"""
    B, H, W, C = 2, 5, 9, 12
    m, x = make_map(cdll, dev, B, H, W, 48, 48, seed=77 + stride)
    y = torch.full((B, pool_out(H, stride), pool_out(W, stride), 64), float('nan'), device=dev)
    avgpool(cdll, m, C, stride, y=y, unit=1)
    raw = y.cpu()
    assert torch.isnan(raw[..., :16]).all() and torch.isnan(raw[..., 32:]).all()
    unit = torch.zeros_like(raw)
    unit[..., 16:32] = raw[..., 16:32]
    got = merge(cdll, unit.to(dev)).cpu()[..., 16:32]
    t32 = _nhwc(F.avg_pool2d(_nchw(x[..., 16:16 + C]), 3, stride, 1))
    full = torch.zeros(t32.shape[:3] + (16,))
    full[..., :C] = t32
    expected = merge(cdll, split(cdll, full.to(dev))).cpu()
    diff = (got.double() - expected.double()).abs()
    assert (diff <= se.GATE_RTOL * expected.double().abs() + se.GATE_ATOL).all()
    assert expected[..., :C].abs().max() > 0.1
    check_padding(raw[..., 16:32].contiguous(), C, 16)


def stem_inputs(shape):
    B, T, Fq, C = shape
    g = torch.Generator().manual_seed(sum(shape))
    return torch.randn(B, T, Fq, generator=g) * 2.0, torch.randn(C, 1, 7, 7, generator=g) / 7.0, torch.randn(C, generator=g) * 0.3


def check_stem(cdll, dev, shape):
    B, T, Fq, C = shape
    x, w, b = stem_inputs(shape)

    def f(t):
        return torch.relu(F.conv2d(t(x).transpose(2, 1).unsqueeze(1), t(w), t(b), stride=3, padding=1))
    ref = _nhwc(f(lambda v: v.double()))
    y = stem(cdll, x.to(dev), w.to(dev), b.to(dev))
    got = merge(cdll, y).cpu()
    assert got.shape[:3] == ref.shape[:3] and got.shape[3] == (C + 15) // 16 * 16
    err = (got[..., :C].double() - ref).abs().max().item()
    err_torch = (_nhwc(f(lambda v: v)).double() - ref).abs().max().item()
    fmt = S16_RTOL * ref.abs().max().item() + S16_ATOL
    print(f'stem {shape}: kernel {err:.2e}  torch fp32 {err_torch:.2e}  format term {fmt:.2e}')
    assert err_torch > 0.0 and (ref == 0).float().mean() > 0.2 and (ref > 0).float().mean() > 0.2
    assert err <= 4.0 * err_torch + fmt, (err, err_torch, fmt)
    check_padding(y.cpu(), C, got.shape[3])
    return err, err_torch


def check_stem_peak(cdll, dev):
    """weights 1, bias 0 on features of 40: the one output pixel of a 5 x 5 input sums its 25 taps inside the map, 1000, and the second map twice
    that: the word reports 64 * 2000 = 128000 (before the clamp), the map holds 1000 and the clamped 1023.5"""
    x = torch.full((1, 5, 5), 40.0)
    w = torch.ones(16, 1, 7, 7)
    w[1] = 2.0
    peak = torch.zeros(1, dtype=torch.int32, device=dev)
    y = stem(cdll, x.to(dev), w.to(dev), torch.zeros(16, device=dev), peak=peak)
    word = peak.cpu().view(torch.float32).item()
    assert word == 128000.0 and word > 65504.0
    got = merge(cdll, y).cpu().flatten()
    assert got[0] == 1000.0 and got[1] == 65504.0 / 64 and (got[2:] == 1000.0).all()
    peak.zero_()
    stem(cdll, (x / 40).to(dev), w.to(dev), torch.zeros(16, device=dev), peak=peak)
    assert peak.cpu().view(torch.float32).item() == 64 * 50.0


def check_batch_independence(cdll, dev):
    B, H, W, C, ld = 3, 8, 41, 32, 48
    m, _ = make_map(cdll, dev, B, H, W, C, ld, seed=1)
    full = [maxpool(cdll, m, C), avgpool(cdll, m, C, 1), avgpool(cdll, m, C, 2)]
    x, w, b = (t.to(dev) for t in stem_inputs((3, 41, 16, 24)))
    s_full = stem(cdll, x, w, b)
    for i in range(B):
        mi = m[i:i + 1].contiguous()
        alone = [maxpool(cdll, mi, C), avgpool(cdll, mi, C, 1), avgpool(cdll, mi, C, 2)]
        for a, f in zip(alone, full):
            assert (np_bits(a) == np_bits(f[i:i + 1])).all()
        assert (np_bits(stem(cdll, x[i:i + 1].contiguous(), w, b)) == np_bits(s_full[i:i + 1])).all()


# ------------------------------------------------------------------------------------------------ the handle

@functools.lru_cache(maxsize=None)
def case(name):
    return load_case(name)


def module(man, sd):
    from mvector.models.res2net import Res2Net
    m = Res2Net(**man['kwargs'])
    m.load_state_dict(sd, strict=True)
    return m.eval()


def handle(cdll, dev, name, edit=None):
    man, sd, x, emb, _ = case(name)
    sd = {k: v.to(dev) for k, v in sd.items()}
    if edit:
        edit(sd)
    return _hip.Model('res2net', module(man, case(name)[1])._native_cfg(), sd, cdll=cdll), x.to(dev), emb


def check_golden(cdll, dev, name):
    h, x, emb = handle(cdll, dev, name)
    d = cos_dist(h.forward(x).cpu(), emb).max().item()
    rng = h.s16_range()
    print(f'{name}: 1 - cos {d:.2e}  peak {rng["peak"]:.1f}')
    assert d <= 1e-4, d
    assert not rng['saturated']
    return d


def tiny_cfg(**over):
    """MvRes2NetCfg of the res2net_tiny_* goldens with fields replaced"""
    c = _hip.MvRes2NetCfg()
    f = dict(input_size=32, m_channels=16, layers=[1, 1, 1, 1], base_width=32, scale=2, embd_dim=64, pooling_type=_hip.MV_POOL_ASP)
    f.update(over)
    for k, v in f.items():
        if isinstance(v, list):
            for i in range(4):
                getattr(c, k)[i] = v[i]
        else:
            setattr(c, k, v)
    return c


def create_rc(cdll, cfg, sd):
    """mv_res2net_create on a state_dict -> (return code, message); a handle that came to life is released"""
    refs, tensors, _ = _hip._tensor_refs(sd)
    h = ctypes.c_void_p()
    rc = cdll.mv_res2net_create(ctypes.byref(cfg), refs, len(tensors), ctypes.byref(h))
    msg = cdll.mv_last_error().decode() if rc else ''
    if h.value:
        cdll.mv_model_destroy(h)
    return rc, msg
