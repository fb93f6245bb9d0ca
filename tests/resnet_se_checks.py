"""Checks of the ResNetSE kernels (csrc/se2d.hip) and handle that the emulator suite (tests/test_resnet_se.py) and the device suite
(tests/test_gpu_resnet_se.py) share: each takes the bound library `cdll` and the torch device `dev` its buffers live on.

Bars (none comes from what the kernels give):
  squeeze / excite   four times the error torch's own fp32 evaluation (CPU) makes against fp64 on the same inputs: the factor covers a
                     different summation order;
  gate               rtol 2^-20 + atol 2^-29 against the S16 round trip of torch's fp32 result: S16 carries 22 bits, and a one-ulp fp32
                     difference (the kernel contracts x * g + res into one fma, torch rounds twice) can flip the last unit of the lo half;
  rows               bit-equal.
"""
import ctypes
import functools

import numpy as np
import torch

from helpers import cos_dist, load_case
from mvector import _hip

GOLDENS = ['resnetse_tiny_asp', 'resnetse_tiny_sap', 'resnetse_tiny_tap', 'resnetse_tiny_tsp', 'resnetse_tiny2', 'resnetse_default']
CHUNK = _hip.MV_SE2D_SQUEEZE_CHUNK
# (B, H, W, C, ld): the issue's three maps, then planes of chunk - 1, chunk and chunk + 1 pixels
SQUEEZE_SHAPES = [(2, 3, 5, 16, 16), (3, 8, 41, 32, 48), (1, 80, 98, 64, 64),
                  (2, 15, 17, 16, 16), (2, 16, 16, 16, 16), (2, 1, 257, 16, 16)]
assert [s[1] * s[2] for s in SQUEEZE_SHAPES[3:]] == [CHUNK - 1, CHUNK, CHUNK + 1]
EXCITE_SHAPES = [(32, 4), (96, 12), (512, 64)]
MAP_SHAPES = SQUEEZE_SHAPES[:3]
ROWS_SHAPES = [(2, 6, 64), (10, 13, 512), (3, 7, 96), (3, 7, 20)]   # (H, W, C); the last: C * H = 60, four zero columns up to the pitch 64
GATE_RTOL, GATE_ATOL = 2.0 ** -20, 2.0 ** -29


def _st(t):
    return _hip.current_stream(t)


def split(cdll, x):
    """fp32 [..., ld] (ld % 16 == 0) -> the S16 map in a buffer of the same shape"""
    x = x.contiguous()
    y = torch.empty_like(x)
    _hip.check(cdll.mv_map_split_f32(x.data_ptr(), y.data_ptr(), x.numel(), _st(x)), cdll)
    return y


def merge(cdll, m):
    y = torch.empty_like(m)
    _hip.check(cdll.mv_map_merge_f32(m.data_ptr(), y.data_ptr(), m.numel(), _st(m)), cdll)
    return y


def make_map(cdll, dev, B, H, W, C, ld, seed, scale=3.0, shift=0.4):
    """-> (S16 map [B, H, W, ld] with zero channels C.., its merged fp32 values on the CPU)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, ld, generator=g) * scale + shift
    x[..., C:] = 0.0
    m = split(cdll, x.to(dev))
    return m, merge(cdll, m).cpu()


def squeeze(cdll, m, C):
    B, H, W, ld = m.shape
    n = cdll.mv_se2d_squeeze_workspace_floats(B, H, W, C)
    ws = torch.empty(n + 2, dtype=torch.float32, device=m.device)
    s = torch.full((B, C), float('nan'), device=m.device)
    _hip.check(cdll.mv_se2d_squeeze_s16(m.data_ptr(), ld, B, H, W, C, s.data_ptr(), ws.data_ptr(), n, _st(m)), cdll)
    return s


def excite(cdll, s, w1, b1, w2, b2):
    B, C = s.shape
    g = torch.full((B, C), float('nan'), device=s.device)
    _hip.check(cdll.mv_se2d_excite_f32(s.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), g.data_ptr(), B, C, w1.shape[0],
                                       _st(s)), cdll)
    return g


def gate(cdll, x, g, res, C, peak=None, y=None):
    """y: the output map (default: a NaN-filled one at x's leading dimension; x itself = in place)"""
    B, H, W, ldx = x.shape
    if y is None:
        y = torch.full((B, H, W, ldx), float('nan'), device=x.device)
    _hip.check(cdll.mv_se2d_gate_res_relu_s16(x.data_ptr(), ldx, g.data_ptr(), res.data_ptr(), res.shape[-1], y.data_ptr(), y.shape[-1], B, H, W, C,
                                              None if peak is None else peak.data_ptr(), _st(x)), cdll)
    return y


def rows(cdll, m, C, ldy):
    B, H, W, ld = m.shape
    y = torch.full((B, W, ldy), float('nan'), dtype=torch.float16, device=m.device)
    _hip.check(cdll.mv_s16_map_to_rows_f16(m.data_ptr(), ld, B, H, W, C, y.data_ptr(), ldy, _st(m)), cdll)
    return y


# ------------------------------------------------------------------------------------------------ per kernel

def check_squeeze(cdll, dev, shape):
    """-> (error of the kernel, error of torch's fp32 mean), both max-abs against fp64 of the merged inputs"""
    B, H, W, C, ld = shape
    m, x = make_map(cdll, dev, B, H, W, C, ld, seed=sum(shape))
    got = squeeze(cdll, m, C).cpu().double()
    ref = x[..., :C].double().mean((1, 2))
    err = (got - ref).abs().max().item()
    err_torch = (x[..., :C].mean((1, 2)).double() - ref).abs().max().item()
    print(f'squeeze {shape}: kernel {err:.2e}  torch fp32 {err_torch:.2e}')
    assert err_torch > 0.0
    assert err <= 4.0 * err_torch, (err, err_torch)
    return err, err_torch


def excite_inputs(C, R, B=3):
    g = torch.Generator().manual_seed(C + R)
    s = torch.randn(B, C, generator=g) * 0.8 + 0.3
    return s, torch.randn(R, C, generator=g) / C ** 0.5 * 2, torch.randn(R, generator=g) * 0.2, torch.randn(C, R, generator=g) / R ** 0.5 * 2, \
        torch.randn(C, generator=g) * 0.2


def check_excite(cdll, dev, C, R):
    s, w1, b1, w2, b2 = excite_inputs(C, R)

    def f(t):
        return torch.sigmoid(torch.relu(t(s) @ t(w1).T + t(b1)) @ t(w2).T + t(b2))
    ref = f(lambda v: v.double())
    got = excite(cdll, *(v.to(dev) for v in (s, w1, b1, w2, b2))).cpu().double()
    err = (got - ref).abs().max().item()
    err_torch = (f(lambda v: v).double() - ref).abs().max().item()
    print(f'excite C {C} R {R}: kernel {err:.2e}  torch fp32 {err_torch:.2e}')
    assert err_torch > 0.0
    assert err <= 4.0 * err_torch, (err, err_torch)
    return err, err_torch


def gate_case(cdll, dev, shape, ldr_extra=16, seed=0, in_place=False):
    """x with both signs (negative pre-activations), res at its own leading dimension -> (y raw, expected merged values on the CPU)"""
    B, H, W, C, ld = shape
    x, xm = make_map(cdll, dev, B, H, W, C, ld, seed=seed + 11, scale=4.0, shift=-0.5)
    r, rm = make_map(cdll, dev, B, H, W, C, ld + ldr_extra, seed=seed + 12, scale=2.0, shift=0.0)
    g = torch.rand(B, C, generator=torch.Generator().manual_seed(seed + 13))
    y = gate(cdll, x, g.to(dev), r, C, y=x if in_place else None)
    v = torch.zeros(B, H, W, ld)
    v[..., :C] = torch.relu(xm[..., :C] * g[:, None, None, :] + rm[..., :C])   # torch's fp32: a rounded product, then the sum
    return y, merge(cdll, split(cdll, v.to(dev))).cpu()


def check_gate(cdll, dev, shape, in_place=False):
    """The kernel owns the channels 0 .. round_up(C, 16) of y: the values of 0 .. C, exact zero bits in the padding C .. round_up(C, 16) (the gate is
    not read there), and nothing beyond -- channels round_up(C, 16) .. ld belong to whoever shares the buffer (NaN-filled here: they stay NaN;
    in place: the zeros of the map stay zeros)."""
    B, H, W, C, ld = shape
    C16 = (C + 15) // 16 * 16
    y, expected = gate_case(cdll, dev, shape, seed=sum(shape), in_place=in_place)
    got, raw = merge(cdll, y).cpu()[..., :C16], y.cpu()
    expected = expected[..., :C16]
    assert (expected[..., :C] == 0).float().mean() > 0.2 and (expected > 0).float().mean() > 0.2   # the ReLU cuts a good part, and leaves one
    diff = (got.double() - expected.double()).abs()
    bound = GATE_RTOL * expected.double().abs() + GATE_ATOL
    print(f'gate {shape}: largest error / bound {(diff / bound).max().item():.3f}')
    assert (diff <= bound).all(), (diff / bound).max().item()
    assert torch.count_nonzero(got[..., C:]) == 0
    for u in range(C // 16, C16 // 16):     # the unit that holds padding: hi and lo halves of channels C .. are zero bits
        halves = raw[..., 16 * u:16 * u + 16].contiguous().view(torch.int16).reshape(B, H, W, 2, 16)
        assert torch.count_nonzero(halves[..., C - 16 * u:]) == 0
    if ld > C16:
        rest = raw[..., C16:]
        assert torch.count_nonzero(rest.contiguous().view(torch.int32)) == 0 if in_place else torch.isnan(rest).all()


def check_gate_peak(cdll, dev):
    """900 * 1 + 900 = 1800 > 1023.5: the word reports 64 * 1800 = 115200 (before the clamp), the map holds the clamped 1023.5"""
    x = split(cdll, torch.full((1, 2, 3, 16), 900.0).to(dev))
    peak = torch.zeros(1, dtype=torch.int32, device=dev)
    y = gate(cdll, x, torch.ones(1, 16, device=dev), x, 16, peak=peak)
    word = peak.cpu().view(torch.float32).item()
    assert word == 115200.0 and word > 65504.0
    assert torch.equal(merge(cdll, y).cpu(), torch.full((1, 2, 3, 16), 65504.0 / 64))
    peak.zero_()
    small = split(cdll, torch.full((1, 2, 3, 16), 1.5).to(dev))
    gate(cdll, small, torch.ones(1, 16, device=dev), small, 16, peak=peak)
    assert peak.cpu().view(torch.float32).item() == 64 * 3.0


def check_rows(cdll, dev, H, W, C, pitch_extra=0):
    B, ld = 2, (C + 15) // 16 * 16
    m, x = make_map(cdll, dev, B, H, W, C, ld, seed=H * W + C)
    ldy = (C * H + 7) // 8 * 8 + pitch_extra
    y = rows(cdll, m, C, ldy).cpu()
    expected = x[..., :C].half().permute(0, 2, 3, 1).reshape(B, W, C * H)    # [B, H, W, C] -> [B, W, c * H + h]
    assert torch.equal(y[..., :C * H].contiguous().view(torch.int16), expected.contiguous().view(torch.int16))
    assert torch.count_nonzero(y[..., C * H:].contiguous().view(torch.int16)) == 0


# ------------------------------------------------------------------------------------------------ the handle

@functools.lru_cache(maxsize=None)
def case(name):
    return load_case(name)


def module(man, sd):
    from mvector.models.resnet_se import ResNetSE
    m = ResNetSE(**man['kwargs'])
    m.load_state_dict(sd, strict=True)
    return m.eval()


def handle(cdll, dev, name, edit=None):
    man, sd, x, emb, _ = case(name)
    sd = {k: v.to(dev) for k, v in sd.items()}
    if edit:
        edit(sd)
    return _hip.Model('resnet_se', module(man, case(name)[1])._native_cfg(), sd, cdll=cdll), x.to(dev), emb


def check_golden(cdll, dev, name):
    h, x, emb = handle(cdll, dev, name)
    d = cos_dist(h.forward(x).cpu(), emb).max().item()
    rng = h.resnet_se_range()
    print(f'{name}: 1 - cos {d:.2e}  peak {rng["peak"]:.1f}')
    assert d <= 1e-4, d
    assert not rng['saturated']
    return d


def tiny_cfg(**over):
    """MvResNetSeCfg of the tiny goldens with fields replaced (lists for layers / num_filters)"""
    c = _hip.MvResNetSeCfg()
    f = dict(input_size=16, layers=[1, 1, 1, 1], num_filters=[16, 16, 32, 32], embd_dim=64, pooling_type=_hip.MV_POOL_ASP, reduction=8)
    f.update(over)
    for k, v in f.items():
        if isinstance(v, list):
            for i in range(4):
                getattr(c, k)[i] = v[i]
        else:
            setattr(c, k, v)
    return c


def create_rc(cdll, cfg, sd):
    """mv_resnetse_create on a state_dict -> (return code, message); a handle that came to life is released"""
    refs, tensors, _ = _hip._tensor_refs(sd)
    h = ctypes.c_void_p()
    rc = cdll.mv_resnetse_create(ctypes.byref(cfg), refs, len(tensors), ctypes.byref(h))
    msg = cdll.mv_last_error().decode() if rc else ''
    if h.value:
        cdll.mv_model_destroy(h)
    return rc, msg


def np_bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)
