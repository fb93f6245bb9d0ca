"""The kernels of csrc/hfencoder.hip one at a time, through the layer-level entry points mv_hfenc_wave_stats / _layer0 / _rows / _cmn_mask:
cases, fp64 references and per-element bounds shared by tests/test_hf_kernels.py (CPU: the bounds' self-checks, the cases under the emulator)
and tests/test_gpu_hf_kernels.py (device).  Every check takes the bound library `cdll` and the torch device `dev` its buffers live on.

A case has operands (CPU tensors, seeded, as the kernel sees them: fp16 inputs as stored, fp32 weights), an evaluator `*_eval(o, dtype, mutant)`
and a bound.  `*_eval(o, torch.float64)` is the reference; `*_eval(o, torch.float32)` is the ROUNDING MODEL (fp32 evaluation, fp16 at the kernel's
store sites, statistics in the kernel's precision); with `mutant=` it is the model of a subtly wrong kernel (MUTANTS).  The bounds are derived
from operation counts and rounding sites (u = 2^-24; see each `*_bound`), never from what a kernel gave; tests/test_hf_kernels.py shows on the CPU
that each admits the rounding model and rejects every applicable mutant on the case's own operands.

Conventions: `ratio` = max |got - ref| / bound, a NaN where none is expected counts as infinite; outputs, pitch gaps and the rows behind a result
are filled with NaN or a sentinel before the launch and asserted untouched."""
import ctypes
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from conv1d_cases import half_ulp_fp16
from mvector import _hip

U = 2.0 ** -24            # unit roundoff of fp32
ENC_EPS = 1e-5            # GroupNorm / LayerNorm of the feature encoder
ZS_EPS = 1e-7             # the processor's z-score
GELU_LIP = 1.13           # max |gelu'| = 1.1290 (at x = sqrt(2))
TINY = 2.0 ** -149        # a bound is never zero: the smallest fp32 subnormal
SENTINEL = 7.0

MUTANTS = ('tanh_gelu', 'unbiased', 'eps_swap', 'eps_x100', 'drop_tap', 'mean_unmasked', 'half_up', 'frames_plus', 'frames_minus')


def _f32(v):
    """the fp32 value of a Python float, as a float (what a kernel's fp32 constant or argument holds)"""
    return torch.tensor(v, dtype=torch.float32).item()


def _swap_eps(eps, mutant):
    if mutant == 'eps_swap':
        return ZS_EPS if eps > 1e-6 else ENC_EPS
    return eps * 100.0 if mutant == 'eps_x100' else eps


def gelu(x, mutant=None):
    if mutant == 'tanh_gelu':
        return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))
    return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752440))


def gelu_own_error(z64):
    """the roundings of hf_gelu(v) = 0.5f * v * (1 + erff(v * c)) on an fp32 v: the argument v * c carries 2 u relative (the product, the constant)
    -> |erf'(x) x| 2 u <= 1 u on erf; erff itself a few ulp (4 ulp = 8 u at |erf| <= 1); the sum 1 + erf one rounding at <= 2: 2 u.  Together 11 u
    ABSOLUTE on (1 + erf) -- where erf is near -1 the sum cancels and keeps that absolute error -- times 0.5 |v|; the product one more rounding."""
    return (5.5 * z64.abs() + gelu(z64).abs()) * U


def ratio_of(got, ref, bnd):
    r = (got.double() - ref).abs() / bnd
    r = torch.where(torch.isnan(r), torch.full_like(r, float('inf')), r)
    return r.max().item() if r.numel() else 0.0


def _dev(t, dev):
    return None if t is None else t.to(dev).contiguous()


def _sync(dev):
    if dev != 'cpu':
        torch.cuda.synchronize()


def _same_bits(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return torch.equal(a.view(it), b.view(it))


def row_lens(num_samples, B, L):
    if num_samples is None:
        return [L] * B
    return [min(max(int(n), 0), L) for n in num_samples]


def conv_frames(n, k, s):
    return (n - k) // s + 1 if n >= k else 0


# ================================================================================================ wave statistics

WAVE_ROWS = ('noise', 'dc1000', 'constant', 'quiet', 'noise', 'quiet')
# name -> (L, num_samples or None).  Rows wav_stride = L + 24 apart, NaN in the gap.  256 = the threads of the strided loop and the tree.
WAVE_CASES = {f'L{L}': (L, None) for L in (1, 255, 256, 257, 1000)}
WAVE_CASES['L1000_lengths'] = (1000, [0, -5, 2000, 500, 257, 1])


def wave_operands(name):
    L, ns = WAVE_CASES[name]
    g = torch.Generator().manual_seed(1000 + list(WAVE_CASES).index(name))
    B, stride = len(WAVE_ROWS), L + 24
    wav = torch.full((B, stride), float('nan'))
    for b, kind in enumerate(WAVE_ROWS):
        r = torch.randn(L, generator=g)
        wav[b, :L] = {'noise': 0.1 * r, 'dc1000': 1000.0 + r, 'constant': torch.full((L,), 0.25), 'quiet': 3e-4 * r}[kind]
    lens = row_lens(ns, B, L)
    for b, n in enumerate(lens):
        wav[b, n:] = float('nan')     # behind n_b, and the pitch gap
    return SimpleNamespace(name=name, L=L, B=B, stride=stride, wav=wav, num_samples=None if ns is None else torch.tensor(ns, dtype=torch.int64),
                           lens=lens)


def wave_eval(o, dtype=torch.float64, mutant=None):
    """[B, 2] (mean, sqrt(var + 1e-7)); n_b = 0: (0, 1).  The kernel sums in fp64 at either dtype; fp32: its float casts, fp32 add and sqrtf."""
    out = torch.zeros(o.B, 2, dtype=torch.float64)
    eps = _swap_eps(ZS_EPS, mutant)
    for b, n in enumerate(o.lens):
        if n == 0:
            out[b, 1] = 1.0
            continue
        x = o.wav[b, :n].double()
        mean = x.mean()
        var = ((x - mean) ** 2).sum() / ((n - 1) if mutant == 'unbiased' else n)
        if dtype == torch.float32:
            out[b, 0] = mean.float().double()
            out[b, 1] = torch.sqrt(var.float() + torch.tensor(eps, dtype=torch.float32)).double()
        else:
            out[b, 0], out[b, 1] = mean, torch.sqrt(var + _f32(eps))
    return out


def wave_bound(o, ref):
    """mean: the fp64 sum of n fp32 values errs by n 2^-53 mean|x| -- nothing -- and is rounded to fp32 once: u |mean| (+ that term).
    sd = sqrtf((float)var + 1e-7f): var from fp64 (nothing), its cast u, the add u, both relative to var + eps: 2 u, halved by the root; sqrtf
    at most 1 ulp = 2 u: 3 u sd, taken as 4 u sd (the fp32 constant 1e-7f is what the reference adds).  n_b = 0: exact."""
    bnd = torch.zeros_like(ref)
    for b, n in enumerate(o.lens):
        if n == 0:
            continue
        bnd[b, 0] = U * ref[b, 0].abs() + n * 2.0 ** -53 * o.wav[b, :n].double().abs().mean() + TINY
        bnd[b, 1] = 4.0 * U * ref[b, 1]
    return bnd


def wave_mutants(o):
    return ('unbiased', 'eps_swap', 'eps_x100')


def wave_run(cdll, dev, name, log=print):
    o = wave_operands(name)
    stats = torch.full((o.B + 1, 2), float('nan'), device=dev)
    wav = o.wav.to(dev)
    _hip.check(cdll.mv_hfenc_wave_stats(wav.data_ptr(), o.B, o.L, o.stride, _hip._ptr(_dev(o.num_samples, dev)), stats.data_ptr(),
                                        _hip.current_stream(wav)), cdll)
    _sync(dev)
    got = stats.cpu()
    assert torch.isnan(got[o.B]).all(), 'wave statistics wrote behind row B'
    ref = wave_eval(o)
    bnd = wave_bound(o, ref)
    for b, n in enumerate(o.lens):
        if n == 0:
            assert got[b].tolist() == [0.0, 1.0]
        if WAVE_ROWS[b] == 'constant' and n > 0:   # variance 0 exactly (fp64 sums of one value): sd = sqrtf(1e-7f)
            assert got[b, 0] == 0.25 and got[b, 1] == torch.sqrt(torch.tensor(1e-7, dtype=torch.float32))
    live = torch.tensor([n > 0 for n in o.lens])
    r = ratio_of(got[:o.B][live], ref[live], bnd[live])
    log(f'hf wave_stats {name:16s} max ratio {r:.3f}')
    assert r <= 1.0, (name, r)
    return r


# ================================================================================================ layer 0

def _l0(k, s, C, T0, mode, bias, wstats, extra=0, lens=None):
    return dict(k=k, s=s, C=C, T0=T0, mode=mode, bias=bias, wstats=wstats, extra=extra, lens=lens)


_VL = (0, 1, 128, 129, 257)    # T0_b of a variable-length batch (T0 = 257)
L0_CASES = {
    # hf_l0_kernel<*, 10>
    'k10s5_C512_T257_group': _l0(10, 5, 512, 257, 'group', False, True, extra=4),
    'k10s5_C320_T129_group_bias': _l0(10, 5, 320, 129, 'group', True, False),
    'k10s5_C64_T128_layer': _l0(10, 5, 64, 128, 'layer', True, True),
    'k3s2_C64_T127_group_bias': _l0(3, 2, 64, 127, 'group', True, True, extra=1),
    'k3s2_C320_T1_layer': _l0(3, 2, 320, 1, 'layer', True, False),
    'k1s1_C64_T129_group': _l0(1, 1, 64, 129, 'group', False, True),
    'k1s1_C512_T1_group_bias': _l0(1, 1, 512, 1, 'group', True, False),
    # hf_l0_kernel<*, 16>
    'k11s1_C64_T257_group_bias': _l0(11, 1, 64, 257, 'group', True, True),
    'k11s1_C320_T128_layer': _l0(11, 1, 320, 128, 'layer', True, False),
    'k16s8_C64_T128_group': _l0(16, 8, 64, 128, 'group', False, True),          # one full chunk: the LDS row to its last sample
    'k16s8_C512_T129_layer': _l0(16, 8, 512, 129, 'layer', True, False, extra=7),
    'k16s8_C320_T257_group_bias': _l0(16, 8, 320, 257, 'group', True, True, extra=7),
    # variable length: T0_b in {0, 1, 128, 129, T0} in one batch, NaN behind n_b
    'k10s5_C64_varlen_group': _l0(10, 5, 64, 257, 'group', True, True, lens=_VL),
    'k10s5_C64_varlen_layer': _l0(10, 5, 64, 257, 'layer', True, True, lens=_VL),
    'k16s8_C64_varlen_group': _l0(16, 8, 64, 257, 'group', False, False, lens=_VL),
}
ZERO_CH, DROP_CH, LOWVAR_CH = 0, 1, 2     # all-zero taps (bias 3.0); the channel the drop_tap mutant hits; taps scaled to an output variance of 1e-4


def l0_operands(name):
    c = L0_CASES[name]
    g = torch.Generator().manual_seed(2000 + list(L0_CASES).index(name))
    k, s, C, T0 = c['k'], c['s'], c['C'], c['T0']
    L = (T0 - 1) * s + k + c['extra']
    B = len(c['lens']) if c['lens'] else 2
    stride = L + 8
    wav = torch.full((B, stride), float('nan'))
    wav[:, :L] = 0.1 * torch.randn(B, L, generator=g) + 0.02
    ns = None
    if c['lens']:   # n_b: the samples of T0_b frames plus a few that belong to no frame
        ns = torch.tensor([0 if t == 0 else min((t - 1) * s + k + (b % s), L) for b, t in enumerate(c['lens'])], dtype=torch.int64)
        ns[0] = k - 1                                 # T0_b = 0 with samples present
        for b in range(B):
            wav[b, int(ns[b]):] = float('nan')
    lens = row_lens(ns, B, L)
    o = SimpleNamespace(name=name, k=k, s=s, C=C, T0=T0, L=L, B=B, stride=stride, wav=wav, num_samples=ns, lens=lens, mode=c['mode'],
                        T0b=[conv_frames(n, k, s) for n in lens])
    if c['lens']:
        assert tuple(o.T0b) == tuple(c['lens'])
    o.wstats = None
    if c['wstats']:   # the row's own z-score statistics, as mv_hfenc_wave_stats leaves them: fp32 operands of this kernel
        ws = wave_eval(SimpleNamespace(B=B, lens=lens, wav=wav), torch.float32)
        o.wstats = ws.float()
    o.w = torch.randn(C, k, generator=g) * (1.0 / k) ** 0.5
    o.w[ZERO_CH] = 0.0
    o.bias = None
    if c['bias']:
        o.bias = 0.1 * torch.randn(C, generator=g)
        o.bias[ZERO_CH] = 3.0
    o.gamma = o.beta = None
    if o.mode == 'group':
        o.gamma = 1.0 + 0.3 * torch.randn(C, generator=g)
        o.beta = (0.2 if T0 > 1 else 1.5) * torch.randn(C, generator=g)   # (one frame: the output is gelu(beta) alone -- spread over the GELU's range)
    if T0 > 1:   # LOWVAR_CH: its taps scaled so that the conv output of the longest row has variance 1e-4
        v = _l0_conv(o, torch.float64)[0]
        b = max(range(B), key=lambda i: o.T0b[i])
        sd = v[b, :o.T0b[b], LOWVAR_CH].std(unbiased=False).item()
        o.w[LOWVAR_CH] *= 1e-2 / sd
    return o


def _l0_conv(o, dtype, drop=False):
    """-> (v [B, T0, C] = conv + bias on the z-scored samples, S [B, T0, C] = the same on absolute values); samples behind n_b read as they lie"""
    x = o.wav[:, :o.L].to(dtype)
    if o.wstats is not None:
        x = (x - o.wstats[:, :1].to(dtype)) / o.wstats[:, 1:].to(dtype)
    w = o.w.to(dtype).clone()
    if drop:
        w[DROP_CH, -1] = 0.0
    bias = None if o.bias is None else o.bias.to(dtype)
    v = F.conv1d(x.unsqueeze(1), w.unsqueeze(1), bias, stride=o.s).transpose(1, 2)
    S = F.conv1d(torch.nan_to_num(x).abs().unsqueeze(1), w.abs().unsqueeze(1), None if bias is None else bias.abs(), stride=o.s).transpose(1, 2)
    return v, S


def l0_eval(o, dtype=torch.float64, mutant=None, parts=False):
    """-> (y [B, T0, C] fp64 values -- the fp32 model's rounded to fp16 --, cstats [B, C, 2] or None).  The GroupNorm sums are fp64 at either dtype
    (over the fp32 conv values in the model, as in the kernel)."""
    v, S = _l0_conv(o, dtype, drop=mutant == 'drop_tap')
    T0b = [min(max(t + {'frames_plus': 1, 'frames_minus': -1}.get(mutant, 0), 0), o.T0) for t in o.T0b]
    live = torch.zeros(o.B, o.T0, 1, dtype=torch.bool)
    for b, t in enumerate(T0b):
        live[b, :t] = True
    f32 = dtype == torch.float32
    cstats = None
    z = v
    if o.mode == 'group':
        eps = _f32(_swap_eps(ENC_EPS, mutant))
        cstats = torch.zeros(o.B, o.C, 2, dtype=torch.float64)
        cstats[..., 1] = 1.0
        for b, t in enumerate(T0b):
            if t == 0:
                continue
            vb = v[b, :t].double()
            m = vb.mean(0)
            var = ((vb - m) ** 2).sum(0) / ((t - 1) if mutant == 'unbiased' else t)
            cstats[b, :, 0], cstats[b, :, 1] = m, 1.0 / torch.sqrt(var + eps)
        if f32:
            cstats = cstats.float().double()
        cs = cstats.to(dtype)
        z = (v - cs[:, None, :, 0]) * cs[:, None, :, 1] * o.gamma.to(dtype) + o.beta.to(dtype)
        y = gelu(z, mutant)
    else:
        y = v
    if f32:
        y = y.half()
    y = torch.where(live, y.double(), torch.zeros((), dtype=torch.float64))
    return (y, cstats, v.double(), S.double(), z.double(), live) if parts else (y, cstats)


def l0_bound(o):
    """(ref y, ref cstats, bound y, bound cstats).  Per element, S = sum_j |w_j| |x_j| + |bias| of the frame:
      conv     k fmas onto the bias: (k + 1) u S in any order; with wstats every sample (x - mean) / sd carries a subtraction and a division,
               3 u relative, on its product: e_v = (k + 1 + 3) u S (k + 1 without wstats).  "layer" mode stores it: e_v + half an fp16 ulp.
      GroupNorm sums: fp64 over the kernel's fp32 conv values -- their own error is nothing; the conv errors move the mean by at most
               mean_t(e_v) and the biased variance by 2 sd max_t(e_v) (Cauchy-Schwarz; the mean's own shift cancels), so rstd = (var + eps)^-1/2 by
               rstd^3 sd max_t(e_v).  Both are rounded to fp32 once: + u |mean|, + 2 u rstd (the cast, and the second-order terms).
      z = (v - m) r g + b: |g| r (e_v + e_mean) + |g| |v - m| e_rstd, three roundings of the product chain 3 u |(v - m) r g|, the fma u |z|.
      GELU     Lipschitz 1.13 on e_z, its own roundings gelu_own_error(z); the fp16 store: half an ulp at |ref| + e.
    Frames from T0_b on are exact zeros; cstats at T0_b = 0 exactly (0, 1)."""
    y, cstats, v, S, z, live = l0_eval(o, parts=True)
    e_v = (o.k + 1 + (3 if o.wstats is not None else 0)) * U * S
    if o.mode == 'layer':
        e = e_v
        cb = None
    else:
        cb = torch.full_like(cstats, TINY)
        e_mean = torch.zeros(o.B, 1, o.C, dtype=torch.float64)
        e_rstd = torch.zeros(o.B, 1, o.C, dtype=torch.float64)
        for b, t in enumerate(o.T0b):
            if t == 0:
                continue
            m, r = cstats[b, :, 0], cstats[b, :, 1]
            sd = v[b, :t].std(0, unbiased=False)
            e_mean[b, 0] = e_v[b, :t].mean(0) + U * m.abs()
            e_rstd[b, 0] = r ** 3 * sd * e_v[b, :t].max(0).values + 2.0 * U * r
            cb[b, :, 0], cb[b, :, 1] = e_mean[b, 0] + TINY, e_rstd[b, 0]
        g = o.gamma.double().abs()
        m, r = cstats[:, None, :, 0], cstats[:, None, :, 1]
        lin = torch.nan_to_num((v - m).abs())
        e_z = g * r * (e_v + e_mean) + g * lin * e_rstd + 3.0 * U * lin * r * g + U * torch.nan_to_num(z).abs()
        e = GELU_LIP * e_z + gelu_own_error(torch.nan_to_num(z))
    e = torch.where(live, e, torch.zeros((), dtype=torch.float64))
    return y, cstats, e + half_ulp_fp16(y.abs() + e), cb


def l0_ratio(o, got_y, got_c, ref_y, ref_c, by, bc):
    r = ratio_of(got_y, ref_y, by)
    return r if ref_c is None else max(r, ratio_of(got_c, ref_c, bc))


def l0_mutants(o):
    m = ['drop_tap']
    if o.mode == 'group':
        m += ['tanh_gelu', 'unbiased', 'eps_swap', 'eps_x100']
    if o.num_samples is not None:
        m += ['frames_plus', 'frames_minus']
    return m


def l0_launch(cdll, dev, o, rows=None, L=None, num_samples='own'):
    """-> (y [B + 1, T0, C] raw with a sentinel row behind, cstats [B + 1, C, 2] NaN-filled); rows / L: a sub-batch at another row length"""
    rows = list(range(o.B)) if rows is None else rows
    L = o.L if L is None else L
    B, T0 = len(rows), conv_frames(L, o.k, o.s)
    wav = o.wav[rows].to(dev).contiguous()
    ns = o.num_samples[rows] if (num_samples == 'own' and o.num_samples is not None) else None
    keep = [_dev(t, dev) for t in (ns, None if o.wstats is None else o.wstats[rows], o.w, o.bias, o.gamma, o.beta)]
    y = torch.full((B + 1, T0, o.C), SENTINEL, dtype=torch.float16, device=dev)
    cstats = torch.full((B + 1, o.C, 2), float('nan'), device=dev)
    need = ctypes.c_size_t()
    _hip.check(cdll.mv_hfenc_layer0_workspace_bytes(B, L, o.C, o.k, o.s, ctypes.byref(need)), cdll)
    ws = torch.empty(need.value + 8, dtype=torch.uint8, device=dev)
    _hip.check(cdll.mv_hfenc_layer0(wav.data_ptr(), B, L, o.stride, *[_hip._ptr(t) for t in keep], o.C, o.k, o.s, y.data_ptr(), cstats.data_ptr(),
                                    ws.data_ptr(), need.value, _hip.current_stream(wav)), cdll)
    _sync(dev)
    return y.cpu(), cstats.cpu()


def l0_run(cdll, dev, name, log=print):
    o = l0_operands(name)
    y, cs = l0_launch(cdll, dev, o)
    assert bool((y[o.B] == SENTINEL).all()), 'layer 0 wrote behind its last row'
    assert torch.isnan(cs[o.B]).all(), 'layer 0 wrote cstats behind its last row'
    ref_y, ref_c, by, bc = l0_bound(o)
    group = o.mode == 'group'
    if not group:
        assert torch.isnan(cs).all(), '"layer" mode touched cstats'
    got = y[:o.B].double()
    for b, t in enumerate(o.T0b):
        assert torch.count_nonzero(got[b, t:]) == 0, f'row {b}: frames from T0_b = {t} on are not zero'
        if group and t == 0:
            assert cs[b, :, 0].abs().max() == 0 and bool((cs[b, :, 1] == 1).all())
        if group and t > 0:   # variance 0: the output is half(gelu(beta)) in every frame, exactly
            want = gelu(o.beta[ZERO_CH].double()).half()
            assert bool((y[b, :t, ZERO_CH] == want).all()), (name, b, y[b, :t, ZERO_CH].unique(), want)
    r = l0_ratio(o, got, cs[:o.B].double(), ref_y, ref_c, by, bc)
    log(f'hf layer0 {name:30s} max ratio {r:.3f}' + (f' (y {ratio_of(got, ref_y, by):.3f})' if group else ''))
    assert r <= 1.0, (name, r)
    if o.num_samples is not None:   # row b's own frames: the bits of the same row alone with L = n_b
        for b, t in enumerate(o.T0b):
            if t == 0:
                continue
            ya, ca = l0_launch(cdll, dev, o, rows=[b], L=o.lens[b], num_samples=None)
            assert _same_bits(ya[0], y[b, :t]), f'row {b}: the bits depend on the batch'
            assert not group or _same_bits(ca[0], cs[b])
    return r


# ================================================================================================ rows

MODES = {'gelu': _hip.MV_HF_ROWS_GELU, 'ln_gelu': _hip.MV_HF_ROWS_LN_GELU, 'ln_f32': _hip.MV_HF_ROWS_LN_F32}
# a single row is the zero-centred low-variance one: at mean 0.5 the worst case of the fp32 mean, (C - 1) u S1 / C, is 0.5 % of the row's spread
# and hides an unbiased variance; around zero it is 3e-5 of it
ROW_KINDS = {1: ['lowvar0'], 4: ['constant', 'mean1000', 'peak', 'lowvar'], 5: ['constant', 'mean1000', 'peak', 'lowvar', 'noise'],
             9: ['constant', 'mean1000', 'peak', 'lowvar', 'lowvar0'] + ['noise'] * 4}
# every mode at every width; n_rows walks {1, 4, 5, 9} (four waves per workgroup: a ragged last workgroup, a single wave, exact)
ROWS_CASES = {f'{mode}_C{C}_R{R}': (mode, C, R)
              for i, mode in enumerate(MODES) for j, (C, R) in enumerate(zip((64, 192, 512, 576, 1024), (9, 5, 4, 1, 9)))}
ROWS_CASES.update({'ln_gelu_C512_R1': ('ln_gelu', 512, 1), 'ln_f32_C512_R5': ('ln_f32', 512, 5), 'gelu_C512_R9': ('gelu', 512, 9),
                   'ln_f32_C64_R4': ('ln_f32', 64, 4)})


def rows_operands(name):
    mode, C, R = ROWS_CASES[name]
    g = torch.Generator().manual_seed(3000 + list(ROWS_CASES).index(name))
    x = torch.empty(R, C)
    for r, kind in enumerate(ROW_KINDS[R]):
        if kind == 'constant':
            x[r] = 0.75
        elif kind == 'mean1000':     # fp16 spacing at 1000 is 0.5
            x[r] = 1000.0 + 0.5 * torch.randint(-16, 17, (C,), generator=g)
        elif kind == 'peak':
            x[r] = 65504.0 * (2.0 * torch.randint(0, 2, (C,), generator=g) - 1.0)
        elif kind == 'lowvar':       # fp16 spacing at 0.5 is 2^-12: +-22 steps, uniform: sd 3.1e-3, variance 1e-5
            x[r] = 0.5 + 2.0 ** -12 * torch.randint(-22, 23, (C,), generator=g)
        elif kind == 'lowvar0':      # the same spread around zero
            x[r] = 2.0 ** -12 * torch.randint(-22, 23, (C,), generator=g)
        else:
            x[r] = 1.5 * torch.randn(C, generator=g) + 0.3
    if mode == 'gelu':   # no normalisation in front: values of the GELU's interesting range in every row
        x = 2.5 * torch.randn(R, C, generator=g)
    x = x.half()
    assert torch.equal(x.float().half(), x) and bool(torch.isfinite(x).all())
    o = SimpleNamespace(name=name, mode=mode, C=C, R=R, x=x, kinds=ROW_KINDS[R], eps=ENC_EPS, gamma=None, beta=None)
    if mode != 'gelu':
        o.gamma = 1.0 + 0.3 * torch.randn(C, generator=g)
        o.beta = 0.2 * torch.randn(C, generator=g)
    return o


def rows_eval(o, dtype=torch.float64, mutant=None, parts=False):
    x = o.x.to(dtype)
    f32 = dtype == torch.float32
    if o.mode == 'gelu':
        y = gelu(x, mutant)
        return y.half().double() if f32 else y
    eps = _f32(_swap_eps(o.eps, mutant))
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).sum(-1, keepdim=True) / ((o.C - 1) if mutant == 'unbiased' else o.C)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=dtype))
    z = d * rstd * o.gamma.to(dtype) + o.beta.to(dtype)
    if parts:
        return mean, d, var, rstd, z
    if o.mode == 'ln_f32':
        return z.double()
    y = gelu(z, mutant)
    return y.half().double() if f32 else y


def rows_bound(o):
    """(ref, bound) [R, C].  GELU mode: the input is exact: gelu_own_error(x), then the fp16 store's half ulp.
    LayerNorm over C fp16 values held exactly in fp32, S1 = sum |x|:
      mean   C - 1 additions in any order (lanes, then the wave tree): (C - 1) u S1, over C; the division 2 u |mean|: e_mean.
      d      x - mean: u |d| + e_mean.  The SAME computed mean shifts every d: as sum d = 0 the shift enters sum d^2 in second order, C e_mean^2.
      var    the roundings of the d: 2 u Q; C products and additions: (C + 1) u Q; the division and + eps: 3 u.  Relative to var + eps:
             rho = (C + 6) u + e_mean^2 / (var + eps).
      rstd   1 / sqrtf: rho / 2 + 4 u (root and division at 1 ulp = 2 u each).
      z      (d rstd) g + b: |g| rstd (e_mean + u |d|) + |g| |d| rstd (rho / 2 + 4 u) + u |d rstd g| + u |z|.
    LN_F32 stores z: that bound.  LN_GELU: 1.13 e_z + gelu_own_error(z), then the fp16 store."""
    if o.mode == 'gelu':
        ref = rows_eval(o)
        e = gelu_own_error(o.x.double())
        return ref, e + half_ulp_fp16(ref.abs() + e)
    mean, d, var, rstd, z = rows_eval(o, parts=True)
    g = o.gamma.double().abs()
    S1 = o.x.double().abs().sum(-1, keepdim=True)
    e_mean = (o.C - 1) * U * S1 / o.C + 2.0 * U * mean.abs()
    rho = (o.C + 6) * U + e_mean ** 2 / (var + _f32(o.eps))
    e_z = g * rstd * (e_mean + U * d.abs()) + g * d.abs() * rstd * (rho / 2 + 4.0 * U) + U * (d * rstd).abs() * g + U * z.abs() + TINY
    if o.mode == 'ln_f32':
        return z, e_z
    ref = gelu(z)
    e = GELU_LIP * e_z + gelu_own_error(z)
    return ref, e + half_ulp_fp16(ref.abs() + e)


def rows_mutants(o):
    return ('tanh_gelu',) if o.mode == 'gelu' else (('unbiased', 'eps_swap', 'eps_x100') + (('tanh_gelu',) if o.mode == 'ln_gelu' else ()))


def rows_launch(cdll, dev, x, mode, gamma=None, beta=None, eps=ENC_EPS, extra_rows=2):
    """x [R, C] fp16 -> the whole output buffer [R + extra_rows, C]: in place for the fp16 modes (the forward's way), NaN-filled fp32 for LN_F32;
    the rows behind R hold the sentinel on the way in"""
    R, C = x.shape
    buf = torch.full((R + extra_rows, C), SENTINEL, dtype=torch.float16)
    buf[:R] = x
    buf = buf.to(dev)
    y = torch.full((R + extra_rows, C), float('nan'), device=dev) if mode == 'ln_f32' else buf
    gd, bd = _dev(gamma, dev), _dev(beta, dev)
    _hip.check(cdll.mv_hfenc_rows(buf.data_ptr(), y.data_ptr(), _hip._ptr(gd), _hip._ptr(bd), eps, R, C, MODES[mode], _hip.current_stream(buf)), cdll)
    _sync(dev)
    if mode == 'ln_f32':
        assert _same_bits(buf.cpu()[:R], x), 'LN_F32 changed its input'
    return y.cpu()


def rows_run(cdll, dev, name, log=print):
    o = rows_operands(name)
    y = rows_launch(cdll, dev, o.x, o.mode, o.gamma, o.beta, o.eps)
    tail = y[o.R:]
    assert torch.isnan(tail).all() if o.mode == 'ln_f32' else bool((tail == SENTINEL).all()), 'rows wrote behind n_rows'
    ref, bnd = rows_bound(o)
    got = y[:o.R].double()
    if o.mode != 'gelu' and 'constant' in o.kinds:   # d = 0 exactly: beta, or half(gelu(beta))
        want = o.beta if o.mode == 'ln_f32' else gelu(o.beta.double()).half()
        assert torch.equal(y[o.kinds.index('constant')], want), 'a constant row is not exactly beta'
    r = ratio_of(got, ref, bnd)
    log(f'hf rows {name:22s} max ratio {r:.3f}')
    assert r <= 1.0, (name, r)
    return r


def all_finite_halves():
    """every finite fp16 value, 63488 = 992 rows of 64"""
    bits = torch.arange(0, 65536, dtype=torch.int32)
    bits = bits[(bits & 0x7c00) != 0x7c00]
    assert bits.numel() == 63488
    return bits.to(torch.int16).view(torch.float16).reshape(992, 64)


def gelu_exhaustive_run(cdll, dev, log=print):
    x = all_finite_halves()
    o = SimpleNamespace(mode='gelu', x=x, C=64, R=992)
    y = rows_launch(cdll, dev, x, 'gelu')
    assert bool((y[992:] == SENTINEL).all())
    ref, bnd = rows_bound(o)
    r = ratio_of(y[:992].double(), ref, bnd)
    log(f'hf rows gelu, every finite fp16 value: max ratio {r:.3f}')
    assert r <= 1.0, r
    special = torch.zeros(1, 64, dtype=torch.float16)
    special[0, 0], special[0, 1], special[0, 2] = float('nan'), float('inf'), float('-inf')
    ys = rows_launch(cdll, dev, special, 'gelu')[0]
    assert torch.isnan(ys[0]) and torch.count_nonzero(ys[3:]) == 0
    t = F.gelu(special[0, :3].float())
    log(f'hf rows gelu(+inf, -inf) = ({ys[1].item()}, {ys[2].item()}); torch: ({t[1].item()}, {t[2].item()})')
    return r


# ================================================================================================ time mean and mask

GEOM = ([10, 3], [5, 2])     # the layers of the num_samples form: T' = T_1(T_0(n))


def _samples_for(T):
    """the fewest samples with T frames behind GEOM"""
    n = T
    for k, s in zip(reversed(GEOM[0]), reversed(GEOM[1])):
        n = (n - 1) * s + k
    return n


def frames_behind(n):
    for k, s in zip(*GEOM):
        n = conv_frames(n, k, s)
    return n


def tie_ratio(T):
    """a ratio whose fp32 product with T is exactly (even + 0.5): half-even rounds down, half-up rounds up"""
    for m in range(0, T + 1, 2):
        r = torch.tensor((m + 0.5) / T, dtype=torch.float32)
        if (r * torch.tensor(float(T))).item() == m + 0.5 and m + 0.5 < T + 1:
            return r.item()
    raise AssertionError(T)


# name -> (T, C, cmn, form): 'ratio' | 'samples'.  T walks the four time phases; 192 channels: three 64-channel workgroups per row
CMN_CASES = {f'T{T}_C{C}_ratio': (T, C, 1, 'ratio') for T, C in ((1, 64), (3, 192), (4, 64), (5, 192), (7, 64), (50, 192))}
CMN_CASES.update({'T1_C192_ratio_nocmn': (1, 192, 0, 'ratio'), 'T5_C64_ratio_nocmn': (5, 64, 0, 'ratio'), 'T7_C192_whole': (7, 192, 1, 'none'), 'T5_C64_samples': (5, 64, 1, 'samples'),
                  'T50_C192_samples': (50, 192, 1, 'samples'), 'T4_C64_samples_nocmn': (4, 64, 0, 'samples')})


def cmn_operands(name):
    T, C, cmn, form = CMN_CASES[name]
    g = torch.Generator().manual_seed(4000 + list(CMN_CASES).index(name))
    o = SimpleNamespace(name=name, T=T, C=C, cmn=cmn, form=form, ratio=None, num_samples=None, L=0)
    if form == 'samples':
        Tb = [0, 1, T, max(T // 2, 1), T]
        o.L = _samples_for(T) + 3
        o.num_samples = torch.tensor([_samples_for(t) - (1 if t == 0 else 0) + (b % 2) for b, t in enumerate(Tb)], dtype=torch.int64)
        o.num_samples[4] = o.L + 1000           # above L: clamped
        o.Tb = [frames_behind(min(max(int(n), 0), o.L)) for n in o.num_samples]
        assert o.Tb == Tb and frames_behind(o.L) == T
        o.mask = list(o.Tb)
    else:
        ratios = [0.0, 1.0, 1.2, 0.5, tie_ratio(T), 0.61] if form == 'ratio' else None
        o.ratio = None if ratios is None else torch.tensor(ratios, dtype=torch.float32)
        B = 6 if ratios else 3
        o.Tb = [T] * B
        o.mask = [T] * B if ratios is None else [int(torch.round(r * T)) for r in o.ratio]     # (torch.round: half to even, in fp32)
        if ratios and T in (5, 7):
            assert o.mask[3] == {5: 2, 7: 4}[T]
    o.B = len(o.Tb)
    o.x = 2.0 * torch.randn(o.B, T, C, generator=g) + 0.7
    if form == 'samples':   # behind a row's own frames: filler that must neither reach the mean nor survive
        for b, t in enumerate(o.Tb):
            o.x[b, t:] = float('nan')
            o.x[b, t + 1:] = 1e30
    return o


def cmn_eval(o, dtype=torch.float64, mutant=None):
    x = o.x.to(dtype)
    y = torch.zeros_like(x)
    for b in range(o.B):
        Tb, mask = o.Tb[b], o.mask[b]
        if o.form == 'samples':
            Tb = mask = min(max(Tb + {'frames_plus': 1, 'frames_minus': -1}.get(mutant, 0), 0), o.T)
        elif o.form == 'ratio' and mutant == 'half_up':
            mask = int(torch.floor(o.ratio[b] * o.T + 0.5))
        n = min(mask, Tb) if mutant == 'mean_unmasked' else Tb
        mean = x[b, :n].sum(0) / n if (o.cmn and n > 0) else torch.zeros(o.C, dtype=dtype)
        keep = min(mask, o.T)
        y[b, :keep] = x[b, :keep] - mean
    return y.double()


def cmn_bound(o):
    """(ref, bound).  The mean of Tb fp32 values: Tb - 1 additions in any order (four phases, then their sum), (Tb - 1) u S1 with S1 = sum_t |x_t|,
    over Tb; the division 2 u |mean|; the subtraction u |x - mean|.  Without cmn the kernel subtracts 0.0: exact.  Masked frames are exact zeros."""
    ref = cmn_eval(o)
    bnd = torch.full_like(ref, TINY)
    for b in range(o.B):
        Tb, keep = o.Tb[b], min(o.mask[b], o.T)
        if not o.cmn or Tb == 0:
            continue
        xb = o.x[b, :Tb].double()
        e_mean = (Tb - 1) * U * xb.abs().sum(0) / Tb + 2.0 * U * xb.mean(0).abs()
        bnd[b, :keep] = e_mean + U * ref[b, :keep].abs() + TINY
    return ref, bnd


def cmn_mutants(o):
    """mean_unmasked needs a partly masked row (none at T = 1); half_up a tie (tie_ratio: every ratio case has one) -- but one frame minus its own
    mean is zero masked or not, so at T = 1 the mask shows without cmn only; the frame count of a row only exists in the num_samples form"""
    if o.form == 'samples':
        return ('frames_plus', 'frames_minus')
    if o.form == 'none':
        return ()
    return (('half_up',) if (o.T > 1 or not o.cmn) else ()) + (('mean_unmasked',) if o.cmn and any(0 < m < o.T for m in o.mask) else ())


def cmn_launch(cdll, dev, x, T, C, cmn, ratio=None, num_samples=None, L=0, geom=GEOM):
    B = x.shape[0]
    buf = torch.full((B + 1, T, C), SENTINEL)
    buf[:B] = x
    buf = buf.to(dev)
    rd, nd = _dev(ratio, dev), _dev(num_samples, dev)
    n = len(geom[0])
    ks, ss = (ctypes.c_int32 * n)(*geom[0]), (ctypes.c_int32 * n)(*geom[1])
    _hip.check(cdll.mv_hfenc_cmn_mask(buf.data_ptr(), B, T, C, _hip._ptr(rd), _hip._ptr(nd), L, ks, ss, n, cmn, _hip.current_stream(buf)), cdll)
    _sync(dev)
    return buf.cpu()


def cmn_run(cdll, dev, name, log=print):
    o = cmn_operands(name)
    y = cmn_launch(cdll, dev, o.x, o.T, o.C, o.cmn, o.ratio, o.num_samples, o.L)
    assert bool((y[o.B] == SENTINEL).all()), 'the time mean wrote behind its last row'
    got = y[:o.B]
    for b in range(o.B):
        keep = min(o.mask[b], o.T)
        assert torch.count_nonzero(got[b, keep:].contiguous().view(torch.int32)) == 0, f'row {b}: frames from {keep} on are not zero bits'
        if not o.cmn:
            assert _same_bits(got[b, :keep], o.x[b, :keep])
    ref, bnd = cmn_bound(o)
    r = ratio_of(got.double(), ref, bnd)
    log(f'hf cmn_mask {name:22s} max ratio {r:.3f}')
    assert r <= 1.0, (name, r)
    return r


# ================================================================================================ self-checks of the bounds (no launch)

FAMILIES = {
    'wave': (WAVE_CASES, wave_operands, wave_mutants),
    'layer0': (L0_CASES, l0_operands, l0_mutants),
    'rows': (ROWS_CASES, rows_operands, rows_mutants),
    'cmn': (CMN_CASES, cmn_operands, cmn_mutants),
}


def model_ratios(family, name):
    """-> (ratio of the fp32 rounding model, {mutant: ratio of the mutated model}) on the case's own operands"""
    _, operands, mutants = FAMILIES[family]
    o = operands(name)
    if family == 'wave':
        ref = wave_eval(o)
        bnd = wave_bound(o, ref) + TINY
        f = lambda m: ratio_of(wave_eval(o, torch.float32, m), ref, bnd)   # noqa: E731
    elif family == 'layer0':
        ref_y, ref_c, by, bc = l0_bound(o)
        f = lambda m: l0_ratio(o, *l0_eval(o, torch.float32, m), ref_y, ref_c, by, bc)   # noqa: E731
    elif family == 'rows':
        ref, bnd = rows_bound(o)
        f = lambda m: ratio_of(rows_eval(o, torch.float32, m), ref, bnd)   # noqa: E731
    else:
        ref, bnd = cmn_bound(o)
        f = lambda m: ratio_of(cmn_eval(o, torch.float32, m), ref, bnd)   # noqa: E731
    return f(None), {m: f(m) for m in mutants(o)}


# ================================================================================================ the pieces are what the forward runs

def composed_forward(cdll, dev, cfg, sd, wav, lens_ratio=None, num_samples=None, subtract_time_mean=True):
    """mv_hfenc_forward / _varlen restated from the layer-level entry points and mv_conv1d_forward: the same launches, buffers of its own"""
    import layer_checks as lc
    st = _hip.current_stream(torch.zeros(1, device=dev))
    chk = lambda rc: _hip.check(rc, cdll)   # noqa: E731
    p = lambda k: sd[k].detach().float().to(dev).contiguous()   # noqa: E731
    fe = 'feature_extractor.conv_layers.'
    dims, ks, ss = list(cfg['conv_dim']), list(cfg['conv_kernel']), list(cfg['conv_stride'])
    group, has_bias = cfg.get('feat_extract_norm', 'group') == 'group', bool(cfg.get('conv_bias', False))
    wav = wav.float().to(dev).contiguous()
    B, L = wav.shape
    T, n = [], L
    for k, s in zip(ks, ss):
        n = conv_frames(n, k, s)
        T.append(n)
    nd = _dev(num_samples, dev)
    wstats = None
    if cfg.get('do_normalize', True):
        wstats = torch.empty(B, 2, device=dev)
        chk(cdll.mv_hfenc_wave_stats(wav.data_ptr(), B, L, wav.stride(0), _hip._ptr(nd), wstats.data_ptr(), st))
    w0 = p(fe + '0.conv.weight').reshape(dims[0], ks[0]).contiguous()
    bias0 = p(fe + '0.conv.bias') if has_bias else None
    g0, b0 = p(fe + '0.layer_norm.weight'), p(fe + '0.layer_norm.bias')
    x = torch.empty(B, T[0], dims[0], dtype=torch.float16, device=dev)
    cstats = torch.empty(B, dims[0], 2, device=dev)
    need = ctypes.c_size_t()
    chk(cdll.mv_hfenc_layer0_workspace_bytes(B, L, dims[0], ks[0], ss[0], ctypes.byref(need)))
    ws = torch.empty(need.value + 8, dtype=torch.uint8, device=dev)
    chk(cdll.mv_hfenc_layer0(wav.data_ptr(), B, L, wav.stride(0), _hip._ptr(nd), _hip._ptr(wstats), w0.data_ptr(), _hip._ptr(bias0),
                             g0.data_ptr() if group else None, b0.data_ptr() if group else None, dims[0], ks[0], ss[0], x.data_ptr(),
                             cstats.data_ptr(), ws.data_ptr(), need.value, st))
    if not group:
        chk(cdll.mv_hfenc_rows(x.data_ptr(), x.data_ptr(), g0.data_ptr(), b0.data_ptr(), ENC_EPS, B * T[0], dims[0], MODES['ln_gelu'], st))
    keep = []
    for i in range(1, len(dims)):
        packed = lc.pack_weight(cdll, p(fe + f'{i}.conv.weight'))
        bias = p(fe + f'{i}.conv.bias') if has_bias else None
        y = torch.empty(B, T[i], dims[i], dtype=torch.float16, device=dev)
        d = _hip.MvConv1dDesc()
        d.x, d.ldx, d.y, d.ldy = x.data_ptr(), dims[i - 1], y.data_ptr(), dims[i]
        d.x_dtype = d.y_dtype = _hip.MV_DT_F16
        d.w_packed, d.bias = packed.data_ptr(), _hip._ptr(bias)
        d.B, d.T_in, d.T_out, d.cin, d.cout, d.k = B, T[i - 1], T[i], dims[i - 1], dims[i], ks[i]
        d.dilation, d.stride, d.pad, d.pad_mode, d.tile = 1, ss[i], 0, _hip.MV_PAD_ZERO, 0
        chk(cdll.mv_conv1d_forward(ctypes.byref(d), st))
        if group:
            chk(cdll.mv_hfenc_rows(y.data_ptr(), y.data_ptr(), None, None, 0.0, B * T[i], dims[i], MODES['gelu'], st))
        else:
            gi, bi = p(fe + f'{i}.layer_norm.weight'), p(fe + f'{i}.layer_norm.bias')
            keep += [gi, bi]
            chk(cdll.mv_hfenc_rows(y.data_ptr(), y.data_ptr(), gi.data_ptr(), bi.data_ptr(), ENC_EPS, B * T[i], dims[i], MODES['ln_gelu'], st))
        keep += [packed, bias, x]
        x = y
    out = torch.empty(B, T[-1], dims[-1], device=dev)
    pw, pb = p('feature_projection.layer_norm.weight'), p('feature_projection.layer_norm.bias')
    chk(cdll.mv_hfenc_rows(x.data_ptr(), out.data_ptr(), pw.data_ptr(), pb.data_ptr(), float(cfg.get('layer_norm_eps', 1e-5)), B * T[-1], dims[-1],
                           MODES['ln_f32'], st))
    nl = len(dims)
    rd = _dev(lens_ratio, dev)
    chk(cdll.mv_hfenc_cmn_mask(out.data_ptr(), B, T[-1], dims[-1], _hip._ptr(rd), _hip._ptr(nd), L, (ctypes.c_int32 * nl)(*ks),
                               (ctypes.c_int32 * nl)(*ss), nl, 1 if subtract_time_mean else 0, st))
    _sync(dev)
    return out.cpu()


def composition_case(cdll, dev, fixture, varlen=False):
    """a width-64 fixture at L = 2400, B = 3: the composed forward has the bits of the handle's"""
    import hf_cases as hc
    cfg, sd, wav, _ = hc.load_fixture(fixture)
    wav = wav[:, :2400].contiguous()
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    h = _hip.HfEncoder(cfg, sd_dev, cdll=cdll)
    if varlen:
        ns = torch.tensor([2400, 399, 1237], dtype=torch.int64)
        want = h(wav.to(dev), num_samples=ns.to(dev)).cpu()
        got = composed_forward(cdll, dev, cfg, sd, wav, num_samples=ns)
        assert want[1].abs().max() == 0 and want[2].abs().max() > 0
    else:
        ratio = torch.tensor(hc.RATIO3)
        want = h(wav.to(dev), ratio.to(dev)).cpu()
        got = composed_forward(cdll, dev, cfg, sd, wav, lens_ratio=ratio)
    assert want.shape == got.shape and bool(torch.isfinite(want).all())
    assert torch.equal(got, want), f'{fixture}: the composed forward differs in {int((got != want).sum())} elements'


# ================================================================================================ refusals

def refusal_case(cdll, dev):
    """every entry point refuses by name and launches nothing: the outputs keep their fill"""
    t = lambda *s, dt=torch.float32: torch.full(s, SENTINEL, dtype=dt, device=dev)   # noqa: E731
    wav, w, y, cs, ws = t(2, 64), t(96, 4), t(2, 31, 96, dt=torch.float16), t(2, 96, 2), t(4096)
    st = _hip.current_stream(wav)

    def refused(rc, what):
        assert rc != 0 and what.encode() in cdll.mv_last_error(), (rc, cdll.mv_last_error())

    l0 = lambda C, k, s, L=64, stride=64, gamma=None, beta=None, wsb=16384: cdll.mv_hfenc_layer0(   # noqa: E731
        wav.data_ptr(), 2, L, stride, None, None, w.data_ptr(), None, gamma, beta, C, k, s, y.data_ptr(), cs.data_ptr(), ws.data_ptr(), wsb, st)
    refused(l0(96, 4, 2), 'multiples of 64 up to 1024')
    refused(l0(2048, 4, 2), 'multiples of 64 up to 1024')
    refused(l0(64, 17, 2), '1 <= k <= 16 and 1 <= s <= 8')
    refused(l0(64, 4, 9), '1 <= k <= 16 and 1 <= s <= 8')
    refused(l0(64, 4, 2, L=3), 'no frame')
    refused(l0(64, 4, 2, stride=63), 'wav_stride below the row length')
    refused(l0(64, 4, 2, gamma=w.data_ptr()), 'gamma and beta come together')
    refused(l0(64, 4, 2, gamma=w.data_ptr(), beta=w.data_ptr(), wsb=8), 'workspace of 2048 bytes')
    rows = lambda x, yy, C, mode, n=2, gamma=w.data_ptr(), eps=1e-5: cdll.mv_hfenc_rows(x, yy, gamma, gamma, eps, n, C, mode, st)   # noqa: E731
    refused(rows(y.data_ptr(), y.data_ptr(), 96, 0), 'multiples of 64 up to 1024')
    refused(rows(y.data_ptr(), y.data_ptr(), 1088, 0), 'multiples of 64 up to 1024')
    refused(rows(y.data_ptr(), y.data_ptr(), 64, 3), 'mode must be')
    refused(rows(y.data_ptr(), y.data_ptr(), 64, 0, n=0), 'n_rows must be positive')
    refused(rows(y.data_ptr(), y.data_ptr(), 64, 1, gamma=None), 'LayerNorm needs gamma and beta')
    refused(rows(y.data_ptr(), y.data_ptr(), 64, 2), 'cannot share')
    refused(rows(y.data_ptr() + 2, y.data_ptr() + 2, 512, 0), '16-byte aligned at C = 512')
    refused(rows(None, y.data_ptr(), 64, 0), 'null argument')
    refused(cdll.mv_hfenc_wave_stats(wav.data_ptr(), 2, 64, 63, None, cs.data_ptr(), st), 'wav_stride below the row length')
    refused(cdll.mv_hfenc_wave_stats(None, 2, 64, 64, None, cs.data_ptr(), st), 'null argument')
    ks, ss = (ctypes.c_int32 * 2)(10, 3), (ctypes.c_int32 * 2)(5, 2)
    ns = torch.zeros(2, dtype=torch.int64, device=dev)
    refused(cdll.mv_hfenc_cmn_mask(ws.data_ptr(), 2, 4, 96, None, None, 0, None, None, 0, 1, st), 'multiples of 64 up to 1024')
    refused(cdll.mv_hfenc_cmn_mask(ws.data_ptr(), 2, 4, 64, cs.data_ptr(), ns.data_ptr(), 0, ks, ss, 2, 1, st), 'not both')
    refused(cdll.mv_hfenc_cmn_mask(ws.data_ptr(), 2, 4, 64, None, ns.data_ptr(), 60, ks, ss, 2, 1, st), 'T is not the frame count')
    refused(cdll.mv_hfenc_cmn_mask(ws.data_ptr(), 2, 4, 64, None, ns.data_ptr(), 60, ks, ss, 9, 1, st), 'num_layers must be')
    refused(cdll.mv_hfenc_cmn_mask(ws.data_ptr(), 2, 0, 64, None, None, 0, None, None, 0, 1, st), 'T must be positive')
    _sync(dev)
    for buf in (y, cs, ws):
        assert bool((buf == SENTINEL).all()), 'a refused call wrote'


if __name__ == '__main__':
    for fam, (cases, _, _) in FAMILIES.items():
        for name in cases:
            model, wrong = model_ratios(fam, name)
            print(f'{fam:7s} {name:32s} model {model:.3f}  ' + '  '.join(f'{m} {r:.3g}' for m, r in wrong.items()))
