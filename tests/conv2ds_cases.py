"""Pinned cases, the fp64 reference and the per-element bound of the conv2ds layer checks: tests/test_conv2ds_kernels.py (CPU: the bound's
self-checks, the plan tests, the cases under the emulator) and tests/test_gpu_conv2ds_kernels.py (device).

conv2ds_launch runs one of the forty rows of csrc/conv2ds.hip's kernel table (CS_KERNELS: conv2ds_kernel<KS, NBW, SPW, MAXT, TRACK>) in a launch
shape that cs_plan picks from the layer, the eight hints of MvConv2dsDesc and the chip's compute-unit count.  A case here NAMES its row and the plan
fields it is about, and uses only knobs that make those fields independent of the compute-unit count (nbw, ct, rows, ring, wgs, spw, nprod, wg, the
operand combination); mv_conv2ds_plan_info -- the plan conv2ds_launch itself makes, nothing restated here -- is asserted for chips of 8, 64, 256
and 304 compute units, and again for the device at hand before the launch.

Reference and bound: see `bound`.  Nothing here comes from device output; `python tests/conv2ds_cases.py` prints, per pinned case, what an fp32
evaluation of the kernel's three-term sum, a reference with one product left out and a reference without the Wlo.Xhi term make of the bound on
the CPU; `python tests/conv2ds_cases.py plan` reprints PRODUCTION_PLAN."""
import re
import types

import torch
import torch.nn.functional as F

import conftest  # noqa: F401  (puts the package on the path when this module runs as a script)
import layer_checks as lc
from conv1d_cases import U32, half_ulp_fp16
from mvector import _hip

PLAN_CUS = (8, 64, 256, 304)    # the emulator's chip, a quarter partition, the MI355X, a larger part
XS = 64.0                       # S16 maps store 64 * value
SAT = 65504.0 / XS              # ... and saturate at |value| = 1023.5
SILU_LIPSCHITZ = 1.1            # max |d/dv v * sigmoid(v)| = 1.0998


# ---- the operands as the kernel holds them, restated in torch (no kernel) -----------------------------------------------------------------------

def split16(t):
    """(hi, lo) fp64 of a map's values as mv_map_split_f32 / the kernel's store split them: V = 64 * value in fp32, clamped to the fp16 range,
    hi = fp16(V), lo = fp16(V - hi) -- the scaled words, not divided by 64"""
    V = (t.float() * XS).clamp(-65504.0, 65504.0)
    hi = V.half()
    lo = (V - hi.float()).half()
    return hi.double(), lo.double()


def pack_weight(o):
    """(Whi, Wlo [cout, cin_k, ks, ks] fp64, oscale) as conv2ds_pack_host makes them of the BatchNorm-folded weight: scaled by the power of two
    that puts the largest magnitude into [512, 1024), hi = fp16(V), lo = fp16(V - hi); oscale = 2^-s / 64"""
    dense = o.wfull * o.bn_scale.view(-1, 1, 1, 1)          # (fp32, as mv_conv2ds_pack_weight folds out_scale)
    mx = dense.abs().max()
    _, e = torch.frexp(mx)
    s = 10 - int(e)
    V = torch.ldexp(dense, torch.tensor(s))
    hi = V.half()
    lo = (V - hi.float()).half()
    return hi.double(), lo.double(), 2.0 ** -s / XS


def packed_words(packed, o):
    """(Whi, Wlo) decoded from the buffer mv_conv2ds_pack_weight filled: [cout16][taps][units][hi 16 | lo 16] fp16"""
    taps, units = o.ks * o.ks, -(-o.cin_k // 32) * 2
    h = packed.cpu().contiguous().view(torch.float16).reshape(o.c16, taps, units, 2, 16)
    dec = lambda part: h[:, :, :, part, :].reshape(o.c16, taps, units * 16)[:o.cout, :, :o.cin_k].permute(0, 2, 1).reshape(o.cout, o.cin_k, o.ks, o.ks).double()
    return dec(0), dec(1)


def _inputs(o):
    """(Xhi, Xlo) [B, cin_k, H, W] fp64: the input channels in the packed weight's order"""
    if o.concat:
        r = -(-o.cin_a // 16) * 16
        x = torch.cat([o.xa[..., :r], o.xb[..., :r]], dim=-1)
    else:
        x = o.xa[..., :o.cin_k]
    hi, lo = split16(x)
    return hi.permute(0, 3, 1, 2), lo.permute(0, 3, 1, 2)


def _operand(t, o):
    """an epilogue operand's value as the kernel decodes it: (hi + lo) / 64"""
    if t is None:
        return None
    hi, lo = split16(t[..., :o.cout])
    return (hi + lo) / XS


def split_error(v):
    """what the store's split loses of a value of magnitude v (fp64, >= 0): X = 64 v is stored as hi = fp16(X), lo = fp16(X - hi);
    |X - hi| <= half_ulp(X) and lo is within half_ulp(|X - hi|) of it, never finer than half the subnormal spacing 2^-24"""
    return half_ulp_fp16(half_ulp_fp16(v * XS)) / XS


def bound(pre, S, n, o, r1, r2, add):
    """(ref, bound, ref2, bound2), fp64 [B, Ho, Wo, cout]: the layer's outputs y and y2 (None without a second output) over `pre` = the kernel's
    three-term sum Whi.Xhi + Whi.Xlo + Wlo.Xhi times oscale, plus the bias, evaluated in fp64 on the operands as the kernel holds them (the
    fp16 pairs of the S16 input, the pairs mv_conv2ds_pack_weight made of the weights); S = the same sum on absolute values, n = cin * ks^2.

    The bound, per output element (derived, not measured), in the domain of the map's values:
      * accumulation: the products of two fp16 values are exact in fp32.  Summing the 3 n products and the bias in fp32 IN ANY ORDER errs by at most
        (3 n + 1) u S to first order, u = 2^-24 (every partial sum is bounded by S; Higham, Accuracy and Stability, eq. 4.4).  Taken as
        acc = (3 n + 2) * 2^-23 * S: doubled, because the rounding of the MFMA's internal adder is not documented as round-to-nearest (the same
        unit tests/conv1d_cases.py uses).  The scaling by oscale * 64 is a power of two: exact.
      * the epilogue carries acc through maps with Lipschitz constants clamp 1, SiLU 1.1, tanh 1; the AFF mix r1 (1 + th) + r2 (1 - th) moves by
        (|r1| + |r2|) per unit of th.
      * the epilogue's own fp32 roundings, each a correctly rounded operation (u relative) unless noted, taken twice:
          clamp (+ residual): the fma with the bias u |pre|, the operand's hi + lo u |r1|, the sum u |pre + r1|:  4 u (|pre| + |r1|)
          SiLU: the fma 1.1 * 2 u |pre|; expf (a few ulp), 1 + e, the division, on a result of magnitude |ref|:  8 u |ref|
          AFF: the fma and tanhf (a few ulp of a value <= 1), 1 +- th, two products, the sum:  (|r1| + |r2|) (2 u |pre| + 16 u)
        e = the sum of the two.  The store clamps to +-1023.5 and splits a value within e of ref:  bound = e + split_error(|ref| + e).
      * second output: the clamped y (before its split) + add, both decoded exactly, one rounded sum: e2 = e + 4 u (|ref| + |add|),
        bound2 = e2 + split_error(|ref2| + e2)."""
    acc = (3 * n + 2) * 2.0 * U32 * S
    if o.epi == 0:
        v = pre if r1 is None else pre + r1
        e = acc + 4.0 * U32 * (pre.abs() + (0.0 if r1 is None else r1.abs()))
        v = v.clamp(o.lo, o.hi)
    elif o.epi == 1:
        v = F.silu(pre)
        e = SILU_LIPSCHITZ * (acc + 2.0 * U32 * pre.abs()) + 8.0 * U32 * v.abs()
    else:
        th = torch.tanh(pre)
        v = r1 * (1.0 + th) + r2 * (1.0 - th)
        e = (r1.abs() + r2.abs()) * (acc + 2.0 * U32 * pre.abs() + 16.0 * U32)
    v = v.clamp(-SAT, SAT)
    bnd = e + split_error(v.abs() + e)
    if add is None:
        return v, bnd, None, None
    v2 = (v + add).clamp(-SAT, SAT)
    e2 = e + 4.0 * U32 * (v.abs() + add.abs())
    return v, bnd, v2, e2 + split_error(v2.abs() + e2)


def reference(o, drop=None, weights=None):
    """(ref, bound, ref2, bound2) of the conv2ds_case operands `o` (lc.conv2ds_operands).  drop: the deliberately wrong references of the
    self-checks -- 'product': the whole product of the last input channel at tap (0, 0) is missing from every output sum; 'cross': the Wlo.Xhi
    term is.  weights: (Whi, Wlo, oscale) decoded from the packed buffer instead of the restated packing."""
    xhi, xlo = _inputs(o)
    whi, wlo, oscale = weights or pack_weight(o)
    conv = lambda x_, w_: F.conv2d(x_, w_, None, stride=(o.stride, o.sw), padding=o.p).permute(0, 2, 3, 1)
    # Whi.(Xhi + Xlo) + Wlo.Xhi as one convolution over twice the channels (hi + lo of an fp16 pair is exact in fp64)
    two = lambda a, b: torch.cat([a, b], dim=1)
    wl = torch.zeros_like(wlo) if drop == 'cross' else wlo
    bias = o.bias.double()
    pre = conv(two(xhi + xlo, xhi), two(whi, wl)) * oscale + bias
    S = conv(two(xhi.abs() + xlo.abs(), xhi.abs()), two(whi.abs(), wlo.abs())) * oscale + bias.abs()
    if drop == 'product':
        c = o.cin_k - 1 if not o.concat else -(-o.cin_a // 16) * 16 + o.cin_a - 1     # the last channel that carries weights
        w1, w2 = torch.zeros_like(whi), torch.zeros_like(wlo)
        w1[:, c, 0, 0], w2[:, c, 0, 0] = whi[:, c, 0, 0], wlo[:, c, 0, 0]
        pre = pre - conv(two(xhi + xlo, xhi), two(w1, w2)) * oscale
    return bound(pre, S, o.cin * o.ks * o.ks, o, _operand(o.res, o), _operand(o.res2, o), _operand(o.add, o))


def store16(v32):
    """a fp32 value as the kernel stores it and a reader decodes it, fp64"""
    hi, lo = split16(v32)
    return (hi + lo) / XS


def model32(o):
    """(y, y2) of the fp32 rounding model: the three-term sum, the epilogue and the second output evaluated in fp32, stored as the kernel stores"""
    xhi, xlo = _inputs(o)
    whi, wlo, oscale = pack_weight(o)
    conv = lambda x_, w_: F.conv2d(x_.float(), w_.float(), None, stride=(o.stride, o.sw), padding=o.p).permute(0, 2, 3, 1)
    pre = (conv(xhi, whi) + conv(xlo, whi) + conv(xhi, wlo)) * float(oscale) + o.bias
    f = lambda t: None if t is None else _operand(t, o).float()
    r1, r2, add = f(o.res), f(o.res2), f(o.add)
    if o.epi == 0:
        v = (pre if r1 is None else pre + r1).clamp(o.lo, o.hi)
    elif o.epi == 1:
        v = pre / (1.0 + torch.exp(-pre))
    else:
        th = torch.tanh(pre)
        v = r1 * (1.0 + th) + r2 * (1.0 - th)
    v = v.clamp(-SAT, SAT)
    return store16(v), (None if add is None else store16(v + add))


def ratios(got, ref64, bnd):
    """(max ratio, mean ratio, median bound) of |got - ref64| / bound"""
    r = (got.double() - ref64).abs() / bnd
    return r.max().item(), r.mean().item(), bnd.median().item()


def decode(buf, o):
    """the values of an S16 output buffer's channel slice, from its words, fp64"""
    hi, lo = lc.s16_words(buf)
    return ((hi + lo) / XS)[..., :o.cout]


def assert_within_bound(o, y, y2, kernel='', tag='', log=None, device_x=None, device_w=None):
    """lc.conv2ds_case's hook: every element of y (and y2) within its bound of the fp64 reference.  device_x / device_w: the S16 operands and the
    packed weights the launch read -- they must hold the words the reference restates (so the reference IS on the kernel's operands)."""
    weights = None
    if device_w is not None:
        whi, wlo = packed_words(device_w[0], o)
        rhi, rlo, oscale = pack_weight(o)
        assert torch.equal(whi, rhi) and torch.equal(wlo, rlo) and device_w[1] == oscale, f'{tag}: mv_conv2ds_pack_weight and its restatement differ'
        weights = (whi, wlo, device_w[1])
    for buf, t in zip(device_x or (), (o.xa, o.xb, o.res, o.res2, o.add)):
        if t is not None:
            hi, lo = lc.s16_words(buf)
            rhi, rlo = split16(t)
            assert torch.equal(hi, rhi) and torch.equal(lo, rlo), f'{tag}: mv_map_split_f32 and its restatement differ'
    ref, bnd, ref2, bnd2 = reference(o, weights=weights)
    worst = 0.0
    for name, buf, r, b in (('y', y, ref, bnd), ('y2', y2, ref2, bnd2)):
        if buf is None:
            continue
        mx, mean, med = ratios(decode(buf, o), r, b)
        if log is not None:
            log(f'conv2ds bound {tag:28s} {name:2s} {kernel:42s} max ratio {mx:.3f}  mean ratio {mean:.3f}  median bound {med:.2e}')
        assert mx <= 1.0, f'{tag} {kernel} {name}: |got - ref64| / bound reaches {mx:.3f} (mean {mean:.3f}, median bound {med:.2e})'
        worst = max(worst, mx)
    return worst


PINNED = {}
_C = lc.CONV2DS_CASES
_T = dict(peak=True, lo=0.0, hi=3.0e38)        # TRACK: a peak word, and nothing clamped above so that the word is the map's maximum
EPILOGUES = {
    'clamp': dict(),
    'clamp_res': dict(with_res=True),
    'clamp_sum': dict(with_sum=True),
    'silu': dict(epi=1),
    'aff': dict(epi=2),
}


def _row_cases():
    """one case per row of the kernel table: 32 -> 16 * NBW channels (one channel group), 2 x 6 x 20 pixels -- 3x3: four tiles of <= 3 rows per
    utterance, the last with one row, 20 = 16 + 4 columns; 1x1: 120 of a tile's 128 pixels -- on two workgroups.  The epilogues take turns, so
    that each runs with one and with several blocks per wave (test_every_epilogue_runs_with_one_and_with_several_blocks_per_wave)."""
    out, i = {}, 0
    for ks in (1, 3):
        for nbw, spw in ((1, 8), (1, 4), (1, 2), (1, 1), (2, 8), (2, 4), (2, 2), (3, 8), (3, 4), (3, 2)):
            for track in (False, True):
                epi = list(EPILOGUES)[i % len(EPILOGUES)]
                i += 1
                cfg = dict(ks=ks, cin=32, cout=16 * nbw, nbw=nbw, spw=spw, H=6, W=20, B=2, wg=2, **EPILOGUES[epi])
                if ks == 3:
                    cfg['rows'] = 3
                if track:
                    cfg.update(_T)
                out[f'row_k{ks}_b{nbw}_s{spw}_{"track" if track else "plain"}_{epi}'] = cfg
            i += 1     # (the two TRACK forms of a shape get different epilogues, and the next shape starts one further)
    return out


_WALK3 = dict(ks=3, cout=32, H=10, W=37, B=2, rows=2, wg=4)      # 15 tiles per utterance, 30 in all, on 4 workgroups: 8, 8, 7, 7 tiles each
_WALK1 = dict(ks=1, cout=48, H=10, W=37, B=3, wg=2)              # 370 pixels: 3 tiles per utterance (the last of 114 pixels), 9 in all: 5 and 4
CONFIGS = {
    **_row_cases(),
    # ---- the walk: one ring through the stages of consecutive tiles, across utterance boundaries, workgroups that stop a round early ----
    'walk3_ring2_1_stage': dict(_WALK3, cin=32, ring=2),
    'walk3_ring2_1_stage_track': dict(_WALK3, cin=32, ring=2, **_T),
    'walk3_ring3_2_stages': dict(_WALK3, cin=64, ring=3),                       # stages per tile = ns - 1
    'walk3_ring3_2_stages_track': dict(_WALK3, cin=64, ring=3, **_T),
    'walk3_ring_max_5_stages': dict(_WALK3, cin=160, wgs=1),                    # the deepest ring (4), more stages per tile than slots
    'walk3_ring_max_5_stages_track': dict(_WALK3, cin=160, wgs=1, **_T),
    'walk1_ring2_1_stage': dict(_WALK1, cin=96, ring=2),                        # stages per tile = ns - 1
    'walk1_ring2_1_stage_track': dict(_WALK1, cin=96, ring=2, **_T),
    'walk1_ring2_3_stages': dict(_WALK1, cin=208, ring=2),                      # 13 units: 7 chunks, the last half empty; 3 stages > ns
    'walk1_ring3_2_stages': dict(_WALK1, cin=160, ring=3),                      # stages per tile = ns - 1
    'walk1_ring3_2_stages_track': dict(_WALK1, cin=160, ring=3, **_T),
    'walk1_ring_max_4_stages': dict(_WALK1, cin=320, cout=16),                  # the deepest ring of a 1x1 layer (3), 4 stages per tile
    'walk1_ring_max_4_stages_track': dict(_WALK1, cin=320, cout=16, **_T),
    # ---- producer forms: 15 transfers per stage (5 patch rows x 3 column groups) on 1, 2 and 4 producer waves ----
    'producers_1': dict(ks=3, cin=32, cout=32, H=10, W=37, B=2, rows=3, wg=5, nprod=1),
    'producers_2_padded': dict(ks=3, cin=32, cout=32, H=10, W=37, B=2, rows=3, wg=5, nprod=2),     # 8 + 7: one padding transfer to the dump KiB
    'producers_4_padded': dict(ks=3, cin=32, cout=32, H=10, W=37, B=2, rows=3, wg=5, nprod=4, wgs=1),     # 4 + 4 + 4 + 3
    'producers_4_1x1': dict(ks=1, cin=64, cout=96, H=10, W=37, B=2, nbw=2, wg=2),                  # 48 transfers on four waves
    'producers_3': dict(ks=3, cin=32, cout=48, H=10, W=37, B=2, rows=3, wg=5, nbw=3, spw=8),       # the wave limit leaves three of four
    'six_consumers_two_producers': dict(_C[22], wg=2),
    'six_consumers_four_stages': dict(_C[23], wg=2),
    # ---- ragged geometry (the configurations of the layer checks, their launch shape pinned where it followed the chip) ----
    'padded_13_second_out': dict(_C[1], rows=3, wg=7),                           # cout 13; Wo = 37, Ho = 10 = 3 + 3 + 3 + 1
    'strided_1x1': dict(_C[2], wg=2),
    'strided_1x1_odd': dict(_C[12], wg=2),                                      # 5 x 37 -> 3 x 19
    'strided_3x3_odd': dict(_C[13], rows=2, wg=3),                              # 5 x 33 -> 3 x 17
    'strided_3x3_no_clamp': dict(_C[3], rows=2, wg=7),                          # 9 x 150 -> 5 x 75
    'freq_stride_3x3': dict(_C[34], rows=2, wg=7),                              # stride on the frequency axis only
    'freq_stride_1x1': dict(_C[35], wg=3),
    'concat_silu': dict(_C[5], wg=4),
    'concat_straddle': dict(_C[6], wg=4),                                       # a K chunk with one unit of each source
    'aff_four_blocks': dict(_C[7], wg=4),
    'odd_units_104': dict(_C[8], rows=2, wg=5),                                 # 13 units of input: a half-empty last K chunk; cout 104
    'three_channel_tiles': dict(_C[16], wg=2),                                  # the last channel tile has 4 of 6 blocks
    'channel_tiles_3x3_rows_3': dict(_C[17], wg=4),
    'thirteen_blocks_residual': dict(_C[11], wg=2),
    'three_blocks_unsplit_pixels': dict(_C[30], rows=4, wg=5),
    'large_activations': dict(_C[37], rows=3, wg=3),
    # ---- the peak word with a second output that is the larger map ----
    'peak_second_out_b1': dict(ks=3, cin=32, cout=32, H=10, W=37, B=2, rows=3, wg=5, with_sum=True, add_scale=8.0, **_T),
    'peak_second_out_b2': dict(ks=1, cin=64, cout=64, H=10, W=37, B=2, nbw=2, spw=4, wg=2, with_sum=True, add_scale=8.0, **_T),
    'peak_second_out_b3': dict(ks=3, cin=48, cout=48, H=10, W=37, B=2, rows=3, wg=5, nbw=3, spw=4, with_sum=True, add_scale=8.0, **_T),
    # ---- a NaN input reaches exactly the outputs that read it, with several blocks per wave ----
    'nan_3x3_b2': dict(ks=3, cin=32, cout=32, H=6, W=20, B=1, rows=3, wg=2, nbw=2, spw=8, lo=0.0, hi=3.0e38, nan_at=(0, 2, 5, 3)),
    'nan_3x3_b3_track': dict(ks=3, cin=32, cout=48, H=6, W=20, B=1, rows=3, wg=2, nbw=3, spw=4, nan_at=(0, 2, 17, 30), **_T),
    'nan_silu_b2_track': dict(ks=1, cin=32, cout=32, H=6, W=20, B=1, wg=1, nbw=2, spw=4, epi=1, nan_at=(0, 2, 5, 3), peak=True),
    'nan_aff_b2_track': dict(ks=1, cin=32, cout=32, H=4, W=20, B=1, wg=1, nbw=2, spw=2, epi=2, nan_at=(0, 1, 7, 30), peak=True),
}
FIELDS = ('kernel', 'ncons', 'nprod', 'ns', 'pp', 'wgs_per_cu', 'rows', 'ct', 'ctiles', 'tiles', 'wg_per_ct', 'stages_per_tile')


def kernel_name(ks, nbw, spw, track):
    return f'conv2ds_kernel<{ks}, {nbw}, {spw}, {768 if nbw == 1 else 512}, {"true" if track else "false"}>'


# name -> (the table row's parameters, ncons, nprod, ns, pp, wgs_per_cu, rows, ct, ctiles, tiles, wg_per_ct, stages_per_tile): the plan every chip makes
EXPECT = {
    'row_k1_b1_s8_plain_clamp': ('1, 1, 8, 768, false', 1, 2, 3, 24, 1, 8, 1, 1, 1, 2, 1),
    'row_k1_b1_s8_track_clamp_res': ('1, 1, 8, 768, true', 1, 2, 3, 24, 1, 8, 1, 1, 1, 2, 1),
    'row_k1_b1_s4_plain_silu': ('1, 1, 4, 768, false', 2, 2, 3, 24, 1, 8, 1, 1, 1, 2, 1),
    'row_k1_b1_s4_track_aff': ('1, 1, 4, 768, true', 2, 2, 3, 24, 1, 8, 1, 1, 1, 2, 1),
    'row_k1_b1_s2_plain_clamp_res': ('1, 1, 2, 768, false', 4, 2, 3, 24, 1, 8, 1, 1, 1, 2, 1),
    'row_k1_b1_s2_track_clamp_sum': ('1, 1, 2, 768, true', 4, 2, 3, 24, 1, 8, 1, 1, 1, 2, 1),
    'row_k1_b1_s1_plain_aff': ('1, 1, 1, 768, false', 8, 2, 3, 24, 1, 8, 1, 1, 1, 2, 1),
    'row_k1_b1_s1_track_clamp': ('1, 1, 1, 768, true', 8, 2, 3, 24, 1, 8, 1, 1, 1, 2, 1),
    'row_k1_b2_s8_plain_clamp_sum': ('1, 2, 8, 512, false', 1, 2, 3, 24, 1, 8, 2, 1, 1, 2, 1),
    'row_k1_b2_s8_track_silu': ('1, 2, 8, 512, true', 1, 4, 3, 12, 1, 8, 2, 1, 1, 2, 1),
    'row_k1_b2_s4_plain_clamp': ('1, 2, 4, 512, false', 2, 4, 3, 12, 1, 8, 2, 1, 1, 2, 1),
    'row_k1_b2_s4_track_clamp_res': ('1, 2, 4, 512, true', 2, 2, 3, 24, 1, 8, 2, 1, 1, 2, 1),
    'row_k1_b2_s2_plain_silu': ('1, 2, 2, 512, false', 4, 4, 3, 12, 1, 8, 2, 1, 1, 2, 1),
    'row_k1_b2_s2_track_aff': ('1, 2, 2, 512, true', 4, 2, 3, 24, 1, 8, 2, 1, 1, 2, 1),
    'row_k1_b3_s8_plain_clamp_res': ('1, 3, 8, 512, false', 1, 4, 3, 12, 1, 8, 3, 1, 1, 2, 1),
    'row_k1_b3_s8_track_clamp_sum': ('1, 3, 8, 512, true', 1, 4, 3, 12, 1, 8, 3, 1, 1, 2, 1),
    'row_k1_b3_s4_plain_aff': ('1, 3, 4, 512, false', 2, 4, 3, 12, 1, 8, 3, 1, 1, 2, 1),
    'row_k1_b3_s4_track_clamp': ('1, 3, 4, 512, true', 2, 4, 3, 12, 1, 8, 3, 1, 1, 2, 1),
    'row_k1_b3_s2_plain_clamp_sum': ('1, 3, 2, 512, false', 4, 4, 3, 12, 1, 8, 3, 1, 1, 2, 1),
    'row_k1_b3_s2_track_silu': ('1, 3, 2, 512, true', 4, 4, 3, 12, 1, 8, 3, 1, 1, 2, 1),
    'row_k3_b1_s8_plain_clamp': ('3, 1, 8, 768, false', 1, 2, 4, 8, 2, 3, 1, 1, 4, 2, 1),
    'row_k3_b1_s8_track_clamp_res': ('3, 1, 8, 768, true', 1, 2, 4, 8, 2, 3, 1, 1, 4, 2, 1),
    'row_k3_b1_s4_plain_silu': ('3, 1, 4, 768, false', 2, 2, 4, 8, 2, 3, 1, 1, 4, 2, 1),
    'row_k3_b1_s4_track_aff': ('3, 1, 4, 768, true', 2, 2, 4, 8, 2, 3, 1, 1, 4, 2, 1),
    'row_k3_b1_s2_plain_clamp_res': ('3, 1, 2, 768, false', 4, 2, 4, 8, 2, 3, 1, 1, 4, 2, 1),
    'row_k3_b1_s2_track_clamp_sum': ('3, 1, 2, 768, true', 4, 2, 4, 8, 2, 3, 1, 1, 4, 2, 1),
    'row_k3_b1_s1_plain_aff': ('3, 1, 1, 768, false', 8, 2, 4, 8, 1, 3, 1, 1, 4, 2, 1),
    'row_k3_b1_s1_track_clamp': ('3, 1, 1, 768, true', 8, 2, 4, 8, 1, 3, 1, 1, 4, 2, 1),
    'row_k3_b2_s8_plain_clamp_sum': ('3, 2, 8, 512, false', 1, 2, 4, 8, 2, 3, 2, 1, 4, 2, 1),
    'row_k3_b2_s8_track_silu': ('3, 2, 8, 512, true', 1, 3, 4, 5, 2, 3, 2, 1, 4, 2, 1),
    'row_k3_b2_s4_plain_clamp': ('3, 2, 4, 512, false', 2, 2, 4, 8, 2, 3, 2, 1, 4, 2, 1),
    'row_k3_b2_s4_track_clamp_res': ('3, 2, 4, 512, true', 2, 2, 4, 8, 2, 3, 2, 1, 4, 2, 1),
    'row_k3_b2_s2_plain_silu': ('3, 2, 2, 512, false', 4, 4, 4, 4, 1, 3, 2, 1, 4, 2, 1),
    'row_k3_b2_s2_track_aff': ('3, 2, 2, 512, true', 4, 2, 4, 8, 1, 3, 2, 1, 4, 2, 1),
    'row_k3_b3_s8_plain_clamp_res': ('3, 3, 8, 512, false', 1, 3, 4, 5, 2, 3, 3, 1, 4, 2, 1),
    'row_k3_b3_s8_track_clamp_sum': ('3, 3, 8, 512, true', 1, 3, 4, 5, 2, 3, 3, 1, 4, 2, 1),
    'row_k3_b3_s4_plain_aff': ('3, 3, 4, 512, false', 2, 2, 4, 8, 2, 3, 3, 1, 4, 2, 1),
    'row_k3_b3_s4_track_clamp': ('3, 3, 4, 512, true', 2, 2, 4, 8, 2, 3, 3, 1, 4, 2, 1),
    'row_k3_b3_s2_plain_clamp_sum': ('3, 3, 2, 512, false', 4, 4, 4, 4, 1, 3, 3, 1, 4, 2, 1),
    'row_k3_b3_s2_track_silu': ('3, 3, 2, 512, true', 4, 4, 4, 4, 1, 3, 3, 1, 4, 2, 1),
    'walk3_ring2_1_stage': ('3, 1, 4, 768, false', 4, 2, 2, 6, 2, 2, 2, 1, 15, 4, 1),
    'walk3_ring2_1_stage_track': ('3, 1, 4, 768, true', 4, 2, 2, 6, 2, 2, 2, 1, 15, 4, 1),
    'walk3_ring3_2_stages': ('3, 1, 4, 768, false', 4, 2, 3, 6, 2, 2, 2, 1, 15, 4, 2),
    'walk3_ring3_2_stages_track': ('3, 1, 4, 768, true', 4, 2, 3, 6, 2, 2, 2, 1, 15, 4, 2),
    'walk3_ring_max_5_stages': ('3, 1, 4, 768, false', 4, 2, 4, 6, 1, 2, 2, 1, 15, 4, 5),
    'walk3_ring_max_5_stages_track': ('3, 1, 4, 768, true', 4, 2, 4, 6, 1, 2, 2, 1, 15, 4, 5),
    'walk1_ring2_1_stage': ('1, 1, 4, 768, false', 6, 2, 2, 24, 1, 8, 3, 1, 3, 2, 1),
    'walk1_ring2_1_stage_track': ('1, 1, 4, 768, true', 6, 2, 2, 24, 1, 8, 3, 1, 3, 2, 1),
    'walk1_ring2_3_stages': ('1, 1, 4, 768, false', 6, 2, 2, 24, 1, 8, 3, 1, 3, 2, 3),
    'walk1_ring3_2_stages': ('1, 1, 4, 768, false', 6, 2, 3, 24, 1, 8, 3, 1, 3, 2, 2),
    'walk1_ring3_2_stages_track': ('1, 1, 4, 768, true', 6, 2, 3, 24, 1, 8, 3, 1, 3, 2, 2),
    'walk1_ring_max_4_stages': ('1, 1, 4, 768, false', 2, 2, 3, 24, 1, 8, 1, 1, 3, 2, 4),
    'walk1_ring_max_4_stages_track': ('1, 1, 4, 768, true', 2, 2, 3, 24, 1, 8, 1, 1, 3, 2, 4),
    'producers_1': ('3, 1, 4, 768, false', 4, 1, 4, 15, 2, 3, 2, 1, 12, 5, 1),
    'producers_2_padded': ('3, 1, 4, 768, false', 4, 2, 4, 8, 2, 3, 2, 1, 12, 5, 1),
    'producers_4_padded': ('3, 1, 4, 768, false', 4, 4, 4, 4, 1, 3, 2, 1, 12, 5, 1),
    'producers_4_1x1': ('1, 2, 8, 512, false', 3, 4, 3, 12, 1, 8, 6, 1, 3, 2, 1),
    'producers_3': ('3, 3, 8, 512, false', 1, 3, 4, 5, 2, 3, 3, 1, 12, 5, 1),
    'six_consumers_two_producers': ('1, 2, 8, 512, false', 6, 2, 3, 24, 1, 8, 12, 1, 3, 2, 1),
    'six_consumers_four_stages': ('1, 2, 8, 512, false', 6, 2, 3, 24, 1, 8, 12, 1, 3, 2, 4),
    'padded_13_second_out': ('3, 1, 4, 768, false', 2, 2, 4, 8, 2, 3, 1, 1, 12, 7, 1),
    'strided_1x1': ('1, 2, 2, 512, false', 4, 4, 3, 12, 1, 8, 2, 1, 1, 2, 1),
    'strided_1x1_odd': ('1, 1, 4, 768, false', 6, 2, 3, 24, 1, 8, 3, 1, 1, 2, 1),
    'strided_3x3_odd': ('3, 1, 4, 768, false', 4, 2, 3, 13, 2, 2, 2, 1, 4, 3, 1),
    'strided_3x3_no_clamp': ('3, 2, 8, 512, false', 4, 4, 4, 7, 1, 2, 8, 1, 15, 7, 2),
    'freq_stride_3x3': ('3, 1, 4, 768, false', 4, 2, 4, 8, 2, 2, 2, 1, 9, 7, 1),
    'freq_stride_1x1': ('1, 2, 2, 512, false', 4, 4, 3, 12, 1, 8, 2, 1, 2, 3, 1),
    'concat_silu': ('1, 1, 4, 768, false', 2, 2, 3, 24, 1, 8, 1, 1, 3, 4, 2),
    'concat_straddle': ('1, 1, 4, 768, false', 2, 2, 3, 24, 1, 8, 1, 1, 3, 4, 1),
    'aff_four_blocks': ('1, 1, 4, 768, false', 8, 2, 3, 24, 1, 8, 4, 1, 3, 4, 1),
    'odd_units_104': ('3, 1, 8, 768, false', 7, 2, 4, 6, 1, 2, 7, 1, 9, 5, 4),
    'three_channel_tiles': ('1, 2, 8, 512, false', 3, 4, 3, 12, 1, 8, 6, 3, 2, 2, 1),
    'channel_tiles_3x3_rows_3': ('3, 2, 8, 512, false', 3, 1, 4, 15, 2, 3, 6, 2, 6, 4, 2),
    'thirteen_blocks_residual': ('1, 2, 8, 512, false', 4, 2, 3, 24, 1, 8, 7, 2, 1, 2, 1),
    'three_blocks_unsplit_pixels': ('3, 1, 8, 768, false', 3, 2, 4, 9, 2, 4, 3, 1, 12, 5, 2),
    'large_activations': ('3, 1, 4, 768, false', 4, 2, 4, 8, 2, 3, 2, 1, 4, 3, 1),
    'peak_second_out_b1': ('3, 1, 4, 768, true', 4, 2, 4, 8, 2, 3, 2, 1, 12, 5, 1),
    'peak_second_out_b2': ('1, 2, 4, 512, true', 4, 2, 3, 24, 1, 8, 4, 1, 3, 2, 1),
    'peak_second_out_b3': ('3, 3, 4, 512, true', 2, 2, 4, 8, 2, 3, 3, 1, 12, 5, 2),
    'nan_3x3_b2': ('3, 2, 8, 512, false', 1, 3, 4, 5, 2, 3, 2, 1, 4, 2, 1),
    'nan_3x3_b3_track': ('3, 3, 4, 512, true', 2, 2, 4, 8, 2, 3, 3, 1, 4, 2, 1),
    'nan_silu_b2_track': ('1, 2, 4, 512, true', 2, 4, 3, 12, 1, 8, 2, 1, 1, 1, 1),
    'nan_aff_b2_track': ('1, 2, 2, 512, true', 4, 2, 3, 24, 1, 8, 2, 1, 1, 1, 1),
}


def _expect(row):
    e = dict(zip(FIELDS, row))
    ks, nbw, spw, _, track = re.fullmatch(r'(\d), (\d), (\d), (\d+), (true|false)', row[0]).groups()
    e.update(kernel=f'conv2ds_kernel<{row[0]}>', nbw=int(nbw), spw=int(spw), track=int(track == 'true'), grid=e['wg_per_ct'] * e['ctiles'])
    assert e['kernel'] == kernel_name(int(ks), int(nbw), int(spw), track == 'true')
    return e


PINNED = {name: dict(cfg=cfg, expect=_expect(EXPECT[name])) for name, cfg in CONFIGS.items()}
# rows of the kernel table that no admissible combination of hints reaches -> the refusal that proves it (none: every row has a pinned case.  What
# the hints cannot ask for is no row either: one segment per wave with several blocks per wave)
UNREACHABLE = {}
NOT_ROWS = {(ks, nbw, 1): 'segments per wave must be 8, 4, 2 (or 1 with one block per wave)' for ks in (1, 3) for nbw in (2, 3)}
WALKS = [n for n in PINNED if n.startswith('walk')]
# 10 s and more each under the emulator: MV_SLOW_EMU=1 (the device tier runs them all)
SLOW_EMU = ('walk3_ring_max_5_stages', 'walk3_ring_max_5_stages_track')


def seed_of(name):
    return list(PINNED).index(name) + 200


def operands(name):
    cfg = {k: v for k, v in PINNED[name]['cfg'].items() if k in lc.conv2ds_operands.__code__.co_varnames}
    return lc.conv2ds_operands(seed=seed_of(name), **cfg)


def plans(cdll, name, cus=PLAN_CUS):
    """{cus: mv_conv2ds_plan_info} of the case's own descriptor (lc.conv2ds_case builds it; nothing is launched)"""
    return lc.conv2ds_case(cdll, 'cpu', seed=seed_of(name), plan_cus=cus, **PINNED[name]['cfg'])


def run(cdll, device, name, log=print):
    """plan asserted for the device at hand, launch, conv2ds_case's assertions, the bound"""
    return lc.conv2ds_case(cdll, device, seed=seed_of(name), expect=PINNED[name]['expect'], tag=name, log=log, **PINNED[name]['cfg'])


# ---- one sum whatever the shape (conv2ds.hip: "none changes a bit of the result -- every output element is the same K-ordered sum in every shape") ----
# name -> (the layer, [launch form: the hints; the row follows from ks, nbw, spw]).  Every form runs with and without a peak word.
SAME_BITS = {
    '3x3': (dict(ks=3, cin=32, cout=48, H=9, W=21, B=3), [
        dict(nbw=1, spw=8, rows=2, wg=7), dict(nbw=1, spw=8, rows=3, ring=2, wg=4, nprod=1), dict(nbw=1, spw=2, ct=2, rows=4, ring=3, wg=5),
        dict(nbw=2, spw=8, rows=5, wg=3, wgs=1), dict(nbw=2, spw=4, rows=8, wg=2, nprod=2), dict(nbw=3, spw=8, rows=1, wg=11),
        dict(nbw=3, spw=4, rows=7, wg=3, ring=2), dict(nbw=3, spw=2, rows=3, wg=18)]),
    '3x3_stride2': (dict(ks=3, stride=2, cin=32, cout=48, H=11, W=37, B=2, lo=-65504.0, hi=65504.0), [
        dict(nbw=1, spw=8, rows=1, wg=5), dict(nbw=1, spw=8, rows=5, ring=2, wg=2), dict(nbw=2, spw=8, rows=2, wg=4, nprod=1),
        dict(nbw=2, spw=4, rows=3, wg=3, wgs=1), dict(nbw=3, spw=4, rows=4, wg=8), dict(nbw=3, spw=2, rows=2, wg=7, nprod=2)]),
    '1x1': (dict(ks=1, cin=96, cout=48, H=10, W=37, B=2), [
        dict(nbw=1, spw=8, wg=6), dict(nbw=1, spw=4, ring=2, wg=2), dict(nbw=1, spw=2, ct=2, wg=4), dict(nbw=1, spw=1, ct=1, wg=5),
        dict(nbw=2, spw=8, wg=1), dict(nbw=2, spw=2, ct=2, wg=3, nprod=2), dict(nbw=3, spw=4, ring=2, wg=4), dict(nbw=3, spw=2, wg=2)]),
    '1x1_residual_second_out': (dict(ks=1, cin=64, cout=48, H=10, W=37, B=2, with_res=True, with_sum=True), [
        dict(nbw=1, spw=8, wg=6), dict(nbw=1, spw=2, ct=2, ring=2, wg=2), dict(nbw=2, spw=8, wg=4), dict(nbw=2, spw=4, wg=1),
        dict(nbw=3, spw=8, wg=3), dict(nbw=3, spw=2, ring=2, wg=5)]),
    'concat_silu': (dict(ks=1, cin=96, cout=48, H=10, W=37, B=2, concat=True, epi=1), [
        dict(nbw=1, spw=8, wg=6), dict(nbw=1, spw=4, ring=2, wg=2), dict(nbw=2, spw=8, wg=3), dict(nbw=2, spw=4, wg=4, nprod=2),
        dict(nbw=3, spw=4, wg=1), dict(nbw=3, spw=2, ring=2, wg=5)]),
    'aff': (dict(ks=1, cin=32, cout=48, H=10, W=37, B=2, epi=2), [
        dict(nbw=1, spw=8, wg=6), dict(nbw=1, spw=2, ct=2, ring=2, wg=2), dict(nbw=2, spw=8, wg=3), dict(nbw=2, spw=2, ct=2, wg=4),
        dict(nbw=3, spw=8, wg=1), dict(nbw=3, spw=4, ring=2, wg=5)]),
}
ALONE = '3x3'      # this group also launches every utterance of its batch alone
# 10 s and more under the emulator: MV_SLOW_EMU=1 (the device tier runs them all); '3x3_small' is the emulator's everyday 3x3 group
SAME_BITS['3x3_small'] = (dict(ks=3, cin=16, cout=48, H=5, W=18, B=2), [
    dict(nbw=1, spw=8, rows=2, wg=3), dict(nbw=2, spw=4, rows=5, ring=2, wg=2), dict(nbw=3, spw=8, rows=1, wg=7, nprod=1), dict(nbw=3, spw=2, rows=3, wg=4)])
SLOW_EMU_SAME_BITS = ('3x3', '3x3_stride2')
_KNOB_FIELD = dict(rows='rows', ring='ns', wg='wg_per_ct', nprod='nprod', ct='ct', wgs='wgs_per_cu')


def same_bits_case(cdll, device, name, log=print):
    """the same operands under every launch form of the group, each on its pinned row (and with the plan fields its hints ask for), with and
    without a peak word: the same S16 words in y and y2, the same peak bits"""
    base, forms = SAME_BITS[name]
    first = None
    for knobs in forms:
        for track in (True, False):
            want = dict(kernel=kernel_name(base['ks'], knobs['nbw'], knobs['spw'], track), **{_KNOB_FIELD[k]: v for k, v in knobs.items() if k in _KNOB_FIELD})
            cfg = dict(base, **knobs, **(dict(_T, lo=base.get('lo', 0.0)) if track else dict(lo=base.get('lo', 0.0), hi=3.0e38)))
            got = lc.conv2ds_case(cdll, device, seed=7, return_words=True, expect=want, tag=f'{name} {knobs}', log=log if track else None, **cfg)
            if first is None:
                first, first_knobs = got, knobs
                continue
            for what, a, b in zip(('y', 'y2'), got[:2], first[:2]):
                assert (a is None) == (b is None)
                if a is not None:
                    assert torch.equal(a, b), f'{name}: {what} of {knobs} (peak word: {track}) differs from {first_knobs} in {int((a != b).sum())} words'
            if track:
                assert got[2] == first[2], f'{name}: peak bits {got[2]:#x} of {knobs}, {first[2]:#x} of {first_knobs}'
    if name == ALONE:
        for b in range(base['B']):
            alone = lc.conv2ds_case(cdll, device, seed=7, return_words=True, only_b=b, tag=f'{name} utterance {b} alone', **dict(base, **forms[0], **_T))
            assert torch.equal(alone[0][0], first[0][b]), f'{name}: utterance {b} launched alone differs from its rows of the batch'


# ---- the plan at production shapes, 256 compute units ------------------------------------------------------------------------------------------
# The conv2ds layers of the shipped default models as their native forwards fill the descriptors (csrc/eres2net.hip, resnet_se.hip, res2net.hip,
# campp_head.hip through s16_conv_desc: no hints), 80 features x 298 frames, with TRACK as the model passes a peak word.  The values are the plan's
# as it is today: the table says what the models run, and a changed planner shows up here as a diff.
_r16 = lambda n: -(-n // 16) * 16
_down = lambda n: (n - 1) // 2 + 1


def _layer(ks, cin16, cout16, H, W, stride=1, stride_w=0, res=False, y2=False, concat=False, epi=0, track=False):
    return dict(ks=ks, cin16=cin16, cout16=cout16, H=H, W=W, stride=stride, stride_w=stride_w, res=res, y2=y2, concat=concat, epi=epi, track=track)


def _aff(out, tag, ch, H, W, track=False):
    chp, inter = _r16(ch), _r16(ch // 4)
    out[f'{tag}.att1'] = _layer(1, 2 * chp, inter, H, W, concat=True, epi=1, track=track)
    out[f'{tag}.att2'] = _layer(1, inter, chp, H, W, epi=2, track=track)


def _eres2net_layers(version, m, base_width, scale, blocks=(3, 4, 6, 3), F_=80, T=298):
    """eres2net.py _Res2Block / ERes2Net / ERes2NetV2 as csrc/eres2net.hip runs them: the first block of every stage and (where it differs: no shortcut
    conv, stride 1) its second"""
    out, H, W, in_c, sizes = {}, F_, T, m, []
    for l in range(4):
        planes, fuse = m << l, l >= 2
        wpad, out_c = _r16(planes * base_width // 64), 2 * (m << l)
        for j in range(min(2, blocks[l])):
            stride = 2 if (j == 0 and l > 0) else 1
            Ho, Wo = (_down(H), _down(W)) if stride == 2 else (H, W)
            t = f'layer{l + 1}.{j}'
            out[f'{t}.conv1'] = _layer(1, _r16(in_c), scale * wpad, H, W, stride=stride)
            if fuse:
                out[f'{t}.convs'] = _layer(3, wpad, wpad, Ho, Wo)
                _aff(out, f'{t}.fuse', planes * base_width // 64, Ho, Wo)
            else:
                out[f'{t}.convs'] = _layer(3, wpad, wpad, Ho, Wo, y2=True)
                out[f'{t}.convs.last'] = _layer(3, wpad, wpad, Ho, Wo)
            out[f'{t}.conv3'] = _layer(1, scale * wpad, _r16(out_c), Ho, Wo, res=True)
            if stride != 1 or in_c != out_c:
                out[f'{t}.shortcut'] = _layer(1, _r16(in_c), _r16(out_c), H, W, stride=stride)
            H, W, in_c = Ho, Wo, out_c
        sizes.append((H, W))
    if version == 1:
        for i in (1, 2, 3):
            out[f'layer{i}_downsample'] = _layer(3, m << i, m << (i + 1), *sizes[i - 1], stride=2)
            _aff(out, ('fuse_mode12', 'fuse_mode123', 'fuse_mode1234')[i - 1], m << (i + 1), *sizes[i])
    else:
        out['layer3_ds'] = _layer(3, m * 8, m * 16, *sizes[2], stride=2)
        _aff(out, 'fuse34', m * 16, *sizes[3])
    return out


def _resnet_se_layers(filters=(32, 64, 128, 256), F_=80, T=298):
    """resnet_se.py SEBottleneck (expansion 2) as csrc/resnet_se.hip runs it: every conv with the model's peak word"""
    out, H, W, in_c = {}, F_, T, filters[0]
    for l, p in enumerate(filters):
        for j in range(2):
            stride = 2 if (j == 0 and l > 0) else 1
            Ho, Wo = (_down(H), _down(W)) if stride == 2 else (H, W)
            t = f'layer{l + 1}.{j}'
            out[f'{t}.conv1'] = _layer(1, _r16(in_c), _r16(p), H, W, track=True)
            out[f'{t}.conv2'] = _layer(3, _r16(p), _r16(p), H, W, stride=stride, track=True)
            out[f'{t}.conv3'] = _layer(1, _r16(p), _r16(2 * p), Ho, Wo, track=True)
            if stride != 1 or in_c != 2 * p:
                out[f'{t}.downsample'] = _layer(1, _r16(in_c), _r16(2 * p), H, W, stride=stride, track=True)
            H, W, in_c = Ho, Wo, 2 * p
    return out


def _res2net_layers(m=32, base_width=32, scale=2, F_=80, T=298):
    """res2net.py Bottle2neck (expansion 4; scale 2: one 3x3 conv per block, the other slice passes to conv3 -- pooled into conv3's input buffer in
    a stage's first block, as the concatenation's second source in the others) behind the 7x7 stride-3 stem and the 3x3 stride-2 max pool"""
    stem = lambda n: (n + 2 - 7) // 3 + 1
    out, H, W, in_c = {}, _down(stem(F_)), _down(stem(T)), m
    for l in range(4):
        planes = m << l
        wpad, out_c = _r16(planes * base_width // 64), 4 * planes
        for j in range(2):
            stride = 2 if (j == 0 and l > 0) else 1
            Ho, Wo = (_down(H), _down(W)) if stride == 2 else (H, W)
            t = f'layer{l + 1}.{j}'
            out[f'{t}.conv1'] = _layer(1, _r16(in_c), scale * wpad, H, W, track=True)
            out[f'{t}.convs'] = _layer(3, wpad, wpad, H, W, stride=stride, track=True)
            out[f'{t}.conv3'] = _layer(1, scale * wpad, _r16(out_c), Ho, Wo, res=True, concat=j > 0, track=True)
            if j == 0:
                out[f'{t}.downsample'] = _layer(1, _r16(in_c), _r16(out_c), H, W, stride=stride, track=True)
            H, W, in_c = Ho, Wo, out_c
    return out


def _campp_head_layers(F_=80, T=298):
    """campplus.py FCM as csrc/campp_head.hip's exact form runs it: 32 channels, the stride on the frequency axis only, every conv with the peak word"""
    out, H = {}, F_
    for i in range(4):
        stride = 2 if i % 2 == 0 else 1
        Ho = (H - 1) // stride + 1
        out[f'block{i}.conv1'] = _layer(3, 32, 32, H, T, stride=stride, stride_w=1, track=True)
        if i % 2 == 0:
            out[f'block{i}.shortcut'] = _layer(1, 32, 32, H, T, stride=stride, stride_w=1, track=True)
        out[f'block{i}.conv2'] = _layer(3, 32, 32, Ho, T, stride_w=1, res=True, track=True)
        H = Ho
    out['conv2'] = _layer(3, 32, 32, H, T, stride=2, stride_w=1, track=True)
    return out


# model -> (its conv2ds layers, the batch sizes bench.py runs it at: the per-GPU batch and the batch-1 latency leg; the 54.9 M ERes2NetV2: its bucketed share)
PRODUCTION_MODELS = {
    'eres2net': (_eres2net_layers(1, 32, 32, 2), (1, 256)),
    'eres2netv2': (_eres2net_layers(2, 32, 26, 2), (1, 256)),
    'eres2netv2_w96s4': (_eres2net_layers(2, 96, 26, 4), (1, 64)),
    'resnet_se': (_resnet_se_layers(), (1, 256)),
    'res2net': (_res2net_layers(), (1, 256)),
    'campp_head': (_campp_head_layers(), (1, 256)),
}


def production_desc(L, B):
    """the layer's descriptor with stand-in pointers (the plan looks at which are null only): nothing is allocated, nothing can be launched"""
    p = 1 << 20
    d = _hip.MvConv2dsDesc()
    d.x, d.ldx, d.w, d.bias, d.oscale, d.y, d.ldy = p, L['cin16'], p, p, 1.0, p, L['cout16']
    if L['concat']:
        d.x2, d.ldx2, d.cin1 = p, L['cin16'], L['cin16'] // 2
    if L['res'] or L['epi'] == 2:
        d.res, d.ldres = p, L['cout16']
    if L['epi'] == 2:
        d.res2, d.ldres2 = p, L['cout16']
    if L['y2']:
        d.add, d.ldadd, d.y2, d.ldy2 = p, L['cout16'], p, L['cout16']
    if L['track']:
        d.peak = p
    d.B, d.H, d.W, d.cin16, d.cout16, d.ks, d.stride, d.stride_w, d.epi = B, L['H'], L['W'], L['cin16'], L['cout16'], L['ks'], L['stride'], L['stride_w'], L['epi']
    d.lo, d.hi = 0.0, 20.0
    return d


def production_plan(cdll, model, name, B, cus=256):
    p = _hip.conv2ds_plan_info(production_desc(PRODUCTION_MODELS[model][0][name], B), cus, cdll)
    return p['kernel'][len('conv2ds_kernel'):], p['ctiles'], p['rows'], p['ns'], p['wgs_per_cu'], p['grid']


def production_keys():
    return [(model, name, B) for model, (layers, batches) in PRODUCTION_MODELS.items() for name in layers for B in batches]


# (kernel row, ctiles, rows, ns, wgs_per_cu, grid) per (model, layer, batch) at 256 compute units: tests/golden/conv2ds_production_plan.json,
# rewritten by `python tests/conv2ds_cases.py plan`
PRODUCTION_PLAN_FILE = __import__('os').path.join(__import__('os').path.dirname(__import__('os').path.abspath(__file__)), 'golden', 'conv2ds_production_plan.json')


def load_production_plan():
    import json
    with open(PRODUCTION_PLAN_FILE) as f:
        return {tuple(k.rsplit('/', 2)[:2]) + (int(k.rsplit('/', 2)[2]),): tuple(v) for k, v in json.load(f).items()}


if __name__ == '__main__':
    import sys
    if sys.argv[1:] == ['plan']:   # rewrite the production table from the emulator build of the library
        import json
        from emu_lib import emu_cdll
        table = {f'{m}/{n}/{B}': production_plan(emu_cdll(), m, n, B) for m, n, B in production_keys()}
        with open(PRODUCTION_PLAN_FILE, 'w') as f:
            f.write('{\n' + ',\n'.join(f'  {json.dumps(k)}: {json.dumps(v)}' for k, v in table.items()) + '\n}\n')
        print(f'{len(table)} plans -> {PRODUCTION_PLAN_FILE}')
    else:
        for name in PINNED:
            if 'nan_at' in PINNED[name]['cfg']:
                continue
            o = operands(name)
            ref, bnd, ref2, bnd2 = reference(o)
            y, y2 = model32(o)
            mx, mean, med = ratios(y, ref, bnd)
            prod = ratios(reference(o, drop='product')[0], ref, bnd)[0]
            cross = ratios(reference(o, drop='cross')[0], ref, bnd)[0]
            print(f'{name:34s} cin * ks^2 {o.cin * o.ks * o.ks:5d}  fp32 model: max ratio {mx:.3f} mean {mean:.3f}  median bound {med:.2e}  '
                  f'dropped product: {prod:8.1f}  without Wlo.Xhi: {cross:6.2f}')
