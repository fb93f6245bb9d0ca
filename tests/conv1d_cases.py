"""Pinned cases, the fp64 reference and the per-element bound of the conv1d layer checks: tests/test_conv1d_kernels.py (CPU: the bound's
self-checks, the plan tests, the cases under the emulator) and tests/test_gpu_conv1d_kernels.py (device).

conv1d_launch picks one of the sixteen rows of csrc/conv1d.hip's kernel table (enum ConvKernel) from the shape, the operands, MvConv1dDesc.tile /
persist_blocks_hint and the chip's compute-unit count.  A case here NAMES the row it has to run and uses only knobs that make the plan independent
of the compute-unit count (tile, persist_blocks_hint, the operand combination); mv_conv1d_plan_info -- the plan conv1d_launch itself makes, nothing
restated here -- is asserted for chips of 8, 64, 256 and 304 compute units, and again for the device at hand before the launch.

Reference and bound: see `bound`.  Nothing here comes from device output; `python tests/conv1d_cases.py` prints, per pinned case, what the fp32
rounding model (the layer checks' reference before this module, output rounded to fp16) and a reference with one product term left out make of the
bound on the CPU."""
import torch
import torch.nn.functional as F

import conftest  # noqa: F401  (puts the package on the path when this module runs as a script)
import layer_checks as lc
from mvector import _hip

PLAN_CUS = (8, 64, 256, 304)    # the emulator's chip, a quarter partition, the MI355X, a larger part
ACT64 = {0: lambda v: v, 1: torch.relu, 2: torch.tanh, 3: torch.sigmoid}
ACT_LIPSCHITZ = {0: 1.0, 1: 1.0, 2: 1.0, 3: 0.25}
U32 = 2.0 ** -24                # unit roundoff of fp32


def half_ulp_fp16(v):
    """half the spacing of fp16 at magnitude v (fp64 tensor, >= 0); the spacing is floored at the subnormal spacing 2^-24"""
    _, e = torch.frexp(v.clamp(min=2.0 ** -30))          # v = m * 2^e, m in [0.5, 1): floor(log2 v) = e - 1
    return 0.5 * torch.ldexp(torch.ones_like(v), e - 11).clamp(min=2.0 ** -24)


def bound(pre64, S, n, pre_act, scale, shift, post_act, gate, y_f32):
    """(ref64, bound), both [B, T_out, cout] fp64, of a conv1d epilogue over `pre64` = conv + bias + row bias evaluated in fp64 on the operands as
    the kernel rounds them (x to fp16; x + x2 in fp32, then fp16; the in-affine fma + ReLU rounded once to fp16; weights to fp16).  Everything
    behind those sites -- pre-activation, affine, post-activation, gate -- is fp64 here; an fp16 output clamps to +-65504.

    The bound, per output element (derived, not measured):
      S = sum_i |x_i| |w_i| + |bias| + |row_bias|   (the same conv on absolute values), n = cin * k products.
      * accumulation: the products of two fp16 values are exact in fp32.  Summing n products, the bias and the row bias in fp32 IN ANY ORDER errs by
        at most (n + 1) u S to first order, u = 2^-24 (every partial sum is bounded by S; Higham, Accuracy and Stability, eq. 4.4).  Taken as
        acc = (n + 2) * 2^-23 * S: doubled, because the rounding of the MFMA's internal adder is not documented as round-to-nearest.
      * the epilogue carries acc through maps with Lipschitz constants ReLU / tanh <= 1, sigmoid <= 1/4, the affine |scale|, the gate (in [0, 1)) <= 1.
      * the epilogue's own fp32 roundings (affine fma, the library's tanhf / expf at a few ulp, the gate product): 4 * 2^-24 * (|ref| + 1).
      e = the sum of the two.  fp32 output: bound = e.  fp16 output: the store rounds a value within e of ref, so
      bound = e + half_ulp_fp16(|ref| + e)."""
    e = (n + 2) * 2.0 * U32 * S
    v = ACT64[pre_act](pre64)
    e = e * ACT_LIPSCHITZ[pre_act]
    if scale is not None:
        v = v * scale.double() + shift.double()
        e = e * scale.double().abs()
    v = ACT64[post_act](v)
    e = e * ACT_LIPSCHITZ[post_act]
    if gate is not None:
        v = v * gate.double()
    if not y_f32:
        v = v.clamp(-65504.0, 65504.0)
    e = e + 4.0 * U32 * (v.abs() + 1.0)
    return v, (e if y_f32 else e + half_ulp_fp16(v.abs() + e))


def reference(o, drop_term=False):
    """(ref64, bound) of the conv1d_case operands `o` (lc.conv1d_operands).  drop_term: the deliberately wrong reference of the self-check -- the
    product of the last input channel at tap 0 is missing from every output sum."""
    x = lc.conv1d_rounded_input(o).double()
    w = o.w.half().double()
    conv = lambda x_, w_, b_: F.conv1d(x_, w_, b_, stride=o.stride, dilation=o.dil).transpose(1, 2)
    bias = None if o.bias is None else o.bias.double()     # (no bias: its term leaves the sum and S)
    pre = conv(x, w, bias)
    S = conv(x.abs(), w.abs(), None if bias is None else bias.abs())
    if drop_term:
        w1 = torch.zeros_like(w)
        w1[:, -1, 0] = w[:, -1, 0]
        pre = pre - conv(x, w1, None)
    if o.row_bias:
        pre = pre + o.rb.double().unsqueeze(1)
        S = S + o.rb.double().abs().unsqueeze(1)
    gate = o.gate[:, torch.arange(o.T_out) // o.gate_seg, :] if o.gate_seg else None
    return bound(pre, S, o.cin * o.k, o.pre_act, o.scale, o.shift, o.post_act, gate, o.y_f32)


def ratios(got, ref64, bnd):
    """(max ratio, mean ratio, median bound) of |got - ref64| / bound"""
    r = (got.double() - ref64).abs() / bnd
    return r.max().item(), r.mean().item(), bnd.median().item()


def assert_ratio(got, ref64, bnd, kernel='', tag='', log=None):
    mx, mean, med = ratios(got, ref64, bnd)
    if log is not None:
        log(f'conv1d bound {tag:34s} {kernel:28s} max ratio {mx:.3f}  mean ratio {mean:.3f}  median bound {med:.2e}')
    assert mx <= 1.0, f'{tag} {kernel}: |got - ref64| / bound reaches {mx:.3f} (mean {mean:.3f}, median bound {med:.2e})'
    return mx


def assert_within_bound(o, got, kernel='', tag='', log=None):
    """lc.conv1d_case's hook: every output element within its bound of the fp64 reference"""
    ref64, bnd = reference(o)
    return assert_ratio(got, ref64, bnd, kernel, tag, log)


def model32(o):
    """the fp32 rounding model alone: the layer checks' fp32 reference, the output stored as the kernel stores it"""
    ref = lc.conv1d_ref32(o)
    return ref if o.y_f32 else ref.clamp(-65504.0, 65504.0).half().float()


# ---- the pinned cases: name -> (conv1d_case keywords, the plan every chip has to make) ---------------------------------------------------

def _pin(cfg, kernel, in_stats_kernel='', tail_kernel='', **plan):
    return dict(cfg=cfg, expect=dict(kernel=kernel, in_stats_kernel=in_stats_kernel, tail_kernel=tail_kernel, **plan))


_C = lc.CONV_CASES
_TAPS = dict(B=2, T=75, cin=72, cout=200, k=3, dil=2)      # 150 rows x 200 channels: 2 x 2 tiles of 128, both ragged; an utterance boundary in row tile 0
_EPI = dict(B=2, T=75, cin=136, cout=136, k=1, dil=1, tile=128)
_HF = dict(B=3, dil=1, stride=2, valid=True, pad_mode='zero', pre_act=0, affine=False)
PINNED = {
    # one-shot 128 x 128: second row tile ragged, reflect taps across the utterance boundary inside tile 0, a partial second K stage, a ragged second channel tile
    'glds128_taps': _pin(dict(_TAPS, tile=128), 'CK_GLDS_128', n_tiles=2, co_tiles=2, grid=4),
    'glds128_row_bias_tanh': _pin(dict(_EPI, row_bias=True, post_act=2), 'CK_GLDS_128'),
    'glds128_gate': _pin(dict(_EPI, gate_seg=10, pre_act=0, affine=False), 'CK_GLDS_128'),
    'glds128_second_out': _pin(dict(_EPI, second_out=True), 'CK_GLDS_128'),
    'glds128_y_f32': _pin(dict(_EPI, y_f32=True), 'CK_GLDS_128'),
    # one-shot 64 x 64 on its four-stage ring: nine K stages (the ring wraps twice), a second channel tile of 8
    'glds64_taps': _pin(dict(B=2, T=35, cin=136, cout=72, k=3, dil=2, tile=64), 'CK_GLDS_64', n_tiles=2, co_tiles=2),
    # ... and 1 to 5 K stages around the ring's depth of 4 with 3 in flight
    **{f'glds64_{s}_k_stages': _pin(dict(B=2, T=35, cin=64 * s, cout=64, k=1, dil=1, tile=64), 'CK_GLDS_64') for s in (1, 2, 3, 4, 5)},
    'glds160_row_bias_tanh': _pin(_C[15], 'CK_GLDS_160'),
    'glds160_taps': _pin(_C[16], 'CK_GLDS_160'),
    # fused input statistics: two tiles per utterance, the second ragged; a partial second K stage
    'glds160_in_stats_f16': _pin(dict(B=2, T=170, cin=72, cout=64, k=1, dil=1, tile=160, in_stats=True), 'CK_GLDS_160_IN_STATS', n_tiles=4),
    'glds160_in_stats_f32': _pin(dict(B=2, T=170, cin=72, cout=64, k=1, dil=1, tile=160, in_stats=True, y_f32=True, pre_act=0, affine=False),
                                 'CK_GLDS_160_IN_STATS', n_tiles=4),
    # the statistics from their own launch: B * 2 tiles * 2 = 4 <= the compute units of every chip planned for
    'in_stats_alone': _pin(dict(B=1, T=170, cin=72, cout=64, k=1, dil=1, in_stats=True), 'CK_GLDS_64', in_stats_kernel='CK_IN_STATS'),
    'glds256_row_bias_tanh': _pin(_C[13], 'CK_GLDS_256'),
    'glds256_gate': _pin(_C[14], 'CK_GLDS_256'),
    'glds256_one_k_stage': _pin(_C[18], 'CK_GLDS_256'),
    'persist_taps_ragged_k': _pin(_C[12], 'CK_PERSIST_TAPS'),       # k = 1 with cin % 64 != 0 is the tap kernel's
    'persist_taps': _pin(_C[22], 'CK_PERSIST_TAPS'),
    'persist_taps_walk': _pin(dict(k=3, dil=2, cin=72, cout=1024, T=130, B=9, tile=256, persist_blocks=8), 'CK_PERSIST_TAPS', n_tiles=5, co_tiles=4, grid=8),
    'persist_1x1_strided': _pin(_C[27], 'CK_PERSIST_1X1'),
    'persist_1x1_sum': _pin(_C[19], 'CK_PERSIST_1X1_SUM'),
    'persist_1x1_sum_sq': _pin(_C[20], 'CK_PERSIST_1X1_SUM_SQ'),
    'persist_1x1_sum_sq_no_bn': _pin(_C[21], 'CK_PERSIST_1X1_SUM_SQ'),
    'ring': _pin(_C[17], 'CK_RING'),
    'ring_clock_probe': _pin(_C[28], 'CK_RING'),
    'ring_walk': _pin(dict(k=1, dil=1, cin=192, cout=1024, T=200, B=6, tile=256, persist_blocks=8), 'CK_RING', n_tiles=5, co_tiles=4, grid=8),
    # the ring walk's last partial round on the small-tile kernels (the emulator's ring_tail_case geometries)
    'ring_tail_quarters': _pin(dict(k=1, dil=1, cin=512, cout=512, T=250, B=5, tile=256, persist_blocks=8), 'CK_RING', tail_kernel='CK_GLDS_128_TAIL',
                               tail_nv=2, tail_split=2, grid=8),
    'ring_tail_sixteenths': _pin(dict(k=1, dil=1, cin=512, cout=256, T=290, B=15, tile=256, persist_blocks=16), 'CK_RING', tail_kernel='CK_GLDS_64',
                                 tail_nv=1, tail_split=4, grid=16),
    # through registers: 2 x 2 tiles, both ragged
    'mfma_f32': _pin(dict(_TAPS, x_f32=True), 'CK_MFMA_F32', n_tiles=2, co_tiles=2),
    'mfma_x2': _pin(dict(_TAPS, with_x2=True), 'CK_MFMA_X2', n_tiles=2, co_tiles=2),
    'mfma_in_affine': _pin(dict(B=2, T=75, cin=72, cout=200, k=1, dil=1, in_affine=True, pre_act=0, affine=True, post_act=1), 'CK_MFMA_IN_AFFINE',
                           n_tiles=2, co_tiles=2),
    # the HF encoder's layers 1 .. 6 (csrc/hfencoder.hip): unpadded stride-2 convs, k = 3 and the even k = 2, bias alone in the epilogue, three
    # utterances so that boundaries fall inside a tile; each on the four tile families hf_forward's descriptor can plan to, at both parities of T_in
    # (k = 3 at even T_in and k = 2 at odd T_in leave every utterance's last input row unread: the utterance's stride is not stride * T_out)
    **{f'hf_k{k}_{fam}_T{T}{"" if bias else "_no_bias"}': _pin(dict(_HF, cin=cin, k=k, T=T, cout=256 if tile == 256 else 72, tile=tile, bias=bias),
                                                              kernel)
       for (cin, k) in ((256, 3), (512, 2))
       for fam, tile, kernel, T0 in (('glds64', 64, 'CK_GLDS_64', 60), ('glds128', 128, 'CK_GLDS_128', 110), ('glds160', 160, 'CK_GLDS_160', 110),
                                     ('persist', 256, 'CK_PERSIST_TAPS', 110))
       for T, bias in ((T0, True), (T0 + 1, k == 3))},
}
# 10 to 20 s each under the emulator: MV_SLOW_EMU=1 (the device tier runs them all)
SLOW_EMU = ('persist_taps_walk', 'ring_walk', 'ring_tail_quarters', 'ring_tail_sixteenths')
# the grouped layer (ecapa_variant_checks.grouped_conv_case): tile = 256 keeps it on the ring kernel whatever the chip
GROUPED = dict(cfg=dict(B=2, T=150, cin=256, cout=512, groups=2, tile=256), kernel='CK_RING_GROUPED')


def seed_of(name):
    return list(PINNED).index(name) + 100


def operands(name):
    return lc.conv1d_operands(seed=seed_of(name), **PINNED[name]['cfg'])


def plans(cdll, name, cus=PLAN_CUS):
    """{cus: mv_conv1d_plan_info} of the case's own descriptor (lc.conv1d_case builds it; nothing is launched)"""
    return lc.conv1d_case(cdll, 'cpu', seed=seed_of(name), plan_cus=cus, **PINNED[name]['cfg'])


def run(cdll, device, name, log=print):
    """plan asserted for the device at hand, launch, conv1d_case's structural assertions, the bound"""
    return lc.conv1d_case(cdll, device, seed=seed_of(name), expect=PINNED[name]['expect'], tag=name, log=log, **PINNED[name]['cfg'])


# ---- one accumulation order (conv1d_plan: "Every tile family accumulates in one order, so a different choice gives the same bits") --------------------
_DENSE = dict(B=3, T=100, cin=192, cout=256)
SAME_BITS = {
    # (the dense 1x1 layer on 256 x 256 tiles is the ring kernel's under either hint: 8 resident workgroups or one per tile)
    'dense_1x1': (dict(_DENSE, k=1, dil=1), [(dict(tile=64), 'CK_GLDS_64'), (dict(tile=128), 'CK_GLDS_128'), (dict(tile=160), 'CK_GLDS_160'),
                                             (dict(tile=256, persist_blocks=8), 'CK_RING'), (dict(tile=256, persist_blocks=4096), 'CK_RING')]),
    'taps_k3_d2': (dict(_DENSE, k=3, dil=2), [(dict(tile=64), 'CK_GLDS_64'), (dict(tile=128), 'CK_GLDS_128'), (dict(tile=160), 'CK_GLDS_160'),
                                              (dict(tile=256), 'CK_PERSIST_TAPS')]),
    'dense_1x1_row_bias': (dict(_DENSE, k=1, dil=1, row_bias=True), [(dict(tile=64), 'CK_GLDS_64'), (dict(tile=128), 'CK_GLDS_128'),
                                                                      (dict(tile=160), 'CK_GLDS_160'), (dict(tile=256), 'CK_GLDS_256')]),
    # the HF encoder's k = 3 stride-2 valid layer: "a row's bits do not depend on B" rests on every family accumulating strided taps in one order
    'hf_valid_k3_s2': (dict(_HF, T=111, cin=256, cout=256, k=3), [(dict(tile=64), 'CK_GLDS_64'), (dict(tile=128), 'CK_GLDS_128'),
                                                                   (dict(tile=160), 'CK_GLDS_160'), (dict(tile=256), 'CK_PERSIST_TAPS')]),
}


def same_bits_case(cdll, device, name, log=print):
    base, forms = SAME_BITS[name]
    first = None
    for knobs, kernel in forms:
        y = lc.conv1d_case(cdll, device, seed=7, return_y=True, expect=dict(kernel=kernel), tag=f'{name} {knobs}', log=log, **base, **knobs)
        if first is None:
            first, first_knobs = y, knobs
        else:
            diff = (y.float() - first.float()).abs()
            assert torch.equal(y, first), f'{name}: {knobs} ({kernel}) differs from {first_knobs} in {int((diff > 0).sum())} elements, by up to {diff.max().item()}'


# ---- the plan at production shapes, 256 compute units ------------------------------------------------------------------------------------------
# Layer descriptors as model.hip / campplus.hip fill them (tile 0 unless the model sets one), 298 frames per utterance (CAM++: 149 behind its
# stride-2 layer).  The values are the plan's as it is today: the table documents where the small / 128 / 160 / 256 / ring kernels and the ring's
# tail take over, and a changed threshold shows up here as a diff.

def _layer(cin, cout, k=1, dil=1, T_in=None, ldx=None, stride=1, pad=None, pad_mode='reflect', pre_act=1, affine=True, post_act=0, in_affine=False,
           in_stats=False, gate=False, bias=True, tile=0, frames=298):
    return dict(cin=cin, cout=cout, k=k, dil=dil, T_in=T_in, ldx=ldx, stride=stride, pad=pad, pad_mode=pad_mode, pre_act=pre_act, affine=affine,
                post_act=post_act, in_affine=in_affine, in_stats=in_stats, gate=gate, bias=bias, tile=tile, frames=frames)


PRODUCTION_LAYERS = {
    # EcapaTdnn-1024 (80 features)
    'ecapa_first_window': _layer(400, 1024, T_in=298 + 4, ldx=80, pad=0, pad_mode='zero'),       # k = 5 over 80 features as a 1x1 conv over overlapping rows
    'ecapa_block_1x1': _layer(1024, 1024),
    'ecapa_res2_step': _layer(128, 128, k=3, dil=2),                                            # (the per-step form; short utterances run res2.hip's chain)
    'ecapa_mfa': _layer(3072, 3072),
    'ecapa_asp_hidden': _layer(3072, 128, in_stats=True, pre_act=0, affine=False, bias=False),
    # CAM++ (growth 32, bottleneck 128), T2 = 149
    'campp_tdnn': _layer(320, 128, k=5, stride=2, pad=2, pad_mode='zero', pre_act=0, post_act=1, T_in=298, frames=149),
    'campp_bottleneck': _layer(128, 128, in_affine=True, pre_act=0, post_act=1, pad_mode='zero', frames=149),       # the five-launch form of a dense layer
    'campp_local': _layer(128, 32, k=3, dil=1, pad_mode='zero', pre_act=0, affine=False, gate=True, frames=149),
    'campp_transit1': _layer(512, 256, pre_act=0, affine=False, pad_mode='zero', frames=149),   # (tile = 256 from 16384 rows on: campplus.hip)
    'campp_transit2': _layer(1024, 512, pre_act=0, affine=False, pad_mode='zero', frames=149),
    # the HF encoder (wav2vec2-base, one second of audio) as hf_forward fills the descriptor: no padding, stride 2, the bias (none without conv_bias) alone
    'hf_conv_k3': _layer(512, 512, k=3, stride=2, pad=0, pad_mode='zero', pre_act=0, affine=False, bias=False, T_in=3199, frames=1599),   # layer 1
    'hf_conv_k2': _layer(512, 512, k=2, stride=2, pad=0, pad_mode='zero', pre_act=0, affine=False, bias=False, T_in=199, frames=99),      # layer 5
}
ECAPA_BATCHES, CAMPP_BATCHES = (1, 8, 48, 256), (1, 256)


def production_desc(name, B):
    """the layer's descriptor with stand-in pointers (the plan looks at their alignment only): nothing is allocated, nothing can be launched"""
    L = PRODUCTION_LAYERS[name]
    T = L['frames']
    p = 1 << 20
    d = _hip.MvConv1dDesc()
    d.x, d.x_dtype, d.ldx = p, _hip.MV_DT_F16, L['ldx'] or L['cin']
    d.w_packed, d.bias = p, (p if L['bias'] else None)
    if L['in_affine']:
        d.in_scale = d.in_shift = p
    if L['affine']:
        d.scale = d.shift = p
    if L['gate']:
        d.gate, d.gate_seg_len = p, 100
    if L['in_stats']:
        d.in_stat_sum = d.in_stat_sq = p
    d.pre_act, d.post_act = L['pre_act'], L['post_act']
    d.y, d.y_dtype, d.ldy = p, _hip.MV_DT_F16, L['cout']
    d.B, d.T_in, d.T_out, d.cin, d.cout, d.k = B, L['T_in'] or T, T, L['cin'], L['cout'], L['k']
    d.dilation, d.stride = L['dil'], L['stride']
    d.pad = L['dil'] * (L['k'] - 1) // 2 if L['pad'] is None else L['pad']
    d.pad_mode = _hip.MV_PAD_REFLECT if L['pad_mode'] == 'reflect' else _hip.MV_PAD_ZERO
    d.tile = L['tile']
    if name.startswith('campp_transit') and (L['cout']) % 256 == 0 and B * T >= 16384:
        d.tile = 256
    return d


def production_plan(cdll, name, B, cus=256):
    p = _hip.conv1d_plan_info(production_desc(name, B), 1, cus, cdll)
    kernels = '+'.join(k for k in (p['in_stats_kernel'], p['kernel'], p['tail_kernel']) if k)
    return kernels, p['n_tiles'] * p['co_tiles'], p['grid'], p['tail_nv']


# (kernels, tiles, workgroups of the main launch, tiles of the ring's tail) at 256 compute units
PRODUCTION_PLAN = {
    ('ecapa_first_window', 1): ('CK_GLDS_64', 80, 80, 0),
    ('ecapa_first_window', 8): ('CK_GLDS_128', 152, 152, 0),
    ('ecapa_first_window', 48): ('CK_PERSIST_TAPS', 224, 224, 0),
    ('ecapa_first_window', 256): ('CK_PERSIST_TAPS', 1192, 256, 0),
    ('ecapa_block_1x1', 1): ('CK_GLDS_64', 80, 80, 0),
    ('ecapa_block_1x1', 8): ('CK_GLDS_128', 152, 152, 0),
    ('ecapa_block_1x1', 48): ('CK_RING', 224, 224, 0),
    ('ecapa_block_1x1', 256): ('CK_RING', 1192, 256, 0),
    ('ecapa_res2_step', 1): ('CK_GLDS_64', 10, 10, 0),
    ('ecapa_res2_step', 8): ('CK_GLDS_64', 76, 76, 0),
    ('ecapa_res2_step', 48): ('CK_GLDS_64', 448, 448, 0),
    ('ecapa_res2_step', 256): ('CK_GLDS_160', 477, 477, 0),
    ('ecapa_mfa', 1): ('CK_GLDS_64', 240, 240, 0),
    ('ecapa_mfa', 8): ('CK_GLDS_128', 456, 456, 0),
    ('ecapa_mfa', 48): ('CK_RING', 672, 256, 0),
    ('ecapa_mfa', 256): ('CK_RING', 3576, 256, 0),
    ('ecapa_asp_hidden', 1): ('CK_IN_STATS+CK_GLDS_64', 10, 10, 0),
    ('ecapa_asp_hidden', 8): ('CK_IN_STATS+CK_GLDS_64', 76, 76, 0),
    ('ecapa_asp_hidden', 48): ('CK_IN_STATS+CK_GLDS_64', 448, 448, 0),
    ('ecapa_asp_hidden', 256): ('CK_GLDS_160_IN_STATS', 512, 512, 0),
    ('campp_tdnn', 1): ('CK_GLDS_64', 6, 6, 0),
    ('campp_tdnn', 256): ('CK_GLDS_128', 298, 298, 0),
    ('campp_bottleneck', 1): ('CK_MFMA_IN_AFFINE', 2, 2, 0),
    ('campp_bottleneck', 256): ('CK_MFMA_IN_AFFINE', 298, 298, 0),
    ('campp_local', 1): ('CK_GLDS_128', 2, 2, 0),
    ('campp_local', 256): ('CK_GLDS_128', 298, 298, 0),
    ('campp_transit1', 1): ('CK_GLDS_64', 12, 12, 0),
    ('campp_transit1', 256): ('CK_RING', 149, 152, 0),
    ('campp_transit2', 1): ('CK_GLDS_64', 24, 24, 0),
    ('campp_transit2', 256): ('CK_RING+CK_GLDS_128_TAIL', 298, 256, 42),
    ('hf_conv_k3', 1): ('CK_GLDS_64', 200, 200, 0),
    ('hf_conv_k3', 8): ('CK_GLDS_128', 400, 400, 0),
    ('hf_conv_k3', 48): ('CK_PERSIST_TAPS', 600, 256, 0),
    ('hf_conv_k3', 256): ('CK_PERSIST_TAPS', 3198, 256, 0),
    ('hf_conv_k2', 1): ('CK_GLDS_64', 16, 16, 0),
    ('hf_conv_k2', 8): ('CK_GLDS_64', 104, 104, 0),
    ('hf_conv_k2', 48): ('CK_GLDS_128', 152, 152, 0),
    ('hf_conv_k2', 256): ('CK_PERSIST_TAPS', 198, 200, 0),
}


if __name__ == '__main__':
    import sys
    if sys.argv[1:] == ['plan']:   # reprint PRODUCTION_PLAN from the emulator build of the library
        from emu_lib import emu_cdll
        for name in PRODUCTION_LAYERS:
            for B in (CAMPP_BATCHES if name.startswith('campp') else ECAPA_BATCHES):
                print(f'    ({name!r}, {B}): {production_plan(emu_cdll(), name, B)!r},')
    else:
        for name in PINNED:
            o = operands(name)
            ref64, bnd = reference(o)
            mx, mean, med = ratios(model32(o), ref64, bnd)
            wrong = ratios(reference(o, drop_term=True)[0], ref64, bnd)[0]
            print(f'{name:28s} cin * k {o.cin * o.k:5d}  fp32 model: max ratio {mx:.3f} mean {mean:.3f}  median bound {med:.2e}  dropped term: max ratio {wrong:.1f}')
