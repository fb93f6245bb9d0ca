"""Layer-level parity checks shared by the emulator tests (CPU tensors, emu library) and the GPU tests (CUDA
tensors, product library).  Every check drives one exported C-ABI entry point with seeded inputs and compares
with a plain torch fp32 reference of the same op (inputs rounded to fp16 exactly as the kernel sees them)."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

from mvector import _hip

ACT = {0: lambda v: v, 1: torch.relu, 2: torch.tanh, 3: torch.sigmoid}


def _stream(t):
    return _hip.current_stream(t)


def pack_weight(cdll, w):
    """w: [Cout, Cin, k] fp32 on device -> packed fp16 buffer (torch.float16 tensor)."""
    cout, cin, k = w.shape
    n = cdll.mv_conv1d_packed_elems(cout, cin, k)
    packed = torch.zeros(n, dtype=torch.float16, device=w.device)
    _hip.check(cdll.mv_conv1d_pack_weight(w.contiguous().data_ptr(), cout, cin, k, packed.data_ptr(), _stream(w)), cdll)
    return packed


def conv1d_operands(B=2, T=37, cin=24, cout=40, k=3, dil=2, stride=1, pad_mode='reflect', valid=False, x_f32=False, y_f32=False, with_x2=False,
                    in_affine=False, pre_act=1, affine=True, post_act=0, row_bias=False, gate_seg=0, extra_ld=8, second_out=False, seed=0, out_gain=1.0,
                    bias=True, **launch_only):
    """The seeded fp32 operands of a conv1d_case on the CPU, by the case's keywords (tile, stats, ... only shape the launch): what conv1d_case
    uploads, and what the CPU self-checks of tests/conv1d_cases.py evaluate without a launch."""
    from types import SimpleNamespace
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    o = SimpleNamespace(B=B, T=T, cin=cin, cout=cout, k=k, dil=dil, stride=stride, pad_mode=pad_mode, x_f32=x_f32, y_f32=y_f32, with_x2=with_x2,
                        in_affine=in_affine, pre_act=pre_act, affine=affine, post_act=post_act, row_bias=row_bias, gate_seg=gate_seg)
    o.ldx = cin + extra_ld
    o.xfull = rn(B, T, o.ldx)
    o.x2full = rn(B, T, o.ldx) if with_x2 else None
    o.w = rn(cout, cin, k) * (2.0 / (cin * k)) ** 0.5
    o.bias = rn(cout) * 0.1 if bias else None   # None: a null bias pointer (the HF encoder's "group" mode without conv_bias)
    o.scale = (torch.rand(cout, generator=g) + 0.5) * out_gain if affine else None   # out_gain: drives the outputs beyond the fp16 range (saturation at +-65504)
    o.shift = rn(cout) * 0.1 if affine else None
    o.in_s = torch.rand(cin, generator=g) + 0.5 if in_affine else None
    o.in_t = rn(cin) * 0.2 if in_affine else None
    o.pad = 0 if valid else dil * (k - 1) // 2
    o.T_out = (T + 2 * o.pad - dil * (k - 1) - 1) // stride + 1
    o.rb = rn(B, cout) * 0.3 if row_bias else None
    o.nseg = -(-o.T_out // gate_seg) if gate_seg else 0
    o.gate = torch.rand(B, o.nseg, cout, generator=g) if gate_seg else None
    o.ldy = cout + extra_ld
    o.addsrc = rn(B, o.T_out, o.ldy).half() if second_out else None
    xdt = torch.float32 if x_f32 else torch.float16
    o.x, o.x2 = o.xfull.to(xdt), (o.x2full.to(xdt) if with_x2 else None)   # as stored on the device
    return o


def conv1d_rounded_input(o):
    """[B, cin, T + 2 pad] fp32 holding the fp16 values the MFMAs consume: x (+ x2 in fp32) (through the in-affine fma + ReLU), rounded once, padded"""
    xin = o.x.float()[..., :o.cin]
    if o.with_x2:
        xin = xin + o.x2.float()[..., :o.cin]
    if o.in_affine:   # one rounding, like the kernel's fma (mul + add in fp32 lands on the other side of an fp16 rounding boundary for ~1 element in 30 000:
        #              a 1e-3 difference behind the conv -- found by the device fuzz of round 5, r14x)
        xin = torch.relu((xin.double() * o.in_s.double() + o.in_t.double()).float())
    xin = xin.half().float().transpose(1, 2)
    if o.pad:
        xin = F.pad(xin, (o.pad, o.pad), mode='reflect' if o.pad_mode == 'reflect' else 'constant')
    return xin


def conv1d_ref32(o):
    """torch fp32 reference [B, T_out, cout] on the values the kernel actually consumes (before the fp16 output's clamp)"""
    ref = F.conv1d(conv1d_rounded_input(o), o.w.half().float(), o.bias, stride=o.stride, dilation=o.dil)
    if o.row_bias:
        ref = ref + o.rb.unsqueeze(2)
    ref = ACT[o.pre_act](ref)
    if o.affine:
        ref = ref * o.scale.view(1, -1, 1) + o.shift.view(1, -1, 1)
    ref = ACT[o.post_act](ref).transpose(1, 2)
    if o.gate_seg:
        seg = torch.arange(o.T_out) // o.gate_seg
        ref = ref * o.gate[:, seg, :]
    return ref


# conv1d_case applies the per-element fp64 bound of tests/conv1d_cases.py up to this cin * k (above it the bound is as loose as the global tolerance)
CONV_BOUND_MAX_K = 1024


def conv1d_case(cdll, device, B=2, T=37, cin=24, cout=40, k=3, dil=2, stride=1, pad_mode='reflect', valid=False,
                x_f32=False, y_f32=False, with_x2=False, in_affine=False, pre_act=1, affine=True, post_act=0,
                row_bias=False, gate_seg=0, extra_ld=8, second_out=False, tile=0, stats=0, in_stats=False, seed=0, persist_blocks=0, clock_probe=False, return_y=False, out_gain=1.0,
                bias=True, expect=None, plan_cus=None, log=None, tag=''):
    """expect: {'kernel': ..., ...} -- fields of mv_conv1d_plan_info the descriptor must plan to on this device, asserted before the launch.
    plan_cus: launch nothing; return {cus: plan info} of the case's descriptor for these compute-unit counts (the weights stay unpacked).
    log: receives the per-element bound's line (tests/conv1d_cases.py) where the bound applies."""
    o = conv1d_operands(B=B, T=T, cin=cin, cout=cout, k=k, dil=dil, stride=stride, pad_mode=pad_mode, valid=valid, x_f32=x_f32, y_f32=y_f32,
                        with_x2=with_x2, in_affine=in_affine, pre_act=pre_act, affine=affine, post_act=post_act, row_bias=row_bias,
                        gate_seg=gate_seg, extra_ld=extra_ld, second_out=second_out, seed=seed, out_gain=out_gain, bias=bias)
    ldx, w, bias, scale, shift, in_s, in_t, pad, T_out, rb, gate = o.ldx, o.w, o.bias, o.scale, o.shift, o.in_s, o.in_t, o.pad, o.T_out, o.rb, o.gate

    xd = o.x.to(device)
    x2d = o.x2.to(device) if with_x2 else None
    ldy = o.ldy
    y = torch.full((B, T_out, ldy), 7.0, dtype=torch.float32 if y_f32 else torch.float16, device=device)
    wd = w.to(device)
    packed = pack_weight(cdll, wd) if plan_cus is None else torch.zeros(cdll.mv_conv1d_packed_elems(cout, cin, k), dtype=torch.float16, device=device)
    dev = lambda t: None if t is None else t.to(device).contiguous()
    biasd, scaled, shiftd, in_sd, in_td, rbd, gated = map(dev, (bias, scale, shift, in_s, in_t, rb, gate))
    d = _hip.MvConv1dDesc()
    d.x, d.x2 = xd.data_ptr(), (x2d.data_ptr() if with_x2 else None)
    d.x_dtype = _hip.MV_DT_F32 if x_f32 else _hip.MV_DT_F16
    d.ldx = d.ldx2 = ldx
    d.in_scale, d.in_shift = (in_sd.data_ptr(), in_td.data_ptr()) if in_affine else (None, None)
    d.w_packed, d.bias = packed.data_ptr(), (None if biasd is None else biasd.data_ptr())
    d.row_bias = rbd.data_ptr() if row_bias else None
    d.pre_act, d.post_act = pre_act, post_act
    d.scale, d.shift = (scaled.data_ptr(), shiftd.data_ptr()) if affine else (None, None)
    d.gate, d.gate_seg_len = (gated.data_ptr(), gate_seg) if gate_seg else (None, 0)
    d.y, d.y_dtype, d.ldy = y.data_ptr(), (_hip.MV_DT_F32 if y_f32 else _hip.MV_DT_F16), ldy
    if second_out:
        addsrc = o.addsrc.to(device)
        sumdst = torch.full((B, T_out, ldy), 5.0, dtype=torch.float16, device=device)
        d.add_src, d.sum_dst, d.ld_add, d.ld_sum = addsrc.data_ptr(), sumdst.data_ptr(), ldy, ldy
    d.B, d.T_in, d.T_out, d.cin, d.cout, d.k = B, T, T_out, cin, cout, k
    d.dilation, d.stride, d.pad = dil, stride, pad
    d.pad_mode = _hip.MV_PAD_REFLECT if pad_mode == 'reflect' else _hip.MV_PAD_ZERO
    d.tile = tile
    d.persist_blocks_hint = persist_blocks
    if stats:  # fused per-utterance time statistics of y (mean; mean + std)
        nstat = cdll.mv_conv1d_stats_elems(B, T_out, cout)
        psum = torch.full((nstat,), float('nan'), device=device)
        psq = torch.full((nstat,), float('nan'), device=device) if stats == 2 else None
        d.stat_sum, d.stat_sq = psum.data_ptr(), (psq.data_ptr() if psq is not None else None)
    if in_stats:  # fused per-utterance time statistics of the INPUT x (ASP global mean / std)
        nin = cdll.mv_conv1d_in_stats_elems(B, T, cin)
        isum = torch.full((nin,), float('nan'), device=device)
        isq = torch.full((nin,), float('nan'), device=device)
        d.in_stat_sum, d.in_stat_sq = isum.data_ptr(), isq.data_ptr()
    if clock_probe:   # MvConv1dDesc.clock_probe (ABI 5): the ring kernel's workgroups leave their entry / exit clocks
        probe = torch.zeros(4 * 264, dtype=torch.int64, device=device)
        d.clock_probe = probe.data_ptr()
    if plan_cus is not None:
        return {cus: _hip.conv1d_plan_info(d, 1, cus, cdll) for cus in plan_cus}
    plan = _hip.conv1d_plan_info(d, 1, 0, cdll)
    for name, want in (expect or {}).items():
        assert plan[name] == want, f'{tag}: the plan has {name} = {plan[name]!r}, the case is pinned to {want!r} ({plan})'
    _hip.check(cdll.mv_conv1d_forward(ctypes.byref(d), _stream(xd)), cdll)
    if device != 'cpu':
        torch.cuda.synchronize()
    if clock_probe:
        t = probe.cpu().reshape(-1, 4)
        t = t[t[:, 3] > t[:, 2]]
        assert t.shape[0] >= 1 and bool((t[:, 1] > t[:, 0]).all()), 'no workgroup left its clocks'
        ghz = ((t[:, 1] - t[:, 0]).double() / (t[:, 3] - t[:, 2]).double() * 0.1).median().item()
        assert 0.3 < ghz < 3.5, ghz   # (the emulator's stand-in counters read 1.0)
    if in_stats:
        imean = torch.empty(B, 2 * cin, device=device)
        _hip.check(cdll.mv_conv1d_in_stats_finish(isum.data_ptr(), isq.data_ptr(), B, T, cin, imean.data_ptr(),
                                                  imean.data_ptr() + 4 * cin, 2 * cin, 1e-12, _stream(xd)), cdll)
        xs = xd.cpu().double()[..., :cin]
        rm = xs.mean(1)
        rs = torch.sqrt(((xs - rm.unsqueeze(1)) ** 2).mean(1).clamp(1e-12))
        got_ms = imean.cpu().double()
        e1 = (got_ms[:, :cin] - rm).abs().max().item()
        e2 = (got_ms[:, cin:] - rs).abs().max().item()
        assert e1 < 2e-6 * max(1.0, rm.abs().max().item()) and e2 < 2e-5 * max(1.0, rs.abs().max().item()), f'input statistics {e1} {e2}'

    # ---- torch fp32 reference on the values the kernel actually consumes ----
    ref = conv1d_ref32(o)
    got = y.cpu().float()
    assert torch.all(got[..., cout:] == 7.0), 'kernel wrote outside its channel slice'
    if not y_f32:   # fp16 outputs saturate instead of overflowing (v_med3 / MODE.FP16_OVFL)
        assert bool(torch.isfinite(got).all()), 'the kernel produced an infinity or a NaN'
        ref = ref.clamp(-65504.0, 65504.0)
        if out_gain > 1.0:
            assert (ref.abs() == 65504.0).float().mean().item() > 0.05, 'the case does not saturate'
    err = (got[..., :cout] - ref).abs().max().item()
    tol = 2e-4 if y_f32 else 4e-3 * max(1.0, ref.abs().max().item())
    assert err < tol, f'conv1d mismatch {err} (tol {tol})'
    if cin * k <= CONV_BOUND_MAX_K:   # the per-element bound against fp64
        import conv1d_cases
        launched = '+'.join(name for name in (plan['in_stats_kernel'], plan['kernel'], plan['tail_kernel']) if name)
        conv1d_cases.assert_within_bound(o, got[..., :cout], kernel=launched, tag=tag, log=log)
    if stats:
        mean = torch.empty(B, cout, device=device)
        std = torch.empty(B, cout, device=device) if stats == 2 else None
        _hip.check(cdll.mv_conv1d_stats_finish(psum.data_ptr(), psq.data_ptr() if psq is not None else None,
                                               shiftd.data_ptr() if affine else None, B, T_out, cout, mean.data_ptr(),
                                               std.data_ptr() if std is not None else None, cout, 1e-12, _stream(xd)), cdll)
        rmean = ref.mean(1)
        e1 = (mean.cpu() - rmean).abs().max().item()
        assert e1 < 2e-3 * max(1.0, rmean.abs().max().item()), f'fused time mean {e1}'
        if stats == 2:
            rstd = torch.sqrt(((ref - rmean.unsqueeze(1)) ** 2).mean(1).clamp(1e-12))
            e2 = (std.cpu() - rstd).abs().max().item()
            assert e2 < 2e-3 * max(1.0, rstd.abs().max().item()), f'fused time std {e2}'
    if second_out:
        want = (y.cpu().float()[..., :cout] + addsrc.cpu().float()[..., :cout]).half().float()
        got2 = sumdst.cpu().float()
        assert torch.all(got2[..., cout:] == 5.0)
        assert (got2[..., :cout] - want).abs().max().item() <= 2e-3 * max(1.0, want.abs().max().item())
    return y.cpu() if return_y else err


def ring_tail_case(cdll, device, blocks=8, profile=True, **cfg):
    """The ring GEMM's tail (conv1d_launch): with `blocks` resident workgroups the walk's last partial round runs as 64 x 64 / 128 x 128 sub-tiles on the
    four-stage forms of the small-tile kernels; with one workgroup per tile (blocks = a multiple of 8 >= the tile count) nothing is split.  Both launches
    pass conv1d_case's check against torch -- and carry THE SAME BITS (a row / channel split keeps every element's accumulation order).  Returns the
    numbers of (ring, all conv1d) launches the split form recorded."""
    import ctypes
    def read(k, reset=0):
        n, ms, w = ctypes.c_int32(0), ctypes.c_double(0.0), ctypes.c_double(0.0)
        _hip.check(cdll.mv_profile_read(k, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(w), reset), cdll)
        return n.value, w.value
    read(0, 1)
    cdll.mv_profile_enable(1)
    try:
        y_split = conv1d_case(cdll, device, persist_blocks=blocks, return_y=True, **cfg)
        (n3, w3), (n0, w0) = read(3), read(0)
    finally:
        cdll.mv_profile_enable(0)
        read(0, 1)
    y_whole = conv1d_case(cdll, device, persist_blocks=4096, return_y=True, **cfg)
    assert torch.equal(y_split, y_whole), (y_split.float() - y_whole.float()).abs().max().item()
    B, T, cin, cout = cfg['B'], cfg['T'], cfg['cin'], cfg['cout']
    assert w0 == 2.0 * B * T * cin * cout, (w0, 2.0 * B * T * cin * cout)   # ring part + quarters = the layer's algorithmic FLOPs
    return n3, n0, w3, w0


def conv1d_window_case(cdll, device, B=3, T=300, F_=80, k=5, cout=512, tile=0, seed=0):
    """The first ECAPA conv as the model runs it: reflect-padded channel-last features [B, T + k - 1, F], 1x1 conv with
    cin = k*F and row stride F (overlapping rows), T_out = T.  Reference: plain k-tap conv with reflect padding."""
    g = torch.Generator().manual_seed(seed)
    pad = (k - 1) // 2
    x = torch.randn(B, T, F_, generator=g)
    w = torch.randn(cout, F_, k, generator=g) * (2.0 / (F_ * k)) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1
    xp = F.pad(x.transpose(1, 2), (pad, pad), mode='reflect').transpose(1, 2).contiguous().half().to(device)
    wr = w.permute(0, 2, 1).reshape(cout, k * F_, 1).contiguous().to(device)     # [co][tap*F + ci]
    packed = pack_weight(cdll, wr)
    biasd = bias.to(device)
    y = torch.full((B, T, cout + 8), 7.0, dtype=torch.float16, device=device)
    d = _hip.MvConv1dDesc()
    d.x, d.x_dtype, d.ldx = xp.data_ptr(), _hip.MV_DT_F16, F_
    d.w_packed, d.bias = packed.data_ptr(), (None if biasd is None else biasd.data_ptr())
    d.pre_act, d.post_act = 1, 0
    d.y, d.y_dtype, d.ldy = y.data_ptr(), _hip.MV_DT_F16, cout + 8
    d.B, d.T_in, d.T_out, d.cin, d.cout, d.k = B, T + 2 * pad, T, k * F_, cout, 1
    d.dilation, d.stride, d.pad, d.pad_mode, d.tile = 1, 1, 0, _hip.MV_PAD_ZERO, tile
    _hip.check(cdll.mv_conv1d_forward(ctypes.byref(d), _stream(xp)), cdll)
    if device != 'cpu':
        torch.cuda.synchronize()
    ref = torch.relu(F.conv1d(xp.cpu().float().transpose(1, 2), w.half().float(), bias)).transpose(1, 2)
    got = y.cpu().float()
    assert torch.all(got[..., cout:] == 7.0)
    err = (got[..., :cout] - ref).abs().max().item()
    assert err < 4e-3 * max(1.0, ref.abs().max().item()), f'window conv mismatch {err}'
    return err


def s16_split(cdll, t, device):
    """fp32 channel-last tensor (last axis a multiple of 16) -> device buffer in the S16 form of conv2ds.hip"""
    td = t.to(device).contiguous().float()
    out = torch.zeros_like(td)
    _hip.check(cdll.mv_map_split_f32(td.data_ptr(), out.data_ptr(), td.numel(), _stream(td)), cdll)
    return out


def s16_merge(cdll, buf):
    out = torch.empty_like(buf)
    _hip.check(cdll.mv_map_merge_f32(buf.data_ptr(), out.data_ptr(), buf.numel(), _stream(buf)), cdll)
    if buf.device.type != 'cpu':
        torch.cuda.synchronize()
    return out.cpu()


CONV2DS_BOUND_MAX_K, CONV2DS_BOUND_MAX_WORK = 1024, 1 << 28


def conv2ds_operands(B=2, H=10, W=37, cin=16, cout=16, ks=3, stride=1, stride_w=0, concat=False, epi=0, with_res=False, with_sum=False,
                     lo=0.0, hi=20.0, seed=0, x_scale=1.0, add_scale=1.0, only_b=None):
    """the random operands of conv2ds_case, on the CPU and before any rounding (tests/conv2ds_cases.py evaluates its fp64 reference on them without a
    kernel).  add_scale: gain of the second output's addend (peak cases: max |y2| above max |y|).  only_b: utterance b of the batch alone."""
    import types
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    r16 = lambda n: -(-n // 16) * 16
    cin_a = cin if not concat else cin // 2            # concat: two operands of cin/2 channels each
    lda = r16(cin_a) + 16
    xa = rn(B, H, W, lda) * x_scale
    xb = rn(B, H, W, lda) * x_scale if concat else None
    w = rn(cout, cin, ks, ks) * (2.0 / (cin * ks * ks)) ** 0.5
    bn_scale = torch.rand(cout, generator=g) + 0.5
    bias = rn(cout) * 0.3
    p = ks // 2
    sw = stride_w or stride
    Ho, Wo = (H + 2 * p - ks) // stride + 1, (W + 2 * p - ks) // sw + 1
    c16 = r16(cout)
    ldy = c16 + 16
    res = rn(B, Ho, Wo, c16) if (with_res or epi == 2) else None
    res2 = rn(B, Ho, Wo, c16) if epi == 2 else None
    add = rn(B, Ho, Wo, c16) * add_scale if with_sum else None
    for t in (res, res2, add):   # operands are maps of the same model: their padded channels are zero (eres2net.hip pads weights with zero rows)
        if t is not None:
            t[..., cout:] = 0.0
    if only_b is not None:
        one = lambda t: None if t is None else t[only_b:only_b + 1].contiguous()
        xa, xb, res, res2, add, B = one(xa), one(xb), one(res), one(res2), one(add), 1
    if concat:   # the weight as the packer gets it: the two sources' channels each padded to 16
        wfull = torch.zeros(cout, 2 * r16(cin_a), ks, ks)
        wfull[:, :cin_a] = w[:, :cin_a]
        wfull[:, r16(cin_a):r16(cin_a) + cin_a] = w[:, cin_a:]
        cin_k = 2 * r16(cin_a)
    else:
        wfull, cin_k = w, cin
    return types.SimpleNamespace(B=B, H=H, W=W, cin=cin, cout=cout, ks=ks, stride=stride, sw=sw, concat=concat, epi=epi, with_res=with_res,
                                 with_sum=with_sum, lo=lo, hi=hi, cin_a=cin_a, lda=lda, xa=xa, xb=xb, w=w, wfull=wfull, cin_k=cin_k, bn_scale=bn_scale,
                                 bias=bias, p=p, Ho=Ho, Wo=Wo, c16=c16, ldy=ldy, res=res, res2=res2, add=add)


def s16_words(buf):
    """(hi, lo) fp64 [..., channels] of an S16 buffer (a float32 tensor whose storage holds, per unit of 16 channels, 16 x hi | 16 x lo fp16 of
    64 * value): the stored words themselves, nothing rounded on the way"""
    h = buf.cpu().contiguous().view(torch.float16).reshape(*buf.shape[:-1], buf.shape[-1] // 16, 2, 16)
    return h[..., 0, :].reshape(buf.shape).double(), h[..., 1, :].reshape(buf.shape).double()


def conv2ds_case(cdll, device, B=2, H=10, W=37, cin=16, cout=16, ks=3, stride=1, stride_w=0, concat=False, epi=0, with_res=False, with_sum=False,
                 lo=0.0, hi=20.0, seed=0, nbw=0, ct=0, rows=0, ring=0, wgs=0, spw=0, nprod=0, x_scale=1.0, peak=False, nan_at=None,
                 wg=0, add_scale=1.0, only_b=None, expect=None, plan_cus=None, log=None, tag='', return_words=False):
    """mv_conv2ds_forward (split-fp16 operands on S16 maps) against F.conv2d in fp64 on the SAME 22-bit inputs: the map round trip
    (split -> merge) is what the layer sees, so the bar is the fp32 one of conv2d_case.
    peak: MvConv2dsDesc.peak -- the reported word must hold the largest |64 * value| the layer wanted to store in either output (before the clamp to
    the fp16 range; values beyond 1023.5 are then stored as +-1023.5: the reference values are clamped the same way).  nan_at: input element (b, h, w, c)
    set to NaN -- the outputs that read it must be NaN (a clamp must not turn it into a bound), everything else as without it.
    wg: MvConv2dsDesc.wg_hint.  expect: fields of mv_conv2ds_plan_info the descriptor must plan to on this device, asserted before the launch.
    plan_cus: launch nothing; return {cus: plan info} of the case's descriptor for these compute-unit counts.  log: receives the per-element
    bound's line (tests/conv2ds_cases.py).  return_words: (y, y2 | None, peak bits | None), the raw S16 words of the outputs' channel slices."""
    o = conv2ds_operands(B=B, H=H, W=W, cin=cin, cout=cout, ks=ks, stride=stride, stride_w=stride_w, concat=concat, epi=epi, with_res=with_res,
                         with_sum=with_sum, lo=lo, hi=hi, seed=seed, x_scale=x_scale, add_scale=add_scale, only_b=only_b)
    r16 = lambda n: -(-n // 16) * 16
    B, cin_a, lda, xa, xb, w, bn_scale, bias = o.B, o.cin_a, o.lda, o.xa, o.xb, o.w, o.bn_scale, o.bias
    p, sw, Ho, Wo, c16, ldy, res, res2, add = o.p, o.sw, o.Ho, o.Wo, o.c16, o.ldy, o.res, o.res2, o.add
    dev = lambda t: None if t is None else t.to(device).contiguous()
    sp = lambda t: None if t is None else s16_split(cdll, t, device)
    xad, xbd, resd, res2d, addd = sp(xa), sp(xb), sp(res), sp(res2), sp(add)
    # what the layer reads: the 22-bit values
    mg = lambda t: None if t is None else s16_merge(cdll, t).double()
    xa_q, xb_q, res_q, res2_q, add_q = mg(xad), mg(xbd), mg(resd), mg(res2d), mg(addd)
    assert (xa_q - xa.double()).abs().max().item() <= 3e-7 * max(1.0, xa.abs().max().item()), 'S16 round trip is not 22-bit'
    wd, sd, cin_k = dev(o.wfull), dev(bn_scale), o.cin_k
    n = cdll.mv_conv2ds_packed_elems(cout, cin_k, ks)
    packed = torch.zeros(n, dtype=torch.float32, device=device)
    osc = ctypes.c_float(0.0)
    _hip.check(cdll.mv_conv2ds_pack_weight(wd.data_ptr(), sd.data_ptr(), cout, cin_k, ks, packed.data_ptr(), ctypes.byref(osc), _stream(wd)), cdll)
    biasd = torch.zeros(c16, device=device)
    biasd[:cout] = dev(bias)
    if nan_at is not None:   # (after the split: a NaN's "lo" part is a NaN as well)
        xa_nan = xa.clone()
        xa_nan[nan_at] = float('nan')
        xad = s16_split(cdll, xa_nan, device)
    peak_word = torch.zeros(1, dtype=torch.int32, device=device) if peak else None
    fill = s16_split(cdll, torch.full((B, Ho, Wo, ldy), 7.0), device)
    y = fill.clone()
    y2 = fill.clone() if with_sum else None
    d = _hip.MvConv2dsDesc()
    d.x, d.ldx = xad.data_ptr(), lda
    d.x2, d.ldx2, d.cin1 = (xbd.data_ptr() if concat else None), lda, (r16(cin_a) if concat else 0)
    d.w, d.bias, d.oscale = packed.data_ptr(), biasd.data_ptr(), osc.value
    d.res, d.ldres = (resd.data_ptr() if res is not None else None), c16
    d.res2, d.ldres2 = (res2d.data_ptr() if res2 is not None else None), c16
    d.add, d.ldadd = (addd.data_ptr() if add is not None else None), c16
    d.y, d.ldy = y.data_ptr(), ldy
    d.y2, d.ldy2 = (y2.data_ptr() if with_sum else None), ldy
    d.B, d.H, d.W, d.cin16, d.cout16, d.ks, d.stride, d.epi = B, H, W, r16(cin_k), c16, ks, stride, epi
    d.lo, d.hi = lo, hi
    d.stride_w = stride_w
    d.peak = peak_word.data_ptr() if peak else None
    d.nbw_hint, d.ct_hint, d.rows_hint, d.ring_hint, d.wgs_hint, d.spw_hint, d.nprod_hint, d.wg_hint = nbw, ct, rows, ring, wgs, spw, nprod, wg
    if plan_cus is not None:
        return {cus: _hip.conv2ds_plan_info(d, cus, cdll) for cus in plan_cus}
    plan = _hip.conv2ds_plan_info(d, 0, cdll)
    for name, want in (expect or {}).items():
        assert plan[name] == want, f'{tag}: the plan has {name} = {plan[name]!r}, the case is pinned to {want!r} ({plan})'
    _hip.check(cdll.mv_conv2ds_forward(ctypes.byref(d), _stream(xad)), cdll)
    if device != 'cpu':
        torch.cuda.synchronize()

    xin = xa_q[..., :cin_a]
    if concat:
        xin = torch.cat([xin, xb_q[..., :cin_a]], dim=-1)
    weff = (w * bn_scale.view(-1, 1, 1, 1)).double()
    ref = F.conv2d(xin.permute(0, 3, 1, 2), weff, bias.double(), stride=(stride, sw), padding=p).permute(0, 2, 3, 1)
    if epi == 0:
        if with_res:
            ref = ref + res_q[..., :cout]
        ref = ref.clamp(lo, hi)
    elif epi == 1:
        ref = F.silu(ref)
    else:
        t = torch.tanh(ref)
        ref = res_q[..., :cout] * (1 + t) + res2_q[..., :cout] * (1 - t)
    got = s16_merge(cdll, y).double()
    if peak:
        import struct
        want = ref.abs().max().item() * 64.0            # (before the range clamp; after lo / hi)
        if with_sum:   # the second output is a stored map too: y (as stored, within the range) + add
            want = max(want, (ref.clamp(-65504.0 / 64.0, 65504.0 / 64.0) + add_q[..., :cout]).abs().max().item() * 64.0)
        seen = struct.unpack('f', struct.pack('i', int(peak_word.cpu().item())))[0]
        assert abs(seen - want) <= 2e-5 * want, (seen, want)
        ref = ref.clamp(-65504.0 / 64.0, 65504.0 / 64.0)  # the split saturates at +-1023.5
    if nan_at is not None:
        hit = torch.zeros(B, 1, H, W, dtype=torch.float64)
        hit[nan_at[0], 0, nan_at[1], nan_at[2]] = 1.0
        hit = F.conv2d(hit, torch.ones(1, 1, ks, ks, dtype=torch.float64), stride=(stride, sw), padding=p)[:, 0] > 0   # outputs whose window holds the NaN
        assert torch.isnan(got[..., :cout][hit]).all(), 'a NaN input must reach every output that reads it'
        assert not torch.isnan(got[..., :cout][~hit]).any()
        got = torch.where(hit.unsqueeze(-1).expand_as(got[..., :cout]), ref, got[..., :cout]) if c16 == cout else got
        if c16 != cout:
            got[..., :cout] = torch.where(hit.unsqueeze(-1).expand_as(ref), ref, got[..., :cout])
    assert torch.all(got[..., c16:] == 7.0), 'kernel wrote outside its channel slice'
    if c16 > cout and epi != 2:
        assert torch.all(got[..., cout:c16] == (0.0 if epi != 0 else min(max(0.0, lo), hi))), 'padded channels must stay zero'
    scale = max(1.0, ref.abs().max().item())
    err = (got[..., :cout] - ref).abs().max().item()
    tol = 2e-5 * scale
    assert err < tol, f'conv2ds mismatch {err} (tol {tol})'
    if with_sum:
        got2 = s16_merge(cdll, y2).double()
        err2 = (got2[..., :cout] - (got[..., :cout] + add_q[..., :cout])).abs().max().item()
        assert err2 < 1e-6 * scale, f'conv2ds second output mismatch {err2}'
        assert torch.all(got2[..., c16:] == 7.0)
    # every output element within its derived bound of the fp64 reference on the operands as the kernel holds them: the pinned cases, and every
    # other case up to CONV2DS_BOUND_MAX_K products per output and CONV2DS_BOUND_MAX_WORK products in all (above, the bound is as loose as the
    # tolerance above, and its three fp64 convolutions on the CPU take longer than the layer's test should)
    small = cin * ks * ks <= CONV2DS_BOUND_MAX_K and B * Ho * Wo * cout * cin * ks * ks <= CONV2DS_BOUND_MAX_WORK
    if nan_at is None and (expect is not None or small):
        import conv2ds_cases
        conv2ds_cases.assert_within_bound(o, y, y2, kernel=plan['kernel'], tag=tag, log=log, device_x=(xad, xbd, resd, res2d, addd), device_w=(packed, osc.value))
    if return_words:
        words = lambda t: None if t is None else t.cpu().contiguous().view(torch.int32)[..., :c16].clone()
        return words(y), words(y2), (int(peak_word.cpu().item()) if peak else None)
    return err


CONV2DS_CASES = [
    dict(),                                                                  # 3x3 16 -> 16
    dict(cin=13, cout=13, with_sum=True),                                    # ERes2NetV2 width 13 (padded) + the "sp + spx[i]" second output
    dict(cin=32, cout=32, ks=1, stride=2, H=8, W=41),                        # strided 1x1 (conv1 / shortcut of a stage's first block)
    dict(cin=64, cout=128, ks=3, stride=2, H=9, W=150, hi=65504.0, lo=-65504.0),  # layer1_downsample: no BN / activation
    dict(cin=32, cout=64, ks=1, with_res=True, W=300, H=3),                  # conv3 + bn3 + residual + ReLU20, 8 pixel tiles
    dict(cin=128, cout=16, ks=1, concat=True, epi=1),                        # AFF local_att[0:3]: cat -> 1x1 -> BN -> SiLU
    dict(cin=96, cout=16, ks=1, concat=True, epi=1),                         # concat of two 48-channel operands: a K chunk straddles the sources
    dict(cin=16, cout=64, ks=1, epi=2),                                      # AFF local_att[3:5] + fusion
    dict(cin=104, cout=104, ks=3, H=5, W=40, B=1),                           # width 104: an odd number of 16-channel units, 7 blocks
    dict(cin=256, cout=512, ks=3, stride=2, H=6, W=20, B=1, hi=65504.0, lo=-65504.0),  # layer3_downsample: 32 blocks as three channel tiles of 11 (11, 11, 10), three blocks per wave
    dict(cin=48, cout=144, ks=3, H=3, W=20, B=1),                            # 9 blocks: one channel tile on three consumer waves of three blocks
    dict(cin=48, cout=208, ks=1, H=2, W=37, B=2, with_res=True),             # 1x1: 13 blocks as two channel tiles (7 + 6); three input units: the second K chunk is half empty
    dict(cin=32, cout=48, ks=1, stride=2, H=5, W=37, B=2),                   # strided 1x1 on odd sizes: 5 x 37 -> 3 x 19
    dict(cin=16, cout=32, ks=3, stride=2, H=5, W=33, B=1),                   # strided 3x3 on odd sizes
    dict(cin=48, cout=48, ks=3, H=21, W=50, B=1, with_sum=True),             # 21 rows: tiles of 8 rows on the emulator's 8 compute units, of 3 rows on 256 (cs_rows follows the chip)
    dict(cin=80, cout=80, ks=3, H=10, W=20, B=1, nbw=2),                     # forced two blocks per wave on 5 blocks
    dict(cin=64, cout=256, ks=1, H=4, W=40, B=1, nbw=2, ct=6),               # two blocks per wave, three channel tiles (the last with 4 blocks)
    dict(cin=64, cout=192, ks=3, H=9, W=17, B=1, nbw=2, rows=3),             # two blocks per wave on 12 blocks, tiles of 3 rows
    dict(cin=64, cout=64, ks=3, H=24, W=40, B=2, ring=2, wgs=1),             # shortest ring; 9 tiles per workgroup on the emulator's chip, one on 256 compute units (tests/conv2ds_cases.py walks on both)
    dict(cin=96, cout=48, ks=1, H=30, W=40, B=2, ring=2, wgs=1),             # 1x1, a ring of two
    dict(cin=160, cout=48, ks=1, H=30, W=40, B=2, ring=3, wgs=1),            # 1x1, ring of three
    dict(cin=64, cout=160, ks=3, H=10, W=20, B=1),                           # 10 blocks on four waves of <= 3 (3, 3, 2, 2), four producer waves
    dict(cin=96, cout=192, ks=1, H=6, W=50, B=1, with_res=True),             # residual + short K: two blocks on six consumer waves, two producers
    dict(cin=320, cout=192, ks=1, H=6, W=50, B=1, with_res=True),            # the same layer with four K stages per tile: still two blocks on six consumer waves (the limit of that form)
    dict(cin=48, cout=48, ks=3, H=13, W=40, B=1, nbw=3, spw=4, with_sum=True),   # all three blocks in one wave, two pixel groups
    dict(cin=80, cout=80, ks=3, H=10, W=20, B=1, nbw=3, spw=4),              # five blocks as 3 + 2 on two pixel groups: four consumer waves
    dict(cin=32, cout=32, ks=3, H=11, W=30, B=2, nbw=2, spw=2),              # two blocks per wave, four pixel groups of two segments
    dict(cin=64, cout=64, ks=1, H=7, W=50, B=1, nbw=2, spw=4, with_res=True),  # 1x1: 2 x 2 blocks on two pixel groups
    dict(cin=64, cout=32, ks=1, H=9, W=70, B=2),                             # 1x1 with two blocks and no operands: both blocks in each of four waves of two segments (the default)
    dict(cin=80, cout=80, ks=3, H=12, W=30, B=1),                            # five blocks: the default is 2 + 2 + 1 on three consumer waves
    dict(cin=48, cout=48, ks=3, H=13, W=40, B=1, spw=8),                     # three blocks, the waves do not split the pixels
    dict(cin=32, cout=16, ks=1, H=9, W=50, B=1, spw=2, with_res=True),       # one block, four pixel groups
    dict(cin=32, cout=32, ks=3, H=11, W=30, B=1, spw=2, with_sum=True),      # two blocks, four pixel groups of two segments
    dict(cin=16, cout=16, ks=3, H=11, W=30, B=2, spw=1),                     # one block, eight waves of one segment
    dict(cin=32, cout=32, ks=3, stride=2, stride_w=1, H=9, W=45, B=2, hi=65504.0),   # CAM++ head (exact form): stride on the frequency axis only
    dict(cin=32, cout=32, ks=1, stride=2, stride_w=1, H=8, W=37, B=2, hi=65504.0, lo=-65504.0),  # its 1x1 shortcut conv
    dict(cin=32, cout=32, ks=3, stride=2, stride_w=1, H=80, W=150, B=1, with_res=False, hi=65504.0),  # the head's first block at full height
    dict(cin=32, cout=32, ks=3, H=6, W=18, B=1, x_scale=60.0, hi=65504.0, lo=-65504.0),    # large activations (|x| up to ~270, outputs up to ~600; the split saturates at 1023.5)
]


def tstp_case(cdll, device, B=3, H=5, W=38, C=72, seed=0, s16=False):
    g = torch.Generator().manual_seed(seed)
    ld = C + 8
    x = torch.randn(B, H, W, ld, generator=g) * 2 + 1
    x[0, 0, :, 3] = 1.5   # constant channel: std = sqrt(1e-8)
    xd = x.to(device)
    out = torch.full((B, 2 * C * H), float('nan'), device=device)
    if s16:   # the map in the split form of conv2ds.hip (1.5 * 64 is exact there too)
        xs = s16_split(cdll, x, device)
        x = s16_merge(cdll, xs)
        _hip.check(cdll.mv_tstp_s16(xs.data_ptr(), ld, B, H, W, C, out.data_ptr(), _stream(xd)), cdll)
    else:
        _hip.check(cdll.mv_tstp_f32(xd.data_ptr(), ld, B, H, W, C, out.data_ptr(), _stream(xd)), cdll)
    if device != 'cpu':
        torch.cuda.synchronize()
    xr = x.float()[..., :C].permute(0, 3, 1, 2)            # [B, C, H, W] as the reference holds it
    ref = torch.cat([xr.mean(-1).flatten(1), torch.sqrt(xr.var(-1) + 1e-8).flatten(1)], 1)
    err = (out.cpu() - ref).abs().max().item()
    assert err < 2e-5 * max(1.0, ref.abs().max().item()), f'tstp mismatch {err}'
    return err


def conv2d_first_case(cdll, device, B=2, T=50, F_=16, C=32, seed=0, s16=False):
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(B, T, F_, generator=g)
    w = torch.randn(C, 9, generator=g) * 0.3
    bias = torch.randn(C, generator=g) * 0.1
    fd, wd, bd = feats.to(device), w.to(device), bias.to(device)
    out = torch.empty(B, F_, T, C, dtype=torch.float32, device=device)
    if s16:
        _hip.check(cdll.mv_conv2d_first_s16(fd.data_ptr(), out.data_ptr(), wd.data_ptr(), bd.data_ptr(), B, T, F_, C, _stream(fd)), cdll)
        out = s16_merge(cdll, out)
    else:
        _hip.check(cdll.mv_conv2d_first(fd.data_ptr(), out.data_ptr(), wd.data_ptr(), bd.data_ptr(), B, T, F_, C, _stream(fd)), cdll)
    if device != 'cpu':
        torch.cuda.synchronize()
    ref = torch.relu(F.conv2d(feats.permute(0, 2, 1).unsqueeze(1), w.view(C, 1, 3, 3), bias, padding=1)).permute(0, 2, 3, 1)
    err = (out.cpu().float() - ref).abs().max().item()
    assert err < 1e-5 * max(1.0, ref.abs().max().item()), f'conv2d_first mismatch {err}'
    return err


def profile_classes_case(cdll, device):
    """mv_profile_read classes (include/mvector_hip.h): a ring-kernel launch is recorded as MV_PROF_CONV1D_RING (3) AND counted by a read of
    MV_PROF_CONV1D (0); any other conv1d launch is class 0 only.  bench.py's `roofline` (the ring kernel alone) and `roofline_conv1d_class` rest on it."""
    import ctypes
    def read(k, reset=0):
        n, ms, w = ctypes.c_int32(0), ctypes.c_double(0.0), ctypes.c_double(0.0)
        _hip.check(cdll.mv_profile_read(k, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(w), reset), cdll)
        return n.value, ms.value, w.value
    read(0, 1)
    cdll.mv_profile_enable(1)
    try:
        ring = dict(k=1, dil=1, cin=128, cout=256, T=150, B=2, tile=256)                       # dense 1x1 rows, no statistics: the ring kernel
        taps = dict(k=3, dil=2, cin=64, cout=256, T=130, B=2, tile=256, pre_act=0, affine=False)   # persistent, taps: the double-buffer kernel
        conv1d_case(cdll, device, seed=1, **ring)
        assert read(3)[0] == 1 and read(0)[0] == 1
        conv1d_case(cdll, device, seed=2, **taps)
        conv1d_case(cdll, device, seed=3)                                                      # small non-persistent layer
        n3, ms3, w3 = read(3)
        n0, ms0, w0 = read(0)
        assert (n3, n0) == (1, 3), (n3, n0)
        assert w3 == 2.0 * 2 * 150 * 128 * 256 and w0 > w3 and ms0 >= ms3 >= 0.0
        assert read(1)[0] == 0 and read(2)[0] == 0
    finally:
        cdll.mv_profile_enable(0)
        read(0, 1)
    assert read(3)[0] == 0


CONV_CASES = [
    dict(),                                                           # reflect k3 d2
    dict(k=5, dil=1, cin=80, cout=64, x_f32=True, T=50),              # first layer: fp32 features in
    dict(k=1, dil=1, cin=136, cout=200, T=70, B=3),                   # 1x1, several K stages, 2 co tiles
    dict(k=3, dil=4, with_x2=True, cin=16, cout=16),                  # Res2Net step
    dict(k=3, dil=3, valid=True, pad_mode='zero', T=40),              # TDNN unpadded conv
    dict(k=5, dil=1, stride=2, pad_mode='zero', cin=320, cout=128, T=61),  # CAM++ strided TDNN
    dict(k=1, dil=1, in_affine=True, pre_act=0, affine=True, post_act=1, cin=160, cout=128),  # CAM++ dense bottleneck
    dict(k=3, dil=2, pad_mode='zero', pre_act=0, affine=False, gate_seg=10, cin=128, cout=32, T=45),  # CAM layer
    dict(k=1, dil=1, row_bias=True, post_act=2, cin=192, cout=128, T=33),  # ASP attention hidden layer
    dict(k=1, dil=1, y_f32=True, pre_act=0, affine=False, cin=64, cout=20, T=9, B=5),  # fp32 out, ragged cout
    dict(k=3, dil=1, B=1, T=300, cin=8, cout=8, extra_ld=56),         # many n tiles, narrow slice of a wide row
    dict(k=3, dil=2, cin=16, cout=16, second_out=True, T=41),          # Res2Net step emitting the next step's input
    dict(k=1, dil=1, cin=72, cout=256, T=300, B=1, tile=256),           # 256 x 256 workgroup tile (8 waves)
    dict(k=3, dil=2, cin=64, cout=512, T=70, B=2, tile=256, row_bias=True, post_act=2),  # 256 tile, 2 co tiles, ragged rows
    dict(k=3, dil=3, cin=32, cout=512, T=90, B=3, tile=256, gate_seg=25, pre_act=0, affine=False, pad_mode='zero'),
    dict(k=1, dil=1, cin=136, cout=128, T=170, B=3, tile=160, row_bias=True, post_act=2),  # 128 x 160 tile (ASP hidden layer shape)
    dict(k=3, dil=2, cin=64, cout=200, T=100, B=2, tile=160),            # 160-row tile, taps, ragged channels
    dict(k=1, dil=1, cin=128, cout=768, T=300, B=4, tile=256),           # ring kernel (CK_RING): 15 tiles; eight resident workgroups walk two of them, a full chip has one workgroup per tile
    dict(k=1, dil=1, cin=64, cout=512, T=150, B=7, tile=256),            # a single K stage: below the persistent kernels' two stages, so the one-shot 256 x 256 kernel (CK_GLDS_256), 10 tiles
    dict(k=1, dil=1, cin=128, cout=256, T=90, B=5, tile=256, stats=1),   # fused time mean: utterance boundaries inside 64-row blocks
    dict(k=1, dil=1, cin=192, cout=512, T=298, B=3, tile=256, stats=2),  # fused mean + std (ASP global statistics), ragged last tile
    dict(k=1, dil=1, cin=128, cout=256, T=64, B=4, tile=256, stats=2, affine=False, extra_ld=0),  # boundaries on block edges, no BN
    dict(k=3, dil=2, cin=72, cout=512, T=130, B=5, tile=256, pre_act=0, affine=False),  # persistent, taps, no BatchNorm affine
    # fused INPUT statistics (the ASP hidden layer): per-utterance tiles of 160 frames, fp32 pre-activation out
    dict(k=1, dil=1, cin=192, cout=128, T=45, B=3, in_stats=True, y_f32=True, pre_act=0, affine=False),   # one partial tile per utterance
    dict(k=1, dil=1, cin=320, cout=128, T=298, B=3, in_stats=True, y_f32=True, pre_act=0, affine=False),  # two tiles, ragged second one
    dict(k=1, dil=1, cin=72, cout=64, T=160, B=2, in_stats=True, extra_ld=0),                            # exact tile, partial K stage, fp16 out with epilogue
    dict(k=1, dil=1, cin=128, cout=128, T=1, B=5, in_stats=True, y_f32=True, pre_act=0, affine=False),    # single frame: std = sqrt(eps)
    dict(k=1, dil=1, stride=2, pad_mode='zero', cin=128, cout=256, T=151, B=4, tile=256),   # persistent, 1x1 with a time stride: the double-buffer kernel's plain form (the ring kernel takes dense rows only)
    dict(k=1, dil=1, cin=192, cout=256, T=200, B=6, tile=256, clock_probe=True),   # ring kernel with MvConv1dDesc.clock_probe, three K stages (first / middle / last form of the carried MFMA group)
]


def in_stats_forms_case(cdll, device, B_big, T=298, cin=320, cout=128, seed=0):
    """The ASP hidden layer's conv with fused INPUT statistics in its two launch forms: a batch that fills the chip takes the fused kernel
    (per-utterance 160-frame tiles, statistics beside the MFMAs), one utterance alone takes the stand-alone statistics kernel + the conv on
    64 x 64 tiles.  Row 0 must come out with the SAME bits either way: pre-activations and the partial rows of the statistics."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B_big, T, cin, generator=g).half().to(device)
    w = (torch.randn(cout, cin, 1, generator=g) * (2.0 / cin) ** 0.5).to(device)
    packed = pack_weight(cdll, w)

    def run(xb):
        B = xb.shape[0]
        y = torch.full((B, T, cout), 7.0, dtype=torch.float16, device=device)
        nin = cdll.mv_conv1d_in_stats_elems(B, T, cin)
        isum = torch.full((nin,), float('nan'), device=device)
        isq = torch.full((nin,), float('nan'), device=device)
        d = _hip.MvConv1dDesc()
        d.x, d.x_dtype, d.ldx = xb.data_ptr(), _hip.MV_DT_F16, cin
        d.w_packed = packed.data_ptr()
        d.y, d.y_dtype, d.ldy = y.data_ptr(), _hip.MV_DT_F16, cout
        d.B, d.T_in, d.T_out, d.cin, d.cout, d.k = B, T, T, cin, cout, 1
        d.dilation, d.stride, d.pad, d.pad_mode = 1, 1, 0, _hip.MV_PAD_REFLECT
        d.in_stat_sum, d.in_stat_sq = isum.data_ptr(), isq.data_ptr()
        _hip.check(cdll.mv_conv1d_forward(ctypes.byref(d), _stream(xb)), cdll)
        if device != 'cpu':
            torch.cuda.synchronize()
        return y.cpu(), isum.cpu().view(B, -1), isq.cpu().view(B, -1)
    yb, sb, qb = run(x)
    y1, s1, q1 = run(x[:1].contiguous())
    assert torch.isfinite(yb.float()).all() and torch.isfinite(sb).all()
    assert torch.equal(y1[0], yb[0]), (y1[0].float() - yb[0].float()).abs().max().item()
    assert torch.equal(s1[0], sb[0]) and torch.equal(q1[0], qb[0])


def linear_case(cdll, device, B=5, K=100, O=37, act=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, K, generator=g)
    w = torch.randn(O, K, generator=g) / K ** 0.5
    b = torch.randn(O, generator=g)
    xd, wd, bd = x.to(device), w.to(device), b.to(device)
    y = torch.empty(B, O, device=device)
    _hip.check(cdll.mv_linear_f32(xd.data_ptr(), K, wd.data_ptr(), bd.data_ptr(), act, y.data_ptr(), O, B, K, O, _stream(xd)), cdll)
    ref = ACT[act](x.double() @ w.double().t() + b.double()).float()
    err = (y.cpu() - ref).abs().max().item()
    assert err < 1e-5 * max(1.0, ref.abs().max().item()) + 1e-5, err
    # the workspace form (long reductions over many rows: K slices + slice-ordered sum): same bar, rows independent of the batch they sit in
    need = int(cdll.mv_linear_f32_workspace_floats(B, K, O))
    if need:
        ws = torch.full((need + 7,), float('nan'), device=device)
        y2 = torch.full((B, O + 3), 5.0, device=device)
        _hip.check(cdll.mv_linear_f32_ws(xd.data_ptr(), K, wd.data_ptr(), bd.data_ptr(), act, y2.data_ptr(), O + 3, B, K, O, ws.data_ptr(), need, _stream(xd)), cdll)
        err2 = (y2.cpu()[:, :O] - ref).abs().max().item()
        assert err2 < 1e-5 * max(1.0, ref.abs().max().item()) + 1e-5, err2
        assert torch.all(y2[:, O:] == 5.0) and torch.isnan(ws[need:]).all(), 'wrote outside its output / workspace'
        nb = max(1, B // 3)
        y3 = torch.empty(nb, O, device=device)
        _hip.check(cdll.mv_linear_f32_ws(xd.data_ptr(), K, wd.data_ptr(), bd.data_ptr(), act, y3.data_ptr(), O, nb, K, O, ws.data_ptr(), need, _stream(xd)), cdll)
        assert torch.equal(y3.cpu(), y2.cpu()[:nb, :O]), 'a row\'s bits depend on the batch'
        err = max(err, err2)
    return err


def cosine_case(cdll, device, a, b, expect):
    s = _hip.cosine(torch.from_numpy(a).to(device), torch.from_numpy(b).to(device), cdll=cdll).cpu().numpy()
    err = np.abs(s - expect).max()
    assert err < 2e-6, err
    return err


def time_stats_case(cdll, device, B=3, T=29, C=520, ld=528, unbiased=0, eps=1e-12, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, T, ld, generator=g) * 2 + 0.5).half()
    x[:, :, 3] = 1.25  # constant channel: variance must be exactly clamped
    xd = x.to(device)
    mean = torch.empty(B, C, device=device)
    std = torch.empty(B, C, device=device)
    _hip.check(cdll.mv_time_stats_f16(xd.data_ptr(), ld, B, T, C, mean.data_ptr(), std.data_ptr(), unbiased, eps, _stream(xd)), cdll)
    xf = x.float()[..., :C]
    rm = xf.mean(1)
    var = ((xf - rm.unsqueeze(1)) ** 2).sum(1) / (T - 1 if unbiased else T)
    rs = torch.sqrt(var.clamp(eps) if eps > 0 else var)
    e1 = (mean.cpu() - rm).abs().max().item()
    e2 = (std.cpu() - rs).abs().max().item()
    assert e1 < 1e-5 and e2 < 1e-5, (e1, e2)
    return e1, e2


def bn_relu_rows_case(cdll, device, rows=77, C=520, ldx=528, ldy=544, seed=0):
    """the pre-activation pass of the CAM++ transit layers: relu(x * scale + shift) rounded once to fp16 (saturating), pad columns untouched"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, ldx, generator=g) * 3).half()
    x[0, 0], x[0, 1] = 60000.0, -60000.0
    sc = torch.randn(C, generator=g) * 2
    sh = torch.randn(C, generator=g)
    sc[0], sc[1] = 2.0, 2.0  # overflow of the fp16 range: saturates at 65504 / clamps at 0
    xd, scd, shd = x.to(device), sc.to(device), sh.to(device)
    y = torch.full((rows, ldy), -7.0, dtype=torch.half, device=device)
    _hip.check(cdll.mv_bn_relu_rows_f16(xd.data_ptr(), ldx, scd.data_ptr(), shd.data_ptr(), y.data_ptr(), ldy, rows, C, _stream(xd)), cdll)
    # (the kernel's x * scale + shift is one fused multiply-add, torch rounds the product first: the fp32 results differ by an ulp now and then,
    # which moves a value across an fp16 rounding boundary in ~1e-4 of the elements -- one fp16 ulp at most)
    ref64 = torch.clamp(torch.relu(x.double()[:, :C] * sc.double() + sh.double()), max=65504.0)
    out = y.cpu()
    err = (out[:, :C].double() - ref64).abs()
    # half an fp16 ulp of the exact value (subnormals: 2^-25) + one fp32 rounding of the product (the emulator's host build multiplies and adds
    # separately where the device fuses: visible where x * scale and shift cancel)
    tol = ref64.abs() * 2.0 ** -11 * 1.001 + 2.0 ** -25 + (x.double()[:, :C] * sc.double()).abs() * 2.0 ** -23
    assert bool((err <= tol).all()), (err - tol).max()
    assert bool((out[:, C:] == -7.0).all())
    assert out[0, 0] == 65504.0 and out[0, 1] == 0.0


def asp_pool_case(cdll, device, B=3, T=45, C=192, A=128, ldx=None, online=False, centred=True, wscale=0.08, seed=0):
    """softmax over time of W2 . h (+ b2, which cancels), weighted mean / std of x (pooling.py:117-125)."""
    g = torch.Generator().manual_seed(seed)
    ldx = ldx or C
    h = torch.tanh(torch.randn(B, T, A, generator=g)).half()
    w2 = (torch.rand(C, A, generator=g) * 2 - 1) * wscale
    b2 = torch.randn(C, generator=g)
    x = (torch.randn(B, T, ldx, generator=g) * 1.5 + 0.3).half()
    if centred:
        x[:, :, 5] = 0.75  # constant channel: its variance must come out as exactly the clamp (needs the centred moments)
    log2e = 1.4426950408889634
    packed = pack_weight(cdll, (w2 * log2e).reshape(C, A, 1).to(device))
    hd, xd = h.to(device), x.to(device)
    gmean = x.float()[..., :C].mean(1).to(device) if centred else None
    out = torch.empty(B, 2 * C, device=device)
    bound = -1.0 if online else float(w2.abs().sum(1).max()) * log2e * 1.001
    _hip.check(cdll.mv_asp_pool_f16(hd.data_ptr(), packed.data_ptr(), xd.data_ptr(), ldx, gmean.data_ptr() if centred else None, C,
                                    out.data_ptr(), B, T, C, A, bound, _stream(xd)), cdll)
    # reference in fp64 from the fp16-rounded operands the kernel sees
    w2h = (w2 * log2e).half().double() / log2e
    logits = h.double() @ w2h.t() + b2.double()                # [B, T, C]
    wgt = torch.softmax(logits, dim=1)
    xf = x.double()[..., :C]
    mean = (wgt * xf).sum(1)
    std = torch.sqrt(((wgt * (xf - mean.unsqueeze(1)) ** 2).sum(1)).clamp(1e-12))
    ref = torch.cat([mean, std], 1).float()
    err = (out.cpu() - ref).abs().max().item()
    assert err < 2e-5, err
    return err


FCM_CASES = [
    dict(B=2, Fin=12, T=45, sf=1, mode2=0),                # one time tile, NI = 1, plain conv
    dict(B=2, Fin=12, T=45, sf=2, mode2=0),                # strided in frequency (BasicResBlock.conv1 / FCM.conv2)
    dict(B=1, Fin=9, T=70, sf=2, mode2=0, strided_out=True),  # odd Fin, NI = 2, the [B, T, F8, 32] output layout of FCM.conv2
    dict(B=2, Fin=6, T=100, sf=1, mode2=1, sf2=2),         # conv2 + strided 1x1 shortcut tap on the block input
    dict(B=2, Fin=6, T=33, sf=1, mode2=2),                 # conv2 + identity residual
    dict(B=1, Fin=5, T=330, sf=1, mode2=2),                # two time tiles (T > 320), NI = 3
    dict(B=1, Fin=3, T=16, sf=1, mode2=0),                 # fewer rows than the ring
]


def fcm_conv_case(cdll, device, B, Fin, T, sf, mode2, sf2=1, strided_out=False, seed=0, padded_out=False):
    """3x3 conv2d over (frequency, time) with 32 maps + folded BN bias + (1x1 shortcut | identity) + ReLU (campplus.py:221-292)."""
    g = torch.Generator().manual_seed(seed)
    Fout = (Fin - 1) // sf + 1
    x = torch.randn(B, Fin, T, 32, generator=g).half()
    ntaps = 10 if mode2 == 1 else 9
    w = (torch.randn(ntaps, 32, 32, generator=g) * 0.08).half()
    bias = torch.randn(32, generator=g) * 0.1
    F2 = (Fout - 1) * sf2 + 1 + (1 if sf2 == 2 else 0)
    x2 = torch.randn(B, F2, T, 32, generator=g).half() if mode2 else None
    if strided_out:      # y[b, t, fo, co]
        y = torch.full((B, T, Fout, 32), float('nan')).half().to(device)
        sB, sF, sT = T * Fout * 32, 32, Fout * 32
    elif padded_out:     # y[b, fo, t, co (+ 4 pad)]: rows 72 bytes apart -- not 16-byte aligned, the one-row-per-workgroup kernel's 8-byte stores
        y = torch.full((B, Fout, T, 36), float('nan')).half().to(device)
        sB, sF, sT = Fout * T * 36, T * 36, 36
    else:                # y[b, fo, t, co]
        y = torch.full((B, Fout, T, 32), float('nan')).half().to(device)
        sB, sF, sT = Fout * T * 32, T * 32, 32
    xd, wd, bd = x.to(device), w.to(device), bias.to(device)
    x2d = x2.to(device) if mode2 else None
    _hip.check(cdll.mv_fcm_conv3x3_f16(xd.data_ptr(), Fin, sf, x2d.data_ptr() if mode2 else None, F2 if mode2 else 0, sf2, mode2,
                                       wd.data_ptr(), bd.data_ptr(), y.data_ptr(), sB, sF, sT, B, T, Fout, _stream(xd)), cdll)
    # reference in fp64 from the fp16 operands
    xin = x.double().permute(0, 3, 1, 2)                                        # [B, 32, F, T]
    w33 = w[:9].double().reshape(3, 3, 32, 32).permute(2, 3, 0, 1).contiguous()  # [co, ci, df, dt]
    ref = torch.nn.functional.conv2d(xin, w33, bias.double(), stride=(sf, 1), padding=1)
    if mode2 == 1:
        ref = ref + torch.nn.functional.conv2d(x2.double().permute(0, 3, 1, 2), w[9].double().reshape(32, 32, 1, 1), None, stride=(sf2, 1))[:, :, :Fout]
    elif mode2 == 2:
        ref = ref + x2.double().permute(0, 3, 1, 2)[:, :, ::sf2][:, :, :Fout]
    ref = ref.clamp(min=0).permute(0, 3, 2, 1) if strided_out else ref.clamp(min=0).permute(0, 2, 3, 1)
    out = y.cpu().double()
    if padded_out:
        assert torch.isnan(out[..., 32:]).all(), 'wrote into the padding'
        out = out[..., :32]
    assert torch.isfinite(out).all(), 'unwritten outputs'
    err = (out - ref).abs().max().item()
    assert err < 2e-3 * max(1.0, ref.abs().max().item()), err   # the fp16 rounding of the stored result
    return err


FCM_BLOCK_CASES = [
    dict(B=2, Fin=12, T=45, sf=2),                         # strided block with the 1x1 shortcut tap, NT = 1 (B * tiles < CUs: bands)
    dict(B=2, Fin=6, T=33, sf=1),                          # identity block
    dict(B=1, Fin=9, T=70, sf=2),                          # odd Fin, NT = 2
    dict(B=1, Fin=5, T=330, sf=1),                         # two time tiles (T > 318): halo columns across the tile edge
    dict(B=1, Fin=3, T=16, sf=1),                          # fewer rows than the ring
    dict(B=9, Fin=4, T=62, sf=2, strided_out=True),        # one band per workgroup, T = tile width, [B, T, F, 32] output layout
    dict(B=1, Fin=1, T=5, sf=1),                           # a single row
]


def fcm_block_case(cdll, device, B, Fin, T, sf, strided_out=False, seed=0):
    """BasicResBlock (campplus.py:221-254) in one launch: ReLU(BN2(conv3x3(ReLU(BN1(conv3x3_s(x))))) + shortcut(x)) on fp16 maps,
    BatchNorms folded.  Reference in fp64 from the fp16 operands with the intermediate map rounded to fp16 (what the kernel feeds
    to the second conv's MFMAs)."""
    g = torch.Generator().manual_seed(seed)
    Fout = (Fin - 1) // sf + 1
    shortcut = 1 if sf == 2 else 0
    x = torch.randn(B, Fin, T, 32, generator=g).half()
    w1 = (torch.randn(9, 32, 32, generator=g) * 0.08).half()
    w2 = (torch.randn(10 if shortcut else 9, 32, 32, generator=g) * 0.08).half()
    b1 = torch.randn(32, generator=g) * 0.1
    b2 = torch.randn(32, generator=g) * 0.1
    if strided_out:      # y[b, t, fo, co]
        y = torch.full((B, T, Fout, 32), float('nan')).half().to(device)
        sB, sF, sT = T * Fout * 32, 32, Fout * 32
    else:                # y[b, fo, t, co]
        y = torch.full((B, Fout, T, 32), float('nan')).half().to(device)
        sB, sF, sT = Fout * T * 32, T * 32, 32
    xd, w1d, w2d, b1d, b2d = x.to(device), w1.to(device), w2.to(device), b1.to(device), b2.to(device)
    _hip.check(cdll.mv_fcm_block_f16(xd.data_ptr(), Fin, sf, w1d.data_ptr(), b1d.data_ptr(), w2d.data_ptr(), b2d.data_ptr(), shortcut,
                                     y.data_ptr(), sB, sF, sT, B, T, _stream(xd)), cdll)
    xin = x.double().permute(0, 3, 1, 2)                                         # [B, 32, F, T]
    k33 = lambda w: w[:9].double().reshape(3, 3, 32, 32).permute(2, 3, 0, 1).contiguous()  # [co, ci, df, dt]
    mid = F.conv2d(xin, k33(w1), b1.double(), stride=(sf, 1), padding=1).clamp(min=0).half().double()
    ref = F.conv2d(mid, k33(w2), b2.double(), padding=1)
    if shortcut:
        ref = ref + F.conv2d(xin, w2[9].double().reshape(32, 32, 1, 1), None, stride=(sf, 1))
    else:
        ref = ref + xin
    ref = ref.clamp(min=0).permute(0, 3, 2, 1) if strided_out else ref.clamp(min=0).permute(0, 2, 3, 1)
    out = y.cpu().double()
    assert torch.isfinite(out).all(), 'unwritten outputs'
    err = (out - ref).abs().max().item()
    # fp16 rounding of the stored result + an fp16 ulp flip of the intermediate map where the fp32 accumulation order differs
    assert err < 3e-3 * max(1.0, ref.abs().max().item()), err
    return err


FCM_BLOCK_C1_CASES = [
    dict(B=2, F=12, T=45),      # NT = 1, bands; frames outside [0, T) on both sides of the only tile
    dict(B=1, F=9, T=70),       # odd F (the last mid row reads the padding row below the map), NT = 2
    dict(B=1, F=5, T=330),      # two time tiles: halo columns across the tile edge
    dict(B=3, F=3, T=16),       # the smallest map: every row touches a padding bin
    dict(B=1, F=80, T=131),     # the product's row count
]


def fcm_block_c1_case(cdll, device, B, F, T, seed=0, scale=4.0, outlier=True):
    """head.conv1 + bn1 + ReLU (campplus.py:262-264,283) and the first BasicResBlock in one launch (mv_fcm_block_c1_f16).  Reference in
    fp64: the conv of the fp32 features with the fp16-rounded folded weights, rounded to fp16 (the map the block's MFMAs read), then
    the block as in fcm_block_case."""
    import ctypes
    import torch.nn.functional as Fn
    g = torch.Generator().manual_seed(seed)
    Fout = (F - 1) // 2 + 1
    feats = torch.randn(B, T, F, generator=g) * scale
    if outlier:   # (random-seed sweeps switch it off: where the outlier's large terms cancel in an output, the fp16 ulp of the intermediate maps -- the
        #            reference's too -- is 1e-2 of that output: a property of the metric below, seed-dependent)
        feats[0, T // 2, F // 2] = 20000.0                # far beyond fp16 precision of the hi part alone; exact as hi + lo
    c1w = torch.randn(32, 3, 3, generator=g) * 0.3        # [co][df][dt]
    c1b = torch.randn(32, generator=g) * 0.1
    w1 = (torch.randn(9, 32, 32, generator=g) * 0.08).half()
    w2 = (torch.randn(10, 32, 32, generator=g) * 0.08).half()
    b1 = torch.randn(32, generator=g) * 0.1
    b2 = torch.randn(32, generator=g) * 0.1
    packed = torch.zeros(2 * 64 * 8, dtype=torch.float16)
    c1w_c = c1w.contiguous()
    _hip.check(cdll.mv_fcm_c1_pack(c1w_c.data_ptr(), packed.data_ptr()), cdll)
    y = torch.full((B, Fout, T, 32), float('nan')).half().to(device)
    sB, sF, sT = Fout * T * 32, T * 32, 32
    fd, pd, cbd, w1d, w2d, b1d, b2d = (t.to(device) for t in (feats, packed, c1b, w1, w2, b1, b2))
    _hip.check(cdll.mv_fcm_block_c1_f16(fd.data_ptr(), F, pd.data_ptr(), cbd.data_ptr(), w1d.data_ptr(), b1d.data_ptr(), w2d.data_ptr(),
                                        b2d.data_ptr(), y.data_ptr(), sB, sF, sT, B, T, _stream(fd)), cdll)
    xin = feats.double().permute(0, 2, 1).unsqueeze(1)                                       # [B, 1, F, T]
    c1 = Fn.conv2d(xin, c1w.half().double().unsqueeze(1), c1b.double(), padding=1).clamp(min=0, max=65504).half().double()   # [B, 32, F, T]
    k33 = lambda w: w[:9].double().reshape(3, 3, 32, 32).permute(2, 3, 0, 1).contiguous()   # [co, ci, df, dt]
    mid = Fn.conv2d(c1, k33(w1), b1.double(), stride=(2, 1), padding=1).clamp(min=0).half().double()
    ref = Fn.conv2d(mid, k33(w2), b2.double(), padding=1) + Fn.conv2d(c1, w2[9].double().reshape(32, 32, 1, 1), None, stride=(2, 1))
    ref = ref.clamp(min=0, max=65504).permute(0, 2, 3, 1)
    out = y.cpu().double()
    assert torch.isfinite(out).all(), 'unwritten outputs'
    errs = (out - ref).abs() / ref.abs().clamp(min=1.0)
    err = errs.max().item()
    # fp16 rounding of the stored result + fp16 ulp flips of the two intermediate maps where the fp32 accumulation order differs
    if errs.numel() <= 10_000_000:
        assert err < 4e-3, err
        return err
    # The maximum of this metric grows with the number of outputs.  At the device fuzzer's largest shape (B = 64, F = 80, T = 998: 81.7 M outputs) twelve seeds
    # read 2.5e-3 ... 4.8e-3, two of them beyond 4e-3 with ONE output each (profiles/r15br/diag_fcm_c1_tail.log: 3.5-5.7 k outputs beyond 1e-3, 58-148 beyond 2e-3,
    # 0-12 beyond 3e-3, at scattered interior positions), every output inside what one fp16 ulp flip of each intermediate value in its receptive field can move it
    # (the largest ones 4.6 x or more inside).  Large maps are held to that distribution and to that bound instead of to the small maps' maximum.
    assert err < 6e-3 and int((errs > 4e-3).sum()) <= 1 + errs.numel() // 50_000_000, (err, int((errs > 4e-3).sum()))
    ulp = lambda v: torch.where(v > 0, torch.exp2(torch.floor(torch.log2(v.clamp(min=2.0 ** -14))) - 10), torch.zeros_like(v))
    bound = Fn.conv2d(ulp(mid), k33(w2).abs(), None, padding=1) + Fn.conv2d(ulp(c1), w2[9].double().abs().reshape(32, 32, 1, 1), None, stride=(2, 1))
    bound = bound.permute(0, 2, 3, 1) + 0.5 * ulp(ref.clamp(min=2.0 ** -14))
    assert bool(((out - ref).abs() <= bound).all()), 'an output beyond the one-ulp-flip bound of its receptive field'
    return err


def wave_prepare_case(cdll, device, B=5, L=5000, normalize=True, seed=0):
    from oracle import frontend
    g = torch.Generator().manual_seed(seed)
    pcm = (torch.randn(B, L, generator=g) * 3000).clamp(-32768, 32767).to(torch.int16)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0] = L
    pcm[1] = 0  # digital silence: the reference's normalize raises, the kernel flags the row
    wav, flags = _hip.wave_prepare(pcm.to(device), lens.to(device), -20.0 if normalize else None, cdll=cdll)
    ref, quiet = frontend.wave_prepare(pcm.numpy(), lens.numpy(), -20.0 if normalize else None)
    err = np.abs(wav.cpu().numpy() - ref).max()
    assert err < 2e-6 * max(1.0, np.abs(ref).max()), err
    assert flags.cpu().numpy().astype(bool).tolist() == quiet.tolist()
    return err


# kaldi.fbank keyword arguments (featurizer.py:128 forwards **kwargs) x launch options, shared by the emulator and the device sweep.
# (args, options): options = kernel ('auto' | 'generic' | 'tile'), cmn (False = bare kaldi.fbank rows, KaldiFbank), varlen (num_samples entry point)
_FB80 = dict(sample_frequency=16000, num_mel_bins=80)
FBANK_ARG_CASES = (
    [(dict(_FB80, frame_length=fl), dict(kernel='tile')) for fl in (20, 24, 25, 30)] +          # fbank_tile_kernel<16> (20 / 24 / 30 ms) and <13> (25 ms)
    [(dict(_FB80, frame_length=fl), dict(kernel='generic')) for fl in (20, 24, 25, 30, 32)] +   # fbank_kernel on the same geometries
    [(dict(_FB80, frame_shift=12.5), dict(kernel='tile')), (dict(_FB80, frame_shift=12.5, frame_length=20), dict(kernel='generic'))] +
    [(dict(sample_frequency=16000, num_mel_bins=nb), {}) for nb in (23, 40, 64, 128)] +
    [(dict(sample_frequency=16000), {})] +                                                     # num_mel_bins default (23)
    [(dict(sample_frequency=8000, num_mel_bins=nb), {}) for nb in (23, 40, 64)] +               # 200-sample window: kaldi's 256-point FFT
    [(dict(sample_frequency=8000, num_mel_bins=40, frame_length=fl, frame_shift=fs), {}) for fl, fs in ((20, 10), (30, 12.5))] +
    [(dict(sample_frequency=22050, num_mel_bins=64, frame_length=20), {}), (dict(sample_frequency=11025, num_mel_bins=40), {})] +  # odd window (275)
    [(dict(_FB80, low_freq=100, high_freq=-400), {}), (dict(_FB80, high_freq=7000), {}), (dict(_FB80, low_freq=0), {}),
     (dict(sample_frequency=8000, num_mel_bins=40, low_freq=60, high_freq=3800), {})] +
    [(dict(_FB80, use_power=False), {}), (dict(_FB80, use_log_fbank=False), {}), (dict(_FB80, use_power=False, use_log_fbank=False), {}),
     (dict(_FB80, remove_dc_offset=False), {}), (dict(_FB80, preemphasis_coefficient=0.0), {}),
     (dict(_FB80, remove_dc_offset=False, preemphasis_coefficient=0.0), dict(kernel='generic')),
     (dict(sample_frequency=16000, num_mel_bins=40, remove_dc_offset=False, preemphasis_coefficient=0.5), {})] +
    [(dict(_FB80, window_type=w), {}) for w in ('hamming', 'hanning', 'rectangular', 'blackman')] +
    [(dict(sample_frequency=16000, num_mel_bins=40, window_type='blackman', blackman_coeff=0.4), {})] +
    [(dict(_FB80, snip_edges=False), {}), (dict(_FB80, snip_edges=False, frame_shift=30.0), {}), (dict(_FB80, snip_edges=False), dict(varlen=True)),
     (dict(sample_frequency=8000, num_mel_bins=23, snip_edges=False), dict(cmn=False))] +
    [(dict(_FB80, subtract_mean=True), {}), (dict(_FB80, subtract_mean=True), dict(cmn=False)), (dict(_FB80, min_duration=0.3), dict(varlen=True))] +
    [(dict(_FB80, vtln_warp=1.1), {}), (dict(_FB80, vtln_warp=0.9), dict(cmn=False)), (dict(sample_frequency=16000, num_mel_bins=40, vtln_warp=1.2, vtln_low=300.0, vtln_high=-800.0), {}),
     (dict(sample_frequency=8000, num_mel_bins=23, vtln_warp=0.85, vtln_high=-300.0), dict(varlen=True))] +    # kaldi's VTLN warp of the filter edges
    [(dict(_FB80), dict(cmn=False)), (dict(_FB80), dict(cmn=False, kernel='generic')), (dict(_FB80), dict(varlen=True, kernel='generic')),
     (dict(sample_frequency=16000, num_mel_bins=23), dict(cmn=False))] +
    # use_energy (round 6): the log-energy column in front of / behind the mel columns, raw or windowed, floored or not; with the time mean and the mask,
    # bare, on true lengths, on the mirrored signal, on both kernels
    [(dict(_FB80, use_energy=True), {}), (dict(_FB80, use_energy=True, htk_compat=True), dict(kernel='generic')),
     (dict(_FB80, use_energy=True, raw_energy=False), {}), (dict(_FB80, use_energy=True, raw_energy=False, energy_floor=0.0), dict(cmn=False)),
     (dict(_FB80, use_energy=True, energy_floor=0.0, remove_dc_offset=False), dict(varlen=True)),
     (dict(sample_frequency=8000, num_mel_bins=23, use_energy=True, energy_floor=1e-3, snip_edges=False, htk_compat=True), {}),
     (dict(_FB80, use_energy=True, raw_energy=False, preemphasis_coefficient=0.0, window_type='hamming', subtract_mean=True), dict(cmn=False)),
     (dict(sample_frequency=16000, num_mel_bins=40, use_energy=True, energy_floor=0.0, snip_edges=False), dict(varlen=True))])


FBANK_FRAME_LENGTHS = [20.0, 24.0, 25.0, 26.0, 27.0, 28.0, 30.0, 32.0]   # ms at 16 kHz: 10, 12, 13, 13, 14, 14, 15, 16 groups of 32 samples


def fbank_frame_length_case(cdll, device, frame_length):
    """80 bins at one frame length on rows that start on 8-byte boundaries (the VEC2 instantiations): fbank_tile_kernel and fbank_kernel against the oracle"""
    from oracle import frontend
    args = dict(_FB80, frame_length=frame_length)
    assert _hip.Fbank(args, cdll=cdll).info()['tile_kernel']
    assert not _hip.Fbank(args, cdll=cdll, kernel='generic').info()['tile_kernel']
    wav = frontend.synth_waveforms(2, 24080, seed=3)
    ratio = torch.tensor([1.0, 0.6])
    fbank_case(cdll, device, wav, ratio, args)
    fbank_case(cdll, device, wav, ratio, args, kernel='generic')


def fbank_generic_waves(pass_steps):
    """waves per workgroup of fbank_kernel by the LDS rule of csrc/fbank.hip (generic_waves): the most of 15, 12, 8 whose frame slots (4 frames of 548
    floats per wave) fit 160 KB next to three 512-float tables and the mel weights (64 floats per step of the two passes)"""
    for waves in (15, 12, 8):
        if (waves * 4 * 548 + 3 * 512 + 64 * sum(pass_steps)) * 4 <= 160 * 1024:
            return waves
    return 0


_VTLN12 = dict(sample_frequency=16000, num_mel_bins=40, vtln_warp=1.2, vtln_low=300.0, vtln_high=-800.0)   # 104 mel steps: fbank_kernel on 12 waves


def fbank_generic_kernel_rows(cdll):
    """Which rows of fbank.hip's GENERIC_KERNELS table -- (13 or 16 sample groups, alignment, waves) -- the Fbank tests launch.  The groups follow the
    window (FBANK_ARG_CASES and test_*_fbank_other_frame_lengths_with_80_bins hold 400- and 416-sample windows = 13 groups, and others = 16), the
    alignment the rows (odd strides in fbank_arguments_case, even ones in the frame-length sweep), the waves the mel table: computed here for every
    configuration of both lists, 15 each time except the 40-bin VTLN warp of 1.2 (104 steps, 15 waves hold 102), which runs <13, unaligned, 12>; the
    other three 12-wave rows are fbank_generic_12_waves_case's.  The 8-wave rows (more than 205 steps) are launched by no test: no configuration
    that reaches them is known."""
    cfgs = [args for args, _ in FBANK_ARG_CASES] + [dict(_FB80, frame_length=fl) for fl in FBANK_FRAME_LENGTHS]
    for args in cfgs:
        steps = _hip.Fbank(args, cdll=cdll, kernel='generic').info()['pass_steps']
        assert fbank_generic_waves(steps) == (12 if args.get('vtln_warp') == 1.2 else 15), (args, steps)


FBANK_12_WAVE_CASES = [(25.0, False), (20.0, False), (20.0, True)]   # (frame_length, misaligned) = the rows <13, aligned>, <16, aligned>, <16, unaligned>


def fbank_generic_12_waves_case(cdll, device, frame_length, misaligned):
    """fbank_kernel<NG, VEC2, 12> on B = 2, T = 5 frames (one full quad and one partial) against the oracle"""
    from oracle import frontend
    args = dict(_VTLN12, frame_length=frame_length)
    assert fbank_generic_waves(_hip.Fbank(args, cdll=cdll, kernel='generic').info()['pass_steps']) == 12
    wav = frontend.synth_waveforms(2, int(16 * frame_length) + 160 * 4, seed=52)
    return fbank_case(cdll, device, wav, torch.tensor([1.0, 0.6]), args, kernel='generic', misaligned=misaligned)


def fbank_tile_16_groups_unaligned_case(cdll, device, form):
    """fbank_tile_kernel<16, VEC2 = false>, the one row of fbank.hip's TILE_KERNELS table no other test launches (the 80-bin tests with unaligned
    rows hold windows of 10 / 12 / 13 / 15 sample groups): a 28 ms window (448 samples = 14 groups, no row of its own) on a waveform view that starts
    one float into its buffer.  form 'chunked': B = 2, T = 64 frames with the product workspace (two chunks of 8 quads + the finish pass);
    'beyond_lds': B = 2, T = 300 frames on one workgroup each, more rows than stay in LDS."""
    from oracle import frontend
    args = dict(_FB80, frame_length=28.0)
    T = dict(chunked=64, beyond_lds=300)[form]
    wav = frontend.synth_waveforms(2, 448 + 160 * (T - 1), seed=51)
    assert _hip.Fbank(args, cdll=cdll, kernel='tile').num_frames(wav.shape[1]) == T
    return fbank_case(cdll, device, wav, torch.tensor([1.0, 0.7]), args, kernel='tile', misaligned=True, workspace=form == 'chunked')


def fbank_arguments_case(cdll, device, idx, B=3, seconds=0.5, seed=None, check_rows=None):
    """one entry of FBANK_ARG_CASES on B utterances of `seconds`: a fixed-length batch with a length mask (or bare rows / ragged true lengths).
    check_rows: compare only these rows with the oracle (rows are independent; a batch larger than the chip then costs a few oracle rows)"""
    args, opt = FBANK_ARG_CASES[idx]
    from oracle import frontend
    sf = int(args.get('sample_frequency', 16000))
    L = int(sf * seconds) + 37
    wav = frontend.synth_waveforms(B, L, seed=100 + idx if seed is None else seed)
    cmn = opt.get('cmn', True)
    ns = ratio = None
    if opt.get('varlen'):
        ns = torch.tensor([L, int(0.62 * L), int(0.45 * L), L - 1, int(0.8 * L)] * (B // 5 + 1))[:B]
    elif cmn:
        ratio = torch.tensor([1.0, 0.61, 0.8, 0.33, 0.5] * (B // 5 + 1))[:B]
    return fbank_case(cdll, device, wav, ratio, args, kernel=opt.get('kernel', 'auto'), cmn=cmn, num_samples=ns, check_rows=check_rows)


def fbank_min_duration_edge(cdll, device):
    """A clip of EXACTLY min_duration: torchaudio compares `len(waveform) < min_duration * sample_frequency` in double, so 0.1 s at
    16 kHz = 1600 samples is featurised (8 frames) and 1599 samples are not; the float32 field of the struct alone rounds the threshold to 1601.
    Rows of 1600 / 1599 / 1601 / 3200 samples through the variable-length entry point on both kernels, and the frame count query."""
    from oracle import frontend
    for md, sf in ((0.1, 16000), (0.3, 16000), (0.2, 8000)):
        args = dict(sample_frequency=sf, num_mel_bins=80 if sf == 16000 else 23, min_duration=md)
        edge = int(round(md * sf))
        assert edge == md * sf   # the double product is exact on these values: the edge is the integer itself
        wav = frontend.synth_waveforms(4, 2 * edge, seed=11)
        ns = torch.tensor([edge, edge - 1, edge + 1, 2 * edge])
        for kernel in ('auto', 'generic'):
            fb = _hip.Fbank(args, cdll=cdll, kernel=kernel)
            assert fb.num_frames(edge) == frontend.kaldi_fbank(wav[0, :edge].unsqueeze(0), **args).shape[0] > 0, (md, sf, kernel)
            assert fb.num_frames(edge - 1) == 0
            fbank_case(cdll, device, wav, None, args, kernel=kernel, num_samples=ns)


def fbank_case(cdll, device, wav, ratio, method_args, kernel='auto', cmn=True, num_samples=None, check_rows=None, misaligned=False, workspace=True):
    """HIP Fbank (+ time mean + mask) against the fp32 oracle AND the fp64 arbiter of the same algorithm.  `kernel`: 'auto' | 'generic' | 'tile'
    (MvFbankCfg.kernel).  cmn=False: the bare kaldi.fbank rows (KaldiFbank, featurizer.py:114-132).  num_samples: the variable-length entry point
    (every row on its own length, zero rows behind it).  misaligned: the waveform is a view that starts one float into its buffer (the kernels'
    VEC2 = false instantiations).  workspace=False: one workgroup per utterance.  Log energies are compared in absolute terms (the stated 1e-3);
    linear ones (use_log_fbank=False) relative to the largest energy of the batch."""
    from oracle import frontend
    fb = _hip.Fbank(method_args, cdll=cdll, kernel=kernel, subtract_time_mean=cmn)
    dwav = wav.to(device)
    if misaligned:
        flat = torch.empty(wav.numel() + 1, device=device)
        flat[1:] = wav.reshape(-1)
        dwav = flat[1:].view(wav.shape)
        assert dwav.data_ptr() % 8 == 4 and dwav.is_contiguous()
    out = fb(dwav, None if ratio is None else ratio.to(device), None if num_samples is None else num_samples.to(device), workspace=workspace).cpu()
    if check_rows is not None:   # the launch saw the whole batch; the oracle only these rows
        rows = torch.as_tensor(check_rows)
        out, wav = out[rows], wav[rows]
        ratio = None if ratio is None else ratio[rows]
        num_samples = None if num_samples is None else num_samples[rows]

    def oracle(fn):
        if num_samples is not None:
            rows = []
            for w, n in zip(wav, num_samples.tolist()):
                f = fn(w[:n].unsqueeze(0), **method_args)
                f = f.reshape(-1, out.shape[2]) if f.numel() else f.new_zeros((0, out.shape[2]))
                if cmn and f.shape[0]:
                    f = f - f.mean(0, keepdim=True)
                rows.append(torch.cat([f, f.new_zeros((out.shape[1] - f.shape[0], out.shape[2]))]))
            return torch.stack(rows)
        if not cmn:
            assert ratio is None
            return torch.stack([fn(w.unsqueeze(0), **method_args) for w in wav])
        if fn is frontend.kaldi_fbank:
            return frontend.audio_featurizer(wav, ratio, 'Fbank', method_args)
        return frontend.audio_featurizer_fbank_f64(wav, ratio, method_args)
    if out.numel() == 0:   # no frames (shorter than a window, or than min_duration -- where kaldi.fbank returns a bare empty tensor the reference's
        assert wav.shape[0] == 0 or all(frontend.kaldi_fbank(w.unsqueeze(0), **method_args).numel() == 0 for w in wav)   # wrapper cannot stack)
        return 0.0
    ref = oracle(frontend.kaldi_fbank)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    ref64 = oracle(frontend.kaldi_fbank_f64)
    scale = 1.0 if dict(method_args).get('use_log_fbank', True) else max(float(ref64.abs().max()), 1e-30)
    d = (out - ref).abs() / scale
    # ... and where the fp32 oracle ITSELF sits more than 1e-3 from the arbiter it is no yard-stick for the kernel: those values are left to the arbiter's bar below
    # (device fuzz r15bt, reproduced bit for bit on the emulator: magnitude spectrum, 26 ms frames, the utterance's lowest log energy at -10.7 against a median of 0.5:
    # torch-fp32 6.5e-3 from the arbiter, the kernel 6.0e-4 -- the pair 7.1e-3 apart)
    d = torch.where(((ref.double() - ref64).abs() / scale) > 1e-3, torch.zeros_like(d), d)
    # Two fp32 evaluations of a near-floor log energy (a small difference of fp32 spectra: the bins next to DC, where the pre-emphasis leaves 1e-3 of
    # the power and the transform's rounding noise is that of the whole frame) differ by more than either differs from the exact value.  So the STATED
    # bar (SURVEY 8(c) / BASELINE.md 3: max-abs <= 1e-3) is asserted against the fp64 arbiter of the same algorithm, and as what fp32 can keep: every
    # value within 1e-3 except isolated near-floor bins -- at most 1 + 2 per million values, none beyond 3e-3 -- which is also where the torch-fp32
    # oracle itself sits (device fuzz r14a: B x L = 256 x 52000, oracle32 1.15e-3 / HIP 1.01e-3 from the arbiter on one bin of 3.3 M).  Kernel vs
    # fp32 oracle keeps the looser 2e-3 the same way.
    n = d.numel()
    assert int((d > 2e-3).sum()) <= n * 1e-5 and d.max().item() < 5e-3, (d.max().item(), int((d > 2e-3).sum()), n)
    assert d.mean().item() < 2e-5, d.mean().item()
    fbank_within_stated_bar(out, ref64, scale, ref)
    return d.max().item()


def fbank_within_stated_bar(out, ref64, scale=1.0, ref32=None):
    """|HIP - fp64 arbiter| <= 1e-3 on every value except isolated near-floor bins: at most 1 + 2 per million values, none beyond 3e-3 (beyond
    1.5e-3 in blocks of < 100 k values); mean <= 1e-5.  (Device fuzz r14c: one value of 38 k at 1.03e-3 where the fp32 oracle has 0.92e-3.)"""
    e_hip = (out.double() - ref64).abs() / scale
    n, over = e_hip.numel(), int((e_hip > 1e-3).sum())
    note = () if ref32 is None else ('oracle32', ((ref32.double() - ref64).abs() / scale).max().item())
    assert over <= 1 + 2e-6 * n and e_hip.max().item() < (3e-3 if n >= 100000 else 1.5e-3), (e_hip.max().item(), over, n) + note
    assert e_hip.mean().item() <= 1e-5, e_hip.mean().item()
    return e_hip


def model_case(cdll, device, case, tol=1e-4, max_batch=None, info=None, frames=None, head=0, xvec_probe=None):
    """Golden case through the native model handle (weights from the manifest, reference embedding from golden).  `info`: a dict
    that receives {key: mv_model_info(key)} for the keys it holds (CAM++: 1 = head on fp32 maps, 2 = creation-time calibration).
    `frames`: instead of the golden input, one seeded utterance of that many frames with the golden input's statistics, the reference
    embedding from the oracle (pinned to the reference modules by the goldens)."""
    from helpers import load_case, cos_dist
    man, sd, x, emb_ref, _ = load_case(case)
    if frames is not None:
        from oracle import models as omodels
        g = torch.Generator().manual_seed(frames)
        x = torch.randn(1, frames, x.shape[2], generator=g) * x.std() + x.mean()
        emb_ref = omodels.FORWARDS[man['model']](sd, x)
    if max_batch is not None:
        x, emb_ref = x[:max_batch], emb_ref[:max_batch]
    kw = man['kwargs']
    if man['model'] == 'EcapaTdnn':
        cfg = _hip.MvEcapaCfg()
        cfg.input_size, cfg.embd_dim = kw['input_size'], kw.get('embd_dim', 192)
        ch = kw.get('channels', [512, 512, 512, 512, 1536])
        for i in range(5):
            cfg.channels[i], cfg.kernel_sizes[i], cfg.dilations[i] = ch[i], [5, 3, 3, 3, 1][i], [1, 2, 3, 4, 1][i]
        cfg.attention_channels, cfg.res2net_scale, cfg.se_channels, cfg.global_context = 128, 8, 128, 1
        kind = 'ecapa'
    elif man['model'] == 'TDNN':
        cfg = _hip.MvTdnnCfg()
        cfg.input_size, cfg.channels, cfg.embd_dim = kw['input_size'], kw.get('channels', 512), kw.get('embd_dim', 192)
        kind = 'tdnn'
    elif man['model'] in ('ERes2Net', 'ERes2NetV2'):
        v2 = man['model'] == 'ERes2NetV2'
        cfg = _hip.MvEres2Cfg()
        cfg.version, cfg.input_size, cfg.embd_dim = (2 if v2 else 1), kw['input_size'], kw.get('embd_dim', 192)
        for i, n in enumerate(kw.get('num_blocks', [3, 4, 6, 3])):
            cfg.num_blocks[i] = n
        cfg.m_channels, cfg.mul_channel, cfg.expansion = kw.get('m_channels', 32), 1, 2
        cfg.base_width, cfg.scale = kw.get('base_width', 26 if v2 else 32), kw.get('scale', 2)
        cfg.two_emb_layer = int(kw.get('two_emb_layer', False))
        kind = 'eres2net'
    else:
        cfg = _hip.MvCamppCfg()
        cfg.input_size, cfg.embd_dim = kw['input_size'], kw.get('embd_dim', 512)
        cfg.growth_rate, cfg.bn_size, cfg.init_channels = kw.get('growth_rate', 32), kw.get('bn_size', 4), kw.get('init_channels', 128)
        cfg.head_precision = head   # MV_CAMPP_HEAD_AUTO (0) / _F16 (1) / _F32 (2)
        # the creation-time x-vector sensitivity probe (three utterances through ~330 exact-fp32 GEMM launches): on by default on the device,
        # off under the emulator (5 minutes there) unless a test asks for it
        cfg.xvector_probe = 0 if (xvec_probe if xvec_probe is not None else str(device) != 'cpu') else 1
        kind = 'campp'
    sd_dev = {k: v.to(device) for k, v in sd.items()}
    m = _hip.Model(kind, cfg, sd_dev, cdll=cdll)
    emb = m.forward(x.to(device)).cpu()
    if info is not None:   # (after the forward: keys 8 / 9 report what the exact CAM++ head saw on this input)
        for key in list(info):
            info[key] = m.info(key)
    cd = cos_dist(emb, emb_ref).max().item()
    rel = ((emb - emb_ref).norm(dim=1) / emb_ref.norm(dim=1)).max().item()
    assert cd < tol, f'{case}: 1-cos {cd}'
    return cd, rel


def melspec_case(cdll, device, wav, ratio, method_args, rtol=2e-4):
    from oracle import frontend
    ms = _hip.MelSpec(method_args, cdll=cdll)
    out = ms(wav.to(device), None if ratio is None else ratio.to(device)).cpu()
    ref = frontend.audio_featurizer(wav, ratio, 'MelSpectrogram', method_args)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    scale = ref.abs().max().item()
    err = (out - ref).abs().max().item()
    assert err <= rtol * scale + 1e-6, (err, scale)
    return err / scale if scale > 0.0 else err   # (a single frame: the time mean takes everything away)


# MelSpectrogram(**method_args) keyword arguments beyond the shipped configurations (featurizer.py:41-42), shared by the emulator and the device sweep;
# every FFT kernel (n_fft 400: melspec_tile_kernel, powers of two: melspec_pow2_kernel) and the dense-DFT path meets each table option
MELSPEC_ARG_CASES = [
    dict(mel_scale='slaney'), dict(norm='slaney'), dict(mel_scale='slaney', norm='slaney'),
    dict(normalized=True), dict(normalized='window', n_fft=512), dict(normalized='frame_length'), dict(normalized='frame_length', n_fft=480, n_mels=64),
    dict(window_fn=torch.hamming_window), dict(window_fn=torch.blackman_window, wkwargs=dict(periodic=False), n_fft=1024, hop_length=320, n_mels=64),
    dict(window_fn=torch.kaiser_window, wkwargs=dict(periodic=True, beta=8.0), n_fft=320, win_length=300, hop_length=100, n_mels=40),
    dict(power=1.0), dict(power=1.5, n_fft=512), dict(power=3.0, n_mels=64), dict(power=1.0, n_fft=256, mel_scale='slaney', norm='slaney', n_mels=40),
    dict(center=False), dict(center=False, n_fft=512, hop_length=160, norm='slaney'),
    dict(sample_rate=8000, n_fft=256, n_mels=40, f_min=60.0, f_max=3800.0, mel_scale='slaney'),
    dict(sample_rate=22050, n_fft=1024, hop_length=256, n_mels=80, f_min=0.0, f_max=8000.0, norm='slaney', mel_scale='slaney'),   # librosa-style
    dict(n_fft=400, win_length=320, hop_length=160, n_mels=80, normalized=True, window_fn=torch.hann_window, wkwargs=dict(periodic=False)),
    # pad / pad_mode (round 6): zeros around the signal, the centre extension in torch.stft's other modes -- on the n_fft = 400 FFT kernel, the
    # power-of-two FFT kernel and the dense DFT
    dict(pad=37), dict(pad_mode='constant'), dict(pad_mode='replicate', n_fft=512), dict(pad_mode='circular', n_fft=480, n_mels=64),
    dict(pad=200, pad_mode='constant', center=True, n_fft=256, n_mels=40), dict(pad=64, center=False), dict(pad=5, pad_mode='circular', hop_length=160),
]


def melspec_arguments_case(cdll, device, idx, B=3, seconds=0.5):
    from oracle import frontend
    args = MELSPEC_ARG_CASES[idx]
    L = int(args.get('sample_rate', 16000) * seconds) + 37
    wav = frontend.synth_waveforms(B, L, seed=200 + idx)
    ratio = torch.tensor([1.0, 0.61, 0.8, 0.33, 0.5] * (B // 5 + 1))[:B]
    return melspec_case(cdll, device, wav, ratio, args)


def res2_chain_case(cdll, device, B=2, T=45, width=64, groups=8, k=3, dil=3, seed=0, alone_rows=0, gain=1.0):
    """Fused Res2Net chain vs a torch fp32 evaluation that rounds to fp16 exactly where the kernel does.  gain: multiplies the BatchNorm scales --
    large values drive the step outputs and the next-input sums beyond the fp16 range, where the kernel saturates at +-65504 (MODE.FP16_OVFL since
    round 6; v_med3 / packed min / max before) and never produces an infinity."""
    g = torch.Generator().manual_seed(seed)
    C = width * groups
    x = torch.randn(B, T, C, generator=g).half()
    ws = [torch.randn(width, width, k, generator=g) * (2.0 / (width * k)) ** 0.5 for _ in range(groups - 1)]
    bs = [torch.randn(width, generator=g) * 0.1 for _ in range(groups - 1)]
    ss = [(torch.rand(width, generator=g) + 0.5) * gain for _ in range(groups - 1)]
    ts = [torch.randn(width, generator=g) * 0.1 for _ in range(groups - 1)]
    xd = x.to(device)
    y = torch.full((B, T, C), 9.0, dtype=torch.float16, device=device)
    packed = [pack_weight(cdll, w.to(device)) for w in ws]
    dev = [[t.to(device).contiguous() for t in lst] for lst in (bs, ss, ts)]
    arr = lambda lst: (ctypes.c_void_p * len(lst))(*[t.data_ptr() for t in lst])
    _hip.check(cdll.mv_res2net_chain_f16(xd.data_ptr(), y.data_ptr(), arr(packed), arr(dev[0]), arr(dev[1]), arr(dev[2]), B, T, C,
                                         groups, k, dil, _stream(xd)), cdll)
    if device != 'cpu':
        torch.cuda.synchronize()
    xs = x.float().transpose(1, 2)  # [B, C, T]
    outs = [xs[:, :width]]
    prev = None
    pad = dil * (k - 1) // 2
    for j in range(1, groups):
        inp = xs[:, j * width:(j + 1) * width]
        if j > 1:
            inp = (inp + prev).clamp(-65504.0, 65504.0).half().float()
        z = F.conv1d(F.pad(inp, (pad, pad), mode='reflect'), ws[j - 1].half().float(), bs[j - 1], dilation=dil)
        z = torch.relu(z) * ss[j - 1].view(1, -1, 1) + ts[j - 1].view(1, -1, 1)
        prev = z.clamp(-65504.0, 65504.0).half().float()
        outs.append(prev)
    ref = torch.cat(outs, 1).transpose(1, 2)
    got = y.cpu().float()
    assert bool(torch.isfinite(got).all()), 'the chain produced an infinity or a NaN'
    if gain > 1.0:
        assert (ref.abs() == 65504.0).float().mean().item() > 0.05, 'the case does not saturate'
        sat = ref.abs() == 65504.0
        assert bool((got[sat] == ref[sat]).float().mean() > 0.99), 'saturated values differ'
        # (sums of saturated inputs cancel: where a pre-activation lands within rounding of zero, ReLU x gain turns an fp32 ordering difference into
        #  0 against 65504 -- a property of the case, not of the kernel; the bulk must agree)
        far = ((got - ref).abs() > 1e-2 * 65504.0).float().mean().item()
        assert far < 0.01, far
        return far
    err = (got - ref).abs().max().item()
    assert err < 1e-2 * max(1.0, ref.abs().max().item()), err
    if alone_rows:
        # the same utterances one at a time: a small batch takes the 5-tile chunk form (<= 160 frames per workgroup, halo rows), a batch that
        # fills the chip one workgroup per utterance (or 304-frame chunks) -- every stored row is computed from the rows it sees in the unchunked
        # run with the same arithmetic, so the bits agree
        for b in range(min(alone_rows, B)):
            y1 = torch.full((1, T, C), 9.0, dtype=torch.float16, device=device)
            x1 = xd[b:b + 1].contiguous()
            _hip.check(cdll.mv_res2net_chain_f16(x1.data_ptr(), y1.data_ptr(), arr(packed), arr(dev[0]), arr(dev[1]), arr(dev[2]), 1, T, C,
                                                 groups, k, dil, _stream(xd)), cdll)
            assert torch.equal(y1[0].cpu(), y[b].cpu()), (b, (y1[0].cpu().float() - y[b].cpu().float()).abs().max().item())
    return err


# ---- CAM++ dense layers (mv_cam_dense_block_f16): cases and bars in tests/cam_cases.py, reference in tests/cam_ref.py ----
CAM_SENTINEL = 7.0


def cam_dense_params(cdll, device, layers):
    """the per-layer tensors of a cam_cases.build() on the device, w1 / wl packed as the kernels read them"""
    out = []
    for p in layers:
        d = {k: v.to(device).contiguous() for k, v in p.items()}
        d['w1'] = pack_weight(cdll, p['w1'].unsqueeze(2).to(device))
        d['wl'] = pack_weight(cdll, p['wl'].to(device))
        out.append(d)
    return out


def cam_dense_launch(cdll, device, x0, params, c_in, nlayers, dil, seg_len, form, pad):
    """one launch on a fresh buffer: inputs | NaN where the layers write | sentinel in the pitch columns -> (buffer on the CPU, forms used)"""
    B, T2, _ = x0.shape
    c_out = c_in + 32 * nlayers
    buf = torch.full((B, T2, c_out + pad), CAM_SENTINEL, dtype=torch.float16)
    buf[..., :c_in] = x0
    buf[..., c_in:c_out] = float('nan')
    xd = buf.to(device)
    used = _hip.cam_dense_block(xd, c_in, params, dil, seg_len, form, cdll=cdll)
    if device != 'cpu':
        torch.cuda.synchronize()
    return xd.cpu(), used


def cam_dense_case(cdll, device, name, log=print):
    """One case of tests/cam_cases.py: every layer of the launch against the fp64 layer on the device's OWN input channels, max-abs and mean-abs over
    all layers' new channels within the case's bars; inputs bit-unchanged, pitch columns untouched, every output finite (the output region is NaN
    before the launch: a layer that read a predecessor's channels before they landed shows up).  Returns (buffer, max-abs, mean-abs)."""
    import cam_cases as cc
    import cam_ref
    c = cc.CASES[name]
    x0, layers = cc.build(name)
    params = cam_dense_params(cdll, device, layers)
    got, used = cam_dense_launch(cdll, device, x0, params, c['c_in'], c['nlayers'], c['dil'], c['seg_len'], c['form'], c['pad'])
    c_out = c['c_in'] + 32 * c['nlayers']
    assert used == [cc.run_form(c)] * c['nlayers'], f'{name}: forms {used}'
    assert torch.equal(got[..., :c['c_in']].view(torch.int16), x0.view(torch.int16)), f'{name}: the input channels changed'
    assert bool((got[..., c_out:] == CAM_SENTINEL).all()), f'{name}: the launch wrote into the pitch columns'
    new = cc.new_channels(got, c)
    assert bool(torch.isfinite(new.float()).all()), f'{name}: {int((~torch.isfinite(new.float())).sum())} outputs are not finite (NaN: never written, or computed from channels that had not landed)'
    ref, gates = cam_ref.teacher_forced(got, c['c_in'], layers, c['dil'], c['seg_len'], return_gates=True)
    cc.check_gate_spread(gates, name)
    mx, mean = cc.distances(new, ref)
    bmx, bmean = cc.bars(name)
    per_layer = (new.double() - ref).abs().reshape(-1, c['nlayers'], 32).amax((0, 2))
    log(f'cam_dense {name}: form {cc.run_form(c)} max-abs {mx:.3e} (bar {bmx:.3e}, {mx / bmx:.2f}) mean-abs {mean:.3e} (bar {bmean:.3e}, {mean / bmean:.2f}) '
        f'worst layer {int(per_layer.argmax())}')
    assert mx <= bmx and mean <= bmean, f'{name}: max-abs {mx:.3e} (bar {bmx:.3e}), mean-abs {mean:.3e} (bar {bmean:.3e}), per layer {per_layer.tolist()}'
    return got, mx, mean


def cam_dense_batch_rows_case(cdll, device, form, T2, c_in, nlayers, dil, seg_len=100, B=5):
    """row b of a B = 5 launch carries the same bits as the B = 1 launch on that row (one workgroup, or one column of workgroups, per utterance;
    no summation crosses utterances)"""
    import cam_cases as cc
    name = f'rows_form{form}'
    cc.CASES[name] = cc._case(form, T2, c_in, nlayers, dil, seg_len, B=B)
    try:
        x0, layers = cc.build(name)
    finally:
        del cc.CASES[name]
    params = cam_dense_params(cdll, device, layers)
    full, _ = cam_dense_launch(cdll, device, x0, params, c_in, nlayers, dil, seg_len, form, 8)
    assert bool(torch.isfinite(full.float()).all())
    for b in range(B):
        one, _ = cam_dense_launch(cdll, device, x0[b:b + 1], params, c_in, nlayers, dil, seg_len, form, 8)
        assert torch.equal(one[0].view(torch.int16), full[b].view(torch.int16)), (form, b, (one[0].float() - full[b].float()).abs().max().item())


def cam_dense_refusal_case(cdll, device, form, T2, c_in, nlayers, dil, seg_len):
    """a pinned form outside its predicate: MV_ERR_UNSUPPORTED with a message naming the form, the buffer untouched"""
    import cam_cases as cc
    name = 'refusal'
    cc.CASES[name] = cc._case(form, T2, c_in, nlayers, dil, seg_len, B=1)
    try:
        x0, layers = cc.build(name)
    finally:
        del cc.CASES[name]
    params = cam_dense_params(cdll, device, layers)
    try:
        got, _ = cam_dense_launch(cdll, device, x0, params, c_in, nlayers, dil, seg_len, form, 0)
    except RuntimeError as e:
        assert f'form {form}' in str(e) and f'(code {_hip.MV_ERR_UNSUPPORTED})' in str(e), str(e)
        return str(e)
    raise AssertionError(f'form {form} accepted T2 {T2}, c_in {c_in}, seg_len {seg_len}: {torch.isfinite(got.float()).all()}')


# ------------------------------------------------------------------------------------------------ csrc/pool.hip: reductions and row passes, per kernel
# One case function per launcher, the same for the emulator (tests/test_pool_rows.py) and the device (tests/test_gpu_pool_rows.py).  Every case:
# an fp64 reference from the fp16-rounded operands the kernel sees; pitch columns (and a guard behind contiguous buffers) filled with a sentinel that
# must come back bit-unchanged; inputs bit-unchanged; the output region NaN before the call, so an element nobody wrote shows up.

POOL_SENTINEL = 7.0
U32 = 2.0 ** -24        # unit roundoff of fp32 (round to nearest)


def _gamma(m):
    """the standard bound of m consecutive fp32 roundings"""
    return m * U32 / (1.0 - m * U32)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _dev_copy(t, device):
    """a device copy whose storage is the test's own (on the CPU `.to` would alias the original and hide a kernel that writes its input)"""
    return t.clone().to(device)


def _raises(fn, cdll):
    """the message of a refused call (the launcher returned an error code)"""
    rc = fn()
    assert rc != 0, 'the call was accepted'
    return cdll.mv_last_error().decode(errors='replace')


def time_stats_data(B, T, C, ld, seed=0):
    """fp16 rows [B, T, ld], drawn utterance by utterance (row b is the same whatever B is); channel 3 constant, sentinel in the pitch columns"""
    x = torch.empty(B, T, ld, dtype=torch.float16)
    for b in range(B):
        x[b] = (torch.randn(T, ld, generator=torch.Generator().manual_seed(1000 + 7919 * seed + b)) * 2 + 0.5).half()
    x[:, :, 3] = 1.25
    x[..., C:] = POOL_SENTINEL
    return x


def time_stats_launch(cdll, device, x, C, want_std=True, unbiased=0, eps=1e-12, pre=None, out_pad=0, joint=False):
    """mv_time_stats_ex_f16 on x (fp16 [B, T, ld], CPU).  joint: mean | std in ONE row of pitch 2C + out_pad, std = mean + C (CAM++ StatsPool);
    else two buffers of pitch C + out_pad.  Checks inputs, pitch columns and that every output was written; returns (mean, std) [B, C] on the CPU."""
    B, T, ld = x.shape
    xd = _dev_copy(x, device)
    sc = sh = None
    if pre is not None:
        sc, sh = _dev_copy(pre[0], device), _dev_copy(pre[1], device)
    if joint:
        ld_out = 2 * C + out_pad
        out = torch.full((B, ld_out), float('nan'), device=device)
        out[:, 2 * C:] = POOL_SENTINEL
        mean_ptr, std_ptr = out.data_ptr(), out.data_ptr() + 4 * C
        assert want_std
    else:
        ld_out = C + out_pad
        out = torch.full((2, B, ld_out), float('nan'), device=device)
        out[:, :, C:] = POOL_SENTINEL
        mean_ptr, std_ptr = out[0].data_ptr(), (out[1].data_ptr() if want_std else None)
    _hip.check(cdll.mv_time_stats_ex_f16(xd.data_ptr(), ld, B, T, C, mean_ptr, std_ptr, ld_out, unbiased, eps, sc.data_ptr() if pre else None,
                                         sh.data_ptr() if pre else None, _stream(xd)), cdll)
    o = out.cpu()
    assert _same_bits(xd, x), 'time_stats wrote its input'
    if pre is not None:
        assert _same_bits(sc, pre[0]) and _same_bits(sh, pre[1])
    if joint:
        assert bool((o[:, 2 * C:] == POOL_SENTINEL).all()), 'time_stats wrote behind mean | std'
        return o[:, :C], o[:, C:2 * C]
    assert bool((o[:, :, C:] == POOL_SENTINEL).all()), 'time_stats wrote the pitch columns of its output'
    if not want_std:
        assert bool(torch.isnan(o[1, :, :C]).all()), 'std = NULL, and the buffer beside the mean was written'
        return o[0, :, :C], None
    return o[0, :, :C], o[1, :, :C]


def time_stats_check(x, C, mean, std, unbiased=0, eps=1e-12, pre=None, log=print, tag=''):
    """mean / std of time_stats_kernel against fp64, per element, under bars derived from the kernel's own summation order.

    The kernel takes the moments about k = v[b, 0, c]:  z1 = sum_t (v_t - k),  z2 = sum_t (v_t - k)^2,  mean = k + z1 / T,
    var = max(z2 - z1^2 / T, 0) / (T or T - 1), clamped from below, std = sqrt(var).  A lane adds its rows t_first, t_first + 16, ... in one chain of
    n = ceil(T / 16) fp32 additions; two shuffles add the four row groups of a wave, three additions the four LDS partials of the waves: a term passes
    through at most n + 5 additions, after the one rounding of d = v_t - k itself (two fp16 values do not always differ by an fp32 number).  With
    u = 2^-24 and gamma_m = m u / (1 - m u), S1 = sum |v_t - k| and S2 = sum (v_t - k)^2 taken from the fp64 data:
        |z1 - Z1| <= gamma_(n+6) S1 =: e1         |z2 - Z2| <= gamma_(n+7) S2 =: e2      (the square of a rounded d, then its chain)
        mean:  the division z1 / T rounds once more (gamma_(n+7) S1 / T in all), the final addition rounds the result: u |mean|
        m2 = z2 - z1^2 / T:  e2 + (2 |Z1| e1 + e1^2) / T + 2 u Z1^2 / T (product, division) + u S2 (the subtraction: |m2| <= S2)
        var:   that / denom, + 4 u var for the division, the clamp's operands and the square root (std^2 is compared: sqrt amplifies near zero)
    The pre-activation v = relu(x * scale + shift) is an fp32 value itself: eps_t = u (|x scale| + |x scale + shift|) (product and sum; fused, less)
    enters e1 as sum eps_t and e2 as sum 2 |v_t - k| eps_t; k is recomputed by the same operations, so its own error cancels.
    Bars = 2 x these bounds (the factor tests/cam_cases.py gives its bars).  max(., 0) and the clamp are contractions: they need no term.
    A channel with a NaN frame must come out NaN (mean and std), and no other may."""
    B, T, ld = x.shape
    xd = x.double()[..., :C]
    nanch = torch.isnan(xd).any(1)
    xd = torch.nan_to_num(xd, nan=0.0)
    if pre is not None:
        s64, t64 = pre[0].double(), pre[1].double()
        v = torch.relu(xd * s64 + t64)
        ev = U32 * ((xd * s64).abs() + (xd * s64 + t64).abs())
    else:
        v, ev = xd, torch.zeros_like(xd)
    d = v - v[:, :1]
    S1, Z1, S2 = d.abs().sum(1), d.sum(1), (d * d).sum(1)
    n = (T + 15) // 16
    mean_ref = v.mean(1)
    bar_mean = 2 * (_gamma(n + 7) * S1 / T + ev.sum(1) / T + U32 * mean_ref.abs())
    assert torch.equal(torch.isnan(mean), nanch), f'time_stats {tag}: the NaN means are not those of the channels with a NaN frame'
    err = (mean.double() - mean_ref).abs()
    ok = (err <= bar_mean) | nanch
    ratio = (err / bar_mean.clamp_min(1e-300))[~nanch].max().item()
    assert bool(ok.all()), f'time_stats {tag}: mean misses its bar: err {err[~ok].max().item():.3e}, ratio {ratio:.3f} at {torch.nonzero(~ok)[0].tolist()}'
    r2 = float('nan')
    if std is not None:
        denom = T - 1 if unbiased else T
        var_ref = ((v - mean_ref.unsqueeze(1)) ** 2).sum(1) / denom
        eps32 = float(np.float32(eps))
        if eps > 0:
            var_ref = var_ref.clamp_min(eps32)
        e1 = _gamma(n + 6) * S1 + ev.sum(1)
        e2 = _gamma(n + 7) * S2 + (2 * d.abs() * ev).sum(1)
        em2 = e2 + (2 * Z1.abs() * e1 + e1 * e1) / T + 2 * U32 * Z1 * Z1 / T + U32 * S2
        bar_var = 2 * (em2 / denom + 4 * U32 * var_ref)
        assert torch.equal(torch.isnan(std), nanch), f'time_stats {tag}: the NaN stds are not those of the channels with a NaN frame'
        errv = (std.double() ** 2 - var_ref).abs()
        okv = (errv <= bar_var) | nanch
        r2 = (errv / bar_var.clamp_min(1e-300))[~nanch].max().item()
        assert bool(okv.all()), f'time_stats {tag}: std^2 misses its bar: err {errv[~okv].max().item():.3e}, ratio {r2:.3f} at {torch.nonzero(~okv)[0].tolist()}'
        # a constant channel: d = 0 in every frame, the variance is exactly zero -> exactly the clamp
        const = (d == 0).all(1) & ~nanch
        want = float(np.sqrt(np.float32(eps))) if eps > 0 else 0.0
        assert bool((std[const] == want).all()), f'time_stats {tag}: a constant channel does not give exactly sqrt(clamp_eps)'
    if pre is None:
        assert bool(((mean[:, 3] == 1.25) | nanch[:, 3]).all())
    log(f'time_stats {tag}: B={B} T={T} C={C} mean err/bar {ratio:.3f}, std^2 err/bar {r2:.3f}')
    return ratio, r2


def time_stats_ex_case(cdll, device, B=2, T=49, C=264, ld=272, want_std=True, unbiased=0, eps=1e-12, seed=0, log=print):
    """one call (B small: the <PIPE> form) at a (T, C) edge"""
    x = time_stats_data(B, T, C, ld, seed)
    mean, std = time_stats_launch(cdll, device, x, C, want_std, unbiased, eps)
    return time_stats_check(x, C, mean, std, unbiased, eps, log=log, tag=f'T{T}_C{C}')


def time_stats_forms_case(cdll, device, T=33, C=136, ld=144, B_big=1025, log=print):
    """The three instantiations on the same rows: the general form (ceil(C / 128) * B_big > 1024 workgroups, std requested), <LEAN> (the same call with
    std = NULL) and <PIPE> (the first two utterances alone), each against fp64 -- and the mean of a row bit-identical across the three, as pool.hip
    promises ("same additions in the same order: the same mean").  Three channels of the large calls hold a NaN frame (utterances the <PIPE> call
    does not see): they come out NaN in both large-grid forms, every other channel meets its fp64 bar."""
    assert (C + 127) // 128 * B_big > 1024
    x = time_stats_data(B_big, T, C, ld, seed=7)
    x[7, 0, 9] = x[B_big // 2, T // 2, 3] = x[B_big - 1, T - 1, C - 1] = float('nan')
    m_gen, s_gen = time_stats_launch(cdll, device, x, C, True)
    m_lean, _ = time_stats_launch(cdll, device, x, C, False)
    m_pipe, s_pipe = time_stats_launch(cdll, device, x[:2].clone(), C, True)
    time_stats_check(x, C, m_gen, s_gen, log=log, tag='general')
    time_stats_check(x, C, m_lean, None, log=log, tag='lean')
    time_stats_check(x[:2], C, m_pipe, s_pipe, log=log, tag='pipe')
    assert _same_bits(m_gen, m_lean), 'the LEAN mean differs from the general form\'s'
    assert _same_bits(m_gen[:2], m_pipe), 'the PIPE mean differs from the general form\'s on the same rows'


def time_stats_preact_case(cdll, device, B=2, T=49, C=264, ld=272, out_pad=0, log=print):
    """the CAM++ StatsPool call: pre-activation relu(x * scale + shift) with scales of both signs, unbiased std without a clamp, mean | std in one row
    of pitch 2C (+ out_pad columns that keep their sentinel).  Channel 5 is zeroed by the ReLU in every frame: mean and variance exactly 0."""
    x = time_stats_data(B, T, C, ld, seed=3)
    g = torch.Generator().manual_seed(11)
    sc = torch.randn(C, generator=g) * 1.5
    sc[::2] = sc[::2].abs() + 0.1
    sc[1::2] = -sc[1::2].abs() - 0.1
    sh = torch.randn(C, generator=g)
    sc[5], sh[5] = 1.0, -1000.0
    mean, std = time_stats_launch(cdll, device, x, C, True, 1, 0.0, pre=(sc, sh), out_pad=out_pad, joint=True)
    assert bool((mean[:, 5] == 0).all()) and bool((std[:, 5] == 0).all()), 'a channel the ReLU zeroes in every frame must have mean and variance exactly 0'
    return time_stats_check(x, C, mean, std, 1, 0.0, pre=(sc, sh), log=log, tag=f'preact_pad{out_pad}')


def time_stats_nan_case(cdll, device, B=2, T=49, C=264, ld=272, pre=False, B_big=0):
    """a NaN frame makes that channel's mean and std NaN; every other output has the bits it has without the NaN.  B_big: the general and LEAN forms"""
    B = B_big or B
    x = time_stats_data(B, T, C, ld, seed=5)
    p = None
    if pre:
        g = torch.Generator().manual_seed(12)
        p = (torch.randn(C, generator=g), torch.randn(C, generator=g))
    xn = x.clone()
    hits = [(0, 0, 9), (B - 1, T - 1, C - 1), (B - 1, T // 2, 3)]      # the first frame (k itself), the last frame of the last (scalar-path) channel, the constant channel
    for b, t, c in hits:
        xn[b, t, c] = float('nan')
    for want_std in ((True, False) if B_big else (True,)):
        kw = dict(want_std=want_std, unbiased=1 if pre else 0, eps=0.0 if pre else 1e-12, pre=p)
        m0, s0 = time_stats_launch(cdll, device, x, C, **kw)
        m1, s1 = time_stats_launch(cdll, device, xn, C, **kw)
        mask = torch.zeros(B, C, dtype=torch.bool)
        for b, _, c in hits:
            mask[b, c] = True
        for a0, a1, what in ((m0, m1, 'mean'), (s0, s1, 'std')):
            if a1 is None:
                continue
            assert bool(torch.isnan(a1[mask]).all()), f'time_stats: a NaN frame left a finite {what}: {a1[mask].tolist()}'
            assert _same_bits(a0[~mask], a1[~mask]), f'time_stats: a NaN frame changed the {what} of another channel'


def time_stats_batch_rows_case(cdll, device, T=49, C=264, ld=272):
    x = time_stats_data(5, T, C, ld, seed=0)
    m5, s5 = time_stats_launch(cdll, device, x, C)
    m1, s1 = time_stats_launch(cdll, device, x[:1].clone(), C)
    assert _same_bits(m5[:1], m1) and _same_bits(s5[:1], s1)


def time_stats_refusal_case(cdll, device):
    """unbiased with T = 1, ld_out < C, a misaligned x: refused with a message, nothing launched"""
    x = _dev_copy(time_stats_data(2, 3, 16, 24), device)
    out = torch.full((2, 2, 16), float('nan'), device=device)
    f = cdll.mv_time_stats_ex_f16
    msgs = [_raises(lambda: f(x.data_ptr(), 24, 6, 1, 16, out[0].data_ptr(), out[1].data_ptr(), 16, 1, 0.0, None, None, _stream(x)), cdll),
            _raises(lambda: f(x.data_ptr(), 24, 2, 3, 16, out[0].data_ptr(), out[1].data_ptr(), 15, 0, 0.0, None, None, _stream(x)), cdll),
            _raises(lambda: f(x.data_ptr() + 2, 24, 1, 3, 16, out[0].data_ptr(), out[1].data_ptr(), 16, 0, 0.0, None, None, _stream(x)), cdll)]
    assert bool(torch.isnan(out.cpu()).all()), 'a refused call wrote its output'
    return msgs


# ---- seg_mean

def seg_mean_data(B, T, C, seed=0):
    ld = C + 8
    x = torch.empty(B, T, ld, dtype=torch.float16)
    for b in range(B):   # utterance by utterance: row 0 of a B = 5 call is row 0 of a B = 1 call
        x[b] = (torch.randn(T, ld, generator=torch.Generator().manual_seed(3000 + 17 * seed + b)) * 1.5 + 0.7).half()
    x[..., C:] = POOL_SENTINEL
    return x


def seg_mean_launch(cdll, device, x, C, seg_len):
    B, T, ld = x.shape
    nseg = (T + seg_len - 1) // seg_len
    xd = _dev_copy(x, device)
    ctx = torch.full((B * nseg * C + 8,), float('nan'), device=device)
    ctx[-8:] = POOL_SENTINEL
    _hip.check(cdll.mv_seg_mean_f16(xd.data_ptr(), ld, B, T, C, seg_len, ctx.data_ptr(), _stream(xd)), cdll)
    o = ctx.cpu()
    assert _same_bits(xd, x), 'seg_mean wrote its input'
    assert bool((o[-8:] == POOL_SENTINEL).all()), 'seg_mean wrote behind its output'
    return o[:-8].view(B, nseg, C)


def seg_mean_case(cdll, device, T=101, seg_len=100, C=136, B=3, log=print):
    """ctx[b, s, c] = mean over T + mean over segment s, the last segment divided by its own length, against fp64.

    Bar, from seg_mean_kernel's order: a segment of L frames is summed by 16 row phases, each a chain of ceil(L / 16) fp32 additions, then the 16 LDS
    partials in one chain of 15 more, then one division: gamma_(ceil(L/16)+16) sum_seg |x| / L.  The utterance total adds the nseg segment sums (nseg
    more) and is divided by T: gamma_(ceil(seg_len/16)+16+nseg) sum |x| / T.  Their sum rounds once: u |ctx|.  Bar = 2 x the bound."""
    x = seg_mean_data(B, T, C)
    ctx = seg_mean_launch(cdll, device, x, C, seg_len)
    xd = x.double()[..., :C]
    nseg = ctx.shape[1]
    gm = xd.mean(1)
    n_all = (min(seg_len, T) + 15) // 16 + 16 + nseg
    bar_gm = _gamma(n_all) * xd.abs().sum(1) / T
    ratio = 0.0
    for s in range(nseg):
        seg = xd[:, s * seg_len:min((s + 1) * seg_len, T)]
        L = seg.shape[1]
        ref = gm + seg.mean(1)
        bar = 2 * (bar_gm + _gamma((L + 15) // 16 + 16) * seg.abs().sum(1) / L + U32 * ref.abs())
        err = (ctx[:, s].double() - ref).abs()
        ratio = max(ratio, (err / bar).max().item())
        assert bool((err <= bar).all()), f'seg_mean T={T} seg_len={seg_len} C={C}: segment {s} misses its bar, err {err.max().item():.3e}, err/bar {(err / bar).max().item():.3f}'
    log(f'seg_mean T={T} seg_len={seg_len} C={C}: err/bar {ratio:.3f}')
    return ratio


def seg_mean_nan_case(cdll, device, T=30, seg_len=7, C=136, B=3):
    x = seg_mean_data(B, T, C, seed=1)
    xn = x.clone()
    xn[1, T - 1, C - 1] = float('nan')     # the last frame of the ragged last segment
    xn[0, 0, 0] = float('nan')
    c0, c1 = seg_mean_launch(cdll, device, x, C, seg_len), seg_mean_launch(cdll, device, xn, C, seg_len)
    mask = torch.zeros_like(c0, dtype=torch.bool)
    mask[1, :, C - 1] = True               # every segment: the utterance mean is part of each
    mask[0, :, 0] = True
    assert bool(torch.isnan(c1[mask]).all()), 'seg_mean: a NaN frame left a finite context'
    assert _same_bits(c0[~mask], c1[~mask]), 'seg_mean: a NaN frame changed another channel'


def seg_mean_batch_rows_case(cdll, device, T=101, seg_len=100, C=136):
    x = seg_mean_data(5, T, C)
    assert _same_bits(seg_mean_launch(cdll, device, x, C, seg_len)[:1], seg_mean_launch(cdll, device, x[:1].clone(), C, seg_len))


# ---- se_gate_residual

def se_gate_launch(cdll, device, y, gate, cat, res_col, out_col, res_own, T, C):
    """out = gate * y + res.  cat: the buffer `out` is a column slice of (at out_col); res: the slice at res_col of the same buffer, or res_own."""
    n, ldy = y.shape
    B = n // T
    yd, gd, cd = _dev_copy(y, device), _dev_copy(gate, device), _dev_copy(cat, device)
    rd = _dev_copy(res_own, device) if res_own is not None else None
    res_ptr, ldr = (rd.data_ptr(), rd.shape[1]) if rd is not None else (cd.data_ptr() + 2 * res_col, cd.shape[1])
    _hip.check(cdll.mv_se_gate_residual_f16(yd.data_ptr(), ldy, gd.data_ptr(), res_ptr, ldr, cd.data_ptr() + 2 * out_col, cd.shape[1], B, T, C, _stream(yd)), cdll)
    o = cd.cpu()
    assert _same_bits(yd, y) and _same_bits(gd, gate), 'se_gate_residual wrote an input'
    if rd is not None:
        assert _same_bits(rd, res_own), 'se_gate_residual wrote its residual'
    keep = torch.ones(cat.shape[1], dtype=torch.bool)
    keep[out_col:out_col + C] = False
    assert _same_bits(o[:, keep], cat[:, keep]), 'se_gate_residual wrote outside its output slice'
    return o[:, out_col:out_col + C]


def se_gate_data(B, T, C, ldy, own, seed=0):
    n = B * T
    rows = lambda b, w, s: torch.cat([torch.randn(T, w, generator=torch.Generator().manual_seed(4000 + 31 * seed + 7 * bb + s)) for bb in range(b)])
    y = (rows(B, ldy, 0) * 2).half()
    y[:, C:] = POOL_SENTINEL
    gate = torch.cat([torch.rand(1, C, generator=torch.Generator().manual_seed(4500 + 31 * seed + b)) for b in range(B)])   # sigmoid outputs, each utterance its own
    res = (rows(B, C, 1) * 2).half()
    if T * C >= 3:      # planted in utterance 0, row 0: beyond +65504 and below -65504 (stored saturated), and g * y cancelling r to the last bits
        y[0, 0], gate[0, 0], res[0, 0] = 30000.0, 2.0, 30000.0
        y[0, 1], gate[0, 1], res[0, 1] = -30000.0, 2.0, -30000.0
        y[0, 2], gate[0, 2], res[0, 2] = 3.0, 1.0 / 3.0, -1.0
    if own:     # the residual in a buffer of its own (pitch C + 16), out at column 8 of a buffer of pitch C + 16
        res_own = torch.full((n, C + 16), POOL_SENTINEL, dtype=torch.float16)
        res_own[:, :C] = res
        cat = torch.full((n, C + 16), POOL_SENTINEL, dtype=torch.float16)
        res_col, out_col = None, 8
    else:       # res and out: disjoint column slices of one buffer (pitch 2C + 16: res at column 8, out at column C + 8), as in the model's concat buffer
        res_own = None
        cat = torch.full((n, 2 * C + 16), POOL_SENTINEL, dtype=torch.float16)
        res_col, out_col = 8, C + 8
        cat[:, 8:8 + C] = res
    cat[:, out_col:out_col + C] = float('nan')
    return y, gate, res, cat, res_col, out_col, res_own


def se_gate_residual_case(cdll, device, B=3, T=7, C=72, ldy=80, own=False, log=print):
    """Bar per element, as bn_relu_rows_case: half an fp16 ulp of the exact value (x 1.001, which also covers the fp32 rounding of the sum; subnormals
    2^-25) + one fp32 rounding of the product g * y (the device fuses the multiply-add, the host build of the emulator need not: visible where g * y
    and r cancel)."""
    y, gate, res, cat, res_col, out_col, res_own = se_gate_data(B, T, C, ldy, own)
    out = se_gate_launch(cdll, device, y, gate, cat, res_col, out_col, res_own, T, C)
    g = gate.double().repeat_interleave(T, 0)
    prod = g * y.double()[:, :C]
    ref = (prod + res.double()).clamp(-65504.0, 65504.0)
    err = (out.double() - ref).abs()
    tol = ref.abs() * 2.0 ** -11 * 1.001 + 2.0 ** -25 + prod.abs() * U32
    assert not bool(torch.isnan(out).any()), 'se_gate_residual left an element unwritten'
    ratio = (err / tol).max().item()
    assert bool((err <= tol).all()), f'se_gate_residual: err/bar {ratio:.3f}'
    assert out[0, 0] == 65504.0 and out[0, 1] == -65504.0
    log(f'se_gate_residual B={B} T={T} C={C} {"own" if own else "slices"}: err/bar {ratio:.3f}')
    return ratio


def se_gate_nan_case(cdll, device, where, B=3, T=7, C=72, ldy=80):
    y, gate, res, cat, res_col, out_col, res_own = se_gate_data(B, T, C, ldy, False, seed=1)
    out0 = se_gate_launch(cdll, device, y, gate, cat, res_col, out_col, res_own, T, C)
    mask = torch.zeros(B * T, C, dtype=torch.bool)
    r, c = T + 2, C - 3                     # utterance 1
    if where == 'y':
        y = y.clone(); y[r, c] = float('nan'); mask[r, c] = True
    elif where == 'res':
        cat = cat.clone(); cat[r, res_col + c] = float('nan'); mask[r, c] = True
    else:
        gate = gate.clone(); gate[1, c] = float('nan'); mask[T:2 * T, c] = True
    out1 = se_gate_launch(cdll, device, y, gate, cat, res_col, out_col, res_own, T, C)
    assert bool(torch.isnan(out1[mask]).all()), f'se_gate_residual: a NaN in {where} came out finite: {out1[mask].tolist()}'
    assert _same_bits(out0[~mask], out1[~mask])


def se_gate_batch_rows_case(cdll, device, T=7, C=72, ldy=80):
    y, gate, res, cat, res_col, out_col, _ = se_gate_data(5, T, C, ldy, False)
    o5 = se_gate_launch(cdll, device, y, gate, cat, res_col, out_col, None, T, C)
    o1 = se_gate_launch(cdll, device, y[:T].clone(), gate[:1].clone(), cat[:T].clone(), res_col, out_col, None, T, C)
    assert _same_bits(o5[:T], o1)


# ---- asp_hidden_act

def asp_hidden_data(B, T, A, seed=0):
    g = torch.Generator().manual_seed(5000 + seed)
    z = (torch.randn(B * T, A, generator=g) * 1.5).half()
    z[0, 0], z[1, 1], z[2, 2], z[3, 3] = 30.0, -30.0, 100.0, 45.0       # tanhf where the value has saturated to +-1 (scale[0 .. 3] = +-1 below)
    rb = torch.randn(B, A, generator=g) + torch.arange(B).float().unsqueeze(1) * 1.5 - 1.0     # the utterances' biases 1.5 apart: a wrong b is far outside the bar
    sc = torch.randn(A, generator=g) * 1.5
    sh = torch.randn(A, generator=g) * 0.5
    sc[0], sc[1], sc[2], sc[3] = 1.0, 1.0, -1.0, 0.8
    return z, rb, sc, sh


def asp_hidden_launch(cdll, device, z, rb, sc, sh, B, T, A):
    buf = torch.full((B * T * A + 8,), POOL_SENTINEL, dtype=torch.float16)
    buf[:-8] = z.reshape(-1)
    bd, rd, sd, td = _dev_copy(buf, device), _dev_copy(rb, device), _dev_copy(sc, device), _dev_copy(sh, device)
    _hip.check(cdll.mv_asp_hidden_act_f16(bd.data_ptr(), rd.data_ptr(), sd.data_ptr(), td.data_ptr(), B, T, A, _stream(bd)), cdll)
    o = bd.cpu()
    assert _same_bits(rd, rb) and _same_bits(sd, sc) and _same_bits(td, sh), 'asp_hidden_act wrote a parameter'
    assert bool((o[-8:] == POOL_SENTINEL).all()), 'asp_hidden_act wrote behind its rows'
    return o[:-8].view(B * T, A)


def asp_hidden_act_case(cdll, device, B=3, T=5, A=136, log=print):
    """h = tanh(relu(z + rb[b]) * scale + shift) in place, against fp64.  Bar per element: half an fp16 ulp of the exact value x 1.001 (subnormals 2^-25;
    the 0.001 covers tanhf's own ulp or two of fp32 and the rounding of the last addition, whose effect on h is at most u |a| tanh'(a) <= u |h|) + the
    fp32 term of p = relu(z + rb) * scale: the sum z + rb and the product round once each, 2 u |p|, and reach h multiplied by tanh' <= 1."""
    z, rb, sc, sh = asp_hidden_data(B, T, A)
    out = asp_hidden_launch(cdll, device, z, rb, sc, sh, B, T, A)
    p = torch.relu(z.double() + rb.double().repeat_interleave(T, 0)) * sc.double()
    ref = torch.tanh(p + sh.double())
    err = (out.double() - ref).abs()
    tol = ref.abs() * 2.0 ** -11 * 1.001 + 2.0 ** -25 + 2 * U32 * p.abs()
    ratio = (err / tol).max().item()
    assert bool((err <= tol).all()), f'asp_hidden_act A={A}: err/bar {ratio:.3f} at {torch.nonzero(err > tol)[0].tolist()}'
    assert (ref.abs() > 0.9999).sum() >= 3          # the saturated plants are there
    log(f'asp_hidden_act B={B} T={T} A={A}: err/bar {ratio:.3f}')
    return ratio


def asp_hidden_nan_case(cdll, device, B=3, T=5, A=136):
    z, rb, sc, sh = asp_hidden_data(B, T, A, seed=1)
    out0 = asp_hidden_launch(cdll, device, z, rb, sc, sh, B, T, A)
    zn = z.clone()
    zn[T + 1, A - 1] = float('nan')
    rbn = rb.clone()
    rbn[2, 4] = float('nan')
    out1 = asp_hidden_launch(cdll, device, zn, rbn, sc, sh, B, T, A)
    mask = torch.zeros(B * T, A, dtype=torch.bool)
    mask[T + 1, A - 1] = True
    mask[2 * T:3 * T, 4] = True
    assert bool(torch.isnan(out1[mask]).all()), f'asp_hidden_act: a NaN came out finite: {out1[mask].tolist()}'
    assert _same_bits(out0[~mask], out1[~mask])


# ---- the casts and copies: bitwise against numpy

def pool_features(B, T, F, seed):
    """as _features of tests/test_feature_dims.py: values beyond the fp16 range on either side, and 65519 (rounds to inf in fp16 without the clamp)"""
    x = torch.randn(B, T, F, generator=torch.Generator().manual_seed(seed)) * 3
    x[0, 0, 0], x[-1, -1, -1] = 1.0e6, -7.0e4
    if F > 2:
        x[0, 1, 2] = 65519.0
    return x


def _equal_f16(got, want):
    """bitwise, a NaN matching any NaN"""
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(got.view(np.uint16)[~gn], want.view(np.uint16)[~wn])


def cast_pad_case(cdll, device, F=13, pad=2, B=2, T=9, nan=False):
    """mv_cast_pad_f16 (the choice EcapaModel::forward makes: the 16-byte kernel for ldd == F, the ragged one otherwise) against np.pad(mode='reflect'),
    clip(+-65504), astype(float16); columns F .. ldd-1 are +0"""
    ldd = (F + 7) // 8 * 8
    x = pool_features(B, T, F, F + pad)
    if nan:
        x[0, 0, 1 % F], x[1, T - 1, F - 1], x[1, T // 2, 0] = float('nan'), float('nan'), float('nan')   # the first and last frames are mirrored into the padding
    Tp = T + 2 * pad
    xd = _dev_copy(x, device)
    out = torch.full((B * Tp * ldd + 8,), float('nan'), dtype=torch.float16, device=device)
    out[-8:] = POOL_SENTINEL
    _hip.check(cdll.mv_cast_pad_f16(xd.data_ptr(), out.data_ptr(), B, T, F, ldd, pad, _stream(xd)), cdll)
    o = out.cpu()
    assert _same_bits(xd, x) and bool((o[-8:] == POOL_SENTINEL).all())
    want = np.zeros((B, Tp, ldd), np.float16)
    xp = np.pad(x.numpy(), ((0, 0), (pad, pad), (0, 0)), mode='reflect')
    want[:, :, :F] = np.clip(xp, -65504.0, 65504.0).astype(np.float16)
    got = o[:-8].view(B, Tp, ldd).numpy()
    if nan:
        assert np.isnan(want).sum() >= 3
    assert _equal_f16(got, want), np.argwhere(got.view(np.uint16) != want.view(np.uint16))[:4]


def cast_rows_case(cdll, device, C=13, ldd=16, n=37, nan=False):
    lds = C + 3
    x = torch.full((n, lds), POOL_SENTINEL)
    x[:, :C] = pool_features(1, n, C, C)[0]
    if nan:
        x[0, 0], x[n - 1, C - 1] = float('nan'), float('nan')
    xd = _dev_copy(x, device)
    out = torch.full((n * ldd + 8,), float('nan'), dtype=torch.float16, device=device)
    out[-8:] = POOL_SENTINEL
    _hip.check(cdll.mv_cast_rows_f16(xd.data_ptr(), lds, out.data_ptr(), ldd, n, C, _stream(xd)), cdll)
    o = out.cpu()
    assert _same_bits(xd, x) and bool((o[-8:] == POOL_SENTINEL).all())
    want = np.zeros((n, ldd), np.float16)      # columns C .. ldd-1: +0
    want[:, :C] = np.clip(x.numpy()[:, :C], -65504.0, 65504.0).astype(np.float16)
    assert _equal_f16(o[:-8].view(n, ldd).numpy(), want)


def copy_slice_case(cdll, device, C=64, lds=512, ldd=520, n=37, src_col=128, dst_col=8):
    g = torch.Generator().manual_seed(6000)
    src = (torch.randn(n, lds, generator=g) * 3).half()
    src[0, src_col], src[1, src_col + 1], src[2, src_col + C - 1] = float('inf'), float('nan'), 6.0e-8    # a copy keeps everything: inf, NaN, subnormals
    dst = torch.full((n, ldd), POOL_SENTINEL, dtype=torch.float16)
    dst[:, dst_col:dst_col + C] = float('nan')
    dst[:, dst_col:dst_col + C].view(torch.int16).fill_(0x7e55)          # (a NaN with a payload of its own: the copied NaN must not be taken for it)
    sd, dd = _dev_copy(src, device), _dev_copy(dst, device)
    _hip.check(cdll.mv_copy_slice_f16(sd.data_ptr() + 2 * src_col, lds, dd.data_ptr() + 2 * dst_col, ldd, C, n, _stream(sd)), cdll)
    o = dd.cpu()
    want = dst.clone()
    want[:, dst_col:dst_col + C] = src[:, src_col:src_col + C]
    assert _same_bits(sd, src) and _same_bits(o, want)


def pad_rows_f32_case(cdll, device, F=13, ldd=16, n=37):
    x = pool_features(1, n, F, F)[0].contiguous()
    x[3, 0] = float('inf')
    xd = _dev_copy(x, device)
    out = torch.full((n * ldd + 4,), float('nan'), device=device)
    out[-4:] = POOL_SENTINEL
    _hip.check(cdll.mv_pad_rows_f32(xd.data_ptr(), F, out.data_ptr(), ldd, n, _stream(xd)), cdll)
    o = out.cpu()
    want = torch.zeros(n, ldd)
    want[:, :F] = x                                       # an exact copy: no clamp, the first conv converts to fp16 itself
    assert _same_bits(xd, x) and bool((o[-4:] == POOL_SENTINEL).all())
    assert _same_bits(o[:-4].view(n, ldd), want)


def bn_relu_rows_nan_case(cdll, device, rows=9, C=72, ldx=80, ldy=88):
    """relu(NaN * scale + shift) is NaN (torch.relu keeps it); every other element keeps its bits"""
    g = torch.Generator().manual_seed(21)
    x = (torch.randn(rows, ldx, generator=g) * 3).half()
    sc, sh = torch.randn(C, generator=g) * 2, torch.randn(C, generator=g)
    xn = x.clone()
    xn[4, C - 1] = float('nan')
    scn = sc.clone()
    scn[7] = float('nan')
    outs = []
    for xx, ss in ((x, sc), (xn, scn)):
        xd, sd, td = _dev_copy(xx, device), _dev_copy(ss, device), _dev_copy(sh, device)
        y = torch.full((rows, ldy), -7.0, dtype=torch.half, device=device)
        _hip.check(cdll.mv_bn_relu_rows_f16(xd.data_ptr(), ldx, sd.data_ptr(), td.data_ptr(), y.data_ptr(), ldy, rows, C, _stream(xd)), cdll)
        outs.append(y.cpu())
    mask = torch.zeros(rows, ldy, dtype=torch.bool)
    mask[4, C - 1] = True
    mask[:, 7] = True
    assert bool(torch.isnan(outs[1][mask]).all()), f'bn_relu_rows: a NaN came out finite: {outs[1][mask].tolist()}'
    assert _same_bits(outs[0][~mask], outs[1][~mask])
