"""Shared checks of EcapaTdnn with grouped TDNN convolutions and other SE-Res2Net block counts (mv_ecapa_create_ex) and of the grouped
conv1d layer (mv_conv1d_forward_grouped): used by tests/test_ecapa_variants.py (SIMT emulator) and tests/test_gpu_ecapa_variants.py (MI355X)."""
import ctypes

import torch
import torch.nn.functional as F

from mvector import _hip

# the fixtures of tools/make_ecapa_variant_golden.py
GOLDENS = ['ecapa_grouped_tiny', 'ecapa_blocks4_tiny', 'ecapa_blocks1_tiny', 'ecapa_grouped_sap_tiny', 'ecapa_grouped_c1024']


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream if t.is_cuda else None


def _sync(device):
    if str(device) != 'cpu':
        torch.cuda.synchronize()


def pack_grouped(cdll, w, groups):
    """grouped nn.Conv1d weight [cout, cin / g, k] (on the target device) -> the packed fp16 operand of mv_conv1d_forward_grouped"""
    cout, cin_g, k = w.shape
    cin = cin_g * groups
    n = cdll.mv_conv1d_grouped_packed_elems(cout, cin, k, groups)
    assert n > 0
    out = torch.empty(int(n), dtype=torch.float16, device=w.device)
    _hip.check(cdll.mv_conv1d_pack_weight_grouped(w.contiguous().data_ptr(), cout, cin, k, groups, out.data_ptr(), _stream(w)), cdll)
    return out


def desc(x, ldx, packed, bias, scale, shift, y, ldy, B, T, cin, cout, k=1, dil=1, tile=0, persist_blocks=0):
    """MvConv1dDesc of a TDNNBlock layer (conv -> ReLU -> BatchNorm affine, reflect 'same' padding) over fp16 x [B, T, ldx] -> fp16 y"""
    d = _hip.MvConv1dDesc()
    d.x, d.x_dtype, d.ldx = x.data_ptr(), _hip.MV_DT_F16, ldx
    d.w_packed, d.bias, d.scale, d.shift = packed.data_ptr(), bias.data_ptr(), scale.data_ptr(), shift.data_ptr()
    d.pre_act, d.post_act = _hip.MV_ACT_RELU, _hip.MV_ACT_NONE
    d.y, d.y_dtype, d.ldy = y.data_ptr(), _hip.MV_DT_F16, ldy
    d.B, d.T_in, d.T_out, d.cin, d.cout, d.k = B, T, T, cin, cout, k
    d.dilation, d.stride, d.pad, d.pad_mode = dil, 1, dil * (k - 1) // 2, _hip.MV_PAD_REFLECT
    d.tile, d.persist_blocks_hint = tile, persist_blocks
    return d


def grouped_conv_case(cdll, device, B, T, cin, cout, groups, k=1, dil=1, tile=0, persist_blocks=0, seed=0, extra_ld=8, bound=False,
                      expect_kernel=None, plan_cus=None, log=None):
    """A grouped TDNNBlock layer through mv_conv1d_forward_grouped against F.conv1d(groups=g) on the fp16-rounded operands.  A native layer
    must also give, bit for bit, the g dense layers over the groups' slices of x (every output element: bias + the same K sum in the same
    order).  Returns whether the layer ran native.
    expect_kernel: the row of conv1d's kernel table the layer must plan to on this device (mv_conv1d_plan_info), asserted before the launch.
    bound: also hold every element to the per-element bound of tests/conv1d_cases.py against fp64 (k = 1).
    plan_cus: launch nothing; return the plan info of the layer's descriptor on a chip of that many compute units."""
    g = torch.Generator().manual_seed(seed)
    cin_g, cout_g = cin // groups, cout // groups
    ldx, ldy = cin + extra_ld, cout + extra_ld
    x = torch.randn(B, T, ldx, generator=g).half()
    w = torch.randn(cout, cin_g, k, generator=g) * (2.0 / (cin_g * k)) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1
    scale = torch.rand(cout, generator=g) + 0.5
    shift = torch.randn(cout, generator=g) * 0.1
    xd, wd, bd, sd, td = (t.to(device).contiguous() for t in (x, w, bias, scale, shift))
    y = torch.full((B, T, ldy), 7.0, dtype=torch.float16, device=device)
    native = bool(cdll.mv_conv1d_grouped_native(cout, cin, k, groups))
    packed = pack_grouped(cdll, wd, groups)
    d = desc(xd, ldx, packed, bd, sd, td, y, ldy, B, T, cin, cout, k, dil, tile, persist_blocks)
    if plan_cus is not None:
        return _hip.conv1d_plan_info(d, groups, plan_cus, cdll)
    plan = _hip.conv1d_plan_info(d, groups, 0, cdll)
    if expect_kernel is not None:
        assert plan['kernel'] == expect_kernel, plan
    _hip.check(cdll.mv_conv1d_forward_grouped(ctypes.byref(d), groups, _stream(xd)), cdll)
    _sync(device)
    got = y.cpu()
    assert torch.all(got[..., cout:] == 7.0), 'wrote beyond cout'
    if k == 1:   # per group as a matmul on the device (fp64): the full-size layers of the GPU tests
        xg = xd[..., :cin].double().reshape(B * T, groups, cin_g).transpose(0, 1)                # [g, rows, cin_g]
        ref = torch.bmm(xg, wd.half().double().reshape(groups, cout_g, cin_g).transpose(1, 2))   # [g, rows, cout_g]
        ref = ref.transpose(0, 1).reshape(B, T, cout).cpu() + bias.double()
        if bound:   # S = sum |x| |w| + |bias| by the same product on absolute values; the epilogue and the bound are conv1d_cases.bound's
            import conv1d_cases
            S = torch.bmm(xg.abs(), wd.half().double().abs().reshape(groups, cout_g, cin_g).transpose(1, 2))
            S = S.transpose(0, 1).reshape(B, T, cout).cpu() + bias.double().abs()
            ref64, bnd = conv1d_cases.bound(ref, S, cin_g * k, _hip.MV_ACT_RELU, scale, shift, _hip.MV_ACT_NONE, None, False)
            conv1d_cases.assert_ratio(got[..., :cout], ref64, bnd, plan['kernel'], f'grouped g={groups} {cin}->{cout}', log)
    else:
        assert not bound, 'the per-element bound is wired for k = 1'
        pad = dil * (k - 1) // 2
        xin = F.pad(x[..., :cin].double().transpose(1, 2), (pad, pad), mode='reflect')
        ref = F.conv1d(xin, w.half().double(), bias.double(), dilation=dil, groups=groups).transpose(1, 2)
    ref = torch.relu(ref) * scale.double() + shift.double()
    out = got[..., :cout].double()
    assert torch.isfinite(out).all()
    rel = ((out - ref).abs() / (ref.abs() + 0.05)).max().item()
    assert rel < 4e-3, rel
    if native:
        y2 = torch.full((B, T, ldy), 7.0, dtype=torch.float16, device=device)
        for gi in range(groups):
            sl = slice(gi * cout_g, (gi + 1) * cout_g)
            pk = pack_grouped(cdll, wd[sl].contiguous(), 1)
            b_, s_, t_ = bd[sl].contiguous(), sd[sl].contiguous(), td[sl].contiguous()
            d2 = desc(xd, ldx, pk, b_, s_, t_, y2, ldy, B, T, cin_g, cout_g, k, dil)
            d2.x = xd.data_ptr() + 2 * gi * cin_g
            d2.y = y2.data_ptr() + 2 * gi * cout_g
            _hip.check(cdll.mv_conv1d_forward(ctypes.byref(d2), _stream(xd)), cdll)
            _sync(device)
        assert torch.equal(y2.cpu()[..., :cout], got[..., :cout]), 'the grouped GEMM differs from its groups run one by one'
    return native


def module_and_weights(kwargs, seed):
    import mvector.models as M
    from oracle import weights
    m = M.EcapaTdnn(**kwargs)
    sd = weights.make_state_dict(weights.shapes_of(m.state_dict()), seed)
    m.load_state_dict(sd)
    return m.eval(), sd


def golden_module(man, sd):
    import mvector.models as M
    m = M.EcapaTdnn(**man['kwargs'])
    m.load_state_dict(sd)
    return m.eval()


def handle(m, sd, cdll=None, device='cpu'):
    return _hip.Model('ecapa', m._native_cfg(), {k: v.to(device) for k, v in sd.items()}, cdll=cdll,
                      pooling_type=m._native_pooling_type())


def info(h):
    """(grouped layers on the grouped GEMM, expanded grouped layers, expanded 1x1 ones, SE-Res2Net blocks)"""
    return tuple(int(h.info(k)) for k in (_hip.MV_INFO_ECAPA_GROUPED_NATIVE, _hip.MV_INFO_ECAPA_GROUPED_EXPANDED, _hip.MV_INFO_ECAPA_EXPANDED_1X1,
                                          _hip.MV_INFO_ECAPA_BLOCKS))
