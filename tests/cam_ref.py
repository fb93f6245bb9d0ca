"""Plain reference of one CAMDenseTDNNLayer (mvector/models/campplus.py:94-150, `_dense_layer_forward`), channel-last, in torch.float64 -- and
the rounding model of the three device forms (csrc/camblock.hip, csrc/camdense.hip).

    a    = ReLU(BN1(x))                                  x [B, T2, cin], BatchNorm folded to scale / shift
    h    = ReLU(BN2(W1 . a))                             1x1 conv, bottleneck 128
    ctx  = mean_T(h) + mean over the frame's seg_len-frame segment (the LAST segment over its true length: avg_pool1d ceil_mode)
    gate = sigmoid(Wb . ReLU(Wa . ctx + ba) + bb)        per segment
    y    = conv_k3,dil(h, zero padding) * gate           32 new channels

The weights are taken as the kernel sees them (w1 / wl already rounded to fp16, everything else fp32).  With fp16_sites=True (and dtype=float32)
the evaluation rounds to fp16 exactly where the kernels store or feed fp16 -- read off the sources:
  * BN1 + ReLU in place in the LDS stage: fp32 FMA of the fp16 input (one rounding), ReLU, one rounding to fp16
    (camdense.hip transform(), camblock.hip cell_math(): ReLU before or after the rounding gives the same bits);
  * h: fp32 MFMA accumulators, fp32 FMA with the BN2 scale / shift, clamp to [0, 65504], one rounding to fp16 into LDS (the long form: into LDS
    and from there to the global h buffer, the same bits); the k = 3 conv reads the fp16 h;
  * y: fp32 accumulators times the fp32 gate, clamp to +-65504 (the fp16 range: it saturates, it never overflows), one rounding to fp16.
The context sums differ BETWEEN the forms (ctx_from):
  * 'fp32'  cam_dense_block_kernel takes the column sums from the epilogue's registers, i.e. from the clamped fp32 h BEFORE its rounding to fp16
            (camblock.hip, "the fp32 value: the reference's context is the mean of an unrounded h");
  * 'fp16'  cam_dense_layer_kernel and the long form sum the ROUNDED h they read back from LDS (camdense.hip phase B / the gemm kernel's tail).
Context FCs, sigmoid and gate are fp32 in every form.

`wrong` evaluates a deliberately WRONG layer (tests/cam_cases.py: the bars of a case must be able to see the bug the case is named after)."""
import torch

F16_MAX = 65504.0
CTX_FROM = {1: 'fp32', 2: 'fp16', 3: 'fp16'}   # launch form -> where its context sums come from

WRONG = ('last_seg_len',    # last-segment mean divided by seg_len instead of its true length
         'gate_seg0',       # segment 0's gate used on segment 1
         'tap_plus',        # the +dil tap of the last dil rows read as the row itself instead of zero
         'tap_minus',       # the -dil tap of the first dil rows likewise
         'time_mean_160')   # the time mean taken over 160 rows instead of T2


def _r16(v):
    return v.clamp(-F16_MAX, F16_MAX).half().to(v.dtype)


def dense_layer(x, p, dil, seg_len, dtype=torch.float64, fp16_sites=False, ctx_from='fp16', wrong=None, return_gate=False):
    """x [B, T2, cin] (the fp16 values of the concat buffer), p: dict of w1 [128, cin], bn1_s, bn1_t [cin], bn2_s, bn2_t [128], wl [32, 128, 3],
    wa [64, 128], ba [64], wb [32, 64], bb [32] -> y [B, T2, 32] in `dtype` (fp16-representable when fp16_sites)."""
    assert wrong is None or wrong in WRONG, wrong
    B, T2, cin = x.shape
    q = {k: v.to(dtype) for k, v in p.items()}
    if fp16_sites:   # one rounding of x * s + t, as the kernel's FMA (fp64 holds the product exactly)
        a = torch.relu((x.double() * p['bn1_s'].double() + p['bn1_t'].double()).to(dtype))
        a = _r16(a)
    else:
        a = torch.relu(x.to(dtype) * q['bn1_s'] + q['bn1_t'])
    h = torch.relu((a @ q['w1'].t()) * q['bn2_s'] + q['bn2_t']).clamp(max=F16_MAX)
    h16 = _r16(h) if fp16_sites else h
    hs = h if (ctx_from == 'fp32' or not fp16_sites) else h16
    nseg = -(-T2 // seg_len)
    total = hs.sum(1) / (160.0 if wrong == 'time_mean_160' else float(T2))
    gates = []
    for sg in range(nseg):
        lo, hi = sg * seg_len, min(T2, (sg + 1) * seg_len)
        ln = seg_len if (wrong == 'last_seg_len' and sg == nseg - 1) else hi - lo
        ctx = total + hs[:, lo:hi].sum(1) / float(ln)
        g1 = torch.relu(ctx @ q['wa'].t() + q['ba'])
        gates.append(torch.sigmoid(g1 @ q['wb'].t() + q['bb']))
    gate = torch.stack(gates, 1)                                   # [B, nseg, 32]
    seg_of = torch.arange(T2) // seg_len
    if wrong == 'gate_seg0':
        seg_of = torch.zeros_like(seg_of)
    hp = torch.zeros(B, T2 + 2 * dil, h16.shape[2], dtype=dtype)
    hp[:, dil:dil + T2] = h16
    # row t reads hp[t] (tap -dil), hp[t + dil] (itself), hp[t + 2 dil] (tap +dil)
    if wrong == 'tap_plus':
        for t in range(max(0, T2 - dil), T2):
            hp[:, t + 2 * dil] = h16[:, t]
    if wrong == 'tap_minus':
        for t in range(min(dil, T2)):
            hp[:, t] = h16[:, t]
    y = sum(hp[:, tap * dil:tap * dil + T2] @ q['wl'][:, :, tap].t() for tap in range(3))
    y = y * gate[:, seg_of]
    y = _r16(y) if fp16_sites else y
    return (y, gate) if return_gate else y


def block_chain(x0, layers, dil, seg_len, ctx_from):
    """the rounding model's own chain: layer l of the model on the model's channels [0, cin_l) -> the full concat tensor (fp32, fp16 values)"""
    x = x0.float()
    for p in layers:
        y = dense_layer(x, p, dil, seg_len, torch.float32, True, ctx_from)
        x = torch.cat([x, y], 2)
    return x


def teacher_forced(xfull, c_in, layers, dil, seg_len, wrong=None, stale=None, return_gates=False):
    """fp64 reference of every layer on the GIVEN buffer's own channels [0, cin_l): [B, T2, 32 * nlayers] -- error never compounds over the layers.
    stale = (layer, first_row): that layer reads one 16-row tile of its newest 32 input channels as they were BEFORE the previous layer's write
    (zeros here), the ordering bug of a layer that starts before its predecessor's stores have landed."""
    outs, gates = [], []
    for l, p in enumerate(layers):
        cin = c_in + 32 * l
        xin = xfull[..., :cin].double()
        if stale is not None and stale[0] == l:
            xin = xin.clone()
            xin[:, stale[1]:stale[1] + 16, cin - 32:] = 0.0
        y, g = dense_layer(xin, p, dil, seg_len, wrong=wrong, return_gate=True)
        outs.append(y)
        gates.append(g)
    out = torch.cat(outs, 2)
    return (out, gates) if return_gates else out
