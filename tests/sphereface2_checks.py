"""Checks of the fused SphereFace2 loss (csrc/sphereface2.hip) shared by tests/test_sphereface2_triplet.py (the emulator build, CPU tensors) and
tests/test_gpu_sphereface2_triplet.py (the product library on the device).  Each takes the bound library (None = the product library) and a
device.

The oracle (``oracle``) is a numpy restatement of the definition in include/mvector_hip.h: the front -- h, g, zp / zn -- in numpy.float32, one
operation at a time; everything behind it -- softplus, sigma, the row sums, the mean, dz and the gradients -- in fp64.

Bars.  They follow from the arithmetic the kernels chose, never from what they returned.  u = 2^-53 (fp64), N the number of columns.
  * z: the kernels compute the oracle's fp32 expression operation by operation (no contraction, a correctly rounded sqrt), so kernel and oracle
    hand THE SAME z_j to fp64: nothing of the front enters a bar.
  * l_j = wgt (max(x, 0) + log1p(exp(-|x|))): an fp64 exp and log1p are good to 2 u relative on either side, the sum and the product add 2 u:
    6 u relative per side, 12 u between the two.  The N terms are >= 0 and are added in fp64 in some order on either side, (N - 1) u relative
    each.  So |loss_b - ref| <= (2 N + 10) u loss_b, and the row is rounded ONCE to fp32:
        row bar = 2^-24 |loss_ref| + (N + 16) 2^-50 |loss_ref|     (the second term generous by a factor of four)
    which stays below the cap 2^-20 max(|loss_ref|, 1) for every N below 2^29.  The batch mean adds B fp64 terms and rounds once:
    2^-24 |loss| + the mean of the rows' fp64 parts + B u |loss|.
  * w_j = +-wgt sigma(x): exp 2 u, 1 + e, the quotient and the product 3 u: 5 u per side.  sum_j w_j has terms of either sign:
        |saved[b, 1] - ref| <= (N + 16) 2^-50 sum_j |w_j|.
  * gradient (g / B) w_j dz_j, dz = s t h^(t-1) dx: g / B 1 u, the products 4 u, s t 1 u, h^(t-1) at most 6 u, w 5 u: 17 u per side on the whole
    product.  Type A's dx = cos_m -+ q, q = c sin_m / sqrt(1 - c^2) in fp64 from the fp32 c: the product, the quotient and the root add 3 u to q
    and 1 - c^2 carries 2 u / (1 - c^2) of its own, halved by the root, so q is good to (3 + cond) u with cond = 1 / (1 - c^2) -- an ABSOLUTE
    error of dx, which may cancel.  With K = (|g| / B) |w| s t |h^(t-1)|:
        grad bar = 2^-24 |grad_ref| + K (2^-47 |dx| + (1 + cond) 2^-50 |q|)
    (64 u >= 2 * 17 u and 8 (1 + cond) u >= 2 (3 + cond) u), asserted to stay below the cap 2^-16 K |dx| -- 2^-16 of the per-element weight,
    the form tests/margin_loss_checks.py asserts.  (It would not where dx cancels to below 2^-33 of q; no shape here comes near: with cosines in
    (-0.95, 0.95) |dx| >= 0.2 at margin 0.25, and at margin 1.2, where dx changes sign at c = 0.36, no draw lies within 2^-33 of it.)
  * bias gradient (g / B) sum_b saved[b, 1]: 2^-24 |ref| + (|g| / B) (sum_b (N + 16) 2^-50 sum_j |w_j| + (B + 4) u sum_b |W_b|), below the cap
    2^-16 (|g| / B) sum_b sum_j |w_j|.
  A 16-bit gradient is compared for equality with the fp32 gradient rounded once by torch.

Against the reference's results (tests/golden/margin_loss.npz; fp64 throughout, the constants in double) the distance is that of the fp32 front.
  An error d in the argument x of g reaches z through s g' = s t h^(t-1) <= s t.  Type C: x + 1 rounds once (2^-24 * 2), the t - 1 products and
  2 h^t - 1 add t roundings of a value <= 1 behind a derivative of at most 2 t, the margin as a float, the difference, the product with s and
  the sum with b four more of |z|: |dz| <= (2 t + 6) 2^-24 max(|z|, s t).  Type A forms x first: c c, 1 - c c, the root (its input error
  amplified by cond / 2), two products with float constants, the sum: (6 + cond) 2^-24 more behind s t.  So with
  ops = 2 t + 6 (C), 2 t + 12 + max_j cond_j (A) and zscale = max(max_j |z_j|, s t):
      |loss_b - golden| <= ops 2^-24 zscale sum_j |w_j|                    (d l / d z = w)
      |grad - golden|   <= (|g| / B) |w| (|dz| + s t) ops 2^-24 (zscale + 1)  (|d w / d z| <= |w|; dz's own fp32 inputs: the + 1, with s t its scale)
  plus the bars above.  ``golden_bounds`` returns them and the test prints the observed distance beside each."""
import ctypes
import math

import numpy as np
import pytest
import torch

from mvector import _hip
from margin_loss_checks import S, U50, label_columns, make_labels, make_logits, same_bits   # the same draws as the margin losses'

NS = (1, 2, 3, 5, S - 1, S, S + 1, 2 * S + 3)
BS = (1, 3)
TS = (1, 2, 3, 4)
TYPES = ('C', 'A', 'A_wide')
DEVICE_SHAPE = (2, 1_000_003)
BIAS = -0.5


def params(name, t=3, scale=30.0, lanbuda=0.7):
    """'C' and 'A' at margin 0.25 (every cosine of make_logits lies above th: the target always takes cos(theta + m)); 'A_wide' at margin 1.2
    (th = -0.36: about a third of the targets take the continuation c - mmm)"""
    return dict(margin=1.2 if name == 'A_wide' else 0.25, scale=scale, lanbuda=lanbuda, t=t, margin_type=name[0])


def make_bias(dev, value=BIAS):
    return torch.full((1, 1), value, dtype=torch.float32, device=dev)


# ------------------------------------------------------------------------------------------------ the oracle
def front(c, is_target, p, bias):
    """numpy float32 [B, N] cosines -> (z, h): zp at the target, zn elsewhere, and the h of g's argument; one float32 operation at a time"""
    f32 = np.float32
    s, m, t = f32(p['scale']), f32(p['margin']), int(p['t'])
    margin = p['margin']
    cos_m, sin_m = f32(math.cos(margin)), f32(math.sin(margin))
    th, mmm = f32(math.cos(math.pi - margin)), f32(1.0 + math.cos(math.pi - margin))
    with np.errstate(invalid='ignore'):
        if p['margin_type'] == 'A':
            sine = np.sqrt(f32(1.0) - c * c)
            a, bb = c * cos_m, sine * sin_m
            toward = np.where(c > th, a - bb, c - mmm)
            x = np.where(is_target, toward, a + bb)
        else:
            x = c
        h = (x + f32(1.0)) / f32(2.0)
        pw = h.copy()
        for _ in range(t - 1):
            pw = pw * h
        g = f32(2.0) * pw - f32(1.0)
        if p['margin_type'] == 'C':
            g = np.where(is_target, g - m, g + m)
        z = s * g + f32(bias)
    assert z.dtype == np.float32 and h.dtype == np.float32
    return z, h


def oracle(logits, labels, p, bias=BIAS, g=1.0):
    """logits: numpy float32 [B, N]; labels: int64 [B] -> dict of the definition's quantities and their bars (see the module docstring)"""
    B, N = logits.shape
    t, s = int(p['t']), float(np.float32(p['scale']))
    lam = float(np.float32(p['lanbuda']))
    valid = (labels >= 0) & (labels < N)
    is_target = np.zeros((B, N), dtype=bool)
    is_target[np.arange(B)[valid], labels[valid]] = True
    z, h = front(logits, is_target, p, bias)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        x = np.where(is_target, -z.astype(np.float64), z.astype(np.float64))
        wgt = np.where(is_target, lam, 1.0 - lam)
        e = np.exp(-np.abs(x))
        l = wgt * (np.maximum(x, 0.0) + np.log1p(e))
        l = np.where(np.isnan(x), np.nan, l)
        sig = np.where(x >= 0, 1.0, e) / (1.0 + e)
        w = np.where(is_target, -wgt, wgt) * sig
        rows = l.sum(axis=1)
        W = w.sum(axis=1)
        rows[~valid], W[~valid] = np.nan, np.nan
        hd = h.astype(np.float64)
        hp = np.ones_like(hd)
        for _ in range(t - 1):
            hp = hp * hd
        hpa = np.abs(hp)                                  # past pi the continuation c - mmm takes x below -1 and h below 0
        cd = logits.astype(np.float64)
        cos_m, sin_m = float(np.float32(math.cos(p['margin']))), float(np.float32(math.sin(p['margin'])))
        th = np.float32(math.cos(math.pi - p['margin']))
        if p['margin_type'] == 'A':
            cond = 1.0 / (1.0 - cd * cd)
            q = cd * sin_m / np.sqrt(1.0 - cd * cd)
            dx = np.where(is_target, np.where(logits > th, cos_m + q, 1.0), cos_m - q)
            q = np.where(is_target & ~(logits > th), 0.0, q)
        else:
            cond, q, dx = np.ones_like(cd), np.zeros_like(cd), np.ones_like(cd)
        dz = s * t * hp * dx
        grad = (g / B) * w * dz
        grad[~valid] = np.nan
        bias_grad = (g / B) * W.sum()
        K = (abs(g) / B) * np.abs(w) * s * t * hpa
        absw = np.abs(w).sum(axis=1)
        row64 = (N + 16) * U50 * np.abs(rows)
        loss = rows.mean()
        ref = dict(z=z, h=h, w=w, dz=dz, pred=np.argmax(np.where(np.isnan(logits), -np.inf, logits), axis=1).astype(np.int32), rows=rows, W=W,
                   loss=loss, grad=grad, bias_grad=bias_grad, valid=valid, absw=absw,
                   row_bar=2.0 ** -24 * np.abs(rows) + row64, row_cap=2.0 ** -20 * np.maximum(np.abs(rows), 1.0),
                   W_bar=(N + 16) * U50 * absw,
                   loss_bar=2.0 ** -24 * abs(loss) + row64.mean() + B * 2.0 ** -53 * abs(loss),
                   grad_bar=2.0 ** -24 * np.abs(grad) + K * (2.0 ** -47 * np.abs(dx) + (1.0 + cond) * U50 * np.abs(q)),
                   grad_cap=2.0 ** -16 * K * np.abs(dx),
                   bias_bar=2.0 ** -24 * abs(bias_grad) + (abs(g) / B) * (((N + 16) * U50 * absw).sum() + (B + 4) * 2.0 ** -53 * np.abs(W).sum()),
                   bias_cap=2.0 ** -16 * (abs(g) / B) * absw.sum(), cond=cond, K=K)
    return ref


def golden_bounds(ref, p, g=1.0):
    """the distance the fp32 front may put between the kernels and an fp64 evaluation of the same inputs (module docstring): per row for the
    loss, per element for the gradient, one number for the bias gradient"""
    t, s = int(p['t']), float(p['scale'])
    B = ref['rows'].shape[0]
    ops = 2 * t + 6 if p['margin_type'] == 'C' else 2 * t + 12 + ref['cond'].max(axis=1)
    zscale = np.maximum(np.abs(ref['z'].astype(np.float64)).max(axis=1), s * t)
    rows = ops * 2.0 ** -24 * zscale * ref['absw'] + ref['row_bar']
    elem = (abs(g) / B) * np.abs(ref['w']) * (np.abs(ref['dz']) + s * t) * (ops * 2.0 ** -24 * (zscale + 1.0))[:, None] + ref['grad_bar']
    bias = (abs(g) / B) * (ops * 2.0 ** -24 * zscale * ref['absw']).sum() + ref['bias_bar']
    return rows, elem, bias


def run(cdll, logits, labels, bias, p, g=1.0, out=None):
    loss, rows, pred, saved = _hip.sphereface2_forward(logits, labels, bias, cdll=cdll, **p)
    gt = torch.tensor(g, dtype=torch.float32, device=logits.device)
    grad, bias_grad = _hip.sphereface2_backward(logits, labels, bias, saved, gt, out=out, cdll=cdll, **p)
    return loss, rows, pred, saved, grad, bias_grad


# ------------------------------------------------------------------------------------------------ the checks
def check_case(cdll, dev, margin_type, t, B, N, pad=0, seed=0, g=0.75, report=None):
    """forward and backward of one shape against the oracle: pred equal; loss rows, mean, saved, gradient and bias gradient within their bars"""
    p = params(margin_type, t)
    logits, base = make_logits(B, N, 1, seed + 31 * N + B, pad=pad, device=dev)
    labels = make_labels(B, N, seed)
    loss, rows, pred, saved, grad, bias_grad = run(cdll, logits, labels.to(dev), make_bias(dev), p, g)
    ref = oracle(logits.cpu().numpy(), labels.numpy(), p, BIAS, g)
    saved = saved.cpu().numpy()
    assert np.array_equal(pred.cpu().numpy(), ref['pred'])
    assert np.all(ref['row_bar'] <= ref['row_cap']) and np.all(ref['grad_bar'] <= ref['grad_cap'] + 1e-300) and ref['bias_bar'] <= ref['bias_cap']
    rows_err = np.abs(rows.cpu().numpy().astype(np.float64) - ref['rows'])
    assert np.all(rows_err <= ref['row_bar']), (margin_type, t, B, N, rows_err, ref['row_bar'])
    assert np.all(np.abs(saved[:, 0] - ref['rows']) <= ref['row_bar'])
    assert np.all(np.abs(saved[:, 1] - ref['W']) <= ref['W_bar']), (margin_type, t, B, N)
    loss_err = abs(float(loss) - ref['loss'])
    assert loss_err <= ref['loss_bar'], (margin_type, t, B, N, loss_err, ref['loss_bar'])
    grad_err = np.abs(grad.cpu().numpy().astype(np.float64) - ref['grad'])
    assert np.all(grad_err <= ref['grad_bar']), (margin_type, t, B, N, (grad_err / np.maximum(ref['grad_bar'], 1e-300)).max())
    bias_err = abs(float(bias_grad) - ref['bias_grad'])
    assert bias_grad.shape == (1,) and bias_err <= ref['bias_bar'], (margin_type, t, B, N, bias_err, ref['bias_bar'])
    if pad:
        assert torch.all(base[:, N:] == 7.0)
    if report is not None:
        report.append((margin_type, t, B, N, float(np.max(rows_err / ref['row_cap'])), float(np.max(grad_err / np.maximum(ref['grad_cap'], 1e-300))),
                       bias_err / max(ref['bias_cap'], 1e-300)))
    return ref


def print_report(report):
    print('\ntype, t, B, N: loss-row error / cap, gradient error / cap, bias-gradient error / cap')
    for r in report:
        print(f'  {r[0]} t={r[1]} B={r[2]} N={r[3]:<8d}: {r[4]:.3g}  {r[5]:.3g}  {r[6]:.3g}')


def check_type(cdll, dev, margin_type, t):
    """every shape of the list for one margin type and t: a row stride above N at B = 3, and a contiguous B = 3 whose odd N misaligns row 1"""
    report = []
    for i, N in enumerate(NS):
        for B in BS:
            check_case(cdll, dev, margin_type, t, B, N, pad=(5 if B == 3 else 0), seed=i, report=report)
        check_case(cdll, dev, margin_type, t, 3, N, pad=0, seed=i + 1, report=report)
    print_report(report)


def check_device_shape(cdll, dev, margin_type):
    report = []
    check_case(cdll, dev, margin_type, 3, DEVICE_SHAPE[0], DEVICE_SHAPE[1], seed=3, report=report)
    print_report(report)


def check_labels_cover_the_columns():
    """the label draws put a target at columns 0, N - 1, S - 1 and S"""
    seen = set()
    for i, N in enumerate(NS):
        for B, seed in ((1, i), (3, i), (3, i + 1)):
            seen |= {(N, int(c)) for c in make_labels(B, N, seed)}
    for N in NS:
        for c in label_columns(N):
            assert (N, c) in seen, (N, c)


def check_half_inputs(cdll, dev):
    """fp16 / bf16 logits: loss, loss_rows, pred, saved and the bias gradient are the bits of the fp32 path on the upcast logits, the gradient is
    the fp32 path's rounded once to the dtype"""
    for dtype in (torch.float16, torch.bfloat16):
        for margin_type in TYPES:
            p = params(margin_type)
            for B, N, pad in ((3, 5, 0), (3, S + 1, 3), (1, 2 * S + 3, 0)):
                logits, _ = make_logits(B, N, 1, 5 + N, pad=pad, device=dev, dtype=dtype)
                labels = make_labels(B, N, 1).to(dev)
                got = run(cdll, logits, labels, make_bias(dev), p, 0.5)
                want = run(cdll, logits.float(), labels, make_bias(dev), p, 0.5)
                for a, b, what in zip(got[:4] + got[5:], want[:4] + want[5:], ('loss', 'loss_rows', 'pred', 'saved', 'bias_grad')):
                    assert same_bits(a, b), (dtype, margin_type, B, N, what)
                assert got[4].dtype == dtype and torch.equal(got[4], want[4].to(dtype)), (dtype, margin_type, B, N)


def check_in_place(cdll, dev):
    """out = the logits themselves gives the bits of the out-of-place backward"""
    for margin_type in TYPES:
        p = params(margin_type)
        for dtype in (torch.float32, torch.float16):
            for B, N, pad in ((3, 5, 0), (3, S + 1, 0), (2, 2 * S + 3, 7)):
                logits, base = make_logits(B, N, 1, 9 + N, pad=pad, device=dev, dtype=dtype)
                labels = make_labels(B, N, 2).to(dev)
                bias = make_bias(dev)
                *_, saved, want, want_bias = run(cdll, logits, labels, bias, p, 1.25)
                gt = torch.tensor(1.25, dtype=torch.float32, device=dev)
                got, got_bias = _hip.sphereface2_backward(logits, labels, bias, saved, gt, out=logits, cdll=cdll, **p)
                assert got.data_ptr() == logits.data_ptr() and same_bits(got, want) and same_bits(got_bias, want_bias), (margin_type, dtype, B, N)
                if pad:
                    assert torch.all(base[:, N:] == 7.0)


def raw_forward(cdll, logits, labels, bias, p, fill):
    """mv_sphereface2_forward with every output and the workspace pre-filled with the byte ``fill``"""
    cfg = _hip.sphereface2_cfg(**p)
    B, N = logits.shape
    dev = logits.device
    mk = lambda n: torch.full((max(n, 1),), fill, dtype=torch.uint8, device=dev)
    nbytes = int(cdll.mv_sphereface2_workspace_bytes(B, N))
    loss, rows, pred, saved, ws = mk(4), mk(4 * B), mk(4 * B), mk(8 * _hip.MV_SF2_SAVED * B), mk(max(nbytes, 16))
    _hip.check(cdll.mv_sphereface2_forward(ctypes.byref(cfg), logits.data_ptr(), _hip._MARGIN_DTYPES[logits.dtype], labels.data_ptr(),
                                           bias.data_ptr(), B, N, logits.stride(0), loss.data_ptr(), rows.data_ptr(), pred.data_ptr(),
                                           saved.data_ptr(), ws.data_ptr(), nbytes, _hip.current_stream(logits)), cdll)
    return loss[:4].view(torch.float32)[0], rows[:4 * B].view(torch.float32), pred[:4 * B].view(torch.int32), \
        saved[:8 * _hip.MV_SF2_SAVED * B].view(torch.float64).reshape(B, -1)


def check_no_hidden_state(cdll, dev, second_stream=False):
    """a row alone equals the row in a batch (also where the batch misaligns it); buffers pre-filled with 0xFF give what zeros give; on the
    device the same on a second stream"""
    lib = cdll or _hip.lib()
    for margin_type in TYPES:
        p = params(margin_type)
        for N in (5, S + 1, 2 * S + 3):
            B = 3
            logits, _ = make_logits(B, N, 1, 17 + N, device=dev)
            labels = make_labels(B, N, 0).to(dev)
            bias = make_bias(dev)
            loss, rows, pred, saved, grad, bias_grad = run(cdll, logits, labels, bias, p, 1.0)
            grad_b = run(cdll, logits, labels, bias, p, float(B))[4]
            for b in range(B):
                # the row where it lies in the batch, and a copy of it (16-byte aligned whatever the batch did to the row); the gradient of the
                # batch with g = B against the row's with g = 1: g / B is 1 in both
                for one in (logits[b:b + 1], logits[b:b + 1].clone()):
                    _, r1, p1, s1, g1, _ = run(cdll, one, labels[b:b + 1], bias, p, 1.0)
                    assert same_bits(r1, rows[b:b + 1]) and same_bits(p1, pred[b:b + 1]) and same_bits(s1, saved[b:b + 1]), (margin_type, N, b)
                    assert same_bits(g1, grad_b[b:b + 1]), (margin_type, N, b)
            outs = [raw_forward(lib, logits, labels, bias, p, fill) for fill in (0x00, 0xFF)]
            for a, b_, c in zip(outs[0], outs[1], (loss, rows, pred, saved)):
                assert same_bits(a, b_) and same_bits(a, c), (margin_type, N)
            for fill in (0.0, float('nan')):
                out = torch.full_like(logits, fill)
                got = _hip.sphereface2_backward(logits, labels, bias, saved, torch.ones((), device=dev), out=out, cdll=cdll, **p)
                assert same_bits(got[0], grad) and same_bits(got[1], bias_grad)
            if second_stream:
                stream = torch.cuda.Stream()
                stream.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(stream):
                    other = run(cdll, logits, labels, bias, p, 1.0)
                stream.synchronize()
                for a, b_ in zip(other, (loss, rows, pred, saved, grad, bias_grad)):
                    assert same_bits(a, b_), (margin_type, N)


def check_bad_labels(cdll, dev):
    """labels -1, N and 2^31 - 1: the row, the mean, every column of the row's gradient and the bias gradient are NaN, pred is valid, the other
    rows are what they are with a valid label there, and the columns behind the row (the stride's padding) are untouched"""
    for margin_type in TYPES:
        p = params(margin_type)
        for N in (3, S + 1):
            B = 3
            logits, base = make_logits(B, N, 1, 23 + N, pad=9, device=dev)
            good = make_labels(B, N, 1).to(dev)
            bias = make_bias(dev)
            _, rows0, pred0, saved0, grad0, _ = run(cdll, logits, good, bias, p, 1.0)
            for bad in (-1, N, 2 ** 31 - 1):
                labels = good.clone()
                labels[1] = bad
                out_base = torch.full_like(base, 7.0)
                out = out_base[:, :N]
                loss, rows, pred, saved, grad, bias_grad = run(cdll, logits, labels, bias, p, 1.0, out=out)
                assert math.isnan(float(loss)) and math.isnan(float(rows[1])) and bool(torch.isnan(grad[1]).all()), (margin_type, N, bad)
                assert math.isnan(float(bias_grad)) and bool(torch.isnan(saved[1]).all())
                assert torch.equal(pred, pred0)
                for b in (0, 2):
                    assert same_bits(rows[b], rows0[b]) and same_bits(saved[b], saved0[b]) and same_bits(grad[b], grad0[b]), (margin_type, N, bad, b)
                assert torch.all(out_base[:, N:] == 7.0) and torch.all(base[:, N:] == 7.0)


def check_nan_logit(cdll, dev):
    """a NaN logit: its row, the mean, its own gradient and the bias gradient are NaN; the other rows are unchanged"""
    for margin_type in TYPES:
        p = params(margin_type)
        B, N = 3, S + 1
        logits, _ = make_logits(B, N, 1, 41, device=dev)
        labels = make_labels(B, N, 0).to(dev)
        bias = make_bias(dev)
        _, rows0, _, _, grad0, _ = run(cdll, logits, labels, bias, p, 1.0)
        logits = logits.clone()
        logits[1, N - 2] = float('nan')
        loss, rows, _, _, grad, bias_grad = run(cdll, logits, labels, bias, p, 1.0)
        assert math.isnan(float(loss)) and math.isnan(float(rows[1])) and math.isnan(float(bias_grad)) and math.isnan(float(grad[1, N - 2]))
        for b in (0, 2):
            assert same_bits(rows[b], rows0[b]) and same_bits(grad[b], grad0[b])


def check_refusals(cdll, dev):
    """every refusal of include/mvector_hip.h by name; B = 0 touches nothing"""
    lib = cdll or _hip.lib()
    B, N = 2, 6
    x = torch.zeros((B, N), dtype=torch.float32, device=dev)
    y = torch.zeros((B,), dtype=torch.int64, device=dev)
    f = lambda n, dt=torch.float32: torch.zeros((max(n, 1),), dtype=dt, device=dev)
    loss, rows, pred, saved, gout, out, bgrad, bias = f(1), f(B), f(B, torch.int32), f(B * 2, torch.float64), f(1), torch.zeros_like(x), f(1), f(1)
    ws = torch.zeros((4096,), dtype=torch.uint8, device=dev)

    def fwd(cfg=None, logits=x, dtype=0, labels=y, bias_=bias, B_=B, N_=N, stride=N, loss_=loss, ws_=ws, ws_bytes=4096, null_cfg=False):
        cfg = cfg or _hip.sphereface2_cfg()
        return lib.mv_sphereface2_forward(None if null_cfg else ctypes.byref(cfg), _hip._ptr(logits), dtype, _hip._ptr(labels), _hip._ptr(bias_),
                                          B_, N_, stride, _hip._ptr(loss_), rows.data_ptr(), pred.data_ptr(), saved.data_ptr(), _hip._ptr(ws_),
                                          ws_bytes, None)

    def bwd(cfg=None, logits=x, dtype=0, labels=y, bias_=bias, B_=B, N_=N, stride=N, saved_=saved, gout_=gout, out_=out, out_ptr=None, out_stride=N,
            bgrad_=bgrad, null_cfg=False):
        cfg = cfg or _hip.sphereface2_cfg()
        return lib.mv_sphereface2_backward(None if null_cfg else ctypes.byref(cfg), _hip._ptr(logits), dtype, _hip._ptr(labels), _hip._ptr(bias_), B_,
                                           N_, stride, _hip._ptr(saved_), _hip._ptr(gout_),
                                           out_ptr if out_ptr is not None else _hip._ptr(out_), out_stride, _hip._ptr(bgrad_), None)

    def refused(rc, text):
        assert rc != 0
        with pytest.raises(RuntimeError, match=text):
            _hip.check(rc, lib)

    def cfg_with(**fields):
        cfg = _hip.sphereface2_cfg()
        for k, v in fields.items():
            setattr(cfg, k, v)
        return cfg

    assert fwd() == 0 and bwd() == 0
    for call in (fwd, bwd):
        refused(call(null_cfg=True), 'null cfg')
        refused(call(B_=-1), 'negative B or N')
        refused(call(N_=-1, stride=0), 'negative B or N')
        refused(call(cfg=cfg_with(margin_type=2)), 'unknown margin_type')
        refused(call(cfg=cfg_with(margin_type=-1)), 'unknown margin_type')
        for t in (0, 9, -3):
            refused(call(cfg=cfg_with(t=t)), 't outside 1 .. 8')
        for lam in (-0.1, 1.5, float('nan')):
            refused(call(cfg=cfg_with(lanbuda=lam)), 'lanbuda outside \\[0, 1\\]')
        assert call(cfg=cfg_with(lanbuda=0.0)) == 0 and call(cfg=cfg_with(lanbuda=1.0)) == 0 and call(cfg=cfg_with(t=8)) == 0
        refused(call(dtype=3), 'unknown dtype')
        refused(call(stride=N - 1), 'stride below N')
        refused(call(N_=2 ** 31, stride=2 ** 31), 'N above 2\\^31 - 1')
        refused(call(stride=2 ** 61), 'B \\* stride beyond int64')
        refused(call(B_=2 ** 31), 'B above 2\\^31 - 1')
        refused(call(N_=0, stride=0), 'N = 0')
        refused(call(B_=2 ** 31 - 1, N_=2 * S, stride=2 * S), 'B \\* segments above 2\\^31 - 1')
        refused(call(logits=None), 'null logits or labels')
        refused(call(labels=None), 'null logits or labels')
        refused(call(bias_=None), 'null bias')
    refused(fwd(loss_=None), 'null output')
    refused(fwd(ws_=None), 'null workspace')
    need = int(lib.mv_sphereface2_workspace_bytes(B, N))
    assert need == 48 and lib.mv_sphereface2_workspace_bytes(B, -1) == 0 and lib.mv_sphereface2_workspace_bytes(0, N) == 0
    refused(fwd(ws_bytes=need - 1), 'workspace smaller than mv_sphereface2_workspace_bytes')
    rc = lib.mv_sphereface2_forward(ctypes.byref(_hip.sphereface2_cfg()), x.data_ptr(), 0, y.data_ptr(), bias.data_ptr(), B, N, N,
                                    loss.data_ptr(), rows.data_ptr(), pred.data_ptr(), saved.data_ptr(), ws.data_ptr() + 4, 4000, None)
    refused(rc, 'workspace not 16-byte aligned')
    for name in ('saved_', 'gout_', 'out_', 'bgrad_'):
        refused(bwd(**{name: None}), 'null saved, grad_out, out or bias_grad')
    refused(bwd(out_stride=N - 1), 'out_stride below N')
    refused(bwd(out_stride=2 ** 61), 'B \\* out_stride beyond int64')
    refused(bwd(B_=2 ** 31 - 1), 'B \\* column tiles \\+ 1 above 2\\^31 - 1')     # one tile a row, and the bias gradient's workgroup
    refused(bwd(out_ptr=x.data_ptr() + 4), 'out overlaps logits')                 # shifted by one element
    refused(bwd(out_ptr=x.data_ptr(), out_stride=N + 1), 'out overlaps logits')   # the same base, another stride
    assert bwd(out_ptr=x.data_ptr()) == 0                                         # in place
    # B = 0: MV_OK with null pointers everywhere, nothing touched
    cfg = _hip.sphereface2_cfg()
    assert lib.mv_sphereface2_forward(ctypes.byref(cfg), None, 0, None, None, 0, N, N, None, None, None, None, None, 0, None) == 0
    assert lib.mv_sphereface2_backward(ctypes.byref(cfg), None, 0, None, None, 0, N, N, None, None, None, N, None, None) == 0
    # the Python wrapper names what it refuses itself
    with pytest.raises(ValueError, match='not one of'):
        _hip.sphereface2_forward(x, y, bias, margin_type='B', cdll=cdll)
    with pytest.raises(ValueError, match='not an integer'):
        _hip.sphereface2_forward(x, y, bias, t=2.5, cdll=cdll)
    with pytest.raises(ValueError, match='2-D fp32, fp16 or bf16'):
        _hip.sphereface2_forward(x.double(), y, bias, cdll=cdll)
    with pytest.raises(ValueError, match='bias must be one fp32 value'):
        _hip.sphereface2_forward(x, y, bias.double(), cdll=cdll)


def check_golden(cdll, dev, golden):
    """the native path on the inputs of tests/golden/margin_loss.npz against the reference's fp64 results: within the bound of the fp32 front"""
    logits = torch.from_numpy(golden['logits']).to(dev)
    labels = torch.from_numpy(golden['labels'])
    print()
    for case in ('sphereface2_C', 'sphereface2_A'):
        args = golden[case + '.args']
        p = dict(margin=float(args[0]), scale=float(args[1]), lanbuda=float(args[2]), t=int(args[3]), margin_type='CA'[int(args[4])])
        loss, rows, _, _, grad, bias_grad = run(cdll, logits, labels.to(dev), make_bias(dev), p, 1.0)
        ref = oracle(golden['logits'], golden['labels'], p, BIAS, 1.0)
        row_b, elem_b, bias_b = golden_bounds(ref, p, 1.0)
        d_loss = abs(float(loss) - float(golden[case + '.loss']))
        d_grad = np.abs(grad.cpu().numpy().astype(np.float64) - golden[case + '.grad'])
        d_bias = abs(float(bias_grad) - float(golden[case + '.bias_grad'].reshape(-1)[0]))
        print(f'  {case}: |loss - golden| {d_loss:.3g} (bound {row_b.mean():.3g}); max |grad - golden| / bound {(d_grad / elem_b).max():.3g} '
              f'(max distance {d_grad.max():.3g}); |bias_grad - golden| {d_bias:.3g} (bound {bias_b:.3g})')
        assert d_loss <= row_b.mean() and np.all(d_grad <= elem_b) and d_bias <= bias_b, case
