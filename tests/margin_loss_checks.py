"""Checks of the fused margin-softmax losses (csrc/marginloss.hip) shared by tests/test_margin_loss.py (the emulator build, CPU tensors) and
tests/test_gpu_margin_loss.py (the product library on the device).  Each takes the bound library (None = the product library) and a device.

The oracle (``oracle``) is a numpy restatement of the definition in include/mvector_hip.h: the centre cosines and z in numpy.float32, one
operation at a time; everything behind z -- the row maximum, lse, the row loss, the mean, p, q, dz and the gradient -- in fp64.

Bars.  They follow from the arithmetic the kernels chose, never from what they returned.  u = 2^-53 (fp64), N the number of centres.
  * z is compared for equality: the kernels compute the oracle's fp32 expression operation by operation (no contraction, a correctly rounded
    sqrt), so kernel and oracle add THE SAME terms.
  * S = sum exp(z_j - M): the arguments are exact in fp64 (both operands are floats); an fp64 exp is good to 2 u relative on either side;
    the N positive terms are added in fp64 in some order on either side, (N - 1) u relative each.  log adds 2 u |log S| + 2 u, the sum M + log S
    one more u |lse|.  So |lse - lse_ref| <= 2 (N + 4) u + 6 u |lse|.
  * sum z_j has terms of either sign: |error| <= 2 (N - 1) u sum |z_j| over both sides, so the mean's is 2 u sum |z_j| <= 2 N u mean |z|.
  * the row loss combines these with weights of at most 1 (three more roundings, 3 u each of the magnitudes) and is rounded ONCE to fp32.
  Hence  row bar = 2^-24 |loss_ref| + (N + 16) 2^-50 (|lse| + |z_y| + mean |z| + 1), generous by a factor of four or so in its second term
  and still, at N = 10^6, a thousand times below the 2^-24 |loss| of the fp32 rounding.  check_case asserts that it stays below the
  issue's condition 2^-20 max(|lse|, |z_y|, |mean z|, 1).  The batch mean adds B fp64 terms and rounds once: 2^-24 |loss| + the mean of the row
  bars' fp64 parts + B u |loss|.
  * gradient: p_j = exp(z_j - lse) inherits the error of lse as a RELATIVE error d = 2 (N + 4) u + 6 u |lse| + 2 u; (p - q) therefore carries
    the ABSOLUTE error p d -- the cancellation at the target is why the bar has a term in p and not only in |p - q|; g / B, the two products
    and dz (on the phi branch a quotient and an fp64 sqrt of 1 - c^2 with |c| <= 1 - 2^-12, conditioned by at most 2^12) add a few u
    relative; the result is rounded once to fp32.  Hence
        grad bar = 2^-24 |grad_ref| + (|g| / B) |dz| p (N + 32) 2^-50 + 2^-36 |grad_ref|
    and check_case asserts that this stays below the issue's cap (|g| / B) |dz| (2^-16 p + 2^-22 |p - q|).
  A 16-bit result is compared for equality with the fp32 result rounded once by torch."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from mvector import _hip

S = _hip.MV_MARGIN_SEG
U50 = 2.0 ** -50
KINDS = {   # name: (kind, arguments beside label_smoothing)
    'ce': ('ce', {}),
    'am': ('am', dict(margin=0.3, scale=30.0)),
    'arm': ('arm', dict(margin=0.3, scale=30.0)),
    'aam': ('aam', dict(margin=0.25, scale=30.0)),
    'aam_easy': ('aam', dict(margin=0.25, scale=30.0, easy_margin=True)),
    'subcenter2': ('subcenter', dict(margin=0.25, scale=30.0, K=2)),
    'subcenter3': ('subcenter', dict(margin=0.25, scale=30.0, K=3)),
    'subcenter3_easy': ('subcenter', dict(margin=0.25, scale=30.0, K=3, easy_margin=True)),
}
NS = (1, 2, 3, 5, S - 1, S, S + 1, 2 * S + 3)
BS = (1, 3)
DEVICE_SHAPES = ((2, 1_000_003, 1, 'aam'), (2, 333_337, 3, 'subcenter3'))


def params(name, eps=0.0):
    kind, kw = KINDS[name]
    return dict(dict(kind=kind, margin=0.2, scale=32.0, easy_margin=False, K=1), label_smoothing=eps, **kw)


def label_columns(N):
    """labels at column 0, N - 1, S - 1 and S where the row has them"""
    return sorted({0, N - 1} | {c for c in (S - 1, S) if c < N})


def make_logits(B, N, K, seed, pad=0, device='cpu', dtype=torch.float32):
    """cosine-like logits in (-1, 1) with a row stride of N * K + pad; the pad columns hold a sentinel no kernel may touch.  Returns the
    [B, N * K] view and its base tensor."""
    g = torch.Generator().manual_seed(seed)
    base = torch.full((B, N * K + pad), 7.0, dtype=torch.float32)
    base[:, :N * K] = torch.rand(B, N * K, generator=g) * 1.9 - 0.95
    base = base.to(dtype).to(device)
    return base[:, :N * K], base


def make_labels(B, N, seed):
    cols = label_columns(N)
    return torch.tensor([cols[(seed + b) % len(cols)] for b in range(B)], dtype=torch.int64)


# ------------------------------------------------------------------------------------------------ the oracle
def oracle(logits, labels, p, g=1.0):
    """logits: numpy float32 [B, N * K]; labels: int64 [B] -> dict of the definition's quantities (see the module docstring)"""
    f32 = np.float32
    B, K = logits.shape[0], p['K']
    N = logits.shape[1] // K
    kind, s, eps = p['kind'], f32(p['scale']), float(f32(p['label_smoothing']))
    grp = logits.reshape(B, N, K)
    ka = np.argmax(grp, axis=2)
    c = np.take_along_axis(grp, ka[:, :, None], axis=2)[:, :, 0]
    valid = (labels >= 0) & (labels < N)
    y = np.where(valid, labels, 0)
    rows = np.arange(B)
    cy = c[rows, y]
    cos_m, sin_m = f32(math.cos(p['margin'])), f32(math.sin(p['margin']))
    th, mmm = f32(math.cos(math.pi - p['margin'])), f32(1.0 + math.cos(math.pi - p['margin']))
    phi_branch = np.zeros(B, dtype=bool)
    with np.errstate(invalid='ignore'):
        if kind == 'ce':
            z, zy = c.copy(), cy.copy()
        elif kind in ('am', 'arm'):
            z = s * c
            zy = s * (cy - f32(p['margin']))
        else:
            z = s * c
            sine = np.sqrt(f32(1.0) - cy * cy)
            phi = cy * cos_m - sine * sin_m
            phi_branch = cy > 0 if p['easy_margin'] else cy > th
            zy = (np.where(phi_branch, phi, cy) if p['easy_margin'] else np.where(phi_branch, phi, cy - mmm)) * s
        zy = np.where(valid, zy, f32('nan')).astype(f32)
        z[rows[valid], y[valid]] = zy[valid]
        zeroed = np.zeros_like(z, dtype=bool)
        if kind == 'arm':
            zeroed = (z - zy[:, None]) < 0
            z = np.where(zeroed, f32(0), z)
        assert z.dtype == np.float32 and zy.dtype == np.float32
        zd = z.astype(np.float64)
        M = zd.max(axis=1)
        logS = np.log(np.exp(zd - M[:, None]).sum(axis=1))
        lse = M + logS
        meanz = zd.mean(axis=1)
        rows_loss = (1.0 - eps) * (lse - zy.astype(np.float64))
        if eps > 0:
            rows_loss = rows_loss + eps * (lse - meanz)
        pj = np.exp(zd - lse[:, None])
        q = np.full_like(zd, eps / N)
        q[rows, y] += 1.0 - eps
        dz = np.full_like(zd, 1.0 if kind == 'ce' else float(s))
        dz[zeroed] = 0.0
        cyd = cy.astype(np.float64)
        dphi = float(s) * (float(cos_m) + cyd * float(sin_m) / np.sqrt(1.0 - cyd * cyd))
        sel = valid & phi_branch
        dz[rows[sel], y[sel]] = dphi[sel]
        gc = (g / B) * (pj - q) * dz
        gc[~valid] = np.nan
        grad = np.zeros((B, N, K))
        np.put_along_axis(grad, ka[:, :, None], gc[:, :, None], axis=2)
        grad[~valid] = np.nan
    row_bar64 = (N + 16) * U50 * (np.abs(lse) + np.abs(zy.astype(np.float64)) + np.abs(zd).mean(axis=1) + 1.0)
    gbar_c = 2.0 ** -24 * np.abs(gc) + (abs(g) / B) * np.abs(dz) * pj * (N + 32) * U50 + 2.0 ** -36 * np.abs(gc)
    gcap_c = (abs(g) / B) * np.abs(dz) * (2.0 ** -16 * pj + 2.0 ** -22 * np.abs(pj - q))
    expand = lambda a: np.repeat(a[:, :, None], K, axis=2).reshape(B, N * K)
    return dict(zy=zy, z=z, pred=np.argmax(c, axis=1).astype(np.int32), M=M, logS=logS, lse=lse, meanz=meanz, rows=rows_loss,
                loss=rows_loss.mean(), grad=grad.reshape(B, N * K), valid=valid, row_bar=2.0 ** -24 * np.abs(rows_loss) + row_bar64,
                row_cap=2.0 ** -20 * np.maximum.reduce([np.abs(lse), np.abs(zy.astype(np.float64)), np.abs(meanz), np.ones(B)]),
                loss_bar=2.0 ** -24 * abs(rows_loss.mean()) + row_bar64.mean() + B * 2.0 ** -53 * abs(rows_loss.mean()),
                grad_bar=expand(gbar_c), grad_cap=expand(gcap_c))


def torch_fp32_restatement(logits, labels, p, g=1.0):
    """the package's torch expression in fp32 on the CPU: where eager torch itself sits against the oracle (printed, no bar)"""
    from mvector.loss.softmax_family import margin_logits
    x = logits.detach().float().cpu().clone().requires_grad_(True)
    z = margin_logits(x, labels.cpu(), p['kind'], p['margin'], p['scale'], p['easy_margin'], p['K'])
    loss = torch.nn.functional.cross_entropy(z, labels.cpu(), label_smoothing=p['label_smoothing'])
    (loss * g).backward()
    return loss.detach(), x.grad


def torch_fp32_target(logits, labels, p):
    """z of the target column as the reference's modules evaluate it: torch float32 tensors on the CPU, one torch operation -- one rounding --
    at a time, Python scalars entering as torch takes them (as float32).  The square root alone goes through fp64 and back: for the square
    root of a float that IS the correctly rounded float (53 >= 2 * 24 + 2 bits: the second rounding cannot move it), which is what
    torch.sqrt returns on its scalar and AVX2 paths; the AVX512 path of torch 2.10 returns the neighbouring float for about 0.6 % of its
    inputs (sqrt(0x3f004163) -> 0x3f353329, correctly rounded 0x3f35332a), and a check of bits cannot stand on which host it runs on."""
    x = logits.detach().float().cpu()
    B, K = x.shape[0], p['K']
    cosine = x if K == 1 else torch.max(x.reshape(B, -1, K), 2)[0]
    cy = cosine.gather(1, labels.cpu().reshape(-1, 1))
    if p['kind'] == 'ce':
        return cy[:, 0]
    if p['kind'] in ('am', 'arm'):
        delta = torch.zeros_like(cy).fill_(p['margin'])     # the margin written into a float32 tensor
        return (p['scale'] * (cy - delta))[:, 0]
    margin = p['margin']
    sine = torch.sqrt((1.0 - torch.pow(cy, 2)).double()).float()
    phi = cy * math.cos(margin) - sine * math.sin(margin)
    if p['easy_margin']:
        phi = torch.where(cy > 0, phi, cy)
    else:
        phi = torch.where(cy > math.cos(math.pi - margin), phi, cy - (1.0 + math.cos(math.pi - margin)))
    return (phi * p['scale'])[:, 0]


def run(cdll, logits, labels, p, g=1.0, out=None):
    loss, rows, pred, saved = _hip.margin_ce_forward(logits, labels, cdll=cdll, **p)
    gt = torch.tensor(g, dtype=torch.float32, device=logits.device)
    grad = _hip.margin_ce_backward(logits, labels, saved, gt, out=out, cdll=cdll, **p)
    return loss, rows, pred, saved, grad


def same_bits(a, b):
    """tensors equal bit for bit (NaNs of the same bits included)"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.bfloat16:
        a, b = a.view(torch.int16), b.view(torch.int16)
    return a.numpy().tobytes() == b.numpy().tobytes()


# ------------------------------------------------------------------------------------------------ the checks
def check_case(cdll, dev, name, B, N, eps=0.0, pad=0, seed=0, g=0.75, report=None):
    """forward and backward of one shape against the oracle: z_y and pred equal, loss rows, mean and gradient within their derived bars"""
    p = params(name, eps)
    K = p['K']
    logits, _ = make_logits(B, N, K, seed + 31 * N + B, pad=pad, device=dev)
    labels = make_labels(B, N, seed)
    loss, rows, pred, saved, grad = run(cdll, logits, labels.to(dev), p, g)
    ref = oracle(logits.cpu().numpy(), labels.numpy(), p, g)
    saved = saved.cpu().numpy()
    # z_y: the bits of the oracle's fp32 expression AND of the torch fp32 expression
    zy = saved[:, 2].astype(np.float32)
    assert np.array_equal(saved[:, 2], zy.astype(np.float64))
    assert zy.tobytes() == ref['zy'].tobytes(), (name, B, N, zy, ref['zy'])
    t_zy = torch_fp32_target(logits, labels, p)
    assert zy.tobytes() == t_zy.numpy().tobytes(), (name, B, N, zy, t_zy)
    t_loss, t_grad = torch_fp32_restatement(logits, labels, p, g)
    assert np.array_equal(pred.cpu().numpy(), ref['pred'])
    assert np.array_equal(saved[:, 0], ref['M'])                         # a maximum is exact
    assert np.all(ref['row_bar'] <= ref['row_cap']) and np.all(ref['grad_bar'] <= ref['grad_cap'] + 1e-300)
    rows_err = np.abs(rows.cpu().numpy().astype(np.float64) - ref['rows'])
    assert np.all(rows_err <= ref['row_bar']), (name, B, N, rows_err, ref['row_bar'])
    assert np.all(np.abs(saved[:, 3] - ref['rows']) <= ref['row_bar'])
    assert np.all(np.abs(saved[:, 1] - ref['logS']) <= ref['row_bar'])
    loss_err = abs(float(loss) - ref['loss'])
    assert loss_err <= ref['loss_bar'], (name, B, N, loss_err, ref['loss_bar'])
    if N == 1 and eps == 0:
        assert np.all(rows.cpu().numpy() == 0) and float(loss) == 0
    grad_err = np.abs(grad.cpu().numpy().astype(np.float64) - ref['grad'])
    assert np.all(grad_err <= ref['grad_bar']), (name, B, N, (grad_err / np.maximum(ref['grad_bar'], 1e-300)).max())
    if report is not None:
        with np.errstate(invalid='ignore', divide='ignore'):
            cap = np.maximum(ref['grad_cap'], 1e-300)
            report.append((name, B, N, eps, float(np.max(rows_err / ref['row_cap'])), float(np.max(grad_err / cap)),
                           float(np.max(np.abs(t_grad.numpy().astype(np.float64) - ref['grad']) / cap)),
                           abs(float(t_loss) - ref['loss']) / max(abs(ref['loss']), 1.0), loss_err / max(abs(ref['loss']), 1.0)))
    return ref


def print_report(report):
    print('\nkind, B, N, eps: kernel loss-row error / cap, kernel grad error / cap, torch-fp32 grad error / cap (for information), '
          'torch-fp32 loss rel. error (for information), kernel loss rel. error')
    for r in report:
        print(f'  {r[0]:16s} B={r[1]} N={r[2]:<8d} eps={r[3]}: {r[4]:.3g}  {r[5]:.3g}  {r[6]:.3g}  {r[7]:.3g}  {r[8]:.3g}')


def check_kind(cdll, dev, name):
    """every shape of the list for one kind; eps = 0.1 and a row stride above N * K take turns so that each occurs at every N"""
    report = []
    for i, N in enumerate(NS):
        for B in BS:
            eps = 0.1 if (i + B) % 2 else 0.0
            check_case(cdll, dev, name, B, N, eps=eps, pad=(5 if B == 3 else 0), seed=i, report=report)
        check_case(cdll, dev, name, 3, N, eps=0.1 if i % 2 else 0.0, pad=0, seed=i + 1, report=report)   # contiguous: an odd N * K misaligns row 1
    print_report(report)


def check_device_shape(cdll, dev, B, N, K, name):
    report = []
    p = params(name)
    assert p['K'] == K
    check_case(cdll, dev, name, B, N, eps=0.1, seed=3, report=report)
    print_report(report)


def check_half_inputs(cdll, dev):
    """fp16 / bf16 logits: loss, loss_rows, pred and saved are the bits of the fp32 path on the upcast logits, the gradient is the fp32
    path's rounded once to the dtype"""
    for dtype in (torch.float16, torch.bfloat16):
        for name in ('ce', 'arm', 'aam', 'subcenter3'):
            p = params(name, 0.1)
            for B, N, pad in ((3, 5, 0), (3, S + 1, 3), (1, 2 * S + 3, 0)):
                logits, _ = make_logits(B, N, p['K'], 5 + N, pad=pad, device=dev, dtype=dtype)
                labels = make_labels(B, N, 1).to(dev)
                got = run(cdll, logits, labels, p, 0.5)
                want = run(cdll, logits.float(), labels, p, 0.5)
                for a, b, what in zip(got[:4], want[:4], ('loss', 'loss_rows', 'pred', 'saved')):
                    assert same_bits(a, b), (dtype, name, B, N, what)
                assert got[4].dtype == dtype and torch.equal(got[4], want[4].to(dtype)), (dtype, name, B, N)


def check_in_place(cdll, dev):
    """out = the logits themselves gives the bits of the out-of-place backward, for every kind"""
    for name in KINDS:
        p = params(name, 0.1)
        for dtype in (torch.float32, torch.float16):
            for B, N, pad in ((3, 5, 0), (3, S + 1, 0), (2, 2 * S + 3, 7)):
                logits, base = make_logits(B, N, p['K'], 9 + N, pad=pad, device=dev, dtype=dtype)
                labels = make_labels(B, N, 2).to(dev)
                *_, saved, want = run(cdll, logits, labels, p, 1.25)
                gt = torch.tensor(1.25, dtype=torch.float32, device=dev)
                got = _hip.margin_ce_backward(logits, labels, saved, gt, out=logits, cdll=cdll, **p)
                assert got.data_ptr() == logits.data_ptr() and same_bits(got, want), (name, dtype, B, N)
                if pad:
                    assert torch.all(base[:, N * p['K']:] == 7.0)


def raw_forward(cdll, logits, labels, p, fill):
    """mv_margin_ce_forward with every output and the workspace pre-filled with the byte ``fill``"""
    cfg = _hip.margin_cfg(**p)
    B, N = logits.shape[0], logits.shape[1] // p['K']
    dev = logits.device
    mk = lambda n: torch.full((max(n, 1),), fill, dtype=torch.uint8, device=dev)
    nbytes = int(cdll.mv_margin_ce_workspace_bytes(B, N, p['K']))
    loss, rows, pred, saved, ws = mk(4), mk(4 * B), mk(4 * B), mk(8 * _hip.MV_MARGIN_SAVED * B), mk(max(nbytes, 16))
    _hip.check(cdll.mv_margin_ce_forward(ctypes.byref(cfg), logits.data_ptr(), _hip._MARGIN_DTYPES[logits.dtype], labels.data_ptr(), B, N,
                                         logits.stride(0), loss.data_ptr(), rows.data_ptr(), pred.data_ptr(), saved.data_ptr(), ws.data_ptr(),
                                         nbytes, _hip.current_stream(logits)), cdll)
    return loss[:4].view(torch.float32)[0], rows[:4 * B].view(torch.float32), pred[:4 * B].view(torch.int32), \
        saved[:8 * _hip.MV_MARGIN_SAVED * B].view(torch.float64).reshape(B, -1)


def check_no_hidden_state(cdll, dev, second_stream=False):
    """a row alone equals the row in a batch (also where the batch misaligns it); buffers pre-filled with 0xFF give what zeros give; on the
    device the same on a second stream"""
    lib = cdll or _hip.lib()
    for name in ('ce', 'arm', 'aam', 'subcenter3'):
        p = params(name, 0.1)
        for N in (5, S + 1, 2 * S + 3):
            B = 3
            logits, _ = make_logits(B, N, p['K'], 17 + N, device=dev)
            labels = make_labels(B, N, 0).to(dev)
            loss, rows, pred, saved, grad = run(cdll, logits, labels, p, 1.0)
            grad_b = run(cdll, logits, labels, p, float(B))[4]
            for b in range(B):
                # the row where it lies in the batch, and a copy of it (16-byte aligned whatever the batch did to the row); the gradient of the
                # batch with g = B against the row's with g = 1: g / B is 1 in both
                for one in (logits[b:b + 1], logits[b:b + 1].clone()):
                    _, r1, p1, s1, g1 = run(cdll, one, labels[b:b + 1], p, 1.0)
                    assert same_bits(r1, rows[b:b + 1]) and same_bits(p1, pred[b:b + 1]) and same_bits(s1, saved[b:b + 1]), (name, N, b)
                    assert same_bits(g1, grad_b[b:b + 1]), (name, N, b)
            outs = [raw_forward(lib, logits, labels, p, fill) for fill in (0x00, 0xFF)]
            for a, b_, c in zip(outs[0], outs[1], (loss, rows, pred, saved)):
                assert same_bits(a, b_) and same_bits(a, c), (name, N)
            for fill in (0.0, float('nan')):
                out = torch.full_like(logits, fill)
                assert same_bits(_hip.margin_ce_backward(logits, labels, saved, torch.ones((), device=dev), out=out, cdll=cdll, **p), grad)
            if second_stream:
                stream = torch.cuda.Stream()
                stream.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(stream):
                    other = run(cdll, logits, labels, p, 1.0)
                stream.synchronize()
                for a, b_ in zip(other, (loss, rows, pred, saved, grad)):
                    assert same_bits(a, b_), (name, N)


def check_bad_labels(cdll, dev):
    """labels -1, N and 2^31 - 1: the row and the mean are NaN, every column of the row's gradient is NaN, pred is valid, the other rows are
    what they are with a valid label there, and the columns behind the row (the stride's padding) are untouched"""
    for name in ('ce', 'arm', 'aam', 'subcenter3'):
        p = params(name, 0.1)
        for N in (3, S + 1):
            B, K = 3, p['K']
            logits, base = make_logits(B, N, K, 23 + N, pad=9, device=dev)
            good = make_labels(B, N, 1).to(dev)
            _, rows0, pred0, saved0, grad0 = run(cdll, logits, good, p, 1.0)
            for bad in (-1, N, 2 ** 31 - 1):
                labels = good.clone()
                labels[1] = bad
                out_base = torch.full_like(base, 7.0)
                out = out_base[:, :N * K]
                loss, rows, pred, saved, grad = run(cdll, logits, labels, p, 1.0, out=out)
                assert math.isnan(float(loss)) and math.isnan(float(rows[1])) and bool(torch.isnan(grad[1]).all()), (name, N, bad)
                assert torch.equal(pred, pred0)
                for b in (0, 2):
                    assert same_bits(rows[b], rows0[b]) and same_bits(saved[b], saved0[b]) and same_bits(grad[b], grad0[b]), (name, N, bad, b)
                assert torch.all(out_base[:, N * K:] == 7.0) and torch.all(base[:, N * K:] == 7.0)


def check_nan_logit(cdll, dev):
    for name in ('ce', 'aam', 'subcenter3'):
        p = params(name)
        B, N, K = 3, S + 1, p['K']
        logits, _ = make_logits(B, N, K, 41, device=dev)
        labels = make_labels(B, N, 0).to(dev)
        _, rows0, _, _, grad0 = run(cdll, logits, labels, p, 1.0)
        logits = logits.clone()
        logits[1, (N - 2) * K] = float('nan')
        loss, rows, _, _, grad = run(cdll, logits, labels, p, 1.0)
        assert math.isnan(float(loss)) and math.isnan(float(rows[1]))
        picked = grad[1].reshape(N, K)
        assert bool(torch.isnan(picked).any(dim=1).all())        # the column of every centre that received a gradient
        for b in (0, 2):
            assert same_bits(rows[b], rows0[b]) and same_bits(grad[b], grad0[b])


def check_refusals(cdll, dev):
    """every refusal of include/mvector_hip.h by name; B = 0 touches nothing"""
    lib = cdll or _hip.lib()
    B, N = 2, 6
    x = torch.zeros((B, N), dtype=torch.float32, device=dev)
    y = torch.zeros((B,), dtype=torch.int64, device=dev)
    f = lambda n, dt=torch.float32: torch.zeros((max(n, 1),), dtype=dt, device=dev)
    loss, rows, pred, saved, gout, out = f(1), f(B), f(B, torch.int32), f(B * 4, torch.float64), f(1), torch.zeros_like(x)
    ws = torch.zeros((4096,), dtype=torch.uint8, device=dev)

    def fwd(cfg=None, logits=x, dtype=0, labels=y, B_=B, N_=N, stride=N, loss_=loss, ws_=ws, ws_bytes=4096, null_cfg=False):
        cfg = cfg or _hip.margin_cfg('aam')
        return lib.mv_margin_ce_forward(None if null_cfg else ctypes.byref(cfg), _hip._ptr(logits), dtype, _hip._ptr(labels), B_, N_, stride,
                                        _hip._ptr(loss_), rows.data_ptr(), pred.data_ptr(), saved.data_ptr(), _hip._ptr(ws_), ws_bytes, None)

    def bwd(cfg=None, logits=x, dtype=0, B_=B, N_=N, stride=N, saved_=saved, gout_=gout, out_=out, out_ptr=None, out_stride=N):
        cfg = cfg or _hip.margin_cfg('aam')
        return lib.mv_margin_ce_backward(ctypes.byref(cfg), _hip._ptr(logits), dtype, y.data_ptr(), B_, N_, stride, _hip._ptr(saved_),
                                         _hip._ptr(gout_), out_ptr if out_ptr is not None else _hip._ptr(out_), out_stride, None)

    def refused(rc, text):
        assert rc != 0
        with pytest.raises(RuntimeError, match=text):
            _hip.check(rc, lib)

    assert fwd() == 0 and bwd() == 0
    for call in (fwd, bwd):
        refused(call(B_=-1), 'negative B or N')
        refused(call(N_=-1, stride=0), 'negative B or N')
        refused(call(cfg=_hip.margin_cfg('subcenter', K=0)), 'K outside 1 .. 8')
        refused(call(cfg=_hip.margin_cfg('subcenter', K=9), N_=0, stride=0), 'K outside 1 .. 8')
        refused(call(cfg=_hip.margin_cfg('aam', K=2), N_=3), 'K != 1 with a kind other than MV_LOSS_SUBCENTER')
        refused(call(stride=N - 1), 'stride below N \\* K')
        refused(call(cfg=_hip.margin_cfg('subcenter', K=2), N_=3, stride=5), 'stride below N \\* K')
        for eps in (-0.1, 1.0, float('nan')):
            refused(call(cfg=_hip.margin_cfg('ce', label_smoothing=eps)), 'eps \\(label smoothing\\) outside \\[0, 1\\)')
        refused(call(cfg=_hip.margin_cfg(7)), 'unknown kind')
        refused(call(cfg=_hip.margin_cfg(-1)), 'unknown kind')
        refused(call(dtype=3), 'unknown dtype')
        refused(call(logits=None), 'null logits or labels')
        refused(call(cfg=_hip.margin_cfg('subcenter', K=2), N_=2 ** 30, stride=2 ** 31), 'N \\* K above 2\\^31 - 1')
        refused(call(N_=2 ** 31, stride=2 ** 31), 'N \\* K above 2\\^31 - 1')
        refused(call(stride=2 ** 61), 'B \\* stride beyond int64')
        refused(call(N_=0, stride=0), 'N = 0')
        refused(call(B_=2 ** 31 - 1, N_=2 * S, stride=2 * S), 'B \\* segments above 2\\^31 - 1')
    refused(fwd(null_cfg=True), 'null cfg')
    refused(fwd(labels=None), 'null logits or labels')
    refused(fwd(loss_=None), 'null output')
    refused(fwd(ws_=None), 'null workspace')
    need = int(lib.mv_margin_ce_workspace_bytes(B, N, 1))
    assert need == 64 and lib.mv_margin_ce_workspace_bytes(B, -1, 1) == 0 and lib.mv_margin_ce_workspace_bytes(B, N, 9) == 0
    refused(fwd(ws_bytes=need - 1), 'workspace smaller than mv_margin_ce_workspace_bytes')
    rc = lib.mv_margin_ce_forward(ctypes.byref(_hip.margin_cfg('aam')), x.data_ptr(), 0, y.data_ptr(), B, N, N, loss.data_ptr(), rows.data_ptr(),
                                  pred.data_ptr(), saved.data_ptr(), ws.data_ptr() + 4, 4000, None)
    refused(rc, 'workspace not 16-byte aligned')
    refused(bwd(saved_=None), 'null saved, grad_out or out')
    refused(bwd(gout_=None), 'null saved, grad_out or out')
    refused(bwd(out_=None), 'null saved, grad_out or out')
    refused(bwd(out_stride=N - 1), 'out_stride below N \\* K')
    refused(bwd(out_ptr=x.data_ptr() + 4), 'out overlaps logits')                 # shifted by one element
    refused(bwd(out_ptr=x.data_ptr(), out_stride=N + 1), 'out overlaps logits')   # the same base, another stride
    assert bwd(out_ptr=x.data_ptr()) == 0                                         # in place
    # B = 0: MV_OK with null pointers everywhere, nothing touched
    cfg = _hip.margin_cfg('aam')
    assert lib.mv_margin_ce_forward(ctypes.byref(cfg), None, 0, None, 0, N, N, None, None, None, None, None, 0, None) == 0
    assert lib.mv_margin_ce_backward(ctypes.byref(cfg), None, 0, None, 0, N, N, None, None, None, N, None) == 0
    # the Python wrapper names what it refuses itself
    with pytest.raises(ValueError, match='not one of'):
        _hip.margin_ce_forward(x, y, 'sphere', cdll=cdll)
    with pytest.raises(ValueError, match='2-D fp32, fp16 or bf16'):
        _hip.margin_ce_forward(x.double(), y, 'ce', cdll=cdll)
    with pytest.raises(ValueError, match='no multiple of K'):
        _hip.margin_ce_forward(x[:, :5], y, 'subcenter', K=3, cdll=cdll)
