"""Checks of the batch-hard triplet term (csrc/triplet.hip) shared by tests/test_sphereface2_triplet.py (the emulator build, CPU tensors) and
tests/test_gpu_sphereface2_triplet.py (the product library on the device).  Each takes the bound library (None = the product library) and a
device.

The oracle (``oracle``) is a numpy restatement of the definition in include/mvector_hip.h, fp64 throughout, written densely: the whole [B, B]
matrix, the mined pairs as a sparse matrix G (alpha_i at (i, p_i), beta_i at (i, q_i)) and dF^ = G F^ + G^T F^.

Two conditions on the INPUTS, asserted on the oracle (``assert_conditions``): the best candidate and the runner-up of every mining differ by at
least 1e-9 -- far above the D 2^-52 of either side's sums, so both sides mine the same rows -- and every hinge argument lies at least 1e-6 from
its kink, so both sides take the same branch.  D = 1 with normalize makes every similarity exactly +-1: that is the tie case, it pins "the lower
index wins" and is exempt from the gap condition only.

Bars.  They follow from the arithmetic the kernels chose, never from what they returned.  u = 2^-53.
  * n_i: D squares added in fp64 in some order on either side, (D + 1) u relative, the root 1 u; f^ = f / n one more: f^ is good to (D + 3) u
    relative per side (exact without normalize).  sim_ij adds D products: D u sum_d |f^_id f^_jd| per side on top of the factors' errors.  So
        mined bar = (D + 8) 2^-50 S_ij,  S_ij = sum_d |f^_id f^_jd|        (8 (D + 8) u >= 2 (3 D + 7) u)
    below the cap 2^-20 max(|value|, 1) (S <= 1 with normalize; for randn rows of 2047 columns S is about 1300 and the bar 2e-9).
  * loss: every term moves by at most its mined values' bars; three sums of B terms and four more operations, rounded ONCE to fp32:
        loss bar = 2^-24 |loss| + (1 + weight) mean_i (bar_ap + bar_an) + (B + 8) u (mean rank + weight (mean over + mean short)).
  * gradient: dF^_id is a sum of a few coefficient * f^ terms; with A_id = sum of their magnitudes it is good to (D + 8) u A_id per side (the
    coefficients carry 2 u).  The projection takes a dot product of D terms: its error is (D + 8) u sum_d A_id |f^_id|, and
    df = (dF^ - dot f^) / n adds four operations.  So, per side generous by a factor of four again,
        grad bar = eps |grad_ref| + tiny + |g| (D + 16) 2^-50 (A_id + |f^_id| sum_d A_id |f^_id|) / n_i
    (without normalize the second summand and n drop out), eps the rounding of the features' dtype: 2^-24 (fp32), 2^-11 (fp16), 2^-8 (bf16),
    tiny half its smallest subnormal.  For fp32 the bar is asserted to stay below the cap 2^-16 |g| (A_id + ...) / n_i + eps |grad_ref|, the
    form tests/margin_loss_checks.py asserts: 2^-16 of the per-element weight.  A 16-bit gradient cannot fit under a 2^-16 cap -- the dtype's own
    rounding is 2^-11 or 2^-8 -- so there only the fp64 part of the bar is held against the cap and the rounding is the dtype's, once."""
import ctypes
import math

import numpy as np
import pytest
import torch

from mvector import _hip

U50 = 2.0 ** -50
SHAPES = ((2, 1), (3, 5), (7, 24), (64, 192), (257, 513), (12, 2047))
SEEDS = (0, 1, 2)
PATTERNS = ('pairs', 'singleton', 'different', 'same')
EPS = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
TINY = {torch.float32: 2.0 ** -150, torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -134}


def params(normalize=True, add_absolute=True):
    return dict(margin=0.5, normalize=normalize, add_absolute=add_absolute, absolute_loss_weight=0.7, ap_value=0.8, an_value=0.4)


def make_features(B, D, seed, dtype=torch.float32, pad=0, device='cpu'):
    """randn features with a row stride of D + pad; the pad columns hold a sentinel no kernel may touch.  Returns the view and its base."""
    g = torch.Generator().manual_seed(seed)
    base = torch.full((B, D + pad), 7.0, dtype=torch.float32)
    base[:, :D] = torch.randn(B, D, generator=g)
    base = base.to(dtype).to(device)
    return base[:, :D], base


def make_labels(B, pattern):
    """pairs (0 0 1 1 ..); pairs with the last row a class of its own; all different; all the same (no negative anywhere).  The values are
    scattered over int64: the kernels compare labels, they do not index with them."""
    i = torch.arange(B, dtype=torch.int64)
    if pattern == 'pairs':
        y = i // 2
    elif pattern == 'singleton':
        y = i // 2
        y[B - 1] = B
    elif pattern == 'different':
        y = i
    else:
        y = torch.zeros(B, dtype=torch.int64)
    return y * 1_000_003 - 7


# ------------------------------------------------------------------------------------------------ the oracle
def oracle(features, labels, p, g=1.0, dtype=torch.float32):
    """features: numpy float64 [B, D] (the upcast values); labels int64 [B] -> dict of the definition's quantities and their bars"""
    f = np.asarray(features, dtype=np.float64)
    B, D = f.shape
    w = float(p['absolute_loss_weight']) if p['add_absolute'] else 0.0
    with np.errstate(invalid='ignore', divide='ignore'):
        n = np.sqrt((f * f).sum(axis=1))
        fh = f / n[:, None] if p['normalize'] else f
        sim = fh @ fh.T
        S = np.abs(fh) @ np.abs(fh).T
        same = labels[:, None] == labels[None, :]
        pos = np.where(same, sim, np.inf)
        neg = np.where(same, -np.inf, sim)
        pi = np.argmin(pos, axis=1)                      # the first occurrence: the lower index wins ties
        qi = np.argmax(neg, axis=1)
        has_neg = (~same).any(axis=1)
        rows = np.arange(B)
        ap, an = pos[rows, pi], np.where(has_neg, neg[rows, qi], -np.inf)
        qi = np.where(has_neg, qi, -1)
        arg = p['margin'] - (ap - an)
        rank = np.where(arg < 0, 0.0, arg)
        short_arg, over_arg = p['ap_value'] - ap, an - p['an_value']
        short = np.where(short_arg > 0, short_arg, 0.0)
        over = np.where(over_arg > 0, over_arg, 1.0)
        loss = rank.mean() + (w * (over.mean() + short.mean()) if p['add_absolute'] else 0.0)
        on = (arg >= 0).astype(np.float64)
        alpha = -on / B - (w / B) * (short_arg > 0)
        beta = on / B + (w / B) * (over_arg > 0)
        G = np.zeros((B, B))
        G[rows, pi] += alpha
        G[rows[has_neg], qi[has_neg]] += beta[has_neg]
        Ga = np.zeros((B, B))
        Ga[rows, pi] += np.abs(alpha)
        Ga[rows[has_neg], qi[has_neg]] += np.abs(beta[has_neg])
        dfh = G @ fh + G.T @ fh
        A = Ga @ np.abs(fh) + Ga.T @ np.abs(fh)
        if p['normalize']:
            grad = (dfh - (dfh * fh).sum(axis=1, keepdims=True) * fh) / n[:, None]
            weight = (A + np.abs(fh) * (A * np.abs(fh)).sum(axis=1, keepdims=True)) / n[:, None]
        else:
            grad, weight = dfh, A
        grad, weight = g * grad, abs(g) * weight
        bar_ap = (D + 8) * U50 * S[rows, pi]
        bar_an = np.where(has_neg, (D + 8) * U50 * S[rows, np.maximum(qi, 0)], 0.0)
        terms = rank.mean() + w * (np.where(np.isfinite(over), over, 0).mean() + short.mean())
    return dict(n=n, fh=fh, sim=sim, pos=pos, neg=neg, has_neg=has_neg, index=np.stack([pi, qi], axis=1).astype(np.int32),
                mined=np.stack([ap, an], axis=1), mined_bar=np.stack([bar_ap, bar_an], axis=1),
                mined_cap=2.0 ** -20 * np.maximum(np.abs(np.stack([ap, np.where(has_neg, an, 0.0)], axis=1)), 1.0),
                args=(arg, short_arg, over_arg), loss=loss,
                loss_bar=2.0 ** -24 * abs(loss) + (1.0 + w) * (bar_ap + bar_an).mean() + (B + 8) * 2.0 ** -53 * terms,
                grad=grad, grad_bar=EPS[dtype] * np.abs(grad) + TINY[dtype] + (D + 16) * U50 * weight,
                grad_bar64=(D + 16) * U50 * weight, grad_cap=2.0 ** -16 * weight)


def assert_conditions(ref, p, tie_case=False):
    """the two conditions on the inputs (module docstring)"""
    if not tie_case:
        for cand, best in ((ref['pos'], np.min), (ref['neg'], np.max)):
            for i in range(cand.shape[0]):
                row = np.sort(cand[i][np.isfinite(cand[i])])
                if row.size >= 2:
                    gap = row[1] - row[0] if best is np.min else row[-1] - row[-2]
                    assert gap >= 1e-9, (i, gap)
    arg, short_arg, over_arg = ref['args']
    kinks = [arg[np.isfinite(arg)]]
    if p['add_absolute']:
        kinks += [short_arg, over_arg[np.isfinite(over_arg)]]
    for k in kinks:
        assert np.all(np.abs(k) >= 1e-6), np.abs(k).min()


def run(cdll, features, labels, p, g=1.0):
    loss, mined, index = _hip.triplet_forward(features, labels, cdll=cdll, **p)
    gt = torch.tensor(g, dtype=torch.float32, device=features.device)
    grad = _hip.triplet_backward(features, labels, mined, index, gt, cdll=cdll, **p)
    return loss, mined, index, grad


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.bfloat16:
        a, b = a.view(torch.int16), b.view(torch.int16)
    return a.numpy().tobytes() == b.numpy().tobytes()


# ------------------------------------------------------------------------------------------------ the checks
def check_case(cdll, dev, B, D, seed, pattern, normalize, add_absolute, dtype=torch.float32, pad=0, g=0.75, report=None):
    p = params(normalize, add_absolute)
    features, base = make_features(B, D, seed, dtype=dtype, pad=pad, device=dev)
    labels = make_labels(B, pattern)
    loss, mined, index, grad = run(cdll, features, labels.to(dev), p, g)
    ref = oracle(features.cpu().double().numpy(), labels.numpy(), p, g, dtype)
    tie_case = D == 1 and normalize
    assert_conditions(ref, p, tie_case)
    what = (B, D, seed, pattern, normalize, add_absolute, dtype)
    index, mined = index.cpu().numpy(), mined.cpu().numpy()
    assert np.array_equal(index, ref['index']), (what, index, ref['index'])
    if pattern == 'same':
        assert np.all(index[:, 1] == -1) and np.all(mined[:, 1] == -np.inf)
    finite = np.isfinite(ref['mined'])
    assert np.all(ref['mined_bar'] <= ref['mined_cap']) and np.all(ref['grad_bar64'] <= ref['grad_cap'] + 1e-300)
    with np.errstate(invalid='ignore'):
        mined_err = np.abs(np.where(finite, mined - ref['mined'], 0.0))
    assert np.array_equal(np.isfinite(mined), finite) and np.all(mined_err <= ref['mined_bar']), (what, mined_err.max())
    if tie_case:
        assert np.all(np.abs(mined[finite]) == 1.0)      # the tie case is exact
    # sim_ij and sim_ji are the same bits: two rows that mined each other hold the same value
    for col in (0, 1):
        for i in range(B):
            j = index[i, col]
            if j >= 0 and j != i and index[j, col] == i:
                assert mined[i, col].tobytes() == mined[j, col].tobytes(), (what, i, j, col)
    loss_err = abs(float(loss) - ref['loss'])
    assert loss_err <= ref['loss_bar'], (what, loss_err, ref['loss_bar'])
    assert grad.dtype == dtype and grad.shape == (B, D)
    grad_err = np.abs(grad.cpu().double().numpy() - ref['grad'])
    assert np.all(grad_err <= ref['grad_bar']), (what, (grad_err / ref['grad_bar']).max())
    if pad:
        assert torch.all(base[:, D:] == 7.0)
    if report is not None:
        report.append((what, float((mined_err / ref['mined_cap']).max()), loss_err / max(abs(ref['loss']), 1.0),
                       float((grad_err / (ref['grad_cap'] + EPS[dtype] * np.abs(ref['grad']) + TINY[dtype])).max())))
    return ref


def print_report(report):
    print('\n(B, D, seed, labels, normalize, add_absolute, dtype): mined error / cap, loss rel. error, gradient error / (cap + the dtype\'s rounding and subnormal step)')
    for r in report:
        print(f'  {r[0]}: {r[1]:.3g}  {r[2]:.3g}  {r[3]:.3g}')


def check_shape(cdll, dev, B, D, seeds=SEEDS, patterns=PATTERNS, normalizes=(True, False), halves=(torch.float16, torch.bfloat16)):
    """one (B, D): every seed, label pattern and normalize in fp32, add_absolute taking turns; the 16-bit dtypes on seed 0 with pairs (normalised)
    and with one singleton class (not normalised)"""
    report = []
    for seed in seeds:
        for pattern in patterns:
            k = PATTERNS.index(pattern)
            for normalize in normalizes:
                check_case(cdll, dev, B, D, seed, pattern, normalize, bool((seed + k + normalize) % 2), pad=(3 if seed == 1 else 0), report=report)
    for dtype in halves:
        for pattern in patterns:
            if pattern in ('pairs', 'singleton'):
                check_case(cdll, dev, B, D, 0, pattern, pattern == 'pairs', True, dtype=dtype, report=report)
    print_report(report)


def check_against_torch_autograd():
    """the oracle itself against autograd through the package's torch expression in fp64 (its cross-entropy taken off again)"""
    from mvector.loss import TripletAngularMarginLoss
    for B, D in ((7, 24), (64, 192)):
        for pattern in PATTERNS:
            for normalize in (True, False):
                p = params(normalize, True)
                features, _ = make_features(B, D, 1)
                idx = torch.from_numpy(np.unique(make_labels(B, pattern).numpy(), return_inverse=True)[1])   # the same classes, as columns
                ref = oracle(features.double().numpy(), idx.numpy(), p, 1.0)
                module = TripletAngularMarginLoss(margin=p['margin'], normalize_feature=normalize, add_absolute=True,
                                                  absolute_loss_weight=p['absolute_loss_weight'], ap_value=p['ap_value'], an_value=p['an_value'])
                x = features.double().requires_grad_(True)
                logits = torch.zeros((B, int(idx.max()) + 1), dtype=torch.float64)
                loss = module({'features': x, 'logits': logits}, idx) - torch.nn.functional.cross_entropy(logits, idx)
                loss.backward()
                assert abs(float(loss.detach()) - ref['loss']) <= 1e-12 * max(1.0, abs(ref['loss'])), (B, D, pattern, normalize)
                assert np.all(np.abs(x.grad.numpy() - ref['grad']) <= 1e-12 * np.maximum(1.0, np.abs(ref['grad']))), (B, D, pattern, normalize)


def check_no_hidden_state(cdll, dev, second_stream=False):
    """outputs and workspace pre-filled with 0xFF or zeros give the same bits; a second call gives the first call's; on the device a second stream"""
    lib = cdll or _hip.lib()
    p = params()
    cfg = _hip.triplet_cfg(**p)
    for B, D in ((7, 24), (64, 192)):
        features, _ = make_features(B, D, 0, device=dev)
        labels = make_labels(B, 'pairs').to(dev)
        want = run(cdll, features, labels, p, 1.0)
        outs = []
        for fill in (0x00, 0xFF):
            mk = lambda n: torch.full((n,), fill, dtype=torch.uint8, device=dev)
            nbytes = int(lib.mv_triplet_workspace_bytes(B, D))
            loss, mined, index, ws, out = mk(4), mk(16 * B), mk(8 * B), mk(nbytes), mk(4 * B * D)
            _hip.check(lib.mv_triplet_forward(ctypes.byref(cfg), features.data_ptr(), 0, labels.data_ptr(), B, D, D, loss.data_ptr(),
                                              mined.data_ptr(), index.data_ptr(), ws.data_ptr(), nbytes, _hip.current_stream(features)), lib)
            ws.fill_(fill)
            gt = torch.ones((1,), dtype=torch.float32, device=dev)
            _hip.check(lib.mv_triplet_backward(ctypes.byref(cfg), features.data_ptr(), 0, B, D, D, mined.data_ptr(), index.data_ptr(),
                                               gt.data_ptr(), out.data_ptr(), D, ws.data_ptr(), nbytes, _hip.current_stream(features)), lib)
            outs.append((loss.view(torch.float32)[0], mined.view(torch.float64).reshape(B, 2), index.view(torch.int32).reshape(B, 2),
                         out.view(torch.float32).reshape(B, D)))
        for a, b_, c in zip(outs[0], outs[1], want):
            assert same_bits(a, b_) and same_bits(a, c), (B, D)
        if second_stream:
            stream = torch.cuda.Stream()
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                other = run(cdll, features, labels, p, 1.0)
            stream.synchronize()
            for a, b_ in zip(other, want):
                assert same_bits(a, b_), (B, D)


def check_zero_norm_row(cdll, dev):
    """a row of zeros: with normalize it is 0 / 0 -- the loss and, as in the torch expression's dense products, every gradient row are NaN, and
    nothing is read out of bounds; without normalize it is a row like any other"""
    from mvector.loss import TripletAngularMarginLoss
    B, D = 7, 24
    labels = make_labels(B, 'pairs')
    features, base = make_features(B, D, 0, pad=3, device=dev)
    features[2] = 0.0
    p = params(True, True)
    loss, mined, index, grad = run(cdll, features, labels.to(dev), p, 1.0)
    x = features.cpu().double().requires_grad_(True)
    module = TripletAngularMarginLoss(absolute_loss_weight=0.7)
    idx = torch.arange(B) // 2
    ref_loss = module({'features': x, 'logits': torch.zeros((B, 4), dtype=torch.float64)}, idx)
    ref_loss.backward()
    assert math.isnan(float(ref_loss.detach())) and bool(torch.isnan(x.grad).all())
    assert math.isnan(float(loss)) and bool(torch.isnan(grad).all()) and bool(torch.isnan(mined).any(dim=1).all())
    assert int(index.min()) >= -1 and int(index.max()) < B and torch.all(base[:, D:] == 7.0)
    p = params(False, True)
    ref = oracle(features.cpu().double().numpy(), labels.numpy(), p, 1.0)
    assert_conditions(ref, p, tie_case=True)     # every similarity of the zero row is 0: a tie, the lower index wins
    loss, mined, index, grad = run(cdll, features, labels.to(dev), p, 1.0)
    assert np.array_equal(index.cpu().numpy(), ref['index']) and abs(float(loss) - ref['loss']) <= ref['loss_bar']
    assert np.all(np.abs(grad.cpu().double().numpy() - ref['grad']) <= ref['grad_bar'])


def check_refusals(cdll, dev):
    """every refusal of include/mvector_hip.h by name; B = 0 touches nothing"""
    lib = cdll or _hip.lib()
    B, D = 4, 6
    x = torch.ones((B, D), dtype=torch.float32, device=dev)
    y = torch.zeros((B,), dtype=torch.int64, device=dev)
    loss = torch.zeros((1,), dtype=torch.float32, device=dev)
    mined = torch.zeros((B, 2), dtype=torch.float64, device=dev)
    index = torch.zeros((B, 2), dtype=torch.int32, device=dev)
    gout, out = torch.ones((1,), dtype=torch.float32, device=dev), torch.zeros_like(x)
    ws = torch.zeros((4096,), dtype=torch.uint8, device=dev)
    cfg = _hip.triplet_cfg()

    def fwd(x_=x, dtype=0, y_=y, B_=B, D_=D, stride=D, loss_=loss, ws_=ws, ws_bytes=4096, null_cfg=False):
        return lib.mv_triplet_forward(None if null_cfg else ctypes.byref(cfg), _hip._ptr(x_), dtype, _hip._ptr(y_), B_, D_, stride,
                                      _hip._ptr(loss_), mined.data_ptr(), index.data_ptr(), _hip._ptr(ws_), ws_bytes, None)

    def bwd(x_=x, dtype=0, B_=B, D_=D, stride=D, mined_=mined, gout_=gout, out_=out, out_ptr=None, out_stride=D, ws_=ws, ws_bytes=4096,
            null_cfg=False):
        return lib.mv_triplet_backward(None if null_cfg else ctypes.byref(cfg), _hip._ptr(x_), dtype, B_, D_, stride, _hip._ptr(mined_),
                                       index.data_ptr(), _hip._ptr(gout_), out_ptr if out_ptr is not None else _hip._ptr(out_), out_stride,
                                       _hip._ptr(ws_), ws_bytes, None)

    def refused(rc, text):
        assert rc != 0
        with pytest.raises(RuntimeError, match=text):
            _hip.check(rc, lib)

    assert fwd() == 0 and bwd() == 0
    need = int(lib.mv_triplet_workspace_bytes(B, D))
    assert need == (2 * B * D + B) * 8 and lib.mv_triplet_workspace_bytes(4097, D) == 0 and lib.mv_triplet_workspace_bytes(B, 2049) == 0
    assert lib.mv_triplet_workspace_bytes(4096, 2048) == (2 * 4096 * 2048 + 4096) * 8 and lib.mv_triplet_workspace_bytes(B, 0) == 0
    for call in (fwd, bwd):
        refused(call(null_cfg=True), 'null cfg')
        refused(call(B_=-1), 'negative B or D')
        refused(call(D_=-1), 'negative B or D')
        refused(call(dtype=3), 'unknown dtype')
        refused(call(B_=4097), 'B above MV_TRIPLET_MAX_B')
        refused(call(D_=0, stride=0), 'D outside 1 .. MV_TRIPLET_MAX_D')
        refused(call(D_=2049, stride=2049), 'D outside 1 .. MV_TRIPLET_MAX_D')
        refused(call(stride=D - 1), 'stride below D')
        refused(call(stride=2 ** 61), 'B \\* stride beyond int64')
        refused(call(x_=None), 'null features')
        refused(call(ws_=None), 'null workspace')
        refused(call(ws_bytes=need - 1), 'workspace smaller than mv_triplet_workspace_bytes')
    refused(fwd(y_=None), 'null features or labels')
    refused(fwd(loss_=None), 'null output')
    refused(lib.mv_triplet_forward(ctypes.byref(cfg), x.data_ptr(), 0, y.data_ptr(), B, D, D, loss.data_ptr(), mined.data_ptr(), index.data_ptr(),
                                   ws.data_ptr() + 4, 4000, None), 'workspace not 16-byte aligned')
    refused(bwd(mined_=None), 'null mined, index, grad_out or out')
    refused(bwd(gout_=None), 'null mined, index, grad_out or out')
    refused(bwd(out_=None), 'null mined, index, grad_out or out')
    refused(bwd(out_stride=D - 1), 'out_stride below D')
    refused(bwd(out_stride=2 ** 61), 'B \\* out_stride beyond int64')
    refused(bwd(out_ptr=x.data_ptr()), 'out overlaps features')
    refused(bwd(out_ptr=x.data_ptr() + 4 * (B * D - 1)), 'out overlaps features')
    # an index the forward never writes: the row is NaN, nothing is read through it
    index[1, 0], index[2, 1] = B, -2
    assert bwd() == 0 and bool(torch.isnan(out[1]).all()) and bool(torch.isnan(out[2]).all()) and bool(torch.isfinite(out[0]).all())
    index.zero_()
    # B = 0: MV_OK with null pointers everywhere, nothing touched
    assert lib.mv_triplet_forward(ctypes.byref(cfg), None, 0, None, 0, D, D, None, None, None, None, 0, None) == 0
    assert lib.mv_triplet_backward(ctypes.byref(cfg), None, 0, 0, D, D, None, None, None, None, D, None, 0, None) == 0
    with pytest.raises(ValueError, match='2-D fp32, fp16 or bf16'):
        _hip.triplet_forward(x.double(), y, cdll=cdll)
    with pytest.raises(ValueError, match='labels must have shape'):
        _hip.triplet_forward(x, y[:2], cdll=cdll)


def check_golden(cdll, dev, golden):
    """the native calls on the inputs of tests/golden/margin_loss.npz against the reference's fp64 results: the triplet term at the bar of its
    oracle, the cross-entropy (mv_margin_ce_forward, kind CE) at the bar tests/margin_loss_checks.py derives for it"""
    import margin_loss_checks as mlc
    features = torch.from_numpy(golden['features']).to(dev)
    logits = torch.from_numpy(golden['logits']).to(dev)
    labels = torch.from_numpy(golden['labels'])
    print()
    for case in ('triplet_ls0', 'triplet_ls1'):
        args = golden[case + '.args']
        p = dict(margin=float(args[0]), normalize=True, add_absolute=True, absolute_loss_weight=float(args[1]), ap_value=float(args[2]),
                 an_value=float(args[3]))
        ce_p = dict(kind='ce', margin=0.0, scale=1.0, easy_margin=False, K=1, label_smoothing=float(args[4]))
        loss, mined, index, grad = run(cdll, features, labels.to(dev), p, 1.0)
        ce, _, _, saved = _hip.margin_ce_forward(logits, labels.to(dev), cdll=cdll, **ce_p)
        ce_grad = _hip.margin_ce_backward(logits, labels.to(dev), saved, torch.ones((), device=dev), cdll=cdll, **ce_p)
        ref = oracle(golden['features'].astype(np.float64), golden['labels'], p, 1.0)
        assert_conditions(ref, p)
        ce_ref = mlc.oracle(golden['logits'], golden['labels'], ce_p, 1.0)
        total = float(loss + ce)
        # the label smoothing reaches the cross-entropy kernels as a float: eps 2^-24 of it on q_j, and on the two terms of the row loss
        eps_q = ce_p['label_smoothing'] * 2.0 ** -24
        eps_loss = eps_q * (np.abs(ce_ref['lse'] - ce_ref['zy']) + np.abs(ce_ref['lse'] - ce_ref['meanz'])).mean()
        bar = ref['loss_bar'] + ce_ref['loss_bar'] + eps_loss + 2.0 ** -24 * abs(total)
        ce_grad_bar = ce_ref['grad_bar'] + eps_q / len(golden['labels'])
        d_loss = abs(total - float(golden[case + '.loss']))
        d_feat = np.abs(grad.cpu().double().numpy() - golden[case + '.grad_features'])
        d_logit = np.abs(ce_grad.cpu().double().numpy() - golden[case + '.grad'])
        print(f'  {case}: |loss - golden| {d_loss:.3g} (bar {bar:.3g}); max |grad_features - golden| / bar {(d_feat / ref["grad_bar"]).max():.3g}; '
              f'max |grad - golden| / bar {(d_logit / ce_grad_bar).max():.3g}')
        assert d_loss <= bar and np.all(d_feat <= ref['grad_bar']) and np.all(d_logit <= ce_grad_bar), case
