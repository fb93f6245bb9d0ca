"""Checks of the cohort score normalisation (csrc/scorenorm.hip) shared by tests/test_score_norm.py (the emulator build, CPU tensors) and
tests/test_gpu_score_norm.py (the product library on the device).  Each takes the bound library (None = the product library) and a device.

Statistics.  The oracle takes the fp32 cohort scores from ``_hip.cosine`` of the SAME library, selects the min(top_n, m) largest per row by the
order key (-0 and +0 one value, every NaN above +inf, equal keys by the lower cohort row) and computes mean and population std in numpy fp64.
The bar is derived, not measured: |got - ref| <= 2^-23 |ref| + b.
  * 2^-23 |ref| covers the one rounding to fp32 (2^-24 relative) with a factor two to spare.
  * b is the fp64 accumulation bound of library and oracle together.  A sum of N' terms in any order is off by at most (N' - 1) 2^-53 sum|x|;
    two such sums differ by at most N' 2^-52 max|x| after the division by N'.  So b_mean = N' 2^-52 max|x|.
  * std: with dmax = max|x - mean| <= 2 max|x|, an error e in the mean moves every square by at most 2 dmax e, and summing N' squares adds
    N' 2^-52 dmax^2 / N' after the division; the square root divides the error of the variance by 2 std:
    b_std = (2 dmax b_mean + N' 2^-52 dmax^2) / (2 std).
The inputs are chosen (seeds searched on the CPU, in fp64) so that every reference std is >= 1e-3; b is then asserted below 2^-26 |ref|, a
quarter of an fp32 ulp, when the reference is built.  Where a NaN is selected both must be NaN.

Normalisation.  ``==`` on the float bits against the numpy.float32 expression (NaNs match as NaNs)."""
import functools

import numpy as np
import pytest
import torch

from helpers import load_case
from oracle import frontend
from search_checks import keys_of

TIERS = (4096, 12288)   # the last m of the two lower LDS tiers of cohort_topn_stats_kernel (csrc/scorenorm.hip: CS_TIER_SMALL, CS_TIER_MID)
# (n, m, dim, top_n): the smallest valid call; small cohort, small top_n; top_n == m; one entry below the cut; top_n > m; the typical AS-norm
# shape; one key behind a tier (and segment) edge; the last and first m of every tier
CASES = ((1, 2, 1, 2), (3, 17, 192, 5), (17, 300, 192, 300), (5, 301, 64, 300), (4, 100, 192, 300), (2, 1000, 192, 300), (2, 4097, 16, 300),
         (2, TIERS[0], 16, 300), (2, TIERS[1], 8, 300), (2, TIERS[1] + 1, 8, 300))
DEVICE_CASES = ((2, 32768, 8, 400),)   # the largest cohort
EPS32, EPS64 = 2.0 ** -23, 2.0 ** -52


# ------------------------------------------------------------------------------------------------ oracle
def top_values(cos, top_n):
    """[n, m] fp32 scores -> [n, N'] the selected scores per row, best first (key descending, then the lower column)"""
    n, m = cos.shape
    key = keys_of(cos).astype(np.int64)
    order = np.argsort(-key, axis=1, kind='stable')[:, :min(top_n, m)]
    return np.take_along_axis(cos, order, axis=1)


def reference_stats(cos, top_n, need_std=1e-3):
    """-> (mean, std, b_mean, b_std) in fp64 per row; rows with a NaN among the selected scores have NaN everywhere"""
    kept = top_values(cos, top_n).astype(np.float64)
    np_ = kept.shape[1]
    with np.errstate(invalid='ignore'):
        mean, std = kept.mean(axis=1), kept.std(axis=1)
        xmax = np.abs(kept).max(axis=1)
        dmax = np.abs(kept - mean[:, None]).max(axis=1)
        b_mean = np_ * EPS64 * xmax
        b_std = (2 * dmax * b_mean + np_ * EPS64 * dmax ** 2) / (2 * std)
    ok = ~np.isnan(mean)
    if need_std is not None:
        assert (std[ok] >= need_std).all(), f'a reference std below {need_std}: {std[ok].min()}'
        assert (b_mean[ok] <= 2.0 ** -26 * np.abs(mean[ok]) + 1e-12).all() and (b_std[ok] <= 2.0 ** -26 * std[ok]).all(), 'the fp64 bound is not far below an fp32 ulp'
    return mean, std, b_mean, b_std


def assert_stats(got, ref, what=''):
    (gm, gs), (mean, std, b_mean, b_std) = got, ref
    assert gm.dtype == np.float32 and gs.dtype == np.float32 and gm.shape == mean.shape and gs.shape == std.shape, what
    nan = np.isnan(mean)
    assert np.array_equal(np.isnan(gm), nan) and np.array_equal(np.isnan(gs), nan), f'{what}: NaN rows differ'
    with np.errstate(invalid='ignore'):
        em, es = np.abs(gm.astype(np.float64) - mean), np.abs(gs.astype(np.float64) - std)
        bad_m = ~nan & ~(em <= EPS32 * np.abs(mean) + b_mean)
        bad_s = ~nan & ~(es <= EPS32 * np.abs(std) + np.where(np.isfinite(b_std), b_std, 0.0))
    assert not bad_m.any(), f'{what}: mean off in rows {np.flatnonzero(bad_m)[:4].tolist()}: {em[bad_m][:4]}'
    assert not bad_s.any(), f'{what}: std off in rows {np.flatnonzero(bad_s)[:4].tolist()}: {es[bad_s][:4]}'


# ------------------------------------------------------------------------------------------------ data
def _randn(n, m, dim, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, dim, generator=g), torch.randn(m, dim, generator=g)


@functools.lru_cache(maxsize=None)
def seed_for(n, m, dim, top_n):
    """the first seed from the case's base on whose fp64 cosines give every row a top-N' std of at least 2e-3 (dim 1 has scores of +-1 only:
    a seed is needed whose two cohort values differ in sign)"""
    for seed in range(2000 + n + m + dim + top_n, 2100 + n + m + dim + top_n):
        x, c = (t.numpy().astype(np.float64) for t in _randn(n, m, dim, seed))
        cos = (x / np.linalg.norm(x, axis=1, keepdims=True)) @ (c / np.linalg.norm(c, axis=1, keepdims=True)).T
        if np.sort(cos, axis=1)[:, -min(top_n, m):].std(axis=1).min() >= 2e-3:
            return seed
    raise AssertionError('no seed with a reference std >= 2e-3')


def data(n, m, dim, top_n, device):
    x, c = _randn(n, m, dim, seed_for(n, m, dim, top_n))
    return x.to(device), c.to(device)


def stats(cdll, x, cohort, top_n, hint=0):
    from mvector import _hip
    mean, std = _hip.cohort_stats(x, cohort, top_n, rows_hint=hint, cdll=cdll)
    assert mean.device == x.device and std.device == x.device and mean.shape == (x.shape[0],) and std.shape == (x.shape[0],)
    return mean.cpu().numpy(), std.cpu().numpy()


def cos_matrix(cdll, x, cohort):
    from mvector import _hip
    return _hip.cosine(x, cohort, cdll=cdll).cpu().numpy()


def same_bits(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ------------------------------------------------------------------------------------------------ statistics
def check_stats_case(cdll, device, n, m, dim, top_n):
    x, cohort = data(n, m, dim, top_n, device)
    ref = reference_stats(cos_matrix(cdll, x, cohort), top_n)
    first = None
    for hint in dict.fromkeys((0, 1, 3, n)):
        got = stats(cdll, x, cohort, top_n, hint)
        assert_stats(got, ref, f'({n}, {m}, {dim}, {top_n}) rows_hint {hint}')
        first = first or got
        assert same_bits(got, first), f'({n}, {m}, {dim}, {top_n}): rows_hint {hint} gives other bits than rows_hint 0'
    return first, ref


@functools.lru_cache(maxsize=None)
def _tie_data(m, base, top_n):
    """3 embeddings and a cohort of m rows drawn from ``base`` distinct ones; the seed is searched on the CPU (fp64 cosines) so that every
    row's top-N' std is at least 2e-3 -- two groups whose scores nearly agree would leave a std that the bar's b term cannot serve"""
    for seed in range(41, 141):
        g = torch.Generator().manual_seed(seed)
        rows = torch.randn(base, 48, generator=g)
        cohort = rows[torch.randint(0, base, (m,), generator=g)].contiguous()
        x = torch.randn(3, 48, generator=g)
        a, b = x.numpy().astype(np.float64), cohort.numpy().astype(np.float64)
        cos = (a / np.linalg.norm(a, axis=1, keepdims=True)) @ (b / np.linalg.norm(b, axis=1, keepdims=True)).T
        if np.sort(cos, axis=1)[:, -top_n:].std(axis=1).min() >= 2e-3:
            return x, cohort
    raise AssertionError('no seed with a reference std >= 2e-3')


def check_ties(cdll, device):
    """cohorts of bit-identical copies of a few rows: the copies score bit-equal, so the cut key is shared by many entries scattered over the
    threads' segments and over the tier edge"""
    g = torch.Generator().manual_seed(41)
    for m, base, top_n in ((700, 5, 300), (4500, 7, 1000), (257, 2, 150)):   # (the selection spans more than one group: the std is not 0)
        x, cohort = (t.to(device) for t in _tie_data(m, base, top_n))
        cos = cos_matrix(cdll, x, cohort)
        for r in range(3):
            assert len(np.unique(cos[r])) <= base, 'copies of a cohort row do not score bit-equal'
        kept = top_values(cos, top_n)
        assert (np.sum(cos == kept[:, -1:], axis=1) > np.sum(kept == kept[:, -1:], axis=1)).all(), 'the cut does not fall inside a group of equal scores'
        ref = reference_stats(cos, top_n)
        for hint in (0, 2):
            assert_stats(stats(cdll, x, cohort, top_n, hint), ref, f'ties, m {m}, rows_hint {hint}')
    # one row repeated: N' copies of one value v -> mean == v and std == 0 exactly
    for m, top_n in ((40, 300), (700, 300), (5000, 300)):
        cohort = torch.randn(1, 48, generator=g).repeat(m, 1).to(device)
        x = torch.randn(4, 48, generator=g).to(device)
        cos = cos_matrix(cdll, x, cohort)
        assert (cos == cos[:, :1]).all()
        mean, std = stats(cdll, x, cohort, top_n)
        assert np.array_equal(mean, cos[:, 0]) and np.array_equal(std, np.zeros(4, dtype=np.float32)), (m, mean, cos[:, 0], std)


def check_special_values(cdll, device):
    g = torch.Generator().manual_seed(5)
    n, m, dim, top_n = 4, 60, 16, 20
    x, cohort = torch.randn(n, dim, generator=g), torch.randn(m, dim, generator=g)
    cohort[7] = 0.0                       # a zero cohort row: mv_cosine_f32 gives 0 for it
    x[2] = float('nan')
    x, cohort = x.to(device), cohort.to(device)
    cos = cos_matrix(cdll, x, cohort)
    assert np.isnan(cos[2]).all() and (cos[[0, 1, 3], 7] == 0).all()
    ref = reference_stats(cos, top_n)
    got = stats(cdll, x, cohort, top_n)
    assert_stats(got, ref, 'a NaN embedding row')
    assert np.isnan(got[0]).tolist() == [False, False, True, False] and np.isnan(got[1]).tolist() == [False, False, True, False]
    # the zero row inside the selection (top_n == m) and +-0 scores: a cohort of zero rows and the negated embedding
    got = stats(cdll, x, cohort, m)
    assert_stats(got, reference_stats(cos, m), 'top_n == m with a zero cohort row')
    zeros = torch.zeros(5, dim, device=device)
    mean, std = stats(cdll, x[:2], zeros, 3)
    assert (mean == 0).all() and (std == 0).all()
    signed = torch.cat([zeros, x[:1], -x[:1]])
    cos2 = cos_matrix(cdll, x[:2], signed)
    assert_stats(stats(cdll, x[:2], signed, 4), reference_stats(cos2, 4, need_std=None), 'zero scores inside the selection')
    # a NaN cohort row ranks on top of every selection: every row comes out NaN
    bad = cohort.clone()
    bad[11, 3] = float('nan')
    mean, std = stats(cdll, x, bad, top_n)
    assert np.isnan(mean).all() and np.isnan(std).all()
    # no rows: nothing is touched
    from mvector import _hip
    lib = cdll or _hip.lib()
    out = torch.full((64,), 0xFF, dtype=torch.uint8, device=device)
    ws = torch.full((64,), 0xFF, dtype=torch.uint8, device=device)
    assert lib.mv_cohort_stats_f32(None, 0, cohort.data_ptr(), m, dim, top_n, out.data_ptr(), out.data_ptr() + 32, 0, ws.data_ptr(), 64, _hip.current_stream(x)) == 0
    assert bool((out == 0xFF).all()) and bool((ws == 0xFF).all())
    m0, s0 = _hip.cohort_stats(x[:0], cohort, top_n, cdll=cdll)
    assert m0.shape == (0,) and s0.shape == (0,)


def raw_stats(lib, x, cohort, top_n, hint, fill, stream=None):
    """the C entry point with outputs and workspace pre-filled with ``fill`` bytes -> (mean, std)"""
    from mvector import _hip
    n, m, dim = x.shape[0], cohort.shape[0], x.shape[1]
    need = int(lib.mv_cohort_stats_workspace_bytes(n, m, dim, hint))
    assert need >= m * 4 and need % (m * 4) == 0
    mean = torch.full((n * 4 + 16,), fill, dtype=torch.uint8, device=x.device)
    std = torch.full((n * 4 + 16,), fill, dtype=torch.uint8, device=x.device)
    ws = torch.full((need + 16,), fill, dtype=torch.uint8, device=x.device)
    _hip.check(lib.mv_cohort_stats_f32(x.data_ptr(), n, cohort.data_ptr(), m, dim, top_n, mean.data_ptr(), std.data_ptr(), hint, ws.data_ptr(), need,
                                       stream if stream is not None else _hip.current_stream(x)), lib)
    assert bool((mean[n * 4:] == fill).all()) and bool((std[n * 4:] == fill).all()) and bool((ws[need:] == fill).all()), 'wrote past a buffer'
    return mean[:n * 4].cpu().numpy().view(np.float32), std[:n * 4].cpu().numpy().view(np.float32)


def check_no_hidden_state(cdll, device, second_stream=False):
    from mvector import _hip
    lib = cdll or _hip.lib()
    n, m, dim, top_n = 21, 301, 64, 100
    x, cohort = data(n, m, dim, top_n, device)
    ref = reference_stats(cos_matrix(cdll, x, cohort), top_n)
    for hint in (0, 4):
        ff = raw_stats(lib, x, cohort, top_n, hint, 0xFF)
        zz = raw_stats(lib, x, cohort, top_n, hint, 0x00)
        assert_stats(ff, ref, f'0xFF-filled buffers, rows_hint {hint}')
        assert same_bits(ff, zz), 'the result depends on what the buffers held'
    assert same_bits(stats(cdll, x, cohort, top_n), ff), 'a repeated call gives other bits'
    for r in (0, 15, 16, 20):   # a row's statistics do not depend on the batch it sits in
        one = stats(cdll, x[r:r + 1], cohort, top_n)
        assert one[0].tobytes() == ff[0][r:r + 1].tobytes() and one[1].tobytes() == ff[1][r:r + 1].tobytes(), r
    if second_stream:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            other = stats(cdll, x, cohort, top_n)
        side.synchronize()
        assert same_bits(other, ff), 'another stream gives other bits'


def check_refusals(cdll, device):
    """a refusal is a returned status with a message that names the limit; nothing is launched"""
    from mvector import _hip
    lib = cdll or _hip.lib()
    msg = lambda: lib.mv_last_error().decode()
    n, m, dim, top_n = 3, 20, 16, 5
    x, cohort = data(n, m, dim, top_n, device)
    mean = torch.full((n,), 7.0, device=device)
    std = torch.full((n,), 7.0, device=device)
    need = int(lib.mv_cohort_stats_workspace_bytes(n, m, dim, 0))
    assert need == n * m * 4 and int(lib.mv_cohort_stats_workspace_bytes(n, m, dim, 2)) == 2 * m * 4
    assert int(lib.mv_cohort_stats_workspace_bytes(10 ** 9, 32768, dim, 0)) == int(lib.mv_cohort_stats_workspace_bytes(10 ** 8, 32768, dim, 0))
    ws = torch.zeros(need, dtype=torch.uint8, device=device)

    def call(x_ptr=x.data_ptr(), n=n, c_ptr=cohort.data_ptr(), m=m, dim=dim, top_n=top_n, m_ptr=mean.data_ptr(), s_ptr=std.data_ptr(), ws_ptr=ws.data_ptr(),
             nbytes=need):
        return lib.mv_cohort_stats_f32(x_ptr, n, c_ptr, m, dim, top_n, m_ptr, s_ptr, 0, ws_ptr, nbytes, _hip.current_stream(x))
    for null in ('x_ptr', 'c_ptr', 'm_ptr', 's_ptr'):
        assert call(**{null: None}) == -1 and 'null tensor' in msg(), null
    assert call(ws_ptr=None) == -1 and 'null workspace' in msg()
    assert call(n=-1) == -1 and 'negative n' in msg()
    assert call(m=0) == -1 and 'm below 1' in msg()
    assert call(top_n=0) == -1 and 'top_n below 1' in msg()
    assert call(dim=0) == -1 and 'dim below 1' in msg()
    assert call(m=32769) == _hip.MV_ERR_UNSUPPORTED and 'm above MV_COHORT_MAX_ROWS' in msg()
    assert call(nbytes=need - 1) == -4 and 'workspace smaller' in msg()
    for bad in (dict(n=-1), dict(m=0), dict(dim=0), dict(m=32769)):
        args = dict(n=n, m=m, dim=dim)
        args.update(bad)
        assert int(lib.mv_cohort_stats_workspace_bytes(args['n'], args['m'], args['dim'], 0)) == 0, bad
    assert bool((mean == 7.0).all()) and bool((std == 7.0).all()), 'a refused call wrote to its output'
    assert call() == 0 and bool((std != 7.0).all())
    with pytest.raises(RuntimeError, match='top_n below 1'):
        _hip.cohort_stats(x, cohort, 0, cdll=cdll)
    # the normalisation
    sc = torch.full((2, 3), 7.0, device=device)
    st = torch.ones(3, device=device)

    def norm(s_ptr=sc.data_ptr(), nt=2, ne=3, tm=st.data_ptr(), ts=st.data_ptr(), em=st.data_ptr(), es=st.data_ptr(), mode=_hip.MV_SNORM_S, o_ptr=sc.data_ptr()):
        return lib.mv_score_norm_f32(s_ptr, nt, ne, tm, ts, em, es, mode, o_ptr, _hip.current_stream(sc))
    assert norm(s_ptr=None) == -1 and 'null tensor' in msg()
    assert norm(o_ptr=None) == -1 and 'null tensor' in msg()
    assert norm(nt=-1) == -1 and 'negative n_trials or n_enroll' in msg()
    assert norm(ne=-1) == -1 and 'negative n_trials or n_enroll' in msg()
    assert norm(mode=3) == -1 and 'unknown mode' in msg()
    assert norm(mode=-1) == -1 and 'unknown mode' in msg()
    assert norm(nt=1 << 16, ne=1 << 15) == -1 and 'more than 2^31 - 1 elements' in msg()
    for mode, used in ((_hip.MV_SNORM_S, ('tm', 'ts', 'em', 'es')), (_hip.MV_SNORM_Z, ('em', 'es')), (_hip.MV_SNORM_T, ('tm', 'ts'))):
        for name in ('tm', 'ts', 'em', 'es'):
            if name in used:
                assert norm(mode=mode, **{name: None}) == -1 and ('null trial statistics' if name[0] == 't' else 'null enrolment statistics') in msg(), (mode, name)
    assert bool((sc == 7.0).all()), 'a refused call wrote to its output'
    assert norm(nt=0) == 0 and norm(ne=0) == 0 and norm(nt=0, s_ptr=None, o_ptr=None) == 0 and bool((sc == 7.0).all())   # empty: nothing is touched
    with pytest.raises(ValueError, match='mode'):
        _hip.score_norm(sc, (st[:2], st[:2]), (st, st), mode='x', cdll=cdll)
    assert lib.mv_abi_version() == 5


# ------------------------------------------------------------------------------------------------ normalisation
def numpy_norm(s, tm, ts, em, es, mode):
    """the contract's expression in numpy.float32, one rounded operation after the other"""
    f = np.float32
    assert all(v.dtype == f for v in (s, tm, ts, em, es))
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        t = (s - tm[:, None]) / ts[:, None]
        z = (s - em[None, :]) / es[None, :]
        return {'s': f(0.5) * (t + z), 'z': z, 't': t}[mode]


def assert_same_floats(got, want, what=''):
    assert got.dtype == np.float32 and got.shape == want.shape, what
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    assert bool(same.all()), f'{what}: differs at {np.argwhere(~same)[:4].tolist()}: {got[~same][:4]} != {want[~same][:4]}'


def check_normalisation(cdll, device):
    from mvector import _hip
    g = torch.Generator().manual_seed(8)
    for nt, ne in ((1, 1), (3, 5), (257, 33)):
        s = torch.randn(nt, ne, generator=g) * 0.3
        tm, em = torch.randn(nt, generator=g) * 0.1, torch.randn(ne, generator=g) * 0.1
        ts, es = torch.rand(nt, generator=g) * 0.1 + 0.01, torch.rand(ne, generator=g) * 0.1 + 0.01
        if nt > 2:   # std == 0 and NaN statistics: the IEEE results, as numpy gives them (x / 0 = +-inf, 0 / 0 = NaN)
            ts[1], tm[2] = 0.0, float('nan')
            es[0], es[3], em[4] = 0.0, float('nan'), float('inf')
            s[1, 2] = tm[1]
        host = [v.numpy() for v in (s, tm, ts, em, es)]
        dev = [v.to(device) for v in (s, tm, ts, em, es)]
        for mode in ('s', 'z', 't'):
            want = numpy_norm(*host, mode)
            got = _hip.score_norm(dev[0], (dev[1], dev[2]), (dev[3], dev[4]), mode, cdll=cdll)
            assert got.device == dev[0].device
            assert_same_floats(got.cpu().numpy(), want, f'{nt} x {ne} mode {mode}')
            # the unused side as null pointers
            got = _hip.score_norm(dev[0], None if mode == 'z' else (dev[1], dev[2]), None if mode == 't' else (dev[3], dev[4]), mode, cdll=cdll)
            assert_same_floats(got.cpu().numpy(), want, f'{nt} x {ne} mode {mode}, null unused side')
            # pointers one float behind a 16-byte boundary: both, the input alone, the output alone
            for off_in, off_out in ((1, 1), (1, 0), (0, 1), (2, 3)):
                src = torch.zeros(nt * ne + 4, device=device)[off_in:off_in + nt * ne].view(nt, ne).copy_(dev[0])
                dst = torch.full((nt * ne + 8,), 9.0, device=device)
                out = dst[off_out:off_out + nt * ne].view(nt, ne)
                assert src.data_ptr() % 16 == 4 * off_in and out.data_ptr() % 16 == 4 * off_out
                _hip.score_norm(src, (dev[1], dev[2]), (dev[3], dev[4]), mode, out=out, cdll=cdll)
                assert_same_floats(out.cpu().numpy(), want, f'{nt} x {ne} mode {mode}, offsets {off_in}, {off_out}')
                assert bool((dst[:off_out] == 9.0).all()) and bool((dst[off_out + nt * ne:] == 9.0).all()), 'wrote outside the matrix'
            # in place
            work = dev[0].clone()
            assert _hip.score_norm(work, (dev[1], dev[2]), (dev[3], dev[4]), mode, out=work, cdll=cdll) is work
            assert_same_floats(work.cpu().numpy(), want, f'{nt} x {ne} mode {mode}, in place')


# ------------------------------------------------------------------------------------------------ a tiny evaluation set
def make_eval_set(tmp_path, n_spk=3, per_spk=3, n_cohort=5, seed=5, num_workers=0):
    """wav files of different lengths, enrol / trial / cohort lists (two utterances per cohort speaker) and a TDNN checkpoint"""
    import scipy.io.wavfile as wavfile
    man, sd, _, _, _ = load_case('tdnn')
    model_dir = tmp_path / 'model'
    model_dir.mkdir()
    torch.save({'0.' + k: v for k, v in sd.items()}, str(model_dir / 'model.pth'))
    rng = np.random.default_rng(seed)
    lines = {'enroll': [], 'trials': [], 'cohort': []}
    for spk in range(n_spk + n_cohort):
        base = frontend.synth_waveforms(1, 16000, seed=100 + spk)[0].numpy()
        for u in range(per_spk if spk < n_spk else 2):
            n = int(rng.integers(9000, 16000))
            x = base[:n] + 0.02 * rng.standard_normal(n).astype(np.float32)
            pcm = np.clip(x * 20000, -32768, 32767).astype(np.int16)
            path = str(tmp_path / f's{spk}_u{u}.wav')
            wavfile.write(path, 16000, pcm)
            lines['cohort' if spk >= n_spk else 'enroll' if u == 0 else 'trials'].append(f'{path}\t{spk}\n')
    for k, v in lines.items():
        with open(str(tmp_path / f'{k}.txt'), 'w') as f:
            f.writelines(v)
    cfg = dict(dataset_conf=dict(dataset=dict(min_duration=0.3, sample_rate=16000, use_dB_normalization=True, target_dB=-20),
                                 eval_conf=dict(batch_size=4, max_duration=20), dataLoader=dict(num_workers=num_workers),
                                 enroll_list=str(tmp_path / 'enroll.txt'), trials_list=str(tmp_path / 'trials.txt')),
               preprocess_conf=dict(feature_method='Fbank', method_args=dict(sample_frequency=16000, num_mel_bins=80)),
               model_conf=dict(model='TDNN', model_args=dict(embd_dim=192)))
    return cfg, str(model_dir), str(tmp_path / 'cohort.txt')


def embed_lists(trainer, cohort_list):
    """the three lists embedded the way evaluate_normalized embeds them (the model is loaded already)"""
    from torch.utils.data import DataLoader
    from mvector.data_utils.collate_fn import collate_fn, collate_waveforms
    from mvector.data_utils.reader import MVectorDataset
    use_wave = trainer._loaders()
    ds = trainer.configs.dataset_conf
    cohort_set = MVectorDataset(data_list_path=cohort_list, audio_featurizer=trainer.audio_featurizer, mode='eval', return_waveform=use_wave,
                                max_duration=ds.eval_conf.max_duration, **dict(ds.dataset))
    loader = DataLoader(dataset=cohort_set, collate_fn=collate_waveforms if use_wave else collate_fn, shuffle=False, batch_size=ds.eval_conf.batch_size)
    return [trainer._embed(l, trainer.model, use_wave) for l in (trainer.enroll_loader, trainer.trials_loader, loader)]
