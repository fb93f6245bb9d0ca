"""Checks of the fused cosine + top-k search (csrc/search.hip) shared by tests/test_search.py (the emulator build, CPU tensors) and
tests/test_gpu_search.py (the product library on the device).  Each takes the bound library (None = the product library) and a device.

Nothing here is a tolerance.  The search promises the top-k of the matrix mv_cosine_f32 writes, so the reference is computed in numpy from
the downloaded ``_hip.cosine`` matrix of the SAME library: descending by the order-preserving key of the score (-0 and +0 one key, every NaN
above +inf), equal keys by the lower row first.  Indices must be equal and scores must compare ``==`` (or both be NaN)."""
import numpy as np
import pytest
import torch

HINTS = (0, 1, 2, 3, 7)
# (n, m, dim, k): one tile; a ragged tile; ragged tiles on both sides; around 16 tiles with two query tiles and a ragged third; many tiles at the
# largest k; rows of 200 bytes (unaligned: the guarded loads); a dim that is a multiple of 4 but not of 16; the shortest row; one K block
EQUAL_CASES = ((1, 1, 192, 1), (1, 15, 192, 1), (17, 17, 192, 5), (33, 255, 192, 8), (33, 256, 192, 8), (33, 257, 192, 8), (16, 1023, 192, 64),
               (16, 1025, 192, 64), (3, 4097, 50, 7), (5, 300, 200, 4), (2, 40, 1, 3), (2, 40, 16, 3))
# dim above 256 (the gallery fragment is re-read per query tile instead of kept in registers), also with a ragged last K block
WIDE_CASES = ((17, 70, 272, 5), (3, 33, 515, 4))
LARGE_CASES = ((33, 20000, 192, 64, 5), (1, 100003, 192, 1, 11))   # (..., the pinned hint beside the automatic one)


def keys_of(scores):
    """uint32 keys in the order of the float32 scores: -0 == +0, NaN above +inf"""
    u = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = np.where(u == 0x80000000, 0, u)
    key = np.where(u >= 0x80000000, 0xFFFFFFFF - u, u + 0x80000000)
    return np.where((u & 0x7FFFFFFF) > 0x7F800000, 0xFFFFFFFF, key)


def reference(cos, k):
    """the rule on a downloaded cosine matrix [n, m] -> (scores [n, k], index [n, k]); (-inf, -1) behind m"""
    n, m = cos.shape
    s = np.full((n, k), -np.inf, dtype=np.float32)
    idx = np.full((n, k), -1, dtype=np.int32)
    key = keys_of(cos).astype(np.int64)
    for r in range(n):
        order = np.lexsort((np.arange(m), -key[r]))[:k]   # key descending, then row ascending
        idx[r, :order.size] = order
        s[r, :order.size] = cos[r, order]
    return s, idx


def assert_same(got, want, what=''):
    (gs, gi), (ws, wi) = got, want
    assert gs.dtype == np.float32 and gi.dtype == np.int32 and gs.shape == ws.shape and gi.shape == wi.shape, what
    assert np.array_equal(gi, wi), f'{what}: indices differ at {np.argwhere(gi != wi)[:4].tolist()}'
    same = (gs == ws) | (np.isnan(gs) & np.isnan(ws))
    assert bool(same.all()), f'{what}: scores differ at {np.argwhere(~same)[:4].tolist()}'


def data(n, m, dim, seed, device, misalign=False):
    g = torch.Generator().manual_seed(seed)
    if not misalign:
        return torch.randn(n, dim, generator=g).to(device), torch.randn(m, dim, generator=g).to(device)
    # rows that start 4 bytes behind a 16-byte boundary
    q = torch.randn(n * dim + 1, generator=g).to(device)[1:].view(n, dim)
    gal = torch.randn(m * dim + 1, generator=g).to(device)[1:].view(m, dim)
    assert q.data_ptr() % 16 == 4 and gal.data_ptr() % 16 == 4 and q.is_contiguous()
    return q, gal


def search(cdll, q, gal, k, hint=0):
    from mvector import _hip
    s, i = _hip.cosine_topk(q, gal, k, slices_hint=hint, cdll=cdll)
    assert s.device == q.device and i.device == q.device
    return s.cpu().numpy(), i.cpu().numpy()


def cos_matrix(cdll, q, gal):
    from mvector import _hip
    return _hip.cosine(q, gal, cdll=cdll).cpu().numpy()


def check_equals_cosine(cdll, device, n, m, dim, k, hints=HINTS, misalign=False):
    q, gal = data(n, m, dim, 1000 + n + m + dim + k, device, misalign)
    want = reference(cos_matrix(cdll, q, gal), k)
    first = None
    for hint in hints:
        got = search(cdll, q, gal, k, hint)
        assert_same(got, want, f'({n}, {m}, {dim}, {k}) slices_hint {hint}')
        if first is None:
            first = got
        assert got[0].tobytes() == first[0].tobytes() and got[1].tobytes() == first[1].tobytes(), f'slices_hint {hint}: other bits than {hints[0]}'


def slice_starts(m, slices):
    """first rows of the slices 1 .. S - 1 (include/mvector_hip.h: slice s starts at row 16 floor(s T / S), T = ceil(m / 16))"""
    tiles = -(-m // 16)
    s = min(slices, tiles)
    return [16 * (j * tiles // s) for j in range(1, s)]


def check_ties(cdll, device):
    """exact copies and copies scaled by powers of two on both sides of every slice boundary of S = 2 and S = 3: the lower row comes first"""
    m, dim, k = 117, 192, 6
    bounds = sorted(set(slice_starts(m, 2) + slice_starts(m, 3)))
    assert bounds == [32, 64, 80]
    g = torch.Generator().manual_seed(77)
    gal = torch.randn(m, dim, generator=g)
    q = torch.empty(len(bounds), dim)
    for j, b in enumerate(bounds):
        v = torch.randn(dim, generator=g)
        gal[b - 2], gal[b - 1], gal[b], gal[b + 1] = v, 2.0 * v, 0.5 * v, v
        q[j] = v + 0.05 * torch.randn(dim, generator=g)
    q, gal = q.to(device), gal.to(device)
    cos = cos_matrix(cdll, q, gal)
    for j, b in enumerate(bounds):   # scaling a row by a power of two changes no bit of its cosine: the four are one value
        assert len({cos[j, c].tobytes() for c in range(b - 2, b + 2)}) == 1 and cos[j, b] == cos[j].max(), (j, b)
    want = reference(cos, k)
    for hint in (2, 3, 1, 0):
        got = search(cdll, q, gal, k, hint)
        assert_same(got, want, f'ties, slices_hint {hint}')
        for j, b in enumerate(bounds):
            assert got[1][j, :4].tolist() == [b - 2, b - 1, b, b + 1], (hint, j, got[1][j])
    # one vector in every row: rows 0 .. k - 1
    same = torch.randn(1, dim, generator=g).repeat(40, 1).to(device)
    q3 = torch.randn(3, dim, generator=g).to(device)
    for hint in (0, 2, 3):
        s, i = search(cdll, q3, same, 8, hint)
        assert np.array_equal(i, np.tile(np.arange(8, dtype=np.int32), (3, 1))), (hint, i)
        assert_same((s, i), reference(cos_matrix(cdll, q3, same), 8), f'identical gallery, slices_hint {hint}')


def check_special_values(cdll, device):
    g = torch.Generator().manual_seed(5)
    n, m, dim, k = 4, 40, 16, 5
    q, gal = torch.randn(n, dim, generator=g), torch.randn(m, dim, generator=g)
    gal[3] = float('nan')
    gal[5, 2] = float('inf')
    gal[7] = 0.0
    gal[20, 0] = float('nan')
    q[2] = float('nan')
    q, gal = q.to(device), gal.to(device)
    cos = cos_matrix(cdll, q, gal)
    assert np.isnan(cos[2]).all() and np.isnan(cos[:, 3]).all() and (cos[[0, 1, 3], 7] == 0).all()
    want = reference(cos, k)
    for hint in (0, 1, 3):
        got = search(cdll, q, gal, k, hint)
        assert_same(got, want, f'special values, slices_hint {hint}')
        assert got[1][2].tolist() == [0, 1, 2, 3, 4] and np.isnan(got[0][2]).all()          # a NaN query: every score is NaN, the rows in order
        assert got[1][0, :3].tolist() == [3, 5, 20] and np.isnan(got[0][0, :3]).all()        # NaN ranks above everything (inf / inf is one too)
    # more slots than rows
    s, i = search(cdll, q, gal[:3], 8)
    assert_same((s, i), reference(cos[:, :3], 8), 'k > m')
    assert (i[:, 3:] == -1).all() and np.isneginf(s[:, 3:]).all() and (i[:, :3] >= 0).all()
    # an empty gallery, no queries
    s, i = search(cdll, q, gal[:0], 4, 2)
    assert s.shape == (n, 4) and (i == -1).all() and np.isneginf(s).all()
    s, i = search(cdll, q[:0], gal, 4)
    assert s.shape == (0, 4) and i.shape == (0, 4)


def raw_call(lib, q, gal, k, hint, fill, stream=None):
    """the C entry point with outputs and workspace pre-filled with ``fill`` bytes -> (scores, index, workspace bytes used)"""
    from mvector import _hip
    n, m, dim = q.shape[0], gal.shape[0], q.shape[1]
    need = int(lib.mv_cosine_topk_workspace_bytes(n, m, dim, k, hint))
    assert need >= n * k * 8
    s = torch.full((n * k * 4 + 16,), fill, dtype=torch.uint8, device=q.device)
    i = torch.full((n * k * 4 + 16,), fill, dtype=torch.uint8, device=q.device)
    ws = torch.full((need + 16,), fill, dtype=torch.uint8, device=q.device)
    _hip.check(lib.mv_cosine_topk_f32(q.data_ptr(), n, gal.data_ptr(), m, dim, k, s.data_ptr(), i.data_ptr(), hint, ws.data_ptr(), need,
                                      stream if stream is not None else _hip.current_stream(q)), lib)
    assert bool((s[n * k * 4:] == fill).all()) and bool((i[n * k * 4:] == fill).all()) and bool((ws[need:] == fill).all()), 'wrote past a buffer'
    return s[:n * k * 4].cpu().numpy().view(np.float32).reshape(n, k), i[:n * k * 4].cpu().numpy().view(np.int32).reshape(n, k)


def check_no_hidden_state(cdll, device, second_stream=False):
    from mvector import _hip
    lib = cdll or _hip.lib()
    n, m, dim, k = 33, 300, 192, 8
    q, gal = data(n, m, dim, 9, device)
    want = reference(cos_matrix(cdll, q, gal), k)
    for hint in (0, 3):
        ff = raw_call(lib, q, gal, k, hint, 0xFF)
        zz = raw_call(lib, q, gal, k, hint, 0x00)
        assert_same(ff, want, f'0xFF-filled buffers, slices_hint {hint}')
        assert ff[0].tobytes() == zz[0].tobytes() and ff[1].tobytes() == zz[1].tobytes(), 'the result depends on what the buffers held'
    again = search(cdll, q, gal, k)
    assert again[0].tobytes() == ff[0].tobytes() and again[1].tobytes() == ff[1].tobytes(), 'a repeated call gives other bits'
    host = _hip.cosine_topk(q, gal, k, cdll=cdll, to_host=True)   # both outputs in one transfer
    assert isinstance(host[0], np.ndarray) and host[0].tobytes() == ff[0].tobytes() and host[1].tobytes() == ff[1].tobytes()
    for r in (0, 15, 16, 32):   # a query's answer does not depend on the batch it sits in
        one = search(cdll, q[r:r + 1], gal, k)
        assert one[0].tobytes() == ff[0][r:r + 1].tobytes() and one[1].tobytes() == ff[1][r:r + 1].tobytes(), r
    # a k > m tail and an empty gallery over poisoned buffers: every slot is written
    tail = raw_call(lib, q, gal[:5], k, 0, 0xFF)
    assert (tail[1][:, 5:] == -1).all() and np.isneginf(tail[0][:, 5:]).all()
    empty = raw_call(lib, q, gal[:0], k, 0, 0xFF)
    assert (empty[1] == -1).all() and np.isneginf(empty[0]).all()
    # no queries: nothing is touched
    s = torch.full((64,), 7.0, device=device)
    i = torch.full((64,), 7, dtype=torch.int32, device=device)
    ws = torch.full((64,), 7, dtype=torch.uint8, device=device)
    assert lib.mv_cosine_topk_f32(None, 0, gal.data_ptr(), m, dim, k, s.data_ptr(), i.data_ptr(), 0, ws.data_ptr(), 64, _hip.current_stream(q)) == 0
    assert bool((s == 7.0).all()) and bool((i == 7).all()) and bool((ws == 7).all())
    if second_stream:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            other = search(cdll, q, gal, k)
        side.synchronize()
        assert other[0].tobytes() == ff[0].tobytes() and other[1].tobytes() == ff[1].tobytes(), 'another stream gives other bits'


def check_refusals(cdll, device):
    """a refusal is a returned status with a message that names the limit; nothing is launched"""
    from mvector import _hip
    lib = cdll or _hip.lib()
    msg = lambda: lib.mv_last_error().decode()
    n, m, dim, k = 3, 20, 16, 4
    q, gal = data(n, m, dim, 3, device)
    s = torch.full((n, k), 7.0, device=device)
    i = torch.full((n, k), 7, dtype=torch.int32, device=device)
    need = int(lib.mv_cosine_topk_workspace_bytes(n, m, dim, k, 0))
    assert need >= n * k * 8 and int(lib.mv_cosine_topk_workspace_bytes(n, m, dim, k, 1)) == n * k * 8
    ws = torch.zeros(need, dtype=torch.uint8, device=device)

    def call(q_ptr=q.data_ptr(), n=n, g_ptr=gal.data_ptr(), m=m, dim=dim, k=k, s_ptr=s.data_ptr(), i_ptr=i.data_ptr(), ws_ptr=ws.data_ptr(), nbytes=need):
        return lib.mv_cosine_topk_f32(q_ptr, n, g_ptr, m, dim, k, s_ptr, i_ptr, 0, ws_ptr, nbytes, _hip.current_stream(q))
    for null in ('q_ptr', 'g_ptr', 's_ptr', 'i_ptr'):
        assert call(**{null: None}) == -1 and 'null tensor' in msg(), null
    assert call(ws_ptr=None) == -1 and 'null workspace' in msg()
    assert call(n=-1) == -1 and 'negative n or m' in msg()
    assert call(m=-1) == -1 and 'negative n or m' in msg()
    assert call(k=0) == -1 and 'k outside 1 .. 64' in msg()
    assert call(k=65) == -1 and 'k outside 1 .. 64' in msg()
    assert call(dim=0) == -1 and 'dim below 1' in msg()
    assert call(dim=2048) == _hip.MV_ERR_UNSUPPORTED and 'dim above 2047' in msg()
    assert call(nbytes=need - 1) == -4 and 'workspace smaller' in msg()
    for bad in (dict(n=-1), dict(m=-1), dict(k=0), dict(k=65), dict(dim=0), dict(dim=2048)):
        args = dict(n=n, m=m, dim=dim, k=k)
        args.update(bad)
        assert int(lib.mv_cosine_topk_workspace_bytes(args['n'], args['m'], args['dim'], args['k'], 0)) == 0, bad
    assert bool((s == 7.0).all()) and bool((i == 7).all()), 'a refused call wrote to its output'
    assert call() == 0 and bool((i >= 0).all())
    with pytest.raises(RuntimeError, match='k outside 1 .. 64'):
        _hip.cosine_topk(q, gal, 65, cdll=cdll)
    with pytest.raises(RuntimeError, match='dim above 2047'):
        _hip.cosine_topk(torch.zeros(1, 2048, device=device), torch.zeros(2, 2048, device=device), 1, cdll=cdll)
    assert lib.mv_abi_version() == 5
