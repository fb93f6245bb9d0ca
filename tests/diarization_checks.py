"""Checks of the speaker-diarization kernels (csrc/diarize.hip) shared by tests/test_diarization.py (the emulator build, CPU tensors) and
tests/test_gpu_diarization.py (the product library on the device).  Each takes the bound library (None = the product library) and a device."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN

GOLDEN_N = (33, 40, 300, 301, 700, 1200)
TOL = 1e-6   # the solver's default stop rule, relative to ub = 2 max degree


def golden(n):
    z = np.load(os.path.join(GOLDEN, f'diarization_{n}.npz'))
    return {k: z[k] for k in z.files}


def synth_embeddings(n, speakers=2, sigma=0.6, seed=0):
    """seeded 192-d centres plus Gaussian noise in contiguous turns (the recipe of tools/make_diarization_golden.py)"""
    rng = np.random.default_rng(1000 + seed + n)
    centres = rng.standard_normal((speakers, 192))
    who = []
    while len(who) < n:
        who += [int(rng.integers(speakers))] * int(rng.integers(3, 31))
    who = np.array(who[:n])
    return (centres[who] + sigma * rng.standard_normal((n, 192))).astype(np.float32)


_SIM = {}


def similarity(n):
    """fp32 cosine matrix of the check at size n, computed once"""
    if n not in _SIM:
        from mvector.infer_utils.speaker_diarization import SpectralCluster
        X = golden(n)['X'].astype(np.float32) if n in GOLDEN_N else synth_embeddings(n, 3 if n > 100 else 2)
        _SIM[n] = SpectralCluster.get_sim_mat(X)
        _SIM[n].setflags(write=False)
    return _SIM[n]


def _n_prune(n):
    from mvector.infer_utils.speaker_diarization import SpectralCluster
    return SpectralCluster().n_prune(n)   # the reference's int((1 - pval) * N)


def host_affinity(sim, n_prune):
    """the host restatement on the same fp32 matrix: prune (ties: lower column first), symmetrise, zero diagonal"""
    A = sim.copy()
    for i in range(A.shape[0]):
        A[i, np.argsort(A[i], kind='stable')[:n_prune]] = 0
    M = 0.5 * (A + A.T)
    M[np.diag_indices(M.shape[0])] = 0
    return M


def check_affinity(cdll, device, n):
    from mvector import _hip
    sim = similarity(n)
    n_prune = _n_prune(n)
    M, degree = _hip.affinity_laplacian(torch.from_numpy(sim.copy()).to(device), n_prune, cdll=cdll)
    want = host_affinity(sim, n_prune)
    assert M.dtype == torch.float32 and np.array_equal(M.cpu().numpy(), want), f'N={n}: M differs from the host restatement'
    ref = np.abs(want.astype(np.float64)).sum(axis=1)
    rel = (np.abs(degree.cpu().numpy() - ref) / ref).max()
    print(f'affinity N={n} n_prune={n_prune}: degree max rel err {rel:.2e}')
    assert rel <= 1e-12, rel
    return M, degree


def check_tie_rule(cdll, device):
    """row 0 holds three equal values across the cut: the two in the LOWER columns fall, the third stays"""
    from mvector import _hip
    rng = np.random.default_rng(3)
    S = rng.uniform(0.3, 0.8, size=(6, 6)).astype(np.float32)
    S[1:, 0] = -1.0                                   # every other row drops its column 0: M[0] is half of row 0's own survivors
    S[0] = [0.5, 0.2, 0.2, 0.2, 0.9, 0.1]
    M, _ = _hip.affinity_laplacian(torch.from_numpy(S).to(device), 3, cdll=cdll)   # 0.1 and two of the three 0.2 fall
    M = M.cpu().numpy()
    assert M[0].tolist() == [0.0, 0.0, 0.0, np.float32(0.5) * np.float32(0.2), np.float32(0.5) * np.float32(0.9), 0.0], M[0]
    assert np.array_equal(M, host_affinity(S, 3))


def check_eig(cdll, device, n, second_stream=False):
    import scipy.linalg
    from mvector import _hip
    M, degree = check_affinity(cdll, device, n)
    L = np.diag(degree.cpu().numpy()) - M.cpu().numpy().astype(np.float64)
    exact = scipy.linalg.eigvalsh(L)
    m = min(16, n)
    lam, V, info = _hip.laplacian_eig_lowest(M, degree, m=m, cdll=cdll)
    ub = 2 * degree.max().item()
    err = np.abs(lam - exact[:m]).max()
    Vh = V.cpu().numpy()
    orth = np.abs(Vh.T @ Vh - np.eye(m)).max()
    print(f'eig N={n} m={m}: {info}, |lambda - eigvalsh| max {err:.2e} = {err / ub:.2e} ub, |VtV - I| max {orth:.2e}')
    assert info['ub'] == ub and info['converged'] == 1
    assert err <= TOL * ub, (err, TOL * ub)             # a Ritz value lies within its residual of an eigenvalue: the stop rule is the bar
    assert info['residual'] <= TOL * ub, info
    assert orth <= 1e-12, orth
    true_res = np.linalg.norm(L @ Vh - Vh * lam, axis=0).max()
    assert true_res <= 2 * TOL * ub, true_res          # the reported residual is the real one (M X is summed in another order here)
    if second_stream:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            M2, degree2 = _hip.affinity_laplacian(torch.from_numpy(similarity(n).copy()).to(device), _n_prune(n), cdll=cdll)
            lam2, V2, info2 = _hip.laplacian_eig_lowest(M2, degree2, m=m, cdll=cdll)
        torch.cuda.current_stream().wait_stream(side)
        assert torch.equal(M2, M) and torch.equal(degree2, degree)
    else:
        lam2, V2, info2 = _hip.laplacian_eig_lowest(M, degree, m=m, cdll=cdll)
    assert np.array_equal(lam, lam2) and torch.equal(V, V2) and info == info2, 'not bit-identical on a second call'
    return M, degree


def check_not_converged(cdll, device, n=65):
    from mvector import _hip
    M, degree = check_affinity(cdll, device, n)
    with pytest.raises(RuntimeError, match=r'residual .* above tol \* ub .*code -6; residual'):
        _hip.laplacian_eig_lowest(M, degree, m=16, max_iters=1, cdll=cdll)
    # the raw call: the distinct status, and finite Ritz pairs with the info block filled in rather than garbage
    lib = cdll or _hip.lib()
    cfg = _hip.MvEigCfg()
    lib.mv_laplacian_eig_default_cfg(ctypes.byref(cfg))
    cfg.max_iters = 1
    nbytes = lib.mv_laplacian_eig_lowest_workspace_bytes(n, ctypes.byref(cfg))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    lam = (ctypes.c_double * 16)()
    vecs = torch.full((n, 16), float('nan'), dtype=torch.float64, device=device)
    info = _hip.MvEigInfo()
    rc = lib.mv_laplacian_eig_lowest(M.data_ptr(), degree.data_ptr(), n, ctypes.byref(cfg), lam, vecs.data_ptr(), ctypes.byref(info), ws.data_ptr(),
                                     nbytes, _hip.current_stream(M))
    assert rc == _hip.MV_ERR_NOT_CONVERGED == -6
    assert info.iterations == 1 and info.converged == 0 and info.residual > TOL * info.ub and np.isfinite(info.residual)
    assert torch.isfinite(vecs).all() and np.isfinite(np.array(lam[:])).all()


def check_wave_chunks(cdll, device):
    from mvector import _hip
    rng = np.random.default_rng(11)
    L, chunk_len = 5000, 1200                                      # more than one pass of the 256 threads over a row
    wav = (0.1 * rng.standard_normal(L)).astype(np.float32)
    wav[3000:4200] = 0.0                                           # an all-zero chunk
    start = np.array([0, 100, 777, L - chunk_len, 3000, 2500], dtype=np.int64)   # at the start, short, empty, ending exactly at L, silent, plain
    length = np.array([chunk_len, 500, 0, chunk_len, chunk_len, 1199], dtype=np.int64)
    t = lambda a: torch.from_numpy(a).to(device)
    rows, quiet = _hip.wave_chunks(t(wav), t(start), t(length), chunk_len, cdll=cdll)
    want = np.zeros((len(start), chunk_len), dtype=np.float32)
    for i, (s, n) in enumerate(zip(start, length)):
        want[i, :n] = wav[s:s + n]
    assert np.array_equal(rows.cpu().numpy(), want) and quiet.tolist() == [0] * 6       # without normalisation: bit-equal to slicing
    scaled, quiet = _hip.wave_chunks(t(wav), t(start), t(length), chunk_len, target_db=-20.0, cdll=cdll)
    scaled = scaled.cpu().numpy()
    assert quiet.tolist() == [0, 0, 1, 0, 1, 0]                    # the empty and the silent chunk: flagged ...
    assert np.array_equal(scaled[2], want[2]) and np.array_equal(scaled[4], want[4])    # ... and left unscaled
    for i in (0, 1, 3, 5):
        mean_sq = np.sum(want[i].astype(np.float64) ** 2) / chunk_len                  # over the padded row
        gain = 10.0 ** ((-20.0 - 10.0 * np.log10(mean_sq)) / 20.0)
        nz = want[i] != 0
        rel = np.abs(scaled[i][nz].astype(np.float64) / want[i][nz].astype(np.float64) / gain - 1).max()
        print(f'wave_chunks row {i}: gain {gain:.4f}, max rel err {rel:.2e}')
        assert rel <= 1e-6, rel
        assert not scaled[i][~nz].any()


def check_refusals(cdll, device):
    """a refusal is a returned status with a message that names the limit; nothing is launched"""
    from mvector import _hip
    lib = cdll or _hip.lib()
    buf = torch.zeros(1 << 17, dtype=torch.uint8, device=device)
    p = buf.data_ptr()
    msg = lambda: lib.mv_last_error().decode()
    assert lib.mv_affinity_laplacian_f32(p, 0, 0, p + 4096, p + 8192, p + 16384, 4096, None) == -1 and 'N outside 1 .. 16384' in msg()
    assert lib.mv_affinity_laplacian_f32(p, 16385, 0, p + 4096, p + 8192, p + 16384, 4096, None) == -1 and 'N outside 1 .. 16384' in msg()
    assert lib.mv_affinity_laplacian_workspace_bytes(16385) == 0 and lib.mv_affinity_laplacian_workspace_bytes(16384) > 0
    assert lib.mv_affinity_laplacian_f32(p, 8, 8, p + 4096, p + 8192, p + 16384, 4096, None) == -1 and 'n_prune outside 0 .. N - 1' in msg()
    assert lib.mv_affinity_laplacian_f32(p, 8, 2, p + 4096, p + 8192, None, 4096, None) == -1 and 'null workspace' in msg()
    assert lib.mv_affinity_laplacian_f32(p, 8, 2, p + 4096, p + 8192, p + 16384, 63, None) == -4 and 'workspace smaller' in msg()
    cfg = _hip.MvEigCfg()
    lib.mv_laplacian_eig_default_cfg(ctypes.byref(cfg))
    assert (cfg.m, cfg.block, cfg.degree, cfg.max_iters, cfg.tol) == (16, 0, 16, 60, 1e-6)
    lam = (ctypes.c_double * 32)()
    info = _hip.MvEigInfo()
    call = lambda n, ws, nbytes: lib.mv_laplacian_eig_lowest(p, p + 4096, n, ctypes.byref(cfg), lam, p + 8192, ctypes.byref(info), ws, nbytes, None)
    cfg.m = 17
    assert lib.mv_laplacian_eig_lowest_workspace_bytes(40, ctypes.byref(cfg)) == 0
    assert call(40, p + 65536, 1 << 16) == -1 and 'm outside 1 .. min(16, N)' in msg()
    cfg.m = 6
    assert call(5, p + 65536, 1 << 16) == -1 and 'm outside 1 .. min(16, N)' in msg()
    cfg.m = 1
    assert call(1, p + 65536, 1 << 16) == -1 and 'N outside 2 .. 16384' in msg()
    assert call(16385, p + 65536, 1 << 16) == -1 and 'N outside 2 .. 16384' in msg()
    cfg.m = 4
    need = lib.mv_laplacian_eig_lowest_workspace_bytes(8, ctypes.byref(cfg))
    assert 0 < need < (1 << 16)
    assert call(8, None, need) == -1 and 'null workspace' in msg()
    assert call(8, p + 65536, need - 1) == -4 and 'workspace smaller' in msg()
    with pytest.raises(RuntimeError, match='n_prune outside'):
        _hip.affinity_laplacian(torch.zeros((4, 4), device=device), 4, cdll=cdll)


def check_spectral_cluster_golden(cdll, device, n):
    """SpectralCluster on a tensor (the device path) gives the reference's labels exactly on the golden embeddings"""
    from mvector.infer_utils.speaker_diarization import SpeakerDiarization, SpectralCluster
    g = golden(n)
    sc = SpectralCluster(cdll=cdll)
    labels = SpeakerDiarization._correct_labels(sc(torch.from_numpy(g['X'].astype(np.float32)).to(device)))
    assert np.array_equal(labels, g['labels']), f'N={n}'
    assert sc.last_info['converged'] == 1
    sd = SpeakerDiarization()
    sd.spectral_cluster = sc
    merged, centres = sd.clustering(torch.from_numpy(g['X'].astype(np.float32)).to(device))
    assert np.array_equal(merged, g['merged']) and np.abs(centres - g['centres']).max() <= 1e-6
    segments = [[0.75 * i, 0.75 * i + 1.5, None] for i in range(n)]
    assert sd.postprocess(segments, merged) == json.loads(str(g['postprocess']))
