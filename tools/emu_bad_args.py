"""Bad arguments at the C ABI (no GPU): every field of MvConv1dDesc / MvConv2dsDesc of a VALID layer call -- and every pointer / integer
argument of the positional entry points (linear, time statistics, ASP pooling, Res2Net chain, BN + ReLU rows, TSTP, wave preparation, cosine, the CAM++ dense
block, the reductions and row passes of pool.hip) -- is replaced, one at a
time, by values a caller can get wrong -- a null pointer, 0, -1, a huge size, an enum out of range, a leading dimension smaller than the row --
and the entry point is called on the emulator build.  The contract (include/mvector_hip.h): a call the library cannot run returns an error code
and a message; it never crashes and never touches memory outside the caller's buffers.

    python tools/emu_bad_args.py                 # plain emulator build
    python tools/emu_bad_args.py --mode asan     # AddressSanitizer build: an accepted bad value that reads or writes out of bounds is reported

Output: one line per (entry point, field, value): "rejected" (error code + message), "accepted" (returned MV_OK: fine for optional operands and
hints, listed so that a reader can judge) -- and, if the process dies, the last line printed names the call that killed it.
"""
import argparse
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'tests'), ROOT, os.path.join(ROOT, 'voiceprintrecognition-pytorch_amd'), os.path.join(ROOT, 'tools')]

POINTER_T = ctypes.c_void_p


def candidates(name, typ, value):
    if typ is POINTER_T:
        # only the REQUIRED tensors: dropping an optional operand (second input, residual, bias ...) is a different, valid call whose other arguments
        # -- the channel split of a concatenation, say -- the caller would have set differently
        return [None] if value and name in ('x', 'w', 'w_packed', 'y') else []
    if typ in (ctypes.c_int32, ctypes.c_int64):
        # (sizes LARGER than the buffers are the caller's statement about its own memory: the library has no way to see behind a pointer, so only
        # values that are wrong whatever the buffers are get tried)
        vals = [0, -1]
        if name.startswith('ld') or name in ('ld_add', 'ld_sum'):
            vals += [1, 7]                       # a row shorter than its channels / not a multiple of the vector width
        if name in ('cin16', 'cout16', 'cin1'):
            vals += [value + 1, 8]               # not padded to 16
        if name in ('ks', 'k'):
            vals += [2, 4, 9]
        if name in ('x_dtype', 'y_dtype', 'pad_mode', 'pre_act', 'post_act', 'epi', 'x2_mode', 'stride', 'stride_w', 'dilation', 'tile'):
            vals += [99, 2 ** 31 - 1]
        if name in ('x_dtype', 'y_dtype'):
            vals = [-1, 99, 2 ** 31 - 1]          # (the other VALID code would be a wrong statement about the buffer's element size, not a bad argument)
        return [v for v in dict.fromkeys(vals) if v != value]
    if typ is ctypes.c_float:
        return [float('nan'), 0.0, -1.0] if name == 'oscale' else []
    return []


class TamperArgs:
    """the same for entry points with positional arguments: every pointer argument that was given becomes null, every integer 0 and -1 -- the
    LAST argument (the stream) excepted.  A null pointer for an OPTIONAL operand is a valid call; it shows up under ACCEPTED."""

    def __init__(self, cdll, fn_name, log):
        from mvector import _hip
        self._cdll, self._fn, self._log = cdll, fn_name, log
        self._argtypes = _hip._SIGNATURES[fn_name][1]

    def __getattr__(self, name):
        real = getattr(self._cdll, name)
        if name != self._fn:
            return real

        def call(*args):
            for i, (typ, val) in enumerate(zip(self._argtypes[:-1], args[:-1])):
                if typ is POINTER_T:
                    bads = [None] if val else []
                elif typ in (ctypes.c_int32, ctypes.c_int64):
                    bads = [v for v in (0, -1) if v != val]
                else:
                    bads = []
                for bad in bads:
                    print(f'CALL {self._fn} arg{i} = {bad!r}', flush=True)
                    rc = real(*(args[:i] + (bad,) + args[i + 1:]))
                    msg = self._cdll.mv_last_error().decode() if rc != 0 else ''
                    self._log.append((self._fn, f'arg{i}', bad, rc, msg))
                    print(f'  -> {"accepted" if rc == 0 else "rejected: " + msg[:120]}', flush=True)
            return real(*args)
        return call


class Tamper:
    """stands in for the bound library: the named entry point is first called with every tampered copy of its descriptor"""

    def __init__(self, cdll, fn_name, desc_type, log):
        self._cdll, self._fn, self._type, self._log = cdll, fn_name, desc_type, log

    def __getattr__(self, name):
        real = getattr(self._cdll, name)
        if name != self._fn:
            return real

        def call(desc_ref, stream):
            d = desc_ref._obj
            for field, typ in self._type._fields_:
                saved = getattr(d, field)
                for bad in candidates(field, typ, saved):
                    print(f'CALL {self._fn} {field} = {bad!r}', flush=True)     # (the line that names a crash)
                    setattr(d, field, bad)
                    rc = real(ctypes.byref(d), stream)
                    msg = self._cdll.mv_last_error().decode() if rc != 0 else ''
                    self._log.append((self._fn, field, bad, rc, msg))
                    print(f'  -> {"accepted" if rc == 0 else "rejected: " + msg[:120]}', flush=True)
                    setattr(d, field, saved)
            return real(desc_ref, stream)
        return call


def cam_dense_block_calls(cdll, log):
    """mv_cam_dense_block_f16 / mv_cam_dense_block_workspace_bytes: one valid two-layer call (block kernel geometry), then one argument at a time made
    wrong -- null pointers (the buffer, a parameter array, one layer's pointer inside an array, the workspace), nlayers 0 and 25, T2 0, a row pitch that
    is no multiple of 8 or shorter than the block's channels, a form that does not exist, each pinned form outside its geometry, a short workspace"""
    import torch
    import layer_checks as lc
    from mvector import _hip
    # (the inputs are drawn here: the tool needs nothing of the tests beyond the weight packing that every entry point above uses)
    n, c_in, T2, dil, seg_len = 2, 128, 17, 1, 100
    c_out = c_in + 32 * n
    g = torch.Generator().manual_seed(17)
    rn = lambda *s: torch.randn(*s, generator=g)
    x0 = rn(1, T2, c_in).half()
    params = []
    for l in range(n):
        cin = c_in + 32 * l
        params.append(dict(w1=lc.pack_weight(cdll, rn(128, cin, 1) * (2.0 / cin) ** 0.5), bn1_s=1.0 + 0.1 * rn(cin), bn1_t=0.3 * rn(cin),
                           bn2_s=1.0 + 0.1 * rn(128), bn2_t=0.3 * rn(128), wl=lc.pack_weight(cdll, rn(32, 128, 3) * (2.0 / 384) ** 0.5),
                           wa=rn(64, 128) * 0.1, ba=0.2 * rn(64), wb=rn(32, 64) * 0.04, bb=0.3 * rn(32)))
    nbytes = ctypes.c_size_t(0)
    fn_ws = 'mv_cam_dense_block_workspace_bytes'
    for label, args in (('bytes = NULL', (1, T2, n, None)), ('B = 0', (0, T2, n, ctypes.byref(nbytes))), ('T2 = 0', (1, 0, n, ctypes.byref(nbytes))),
                        ('nlayers = 0', (1, T2, 0, ctypes.byref(nbytes))), ('nlayers = 25', (1, T2, 25, ctypes.byref(nbytes)))):
        print(f'CALL {fn_ws} {label}', flush=True)
        rc = getattr(cdll, fn_ws)(*args)
        msg = cdll.mv_last_error().decode() if rc != 0 else ''
        log.append((fn_ws, label, None, rc, msg))
        print(f'  -> {"accepted" if rc == 0 else "rejected: " + msg[:120]}', flush=True)
    _hip.check(cdll.mv_cam_dense_block_workspace_bytes(1, T2, n, ctypes.byref(nbytes)), cdll)
    ws = torch.empty(nbytes.value, dtype=torch.uint8)
    arrays = {f: (ctypes.c_void_p * n)(*[L[f].data_ptr() for L in params]) for f in _hip.CAM_LAYER_FIELDS}

    def call(label, **bad):
        buf = torch.zeros(1, T2, c_out + 8, dtype=torch.float16)
        buf[..., :c_in] = x0
        a = dict(x=buf.data_ptr(), ldx=c_out + 8, B=1, T2=T2, c_in=c_in, nlayers=n, dil=dil, seg_len=seg_len, form=1, used=None,
                 ws=ws.data_ptr(), ws_bytes=nbytes.value, **arrays)
        a.update(bad)
        print(f'CALL mv_cam_dense_block_f16 {label}', flush=True)
        rc = cdll.mv_cam_dense_block_f16(a['x'], a['ldx'], a['B'], a['T2'], a['c_in'], a['nlayers'], *[a[f] for f in _hip.CAM_LAYER_FIELDS], a['dil'],
                                         a['seg_len'], a['form'], a['used'], a['ws'], a['ws_bytes'], None)
        msg = cdll.mv_last_error().decode() if rc != 0 else ''
        if label != 'valid':
            log.append(('mv_cam_dense_block_f16', label, None, rc, msg))
        print(f'  -> {"accepted" if rc == 0 else "rejected: " + msg[:120]}', flush=True)
        return rc

    assert call('valid') == 0
    call('x = NULL', x=None)
    call('workspace = NULL', ws=None)
    call('workspace one byte short', ws_bytes=nbytes.value - 1)
    for f in _hip.CAM_LAYER_FIELDS:
        call(f'{f} = NULL', **{f: None})
        holed = (ctypes.c_void_p * n)(*[L[f].data_ptr() for L in params])
        holed[n - 1] = None
        call(f'{f}[{n - 1}] = NULL', **{f: holed})
    for k, vals in (('nlayers', (0, 25, -1)), ('T2', (0, -1)), ('B', (0, -1)), ('ldx', (c_out + 4, c_out - 8, 0, -8)), ('c_in', (0, 100, -32)), ('dil', (0, -1)),
                    ('seg_len', (0, -1)), ('form', (-1, 4))):
        for v in vals:
            call(f'{k} = {v}', **{k: v})
    # each pinned form outside its geometry (the valid call is T2 = 17, c_in = 128, dil 1, seg_len 100)
    call('form 1, dil = 3', form=1, dil=3)
    call('form 1, seg_len = 5 (four segments)', form=1, seg_len=5)
    call('form 2, dil = 3', form=2, dil=3)
    call('form 3, T2 = 17', form=3)
    call('form 0, dil = 3 (no fused form)', form=0, dil=3)


def pool_rows_calls(cdll, log):
    """the layer-level entry points of csrc/pool.hip's reductions and row passes: one small valid call each, every pointer null and every integer 0
    and -1 in turn (the inputs are drawn here: the tool needs nothing of the tests)"""
    import torch
    from mvector import _hip
    g = torch.Generator().manual_seed(23)
    h16 = lambda *s: torch.randn(*s, generator=g).half()
    f32 = lambda *s: torch.randn(*s, generator=g)
    t = lambda name: getattr(TamperArgs(cdll, name, log), name)
    B, T, C, ld = 2, 9, 72, 80
    x = h16(B, T, ld)
    out = torch.zeros(B, 2 * C + 8)
    sc, sh = f32(C), f32(C)
    _hip.check(t('mv_time_stats_ex_f16')(x.data_ptr(), ld, B, T, C, out.data_ptr(), out.data_ptr() + 4 * C, 2 * C + 8, 1, 0.0, sc.data_ptr(), sh.data_ptr(), None), cdll)
    ctx = torch.zeros(B, 3, C)
    _hip.check(t('mv_seg_mean_f16')(x.data_ptr(), ld, B, T, C, 4, ctx.data_ptr(), None), cdll)
    y, gate, cat = h16(B * T, ld), torch.rand(B, C, generator=g), h16(B * T, 2 * C + 16)
    _hip.check(t('mv_se_gate_residual_f16')(y.data_ptr(), ld, gate.data_ptr(), cat.data_ptr() + 16, 2 * C + 16, cat.data_ptr() + 2 * (C + 8), 2 * C + 16, B, T, C,
                                            None), cdll)
    z, rb = h16(B * T, C), f32(B, C)
    _hip.check(t('mv_asp_hidden_act_f16')(z.data_ptr(), rb.data_ptr(), sc.data_ptr(), sh.data_ptr(), B, T, C, None), cdll)
    for F in (16, 13):      # the 16-byte kernel, the ragged kernel
        ldd, pad = (F + 7) // 8 * 8, 2
        feats, dst = f32(B, T, F), torch.zeros(B * (T + 2 * pad) * ldd, dtype=torch.float16)
        _hip.check(t('mv_cast_pad_f16')(feats.data_ptr(), dst.data_ptr(), B, T, F, ldd, pad, None), cdll)
    src, dst = f32(5, 16), torch.zeros(5, 16, dtype=torch.float16)
    _hip.check(t('mv_cast_rows_f16')(src.data_ptr(), 16, dst.data_ptr(), 16, 5, 13, None), cdll)
    s16, d16 = h16(5, 32), torch.zeros(5, 40, dtype=torch.float16)
    _hip.check(t('mv_copy_slice_f16')(s16.data_ptr() + 16, 32, d16.data_ptr() + 16, 40, 16, 5, None), cdll)
    s32, d32 = f32(5, 13), torch.zeros(5, 16)
    _hip.check(t('mv_pad_rows_f32')(s32.data_ptr(), 13, d32.data_ptr(), 16, 5, None), cdll)


def worker(only=''):
    import layer_checks as lc
    from mvector import _hip
    from emu_lib import emu_cdll
    cdll = emu_cdll()
    log = []
    if only in ('', 'cam'):
        cam_dense_block_calls(cdll, log)
    if only == '':
        pool_rows_calls(cdll, log)
    if only == 'pool':
        pool_rows_calls(cdll, log)
        rej = sum(1 for e in log if e[3] != 0)
        print(f'SUMMARY {len(log)} tampered calls: {rej} rejected, {len(log) - rej} accepted, 0 crashed', flush=True)
        print('ACCEPTED ' + '; '.join(f'{e[0]}.{e[1]}={e[2]!r}' for e in log if e[3] == 0), flush=True)
        return
    if only == 'cam':
        rej = sum(1 for e in log if e[3] != 0)
        print(f'SUMMARY {len(log)} tampered calls: {rej} rejected, {len(log) - rej} accepted, 0 crashed', flush=True)
        print('ACCEPTED ' + '; '.join(f'{e[0]}.{e[1]}' for e in log if e[3] == 0), flush=True)
        return
    # one valid layer per entry point, small enough that an "accepted" variant costs little
    lc.conv1d_case(Tamper(cdll, 'mv_conv1d_forward', _hip.MvConv1dDesc, log), 'cpu', B=2, T=21, cin=24, cout=40, k=3, dil=2, with_x2=True, row_bias=True)
    lc.conv1d_case(Tamper(cdll, 'mv_conv1d_forward', _hip.MvConv1dDesc, log), 'cpu', B=5, T=90, cin=128, cout=256, k=1, dil=1, tile=256, stats=2)
    lc.conv2ds_case(Tamper(cdll, 'mv_conv2ds_forward', _hip.MvConv2dsDesc, log), 'cpu', B=1, H=5, W=9, cin=16, cout=32, ks=3, with_res=True, with_sum=True)
    lc.conv2ds_case(Tamper(cdll, 'mv_conv2ds_forward', _hip.MvConv2dsDesc, log), 'cpu', B=1, H=4, W=9, cin=64, cout=16, ks=1, concat=True, epi=1)
    import torch
    lc.linear_case(TamperArgs(cdll, 'mv_linear_f32', log), 'cpu', B=3, K=40, O=12)
    lc.time_stats_case(TamperArgs(cdll, 'mv_time_stats_f16', log), 'cpu', B=2, T=9, C=72, ld=80)
    lc.asp_pool_case(TamperArgs(cdll, 'mv_asp_pool_f16', log), 'cpu', B=2, T=20, C=72, A=64)
    lc.res2_chain_case(TamperArgs(cdll, 'mv_res2net_chain_f16', log), 'cpu', B=1, T=20, width=64, dil=2)
    lc.bn_relu_rows_case(TamperArgs(cdll, 'mv_bn_relu_rows_f16', log), 'cpu', rows=9, C=72, ldx=80, ldy=88)
    lc.tstp_case(TamperArgs(cdll, 'mv_tstp_f32', log), 'cpu', B=2, H=3, W=10, C=16)
    lc.wave_prepare_case(TamperArgs(cdll, 'mv_wave_prepare_i16', log), 'cpu', B=2, L=300)
    a, b = torch.randn(5, 16), torch.randn(7, 16)
    lc.cosine_case(TamperArgs(cdll, 'mv_cosine_f32', log), 'cpu', a.numpy(), b.numpy(),
                   (torch.nn.functional.normalize(a, dim=1) @ torch.nn.functional.normalize(b, dim=1).t()).numpy())
    rej = sum(1 for e in log if e[3] != 0)
    print(f'SUMMARY {len(log)} tampered calls: {rej} rejected, {len(log) - rej} accepted, 0 crashed', flush=True)
    acc = sorted({(e[0], e[1], e[2]) for e in log if e[3] == 0})
    print('ACCEPTED ' + '; '.join(f'{f}.{k}={v!r}' for f, k, v in acc), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', default='plain', choices=['plain', 'asan', 'ubsan'])
    ap.add_argument('--only', default='', choices=['', 'cam', 'pool'],
                    help='cam: the CAM++ dense-block entry points alone (what tests/test_cam_dense.py runs); pool: the row passes of pool.hip (tests/test_pool_rows.py)')
    ap.add_argument('--worker', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        worker(args.only)
        return
    import emu_fuzz
    env = emu_fuzz.mode_env(args.mode)
    subprocess.check_call([sys.executable, os.path.join(ROOT, 'tests', 'emu', 'build_emu.py')], env={**env, 'LD_PRELOAD': ''}, stdout=subprocess.DEVNULL)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--worker', '--only', args.only], env=env, cwd=ROOT, capture_output=True, text=True)
    lines = r.stdout.splitlines()
    if r.returncode != 0 or not any(l.startswith('SUMMARY') for l in lines):
        calls = [l for l in lines if l.startswith('CALL')]
        print(f'{args.mode}: the process died (rc {r.returncode}) in: {calls[-1] if calls else "?"}')
        print('\n'.join(l for l in (r.stdout + r.stderr).splitlines() if 'ERROR' in l or ' #0 ' in l or ' #1 ' in l or 'located' in l or 'SUMMARY' in l))
        if 'Traceback' in r.stderr:              # the worker itself raised: say where
            print(r.stderr[-1500:])
        sys.exit(1)
    for l in lines:
        if l.startswith(('SUMMARY', 'ACCEPTED')):
            print(f'{args.mode}: {l}')


if __name__ == '__main__':
    main()
