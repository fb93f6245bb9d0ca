"""ctypes binding of libmvector_hip.so (the C ABI declared in include/mvector_hip.h).

This is the only place the Python package touches native code.  There is NO fallback: if the library is
missing or a call fails, a RuntimeError carrying ``mv_last_error()`` is raised.  Tensors are passed as raw
``data_ptr()`` values together with the current HIP stream; PyTorch is used for device memory and streams only.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'lib', 'libmvector_hip.so')

MV_ACT_NONE, MV_ACT_RELU, MV_ACT_TANH, MV_ACT_SIGMOID = 0, 1, 2, 3
MV_PAD_ZERO, MV_PAD_REFLECT = 0, 1
MV_DT_F32, MV_DT_F16 = 0, 1
MV_POOL_ASP, MV_POOL_SAP, MV_POOL_TAP, MV_POOL_TSP = 0, 1, 2, 3
POOLING_TYPES = {'ASP': MV_POOL_ASP, 'SAP': MV_POOL_SAP, 'TAP': MV_POOL_TAP, 'TSP': MV_POOL_TSP}   # the reference's `pooling_type` strings

c_i32, c_i64, c_f32, c_vp, c_sz = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t


class MvFbankCfg(ctypes.Structure):
    _fields_ = [('sample_frequency', c_f32), ('frame_length_ms', c_f32), ('frame_shift_ms', c_f32),
                ('num_mel_bins', c_i32), ('low_freq', c_f32), ('high_freq', c_f32),
                ('preemphasis_coefficient', c_f32), ('remove_dc_offset', c_i32), ('use_power', c_i32),
                ('use_log_fbank', c_i32), ('subtract_time_mean', c_i32), ('window_type', c_i32), ('blackman_coeff', c_f32),
                ('snip_edges', c_i32), ('subtract_mean', c_i32), ('min_duration', c_f32), ('vtln_warp', c_f32), ('vtln_low', c_f32),
                ('vtln_high', c_f32), ('kernel', c_i32), ('min_samples', c_i64), ('use_energy', c_i32), ('raw_energy', c_i32),
                ('energy_floor', c_f32), ('htk_compat', c_i32)]


class MvMelSpecCfg(ctypes.Structure):
    _fields_ = [('sample_rate', c_i32), ('n_fft', c_i32), ('win_length', c_i32), ('hop_length', c_i32),
                ('f_min', c_f32), ('f_max', c_f32), ('n_mels', c_i32), ('power', c_f32), ('center', c_i32),
                ('subtract_time_mean', c_i32), ('mel_scale', c_i32), ('norm', c_i32), ('normalized', c_i32), ('window', c_vp),
                ('pad', c_i32), ('pad_mode', c_i32)]


class MvSpectrogramCfg(ctypes.Structure):
    _fields_ = [('n_fft', c_i32), ('win_length', c_i32), ('hop_length', c_i32), ('pad', c_i32), ('power', c_f32), ('normalized', c_i32),
                ('center', c_i32), ('pad_mode', c_i32), ('subtract_time_mean', c_i32), ('window', c_vp)]


class MvMfccCfg(ctypes.Structure):
    _fields_ = [('mel', MvMelSpecCfg), ('n_mfcc', c_i32), ('dct_norm', c_i32), ('log_mels', c_i32), ('top_db', c_f32),
                ('subtract_time_mean', c_i32)]


MV_HFENC_MAX_LAYERS = 8
MV_HF_NORM_GROUP, MV_HF_NORM_LAYER = 0, 1
MV_ACT_GELU = 4
MV_HF_ROWS_GELU, MV_HF_ROWS_LN_GELU, MV_HF_ROWS_LN_F32 = 0, 1, 2


class MvHfEncoderCfg(ctypes.Structure):
    _fields_ = [('num_layers', c_i32), ('conv_dim', c_i32 * MV_HFENC_MAX_LAYERS), ('conv_kernel', c_i32 * MV_HFENC_MAX_LAYERS),
                ('conv_stride', c_i32 * MV_HFENC_MAX_LAYERS), ('feat_extract_norm', c_i32), ('conv_bias', c_i32), ('do_normalize', c_i32),
                ('activation', c_i32), ('layer_norm_eps', c_f32), ('subtract_time_mean', c_i32)]


class MvW2vBertCfg(ctypes.Structure):
    _fields_ = [('num_mel_bins', c_i32), ('stride', c_i32), ('sampling_rate', c_i32), ('layer_norm_eps', c_f32), ('subtract_time_mean', c_i32)]


class MvTensorRef(ctypes.Structure):
    _fields_ = [('name', ctypes.c_char_p), ('data', c_vp), ('numel', c_i64)]


class MvEcapaCfg(ctypes.Structure):
    _fields_ = [('input_size', c_i32), ('embd_dim', c_i32), ('channels', c_i32 * 5), ('kernel_sizes', c_i32 * 5),
                ('dilations', c_i32 * 5), ('attention_channels', c_i32), ('res2net_scale', c_i32),
                ('se_channels', c_i32), ('global_context', c_i32)]


MV_ECAPA_MAX_BLOCKS = 16
MV_INFO_ECAPA_GROUPED_NATIVE, MV_INFO_ECAPA_GROUPED_EXPANDED, MV_INFO_ECAPA_EXPANDED_1X1, MV_INFO_ECAPA_BLOCKS = 20, 21, 22, 23


class MvEcapaCfgEx(ctypes.Structure):
    """EcapaTdnn with N = nblocks SE-Res2Net blocks and per-layer groups (mv_ecapa_create_ex): arrays of N + 2 used entries"""
    _fields_ = [('input_size', c_i32), ('embd_dim', c_i32), ('nblocks', c_i32), ('channels', c_i32 * (MV_ECAPA_MAX_BLOCKS + 2)),
                ('kernel_sizes', c_i32 * (MV_ECAPA_MAX_BLOCKS + 2)), ('dilations', c_i32 * (MV_ECAPA_MAX_BLOCKS + 2)),
                ('groups', c_i32 * (MV_ECAPA_MAX_BLOCKS + 2)), ('attention_channels', c_i32), ('res2net_scale', c_i32),
                ('se_channels', c_i32), ('global_context', c_i32)]


class MvCamppCfg(ctypes.Structure):
    _fields_ = [('input_size', c_i32), ('embd_dim', c_i32), ('growth_rate', c_i32), ('bn_size', c_i32),
                ('init_channels', c_i32), ('head_precision', c_i32), ('xvector_probe', c_i32)]


class MvEres2Cfg(ctypes.Structure):
    _fields_ = [('version', c_i32), ('input_size', c_i32), ('embd_dim', c_i32), ('num_blocks', c_i32 * 4),
                ('m_channels', c_i32), ('mul_channel', c_i32), ('expansion', c_i32), ('base_width', c_i32),
                ('scale', c_i32), ('two_emb_layer', c_i32)]


MV_RESNETSE_NO_PEAK = 0x100   # or-ed into MvResNetSeCfg.pooling_type: a handle without the saturation word (tools that time what it costs)
MV_INFO_S16_PEAK, MV_INFO_S16_SATURATED = 30, 31   # ResNetSE and Res2Net handles: the range of their S16 maps since create
MV_INFO_RESNETSE_PEAK, MV_INFO_RESNETSE_SATURATED = MV_INFO_S16_PEAK, MV_INFO_S16_SATURATED   # (the names the keys were introduced under)
MV_RES2NET_NO_PEAK = 0x100    # or-ed into MvRes2NetCfg.pooling_type, as MV_RESNETSE_NO_PEAK
MV_SE2D_SQUEEZE_CHUNK = 256   # pixels per partial sum of mv_se2d_squeeze_s16


class MvResNetSeCfg(ctypes.Structure):
    _fields_ = [('input_size', c_i32), ('layers', c_i32 * 4), ('num_filters', c_i32 * 4), ('embd_dim', c_i32), ('pooling_type', c_i32),
                ('reduction', c_i32)]


class MvRes2NetCfg(ctypes.Structure):
    _fields_ = [('input_size', c_i32), ('m_channels', c_i32), ('layers', c_i32 * 4), ('base_width', c_i32), ('scale', c_i32), ('embd_dim', c_i32),
                ('pooling_type', c_i32)]


class MvConv2dsDesc(ctypes.Structure):
    _fields_ = [('x', c_vp), ('x2', c_vp), ('cin1', c_i32), ('ldx', c_i64), ('ldx2', c_i64), ('w', c_vp), ('bias', c_vp),
                ('oscale', c_f32), ('res', c_vp), ('res2', c_vp), ('ldres', c_i64), ('ldres2', c_i64), ('add', c_vp),
                ('ldadd', c_i64), ('y', c_vp), ('ldy', c_i64), ('y2', c_vp), ('ldy2', c_i64), ('B', c_i32), ('H', c_i32),
                ('W', c_i32), ('cin16', c_i32), ('cout16', c_i32), ('ks', c_i32), ('stride', c_i32), ('epi', c_i32),
                ('lo', c_f32), ('hi', c_f32), ('cin_alg', c_i32), ('cout_alg', c_i32), ('stride_w', c_i32), ('peak', c_vp), ('nbw_hint', c_i32),
                ('ct_hint', c_i32), ('rows_hint', c_i32), ('ring_hint', c_i32), ('wgs_hint', c_i32), ('spw_hint', c_i32), ('nprod_hint', c_i32),
                ('wg_hint', c_i32)]


class MvConv2dsPlanInfo(ctypes.Structure):
    """what a conv2ds forward would launch (mv_conv2ds_plan_info): the row of csrc/conv2ds.hip's kernel table by name, and the launch shape"""
    _fields_ = [('kernel', ctypes.c_char_p), ('nbw', c_i32), ('spw', c_i32), ('track', c_i32), ('ncons', c_i32), ('nprod', c_i32), ('ns', c_i32),
                ('pp', c_i32), ('wgs_per_cu', c_i32), ('rows', c_i32), ('ct', c_i32), ('ctiles', c_i32), ('tiles', c_i32), ('wg_per_ct', c_i32),
                ('grid', c_i32), ('stages_per_tile', c_i32), ('lds_bytes', c_i32)]


class MvTdnnCfg(ctypes.Structure):
    _fields_ = [('input_size', c_i32), ('channels', c_i32), ('embd_dim', c_i32)]


class MvConv1dDesc(ctypes.Structure):
    _fields_ = [('x', c_vp), ('x2', c_vp), ('x_dtype', c_i32), ('ldx', c_i64), ('ldx2', c_i64), ('in_scale', c_vp),
                ('in_shift', c_vp), ('w_packed', c_vp), ('bias', c_vp), ('row_bias', c_vp), ('pre_act', c_i32),
                ('scale', c_vp), ('shift', c_vp), ('post_act', c_i32), ('gate', c_vp), ('gate_seg_len', c_i32),
                ('y', c_vp), ('y_dtype', c_i32), ('ldy', c_i64), ('add_src', c_vp), ('sum_dst', c_vp), ('ld_add', c_i64),
                ('ld_sum', c_i64), ('B', c_i32), ('T_in', c_i32), ('T_out', c_i32),
                ('cin', c_i32), ('cout', c_i32), ('k', c_i32), ('dilation', c_i32), ('stride', c_i32), ('pad', c_i32),
                ('pad_mode', c_i32), ('tile', c_i32), ('stat_sum', c_vp), ('stat_sq', c_vp), ('in_stat_sum', c_vp), ('in_stat_sq', c_vp),
                ('persist_blocks_hint', c_i32), ('clock_probe', c_vp)]


class MvConv1dPlanInfo(ctypes.Structure):
    """what a conv1d forward would launch (mv_conv1d_plan_info): rows of csrc/conv1d.hip's kernel table by name, b'' where there is no such launch"""
    _fields_ = [('kernel', ctypes.c_char_p), ('in_stats_kernel', ctypes.c_char_p), ('tail_kernel', ctypes.c_char_p),
                ('n_tiles', c_i32), ('co_tiles', c_i32), ('grid', c_i32), ('tail_nv', c_i32), ('tail_split', c_i32)]


class MvEigCfg(ctypes.Structure):
    _fields_ = [('m', c_i32), ('block', c_i32), ('degree', c_i32), ('max_iters', c_i32), ('tol', ctypes.c_double), ('seed', ctypes.c_uint64)]


class MvEigInfo(ctypes.Structure):
    _fields_ = [('iterations', c_i32), ('products', c_i32), ('retries', c_i32), ('converged', c_i32), ('residual', ctypes.c_double),
                ('ub', ctypes.c_double)]


class MvResamplerInfo(ctypes.Structure):
    _fields_ = [('up', c_i32), ('down', c_i32), ('half', c_i32), ('K', c_i32), ('tile', c_i32), ('table_in_lds', c_i32)]


class MvVerifCfg(ctypes.Structure):
    _fields_ = [('p_target', ctypes.c_double), ('c_miss', ctypes.c_double), ('c_fa', ctypes.c_double)]


class MvVadCfg(ctypes.Structure):
    _fields_ = [('frame_length', c_i32), ('frame_shift', c_i32), ('frames_context', c_i32), ('reserved', c_i32),
                ('energy_threshold', ctypes.c_double), ('energy_mean_scale', ctypes.c_double), ('proportion_threshold', ctypes.c_double),
                ('scale', ctypes.c_double)]


class MvVadSmoothCfg(ctypes.Structure):
    _fields_ = [('frame_shift', c_i32), ('min_silence', c_i32), ('min_speech', c_i32), ('speech_pad', c_i32)]   # samples


class MvVerifResult(ctypes.Structure):
    _fields_ = [('n_target', c_i64), ('n_impostor', c_i64), ('i1', c_i64), ('i2', c_i64), ('tgt_i1', c_i64), ('tgt_i2', c_i64),
                ('min_cost', ctypes.c_double), ('score_i1', c_f32), ('reserved', c_i32)]


_SIGNATURES = {
    'mv_last_error': (ctypes.c_char_p, []),
    'mv_abi_version': (c_i32, []),
    'mv_fbank_default_cfg': (None, [ctypes.POINTER(MvFbankCfg)]),
    'mv_fbank_create': (c_i32, [ctypes.POINTER(MvFbankCfg), ctypes.POINTER(c_vp)]),
    'mv_fbank_destroy': (c_i32, [c_vp]),
    'mv_fbank_info': (c_i32, [c_vp, ctypes.POINTER(c_i32), ctypes.POINTER(c_i32)]),
    'mv_fbank_num_frames': (c_i32, [c_vp, c_i64, ctypes.POINTER(c_i64)]),
    'mv_fbank_forward': (c_i32, [c_vp, c_vp, c_i32, c_i64, c_i64, c_vp, c_vp, c_vp]),
    'mv_fbank_forward_varlen': (c_i32, [c_vp, c_vp, c_i32, c_i64, c_i64, c_vp, c_vp, c_vp]),
    'mv_fbank_forward_varlen_ws': (c_i32, [c_vp, c_vp, c_i32, c_i64, c_i64, c_vp, c_vp, c_vp, ctypes.c_size_t, c_vp]),
    'mv_fbank_workspace_bytes': (c_i32, [c_vp, c_i32, c_i64, ctypes.POINTER(ctypes.c_size_t)]),
    'mv_fbank_forward_ws': (c_i32, [c_vp, c_vp, c_i32, c_i64, c_i64, c_vp, c_vp, c_vp, ctypes.c_size_t, c_vp]),
    'mv_melspec_default_cfg': (None, [ctypes.POINTER(MvMelSpecCfg)]),
    'mv_melspec_create': (c_i32, [ctypes.POINTER(MvMelSpecCfg), ctypes.POINTER(c_vp)]),
    'mv_melspec_info': (c_i32, [c_vp, ctypes.POINTER(c_i32)]),
    'mv_melspec_destroy': (c_i32, [c_vp]),
    'mv_melspec_num_frames': (c_i32, [c_vp, c_i64, ctypes.POINTER(c_i64)]),
    'mv_melspec_workspace_bytes': (c_sz, [c_vp, c_i32, c_i64]),
    'mv_melspec_forward': (c_i32, [c_vp, c_vp, c_i32, c_i64, c_i64, c_vp, c_vp, c_vp, c_sz, c_vp]),
    'mv_melspec_forward_varlen': (c_i32, [c_vp, c_vp, c_i32, c_i64, c_i64, c_vp, c_vp, c_vp, c_sz, c_vp]),
    'mv_ecapa_create': (c_i32, [ctypes.POINTER(MvEcapaCfg), ctypes.POINTER(MvTensorRef), c_i32, ctypes.POINTER(c_vp)]),
    'mv_campp_create': (c_i32, [ctypes.POINTER(MvCamppCfg), ctypes.POINTER(MvTensorRef), c_i32, ctypes.POINTER(c_vp)]),
    'mv_tdnn_create': (c_i32, [ctypes.POINTER(MvTdnnCfg), ctypes.POINTER(MvTensorRef), c_i32, ctypes.POINTER(c_vp)]),
    'mv_ecapa_create_pooled': (c_i32, [ctypes.POINTER(MvEcapaCfg), c_i32, ctypes.POINTER(MvTensorRef), c_i32, ctypes.POINTER(c_vp)]),
    'mv_tdnn_create_pooled': (c_i32, [ctypes.POINTER(MvTdnnCfg), c_i32, ctypes.POINTER(MvTensorRef), c_i32, ctypes.POINTER(c_vp)]),
    'mv_ecapa_create_ex': (c_i32, [ctypes.POINTER(MvEcapaCfgEx), c_i32, ctypes.POINTER(MvTensorRef), c_i32, ctypes.POINTER(c_vp)]),
    'mv_eres2net_create': (c_i32, [ctypes.POINTER(MvEres2Cfg), ctypes.POINTER(MvTensorRef), c_i32, ctypes.POINTER(c_vp)]),
    'mv_resnetse_create': (c_i32, [ctypes.POINTER(MvResNetSeCfg), ctypes.POINTER(MvTensorRef), c_i32, ctypes.POINTER(c_vp)]),
    'mv_se2d_squeeze_workspace_floats': (c_sz, [c_i32, c_i32, c_i32, c_i32]),
    'mv_se2d_squeeze_s16': (c_i32, [c_vp, c_i64, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_sz, c_vp]),
    'mv_se2d_excite_f32': (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp]),
    'mv_se2d_gate_res_relu_s16': (c_i32, [c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_i64, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    'mv_s16_map_to_rows_f16': (c_i32, [c_vp, c_i64, c_i32, c_i32, c_i32, c_i32, c_vp, c_i64, c_vp]),
    'mv_res2net_create': (c_i32, [ctypes.POINTER(MvRes2NetCfg), ctypes.POINTER(MvTensorRef), c_i32, ctypes.POINTER(c_vp)]),
    'mv_conv2d_stem7_s16': (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp]),
    'mv_conv2d_stem7_peak_s16': (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    'mv_maxpool3s2_s16': (c_i32, [c_vp, c_i64, c_vp, c_i64, c_i32, c_i32, c_i32, c_i32, c_vp]),
    'mv_avgpool3_s16': (c_i32, [c_vp, c_i64, c_vp, c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp]),
    'mv_conv2d_first': (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp]),
    'mv_tstp_f32': (c_i32, [c_vp, c_i64, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    'mv_conv2ds_packed_elems': (c_i64, [c_i32, c_i32, c_i32]),
    'mv_conv2ds_pack_weight': (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, ctypes.POINTER(c_f32), c_vp]),
    'mv_conv2ds_forward': (c_i32, [ctypes.POINTER(MvConv2dsDesc), c_vp]),
    'mv_conv2ds_plan_info': (c_i32, [ctypes.POINTER(MvConv2dsDesc), c_i32, ctypes.POINTER(MvConv2dsPlanInfo)]),
    'mv_map_split_f32': (c_i32, [c_vp, c_vp, c_i64, c_vp]),
    'mv_map_merge_f32': (c_i32, [c_vp, c_vp, c_i64, c_vp]),
    'mv_conv2d_first_s16': (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp]),
    'mv_tstp_s16': (c_i32, [c_vp, c_i64, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    'mv_model_destroy': (c_i32, [c_vp]),
    'mv_model_embd_dim': (c_i32, [c_vp, ctypes.POINTER(c_i32)]),
    'mv_model_info': (c_i32, [c_vp, c_i32, ctypes.POINTER(c_f32)]),
    'mv_model_workspace_bytes': (c_i32, [c_vp, c_i32, c_i32, ctypes.POINTER(c_sz)]),
    'mv_model_forward': (c_i32, [c_vp, c_vp, c_i32, c_i32, c_vp, c_vp, c_sz, c_vp]),
    'mv_cosine_f32': (c_i32, [c_vp, c_i32, c_vp, c_i32, c_i32, c_vp, c_vp]),
    'mv_l2_normalize_f32': (c_i32, [c_vp, c_i32, c_i32, c_vp]),
    'mv_cosine_topk_workspace_bytes': (c_sz, [c_i32, c_i32, c_i32, c_i32, c_i32]),
    'mv_cosine_topk_f32': (c_i32, [c_vp, c_i32, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_i32, c_vp, c_sz, c_vp]),
    'mv_conv1d_packed_elems': (c_i64, [c_i32, c_i32, c_i32]),
    'mv_conv1d_pack_weight': (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp]),
    'mv_conv1d_forward': (c_i32, [ctypes.POINTER(MvConv1dDesc), c_vp]),
    'mv_conv1d_grouped_native': (c_i32, [c_i32, c_i32, c_i32, c_i32]),
    'mv_conv1d_grouped_packed_elems': (c_i64, [c_i32, c_i32, c_i32, c_i32]),
    'mv_conv1d_pack_weight_grouped': (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    'mv_conv1d_forward_grouped': (c_i32, [ctypes.POINTER(MvConv1dDesc), c_i32, c_vp]),
    'mv_conv1d_plan_info': (c_i32, [ctypes.POINTER(MvConv1dDesc), c_i32, c_i32, ctypes.POINTER(MvConv1dPlanInfo)]),
    'mv_conv1d_stats_elems': (c_i64, [c_i32, c_i32, c_i32]),
    'mv_conv1d_in_stats_elems': (c_i64, [c_i32, c_i32, c_i32]),
    'mv_conv1d_in_stats_finish': (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_i64, c_f32, c_vp]),
    'mv_conv1d_stats_finish': (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_i64, c_f32, c_vp]),
    'mv_res2net_chain_f16': (c_i32, [c_vp, c_vp, ctypes.POINTER(c_vp), ctypes.POINTER(c_vp), ctypes.POINTER(c_vp),
                             ctypes.POINTER(c_vp), c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp]),
    'mv_linear_f32': (c_i32, [c_vp, c_i64, c_vp, c_vp, c_i32, c_vp, c_i64, c_i32, c_i32, c_i32, c_vp]),
    'mv_linear_f32_workspace_floats': (c_sz, [c_i32, c_i32, c_i32]),
    'mv_linear_f32_ws': (c_i32, [c_vp, c_i64, c_vp, c_vp, c_i32, c_vp, c_i64, c_i32, c_i32, c_i32, c_vp, c_sz, c_vp]),
    'mv_profile_enable': (c_i32, [c_i32]),
    'mv_profile_read': (c_i32, [c_i32, ctypes.POINTER(c_i32), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), c_i32]),
    'mv_wave_prepare_i16': (c_i32, [c_vp, c_i64, c_vp, c_i32, c_i64, c_i32, c_f32, c_f32, c_vp, c_i64, c_vp, c_vp]),
    'mv_resampler_create': (c_i32, [c_i32, c_i32, ctypes.POINTER(c_vp)]),
    'mv_resampler_destroy': (c_i32, [c_vp]),
    'mv_resampler_info': (c_i32, [c_vp, ctypes.POINTER(MvResamplerInfo)]),
    'mv_resampler_taps': (c_i32, [c_vp, ctypes.POINTER(c_f32), c_i32]),
    'mv_resampler_out_len': (c_i64, [c_vp, c_i64]),
    'mv_resampler_workspace_bytes': (c_sz, [c_vp, c_i32, c_i64]),
    'mv_resampler_forward_i16': (c_i32, [c_vp, c_vp, c_i64, c_i32, c_vp, c_i32, c_i64, c_i32, c_f32, c_f32, c_vp, c_i64, c_i64, c_vp, c_vp, c_vp, c_sz,
                                         c_vp]),
    'mv_asp_pool_f16': (c_i32, [c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp]),
    'mv_sap_pool_f16': (c_i32, [c_vp, c_vp, c_vp, c_i64, c_vp, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp]),
    'mv_time_mean_var_f16': (c_i32, [c_vp, c_i64, c_i32, c_i32, c_i32, c_vp, c_i64, c_vp]),
    'mv_spectrogram_default_cfg': (None, [ctypes.POINTER(MvSpectrogramCfg)]),
    'mv_spectrogram_create': (c_i32, [ctypes.POINTER(MvSpectrogramCfg), ctypes.POINTER(c_vp)]),
    'mv_spectrogram_info': (c_i32, [c_vp, ctypes.POINTER(c_i32)]),
    'mv_spectrogram_destroy': (c_i32, [c_vp]),
    'mv_spectrogram_num_frames': (c_i32, [c_vp, c_i64, ctypes.POINTER(c_i64)]),
    'mv_spectrogram_workspace_bytes': (c_sz, [c_vp, c_i32, c_i64]),
    'mv_spectrogram_forward': (c_i32, [c_vp, c_vp, c_i32, c_i64, c_i64, c_vp, c_vp, c_vp, c_sz, c_vp]),
    'mv_spectrogram_forward_varlen': (c_i32, [c_vp, c_vp, c_i32, c_i64, c_i64, c_vp, c_vp, c_vp, c_sz, c_vp]),
    'mv_mfcc_default_cfg': (None, [ctypes.POINTER(MvMfccCfg)]),
    'mv_mfcc_create': (c_i32, [ctypes.POINTER(MvMfccCfg), ctypes.POINTER(c_vp)]),
    'mv_mfcc_info': (c_i32, [c_vp, ctypes.POINTER(c_i32), ctypes.POINTER(c_i32)]),
    'mv_mfcc_destroy': (c_i32, [c_vp]),
    'mv_mfcc_num_frames': (c_i32, [c_vp, c_i64, ctypes.POINTER(c_i64)]),
    'mv_mfcc_workspace_bytes': (c_sz, [c_vp, c_i32, c_i64]),
    'mv_mfcc_forward': (c_i32, [c_vp, c_vp, c_i32, c_i64, c_i64, c_vp, c_vp, c_vp, c_sz, c_vp]),
    'mv_mfcc_forward_varlen': (c_i32, [c_vp, c_vp, c_i32, c_i64, c_i64, c_vp, c_vp, c_vp, c_sz, c_vp]),
    'mv_hfenc_default_cfg': (None, [ctypes.POINTER(MvHfEncoderCfg)]),
    'mv_hfenc_create': (c_i32, [ctypes.POINTER(MvHfEncoderCfg), ctypes.POINTER(MvTensorRef), c_i32, ctypes.POINTER(c_vp)]),
    'mv_hfenc_destroy': (c_i32, [c_vp]),
    'mv_hfenc_num_frames': (c_i32, [c_vp, c_i64, ctypes.POINTER(c_i64)]),
    'mv_hfenc_workspace_bytes': (c_i32, [c_vp, c_i32, c_i64, ctypes.POINTER(c_sz)]),
    'mv_hfenc_forward': (c_i32, [c_vp, c_vp, c_i32, c_i64, c_i64, c_vp, c_vp, c_vp, c_sz, c_vp]),
    'mv_hfenc_forward_varlen': (c_i32, [c_vp, c_vp, c_i32, c_i64, c_i64, c_vp, c_vp, c_vp, c_sz, c_vp]),
    'mv_hfenc_forward_timed': (c_i32, [c_vp, c_vp, c_i32, c_i64, c_i64, c_vp, c_vp, c_vp, c_sz, c_vp, ctypes.POINTER(c_f32), c_i32]),
    'mv_hfenc_wave_stats': (c_i32, [c_vp, c_i32, c_i64, c_i64, c_vp, c_vp, c_vp]),
    'mv_hfenc_layer0_workspace_bytes': (c_i32, [c_i32, c_i64, c_i32, c_i32, c_i32, ctypes.POINTER(c_sz)]),
    'mv_hfenc_layer0': (c_i32, [c_vp, c_i32, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_sz, c_vp]),
    'mv_hfenc_rows': (c_i32, [c_vp, c_vp, c_vp, c_vp, c_f32, c_i64, c_i32, c_i32, c_vp]),
    'mv_hfenc_cmn_mask': (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_i64, ctypes.POINTER(c_i32), ctypes.POINTER(c_i32), c_i32, c_i32, c_vp]),
    'mv_w2vbert_create': (c_i32, [ctypes.POINTER(MvW2vBertCfg), c_vp, c_vp, ctypes.POINTER(c_vp)]),
    'mv_w2vbert_destroy': (c_i32, [c_vp]),
    'mv_w2vbert_num_frames': (c_i32, [c_vp, c_i64, ctypes.POINTER(c_i64)]),
    'mv_w2vbert_workspace_bytes': (c_i32, [c_vp, c_i32, c_i64, ctypes.POINTER(c_sz)]),
    'mv_w2vbert_forward': (c_i32, [c_vp, c_vp, c_i32, c_i64, c_i64, c_vp, c_vp, c_vp, c_sz, c_vp]),
    'mv_w2vbert_forward_varlen': (c_i32, [c_vp, c_vp, c_i32, c_i64, c_i64, c_vp, c_vp, c_vp, c_sz, c_vp]),
    'mv_w2vbert_binstats_f32': (c_i32, [c_vp, c_i32, c_i32, c_vp, c_i64, c_vp, c_vp, c_vp]),
    'mv_w2vbert_rows_f32': (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_f32, c_i32, c_i32, c_vp, c_i64, c_vp, c_vp]),
    'mv_w2vbert_cmn_mask_f32': (c_i32, [c_vp, c_i32, c_i32, c_vp, c_vp, c_i64, c_i32, c_vp]),
    'mv_fcm_conv3x3_f16': (c_i32, [c_vp, c_i32, c_i32, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_i32, c_i32, c_i32, c_vp]),
    'mv_fcm_block_f16': (c_i32, [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_i64, c_i64, c_i64, c_i32, c_i32, c_vp]),
    'mv_fcm_block_c1_f16': (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_i32, c_i32, c_vp]),
    'mv_fcm_c1_pack': (c_i32, [c_vp, c_vp]),
    'mv_time_stats_f16': (c_i32, [c_vp, c_i64, c_i32, c_i32, c_i32, c_vp, c_vp, c_i32, c_f32, c_vp]),
    'mv_bn_relu_rows_f16': (c_i32, [c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_i64, c_i32, c_vp]),
    'mv_time_stats_ex_f16': (c_i32, [c_vp, c_i64, c_i32, c_i32, c_i32, c_vp, c_vp, c_i64, c_i32, c_f32, c_vp, c_vp, c_vp]),
    'mv_seg_mean_f16': (c_i32, [c_vp, c_i64, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    'mv_se_gate_residual_f16': (c_i32, [c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_i64, c_i32, c_i32, c_i32, c_vp]),
    'mv_asp_hidden_act_f16': (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp]),
    'mv_cast_pad_f16': (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i64, c_i32, c_vp]),
    'mv_cast_rows_f16': (c_i32, [c_vp, c_i64, c_vp, c_i64, c_i64, c_i32, c_vp]),
    'mv_copy_slice_f16': (c_i32, [c_vp, c_i64, c_vp, c_i64, c_i32, c_i64, c_vp]),
    'mv_pad_rows_f32': (c_i32, [c_vp, c_i32, c_vp, c_i64, c_i64, c_vp]),
    'mv_cam_dense_block_workspace_bytes': (c_i32, [c_i32, c_i32, c_i32, ctypes.POINTER(c_sz)]),
    'mv_cam_dense_block_f16': (c_i32, [c_vp, c_i64, c_i32, c_i32, c_i32, c_i32] + [ctypes.POINTER(c_vp)] * 10 +
                               [c_i32, c_i32, c_i32, ctypes.POINTER(c_i32), c_vp, c_sz, c_vp]),
    'mv_wave_chunks_f32': (c_i32, [c_vp, c_i64, c_vp, c_vp, c_i32, c_i64, c_i32, c_f32, c_f32, c_vp, c_i64, c_vp, c_vp]),
    'mv_affinity_laplacian_workspace_bytes': (c_sz, [c_i32]),
    'mv_affinity_laplacian_f32': (c_i32, [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_sz, c_vp]),
    'mv_laplacian_eig_default_cfg': (None, [ctypes.POINTER(MvEigCfg)]),
    'mv_laplacian_eig_lowest_workspace_bytes': (c_sz, [c_i32, ctypes.POINTER(MvEigCfg)]),
    'mv_laplacian_eig_lowest': (c_i32, [c_vp, c_vp, c_i32, ctypes.POINTER(MvEigCfg), ctypes.POINTER(ctypes.c_double), c_vp,
                                        ctypes.POINTER(MvEigInfo), c_vp, c_sz, c_vp]),
    'mv_sort_scores_tile': (c_i32, []),
    'mv_sort_scores_workspace_bytes': (c_sz, [c_i64]),
    'mv_sort_scores_f32': (c_i32, [c_vp, c_i64, c_vp, c_vp, c_vp, c_sz, c_vp]),
    'mv_verif_metrics_workspace_bytes': (c_sz, [c_i64, c_i64]),
    'mv_verif_metrics_f32': (c_i32, [c_vp, c_i64, c_i64, c_vp, c_vp, ctypes.POINTER(MvVerifCfg), ctypes.POINTER(MvVerifResult), c_vp, c_vp,
                                     c_vp, c_sz, c_vp]),
    'mv_cohort_stats_workspace_bytes': (c_sz, [c_i32, c_i32, c_i32, c_i32]),
    'mv_cohort_stats_f32': (c_i32, [c_vp, c_i32, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_i32, c_vp, c_sz, c_vp]),
    'mv_score_norm_f32': (c_i32, [c_vp, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp]),
    'mv_vad_energy_workspace_bytes': (c_sz, [ctypes.POINTER(MvVadCfg), c_i32, c_i64]),
    'mv_vad_energy_f32': (c_i32, [ctypes.POINTER(MvVadCfg), c_vp, c_i64, c_vp, c_i32, c_i64, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    'mv_vad_regions_workspace_bytes': (c_sz, [c_i32, c_i32]),
    'mv_vad_regions_i32': (c_i32, [ctypes.POINTER(MvVadSmoothCfg), c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_i64, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    'mv_wave_gather_workspace_bytes': (c_sz, [c_i32, c_i32]),
    'mv_wave_gather_f32': (c_i32, [c_vp, c_i64, c_vp, c_vp, c_vp, c_i32, c_i32, c_i64, c_vp, c_i64, c_i64, c_vp, c_vp, c_sz, c_vp]),
    'mv_margin_ce_workspace_bytes': (c_sz, [c_i64, c_i64, c_i32]),
    'mv_margin_ce_forward': (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    'mv_margin_ce_backward': (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp]),
    'mv_sphereface2_workspace_bytes': (c_sz, [c_i64, c_i64]),
    'mv_sphereface2_forward': (c_i32, [c_vp, c_vp, c_i32, c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    'mv_sphereface2_backward': (c_i32, [c_vp, c_vp, c_i32, c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp]),
    'mv_triplet_workspace_bytes': (c_sz, [c_i64, c_i64]),
    'mv_triplet_forward': (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    'mv_triplet_backward': (c_i32, [c_vp, c_vp, c_i32, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_sz, c_vp]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None


def bind(cdll):
    """Attach prototypes to a loaded library (also used by the test-suite for its emulator build)."""
    for name, (restype, argtypes) in _SIGNATURES.items():
        fn = getattr(cdll, name)
        fn.restype = restype
        fn.argtypes = argtypes
    return cdll


def bind_partial(cdll):
    """Prototypes for whatever subset of the ABI a (probe) library exports; tools only."""
    for name, (restype, argtypes) in _SIGNATURES.items():
        fn = getattr(cdll, name, None)
        if fn is not None:
            fn.restype = restype
            fn.argtypes = argtypes
    return cdll


def available():
    return os.path.exists(LIB_PATH)


def lib():
    """The bound library; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f'{LIB_PATH} is missing: the HIP library has not been built (run `python __graft_entry__.py` or '
                f'`python voiceprintrecognition-pytorch_amd/build_native.py`). There is no non-HIP device path.')
        cdll = bind(ctypes.CDLL(LIB_PATH))
        if cdll.mv_abi_version() != 5:
            raise RuntimeError('libmvector_hip.so ABI version mismatch')
        _lib = cdll
    return _lib


def check(rc, cdll=None):
    if rc != 0:
        cdll = cdll or lib()
        raise RuntimeError(f'libmvector_hip: {cdll.mv_last_error().decode(errors="replace")} (code {rc})')


def current_stream(tensor):
    if tensor.is_cuda:
        return torch.cuda.current_stream(tensor.device).cuda_stream
    return None


def _ptr(t):
    return None if t is None else t.data_ptr()


def conv1d_plan_info(desc, groups=1, cus=0, cdll=None):
    """What mv_conv1d_forward (groups = 1) / mv_conv1d_forward_grouped would launch for the MvConv1dDesc ``desc`` on a chip of ``cus`` compute
    units (0: the current device's), nothing launched (mv_conv1d_plan_info): {'kernel', 'in_stats_kernel', 'tail_kernel'} -- rows of csrc/conv1d.hip's
    kernel table by name, '' for no such launch -- and {'n_tiles', 'co_tiles', 'grid', 'tail_nv', 'tail_split'}.  A descriptor the forward refuses
    raises the forward's error."""
    cdll = cdll or lib()
    info = MvConv1dPlanInfo()
    check(cdll.mv_conv1d_plan_info(ctypes.byref(desc), groups, cus, ctypes.byref(info)), cdll)
    out = {name: getattr(info, name).decode() for name in ('kernel', 'in_stats_kernel', 'tail_kernel')}
    out.update((name, getattr(info, name)) for name in ('n_tiles', 'co_tiles', 'grid', 'tail_nv', 'tail_split'))
    return out


def conv2ds_plan_info(desc, cus=0, cdll=None):
    """What mv_conv2ds_forward would launch for the MvConv2dsDesc ``desc`` on a chip of ``cus`` compute units (0: the current device's), nothing
    launched (mv_conv2ds_plan_info): {'kernel'} -- the row of csrc/conv2ds.hip's kernel table by name -- and the launch shape, every integer field
    of MvConv2dsPlanInfo.  A descriptor the forward refuses raises the forward's error."""
    cdll = cdll or lib()
    info = MvConv2dsPlanInfo()
    check(cdll.mv_conv2ds_plan_info(ctypes.byref(desc), cus, ctypes.byref(info)), cdll)
    out = {'kernel': info.kernel.decode()}
    out.update((name, getattr(info, name)) for name, _ in MvConv2dsPlanInfo._fields_[1:])
    return out


# mv_melspec_info / mv_spectrogram_info / mv_mfcc_info: the kernel behind the STFT of a handle
_STFT_KERNELS = {0: 'stft_power_kernel (dense DFT)', 1: 'melspec_tile_kernel', 2: 'melspec_pow2_kernel'}


def _forward_inputs(wav, lens_ratio, num_samples, check_shape=True):
    """what every front-end forward does to its arguments first: ``wav`` [B, L] fp32 with unit stride along time; ``lens_ratio`` (fp32) or
    ``num_samples`` (int64 [B]) -- never both -- contiguous on wav's device"""
    if lens_ratio is not None and num_samples is not None:
        raise ValueError('lens_ratio and num_samples are mutually exclusive')
    assert wav.dim() == 2 and wav.dtype == torch.float32
    if wav.stride(1) != 1:
        wav = wav.contiguous()
    if num_samples is not None:
        num_samples = num_samples.to(device=wav.device, dtype=torch.int64).contiguous()
        if check_shape and num_samples.shape != (wav.shape[0],):
            raise ValueError(f'num_samples must have shape ({wav.shape[0]},), got {tuple(num_samples.shape)}')
    if lens_ratio is not None:
        lens_ratio = lens_ratio.to(device=wav.device, dtype=torch.float32).contiguous()
    return wav, lens_ratio, num_samples


class _FrontEnd:
    """what the front-end handles share: the native handle ``_h`` of the library ``_cdll`` behind the entry points ``_prefix`` + name, its frame
    count and its release; and the forward of the STFT handles (MelSpec / Spectrogram / Mfcc): [B, L] fp32 -> [B, T, dim]"""
    _prefix = None

    def _fn(self, name):
        return getattr(self._cdll, self._prefix + name)

    def num_frames(self, num_samples):
        t = c_i64()
        check(self._fn('num_frames')(self._h, num_samples, ctypes.byref(t)), self._cdll)
        return t.value

    def __call__(self, wav, lens_ratio=None, num_samples=None):
        """wav [B, L] fp32 -> [B, T(L), dim], on the caller's stream with a workspace per call.  ``lens_ratio``: the reference's batched
        semantics (mean over all T frames, then mask).  ``num_samples`` (int64 [B]): every row featurised on its own length, zero rows beyond
        it (mv_*_forward_varlen).  One native call either way."""
        wav, lens_ratio, num_samples = _forward_inputs(wav, lens_ratio, num_samples)
        B, L = wav.shape
        T = self.num_frames(L)
        out = torch.empty((B, T, self.dim), dtype=torch.float32, device=wav.device)
        if B == 0 or T == 0:
            return out
        nbytes = self._fn('workspace_bytes')(self._h, B, L)
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=wav.device)
        form, lens = ('forward', lens_ratio) if num_samples is None else ('forward_varlen', num_samples)
        check(self._fn(form)(self._h, wav.data_ptr(), B, L, wav.stride(0), _ptr(lens), out.data_ptr(), ws.data_ptr(), nbytes,
                             current_stream(wav)), self._cdll)
        return out

    def __del__(self):
        try:
            if getattr(self, '_h', None):
                self._fn('destroy')(self._h)
        except Exception:
            pass


class Fbank(_FrontEnd):
    """Handle of the fused Fbank + CMN + mask kernel (mv_fbank_*)."""
    _prefix = 'mv_fbank_'

    WINDOW_TYPES = {'povey': 0, 'hamming': 1, 'hanning': 2, 'rectangular': 3, 'blackman': 4}
    KERNELS = {'auto': 0, 'generic': 1, 'tile': 2}

    def __init__(self, method_args=None, subtract_time_mean=True, cdll=None, kernel='auto'):
        """``method_args``: the keyword arguments of torchaudio.compliance.kaldi.fbank (featurizer.py:128 forwards them).  ``kernel``:
        'auto' | 'generic' (fbank_kernel) | 'tile' (fbank_tile_kernel; refused when the geometry has no instantiation) -- tests / tools."""
        self._cdll = cdll or lib()
        cfg = MvFbankCfg()
        self._cdll.mv_fbank_default_cfg(ctypes.byref(cfg))
        args = dict(method_args or {})
        mapping = {'sample_frequency': 'sample_frequency', 'frame_length': 'frame_length_ms',
                   'frame_shift': 'frame_shift_ms', 'num_mel_bins': 'num_mel_bins', 'low_freq': 'low_freq',
                   'high_freq': 'high_freq', 'preemphasis_coefficient': 'preemphasis_coefficient',
                   'remove_dc_offset': 'remove_dc_offset', 'use_power': 'use_power', 'use_log_fbank': 'use_log_fbank',
                   'blackman_coeff': 'blackman_coeff', 'snip_edges': 'snip_edges', 'subtract_mean': 'subtract_mean',
                   'min_duration': 'min_duration', 'vtln_warp': 'vtln_warp', 'vtln_low': 'vtln_low', 'vtln_high': 'vtln_high',
                   'use_energy': 'use_energy', 'raw_energy': 'raw_energy', 'energy_floor': 'energy_floor', 'htk_compat': 'htk_compat'}
        # arguments whose other values are not implemented (dither draws random numbers; non-power-of-two FFT sizes).  use_energy (since round 6) adds
        # the log-energy column: the output has num_mel_bins + 1 columns, which AudioFeaturizer.feature_dim -- like the reference's,
        # featurizer.py:110-111 -- does not count
        fixed = {'dither': 0.0, 'round_to_power_of_two': True, 'channel': (-1, 0)}
        ignored = ()
        for k, v in args.items():
            if k in mapping:
                field = mapping[k]
                typ = dict(MvFbankCfg._fields_)[field]
                setattr(cfg, field, int(v) if typ is c_i32 else float(v))
            elif k == 'window_type':
                if v not in self.WINDOW_TYPES:
                    raise Exception('Invalid window type ' + str(v))   # torchaudio's own message
                cfg.window_type = self.WINDOW_TYPES[v]
            elif k in fixed:
                allowed = fixed[k] if isinstance(fixed[k], tuple) else (fixed[k],)
                if v not in allowed:
                    raise NotImplementedError(f'Fbank argument {k}={v!r} is not implemented by the HIP kernel')
            elif k not in ignored:
                raise TypeError(f"fbank() got an unexpected keyword argument '{k}'")
        # torchaudio compares `len(waveform) < min_duration * sample_frequency` in double: the sample threshold goes down as an integer (the struct's
        # float32 min_duration rounds 0.1 s to 1601 samples at 16 kHz)
        import math
        cfg.min_samples = int(math.ceil(float(args.get('min_duration', 0.0)) * float(args.get('sample_frequency', cfg.sample_frequency))))
        cfg.subtract_time_mean = 1 if subtract_time_mean else 0
        cfg.kernel = self.KERNELS[kernel]
        self.num_mel_bins = cfg.num_mel_bins
        self.num_columns = cfg.num_mel_bins + (1 if cfg.use_energy else 0)
        self._needs_ws = (not cfg.snip_edges) or bool(cfg.use_energy)   # forms that cannot run without the caller workspace
        self._h = c_vp()
        check(self._cdll.mv_fbank_create(ctypes.byref(cfg), ctypes.byref(self._h)), self._cdll)

    def info(self):
        """{'tile_kernel': bool, 'pass_steps': (s0, s1)} -- which kernel the handle launches (mv_fbank_info)"""
        tk, steps = c_i32(), (c_i32 * 2)()
        check(self._cdll.mv_fbank_info(self._h, ctypes.byref(tk), steps), self._cdll)
        return {'tile_kernel': bool(tk.value), 'pass_steps': (steps[0], steps[1])}

    def __call__(self, wav, lens_ratio=None, num_samples=None, workspace=True):
        """wav [B, L] fp32 -> [B, T(L), F].  ``lens_ratio``: the reference's batched semantics (mean over all T frames,
        then mask).  ``num_samples`` (int64 [B]): every row featurised on its own length, zero rows beyond it.
        ``workspace=False`` keeps one workgroup per utterance (mv_fbank_forward without scratch; same bits, see the header)."""
        assert lens_ratio is None or num_samples is None
        wav, lens_ratio, num_samples = _forward_inputs(wav, lens_ratio, num_samples, check_shape=False)
        B, L = wav.shape
        T = self.num_frames(L)
        out = torch.empty((B, T, self.num_columns), dtype=torch.float32, device=wav.device)
        if B == 0 or T == 0:
            return out
        # per-call scratch (the several-workgroups-per-utterance form of long utterances / batches smaller than the chip; the mirrored signal
        # of snip_edges=False): from torch's stream-aware caching allocator, so concurrent forwards on other streams never share it (the handle
        # owns no mutable state)
        need = ctypes.c_size_t()
        check(self._cdll.mv_fbank_workspace_bytes(self._h, B, L, ctypes.byref(need)), self._cdll)
        ws = torch.empty(need.value, dtype=torch.uint8, device=wav.device) if need.value and (workspace or self._needs_ws) else None
        # the _ws entry points with a null workspace are the plain ones
        form, lens = ('forward_ws', lens_ratio) if num_samples is None else ('forward_varlen_ws', num_samples)
        check(self._fn(form)(self._h, wav.data_ptr(), B, L, wav.stride(0), _ptr(lens), out.data_ptr(), _ptr(ws),
                             need.value if ws is not None else 0, current_stream(wav)), self._cdll)
        return out


_PAD_MODES = {'reflect': 0, 'constant': 1, 'replicate': 2, 'circular': 3}
_MEL_KEYS = ('sample_rate', 'n_fft', 'win_length', 'hop_length', 'f_min', 'f_max', 'pad', 'n_mels', 'power', 'normalized', 'center', 'pad_mode',
             'onesided', 'norm', 'mel_scale', 'window_fn', 'wkwargs')
_SPEC_KEYS = ('n_fft', 'win_length', 'hop_length', 'pad', 'window_fn', 'power', 'normalized', 'wkwargs', 'center', 'pad_mode', 'onesided',
              'return_complex')
_MFCC_KEYS = ('sample_rate', 'n_mfcc', 'dct_type', 'norm', 'log_mels', 'melkwargs')


def _stft_unsupported(a, what):
    """the STFT options the kernels do not implement: two-sided spectra (torchaudio's own MelScale refuses their bin count), power=None (the
    complex spectrogram) and padding modes torch.nn.functional.pad does not know (its own error class)"""
    if a.get('onesided') not in (None, True) or ('power' in a and a['power'] is None):
        raise NotImplementedError(f'{what} option not implemented by the HIP kernel')
    if a.get('pad_mode', 'reflect') not in _PAD_MODES:
        raise NotImplementedError(f"Unrecognised padding mode {a.get('pad_mode')}")


def _stft_fields(cfg, a, what):
    """the STFT keyword arguments torchaudio's Spectrogram / MelSpectrogram share, checked as torchaudio checks them, into `cfg`
    (an MvSpectrogramCfg or an MvMelSpecCfg); returns the host window tensor that cfg.window points to (None for the default), which the
    caller keeps alive until create has copied it"""
    _stft_unsupported(a, what)
    if a.get('normalized', False) not in (False, True, 'window', 'frame_length'):
        raise ValueError(f"Invalid normalized parameter: {a.get('normalized')}")
    cfg.n_fft = int(a.get('n_fft', 400))
    win = a.get('win_length')
    cfg.win_length = int(win if win is not None else cfg.n_fft)
    hop = a.get('hop_length')
    cfg.hop_length = int(hop if hop is not None else cfg.win_length // 2)
    cfg.power = float(a.get('power', 2.0))
    cfg.center = 1 if a.get('center', True) else 0
    cfg.normalized = {False: 0, True: 1, 'window': 1, 'frame_length': 2}[a.get('normalized', False)]
    cfg.pad = int(a.get('pad', 0))
    cfg.pad_mode = _PAD_MODES[a.get('pad_mode', 'reflect')]
    win_host = None
    if a.get('window_fn') is not None:   # torchaudio evaluates window_fn(win_length, **wkwargs) once, at construction: so does this
        win_host = a['window_fn'](cfg.win_length, **(a.get('wkwargs') or {})).detach().to(device='cpu', dtype=torch.float32).contiguous()
        if win_host.shape != (cfg.win_length,):
            raise ValueError(f'window_fn returned {tuple(win_host.shape)}, expected ({cfg.win_length},)')
        cfg.window = win_host.data_ptr()
    return win_host


class MelSpec(_FrontEnd):
    """Handle of the MelSpectrogram + CMN + mask path (mv_melspec_*).  Output [B, T, n_mels]."""
    _prefix = 'mv_melspec_'
    PAD_MODES = _PAD_MODES

    def __init__(self, method_args=None, subtract_time_mean=True, cdll=None):
        self._cdll = cdll or lib()
        cfg = MvMelSpecCfg()
        self._cdll.mv_melspec_default_cfg(ctypes.byref(cfg))
        win_host = self.fill_cfg(cfg, method_args, subtract_time_mean)  # noqa: F841  (alive until create has copied it)
        self.n_mels = self.dim = cfg.n_mels
        self._h = c_vp()
        check(self._cdll.mv_melspec_create(ctypes.byref(cfg), ctypes.byref(self._h)), self._cdll)

    @classmethod
    def fill_cfg(cls, cfg, method_args, subtract_time_mean=True):
        """MelSpectrogram(**method_args) checked as torchaudio checks it, into an MvMelSpecCfg (also the mel stage of Mfcc); returns the
        host window tensor that cfg.window points to (None for the default), which must stay alive until create"""
        a = dict(method_args or {})
        for k in a:
            if k not in _MEL_KEYS:
                raise TypeError(f"MelSpectrogram got an unexpected keyword argument '{k}'")
        _stft_unsupported(a, 'MelSpectrogram')   # (in front of MelScale's checks, which torchaudio makes at construction; `normalized` is read later)
        if a.get('norm') not in (None, 'slaney'):
            raise ValueError('norm must be one of None or "slaney"')          # torchaudio.functional.melscale_fbanks' own messages
        if a.get('mel_scale', 'htk') not in ('htk', 'slaney'):
            raise ValueError('mel_scale should be one of "htk" or "slaney".')
        win_host = _stft_fields(cfg, a, 'MelSpectrogram')
        cfg.sample_rate = int(a.get('sample_rate', 16000))
        cfg.f_min = float(a.get('f_min', 0.0))
        f_max = a.get('f_max')
        cfg.f_max = float(f_max if f_max is not None else cfg.sample_rate // 2)
        cfg.n_mels = int(a.get('n_mels', 128))
        cfg.subtract_time_mean = 1 if subtract_time_mean else 0
        cfg.mel_scale = 1 if a.get('mel_scale', 'htk') == 'slaney' else 0
        cfg.norm = 1 if a.get('norm') == 'slaney' else 0
        return win_host

    def info(self):
        """{'tile_kernel': bool, 'kernel': name}: True when an FFT kernel runs -- melspec_tile_kernel (n_fft = 400) or melspec_pow2_kernel
        (n_fft 128 ... 1024, power of two) --, False for the dense-DFT kernels"""
        tk = c_i32()
        check(self._cdll.mv_melspec_info(self._h, ctypes.byref(tk)), self._cdll)
        return {'tile_kernel': bool(tk.value), 'kernel': _STFT_KERNELS[tk.value]}


class Spectrogram(_FrontEnd):
    """Handle of the Spectrogram + CMN + mask path (mv_spectrogram_*): torchaudio.transforms.Spectrogram(**method_args), then
    AudioFeaturizer's time mean and mask.  Output [B, T, n_fft // 2 + 1]."""
    _prefix = 'mv_spectrogram_'

    def __init__(self, method_args=None, subtract_time_mean=True, cdll=None):
        self._cdll = cdll or lib()
        a = dict(method_args or {})
        for k in a:
            if k not in _SPEC_KEYS:
                raise TypeError(f"Spectrogram got an unexpected keyword argument '{k}'")
        cfg = MvSpectrogramCfg()
        self._cdll.mv_spectrogram_default_cfg(ctypes.byref(cfg))
        win_host = _stft_fields(cfg, a, 'Spectrogram')  # noqa: F841  (alive until create has copied it)
        cfg.subtract_time_mean = 1 if subtract_time_mean else 0
        self.dim = cfg.n_fft // 2 + 1
        self._h = c_vp()
        check(self._cdll.mv_spectrogram_create(ctypes.byref(cfg), ctypes.byref(self._h)), self._cdll)

    def info(self):
        """{'kernel': name}: the fused n_fft = 400 launch or the dense DFT"""
        k = c_i32()
        check(self._cdll.mv_spectrogram_info(self._h, ctypes.byref(k)), self._cdll)
        return {'kernel': _STFT_KERNELS[k.value] + (' (spectrogram)' if k.value == 1 else '')}


class Mfcc(_FrontEnd):
    """Handle of the MFCC + CMN + mask path (mv_mfcc_*): torchaudio.transforms.MFCC(**method_args), then AudioFeaturizer's time mean
    and mask.  Output [B, T, n_mfcc].  With log_mels=False the top_db floor is taken over the whole batch of the call, as torchaudio does."""
    _prefix = 'mv_mfcc_'

    def __init__(self, method_args=None, subtract_time_mean=True, cdll=None):
        self._cdll = cdll or lib()
        a = dict(method_args or {})
        for k in a:
            if k not in _MFCC_KEYS:
                raise TypeError(f"MFCC got an unexpected keyword argument '{k}'")
        # torchaudio.transforms.MFCC.__init__: the DCT type, then the mel stage, then the coefficient count, then create_dct's norm
        if a.get('dct_type', 2) != 2:
            raise ValueError(f"DCT type not supported: {a.get('dct_type')}")
        melkwargs = dict(a.get('melkwargs') or {})
        if 'sample_rate' in melkwargs:
            raise TypeError("MelSpectrogram got multiple values for keyword argument 'sample_rate'")
        melkwargs['sample_rate'] = a.get('sample_rate', 16000)
        cfg = MvMfccCfg()
        self._cdll.mv_mfcc_default_cfg(ctypes.byref(cfg))
        self._mel_window = MelSpec.fill_cfg(cfg.mel, melkwargs, subtract_time_mean=False)
        n_mfcc = int(a.get('n_mfcc', 40))
        if n_mfcc > cfg.mel.n_mels:
            raise ValueError('Cannot select more MFCC coefficients than # mel bins')
        if a.get('norm', 'ortho') not in (None, 'ortho'):
            raise AssertionError(f"norm must be None or 'ortho', got {a.get('norm')!r}")   # (create_dct asserts)
        cfg.n_mfcc = n_mfcc
        cfg.dct_norm = 1 if a.get('norm', 'ortho') == 'ortho' else 0
        cfg.log_mels = 1 if a.get('log_mels', False) else 0
        cfg.top_db = 80.0
        cfg.subtract_time_mean = 1 if subtract_time_mean else 0
        self.dim = n_mfcc
        self._h = c_vp()
        check(self._cdll.mv_mfcc_create(ctypes.byref(cfg), ctypes.byref(self._h)), self._cdll)
        self._mel_window = None

    def info(self):
        """{'mel_kernel': name of the mel stage's kernel, 'dct_lds': bool}"""
        k, d = c_i32(), c_i32()
        check(self._cdll.mv_mfcc_info(self._h, ctypes.byref(k), ctypes.byref(d)), self._cdll)
        return {'mel_kernel': _STFT_KERNELS[k.value], 'dct_lds': bool(d.value)}


def _tensor_refs(state_dict, device=None):
    """(MvTensorRef array, the fp32 tensors it points to -- to be kept alive until create has read them) of a state_dict's floating-point entries"""
    names, tensors = [], []
    for k, v in state_dict.items():
        if not torch.is_floating_point(v):
            continue
        t = v.detach().to(device=device if device is not None else v.device, dtype=torch.float32).contiguous()
        names.append(k.encode())
        tensors.append(t)
    refs = (MvTensorRef * max(len(tensors), 1))()
    for i, (n, t) in enumerate(zip(names, tensors)):
        refs[i].name = n
        refs[i].data = t.data_ptr()
        refs[i].numel = t.numel()
    return refs, tensors, names


class HfEncoder(_FrontEnd):
    """Handle of the HuggingFace (Wav2Vec2 / WavLM) front-end (mv_hfenc_*): the processor's z-score, the convolutional feature encoder and
    feature_projection.layer_norm -- `extract_features` --, then AudioFeaturizer's time mean and mask.  Output [B, T', conv_dim[-1]].

    ``cfg``: the model's config as a dict (``model.config.to_dict()``; read are conv_dim, conv_kernel, conv_stride, feat_extract_norm,
    feat_extract_activation, conv_bias, layer_norm_eps) plus ``do_normalize`` (the processor's); ``state_dict``: the Wav2Vec2Model / WavLMModel's,
    under its own key names, on the device the handle is to run on.  Needs no `transformers`."""

    _prefix = 'mv_hfenc_'
    NORMS = {'group': MV_HF_NORM_GROUP, 'layer': MV_HF_NORM_LAYER}

    def __init__(self, cfg, state_dict, subtract_time_mean=True, cdll=None, device=None):
        self._cdll = cdll or lib()
        c = MvHfEncoderCfg()
        dims, kernels, strides = list(cfg['conv_dim']), list(cfg['conv_kernel']), list(cfg['conv_stride'])
        if not (len(dims) == len(kernels) == len(strides)):
            raise ValueError('conv_dim, conv_kernel and conv_stride must have one entry per layer')
        if not 1 <= len(dims) <= MV_HFENC_MAX_LAYERS:
            raise NotImplementedError(f'a feature encoder of {len(dims)} layers is not implemented by the HIP kernels (1 .. {MV_HFENC_MAX_LAYERS})')
        act = cfg.get('feat_extract_activation', 'gelu')
        if act != 'gelu':
            raise NotImplementedError(f"feat_extract_activation {act!r} is not implemented by the HIP kernels (only 'gelu')")
        norm = cfg.get('feat_extract_norm', 'group')
        if norm not in self.NORMS:
            raise ValueError(f"feat_extract_norm {norm!r} is not one of ['group', 'layer']")   # (the HF config's own check)
        c.num_layers = len(dims)
        for i, (d, k, s) in enumerate(zip(dims, kernels, strides)):
            c.conv_dim[i], c.conv_kernel[i], c.conv_stride[i] = int(d), int(k), int(s)
        c.feat_extract_norm = self.NORMS[norm]
        c.conv_bias = 1 if cfg.get('conv_bias', False) else 0
        c.do_normalize = 1 if cfg.get('do_normalize', True) else 0
        c.activation = MV_ACT_GELU
        c.layer_norm_eps = float(cfg.get('layer_norm_eps', 1e-5))
        c.subtract_time_mean = 1 if subtract_time_mean else 0
        self.dim = int(dims[-1])
        self.num_layers = len(dims)
        refs, tensors, _ = _tensor_refs(state_dict, device)
        if tensors and tensors[0].is_cuda:
            torch.cuda.current_stream(tensors[0].device).synchronize()
        self._h = c_vp()
        check(self._cdll.mv_hfenc_create(ctypes.byref(c), refs, len(tensors), ctypes.byref(self._h)), self._cdll)

    def __call__(self, wav, lens_ratio=None, num_samples=None, stage_ms=None):
        """wav [B, L] fp32 -> [B, T', dim] fp32 on the same device, the caller's stream, a workspace per call.  ``lens_ratio``: the reference's
        batched semantics (mean over all T' frames, then mask).  ``num_samples`` (int64 [B]): every row featurised on its own length, zero
        frames beyond it (mv_hfenc_forward_varlen; the lengths go to the device and are never read back).  ``stage_ms``: a list that receives
        the milliseconds of every layer and of the tail (mv_hfenc_forward_timed: waits for the forward; tools only; not with ``num_samples``)"""
        wav, lens_ratio, num_samples = _forward_inputs(wav, lens_ratio, None if num_samples is None else torch.as_tensor(num_samples))
        if num_samples is not None and stage_ms is not None:
            raise ValueError('stage_ms times the fixed-length forward: it cannot be combined with num_samples')
        B, L = wav.shape
        T = self.num_frames(L)
        if B == 0:
            return torch.empty((0, max(T, 0), self.dim), dtype=torch.float32, device=wav.device)
        need = c_sz()
        check(self._cdll.mv_hfenc_workspace_bytes(self._h, B, L, ctypes.byref(need)), self._cdll)
        ws = torch.empty(max(need.value, 16), dtype=torch.uint8, device=wav.device)
        out = torch.empty((B, max(T, 1), self.dim), dtype=torch.float32, device=wav.device)   # (T <= 0: the forward refuses, with its message)
        if num_samples is not None:
            check(self._cdll.mv_hfenc_forward_varlen(self._h, wav.data_ptr(), B, L, wav.stride(0), num_samples.data_ptr(), out.data_ptr(),
                                                     ws.data_ptr(), need.value, current_stream(wav)), self._cdll)
            return out
        if stage_ms is not None:
            ms = (c_f32 * (self.num_layers + 1))()
            check(self._cdll.mv_hfenc_forward_timed(self._h, wav.data_ptr(), B, L, wav.stride(0), _ptr(lens_ratio), out.data_ptr(), ws.data_ptr(),
                                                    need.value, current_stream(wav), ms, self.num_layers + 1), self._cdll)
            stage_ms[:] = list(ms)
            return out
        check(self._cdll.mv_hfenc_forward(self._h, wav.data_ptr(), B, L, wav.stride(0), _ptr(lens_ratio), out.data_ptr(), ws.data_ptr(), need.value,
                                          current_stream(wav)), self._cdll)
        return out


def _w2vbert_row_args(x, num_samples, L):
    """what the kernel-level entry points of the Wav2Vec2-BERT front-end share: fp32 contiguous rows, the optional int64 lengths on their device"""
    assert x.dtype == torch.float32 and x.is_contiguous()
    if num_samples is not None:
        num_samples = torch.as_tensor(num_samples).to(device=x.device, dtype=torch.int64).contiguous()
    return num_samples, int(L if L is not None else 0)


def w2vbert_binstats(x, num_samples=None, L=None, cdll=None):
    """mv_w2vbert_binstats_f32: x [B, T, 80] fp32 -> (mean, var) [B, 80]: per bin over the row's frames, unbiased variance, fp64 sums rounded once.
    ``num_samples`` (int64 [B]) with the padded length ``L``: the row's own frame count (0 below 560 samples)."""
    cdll = cdll or lib()
    num_samples, L = _w2vbert_row_args(x, num_samples, L)
    B, T, _ = x.shape
    mean, var = torch.empty((B, 80), dtype=torch.float32, device=x.device), torch.empty((B, 80), dtype=torch.float32, device=x.device)
    check(cdll.mv_w2vbert_binstats_f32(x.data_ptr(), B, T, _ptr(num_samples), L, mean.data_ptr(), var.data_ptr(), current_stream(x)), cdll)
    return mean, var


def w2vbert_rows(x, mean, var, ln_weight, ln_bias, eps, num_samples=None, L=None, out=None, cdll=None):
    """mv_w2vbert_rows_f32: normalise x [B, T, 80] with (mean, var) [B, 80], stack pairs of frames (a frame behind the row's count is zeros),
    LayerNorm over the 160 columns -> [B, ceil(T / 2), 160].  ``out``: a buffer to write into (tests prefill it)."""
    cdll = cdll or lib()
    num_samples, L = _w2vbert_row_args(x, num_samples, L)
    B, T, _ = x.shape
    if out is None:
        out = torch.empty((B, (T + 1) // 2, 160), dtype=torch.float32, device=x.device)
    check(cdll.mv_w2vbert_rows_f32(x.data_ptr(), mean.data_ptr(), var.data_ptr(), ln_weight.data_ptr(), ln_bias.data_ptr(), eps, B, T,
                                   _ptr(num_samples), L, out.data_ptr(), current_stream(x)), cdll)
    return out


def w2vbert_cmn_mask(out, lens_ratio=None, num_samples=None, L=None, cmn=True, cdll=None):
    """mv_w2vbert_cmn_mask_f32, in place on out [B, T2, 160]: minus the time mean over the row's stacked frames, zeros behind the mask length"""
    cdll = cdll or lib()
    num_samples, L = _w2vbert_row_args(out, num_samples, L)
    if lens_ratio is not None:
        lens_ratio = lens_ratio.to(device=out.device, dtype=torch.float32).contiguous()
    B, T2, _ = out.shape
    check(cdll.mv_w2vbert_cmn_mask_f32(out.data_ptr(), B, T2, _ptr(lens_ratio), _ptr(num_samples), L, 1 if cmn else 0, current_stream(out)), cdll)
    return out


class W2vBert(_FrontEnd):
    """Handle of the HuggingFace Wav2Vec2-BERT (w2v-bert-2.0) front-end (mv_w2vbert_*): the SeamlessM4TFeatureExtractor's input_features (waveform *
    2^15, 80-bin Kaldi log-mel, per-bin normalisation over time, pairs of frames stacked) and feature_projection.layer_norm -- `extract_features`
    --, then AudioFeaturizer's time mean and mask.  Output [B, T2, stride * num_mel_bins].

    ``cfg``: a dict with the processor's ``num_mel_bins``, ``stride``, ``sampling_rate`` and the model config's ``layer_norm_eps``;
    ``state_dict``: holds ``feature_projection.layer_norm.weight`` / ``.bias``.  ``device``: where the handle is to run (None: the current
    device; the emulator build ignores it).  Needs no `transformers`."""

    _prefix = 'mv_w2vbert_'

    def __init__(self, cfg, state_dict, device=None, subtract_time_mean=True, cdll=None):
        self._cdll = cdll or lib()
        c = MvW2vBertCfg()
        c.num_mel_bins = int(cfg.get('num_mel_bins', 80))
        c.stride = int(cfg.get('stride', 2))
        c.sampling_rate = int(cfg.get('sampling_rate', 16000))
        c.layer_norm_eps = float(cfg.get('layer_norm_eps', 1e-5))
        c.subtract_time_mean = 1 if subtract_time_mean else 0
        self.dim = c.num_mel_bins * c.stride
        ln = []
        for k in ('feature_projection.layer_norm.weight', 'feature_projection.layer_norm.bias'):
            if k not in state_dict:
                raise KeyError(f'W2vBert: the state_dict has no {k!r}')
            t = state_dict[k].detach().to(device='cpu', dtype=torch.float32).contiguous()
            if t.numel() != self.dim:
                raise ValueError(f'W2vBert: {k!r} has {t.numel()} elements, expected stride * num_mel_bins = {self.dim}')
            ln.append(t)
        self._h = c_vp()
        if device is not None and torch.device(device).type == 'cuda':
            with torch.cuda.device(device):
                check(self._cdll.mv_w2vbert_create(ctypes.byref(c), ln[0].data_ptr(), ln[1].data_ptr(), ctypes.byref(self._h)), self._cdll)
        else:
            check(self._cdll.mv_w2vbert_create(ctypes.byref(c), ln[0].data_ptr(), ln[1].data_ptr(), ctypes.byref(self._h)), self._cdll)

    def __call__(self, wav, lens_ratio=None, num_samples=None):
        """wav [B, L] fp32 -> [B, T2, dim] fp32 on the same device, the caller's stream, a workspace per call: one native call.  ``lens_ratio``:
        the reference's batched semantics (every row normalised over all frames of the padded length, then the mask).  ``num_samples`` (int64
        [B]): every row featurised on its own length, zero frames beyond it (mv_w2vbert_forward_varlen; the lengths are never read back)."""
        wav, lens_ratio, num_samples = _forward_inputs(wav, lens_ratio, None if num_samples is None else torch.as_tensor(num_samples))
        B, L = wav.shape
        T2 = self.num_frames(L)
        out = torch.empty((B, T2, self.dim), dtype=torch.float32, device=wav.device)
        if B == 0:
            return out
        need = c_sz()
        check(self._cdll.mv_w2vbert_workspace_bytes(self._h, B, L, ctypes.byref(need)), self._cdll)
        ws = torch.empty(max(need.value, 16), dtype=torch.uint8, device=wav.device)
        form, lens = ('forward', lens_ratio) if num_samples is None else ('forward_varlen', num_samples)
        check(self._fn(form)(self._h, wav.data_ptr(), B, L, wav.stride(0), _ptr(lens), out.data_ptr(), ws.data_ptr(), need.value,
                             current_stream(wav)), self._cdll)
        return out

    def binstats(self, x, num_samples=None, L=None):
        return w2vbert_binstats(x, num_samples, L, cdll=self._cdll)

    def rows(self, x, mean, var, ln_weight, ln_bias, eps, num_samples=None, L=None, out=None):
        return w2vbert_rows(x, mean, var, ln_weight, ln_bias, eps, num_samples, L, out, cdll=self._cdll)


class Model:
    """Handle of a native backbone (mv_*_create / mv_model_forward) built from a reference-layout state_dict.

    ``pooling_type`` ('ASP' | 'SAP' | 'TAP' | 'TSP', or an MV_POOL_* code): the head of an 'ecapa' or 'tdnn' backbone
    (mv_*_create_pooled); other kinds have one head and take 'ASP' only, which stands for "the model's own" ('resnet_se', 'res2net': the
    head their config's pooling_type names)."""

    def __init__(self, kind, cfg, state_dict, cdll=None, pooling_type='ASP'):
        self._cdll = cdll or lib()
        if isinstance(pooling_type, str):
            if pooling_type not in POOLING_TYPES:
                raise ValueError(f'pooling_type {pooling_type!r} is not one of {sorted(POOLING_TYPES)}')
            pool = POOLING_TYPES[pooling_type]
        else:
            pool = int(pooling_type)   # (a code the library does not know is refused by the create call, with its message)
        if pool != MV_POOL_ASP and kind not in ('ecapa', 'tdnn'):
            raise ValueError(f'pooling_type {pooling_type!r}: only the ecapa and tdnn handles take a pooling head')
        refs, tensors, _ = _tensor_refs(state_dict)   # (floating-point entries only: no num_batches_tracked)
        self._h = c_vp()
        if isinstance(cfg, MvEcapaCfgEx):   # EcapaTdnn with other block counts / grouped convolutions: one create call for every head
            if kind != 'ecapa':
                raise ValueError(f'an MvEcapaCfgEx config belongs to the ecapa handle, not {kind!r}')
            create = lambda c, r, n, out: self._cdll.mv_ecapa_create_ex(c, pool, r, n, out)   # noqa: E731
        elif pool == MV_POOL_ASP:   # (the plain create calls: the handles every ASP model has always built)
            create = {'ecapa': self._cdll.mv_ecapa_create, 'campp': self._cdll.mv_campp_create,
                      'tdnn': self._cdll.mv_tdnn_create, 'eres2net': self._cdll.mv_eres2net_create,
                      'resnet_se': self._cdll.mv_resnetse_create, 'res2net': self._cdll.mv_res2net_create}[kind]
        else:
            pooled = {'ecapa': self._cdll.mv_ecapa_create_pooled, 'tdnn': self._cdll.mv_tdnn_create_pooled}[kind]
            create = lambda c, r, n, out: pooled(c, pool, r, n, out)   # noqa: E731
        if tensors and tensors[0].is_cuda:
            torch.cuda.current_stream(tensors[0].device).synchronize()  # weights fully written before create() reads them
        check(create(ctypes.byref(cfg), refs, len(tensors), ctypes.byref(self._h)), self._cdll)
        e = c_i32()
        check(self._cdll.mv_model_embd_dim(self._h, ctypes.byref(e)), self._cdll)
        self.embd_dim = e.value
        self._ws = {}   # one workspace per (device, stream): forwards of ONE handle on different streams run concurrently (the C ABI's contract)

    def workspace_bytes(self, B, T):
        n = c_sz()
        check(self._cdll.mv_model_workspace_bytes(self._h, B, T, ctypes.byref(n)), self._cdll)
        return n.value

    def info(self, key):
        """mv_model_info: 1 = CAM++ head on fp32 maps (1.0 / 0.0), 2 = its creation-time calibration 1 - cos, 3 + p = probe p's figure;
        EcapaTdnn: MV_INFO_ECAPA_* (20 grouped layers on the grouped GEMM, 21 expanded, 22 expanded 1x1 ones, 23 SE-Res2Net blocks);
        ResNetSE, Res2Net: MV_INFO_S16_* (30 largest map value since create, 31 saturated; both wait for the device)"""
        v = c_f32()
        check(self._cdll.mv_model_info(self._h, key, ctypes.byref(v)), self._cdll)
        return v.value

    def s16_range(self):
        """ResNetSE and Res2Net handles: {'peak': largest |map value| a launch wanted to store since create, 'saturated': it exceeded the S16 range
        1023.5 (the embeddings of that call are not to be trusted)}.  WAITS FOR THE DEVICE, like campp_head(range=True): a diagnostic, never on a
        hot path."""
        return {'peak': self.info(MV_INFO_S16_PEAK), 'saturated': self.info(MV_INFO_S16_SATURATED) == 1.0}

    resnet_se_range = s16_range   # (the name it was introduced under)

    XVEC_WARN = 2.5e-5   # MV_CAMPP_XVEC_WARN (include/mvector_hip.h)

    def campp_head(self, range=False):
        """CAM++ handles: {'head': 'f16' | 'f32', 'calibration': largest probe figure (-1 when pinned), 'probes': the three figures} -- the
        FCM head the handle chose at create (include/mvector_hip.h, MvCamppCfg.head_precision).  Host-side getters only: no device call, usable
        anywhere (also under stream capture).  range=True adds the exact head's peak / saturation on the caller's inputs since create, which WAITS
        FOR THE DEVICE (hipDeviceSynchronize + a blocking copy, csrc/campplus.hip): a diagnostic, never on a hot path."""
        d = {'head': 'f32' if self.info(1) == 1.0 else 'f16', 'calibration': self.info(2), 'probes': tuple(self.info(3 + p) for p in [0, 1, 2])}
        # what the head probes cannot see (since ABI 5): 1 - cos between the shipped (fp16-operand) and an exact-fp32 evaluation of the x-vector part
        # on the three probes; -1 = not measured.  Above XVEC_WARN the 1e-4 contract is at risk on this checkpoint whatever head runs.
        d.update(xvector_sensitivity=self.info(10), xvector_probes=tuple(self.info(11 + p) for p in [0, 1, 2]))
        d['xvector_warning'] = d['xvector_sensitivity'] > self.XVEC_WARN
        if d['head'] == 'f32':   # the exact head's range (include/mvector_hip.h, MV_INFO_CAMPP_HEAD_*): gain 2^k and the probes' peak, fixed at create
            d.update(gain_log2=int(self.info(6)), probe_peak=self.info(7))
            if range:
                d.update(peak=self.info(8), saturated=self.info(9) == 1.0)
        return d

    def forward(self, feats):
        assert feats.dim() == 3 and feats.dtype == torch.float32
        feats = feats.contiguous()
        B, T, _ = feats.shape
        emb = torch.empty((B, self.embd_dim), dtype=torch.float32, device=feats.device)
        if B == 0:
            return emb
        nbytes = self.workspace_bytes(B, T)
        stream = current_stream(feats)
        key = (str(feats.device), stream)
        ws = self._ws.get(key)
        if ws is None or ws.numel() < nbytes:
            self._ws.pop(key, None)   # (drop the smaller buffer before the larger one is allocated)
            ws = None
            if len(self._ws) >= 4:    # a caller that creates streams by the dozen must not pin a workspace for each
                self._ws.clear()
            ws = self._ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=feats.device)
        check(self._cdll.mv_model_forward(self._h, feats.data_ptr(), B, T, emb.data_ptr(), ws.data_ptr(), ws.numel(), stream), self._cdll)
        return emb

    def __del__(self):
        try:
            if getattr(self, '_h', None):
                self._cdll.mv_model_destroy(self._h)
        except Exception:
            pass


def wave_prepare(pcm, num_samples=None, target_db=None, max_gain_db=300.0, cdll=None):
    """int16 [B, L] on the device -> (float32 [B, L], too_quiet int32 [B]); ``target_db`` None = no dB normalisation."""
    cdll = cdll or lib()
    assert pcm.dim() == 2 and pcm.dtype == torch.int16
    if pcm.stride(1) != 1:
        pcm = pcm.contiguous()
    B, L = pcm.shape
    wav = torch.empty((B, L), dtype=torch.float32, device=pcm.device)
    flags = torch.zeros((B,), dtype=torch.int32, device=pcm.device)
    if num_samples is not None:
        num_samples = num_samples.to(device=pcm.device, dtype=torch.int64).contiguous()
    check(cdll.mv_wave_prepare_i16(pcm.data_ptr(), pcm.stride(0) if B else L, _ptr(num_samples), B, L, 0 if target_db is None else 1,
                                   float(target_db or 0.0), float(max_gain_db), wav.data_ptr(), L, flags.data_ptr(), current_stream(pcm)),
          cdll)
    return wav, flags


class Resampler:
    """Handle of the down-mix + polyphase resampler (mv_resampler_*): interleaved int16 PCM at ``src_rate`` -> mono fp32 at ``dst_rate`` with the
    filter of scipy.signal.resample_poly(x, up, down).  Refused (RuntimeError naming the limit): a rate <= 0, max(up, down) > 1024."""

    def __init__(self, src_rate, dst_rate, cdll=None):
        self._cdll = cdll or lib()
        self._h = c_vp()
        check(self._cdll.mv_resampler_create(int(src_rate), int(dst_rate), ctypes.byref(self._h)), self._cdll)
        info = MvResamplerInfo()
        check(self._cdll.mv_resampler_info(self._h, ctypes.byref(info)), self._cdll)
        self.src_rate, self.dst_rate = int(src_rate), int(dst_rate)
        self.up, self.down, self.half, self.K, self.tile, self.table_in_lds = (info.up, info.down, info.half, info.K, info.tile,
                                                                               bool(info.table_in_lds))

    def taps(self):
        """the 2 * half + 1 fp32 coefficients in filter order (numpy)"""
        import numpy as np
        n = 2 * self.half + 1
        buf = (c_f32 * n)()
        check(self._cdll.mv_resampler_taps(self._h, buf, n), self._cdll)
        return np.frombuffer(buf, dtype=np.float32).copy()

    def out_len(self, n):
        return int(self._cdll.mv_resampler_out_len(self._h, int(n)))

    def __call__(self, pcm, num_frames=None, target_db=None, max_gain_db=300.0):
        """int16 [B, L] or [B, L, C] (interleaved frames, any row stride) -> (wav [B, out_len(L)] fp32, num_out int64 [B], too_quiet int32 [B])
        on the caller's stream; ``num_frames`` int64 [B] = the rows' own frame counts, ``target_db`` None = no dB normalisation."""
        assert pcm.dtype == torch.int16 and pcm.dim() in (2, 3)
        if pcm.dim() == 2:
            pcm = pcm.unsqueeze(-1)
        B, L, C = pcm.shape
        if B and L and (pcm.stride(2) != 1 or pcm.stride(1) != C or pcm.stride(0) < L * C):
            pcm = pcm.contiguous()
        L_out = self.out_len(L)
        wav = torch.empty((B, L_out), dtype=torch.float32, device=pcm.device)
        num_out = torch.zeros((B,), dtype=torch.int64, device=pcm.device)
        flags = torch.zeros((B,), dtype=torch.int32, device=pcm.device)
        if num_frames is not None:
            num_frames = num_frames.to(device=pcm.device, dtype=torch.int64).contiguous()
            if num_frames.shape != (B,):
                raise ValueError(f'num_frames must have shape ({B},), got {tuple(num_frames.shape)}')
        nbytes = int(self._cdll.mv_resampler_workspace_bytes(self._h, B, L))
        ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=pcm.device)   # per call: streams never share it
        check(self._cdll.mv_resampler_forward_i16(self._h, pcm.data_ptr(), pcm.stride(0) if B and L else L * C, C, _ptr(num_frames), B, L,
                                                  0 if target_db is None else 1, float(target_db or 0.0), float(max_gain_db), wav.data_ptr(), L_out,
                                                  L_out, num_out.data_ptr(), flags.data_ptr(), ws.data_ptr(), nbytes, current_stream(pcm)), self._cdll)
        return wav, num_out, flags

    def __del__(self):
        try:
            if getattr(self, '_h', None):
                self._cdll.mv_resampler_destroy(self._h)
        except Exception:
            pass


def cosine(a, b, cdll=None):
    """[N, D] x [M, D] -> [N, M] cosine similarity on the device of ``a``."""
    cdll = cdll or lib()
    a = a.to(torch.float32).contiguous()
    b = b.to(device=a.device, dtype=torch.float32).contiguous()
    assert a.dim() == 2 and b.dim() == 2 and a.shape[1] == b.shape[1]
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    if out.numel():
        check(cdll.mv_cosine_f32(a.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], a.shape[1], out.data_ptr(),
                                 current_stream(a)), cdll)
    return out


def cosine_topk(q, g, k, slices_hint=0, cdll=None, to_host=False):
    """[N, D] queries x [M, D] gallery -> (scores fp32 [N, k], index int32 [N, k]) on the device of ``q``: per query the ``k`` best rows of
    ``cosine(q, g)`` -- the same score bits -- best first, equal scores by the lower row first, NaN above +inf; slots behind M hold
    (-inf, -1).  The [N, M] matrix is never built (mv_cosine_topk_f32).  ``slices_hint`` pins the number of gallery slices (tests).
    ``to_host``: the two as numpy arrays -- they share one device buffer, so both come down in one transfer."""
    cdll = cdll or lib()
    q = q.to(torch.float32).contiguous()
    g = g.to(device=q.device, dtype=torch.float32).contiguous()
    assert q.dim() == 2 and g.dim() == 2 and q.shape[1] == g.shape[1]
    n, m, dim, k = q.shape[0], g.shape[0], q.shape[1], int(k)
    out = torch.empty((2, n, max(k, 0)), dtype=torch.int32, device=q.device)
    scores, index = out[0].view(torch.float32), out[1]
    nbytes = int(cdll.mv_cosine_topk_workspace_bytes(n, m, dim, k, int(slices_hint)))
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=q.device)
    check(cdll.mv_cosine_topk_f32(q.data_ptr(), n, g.data_ptr(), m, dim, k, scores.data_ptr(), index.data_ptr(), int(slices_hint), ws.data_ptr(),
                                  nbytes, current_stream(q)), cdll)
    if to_host:
        host = out.cpu().numpy()
        return host[0].view('float32'), host[1]
    return scores, index


MV_SNORM_S, MV_SNORM_Z, MV_SNORM_T = 0, 1, 2
MV_COHORT_MAX_ROWS = 32768
SCORE_NORM_MODES = {'s': MV_SNORM_S, 'z': MV_SNORM_Z, 't': MV_SNORM_T}


def cohort_stats(x, cohort, top_n, rows_hint=0, cdll=None):
    """[N, D] embeddings x [M, D] cohort -> (mean, std), both fp32 [N], on the device of ``x``: the statistics of each row's
    min(top_n, M) largest cohort scores -- the scores are those of ``cosine(x, cohort)`` bit for bit, the sums run in fp64 in one fixed order
    (mv_cohort_stats_f32).  The [N, M] matrix is never built: the rows go through a workspace of R rows.  ``rows_hint`` pins R (tests)."""
    cdll = cdll or lib()
    x = x.to(torch.float32).contiguous()
    cohort = cohort.to(device=x.device, dtype=torch.float32).contiguous()
    assert x.dim() == 2 and cohort.dim() == 2 and x.shape[1] == cohort.shape[1]
    n, m, dim = x.shape[0], cohort.shape[0], x.shape[1]
    out = torch.empty((2, n), dtype=torch.float32, device=x.device)
    nbytes = int(cdll.mv_cohort_stats_workspace_bytes(n, m, dim, int(rows_hint)))
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=x.device)
    check(cdll.mv_cohort_stats_f32(x.data_ptr(), n, cohort.data_ptr(), m, dim, int(top_n), out[0].data_ptr(), out[1].data_ptr(), int(rows_hint),
                                   ws.data_ptr(), nbytes, current_stream(x)), cdll)
    return out[0], out[1]


def score_norm(scores, trial_stats, enroll_stats, mode='s', out=None, cdll=None):
    """scores [T, E] fp32 with ``trial_stats`` = (mean [T], std [T]) and ``enroll_stats`` = (mean [E], std [E]) -> the normalised matrix
    (mv_score_norm_f32): mode 'z' (s - mean_e) / std_e, 't' (s - mean_t) / std_t, 's' half their sum -- the numpy.float32 expression bit for
    bit.  The statistics of the side a mode does not use may be None.  ``out`` may be ``scores`` itself (in place)."""
    cdll = cdll or lib()
    if mode not in SCORE_NORM_MODES:
        raise ValueError(f"score_norm: mode {mode!r} is not one of 's', 'z', 't'")
    assert scores.dim() == 2 and scores.dtype == torch.float32 and scores.is_contiguous()
    n_t, n_e = scores.shape

    def side(stats, count, what):
        if stats is None:
            return None, None
        mean, std = (s.to(device=scores.device, dtype=torch.float32).contiguous() for s in stats)
        assert mean.shape == (count,) and std.shape == (count,), f'score_norm: {what} statistics are not [{count}]'
        return mean, std
    tm, ts = side(trial_stats, n_t, 'trial')
    em, es = side(enroll_stats, n_e, 'enrolment')
    if out is None:
        out = torch.empty_like(scores)
    assert out.shape == scores.shape and out.dtype == torch.float32 and out.is_contiguous() and out.device == scores.device
    check(cdll.mv_score_norm_f32(scores.data_ptr(), n_t, n_e, _ptr(tm), _ptr(ts), _ptr(em), _ptr(es), SCORE_NORM_MODES[mode], out.data_ptr(),
                                 current_stream(scores)), cdll)
    return out


MV_LOSS_CE, MV_LOSS_AM, MV_LOSS_ARM, MV_LOSS_AAM, MV_LOSS_SUBCENTER = 0, 1, 2, 3, 4
MV_DT_BF16 = 2
MV_MARGIN_SEG, MV_MARGIN_CHUNK, MV_MARGIN_SAVED = 4096, 8, 4
LOSS_KINDS = {'ce': MV_LOSS_CE, 'am': MV_LOSS_AM, 'arm': MV_LOSS_ARM, 'aam': MV_LOSS_AAM, 'subcenter': MV_LOSS_SUBCENTER}
_MARGIN_DTYPES = {torch.float32: MV_DT_F32, torch.float16: MV_DT_F16, torch.bfloat16: MV_DT_BF16}


class MvMarginLossCfg(ctypes.Structure):
    _fields_ = [('kind', c_i32), ('K', c_i32), ('easy_margin', c_i32), ('margin', c_f32), ('scale', c_f32), ('cos_m', c_f32), ('sin_m', c_f32),
                ('th', c_f32), ('mmm', c_f32), ('eps', c_f32)]


def margin_cfg(kind, margin=0.2, scale=32.0, easy_margin=False, K=1, label_smoothing=0.0):
    """MvMarginLossCfg of a loss: ``kind`` a key of LOSS_KINDS or an MV_LOSS_* code; cos_m, sin_m, th and mmm formed here in double from
    ``margin`` as the reference's constructors form them, then passed as floats"""
    import math
    cfg = MvMarginLossCfg()
    if isinstance(kind, str):
        if kind not in LOSS_KINDS:
            raise ValueError(f'margin loss: kind {kind!r} is not one of {sorted(LOSS_KINDS)}')
        kind = LOSS_KINDS[kind]
    cfg.kind, cfg.K, cfg.easy_margin = int(kind), int(K), int(bool(easy_margin))
    cfg.margin, cfg.scale, cfg.eps = float(margin), float(scale), float(label_smoothing)
    cfg.cos_m, cfg.sin_m = math.cos(margin), math.sin(margin)
    cfg.th, cfg.mmm = math.cos(math.pi - margin), 1.0 + math.cos(math.pi - margin)
    return cfg


def _margin_geometry(logits, labels, cfg, who):
    if logits.dim() != 2 or logits.dtype not in _MARGIN_DTYPES:
        raise ValueError(f'{who}: logits must be a 2-D fp32, fp16 or bf16 tensor, got {tuple(logits.shape)} {logits.dtype}')
    if logits.shape[1] > 1 and logits.stride(1) != 1:
        raise ValueError(f'{who}: the logits need unit stride along the classes')
    B, cols = logits.shape
    K = max(int(cfg.K), 1)
    if cols % K:
        raise ValueError(f'{who}: {cols} columns are no multiple of K = {K}')
    labels = labels.to(device=logits.device, dtype=torch.int64).contiguous()
    if labels.shape != (B,):
        raise ValueError(f'{who}: labels must have shape ({B},), got {tuple(labels.shape)}')
    stride = logits.stride(0) if B > 1 else max(logits.stride(0), cols)
    return labels, B, cols // K, stride


def margin_ce_forward(logits, labels, kind, margin=0.2, scale=32.0, easy_margin=False, K=1, label_smoothing=0.0, cdll=None):
    """The fused margin-softmax forward (mv_margin_ce_forward) on ``logits`` [B, N * K] (fp32 / fp16 / bf16, any row stride) and ``labels`` [B] ->
    (loss fp32 scalar, loss_rows fp32 [B], pred int32 [B], saved fp64 [B, MV_MARGIN_SAVED] = {max z, log sum exp(z - max), z_y, row loss}), all on
    the logits' device and stream.  ``kind``: 'ce', 'am', 'arm', 'aam' or 'subcenter'.  Nothing synchronises."""
    cdll = cdll or lib()
    cfg = margin_cfg(kind, margin, scale, easy_margin, K, label_smoothing)
    labels, B, N, stride = _margin_geometry(logits, labels, cfg, 'margin_ce_forward')
    dev = logits.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    loss_rows = torch.empty((B,), dtype=torch.float32, device=dev)
    pred = torch.empty((B,), dtype=torch.int32, device=dev)
    saved = torch.empty((B, MV_MARGIN_SAVED), dtype=torch.float64, device=dev)
    nbytes = int(cdll.mv_margin_ce_workspace_bytes(B, N, int(cfg.K)))
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)
    check(cdll.mv_margin_ce_forward(ctypes.byref(cfg), logits.data_ptr(), _MARGIN_DTYPES[logits.dtype], labels.data_ptr(), B, N, stride,
                                    loss.data_ptr(), loss_rows.data_ptr(), pred.data_ptr(), saved.data_ptr(), ws.data_ptr(), nbytes,
                                    current_stream(logits)), cdll)
    if B == 0:
        loss.fill_(float('nan'))   # the mean of no rows, as torch's
    return loss, loss_rows, pred, saved


def margin_ce_backward(logits, labels, saved, grad_out, kind, margin=0.2, scale=32.0, easy_margin=False, K=1, label_smoothing=0.0, out=None,
                       cdll=None):
    """The gradient of the loss of ``margin_ce_forward`` with respect to the logits, in the logits' dtype (mv_margin_ce_backward): ``saved`` from the
    forward of the same arguments, ``grad_out`` the upstream scalar as an fp32 tensor on the device (read there: nothing synchronises).  ``out``:
    where to write; ``out=logits`` runs in place, any other overlap is refused."""
    cdll = cdll or lib()
    cfg = margin_cfg(kind, margin, scale, easy_margin, K, label_smoothing)
    labels, B, N, stride = _margin_geometry(logits, labels, cfg, 'margin_ce_backward')
    grad_out = grad_out.to(device=logits.device, dtype=torch.float32).reshape(-1)
    assert grad_out.numel() == 1, 'margin_ce_backward: grad_out is not a scalar'
    assert saved.shape == (B, MV_MARGIN_SAVED) and saved.dtype == torch.float64 and saved.is_contiguous() and saved.device == logits.device
    if out is None:
        out = torch.empty((B, logits.shape[1]), dtype=logits.dtype, device=logits.device)
    assert out.shape == logits.shape and out.dtype == logits.dtype and out.device == logits.device
    assert out.shape[1] <= 1 or out.stride(1) == 1, 'margin_ce_backward: out needs unit stride along the classes'
    out_stride = out.stride(0) if B > 1 else max(out.stride(0), out.shape[1])
    check(cdll.mv_margin_ce_backward(ctypes.byref(cfg), logits.data_ptr(), _MARGIN_DTYPES[logits.dtype], labels.data_ptr(), B, N, stride,
                                     saved.data_ptr(), grad_out.data_ptr(), out.data_ptr(), out_stride, current_stream(logits)), cdll)
    return out


MV_SF2_TYPE_C, MV_SF2_TYPE_A, MV_SF2_MAX_T, MV_SF2_SAVED = 0, 1, 8, 2
SF2_MARGIN_TYPES = {'C': MV_SF2_TYPE_C, 'A': MV_SF2_TYPE_A}
MV_TRIPLET_MAX_B, MV_TRIPLET_MAX_D, MV_TRIPLET_ANCHORS = 4096, 2048, 4


class MvSphereFace2Cfg(ctypes.Structure):
    _fields_ = [('margin_type', c_i32), ('t', c_i32), ('scale', c_f32), ('margin', c_f32), ('lanbuda', c_f32), ('cos_m', c_f32), ('sin_m', c_f32),
                ('th', c_f32), ('mmm', c_f32)]


class MvTripletCfg(ctypes.Structure):
    _fields_ = [('margin', ctypes.c_double), ('absolute_loss_weight', ctypes.c_double), ('ap_value', ctypes.c_double),
                ('an_value', ctypes.c_double), ('normalize', c_i32), ('add_absolute', c_i32)]


def sphereface2_cfg(margin=0.2, scale=32.0, lanbuda=0.7, t=3, margin_type='C'):
    """MvSphereFace2Cfg: ``margin_type`` 'C', 'A' or an MV_SF2_TYPE_* code; cos_m, sin_m, th and mmm formed here in double from ``margin`` as the
    reference's constructor forms them, then passed as floats.  ``t`` must be an integer (the library refuses one outside 1 .. 8)."""
    import math
    cfg = MvSphereFace2Cfg()
    if isinstance(margin_type, str):
        if margin_type not in SF2_MARGIN_TYPES:
            raise ValueError(f'sphereface2: margin_type {margin_type!r} is not one of {sorted(SF2_MARGIN_TYPES)}')
        margin_type = SF2_MARGIN_TYPES[margin_type]
    if int(t) != t:
        raise ValueError(f'sphereface2: t = {t!r} is not an integer')
    cfg.margin_type, cfg.t = int(margin_type), int(t)
    cfg.scale, cfg.margin, cfg.lanbuda = float(scale), float(margin), float(lanbuda)
    cfg.cos_m, cfg.sin_m = math.cos(margin), math.sin(margin)
    cfg.th, cfg.mmm = math.cos(math.pi - margin), 1.0 + math.cos(math.pi - margin)
    return cfg


def triplet_cfg(margin=0.5, normalize=True, add_absolute=True, absolute_loss_weight=1.0, ap_value=0.8, an_value=0.4):
    cfg = MvTripletCfg()
    cfg.margin, cfg.absolute_loss_weight, cfg.ap_value, cfg.an_value = float(margin), float(absolute_loss_weight), float(ap_value), float(an_value)
    cfg.normalize, cfg.add_absolute = int(bool(normalize)), int(bool(add_absolute))
    return cfg


def _rows_geometry(x, labels, who, what):
    """(labels int64 [B] on x's device, B, columns, row stride) of a 2-D fp32 / fp16 / bf16 matrix with unit stride along its columns"""
    if x.dim() != 2 or x.dtype not in _MARGIN_DTYPES:
        raise ValueError(f'{who}: {what} must be a 2-D fp32, fp16 or bf16 tensor, got {tuple(x.shape)} {x.dtype}')
    if x.shape[1] > 1 and x.stride(1) != 1:
        raise ValueError(f'{who}: the {what} need unit stride along their columns')
    B, cols = x.shape
    labels = labels.to(device=x.device, dtype=torch.int64).contiguous()
    if labels.shape != (B,):
        raise ValueError(f'{who}: labels must have shape ({B},), got {tuple(labels.shape)}')
    return labels, B, cols, (x.stride(0) if B > 1 else max(x.stride(0), cols))


def _sf2_bias(bias, logits, who):
    if bias.dtype != torch.float32 or bias.numel() != 1 or bias.device != logits.device:
        raise ValueError(f'{who}: bias must be one fp32 value on the logits\' device, got {tuple(bias.shape)} {bias.dtype} on {bias.device}')
    return bias.detach()


def sphereface2_forward(logits, labels, bias, margin=0.2, scale=32.0, lanbuda=0.7, t=3, margin_type='C', cdll=None):
    """The fused SphereFace2 forward (mv_sphereface2_forward) on the cosines ``logits`` [B, N] (fp32 / fp16 / bf16, any row stride), ``labels`` [B]
    and ``bias``, one fp32 value ON THE LOGITS' DEVICE (read there) -> (loss fp32 scalar, loss_rows fp32 [B], pred int32 [B], saved fp64
    [B, MV_SF2_SAVED] = {row loss, the row's sum of the column weights}), all on the logits' device and stream.  Nothing synchronises."""
    cdll = cdll or lib()
    cfg = sphereface2_cfg(margin, scale, lanbuda, t, margin_type)
    labels, B, N, stride = _rows_geometry(logits, labels, 'sphereface2_forward', 'logits')
    bias = _sf2_bias(bias, logits, 'sphereface2_forward')
    dev = logits.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    loss_rows = torch.empty((B,), dtype=torch.float32, device=dev)
    pred = torch.empty((B,), dtype=torch.int32, device=dev)
    saved = torch.empty((B, MV_SF2_SAVED), dtype=torch.float64, device=dev)
    nbytes = int(cdll.mv_sphereface2_workspace_bytes(B, N))
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)
    check(cdll.mv_sphereface2_forward(ctypes.byref(cfg), logits.data_ptr(), _MARGIN_DTYPES[logits.dtype], labels.data_ptr(), bias.data_ptr(), B, N,
                                      stride, loss.data_ptr(), loss_rows.data_ptr(), pred.data_ptr(), saved.data_ptr(), ws.data_ptr(), nbytes,
                                      current_stream(logits)), cdll)
    if B == 0:
        loss.fill_(float('nan'))   # the mean of no rows, as torch's
    return loss, loss_rows, pred, saved


def sphereface2_backward(logits, labels, bias, saved, grad_out, margin=0.2, scale=32.0, lanbuda=0.7, t=3, margin_type='C', out=None, cdll=None):
    """The gradients of the loss of ``sphereface2_forward`` (mv_sphereface2_backward) -> (grad of the logits in their dtype, bias_grad fp32 [1]):
    ``saved`` from the forward of the same arguments, ``grad_out`` the upstream scalar as an fp32 tensor on the device (read there: nothing
    synchronises).  ``out``: where to write the logits' gradient; ``out=logits`` runs in place, any other overlap is refused."""
    cdll = cdll or lib()
    cfg = sphereface2_cfg(margin, scale, lanbuda, t, margin_type)
    labels, B, N, stride = _rows_geometry(logits, labels, 'sphereface2_backward', 'logits')
    bias = _sf2_bias(bias, logits, 'sphereface2_backward')
    grad_out = grad_out.to(device=logits.device, dtype=torch.float32).reshape(-1)
    assert grad_out.numel() == 1, 'sphereface2_backward: grad_out is not a scalar'
    assert saved.shape == (B, MV_SF2_SAVED) and saved.dtype == torch.float64 and saved.is_contiguous() and saved.device == logits.device
    if out is None:
        out = torch.empty((B, N), dtype=logits.dtype, device=logits.device)
    assert out.shape == logits.shape and out.dtype == logits.dtype and out.device == logits.device
    assert out.shape[1] <= 1 or out.stride(1) == 1, 'sphereface2_backward: out needs unit stride along the classes'
    out_stride = out.stride(0) if B > 1 else max(out.stride(0), N)
    bias_grad = torch.zeros((1,), dtype=torch.float32, device=logits.device) if B == 0 else torch.empty((1,), dtype=torch.float32, device=logits.device)
    check(cdll.mv_sphereface2_backward(ctypes.byref(cfg), logits.data_ptr(), _MARGIN_DTYPES[logits.dtype], labels.data_ptr(), bias.data_ptr(), B, N,
                                       stride, saved.data_ptr(), grad_out.data_ptr(), out.data_ptr(), out_stride, bias_grad.data_ptr(),
                                       current_stream(logits)), cdll)
    return out, bias_grad


def triplet_forward(features, labels, margin=0.5, normalize=True, add_absolute=True, absolute_loss_weight=1.0, ap_value=0.8, an_value=0.4,
                    cdll=None):
    """The batch-hard triplet term (mv_triplet_forward; WITHOUT the cross-entropy of the class) on ``features`` [B, D] (fp32 / fp16 / bf16, any
    row stride) and ``labels`` [B] -> (loss fp32 scalar, mined fp64 [B, 2] = {hardest positive, hardest negative similarity}, index int32
    [B, 2] = their rows, -1 for no negative), all on the features' device and stream.  Nothing synchronises."""
    cdll = cdll or lib()
    cfg = triplet_cfg(margin, normalize, add_absolute, absolute_loss_weight, ap_value, an_value)
    labels, B, D, stride = _rows_geometry(features, labels, 'triplet_forward', 'features')
    dev = features.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    mined = torch.empty((B, 2), dtype=torch.float64, device=dev)
    index = torch.empty((B, 2), dtype=torch.int32, device=dev)
    nbytes = int(cdll.mv_triplet_workspace_bytes(B, D))
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)
    check(cdll.mv_triplet_forward(ctypes.byref(cfg), features.data_ptr(), _MARGIN_DTYPES[features.dtype], labels.data_ptr(), B, D, stride,
                                  loss.data_ptr(), mined.data_ptr(), index.data_ptr(), ws.data_ptr(), nbytes, current_stream(features)), cdll)
    if B == 0:
        loss.fill_(float('nan'))
    return loss, mined, index


def triplet_backward(features, labels, mined, index, grad_out, margin=0.5, normalize=True, add_absolute=True, absolute_loss_weight=1.0,
                     ap_value=0.8, an_value=0.4, out=None, cdll=None):
    """The gradient of the loss of ``triplet_forward`` with respect to the features, in their dtype (mv_triplet_backward): ``mined`` and ``index``
    from the forward of the same arguments (``labels`` is only checked for its shape: the mined rows carry what the gradient needs), ``grad_out``
    the upstream scalar as an fp32 tensor on the device."""
    cdll = cdll or lib()
    cfg = triplet_cfg(margin, normalize, add_absolute, absolute_loss_weight, ap_value, an_value)
    labels, B, D, stride = _rows_geometry(features, labels, 'triplet_backward', 'features')
    dev = features.device
    grad_out = grad_out.to(device=dev, dtype=torch.float32).reshape(-1)
    assert grad_out.numel() == 1, 'triplet_backward: grad_out is not a scalar'
    assert mined.shape == (B, 2) and mined.dtype == torch.float64 and mined.is_contiguous() and mined.device == dev
    assert index.shape == (B, 2) and index.dtype == torch.int32 and index.is_contiguous() and index.device == dev
    if out is None:
        out = torch.empty((B, D), dtype=features.dtype, device=dev)
    assert out.shape == features.shape and out.dtype == features.dtype and out.device == dev
    assert out.shape[1] <= 1 or out.stride(1) == 1, 'triplet_backward: out needs unit stride along the features'
    out_stride = out.stride(0) if B > 1 else max(out.stride(0), D)
    nbytes = int(cdll.mv_triplet_workspace_bytes(B, D))
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)
    check(cdll.mv_triplet_backward(ctypes.byref(cfg), features.data_ptr(), _MARGIN_DTYPES[features.dtype], B, D, stride, mined.data_ptr(),
                                   index.data_ptr(), grad_out.data_ptr(), out.data_ptr(), out_stride, ws.data_ptr(), nbytes,
                                   current_stream(features)), cdll)
    return out


MV_VAD_TILE_FRAMES = 256
VAD_DEFAULTS =dict(frame_length=400, frame_shift=160, frames_context=0, energy_threshold=5.0, energy_mean_scale=0.5, proportion_threshold=0.6,
                    scale=32768.0)   # compute-vad's own; scale: [-1, 1) samples in the int16 range its thresholds assume


def vad_cfg(**cfg):
    """MvVadCfg of VAD_DEFAULTS with ``cfg`` on top; an unknown field is a TypeError"""
    unknown = sorted(set(cfg) - set(VAD_DEFAULTS))
    if unknown:
        raise TypeError(f'vad_energy: unknown configuration field(s) {unknown}; the fields are {sorted(VAD_DEFAULTS)}')
    values = dict(VAD_DEFAULTS, **cfg)
    out = MvVadCfg()
    for name in ('frame_length', 'frame_shift', 'frames_context'):
        setattr(out, name, int(values[name]))
    for name in ('energy_threshold', 'energy_mean_scale', 'proportion_threshold', 'scale'):
        setattr(out, name, float(values[name]))
    return out


def vad_num_frames(n, frame_length=400, frame_shift=160):
    return 0 if n < frame_length else 1 + (n - frame_length) // frame_shift


def vad_energy(wav, lengths=None, max_runs=None, cdll=None, **cfg):
    """Energy VAD of fp32 waveform rows (mv_vad_energy_f32): ``wav`` [L] or [B, L] with unit stride along time (any row stride and
    alignment), ``lengths`` int64 [B] = the rows' own sample counts -> dict of tensors on wav's device:
    'num_frames' int32 [B], 'num_runs' int32 [B], 'runs' int32 [B, max_runs, 2] (frames [a, b); the first min(num_runs, max_runs) pairs of a
    row are written), 'log_energy' fp64 [B, T(L)], 'threshold' fp64 [B], 'decisions' uint8 [B, T(L)] (zeros at t >= num_frames), and 'packed':
    the int32 buffer the first three are views of -- one download brings them all.  ``max_runs`` None = ceil(T(L) / 2), the most a row can
    have.  ``cfg``: the fields of VAD_DEFAULTS.  Nothing synchronises."""
    cdll = cdll or lib()
    assert wav.dtype == torch.float32 and wav.dim() in (1, 2)
    if wav.dim() == 1:
        wav = wav.unsqueeze(0)
    B, L = wav.shape
    if L > 1 and wav.stride(1) != 1 or B > 1 and wav.stride(0) < L:
        wav = wav.contiguous()
    c = vad_cfg(**cfg)
    if lengths is not None:
        lengths = lengths.to(device=wav.device, dtype=torch.int64).contiguous()
        if lengths.shape != (B,):
            raise ValueError(f'lengths must have shape ({B},), got {tuple(lengths.shape)}')
    # (a configuration the library refuses gives T = 0 here and its message below)
    T = vad_num_frames(L, c.frame_length, c.frame_shift) if 1 <= c.frame_shift <= c.frame_length else 0
    if max_runs is None:
        max_runs = (T + 1) // 2
    packed = torch.empty((2 * B + 2 * B * max(int(max_runs), 0),), dtype=torch.int32, device=wav.device)
    num_frames, num_runs, runs = packed[:B], packed[B:2 * B], packed[2 * B:].view(B, max(int(max_runs), 0), 2)
    log_energy = torch.empty((B, T), dtype=torch.float64, device=wav.device)
    threshold = torch.empty((B,), dtype=torch.float64, device=wav.device)
    decisions = torch.empty((B, T), dtype=torch.uint8, device=wav.device)
    nbytes = int(cdll.mv_vad_energy_workspace_bytes(ctypes.byref(c), B, L))
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=wav.device)   # per call: streams never share it
    check(cdll.mv_vad_energy_f32(ctypes.byref(c), wav.data_ptr(), wav.stride(0) if B > 1 else L, _ptr(lengths), B, L, num_frames.data_ptr(),
                                 num_runs.data_ptr(), runs.data_ptr() if runs.numel() else None, int(max_runs), log_energy.data_ptr() if T else None,
                                 threshold.data_ptr(), decisions.data_ptr() if T else None, ws.data_ptr(), nbytes, current_stream(wav)), cdll)
    return dict(num_frames=num_frames, num_runs=num_runs, runs=runs, log_energy=log_energy, threshold=threshold, decisions=decisions, packed=packed)


MV_VAD_REGION_TILE = 256      # runs per tile of mv_vad_regions_i32, regions per search table of mv_wave_gather_f32
MV_WAVE_GATHER_TILE = 4096    # outputs per workgroup of mv_wave_gather_f32


def vad_regions(vad_out, lengths, frame_shift, min_silence, min_speech, speech_pad, L=None, cdll=None):
    """The runs of ``vad_energy`` (its dict, as it is) -> the speech regions in samples (mv_vad_regions_i32: the four steps of
    ``EnergyVad.smooth`` in integers on the device): (num_regions int32 [B], regions int32 [B, max_runs, 2] -- the first num_regions pairs of a
    row are written --, kept int64 [B] = the sum of a row's region lengths).  ``lengths`` int64 [B] = the rows' own sample counts, ``L`` the
    samples of a full row (None: ``lengths`` are taken as they are, and have to be given); the other four in samples.  A row whose run list was
    truncated (num_runs above max_runs) has -1 in num_regions and kept.  Nothing synchronises."""
    cdll = cdll or lib()
    num_frames, num_runs, runs = vad_out['num_frames'], vad_out['num_runs'], vad_out['runs']
    B, max_runs = runs.shape[0], runs.shape[1]
    if lengths is not None:
        lengths = lengths.to(device=runs.device, dtype=torch.int64).contiguous()
        if lengths.shape != (B,):
            raise ValueError(f'lengths must have shape ({B},), got {tuple(lengths.shape)}')
    elif L is None:
        raise ValueError('vad_regions: lengths or L')
    c = MvVadSmoothCfg(int(frame_shift), int(min_silence), int(min_speech), int(speech_pad))
    num_regions = torch.empty((B,), dtype=torch.int32, device=runs.device)
    regions = torch.empty((B, max_runs, 2), dtype=torch.int32, device=runs.device)
    kept = torch.empty((B,), dtype=torch.int64, device=runs.device)
    nbytes = int(cdll.mv_vad_regions_workspace_bytes(B, max_runs))
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=runs.device)   # per call: streams never share it
    check(cdll.mv_vad_regions_i32(ctypes.byref(c), num_frames.data_ptr(), num_runs.data_ptr(), runs.data_ptr() if runs.numel() else None, max_runs,
                                  _ptr(lengths), B, 0x7FFFFFFF if L is None else int(L), num_regions.data_ptr(),
                                  regions.data_ptr() if regions.numel() else None, kept.data_ptr(), ws.data_ptr(), nbytes, current_stream(runs)), cdll)
    return num_regions, regions, kept


def wave_gather(wav, lengths, num_regions, regions, cdll=None):
    """Row b of the result = wav[b, s : e) of the row's first num_regions[b] ``regions`` (int32 [B, max_regions, 2], clamped to the row's
    ``lengths`` entry; None: L) one behind the other, zeros behind them (mv_wave_gather_f32; the samples are copied bit for bit) ->
    (out fp32 [B, L], out_samples int64 [B]); a row with num_regions < 0 is zeros with out_samples -1.  Nothing synchronises."""
    cdll = cdll or lib()
    assert wav.dtype == torch.float32 and wav.dim() == 2 and regions.dim() == 3 and regions.shape[0] == wav.shape[0] and regions.shape[2] == 2
    B, L = wav.shape
    if L > 1 and wav.stride(1) != 1 or B > 1 and wav.stride(0) < L:
        wav = wav.contiguous()
    if lengths is not None:
        lengths = lengths.to(device=wav.device, dtype=torch.int64).contiguous()
        if lengths.shape != (B,):
            raise ValueError(f'lengths must have shape ({B},), got {tuple(lengths.shape)}')
    num_regions = num_regions.to(device=wav.device, dtype=torch.int32).contiguous()
    regions = regions.to(device=wav.device, dtype=torch.int32).contiguous()
    max_regions = regions.shape[1]
    out = torch.empty((B, L), dtype=torch.float32, device=wav.device)
    out_samples = torch.empty((B,), dtype=torch.int64, device=wav.device)
    nbytes = int(cdll.mv_wave_gather_workspace_bytes(B, max_regions))
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=wav.device)
    check(cdll.mv_wave_gather_f32(wav.data_ptr() if L else None, wav.stride(0) if B > 1 else L, _ptr(lengths), num_regions.data_ptr(),
                                  regions.data_ptr() if regions.numel() else None, max_regions, B, L, out.data_ptr() if L else None, L, L,
                                  out_samples.data_ptr(), ws.data_ptr(), nbytes, current_stream(wav)), cdll)
    return out, out_samples


def wave_chunks(wav, start, length, chunk_len, target_db=None, max_gain_db=300.0, cdll=None):
    """One resident fp32 waveform [L] and the chunk table (int64 tensors start / length, [n]) -> (rows [n, chunk_len] fp32, too_quiet int32
    [n]): row i = wav[start_i : start_i + length_i] followed by zeros, dB-normalised over the padded row unless ``target_db`` is None."""
    cdll = cdll or lib()
    assert wav.dim() == 1 and wav.dtype == torch.float32 and start.shape == length.shape and start.dim() == 1
    wav = wav.contiguous()
    start = start.to(device=wav.device, dtype=torch.int64).contiguous()
    length = length.to(device=wav.device, dtype=torch.int64).contiguous()
    n, chunk_len = start.shape[0], int(chunk_len)
    rows = torch.empty((n, chunk_len), dtype=torch.float32, device=wav.device)
    flags = torch.zeros((n,), dtype=torch.int32, device=wav.device)
    check(cdll.mv_wave_chunks_f32(wav.data_ptr(), wav.shape[0], start.data_ptr(), length.data_ptr(), n, chunk_len, 0 if target_db is None else 1,
                                  float(target_db or 0.0), float(max_gain_db), rows.data_ptr(), chunk_len, flags.data_ptr(), current_stream(wav)),
          cdll)
    return rows, flags


def affinity_laplacian(sim, n_prune, cdll=None):
    """Cosine matrix [N, N] fp32 -> (M [N, N] fp32, degree [N] fp64): per row the ``n_prune`` smallest entries dropped (ties: the lower column
    first), M = 0.5 * (pruned + pruned^T) with a zero diagonal, degree_i = sum_j |M_ij|.  The Laplacian is diag(degree) - M."""
    cdll = cdll or lib()
    assert sim.dim() == 2 and sim.shape[0] == sim.shape[1] and sim.dtype == torch.float32
    sim = sim.contiguous()
    N = sim.shape[0]
    M = torch.empty_like(sim)
    degree = torch.empty((N,), dtype=torch.float64, device=sim.device)
    ws = torch.empty((max(int(cdll.mv_affinity_laplacian_workspace_bytes(N)), 16),), dtype=torch.uint8, device=sim.device)
    check(cdll.mv_affinity_laplacian_f32(sim.data_ptr(), N, int(n_prune), M.data_ptr(), degree.data_ptr(), ws.data_ptr(), ws.numel(),
                                         current_stream(sim)), cdll)
    return M, degree


MV_ERR_NOT_CONVERGED = -6


def laplacian_eig_lowest(M, degree, m=16, block=0, filter_degree=None, max_iters=None, tol=None, seed=None, cdll=None):
    """The ``m`` lowest eigenpairs of diag(degree) - M (mv_laplacian_eig_lowest) -> (eigenvalues float64 numpy [m] ascending, eigenvectors
    [N, m] float64 on the device of ``M``, info dict).  Synchronises the current stream.  Raises RuntimeError carrying the residual when the
    iteration does not converge: there is no other path."""
    cdll = cdll or lib()
    assert M.dim() == 2 and M.shape[0] == M.shape[1] and M.dtype == torch.float32 and degree.dtype == torch.float64
    M, degree = M.contiguous(), degree.to(M.device).contiguous()
    N = M.shape[0]
    cfg = MvEigCfg()
    cdll.mv_laplacian_eig_default_cfg(ctypes.byref(cfg))
    cfg.m, cfg.block = int(m), int(block)
    for field, value in (('degree', filter_degree), ('max_iters', max_iters), ('tol', tol), ('seed', seed)):
        if value is not None:
            setattr(cfg, field, value)
    nbytes = int(cdll.mv_laplacian_eig_lowest_workspace_bytes(N, ctypes.byref(cfg)))
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=M.device)
    lambdas = (ctypes.c_double * max(cfg.m, 1))()
    vecs = torch.empty((N, max(cfg.m, 0)), dtype=torch.float64, device=M.device)
    info = MvEigInfo()
    rc = cdll.mv_laplacian_eig_lowest(M.data_ptr(), degree.data_ptr(), N, ctypes.byref(cfg), lambdas, vecs.data_ptr(), ctypes.byref(info),
                                      ws.data_ptr(), nbytes, current_stream(M))
    out = {f: getattr(info, f) for f, _ in MvEigInfo._fields_}
    if rc == MV_ERR_NOT_CONVERGED:
        raise RuntimeError(f'libmvector_hip: {cdll.mv_last_error().decode(errors="replace")} (code {rc}; residual {info.residual:.3e}, '
                           f'ub {info.ub:.3e}, {info.iterations} iterations, {info.products} products)')
    check(rc, cdll)
    import numpy as np
    return np.array(lambdas[:cfg.m], dtype=np.float64), vecs, out


def sort_scores(scores, cdll=None):
    """fp32 scores of any shape -> (sorted [N] fp32 ascending, index [N] int32) with sorted[i] = scores.reshape(-1)[index[i]], in the order
    of ``numpy.argsort(scores, kind='stable')``: equal scores keep their flat-index order, NaNs come last (mv_sort_scores_f32)."""
    cdll = cdll or lib()
    assert scores.dtype == torch.float32
    flat = scores.contiguous().reshape(-1)
    N = flat.shape[0]
    out = torch.empty((N,), dtype=torch.float32, device=flat.device)
    index = torch.empty((N,), dtype=torch.int32, device=flat.device)   # N <= 2^31 - 1: every index is a non-negative int32
    nbytes = int(cdll.mv_sort_scores_workspace_bytes(N))
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=flat.device)
    check(cdll.mv_sort_scores_f32(flat.data_ptr(), N, out.data_ptr(), index.data_ptr(), ws.data_ptr(), nbytes, current_stream(flat)), cdll)
    return out, index


def verification_metrics(scores, trial_labels, enroll_labels, p_target=0.01, c_miss=1, c_fa=1, curve=False, cdll=None):
    """Score matrix [n_trials, n_enroll] fp32 and the two int32 label vectors, all on one device -> dict of the counts EER, minDCF and the
    threshold are made of (the fields of MvVerifResult: n_target, n_impostor, i1, i2, tgt_i1, tgt_i2, min_cost, score_i1); with ``curve`` also
    'sorted_scores' [N] fp32 and 'tgt_cum' [N] int32 (targets among the sorted positions 0 .. i) on the device.  Equal scores are ordered by
    their flat index.  Synchronises the current stream (mv_verif_metrics_f32)."""
    cdll = cdll or lib()
    assert scores.dim() == 2 and scores.dtype == torch.float32
    scores = scores.contiguous()
    n_trials, n_enroll = scores.shape
    trial_labels = trial_labels.to(device=scores.device, dtype=torch.int32).contiguous()
    enroll_labels = enroll_labels.to(device=scores.device, dtype=torch.int32).contiguous()
    assert trial_labels.shape == (n_trials,) and enroll_labels.shape == (n_enroll,)
    N = n_trials * n_enroll
    cfg = MvVerifCfg(float(p_target), float(c_miss), float(c_fa))
    res = MvVerifResult()
    sorted_scores = torch.empty((N,), dtype=torch.float32, device=scores.device) if curve else None
    tgt_cum = torch.empty((N,), dtype=torch.int32, device=scores.device) if curve else None
    nbytes = int(cdll.mv_verif_metrics_workspace_bytes(n_trials, n_enroll))
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=scores.device)
    check(cdll.mv_verif_metrics_f32(scores.data_ptr(), n_trials, n_enroll, trial_labels.data_ptr(), enroll_labels.data_ptr(), ctypes.byref(cfg),
                                    ctypes.byref(res), _ptr(sorted_scores), _ptr(tgt_cum), ws.data_ptr(), nbytes, current_stream(scores)), cdll)
    out = {f: getattr(res, f) for f, _ in MvVerifResult._fields_ if f != 'reserved'}
    if curve:
        out['sorted_scores'], out['tgt_cum'] = sorted_scores, tgt_cum
    return out


MV_ERR_UNSUPPORTED = -3
CAM_FORM_AUTO, CAM_FORM_BLOCK, CAM_FORM_LAYER, CAM_FORM_LONG = 0, 1, 2, 3
CAM_LAYER_FIELDS = ('w1', 'bn1_s', 'bn1_t', 'bn2_s', 'bn2_t', 'wl', 'wa', 'ba', 'wb', 'bb')


def cam_dense_block(x, c_in, layers, dil, seg_len=100, form=CAM_FORM_AUTO, cdll=None):
    """The dense layers of one CAM++ block in place on the fp16 concat buffer x [B, T2, ldx] (mv_cam_dense_block_f16).  layers: one dict per
    layer with the tensors of CAM_LAYER_FIELDS (w1 / wl packed by mv_conv1d_pack_weight).  Returns the form each layer ran."""
    cdll = cdll or lib()
    B, T2, ldx = x.shape
    n = len(layers)
    nbytes = c_sz(0)
    check(cdll.mv_cam_dense_block_workspace_bytes(B, T2, n, ctypes.byref(nbytes)), cdll)
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=x.device)
    arrays = [(c_vp * n)(*[L[f].data_ptr() for L in layers]) for f in CAM_LAYER_FIELDS]
    used = (c_i32 * n)()
    check(cdll.mv_cam_dense_block_f16(x.data_ptr(), ldx, B, T2, c_in, n, *arrays, dil, seg_len, form, used, ws.data_ptr(), nbytes.value,
                                      current_stream(x)), cdll)
    return list(used)
