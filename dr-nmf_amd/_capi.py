"""ctypes binding of libdrnmf.so (C ABI in include/drnmf.h; the LSTM baseline's in include/drnmf_lstm.h; the
STOI score's in include/drnmf_score.h; the ragged STFT / iSTFT / int16 stages' in include/drnmf_enhance.h; the
device-side SDR's in include/drnmf_sdr.h; the training-data front end's in include/drnmf_dataset.h; the streaming
STFT / iSTFT's in include/drnmf_stream.h; the sparse-NMF baseline's inference in include/drnmf_snmf.h, on fp16
operands in include/drnmf_snmf_f16.h, with per-row noise atoms in include/drnmf_snmf_adapt.h, their online
form in include/drnmf_snmf_online.h, under the KL cost in include/drnmf_snmf_kl.h; ESTOI beside STOI in include/drnmf_estoi.h;
the device-side mixer's in include/drnmf_mix.h; the waveform losses' in include/drnmf_waveloss.h; the device-side
reverberator's in include/drnmf_reverb.h; the STOI criterion's in include/drnmf_stoi_loss.h; the device-side
resampler's in include/drnmf_resample.h).

The library is the product path: there is NO fallback.  If the shared object is missing or a
call fails, an exception is raised.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libdrnmf.so")

OK = 0
COMM_ID_BYTES = 128          # DRNMF_COMM_ID_BYTES
DIV_ED, DIV_KL, DIV_BETA = 0, 1, 2
MATRIX_F32, MATRIX_BF16X3 = 0, 1     # DRNMF_MATRIX_*


class CellDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("B", "T", "F", "N", "K", "n_D", "n_alph", "alph_len", "n_lam",
                 "return_all_hidden", "operand_f16", "divergence")]


class DenseDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("B", "T", "F", "N", "K", "connect_input", "activation", "return_all_hidden",
                 "operand_f16")]


ACTIVATIONS = {"linear": 0, "relu": 1, "tanh": 2, "sigmoid": 3, "softplus": 4, "hard_sigmoid": 5}

_vp, _i32, _i64, _f32, _sz = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_size_t
_DP = C.POINTER(CellDesc)
_DDP = C.POINTER(DenseDesc)

# name -> (restype, argtypes); mirrors include/drnmf.h one to one
SIGNATURES = {
    "drnmf_version": (_i32, []),
    "drnmf_create": (_i32, [C.POINTER(_vp), _i32]),
    "drnmf_destroy": (_i32, [_vp]),
    "drnmf_create_unbound": (_i32, [C.POINTER(_vp)]),
    "drnmf_last_error": (C.c_char_p, [_vp]),
    "drnmf_params_bytes": (_sz, [_DP]),
    "drnmf_prepare_params": (_i32, [_vp, _DP, _vp, _vp, _vp, _vp, _vp]),
    "drnmf_cell_workspace_bytes": (_sz, [_DP]),
    "drnmf_cell_launches_per_frame": (_i32, [_DP]),
    "drnmf_cell_forward": (_i32, [_vp, _DP, _vp, _f32, _vp, _vp, _f32, _f32, _f32, _vp, _vp, _sz,
                                  _vp]),
    "drnmf_cell_forward_stateful": (_i32, [_vp, _DP, _vp, _f32, _vp, _vp, _f32, _f32, _f32, _vp, _vp,
                                           _vp, _vp, _sz, _vp]),
    "drnmf_cell_forward_ista": (_i32, [_vp, _DP, _vp, _f32, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _sz,
                                       _vp]),
    "drnmf_cell_profile": (_i32, [_vp, _DP, _vp, _f32, _vp, _vp, _f32, _f32, _f32, _vp, _vp, _sz,
                                  _vp, _i32, C.POINTER(C.c_float)]),
    "drnmf_dense_params_bytes": (_sz, [_DDP]),
    "drnmf_dense_prepare_params": (_i32, [_vp, _DDP, _vp, _vp, _vp, _vp, _vp, _vp]),
    "drnmf_dense_workspace_bytes": (_sz, [_DDP]),
    "drnmf_dense_cell_forward": (_i32, [_vp, _DDP, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _sz,
                                        _vp]),
    "drnmf_dense_backward_workspace_bytes": (_sz, [_DDP]),
    "drnmf_dense_cell_backward": (_i32, [_vp, _DDP, _vp, _f32] + [_vp] * 13 + [_sz, _vp]),
    "drnmf_dense_cell_forward_dropout": (_i32, [_vp, _DDP, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "drnmf_dense_cell_backward_dropout": (_i32, [_vp, _DDP, _vp, _f32] + [_vp] * 14 + [_sz, _vp]),
    "drnmf_dense_cell_forward_dropout_stateful": (_i32, [_vp, _DDP, _vp, _f32] + [_vp] * 7 + [_sz, _vp]),
    "drnmf_dense_cell_backward_stateful": (_i32, [_vp, _DDP, _vp, _f32] + [_vp] * 13 + [_sz, _vp]),
    "drnmf_padded_f": (_i32, [_i32]),
    "drnmf_head_forward": (_i32, [_vp, _i64, _i32, _i32, _vp, _i64, _i32, _vp, _vp, _i32, _vp,
                                  _vp, _vp, _vp, _vp]),
    "drnmf_loss_head_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "drnmf_snmf_cost_head_backward": (_i32, [_vp, _i64, _i32, _i32, _vp, _vp, _i64, _i32, _vp, _vp,
                                             _vp, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _sz,
                                             _vp]),
    "drnmf_loss_head_backward": (_i32, [_vp, _i64, _i32, _i32, _vp, _vp, _i64, _i32, _vp, _vp, _i32,
                                        _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz,
                                        _vp]),
    "drnmf_cell_backward_workspace_bytes": (_sz, [_DP]),
    "drnmf_cell_backward": (_i32, [_vp, _DP, _vp, _vp, _vp, _f32, _f32, _f32, _vp, _vp, _vp, _sz,
                                   _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    "drnmf_cell_backward_stateful": (_i32, [_vp, _DP, _vp, _vp, _vp, _f32, _f32, _f32, _vp, _vp, _vp, _vp, _sz,
                                            _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    "drnmf_cell_backward_ista": (_i32, [_vp, _DP, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _sz, _vp, _sz,
                                        _vp, _vp, _vp, _vp, _vp]),
    "drnmf_cell_backward_ista_stateful": (_i32, [_vp, _DP, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _sz, _vp, _sz,
                                                 _vp, _vp, _vp, _vp, _vp]),
    "drnmf_cell_backward_profile": (_i32, [_vp, _DP, _vp, _vp, _vp, _f32, _f32, _f32, _vp, _vp, _vp,
                                           _sz, _vp, _sz, _vp, _vp, _vp, _vp, _vp,
                                           C.POINTER(C.c_float)]),
    "drnmf_adam_step": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _f32, _f32, _f32, _f32, _f32, _vp]),
    "drnmf_sumsq": (_i32, [_vp, _i64, _vp, _vp, _vp]),
    "drnmf_adam_step_flat": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _f32, _f32, _f32,
                                    _f32, _i32, _f32, _vp, _vp]),
    "drnmf_adam_step_flat_counted": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double,
                                            C.c_double, C.c_double, _f32, _f32, _i32, _f32, _vp, _vp, _vp,
                                            _vp]),
    "drnmf_check_status": (_i32, [_vp]),
    "drnmf_status_take_device": (_i32, [_vp, _vp, _vp]),
    "drnmf_reload_env": (_i32, []),
    "drnmf_set_matrix_mode": (_i32, [_vp, _i32]),
    "drnmf_get_matrix_mode": (_i32, [_vp]),
    "drnmf_persist_admitted": (_i32, [_vp]),
    "drnmf_persist_admit_reason": (C.c_char_p, [_vp]),
    "drnmf_host_report_ring": (_i32, [_vp, C.POINTER(C.POINTER(C.c_float)), C.POINTER(_i32)]),
    "drnmf_ista_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "drnmf_ista_forward": (_i32, [_vp, _i64, _i32, _i32, _i32, _i32, _f32, _f32, _f32, _vp, _vp,
                                  _vp, _vp, _sz, _vp]),
    "drnmf_mu_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "drnmf_mu_forward": (_i32, [_vp, _i64, _i32, _i32, _i32, _f32, _f32, _vp, _vp, _vp, _vp, _vp,
                                _vp, _sz, _vp]),
    "drnmf_snmf_train_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "drnmf_snmf_train_init": (_i32, [_vp, _i64, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "drnmf_snmf_train_step": (_i32, [_vp, _i64, _i32, _i32, _f32, _f32, _vp, _vp, _vp, _i32, _vp,
                                     _vp, _sz, _vp]),
    "drnmf_stft_frames": (_i32, [_i64, _i32, _i32]),
    "drnmf_stft_mag": (_i32, [_vp, _i32, _i64, _i32, _i32, _i32, _vp, _vp, _vp]),
    "drnmf_stft": (_i32, [_vp, _i32, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "drnmf_istft_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "drnmf_istft_masked": (_i32, [_vp, _i32, _i32, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _sz,
                                  _vp]),
    "drnmf_snr": (_i32, [_vp, _i32, _i64, _vp, _vp, _vp, _vp]),
    "drnmf_divide_a_by_aplusb": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp]),
    "drnmf_add": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp]),
    "drnmf_loss_forward_workspace_bytes": (_sz, [_i64]),
    "drnmf_loss_forward": (_i32, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32,
                                  _f32, _vp, _vp, _sz, _vp]),
    "drnmf_wav_int16_workspace_bytes": (_sz, []),
    "drnmf_wav_int16": (_i32, [_vp, _i64, _vp, _vp, _vp, _sz, _vp]),
    "drnmf_sdr_workspace_bytes": (_sz, [_i32, _i64, _i32]),
    "drnmf_sdr_corr": (_i32, [_vp, _i32, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "drnmf_comm_unique_id": (_i32, [_vp, _vp]),
    "drnmf_comm_init": (_i32, [_vp, _vp, _i32, _i32]),
    "drnmf_comm_destroy": (_i32, [_vp]),
    "drnmf_comm_info": (_i32, [_vp, C.POINTER(_i32), C.POINTER(_i32)]),
    "drnmf_allreduce_grads": (_i32, [_vp, _vp, _i64, _vp]),
    "drnmf_broadcast_params": (_i32, [_vp, _vp, _i64, _i32, _vp]),
    "drnmf_sdr_project": (_i32, [_vp, _i32, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
}


class LstmDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "T", "F", "H", "K", "recurrent_activation", "operand_f16")]


_LDP = C.POINTER(LstmDesc)

# name -> (restype, argtypes); mirrors include/drnmf_lstm.h one to one (a table of its own: SIGNATURES is
# drnmf.h's)
LSTM_SIGNATURES = {
    "drnmf_lstm_params_bytes": (_sz, [_LDP]),
    "drnmf_lstm_prepare_params": (_i32, [_vp, _LDP, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "drnmf_lstm_workspace_bytes": (_sz, [_LDP]),
    "drnmf_lstm_forward": (_i32, [_vp, _LDP, _vp, _f32, _vp, _vp, _i32, _vp, _sz, _vp]),
    "drnmf_lstm_forward_stateful": (_i32, [_vp, _LDP, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _sz,
                                           _vp]),
    "drnmf_lstm_head_forward": (_i32, [_vp, _LDP, _vp, _i32, _vp, _vp, _vp]),
    "drnmf_lstm_train_workspace_bytes": (_sz, [_LDP]),
    "drnmf_lstm_train_forward": (_i32, [_vp, _LDP, _vp, _f32, _vp, _vp, _i32, _vp, _sz, _vp]),
    "drnmf_lstm_train_forward_stateful": (_i32, [_vp, _LDP, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp,
                                                 _sz, _vp]),
    "drnmf_lstm_loss_head_backward": (_i32, [_vp, _LDP, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                             _sz, _vp]),
    "drnmf_lstm_backward": (_i32, [_vp, _LDP, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
}

# name -> (restype, argtypes); mirrors include/drnmf_score.h one to one (a table of its own, like LSTM_SIGNATURES)
SCORE_SIGNATURES = {
    "drnmf_stoi_vad_frames": (_i32, [_i64, _i32]),
    "drnmf_stoi_workspace_bytes": (_sz, [_i32, _i64, _i32]),
    "drnmf_stoi": (_i32, [_vp, _i32, _i64, C.POINTER(_i64), _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
}

# name -> (restype, argtypes); mirrors include/drnmf_enhance.h one to one (a table of its own, like the two above)
ENHANCE_SIGNATURES = {
    "drnmf_stft_ragged": (_i32, [_vp, _i32, _i64, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _vp,
                                 _vp]),
    "drnmf_istft_ragged_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    "drnmf_istft_ragged": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i32,
                                  _vp, _sz, _vp]),
    "drnmf_wav_int16_rows_workspace_bytes": (_sz, [_i32]),
    "drnmf_wav_int16_rows": (_i32, [_vp, _i32, _i64, _vp, _vp, _vp, _vp, _sz, _vp]),
}

# name -> (restype, argtypes); mirrors include/drnmf_sdr.h one to one (a table of its own, like the three above)
SDR_SIGNATURES = {
    "drnmf_toeplitz_solve": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "drnmf_sdr_ragged_workspace_bytes": (_sz, [_i32, _i64, _i32]),
    "drnmf_sdr_ragged": (_i32, [_vp, _i32, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
}

# name -> (restype, argtypes); mirrors include/drnmf_dataset.h one to one (a table of its own, like the four above)
DATASET_SIGNATURES = {
    "drnmf_stft_pair_chunks": (_i32, [_vp, _i32, _i64, _i64, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _f32,
                                      _vp, _vp, _vp, _vp, _vp, _vp]),
    "drnmf_stft_pair_frames": (_i32, [_vp, _i32, _i64, _i64, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp,
                                      _vp, _vp, _vp]),
}
TRANSFORMS = {"mag": 0, "logmag": 1}     # DRNMF_TRANSFORM_*

# name -> (restype, argtypes); mirrors include/drnmf_target.h one to one (a table of its own, like the others)
TARGET_SIGNATURES = {
    "drnmf_stft_pair_chunks_target": (_i32, [_vp, _i32, _i64, _i64, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32,
                                             _i32, _f32, _vp, _vp, _vp, _vp, _vp, _vp]),
}
TARGETS = {"mag": 0, "psa": 1, "tpsa": 2}     # DRNMF_TARGET_*

# name -> (restype, argtypes); mirrors include/drnmf_estoi.h one to one (a table of its own, like the others)
ESTOI_SIGNATURES = {
    "drnmf_stoi_ext_workspace_bytes": (_sz, [_i32, _i64, _i32]),
    "drnmf_stoi_ext": (_i32, [_vp, _i32, _i64, C.POINTER(_i64), _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz,
                              _vp]),
}

# name -> (restype, argtypes); mirrors include/drnmf_stream.h one to one (a table of its own, like the five above)
STREAM_SIGNATURES = {
    "drnmf_stream_counts": (_i32, [_i64, _i32, _i32, _i32, _i32, C.POINTER(_i64), C.POINTER(_i64)]),
    "drnmf_stream_state_bytes": (_sz, [_i32, _i32, _i32]),
    "drnmf_stream_reset": (_i32, [_vp, _i32, _i32, _i32, _vp, _sz, _vp]),
    "drnmf_stream_forward": (_i32, [_vp, _i32, _i64, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                    _sz, _vp]),
    "drnmf_stream_inverse": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _i64, _vp,
                                    _sz, _vp]),
}

# name -> (restype, argtypes); mirrors include/drnmf_snmf.h one to one (a table of its own, like the six above)
SNMF_SIGNATURES = {
    "drnmf_snmf_mask_admitted": (_i32, [_i32, _i32, _f32]),
    "drnmf_snmf_mask_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    "drnmf_snmf_mask_forward": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _f32, _f32, _f32, _f32, _i32, _vp, _vp, _vp,
                                       _vp, _i32, _vp, _sz, _vp]),
}
SNMF_PATHS = {"auto": 0, "gemm": 1, "tile": 2}     # DRNMF_SNMF_PATH_*
SNMF_TILE_AUTO_MAX_ROWS = 8192                     # csrc/snmf_mask.hip TILE_AUTO_MAX_ROWS: 'auto' takes the tile kernel up to here

# name -> (restype, argtypes); mirrors include/drnmf_snmf_f16.h one to one (a table of its own, like the seven above)
SNMF_F16_SIGNATURES = {
    "drnmf_snmf_f16_admitted": (_i32, [_i32, _i32, _f32]),
    "drnmf_snmf_f16_dict_bytes": (_sz, [_i32, _i32]),
    "drnmf_snmf_f16_pack_dict": (_i32, [_vp, _i32, _i32, _vp, _vp, _sz, _vp]),
    "drnmf_snmf_f16_forward": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _f32, _f32, _f32, _i32, _vp, _vp, _vp, _vp,
                                      _vp, _vp]),
}
SNMF_F16_MAX_N = 512                               # csrc/snmf_f16.hip MAX_N

# name -> (restype, argtypes); mirrors include/drnmf_snmf_adapt.h one to one (a table of its own, like those above)
SNMF_ADAPT_SIGNATURES = {
    "drnmf_snmf_adapt_admitted": (_i32, [_i32, _i32, _f32]),
    "drnmf_snmf_adapt_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32, _i32]),
    "drnmf_snmf_adapt_forward": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _f32, _f32, _i32, _vp, _vp, _vp,
                                        _vp, _vp, _vp, _vp, _sz, _vp]),
}
SNMF_ADAPT_MAX_N = 512                             # csrc/snmf_adapt.hip MAX_N

# name -> (restype, argtypes); mirrors include/drnmf_snmf_kl.h one to one (a table of its own, like those above)
SNMF_KL_SIGNATURES = {
    "drnmf_snmf_kl_admitted": (_i32, [_i32, _i32]),
    "drnmf_snmf_kl_workspace_bytes": (_sz, []),
    "drnmf_snmf_kl_auto_max_rows": (_i64, []),
    "drnmf_snmf_kl_forward": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _f32, _f32, _f32, _i32, _vp, _vp, _vp, _f32,
                                     _vp, _vp, _sz, _vp]),
}
SNMF_KL_MAX_N = 512                                # csrc/snmf_kl.hip KL_MAX_N
SNMF_KL_AUTO_MAX_ROWS = 8192                        # csrc/snmf_kl.hip KL_AUTO_MAX_ROWS: a beta = 1 model's 'auto' takes the KL kernel up to here

# name -> (restype, argtypes); mirrors include/drnmf_snmf_online.h one to one (a table of its own, like those above)
SNMF_ONLINE_SIGNATURES = {
    "drnmf_snmf_online_admitted": (_i32, [_i32, _i32, _f32, _i32]),
    "drnmf_snmf_online_state_bytes": (_sz, [_i32, _i32, _i32, _i32, _i32]),
    "drnmf_snmf_online_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "drnmf_snmf_online_reset": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _sz, _vp]),
    "drnmf_snmf_online_forward": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _f32, _f32, _f32,
                                         _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    "drnmf_snmf_online_read": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
}
SNMF_ONLINE_MAX_N = 512                            # csrc/snmf_online.hip: snmf_tile.h's MAX_N
SNMF_ONLINE_BLOCKS = tuple(range(16, 257, 16))     # csrc/snmf_online.hip MIN_BLOCK .. MAX_BLOCK

# name -> (restype, argtypes); mirrors include/drnmf_mix.h one to one (a table of its own, like those above)
MIX_SIGNATURES = {
    "drnmf_mix_workspace_bytes": (_sz, [_i32, _i64]),
    "drnmf_mix_energy": (_i32, [_vp, _i32, _i64, _vp, _i32, _vp, _vp, _vp, _sz, _vp]),
    "drnmf_mix_forward": (_i32, [_vp, _i32, _i64, _vp, _i32, _vp, _i32, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp,
                                 _vp, _vp, _sz, _vp]),
}
MIX_BLOCK = 4096                                   # DRNMF_MIX_BLOCK

# name -> (restype, argtypes); mirrors include/drnmf_waveloss.h one to one (a table of its own, like those above)
WAVELOSS_SIGNATURES = {
    "drnmf_istft_ragged_vjp": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp,
                                      _i64, _vp]),
    "drnmf_wave_loss_workspace_bytes": (_sz, [_i32, _i64]),
    "drnmf_wave_loss": (_i32, [_vp, _i32, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "drnmf_head_backward_cot": (_i32, [_vp, _i64, _i32, _i32, _vp, _i64, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _i64,
                                       _vp, _vp, _vp, _vp, _sz, _vp]),
    "drnmf_lstm_head_backward_cot": (_i32, [_vp, _LDP, _vp, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
}
WAVE_LOSSES = {"wave_mse": 0, "si_sdr": 1}     # DRNMF_WAVE_LOSS_*
WAVE_LOSS_BLOCK = 4096                         # DRNMF_WAVE_LOSS_BLOCK

# name -> (restype, argtypes); mirrors include/drnmf_reverb.h one to one (a table of its own, like those above)
REVERB_SIGNATURES = {
    "drnmf_reverb_forward": (_i32, [_vp, _i32, _i64, _vp, _i32, _vp, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}
REVERB_TILE = 2048                                 # DRNMF_REVERB_TILE
REVERB_CHUNK = 1024                                # DRNMF_REVERB_CHUNK

# name -> (restype, argtypes); mirrors include/drnmf_stoi_loss.h one to one (a table of its own, like those above)
STOI_LOSS_SIGNATURES = {
    "drnmf_stoi_loss_workspace_bytes": (_sz, [_i32, _i64, _i32]),
    "drnmf_stoi_loss": (_i32, [_vp, _i32, _i64, C.POINTER(_i64), _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _sz,
                               _vp]),
}
STOI_LOSS_STOI = 0                                 # DRNMF_STOI_LOSS_STOI

# name -> (restype, argtypes); mirrors include/drnmf_resample.h one to one (a table of its own, like those above)
RESAMPLE_SIGNATURES = {
    "drnmf_resample_rate": (_i32, [_i64, _i64, C.POINTER(_i32), C.POINTER(_i32)]),
    "drnmf_resample_taps_len": (_i64, [_i32, _i32, _i32]),
    "drnmf_resample_out_len": (_i64, [_i64, _i32, _i32]),
    "drnmf_resample_tile": (_i32, [_i32, _i32, _i32]),
    "drnmf_resample_taps": (_i32, [_vp, _i32, _i32, _i32, C.c_double, _vp, _vp]),
    "drnmf_resample_forward": (_i32, [_vp, _i32, _i64, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _i64, _vp, _vp]),
    "drnmf_resample_chunk": (_i32, [_vp, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _i64,
                                    _vp, _vp]),
    "drnmf_resample_carry": (_i32, [_vp, _i32, _i32, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
}
RESAMPLE_MAX_PQ = 640                              # DRNMF_RESAMPLE_MAX_PQ
RESAMPLE_NZ, RESAMPLE_BETA = 10, 5.0               # DRNMF_RESAMPLE_NZ, DRNMF_RESAMPLE_BETA
RESAMPLE_TILE = 2048                               # DRNMF_RESAMPLE_TILE

# every table above, one per header: lib() binds them all (a new header adds its table's name here)
SIGNATURE_TABLES = (SIGNATURES, LSTM_SIGNATURES, SCORE_SIGNATURES, ENHANCE_SIGNATURES, SDR_SIGNATURES,
                    DATASET_SIGNATURES, STREAM_SIGNATURES, SNMF_SIGNATURES, SNMF_F16_SIGNATURES, TARGET_SIGNATURES,
                    ESTOI_SIGNATURES, SNMF_ADAPT_SIGNATURES, SNMF_KL_SIGNATURES, SNMF_ONLINE_SIGNATURES,
                    MIX_SIGNATURES, WAVELOSS_SIGNATURES, REVERB_SIGNATURES, STOI_LOSS_SIGNATURES,
                    RESAMPLE_SIGNATURES)

_lib = None
_handles = {}


class DrnmfError(RuntimeError):
    pass


def lib():
    """Load libdrnmf.so (once).  Raises ImportError with the build command if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "libdrnmf.so not found at %s -- build it with `python dr-nmf_amd/build.py` "
                "(or __graft_entry__.build()).  There is no CPU fallback." % LIB_PATH)
        # torch first: it ships its own libamdhip64, and the process must hold ONE HIP runtime.
        # Loaded before torch, libdrnmf.so would pull in /opt/rocm's copy and the second runtime
        # to initialise reports "no ROCm-capable device".
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for table in SIGNATURE_TABLES:
            for name, (res, args) in table.items():
                fn = getattr(L, name)
                fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def handle(device=0):
    """One library handle per device per process."""
    if device not in _handles:
        L = lib()
        h = _vp()
        rc = L.drnmf_create(C.byref(h), int(device))
        if rc != OK:
            raise DrnmfError("drnmf_create(device=%d) failed (%d): %s" %
                             (device, rc, L.drnmf_last_error(None).decode()))
        _handles[device] = h
    return _handles[device]


def check(rc, h, what):
    if rc != OK:
        msg = lib().drnmf_last_error(h).decode(errors="replace")
        exc = ValueError if rc in (-1, -2, -4) else DrnmfError
        raise exc("%s failed (%d): %s" % (what, rc, msg))


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else _vp(t.data_ptr())
