"""ctypes binding of libvr_mi355.so (include/vr_mi355.h).  Fails loudly when the library or a GPU
is missing -- there is no CPU or PyTorch fallback in this package."""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (VR_LIB_PATH: another build of the same library, for A / B runs of two builds in one gpurun call)
LIB_PATH = os.environ.get('VR_LIB_PATH') or os.path.join(_HERE, 'libvr_mi355.so')

c_f32p = ctypes.c_void_p
VR_CREATE_COMPLEX = 1         # include/vr_mi355.h
VR_LOSS_L1, VR_LOSS_MAG_L1_WAVE_SDR, VR_LOSS_MAG_L1_WAVE_WSDR = 0, 1, 3          # (kind 2 is not a loss: the header says why)
LOSS_KINDS = {'l1': VR_LOSS_L1, 'mag_l1_wave_sdr': VR_LOSS_MAG_L1_WAVE_SDR, 'mag_l1_wave_wsdr': VR_LOSS_MAG_L1_WAVE_WSDR}
VR_STREAM_TTA, VR_STREAM_MEASURE, VR_STREAM_POSTPROCESS, VR_STREAM_PCM16_OUT = 1, 2, 4, 8
VR_PCM_S16, VR_PCM_S24, VR_PCM_S32, VR_PCM_F32 = 1, 2, 3, 4          # enum vr_pcm_format
VR_PSEUDO_SPEC, VR_PSEUDO_ROWS = 0, 1          # enum vr_pseudo_layout
PSEUDO_LAYOUTS = {'spec': VR_PSEUDO_SPEC, 'rows': VR_PSEUDO_ROWS}
PCM_SAMPLE_BYTES = {VR_PCM_S16: 2, VR_PCM_S24: 3, VR_PCM_S32: 4, VR_PCM_F32: 4}
c_i64p = ctypes.POINTER(ctypes.c_int64)

_SIGNATURES = {
    'vr_last_error': (ctypes.c_char_p, []),
    'vr_create': (ctypes.c_int, [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_void_p)]),
    'vr_create_ex': (ctypes.c_int, [ctypes.c_int] * 6 + [ctypes.POINTER(ctypes.c_void_p)]),
    'vr_destroy': (ctypes.c_int, [ctypes.c_void_p]),
    'vr_num_params': (ctypes.c_int, [ctypes.c_void_p]),
    'vr_param_info': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, c_i64p,
                                     ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                     ctypes.POINTER(ctypes.c_int)]),
    'vr_set_param': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, c_i64p, ctypes.c_int]),
    'vr_get_param': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int64]),
    'vr_set_mode': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    'vr_forward': (ctypes.c_int, [ctypes.c_void_p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                  c_f32p, ctypes.c_int]),
    'vr_stft': (ctypes.c_int, [ctypes.c_void_p, c_f32p, ctypes.c_int, ctypes.c_int64, c_f32p, ctypes.c_int]),
    'vr_istft': (ctypes.c_int, [ctypes.c_void_p, c_f32p, ctypes.c_int, ctypes.c_int, c_f32p, ctypes.c_int]),
    'vr_separate': (ctypes.c_int, [ctypes.c_void_p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                   ctypes.c_int, c_f32p, c_f32p, ctypes.c_int]),
    'vr_separate_wave': (ctypes.c_int, [ctypes.c_void_p, c_f32p, ctypes.c_int, ctypes.c_int64, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_int, c_f32p, c_f32p, ctypes.c_int]),
    'vr_separate_many': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int,
                                        ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]),
    'vr_separate_wave_many': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, c_i64p,
                                             ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                             ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]),
    'vr_evaluate_wave_many': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                             ctypes.c_int, c_i64p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                             ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                             ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]),
    'vr_evaluate_wave': (ctypes.c_int, [ctypes.c_void_p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, c_f32p, c_f32p, ctypes.c_int]),
    'vr_evaluate_plan': (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, ctypes.c_int64, c_i64p, c_i64p]),
    'vr_pseudo_many': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                      ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]),
    'vr_pseudo_wave_many': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                           ctypes.c_int, c_i64p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]),
    'vr_pseudo': (ctypes.c_int, [ctypes.c_void_p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                 ctypes.c_int, c_f32p, ctypes.c_int]),
    'vr_pseudo_wave': (ctypes.c_int, [ctypes.c_void_p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_int, c_f32p, ctypes.c_int]),
    'vr_pcm_available': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]),
    'vr_stft_pcm': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, c_f32p, ctypes.c_int]),
    'vr_istft_pcm16': (ctypes.c_int, [ctypes.c_void_p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]),
    'vr_separate_pcm': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64] + [ctypes.c_int] * 5
                        + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    'vr_separate_pcm_many': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, c_i64p,
                                            ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]),
    'vr_separate_wave_many_img': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, c_i64p,
                                                 ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                                 ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                                 ctypes.POINTER(ctypes.c_void_p), c_f32p]),
    'vr_separate_pcm_many_img': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, c_i64p,
                                                ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int,
                                                ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.c_int,
                                                ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), c_f32p]),
    'vr_spec_image_many': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int,
                                          c_f32p]),
    'vr_spec_image': (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_void_p, ctypes.c_int, c_f32p]),
    'vr_pcm_convert_host': (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, c_f32p]),
    'vr_pcm16_from_float_host': (ctypes.c_int, [c_f32p, ctypes.c_int64, ctypes.c_void_p]),
    'vr_stream_open': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                      ctypes.POINTER(ctypes.c_void_p)]),
    'vr_stream_push': (ctypes.c_int, [ctypes.c_void_p, c_f32p, ctypes.c_int, ctypes.c_int64, c_f32p, c_f32p, ctypes.c_int,
                                      ctypes.c_int64, c_i64p]),
    'vr_stream_flush': (ctypes.c_int, [ctypes.c_void_p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int64, c_i64p]),
    'vr_stream_push_many': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, c_i64p,
                                           ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                           ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, c_i64p, c_i64p]),
    'vr_stream_push_pcm': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, c_f32p, c_f32p,
                                          ctypes.c_int, ctypes.c_int64, c_i64p]),
    'vr_stream_push_many_pcm': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, c_i64p,
                                               ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                               ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.c_int,
                                               c_i64p, c_i64p]),
    'vr_stream_coef': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]),
    'vr_stream_info': (ctypes.c_int, [ctypes.c_void_p, c_i64p, c_i64p, c_i64p]),
    'vr_stream_close': (ctypes.c_int, [ctypes.c_void_p]),
    'vr_stream_plan': (ctypes.c_int, [ctypes.c_int] * 5 + [ctypes.c_int64, ctypes.c_int, c_i64p, c_i64p, c_i64p]),
    'vr_stream_plan_ex': (ctypes.c_int, [ctypes.c_int] * 5 + [ctypes.c_int64, ctypes.c_int, c_i64p, c_i64p, c_i64p]),
    'vr_debug_stream_post_weight': (ctypes.c_int, [c_f32p, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int, c_f32p,
                                                   ctypes.POINTER(ctypes.c_int)]),
    'vr_arena_bytes': (ctypes.c_int, [ctypes.c_void_p, c_i64p, c_i64p]),
    'vr_train_step': (ctypes.c_int, [ctypes.c_void_p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, ctypes.POINTER(ctypes.c_float), c_f32p, ctypes.c_int]),
    'vr_forward_train': (ctypes.c_int, [ctypes.c_void_p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_f32p, ctypes.c_int]),
    'vr_backward': (ctypes.c_int, [ctypes.c_void_p, c_f32p, ctypes.c_int]),
    'vr_param_arena': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64)]),
    'vr_adam_step': (ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_double] * 5),
    'vr_zero_grad': (ctypes.c_int, [ctypes.c_void_p]),
    'vr_get_adam_state': (ctypes.c_int, [ctypes.c_void_p, c_f32p, c_f32p, ctypes.c_int64, c_i64p]),
    'vr_set_adam_state': (ctypes.c_int, [ctypes.c_void_p, c_f32p, c_f32p, ctypes.c_int64, ctypes.c_int64]),
    'vr_graph_generation': (ctypes.c_int, [ctypes.c_void_p, c_i64p, ctypes.POINTER(ctypes.c_int)]),
    'vr_get_grad': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, c_f32p, ctypes.c_int64]),
    'vr_set_dropout': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, c_f32p, ctypes.c_int]),
    'vr_grad_arena': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64)]),
    'vr_set_option': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]),
    'vr_set_loss': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_double]),
    'vr_get_loss': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)]),
    'vr_loss_terms': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    'vr_loss_terms_wsdr': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                          ctypes.POINTER(ctypes.c_double)]),
    'vr_augment_batch': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    'vr_augment_batch_complex': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    'vr_dataset_create': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    'vr_dataset_create_waves': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    'vr_dataset_add_waves': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
                                            ctypes.POINTER(ctypes.c_int)]),
    'vr_dataset_add_pcm': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    'vr_dataset_destroy': (ctypes.c_int, [ctypes.c_void_p]),
    'vr_pipeline_buffer': (ctypes.c_int, [ctypes.c_void_p, c_i64p, ctypes.c_int]),
    'vr_dataset_add': (ctypes.c_int, [ctypes.c_void_p, c_f32p, c_f32p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int)]),
    'vr_dataset_info': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), c_i64p]),
    'vr_dataset_rows': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_i64p]),
    'vr_dataset_batch': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_f32p, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    'vr_dataset_batch_complex': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_f32p, ctypes.c_int,
                                                ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    # (the _ex entry points: a table of vr_aug_ex in place of vr_aug, dataset._AugEx)
    'vr_augment_batch_ex': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    'vr_augment_batch_complex_ex': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                   ctypes.c_void_p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    'vr_dataset_batch_ex': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_f32p, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    'vr_dataset_batch_complex_ex': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_f32p, ctypes.c_int,
                                                   ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    'vr_dataset_peak': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float),
                                       ctypes.POINTER(ctypes.c_int), c_i64p]),
    'vr_dataset_windows': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_int]),
    'vr_dataset_windows_complex': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    'vr_validate_step': (ctypes.c_int, [ctypes.c_void_p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.POINTER(ctypes.c_float)]),
    'vr_comm_unique_id': (ctypes.c_int, [ctypes.c_void_p]),
    'vr_comm_init': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    'vr_comm_destroy': (ctypes.c_int, [ctypes.c_void_p]),
    'vr_allreduce_grads': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    'vr_broadcast_params': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    'vr_debug_kernel': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, c_i64p, ctypes.c_int, ctypes.POINTER(ctypes.c_float),
                                       ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int,
                                       ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]),
    'vr_resample': (ctypes.c_int, [ctypes.c_int, c_f32p, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, c_f32p, ctypes.c_int64]),
    'vr_xcorr_argmax': (ctypes.c_int, [ctypes.c_int, c_f32p, ctypes.c_int64, c_f32p, ctypes.c_int64, c_i64p]),
    'vr_resample_ratio': (ctypes.c_int, [ctypes.c_int, c_f32p, ctypes.c_int, ctypes.c_int64, ctypes.c_double, c_f32p, ctypes.c_int64]),
    'vr_pitch_plan': (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.POINTER(ctypes.c_int),
                                     ctypes.POINTER(ctypes.c_int), c_i64p, c_i64p]),
    'vr_phase_vocoder': (ctypes.c_int, [ctypes.c_void_p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, c_f32p, ctypes.c_int]),
    'vr_istft_length': (ctypes.c_int, [ctypes.c_void_p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int64, c_f32p, ctypes.c_int]),
    'vr_pitch_shift_many': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int, c_i64p,
                                           ctypes.c_double, ctypes.c_double, ctypes.c_int64, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]),
    'vr_pitch_pair_many': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                          ctypes.c_int, c_i64p, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int,
                                          ctypes.c_int64, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                          ctypes.c_int]),
    'vr_pair_window_plan': (ctypes.c_int, [ctypes.c_int64] * 5 + [ctypes.c_void_p]),
    'vr_align_pair_many': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                          ctypes.c_int, c_i64p, c_i64p, ctypes.c_int, ctypes.c_void_p]),
    'vr_pair_rows_many': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                         ctypes.c_int, c_i64p, c_i64p, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_void_p),
                                         ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.POINTER(ctypes.c_float)]),
    'vr_resampler_open': (ctypes.c_int, [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_void_p)]),
    'vr_resampler_push': (ctypes.c_int, [ctypes.c_void_p, c_f32p, ctypes.c_int, ctypes.c_int64, c_f32p, ctypes.c_int, ctypes.c_int64, c_i64p]),
    'vr_resampler_flush': (ctypes.c_int, [ctypes.c_void_p, c_f32p, ctypes.c_int, ctypes.c_int64, c_i64p]),
    'vr_resampler_push_many': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, c_i64p,
                                              ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, c_i64p, c_i64p]),
    'vr_resampler_push_pcm': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, c_f32p,
                                             ctypes.c_int, ctypes.c_int64, c_i64p]),
    'vr_resampler_push_many_pcm': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.c_int,
                                                  c_i64p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                                  ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, c_i64p, c_i64p]),
    'vr_resampler_info': (ctypes.c_int, [ctypes.c_void_p, c_i64p, c_i64p]),
    'vr_resampler_close': (ctypes.c_int, [ctypes.c_void_p]),
    'vr_resampler_plan': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int, c_i64p]),
    'vr_profile_begin': (ctypes.c_int, [ctypes.c_void_p]),
    'vr_profile_end': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double),
                                      ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int),
                                      ctypes.POINTER(ctypes.c_double)]),
    'vr_profile_report': (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64]),
    'vr_debug_conv2d': (ctypes.c_int, [ctypes.c_void_p, c_f32p] + [ctypes.c_int] * 4 + [c_f32p] + [ctypes.c_int] * 6
                        + [c_f32p, ctypes.c_float, c_f32p, c_f32p, c_f32p]),
    'vr_debug_conv2d_backward': (ctypes.c_int, [ctypes.c_void_p, c_f32p] + [ctypes.c_int] * 4 + [c_f32p]
                                 + [ctypes.c_int] * 6 + [c_f32p, ctypes.c_float, c_f32p, c_f32p, c_f32p]),
    'vr_debug_merge_artifacts_weight': (ctypes.c_int, [c_f32p, ctypes.c_int, ctypes.c_float, ctypes.c_int, ctypes.c_int,
                                                       c_f32p]),
    'vr_debug_record_taps': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    'vr_debug_get_tap': (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_char_p, c_f32p, ctypes.c_int64, c_i64p]),
}

_lib = None


def lib():
    """Load libvr_mi355.so once; raise if it has not been built (python __graft_entry__.py)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError('%s is missing: build it with `python __graft_entry__.py` '
                               '(there is no CPU fallback)' % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError here = header / library mismatch
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def exported_symbols():
    return sorted(_SIGNATURES)


class VRError(RuntimeError):
    pass


class VRArgumentError(VRError, ValueError):
    """VR_ERR_BAD_ARGUMENT of the sample-format entry points (vr_*_pcm*, VR_STREAM_PCM16_OUT): the ValueError every other entry point
    raises for it, and a VRError like every other refusal of the library."""


class VRUnsupported(VRError):
    """VR_ERR_UNSUPPORTED: the handle has no kernel for the request (vr_pair_rows_many at hop_length != n_fft / 2); the caller's other
    route applies."""


def check(rc, arg_error=ValueError):
    """Map vr_status to the exception the reference would raise at the same spot.  arg_error: what VR_ERR_BAD_ARGUMENT raises (the
    sample-format entry points pass VRArgumentError)."""
    if rc >= 0:
        return rc
    msg = lib().vr_last_error().decode('utf-8', 'replace')
    if rc == -5:
        raise ValueError(msg)              # spec_utils.crop_center ValueError (lib/spec_utils.py:15)
    if rc == -6:
        raise AssertionError(msg)          # assert mask.size()[3] > 0 (lib/nets.py:129,139)
    if rc == -7:
        raise IndexError(msg)              # merge_artifacts on a mask with no frame above the threshold
    if rc == -2:
        raise arg_error(msg)
    if rc == -8:
        raise VRError('libvr_mi355 RCCL error: %s' % msg)
    if rc == -9:
        raise VRUnsupported(msg)
    raise VRError('libvr_mi355 error %d: %s' % (rc, msg))


def debug_kernel(handle, name, dims, fparams, inputs, outputs):
    """vr_debug_kernel: `inputs` / `outputs` are lists of C-contiguous float32 numpy arrays (or None)."""
    dims_a = (ctypes.c_int64 * max(len(dims), 1))(*[int(d) for d in dims])
    fp_a = (ctypes.c_float * max(len(fparams), 1))(*[float(f) for f in fparams])
    ins = (ctypes.c_void_p * max(len(inputs), 1))(*[a.ctypes.data if a is not None else None for a in inputs])
    outs = (ctypes.c_void_p * max(len(outputs), 1))(*[a.ctypes.data if a is not None else None for a in outputs])
    for a in list(inputs) + list(outputs):
        assert a is None or (a.flags['C_CONTIGUOUS'] and a.dtype == np.float32)
    check(lib().vr_debug_kernel(handle.h, name.encode(), dims_a, len(dims), fp_a, len(fparams), ins, len(inputs), outs,
                                len(outputs)))


def np_ptr(a):
    assert a.flags['C_CONTIGUOUS']
    return ctypes.c_void_p(a.ctypes.data)


def ptr_table(addresses):
    """A host table of data pointers (vr_separate_many / vr_separate_wave_many) from integer addresses."""
    return (ctypes.c_void_p * len(addresses))(*[int(a) for a in addresses])


def stream_plan(n_fft, hop, cropsize, offset, tta, samples_in, flushed):
    """vr_stream_plan (host only): -> (frames_ready, (crops_ready pass 0, pass 1), samples_out)."""
    fr, out = ctypes.c_int64(), ctypes.c_int64()
    crops = (ctypes.c_int64 * 2)()
    check(lib().vr_stream_plan(int(n_fft), int(hop), int(cropsize), int(offset), 1 if tta else 0, int(samples_in), 1 if flushed else 0,
                               ctypes.byref(fr), crops, ctypes.byref(out)))
    return int(fr.value), (int(crops[0]), int(crops[1])), int(out.value)


def stream_plan_ex(n_fft, hop, cropsize, offset, flags, samples_in, flushed):
    """vr_stream_plan_ex (host only): stream_plan with the flags of vr_stream_open (VR_STREAM_TTA, VR_STREAM_POSTPROCESS) in place of tta."""
    fr, out = ctypes.c_int64(), ctypes.c_int64()
    crops = (ctypes.c_int64 * 2)()
    check(lib().vr_stream_plan_ex(int(n_fft), int(hop), int(cropsize), int(offset), int(flags), int(samples_in), 1 if flushed else 0,
                                  ctypes.byref(fr), crops, ctypes.byref(out)))
    return int(fr.value), (int(crops[0]), int(crops[1])), int(out.value)


def stream_post_weight(frame_min, cuts=()):
    """vr_debug_stream_post_weight (host only): the merge_artifacts weights of the per-frame mask minima `frame_min` from the incremental
    form a postprocess stream runs, taken in steps that end in front of the frames `cuts`.  -> (weight [T], frames final after each
    step and after the flush [len(cuts) + 1])."""
    import numpy as np
    f = np.ascontiguousarray(frame_min, dtype=np.float32)
    c = (ctypes.c_int * max(len(cuts), 1))(*[int(x) for x in cuts])
    w = np.empty(f.size, np.float32)
    fin = (ctypes.c_int * (len(cuts) + 1))()
    check(lib().vr_debug_stream_post_weight(np_ptr(f), int(f.size), c, len(cuts), np_ptr(w), fin))
    return w, np.array(list(fin), dtype=np.int64)


STREAM_POST_DELAY = 161      # frames a postprocess stream's output lags its masks: 3 * fade_size + min_range + 1


def evaluate_plan(hop, L, window):
    """vr_evaluate_plan (host only): -> (samples, n_windows) of a song of L samples scored in windows of `window` samples."""
    samples, windows = ctypes.c_int64(), ctypes.c_int64()
    check(lib().vr_evaluate_plan(int(hop), int(L), int(window), ctypes.byref(samples), ctypes.byref(windows)))
    return int(samples.value), int(windows.value)


def resampler_plan(sr_in, sr_out, samples_in, flushed):
    """vr_resampler_plan (host only): output samples per channel that are final after samples_in input samples (flushed: in all)."""
    out = ctypes.c_int64()
    check(lib().vr_resampler_plan(int(sr_in), int(sr_out), int(samples_in), 1 if flushed else 0, ctypes.byref(out)))
    return int(out.value)


def pitch_plan(L, n_fft, hop, rate, ratio):
    """vr_pitch_plan (host only): -> (T, T_stretch, n_stretch, n_resampled) of one shift of a signal of L samples."""
    T, Ts = ctypes.c_int(), ctypes.c_int()
    ns, nr = ctypes.c_int64(), ctypes.c_int64()
    check(lib().vr_pitch_plan(int(L), int(n_fft), int(hop), float(rate), float(ratio), ctypes.byref(T), ctypes.byref(Ts), ctypes.byref(ns),
                              ctypes.byref(nr)))
    return int(T.value), int(Ts.value), int(ns.value), int(nr.value)


class PairWindow(ctypes.Structure):         # include/vr_mi355.h: vr_pair_window
    _fields_ = [(k, ctypes.c_int64) for k in ('a_start', 'a_end', 'b_start', 'b_end', 'lag', 'a_off', 'b_off', 'n')]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def pair_window_plan(a_start, a_end, b_start, b_end, lag):
    """vr_pair_window_plan (host only): the common window of a pair from its two trimmed ranges and the lag -> PairWindow; ValueError
    when it is empty."""
    w = PairWindow()
    check(lib().vr_pair_window_plan(int(a_start), int(a_end), int(b_start), int(b_end), int(lag), ctypes.byref(w)))
    return w


class Crop(ctypes.Structure):               # include/vr_mi355.h: vr_crop
    _fields_ = [('song', ctypes.c_int), ('mix_song', ctypes.c_int), ('start', ctypes.c_int64), ('mix_start', ctypes.c_int64)]


class Window(ctypes.Structure):             # include/vr_mi355.h: vr_window
    _fields_ = [('song', ctypes.c_int), ('reserved', ctypes.c_int), ('start', ctypes.c_int64), ('scale', ctypes.c_float)]


def _wave_pair(mix, inst):
    """-> (pointer, pointer, n, on_device) of two aligned float32 [2, n] waves, numpy or cuda"""
    if tuple(mix.shape) != tuple(inst.shape) or len(mix.shape) != 2 or mix.shape[0] != 2:
        raise ValueError('a pair of aligned waves is two [2, n] arrays of one n, found %s and %s' % (tuple(mix.shape), tuple(inst.shape)))
    if isinstance(mix, np.ndarray) != isinstance(inst, np.ndarray):
        raise ValueError('both waves on the host or both on the device')
    if isinstance(mix, np.ndarray):
        for w in (mix, inst):
            if w.dtype != np.float32 or not w.flags['C_CONTIGUOUS']:
                raise ValueError('a host wave must be a C-contiguous float32 array')
        return np_ptr(mix), np_ptr(inst), int(mix.shape[1]), 0
    import torch
    for w in (mix, inst):
        if not w.is_cuda or w.dtype != torch.float32 or not w.is_contiguous():
            raise ValueError('a device wave must be a contiguous float32 cuda tensor')
    return ctypes.c_void_p(mix.data_ptr()), ctypes.c_void_p(inst.data_ptr()), int(mix.shape[1]), 1


class Dataset:
    """Owns one vr_dataset: songs resident on one GPU, independent of any Handle."""

    def __init__(self, device, bins):
        self._d = ctypes.c_void_p()
        check(lib().vr_dataset_create(int(device), int(bins), ctypes.byref(self._d)))
        self.device, self.bins = int(device), int(bins)
        self.n_fft = self.hop_length = None

    @classmethod
    def waves(cls, device, n_fft, hop_length):
        """A WAVE store (vr_dataset_create_waves): songs are kept as their two aligned waves, and batches, windows and peaks form the
        STFT rows they need on the device.  hop_length != n_fft / 2 or an n_fft the frame-tiled STFT does not take: VRUnsupported,
        raised without a device."""
        self = cls.__new__(cls)
        self._d = ctypes.c_void_p()
        check(lib().vr_dataset_create_waves(int(device), int(n_fft), int(hop_length), ctypes.byref(self._d)))
        self.device, self.bins = int(device), int(n_fft) // 2 + 1
        self.n_fft, self.hop_length = int(n_fft), int(hop_length)
        return self

    def close(self):
        if getattr(self, '_d', None) and self._d.value:
            lib().vr_dataset_destroy(self._d)
            self._d = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def d(self):
        if not self._d.value:
            raise VRError('dataset is closed')
        return self._d

    def add(self, X, y):
        """One song: X, y complex64 [rows, 2, bins], C-contiguous (a np.memmap of the cache file will do) -> its index."""
        song = ctypes.c_int()
        check(lib().vr_dataset_add(self.d, np_ptr(X), np_ptr(y), int(X.shape[0]), ctypes.byref(song)))
        return int(song.value)

    def add_waves(self, mix, inst):
        """One song of a wave store: mix, inst aligned float32 [2, n], both C-contiguous numpy arrays or both cuda tensors -> its index."""
        pm, pi, n, on_dev = _wave_pair(mix, inst)
        song = ctypes.c_int()
        check(lib().vr_dataset_add_waves(self.d, pm, pi, on_dev, n, ctypes.byref(song)))
        return int(song.value)

    def add_pcm(self, mix, inst):
        """One song of a wave store as the files' sample bytes: mix, inst audio.RawPcm of equal frames (`bytes` a uint8 numpy array or
        cuda tensor, both on the same side); the bytes are stored as they are -> its index."""
        if int(mix.frames) != int(inst.frames):
            raise ValueError('add_pcm: %d and %d frames, a pair has as many of both' % (mix.frames, inst.frames))
        ptrs, sides = [], []
        for r in (mix, inst):
            if r.fmt not in PCM_SAMPLE_BYTES:
                raise ValueError('add_pcm: unknown sample format %d' % r.fmt)
            need = r.frames * r.channels * PCM_SAMPLE_BYTES[r.fmt]
            b = r.bytes
            if isinstance(b, np.ndarray):
                if b.dtype != np.uint8 or not b.flags['C_CONTIGUOUS'] or b.size < need:
                    raise ValueError('add_pcm: bytes must be a C-contiguous uint8 array of at least %d bytes' % need)
                ptrs.append(ctypes.c_void_p(b.ctypes.data))
                sides.append(0)
            else:
                if not b.is_cuda or not b.is_contiguous() or b.element_size() != 1 or b.numel() < need:
                    raise ValueError('add_pcm: bytes must be a contiguous uint8 cuda tensor of at least %d bytes' % need)
                ptrs.append(ctypes.c_void_p(b.data_ptr()))
                sides.append(1)
        if sides[0] != sides[1]:
            raise ValueError('add_pcm: both waves on the host or both on the device')
        song = ctypes.c_int()
        check(lib().vr_dataset_add_pcm(self.d, ptrs[0], ptrs[1], sides[0], int(mix.frames), mix.channels, inst.channels, mix.fmt, inst.fmt,
                                       ctypes.byref(song)))
        return int(song.value)

    def info(self):
        n, b = ctypes.c_int(), ctypes.c_int64()
        check(lib().vr_dataset_info(self.d, ctypes.byref(n), ctypes.byref(b)))
        return int(n.value), int(b.value)

    def rows(self, song):
        r = ctypes.c_int64()
        check(lib().vr_dataset_rows(self.d, int(song), ctypes.byref(r)))
        return int(r.value)

    def peak(self, song, where=False):
        """np.max([np.abs(X).max(), np.abs(y).max()]) of one song, taken on the device from its resident rows -> np.float32.
        where=True: -> (peak, complex64 element that attains it, slab (0 = X, 1 = y), flat complex index in the slab)."""
        p, at = ctypes.c_float(), (ctypes.c_float * 2)()
        slab, index = ctypes.c_int(), ctypes.c_int64()
        check(lib().vr_dataset_peak(self.d, int(song), ctypes.byref(p), at, ctypes.byref(slab), ctypes.byref(index)))
        peak = np.float32(p.value)
        return (peak, np.complex64(complex(at[0], at[1])), int(slab.value), int(index.value)) if where else peak


class Handle:
    """Owns one vr_handle (one GPU, one stream)."""

    def __init__(self, device, n_fft, hop_length, nout, nout_lstm, is_complex=False):
        self._h = ctypes.c_void_p()
        if is_complex:
            check(lib().vr_create_ex(int(device), int(n_fft), int(hop_length), int(nout), int(nout_lstm), VR_CREATE_COMPLEX,
                                     ctypes.byref(self._h)))
        else:
            check(lib().vr_create(int(device), int(n_fft), int(hop_length), int(nout), int(nout_lstm),
                                  ctypes.byref(self._h)))
        self.device = int(device)

    def close(self):
        if getattr(self, '_h', None) and self._h.value:
            lib().vr_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def h(self):
        if not self._h.value:
            raise VRError('handle is closed')
        return self._h

    def pipeline_buffer_bytes(self, release=False):
        """vr_pipeline_buffer: device bytes this handle holds for the training input pipeline (over a wave store: the rows of one batch),
        which vr_arena_bytes does not count; release=True frees them (the next batch allocates again)."""
        b = ctypes.c_int64()
        check(lib().vr_pipeline_buffer(self.h, ctypes.byref(b), 1 if release else 0))
        return int(b.value)

    def param_infos(self):
        out = []
        n = lib().vr_num_params(self.h)
        buf = ctypes.create_string_buffer(256)
        shape = (ctypes.c_int64 * 4)()
        nd, is64, tr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        for i in range(n):
            check(lib().vr_param_info(self.h, i, buf, 256, shape, ctypes.byref(nd), ctypes.byref(is64),
                                      ctypes.byref(tr)))
            out.append((buf.value.decode(), tuple(int(shape[j]) for j in range(nd.value)), bool(is64.value),
                        bool(tr.value)))
        return out

    def set_param(self, key, arr):
        arr = np.require(arr, requirements=['C'])      # (ascontiguousarray would turn 0-d into 1-d)
        shape = (ctypes.c_int64 * max(arr.ndim, 1))(*arr.shape)
        check(lib().vr_set_param(self.h, key.encode(), np_ptr(arr), shape, arr.ndim))

    def get_param(self, key, shape, is_int64):
        arr = np.empty(shape, dtype=np.int64 if is_int64 else np.float32)
        check(lib().vr_get_param(self.h, key.encode(), np_ptr(arr), arr.nbytes))
        return arr
