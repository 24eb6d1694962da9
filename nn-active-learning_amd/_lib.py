"""ctypes binding of libalq.so (include/alq.h).  No fallback: if the HIP library is missing the
import of any device function raises, so a CPU-only or stale install fails loudly."""
import ctypes as C
import enum
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, os.environ.get('ALQ_LIB', 'libalq.so'))   # ALQ_LIB: diagnostic builds
BUILD_SCRIPT = os.path.join(_HERE, 'csrc', 'build.sh')

ALQ_CONV, ALQ_CONVT, ALQ_POOL, ALQ_FC = 0, 1, 2, 3
ALQ_EINVAL = -1


class EngineInfo(enum.IntEnum):
    """The `what` of alq_model_engine_info (the ALQ_INFO_* enum of include/alq.h, which documents every index)."""
    SUBNORMALS_OK = 0
    C3D_FWD = 1
    C3D_BWD = 2
    C3D_ONE_ACC = 3
    FLIP_OVERFLOW = 5
    F16_DERIVED = 6
    T3D_FWD = 7
    T3D_BWD = 8
    E3D_BWD = 9
    D3D_FWD = 10
    D3D_BWD = 11
    F3D_FWD = 12
    C3D_BWD_FORM = 13
    HOST_PACK_ELEMS = 14
    LSUM = 15
    DCP_FORM = 16
    E3D_BWD_FORM = 17


class AlqError(RuntimeError):
    pass


class LayerT(C.Structure):
    """Mirror of alq_layer_t."""
    _fields_ = [('type', C.c_int32), ('cout', C.c_int32), ('k', C.c_int32 * 3), ('s', C.c_int32 * 3),
                ('relu', C.c_int32), ('skip_src', C.c_int32)]


class LossT(C.Structure):
    """Mirror of alq_loss_t."""
    _fields_ = [('kind', C.c_int32), ('focal_gamma', C.c_float), ('gce_q', C.c_float), ('lwf_T', C.c_float),
                ('d_class_w', C.c_void_p), ('d_sample_w', C.c_void_p), ('d_targets', C.c_void_p), ('d_old_logits', C.c_void_p)]


class TileLattice(C.Structure):
    """Mirror of alq_tile_lattice_t (order Z, H, W)."""
    _fields_ = [('dims', C.c_int32 * 3), ('tile', C.c_int32 * 3), ('stride', C.c_int32 * 3)]


class DcrfParams(C.Structure):
    """Mirror of alq_dcrf_params (defaults: the reference's DCRF_postprocess_2D call)."""
    _fields_ = [('sdims_smooth', C.c_float * 2), ('sdims_app', C.c_float * 2), ('schan', C.c_float), ('compat_smooth', C.c_float),
                ('compat_app', C.c_float), ('niter', C.c_int32)]


_P = C.c_void_p
_SIGNATURES = {
    'alq_last_error': (C.c_char_p, []),
    'alq_version': (C.c_int, []),
    'alq_ctx_create': (C.c_int, [C.c_int, _P, C.POINTER(_P)]),
    'alq_ctx_destroy': (C.c_int, [_P]),
    'alq_ctx_use_side_stream': (C.c_int, [_P, C.c_int]),
    'alq_ctx_set_stream': (C.c_int, [_P, _P]),
    'alq_ctx_synchronize': (C.c_int, [_P]),
    'alq_model_create': (C.c_int, [_P, C.POINTER(LayerT), C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(_P)]),
    'alq_model_destroy': (C.c_int, [_P]),
    'alq_model_num_param_layers': (C.c_int, [_P]),
    'alq_model_max_batch': (C.c_int, [_P]),
    'alq_model_out_voxels': (C.c_int, [_P]),
    'alq_dense_head_work_bytes': (C.c_size_t, [C.c_int, C.c_int]),
    'alq_dense_head_fwd': (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, _P, _P, _P, _P]),
    'alq_dense_head_bwd': (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, C.c_int, _P, _P, _P, _P]),
    'alq_dense_head_bwd_geometry': (C.c_int, [C.c_int64, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int),
                                              C.POINTER(C.c_int)]),
    'alq_fcgemm_geometry': (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    'alq_model_param_sizes': (C.c_int, [_P, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'alq_model_layer_out_elems': (C.c_int, [_P, C.c_int, C.POINTER(C.c_int64)]),
    'alq_model_set_weights': (C.c_int, [_P, C.c_int, _P, _P]),
    'alq_model_set_weights_device': (C.c_int, [_P, C.c_int, _P, _P]),
    'alq_model_layer_packs_on_device': (C.c_int, [_P, C.c_int]),
    'alq_gather_normalize': (C.c_int, [_P, C.POINTER(_P), C.c_int, C.c_int, C.POINTER(C.c_int64), _P, C.c_int64,
                                       C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int, C.c_int, _P]),
    'alq_forward': (C.c_int, [_P, _P, C.c_int, _P, _P, _P, C.c_int]),
    'alq_score_entropy': (C.c_int, [_P, _P, C.c_int64, _P, _P]),
    'alq_topk_work_bytes': (C.c_size_t, [C.c_int64]),
    'alq_topk_uncertain': (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, _P]),
    'alq_topk_merge': (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, _P]),
    'alq_fisher': (C.c_int, [_P, _P, C.c_int, _P, C.c_double, _P, _P, _P, _P, _P, _P]),
    'alq_forward_rows': (C.c_int, [_P, _P, _P, C.c_int, _P, _P, _P, C.c_int]),
    'alq_fisher_rows': (C.c_int, [_P, _P, _P, C.c_int, _P, C.c_double, _P, _P, _P, _P, _P, _P]),
    'alq_model_num_params': (C.c_int64, [_P]),
    'alq_forward_dropout': (C.c_int, [_P, _P, C.c_int, C.c_float, C.c_uint64, C.c_int64, C.POINTER(C.c_int32), C.c_int, _P, _P]),
    'alq_param_grads': (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_float, C.c_float, C.c_uint64, C.c_int64,
                                  C.POINTER(C.c_int32), C.c_int, C.c_int, _P, _P, _P]),
    'alq_grad_sqnorms': (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P]),
    'alq_hess_vecp': (C.c_int, [_P, _P, C.c_int, _P, C.c_float, _P, _P, C.c_int, _P, _P]),
    'alq_class_layer_sums': (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P]),
    'alq_diag_fisher': (C.c_int, [_P, _P, C.c_int, _P, _P]),
    'alq_topk_mask_work_bytes': (C.c_size_t, [C.c_int64]),
    'alq_topk_mask': (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, _P]),
    'alq_threshold_mask': (C.c_int, [_P, _P, C.c_int64, C.c_double, _P]),
    'alq_committee_update': (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, _P, _P, _P]),
    'alq_eval_counts': (C.c_int, [_P, _P, _P, C.c_int64, _P, C.c_int, C.c_int64, _P, _P]),
    'alq_sgd_step': (C.c_int, [_P, _P, _P, C.c_int64, C.c_float]),
    'alq_adam_step': (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int64]),
    'alq_loss_stats': (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.POINTER(LossT), _P]),
    'alq_param_grads_loss': (C.c_int, [_P, _P, C.c_int, _P, C.POINTER(LossT), C.c_float, C.c_float, C.c_float, C.c_uint64, C.c_int64,
                                       C.POINTER(C.c_int32), C.c_int, _P, _P, _P]),
    'alq_rmsprop_step': (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float]),
    'alq_mt_trip_voxels': (C.c_int64, []),
    'alq_mt_cotangent': (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, _P, C.POINTER(LossT), C.c_float, C.c_float, C.c_int, _P, _P]),
    'alq_mt_stats': (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, _P, C.POINTER(LossT), C.c_int, _P]),
    'alq_param_grads_loss_mt': (C.c_int, [_P, _P, C.c_int, _P, C.POINTER(LossT), C.c_float, _P, C.c_int, C.c_float, C.c_float,
                                          C.c_uint64, C.c_int64, C.POINTER(C.c_int32), C.c_int, _P, _P, _P]),
    'alq_dense_head_fwd_au': (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P]),
    'alq_model_set_aleatoric': (C.c_int, [_P, C.c_int]),
    'alq_forward_au': (C.c_int, [_P, _P, C.c_int, C.c_float, C.c_uint64, C.c_int64, C.POINTER(C.c_int32), C.c_int, _P, _P, _P, _P]),
    'alq_mt_au_trip_voxels': (C.c_int64, []),
    'alq_mt_cotangent_au': (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int64, _P, C.POINTER(LossT), C.c_float, C.c_float, C.c_float, C.c_float,
                                      C.c_int, _P, _P]),
    'alq_mt_stats_au': (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int64, _P, C.POINTER(LossT), C.c_float, C.c_int, _P]),
    'alq_param_grads_loss_mt_au': (C.c_int, [_P, _P, C.c_int, _P, C.POINTER(LossT), C.c_float, _P, C.c_int, C.c_float, C.c_float, C.c_float,
                                             C.c_float, C.c_uint64, C.c_int64, C.POINTER(C.c_int32), C.c_int, _P, _P, _P]),
    'alq_ema_step': (C.c_int, [_P, _P, _P, C.c_int64, C.c_float]),
    'alq_perturb_input': (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_int64, C.c_int,
                                    C.c_float]),
    'alq_sq_accum': (C.c_int, [_P, _P, C.c_int64, C.c_int, _P]),
    'alq_shrink_sum': (C.c_int, [_P, _P, C.c_int, C.c_int64, C.POINTER(C.c_int64), C.c_int, _P]),
    'alq_fisher_classes': (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    'alq_row_norms': (C.c_int, [_P, _P, C.c_int64, C.c_int, _P]),
    'alq_cosine_sims': (C.c_int, [_P, _P, C.c_int64, _P, C.c_int, C.c_int, _P, _P, _P]),
    'alq_colsum_work_bytes': (C.c_size_t, [C.c_int64, C.c_int]),
    'alq_colsum_max': (C.c_int, [_P, _P, C.c_int64, C.c_int, _P, _P, _P, _P]),
    'alq_take_colmax': (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, _P]),
    'alq_fold_rowmax': (C.c_int, [_P, _P, C.c_int, C.c_int64, _P]),
    'alq_local_var2d': (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int, _P, C.c_int64, _P]),
    'alq_segment_min': (C.c_int, [_P, _P, C.POINTER(C.c_int64), C.c_int32, _P, _P, C.c_int64, _P]),
    'alq_cc_work_bytes': (C.c_size_t, [C.POINTER(C.c_int64)]),
    'alq_cc_label': (C.c_int, [_P, _P, C.POINTER(C.c_int64), C.c_int, C.c_int, _P]),
    'alq_cc_keep_largest': (C.c_int, [_P, _P, C.POINTER(C.c_int64), C.c_int, C.c_int, _P, _P, _P]),
    'alq_fill_holes': (C.c_int, [_P, _P, C.POINTER(C.c_int64), _P, _P, _P]),
    'alq_cc_sizes': (C.c_int, [_P, _P, C.c_int64, _P]),
    'alq_cc_relabel': (C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int32, _P, _P]),
    'alq_surface_mask': (C.c_int, [_P, _P, C.POINTER(C.c_int64), C.c_int, _P]),
    'alq_edt_max_axis': (C.c_int, []),
    'alq_edt_work_bytes': (C.c_size_t, [C.POINTER(C.c_int64)]),
    'alq_edt_geometry': (C.c_int, [C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    'alq_edt_sq': (C.c_int, [_P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_double), _P, _P]),
    'alq_masked_work_bytes': (C.c_size_t, [C.c_int64]),
    'alq_masked_geometry': (C.c_int, [C.c_int64, C.POINTER(C.c_int32)]),
    'alq_masked_dist_stats': (C.c_int, [_P, _P, _P, C.c_int64, _P, _P]),
    'alq_masked_select': (C.c_int, [_P, _P, _P, C.c_int64, C.POINTER(C.c_int64), C.c_int, _P, _P]),
    'alq_confusion_counts': (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, _P, _P]),
    'alq_confusion_window': (C.c_int, [C.c_int]),
    'alq_unc_accumulate': (C.c_int, [_P, _P, C.c_int, C.c_int64, C.c_int, _P, _P]),
    'alq_slice_scores': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, _P, _P, _P, _P, _P, _P]),
    'alq_slice_scores_geometry': (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.POINTER(C.c_int64)]),
    'alq_dcrf_work_bytes': (C.c_size_t, [C.POINTER(C.c_int64)]),
    'alq_dcrf2d': (C.c_int, [_P, _P, _P, C.POINTER(C.c_int64), C.POINTER(DcrfParams), _P, _P, _P]),
    'alq_llfc_grads': (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    'alq_llfc_hess_max_bytes': (C.c_size_t, []),
    'alq_llfc_hess': (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P]),
    'alq_llfc_if_path': (C.c_int, [C.c_int, C.c_int]),
    'alq_llfc_if_work_bytes': (C.c_size_t, [C.c_int, C.c_int]),
    'alq_llfc_stoch_if': (C.c_int, [_P, _P, _P, _P, C.c_int, _P, _P, C.c_int, _P, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int,
                                    _P, _P]),
    'alq_aopt_tile': (C.c_int, []),
    'alq_aopt_max_workgroups': (C.c_int, []),
    'alq_aopt_work_bytes': (C.c_size_t, [C.c_int64, C.c_int]),
    'alq_aopt_svec': (C.c_int, [_P, _P, C.c_int64, C.c_int, _P]),
    'alq_aopt_stats': (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, _P, _P, C.c_double, C.c_double, _P, _P]),
    'alq_aopt_direction': (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, _P, _P, _P, _P, C.c_double, C.c_double, C.c_double, _P, _P, _P]),
    'alq_aopt_linesearch': (C.c_int, [_P, _P, _P, C.c_int64, _P, C.c_int, _P, _P]),
    'alq_aopt_update': (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int, C.c_double, _P, _P]),
    'alq_vol_pack': (C.c_int, [_P, C.POINTER(_P), C.c_int, C.c_int, C.POINTER(C.c_int32), _P]),
    'alq_mask_pack': (C.c_int, [_P, _P, C.POINTER(C.c_int32), _P]),
    'alq_slice_batch_check': (C.c_int, [C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.c_int]),
    'alq_slice_batch': (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int,
                                  C.POINTER(C.c_int32), C.c_int, _P, _P, _P]),
    'alq_slice_batch_trip_rows': (C.c_int64, []),
    'alq_slice_batch_launch_samples': (C.c_int, []),
    'alq_tile_lattice_check': (C.c_int, [C.POINTER(TileLattice)]),
    'alq_tile_count': (C.c_int64, [C.POINTER(TileLattice), C.POINTER(C.c_int32)]),
    'alq_tile_origin': (C.c_int, [C.POINTER(TileLattice), C.c_int64, C.POINTER(C.c_int32)]),
    'alq_tile_gather': (C.c_int, [_P, _P, C.c_int, C.POINTER(TileLattice), C.c_int64, C.c_int64, C.c_float, _P]),
    'alq_tile_blend': (C.c_int, [_P, _P, C.c_int, C.POINTER(TileLattice), C.c_int64, C.c_int64, _P, _P, _P, _P]),
    'alq_tile_blend_trip_voxels': (C.c_int64, []),
    'alq_tile_finalize': (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int32), C.c_int, _P, _P]),
    'alq_slic_work_bytes': (C.c_size_t, [C.POINTER(C.c_int64), C.c_int, C.c_int, C.c_int]),
    'alq_slic_geometry': (C.c_int, [_P, C.POINTER(C.c_int64), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    'alq_slic': (C.c_int, [_P, _P, _P, C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_int,
                           C.c_double, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    'alq_comm_unique_id':(C.c_int, [_P]),
    'alq_comm_init': (C.c_int, [_P, _P, C.c_int, C.c_int]),
    'alq_comm_destroy': (C.c_int, [_P]),
    'alq_allreduce_sum': (C.c_int, [_P, _P, C.c_int64]),
    'alq_prof_enable': (C.c_int, [_P, C.c_int]),
    'alq_prof_reset': (C.c_int, [_P]),
    'alq_prof_num_classes': (C.c_int, []),
    'alq_prof_class_name': (C.c_char_p, [C.c_int]),
    'alq_prof_read': (C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    'alq_model_debug_copy': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.POINTER(C.c_int64)]),
    'alq_debug_rowmax_abs': (C.c_int, [_P, _P, C.c_int, C.c_int64, _P]),
    'alq_debug_fwd_bounds': (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int32),
                                       C.c_int, C.c_int, _P]),
    'alq_debug_set_stamp_buffer': (C.c_int, [_P]),
    'alq_debug_set': (C.c_int, [C.c_int, C.c_int]),
    'alq_model_engine_info': (C.c_int, [_P, C.c_int]),
    'alq_ref64_scores': (C.c_int, [_P, _P, C.c_int, _P, _P, _P, _P, _P, C.c_int, _P, C.c_int, C.c_double, C.c_int, _P, _P, _P, _P, _P, _P]),
    'alq_synth_patches': (C.c_int, [_P, C.c_uint64, C.c_int64, C.c_int64, C.c_int64, _P]),
}

_lib = None


def build(force=False):
    """Compiles csrc/*.hip for gfx950 into libalq.so (hipcc cross-compiles without a GPU)."""
    global _lib
    if os.path.exists(LIB_PATH) and not force:
        srcs = [os.path.join(_HERE, 'csrc', f) for f in os.listdir(os.path.join(_HERE, 'csrc'))
                if f.endswith(('.hip', '.h', '.inc'))] + [os.path.join(os.path.dirname(_HERE), 'include', 'alq.h')]
        if all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(s) for s in srcs):
            return LIB_PATH
    subprocess.check_call(['bash', BUILD_SCRIPT])
    _lib = None
    return LIB_PATH


def lib():
    """The loaded library; raises AlqError when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AlqError('%s is missing: run `python __graft_entry__.py` (or csrc/build.sh); there is no '
                           'CPU fallback for the device path' % LIB_PATH)
        # libalq.so needs libamdhip64.so.7; PyTorch-ROCm ships its own copy under that SONAME.  Load
        # torch FIRST so that the process holds ONE HIP runtime and torch's device pointers and
        # stream handles are valid inside libalq (loading libalq first would pull in /opt/rocm's
        # copy beside torch's: two runtimes, "no ROCm-capable device" on the second).
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def exported_names():
    return sorted(_SIGNATURES)


def check(rc):
    if rc != 0:
        raise AlqError('libalq error %d: %s' % (rc, lib().alq_last_error().decode()))


def ptr(t, byte_offset=0):
    """The address of a tensor's memory, `byte_offset` bytes in, as the C ABI takes it; None (an argument left out) stays None."""
    return None if t is None else C.c_void_p(t.data_ptr() + byte_offset)


def check_tensor(t, dtype, numel=None, device=None, optional=False):
    """What every entry point asks of a tensor it hands to the library: `dtype` (or one of a tuple of them), contiguous, on
    `device` and of `numel` elements where those are given.  AssertionError otherwise; None passes only with `optional`."""
    ok = optional if t is None else (
        (t.dtype in dtype if isinstance(dtype, tuple) else t.dtype == dtype) and t.is_contiguous() and
        (device is None or t.device == device) and (numel is None or int(t.numel()) == int(numel)))
    if not ok:
        raise AssertionError('expected a contiguous %s tensor (elements: %s, device: %s), got %s' % (
            dtype, numel, device, t if t is None else (t.dtype, tuple(t.shape), t.stride(), t.device)))
