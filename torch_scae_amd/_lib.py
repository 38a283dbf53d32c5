"""ctypes binding of libscae_hip.so (C ABI: include/scae_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` /
``make -C torch_scae_amd/csrc``.  There is NO fallback: if it is missing, or a
tensor is not on a HIP device, the ops raise.
"""
import ctypes
import os
from ctypes import (POINTER, Structure, c_char_p, c_double, c_float, c_int,
                    c_int64, c_uint32, c_uint64, c_void_p)

_HERE = os.path.dirname(os.path.abspath(__file__))
# (SCAE_HIP_LIB: another build of the same library, for A/B measurements)
LIB_PATH = os.environ.get("SCAE_HIP_LIB") or os.path.join(_HERE, "lib",
                                                        "libscae_hip.so")

P = c_void_p  # device pointer


class DecoderDesc(Structure):
    """struct scae_decoder_desc"""
    _fields_ = [("templates", P), ("templates_alpha", P), ("pose", P),
                ("presence", P), ("bg_image", P), ("bg_value", P),
                ("bg_mixing_logit", P), ("temperature_logit", P),
                ("out_scale", P),
                ("B", c_int), ("M", c_int), ("C", c_int), ("th", c_int),
                ("tw", c_int), ("H", c_int), ("W", c_int),
                ("template_repeat", c_int)]


class LikelihoodBwdDesc(Structure):
    """struct scae_likelihood_bwd_desc"""
    _fields_ = [(n, P) for n in (
        "vote", "scale", "vote_presence", "dummy_vote", "x", "presence",
        "posterior", "winner_idx", "g_lpp", "g_winner", "g_winner_presence",
        "g_soft_winner", "g_soft_winner_presence", "g_posterior",
        "g_mixing_log_prob", "g_mixing_logit", "gvote", "gscale",
        "gvote_presence", "gx", "gpresence", "gdummy_partial")] + [
        ("B", c_int), ("O", c_int), ("M", c_int)]


class GemmDesc(Structure):
    """struct scae_gemm_desc"""
    _fields_ = [("A", P), ("B", P), ("C", P), ("bias", P), ("mask", P),
                ("asum", P), ("batch", c_int), ("M", c_int), ("N", c_int),
                ("K", c_int), ("a_kcontig", c_int), ("lda", c_int),
                ("a_batch", c_int64), ("b_kcontig", c_int), ("ldb", c_int),
                ("b_batch", c_int64), ("ldc", c_int), ("c_batch", c_int64),
                ("bias_ld", c_int), ("bias_batch", c_int64), ("ldmask", c_int),
                ("mask_batch", c_int64), ("asum_batch", c_int64),
                ("relu", c_int), ("asum_ld", c_int), ("c_nomask", P)]


class MlpChainLayer(Structure):
    """struct scae_mlp_chain_layer"""
    _fields_ = [("w", P), ("w_gs", c_int64), ("ldw", c_int), ("K", c_int),
                ("N", c_int), ("bias", P), ("bias_gs", c_int64),
                ("bias_ld", c_int), ("gate", P), ("gate_gs", c_int64),
                ("gate_bs", c_int64), ("out", P), ("out_gs", c_int64),
                ("out_bs", c_int64), ("relu", c_int)]


class MlpChainDesc(Structure):
    """struct scae_mlp_chain_desc"""
    _fields_ = [("layer", MlpChainLayer * 4), ("n_layers", c_int), ("in_", P),
                ("in_gs", c_int64), ("in_bs", c_int64), ("in_dim", c_int),
                ("B", c_int), ("G", c_int), ("row_tile", c_int),
                ("bf16", c_int)]


class VotesDesc(Structure):
    """struct scae_votes_desc"""
    _fields_ = [(n, P) for n in ("all_param", "cpr_static", "bias_cvr",
                                 "bias_caps", "bias_vote", "bias_scale",
                                 "noise_caps", "noise_vote")] + \
        [("noise_scale", c_float), ("V", c_int), ("ld_param", c_int),
         ("similarity", c_int), ("learn_vote_scale", c_int),
         ("allow_deformations", c_int)] + \
        [(n, P) for n in ("vote", "scale", "vote_presence", "logit_caps",
                          "logit_vote", "reg_partial", "caps_presence",
                          "caps_arg", "gvote", "gscale", "gvote_presence",
                          "glogit_caps", "glogit_vote", "greg", "gcaps_presence",
                          "gall_param", "gcpr_in", "gall_param_gated")]


class MlpChainForm(Structure):
    """struct scae_mlp_chain_form"""
    _fields_ = [("rows", c_int), ("narrow", c_int),
                ("scratch_in_weights", c_int)]


class SumSegment(Structure):
    """struct scae_sum_segment"""
    _fields_ = [("dst", P), ("begin", c_int64), ("end", c_int64),
                ("period", c_int64)]


class SumJob(Structure):
    """struct scae_sum_job"""
    _fields_ = [("src", P), ("rows", c_int64), ("cols", c_int64),
                ("segments", POINTER(SumSegment)), ("n_segments", c_int)]


class ScaledSum(Structure):
    """struct scae_scaled_sum"""
    _fields_ = [("src", P), ("n", c_int64), ("scale", c_float), ("dst", P)]


class TrainLogDesc(Structure):
    """struct scae_train_log_desc"""
    _fields_ = [("rows", P), ("step", P), ("capacity", c_int), ("acc", P),
                ("prior_prob", P), ("post_prob", P), ("label", P), ("ncls", c_int),
                ("lr", P)]


class LossExtras(Structure):
    """struct scae_loss_extras"""
    _fields_ = [("rec_sums", P), ("n_rec", c_int), ("reg", P),
                ("w_reg", c_float), ("g_rec_sums", P), ("g_reg", P),
                ("loss", P), ("g_loss", P), ("defer_combine", c_int),
                ("out12", P), ("train_log", POINTER(TrainLogDesc))]


class KMeansDesc(Structure):
    """struct scae_kmeans_desc"""
    _fields_ = [("x", P), ("N", c_int64), ("F", c_int), ("k", c_int), ("R", c_int),
                ("G", c_int), ("max_iter", c_int), ("centroids", P), ("labels", P),
                ("part_sum", P), ("part_count", P), ("part_changed", P),
                ("part_inertia", P), ("state", P), ("inertia", P)]


class ProbeDesc(Structure):
    """struct scae_probe_desc"""
    _fields_ = [("x", P), ("y", P), ("N", c_int64), ("F", c_int), ("C", c_int), ("R", c_int),
                ("G", c_int), ("max_iter", c_int), ("mean", P), ("scale", P), ("l2", P),
                ("step", P), ("tol", P), ("W", P), ("V", P), ("grad", P), ("t", P),
                ("part_grad", P), ("part_loss", P), ("history", P), ("state", P)]


class TsneDesc(Structure):
    """struct scae_tsne_desc"""
    _fields_ = [("N", c_int), ("G", c_int), ("n_iter", c_int), ("exaggeration_iter", c_int),
                ("check_every", c_int), ("early_exaggeration", c_float),
                ("learning_rate", c_float), ("P", P), ("Y", P), ("velocity", P), ("gains", P),
                ("part", P), ("rows", P), ("block", P), ("plogp", P), ("history", P)]


class TsneSparseDesc(Structure):
    """struct scae_tsne_sparse_desc"""
    _fields_ = [("N", c_int), ("G", c_int), ("n_iter", c_int), ("exaggeration_iter", c_int),
                ("check_every", c_int), ("early_exaggeration", c_float),
                ("learning_rate", c_float), ("indptr", P), ("cols", P), ("vals", P),
                ("nnz", c_int64), ("Y", P), ("velocity", P), ("gains", P), ("part", P),
                ("rows", P), ("block", P), ("plogp", P), ("history", P)]


class SeedFoldDesc(Structure):
    """struct scae_seed_fold_desc"""
    _fields_ = [(n, P) for n in (
        "seeds", "wq", "bq", "wk", "bk", "wv", "bv", "wo", "bo", "w2", "b2",
        "q", "wkf", "bkf", "wvf", "bvf", "wv2e", "wowv")] + \
        [("O", c_int), ("C", c_int), ("D", c_int)]


class FirstLayerDesc(Structure):
    """struct scae_first_layer_desc"""
    _fields_ = [("img", P), ("w", P), ("bias", P), ("out", P)] + \
        [(n, c_int) for n in ("B", "Cin", "IH", "IW", "Cout", "stride",
                              "n_layers")] + \
        [("rw", P * 8), ("rwf", P * 8), ("rwd", P * 8),
         ("rCout", c_int * 8), ("rCin", c_int * 8),
         ("out_h", P), ("rwfh", P * 8), ("rwdh", P * 8)]


class BatchSourceDesc(Structure):
    """struct scae_batch_source_desc"""
    _fields_ = [("images", P), ("labels", P), ("index", P), ("rows", c_int64),
                ("n", c_int64)] + \
        [(n, c_int) for n in ("image_u8", "label_u8", "C", "h", "w", "H", "W",
                              "shuffle", "translate")] + \
        [("seed", c_uint64), ("epoch", c_int64), ("position", c_int64),
         ("rank", c_int), ("world", c_int), ("wrap", c_int),
         ("affine", P), ("affine_rows", c_int64)]


class SeedFoldGrads(Structure):
    """struct scae_seed_fold_grads"""
    _fields_ = [(n, P) for n in (
        "g_q", "g_wkf", "g_bkf", "g_wvf", "g_bvf", "d_seeds", "d_wq", "d_bq",
        "d_wk", "d_bk", "d_wv", "d_bv", "d_wo", "d_bo", "d_w2", "d_b2",
        "gv2e", "t1")]


# name -> argtypes; mirrors include/scae_hip.h one to one
SIGNATURES = {
    "scae_abi_version": [],
    "scae_error_string": [c_int],
    "scae_uniform_f32": [P, c_int64, P, P],
    "scae_geometric_transform_fwd_f32": [P, P, c_int64, c_int, c_int, c_int, P],
    "scae_geometric_transform_bwd_f32": [P, P, P, c_int64, c_int, c_int, c_int,
                                         P],
    "scae_mat3_mul_fwd_f32": [P, P, P, c_int64, c_int, P],
    "scae_mat3_mul_bwd_f32": [P, P, P, P, P, c_int64, c_int, P],
    "scae_qkv_attention_fwd_f32": [P, P, P, P, P, P, c_int, c_int, c_int,
                                   c_int, c_int, c_float, P],
    "scae_qkv_attention_fwd_bf16": [P, P, P, P, P, P, c_int, c_int, c_int,
                                    c_int, c_int, c_float, P],
    "scae_qkv_attention_bwd_f32": [P, P, P, P, P, P, P, P, P, c_int, c_int,
                                   c_int, c_int, c_int, c_float, P],
    "scae_set_encoder_param_count": [c_int] * 5,
    "scae_set_encoder_grid": [c_int],
    "scae_set_encoder_supported": [c_int] * 6,
    "scae_set_encoder_fwd_f32": [c_int, P, P, P, P, P, P, P, P] + [c_int] * 7 + [P],
    "scae_set_encoder_bwd_f32": [c_int, P, P, P, P, P, P, P, P, P, P]
                                + [c_int] * 7 + [P],
    "scae_render_gmm_sums_bwd_likelihood_f32": [P] * 13,
    "scae_set_encoder_fwd_logprob_f32": [c_int, P, P, P, P, P, P, P, P] + [c_int] * 7
                                        + [P] * 6,
    "scae_set_encoder_fwd_logprob_bf16": [c_int, P, P, P, P, P, P, P, P] + [c_int] * 7
                                         + [P] * 6,
    "scae_set_encoder_bf16_supported": [c_int] * 6,
    "scae_set_encoder_fwd_bf16": [c_int, P, P, P, P, P, P, P, P] + [c_int] * 7 + [P],
    "scae_set_encoder_bwd_bf16": [c_int, P, P, P, P, P, P, P, P, P, P]
                                 + [c_int] * 7 + [P],
    "scae_seed_attention_splits": [c_int] * 2,
    "scae_seed_attention_grid": [c_int] * 2,
    "scae_seed_attention_supported": [c_int] * 4,
    "scae_seed_attention_fwd_f32": [P] * 9 + [c_int] * 5 + [P],
    "scae_seed_attention_bwd_f32": [P] * 10 + [c_int] * 5 + [P],
    "scae_seed_attention_mfma_supported": [c_int] * 4,
    "scae_seed_attention_mfma_rows": [c_int],
    "scae_seed_attention_mfma_fwd_f32": [P] * 7 + [c_int] * 4 + [P],
    "scae_seed_attention_mfma_bwd_f32": [P] * 8 + [c_int] * 4 + [P],
    "scae_seed_attention_mfma_fwd_bf16": [P] * 7 + [c_int] * 4 + [P],
    "scae_seed_attention_mfma_bwd_bf16": [P] * 8 + [c_int] * 4 + [P],
    "scae_seed_attention_mfma_bwd_gemm_f32": [P] * 8 + [c_int] * 4
    + [POINTER(GemmDesc), c_int, P],
    "scae_seed_attention_mfma_bwd_gemm_bf16": [P] * 8 + [c_int] * 4
    + [POINTER(GemmDesc), c_int, P],
    "scae_object_encoder_bwd_supported": [c_int] * 9,
    "scae_object_encoder_bwd_gemm_f32": [P] * 8 + [c_int] * 4
    + [POINTER(GemmDesc), c_int] + [c_int, P, P, P, P, P, P, P, P, P] + [c_int] * 7 + [P],
    "scae_object_encoder_bwd_gemm_bf16": [P] * 8 + [c_int] * 4
    + [POINTER(GemmDesc), c_int] + [c_int, P, P, P, P, P, P, P, P, P] + [c_int] * 7 + [P],
    "scae_seed_attention_mfma_reduce_f32": [P, c_int] + [P] * 7 + [c_int] * 2 + [P],
    "scae_seed_fold_supported": [c_int] * 3,
    "scae_seed_fold_fwd_f32": [POINTER(SeedFoldDesc), P],
    "scae_seed_fold_bwd_f32": [POINTER(SeedFoldDesc), POINTER(SeedFoldGrads), P],
    "scae_layer_norm_rows": [c_int64],
    "scae_layer_norm_fwd_f32": [P] * 6 + [c_int64, c_int, c_float, P],
    "scae_layer_norm_bwd_f32": [P] * 7 + [c_int64, c_int, P],
    "scae_gemm_f32": [P] * 6 + [c_int] * 6 + [c_int64, c_int, c_int, c_int64,
                                              c_int, c_int64, c_int, c_int64,
                                              c_int, c_int64, c_int64, c_int, c_int,
                                              P],
    "scae_gemm_bf16": [P] * 6 + [c_int] * 6 + [c_int64, c_int, c_int, c_int64,
                                              c_int, c_int64, c_int, c_int64,
                                              c_int, c_int64, c_int64, c_int, c_int,
                                              P],
    "scae_gemm_pair_f32": [POINTER(GemmDesc), POINTER(GemmDesc), P],
    # the library's own record of a step's kernel launches (train_step.TrainStep)
    "scae_launch_list_begin": [P],
    "scae_launch_list_end": [P],
    "scae_launch_list_size": [P],
    "scae_launch_list_run": [P, P],
    "scae_launch_list_lane": [P, c_int],
    "scae_launch_list_timeline": [P, P, P, POINTER(c_float), c_int],
    "scae_launch_list_free": [P],
    "scae_gemm_multi_f32": [POINTER(GemmDesc), c_int, P],
    "scae_gemm_multi_bf16": [POINTER(GemmDesc), c_int, P],
    "scae_mlp_chain_max_width": [],
    "scae_mlp_chain_fwd_f32": [POINTER(MlpChainDesc), P],
    "scae_mlp_chain_bwd_f32": [POINTER(MlpChainDesc), P],
    "scae_mlp_chain_votes_fwd_f32": [POINTER(MlpChainDesc), POINTER(VotesDesc), P],
    "scae_mlp_chain_votes_bwd_f32": [POINTER(MlpChainDesc), POINTER(VotesDesc), P],
    "scae_mlp_chain_get_form": [POINTER(MlpChainDesc), POINTER(VotesDesc), c_int,
                                POINTER(MlpChainForm)],
    "scae_gemm_pair_bf16": [POINTER(GemmDesc), POINTER(GemmDesc), P],
    "scae_conv3x3_wf_floats": [c_int, c_int],
    "scae_conv3x3_relayout_f32": [P, P, P, c_int, c_int, P],
    "scae_conv3x3_bf16r_supported": [c_int] * 6,
    "scae_conv3x3_first_fwd_relayout_bf16": [P] * 4 + [c_int] * 7 + [P] * 8,
    "scae_cvt_bf16_batch": [c_int, P, P, P, P],
    "scae_conv3x3_fwd_bf16r": [P] * 7 + [c_int] * 6 + [P],
    "scae_conv3x3_dgrad_bf16r": [P] * 5 + [c_int] * 6 + [P],
    "scae_conv3x3_wgrad_bf16r_splits": [c_int] * 5,
    "scae_conv3x3_wgrad_bf16r": [P] * 3 + [c_int] * 6 + [P],
    "scae_conv3x3_relayout_batch_f32": [c_int, P, P, P, P, P, P],
    "scae_conv3x3_first_fwd_f32": [P] * 4 + [c_int] * 6 + [P],
    "scae_conv3x3_first_fwd_relayout_f32": [P] * 4 + [c_int] * 7 + [P] * 6,
    "scae_conv3x3_first_wgrad_reduce_f32": [P] * 3 + [c_int] * 7 + [P] * 7,
    "scae_conv3x3_first_wgrad_rows": [c_int] * 2,
    "scae_conv3x3_first_wgrad_f32": [P] * 3 + [c_int] * 6 + [P],
    "scae_conv3x3_fwd_f32": [P] * 6 + [c_int] * 6 + [P],
    "scae_conv3x3_fwd_fold_f32": [P] * 6 + [c_int] * 6 + [POINTER(SeedFoldDesc), P],
    "scae_conv3x3_fwd_res_supported": [c_int] * 6,
    "scae_conv3x3_fwd_res_f32": [P] * 6 + [c_int] * 7 + [P],
    "scae_conv3x3_fwd_bf16": [P] * 6 + [c_int] * 6 + [P],
    "scae_conv3x3_dgrad_f32": [P] * 4 + [c_int] * 6 + [P],
    "scae_conv3x3_bwd_pair_f32": [P] * 5 + [c_int] * 6 + [P],
    "scae_conv3x3_bwd_pair_reduce_f32": [P] * 5 + [c_int] * 6 + [P, c_int] + [P] * 7
    + [c_int] * 2 + [P],
    "scae_conv3x3_bwd_pair_fold_f32": [P] * 5 + [c_int] * 6
    + [POINTER(SeedFoldDesc), POINTER(SeedFoldGrads), P],
    "scae_conv3x3_bwd_pair_bf16": [P] * 5 + [c_int] * 6 + [P],
    "scae_conv3x3_wgrad_reduce_batch_f32": [c_int] + [P] * 7,
    "scae_conv3x3_wgrad_splits": [c_int] * 5,
    "scae_conv3x3_wgrad_f32": [P] * 5 + [c_int] * 6 + [P],
    "scae_attention_pool_supported": [c_int] * 3,
    "scae_attention_pool_fwd_f32": [P, P] + [c_int] * 4 + [P],
    "scae_attention_pool_bwd_f32": [P, P, P] + [c_int] * 4 + [P],
    "scae_stage_batch": [P, P, c_int64, P, P, c_int64, P],
    "scae_step_prologue_f32": [P, P, c_int64, P, P, c_int64, P, c_int64, P,
                               POINTER(SeedFoldDesc), P],
    "scae_step_prologue_first_f32": [P, P, c_int64, P, P, c_int64, P, c_int64,
                                     P, POINTER(SeedFoldDesc),
                                     POINTER(FirstLayerDesc), P],
    "scae_gather_batch_f32": [P, P, c_int, POINTER(BatchSourceDesc), P],
    "scae_step_prologue_source_f32": [P, P, c_int, POINTER(BatchSourceDesc), P, c_int64, P,
                                      POINTER(SeedFoldDesc), POINTER(FirstLayerDesc), P],
    "scae_rmsprop_step_f32": [P, P, P, P, c_int64, c_float, P, c_float, c_float,
                              c_float, c_float, c_float, P],
    "scae_rmsprop_sums_step_f32": [P, P, P, P, c_int64, c_float, P, c_float, c_float,
                                   c_float, c_float, POINTER(SumJob), c_int, P],
    "scae_flat_opt_step_f32": [P, P, P, P, P, c_int64, P, P, c_int, c_double, c_double, c_float,
                               c_float, c_float, c_int, c_float, c_int, P],
    "scae_flat_opt_sums_step_f32": [P, P, P, P, P, c_int64, P, P, c_int, c_double, c_double,
                                    c_float, c_float, c_int, c_float, POINTER(SumJob), c_int, P],
    "scae_grad_sq_partials_f32": [P, c_int64, P, c_int, POINTER(c_int), P],
    "scae_grad_sq_partials_sums_f32": [P, c_int64, P, c_int, POINTER(c_int), POINTER(SumJob),
                                       c_int, P],
    "scae_rmsprop_clip_step_f32": [P, P, P, P, c_int64, c_float, P, c_float, c_float, c_float,
                                   c_float, c_float, P, c_int, c_float, P, P],
    "scae_flat_opt_clip_step_f32": [P, P, P, P, P, c_int64, P, P, c_int, c_double, c_double,
                                    c_float, c_float, c_float, c_int, c_float, c_int, P, c_int,
                                    c_float, P, P],
    # gradient accumulation (grad_accumulate.hip; the accumulate forms take acc after grad)
    "scae_grad_accumulate_f32": [P, P, c_int64, P],
    "scae_grad_accumulate_sums_f32": [P, P, c_int64, POINTER(SumJob), c_int, P],
    "scae_grad_sq_acc_partials_f32": [P, P, c_int64, P, c_int, POINTER(c_int), P],
    "scae_grad_sq_acc_partials_sums_f32": [P, P, c_int64, P, c_int, POINTER(c_int),
                                           POINTER(SumJob), c_int, P],
    "scae_rmsprop_acc_step_f32": [P, P, P, P, P, c_int64, c_float, P, c_float, c_float,
                                  c_float, c_float, c_float, P],
    "scae_rmsprop_acc_sums_step_f32": [P, P, P, P, P, c_int64, c_float, P, c_float, c_float,
                                       c_float, c_float, POINTER(SumJob), c_int, P],
    "scae_rmsprop_acc_clip_step_f32": [P, P, P, P, P, c_int64, c_float, P, c_float, c_float,
                                       c_float, c_float, c_float, P, c_int, c_float, P, P],
    "scae_flat_opt_acc_step_f32": [P, P, P, P, P, P, c_int64, P, P, c_int, c_double, c_double,
                                   c_float, c_float, c_float, c_int, c_float, c_int, P],
    "scae_flat_opt_acc_sums_step_f32": [P, P, P, P, P, P, c_int64, P, P, c_int, c_double,
                                        c_double, c_float, c_float, c_int, c_float,
                                        POINTER(SumJob), c_int, P],
    "scae_flat_opt_acc_clip_step_f32": [P, P, P, P, P, P, c_int64, P, P, c_int, c_double,
                                        c_double, c_float, c_float, c_float, c_int, c_float,
                                        c_int, P, c_int, c_float, P, P],
    # the non-finite guard: the clip forms' arguments, then guard_state after norm_out
    "scae_rmsprop_guard_step_f32": [P, P, P, P, c_int64, c_float, P, c_float, c_float, c_float,
                                    c_float, c_float, P, c_int, c_float, P, P, P],
    "scae_rmsprop_acc_guard_step_f32": [P, P, P, P, P, c_int64, c_float, P, c_float, c_float,
                                        c_float, c_float, c_float, P, c_int, c_float, P, P, P],
    "scae_flat_opt_guard_step_f32": [P, P, P, P, P, c_int64, P, P, c_int, c_double, c_double,
                                     c_float, c_float, c_float, c_int, c_float, c_int, P, c_int,
                                     c_float, P, P, P],
    "scae_flat_opt_acc_guard_step_f32": [P, P, P, P, P, P, c_int64, P, P, c_int, c_double,
                                         c_double, c_float, c_float, c_float, c_int, c_float,
                                         c_int, P, c_int, c_float, P, P, P],
    # per-segment norms of a flat buffer into a device ring (grad_norms.hip)
    "scae_segment_norms_chunk": [],
    "scae_segment_norms_f32": [P, P, c_int64, P, c_int, P, c_int, P, c_int, c_int, c_float,
                               P, P, P, c_int, P],
    "scae_capsule_head_fwd_f32": [P, P, c_float, c_int, P, P, P, P, P] + [c_int] * 4 + [P],
    "scae_capsule_head_conv_supported": [c_int] * 4,
    "scae_capsule_head_conv_preferred": [c_int] * 5,
    "scae_capsule_head_conv_fwd_f32": [P, P, P, c_int, P, P, c_float, c_int, P, P, P, P, P]
    + [c_int] * 4 + [P],
    "scae_capsule_head_conv_fwd_tc_f32": [P, P, P, c_int, P, P, c_float, c_int, P, P, P, P, P]
    + [c_int] * 4 + [P] * 8 + [c_int] * 6 + [P],
    "scae_capsule_head_bwd_f32": [P, P, P, c_float, c_int, P, P, P, P, P] + [c_int] * 4 + [P],
    "scae_capsule_head_bwd_tc_f32": [P, P, P, c_float, c_int, P, P, P, P] + [c_int] * 4
    + [P] * 12 + [c_int] * 6 + [P],
    "scae_template_color_supported": [c_int] * 4,
    "scae_template_color_partial_rows": [c_int] * 2,
    "scae_template_color_fwd_f32": [P] * 9 + [c_int] * 8 + [P],
    "scae_template_color_bwd_f32": [P] * 12 + [c_int] * 8 + [P],
    "scae_sum_rows_f32": [P, c_int64, c_int64, POINTER(SumSegment), c_int, P],
    "scae_sum_rows_multi_f32": [POINTER(SumJob), c_int, P],
    "scae_scaled_sums_f32": [POINTER(ScaledSum), c_int, P],
    "scae_class_probs_supported": [c_int] * 2,
    "scae_class_probs_f32": [P] * 6 + [c_int] * 4 + [POINTER(ScaledSum), c_int, P],
    "scae_capsule_votes_fwd_f32": [P] * 8 + [c_float] + [P] * 8
                                  + [c_int] * 7 + [P],
    "scae_capsule_votes_bwd_f32": [P] * 8 + [c_float] + [P] * 11
                                  + [c_int] * 7 + [P],
    "scae_capsule_likelihood_fwd_f32": [P] * 17 + [c_int] * 3 + [P],
    "scae_capsule_likelihood_bwd_f32": [P] * 22 + [c_int] * 3 + [P],
    "scae_loss_tail_supported": [c_int] * 3,
    "scae_loss_tail_workspace_floats": [c_int] * 3,
    "scae_loss_tail_fwd_f32": [P] * 6 + [POINTER(LossExtras), P, P] + [c_int] * 8
    + [POINTER(c_float), c_float, P],
    "scae_loss_tail_defer_preferred": [c_int] * 2,
    "scae_loss_tail_combine_f32": [P] * 6 + [POINTER(LossExtras), P, P] + [c_int] * 8
    + [POINTER(c_float), c_float, P],
    "scae_loss_tail_fwd_class_probs_f32": [P] * 6 + [POINTER(LossExtras), P, P]
    + [c_int] * 8 + [POINTER(c_float), c_float] + [P] * 6 + [c_int] * 4
    + [POINTER(ScaledSum), c_int, P],
    "scae_loss_tail_bwd_f32": [P] * 6 + [POINTER(LossExtras)] + [P] * 7
    + [c_int] * 8 + [POINTER(c_float), c_float, P],
    "scae_eval_tail_f32": [P] * 6 + [POINTER(LossExtras), P, P] + [c_int] * 8
    + [POINTER(c_float), c_float] + [P] * 5,
    "scae_loss_tail_fwd_class_probs_sink_f32": [P] * 6 + [POINTER(LossExtras), P, P]
    + [c_int] * 8 + [POINTER(c_float), c_float] + [P] * 6 + [c_int] * 4
    + [POINTER(ScaledSum), c_int, P, P],
    "scae_eval_tail_sink_f32": [P] * 6 + [POINTER(LossExtras), P, P] + [c_int] * 8
    + [POINTER(c_float), c_float] + [P] * 6,
    "scae_eval_tail_records_f32": [P] * 6 + [POINTER(LossExtras), P, P] + [c_int] * 8
    + [POINTER(c_float), c_float] + [P] * 7,
    "scae_eval_records_f32": [P] * 6 + [c_int] * 4 + [P, P],
    "scae_eval_accumulate_f32": [P] * 5 + [c_int] * 2 + [P] * 3,
    "scae_train_log_f32": [P] * 3 + [POINTER(TrainLogDesc), c_int, P],
    "scae_eval_features_f32": [P, P, c_int, c_int, c_int, P, P],
    "scae_kmeans_supported": [c_int] * 2,
    "scae_kmeans_groups": [c_int64, c_int],
    "scae_kmeans_lloyd_f32": [POINTER(KMeansDesc), c_int, P],
    "scae_kmeans_pp_f32": [P, c_int64, c_int, c_int, c_int, c_uint32, P, P, P, P],
    "scae_kmeans_assign_f32": [P, c_int64, c_int, c_int, P, P, P],
    "scae_kmeans_contingency": [P, P, c_int64, c_int, c_int, P, P, P],
    "scae_probe_supported": [c_int] * 3,
    "scae_probe_groups": [c_int64, c_int],
    "scae_probe_predict_blocks": [c_int64],
    "scae_probe_moments_f64": [P, P, c_int64, c_int, c_int, P, P, P, P],
    "scae_probe_fit_f32": [POINTER(ProbeDesc), c_int, P],
    "scae_probe_predict_f32": [P, c_int64, c_int, c_int] + [P] * 8,
    "scae_tsne_supported": [c_int] * 2,
    "scae_tsne_groups": [c_int],
    "scae_tsne_affinities_f32": [P, c_int, c_int, c_float, P, P, P, P, P],
    "scae_tsne_run_f32": [POINTER(TsneDesc), c_int, c_int, P],
    "scae_tsne_sparse_supported": [c_int] * 3,
    "scae_tsne_sparse_groups": [c_int],
    "scae_tsne_knn_bandwidths_f32": [P, c_int, c_int, c_float, P, P, P],
    "scae_tsne_sparse_run_f32": [POINTER(TsneSparseDesc), c_int, c_int, P],
    "scae_knn_wide_f32": [P, c_int64, c_int, c_int, P, P, P, P],
    "scae_knn_supported": [c_int64, c_int64, c_int, c_int],
    "scae_knn_groups": [c_int64, c_int64],
    "scae_knn_f32": [P, c_int64, P, c_int64, c_int, c_int, c_int, P, P, P, P],
    "scae_knn_vote_f32": [P, P, c_int64, c_int, P, c_int64, POINTER(c_int), c_int, c_int, P, P],
    "scae_knn_ranks_f32": [P, c_int64, c_int, P, c_int, P, P, P, P, P],
    "scae_cluster_quality_supported": [c_int64, c_int, c_int64],
    "scae_cluster_quality_labels": [P, c_int64, c_int64, P, P, P],
    "scae_cluster_quality_silhouette_f32": [P, P, P, P, c_int64, c_int, c_int64] + [P] * 7,
    "scae_cluster_quality_dispersion_f32": [P, P, c_int64, c_int, c_int64, P, P],
    "scae_template_render_fwd_f32": [POINTER(DecoderDesc), P, P, P],
    "scae_render_gmm_logprob_fwd_f32": [POINTER(DecoderDesc), P, P, P, P, P],
    "scae_render_gmm_bwd_f32": [POINTER(DecoderDesc)] + [P] * 12 + [P],
    "scae_render_gmm_logprob_tiles": [POINTER(DecoderDesc)],
    "scae_render_gmm_forms": [POINTER(DecoderDesc), c_int, P, P, POINTER(c_int)],
    "scae_render_gmm_logprob_sums_fwd_f32": [POINTER(DecoderDesc)] + [P] * 4 + [P],
    "scae_render_gmm_sums_bwd_f32": [POINTER(DecoderDesc)] + [P] * 10 + [P],
    "scae_gmm_log_prob_fwd_f32": [P] * 5 + [c_int] * 4 + [c_int64, P],
    "scae_gmm_log_prob_bwd_f32": [P] * 9 + [c_int] * 4 + [c_int64, P],
    "scae_gmm_mean_f32": [P] * 3 + [c_int] * 4 + [c_int64, P],
    "scae_gmm_mode_f32": [P] * 4 + [c_int] * 5 + [c_int64, P],
    "scae_render_gmm_mode_f32": [POINTER(DecoderDesc), P, c_int, c_int, c_int, P],
    "scae_render_gmm_parts_f32": [POINTER(DecoderDesc), P, P, P, c_int] + [P] * 7 + [c_int, c_int, P],
    "scae_render_gmm_parts_geometry": [POINTER(DecoderDesc), c_int, POINTER(c_int)],
    "scae_image_sheet_f32": [c_int, POINTER(P), POINTER(c_int)] + [c_int] * 5 + [c_float, P, P],
}

# (everything else returns int)
_RESTYPES = {"scae_error_string": c_char_p,
             "scae_loss_tail_workspace_floats": c_int64,
             "scae_conv3x3_wf_floats": c_int64,
             "scae_launch_list_begin": P,
             "scae_launch_list_free": None}
EVAL_ACC_DOUBLES = 17        # SCAE_EVAL_ACC_DOUBLES: the accumulator of scae_eval_*
TRAIN_LOG_ROW = 19           # SCAE_TRAIN_LOG_ROW: one row of scae_train_log_desc's ring
KMEANS_STATE_INTS = 4        # SCAE_KMEANS_STATE_INTS: per restart of scae_kmeans_desc's state
PROBE_STATE_INTS = 4         # SCAE_PROBE_STATE_INTS: per problem of scae_probe_desc's state
TSNE_MAX_N = 32768           # SCAE_TSNE_MAX_N
TSNE_MAX_F = 256             # SCAE_TSNE_MAX_F
TSNE_HISTORY_COLS = 3        # SCAE_TSNE_HISTORY_COLS: iteration, KL, gradient norm
TSNE_BLOCK_DOUBLES = 640     # SCAE_TSNE_BLOCK_DOUBLES: scae_tsne_desc's block workspace
TSNE_MAX_NEIGHBORS = 128     # SCAE_TSNE_MAX_NEIGHBORS
TSNE_SPARSE_MAX_N = 262144   # SCAE_TSNE_SPARSE_MAX_N
TSNE_SPARSE_BLOCK_DOUBLES = 5120   # SCAE_TSNE_SPARSE_BLOCK_DOUBLES
KNN_MAX_K = 64               # SCAE_KNN_MAX_K
KNN_MAX_F = 256              # SCAE_KNN_MAX_F
KNN_MAX_KS = 8               # SCAE_KNN_MAX_KS
CLUSTER_QUALITY_MAX_F = 256  # SCAE_CLUSTER_QUALITY_MAX_F
EVAL_SINK_INT64S = 4         # struct scae_eval_sink: rows, capacity, cursor, overflow
# struct scae_eval_records: rows, capacity, cursor, overflow, confusion, ncls, labelled
EVAL_RECORDS_INT64S = 7
EVAL_RECORD_FLOATS = 9       # SCAE_EVAL_RECORD_FLOATS: one row of scae_eval_records
EVAL_RECORDS_MAX_CLASSES = 64   # SCAE_EVAL_RECORDS_MAX_CLASSES
FLAT_OPT_STATE_INTS = 2112   # SCAE_FLAT_OPT_STATE_INTS: the step_state of scae_flat_opt_*
GRAD_SQ_MAX_PARTIALS = 4096  # SCAE_GRAD_SQ_MAX_PARTIALS: scae_grad_sq_partials_*
NORM_CHUNK = 2048            # SCAE_NORM_CHUNK: elements per chunk of scae_segment_norms_f32
NORM_GROUP_CHUNKS = 16       # SCAE_NORM_GROUP_CHUNKS: chunks per workgroup, at most
NORM_INF = 0                 # SCAE_NORM_INF: scae_segment_norms_f32's norm_kind for p = inf
ABI_VERSION = 3     # SCAE_ABI_VERSION of the include/scae_hip.h this binding mirrors

_lib = None


class ScaeHipError(RuntimeError):
    pass


def load():
    """Load (once) and return the ctypes handle; raises if not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ScaeHipError(
            f"{LIB_PATH} is missing: build it with `python -c 'import "
            f"__graft_entry__ as g; g.build()'` or `make -C torch_scae_amd/csrc`."
            " torch_scae_amd has no CPU / eager fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.argtypes = argtypes
        fn.restype = _RESTYPES.get(name, c_int)
        if argtypes and argtypes[-1] is P and not name.startswith("scae_launch_list"):
            setattr(lib, name, _recording(fn))     # a launcher: (..., void *stream)
    if lib.scae_abi_version() != ABI_VERSION:
        raise ScaeHipError(
            f"{LIB_PATH} has ABI version {lib.scae_abi_version()}, this package "
            f"binds version {ABI_VERSION}: rebuild it (make -C torch_scae_amd/csrc)")
    _lib = lib
    return lib


# Launch recording (train_step.TrainStep(replay="launches")): while a recorder is installed
# every successful launcher call is kept as (function, arguments); the list IS the step -- the
# same launches a captured HIP graph holds -- and can be re-issued on any stream without the
# Python above the C ABI.  The arguments keep what they point to alive (device buffers of the
# capture's private pool are owned by the graph object).
_RECORDER = None


def _recording(fn):
    def launcher(*args):
        rc = fn(*args)
        if _RECORDER is not None and rc == 0:
            # arguments converted ONCE to the C types of the prototype (a replay then only
            # passes ready ctypes objects: the per-call conversion of ~20 Python ints / floats
            # per launcher was most of a replay's host time)
            conv = []
            for t, a in zip(fn.argtypes, args):
                if a is None or isinstance(a, (int, float)):
                    a = t(a) if a is not None else t()
                conv.append(a)
            _RECORDER.append((fn, tuple(conv[:-1]), args))
        return rc
    launcher.__name__ = getattr(fn, "__name__", "launcher")
    return launcher


class recorder:
    """``with _lib.recorder() as launches:`` -- collects the launcher calls made inside."""

    def __enter__(self):
        global _RECORDER
        self.prev, self.launches = _RECORDER, []
        _RECORDER = self.launches
        return self.launches

    def __exit__(self, *exc):
        global _RECORDER
        _RECORDER = self.prev
        return False


def replay(launches, stream):
    """Re-issue recorded launches on ``stream`` (a ``c_void_p`` handle): every launcher's
    last argument is its stream."""
    for fn, cargs, _keep in launches:
        rc = fn(*cargs, stream)
        if rc != 0:
            check(rc, getattr(fn, "__name__", "launch"))


ERR_UNSUPPORTED = -2     # SCAE_ERR_UNSUPPORTED


def check(rc, what):
    if rc != 0:
        msg = load().scae_error_string(rc)
        raise ScaeHipError(f"{what} failed with code {rc}: "
                           f"{msg.decode() if msg else '?'}")


def call(name, *args):
    check(getattr(load(), name)(*args), name)


def try_call(name, *args):
    """``call`` for a merged launcher that may decline a shape: True when it
    ran, False for SCAE_ERR_UNSUPPORTED (the caller launches the parts in
    turn); any other error raises."""
    rc = getattr(load(), name)(*args)
    if rc == ERR_UNSUPPORTED:
        return False
    check(rc, name)
    return True
