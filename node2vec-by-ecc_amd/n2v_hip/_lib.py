"""ctypes binding of libn2v_hip.so (the C-ABI declared in include/n2v_hip.h).

There is no CPU fallback: if the HIP library is missing or a call fails, this raises.
"""
import ctypes as C
import os

# torch first: it ships its own libamdhip64; loading ours before torch's would put a second,
# device-less HIP runtime into the process (kernel launches then fail with "no ROCm-capable
# device").  With torch loaded first the library binds to the runtime torch initialised.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("N2V_HIP_LIB") or os.path.join(_HERE, "libn2v_hip.so")  # override: A/B builds

N2V_OK = 0
N2V_STATUS_ZERO_NORM = 1
N2V_STATUS_ZERO_POP = 2
RNG_UNIFORMS = 0
RNG_PHILOX = 1
RNG_UNIFORMS_TILED = 2

# name -> (restype, argtypes); mirrors include/n2v_hip.h, n2v_bine.h and n2v_sim.h one to one
_i64, _i32, _u64, _f64, _ptr = C.c_int64, C.c_int32, C.c_uint64, C.c_double, C.c_void_p
BINE_SEQUENTIAL = 0
BINE_PARALLEL = 1
BINE_PARALLEL_STORE = 2
SIGNATURES = {
    "n2v_abi_version": (C.c_int, []),
    "n2v_last_error": (C.c_char_p, []),
    "n2v_alias_setup_tables": (C.c_int, [_i64, _ptr, _ptr, _ptr]),
    "n2v_build_node_tables": (C.c_int, [_i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "n2v_build_node_tables_pop": (C.c_int, [_i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "n2v_build_edge_tables_wave_pop": (C.c_int, [_i64, _ptr, _ptr, _ptr, _ptr, _f64, _ptr, _ptr, _i64, _i64, _ptr, _ptr, _i64,
                                                 _ptr, _i64, _ptr]),
    "n2v_walk_on_the_fly_pop": (C.c_int, [_ptr, _ptr, _ptr, _f64, _f64, _i32, _i64, _ptr, _ptr, _i64, _i64, _i64, _i64, _i64,
                                          _i32, _i32, _ptr, _ptr, _u64, _ptr, _i64, _ptr, _ptr, _ptr, _ptr]),
    "n2v_build_edge_tables_wave": (C.c_int, [_i64, _ptr, _ptr, _ptr, _ptr, _f64, _f64, _i32, _ptr, _ptr, _i64, _i64,
                                             _ptr, _ptr, _ptr, _ptr, _ptr, _i64, _ptr, _i64, _ptr]),
    "n2v_edge_tables_wave_scratch_bytes": (C.c_int64, [_i64]),
    "n2v_build_edge_recs": (C.c_int, [_i64, _i64, _ptr, _ptr, _ptr, _i64, _i64, _i64, _ptr, _ptr]),
    "n2v_walk": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _i64, _i64, _i64, _i64, _i64, _i32, _i32, _ptr, _ptr,
                           _u64, _ptr, _ptr, _ptr]),
    "n2v_mt19937_jump_host": (C.c_int, [_ptr, _i64, _i32, _ptr]),
    "n2v_mt19937_jump_polys_host": (C.c_int, [_i64, _i32, _ptr]),
    "n2v_mt19937_jump_device": (C.c_int, [_ptr, _i32, _ptr, _i32, _ptr]),
    "n2v_mt19937_fill": (C.c_int, [_ptr, _i32, _i32, _i64, _i64, _ptr, _ptr, _ptr]),
    "n2v_mt19937_fill_tiled": (C.c_int, [_ptr, _i32, _i32, _i64, _i64, _i32, _ptr, _ptr, _ptr]),
    "n2v_build_fat_slots": (C.c_int, [_i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "n2v_walk_fat": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _i64, _i64, _i64, _i64, _i64, _i32, _i32, _ptr, _ptr, _i64, _u64,
                               _ptr, _ptr, _ptr]),
    "n2v_walk_on_the_fly": (C.c_int, [_ptr, _ptr, _ptr, _f64, _f64, _i32, _i64, _ptr, _i64, _i64, _i64, _i64, _i64, _i32,
                                      _i32, _ptr, _ptr, _u64, _ptr, _i64, _ptr, _ptr, _ptr, _ptr]),
    "n2v_walk_otf_lds_slots": (C.c_int32, []),
    "n2v_walk_otf_max_waves": (C.c_int32, []),
    "n2v_walk_hybrid": (C.c_int, [_ptr, _ptr, _ptr, _f64, _f64, _i32, _i64, _ptr, _ptr, _ptr, _ptr, _i64, _i64, _i64, _i64,
                                  _i64, _i32, _i32, _ptr, _ptr, _u64, _ptr, _i64, _ptr, _ptr, _ptr, _ptr]),
    "n2v_sgns_init": (C.c_int, [_ptr, _ptr, _i64, _i32, _i32, _u64, _ptr]),
    "n2v_build_neg_lut": (C.c_int, [_ptr, _i64, _i32, _ptr, _ptr]),
    "n2v_sgns_train": (C.c_int, [_ptr, _ptr, _i64, _i32, _ptr, _ptr, _i64, _i32, _i32, _i32, _i32, _ptr, _ptr,
                                 _ptr, _i32, C.c_float, C.c_float, _i64, _i64, _i64, _i64, _u64, _u64, _ptr, _i32,
                                 _i32, _i32, _ptr, _ptr]),
    "n2v_sgns_train_span": (C.c_int, [_ptr, _ptr, _i64, _i32, _ptr, _ptr, _i64, _i32, _i32, _i32, _i32, _ptr, _ptr,
                                      _ptr, _i32, C.c_float, C.c_float, _i64, _i64, _i64, _u64, _ptr, _i32, _i32, _i32,
                                      _ptr, _i32, _i32, _i64, _i64, _ptr, _ptr]),
    "n2v_sgns_default_blocks": (C.c_int32, [_i64, _i32]),
    "n2v_cbow_max_sentence": (C.c_int32, []),
    "n2v_cbow_corpus_check": (C.c_int, [_ptr, _ptr, _i64, _i64, _i64, _i32, _ptr, _ptr]),
    "n2v_cbow_train": (C.c_int, [_ptr, _ptr, _i64, _i64, _i32, _ptr, _ptr, _i64, _i32, _i32, _i32, _i32, _i32, _ptr, _ptr,
                                 _ptr, _i32, C.c_float, C.c_float, _i64, _i64, _i64, _i64, _u64, _u64, _ptr, _i32, _i32,
                                 _ptr, _ptr]),
    "n2v_sgns_csr_train": (C.c_int, [_ptr, _ptr, _i64, _i64, _i32, _ptr, _i32, _i64, _i64, _ptr, _ptr, _i64, _i32, _i32,
                                     _i32, _i32, _ptr, _ptr, _ptr, _i32, C.c_float, C.c_float, _i64, _i64, _i64, _i64,
                                     _u64, _u64, _ptr, _i32, _i32, _ptr, _ptr]),
    "n2v_merge_snapshot": (C.c_int, [_ptr, _ptr, _ptr, _i64, _i32, _ptr, _ptr, _ptr, _ptr, _ptr, _i32, _ptr]),
    "n2v_merge_hot_apply": (C.c_int, [_ptr, _ptr, _ptr, _i32, _ptr, _ptr, _i64, _ptr, _i32, _ptr]),
    "n2v_merge_flush": (C.c_int, [_ptr, _ptr, _ptr, _i64, _i32, _ptr, _ptr, _ptr, _i32, _ptr]),
    "n2v_merge_pack_rows": (C.c_int, [_ptr, _ptr, _i32, _ptr, _i64, _ptr, _i32, _ptr]),
    "n2v_tsum_pack": (C.c_int, [_ptr, _i32, _i32, _ptr, _i32, _ptr]),
    "n2v_tsum_apply": (C.c_int, [_ptr, _i32, _i32, _ptr, _i32, _ptr]),
    # include/n2v_bine.h
    "n2v_bine_spmv": (C.c_int, [_i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "n2v_bine_hits_normalise": (C.c_int, [_i64, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "n2v_bine_walk_counts": (C.c_int, [_ptr, _i64, _i64, _i32, _i32, _ptr, _ptr, _ptr]),
    "n2v_bine_walk_lengths": (C.c_int, [_ptr, _ptr, _ptr, _i64, _i64, _f64, _i32, _u64, _ptr, _ptr]),
    "n2v_bine_walk": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _i64, _i64, _u64, _ptr, _ptr]),
    "n2v_bine_neg_pools": (C.c_int, [_ptr, _ptr, _i64, _i64, _i64, _i64, _i32, _f64, _u64, _ptr, _ptr]),
    "n2v_lsh_sha1_labels": (C.c_int, [_ptr, _i32, _ptr, _i64, _ptr, _ptr]),
    "n2v_lsh_minhash": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _i64, _i64, _ptr, _ptr]),
    "n2v_lsh_forest_query": (C.c_int, [_ptr, _ptr, _ptr, _i64, _i32, _ptr, _ptr, _ptr]),
    "n2v_lsh_leader_round": (C.c_int, [_ptr, _ptr, _i64, _ptr, _ptr, _ptr]),
    "n2v_lsh_pools": (C.c_int, [_ptr, _ptr, _i32, _ptr, _i64, _i32, _i32, _u64, _i32, _ptr, _i64, _i32, _ptr, _ptr]),
    "n2v_bine_init": (C.c_int, [_ptr, _ptr, _i64, _i32, _i32, _u64, _ptr]),
    "n2v_bine_train_pass": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _i64, _i64, _ptr, _ptr, _i32, _i32, _ptr, _ptr, _ptr,
                                      _ptr, _ptr, _ptr, _i32, _i32, _i32, _f64, _f64, _f64, _ptr, _i32, _u64, _u64,
                                      _i32, _i32, _ptr]),
    "n2v_bine_lambda_step": (C.c_int, [_ptr, _f64, _ptr]),
    "n2v_bine_rec_segments": (C.c_int32, [_i64, _i64]),
    "n2v_bine_rec_topn": (C.c_int, [_ptr, _i64, _i32, _i32, _ptr, _i64, _ptr, _i64, _i32, _i32, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "n2v_bine_rec_metrics": (C.c_int, [_ptr, _i64, _i32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    # include/n2v_sim.h
    "n2v_sim_prepare": (C.c_int, [_ptr, _i32, _i32, _ptr, _i64, _i32, _ptr, _i32, _ptr]),
    "n2v_sim_block": (C.c_int, [_ptr, _i64, _i64, _ptr, _i64, _i32, _i32, _i64, _ptr, _i64, _ptr]),
    "n2v_sim_topk_scan": (C.c_int, [_ptr, _i64, _i64, _ptr, _i64, _i32, _i32, _i32, _ptr, _ptr, _i64, _ptr, _ptr, _ptr,
                                    _i64, _ptr, _ptr]),
    "n2v_sim_rows_count": (C.c_int, [_ptr, _i64, _i64, _i64, C.c_float, _ptr, _ptr]),
    "n2v_sim_rows_fill": (C.c_int, [_ptr, _i64, _i64, _i64, C.c_float, _ptr, _ptr, _ptr, _ptr]),
    "n2v_sim_rows_topk": (C.c_int, [_ptr, _i64, _i64, _i64, _i32, _ptr, _ptr, _ptr]),
    "n2v_sim_knn_max_k": (C.c_int32, []),
    "n2v_sim_knn_max_seg": (C.c_int32, []),
    "n2v_sim_knn_scratch": (C.c_int64, [_i64, _i32, _i32]),
    "n2v_sim_knn": (C.c_int, [_ptr, _i64, _ptr, _i64, _i32, _i32, _ptr, _i32, _i32, _ptr, _ptr, _ptr, _ptr]),
    "n2v_eccknn_max_k": (C.c_int32, []),
    "n2v_eccknn_max_dense": (C.c_int64, []),
    "n2v_eccknn_densify": (C.c_int, [_ptr, _ptr, _ptr, _i64, _i64, _i64, _ptr, _ptr, _ptr]),
    "n2v_eccknn_sim": (C.c_int, [_ptr, _ptr, _i64, _i64, _ptr, _i32, _i32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "n2v_eccknn_sparse_chunk": (C.c_int32, []),
    "n2v_eccknn_csr_check": (C.c_int, [_ptr, _ptr, _i64, _i64, _i64, _ptr, _ptr]),
    "n2v_eccknn_sim_sparse": (C.c_int, [_ptr, _ptr, _ptr, _i64, _i64, _i64, _ptr, _i32, _i32, _ptr, _ptr, _ptr, _ptr, _ptr,
                                        _ptr, _ptr]),
    "n2v_eccknn_baselines": (C.c_int, [_ptr, _ptr, _ptr, _i64, _ptr, _ptr, _ptr, _i64, _f64, _i32, _f64, _f64, _ptr, _ptr, _ptr]),
    "n2v_eccknn_pearson": (C.c_int, [_ptr, _ptr, _i64, _i64, _ptr, _i32, _i32, _f64, _ptr, _ptr, _f64, _ptr, _ptr, _ptr, _ptr,
                                     _ptr, _ptr, _ptr, _ptr]),
    "n2v_eccknn_pearson_sparse": (C.c_int, [_ptr, _ptr, _ptr, _i64, _i64, _i64, _ptr, _i32, _i32, _f64, _ptr, _ptr, _f64, _ptr,
                                            _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "n2v_eccknn_estimate": (C.c_int, [_ptr, _i64, _ptr, _ptr, _ptr, _i64, _ptr, _ptr, _i64, _i32, _i32, _ptr, _ptr, _ptr,
                                      _ptr]),
    "n2v_eccknn_row_moments": (C.c_int, [_ptr, _ptr, _i64, _i64, _f64, _ptr, _ptr, _ptr]),
    "n2v_eccknn_estimate_centered": (C.c_int, [_ptr, _i64, _ptr, _ptr, _ptr, _i64, _ptr, _ptr, _i64, _i32, _i32, _i32, _i32,
                                               _f64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "n2v_eccknn_topn_centered": (C.c_int, [_ptr, _i64, _ptr, _ptr, _ptr, _i64, _i32, _ptr, _ptr, _i64, _ptr, _i64, _i32, _i32,
                                           _f64, _f64, _f64, _i32, _i32, _i32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr,
                                           _ptr]),
    "n2v_eccknn_predict": (C.c_int, [_ptr, _ptr, _ptr, _i64, _f64, _f64, _f64, _ptr, _ptr, _ptr]),
    "n2v_eccknn_estimate_sweep": (C.c_int, [_ptr, _i64, _ptr, _ptr, _ptr, _i64, _ptr, _ptr, _i64, _ptr, _i32, _ptr, _i32, _ptr,
                                            _ptr, _ptr, _ptr]),
    "n2v_eccknn_estimate_sweep_centered": (C.c_int, [_ptr, _i64, _ptr, _ptr, _ptr, _i64, _ptr, _ptr, _i64, _ptr, _i32, _ptr, _i32,
                                                     _i32, _i32, _f64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "n2v_eccknn_errors": (C.c_int, [_ptr, _ptr, _i64, _i64, _ptr, _ptr, _ptr]),
    "n2v_svd_max_factors": (C.c_int32, []),
    "n2v_svd_max_strata": (C.c_int32, []),
    "n2v_svd_blocks_check": (C.c_int, [_ptr, _ptr, _ptr, _i64, _i64, _i64, _i64, _ptr, _ptr]),
    "n2v_svd_epoch": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _i64, _i64, _i64, _i64, _i32, _f64, _i32, _f64, _f64, _f64, _f64, _f64,
                                _f64, _f64, _f64, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "n2v_svd_estimate": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _i64, _i64, _i32, _f64, _i32, _ptr, _ptr, _i64, _ptr, _ptr, _ptr]),
    "n2v_nmf_depth": (C.c_int32, []),
    "n2v_nmf_lists_check": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _i64, _i64, _i64, _ptr, _ptr, _ptr]),
    "n2v_nmf_epoch": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _i64, _i64, _i64, _i32, _f64, _f64, _ptr, _ptr,
                                _ptr, _ptr, _ptr]),
    "n2v_topn_segments": (C.c_int32, [_i64, _i64]),
    "n2v_eccknn_topn": (C.c_int, [_ptr, _i64, _ptr, _ptr, _ptr, _i64, _i32, _ptr, _ptr, _i64, _ptr, _i64, _i32, _i32, _f64,
                                  _f64, _f64, _i32, _i32, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "n2v_svd_topn": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _i64, _i64, _i32, _f64, _i32, _ptr, _ptr, _i64, _ptr, _i64, _f64, _f64,
                               _f64, _i32, _i32, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "n2v_slopeone_dev": (C.c_int, [_ptr, _ptr, _i64, _i64, _ptr, _ptr, _ptr, _ptr]),
    "n2v_slopeone_dev_sparse": (C.c_int, [_ptr, _ptr, _ptr, _i64, _i64, _i64, _ptr, _ptr, _ptr, _ptr]),
    "n2v_slopeone_estimate": (C.c_int, [_ptr, _ptr, _i64, _ptr, _ptr, _i64, _i64, _ptr, _ptr, _ptr, _i64, _ptr, _ptr, _ptr,
                                        _ptr]),
    "n2v_slopeone_topn": (C.c_int, [_ptr, _ptr, _i64, _ptr, _ptr, _i64, _i64, _ptr, _ptr, _ptr, _i64, _ptr, _i64, _f64, _f64,
                                    _f64, _i32, _i32, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "n2v_cocl_max_clusters": (C.c_int32, []),
    "n2v_cocl_averages": (C.c_int, [_ptr, _ptr, _ptr, _i64, _i64, _i64, _ptr, _ptr, _i32, _i32, _f64, _ptr, _ptr, _ptr, _ptr, _ptr,
                                    _ptr]),
    "n2v_cocl_assign": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _i64, _i64, _i64, _i32, _i32, _i32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr,
                                  _ptr, _ptr]),
    "n2v_cocl_estimate": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _i64, _i64, _i32, _i32, _f64, _ptr, _ptr, _i64, _ptr,
                                    _ptr, _ptr]),
    "n2v_cocl_topn": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _i64, _i64, _i32, _i32, _ptr, _ptr, _i64, _ptr, _i64,
                                _f64, _f64, _f64, _i32, _i32, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "n2v_eccstats_log_table":(C.c_int, [_i64, _ptr]),
    "n2v_eccstats_groups_scratch": (C.c_int64, [_i64]),
    "n2v_eccstats_groups": (C.c_int, [_ptr, _ptr, _i64, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "n2v_eccstats_irg": (C.c_int, [_ptr, _i64, _ptr, _i64, _ptr, _ptr, _ptr]),
    "n2v_eccstats_segsum": (C.c_int, [_ptr, _i64, _ptr, _ptr, _i64, _ptr, _ptr, _i64, _i32, _ptr, _ptr, _ptr, _ptr]),
    "n2v_eccstats_moments_scratch": (C.c_int64, [_i64]),
    "n2v_eccstats_moments": (C.c_int, [_ptr, _i64, _ptr, _ptr, _ptr]),
    "n2v_eccstats_finish": (C.c_int, [_i32, _ptr, _ptr, _ptr, _i64, _ptr, _ptr]),
    "n2v_eccsplit_tile": (C.c_int32, []),
    "n2v_eccsplit_scratch": (C.c_int64, [_i64]),
    "n2v_eccsplit_sort_key": (C.c_int, [_ptr, _i64, _ptr, _ptr]),
    "n2v_eccsplit_mark": (C.c_int, [_ptr, _i64, _i64, _ptr, _ptr]),
    "n2v_eccsplit_select": (C.c_int, [_ptr, _i64, _ptr, _i64, _i32, _ptr, _ptr, _ptr, _ptr]),
    "n2v_eccsplit_first": (C.c_int, [_ptr, _ptr, _i64, _ptr, _ptr, _i64, _i64, _i64, _ptr, _ptr]),
    "n2v_eccsplit_nodes": (C.c_int, [_ptr, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "n2v_eccsplit_ranks": (C.c_int, [_ptr, _ptr, _i64, _ptr, _ptr, _ptr]),
    "n2v_eccsplit_keys": (C.c_int, [_ptr, _i64, _ptr, _ptr, _i64, _i64, _i64, _ptr, _ptr, _i64, _ptr, _ptr]),
    "n2v_eccsplit_pairs": (C.c_int, [_ptr, _ptr, _i64, _ptr, _ptr, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "n2v_eccsplit_fill": (C.c_int, [_ptr, _ptr, _i64, _ptr, _i64, _ptr, _ptr, _ptr, _ptr]),
    "n2v_ecccons_check_i32": (C.c_int, [_ptr, _i64, _i32, _i32, _ptr, _ptr]),
    "n2v_ecccons_check_i64": (C.c_int, [_ptr, _i64, _i64, _i64, _ptr, _ptr]),
    "n2v_ecccons_check_ptr": (C.c_int, [_ptr, _i64, _i64, _ptr, _ptr]),
    "n2v_ecccons_join": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "n2v_ecccons_crosstab": (C.c_int, [_ptr, _ptr, _i64, _i32, _ptr, _ptr, _ptr, _ptr]),
    "n2v_ecccons_profile": (C.c_int, [_ptr, _ptr, _i64, _ptr, _ptr, _i64, _ptr, _i64, _i32, _i32, _ptr, _ptr]),
    "n2v_ecccons_feature_rows": (C.c_int, [_ptr, _ptr, _i64, _i64, _ptr, _i64, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "n2v_ecccons_features": (C.c_int, [_ptr, _i64, _ptr, _ptr, _i64, _i64, _i64, _ptr, _i32, _ptr, _ptr, _i64, _i32, _ptr, _ptr,
                                       _ptr]),
    "n2v_forest_feature_tile": (C.c_int32, [_i32, _i32]),
    "n2v_forest_glog_table": (C.c_int, [_i64, _ptr]),
    "n2v_forest_check_x": (C.c_int, [_ptr, _i64, _ptr, _ptr]),
    "n2v_forest_check_bins": (C.c_int, [_ptr, _i64, _i32, _ptr, _ptr]),
    "n2v_forest_check_classes": (C.c_int, [_ptr, _i64, _i32, _ptr, _ptr]),
    "n2v_forest_check_tree": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _i32, _i64, _i32, _i32, _ptr, _ptr]),
    "n2v_forest_edges": (C.c_int, [_ptr, _i64, _i32, _i32, _ptr, _ptr, _ptr]),
    "n2v_forest_bin": (C.c_int, [_ptr, _i64, _i32, _i32, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "n2v_forest_bootstrap": (C.c_int, [_u64, _i32, _i64, _ptr, _ptr]),
    "n2v_forest_quantise": (C.c_int, [_ptr, _i64, _i32, _ptr, _ptr, _ptr, _ptr]),
    "n2v_forest_feature_keys": (C.c_int, [_u64, _i32, _i32, _i32, _i32, _ptr, _ptr]),
    "n2v_forest_hist": (C.c_int, [_ptr, _i64, _i32, _i32, _i32, _i32, _ptr, _ptr, _i32, _i32, _i64, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "n2v_forest_split": (C.c_int, [_ptr, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _ptr, _i64, _u64, _i32, _i32, _ptr, _i32, _ptr,
                                   _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "n2v_forest_route_flags": (C.c_int, [_ptr, _i64, _i32, _ptr, _ptr, _i32, _i64, _ptr, _ptr, _ptr, _i32, _ptr, _ptr]),
    "n2v_forest_route_scatter": (C.c_int, [_ptr, _ptr, _i32, _i64, _ptr, _ptr, _ptr, _ptr, _i32, _i32, _i32, _i64, _ptr, _ptr, _ptr,
                                           _ptr]),
    "n2v_forest_predict": (C.c_int, [_ptr, _i64, _i32, _ptr, _ptr, _ptr, _ptr, _ptr, _i32, _i32, _i32, _ptr, _ptr]),
    "n2v_forest_argmax": (C.c_int, [_ptr, _i64, _i32, _ptr, _ptr]),
}

_lib = None


class N2VError(RuntimeError):
    pass


def load():
    """Load the HIP library; fail loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise ImportError(
            "libn2v_hip.so not found at %s — build it with `python __graft_entry__.py` "
            "(or `make -C node2vec-by-ecc_amd/csrc`); there is no CPU fallback." % SO_PATH)
    lib = C.CDLL(SO_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != N2V_OK:
        msg = load().n2v_last_error()
        raise N2VError("libn2v_hip error %d: %s" % (rc, msg.decode() if msg else "?"))


def ptr(t):
    """Device (or host) pointer of a torch tensor the caller of this function allocated itself, None -> NULL.  A tensor that
    comes from outside the package goes through tensor() below."""
    if t is None:
        return None
    if not t.is_contiguous():
        raise ValueError("non-contiguous tensor passed to the C-ABI")
    return t.data_ptr()


def call_device(fn, name, t):
    """The device a wrapper's call runs on: that of its first tensor argument `t`, which has to be a GPU tensor.  A CPU
    tensor's address must never reach a kernel.  Reads t.device only."""
    if t is None:
        raise ValueError("%s: %s is required, got None" % (fn, name))
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: %s must be a torch tensor, got %s" % (fn, name, type(t).__name__))
    if t.device.type != "cuda":
        raise ValueError("%s: %s is on %s; the call runs on a GPU and takes device tensors" % (fn, name, t.device))
    return t.device


def _shape_text(shape):
    return "[" + ", ".join("n" if s is None else str(s) for s in shape) + "]"


def tensor(fn, name, t, dtype, device, shape=None, optional=False):
    """The pointer of a caller-supplied tensor after the one check of the wrappers' contract: `t` is a contiguous torch
    tensor of `dtype` on `device` (the device the call runs on), and of `shape` when one is given: an int n is a 1-D
    tensor of n entries, a tuple is the exact shape with None for a free extent, so (None,) is any 1-D tensor.  None is
    NULL where `optional`.  Anything else is a ValueError that names the function `fn` and the argument `name`; a
    non-tensor is a TypeError.  Host work only: dtype, device, dim(), shape, numel() and is_contiguous() are read, nothing
    is launched and nothing synchronises."""
    if t is None:
        if optional:
            return None
        raise ValueError("%s: %s is required, got None" % (fn, name))
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: %s must be a torch tensor, got %s" % (fn, name, type(t).__name__))
    ok = t.dtype == dtype and t.device == device and t.is_contiguous()
    if ok and shape is not None:                                    # written out: this runs on every call of every wrapper
        have = t.shape
        if shape.__class__ is tuple:
            ok = len(have) == len(shape)
            if ok:
                for want, got in zip(shape, have):
                    if want is not None and want != got:
                        ok = False
                        break
        else:
            ok = len(have) == 1 and have[0] == shape
    if not ok:
        if shape is not None and not isinstance(shape, tuple):
            shape = (int(shape),)
        raise ValueError("%s: %s must be a contiguous %s tensor%s on %s, the device the call runs on; got %s%s %s on %s"
                         % (fn, name, str(dtype).replace("torch.", ""), "" if shape is None else " " + _shape_text(shape),
                            device, "" if t.is_contiguous() else "non-contiguous ", str(t.dtype).replace("torch.", ""),
                            _shape_text(tuple(t.shape)), t.device))
    return t.data_ptr()


def stream_ptr(device):
    import torch
    return torch.cuda.current_stream(device).cuda_stream
