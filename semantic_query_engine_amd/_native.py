"""ctypes binding of libsqe.so (include/sqe.h).

The HIP library is the product; there is no CPU fallback.  If ``libsqe.so`` is missing
or does not export a symbol the header declares, importing this module raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SQE_LIB", os.path.join(_HERE, "libsqe.so"))

c_float_p = C.POINTER(C.c_float)
c_i64_p = C.POINTER(C.c_int64)
c_i32_p = C.POINTER(C.c_int32)


class BertCfg(C.Structure):
    _fields_ = [("vocab_size", C.c_int32), ("hidden", C.c_int32), ("layers", C.c_int32),
                ("heads", C.c_int32), ("inter", C.c_int32), ("max_pos", C.c_int32),
                ("type_vocab", C.c_int32), ("ln_eps", C.c_float)]


class Stats(C.Structure):
    _fields_ = [("scan_ms", C.c_double), ("prep_ms", C.c_double), ("select_ms", C.c_double),
                ("add_ms", C.c_double), ("encode_ms", C.c_double), ("cache_ms", C.c_double),
                ("scan_calls", C.c_int64), ("search_calls", C.c_int64), ("scan_rows", C.c_int64),
                ("scan_flops", C.c_int64), ("scan_bytes", C.c_int64), ("uncertified", C.c_int64),
                ("sample_ms", C.c_double), ("i8_collected", C.c_int64), ("i8_rescored", C.c_int64),
                ("i8_overflows", C.c_int64)]


class I8Launch(C.Structure):
    _fields_ = [("rows", C.c_int64), ("tile_stride", C.c_int64), ("dim", C.c_int32), ("B", C.c_int32), ("b_pad", C.c_int32),
                ("k", C.c_int32), ("tile_rows", C.c_int32), ("q_pitch", C.c_int32), ("query_block", C.c_int32),
                ("n_chunks", C.c_int32), ("list_cap", C.c_int32), ("sample_int8", C.c_int32), ("sample_step", C.c_int32),
                ("sample_tiles", C.c_int32), ("sample_chunks", C.c_int32), ("sample_b_pad", C.c_int32), ("sample_m", C.c_int32),
                ("uncertified", C.c_int32), ("pool_cap", C.c_int32), ("kernel", C.c_int32)]


class ScanLaunch(C.Structure):
    _fields_ = [("rows", C.c_int64), ("dim", C.c_int32), ("B", C.c_int32), ("k", C.c_int32), ("kp", C.c_int32), ("bn", C.c_int32),
                ("qblocks", C.c_int32), ("b_pad", C.c_int32), ("n_tiles", C.c_int32), ("n_chunks", C.c_int32),
                ("tiles_per_chunk", C.c_int32), ("ngroups", C.c_int32), ("trig", C.c_int32), ("gshift", C.c_int32),
                ("gshift_k", C.c_int32), ("k_rows", C.c_int32), ("list_cap", C.c_int32), ("exact_cap", C.c_int32),
                ("family", C.c_int32), ("nst", C.c_int32), ("nstb", C.c_int32), ("certified", C.c_int32), ("uncertified", C.c_int32)]


class IndexState(C.Structure):
    _fields_ = [("rows", C.c_int64), ("i8_rows", C.c_int64), ("i8_tile_stride", C.c_int64), ("dim", C.c_int32),
                ("scan_pitch", C.c_int32), ("last_B", C.c_int32), ("last_i8", C.c_int32)]


class DeleteLast(C.Structure):
    _fields_ = [("n_old", C.c_int64), ("n_new", C.c_int64), ("first_pos", C.c_int64), ("block_rows", C.c_int64),
                ("staged_blocks", C.c_int64), ("direct_blocks", C.c_int64), ("staged_rows", C.c_int64), ("direct_rows", C.c_int64),
                ("stage_bytes", C.c_int64)]


class IvfSearchState(C.Structure):
    _fields_ = [("n_assigned", C.c_int64), ("total_tiles", C.c_int64), ("i8_tile_stride", C.c_int64), ("B", C.c_int32),
                ("nprobe", C.c_int32), ("k", C.c_int32), ("kp", C.c_int32), ("max_len", C.c_int32), ("nlist", C.c_int32),
                ("dim", C.c_int32), ("scan_pitch", C.c_int32), ("q8_pitch", C.c_int32), ("coarse", C.c_int32),
                ("list_kernel", C.c_int32), ("grid", C.c_int32), ("split", C.c_int32), ("queued", C.c_int32),
                ("n_units1", C.c_int32), ("n_units4", C.c_int32), ("n_unitsS", C.c_int32), ("n_unitsR", C.c_int32),
                ("sub_batches", C.c_int32), ("fallback", C.c_int32), ("list_cap", C.c_int32), ("persistent", C.c_int32)]


class LexInfo(C.Structure):
    _fields_ = [("documents", C.c_int64), ("postings", C.c_int64), ("n_terms", C.c_int32), ("chunk_rows", C.c_int32),
                ("chunks", C.c_int32), ("rebuilds", C.c_int32), ("avgdl", C.c_double), ("last_rebuild_ms", C.c_double)]


class FieldClause(C.Structure):
    _fields_ = [("field", C.c_int32), ("op", C.c_int32), ("lo", C.c_int64), ("hi", C.c_int64)]


class FieldAgg(C.Structure):
    _fields_ = [("kind", C.c_int32), ("field", C.c_int32), ("size", C.c_int32), ("pad", C.c_int32), ("interval", C.c_int64),
                ("offset", C.c_int64)]


class FieldAggResult(C.Structure):
    _fields_ = [("count", C.c_int64), ("min", C.c_int64), ("max", C.c_int64), ("sum_lo", C.c_int64), ("sum_hi", C.c_int64),
                ("n_buckets", C.c_int64), ("other", C.c_int64)]


class AggRoute(C.Structure):
    _fields_ = [("route", C.c_int32), ("select_blocks", C.c_int32), ("span", C.c_int64), ("slots", C.c_int64),
                ("occupied_blocks", C.c_int32), ("pad", C.c_int32)]


class AggLast(C.Structure):
    _fields_ = [("n_aggs", C.c_int32), ("pad", C.c_int32), ("agg", AggRoute * 8)]


class FieldSort(C.Structure):
    _fields_ = [("field", C.c_int32), ("flags", C.c_int32)]


class SortLast(C.Structure):
    _fields_ = [("slabs", C.c_int32), ("slabs_occupied", C.c_int32), ("merge_levels", C.c_int32), ("fan_in", C.c_int32),
                ("candidates", C.c_int64)]


class WhereLast(C.Structure):
    _fields_ = [("route", C.c_int32), ("depth", C.c_int32), ("first_pass_i8", C.c_int32), ("pad", C.c_int32),
                ("selected", C.c_int64), ("live", C.c_int64), ("swept", C.c_int64)]


class WithinLast(C.Structure):
    _fields_ = [("kind", C.c_int32), ("route", C.c_int32), ("depth", C.c_int32), ("pad", C.c_int32),
                ("selected", C.c_int64), ("live", C.c_int64), ("swept", C.c_int64)]


class EncoderGemm(C.Structure):
    _fields_ = [("family", C.c_int32), ("menu", C.c_int32), ("slices", C.c_int32)]


class EncoderState(C.Structure):
    _fields_ = [("B", C.c_int32), ("S", C.c_int32), ("T", C.c_int32), ("t_pad", C.c_int32), ("mode", C.c_int32),
                ("att_nw", C.c_int32), ("att_nq", C.c_int32), ("pre_slices", C.c_int32), ("pre_stride", C.c_int64),
                ("gemm", EncoderGemm * 4)]


# name -> (restype, argtypes): every symbol include/sqe.h declares
SIGNATURES = {
    "sqe_version": (C.c_int, []),
    "sqe_last_error": (C.c_char_p, []),
    "sqe_create": (C.c_int, [c_i32_p, C.c_int, C.POINTER(C.c_void_p)]),
    "sqe_create_sharded": (C.c_int, [c_i32_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "sqe_group_info": (C.c_int, [C.c_void_p, c_i32_p, c_i32_p, c_i32_p, C.c_int]),
    "sqe_destroy": (None, [C.c_void_p]),
    "sqe_synchronize": (C.c_int, [C.c_void_p]),
    "sqe_stream": (C.c_void_p, [C.c_void_p]),
    "sqe_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "sqe_device_info": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, c_i32_p, c_i64_p]),
    "sqe_index_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "sqe_index_destroy": (None, [C.c_void_p]),
    "sqe_index_reserve": (C.c_int, [C.c_void_p, C.c_int64]),
    "sqe_index_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "sqe_index_add_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "sqe_index_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "sqe_index_count": (C.c_int, [C.c_void_p, c_i64_p]),
    "sqe_index_get_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "sqe_index_delete": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "sqe_index_ids": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "sqe_index_delete_last": (C.c_int, [C.c_void_p, C.POINTER(DeleteLast)]),
    "sqe_index_next_id": (C.c_int, [C.c_void_p, c_i64_p]),
    "sqe_index_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    "sqe_index_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "sqe_index_search_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "sqe_index_search_filtered": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "sqe_index_search_filtered_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                                   C.c_void_p]),
    "sqe_index_search_filtered_each": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                 C.c_void_p, C.c_void_p]),
    "sqe_index_search_filtered_each_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "sqe_index_search_excluding": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                             C.c_void_p, C.c_void_p]),
    "sqe_index_search_excluding_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "sqe_index_range_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sqe_index_range_search_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sqe_index_set_keys": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "sqe_index_get_keys": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "sqe_index_set_field": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64]),
    "sqe_index_get_field": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "sqe_index_field_info": (C.c_int, [C.c_void_p, c_i32_p, c_i64_p]),
    "sqe_index_match_fields": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                         C.c_void_p]),
    "sqe_index_match_fields_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64,
                                                C.c_void_p, C.c_void_p]),
    "sqe_index_search_where": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                                         C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "sqe_index_search_where_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                                                C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "sqe_index_search_where_each": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                              C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sqe_index_search_where_each_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                     C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sqe_index_aggregate_fields": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                             C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sqe_index_aggregate_last": (C.c_int, [C.c_void_p, C.POINTER(AggLast)]),
    "sqe_index_sort_fields": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int,
                                        C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sqe_index_sort_last": (C.c_int, [C.c_void_p, C.POINTER(SortLast)]),
    "sqe_index_where_last": (C.c_int, [C.c_void_p, C.POINTER(WhereLast)]),
    "sqe_where_depth": (C.c_int, [C.c_int, C.c_int64, C.c_int64]),
    # the row-set arguments (clauses, n_clauses, set_values, n_set, allow_ids, n_allow) follow those of the unrestricted call
    "sqe_index_range_search_where": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                               C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sqe_index_range_search_where_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                      C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sqe_index_search_collapsed_where": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                                                   C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sqe_index_search_collapsed_where_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                          C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sqe_index_search_mmr_where": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                             C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sqe_index_search_mmr_where_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                    C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                    C.c_void_p]),
    "sqe_index_within_last": (C.c_int, [C.c_void_p, C.POINTER(WithinLast)]),
    "sqe_index_search_collapsed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sqe_index_search_collapsed_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sqe_index_train": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_uint64]),
    "sqe_index_train_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_uint64]),
    "sqe_index_ivf_export": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "sqe_index_i8_last": (C.c_int, [C.c_void_p, C.POINTER(I8Launch)]),
    "sqe_index_i8_read": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64]),
    "sqe_index_scan_last": (C.c_int, [C.c_void_p, C.POINTER(ScanLaunch)]),
    "sqe_index_scan_read": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64]),
    "sqe_index_state": (C.c_int, [C.c_void_p, C.POINTER(IndexState)]),
    "sqe_index_state_read": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64]),
    "sqe_index_ivf_state": (C.c_int, [C.c_void_p, C.POINTER(IvfSearchState)]),
    "sqe_index_ivf_state_read": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64]),
    "sqe_index_save": (C.c_int, [C.c_void_p, C.c_char_p]),
    "sqe_index_load": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p)]),
    "sqe_merge_topk_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "sqe_cosine_best": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, c_float_p, c_i32_p]),
    "sqe_cosine_all": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "sqe_cache_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "sqe_cache_destroy": (None, [C.c_void_p]),
    "sqe_cache_set_slot": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "sqe_cache_best": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, c_float_p, c_i32_p]),
    "sqe_encoder_create": (C.c_int, [C.c_void_p, C.POINTER(BertCfg), C.POINTER(C.c_void_p)]),
    "sqe_encoder_destroy": (None, [C.c_void_p]),
    "sqe_encoder_load_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, c_i64_p, C.c_int]),
    "sqe_encoder_finalize": (C.c_int, [C.c_void_p]),
    "sqe_tokenizer_create": (C.c_int, [C.c_char_p, C.c_int64, C.POINTER(C.c_void_p)]),
    "sqe_tokenizer_destroy": (None, [C.c_void_p]),
    "sqe_tokenize": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64, C.c_int, c_i32_p, c_i32_p]),
    "sqe_tokenize_batch": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), c_i64_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "sqe_tokenize_pair_batch": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), c_i64_p, C.POINTER(C.c_char_p), c_i64_p, C.c_int, C.c_int,
                                          C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sqe_encoder_labels": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "sqe_encode_pairs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "sqe_encode_pairs_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "sqe_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "sqe_encode_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "sqe_encoder_state": (C.c_int, [C.c_void_p, C.POINTER(EncoderState)]),
    "sqe_encoder_state_read": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64]),
    "sqe_set_profiling": (C.c_int, [C.c_void_p, C.c_int]),
    "sqe_stats": (C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    "sqe_stats_reset": (C.c_int, [C.c_void_p]),
    "sqe_index_search_mmr": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "sqe_index_search_mmr_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
    "sqe_index_search_fused": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                         C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sqe_index_search_fused_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sqe_lex_create": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_void_p)]),
    "sqe_lex_destroy": (None, [C.c_void_p]),
    "sqe_lex_put": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "sqe_lex_delete": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "sqe_lex_count": (C.c_int, [C.c_void_p, c_i64_p]),
    "sqe_lex_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "sqe_lex_search_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "sqe_lex_search_bool": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "sqe_lex_search_bool_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                             C.c_void_p]),
    "sqe_lex_match": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]),
    "sqe_lex_match_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p,
                                       C.c_void_p]),
    "sqe_lex_put_ordered": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "sqe_lex_search_phrase": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                        C.c_void_p]),
    "sqe_lex_search_phrase_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                               C.c_void_p, C.c_void_p]),
    "sqe_lex_match_phrase": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p,
                                       C.c_void_p]),
    "sqe_lex_match_phrase_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64,
                                              C.c_void_p, C.c_void_p]),
    "sqe_lex_info": (C.c_int, [C.c_void_p, C.POINTER(LexInfo)]),
    "sqe_lex_state_read": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64]),
    "sqe_index_search_hybrid": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                          C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sqe_index_search_hybrid_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                 C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sqe_collapse_swept": (C.c_int, [C.c_void_p, c_i64_p]),
    "sqe_exclude_swept": (C.c_int, [C.c_void_p, c_i64_p]),
}

_lib: Optional[C.CDLL] = None


class SqeError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libsqe error {code}: {msg}")
        self.code = code


def load() -> C.CDLL:
    """Load libsqe.so and bind every declared symbol; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C semantic_query_engine_amd/csrc` (hipcc, gfx950). There is no CPU fallback.")
    # A PyTorch-ROCm wheel bundles its own libamdhip64.so.7 / libhsa-runtime64.so.1.  If libsqe.so pulls in the system
    # copies first and torch is imported later, the process holds two HIP runtimes and torch's finds no device
    # (hipErrorNoDevice at its first CUDA call).  With torch loaded first the dynamic linker binds libsqe.so to the
    # copies already in the process (same SONAMEs).  Nothing of torch is used here.
    # A caller that never imports torch (a plain ctypes / NumPy host) can skip the multi-second import: SQE_NO_TORCH_PRELOAD=1.
    import sys
    if "torch" not in sys.modules and os.environ.get("SQE_NO_TORCH_PRELOAD", "0") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        raise SqeError(rc, load().sqe_last_error().decode("utf-8", "replace"))
