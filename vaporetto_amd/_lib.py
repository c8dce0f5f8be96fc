"""ctypes binding of libvaporetto_hip.so (the C ABI declared in include/vaporetto_hip.h).

The library is the product: there is no Python or CPU fallback.  If it has not been built, loading fails
loudly; build it with `python -m vaporetto_amd.build` (or `__graft_entry__.build()`).
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libvaporetto_hip.so")

VPT_OK, VPT_INVALID_MODEL, VPT_INVALID_ARGUMENT, VPT_RUNTIME_ERROR = 0, 1, 2, 3
VPT_FLAG_KYTEA_FULLWIDTH = 1
VPT_FLAG_SPLIT_LINEBREAKS = 1 << 7
VPT_FLAG_LINEBREAKS_FIRST = 1 << 8
VPT_FLAG_CONCAT_GRAPHEMES = 1 << 9
VPT_LISTING_SCORES, VPT_LISTING_TAG_SCORES, VPT_LISTING_TAGGED, VPT_LISTING_NO_NORM_ORDER = 1, 2, 4, 8
VPT_EVAL_TAGS_NONE, VPT_EVAL_TAGS_GOLD, VPT_EVAL_TAGS_PREDICTED = 0, 1, 2


def VPT_FLAG_WSCONST(char_type: int) -> int:
    return 1 << int(char_type)


class ModelInfo(C.Structure):
    _fields_ = [
        ("n_char_ngrams", C.c_uint32), ("n_type_ngrams", C.c_uint32), ("n_dict_words", C.c_uint32),
        ("n_tag_models", C.c_uint32), ("bias", C.c_int32), ("char_window", C.c_uint32), ("type_window", C.c_uint32),
        ("max_pattern_chars", C.c_uint32), ("n_short_entries", C.c_uint32), ("n_long_nodes", C.c_uint32),
        ("type_kind", C.c_uint32), ("device_table_bytes", C.c_uint64), ("hot_table_bytes", C.c_uint64),
        ("packed", C.c_uint32), ("n_displaced", C.c_uint32), ("type_rows", C.c_uint32), ("n_overflow_children", C.c_uint32),
        ("predict_tags", C.c_uint32),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TrainParams(C.Structure):
    _fields_ = [("charw", C.c_uint32), ("charn", C.c_uint32), ("typew", C.c_uint32), ("typen", C.c_uint32), ("dictn", C.c_uint32),
                ("flags", C.c_uint32)]


class TrainStats(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("cg_steps", C.c_uint32), ("gnorm0", C.c_double), ("gnorm", C.c_double),
                ("objective", C.c_double)]


VPT_TRAIN_TAGS = 1
VPT_TRAIN_L1R = 4
VPT_TRAIN_TAGS_L1R = 8
VPT_TRAIN_L1R_LR = 16
VPT_TRAIN_TAGS_L1R_LR = 32
VPT_POSTINGS_MERGE_ORDERED = 1


class PostingsSegment(C.Structure):
    """vpt_postings_segment: the pointers are device pointers for vpt_postings_merge_device, host pointers for vpt_postings_merge"""
    _fields_ = [("d_term_offsets", C.c_void_p), ("d_post_docs", C.c_void_p), ("d_post_tfs", C.c_void_p), ("n_terms", C.c_uint32),
                ("capacity", C.c_uint64)]


class PostingsPositionalSegment(C.Structure):
    """vpt_postings_positional_segment: device pointers for vpt_postings_merge_positional_device, host pointers for vpt_postings_merge_positional"""
    _fields_ = [("d_term_offsets", C.c_void_p), ("d_post_docs", C.c_void_p), ("d_post_tfs", C.c_void_p), ("d_post_first", C.c_void_p),
                ("d_post_positions", C.c_void_p), ("n_terms", C.c_uint32), ("capacity", C.c_uint64), ("capacity_positions", C.c_uint64)]


class TagProblemInfo(C.Structure):
    _fields_ = [("slot", C.c_uint32), ("n_classes", C.c_uint32), ("path", C.c_uint32), ("model", C.c_uint32), ("n_rows", C.c_uint64),
                ("n_features", C.c_uint64), ("nnz", C.c_uint64), ("surface_bytes", C.c_uint64), ("cand_bytes", C.c_uint64),
                ("seconds_setup", C.c_double), ("seconds_solve", C.c_double)]


class TagTrainSummary(C.Structure):
    _fields_ = [("problems_in_kernel", C.c_uint64), ("problems_large", C.c_uint64), ("seconds_in_kernel", C.c_double),
                ("seconds_large", C.c_double), ("seconds_large_solve", C.c_double), ("seconds_construction", C.c_double),
                ("seconds_add_host", C.c_double), ("seconds_construction_host", C.c_double)]


# every symbol include/vaporetto_hip.h declares: name -> (restype, argtypes)
_P = C.c_void_p
SIGNATURES = {
    "vpt_last_error": (C.c_char_p, []),
    "vpt_version": (C.c_char_p, []),
    "vpt_predictor_create": (C.c_int, [_P, C.c_size_t, C.c_int, C.c_int, C.POINTER(_P)]),
    "vpt_predictor_destroy": (None, [_P]),
    "vpt_predictor_save": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "vpt_predictor_load": (C.c_int, [_P, C.c_size_t, C.c_int, C.POINTER(_P)]),
    "vpt_predictor_clone_to_device": (C.c_int, [_P, C.c_int, C.POINTER(_P)]),
    "vpt_predictor_describe": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(_P), C.POINTER(C.c_size_t)]),
    "vpt_predictor_adopt_device": (C.c_int, [_P, C.c_size_t, _P, C.c_size_t, C.c_int, C.POINTER(_P)]),
    "vpt_count_boundaries": (C.c_int, [_P, _P, C.c_size_t, _P]),
    "vpt_predict_batch": (C.c_int, [_P, _P, _P, C.c_size_t, _P, _P, _P]),
    "vpt_predict_batch_flags": (C.c_int, [_P, _P, _P, C.c_size_t, _P, _P, _P, C.c_uint]),
    "vpt_predict_one": (C.c_int, [_P, _P, C.c_size_t, _P, _P, C.POINTER(C.c_size_t)]),
    "vpt_host_alloc": (C.c_int, [C.c_size_t, C.POINTER(_P)]),
    "vpt_host_free": (None, [_P]),
    "vpt_predict_batch_sharded": (C.c_int, [_P, C.c_size_t, _P, _P, C.c_size_t, _P, _P, _P, C.c_uint]),
    "vpt_shard_bounds": (C.c_int, [_P, C.c_size_t, C.c_size_t, _P]),
    "vpt_char_types_batch": (C.c_int, [_P, _P, _P, C.c_size_t, _P, C.c_uint, _P]),
    "vpt_char_types_batch_device": (C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, C.c_uint64, _P, _P]),
    "vpt_predictor_n_tags": (C.c_int, [_P, C.POINTER(C.c_uint32)]),
    "vpt_fill_tags_batch": (C.c_int, [_P, _P, _P, C.c_size_t, _P, _P, _P]),
    "vpt_batch_last_plan": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "vpt_batch_last_text_policy": (C.c_int, [_P, C.POINTER(C.c_uint32)]),
    "vpt_text_policy_for": (C.c_int, [C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "vpt_batch_tag_plan": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    "vpt_predictor_tag_score_stride": (C.c_int, [_P, C.POINTER(C.c_uint32)]),
    "vpt_fill_tags_scores_batch": (C.c_int, [_P, _P, _P, C.c_size_t, _P, _P, C.c_uint, _P, _P, _P]),
    "vpt_fill_tags_scores_batch_device": (C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, C.c_uint64, _P, _P, _P, _P, _P]),
    "vpt_fill_tags_batch_flags": (C.c_int, [_P, _P, _P, C.c_size_t, _P, _P, _P, C.c_uint]),
    "vpt_batch_set_flags": (C.c_int, [_P, C.c_uint]),
    "vpt_write_tokenized_batch": (C.c_int, [_P, _P, _P, C.c_size_t, _P, _P, _P, C.c_uint64, _P]),
    "vpt_predict_write_batch_device": (C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, C.c_uint64, C.c_uint64, _P, _P, _P, C.c_uint64, _P, _P]),
    "vpt_write_tokenized_batch_device": (C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, C.c_uint64, _P, _P, C.c_uint64, _P, _P]),
    "vpt_predictor_max_tag_suffix": (C.c_int, [_P, C.POINTER(C.c_uint32)]),
    "vpt_count_boundaries_device": (C.c_int, [_P, _P, _P, _P, C.c_size_t, _P, _P]),
    "vpt_tokenize_batch": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_uint, C.c_int, _P, C.c_uint64, _P]),
    "vpt_write_tagged_batch": (C.c_int, [_P, _P, _P, C.c_size_t, _P, _P, C.c_uint, _P, C.c_uint64, _P]),
    "vpt_write_tagged_batch_device": (C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, C.c_uint64, _P, _P, _P, C.c_uint64, _P, _P]),
    "vpt_fill_tags_batch_device": (C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, C.c_uint64, _P, _P, _P]),
    "vpt_expand_tags_batch_device": (C.c_int, [_P, _P, C.c_size_t, C.c_uint64, _P, _P]),
    "vpt_token_spans_batch_device": (C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, C.c_uint64, _P, _P, _P, C.c_uint64, _P]),
    "vpt_token_spans_batch": (C.c_int, [_P, _P, _P, C.c_size_t, _P, _P, _P, _P, C.c_uint64]),
    "vpt_token_stream_batch": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_uint, _P, _P, C.c_uint64]),
    "vpt_predictor_n_tag_strings": (C.c_int, [_P, C.POINTER(C.c_uint32)]),
    "vpt_predictor_tag_string": (C.c_int, [_P, C.c_uint32, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    "vpt_token_tags_batch_device": (C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, C.c_uint64, _P, _P, _P, _P, C.c_uint64, _P]),
    "vpt_tag_stop_create": (C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, C.POINTER(_P)]),
    "vpt_tag_stop_destroy": (None, [_P]),
    "vpt_token_filter_tile": (C.c_int, [C.POINTER(C.c_uint32)]),
    "vpt_token_filter_batch_device": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_size_t, C.c_uint64, _P, _P, _P, _P, _P, C.c_uint64, _P]),
    "vpt_token_stream_tagged_batch": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_uint, _P, _P, _P, _P, _P, _P, _P, C.c_uint64]),
    "vpt_vocab_create": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_int32, C.POINTER(_P)]),
    "vpt_vocab_destroy": (None, [_P]),
    "vpt_vocab_info": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "vpt_vocab_surface": (C.c_int, [_P, C.c_uint32, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    "vpt_vocab_tile": (C.c_int, [C.POINTER(C.c_uint32)]),
    "vpt_token_ids_batch_device": (C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, _P, _P, _P, C.c_uint64, C.c_uint, _P, _P]),
    "vpt_token_stream_ids_batch": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_uint, _P, _P, _P, C.c_uint, _P, _P, _P, _P, _P, _P, C.c_uint64]),
    "vpt_vocab_counter_create": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(_P)]),
    "vpt_vocab_counter_destroy": (None, [_P]),
    "vpt_vocab_counter_reset": (C.c_int, [_P]),
    "vpt_vocab_counter_info": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "vpt_vocab_count_batch_device": (C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, _P, _P, _P, C.c_uint64, C.c_uint, _P]),
    "vpt_vocab_counter_finish": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_size_t)]),
    "vpt_token_stream_count_batch": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_uint, _P, _P, _P, C.c_uint]),
    "vpt_postings_batch_device": (C.c_int, [_P, _P, _P, C.c_size_t, _P, C.c_uint64, C.c_uint32, C.c_uint64, _P, _P, _P, C.c_uint64, _P, _P, _P, _P]),
    "vpt_postings_tile": (C.c_int, [C.POINTER(C.c_uint32)]),
    "vpt_token_stream_postings_batch": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_uint, _P, _P, _P, C.c_uint, C.c_uint64, _P, _P, _P, C.c_uint64,
                                                  C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "vpt_postings_merge_device": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_uint32, C.c_uint, _P, _P, _P, C.c_uint64, _P, _P]),
    "vpt_postings_merge_limits": (C.c_int, [C.POINTER(C.c_uint32)]),
    "vpt_postings_merge": (C.c_int, [_P, _P, C.c_size_t, C.c_uint32, C.c_uint, _P, _P, _P, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "vpt_postings_merge_positional_device": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_uint32, C.c_uint, _P, _P, _P, _P, C.c_uint64, _P, C.c_uint64, _P, _P]),
    "vpt_postings_merge_positional": (C.c_int, [_P, _P, C.c_size_t, C.c_uint32, C.c_uint, _P, _P, _P, _P, C.c_uint64, _P, C.c_uint64,
                                                C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "vpt_postings_search_device": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, _P, _P, _P, _P, C.c_uint32, C.c_uint64,
                                             C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint64, _P, _P, _P, _P, _P, _P]),
    "vpt_postings_search_limits": (C.c_int, [C.POINTER(C.c_uint32)]),
    "vpt_postings_search": (C.c_int, [_P, _P, _P, _P, C.c_uint32, C.c_uint64, C.c_uint64, _P, _P, _P, _P, C.c_uint32, C.c_float, C.c_float, C.c_float,
                                      C.c_uint32, _P, _P, _P, _P, _P]),
    "vpt_okapi_idf": (C.c_int, [C.c_uint64, C.c_uint64, C.POINTER(C.c_float)]),
    "vpt_postings_boolean_search_device": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, _P, _P, _P, _P, _P, C.c_uint32,
                                                     C.c_uint64, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint64, _P, _P, _P, _P, _P, _P]),
    "vpt_postings_boolean_search": (C.c_int, [_P, _P, _P, _P, C.c_uint32, C.c_uint64, C.c_uint64, _P, _P, _P, _P, _P, C.c_uint32, C.c_float, C.c_float,
                                              C.c_float, C.c_uint32, _P, _P, _P, _P, _P]),
    "vpt_postings_positions_device": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_uint64, _P, _P, C.c_uint32, _P, C.c_uint64, _P, _P, _P]),
    "vpt_postings_phrase_search_device": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, _P, _P, _P, _P,
                                                    C.c_uint32, C.c_uint64, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint64, _P, _P, _P, _P, _P, _P,
                                                    _P]),
    "vpt_postings_phrase_limits": (C.c_int, [C.POINTER(C.c_uint32)]),
    "vpt_postings_phrase_search": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_uint32, C.c_uint64, C.c_uint64, _P, _P, _P, _P, C.c_uint32, C.c_float, C.c_float,
                                             C.c_float, C.c_uint32, _P, _P, _P, _P, _P, _P]),
    "vpt_token_stream_positional_postings_batch": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_uint, _P, _P, _P, C.c_uint, C.c_uint64, _P, _P, _P, _P, C.c_uint64,
                                                             _P, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "vpt_postings_phrase_lists_device": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, _P, _P,
                                                   C.c_uint32, C.c_uint64, C.c_uint64, _P, _P, _P, C.c_uint64, _P, _P]),
    "vpt_postings_clause_search_device": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint32, C.c_uint64, _P, _P, _P, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64,
                                                    _P, _P, _P, _P, _P, C.c_uint32, C.c_uint64, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint64, _P,
                                                    _P, _P, _P, _P, _P]),
    "vpt_postings_phrase_lists": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_uint32, C.c_uint64, C.c_uint64, _P, _P, C.c_uint32, _P, _P, _P, C.c_uint64, _P]),
    "vpt_postings_clause_search": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_uint32, C.c_uint64, C.c_uint64, _P, _P, _P, _P, _P, _P, C.c_uint32, C.c_float,
                                             C.c_float, C.c_float, C.c_uint32, _P, _P, _P, _P, _P]),
    "vpt_postings_sloppy_phrase_search_device": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, _P, _P, _P,
                                                           _P, _P, C.c_uint32, C.c_uint64, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint64, _P, _P,
                                                           _P, _P, _P, _P, _P]),
    "vpt_postings_sloppy_phrase_lists_device": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, _P, _P,
                                                          _P, C.c_uint32, C.c_uint64, C.c_uint64, _P, _P, _P, C.c_uint64, _P, _P]),
    "vpt_postings_sloppy_phrase_limits": (C.c_int, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "vpt_postings_sloppy_phrase_search": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_uint32, C.c_uint64, C.c_uint64, _P, _P, _P, _P, _P, C.c_uint32, C.c_float,
                                                    C.c_float, C.c_float, C.c_uint32, _P, _P, _P, _P, _P, _P]),
    "vpt_postings_sloppy_phrase_lists": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_uint32, C.c_uint64, C.c_uint64, _P, _P, _P, C.c_uint32, _P, _P, _P,
                                                   C.c_uint64, _P]),
    "vpt_postings_sloppy_clause_search": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_uint32, C.c_uint64, C.c_uint64, _P, _P, _P, _P, _P, _P, _P, C.c_uint32,
                                                    C.c_float, C.c_float, C.c_float, C.c_uint32, _P, _P, _P, _P, _P]),
    "vpt_concat_graphemes_batch": (C.c_int, [_P, _P, _P, C.c_size_t, _P, C.c_uint, _P]),
    "vpt_concat_graphemes_batch_device": (C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, C.c_uint64, _P, _P]),
    "vpt_concat_graphemes_tile": (C.c_int, [C.POINTER(C.c_uint32)]),
    "vpt_pattern_tagger_create": (C.c_int, [_P, _P, _P, C.c_size_t, _P, _P, _P, _P, C.POINTER(_P)]),
    "vpt_pattern_tagger_destroy": (None, [_P]),
    "vpt_pattern_tagger_n_tags": (C.c_int, [_P, C.POINTER(C.c_uint32)]),
    "vpt_pattern_tagger_tag": (C.c_int, [_P, C.c_uint32, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    "vpt_pattern_tagger_max_tag_suffix": (C.c_int, [_P, C.POINTER(C.c_uint32)]),
    "vpt_pattern_tagger_info": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "vpt_pattern_tagger_tile": (C.c_int, [C.POINTER(C.c_uint32)]),
    "vpt_batch_set_pattern_tagger": (C.c_int, [_P, _P]),
    "vpt_fill_tags_batch_rules": (C.c_int, [_P, _P, _P, C.c_size_t, _P, _P, _P, C.c_uint, _P]),
    "vpt_write_tagged_batch_rules": (C.c_int, [_P, _P, _P, C.c_size_t, _P, _P, C.c_uint, _P, C.c_uint64, _P, _P]),
    "vpt_tokenize_batch_rules": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_uint, C.c_int, _P, C.c_uint64, _P, _P]),
    "vpt_predictor_max_tag_listing": (C.c_int, [_P, C.POINTER(C.c_uint32)]),
    "vpt_predict_listing_batch": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_uint, C.c_uint, _P, _P, _P, C.c_uint64, _P]),
    "vpt_predict_listing_batch_device": (C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, C.c_uint64, C.c_uint64, _P, _P, C.c_uint, _P, C.c_uint64, _P, _P]),
    "vpt_parse_tokenized_batch": (C.c_int, [_P, _P, C.c_size_t, _P, _P, _P, _P, _P, _P, _P, _P]),
    "vpt_parse_tokenized_batch_device": (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.c_uint64, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "vpt_parse_partial_batch": (C.c_int, [_P, _P, C.c_size_t, _P, _P, _P, _P, _P, _P, _P, _P]),
    "vpt_parse_partial_batch_device": (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.c_uint64, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "vpt_write_partial_batch": (C.c_int, [_P, _P, C.c_size_t, _P, _P, _P, _P, _P, _P, _P, C.c_uint64, _P]),
    "vpt_write_partial_batch_device": (C.c_int, [_P, _P, _P, _P, C.c_size_t, _P, _P, _P, _P, _P, _P, _P, C.c_uint64, _P, _P]),
    "vpt_evaluate_labels_batch_device": (C.c_int, [_P, _P, _P, C.c_size_t, _P, _P, _P, _P, _P, _P, C.c_int, _P, _P]),
    "vpt_evaluate_batch": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_uint, C.c_int, _P]),
    "vpt_batch_create": (C.c_int, [_P, C.POINTER(_P)]),
    "vpt_batch_destroy": (None, [_P]),
    "vpt_predict_batch_device": (C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, C.c_uint64, C.c_uint64, _P, _P, _P]),
    "vpt_batch_sync": (C.c_int, [_P]),
    "vpt_batch_set_max_sentence_chars": (C.c_int, [_P, C.c_uint64]),
    "vpt_batch_set_timing": (C.c_int, [_P, C.c_int]),
    "vpt_batch_kernel_ms": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]),
    "vpt_batch_kernel_times": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "vpt_batch_phase_cycles": (C.c_int, [_P, C.POINTER(C.c_uint64 * 8)]),
    "vpt_batch_node_reads": (C.c_int, [_P, C.POINTER(C.c_uint64 * 8)]),
    "vpt_model_inspect": (C.c_int, [_P, C.c_size_t, C.c_int, C.POINTER(ModelInfo)]),
    "vpt_model_read_len": (C.c_int, [_P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "vpt_predictor_info": (C.c_int, [_P, C.POINTER(ModelInfo)]),
    "vpt_trainer_create": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_int, C.POINTER(_P)]),
    "vpt_trainer_destroy": (None, [_P]),
    "vpt_trainer_add_batch": (C.c_int, [_P, _P, _P, C.c_size_t, _P, C.c_uint]),
    "vpt_trainer_add_batch_device": (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.c_uint64, _P, C.c_uint, _P]),
    "vpt_trainer_n_features": (C.c_int, [_P, C.POINTER(C.c_size_t)]),
    "vpt_trainer_csr": (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "vpt_trainer_train": (C.c_int, [_P, _P, C.c_int, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "vpt_trainer_model": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "vpt_trainer_weights": (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "vpt_trainer_last_stats": (C.c_int, [_P, _P]),
    "vpt_trainer_add_tagged_batch": (C.c_int, [_P, _P, _P, C.c_size_t, _P, _P, _P, _P, _P, C.c_uint64, C.c_uint64, C.c_uint]),
    "vpt_trainer_add_tagged_batch_device": (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.c_uint64, _P, _P, _P, _P, _P, C.c_uint64, C.c_uint64,
                                                      C.c_uint, _P]),
    "vpt_trainer_set_tag_dictionary": (C.c_int, [_P, _P, _P, C.c_size_t, _P, _P, _P]),
    "vpt_trainer_set_tag_path": (C.c_int, [_P, C.c_int]),
    "vpt_trainer_n_tag_problems": (C.c_int, [_P, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "vpt_trainer_tag_problem": (C.c_int, [_P, C.c_size_t, _P, _P, _P, _P, _P, _P, _P, _P]),
    "vpt_trainer_tag_weights": (C.c_int, [_P, C.c_size_t, _P, C.c_size_t, _P]),
    "vpt_trainer_tag_summary": (C.c_int, [_P, _P]),
}

_lib = None


def _init_torch_hip_first():
    """PyTorch wheels bundle their own libamdhip64/libhsa-runtime64 (different soname from /opt/rocm's, which
    this library links).  Two HIP runtimes can share a process only if torch's initialises first, so when torch
    is importable and sees a GPU, let it.  Torch is never used for compute here."""
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except ImportError:
        pass


def load():
    """Loads the shared library; raises if it is missing (no fallback)."""
    global _lib
    if _lib is None:
        _init_torch_hip_first()
        if not os.path.exists(LIB_PATH):
            raise OSError("%s is missing: build it with `python -m vaporetto_amd.build` "
                          "(there is no CPU or Python fallback)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def last_error() -> str:
    return load().vpt_last_error().decode("utf-8", "replace")
