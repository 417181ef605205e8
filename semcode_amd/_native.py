"""ctypes binding of libsemcode_hip.so (include/semcode_hip.h).

This is the only place Python touches the C ABI.  There is no CPU fallback: if the shared
library is missing, or no MI355X is visible when a runtime is created, the error is raised
to the caller (the seams in embeddings/ and storage/ let it propagate as an ordinary
exception, which IndexerService / SemanticSearchPipeline already catch --
reference src/semcode/services/indexer.py:57-63, src/semcode/rag/pipeline.py:95-110).
"""
from __future__ import annotations

import ctypes as C
import sys
import threading
from pathlib import Path

import numpy as np

LIB_PATH = Path(__file__).resolve().parent / "_lib" / "libsemcode_hip.so"

METRICS = {"IP": 0, "L2": 1, "COSINE": 2}
KINDS = {"FLAT": 0, "IVF_FLAT": 1}


class ScError(RuntimeError):
    """A libsemcode_hip call returned a negative sc_status."""

    def __init__(self, status: int, message: str):
        super().__init__(f"libsemcode_hip error {status}: {message}")
        self.status = status


class _Cfg(C.Structure):
    _fields_ = [("device", C.c_int32), ("stream", C.c_void_p), ("flags", C.c_int32)]


class EncoderCfg(C.Structure):
    _fields_ = [("vocab", C.c_int32), ("hidden", C.c_int32), ("layers", C.c_int32), ("heads", C.c_int32), ("ffn", C.c_int32),
                ("max_pos", C.c_int32), ("type_vocab", C.c_int32), ("ln_eps", C.c_float), ("normalize", C.c_int32),
                ("synth_seed", C.c_uint64), ("pos_type", C.c_int32), ("ffn_type", C.c_int32), ("rope_theta", C.c_float),
                ("arch", C.c_int32), ("local_window", C.c_int32), ("global_every", C.c_int32), ("rope_theta_local", C.c_float),
                ("kv_heads", C.c_int32)]

    # The fields above are sc_encoder_cfg as it stood when kv_heads was appended; what later models append lives in EncoderCfgFull, the
    # whole struct.  The library reads and writes sizeof(sc_encoder_cfg) bytes through every sc_encoder_cfg pointer (sc_encoder_info
    # fills all of it), so an object of the shorter layout must never reach it: constructing EncoderCfg gives the whole struct.
    # The declared fields end where the struct ended when qk_norm was appended; the object always owns all of sizeof(sc_encoder_cfg) bytes,
    # zeroed (EncoderCfgFull.CFG_BYTES: all-zero tail fields mean the behaviour without them).
    def __new__(cls, *args, **kw):
        real = EncoderCfgFull if cls is EncoderCfg else cls
        return real.from_buffer(bytearray(real.CFG_BYTES))


class EncoderCfgFull(EncoderCfg):
    """sc_encoder_cfg: EncoderCfg's fields, then head_dim and qk_norm (arch 2: Qwen3-Embedding, Qwen2.5-1.5B).  The two fields the T5
    encoder appended (arch 3: rel_buckets, rel_max_distance) lie behind the declared ones, in the object's own CFG_BYTES buffer, and are
    read and written through the properties below; keyword arguments reach them as they reach a declared field."""
    _fields_ = [("head_dim", C.c_int32), ("qk_norm", C.c_int32)]
    TAIL_FIELDS = ("rel_buckets", "rel_max_distance")  # int32 each, behind qk_norm in include/semcode_hip.h (tests/test_t5.py checks both against it)
    CFG_BYTES = 88 + 4 * len(TAIL_FIELDS)  # sizeof(sc_encoder_cfg)

    def _tail(self, name):
        return C.c_int32.from_address(C.addressof(self) + 88 + 4 * self.TAIL_FIELDS.index(name))

    rel_buckets = property(lambda self: self._tail("rel_buckets").value, lambda self, v: setattr(self._tail("rel_buckets"), "value", int(v)))
    rel_max_distance = property(lambda self: self._tail("rel_max_distance").value, lambda self, v: setattr(self._tail("rel_max_distance"), "value", int(v)))


class ScoreHead(C.Structure):
    """sc_score_head: the score head of an arch 1 (kind 1) or arch 2 (kind 2) reranker; the pointers are host f32 arrays the library copies."""
    _fields_ = [("kind", C.c_int32), ("pooling", C.c_int32), ("num_labels", C.c_int32), ("norm_eps", C.c_float),
                ("dense_w", C.c_void_p), ("dense_b", C.c_void_p), ("norm_g", C.c_void_p), ("norm_b", C.c_void_p), ("cls_w", C.c_void_p), ("cls_b", C.c_void_p)]


_lib = None
_lib_lock = threading.Lock()

_f32p = C.POINTER(C.c_float)
_i64p = C.POINTER(C.c_int64)

# name -> (restype, argtypes): exactly the entry points include/semcode_hip.h declares
SIGNATURES = {
    "sc_version": (C.c_char_p, []),
    "sc_last_error": (C.c_int32, [C.c_char_p, C.c_size_t]),
    "sc_runtime_create": (C.c_int32, [C.POINTER(_Cfg), C.POINTER(C.c_void_p)]),
    "sc_runtime_destroy": (C.c_int32, [C.c_void_p]),
    "sc_runtime_set_stream": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "sc_runtime_synchronize": (C.c_int32, [C.c_void_p]),
    "sc_runtime_device_info": (C.c_int32, [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "sc_runtime_set_profiling": (C.c_int32, [C.c_void_p, C.c_int32]),
    "sc_runtime_profile_read": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "sc_runtime_profile_reset": (C.c_int32, [C.c_void_p]),
    "sc_synth_fill_dev": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_uint64, C.c_int64]),
    "sc_encoder_blob_bytes": (C.c_int32, [C.POINTER(EncoderCfg), C.POINTER(C.c_int64)]),
    "sc_encoder_create": (C.c_int32, [C.c_void_p, C.POINTER(EncoderCfg), C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "sc_encoder_destroy": (C.c_int32, [C.c_void_p]),
    "sc_encoder_set_path": (C.c_int32, [C.c_void_p, C.c_int32]),
    "sc_encoder_set_pooling": (C.c_int32, [C.c_void_p, C.c_int32]),
    "sc_encoder_get_pooling": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int32)]),
    "sc_encoder_info": (C.c_int32, [C.c_void_p, C.POINTER(EncoderCfg)]),
    "sc_encoder_embed_ids": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "sc_encoder_embed_ids_dev": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "sc_encoder_embed_ids_into": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sc_encoder_embed_ids_into_async": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "sc_encoder_wait": (C.c_int32, [C.c_void_p]),
    "sc_encoder_packed_rows": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]),
    "sc_encoder_embed_packed": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "sc_encoder_set_output_proj": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]),
    "sc_encoder_out_dim": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int32)]),
    "sc_diag_output_proj": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "sc_encoder_set_pair_head": (C.c_int32, [C.c_void_p] * 5 + [C.c_int32]),
    "sc_encoder_score_pairs": (C.c_int32, [C.c_void_p] * 4 + [C.c_int32, C.c_void_p, C.c_void_p]),
    "sc_encoder_set_score_head": (C.c_int32, [C.c_void_p, C.POINTER(ScoreHead)]),
    "sc_encoder_score_seqs": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "sc_encoder_set_token_head": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32]),
    "sc_encoder_embed_tokens": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "sc_encoder_embed_tokens_into": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "sc_encoder_score_late": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 3
                              + [C.c_int32, C.c_void_p]),
    "sc_diag_maxsim": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 3
                       + [C.c_int32, C.c_int32, C.c_void_p]),
    "sc_diag_maxsim_host": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 3 + [C.c_int32, C.c_int32, C.c_void_p]),
    "sc_diag_score_head": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(ScoreHead), C.c_void_p]),
    "sc_diag_embed_pairs": (C.c_int32, [C.c_void_p, C.c_int32] + [C.c_void_p] * 3 + [C.c_int32] * 5 + [C.c_void_p] * 5 + [C.c_float, C.c_int32, C.c_int32,
                                                                                                                       C.c_void_p, C.c_void_p]),
    "sc_diag_pair_head": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 4 + [C.c_int32, C.c_void_p]),
    "sc_encoder_embed_packed_into": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sc_encoder_embed_packed_into_async": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "sc_tokenizer_create": (C.c_int32, [C.c_char_p, C.c_size_t, C.c_int32, C.POINTER(C.c_void_p)]),
    "sc_tokenizer_destroy": (C.c_int32, [C.c_void_p]),
    "sc_tokenizer_info": (C.c_int32, [C.c_void_p] + [C.POINTER(C.c_int32)] * 5),
    "sc_tokenizer_encode": (C.c_int32, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]),
    "sc_diag_gemm_bf16": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "sc_diag_gemm_bf16_ex": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_void_p, C.c_void_p]),
    "sc_diag_gemm_path": (C.c_int32, [C.c_int32] * 5 + [C.c_void_p]),
    "sc_diag_gemm_splitk": (C.c_int32, [C.c_int32] * 4),
    "sc_diag_gemm_bench": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double)]),
    "sc_diag_gemm_trace": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64]),
    "sc_diag_set_option": (C.c_int32, [C.c_char_p, C.c_int32]),
    "sc_diag_gemm_i8": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "sc_diag_encoder_read": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t]),
    "sc_diag_attention_run": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),  # (rt, DiagAttn*, qkv, out)
    "sc_diag_rope": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float]),
    "sc_diag_rel_buckets": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "sc_diag_ffn_act": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "sc_diag_fold_ln": (C.c_int32, [C.c_void_p] * 5 + [C.c_int32, C.c_int32] + [C.c_void_p] * 3),
    "sc_diag_gemm_strip": (C.c_int32, [C.c_int32] * 4),
    "sc_diag_gemm_lna": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 5 + [C.c_float, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_float, C.c_int32, C.c_void_p, C.c_void_p]),
    "sc_diag_gemm_resln": (C.c_int32, [C.c_void_p, C.c_int32] + [C.c_void_p] * 6 + [C.c_float, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "sc_diag_layernorm": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]),
    "sc_diag_qknorm_rope": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p,
                                         C.c_float]),
    "sc_diag_rmsnorm": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_float, C.c_void_p]),
    "sc_diag_mean_pool": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "sc_diag_mean_pool_ln": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                                         C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "sc_diag_embed": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 5 +
                                 [C.c_float, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "sc_index_create": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_void_p)]),
    "sc_index_destroy": (C.c_int32, [C.c_void_p]),
    "sc_index_info": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "sc_index_reserve": (C.c_int32, [C.c_void_p, C.c_int64]),
    "sc_index_add": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    "sc_index_overwrite": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "sc_index_put_rows": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "sc_index_put_rows_dev": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "sc_index_delete_rows": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    "sc_index_last_delete_stats": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "sc_index_get_rows": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "sc_index_fill_synthetic": (C.c_int32, [C.c_void_p, C.c_int64, C.c_uint64, C.c_int64]),
    "sc_index_fill_synthetic_clustered": (C.c_int32, [C.c_void_p, C.c_int64, C.c_uint64, C.c_int64, C.c_int32, C.c_float]),
    "sc_index_release_scratch": (C.c_int32, [C.c_void_p]),
    "sc_index_search": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "sc_index_search_dev": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "sc_index_search_masked": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "sc_index_search_masked_dev": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "sc_index_last_mask_stats": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "sc_index_set_groups": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    "sc_index_search_grouped": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "sc_index_search_grouped_dev": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "sc_index_last_group_stats": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "sc_index_search_mmr": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "sc_index_search_mmr_dev": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "sc_index_last_mmr_stats": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "sc_diag_mmr_select_host": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p]),
    "sc_lex_terms": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "sc_index_set_terms": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p]),
    "sc_index_drop_terms": (C.c_int32, [C.c_void_p]),
    "sc_index_lex_stats": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p]),
    "sc_index_search_lexical": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_int64,
                                            C.c_void_p, C.c_void_p]),
    "sc_index_search_lexical_dev": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_int64,
                                                C.c_void_p, C.c_void_p]),
    "sc_index_search_hybrid": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float,
                                           C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "sc_index_search_hybrid_dev": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float,
                                               C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "sc_index_last_lex_stats": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "sc_diag_lex_score_host": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "sc_diag_rrf_host": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "sc_index_put_tokens": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "sc_index_put_tokens_dev": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "sc_index_reserve_tokens": (C.c_int32, [C.c_void_p, C.c_int64]),
    "sc_index_compact_tokens": (C.c_int32, [C.c_void_p]),
    "sc_index_get_tokens": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]),
    "sc_index_token_stats": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int64)]),
    "sc_index_drop_tokens": (C.c_int32, [C.c_void_p]),
    "sc_index_rerank_late": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "sc_index_search_late": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "sc_diag_late_search_host": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                             C.c_void_p]),
    "sc_diag_round_bf16": (C.c_int32, [C.c_void_p, C.c_int64, C.c_void_p]),
    "sc_index_train": (C.c_int32, [C.c_void_p, C.c_int32, C.c_uint64]),
    "sc_index_ivf_assignments": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "sc_index_set_ivf": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]),
    "sc_index_assign_lists": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32]),
    "sc_index_ivf_info": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]),
    "sc_index_set_search_mode": (C.c_int32, [C.c_void_p, C.c_int32]),
    "sc_index_last_search_stats": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "sc_index_set_coarse_stage": (C.c_int32, [C.c_void_p, C.c_int32]),
    "sc_index_last_coarse_stats": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "sc_index_last_collect_stats": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "sc_index_last_wide": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int32)]),
    "sc_index_last_tail_rows": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int64)]),
    "sc_index_last_probe_stats": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "sc_diag_ivf_plan": (C.c_int32, [C.c_char_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                     C.c_int64, C.POINTER(C.c_int64)]),
    "sc_diag_ivf_exact_path": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "sc_diag_encoder_plan": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32] + [C.c_int32] * 8 + [C.c_void_p, C.c_int64,
                                         C.POINTER(C.c_int64)]),
    "sc_diag_encoder_plan_keep": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64,
                                              C.POINTER(C.c_int64)]),
    "sc_comm_unique_id": (C.c_int32, [C.c_void_p, C.c_size_t]),
    "sc_comm_create": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "sc_comm_destroy": (C.c_int32, [C.c_void_p]),
    "sc_comm_info": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "sc_comm_rccl_version": (C.c_int32, [C.POINTER(C.c_int32)]),
    "sc_comm_allgather_topk": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "sc_comm_broadcast": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32]),
    "sc_index_search_sharded": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "sc_index_search_sharded_dev": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "sc_index_train_sharded": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "sc_comm_allreduce_max": (C.c_int32, [C.c_void_p, C.POINTER(C.c_double)]),
    "sc_topk_merge_host": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}


def lib() -> C.CDLL:
    """Load the shared library once; raise loudly when it has not been built."""
    global _lib
    with _lib_lock:
        if _lib is None:
            if not LIB_PATH.exists():
                raise RuntimeError(
                    f"{LIB_PATH} is missing: build it with `python -m semcode_amd.csrc.build` "
                    "(needs hipcc); semcode_amd has no CPU fallback."
                )
            # PyTorch wheels bundle their own libamdhip64 / libhsa-runtime64 under the system library's sonames, and the
            # copy that is loaded first serves the whole process.  With ours first, a later torch.cuda call in the same
            # process (torch.distributed in bench.py / storage.sharded, device tensors handed to the *_dev entry points)
            # fails with "No HIP GPUs are available"; so where torch is installed it is loaded first.  The library itself
            # never calls into torch.
            try:
                import torch  # noqa: F401
            except Exception:  # pragma: no cover - torch is optional for the library
                pass
            handle = C.CDLL(str(LIB_PATH))
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(handle, name)  # AttributeError if the .so lacks a declared symbol
                fn.restype = res
                fn.argtypes = args
            _lib = handle
    return _lib


def _check(status: int) -> None:
    if status != 0:
        buf = C.create_string_buffer(512)
        lib().sc_last_error(buf, 512)
        raise ScError(status, buf.value.decode("utf-8", "replace"))


def pack_allow(allow, rows: int) -> np.ndarray:
    """The bitset of a masked search as uint32 words (bit r & 31 of word r >> 5 = row r may be returned): a uint32 array is taken as
    the words themselves, a boolean array must have one entry per row and is packed."""
    a = np.asarray(allow)
    if a.dtype == np.bool_:
        if a.shape != (rows,):
            raise ValueError(f"a boolean mask must have one entry per row ({rows}), got shape {a.shape}")
        bits = np.packbits(a, bitorder="little")
        words = np.zeros((rows + 31) // 32 * 4, dtype=np.uint8)
        words[: bits.size] = bits
        return words.view("<u4")
    if a.dtype != np.uint32 or a.ndim != 1:
        raise ValueError("allow must be a 1-d uint32 word array or a boolean array with one entry per row")
    return np.ascontiguousarray(a)


def _result_arrays(Q: int, k: int) -> "tuple[np.ndarray, np.ndarray]":
    """The (dist [Q, k] f32, rows [Q, k] i64) a host-pointer search writes."""
    return np.empty((Q, k), dtype=np.float32), np.empty((Q, k), dtype=np.int64)


LEX_MAX_QTERMS = 32   # terms of one lexical query (csrc/lex_rule.h)
LEX_DF_SIZE = 65536   # entries of the df table
LEX_PAD = 0xFFFF      # the padding slot of a term row


def lex_terms(texts, T: int = 128) -> "tuple[np.ndarray, np.ndarray]":
    """The term rows of these texts (sc_lex_terms; no GPU): (terms [n, T] uint16 sorted ascending and padded with 0xFFFF, dl [n] int32).
    str entries are taken as UTF-8, bytes as they are."""
    raw = [t.encode("utf-8") if isinstance(t, str) else bytes(t) for t in texts]
    n = len(raw)
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(r) for r in raw], out=offsets[1:])
    blob = np.frombuffer(b"".join(raw) or b"\0", dtype=np.uint8)
    terms = np.empty((n, int(T)), dtype=np.uint16)
    counts = np.empty(n, dtype=np.int32)
    _check(lib().sc_lex_terms(blob.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p), n, int(T), terms.ctypes.data_as(C.c_void_p),
                              counts.ctypes.data_as(C.c_void_p)))
    return terms, counts


def diag_lex_score_host(terms, qterms, qweights, k1: float, b: float, avgdl: float) -> "tuple[np.ndarray, np.ndarray]":
    """The score rule of csrc/lex_rule.h on the CPU (sc_diag_lex_score_host): terms [n, T], one query -> (score [n] f32, hit [n] bool)."""
    t = np.ascontiguousarray(terms, dtype=np.uint16)
    qt = np.ascontiguousarray(qterms, dtype=np.uint16).reshape(-1)
    qw = np.ascontiguousarray(qweights, dtype=np.float32).reshape(-1)
    score = np.empty(t.shape[0], dtype=np.float32)
    hit = np.empty(t.shape[0], dtype=np.uint8)
    _check(lib().sc_diag_lex_score_host(t.ctypes.data_as(C.c_void_p), t.shape[0], t.shape[1], qt.ctypes.data_as(C.c_void_p), qw.ctypes.data_as(C.c_void_p), qt.shape[0],
                                        float(k1), float(b), float(avgdl), score.ctypes.data_as(C.c_void_p), hit.ctypes.data_as(C.c_void_p)))
    return score, hit.astype(bool)


def diag_rrf_host(dense_rows, lex_rows, k: int, c: int = 60, dense_weight: float = 1.0, lexical_weight: float = 1.0) -> "tuple[np.ndarray, np.ndarray]":
    """The fusion rule of csrc/lex_rule.h on the CPU (sc_diag_rrf_host): two best-first row lists [F] (-1 = padding) -> (score [k], rows [k])."""
    d = np.ascontiguousarray(dense_rows, dtype=np.int64).reshape(-1)
    l = np.ascontiguousarray(lex_rows, dtype=np.int64).reshape(-1)
    if d.shape != l.shape:
        raise ValueError("the two lists must have one length")
    score = np.empty(k, dtype=np.float32)
    rows = np.empty(k, dtype=np.int64)
    _check(lib().sc_diag_rrf_host(d.ctypes.data_as(C.c_void_p), l.ctypes.data_as(C.c_void_p), d.shape[0], int(k), int(c), float(dense_weight), float(lexical_weight),
                                  score.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p)))
    return score, rows


TOKEN_FORMATS = {"f32": 0, "bf16": 1}  # storage of the token store (csrc/late_rule.h)


def pack_token_lists(token_vectors) -> "tuple[np.ndarray, np.ndarray]":
    """Ragged token vectors as (counts [n] int32, vecs [sum counts, W] f32): a pair (counts, vecs) is checked and passed on, a sequence of
    [n_i, W] arrays (None or empty: no tokens) is concatenated."""
    if isinstance(token_vectors, tuple) and len(token_vectors) == 2 and np.ndim(token_vectors[0]) == 1 and np.ndim(token_vectors[1]) == 2:
        counts = np.ascontiguousarray(token_vectors[0], dtype=np.int32)
        vecs = np.ascontiguousarray(token_vectors[1], dtype=np.float32)
        if int(counts.sum()) != vecs.shape[0]:
            raise ValueError(f"counts sum to {int(counts.sum())}, vecs has {vecs.shape[0]} rows")
        return counts, vecs
    parts = [None if t is None else np.ascontiguousarray(t, dtype=np.float32) for t in token_vectors]
    real = [p for p in parts if p is not None and p.size]
    if any(p.ndim != 2 for p in real) or len({p.shape[1] for p in real}) > 1:
        raise ValueError("every entry must be a [n_i, W] float array of one W")
    counts = np.array([0 if p is None or not p.size else p.shape[0] for p in parts], dtype=np.int32)
    vecs = np.concatenate(real, axis=0) if real else np.empty((0, 0), dtype=np.float32)
    return counts, np.ascontiguousarray(vecs)


def pack_questions(questions) -> "tuple[np.ndarray, np.ndarray]":
    """(Q [sum nq, W] f32, q_off [Bq + 1] int32) of a batch of questions' token vectors (see pack_token_lists for the forms; a pair is
    (Q, q_off) here)."""
    if isinstance(questions, tuple) and len(questions) == 2 and np.ndim(questions[0]) == 2 and np.ndim(questions[1]) == 1:
        return np.ascontiguousarray(questions[0], dtype=np.float32), np.ascontiguousarray(questions[1], dtype=np.int32)
    counts, vecs = pack_token_lists(list(questions))
    q_off = np.zeros(counts.shape[0] + 1, dtype=np.int32)
    np.cumsum(counts, out=q_off[1:])
    return vecs, q_off


def diag_late_search_host(questions, docs, k: int, allow=None) -> "tuple[np.ndarray, np.ndarray]":
    """sc_index_search_late on the CPU (sc_diag_late_search_host; no GPU): docs as Index.put_tokens takes them -> (score [Bq, k],
    rows [Bq, k]), rows without a row_base."""
    Q, q_off = pack_questions(questions)
    counts, D = pack_token_lists(docs)
    n = counts.shape[0]
    d_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=d_off[1:])
    W = Q.shape[1]
    if D.shape[0] and D.shape[1] != W:
        raise ValueError("questions and documents must have one W")
    Bq = q_off.shape[0] - 1
    score, rows = _result_arrays(Bq, k)
    words = None if allow is None else pack_allow(allow, n)
    if words is not None and words.size == 0:
        words = np.zeros(1, dtype=np.uint32)
    _check(lib().sc_diag_late_search_host(Q.ctypes.data_as(C.c_void_p), q_off.ctypes.data_as(C.c_void_p), Bq, D.ctypes.data_as(C.c_void_p) if D.shape[0] else None,
                                          d_off.ctypes.data_as(C.c_void_p), n, W, int(k), None if words is None else words.ctypes.data_as(C.c_void_p),
                                          0 if words is None else words.shape[0], score.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p)))
    return score, rows


def diag_round_bf16(x) -> np.ndarray:
    """What the token store keeps for x at fmt 'bf16': every float rounded to nearest-even on its upper 16 bits (sc_diag_round_bf16)."""
    a = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty_like(a)
    _check(lib().sc_diag_round_bf16(a.ctypes.data_as(C.c_void_p), a.size, out.ctypes.data_as(C.c_void_p)))
    return out


def _as_f32(a, shape_last: int | None = None) -> np.ndarray:
    arr = np.ascontiguousarray(a, dtype=np.float32)
    if shape_last is not None and (arr.ndim != 2 or arr.shape[1] != shape_last):
        raise ValueError(f"expected a [n, {shape_last}] float array, got shape {arr.shape}")
    return arr


class Runtime:
    """One per process / GPU (sc_runtime)."""

    def __init__(self, device: int = 0, stream: int | None = None):
        self._h = C.c_void_p()
        cfg = _Cfg(device=device, stream=C.c_void_p(stream) if stream else None, flags=0)
        _check(lib().sc_runtime_create(C.byref(cfg), C.byref(self._h)))
        self.device = device

    def close(self) -> None:
        if self._h:
            lib().sc_runtime_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover - best effort
        try:
            if not sys.is_finalizing():  # at interpreter shutdown handle order is arbitrary: leave it to process exit
                self.close()
        except Exception:
            pass

    @property
    def handle(self) -> C.c_void_p:
        if not self._h:
            raise RuntimeError("runtime is closed")
        return self._h

    def set_stream(self, stream: int) -> None:
        _check(lib().sc_runtime_set_stream(self.handle, C.c_void_p(stream)))

    def synchronize(self) -> None:
        _check(lib().sc_runtime_synchronize(self.handle))

    def device_info(self) -> dict:
        name = C.create_string_buffer(256)
        cus, hbm = C.c_int32(), C.c_int64()
        _check(lib().sc_runtime_device_info(self.handle, name, 256, C.byref(cus), C.byref(hbm)))
        return {"name": name.value.decode(), "cus": cus.value, "hbm_bytes": hbm.value}

    def set_profiling(self, enabled: "bool | int") -> None:
        """False / 0: off; True / 1: bracket every launch; n > 1: every n-th launch of the encoder kernel classes."""
        _check(lib().sc_runtime_set_profiling(self.handle, int(enabled)))

    def profile_read(self, which: int) -> tuple[float, int]:
        ms, n = C.c_double(), C.c_int64()
        _check(lib().sc_runtime_profile_read(self.handle, which, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def profile_reset(self) -> None:
        _check(lib().sc_runtime_profile_reset(self.handle))

    def synth_fill_dev(self, dev_ptr: int, rows: int, dim: int, ld: int, seed: int, first_row: int = 0) -> None:
        _check(lib().sc_synth_fill_dev(self.handle, C.c_void_p(dev_ptr), rows, dim, ld, seed, first_row))


_shared_runtimes: dict = {}
_shared_lock = threading.Lock()  # not _lib_lock: Runtime() takes that one inside lib()


def shared_runtime(device: int = 0) -> Runtime:
    """The process-wide runtime of a device.  The embedding client and the vector store use it by default, so that the
    encoder's output buffer and the index live on one device and one stream and a batch can go from one to the other
    without touching host memory (Encoder.embed_ids_into).  Never closed explicitly: it lives as long as the process."""
    with _shared_lock:
        rt = _shared_runtimes.get(int(device))
        if rt is None or not rt._h:
            rt = Runtime(device=int(device))
            _shared_runtimes[int(device)] = rt
        return rt


class Index:
    """HBM-resident vector index (sc_index): FLAT or IVF_FLAT, metric IP / L2 / COSINE."""

    def __init__(self, rt: Runtime, dim: int, metric: str = "IP", kind: str = "FLAT", nlist: int = 128, row_base: int = 0):
        if metric not in METRICS:
            raise ValueError(f"unknown metric {metric!r}")
        if kind not in KINDS:
            raise ValueError(f"unknown index kind {kind!r}")
        self.rt = rt
        self.dim = int(dim)
        self.metric = metric
        self.kind = kind
        self.row_base = int(row_base)
        self._h = C.c_void_p()
        _check(lib().sc_index_create(rt.handle, self.dim, METRICS[metric], KINDS[kind], int(nlist), self.row_base, C.byref(self._h)))

    def close(self) -> None:
        if self._h:
            lib().sc_index_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            if not sys.is_finalizing():
                self.close()
        except Exception:
            pass

    @property
    def handle(self) -> C.c_void_p:
        if not self._h:
            raise RuntimeError("index is closed")
        return self._h

    def info(self) -> dict:
        rows, dim, ld = C.c_int64(), C.c_int32(), C.c_int32()
        _check(lib().sc_index_info(self.handle, C.byref(rows), C.byref(dim), C.byref(ld)))
        return {"rows": rows.value, "dim": dim.value, "ld": ld.value}

    def __len__(self) -> int:
        return self.info()["rows"]

    def reserve(self, rows: int) -> None:
        _check(lib().sc_index_reserve(self.handle, int(rows)))

    def add(self, vecs) -> None:
        v = _as_f32(vecs, self.dim)
        _check(lib().sc_index_add(self.handle, v.ctypes.data_as(C.c_void_p), v.shape[0]))

    def overwrite(self, vecs, rows) -> None:
        v = _as_f32(vecs, self.dim)
        r = np.ascontiguousarray(rows, dtype=np.int64)
        if r.shape != (v.shape[0],):
            raise ValueError("rows must have one entry per vector")
        _check(lib().sc_index_overwrite(self.handle, v.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), v.shape[0]))

    def put_rows(self, vecs, rows) -> None:
        """rows[i] <- vecs[i]; a row number is an existing row (replace) or the next free one (append)."""
        v = _as_f32(vecs, self.dim)
        r = np.ascontiguousarray(rows, dtype=np.int64)
        if r.shape != (v.shape[0],):
            raise ValueError("rows must have one entry per vector")
        _check(lib().sc_index_put_rows(self.handle, v.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), v.shape[0]))

    def put_rows_dev(self, vecs_ptr: int, rows) -> None:
        """Same with a DEVICE pointer to tight [n, dim] f32 vectors (e.g. a torch tensor's data_ptr())."""
        r = np.ascontiguousarray(rows, dtype=np.int64)
        _check(lib().sc_index_put_rows_dev(self.handle, C.c_void_p(int(vecs_ptr)), r.ctypes.data_as(C.c_void_p), r.shape[0]))

    def delete_rows(self, rows) -> None:
        """Remove the given rows (distinct, in [0, len)); the survivors keep their order and are renumbered densely:
        new number = old number - deleted rows below it.  Nothing changes if the call fails."""
        r = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        _check(lib().sc_index_delete_rows(self.handle, r.ctypes.data_as(C.c_void_p), r.shape[0]))

    def last_delete_stats(self) -> dict:
        """What the last delete_rows moved: `rows_moved` (survivors above the first deleted stored position), `bytes_moved` (over every
        per-row array), and the shadows that were valid before it as bit sets (1 bf16, 2 int8, 4 centred IVF): `shadows_kept`
        were compacted with the rows, `shadows_dropped` invalidated (only when every row was deleted)."""
        rows, nbytes, kept, dropped = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
        _check(lib().sc_index_last_delete_stats(self.handle, C.byref(rows), C.byref(nbytes), C.byref(kept), C.byref(dropped)))
        return {"rows_moved": int(rows.value), "bytes_moved": int(nbytes.value), "shadows_kept": int(kept.value), "shadows_dropped": int(dropped.value)}

    def get_rows(self, first: int, n: int) -> np.ndarray:
        out = np.empty((n, self.dim), dtype=np.float32)
        _check(lib().sc_index_get_rows(self.handle, int(first), int(n), out.ctypes.data_as(C.c_void_p)))
        return out

    def fill_synthetic(self, n: int, seed: int, first_row: int = 0) -> None:
        _check(lib().sc_index_fill_synthetic(self.handle, int(n), int(seed), int(first_row)))

    def fill_synthetic_clustered(self, n: int, seed: int, nclusters: int, spread: float, first_row: int = 0) -> None:
        _check(lib().sc_index_fill_synthetic_clustered(self.handle, int(n), int(seed), int(first_row), int(nclusters), float(spread)))

    def release_scratch(self) -> None:
        _check(lib().sc_index_release_scratch(self.handle))

    def search(self, queries, k: int = 10, nprobe: int = 16) -> tuple[np.ndarray, np.ndarray]:
        """queries [Q, dim] -> (dist [Q, k] f32, rows [Q, k] i64), best first."""
        q = _as_f32(queries, self.dim)
        Q = q.shape[0]
        dist, rows = _result_arrays(Q, k)
        _check(lib().sc_index_search(self.handle, q.ctypes.data_as(C.c_void_p), Q, int(k), int(nprobe),
                                     dist.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p)))
        return dist, rows

    def search_masked(self, queries, allow, k: int = 10) -> tuple[np.ndarray, np.ndarray]:
        """Exact search over the allowed rows only (sc_index_search_masked): allow = uint32 bitset words over local row numbers or a
        boolean array of length len(index).  -> (dist [Q, k], rows [Q, k]) as search(); fewer than k allowed rows: padded with -1."""
        q = _as_f32(queries, self.dim)
        Q = q.shape[0]
        allow_ptr, allow_words, _keep = self._allow_args(pack_allow(allow, len(self)))  # (packed here: the bitset is required, None is refused)
        dist, rows = _result_arrays(Q, k)
        _check(lib().sc_index_search_masked(self.handle, q.ctypes.data_as(C.c_void_p), Q, int(k), allow_ptr, allow_words,
                                            dist.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p)))
        return dist, rows

    def search_masked_dev(self, q_ptr: int, Q: int, k: int, allow_ptr: int, allow_words: int, dist_ptr: int, rows_ptr: int) -> None:
        """Device-pointer variant (enqueued on the runtime's stream; synchronises it once: sc_index_search_masked_dev)."""
        _check(lib().sc_index_search_masked_dev(self.handle, C.c_void_p(q_ptr), int(Q), int(k), C.c_void_p(allow_ptr), int(allow_words),
                                                C.c_void_p(dist_ptr), C.c_void_p(rows_ptr)))

    def last_mask_stats(self) -> dict:
        """After a masked search: rows the bitset allowed, rows the answering scan read per pass (0: none launched), and whether the
        gathered kernel ran (sc_index_last_mask_stats)."""
        a, sc, g = C.c_int64(), C.c_int64(), C.c_int32()
        _check(lib().sc_index_last_mask_stats(self.handle, C.byref(a), C.byref(sc), C.byref(g)))
        return {"allowed_rows": int(a.value), "scanned_rows": int(sc.value), "gathered": bool(g.value)}

    def set_groups(self, labels) -> None:
        """Install one opaque int32 label per current row for search_grouped (sc_index_set_groups): a device copy that replaces any
        earlier set; valid until the row count changes (an append) or delete_rows renumbers the rows."""
        lab = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
        _check(lib().sc_index_set_groups(self.handle, lab.ctypes.data_as(C.c_void_p), lab.shape[0]))

    def search_grouped(self, queries, k: int = 10, allow=None) -> tuple[np.ndarray, np.ndarray]:
        """Exact search with at most one hit per label (sc_index_search_grouped): the best allowed row of each of the k best labels,
        best first; allow = None (every row) or as for search_masked.  Fewer than k labels: padded with -1."""
        q = _as_f32(queries, self.dim)
        Q = q.shape[0]
        dist, rows = _result_arrays(Q, k)
        allow_ptr, allow_words, _keep = self._allow_args(allow)
        _check(lib().sc_index_search_grouped(self.handle, q.ctypes.data_as(C.c_void_p), Q, int(k), allow_ptr, allow_words,
                                             dist.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p)))
        return dist, rows

    def search_grouped_dev(self, q_ptr: int, Q: int, k: int, allow_ptr: int, allow_words: int, dist_ptr: int, rows_ptr: int) -> None:
        """Device-pointer variant (allow_ptr 0 with allow_words 0: every row; synchronises the stream once per round:
        sc_index_search_grouped_dev)."""
        _check(lib().sc_index_search_grouped_dev(self.handle, C.c_void_p(q_ptr), int(Q), int(k), C.c_void_p(allow_ptr) if allow_ptr else None, int(allow_words),
                                                 C.c_void_p(dist_ptr), C.c_void_p(rows_ptr)))

    def last_group_stats(self) -> dict:
        """After a grouped search: width of round 0, queries that needed exclusion rounds, exclusion rounds run (summed over the
        queries) and rows read by all scans of the call (sc_index_last_group_stats)."""
        w, c, r, sc = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        _check(lib().sc_index_last_group_stats(self.handle, C.byref(w), C.byref(c), C.byref(r), C.byref(sc)))
        return {"first_width": int(w.value), "queries_continued": int(c.value), "rounds": int(r.value), "rows_scanned": int(sc.value)}

    def search_mmr(self, queries, k: int = 10, fetch_k: int = 40, lam: float = 0.5, allow=None) -> tuple[np.ndarray, np.ndarray]:
        """Diversified exact search by maximal marginal relevance (sc_index_search_mmr): the greedy selection of k out of the exact
        top-fetch_k (k <= fetch_k <= 128) of the allowed rows, lam in [0, 1] weighing relevance against redundancy, in selection
        order; allow = None (every row) or as for search_masked.  Fewer than k allowed rows: padded with -1."""
        q = _as_f32(queries, self.dim)
        Q = q.shape[0]
        dist, rows = _result_arrays(Q, k)
        allow_ptr, allow_words, _keep = self._allow_args(allow)
        _check(lib().sc_index_search_mmr(self.handle, q.ctypes.data_as(C.c_void_p), Q, int(k), int(fetch_k), float(lam), allow_ptr, allow_words,
                                         dist.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p)))
        return dist, rows

    def search_mmr_dev(self, q_ptr: int, Q: int, k: int, fetch_k: int, lam: float, allow_ptr: int, allow_words: int, dist_ptr: int, rows_ptr: int) -> None:
        """Device-pointer variant (allow_ptr 0 with allow_words 0: every row; synchronises only where the searches underneath do:
        sc_index_search_mmr_dev)."""
        _check(lib().sc_index_search_mmr_dev(self.handle, C.c_void_p(q_ptr), int(Q), int(k), int(fetch_k), float(lam), C.c_void_p(allow_ptr) if allow_ptr else None,
                                             int(allow_words), C.c_void_p(dist_ptr), C.c_void_p(rows_ptr)))

    def last_mmr_stats(self) -> dict:
        """After an MMR search: its fetch_k, the smallest candidate count of the batch and the rows read by its candidate scans
        (sc_index_last_mmr_stats)."""
        f, c, sc = C.c_int32(), C.c_int32(), C.c_int64()
        _check(lib().sc_index_last_mmr_stats(self.handle, C.byref(f), C.byref(c), C.byref(sc)))
        return {"fetch_k": int(f.value), "min_candidates": int(c.value), "rows_scanned": int(sc.value)}

    def set_terms(self, terms, first_row: int = 0) -> None:
        """Install or overwrite the term rows [first_row, first_row + len(terms)) of the lexical search (sc_index_set_terms): terms
        [n, T] uint16 as lex_terms() makes them, T fixed by the first install; first_row at most the term rows held.  Valid while
        the index has exactly as many rows; delete_rows drops them."""
        t = np.ascontiguousarray(terms, dtype=np.uint16)
        if t.ndim != 2:
            raise ValueError(f"terms must be a [n, T] uint16 array, got shape {t.shape}")
        _check(lib().sc_index_set_terms(self.handle, int(first_row), t.shape[0], t.shape[1], t.ctypes.data_as(C.c_void_p)))

    def drop_terms(self) -> None:
        """Remove the term rows and free their device array (sc_index_drop_terms)."""
        _check(lib().sc_index_drop_terms(self.handle))

    def lex_stats(self) -> dict:
        """rows, sum_dl and df [65536] uint32 (rows holding each term) of the term rows (sc_index_lex_stats); the caller derives avgdl
        and the IDF weights from them."""
        rows, total = C.c_int64(), C.c_int64()
        df = np.empty(LEX_DF_SIZE, dtype=np.uint32)
        _check(lib().sc_index_lex_stats(self.handle, C.byref(rows), C.byref(total), df.ctypes.data_as(C.c_void_p)))
        return {"rows": int(rows.value), "sum_dl": int(total.value), "df": df}

    @staticmethod
    def _lex_query_args(qterms, qweights, nterms) -> "tuple[np.ndarray, np.ndarray, np.ndarray]":
        qt = np.ascontiguousarray(qterms, dtype=np.uint16)
        qw = np.ascontiguousarray(qweights, dtype=np.float32)
        nt = np.ascontiguousarray(nterms, dtype=np.int32).reshape(-1)
        if qt.ndim != 2 or qt.shape[1] != LEX_MAX_QTERMS or qw.shape != qt.shape or nt.shape[0] != qt.shape[0]:
            raise ValueError(f"expected qterms / qweights [Q, {LEX_MAX_QTERMS}] and nterms [Q], got {qt.shape}, {qw.shape}, {nt.shape}")
        return qt, qw, nt

    def _allow_args(self, allow):
        if allow is None:
            return None, 0, None
        words = pack_allow(allow, len(self))
        if words.size == 0:  # an empty index: still a valid pointer
            words = np.zeros(1, dtype=np.uint32)
        return words.ctypes.data_as(C.c_void_p), words.shape[0], words

    def search_lexical(self, qterms, qweights, nterms, k: int = 10, k1: float = 1.2, b: float = 0.75, avgdl: float = 1.0, allow=None) -> tuple[np.ndarray, np.ndarray]:
        """BM25 over the term rows (sc_index_search_lexical): qterms [Q, 32] uint16 strictly ascending per query, qweights [Q, 32] f32
        finite and > 0, nterms [Q] -> (score [Q, k] f32, rows [Q, k] i64), larger score first, ties to the lower row, padded with
        -1 / -inf; rows without a query term are never hits.  allow as for search_masked, or None."""
        qt, qw, nt = self._lex_query_args(qterms, qweights, nterms)
        Q = qt.shape[0]
        score, rows = _result_arrays(Q, k)
        allow_ptr, allow_words, _keep = self._allow_args(allow)
        _check(lib().sc_index_search_lexical(self.handle, Q, int(k), qt.ctypes.data_as(C.c_void_p), qw.ctypes.data_as(C.c_void_p), nt.ctypes.data_as(C.c_void_p),
                                             float(k1), float(b), float(avgdl), allow_ptr, allow_words, score.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p)))
        return score, rows

    def search_lexical_dev(self, Q: int, k: int, qterms_ptr: int, qweights_ptr: int, nterms_ptr: int, k1: float, b: float, avgdl: float, allow_ptr: int,
                           allow_words: int, score_ptr: int, rows_ptr: int) -> None:
        """Device-pointer variant (allow_ptr 0 with allow_words 0: every row; synchronises the stream once: sc_index_search_lexical_dev)."""
        _check(lib().sc_index_search_lexical_dev(self.handle, int(Q), int(k), C.c_void_p(qterms_ptr), C.c_void_p(qweights_ptr), C.c_void_p(nterms_ptr), float(k1), float(b),
                                                 float(avgdl), C.c_void_p(allow_ptr) if allow_ptr else None, int(allow_words), C.c_void_p(score_ptr), C.c_void_p(rows_ptr)))

    def search_hybrid(self, queries, qterms, qweights, nterms, k: int = 10, fetch_k: int = 40, k1: float = 1.2, b: float = 0.75, avgdl: float = 1.0, c: int = 60,
                      dense_weight: float = 1.0, lexical_weight: float = 1.0, allow=None) -> tuple[np.ndarray, np.ndarray]:
        """Dense top-fetch_k and lexical top-fetch_k fused by weighted reciprocal rank (sc_index_search_hybrid): score of a row =
        dense_weight / (c + its dense rank) + lexical_weight / (c + its lexical rank), ranks from 0, a missing rank contributing 0;
        -> (fused score [Q, k], rows [Q, k]) best first, ties to the lower row, padded with -1 / -inf.  k <= fetch_k <= 128."""
        q = _as_f32(queries, self.dim)
        qt, qw, nt = self._lex_query_args(qterms, qweights, nterms)
        Q = q.shape[0]
        if qt.shape[0] != Q:
            raise ValueError(f"{Q} query vectors but {qt.shape[0]} term lists")
        score, rows = _result_arrays(Q, k)
        allow_ptr, allow_words, _keep = self._allow_args(allow)
        _check(lib().sc_index_search_hybrid(self.handle, q.ctypes.data_as(C.c_void_p), Q, int(k), int(fetch_k), qt.ctypes.data_as(C.c_void_p),
                                            qw.ctypes.data_as(C.c_void_p), nt.ctypes.data_as(C.c_void_p), float(k1), float(b), float(avgdl), int(c), float(dense_weight),
                                            float(lexical_weight), allow_ptr, allow_words, score.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p)))
        return score, rows

    def search_hybrid_dev(self, q_ptr: int, Q: int, k: int, fetch_k: int, qterms_ptr: int, qweights_ptr: int, nterms_ptr: int, k1: float, b: float, avgdl: float, c: int,
                          dense_weight: float, lexical_weight: float, allow_ptr: int, allow_words: int, score_ptr: int, rows_ptr: int) -> None:
        """Device-pointer variant (sc_index_search_hybrid_dev)."""
        _check(lib().sc_index_search_hybrid_dev(self.handle, C.c_void_p(q_ptr), int(Q), int(k), int(fetch_k), C.c_void_p(qterms_ptr), C.c_void_p(qweights_ptr),
                                                C.c_void_p(nterms_ptr), float(k1), float(b), float(avgdl), int(c), float(dense_weight), float(lexical_weight),
                                                C.c_void_p(allow_ptr) if allow_ptr else None, int(allow_words), C.c_void_p(score_ptr), C.c_void_p(rows_ptr)))

    def last_lex_stats(self) -> dict:
        """After a lexical or hybrid search: term rows a pass streams, their bytes, passes run (sc_index_last_lex_stats)."""
        r, by, p = C.c_int64(), C.c_int64(), C.c_int32()
        _check(lib().sc_index_last_lex_stats(self.handle, C.byref(r), C.byref(by), C.byref(p)))
        return {"rows_scanned": int(r.value), "bytes_per_pass": int(by.value), "passes": int(p.value)}

    # ---- the token store (late interaction): sc_index_put_tokens and the calls that score from it
    def put_tokens(self, rows, token_vectors, fmt: str = "f32") -> None:
        """Store the token vectors of `rows` (distinct local row numbers): token_vectors is one [n_i, W] f32 array per row (n_i 0 .. 2 048;
        0 or None removes the row's tokens), or a pair (counts [n], vecs [sum counts, W]).  W and fmt ('f32' | 'bf16': rounded to
        nearest-even once, here) are fixed by the first call.  A row's previous tokens become dead (compact_tokens)."""
        r = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        counts, vecs = pack_token_lists(token_vectors)
        if counts.shape[0] != r.shape[0]:
            raise ValueError("token_vectors must have one entry per row")
        if vecs.shape[0] == 0:
            st = self.token_stats()
            if not st["W"]:
                raise ValueError("no token vectors given and none installed: W is unknown")
            vecs = np.empty((0, st["W"]), dtype=np.float32)
        _check(lib().sc_index_put_tokens(self.handle, r.ctypes.data_as(C.c_void_p), r.shape[0], counts.ctypes.data_as(C.c_void_p), vecs.ctypes.data_as(C.c_void_p),
                                         vecs.shape[1], TOKEN_FORMATS[fmt]))

    def put_tokens_dev(self, rows, counts, vecs_ptr: int, src, W: int, fmt: str = "f32") -> None:
        """put_tokens with the vectors on the device (sc_index_put_tokens_dev): vecs_ptr = device address of [.., W] f32, counts [n] the
        tokens of each row, src = the source token of every stored token in stored order (int32 [sum counts], a gather list) or None:
        the first sum(counts) tokens in order.  Copied (f32) or rounded (bf16) on the device into the pool."""
        r = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        c = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
        if c.shape[0] != r.shape[0]:
            raise ValueError("counts must have one entry per row")
        s = None if src is None else np.ascontiguousarray(src, dtype=np.int32).reshape(-1)
        if s is not None and s.shape[0] != int(c.sum()):
            raise ValueError("src must name one source token per stored token")
        _check(lib().sc_index_put_tokens_dev(self.handle, r.ctypes.data_as(C.c_void_p), r.shape[0], c.ctypes.data_as(C.c_void_p), C.c_void_p(int(vecs_ptr)) if vecs_ptr else None,
                                             None if s is None else s.ctypes.data_as(C.c_void_p), int(W), TOKEN_FORMATS[fmt]))

    def reserve_tokens(self, tokens: int) -> None:
        """Pre-size the token pool (sc_index_reserve_tokens)."""
        _check(lib().sc_index_reserve_tokens(self.handle, int(tokens)))

    def compact_tokens(self) -> None:
        """Gather the live tokens in row order into a fresh pool: dead = 0 afterwards (sc_index_compact_tokens)."""
        _check(lib().sc_index_compact_tokens(self.handle))

    def drop_tokens(self) -> None:
        _check(lib().sc_index_drop_tokens(self.handle))

    def token_stats(self) -> dict:
        """rows_with_tokens, live and dead tokens, W, fmt ('f32' | 'bf16'; W 0: nothing installed), pool_bytes (sc_index_token_stats)."""
        rw, live, dead, pool = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        W, fmt = C.c_int32(), C.c_int32()
        _check(lib().sc_index_token_stats(self.handle, C.byref(rw), C.byref(live), C.byref(dead), C.byref(W), C.byref(fmt), C.byref(pool)))
        return {"rows_with_tokens": int(rw.value), "live": int(live.value), "dead": int(dead.value), "W": int(W.value), "fmt": "bf16" if fmt.value == 1 else "f32",
                "pool_bytes": int(pool.value)}

    def token_counts(self, rows) -> np.ndarray:
        """Tokens stored for each of `rows` (int32 [n]; no vectors are copied)."""
        r = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        counts = np.empty(r.shape[0], dtype=np.int32)
        _check(lib().sc_index_get_tokens(self.handle, r.ctypes.data_as(C.c_void_p), r.shape[0], counts.ctypes.data_as(C.c_void_p), None, 0))
        return counts

    def get_tokens(self, rows) -> "tuple[np.ndarray, np.ndarray]":
        """(counts [n] int32, vecs [sum counts, W] f32): the rows' stored token vectors, widened as stored (sc_index_get_tokens)."""
        r = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        counts = np.empty(r.shape[0], dtype=np.int32)
        _check(lib().sc_index_get_tokens(self.handle, r.ctypes.data_as(C.c_void_p), r.shape[0], counts.ctypes.data_as(C.c_void_p), None, 0))
        total = int(counts.sum())
        vecs = np.empty((total, self.token_stats()["W"]), dtype=np.float32)
        if total:
            _check(lib().sc_index_get_tokens(self.handle, r.ctypes.data_as(C.c_void_p), r.shape[0], counts.ctypes.data_as(C.c_void_p), vecs.ctypes.data_as(C.c_void_p), total))
        return counts, vecs

    def rerank_late(self, questions, cand) -> np.ndarray:
        """MaxSim scores of every question against its candidates from the stored token vectors (sc_index_rerank_late): questions = one
        [nq, W] f32 array per question (1 <= nq <= 128) or a pair (Q [sum nq, W], q_off [Bq + 1]); cand [Bq, C] = row_base + local row as
        the searches return them, -1 = padding.  -> scores [Bq, C] f32 in candidate order; padding and rows without tokens: -inf."""
        Q, q_off = pack_questions(questions)
        c = np.ascontiguousarray(cand, dtype=np.int64)
        if c.ndim != 2 or c.shape[0] != q_off.shape[0] - 1:
            raise ValueError(f"cand must be [Bq, C] with one row per question, got shape {c.shape}")
        out = np.empty(c.shape, dtype=np.float32)
        _check(lib().sc_index_rerank_late(self.handle, Q.ctypes.data_as(C.c_void_p), q_off.ctypes.data_as(C.c_void_p), c.shape[0], c.ctypes.data_as(C.c_void_p), c.shape[1],
                                          out.ctypes.data_as(C.c_void_p)))
        return out

    def search_late(self, questions, k: int = 10, allow=None) -> "tuple[np.ndarray, np.ndarray]":
        """The exact, exhaustive MaxSim top-k over the rows that have tokens (sc_index_search_late): questions as rerank_late; allow as
        for search_masked, or None.  -> (score [Bq, k] f32, rows [Bq, k] i64), larger score first, ties to the lower row, padded
        with -1 / -inf."""
        Q, q_off = pack_questions(questions)
        Bq = q_off.shape[0] - 1
        score, rows = _result_arrays(Bq, k)
        allow_ptr, allow_words, _keep = self._allow_args(allow)
        _check(lib().sc_index_search_late(self.handle, Q.ctypes.data_as(C.c_void_p), q_off.ctypes.data_as(C.c_void_p), Bq, int(k), allow_ptr, allow_words,
                                          score.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p)))
        return score, rows

    def train(self, niter: int = 10, seed: int = 0) -> None:
        """IVF_FLAT: k-means + list build (sc_index_train)."""
        _check(lib().sc_index_train(self.handle, int(niter), int(seed)))

    def ivf_info(self) -> dict:
        n = C.c_int32()
        _check(lib().sc_index_ivf_info(self.handle, C.byref(n), None, None))
        if n.value == 0:
            return {"nlist": 0}
        cent = np.empty((n.value, self.dim), dtype=np.float32)
        sizes = np.empty((n.value,), dtype=np.int64)
        _check(lib().sc_index_ivf_info(self.handle, C.byref(n), cent.ctypes.data_as(C.c_void_p), sizes.ctypes.data_as(C.c_void_p)))
        return {"nlist": n.value, "centroids": cent, "list_sizes": sizes}

    def ivf_assignments(self) -> np.ndarray:
        """List of every row, insertion order (int32 [rows]); the index must be trained."""
        out = np.empty(len(self), dtype=np.int32)
        _check(lib().sc_index_ivf_assignments(self.handle, out.ctypes.data_as(C.c_void_p)))
        return out

    def set_ivf(self, centroids, assign) -> None:
        """Install a saved IVF structure (centroids [nlist, dim], list of every row) without re-running k-means."""
        c = _as_f32(centroids, self.dim)
        a = np.ascontiguousarray(assign, dtype=np.int32)
        if a.shape != (len(self),):
            raise ValueError("assign must have one entry per stored row")
        _check(lib().sc_index_set_ivf(self.handle, c.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), c.shape[0]))

    def assign_lists(self, centroids) -> None:
        """Build the IVF lists for given centroids [nlist, dim] (no k-means): what every rank of a sharded collection does
        with the centroids one rank trained."""
        c = _as_f32(centroids, self.dim)
        _check(lib().sc_index_assign_lists(self.handle, c.ctypes.data_as(C.c_void_p), c.shape[0]))

    def set_search_mode(self, mode: str) -> None:
        """'auto' | 'exact' | 'batched' | 'ivf' (per-query probing) | 'ivf_listmajor' (exact f32 list-major probing) | 'ivf_coarse' (list-major probing
        behind the int8 coarse stage; L2 only) -- see sc_index_set_search_mode."""
        _check(lib().sc_index_set_search_mode(self.handle, {"auto": 0, "exact": 1, "batched": 2, "ivf": 3, "ivf_listmajor": 4, "ivf_coarse": 5}[mode]))

    def set_coarse_stage(self, bits: int) -> None:
        """First coarse stage of the batched path: 0 auto (int8, then bf16), 8 int8 only, 16 bf16 only (sc_index_set_coarse_stage)."""
        _check(lib().sc_index_set_coarse_stage(self.handle, int(bits)))

    def last_search_stats(self) -> dict:
        """path; `uncertified` = queries that ended in the exact scan; for the batched path also the stage it started on
        (`coarse_bits` 8 / 16), how many queries the int8 stage handed to the bf16 stage (`handed_to_bf16`), and how many
        queries went through a collect pass after a failed certificate / were answered by it (`collect_tried`, `collect_resolved`)."""
        path, unc, bits, handed = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        _check(lib().sc_index_last_search_stats(self.handle, C.byref(path), C.byref(unc)))
        _check(lib().sc_index_last_coarse_stats(self.handle, C.byref(bits), C.byref(handed)))
        out = {"path": {0: "none", 1: "exact", 2: "batched", 3: "ivf", 4: "ivf_listmajor", 5: "ivf_coarse", 6: "masked", 7: "grouped", 8: "mmr", 9: "lexical", 10: "hybrid"}[path.value], "uncertified": unc.value}
        if path.value in (3, 4, 5):
            tail = C.c_int64()
            _check(lib().sc_index_last_tail_rows(self.handle, C.byref(tail)))
            out["tail_rows"] = int(tail.value)
        if path.value == 2:
            tried, resolved = C.c_int32(), C.c_int32()
            _check(lib().sc_index_last_collect_stats(self.handle, C.byref(tried), C.byref(resolved)))
            wide = C.c_int32()
            _check(lib().sc_index_last_wide(self.handle, C.byref(wide)))
            out.update(coarse_bits=bits.value, handed_to_bf16=handed.value, collect_tried=tried.value, collect_resolved=resolved.value, wide=bool(wide.value))
        return out

    def search_sharded(self, comm: "Comm", queries, k: int = 10, nprobe: int = 16) -> tuple[np.ndarray, np.ndarray]:
        """Row-sharded search (every rank calls it with the same queries): -> the merged global (dist, rows) [Q, k]."""
        q = _as_f32(queries, self.dim)
        Q = q.shape[0]
        dist, rows = _result_arrays(Q, k)
        _check(lib().sc_index_search_sharded(self.handle, comm.handle, q.ctypes.data_as(C.c_void_p), Q, int(k), int(nprobe),
                                             dist.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p)))
        return dist, rows

    def search_sharded_dev(self, comm: "Comm", q_ptr: int, Q: int, k: int, all_dist_ptr: int, all_rows_ptr: int, nprobe: int = 16) -> None:
        """Device-pointer variant: every shard's [Q, k] into all_dist / all_rows [world, Q, k] (sc_index_search_sharded_dev)."""
        _check(lib().sc_index_search_sharded_dev(self.handle, comm.handle, C.c_void_p(q_ptr), int(Q), int(k), int(nprobe),
                                                 C.c_void_p(all_dist_ptr), C.c_void_p(all_rows_ptr)))

    def train_sharded(self, comm: "Comm", niter: int = 10, root: int = 0) -> None:
        _check(lib().sc_index_train_sharded(self.handle, comm.handle, int(niter), int(root)))

    def last_probe_stats(self) -> dict:
        """After a list-major IVF probe: rows of the distinct probed lists, rows streamed, work items (sc_index_last_probe_stats)."""
        u, st, g = C.c_int64(), C.c_int64(), C.c_int32()
        _check(lib().sc_index_last_probe_stats(self.handle, C.byref(u), C.byref(st), C.byref(g)))
        return {"unique_rows": u.value, "streamed_rows": st.value, "groups": g.value}

    def search_dev(self, q_ptr: int, Q: int, k: int, dist_ptr: int, rows_ptr: int, nprobe: int = 16) -> None:
        """Device-pointer variant (enqueued on the runtime's stream; see sc_index_search_dev for where it synchronises)."""
        _check(lib().sc_index_search_dev(self.handle, C.c_void_p(q_ptr), int(Q), int(k), int(nprobe), C.c_void_p(dist_ptr), C.c_void_p(rows_ptr)))


COMM_ID_BYTES = 128


def comm_unique_id() -> bytes:
    """The RCCL rendezvous id (rank 0 creates it and hands the 128 bytes to the other ranks out of band)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(lib().sc_comm_unique_id(buf, COMM_ID_BYTES))
    return buf.raw


class Comm:
    """RCCL communicator of the path's two collectives (sc_comm): the all-gather of per-shard top-k and the centroid broadcast.
    Device pointers in, device pointers out, everything on the runtime's stream."""

    def __init__(self, rt: Runtime, rank: int, world: int, unique_id: bytes):
        if len(unique_id) != COMM_ID_BYTES:
            raise ValueError(f"unique_id must be {COMM_ID_BYTES} bytes")
        self.rt, self.rank, self.world = rt, int(rank), int(world)
        self._h = C.c_void_p()
        _check(lib().sc_comm_create(rt.handle, self.rank, self.world, unique_id, COMM_ID_BYTES, C.byref(self._h)))

    def close(self) -> None:
        if self._h:
            lib().sc_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            if not sys.is_finalizing():
                self.close()
        except Exception:
            pass

    @property
    def handle(self) -> C.c_void_p:
        if not self._h:
            raise RuntimeError("communicator is closed")
        return self._h

    def info(self) -> dict:
        """What the communicator itself reports (sc_comm_info, sc_comm_rccl_version): rank, world, RCCL version."""
        r, w, v = C.c_int32(), C.c_int32(), C.c_int32()
        _check(lib().sc_comm_info(self.handle, C.byref(r), C.byref(w)))
        _check(lib().sc_comm_rccl_version(C.byref(v)))
        return {"rank": r.value, "world": w.value, "rccl_version": v.value}

    def allgather_topk(self, dist_ptr: int, rows_ptr: int, Q: int, k: int, all_dist_ptr: int, all_rows_ptr: int) -> None:
        _check(lib().sc_comm_allgather_topk(self.handle, C.c_void_p(dist_ptr), C.c_void_p(rows_ptr), int(Q), int(k),
                                            C.c_void_p(all_dist_ptr), C.c_void_p(all_rows_ptr)))

    def broadcast(self, buf_ptr: int, nbytes: int, root: int = 0) -> None:
        _check(lib().sc_comm_broadcast(self.handle, C.c_void_p(buf_ptr), int(nbytes), int(root)))

    def allreduce_max(self, value: float) -> float:
        v = C.c_double(float(value))
        _check(lib().sc_comm_allreduce_max(self.handle, C.byref(v)))
        return v.value


BERT_BASE = dict(vocab=30522, hidden=768, layers=12, heads=12, ffn=3072, max_pos=512, type_vocab=2, ln_eps=1e-12)
SEQ_BUCKETS = (32, 64, 128, 256, 512, 1024, 2048)  # > 512: ALiBi or rotary encoders (no position table), or a position table that long
POOLINGS = {"mean": 0, "cls": 1}  # sc_encoder_set_pooling
POOLINGS_T5 = {"mean": 0, "first": 1}  # ... of a T5 encoder (arch 3): "first" = the first token's row (CodeT5+)
POOLINGS_QWEN2 = {"mean": 0, "last": 2}  # ... of a qwen2 encoder (arch 2): "last" = the last real token's row; no "cls" there


def encoder_cfg(c: dict, normalize: bool = False, synth_seed: int = 0) -> EncoderCfg:
    """sc_encoder_cfg of a complete configuration dict (the keys of BERT_BASE plus the architecture switches alibi / rotary / geglu /
    swiglu / rope_theta and, for the pre-LN ModernBERT family, modernbert / local_window / global_every / rope_theta_local; for the causal
    Qwen2 / Qwen3 family, qwen2 / kv_heads / head_dim (0, 64 or 128: heads of 128 are stated, never derived) / qk_norm)."""
    if sum(1 for k in ("modernbert", "qwen2", "t5") if c.get(k)) > 1:
        raise ValueError("encoder configuration: modernbert, qwen2 and t5 are architectures, pick one")
    if c.get("t5"):  # the T5 encoder (arch 3): relative position bias (pos_type 3), ffn "relu" (3) or "gated-gelu" (4)
        ffn = {"relu": 3, "gated-gelu": 4}.get(c.get("t5_ffn"))
        if ffn is None:
            raise ValueError(f"encoder configuration: t5_ffn must be 'relu' or 'gated-gelu', got {c.get('t5_ffn')!r}")
        return EncoderCfg(vocab=c["vocab"], hidden=c["hidden"], layers=c["layers"], heads=c["heads"], ffn=c["ffn"], max_pos=c["max_pos"],
                          type_vocab=c.get("type_vocab") or 1, ln_eps=c["ln_eps"], normalize=1 if normalize else 0, synth_seed=synth_seed, pos_type=3,
                          ffn_type=ffn, arch=3, head_dim=int(c.get("head_dim") or 0), rel_buckets=int(c.get("rel_buckets") or 0),
                          rel_max_distance=int(c.get("rel_max_distance") or 0))
    if c.get("rotary") and c.get("alibi"):
        raise ValueError("encoder configuration: rotary and alibi are two position schemes, pick one")
    if c.get("swiglu") and c.get("geglu"):
        raise ValueError("encoder configuration: swiglu and geglu are two feed-forward gates, pick one")
    return EncoderCfg(vocab=c["vocab"], hidden=c["hidden"], layers=c["layers"], heads=c["heads"], ffn=c["ffn"],
                      max_pos=c["max_pos"], type_vocab=c["type_vocab"], ln_eps=c["ln_eps"], normalize=1 if normalize else 0,
                      synth_seed=synth_seed, pos_type=2 if c.get("rotary") else 1 if c.get("alibi") else 0,
                      ffn_type=2 if c.get("swiglu") else 1 if c.get("geglu") else 0, rope_theta=float(c.get("rope_theta") or 0.0),
                      # pre-LN ModernBERT (sc_encoder_cfg.arch 1): local attention in the layers with l % global_every != 0
                      # pre-norm causal decoder (arch 2, Qwen2): kv_heads K / V heads of the grouped-query attention (0 = heads)
                      arch=2 if c.get("qwen2") else 1 if c.get("modernbert") else 0, local_window=int(c.get("local_window") or 0),
                      global_every=int(c.get("global_every") or 0), rope_theta_local=float(c.get("rope_theta_local") or 0.0),
                      kv_heads=int(c.get("kv_heads") or 0), head_dim=int(c.get("head_dim") or 0), qk_norm=1 if c.get("qk_norm") else 0)


class Encoder:
    """Transformer-encoder forward on the device (sc_encoder): token ids in, pooled f32 vectors out.  pooling: "mean" (masked mean over
    the real tokens), "cls" (the last hidden state of the first token: bge, arctic-embed, mxbai, gte) or, on qwen2 encoders only, "last"
    (the last real token's row: causal embedding models; "cls" is refused there)."""

    def __init__(self, rt: Runtime, cfg: dict | None = None, weights: np.ndarray | None = None, normalize: bool = False,
                 synth_seed: int = 0, pooling: str = "mean"):
        c = dict(BERT_BASE)
        c.update(cfg or {})
        self.cfg = encoder_cfg(c, normalize=normalize, synth_seed=synth_seed)
        if pooling not in self.poolings:
            raise ValueError(f"encoder pooling must be one of {sorted(self.poolings)}, got {pooling!r}")
        self.rt = rt
        self.hidden = c["hidden"]
        self.max_pos = c["max_pos"]
        self.num_labels = 0  # of the installed pair head (set_pair_head)
        self.score_labels = 0  # of the installed score head (set_score_head)
        self.token_width = 0  # W of the installed token head (set_token_head)
        self._h = C.c_void_p()
        need = C.c_int64()
        _check(lib().sc_encoder_blob_bytes(C.byref(self.cfg), C.byref(need)))
        self.blob_bytes = need.value
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
            _check(lib().sc_encoder_create(rt.handle, C.byref(self.cfg), w.ctypes.data_as(C.c_void_p), w.nbytes, C.byref(self._h)))
        else:
            _check(lib().sc_encoder_create(rt.handle, C.byref(self.cfg), None, 0, C.byref(self._h)))
        if pooling != "mean":
            self.pooling = pooling

    @property
    def poolings(self) -> dict:
        """The pooling modes of this encoder's architecture: name -> sc_encoder_set_pooling value."""
        return POOLINGS_QWEN2 if self.cfg.arch == 2 else POOLINGS_T5 if self.cfg.arch == 3 else POOLINGS

    @property
    def pooling(self) -> str:
        v = C.c_int32()
        _check(lib().sc_encoder_get_pooling(self.handle, C.byref(v)))
        return next(k for k, n in self.poolings.items() if n == v.value)

    @pooling.setter
    def pooling(self, mode: str) -> None:
        if mode not in self.poolings:
            raise ValueError(f"encoder pooling must be one of {sorted(self.poolings)}, got {mode!r}")
        _check(lib().sc_encoder_set_pooling(self.handle, self.poolings[mode]))

    def close(self) -> None:
        if self._h:
            lib().sc_encoder_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            if not sys.is_finalizing():
                self.close()
        except Exception:
            pass

    @property
    def handle(self) -> C.c_void_p:
        if not self._h:
            raise RuntimeError("encoder is closed")
        return self._h

    @property
    def out_dim(self) -> int:
        """Width of the vectors the embedding calls return: hidden, or E of the installed output projection (sc_encoder_out_dim)."""
        v = C.c_int32()
        _check(lib().sc_encoder_out_dim(self.handle, C.byref(v)))
        return v.value

    def set_output_proj(self, W=None, b=None) -> None:
        """Install the output projection behind the pooling (sc_encoder_set_output_proj): W [E, hidden], b [E] or None; the embedding calls
        then return [B, E] = W pooled + b, L2-normalised when the encoder normalises.  W None removes it."""
        if W is None:
            _check(lib().sc_encoder_set_output_proj(self.handle, None, None, 0))
            return
        W = np.ascontiguousarray(W, np.float32)
        if W.ndim != 2 or W.shape[1] != self.hidden:
            raise ValueError(f"output projection must be [E, {self.hidden}], got {W.shape}")
        b = None if b is None else np.ascontiguousarray(b, np.float32).reshape(-1)
        if b is not None and b.shape != (W.shape[0],):
            raise ValueError("output projection bias must be [E]")
        _check(lib().sc_encoder_set_output_proj(self.handle, W.ctypes.data_as(C.c_void_p), None if b is None else b.ctypes.data_as(C.c_void_p), W.shape[0]))

    def set_path(self, path: str) -> None:
        """'auto' | 'batch' (LayerNorm-folded 256-tile pipeline for every size) | 'small' (split-K + LayerNorm kernels)."""
        _check(lib().sc_encoder_set_path(self.handle, {"auto": 0, "batch": 1, "small": 2}[path]))

    def embed_ids(self, ids: np.ndarray, lens: np.ndarray) -> np.ndarray:
        """ids [B, S] int32 with S in SEQ_BUCKETS, lens [B] -> [B, hidden] f32."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        if ids.ndim != 2 or lens.shape != (ids.shape[0],):
            raise ValueError("ids must be [B, S] and lens [B]")
        B, S = ids.shape
        out = np.empty((B, self.out_dim), dtype=np.float32)
        _check(lib().sc_encoder_embed_ids(self.handle, ids.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), B, S,
                                          out.ctypes.data_as(C.c_void_p)))
        return out

    def embed_ids_into(self, ids: np.ndarray, lens: np.ndarray, index: "Index", rows: np.ndarray, want_host: bool = False,
                       wait: bool = True) -> "np.ndarray | None":
        """Embed one batch and store the vectors in `index` rows `rows` (existing rows are replaced, the next free rows
        appended) without a trip through host memory; returns the vectors only if want_host.  wait=False: return as soon as
        the batch is enqueued (at most two in flight; call wait() before relying on completion)."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        if ids.ndim != 2 or lens.shape != (ids.shape[0],) or rows.shape != (ids.shape[0],):
            raise ValueError("ids must be [B, S], lens [B] and rows [B]")
        B, S = ids.shape
        if not wait and not want_host:
            _check(lib().sc_encoder_embed_ids_into_async(self.handle, ids.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), B, S,
                                                         index.handle, rows.ctypes.data_as(C.c_void_p)))
            return None
        out = np.empty((B, self.out_dim), dtype=np.float32) if want_host else None
        _check(lib().sc_encoder_embed_ids_into(self.handle, ids.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), B, S, index.handle,
                                               rows.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p) if want_host else None))
        return out

    def wait(self) -> None:
        """Block until every batch enqueued with embed_ids_into(..., wait=False) has finished."""
        _check(lib().sc_encoder_wait(self.handle))

    # ---- packed variable-length batches: the ids of the texts one after another, unpadded, and offsets [B + 1] (offsets[0] == 0)
    @staticmethod
    def _packed_args(ids_flat, offsets) -> "tuple[np.ndarray, np.ndarray, int]":
        ids_flat = np.ascontiguousarray(ids_flat, dtype=np.int32)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if ids_flat.ndim != 1 or offsets.ndim != 1 or len(offsets) < 2:
            raise ValueError("ids_flat must be [total] and offsets [B + 1]")
        if int(offsets[-1]) != len(ids_flat) or (np.diff(offsets) < 0).any():
            raise ValueError("offsets must ascend and end at len(ids_flat)")
        return ids_flat, offsets, len(offsets) - 1

    def packed_rows(self, offsets) -> int:
        """Token rows the packed forward runs for these offsets (ceil32 per text, the total rounded up to 256); no GPU work."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        rows = C.c_int64()
        _check(lib().sc_encoder_packed_rows(self.handle, offsets.ctypes.data_as(C.c_void_p), len(offsets) - 1, C.byref(rows)))
        return rows.value

    def embed_packed(self, ids_flat, offsets) -> np.ndarray:
        """embed_ids without padding: text i = ids_flat[offsets[i]:offsets[i + 1]] -> [B, hidden] f32."""
        ids_flat, offsets, B = self._packed_args(ids_flat, offsets)
        out = np.empty((B, self.out_dim), dtype=np.float32)
        _check(lib().sc_encoder_embed_packed(self.handle, ids_flat.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p), B,
                                             out.ctypes.data_as(C.c_void_p)))
        return out

    def embed_packed_into(self, ids_flat, offsets, index: "Index", rows: np.ndarray, want_host: bool = False, wait: bool = True) -> "np.ndarray | None":
        """embed_ids_into on packed input (same in-flight rules; wait() covers both kinds)."""
        ids_flat, offsets, B = self._packed_args(ids_flat, offsets)
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        if rows.shape != (B,):
            raise ValueError("rows must be [B]")
        if not wait and not want_host:
            _check(lib().sc_encoder_embed_packed_into_async(self.handle, ids_flat.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p), B,
                                                            index.handle, rows.ctypes.data_as(C.c_void_p)))
            return None
        out = np.empty((B, self.out_dim), dtype=np.float32) if want_host else None
        _check(lib().sc_encoder_embed_packed_into(self.handle, ids_flat.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p), B, index.handle,
                                                  rows.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p) if want_host else None))
        return out

    # ---- pairs (cross-encoder): [CLS] question [SEP] passage [SEP] as one packed sequence, segment ids from first_lens
    def set_pair_head(self, cls_w, cls_b, pooler_w=None, pooler_b=None) -> None:
        """Install (or replace) the classification head: cls_w [num_labels, H], cls_b [num_labels], optionally the pooler
        (pooler_w [H, H], pooler_b [H]; tanh).  cls_w None removes the head."""
        if cls_w is None:
            _check(lib().sc_encoder_set_pair_head(self.handle, None, None, None, None, 0))
            self.num_labels = 0
            return
        cls_w, cls_b = _f32(cls_w).reshape(-1, self.hidden), _f32(cls_b).reshape(-1)
        if cls_b.shape[0] != cls_w.shape[0]:
            raise ValueError("cls_w must be [num_labels, hidden] and cls_b [num_labels]")
        if pooler_w is not None:
            pooler_w, pooler_b = _f32(pooler_w), _f32(pooler_b)
            if pooler_w.shape != (self.hidden, self.hidden) or pooler_b.shape != (self.hidden,):
                raise ValueError("pooler_w must be [hidden, hidden] and pooler_b [hidden]")
        _check(lib().sc_encoder_set_pair_head(self.handle, _ptr(pooler_w), _ptr(pooler_b) if pooler_w is not None else None, _ptr(cls_w), _ptr(cls_b),
                                              int(cls_w.shape[0])))
        self.num_labels = int(cls_w.shape[0])

    def score_pairs(self, ids_flat, offsets, first_lens, want_cls: bool = False):
        """Packed pairs -> logits [B, num_labels] (and the [CLS] rows [B, hidden] the head read, with want_cls).  first_lens [B]: the
        tokens of each pair that take segment id 0."""
        ids_flat, offsets, B = self._packed_args(ids_flat, offsets)
        first_lens = np.ascontiguousarray(first_lens, dtype=np.int32)
        if first_lens.shape != (B,):
            raise ValueError("first_lens must be [B]")
        logits = np.empty((B, max(1, self.num_labels)), dtype=np.float32)
        cls = np.empty((B, self.hidden), dtype=np.float32) if want_cls else None
        _check(lib().sc_encoder_score_pairs(self.handle, _ptr(ids_flat), _ptr(offsets), _ptr(first_lens), B, _ptr(logits), _ptr(cls)))
        return (logits, cls) if want_cls else logits

    # ---- score heads of the ModernBERT (kind 1) and Qwen2 / Qwen3 (kind 2) rerankers: one packed sequence per pair, no segment ids
    def set_score_head(self, head: "dict | None") -> None:
        """Install (or replace) the score head; None removes it.  head: see score_head_struct."""
        if head is None:
            _check(lib().sc_encoder_set_score_head(self.handle, None))
            self.score_labels = 0
            return
        st, _keep = score_head_struct(head, self.hidden)
        _check(lib().sc_encoder_set_score_head(self.handle, C.byref(st)))
        self.score_labels = int(st.num_labels)

    def score_seqs(self, ids_flat, offsets, want_rows: bool = False):
        """Packed sequences -> logits [B, num_labels] (and, with want_rows, the f32 rows [B, hidden] the head read)."""
        ids_flat, offsets, B = self._packed_args(ids_flat, offsets)
        logits = np.empty((B, max(1, self.score_labels)), dtype=np.float32)
        rows = np.empty((B, self.hidden), dtype=np.float32) if want_rows else None
        _check(lib().sc_encoder_score_seqs(self.handle, _ptr(ids_flat), _ptr(offsets), B, _ptr(logits), _ptr(rows)))
        return (logits, rows) if want_rows else logits

    # ---- late interaction (ColBERT): one vector per token, MaxSim over (query, document) pairs
    def set_token_head(self, w) -> None:
        """Install (or replace) the per-token projection w [W, hidden] (no bias; rounded to bf16 once); None removes it."""
        if w is None:
            _check(lib().sc_encoder_set_token_head(self.handle, None, 0))
            self.token_width = 0
            return
        w = _f32(w)
        if w.ndim != 2 or w.shape[1] != self.hidden:
            raise ValueError("w must be [W, hidden]")
        _check(lib().sc_encoder_set_token_head(self.handle, _ptr(w), int(w.shape[0])))
        self.token_width = int(w.shape[0])

    def embed_tokens(self, ids_flat, offsets, expand_id: int = -1) -> "tuple[np.ndarray, np.ndarray]":
        """Packed texts -> (vectors [sum n_i, W] f32, L2-normalised, text after text; counts [B] = n_i).  expand_id < 0 (documents):
        n_i = len_i.  expand_id >= 0 (queries): n_i = len_i rounded up to 32, the added rows carry that token ([MASK]) and are
        never attended as keys."""
        ids_flat, offsets, B = self._packed_args(ids_flat, offsets)
        lens = np.diff(offsets)
        n = (lens + 31) // 32 * 32 if expand_id >= 0 else lens
        out = np.empty((int(n.sum()), max(1, getattr(self, "token_width", 0))), dtype=np.float32)
        counts = np.empty(B, dtype=np.int32)
        _check(lib().sc_encoder_embed_tokens(self.handle, _ptr(ids_flat), _ptr(offsets), B, int(expand_id), _ptr(out), _ptr(counts)))
        return out, counts

    def embed_tokens_into(self, ids_flat, offsets, keep, index: "Index", rows, fmt: str = "f32") -> np.ndarray:
        """Packed documents -> their kept token vectors as the tokens of `rows` of `index`, written by the token head straight into the
        index's token pool (sc_encoder_embed_tokens_into): what embed_tokens, dropping the tokens whose keep flag is 0 and
        Index.put_tokens store, without a vector crossing to the host.  keep: one uint8 per token or None (all kept).  -> kept counts [B]."""
        ids_flat, offsets, B = self._packed_args(ids_flat, offsets)
        if keep is not None:
            keep = np.ascontiguousarray(keep, dtype=np.uint8)
            if keep.shape != ids_flat.shape:
                raise ValueError("keep must hold one flag per token")
        r = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        if r.shape[0] != B:
            raise ValueError("rows must hold one row number per text")
        counts = np.empty(B, dtype=np.int32)
        _check(lib().sc_encoder_embed_tokens_into(self.handle, _ptr(ids_flat), _ptr(offsets), B, _ptr(keep), index.handle, _ptr(r), TOKEN_FORMATS[fmt], _ptr(counts)))
        return counts

    def score_late(self, q_ids, q_offsets, d_ids, d_offsets, pair_q, pair_d, expand_id: int = -1, d_keep=None) -> np.ndarray:
        """MaxSim scores [P] of the pairs (pair_q[p], pair_d[p]) over the token vectors of the packed queries and documents; the vectors
        stay on the device.  d_keep: one uint8 per document token, 0 = left out of every maximum (punctuation); None = all kept."""
        q_ids, q_offsets, Bq = self._packed_args(q_ids, q_offsets)
        d_ids, d_offsets, Bd = self._packed_args(d_ids, d_offsets)
        pair_q = np.ascontiguousarray(pair_q, dtype=np.int32)
        pair_d = np.ascontiguousarray(pair_d, dtype=np.int32)
        if pair_q.ndim != 1 or pair_q.shape != pair_d.shape:
            raise ValueError("pair_q and pair_d must be [P]")
        if d_keep is not None:
            d_keep = np.ascontiguousarray(d_keep, dtype=np.uint8)
            if d_keep.shape != d_ids.shape:
                raise ValueError("d_keep must hold one flag per document token")
        out = np.empty(max(1, len(pair_q)), dtype=np.float32)
        _check(lib().sc_encoder_score_late(self.handle, _ptr(q_ids), _ptr(q_offsets), Bq, int(expand_id), _ptr(d_ids), _ptr(d_offsets), Bd, _ptr(d_keep),
                                           _ptr(pair_q), _ptr(pair_d), len(pair_q), _ptr(out)))
        return out[: len(pair_q)]

    def embed_ids_dev(self, ids_ptr: int, lens_ptr: int, B: int, S: int, out_ptr: int) -> None:
        _check(lib().sc_encoder_embed_ids_dev(self.handle, C.c_void_p(ids_ptr), C.c_void_p(lens_ptr), int(B), int(S), C.c_void_p(out_ptr)))


class NativeTokenizer:
    """C++ WordPiece (ASCII fast path + BERT's Unicode normalisation, multi-threaded).  encode_batch also returns which texts it
    left alone (malformed UTF-8 only)."""

    def __init__(self, vocab_path, lowercase: bool = True):
        data = Path(vocab_path).read_bytes()
        self._h = C.c_void_p()
        _check(lib().sc_tokenizer_create(data, len(data), 1 if lowercase else 0, C.byref(self._h)))
        v = [C.c_int32() for _ in range(5)]
        _check(lib().sc_tokenizer_info(self._h, *[C.byref(x) for x in v]))
        self.vocab_size, self.pad_id, self.unk_id, self.cls_id, self.sep_id = (x.value for x in v)

    def close(self) -> None:
        if self._h:
            lib().sc_tokenizer_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            if not sys.is_finalizing():
                self.close()
        except Exception:
            pass

    def encode_batch(self, texts, max_tokens: int, S: int, threads: int = 0):
        """-> (ids [n,S] int32, lens [n] int32, needs_fallback [n] bool)"""
        raw = [t.encode("utf-8") for t in texts]
        offsets = np.zeros(len(raw) + 1, dtype=np.int64)
        np.cumsum([len(r) for r in raw], out=offsets[1:])
        blob = b"".join(raw)
        n = len(raw)
        ids = np.empty((n, S), dtype=np.int32)
        lens = np.empty((n,), dtype=np.int32)
        fb = np.empty((n,), dtype=np.uint8)
        _check(lib().sc_tokenizer_encode(self._h, blob, offsets.ctypes.data_as(C.c_void_p), n, int(max_tokens), int(S),
                                         ids.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), fb.ctypes.data_as(C.c_void_p), int(threads)))
        return ids, lens, fb.astype(bool)


def diag_gemm_bf16(rt: Runtime, A, W, bias, R=None, epi: int = 0) -> np.ndarray:
    """One GEMM kernel launch on host data (parity tests): out [M,N] = A [M,K] @ W [N,K].T (+ epilogue)."""
    A = np.ascontiguousarray(A, np.float32)
    W = np.ascontiguousarray(W, np.float32)
    bias = np.ascontiguousarray(bias, np.float32)
    M, K = A.shape
    N = W.shape[0]
    out = np.empty((M, N), np.float32)
    Rp = None
    if R is not None:
        R = np.ascontiguousarray(R, np.float32)
        Rp = R.ctypes.data_as(C.c_void_p)
    _check(lib().sc_diag_gemm_bf16(rt.handle, epi, A.ctypes.data_as(C.c_void_p), W.ctypes.data_as(C.c_void_p),
                                   bias.ctypes.data_as(C.c_void_p), Rp, M, N, K, out.ctypes.data_as(C.c_void_p)))
    return out


IVF_ITEM_DTYPE = np.dtype([("row0", "<i8"), ("rows", "<i4"), ("slot_base", "<i4")])


def diag_ivf_plan(path: str, probes, list_off, k: int, ld: int, cus: int, wide: bool = True) -> "dict[str, np.ndarray]":
    """The host plan of a batched IVF probe (sc_diag_ivf_plan; no device): path "listmajor" or "coarse", probes [Q, nprobe] list ids,
    list_off [nlist + 1].  Every table the search would upload and every number it would report, by name; scalars as arrays of one."""
    probes = np.ascontiguousarray(probes, np.int64)
    list_off = np.ascontiguousarray(list_off, np.int64)
    if probes.ndim != 2 or list_off.ndim != 1 or list_off.size < 2:
        raise ValueError("diag_ivf_plan: probes must be [Q, nprobe], list_off [nlist + 1]")
    args = (path.encode(), _ptr(probes), probes.shape[0], probes.shape[1], _ptr(list_off), list_off.size - 1, int(k), int(ld), int(cus), 1 if wide else 0)
    return _diag_records(lib().sc_diag_ivf_plan, args)


def _diag_records(fn, args) -> "dict[str, np.ndarray]":
    """Calls a host-plan diag entry twice (size, then data) and cuts its named records apart."""
    need = C.c_int64()
    _check(fn(*args, None, 0, C.byref(need)))
    blob = np.empty(need.value, np.uint8)
    _check(fn(*args, _ptr(blob), blob.size, C.byref(need)))
    out, at, kinds = {}, 0, (np.dtype("<i4"), np.dtype("<i8"), np.dtype("<u4"), IVF_ITEM_DTYPE)
    while at < blob.size:
        name = blob[at:at + 16].tobytes().split(b"\0")[0].decode()
        dt = kinds[int(blob[at + 16:at + 20].view("<i4")[0])]
        n = int(blob[at + 24:at + 32].view("<i8")[0])
        out[name] = blob[at + 32:at + 32 + n * dt.itemsize].view(dt).copy()
        at += 32 + (n * dt.itemsize + 7) // 8 * 8
    return out


def diag_ivf_exact_path(ld: int, R: int, k: int, nprobe: int, cus: int) -> str:
    """The exact probe that answers a sub-batch of R queries the IVF coarse stage hands on (sc_diag_ivf_exact_path; no device):
    "ivf_listmajor", "ivf" (per-query probing) or "none"."""
    path = C.c_int32()
    _check(lib().sc_diag_ivf_exact_path(int(ld), int(R), int(k), int(nprobe), int(cus), C.byref(path)))
    return {0: "none", 3: "ivf", 4: "ivf_listmajor"}[path.value]


def diag_encoder_plan(ids, offsets, kind: str = "texts", first_lens=None, expand_id: int = -1, query: bool = False, *, max_pos: int = 2048, pos_type: int = 0,
                      vocab: int = 30522, type_vocab: int = 2, arch: int = 0, global_every: int = 0, local_window: int = 0) -> "dict[str, np.ndarray]":
    """The host plan of a packed encoder call (sc_diag_encoder_plan; no device, no encoder): kind "texts", "pairs" (first_lens), "scored" or
    "tokens" (expand_id; query: the query side of score_late), the model's bounds as keywords.  The checks of the entry points run first
    (ScError with their messages); then every array the call would upload, by name; scalars as arrays of one."""
    ids = np.ascontiguousarray(ids, np.int32)
    offsets = np.ascontiguousarray(offsets, np.int64)
    fl = None if first_lens is None else np.ascontiguousarray(first_lens, np.int32)
    args = (_ptr(ids), _ptr(offsets), offsets.size - 1, ("texts", "pairs", "scored", "tokens").index(kind), _ptr(fl), int(expand_id),
            1 if query else 0, int(max_pos), int(pos_type), int(vocab), int(type_vocab), int(arch), int(global_every), int(local_window))
    return _diag_records(lib().sc_diag_encoder_plan, args)


def diag_encoder_plan_keep(ids, offsets, keep=None, *, max_pos: int = 2048, pos_type: int = 0, vocab: int = 30522) -> "dict[str, np.ndarray]":
    """The host plan of the documents' token call under keep flags (sc_diag_encoder_plan_keep; no device, no encoder): dst [M] is -1 on
    dropped, alignment and tail rows and counts the kept rows up text after text; counts [B] the kept tokens per text."""
    ids = np.ascontiguousarray(ids, np.int32)
    offsets = np.ascontiguousarray(offsets, np.int64)
    kp = None if keep is None else np.ascontiguousarray(keep, np.uint8)
    if kp is not None and kp.shape != ids.shape:
        raise ValueError("keep must hold one flag per token")
    return _diag_records(lib().sc_diag_encoder_plan_keep, (_ptr(ids), _ptr(offsets), offsets.size - 1, _ptr(kp), int(max_pos), int(pos_type), int(vocab)))


def diag_set_option(name: str, value: int) -> None:
    """Process-wide test / tuning switch of the library (sc_diag_set_option)."""
    _check(lib().sc_diag_set_option(name.encode(), int(value)))


def diag_gemm_bench(rt: Runtime, M: int, N: int, K: int, epi: int = 0, iters: int = 20, variant: int = 0) -> float:
    """ms per launch of one GEMM shape on device-resident synthetic data (tuning aid)."""
    ms = C.c_double()
    _check(lib().sc_diag_gemm_bench(rt.handle, epi, M, N, K, iters, variant, C.byref(ms)))
    return ms.value


def diag_gemm_trace(rt: Runtime, M: int, N: int, K: int, epi: int = 0, launches: int = 1) -> np.ndarray:
    """Per-workgroup time stamps of back-to-back 256-tile GEMM launches: [launches, ntiles, 8] uint64 (see include/semcode_hip.h)."""
    nt = (M // 256) * (N // 256)
    out = np.zeros((launches, nt, 8), np.uint64)
    _check(lib().sc_diag_gemm_trace(rt.handle, epi, M, N, K, out.ctypes.data_as(C.c_void_p), out.size))
    return out


def diag_gemm_i8(rt: Runtime, A, W) -> np.ndarray:
    """out [M,N] int32 = A [M,K] int8 @ W [N,K].T on the int8 form of the 256 tile (exact)."""
    A = np.ascontiguousarray(A, np.int8)
    W = np.ascontiguousarray(W, np.int8)
    M, K = A.shape
    N = W.shape[0]
    out = np.empty((M, N), np.int32)
    _check(lib().sc_diag_gemm_i8(rt.handle, A.ctypes.data_as(C.c_void_p), W.ctypes.data_as(C.c_void_p), M, N, K, out.ctypes.data_as(C.c_void_p)))
    return out


def diag_rope(rt: Runtime, qk, S: int, heads: int, theta: float) -> np.ndarray:
    """The stand-alone rotary kernel on qk [rows, heads * 64] (row r = position r % S): the rotated values, bf16-rounded."""
    out = np.array(qk, dtype=np.float32, order="C")
    rows = out.shape[0]
    if out.shape != (rows, heads * 64):
        raise ValueError("qk must be [rows, heads * 64]")
    _check(lib().sc_diag_rope(rt.handle, out.ctypes.data_as(C.c_void_p), rows, int(S), int(heads), float(theta)))
    return out


def diag_rel_buckets(rel_buckets: int, max_distance: int, span: int) -> np.ndarray:
    """T5's bucket rule as the library evaluates it: [2 span - 1] int32, entry d + span - 1 = bucket(d), d = key - query.  No device."""
    out = np.empty(max(2 * int(span) - 1, 1), np.int32)  # (a span below 1 is the library's to refuse)
    _check(lib().sc_diag_rel_buckets(int(rel_buckets), int(max_distance), int(span), out.ctypes.data_as(C.c_void_p)))
    return out


def diag_output_proj(rt: Runtime, x, W, b=None, normalize: bool = True) -> np.ndarray:
    """output_proj_kernel on its own: x [B, H] f32, W [E, H], b [E] or None -> [B, E] = W x + b, L2-normalised if asked."""
    x, W = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(W, np.float32)
    b = None if b is None else np.ascontiguousarray(b, np.float32)
    out = np.empty((x.shape[0], W.shape[0]), np.float32)
    _check(lib().sc_diag_output_proj(rt.handle, x.ctypes.data_as(C.c_void_p), x.shape[0], x.shape[1], W.ctypes.data_as(C.c_void_p),
                                     None if b is None else b.ctypes.data_as(C.c_void_p), W.shape[0], 1 if normalize else 0, out.ctypes.data_as(C.c_void_p)))
    return out


# ---- single-kernel diagnostics of the LayerNorm-folded pipeline and the stand-alone encoder kernels (tests/test_fold_kernels_gpu.py)
EPI_LNA_BIAS, EPI_LNA_GELU, EPI_RESLN_STATS, EPI_LNA_BIAS_ROPE = 3, 4, 5, 6


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def block64(a: np.ndarray) -> np.ndarray:
    """[M, N] row-major -> [N / 64, M, 64]: the 64-column blocks the QKV and FFN1 epilogues write (SC_LDC_BLOCKED64)."""
    M, N = a.shape
    return np.ascontiguousarray(a.reshape(M, N // 64, 64).transpose(1, 0, 2))


def unblock64(a: np.ndarray, M: int, N: int) -> np.ndarray:
    """Inverse of block64."""
    return np.ascontiguousarray(np.asarray(a).reshape(N // 64, M, 64).transpose(1, 0, 2).reshape(M, N))


ATTN_FULL, ATTN_WINDOW, ATTN_CAUSAL, ATTN_CLS = range(4)


class DiagAttn(C.Structure):
    """sc_diag_attn of include/semcode_hip.h."""
    _fields_ = [(n, C.c_int32) for n in ("mask", "B", "S", "heads", "kv_heads", "head_dim", "blocked_rows", "local_window")] + \
               [(n, C.c_void_p) for n in ("starts", "lens", "slopes", "rel_bias")] + [("rel_buckets", C.c_int32), ("rel_max_distance", C.c_int32)]


def _diag_attention_rows(starts, lens, S: int = 0, blocked_rows: int = 0) -> int:
    """Rows of qkv one attention launch reads: blocked_rows if given, else B * S (starts None) or the last sequence's end rounded up to 256."""
    if blocked_rows:
        return int(blocked_rows)
    return len(lens) * int(S) if starts is None else (int((np.asarray(starts) + (np.asarray(lens) + 31) // 32 * 32).max()) + 255) // 256 * 256


def _diag_attention(rt, mask: int, qkv, lens, heads: int, B=None, S: int = 0, starts=None, kv_heads: int = 0, head_dim: int = 64, blocked_rows: int = 0,
                    local_window: int = 0, slopes=None, rel_bias=None, max_distance: int = 0) -> np.ndarray:
    """One sc_diag_attention_run call.  qkv [R, (heads + 2 kv_heads) * head_dim] row-major as [Q | K | V] (kv_heads = heads but under the causal
    mask), R = _diag_attention_rows; a rectangle may come as its B * S rows alone and is padded with zero rows.  blocked_rows > 0 hands it over
    in 64-column blocks.  -> [B, H] (CLS), [B * S, H] (rectangle) or [R, H] (packed), H = heads * head_dim."""
    qkv, lens = _f32(qkv), np.ascontiguousarray(lens, np.int32)
    starts = None if starts is None else np.ascontiguousarray(starts, np.int32)
    sl, rb = (None if a is None else _f32(a) for a in (slopes, rel_bias))
    B, S, heads, head_dim = len(lens) if B is None else int(B), int(S), int(heads), int(head_dim)
    H, cols = heads * head_dim, (heads + 2 * (int(kv_heads) if mask == ATTN_CAUSAL else heads)) * head_dim
    R = _diag_attention_rows(starts, lens[:B], S, blocked_rows)
    if starts is None and qkv.shape == (B * S, cols) and R > B * S:
        qkv = np.concatenate([qkv, np.zeros((R - B * S, cols), np.float32)])
    if qkv.shape != (R, cols) or lens.ndim != 1 or len(lens) < B or (starts is not None and starts.shape != lens.shape):
        raise ValueError(f"diag_attention: qkv must be [{R}, {cols}], lens (and starts, if given) [B]")
    if blocked_rows:
        qkv = block64(qkv)
    out = np.empty((B if mask == ATTN_CLS else B * S if starts is None else R, H), np.float32)
    addr = lambda a: None if a is None else a.ctypes.data
    desc = DiagAttn(mask, B, S, heads, int(kv_heads), head_dim, int(blocked_rows), int(local_window), addr(starts), addr(lens), addr(sl), addr(rb),
                    0 if rb is None else rb.shape[0], int(max_distance))
    _check(lib().sc_diag_attention_run(None if rt is None else rt.handle, C.addressof(desc), _ptr(qkv), _ptr(out)))
    return out


def diag_attention(rt: Runtime, qkv, lens, B: int, S: int, heads: int, head_dim: int = 64, blocked_rows: int = 0) -> np.ndarray:
    return _diag_attention(rt, ATTN_FULL, qkv, lens, heads, B=B, S=S, head_dim=head_dim, blocked_rows=blocked_rows)


def diag_attention_ex(rt: Runtime, qkv, lens, B: int, S: int, heads: int, blocked_rows: int = 0, slopes=None, head_dim: int = 64) -> np.ndarray:
    """sc_launch_attention as the pipelines call it: blocked_rows > 0 lays qkv [B*S, 3H] out as [3H/64][blocked_rows][64] (rows beyond
    B*S zero); slopes [heads] = ALiBi; head_dim 64 or 32 (H = heads * head_dim)."""
    return _diag_attention(rt, ATTN_FULL, qkv, lens, heads, B=B, S=S, head_dim=head_dim, blocked_rows=blocked_rows, slopes=slopes)


def diag_attention_bias(rt: Runtime, qkv, lens, B: int, S: int, heads: int, rel_bias, max_distance: int, blocked_rows: int = 0) -> np.ndarray:
    """sc_launch_attention_rel as the T5 forward calls it: diag_attention_ex with rel_bias [buckets, heads] in place of slopes."""
    return _diag_attention(rt, ATTN_FULL, qkv, lens, heads, B=B, S=S, blocked_rows=blocked_rows, rel_bias=rel_bias, max_distance=max_distance)


def diag_attention_cls(rt: Runtime, qkv, lens, B: int, S: int, heads: int, head_dim: int = 64, slopes=None) -> np.ndarray:
    """attention_cls_kernel on its own: qkv [B*S, 3H] row-major, one query row per text (its first) -> [B, H], H = heads * head_dim."""
    return _diag_attention(rt, ATTN_CLS, qkv, lens, heads, B=B, S=S, head_dim=head_dim, slopes=slopes)


def diag_attention_packed(rt: Runtime, qkv, starts, lens, heads: int, blocked_rows: int = 0, slopes=None, head_dim: int = 64) -> np.ndarray:
    """The packed attention kernel on its own: qkv [R, 3H] row-major, sequence b on the rows starts[b] .. starts[b] + ceil32(lens[b]);
    R = blocked_rows (> 0: handed over as [3H/64][R][64]) or the last sequence's end rounded up to 256.  -> [R, H], H = heads * head_dim."""
    return _diag_attention(rt, ATTN_FULL, qkv, lens, heads, starts=starts, head_dim=head_dim, blocked_rows=blocked_rows, slopes=slopes)


def diag_attention_bias_packed(rt: Runtime, qkv, starts, lens, heads: int, rel_bias, max_distance: int, blocked_rows: int = 0) -> np.ndarray:
    """The packed form: diag_attention_packed with rel_bias [buckets, heads] in place of slopes."""
    return _diag_attention(rt, ATTN_FULL, qkv, lens, heads, starts=starts, blocked_rows=blocked_rows, rel_bias=rel_bias, max_distance=max_distance)


def diag_attention_window(rt: Runtime, qkv, lens, heads: int, local_window: int, S: int = 0, starts=None, blocked_rows: int = 0) -> np.ndarray:
    """The windowed attention kernels on their own (head dimension 64): a query sees the real keys with |i - j| <= local_window / 2.
    starts None: a rectangle, qkv [B*S, 3H] -> [B*S, H].  Else packed rows as diag_attention_packed: qkv [R, 3H] -> [R, H]."""
    return _diag_attention(rt, ATTN_WINDOW, qkv, lens, heads, S=S, starts=starts, blocked_rows=blocked_rows, local_window=local_window)


def diag_attention_causal(rt: Runtime, qkv, lens, heads: int, kv_heads: int, S: int = 0, starts=None, blocked_rows: int = 0, head_dim: int = 64) -> np.ndarray:
    """The causal grouped-query attention kernels on their own (head dimension 64 or 128): a query sees the real keys at or before its own
    position; query head h reads K / V head h // (heads // kv_heads).  qkv columns are [Q (heads) | K (kv_heads) | V (kv_heads)] x head_dim.
    starts None: a rectangle, qkv [B*S, (heads + 2 kv_heads) * head_dim] -> [B*S, heads * head_dim].  Else packed rows as diag_attention_packed."""
    return _diag_attention(rt, ATTN_CAUSAL, qkv, lens, heads, S=S, starts=starts, kv_heads=kv_heads, head_dim=head_dim, blocked_rows=blocked_rows)


def diag_ffn_act(rt: Runtime, kind: int, h) -> np.ndarray:
    """The kernel between the two FFN GEMMs, kind = ffn_type.  1 GEGLU, 2 SwiGLU, 4 the tanh-GELU gate: h [rows, 2F] (gate | up) -> act(gate) * up;
    3: the ReLU pass on h [rows, F].  bf16-rounded, [rows, F]."""
    h = _f32(h)
    rows, F = h.shape[0], h.shape[1] // (1 if kind == 3 else 2)
    out = np.empty((rows, F), np.float32)
    _check(lib().sc_diag_ffn_act(rt.handle, int(kind), _ptr(h), rows, F, _ptr(out)))
    return out


def diag_geglu(rt: Runtime, h) -> np.ndarray:
    """The GEGLU kernel on h [rows, 2F] (gate | up): gelu(gate) * up, bf16-rounded, [rows, F]."""
    return diag_ffn_act(rt, 1, h)


def diag_swiglu(rt: Runtime, h) -> np.ndarray:
    """The SwiGLU kernel on h [rows, 2F] (gate | up): silu(gate) * up, bf16-rounded, [rows, F]."""
    return diag_ffn_act(rt, 2, h)


def diag_fold_ln(rt: Runtime, W, gamma, beta, bias=None):
    """fold_ln_weights_kernel: (Wf [N,K] bf16 values, c1 [N], c2 [N])."""
    W, gamma, beta = _f32(W), _f32(gamma), _f32(beta)
    bias = None if bias is None else _f32(bias)
    N, K = W.shape
    Wf, c1, c2 = np.empty((N, K), np.float32), np.empty(N, np.float32), np.empty(N, np.float32)
    _check(lib().sc_diag_fold_ln(rt.handle, _ptr(W), _ptr(gamma), _ptr(beta), _ptr(bias), N, K, _ptr(Wf), _ptr(c1), _ptr(c2)))
    return Wf, c1, c2


def diag_gemm_lna(rt: Runtime, epi: int, A, Wf, c1, c2, stats_in, eps: float, blocked: bool = False, rope_S: int = 0, rope_theta: float = 0.0,
                  rope_ncols: int = 0):
    """One EPI_LNA_* GEMM launch: (C [M,N], fin [M,2]).  stats_in [K/256, M, 2]; blocked: C written in 64-column blocks (un-blocked here)."""
    A, Wf, c1, c2, stats_in = _f32(A), _f32(Wf), _f32(c1), _f32(c2), _f32(stats_in)
    M, K = A.shape
    N = Wf.shape[0]
    if stats_in.shape != (K // 256, M, 2) or Wf.shape != (N, K) or c1.shape != (N,) or c2.shape != (N,):
        raise ValueError("diag_gemm_lna: shapes")
    Cc, fin = np.empty((M, N), np.float32), np.empty((M, 2), np.float32)
    _check(lib().sc_diag_gemm_lna(rt.handle, epi, 1 if blocked else 0, _ptr(A), _ptr(Wf), _ptr(c1), _ptr(c2), _ptr(stats_in), float(eps), M, N, K,
                                  int(rope_S), float(rope_theta), int(rope_ncols), _ptr(Cc), _ptr(fin)))
    return (unblock64(Cc, M, N) if blocked else Cc), fin


def diag_gemm_strip(M: int = 0, N: int = 0, K: int = 0, cus: int = 0) -> int:
    """Tiles per strip the EPI_LNA_* launcher picks for this shape under the current options (0 = per-tile kernel); no launch, and
    no device when cus > 0.  M == 0: what the most recent EPI_LNA_* launch of this process used."""
    return int(lib().sc_diag_gemm_strip(int(M), int(N), int(K), int(cus)))


def diag_gemm_resln(rt: Runtime, A, W, bias, gam, R, fin, eps: float, a_blocked: bool = False):
    """One EPI_RESLN_STATS GEMM launch: (C [M,N], stats_out [N/256, M, 2]).  a_blocked: A handed over in 64-column blocks."""
    A, W, bias, gam, R, fin = _f32(A), _f32(W), _f32(bias), _f32(gam), _f32(R), _f32(fin)
    M, K = A.shape
    N = W.shape[0]
    if W.shape != (N, K) or R.shape != (M, N) or fin.shape != (M, 2) or bias.shape != (N,) or gam.shape != (N,):
        raise ValueError("diag_gemm_resln: shapes")
    Ad = block64(A) if a_blocked else A
    Cc, st = np.empty((M, N), np.float32), np.empty((N // 256, M, 2), np.float32)
    _check(lib().sc_diag_gemm_resln(rt.handle, 1 if a_blocked else 0, _ptr(Ad), _ptr(W), _ptr(bias), _ptr(gam), _ptr(R), _ptr(fin), float(eps), M, N, K,
                                    _ptr(Cc), _ptr(st)))
    return Cc, st


GEMM_PATH_FIELDS = ("tile", "splitk", "order", "pp", "nt")


def diag_gemm_bf16_ex(rt: Runtime, A, W, bias, R=None, epi: int = 0, c_blocked: bool = False, a_blocked: bool = False, splitk: bool = False,
                      tile128: bool = False):
    """One plain GEMM launch in the forms the forward passes use: (out [M,N], path).  c_blocked: C written in 64-column blocks (un-blocked
    here); a_blocked: A handed over in 64-column blocks; splitk: the split-K scratch is offered; tile128: the 128-tile kernel is forced.
    path = what the launcher ran, by GEMM_PATH_FIELDS.  The library checks the arguments before it looks at rt (None reaches them)."""
    A, W, bias = _f32(A), _f32(W), _f32(bias)
    R = None if R is None else _f32(R)
    M, K = A.shape
    N = W.shape[0]
    if W.shape != (N, K) or bias.shape != (N,) or (R is not None and R.shape != (M, N)):
        raise ValueError("diag_gemm_bf16_ex: shapes")
    Ad = block64(A) if a_blocked and K % 64 == 0 else A
    out, path = np.empty((M, N), np.float32), np.zeros(5, np.int32)
    flags = (1 if c_blocked else 0) | (2 if a_blocked else 0) | (4 if splitk else 0) | (8 if tile128 else 0)
    _check(lib().sc_diag_gemm_bf16_ex(None if rt is None else rt.handle, int(epi), flags, _ptr(Ad), _ptr(W), _ptr(bias), _ptr(R), M, N, K, _ptr(out),
                                      _ptr(path)))
    return (unblock64(out, M, N) if c_blocked else out), dict(zip(GEMM_PATH_FIELDS, (int(v) for v in path)))


def diag_gemm_path(M: int = 0, N: int = 0, K: int = 0, cus: int = 0, splitk: bool = False) -> "dict[str, int]":
    """The kernel the plain GEMM launcher picks for this shape under the current options, by GEMM_PATH_FIELDS; no launch, and no device
    when cus > 0.  M == 0: what the most recent plain launch of this process ran."""
    path = np.zeros(5, np.int32)
    _check(lib().sc_diag_gemm_path(int(M), int(N), int(K), int(cus), 1 if splitk else 0, _ptr(path)))
    return dict(zip(GEMM_PATH_FIELDS, (int(v) for v in path)))


def diag_gemm_splitk(M: int, N: int, K: int, cus: int = 0) -> int:
    """K slices the split-K rule gives this shape on a device with `cus` compute units (1 = no split; cus 0: the current device's)."""
    return int(lib().sc_diag_gemm_splitk(int(M), int(N), int(K), int(cus)))


def diag_qknorm_rope(rt: Runtime, x, heads: int, kv_heads: int, head_dim: int, S: int, theta: float, pos=None, gamma_q=None, gamma_k=None,
                     eps: float = 1e-6) -> np.ndarray:
    """qknorm_rope_kernel (pos None: row r = position r % S) or its packed form (pos [rows]; S = the table's length) on
    x [rows, (heads + 2 kv_heads) * head_dim] as [Q | K | V]: the Q and K heads RMS-normalised per head (gamma_q, gamma_k [head_dim]; both
    None: no norm) and rotated, the V columns untouched; everything bf16-rounded."""
    out = np.array(x, dtype=np.float32, order="C")
    rows = out.shape[0]
    if out.shape != (rows, (heads + 2 * kv_heads) * head_dim):
        raise ValueError("x must be [rows, (heads + 2 kv_heads) * head_dim]")
    if pos is not None:
        pos = np.ascontiguousarray(pos, np.int32)
        if pos.shape != (rows,):
            raise ValueError("pos must be [rows]")
    gq = None if gamma_q is None else _f32(gamma_q)
    gk = None if gamma_k is None else _f32(gamma_k)
    _check(lib().sc_diag_qknorm_rope(rt.handle, _ptr(out), rows, int(S), None if pos is None else _ptr(pos), int(heads), int(kv_heads), int(head_dim),
                                     float(theta), None if gq is None else _ptr(gq), None if gk is None else _ptr(gk), float(eps)))
    return out


def diag_rmsnorm(rt: Runtime, x, gamma, eps: float) -> np.ndarray:
    """rmsnorm_kernel: x [tokens, H] -> x * rsqrt(mean(x^2) + eps) * gamma, rows rounded to bf16 on the way in and out."""
    x, gamma = _f32(x), _f32(gamma)
    out = np.empty_like(x)
    _check(lib().sc_diag_rmsnorm(rt.handle, _ptr(x), x.shape[0], x.shape[1], _ptr(gamma), float(eps), _ptr(out)))
    return out


def diag_layernorm(rt: Runtime, x, gamma, beta, eps: float) -> np.ndarray:
    x, gamma, beta = _f32(x), _f32(gamma), _f32(beta)
    out = np.empty_like(x)
    _check(lib().sc_diag_layernorm(rt.handle, _ptr(x), x.shape[0], x.shape[1], _ptr(gamma), _ptr(beta), float(eps), _ptr(out)))
    return out


def diag_mean_pool(rt: Runtime, x, lens, S: int, normalize: bool) -> np.ndarray:
    """x [B*S, H] -> [B, H] f32 (normalize False: the sliced kernel; True: the one-workgroup kernel + L2 normalisation)."""
    x = _f32(x)
    lens = np.ascontiguousarray(lens, np.int32)
    B, H = lens.size, x.shape[1]
    out = np.empty((B, H), np.float32)
    _check(lib().sc_diag_mean_pool(rt.handle, _ptr(x), _ptr(lens), B, int(S), H, 1 if normalize else 0, _ptr(out)))
    return out


def diag_mean_pool_ln(rt: Runtime, y, stats, gamma, beta, eps: float, lens, S: int) -> np.ndarray:
    """y [tokens_pad, H] raw rows, stats [slots, tokens_pad, 2] -> [B, H] f32 = masked mean of LayerNorm(y)."""
    y, stats, gamma, beta = _f32(y), _f32(stats), _f32(gamma), _f32(beta)
    lens = np.ascontiguousarray(lens, np.int32)
    B, (tp, H) = lens.size, y.shape
    if stats.shape[1:] != (tp, 2):
        raise ValueError("diag_mean_pool_ln: stats must be [slots, tokens_pad, 2]")
    out = np.empty((B, H), np.float32)
    _check(lib().sc_diag_mean_pool_ln(rt.handle, _ptr(y), _ptr(stats), stats.shape[0], tp, _ptr(gamma), _ptr(beta), float(eps), _ptr(lens), B, int(S), H,
                                      _ptr(out)))
    return out


def diag_embed(rt: Runtime, ids, wemb, pemb, temb, max_pos: int, ln=None, tokens_pad: int = 0, slots: int = 1):
    """The embedding kernels on ids [B, S].  ln None: embed_raw_kernel -> (rows [tokens_pad, H], stats [slots, tokens_pad, 2]);
    ln = (gamma, beta, eps): embed_ln_kernel -> rows [B*S, H].  pemb None: no position table."""
    ids = np.ascontiguousarray(ids, np.int32)
    S, tokens = ids.shape[1], ids.size
    wemb, temb = _f32(wemb), _f32(temb)
    pemb = None if pemb is None else _f32(pemb)
    vocab, H = wemb.shape
    if ln is None:
        tp = max(int(tokens_pad), tokens)
        rows, stats = np.empty((tp, H), np.float32), np.empty((slots, tp, 2), np.float32)
        _check(lib().sc_diag_embed(rt.handle, 0, _ptr(ids), tokens, S, H, vocab, int(max_pos), _ptr(wemb), _ptr(pemb), _ptr(temb), None, None, 0.0, tp,
                                   int(slots), _ptr(rows), _ptr(stats)))
        return rows, stats
    gamma, beta = _f32(ln[0]), _f32(ln[1])
    rows = np.empty((tokens, H), np.float32)
    _check(lib().sc_diag_embed(rt.handle, 1, _ptr(ids), tokens, S, H, vocab, int(max_pos), _ptr(wemb), _ptr(pemb), _ptr(temb), _ptr(gamma), _ptr(beta),
                               float(ln[2]), 0, 0, _ptr(rows), None))
    return rows


def topk_merge_host(metric: str, dist: np.ndarray, rows: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """Merge per-shard results dist/rows [lists, Q, k] -> global best-first [Q, k]."""
    d = np.ascontiguousarray(dist, dtype=np.float32)
    r = np.ascontiguousarray(rows, dtype=np.int64)
    if d.ndim != 3 or d.shape != r.shape:
        raise ValueError("dist and rows must both be [lists, Q, k]")
    lists, Q, k = d.shape
    od, orow = _result_arrays(Q, k)
    _check(lib().sc_topk_merge_host(METRICS[metric], lists, Q, k, d.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p),
                                    od.ctypes.data_as(C.c_void_p), orow.ctypes.data_as(C.c_void_p)))
    return od, orow


def diag_embed_pairs(rt: Runtime, ids, pos, types, wemb, pemb, temb, max_pos: int, ln=None, tokens_pad: int = 0, slots: int = 1):
    """The typed embedding kernels on ids / pos / types [tokens]: diag_embed with a position and a segment id per row; temb [type_vocab, H]."""
    ids, pos, types = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in (ids, pos, types))
    tokens = ids.size
    wemb, temb = _f32(wemb), _f32(temb)
    pemb = None if pemb is None else _f32(pemb)
    vocab, H = wemb.shape
    if ln is None:
        tp = max(int(tokens_pad), tokens)
        rows, stats = np.empty((tp, H), np.float32), np.empty((slots, tp, 2), np.float32)
        _check(lib().sc_diag_embed_pairs(rt.handle, 0, _ptr(ids), _ptr(pos), _ptr(types), tokens, H, vocab, int(max_pos), temb.shape[0], _ptr(wemb), _ptr(pemb),
                                         _ptr(temb), None, None, 0.0, tp, int(slots), _ptr(rows), _ptr(stats)))
        return rows, stats
    gamma, beta = _f32(ln[0]), _f32(ln[1])
    rows = np.empty((tokens, H), np.float32)
    _check(lib().sc_diag_embed_pairs(rt.handle, 1, _ptr(ids), _ptr(pos), _ptr(types), tokens, H, vocab, int(max_pos), temb.shape[0], _ptr(wemb), _ptr(pemb),
                                     _ptr(temb), _ptr(gamma), _ptr(beta), float(ln[2]), 0, 0, _ptr(rows), None))
    return rows


def diag_pair_head(rt: Runtime, cls, cls_w, cls_b, pooler_w=None, pooler_b=None) -> np.ndarray:
    """pair_head_kernel on cls [B, H]: logits [B, num_labels] = cls_w p + cls_b, p = tanh(pooler_w cls + pooler_b) or cls."""
    cls, cls_w, cls_b = _f32(cls), _f32(cls_w), _f32(cls_b)
    B, H = cls.shape
    nl = cls_w.shape[0]
    pooler_w = None if pooler_w is None else _f32(pooler_w)
    pooler_b = None if pooler_w is None else _f32(pooler_b)
    out = np.empty((B, nl), np.float32)
    _check(lib().sc_diag_pair_head(rt.handle, _ptr(cls), B, H, _ptr(pooler_w), _ptr(pooler_b), _ptr(cls_w), _ptr(cls_b), nl, _ptr(out)))
    return out


SCORE_POOLING = {"mean": 0, "cls": 1, "last": 2}


def score_head_struct(head: dict, hidden: int) -> "tuple[ScoreHead, list]":
    """head = {kind: 1 | 2, pooling: "mean" | "cls" | "last" (or 0 / 1 / 2), cls_w [num_labels, H], cls_b or None, and for kind 1 dense_w [H, H],
    dense_b or None, norm_g [H], norm_b or None, norm_eps} -> (sc_score_head, the arrays it points into: keep them alive for the call)."""
    pooling = head.get("pooling", "last" if head.get("kind") == 2 else "cls")
    st = ScoreHead(kind=int(head.get("kind", 0)), pooling=int(SCORE_POOLING.get(pooling, pooling)), norm_eps=float(head.get("norm_eps", 0.0)))
    keep = []
    for name, shape in (("dense_w", (hidden, hidden)), ("dense_b", (hidden,)), ("norm_g", (hidden,)), ("norm_b", (hidden,)), ("cls_w", (-1, hidden)), ("cls_b", (-1,))):
        a = head.get(name)
        if a is None:
            continue
        a = _f32(a).reshape(shape)
        keep.append(a)
        setattr(st, name, a.ctypes.data)
    cls_w, cls_b = head.get("cls_w"), head.get("cls_b")
    st.num_labels = int(head["num_labels"]) if "num_labels" in head else (0 if cls_w is None else int(_f32(cls_w).reshape(-1, hidden).shape[0]))
    if cls_w is not None and cls_b is not None and _f32(cls_b).size != _f32(cls_w).size // hidden:
        raise ValueError("cls_w must be [num_labels, hidden] and cls_b [num_labels]")
    return st, keep


def diag_score_head(rt: Runtime, rows, head: dict) -> np.ndarray:
    """score_head_kernel (kind 1) / score_linear_kernel (kind 2) on rows [B, H] f32 as they are -> logits [B, num_labels]."""
    rows = _f32(rows)
    B, H = rows.shape
    st, _keep = score_head_struct(head, H)
    out = np.empty((B, max(1, int(st.num_labels))), np.float32)
    _check(lib().sc_diag_score_head(rt.handle, _ptr(rows), B, H, C.byref(st), _ptr(out)))
    return out
