"""ctypes binding of libcrisperwhisper.so (include/crisperwhisper.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C crisperwhisper_amd/csrc``.
There is no CPU fallback: if the library is missing or fails to load, every use raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# CW_LIB_PATH: a development build of the same library (A/B of compile-time variants, e.g. -DCW_PHASE_TIMING); never a fallback
LIB_PATH = os.environ.get("CW_LIB_PATH") or os.path.join(_HERE, "libcrisperwhisper.so")

CW_DTYPE_F32, CW_DTYPE_BF16, CW_DTYPE_F16 = 0, 1, 2
N_SAMPLES, N_FRAMES, N_CTX = 480000, 3000, 1500
STAGES = ("mel", "encoder", "cross_kv", "decode", "timestamps")
ALIGN_HEADS_MAX_BYTES = 8 << 30   # CW_ALIGN_HEADS_MAX_BYTES: attention rows one cw_align_heads call may capture


class NativeLibraryError(RuntimeError):
    pass


class ModelDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "d_model", "n_heads", "ffn_dim", "enc_layers", "dec_layers", "n_mels", "vocab_size",
        "max_target_positions", "median_filter_width", "dtype", "max_batch", "n_align")] + [
        ("align_layers", C.POINTER(C.c_int32)), ("align_heads", C.POINTER(C.c_int32))]


class GenCfg(C.Structure):
    _fields_ = [("eos_token_id", C.c_int32), ("pad_token_id", C.c_int32),
                ("no_timestamps_token_id", C.c_int32), ("max_initial_timestamp_index", C.c_int32),
                ("suppress_tokens", C.POINTER(C.c_int32)), ("n_suppress", C.c_int32),
                ("begin_suppress_tokens", C.POINTER(C.c_int32)), ("n_begin_suppress", C.c_int32)]


class TranscribeCfg(C.Structure):
    _fields_ = [("sot_token", C.c_int32), ("language_token", C.c_int32), ("task_token", C.c_int32),
                ("max_new_tokens", C.c_int32), ("min_new_tokens", C.c_int32), ("max_length", C.c_int32),
                ("lang_ids", C.POINTER(C.c_int32)), ("n_lang_ids", C.c_int32)]


_P = C.c_void_p
_I = C.c_int32


class GemmEpiArgs(C.Structure):
    """cw_test_gemm_epi_args (include/crisperwhisper.h)"""
    _fields_ = [(n, _I) for n in ("epi", "fp8", "M", "N", "K", "conv", "n_rows", "T_out", "C_in", "stride", "nb")] + [
        (n, _P) for n in ("row_off", "row_valid", "A", "W", "bias", "resid", "pos")] + [
        (n, _I) for n in ("ldo", "T", "S_pad", "H", "d_model")] + [(n, _P) for n in ("out", "out1", "out2")]


class FoldArgs(C.Structure):
    """cw_test_fold_args (include/crisperwhisper.h)"""
    _fields_ = [(n, _I) for n in ("op", "N", "J", "K")] + [("scale", C.c_float)] + [
        (n, _P) for n in ("a", "s", "v", "w16", "out16", "c_out", "w_out", "image")]


class StackSegArgs(C.Structure):
    """cw_test_stack_seg (include/crisperwhisper.h)"""
    _fields_ = [(n, _P) for n in ("x", "bias", "wsum", "resid")] + [(n, _I) for n in ("n_tiles", "nt", "epi", "pstats_blocks")] + [
        (n, _P) for n in ("out", "out2", "pstats")]


class GemvStackArgs(C.Structure):
    """cw_test_gemv_stack_args (include/crisperwhisper.h)"""
    _fields_ = [(n, _I) for n in ("Mb", "K", "nt", "wpk", "nseg")] + [("W", _P), ("seg", StackSegArgs * 3), ("zero", _P),
                                                                     ("zero_n4", _I)]


class GemvEpiArgs(C.Structure):
    """cw_test_gemv_epi_args (include/crisperwhisper.h)"""
    _fields_ = [(n, _I) for n in ("op", "epi", "Mb", "N", "K", "ldo", "wpk", "x16", "inplace", "frag_in", "H", "cap", "d_model",
                                  "n_pstats", "n_stats")] + [
        (n, _P) for n in ("x", "W", "bias", "ln_g", "ln_b", "resid", "part_o", "part_ml", "pstats", "pos", "cvec_in", "stats_in",
                          "wsum", "out", "sk", "sv", "y", "stats", "cvec", "nt", "frag_tail_ok")]


_SIGS = {
    "cw_abi_version": (_I, []),
    "cw_create": (_P, [C.POINTER(ModelDesc), _I]),
    "cw_destroy": (None, [_P]),
    "cw_last_error": (C.c_char_p, [_P]),
    "cw_sync": (_I, [_P]),
    "cw_load_tensor": (_I, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), _I]),
    "cw_check_weights": (_I, [_P]),
    "cw_set_generation": (_I, [_P, C.POINTER(GenCfg)]),
    "cw_mel": (_I, [_P, _P, _I, _P, _P, _P]),
    "cw_upload_pcm": (_I, [_P, _P, _I, _P]),
    "cw_mel_resident": (_I, [_P, _I]),
    "cw_set_features": (_I, [_P, _P, _I]),
    "cw_encode": (_I, [_P, _I, _P, _P, _P]),
    "cw_get_encoder_output": (_I, [_P, _P, _I]),
    "cw_decode": (_I, [_P, _I, _P, _I, _I, _I, _P, _P, _P, _P]),
    "cw_set_thresholds": (_I, [_P, C.c_float, C.c_float]),
    "cw_set_sampling": (_I, [_P, C.c_float, C.c_uint64, _P, _I]),
    "cw_decode_rows": (_I, [_P, _I, _P, _I, _I, _I, _P, _P, _P, _P, _P]),
    "cw_no_speech_probs": (_I, [_P, _I, _I, _P]),
    "cw_detect_language": (_I, [_P, _I, _I, _P, _I, _P, _P, _P]),
    "cw_test_language_probs": (_I, [_P, _P, _I, _P, _I, _I, _P, _P, _P]),
    "cw_get_transcribe_languages": (_I, [_P, _P, _P, _I]),
    "cw_get_avg_logprobs": (_I, [_P, _P, _I]),
    "cw_set_token_logprobs": (_I, [_P, _I]),
    "cw_get_token_logprobs": (_I, [_P, _P, _I]),
    "cw_get_transcribe_token_logprobs": (_I, [_P, _P, _I, _I]),
    "cw_set_top_logprobs": (_I, [_P, _I]),
    "cw_get_top_logprobs": (_I, [_P, _P, _P, _I]),
    "cw_get_transcribe_top_logprobs": (_I, [_P, _P, _P, _I, _I]),
    "cw_set_token_entropy": (_I, [_P, _I]),
    "cw_get_token_entropy": (_I, [_P, _P, _I]),
    "cw_get_transcribe_token_entropy": (_I, [_P, _P, _I, _I]),
    "cw_set_sequence_bias": (_I, [_P, _I, _P, _P, _P]),
    "cw_get_logits": (_I, [_P, _P, _I]),
    "cw_set_logits_capture": (_I, [_P, _P, _I]),
    "cw_get_alignment": (_I, [_P, _P, _I, _I]),
    "cw_resampled_length": (C.c_int64, [C.c_int64, _I, _I]),
    "cw_ingest": (_I, [_P, _P, _I, _I, C.c_int64, _I, _I, _I, _P]),
    "cw_resample_taps": (_I, [_I, _I, _P, _I, _P, _P, _P]),
    "cw_flac_info": (_I, [_P, C.c_int64, _P, _P, _P, _P]),
    "cw_flac_decode": (_I, [_P, C.c_int64, _P, C.c_int64, _P]),
    "cw_flac_last_error": (C.c_char_p, []),
    "cw_token_timestamps": (_I, [_P, _I, _I, _I, _P, _P]),
    "cw_beam_begin": (_I, [_P, _I, _I, _P, _I, _I, _I]),
    "cw_beam_step": (_I, [_P, _I, _P, _P]),
    "cw_beam_advance": (_I, [_P, _P, _P]),
    "cw_beam_finish": (_I, [_P, _I, _I, _P]),
    "cw_transcribe": (_I, [_P, _I, _P, C.POINTER(TranscribeCfg), _P, _P, _P, _I, _P]),
    "cw_transcribe_prompted": (_I, [_P, _I, _P, C.POINTER(TranscribeCfg), _P, _I, _P, _P, _P, _I, _P]),
    "cw_align_tokens": (_I, [_P, _I, _P, _P, _I, _P, _I, _P]),
    "cw_align_prefill_runs": (_I, [_P]),
    "cw_align_heads": (_I, [_P, _I, _P, _P, _I, _P, _I, _I, _P, _P, _P, _P, _P, _I, _P]),
    "cw_align_heads_times": (_I, [_P, _P]),
    "cw_test_align_similarity": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _I, _P]),
    "cw_set_alignment_scores": (_I, [_P, _I, _I]),
    "cw_get_alignment_scores": (_I, [_P, _P, _P, _I, _I]),
    "cw_get_transcribe_alignment_scores": (_I, [_P, _P, _P, _I, _I]),
    "cw_test_align_path_scores": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _I, _P, _P]),
    "cw_score_tokens": (_I, [_P, _I, _I, _P, _I, _P, _I, _P, _P, _P]),
    "cw_align_score_tokens": (_I, [_P, _I, _P, _P, _I, _P, _I, _P, _P, _P, _P]),
    "cw_align_cut_tokens": (_I, [_P, _I, _P, _P, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "cw_test_score_head_stop": (_I, [_P, _I, _I, _I, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P]),
    "cw_test_align_cut": (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "cw_score_prefill_runs": (_I, [_P]),
    "cw_set_score_top_logprobs": (_I, [_P, _I]),
    "cw_get_score_top_logprobs": (_I, [_P, _P, _P, _I, _I]),
    "cw_set_score_entropy": (_I, [_P, _I]),
    "cw_get_score_entropy": (_I, [_P, _P, _I, _I]),
    "cw_test_score_head_entropy": (_I, [_P, _I, _I, _I, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    "cw_test_score_rows_entropy": (_I, [_P, _I, _I, _I, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "cw_time_score_head_entropy": (_I, [_P, _I, _I, _I, _I, _P]),
    "cw_test_score_head_top": (_I, [_P, _I, _I, _I, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P]),
    "cw_test_score_head_stop_top": (_I, [_P, _I, _I, _I, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "cw_test_score_rows_top": (_I, [_P, _I, _I, _I, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "cw_time_score_head_top": (_I, [_P, _I, _I, _I, _I, _P]),
    "cw_align_matrix": (_I, [_P, _P, _I, _I, _I, _I, _P, _I, _P]),
    "cw_dtw": (_I, [_P, _P, _I, _I, _P, _P, _P]),
    "cw_adjust_pauses": (_I, [_P, _P, _P, _I, C.c_double]),
    "cw_vocab_create": (_P, [_I, _P, _P, _P, _P, _I, _I, _I, _I, _I]),
    "cw_vocab_destroy": (None, [_P]),
    "cw_collate_begin": (_P, [_P, C.c_double]),
    "cw_beam_host_new": (_P, [_I, _I, _I, _I, _I, _I, _I, C.c_double, _I, _P]),
    "cw_beam_host_step": (_I, [_P, _P, _P, _P, _P]),
    "cw_beam_host_result": (_I, [_P, _P, _P, _P]),
    "cw_beam_host_token_logprobs": (_I, [_P, _P]),
    "cw_beam_host_free": (None, [_P]),
    "cw_collate_set_mode": (_I, [_P, _I]),
    "cw_collate_feed": (_I, [_P, _P, _I, _P, _I, _I, C.c_double, C.c_double, C.c_double]),
    "cw_collate_finish": (_I, [_P, _P, _P, _P, _P]),
    "cw_collate_get": (_I, [_P, _P, _P, _P, _P, _P]),
    "cw_collate_token_groups_total": (C.c_int64, [_P]),
    "cw_collate_get_token_groups": (_I, [_P, _P, _P]),
    "cw_collate_get_languages": (_I, [_P, _P]),
    "cw_collate_free": (None, [_P]),
    "cw_set_option": (_I, [_P, C.c_char_p, _I]),
    "cw_test_set_option": (_I, [C.c_char_p, _I]),
    "cw_test_gemm": (_I, [_P, _I, _I, _I, _P, _P, _P, _I, _P]),
    "cw_test_gemm_fp8": (_I, [_P, _I, _I, _I, _P, _P, _P, _I, _P]),
    "cw_test_gemm_epi": (_I, [_P, C.POINTER(GemmEpiArgs)]),
    "cw_test_rownorm": (_I, [_P, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "cw_test_mel_stages": (_I, [_P, _I, _P, _P, _P]),
    "cw_test_gemv": (_I, [_P, _I, _I, _I, _P, _P, _P, _P, _P, _I, _P]),
    "cw_has_experiments": (_I, []),
    "cw_test_skinny": (_I, [_P, _I, _I, _I, _I, _P, _P, _P, _I, _I, _P, _P]),
    "cw_test_attention": (_I, [_P, _I, _I, _I, _P, _P, _P, _P]),
    "cw_test_cross_attention": (_I, [_P, _I, _I, _I, _I, _P, _P, _P, _I, _P, _P, _P, _P]),
    "cw_test_cross_attention_fused": (_I, [_P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _I, _P, _P, _I, _P, _P, _P, _P]),
    "cw_test_fold": (_I, [_P, C.POINTER(FoldArgs)]),
    "cw_test_gemv_stack": (_I, [_P, C.POINTER(GemvStackArgs)]),
    "cw_test_gemv_epi": (_I, [_P, C.POINTER(GemvEpiArgs)]),
    "cw_test_self_attention": (_I, [_P, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P, _I, _I, _I, _I, _P, _P, _P]),
    "cw_test_beam_state": (_I, [_P, _I, _P, _P, _P]),
    "cw_test_prefill_gemm": (_I, [_P, _I, _I, _I, _I, _P, _P, _P, _P]),
    "cw_test_prefill_attention": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "cw_test_prefill_align_attention": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "cw_test_score_head": (_I, [_P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    "cw_time_score_head": (_I, [_P, _I, _I, _I, _P]),
    "cw_test_beam_topk": (_I, [_P, _I, _P, _P, _I, _I, _I, _I, _P, _P]),
    "cw_test_beam_x": (_I, [_P, _I, _P]),
    "cw_test_decode_state": (_I, [_P, _I, _I, _I, _I, _P]),
    "cw_test_sample": (_I, [_P, _I, _P, _P, _I, _I, _I, _I, _P]),
    "cw_test_sample_seeded": (_I, [_P, _I, _P, _P, _I, _I, _I, _I, C.c_float, C.c_uint64, _P, _P]),
    "cw_test_sample_logprobs": (_I, [_P, _I, _P, _P, _I, _I, _I, _I, C.c_float, C.c_uint64, _P, _P, _P, _P]),
    "cw_test_sample_top_logprobs": (_I, [_P, _I, _P, _P, _I, _I, _I, _I, C.c_float, C.c_uint64, _P, _P, _I, _P, _P, _P, _P]),
    "cw_test_sample_entropy": (_I, [_P, _I, _P, _P, _I, _I, _I, _I, C.c_float, C.c_uint64, _P, _P, _I, _P, _P, _P, _P, _P]),
    "cw_test_sample_biased": (_I, [_P, _I, _P, _P, _I, _I, _I, _I, C.c_float, C.c_uint64, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    "cw_stage_times": (_I, [_P, _P, _P, _I]),
    "cw_time_kernel": (_I, [_P, _I, _I, _I, _P, _P]),
    "cw_time_decode_stage": (_I, [_P, _I, _I, _I, _P, _P, _P, _P]),
    "cw_decode_stage_name": (C.c_char_p, [_I]),
    "cw_handoff_fallbacks": (_I, [_P]),
    "cw_handoff_resumes": (_I, [_P]),
    "cw_decode_stage_launches": (_I, [_P, _I]),
}

_lib = None


def exported_symbols():
    return sorted(_SIGS)


def load():
    """Load the shared library and attach prototypes.  Raises NativeLibraryError if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C crisperwhisper_amd/csrc` (hipcc, gfx950).  There is no CPU fallback.")
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise NativeLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in _SIGS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise NativeLibraryError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
