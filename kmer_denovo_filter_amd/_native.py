"""ctypes binding of include/kdf.h (libkdf.so).

This is the stub a maintainer of the reference would add.
There is no CPU fallback: if the library is missing or no GPU is visible the
calls raise, loudly.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, byref, c_char_p, c_int, c_int32, c_int64, c_uint16, c_uint32, c_uint64, c_void_p

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libkdf.so")

KDF_OK = 0
KDF_ERR_INVALID, KDF_ERR_HIP, KDF_ERR_NOMEM, KDF_ERR_TABLE_FULL, KDF_ERR_IO, KDF_ERR_STATE = 1, 2, 3, 4, 5, 6

# every symbol include/kdf.h declares: (name, restype, argtypes)
_P = c_void_p
SYMBOLS = [
    ("kdf_create", c_int, [c_int, c_int, c_uint64, POINTER(_P)]),
    ("kdf_destroy", None, [_P]),
    ("kdf_last_error", c_char_p, [_P]),
    ("kdf_set_stream", c_int, [_P, _P]),
    ("kdf_synchronize", c_int, [_P]),
    ("kdf_clear", c_int, [_P]),
    ("kdf_reserve", c_int, [_P, c_uint64]),
    ("kdf_stats", c_int, [_P, POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64)]),
    ("kdf_flush", c_int, [_P]),
    ("kdf_set_option", c_int, [_P, c_char_p, c_int64]),
    ("kdf_get_stat", c_int, [_P, c_char_p, POINTER(c_int64)]),
    ("kdf_profile", c_int, [_P, c_int]),
    ("kdf_profile_read", c_int, [_P, POINTER(ctypes.c_double), POINTER(c_uint64), POINTER(c_uint64)]),
    ("kdf_profile_stages", c_int, [_P, POINTER(ctypes.c_double), POINTER(c_uint64)]),
    ("kdf_count_reads", c_int, [_P, _P, _P, c_uint64]),
    ("kdf_count_reads_dev", c_int, [_P, _P, _P, c_uint64]),
    ("kdf_add_pairs", c_int, [_P, _P, _P, _P, c_uint64]),
    ("kdf_host_alloc", c_int, [c_uint64, POINTER(c_void_p)]),
    ("kdf_host_free", c_int, [_P]),
    ("kdf_upload_reads_async", c_int, [_P, c_int, _P, _P, c_uint64]),
    ("kdf_count_uploaded", c_int, [_P, c_int, c_int]),
    ("kdf_add_pairs_dev", c_int, [_P, _P, _P, _P, c_uint64]),
    ("kdf_set_counts_dev", c_int, [_P, c_void_p, c_void_p, c_void_p, c_uint64]),
    ("kdf_add_pairs_multi_dev", c_int, [_P, c_uint32, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p), POINTER(c_uint64)]),
    ("kdf_load_filter", c_int, [_P, _P, _P, c_uint64]),
    ("kdf_load_filter_dev", c_int, [_P, _P, _P, c_uint64]),
    ("kdf_reset_counts", c_int, [_P]),
    ("kdf_count_reads_filtered", c_int, [_P, _P, _P, c_uint64]),
    ("kdf_count_reads_filtered_dev", c_int, [_P, _P, _P, c_uint64]),
    ("kdf_query", c_int, [_P, _P, _P, c_uint64, _P]),
    ("kdf_query_dev", c_int, [_P, _P, _P, c_uint64, _P]),
    ("kdf_count_ge", c_int, [_P, c_uint32, POINTER(c_uint64)]),
    ("kdf_histogram", c_int, [_P, c_uint32, _P]),
    ("kdf_histogram_dev", c_int, [_P, c_uint32, _P]),
    ("kdf_count_stats", c_int, [_P, POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64)]),
    ("kdf_export_ge", c_int, [_P, c_uint32, _P, _P, _P, c_uint64, POINTER(c_uint64)]),
    ("kdf_export_ge_dev", c_int, [_P, c_uint32, _P, _P, _P, c_uint64, c_int, POINTER(c_uint64)]),
    ("kdf_count_join", c_int, [_P, _P, c_uint32, c_uint32, c_uint32, c_uint32, POINTER(c_uint64)]),
    ("kdf_export_join_dev", c_int, [_P, _P, c_uint32, c_uint32, c_uint32, c_uint32, _P, _P, _P, _P, c_uint64, c_int, POINTER(c_uint64)]),
    ("kdf_export_join", c_int, [_P, _P, c_uint32, c_uint32, c_uint32, c_uint32, _P, _P, _P, _P, c_uint64, POINTER(c_uint64)]),
    ("kdf_export_join_w_dev", c_int, [_P, _P, c_uint32, c_uint32, c_uint32, c_uint32, _P, _P, _P, c_uint64, c_int, POINTER(c_uint64)]),
    ("kdf_export_join_w", c_int, [_P, _P, c_uint32, c_uint32, c_uint32, c_uint32, _P, _P, _P, c_uint64, POINTER(c_uint64)]),
    ("kdf_export_parts_dev", c_int, [_P, c_uint32, c_uint32, _P, _P, _P, c_uint64, POINTER(c_uint64), POINTER(c_uint64)]),
    ("kdf_export_parts_packed_dev", c_int, [_P, c_uint32, c_uint32, _P, c_uint64, POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64)]),
    ("kdf_scan_reads", c_int, [_P, _P, _P, c_uint64, _P, c_int64, _P, _P]),
    ("kdf_scan_reads_dev", c_int, [_P, _P, _P, c_uint64, _P]),
    ("kdf_read_hits_dev", c_int, [_P, _P, _P, c_uint64, _P, c_int64, _P, _P]),
    ("kdf_read_hits", c_int, [_P, _P, _P, c_uint64, _P, c_int64, _P, _P]),
    ("kdf_hit_list_dev", c_int, [_P, _P, c_uint64, _P, c_int64, _P, _P, c_uint64, POINTER(c_uint64)]),
    ("kdf_hit_list", c_int, [_P, _P, c_uint64, _P, c_int64, _P, _P, c_uint64, POINTER(c_uint64)]),
    # hits in reference coordinates
    ("kdf_hit_coverage_dev", c_int, [_P, _P, c_uint64, _P, c_int64, _P, _P, c_uint64, _P, _P, _P, c_uint64]),
    ("kdf_hit_coverage", c_int, [_P, _P, c_uint64, _P, c_int64, _P, _P, c_uint64, _P, _P, _P, c_uint64]),
    ("kdf_coverage_list_dev", c_int, [_P, _P, _P, c_uint64, c_uint64, c_uint32, _P, _P, _P, c_uint64, POINTER(c_uint64)]),
    ("kdf_coverage_list", c_int, [_P, _P, _P, c_uint64, c_uint64, c_uint32, _P, _P, _P, c_uint64, POINTER(c_uint64)]),
    ("kdf_hit_keys_dev", c_int, [_P, _P, c_uint64, _P, c_uint64, _P]),
    ("kdf_hit_keys", c_int, [_P, _P, c_uint64, _P, c_uint64, _P]),
    # VCF mode on the device
    ("kdf_variant_windows_dev", c_int, [_P, _P, _P, c_uint64, _P, c_int64, _P, _P, c_uint64, _P, _P, c_uint64, _P, c_uint32, _P, _P, _P, c_uint64,
                                        _P, c_uint64, _P, _P, _P, _P, c_uint64, _P, _P, c_uint64, POINTER(c_uint64), POINTER(c_uint64)]),
    ("kdf_variant_windows", c_int, [_P, _P, _P, c_uint64, _P, c_int64, _P, _P, c_uint64, _P, _P, c_uint64, _P, c_uint32, _P, _P, _P, c_uint64,
                                    _P, c_uint64, _P, _P, _P, _P, c_uint64, _P, _P, c_uint64, POINTER(c_uint64), POINTER(c_uint64)]),
    ("kdf_variant_evidence_dev", c_int, [_P, _P, _P, c_uint64, _P, _P, c_uint64, c_uint64, _P, _P]),
    ("kdf_variant_evidence", c_int, [_P, _P, _P, c_uint64, _P, _P, c_uint64, c_uint64, _P, _P]),
    # regions of informative reads
    ("kdf_cluster_intervals_dev", c_int, [_P, _P, _P, _P, c_int64, c_int64, _P, _P, c_uint64, POINTER(c_uint64)]),
    ("kdf_cluster_intervals", c_int, [_P, _P, _P, _P, c_int64, c_int64, _P, _P, c_uint64, POINTER(c_uint64)]),
    ("kdf_group_distinct_dev", c_int, [_P, _P, _P, c_int, c_uint64, c_int64, _P]),
    ("kdf_group_distinct", c_int, [_P, _P, _P, c_int, c_uint64, c_int64, _P]),
    # k-mer FASTA codec
    ("kdf_kmer_text_bytes", c_uint64, [c_int, c_int, c_uint64, c_uint64]),
    ("kdf_format_kmers_dev", c_int, [_P, _P, _P, c_uint64, c_int, c_int, c_uint64, c_uint64, c_uint64, _P]),
    ("kdf_format_kmers", c_int, [_P, _P, _P, c_uint64, c_int, c_int, c_uint64, c_uint64, c_uint64, _P]),
    ("kdf_parse_kmer_fasta_dev", c_int, [_P, _P, c_uint64, c_int, c_int, c_int, _P, _P, c_uint64, POINTER(c_uint64), POINTER(c_uint64),
                                         POINTER(c_uint64)]),
    ("kdf_parse_kmer_fasta", c_int, [_P, _P, c_uint64, c_int, c_int, c_int, _P, _P, c_uint64, POINTER(c_uint64), POINTER(c_uint64),
                                     POINTER(c_uint64)]),
    # index record codec: one function per operation, `mem` says where the arrays lie
    ("kdf_index_record_bytes", c_uint64, [c_int, c_int]),
    ("kdf_index_encode", c_int, [_P, c_int, _P, _P, _P, _P, c_uint64, c_int, c_uint64, c_uint64, _P]),
    ("kdf_index_decode", c_int, [_P, c_int, _P, c_uint64, c_int, c_int, _P, _P, _P, POINTER(c_uint64)]),
    ("kdf_jf_positions", c_int, [_P, c_int, _P, _P, c_uint64, c_int, POINTER(c_uint64), c_uint64, _P]),
    ("kdf_jf_order", c_int, [_P, c_int, _P, _P, c_uint64, c_int, POINTER(c_uint64), c_uint64, _P]),
    ("kdf_window_counts_dev", c_int, [_P, _P, _P, c_uint64, _P, _P]),
    ("kdf_window_counts", c_int, [_P, _P, _P, c_uint64, _P, _P]),
    ("kdf_read_depth_dev", c_int, [_P, _P, _P, c_uint64, _P, c_int64, c_uint32, _P]),
    ("kdf_read_depth", c_int, [_P, _P, _P, c_uint64, _P, c_int64, c_uint32, _P]),
    ("kdf_stream_words", None, [c_uint64, POINTER(c_uint64), POINTER(c_uint64)]),
    ("kdf_bin_sieve_geometry", c_int, [c_uint64, c_int, c_int, c_int, POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32)]),
    ("kdf_pack_reads", c_int, [_P, _P, c_int64, _P, _P, _P, POINTER(c_uint64)]),
    ("kdf_canonical", c_int, [c_char_p, c_int, POINTER(c_uint64), POINTER(c_uint64)]),
    ("kdf_bam_open", c_int, [c_char_p, c_uint32, c_int, c_int, POINTER(_P)]),
    ("kdf_bam_open_range", c_int, [c_char_p, c_uint32, c_int, c_int, c_int, c_int, POINTER(_P)]),
    ("kdf_fasta_open", c_int, [c_char_p, c_int, POINTER(_P)]),
    ("kdf_reader_next", c_int, [_P, c_uint64, c_int64, _P, _P, _P, POINTER(c_int64), POINTER(c_uint64)]),
    ("kdf_reader_last_meta", c_int, [_P, POINTER(POINTER(c_uint16)), POINTER(POINTER(c_int32)),
                                     POINTER(POINTER(c_int32)), POINTER(c_char_p), POINTER(POINTER(c_int64))]),
    ("kdf_reader_want_aux", c_int, [_P, c_int]),
    ("kdf_reader_last_aux", c_int, [_P, POINTER(POINTER(c_uint32)), POINTER(POINTER(c_int64)),
                                    POINTER(c_char_p), POINTER(POINTER(c_int64))]),
    ("kdf_reader_last_quals", c_int, [_P, POINTER(POINTER(ctypes.c_uint8)), POINTER(POINTER(c_int64)),
                                      POINTER(POINTER(ctypes.c_uint8))]),
    ("kdf_device_memory", c_int, [c_int, POINTER(c_uint64), POINTER(c_uint64)]),
    ("kdf_reader_last_ordinals", c_int, [_P, POINTER(POINTER(c_uint64))]),
    ("kdf_bam_write_subset", c_int, [c_char_p, c_char_p, _P, c_uint64, _P, _P, c_int, c_int, POINTER(c_uint64)]),
    ("kdf_reader_ref_count", c_int, [_P]),
    ("kdf_reader_ref_name", c_char_p, [_P, c_int]),
    ("kdf_reader_ref_length", c_int, [_P, c_int]),
    ("kdf_reader_close", None, [_P]),
    ("kdf_reader_error", c_char_p, [_P]),
    # long keys (odd k 65..201): n x W row-major words
    ("kdf_key_words", c_int, [c_int]),
    ("kdf_canonical_w", c_int, [c_char_p, c_int, POINTER(c_uint64)]),
    ("kdf_add_pairs_w", c_int, [_P, _P, _P, c_uint64]),
    ("kdf_add_pairs_w_dev", c_int, [_P, _P, _P, c_uint64]),
    ("kdf_load_filter_w", c_int, [_P, _P, c_uint64]),
    ("kdf_load_filter_w_dev", c_int, [_P, _P, c_uint64]),
    ("kdf_query_w", c_int, [_P, _P, c_uint64, _P]),
    ("kdf_query_w_dev", c_int, [_P, _P, c_uint64, _P]),
    ("kdf_export_ge_w", c_int, [_P, c_uint32, _P, _P, c_uint64, POINTER(c_uint64)]),
    ("kdf_export_ge_w_dev", c_int, [_P, c_uint32, _P, _P, c_uint64, c_int, POINTER(c_uint64)]),
    # ... across ranks: the dump grouped by owner rank, set_counts
    ("kdf_export_parts_w_packed_dev", c_int, [_P, c_uint32, c_uint32, _P, c_uint64, POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64)]),
    ("kdf_set_counts_w_dev", c_int, [_P, _P, _P, c_uint64]),
    # two-pass counting: the counting sieve
    ("kdf_prefilter_begin", c_int, [_P, c_uint32, c_uint32]),
    ("kdf_prefilter_add_reads", c_int, [_P, _P, _P, c_uint64]),
    ("kdf_prefilter_add_reads_dev", c_int, [_P, _P, _P, c_uint64]),
    ("kdf_prefilter_add_uploaded", c_int, [_P, c_int]),
    ("kdf_prefilter_arm", c_int, [_P]),
    ("kdf_prefilter_drop", c_int, [_P]),
    ("kdf_prefilter_fill", c_int, [_P, POINTER(c_uint64)]),
    ("kdf_prefilter_words", c_int, [_P, POINTER(c_uint64)]),
    ("kdf_prefilter_export_dev", c_int, [_P, c_uint64, c_uint64, _P]),
    ("kdf_prefilter_export", c_int, [_P, c_uint64, c_uint64, _P]),
    ("kdf_prefilter_merge_dev", c_int, [_P, c_uint64, c_uint64, c_uint32, _P, c_int]),
    ("kdf_prefilter_merge", c_int, [_P, c_uint64, c_uint64, c_uint32, _P, c_int]),
    # read spool: a sample's packed stream kept resident and replayed
    ("kdf_spool_create", c_int, [c_int, c_uint64, c_uint64, POINTER(_P)]),
    ("kdf_spool_destroy", None, [_P]),
    ("kdf_spool_error", c_char_p, [_P]),
    ("kdf_spool_set_option", c_int, [_P, c_char_p, c_int64]),
    ("kdf_spool_get_stat", c_int, [_P, c_char_p, POINTER(c_int64)]),
    ("kdf_spool_append", c_int, [_P, _P, _P, c_uint64]),
    ("kdf_spool_append_dev", c_int, [_P, _P, _P, _P, c_uint64]),
    ("kdf_spool_append_uploaded", c_int, [_P, _P, c_int]),
    ("kdf_spool_replay", c_int, [_P, _P, c_int]),
    ("kdf_spool_read_segment", c_int, [_P, c_uint64, _P, _P, POINTER(c_uint64)]),
    ("kdf_spool_clear", c_int, [_P]),
    # ... with read offsets: the per-read consumers over a spool
    ("kdf_spool_append_reads", c_int, [_P, _P, _P, c_uint64, _P, c_int64]),
    ("kdf_spool_append_reads_dev", c_int, [_P, _P, _P, _P, c_uint64, _P, c_int64]),
    ("kdf_spool_append_uploaded_reads", c_int, [_P, _P, c_int, _P, c_int64]),
    ("kdf_spool_read_offsets", c_int, [_P, c_uint64, _P, POINTER(c_uint64), POINTER(c_uint64)]),
    ("kdf_spool_segment_dev", c_int, [_P, c_uint64, POINTER(_P), POINTER(_P), POINTER(c_uint64), POINTER(_P), POINTER(c_uint64),
                                      POINTER(c_uint64)]),
    ("kdf_spool_read_hits", c_int, [_P, _P, _P]),
    ("kdf_spool_read_depth", c_int, [_P, _P, c_uint32, _P]),
    ("kdf_spool_select_reads", c_int, [_P, _P, c_uint32, _P, c_uint64, POINTER(c_uint64)]),
    # distinct k-mer sketch (HyperLogLog registers over the canonical k-mers of read streams)
    ("kdf_sketch_begin", c_int, [_P, c_uint32]),
    ("kdf_sketch_add_reads", c_int, [_P, _P, _P, c_uint64]),
    ("kdf_sketch_add_reads_dev", c_int, [_P, _P, _P, c_uint64]),
    ("kdf_sketch_add_uploaded", c_int, [_P, c_int]),
    ("kdf_sketch_registers", c_int, [_P, _P]),
    ("kdf_sketch_registers_dev", c_int, [_P, _P]),
    ("kdf_sketch_merge", c_int, [_P, _P]),
    ("kdf_sketch_estimate", c_int, [_P, POINTER(ctypes.c_double)]),
    ("kdf_sketch_drop", c_int, [_P]),
    ("kdf_sketch_estimate_registers", c_int, [_P, c_uint32, POINTER(ctypes.c_double)]),
    ("kdf_spool_sketch", c_int, [_P, _P]),
    # device BAM feeder: the raw range planner (host) and the batch decoder (device)
    ("kdf_bamraw_open", c_int, [c_char_p, c_uint32, c_int, c_int, c_int, c_uint64, POINTER(_P)]),
    ("kdf_bamraw_subranges", c_int, [_P, POINTER(c_uint64)]),
    ("kdf_bamraw_next", c_int, [_P, _P, c_uint64, c_uint32, _P, c_uint64, _P, c_uint64, POINTER(c_uint64), POINTER(c_uint64),
                                POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64)]),
    ("kdf_bamraw_seek", c_int, [_P, c_uint64]),
    ("kdf_bamraw_close", None, [_P]),
    ("kdf_bamraw_error", c_char_p, [_P]),
    ("kdf_bgzf_inflate_dev", c_int, [_P, _P, _P, c_uint64, _P, c_uint64, _P]),
    ("kdf_bamdev_decode_dev", c_int, [_P, _P, _P, c_uint64, _P, c_uint64, c_uint32, c_int, _P, _P, c_uint64, _P, c_uint64,
                                      POINTER(c_uint64), POINTER(c_uint64), _P]),
    # device FASTA feeder (the state: FastaState below)
    ("kdf_fasta_pack_dev", c_int, [_P, _P, c_uint64, c_int, _P, _P, _P, c_uint64, c_uint32, _P, _P, c_uint64, _P, c_uint64,
                                   POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64)]),
    ("kdf_fasta_pack", c_int, [_P, _P, c_uint64, c_int, _P, _P, _P, c_uint64, c_uint32, _P, _P, c_uint64, _P, c_uint64,
                               POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64)]),
    # device FASTQ feeder (the state: FastqState below): one function with a `mem` argument
    ("kdf_fastq_pack", c_int, [_P, c_int, _P, c_uint64, c_int, c_uint32, _P, _P, _P, c_uint64, _P, c_uint64,
                               POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint32)]),
    # FASTQ record extract: the kept records of a chunk back out as text, one function with a `mem` argument
    ("kdf_fq_extract", c_int, [_P, c_int, _P, c_uint64, c_int, _P, c_uint64, _P, c_uint64, _P,
                                  POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint32)]),
]

KDF_MEM_HOST, KDF_MEM_DEVICE = 0, 1          # the `mem` argument of the index record codec, the FASTQ feeder and the FASTQ record extract
KDF_FA_IN_RECORD, KDF_FA_MID_LINE, KDF_FA_IN_HEADER = 1, 2, 4
KDF_FASTA_TILE_BYTES = 4096


class FastaState(ctypes.Structure):
    """kdf_fasta_state: what the device FASTA feeder carries from chunk to chunk (all zero before the first)."""
    _fields_ = [("flags", c_uint32), ("reserved", c_uint32), ("records", c_uint64), ("positions", c_uint64)]

    def copy(self) -> "FastaState":
        return FastaState(self.flags, self.reserved, self.records, self.positions)


KDF_FQ_BAD_HEADER, KDF_FQ_BAD_PLUS, KDF_FQ_LENGTH, KDF_FQ_TRUNCATED = 1, 2, 3, 4
KDF_FASTQ_TILE_BYTES = 4096


class FastqState(ctypes.Structure):
    """kdf_fastq_state: the running totals the device FASTQ feeder keeps from chunk to chunk (all zero before the first)."""
    _fields_ = [("records", c_uint64), ("positions", c_uint64), ("bytes", c_uint64)]

    def copy(self) -> "FastqState":
        return FastqState(self.records, self.positions, self.bytes)


_lib = None


class KdfError(RuntimeError):
    """Engine failure; mirrors the reference's RuntimeError("jellyfish ... failed: ...")."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"kdf engine failed ({code}): {msg}")
        self.code = code


class FastqFormatError(KdfError):
    """A text that is no four-line FASTQ (KDF_ERR_IO of kdf_fastq_pack).  ``offset``: the first byte of the first bad record
    -- within the call's text, or within the file when ``reads.stream_fastq_device`` raises it; ``rule``: KDF_FQ_*."""

    def __init__(self, code: int, msg: str, offset: int, rule: int):
        super().__init__(code, msg)
        self.offset, self.rule = int(offset), int(rule)


def _preload_torch_hip():
    """PyTorch-ROCm wheels bundle their own libamdhip64/libhsa-runtime64.  If
    libkdf.so pulled /opt/rocm's copies first, a later `import torch` would load
    a SECOND HSA runtime into the process and find no device.  Loading torch's
    copies first (same SONAMEs) makes both sides share one runtime, in either
    import order.  torch itself is not imported and the GPU is not touched."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if not spec or not spec.submodule_search_locations:
        return
    libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        path = os.path.join(libdir, name)
        if os.path.exists(path):
            try:
                ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
            except OSError:
                return


def load() -> ctypes.CDLL:
    """Load libkdf.so, building it first if the source tree has hipcc and no .so."""
    global _lib
    if _lib is not None:
        return _lib
    _preload_torch_hip()
    if not os.path.exists(LIB_PATH):
        from .build import build_native
        try:
            build_native()
        except Exception as e:  # noqa: BLE001
            raise ImportError(
                f"libkdf.so is not built ({LIB_PATH}) and building it failed: {e}. "
                "Run `python -m kmer_denovo_filter_amd.build`. There is no CPU fallback."
            ) from e
    lib = ctypes.CDLL(LIB_PATH)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)          # AttributeError if the ABI is incomplete
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, handle=None):
    if rc != KDF_OK:
        lib = load()
        msg = lib.kdf_last_error(handle)
        raise KdfError(rc, msg.decode(errors="replace") if msg else "unknown error")


def check_spool(rc: int, spool=None):
    if rc != KDF_OK:
        lib = load()
        msg = lib.kdf_spool_error(spool)
        raise KdfError(rc, msg.decode(errors="replace") if msg else "unknown error")


def check_bamraw(rc: int, reader=None):
    if rc != KDF_OK:
        lib = load()
        msg = lib.kdf_bamraw_error(reader)
        raise KdfError(rc, msg.decode(errors="replace") if msg else "unknown error")


def check_reader(rc: int, reader=None):
    if rc != KDF_OK:
        lib = load()
        msg = lib.kdf_reader_error(reader)
        raise KdfError(rc, msg.decode(errors="replace") if msg else "unknown error")
