"""ctypes binding of include/fqgpu.h (one Python name per C entry point)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# FQGPU_LIB: another build of the same ABI (tools/traffic_experiment.py loads the -DFQGPU_EXPERIMENTS one)
LIB_PATH = os.environ.get("FQGPU_LIB") or os.path.join(HERE, "libfqgpu.so")

SEQ_MODELS, SEQ_ALPHA = 256, 4
QUAL_MODELS, QUAL_ALPHA = 8192, 64
REC_DTYPE = np.dtype([("seq_off", "<u4"), ("qual_off", "<u4"), ("len", "<u4")])
SEQ_FT_DTYPE = np.dtype(
    [("norm", "<i2", (SEQ_MODELS, SEQ_ALPHA)), ("logs", "<u4", (SEQ_MODELS,)), ("max_log", "<u4")]
)
QUAL_FT_DTYPE = np.dtype(
    [("norm", "<i2", (QUAL_MODELS, QUAL_ALPHA)), ("logs", "<u4", (QUAL_MODELS,)), ("max_log", "<u4")]
)
F_WRITE_BACK_N = 1
F_DECODE_INDEX = 2  # extension: the encode also leaves a decode index per stream
# FQGPU_DEC_FORM_*: the kernel forms of a decode launch (Context.decode_forms)
DEC_FORM_BOTH, DEC_FORM_QUAL_RESIDENT, DEC_FORM_QUAL_COMPACT, DEC_FORM_SEQ = 0x001, 0x002, 0x004, 0x008
DEC_FORM_CHUNKS_QUAL_RESIDENT, DEC_FORM_CHUNKS_QUAL_COMPACT, DEC_FORM_CHUNKS_SEQ, DEC_FORM_SNAP = 0x010, 0x020, 0x040, 0x100

ERRORS = {0: "OK", -1: "OVERFLOW", -2: "SHORT_READ", -3: "CORRUPT", -4: "ARG", -5: "NO_DEVICE",
          -6: "NOMEM", -7: "HIP"}


class FqgpuError(RuntimeError):
    def __init__(self, code, where=""):
        self.code = code
        msg = lib().fqgpu_strerror(code).decode() if _lib is not None else ""
        super().__init__("fqgpu %s: %s (%d) %s" % (where, ERRORS.get(code, "?"), code, msg))


class Timing(C.Structure):
    _fields_ = [("total_ms", C.c_float), ("kernel_ms", C.c_float * 32), ("kernel_calls", C.c_int * 32),
                ("kernel_name", C.c_char_p * 32), ("n_kernels", C.c_int)]


def lib_path():
    return LIB_PATH


def build(verbose=False):
    """Compile every HIP translation unit for gfx950 and link libfqgpu.so in-tree."""
    cmd = ["make", "-C", os.path.join(HERE, "csrc"), "-j", "6"]
    subprocess.run(cmd, check=True, stdout=None if verbose else subprocess.DEVNULL)
    return LIB_PATH


_lib = None

_PROTOS = {
    # name: (restype, argtypes)
    "fqgpu_device_count": (C.c_int, []),
    "fqgpu_strerror": (C.c_char_p, [C.c_int]),
    "fqgpu_version": (C.c_char_p, []),
    "fqgpu_bound_seq": (C.c_size_t, [C.c_size_t]),
    "fqgpu_bound_qual": (C.c_size_t, [C.c_size_t]),
    "fqgpu_freq_tables": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fqgpu_tables_from_counts": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fqgpu_ctx_create": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "fqgpu_ctx_destroy": (None, [C.c_void_p]),
    "fqgpu_ctx_set_chain_params": (C.c_int, [C.c_void_p, C.c_uint, C.c_uint]),
    "fqgpu_ctx_dump_tables": (C.c_int, [C.c_void_p, C.c_int, C.c_uint, C.c_void_p, C.c_size_t,
                                        C.c_void_p, C.c_size_t]),
    "fqgpu_encode_block": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                     C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                     C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                     C.POINTER(C.c_size_t), C.c_uint]),
    "fqgpu_encode_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint,
                                     C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "fqgpu_encode_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "fqgpu_encode_wait": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "fqgpu_encode_cancel": (C.c_int, [C.c_void_p]),
    "fqgpu_encode_headers_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint, C.c_void_p, C.c_size_t]),
    "fqgpu_encode_headers_wait": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "fqgpu_encode_headers_end": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "fqgpu_encode_end": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                   C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_size_t, C.POINTER(C.c_size_t)]),
    "fqgpu_decode_block": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                     C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                     C.c_size_t, C.c_void_p, C.c_size_t]),
    "fqgpu_encode_index": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "fqgpu_decode_block_indexed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                             C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                             C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "fqgpu_decode_chunk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                     C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                     C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                     C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "fqgpu_decode_chunk_indexing": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                              C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                              C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "fqgpu_decode_index": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "fqgpu_decode_chunk_range": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                           C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                           C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                                           C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p,
                                           C.POINTER(C.c_size_t)]),
    "fqgpu_decode_chunk_fasta": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                           C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                           C.c_size_t, C.c_size_t, C.c_size_t,
                                           C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p,
                                           C.POINTER(C.c_size_t)]),
    "fqgpu_dblock_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                      C.POINTER(C.c_void_p)]),
    "fqgpu_dblock_create_from_raw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "fqgpu_dblock_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                       C.POINTER(C.c_size_t)]),
    "fqgpu_dblock_destroy": (None, [C.c_void_p]),
    "fqgpu_dblock_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint]),
    "fqgpu_dblock_wipe": (C.c_int, [C.c_void_p, C.c_void_p]),
    "fqgpu_dblocks_decode": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t]),
    "fqgpu_dblocks_decode_indexing": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t]),
    "fqgpu_sync": (C.c_int, [C.c_void_p]),
    "fqgpu_dblock_status": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                      C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "fqgpu_dblock_longest_chain": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]),
    "fqgpu_dblock_qual_segment_classes": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]),
    "fqgpu_dblock_qual_segments": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                             C.POINTER(C.c_size_t)]),
    "fqgpu_ctx_set_index_stride": (C.c_int, [C.c_void_p, C.c_uint]),
    "fqgpu_dblock_index_bytes": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_size_t)]),
    "fqgpu_dblock_fetch_index": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "fqgpu_dblock_load_index": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "fqgpu_ctx_set_lanes": (C.c_int, [C.c_void_p, C.c_uint]),
    "fqgpu_ctx_fill_scratch": (C.c_int, [C.c_void_p, C.c_ubyte, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "fqgpu_ctx_reserve": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t]),
    "fqgpu_ctx_set_seq_segment": (C.c_int, [C.c_void_p, C.c_uint]),
    "fqgpu_ctx_set_seq_group": (C.c_int, [C.c_void_p, C.c_uint, C.c_uint]),
    "fqgpu_ctx_decode_forms": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_uint)] * 4),
    "fqgpu_ctx_set_seq_handover": (C.c_int, [C.c_void_p, C.c_uint, C.c_uint]),
    "fqgpu_dblock_seq_handover": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]),
    "fqgpu_dblock_fetch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "fqgpu_dblock_load_streams": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                            C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t]),
    "fqgpu_ctx_enable_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "fqgpu_ctx_last_timing": (C.c_int, [C.c_void_p, C.POINTER(Timing)]),
    "fqgpu_ctx_timing_only": (C.c_int, [C.c_void_p, C.c_char_p]),
    "fqgpu_chunk_crc32": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_size_t)]),
    "fqgpu_dblock_crc32": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_size_t)]),
    "fqgpu_crc32_combine": (C.c_uint32, [C.c_uint32, C.c_uint32, C.c_uint64]),
    "fqgpu_ctx_set_check_only": (C.c_int, [C.c_void_p, C.c_int]),
    "fqgpu_stats_words": (C.c_size_t, [C.c_uint]),
    "fqgpu_chunk_stats": (C.c_int, [C.c_void_p, C.c_uint, C.c_void_p, C.c_size_t]),
    "fqgpu_dblock_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p, C.c_size_t]),
    "fqgpu_stats_merge": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "fqgpu_filter_check": (C.c_int, [C.c_void_p]),
    "fqgpu_chunk_filter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p, C.c_void_p]),
    "fqgpu_dblock_filter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                      C.c_void_p, C.c_void_p]),
    "fqgpu_trim_check": (C.c_int, [C.c_void_p]),
    "fqgpu_chunk_trim": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "fqgpu_dblock_trim": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "fqgpu_adapter_check": (C.c_int, [C.c_void_p]),
    "fqgpu_chunk_clip": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "fqgpu_dblock_clip": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                    C.POINTER(C.c_size_t), C.c_void_p, C.c_void_p, C.c_void_p]),
    "fqgpu_tail_check": (C.c_int, [C.c_void_p]),
    "fqgpu_chunk_tailtrim": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                       C.POINTER(C.c_size_t), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fqgpu_dblock_tailtrim": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.POINTER(C.c_size_t), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fqgpu_chunk_select_marked": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p,
                                            C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fqgpu_dblock_select_marked": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t,
                                             C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    "fqgpu_chunk_select_limited": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fqgpu_dblock_select_limited": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
    "fqgpu_overlap_check": (C.c_int, [C.c_void_p]),
    "fqgpu_overlap_merge": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "fqgpu_chunk_pair_overlap": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "fqgpu_dblock_pair_overlap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p,
                                            C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fqgpu_correct_check": (C.c_int, [C.c_void_p]),
    "fqgpu_chunk_pair_correct": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
    "fqgpu_dblock_pair_correct": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "fqgpu_merge_check": (C.c_int, [C.c_void_p]),
    "fqgpu_chunk_pair_merge": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fqgpu_dblock_pair_merge": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fqgpu_chunk_pair_names": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t)]),
    "fqgpu_dblock_pair_names": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t)]),
    "fqgpu_read_id_len": (C.c_size_t, [C.c_void_p, C.c_size_t]),
    "fqgpu_probe_words": (C.c_size_t, [C.c_uint, C.c_uint]),
    "fqgpu_probes_check": (C.c_int, [C.c_void_p]),
    "fqgpu_chunk_probe": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p, C.c_size_t, C.c_void_p]),
    "fqgpu_dblock_probe": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p, C.c_size_t, C.c_void_p]),
    "fqgpu_probe_merge": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "fqgpu_host_alloc": (C.c_void_p, [C.c_size_t]),
    "fqgpu_host_free": (None, [C.c_void_p]),
    "fqgpu_host_trim": (C.c_size_t, []),
    "fqgpu_memcompress_bound": (C.c_size_t, [C.c_size_t]),
    "fqgpu_memcompress": (C.c_size_t, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "fqgpu_memdecompress": (C.c_size_t, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "fqgpu_parse_fastq": (C.c_long, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "fqgpu_synth_fastq": (C.c_size_t, [C.c_void_p, C.c_size_t, C.c_int, C.c_uint64, C.c_uint64,
                                       C.POINTER(C.c_uint64)]),
}
EXPORTS = sorted(_PROTOS)


def lib():
    """The loaded extension.  Raises if libfqgpu.so has not been built: no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libfqgpu.so is not built (run __graft_entry__.build() or "
                               "`make -C fqcomp28_amd/csrc`); the product path has no CPU fallback")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _PROTOS.items():
            fn = getattr(L, name)  # AttributeError = a symbol the header declares is missing
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _check(rc, where):
    if rc != 0:
        raise FqgpuError(rc, where)


def _bad(bad_record):
    """*bad_record of a C call: None when it names no record"""
    return None if bad_record.value == (1 << 64) - 1 else bad_record.value


def _chunk_args(header_format, header_fields, readlens, seq, qual, n_count, n_pos, index):
    """The arguments fqgpu_decode_chunk and fqgpu_decode_chunk_range share, from hdr to qual_index_len, and the
    objects they point into (to be kept until the call has returned)."""
    types, seps, first = header_format
    types = np.ascontiguousarray(types, dtype=np.uint8)
    first = np.frombuffer(bytes(first), dtype=np.uint8)
    parts = [np.ascontiguousarray(np.frombuffer(bytes(x), dtype=np.uint8)) for f in header_fields for x in f]
    sizes = np.array([[len(x) for x in f] for f in header_fields], dtype=np.uint32).reshape(-1, 3)
    ptrs = (C.c_void_p * max(len(parts), 1))(*[x.ctypes.data if x.size else None for x in parts])
    hs = _HeaderStreams(types.ctypes.data, bytes(seps), len(types), first.ctypes.data, first.size,
                        sizes.ctypes.data, C.cast(ptrs, C.POINTER(C.c_void_p)))
    readlens = np.ascontiguousarray(readlens, dtype=np.uint16)
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    qual = np.ascontiguousarray(qual, dtype=np.uint8)
    n_count = np.ascontiguousarray(n_count, dtype=np.uint16)
    n_pos = np.ascontiguousarray(n_pos, dtype=np.uint16)
    si, qi = (np.ascontiguousarray(x, dtype=np.uint8) for x in index) if index is not None else (np.zeros(0, np.uint8),) * 2
    args = (C.byref(hs), _p(readlens), len(readlens), _p(seq), seq.size, _p(qual), qual.size, _p(n_count), n_count.size,
            _p(n_pos) if n_pos.size else None, n_pos.size, _p(si) if si.size else None, si.size,
            _p(qi) if qi.size else None, qi.size)
    return args, (types, first, parts, sizes, ptrs, hs, readlens, seq, qual, n_count, n_pos, si, qi)


def device_count():
    return lib().fqgpu_device_count()


def bound_seq(n):
    return lib().fqgpu_bound_seq(n)


def bound_qual(n):
    return lib().fqgpu_bound_qual(n)


def parse_fastq(raw):
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    n = lib().fqgpu_parse_fastq(_p(raw), raw.size, None, 0)
    if n < 0:
        raise FqgpuError(-4, "parse_fastq")
    recs = np.zeros(n, dtype=REC_DTYPE)
    lib().fqgpu_parse_fastq(_p(raw), raw.size, _p(recs), n)
    return recs


def memcompress(data):
    """misc-stream compressor (host code; own format, see fq_misc.cpp) -> uint8 array"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    out = np.empty(lib().fqgpu_memcompress_bound(data.size), dtype=np.uint8)
    n = lib().fqgpu_memcompress(_p(out), out.size, _p(data), data.size)
    return out[:n].copy()


def memdecompress(cdata, original_size):
    cdata = np.ascontiguousarray(cdata, dtype=np.uint8)
    out = np.empty(original_size, dtype=np.uint8)
    n = lib().fqgpu_memdecompress(_p(out), out.size, _p(cdata), cdata.size)
    if n == 2 ** 64 - 1 or (cdata.size and n != original_size):
        raise FqgpuError(-3, "memdecompress")
    return out[:0] if cdata.size == 0 else out


def crc32_combine(crc_a, crc_b, len_b):
    """fqgpu_crc32_combine: the zlib CRC-32 of A || B from the digests of A and B and the length of B"""
    return lib().fqgpu_crc32_combine(crc_a, crc_b, len_b)


def stats_words(positions):
    """fqgpu_stats_words: uint64 words of a read summary with `positions` rows (0: positions out of range)"""
    return lib().fqgpu_stats_words(positions)


def stats_merge(dst, src):
    """fqgpu_stats_merge: dst += src in place (two uint64 arrays) -> rc"""
    assert dst.dtype == np.uint64 and src.dtype == np.uint64 and dst.flags.c_contiguous and src.flags.c_contiguous
    return lib().fqgpu_stats_merge(_p(dst), dst.size, _p(src), src.size)


STATS_HEAD_WORDS, STATS_MEANQ_AT, STATS_GC_AT = 176, 8, 72


def stats_view(words):
    """The parts of a read summary (include/fqgpu.h) as numpy views of `words`, a uint64 array of stats_words(P)."""
    assert words.dtype == np.uint64 and words.ndim == 1
    rows = int(words[5]) + 1
    assert words.size == STATS_HEAD_WORDS + 70 * rows, "not a summary of the positions it names"
    at = STATS_HEAD_WORDS
    view = dict(n_records=words[0:1], n_bases=words[1:2], min_len=words[2:3], max_len=words[3:4], reads_with_n=words[4:5],
                positions=words[5:6], meanq_hist=words[STATS_MEANQ_AT:STATS_MEANQ_AT + 64],
                gc_hist=words[STATS_GC_AT:STATS_GC_AT + 101], len_hist=words[at:at + rows])
    view["base_pos"] = words[at + rows:at + 6 * rows].reshape(rows, 5)
    view["qual_pos"] = words[at + 6 * rows:at + 70 * rows].reshape(rows, 64)
    return view


def _stats_call(fn, positions, *front):
    """-> (rc, words): a device summary call on a fresh uint64 array of the size `positions` asks for"""
    out = np.zeros(max(stats_words(positions), 1), dtype=np.uint64)
    rc = fn(*front, positions, _p(out), out.size)
    return rc, out


FILTER_NONE = 0xFFFFFFFF
FILTER_REPORT_WORDS = 16
FILTER_REPORT_NAMES = ("n_records", "n_kept", "bases_in", "bases_kept", "bytes_kept", "dropped_short", "dropped_long", "dropped_n",
                       "dropped_mean_q", "dropped_low_q")


def read_filter(min_len=0, max_len=FILTER_NONE, max_n=FILTER_NONE, min_mean_q=0, low_q=0, max_low_pct=0, reserved=(0, 0)):
    """an fqgpu_filter (include/fqgpu.h) as a uint32 array of eight words; the defaults keep every read"""
    return np.array([min_len, max_len, max_n, min_mean_q, low_q, max_low_pct, reserved[0], reserved[1]], dtype=np.uint32)


def filter_check(flt):
    """fqgpu_filter_check -> rc (host only)"""
    return lib().fqgpu_filter_check(_p(flt))


def _select_call(fn, front, specs, n_recs, extra=(), more=(), want_win=True, want_places=True, out_cap=None, want_keep=True, query=False,
                 report_words=FILTER_REPORT_WORDS):
    """A device selection call (filter, trim, clip, tailtrim, select_marked, select_limited) -> dict(rc, out, out_len, report,
    keep) plus the arrays named in `more`.  specs: the call's adapter, tail, trim and filter words in the order of its arguments
    (None: NULL); extra: the C arguments it takes between the specs and `out` (a range's first, end, mark, limits); more: the
    outputs it takes behind keep_out, of "win" -- the records' windows, uint32[n_recs], start | n << 16 -- and "places" --
    uint16[n_recs, 4], a0, a1, e, e2 of every record --, each allocated unless want_win / want_places is false (then NULL, and
    None in the dict).  out_cap None: the size is asked for first (out=NULL), then the call is made with a buffer of that size --
    query: the size is asked for and that is all; a number: ONE call with a buffer of that many bytes.  report_words: the words
    of the call's report."""
    report = np.zeros(report_words, dtype=np.uint64)
    keep = np.zeros((n_recs + 7) // 8, dtype=np.uint8) if want_keep else None
    arrays = dict(win=np.zeros(n_recs, dtype=np.uint32) if want_win else None, places=np.zeros((n_recs, 4), dtype=np.uint16) if want_places else None)
    arrays = {name: arrays[name] for name in more}
    n = C.c_size_t(0)
    words = [None if s is None else np.ascontiguousarray(s, dtype=np.uint32) for s in specs]
    head = (*front, *[_p(w) for w in words], *extra)
    tail = (C.byref(n), _p(report), _p(keep), *[_p(a) for a in arrays.values()])
    if out_cap is None:
        rc = fn(*head, None, 0, *tail)
        if rc != 0 or query:
            return dict(rc=rc, out=None, out_len=n.value, report=report, keep=keep, **arrays)
        out_cap = n.value
    out = np.zeros(max(out_cap, 1), dtype=np.uint8)
    rc = fn(*head, _p(out), out_cap, *tail)
    return dict(rc=rc, out=out[:n.value] if rc == 0 else out, out_len=n.value, report=report, keep=keep, **arrays)


TRIM_REPORT_WORDS = 16
TRIM_REPORT_NAMES = FILTER_REPORT_NAMES + ("reads_trimmed", "bases_cut_front", "bases_cut_tail", "reads_emptied")


def read_trim(cut_front=0, cut_tail=0, q_front=0, q_tail=0, crop=FILTER_NONE, reserved=(0, 0, 0)):
    """an fqgpu_trim (include/fqgpu.h) as a uint32 array of eight words; the defaults cut nothing"""
    return np.array([cut_front, cut_tail, q_front, q_tail, crop, reserved[0], reserved[1], reserved[2]], dtype=np.uint32)


def trim_check(trim):
    """fqgpu_trim_check -> rc (host only)"""
    return lib().fqgpu_trim_check(_p(trim))


ADAPTER_MAX = 64
CLIP_REPORT_NAMES = TRIM_REPORT_NAMES + ("reads_with_adapter", "bases_cut_adapter")


def read_adapter(seq, min_overlap=5, max_err_pct=10, reserved=0, length=None):
    """an fqgpu_adapter (include/fqgpu.h) as a uint32 array of twenty words: the sixty-four bytes of seq, zero behind it, then
    len, min_overlap, max_err_pct, reserved.  seq: str or bytes, at most ADAPTER_MAX of it is stored; length: what len says
    when it is not len(seq) (for the checks' tests)"""
    seq = seq.encode() if isinstance(seq, str) else bytes(seq)
    a = np.zeros(ADAPTER_MAX // 4 + 4, dtype=np.uint32)
    a[:ADAPTER_MAX // 4].view(np.uint8)[:min(len(seq), ADAPTER_MAX)] = np.frombuffer(seq[:ADAPTER_MAX], dtype=np.uint8)
    a[ADAPTER_MAX // 4:] = (len(seq) if length is None else length, min_overlap, max_err_pct, reserved)
    return a


def adapter_check(adapter):
    """fqgpu_adapter_check -> rc (host only)"""
    return lib().fqgpu_adapter_check(_p(adapter))


TAIL_REPORT_WORDS = 24
TAIL_REPORT_NAMES = CLIP_REPORT_NAMES + ("reads_with_poly_tail", "bases_cut_poly", "reads_window_cut", "bases_cut_window")
POLY_BASES = {"A": 1, "C": 2, "G": 4, "T": 8}


def read_tail(poly="", poly_min_len=None, poly_every=None, poly_max_mism=None, window_len=0, window_q=0, reserved=(0, 0)):
    """an fqgpu_tail (include/fqgpu.h) as a uint32 array of eight words.  poly: the bases of the set as a string of ACGT, or
    the bit mask itself; with a set, the defaults are a shortest tail of 10, one mismatch per 8 bases and at most 5 (the
    tool's); without, zero.  The defaults cut nothing."""
    bases = sum(POLY_BASES[c] for c in set(poly)) if isinstance(poly, str) else int(poly)
    on = bases != 0
    pick = lambda v, d: (d if on else 0) if v is None else v  # noqa: E731
    return np.array([bases, pick(poly_min_len, 10), pick(poly_every, 8), pick(poly_max_mism, 5), window_len, window_q, reserved[0], reserved[1]],
                    dtype=np.uint32)


def tail_check(tail):
    """fqgpu_tail_check -> rc (host only)"""
    return lib().fqgpu_tail_check(_p(tail))


MARKED_REPORT_NAMES = TAIL_REPORT_NAMES + ("dropped_unmarked",)
DROPPED_UNMARKED = 20
NO_MISMATCH = (1 << 64) - 1
LIMITED_REPORT_NAMES = MARKED_REPORT_NAMES + ("reads_cut_limit", "bases_cut_limit")
READS_CUT_LIMIT, BASES_CUT_LIMIT = 21, 22


def _range_call(fn, front, specs, first, end, mark, *limit, **kw):
    """A device marked or limited call over the records [first, end) -> _select_call's dict with win and places, everything
    relative to `first`.  mark: None (NULL), or uint8 of (end - first + 7) // 8 bytes in the keep bits' layout; limit: the
    limited calls' one more argument -- None (NULL), or uint16 of end - first limits"""
    mark = None if mark is None else np.ascontiguousarray(mark, dtype=np.uint8)
    limit = [None if v is None else np.ascontiguousarray(v, dtype=np.uint16) for v in limit]
    return _select_call(fn, front, specs, max(end - first, 0), extra=(first, end, _p(mark), *[_p(v) for v in limit]), more=("win", "places"),
                        report_words=TAIL_REPORT_WORDS, **kw)


OVERLAP_MAX_LEN, OVERLAP_ROWS, OVERLAP_HEAD_WORDS = 512, 1024, 16
OVERLAP_WORDS = OVERLAP_HEAD_WORDS + OVERLAP_ROWS
OVERLAP_NAMES = ("n_pairs", "pairs_overlapped", "pairs_read_through", "bases_behind_a", "bases_behind_b", "pairs_not_analysed", "mismatches",
                 "overlap_bases", "fingerprint")


def read_overlap(min_overlap=30, max_mism=5, max_err_pct=20, reserved=(0, 0, 0, 0, 0)):
    """an fqgpu_overlap (include/fqgpu.h) as a uint32 array of eight words; the defaults are the tool's"""
    return np.array([min_overlap, max_mism, max_err_pct, *reserved], dtype=np.uint32)


def overlap_check(spec):
    """fqgpu_overlap_check -> rc (host only)"""
    return lib().fqgpu_overlap_check(_p(None if spec is None else np.ascontiguousarray(spec, dtype=np.uint32)))


def overlap_merge(dst, src):
    """fqgpu_overlap_merge: dst += src in place (two uint64 arrays) -> rc"""
    assert dst.dtype == np.uint64 and src.dtype == np.uint64 and dst.flags.c_contiguous and src.flags.c_contiguous
    return lib().fqgpu_overlap_merge(_p(dst), dst.size, _p(src), src.size)


def _overlap_call(fn, front, count, spec, want_arrays=True, cap_words=None):
    """A device overlap call -> dict(rc, out, limit_a, limit_b, insert): out a fresh uint64 array of OVERLAP_WORDS (cap_words: of
    that many words instead), the three arrays uint16[count] or None"""
    spec = None if spec is None else np.ascontiguousarray(spec, dtype=np.uint32)
    cap = OVERLAP_WORDS if cap_words is None else cap_words
    out = np.zeros(max(cap, 1), dtype=np.uint64)
    arrays = [np.zeros(max(count, 1), dtype=np.uint16) if want_arrays else None for _ in range(3)]
    rc = fn(*front, count, _p(spec), _p(out), cap, *[_p(a) for a in arrays])
    la, lb, ins = [None if a is None else a[:count] for a in arrays]
    return dict(rc=rc, out=out, limit_a=la, limit_b=lb, insert=ins)


CORRECT_REPORT_WORDS = 8
CORRECT_REPORT_NAMES = ("n_pairs", "pairs_with_insert", "pairs_corrected", "bases_corrected_a", "bases_corrected_b", "n_resolved",
                        "mismatches_seen", "overlap_bases")


def read_correct(good_q=30, bad_q=14, reserved=(0, 0, 0, 0, 0, 0)):
    """an fqgpu_correct (include/fqgpu.h) as a uint32 array of eight words; the defaults are the tool's"""
    return np.array([good_q, bad_q, *reserved], dtype=np.uint32)


def correct_check(spec):
    """fqgpu_correct_check -> rc (host only)"""
    return lib().fqgpu_correct_check(_p(None if spec is None else np.ascontiguousarray(spec, dtype=np.uint32)))


def _correct_call(fn, front, count, insert, spec, want_arrays=True, want_report=True):
    """A device correcting call -> dict(rc, report, fixed_a, fixed_b): report a fresh uint64 array of CORRECT_REPORT_WORDS, the
    two arrays uint16[count] or None; insert: None (NULL), or uint16 -- fewer than count (a count the call is to refuse) are
    padded with zeros, so that the library never reads behind them.  THE CALL CHANGES BOTH CHUNKS"""
    spec = None if spec is None else np.ascontiguousarray(spec, dtype=np.uint32)
    insert = None if insert is None else np.ascontiguousarray(insert, dtype=np.uint16)
    if insert is not None and insert.size < count:
        insert = np.concatenate((insert, np.zeros(count - insert.size, dtype=np.uint16)))
    report = np.zeros(CORRECT_REPORT_WORDS, dtype=np.uint64)
    arrays = [np.zeros(max(count, 1), dtype=np.uint16) if want_arrays else None for _ in range(2)]
    rc = fn(*front, count, _p(insert), _p(spec), _p(report) if want_report else None, *[_p(a) for a in arrays])
    fa, fb = [None if a is None else a[:count] for a in arrays]
    return dict(rc=rc, report=report, fixed_a=fa, fixed_b=fb)


MERGE_REPORT_WORDS = 16
MERGE_REPORT_NAMES = ("n_pairs", "pairs_with_insert", "pairs_merged", "bases_merged", "bytes_out", "overlap_bases", "places_disagree",
                      "places_n", "bases_dropped_a", "bases_dropped_b", "pairs_unmarked", "pairs_too_short")


def read_merge(floor_q=2, min_len=1, reserved=(0, 0, 0, 0, 0, 0)):
    """an fqgpu_merge (include/fqgpu.h) as a uint32 array of eight words; the defaults are the tool's"""
    return np.array([floor_q, min_len, *reserved], dtype=np.uint32)


def merge_check(spec):
    """fqgpu_merge_check -> rc (host only)"""
    return lib().fqgpu_merge_check(_p(None if spec is None else np.ascontiguousarray(spec, dtype=np.uint32)))


def _merge_call(fn, front, count, insert, mark, spec, cap=None, out=None, want_out=True, want_merged=True, want_report=True,
                want_len=True):
    """A device merging call -> dict(rc, out, out_len, report, merged): report a fresh uint64 array of MERGE_REPORT_WORDS, merged
    the uint8 bits of the merged pairs or None, out_len the call's *out_len, out the merged bytes (uint8[out_len]) when the call
    wrote them, else the buffer as the call left it.  insert: None (NULL), or uint16 -- fewer than count are padded with zeros,
    so that the library never reads behind them; mark: None, or the uint8 bits.  out: the caller's own uint8 buffer (its size is
    the capacity said, or `cap` if given); else cap bytes are provided -- cap None: as many as a size query (out == NULL) asks
    for; want_out False: out == NULL"""
    spec = None if spec is None else np.ascontiguousarray(spec, dtype=np.uint32)
    insert = None if insert is None else np.ascontiguousarray(insert, dtype=np.uint16)
    if insert is not None and insert.size < count:
        insert = np.concatenate((insert, np.zeros(count - insert.size, dtype=np.uint16)))
    mark = None if mark is None else np.ascontiguousarray(mark, dtype=np.uint8)
    n_bits = max((count + 7) // 8, 1)

    def call(buf, cap_said):
        report = np.zeros(MERGE_REPORT_WORDS, dtype=np.uint64)
        merged = np.zeros(n_bits, dtype=np.uint8) if want_merged else None
        n = C.c_size_t(0)
        rc = fn(*front, count, _p(insert), _p(mark), _p(spec), _p(buf), cap_said, C.byref(n) if want_len else None,
                _p(report) if want_report else None, _p(merged))
        return rc, int(n.value), report, None if merged is None else merged[:(count + 7) // 8]

    if not want_out:
        rc, n, report, merged = call(None, 0)
        return dict(rc=rc, out=None, out_len=n, report=report, merged=merged)
    if out is None:
        if cap is None:
            rc, n, report, merged = call(None, 0)
            if rc != 0:
                return dict(rc=rc, out=None, out_len=n, report=report, merged=merged)
            cap = n
        out = np.zeros(max(cap, 1), dtype=np.uint8)
    elif cap is None:
        cap = out.size
    rc, n, report, merged = call(out, cap)
    return dict(rc=rc, out=out[:n] if rc == 0 else out, out_len=n, report=report, merged=merged)


def read_id_len(header_line):
    """fqgpu_read_id_len (host only): the length of the read id of a header line (bytes, with its '@')"""
    line = np.frombuffer(bytes(header_line), dtype=np.uint8)
    return lib().fqgpu_read_id_len(_p(line) if line.size else None, line.size)


PROBES_MAX = 16
PROBE_HEAD_WORDS, PROBE_TABLE_HEAD_WORDS = 8, 8
PROBE_WINDOW_ROWS = 320  # rows the device sums on chip (select.hip); a hit between this and `positions` is added one by one
PROBE_TABLE_NAMES = ("reads_with", "bases_behind", "reads_whole", "reads_emptied")
_ADAPTER_WORDS = ADAPTER_MAX // 4 + 4


def read_probes(adapters, n=None, reserved=(0, 0, 0)):
    """an fqgpu_probes (include/fqgpu.h) as a uint32 array of 4 + 16 * 20 words: n, three reserved words, then the probes --
    `adapters` is a list of read_adapter arrays, at most PROBES_MAX of it is stored; n: what n says when it is not
    len(adapters) (for the checks' tests)"""
    p = np.zeros(4 + PROBES_MAX * _ADAPTER_WORDS, dtype=np.uint32)
    p[0] = len(adapters) if n is None else n
    p[1:4] = reserved
    for k, a in enumerate(adapters[:PROBES_MAX]):
        p[4 + k * _ADAPTER_WORDS:4 + (k + 1) * _ADAPTER_WORDS] = np.ascontiguousarray(a, dtype=np.uint32)
    return p


def probes_check(probes):
    """fqgpu_probes_check -> rc (host only)"""
    return lib().fqgpu_probes_check(_p(probes))


def probe_words(n_probes, positions):
    """fqgpu_probe_words: uint64 words of an adapter-content result (0: n_probes or positions out of range)"""
    return lib().fqgpu_probe_words(n_probes, positions)


def probe_merge(dst, src):
    """fqgpu_probe_merge: dst += src in place (two uint64 arrays) -> rc"""
    assert dst.dtype == np.uint64 and src.dtype == np.uint64 and dst.flags.c_contiguous and src.flags.c_contiguous
    return lib().fqgpu_probe_merge(_p(dst), dst.size, _p(src), src.size)


def probe_view(words):
    """The parts of an adapter-content result (include/fqgpu.h) as numpy views of `words`, a uint64 array of
    probe_words(n, P): the head's words by name, `tables` uint64[n + 1, 8] (PROBE_TABLE_NAMES in front) and `rows`
    uint64[n + 1, P + 1]; table n is "any"."""
    assert words.dtype == np.uint64 and words.ndim == 1 and words.size >= PROBE_HEAD_WORDS
    n, P = int(words[2]), int(words[3])
    stride = PROBE_TABLE_HEAD_WORDS + P + 1
    assert words.size == PROBE_HEAD_WORDS + (n + 1) * stride, "not a result of the probes and positions it names"
    body = words[PROBE_HEAD_WORDS:].reshape(n + 1, stride)
    return dict(n_records=words[0:1], n_bases=words[1:2], n_probes=words[2:3], positions=words[3:4], fingerprint=words[4:5],
                tables=body[:, :PROBE_TABLE_HEAD_WORDS], rows=body[:, PROBE_TABLE_HEAD_WORDS:])


def _probe_call(fn, front, probes, positions, n_recs, want_places=True, cap_words=None):
    """A device probe call -> dict(rc, out, places): out a fresh uint64 array of the size probes and positions ask for
    (cap_words: of that many words instead), places uint16[n_recs, n] or None"""
    probes = np.ascontiguousarray(probes, dtype=np.uint32)
    n = int(probes[0])
    out = np.zeros(max(probe_words(n, positions), 1) if cap_words is None else max(cap_words, 1), dtype=np.uint64)
    places = np.zeros((n_recs, min(max(n, 1), PROBES_MAX)), dtype=np.uint16) if want_places else None
    rc = fn(*front, _p(probes), positions, _p(out), out.size if cap_words is None else cap_words, _p(places))
    return dict(rc=rc, out=out, places=places)


def pinned_empty(n_bytes):
    """uint8 array in page-locked host memory (fqgpu_host_alloc); freed when the array dies"""
    p = lib().fqgpu_host_alloc(max(1, n_bytes))
    if not p:
        raise MemoryError("fqgpu_host_alloc")
    buf = (C.c_uint8 * max(1, n_bytes)).from_address(p)
    arr = np.frombuffer(buf, dtype=np.uint8, count=n_bytes)
    import weakref
    weakref.finalize(buf, lib().fqgpu_host_free, p)
    return arr


def synth_fastq(n_bytes, mode, seed=28, first_read_id=0):
    """-> (uint8 array of whole records, number of reads)"""
    buf = np.empty(n_bytes, dtype=np.uint8)
    n_reads = C.c_uint64(0)
    used = lib().fqgpu_synth_fastq(_p(buf), n_bytes, mode, seed, first_read_id, C.byref(n_reads))
    return buf[:used], int(n_reads.value)


def freq_tables(raw, recs, device=0, want_counts=False):
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    sft = np.zeros(1, dtype=SEQ_FT_DTYPE)
    qft = np.zeros(1, dtype=QUAL_FT_DTYPE)
    sc = np.zeros((SEQ_MODELS, SEQ_ALPHA), dtype=np.uint32) if want_counts else None
    qc = np.zeros((QUAL_MODELS, QUAL_ALPHA), dtype=np.uint32) if want_counts else None
    _check(lib().fqgpu_freq_tables(device, _p(raw), raw.size, _p(recs), len(recs), _p(sft), _p(qft),
                                   _p(sc), _p(qc)), "freq_tables")
    return (sft, qft, sc, qc) if want_counts else (sft, qft)


def tables_from_counts(seq_counts, qual_counts, device=0):
    sft = np.zeros(1, dtype=SEQ_FT_DTYPE)
    qft = np.zeros(1, dtype=QUAL_FT_DTYPE)
    sc = np.ascontiguousarray(seq_counts, dtype=np.uint32)
    qc = np.ascontiguousarray(qual_counts, dtype=np.uint32)
    _check(lib().fqgpu_tables_from_counts(device, _p(sc), _p(qc), _p(sft), _p(qft)), "tables_from_counts")
    return sft, qft


class DBlock:
    """Device-resident block (fqgpu_dblock)."""

    def __init__(self, ctx, raw, recs=None):
        """recs=None: the record table is built on the GPU (fqgpu_dblock_create_from_raw)."""
        raw = np.ascontiguousarray(raw, dtype=np.uint8)
        self.ctx = ctx
        h = C.c_void_p()
        if recs is None:
            _check(lib().fqgpu_dblock_create_from_raw(ctx.h, _p(raw), raw.size, C.byref(h)), "dblock_create_from_raw")
            self.h = h
            n, rl = C.c_size_t(), C.c_size_t()
            _check(lib().fqgpu_dblock_records(ctx.h, h, None, 0, C.byref(n), C.byref(rl)), "dblock_records")
            self.raw_len, self.n_recs = rl.value, n.value
        else:
            recs = np.ascontiguousarray(recs, dtype=REC_DTYPE)
            self.raw_len, self.n_recs = raw.size, len(recs)
            _check(lib().fqgpu_dblock_create(ctx.h, _p(raw), raw.size, _p(recs), len(recs), C.byref(h)),
                   "dblock_create")
            self.h = h

    def records(self):
        recs = np.zeros(self.n_recs, dtype=REC_DTYPE)
        _check(lib().fqgpu_dblock_records(self.ctx.h, self.h, _p(recs), self.n_recs, None, None), "dblock_records")
        return recs

    def close(self):
        if getattr(self, "h", None):
            lib().fqgpu_dblock_destroy(self.h)
            self.h = None

    __del__ = close

    def encode(self, flags=0):
        _check(lib().fqgpu_dblock_encode(self.ctx.h, self.h, flags), "dblock_encode")

    def fetch_index(self, stream):
        """decode index of one stream (0 = sequence, 1 = quality) of the last encode with F_DECODE_INDEX"""
        n = C.c_size_t(0)
        _check(lib().fqgpu_dblock_index_bytes(self.h, stream, C.byref(n)), "dblock_index_bytes")
        out = np.zeros(n.value, dtype=np.uint8)
        if n.value:
            _check(lib().fqgpu_dblock_fetch_index(self.ctx.h, self.h, stream, _p(out), out.size), "dblock_fetch_index")
        return out

    def load_index(self, stream, data):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        return lib().fqgpu_dblock_load_index(self.ctx.h, self.h, stream, _p(data) if data.size else None, data.size)

    def wipe(self):
        _check(lib().fqgpu_dblock_wipe(self.ctx.h, self.h), "dblock_wipe")

    def crc32(self, want_len=False):
        """fqgpu_dblock_crc32: zlib CRC-32 of the canonical bytes of the raw block as it lies on the device
        (want_len: -> (crc, canonical length))"""
        crc, n = C.c_uint32(0), C.c_size_t(0)
        _check(lib().fqgpu_dblock_crc32(self.ctx.h, self.h, C.byref(crc), C.byref(n)), "dblock_crc32")
        return (crc.value, n.value) if want_len else crc.value

    def stats(self, positions):
        """fqgpu_dblock_stats: the read summary of the raw block as it lies on the device -> uint64 array (stats_view)"""
        rc, out = _stats_call(lib().fqgpu_dblock_stats, positions, self.ctx.h, self.h)
        _check(rc, "dblock_stats")
        return out

    def probe(self, probes, positions, want_places=True, **kw):
        """fqgpu_dblock_probe: the adapter content of the raw block as it lies on the device, for `probes` (read_probes) ->
        dict(rc, out, places); see _probe_call, probe_view"""
        return _probe_call(lib().fqgpu_dblock_probe, (self.ctx.h, self.h), probes, positions, self.n_recs, want_places, **kw)

    def filter(self, flt, **kw):
        """fqgpu_dblock_filter: the reads of the raw block, as it lies on the device, that pass `flt` (read_filter) ->
        dict(rc, out, out_len, report, keep); see _select_call"""
        return _select_call(lib().fqgpu_dblock_filter, (self.ctx.h, self.h), (flt,), self.n_recs, **kw)

    def trim(self, trim, flt=None, **kw):
        """fqgpu_dblock_trim: the reads of the raw block, as it lies on the device, trimmed by `trim` (read_trim) and then
        judged by `flt` (read_filter; None: every read that is not emptied is kept) -> dict(rc, out, out_len, report, keep,
        win); see _select_call"""
        return _select_call(lib().fqgpu_dblock_trim, (self.ctx.h, self.h), (trim, flt), self.n_recs, more=("win",), **kw)

    def clip(self, adapter, trim=None, flt=None, **kw):
        """fqgpu_dblock_clip: the reads of the raw block clipped at `adapter` (read_adapter; None: no adapter), trimmed by
        `trim` (None: nothing beyond the clip) and then judged by `flt` -> dict(rc, out, out_len, report, keep, win); see
        _select_call"""
        return _select_call(lib().fqgpu_dblock_clip, (self.ctx.h, self.h), (adapter, trim, flt), self.n_recs, more=("win",), **kw)

    def tailtrim(self, adapter=None, tail=None, trim=None, flt=None, **kw):
        """fqgpu_dblock_tailtrim: the reads of the raw block clipped at `adapter` (None: no adapter), their poly-X tail and the
        sliding-window cut of `tail` (read_tail; None: neither) taken, trimmed by `trim` and then judged by `flt` ->
        dict(rc, out, out_len, report, keep, win, places); see _select_call"""
        return _select_call(lib().fqgpu_dblock_tailtrim, (self.ctx.h, self.h), (adapter, tail, trim, flt), self.n_recs, more=("win", "places"),
                            report_words=TAIL_REPORT_WORDS, **kw)

    def select_marked(self, first, end, mark=None, adapter=None, tail=None, trim=None, flt=None, **kw):
        """fqgpu_dblock_select_marked: the records [first, end) of the raw block judged as tailtrim judges them, a record whose
        bit in `mark` is 0 dropped whatever its verdict -> dict(rc, out, out_len, report, keep, win, places), all relative to
        `first`; see _range_call"""
        return _range_call(lib().fqgpu_dblock_select_marked, (self.ctx.h, self.h), (adapter, tail, trim, flt), first, end, mark, **kw)

    def select_limited(self, first, end, mark=None, limit=None, adapter=None, tail=None, trim=None, flt=None, **kw):
        """fqgpu_dblock_select_limited: select_marked with a per-record limit (uint16 of end - first entries; None: NULL) in
        front of its steps -> as select_marked, report words 21 / 22 counted"""
        return _range_call(lib().fqgpu_dblock_select_limited, (self.ctx.h, self.h), (adapter, tail, trim, flt), first, end, mark, limit, **kw)

    def pair_correct(self, first, other, other_first, count, insert, spec, **kw):
        """fqgpu_dblock_pair_correct: with the insert sizes `insert` (pair_overlap's) the mismatched bases inside the overlap of
        this block's records first + i (mate 1) and `other`'s other_first + i (mate 2), i < count, corrected for `spec`
        (read_correct); it CHANGES both blocks' raw bytes -> dict(rc, report, fixed_a, fixed_b); see _correct_call"""
        return _correct_call(lib().fqgpu_dblock_pair_correct, (self.ctx.h, self.h, first, other.h if other is not None else None, other_first),
                             count, insert, spec, **kw)

    def pair_merge(self, first, other, other_first, count, insert, mark, spec, **kw):
        """fqgpu_dblock_pair_merge: with the insert sizes `insert` (pair_overlap's) and the mark bits `mark` (None: every pair)
        this block's records first + i (mate 1) and `other`'s other_first + i (mate 2), i < count, merged into one read each for
        `spec` (read_merge); both blocks stay as they are -> dict(rc, out, out_len, report, merged); see _merge_call"""
        return _merge_call(lib().fqgpu_dblock_pair_merge, (self.ctx.h, self.h, first, other.h if other is not None else None, other_first),
                           count, insert, mark, spec, **kw)

    def pair_overlap(self, first, other, other_first, count, spec, **kw):
        """fqgpu_dblock_pair_overlap: the mate overlap of this block's records first + i (mate 1) and `other`'s other_first + i
        (mate 2), i < count, for `spec` (read_overlap) -> dict(rc, out, limit_a, limit_b, insert); see _overlap_call"""
        return _overlap_call(lib().fqgpu_dblock_pair_overlap, (self.ctx.h, self.h, first, other.h if other is not None else None, other_first),
                             count, spec, **kw)

    def pair_names(self, first, other, other_first, count):
        """fqgpu_dblock_pair_names: the read ids of this block's records first + i against `other`'s other_first + i, i < count
        -> (rc, mismatch): the first i whose ids differ, None when there is none"""
        m = C.c_size_t(7)
        rc = lib().fqgpu_dblock_pair_names(self.ctx.h, self.h, first, other.h if other is not None else None, other_first, count, C.byref(m))
        return rc, None if m.value == NO_MISMATCH else m.value

    def status(self):
        a, b, c, d = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
        rc = lib().fqgpu_dblock_status(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d))
        return rc, dict(seq_len=a.value, qual_len=b.value, n_pos_len=c.value, n_bases=d.value)

    def longest_chain(self):
        """(seq, qual): longest serial run of symbols one lane walked in the last encode."""
        a, b = C.c_uint(), C.c_uint()
        _check(lib().fqgpu_dblock_longest_chain(self.h, C.byref(a), C.byref(b)), "dblock_longest_chain")
        return a.value, b.value

    def seq_handover(self):
        """(handed over, kept): segment groups of the sequence chains of the last encode (Context.set_seq_handover)"""
        a, b = C.c_uint(), C.c_uint()
        _check(lib().fqgpu_dblock_seq_handover(self.h, C.byref(a), C.byref(b)), "dblock_seq_handover")
        return a.value, b.value

    def qual_segment_classes(self):
        """segments of the quality chains of the last encode by class -> dict(transparent, anchored, uniform, opaque)"""
        c = (C.c_size_t * 4)()
        _check(lib().fqgpu_dblock_qual_segment_classes(self.ctx.h, self.h, c), "dblock_qual_segment_classes")
        return dict(transparent=c[0], anchored=c[1], uniform=c[2], opaque=c[3])

    def qual_segments(self):
        """fqgpu_dblock_qual_segments: the segments of the quality chains of the last encode one by one -> dict(cls: uint8,
        anchor: uint32, ctx: uint32), see include/fqgpu.h"""
        n = C.c_size_t(0)
        rc = lib().fqgpu_dblock_qual_segments(self.ctx.h, self.h, None, None, None, 0, C.byref(n))
        if rc != -1:  # (FQGPU_E_OVERFLOW: there are segments, n says how many)
            _check(rc, "dblock_qual_segments")
        cls, anchor, ctx = np.zeros(n.value, dtype=np.uint8), np.zeros(n.value, dtype=np.uint32), np.zeros(n.value, dtype=np.uint32)
        if n.value:
            _check(lib().fqgpu_dblock_qual_segments(self.ctx.h, self.h, _p(cls), _p(anchor), _p(ctx), n.value, C.byref(n)),
                   "dblock_qual_segments")
        return dict(cls=cls, anchor=anchor, ctx=ctx)

    def fetch(self, raw=False):
        rc, st = self.status()
        _check(rc, "dblock_status")
        seq = np.zeros(st["seq_len"], dtype=np.uint8)
        qual = np.zeros(st["qual_len"], dtype=np.uint8)
        rl = np.zeros(self.n_recs, dtype=np.uint16)
        nc = np.zeros(self.n_recs, dtype=np.uint16)
        npos = np.zeros(st["n_pos_len"], dtype=np.uint16)
        rw = np.zeros(self.raw_len, dtype=np.uint8) if raw else None
        _check(lib().fqgpu_dblock_fetch(self.ctx.h, self.h, _p(seq), _p(qual), _p(rl), _p(nc), _p(npos),
                                        _p(rw)), "dblock_fetch")
        return dict(seq=seq, qual=qual, readlens=rl, n_count=nc, n_pos=npos, raw=rw)

    def fetch_raw(self):
        rw = np.zeros(self.raw_len, dtype=np.uint8)
        _check(lib().fqgpu_dblock_fetch(self.ctx.h, self.h, None, None, None, None, None, _p(rw)),
               "dblock_fetch")
        return rw

    def load_streams(self, seq, qual, n_count, n_pos):
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        qual = np.ascontiguousarray(qual, dtype=np.uint8)
        n_count = np.ascontiguousarray(n_count, dtype=np.uint16)
        n_pos = np.ascontiguousarray(n_pos, dtype=np.uint16)
        _check(lib().fqgpu_dblock_load_streams(self.ctx.h, self.h, _p(seq), seq.size, _p(qual), qual.size,
                                               _p(n_count), _p(n_pos), n_pos.size), "load_streams")


class _HeaderStreams(C.Structure):
    """fqgpu_header_streams"""
    _fields_ = [("field_types", C.c_void_p), ("separators", C.c_char_p), ("n_fields", C.c_uint),
                ("first_header", C.c_void_p), ("first_header_len", C.c_size_t), ("sizes", C.c_void_p),
                ("streams", C.POINTER(C.c_void_p))]


class Context:
    """fqgpu_ctx: the device-side equivalent of a reference Compression/DecompressionWorkspace."""

    def __init__(self, seq_ft, qual_ft, device=0):
        self.seq_ft = np.ascontiguousarray(seq_ft)
        self.qual_ft = np.ascontiguousarray(qual_ft)
        assert self.seq_ft.nbytes == SEQ_FT_DTYPE.itemsize and self.qual_ft.nbytes == QUAL_FT_DTYPE.itemsize
        h = C.c_void_p()
        _check(lib().fqgpu_ctx_create(device, _p(self.seq_ft), _p(self.qual_ft), C.byref(h)), "ctx_create")
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            lib().fqgpu_ctx_destroy(self.h)
            self.h = None

    __del__ = close

    def set_chain_params(self, segment=0, seq_generic=False, seq_segment=None, seq_group=None):
        """seq_group: (max_segments, min_groups) of fqgpu_ctx_set_seq_group, or max_segments alone."""
        flags = 1 if seq_generic else 0
        if seq_segment is not None:
            _check(lib().fqgpu_ctx_set_seq_segment(self.h, seq_segment), "set_seq_segment")
        if seq_group is not None:
            q, g = seq_group if isinstance(seq_group, tuple) else (seq_group, 0)
            _check(lib().fqgpu_ctx_set_seq_group(self.h, q, g), "set_seq_group")
        _check(lib().fqgpu_ctx_set_chain_params(self.h, segment, flags), "set_chain_params")

    def set_seq_handover(self, cap, prefix_segments=1):
        """fqgpu_ctx_set_seq_handover: groups down to `cap` states behind `prefix_segments` segments leave the set walk
        (cap 0: none does)"""
        _check(lib().fqgpu_ctx_set_seq_handover(self.h, cap, prefix_segments), "set_seq_handover")

    def set_index_stride(self, symbols):
        _check(lib().fqgpu_ctx_set_index_stride(self.h, symbols), "set_index_stride")

    def set_lanes(self, lanes):
        _check(lib().fqgpu_ctx_set_lanes(self.h, lanes), "set_lanes")

    def sync(self):
        _check(lib().fqgpu_sync(self.h), "sync")

    def fill_scratch(self, byte):
        """fqgpu_ctx_fill_scratch (a diagnostic for tests): every device scratch buffer of the handle, but the ones that
        carry state on purpose, set to `byte` up to its capacity -> (buffers, bytes) filled"""
        n, nb = C.c_size_t(0), C.c_size_t(0)
        _check(lib().fqgpu_ctx_fill_scratch(self.h, byte, C.byref(n), C.byref(nb)), "fill_scratch")
        return n.value, nb.value

    def decode_forms(self):
        """fqgpu_ctx_decode_forms (a diagnostic for tests): which kernel forms the handle's last decode launch used ->
        dict(forms: DEC_FORM_* bits, qual_chains, qual_strides, n_cus)"""
        f, c, s, n = C.c_uint(0), C.c_uint(0), C.c_uint(0), C.c_uint(0)
        _check(lib().fqgpu_ctx_decode_forms(self.h, C.byref(f), C.byref(c), C.byref(s), C.byref(n)), "decode_forms")
        return dict(forms=f.value, qual_chains=c.value, qual_strides=s.value, n_cus=n.value)

    def chunk_crc32(self):
        """fqgpu_chunk_crc32 -> (rc, crc, len): the chunk on the staging block -- the one encode_raw has just coded, or
        the one the last whole-chunk decode restored"""
        crc, n = C.c_uint32(0), C.c_size_t(0)
        rc = lib().fqgpu_chunk_crc32(self.h, C.byref(crc), C.byref(n))
        return rc, crc.value, n.value

    def chunk_stats(self, positions):
        """fqgpu_chunk_stats -> (rc, words): the read summary of the chunk on the staging block, where chunk_crc32 is valid"""
        return _stats_call(lib().fqgpu_chunk_stats, positions, self.h)

    def chunk_probe(self, probes, positions, n_recs, want_places=True, **kw):
        """fqgpu_chunk_probe: the adapter content of the chunk on the staging block (n_recs records), where chunk_stats is
        valid -> dict(rc, out, places); see _probe_call"""
        return _probe_call(lib().fqgpu_chunk_probe, (self.h,), probes, positions, n_recs, want_places, **kw)

    def chunk_filter(self, flt, n_recs, **kw):
        """fqgpu_chunk_filter: the reads of the chunk on the staging block (n_recs records) that pass `flt`, where chunk_stats
        is valid -> dict(rc, out, out_len, report, keep); see _select_call"""
        return _select_call(lib().fqgpu_chunk_filter, (self.h,), (flt,), n_recs, **kw)

    def chunk_trim(self, trim, n_recs, flt=None, **kw):
        """fqgpu_chunk_trim: the reads of the chunk on the staging block (n_recs records) trimmed by `trim` and then judged by
        `flt`, where chunk_filter is valid -> dict(rc, out, out_len, report, keep, win); see _select_call"""
        return _select_call(lib().fqgpu_chunk_trim, (self.h,), (trim, flt), n_recs, more=("win",), **kw)

    def chunk_clip(self, adapter, n_recs, trim=None, flt=None, **kw):
        """fqgpu_chunk_clip: the reads of the chunk on the staging block (n_recs records) clipped at `adapter`, trimmed by
        `trim` and then judged by `flt`, where chunk_trim is valid -> dict(rc, out, out_len, report, keep, win); see _select_call"""
        return _select_call(lib().fqgpu_chunk_clip, (self.h,), (adapter, trim, flt), n_recs, more=("win",), **kw)

    def chunk_tailtrim(self, n_recs, adapter=None, tail=None, trim=None, flt=None, **kw):
        """fqgpu_chunk_tailtrim: the reads of the chunk on the staging block (n_recs records) clipped at `adapter`, their
        poly-X tail and the sliding-window cut of `tail` taken, trimmed by `trim` and then judged by `flt`, where chunk_clip is
        valid -> dict(rc, out, out_len, report, keep, win, places); see _select_call"""
        return _select_call(lib().fqgpu_chunk_tailtrim, (self.h,), (adapter, tail, trim, flt), n_recs, more=("win", "places"),
                            report_words=TAIL_REPORT_WORDS, **kw)

    def chunk_select_marked(self, first, end, mark=None, adapter=None, tail=None, trim=None, flt=None, **kw):
        """fqgpu_chunk_select_marked: the records [first, end) of the chunk on the staging block, where chunk_tailtrim is
        valid, against `mark` -> dict(rc, out, out_len, report, keep, win, places); see _range_call"""
        return _range_call(lib().fqgpu_chunk_select_marked, (self.h,), (adapter, tail, trim, flt), first, end, mark, **kw)

    def chunk_select_limited(self, first, end, mark=None, limit=None, adapter=None, tail=None, trim=None, flt=None, **kw):
        """fqgpu_chunk_select_limited: chunk_select_marked with a per-record limit -> as DBlock.select_limited"""
        return _range_call(lib().fqgpu_chunk_select_limited, (self.h,), (adapter, tail, trim, flt), first, end, mark, limit, **kw)

    def chunk_pair_correct(self, first, other, other_first, count, insert, spec, **kw):
        """fqgpu_chunk_pair_correct: the correction inside the mate overlap of the chunk staged here (mate 1) and the chunk staged
        on the Context `other` (mate 2); it CHANGES both staged chunks -> as DBlock.pair_correct"""
        return _correct_call(lib().fqgpu_chunk_pair_correct, (self.h, first, other.h if other is not None else None, other_first), count, insert,
                             spec, **kw)

    def chunk_pair_merge(self, first, other, other_first, count, insert, mark, spec, **kw):
        """fqgpu_chunk_pair_merge: the mates of the chunk staged here (mate 1) and of the chunk staged on the Context `other`
        (mate 2) merged; both staged chunks stay as they are -> as DBlock.pair_merge"""
        return _merge_call(lib().fqgpu_chunk_pair_merge, (self.h, first, other.h if other is not None else None, other_first), count, insert,
                           mark, spec, **kw)

    def chunk_pair_overlap(self, first, other, other_first, count, spec, **kw):
        """fqgpu_chunk_pair_overlap: the mate overlap of the chunk staged here (mate 1) and the chunk staged on the Context
        `other` (mate 2) -> as DBlock.pair_overlap"""
        return _overlap_call(lib().fqgpu_chunk_pair_overlap, (self.h, first, other.h if other is not None else None, other_first), count, spec, **kw)

    def chunk_pair_names(self, first, other, other_first, count):
        """fqgpu_chunk_pair_names: the read ids of the chunk staged here against those of the chunk staged on the Context
        `other` -> (rc, mismatch) as DBlock.pair_names"""
        m = C.c_size_t(7)
        rc = lib().fqgpu_chunk_pair_names(self.h, first, other.h if other is not None else None, other_first, count, C.byref(m))
        return rc, None if m.value == NO_MISMATCH else m.value

    def set_check_only(self, on=True):
        """fqgpu_ctx_set_check_only: decode_chunk(want_raw=False) decodes and judges, nothing of the chunk comes back"""
        _check(lib().fqgpu_ctx_set_check_only(self.h, 1 if on else 0), "set_check_only")

    def enable_timing(self, on=True, only=None):
        """HIP-event spans around the kernel groups; only: restrict them to one group's label"""
        _check(lib().fqgpu_ctx_timing_only(self.h, only.encode() if only else None), "timing_only")
        _check(lib().fqgpu_ctx_enable_timing(self.h, 1 if on else 0), "enable_timing")

    def last_timing(self):
        t = Timing()
        _check(lib().fqgpu_ctx_last_timing(self.h, C.byref(t)), "last_timing")
        return t.total_ms, [(t.kernel_name[i].decode(), t.kernel_ms[i], t.kernel_calls[i])
                            for i in range(t.n_kernels)]

    def dump_tables(self, stream, model):
        alpha = QUAL_ALPHA if stream else SEQ_ALPHA
        ct = np.zeros(1 + 2048 + 2 * alpha, dtype=np.uint32)
        dt = np.zeros(1 + 4096, dtype=np.uint32)
        _check(lib().fqgpu_ctx_dump_tables(self.h, stream, model, _p(ct), ct.size, _p(dt), dt.size),
               "dump_tables")
        log = int(ct[0] & 0xFFFF)
        return ct[: 1 + (1 << (log - 1)) + 2 * alpha].copy(), dt[: 1 + (1 << log)].copy()

    def dblock(self, raw, recs=None):
        return DBlock(self, raw, recs)

    def decode_dblocks(self, blocks):
        arr = (C.c_void_p * len(blocks))(*[b.h for b in blocks])
        _check(lib().fqgpu_dblocks_decode(self.h, arr, len(blocks)), "dblocks_decode")

    def decode_dblocks_indexing(self, blocks):
        """fqgpu_dblocks_decode_indexing: decodes the blocks from their streams alone and leaves both decode indexes on
        each (DBlock.fetch_index); a damaged block shows in its status()"""
        arr = (C.c_void_p * len(blocks))(*[b.h for b in blocks])
        _check(lib().fqgpu_dblocks_decode_indexing(self.h, arr, len(blocks)), "dblocks_decode_indexing")

    @staticmethod
    def host_buffers(n_recs, n_bases, seq_cap=None, qual_cap=None):
        """Output buffers a worker keeps across chunks (the reference reuses its CompressedBuffersDst)."""
        return dict(seq=np.zeros(bound_seq(n_bases) if seq_cap is None else seq_cap, dtype=np.uint8),
                    qual=np.zeros(bound_qual(n_bases) if qual_cap is None else qual_cap, dtype=np.uint8),
                    readlens=np.zeros(n_recs, dtype=np.uint16), n_count=np.zeros(n_recs, dtype=np.uint16),
                    n_pos=np.zeros(n_bases + 1, dtype=np.uint16))

    def encode_block_into(self, raw, recs, bufs, flags=0):
        """fqgpu_encode_block on the caller's arrays, nothing copied or allocated on the Python side.
        raw is written to when flags has F_WRITE_BACK_N.  -> (rc, seq_len, qual_len, n_pos_len)"""
        sl, ql, nn = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        rc = lib().fqgpu_encode_block(self.h, _p(raw), raw.size, _p(recs), len(recs), _p(bufs["seq"]),
                                      bufs["seq"].size, C.byref(sl), _p(bufs["qual"]), bufs["qual"].size,
                                      C.byref(ql), _p(bufs["readlens"]), _p(bufs["n_count"]), _p(bufs["n_pos"]),
                                      bufs["n_pos"].size, C.byref(nn), flags)
        return rc, sl.value, ql.value, nn.value

    def encode_block(self, raw, recs, flags=0, seq_cap=None, qual_cap=None):
        """Host-pointer call (fqgpu_encode_block) -> dict like the oracle's."""
        raw = np.array(raw, dtype=np.uint8, copy=True)
        recs = np.ascontiguousarray(recs, dtype=REC_DTYPE)
        bufs = self.host_buffers(len(recs), int(recs["len"].sum()), seq_cap, qual_cap)
        rc, sl, ql, nn = self.encode_block_into(raw, recs, bufs, flags)
        return dict(rc=rc, seq=bufs["seq"][:sl].copy(), qual=bufs["qual"][:ql].copy(), readlens=bufs["readlens"],
                    n_count=bufs["n_count"], n_pos=bufs["n_pos"][:nn].copy(), raw_after=raw)

    def encode_raw(self, raw, flags=0, recs=None, header_format=None, want_crc=False, want_stats=None, want_probes=None):
        """The two-halves call on an UNPARSED chunk (fqgpu_encode_begin / _records / _wait / _end): the
        record table comes back from the GPU.  -> dict like encode_block's, plus recs and used_len.
        header_format = (types, separators, first_header) -- types[i] 0 = NUMERIC / 1 = STRING, separators as bytes,
        first_header with its '@' -- also codes the header fields on the device (fqgpu_encode_headers_*):
        `header_fields` = [(flags, content, lengths) per field] or, for a header that cannot be coded,
        `headers_rc` = FQGPU_E_HEADER and `bad_record`.  want_crc: fqgpu_chunk_crc32 between begin and end ->
        `crc32`, `crc_len`; want_stats=P: fqgpu_chunk_stats there too -> `stats`; want_probes=(probes, P): fqgpu_chunk_probe
        there too -> `probe`, `probe_places`."""
        raw = np.array(raw, dtype=np.uint8, copy=True)
        n, nb, used = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        if recs is not None:
            recs = np.ascontiguousarray(recs, dtype=REC_DTYPE)
        rc = lib().fqgpu_encode_begin(self.h, _p(raw), raw.size, _p(recs) if recs is not None else None,
                                      0 if recs is None else len(recs), flags, C.byref(n), C.byref(nb), C.byref(used))
        if rc:
            return dict(rc=rc)
        hdr = {}
        if want_crc:
            crc, crc_len = C.c_uint32(0), C.c_size_t(0)
            rc = lib().fqgpu_chunk_crc32(self.h, C.byref(crc), C.byref(crc_len))
            if rc:
                lib().fqgpu_encode_cancel(self.h)
                return dict(rc=rc)
            hdr["crc32"], hdr["crc_len"] = crc.value, crc_len.value
        if want_stats is not None:
            rc, hdr["stats"] = self.chunk_stats(want_stats)
            if rc:
                lib().fqgpu_encode_cancel(self.h)
                return dict(rc=rc)
        if want_probes is not None:
            got = self.chunk_probe(want_probes[0], want_probes[1], n.value)
            if got["rc"]:
                lib().fqgpu_encode_cancel(self.h)
                return dict(rc=got["rc"])
            hdr["probe"], hdr["probe_places"] = got["out"], got["places"]
        if header_format is not None:
            types, seps, first = header_format
            types = np.ascontiguousarray(types, dtype=np.uint8)
            first = np.frombuffer(bytes(first), dtype=np.uint8)
            rc = lib().fqgpu_encode_headers_begin(self.h, _p(types), bytes(seps), len(types), _p(first), first.size)
            if rc:
                lib().fqgpu_encode_cancel(self.h)
                return dict(rc=rc)
        table = np.zeros(n.value, dtype=REC_DTYPE)
        rc = lib().fqgpu_encode_records(self.h, _p(table), len(table))
        if rc:
            return dict(rc=rc)
        if header_format is not None:
            sizes = np.zeros((len(types), 3), dtype=np.uint32)
            total, bad = C.c_size_t(0), C.c_size_t(0)
            rc = lib().fqgpu_encode_headers_wait(self.h, _p(sizes), C.byref(total), C.byref(bad))
            hdr["headers_rc"] = rc
            if rc:
                hdr["bad_record"] = bad.value
            else:
                out = np.zeros(max(total.value, 1), dtype=np.uint8)
                _check(lib().fqgpu_encode_headers_end(self.h, _p(out), out.size), "fqgpu_encode_headers_end")
                fields, at = [], 0
                for f in range(len(types)):
                    parts = []
                    for k in range(3):
                        parts.append(out[at:at + int(sizes[f, k])].copy())
                        at += int(sizes[f, k])
                    fields.append(tuple(parts))
                assert at == total.value
                hdr["header_fields"] = fields
        sl, ql, nn = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        rc = lib().fqgpu_encode_wait(self.h, C.byref(sl), C.byref(ql), C.byref(nn))
        if rc:
            return dict(rc=rc)
        seq, qual = np.zeros(sl.value, np.uint8), np.zeros(ql.value, np.uint8)
        readlens, n_count, n_pos = np.zeros(n.value, np.uint16), np.zeros(n.value, np.uint16), np.zeros(nn.value, np.uint16)
        rc = lib().fqgpu_encode_end(self.h, _p(raw), _p(seq), seq.size, C.byref(sl), _p(qual), qual.size, C.byref(ql),
                                    _p(readlens), _p(n_count), _p(n_pos), n_pos.size, C.byref(nn))
        if rc == 0 and (flags & F_DECODE_INDEX):
            hdr["index"] = []
            for s in (0, 1):
                n_idx = C.c_size_t(0)
                _check(lib().fqgpu_encode_index(self.h, s, None, 0, C.byref(n_idx)), "fqgpu_encode_index")
                idx = np.zeros(n_idx.value, dtype=np.uint8)
                _check(lib().fqgpu_encode_index(self.h, s, _p(idx) if idx.size else None, idx.size, C.byref(n_idx)), "fqgpu_encode_index")
                hdr["index"].append(idx)
        return dict(rc=rc, seq=seq, qual=qual, readlens=readlens, n_count=n_count, n_pos=n_pos, raw_after=raw,
                    recs=table, used_len=used.value, n_bases=nb.value, **hdr)

    def decode_chunk(self, header_format, header_fields, readlens, seq, qual, n_count, n_pos, raw_len, index=None,
                     build_index=False, want_raw=True, want_stats=None, want_probes=None):
        """Both decode passes on the device (fqgpu_decode_chunk): headers decoded from their field streams, the chunk
        laid out, sequence and quality decoded.  header_format = (types, separators, first_header) and header_fields =
        [(flags, content, lengths) per field] as encode_raw takes and returns them; index as in decode_block.
        -> dict(rc, raw, recs, laid_out_len, bad_record); bad_record is None unless the layout was refused.
        build_index=True (index must be None): fqgpu_decode_chunk_indexing, the decode builds the chunk's decode indexes
        on the way -> also "index": (seq, qual), two empty arrays after a failure; want_raw=False: raw is None and
        raw_out == NULL goes down -- index only with build_index, or a decode that only checks on a handle in checking
        mode (set_check_only); without either the call is refused (FQGPU_E_ARG).  want_stats=P: fqgpu_chunk_stats
        behind the decode -> also "stats_rc", "stats"; want_probes=(probes, P): fqgpu_chunk_probe behind the decode -> also
        "probe_rc", "probe", "probe_places"."""
        args, keep = _chunk_args(header_format, header_fields, readlens, seq, qual, n_count, n_pos, index)
        raw = np.zeros(raw_len, dtype=np.uint8) if want_raw else None  # (None: index only, or a handle that only checks)
        recs = np.zeros(len(readlens), dtype=REC_DTYPE)
        laid, bad = C.c_size_t(0), C.c_size_t(0)
        if build_index:
            assert index is None, "an indexing decode takes no index"
            rc = lib().fqgpu_decode_chunk_indexing(self.h, *args[:11], _p(raw), raw_len, _p(recs), C.byref(laid), C.byref(bad))
            built = []
            for s in (0, 1):
                n_idx = C.c_size_t(0)
                lib().fqgpu_decode_index(self.h, s, None, 0, C.byref(n_idx))
                idx = np.zeros(n_idx.value, dtype=np.uint8)
                if idx.size:
                    _check(lib().fqgpu_decode_index(self.h, s, _p(idx), idx.size, C.byref(n_idx)), "fqgpu_decode_index")
                built.append(idx)
            return dict(rc=rc, raw=raw, recs=recs, laid_out_len=laid.value, bad_record=_bad(bad), index=tuple(built),
                        **self._want_stats(want_stats), **self._want_probes(want_probes, len(readlens)))
        rc = lib().fqgpu_decode_chunk(self.h, *args, _p(raw), raw_len, _p(recs), C.byref(laid), C.byref(bad))
        return dict(rc=rc, raw=raw, recs=recs, laid_out_len=laid.value, bad_record=_bad(bad), **self._want_stats(want_stats),
                    **self._want_probes(want_probes, len(readlens)))

    def _want_stats(self, positions):
        if positions is None:
            return {}
        rc, words = self.chunk_stats(positions)
        return dict(stats_rc=rc, stats=words)

    def _want_probes(self, want, n_recs):
        if want is None:
            return {}
        got = self.chunk_probe(want[0], want[1], n_recs)
        return dict(probe_rc=got["rc"], probe=got["out"], probe_places=got["places"])

    def decode_chunk_range(self, header_format, header_fields, readlens, seq, qual, n_count, n_pos, raw_len, first, end,
                           index=None, out_cap=None):
        """Records [first, end) of a chunk (fqgpu_decode_chunk_range), arguments as decode_chunk.  out_cap None: a buffer
        of the range's size (asked for first); 0: the size query alone (raw is None).  -> dict(rc, raw, recs, out_len,
        bad_record); raw holds out_len bytes on success, recs the range's records relative to raw."""
        args, keep = _chunk_args(header_format, header_fields, readlens, seq, qual, n_count, n_pos, index)
        return self._decode_range(lib().fqgpu_decode_chunk_range, args, raw_len, first, end, out_cap, out=None)

    def decode_chunk_fasta(self, header_format, header_fields, readlens, seq, n_count, n_pos, raw_len, first, end,
                           seq_index=None, out_cap=None, out=None):
        """Records [first, end) of a chunk as FASTA, from the sequence stream alone (fqgpu_decode_chunk_fasta): arguments
        as decode_chunk_range without the quality stream; seq_index: the chunk's sequence decode index or None; raw_len:
        the chunk's FASTQ size.  out: a caller's uint8 buffer to decode into (its size is out_cap).  -> as
        decode_chunk_range; recs hold seq_off into the FASTA bytes and qual_off 0."""
        index = None if seq_index is None else (seq_index, np.zeros(0, np.uint8))
        a, keep = _chunk_args(header_format, header_fields, readlens, seq, np.zeros(0, np.uint8), n_count, n_pos, index)
        args = a[:5] + a[7:13]  # (no quality stream, no quality index)
        if out is not None:
            out_cap = out.size
        return self._decode_range(lib().fqgpu_decode_chunk_fasta, args, raw_len, first, end, out_cap, out)

    def _decode_range(self, fn, args, raw_len, first, end, out_cap, out):
        olen, bad = C.c_size_t(0), C.c_size_t(0)

        def call(out, cap, recs):
            return fn(self.h, *args, raw_len, first, end, _p(out) if out is not None else None, cap,
                      C.byref(olen), _p(recs) if recs is not None else None, C.byref(bad))

        n_out = max(end - first, 0)
        if out_cap is None:
            rc = call(None, 0, None)
            if rc != 0:
                return dict(rc=rc, raw=None, recs=None, out_len=olen.value, bad_record=_bad(bad))
            out_cap = olen.value
        raw = recs = None
        if out_cap:
            raw = out if out is not None else np.zeros(out_cap, dtype=np.uint8)
            recs = np.zeros(n_out, dtype=REC_DTYPE)
        rc = call(raw, out_cap, recs)
        if raw is not None and rc == 0:
            raw = raw[:olen.value]
        return dict(rc=rc, raw=raw, recs=recs, out_len=olen.value, bad_record=_bad(bad))

    def decode_block(self, seq, qual, n_count, n_pos, recs, raw_skeleton, index=None):
        """index = (sequence index, quality index) as encode_raw(flags=F_DECODE_INDEX) returns them:
        fqgpu_decode_block_indexed, every stream decoded from all its snapshots at once"""
        out = np.array(raw_skeleton, dtype=np.uint8, copy=True)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        qual = np.ascontiguousarray(qual, dtype=np.uint8)
        n_count = np.ascontiguousarray(n_count, dtype=np.uint16)
        n_pos = np.ascontiguousarray(n_pos, dtype=np.uint16)
        recs = np.ascontiguousarray(recs, dtype=REC_DTYPE)
        if index is not None:
            si, qi = (np.ascontiguousarray(x, dtype=np.uint8) for x in index)
            rc = lib().fqgpu_decode_block_indexed(self.h, _p(seq), seq.size, _p(qual), qual.size, _p(n_count), n_count.size,
                                                  _p(n_pos), n_pos.size, _p(recs), len(recs), _p(out), out.size,
                                                  _p(si) if si.size else None, si.size, _p(qi) if qi.size else None, qi.size)
            return rc, out
        rc = lib().fqgpu_decode_block(self.h, _p(seq), seq.size, _p(qual), qual.size, _p(n_count), n_count.size,
                                      _p(n_pos), n_pos.size, _p(recs), len(recs), _p(out), out.size)
        return rc, out
