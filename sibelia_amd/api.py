"""Host-side mirror of the reference's BlockFinder surface over the C ABI (include/sibelia_amd.h).

`BlockFinder` keeps the reference's method names and argument meaning
(reference src/blockfinder.h:40-45): PerformGraphSimplifications(k, minBranchSize, maxIterations, f),
SerializeCondensedGraph(k, out), plus the enumeration / state accessors the parity tests need.
All compute happens in libsibelia_amd.so's HIP kernels; importing this module without the
built library, or constructing a BlockFinder without a GPU, fails loudly -- there is no fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from . import formats
from .build import LIB

INST_DTYPE = np.dtype([("id", "<u4"), ("chr", "<u4"), ("pos", "<u4")])
EDGE_DTYPE = formats.EDGE_DTYPE
PROGRESS_FN = C.CFUNCTYPE(None, C.c_size_t, C.c_int, C.c_void_p)

EXPORTS = ["sbl_create", "sbl_destroy", "sbl_load", "sbl_enumerate", "sbl_simplify_stage", "sbl_get_state", "sbl_nchr",
           "sbl_list_edges", "sbl_last_stats", "sbl_last_error", "sbl_strerror", "sbl_set_window",
           "sbl_save_state", "sbl_restore_state", "sbl_load_fasta", "sbl_record_name", "sbl_kmer_hashes", "sbl_generate_blocks", "sbl_synteny_stats", "sbl_postprocess", "sbl_serialize_graph",
           "sbl_set_tempfile_mode", "sbl_rand_advance", "sbl_shard_layout", "sbl_shard_exchange_plan", "sbl_glue_stripes", "sbl_comm_unique_id", "sbl_comm_attach_rccl", "sbl_comm_attach_local", "sbl_comm_detach",
           "sbl_longk_slices", "sbl_longk_value_bounds", "sbl_longk_owner", "sbl_longk_halo_plan",
           "sbl_blocks_sequences", "sbl_blocks_sequences_times", "sbl_blocks_gff", "sbl_blocks_coords",
           "sbl_correct_boundaries", "sbl_align_windows", "sbl_correct_stats",
           "sbl_align_pairs", "sbl_align_unique_blocks", "sbl_align_stats", "sbl_record_size",
           "sbl_align_groups", "sbl_align_block_groups", "sbl_align_set_gap_open", "sbl_align_get_gap_open",
           "sbl_align_set_wide", "sbl_align_get_wide", "sbl_align_wide_stats",
           "sbl_uncovered_calls", "sbl_spell_text", "sbl_spell_text_times", "sbl_group_variants", "sbl_group_variants_times", "sbl_group_distances", "sbl_group_distances_times",
           "sbl_group_concat", "sbl_group_concat_times", "sbl_group_mask", "sbl_group_mask_times", "sbl_group_set_masked", "sbl_group_get_masked", "sbl_group_bootstrap", "sbl_group_bootstrap_times", "sbl_tiny_index",
           "sbl_group_set_partial", "sbl_group_get_partial", "sbl_group_bootstrap_pairs", "sbl_nj_batch", "sbl_nj_batch_times", "sbl_group_parsimony", "sbl_group_parsimony_times",
           "sbl_test_touched_list", "sbl_test_graph_build", "sbl_test_graph_fetch"]

ALIGN_MAX_LEN = 2047                               # SBL_ALIGN_MAX_LEN


class StageStats(C.Structure):
    _fields_ = [("strand_kmers", C.c_uint64), ("bif_count", C.c_uint64), ("instances", C.c_uint64), ("bulges", C.c_uint64),
                ("iterations", C.c_uint32), ("rounds", C.c_uint32), ("replays", C.c_uint32), ("grow_replays", C.c_uint32),
                ("enumerate_ms", C.c_double), ("simplify_ms", C.c_double), ("copyback_ms", C.c_double), ("total_ms", C.c_double),
                ("kmer_table_ms", C.c_double), ("kmer_table_bytes", C.c_uint64),
                ("snapshot_ms", C.c_double), ("reserve_ms", C.c_double), ("commit_ms", C.c_double), ("probe_ms", C.c_double),
                ("executed", C.c_uint64), ("transactions", C.c_uint64),
                ("exchange_ms", C.c_double), ("exchange_bytes", C.c_uint64), ("chain_transactions", C.c_uint64),
                ("commit_event_ms", C.c_double), ("commit_event_launches", C.c_uint64),
                ("dict_checked", C.c_uint64), ("dict_mismatches", C.c_uint64),
                ("ro_ranks", C.c_uint64), ("verdict_ms", C.c_double), ("verdict_bytes", C.c_uint64),
                ("longk_path", C.c_uint64), ("fp_verified", C.c_uint64), ("device_bytes", C.c_uint64)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class CorrectStats(C.Structure):
    _fields_ = [("groups", C.c_uint64), ("alignments", C.c_uint64), ("levels", C.c_uint64), ("launches", C.c_uint64), ("cells", C.c_uint64),
                ("kernel_ms", C.c_double)]


class SyntenyStats(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("groups_resolved", "batch_launches", "batch_indices", "speculated_used", "single_launches",
                                          "batch_declines", "single_declines", "general_indices", "tiny_max_elements", "tiny_max_records",
                                          "general_max_elements", "general_max_records", "tiny_max_keys")]


TINY_INDEXED, TINY_DECLINED, TINY_NOT_ELIGIBLE = 0, 1, 2      # SBL_TINY_*


class TinyRange(C.Structure):
    _fields_ = [("chr", C.c_uint32), ("pad_", C.c_uint32), ("start", C.c_uint64), ("end", C.c_uint64)]


class TinyResult(C.Structure):
    _fields_ = [("status", C.c_uint32), ("bif_count", C.c_uint32), ("first_pos", C.c_uint64), ("npos", C.c_uint64),
                ("first_neg", C.c_uint64), ("nneg", C.c_uint64)]


class AlignDesc(C.Structure):
    _fields_ = [("a", C.c_char_p), ("b", C.c_char_p), ("na", C.c_uint32), ("nb", C.c_uint32)]


GALIGN_OK, GALIGN_SKIPPED = 0, 1                   # SBL_GALIGN_OK, SBL_GALIGN_SKIPPED


class PairDesc(C.Structure):
    _fields_ = [("chr_a", C.c_uint32), ("start_a", C.c_uint64), ("end_a", C.c_uint64), ("rev_a", C.c_uint32),
                ("chr_b", C.c_uint32), ("start_b", C.c_uint64), ("end_b", C.c_uint64), ("rev_b", C.c_uint32)]


PAIR_RESULT_DTYPE = np.dtype([("status", "<u4"), ("score", "<i4"), ("band_w", "<u4"), ("passes", "<u4"),
                              ("first_run", "<u8"), ("nruns", "<u8"), ("row_off", "<u8"), ("row_len", "<u8")])
ALIGN_RUN_DTYPE = np.dtype([("op", "<u4"), ("len", "<u4")])


class AlignStats(C.Structure):
    _fields_ = [("pairs", C.c_uint64), ("skipped", C.c_uint64), ("passes", C.c_uint64), ("launches", C.c_uint64), ("cells", C.c_uint64),
                ("kernel_ms", C.c_double), ("spell_ms", C.c_double)]


class AlignWideStats(C.Structure):                # sbl_align_wide_stats_t
    _fields_ = [("pairs", C.c_uint64), ("passes", C.c_uint64), ("launches", C.c_uint64), ("cells", C.c_uint64), ("kernel_ms", C.c_double)]


class PairAlignment:
    """One sbl_pair_result: status (GALIGN_OK / GALIGN_SKIPPED), score, band_w, passes, runs [(op, length)] with op in '=XID', and the
    two gapped rows.  A skipped pair has score None, no runs and no rows."""
    __slots__ = ("status", "score", "band_w", "passes", "runs", "row_a", "row_b")

    def __init__(self, r, runs, rows):
        self.status, self.band_w, self.passes = int(r["status"]), int(r["band_w"]), int(r["passes"])
        if self.status == GALIGN_OK:
            at, n, off, ln = int(r["first_run"]), int(r["nruns"]), int(r["row_off"]), int(r["row_len"])
            self.score = int(r["score"])
            self.runs = [(chr(int(o)), int(l)) for o, l in runs[at:at + n]]
            self.row_a, self.row_b = rows[off:off + ln], rows[off + ln:off + 2 * ln]
        else:
            self.score, self.runs, self.row_a, self.row_b = None, [], b"", b""


class GroupInst(C.Structure):
    _fields_ = [("chr", C.c_uint32), ("start", C.c_uint64), ("end", C.c_uint64), ("rev", C.c_uint32)]


GROUP_RESULT_DTYPE = np.dtype([("status", "<u4"), ("ninst", "<u4"), ("L", "<u8"), ("row_off", "<u8")])
MEMBER_RESULT_DTYPE = np.dtype([("score", "<i4"), ("band_w", "<u4"), ("passes", "<u4")])
SEGMENT_DTYPE = np.dtype([("group", "<u8"), ("start", "<u8"), ("end", "<u8"), ("before", "<u8"), ("text_off", "<u8"),
                          ("lead", "<u4"), ("gapped", "<u4")])                                        # sbl_group_segment


class PairCounts(C.Structure):                     # sbl_pair_counts
    _fields_ = [("match", C.c_uint64), ("mismatch", C.c_uint64), ("ambiguous", C.c_uint64), ("gap", C.c_uint64)]


class ConcatPart(C.Structure):                     # sbl_concat_part
    _fields_ = [("group", C.c_uint64), ("first", C.c_uint64), ("ncols", C.c_uint64)]


class ConcatSite(C.Structure):                     # sbl_concat_site
    _fields_ = [("group", C.c_uint64), ("col", C.c_uint64), ("before", C.c_uint64)]


CONCAT_ALL, CONCAT_VARIABLE = 0, 1                 # SBL_CONCAT_ALL, SBL_CONCAT_VARIABLE


class MaskInterval(C.Structure):                   # sbl_mask_interval
    _fields_ = [("group", C.c_uint64), ("row", C.c_uint64), ("first", C.c_uint64), ("last", C.c_uint64),
                ("before_first", C.c_uint64), ("before_last", C.c_uint64), ("ndiff", C.c_uint64)]


class NjEdge(C.Structure):                         # sbl_nj_edge
    _fields_ = [("parent", C.c_uint32), ("child", C.c_uint32), ("length", C.c_double)]


NJ_EDGE_DTYPE = np.dtype([("parent", "<u4"), ("child", "<u4"), ("length", "<f8")])      # tree.EDGE_RECORD


class ParsimonyChange(C.Structure):                # sbl_parsimony_change
    _fields_ = [("site", C.c_uint64), ("edge", C.c_uint32), ("from_", C.c_uint8), ("to", C.c_uint8), ("pad_", C.c_uint8 * 2)]


PARSIMONY_CHANGE_DTYPE = np.dtype([("site", "<u8"), ("edge", "<u4"), ("from", "u1"), ("to", "u1"), ("pad_", "u1", (2,))])


class GroupAlignment:
    """One sbl_group_result: status (GALIGN_OK / GALIGN_SKIPPED), L, row_off, the rows (centre first, members in the order given) and
    per member (score, band_w, passes).  A skipped group has L = 0, no rows and member scores None."""
    __slots__ = ("status", "L", "row_off", "rows", "members")

    def __init__(self, r, members, text):
        self.status, self.L, self.row_off = int(r["status"]), int(r["L"]), int(r["row_off"])
        ok = self.status == GALIGN_OK
        self.rows = [text[self.row_off + i * self.L:self.row_off + (i + 1) * self.L] for i in range(int(r["ninst"]))] if ok else []
        self.members = [(int(m["score"]) if ok else None, int(m["band_w"]), int(m["passes"])) for m in members[1:]]


from .formats import CALL_DELETION, CALL_INSERTION, CALL_UNMAPPED, PIECE_LITERAL, PIECE_RECORD      # noqa: E402,F401  SBL_CALL_*, SBL_PIECE_*
CALL_DTYPE = np.dtype([("kind", "<u4"), ("chr", "<u4"), ("start", "<u8"), ("end", "<u8"), ("ref_chr", "<u4"), ("pad_", "<u4"), ("pos", "<u8")])
PIECE_DTYPE = formats.PIECE_DTYPE


class SibeliaError(RuntimeError):
    pass


_lib = None


def load_library():
    """dlopen libsibelia_amd.so (built in-tree by sibelia_amd.build / __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            raise SibeliaError("libsibelia_amd.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(the HIP extension is mandatory, there is no host fallback)")
        L = C.CDLL(LIB)
        L.sbl_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
        L.sbl_destroy.argtypes = [C.c_void_p]
        L.sbl_destroy.restype = None
        L.sbl_load.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_uint64)]
        L.sbl_enumerate.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                                    C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.sbl_simplify_stage.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
        L.sbl_get_state.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.sbl_nchr.argtypes = [C.c_void_p]
        L.sbl_nchr.restype = C.c_uint32
        L.sbl_list_edges.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.sbl_last_stats.argtypes = [C.c_void_p, C.POINTER(StageStats)]
        L.sbl_last_error.argtypes = [C.c_void_p]
        L.sbl_last_error.restype = C.c_char_p
        L.sbl_strerror.argtypes = [C.c_int]
        L.sbl_strerror.restype = C.c_char_p
        L.sbl_set_window.argtypes = [C.c_void_p, C.c_uint32]
        L.sbl_save_state.argtypes = [C.c_void_p]
        L.sbl_restore_state.argtypes = [C.c_void_p]
        L.sbl_load_fasta.argtypes = [C.c_void_p, C.c_char_p]
        L.sbl_record_name.argtypes = [C.c_void_p, C.c_uint32]
        L.sbl_record_name.restype = C.c_char_p
        L.sbl_record_size.argtypes = [C.c_void_p, C.c_uint32]
        L.sbl_record_size.restype = C.c_uint64
        L.sbl_generate_blocks.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.sbl_synteny_stats.argtypes = [C.c_void_p, C.POINTER(SyntenyStats)]
        L.sbl_test_touched_list.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sbl_test_graph_build.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.sbl_test_graph_fetch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint64]
        L.sbl_tiny_index.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(TinyRange), C.c_uint32, C.c_int,
                                     C.POINTER(C.POINTER(TinyResult)), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.sbl_postprocess.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                                      C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]
        L.sbl_serialize_graph.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.sbl_kmer_hashes.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        for fn in (L.sbl_blocks_sequences, L.sbl_blocks_gff, L.sbl_blocks_coords):
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.sbl_blocks_sequences_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.sbl_correct_boundaries.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                                             C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]
        L.sbl_align_windows.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(AlignDesc), C.c_void_p]
        L.sbl_correct_stats.argtypes = [C.c_void_p, C.POINTER(CorrectStats)]
        tail = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.sbl_align_pairs.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(PairDesc)] + tail
        L.sbl_align_unique_blocks.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)] + tail
        L.sbl_align_stats.argtypes = [C.c_void_p, C.POINTER(AlignStats)]
        gtail = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.sbl_align_groups.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(GroupInst)] + gtail
        L.sbl_align_block_groups.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)] + gtail
        L.sbl_align_set_gap_open.argtypes = [C.c_void_p, C.c_uint32]
        L.sbl_align_get_gap_open.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.sbl_align_set_wide.argtypes = [C.c_void_p, C.c_uint32]
        L.sbl_align_get_wide.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.sbl_align_wide_stats.argtypes = [C.c_void_p, C.POINTER(AlignWideStats)]
        L.sbl_uncovered_calls.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.sbl_spell_text.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_char_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.sbl_spell_text_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.sbl_group_variants.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.sbl_group_variants_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.sbl_group_distances.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.POINTER(PairCounts))]
        L.sbl_group_distances_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.sbl_group_concat.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint32, C.c_char_p, C.POINTER(C.c_uint64),
                                       C.POINTER(C.POINTER(ConcatPart)), C.POINTER(C.c_uint64), C.POINTER(C.POINTER(ConcatSite)), C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.sbl_group_concat_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.sbl_group_bootstrap.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32,
                                          C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.sbl_group_bootstrap_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.sbl_group_mask.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(C.POINTER(MaskInterval)), C.POINTER(C.c_uint64)]
        L.sbl_group_mask_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.sbl_group_set_masked.argtypes = [C.c_void_p, C.c_uint32]
        L.sbl_group_set_partial.argtypes = [C.c_void_p, C.c_uint32]
        L.sbl_group_get_partial.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.sbl_group_bootstrap_pairs.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint64))]
        L.sbl_group_get_masked.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.sbl_nj_batch.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_uint32, C.c_uint32, C.POINTER(C.POINTER(NjEdge)), C.POINTER(C.POINTER(C.c_uint64))]
        L.sbl_nj_batch_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.sbl_group_parsimony.argtypes = [C.c_void_p, C.POINTER(NjEdge), C.c_uint32, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(C.c_uint8)),
                                          C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.POINTER(ParsimonyChange)), C.POINTER(C.c_uint64)]
        L.sbl_group_parsimony_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.sbl_comm_unique_id.argtypes = [C.c_void_p]
        L.sbl_comm_attach_rccl.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.sbl_group_create_local.argtypes = [C.c_uint32]
        L.sbl_group_create_local.restype = C.c_void_p
        L.sbl_group_destroy.argtypes = [C.c_void_p]
        L.sbl_group_destroy.restype = None
        L.sbl_comm_attach_local.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.sbl_comm_detach.argtypes = [C.c_void_p]
        _lib = L
    return _lib


def _view(ptr, n, dtype):
    if not n:
        return np.zeros(0, dtype=dtype)
    buf = (C.c_char * (n * dtype.itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype, count=n).copy()


class BlockFinder:
    """SyntenyFinder::BlockFinder for the hot path, backed by one MI355X.

    seqs: upper-case sequences as delivered by the reference FASTA reader (one per FASTARecord)."""

    def __init__(self, seqs: Sequence[bytes], device: int = -1, fasta: Optional[str] = None):
        self.L = load_library()
        self.h = C.c_void_p()
        rc = self.L.sbl_create(C.byref(self.h), device)
        if rc:
            raise SibeliaError("sbl_create: " + self.L.sbl_strerror(rc).decode())
        if fasta is not None:          # FASTAReader + Init on the device (reference src/fasta.cpp:23-104, src/blockfinder.cpp:65-76)
            self._check(self.L.sbl_load_fasta(self.h, os.fsencode(fasta)), "sbl_load_fasta")
            return
        n = len(seqs)
        arr = (C.c_char_p * n)(*[bytes(s) for s in seqs])
        lens = (C.c_uint64 * n)(*[len(s) for s in seqs])
        self._check(self.L.sbl_load(self.h, n, arr, lens), "sbl_load")

    @classmethod
    def from_fasta(cls, path: str, device: int = -1) -> "BlockFinder":
        return cls((), device=device, fasta=path)

    def record_names(self) -> List[str]:
        return [self.L.sbl_record_name(self.h, i).decode() for i in range(self.L.sbl_nchr(self.h))]

    def record_sizes(self) -> List[int]:
        """Lengths of the records as loaded, from the library: the same after either loader."""
        return [int(self.L.sbl_record_size(self.h, i)) for i in range(self.L.sbl_nchr(self.h))]

    def _check(self, rc, what):
        if rc:
            # (a parse error quotes the offending byte and the path as they are: any byte, so decoded the way Python decodes file names)
            msg = os.fsdecode(self.L.sbl_last_error(self.h)) if self.h else ""
            raise SibeliaError("%s: %s (%s)" % (what, self.L.sbl_strerror(rc).decode(), msg))

    def close(self):
        if getattr(self, "h", None):
            self.L.sbl_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- reference surface ---------------------------------------------------------------
    def PerformGraphSimplifications(self, k: int, minBranchSize: int, maxIterations: int,
                                    f: Optional[Callable[[int, int], None]] = None) -> int:
        b = C.c_uint64()
        cb = PROGRESS_FN(lambda p, s, u: f(p, s)) if f else None
        rc = self.L.sbl_simplify_stage(self.h, k, minBranchSize, maxIterations, C.cast(cb, C.c_void_p) if cb else None, None, C.byref(b))
        self._check(rc, "sbl_simplify_stage")
        return b.value

    def SerializeCondensedGraph(self, k: int, out) -> None:
        out.write(formats.dot_text(self.list_edges(k)).decode("latin1"))

    # ---- backend protocol shared with the oracle wrapper (tests/vectors.py) ------------------
    def enumerate(self, k: int) -> Tuple[int, np.ndarray, np.ndarray]:
        bc = C.c_uint32()
        p, q = C.c_void_p(), C.c_void_p()
        n, m = C.c_uint64(), C.c_uint64()
        self._check(self.L.sbl_enumerate(self.h, k, C.byref(bc), C.byref(p), C.byref(n), C.byref(q), C.byref(m)), "sbl_enumerate")
        return bc.value, _view(p.value, n.value, INST_DTYPE), _view(q.value, m.value, INST_DTYPE)

    def simplify_stage(self, k: int, min_branch: int, max_iter: int) -> int:
        return self.PerformGraphSimplifications(k, min_branch, max_iter)

    def state(self) -> Tuple[List[bytes], List[np.ndarray]]:
        seqs, pos = [], []
        for c in range(self.L.sbl_nchr(self.h)):
            s, p, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
            self._check(self.L.sbl_get_state(self.h, c, C.byref(s), C.byref(p), C.byref(n)), "sbl_get_state")
            seqs.append(_view(s.value, n.value, np.dtype("u1")).tobytes())
            pos.append(_view(p.value, n.value, np.dtype("<u4")))
        return seqs, pos

    def state_views(self) -> Tuple[List[np.ndarray], List[np.ndarray]]:
        """The same state as zero-copy numpy views of the library's pinned staging buffer (one bulk device-to-host copy of
        ch[] + op[], 5 B per base; chromosomes are slices of it).  Borrowed: valid until the next mutating call."""
        seqs, pos = [], []
        for c in range(self.L.sbl_nchr(self.h)):
            s, p, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
            self._check(self.L.sbl_get_state(self.h, c, C.byref(s), C.byref(p), C.byref(n)), "sbl_get_state")
            if not n.value:
                seqs.append(np.zeros(0, np.uint8)); pos.append(np.zeros(0, "<u4")); continue
            seqs.append(np.frombuffer((C.c_char * n.value).from_address(s.value), dtype=np.uint8, count=n.value))
            pos.append(np.frombuffer((C.c_char * (4 * n.value)).from_address(p.value), dtype="<u4", count=n.value))
        return seqs, pos

    def list_edges(self, k: int) -> np.ndarray:
        e, n = C.c_void_p(), C.c_uint64()
        self._check(self.L.sbl_list_edges(self.h, k, C.byref(e), C.byref(n)), "sbl_list_edges")
        return _view(e.value, n.value, EDGE_DTYPE)

    def GenerateSyntenyBlocks(self, k: int, trimK: int, minSize: int, sharedOnly: bool = False) -> np.ndarray:
        """BlockFinder::GenerateSyntenyBlocks (reference src/blockfinder.h:43): BlockInstance records (id, chr, start, end)."""
        b, n = C.c_void_p(), C.c_uint64()
        self._check(self.L.sbl_generate_blocks(self.h, k, trimK, minSize, int(sharedOnly), C.byref(b), C.byref(n)), "sbl_generate_blocks")
        return _view(b.value, n.value, formats.BLOCK_DTYPE)

    generate_blocks = GenerateSyntenyBlocks

    def synteny_stats(self) -> dict:
        """Path counters of the last GenerateSyntenyBlocks (sbl_synteny_stats_t, include/sibelia_amd.h): how many candidate blocks the
        small-block kernel indexed (batched / single), how many it declined, how many took the general child index, and the largest of each."""
        s = SyntenyStats()
        self._check(self.L.sbl_synteny_stats(self.h, C.byref(s)), "sbl_synteny_stats")
        return {f: int(getattr(s, f)) for f, _ in s._fields_}

    def tiny_index(self, blocks: Sequence[Sequence[Tuple[int, int, int]]], k: int, batched: bool):
        """TEST ENTRY POINT (sbl_tiny_index, include/sibelia_amd.h): the small-block index at k of every candidate block -- a list of
        (chr, start, end) ranges of the ORIGINAL records -- as GenerateSyntenyBlocks' TrimBlocks reads it; batched: all eligible blocks in
        one launch of the batched kernel, else one launch of the one-block kernel each.  -> per block (status, bif_count, pos, neg) with
        status TINY_INDEXED / TINY_DECLINED / TINY_NOT_ELIGIBLE and INST_DTYPE arrays (count 0 and empty arrays unless indexed)."""
        first = [0]
        for b in blocks:
            first.append(first[-1] + len(b))
        flat = [r for b in blocks for r in b]
        ranges = (TinyRange * max(1, len(flat)))()
        for d, (c, s, e) in zip(ranges, flat):
            d.chr, d.start, d.end = int(c), int(s), int(e)
        res, pos, neg = C.POINTER(TinyResult)(), C.c_void_p(), C.c_void_p()
        self._check(self.L.sbl_tiny_index(self.h, len(blocks), (C.c_uint64 * len(first))(*first), ranges, k, int(bool(batched)),
                                          C.byref(res), C.byref(pos), C.byref(neg)), "sbl_tiny_index")
        out = []
        for i in range(len(blocks)):
            r = res[i]
            p = _view((pos.value or 0) + r.first_pos * INST_DTYPE.itemsize, r.npos, INST_DTYPE)
            q = _view((neg.value or 0) + r.first_neg * INST_DTYPE.itemsize, r.nneg, INST_DTYPE)
            out.append((int(r.status), int(r.bif_count), p, q))
        return out

    def test_touched_list(self, touch: np.ndarray):
        """TEST ENTRY POINT (sbl_test_touched_list, include/sibelia_amd.h): the list of touched ids an incremental snapshot of the
        simplification stage starts from, for the uint8 flags touch[0 .. nid] (id nid is never listed).
        -> (listed ids in the kernel's order, the walking probe's count word, touch and need as the kernel leaves them)"""
        touch = np.ascontiguousarray(touch, dtype=np.uint8)
        nid = len(touch) - 1
        lst, out = np.empty(nid + 1, dtype=np.uint32), np.empty(2, dtype=np.uint32)
        ta, na = np.empty(nid + 1, dtype=np.uint8), np.empty(nid + 1, dtype=np.uint8)
        self._check(self.L.sbl_test_touched_list(self.h, touch.ctypes.data, nid, lst.ctypes.data, out.ctypes.data, ta.ctypes.data, na.ctypes.data),
                    "sbl_test_touched_list")
        assert out[0] <= nid, "k_touched_list counted %d of %d ids" % (out[0], nid)
        return lst[:int(out[0])].copy(), int(out[1]), ta, na

    def test_graph_build(self, k: int, D: int) -> dict:
        """TEST ENTRY POINT (sbl_test_graph_build / sbl_test_graph_fetch, include/sibelia_amd.h): the set-up of a simplification stage
        for (k, D) on the loaded state, which stays as it is.  -> nid, E, nblk, index_from_marks; melem / mid / maux (per strand);
        lists[strand][id] = the element slots of the id's instances in list order (lsize[strand][id] of them); nidst and nmark along
        the lists; perm; bidx (nblk x 4 uint64)."""
        out = np.zeros(8, dtype=np.uint32)
        self._check(self.L.sbl_test_graph_build(self.h, k, D, out.ctypes.data), "sbl_test_graph_build")
        nid, n, nblk, E = int(out[0]), (int(out[1]), int(out[2])), int(out[3]), int(out[4])

        def fetch(what, strand, count, dtype=np.uint32):
            a = np.empty(count, dtype=dtype)
            self._check(self.L.sbl_test_graph_fetch(self.h, what, strand, a.ctypes.data, a.nbytes), "sbl_test_graph_fetch")
            return a
        r = {"nid": nid, "E": E, "nblk": nblk, "index_from_marks": bool(out[5]),
             "melem": [fetch(0, t, n[t]) for t in (0, 1)], "mid": [fetch(1, t, n[t]) for t in (0, 1)], "maux": [fetch(2, t, n[t]) for t in (0, 1)],
             "head": [fetch(3, t, nid) for t in (0, 1)], "lsize": [fetch(4, t, nid) for t in (0, 1)],
             "perm": fetch(7, 0, nid), "bidx": fetch(8, 0, 4 * nblk, np.uint64).reshape(nblk, 4),
             "nodeof": [fetch(11, t, E) for t in (0, 1)]}
        ninst = n[0] + n[1]
        nnext, nslot, nidst, nmark = (fetch(w, 0, ninst) for w in (5, 6, 9, 10))
        r["nslot"], r["nidst"], r["nmark"] = nslot, nidst, nmark
        lists, nodes = [[], []], [[], []]
        for t in (0, 1):
            for i in range(nid):
                nd, chain = int(r["head"][t][i]), []
                while nd != 0xFFFFFFFF:
                    assert nd < ninst and len(chain) <= ninst, "instance list of id %d, strand %d leaves the nodes or loops" % (i, t)
                    chain.append(nd)
                    nd = int(nnext[nd])
                nodes[t].append(np.array(chain, dtype=np.int64))
                lists[t].append(nslot[chain] if chain else np.empty(0, dtype=np.uint32))
        r["lists"], r["nodes"] = lists, nodes
        return r

    def _names_array(self, what: str, names: Optional[Sequence[str]]):
        """`names` as the `const char *const *` of the C entry points, which read one name per loaded record (include/sibelia_amd.h);
        None stays NULL: the names of the loaded records."""
        if names is None:
            return None
        if len(names) != self.L.sbl_nchr(self.h):
            raise ValueError("%s: %d names for %d records" % (what, len(names), self.L.sbl_nchr(self.h)))
        return (C.c_char_p * len(names))(*[x.encode() for x in names])

    def postprocess(self, names: Optional[Sequence[str]] = None, glue: bool = True):
        """GlueStripes (reference src/postprocessor.cpp:37-154) on the blocks of the last GenerateSyntenyBlocks + the texts of
        blocks_coords.txt, genomes_permutations.txt, coverage_report.txt (src/outputgenerator.cpp:162-233)."""
        nm = self._names_array("postprocess", names)
        b, n = C.c_void_p(), C.c_uint64()
        t = [C.c_char_p() for _ in range(3)]
        self._check(self.L.sbl_postprocess(self.h, int(glue), nm, C.byref(b), C.byref(n), C.byref(t[0]), C.byref(t[1]), C.byref(t[2])), "sbl_postprocess")
        return _view(b.value, n.value, formats.BLOCK_DTYPE), [x.value for x in t]

    def correct_boundaries(self, min_block_size: int, n_reference_chr: int, names: Optional[Sequence[str]] = None):
        """Postprocessor::ImproveBlockBoundaries (reference src/postprocessor.cpp:156-348; --correctboundaries) on the blocks of the last
        postprocess: records 0 .. n_reference_chr - 1 are the reference set.  Replaces the context's list; returns it and the three
        texts of postprocess rendered again.  The alignments run in batches on the device (csrc/boundary_align.hip)."""
        nm = self._names_array("correct_boundaries", names)
        b, n = C.c_void_p(), C.c_uint64()
        t = [C.c_char_p() for _ in range(3)]
        self._check(self.L.sbl_correct_boundaries(self.h, min_block_size, n_reference_chr, nm, C.byref(b), C.byref(n),
                                                  C.byref(t[0]), C.byref(t[1]), C.byref(t[2])), "sbl_correct_boundaries")
        return _view(b.value, n.value, formats.BLOCK_DTYPE), [x.value for x in t]

    def align_windows(self, pairs: Sequence[Tuple[bytes, bytes]]) -> np.ndarray:
        """The batched local alignment behind correct_boundaries (Postprocessor::LocalAlignment, reference src/postprocessor.cpp:257-277)
        for pairs of byte strings of at most ALIGN_MAX_LEN characters: one row (a begin, a end, b begin, b end) per pair."""
        pairs = [(bytes(a), bytes(b)) for a, b in pairs]
        desc = (AlignDesc * max(1, len(pairs)))()
        for d, (a, b) in zip(desc, pairs):
            d.a, d.b, d.na, d.nb = a, b, len(a), len(b)
        out = np.zeros((len(pairs), 4), dtype=np.uint32)
        self._check(self.L.sbl_align_windows(self.h, len(pairs), desc, out.ctypes.data), "sbl_align_windows")
        return out

    def correct_stats(self) -> dict:
        """Counters of the last correct_boundaries / align_windows: groups, alignments, levels, launches, cells, kernel_ms."""
        s = CorrectStats()
        self._check(self.L.sbl_correct_stats(self.h, C.byref(s)), "sbl_correct_stats")
        return {f: getattr(s, f) for f, _ in s._fields_}

    def _pair_alignments(self, n, res, runs, nruns, rows, rows_len) -> List[PairAlignment]:
        r = _view(res.value, n, PAIR_RESULT_DTYPE)
        u = _view(runs.value, nruns.value, ALIGN_RUN_DTYPE)
        text = C.string_at(rows.value, rows_len.value) if rows_len.value else b""
        return [PairAlignment(x, u, text) for x in r]

    def align_pairs(self, pairs: Sequence[Tuple[int, int, int, bool, int, int, int, bool]]) -> List[PairAlignment]:
        """Banded global alignment (csrc/block_align.hip; defined in include/sibelia_amd.h) of pairs of ranges of the original records:
        (chr_a, start_a, end_a, rev_a, chr_b, start_b, end_b, rev_b), half-open; rev: read downwards through the complement table."""
        desc = (PairDesc * max(1, len(pairs)))()
        for d, p in zip(desc, pairs):
            d.chr_a, d.start_a, d.end_a, d.rev_a, d.chr_b, d.start_b, d.end_b, d.rev_b = [int(x) for x in p]
        res, runs, rows = C.c_void_p(), C.c_void_p(), C.c_void_p()
        nruns, rows_len = C.c_uint64(), C.c_uint64()
        self._check(self.L.sbl_align_pairs(self.h, len(pairs), desc, C.byref(res), C.byref(runs), C.byref(nruns), C.byref(rows), C.byref(rows_len)), "sbl_align_pairs")
        return self._pair_alignments(len(pairs), res, runs, nruns, rows, rows_len)

    def align_unique_blocks(self, min_block_size: int, n_reference_chr: int):
        """The alignments C-Sibelia.py makes of a two-genome run (reference src/csibelia/C-Sibelia.py:314-323), on the current block list:
        every id with one instance on records 0 .. n_reference_chr - 1 and one outside them, both at least min_block_size long, the
        reference instance first.  -> (ids ascending, descriptors as in align_pairs, [PairAlignment])."""
        ids, desc, res, runs, rows = (C.c_void_p() for _ in range(5))
        n, nruns, rows_len = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.L.sbl_align_unique_blocks(self.h, min_block_size, n_reference_chr, C.byref(ids), C.byref(desc), C.byref(n), C.byref(res),
                                                   C.byref(runs), C.byref(nruns), C.byref(rows), C.byref(rows_len)), "sbl_align_unique_blocks")
        d = C.cast(desc, C.POINTER(PairDesc))
        descs = [(d[i].chr_a, d[i].start_a, d[i].end_a, bool(d[i].rev_a), d[i].chr_b, d[i].start_b, d[i].end_b, bool(d[i].rev_b)) for i in range(n.value)]
        return [int(x) for x in _view(ids.value, n.value, np.dtype("<i4"))], descs, self._pair_alignments(n.value, res, runs, nruns, rows, rows_len)

    def _group_alignments(self, first, res, members, rows, rows_len) -> List[GroupAlignment]:
        r = _view(res.value, len(first) - 1, GROUP_RESULT_DTYPE)
        m = _view(members.value, int(first[-1]), MEMBER_RESULT_DTYPE)
        text = C.string_at(rows.value, rows_len.value) if rows_len.value else b""
        self._group_ninst = [int(x) for x in r["ninst"]]      # for group_variants: rows per group of the last groups call
        return [GroupAlignment(x, m[int(first[g]):int(first[g + 1])], text) for g, x in enumerate(r)]

    def align_groups(self, groups: Sequence[Sequence[Tuple[int, int, int, bool]]]) -> List[GroupAlignment]:
        """Centre-star multiple alignment (csrc/block_align.hip; defined in include/sibelia_amd.h) of groups of ranges of
        the original records: per group a list of (chr, start, end, rev), half-open, the first one the centre."""
        first = [0]
        for g in groups:
            first.append(first[-1] + len(g))
        flat = [i for g in groups for i in g]
        inst = (GroupInst * max(1, len(flat)))()
        for d, i in zip(inst, flat):
            d.chr, d.start, d.end, d.rev = [int(x) for x in i]
        res, members, rows = C.c_void_p(), C.c_void_p(), C.c_void_p()
        rows_len = C.c_uint64()
        self._check(self.L.sbl_align_groups(self.h, len(groups), (C.c_uint64 * len(first))(*first), inst, C.byref(res), C.byref(members),
                                            C.byref(rows), C.byref(rows_len)), "sbl_align_groups")
        return self._group_alignments(first, res, members, rows, rows_len)

    def align_block_groups(self, min_block_size: int):
        """The multiple alignments of the current block list: every id with at least two instances of at least min_block_size bases, all
        of them by ascending (chr, start, end, rev), the first one the centre.
        -> (ids ascending, per id its [(chr, start, end, rev)], [GroupAlignment])."""
        ids, first, inst, res, members, rows = (C.c_void_p() for _ in range(6))
        n, rows_len = C.c_uint64(), C.c_uint64()
        self._check(self.L.sbl_align_block_groups(self.h, min_block_size, C.byref(ids), C.byref(first), C.byref(inst), C.byref(n), C.byref(res),
                                                  C.byref(members), C.byref(rows), C.byref(rows_len)), "sbl_align_block_groups")
        f = [int(x) for x in _view(first.value, n.value + 1, np.dtype("<u8"))]
        d = C.cast(inst, C.POINTER(GroupInst))
        insts = [[(d[i].chr, d[i].start, d[i].end, bool(d[i].rev)) for i in range(f[g], f[g + 1])] for g in range(n.value)]
        return [int(x) for x in _view(ids.value, n.value, np.dtype("<i4"))], insts, self._group_alignments(f, res, members, rows, rows_len)

    def _want_mask(self, what: str, want: Optional[Sequence[bool]]) -> Optional[bytes]:
        """One byte per group of the last groups call for the `want` of group_variants / group_distances / group_concat (None: all)."""
        ngroups = len(getattr(self, "_group_ninst", []))
        if want is not None and len(want) != ngroups:
            raise ValueError("%s: %d flags for %d groups" % (what, len(want), ngroups))
        return None if want is None else bytes(1 if w else 0 for w in want) + b"\0"

    def _class_array(self, what: str, cls: Sequence[int], scalars: Sequence[int], words: str):
        """The classes of the instances of the last groups call for the library; scalars: what else must fit 32 bits; words: the error's."""
        ninst = getattr(self, "_group_ninst", [])
        cls = [int(x) for x in cls]
        if ninst and len(cls) != sum(ninst):
            raise ValueError("%s: %d classes for %d instances" % (what, len(cls), sum(ninst)))
        if any(not 0 <= int(v) <= 2 ** 32 - 1 for v in scalars) or any(not 0 <= x <= 2 ** 32 - 1 for x in cls):
            raise SibeliaError("sbl_%s: bad argument (%s outside 32 bits)" % (what, words))
        return (C.c_uint32 * max(1, len(cls)))(*cls)

    def group_variants(self, want: Optional[Sequence[bool]] = None):
        """The variant segments of the groups of the LAST align_groups / align_block_groups call (csrc/group_variants.hip; defined in
        include/sibelia_amd.h), read off the rows that call left on the device.  want: one flag per group (None: all).
        -> [(group, start, end, before, lead, [gapped slice rows[i][start - lead:end] per row, centre first])] in ascending
        (group, start).  The records as the library returns them (SEGMENT_DTYPE, `gapped` included) stay in `last_group_segments`."""
        mask = self._want_mask("group_variants", want)
        ninst = getattr(self, "_group_ninst", [])
        segs, text = C.c_void_p(), C.c_void_p()
        n, ln = C.c_uint64(), C.c_uint64()
        self._check(self.L.sbl_group_variants(self.h, mask, C.byref(segs), C.byref(n), C.byref(text), C.byref(ln)), "sbl_group_variants")
        self.last_group_segments = v = _view(segs.value, n.value, SEGMENT_DTYPE)
        packed = C.string_at(text.value, ln.value) if ln.value else b""
        out = []
        for x in v:
            g, s, e, lead, at = int(x["group"]), int(x["start"]), int(x["end"]), int(x["lead"]), int(x["text_off"])
            w = e - s + lead
            out.append((g, s, e, int(x["before"]), lead, [packed[at + i * w:at + (i + 1) * w] for i in range(ninst[g])]))
        return out

    def _times(self, what) -> Tuple[float, float]:
        k, d = C.c_double(), C.c_double()
        self._check(getattr(self.L, what)(self.h, C.byref(k), C.byref(d)), what)
        return k.value, d.value

    def group_variants_times(self) -> Tuple[float, float]:
        """(kernel ms, device-to-host copy ms of the slices) of the last group_variants call, from event pairs."""
        return self._times("sbl_group_variants_times")

    def group_distances(self, cls: Sequence[int], nclass: int, want: Optional[Sequence[bool]] = None) -> np.ndarray:
        """The pairwise counts of the groups of the LAST align_groups / align_block_groups call (csrc/group_distances.hip; defined in
        include/sibelia_amd.h), counted on the rows that call left on the device.  cls: one class below nclass per
        instance of that call, flat, in group order; want: one flag per group (None: all).
        -> uint64 array of shape (nclass, nclass, 4), a copy: [f, g] = (match, mismatch, ambiguous, gap(f -> g)) summed over every
        ordered pair of rows of classes (f, g)."""
        mask = self._want_mask("group_distances", want)
        arr = self._class_array("group_distances", cls, (nclass,), "a class or their number")
        out = C.POINTER(PairCounts)()
        self._check(self.L.sbl_group_distances(self.h, mask, arr, int(nclass), C.byref(out)), "sbl_group_distances")
        n = int(nclass)
        return _view(C.cast(out, C.c_void_p).value, n * n * 4, np.dtype("<u8")).reshape(n, n, 4)

    def group_distances_times(self) -> Tuple[float, float]:
        """(kernel ms, device-to-host copy ms of the matrix) of the last group_distances call, from event pairs."""
        return self._times("sbl_group_distances_times")

    def group_concat(self, cls: Sequence[int], nclass: int, headers: Sequence[bytes], mode: int, width: int = 80, want: Optional[Sequence[bool]] = None):
        """The concatenation of the groups of the LAST align_groups / align_block_groups call (csrc/group_concat.hip; defined in
        include/sibelia_amd.h), made from the rows that call left on the device.  cls: one class below nclass per instance
        of that call, flat, in group order; headers: one byte string per class, written as it is ('>' and line feed included); mode:
        CONCAT_ALL or CONCAT_VARIABLE; want: one flag per group (None: all).
        -> (text, [(group, first, ncols)], [(group, col, before)]), all copies."""
        mask = self._want_mask("group_concat", want)
        arr = self._class_array("group_concat", cls, (nclass, mode, width), "a class, their number, the mode or the width")
        if len(headers) != int(nclass):
            raise ValueError("group_concat: %d headers for %d classes" % (len(headers), int(nclass)))
        first = [0]
        for h in headers:
            first.append(first[-1] + len(h))
        parts, sites, text = C.POINTER(ConcatPart)(), C.POINTER(ConcatSite)(), C.c_void_p()
        nparts, nsites, ln = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.L.sbl_group_concat(self.h, mask, arr, int(nclass), int(mode), int(width), b"".join(headers) + b"\0", (C.c_uint64 * len(first))(*first),
                                            C.byref(parts), C.byref(nparts), C.byref(sites), C.byref(nsites), C.byref(text), C.byref(ln)), "sbl_group_concat")
        p = _view(C.cast(parts, C.c_void_p).value, nparts.value * 3, np.dtype("<u8")).reshape(-1, 3)
        s = _view(C.cast(sites, C.c_void_p).value, nsites.value * 3, np.dtype("<u8")).reshape(-1, 3)
        return (C.string_at(text.value, ln.value) if ln.value else b"", [tuple(x) for x in p.tolist()], [tuple(x) for x in s.tolist()])

    def group_concat_times(self) -> Tuple[float, float]:
        """(kernel ms, device-to-host copy ms of the text) of the last group_concat call, from event pairs."""
        return self._times("sbl_group_concat_times")

    def group_bootstrap(self, cls: Sequence[int], nclass: int, replicates: int, seed: int, draws: int = 0, want: Optional[Sequence[bool]] = None):
        """The bootstrap pair counts of the groups of the LAST align_groups / align_block_groups call (csrc/group_boot.hip; defined in
        include/sibelia_amd.h) over the variable columns of group_concat's mode CONCAT_VARIABLE, counted on the rows that
        call left on the device.  cls, nclass, want: as for group_concat; replicates: 0 .. 100000; seed: 64 bits; draws: draws per
        replicate, 0 for as many as there are sites.
        -> (uint64 array of shape (replicates + 1, nclass, nclass), a copy: [0] the sites in which two classes differ, [r] the draws of
        replicate r in which they do; C, the number of sites; K, the number of columns in which every row holds one of A C G T)."""
        mask = self._want_mask("group_bootstrap", want)
        arr = self._class_array("group_bootstrap", cls, (nclass, replicates, draws), "a class, their number, the replicates or the draws")
        if not 0 <= int(seed) <= 2 ** 64 - 1:
            raise SibeliaError("sbl_group_bootstrap: bad argument (the seed outside 64 bits)")
        out, nsites, nclean = C.POINTER(C.c_uint64)(), C.c_uint64(), C.c_uint64()
        self._check(self.L.sbl_group_bootstrap(self.h, mask, arr, int(nclass), int(replicates), int(seed), int(draws), C.byref(out), C.byref(nsites), C.byref(nclean)),
                    "sbl_group_bootstrap")
        n, b = int(nclass), int(replicates) + 1
        self._boot_nclass, self._boot_sites = n, nsites.value
        return _view(C.cast(out, C.c_void_p).value, b * n * n, np.dtype("<u8")).reshape(b, n, n), nsites.value, nclean.value

    def group_bootstrap_times(self) -> Tuple[float, float]:
        """(kernel ms of all phases, device-to-host copy ms of the counts) of the last group_bootstrap call, from event pairs."""
        return self._times("sbl_group_bootstrap_times")

    def group_bootstrap_pairs(self) -> np.ndarray:
        """The clean columns per pair of classes of the last group_bootstrap call (include/sibelia_amd.h): [f, g] the
        columns of the used groups that hold both f and g in which every present row holds one of A C G T; without set_partial every
        cell is that call's K.  -> uint64 array of shape (nclass, nclass), a copy.  Refused before any group_bootstrap call."""
        out = C.POINTER(C.c_uint64)()
        self._check(self.L.sbl_group_bootstrap_pairs(self.h, C.byref(out)), "sbl_group_bootstrap_pairs")
        n = self._boot_nclass
        return _view(C.cast(out, C.c_void_p).value, n * n, np.dtype("<u8")).reshape(n, n)

    def nj_batch(self, D):
        """The neighbour-joining trees of a batch of distance matrices (csrc/tree_nj.hip; defined in include/sibelia_amd.h, DESIGN.md
        0.13), one workgroup per matrix: bit for bit the trees of tree.neighbour_joining.  D: array of shape (ntrees, n, n), 3 <= n <= 64,
        finite, every matrix symmetric with a zero diagonal.  Needs no groups call and leaves what the group_* calls own alone.
        -> (structured array of shape (ntrees, 2n - 3) with parent, child, length: the edges in the order of Tree.edges;
        uint64 array of shape (ntrees, n - 3): per join the leaves below the new node as a bit mask, complemented where it holds file 0,
        the convention of tree.bipartitions).  Both are copies."""
        D = np.ascontiguousarray(D, dtype=np.float64)
        if D.ndim != 3 or D.shape[1] != D.shape[2]:
            raise SibeliaError("sbl_nj_batch: bad argument (the matrices must have the shape (trees, files, files))")
        ntrees, n = int(D.shape[0]), int(D.shape[1])
        if ntrees > 2 ** 32 - 1:
            raise SibeliaError("sbl_nj_batch: bad argument (the number of matrices outside 32 bits)")
        edges, splits = C.POINTER(NjEdge)(), C.POINTER(C.c_uint64)()
        self._check(self.L.sbl_nj_batch(self.h, D.ctypes.data_as(C.POINTER(C.c_double)) if D.size else None, n, ntrees, C.byref(edges), C.byref(splits)), "sbl_nj_batch")
        ne, ns = 2 * n - 3, n - 3
        return (_view(C.cast(edges, C.c_void_p).value, ntrees * ne, NJ_EDGE_DTYPE).reshape(ntrees, ne),
                _view(C.cast(splits, C.c_void_p).value, ntrees * ns, np.dtype("<u8")).reshape(ntrees, ns))

    def nj_batch_times(self) -> Tuple[float, float]:
        """(kernel ms, ms of the uploads of the matrices and the copies of the results) of the last nj_batch call, from event pairs."""
        return self._times("sbl_nj_batch_times")

    def group_parsimony(self, edges):
        """Fitch parsimony of the sites of the LAST group_bootstrap call on a tree (csrc/group_parsimony.hip; defined in
        include/sibelia_amd.h), read from the packed sites that call left on the device.  edges: the 2 n - 3 edges of an
        unrooted binary tree over leaves 0 .. n - 1 (that call's classes) and internal nodes n .. 2 n - 3: a structured array with parent
        and child (NJ_EDGE_DTYPE, a row of nj_batch) or a sequence of (node, node[, length]); lengths are ignored, 3 <= n <= 64.
        -> (uint64 array (2 n - 3, 4, 4): per edge the changes [from, to], from on the side of leaf 0, bases coded A C T G = 0 1 2 3;
        uint8 array (C,): the steps of every site; uint8 array (C,): the least steps its bases allow; structured array
        (PARSIMONY_CHANGE_DTYPE: site, edge, from, to) of all changes in ascending (site, edge)).  All are copies."""
        if isinstance(edges, np.ndarray) and edges.dtype.names:
            pairs = list(zip(edges["parent"].tolist(), edges["child"].tolist()))
        else:
            pairs = [(e[0], e[1]) for e in edges]
        if (len(pairs) + 3) % 2 or any(not 0 <= int(x) <= 2 ** 32 - 1 for e in pairs for x in e):
            raise SibeliaError("sbl_group_parsimony: bad argument (a tree of n leaves has 2 n - 3 edges between nodes of 32 bits)")
        n = (len(pairs) + 3) // 2
        arr = (NjEdge * max(1, len(pairs)))(*[NjEdge(int(u), int(v), 0.0) for u, v in pairs])
        counts, steps, least, changes = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint8)(), C.POINTER(ParsimonyChange)()
        nchanges = C.c_uint64()
        self._check(self.L.sbl_group_parsimony(self.h, arr, n, C.byref(counts), C.byref(steps), C.byref(least), C.byref(changes), C.byref(nchanges)), "sbl_group_parsimony")
        nsites = self._boot_sites                                                # the sites of the last successful group_bootstrap call
        return (_view(C.cast(counts, C.c_void_p).value, (2 * n - 3) * 16, np.dtype("<u8")).reshape(2 * n - 3, 4, 4),
                _view(C.cast(steps, C.c_void_p).value, nsites, np.dtype("u1")), _view(C.cast(least, C.c_void_p).value, nsites, np.dtype("u1")),
                _view(C.cast(changes, C.c_void_p).value, nchanges.value, PARSIMONY_CHANGE_DTYPE))

    def group_parsimony_times(self) -> Tuple[float, float]:
        """(kernel ms of the two passes and the scan, device-to-host copy ms of the four arrays) of the last group_parsimony call."""
        return self._times("sbl_group_parsimony_times")

    def set_partial(self, on) -> None:
        """True: every later group_concat / group_bootstrap call of this finder uses the groups that hold every class AT MOST once (the
        soft core): an absent class's row is gaps, columns are judged on the present rows, pairs are counted where both are present.
        False (the default): as without the setting.  Anything but 0 / 1 is refused and the value stays as it was."""
        if not 0 <= int(on) <= 2 ** 32 - 1:
            raise SibeliaError("sbl_group_set_partial: bad argument (the partial groups setting is 0 or 1)")
        self._check(self.L.sbl_group_set_partial(self.h, int(on)), "sbl_group_set_partial")

    @property
    def partial(self) -> int:
        v = C.c_uint32()
        self._check(self.L.sbl_group_get_partial(self.h, C.byref(v)), "sbl_group_get_partial")
        return v.value

    def group_mask(self, window: int, max_diff: int, want: Optional[Sequence[bool]] = None):
        """The SNP-density mask of the groups of the LAST align_groups / align_block_groups call (csrc/group_mask.hip; defined in
        include/sibelia_amd.h): per member row the maximal intervals in which more than max_diff differences from the
        centre row lie within `window` consecutive centre bases.  The rows with those intervals replaced by N stay on the device, for
        group_variants / group_distances / group_concat under set_masked(True).  want: one flag per group (None: all).
        -> [(group, row, first, last, before_first, before_last, ndiff)] in ascending (group, row, first), a copy."""
        mask = self._want_mask("group_mask", want)
        if any(not 0 <= int(v) <= 2 ** 32 - 1 for v in (window, max_diff)):
            raise SibeliaError("sbl_group_mask: bad argument (the window or the number of differences outside 32 bits)")
        iv, n = C.POINTER(MaskInterval)(), C.c_uint64()
        self._check(self.L.sbl_group_mask(self.h, mask, int(window), int(max_diff), C.byref(iv), C.byref(n)), "sbl_group_mask")
        v = _view(C.cast(iv, C.c_void_p).value, n.value * 7, np.dtype("<u8")).reshape(-1, 7)
        return [tuple(x) for x in v.tolist()]

    def group_mask_times(self) -> Tuple[float, float]:
        """(kernel ms, device-to-host copy ms of the intervals) of the last group_mask call, from event pairs."""
        return self._times("sbl_group_mask_times")

    def set_masked(self, on) -> None:
        """True: every later group_variants / group_distances / group_concat call of this finder reads the masked rows of group_mask
        instead of the rows, and is refused while no mask is valid.  False (the default): as without the setting.  Anything but 0 / 1 is
        refused and the value stays as it was."""
        if not 0 <= int(on) <= 2 ** 32 - 1:
            raise SibeliaError("sbl_group_set_masked: bad argument (the masked rows setting is 0 or 1)")
        self._check(self.L.sbl_group_set_masked(self.h, int(on)), "sbl_group_set_masked")

    @property
    def masked(self) -> int:
        v = C.c_uint32()
        self._check(self.L.sbl_group_get_masked(self.h, C.byref(v)), "sbl_group_get_masked")
        return v.value

    def align_stats(self) -> dict:
        """Counters of the last align_pairs / align_unique_blocks / align_groups / align_block_groups: pairs, skipped, passes, launches,
        cells, kernel_ms, spell_ms."""
        s = AlignStats()
        self._check(self.L.sbl_align_stats(self.h, C.byref(s)), "sbl_align_stats")
        return {f: getattr(s, f) for f, _ in s._fields_}

    def set_gap_open(self, n: int) -> None:
        """The cost of opening a gap run in every later align_* call of this finder (include/sibelia_amd.h): a run of L gap
        columns costs n + 75 L.  0 (the default) is the linear gap cost; above 100000 is refused and the value stays as it was."""
        if not 0 <= int(n) <= 2 ** 32 - 1:
            raise SibeliaError("sbl_align_set_gap_open: bad argument (a gap opening cost outside 0 .. 100000)")
        self._check(self.L.sbl_align_set_gap_open(self.h, int(n)), "sbl_align_set_gap_open")

    @property
    def gap_open(self) -> int:
        v = C.c_uint32()
        self._check(self.L.sbl_align_get_gap_open(self.h, C.byref(v)), "sbl_align_get_gap_open")
        return v.value

    def set_wide(self, on) -> None:
        """Bands beyond the LDS in every later align_* call of this finder (include/sibelia_amd.h): a pair whose band has
        more offsets than the widest LDS class holds runs in the global band class instead of being skipped.  False (the default): as
        without the setting.  Anything but 0 / 1 is refused and the value stays as it was."""
        if not 0 <= int(on) <= 2 ** 32 - 1:
            raise SibeliaError("sbl_align_set_wide: bad argument (the wide band setting is 0 or 1)")
        self._check(self.L.sbl_align_set_wide(self.h, int(on)), "sbl_align_set_wide")

    @property
    def wide(self) -> int:
        v = C.c_uint32()
        self._check(self.L.sbl_align_get_wide(self.h, C.byref(v)), "sbl_align_get_wide")
        return v.value

    def align_wide_stats(self) -> dict:
        """What the global band class did in the last align_* call: pairs (that ran at least one pass in it), passes, launches, cells,
        kernel_ms.  All zero with the setting off; align_stats() counts every class, this one included."""
        s = AlignWideStats()
        self._check(self.L.sbl_align_wide_stats(self.h, C.byref(s)), "sbl_align_wide_stats")
        return {f: getattr(s, f) for f, _ in s._fields_}

    def uncovered_calls(self, lists: Sequence[np.ndarray], min_block_size: int, n_reference_chr: int) -> np.ndarray:
        """What C-Sibelia.py calls from the regions no block covers (reference src/csibelia/C-Sibelia.py:373-427):
        `lists` are the block lists of the stages in order, the last one the final list; records 0 .. n_reference_chr - 1 are the
        reference set.  -> CALL_DTYPE records (kind CALL_DELETION / CALL_INSERTION / CALL_UNMAPPED, chr, start, end, ref_chr, pos),
        0-based half-open, in record order and ascending start.  Interval bookkeeping on the host (csrc/uncovered.hip)."""
        arrs = [np.ascontiguousarray(b, dtype=formats.BLOCK_DTYPE) for b in lists]
        first = np.cumsum([0] + [len(a) for a in arrs], dtype=np.uint64)
        flat = np.concatenate(arrs + [np.zeros(1, dtype=formats.BLOCK_DTYPE)])      # never empty: the library wants an address
        calls, n = C.c_void_p(), C.c_uint64()
        self._check(self.L.sbl_uncovered_calls(self.h, len(arrs), first.ctypes.data_as(C.POINTER(C.c_uint64)), flat.ctypes.data, min_block_size,
                                               n_reference_chr, C.byref(calls), C.byref(n)), "sbl_uncovered_calls")
        return _view(calls.value, n.value, CALL_DTYPE)

    def spell_text(self, pieces: np.ndarray, literals: bytes = b"") -> bytes:
        """The concatenation of `pieces` (PIECE_DTYPE, e.g. formats.TextPieces.pieces()): ranges of `literals` as they are, forward ranges
        of the original records upper-cased, wrapped into lines of `width` bases where width > 0.  Spelled by k_spell_text
        (csrc/spell_text.hip) from the records on the device."""
        arr = np.ascontiguousarray(pieces, dtype=PIECE_DTYPE)
        hold = C.create_string_buffer(PIECE_DTYPE.itemsize)
        t, ln = C.c_void_p(), C.c_uint64()
        self._check(self.L.sbl_spell_text(self.h, len(arr), arr.ctypes.data if len(arr) else C.addressof(hold), bytes(literals), len(literals),
                                          C.byref(t), C.byref(ln)), "sbl_spell_text")
        return C.string_at(t, ln.value) if ln.value else b""

    def spell_text_times(self) -> Tuple[float, float]:
        """(kernel ms, device-to-host copy ms) of the last spell_text call, from event pairs."""
        return self._times("sbl_spell_text_times")

    def _block_report(self, fn, what, blocks, names) -> bytes:
        nm = self._names_array(what, names)
        b, n = None, 0
        if blocks is not None:
            arr = np.ascontiguousarray(blocks, dtype=formats.BLOCK_DTYPE)
            n = len(arr)
            # (blocks == NULL selects the context's list: an explicit empty list still needs an address)
            hold = C.create_string_buffer(formats.BLOCK_DTYPE.itemsize)
            b = arr.ctypes.data if n else C.addressof(hold)
        t, ln = C.c_void_p(), C.c_uint64()
        self._check(fn(self.h, b, n, nm, C.byref(t), C.byref(ln)), what)
        return C.string_at(t, ln.value) if ln.value else b""

    def blocks_sequences(self, blocks: Optional[np.ndarray] = None, names: Optional[Sequence[str]] = None) -> bytes:
        """OutputGenerator::ListBlocksSequences (reference src/outputgenerator.cpp:287-318): the text of blocks_sequences.fasta for
        `blocks` (None: the blocks of the last GenerateSyntenyBlocks / postprocess), spelled by k_spell_text (csrc/spell_text.hip) from
        the original records on the device."""
        return self._block_report(self.L.sbl_blocks_sequences, "sbl_blocks_sequences", blocks, names)

    def blocks_sequences_times(self) -> Tuple[float, float]:
        """(kernel ms, device-to-host copy ms) of the last blocks_sequences call, from event pairs."""
        return self._times("sbl_blocks_sequences_times")

    def blocks_gff(self, blocks: Optional[np.ndarray] = None, names: Optional[Sequence[str]] = None) -> bytes:
        """OutputGenerator::ListBlocksIndicesGFF (reference src/outputgenerator.cpp:598-631): the text of blocks_coords.gff."""
        return self._block_report(self.L.sbl_blocks_gff, "sbl_blocks_gff", blocks, names)

    def blocks_coords(self, blocks: Optional[np.ndarray] = None, names: Optional[Sequence[str]] = None) -> bytes:
        """OutputGenerator::ListBlocksIndices (reference src/outputgenerator.cpp:227-233): the text of blocks_coords.txt for any list."""
        return self._block_report(self.L.sbl_blocks_coords, "sbl_blocks_coords", blocks, names)

    def serialize_graph(self, k: int) -> bytes:
        """BlockFinder::SerializeGraph (reference src/blockfinder.h:41): DOT text of the uncondensed graph."""
        t, n = C.c_void_p(), C.c_uint64()
        self._check(self.L.sbl_serialize_graph(self.h, k, C.byref(t), C.byref(n)), "sbl_serialize_graph")
        return C.string_at(t, n.value)

    def kmer_hashes(self, k: int) -> np.ndarray:
        """H0: hashes of the reference's hashing.h for every k-mer, strand 0 then 1, chromosomes ascending, walk order."""
        v, n = C.c_void_p(), C.c_uint64()
        self._check(self.L.sbl_kmer_hashes(self.h, k, C.byref(v), C.byref(n)), "sbl_kmer_hashes")
        return _view(v.value, n.value, np.dtype("<u8"))

    def stats(self) -> dict:
        s = StageStats()
        self.L.sbl_last_stats(self.h, C.byref(s))
        return s.as_dict()

    def save_state(self) -> None:
        self._check(self.L.sbl_save_state(self.h), "sbl_save_state")

    def restore_state(self) -> None:
        self._check(self.L.sbl_restore_state(self.h), "sbl_restore_state")

    def set_tempfile_mode(self, on: bool = True) -> None:
        """BlockFinder(chrList, tempDir) of the reference: keep the rand() stream in step with its temp-file names (include/sibelia_amd.h)."""
        self.L.sbl_set_tempfile_mode.argtypes = [C.c_void_p, C.c_int]
        self._check(self.L.sbl_set_tempfile_mode(self.h, int(on)), "sbl_set_tempfile_mode")

    def rand_advance(self, n: int) -> None:
        self.L.sbl_rand_advance.argtypes = [C.c_void_p, C.c_uint64]
        self._check(self.L.sbl_rand_advance(self.h, int(n)), "sbl_rand_advance")

    def set_window(self, w: int) -> None:
        self.L.sbl_set_window(self.h, w)

    # ---- multi-GPU: hash-prefix sharded enumeration (include/sibelia_amd.h, csrc/shard.hip) ----
    def attach_rccl(self, rank: int, nranks: int, unique_id: bytes) -> None:
        """Collective over all ranks; unique_id = comm_unique_id() of rank 0, distributed by the host."""
        buf = C.create_string_buffer(bytes(unique_id), COMM_ID_BYTES)
        self._check(self.L.sbl_comm_attach_rccl(self.h, rank, nranks, buf), "sbl_comm_attach_rccl")

    def attach_local(self, group: "LocalGroup", rank: int) -> None:
        self._group = group                         # keep the group alive as long as the context uses it
        self._check(self.L.sbl_comm_attach_local(self.h, group.h, rank), "sbl_comm_attach_local")

    def detach(self) -> None:
        self._check(self.L.sbl_comm_detach(self.h), "sbl_comm_detach")
        self._group = None


COMM_ID_BYTES = 128


def shard_layout(nranks: int, rank: int, bits: int, ntiles: int) -> Tuple[np.ndarray, Tuple[int, int]]:
    """Device-free layout arithmetic of the sharded k-mer table (csrc/shard.hip uses the same entry point): first bucket of
    every owner (nranks + 1 values; owner(b) = (b * nranks) >> bits) and the tile range this rank scans."""
    L = load_library()
    fb = (C.c_uint32 * (nranks + 1))()
    tr = (C.c_uint64 * 2)()
    L.sbl_shard_layout.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]
    rc = L.sbl_shard_layout(nranks, rank, bits, ntiles, fb, tr)
    if rc:
        raise SibeliaError("sbl_shard_layout: " + L.sbl_strerror(rc).decode())
    return np.array(fb, dtype=np.uint32), (int(tr[0]), int(tr[1]))


def shard_exchange_plan(nranks: int, rank: int, count: np.ndarray, send_at: np.ndarray, record_bytes: int = 8):
    """Byte counts / offsets of the one all-to-all: count[p, q] = records rank p holds for owner q (all-gathered), send_at = where
    the owners' ranges start in this rank's partitioned arrays.  Returns (sbytes, soff, rbytes, roff, nrecv)."""
    L = load_library()
    cnt = np.ascontiguousarray(count, dtype=np.uint64).reshape(nranks, nranks)
    sa = np.ascontiguousarray(send_at, dtype=np.uint32)
    out = [np.zeros(nranks, dtype=np.uint64) for _ in range(4)]
    nrecv = C.c_uint64()
    L.sbl_shard_exchange_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_void_p] * 4 + [C.c_void_p]
    rc = L.sbl_shard_exchange_plan(nranks, rank, cnt.ctypes.data, sa.ctypes.data, record_bytes, *[o.ctypes.data for o in out], C.byref(nrecv))
    if rc:
        raise SibeliaError("sbl_shard_exchange_plan: " + L.sbl_strerror(rc).decode())
    return out[0], out[1], out[2], out[3], int(nrecv.value)


def longk_slices(nranks: int, np_: int) -> np.ndarray:
    """Position slices of the sharded rank doubling (csrc/longk.hip): first[r] = np * r / nranks, nranks + 1 values."""
    L = load_library()
    out = np.zeros(nranks + 1, dtype=np.uint64)
    L.sbl_longk_slices.argtypes = [C.c_uint32, C.c_uint64, C.c_void_p]
    if L.sbl_longk_slices(nranks, np_, out.ctypes.data):
        raise SibeliaError("sbl_longk_slices")
    return out


def longk_value_bounds(nranks: int, maxvalue: int) -> np.ndarray:
    L = load_library()
    out = np.zeros(nranks + 1, dtype=np.uint64)
    L.sbl_longk_value_bounds.argtypes = [C.c_uint32, C.c_uint64, C.c_void_p]
    if L.sbl_longk_value_bounds(nranks, maxvalue, out.ctypes.data):
        raise SibeliaError("sbl_longk_value_bounds")
    return out


def longk_owner(bounds: np.ndarray, x: int) -> int:
    L = load_library()
    b = np.ascontiguousarray(bounds, dtype=np.uint64)
    o = C.c_uint32()
    L.sbl_longk_owner.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    if L.sbl_longk_owner(len(b) - 1, b.ctypes.data, int(x), C.byref(o)):
        raise SibeliaError("sbl_longk_owner")
    return int(o.value)


def longk_halo_plan(nranks: int, rank: int, np_: int, H: int):
    """(sbytes, soff, rbytes, roff) of the halo fetch of the sharded rank doubling: 4-B ranks, offsets into the sender's slice /
    the receiver's halo."""
    L = load_library()
    out = [np.zeros(nranks, dtype=np.uint64) for _ in range(4)]
    L.sbl_longk_halo_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64] + [C.c_void_p] * 4
    if L.sbl_longk_halo_plan(nranks, rank, np_, H, *[o.ctypes.data for o in out]):
        raise SibeliaError("sbl_longk_halo_plan")
    return out


def glue_stripes(blocks: np.ndarray, nchr: int) -> np.ndarray:
    """Postprocessor::GlueStripes (reference src/postprocessor.cpp:37-154) on a block array (formats.BLOCK_DTYPE); host bookkeeping only."""
    L = load_library()
    b = np.ascontiguousarray(blocks, dtype=formats.BLOCK_DTYPE).copy()
    n = C.c_uint64(len(b))
    L.sbl_glue_stripes.restype = C.c_int
    L.sbl_glue_stripes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_uint32]
    rc = L.sbl_glue_stripes(b.ctypes.data if len(b) else None, C.byref(n), int(nchr))
    if rc:
        raise SibeliaError("sbl_glue_stripes failed: %d" % rc)
    return b[:n.value]


def comm_unique_id() -> bytes:
    L = load_library()
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = L.sbl_comm_unique_id(buf)
    if rc:
        raise SibeliaError("sbl_comm_unique_id: " + L.sbl_strerror(rc).decode())
    return buf.raw


class LocalGroup:
    """Contexts of one process, one host thread per virtual rank (tests: several ranks on one GPU)."""

    def __init__(self, nranks: int):
        self.L = load_library()
        self.n = nranks
        self.h = C.c_void_p(self.L.sbl_group_create_local(nranks))
        if not self.h:
            raise SibeliaError("sbl_group_create_local failed")

    def run(self, fns):
        """Run one callable per rank concurrently (the calls are collective) and return their results."""
        import threading
        out, err = [None] * self.n, [None] * self.n

        def body(i):
            try:
                out[i] = fns[i]()
            except BaseException as e:          # noqa: BLE001 - reported to the caller below
                err[i] = e
        th = [threading.Thread(target=body, args=(i,)) for i in range(self.n)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        for e in err:
            if e is not None:
                raise e
        return out

    def __del__(self):
        try:
            if self.h:
                self.L.sbl_group_destroy(self.h)
                self.h = None
        except Exception:
            pass
