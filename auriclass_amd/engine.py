"""ctypes binding of libmhx.so (include/mhx.h): the GPU engine that stands where AuriClass
shells out to `mash` (/root/reference/auriclass/classes.py:92-104, 305-318, 576-596, 696-713).

There is no CPU fallback: if the library is missing or no HIP device is usable, the calls
raise :class:`EngineError` instead of computing anything another way.
"""
from __future__ import annotations

import ctypes
import os
import re
import subprocess
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import numpy as np

_PKG = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("MHX_LIB", _PKG / "lib" / "libmhx.so"))  # MHX_LIB: experiment builds
HEADER_PATH = _PKG.parent / "include" / "mhx.h"

MHX_OK = 0
MHX_E_NO_DEVICE = -1
MHX_E_ARG = -2
MHX_E_IO = -3
MHX_E_NO_RECORDS = -4
MHX_E_FORMAT = -5
MHX_E_HIP = -6
MHX_E_CAPACITY = -7
MHX_E_MISMATCH = -8
MHX_E_INTERNAL = -9
MERGE_BINNED, MERGE_TABLE, MERGE_HOST = 1, 2, 3   # Sketcher.merge_info()["path"]

FMT_SEQ = 0
FMT_FASTQ4 = 1


class EngineError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"mhx error {code}: {message}")
        self.code = code
        self.message = message


class NoRecordsError(EngineError):
    """mash: 'ERROR: Did not find fasta records in ...'"""


def build(force: bool = False) -> Path:
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.run(["make", "-s", "-C", str(_PKG / "csrc"), "clean"], check=True)
    subprocess.run(["make", "-s", "-j4", "-C", str(_PKG / "csrc")], check=True)
    return LIB_PATH


_lib: Optional[ctypes.CDLL] = None


def declared_symbols() -> List[str]:
    """Entry points declared in include/mhx.h."""
    text = HEADER_PATH.read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mhx_[a-z0-9_]+)\s*\(", text)))


def load() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise EngineError(MHX_E_NO_DEVICE, f"{LIB_PATH} not built (run `python -c 'import __graft_entry__ as g; g.build()'`); "
                                           "there is no CPU fallback")
    L = ctypes.CDLL(str(LIB_PATH))
    c = ctypes
    u64p, u32p = c.POINTER(c.c_uint64), c.POINTER(c.c_uint32)
    L.mhx_init.argtypes = [c.c_int]
    L.mhx_last_error.restype = c.c_char_p
    L.mhx_version.restype = c.c_char_p
    L.mhx_device_name.argtypes = [c.c_char_p, c.c_size_t]
    L.mhx_sketch_files.argtypes = [c.POINTER(c.c_char_p), c.c_int, c.c_int, c.c_uint32, c.c_int, c.c_uint32, c.c_char_p,
                                   c.c_char_p, c.c_size_t, c.POINTER(c.c_size_t), c.POINTER(c.c_double)]
    L.mhx_dist_files.argtypes = [c.c_char_p, c.c_char_p, c.c_char_p, c.c_size_t, c.POINTER(c.c_size_t)]
    L.mhx_dist_files_multi.argtypes = [c.c_char_p, c.POINTER(c.c_char_p), c.c_int, c.c_char_p, c.c_size_t, c.POINTER(c.c_size_t)]
    L.mhx_bounds.argtypes = [c.c_int, c.c_double, c.c_char_p, c.c_size_t, c.POINTER(c.c_size_t)]
    L.mhx_fasta_total_bases.argtypes = [c.c_char_p, u64p]
    L.mhx_sniff_fastq.argtypes = [c.c_char_p]
    L.mhx_sniff_fasta.argtypes = [c.c_char_p]
    L.mhx_fastq_tail_complete.argtypes = [c.c_char_p, c.c_size_t]
    L.mhx_fastq_tail_complete.restype = c.c_int
    L.mhx_sketcher_create.argtypes = [c.c_int, c.c_uint32, c.c_uint32, c.c_uint64, c.POINTER(c.c_void_p)]
    L.mhx_sketcher_create_scaled.argtypes = [c.c_int, c.c_uint32, c.c_uint32, c.c_uint64, c.c_uint32, c.POINTER(c.c_void_p)]
    L.mhx_sketcher_destroy.argtypes = [c.c_void_p]
    L.mhx_sketcher_destroy.restype = None
    L.mhx_sketcher_reset.argtypes = [c.c_void_p]
    L.mhx_sketcher_push_device.argtypes = [c.c_void_p, c.c_void_p, c.c_uint64, c.c_int]
    L.mhx_sketcher_push_host.argtypes = [c.c_void_p, c.c_void_p, c.c_uint64, c.c_int]
    L.mhx_sketcher_sync.argtypes = [c.c_void_p]
    L.mhx_sketcher_finish.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, u32p]
    L.mhx_sketcher_stats.argtypes = [c.c_void_p, c.c_void_p]
    L.mhx_sketcher_record_count.argtypes = [c.c_void_p, c.c_void_p]
    L.mhx_set_profiling.argtypes = [c.c_int]
    L.mhx_stream.restype = c.c_void_p
    L.mhx_sketcher_threshold.argtypes = [c.c_void_p, u64p]
    L.mhx_sketcher_export.argtypes = [c.c_void_p, c.c_uint64, c.c_void_p, c.c_void_p, c.c_uint32, u32p]
    L.mhx_merge_partials.argtypes = [c.c_void_p, c.c_void_p, c.c_uint64, c.c_uint32, c.c_uint32, c.c_void_p, c.c_void_p, u32p]
    L.mhx_merge_shard_partials.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint32, c.c_int, c.c_uint32, c.c_uint32,
                                           c.c_void_p, c.c_void_p, u32p]
    L.mhx_dist_batch.argtypes = [c.c_void_p, c.c_void_p, c.c_uint32, c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32,
                                 c.c_int, c.c_uint32, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int]
    L.mhx_last_dist_kernel_ms.restype = c.c_double
    L.mhx_last_dist_fallback_blocks.restype = c.c_int
    L.mhx_last_dist_ranges.restype = c.c_int
    L.mhx_p_value.argtypes = [c.c_uint64, c.c_uint64, c.c_uint64, c.c_int, c.c_uint64]
    L.mhx_p_value.restype = c.c_double
    L.mhx_msh_write.argtypes = [c.c_char_p, c.c_int, c.c_uint32, c.c_uint32, c.POINTER(c.c_char_p), c.POINTER(c.c_char_p),
                                u64p, c.POINTER(u64p), u32p]
    L.mhx_sketcher_export_slab.argtypes = [c.c_void_p, c.c_void_p, c.c_uint32]
    L.mhx_sketcher_export_begin.argtypes = [c.c_void_p, c.c_void_p]
    L.mhx_sketcher_export_pack.argtypes = [c.c_void_p, c.c_void_p, c.c_uint64]
    L.mhx_sketcher_export_into.argtypes = [c.c_void_p, c.c_void_p, c.c_uint64, c.c_void_p]
    L.mhx_sketcher_merge_gathered.argtypes = [c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint64, c.c_uint32, c.c_void_p, c.c_void_p, u32p, u64p]
    if hasattr(L, "mhx_sketcher_merge_info"):   # (MHX_LIB may name an experiment build older than the accessor: tools/merge_time.py A/B)
        L.mhx_sketcher_merge_info.argtypes = [c.c_void_p, c.c_void_p]
    L.mhx_sketcher_merge_slabs.argtypes = [c.c_void_p, c.c_void_p, c.c_int, c.c_uint32, c.c_uint64, c.c_void_p, c.c_uint32,
                                           c.c_void_p, c.c_void_p, u32p]
    L.mhx_gunzip_buffer.argtypes = [c.c_char_p, c.c_size_t, c.c_void_p, c.c_size_t, c.POINTER(c.c_size_t)]
    L.mhx_gunzip_buffer_mt.argtypes = [c.c_char_p, c.c_size_t, c.c_void_p, c.c_size_t, c.POINTER(c.c_size_t), c.c_int]
    L.mhx_gunzip_device.argtypes = [c.c_char_p, c.c_size_t, c.c_void_p, c.c_size_t, c.POINTER(c.c_size_t)]
    L.mhx_last_inflate_stats.argtypes = [c.c_void_p]
    if hasattr(L, "mhx_fasta_stream"):   # (MHX_LIB may name an experiment build older than the parser's test entry)
        L.mhx_fasta_stream.argtypes = [c.c_char_p, c.c_uint64, c.c_void_p, c.c_uint64, u64p, c.c_void_p, c.c_uint64, u64p, u32p]
    L.mhx_last_fastq_route.argtypes = []
    L.mhx_last_fastq_route.restype = c.c_int
    if hasattr(L, "mhx_screen_files"):   # (MHX_LIB may name an experiment build older than the screen: tools/ab.py)
        L.mhx_screen_files.argtypes = [c.c_char_p, c.POINTER(c.c_char_p), c.c_int, c.c_char_p, c.c_size_t, c.POINTER(c.c_size_t),
                                       c.POINTER(c.c_double)]
        L.mhx_screener_create.argtypes = [c.c_int, c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32, c.c_uint32, c.c_int, c.c_int,
                                          c.POINTER(c.c_void_p)]
        L.mhx_screener_destroy.argtypes = [c.c_void_p]
        L.mhx_screener_destroy.restype = None
        L.mhx_screener_reset.argtypes = [c.c_void_p]
        L.mhx_screener_push_device.argtypes = [c.c_void_p, c.c_void_p, c.c_uint64, c.c_int]
        L.mhx_screener_push_host.argtypes = [c.c_void_p, c.c_void_p, c.c_uint64, c.c_int]
        L.mhx_screener_sync.argtypes = [c.c_void_p]
        L.mhx_screener_finish.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.POINTER(c.c_double), c.c_void_p]
        L.mhx_screen_identity.argtypes = [c.c_uint64, c.c_uint64, c.c_int]
        L.mhx_screen_identity.restype = c.c_double
        L.mhx_screen_p_value.argtypes = [c.c_uint64, c.c_uint64, c.c_double, c.c_int]
        L.mhx_screen_p_value.restype = c.c_double
    if hasattr(L, "mhx_screener_finish_winner"):   # (or older than the winner-take-all form of the screen)
        L.mhx_screener_finish_winner.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.POINTER(c.c_double), c.c_void_p]
        L.mhx_screen_files_opts.argtypes = [c.c_char_p, c.POINTER(c.c_char_p), c.c_int, c.POINTER(ScreenOpts), c.c_char_p, c.c_size_t,
                                            c.POINTER(c.c_size_t), c.POINTER(c.c_double)]
    if hasattr(L, "mhx_sketch_segments"):   # (or older than the segmented sketch, `mash sketch -i`)
        L.mhx_sketch_segments.argtypes = [c.c_void_p, c.c_uint64, c.c_void_p, c.c_uint32, c.c_int, c.c_uint32, c.c_void_p, c.c_void_p,
                                          c.c_uint32, c.c_int]
        L.mhx_sketch_segments_cut.argtypes = []
        L.mhx_sketch_segments_cut.restype = c.c_uint32
        L.mhx_sketch_files_individual.argtypes = [c.POINTER(c.c_char_p), c.c_int, c.c_int, c.c_uint32, c.c_char_p, c.c_char_p,
                                                  c.c_size_t, c.POINTER(c.c_size_t), u64p]
    if hasattr(L, "mhx_dist_triangle"):   # (or older than the all-pairs call, `mash triangle`)
        L.mhx_dist_triangle.argtypes = [c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32, c.c_int, c.c_uint32, c.c_void_p, c.c_void_p,
                                        c.c_void_p, c.c_int]
        L.mhx_dist_triangle_edges.argtypes = [c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32, c.c_int, c.c_uint32, c.c_double, c.c_void_p,
                                              c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint64, u64p, c.c_int]
        L.mhx_triangle_files.argtypes = [c.POINTER(c.c_char_p), c.c_int, c.POINTER(TriangleOpts), c.c_char_p, c.c_size_t,
                                         c.POINTER(c.c_size_t)]
    if hasattr(L, "mhx_dist_cluster"):   # (or older than the clustering)
        L.mhx_dist_cluster.argtypes = [c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32, c.c_int, c.c_uint32, c.c_double, c.c_void_p, c.c_void_p,
                                       u32p, u64p, c.c_int]
        L.mhx_cluster_files.argtypes = [c.POINTER(c.c_char_p), c.c_int, c.POINTER(ClusterOpts), c.c_char_p, c.c_char_p, c.c_size_t,
                                        c.POINTER(c.c_size_t)]
    if hasattr(L, "mhx_dist_mst"):   # (or older than the single-linkage tree)
        L.mhx_dist_mst.argtypes = [c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32, c.c_int, c.c_uint32, c.c_void_p, c.c_void_p, c.c_void_p,
                                   c.c_void_p, c.c_void_p, c.c_int]
        L.mhx_mst_labels.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint32, c.c_int, c.c_double, c.c_void_p, u32p]
        L.mhx_tree_files.argtypes = [c.POINTER(c.c_char_p), c.c_int, c.POINTER(TreeOpts), c.c_char_p, c.c_size_t, c.POINTER(c.c_size_t)]
    if hasattr(L, "mhx_dist_linkage"):   # (or older than complete / average linkage)
        L.mhx_dist_linkage.argtypes = [c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32, c.c_int, c.c_uint32, c.c_int, c.c_void_p, c.c_void_p,
                                       c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int]
        L.mhx_last_linkage_rescans.restype = c.c_int
        L.mhx_linkage_labels.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint32, c.c_double, c.c_void_p]
        L.mhx_linkage_labels.restype = c.c_int64      # host only: the number of clusters, or a negative MHX_E_* code
        L.mhx_linkage_fixed_distance.argtypes = [c.c_uint32, c.c_uint32, c.c_int]
        L.mhx_linkage_fixed_distance.restype = c.c_uint64   # host only
        L.mhx_linkage_files.argtypes = [c.POINTER(c.c_char_p), c.c_int, c.POINTER(LinkageOpts), c.c_char_p, c.c_char_p, c.c_size_t,
                                        c.POINTER(c.c_size_t)]
    if hasattr(L, "mhx_dist_medoids"):   # (or older than the medoids)
        L.mhx_dist_medoids.argtypes = [c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32, c.c_int, c.c_uint32, c.c_void_p, c.c_void_p, c.c_void_p,
                                       c.c_void_p, c.c_void_p, c.c_int]
        L.mhx_dist_to.argtypes = [c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32, c.c_int, c.c_uint32, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int]
        L.mhx_last_medoid_blocks.restype = c.c_uint64
        L.mhx_cluster_reps_files.argtypes = [c.POINTER(c.c_char_p), c.c_int, c.POINTER(ClusterRepsOpts), c.c_char_p, c.c_char_p, c.c_size_t,
                                             c.POINTER(c.c_size_t)]
    if hasattr(L, "mhx_dist_nj"):   # (or older than neighbour joining)
        L.mhx_dist_nj.argtypes = [c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32, c.c_int, c.c_uint32, c.c_void_p, c.c_void_p, c.c_void_p,
                                  c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int]
        L.mhx_last_nj_clamps.restype = c.c_uint64
        L.mhx_nj_files.argtypes = [c.POINTER(c.c_char_p), c.c_int, c.c_int, c.c_int, c.c_char_p, c.c_size_t, c.POINTER(c.c_size_t)]
    if hasattr(L, "mhx_dist_nj_support"):   # (or older than the jackknife support of the neighbour-joining tree)
        L.mhx_resample_rows.argtypes = [c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32, c.c_uint32, c.c_uint64, c.c_uint32, c.c_double, c.c_void_p,
                                        c.c_void_p, u32p, c.c_int]
        L.mhx_dist_nj_support.argtypes = [c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32, c.c_int, c.c_uint32, c.c_uint32, c.c_double, c.c_uint64,
                                          c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
                                          c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int]
        L.mhx_nj_files_opts.argtypes = [c.POINTER(c.c_char_p), c.c_int, c.POINTER(NjOpts), c.c_char_p, c.c_size_t, c.POINTER(c.c_size_t)]
        # mhx_nj_split_support is host only and is called with explicit ctypes values (nj_split_support): no argtypes here
    if hasattr(L, "mhx_dist_search"):   # (or older than the reference-set search)
        L.mhx_dist_search.argtypes = [c.c_void_p, c.c_void_p, c.c_uint32, c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32, c.c_int, c.c_uint32,
                                      c.c_double, c.c_uint32, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int]
        L.mhx_search_files.argtypes = [c.c_char_p, c.POINTER(c.c_char_p), c.c_int, c.POINTER(SearchOpts), c.c_char_p, c.c_size_t,
                                       c.POINTER(c.c_size_t)]
    if hasattr(L, "mhx_dist_within"):   # (or older than the bounded neighbourhood call)
        L.mhx_dist_within.argtypes = [c.c_void_p, c.c_void_p, c.c_uint32, c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32, c.c_int, c.c_uint32,
                                      c.c_double, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint64, u64p, c.c_int]
        L.mhx_within_files.argtypes = [c.c_char_p, c.POINTER(c.c_char_p), c.c_int, c.POINTER(WithinOpts), c.c_char_p, c.c_size_t,
                                       c.POINTER(c.c_size_t)]
    if hasattr(L, "mhx_dist_support"):   # (or older than the jackknife support of search hits)
        L.mhx_dist_support.argtypes = [c.c_void_p, c.c_void_p, c.c_uint32, c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32, c.c_uint32, c.c_void_p,
                                       c.c_void_p, c.c_uint32, c.c_uint32, c.c_double, c.c_uint64, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
                                       c.c_void_p, c.c_int]
        L.mhx_search_files_support.argtypes = [c.c_char_p, c.POINTER(c.c_char_p), c.c_int, c.POINTER(SearchSupportOpts), c.c_char_p, c.c_char_p,
                                               c.c_size_t, c.POINTER(c.c_size_t)]
    if hasattr(L, "mhx_dist_contain"):   # (or older than the containment from sketches)
        L.mhx_dist_contain.argtypes = [c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32, c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32, c.c_uint32,
                                       c.c_void_p, c.c_void_p, c.c_void_p, c.c_int]
        L.mhx_contain_files.argtypes = [c.c_char_p, c.POINTER(c.c_char_p), c.c_int, c.POINTER(ContainOpts), c.c_char_p, c.c_size_t,
                                        c.POINTER(c.c_size_t)]
    if hasattr(L, "mhx_dist_contain_winner"):   # (or older than the winner-take-all containment)
        L.mhx_dist_contain_winner.argtypes = [c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32, c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32, c.c_uint32,
                                              c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int]
        L.mhx_last_contain_winner_pairs.restype = c.c_uint64
        L.mhx_contain_files_winner.argtypes = L.mhx_contain_files.argtypes
    if hasattr(L, "mhx_dist_contain_search"):   # (or older than the containment search)
        L.mhx_dist_contain_search.argtypes = [c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32, c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32, c.c_uint32,
                                              c.c_int, c.c_double, c.c_uint32, c.c_uint32, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
                                              c.c_int]
        L.mhx_contain_files_search.argtypes = [c.c_char_p, c.POINTER(c.c_char_p), c.c_int, c.POINTER(ContainSearchOpts), c.c_char_p, c.c_size_t,
                                               c.POINTER(c.c_size_t)]
    if hasattr(L, "mhx_dist_contain_within"):   # (or older than contain --all)
        L.mhx_dist_contain_within.argtypes = [c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32, c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32, c.c_uint32,
                                              c.c_int, c.c_double, c.c_uint32, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint64, u64p,
                                              c.c_int]
        L.mhx_contain_files_within.argtypes = [c.c_char_p, c.POINTER(c.c_char_p), c.c_int, c.POINTER(ContainWithinOpts), c.c_char_p, c.c_size_t,
                                               c.POINTER(c.c_size_t)]
    _lib = L
    return L


def _check(rc: int) -> None:
    if rc == MHX_OK:
        return
    msg = load().mhx_last_error().decode("utf-8", "replace")
    if rc == MHX_E_NO_RECORDS:
        raise NoRecordsError(rc, msg)
    raise EngineError(rc, msg)


_initialised = False


def init(device: Optional[int] = None) -> None:
    """Select the GPU (default: LOCAL_RANK or 0). Raises EngineError when none is usable."""
    global _initialised
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0")) if not _initialised else -1
    _check(load().mhx_init(device))
    _initialised = True


def device_name() -> str:
    init()
    buf = ctypes.create_string_buffer(256)
    _check(load().mhx_device_name(buf, len(buf)))
    return buf.value.decode()


def stream_handle() -> int:
    init()
    return load().mhx_stream() or 0


def _text_call(fn, *args, guess: int = 1 << 16) -> str:
    """The C ABI's two-call text pattern (size, then fill) with the first call already carrying a buffer: a text that
    fits it -- the 24 rows of an AuriClass `mash dist`, the bounds table -- costs ONE call (the library does the whole
    work in either call); a longer one reports its size (MHX_E_CAPACITY, `need`) and is fetched by a second call."""
    need = ctypes.c_size_t(0)
    buf = ctypes.create_string_buffer(guess)
    rc = fn(*args, buf, guess, ctypes.byref(need))
    if rc == MHX_E_CAPACITY and need.value > guess:
        buf = ctypes.create_string_buffer(need.value)
        rc = fn(*args, buf, need.value, ctypes.byref(need))
    _check(rc)
    return buf.value.decode("utf-8", "surrogateescape")   # names inside a .msh are arbitrary bytes


# --------------------------------------------------------------------------- file level
def sketch_files(paths: Sequence, k: int, s: int, out_msh, reads: bool = False, min_mult: int = 1, individual: bool = False
                 ) -> Tuple[str, float]:
    """`mash sketch [-r -m M | -i] -o OUT -k K -s S paths...` -> (stderr text, estimated genome size).
    individual: one reference per record of every file (`-i`, mhx_sketch_files_individual) instead of one per file; not
    together with reads."""
    if individual and reads:
        raise ValueError("sketch_files: individual=True (-i) cannot be combined with reads=True (-r)")
    init()
    L = load()
    arr = (ctypes.c_char_p * len(paths))(*[os.fsencode(str(p)) for p in paths])
    need = ctypes.c_size_t(0)
    est = ctypes.c_double(0.0)
    cap = 4096 + sum(len(str(p)) for p in paths) * 2 + len(str(out_msh))
    buf = ctypes.create_string_buffer(cap)
    if individual:
        rc = L.mhx_sketch_files_individual(arr, len(paths), k, s, os.fsencode(str(out_msh)), buf, cap, ctypes.byref(need), None)
    else:
        rc = L.mhx_sketch_files(arr, len(paths), k, s, int(reads), min_mult, os.fsencode(str(out_msh)), buf, cap,
                                ctypes.byref(need), ctypes.byref(est))
    if rc == MHX_E_NO_RECORDS:
        raise NoRecordsError(rc, L.mhx_last_error().decode())
    _check(rc)
    return buf.value.decode("utf-8", "surrogateescape"), est.value


def dist_files(ref_msh, qry_msh) -> str:
    """`mash dist REF QUERY` stdout."""
    init()
    return _text_call(load().mhx_dist_files, os.fsencode(str(ref_msh)), os.fsencode(str(qry_msh)))


def dist_files_multi(ref_msh, qry_paths: Sequence) -> str:
    """`mash dist REF QUERY [QUERY ...]` stdout: the rows of dist_files(ref, q) for every q, in argument order, from ONE
    call that reads and stages the reference once and compares all query sketches together.  The first buffer holds
    64 KiB per query file (25 times the 24 rows of an AuriClass reference set); a larger reference set costs the
    second, correct-but-slower call of _text_call."""
    init()
    paths = [os.fsencode(str(p)) for p in qry_paths]
    arr = (ctypes.c_char_p * len(paths))(*paths)
    return _text_call(load().mhx_dist_files_multi, os.fsencode(str(ref_msh)), arr, len(paths), guess=max(1, len(paths)) << 16)


class ScreenOpts(ctypes.Structure):
    """mhx_screen_opts of include/mhx.h"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("winner", ctypes.c_int32), ("min_identity", ctypes.c_double),
                ("max_p_value", ctypes.c_double)]


def screen_files(ref_msh, paths: Sequence, winner: bool = False, min_identity: float = -1.0, max_p_value: float = 1.0) -> Tuple[str, float]:
    """`mash screen [-w] [-i min_identity] [-v max_p_value] REF.msh paths...` -> (stdout text, estimated set size of the
    read set): one row per reference, "identity\\tshared/n\\tmedian\\tp\\tname\\tcomment".  All paths form one read set.
    winner: winner-take-all, every hash credited to the best reference that holds it (genome lengths from the reference
    file).  The defaults print every row (mash's own -i default is 0: rows with identity > 0)."""
    init()
    files = [os.fsencode(str(p)) for p in paths]
    arr = (ctypes.c_char_p * len(files))(*files)
    size = ctypes.c_double(0.0)
    if not winner and min_identity == -1.0 and max_p_value == 1.0:
        text = _text_call(lambda buf, cap, need: load().mhx_screen_files(os.fsencode(str(ref_msh)), arr, len(files), buf, cap, need,
                                                                         ctypes.byref(size)))
        return text, size.value
    opts = ScreenOpts(ctypes.sizeof(ScreenOpts), int(bool(winner)), float(min_identity), float(max_p_value))
    text = _text_call(lambda buf, cap, need: load().mhx_screen_files_opts(os.fsencode(str(ref_msh)), arr, len(files), ctypes.byref(opts),
                                                                          buf, cap, need, ctypes.byref(size)))
    return text, size.value


class TriangleOpts(ctypes.Structure):
    """mhx_triangle_opts of include/mhx.h"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("edge", ctypes.c_int32), ("comment", ctypes.c_int32), ("max_dist", ctypes.c_double),
                ("max_p_value", ctypes.c_double)]


def triangle_files(paths: Sequence, edge: bool = False, comment: bool = False, max_dist: float = 1.0, max_p_value: float = 1.0) -> str:
    """`mash triangle [-E] [-C] [-d max_dist] [-v max_p_value] paths...` stdout: the references of all sketch files are one
    set; the lower-triangle distance matrix ("\\t<n>", then a line per reference: name, or comment under `comment`, and its
    distances to the references before it), or with `edge` the list "name_i\\tname_j\\tdist\\tp\\tcommon/denom" of the pairs
    j < i with distance <= max_dist and p <= max_p_value.  A bound below 1 implies the edge list, as in Mash."""
    init()
    files = [os.fsencode(str(p)) for p in paths]
    arr = (ctypes.c_char_p * len(files))(*files)
    opts = TriangleOpts(ctypes.sizeof(TriangleOpts), int(bool(edge)), int(bool(comment)), float(max_dist), float(max_p_value))
    return _text_call(lambda buf, cap, need: load().mhx_triangle_files(arr, len(files), ctypes.byref(opts), buf, cap, need), guess=1 << 20)


class SearchOpts(ctypes.Structure):
    """mhx_search_opts of include/mhx.h"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("top", ctypes.c_uint32), ("max_dist", ctypes.c_double), ("max_p_value", ctypes.c_double)]


class SearchSupportOpts(ctypes.Structure):
    """mhx_search_support_opts of include/mhx.h"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("top", ctypes.c_uint32), ("max_dist", ctypes.c_double), ("max_p_value", ctypes.c_double),
                ("replicates", ctypes.c_uint32), ("keep", ctypes.c_double), ("seed", ctypes.c_uint64)]


def search_files(ref_msh, qry_paths: Sequence, top: int = 5, max_dist: float = 1.0, max_p_value: float = 1.0, replicates: int = 0,
                 keep: float = 0.5, seed: int = 42, clades=None) -> str:
    """For every query sketch of the files, in argument order and then file order, its `top` closest references of REF.msh
    with distance <= max_dist, best first, as `mash dist` rows "ref\\tquery\\tdist\\tp\\tcommon/denom"; a query without hits
    prints nothing.  max_p_value drops rows from the `top` already chosen and never promotes a lower-ranked pair.
    replicates = R > 0 (mhx_search_files_support): a sixth column "c/R", in how many of R jackknife replicates of the sketches
    (keep, seed) the row's reference is the best of the query's hits; with `clades` (AuriClass's clade_config.csv) two more, the
    clade of the row's reference and "g/R", the replicates whose best hit has that clade."""
    init()
    files = [os.fsencode(str(p)) for p in qry_paths]
    arr = (ctypes.c_char_p * len(files))(*files)
    if replicates != 0 or clades is not None:
        sopts = SearchSupportOpts(ctypes.sizeof(SearchSupportOpts), int(top), float(max_dist), float(max_p_value), int(replicates), float(keep), int(seed))
        table = None if clades is None else os.fsencode(str(clades))
        return _text_call(lambda buf, cap, need: load().mhx_search_files_support(os.fsencode(str(ref_msh)), arr, len(files), ctypes.byref(sopts), table,
                                                                                 buf, cap, need), guess=1 << 20)
    opts = SearchOpts(ctypes.sizeof(SearchOpts), int(top), float(max_dist), float(max_p_value))
    return _text_call(lambda buf, cap, need: load().mhx_search_files(os.fsencode(str(ref_msh)), arr, len(files), ctypes.byref(opts), buf, cap,
                                                                     need), guess=1 << 20)


class WithinOpts(ctypes.Structure):
    """mhx_within_opts of include/mhx.h"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("order", ctypes.c_uint32), ("max_dist", ctypes.c_double), ("max_p_value", ctypes.c_double)]


def within_files(ref_msh, qry_paths: Sequence, max_dist: float, max_p_value: float = 1.0, order: int = 0) -> str:
    """`mash dist -d max_dist -v max_p_value REF QUERY [QUERY ...]` stdout: for every query sketch of the files, in argument order
    and then file order, EVERY reference of REF.msh with distance <= max_dist and p <= max_p_value as a `mash dist` row
    "ref\\tquery\\tdist\\tp\\tcommon/denom" -- no cap on the hits of a query; a query without hits prints nothing.  order 0: the
    hits of a query in reference order (what mash prints); order 1: best first, the order of search_files."""
    init()
    files = [os.fsencode(str(p)) for p in qry_paths]
    arr = (ctypes.c_char_p * len(files))(*files)
    opts = WithinOpts(ctypes.sizeof(WithinOpts), int(order), float(max_dist), float(max_p_value))
    return _text_call(lambda buf, cap, need: load().mhx_within_files(os.fsencode(str(ref_msh)), arr, len(files), ctypes.byref(opts), buf, cap,
                                                                     need), guess=1 << 20)


class ContainOpts(ctypes.Structure):
    """mhx_contain_opts of include/mhx.h"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("comment", ctypes.c_int32), ("min_identity", ctypes.c_double), ("max_p_value", ctypes.c_double)]


def _count(v) -> int:
    """`top` / `min_shared` on their way into an unsigned word of the library, which refuses 0: a negative value goes in as 0 and
    is refused with it, where as it is it would wrap to a large count; one beyond 32 bits stays as large as a word gets"""
    return min(max(int(v), 0), 0xFFFFFFFF)


class ContainSearchOpts(ctypes.Structure):
    """mhx_contain_search_opts of include/mhx.h"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("comment", ctypes.c_int32), ("top", ctypes.c_uint32), ("min_shared", ctypes.c_uint32),
                ("min_identity", ctypes.c_double), ("max_p_value", ctypes.c_double)]


class ContainWithinOpts(ctypes.Structure):
    """mhx_contain_within_opts of include/mhx.h"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("comment", ctypes.c_int32), ("order", ctypes.c_uint32), ("min_identity", ctypes.c_double),
                ("min_shared", ctypes.c_uint32), ("max_p_value", ctypes.c_double)]


def contain_files(ref_msh, qry_paths: Sequence, min_identity: float = 0.0, max_p_value: float = 1.0, comment: bool = False,
                  winner: bool = False, top=None, min_shared: int = 1, all_hits: bool = False, order: int = 1) -> str:
    """Which share of each reference sketch of REF.msh every query sketch holds, from the sketches alone (mhx_contain_files):
    one row "reference\\tquery\\tidentity\\tp-value\\tshared/n_ref\\tshared/n_qry" per (query, reference), the queries in
    argument then file order, the references in file order.  The sketch size of REF.msh may differ from the queries'.
    min_identity and max_p_value drop rows; comment prints the comment fields in place of the names.
    winner: winner-take-all rows (mhx_contain_files_winner) -- every shared hash is credited to the best-ranked reference it
    was found in (ratio, then the genome length of REF.msh's length fields, then file order), and what a reference won
    stands in the place of `shared` in every column and in both filters.
    top = 1 .. 64 (mhx_contain_files_search): per query only the `top` references it holds the largest share of, ranked on the
    device (share, then `shared`, then file order), best first; min_identity and min_shared (>= 1) say what a hit is and act
    before the cut, max_p_value drops rows from the result already chosen.  Not with `winner`.  top=None: the full table.
    all_hits (mhx_contain_files_within): per query EVERY reference that is a hit by min_identity and min_shared, with no cap,
    taken out on the device as CSR; order 1: best first as with `top`, order 0: in the order of REF.msh; max_p_value drops rows.
    A query without hits prints nothing.  Not with `winner` or `top`."""
    init()
    files = [os.fsencode(str(p)) for p in qry_paths]
    arr = (ctypes.c_char_p * len(files))(*files)
    if all_hits:
        if winner or top is not None:
            raise EngineError(MHX_E_ARG, "contain: all_hits lists every hit of a pair rule: not with winner or top")
        wopts = ContainWithinOpts(ctypes.sizeof(ContainWithinOpts), int(bool(comment)), _count(order), float(min_identity), _count(min_shared),
                                  float(max_p_value))
        return _text_call(lambda buf, cap, need: load().mhx_contain_files_within(os.fsencode(str(ref_msh)), arr, len(files), ctypes.byref(wopts), buf,
                                                                                 cap, need), guess=1 << 20)
    if top is not None:
        if winner:
            raise EngineError(MHX_E_ARG, "contain: top ranks pairs, the winner-take-all form ranks per hash: not both")
        sopts = ContainSearchOpts(ctypes.sizeof(ContainSearchOpts), int(bool(comment)), _count(top), _count(min_shared), float(min_identity), float(max_p_value))
        return _text_call(lambda buf, cap, need: load().mhx_contain_files_search(os.fsencode(str(ref_msh)), arr, len(files), ctypes.byref(sopts), buf,
                                                                                 cap, need), guess=1 << 20)
    opts = ContainOpts(ctypes.sizeof(ContainOpts), int(bool(comment)), float(min_identity), float(max_p_value))
    if winner:
        return _text_call(lambda buf, cap, need: load().mhx_contain_files_winner(os.fsencode(str(ref_msh)), arr, len(files), ctypes.byref(opts),
                                                                                 buf, cap, need), guess=1 << 20)
    return _text_call(lambda buf, cap, need: load().mhx_contain_files(os.fsencode(str(ref_msh)), arr, len(files), ctypes.byref(opts), buf, cap,
                                                                      need), guess=1 << 20)


class ClusterOpts(ctypes.Structure):
    """mhx_cluster_opts of include/mhx.h"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("comment", ctypes.c_int32), ("rep", ctypes.c_int32), ("max_dist", ctypes.c_double)]


CLUSTER_REPS = {"first": 0, "longest": 1}


def cluster_files(paths: Sequence, max_dist: float, comment: bool = False, rep: str = "first", out=None) -> str:
    """Single-linkage clusters of the references of all sketch files (one set) at distance <= max_dist, a row per reference:
    "cluster\\tsize\\trepresentative\\tmember\\tdegree", clusters numbered from 1 by their lowest member, members in index
    order, names (comments under `comment`).  rep: "first" (the lowest index) or "longest" (the greatest genome length, ties
    to the lower index).  out: a path that receives the representatives, unchanged, as a sketch file."""
    if rep not in CLUSTER_REPS:
        raise ValueError("cluster_files: rep must be 'first' or 'longest'")
    init()
    files = [os.fsencode(str(p)) for p in paths]
    arr = (ctypes.c_char_p * len(files))(*files)
    opts = ClusterOpts(ctypes.sizeof(ClusterOpts), int(bool(comment)), CLUSTER_REPS[rep], float(max_dist))
    out_path = None if out is None else os.fsencode(str(out))
    return _text_call(lambda buf, cap, need: load().mhx_cluster_files(arr, len(files), ctypes.byref(opts), out_path, buf, cap, need), guess=1 << 20)


class TreeOpts(ctypes.Structure):
    """mhx_tree_opts of include/mhx.h"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("comment", ctypes.c_int32), ("newick", ctypes.c_int32)]


def tree_files(paths: Sequence, comment: bool = False, newick: bool = False) -> str:
    """The single-linkage tree of the references of all sketch files (one set), a row per merge in merge order:
    "name_i\\tname_j\\tdist\\tp\\tcommon/denom\\tclusters" -- the triangle's edge-list row of the pair and the clusters left
    after the merge; names, or comments under `comment`.  newick: the dendrogram in Newick format instead (node height = merge
    distance)."""
    init()
    files = [os.fsencode(str(p)) for p in paths]
    arr = (ctypes.c_char_p * len(files))(*files)
    opts = TreeOpts(ctypes.sizeof(TreeOpts), int(bool(comment)), int(bool(newick)))
    return _text_call(lambda buf, cap, need: load().mhx_tree_files(arr, len(files), ctypes.byref(opts), buf, cap, need), guess=1 << 20)


class LinkageOpts(ctypes.Structure):
    """mhx_linkage_opts of include/mhx.h"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("comment", ctypes.c_int32), ("linkage", ctypes.c_int32), ("mode", ctypes.c_int32),
                ("rep", ctypes.c_int32), ("max_dist", ctypes.c_double)]


LINKAGES = {"complete": 1, "average": 2}
LINKAGE_MODES = {"merges": 0, "newick": 1, "cut": 2}


def linkage_files(paths: Sequence, linkage: str, mode: str = "merges", comment: bool = False, max_dist: float = 1.0, rep: str = "first",
                  out=None) -> str:
    """Complete or average linkage of the references of all sketch files (one set).  mode "merges": a row per merge in merge
    order, "name_a\\tname_b\\tdist\\tsize\\tclusters"; "newick": the dendrogram as tree_files prints one; "cut": the clusters
    at max_dist, a row per reference "cluster\\tsize\\trepresentative\\tmember", ordered as cluster_files orders them, with rep
    and out (the representatives as a sketch file) as there."""
    if linkage not in LINKAGES:
        raise ValueError("linkage_files: linkage must be 'complete' or 'average'")
    if mode not in LINKAGE_MODES:
        raise ValueError("linkage_files: mode must be 'merges', 'newick' or 'cut'")
    if rep not in CLUSTER_REPS:
        raise ValueError("linkage_files: rep must be 'first' or 'longest'")
    init()
    files = [os.fsencode(str(p)) for p in paths]
    arr = (ctypes.c_char_p * len(files))(*files)
    opts = LinkageOpts(ctypes.sizeof(LinkageOpts), int(bool(comment)), LINKAGES[linkage], LINKAGE_MODES[mode], CLUSTER_REPS[rep], float(max_dist))
    out_path = None if out is None else os.fsencode(str(out))
    return _text_call(lambda buf, cap, need: load().mhx_linkage_files(arr, len(files), ctypes.byref(opts), out_path, buf, cap, need), guess=1 << 20)


class ClusterRepsOpts(ctypes.Structure):
    """mhx_cluster_reps_opts of include/mhx.h"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("comment", ctypes.c_int32), ("linkage", ctypes.c_int32), ("rep", ctypes.c_int32),
                ("max_dist", ctypes.c_double)]


CLUSTER_REPS_LINKAGES = {"single": 0, "complete": 1, "average": 2}
CLUSTER_REPS_REPS = {"first": 0, "longest": 1, "medoid": 2}


def cluster_reps_files(paths: Sequence, max_dist: float, linkage: str = "single", rep: str = "medoid", comment: bool = False, out=None) -> str:
    """The clusters of the references of all sketch files (one set) at max_dist -- single linkage as cluster_files, complete or
    average linkage as the cut of linkage_files -- with the distance of every member to its representative, a row per reference:
    "cluster\\tsize\\trepresentative\\tmember\\tdist\\tp\\tcommon/denom", ordered as cluster_files orders its rows; the last
    three fields are the triangle's edge-list fields of the pair (member, representative).  rep: "first", "longest" or "medoid"
    (the member with the smallest sum of distances to the others, ties to the lower index).  out as in cluster_files."""
    if linkage not in CLUSTER_REPS_LINKAGES:
        raise ValueError("cluster_reps_files: linkage must be 'single', 'complete' or 'average'")
    if rep not in CLUSTER_REPS_REPS:
        raise ValueError("cluster_reps_files: rep must be 'first', 'longest' or 'medoid'")
    init()
    files = [os.fsencode(str(p)) for p in paths]
    arr = (ctypes.c_char_p * len(files))(*files)
    opts = ClusterRepsOpts(ctypes.sizeof(ClusterRepsOpts), int(bool(comment)), CLUSTER_REPS_LINKAGES[linkage], CLUSTER_REPS_REPS[rep], float(max_dist))
    out_path = None if out is None else os.fsencode(str(out))
    return _text_call(lambda buf, cap, need: load().mhx_cluster_reps_files(arr, len(files), ctypes.byref(opts), out_path, buf, cap, need), guess=1 << 20)


class NjOpts(ctypes.Structure):
    """mhx_nj_opts of include/mhx.h"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("comment", ctypes.c_int32), ("newick", ctypes.c_int32), ("replicates", ctypes.c_uint32),
                ("keep", ctypes.c_double), ("seed", ctypes.c_uint64)]


def nj_files(paths: Sequence, comment: bool = False, newick: bool = False, replicates: int = 0, keep: float = 0.5, seed: int = 42) -> str:
    """Neighbour joining over the references of all sketch files (one set), a row per join in join order:
    "name_a\\tname_b\\tlen_a\\tlen_b\\tdist\\tnodes" -- the two nodes (a node is named by its lowest leaf; comments under
    `comment`), their branch lengths, their distance and the nodes left after the join.  newick: the unrooted tree in Newick
    format instead, its root the trifurcation the last two joins leave.
    replicates = R > 0: jackknife support (dist_nj_support; every replicate keeps the share `keep` of the hashes, chosen by
    `seed`) -- a seventh column "c/R" in the table, the label floor(100 c / R) behind the ")" of every inner node but the root in
    the Newick text."""
    init()
    files = [os.fsencode(str(p)) for p in paths]
    arr = (ctypes.c_char_p * len(files))(*files)
    if replicates > 0:
        opts = NjOpts(ctypes.sizeof(NjOpts), int(bool(comment)), int(bool(newick)), int(replicates), float(keep), int(seed))
        return _text_call(lambda buf, cap, need: load().mhx_nj_files_opts(arr, len(files), ctypes.byref(opts), buf, cap, need), guess=1 << 20)
    return _text_call(lambda buf, cap, need: load().mhx_nj_files(arr, len(files), int(bool(comment)), int(bool(newick)), buf, cap, need), guess=1 << 20)


def screen_identity(shared: int, n: int, k: int) -> float:
    return load().mhx_screen_identity(shared, n, k)


def screen_p_value(shared: int, n: int, set_size: float, k: int) -> float:
    return load().mhx_screen_p_value(shared, n, set_size, k)


def bounds(k: int, p: float) -> str:
    """`mash bounds -k K -p P` stdout (host arithmetic; needs no GPU)."""
    return _text_call(load().mhx_bounds, k, p)


def fasta_total_bases(path) -> int:
    v = ctypes.c_uint64(0)
    _check(load().mhx_fasta_total_bases(os.fsencode(str(path)), ctypes.byref(v)))
    return v.value


def fastq_tail_complete(tail: bytes) -> bool:
    """Is the last record of a 4-line FASTQ complete (its last bytes are enough)?  See mhx_fastq_tail_complete."""
    return bool(load().mhx_fastq_tail_complete(tail, len(tail)))


def sniff_fastq(path) -> bool:
    rc = load().mhx_sniff_fastq(os.fsencode(str(path)))
    if rc < 0:
        _check(rc)
    return bool(rc)


def sniff_fasta(path) -> bool:
    rc = load().mhx_sniff_fasta(os.fsencode(str(path)))
    if rc < 0:
        _check(rc)
    return bool(rc)


def p_value(common: int, len_ref: int, len_qry: int, k: int, denom: int) -> float:
    return load().mhx_p_value(common, len_ref, len_qry, k, denom)


def msh_write(path, k: int, s: int, names: Sequence[str], comments: Sequence[str], lengths: Sequence[int],
              hashes: Sequence[np.ndarray]) -> None:
    n = len(names)
    c = ctypes
    arrs = [np.ascontiguousarray(h, dtype=np.uint64) for h in hashes]
    u64p = c.POINTER(c.c_uint64)
    _check(load().mhx_msh_write(
        os.fsencode(str(path)), k, s, n,
        (c.c_char_p * n)(*[x.encode() for x in names]), (c.c_char_p * n)(*[x.encode() for x in comments]),
        (c.c_uint64 * n)(*lengths), (u64p * n)(*[a.ctypes.data_as(u64p) for a in arrs]),
        (c.c_uint32 * n)(*[len(a) for a in arrs])))


# --------------------------------------------------------------------------- buffer level
class Sketcher:
    """Device sketch accumulator (one reference)."""

    def __init__(self, k: int, s: int, min_mult: int = 1, expected_bytes: int = 0, budget_scale: int = 1):
        init()
        self.k, self.s, self.m = k, s, max(1, min_mult)
        h = ctypes.c_void_p()
        _check(load().mhx_sketcher_create_scaled(k, s, self.m, expected_bytes, budget_scale, ctypes.byref(h)))
        self._h = h
        self._keep: list = []   # owners of pushed device memory, released at the next settling call

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.mhx_sketcher_destroy(h)

    def __del__(self):
        try:                      # the module globals may already be gone at interpreter shutdown
            self.close()
        except Exception:
            pass

    def reset(self) -> None:
        _check(load().mhx_sketcher_reset(self._h))
        self._keep.clear()

    def push_device(self, ptr: int, nbytes: int, fmt: int, keep=None) -> None:
        """Feeds `nbytes` of device memory at `ptr` (asynchronous, on the engine's stream).
        LIFETIME: the bytes must stay valid AND unchanged until sync(), finish(), an export or reset() has returned --
        a synchronisation of the stream alone is not enough: FASTQ spans whose reads are longer than ~2.7 kb are read
        a second time by a repair pass that those calls start (include/mhx.h).  `keep`: any object (e.g. the torch
        tensor that owns the memory) to be referenced by this sketcher until then, so that dropping the caller's last
        reference cannot hand the memory to someone else in between."""
        _check(load().mhx_sketcher_push_device(self._h, ctypes.c_void_p(ptr), nbytes, fmt))
        if keep is not None:
            self._keep.append(keep)

    def push_host(self, data, fmt: int) -> None:
        a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        a = np.ascontiguousarray(a)
        _check(load().mhx_sketcher_push_host(self._h, a.ctypes.data, a.size, fmt))

    def sync(self) -> None:
        _check(load().mhx_sketcher_sync(self._h))
        self._keep.clear()

    def finish(self) -> Tuple[np.ndarray, np.ndarray]:
        hashes = np.zeros(self.s, dtype=np.uint64)
        counts = np.zeros(self.s, dtype=np.uint32)
        n = ctypes.c_uint32(0)
        _check(load().mhx_sketcher_finish(self._h, hashes.ctypes.data, counts.ctypes.data, ctypes.byref(n)))
        self._keep.clear()
        return hashes[:n.value].copy(), counts[:n.value].copy()

    def stats(self) -> dict:
        raw = np.zeros(8, dtype=np.uint64)
        _check(load().mhx_sketcher_stats(self._h, raw.ctypes.data))
        return {"kmers": int(raw[0]), "inserts": int(raw[1]), "lines": int(raw[2]), "flags": int(raw[3]),
                "occupied": int(raw[4]), "hash_ms": float(raw[5:6].view(np.float64)[0]), "launches": int(raw[6]),
                "threshold": int(raw[7])}

    def record_count(self) -> int:
        """FASTQ records pushed so far whose sequence line holds >= k bytes (mash's sequence count)."""
        n = ctypes.c_uint64(0)
        _check(load().mhx_sketcher_record_count(self._h, ctypes.byref(n)))
        return int(n.value)

    def threshold(self) -> int:
        v = ctypes.c_uint64(0)
        _check(load().mhx_sketcher_threshold(self._h, ctypes.byref(v)))
        return v.value

    def export_slab(self, device_ptr: int, cap: int) -> None:
        """Partial result as one device-resident int64 slab [n, T, flags, hashes[cap], counts (u32 pairs)];
        `device_ptr` must hold 3 + cap + cap // 2 int64 words (see include/mhx.h)."""
        _check(load().mhx_sketcher_export_slab(self._h, ctypes.c_void_p(device_ptr), cap))

    def export_begin(self) -> np.ndarray:
        """Sharded path, step 1: compacts this shard's partial result (every (hash, count) <= its threshold) on the
        device and returns the 8-word header [n, T, flags, #(2^64-1), occupied slots, 0, 0, 0] the ranks exchange."""
        hdr = np.zeros(8, dtype=np.uint64)
        _check(load().mhx_sketcher_export_begin(self._h, hdr.ctypes.data))
        return hdr

    def export_pack(self, dst_ptr: int, cap_entries: int) -> None:
        """Step 2: the partial result as one slab [hashes[cap_entries] | counts u32[cap_entries]] at `dst_ptr`
        (device or host memory; cap_entries + cap_entries // 2 eight-byte words)."""
        _check(load().mhx_sketcher_export_pack(self._h, ctypes.c_void_p(dst_ptr), cap_entries))

    def merge_slabs(self, slabs_ptr: int, on_device: bool, n_ranks: int, cap_entries: int, headers: np.ndarray, own_rank: int
                    ) -> Tuple[np.ndarray, np.ndarray]:
        """Step 3: adds the other ranks' gathered slabs to this sketcher's table ON THE DEVICE and extracts the sketch of
        the union (EngineError(MHX_E_CAPACITY) when the partials do not determine it).  The sketcher must be reset()
        before it is pushed to again."""
        headers = np.ascontiguousarray(headers, dtype=np.uint64).reshape(-1)
        assert headers.size == 8 * n_ranks
        hashes = np.zeros(self.s, dtype=np.uint64)
        counts = np.zeros(self.s, dtype=np.uint32)
        n = ctypes.c_uint32(0)
        _check(load().mhx_sketcher_merge_slabs(self._h, ctypes.c_void_p(slabs_ptr), int(on_device), n_ranks, cap_entries,
                                               headers.ctypes.data, own_rank, hashes.ctypes.data, counts.ctypes.data, ctypes.byref(n)))
        return hashes[:n.value].copy(), counts[:n.value].copy()

    def merge_info(self) -> dict:
        """The last merge on this sketcher: `path` that produced the answer (MERGE_BINNED, MERGE_TABLE, MERGE_HOST; 0: none),
        `flags` the binned attempt returned (None when it did not run) and its `nbins`, `region`, `table_slots`."""
        raw = np.zeros(8, dtype=np.uint64)
        if not hasattr(load(), "mhx_sketcher_merge_info"):
            raise EngineError(MHX_E_ARG, f"{LIB_PATH} is older than mhx_sketcher_merge_info")
        _check(load().mhx_sketcher_merge_info(self._h, raw.ctypes.data))
        ran = bool(raw[1])
        return {"path": int(raw[0]), "flags": int(raw[2]) if ran else None, "nbins": int(raw[3]), "region": int(raw[4]),
                "table_slots": int(raw[5])}

    def export_into(self, device_ptr: int, cap_entries: int) -> np.ndarray:
        """One-collective form of the exchange (device buffers): the partial result straight into the send slab
        [header8 | hashes[cap_entries] | counts u32[cap_entries]] at `device_ptr`; returns the header."""
        hdr = np.zeros(8, dtype=np.uint64)
        _check(load().mhx_sketcher_export_into(self._h, ctypes.c_void_p(device_ptr), cap_entries, hdr.ctypes.data))
        return hdr

    def merge_gathered(self, slabs_ptr: int, n_ranks: int, cap_entries: int, own_rank: int):
        """Merges the gathered header-carrying slabs on the device.  Returns (hashes, counts, 0), or (None, None, need)
        when some shard holds `need` > cap_entries entries: repeat export_into / all-gather with a larger capacity."""
        hashes = np.zeros(self.s, dtype=np.uint64)
        counts = np.zeros(self.s, dtype=np.uint32)
        n = ctypes.c_uint32(0)
        need = ctypes.c_uint64(0)
        rc = load().mhx_sketcher_merge_gathered(self._h, ctypes.c_void_p(slabs_ptr), n_ranks, cap_entries, own_rank,
                                                hashes.ctypes.data, counts.ctypes.data, ctypes.byref(n), ctypes.byref(need))
        if rc == MHX_E_CAPACITY and need.value:
            return None, None, int(need.value)
        _check(rc)
        return hashes[:n.value].copy(), counts[:n.value].copy(), 0

    def export(self, limit: int) -> Tuple[np.ndarray, np.ndarray]:
        cap = 1 << 16
        while True:
            hashes = np.zeros(cap, dtype=np.uint64)
            counts = np.zeros(cap, dtype=np.uint32)
            n = ctypes.c_uint32(0)
            rc = load().mhx_sketcher_export(self._h, limit, hashes.ctypes.data, counts.ctypes.data, cap, ctypes.byref(n))
            if rc == MHX_E_CAPACITY and n.value > cap:
                cap = n.value + 16
                continue
            _check(rc)
            return hashes[:n.value].copy(), counts[:n.value].copy()


class Screener:
    """Containment screen of a fixed reference set (`mash screen` at buffer level): rows is [nr, stride] uint64 with
    lens[i] valid ascending hashes in row i, as dist_batch takes them.  Push the read set as into a Sketcher, then
    finish() -> (shared[nr], median[nr], set_size, counts or None)."""

    def __init__(self, k: int, rows: np.ndarray, lens: np.ndarray, s_ref: int, with_set_size: bool = True):
        init()
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        assert rows.ndim == 2 and lens.shape == (rows.shape[0],)
        self.k, self.nr, self.stride, self.s_ref = k, rows.shape[0], rows.shape[1], s_ref
        self.lens = lens.copy()
        h = ctypes.c_void_p()
        _check(load().mhx_screener_create(k, rows.ctypes.data, lens.ctypes.data, self.nr, self.stride, s_ref, int(with_set_size), 0,
                                          ctypes.byref(h)))
        self._h = h
        self._keep: list = []

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.mhx_screener_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self) -> None:
        """Multiplicities back to zero; the table built from the references is kept."""
        _check(load().mhx_screener_reset(self._h))
        self._keep.clear()

    def push_device(self, ptr: int, nbytes: int, fmt: int, keep=None) -> None:
        """As Sketcher.push_device (same lifetime rule for the pushed bytes)."""
        _check(load().mhx_screener_push_device(self._h, ctypes.c_void_p(ptr), nbytes, fmt))
        if keep is not None:
            self._keep.append(keep)

    def push_host(self, data, fmt: int) -> None:
        a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        a = np.ascontiguousarray(a)
        _check(load().mhx_screener_push_host(self._h, a.ctypes.data, a.size, fmt))

    def sync(self) -> None:
        _check(load().mhx_screener_sync(self._h))
        self._keep.clear()

    def finish(self, with_counts: bool = False, winner: bool = False, ref_length=None):
        """winner: winner-take-all (`mash screen -w`, mhx_screener_finish_winner) -- every hash found is credited to the
        best reference that holds it; ref_length: [nr] genome lengths that break ties of the score (None: all equal)."""
        shared = np.zeros(self.nr, dtype=np.uint32)
        median = np.zeros(self.nr, dtype=np.uint32)
        counts = np.zeros((self.nr, self.stride), dtype=np.uint32) if with_counts else None
        size = ctypes.c_double(0.0)
        if winner:
            length = None
            if ref_length is not None:
                length = np.ascontiguousarray(ref_length, dtype=np.uint64)
                assert length.shape == (self.nr,)
            _check(load().mhx_screener_finish_winner(self._h, length.ctypes.data if length is not None else None, shared.ctypes.data,
                                                     median.ctypes.data, ctypes.byref(size), counts.ctypes.data if with_counts else None))
        else:
            assert ref_length is None, "ref_length is read by the winner-take-all form only"
            _check(load().mhx_screener_finish(self._h, shared.ctypes.data, median.ctypes.data, ctypes.byref(size),
                                              counts.ctypes.data if with_counts else None))
        self._keep.clear()
        return shared, median, size.value, counts


def gunzip(data: bytes, threads: int = 1, size_hint: int = 0) -> bytes:
    """Inflate an in-memory .gz (all members) with the ingest's own DEFLATE decoder (host code, no GPU);
    threads > 1: the first member is decoded by that many threads (mhx_gunzip_buffer_mt)."""
    L = load()
    need = ctypes.c_size_t(0)

    def call(buf, cap):
        if threads > 1:
            return L.mhx_gunzip_buffer_mt(data, len(data), buf, cap, ctypes.byref(need), threads)
        return L.mhx_gunzip_buffer(data, len(data), buf, cap, ctypes.byref(need))

    if size_hint:
        out = ctypes.create_string_buffer(size_hint)
        rc = call(out, size_hint)
        if rc == MHX_OK:
            return out.raw[:need.value]
        if rc != MHX_E_CAPACITY:
            raise EngineError(rc, L.mhx_last_error().decode())
    else:
        rc = call(None, 0)
        if rc:
            raise EngineError(rc, L.mhx_last_error().decode())
    out = ctypes.create_string_buffer(max(1, need.value))
    rc = call(out, need.value)
    if rc:
        raise EngineError(rc, L.mhx_last_error().decode())
    return out.raw[:need.value]


def gunzip_device(data: bytes, out=None):
    """Inflate an in-memory .gz (all members) on the GPU (mhx_gunzip_device) into a torch.uint8 tensor on the engine's
    device.  out: a contiguous uint8 CUDA tensor to inflate into (the result is a view of it), else one is allocated --
    sized from the last trailer's ISIZE, so a single member under 4 GiB is decoded once; a second call with the size the
    first one reported follows only when that guess is short.  Bytes and errors are those of gunzip(): the host decoder
    has the last word."""
    import torch

    init()
    L = load()
    data = bytes(data)
    need = ctypes.c_size_t(0)
    torch.cuda.synchronize()  # the call runs on the engine's stream
    if out is not None:
        assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous()
        _check(L.mhx_gunzip_device(data, len(data), ctypes.c_void_p(out.data_ptr()), out.numel(), ctypes.byref(need)))
        return out[:need.value]
    guess = int.from_bytes(data[-4:], "little") if len(data) >= 18 else 0
    out = torch.empty(max(1, guess), dtype=torch.uint8, device=f"cuda:{torch.cuda.current_device()}")
    rc = L.mhx_gunzip_device(data, len(data), ctypes.c_void_p(out.data_ptr()), out.numel(), ctypes.byref(need))
    if rc == MHX_E_CAPACITY:
        out = torch.empty(max(1, need.value), dtype=torch.uint8, device=out.device)
        rc = L.mhx_gunzip_device(data, len(data), ctypes.c_void_p(out.data_ptr()), out.numel(), ctypes.byref(need))
    _check(rc)
    return out[:need.value]


def inflate_stats() -> dict:
    """Counters of the last gunzip_device call."""
    v = np.zeros(8, dtype=np.uint64)
    _check(load().mhx_last_inflate_stats(v.ctypes.data))
    keys = ("members", "segments", "redone", "hops", "host_bytes", "inflated", "ms", "reserved")
    return {k: int(x) for k, x in zip(keys, v)}


FASTA_NOT_FOR_DEVICE = 1   # mhx_fasta_stream: the file-level calls hand such a file to the host record parser


def fasta_stream(data: bytes):
    """The device FASTA parser alone (mhx_fasta_stream, a test tool): (stream, seps, relaunches) -- the dense sequence
    stream as bytes, the ascending positions of the record separators in it (np.uint64) and how often the kernels ran again
    because the record list had to grow -- or None when the file is not for the device parser (it does not start with
    '>', or a line starts with '@' or '+')."""
    init()
    L = load()
    data = bytes(data)
    out = np.empty(len(data) + 1, dtype=np.uint8)          # the stream is never longer than the file
    seps = np.empty(len(data) // 2 + 1, dtype=np.uint64)   # a record takes two bytes at the least: '>' and a newline
    total, nseps, relaunches = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
    rc = L.mhx_fasta_stream(data, len(data), out.ctypes.data, out.size, ctypes.byref(total), seps.ctypes.data, seps.size,
                            ctypes.byref(nseps), ctypes.byref(relaunches))
    if rc == FASTA_NOT_FOR_DEVICE:
        return None
    _check(rc)
    return out[:total.value].tobytes(), seps[:nseps.value].copy(), relaunches.value


FASTQ_ROUTES = {0: None, 1: "device-streamed", 2: "device-whole", 3: "record-parser"}


def last_fastq_route():
    """Parser the last sketch_files(..., reads=True) call took (see mhx_last_fastq_route): "device-streamed",
    "device-whole", "record-parser", or None."""
    return FASTQ_ROUTES[load().mhx_last_fastq_route()]


def set_profiling(on: bool) -> None:
    load().mhx_set_profiling(int(on))


def merge_partials(hashes: np.ndarray, counts: np.ndarray, s: int, min_mult: int = 1) -> Tuple[np.ndarray, np.ndarray]:
    hashes = np.ascontiguousarray(hashes, dtype=np.uint64)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    oh = np.zeros(s, dtype=np.uint64)
    oc = np.zeros(s, dtype=np.uint32)
    n = ctypes.c_uint32(0)
    _check(load().mhx_merge_partials(hashes.ctypes.data, counts.ctypes.data, hashes.size, s, min_mult,
                                     oh.ctypes.data, oc.ctypes.data, ctypes.byref(n)))
    return oh[:n.value].copy(), oc[:n.value].copy()


def merge_shard_partials(hashes: Sequence[np.ndarray], counts: Sequence[np.ndarray], thresholds: Sequence[int], k: int, s: int,
                         min_mult: int = 1) -> Tuple[np.ndarray, np.ndarray]:
    """Merge of the shards' exports (one array pair and one admission threshold per shard) with the exactness
    rule of the sharded path: EngineError(MHX_E_CAPACITY) when the partials do not determine the union's sketch."""
    assert len(hashes) == len(counts) == len(thresholds) and len(thresholds) > 0
    sizes = np.array([len(h) for h in hashes], dtype=np.uint64)
    allh = np.ascontiguousarray(np.concatenate([np.asarray(h, dtype=np.uint64) for h in hashes]) if len(hashes) else np.zeros(0, np.uint64))
    allc = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.uint32) for x in counts]) if len(counts) else np.zeros(0, np.uint32))
    thr = np.array([int(x) for x in thresholds], dtype=np.uint64)
    oh = np.zeros(s, dtype=np.uint64)
    oc = np.zeros(s, dtype=np.uint32)
    n = ctypes.c_uint32(0)
    _check(load().mhx_merge_shard_partials(allh.ctypes.data, allc.ctypes.data, sizes.ctypes.data, thr.ctypes.data, len(thr), k, s,
                                           min_mult, oh.ctypes.data, oc.ctypes.data, ctypes.byref(n)))
    return oh[:n.value].copy(), oc[:n.value].copy()


def dist_batch(q: np.ndarray, q_len: np.ndarray, r: np.ndarray, r_len: np.ndarray, k: int, s: int
               ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Host arrays in, host arrays out: common, denom, dist of shape [nq, nr]."""
    init()
    q = np.ascontiguousarray(q, dtype=np.uint64)
    r = np.ascontiguousarray(r, dtype=np.uint64)
    assert q.ndim == 2 and r.ndim == 2 and q.shape[1] == r.shape[1]
    q_len = np.ascontiguousarray(q_len, dtype=np.uint32)
    r_len = np.ascontiguousarray(r_len, dtype=np.uint32)
    nq, nr, stride = q.shape[0], r.shape[0], q.shape[1]
    common = np.zeros((nq, nr), dtype=np.uint32)
    denom = np.zeros((nq, nr), dtype=np.uint32)
    dist = np.zeros((nq, nr), dtype=np.float64)
    _check(load().mhx_dist_batch(q.ctypes.data, q_len.ctypes.data, nq, r.ctypes.data, r_len.ctypes.data, nr, stride,
                                 k, s, common.ctypes.data, denom.ctypes.data, dist.ctypes.data, 0))
    return common, denom, dist


def sketch_segments_cut() -> int:
    """L of sketch_segments: segments of up to L windows are sketched together by one launch, larger ones one by one."""
    return int(load().mhx_sketch_segments_cut())


def sketch_segments(data, seg_off, k: int, s: int, stride: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """One bottom-s list per segment of a dense sequence stream (`mash sketch -i` at buffer level, mhx_sketch_segments):
    data is the MHX_FMT_SEQ stream (bytes or a uint8 array), seg_off the n_seg + 1 ascending byte offsets of the segments.
    Returns (rows [n_seg, stride] uint64, len [n_seg] uint32): row i holds the len[i] = min(s, distinct) smallest hashes of
    segment i, ascending, zero behind them -- as dist_batch and Screener take them.  stride: min(s, the largest window
    count of a segment) unless given (a smaller one raises EngineError(MHX_E_ARG))."""
    init()
    a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    a = np.ascontiguousarray(a, dtype=np.uint8)
    off = np.ascontiguousarray(seg_off, dtype=np.uint64).reshape(-1)
    n_seg = max(0, off.size - 1)
    if stride is None:
        span = np.diff(off.astype(np.int64)) if n_seg else np.zeros(0, np.int64)
        stride = int(min(s, max(0, int(span.max()) - k + 1))) if n_seg else 0
    rows = np.zeros((n_seg, stride), dtype=np.uint64)
    lens = np.zeros(n_seg, dtype=np.uint32)
    _check(load().mhx_sketch_segments(a.ctypes.data, a.size, off.ctypes.data, n_seg, k, s, rows.ctypes.data, lens.ctypes.data, stride, 0))
    return rows, lens


def sketch_segments_device(bytes_ptr: int, nbytes: int, seg_off_ptr: int, n_seg: int, k: int, s: int, rows_ptr: int, len_ptr: int,
                           stride: int) -> None:
    """Device pointers in and out (see mhx_sketch_segments for what must be readable around the stream); complete when it
    returns.  rows_ptr / len_ptr can go straight into dist_batch_device or a screener built with device pointers."""
    init()
    v = ctypes.c_void_p
    _check(load().mhx_sketch_segments(v(bytes_ptr), nbytes, v(seg_off_ptr), n_seg, k, s, v(rows_ptr), v(len_ptr), stride, 1))


def dist_batch_device(q_ptr: int, q_len_ptr: int, nq: int, r_ptr: int, r_len_ptr: int, nr: int, stride: int, k: int, s: int,
                      common_ptr: int, denom_ptr: int, dist_ptr: int) -> float:
    """Device pointers in and out; returns the kernel time in ms (HIP events on the engine stream)."""
    init()
    v = ctypes.c_void_p
    _check(load().mhx_dist_batch(v(q_ptr), v(q_len_ptr), nq, v(r_ptr), v(r_len_ptr), nr, stride, k, s,
                                 v(common_ptr), v(denom_ptr), v(dist_ptr), 1))
    return load().mhx_last_dist_kernel_ms()


def _triangle_rows(rows, lens):
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    assert rows.ndim == 2 and lens.shape == (rows.shape[0],)
    return rows, lens


def dist_triangle(rows: np.ndarray, lens: np.ndarray, k: int, s: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """All pairs j < i of ONE set of hash lists (rows [n, stride], lens [n], as dist_batch takes a matrix): packed
    (common, denom, dist) of n (n - 1) / 2 entries, pair (i, j) at i (i - 1) / 2 + j -- the lower triangle row by row."""
    init()
    rows, lens = _triangle_rows(rows, lens)
    n = rows.shape[0]
    pairs = n * (n - 1) // 2 if n > 1 else 0
    common = np.zeros(pairs, dtype=np.uint32)
    denom = np.zeros(pairs, dtype=np.uint32)
    dist = np.zeros(pairs, dtype=np.float64)
    _check(load().mhx_dist_triangle(rows.ctypes.data, lens.ctypes.data, n, rows.shape[1], k, s, common.ctypes.data, denom.ctypes.data,
                                    dist.ctypes.data, 0))
    return common, denom, dist


def dist_triangle_edges(rows: np.ndarray, lens: np.ndarray, k: int, s: int, max_dist: float, cap: Optional[int] = None):
    """The pairs j < i with distance <= max_dist as (edge_i, edge_j, common, denom, dist), ascending by (i, j); nothing of
    size n^2 is kept anywhere.  cap: room for that many edges (default 65 536); when it is too small the call is repeated
    once with the size the library reported."""
    init()
    rows, lens = _triangle_rows(rows, lens)
    n = rows.shape[0]
    cap = 1 << 16 if cap is None else int(cap)
    found = ctypes.c_uint64(0)
    for _ in range(2):
        ei, ej = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32)
        common, denom = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32)
        dist = np.zeros(cap, dtype=np.float64)
        rc = load().mhx_dist_triangle_edges(rows.ctypes.data, lens.ctypes.data, n, rows.shape[1], k, s, float(max_dist), ei.ctypes.data,
                                            ej.ctypes.data, common.ctypes.data, denom.ctypes.data, dist.ctypes.data, cap, ctypes.byref(found), 0)
        if rc != MHX_E_CAPACITY or found.value <= cap:
            break
        cap = found.value
    _check(rc)
    m = found.value
    return ei[:m].copy(), ej[:m].copy(), common[:m].copy(), denom[:m].copy(), dist[:m].copy()


def dist_triangle_device(rows_ptr: int, len_ptr: int, n: int, stride: int, k: int, s: int, common_ptr: int, denom_ptr: int,
                         dist_ptr: int) -> float:
    """Device pointers in and out (packed outputs as dist_triangle); returns the kernel time in ms."""
    init()
    v = ctypes.c_void_p
    _check(load().mhx_dist_triangle(v(rows_ptr), v(len_ptr), n, stride, k, s, v(common_ptr), v(denom_ptr), v(dist_ptr), 1))
    return load().mhx_last_dist_kernel_ms()


def dist_triangle_edges_device(rows_ptr: int, len_ptr: int, n: int, stride: int, k: int, s: int, max_dist: float, edge_i_ptr: int,
                               edge_j_ptr: int, common_ptr: int, denom_ptr: int, dist_ptr: int, cap: int) -> int:
    """Device pointers in and out: the edge list stays on the device, PREFILTERED ONLY (a pair within 1e-9 relative of the
    bound may be in it although its distance rounds above max_dist) and in the order of arrival.  Returns the number of
    edges; EngineError(MHX_E_CAPACITY) when it exceeds cap (the message names the number needed)."""
    init()
    v = ctypes.c_void_p
    found = ctypes.c_uint64(0)
    _check(load().mhx_dist_triangle_edges(v(rows_ptr), v(len_ptr), n, stride, k, s, float(max_dist), v(edge_i_ptr), v(edge_j_ptr),
                                          v(common_ptr), v(denom_ptr), v(dist_ptr), cap, ctypes.byref(found), 1))
    return int(found.value)


def dist_cluster(rows: np.ndarray, lens: np.ndarray, k: int, s: int, max_dist: float) -> Tuple[np.ndarray, np.ndarray, int, int]:
    """Single-linkage clusters of ONE set of hash lists (rows [n, stride], lens [n], as dist_triangle takes them) at distance
    <= max_dist (the host libm distance of dist_triangle): (label, degree, n_clusters, n_edges) with label[i] the lowest
    index in i's cluster and degree[i] the neighbours of i.  The device joins the pairs as it computes them: no edge list and
    nothing of size n^2 exists anywhere."""
    init()
    rows, lens = _triangle_rows(rows, lens)
    n = rows.shape[0]
    label = np.zeros(n, dtype=np.uint32)
    degree = np.zeros(n, dtype=np.uint32)
    n_clusters, n_edges = ctypes.c_uint32(0), ctypes.c_uint64(0)
    _check(load().mhx_dist_cluster(rows.ctypes.data, lens.ctypes.data, n, rows.shape[1], k, s, float(max_dist), label.ctypes.data,
                                   degree.ctypes.data, ctypes.byref(n_clusters), ctypes.byref(n_edges), 0))
    return label, degree, int(n_clusters.value), int(n_edges.value)


def dist_cluster_device(rows_ptr: int, len_ptr: int, n: int, stride: int, k: int, s: int, max_dist: float, label_ptr: int,
                        degree_ptr: int = 0) -> Tuple[int, int]:
    """Device pointers in and out (label [n] and degree [n] or 0; a sketch_segments_device result goes straight in): EXACT
    like the host form -- the bound reaches the device as a table of integers -- and the same from call to call.  Returns
    (n_clusters, n_edges); the kernel time is load().mhx_last_dist_kernel_ms()."""
    init()
    v = ctypes.c_void_p
    n_clusters, n_edges = ctypes.c_uint32(0), ctypes.c_uint64(0)
    _check(load().mhx_dist_cluster(v(rows_ptr), v(len_ptr), n, stride, k, s, float(max_dist), v(label_ptr), v(degree_ptr or None),
                                   ctypes.byref(n_clusters), ctypes.byref(n_edges), 1))
    return int(n_clusters.value), int(n_edges.value)


def dist_medoids(rows: np.ndarray, lens: np.ndarray, k: int, s: int, label) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """The medoid of every cluster of a partition of ONE set of hash lists (rows [n, stride], lens [n], as dist_triangle takes
    them; label[i] the lowest index of i's cluster, as dist_cluster, mst_labels and linkage_labels give it): (medoid, sum,
    common, denom) with sum[i] the sum of linkage_fixed_distance over the other members of i's cluster, medoid[i] the member of
    i's cluster with the smallest (sum, index), and common[i] / denom[i] the pair (i, medoid[i]).  Every value is an exact
    integer; the blocks run of the blocks scheduled are load().mhx_last_medoid_blocks() (>> 32 and & 0xFFFFFFFF)."""
    init()
    rows, lens = _triangle_rows(rows, lens)
    n = rows.shape[0]
    label = np.ascontiguousarray(label, dtype=np.uint32)
    assert label.shape == (n,)
    medoid, common, denom = (np.zeros(n, dtype=np.uint32) for _ in range(3))
    total = np.zeros(n, dtype=np.uint64)
    _check(load().mhx_dist_medoids(rows.ctypes.data, lens.ctypes.data, n, rows.shape[1], k, s, label.ctypes.data, medoid.ctypes.data, total.ctypes.data,
                                   common.ctypes.data, denom.ctypes.data, 0))
    return medoid, total, common, denom


def dist_medoids_device(rows_ptr: int, len_ptr: int, n: int, stride: int, k: int, s: int, label_ptr: int, medoid_ptr: int, sum_ptr: int = 0,
                        common_ptr: int = 0, denom_ptr: int = 0) -> int:
    """Device pointers in and out (label and medoid uint32 [n]; sum uint64 [n] or 0; common and denom uint32 [n], both or
    neither): the labels are copied to the host and checked there before anything is launched; the results equal the host
    form's bit for bit and are the same from call to call.  Returns the blocks of the triangle the call ran."""
    init()
    v = ctypes.c_void_p
    _check(load().mhx_dist_medoids(v(rows_ptr), v(len_ptr), n, stride, k, s, v(label_ptr), v(medoid_ptr), v(sum_ptr or None), v(common_ptr or None),
                                   v(denom_ptr or None), 1))
    return int(load().mhx_last_medoid_blocks() >> 32)


def dist_to(rows: np.ndarray, lens: np.ndarray, k: int, s: int, target) -> Tuple[np.ndarray, np.ndarray]:
    """(common, denom) of the pair (i, target[i]) of ONE set of hash lists for every i, by the pair rule of dist_triangle; a
    list against itself goes through the rule like any other pair."""
    init()
    rows, lens = _triangle_rows(rows, lens)
    n = rows.shape[0]
    target = np.ascontiguousarray(target, dtype=np.uint32)
    assert target.shape == (n,)
    common, denom = (np.zeros(n, dtype=np.uint32) for _ in range(2))
    _check(load().mhx_dist_to(rows.ctypes.data, lens.ctypes.data, n, rows.shape[1], k, s, target.ctypes.data, common.ctypes.data, denom.ctypes.data, 0))
    return common, denom


def dist_to_device(rows_ptr: int, len_ptr: int, n: int, stride: int, k: int, s: int, target_ptr: int, common_ptr: int, denom_ptr: int) -> float:
    """Device pointers in and out (three uint32 [n]); the targets are checked on the host first.  Returns the kernel time in ms."""
    init()
    v = ctypes.c_void_p
    _check(load().mhx_dist_to(v(rows_ptr), v(len_ptr), n, stride, k, s, v(target_ptr), v(common_ptr), v(denom_ptr), 1))
    return load().mhx_last_dist_kernel_ms()


def dist_mst(rows: np.ndarray, lens: np.ndarray, k: int, s: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """The single-linkage tree of ONE set of hash lists (rows [n, stride], lens [n], as dist_triangle takes them): the n - 1
    edges (edge_i, edge_j, common, denom, dist) of the minimum spanning tree of all pairs, edge_i > edge_j, in edge order --
    the greater Jaccard index first, compared exactly, ties by the lower min(i, j), then the lower max(i, j) -- which is the
    merge order of the dendrogram; dist is the host libm distance of dist_triangle.  mst_labels cuts it at any distance."""
    init()
    rows, lens = _triangle_rows(rows, lens)
    n = rows.shape[0]
    m = max(n - 1, 0)
    edge_i, edge_j, common, denom = (np.zeros(m, dtype=np.uint32) for _ in range(4))
    dist = np.zeros(m, dtype=np.float64)
    _check(load().mhx_dist_mst(rows.ctypes.data, lens.ctypes.data, n, rows.shape[1], k, s, edge_i.ctypes.data, edge_j.ctypes.data,
                               common.ctypes.data, denom.ctypes.data, dist.ctypes.data, 0))
    return edge_i, edge_j, common, denom, dist


def dist_mst_device(rows_ptr: int, len_ptr: int, n: int, stride: int, k: int, s: int, edge_i_ptr: int, edge_j_ptr: int, common_ptr: int,
                    denom_ptr: int, dist_ptr: int = 0) -> int:
    """Device pointers in and out (four uint32 [n - 1] and dist, double [n - 1] or 0; a sketch_segments_device result goes
    straight in): the edge SET is exact and the same from call to call, its order is that of arrival, dist is the device's
    log.  Returns the number of edges, n - 1 (0 for n <= 1); the rounds taken are load().mhx_last_mst_rounds()."""
    init()
    v = ctypes.c_void_p
    _check(load().mhx_dist_mst(v(rows_ptr), v(len_ptr), n, stride, k, s, v(edge_i_ptr), v(edge_j_ptr), v(common_ptr), v(denom_ptr),
                               v(dist_ptr or None), 1))
    return max(n - 1, 0)


def mst_labels(edge_i, edge_j, common, denom, n: int, k: int, max_dist: float) -> Tuple[np.ndarray, int]:
    """The clusters of dist_cluster at max_dist from the tree of dist_mst alone, on the host (mhx_mst_labels: no device needed):
    a union-find over the tree edges whose libm distance (the double dist_triangle gives) is <= max_dist; (label, n_clusters),
    label[i] = the lowest index of i's cluster."""
    cols = [np.ascontiguousarray(a, dtype=np.uint32) for a in (edge_i, edge_j, common, denom)]
    assert all(a.shape == (max(n - 1, 0),) for a in cols)
    label = np.zeros(n, dtype=np.uint32)
    n_clusters = ctypes.c_uint32(0)
    _check(load().mhx_mst_labels(*(a.ctypes.data for a in cols), n, k, float(max_dist), label.ctypes.data, ctypes.byref(n_clusters)))
    return label, int(n_clusters.value)


def _linkage_code(linkage) -> int:
    code = LINKAGES.get(linkage, linkage)
    if code not in (1, 2):
        raise ValueError("linkage must be 'complete' or 'average'")
    return int(code)


def dist_linkage(rows: np.ndarray, lens: np.ndarray, k: int, s: int, linkage
                 ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """Complete ("complete", 1) or average ("average", 2: UPGMA) linkage of ONE set of hash lists (rows [n, stride], lens [n], as
    dist_triangle takes them): the n - 1 merges in merge order, (merge_a, merge_b, size, num, den, dist) -- the two cluster ids
    (a cluster's id is its lowest member, merge_a > merge_b, the merged cluster keeps merge_b), the members after the merge, the
    linkage value num / den (complete: common / denom of the decisive leaf pair; average: the sum of the fixed-point distances
    over |A| |B|) and the height (complete: the host libm distance of dist_triangle; average: num / den * 2^-32).
    linkage_labels cuts the merges at any distance."""
    init()
    rows, lens = _triangle_rows(rows, lens)
    n = rows.shape[0]
    m = max(n - 1, 0)
    merge_a, merge_b, size = (np.zeros(m, dtype=np.uint32) for _ in range(3))
    num, den = (np.zeros(m, dtype=np.uint64) for _ in range(2))
    dist = np.zeros(m, dtype=np.float64)
    _check(load().mhx_dist_linkage(rows.ctypes.data, lens.ctypes.data, n, rows.shape[1], k, s, _linkage_code(linkage), merge_a.ctypes.data,
                                   merge_b.ctypes.data, size.ctypes.data, num.ctypes.data, den.ctypes.data, dist.ctypes.data, 0))
    return merge_a, merge_b, size, num, den, dist


def dist_linkage_device(rows_ptr: int, len_ptr: int, n: int, stride: int, k: int, s: int, linkage, merge_a_ptr: int, merge_b_ptr: int,
                        size_ptr: int, num_ptr: int, den_ptr: int, dist_ptr: int = 0) -> int:
    """Device pointers in and out (three uint32 [n - 1], two uint64 [n - 1] and dist, double [n - 1] or 0): the merges in merge
    order, every integer exact and the same from call to call, dist in the device's arithmetic.  Returns the number of merges,
    n - 1 (0 for n <= 1); the rows scanned again are load().mhx_last_linkage_rescans()."""
    init()
    v = ctypes.c_void_p
    _check(load().mhx_dist_linkage(v(rows_ptr), v(len_ptr), n, stride, k, s, _linkage_code(linkage), v(merge_a_ptr), v(merge_b_ptr), v(size_ptr),
                                   v(num_ptr), v(den_ptr), v(dist_ptr or None), 1))
    return max(n - 1, 0)


def linkage_labels(merge_a, merge_b, dist, n: int, max_dist: float) -> Tuple[np.ndarray, int]:
    """The clusters of the merges of dist_linkage at max_dist, on the host (mhx_linkage_labels: no device needed): the merges
    from the first one on while dist[t] <= max_dist; (label, n_clusters), label[i] = the lowest index of i's cluster."""
    a, b = (np.ascontiguousarray(x, dtype=np.uint32) for x in (merge_a, merge_b))
    d = np.ascontiguousarray(dist, dtype=np.float64)
    assert all(x.shape == (max(n - 1, 0),) for x in (a, b, d))
    label = np.zeros(n, dtype=np.uint32)
    rc = load().mhx_linkage_labels(a.ctypes.data, b.ctypes.data, d.ctypes.data, n, float(max_dist), label.ctypes.data)
    if rc < 0:
        _check(int(rc))
    return label, int(rc)


def linkage_fixed_distance(common: int, denom: int, k: int) -> int:
    """The fixed-point distance of average linkage in units of 2^-32 (mhx_linkage_fixed_distance: integers alone, no device
    needed); 2^64 - 1 for arguments outside its domain."""
    return int(load().mhx_linkage_fixed_distance(common, denom, k))


def dist_nj(rows: np.ndarray, lens: np.ndarray, k: int, s: int
            ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """Neighbour joining over ONE set of hash lists (rows [n, stride], lens [n], as dist_triangle takes them): the n - 1 joins
    in join order, (join_a, join_b, d, r_a, r_b, len_a, len_b) -- the two node ids (a node's id is its lowest leaf, join_a >
    join_b, the new node keeps join_b), their distance and their row sums in units of 2^-32 as they were before the join, and
    the two branch lengths (they may be negative).  Distances are the fixed-point distance of the average linkage and an
    update never goes below 0 (a deviation from the textbook; load().mhx_last_nj_clamps() counts how often that mattered)."""
    init()
    rows, lens = _triangle_rows(rows, lens)
    n = rows.shape[0]
    m = max(n - 1, 0)
    join_a, join_b = (np.zeros(m, dtype=np.uint32) for _ in range(2))
    d, r_a, r_b = (np.zeros(m, dtype=np.uint64) for _ in range(3))
    len_a, len_b = (np.zeros(m, dtype=np.float64) for _ in range(2))
    _check(load().mhx_dist_nj(rows.ctypes.data, lens.ctypes.data, n, rows.shape[1], k, s, join_a.ctypes.data, join_b.ctypes.data, d.ctypes.data,
                              r_a.ctypes.data, r_b.ctypes.data, len_a.ctypes.data, len_b.ctypes.data, 0))
    return join_a, join_b, d, r_a, r_b, len_a, len_b


def dist_nj_device(rows_ptr: int, len_ptr: int, n: int, stride: int, k: int, s: int, join_a_ptr: int, join_b_ptr: int, d_ptr: int, r_a_ptr: int,
                   r_b_ptr: int, len_a_ptr: int = 0, len_b_ptr: int = 0) -> int:
    """Device pointers in and out (two uint32 [n - 1], three uint64 [n - 1] and len_a, len_b, double [n - 1], both or neither 0):
    the joins in join order, the same bytes as dist_nj gives.  rows_ptr / len_ptr may be what sketch_segments_device wrote.
    Returns the number of joins, n - 1 (0 for n <= 1)."""
    init()
    v = ctypes.c_void_p
    _check(load().mhx_dist_nj(v(rows_ptr), v(len_ptr), n, stride, k, s, v(join_a_ptr), v(join_b_ptr), v(d_ptr), v(r_a_ptr), v(r_b_ptr),
                              v(len_a_ptr or None), v(len_b_ptr or None), 1))
    return max(n - 1, 0)


def resample_rows(rows: np.ndarray, lens: np.ndarray, s: int, seed: int, replicate: int, keep: float) -> Tuple[np.ndarray, np.ndarray, int]:
    """One jackknife replicate of a set of hash lists (mhx_resample_rows): every list keeps the hashes the keep function of
    include/mhx.h admits, in order, and all are cut to s_r, the smallest kept count among the full lists (len == s).
    (rows [n, stride] with zeros behind the new lengths, lens [n], s_r)."""
    init()
    rows, lens = _triangle_rows(rows, lens)
    out_rows = np.zeros_like(rows)
    out_len = np.zeros_like(lens)
    s_r = ctypes.c_uint32(0)
    _check(load().mhx_resample_rows(rows.ctypes.data, lens.ctypes.data, rows.shape[0], rows.shape[1], s, seed, replicate, float(keep),
                                    out_rows.ctypes.data, out_len.ctypes.data, ctypes.byref(s_r), 0))
    return out_rows, out_len, int(s_r.value)


def dist_nj_support(rows: np.ndarray, lens: np.ndarray, k: int, s: int, replicates: int, keep: float = 0.5, seed: int = 42):
    """Neighbour joining with jackknife support (mhx_dist_nj_support): (join_a, join_b, d, r_a, r_b, len_a, len_b) exactly as
    dist_nj gives them, then support [n - 1] -- in how many of the `replicates` trees the split of each join is found --,
    rep_join_a and rep_join_b [replicates, n - 1], the joins of every replicate, and rep_s [replicates], its sketch size."""
    init()
    rows, lens = _triangle_rows(rows, lens)
    n = rows.shape[0]
    m = max(n - 1, 0)
    join_a, join_b = (np.zeros(m, dtype=np.uint32) for _ in range(2))
    d, r_a, r_b = (np.zeros(m, dtype=np.uint64) for _ in range(3))
    len_a, len_b = (np.zeros(m, dtype=np.float64) for _ in range(2))
    support = np.zeros(m, dtype=np.uint32)
    rep_a, rep_b = (np.zeros((replicates, m), dtype=np.uint32) for _ in range(2))
    rep_s = np.zeros(replicates, dtype=np.uint32)
    _check(load().mhx_dist_nj_support(rows.ctypes.data, lens.ctypes.data, n, rows.shape[1], k, s, replicates, float(keep), seed, join_a.ctypes.data,
                                      join_b.ctypes.data, d.ctypes.data, r_a.ctypes.data, r_b.ctypes.data, len_a.ctypes.data, len_b.ctypes.data,
                                      support.ctypes.data, rep_a.ctypes.data, rep_b.ctypes.data, rep_s.ctypes.data, 0))
    return join_a, join_b, d, r_a, r_b, len_a, len_b, support, rep_a, rep_b, rep_s


def dist_nj_support_device(rows_ptr: int, len_ptr: int, n: int, stride: int, k: int, s: int, replicates: int, keep: float, seed: int, join_a_ptr: int,
                           join_b_ptr: int, d_ptr: int, r_a_ptr: int, r_b_ptr: int, len_a_ptr: int = 0, len_b_ptr: int = 0):
    """Device pointers for the rows, the lengths and the seven outputs of the main tree (as dist_nj_device takes them; what
    sketch_segments_device wrote goes straight in); the support values come back on the host: (support [n - 1], rep_join_a,
    rep_join_b [replicates, n - 1], rep_s [replicates])."""
    init()
    v = ctypes.c_void_p
    m = max(n - 1, 0)
    support = np.zeros(m, dtype=np.uint32)
    rep_a, rep_b = (np.zeros((replicates, m), dtype=np.uint32) for _ in range(2))
    rep_s = np.zeros(replicates, dtype=np.uint32)
    _check(load().mhx_dist_nj_support(v(rows_ptr), v(len_ptr), n, stride, k, s, replicates, float(keep), seed, v(join_a_ptr), v(join_b_ptr), v(d_ptr),
                                      v(r_a_ptr), v(r_b_ptr), v(len_a_ptr or None), v(len_b_ptr or None), support.ctypes.data, rep_a.ctypes.data,
                                      rep_b.ctypes.data, rep_s.ctypes.data, 1))
    return support, rep_a, rep_b, rep_s


def nj_split_support(join_a, join_b, rep_join_a, rep_join_b, n: int) -> np.ndarray:
    """support [n - 1] of the joins of a tree among the replicate trees rep_join_a / rep_join_b [replicates, n - 1], on the
    host (mhx_nj_split_support: no device needed, exact): the number of replicates that hold the split of each join; a split
    with at most one leaf on a side is in every tree."""
    m = max(n - 1, 0)
    a, b = (np.ascontiguousarray(x, dtype=np.uint32) for x in (join_a, join_b))
    ra, rb = (np.ascontiguousarray(x, dtype=np.uint32).reshape(-1, m) if m else np.zeros((0, 0), np.uint32) for x in (rep_join_a, rep_join_b))
    assert a.shape == (m,) and b.shape == (m,) and ra.shape == rb.shape
    support = np.zeros(m, dtype=np.uint32)
    v = ctypes.c_void_p
    _check(load().mhx_nj_split_support(v(a.ctypes.data), v(b.ctypes.data), v(ra.ctypes.data), v(rb.ctypes.data), ctypes.c_uint32(n),
                                       ctypes.c_uint32(ra.shape[0]), v(support.ctypes.data)))
    return support


def dist_search(q: np.ndarray, q_len: np.ndarray, r: np.ndarray, r_len: np.ndarray, k: int, s: int, top: int, max_dist: float = 1.0
                ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """For every query list its `top` (1 .. 64) closest references with distance <= max_dist, ranked on the device by the
    exact Jaccard index (ties: the lower reference index): (ref, common, denom, dist) of shape [nq, top], best first and zero
    behind n_hits [nq].  Rows and lengths as dist_batch takes them; no [nq, nr] array exists anywhere."""
    init()
    q = np.ascontiguousarray(q, dtype=np.uint64)
    r = np.ascontiguousarray(r, dtype=np.uint64)
    assert q.ndim == 2 and r.ndim == 2 and q.shape[1] == r.shape[1]
    q_len = np.ascontiguousarray(q_len, dtype=np.uint32)
    r_len = np.ascontiguousarray(r_len, dtype=np.uint32)
    nq, nr, stride = q.shape[0], r.shape[0], q.shape[1]
    cells = (nq, max(int(top), 0))
    ref, common, denom = np.zeros(cells, dtype=np.uint32), np.zeros(cells, dtype=np.uint32), np.zeros(cells, dtype=np.uint32)
    dist = np.zeros(cells, dtype=np.float64)
    n_hits = np.zeros(nq, dtype=np.uint32)
    _check(load().mhx_dist_search(q.ctypes.data, q_len.ctypes.data, nq, r.ctypes.data, r_len.ctypes.data, nr, stride, k, s, float(max_dist),
                                  int(top), ref.ctypes.data, common.ctypes.data, denom.ctypes.data, dist.ctypes.data, n_hits.ctypes.data, 0))
    return ref, common, denom, dist, n_hits


def dist_search_device(q_ptr: int, q_len_ptr: int, nq: int, r_ptr: int, r_len_ptr: int, nr: int, stride: int, k: int, s: int, top: int,
                       max_dist: float, ref_ptr: int, common_ptr: int, denom_ptr: int, dist_ptr: int, n_hits_ptr: int) -> float:
    """Device pointers in and out ([nq, top] lists and n_hits [nq]; a sketch_segments_device result goes straight in on either
    side): the lists stay on the device, PREFILTERED ONLY (see dist_triangle_edges_device) but in rank order, dist (may be 0)
    is the device's log, entries behind n_hits are unspecified.  Returns the kernel time in ms."""
    init()
    v = ctypes.c_void_p
    _check(load().mhx_dist_search(v(q_ptr), v(q_len_ptr), nq, v(r_ptr), v(r_len_ptr), nr, stride, k, s, float(max_dist), int(top), v(ref_ptr),
                                  v(common_ptr), v(denom_ptr), v(dist_ptr or None), v(n_hits_ptr), 1))
    return load().mhx_last_dist_kernel_ms()


def _within_rows(q, q_len, r, r_len):
    q = np.ascontiguousarray(q, dtype=np.uint64)
    r = np.ascontiguousarray(r, dtype=np.uint64)
    assert q.ndim == 2 and r.ndim == 2 and q.shape[1] == r.shape[1]
    return q, np.ascontiguousarray(q_len, dtype=np.uint32), r, np.ascontiguousarray(r_len, dtype=np.uint32)


def dist_within(q: np.ndarray, q_len: np.ndarray, r: np.ndarray, r_len: np.ndarray, k: int, s: int, max_dist: float, cap: Optional[int] = None
                ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """For every query list ALL references with distance <= max_dist, as CSR: (row_off [nq + 1], ref, common, denom, dist);
    the hits of query i are [row_off[i], row_off[i + 1]) of the four arrays, ascending by reference index.  Exact (the bound
    reaches the device as integers) and the same from run to run.  Rows and lengths as dist_batch takes them; no [nq, nr] array
    exists anywhere.  cap: room for that many hits (default 65 536); when it is too small the call is repeated once with
    the size the library reported."""
    init()
    q, q_len, r, r_len = _within_rows(q, q_len, r, r_len)
    nq, nr, stride = q.shape[0], r.shape[0], q.shape[1]
    cap = 1 << 16 if cap is None else int(cap)
    row_off = np.zeros(nq + 1, dtype=np.uint64)
    found = ctypes.c_uint64(0)
    for _ in range(2):
        ref, common, denom = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32)
        dist = np.zeros(cap, dtype=np.float64)
        rc = load().mhx_dist_within(q.ctypes.data, q_len.ctypes.data, nq, r.ctypes.data, r_len.ctypes.data, nr, stride, k, s, float(max_dist),
                                    row_off.ctypes.data, ref.ctypes.data, common.ctypes.data, denom.ctypes.data, dist.ctypes.data, cap,
                                    ctypes.byref(found), 0)
        if rc != MHX_E_CAPACITY or found.value <= cap:
            break
        cap = found.value
    _check(rc)
    m = found.value
    return row_off, ref[:m].copy(), common[:m].copy(), denom[:m].copy(), dist[:m].copy()


def dist_within_counts(q: np.ndarray, q_len: np.ndarray, r: np.ndarray, r_len: np.ndarray, k: int, s: int, max_dist: float) -> np.ndarray:
    """The counting form of dist_within: row_off [nq + 1] alone (row_off[nq] the number of hits), no hit is stored."""
    init()
    q, q_len, r, r_len = _within_rows(q, q_len, r, r_len)
    nq = q.shape[0]
    row_off = np.zeros(nq + 1, dtype=np.uint64)
    found = ctypes.c_uint64(0)
    _check(load().mhx_dist_within(q.ctypes.data, q_len.ctypes.data, nq, r.ctypes.data, r_len.ctypes.data, r.shape[0], q.shape[1], k, s, float(max_dist),
                                  row_off.ctypes.data, None, None, None, None, 0, ctypes.byref(found), 0))
    return row_off


def dist_within_device(q_ptr: int, q_len_ptr: int, nq: int, r_ptr: int, r_len_ptr: int, nr: int, stride: int, k: int, s: int, max_dist: float,
                       row_off_ptr: int, ref_ptr: int, common_ptr: int, denom_ptr: int, dist_ptr: int, cap: int) -> int:
    """Device pointers in and out (row_off [nq + 1] of 64-bit words, the hit arrays [cap]; a sketch_segments_device result goes
    straight in on either side): the CSR stays on the device, exact and in its final order -- the integers are those of
    dist_within bit for bit --, dist (may be 0) is the device's log.  ref_ptr == 0 with cap == 0 only counts.  Returns the
    number of hits; EngineError(MHX_E_CAPACITY) when it exceeds cap (row_off is complete then, the message names the number)."""
    init()
    v = ctypes.c_void_p
    found = ctypes.c_uint64(0)
    _check(load().mhx_dist_within(v(q_ptr), v(q_len_ptr), nq, v(r_ptr), v(r_len_ptr), nr, stride, k, s, float(max_dist), v(row_off_ptr),
                                  v(ref_ptr or None), v(common_ptr or None), v(denom_ptr or None), v(dist_ptr or None), int(cap), ctypes.byref(found), 1))
    return int(found.value)


def dist_contain(q: np.ndarray, q_len: np.ndarray, r: np.ndarray, r_len: np.ndarray, s_q: int, s_r: int
                 ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Containment of every reference list in every query list (mhx_dist_contain): (shared, n_qry, n_ref) of shape [nq, nr].
    Rows and lengths as dist_batch takes them, one stride for both sets; s_q and s_r are the sketch sizes of the two sets and
    may differ.  Within tau, the smaller of the two lists' bounds, n_ref hashes of the reference and n_qry of the query lie,
    `shared` of them in both: shared == n_ref when the query's input contains the reference's."""
    init()
    q = np.ascontiguousarray(q, dtype=np.uint64)
    r = np.ascontiguousarray(r, dtype=np.uint64)
    assert q.ndim == 2 and r.ndim == 2 and q.shape[1] == r.shape[1]
    q_len = np.ascontiguousarray(q_len, dtype=np.uint32)
    r_len = np.ascontiguousarray(r_len, dtype=np.uint32)
    nq, nr, stride = q.shape[0], r.shape[0], q.shape[1]
    shared, n_qry, n_ref = (np.zeros((nq, nr), dtype=np.uint32) for _ in range(3))
    _check(load().mhx_dist_contain(q.ctypes.data, q_len.ctypes.data, nq, int(s_q), r.ctypes.data, r_len.ctypes.data, nr, int(s_r), stride,
                                   shared.ctypes.data, n_qry.ctypes.data, n_ref.ctypes.data, 0))
    return shared, n_qry, n_ref


def dist_contain_device(q_ptr: int, q_len_ptr: int, nq: int, s_q: int, r_ptr: int, r_len_ptr: int, nr: int, s_r: int, stride: int,
                        shared_ptr: int, n_qry_ptr: int, n_ref_ptr: int) -> float:
    """Device pointers in and out ([nq, nr] each; a sketch_segments_device result goes straight in on either side): the same
    integers as dist_contain.  Lengths the host cannot see are clipped to the stride and the sketch size.  Returns the
    kernel time in ms."""
    init()
    v = ctypes.c_void_p
    _check(load().mhx_dist_contain(v(q_ptr), v(q_len_ptr), nq, int(s_q), v(r_ptr), v(r_len_ptr), nr, int(s_r), stride, v(shared_ptr), v(n_qry_ptr),
                                   v(n_ref_ptr), 1))
    return load().mhx_last_dist_kernel_ms()


def dist_contain_search(q: np.ndarray, q_len: np.ndarray, r: np.ndarray, r_len: np.ndarray, s_q: int, s_r: int, k: int, top: int,
                        min_identity: float = 0.0, min_shared: int = 1
                        ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """For every query list the `top` (1 .. 64) references it holds the largest share of (mhx_dist_contain_search), ranked on the
    device by the exact share shared / n_ref (ties: the larger `shared`, then the lower reference index): (hit_ref, hit_shared,
    hit_n_ref, hit_n_qry) of shape [nq, top], best first and zero behind n_hits [nq].  The integers of a pair are
    dist_contain's; a hit shares at least min_shared (>= 1) hashes and has identity(shared, n_ref, k) >= min_identity.  Rows
    and lengths as dist_contain takes them; no [nq, nr] array exists anywhere."""
    init()
    q = np.ascontiguousarray(q, dtype=np.uint64)
    r = np.ascontiguousarray(r, dtype=np.uint64)
    assert q.ndim == 2 and r.ndim == 2 and q.shape[1] == r.shape[1]
    q_len = np.ascontiguousarray(q_len, dtype=np.uint32)
    r_len = np.ascontiguousarray(r_len, dtype=np.uint32)
    nq, nr, stride = q.shape[0], r.shape[0], q.shape[1]
    cells = (nq, min(_count(top), 64))   # (a top the library refuses is refused before it writes)
    ref, shared, n_ref, n_qry =(np.zeros(cells, dtype=np.uint32) for _ in range(4))
    n_hits = np.zeros(nq, dtype=np.uint32)
    _check(load().mhx_dist_contain_search(q.ctypes.data, q_len.ctypes.data, nq, int(s_q), r.ctypes.data, r_len.ctypes.data, nr, int(s_r), stride, int(k),
                                          float(min_identity), _count(min_shared), _count(top), ref.ctypes.data, shared.ctypes.data, n_ref.ctypes.data,
                                          n_qry.ctypes.data, n_hits.ctypes.data, 0))
    return ref, shared, n_ref, n_qry, n_hits


def dist_contain_search_device(q_ptr: int, q_len_ptr: int, nq: int, s_q: int, r_ptr: int, r_len_ptr: int, nr: int, s_r: int, stride: int, k: int,
                               top: int, min_identity: float, min_shared: int, ref_ptr: int, shared_ptr: int, n_ref_ptr: int, n_qry_ptr: int,
                               n_hits_ptr: int) -> float:
    """Device pointers in and out ([nq, top] lists and n_hits [nq]; a sketch_segments_device result goes straight in on either
    side): the same lists as dist_contain_search, exact, entries behind n_hits unspecified.  Lengths the host cannot see are
    clipped to the stride and the sketch size.  Returns the kernel time in ms."""
    init()
    v = ctypes.c_void_p
    _check(load().mhx_dist_contain_search(v(q_ptr), v(q_len_ptr), nq, int(s_q), v(r_ptr), v(r_len_ptr), nr, int(s_r), stride, int(k), float(min_identity),
                                          _count(min_shared), _count(top), v(ref_ptr), v(shared_ptr), v(n_ref_ptr), v(n_qry_ptr), v(n_hits_ptr), 1))
    return load().mhx_last_dist_kernel_ms()


def dist_contain_within(q: np.ndarray, q_len: np.ndarray, r: np.ndarray, r_len: np.ndarray, s_q: int, s_r: int, k: int, min_identity: float = 0.0,
                        min_shared: int = 1, cap: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """For every query list ALL references it holds (mhx_dist_contain_within), as CSR: (row_off [nq + 1], ref, shared, n_ref,
    n_qry); the hits of query i are [row_off[i], row_off[i + 1]) of the four arrays, ascending by reference index.  A hit is
    dist_contain_search's: it shares at least min_shared (>= 1) hashes and has identity(shared, n_ref, k) >= min_identity.
    Exact and the same from run to run.  Rows and lengths as dist_contain takes them; no [nq, nr] array exists anywhere.
    cap: room for that many hits (default 65 536); when it is too small the call is repeated once with the size the library
    reported."""
    init()
    q, q_len, r, r_len = _within_rows(q, q_len, r, r_len)
    nq, nr, stride = q.shape[0], r.shape[0], q.shape[1]
    cap = 1 << 16 if cap is None else int(cap)
    row_off = np.zeros(nq + 1, dtype=np.uint64)
    found = ctypes.c_uint64(0)
    for _ in range(2):
        ref, shared, n_ref, n_qry = (np.zeros(cap, dtype=np.uint32) for _ in range(4))
        rc = load().mhx_dist_contain_within(q.ctypes.data, q_len.ctypes.data, nq, int(s_q), r.ctypes.data, r_len.ctypes.data, nr, int(s_r), stride, int(k),
                                            float(min_identity), _count(min_shared), row_off.ctypes.data, ref.ctypes.data, shared.ctypes.data,
                                            n_ref.ctypes.data, n_qry.ctypes.data, cap, ctypes.byref(found), 0)
        if rc != MHX_E_CAPACITY or found.value <= cap:
            break
        cap = found.value
    _check(rc)
    m = found.value
    return row_off, ref[:m].copy(), shared[:m].copy(), n_ref[:m].copy(), n_qry[:m].copy()


def dist_contain_within_counts(q: np.ndarray, q_len: np.ndarray, r: np.ndarray, r_len: np.ndarray, s_q: int, s_r: int, k: int,
                               min_identity: float = 0.0, min_shared: int = 1) -> np.ndarray:
    """The counting form of dist_contain_within: row_off [nq + 1] alone (row_off[nq] the number of hits), no hit is stored."""
    init()
    q, q_len, r, r_len = _within_rows(q, q_len, r, r_len)
    nq = q.shape[0]
    row_off = np.zeros(nq + 1, dtype=np.uint64)
    found = ctypes.c_uint64(0)
    _check(load().mhx_dist_contain_within(q.ctypes.data, q_len.ctypes.data, nq, int(s_q), r.ctypes.data, r_len.ctypes.data, r.shape[0], int(s_r), q.shape[1],
                                          int(k), float(min_identity), _count(min_shared), row_off.ctypes.data, None, None, None, None, 0,
                                          ctypes.byref(found), 0))
    return row_off


def dist_contain_within_device(q_ptr: int, q_len_ptr: int, nq: int, s_q: int, r_ptr: int, r_len_ptr: int, nr: int, s_r: int, stride: int, k: int,
                               min_identity: float, min_shared: int, row_off_ptr: int, ref_ptr: int, shared_ptr: int, n_ref_ptr: int, n_qry_ptr: int,
                               cap: int) -> int:
    """Device pointers in and out (row_off [nq + 1] of 64-bit words, the hit arrays [cap]; a sketch_segments_device result goes
    straight in on either side): the CSR stays on the device, exact and in its final order -- the integers are those of
    dist_contain_within bit for bit.  Lengths the host cannot see are clipped to the stride and the sketch size.  All four hit
    pointers 0 with cap == 0 only counts.  Returns the number of hits; EngineError(MHX_E_CAPACITY) when it exceeds cap (row_off
    is complete then, the message names the number)."""
    init()
    v = ctypes.c_void_p
    found = ctypes.c_uint64(0)
    _check(load().mhx_dist_contain_within(v(q_ptr), v(q_len_ptr), nq, int(s_q), v(r_ptr), v(r_len_ptr), nr, int(s_r), stride, int(k), float(min_identity),
                                          _count(min_shared), v(row_off_ptr), v(ref_ptr or None), v(shared_ptr or None), v(n_ref_ptr or None),
                                          v(n_qry_ptr or None), int(cap), ctypes.byref(found), 1))
    return int(found.value)


def dist_contain_winner(q: np.ndarray, q_len: np.ndarray, r: np.ndarray, r_len: np.ndarray, s_q: int, s_r: int, ref_length=None
                        ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """Winner-take-all containment (mhx_dist_contain_winner): (won, shared, n_qry, n_ref) of shape [nq, nr]; the last three are
    dist_contain's.  Every value a query shares with the reference set is credited to the best-ranked reference it was found
    in -- the greater shared / n_ref for this query, then the greater ref_length (u64 [nr], None: all equal), then the lower
    index -- and won[q, r] counts what r was credited with."""
    init()
    q = np.ascontiguousarray(q, dtype=np.uint64)
    r = np.ascontiguousarray(r, dtype=np.uint64)
    assert q.ndim == 2 and r.ndim == 2 and q.shape[1] == r.shape[1]
    q_len = np.ascontiguousarray(q_len, dtype=np.uint32)
    r_len = np.ascontiguousarray(r_len, dtype=np.uint32)
    nq, nr, stride = q.shape[0], r.shape[0], q.shape[1]
    if ref_length is not None:
        ref_length = np.ascontiguousarray(ref_length, dtype=np.uint64)
        assert ref_length.shape == (nr,)
    won, shared, n_qry, n_ref = (np.zeros((nq, nr), dtype=np.uint32) for _ in range(4))
    _check(load().mhx_dist_contain_winner(q.ctypes.data, q_len.ctypes.data, nq, int(s_q), r.ctypes.data, r_len.ctypes.data, nr, int(s_r), stride,
                                          None if ref_length is None else ref_length.ctypes.data, won.ctypes.data, shared.ctypes.data,
                                          n_qry.ctypes.data, n_ref.ctypes.data, 0))
    return won, shared, n_qry, n_ref


def dist_contain_winner_device(q_ptr: int, q_len_ptr: int, nq: int, s_q: int, r_ptr: int, r_len_ptr: int, nr: int, s_r: int, stride: int,
                               ref_length_ptr: int, won_ptr: int, shared_ptr: int, n_qry_ptr: int, n_ref_ptr: int) -> float:
    """Device pointers in and out ([nq, nr] each; ref_length_ptr: u64 [nr] on the device, or 0): the same integers as
    dist_contain_winner.  Returns the kernel time in ms, the plain pass included."""
    init()
    v = ctypes.c_void_p
    _check(load().mhx_dist_contain_winner(v(q_ptr), v(q_len_ptr), nq, int(s_q), v(r_ptr), v(r_len_ptr), nr, int(s_r), stride, v(ref_length_ptr or None),
                                          v(won_ptr), v(shared_ptr), v(n_qry_ptr), v(n_ref_ptr), 1))
    return load().mhx_last_dist_kernel_ms()


def _support_cand(cand, n_cand, nq: int):
    if cand is None:
        return None, None
    cand = np.ascontiguousarray(cand, dtype=np.uint32)
    n_cand = np.ascontiguousarray(n_cand, dtype=np.uint32)
    assert cand.ndim == 2 and cand.shape[0] == nq and n_cand.shape == (nq,)
    return cand, n_cand


def dist_support(q: np.ndarray, q_len: np.ndarray, r: np.ndarray, r_len: np.ndarray, s: int, replicates: int, keep: float = 0.5, seed: int = 42,
                 cand=None, n_cand=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """Jackknife support of search hits (mhx_dist_support).  cand [nq, top] holds per query the indices of its candidate
    references, the first n_cand [nq] of a row valid; cand None: references 0 .. nr - 1 (nr <= 64) for every query.  Returns
    first [nq, top], in how many of the `replicates` resampled sketches each candidate is the best one, rep_best [nq, R] (the
    best reference of every replicate, 0xFFFFFFFF without candidates), rep_s [nq, R] (its sketch size s_r), and rep_common,
    rep_denom [nq, top, R], the pair results of every replicate."""
    init()
    q = np.ascontiguousarray(q, dtype=np.uint64)
    r = np.ascontiguousarray(r, dtype=np.uint64)
    assert q.ndim == 2 and r.ndim == 2 and q.shape[1] == r.shape[1]
    q_len = np.ascontiguousarray(q_len, dtype=np.uint32)
    r_len = np.ascontiguousarray(r_len, dtype=np.uint32)
    nq, nr, stride = q.shape[0], r.shape[0], q.shape[1]
    cand, n_cand = _support_cand(cand, n_cand, nq)
    top = nr if cand is None else cand.shape[1]
    R = max(int(replicates), 0)
    first = np.zeros((nq, top), dtype=np.uint32)
    rep_best, rep_s = np.zeros((nq, R), dtype=np.uint32), np.zeros((nq, R), dtype=np.uint32)
    rep_common, rep_denom = np.zeros((nq, top, R), dtype=np.uint32), np.zeros((nq, top, R), dtype=np.uint32)
    _check(load().mhx_dist_support(q.ctypes.data, q_len.ctypes.data, nq, r.ctypes.data, r_len.ctypes.data, nr, stride, s,
                                   None if cand is None else cand.ctypes.data, None if cand is None else n_cand.ctypes.data, top, int(replicates),
                                   float(keep), seed, first.ctypes.data, rep_best.ctypes.data, rep_s.ctypes.data, rep_common.ctypes.data,
                                   rep_denom.ctypes.data, 0))
    return first, rep_best, rep_s, rep_common, rep_denom


def dist_support_device(q_ptr: int, q_len_ptr: int, nq: int, r_ptr: int, r_len_ptr: int, nr: int, stride: int, s: int, top: int, replicates: int,
                        keep: float, seed: int, cand_ptr: int, n_cand_ptr: int, first_ptr: int, rep_best_ptr: int = 0, rep_s_ptr: int = 0,
                        rep_common_ptr: int = 0, rep_denom_ptr: int = 0) -> float:
    """Device pointers in and out (shapes as dist_support; cand_ptr 0: references 0 .. nr - 1, top == nr; each rep_* pointer
    may be 0, rep_common and rep_denom both or neither): the same bytes as dist_support gives, left on the device.  The
    hits of dist_search_device go straight in as candidates.  Returns the kernel time in ms."""
    init()
    v = ctypes.c_void_p
    _check(load().mhx_dist_support(v(q_ptr), v(q_len_ptr), nq, v(r_ptr), v(r_len_ptr), nr, stride, s, v(cand_ptr or None), v(n_cand_ptr or None), int(top),
                                   int(replicates), float(keep), seed, v(first_ptr), v(rep_best_ptr or None), v(rep_s_ptr or None),
                                   v(rep_common_ptr or None), v(rep_denom_ptr or None), 1))
    return load().mhx_last_dist_kernel_ms()
