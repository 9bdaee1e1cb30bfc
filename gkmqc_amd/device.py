"""ctypes binding of the C ABI exported by ``bin/gkmkern_pylib.so``.

Two layers, both declared under ``include/``:
  * ``gkm_main_pywrapper`` -- the drop-in boundary (include/gkmkern_pylib.h), bound exactly
    as the reference binds it (scripts/gkmsvm.py:48-61,85-88);
  * ``gkmhip_*`` -- the device layer (include/gkm_hip.h) used by bench.py and the GPU tests
    with device memory and streams supplied by PyTorch-ROCm.

There is no CPU compute path here: if the shared object is missing the import of the
library fails loudly, and on a box without a GPU the device calls return errors.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(HERE, "bin")
LIB_NAME = "gkmkern_pylib.so"

KERNEL_AUTO, KERNEL_DIRECT, KERNEL_BITSLICE = 0, 1, 2
# the bit-sliced kernel with group records where a same-length launch takes shift records by default: the cross-check
KERNEL_BITSLICE_GROUPS = 3


class gkmOpt(ctypes.Structure):
    """Same layout as the reference's gkmOpt (src/libgkm.h:149-161)."""
    _fields_ = (
        ("kernel_type", ctypes.c_int), ("L", ctypes.c_int), ("k", ctypes.c_int), ("d", ctypes.c_int),
        ("M", ctypes.c_uint8), ("H", ctypes.c_double), ("gamma", ctypes.c_double),
        ("posfile", ctypes.c_char_p), ("negfile", ctypes.c_char_p),
        ("nthreads", ctypes.c_int), ("verbosity", ctypes.c_int),
    )


class GkmError(RuntimeError):
    pass


_lib = None


def lib_path():
    # GKM_LIB_PATH: load another build of the same library (A/B timing of kernel variants)
    return os.environ.get("GKM_LIB_PATH") or os.path.join(LIB_DIR, LIB_NAME)


def load():
    """Load (once) and prototype the shared object.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm bundles its own HIP runtime: if this library (linked against /opt/rocm) were
    # loaded first, torch would afterwards find "no HIP GPUs".  Import torch first when it exists
    # so that one runtime serves both.  (The reference's own caller does not use torch at all.)
    import importlib.util
    if importlib.util.find_spec("torch") is not None:
        import torch  # noqa: F401
    path = lib_path()
    if not os.path.exists(path):
        raise GkmError("%s is missing: build it with `make -C gkmqc_amd/csrc` "
                       "(or `python -c 'import __graft_entry__ as g; g.build()'`)" % path)
    L = ctypes.CDLL(path)
    vp, i32, i64, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    L.gkm_main_pywrapper.restype = i32
    L.gkm_main_pywrapper.argtypes = (ctypes.POINTER(gkmOpt), vp, vp)
    L.gkm_check_parameter_values.restype = ctypes.c_char_p
    L.gkm_check_parameter_values.argtypes = (i32, i32, i32, i32)
    L.gkm_mismatch_weights.restype = i32
    L.gkm_mismatch_weights.argtypes = (i32, i32, i32, vp)
    L.gkm_position_weights.restype = None
    L.gkm_position_weights.argtypes = (i32, i32, ctypes.c_uint8, dbl, vp)
    L.gkm_problem_read.restype = vp
    L.gkm_problem_read.argtypes = (ctypes.c_char_p, ctypes.c_char_p)
    L.gkm_problem_read_one.restype = vp
    L.gkm_problem_read_one.argtypes = (ctypes.c_char_p,)
    L.gkm_problem_name.restype = ctypes.c_char_p
    L.gkm_problem_name.argtypes = (vp, i32)
    L.gkm_problem_free.restype = None
    L.gkm_problem_free.argtypes = (vp,)
    for name in ("gkm_problem_size", "gkm_problem_npos"):
        getattr(L, name).restype = i32
        getattr(L, name).argtypes = (vp,)
    L.gkm_problem_seqlen.restype = i32
    L.gkm_problem_seqlen.argtypes = (vp, i32)
    L.gkm_problem_codes.restype = ctypes.POINTER(ctypes.c_uint8)
    L.gkm_problem_codes.argtypes = (vp, i32)
    L.gkm_problem_offsets.restype = ctypes.POINTER(ctypes.c_int64)
    L.gkm_problem_offsets.argtypes = (vp,)
    L.gkm_problem_all_codes.restype = ctypes.POINTER(ctypes.c_uint8)
    L.gkm_problem_all_codes.argtypes = (vp,)
    for name in ("gkm_problem_invalid_chars", "gkm_problem_truncated"):
        getattr(L, name).restype = ctypes.c_long
        getattr(L, name).argtypes = (vp,)

    L.gkmhip_last_error.restype = ctypes.c_char_p
    L.gkmhip_device_count.restype = i32
    L.gkmhip_create.restype = vp
    L.gkmhip_create.argtypes = (i32, i32, i32, vp, i32, dbl)
    L.gkmhip_destroy.restype = None
    L.gkmhip_destroy.argtypes = (vp,)
    L.gkmhip_set_kernel.restype = i32
    L.gkmhip_set_kernel.argtypes = (vp, i32)
    L.gkmhip_set_scratch_slot.restype = i32
    L.gkmhip_set_scratch_slot.argtypes = (vp, i32)
    L.gkmhip_set_sequences.restype = i32
    L.gkmhip_set_sequences.argtypes = (vp, i32, vp, vp, vp, i32, vp)
    L.gkmhip_gram_rows.restype = i32
    L.gkmhip_gram_rows.argtypes = (vp, vp, i32, i32, vp, i64, vp, i64, vp)
    if hasattr(L, "gkmhip_gram_rows_packed"):   # (older builds loaded through GKM_LIB_PATH for A/B timing lack it)
        L.gkmhip_gram_rows_packed.restype = i32
        L.gkmhip_gram_rows_packed.argtypes = (vp, vp, i32, vp, vp, vp)
        L.gkmhip_allgather_bytes_per_rank.restype = ctypes.c_longlong
    L.gkmhip_gram_rows_full.restype = i32
    L.gkmhip_gram_rows_full.argtypes = (vp, vp, i32, i32, vp, i64, vp)
    L.gkmhip_gram_block.restype = i32
    L.gkmhip_gram_block.argtypes = (vp, vp, i32, i32, i32, vp, i64, vp)
    L.gkmhip_normalize_block.restype = i32
    L.gkmhip_normalize_block.argtypes = (vp, vp, i32, i32, i32, vp, i64, vp, vp)
    L.gkmhip_explain_block.restype = i32
    L.gkmhip_explain_block.argtypes = (vp, vp, i32, i32, i32, vp, vp, vp, vp, vp)
    L.gkmhip_ism_block.restype = i32
    L.gkmhip_ism_block.argtypes = (vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp)
    L.gkmhip_ism_rbf_block.restype = i32
    L.gkmhip_ism_rbf_block.argtypes = (vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp)
    L.gkmhip_hyp_block.restype = i32
    L.gkmhip_hyp_block.argtypes = (vp, vp, i32, i32, i32, vp, vp, vp, vp)
    L.gkmhip_lmer_weights.restype = i32
    L.gkmhip_lmer_weights.argtypes = (vp, vp, vp, vp, i32, ctypes.c_uint32, ctypes.c_uint32, vp, vp)
    L.gkmhip_lmer_score.restype = i32
    L.gkmhip_lmer_score.argtypes = (vp, i32, i32, vp, vp, vp)
    L.gkmhip_lmer_importance.restype = i32
    L.gkmhip_lmer_importance.argtypes = (vp, vp, vp, vp, i32, ctypes.c_uint32, ctypes.c_uint32, vp, vp)
    L.gkmhip_lmer_explain.restype = i32
    L.gkmhip_lmer_explain.argtypes = (vp, i32, i32, vp, vp, vp, vp)
    L.gkmhip_lmer_hyp.restype = i32
    L.gkmhip_lmer_hyp.argtypes = (vp, i32, i32, vp, vp, vp)
    L.gkmhip_scan_lmers.restype = i32
    L.gkmhip_scan_lmers.argtypes = (vp, vp, vp, i64, vp, vp)
    L.gkmhip_scan_profiles.restype = i32
    L.gkmhip_scan_profiles.argtypes = (vp, vp, i64, vp, i32, i32, i64, vp, vp)
    L.gkmhip_scan_score.restype = i32
    L.gkmhip_scan_score.argtypes = (vp, vp, i64, vp, i32, i32, i64, vp, vp, vp)
    L.gkmhip_scan_group.restype = i32
    L.gkmhip_scan_group.argtypes = (vp, i32, i32)
    if hasattr(L, "gkmhip_wsim_profiles"):   # (as the calls below: older builds lack them; GramContext's wsim methods say so)
        L.gkmhip_wsim_profiles.restype = i32
        L.gkmhip_wsim_profiles.argtypes = (vp, vp, i64, vp, i64, i32, i32, i32, i64, i64, vp, i64, vp, vp)
        L.gkmhip_wsim_normalize.restype = i32
        L.gkmhip_wsim_normalize.argtypes = (vp, vp, i64, i64, i64, vp, vp, vp)
        L.gkmhip_wsim_best.restype = i32
        L.gkmhip_wsim_best.argtypes = (vp, vp, i64, i64, i64, i64, i64, i64, i64, i64, vp, vp, vp)
        L.gkmhip_wsim_group.restype = i32
        L.gkmhip_wsim_group.argtypes = (i32, i32, i32, i32, i32, vp, vp)
    if hasattr(L, "gkmhip_walign_block"):   # (older builds lack them; GramContext's walign methods say so)
        L.gkmhip_walign_tile.restype = i32
        L.gkmhip_walign_tile.argtypes = (vp, vp)
        L.gkmhip_walign_scratch_bytes.restype = i64
        L.gkmhip_walign_scratch_bytes.argtypes = (i64, i64)
        L.gkmhip_walign_block.restype = i32
        L.gkmhip_walign_block.argtypes = (vp, vp, i64, i64, i64, i32, dbl, dbl, vp, vp, vp, vp, i64, vp, vp, vp, i64, vp)
        L.gkmhip_walign_trace.restype = i32
        L.gkmhip_walign_trace.argtypes = (vp, vp, i64, i64, i64, i64, i64, vp, i64, vp, vp)
    if hasattr(L, "gkmhip_regions_count"):   # (as the panel calls below: older builds lack them; GramContext's
                                             # region methods say so when called on one)
        L.gkmhip_regions_scratch_bytes.restype = i64
        L.gkmhip_regions_scratch_bytes.argtypes = (i64, i64)
        L.gkmhip_regions_count.restype = i32
        L.gkmhip_regions_count.argtypes = (vp, vp, i64, vp, i64, i32, i32, i64, dbl, i64, vp, i64, vp, vp)
        L.gkmhip_regions_fill.restype = i32
        L.gkmhip_regions_fill.argtypes = (vp, vp, i64, vp, i64, i32, i32, i64, dbl, i64, vp, i64, i64, vp, vp, vp, vp, vp, vp)
        L.gkmhip_regions_span.restype = i32
        L.gkmhip_regions_span.argtypes = ()
    if hasattr(L, "gkmhip_dist_digits"):     # (likewise: GramContext's dist methods say so on an older build)
        L.gkmhip_dist_digit_bits.restype = i32
        L.gkmhip_dist_digit_bits.argtypes = ()
        L.gkmhip_dist_scratch_bytes.restype = i64
        L.gkmhip_dist_scratch_bytes.argtypes = (i64, i64)
        L.gkmhip_dist_digits.restype = i32
        L.gkmhip_dist_digits.argtypes = (vp, vp, i64, vp, i64, i32, i32, i64, vp, i32, i32, vp, vp, i64, vp)
        L.gkmhip_dist_edges.restype = i32
        L.gkmhip_dist_edges.argtypes = (vp, vp, i64, vp, i64, i32, i32, i64, vp, i32, vp, vp, i64, vp)
        L.gkmhip_dist_collect.restype = i32
        L.gkmhip_dist_collect.argtypes = (vp, vp, i64, vp, i64, i32, i32, i64, vp, i32, i32, vp, i64, vp, vp, i64, vp)
    L.gkmhip_delta_sat.restype = i32
    L.gkmhip_delta_sat.argtypes = (vp, vp, i64, i64, i64, vp, vp, vp)
    L.gkmhip_delta_variants.restype = i32
    L.gkmhip_delta_variants.argtypes = (vp, vp, vp, i64, vp, i32, vp, i64, vp, vp, vp)
    if hasattr(L, "gkmhip_panel_score"):   # (older builds loaded through GKM_LIB_PATH for A/B timing lack them)
        L.gkmhip_panel_score.restype = i32
        L.gkmhip_panel_score.argtypes = (vp, i32, i32, vp, i32, i32, vp, vp)
        L.gkmhip_panel_scan_score.restype = i32
        L.gkmhip_panel_scan_score.argtypes = (vp, vp, i64, vp, i32, i32, i64, vp, i32, i32, vp, vp)
        L.gkmhip_panel_delta_sat.restype = i32
        L.gkmhip_panel_delta_sat.argtypes = (vp, vp, i64, i64, i64, vp, i32, i32, vp, vp)
        L.gkmhip_panel_delta_variants.restype = i32
        L.gkmhip_panel_delta_variants.argtypes = (vp, vp, vp, i64, vp, i32, vp, i64, vp, i32, i32, vp, vp)
    if hasattr(L, "gkmhip_panel_weights"):   # (older builds lack it; GramContext.panel_weights says so)
        L.gkmhip_panel_weights.restype = i32
        L.gkmhip_panel_weights.argtypes = (vp, vp, vp, vp, i32, i32, i32, ctypes.c_uint32, ctypes.c_uint32, vp, vp)
    if hasattr(L, "gkmhip_lmer_contract"):   # (older builds lack them; GramContext's contract methods say so)
        L.gkmhip_contract_max_windows.restype = i64
        L.gkmhip_contract_max_windows.argtypes = (i32, i32)
        L.gkmhip_contract_scratch_bytes.restype = i64
        L.gkmhip_contract_scratch_bytes.argtypes = (i32, i32, i64)
        L.gkmhip_lmer_contract.restype = i32
        L.gkmhip_lmer_contract.argtypes = (vp, vp, vp, i64, vp, vp)
        L.gkmhip_panel_contract.restype = i32
        L.gkmhip_panel_contract.argtypes = (vp, vp, i32, i32, vp, i64, vp, i64, vp)
    L.gkmhip_nullidx_tile.restype = i32
    L.gkmhip_nullidx_tile.argtypes = ()
    L.gkmhip_nullidx_scratch_bytes.restype = i64
    L.gkmhip_nullidx_scratch_bytes.argtypes = (i64, i32)
    L.gkmhip_nullidx_keys.restype = i32
    L.gkmhip_nullidx_keys.argtypes = (i32, vp, i64, i32, vp, vp, vp, vp, vp)
    L.gkmhip_nullidx_cells.restype = i32
    L.gkmhip_nullidx_cells.argtypes = (i32, vp, i64, i32, vp, vp, i64, vp)
    L.gkmhip_nullidx_sort.restype = i32
    L.gkmhip_nullidx_sort.argtypes = (i32, vp, i64, i32, vp, vp, i64, vp)
    L.gkmhip_ism_self_profiles.restype = i32
    L.gkmhip_ism_self_profiles.argtypes = (vp, i32, i32, vp, vp)
    L.gkmhip_self_profiles.restype = i32
    L.gkmhip_self_profiles.argtypes = (vp, i32, i32, vp, vp)
    L.gkmhip_self_norms.restype = i32
    L.gkmhip_self_norms.argtypes = (vp, vp, vp)
    L.gkmhip_normalize_rows_full.restype = i32
    L.gkmhip_normalize_rows_full.argtypes = (vp, vp, i32, i32, vp, i64, vp, vp)
    L.gkmhip_normalize.restype = i32
    L.gkmhip_normalize.argtypes = (vp, vp, i64, vp, i32, vp)
    L.gkmhip_malloc.restype = vp
    L.gkmhip_malloc.argtypes = (i32, ctypes.c_size_t)
    L.gkmhip_free.restype = None
    L.gkmhip_free.argtypes = (vp,)
    L.gkmhip_memcpy_d2h.restype = i32
    L.gkmhip_memcpy_d2h.argtypes = (vp, vp, ctypes.c_size_t)
    L.gkmhip_memcpy_h2d.restype = i32
    L.gkmhip_memcpy_h2d.argtypes = (vp, vp, ctypes.c_size_t)
    L.gkmhip_sync.restype = i32
    L.gkmhip_sync.argtypes = (vp,)
    L.gkmhip_copy_lower_to_rows.restype = i32
    L.gkmhip_copy_lower_to_rows.argtypes = (vp, vp, i64, i32, vp, i32)
    L.gkmhip_gram_to_host_rows.restype = i32
    L.gkmhip_gram_to_host_rows.argtypes = (vp, vp, i64, vp, i32)
    L.gkmhip_gram_part_to_host_rows.restype = i32
    L.gkmhip_gram_part_to_host_rows.argtypes = (vp, vp, i64, vp, i32, i32, i32)
    L.gkmhip_release_host_cache.restype = None
    L.gkmhip_current_device.restype = i32
    L.gkmhip_set_current_device.restype = i32
    L.gkmhip_set_current_device.argtypes = (i32,)
    L.gkmhip_n_sequences.restype = i32
    L.gkmhip_n_sequences.argtypes = (vp,)
    L.gkmhip_device_of.restype = i32
    L.gkmhip_device_of.argtypes = (vp,)
    L.gkmhip_gram_allgather.restype = i32
    L.gkmhip_gram_allgather.argtypes = (vp, i32, vp, i64, i32, i32)
    if hasattr(L, "gkmhip_gram_rank_alone"):   # (a GKM_LIB_PATH library built from an older revision lacks it: A/B runs)
        L.gkmhip_gram_rank_alone.restype = i32
        L.gkmhip_gram_rank_alone.argtypes = (vp, i32, i32, i32, vp, i64, i32, vp)
    L.gkmhip_last_transport.restype = ctypes.c_char_p
    L.gkmhip_release_comms.restype = None
    if hasattr(L, "gkmhip_kernel_timeline_spans"):
        L.gkmhip_kernel_timeline_spans.restype = i32
        L.gkmhip_kernel_timeline_spans.argtypes = (vp, vp, i32)
    if hasattr(L, "gkmhip_allgather_chunk_times"):
        L.gkmhip_allgather_chunk_times.restype = i32
        L.gkmhip_allgather_chunk_times.argtypes = (i32, vp, i32)
    if hasattr(L, "gkmhip_allgather_stats"):   # (older builds loaded through GKM_LIB_PATH for A/B timing lack them)
        L.gkmhip_allgather_alloc_count.restype = ctypes.c_long
        L.gkmhip_allgather_stats.restype = i32
        L.gkmhip_allgather_stats.argtypes = (vp, i32)
    L.gkmhip_assemble_normalize.restype = i32
    L.gkmhip_assemble_normalize.argtypes = (vp, vp, i64, vp, vp, i64, vp, i32, vp)
    L.gkmhip_last_kernel_ms.restype = dbl
    L.gkmhip_last_kernel_ms.argtypes = (vp,)
    if hasattr(L, "gkmhip_kernel_timeline"):
        L.gkmhip_kernel_timeline.argtypes = (vp, ctypes.c_int)
        L.gkmhip_kernel_timeline_ms.restype = dbl
        L.gkmhip_kernel_timeline_ms.argtypes = (vp, ctypes.POINTER(ctypes.c_int))
    L.gkmhip_last_comparisons.restype = dbl
    L.gkmhip_last_comparisons.argtypes = (vp,)
    L.gkmhip_last_kernel_name.restype = ctypes.c_char_p
    L.gkmhip_last_kernel_name.argtypes = (vp,)
    if hasattr(L, "gkmhip_last_riders"):   # (older builds loaded through GKM_LIB_PATH for A/B timing lack it)
        L.gkmhip_last_riders.restype = i32
        L.gkmhip_last_riders.argtypes = (vp,)
    if hasattr(L, "gkmhip_last_variant"):
        L.gkmhip_last_variant.restype = i32
        L.gkmhip_last_variant.argtypes = (vp,)
    _lib = L
    return L


# ------------------------------------------------------------------ host tables
def check_parameters(kernel_type, L, k, d):
    msg = load().gkm_check_parameter_values(kernel_type, L, k, d)
    return msg.decode() if msg else None


def mismatch_weights(kernel_type, L, k):
    out = np.zeros(L + 1, dtype=np.float64)
    if load().gkm_mismatch_weights(kernel_type, L, k, out.ctypes.data):
        raise GkmError("invalid (kernel_type, L, k)")
    return out


def position_weights(kernel_type, n, M=50, H=50.0):
    out = np.zeros(max(n, 0), dtype=np.uint8)
    load().gkm_position_weights(kernel_type, n, M, float(H), out.ctypes.data)
    return out


def distance_weights(kernel_type, max_n, M=50, H=50.0):
    """wd[D] = positional weight of an l-mer at distance D from the centre l-mer; the
    reference's w(n, p) (src/libgkm.c:912-925) equals wd[|n//2 - p|] for every n."""
    dmax = max_n // 2 + 1
    return np.ascontiguousarray(position_weights(kernel_type, 2 * dmax + 1, M, H)[dmax:])


def wsim_group(L, d, width, stride_x, stride_y):
    """(gx, gy): the windows of x and of y that one tile of k_wsim_profiles holds, a function of the five arguments only
    (include/gkm_hip.h gkmhip_wsim_group; needs no device); (0, 0) for arguments the launch refuses."""
    lib = load()
    if not hasattr(lib, "gkmhip_wsim_group"):
        raise GkmError("%s holds no gkmhip_wsim_group: it was built before the window-pair calls" % lib_path())
    gx, gy = ctypes.c_int(0), ctypes.c_int(0)
    lib.gkmhip_wsim_group(int(L), int(d), int(width), int(stride_x), int(stride_y), ctypes.addressof(gx),
                          ctypes.addressof(gy))
    return gx.value, gy.value


def _walign_lib():
    lib = load()
    if not hasattr(lib, "gkmhip_walign_block"):
        raise GkmError("%s holds no gkmhip_walign_block: it was built before the window-alignment calls" % lib_path())
    return lib


def walign_tile():
    """(rows, columns) of a DP tile of k_walign_tiles (include/gkm_hip.h gkmhip_walign_tile; needs no device)."""
    rows, cols = ctypes.c_int(0), ctypes.c_int(0)
    _walign_lib().gkmhip_walign_tile(ctypes.addressof(rows), ctypes.addressof(cols))
    return rows.value, cols.value


def walign_scratch_bytes(nwx, nwy):
    """The bytes of device scratch gkmhip_walign_block needs for a block of nwx x nwy cells; -1 for a shape it refuses
    (needs no device)."""
    return int(_walign_lib().gkmhip_walign_scratch_bytes(int(nwx), int(nwy)))


def _contract_lib():
    lib = load()
    if not hasattr(lib, "gkmhip_lmer_contract"):
        raise GkmError("%s holds no gkmhip_lmer_contract: it was built before the window contraction calls" % lib_path())
    return lib


def contract_max_windows(L, n_models=0):
    """The most windows one lmer_contract (n_models = 0) or panel_contract call takes; -1 for refused arguments (needs no
    device)."""
    return int(_contract_lib().gkmhip_contract_max_windows(int(L), int(n_models)))


def contract_scratch_bytes(L, n_models, nwin):
    """The bytes of partial values the context holds for such a call (0 for L <= 6); -1 for refused arguments."""
    return int(_contract_lib().gkmhip_contract_scratch_bytes(int(L), int(n_models), int(nwin)))


_KNN_LIB = None


def _knn_lib():
    global _KNN_LIB
    if _KNN_LIB is None:
        lib = load()
        if not hasattr(lib, "gkmhip_knn_merge"):
            raise GkmError("%s holds no gkmhip_knn_merge: it was built before the neighbour calls" % lib_path())
        vp, i32, i64, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
        lib.gkmhip_knn_merge.restype = i32
        lib.gkmhip_knn_merge.argtypes = (i32, vp, i64, i64, i64, vp, i64, i32, i32, vp, vp, vp)
        lib.gkmhip_pairs_count.restype = i32
        lib.gkmhip_pairs_count.argtypes = (i32, vp, i64, i64, i64, vp, i64, i32, dbl, vp, vp)
        lib.gkmhip_pairs_fill.restype = i32
        lib.gkmhip_pairs_fill.argtypes = (i32, vp, i64, i64, i64, vp, i64, i32, dbl, vp, i64, vp, vp, vp, vp)
        _KNN_LIB = lib
    return _KNN_LIB


def _knn_chk(rc, what):
    if rc:
        raise GkmError("%s failed (%d): %s" % (what, rc, load().gkmhip_last_error().decode()))


def knn_merge(device, K_ptr, ld, nrows, ncols, row_id_ptr, col_base, mode, kcap, best_idx_ptr, best_val_ptr, stream=0):
    """The eligible cells of a device block merged into every row's running list of its kcap best columns (include/
    gkm_hip.h gkmhip_knn_merge): all arguments but the sizes are device pointers; one call per column block."""
    _knn_chk(_knn_lib().gkmhip_knn_merge(int(device), K_ptr, int(ld), int(nrows), int(ncols), row_id_ptr, int(col_base),
                                         int(mode), int(kcap), best_idx_ptr, best_val_ptr, stream), "gkmhip_knn_merge")


def pairs_count(device, K_ptr, ld, nrows, ncols, row_id_ptr, col_base, mode, threshold, count_ptr, stream=0):
    """count[i] = the eligible cells of row i at or above `threshold` (gkmhip_pairs_count); count: device int64."""
    _knn_chk(_knn_lib().gkmhip_pairs_count(int(device), K_ptr, int(ld), int(nrows), int(ncols), row_id_ptr, int(col_base),
                                           int(mode), float(threshold), count_ptr, stream), "gkmhip_pairs_count")


def pairs_fill(device, K_ptr, ld, nrows, ncols, row_id_ptr, col_base, mode, threshold, offset_ptr, capacity, out_i_ptr,
               out_j_ptr, out_v_ptr, stream=0):
    """Those cells as (row_id[i], column, value) from slot offset[i] on, ascending column within a row
    (gkmhip_pairs_fill); nothing is written at or beyond `capacity`."""
    _knn_chk(_knn_lib().gkmhip_pairs_fill(int(device), K_ptr, int(ld), int(nrows), int(ncols), row_id_ptr, int(col_base),
                                          int(mode), float(threshold), offset_ptr, int(capacity), out_i_ptr, out_j_ptr,
                                          out_v_ptr, stream), "gkmhip_pairs_fill")


class FlatSequences:
    """All sequences of a problem back to back: `codes` (uint8, 0..3) and `off` (int64, n+1).
    Behaves like a list of per-sequence arrays (views) where one is needed."""

    def __init__(self, codes, off):
        self.codes, self.off = codes, off

    def __len__(self):
        return len(self.off) - 1

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        return self.codes[self.off[i]:self.off[i + 1]]

    def __iter__(self):
        return (self[i] for i in range(len(self)))


def read_problem(posfile, negfile):
    """FASTA pair -> (FlatSequences of base codes, n_pos, n_invalid_chars, n_truncated).
    Two bulk copies out of the C reader, no per-sequence work in Python."""
    L = load()
    h = L.gkm_problem_read(os.fsencode(posfile), os.fsencode(negfile))
    if not h:
        raise GkmError("cannot read %s / %s" % (posfile, negfile))
    try:
        n = L.gkm_problem_size(h)
        off = np.ctypeslib.as_array(L.gkm_problem_offsets(h), shape=(n + 1,)).copy()
        total = int(off[-1])
        codes = (np.ctypeslib.as_array(L.gkm_problem_all_codes(h), shape=(total,)).copy() if total
                 else np.zeros(0, np.uint8))
        return (FlatSequences(codes, off), L.gkm_problem_npos(h), L.gkm_problem_invalid_chars(h),
                L.gkm_problem_truncated(h))
    finally:
        L.gkm_problem_free(h)


def read_fasta(path):
    """One FASTA file -> (FlatSequences of base codes, header names, n_invalid_chars, n_truncated), with the record
    rules, invalid characters and truncation of `read_problem` (the same C parser), so that a query is encoded exactly
    as it would have been for training."""
    L = load()
    h = L.gkm_problem_read_one(os.fsencode(path))
    if not h:
        raise GkmError("cannot read %s" % path)
    try:
        n = L.gkm_problem_size(h)
        off = np.ctypeslib.as_array(L.gkm_problem_offsets(h), shape=(n + 1,)).copy()
        total = int(off[-1])
        codes = (np.ctypeslib.as_array(L.gkm_problem_all_codes(h), shape=(total,)).copy() if total
                 else np.zeros(0, np.uint8))
        names = [L.gkm_problem_name(h, i).decode("utf-8", "replace") for i in range(n)]
        return FlatSequences(codes, off), names, L.gkm_problem_invalid_chars(h), L.gkm_problem_truncated(h)
    finally:
        L.gkm_problem_free(h)


def encode(seq):
    """bytes/str of ACGT (any case; other characters count as A) -> uint8 codes 0..3."""
    if isinstance(seq, str):
        seq = seq.encode()
    lut = np.zeros(256, dtype=np.uint8)
    for ch, v in ((b"C", 1), (b"G", 2), (b"T", 3), (b"c", 1), (b"g", 2), (b"t", 3)):
        lut[ch[0]] = v
    return lut[np.frombuffer(seq, dtype=np.uint8)]


# ------------------------------------------------------------------ device layer
def _row_pointers(host, n):
    """The row-pointer table of the copy-out calls for a 2-D fp64 numpy array with at least n rows and n columns (rows
    may be wider: the reference's caller hands in a larger matrix, scripts/gkmsvm.py:67-99)."""
    if not (isinstance(host, np.ndarray) and host.ndim == 2 and host.dtype == np.float64 and host.flags.writeable
            and host.strides[1] == 8 and host.strides[0] >= 8 * host.shape[1] and host.shape[0] >= n and host.shape[1] >= n):
        raise GkmError("the host matrix must be a writeable 2-D fp64 array of at least n x n with unit column stride")
    return (host.ctypes.data + np.arange(host.shape[0]) * host.strides[0]).astype(np.uintp)


class GramContext:
    """Owns one gkmhip_ctx: parameters + uploaded sequences on one GPU."""

    def __init__(self, kernel_type, L, k, d, M=50, H=50.0, gamma=1.0, device=0):
        bad = check_parameters(kernel_type, L, k, d)
        if bad:
            raise GkmError(bad)
        self.lib = load()
        self.kernel_type, self.L, self.k, self.d, self.M, self.H, self.gamma = kernel_type, L, k, d, M, H, gamma
        self.weighted = kernel_type in (4, 5)
        self.rbf = kernel_type in (3, 5)
        self.c = mismatch_weights(kernel_type, L, k)
        self.device = device
        self.n = 0
        self.handle = self.lib.gkmhip_create(device, L, d, self.c.ctypes.data, int(self.rbf), float(gamma))
        if not self.handle:
            raise GkmError("gkmhip_create: " + self.lib.gkmhip_last_error().decode())

    def _chk(self, rc, what):
        if rc:
            raise GkmError("%s failed (%d): %s" % (what, rc, self.lib.gkmhip_last_error().decode()))

    def close(self):
        if getattr(self, "handle", None):
            self.lib.gkmhip_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_kernel(self, which):
        self._chk(self.lib.gkmhip_set_kernel(self.handle, which), "gkmhip_set_kernel")

    def set_scratch_slot(self, slot):
        """Launches alternating between two streams alternate the scratch slot (include/gkm_hip.h)."""
        self._chk(self.lib.gkmhip_set_scratch_slot(self.handle, slot), "gkmhip_set_scratch_slot")

    def set_sequences(self, seqs, stream=0):
        """seqs: list of uint8 arrays of base codes 0..3, or a FlatSequences."""
        n = len(seqs)
        if isinstance(seqs, FlatSequences):
            off = np.ascontiguousarray(seqs.off, dtype=np.int64)
            codes = np.ascontiguousarray(seqs.codes, dtype=np.uint8)
            lens = np.diff(off)
        else:
            lens = np.array([len(s) for s in seqs], dtype=np.int64)
            off = np.zeros(n + 1, dtype=np.int64)
            np.cumsum(lens, out=off[1:])
            codes = np.concatenate(seqs).astype(np.uint8) if n else np.zeros(0, np.uint8)
        if (lens < self.L).any():
            raise GkmError("a sequence is shorter than L")
        wd = None
        if self.weighted:
            wd = distance_weights(self.kernel_type, int(lens.max()) - self.L + 1, self.M, self.H)
        self._keep = (codes, off, wd)
        self._chk(self.lib.gkmhip_set_sequences(
            self.handle, n, codes.ctypes.data, off.ctypes.data,
            wd.ctypes.data if wd is not None else None, len(wd) if wd is not None else 0, stream),
            "gkmhip_set_sequences")
        self.n = n
        self.lens = lens

    def gram_rows(self, rows, G_ptr, ld, P_ptr=None, ldp=0, local_rows=True, stream=0):
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        self._chk(self.lib.gkmhip_gram_rows(self.handle, rows.ctypes.data, len(rows), int(local_rows), G_ptr, ld,
                                            P_ptr, ldp, stream), "gkmhip_gram_rows")

    def gram_rows_packed(self, rows, G_ptr, row_off, stream=0):
        """Row rows[i] -> G_ptr + row_off[i] doubles, columns 0..rows[i] only (packed slabs, sharding.py)."""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        row_off = np.ascontiguousarray(row_off[:len(rows)], dtype=np.int64)
        self._chk(self.lib.gkmhip_gram_rows_packed(self.handle, rows.ctypes.data, len(rows), G_ptr, row_off.ctypes.data,
                                                   stream), "gkmhip_gram_rows_packed")

    def gram_rows_full(self, rows, G_ptr, ld, local_rows=True, stream=0):
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        self._chk(self.lib.gkmhip_gram_rows_full(self.handle, rows.ctypes.data, len(rows), int(local_rows), G_ptr, ld,
                                                 stream), "gkmhip_gram_rows_full")

    def gram_block(self, rows, col_begin, col_end, G_ptr, ld, stream=0):
        """Raw G(rows[i], j) for col_begin <= j < col_end into G_ptr[i*ld + (j - col_begin)] (include/gkm_hip.h)."""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        self._chk(self.lib.gkmhip_gram_block(self.handle, rows.ctypes.data, len(rows), int(col_begin), int(col_end), G_ptr,
                                             ld, stream), "gkmhip_gram_block")

    def normalize_block(self, rows, col_begin, col_end, G_ptr, ld, sq_ptr, stream=0):
        """Kernel values in place on a block written by gram_block with the same rows and range."""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        self._chk(self.lib.gkmhip_normalize_block(self.handle, rows.ctypes.data, len(rows), int(col_begin), int(col_end),
                                                  G_ptr, ld, sq_ptr, stream), "gkmhip_normalize_block")

    def explain_block(self, rows, col_begin, col_end, share, coef_ptr, xscale_ptr, out_ptr, stream=0):
        """Per-base importance of the queries [col_begin, col_end) against the support vectors `rows` into out_ptr (the
        bases of the range back to back): share = d + 1 host doubles, coef_ptr = len(rows) device doubles, xscale_ptr =
        one device double per query or None (include/gkm_hip.h gkmhip_explain_block)."""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        share = np.ascontiguousarray(share, dtype=np.float64)
        if len(share) != self.d + 1:
            raise GkmError("explain_block: share needs d + 1 = %d values" % (self.d + 1))
        self._chk(self.lib.gkmhip_explain_block(self.handle, rows.ctypes.data, len(rows), int(col_begin), int(col_end),
                                                share.ctypes.data, coef_ptr, xscale_ptr, out_ptr, stream),
                  "gkmhip_explain_block")

    def ism_block(self, rows, col_begin, col_end, fold_u, fold_b, gcoef, coef_ptr, out_ptr, base_ptr=None, stream=0):
        """In-silico mutagenesis, support-vector side, of the queries [col_begin, col_end) against the support vectors
        `rows` into out_ptr (4 doubles per base of the range, columns A, C, G, T) and base_ptr (one double per query, or
        None): fold_u, fold_b, gcoef = d + 1 host doubles each, coef_ptr = len(rows) device doubles
        (include/gkm_hip.h gkmhip_ism_block)."""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        fold = [np.ascontiguousarray(v, dtype=np.float64) for v in (fold_u, fold_b, gcoef)]
        if any(len(v) != self.d + 1 for v in fold):
            raise GkmError("ism_block: fold_u, fold_b and gcoef need d + 1 = %d values each" % (self.d + 1))
        self._chk(self.lib.gkmhip_ism_block(self.handle, rows.ctypes.data, len(rows), int(col_begin), int(col_end),
                                            fold[0].ctypes.data, fold[1].ctypes.data, fold[2].ctypes.data, coef_ptr,
                                            out_ptr, base_ptr, stream), "gkmhip_ism_block")

    def ism_rbf_block(self, rows, col_begin, col_end, fold_u, fold_b, dual_ptr, sq_ptr, gx_ptr, ld, ysq_ptr, out_ptr,
                      base_ptr=None, stream=0):
        """Every single-base mutant's RBF decision sum for the queries [col_begin, col_end) against the support vectors
        `rows` into out_ptr (4 doubles per base of the range, columns A, C, G, T; 0.0 at the query's own base) and
        base_ptr (one double per query, or None): fold_u, fold_b = d + 1 host doubles each, dual_ptr = len(rows) device
        doubles, sq_ptr = the norms of every uploaded sequence, gx_ptr = gram_block's raw values of the same rows and
        range with leading dimension ld, ysq_ptr = 4 device doubles per base, the mutants' norms (include/gkm_hip.h
        gkmhip_ism_rbf_block).  Kernel types 3 and 5 only."""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        fold = [np.ascontiguousarray(v, dtype=np.float64) for v in (fold_u, fold_b)]
        if any(len(v) != self.d + 1 for v in fold):
            raise GkmError("ism_rbf_block: fold_u and fold_b need d + 1 = %d values each" % (self.d + 1))
        self._chk(self.lib.gkmhip_ism_rbf_block(self.handle, rows.ctypes.data, len(rows), int(col_begin), int(col_end),
                                                fold[0].ctypes.data, fold[1].ctypes.data, dual_ptr, sq_ptr, gx_ptr,
                                                int(ld), ysq_ptr, out_ptr, base_ptr, stream), "gkmhip_ism_rbf_block")

    def hyp_block(self, rows, col_begin, col_end, share, coef_ptr, out_ptr, stream=0):
        """Raw hypothetical importance of the queries [col_begin, col_end) against the support vectors `rows` into
        out_ptr (4 doubles per base of the range, columns A, C, G, T): share = d + 1 host doubles, coef_ptr = len(rows)
        device doubles (include/gkm_hip.h gkmhip_hyp_block)."""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        share = np.ascontiguousarray(share, dtype=np.float64)
        if len(share) != self.d + 1:
            raise GkmError("hyp_block: share needs d + 1 = %d values" % (self.d + 1))
        self._chk(self.lib.gkmhip_hyp_block(self.handle, rows.ctypes.data, len(rows), int(col_begin), int(col_end),
                                            share.ctypes.data, coef_ptr, out_ptr, stream), "gkmhip_hyp_block")

    def ism_self_profiles(self, col_begin, col_end, prof_ptr, stream=0):
        """P_m(y, y) of every single-base mutant y of the queries [col_begin, col_end) into prof_ptr (int64, 4 (d + 1) per
        base of the range; include/gkm_hip.h gkmhip_ism_self_profiles)."""
        self._chk(self.lib.gkmhip_ism_self_profiles(self.handle, int(col_begin), int(col_end), prof_ptr, stream),
                  "gkmhip_ism_self_profiles")

    def self_profiles(self, col_begin, col_end, pself_ptr, stream=0):
        """The exact P_m(x, x) of the uploaded sequences [col_begin, col_end) into pself_ptr (int64, d + 1 per sequence;
        include/gkm_hip.h gkmhip_self_profiles)."""
        self._chk(self.lib.gkmhip_self_profiles(self.handle, int(col_begin), int(col_end), pself_ptr, stream),
                  "gkmhip_self_profiles")

    def lmer_weights(self, c, v_ptr, cv_ptr, nv, u_begin, u_end, W_ptr, stream=0):
        """L-mer weights W[u - u_begin] for the codes [u_begin, u_end) from nv canonical classes (v_ptr: device uint32
        codes, cv_ptr: device doubles) into W_ptr: c = d + 1 host doubles (include/gkm_hip.h gkmhip_lmer_weights)."""
        c = np.ascontiguousarray(c, dtype=np.float64)
        if len(c) != self.d + 1:
            raise GkmError("lmer_weights: c needs d + 1 = %d values" % (self.d + 1))
        if not 0 <= int(u_begin) < int(u_end) <= 4 ** self.L:
            raise GkmError("lmer_weights: the code range must satisfy 0 <= u_begin < u_end <= 4^L")
        if int(nv) < 0:
            raise GkmError("lmer_weights: nv must not be negative")
        self._chk(self.lib.gkmhip_lmer_weights(self.handle, c.ctypes.data, v_ptr, cv_ptr, int(nv), int(u_begin), int(u_end),
                                               W_ptr, stream), "gkmhip_lmer_weights")

    def lmer_score(self, col_begin, col_end, W_ptr, out_ptr, stream=0):
        """sum_p w_j[p] W[code(u_p)] of the uploaded sequences [col_begin, col_end) into out_ptr: W_ptr = 4^L device
        doubles indexed by code (include/gkm_hip.h gkmhip_lmer_score)."""
        self._chk(self.lib.gkmhip_lmer_score(self.handle, int(col_begin), int(col_end), W_ptr, out_ptr, stream),
                  "gkmhip_lmer_score")

    def lmer_importance(self, share, v_ptr, cv_ptr, nv, u_begin, u_end, V_ptr, stream=0):
        """Per-base importance V[(u - u_begin) L + i] for the codes [u_begin, u_end) from nv canonical classes (v_ptr:
        device uint32 codes, cv_ptr: device doubles) into V_ptr: share = d + 1 host doubles (include/gkm_hip.h
        gkmhip_lmer_importance)."""
        share = np.ascontiguousarray(share, dtype=np.float64)
        if len(share) != self.d + 1:
            raise GkmError("lmer_importance: share needs d + 1 = %d values" % (self.d + 1))
        if not 0 <= int(u_begin) < int(u_end) <= 4 ** self.L:
            raise GkmError("lmer_importance: the code range must satisfy 0 <= u_begin < u_end <= 4^L")
        if int(nv) < 0:
            raise GkmError("lmer_importance: nv must not be negative")
        self._chk(self.lib.gkmhip_lmer_importance(self.handle, share.ctypes.data, v_ptr, cv_ptr, int(nv), int(u_begin),
                                                  int(u_end), V_ptr, stream), "gkmhip_lmer_importance")

    def lmer_explain(self, col_begin, col_end, V_ptr, xscale_ptr, E_ptr, stream=0):
        """xscale_j sum_i w_j[t-i] V[code(u_{t-i})][i] for every base t of the uploaded sequences [col_begin, col_end)
        into E_ptr (the bases of the range back to back): V_ptr = 4^L x L device doubles, xscale_ptr = one device double
        per sequence (include/gkm_hip.h gkmhip_lmer_explain)."""
        self._chk(self.lib.gkmhip_lmer_explain(self.handle, int(col_begin), int(col_end), V_ptr, xscale_ptr, E_ptr,
                                               stream), "gkmhip_lmer_explain")

    def lmer_hyp(self, col_begin, col_end, V_ptr, R_ptr, stream=0):
        """The same sum, unscaled, with base t set to each of A, C, G, T into R_ptr (4 doubles per base of the range;
        include/gkm_hip.h gkmhip_lmer_hyp)."""
        self._chk(self.lib.gkmhip_lmer_hyp(self.handle, int(col_begin), int(col_end), V_ptr, R_ptr, stream),
                  "gkmhip_lmer_hyp")

    def scan_lmers(self, codes_ptr, valid_ptr, nbases, lm_ptr, stream=0):
        """One word per forward l-mer of `nbases` device base codes into lm_ptr (nbases - L + 1 uint32): the code, bit 31
        set where the l-mer covers a base whose valid byte is 0 (include/gkm_hip.h gkmhip_scan_lmers)."""
        self._chk(self.lib.gkmhip_scan_lmers(self.handle, codes_ptr, valid_ptr, int(nbases), lm_ptr, stream),
                  "gkmhip_scan_lmers")

    def scan_profiles(self, lm_ptr, nlm, wt_ptr, width, stride, nwin, prof_ptr, stream=0):
        """The exact self profiles of `nwin` windows of `width` bases at `stride`, the first at lm_ptr, into prof_ptr
        (int64, d + 1 per window): wt_ptr = width - L + 1 device bytes (include/gkm_hip.h gkmhip_scan_profiles)."""
        self._chk(self.lib.gkmhip_scan_profiles(self.handle, lm_ptr, int(nlm), wt_ptr, int(width), int(stride), int(nwin),
                                                prof_ptr, stream), "gkmhip_scan_profiles")

    def scan_score(self, lm_ptr, nlm, wt_ptr, width, stride, nwin, W_ptr, out_ptr, stream=0):
        """sum_p wt[p] W[l-mer p of the window] of the same windows into out_ptr (include/gkm_hip.h gkmhip_scan_score)."""
        self._chk(self.lib.gkmhip_scan_score(self.handle, lm_ptr, int(nlm), wt_ptr, int(width), int(stride), int(nwin),
                                             W_ptr, out_ptr, stream), "gkmhip_scan_score")

    def scan_group(self, width, stride):
        """Windows per stretch of k_scan_profiles for (L, width, stride); 0 where the scan refuses them."""
        return self.lib.gkmhip_scan_group(self.handle, int(width), int(stride))

    def _need_wsim(self):
        if not hasattr(self.lib, "gkmhip_wsim_profiles"):
            raise GkmError("%s holds no gkmhip_wsim_profiles: it was built before the window-pair calls" % lib_path())

    def wsim_profiles(self, lmx_ptr, nlmx, lmy_ptr, nlmy, width, stride_x, stride_y, nwx, nwy, G_ptr, ld, prof_ptr=None,
                      stream=0):
        """The raw kernel values of nwx windows of x by nwy windows of y, `width` bases each at the two strides, into
        G_ptr (doubles, leading dimension ld), and their exact profiles into prof_ptr (int32, nwx x nwy x (d + 1)) unless
        it is None: lmx_ptr, lmy_ptr the words of scan_lmers from the first window on (include/gkm_hip.h
        gkmhip_wsim_profiles)."""
        self._need_wsim()
        self._chk(self.lib.gkmhip_wsim_profiles(self.handle, lmx_ptr, int(nlmx), lmy_ptr, int(nlmy), int(width),
                                                int(stride_x), int(stride_y), int(nwx), int(nwy), G_ptr, int(ld), prof_ptr,
                                                stream), "gkmhip_wsim_profiles")

    def wsim_normalize(self, G_ptr, ld, nwx, nwy, sqx_ptr, sqy_ptr, stream=0):
        """In place G / (sqx[i] sqy[j]), RBF contexts exp(gamma (K - 1)); no unit diagonal (gkmhip_wsim_normalize)."""
        self._need_wsim()
        self._chk(self.lib.gkmhip_wsim_normalize(self.handle, G_ptr, int(ld), int(nwx), int(nwy), sqx_ptr, sqy_ptr, stream),
                  "gkmhip_wsim_normalize")

    def wsim_best(self, K_ptr, ld, nwx, nwy, start_x, stride_x, start_y, stride_y, min_separation, best_j_ptr, best_k_ptr,
                  stream=0):
        """Per row the eligible column with the largest K (the lower one on a tie) into best_j_ptr (int64, -1: none) and
        its value into best_k_ptr (NaN: none); eligible: not a NaN, and the two windows' starts at least min_separation
        bases apart (gkmhip_wsim_best)."""
        self._need_wsim()
        self._chk(self.lib.gkmhip_wsim_best(self.handle, K_ptr, int(ld), int(nwx), int(nwy), int(start_x), int(stride_x),
                                            int(start_y), int(stride_y), int(min_separation), best_j_ptr, best_k_ptr,
                                            stream), "gkmhip_wsim_best")

    def wsim_group(self, width, stride_x, stride_y):
        """(gx, gy): the windows of a tile of k_wsim_profiles for this context's (L, d); (0, 0) where refused."""
        return wsim_group(self.L, self.d, width, stride_x, stride_y)

    def _need_walign(self):
        if not hasattr(self.lib, "gkmhip_walign_block"):
            raise GkmError("%s holds no gkmhip_walign_block: it was built before the window-alignment calls" % lib_path())

    def walign_block(self, K_ptr, ld, nwx, nwy, flip, offset, gap, top_ptr, left_ptr, corner_ptr, D_ptr, ldd, best_h_ptr,
                     best_ic_ptr, scratch_ptr, scratch_bytes, stream=0):
        """The local-alignment DP over one block of K in DP coordinates (column c reads K[i ld + nwy - 1 - c] with flip):
        top (nwy doubles) and left (nwx doubles) are read as the cells beyond the block's edges and overwritten in place with
        its last row and column, corner is H(-1, -1); D (uint8 [nwx][ldd]) may be None; best_h (one double) and best_ic (two
        int64) receive the block's best cell (gkmhip_walign_block)."""
        self._need_walign()
        self._chk(self.lib.gkmhip_walign_block(self.handle, K_ptr, int(ld), int(nwx), int(nwy), int(bool(flip)), float(offset),
                                               float(gap), top_ptr, left_ptr, corner_ptr, D_ptr, int(ldd), best_h_ptr,
                                               best_ic_ptr, scratch_ptr, int(scratch_bytes), stream), "gkmhip_walign_block")

    def walign_trace(self, D_ptr, ldd, nwx, nwy, end_i, end_c, path_ptr, capacity, count_ptr, stream=0):
        """Walks D back from (end_i, end_c): the DIAG cells as (i, c) int32 pairs into path, end first; count: three int64,
        the pairs and the cell at which the walk stopped (gkmhip_walign_trace)."""
        self._need_walign()
        self._chk(self.lib.gkmhip_walign_trace(self.handle, D_ptr, int(ldd), int(nwx), int(nwy), int(end_i), int(end_c),
                                               path_ptr, int(capacity), count_ptr, stream), "gkmhip_walign_trace")

    def walign_tile(self):
        """(rows, columns) of a DP tile of k_walign_tiles."""
        return walign_tile()

    def walign_scratch_bytes(self, nwx, nwy):
        return walign_scratch_bytes(nwx, nwy)

    def _need_regions(self):
        if not hasattr(self.lib, "gkmhip_regions_count"):
            raise GkmError("%s holds no gkmhip_regions_count: it was built before the region calls" % lib_path())

    def regions_scratch_bytes(self, nlm, nwin):
        """Device bytes regions_count and regions_fill need for nwin windows over nlm l-mer words; -1 where refused."""
        self._need_regions()
        return self.lib.gkmhip_regions_scratch_bytes(int(nlm), int(nwin))

    def regions_span(self):
        """Windows one workgroup of the region kernels owns."""
        self._need_regions()
        return self.lib.gkmhip_regions_span()

    def regions_count(self, score_ptr, ld, lm_ptr, nlm, width, stride, nwin, threshold, gap, scratch_ptr, scratch_bytes,
                      stream=0):
        """-> the regions among the nwin windows of a scan launch whose finished scores are score_ptr[i * ld] (device
        doubles): runs of windows without a flagged word and with a score >= threshold, at most `gap` others between two
        of them (include/gkm_hip.h gkmhip_regions_count).  Waits for the stream."""
        self._need_regions()
        count = ctypes.c_int64(-1)
        self._chk(self.lib.gkmhip_regions_count(self.handle, score_ptr, int(ld), lm_ptr, int(nlm), int(width), int(stride),
                                                int(nwin), float(threshold), int(gap), scratch_ptr, int(scratch_bytes),
                                                ctypes.addressof(count), stream), "gkmhip_regions_count")
        return count.value

    def regions_fill(self, score_ptr, ld, lm_ptr, nlm, width, stride, nwin, threshold, gap, scratch_ptr, scratch_bytes,
                     capacity, first_ptr, last_ptr, summit_ptr, windows_ptr, peak_ptr, stream=0):
        """After regions_count with the same arguments and scratch: the regions' first, last and summit windows and window
        counts (int32) and peaks (float64) into device arrays of `capacity` elements (gkmhip_regions_fill)."""
        self._need_regions()
        self._chk(self.lib.gkmhip_regions_fill(self.handle, score_ptr, int(ld), lm_ptr, int(nlm), int(width), int(stride),
                                               int(nwin), float(threshold), int(gap), scratch_ptr, int(scratch_bytes),
                                               int(capacity), first_ptr, last_ptr, summit_ptr, windows_ptr, peak_ptr,
                                               stream), "gkmhip_regions_fill")

    def _need_dist(self):
        if not hasattr(self.lib, "gkmhip_dist_digits"):
            raise GkmError("%s holds no gkmhip_dist_digits: it was built before the distribution calls" % lib_path())

    def dist_digit_bits(self):
        """B, the key bits one refinement level resolves (include/gkm_hip.h gkmhip_dist_digit_bits)."""
        self._need_dist()
        return self.lib.gkmhip_dist_digit_bits()

    def dist_scratch_bytes(self, nlm, nwin):
        """Device bytes each dist call needs for nwin windows over nlm l-mer words; -1 where refused."""
        self._need_dist()
        return self.lib.gkmhip_dist_scratch_bytes(int(nlm), int(nwin))

    @staticmethod
    def _prefix_array(prefix):
        """the HOST prefixes of a dist call -> (the contiguous uint64 array, held until the C call returns, its pointer)"""
        prefix = np.ascontiguousarray(prefix, dtype=np.uint64).reshape(-1)
        return prefix, (prefix.ctypes.data if len(prefix) else None)

    def dist_digits(self, score_ptr, ld, lm_ptr, nlm, width, stride, nwin, prefix, prefix_bits, hist_ptr, scratch_ptr,
                    scratch_bytes, stream=0):
        """Adds the scored windows of a scan launch (finished scores score_ptr[i * ld], device doubles) to the device
        uint64 histogram at hist_ptr by the next digit of their keys: prefix, a HOST sequence of up to 64 strictly
        ascending values of prefix_bits bits, selects the windows and the histogram's row; an empty one is level 0
        (include/gkm_hip.h gkmhip_dist_digits).  Does not wait."""
        self._need_dist()
        prefix, pptr = self._prefix_array(prefix)
        self._chk(self.lib.gkmhip_dist_digits(self.handle, score_ptr, int(ld), lm_ptr, int(nlm), int(width), int(stride),
                                              int(nwin), pptr, len(prefix), int(prefix_bits), hist_ptr, scratch_ptr,
                                              int(scratch_bytes), stream), "gkmhip_dist_digits")

    def dist_edges(self, score_ptr, ld, lm_ptr, nlm, width, stride, nwin, edges_ptr, nedges, hist_ptr, scratch_ptr,
                   scratch_bytes, stream=0):
        """Adds the scored windows to the nedges + 1 device uint64 counters at hist_ptr, a score v at the number of
        edges <= v: edges_ptr = nedges ascending device doubles (gkmhip_dist_edges).  Does not wait."""
        self._need_dist()
        self._chk(self.lib.gkmhip_dist_edges(self.handle, score_ptr, int(ld), lm_ptr, int(nlm), int(width), int(stride),
                                             int(nwin), edges_ptr, int(nedges), hist_ptr, scratch_ptr, int(scratch_bytes),
                                             stream), "gkmhip_dist_edges")

    def dist_collect(self, score_ptr, ld, lm_ptr, nlm, width, stride, nwin, prefix, prefix_bits, out_ptr, capacity,
                     counter_ptr, scratch_ptr, scratch_bytes, stream=0):
        """Appends the scores of the scored windows whose keys begin with one of the HOST prefixes to the device doubles
        at out_ptr, from the device int64 at counter_ptr on, which advances by the matches; positions >= capacity are
        dropped (gkmhip_dist_collect).  Does not wait."""
        self._need_dist()
        prefix, pptr = self._prefix_array(prefix)
        self._chk(self.lib.gkmhip_dist_collect(self.handle, score_ptr, int(ld), lm_ptr, int(nlm), int(width), int(stride),
                                               int(nwin), pptr, len(prefix), int(prefix_bits), out_ptr, int(capacity),
                                               counter_ptr, scratch_ptr, int(scratch_bytes), stream),
                  "gkmhip_dist_collect")

    def delta_sat(self, lm_ptr, nlm, t_begin, t_end, W_ptr, out_ptr, stream=0):
        """Every SNV of the positions [t_begin, t_end) of the bases the nlm words at lm_ptr cover -> out_ptr, (t_end -
        t_begin) x 4 doubles: the change in the summed W of the l-mers over the position (include/gkm_hip.h
        gkmhip_delta_sat)."""
        self._chk(self.lib.gkmhip_delta_sat(self.handle, lm_ptr, int(nlm), int(t_begin), int(t_end), W_ptr, out_ptr, stream),
                  "gkmhip_delta_sat")

    def delta_variants(self, lm_ptr, codes_ptr, nbases, var, alt, W_ptr, out_ptr, stream=0):
        """One delta per row (pos, ref_len, alt_off, alt_len) of the HOST int32 array var, alt the HOST uint8 array of all
        alternate bases; lm_ptr / codes_ptr: the device words and codes of the nbases bases (include/gkm_hip.h
        gkmhip_delta_variants)."""
        var, alt, args = self._variant_arrays(var, alt)
        self._chk(self.lib.gkmhip_delta_variants(self.handle, lm_ptr, codes_ptr, int(nbases), *args, W_ptr, out_ptr, stream),
                  "gkmhip_delta_variants")

    @staticmethod
    def _variant_arrays(var, alt):
        """The host arrays of a variant launch -> (var, alt, args): the contiguous int32 (n, 4) and uint8 arrays, which the
        caller holds until the C call returns, and (var pointer, nvar, alt pointer or None, nalt) as the entries take
        them."""
        var = np.ascontiguousarray(var, dtype=np.int32).reshape(-1, 4)
        alt = np.ascontiguousarray(alt, dtype=np.uint8)
        return var, alt, (var.ctypes.data, len(var), alt.ctypes.data if len(alt) else None, len(alt))

    # l-mer weight panels (include/gkm_hip.h; gkm_panel.hip, gkm_delta.hip): P_ptr = 4^L rows of `ms` device doubles, the
    # first `nm` of a row the models' weights; the model index is the last axis of every output
    def panel_score(self, col_begin, col_end, P_ptr, nm, ms, out_ptr, stream=0):
        """lmer_score for every model of a panel -> out_ptr, (col_end - col_begin) x nm doubles (gkmhip_panel_score)."""
        self._chk(self.lib.gkmhip_panel_score(self.handle, int(col_begin), int(col_end), P_ptr, int(nm), int(ms), out_ptr,
                                              stream), "gkmhip_panel_score")

    def panel_scan_score(self, lm_ptr, nlm, wt_ptr, width, stride, nwin, P_ptr, nm, ms, out_ptr, stream=0):
        """scan_score for every model of a panel -> out_ptr, nwin x nm doubles (gkmhip_panel_scan_score)."""
        self._chk(self.lib.gkmhip_panel_scan_score(self.handle, lm_ptr, int(nlm), wt_ptr, int(width), int(stride), int(nwin),
                                                   P_ptr, int(nm), int(ms), out_ptr, stream), "gkmhip_panel_scan_score")

    def panel_delta_sat(self, lm_ptr, nlm, t_begin, t_end, P_ptr, nm, ms, out_ptr, stream=0):
        """delta_sat for every model of a panel -> out_ptr, (t_end - t_begin) x 4 x nm doubles (gkmhip_panel_delta_sat)."""
        self._chk(self.lib.gkmhip_panel_delta_sat(self.handle, lm_ptr, int(nlm), int(t_begin), int(t_end), P_ptr, int(nm),
                                                  int(ms), out_ptr, stream), "gkmhip_panel_delta_sat")

    def panel_delta_variants(self, lm_ptr, codes_ptr, nbases, var, alt, P_ptr, nm, ms, out_ptr, stream=0):
        """delta_variants for every model of a panel -> out_ptr, len(var) x nm doubles (gkmhip_panel_delta_variants)."""
        var, alt, args = self._variant_arrays(var, alt)
        self._chk(self.lib.gkmhip_panel_delta_variants(self.handle, lm_ptr, codes_ptr, int(nbases), *args, P_ptr, int(nm),
                                                       int(ms), out_ptr, stream), "gkmhip_panel_delta_variants")

    def panel_weights(self, c, v_ptr, CV_ptr, nv, nm, ms, u_begin, u_end, P_ptr, stream=0):
        """lmer_weights for every model of a panel in one pass -> P_ptr, (u_end - u_begin) rows of ms device doubles (the
        panel's device image; columns nm.. come back +0.0): nv classes (v_ptr: device uint32 codes) with CV_ptr = nv rows
        of ms device doubles, CV[i, m] class i's coefficient for model m; c = d + 1 host doubles (include/gkm_hip.h
        gkmhip_panel_weights)."""
        if not hasattr(self.lib, "gkmhip_panel_weights"):
            raise GkmError("panel_weights: this build of the library has no gkmhip_panel_weights")
        c = np.ascontiguousarray(c, dtype=np.float64)
        if len(c) != self.d + 1:
            raise GkmError("panel_weights: c needs d + 1 = %d values" % (self.d + 1))
        if not 0 <= int(u_begin) < int(u_end) <= 4 ** self.L:
            raise GkmError("panel_weights: the code range must satisfy 0 <= u_begin < u_end <= 4^L")
        if int(nv) < 0:
            raise GkmError("panel_weights: nv must not be negative")
        self._chk(self.lib.gkmhip_panel_weights(self.handle, c.ctypes.data, v_ptr, CV_ptr, int(nv), int(nm), int(ms),
                                                int(u_begin), int(u_end), P_ptr, stream), "gkmhip_panel_weights")

    # windows of position weights contracted with a table or a panel (include/gkm_hip.h; gkm_contract.hip): P_ptr = nwin x L x 4
    # device doubles
    def lmer_contract(self, W_ptr, P_ptr, nwin, out_ptr, stream=0):
        """a(P) of every window against the table at W_ptr (4^L device doubles) -> out_ptr, nwin doubles
        (gkmhip_lmer_contract)."""
        self._chk(_contract_lib().gkmhip_lmer_contract(self.handle, W_ptr, P_ptr, int(nwin), out_ptr, stream),
                  "gkmhip_lmer_contract")

    def panel_contract(self, rows_ptr, nm, ms, P_ptr, nwin, out_ptr, ld, stream=0):
        """lmer_contract for every model of a panel -> out_ptr, nwin x ld doubles of which the first nm of a row are
        written (gkmhip_panel_contract)."""
        self._chk(_contract_lib().gkmhip_panel_contract(self.handle, rows_ptr, int(nm), int(ms), P_ptr, int(nwin), out_ptr,
                                                        int(ld), stream), "gkmhip_panel_contract")

    def self_norms(self, sq_ptr, stream=0):
        self._chk(self.lib.gkmhip_self_norms(self.handle, sq_ptr, stream), "gkmhip_self_norms")

    def normalize_rows_full(self, rows, G_ptr, ld, sq_ptr, local_rows=True, stream=0):
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        self._chk(self.lib.gkmhip_normalize_rows_full(self.handle, rows.ctypes.data, len(rows), int(local_rows), G_ptr,
                                                      ld, sq_ptr, stream), "gkmhip_normalize_rows_full")

    def normalize(self, G_ptr, ld, sq_ptr=None, symmetric=False, stream=0):
        self._chk(self.lib.gkmhip_normalize(self.handle, G_ptr, ld, sq_ptr, int(symmetric), stream),
                  "gkmhip_normalize")

    def assemble_normalize(self, slabs_ptr, lds, slot_ptr, K_ptr, ld, sq_ptr, symmetric=False, stream=0):
        """Un-permute (matrix row a = row slot[a] of the gathered slabs; with lds == 1 slot[a] is the element offset
        at which row a starts: packed slabs) + normalise in one pass."""
        self._chk(self.lib.gkmhip_assemble_normalize(self.handle, slabs_ptr, lds, slot_ptr, K_ptr, ld, sq_ptr,
                                                     int(symmetric), stream), "gkmhip_assemble_normalize")

    def copy_lower_to_rows(self, K_ptr, ld, n, host, nthreads=1):
        """host[a, :a + 1] = K[a, :a + 1] for the n rows of a device matrix with leading dimension ld, through the pinned
        staging pipeline; nothing else of `host` is written (include/gkm_hip.h gkmhip_copy_lower_to_rows).  The copies
        run on a stream of the call's own: K must be complete."""
        rows = _row_pointers(host, n)
        self._chk(self.lib.gkmhip_copy_lower_to_rows(self.handle, K_ptr, int(ld), int(n), rows.ctypes.data, int(nthreads)),
                  "gkmhip_copy_lower_to_rows")

    def gram_to_host_rows(self, G_ptr, ld, host, nthreads=1, part=0, nparts=1):
        """The whole normalised matrix of the uploaded sequences into host[a, :a + 1], G_ptr = device scratch of n x ld
        doubles; nparts > 1: only the row blocks of context `part` of `nparts` (include/gkm_hip.h
        gkmhip_gram_to_host_rows / gkmhip_gram_part_to_host_rows)."""
        rows = _row_pointers(host, self.n)
        if nparts == 1 and part == 0:
            self._chk(self.lib.gkmhip_gram_to_host_rows(self.handle, G_ptr, int(ld), rows.ctypes.data, int(nthreads)),
                      "gkmhip_gram_to_host_rows")
        else:
            self._chk(self.lib.gkmhip_gram_part_to_host_rows(self.handle, G_ptr, int(ld), rows.ctypes.data, int(nthreads),
                                                             int(part), int(nparts)), "gkmhip_gram_part_to_host_rows")

    def last_kernel_ms(self):
        return self.lib.gkmhip_last_kernel_ms(self.handle)

    def kernel_timeline(self, on):
        """While on, every launch keeps its own event pair: kernel_timeline_ms() sums the Gram kernels of a loop."""
        self._chk(self.lib.gkmhip_kernel_timeline(self.handle, 1 if on else 0), "gkmhip_kernel_timeline")

    def kernel_timeline_ms(self):
        k = ctypes.c_int(0)
        ms = self.lib.gkmhip_kernel_timeline_ms(self.handle, ctypes.byref(k))
        return ms, k.value

    def last_comparisons(self):
        return self.lib.gkmhip_last_comparisons(self.handle)

    def last_kernel_name(self):
        return self.lib.gkmhip_last_kernel_name(self.handle).decode()

    def last_riders(self):
        """Rows the most recent Gram launch carried as riders (bit rows 30, 31 of the same-length variant's lanes), 0 if none."""
        return int(self.lib.gkmhip_last_riders(self.handle)) if hasattr(self.lib, "gkmhip_last_riders") else 0

    def last_variant(self):
        """k_gram_bitslice's variant (its PK) of the most recent Gram launch: 1, 2 several pieces per lane, 4 / 5 same length
        with group records (5: riders), 6 / 7 the same with shift records; 0 for k_gram_direct."""
        return int(self.lib.gkmhip_last_variant(self.handle)) if hasattr(self.lib, "gkmhip_last_variant") else 0


def cross_kernel(seqs, rows, kernel_type, L, k, d, M=50, H=50.0, gamma=1.0, device=0, kernel=KERNEL_AUTO):
    """K(rows[i], j) for every sequence j (prediction-style rectangular kernel): torch fp64
    [len(rows), n] with 1.0 where j == rows[i], plus the self norms."""
    import torch
    ctx = GramContext(kernel_type, L, k, d, M, H, gamma, device)
    try:
        ctx.set_kernel(kernel)
        dev = torch.device("cuda", device)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            ctx.set_sequences(seqs, stream)
            n = len(seqs)
            rows = np.ascontiguousarray(sorted(rows), dtype=np.int32)
            G = torch.zeros((len(rows), n), dtype=torch.float64, device=dev)
            sq = torch.zeros(n, dtype=torch.float64, device=dev)
            ctx.self_norms(sq.data_ptr(), stream)
            ctx.gram_rows_full(rows, G.data_ptr(), n, True, stream)
            ctx.normalize_rows_full(rows, G.data_ptr(), n, sq.data_ptr(), True, stream)
            torch.cuda.synchronize(dev)
            return dict(K=G, sqnorm=sq, rows=rows, kernel=ctx.last_kernel_name(), variant=ctx.last_variant())
    finally:
        ctx.close()


# ------------------------------------------------------------------ the genome window index (no context)
NULLIDX_MAX_WIDTH = 2047
NULLIDX_NOKEY = 0xFFFFFFFF


def nullidx_tile():
    """Windows per workgroup of k_nullidx_keys (include/gkm_hip.h gkmhip_nullidx_tile)."""
    return load().gkmhip_nullidx_tile()


def nullidx_check(T, width):
    """Raise for what the index refuses: a width outside 1..2047, 2^31 - 1 bytes or more."""
    if not 1 <= int(width) <= NULLIDX_MAX_WIDTH:
        raise GkmError("the window width must lie in 1..%d, not %d" % (NULLIDX_MAX_WIDTH, int(width)))
    if int(T) >= 2 ** 31 - 1:
        raise GkmError("a record of %d bytes is too long for the index (fewer than 2^31 - 1)" % int(T))


def nullidx_build(raw, width, device=0, times=None):
    """The window index of one chromosome on the GPU (include/gkm_hip.h gkmhip_nullidx_*).

    raw: the record's FASTA letters, uint8, case kept, no line breaks; width: the window width t.
    Returns dict(key=uint32 [max(0, T - t)] (NULLIDX_NOKEY where the window holds an N), pos=int32 [len], ptr=int32
    [t + 1, t + 1], len=int, na / cg / rp = uint8 [(T + 7) // 8], numpy.packbits' layout).
    times: a dict that receives the seconds of upload, keys, cells, sort and download, each ended by a synchronise."""
    import time
    import torch
    L = load()
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    T, t = len(raw), int(width)
    nullidx_check(T, t)
    nwin, cells, nb = max(0, T - t), (t + 1) ** 2, (T + 7) // 8
    if T == 0:
        z = np.zeros(0, np.uint8)
        return dict(key=np.zeros(0, np.uint32), pos=np.zeros(0, np.int32), ptr=np.zeros((t + 1, t + 1), np.int32), len=0,
                    na=z, cg=z.copy(), rp=z.copy())
    dev = torch.device("cuda", device)

    def chk(rc, what):
        if rc:
            raise GkmError("%s failed (%d): %s" % (what, rc, L.gkmhip_last_error().decode()))

    def lap(name, t0):
        if times is not None:
            torch.cuda.current_stream().synchronize()
            times[name] = times.get(name, 0.0) + time.perf_counter() - t0
        return time.perf_counter()

    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        t0 = time.perf_counter()
        d_seq = torch.from_numpy(raw if raw.flags.writeable else raw.copy()).to(dev)
        t0 = lap("upload", t0)
        nbp = (nb + 7) // 8 * 8     # (every plane starts 8-byte aligned)
        d_planes = torch.empty((3, nbp), dtype=torch.uint8, device=dev)
        d_key = torch.empty(max(nwin, 1), dtype=torch.int32, device=dev)
        d_pos = torch.empty(max(nwin, 1), dtype=torch.int32, device=dev)
        d_ptr = torch.empty(cells + 1, dtype=torch.int32, device=dev)
        sbytes = L.gkmhip_nullidx_scratch_bytes(T, t)
        if sbytes < 0:
            raise GkmError("gkmhip_nullidx_scratch_bytes: " + L.gkmhip_last_error().decode())
        d_scratch = torch.empty(sbytes, dtype=torch.uint8, device=dev)
        t0 = lap("allocate", t0)
        chk(L.gkmhip_nullidx_keys(device, d_seq.data_ptr(), T, t, d_key.data_ptr(), d_planes[0].data_ptr(),
                                  d_planes[1].data_ptr(), d_planes[2].data_ptr(), stream), "gkmhip_nullidx_keys")
        t0 = lap("keys", t0)
        chk(L.gkmhip_nullidx_cells(device, d_key.data_ptr(), T, t, d_ptr.data_ptr(), d_scratch.data_ptr(), sbytes, stream),
            "gkmhip_nullidx_cells")
        t0 = lap("cells", t0)
        chk(L.gkmhip_nullidx_sort(device, d_key.data_ptr(), T, t, d_pos.data_ptr(), d_scratch.data_ptr(), sbytes, stream),
            "gkmhip_nullidx_sort")
        t0 = lap("sort", t0)
        ptr = d_ptr.cpu().numpy()
        n = int(ptr[cells])
        planes = d_planes[:, :nb].cpu().numpy()
        out = dict(key=d_key[:nwin].cpu().numpy().view(np.uint32), pos=d_pos[:n].cpu().numpy(),
                   ptr=ptr[:cells].reshape(t + 1, t + 1).copy(), len=n,
                   na=np.ascontiguousarray(planes[0]), cg=np.ascontiguousarray(planes[1]),
                   rp=np.ascontiguousarray(planes[2]))
        lap("download", t0)
        return out


_CTX_CACHE = {}
_CTX_CACHE_LOCK = __import__("threading").Lock()   # init_many's workers insert and release concurrently


def cached_context(kernel_type, L, k, d, M=50, H=50.0, gamma=1.0, device=0, slot=0):
    """One long-lived GramContext per (device, parameters).  Destroying a context frees device memory,
    which waits for EVERYTHING on the device (hipFree): a caller that evaluates subset after subset
    with the cross-validation of the previous one still running on another stream (gkmsvm.init_many)
    keeps its context instead, re-uploads the next subset's sequences into the same buffers and so
    never blocks on the other stream.  `slot` tells apart callers that work on the same device at the same time
    (gkmsvm.init_many with one worker per entry of `gpus`)."""
    key = (device, slot, kernel_type, L, k, d, int(M), float(H), float(gamma))
    with _CTX_CACHE_LOCK:
        ctx = _CTX_CACHE.get(key)
        if ctx is None or not ctx.handle:
            ctx = _CTX_CACHE[key] = GramContext(kernel_type, L, k, d, M, H, gamma, device)
    return ctx


def release_cached_contexts(device=None, slot=None):
    """Close the cached contexts (all of them, or those of one device / slot): each keeps its device scratch --
    the tile-transposed output alone is ~0.6 GB at n = 10 000 -- for as long as it lives."""
    with _CTX_CACHE_LOCK:
        gone = [_CTX_CACHE.pop(key) for key in list(_CTX_CACHE)
                if (device is None or key[0] == device) and (slot is None or key[1] == slot)]
    for ctx in gone:     # (hipFree waits for the device: outside the lock)
        ctx.close()


def gram_matrix(seqs, kernel_type, L, k, d, M=50, H=50.0, gamma=1.0, device=0, want_profiles=False,
                kernel=KERNEL_AUTO, symmetric=False, keep_context=False, context_slot=0, wait=True):
    """Whole Gram matrix of `seqs` on one GPU (device memory through torch).

    Returns dict(K=torch fp64 [n,n] (lower triangle + unit diagonal; upper too if symmetric),
    P=int32 [n,n,d+1] or None, sqnorm=[n], kernel=name, riders / variant=GramContext.last_riders() / last_variant() of
    the launch, ms=device ms of the gram kernel).
    keep_context: use (and keep) the cached context of these parameters, see cached_context().
    wait=False (with keep_context): return as soon as the work is enqueued on torch's current stream -- whatever the
    caller enqueues on that stream next is ordered behind it, and the host is free meanwhile (gkmsvm.init draws the
    cross-validation folds while the Gram kernel runs); `ms` is then None."""
    import torch
    ctx = (cached_context(kernel_type, L, k, d, M, H, gamma, device, context_slot) if keep_context
           else GramContext(kernel_type, L, k, d, M, H, gamma, device))
    try:
        ctx.set_kernel(kernel)
        dev = torch.device("cuda", device)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            ctx.set_sequences(seqs, stream)
            n = len(seqs)
            G = torch.zeros((n, n), dtype=torch.float64, device=dev)
            P = torch.zeros((n, n, d + 1), dtype=torch.int32, device=dev) if want_profiles else None
            sq = torch.zeros(n, dtype=torch.float64, device=dev)
            ctx.gram_rows(np.arange(n), G.data_ptr(), n, P.data_ptr() if want_profiles else None, n, False, stream)
            riders, variant = ctx.last_riders(), ctx.last_variant()
            ctx.normalize(G.data_ptr(), n, sq.data_ptr(), symmetric, stream)
            if not (keep_context and not wait):
                torch.cuda.current_stream().synchronize()   # (this stream only: others may carry unrelated work)
            return dict(K=G, P=P, sqnorm=sq, kernel=ctx.last_kernel_name(), riders=riders, variant=variant,
                        ms=ctx.last_kernel_ms() if (wait or not keep_context) else None,
                        comparisons=ctx.last_comparisons())
    finally:
        if not keep_context:
            ctx.close()


def allgather_stats():
    """Per-rank HIP-event timings of the most recent gkmhip_gram_allgather (include/gkm_hip.h)."""
    buf = np.zeros(3 + 4 * 64)
    got = load().gkmhip_allgather_stats(buf.ctypes.data, len(buf))
    if not got:
        return None
    G = int(buf[0])
    per = buf[3:3 + 4 * G].reshape(G, 4)
    return dict(ranks=G, chunks=int(buf[1]), transport=("none", "p2p", "rccl")[int(buf[2])],
                kernel_ms=per[:, 0].tolist(), transfer_ms=per[:, 1].tolist(), assemble_ms=per[:, 2].tolist(),
                comparisons=per[:, 3].tolist())


def gram_matrix_multi(seqs, kernel_type, L, k, d, M=50, H=50.0, gamma=1.0, devices=(0,), symmetric=False, chunks=0,
                      kernel=KERNEL_AUTO, ld=None, out=None):
    """Whole Gram matrix computed on several GPUs by ONE process (include/gkm_hip.h,
    gkmhip_gram_allgather): rows sharded by folded row blocks, slabs all-gathered over xGMI (RCCL),
    every device ends up with the whole normalised matrix -- bit-identical to gram_matrix().
    `devices` may name a device more than once (rehearsal on a one-GPU box: peer copies instead of RCCL).
    ld: the leading dimension of every device's matrix (default n); out: the matrices to write, one fp64 [n, ld] tensor
    per entry of devices on that device (default: zeroed ones) -- columns n..ld-1 are left as they are.

    Returns dict(K=[torch fp64 [n,ld] per entry of devices], transport="rccl"|"p2p"|"none", ms=wall)."""
    import time
    import torch
    lib = load()
    ctxs = []
    try:
        for dv in devices:
            c = GramContext(kernel_type, L, k, d, M, H, gamma, dv)
            c.set_kernel(kernel)
            ctxs.append(c)
        n = len(seqs)
        ld = n if ld is None else int(ld)
        if out is not None and (len(out) != len(devices) or any(
                K.dtype != torch.float64 or tuple(K.shape) != (n, ld) or not K.is_contiguous() or K.device.index != dv
                for K, dv in zip(out, devices))):
            raise GkmError("out needs one contiguous fp64 [n, ld] tensor per entry of devices, on that device")
        Ks = []
        for g, (c, dv) in enumerate(zip(ctxs, devices)):
            with torch.cuda.device(dv):
                c.set_sequences(seqs, torch.cuda.current_stream().cuda_stream)
                Ks.append(out[g] if out is not None
                          else torch.zeros((n, max(ld, 0)), dtype=torch.float64, device=torch.device("cuda", dv)))
        for dv in set(devices):
            torch.cuda.synchronize(dv)
        handles = (ctypes.c_void_p * len(ctxs))(*[c.handle for c in ctxs])
        outs = (ctypes.c_void_p * len(ctxs))(*[K.data_ptr() for K in Ks])
        t0 = time.perf_counter()
        rc = lib.gkmhip_gram_allgather(handles, len(ctxs), outs, ld, int(symmetric), int(chunks))
        wall = time.perf_counter() - t0
        if rc:
            raise GkmError("gkmhip_gram_allgather failed (%d): %s" % (rc, lib.gkmhip_last_error().decode()))
        return dict(K=Ks, transport=lib.gkmhip_last_transport().decode(), ms=wall * 1e3)
    finally:
        for c in ctxs:
            c.close()
