"""ctypes binding of include/malva_hip.h.  No fallback: a missing or unloadable
libmalva_hip.so is an error.

One HIP runtime per process.  libmalva_hip.so asks the loader for `libamdhip64.so.7` and gets whichever copy is
already mapped, else /opt/rocm's.  PyTorch-ROCm bundles its own copy and asks for it by FILE name
(`libamdhip64.so`), which never matches an already mapped /opt/rocm copy: a process that mapped /opt/rocm's first
and imports torch later ends up with two runtimes, and torch then reports "No HIP GPUs".  lib() therefore maps
torch's copy first whenever torch is installed (without importing torch), so the order of `import torch` and
Context() no longer matters.  MALVA_HIP_RUNTIME=system keeps /opt/rocm's (for processes that never import torch)."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np

BF_ALT, BF_CTX = 0, 1
MG_ERR_ARG = -1
MG_MAX_KMER = 128
MAX_ROW = (MG_MAX_KMER + 1 + 7) // 8 * 8   # 136: MG_MAX_KMER bytes + NUL, rounded to 8 (the stride the command line uses)
STREAM_DEFAULT = 1          # MG_STREAM_DEFAULT: HIP's legacy default stream (a NULL handle means the context's own stream)
COMM_NONE, COMM_RCCL, COMM_LOCAL = 0, 1, 2
COMM_ID_BYTES = 128
LD_MAX_GROUPS, LD_MAX_WINDOW = 256, 1024   # MG_LD_MAX_GROUPS, MG_LD_MAX_WINDOW
IBD_MAX_SAMPLES = 16384     # MG_IBD_MAX_SAMPLES
GRM_MAX_SAMPLES, GRM_SHIFT, GRM_MAX_Q = 16384, 10, 32639   # MG_GRM_MAX_SAMPLES, MG_GRM_SHIFT, MG_GRM_MAX_Q
PCA_MAX_N, PCA_MAX_K = 16384, 32   # MG_PCA_MAX_N, MG_PCA_MAX_K
IBD_SEG = np.dtype([(f, np.uint32) for f in ("a", "b", "chrom", "start_pos", "end_pos", "n", "ibs2", "zero")])   # mg_ibd_seg, 32 bytes
LD_PAIR = np.dtype([("i", np.uint32), ("j", np.uint32), ("n", np.uint32), ("sign", np.int32), ("r2", np.float64)])   # mg_ld_pair, 24 bytes
SAMPLE_SLOTS = 32           # MG_SAMPLE_SLOTS: the counters per plane of mg_sample_counts (MG_SS_*)
GT_NORMAL, GT_OVERCOV, GT_SINGLE, GT_NOCOV = 0, 1, 2, 3

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class MalvaError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("malva_hip error %d: %s" % (code, msg))
        self.code = code


def library_path():
    return os.path.join(_HERE, "lib", "libmalva_hip.so")


def _map_process_hip_runtime():
    """see the module docstring; returns the path mapped, or None"""
    if os.environ.get("MALVA_HIP_RUNTIME", "") == "system" or "torch" in sys.modules:
        return None                      # torch already imported: its runtime is mapped and ours will bind to it
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return None
    path = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if not os.path.exists(path):
        return None
    C.CDLL(path, mode=C.RTLD_GLOBAL)
    return path


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise MalvaError(-100, "%s not built: run `make lib` (hipcc --offload-arch=gfx950)" % path)
    _map_process_hip_runtime()
    L = C.CDLL(path)
    vp, cp, sz, u64, u32, i32, i64 = C.c_void_p, C.c_char_p, C.c_size_t, C.c_uint64, C.c_uint32, C.c_int32, C.c_int64
    fl, it = C.c_float, C.c_int
    sig = {
        "mg_create": [C.POINTER(vp), it, u32, u32, u64],
        "mg_destroy": [vp],
        "mg_set_stream": [vp, vp],
        "mg_synchronize": [vp],
        "mg_bf_insert": [vp, it, vp, sz, sz],
        "mg_bf_test": [vp, it, vp, sz, sz, vp],
        "mg_bf_finalize": [vp, it],
        "mg_bf_increment": [vp, it, vp, sz, sz, vp],
        "mg_bf_get_count": [vp, it, vp, sz, sz, vp],
        "mg_bf_info": [vp, it, vp, vp, vp],
        "mg_map_insert": [vp, vp, sz, sz],
        "mg_map_test": [vp, vp, sz, sz, vp],
        "mg_map_increment": [vp, vp, sz, sz, vp],
        "mg_map_get_count": [vp, vp, sz, sz, vp],
        "mg_map_size": [vp, vp],
        "mg_ref_scan": [vp, vp, sz],
        "mg_ref_scan_resident": [vp, u64, sz],
        "mg_reference_upload_device": [vp, vp, sz],
        "mg_kmc_scan": [vp, vp, vp, vp, sz],
        "mg_kmc_scan_device": [vp, vp, vp, vp, sz],
        "mg_kmc_pack_rows_device": [vp, vp, vp, vp, sz, vp],
        "mg_kmc_scan_rows_device": [vp, vp, sz],
        "mg_host_alloc": [C.POINTER(vp), sz],
        "mg_host_free": [vp],
        "mg_kmc_set_lut": [vp, vp, sz, u32, u32, u32, u32, u64, u64],
        "mg_reads_begin": [vp, u32, u32, u32, u32],
        "mg_reads_add": [vp, vp, sz],
        "mg_reads_add_device": [vp, vp, sz],
        "mg_reads_finish": [vp, vp],
        "mg_reads_export": [vp, vp, vp, vp, sz, vp],
        "mg_reads_stats": [vp, vp, vp],
        "mg_kmc_scan_records": [vp, vp, sz, u64],
        "mg_kmc_decode_records": [vp, vp, sz, u64, vp, vp, vp],
        "mg_counters_size": [vp, vp, vp],
        "mg_counters_export_device": [vp, vp],
        "mg_counters_import_device": [vp, vp],
        "mg_counters_reset": [vp],
        "mg_counters_view": [vp, vp, vp, vp],
        "mg_cohort_begin": [vp, u32],
        "mg_cohort_select": [vp, u32],
        "mg_cohort_end": [vp],
        "mg_cohort_info": [vp, vp, vp],
        "mg_cover_blocks_cohort_device": [vp, vp, vp, vp, vp, it, vp, vp],
        "mg_cohort_stats": [vp, vp],
        "mg_format_calls": [vp, C.POINTER(Cells), vp, sz, vp, vp],          # (typed: anything but a Cells or None is an ArgumentError, not a wild pointer)
        "mg_format_calls_device": [vp, C.POINTER(Cells), vp, sz, vp, vp],
        "mg_format_stats": [vp, vp],
        "mg_site_counts": [vp, sz, u32, it, vp, vp, vp, it, i32, vp, it, vp, vp],
        "mg_site_counts_device": [vp, sz, u32, it, vp, vp, vp, it, i32, vp, it, vp, vp],
        "mg_format_site_info": [vp, sz, vp, vp, vp, vp, sz, vp, vp],
        "mg_format_site_info_device": [vp, sz, vp, vp, vp, vp, sz, vp, vp],
        "mg_site_stats": [vp, vp],
        "mg_pack_dosage": [vp, sz, u32, it, vp, vp, vp, it, i32, vp, vp],
        "mg_pack_dosage_device": [vp, sz, u32, it, vp, vp, vp, it, i32, vp, vp],
        "mg_pair_counts": [vp, sz, vp, u32, vp, u32, it, vp],
        "mg_pair_counts_device": [vp, sz, vp, u32, vp, u32, it, vp],
        "mg_pairs_stats": [vp, vp],
        "mg_sample_counts": [vp, sz, u32, it, vp, vp, vp, it, i32, vp, vp, vp, vp, it, vp],
        "mg_sample_counts_device": [vp, sz, u32, it, vp, vp, vp, it, i32, vp, vp, vp, vp, it, vp],
        "mg_sample_stats": [vp, vp],
        "mg_site_geno_counts": [vp, sz, u32, it, vp, vp, vp, it, i32, vp, it, vp, vp, vp],
        "mg_site_geno_counts_device": [vp, sz, u32, it, vp, vp, vp, it, i32, vp, it, vp, vp, vp],
        "mg_hwe_exact": [vp, sz, vp, vp, vp, vp, vp],
        "mg_hwe_exact_device": [vp, sz, vp, vp, vp, vp, vp],
        "mg_hwe_stats": [vp, vp],
        "mg_pack_site_dosage": [vp, sz, u32, it, vp, vp, vp, it, i32, vp, vp],
        "mg_pack_site_dosage_device": [vp, sz, u32, it, vp, vp, vp, it, i32, vp, vp],
        "mg_ld_window": [vp, sz, sz, u32, vp, vp, vp, u32, C.c_uint64, u32, C.c_double, vp, sz, vp, vp],
        "mg_ld_window_device": [vp, sz, sz, u32, vp, vp, vp, u32, C.c_uint64, u32, C.c_double, vp, sz, vp, vp],
        "mg_ld_stats": [vp, vp],
        "mg_sites_to_planes": [vp, sz, u32, vp, vp],
        "mg_sites_to_planes_device": [vp, sz, u32, vp, vp],
        "mg_ibd_begin": [vp, u32, u32, C.c_uint64],
        "mg_ibd_step": [vp, sz, u32, vp, vp, vp, it, vp, sz, vp],
        "mg_ibd_step_device": [vp, sz, u32, vp, vp, vp, it, vp, sz, vp],
        "mg_ibd_end": [vp],
        "mg_ibd_stats": [vp, vp],
        "mg_grm_weights": [vp, sz, u32, u32, vp, it, u32, u32, vp],
        "mg_grm_weights_device": [vp, sz, u32, u32, vp, it, u32, u32, vp],
        "mg_grm_begin": [vp, u32, it, u32, u32],
        "mg_grm_step": [vp, sz, u32, vp],
        "mg_grm_step_device": [vp, sz, u32, vp],
        "mg_grm_read": [vp, vp, vp, vp],
        "mg_grm_end": [vp],
        "mg_grm_stats": [vp, vp],
        "mg_pca_load_tri_f32": [vp, u32, vp],
        "mg_pca_load_f64": [vp, u32, vp],
        "mg_pca_load_tri_f32_device": [vp, u32, vp],
        "mg_pca_load_f64_device": [vp, u32, vp],
        "mg_pca_solve": [vp, u32, C.c_double, u32, vp, vp, vp, vp, vp],
        "mg_pca_solve_device": [vp, u32, C.c_double, u32, vp, vp, vp, vp, vp],
        "mg_pca_end": [vp],
        "mg_pca_stats": [vp, vp],
        "mg_genotype_cohort": [vp, sz, u32, vp, vp, vp, fl, it, it, u32, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp],
        "mg_genotype_cohort_device": [vp, sz, u32, vp, vp, vp, fl, it, it, u32, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp],
        "mg_cohort_prior_stats": [vp, vp],
        "mg_estimate_priors": [vp, sz, u32, vp, vp, vp, fl, it, it, u32, C.c_double, vp, vp],
        "mg_estimate_priors_device": [vp, sz, u32, vp, vp, vp, fl, it, it, u32, C.c_double, vp, vp],
        "mg_estimate_priors_stats": [vp, vp],
        "mg_encode_calls_bcf": [vp, C.POINTER(Cells), C.POINTER(BcfKeys), vp, sz, vp, vp],
        "mg_encode_calls_bcf_device": [vp, C.POINTER(Cells), C.POINTER(BcfKeys), vp, sz, vp, vp],
        "mg_bcf_stats": [vp, vp],
        "mg_phred_likelihoods": [vp, sz, u32, vp, vp, vp, fl, it, it, i32, vp],
        "mg_phred_likelihoods_device": [vp, sz, u32, vp, vp, vp, fl, it, it, i32, vp],
        "mg_pl_stats": [vp, vp],
        "mg_cover_blocks_cohort": [vp, C.POINTER(BlocksHost), it, vp, vp],
        "mg_comm_unique_id": [vp],
        "mg_comm_init": [vp, it, it, vp],
        "mg_comm_init_all": [C.POINTER(vp), it],
        "mg_comm_destroy": [vp],
        "mg_comm_info": [vp, vp, vp, vp],
        "mg_counters_allreduce": [vp],
        "mg_counters_allreduce_all": [C.POINTER(vp), it],
        "mg_counters_allreduce_begin": [vp],
        "mg_counters_allreduce_end": [vp],
        "mg_exchange_stats": [vp, vp, vp],
        "mg_lookup_cover": [vp, vp, sz, sz, vp, vp, sz, vp, sz, vp],
        "mg_genotype": [vp, vp, vp, vp, sz, fl, it, it, vp, vp, vp, vp, vp, vp],
        "mg_cover_blocks": [vp, C.POINTER(BlocksHost), it, vp, vp],
        "mg_decode_gt_text": [vp, vp, sz, sz, vp, vp, vp, u32, vp, it, vp, vp, vp, vp, vp],
        "mg_decode_gt_entries": [vp, vp, vp],
        "mg_cut_blocks": [vp, sz, vp, vp, vp, vp, vp, vp],
        "mg_cut_blocks_device": [vp, vp, vp, vp, vp],
        "mg_cover_blocks_device": [vp, vp, vp, vp, vp, it, vp, vp],
        "mg_index_blocks_device": [vp, vp, vp, vp, vp, it, vp],
        "mg_genotype_device": [vp, vp, vp, vp, sz, fl, it, it, vp, vp, vp, vp, vp, vp],
        "mg_index_isolated": [vp, sz, vp, vp, vp, vp, sz, vp, vp, vp],
        "mg_index_blocks": [vp, C.POINTER(BlocksHost), it, vp],
        "mg_reference_upload": [vp, vp, sz],
        "mg_call_isolated": [vp, sz, vp, vp, vp, vp, sz, vp, vp, vp, fl, it, it, vp, vp, vp, vp, vp, vp, vp],
        "mg_call_isolated_device": [vp, sz, vp, vp, vp, vp, vp, vp, vp, fl, it, it, vp, vp, vp, vp, vp, vp, vp],
        "mg_bf_export": [vp, it, vp, vp],
        "mg_bf_import": [vp, it, it, u64, vp, vp, u64],
        "mg_bf_export_sparse": [vp, it, vp, vp],
        "mg_bf_import_sparse": [vp, it, it, u64, vp, vp, u64],
        "mg_map_export": [vp, vp, sz, vp],
        "mg_map_import": [vp, vp, sz, sz, vp],
        "mg_debug_bf_index": [vp, it, vp, sz, sz, vp],
        "mg_debug_packed_index": [vp, it, vp, vp, sz, u32, vp],
        "mg_debug_tile_scan": [vp, vp, u64, vp],
        "mg_debug_row_scan": [vp, vp, u64, it, vp, vp],
        "mg_debug_bucket_count": [vp, vp, u64, vp, vp],
        "mg_scan_stats": [vp, vp, vp],
        "mg_blocks_stats": [vp, vp, vp],
        "mg_set_option": [vp, cp, i64],
        "mg_get_option": [vp, cp, C.POINTER(C.c_int64)],
    }
    for name, args in sig.items():
        f = getattr(L, name)          # AttributeError if the library lacks a declared symbol
        f.argtypes = args
        f.restype = C.c_int
    L.mg_kmc_rows_bytes.argtypes = [sz]
    L.mg_kmc_rows_bytes.restype = C.c_size_t
    L.mg_last_error.argtypes = [vp]
    L.mg_last_error.restype = cp
    _LIB = L
    return L


EXPORTED = ["mg_create", "mg_destroy", "mg_last_error", "mg_set_stream", "mg_synchronize", "mg_bf_insert", "mg_bf_test",
            "mg_bf_finalize", "mg_bf_increment", "mg_bf_get_count", "mg_bf_info", "mg_map_insert", "mg_map_test",
            "mg_map_increment", "mg_map_get_count", "mg_map_size", "mg_ref_scan", "mg_ref_scan_resident", "mg_reference_upload_device", "mg_kmc_scan", "mg_kmc_scan_device", "mg_kmc_rows_bytes", "mg_kmc_pack_rows_device", "mg_kmc_scan_rows_device",
            "mg_host_alloc", "mg_host_free", "mg_kmc_set_lut", "mg_kmc_scan_records", "mg_kmc_decode_records",
            "mg_reads_begin", "mg_reads_add", "mg_reads_add_device", "mg_reads_finish", "mg_reads_export", "mg_reads_stats",
            "mg_counters_size", "mg_counters_export_device", "mg_counters_import_device", "mg_counters_reset", "mg_counters_view",
            "mg_cohort_begin", "mg_cohort_select", "mg_cohort_end", "mg_cohort_info", "mg_cover_blocks_cohort_device", "mg_cohort_stats", "mg_cover_blocks_cohort",
            "mg_format_calls", "mg_format_calls_device", "mg_format_stats",
            "mg_site_counts", "mg_site_counts_device", "mg_format_site_info",
            "mg_format_site_info_device", "mg_site_stats", "mg_pack_dosage", "mg_pack_dosage_device", "mg_pair_counts", "mg_pair_counts_device",
            "mg_pairs_stats", "mg_sample_counts", "mg_sample_counts_device", "mg_sample_stats",
            "mg_site_geno_counts", "mg_site_geno_counts_device", "mg_hwe_exact", "mg_hwe_exact_device", "mg_hwe_stats",
            "mg_pack_site_dosage", "mg_pack_site_dosage_device", "mg_ld_window", "mg_ld_window_device", "mg_ld_stats",
            "mg_sites_to_planes", "mg_sites_to_planes_device", "mg_ibd_begin", "mg_ibd_step", "mg_ibd_step_device", "mg_ibd_end", "mg_ibd_stats",
            "mg_grm_weights", "mg_grm_weights_device", "mg_grm_begin", "mg_grm_step", "mg_grm_step_device", "mg_grm_read", "mg_grm_end", "mg_grm_stats",
            "mg_pca_load_tri_f32", "mg_pca_load_f64", "mg_pca_load_tri_f32_device", "mg_pca_load_f64_device", "mg_pca_solve", "mg_pca_solve_device", "mg_pca_end", "mg_pca_stats",
            "mg_genotype_cohort", "mg_genotype_cohort_device", "mg_cohort_prior_stats", "mg_estimate_priors", "mg_estimate_priors_device", "mg_estimate_priors_stats", "mg_encode_calls_bcf", "mg_encode_calls_bcf_device", "mg_bcf_stats",
            "mg_phred_likelihoods", "mg_phred_likelihoods_device", "mg_pl_stats",
            "mg_comm_unique_id", "mg_comm_init", "mg_comm_init_all", "mg_comm_destroy", "mg_comm_info", "mg_counters_allreduce",
            "mg_counters_allreduce_all", "mg_counters_allreduce_begin", "mg_counters_allreduce_end", "mg_exchange_stats", "mg_decode_gt_text", "mg_decode_gt_entries", "mg_cut_blocks", "mg_cut_blocks_device", "mg_cover_blocks_device", "mg_index_blocks_device", "mg_genotype_device",
            "mg_index_isolated",
            "mg_lookup_cover", "mg_cover_blocks", "mg_index_blocks", "mg_genotype", "mg_reference_upload", "mg_call_isolated", "mg_call_isolated_device",
            "mg_bf_export", "mg_bf_import", "mg_bf_export_sparse", "mg_bf_import_sparse", "mg_map_export", "mg_map_import", "mg_debug_bf_index",
            "mg_debug_packed_index", "mg_debug_tile_scan", "mg_debug_row_scan", "mg_debug_bucket_count", "mg_scan_stats", "mg_blocks_stats", "mg_set_option", "mg_get_option"]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class PanelDev(C.Structure):
    """mg_panel_dev: a panel resident in HBM (every pointer a device pointer)"""
    _fields_ = [("n_vars", C.c_uint64), ("n_contigs", C.c_uint32), ("n_samples", C.c_uint32), ("contig_base", C.c_void_p), ("contig_len", C.c_void_p),
                ("contig_id", C.c_void_p), ("pos", C.c_void_p), ("ref_size", C.c_void_p), ("min_size", C.c_void_p), ("present", C.c_void_p),
                ("var_allele_off", C.c_void_p), ("allele_off", C.c_void_p), ("pool", C.c_void_p), ("canon", C.c_void_p), ("gt", C.c_void_p),
                ("sp_off", C.c_void_p), ("sp_sample", C.c_void_p), ("sp_gt", C.c_void_p), ("sp_default", C.c_uint32), ("pool_bytes", C.c_uint64)]


CELLS_GP, CELLS_PL = 1, 2    # MG_CELLS_GP, MG_CELLS_PL


class Cells(C.Structure):
    """mg_cells: a batch's cells for mg_format_calls* / mg_encode_calls_bcf* (host pointers in a host form, device pointers in a device form)"""
    _fields_ = [("n_vars", C.c_size_t), ("n_planes", C.c_uint32), ("haploid", C.c_int), ("gt1", C.c_void_p), ("gt2", C.c_void_p), ("gq", C.c_void_p),
                ("use_mask", C.c_int), ("min_gq", C.c_int32), ("cov", C.c_void_p), ("var_allele_off", C.c_void_p), ("probs", C.c_void_p),
                ("var_gt_off", C.c_void_p), ("status", C.c_void_p), ("pl", C.c_void_p), ("allele_class", C.c_void_p), ("fields", C.c_uint32)]


class BlocksHost(C.Structure):
    """mg_blocks_host: a batch of blocks in host memory for mg_cover_blocks, mg_cover_blocks_cohort and mg_index_blocks (every pointer a host pointer)"""
    _fields_ = [("n_blocks", C.c_size_t), ("blk_ref_base", C.c_void_p), ("blk_ref_len", C.c_void_p), ("blk_var_off", C.c_void_p),
                ("n_vars", C.c_size_t), ("pos", C.c_void_p), ("ref_size", C.c_void_p), ("min_size", C.c_void_p), ("present", C.c_void_p),
                ("var_allele_off", C.c_void_p), ("allele_off", C.c_void_p), ("pool", C.c_void_p), ("pool_len", C.c_size_t), ("canon", C.c_void_p),
                ("n_samples", C.c_uint32), ("gt", C.c_void_p), ("sp_off", C.c_void_p), ("sp_sample", C.c_void_p), ("sp_gt", C.c_void_p),
                ("sp_default", C.c_uint16)]


class BcfKeys(C.Structure):
    """mg_bcf_keys: the header's dictionary indexes of the FORMAT fields"""
    _fields_ = [("gt", C.c_int32), ("gq", C.c_int32), ("cov", C.c_int32), ("gp", C.c_int32), ("pl", C.c_int32)]


def _pl_fields(gp):
    """the field bits of a PL call, with GP in front of PL or without"""
    return CELLS_PL | (CELLS_GP if gp else 0)


def _bcf_keys(keys):
    """(gt, gq, cov[, gp[, pl]]) -> BcfKeys, what is not given 0"""
    return BcfKeys(*[int(k) for k in keys])


def sparse_genotypes(gt, n_samples, default=1 << 14):
    """dense [n_vars, n_samples] genotype words -> (sp_off, sp_sample, sp_gt): the entries other than `default` (0|0 phased)"""
    gt = np.ascontiguousarray(gt, dtype=np.uint16).reshape(-1, max(int(n_samples), 1)) if n_samples else np.zeros((len(gt), 0), np.uint16)
    keep = gt != np.uint16(default)
    off = np.zeros(gt.shape[0] + 1, dtype=np.uint32)
    off[1:] = np.cumsum(keep.sum(axis=1))
    rows, cols = np.nonzero(keep)
    return off, cols.astype(np.uint32), gt[rows, cols].astype(np.uint16)


def _blocks_host(blk_ref_base, blk_ref_len, blk_var_off, pos, ref_size, min_size, present, var_allele_off, allele_off, pool, canon, gt, n_samples,
                 sparse, sp_default):
    """the arrays of a host batch of blocks as numpy arrays of the ABI's types -> BlocksHost (which keeps the arrays it points into alive).
    sparse: the genotypes as the entries other than the word sp_default (sparse_genotypes), and no `gt`"""
    types = (np.uint64, np.uint32, np.uint32, np.int32, np.uint32, np.uint32, np.uint8, np.uint8, np.uint32, np.uint32, np.uint8, np.uint16)
    given = (blk_ref_base, blk_ref_len, blk_var_off, pos, ref_size, min_size, present, canon, var_allele_off, allele_off, pool, gt)
    bb, bl, bo, pos, rs, ms, pr, canon, vo, ao, pool, gt = arrays = [np.ascontiguousarray(g, dtype=t) for g, t in zip(given, types)]
    n = len(pos)
    x = BlocksHost(n_blocks=len(bb), blk_ref_base=_p(bb), blk_ref_len=_p(bl), blk_var_off=_p(bo), n_vars=n, pos=_p(pos), ref_size=_p(rs), min_size=_p(ms),
                   present=_p(pr), var_allele_off=_p(vo), allele_off=_p(ao), pool=_p(pool), pool_len=pool.size, canon=_p(canon), n_samples=n_samples,
                   sp_default=sp_default)
    if sparse:
        arrays += sparse_genotypes(gt.reshape(n, -1) if n else gt, n_samples, sp_default)
        x.sp_off, x.sp_sample, x.sp_gt = (_p(q) for q in arrays[-3:])
    else:
        x.gt = _p(gt)
    x.arrays = arrays
    return x


def host_alloc(n_bytes):
    """pinned host memory (mg_host_alloc) as a uint8 array; the array must be passed to host_free() when done"""
    ptr = C.c_void_p()
    rc = lib().mg_host_alloc(C.byref(ptr), n_bytes)
    if rc != 0:
        raise MalvaError(rc, "mg_host_alloc(%d) failed" % n_bytes)
    arr = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n_bytes,))
    return arr, ptr


def host_free(ptr):
    lib().mg_host_free(ptr)


def comm_unique_id() -> bytes:
    """ncclGetUniqueId through the library: rank 0 calls it and ships the bytes to the other ranks"""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = lib().mg_comm_unique_id(buf)
    if rc != 0:
        raise MalvaError(rc, "mg_comm_unique_id failed (librccl.so.1 not loadable?)")
    return buf.raw


def _ctx_array(ctxs):
    arr = (C.c_void_p * len(ctxs))(*[c.h for c in ctxs])
    return arr


def comm_init_all(ctxs):
    """one process, several contexts: one per device (RCCL group) or all on one device (kernel sum)"""
    rc = lib().mg_comm_init_all(_ctx_array(ctxs), len(ctxs))
    if rc != 0:
        raise MalvaError(rc, lib().mg_last_error(ctxs[0].h).decode())


def counters_allreduce_all(ctxs):
    rc = lib().mg_counters_allreduce_all(_ctx_array(ctxs), len(ctxs))
    if rc != 0:
        raise MalvaError(rc, lib().mg_last_error(ctxs[0].h).decode())


def rows_of(kmers, stride=None):
    """list of bytes -> contiguous uint8 [n, stride], NUL padded"""
    n = len(kmers)
    if stride is None:
        stride = (max((len(k) for k in kmers), default=1) + 1 + 7) // 8 * 8
    arr = np.zeros((n, stride), dtype=np.uint8)
    for i, k in enumerate(kmers):
        if len(k) >= stride:
            raise ValueError("k-mer longer than the row stride")
        arr[i, : len(k)] = np.frombuffer(k, dtype=np.uint8)
    return arr


def _rows(rows):
    if isinstance(rows, (list, tuple)):
        rows = rows_of(rows)
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    assert rows.ndim == 2
    return rows


class Context:
    """One GPU's filters, exact map and kernels (mg_ctx)."""

    def __init__(self, k=35, ref_k=43, bf_bits=1 << 33, device=0):
        self._L = lib()
        self.h = C.c_void_p()
        rc = self._L.mg_create(C.byref(self.h), device, k, ref_k, bf_bits)
        if rc != 0:
            self.h = None
            raise MalvaError(rc, "mg_create failed (no usable HIP device, bad sizes or out of memory)")
        self.k, self.ref_k, self.bf_bits = k, ref_k, bf_bits

    def close(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            self._L.mg_destroy(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:      # interpreter shutdown: the library may already be gone
            pass

    def _ck(self, rc):
        if rc != 0:
            raise MalvaError(rc, self._L.mg_last_error(self.h).decode())

    # lifetime / options
    def set_stream(self, stream_handle):
        self._ck(self._L.mg_set_stream(self.h, C.c_void_p(stream_handle)))

    def synchronize(self):
        self._ck(self._L.mg_synchronize(self.h))

    def set_option(self, name, value):
        self._ck(self._L.mg_set_option(self.h, name.encode(), int(value)))

    def get_option(self, name):
        v = C.c_int64(0)
        self._ck(self._L.mg_get_option(self.h, name.encode(), C.byref(v)))
        return v.value

    # BF
    def bf_insert(self, which, rows):
        rows = _rows(rows)
        self._ck(self._L.mg_bf_insert(self.h, which, _p(rows), rows.shape[1], rows.shape[0]))

    def bf_test(self, which, rows):
        rows = _rows(rows)
        out = np.zeros(rows.shape[0], dtype=np.uint8)
        self._ck(self._L.mg_bf_test(self.h, which, _p(rows), rows.shape[1], rows.shape[0], _p(out)))
        return out.astype(bool)

    def bf_finalize(self, which):
        self._ck(self._L.mg_bf_finalize(self.h, which))

    def bf_increment(self, which, rows, counters):
        rows = _rows(rows)
        counters = np.ascontiguousarray(counters, dtype=np.uint32)
        assert counters.shape[0] == rows.shape[0]
        self._ck(self._L.mg_bf_increment(self.h, which, _p(rows), rows.shape[1], rows.shape[0], _p(counters)))

    def bf_get_count(self, which, rows):
        rows = _rows(rows)
        out = np.zeros(rows.shape[0], dtype=np.uint16)
        self._ck(self._L.mg_bf_get_count(self.h, which, _p(rows), rows.shape[1], rows.shape[0], _p(out)))
        return out

    def bf_info(self, which):
        size, nset, mode = C.c_uint64(), C.c_uint64(), C.c_int()
        self._ck(self._L.mg_bf_info(self.h, which, C.byref(size), C.byref(nset), C.byref(mode)))
        return size.value, nset.value, mode.value

    def bf_index(self, which, rows):
        rows = _rows(rows)
        out = np.zeros(rows.shape[0], dtype=np.uint64)
        self._ck(self._L.mg_debug_bf_index(self.h, which, _p(rows), rows.shape[1], rows.shape[0], _p(out)))
        return out

    def packed_index(self, which, hi, lo, klen):
        hi = np.ascontiguousarray(hi, dtype=np.uint64)
        lo = np.ascontiguousarray(lo, dtype=np.uint64)
        out = np.zeros(hi.shape[0], dtype=np.uint64)
        self._ck(self._L.mg_debug_packed_index(self.h, which, _p(hi), _p(lo), hi.shape[0], klen, _p(out)))
        return out

    def tile_scan(self, x):
        """finalize's scan of its tile sums on the caller's values: (exclusive prefix modulo 2^32, total)"""
        x = np.array(x, dtype=np.uint32)
        total = C.c_uint64()
        self._ck(self._L.mg_debug_tile_scan(self.h, _p(x) if x.size else None, x.size, C.byref(total)))
        return x, total.value

    def row_scan(self, length, flag=False):
        """the row encoders' scan on the caller's row lengths: (row_off [n + 1] uint64, total); flag: as behind a row of 4 GB or more"""
        length = np.ascontiguousarray(length, dtype=np.uint32)
        row_off = np.zeros(length.size + 1, dtype=np.uint64)
        total = C.c_uint64()
        self._ck(self._L.mg_debug_row_scan(self.h, _p(length) if length.size else None, length.size, int(flag), _p(row_off), C.byref(total)))
        return row_off, total.value

    def bucket_count(self, idx):
        """(rank or -1, u16 counter) of filter slots of `bf` as the call-time lookups read them from the records"""
        idx = np.ascontiguousarray(idx, dtype=np.uint64)
        rank = np.zeros(idx.size, dtype=np.int64)
        count = np.zeros(idx.size, dtype=np.uint32)
        self._ck(self._L.mg_debug_bucket_count(self.h, _p(idx), idx.size, _p(rank), _p(count)))
        return rank, count

    def bf_export(self, which):
        size, nset, mode = self.bf_info(which)
        words = np.zeros((size + 63) // 64, dtype=np.uint64)
        counts = np.zeros(nset if mode else 0, dtype=np.uint16)
        self._ck(self._L.mg_bf_export(self.h, which, _p(words), _p(counts) if counts.size else None))
        return mode, size, words, counts

    def bf_import(self, which, mode, size, words, counts):
        words = np.ascontiguousarray(words, dtype=np.uint64)
        counts = np.ascontiguousarray(counts, dtype=np.uint16)
        self._ck(self._L.mg_bf_import(self.h, which, int(mode), size, _p(words), _p(counts) if counts.size else None,
                                      counts.size))

    def bf_export_sparse(self, which):
        size, nset, mode = self.bf_info(which)
        pos = np.zeros(nset, dtype=np.uint64)
        counts = np.zeros(nset, dtype=np.uint16)
        self._ck(self._L.mg_bf_export_sparse(self.h, which, _p(pos) if nset else None, _p(counts) if nset else None))
        return mode, size, pos, counts

    def bf_import_sparse(self, which, mode, size, pos, counts):
        pos = np.ascontiguousarray(pos, dtype=np.uint64)
        counts = np.ascontiguousarray(counts, dtype=np.uint16)
        self._ck(self._L.mg_bf_import_sparse(self.h, which, int(mode), size, _p(pos) if pos.size else None,
                                             _p(counts) if counts.size else None, pos.size))

    # KMAP
    def map_insert(self, rows):
        rows = _rows(rows)
        self._ck(self._L.mg_map_insert(self.h, _p(rows), rows.shape[1], rows.shape[0]))

    def map_test(self, rows):
        rows = _rows(rows)
        out = np.zeros(rows.shape[0], dtype=np.uint8)
        self._ck(self._L.mg_map_test(self.h, _p(rows), rows.shape[1], rows.shape[0], _p(out)))
        return out.astype(bool)

    def map_increment(self, rows, counters):
        rows = _rows(rows)
        counters = np.ascontiguousarray(counters, dtype=np.int32)
        self._ck(self._L.mg_map_increment(self.h, _p(rows), rows.shape[1], rows.shape[0], _p(counters)))

    def map_get_count(self, rows):
        rows = _rows(rows)
        out = np.zeros(rows.shape[0], dtype=np.int32)
        self._ck(self._L.mg_map_get_count(self.h, _p(rows), rows.shape[1], rows.shape[0], _p(out)))
        return out

    def map_size(self):
        n = C.c_uint64()
        self._ck(self._L.mg_map_size(self.h, C.byref(n)))
        return n.value

    def map_export(self):
        n = self.map_size()
        vals = np.zeros(n, dtype=np.int32)
        stride = (self.k + 1 + 7) // 8 * 8
        rows = np.zeros((n, stride), dtype=np.uint8)
        rc = self._L.mg_map_export(self.h, _p(rows), stride, _p(vals)) if n else 0
        if rc == MG_ERR_ARG and stride < MAX_ROW:                # a key longer than k in the host's list: the widest row always fits
            rows = np.zeros((n, MAX_ROW), dtype=np.uint8)
            rc = self._L.mg_map_export(self.h, _p(rows), MAX_ROW, _p(vals))
        self._ck(rc)
        keys = [bytes(r).split(b"\0", 1)[0] for r in rows]
        return keys, vals

    def map_import(self, keys, vals):
        rows = _rows(keys)
        vals = np.ascontiguousarray(vals, dtype=np.int32)
        self._ck(self._L.mg_map_import(self.h, _p(rows), rows.shape[1], rows.shape[0], _p(vals)))

    # scans
    def ref_scan(self, contig):
        """contig: bytes, or a uint8 array (no copy: a whole-genome contig is gigabytes)"""
        buf = np.frombuffer(contig, dtype=np.uint8) if isinstance(contig, (bytes, bytearray, memoryview)) else np.ascontiguousarray(contig, dtype=np.uint8)
        self._ck(self._L.mg_ref_scan(self.h, _p(buf), buf.size))

    def ref_scan_resident(self, offset, length):
        """the contig at [offset, offset + length) of the uploaded reference (no PCIe)"""
        self._ck(self._L.mg_ref_scan_resident(self.h, int(offset), int(length)))

    def reference_upload_device(self, d_ptr, length):
        self._ck(self._L.mg_reference_upload_device(self.h, C.c_void_p(d_ptr), int(length)))

    def kmc_scan(self, hi, lo, cnt):
        hi = np.ascontiguousarray(hi, dtype=np.uint64)
        lo = np.ascontiguousarray(lo, dtype=np.uint64)
        cnt = np.ascontiguousarray(cnt, dtype=np.uint32)
        assert hi.shape == lo.shape == cnt.shape
        self._ck(self._L.mg_kmc_scan(self.h, _p(hi), _p(lo), _p(cnt), hi.shape[0]))

    def kmc_scan_device(self, d_hi, d_lo, d_cnt, n):
        self._ck(self._L.mg_kmc_scan_device(self.h, C.c_void_p(d_hi), C.c_void_p(d_lo), C.c_void_p(d_cnt), n))

    # KMC database feed
    def kmc_set_lut(self, lut, lut_prefix_len, suffix_bytes, counter_bytes, min_count, max_count, total_records):
        lut = np.ascontiguousarray(lut, dtype=np.uint64)
        self._ck(self._L.mg_kmc_set_lut(self.h, _p(lut), lut.size, lut_prefix_len, suffix_bytes, counter_bytes, min_count, max_count,
                                        total_records))
        self._kmc_rec = suffix_bytes + counter_bytes

    def kmc_scan_records(self, records, first_record=0):
        records = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1)
        assert records.size % self._kmc_rec == 0
        self._ck(self._L.mg_kmc_scan_records(self.h, _p(records), records.size // self._kmc_rec, first_record))

    def kmc_decode_records(self, records, first_record=0):
        records = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1)
        n = records.size // self._kmc_rec
        hi, lo, cnt = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
        self._ck(self._L.mg_kmc_decode_records(self.h, _p(records), n, first_record, _p(hi), _p(lo), _p(cnt)))
        return hi, lo, cnt

    # counting from reads (the KMC step, MALVA:104-110)
    def reads_begin(self, min_count=2, max_count=255, part=0, n_parts=1):
        self._ck(self._L.mg_reads_begin(self.h, min_count, max_count, part, n_parts))

    def reads_add(self, seq):
        """seq: bytes of whole records, a byte outside ACGT (newline) between two of them"""
        buf = np.frombuffer(bytes(seq), dtype=np.uint8)
        self._ck(self._L.mg_reads_add(self.h, _p(buf), buf.size))

    def reads_add_device(self, d_ptr, nbytes):
        self._ck(self._L.mg_reads_add_device(self.h, C.c_void_p(d_ptr), int(nbytes)))

    def reads_finish(self):
        """-> rows kept (count >= min) and scanned"""
        n = C.c_uint64(0)
        self._ck(self._L.mg_reads_finish(self.h, C.byref(n)))
        return n.value

    def reads_export(self, cap=None, with_total=False):
        """-> (hi, lo, cnt) of the kept rows, any order: all of them, or the first `cap`; with_total adds the library's
        count of all the kept rows"""
        n = C.c_uint64(0)
        if cap is None:
            self._ck(self._L.mg_reads_export(self.h, None, None, None, 0, C.byref(n)))
            cap = n.value
        hi, lo, cnt = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint32)
        self._ck(self._L.mg_reads_export(self.h, _p(hi), _p(lo), _p(cnt), cap, C.byref(n)))
        m = min(cap, n.value)
        out = (hi[:m], lo[:m], cnt[:m])
        return out + (n.value,) if with_total else out

    def reads_stats(self):
        """-> (ms: pack, window + filter, file, reduce, scan; counts: bases, windows, survivors, passes, kept)"""
        ms, cn = (C.c_float * 5)(), (C.c_uint64 * 5)()
        self._ck(self._L.mg_reads_stats(self.h, ms, cn))
        return list(ms), list(cn)

    def kmc_rows_bytes(self, n):
        return self._L.mg_kmc_rows_bytes(n)

    def kmc_pack_rows_device(self, d_hi, d_lo, d_cnt, n, d_rows_out):
        self._ck(self._L.mg_kmc_pack_rows_device(self.h, C.c_void_p(d_hi), C.c_void_p(d_lo), C.c_void_p(d_cnt), n, C.c_void_p(d_rows_out)))

    def kmc_scan_rows_device(self, d_rows, n):
        self._ck(self._L.mg_kmc_scan_rows_device(self.h, C.c_void_p(d_rows), n))

    def scan_stats(self):
        """-> (filter ms, probe ms, hits ms, open rows, bf-hit rows)"""
        ms = (C.c_float * 3)()
        nr = (C.c_uint64 * 2)()
        self._ck(self._L.mg_scan_stats(self.h, ms, nr))
        return float(ms[0]), float(ms[1]), float(ms[2]), int(nr[0]), int(nr[1])

    def blocks_stats(self):
        """-> (tier 1 ms, tier 2 ms, tier 3 ms, records beyond tier 1, lone signature k-mers, general signature k-mers, records tier 3 took)"""
        ms = (C.c_float * 3)()
        nr = (C.c_uint64 * 4)()
        self._ck(self._L.mg_blocks_stats(self.h, ms, nr))
        return float(ms[0]), float(ms[1]), float(ms[2]), int(nr[0]), int(nr[1]), int(nr[2]), int(nr[3])

    # counters exchange
    def decode_gt_text(self, text, span_off, span_len, gt_index, n_columns, keep=None, haploid=False):
        """-> (sp_default, sp_off, sp_sample, sp_gt, raw_mask, max_allele): the panel genotypes of a batch of records from
        the text of their sample columns (mg_decode_gt_text + mg_decode_gt_entries)"""
        text = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, dtype=np.uint8)
        so, sl = np.ascontiguousarray(span_off, dtype=np.uint64), np.ascontiguousarray(span_len, dtype=np.uint32)
        gi = np.ascontiguousarray(gt_index, dtype=np.int32)
        n = len(so)
        kp = None if keep is None else np.ascontiguousarray(keep, dtype=np.uint8)
        dflt, ne = C.c_uint16(), C.c_uint64()
        sp_off = np.zeros(n + 1, dtype=np.uint32)
        mask, mx = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
        self._ck(self._L.mg_decode_gt_text(self.h, _p(text), text.size, n, _p(so), _p(sl), _p(gi), n_columns, _p(kp), int(haploid), C.byref(dflt), _p(sp_off),
                                           _p(mask), _p(mx), C.byref(ne)))
        ss, sg = np.zeros(ne.value, dtype=np.uint32), np.zeros(ne.value, dtype=np.uint16)
        if n:
            self._ck(self._L.mg_decode_gt_entries(self.h, _p(ss), _p(sg)))
        return dflt.value, sp_off, ss, sg, mask, mx

    def counters_size(self):
        a, b = C.c_uint64(), C.c_uint64()
        self._ck(self._L.mg_counters_size(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def counters_export_device(self, d_ptr):
        self._ck(self._L.mg_counters_export_device(self.h, C.c_void_p(d_ptr)))

    def counters_import_device(self, d_ptr):
        self._ck(self._L.mg_counters_import_device(self.h, C.c_void_p(d_ptr)))

    def counters_view(self):
        """-> (device pointer, n_bf, n_map) of the contiguous [bf | map] u32 counter vector"""
        p, a, b = C.c_void_p(), C.c_uint64(), C.c_uint64()
        self._ck(self._L.mg_counters_view(self.h, C.byref(p), C.byref(a), C.byref(b)))
        return p.value, a.value, b.value

    def counters_reset(self):
        self._ck(self._L.mg_counters_reset(self.h))

    # cohort mode: the counters of several samples side by side (planes)
    def cohort_begin(self, n_planes):
        self._ck(self._L.mg_cohort_begin(self.h, int(n_planes)))

    def cohort_select(self, plane):
        self._ck(self._L.mg_cohort_select(self.h, int(plane)))

    def cohort_end(self):
        self._ck(self._L.mg_cohort_end(self.h))

    def cohort_info(self):
        """-> (planes, selected plane); (0, 0) outside cohort mode"""
        a, b = C.c_uint32(), C.c_uint32()
        self._ck(self._L.mg_cohort_info(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def cover_blocks_cohort_device(self, panel: "PanelDev", d_blk_var_off, d_var_block, d_n_blocks, haploid, d_cov, d_overflow):
        """d_cov: [planes][slots] u32, plane-major"""
        v = C.c_void_p
        self._ck(self._L.mg_cover_blocks_cohort_device(self.h, C.byref(panel), v(d_blk_var_off), v(d_var_block), v(d_n_blocks), int(haploid), v(d_cov), v(d_overflow)))

    def cohort_stats(self):
        """-> device ms of the most recent cover_blocks_cohort_device: (tier 1 over all planes, tiers 2-3 of all planes)"""
        ms = (C.c_float * 2)()
        self._ck(self._L.mg_cohort_stats(self.h, ms))
        return float(ms[0]), float(ms[1])

    def _rows(self, entry, keys, gt1, gt2, gq, haploid, min_gq, cap, fields=0, cov=None, var_allele_off=None, probs=None, var_gt_off=None, status=None, pl=None):
        """the host form of a row encoder (entry: mg_format_calls or mg_encode_calls_bcf, the latter with keys): the arrays as numpy
        arrays of the ABI's types into one mg_cells -> (bytes, row_off).  cap: the buffer to try first (default: sized by a first call);
        a buffer that is too small raises MalvaError(MG_ERR_LIMIT) with .needed, .row_off and .text set."""
        kept = []                     # (the converted arrays live as long as the struct's pointers are in use)

        def ptr(x, t):
            if x is None:
                return None
            kept.append(np.ascontiguousarray(x, dtype=t))
            return kept[-1].ctypes.data
        planes, n = np.shape(gt1)
        x = Cells(n, planes, int(haploid), ptr(gt1, np.int32), ptr(gt2, np.int32), ptr(gq, np.int32), int(min_gq is not None), int(min_gq or 0),
                  ptr(cov, np.uint32), ptr(var_allele_off, np.uint32), ptr(probs, np.float64), ptr(var_gt_off, np.uint64), ptr(status, np.uint8),
                  ptr(pl, np.int32), None, fields)
        head = (self.h, C.byref(x)) if keys is None else (self.h, C.byref(x), C.byref(_bcf_keys(keys)))
        row_off = np.zeros(n + 1, dtype=np.uint64)
        need = C.c_uint64(0)

        def call(c):
            out = np.zeros(max(c, 1), dtype=np.uint8)
            return entry(*head, _p(out) if c else None, c, _p(row_off), C.byref(need)), out
        rc, out = call(0 if cap is None else int(cap))
        if rc == -5 and cap is None and need.value:
            rc, out = call(need.value)
        if rc != 0:
            e = MalvaError(rc, self._L.mg_last_error(self.h).decode())
            e.needed, e.row_off, e.text = need.value, row_off, out
            raise e
        return out[:need.value].tobytes(), row_off

    def _rows_device(self, entry, keys, n_vars, planes, haploid, min_gq, d_out, cap, d_row_off, fields=0, **arrays):
        """the device form of a row encoder: arrays are mg_cells' members as device pointers -> (return code: 0 or MG_ERR_LIMIT, bytes the rows need)"""
        x = Cells(n_vars=n_vars, n_planes=planes, haploid=int(haploid), use_mask=int(min_gq is not None), min_gq=int(min_gq or 0), fields=fields, **arrays)
        head = (self.h, C.byref(x)) if keys is None else (self.h, C.byref(x), C.byref(_bcf_keys(keys)))
        need = C.c_uint64(0)
        rc = entry(*head, C.c_void_p(d_out), int(cap), C.c_void_p(d_row_off), C.byref(need))
        if rc not in (0, -5) or (rc == -5 and not need.value):
            self._ck(rc)
        return rc, need.value

    # the sample columns of a multi-sample VCF
    def format_calls(self, gt1, gt2, gq, haploid, cov=None, var_allele_off=None, text_cap=None, min_gq=None):
        """gt1 / gt2 / gq: [planes, n_vars] int32 -> (bytes, row_off): row v = bytes[row_off[v]:row_off[v + 1]], a tab and a
        `GT:GQ[:COVS]` cell per plane, then a newline.  cov: [planes, slots] with var_allele_off [n_vars + 1].  text_cap: the
        buffer to try first (default: sized by a first call); a buffer that is too small raises MalvaError(MG_ERR_LIMIT) with
        .needed and .row_off set.  min_gq: cells whose gq is below it print a missing genotype."""
        return self._rows(self._L.mg_format_calls, None, gt1, gt2, gq, haploid, min_gq, text_cap, cov=cov, var_allele_off=var_allele_off)

    def format_calls_device(self, n_vars, planes, haploid, d_gt1, d_gt2, d_gq, d_cov, d_var_allele_off, d_text, text_cap, d_row_off):
        """the same from device pointers into device buffers -> (return code: 0 or MG_ERR_LIMIT, bytes the text needs)"""
        return self._rows_device(self._L.mg_format_calls_device, None, n_vars, planes, haploid, None, d_text, text_cap, d_row_off, gt1=d_gt1, gt2=d_gt2, gq=d_gq,
                                 cov=d_cov, var_allele_off=d_var_allele_off)

    def format_calls_gp(self, gt1, gt2, gq, haploid, var_allele_off, probs, var_gt_off, status, cov=None, text_cap=None, min_gq=None):
        """format_calls with the field GP behind every cell's last (MG_CELLS_GP).  probs: [planes, var_gt_off[n_vars]] float64,
        a record's likelihoods in the reference's order; var_gt_off: [n_vars + 1] uint64; status: [planes, n_vars] uint8;
        var_allele_off is required, cov optional."""
        return self._rows(self._L.mg_format_calls, None, gt1, gt2, gq, haploid, min_gq, text_cap, CELLS_GP, cov, var_allele_off, probs, var_gt_off, status)

    def format_calls_gp_device(self, n_vars, planes, haploid, d_gt1, d_gt2, d_gq, d_cov, d_var_allele_off, d_probs, d_var_gt_off, d_status, d_text, text_cap,
                               d_row_off, min_gq=None):
        """the same from device pointers into device buffers -> (return code: 0 or MG_ERR_LIMIT, bytes the text needs)"""
        return self._rows_device(self._L.mg_format_calls_device, None, n_vars, planes, haploid, min_gq, d_text, text_cap, d_row_off, CELLS_GP, gt1=d_gt1, gt2=d_gt2,
                                 gq=d_gq, cov=d_cov, var_allele_off=d_var_allele_off, probs=d_probs, var_gt_off=d_var_gt_off, status=d_status)

    def format_calls_pl(self, gt1, gt2, gq, haploid, var_allele_off, var_gt_off, pl, probs=None, status=None, cov=None, text_cap=None, min_gq=None):
        """format_calls with the field PL behind every cell's last (MG_CELLS_PL): pl [planes, var_gt_off[n_vars]] int32, a
        record's values in VCF order, MG_PL_MISSING = INT32_MIN a missing one.  probs and status (both or neither): GP in front of PL."""
        return self._rows(self._L.mg_format_calls, None, gt1, gt2, gq, haploid, min_gq, text_cap, _pl_fields(probs is not None or status is not None), cov, var_allele_off, probs, var_gt_off,
                          status, pl)

    def format_calls_pl_device(self, n_vars, planes, haploid, d_gt1, d_gt2, d_gq, d_cov, d_var_allele_off, d_probs, d_var_gt_off, d_status, d_pl, d_text, text_cap,
                               d_row_off, min_gq=None):
        """the same from device pointers into device buffers -> (return code: 0 or MG_ERR_LIMIT, bytes the text needs)"""
        return self._rows_device(self._L.mg_format_calls_device, None, n_vars, planes, haploid, min_gq, d_text, text_cap, d_row_off, _pl_fields(d_probs or d_status),
                                 gt1=d_gt1, gt2=d_gt2, gq=d_gq, cov=d_cov, var_allele_off=d_var_allele_off, probs=d_probs, var_gt_off=d_var_gt_off, status=d_status,
                                 pl=d_pl)

    # Phred-scaled genotype likelihoods, prior-free
    def phred_likelihoods(self, cov, var_allele_off, error_rate, max_cov, haploid, cap=255, var_gt_off=None, pl_out=None):
        """cov: [planes, slots] uint32 -> (pl [planes, var_gt_off[-1]] int32 in VCF order, var_gt_off): the definition is
        mg_phred_likelihoods' in include/malva_hip.h.  var_gt_off: made from var_allele_off unless given; pl_out: written in place."""
        cov = np.ascontiguousarray(cov, dtype=np.uint32)
        vo = np.ascontiguousarray(var_allele_off, dtype=np.uint32)
        planes, n = cov.shape[0], len(vo) - 1
        if var_gt_off is None:
            A = np.diff(vo.astype(np.int64))
            var_gt_off = np.zeros(n + 1, dtype=np.uint64)
            var_gt_off[1:] = np.cumsum(A if haploid else A * (A + 1) // 2)
        go = np.ascontiguousarray(var_gt_off, dtype=np.uint64)
        pl = np.zeros((planes, int(go[-1])), dtype=np.int32) if pl_out is None else pl_out
        self._ck(self._L.mg_phred_likelihoods(self.h, n, planes, _p(cov), _p(vo), _p(go), C.c_float(error_rate), int(max_cov), int(haploid), int(cap), _p(pl)))
        return pl, go

    def phred_likelihoods_device(self, n_vars, planes, d_cov, d_var_allele_off, d_var_gt_off, error_rate, max_cov, haploid, cap, d_pl_out):
        """the same from device pointers into a device buffer, asynchronous on the context's stream"""
        v = C.c_void_p
        self._ck(self._L.mg_phred_likelihoods_device(self.h, n_vars, planes, v(d_cov), v(d_var_allele_off), v(d_var_gt_off), C.c_float(error_rate), int(max_cov),
                                                     int(haploid), int(cap), v(d_pl_out)))

    def pl_stats(self):
        """-> device ms of the most recent phred_likelihoods"""
        ms = (C.c_float * 1)()
        self._ck(self._L.mg_pl_stats(self.h, ms))
        return float(ms[0])

    def format_stats(self):
        """-> device ms of the most recent format_calls: (length pass, scan, write pass)"""
        ms = (C.c_float * 3)()
        self._ck(self._L.mg_format_stats(self.h, ms))
        return float(ms[0]), float(ms[1]), float(ms[2])

    # the site tags of a multi-sample VCF
    def site_counts(self, gt1, gt2, gq, haploid, var_allele_off, min_gq=None, ac=None, ns=None):
        """gt1 / gt2 / gq: [planes, n_vars] int32 -> (ac [var_allele_off[n_vars]], ns [n_vars]) uint32: per allele slot the called
        copies over the planes, per record the called planes.  min_gq: cells whose gq is below it are not called.  ac / ns given:
        the counts are added to them (in place)."""
        a = lambda x, t: None if x is None else np.ascontiguousarray(x, dtype=t)
        g1, g2, q, vo = a(gt1, np.int32), a(gt2, np.int32), a(gq, np.int32), a(var_allele_off, np.uint32)
        planes, n = g1.shape
        acc = ac is not None
        assert acc == (ns is not None)
        if acc:
            assert ac.dtype == np.uint32 and ns.dtype == np.uint32 and ac.flags.c_contiguous and ns.flags.c_contiguous
            assert ac.size == int(vo[n]) and ns.size == n
        else:
            ac, ns = np.zeros(int(vo[n]), dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        self._ck(self._L.mg_site_counts(self.h, n, planes, int(haploid), _p(g1), _p(g2), _p(q), int(min_gq is not None), int(min_gq or 0), _p(vo), int(acc),
                                        _p(ac), _p(ns)))
        return ac, ns

    def format_site_info(self, ac, ns, var_allele_off, text_cap=None):
        """-> (bytes, row_off): row v = bytes[row_off[v]:row_off[v + 1]] is record v's `AC=..;AN=..;AF=..;NS=..`.  text_cap as for
        format_calls."""
        ac, ns, vo = (np.ascontiguousarray(x, dtype=np.uint32) for x in (ac, ns, var_allele_off))
        n = ns.size
        row_off = np.zeros(n + 1, dtype=np.uint64)
        need = C.c_uint64(0)

        def call(cap):
            text = np.zeros(max(cap, 1), dtype=np.uint8)
            return self._L.mg_format_site_info(self.h, n, _p(ac), _p(ns), _p(vo), _p(text) if cap else None, cap, _p(row_off), C.byref(need)), text
        rc, text = call(0 if text_cap is None else int(text_cap))
        if rc == -5 and text_cap is None and need.value:
            rc, text = call(need.value)
        if rc != 0:
            e = MalvaError(rc, self._L.mg_last_error(self.h).decode())
            e.needed, e.row_off, e.text = need.value, row_off, text
            raise e
        return text[:need.value].tobytes(), row_off

    def site_stats(self):
        """-> device ms of the most recent site_counts and of the most recent format_site_info"""
        ms = (C.c_float * 2)()
        self._ck(self._L.mg_site_stats(self.h, ms))
        return float(ms[0]), float(ms[1])

    # the pair table of a multi-sample call set
    def pack_dosage(self, gt1, gt2, gq, haploid, var_allele_off, min_gq=None, out=None):
        """gt1 / gt2 / gq: [planes, n_vars] int32 -> uint64 [planes, 3, W], W = (n_vars + 63) // 64: bit v & 63 of word v >> 6 of
        [p, d] is set when (p, v) is a called cell of a biallelic record with allele indexes in {0, 1} and dosage d (haploid:
        2 * gt1).  min_gq: cells whose gq is below it are not called.  out: the array to fill (every word is overwritten)."""
        a = lambda x, t: None if x is None else np.ascontiguousarray(x, dtype=t)
        g1, g2, q, vo = a(gt1, np.int32), a(gt2, np.int32), a(gq, np.int32), a(var_allele_off, np.uint32)
        planes, n = g1.shape
        if out is None:
            out = np.zeros((planes, 3, (n + 63) // 64), dtype=np.uint64)
        assert out.dtype == np.uint64 and out.flags.c_contiguous and out.shape == (planes, 3, (n + 63) // 64)
        self._ck(self._L.mg_pack_dosage(self.h, n, planes, int(haploid), _p(g1), _p(g2), _p(q), int(min_gq is not None), int(min_gq or 0), _p(vo), _p(out)))
        return out

    def pair_counts(self, planes_a, planes_b=None, counts=None, overwrite=False):
        """planes_a [n_a, 3, W], planes_b [n_b, 3, W] (None: B is A) as pack_dosage lays them out -> uint64 [n_a, n_b, 3, 3]:
        [i, j, da, db] = the bits set in both A[i, da] and B[j, db].  counts given: the sums are added to it (in place) unless
        overwrite."""
        A = np.ascontiguousarray(planes_a, dtype=np.uint64)
        B = None if planes_b is None else np.ascontiguousarray(planes_b, dtype=np.uint64)
        n_a, _, W = A.shape
        n_b = n_a if B is None else B.shape[0]
        assert B is None or B.shape[1:] == (3, W)
        acc = counts is not None and not overwrite
        if counts is None:
            counts = np.zeros((n_a, n_b, 3, 3), dtype=np.uint64)
        assert counts.dtype == np.uint64 and counts.flags.c_contiguous and counts.shape == (n_a, n_b, 3, 3)
        self._ck(self._L.mg_pair_counts(self.h, W, _p(A), n_a, _p(B), n_b, int(acc), _p(counts)))
        return counts

    def pairs_stats(self):
        """-> device ms of the most recent pack_dosage and of the most recent pair_counts"""
        ms = (C.c_float * 2)()
        self._ck(self._L.mg_pairs_stats(self.h, ms))
        return float(ms[0]), float(ms[1])

    # the per-sample table of a multi-sample call set
    def sample_counts(self, gt1, gt2, gq, haploid, var_allele_off, status=None, cov=None, allele_class=None, min_gq=None, counts=None, overwrite=False):
        """gt1 / gt2 / gq: [planes, n_vars] int32; status [planes, n_vars] uint8, cov [planes, slots] uint32, allele_class [slots] uint8,
        each or None -> uint64 [planes, SAMPLE_SLOTS], the slots MG_SS_* of include/malva_hip.h.  min_gq: cells whose gq is below it
        are masked.  counts given: the sums are added to it (in place) unless overwrite."""
        a = lambda x, t: None if x is None else np.ascontiguousarray(x, dtype=t)
        g1, g2, q, vo = a(gt1, np.int32), a(gt2, np.int32), a(gq, np.int32), a(var_allele_off, np.uint32)
        st, cv, ac = a(status, np.uint8), a(cov, np.uint32), a(allele_class, np.uint8)
        planes, n = g1.shape
        slots = int(vo[n]) if n else 0
        assert st is None or st.shape == (planes, n)
        assert cv is None or cv.shape == (planes, slots)
        assert ac is None or ac.shape == (slots,)
        acc = counts is not None and not overwrite
        if counts is None:
            counts = np.zeros((planes, SAMPLE_SLOTS), dtype=np.uint64)
        assert counts.dtype == np.uint64 and counts.flags.c_contiguous and counts.shape == (planes, SAMPLE_SLOTS)
        self._ck(self._L.mg_sample_counts(self.h, n, planes, int(haploid), _p(g1), _p(g2), _p(q), int(min_gq is not None), int(min_gq or 0), _p(st), _p(cv), _p(vo),
                                          _p(ac), int(acc), _p(counts)))
        return counts

    def sample_stats(self):
        """-> device ms of the most recent sample_counts"""
        ms = (C.c_float * 1)()
        self._ck(self._L.mg_sample_stats(self.h, ms))
        return float(ms[0])

    # the per-record table of a multi-sample call set
    def site_geno_counts(self, gt1, gt2, gq, haploid, var_allele_off, min_gq=None, n=None, het=None, hom=None):
        """gt1 / gt2 / gq: [planes, n_vars] int32 (gt2 may be None in haploid mode) -> (n [n_vars], het [slots], hom [slots]) uint32: per
        record the usable cells, per allele slot the heterozygous and homozygous ones among them (mg_site_geno_counts in
        include/malva_hip.h).  min_gq: cells whose gq is below it are masked.  n / het / hom given: the counts are added to them (in place)."""
        a = lambda x, t: None if x is None else np.ascontiguousarray(x, dtype=t)
        g1, g2, q, vo = a(gt1, np.int32), a(gt2, np.int32), a(gq, np.int32), a(var_allele_off, np.uint32)
        planes, nv = g1.shape
        slots = int(vo[nv]) if nv else 0
        acc = n is not None
        assert acc == (het is not None) == (hom is not None)
        if acc:
            for x, size in ((n, nv), (het, slots), (hom, slots)):
                assert x.dtype == np.uint32 and x.flags.c_contiguous and x.size == size
        else:
            n, het, hom = np.zeros(nv, dtype=np.uint32), np.zeros(slots, dtype=np.uint32), np.zeros(slots, dtype=np.uint32)
        self._ck(self._L.mg_site_geno_counts(self.h, nv, planes, int(haploid), _p(g1), _p(g2), _p(q), int(min_gq is not None), int(min_gq or 0), _p(vo), int(acc),
                                             _p(n), _p(het), _p(hom)))
        return n, het, hom

    def site_geno_counts_device(self, n_vars, planes, haploid, d_gt1, d_gt2, d_gq, d_var_allele_off, d_n, d_het, d_hom, min_gq=None, accumulate=False):
        """the same from device pointers into device buffers, asynchronous on the context's stream"""
        v = C.c_void_p
        self._ck(self._L.mg_site_geno_counts_device(self.h, n_vars, planes, int(haploid), v(d_gt1), v(d_gt2), v(d_gq), int(min_gq is not None), int(min_gq or 0),
                                                    v(d_var_allele_off), int(accumulate), v(d_n), v(d_het), v(d_hom)))

    def hwe_exact(self, n, het, hom):
        """n / het / hom: [items] uint32 -> (hwe, exc_het) float64 [items]: the exact test of Hardy-Weinberg proportions per item, two-sided
        and for an excess of heterozygotes (mg_hwe_exact in include/malva_hip.h); NaN where het + hom > n"""
        n, het, hom = (np.ascontiguousarray(x, dtype=np.uint32) for x in (n, het, hom))
        assert n.ndim == 1 and n.shape == het.shape == hom.shape
        hwe, exc = np.zeros(n.size, dtype=np.float64), np.zeros(n.size, dtype=np.float64)
        self._ck(self._L.mg_hwe_exact(self.h, n.size, _p(n), _p(het), _p(hom), _p(hwe), _p(exc)))
        return hwe, exc

    def hwe_exact_device(self, n_items, d_n, d_het, d_hom, d_hwe, d_exc_het):
        """the same from device pointers into device buffers, asynchronous on the context's stream"""
        v = C.c_void_p
        self._ck(self._L.mg_hwe_exact_device(self.h, n_items, v(d_n), v(d_het), v(d_hom), v(d_hwe), v(d_exc_het)))

    def hwe_stats(self):
        """-> device ms of the most recent site_geno_counts and of the most recent hwe_exact"""
        ms = (C.c_float * 2)()
        self._ck(self._L.mg_hwe_stats(self.h, ms))
        return float(ms[0]), float(ms[1])

    # the LD table of a multi-sample call set
    def pack_site_dosage(self, gt1, gt2, gq, haploid, var_allele_off, min_gq=None, out=None):
        """gt1 / gt2 / gq: [planes, n_vars] int32 -> uint64 [3, n_vars]: bit p of [d, v] is set when (p, v) is a called cell of a biallelic
        record with allele indexes in {0, 1} and dosage d (haploid: 2 * gt1) -- pack_dosage's cells, bits over samples per record
        (mg_pack_site_dosage in include/malva_hip.h).  out: the array to fill (every word is overwritten)."""
        a = lambda x, t: None if x is None else np.ascontiguousarray(x, dtype=t)
        g1, g2, q, vo = a(gt1, np.int32), a(gt2, np.int32), a(gq, np.int32), a(var_allele_off, np.uint32)
        planes, n = g1.shape
        if out is None:
            out = np.zeros((3, n), dtype=np.uint64)
        assert out.dtype == np.uint64 and out.flags.c_contiguous and out.shape == (3, n)
        self._ck(self._L.mg_pack_site_dosage(self.h, n, planes, int(haploid), _p(g1), _p(g2), _p(q), int(min_gq is not None), int(min_gq or 0), _p(vo), _p(out)))
        return out

    def pack_site_dosage_device(self, n_vars, planes, haploid, d_gt1, d_gt2, d_gq, d_var_allele_off, d_sites_out, min_gq=None):
        """the same from device pointers into a device buffer, asynchronous on the context's stream"""
        v = C.c_void_p
        self._ck(self._L.mg_pack_site_dosage_device(self.h, n_vars, planes, int(haploid), v(d_gt1), v(d_gt2), v(d_gq), int(min_gq is not None), int(min_gq or 0),
                                                    v(d_var_allele_off), v(d_sites_out)))

    def ld_window(self, sites, chrom, pos, window, n_first=None, max_bp=0, min_n=1, min_r2=0.0, pairs_cap=None):
        """sites: uint64 [groups, 3, n_vars] (the groups' pack_site_dosage outputs); chrom / pos: uint32 [n_vars] -> (pairs, row_off): pairs a
        structured array (LD_PAIR: i, j, n, sign, r2) of the emitted pairs ordered by i, then j; record i's are
        pairs[row_off[i]:row_off[i + 1]], i < n_first (default: n_vars) -- mg_ld_window in include/malva_hip.h.  pairs_cap None: the call
        is repeated with the buffer it asked for; a given one that is too small raises MalvaError(MG_ERR_LIMIT) with .needed, .row_off
        and .pairs (the whole buffer) set."""
        S = np.ascontiguousarray(sites, dtype=np.uint64)
        ch, po = (np.ascontiguousarray(x, dtype=np.uint32) for x in (chrom, pos))
        groups, three, n = S.shape
        assert three == 3 and ch.shape == (n,) and po.shape == (n,)
        nf = n if n_first is None else int(n_first)
        row_off = np.zeros(max(nf, 0) + 1, dtype=np.uint64)
        need = C.c_uint64(0)

        def call(cap):
            pairs = np.zeros(max(cap, 1), dtype=LD_PAIR)
            return self._L.mg_ld_window(self.h, n, nf, groups, _p(S), _p(ch), _p(po), int(window), int(max_bp), int(min_n), float(min_r2),
                                        _p(pairs) if cap else None, cap, _p(row_off), C.byref(need)), pairs
        rc, pairs = call(0 if pairs_cap is None else int(pairs_cap))
        if rc == -5 and pairs_cap is None and need.value:
            rc, pairs = call(need.value)
        if rc != 0:
            e = MalvaError(rc, self._L.mg_last_error(self.h).decode())
            e.needed, e.row_off, e.pairs = need.value, row_off, pairs
            raise e
        return pairs[:need.value], row_off

    def ld_window_device(self, n_vars, n_first, groups, d_sites, d_chrom, d_pos, window, max_bp, min_n, min_r2, d_pairs, pairs_cap, d_row_off):
        """the same from device pointers into device buffers -> (return code, pairs needed); MG_ERR_LIMIT (-5) is returned, not raised"""
        v = C.c_void_p
        need = C.c_uint64(0)
        rc = self._L.mg_ld_window_device(self.h, n_vars, n_first, groups, v(d_sites), v(d_chrom), v(d_pos), int(window), int(max_bp), int(min_n), float(min_r2),
                                         v(d_pairs), pairs_cap, v(d_row_off), C.byref(need))
        if rc not in (0, -5):
            self._ck(rc)
        return rc, need.value

    def ld_stats(self):
        """-> device ms of the most recent pack_site_dosage and of the most recent ld_window"""
        ms = (C.c_float * 2)()
        self._ck(self._L.mg_ld_stats(self.h, ms))
        return float(ms[0]), float(ms[1])

    # IBS0-free segments per pair of samples
    def sites_to_planes(self, sites, out=None):
        """sites: uint64 [groups, 3, n_vars] (the groups' pack_site_dosage outputs) -> uint64 [64 * groups, 3, W], W = (n_vars + 63) // 64, laid
        out as pack_dosage's: bit v & 63 of word v >> 6 of [64 g + p, d] is bit p of sites[g, d, v] (mg_sites_to_planes in
        include/malva_hip.h).  out: the array to fill (every word is overwritten)."""
        S = np.ascontiguousarray(sites, dtype=np.uint64)
        groups, three, n = S.shape
        assert three == 3
        if out is None:
            out = np.zeros((64 * groups, 3, (n + 63) // 64), dtype=np.uint64)
        assert out.dtype == np.uint64 and out.flags.c_contiguous and out.shape == (64 * groups, 3, (n + 63) // 64)
        self._ck(self._L.mg_sites_to_planes(self.h, n, groups, _p(S), _p(out)))
        return out

    def sites_to_planes_device(self, n_vars, groups, d_sites, d_planes_out):
        """the same from a device pointer into a device buffer, asynchronous on the context's stream"""
        self._ck(self._L.mg_sites_to_planes_device(self.h, n_vars, groups, C.c_void_p(d_sites), C.c_void_p(d_planes_out)))

    def ibd_begin(self, n_samples, min_records=1, min_bp=0):
        """the state of all pairs of n_samples samples, every pair closed (mg_ibd_begin); a second begin discards the first"""
        self._ck(self._L.mg_ibd_begin(self.h, int(n_samples), int(min_records), int(min_bp)))

    def ibd_step(self, sites, chrom, pos, flush=False, segs_cap=None, segs=None):
        """the next records: sites uint64 [groups, 3, n_vars], chrom / pos uint32 [n_vars] -> the segments closed in this step, a structured
        array (IBD_SEG) ordered by (a, b, start) -- mg_ibd_step in include/malva_hip.h.  segs_cap None: the call is repeated with the buffer it
        asked for; a given one that is too small raises MalvaError(MG_ERR_LIMIT) with .needed set, and the state has not advanced.  segs: the
        buffer to use (at least segs_cap entries)."""
        S = np.ascontiguousarray(sites, dtype=np.uint64)
        ch, po = (np.ascontiguousarray(x, dtype=np.uint32) for x in (chrom, pos))
        groups, three, n = S.shape
        assert three == 3 and ch.shape == (n,) and po.shape == (n,)
        need = C.c_uint64(0)

        def call(cap, buf):
            if buf is None:
                buf = np.zeros(max(cap, 1), dtype=IBD_SEG)
            assert buf.dtype == IBD_SEG and buf.flags.c_contiguous and len(buf) >= cap
            return self._L.mg_ibd_step(self.h, n, groups, _p(S), _p(ch), _p(po), int(bool(flush)), _p(buf) if cap else None, cap, C.byref(need)), buf
        rc, buf = call(0 if segs_cap is None else int(segs_cap), segs)
        if rc == -5 and segs_cap is None and need.value:
            rc, buf = call(need.value, None)
        if rc != 0:
            e = MalvaError(rc, self._L.mg_last_error(self.h).decode())
            e.needed = need.value
            raise e
        return buf[:need.value]

    def ibd_step_device(self, n_vars, groups, d_sites, d_chrom, d_pos, flush, d_segs, segs_cap):
        """the same from device pointers into a device buffer -> (return code, segments needed); MG_ERR_LIMIT (-5) is returned, not raised"""
        v = C.c_void_p
        need = C.c_uint64(0)
        rc = self._L.mg_ibd_step_device(self.h, n_vars, groups, v(d_sites), v(d_chrom), v(d_pos), int(bool(flush)), v(d_segs), segs_cap, C.byref(need))
        if rc not in (0, -5):
            self._ck(rc)
        return rc, need.value

    def ibd_end(self):
        self._ck(self._L.mg_ibd_end(self.h))

    def ibd_stats(self):
        """-> device ms of the most recent transpose and of the most recent ibd_step"""
        ms = (C.c_float * 2)()
        self._ck(self._L.mg_ibd_stats(self.h, ms))
        return float(ms[0]), float(ms[1])

    # the genetic relationship matrix
    def grm_weights(self, sites, n_samples, haploid=False, maf_ppm=0, min_n=1, out=None):
        """sites: uint64 [groups, 3, n_vars], groups == ceil(n_samples / 64) -> int16 [n_vars, 4]: q0 q1 q2 1 of a record that enters, zeros of
        one that does not (mg_grm_weights in include/malva_hip.h).  out: the array to fill."""
        S = np.ascontiguousarray(sites, dtype=np.uint64)
        groups, three, n = S.shape
        assert three == 3
        if out is None:
            out = np.zeros((n, 4), dtype=np.int16)
        assert out.dtype == np.int16 and out.flags.c_contiguous and out.shape == (n, 4)
        self._ck(self._L.mg_grm_weights(self.h, n, groups, int(n_samples), _p(S), int(bool(haploid)), int(maf_ppm), int(min_n), _p(out)))
        return out

    def grm_weights_device(self, n_vars, groups, n_samples, d_sites, haploid, maf_ppm, min_n, d_q_out):
        """the same from a device pointer into a device buffer, asynchronous on the context's stream"""
        self._ck(self._L.mg_grm_weights_device(self.h, n_vars, groups, int(n_samples), C.c_void_p(d_sites), int(bool(haploid)), int(maf_ppm), int(min_n),
                                               C.c_void_p(d_q_out)))

    def grm_begin(self, n_samples, haploid=False, maf_ppm=0, min_n=1):
        """the state of all n (n + 1) / 2 pairs, zero (mg_grm_begin); a second begin discards the first"""
        self._ck(self._L.mg_grm_begin(self.h, int(n_samples), int(bool(haploid)), int(maf_ppm), int(min_n)))

    def grm_step(self, sites):
        """the next records: sites uint64 [groups, 3, n_vars] (mg_grm_step)"""
        S = np.ascontiguousarray(sites, dtype=np.uint64)
        groups, three, n = S.shape
        assert three == 3
        self._ck(self._L.mg_grm_step(self.h, n, groups, _p(S) if n else None))

    def grm_step_device(self, n_vars, groups, d_sites):
        """the same from a device pointer, asynchronous on the context's stream"""
        self._ck(self._L.mg_grm_step_device(self.h, n_vars, groups, C.c_void_p(d_sites)))

    def grm_read(self, n_samples):
        """-> (S int64 [n (n + 1) / 2], N uint64 likewise, records seen, records entered): pair (a, b), a <= b, row-major (mg_grm_read)"""
        k = n_samples * (n_samples + 1) // 2
        S, N, rec = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
        self._ck(self._L.mg_grm_read(self.h, _p(S), _p(N), _p(rec)))
        return S, N, int(rec[0]), int(rec[1])

    def grm_end(self):
        self._ck(self._L.mg_grm_end(self.h))

    def grm_stats(self):
        """-> device ms of the most recent step's weights + expansion and Gram kernel, and of the most recent read"""
        ms = (C.c_float * 3)()
        self._ck(self._L.mg_grm_stats(self.h, ms))
        return float(ms[0]), float(ms[1]), float(ms[2])

    # principal components of a resident symmetric matrix
    def pca_load_tri(self, tri, n):
        """tri: float32 [n (n + 1) / 2], the lower triangle row by row as in GCTA's .grm.bin (mg_pca_load_tri_f32); a second load discards the first"""
        T = np.ascontiguousarray(tri, dtype=np.float32).reshape(-1)
        assert T.size == n * (n + 1) // 2
        self._ck(self._L.mg_pca_load_tri_f32(self.h, int(n), _p(T)))

    def pca_load(self, full):
        """full: float64 [n, n]; only its lower triangle is read and mirrored (mg_pca_load_f64)"""
        A = np.ascontiguousarray(full, dtype=np.float64)
        assert A.ndim == 2 and A.shape[0] == A.shape[1]
        self._ck(self._L.mg_pca_load_f64(self.h, A.shape[0], _p(A)))

    def pca_load_tri_device(self, n, d_tri):
        """the same from a device pointer, asynchronous on the context's stream; a non-finite value is reported by the first solve"""
        self._ck(self._L.mg_pca_load_tri_f32_device(self.h, int(n), C.c_void_p(d_tri)))

    def pca_load_device(self, n, d_full):
        self._ck(self._L.mg_pca_load_f64_device(self.h, int(n), C.c_void_p(d_full)))

    def pca_solve(self, n, k, tol=1e-10, max_iters=2000):
        """-> (values [k], vectors [k, n], resid [k], scale, (products, converged, m)) of the loaded n x n matrix (mg_pca_solve)"""
        values, vectors, resid = np.zeros(k, dtype=np.float64), np.zeros((k, n), dtype=np.float64), np.zeros(k, dtype=np.float64)
        scale, info = np.zeros(1, dtype=np.float64), np.zeros(3, dtype=np.uint32)
        self._ck(self._L.mg_pca_solve(self.h, int(k), float(tol), int(max_iters), _p(values), _p(vectors), _p(resid), _p(scale), _p(info)))
        return values, vectors, resid, float(scale[0]), (int(info[0]), int(info[1]), int(info[2]))

    def pca_solve_device(self, k, tol, max_iters, d_values, d_vectors, d_resid, d_scale, d_info):
        """the same into device buffers: float64 [k], [k, n], [k], [1] and uint32 [3]"""
        self._ck(self._L.mg_pca_solve_device(self.h, int(k), float(tol), int(max_iters), C.c_void_p(d_values), C.c_void_p(d_vectors), C.c_void_p(d_resid),
                                             C.c_void_p(d_scale), C.c_void_p(d_info)))

    def pca_end(self):
        self._ck(self._L.mg_pca_end(self.h))

    def pca_stats(self):
        """-> device ms of the most recent solve: products, orthonormalisation, Rayleigh-Ritz, total"""
        ms = (C.c_float * 4)()
        self._ck(self._L.mg_pca_stats(self.h, ms))
        return tuple(float(x) for x in ms)

    # allele priors re-estimated from the planes of a batch, and the cells genotyped under them
    def genotype_cohort(self, cov, freq, var_allele_off, error_rate, max_cov, haploid, iters=5, weight=1.0, want_probs=False):
        """cov: [planes, slots] uint32; freq: [slots] float32 -> (freq_out [slots] float32, n_informative [n_vars] uint32, gt1, gt2, gq
        [planes, n_vars] int32, status [planes, n_vars] uint8, probs [planes, var_gt_off[-1]] float64 or None, var_gt_off or None): the
        definition is mg_genotype_cohort's in include/malva_hip.h"""
        cov = np.ascontiguousarray(cov, dtype=np.uint32)
        freq = np.ascontiguousarray(freq, dtype=np.float32)
        vo = np.ascontiguousarray(var_allele_off, dtype=np.uint32)
        planes, n = cov.shape[0], len(vo) - 1
        assert cov.shape == (planes, int(vo[n])) and freq.shape == (int(vo[n]),)
        fo, ni = np.zeros(len(freq), dtype=np.float32), np.zeros(n, dtype=np.uint32)
        g1, g2, gq = (np.zeros((planes, n), dtype=np.int32) for _ in range(3))
        st = np.zeros((planes, n), dtype=np.uint8)
        probs = goff = None
        if want_probs:
            A = np.diff(vo.astype(np.int64))
            goff = np.zeros(n + 1, dtype=np.uint64)
            goff[1:] = np.cumsum(A if haploid else A * (A + 1) // 2)
            probs = np.zeros((planes, int(goff[-1])), dtype=np.float64)
        self._ck(self._L.mg_genotype_cohort(self.h, n, planes, _p(cov), _p(freq), _p(vo), C.c_float(error_rate), max_cov, int(haploid), int(iters), float(weight),
                                            _p(fo), _p(ni), _p(g1), _p(g2), _p(gq), _p(st), _p(probs), _p(goff)))
        return fo, ni, g1, g2, gq, st, probs, goff

    def genotype_cohort_device(self, n_vars, planes, d_cov, d_freq, d_var_allele_off, error_rate, max_cov, haploid, iters, weight, d_freq_out, d_n_informative,
                               d_g1, d_g2, d_gq, d_st, d_probs=None, d_gt_off=None):
        v = C.c_void_p
        self._ck(self._L.mg_genotype_cohort_device(self.h, n_vars, planes, v(d_cov), v(d_freq), v(d_var_allele_off), C.c_float(error_rate), max_cov, int(haploid),
                                                   int(iters), float(weight), v(d_freq_out), v(d_n_informative), v(d_g1), v(d_g2), v(d_gq), v(d_st), v(d_probs),
                                                   v(d_gt_off)))

    def cohort_prior_stats(self):
        """-> device ms of the most recent genotype_cohort"""
        ms = (C.c_float * 1)()
        self._ck(self._L.mg_cohort_prior_stats(self.h, ms))
        return float(ms[0])

    # the estimate alone, for any number of planes
    def estimate_priors(self, cov, freq, var_allele_off, error_rate, max_cov, haploid, iters=5, weight=1.0):
        """cov: [planes, slots] uint32 (1..MG_PRIOR_WIDE_MAX_PLANES planes); freq: [slots] float32 -> (freq_out [slots] float32,
        n_informative [n_vars] uint32): the definition is mg_estimate_priors' in include/malva_hip.h"""
        cov = np.ascontiguousarray(cov, dtype=np.uint32)
        freq = np.ascontiguousarray(freq, dtype=np.float32)
        vo = np.ascontiguousarray(var_allele_off, dtype=np.uint32)
        planes, n = cov.shape[0], len(vo) - 1
        assert cov.shape == (planes, int(vo[n])) and freq.shape == (int(vo[n]),)
        fo, ni = np.zeros(len(freq), dtype=np.float32), np.zeros(n, dtype=np.uint32)
        self._ck(self._L.mg_estimate_priors(self.h, n, planes, _p(cov), _p(freq), _p(vo), C.c_float(error_rate), max_cov, int(haploid), int(iters), float(weight),
                                            _p(fo), _p(ni)))
        return fo, ni

    def estimate_priors_device(self, n_vars, planes, d_cov, d_freq, d_var_allele_off, error_rate, max_cov, haploid, iters, weight, d_freq_out, d_n_informative):
        v = C.c_void_p
        self._ck(self._L.mg_estimate_priors_device(self.h, n_vars, planes, v(d_cov), v(d_freq), v(d_var_allele_off), C.c_float(error_rate), max_cov, int(haploid),
                                                   int(iters), float(weight), v(d_freq_out), v(d_n_informative)))

    def estimate_priors_stats(self):
        """-> device ms of the most recent estimate_priors"""
        ms = (C.c_float * 1)()
        self._ck(self._L.mg_estimate_priors_stats(self.h, ms))
        return float(ms[0])

    # the sample columns of a multi-sample BCF
    def encode_calls_bcf(self, gt1, gt2, gq, haploid, keys, cov=None, var_allele_off=None, out_cap=None, min_gq=None):
        """gt1 / gt2 / gq: [planes, n_vars] int32 -> (bytes, row_off): row v = bytes[row_off[v]:row_off[v + 1]] is record v's BCF
        per-sample block, fields GT, GQ and (with cov [planes, slots] and var_allele_off [n_vars + 1]) COVS.  keys: the header's
        dictionary indexes (gt, gq, cov).  out_cap and min_gq as format_calls' text_cap and min_gq; a buffer that is too small
        raises MalvaError(MG_ERR_LIMIT) with .needed, .row_off and .text set."""
        return self._rows(self._L.mg_encode_calls_bcf, keys[:3], gt1, gt2, gq, haploid, min_gq, out_cap, cov=cov, var_allele_off=var_allele_off)

    def encode_calls_bcf_device(self, n_vars, planes, haploid, d_gt1, d_gt2, d_gq, d_cov, d_var_allele_off, keys, d_out, out_cap, d_row_off, min_gq=None):
        """the same from device pointers into device buffers -> (return code: 0 or MG_ERR_LIMIT, bytes the rows need)"""
        return self._rows_device(self._L.mg_encode_calls_bcf_device, keys[:3], n_vars, planes, haploid, min_gq, d_out, out_cap, d_row_off, gt1=d_gt1, gt2=d_gt2,
                                 gq=d_gq, cov=d_cov, var_allele_off=d_var_allele_off)

    def encode_calls_bcf_gp(self, gt1, gt2, gq, haploid, keys, var_allele_off, probs, var_gt_off, status, cov=None, out_cap=None, min_gq=None):
        """encode_calls_bcf with the float field GP behind the record's last (MG_CELLS_GP).  keys: (gt, gq, cov, gp);
        the arrays as format_calls_gp's."""
        return self._rows(self._L.mg_encode_calls_bcf, keys[:4], gt1, gt2, gq, haploid, min_gq, out_cap, CELLS_GP, cov, var_allele_off, probs, var_gt_off, status)

    def encode_calls_bcf_gp_device(self, n_vars, planes, haploid, d_gt1, d_gt2, d_gq, d_cov, d_var_allele_off, d_probs, d_var_gt_off, d_status, keys, d_out, out_cap,
                                   d_row_off, min_gq=None):
        """the same from device pointers into device buffers -> (return code: 0 or MG_ERR_LIMIT, bytes the rows need)"""
        return self._rows_device(self._L.mg_encode_calls_bcf_device, keys[:4], n_vars, planes, haploid, min_gq, d_out, out_cap, d_row_off, CELLS_GP, gt1=d_gt1,
                                 gt2=d_gt2, gq=d_gq, cov=d_cov, var_allele_off=d_var_allele_off, probs=d_probs, var_gt_off=d_var_gt_off, status=d_status)

    def encode_calls_bcf_pl(self, gt1, gt2, gq, haploid, keys, var_allele_off, var_gt_off, pl, probs=None, status=None, cov=None, out_cap=None, min_gq=None):
        """encode_calls_bcf with the integer field PL behind the record's last (MG_CELLS_PL).  keys: (gt, gq, cov, gp, pl);
        the arrays as format_calls_pl's."""
        return self._rows(self._L.mg_encode_calls_bcf, keys[:5], gt1, gt2, gq, haploid, min_gq, out_cap, _pl_fields(probs is not None or status is not None), cov, var_allele_off, probs,
                          var_gt_off, status, pl)

    def encode_calls_bcf_pl_device(self, n_vars, planes, haploid, d_gt1, d_gt2, d_gq, d_cov, d_var_allele_off, d_probs, d_var_gt_off, d_status, d_pl, keys, d_out,
                                   out_cap, d_row_off, min_gq=None):
        """the same from device pointers into device buffers -> (return code: 0 or MG_ERR_LIMIT, bytes the rows need)"""
        return self._rows_device(self._L.mg_encode_calls_bcf_device, keys[:5], n_vars, planes, haploid, min_gq, d_out, out_cap, d_row_off,
                                 _pl_fields(d_probs or d_status), gt1=d_gt1, gt2=d_gt2, gq=d_gq, cov=d_cov, var_allele_off=d_var_allele_off, probs=d_probs,
                                 var_gt_off=d_var_gt_off, status=d_status, pl=d_pl)

    def bcf_stats(self):
        """-> device ms of the most recent encode_calls_bcf: (length pass, scan, write pass)"""
        ms = (C.c_float * 3)()
        self._ck(self._L.mg_bcf_stats(self.h, ms))
        return float(ms[0]), float(ms[1]), float(ms[2])

    # multi-GPU exchange inside the library (RCCL)
    def comm_init(self, rank, world, comm_id: bytes):
        assert len(comm_id) == COMM_ID_BYTES
        buf = C.create_string_buffer(bytes(comm_id), COMM_ID_BYTES)
        self._ck(self._L.mg_comm_init(self.h, rank, world, buf))

    def comm_destroy(self):
        self._ck(self._L.mg_comm_destroy(self.h))

    def comm_info(self):
        r, w, b = C.c_int(), C.c_int(), C.c_int()
        self._ck(self._L.mg_comm_info(self.h, C.byref(r), C.byref(w), C.byref(b)))
        return r.value, w.value, b.value

    def counters_allreduce(self):
        self._ck(self._L.mg_counters_allreduce(self.h))

    def counters_allreduce_begin(self):
        """the exchange on a stream of its own, behind what the context's stream holds; counter-free work may follow"""
        self._ck(self._L.mg_counters_allreduce_begin(self.h))

    def counters_allreduce_end(self):
        self._ck(self._L.mg_counters_allreduce_end(self.h))

    def exchange_stats(self):
        """-> (ms of the most recent exchange, 1 if it ran in the 16-bit packed form)"""
        ms, pk = C.c_float(0), C.c_int(0)
        self._ck(self._L.mg_exchange_stats(self.h, C.byref(ms), C.byref(pk)))
        return float(ms.value), int(pk.value)

    # per-variant path
    def lookup_cover(self, rows, is_ref, sig_kmer_off, allele_sig_off):
        so = np.ascontiguousarray(sig_kmer_off, dtype=np.uint64)
        ao = np.ascontiguousarray(allele_sig_off, dtype=np.uint64)
        n_alleles, n_sigs = len(ao) - 1, len(so) - 1
        cov = np.zeros(n_alleles, dtype=np.uint32)
        if isinstance(rows, (list, tuple)) and len(rows) == 0:
            rows = np.zeros((0, 8), dtype=np.uint8)
        rows = _rows(rows)
        is_ref = np.ascontiguousarray(is_ref, dtype=np.uint8)
        self._ck(self._L.mg_lookup_cover(self.h, _p(rows), rows.shape[1], rows.shape[0], _p(is_ref), _p(so), n_sigs,
                                         _p(ao), n_alleles, _p(cov)))
        return cov

    def cover_blocks(self, blk_ref_base, blk_ref_len, blk_var_off, pos, ref_size, min_size, present, var_allele_off,
                     allele_off, pool, canon, gt, n_samples, haploid, sparse=False, sp_default=1 << 14, all_planes=False):
        """sparse: hand the genotypes over as the entries other than the word sp_default.  all_planes: every plane of a context in cohort
        mode (mg_cover_blocks_cohort), cov as [n_planes][slots]"""
        x = _blocks_host(blk_ref_base, blk_ref_len, blk_var_off, pos, ref_size, min_size, present, var_allele_off, allele_off, pool, canon, gt,
                         n_samples, sparse, sp_default)
        slots = int(var_allele_off[-1])
        cov = np.zeros((self.cohort_info()[0], slots) if all_planes else slots, dtype=np.uint32)
        ovf = np.zeros(x.n_vars, dtype=np.uint8)
        entry = self._L.mg_cover_blocks_cohort if all_planes else self._L.mg_cover_blocks
        self._ck(entry(self.h, C.byref(x), int(haploid), _p(cov), _p(ovf)))
        return cov, ovf

    def index_isolated(self, pos, var_allele_off, allele_off, pool, present_mask, flags):
        """-> overflow flags; lone short variants indexed on the device (extract_kmers + add_kmers_to_bf)"""
        a = lambda x, t: np.ascontiguousarray(x, dtype=t)
        pos, vo, ao, pool, pm, fl = a(pos, np.uint64), a(var_allele_off, np.uint32), a(allele_off, np.uint32), a(pool, np.uint8), a(present_mask, np.uint64), a(flags, np.uint8)
        n = len(pos)
        ovf = np.zeros(n, dtype=np.uint8)
        self._ck(self._L.mg_index_isolated(self.h, n, _p(pos), _p(vo), _p(ao), _p(pool), pool.size, _p(pm), _p(fl), _p(ovf)))
        return ovf

    def cut_blocks(self, pos, ref_size, min_size, contig_id):
        """-> blk_var_off (n_blocks + 1 entries) of the kept records, cut as the reference's record loops cut them"""
        a = lambda x, t: np.ascontiguousarray(x, dtype=t)
        pos, rs, ms, cid = a(pos, np.int32), a(ref_size, np.uint32), a(min_size, np.uint32), a(contig_id, np.uint32)
        n = len(pos)
        off = np.zeros(n + 1, dtype=np.uint32)
        nb = C.c_size_t(0)
        self._ck(self._L.mg_cut_blocks(self.h, n, _p(pos), _p(rs), _p(ms), _p(cid), _p(off), C.byref(nb)))
        return off[:nb.value + 1] if n else off[:0]

    # the record loop on a resident panel (device pointers; asynchronous)
    def cut_blocks_device(self, panel: PanelDev, d_blk_var_off, d_var_block, d_n_blocks):
        v = C.c_void_p
        self._ck(self._L.mg_cut_blocks_device(self.h, C.byref(panel), v(d_blk_var_off), v(d_var_block), v(d_n_blocks)))

    def cover_blocks_device(self, panel: PanelDev, d_blk_var_off, d_var_block, d_n_blocks, haploid, d_cov, d_overflow):
        v = C.c_void_p
        self._ck(self._L.mg_cover_blocks_device(self.h, C.byref(panel), v(d_blk_var_off), v(d_var_block), v(d_n_blocks), int(haploid), v(d_cov), v(d_overflow)))

    def index_blocks_device(self, panel: PanelDev, d_blk_var_off, d_var_block, d_n_blocks, haploid, d_overflow):
        v = C.c_void_p
        self._ck(self._L.mg_index_blocks_device(self.h, C.byref(panel), v(d_blk_var_off), v(d_var_block), v(d_n_blocks), int(haploid), v(d_overflow)))

    def genotype_device(self, d_cov, d_freq, d_var_allele_off, n_vars, error_rate, max_cov, haploid, d_g1, d_g2, d_gq, d_st, d_probs=None, d_gt_off=None):
        v = C.c_void_p
        self._ck(self._L.mg_genotype_device(self.h, v(d_cov), v(d_freq), v(d_var_allele_off), n_vars, C.c_float(error_rate), max_cov, int(haploid),
                                            v(d_g1), v(d_g2), v(d_gq), v(d_st), v(d_probs), v(d_gt_off)))

    def index_blocks(self, blk_ref_base, blk_ref_len, blk_var_off, pos, ref_size, min_size, present, var_allele_off,
                     allele_off, pool, canon, gt, n_samples, haploid, sparse=False, sp_default=1 << 14):
        x = _blocks_host(blk_ref_base, blk_ref_len, blk_var_off, pos, ref_size, min_size, present, var_allele_off, allele_off, pool, canon, gt,
                         n_samples, sparse, sp_default)
        ovf = np.zeros(x.n_vars, dtype=np.uint8)
        self._ck(self._L.mg_index_blocks(self.h, C.byref(x), int(haploid), _p(ovf)))
        return ovf

    def genotype(self, cov, freq, var_allele_off, error_rate, max_cov, haploid, want_probs=False):
        cov = np.ascontiguousarray(cov, dtype=np.uint32)
        freq = np.ascontiguousarray(freq, dtype=np.float32)
        vo = np.ascontiguousarray(var_allele_off, dtype=np.uint32)
        n = len(vo) - 1
        g1 = np.zeros(n, dtype=np.int32)
        g2 = np.zeros(n, dtype=np.int32)
        gq = np.zeros(n, dtype=np.int32)
        st = np.zeros(n, dtype=np.uint8)
        probs = goff = None
        if want_probs:
            A = np.diff(vo.astype(np.int64))
            ng = A if haploid else A * (A + 1) // 2
            goff = np.zeros(n + 1, dtype=np.uint64)
            goff[1:] = np.cumsum(ng)
            probs = np.zeros(int(goff[-1]), dtype=np.float64)
        self._ck(self._L.mg_genotype(self.h, _p(cov), _p(freq), _p(vo), n, C.c_float(error_rate), max_cov, int(haploid),
                                     _p(g1), _p(g2), _p(gq), _p(st), _p(probs), _p(goff)))
        return g1, g2, gq, st, probs, goff

    def reference_upload(self, ascii_bytes):
        buf = np.frombuffer(ascii_bytes, dtype=np.uint8) if isinstance(ascii_bytes, (bytes, bytearray)) else ascii_bytes
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        self._ck(self._L.mg_reference_upload(self.h, _p(buf), buf.size))

    def call_isolated(self, pos, var_allele_off, allele_off, allele_pool, freq, present_mask, flags, error_rate,
                      max_cov, haploid, want_probs=False):
        pos = np.ascontiguousarray(pos, dtype=np.uint64)
        vo = np.ascontiguousarray(var_allele_off, dtype=np.uint32)
        ao = np.ascontiguousarray(allele_off, dtype=np.uint32)
        pool = np.frombuffer(allele_pool, dtype=np.uint8) if isinstance(allele_pool, (bytes, bytearray)) else allele_pool
        pool = np.ascontiguousarray(pool, dtype=np.uint8)
        freq = np.ascontiguousarray(freq, dtype=np.float32)
        pm = np.ascontiguousarray(present_mask, dtype=np.uint64)
        fl = np.ascontiguousarray(flags, dtype=np.uint8)
        n, na = len(pos), int(vo[-1])
        cov = np.zeros(na, dtype=np.uint32)
        g1 = np.zeros(n, dtype=np.int32)
        g2 = np.zeros(n, dtype=np.int32)
        gq = np.zeros(n, dtype=np.int32)
        st = np.zeros(n, dtype=np.uint8)
        probs = goff = None
        if want_probs:
            A = np.diff(vo.astype(np.int64))
            goff = np.zeros(n + 1, dtype=np.uint64)
            goff[1:] = np.cumsum(A if haploid else A * (A + 1) // 2)
            probs = np.zeros(int(goff[-1]), dtype=np.float64)
        self._ck(self._L.mg_call_isolated(self.h, n, _p(pos), _p(vo), _p(ao), _p(pool), pool.size, _p(freq), _p(pm),
                                          _p(fl), C.c_float(error_rate), max_cov, int(haploid), _p(cov), _p(g1), _p(g2),
                                          _p(gq), _p(st), _p(probs), _p(goff)))
        if want_probs:
            return cov, g1, g2, gq, st, probs, goff
        return cov, g1, g2, gq, st

    def call_isolated_device(self, n, d_pos, d_vo, d_ao, d_pool, d_freq, d_pm, d_flags, error_rate, max_cov, haploid,
                             d_cov, d_g1, d_g2, d_gq, d_st, d_probs=None, d_gt_off=None):
        v = C.c_void_p
        self._ck(self._L.mg_call_isolated_device(self.h, n, v(d_pos), v(d_vo), v(d_ao), v(d_pool), v(d_freq), v(d_pm),
                                                 v(d_flags), C.c_float(error_rate), max_cov, int(haploid), v(d_cov),
                                                 v(d_g1), v(d_g2), v(d_gq), v(d_st), v(d_probs), v(d_gt_off)))
