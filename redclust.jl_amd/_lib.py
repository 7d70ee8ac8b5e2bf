"""ctypes binding of libredclust_hip.so (include/redclust_hip.h).  No CPU fallback: if the HIP library is
missing or no GPU is present, every compute entry point raises."""
from __future__ import annotations

import ctypes as C
import glob
import os
import subprocess

import numpy as np

from .types import KmeansResult, KmedoidsResult

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)
CSRC = os.path.join(PKG_DIR, "csrc")
SO = os.environ.get("RC_LIB_PATH") or os.path.join(CSRC, "libredclust_hip.so")   # RC_LIB_PATH: experiment builds
HEADER = os.path.join(ROOT, "include", "redclust_hip.h")

RC_OK = 0
ERRORS = {-1: "RC_ERR_ARG", -2: "RC_ERR_HIP", -3: "RC_ERR_OOM", -4: "RC_ERR_DOMAIN", -5: "RC_ERR_STATE",
          -6: "RC_ERR_CAPACITY"}


class RedClustHIPError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{ERRORS.get(code, code)}: {msg}")
        self.code = code


class RedClustDomainError(RedClustHIPError, ValueError):
    """RC_ERR_DOMAIN: the input violates what MCMCData requires (src/types.jl:145-157) — the reference throws
    ArgumentError there, so this one is a ValueError as well."""


def _check(rc, handle=None):
    """Raise the library's error for a return code other than RC_OK.  handle: the context whose error buffer holds the text
    (None: the calling thread's)."""
    if rc != RC_OK:
        raise (RedClustDomainError if rc == -4 else RedClustHIPError)(rc, lib().rc_last_error(handle).decode())


class RcParams(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("delta1", "delta2", "alpha", "beta", "zeta", "gamma", "eta", "sigma",
                                          "u", "v")] + [("maxK", C.c_int64), ("repulsion", C.c_uint8),
                                                        ("pad_", C.c_uint8 * 7)]


def _params_struct(params: dict) -> RcParams:
    g = params.get
    return RcParams(g("delta1"), g("delta2"), g("alpha"), g("beta"), g("zeta"), g("gamma"), g("eta", 1.0), g("sigma", 1.0),
                    g("u", 1.0), g("v", 1.0), int(g("maxK", 0)), int(bool(g("repulsion", True))))


class RcPairMeasures(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("ari", "ri", "mirkin", "hubert", "mi", "nmi", "vi", "ha", "hb", "id", "nid")]


class RcWbStats(C.Structure):
    _fields_ = [("count_within", C.c_int64), ("count_between", C.c_int64), ("sum_within", C.c_double),
                ("sumlog_within", C.c_double), ("sum_between", C.c_double), ("sumlog_between", C.c_double)]


class RcChainOptions(C.Structure):
    _fields_ = [("numiters", C.c_int64), ("burnin", C.c_int64), ("thin", C.c_int64), ("numGibbs", C.c_int64),
                ("numMH", C.c_int64), ("splitmerge_mode", C.c_int32), ("pad_", C.c_int32), ("seed", C.c_uint64),
                ("first_iter", C.c_uint64), ("r0", C.c_double), ("p0", C.c_double), ("proposalsd_r", C.c_double),
                ("r_trace", C.c_void_p), ("p_trace", C.c_void_p), ("max_samples", C.c_int64)]


class RcChainOutputs(C.Structure):
    _fields_ = [("clusts", C.c_void_p), ("K", C.c_void_p), ("r", C.c_void_p), ("p", C.c_void_p), ("loglik", C.c_void_p),
                ("logposterior", C.c_void_p), ("r_acceptances", C.c_void_p), ("splitmerge_acceptances", C.c_void_p),
                ("splitmerge_splits", C.c_void_p), ("r_all", C.c_void_p), ("p_all", C.c_void_p),
                ("num_samples", C.c_int64), ("runtime_s", C.c_double), ("r_final", C.c_double), ("p_final", C.c_double)]


class RcChainsInput(C.Structure):
    _fields_ = [("n", C.c_int64), ("D", C.c_void_p), ("logD_or_null", C.c_void_p), ("points", C.c_void_p), ("dim", C.c_int64),
                ("storage_bits", C.c_int32), ("pad_", C.c_int32), ("kcap", C.c_int64), ("params", C.POINTER(RcParams)),
                ("init_clusts", C.c_void_p)]


class RcPsmRun(C.Structure):
    _fields_ = [("loss", C.c_double), ("loss_num", C.c_int64), ("sweeps", C.c_int32), ("converged", C.c_int32),
                ("moves", C.c_int64), ("K", C.c_int32)]


class RcPearRun(C.Structure):
    _fields_ = [("pear", C.c_double), ("num", C.c_int64), ("den", C.c_int64), ("sweeps", C.c_int32), ("converged", C.c_int32),
                ("moves", C.c_int64), ("K", C.c_int32)]


class RcMapRun(C.Structure):
    _fields_ = [("loglik", C.c_double), ("logprior", C.c_double), ("logposterior", C.c_double), ("start_logposterior", C.c_double),
                ("sweeps", C.c_int32), ("converged", C.c_int32), ("K", C.c_int32), ("capped", C.c_int32), ("moves", C.c_int64)]


class RcSweepStats(C.Structure):
    _fields_ = [("n_changes", C.c_int64), ("n_rounds", C.c_int64), ("K", C.c_int64)]


def _compile(so, defines=(), verbose=False) -> str:
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared"] + [f"-D{d}" for d in defines] + \
          ["-o", so, os.path.join(CSRC, "redclust_hip.hip")]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd, cwd=CSRC)
    return so


def _sources() -> list:
    """what the library is built from: the translation unit, every include beside it, the header"""
    return [os.path.join(CSRC, "redclust_hip.hip")] + sorted(glob.glob(os.path.join(CSRC, "*.inc.hip"))) + \
           sorted(glob.glob(os.path.join(CSRC, "*.inc.hpp"))) + [HEADER]


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU) unless it is newer than its sources."""
    if not force and os.path.exists(SO) and all(os.path.getmtime(SO) >= os.path.getmtime(s) for s in _sources()):
        return SO
    return _compile(SO, verbose=verbose)


def build_diag(extra_defines=(), name="libredclust_hip_diag.so", verbose: bool = False) -> str:
    """The tuning / diagnostic build (-DRC_DIAG: the RC_* environment switches INTEGRATION.md lists as diagnostic exist only
    here; extra_defines e.g. ("RC_CHAOS=15",), ("RC_POISON",)).  Written to build_exp/ (git- and gpurun-ignored: build it on
    the box that uses it, select it with RC_LIB_PATH)."""
    out_dir = os.path.join(ROOT, "build_exp")
    os.makedirs(out_dir, exist_ok=True)
    return _compile(os.path.join(out_dir, name), ("RC_DIAG", *extra_defines), verbose)


# include/redclust_hip.h's RC_METRIC_* by their names (SciPy's and Distances.jl's)
METRICS = {"euclidean": 0, "sqeuclidean": 1, "cityblock": 2, "chebyshev": 3, "cosine": 4, "correlation": 5}


def check_metric(metric, dim=None) -> str:
    """The metric's name, or a ValueError before the library is touched: an unknown name; correlation with dim < 2."""
    if not isinstance(metric, str) or metric not in METRICS:
        raise ValueError(f"unknown metric {metric!r}: one of {', '.join(METRICS)}")
    if metric == "correlation" and dim is not None and dim < 2:
        raise ValueError("the correlation metric needs dim >= 2: a single coordinate has nothing left after centring")
    return metric


_dp = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_ip = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
_up = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")

# every symbol include/redclust_hip.h declares, with its ctypes signature
SIGNATURES = {
    "rc_create": (C.c_int32, [C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_void_p)]),
    "rc_create_from_points": (C.c_int32, [C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_void_p)]),
    "rc_create_from_points_metric": (C.c_int32, [C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                                 C.POINTER(C.c_void_p)]),
    "rc_pairwise": (C.c_int32, [C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                C.POINTER(C.c_double)]),
    "rc_get_matrix": (C.c_int32, [C.c_void_p, C.c_int32, _dp]),
    "rc_get_matrix_rows": (C.c_int32, [C.c_void_p, C.c_int32, _ip, C.c_int64, _dp]),
    "rc_destroy": (C.c_int32, [C.c_void_p]),
    "rc_last_error": (C.c_char_p, [C.c_void_p]),
    "rc_set_params": (C.c_int32, [C.c_void_p, C.POINTER(RcParams)]),
    "rc_set_state": (C.c_int32, [C.c_void_p, _ip]),
    "rc_get_state": (C.c_int32, [C.c_void_p, C.c_void_p, _ip, C.POINTER(C.c_int64)]),
    "rc_gibbs_sweep": (C.c_int32, [C.c_void_p, C.c_double, C.c_double, C.c_uint64, C.c_uint64]),
    "rc_gibbs_sweep_async": (C.c_int32, [C.c_void_p, C.c_double, C.c_double, C.c_uint64, C.c_uint64]),
    "rc_last_sweep_stats": (C.c_int32, [C.c_void_p, C.POINTER(RcSweepStats)]),
    "rc_synchronize": (C.c_int32, [C.c_void_p]),
    "rc_loglik": (C.c_int32, [C.c_void_p, C.POINTER(C.c_double)]),
    "rc_logprior": (C.c_int32, [C.c_void_p, C.c_double, C.c_double, C.POINTER(C.c_double)]),
    "rc_record_sample": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "rc_cocluster": (C.c_int32, [C.c_void_p, _dp, C.c_int64]),
    "rc_cocluster_counts": (C.c_int32, [C.c_void_p, _up]),
    "rc_cocluster_device_buffer": (C.c_int32, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "rc_cocluster_reset": (C.c_int32, [C.c_void_p]),
    "rc_set_mode": (C.c_int32, [C.c_void_p, C.c_int32]),
    "rc_attach_host_matrices": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rc_splitmerge": (C.c_int32, [C.c_void_p, C.c_double, C.c_double, C.c_int64, C.c_uint64, C.c_uint64, C.c_uint64,
                                  C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]),
    "rc_state_checkpoint": (C.c_int32, [C.c_void_p]),
    "rc_state_restore": (C.c_int32, [C.c_void_p]),
    "rc_debug_rowsums": (C.c_int32, [C.c_void_p, C.c_int64, _ip, _ip, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "rc_debug_rowtotals": (C.c_int32, [C.c_void_p, _ip, _ip]),
    "rc_debug_flog": (C.c_int32, [C.c_void_p, C.c_int32, _dp, C.c_int64, _dp]),
    "rc_bulk_kernel_info": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "rc_set_bulk_kernel": (C.c_int32, [C.c_void_p, C.c_int32]),
    "rc_set_option": (C.c_int32, [C.c_void_p, C.c_char_p, C.c_int64]),
    "rc_bulk_kernel_name": (C.c_char_p, [C.c_void_p]),
    "rc_log_table_folded": (C.c_int32, [C.c_void_p]),
    "rc_within_between": (C.c_int32, [C.c_void_p, C.POINTER(RcWbStats)]),
    "rc_run_chain": (C.c_int32, [C.c_void_p, C.POINTER(RcChainOptions), C.POINTER(RcChainOutputs)]),
    "rc_comm_unique_id": (C.c_int32, [C.c_void_p]),
    "rc_comm_create": (C.c_int32, [C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]),
    "rc_comm_destroy": (C.c_int32, [C.c_void_p]),
    "rc_comm_allreduce_counts": (C.c_int32, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                             C.POINTER(C.c_double)]),
    "rc_run_chains": (C.c_int32, [C.c_int32, C.POINTER(C.c_int32), C.POINTER(RcChainsInput), C.POINTER(RcChainOptions),
                                  C.POINTER(RcChainOutputs), C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "rc_measure_read_ceiling": (C.c_int32, [C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_double)]),
    "rc_scalar_updates": (C.c_int32, [C.c_uint64, C.c_uint64, C.c_double, C.c_double, _ip, C.c_int64, C.c_int64, C.c_double,
                                      C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.POINTER(C.c_uint8)]),
    "rc_loss_matrix": (C.c_int32, [C.c_int32, _ip, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                   C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "rc_pair_measures": (C.c_int32, [C.c_int32, _ip, _ip, C.c_int64, C.POINTER(RcPairMeasures)]),
    "rc_kmedoids": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64, C.c_double, C.c_uint64, _ip, _ip, C.POINTER(C.c_double),
                                C.POINTER(C.c_int64), C.POINTER(C.c_uint8)]),
    "rc_kmedoids_scan": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_uint64, _dp, _ip,
                                     np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")]),
    "rc_kmedoids_scan_split": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_uint64, _dp, _ip,
                                           np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS"), C.POINTER(RcWbStats)]),
    "rc_kmeans": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64, C.c_double, C.c_uint64, C.c_void_p, _ip, _dp, _dp, _ip,
                              C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)]),
    "rc_kmeans_scan": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_uint64, C.c_int64, _dp, _ip,
                                   np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")]),
    "rc_kmeans_scan_split": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_uint64, C.c_int64, _dp, _ip,
                                         np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS"), C.POINTER(RcWbStats)]),
    "rc_sample_k": (C.c_int32, [C.c_int32, C.c_int64, C.c_int64, _dp, _dp, C.c_uint64, _ip, C.POINTER(C.c_double)]),
    "rc_oracle_coclustering": (C.c_int32, [C.c_int32, C.c_int64, C.c_int64, _dp, C.c_int64, C.c_double, C.c_double, C.c_int64,
                                           _dp, C.c_int64, _dp, C.POINTER(C.c_double)]),
    "rc_psm_search": (C.c_int32, [C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                  C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "rc_psm_search_ctx": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                      C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "rc_pear_search": (C.c_int32, [C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                   C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "rc_pear_search_ctx": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                       C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "rc_pear_search_samples": (C.c_int32, [C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                           C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                           C.POINTER(C.c_double)]),
    "rc_vi_gtable": (C.c_int32, [C.c_int64, C.c_void_p]),
    "rc_vi_search": (C.c_int32, [C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                 C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "rc_id_search": (C.c_int32, [C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                 C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "rc_vi_search_groups": (C.c_int32, [C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    "rc_samples_counts": (C.c_int32, [C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.POINTER(C.c_double)]),
    "rc_psm_search_samples": (C.c_int32, [C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                          C.POINTER(C.c_double)]),
    "rc_hclust": (C.c_int32, [C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                              C.POINTER(C.c_double)]),
    "rc_hclust_samples": (C.c_int32, [C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                      C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "rc_hclust_ctx": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                  C.POINTER(C.c_double)]),
    "rc_hclust_cut": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "rc_psm_expected_loss": (C.c_int32, [C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.POINTER(C.c_double)]),
    "rc_psm_expected_loss_ctx": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.POINTER(C.c_double)]),
    "rc_predict": (C.c_int32, [C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.POINTER(RcParams), C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    "rc_predict_points": (C.c_int32, [C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.POINTER(RcParams), C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    "rc_predict_points_metric": (C.c_int32, [C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.POINTER(RcParams), C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    "rc_predict_joint": (C.c_int32, [C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.POINTER(RcParams), C.c_int64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    "rc_partition_distances": (C.c_int32, [C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    "rc_relabel": (C.c_int32, [C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                               C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    "rc_score_labellings": (C.c_int32, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RcParams), C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_double)]),
    "rc_loglik_from_blocks": (C.c_int32, [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(RcParams),
                                          C.POINTER(C.c_double)]),
    "rc_cluster_profiles": (C.c_int32, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "rc_map_search": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RcParams), C.c_int32,
                                  C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "rc_layout_info": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "rc_bulk_plan_info": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "rc_event_overhead_ms": (C.c_int32, [C.c_void_p, C.POINTER(C.c_double)]),
    "rc_kernel_timing": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "rc_capacity_info": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "rc_chain_stats": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
}

_lib = None


def lib():
    """Load the in-tree HIP library; fails loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO):
            raise RedClustHIPError(-2, f"{SO} not built — run `python -c 'import __graft_entry__ as g; g.build()'` "
                                       "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        L = C.CDLL(SO)
        for name, (res, args) in SIGNATURES.items():
            if os.environ.get("RC_LIB_PATH") and not hasattr(L, name):
                continue   # experiment builds of older sources lack the newest entry points
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


class Context:
    """Owns one rc_ctx: device-resident D/logD (fixed point), the label state and the sweep kernels."""

    def __init__(self, D: np.ndarray, logD: np.ndarray | None = None, device: int = 0, kcap: int = 0,
                 storage_bits: int = 64):
        self.L = lib()
        D = np.ascontiguousarray(D, dtype=np.float64)
        if D.ndim != 2 or D.shape[0] != D.shape[1]:
            raise ValueError("D must be a square matrix.")  # types.jl:152-154
        self.n = int(D.shape[0])
        lp = None
        if logD is not None:
            logD = np.ascontiguousarray(logD, dtype=np.float64)
            assert logD.shape == D.shape
            lp = logD.ctypes.data_as(C.c_void_p)
        h = C.c_void_p()
        _check(self.L.rc_create(self.n, D.ctypes.data_as(C.c_void_p), lp, storage_bits, device, kcap, C.byref(h)))
        self.h = h

    @classmethod
    def from_points(cls, points, device: int = 0, kcap: int = 0, storage_bits: int = 64, metric=None):
        """MCMCData(points) on the device: the pairwise distances are computed there.  metric None: Euclidean as the reference
        evaluates it (types.jl:159-162, rc_create_from_points).  A name of METRICS: the matrix of pairwise(points, metric=...)
        (rc_create_from_points_metric; "euclidean" is then predict_points' direct-difference arithmetic).  The context
        remembers .metric; its k-means entry points stay Euclidean on the points themselves."""
        pts = np.ascontiguousarray(points, dtype=np.float64)
        if pts.ndim != 2:
            raise ValueError("points must be an n×dim array (one observation per row)")
        if metric is not None:
            check_metric(metric, int(pts.shape[1]))
        self = cls.__new__(cls)
        self.L = lib()
        self.n = int(pts.shape[0])
        self.dim = int(pts.shape[1])
        self.metric = metric
        h = C.c_void_p()
        if metric is None:
            _check(self.L.rc_create_from_points(self.n, int(pts.shape[1]), pts.ctypes.data_as(C.c_void_p), storage_bits, device,
                                                kcap, C.byref(h)))
        else:
            _check(self.L.rc_create_from_points_metric(self.n, int(pts.shape[1]), pts.ctypes.data_as(C.c_void_p), METRICS[metric],
                                                       storage_bits, device, kcap, C.byref(h)))
        self.h = h
        return self

    def get_matrix(self, which=0):
        out = np.zeros((self.n, self.n))
        self._chk(self.L.rc_get_matrix(self.h, int(which), out.reshape(-1)))
        return out

    def get_matrix_rows(self, which, rows):
        """rows (0-based, caller's order) of the device's D (which=0) or logD (which=1) as an len(rows)×n array"""
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        out = np.zeros((len(rows), self.n))
        if len(rows):
            self._chk(self.L.rc_get_matrix_rows(self.h, int(which), rows, len(rows), out.reshape(-1)))
        return out

    def _chk(self, rc):
        _check(rc, self.h)

    def close(self):
        if getattr(self, "h", None):
            self.L.rc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, delta1, delta2, alpha, beta, zeta, gamma, eta=1.0, sigma=1.0, u=1.0, v=1.0,
                   repulsion=True, maxK=0, **_ignored):
        P = _params_struct(dict(delta1=delta1, delta2=delta2, alpha=alpha, beta=beta, zeta=zeta, gamma=gamma, eta=eta, sigma=sigma,
                                u=u, v=v, repulsion=repulsion, maxK=maxK))
        self._chk(self.L.rc_set_params(self.h, C.byref(P)))

    def set_state(self, clusts):
        c = np.ascontiguousarray(clusts, dtype=np.int64)
        if c.shape != (self.n,):
            raise ValueError("clusts must have length n")
        self._chk(self.L.rc_set_state(self.h, c))

    def get_state(self, want_labels=True):
        """(clusts, clustsizes, K); with want_labels=False clusts is None and nothing is copied from the device."""
        clusts = np.zeros(self.n, np.int64) if want_labels else None
        sizes = np.zeros(self.n, np.int64)
        K = C.c_int64()
        self._chk(self.L.rc_get_state(self.h, clusts.ctypes.data_as(C.c_void_p) if want_labels else None, sizes,
                                      C.byref(K)))
        return clusts, sizes, K.value

    def gibbs_sweep(self, r, p, seed, sweep_index, blocking=True):
        fn = self.L.rc_gibbs_sweep if blocking else self.L.rc_gibbs_sweep_async
        self._chk(fn(self.h, float(r), float(p), int(seed), int(sweep_index)))

    def set_mode(self, mode):
        """'full' (recompute the row-sum table every sweep, the reference's data flow) or 'incremental' (maintain it
        by exact corrections only); results are bit-identical."""
        self._chk(self.L.rc_set_mode(self.h, {"full": 0, "incremental": 1}[mode]))

    def synchronize(self):
        self._chk(self.L.rc_synchronize(self.h))

    def sweep_stats(self):
        s = RcSweepStats()
        self._chk(self.L.rc_last_sweep_stats(self.h, C.byref(s)))
        return dict(n_changes=s.n_changes, n_rounds=s.n_rounds, K=s.K)

    def loglik(self):
        out = C.c_double()
        self._chk(self.L.rc_loglik(self.h, C.byref(out)))
        return out.value

    def logprior(self, r, p):
        out = C.c_double()
        self._chk(self.L.rc_logprior(self.h, float(r), float(p), C.byref(out)))
        return out.value

    def record_sample(self, want_labels=True):
        if want_labels:
            out = np.zeros(self.n, np.int64)
            self._chk(self.L.rc_record_sample(self.h, out.ctypes.data_as(C.c_void_p)))
            return out
        self._chk(self.L.rc_record_sample(self.h, None))
        return None

    def cocluster(self, numsamples):
        out = np.zeros((self.n, self.n))
        self._chk(self.L.rc_cocluster(self.h, out.reshape(-1), int(numsamples)))
        return out

    def cocluster_counts(self):
        out = np.zeros((self.n, self.n), np.uint32)
        self._chk(self.L.rc_cocluster_counts(self.h, out.reshape(-1)))
        return out

    def cocluster_device_buffer(self):
        p = C.c_void_p()
        ld = C.c_int64()
        self._chk(self.L.rc_cocluster_device_buffer(self.h, C.byref(p), C.byref(ld)))
        return p.value, ld.value

    def cocluster_reset(self):
        self._chk(self.L.rc_cocluster_reset(self.h))

    def attach_host_matrices(self, D, logD=None):
        """Borrow the caller's host matrices for the split–merge scans; they must outlive the context's use."""
        self._hostD = np.ascontiguousarray(D, dtype=np.float64)
        self._hostL = None if logD is None else np.ascontiguousarray(logD, dtype=np.float64)
        self._chk(self.L.rc_attach_host_matrices(self.h, self._hostD.ctypes.data_as(C.c_void_p),
                                                 None if self._hostL is None else self._hostL.ctypes.data_as(C.c_void_p)))

    def splitmerge(self, r, p, numGibbs, seed, it, mh_counter):
        a, s = C.c_uint8(), C.c_uint8()
        self._chk(self.L.rc_splitmerge(self.h, float(r), float(p), int(numGibbs), int(seed), int(it), int(mh_counter),
                                       C.byref(a), C.byref(s)))
        return bool(a.value), bool(s.value)

    def checkpoint(self):
        self._chk(self.L.rc_state_checkpoint(self.h))

    def restore(self):
        self._chk(self.L.rc_state_restore(self.h))

    def debug_rowsums(self, label):
        sd = np.zeros(self.n, np.int64)
        sl = np.zeros(self.n, np.int64)
        eD, eL = C.c_int32(), C.c_int32()
        self._chk(self.L.rc_debug_rowsums(self.h, int(label), sd, sl, C.byref(eD), C.byref(eL)))
        return sd, sl, eD.value, eL.value

    def debug_rowtotals(self):
        """rc_debug_rowtotals: (Σ_j Dq[i,j], Σ_j Lq[i,j]) of every row, fixed point, by a kernel independent of the row reductions."""
        td = np.zeros(self.n, np.int64)
        tl = np.zeros(self.n, np.int64)
        self._chk(self.L.rc_debug_rowtotals(self.h, td, tl))
        return td, tl

    def debug_flog(self, which, x):
        """rc_debug_flog: the sweep kernel's own log (which = 0), log1p (1) or -log(-log(x)) (2) of every entry of x, on the device."""
        x = np.ascontiguousarray(x, np.float64)
        out = np.zeros_like(x)
        self._chk(self.L.rc_debug_flog(self.h, int(which), x, x.size, out))
        return out

    def bulk_kernel_info(self):
        w, b = C.c_int32(), C.c_double()
        self._chk(self.L.rc_bulk_kernel_info(self.h, C.byref(w), C.byref(b)))
        return ("k_bulk_sym" if w.value else "k_bulk"), b.value

    def bulk_kernel_name(self) -> str:
        return self.L.rc_bulk_kernel_name(self.h).decode()

    def log_table_folded(self) -> bool:
        """rc_log_table_folded: k_bulk_syml2 reads the log table with the exponent folded in (False: k_bulk_syml2w derives it per entry)."""
        return bool(self.L.rc_log_table_folded(self.h))

    def set_bulk_kernel(self, which):
        self._chk(self.L.rc_set_bulk_kernel(self.h, {"auto": -1, "perm": 0, "sym": 1}[which]))

    def set_option(self, name, value):
        """rc_set_option: "prune" (-1 automatic / 0 / 1), "lds_point_cache" (0 / 1), "chain_workers", "chain_depth" (0 = automatic), "chain_pipeline" (0 / 1),
        "fold_log_table" (1 / 0: 0 keeps a derived context on k_bulk_syml2w, the row reduction that derives the exponent per entry),
        "syml2_unit_rows" (tests: 0 automatic, or 8..128 rows per work unit of k_bulk_syml2; plans its unit lists again)."""
        self._chk(self.L.rc_set_option(self.h, name.encode(), int(value)))

    def run_chain(self, numiters, burnin, thin, numGibbs, numMH, seed, r0, p0, proposalsd_r, splitmerge="as_written",
                  rp_trace=None, first_iter=0):
        """rc_run_chain: the whole iteration loop natively.  Returns a dict of numpy arrays (MCMCResult fields)."""
        ns = max((numiters - burnin) // thin, 0) if thin > 0 else 0   # thin <= 0 is rejected by the library
        n = self.n
        res = dict(clusts=np.zeros((ns, n), np.int64), K=np.zeros(ns, np.int64), r=np.zeros(ns), p=np.zeros(ns),
                   loglik=np.zeros(ns), logposterior=np.zeros(ns), r_acceptances=np.zeros(numiters, np.uint8),
                   splitmerge_acceptances=np.zeros(numiters * numMH, np.uint8),
                   splitmerge_splits=np.zeros(numiters * numMH, np.uint8), r_all=np.zeros(numiters), p_all=np.zeros(numiters))
        o = RcChainOptions(numiters, burnin, thin, numGibbs, numMH, {"as_written": 0, "intended": 1}[splitmerge], 0,
                           int(seed), int(first_iter), float(r0), float(p0), float(proposalsd_r), None, None, ns)
        keep = []
        if rp_trace is not None:
            rt = np.ascontiguousarray(rp_trace[0], dtype=np.float64)
            pt = np.ascontiguousarray(rp_trace[1], dtype=np.float64)
            assert len(rt) >= numiters and len(pt) >= numiters
            keep = [rt, pt]
            o.r_trace, o.p_trace = rt.ctypes.data, pt.ctypes.data
        out = RcChainOutputs()
        for k in ("clusts", "K", "r", "p", "loglik", "logposterior", "r_acceptances", "splitmerge_acceptances",
                  "splitmerge_splits", "r_all", "p_all"):
            setattr(out, k, res[k].ctypes.data if res[k].size else None)
        self._chk(self.L.rc_run_chain(self.h, C.byref(o), C.byref(out)))
        del keep
        res["num_samples"], res["runtime_s"] = int(out.num_samples), float(out.runtime_s)
        res["r_final"], res["p_final"] = float(out.r_final), float(out.p_final)
        for k in ("r_acceptances", "splitmerge_acceptances", "splitmerge_splits"):
            res[k] = res[k].astype(bool)
        return res

    def capacity_info(self) -> dict:
        """Slot capacity now, its ceiling min(n, 32767) (wide beyond 4096 slots), growths so far, the resolver's batch capacity."""
        v = [C.c_int64(0) for _ in range(4)]
        self._chk(self.L.rc_capacity_info(self.h, *[C.byref(x) for x in v]))
        return dict(kcap=int(v[0].value), kcap_max=int(v[1].value), n_grows=int(v[2].value), batch_capacity=int(v[3].value))

    def chain_stats(self) -> dict:
        """Counters of the last run_chain: rollbacks of the speculative pipeline, off-line split evaluations, worker threads,
        capacity growths."""
        v = [C.c_int64(0) for _ in range(4)]
        self._chk(self.L.rc_chain_stats(self.h, *[C.byref(x) for x in v]))
        return dict(rollbacks=int(v[0].value), split_evals=int(v[1].value), workers=int(v[2].value), grows=int(v[3].value))

    def within_between(self) -> dict:
        """rc_within_between: |A|, ΣA, Σlog A and |B|, ΣB, Σlog B of fitprior's split under the current labels."""
        o = RcWbStats()
        self._chk(self.L.rc_within_between(self.h, C.byref(o)))
        return {k: getattr(o, k) for k, _ in RcWbStats._fields_}

    def kmedoids(self, k, maxiter=200, tol=1e-8, seed=0) -> KmedoidsResult:
        """rc_kmedoids: Clustering.jl's kmedoids(D, k; maxiter, tol) (k-medoids++ seeding) on the device's D; the state is untouched."""
        a = np.zeros(self.n, np.int64)
        m = np.zeros(max(int(k), 0), np.int64)
        tc, it, cv = C.c_double(), C.c_int64(), C.c_uint8()
        self._chk(self.L.rc_kmedoids(self.h, int(k), int(maxiter), float(tol), int(seed) & 0xFFFFFFFFFFFFFFFF, a,
                                     m if m.size else np.zeros(1, np.int64), C.byref(tc), C.byref(it), C.byref(cv)))
        return KmedoidsResult(medoids=m, assignments=a, totalcost=tc.value, iterations=int(it.value), converged=bool(cv.value))

    def _scan(self, name, kmin, kmax, maxiter, tol, seed, split, *extra) -> dict:
        """rc_<name>_scan(ctx, kmin, kmax, maxiter, tol, seed, *extra, outputs) or, with split, rc_<name>_scan_split."""
        m = max(int(kmax) - int(kmin) + 1, 1)
        tc, it, cv = np.zeros(m), np.zeros(m, np.int64), np.zeros(m, np.uint8)
        args = (self.h, int(kmin), int(kmax), int(maxiter), float(tol), int(seed) & 0xFFFFFFFFFFFFFFFF, *extra, tc, it, cv)
        if not split:
            self._chk(getattr(self.L, f"rc_{name}_scan")(*args))
            return dict(totalcost=tc, iterations=it, converged=cv.astype(bool))
        wb = (RcWbStats * m)()
        self._chk(getattr(self.L, f"rc_{name}_scan_split")(*args, wb))
        out = dict(totalcost=tc, iterations=it, converged=cv.astype(bool))
        for k, ty in RcWbStats._fields_:
            out[k] = np.array([getattr(x, k) for x in wb], dtype=np.int64 if ty is C.c_int64 else np.float64)
        return out

    def kmedoids_scan(self, kmin, kmax, maxiter=200, tol=1e-8, seed=0, split=False) -> dict:
        """rc_kmedoids_scan: totalcost, iterations and converged of kmedoids(k) for k = kmin..kmax (arrays indexed by k - kmin).
        split=True (rc_kmedoids_scan_split): also every k's within / between split of its final assignment, as within_between
        would return it — count_within, sum_within, sumlog_within and the same three _between, one array each."""
        return self._scan("kmedoids", kmin, kmax, maxiter, tol, seed, split)

    def kmeans(self, k, maxiter=100, tol=1e-6, seed=0, init=None) -> KmeansResult:
        """rc_kmeans: Clustering.jl's kmeans(X, k; maxiter, tol) (k-means++ seeding, or init: k distinct 1-based point indices)
        on the points of a context made by from_points; the state is untouched."""
        k = int(k)
        dim = getattr(self, "dim", 0)
        a, costs = np.zeros(self.n, np.int64), np.zeros(self.n)
        cen, cnt = np.zeros((max(k, 1), max(dim, 1))), np.zeros(max(k, 1), np.int64)
        ip = None
        if init is not None:
            init = np.ascontiguousarray(init, dtype=np.int64)
            if init.shape != (k,):
                raise ValueError("init must hold k point indices")
            ip = init.ctypes.data_as(C.c_void_p)
        tc, it, cv = C.c_double(), C.c_int64(), C.c_uint8()
        self._chk(self.L.rc_kmeans(self.h, k, int(maxiter), float(tol), int(seed) & 0xFFFFFFFFFFFFFFFF, ip, a, cen.reshape(-1),
                                   costs, cnt, C.byref(tc), C.byref(it), C.byref(cv)))
        return KmeansResult(centers=cen[:k, :dim], assignments=a, costs=costs, counts=cnt[:k], totalcost=tc.value,
                            iterations=int(it.value), converged=bool(cv.value))

    def kmeans_scan(self, kmin, kmax, maxiter=100, tol=1e-6, seed=0, split=False, slots_per_chunk=0) -> dict:
        """rc_kmeans_scan: totalcost, iterations and converged of kmeans(k) for k = kmin..kmax (arrays indexed by k - kmin);
        split=True (rc_kmeans_scan_split): also every k's within / between split of the context's D under its final
        assignment, as kmedoids_scan returns it.  slots_per_chunk: runs per device pass (0 = automatic; same results)."""
        return self._scan("kmeans", kmin, kmax, maxiter, tol, seed, split, int(slots_per_chunk))

    def score(self, labellings, r=None, p=None, params=None, want_blocks=False) -> dict:
        """rc_score_labellings: the log-likelihood of each of L labellings (L×n int64 labels in 1..n, or one labelling) under
        the model, against this context's matrices; its state, layout and counts are untouched.  r, p: one value per labelling
        (or None: no log-prior); params: a dict of hyperparameters (None: the context's).  Returns a dict: loglik (L), logprior
        and logposterior = loglik + logprior (L, or None without r and p), K (L), sizes (a list of L int64 arrays: the cluster
        sizes in ascending label order), blocks (with want_blocks a list of L int64 arrays K(K+1)/2 × 4: the upper-triangle
        block sums (D_hi, D_lo, L_hi, L_lo) in row-major (k, t >= k) order, value = hi·2^24 + lo; else None), eD, eL (the
        exponents loglik_from_blocks takes), kernel_ms."""
        lab = np.ascontiguousarray(labellings, dtype=np.int64)
        if lab.ndim == 1:
            lab = lab[None, :]
        if lab.ndim != 2 or lab.shape[1] != self.n:
            raise ValueError("labellings must be an L×n matrix of labels with the context's n columns")
        nl = lab.shape[0]
        if (r is None) != (p is None):
            raise ValueError("give both r and p, or neither")
        if r is not None:
            r = np.ascontiguousarray(np.broadcast_to(np.asarray(r, dtype=np.float64).reshape(-1), (nl,)))
            p = np.ascontiguousarray(np.broadcast_to(np.asarray(p, dtype=np.float64).reshape(-1), (nl,)))
        prm = None if params is None else _params_struct(params)
        valid = lab.size > 0 and lab.min() >= 1 and lab.max() <= self.n            # otherwise the library names the label
        sizes = [np.bincount(row, minlength=self.n + 1)[1:] for row in lab] if valid else []
        sizes = [z[z > 0].astype(np.int64) for z in sizes]
        nblocks = sum(len(z) * (len(z) + 1) // 2 for z in sizes) if want_blocks else 0
        ll, K = np.zeros(max(nl, 1)), np.zeros(max(nl, 1), np.int64)
        lp = np.zeros(max(nl, 1)) if r is not None else None
        blocks = np.zeros((max(nblocks, 1), 4), np.int64) if want_blocks else None
        eD, eL, ms = C.c_int32(), C.c_int32(), C.c_double()
        self._chk(self.L.rc_score_labellings(self.h, nl, lab.ctypes.data, None if r is None else r.ctypes.data,
                                             None if p is None else p.ctypes.data, None if prm is None else C.byref(prm),
                                             ll.ctypes.data, None if lp is None else lp.ctypes.data, K.ctypes.data,
                                             None if blocks is None else blocks.ctypes.data, nblocks, C.byref(eD), C.byref(eL),
                                             C.byref(ms)))
        per = None
        if want_blocks:
            off = np.concatenate([[0], np.cumsum([len(z) * (len(z) + 1) // 2 for z in sizes])])
            per = [blocks[off[i]:off[i + 1]] for i in range(nl)]
        return dict(loglik=ll[:nl], logprior=None if lp is None else lp[:nl], logposterior=None if lp is None else ll[:nl] + lp[:nl],
                    K=K[:nl], sizes=sizes, blocks=per, eD=int(eD.value), eL=int(eL.value), kernel_ms=float(ms.value))

    def map_search(self, init, order, r, p, params=None, maxK: int = 0, maxsweeps: int = 100, want_state: bool = False) -> dict:
        """rc_map_search: the greedy search over all partitions for the labelling of maximum log-posterior under this context's
        matrices; its state, layout and counts are untouched.  init: nruns×n labels (0 = unallocated); order: nruns×n 1-based
        permutations; r, p: a scalar or one value per run; params: a dict of hyperparameters (None: the context's).  Returns a
        dict: labels (nruns×n, sortlabels'd), the per-run arrays loglik, logprior, logposterior (rc_score_labellings' values of
        labels), start_logposterior (NaN for a start with unallocated points), sweeps, converged, K, capped, moves, and best
        (the first run of maximal logposterior), kernel_ms, Kcap (the slot cap); with want_state also blocks (nruns×Kcap×Kcap×4
        int64: the kernel's own final cells (D_hi, D_lo, L_hi, L_lo) by ordered pair of slots, value = hi·2^24 + lo) and
        slots (nruns×n: the kernel's final 1-based slots) — else None."""
        init = np.ascontiguousarray(init, dtype=np.int64)
        order = np.ascontiguousarray(order, dtype=np.int32)
        if init.ndim != 2 or init.shape != order.shape or init.shape[1] != self.n:
            raise ValueError("init and order must be nruns×n arrays of the same shape, n the context's")
        nruns, n = init.shape
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(r, dtype=np.float64).reshape(-1), (nruns,)))
        p = np.ascontiguousarray(np.broadcast_to(np.asarray(p, dtype=np.float64).reshape(-1), (nruns,)))
        prm = None if params is None else _params_struct(params)
        Kcap = int(maxK) if int(maxK) > 0 else min(n, 1024)
        labels = np.zeros((max(nruns, 1), n), np.int64)
        runs = (RcMapRun * max(nruns, 1))()
        state = want_state and 1 <= Kcap <= 1024 and n <= 8192                     # otherwise the library refuses the call
        blocks = np.zeros((max(nruns, 1), Kcap, Kcap, 4), np.int64) if state else None
        slots = np.zeros((max(nruns, 1), n), np.int64) if state else None
        best, ms = C.c_int32(-1), C.c_double()
        self._chk(self.L.rc_map_search(self.h, nruns, init.ctypes.data, order.ctypes.data, r.ctypes.data, p.ctypes.data,
                                       None if prm is None else C.byref(prm), int(maxK), int(maxsweeps), labels.ctypes.data, runs,
                                       None if blocks is None else blocks.ctypes.data, None if slots is None else slots.ctypes.data,
                                       C.byref(best), C.byref(ms)))
        out = dict(labels=labels[:nruns], best=int(best.value), kernel_ms=float(ms.value), Kcap=Kcap,
                   blocks=None if blocks is None else blocks[:nruns], slots=None if slots is None else slots[:nruns])
        for k, ty in RcMapRun._fields_:
            out[k] = np.array([getattr(x, k) for x in runs[:nruns]], dtype=np.float64 if ty is C.c_double else np.int64)
        out["converged"] = out["converged"].astype(bool)
        return out

    def profiles(self, labellings, points=True) -> dict:
        """rc_cluster_profiles: the medoids and the per-point sums behind the silhouette of each of L labellings (L×n int64
        labels in 1..n, or one labelling), against this context's D; its state, layout and counts are untouched and it needs
        neither parameters nor a state.  All in exact integers of Dq = D·2^eD, the diagonal never counted.  Returns a dict:
        K (L); labels, sizes (lists of L int64 arrays: the cluster names in ascending order and their sizes); medoids (a
        list of L int64 arrays, 1-based: per cluster its member of least within, the smallest index on ties), medoid_within
        (likewise, that least within); with points also within, nearest, neighbour (L×n int64: Σ Dq to the other members of
        the own cluster; Σ Dq to the members of the neighbour cluster — the other cluster of least mean, compared exactly, the
        smaller label on ties; that cluster's label, 0 with one cluster) — else None; eD, kernel_ms."""
        lab = np.ascontiguousarray(labellings, dtype=np.int64)
        if lab.ndim == 1:
            lab = lab[None, :]
        if lab.ndim != 2 or lab.shape[1] != self.n:
            raise ValueError("labellings must be an L×n matrix of labels with the context's n columns")
        nl = lab.shape[0]
        valid = lab.size > 0 and lab.min() >= 1 and lab.max() <= self.n            # otherwise the library names the label
        counts = [np.bincount(row, minlength=self.n + 1) for row in lab] if valid else []
        names = [np.flatnonzero(z).astype(np.int64) for z in counts]
        sizes = [z[z > 0].astype(np.int64) for z in counts]
        ktot = sum(len(z) for z in sizes)
        K = np.zeros(max(nl, 1), np.int64)
        med, medw = np.zeros(max(ktot, 1), np.int64), np.zeros(max(ktot, 1), np.int64)
        per = [np.zeros((max(nl, 1), self.n), np.int64) for _ in range(3)] if points else [None] * 3
        eD, ms = C.c_int32(), C.c_double()
        self._chk(self.L.rc_cluster_profiles(self.h, nl, lab.ctypes.data, K.ctypes.data, med.ctypes.data, medw.ctypes.data, ktot,
                                             *(None if x is None else x.ctypes.data for x in per), C.byref(eD), C.byref(ms)))
        off = np.concatenate([[0], np.cumsum([len(z) for z in sizes])]).astype(np.int64)
        return dict(K=K[:nl], labels=names, sizes=sizes, medoids=[med[off[i]:off[i + 1]] for i in range(nl)],
                    medoid_within=[medw[off[i]:off[i + 1]] for i in range(nl)],
                    within=None if per[0] is None else per[0][:nl], nearest=None if per[1] is None else per[1][:nl],
                    neighbour=None if per[2] is None else per[2][:nl], eD=int(eD.value), kernel_ms=float(ms.value))

    def syml2_plan_info(self) -> dict:
        """rc_bulk_plan_info: resident waves, fast units, rows per unit and the most units in one wave of k_bulk_syml2's plan"""
        v = [C.c_int32(0) for _ in range(4)]
        self._chk(self.L.rc_bulk_plan_info(self.h, *[C.byref(x) for x in v]))
        return dict(waves=v[0].value, fast_units=v[1].value, unit_rows=v[2].value, max_units_per_wave=v[3].value)

    def layout_info(self):
        """(layouts built so far, label runs in the internal point order)"""
        a, b = C.c_int32(), C.c_int32()
        self._chk(self.L.rc_layout_info(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def event_overhead_ms(self):
        out = C.c_double()
        self._chk(self.L.rc_event_overhead_ms(self.h, C.byref(out)))
        return out.value

    def kernel_timing(self, enable=-1):
        ms = C.c_double()
        cnt = C.c_int64()
        self._chk(self.L.rc_kernel_timing(self.h, int(enable), C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value


def _chain_buffers(n, numiters, burnin, thin, numMH):
    ns = max((numiters - burnin) // thin, 0) if thin > 0 else 0
    res = dict(clusts=np.zeros((ns, n), np.int64), K=np.zeros(ns, np.int64), r=np.zeros(ns), p=np.zeros(ns),
               loglik=np.zeros(ns), logposterior=np.zeros(ns), r_acceptances=np.zeros(numiters, np.uint8),
               splitmerge_acceptances=np.zeros(numiters * numMH, np.uint8),
               splitmerge_splits=np.zeros(numiters * numMH, np.uint8), r_all=np.zeros(numiters), p_all=np.zeros(numiters))
    out = RcChainOutputs()
    for k in res:
        setattr(out, k, res[k].ctypes.data if res[k].size else None)
    return ns, res, out


class Comm:
    """rc_comm: the RCCL communicator of the chains (one per GPU).  In one process: Comm(device_ids).  One process per
    GPU: rank 0 calls Comm.unique_id(), moves the bytes to the others, every rank calls Comm([device], rank, world, id)."""

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        _check(lib().rc_comm_unique_id(buf))
        return bytes(buf)

    def __init__(self, device_ids, rank_offset: int = 0, world_size: int | None = None, unique_id: bytes | None = None):
        self.L = lib()
        self.devices = [int(d) for d in device_ids]
        world = len(self.devices) if world_size is None else int(world_size)
        devs = (C.c_int32 * len(self.devices))(*self.devices)
        idb = (C.c_uint8 * 128)(*unique_id) if unique_id is not None else None
        h = C.c_void_p()
        _check(self.L.rc_comm_create(len(self.devices), devs, int(rank_offset), world, idb, C.byref(h)))
        self.h = h

    def allreduce_counts(self, ctxs, num_samples):
        """In-place merge of the contexts' co-clustering counts over all chains.  Returns (total_samples, elapsed_ms)."""
        hs = (C.c_void_p * len(ctxs))(*[c.h for c in ctxs])
        ns = (C.c_int64 * len(ctxs))(*[int(x) for x in num_samples])
        tot, ms = C.c_int64(0), C.c_double(0)
        _check(self.L.rc_comm_allreduce_counts(self.h, hs, ns, C.byref(tot), C.byref(ms)))
        return int(tot.value), float(ms.value)

    def close(self):
        if getattr(self, "h", None):
            self.L.rc_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def run_chains(device_ids, params: dict, init_clusts, numiters, burnin, thin, numGibbs, numMH, seed, r0, p0, proposalsd_r, *,
               D=None, logD=None, points=None, storage_bits: int = 64, kcap: int = 0, splitmerge="as_written",
               want_posterior: bool = True):
    """rc_run_chains: len(device_ids) chains in this process (one host thread + context per GPU, chain c seeded seed + c),
    merged over RCCL.  Returns (list of per-chain dicts as Context.run_chain, merged posterior co-clustering or None,
    total number of samples, all-reduce milliseconds)."""
    L = lib()
    devs = [int(d) for d in device_ids]
    nch = len(devs)
    inp = RcChainsInput()
    keep = []
    if D is not None:
        D = np.ascontiguousarray(D, dtype=np.float64); keep.append(D)
        n = int(D.shape[0]); inp.D = D.ctypes.data
        if logD is not None:
            logD = np.ascontiguousarray(logD, dtype=np.float64); keep.append(logD); inp.logD_or_null = logD.ctypes.data
    else:
        points = np.ascontiguousarray(points, dtype=np.float64); keep.append(points)
        n = int(points.shape[0]); inp.points = points.ctypes.data; inp.dim = int(points.shape[1])
    prm = _params_struct(params)
    init = np.ascontiguousarray(init_clusts, dtype=np.int64); keep.append(init)
    inp.n, inp.storage_bits, inp.kcap, inp.params, inp.init_clusts = n, int(storage_bits), int(kcap), C.pointer(prm), init.ctypes.data
    ns = 0
    ress, outs = [], (RcChainOutputs * nch)()
    for c in range(nch):
        ns, res, out = _chain_buffers(n, numiters, burnin, thin, numMH)
        ress.append(res); outs[c] = out
    o = RcChainOptions(numiters, burnin, thin, numGibbs, numMH, {"as_written": 0, "intended": 1}[splitmerge], 0,
                       int(seed), 0, float(r0), float(p0), float(proposalsd_r), None, None, ns)
    post = np.zeros((n, n)) if want_posterior else None
    tot, ms = C.c_int64(0), C.c_double(0)
    _check(L.rc_run_chains(nch, (C.c_int32 * nch)(*devs), C.byref(inp), C.byref(o), outs,
                           post.ctypes.data if post is not None else None, C.byref(tot), C.byref(ms)))
    for c, res in enumerate(ress):
        res["num_samples"], res["runtime_s"] = int(outs[c].num_samples), float(outs[c].runtime_s)
        res["r_final"], res["p_final"] = float(outs[c].r_final), float(outs[c].p_final)
        for k in ("r_acceptances", "splitmerge_acceptances", "splitmerge_splits"):
            res[k] = res[k].astype(bool)
    del keep
    return ress, post, int(tot.value), float(ms.value)


def measure_read_ceiling(device: int = 0, mib: int = 2048, reps: int = 5) -> float:
    """rc_measure_read_ceiling: the device's streaming-read rate in GB/s as measured now (buffer >> Infinity Cache)."""
    L = lib()
    out = C.c_double(0)
    _check(L.rc_measure_read_ceiling(int(device), int(mib), int(reps), C.byref(out)))
    return float(out.value)


def _label_matrix(x, what="samples"):
    """x as a C-contiguous int64 matrix of labels, one labelling per row"""
    x = np.ascontiguousarray(x, dtype=np.int64)
    if x.ndim != 2:
        raise ValueError(f"{what} must be an m×n matrix of labels")
    return x


def _psm_result(labels, runs, nruns, n, best, ms, **extra) -> dict:
    """The dict of the searches: labels (nruns×n), one array per field of the runs' record (RcPsmRun, or RcPearRun), best,
    kernel_ms and what extra names."""
    out = dict(labels=labels[:nruns, :n], best=int(best.value), kernel_ms=float(ms.value), **extra)
    for k, ty in type(runs)._type_._fields_:
        out[k] = np.array([getattr(r, k) for r in runs[:nruns]], dtype=np.float64 if ty is C.c_double else np.int64)
    out["converged"] = out["converged"].astype(bool)
    return out


def loss_matrix(samples, loss: int, device: int = 0, want_matrix: bool = True):
    """rc_loss_matrix: (lossmatrix or None, column sums, 0-based argmin, kernel ms) for an m×n int64 label matrix."""
    L = lib()
    S = _label_matrix(samples)
    m, n = S.shape
    M = np.zeros((m, m)) if want_matrix else None
    cs = np.zeros(m)
    am, ms = C.c_int64(), C.c_double()
    _check(L.rc_loss_matrix(device, S.reshape(-1), m, n, int(loss), None if M is None else M.ctypes.data_as(C.c_void_p),
                            cs.ctypes.data_as(C.c_void_p), C.byref(am), C.byref(ms)))
    return M, cs, int(am.value), float(ms.value)


def _search_runs(init, order, maxK, maxsweeps, call, n=None, record=RcPsmRun) -> dict:
    """What the searches share (record: the type of a run's record): init (nruns×n labels, 0 = unallocated) and order (nruns×n 1-based permutations) coerced and
    checked — n given: the samples' length, which init must have — the output buffers, and the dict of the results.
    call(n, *tail) makes the library call and checks its return code; tail is what every search entry point ends with: nruns,
    init, order, maxK, maxsweeps, labels_out, runs_out, best, kernel_ms.  What it returns (a dict or None) is added to the result."""
    init = np.ascontiguousarray(init, dtype=np.int64)
    order = np.ascontiguousarray(order, dtype=np.int32)
    if init.ndim != 2 or init.shape != order.shape or (n is not None and init.shape[1] != n):
        raise ValueError("init and order must be nruns×n arrays of the same shape" + (", n the samples' length" if n is not None else ""))
    nruns, n = init.shape
    labels = np.zeros((max(nruns, 1), max(n, 1)), np.int64)
    runs = (record * max(nruns, 1))()
    best, ms = C.c_int32(-1), C.c_double()
    extra = call(n, nruns, init.ctypes.data, order.ctypes.data, int(maxK), int(maxsweeps), labels.ctypes.data, runs, C.byref(best),
                 C.byref(ms))
    return _psm_result(labels, runs, nruns, n, best, ms, **(extra or {}))


def _counts_form(family, counts, numsamples, ctx, samples, device, n=None, what=None):
    """Which of the three forms of a consumer of the co-clustering counts a call takes — rc_<family>_samples (samples: an m×n
    label matrix; counts and numsamples are ignored), rc_<family>_ctx (ctx: that context's device counts) or rc_<family>
    (counts: n×n uint32) — as (the library's function, its leading arguments, the handle whose error buffer holds its
    errors, n, whether a counts_ms out-parameter ends its list).  n given: the length of `what`, which the source must match."""
    L = lib()
    if samples is not None:
        S = _label_matrix(samples)
        return getattr(L, f"rc_{family}_samples"), (int(device), S.ctypes.data_as(C.c_void_p), *S.shape), None, S.shape[1], True
    if ctx is not None:
        if n is not None and n != ctx.n:
            raise ValueError(f"{what} must have the context's n columns")
        return getattr(L, f"rc_{family}_ctx"), (ctx.h, int(numsamples)), ctx.h, ctx.n, False
    cnt = np.ascontiguousarray(counts, dtype=np.uint32)
    if n is None and (cnt.ndim != 2 or cnt.shape[0] != cnt.shape[1]):
        raise ValueError("counts must be an n×n matrix")
    if n is not None and cnt.shape != (n, n):
        raise ValueError(f"counts must be an n×n matrix matching {what}")
    return getattr(L, f"rc_{family}"), (int(device), cnt.ctypes.data_as(C.c_void_p), int(numsamples), cnt.shape[0]), None, cnt.shape[0], False


def _psm_search(counts, numsamples, ctx, samples, loss, init, order, maxK, maxsweeps, device) -> dict:
    """psm_search and psm_search_samples (samples: the label matrix) behind their parameter lists; loss None: the PEAR
    search's three entry points, which have the same lists without the loss"""
    cms = C.c_double()
    family, crit, record = ("pear_search", [], RcPearRun) if loss is None else ("psm_search", [int(loss)], RcPsmRun)

    def call(n, *tail):
        fn, head, handle, _, timed = _counts_form(family, counts, numsamples, ctx, samples, device, n, "init")
        _check(fn(*head, *crit, *tail, *([C.byref(cms)] if timed else [])), handle)
        return dict(counts_ms=float(cms.value)) if timed else None
    return _search_runs(init, order, maxK, maxsweeps, call, n=None if samples is None else samples.shape[1], record=record)


def psm_search(counts, numsamples: int, loss: int, init, order, maxK: int = 0, maxsweeps: int = 100, device: int = 0, ctx=None):
    """rc_psm_search (counts: n×n uint32) or, with ctx, rc_psm_search_ctx on that context's device counts (counts is ignored).
    init: nruns×n labels (0 = unallocated), order: nruns×n 1-based permutations.  Returns a dict: labels (nruns×n, sortlabels'd),
    the per-run arrays loss, loss_num, sweeps, converged, moves, K, and best, kernel_ms."""
    return _psm_search(counts, numsamples, ctx, None, loss, init, order, maxK, maxsweeps, device)


def samples_counts(samples, device: int = 0):
    """rc_samples_counts: (n×n uint32 co-clustering counts, kernel ms) of an m×n int64 label matrix (labels 1..n), built on
    the device: counts[i, j] = number of samples in which i and j share a label."""
    L = lib()
    S = _label_matrix(samples)
    m, n = S.shape
    out = np.empty((max(n, 1), max(n, 1)), np.uint32)
    ms = C.c_double()
    _check(L.rc_samples_counts(int(device), S.ctypes.data, m, n, out.ctypes.data, C.byref(ms)))
    return out, float(ms.value)


def psm_search_samples(samples, loss: int, init, order, maxK: int = 0, maxsweeps: int = 100, device: int = 0):
    """rc_psm_search_samples: psm_search on the counts of an m×n int64 label matrix (labels 1..n), which are built on the
    device and stay there.  Returns psm_search's dict and counts_ms, the device time of the counts kernel."""
    return _psm_search(None, None, None, _label_matrix(samples), loss, init, order, maxK, maxsweeps, device)


def pear_search(counts, numsamples: int, init, order, maxK: int = 0, maxsweeps: int = 100, device: int = 0, ctx=None):
    """rc_pear_search (counts: n×n uint32) or, with ctx, rc_pear_search_ctx on that context's device counts.  Arguments as
    psm_search without the loss.  Returns a dict: labels (nruns×n, sortlabels'd), the per-run arrays pear, num, den, sweeps,
    converged, moves, K, and best (the first run of maximal num/den), kernel_ms."""
    return _psm_search(counts, numsamples, ctx, None, None, init, order, maxK, maxsweeps, device)


def pear_search_samples(samples, init, order, maxK: int = 0, maxsweeps: int = 100, device: int = 0):
    """rc_pear_search_samples: pear_search on the counts of an m×n int64 label matrix (labels 1..n), which are built on the
    device and stay there.  Returns pear_search's dict and counts_ms."""
    return _psm_search(None, None, None, _label_matrix(samples), None, init, order, maxK, maxsweeps, device)


def vi_gtable(n: int) -> np.ndarray:
    """rc_vi_gtable: Gq[x] = llrint((phi(x+1) − phi(x))·2^32), x = 0..n−1, phi(x) = x·log x — the table rc_vi_search decides on."""
    L = lib()
    out = np.zeros(max(int(n), 1), np.int64)
    _check(L.rc_vi_gtable(int(n), out.ctypes.data))
    return out


def _exact_search(entry, samples, init, order, maxK, maxsweeps, device) -> dict:
    """rc_vi_search and rc_id_search have one parameter list"""
    S = _label_matrix(samples)
    return _search_runs(init, order, maxK, maxsweeps,
                        lambda n, *tail: _check(entry(int(device), S.ctypes.data, S.shape[0], n, *tail)), n=S.shape[1])


def vi_search(samples, init, order, maxK: int = 0, maxsweeps: int = 100, device: int = 0):
    """rc_vi_search: the exact expected-VI search.  samples: m×n labels in 1..n; init: nruns×n labels (0 = unallocated), order:
    nruns×n 1-based permutations.  Returns psm_search's dict: labels (nruns×n, sortlabels'd), the per-run arrays loss (the
    expected VI), loss_num (the integer Q), sweeps, converged, moves, K, and best, kernel_ms."""
    return _exact_search(lib().rc_vi_search, samples, init, order, maxK, maxsweeps, device)


def id_search(samples, init, order, maxK: int = 0, maxsweeps: int = 100, device: int = 0):
    """rc_id_search: the exact expected-ID search.  Arguments and the returned dict as vi_search; loss is the expected
    information distance (nats), loss_num the integer Q_ID."""
    return _exact_search(lib().rc_id_search, samples, init, order, maxK, maxsweeps, device)


def vi_search_groups(samples, group, init, order, run_group, maxK: int = 0, maxsweeps: int = 100, device: int = 0):
    """rc_vi_search_groups: many exact expected-VI searches over disjoint groups of the samples in one launch.  samples: m×n
    labels in 1..n; group: m group ids in 0..ngroups−1 (−1: in no group), ngroups = the largest id + 1 (at least 1); init, order:
    as vi_search; run_group: the group each of the nruns runs searches.  Run r is vi_search's run on samples[group ==
    run_group[r]].  Returns vi_search's dict, except that best is an int array with one entry per group: the first run of minimal
    loss_num among the group's runs, −1 where it has none."""
    S = _label_matrix(samples)
    grp = np.ascontiguousarray(group, dtype=np.int32)
    rg = np.ascontiguousarray(run_group, dtype=np.int32)
    if grp.ndim != 1 or grp.shape[0] != S.shape[0]:
        raise ValueError("group must hold one group id per sample")
    init = np.ascontiguousarray(init, dtype=np.int64)
    order = np.ascontiguousarray(order, dtype=np.int32)
    if init.ndim != 2 or init.shape != order.shape or init.shape[1] != S.shape[1]:
        raise ValueError("init and order must be nruns×n arrays of the same shape, n the samples' length")
    if rg.ndim != 1 or rg.shape[0] != init.shape[0]:
        raise ValueError("run_group must hold one group id per run")
    (m, n), nruns = S.shape, init.shape[0]
    ngroups = max(int(grp.max()) + 1 if m else 1, 1)
    labels = np.zeros((max(nruns, 1), max(n, 1)), np.int64)
    runs = (RcPsmRun * max(nruns, 1))()
    best, ms = np.full(ngroups, -1, np.int32), C.c_double()
    _check(lib().rc_vi_search_groups(int(device), S.ctypes.data, m, n, grp.ctypes.data, ngroups, nruns, rg.ctypes.data, init.ctypes.data,
                                     order.ctypes.data, int(maxK), int(maxsweeps), labels.ctypes.data, runs, best.ctypes.data, C.byref(ms)))
    out = _psm_result(labels, runs, nruns, n, C.c_int32(-1), ms)
    out["best"] = best.astype(np.int64)
    return out


# rc_hclust_merge_t
HCLUST_MERGE = np.dtype([("a", np.int32), ("b", np.int32), ("size", np.int32), ("m_ab", np.uint32), ("s_ab", np.int64)], align=True)


def hclust(counts, numsamples, linkage: int, maxcut: int = 0, device: int = 0, ctx=None, samples=None):
    """rc_hclust (counts: n×n uint32), rc_hclust_samples (samples: m×n int64 labels; counts and numsamples are ignored) or,
    with ctx, rc_hclust_ctx on that context's device counts.  Returns a dict: merges (n − 1 records of HCLUST_MERGE),
    binder_num (n int64; index t = after t merges), vilb (maxcut f64: the VI-bound loss of the cuts K = 1..maxcut), kernel_ms,
    and counts_ms for the samples form."""
    fn, head, handle, n, timed = _counts_form("hclust", counts, numsamples, ctx, samples, device)
    merges = np.zeros(max(n - 1, 1), HCLUST_MERGE)
    bnum = np.zeros(max(n, 1), np.int64)
    vilb = np.zeros(max(int(maxcut), 1))
    ms, cms = C.c_double(), C.c_double()
    _check(fn(*head, int(linkage), merges.ctypes.data, bnum.ctypes.data, int(maxcut), vilb.ctypes.data, C.byref(ms),
              *([C.byref(cms)] if timed else [])), handle)
    out = dict(counts_ms=float(cms.value)) if timed else {}
    out.update(merges=merges[:max(n - 1, 0)], binder_num=bnum[:n], vilb=vilb[:int(maxcut)], kernel_ms=float(ms.value))
    return out


def hclust_cut(merges, n: int, K: int) -> np.ndarray:
    """rc_hclust_cut (host only): the labelling with K clusters, labels 1..K in sortlabels order."""
    L = lib()
    mg = np.ascontiguousarray(merges, dtype=HCLUST_MERGE)
    labels = np.zeros(max(int(n), 1), np.int64)
    _check(L.rc_hclust_cut(mg.ctypes.data, int(n), int(K), labels.ctypes.data))
    return labels[:int(n)]


def psm_expected_loss(labels, counts, numsamples: int, loss: int, device: int = 0, ctx=None):
    """rc_psm_expected_loss (counts: n×n uint32) or, with ctx, rc_psm_expected_loss_ctx: (loss f64[L], num int64[L], kernel ms)
    of the L×n labellings `labels` (1..n)."""
    lab = np.ascontiguousarray(labels, dtype=np.int64)
    if lab.ndim != 2:
        raise ValueError("labels must be an L×n matrix")
    nl, n = lab.shape
    loss_out, num_out, ms = np.zeros(max(nl, 1)), np.zeros(max(nl, 1), np.int64), C.c_double()
    fn, head, handle, _, _ = _counts_form("psm_expected_loss", counts, numsamples, ctx, None, device, n, "labels")
    _check(fn(*head, int(loss), nl, lab.ctypes.data, loss_out.ctypes.data, num_out.ctypes.data, C.byref(ms)), handle)
    return loss_out[:nl], num_out[:nl], float(ms.value)


def predict(Dnew, samples, r, p, params: dict, seed: int = 0, sample_offset: int = 0, point_offset: int = 0, logDnew=None,
            want_map: bool = True, Kmax: int = 0, want_scores: bool = False, want_sums: bool = False, device: int = 0) -> dict:
    """rc_predict: labels (m×q, 0 = a cluster of its own), map (or None), eD / eL (q), kernel_ms and, when asked for with Kmax,
    scores (m×q×(Kmax+1)) and sums (m×q×Kmax×2) for the q×n distances Dnew of new points to the training points and an m×n
    label matrix with one r and p per sample."""
    L = lib()
    D = np.ascontiguousarray(Dnew, dtype=np.float64)
    S = np.ascontiguousarray(samples, dtype=np.int64)
    r = np.ascontiguousarray(r, dtype=np.float64)
    p = np.ascontiguousarray(p, dtype=np.float64)
    if D.ndim != 2 or S.ndim != 2 or D.shape[1] != S.shape[1]:
        raise ValueError("Dnew must be q×n and samples m×n")
    q, n = D.shape
    m = S.shape[0]
    if r.shape != (m,) or p.shape != (m,):
        raise ValueError("r and p must hold one value per sample")
    lp = None
    if logDnew is not None:
        logDnew = np.ascontiguousarray(logDnew, dtype=np.float64)
        if logDnew.shape != D.shape:
            raise ValueError("logDnew must have Dnew's shape")
        lp = logDnew.ctypes.data
    prm = _params_struct(params)
    labels = np.zeros((max(m, 1), max(q, 1)), np.int64)
    mp = np.zeros_like(labels) if want_map else None
    sc = np.zeros((max(m, 1), max(q, 1), int(Kmax) + 1)) if want_scores else None
    sm = np.zeros((max(m, 1), max(q, 1), max(int(Kmax), 1), 2), np.int64) if want_sums else None
    eD, eL = np.zeros(max(q, 1), np.int32), np.zeros(max(q, 1), np.int32)
    ms = C.c_double()
    M64 = 0xFFFFFFFFFFFFFFFF
    rc = L.rc_predict(int(device), n, q, D.ctypes.data, lp, m, S.ctypes.data, r.ctypes.data, p.ctypes.data, C.byref(prm),
                      int(seed) & M64, int(sample_offset) & M64, int(point_offset) & M64, labels.ctypes.data,
                      None if mp is None else mp.ctypes.data, int(Kmax), None if sc is None else sc.ctypes.data,
                      None if sm is None else sm.ctypes.data, eD.ctypes.data, eL.ctypes.data, C.byref(ms))
    _check(rc)
    out = dict(labels=labels[:m, :q], map=None if mp is None else mp[:m, :q], eD=eD[:q], eL=eL[:q], kernel_ms=float(ms.value))
    if want_scores:
        out["scores"] = sc[:m, :q]
    if want_sums:
        out["sums"] = sm[:m, :q, :int(Kmax)]
    return out


def predict_points(points, new_points, samples, r, p, params: dict, seed: int = 0, sample_offset: int = 0, point_offset: int = 0,
                   want_labels: bool = True, want_map: bool = True, maps=None, pivot_labels=None, want_counts: bool = False,
                   want_mapcounts: bool = False, Kmax: int = 0, want_scores: bool = False, want_sums: bool = False,
                   want_dist: bool = False, want_log: bool = False, device: int = 0, *, metric=None) -> dict:
    """rc_predict_points: as predict for q×dim new points and the n×dim training points, the distances and their logarithms
    taken on the device: labels and map (m×q, or None), eD / eL (q), kernel_ms and, when asked for, scores and sums (with Kmax),
    dist and log (q×n), and — with maps (m×W, rc_relabel's) and pivot_labels (K_p, ascending) — counts and mapcounts
    (q×(K_p+1) uint32).  metric: None for rc_predict_points itself, or a name of METRICS (rc_predict_points_metric)."""
    X = np.ascontiguousarray(points, dtype=np.float64)
    Y = np.ascontiguousarray(new_points, dtype=np.float64)
    if metric is not None:
        check_metric(metric, X.shape[1] if X.ndim == 2 else None)
    L = lib()
    S = np.ascontiguousarray(samples, dtype=np.int64)
    r = np.ascontiguousarray(r, dtype=np.float64)
    p = np.ascontiguousarray(p, dtype=np.float64)
    if X.ndim != 2 or Y.ndim != 2 or S.ndim != 2 or X.shape[0] != S.shape[1] or Y.shape[1] != X.shape[1]:
        raise ValueError("points must be n×dim, new_points q×dim and samples m×n")
    (n, dim), q, m = X.shape, Y.shape[0], S.shape[0]
    if r.shape != (m,) or p.shape != (m,):
        raise ValueError("r and p must hold one value per sample")
    mp_ = pv = None
    W = Kp = 0
    if maps is not None:
        mp_ = np.ascontiguousarray(maps, dtype=np.int64)
        if mp_.ndim != 2 or mp_.shape[0] != m:
            raise ValueError("maps must be m×W")
        W = mp_.shape[1]
    if pivot_labels is not None:
        pv = np.ascontiguousarray(pivot_labels, dtype=np.int64).reshape(-1)
        Kp = len(pv)
    prm = _params_struct(params)
    labels = np.zeros((max(m, 1), max(q, 1)), np.int64) if want_labels else None
    mp = np.zeros((max(m, 1), max(q, 1)), np.int64) if want_map else None
    cnt = np.zeros((max(q, 1), Kp + 1), np.uint32) if want_counts else None
    mcnt = np.zeros((max(q, 1), Kp + 1), np.uint32) if want_mapcounts else None
    sc = np.zeros((max(m, 1), max(q, 1), int(Kmax) + 1)) if want_scores else None
    sm = np.zeros((max(m, 1), max(q, 1), max(int(Kmax), 1), 2), np.int64) if want_sums else None
    dist = np.zeros((max(q, 1), max(n, 1))) if want_dist else None
    lg = np.zeros((max(q, 1), max(n, 1))) if want_log else None
    eD, eL = np.zeros(max(q, 1), np.int32), np.zeros(max(q, 1), np.int32)
    ms = C.c_double()
    M64 = 0xFFFFFFFFFFFFFFFF
    ptr = lambda a: None if a is None else a.ctypes.data
    rest = (int(device), n, dim, X.ctypes.data, q, Y.ctypes.data, m, S.ctypes.data, r.ctypes.data, p.ctypes.data,
            C.byref(prm), int(seed) & M64, int(sample_offset) & M64, int(point_offset) & M64, ptr(labels), ptr(mp),
            ptr(mp_), W, ptr(pv), Kp, ptr(cnt), ptr(mcnt), int(Kmax), ptr(sc), ptr(sm), ptr(dist), ptr(lg),
            eD.ctypes.data, eL.ctypes.data, C.byref(ms))
    rc = L.rc_predict_points(*rest) if metric is None else L.rc_predict_points_metric(METRICS[metric], *rest)
    _check(rc)
    cut = lambda a: None if a is None else a[:m, :q]
    out = dict(labels=cut(labels), map=cut(mp), eD=eD[:q], eL=eL[:q], kernel_ms=float(ms.value),
               counts=None if cnt is None else cnt[:q], mapcounts=None if mcnt is None else mcnt[:q])
    if want_scores:
        out["scores"] = sc[:m, :q]
    if want_sums:
        out["sums"] = sm[:m, :q, :int(Kmax)]
    if want_dist:
        out["dist"] = dist[:q, :n]
    if want_log:
        out["log"] = lg[:q, :n]
    return out


def pairwise(points, new_points=None, metric: str = "euclidean", device: int = 0, want_ms: bool = False):
    """rc_pairwise: the n×n matrix of the n×dim points (new_points None) or the q×n matrix of q×dim new points against them, as
    doubles in the metric's stated arithmetic; with want_ms also the kernels' time in ms."""
    X = np.ascontiguousarray(points, dtype=np.float64)
    Y = None if new_points is None else np.ascontiguousarray(new_points, dtype=np.float64)
    if X.ndim != 2 or (Y is not None and (Y.ndim != 2 or Y.shape[1] != X.shape[1])):
        raise ValueError("points must be n×dim and new_points q×dim")
    check_metric(metric, X.shape[1])
    L = lib()
    n, dim = X.shape
    q = 0 if Y is None else Y.shape[0]
    out = np.zeros((n if Y is None else max(q, 1), max(n, 1)))
    ms = C.c_double()
    _check(L.rc_pairwise(int(device), METRICS[metric], n, dim, X.ctypes.data, q, None if Y is None else Y.ctypes.data, out.ctypes.data,
                         C.byref(ms)))
    out = out if Y is None else out[:q, :n]
    return (out, float(ms.value)) if want_ms else out


def predict_joint(Dnew, Dnn, samples, r, p, params: dict, sweeps: int = 2, seed: int = 0, sample_offset: int = 0, logDnew=None,
                  logDnn=None, want_first: bool = True, want_moves: bool = True, want_sums: bool = False, device: int = 0) -> dict:
    """rc_predict_joint: labels (m×q, names in 1..n+q), first (the labels after pass 0, or None), K (m), moves (m×(sweeps+1), or
    None), sums (m×q×2, when asked for), eD / eL (q) and kernel_ms for the q×n distances Dnew of new points to the training
    points, the q×q distances Dnn among the new points and an m×n label matrix with one r and p per sample."""
    L = lib()
    D = np.ascontiguousarray(Dnew, dtype=np.float64)
    Dn = np.ascontiguousarray(Dnn, dtype=np.float64)
    S = np.ascontiguousarray(samples, dtype=np.int64)
    r = np.ascontiguousarray(r, dtype=np.float64)
    p = np.ascontiguousarray(p, dtype=np.float64)
    if D.ndim != 2 or S.ndim != 2 or D.shape[1] != S.shape[1]:
        raise ValueError("Dnew must be q×n and samples m×n")
    q, n = D.shape
    m = S.shape[0]
    if Dn.shape != (q, q):
        raise ValueError("Dnn must be q×q")
    if r.shape != (m,) or p.shape != (m,):
        raise ValueError("r and p must hold one value per sample")
    if (logDnew is None) != (logDnn is None):
        raise ValueError("give logDnew and logDnn together or neither")
    lp = ln = None
    if logDnew is not None:
        logDnew = np.ascontiguousarray(logDnew, dtype=np.float64)
        logDnn = np.ascontiguousarray(logDnn, dtype=np.float64)
        if logDnew.shape != D.shape or logDnn.shape != Dn.shape:
            raise ValueError("logDnew and logDnn must have the shapes of Dnew and Dnn")
        lp, ln = logDnew.ctypes.data, logDnn.ctypes.data
    prm = _params_struct(params)
    nm = max(int(sweeps), 0) + 1
    labels = np.zeros((max(m, 1), max(q, 1)), np.int64)
    first = np.zeros_like(labels) if want_first else None
    K = np.zeros(max(m, 1), np.int64)
    moves = np.zeros((max(m, 1), nm), np.int64) if want_moves else None
    sm = np.zeros((max(m, 1), max(q, 1), 2), np.int64) if want_sums else None
    eD, eL = np.zeros(max(q, 1), np.int32), np.zeros(max(q, 1), np.int32)
    ms = C.c_double()
    M64 = 0xFFFFFFFFFFFFFFFF
    rc = L.rc_predict_joint(int(device), n, q, D.ctypes.data, Dn.ctypes.data, lp, ln, m, S.ctypes.data, r.ctypes.data, p.ctypes.data,
                            C.byref(prm), int(sweeps), int(seed) & M64, int(sample_offset) & M64, labels.ctypes.data,
                            None if first is None else first.ctypes.data, K.ctypes.data, None if moves is None else moves.ctypes.data,
                            None if sm is None else sm.ctypes.data, eD.ctypes.data, eL.ctypes.data, C.byref(ms))
    _check(rc)
    out = dict(labels=labels[:m, :q], first=None if first is None else first[:m, :q], K=K[:m], moves=None if moves is None else moves[:m],
               eD=eD[:q], eL=eL[:q], kernel_ms=float(ms.value))
    if want_sums:
        out["sums"] = sm[:m, :q]
    return out


def partition_distances(labels, samples, want_sq: bool = True, want_phi: bool = True, device: int = 0) -> dict:
    """rc_partition_distances for L×n labellings and m×n samples (int64 labels in 1..n): a dict with sq and phi (L×m int64, or
    None when not asked for), lab_marg (L×3) and smp_marg (m×3) — Σ n_k², Σ Phiq(n_k), K of every row — and kernel_ms."""
    L = lib()
    lab = np.ascontiguousarray(labels, dtype=np.int64)
    S = np.ascontiguousarray(samples, dtype=np.int64)
    if lab.ndim != 2 or S.ndim != 2 or lab.shape[1] != S.shape[1]:
        raise ValueError("labels must be L×n and samples m×n")
    (nl, n), m = lab.shape, S.shape[0]
    sq = np.zeros((max(nl, 1), max(m, 1)), np.int64) if want_sq else None
    phi = np.zeros((max(nl, 1), max(m, 1)), np.int64) if want_phi else None
    lm, sm = np.zeros((max(nl, 1), 3), np.int64), np.zeros((max(m, 1), 3), np.int64)
    ms = C.c_double()
    rc = L.rc_partition_distances(int(device), S.ctypes.data, m, n, nl, lab.ctypes.data, None if sq is None else sq.ctypes.data,
                                  None if phi is None else phi.ctypes.data, lm.ctypes.data, sm.ctypes.data, C.byref(ms))
    _check(rc)
    return dict(sq=None if sq is None else sq[:nl, :m], phi=None if phi is None else phi[:nl, :m], lab_marg=lm[:nl], smp_marg=sm[:m],
                kernel_ms=float(ms.value))


def relabel(samples, pivot, want_labels: bool = True, want_maps: bool = True, device: int = 0) -> dict:
    """rc_relabel for m×n samples and a pivot of n labels (int64 in 1..n): a dict with labels (m×n int64, or None), maps (m × the
    largest K_s, or None), overlap (m), counts (n×(K_p+1) uint32), pivot_labels (the K_p names, ascending) and kernel_ms."""
    L = lib()
    S = np.ascontiguousarray(samples, dtype=np.int64)
    c = np.ascontiguousarray(pivot, dtype=np.int64)
    if S.ndim != 2 or c.ndim != 1 or S.shape[1] != c.shape[0]:
        raise ValueError("samples must be m×n and the pivot n labels")
    m, n = S.shape
    names = np.unique(c).astype(np.int64)
    Kp = len(names)
    valid = S.size > 0 and S.min() >= 1 and S.max() <= n            # otherwise the library names the label
    W = max(np.count_nonzero(np.bincount(row)) for row in S) if valid else 1       # the largest K_s, without a sort
    labels = np.zeros((max(m, 1), max(n, 1)), np.int64) if want_labels else None
    maps = np.zeros((max(m, 1), max(W, 1)), np.int64) if want_maps else None
    overlap = np.zeros(max(m, 1), np.int64)
    counts = np.zeros((max(n, 1), Kp + 1), np.uint32)
    ms = C.c_double()
    rc = L.rc_relabel(int(device), S.ctypes.data, m, n, c.ctypes.data, Kp, None if labels is None else labels.ctypes.data,
                      None if maps is None else maps.ctypes.data, W, overlap.ctypes.data, counts.ctypes.data, C.byref(ms))
    _check(rc)
    return dict(labels=labels, maps=maps, overlap=overlap, counts=counts, pivot_labels=names, kernel_ms=float(ms.value))


def loglik_from_blocks(blocks, sizes, n: int, eD: int, eL: int, params: dict) -> float:
    """rc_loglik_from_blocks (host only): the log-likelihood of one labelling from its upper-triangle block sums (K(K+1)/2 × 4
    int64 as Context.score returns them), its cluster sizes in ascending label order and the context's exponents, under any
    hyperparameters."""
    L = lib()
    sz = np.ascontiguousarray(sizes, dtype=np.int64).reshape(-1)
    B = np.ascontiguousarray(blocks, dtype=np.int64)
    K = len(sz)
    if B.size != K * (K + 1) // 2 * 4:
        raise ValueError("blocks must hold K(K+1)/2 × 4 integers for the K sizes")
    prm = _params_struct(params)
    out = C.c_double()
    _check(L.rc_loglik_from_blocks(int(n), K, sz.ctypes.data if K else None, B.ctypes.data if B.size else None, int(eD), int(eL),
                                   C.byref(prm), C.byref(out)))
    return float(out.value)


def sample_k(n: int, r, p, seed: int = 0, device: int = 0):
    """rc_sample_k: (K of every sample as int64 in 1..n, kernel ms) for the caller's draws r[i], p[i] — the device part of
    sampleK (prior.py)."""
    L = lib()
    r = np.ascontiguousarray(r, dtype=np.float64)
    p = np.ascontiguousarray(p, dtype=np.float64)
    if r.ndim != 1 or r.shape != p.shape:
        raise ValueError("r and p must be vectors of the same length")
    K = np.zeros(len(r), np.int64)
    ms = C.c_double()
    _check(L.rc_sample_k(int(device), int(n), len(r), r, p, int(seed) & 0xFFFFFFFFFFFFFFFF, K, C.byref(ms)))
    return K, float(ms.value)


def oracle_coclustering(points, K: int, radius: float, sigma: float, weights, iters_per_chunk: int = 0, device: int = 0):
    """rc_oracle_coclustering: (n×n oracle co-clustering matrix, kernel ms) for n×dim points and numiters×K weights —
    the device part of datagen.oracle_coclustering, which checks the arguments."""
    L = lib()
    X = np.ascontiguousarray(points, dtype=np.float64)
    W = np.ascontiguousarray(weights, dtype=np.float64)
    n, dim = X.shape
    out = np.empty((n, n))
    ms = C.c_double()
    rc = L.rc_oracle_coclustering(int(device), n, dim, X.reshape(-1), int(K), float(radius), float(sigma), W.shape[0],
                                  W.reshape(-1), int(iters_per_chunk), out.reshape(-1), C.byref(ms))
    _check(rc)
    return out, float(ms.value)


def pair_measures(a, b, device: int = 0) -> dict:
    """rc_pair_measures as a dict."""
    L = lib()
    a = np.ascontiguousarray(a, dtype=np.int64)
    b = np.ascontiguousarray(b, dtype=np.int64)
    out = RcPairMeasures()
    _check(L.rc_pair_measures(device, a, b, len(a), C.byref(out)))
    return {k: getattr(out, k) for k, _ in RcPairMeasures._fields_}
