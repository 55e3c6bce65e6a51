"""ctypes binding of the C ABI declared in include/rae.h (librae_hip.so).

The product path has no CPU fallback: if the HIP library is missing or a call fails, an
exception is raised.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "librae_hip.so"
LIB_PATH = os.path.join(_HERE, LIB_NAME)
CSRC = os.path.join(os.path.dirname(_HERE), "csrc")
HEADER = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "rae.h")
# hipcc flags of the in-tree build (__graft_entry__.build); part of the build id
BUILD_FLAGS = ("-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-shared", "-Wall",
               "-Wno-unused-parameter", "-Wno-unused-variable")


def source_files():
    """The sources librae_hip.so is built from: csrc/*.hip, csrc/*.hpp and include/rae.h."""
    if not os.path.isdir(CSRC):
        return []
    return [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC))
            if f.endswith((".hip", ".hpp"))] + [HEADER]


def source_build_id():
    """sha256 (16 hex digits) over the build flags and the sources' names and bytes; None
    when the sources are not next to the package.  build() compiles it into the library
    (rae_build_id()) and load() refuses a library whose id differs."""
    files = source_files()
    if not files or not all(os.path.exists(f) for f in files):
        return None
    h = hashlib.sha256(" ".join(BUILD_FLAGS).encode())
    for f in files:
        h.update(os.path.basename(f).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    return h.hexdigest()[:16]


def library_build_id(path=LIB_PATH):
    """The build id compiled into a built library, read from the file's bytes (a marker
    string rae.hip embeds) rather than by dlopen: a library already loaded in this process
    would shadow a rebuilt file of the same path.  None if absent."""
    try:
        with open(path, "rb") as fh:
            blob = fh.read()
    except OSError:
        return None
    i = blob.find(b"RAE_BUILD_ID:")
    if i < 0:
        return None
    j = blob.find(b"\0", i)
    return blob[i + len(b"RAE_BUILD_ID:"):j].decode(errors="replace")

RAE_OK = 0
RAE_DEC = {"sp": 0, "rescal": 1, "rescal+sp": 2}
RAE_OPT = {"adagrad": 0, "sgd": 1}
RAE_NEG_PER_CALL = 0
RAE_NEG_PER_EPOCH = 1

# Every symbol include/rae.h declares (checked by tests/test_abi.py against the header).
EXPORTS = (
    "rae_plan_create", "rae_plan_destroy", "rae_last_error", "rae_version", "rae_build_id",
    "rae_exchange_record_floats", "rae_exchange_floats", "rae_set_negatives",
    "rae_set_cursor", "rae_advance_cursor", "rae_cursor_moves", "rae_step_forward",
    "rae_step_update", "rae_step_forward_at", "rae_step_update_at",
    "rae_train_step", "rae_check", "rae_check_on", "rae_label", "rae_build_index", "rae_index_window",
    "rae_index_dims", "rae_index_read",
    "rae_neg_sample", "rae_neg_sample_philox",
    "rae_time_next", "rae_event_create", "rae_event_destroy", "rae_event_elapsed_ms",
    "rae_stream_copy", "rae_mfma_probe", "rae_plan_forms",
    "rae_dp_block_floats", "rae_set_dp_buffers", "rae_dp_list_max", "rae_dp_pack",
    "rae_dp_unpack", "rae_dp_pack_at", "rae_dp_unpack_at",
    "rae_ipc_export", "rae_ipc_open", "rae_ipc_close", "rae_p2p_signals", "rae_set_peer",
    "rae_set_p2p_timeout", "rae_p2p_prologue",
    "rae_eval_workspace_bytes", "rae_eval_cost",
    "rae_rank_queries", "rae_eval_rank", "rae_rank_workspace_bytes",
    "rae_topk_queries", "rae_eval_topk", "rae_topk_workspace_bytes",
    "rae_relation_scores", "rae_eval_relations", "rae_relscore_workspace_bytes",
    "rae_cluster_count", "rae_b3_metrics",
    "rae_row_keys", "rae_cluster_key_count", "rae_cluster_topk",
    "rae_feature_support", "rae_feature_topk", "rae_feature_topk_workspace_bytes",
    "rae_label_stats", "rae_cluster_exemplars", "rae_cluster_exemplars_workspace_bytes",
)
RAE_IPC_HANDLE_BYTES = 64
# rae_index_dims' values in order, and rae_index_read's regions (include/rae.h RAE_IDXR_*)
INDEX_DIMS = ("L", "l", "s", "G", "rank", "part", "RA", "RW", "HA", "HW", "index_window",
              "posbits", "TC", "NVC", "hch", "HF", "dcap", "dstride", "dnx", "priv", "privnf",
              "LA", "LW")
INDEX_REGIONS = {name: code for code, name in enumerate(
    ("srecA", "srecW", "segA", "segW", "countA", "countW", "pclsA", "pclsW", "thdr", "task",
     "vtask", "hfin", "desc", "pmask", "dpl", "dpc", "dpmax"))}
RAE_IDX_HMAX = 1024               # partition table entries per batch slot and table
# rae_cluster_count forms (include/rae.h RAE_CCOUNT_*)
RAE_CCOUNT_AUTO = 0
RAE_CCOUNT_LDS = 1
RAE_CCOUNT_GLOBAL = 2
RAE_CCOUNT_ACCUMULATE = 0x100
RAE_CCOUNT_LDS_CELLS = 16384      # the LDS form's budget: relations * (n_gold + 1) counters
# rae_cluster_key_count / rae_cluster_topk limits (include/rae.h) and the kernels' grid constants
# (csrc/rae_profile.hpp RAE_CK_*)
RAE_KEYCOUNT_MAX_KEYS = 1 << 22
RAE_KEYCOUNT_MAX_CELLS = 1 << 27
RAE_TOPK_MAX = 32
RAE_CK_BT, RAE_CK_QPT, RAE_CK_GRID = 256, 4, 2048
CCOUNT_FORMS = {"auto": RAE_CCOUNT_AUTO, "lds": RAE_CCOUNT_LDS, "global": RAE_CCOUNT_GLOBAL}


class RaeConfig(C.Structure):
    _fields_ = [
        ("decoder", C.c_int32), ("optimizer", C.c_int32),
        ("n_examples", C.c_int64), ("n_features", C.c_int64), ("n_entities", C.c_int64),
        ("relations", C.c_int32), ("embed", C.c_int32), ("neg_samples", C.c_int32),
        ("batch_size", C.c_int32), ("world_size", C.c_int32), ("rank", C.c_int32),
        ("learning_rate", C.c_float), ("alpha", C.c_float), ("lambda1", C.c_float),
        ("lambda2", C.c_float), ("ext_reg", C.c_int32), ("max_batch_nnz", C.c_int32),
        ("max_row_nnz", C.c_int32), ("neg_mode", C.c_int32), ("neg_stride", C.c_int64),
        ("index_window", C.c_int64), ("mfma_bf16", C.c_int32),
        ("sp_forward", C.c_int32), ("bil_dp", C.c_int32), ("bil_prep", C.c_int32),
        ("dp_update", C.c_int32), ("priv_rows", C.c_int32), ("dp_dense", C.c_int32),
        ("heavy_chunk", C.c_int32), ("dp_xchg", C.c_int32),
    ]


# kernel forms (include/rae.h RAE_SPFWD_* / RAE_BILDP_* / RAE_BILPREP_* / RAE_DPUPD_*)
KERNEL_FORMS = {
    "sp_forward": {"auto": 0, "fused": 1, "split": 2},
    "bil_dp": {"auto": 0, "strided": 1, "staged": 2, "mtile": 3},
    "bil_prep": {"auto": 0, "kernel": 1},
    "dp_update": {"replicated": 0, "partitioned": 1},
    "priv_rows": {"auto": 0, "off": 1, "on": 2},
    "dp_dense": {"auto": 0, "records": 1, "partials": 2},
    "heavy_chunk": {"auto": 0, "off": 1, "on": 2},
    "dp_xchg": {"collective": 0, "p2p": 1, "p2p_pipe": 2},
}


_P = C.c_void_p


class RaeBuffers(C.Structure):
    _fields_ = [
        ("W", _P), ("Wb", _P), ("A", _P), ("Ab", _P), ("C1", _P), ("C2", _P), ("R3", _P),
        ("acc_W", _P), ("acc_Wb", _P), ("acc_A", _P), ("acc_Ab", _P), ("acc_C1", _P),
        ("acc_C2", _P), ("acc_R3", _P),
        ("indptr", _P), ("indices", _P), ("values", _P), ("args1", _P), ("args2", _P),
        ("neg1", _P), ("neg2", _P), ("exchange", _P), ("costs", _P),
    ]


class RaeEvalArgs(C.Structure):
    """rae_eval_args (include/rae.h): the forward-only objective's arguments."""
    _fields_ = [
        ("decoder", C.c_int32), ("relations", C.c_int32), ("embed", C.c_int32),
        ("neg_samples", C.c_int32), ("n_entities", C.c_int64), ("alpha", C.c_float),
        ("W", _P), ("Wb", _P), ("A", _P), ("Ab", _P), ("C1", _P), ("C2", _P), ("R3", _P),
        ("indptr", _P), ("indices", _P), ("values", _P), ("args1", _P), ("args2", _P),
        ("neg1", _P), ("neg2", _P), ("neg_stride", C.c_int64),
        ("row0", C.c_int64), ("nrows", C.c_int64),
        ("terms_out", _P), ("sums_out", _P), ("workspace", _P), ("workspace_bytes", C.c_int64),
    ]


class RaeRankArgs(C.Structure):
    """rae_rank_args (include/rae.h): caller-given queries against every entity."""
    _fields_ = [
        ("Q", _P), ("ldq", C.c_int64), ("nq", C.c_int64), ("add", _P), ("target", _P),
        ("skip", _P), ("A", _P), ("Ab", _P), ("n_entities", C.c_int64), ("embed", C.c_int32),
        ("greater", _P), ("equal", _P), ("lse", _P),
        ("workspace", _P), ("workspace_bytes", C.c_int64),
    ]


class RaeRankOut(C.Structure):
    """rae_rank_out (include/rae.h): the outputs of rae_eval_rank."""
    _fields_ = [
        ("greater", _P), ("equal", _P), ("target", _P), ("lse", _P), ("summary", _P),
        ("hits_k", C.c_int32 * 4),
    ]


# the rank kernel's tile and strip constants (csrc/rae_rank.hpp RAE_RK_*)
RAE_RK_TQ, RAE_RK_TE, RAE_RK_MAXSTRIPS, RAE_RK_QCHUNK, RAE_RK_ROWCHUNK = 128, 128, 128, 4096, 2048


class RaeTopkArgs(C.Structure):
    """rae_topk_args (include/rae.h): the `top` best entities of caller-given queries."""
    _fields_ = [
        ("Q", _P), ("ldq", C.c_int64), ("nq", C.c_int64), ("add", _P), ("skip", _P),
        ("A", _P), ("Ab", _P), ("n_entities", C.c_int64), ("embed", C.c_int32),
        ("top", C.c_int32), ("ents_out", _P), ("scores_out", _P),
        ("workspace", _P), ("workspace_bytes", C.c_int64),
    ]


class RaeTopkOut(C.Structure):
    """rae_topk_out (include/rae.h): the outputs of rae_eval_topk."""
    _fields_ = [("ents", _P), ("scores", _P), ("top", C.c_int32), ("skip_true", C.c_int32)]


# rae_topk_queries: largest `top` and the queries per launch round (csrc/rae_topk.hpp RAE_ETK_*)
RAE_ETK_MAXTOP, RAE_ETK_QCHUNK = 32, 1024


class RaeRelscoreArgs(C.Structure):
    """rae_relscore_args (include/rae.h): the decoder's relation scores of caller-given pairs."""
    _fields_ = [
        ("decoder", C.c_int32), ("relations", C.c_int32), ("embed", C.c_int32),
        ("n_entities", C.c_int64), ("A", _P), ("C1", _P), ("C2", _P), ("R3", _P),
        ("e1", _P), ("e2", _P), ("nq", C.c_int64), ("psi_out", _P), ("ldp", C.c_int64),
        ("workspace", _P), ("workspace_bytes", C.c_int64),
    ]


class RaeRelOut(C.Structure):
    """rae_rel_out (include/rae.h): the outputs of rae_eval_relations."""
    _fields_ = [("psi", _P), ("joint", _P), ("labels_dec", _P), ("labels_joint", _P)]


# the relation-score kernel's constants (csrc/rae_relscore.hpp RAE_RS_*): pairs / rows per launch
# round, K rows per slab, and the examples of one workgroup at `relations`
RAE_RS_ROUND, RAE_RS_TK = 16384, 32


def relscore_block_examples(relations: int) -> int:
    return 128 if relations <= 16 else 64


class RaeFtopkArgs(C.Structure):
    """rae_ftopk_args (include/rae.h): the `top` best features of every relation by W."""
    _fields_ = [
        ("W", _P), ("n_features", C.c_int64), ("relations", C.c_int32), ("ldw", C.c_int64),
        ("support", _P), ("min_support", C.c_int32), ("centre", C.c_int32), ("top", C.c_int32),
        ("feats_out", _P), ("scores_out", _P),
        ("workspace", _P), ("workspace_bytes", C.c_int64),
    ]


# rae_feature_topk: largest `top` and the selection kernel's decomposition (csrc/rae_feature.hpp
# RAE_FT_*): row phases per workgroup, rows of a phase in flight, shortest strip, most strips
RAE_FT_MAXTOP, RAE_FT_WAVES, RAE_FT_U, RAE_FT_STRIP_ROWS, RAE_FT_MAXSTRIPS = 32, 8, 8, 512, 128


def ftopk_strips(d: int) -> int:
    """The strips rae_feature_topk cuts d features into (csrc/rae_feature.hpp ftopk_strips)."""
    return max(1, min(RAE_FT_MAXSTRIPS, -(-int(d) // RAE_FT_STRIP_ROWS)))


def ftopk_strip_rows(d: int) -> int:
    step = RAE_FT_WAVES * RAE_FT_U
    return -(-(-(-int(d) // ftopk_strips(d))) // step) * step


class RaeExemplarArgs(C.Structure):
    """rae_exemplar_args (include/rae.h): per cluster the `top` rows by a per-row score."""
    _fields_ = [
        ("labels", _P), ("scores", _P), ("nrows", C.c_int64), ("relations", C.c_int32),
        ("top", C.c_int32), ("largest", C.c_int32), ("rows_out", _P), ("scores_out", _P),
        ("workspace", _P), ("workspace_bytes", C.c_int64),
    ]


# rae_cluster_exemplars: largest `top` and the decomposition (csrc/rae_exemplar.hpp RAE_CX_*):
# shortest strip, most strips, the LDS a workgroup of several waves keeps its lists within
RAE_CX_MAXTOP, RAE_CX_STRIP_ROWS, RAE_CX_MAXSTRIPS, RAE_CX_LDS_WG = 32, 4096, 128, 64 * 1024


def cex_strips(nrows: int) -> int:
    """The strips rae_cluster_exemplars cuts nrows rows into (csrc/rae_exemplar.hpp cex_strips)."""
    return max(1, min(RAE_CX_MAXSTRIPS, -(-int(nrows) // RAE_CX_STRIP_ROWS)))


def cex_waves(relations: int, top: int) -> int:
    """Waves per workgroup of k_cexemplar: the most of 4, 2, 1 whose lists fit 64 KiB."""
    lb = int(relations) * int(top) * 8
    return 4 if 4 * lb <= RAE_CX_LDS_WG else (2 if 2 * lb <= RAE_CX_LDS_WG else 1)


LABEL_MODES = ("encoder", "decoder", "joint")


class RaeError(RuntimeError):
    pass


_lib = None


def load(path: str | None = None):
    """Load librae_hip.so (raises if it has not been built)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("RAE_LIB", LIB_PATH)
    if not os.path.exists(p):
        raise RaeError(f"{p} not found: build the HIP extension first "
                       "(python __graft_entry__.py build)")
    lib = C.CDLL(p)
    lib.rae_build_id.restype = C.c_char_p
    if path is None and "RAE_LIB" not in os.environ:     # RAE_LIB: explicit variant builds
        want = source_build_id()
        got = lib.rae_build_id().decode()
        if want is not None and got != want:
            raise RaeError(f"{p} was built from other sources (build id {got}, sources {want}): "
                           "rebuild it (python __graft_entry__.py build)")
    lib.rae_last_error.restype = C.c_char_p
    lib.rae_version.restype = C.c_int
    lib.rae_exchange_record_floats.restype = C.c_int64
    lib.rae_exchange_record_floats.argtypes = [C.POINTER(RaeConfig)]
    lib.rae_exchange_floats.restype = C.c_int64
    lib.rae_exchange_floats.argtypes = [C.POINTER(RaeConfig)]
    lib.rae_plan_create.argtypes = [C.POINTER(RaeConfig), C.POINTER(RaeBuffers), C.POINTER(_P)]
    lib.rae_plan_destroy.argtypes = [_P]
    lib.rae_plan_forms.argtypes = [_P, C.POINTER(RaeConfig)]
    lib.rae_dp_block_floats.argtypes = [C.POINTER(RaeConfig), C.c_int32, C.c_int32]
    lib.rae_dp_block_floats.restype = C.c_int64
    lib.rae_set_dp_buffers.argtypes = [_P, _P, _P, C.c_int32, C.c_int32]
    lib.rae_dp_list_max.argtypes = [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    for fn in ("rae_dp_pack", "rae_dp_unpack", "rae_dp_pack_at", "rae_dp_unpack_at"):
        getattr(lib, fn).argtypes = [_P, C.c_int64, _P]
        getattr(lib, fn).restype = C.c_int
    for fn in ("rae_set_dp_buffers", "rae_dp_list_max"):
        getattr(lib, fn).restype = C.c_int
    lib.rae_ipc_export.argtypes = [_P, _P, C.POINTER(C.c_int64)]
    lib.rae_ipc_open.argtypes = [_P, C.POINTER(_P)]
    lib.rae_ipc_close.argtypes = [_P]
    lib.rae_p2p_signals.argtypes = [_P]
    lib.rae_p2p_signals.restype = _P
    lib.rae_set_peer.argtypes = [_P, C.c_int32, _P, _P, _P, _P, _P]
    lib.rae_set_p2p_timeout.argtypes = [_P, C.c_double]
    lib.rae_p2p_prologue.argtypes = [_P, C.c_int64, C.c_int32, _P]
    for fn in ("rae_ipc_export", "rae_ipc_open", "rae_ipc_close", "rae_set_peer",
               "rae_set_p2p_timeout", "rae_p2p_prologue"):
        getattr(lib, fn).restype = C.c_int
    lib.rae_set_negatives.argtypes = [_P, _P, _P, C.c_int32, C.c_int64]
    lib.rae_set_cursor.argtypes = [_P, C.c_int64, _P]
    lib.rae_advance_cursor.argtypes = [_P, C.c_int64, _P]
    lib.rae_cursor_moves.argtypes = [_P]
    lib.rae_cursor_moves.restype = C.c_int64
    lib.rae_step_forward.argtypes = [_P, C.c_int64, _P]
    lib.rae_step_update.argtypes = [_P, C.c_int64, _P]
    lib.rae_step_forward_at.argtypes = [_P, C.c_int64, _P]
    lib.rae_step_update_at.argtypes = [_P, C.c_int64, _P]
    lib.rae_train_step.argtypes = [_P, C.c_int64, _P, _P, _P]
    lib.rae_check.argtypes = [_P]
    lib.rae_check_on.argtypes = [_P, _P]
    lib.rae_build_index.argtypes = [_P, C.c_int64, C.c_int64, _P]
    lib.rae_index_window.argtypes = [_P]
    lib.rae_index_window.restype = C.c_int64
    lib.rae_index_dims.argtypes = [_P, C.POINTER(C.c_int64), C.c_int32]
    lib.rae_index_dims.restype = C.c_int
    lib.rae_index_read.argtypes = [_P, C.c_int64, C.c_int32, _P, C.c_int64]
    lib.rae_index_read.restype = C.c_int
    lib.rae_label.argtypes = [_P, _P, _P, _P, _P, C.c_int32, C.c_int64, C.c_int64, _P, _P, _P]
    lib.rae_eval_workspace_bytes.argtypes = [C.POINTER(RaeEvalArgs)]
    lib.rae_eval_workspace_bytes.restype = C.c_int64
    lib.rae_eval_cost.argtypes = [C.POINTER(RaeEvalArgs), _P]
    lib.rae_eval_cost.restype = C.c_int
    lib.rae_rank_queries.argtypes = [C.POINTER(RaeRankArgs), _P]
    lib.rae_rank_queries.restype = C.c_int
    lib.rae_eval_rank.argtypes = [C.POINTER(RaeEvalArgs), C.POINTER(RaeRankOut), _P]
    lib.rae_eval_rank.restype = C.c_int
    lib.rae_rank_workspace_bytes.argtypes = [C.POINTER(RaeRankArgs), C.POINTER(RaeEvalArgs)]
    lib.rae_rank_workspace_bytes.restype = C.c_int64
    lib.rae_topk_queries.argtypes = [C.POINTER(RaeTopkArgs), _P]
    lib.rae_topk_queries.restype = C.c_int
    lib.rae_eval_topk.argtypes = [C.POINTER(RaeEvalArgs), C.POINTER(RaeTopkOut), _P]
    lib.rae_eval_topk.restype = C.c_int
    lib.rae_topk_workspace_bytes.argtypes = [C.POINTER(RaeTopkArgs), C.POINTER(RaeEvalArgs),
                                             C.c_int32]
    lib.rae_topk_workspace_bytes.restype = C.c_int64
    lib.rae_relation_scores.argtypes = [C.POINTER(RaeRelscoreArgs), _P]
    lib.rae_relation_scores.restype = C.c_int
    lib.rae_eval_relations.argtypes = [C.POINTER(RaeEvalArgs), C.POINTER(RaeRelOut), _P]
    lib.rae_eval_relations.restype = C.c_int
    lib.rae_relscore_workspace_bytes.argtypes = [C.POINTER(RaeRelscoreArgs),
                                                 C.POINTER(RaeEvalArgs)]
    lib.rae_relscore_workspace_bytes.restype = C.c_int64
    lib.rae_cluster_count.argtypes = [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P]
    lib.rae_cluster_count.restype = C.c_int
    lib.rae_b3_metrics.argtypes = [_P, _P, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P]
    lib.rae_b3_metrics.restype = C.c_int
    lib.rae_row_keys.argtypes = [_P, _P, _P, _P, C.c_int64, C.c_int64, C.c_int64, _P, _P]
    lib.rae_row_keys.restype = C.c_int
    lib.rae_cluster_key_count.argtypes = [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P]
    lib.rae_cluster_key_count.restype = C.c_int
    lib.rae_cluster_topk.argtypes = [_P, C.c_int32, C.c_int32, C.c_int64, C.c_int32, _P, _P, _P]
    lib.rae_cluster_topk.restype = C.c_int
    lib.rae_feature_support.argtypes = [_P, _P, _P, C.c_int64, C.c_int64, C.c_int64, C.c_int32,
                                        _P, _P]
    lib.rae_feature_support.restype = C.c_int
    lib.rae_feature_topk_workspace_bytes.argtypes = [C.POINTER(RaeFtopkArgs)]
    lib.rae_feature_topk_workspace_bytes.restype = C.c_int64
    lib.rae_feature_topk.argtypes = [C.POINTER(RaeFtopkArgs), _P]
    lib.rae_feature_topk.restype = C.c_int
    lib.rae_label_stats.argtypes = [_P, _P, _P, _P, _P, C.c_int32, C.c_int64, C.c_int64, _P, _P,
                                    _P, _P]
    lib.rae_label_stats.restype = C.c_int
    lib.rae_cluster_exemplars_workspace_bytes.argtypes = [C.POINTER(RaeExemplarArgs)]
    lib.rae_cluster_exemplars_workspace_bytes.restype = C.c_int64
    lib.rae_cluster_exemplars.argtypes = [C.POINTER(RaeExemplarArgs), _P]
    lib.rae_cluster_exemplars.restype = C.c_int
    lib.rae_neg_sample.argtypes = [_P, C.c_int64, _P, C.c_int64, _P, _P]
    lib.rae_neg_sample_philox.argtypes = [_P, C.c_int64, C.c_uint64, C.c_uint64, C.c_int64, _P, _P]
    lib.rae_time_next.argtypes = [_P, _P, _P]
    lib.rae_stream_copy.argtypes = [_P, _P, C.c_int64, _P]
    lib.rae_mfma_probe.argtypes = [C.c_int64, C.c_int32, _P, _P]
    lib.rae_event_create.argtypes = [C.POINTER(_P)]
    lib.rae_event_destroy.argtypes = [_P]
    lib.rae_event_elapsed_ms.argtypes = [_P, _P, C.POINTER(C.c_float)]
    for fn in ("rae_stream_copy", "rae_mfma_probe", "rae_time_next", "rae_event_create", "rae_event_destroy", "rae_event_elapsed_ms",
               "rae_neg_sample", "rae_neg_sample_philox", "rae_plan_create", "rae_plan_destroy", "rae_plan_forms", "rae_set_negatives", "rae_set_cursor",
               "rae_advance_cursor", "rae_step_forward", "rae_step_update", "rae_train_step",
               "rae_step_forward_at", "rae_step_update_at",
               "rae_check", "rae_check_on", "rae_label", "rae_build_index"):
        getattr(lib, fn).restype = C.c_int
    if path is None:
        _lib = lib
    return lib


def check(rc: int, what: str = "rae call"):
    if rc != RAE_OK:
        msg = load().rae_last_error()
        raise RaeError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def ptr(t) -> int | None:
    """Device pointer of a torch tensor (None for None)."""
    if t is None:
        return None
    return t.data_ptr()
