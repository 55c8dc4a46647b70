"""ctypes loader for libmpfmt.so (the C ABI of include/mpfmt.h).

The product path has NO CPU fallback: if the shared library is missing this module raises, and if
no gfx950 device is visible `Context()` raises `MPFMTError` (MPFMT_ERR_NODEVICE).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("MPFMT_LIB_PATH") or os.path.join(_HERE, "libmpfmt.so")   # override: kernel experiments (tools/)
_LIB = None

OK, ERR_ARG, ERR_STATE, ERR_HIP, ERR_NODEVICE, ERR_CAPACITY, ERR_INFEASIBLE = 0, -1, -2, -3, -4, -5, -6
RETRY = 1            # mpfmt_allgather_free_mask_finish on a ctx driven inside a group: relaunch every ctx, then finish again
GOAL_RECT, GOAL_BALL, GOAL_POINT = 0, 1, 2
MAX_DIM = 16

c_d_p = C.POINTER(C.c_double)
c_i64_p = C.POINTER(C.c_int64)
c_u64_p = C.POINTER(C.c_uint64)
c_u8_p = C.POINTER(C.c_uint8)


class MPFMTError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libmpfmt error %d: %s" % (code, msg))
        self.code = code


class FmtResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("cost", C.c_double), ("z", C.c_int64), ("collision_checks", C.c_int64),
                ("path_len", C.c_int64), ("nnz", C.c_int64), ("ms_graph", C.c_double), ("ms_sweep", C.c_double),
                ("ms_host_loop", C.c_double)]


class WfInfo(C.Structure):
    _fields_ = [("done", C.c_int32), ("nz", C.c_int32), ("nx", C.c_int32), ("nconn", C.c_int32), ("ntrip", C.c_int32),
                ("iters", C.c_int64), ("checks", C.c_int64), ("cmin", C.c_double), ("tot_z", C.c_int64), ("tot_x", C.c_int64),
                ("tot_conn", C.c_int64)]


class SsspInfo(C.Structure):
    _fields_ = [("reached", C.c_int64), ("rounds", C.c_int64), ("relaxations", C.c_int64), ("ms_device", C.c_double)]


class FieldInfo(C.Structure):
    _fields_ = [("reached", C.c_int64), ("invalidated", C.c_int64), ("dirty_columns", C.c_int64), ("columns_read", C.c_int64),
                ("column_visits", C.c_int64), ("entries_read", C.c_int64), ("rounds", C.c_int64), ("relaxations", C.c_int64),
                ("ms_device", C.c_double), ("path", C.c_int32), ("pad_", C.c_int32)]


class TogoInfo(C.Structure):
    _fields_ = [("reached", C.c_int64), ("invalidated", C.c_int64), ("dirty_columns", C.c_int64), ("columns_read", C.c_int64),
                ("column_visits", C.c_int64), ("entries_read", C.c_int64), ("rounds", C.c_int64), ("relaxations", C.c_int64),
                ("atomics", C.c_int64), ("ms_device", C.c_double), ("path", C.c_int32), ("pad_", C.c_int32)]


class ShortcutInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("iterations_done", C.c_int32), ("n_out", C.c_int64), ("max_working_len", C.c_int64),
                ("max_halvings", C.c_int64), ("collision_checks", C.c_int64), ("tests_evaluated", C.c_int64)]


class RoadmapInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("pad_", C.c_int32), ("near_s", C.c_int64), ("usable_s", C.c_int64), ("near_g", C.c_int64),
                ("usable_g", C.c_int64), ("rounds", C.c_int64), ("path_len", C.c_int64), ("ms_device", C.c_double)]


class GrowInfo(C.Structure):
    _fields_ = [("candidates", C.c_int64), ("entries", C.c_int64), ("dropped", C.c_int64)]


class RoadmapMatrixInfo(C.Structure):
    _fields_ = [("groups", C.c_int64), ("rounds", C.c_int64), ("near_s", C.c_int64), ("usable_s", C.c_int64), ("near_g", C.c_int64),
                ("usable_g", C.c_int64), ("ms_device", C.c_double)]


class DiscInfo(C.Structure):
    _fields_ = [("n_out", C.c_int64), ("steps", C.c_int64), ("duration", C.c_double)]


class SteerShortcutInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("iterations_done", C.c_int32), ("n_out", C.c_int64), ("max_working_len", C.c_int64),
                ("inserted", C.c_int64), ("legs_blocked", C.c_int64), ("collision_checks", C.c_int64), ("tests_evaluated", C.c_int64),
                ("cost_in", C.c_double), ("cost_out", C.c_double)]


SHORTCUT_DONE, SHORTCUT_TRUNCATED, SHORTCUT_STUCK = 0, 1, 2
STEER_SHORTCUT_SLACK = 1.0 + 2.0 ** -30          # the acceptance slack of the steering shortcut (include/mpfmt.h), exact in binary64
DI_MF_PROBE_TERMS = 16                # MPFMT_DI_MF_PROBE_TERMS
SPACE_EUCLID, SPACE_DI, SPACE_DUBINS, SPACE_REEDSSHEPP = 0, 1, 2, 3
DISC_DT, DISC_N = 0, 1
ROADMAP_SOLVED, ROADMAP_NO_PATH, ROADMAP_START_BLOCKED, ROADMAP_GOAL_BLOCKED = 0, 1, 2, 3
WF_SINGLE, WF_EAGER, WF_LAZY = 1, 2, 4
COMM_ID_BYTES = 128
OPT_STEER_SHAPES_DELTA = "steer_shapes_delta"     # Context.set_option: shape edits under a swept steering graph in place (default 0)
OPT_SAMPLES_ADD_KEEPS_FIELDS = "samples_add_keeps_fields"      # Context.set_option: an in-place samples_add carries the tracked fields (default 0)

# every symbol include/mpfmt.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("mpfmt_ctx_create", C.c_int32, [C.c_int32, C.POINTER(C.c_void_p)]),
    ("mpfmt_ctx_destroy", C.c_int32, [C.c_void_p]),
    ("mpfmt_last_error", C.c_char_p, [C.c_void_p]),
    ("mpfmt_version", C.c_char_p, []),
    ("mpfmt_set_stream", C.c_int32, [C.c_void_p, C.c_void_p]),
    ("mpfmt_set_shard", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32]),
    ("mpfmt_upload_samples", C.c_int32, [C.c_void_p, c_d_p, C.c_int64, C.c_int32]),
    ("mpfmt_upload_samples_device", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    ("mpfmt_graph_radius", C.c_int32, [C.c_void_p, c_d_p]),
    ("mpfmt_samples_add", C.c_int32, [C.c_void_p, c_d_p, C.c_int64, C.c_double]),
    ("mpfmt_samples_add_device", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_double]),
    ("mpfmt_host_graph_grow", C.c_int32, [C.c_int64, C.c_int64, C.c_int32, c_d_p, c_i64_p, C.POINTER(C.c_int32), c_d_p, c_u64_p, c_d_p, C.c_int32,
                                          c_d_p, c_d_p, C.c_double, c_i64_p, C.POINTER(C.c_int32), c_d_p, c_u64_p, C.c_int64, c_i64_p,
                                          C.POINTER(GrowInfo)]),
    ("mpfmt_upload_boxes", C.c_int32, [C.c_void_p, c_d_p, C.c_int32, C.c_int32, c_d_p, c_d_p, C.c_int32]),
    ("mpfmt_boxes_add", C.c_int32, [C.c_void_p, c_d_p, C.c_int32]),
    ("mpfmt_boxes_remove", C.c_int32, [C.c_void_p, c_i64_p, C.c_int32]),
    ("mpfmt_steer_mask_read", C.c_int32, [C.c_void_p, c_u64_p, c_u8_p]),
    ("mpfmt_rdisc_count", C.c_int32, [C.c_void_p, C.c_double, c_i64_p, c_i64_p]),
    ("mpfmt_rdisc_fill", C.c_int32, [C.c_void_p, c_i64_p, c_d_p]),
    ("mpfmt_rdisc_query", C.c_int32, [C.c_void_p, C.c_int64, C.c_double, c_i64_p, c_d_p, C.c_int64, c_i64_p]),
    ("mpfmt_points_free", C.c_int32, [C.c_void_p, c_i64_p, C.c_int64, c_u64_p]),
    ("mpfmt_edges_free", C.c_int32, [C.c_void_p, c_i64_p, c_i64_p, C.c_int64, c_u64_p]),
    ("mpfmt_graph_edges_free", C.c_int32, [C.c_void_p, c_u64_p]),
    ("mpfmt_states_free", C.c_int32, [C.c_void_p, c_d_p, C.c_int64, c_u64_p]),
    ("mpfmt_motions_free", C.c_int32, [C.c_void_p, c_d_p, c_d_p, C.c_int64, c_u64_p]),
    ("mpfmt_euclid_steer", C.c_int32, [C.c_void_p, c_i64_p, c_i64_p, C.c_int64, c_d_p, c_d_p]),
    ("mpfmt_euclid_propagate", C.c_int32, [C.c_void_p, c_i64_p, C.c_int64, c_d_p, c_d_p, c_d_p, c_d_p]),
    ("mpfmt_expand", C.c_int32, [C.c_void_p, c_u64_p, c_u64_p, c_u64_p, c_d_p, c_i64_p, C.c_int64,
                                 c_i64_p, c_i64_p, c_d_p, c_u8_p, C.c_int64, c_i64_p]),
    ("mpfmt_knn_count", C.c_int32, [C.c_void_p, C.c_int64, c_i64_p, c_i64_p]),
    ("mpfmt_knn_fill", C.c_int32, [C.c_void_p, c_i64_p, c_d_p, c_u64_p]),
    ("mpfmt_knn_graph_edges_free", C.c_int32, [C.c_void_p, c_u64_p]),
    ("mpfmt_knn_fmtstar", C.c_int32, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, c_d_p, c_i64_p, c_d_p, c_i64_p, C.POINTER(FmtResult)]),
    ("mpfmt_fmtstar", C.c_int32, [C.c_void_p, C.c_double, C.c_int64, C.c_int32, C.c_int32, c_d_p,
                                  c_i64_p, c_d_p, c_i64_p, C.POINTER(FmtResult)]),
    ("mpfmt_host_fmt_recursion", C.c_int32, [C.c_int64, C.c_int32, c_d_p, c_i64_p, C.POINTER(C.c_int32), c_d_p, c_u64_p, c_u64_p,
                                             c_d_p, c_d_p, C.c_int64, C.c_int32, c_d_p, c_i64_p, c_d_p, c_i64_p,
                                             C.POINTER(FmtResult)]),
    ("mpfmt_host_graph_sssp", C.c_int32, [C.c_int64, c_i64_p, C.POINTER(C.c_int32), c_d_p, c_u64_p, c_u64_p, C.c_int64, c_d_p, c_i64_p]),
    ("mpfmt_graph_sssp", C.c_int32, [C.c_void_p, c_i64_p, C.c_int64, C.c_int32, c_d_p, c_i64_p, C.POINTER(SsspInfo)]),
    ("mpfmt_graph_sssp_multi", C.c_int32, [C.c_void_p, c_i64_p, C.c_int64, C.c_int32, c_d_p, c_i64_p, C.POINTER(SsspInfo)]),
    ("mpfmt_host_graph_sssp_to", C.c_int32, [C.c_int64, c_i64_p, C.POINTER(C.c_int32), c_d_p, c_u64_p, c_u64_p, c_i64_p, C.c_int64, c_d_p,
                                             c_i64_p]),
    ("mpfmt_graph_sssp_to", C.c_int32, [C.c_void_p, c_i64_p, C.c_int64, C.c_int32, c_d_p, c_i64_p, C.POINTER(SsspInfo)]),
    ("mpfmt_di_prmstar", C.c_int32, [C.c_void_p, C.c_double, C.c_double, C.c_int64, C.c_int32, C.c_int32, c_d_p,
                                     c_i64_p, c_d_p, c_i64_p, C.POINTER(FmtResult)]),
    ("mpfmt_dubins_prmstar", C.c_int32, [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int64, C.c_int32, C.c_int32, c_d_p,
                                         c_i64_p, c_d_p, c_i64_p, C.POINTER(FmtResult)]),
    ("mpfmt_reedsshepp_prmstar", C.c_int32, [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int64, C.c_int32, C.c_int32, c_d_p,
                                             c_i64_p, c_d_p, c_i64_p, C.POINTER(FmtResult)]),
    ("mpfmt_field_begin", C.c_int32, [C.c_void_p, C.c_int64, C.c_int32, C.POINTER(FieldInfo)]),
    ("mpfmt_field_update", C.c_int32, [C.c_void_p, C.POINTER(FieldInfo)]),
    ("mpfmt_field_read", C.c_int32, [C.c_void_p, c_d_p, c_i64_p]),
    ("mpfmt_field_goal", C.c_int32, [C.c_void_p, C.c_int32, c_d_p, c_i64_p, C.POINTER(FmtResult)]),
    ("mpfmt_field_drop", C.c_int32, [C.c_void_p]),
    ("mpfmt_togo_begin", C.c_int32, [C.c_void_p, c_i64_p, C.c_int64, C.c_int32, C.POINTER(TogoInfo)]),
    ("mpfmt_togo_update", C.c_int32, [C.c_void_p, C.POINTER(TogoInfo)]),
    ("mpfmt_togo_read", C.c_int32, [C.c_void_p, c_d_p, c_i64_p]),
    ("mpfmt_togo_targets_add", C.c_int32, [C.c_void_p, c_i64_p, C.c_int64]),
    ("mpfmt_togo_drop", C.c_int32, [C.c_void_p]),
    ("mpfmt_host_field_repair", C.c_int32, [C.c_int64, c_i64_p, C.POINTER(C.c_int32), c_d_p, c_u64_p, c_u64_p, c_u64_p, C.c_int64, c_d_p, c_i64_p,
                                            c_i64_p]),
    ("mpfmt_prmstar", C.c_int32, [C.c_void_p, C.c_double, C.c_int64, C.c_int32, C.c_int32, c_d_p, c_i64_p, c_d_p, c_i64_p,
                                  C.POINTER(FmtResult)]),
    ("mpfmt_knn_prmstar", C.c_int32, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, c_d_p, c_i64_p, c_d_p, c_i64_p,
                                      C.POINTER(FmtResult)]),
    ("mpfmt_roadmap_near", C.c_int32, [C.c_void_p, c_d_p, C.c_int64, C.c_int32, c_i64_p, C.c_int64, c_i64_p, c_d_p, c_u64_p, c_i64_p]),
    ("mpfmt_roadmap_attach", C.c_int32, [C.c_void_p, c_d_p, C.c_int64, c_d_p, c_i64_p, c_d_p]),
    ("mpfmt_roadmap_query", C.c_int32, [C.c_void_p, c_d_p, c_d_p, C.c_int64, C.c_int32, c_d_p, c_i64_p, c_i64_p, C.c_int64, C.POINTER(RoadmapInfo)]),
    ("mpfmt_steer_roadmap_near", C.c_int32, [C.c_void_p, c_d_p, C.c_int64, C.c_int32, c_i64_p, C.c_int64, c_i64_p, c_d_p, c_u64_p, c_i64_p]),
    ("mpfmt_steer_roadmap_attach", C.c_int32, [C.c_void_p, c_d_p, C.c_int64, c_d_p, c_i64_p, c_d_p]),
    ("mpfmt_steer_roadmap_query", C.c_int32, [C.c_void_p, c_d_p, c_d_p, C.c_int64, C.c_int32, c_d_p, c_i64_p, c_i64_p, C.c_int64,
                                              C.POINTER(RoadmapInfo)]),
    ("mpfmt_roadmap_matrix", C.c_int32, [C.c_void_p, c_d_p, C.c_int64, c_d_p, C.c_int64, C.c_int32, c_d_p, C.POINTER(C.c_int32),
                                         C.POINTER(RoadmapMatrixInfo)]),
    ("mpfmt_host_roadmap_query", C.c_int32, [C.c_int64, C.c_int32, c_d_p, c_i64_p, C.POINTER(C.c_int32), c_d_p, c_u64_p, c_u64_p, c_d_p, C.c_int32,
                                             c_d_p, c_d_p, C.c_double, c_d_p, c_d_p, c_d_p, c_i64_p, C.c_int64, C.POINTER(RoadmapInfo)]),
    ("mpfmt_host_adaptive_shortcut", C.c_int32, [c_d_p, C.c_int64, C.c_int32, c_d_p, C.c_int32, c_d_p, c_d_p, C.c_int32, C.c_int64, c_d_p, C.c_int64,
                                                 c_d_p, C.POINTER(ShortcutInfo)]),
    ("mpfmt_adaptive_shortcut_batch", C.c_int32, [C.c_void_p, c_d_p, c_i64_p, C.c_int64, C.c_int32, C.c_int64, c_d_p, c_i64_p, C.c_int64, c_d_p,
                                                  C.POINTER(ShortcutInfo)]),
    ("mpfmt_adaptive_shortcut", C.c_int32, [C.c_void_p, c_d_p, C.c_int64, C.c_int32, C.c_int64, c_d_p, C.c_int64, c_d_p, C.POINTER(ShortcutInfo)]),
    ("mpfmt_host_discretize", C.c_int32, [C.c_int32, C.c_int32, c_d_p, c_d_p, C.c_int64, C.c_int32, C.c_double, C.c_int64, C.c_int32, c_d_p, c_d_p,
                                          C.POINTER(C.c_int32), C.c_int64, C.POINTER(DiscInfo)]),
    ("mpfmt_discretize_batch", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, c_d_p, c_d_p, c_i64_p, C.c_int64, C.c_int32, C.c_double, C.c_int64,
                                           C.c_int32, c_d_p, c_d_p, C.POINTER(C.c_int32), c_i64_p, C.c_int64, C.POINTER(DiscInfo)]),
    ("mpfmt_discretize", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, c_d_p, c_d_p, C.c_int64, C.c_int32, C.c_double, C.c_int64, C.c_int32, c_d_p,
                                     c_d_p, C.POINTER(C.c_int32), C.c_int64, C.POINTER(DiscInfo)]),
    ("mpfmt_steer_motions_free", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, c_d_p, c_d_p, c_d_p, C.c_int64, c_u64_p, c_d_p, c_d_p,
                                             C.POINTER(C.c_int32)]),
    ("mpfmt_steer_shortcut_batch", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, c_d_p, c_d_p, c_i64_p, C.c_int64, C.c_int32, C.c_int64, c_d_p,
                                               c_i64_p, C.c_int64, c_d_p, C.POINTER(C.c_int32), C.POINTER(SteerShortcutInfo)]),
    ("mpfmt_steer_shortcut", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, c_d_p, c_d_p, C.c_int64, C.c_int32, C.c_int64, c_d_p, C.c_int64,
                                         c_d_p, C.POINTER(C.c_int32), C.POINTER(SteerShortcutInfo)]),
    ("mpfmt_mc_edges_collision", C.c_int32, [C.c_void_p, c_i64_p, c_i64_p, C.c_int64, C.c_double, C.c_int64, C.c_uint64, c_i64_p]),
    ("mpfmt_mc_edges_collision_is", C.c_int32, [C.c_void_p, c_i64_p, c_i64_p, C.c_int64, C.c_double, C.c_int64, C.c_uint64, C.POINTER(C.c_uint64)]),
    ("mpfmt_mc_edges_collision_ais", C.c_int32, [C.c_void_p, c_i64_p, c_i64_p, C.c_int64, C.c_double, C.c_int64, C.c_uint64, C.POINTER(C.c_uint64),
                                                 c_d_p]),
    ("mpfmt_dubins_graph_count", C.c_int32, [C.c_void_p, C.c_double, C.c_double, C.c_double, c_i64_p, c_i64_p]),
    ("mpfmt_dubins_graph_fill", C.c_int32, [C.c_void_p, c_i64_p, c_d_p]),
    ("mpfmt_dubins_graph_edges_free", C.c_int32, [C.c_void_p, c_u64_p, c_u8_p]),
    ("mpfmt_dubins_steer", C.c_int32, [C.c_void_p, c_d_p, c_d_p, C.c_int64, C.c_double, C.c_double, c_d_p, c_d_p]),
    ("mpfmt_dubins_fmtstar", C.c_int32, [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int64, C.c_int32, C.c_int32, c_d_p,
                                         c_i64_p, c_d_p, c_i64_p, C.POINTER(FmtResult)]),
    ("mpfmt_reedsshepp_graph_count", C.c_int32, [C.c_void_p, C.c_double, C.c_double, C.c_double, c_i64_p, c_i64_p]),
    ("mpfmt_reedsshepp_graph_fill", C.c_int32, [C.c_void_p, c_i64_p, c_d_p]),
    ("mpfmt_reedsshepp_graph_edges_free", C.c_int32, [C.c_void_p, c_u64_p, c_u8_p]),
    ("mpfmt_reedsshepp_steer", C.c_int32, [C.c_void_p, c_d_p, c_d_p, C.c_int64, C.c_double, C.c_double, c_d_p, c_d_p,
                                           C.POINTER(C.c_int32)]),
    ("mpfmt_reedsshepp_fmtstar", C.c_int32, [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int64, C.c_int32, C.c_int32, c_d_p,
                                             c_i64_p, c_d_p, c_i64_p, C.POINTER(FmtResult)]),
    ("mpfmt_closest", C.c_int32, [C.c_void_p, c_d_p, C.c_int64, c_d_p, c_d_p, c_d_p, c_i64_p, c_i64_p]),
    ("mpfmt_closeR", C.c_int32, [C.c_void_p, c_d_p, C.c_int64, c_d_p, C.c_double, c_i64_p, C.c_int64, c_i64_p, c_d_p, c_d_p,
                                 c_i64_p, c_i64_p]),
    ("mpfmt_upload_shapes2d", C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), c_d_p, c_d_p, c_d_p]),
    ("mpfmt_shapes2d_add", C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), c_d_p]),
    ("mpfmt_shapes2d_remove", C.c_int32, [C.c_void_p, c_i64_p, C.c_int32]),
    ("mpfmt_graph_import", C.c_int32, [C.c_void_p, C.c_double, c_i64_p, c_i64_p, c_d_p]),
    ("mpfmt_sample_free", C.c_int32, [C.c_void_p, C.c_uint64, C.c_int64, c_d_p, C.c_int32, c_d_p, C.c_int32, c_d_p, c_i64_p]),
    ("mpfmt_sample_free_biased", C.c_int32, [C.c_void_p, C.c_uint64, C.c_int64, c_d_p, C.c_int32, c_d_p, C.c_int32, C.c_double, c_d_p,
                                             c_i64_p]),
    ("mpfmt_path_free", C.c_int32, [C.c_void_p, c_d_p, C.c_int64, C.POINTER(C.c_int32), c_u64_p]),
    ("mpfmt_di_graph_count", C.c_int32, [C.c_void_p, C.c_double, C.c_double, c_i64_p, c_i64_p]),
    ("mpfmt_di_graph_fill", C.c_int32, [C.c_void_p, c_i64_p, c_d_p, c_d_p]),
    ("mpfmt_di_graph_edges_free", C.c_int32, [C.c_void_p, c_u64_p, c_u8_p]),
    ("mpfmt_di_graph_step_device", C.c_int32, [C.c_void_p, C.c_double, C.c_double, c_i64_p]),
    ("mpfmt_di_graph_device_ptrs", C.c_int32, [C.c_void_p] + [C.POINTER(C.c_void_p)] * 6),
    ("mpfmt_di_steer", C.c_int32, [C.c_void_p, c_d_p, c_d_p, C.c_int64, C.c_int32, C.c_double, C.c_double, c_d_p, c_d_p]),
    ("mpfmt_di_mf_probe", C.c_int32, [C.c_void_p, C.c_double, C.c_double, C.POINTER(C.c_float), C.POINTER(C.c_uint16), C.POINTER(C.c_uint16), c_d_p, c_i64_p]),
    ("mpfmt_di_fmtstar", C.c_int32, [C.c_void_p, C.c_double, C.c_double, C.c_int64, C.c_int32, C.c_int32, c_d_p,
                                     c_i64_p, c_d_p, c_i64_p, C.POINTER(FmtResult)]),
    ("mpfmt_dubins_fmtstar_wavefront", C.c_int32, [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int64, C.c_int32, C.c_int32, c_d_p,
                                                   C.c_double, C.c_int32, c_i64_p, c_d_p, c_i64_p, C.POINTER(FmtResult), C.POINTER(WfInfo)]),
    ("mpfmt_reedsshepp_fmtstar_wavefront", C.c_int32, [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int64, C.c_int32, C.c_int32, c_d_p,
                                                       C.c_double, C.c_int32, c_i64_p, c_d_p, c_i64_p, C.POINTER(FmtResult), C.POINTER(WfInfo)]),
    ("mpfmt_di_fmtstar_wavefront", C.c_int32, [C.c_void_p, C.c_double, C.c_double, C.c_int64, C.c_int32, C.c_int32, c_d_p, C.c_double,
                                               C.c_int32, c_i64_p, c_d_p, c_i64_p, C.POINTER(FmtResult), C.POINTER(WfInfo)]),
    ("mpfmt_graph_build_device", C.c_int32, [C.c_void_p, C.c_double, c_i64_p]),
    ("mpfmt_graph_step_device", C.c_int32, [C.c_void_p, C.c_double, c_i64_p]),
    ("mpfmt_graph_step_launch", C.c_int32, [C.c_void_p, C.c_double]),
    ("mpfmt_graph_step_finish", C.c_int32, [C.c_void_p, c_i64_p]),
    ("mpfmt_graph_sweep_device", C.c_int32, [C.c_void_p]),
    ("mpfmt_graph_device_ptrs", C.c_int32, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                            C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    ("mpfmt_graph_export", C.c_int32, [C.c_void_p, c_i64_p, c_i64_p, c_d_p, c_u64_p, c_d_p]),
    ("mpfmt_pinned_alloc", C.c_int32, [C.c_int64, C.POINTER(C.c_void_p)]),
    ("mpfmt_pinned_free", C.c_int32, [C.c_void_p]),
    ("mpfmt_export_arena", C.c_int32, [C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]),
    ("mpfmt_graph_export_pinned", C.c_int32, [C.c_void_p, C.POINTER(c_i64_p), C.POINTER(c_i64_p), C.POINTER(c_d_p), C.POINTER(c_u64_p),
                                              c_i64_p, C.POINTER(C.c_double)]),
    ("mpfmt_rdisc_stream", C.c_int32, [C.c_void_p, C.c_double, c_d_p, c_u64_p, C.c_int32, c_i64_p, c_i64_p, c_i64_p, c_d_p, c_i64_p]),
    ("mpfmt_shard_info", C.c_int32, [C.c_void_p, c_i64_p, c_i64_p, c_i64_p]),
    ("mpfmt_fmtstar_wavefront", C.c_int32, [C.c_void_p, C.c_double, C.c_int64, C.c_int32, C.c_int32, c_d_p, C.c_double, C.c_int32,
                                            c_i64_p, c_d_p, c_i64_p, C.POINTER(FmtResult), C.POINTER(WfInfo)]),
    ("mpfmt_wf_begin", C.c_int32, [C.c_void_p, C.c_double, C.c_int64, C.c_int32, C.c_int32, c_d_p, C.c_double, C.c_int32]),
    ("mpfmt_wf_step", C.c_int32, [C.c_void_p, C.POINTER(WfInfo)]),
    ("mpfmt_wf_state", C.c_int32, [C.c_void_p, c_u64_p, c_u64_p, c_d_p, c_i64_p]),
    ("mpfmt_wf_batch", C.c_int32, [C.c_void_p, c_i64_p, C.c_int64, c_i64_p]),
    ("mpfmt_wf_triples", C.c_int32, [C.c_void_p, C.c_int64, c_i64_p, c_i64_p, c_d_p, c_i64_p]),
    ("mpfmt_wf_commit", C.c_int32, [C.c_void_p, C.c_int64, c_i64_p, c_i64_p, c_d_p]),
    ("mpfmt_wf_finish", C.c_int32, [C.c_void_p, c_i64_p, c_d_p, c_i64_p, C.POINTER(FmtResult)]),
    ("mpfmt_comm_unique_id", C.c_int32, [c_u8_p]),
    ("mpfmt_comm_create", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, c_u8_p]),
    ("mpfmt_comm_destroy", C.c_int32, [C.c_void_p]),
    ("mpfmt_group_begin", C.c_int32, []),
    ("mpfmt_group_end", C.c_int32, []),
    ("mpfmt_allgather_free_mask", C.c_int32, [C.c_void_p, C.POINTER(C.c_void_p), c_i64_p, c_i64_p, c_i64_p]),
    ("mpfmt_allgather_free_mask_launch", C.c_int32, [C.c_void_p, C.c_int64]),
    ("mpfmt_allgather_free_mask_finish", C.c_int32, [C.c_void_p, C.POINTER(C.c_void_p), c_i64_p, c_i64_p, c_i64_p]),
    ("mpfmt_allgather_free_mask_relaunch", C.c_int32, [C.c_void_p]),
    ("mpfmt_set_state_bounds", C.c_int32, [C.c_void_p, c_d_p, c_d_p, C.c_int32]),
    ("mpfmt_timing_reset", C.c_int32, [C.c_void_p]),
    ("mpfmt_timing_get", C.c_int32, [C.c_void_p, C.c_char_p, c_d_p, c_i64_p]),
    ("mpfmt_set_option", C.c_int32, [C.c_void_p, C.c_char_p, C.c_int64]),
    ("mpfmt_get_stat", C.c_int32, [C.c_void_p, C.c_char_p, c_i64_p]),
    ("mpfmt_graph_stats", C.c_int32, [C.c_void_p, c_i64_p, c_i64_p, c_i64_p, c_i64_p]),
]


def so_path():
    return _SO


def lib():
    """Load libmpfmt.so.  torch is imported first so that the one HIP runtime already mapped into the
    process (torch bundles libamdhip64.so.7) also serves this library (same SONAME)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(_SO):
            raise ImportError("libmpfmt.so is not built (%s); run `python __graft_entry__.py` / `make -C %s`; "
                              "there is no CPU fallback" % (_SO, os.path.join(_HERE, "csrc")))
        try:
            import torch  # noqa: F401  (maps the HIP runtime)
        except Exception:  # pragma: no cover - torch is plumbing only
            pass
        L = C.CDLL(_SO)
        for name, res, args in SYMBOLS:
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _LIB = L
    return _LIB


def comm_unique_id():
    """128-byte RCCL id (rank 0 calls this; the host distributes it)."""
    u = np.zeros(COMM_ID_BYTES, dtype=np.uint8)
    rc = lib().mpfmt_comm_unique_id(u.ctypes.data_as(c_u8_p))
    if rc != OK:
        raise MPFMTError(rc, lib().mpfmt_last_error(None).decode())
    return u.tobytes()


def group_begin():
    """ncclGroupStart: one host thread driving several ctxs brackets every round of *_launch calls (include/mpfmt.h)."""
    rc = lib().mpfmt_group_begin()
    if rc != OK:
        raise MPFMTError(rc, lib().mpfmt_last_error(None).decode())


def group_end():
    rc = lib().mpfmt_group_end()
    if rc != OK:
        raise MPFMTError(rc, lib().mpfmt_last_error(None).decode())


def nwords(n):
    return (int(n) + 63) // 64


def unpack_bits(mask, n):
    b = np.unpackbits(np.ascontiguousarray(mask).view(np.uint8), bitorder="little")
    return b[:n].astype(bool)


def pack_bits(bits):
    bits = np.asarray(bits, dtype=bool)
    pad = np.zeros(max(nwords(bits.size), 1) * 64, dtype=np.uint8)
    pad[:bits.size] = bits
    return np.packbits(pad, bitorder="little").view(np.uint64)


def _dp(a):
    return None if a is None else a.ctypes.data_as(c_d_p)


def _ip(a):
    return None if a is None else a.ctypes.data_as(c_i64_p)


def _dp_or_none(a):
    return None if a is None else a.ctypes.data_as(c_d_p)


def _up(a):
    return None if a is None else a.ctypes.data_as(c_u64_p)


def host_fmt_recursion(X, colptr0, rowval0, nzval, efree, F, goal_kind, goal_params, ss_lo=None, ss_hi=None, init_idx=1):
    """The sequential part of fmtstar! (fmt.jl:43-101) on a finished graph; host only, no GPU needed.
    colptr0 / rowval0 are 0-based (rowval0 int32), efree / F packed uint64 bit masks (F None: checkpts=false)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    N, d = X.shape
    colptr0 = np.ascontiguousarray(colptr0, dtype=np.int64)
    rowval0 = np.ascontiguousarray(rowval0, dtype=np.int32)
    nzval = np.ascontiguousarray(nzval, dtype=np.float64)
    efree = np.ascontiguousarray(efree, dtype=np.uint64)
    Fp = None if F is None else np.ascontiguousarray(F, dtype=np.uint64)
    lo = None if ss_lo is None else np.ascontiguousarray(ss_lo, dtype=np.float64)
    hi = None if ss_hi is None else np.ascontiguousarray(ss_hi, dtype=np.float64)
    g = np.ascontiguousarray(goal_params, dtype=np.float64)
    A = np.empty(N, dtype=np.int64); Cc = np.empty(N, dtype=np.float64); path = np.empty(N, dtype=np.int64)
    res = FmtResult()
    rc = lib().mpfmt_host_fmt_recursion(N, d, _dp(X), _ip(colptr0), rowval0.ctypes.data_as(C.POINTER(C.c_int32)), _dp(nzval),
                                        _up(efree), None if Fp is None else _up(Fp), None if lo is None else _dp(lo),
                                        None if hi is None else _dp(hi), int(init_idx), int(goal_kind), _dp(g),
                                        _ip(A), _dp(Cc), _ip(path), C.byref(res))
    if rc != 0:
        raise MPFMTError(rc, "mpfmt_host_fmt_recursion rejected its arguments")
    return dict(status=int(res.status), cost=float(res.cost), z=int(res.z), collision_checks=int(res.collision_checks),
                nnz=int(res.nnz), ms_host_loop=float(res.ms_host_loop), A=A, C=Cc, path=path[:res.path_len].copy())


def host_graph_sssp(colptr0, rowval0, nzval, efree, F=None, source=1, want_parents=True):
    """PRM* cost-to-come field of one source (1-based) by a host Dijkstra over the device-native arrays (include/mpfmt.h, "roadmap
    queries"); host only, no GPU needed.  colptr0 / rowval0 0-based (rowval0 int32), efree / F packed uint64 bit masks (F None:
    checkpts=false).  Returns (C, A): C = +Inf for unreached samples, A 1-based parents (0 = none; None without want_parents)."""
    colptr0 = np.ascontiguousarray(colptr0, dtype=np.int64)
    N = colptr0.size - 1
    rowval0 = np.ascontiguousarray(rowval0, dtype=np.int32)
    nzval = np.ascontiguousarray(nzval, dtype=np.float64)
    efree = np.ascontiguousarray(efree, dtype=np.uint64)
    Fp = None if F is None else np.ascontiguousarray(F, dtype=np.uint64)
    Cc = np.empty(max(N, 1), dtype=np.float64)
    A = np.empty(max(N, 1), dtype=np.int64) if want_parents else None
    rc = lib().mpfmt_host_graph_sssp(N, _ip(colptr0), rowval0.ctypes.data_as(C.POINTER(C.c_int32)), _dp(nzval), _up(efree), _up(Fp),
                                     int(source), _dp(Cc), _ip(A))
    if rc != 0:
        raise MPFMTError(rc, "mpfmt_host_graph_sssp rejected its arguments")
    return Cc[:N], (None if A is None else A[:N])


def host_graph_sssp_to(colptr0, rowval0, nzval, efree, F=None, targets=(), want_successors=True):
    """PRM* cost-to-go field of a target set (1-based) by a host Dijkstra over the reversed edges of the device-native arrays
    (include/mpfmt.h, "cost-to-go"); host only, no GPU needed.  Arguments as host_graph_sssp.  Returns (G, S): G = +Inf where no target
    is reachable, 0 on the targets; S 1-based successors (0 = target or unreached; None without want_successors)."""
    colptr0 = np.ascontiguousarray(colptr0, dtype=np.int64)
    N = colptr0.size - 1
    rowval0 = np.ascontiguousarray(rowval0, dtype=np.int32)
    nzval = np.ascontiguousarray(nzval, dtype=np.float64)
    efree = np.ascontiguousarray(efree, dtype=np.uint64)
    Fp = None if F is None else np.ascontiguousarray(F, dtype=np.uint64)
    tg = np.ascontiguousarray(np.atleast_1d(np.asarray(targets, dtype=np.int64)))
    G = np.empty(max(N, 1), dtype=np.float64)
    S = np.empty(max(N, 1), dtype=np.int64) if want_successors else None
    rc = lib().mpfmt_host_graph_sssp_to(N, _ip(colptr0), rowval0.ctypes.data_as(C.POINTER(C.c_int32)), _dp(nzval), _up(efree), _up(Fp),
                                        _ip(tg) if tg.size else None, int(tg.size), _dp(G), _ip(S))
    if rc != 0:
        raise MPFMTError(rc, "mpfmt_host_graph_sssp_to rejected its arguments")
    return G[:N], (None if S is None else S[:N])


def host_field_repair(colptr0, rowval0, nzval, efree, F, dirty, C_old, A_old, source=1):
    """The repair of a tracked field on the host (include/mpfmt.h, "a cost-to-come field kept valid across box edits"), no GPU needed:
    the old field (C_old, A_old) of `source` (1-based), the NEW mask efree and point bitmap F (None: checkpts=false), the bitmap
    `dirty` of the columns the edits flagged (packed uint64 over samples).  Returns (C, A, invalidated)."""
    colptr0 = np.ascontiguousarray(colptr0, dtype=np.int64)
    N = colptr0.size - 1
    rowval0 = np.ascontiguousarray(rowval0, dtype=np.int32)
    nzval = np.ascontiguousarray(nzval, dtype=np.float64)
    efree = np.ascontiguousarray(efree, dtype=np.uint64)
    Fp = None if F is None else np.ascontiguousarray(F, dtype=np.uint64)
    dirty = np.ascontiguousarray(dirty, dtype=np.uint64)
    if dirty.size < nwords(N):
        raise ValueError("dirty must hold one bit per sample")
    Cc = np.array(C_old, dtype=np.float64).reshape(-1).copy()
    A = np.array(A_old, dtype=np.int64).reshape(-1).copy()
    if Cc.size != N or A.size != N:
        raise ValueError("C_old / A_old must have N entries")
    inv = np.zeros(1, dtype=np.int64)
    rc = lib().mpfmt_host_field_repair(N, _ip(colptr0), rowval0.ctypes.data_as(C.POINTER(C.c_int32)), _dp(nzval), _up(efree), _up(Fp), _up(dirty),
                                       int(source), _dp(Cc), _ip(A), _ip(inv))
    if rc != 0:
        raise MPFMTError(rc, "mpfmt_host_field_repair rejected its arguments")
    return Cc, A, int(inv[0])


def _field_info(i):
    return {k: getattr(i, k) for k, _ in FieldInfo._fields_ if k != "pad_"}


def _togo_info(i):
    return {k: getattr(i, k) for k, _ in TogoInfo._fields_ if k != "pad_"}


def _roadmap_info(i):
    return dict(status=int(i.status), near_s=int(i.near_s), usable_s=int(i.usable_s), near_g=int(i.near_g), usable_g=int(i.usable_g),
                rounds=int(i.rounds), path_len=int(i.path_len), ms_device=float(i.ms_device))


def host_roadmap_query(X, colptr0, rowval0, nzval, efree, F, lohi, ss_lo, ss_hi, r, s, g):
    """One pair query (s, g) for states that are not samples, on the host (include/mpfmt.h, "roadmap queries for external states"): no
    GPU needed; the checker of Context.roadmap_query.  X (N, d); colptr0 / rowval0 0-based (rowval0 int32), efree / F packed uint64 bit
    masks (F None: checkpts=false); lohi (M, 2, d); ss_lo / ss_hi or None.  Returns (cost, path (1-based samples between s and g), info)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    N, d = X.shape
    colptr0 = np.ascontiguousarray(colptr0, dtype=np.int64)
    rowval0 = np.ascontiguousarray(rowval0, dtype=np.int32)
    nzval = np.ascontiguousarray(nzval, dtype=np.float64)
    efree = np.ascontiguousarray(efree, dtype=np.uint64)
    Fp = None if F is None else np.ascontiguousarray(F, dtype=np.uint64)
    lohi = np.ascontiguousarray(lohi, dtype=np.float64).reshape(-1, 2, d)
    lo = None if ss_lo is None else np.ascontiguousarray(ss_lo, dtype=np.float64)
    hi = None if ss_hi is None else np.ascontiguousarray(ss_hi, dtype=np.float64)
    s = np.ascontiguousarray(s, dtype=np.float64).reshape(d)
    g = np.ascontiguousarray(g, dtype=np.float64).reshape(d)
    cost = C.c_double(0.0)
    path = np.empty(N + 1, dtype=np.int64)
    info = RoadmapInfo()
    rc = lib().mpfmt_host_roadmap_query(N, d, _dp(X), _ip(colptr0), rowval0.ctypes.data_as(C.POINTER(C.c_int32)), _dp(nzval), _up(efree), _up(Fp),
                                        _dp(lohi), lohi.shape[0], _dp(lo), _dp(hi), float(r), _dp(s), _dp(g), C.byref(cost), _ip(path), N + 1,
                                        C.byref(info))
    if rc != 0:
        raise MPFMTError(rc, "mpfmt_host_roadmap_query rejected its arguments")
    return float(cost.value), path[:info.path_len].copy(), _roadmap_info(info)


def host_graph_grow(X_all, n_old, colptr0, rowval0, nzval, efree, lohi, ss_lo, ss_hi, r_new):
    """The r-disc graph of the first n_old samples of X_all (N, d) grown by the others, on the host (include/mpfmt.h, "growing the sample
    set"): no GPU needed; the normative statement of Context.samples_add.  colptr0 / rowval0 0-based (rowval0 int32), efree packed
    uint64; lohi (M, 2, d); ss_lo / ss_hi or None.  Returns (colptr0, rowval0, nzval, efree, info) of the grown graph at r_new."""
    X = np.ascontiguousarray(X_all, dtype=np.float64)
    N, d = X.shape
    n_old = int(n_old)
    colptr0 = np.ascontiguousarray(colptr0, dtype=np.int64)
    rowval0 = np.ascontiguousarray(rowval0, dtype=np.int32)
    nzval = np.ascontiguousarray(nzval, dtype=np.float64)
    efree = np.ascontiguousarray(efree, dtype=np.uint64)
    lohi = np.ascontiguousarray(lohi, dtype=np.float64).reshape(-1, 2, d)
    lo = None if ss_lo is None else np.ascontiguousarray(ss_lo, dtype=np.float64)
    hi = None if ss_hi is None else np.ascontiguousarray(ss_hi, dtype=np.float64)
    if colptr0.size != n_old + 1 or n_old > N:
        raise ValueError("colptr0 must have n_old + 1 entries, n_old <= N")
    ocp = np.zeros(N + 1, dtype=np.int64)
    nnz = C.c_int64(0)
    info = GrowInfo()
    L = lib()
    args = (n_old, N - n_old, d, _dp(X), _ip(colptr0), _ip32(rowval0), _dp(nzval), _up(efree), _dp(lohi), lohi.shape[0], _dp(lo), _dp(hi),
            float(r_new), _ip(ocp))
    rc = L.mpfmt_host_graph_grow(*args, None, None, None, 0, C.byref(nnz), C.byref(info))
    if rc != 0:
        raise MPFMTError(rc, "mpfmt_host_graph_grow rejected its arguments")
    n = nnz.value
    orv = np.zeros(max(n, 1), dtype=np.int32); onz = np.zeros(max(n, 1), dtype=np.float64); oef = np.zeros(max(nwords(n), 1), dtype=np.uint64)
    if n > 0:
        rc = L.mpfmt_host_graph_grow(*args, _ip32(orv), _dp(onz), _up(oef), n, C.byref(nnz), C.byref(info))
        if rc != 0:
            raise MPFMTError(rc, "mpfmt_host_graph_grow failed")
    return ocp, orv[:n], onz[:n], oef[:nwords(n)], dict(candidates=int(info.candidates), entries=int(info.entries), dropped=int(info.dropped))


def _shortcut_info(i):
    return dict(status=int(i.status), iterations_done=int(i.iterations_done), n_out=int(i.n_out), max_working_len=int(i.max_working_len),
                max_halvings=int(i.max_halvings), collision_checks=int(i.collision_checks), tests_evaluated=int(i.tests_evaluated))


def host_adaptive_shortcut(path, lohi, ss_lo=None, ss_hi=None, iterations=10, max_states=256):
    """adaptive_shortcut (src/postprocessors.jl:28-39) of one path (n, d) against the AABB checker lohi (M, 2, d) on the host: no GPU
    needed; the CPU baseline and the checker of Context.adaptive_shortcut (include/mpfmt.h, "adaptive shortcutting").
    Returns (smoothed path (n_out, d), cumcost (n_out,), info dict)."""
    P = np.ascontiguousarray(path, dtype=np.float64)
    if P.ndim != 2:
        raise ValueError("path must be (n, d)")
    n, d = P.shape
    lohi = np.ascontiguousarray(lohi, dtype=np.float64).reshape(-1, 2, d)
    lo = None if ss_lo is None else np.ascontiguousarray(ss_lo, dtype=np.float64)
    hi = None if ss_hi is None else np.ascontiguousarray(ss_hi, dtype=np.float64)
    cap = max(int(max_states), n, 2)
    out = np.empty((cap, d), dtype=np.float64); cc = np.empty(cap, dtype=np.float64)
    info = ShortcutInfo()
    rc = lib().mpfmt_host_adaptive_shortcut(_dp(P), n, d, _dp(lohi), lohi.shape[0], _dp(lo), _dp(hi), int(iterations), int(max_states), _dp(out), cap,
                                            _dp(cc), C.byref(info))
    if rc != 0:
        raise MPFMTError(rc, "mpfmt_host_adaptive_shortcut rejected its arguments")
    return out[:info.n_out].copy(), cc[:info.n_out].copy(), _shortcut_info(info)


def _steer_shortcut_info(i):
    return dict(status=int(i.status), iterations_done=int(i.iterations_done), n_out=int(i.n_out), max_working_len=int(i.max_working_len),
                inserted=int(i.inserted), legs_blocked=int(i.legs_blocked), collision_checks=int(i.collision_checks),
                tests_evaluated=int(i.tests_evaluated), cost_in=float(i.cost_in), cost_out=float(i.cost_out))


def _steer_params(space, params):
    prm = None if params is None else np.ascontiguousarray(params, dtype=np.float64).reshape(-1)
    if prm is None or prm.size != 2:
        raise ValueError("params = (rho, tmax) for the double integrator, (turn_radius, speed) for the cars")
    return prm


def _disc_info(i):
    return dict(n_out=int(i.n_out), steps=int(i.steps), duration=float(i.duration))


def _disc_args(space, params, dt, n, append_end):
    """(params array or None, mode, dt, n_samples, append_end) of the discretise calls: exactly one of dt / n is given."""
    if (dt is None) == (n is None):
        raise ValueError("give exactly one of dt (time_discretize_solution!) and n (time_space_solution!)")
    prm = None if params is None else np.ascontiguousarray(params, dtype=np.float64).reshape(-1)
    if space in (SPACE_DI, SPACE_DUBINS, SPACE_REEDSSHEPP) and (prm is None or prm.size != 2):
        raise ValueError("params = (rho, r) for the double integrator, (turn_radius, speed) for the cars")
    return prm, (DISC_DT if n is None else DISC_N), (0.0 if dt is None else float(dt)), (0 if n is None else int(n)), (1 if append_end else 0)


def _ip32(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def host_discretize(path, space, params=None, dt=None, n=None, append_end=False):
    """Time discretisation of one path (n_states, d) on the host: the sequential loop of src/statespaces.jl:104-119 (include/mpfmt.h,
    "time discretisation"); no GPU needed; the CPU baseline and the checker of Context.discretize.
    Returns (X (n_out, d), T (n_out,), seg (n_out,) int32 1-based, info dict)."""
    P = np.ascontiguousarray(path, dtype=np.float64)
    if P.ndim != 2:
        raise ValueError("path must be (n, d)")
    prm, mode, dtv, ns, app = _disc_args(space, params, dt, n, append_end)
    info = DiscInfo()
    L = lib()
    rc = L.mpfmt_host_discretize(int(space), P.shape[1], _dp(prm), _dp(P), P.shape[0], mode, dtv, ns, app, None, None, None, 0, C.byref(info))
    if rc != 0:
        raise MPFMTError(rc, "mpfmt_host_discretize rejected its arguments")
    cap = int(info.n_out)
    X = np.empty((cap, P.shape[1]), dtype=np.float64); T = np.empty(cap, dtype=np.float64); seg = np.empty(cap, dtype=np.int32)
    rc = L.mpfmt_host_discretize(int(space), P.shape[1], _dp(prm), _dp(P), P.shape[0], mode, dtv, ns, app, _dp(X), _dp(T), _ip32(seg), cap,
                                 C.byref(info))
    if rc != 0:
        raise MPFMTError(rc, "mpfmt_host_discretize failed")
    return X, T, seg, _disc_info(info)


class Context:
    """One GPU context = one `mpfmt_ctx`.  Thin, numpy-in / numpy-out; indices 1-based like the ABI."""

    def __init__(self, device=0):
        self._L = lib()
        h = C.c_void_p()
        rc = self._L.mpfmt_ctx_create(int(device), C.byref(h))
        if rc != OK:
            raise MPFMTError(rc, self._L.mpfmt_last_error(None).decode())
        self._h = h
        self.N = 0
        self.d = 0
        self.dw = 0
        self.nnz = None
        self._cc_epoch = 0                                   # counts the changes of the collision checker (what a bound checker compares)

    def close(self):
        if getattr(self, "_h", None):
            self._L.mpfmt_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        if rc != OK:
            raise MPFMTError(rc, self._L.mpfmt_last_error(self._h).decode())

    # ---- setup ----------------------------------------------------------------------------------
    def set_stream(self, stream_handle):
        self._chk(self._L.mpfmt_set_stream(self._h, C.c_void_p(stream_handle)))

    def set_state_bounds(self, ss_lo, ss_hi):
        """BoundedStateSpace lo / hi of any state dimension (after upload_shapes2d: the bounds of a steering space over the 2-D world)."""
        lo = np.ascontiguousarray(ss_lo, dtype=np.float64); hi = np.ascontiguousarray(ss_hi, dtype=np.float64)
        self._cc_epoch += 1
        self._chk(self._L.mpfmt_set_state_bounds(self._h, _dp(lo), _dp(hi), len(lo)))

    def set_shard(self, rank, world):
        self._chk(self._L.mpfmt_set_shard(self._h, int(rank), int(world)))

    def upload_samples(self, X):
        """X: (N, d) float64 C-contiguous == Julia d x N column-major."""
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.ndim != 2:
            raise ValueError("X must be (N, d)")
        self._chk(self._L.mpfmt_upload_samples(self._h, _dp(X), X.shape[0], X.shape[1]))
        self.N, self.d = X.shape
        self.nnz = None

    def upload_samples_device(self, ptr, N, d):
        """The same from a device pointer (N x d float64, C-contiguous, on this ctx's GPU): no PCIe crossing."""
        self._chk(self._L.mpfmt_upload_samples_device(self._h, C.c_void_p(int(ptr)), int(N), int(d)))
        self.N, self.d = int(N), int(d)
        self.nnz = None

    def samples_add(self, X_add, r=None):
        """Append X_add (n_add, d) behind the ctx's samples (mpfmt_samples_add).  A resident, swept r-disc graph of an unsharded ctx
        with the N-D AABB checker follows in place -- graph and mask byte for byte those of a fresh step on the concatenated set at r
        (default: the graph's radius, r <= it) -- and stat("samples_add_path") == 1; in every other state the ctx is what upload_samples
        of the concatenated set leaves (then r only has to be finite and positive).  The tracked fields are dropped, unless
        set_option("samples_add_keeps_fields", 1) was given and the call went in place: then stat("samples_add_fields_carried") has
        bit 0 (field) / bit 1 (cost-to-go) set, the fields stay tracked with the changed columns pending, field_update / togo_update
        repair them (path 1) to the bytes of graph_sssp / graph_sssp_to on the grown graph, and field_read / field_goal / togo_read
        raise ERR_STATE until that update."""
        X_add = np.ascontiguousarray(X_add, dtype=np.float64)
        if X_add.ndim == 1:
            X_add = X_add[None]
        if X_add.ndim != 2 or (X_add.shape[0] > 0 and X_add.shape[1] != self.d):
            raise ValueError("X_add must be (n_add, %s)" % self.d)
        self._chk(self._L.mpfmt_samples_add(self._h, _dp(X_add) if X_add.shape[0] else None, X_add.shape[0], self._grow_radius(r)))
        self.N += X_add.shape[0]
        self.nnz = None

    def samples_add_device(self, ptr, n_add, r=None):
        """The same from a device pointer (n_add x d float64, C-contiguous, on this ctx's GPU)."""
        self._chk(self._L.mpfmt_samples_add_device(self._h, C.c_void_p(int(ptr)), int(n_add), self._grow_radius(r)))
        self.N += int(n_add)
        self.nnz = None

    def _grow_radius(self, r):
        if r is not None:
            return float(r)
        g = C.c_double(0.0)
        if self._L.mpfmt_graph_radius(self._h, C.byref(g)) == OK and g.value > 0.0:
            return g.value
        return 1.0                                           # (nothing to grow: any finite positive radius invalidates alike)

    def upload_boxes(self, lohi, ss_lo=None, ss_hi=None, dw=None):
        """lohi: (M, 2, dw) float64 (lo then hi per box)."""
        lohi = np.ascontiguousarray(lohi, dtype=np.float64)
        if lohi.size == 0:
            if dw is None:
                dw = lohi.shape[2] if (lohi.ndim == 3 and lohi.shape[2] > 0) else (len(ss_lo) if ss_lo is not None else self.d)
            lohi = np.zeros((0, 2, dw))
        if lohi.ndim != 3 or lohi.shape[1] != 2:
            raise ValueError("lohi must be (M, 2, dw)")
        M, _, dw = lohi.shape
        lo = None if ss_lo is None else np.ascontiguousarray(ss_lo, dtype=np.float64)
        hi = None if ss_hi is None else np.ascontiguousarray(ss_hi, dtype=np.float64)
        ds = 0 if lo is None else lo.size
        self._cc_epoch += 1
        self._chk(self._L.mpfmt_upload_boxes(self._h, _dp(lohi), M, dw, _dp(lo), _dp(hi), ds))
        self.dw = dw

    def boxes_add(self, lohi):
        """Append boxes lohi (M_add, 2, dw) to the uploaded PointRobotNDBoxes set in place (mpfmt_boxes_add): the free-edge mask of a
        swept resident graph -- Euclidean, or a steering graph with its segment counts -- is brought up to date instead of being thrown
        away (stat("boxes_delta_path") == 1)."""
        lohi = np.ascontiguousarray(lohi, dtype=np.float64)
        if lohi.size == 0:
            lohi = np.zeros((0, 2, self.dw))
        if lohi.ndim == 2:
            lohi = lohi[None]
        if lohi.ndim != 3 or lohi.shape[1] != 2:
            raise ValueError("lohi must be (M_add, 2, dw)")
        if lohi.shape[0] > 0 and lohi.shape[2] != self.dw:
            raise ValueError("boxes of dimension %d added to a set of dimension %d" % (lohi.shape[2], self.dw))
        self._chk(self._L.mpfmt_boxes_add(self._h, _dp(lohi), lohi.shape[0]))
        self._cc_epoch += 1

    def boxes_remove(self, ids):
        """Remove the boxes `ids` (1-based, distinct) from the uploaded set in place (mpfmt_boxes_remove); the others keep their order."""
        ids = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.int64)
        self._chk(self._L.mpfmt_boxes_remove(self._h, _ip(ids), ids.size))
        self._cc_epoch += 1

    def steer_mask_read(self):
        """(mask, nseg) of the resident, swept steering graph as they are (mpfmt_steer_mask_read): after boxes_add / boxes_remove, the
        bytes a whole sweep of the current list writes.  Sweeps nothing; MPFMTError (ERR_STATE) when no swept steering graph is resident."""
        n = self.stat("nnz")
        mask = np.zeros(max(nwords(n), 1), dtype=np.uint64)
        nseg = np.zeros(max(n, 1), dtype=np.uint8)
        self._chk(self._L.mpfmt_steer_mask_read(self._h, _up(mask), nseg.ctypes.data_as(c_u8_p)))
        return mask[:nwords(n)], nseg[:n]

    @staticmethod
    def _encode_shapes2d(shapes):
        """(kinds, nverts, data) of a shape list as mpfmt_upload_shapes2d / mpfmt_shapes2d_add take them."""
        kinds = np.array([0 if s[0] == "circle" else 1 for s in shapes], dtype=np.int32)
        nv = np.array([0 if s[0] == "circle" else len(s[1]) for s in shapes], dtype=np.int32)
        parts = [np.array([s[1][0], s[1][1], s[2]], dtype=np.float64) if s[0] == "circle"
                 else np.ascontiguousarray(s[1], dtype=np.float64).reshape(-1) for s in shapes]
        data = np.concatenate(parts) if parts else np.zeros(1)
        return kinds, nv, data

    def shapes_add(self, shapes):
        """Append shapes (the tuples of upload_shapes2d) to the uploaded 2-D SAT world in place (mpfmt_shapes2d_add): the free-edge mask
        of a swept resident Euclidean graph is brought up to date instead of being thrown away (stat("boxes_delta_path") == 1), and
        the tracked fields stay.  After set_option("steer_shapes_delta", 1) the same holds for the mask and segment counts of a swept
        steering graph (double integrator in R^4, Dubins, Reeds-Shepp): steer_mask_read() gives the bytes of a whole sweep."""
        shapes = list(shapes)
        kinds, nv, data = self._encode_shapes2d(shapes)
        i32 = C.POINTER(C.c_int32)
        self._chk(self._L.mpfmt_shapes2d_add(self._h, len(shapes), kinds.ctypes.data_as(i32), nv.ctypes.data_as(i32), _dp(data)))
        self._cc_epoch += 1

    def shapes_remove(self, ids):
        """Remove the shapes `ids` (1-based, distinct) from the uploaded 2-D SAT world in place (mpfmt_shapes2d_remove); the others
        keep their order."""
        ids = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.int64)
        self._chk(self._L.mpfmt_shapes2d_remove(self._h, _ip(ids), ids.size))
        self._cc_epoch += 1

    def upload_shapes2d(self, shapes, ss_lo=None, ss_hi=None):
        """2-D SAT world: shapes = [("circle", (cx, cy), r) | ("polygon", [(x, y), ...]), ...] (a flat Compound2D)."""
        kinds, nv, data = self._encode_shapes2d(shapes)
        lo = None if ss_lo is None else np.ascontiguousarray(ss_lo, dtype=np.float64)
        hi = None if ss_hi is None else np.ascontiguousarray(ss_hi, dtype=np.float64)
        i32 = C.POINTER(C.c_int32)
        self._cc_epoch += 1
        self._chk(self._L.mpfmt_upload_shapes2d(self._h, len(shapes), kinds.ctypes.data_as(i32), nv.ctypes.data_as(i32), _dp(data),
                                                None if lo is None else _dp(lo), None if hi is None else _dp(hi)))
        self.dw = 2

    # ---- r-disc ---------------------------------------------------------------------------------
    def rdisc_count(self, r):
        colptr = np.empty(self.N + 1, dtype=np.int64)
        nnz = C.c_int64()
        self._chk(self._L.mpfmt_rdisc_count(self._h, float(r), _ip(colptr), C.byref(nnz)))
        self.nnz = nnz.value
        return colptr, nnz.value

    def rdisc_fill(self):
        nnz = self.nnz
        rowval = np.empty(max(nnz, 1), dtype=np.int64)
        nzval = np.empty(max(nnz, 1), dtype=np.float64)
        self._chk(self._L.mpfmt_rdisc_fill(self._h, _ip(rowval), _dp(nzval)))
        return rowval[:nnz], nzval[:nnz]

    def rdisc_graph(self, r):
        """(colptr, rowval, nzval), all 1-based like SparseMatrixCSC."""
        colptr, _ = self.rdisc_count(r)
        rowval, nzval = self.rdisc_fill()
        return colptr, rowval, nzval

    def rdisc_query(self, v, r, cap=None):
        cap = self.N if cap is None else cap
        inds = np.empty(max(cap, 1), dtype=np.int64)
        ds = np.empty(max(cap, 1), dtype=np.float64)
        k = C.c_int64()
        self._chk(self._L.mpfmt_rdisc_query(self._h, int(v), float(r), _ip(inds), _dp(ds), cap, C.byref(k)))
        return inds[:k.value].copy(), ds[:k.value].copy()

    # ---- sweeps ---------------------------------------------------------------------------------
    def points_free(self, idx=None):
        n = self.N if idx is None else len(idx)
        idx = None if idx is None else np.ascontiguousarray(idx, dtype=np.int64)
        mask = np.zeros(max(nwords(n), 1), dtype=np.uint64)
        self._chk(self._L.mpfmt_points_free(self._h, _ip(idx), n, _up(mask)))
        return mask[:nwords(n)]

    def edges_free(self, src, dst):
        src = np.ascontiguousarray(src, dtype=np.int64)
        dst = np.ascontiguousarray(dst, dtype=np.int64)
        E = src.size
        mask = np.zeros(max(nwords(E), 1), dtype=np.uint64)
        self._chk(self._L.mpfmt_edges_free(self._h, _ip(src), _ip(dst), E, _up(mask)))
        return mask[:nwords(E)]

    def graph_edges_free(self):
        mask = np.zeros(max(nwords(self.nnz), 1), dtype=np.uint64)
        self._chk(self._L.mpfmt_graph_edges_free(self._h, _up(mask)))
        return mask[:nwords(self.nnz)]

    def states_free(self, P):
        P = np.ascontiguousarray(P, dtype=np.float64)
        n = P.shape[0]
        mask = np.zeros(max(nwords(n), 1), dtype=np.uint64)
        self._chk(self._L.mpfmt_states_free(self._h, _dp(P), n, _up(mask)))
        return mask[:nwords(n)]

    def motions_free(self, P, Q):
        P = np.ascontiguousarray(P, dtype=np.float64)
        Q = np.ascontiguousarray(Q, dtype=np.float64)
        n = P.shape[0]
        mask = np.zeros(max(nwords(n), 1), dtype=np.uint64)
        self._chk(self._L.mpfmt_motions_free(self._h, _dp(P), _dp(Q), n, _up(mask)))
        return mask[:nwords(n)]

    # ---- Euclidean steer (geometric.jl:18-19) -----------------------------------------------------
    def euclid_steer(self, src, dst):
        """steering_control per edge: (t = |w - v|, u = unit direction) for 1-based src -> dst."""
        src = np.ascontiguousarray(src, dtype=np.int64); dst = np.ascontiguousarray(dst, dtype=np.int64)
        E = src.size
        t = np.empty(max(E, 1)); u = np.empty((max(E, 1), self.d))
        self._chk(self._L.mpfmt_euclid_steer(self._h, _ip(src), _ip(dst), E, _dp(t), _dp(u)))
        return t[:E], u[:E]

    def euclid_propagate(self, src, t, u, s=None):
        """propagate(M, V[src], StepControl(t, u)[, s])."""
        src = np.ascontiguousarray(src, dtype=np.int64)
        t = np.ascontiguousarray(t, dtype=np.float64); u = np.ascontiguousarray(u, dtype=np.float64)
        s = None if s is None else np.ascontiguousarray(s, dtype=np.float64)
        E = src.size
        out = np.empty((max(E, 1), self.d))
        self._chk(self._L.mpfmt_euclid_propagate(self._h, _ip(src), E, _dp(t), _dp(u), _dp(s), _dp(out)))
        return out[:E]

    # ---- expand / solve ---------------------------------------------------------------------------
    def expand(self, W, H, F, Cc, zs, cap=None):
        W = np.ascontiguousarray(W, dtype=np.uint64)
        H = np.ascontiguousarray(H, dtype=np.uint64)
        F = None if F is None else np.ascontiguousarray(F, dtype=np.uint64)
        Cc = np.ascontiguousarray(Cc, dtype=np.float64)
        zs = np.ascontiguousarray(zs, dtype=np.int64)
        cap = self.N if cap is None else cap
        xs = np.empty(max(cap, 1), dtype=np.int64)
        ym = np.empty(max(cap, 1), dtype=np.int64)
        cm = np.empty(max(cap, 1), dtype=np.float64)
        fr = np.empty(max(cap, 1), dtype=np.uint8)
        nx = C.c_int64()
        self._chk(self._L.mpfmt_expand(self._h, _up(W), _up(H), _up(F), _dp(Cc), _ip(zs), zs.size, _ip(xs), _ip(ym),
                                       _dp(cm), fr.ctypes.data_as(c_u8_p), cap, C.byref(nx)))
        n = nx.value
        return xs[:n].copy(), ym[:n].copy(), cm[:n].copy(), fr[:n].astype(bool)

    def fmtstar(self, r, goal_kind, goal_params, init_idx=1, checkpts=True):
        return self._plan(self._L.mpfmt_fmtstar, (float(r),), goal_kind, goal_params, init_idx, checkpts)

    # ---- k-nearest connections (connections = :K, fmt.jl:6,17-19) -------------------------------
    def knn_graph(self, k):
        """(colptr, rowval, nzval, mutual_bits) of the exact k-nearest graph, 1-based CSC: column v = the min(k, N - 1) nearest samples
        of v under (d2, index), rows ascending; mutual bit of entry (y in column x) = x is among the nearest of y."""
        colptr = np.empty(self.N + 1, dtype=np.int64)
        nnz = C.c_int64()
        self._chk(self._L.mpfmt_knn_count(self._h, int(k), _ip(colptr), C.byref(nnz)))
        self.nnz = nnz = nnz.value
        rowval = np.empty(max(nnz, 1), dtype=np.int64)
        nzval = np.empty(max(nnz, 1), dtype=np.float64)
        mutual = np.zeros(max(nwords(nnz), 1), dtype=np.uint64)
        self._chk(self._L.mpfmt_knn_fill(self._h, _ip(rowval), _dp(nzval), _up(mutual)))
        return colptr, rowval[:nnz], nzval[:nnz], mutual[:nwords(nnz)]

    def knn_graph_edges_free(self):
        mask = np.zeros(max(nwords(self.nnz), 1), dtype=np.uint64)
        self._chk(self._L.mpfmt_knn_graph_edges_free(self._h, _up(mask)))
        return mask[:nwords(self.nnz)]

    def knn_fmtstar(self, k, goal_kind, goal_params, init_idx=1, checkpts=True):
        """fmtstar! with connections = :K: forward sets = mutual k-nearest, backward sets = k-nearest; same dict as fmtstar."""
        return self._plan(self._L.mpfmt_knn_fmtstar, (int(k),), goal_kind, goal_params, init_idx, checkpts)

    # ---- PRM* roadmap queries: shortest paths over the resident free-edge graph ------------------------------
    def graph_sssp(self, sources, checkpts=True, want_parents=True):
        """Cost-to-come fields over the resident graph and mask (graph_step_device, knn_graph + knn_graph_edges_free, or a steering graph
        and its sweep: di_graph / dubins_graph / reedsshepp_graph + *_graph_edges_free, or what a steering planner left) for the
        1-based `sources`: dict(C (nsrc, N), +Inf = unreached; A (nsrc, N) 1-based parents or None; info = one dict per source with
        reached, rounds, relaxations, ms_device)."""
        src = np.ascontiguousarray(np.atleast_1d(sources), dtype=np.int64)
        n = src.size
        Cc = np.empty((max(n, 1), max(self.N, 1)), dtype=np.float64)
        A = np.empty((max(n, 1), max(self.N, 1)), dtype=np.int64) if want_parents else None
        info = (SsspInfo * max(n, 1))()
        self._chk(self._L.mpfmt_graph_sssp(self._h, _ip(src), n, int(bool(checkpts)), _dp(Cc), _ip(A), info))
        return dict(C=Cc[:n, :self.N], A=None if A is None else A[:n, :self.N],
                    info=[{k: getattr(info[i], k) for k, _ in SsspInfo._fields_} for i in range(n)])

    def graph_sssp_multi(self, sources, checkpts=True, want_parents=True):
        """graph_sssp with up to 64 sources per pass over the graph (mpfmt_graph_sssp_multi), on the same resident graphs (Euclidean or
        steering): the same dict, C and A bit-identical;
        info[q]["rounds"], ["relaxations"] and ["ms_device"] are those of the source's group of 64."""
        src = np.ascontiguousarray(np.atleast_1d(sources), dtype=np.int64)
        n = src.size
        Cc = np.empty((max(n, 1), max(self.N, 1)), dtype=np.float64)
        A = np.empty((max(n, 1), max(self.N, 1)), dtype=np.int64) if want_parents else None
        info = (SsspInfo * max(n, 1))()
        self._chk(self._L.mpfmt_graph_sssp_multi(self._h, _ip(src), n, int(bool(checkpts)), _dp(Cc), _ip(A), info))
        return dict(C=Cc[:n, :self.N], A=None if A is None else A[:n, :self.N],
                    info=[{k: getattr(info[i], k) for k, _ in SsspInfo._fields_} for i in range(n)])

    def graph_sssp_to(self, targets, checkpts=True, want_successors=True):
        """The cost-to-go field of the 1-based `targets` over whatever swept graph is resident (r-disc, k-nearest, steering;
        mpfmt_graph_sssp_to): dict(G (N,), +Inf = no target reachable, 0 on the targets; S (N,) 1-based successors, 0 = target or
        unreached, None without want_successors; info = reached, rounds, relaxations, ms_device)."""
        tg = np.ascontiguousarray(np.atleast_1d(np.asarray(targets, dtype=np.int64)))
        G = np.empty(max(self.N, 1), dtype=np.float64)
        S = np.empty(max(self.N, 1), dtype=np.int64) if want_successors else None
        info = SsspInfo()
        self._chk(self._L.mpfmt_graph_sssp_to(self._h, _ip(tg) if tg.size else None, int(tg.size), int(bool(checkpts)), _dp(G), _ip(S),
                                              C.byref(info)))
        return dict(G=G[:self.N], S=None if S is None else S[:self.N], info={k: getattr(info, k) for k, _ in SsspInfo._fields_})

    # ---- a cost-to-come field kept valid across box edits (include/mpfmt.h) ---------------------------------------------------
    def field_begin(self, source=1, checkpts=True):
        """Compute the field of `source` (1-based) over the resident swept graph into buffers the context keeps (mpfmt_field_begin);
        returns the info dict (reached, invalidated, dirty_columns, columns_read, column_visits, entries_read, rounds, relaxations,
        ms_device, path)."""
        info = FieldInfo()
        self._chk(self._L.mpfmt_field_begin(self._h, int(source), int(bool(checkpts)), C.byref(info)))
        return _field_info(info)

    def field_update(self):
        """Repair the tracked field after boxes_add / boxes_remove (mpfmt_field_update): info["path"] = 1 repaired, 0 recomputed."""
        info = FieldInfo()
        self._chk(self._L.mpfmt_field_update(self._h, C.byref(info)))
        return _field_info(info)

    def field_read(self, want_parents=True):
        """Host copies (C, A) of the tracked field: C = +Inf for unreached samples, A 1-based parents (None without want_parents)."""
        Cc = np.empty(max(self.N, 1), dtype=np.float64)
        A = np.empty(max(self.N, 1), dtype=np.int64) if want_parents else None
        self._chk(self._L.mpfmt_field_read(self._h, _dp(Cc), _ip(A)))
        return Cc[:self.N], (None if A is None else A[:self.N])

    def field_goal(self, goal_kind, goal_params):
        """The goal extraction and walk-back of prmstar on the tracked field: dict(status, cost, z, collision_checks = 0, nnz,
        ms_host_loop, path)."""
        g = np.ascontiguousarray(goal_params, dtype=np.float64)
        path = np.empty(max(self.N, 1), dtype=np.int64)
        res = FmtResult()
        self._chk(self._L.mpfmt_field_goal(self._h, int(goal_kind), _dp(g), _ip(path), C.byref(res)))
        return dict(status=int(res.status), cost=float(res.cost), z=int(res.z), collision_checks=int(res.collision_checks),
                    nnz=int(res.nnz), ms_host_loop=res.ms_host_loop, path=path[:res.path_len].copy())

    def field_drop(self):
        self._chk(self._L.mpfmt_field_drop(self._h))

    @staticmethod
    def host_field_repair(colptr0, rowval0, nzval, efree, F, dirty, C_old, A_old, source=1):
        """The module's host_field_repair (no device)."""
        return host_field_repair(colptr0, rowval0, nzval, efree, F, dirty, C_old, A_old, source=source)

    # ---- a cost-to-go field kept valid across box edits, on any resident swept graph (include/mpfmt.h) -------------------------
    def togo_begin(self, targets, checkpts=True):
        """Compute the cost-to-go field of the 1-based `targets` over whatever swept graph is resident into buffers the context keeps
        (mpfmt_togo_begin); returns the info dict (reached, invalidated, dirty_columns, columns_read, column_visits, entries_read,
        rounds, relaxations, atomics, ms_device, path)."""
        tg = np.ascontiguousarray(np.atleast_1d(np.asarray(targets, dtype=np.int64)))
        info = TogoInfo()
        self._chk(self._L.mpfmt_togo_begin(self._h, _ip(tg) if tg.size else None, int(tg.size), int(bool(checkpts)), C.byref(info)))
        return _togo_info(info)

    def togo_update(self):
        """Repair the tracked cost-to-go field after boxes_add / boxes_remove (mpfmt_togo_update): info["path"] = 1 repaired,
        0 recomputed."""
        info = TogoInfo()
        self._chk(self._L.mpfmt_togo_update(self._h, C.byref(info)))
        return _togo_info(info)

    def togo_read(self, want_successors=True):
        """Host copies (G, S) of the tracked cost-to-go field: G = +Inf where no target is reachable, S 1-based successors, 0 for
        targets and unreached samples (None without want_successors)."""
        G = np.empty(max(self.N, 1), dtype=np.float64)
        S = np.empty(max(self.N, 1), dtype=np.int64) if want_successors else None
        self._chk(self._L.mpfmt_togo_read(self._h, _dp(G), _ip(S)))
        return G[:self.N], (None if S is None else S[:self.N])

    def togo_targets_add(self, targets):
        """Add 1-based `targets` to the tracked cost-to-go field (mpfmt_togo_targets_add): label decreases that the next togo_update
        pushes from, also while box edits or a carried growth are pending; the update then equals graph_sssp_to of the union.  An
        index outside 1..N raises ERR_ARG, no tracked field ERR_STATE; a refusal leaves the field untouched."""
        tg = np.ascontiguousarray(np.atleast_1d(np.asarray(targets, dtype=np.int64)))
        self._chk(self._L.mpfmt_togo_targets_add(self._h, _ip(tg) if tg.size else None, int(tg.size)))

    def togo_drop(self):
        self._chk(self._L.mpfmt_togo_drop(self._h))

    # ---- roadmap queries for states that are not samples (include/mpfmt.h, "roadmap queries for external states") ----------
    def _states(self, Q):
        Q = np.asarray(Q, dtype=np.float64)
        Q = np.ascontiguousarray(Q.reshape(0, self.d) if Q.size == 0 else np.atleast_2d(Q))
        if Q.ndim != 2 or (Q.shape[0] and Q.shape[1] != self.d):
            raise ValueError("states must be (n, %d)" % self.d)
        return Q

    def roadmap_near(self, Q, direction=0, cap=None):
        """Near lists of the external states Q (n, d) over the resident r-disc graph's radius: (ptr (n + 1,) 0-based, idx 1-based
        ascending, dist, free bits (bool)); direction 0 = tail (q -> sample), 1 = head (sample -> q).  cap: capacity in entries (None:
        ask, then fetch); too small raises MPFMTError(ERR_CAPACITY) whose .total holds the size needed."""
        return self._near(self._L.mpfmt_roadmap_near, Q, direction, cap)

    def _near(self, fn, Q, direction, cap):
        Q = self._states(Q)
        n = Q.shape[0]
        ptr = np.zeros(n + 1, dtype=np.int64)
        total = C.c_int64(0)
        ask = cap is None
        cap = 0 if ask else int(cap)
        while True:
            idx = np.empty(max(cap, 1), dtype=np.int64); dist = np.empty(max(cap, 1), dtype=np.float64)
            mask = np.zeros(max(nwords(cap), 1), dtype=np.uint64)
            rc = fn(self._h, _dp(Q), n, int(direction), _ip(ptr), cap, _ip(idx), _dp(dist), _up(mask), C.byref(total))
            if rc == ERR_CAPACITY and ask:
                cap, ask = int(total.value), False
                continue
            if rc == ERR_CAPACITY:
                e = MPFMTError(rc, self._L.mpfmt_last_error(self._h).decode())
                e.total, e.ptr = int(total.value), ptr
                raise e
            self._chk(rc)
            t = int(total.value)
            return ptr, idx[:t].copy(), dist[:t].copy(), unpack_bits(mask, t)

    def roadmap_attach(self, Q, Cfield):
        """The goal half for many goals over ONE field (a row of graph_sssp): per state of Q (n, d) the head-direction minimum
        fl(C[y] + d(y, q)) over the free near samples -> (cost (n,), +Inf = none; parent (n,) 1-based, 0 = none)."""
        return self._attach(self._L.mpfmt_roadmap_attach, Q, Cfield)

    def _attach(self, fn, Q, Cfield):
        Q = self._states(Q)
        n = Q.shape[0]
        Cf = np.ascontiguousarray(Cfield, dtype=np.float64)
        if Cf.shape != (self.N,):
            raise ValueError("C must have N entries")
        cost = np.empty(max(n, 1), dtype=np.float64); par = np.empty(max(n, 1), dtype=np.int64)
        self._chk(fn(self._h, _dp(Q), n, _dp(Cf), _ip(par), _dp(cost)))
        return cost[:n], par[:n]

    def roadmap_query(self, S, G, checkpts=True):
        """Pair queries between external states S[i] -> G[i] ((n, d) each) over the resident roadmap: (cost (n,), paths = list of 1-based
        sample index arrays between s and g, info = list of dicts: status 0 solved / 1 no path / 2 start blocked / 3 goal blocked,
        near_s, usable_s, near_g, usable_g, rounds, path_len, ms_device)."""
        return self._query(self._L.mpfmt_roadmap_query, S, G, checkpts)

    def _query(self, fn, S, G, checkpts):
        S = self._states(S); G = self._states(G)
        if S.shape != G.shape:
            raise ValueError("S and G must have the same shape")
        n = S.shape[0]
        cost = np.empty(max(n, 1), dtype=np.float64)
        pptr = np.zeros(n + 1, dtype=np.int64)
        info = (RoadmapInfo * max(n, 1))()
        cap = max(64 * n, 1)
        while True:
            path = np.empty(cap, dtype=np.int64)
            rc = fn(self._h, _dp(S), _dp(G), n, int(bool(checkpts)), _dp(cost), _ip(pptr), _ip(path), cap, info)
            if rc == ERR_CAPACITY and int(pptr[n]) > cap:
                cap = int(pptr[n])
                continue
            self._chk(rc)
            break
        return (cost[:n], [path[pptr[i]:pptr[i + 1]].copy() for i in range(n)], [_roadmap_info(info[i]) for i in range(n)])

    # the same three calls on a resident steering graph (include/mpfmt.h, "roadmap queries for external states, steering spaces"): the
    # resident graph's own space parameters are used; shapes and return values are those of the Euclidean namesakes
    def steer_roadmap_near(self, Q, direction=0, cap=None):
        """roadmap_near over the resident double-integrator / Dubins / Reeds-Shepp graph: the entries q would have had as a sample (dist =
        the steering cost in the build's direction, free bits = the sweep's motion test)."""
        return self._near(self._L.mpfmt_steer_roadmap_near, Q, direction, cap)

    def steer_roadmap_attach(self, Q, Cfield):
        """roadmap_attach over the resident steering graph: per state the head-direction minimum fl(C[y] + w(y, q)) over its free entries."""
        return self._attach(self._L.mpfmt_steer_roadmap_attach, Q, Cfield)

    def steer_roadmap_query(self, S, G, checkpts=True):
        """roadmap_query over the resident steering graph: (cost, paths, info) for the pairs S[i] -> G[i], states that are not samples."""
        return self._query(self._L.mpfmt_steer_roadmap_query, S, G, checkpts)

    def roadmap_matrix(self, S, G, checkpts=True):
        """The cost matrix between external starts S (ns, d) and goals G (ng, d) at the price of ns fields, 64 per pass over the graph
        (mpfmt_roadmap_matrix): (cost (ns, ng), status (ns, ng) int32, info dict).  Every cell equals roadmap_query on that pair (cost
        bits and status 0 solved / 1 no path / 2 start blocked / 3 goal blocked); no paths: ask roadmap_query for a chosen cell."""
        S = self._states(S); G = self._states(G)
        ns, ng = S.shape[0], G.shape[0]
        cost = np.empty(max(ns * ng, 1), dtype=np.float64)
        status = np.empty(max(ns * ng, 1), dtype=np.int32)
        info = RoadmapMatrixInfo()
        self._chk(self._L.mpfmt_roadmap_matrix(self._h, _dp(S), ns, _dp(G), ng, int(bool(checkpts)), _dp(cost),
                                               status.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(info)))
        return (cost[:ns * ng].reshape(ns, ng), status[:ns * ng].reshape(ns, ng),
                {k: getattr(info, k) for k, _ in RoadmapMatrixInfo._fields_})

    def prmstar(self, r, goal_kind, goal_params, init_idx=1, checkpts=True):
        """PRM*: graph_step_device(r) (reused when resident), then the exact cost-to-come field of init_idx over the free-edge graph and
        the best goal sample; same dict as fmtstar, with C = +Inf for unreached samples."""
        return self._plan(self._L.mpfmt_prmstar, (float(r),), goal_kind, goal_params, init_idx, checkpts, set_nnz=True)

    def knn_prmstar(self, k, goal_kind, goal_params, init_idx=1, checkpts=True):
        """prmstar over the (directed) k-nearest graph."""
        return self._plan(self._L.mpfmt_knn_prmstar, (int(k),), goal_kind, goal_params, init_idx, checkpts, set_nnz=True)

    def _plan(self, fn, lead, goal_kind, goal_params, init_idx, checkpts, wavefront=None, want_tree=True, set_nnz=False):
        """One single-shot planner call: fn(ctx, *lead, init_idx, checkpts, goal_kind, goal_params[, band, flags], A, C, path, res[, info]).
        lead = the space's scalars (r | k | the steering parameters); wavefront = (band, flags) for the forms with the recursion on the
        device, which also return their counters and may go without the tree; set_nnz: the roadmap planners leave their graph resident
        and self.nnz says so."""
        g = np.ascontiguousarray(goal_params, dtype=np.float64)
        A, Cc, path = self._fmt_arrays(want_tree)
        res, info = FmtResult(), WfInfo()
        args = [self._h, *lead, int(init_idx), int(bool(checkpts)), int(goal_kind), _dp(g)]
        if wavefront is not None:
            args += [float(wavefront[0]), int(wavefront[1])]
        args += [_ip(A), _dp(Cc), _ip(path), C.byref(res)] + ([C.byref(info)] if wavefront is not None else [])
        self._chk(fn(*args))
        if set_nnz:
            self.nnz = int(res.nnz)
        return self._fmt_out(res, A, Cc, path) if wavefront is None else self._wf_out(res, info, A, Cc, path)

    def _fmt_arrays(self, want_tree=True):
        """The output arrays of a plan: parents A and costs C (None without the tree) and the path."""
        A = np.empty(max(self.N, 1), dtype=np.int64) if want_tree else None
        Cc = np.empty(max(self.N, 1), dtype=np.float64) if want_tree else None
        return A, Cc, np.empty(max(self.N, 1), dtype=np.int64)

    def _fmt_out(self, res, A, Cc, path):
        return dict(status=int(res.status), cost=float(res.cost), z=int(res.z), collision_checks=int(res.collision_checks),
                    nnz=int(res.nnz), ms_graph=res.ms_graph, ms_sweep=res.ms_sweep, ms_host_loop=res.ms_host_loop,
                    A=None if A is None else A[:self.N], C=None if Cc is None else Cc[:self.N], path=path[:res.path_len].copy())

    # ---- wavefront solve (recursion on the device) -------------------------------------------------
    @staticmethod
    def _wf_info(i):
        return {k: getattr(i, k) for k, _ in WfInfo._fields_}

    def _wf_out(self, res, info, A, Cc, path):
        out = self._fmt_out(res, A, Cc, path)
        out["info"] = self._wf_info(info)
        return out

    def fmtstar_wavefront(self, r, goal_kind, goal_params, band=0.0, single=False, eager=False, lazy=False, init_idx=1, checkpts=True,
                          want_tree=True):
        """fmtstar! with the recursion on the device (include/mpfmt.h): band = cost width of a batch; single = one node per
        step (the reference's order exactly)."""
        flags = (WF_SINGLE if single else 0) | (WF_EAGER if eager else 0) | (WF_LAZY if lazy else 0)
        return self._plan(self._L.mpfmt_fmtstar_wavefront, (float(r),), goal_kind, goal_params, init_idx, checkpts, wavefront=(band, flags),
                          want_tree=want_tree)

    def wf_begin(self, r, goal_kind, goal_params, band=0.0, single=False, eager=False, init_idx=1, checkpts=True, lazy=False):
        g = np.ascontiguousarray(goal_params, dtype=np.float64)
        flags = (WF_SINGLE if single else 0) | (WF_EAGER if eager else 0) | (WF_LAZY if lazy else 0)
        self._chk(self._L.mpfmt_wf_begin(self._h, float(r), int(init_idx), int(bool(checkpts)), int(goal_kind), _dp(g), float(band), flags))

    def wf_step(self):
        info = WfInfo()
        self._chk(self._L.mpfmt_wf_step(self._h, C.byref(info)))
        return self._wf_info(info)

    def wf_state(self):
        """(W, H, C, A): packed uint64 masks, costs, parents (1-based, 0 = none)."""
        nw = max(nwords(self.N), 1)
        W = np.zeros(nw, dtype=np.uint64); H = np.zeros(nw, dtype=np.uint64)
        Cc = np.empty(max(self.N, 1)); A = np.empty(max(self.N, 1), dtype=np.int64)
        self._chk(self._L.mpfmt_wf_state(self._h, _up(W), _up(H), _dp(Cc), _ip(A)))
        return W[:nwords(self.N)], H[:nwords(self.N)], Cc[:self.N], A[:self.N]

    def wf_batch(self):
        zs = np.empty(max(self.N, 1), dtype=np.int64)
        n = C.c_int64()
        self._chk(self._L.mpfmt_wf_batch(self._h, _ip(zs), self.N, C.byref(n)))
        return zs[:n.value].copy()

    def wf_triples(self):
        x = np.empty(max(self.N, 1), dtype=np.int64); y = np.empty(max(self.N, 1), dtype=np.int64); c = np.empty(max(self.N, 1))
        n = C.c_int64()
        self._chk(self._L.mpfmt_wf_triples(self._h, self.N, _ip(x), _ip(y), _dp(c), C.byref(n)))
        return x[:n.value].copy(), y[:n.value].copy(), c[:n.value].copy()

    def wf_commit(self, x, y, c):
        x = np.ascontiguousarray(x, dtype=np.int64); y = np.ascontiguousarray(y, dtype=np.int64); c = np.ascontiguousarray(c, dtype=np.float64)
        self._chk(self._L.mpfmt_wf_commit(self._h, len(x), _ip(x), _ip(y), _dp(c)))

    def wf_finish(self, want_tree=True):
        A, Cc, path = self._fmt_arrays(want_tree)
        res = FmtResult()
        self._chk(self._L.mpfmt_wf_finish(self._h, _ip(A), _dp(Cc), _ip(path), C.byref(res)))
        return self._fmt_out(res, A, Cc, path)

    # ---- multi-GPU exchange (RCCL behind the ABI) ---------------------------------------------------
    def comm_create(self, rank, world, uid):
        """uid: 128 bytes from comm_unique_id() of rank 0, handed to every rank by the host."""
        u = np.frombuffer(bytes(uid), dtype=np.uint8).copy()
        assert u.size == COMM_ID_BYTES
        self._chk(self._L.mpfmt_comm_create(self._h, int(rank), int(world), u.ctypes.data_as(c_u8_p)))

    def comm_destroy(self):
        self._chk(self._L.mpfmt_comm_destroy(self._h))

    def allgather_free_mask_launch(self, cap_hint=0):
        self._chk(self._L.mpfmt_allgather_free_mask_launch(self._h, int(cap_hint)))

    def allgather_free_mask_finish(self, world, allow_retry=False):
        """(device ptr, stride in words, words per rank, nnz per rank); with allow_retry (single-thread drivers of several ctxs)
        None when the library asks for a relaunch of every ctx (MPFMT_RETRY)."""
        ptr, stride = C.c_void_p(), C.c_int64()
        words = np.zeros(world, dtype=np.int64); nnz = np.zeros(world, dtype=np.int64)
        rc = self._L.mpfmt_allgather_free_mask_finish(self._h, C.byref(ptr), C.byref(stride), _ip(words), _ip(nnz))
        if rc == RETRY and allow_retry:
            return None
        self._chk(rc)
        return ptr.value, stride.value, words, nnz

    def allgather_free_mask_relaunch(self):
        self._chk(self._L.mpfmt_allgather_free_mask_relaunch(self._h))

    def allgather_free_mask(self, world):
        """One RCCL all-gather of the per-shard free-edge masks: (device ptr, stride in words, words per rank, nnz per rank)."""
        self.allgather_free_mask_launch(0)
        return self.allgather_free_mask_finish(world)

    def mc_edges_collision(self, src, dst, sigma, rollouts, seed=0):
        """Colliding rollouts per edge (1-based src / dst): Monte-Carlo collision probability = hits / rollouts."""
        src = np.ascontiguousarray(src, dtype=np.int64); dst = np.ascontiguousarray(dst, dtype=np.int64)
        hits = np.zeros(max(len(src), 1), dtype=np.int64)
        self._chk(self._L.mpfmt_mc_edges_collision(self._h, _ip(src), _ip(dst), len(src), float(sigma), int(rollouts), int(seed), _ip(hits)))
        return hits[:len(src)]

    def mc_edges_collision_is(self, src, dst, sigma, rollouts, seed=0):
        """Importance-sampling estimate of the collision probability per edge (1-based src / dst): (probabilities, raw uint64 sums of
        the colliding rollouts' weights at 2^-40 -- what the scalar loop reproduces exactly)."""
        src = np.ascontiguousarray(src, dtype=np.int64); dst = np.ascontiguousarray(dst, dtype=np.int64)
        wsum = np.zeros(max(len(src), 1), dtype=np.uint64)
        self._chk(self._L.mpfmt_mc_edges_collision_is(self._h, _ip(src), _ip(dst), len(src), float(sigma), int(rollouts), int(seed),
                                                      wsum.ctypes.data_as(C.POINTER(C.c_uint64))))
        wsum = wsum[:len(src)]
        return wsum.astype(np.float64) / (2.0 ** 40) / max(int(rollouts), 1), wsum

    def mc_edges_collision_ais(self, src, dst, sigma, rollouts, seed=0):
        """ADAPTIVE importance sampling (pilot -> cross-entropy mean shift -> mixture): (probabilities, raw uint64 weight sums at 2^-40,
        shifts (E, 2 d) in noise units)."""
        src = np.ascontiguousarray(src, dtype=np.int64); dst = np.ascontiguousarray(dst, dtype=np.int64)
        wsum = np.zeros(max(len(src), 1), dtype=np.uint64)
        sh = np.zeros((max(len(src), 1), 2 * self.d))
        self._chk(self._L.mpfmt_mc_edges_collision_ais(self._h, _ip(src), _ip(dst), len(src), float(sigma), int(rollouts), int(seed),
                                                       wsum.ctypes.data_as(C.POINTER(C.c_uint64)), _dp(sh)))
        wsum = wsum[:len(src)]
        return wsum.astype(np.float64) / (2.0 ** 40) / max(int(rollouts), 1), wsum, sh[:len(src)]

    # ---- steering spaces: double integrator (space "di", params (rho, r)), Dubins and Reeds-Shepp cars (turn_radius, speed, r) ----
    def _steer_graph(self, space, params, tval=False):
        """(colptr, rowval, nzval[, tval]), CSC 1-based."""
        colptr = np.empty(self.N + 1, dtype=np.int64)
        nnz = C.c_int64()
        self._chk(getattr(self._L, f"mpfmt_{space}_graph_count")(self._h, *map(float, params), _ip(colptr), C.byref(nnz)))
        self.nnz = n = nnz.value
        rowval = np.empty(max(n, 1), dtype=np.int64)
        vals = [np.empty(max(n, 1), dtype=np.float64) for _ in range(2 if tval else 1)]
        self._chk(getattr(self._L, f"mpfmt_{space}_graph_fill")(self._h, _ip(rowval), *map(_dp, vals)))
        return (colptr, rowval[:n]) + tuple(v[:n] for v in vals)

    def _steer_graph_edges_free(self, space):
        n = self.nnz
        mask = np.zeros(max(nwords(n), 1), dtype=np.uint64)
        nseg = np.zeros(max(n, 1), dtype=np.uint8)
        self._chk(getattr(self._L, f"mpfmt_{space}_graph_edges_free")(self._h, _up(mask), nseg.ctypes.data_as(c_u8_p)))
        return mask[:nwords(n)], nseg[:n]

    def _steer_plan(self, space, solver, params, goal_kind, goal_params, init_idx, checkpts, **kw):
        """_plan for mpfmt_{space}_{solver}: solver = fmtstar | prmstar | fmtstar_wavefront, params = the steering parameters."""
        return self._plan(getattr(self._L, f"mpfmt_{space}_{solver}"), map(float, params), goal_kind, goal_params, init_idx, checkpts,
                          set_nnz=solver == "prmstar", **kw)

    def dubins_graph(self, turn_radius, speed, r):
        """Chopped backward sets of the Dubins quasi-metric, CSC 1-based: (colptr, rowval, nzval)."""
        return self._steer_graph("dubins", (turn_radius, speed, r))

    def dubins_graph_edges_free(self):
        return self._steer_graph_edges_free("dubins")

    def dubins_steer(self, X0, X1, turn_radius, speed=1.0):
        X0 = np.ascontiguousarray(X0, dtype=np.float64); X1 = np.ascontiguousarray(X1, dtype=np.float64)
        n = len(X0)
        cost = np.empty(max(n, 1)); ctrl = np.empty((max(n, 1), 3, 3))
        self._chk(self._L.mpfmt_dubins_steer(self._h, _dp(X0), _dp(X1), n, float(turn_radius), float(speed), _dp(cost), _dp(ctrl)))
        return cost[:n], ctrl[:n]

    def dubins_fmtstar(self, turn_radius, speed, r, goal_kind, goal_params, init_idx=1, checkpts=True):
        return self._steer_plan("dubins", "fmtstar", (turn_radius, speed, r), goal_kind, goal_params, init_idx, checkpts)

    def reedsshepp_graph(self, turn_radius, speed, r):
        """Chopped Reeds-Shepp neighbourhoods, CSC 1-based: column v = rows w with nzval = reedsshepp(v, w)."""
        return self._steer_graph("reedsshepp", (turn_radius, speed, r))

    def reedsshepp_graph_edges_free(self):
        return self._steer_graph_edges_free("reedsshepp")

    def reedsshepp_steer(self, X0, X1, turn_radius, speed=1.0):
        """(cost, controls (n,5,3), nsegs)."""
        X0 = np.ascontiguousarray(X0, dtype=np.float64); X1 = np.ascontiguousarray(X1, dtype=np.float64)
        n = len(X0)
        cost = np.empty(max(n, 1)); ctrl = np.empty((max(n, 1), 5, 3)); nsegs = np.zeros(max(n, 1), dtype=np.int32)
        self._chk(self._L.mpfmt_reedsshepp_steer(self._h, _dp(X0), _dp(X1), n, float(turn_radius), float(speed), _dp(cost), _dp(ctrl),
                                                 nsegs.ctypes.data_as(C.POINTER(C.c_int32))))
        return cost[:n], ctrl[:n], nsegs[:n]

    def reedsshepp_fmtstar(self, turn_radius, speed, r, goal_kind, goal_params, init_idx=1, checkpts=True):
        return self._steer_plan("reedsshepp", "fmtstar", (turn_radius, speed, r), goal_kind, goal_params, init_idx, checkpts)

    # ---- closest obstacle points ----------------------------------------------------------------
    def closest(self, P, W=None):
        """closest(p, CC, W) per row of P: (d2min, vmin, kmin 1-based / 0, failures)."""
        P = np.ascontiguousarray(np.atleast_2d(P), dtype=np.float64)
        n, d = P.shape
        Wp = None if W is None else _dp(np.ascontiguousarray(W, dtype=np.float64).reshape(d, d))
        d2 = np.empty(max(n, 1)); v = np.empty((max(n, 1), d)); k = np.empty(max(n, 1), dtype=np.int64)
        fails = C.c_int64()
        self._chk(self._L.mpfmt_closest(self._h, _dp(P), n, Wp, _dp(d2), _dp(v), _ip(k), C.byref(fails)))
        return d2[:n], v[:n], k[:n], fails.value

    def closeR(self, P, W, r2):
        """closeR(p, CC, W, r2) per row of P: (ptr 1-based, obstacle 1-based, d2, v, failures)."""
        P = np.ascontiguousarray(np.atleast_2d(P), dtype=np.float64)
        n, d = P.shape
        Wa = np.ascontiguousarray(W, dtype=np.float64).reshape(d, d)
        ptr = np.empty(n + 1, dtype=np.int64)
        total = C.c_int64(); fails = C.c_int64()
        cap = max(4 * n, 1024)
        while True:
            idx = np.empty(cap, dtype=np.int64); d2 = np.empty(cap); v = np.empty((cap, d))
            rc = self._L.mpfmt_closeR(self._h, _dp(P), n, _dp(Wa), float(r2), _ip(ptr), cap, _ip(idx), _dp(d2), _dp(v),
                                      C.byref(total), C.byref(fails))
            if rc == ERR_CAPACITY:
                cap = total.value
                continue
            self._chk(rc)
            t = total.value
            return ptr, idx[:t], d2[:t], v[:t], fails.value

    def graph_import(self, r, colptr, rowval, nzval):
        """Install an exported graph (1-based CSC as returned by rdisc_graph) for the uploaded samples."""
        colptr = np.ascontiguousarray(colptr, dtype=np.int64)
        rowval = np.ascontiguousarray(rowval, dtype=np.int64)
        nzval = np.ascontiguousarray(nzval, dtype=np.float64)
        self._chk(self._L.mpfmt_graph_import(self._h, float(r), _ip(colptr), _ip(rowval), _dp(nzval)))
        self.nnz = int(colptr[-1] - 1)

    def adaptive_shortcut(self, paths, iterations=10, max_states=256):
        """adaptive_shortcut (src/postprocessors.jl:28-39) of a batch of paths under the resident checker, one wavefront per path
        (include/mpfmt.h, "adaptive shortcutting").  paths: a list of (n_i, d) arrays -> a list of (path, cumcost, info) triples; one
        (n, d) array -> one triple."""
        single = isinstance(paths, np.ndarray) and paths.ndim == 2
        plist = [paths] if single else list(paths)
        plist = [np.ascontiguousarray(p, dtype=np.float64) for p in plist]
        for p in plist:
            if p.ndim != 2:
                raise ValueError("every path must be (n, d)")
        B = len(plist)
        d = plist[0].shape[1] if B else max(self.dw, 1)
        for p in plist:
            if p.shape[1] != d:
                raise ValueError("paths of different dimensions")
        off = np.zeros(B + 1, dtype=np.int64)
        off[1:] = np.cumsum([p.shape[0] for p in plist])
        P = np.ascontiguousarray(np.concatenate(plist, axis=0)) if B else np.zeros((1, d))
        if B and self.dw and d != self.dw:
            raise ValueError("paths have dimension %d, the checker's workspace %d" % (d, self.dw))
        info = (ShortcutInfo * max(B, 1))()
        out_off = np.zeros(B + 1, dtype=np.int64)
        if single:
            cap = max(int(max_states), 2)
            out = np.empty((cap, d), dtype=np.float64); cc = np.empty(cap, dtype=np.float64)
            self._chk(self._L.mpfmt_adaptive_shortcut(self._h, _dp(P), P.shape[0], int(iterations), int(max_states), _dp(out), cap, _dp(cc), info))
            n = int(info[0].n_out)
            return out[:n].copy(), cc[:n].copy(), _shortcut_info(info[0])
        cap = max(int(off[-1]), 1)                       # most outputs are shorter than their inputs; grow once when they are not
        for _ in range(2):
            out = np.empty((cap, d), dtype=np.float64); cc = np.empty(cap, dtype=np.float64)
            rc = self._L.mpfmt_adaptive_shortcut_batch(self._h, _dp(P), _ip(off), B, int(iterations), int(max_states), _dp(out), _ip(out_off), cap,
                                                       _dp(cc), info)
            if rc == ERR_CAPACITY and int(out_off[-1]) > cap:
                cap = int(out_off[-1])
                continue
            self._chk(rc)
            break
        return [(out[out_off[b]:out_off[b + 1]].copy(), cc[out_off[b]:out_off[b + 1]].copy(), _shortcut_info(info[b])) for b in range(B)]

    def steer_motions_free(self, space, params, P, Q):
        """The steered motions P[e] -> Q[e] under the resident checker (include/mpfmt.h, "steering shortcut"): (bits (n,) bool, cost (n,),
        dur (n,), nseg (n,) int32).  space: SPACE_DI / _DUBINS / _REEDSSHEPP; params: (rho, tmax) or (turn_radius, speed).  The bit is
        is_free_motion exactly as the space's graph sweep computes it; no samples and no graph are needed."""
        P = np.ascontiguousarray(P, dtype=np.float64); Q = np.ascontiguousarray(Q, dtype=np.float64)
        if P.ndim != 2 or P.shape != Q.shape:
            raise ValueError("P and Q must both be (n, d)")
        prm = _steer_params(space, params)
        n, d = P.shape
        mask = np.zeros(max(nwords(n), 1), dtype=np.uint64)
        cost = np.empty(max(n, 1)); dur = np.empty(max(n, 1)); nseg = np.zeros(max(n, 1), dtype=np.int32)
        self._chk(self._L.mpfmt_steer_motions_free(self._h, int(space), d, _dp(prm), _dp(P), _dp(Q), n, _up(mask), _dp(cost), _dp(dur), _ip32(nseg)))
        return unpack_bits(mask, n), cost[:n], dur[:n], nseg[:n]

    def steer_shortcut(self, paths, space, params, iterations=4, max_states=256):
        """Shortcut of a batch of paths in a steering space under the resident checker, one wavefront per path (include/mpfmt.h,
        "steering shortcut").  paths: a list of (n_i, d) arrays -> a list of (path, cumcost, origin, info) tuples; one (n, d) array -> one
        tuple.  origin: the 1-based input index of every output state, 0 for an inserted one."""
        single = isinstance(paths, np.ndarray) and paths.ndim == 2
        plist = [np.ascontiguousarray(p, dtype=np.float64) for p in ([paths] if single else list(paths))]
        for p in plist:
            if p.ndim != 2 or p.shape[1] != plist[0].shape[1]:
                raise ValueError("every path must be (n, d) with one d")
        prm = _steer_params(space, params)
        B = len(plist)
        if B == 0:
            return []
        d = plist[0].shape[1]
        if single:
            P = plist[0]
            cap = max(int(max_states), 2)
            info = SteerShortcutInfo()
            out = np.empty((cap, d)); cc = np.empty(cap); org = np.zeros(cap, dtype=np.int32)
            self._chk(self._L.mpfmt_steer_shortcut(self._h, int(space), d, _dp(prm), _dp(P), P.shape[0], int(iterations), int(max_states), _dp(out),
                                                   cap, _dp(cc), _ip32(org), C.byref(info)))
            n = int(info.n_out)
            return out[:n].copy(), cc[:n].copy(), org[:n].copy(), _steer_shortcut_info(info)
        off = np.zeros(B + 1, dtype=np.int64)
        off[1:] = np.cumsum([p.shape[0] for p in plist])
        P = np.ascontiguousarray(np.concatenate(plist, axis=0))
        info = (SteerShortcutInfo * B)()
        out_off = np.zeros(B + 1, dtype=np.int64)
        cap = max(int(off[-1]), 1)                       # most outputs are shorter than their inputs; grow once when they are not
        for _ in range(2):
            out = np.empty((cap, d)); cc = np.empty(cap); org = np.zeros(cap, dtype=np.int32)
            rc = self._L.mpfmt_steer_shortcut_batch(self._h, int(space), d, _dp(prm), _dp(P), _ip(off), B, int(iterations), int(max_states),
                                                    _dp(out), _ip(out_off), cap, _dp(cc), _ip32(org), info)
            if rc == ERR_CAPACITY and int(out_off[-1]) > cap:
                cap = int(out_off[-1])
                continue
            self._chk(rc)
            break
        return [(out[out_off[b]:out_off[b + 1]].copy(), cc[out_off[b]:out_off[b + 1]].copy(), org[out_off[b]:out_off[b + 1]].copy(),
                 _steer_shortcut_info(info[b])) for b in range(B)]

    def discretize(self, paths, space, params=None, dt=None, n=None, append_end=False):
        """Time discretisation of a batch of paths on the device, lane = output sample (include/mpfmt.h, "time discretisation"):
        time_discretize_solution! with dt, time_space_solution! with n.  space: SPACE_EUCLID / _DI / _DUBINS / _REEDSSHEPP; params: None,
        (rho, r) or (turn_radius, speed).  paths: a list of (n_i, d) arrays -> (a list of (X, T, seg) triples, a list of info dicts); one
        (n, d) array -> ((X, T, seg), info).  Needs nothing resident on the ctx and leaves it as it was."""
        single = isinstance(paths, np.ndarray) and paths.ndim == 2
        plist = [np.ascontiguousarray(p, dtype=np.float64) for p in ([paths] if single else list(paths))]
        for p in plist:
            if p.ndim != 2 or p.shape[1] != plist[0].shape[1]:
                raise ValueError("every path must be (n, d) with one d")
        prm, mode, dtv, ns, app = _disc_args(space, params, dt, n, append_end)
        B = len(plist)
        if B == 0:
            return [], []
        d = plist[0].shape[1]
        off = np.zeros(B + 1, dtype=np.int64)
        off[1:] = np.cumsum([p.shape[0] for p in plist])
        P = np.ascontiguousarray(np.concatenate(plist, axis=0))
        info = (DiscInfo * B)()
        out_off = np.zeros(B + 1, dtype=np.int64)
        self._chk(self._L.mpfmt_discretize_batch(self._h, int(space), d, _dp(prm), _dp(P), _ip(off), B, mode, dtv, ns, app, None, None, None,
                                                 _ip(out_off), 0, info))                   # the size query
        cap = max(int(out_off[-1]), 1)
        X = np.empty((cap, d), dtype=np.float64); T = np.empty(cap, dtype=np.float64); seg = np.empty(cap, dtype=np.int32)
        self._chk(self._L.mpfmt_discretize_batch(self._h, int(space), d, _dp(prm), _dp(P), _ip(off), B, mode, dtv, ns, app, _dp(X), _dp(T),
                                                 _ip32(seg), _ip(out_off), cap, info))
        res = [(X[out_off[b]:out_off[b + 1]].copy(), T[out_off[b]:out_off[b + 1]].copy(), seg[out_off[b]:out_off[b + 1]].copy()) for b in range(B)]
        infos = [_disc_info(info[b]) for b in range(B)]
        return (res[0], infos[0]) if single else (res, infos)

    def path_free(self, P):
        """is_free_path(p, CC, SS) for the states P (n, d): (free, per-segment bits)."""
        P = np.ascontiguousarray(P, dtype=np.float64)
        n = P.shape[0]
        fr = C.c_int32()
        mask = np.zeros(max(nwords(max(n - 1, 0)), 1), dtype=np.uint64)
        self._chk(self._L.mpfmt_path_free(self._h, _dp(P), n, C.byref(fr), _up(mask)))
        return bool(fr.value), unpack_bits(mask, max(n - 1, 0))

    def sample_free(self, seed, N, init=None, goal_kind=0, goal_params=None, goal_ct=0, goal_bias=0.0):
        """sample_free!(P, N): N free samples drawn on the device (counter-based stream, sequential semantics), left
        uploaded in the context.  Returns (X, attempts)."""
        d = self.dw
        X = np.empty((max(int(N), 1), d), dtype=np.float64)
        att = C.c_int64()
        ini = None if init is None else np.ascontiguousarray(init, dtype=np.float64)
        g = None if goal_params is None else np.ascontiguousarray(goal_params, dtype=np.float64)
        self._chk(self._L.mpfmt_sample_free_biased(self._h, int(seed), int(N), None if ini is None else _dp(ini), int(goal_kind),
                                                   None if g is None else _dp(g), int(goal_ct), float(goal_bias), _dp(X), C.byref(att)))
        self.N, self.d = int(N), d
        return X[:N], int(att.value)

    # ---- double integrator ------------------------------------------------------------------------
    def di_graph(self, rho, r):
        """Sparse cost matrix of the double-integrator space, CSC 1-based: (colptr, rowval, nzval, tval)."""
        return self._steer_graph("di", (rho, r), tval=True)

    def di_graph_edges_free(self):
        return self._steer_graph_edges_free("di")

    def di_graph_step_device(self, rho, r):
        """Double-integrator graph + 5-waypoint edge bits, outputs left in HBM (see include/mpfmt.h).  Returns nnz."""
        nnz = C.c_int64()
        self._chk(self._L.mpfmt_di_graph_step_device(self._h, float(rho), float(r), C.byref(nnz)))
        self.nnz = nnz.value
        return nnz.value

    def di_graph_device_ptrs(self):
        """(colptr, rowval, nzval, tval, free_mask, nseg) device addresses of the resident double-integrator graph."""
        p = [C.c_void_p() for _ in range(6)]
        self._chk(self._L.mpfmt_di_graph_device_ptrs(self._h, *[C.byref(x) for x in p]))
        return tuple(x.value for x in p)

    def di_steer(self, X0, X1, rho, r):
        X0 = np.ascontiguousarray(X0, dtype=np.float64)
        X1 = np.ascontiguousarray(X1, dtype=np.float64)
        n, ns = X0.shape
        cost = np.empty(max(n, 1)); t = np.empty(max(n, 1))
        self._chk(self._L.mpfmt_di_steer(self._h, _dp(X0), _dp(X1), n, ns // 2, float(rho), float(r), _dp(cost), _dp(t)))
        return cost[:n], t[:n]

    def di_mf_probe(self, rho, r):
        """DIAGNOSTIC (mpfmt_di_mf_probe, tests only): what the matrix-core candidate test of the double-integrator build computes on the
        resident samples (64 <= N <= 1024).  Returns a dict: `acc` float32 [npad, npad] (row = target, column = source: Q - T as the
        matrix core delivered it), `opsT` / `opsS` float16 [npad, 16] (the operands of the target / source role) and the threshold's
        terms sp, sv, pc, split, accum, E, T, negT, usable, Pm, Vm, F, G, N0, guards.  Drops a resident steering graph."""
        npad = ((self.N + 63) // 64) * 64 if 64 <= self.N <= 1024 else 64          # (outside that range the library refuses before it writes)
        acc = np.zeros((npad, npad), np.float32); oT = np.zeros((npad, 16), np.uint16); oS = np.zeros((npad, 16), np.uint16)
        terms = np.zeros(DI_MF_PROBE_TERMS); n = C.c_int64()
        rc = self._L.mpfmt_di_mf_probe(self._h, float(rho), float(r), acc.ctypes.data_as(C.POINTER(C.c_float)),
                                       oT.ctypes.data_as(C.POINTER(C.c_uint16)), oS.ctypes.data_as(C.POINTER(C.c_uint16)), _dp(terms), C.byref(n))
        out = dict(zip(("sp", "sv", "pc0", "pc1", "split", "accum", "E", "T", "negT", "usable", "Pm", "Vm", "F", "G", "N0", "guards"), terms.tolist()))
        out["pc"] = np.array([out.pop("pc0"), out.pop("pc1")]); out["usable"] = bool(out["usable"]); out["guards"] = int(out["guards"])
        out["negT"] = np.float32(out["negT"])
        self._chk(rc)
        assert n.value == npad
        out.update(acc=acc, opsT=oT.view(np.float16), opsS=oS.view(np.float16), npad=npad)
        return out

    def di_fmtstar(self, rho, r, goal_kind, goal_params, init_idx=1, checkpts=True):
        return self._steer_plan("di", "fmtstar", (rho, r), goal_kind, goal_params, init_idx, checkpts)

    def di_prmstar(self, rho, r, goal_kind, goal_params, init_idx=1, checkpts=True):
        """PRM* in the double-integrator space (mpfmt_di_prmstar): the graph and its sweep (reused while resident and valid, also after
        boxes_add / boxes_remove), the exact cost-to-come field of init_idx and the best goal sample; the dict of prmstar."""
        return self._steer_plan("di", "prmstar", (rho, r), goal_kind, goal_params, init_idx, checkpts)

    def car_prmstar(self, car, turn_radius, speed, r, goal_kind, goal_params, init_idx=1, checkpts=True):
        """dubins / reedsshepp PRM* (mpfmt_dubins_prmstar, mpfmt_reedsshepp_prmstar); the dict of prmstar."""
        return self._steer_plan(car, "prmstar", (turn_radius, speed, r), goal_kind, goal_params, init_idx, checkpts)

    def car_fmtstar_wavefront(self, car, turn_radius, speed, r, goal_kind, goal_params, band=0.0, single=False, init_idx=1, checkpts=True):
        """dubins / reedsshepp planner with the recursion on the device."""
        return self._steer_plan(car, "fmtstar_wavefront", (turn_radius, speed, r), goal_kind, goal_params, init_idx, checkpts,
                                wavefront=(band, WF_SINGLE if single else 0))

    def di_fmtstar_wavefront(self, rho, r, goal_kind, goal_params, band=0.0, single=False, init_idx=1, checkpts=True, want_tree=True):
        """di_fmtstar with the recursion on the device (directed wavefront form)."""
        return self._steer_plan("di", "fmtstar_wavefront", (rho, r), goal_kind, goal_params, init_idx, checkpts,
                                wavefront=(band, WF_SINGLE if single else 0), want_tree=want_tree)

    # ---- device-resident -------------------------------------------------------------------------
    def graph_build_device(self, r):
        nnz = C.c_int64()
        self._chk(self._L.mpfmt_graph_build_device(self._h, float(r), C.byref(nnz)))
        self.nnz = nnz.value
        return nnz.value

    def graph_sweep_device(self):
        self._chk(self._L.mpfmt_graph_sweep_device(self._h))

    def graph_step_device(self, r):
        """graph_build_device + graph_sweep_device with one host synchronisation (see include/mpfmt.h)."""
        nnz = C.c_int64()
        self._chk(self._L.mpfmt_graph_step_device(self._h, float(r), C.byref(nnz)))
        self.nnz = nnz.value
        return nnz.value

    def graph_step_launch(self, r):
        self._chk(self._L.mpfmt_graph_step_launch(self._h, float(r)))

    def graph_step_finish(self):
        nnz = C.c_int64()
        self._chk(self._L.mpfmt_graph_step_finish(self._h, C.byref(nnz)))
        self.nnz = nnz.value
        return nnz.value

    def graph_device_ptrs(self):
        p = [C.c_void_p() for _ in range(4)]
        self._chk(self._L.mpfmt_graph_device_ptrs(self._h, *[C.byref(x) for x in p]))
        return tuple(x.value for x in p)

    def graph_export(self, pinned=True, want_mask=True):
        """The resident graph + mask (as a step left them) in the ABI's host format: (colptr, rowval, nzval, mask, GB/s).  pinned: the
        destinations come from mpfmt_pinned_alloc (the copies then run at link speed); the arrays returned are copies."""
        N = self.N
        nnz = self.stat("nnz")
        words = (nnz + 63) // 64
        sizes = [8 * (N + 1), 8 * max(nnz, 1), 8 * max(nnz, 1), 8 * max(words, 1)]
        rate = C.c_double()
        if pinned:
            ptrs = []
            for b in sizes:
                p = C.c_void_p()
                rc = self._L.mpfmt_pinned_alloc(b, C.byref(p))
                if rc != 0:
                    raise MPFMTError(rc, "mpfmt_pinned_alloc failed")
                ptrs.append(p)
            try:
                self._chk(self._L.mpfmt_graph_export(self._h, C.cast(ptrs[0], c_i64_p), C.cast(ptrs[1], c_i64_p), C.cast(ptrs[2], c_d_p),
                                                     C.cast(ptrs[3], c_u64_p) if want_mask else None, C.byref(rate)))
                colptr = np.ctypeslib.as_array(C.cast(ptrs[0], c_i64_p), shape=(N + 1,)).copy()
                rowval = np.ctypeslib.as_array(C.cast(ptrs[1], c_i64_p), shape=(max(nnz, 1),))[:nnz].copy()
                nzval = np.ctypeslib.as_array(C.cast(ptrs[2], c_d_p), shape=(max(nnz, 1),))[:nnz].copy()
                mask = np.ctypeslib.as_array(C.cast(ptrs[3], c_u64_p), shape=(max(words, 1),))[:words].copy() if want_mask else None
            finally:
                for p in ptrs:
                    self._L.mpfmt_pinned_free(p)
        else:
            colptr = np.empty(N + 1, dtype=np.int64); rowval = np.empty(max(nnz, 1), dtype=np.int64)
            nzval = np.empty(max(nnz, 1), dtype=np.float64); mask = np.zeros(max(words, 1), dtype=np.uint64)
            self._chk(self._L.mpfmt_graph_export(self._h, _ip(colptr), _ip(rowval), _dp(nzval), _up(mask) if want_mask else None, C.byref(rate)))
            rowval, nzval, mask = rowval[:nnz], nzval[:nnz], (mask[:words] if want_mask else None)
        return colptr, rowval, nzval, mask, rate.value

    def graph_export_arena(self, want_mask=True, copy=True):
        """mpfmt_graph_export_pinned: the resident graph + mask into the ctx's own page-locked arena (kept across calls: only the first
        export of a ctx pays for page-locking).  copy=False returns views of the arena, valid until the next export / close."""
        cp, rv, nz, mk = c_i64_p(), c_i64_p(), c_d_p(), c_u64_p()
        nnz = C.c_int64(); rate = C.c_double()
        self._chk(self._L.mpfmt_graph_export_pinned(self._h, C.byref(cp), C.byref(rv), C.byref(nz), C.byref(mk) if want_mask else None,
                                                    C.byref(nnz), C.byref(rate)))
        n = nnz.value; words = (n + 63) // 64
        colptr = np.ctypeslib.as_array(cp, shape=(self.N + 1,))
        rowval = np.ctypeslib.as_array(rv, shape=(max(n, 1),))[:n]
        nzval = np.ctypeslib.as_array(nz, shape=(max(n, 1),))[:n]
        mask = np.ctypeslib.as_array(mk, shape=(max(words, 1),))[:words] if want_mask else None
        if copy:
            colptr, rowval, nzval = colptr.copy(), rowval.copy(), nzval.copy()
            mask = mask.copy() if mask is not None else None
        return colptr, rowval, nzval, mask, rate.value

    def rdisc_stream(self, r, Cc=None, H=None, want_free=False):
        """Per-column reductions of the r-disc graph without storing it: dict(deg, nnz[, parent (1-based, 0 = none), cost][, free_deg])."""
        N = self.N
        deg = np.zeros(max(N, 1), dtype=np.int64); fdeg = np.zeros(max(N, 1), dtype=np.int64)
        par = np.zeros(max(N, 1), dtype=np.int64); cost = np.zeros(max(N, 1), dtype=np.float64)
        nnz = C.c_int64()
        Cc_ = None if Cc is None else np.ascontiguousarray(Cc, dtype=np.float64)
        H_ = None if H is None else np.ascontiguousarray(H, dtype=np.uint64)
        self._chk(self._L.mpfmt_rdisc_stream(self._h, float(r), _dp(Cc_), _up(H_), int(bool(want_free)), _ip(deg), _ip(fdeg), _ip(par), _dp(cost),
                                             C.byref(nnz)))
        out = {"deg": deg[:N], "nnz": nnz.value}
        if Cc is not None:
            out["parent"], out["cost"] = par[:N], cost[:N]
        if want_free:
            out["free_deg"] = fdeg[:N]
        return out

    def shard_info(self):
        a, b, n = C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(self._L.mpfmt_shard_info(self._h, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def timing_reset(self):
        self._chk(self._L.mpfmt_timing_reset(self._h))

    def timing(self, name):
        ms, n = C.c_double(), C.c_int64()
        self._chk(self._L.mpfmt_timing_get(self._h, name.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def set_option(self, name, value):
        """mpfmt_set_option (include/mpfmt.h lists the options).  OPT_STEER_SHAPES_DELTA = 1: shapes_add / shapes_remove under a swept
        steering graph (double integrator in R^4, Dubins, Reeds-Shepp) bring mask and segment counts up to date in place."""
        self._chk(self._L.mpfmt_set_option(self._h, name.encode(), int(value)))

    def stat(self, name):
        v = C.c_int64()
        self._chk(self._L.mpfmt_get_stat(self._h, name.encode(), C.byref(v)))
        return v.value

    def graph_stats(self):
        v = [C.c_int64() for _ in range(4)]
        self._chk(self._L.mpfmt_graph_stats(self._h, *[C.byref(x) for x in v]))
        return dict(pairs_tested=v[0].value, tiles=v[1].value, slices=v[2].value, cells=v[3].value)
