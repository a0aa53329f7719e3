"""ctypes binding of libwgebra_hip.so (include/wgebra_hip.h).  No fallback: if the HIP library is missing or an
entry point is absent, importing this module raises -- the product path never routes around the GPU kernels."""
from __future__ import annotations

import ctypes
import os
import re

_PKG = os.path.dirname(os.path.abspath(__file__))
# WGEBRA_HIP_LIB selects another build of the SAME library (kernel A/B experiments); never a different backend.
LIB_PATH = os.environ.get("WGEBRA_HIP_LIB") or os.path.join(_PKG, "libwgebra_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "wgebra_hip.h")

# status codes (wg_status)
WG_OK, WG_ERR_DIM_MISMATCH, WG_ERR_PRECONDITION, WG_ERR_INVALID_ARG, WG_ERR_OUT_OF_BOUNDS, WG_ERR_HIP, \
    WG_ERR_UNSUPPORTED, WG_ERR_NO_DEVICE, WG_ERR_WORKSPACE, WG_ERR_ALIASED = range(10)
WG_VIEWS_OVERLAP_MAX_RUNS = 4096  # == the header's: above it wg_debug_views_overlap answers "overlaps" without deciding
WG_GATHER_RCCL, WG_GATHER_NONE, WG_GATHER_PEER_STAGED = 0, 2, 3  # (1 was the SDMA rect-copy engine: removed in ABI 3)
WG_COMM_ID_BYTES, WG_IPC_HANDLE_BYTES = 128, 96
ABI_VERSION = 5  # == WGEBRA_HIP_ABI_VERSION (checked when the library is loaded, and against the header by tests/test_abi_and_host.py)
WG_F32, WG_F16, WG_BF16 = 0, 1, 2
WG_TUNE_F16_TILE, WG_TUNE_F16_SCHED, WG_TUNE_F32_SKINNY, WG_TUNE_F32_PANELS, WG_TUNE_F16_BALANCE, WG_TUNE_F32_MID, WG_TUNE_F32_MID_SPLIT, WG_TUNE_GEMVT_LDS, WG_TUNE_F16_CONT, WG_TUNE_RM_TR_NATIVE = range(10)


class ViewShapeC(ctypes.Structure):
    """wg_view_shape == wgcore::shapes::ViewShape (#[repr(C)], 24 bytes; shapes.rs:9-21)."""
    _fields_ = [("size", ctypes.c_uint32 * 3), ("stride", ctypes.c_uint32), ("stride_mat", ctypes.c_uint32),
                ("offset", ctypes.c_uint32)]


assert ctypes.sizeof(ViewShapeC) == 24


class Gemm16QueryC(ctypes.Structure):
    """wg_gemm16_query: everything the 16-bit Gemm launcher's choice of kernels depends on (wg_debug_gemm16_plan)."""
    _fields_ = ([(n, ctypes.c_uint32) for n in ("trans", "M", "N", "K", "nmats", "lda", "ldb", "ldc")]
                + [(n, ctypes.c_uint64) for n in ("a_batch", "b_batch", "c_batch")]
                + [(n, ctypes.c_uint32) for n in ("a_addr", "b_addr", "c_addr")]
                + [("alpha", ctypes.c_float), ("beta", ctypes.c_float)]
                + [(n, ctypes.c_uint32) for n in ("panels", "panel_cols", "panel_n_main", "panel_n_tail")]
                + [("panel_tail_cols", ctypes.c_uint32 * 8), ("cus", ctypes.c_uint32)]
                + [(n, ctypes.c_int32) for n in ("tile", "sched", "cont", "balance")]
                + [(n, ctypes.c_uint32) for n in ("uneven_xcds", "recording", "bal_valid", "padded")])


GEMM16_LEAVES = ("skinny", "t256x128", "t128", "m16", "pad", "generic", "unsupported")  # wg_gemm16_leaf


class Gemm16PlanC(ctypes.Structure):
    """wg_gemm16_plan: the leaf (index into GEMM16_LEAVES) and what it is launched with."""
    _fields_ = ([(n, ctypes.c_uint32) for n in ("leaf", "tiles_m", "tiles_n", "nsplit", "k_per_split", "c_stream", "a_nt")]
                + [("workspace_bytes", ctypes.c_uint64)]
                + [(n, ctypes.c_uint32) for n in ("cont", "queues", "nwg", "bal_eligible", "bal_calib", "bal_wanted", "tail", "tail_split", "tail_kps",
                                                   "Mp", "Kp", "a_ok", "b_ok", "c_ok", "c_seed")]
                + [("status", ctypes.c_int32), ("message", ctypes.c_char * 128)])


class Gemm32QueryC(ctypes.Structure):
    """wg_gemm32_query: everything the f32 Gemm launcher's choice of kernels depends on (wg_debug_gemm32_plan)."""
    _fields_ = ([(n, ctypes.c_uint32) for n in ("trans", "M", "N", "K", "nmats", "lda", "ldb", "ldc")]
                + [(n, ctypes.c_uint64) for n in ("a_batch", "b_batch", "c_batch")]
                + [("alpha", ctypes.c_float), ("beta", ctypes.c_float), ("cus", ctypes.c_uint32)]
                + [(n, ctypes.c_int32) for n in ("mid", "mid_split", "skinny", "panels")])


GEMM32_LEAVES = ("nothing", "unsupported", "mid", "skinny", "skinny_panels", "skinny_t", "fewrow", "big")  # wg_gemm32_leaf


class Gemm32PlanC(ctypes.Structure):
    """wg_gemm32_plan: the leaf (index into GEMM32_LEAVES) and what it is launched with."""
    _fields_ = ([(n, ctypes.c_uint32) for n in ("leaf", "bm", "bn", "nsplit", "k_per_split", "npanels", "copy_a", "tail_r", "tail_sp", "tail_kps", "flat_tiles")]
                + [("workspace_bytes", ctypes.c_uint64), ("pad_workspace_bytes", ctypes.c_uint64)]
                + [("status", ctypes.c_int32), ("message", ctypes.c_char * 128)])


class GemvQ8QueryC(ctypes.Structure):
    """wg_gemv_q8_query: everything wg_gemv_q8's choice of kernel, cut and grid depends on (wg_debug_gemv_q8_plan)."""
    _fields_ = ([(n, ctypes.c_uint32) for n in ("trans", "rows", "cols", "nrhs", "mats", "group_rows", "ldm", "lds", "ldv", "ldo")]
                + [(n, ctypes.c_uint64) for n in ("m_batch", "s_batch", "v_batch", "o_batch")]
                + [(n, ctypes.c_uint32) for n in ("m_addr16", "v_addr16", "o_addr16", "cus")])


GEMV_Q8_LEAVES = ("nothing", "unsupported", "t", "n", "any_t", "any_n")  # wg_gemv_q8_leaf


class GemvQ8PlanC(ctypes.Structure):
    """wg_gemv_q8_plan: the leaf (index into GEMV_Q8_LEAVES) and what it is launched with."""
    _fields_ = ([(n, ctypes.c_uint32) for n in ("leaf", "rhs_tile", "rhs_groups", "loads", "cols", "nsplit", "k_per_split", "out_per_block")]
                + [("grid", ctypes.c_uint32 * 3), ("block", ctypes.c_uint32), ("workspace_bytes", ctypes.c_uint64)]
                + [("status", ctypes.c_int32), ("message", ctypes.c_char * 128)])


class GemvQ4QueryC(ctypes.Structure):
    """wg_gemv_q4_query: everything wg_gemv_q4's choice of kernel, cut and grid depends on (wg_debug_gemv_q4_plan). `rows`, `ldm` and `m_batch` count bytes."""
    _fields_ = ([(n, ctypes.c_uint32) for n in ("trans", "rows", "cols", "nrhs", "mats", "group_rows", "ldm", "lds", "ldv", "ldo")]
                + [(n, ctypes.c_uint64) for n in ("m_batch", "s_batch", "v_batch", "o_batch")]
                + [(n, ctypes.c_uint32) for n in ("m_addr16", "v_addr16", "cus")])


GEMV_Q4_LEAVES = ("nothing", "unsupported", "t", "any_t")  # wg_gemv_q4_leaf


class GemvQ4PlanC(ctypes.Structure):
    """wg_gemv_q4_plan: the leaf (index into GEMV_Q4_LEAVES) and what it is launched with; `k_per_split` counts logical rows."""
    _fields_ = ([(n, ctypes.c_uint32) for n in ("leaf", "rhs_tile", "rhs_groups", "loads", "cols", "nsplit", "k_per_split", "out_per_block")]
                + [("grid", ctypes.c_uint32 * 3), ("block", ctypes.c_uint32), ("workspace_bytes", ctypes.c_uint64)]
                + [("status", ctypes.c_int32), ("message", ctypes.c_char * 128)])


class GemmQ8QueryC(ctypes.Structure):
    """wg_gemm_q8_query: everything wg_gemm_q8's choice of kernel, column tile, cut and grid depends on (wg_debug_gemm_q8_plan)."""
    _fields_ = ([(n, ctypes.c_uint32) for n in ("k", "outputs", "n", "mats", "group_rows", "x_bf16", "ldm", "lds", "ldx", "ldo")]
                + [(n, ctypes.c_uint64) for n in ("m_batch", "s_batch", "x_batch", "o_batch")]
                + [(n, ctypes.c_uint32) for n in ("m_addr16", "x_addr16", "o_addr16", "cus")])


GEMM_Q8_LEAVES = ("nothing", "unsupported", "mfma", "any")  # wg_gemm_q8_leaf


class GemmQ8PlanC(ctypes.Structure):
    """wg_gemm_q8_plan: the leaf (index into GEMM_Q8_LEAVES) and what it is launched with."""
    _fields_ = ([(n, ctypes.c_uint32) for n in ("leaf", "col_tiles", "col_passes", "out_per_block", "nsplit", "k_per_split")]
                + [("grid", ctypes.c_uint32 * 3), ("block", ctypes.c_uint32), ("workspace_bytes", ctypes.c_uint64)]
                + [("status", ctypes.c_int32), ("message", ctypes.c_char * 128)])


class GemmQ8A8QueryC(ctypes.Structure):
    """wg_gemm_q8a8_query: wg_gemm_q8_query's fields plus the activations' group size and the view of their scales (wg_debug_gemm_q8a8_plan)."""
    _fields_ = ([(n, ctypes.c_uint32) for n in ("k", "outputs", "n", "mats", "group_rows", "x_group_rows", "ldm", "lds", "ldx", "ldxs", "ldo")]
                + [(n, ctypes.c_uint64) for n in ("m_batch", "s_batch", "x_batch", "xs_batch", "o_batch")]
                + [(n, ctypes.c_uint32) for n in ("m_addr16", "x_addr16", "o_addr16", "cus")])


GEMM_Q8A8_LEAVES = ("nothing", "unsupported", "mfma", "any")  # wg_gemm_q8a8_leaf


class GemmQ8A8PlanC(ctypes.Structure):
    """wg_gemm_q8a8_plan: the leaf (index into GEMM_Q8A8_LEAVES) and what it is launched with."""
    _fields_ = ([(n, ctypes.c_uint32) for n in ("leaf", "col_tiles", "col_passes", "out_per_block", "nsplit", "k_per_split")]
                + [("grid", ctypes.c_uint32 * 3), ("block", ctypes.c_uint32), ("workspace_bytes", ctypes.c_uint64)]
                + [("status", ctypes.c_int32), ("message", ctypes.c_char * 128)])


class QuantizeQ8QueryC(ctypes.Structure):
    """wg_quantize_q8_query: everything wg_quantize_q8's choice of kernel and grid depends on (wg_debug_quantize_q8_plan)."""
    _fields_ = ([(n, ctypes.c_uint32) for n in ("rows", "cols", "mats", "group_rows", "src_elem", "ldq", "ldsrc")]
                + [(n, ctypes.c_uint64) for n in ("q_batch", "src_batch")]
                + [(n, ctypes.c_uint32) for n in ("q_addr16", "src_addr16")])


QUANTIZE_Q8_LEAVES = ("nothing", "unsupported", "vec", "any")  # wg_quantize_q8_leaf


class QuantizeQ8PlanC(ctypes.Structure):
    """wg_quantize_q8_plan: the leaf (index into QUANTIZE_Q8_LEAVES), the lanes of a group, and the launch."""
    _fields_ = ([(n, ctypes.c_uint32) for n in ("leaf", "group_lanes", "blocks_per_col")]
                + [("grid", ctypes.c_uint32 * 3), ("block", ctypes.c_uint32)]
                + [("status", ctypes.c_int32), ("message", ctypes.c_char * 128)])


class GemmQ4QueryC(ctypes.Structure):
    """wg_gemm_q4_query: everything wg_gemm_q4's choice of kernel, column tile, cut and grid depends on (wg_debug_gemm_q4_plan). `k` counts logical rows, `ldm` and
    `m_batch` bytes."""
    _fields_ = ([(n, ctypes.c_uint32) for n in ("k", "outputs", "n", "mats", "group_rows", "x_bf16", "ldm", "lds", "ldx", "ldo")]
                + [(n, ctypes.c_uint64) for n in ("m_batch", "s_batch", "x_batch", "o_batch")]
                + [(n, ctypes.c_uint32) for n in ("m_addr16", "x_addr16", "o_addr16", "cus")])


GEMM_Q4_LEAVES = ("nothing", "unsupported", "mfma", "any")  # wg_gemm_q4_leaf


class GemmQ4PlanC(ctypes.Structure):
    """wg_gemm_q4_plan: the leaf (index into GEMM_Q4_LEAVES) and what it is launched with; `step` and `k_per_split` count logical rows."""
    _fields_ = ([(n, ctypes.c_uint32) for n in ("leaf", "step", "col_tiles", "col_passes", "out_per_block", "nsplit", "k_per_split")]
                + [("grid", ctypes.c_uint32 * 3), ("block", ctypes.c_uint32), ("workspace_bytes", ctypes.c_uint64)]
                + [("status", ctypes.c_int32), ("message", ctypes.c_char * 128)])


class GemvQueryC(ctypes.Structure):
    """wg_gemv_query: everything the Gemv launchers' choice of kernel, cut and grid depends on (wg_debug_gemv_plan, wg_debug_gemv_any_plan)."""
    _fields_ = ([(n, ctypes.c_uint32) for n in ("trans", "rows_out", "k", "nrhs", "nmats", "m_elem", "v_elem", "bf16", "gemm16", "ldm", "ldv", "ldo")]
                + [(n, ctypes.c_uint64) for n in ("m_batch", "v_batch", "o_batch")]
                + [(n, ctypes.c_uint32) for n in ("m_addr16", "v_addr16", "cus")] + [("gemvt_lds", ctypes.c_int32)])


GEMV_LEAVES = ("nothing", "unsupported", "small", "n", "t", "tcols", "tlds", "as_gemm32", "as_gemm16")  # wg_gemv_leaf


class GemvPlanC(ctypes.Structure):
    """wg_gemv_plan: the leaf (index into GEMV_LEAVES) and what it is launched with."""
    _fields_ = ([(n, ctypes.c_uint32) for n in ("leaf", "rhs_tile", "rhs_groups", "e", "u", "v", "rl", "lds_cols", "lds_threads", "lds_kc", "lds_bytes", "nsplit", "k_per_split")]
                + [("grid", ctypes.c_uint32 * 3), ("block", ctypes.c_uint32), ("combine_grid", ctypes.c_uint32 * 3), ("workspace_bytes", ctypes.c_uint64)]
                + [("status", ctypes.c_int32), ("message", ctypes.c_char * 128), ("gemm32", Gemm32PlanC)])


class GemvAnyPlanC(ctypes.Structure):
    """wg_gemv_any_plan: cut, chunks of grid.z, workspace and tag of the any-alignment kernels."""
    _fields_ = ([(n, ctypes.c_uint32) for n in ("launch", "nsplit", "per_split", "grid_x", "zchunk", "nchunks", "nt")] + [("workspace_bytes", ctypes.c_uint64)]
                + [("status", ctypes.c_int32), ("message", ctypes.c_char * 128), ("tag", ctypes.c_char * 48)])


class WgError(RuntimeError):
    """A non-OK wg_status.  `.status` is the code, the message is wg_last_error_string()."""

    def __init__(self, status: int, message: str):
        super().__init__(message)
        self.status = status


class DimensionMismatch(WgError, AssertionError):
    """What the reference raises as a panic from assert_eq!(..., "... dimension mismatch.")."""


class PreconditionFailed(WgError, AssertionError):
    pass


class NoDevice(WgError):
    pass


class WorkspaceMustGrow(WgError):
    """A context scratch region would have to grow inside a recording (WG_ERR_WORKSPACE): run the call once eagerly first."""


class AliasedOperands(WgError):
    """The written view of a call shares memory with a view the call reads (WG_ERR_ALIASED): nothing was launched. The reference gets a wgpu validation panic
    for binding one buffer read_write and read; here views of one buffer are legal as long as their footprints are disjoint, and OpAssign / Axpy take the
    identical view on both sides (include/wgebra_hip.h, the aliasing rule)."""


def declared_symbols(header_path: str = HEADER_PATH) -> list[str]:
    """Every function the public header declares (used by the ABI-completeness test)."""
    text = open(header_path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(wg_[a-z0-9_]+)\s*\(", text)))


def _load() -> ctypes.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `make -C wgmath_amd/csrc`. There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    pd = ctypes.POINTER(ctypes.c_double)
    vp, cp, ci, u32, u64, sz = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t
    pvp = ctypes.POINTER(vp)
    S = ViewShapeC
    sig = {
        "wg_abi_version": (ci, []),
        "wg_last_error_string": (cp, []),
        "wg_device_count": (ci, []),
        "wg_ctx_create": (ci, [ci, pvp]),
        "wg_ctx_create_on_stream": (ci, [ci, vp, pvp]),
        "wg_ctx_create_with_cu_count": (ci, [ci, ctypes.c_uint32, ctypes.POINTER(vp)]),
        "wg_ctx_create_with_cu_count_one_xcd": (ci, [ci, ctypes.c_uint32, ctypes.POINTER(vp)]),
        "wg_ctx_destroy": (ci, [vp]),
        "wg_ctx_sync": (ci, [vp]),
        "wg_ctx_device": (ci, [vp]),
        "wg_ctx_stream": (vp, [vp]),
        "wg_ctx_device_info": (ci, [vp, cp, ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(u64)]),
        "wg_ctx_mem_info": (ci, [vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]),
        "wg_ctx_reserve_workspace": (ci, [vp, sz]),
        "wg_debug_f16_balance_plan": (ci, [ctypes.POINTER(ctypes.c_double), u32, u32, ci, ctypes.POINTER(u32), u32, ctypes.POINTER(u32), ctypes.POINTER(u32)]),
        "wg_debug_gemm16_plan": (ci, [ctypes.POINTER(Gemm16QueryC), cp, ctypes.POINTER(Gemm16PlanC), cp, sz, ctypes.POINTER(Gemm16QueryC)]),
        "wg_debug_gemm32_plan": (ci, [ctypes.POINTER(Gemm32QueryC), ctypes.POINTER(Gemm32PlanC), cp, sz, ctypes.POINTER(Gemm32QueryC)]),
        "wg_ctx_f16_balance_info": (ci, [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ci), ctypes.POINTER(u32), ctypes.POINTER(u32)]),
        "wg_debug_views_overlap": (ci, [S, u64, S, u64, u32, ctypes.POINTER(ci)]),
        "wg_debug_take_path": (ci, [vp, cp, sz]),
        "wg_ctx_set_tuning": (ci, [vp, ci, ci]),
        "wg_ctx_get_tuning": (ci, [vp, ci, ctypes.POINTER(ci)]),
        "wg_debug_spin": (ci, [vp, ctypes.c_uint32, ctypes.c_uint32, vp]),
        "wg_geometry_apply": (ci, [vp, ci, ctypes.c_uint32, vp, vp, ctypes.c_uint32]),
        "wg_buf_create": (ci, [vp, sz, u32, pvp]),
        "wg_buf_create_init": (ci, [vp, vp, sz, u32, pvp]),
        "wg_buf_wrap": (ci, [vp, vp, sz, pvp]),
        "wg_buf_destroy": (ci, [vp]),
        "wg_buf_size": (sz, [vp]),
        "wg_buf_device_ptr": (vp, [vp]),
        "wg_buf_write": (ci, [vp, vp, sz, vp, sz]),
        "wg_buf_read": (ci, [vp, vp, sz, vp, sz]),
        "wg_buf_copy": (ci, [vp, vp, sz, vp, sz, sz]),
        "wg_buf_fill_zero": (ci, [vp, vp]),
        "wg_gemm": (ci, [vp, ci, ci, vp, S, vp, S, vp, S]),
        "wg_gemm_ex": (ci, [vp, ci, ci, ctypes.c_float, ctypes.c_float, vp, S, vp, S, vp, S]),
        "wg_gemv": (ci, [vp, ci, ci, vp, S, vp, S, vp, S]),
        "wg_gemv_mixed": (ci, [vp, ci, ci, vp, S, vp, S, vp, S]),
        "wg_gemv_q8": (ci, [vp, ci, u32, vp, S, vp, S, vp, S, vp, S]),
        "wg_debug_gemv_q8_plan": (ci, [ctypes.POINTER(GemvQ8QueryC), ctypes.POINTER(GemvQ8PlanC), cp, sz]),
        "wg_gemv_q4": (ci, [vp, ci, u32, vp, S, vp, S, vp, S, vp, S]),
        "wg_debug_gemv_q4_plan": (ci, [ctypes.POINTER(GemvQ4QueryC), ctypes.POINTER(GemvQ4PlanC), cp, sz]),
        "wg_gemm_q8": (ci, [vp, ci, u32, ci, vp, S, vp, S, vp, S, vp, S]),
        "wg_debug_gemm_q8_plan": (ci, [ctypes.POINTER(GemmQ8QueryC), ctypes.POINTER(GemmQ8PlanC), cp, sz]),
        "wg_gemm_q4": (ci, [vp, ci, u32, ci, vp, S, vp, S, vp, S, vp, S]),
        "wg_debug_gemm_q4_plan": (ci, [ctypes.POINTER(GemmQ4QueryC), ctypes.POINTER(GemmQ4PlanC), cp, sz]),
        "wg_gemm_q8a8": (ci, [vp, ci, u32, u32, vp, S, vp, S, vp, S, vp, S, vp, S]),
        "wg_debug_gemm_q8a8_plan": (ci, [ctypes.POINTER(GemmQ8A8QueryC), ctypes.POINTER(GemmQ8A8PlanC), cp, sz]),
        "wg_quantize_q8": (ci, [vp, ci, u32, vp, S, vp, S, vp, S]),
        "wg_debug_quantize_q8_plan": (ci, [ctypes.POINTER(QuantizeQ8QueryC), ctypes.POINTER(QuantizeQ8PlanC)]),
        "wg_debug_gemv_plan": (ci, [ctypes.POINTER(GemvQueryC), ctypes.POINTER(GemvPlanC), cp, sz]),
        "wg_debug_gemv_any_plan": (ci, [ctypes.POINTER(GemvQueryC), ctypes.POINTER(GemvAnyPlanC), cp, sz]),
        "wg_gemm_out32": (ci, [vp, ci, ci, ctypes.c_float, ctypes.c_float, vp, S, vp, S, vp, S]),
        "wg_debug_gemm_out32_query": (ci, [ctypes.POINTER(Gemm16QueryC)]),
        "wg_gemm_rm": (ci, [vp, ci, ci, vp, S, vp, S, vp, S]),
        "wg_gemv_rm": (ci, [vp, ci, ci, vp, S, vp, S, vp, S]),
        "wg_gemv_reduce": (ci, [vp, ci, ci, ci, vp, vp, S, vp, S]),
        "wg_reduce": (ci, [vp, ci, ci, vp, S, vp]),
        "wg_reduce_fast": (ci, [vp, ci, ci, vp, S, vp]),
        "wg_reduce_batched": (ci, [vp, ci, ci, vp, S, vp]),
        "wg_op_assign": (ci, [vp, ci, ci, vp, S, vp, S]),
        "wg_axpy": (ci, [vp, ctypes.c_float, ci, vp, S, vp, S]),
        "wg_copy_view": (ci, [vp, ci, vp, S, vp, S]),
        "wg_debug_clock_begin": (ci, [vp]),
        "wg_debug_clock_end": (ci, [vp, pd, pd, pd, pd]),
        "wg_debug_mfma_ceiling": (ci, [vp, ctypes.c_double, pd, pd]),
        "wg_comm_unique_id": (ci, [vp]),
        "wg_comm_create": (ci, [vp, ci, ci, vp, pvp]),
        "wg_comm_destroy": (ci, [vp]),
        "wg_comm_rank": (ci, [vp]),
        "wg_comm_size": (ci, [vp]),
        "wg_comm_has_collectives": (ci, [vp]),
        "wg_comm_reported_size": (ci, [vp, ctypes.POINTER(ci)]),
        "wg_comm_bytes_sent": (u64, [vp]),
        "wg_all_gather": (ci, [vp, ci, vp, u64, u64]),
        "wg_comm_join": (ci, [vp]),
        "wg_comm_set_pipelined": (ci, [vp, ci]),
        "wg_comm_set_one_launch": (ci, [vp, ci]),
        "wg_comm_flush": (ci, [vp]),
        "wg_comm_barrier": (ci, [vp]),
        "wg_buf_ipc_export": (ci, [vp, vp]),
        "wg_buf_ipc_open": (ci, [vp, vp, pvp]),
        "wg_comm_stage_reserve": (ci, [vp, sz, pvp, pvp]),
        "wg_comm_set_peer_stages": (ci, [vp, pvp, pvp]),
        "wg_cube_to_matrix": (ci, [vp, ci, vp, S, vp, S]),
        "wg_gemm_sharded": (ci, [vp, ci, ci, ci, u32, vp, S, vp, S, vp, S]),
        "wg_comm_set_wait_timing": (ci, [vp, ci]),
        "wg_comm_wait_times": (ci, [vp, ctypes.POINTER(u32), ctypes.POINTER(ctypes.c_float), u32, ctypes.POINTER(u32)]),
        "wg_gemm_sharded_panels": (ci, [vp, ci, ci, ci, ctypes.POINTER(u32), u32, vp, S, vp, S, vp, S]),
        "wg_encoder_begin": (ci, [vp]),
        "wg_encoder_finish": (ci, [vp, pvp]),
        "wg_queue_submit": (ci, [vp, vp]),
        "wg_cmdbuf_destroy": (ci, [vp]),
        "wg_timestamps_create": (ci, [vp, u32, pvp]),
        "wg_timestamps_destroy": (ci, [vp]),
        "wg_timestamps_clear": (ci, [vp]),
        "wg_timestamps_write": (ci, [vp, vp, ctypes.POINTER(u32)]),
        "wg_timestamps_reserve": (ci, [vp, u32, ctypes.POINTER(u32)]),
        "wg_timestamps_write_at": (ci, [vp, vp, u32]),
        "wg_timestamps_len": (u32, [vp]),
        "wg_timestamps_wait_for_results_ms": (ci, [vp, ctypes.POINTER(ctypes.c_double), u32]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export it: fail loudly
        fn.restype = res
        fn.argtypes = args
    lib._wg_signatures = sig
    # a stale build of the library with every symbol this binding names but other semantics must not pass for the current one
    if lib.wg_abi_version() != ABI_VERSION:
        raise ImportError(f"{LIB_PATH} reports ABI version {lib.wg_abi_version()}, this binding is written for {ABI_VERSION} "
                          f"(include/wgebra_hip.h: WGEBRA_HIP_ABI_VERSION): rebuild with `make -C wgmath_amd/csrc`")
    return lib


def hip_runtime_paths() -> list[str]:
    """Distinct libamdhip64 images mapped into this process."""
    paths = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    paths.add(line.split()[-1])
    except OSError:
        pass
    return sorted(paths)


def assert_single_hip_runtime() -> None:
    """PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64. If this library was loaded BEFORE torch, the
    process ends up with two HIP runtimes and the second one cannot open the GPU ("no HIP device visible"). Import torch
    first whenever both are used in one process (bench.py does for --gpus > 1)."""
    p = hip_runtime_paths()
    if len(p) > 1:
        raise ImportError("two HIP runtimes are loaded in this process: " + ", ".join(p) +
                          ". Import torch BEFORE wgmath_amd so that libwgebra_hip.so binds to torch's bundled runtime.")


lib = _load()

_EXC = {WG_ERR_DIM_MISMATCH: DimensionMismatch, WG_ERR_PRECONDITION: PreconditionFailed, WG_ERR_NO_DEVICE: NoDevice, WG_ERR_WORKSPACE: WorkspaceMustGrow,
        WG_ERR_ALIASED: AliasedOperands}


def check(status: int) -> None:
    if status != WG_OK:
        msg = lib.wg_last_error_string().decode("utf-8", "replace")
        raise _EXC.get(status, WgError)(status, msg or f"wg_status {status}")
