"""Host-side mirror of wgebra's dense operator surface over the C ABI (include/wgebra_hip.h).

  Gemm / GemmVariant         crates/wgebra/src/linalg/gemm.rs:9-127
  Gemv / GemvVariant         crates/wgebra/src/linalg/gemv.rs:9-137
  Reduce / ReduceOp          crates/wgebra/src/linalg/reduce.rs:13-113
  OpAssign / OpAssignVariant crates/wgebra/src/linalg/op_assign.rs:12-95

Signatures keep the reference's parameter order -- dispatch(device, shapes, pass, out, a, b[, variant]) -- so that a test
written against the reference reads the same here.  `device` and `shapes` are accepted for signature compatibility; the
work is enqueued on the stream behind `pass`.  Where the reference panics (assert_eq!), these raise an exception that
is also an AssertionError, carrying the reference's message.
"""
from __future__ import annotations

import enum

import numpy as np

from ._lib import check, lib
from .wgcore import ComputePass, GpuTensor, GpuTensorView, ViewShapeBuffers, as_view, wg_dtype


class GemmVariant(enum.IntEnum):  # gemm.rs:26-35
    Gemm = 0
    GemmFast = 1
    GemmTr = 2
    GemmTrFast = 3


class GemvVariant(enum.IntEnum):  # gemv.rs:25-34
    Gemv = 0
    GemvFast = 1
    GemvTr = 2
    GemvTrFast = 3


class ReduceOp(enum.IntEnum):  # reduce.rs:13-27
    Min = 0
    Max = 1
    Sum = 2
    Prod = 3
    SqNorm = 4


class OpAssignVariant(enum.IntEnum):  # op_assign.rs:12-26
    Add = 0
    Sub = 1
    Mul = 2
    Div = 3
    Copy = 4


def _common_dtype(*views: GpuTensorView):
    dt = views[0]._tensor.dtype
    for v in views[1:]:
        if v._tensor.dtype is not dt and v._tensor.dtype != dt:
            raise TypeError(f"operands must share one element type, got {[str(x.dtype) for x in views]}")
    return wg_dtype(dt)


def _mixed_dtype(out: GpuTensorView, m: GpuTensorView, v: GpuTensorView) -> int:
    """The matrix's wg_dtype of a mixed-precision call: `m` float16 / bfloat16 / float32, `v` and `out` float32 -- anything else is a TypeError."""
    md = wg_dtype(m._tensor.dtype)
    for name, x in (("v", v), ("out", out)):
        if np.dtype(x._tensor.dtype) != np.dtype(np.float32):
            raise TypeError(f"mixed-precision Gemv: `{name}` must be float32, got {x._tensor.dtype} (`m` carries the 16-bit type)")
    return md


def _q8_dtypes(out: GpuTensorView, m: GpuTensorView, scales: GpuTensorView, v: GpuTensorView) -> None:
    """The element types of a q8 call: `m` int8, `scales`, `v` and `out` float32 -- anything else is a TypeError."""
    if np.dtype(m._tensor.dtype) != np.dtype(np.int8):
        raise TypeError(f"q8 Gemv: `m` must be int8, got {m._tensor.dtype}")
    for name, x in (("scales", scales), ("v", v), ("out", out)):
        if np.dtype(x._tensor.dtype) != np.dtype(np.float32):
            raise TypeError(f"q8 Gemv: `{name}` must be float32, got {x._tensor.dtype} (`m` carries the int8 weights)")


def _gemm_q8_dtypes(out: GpuTensorView, m: GpuTensorView, scales: GpuTensorView, x: GpuTensorView) -> int:
    """The wg_dtype of `x` in a q8 Gemm: `m` int8, `scales` and `out` float32, `x` float16 or bfloat16 -- anything else is a TypeError."""
    if np.dtype(m._tensor.dtype) != np.dtype(np.int8):
        raise TypeError(f"q8 Gemm: `m` must be int8, got {m._tensor.dtype}")
    for name, t in (("scales", scales), ("out", out)):
        if np.dtype(t._tensor.dtype) != np.dtype(np.float32):
            raise TypeError(f"q8 Gemm: `{name}` must be float32, got {t._tensor.dtype} (`m` carries the int8 weights)")
    if np.dtype(x._tensor.dtype) == np.dtype(np.float32):
        raise TypeError("q8 Gemm: `x` must be float16 or bfloat16 (float32 activations are Gemv.dispatch_q8*)")
    return wg_dtype(x._tensor.dtype)  # (float16 or bfloat16: every other element type is a TypeError there)


def _gemm_q8a8_dtypes(out: GpuTensorView, m: GpuTensorView, scales: GpuTensorView, x: GpuTensorView, x_scales: GpuTensorView) -> None:
    """The element types of a q8a8 Gemm: `m` and `x` int8, `scales`, `x_scales` and `out` float32 -- anything else is a TypeError."""
    for name, t in (("m", m), ("x", x)):
        if np.dtype(t._tensor.dtype) != np.dtype(np.int8):
            raise TypeError(f"q8a8 Gemm: `{name}` must be int8, got {t._tensor.dtype}" + (" (float16 / bfloat16 activations are Gemm.dispatch_q8*)" if name == "x" else ""))
    for name, t in (("scales", scales), ("x_scales", x_scales), ("out", out)):
        if np.dtype(t._tensor.dtype) != np.dtype(np.float32):
            raise TypeError(f"q8a8 Gemm: `{name}` must be float32, got {t._tensor.dtype} (`m` and `x` carry the int8 values)")


def _gemm_q4_dtypes(out: GpuTensorView, m: GpuTensorView, scales: GpuTensorView, x: GpuTensorView) -> int:
    """The wg_dtype of `x` in a q4 Gemm: `m` uint8 (packed), `scales` and `out` float32, `x` float16 or bfloat16 -- anything else is a TypeError."""
    if np.dtype(m._tensor.dtype) != np.dtype(np.uint8):
        raise TypeError(f"q4 Gemm: `m` must be uint8 (two packed 4-bit weights per byte), got {m._tensor.dtype}")
    for name, t in (("scales", scales), ("out", out)):
        if np.dtype(t._tensor.dtype) != np.dtype(np.float32):
            raise TypeError(f"q4 Gemm: `{name}` must be float32, got {t._tensor.dtype} (`m` carries the packed weights)")
    if np.dtype(x._tensor.dtype) == np.dtype(np.float32):
        raise TypeError("q4 Gemm: `x` must be float16 or bfloat16 (float32 activations are Gemv.dispatch_q4*)")
    return wg_dtype(x._tensor.dtype)  # (float16 or bfloat16: every other element type is a TypeError there)


def _q8_groups(rows: int, group_rows: int) -> int:
    group_rows = int(group_rows)
    if group_rows <= 0 or (group_rows % 16 and group_rows < rows):
        raise ValueError(f"group_rows {group_rows} is neither a positive multiple of 16 nor at least the {rows} rows of the matrix")
    return group_rows


def quantize_q8(w32, group_rows: int):
    """float32 weights (rows x cols, or rows x cols x mats) -> (q int8, scales float32) in the layout of `Gemv.dispatch_q8*`: groups of `group_rows` consecutive ROWS
    of a column share a scale (a partial last group; group_rows >= rows: one scale per column). Per group s = fl32(max|w| / 127) and q = clip(rint(w / s), -127, 127)
    (-128 is never produced); an all-zero group gives s = 0, q = 0. `scales` has ceil(rows / group_rows) rows."""
    w = np.asarray(w32, np.float32)
    if w.ndim not in (2, 3):
        raise ValueError("quantize_q8 takes a matrix (rows x cols) or a cube (rows x cols x mats)")
    rows = w.shape[0]
    g = _q8_groups(rows, group_rows)
    ng = -(-rows // g) if rows else 0
    q = np.zeros(w.shape, np.int8)
    scales = np.zeros((ng,) + w.shape[1:], np.float32)
    for i in range(ng):
        blk = w[i * g:(i + 1) * g]
        s = (np.abs(blk).max(axis=0) / np.float32(127)).astype(np.float32)
        scales[i] = s
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.rint(blk / s)
        q[i * g:(i + 1) * g] = np.clip(np.where(s == 0, np.float32(0), r), -127, 127).astype(np.int8)
    return q, scales


def dequantize_q8(q, scales, group_rows: int) -> np.ndarray:
    """The float32 matrix `Gemv.dispatch_q8*` multiplies with: w[r, c] = fl32(scales[r // group_rows, c] * q[r, c])."""
    q, scales = np.asarray(q), np.asarray(scales, np.float32)
    if q.dtype != np.dtype(np.int8):
        raise TypeError(f"dequantize_q8 takes int8 weights, not {q.dtype}")
    g = _q8_groups(q.shape[0], group_rows)
    idx = np.arange(q.shape[0]) // g
    if scales.shape != (-(-q.shape[0] // g) if q.shape[0] else 0,) + q.shape[1:]:
        raise ValueError(f"scales of shape {scales.shape} do not belong to weights of shape {q.shape} in groups of {g} rows")
    return (scales[idx] * q.astype(np.float32)).astype(np.float32)


def _q4_dtypes(out: GpuTensorView, m: GpuTensorView, scales: GpuTensorView, v: GpuTensorView) -> None:
    """The element types of a q4 call: `m` uint8 (packed bytes), `scales`, `v` and `out` float32 -- anything else is a TypeError."""
    if np.dtype(m._tensor.dtype) != np.dtype(np.uint8):
        raise TypeError(f"q4 Gemv: `m` must be uint8 (two packed weights per byte: pack_q4), got {m._tensor.dtype}")
    for name, x in (("scales", scales), ("v", v), ("out", out)):
        if np.dtype(x._tensor.dtype) != np.dtype(np.float32):
            raise TypeError(f"q4 Gemv: `{name}` must be float32, got {x._tensor.dtype} (`m` carries the packed weights)")


def _q4_groups(k: int, group_rows: int) -> int:
    group_rows = int(group_rows)
    if group_rows <= 0 or (group_rows % 32 and group_rows < k):
        raise ValueError(f"group_rows {group_rows} is neither a positive multiple of 32 nor at least the {k} logical rows of the matrix")
    return group_rows


def pack_q4(q) -> np.ndarray:
    """Integers in -8 .. 7 (k x cols, or k x cols x mats; k even) -> the packed uint8 matrix of `Gemv.dispatch_q4*` (k / 2 x ...): byte j of a column holds logical row
    2 j in its LOW nibble and row 2 j + 1 in its HIGH nibble, each as n = q + 8."""
    q = np.asarray(q)
    if not np.issubdtype(q.dtype, np.integer):
        raise TypeError(f"pack_q4 takes integers, not {q.dtype}")
    if q.ndim not in (2, 3):
        raise ValueError("pack_q4 takes a matrix (k x cols) or a cube (k x cols x mats)")
    if q.shape[0] % 2:
        raise ValueError(f"pack_q4: {q.shape[0]} rows -- two weights share a byte, the row count must be even")
    if q.size and (q.min() < -8 or q.max() > 7):
        raise ValueError("pack_q4: values outside -8 .. 7")
    n = (q.astype(np.int16) + 8).astype(np.uint8)
    return (n[0::2] | (n[1::2] << 4)).astype(np.uint8)


def unpack_q4(packed) -> np.ndarray:
    """The inverse of `pack_q4`: packed uint8 (k / 2 x ...) -> int8 in -8 .. 7 (k x ...)."""
    p = np.asarray(packed)
    if p.dtype != np.dtype(np.uint8):
        raise TypeError(f"unpack_q4 takes uint8 bytes, not {p.dtype}")
    if p.ndim not in (2, 3):
        raise ValueError("unpack_q4 takes a matrix (k / 2 x cols) or a cube (k / 2 x cols x mats)")
    q = np.empty((2 * p.shape[0],) + p.shape[1:], np.int8)
    q[0::2] = (p & 15).astype(np.int8) - 8
    q[1::2] = (p >> 4).astype(np.int8) - 8
    return q


def quantize_q4(w32, group_rows: int):
    """float32 weights (k x cols, or k x cols x mats; k even) -> (packed uint8, scales float32) in the layout of `Gemv.dispatch_q4*`: groups of `group_rows` consecutive
    ROWS of a column share a scale (a partial last group; group_rows >= k: one scale per column). Per group s = fl32(max|w| / 7) and q = clip(rint(w / s), -7, 7)
    (-8 is never produced); an all-zero group gives s = 0, q = 0. `scales` has ceil(k / group_rows) rows."""
    w = np.asarray(w32, np.float32)
    if w.ndim not in (2, 3):
        raise ValueError("quantize_q4 takes a matrix (k x cols) or a cube (k x cols x mats)")
    k = w.shape[0]
    if k % 2:
        raise ValueError(f"quantize_q4: {k} rows -- two weights share a byte, the row count must be even")
    g = _q4_groups(k, group_rows)
    ng = -(-k // g) if k else 0
    q = np.zeros(w.shape, np.int8)
    scales = np.zeros((ng,) + w.shape[1:], np.float32)
    for i in range(ng):
        blk = w[i * g:(i + 1) * g]
        s = (np.abs(blk).max(axis=0) / np.float32(7)).astype(np.float32)
        scales[i] = s
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.rint(blk / s)
        q[i * g:(i + 1) * g] = np.clip(np.where(s == 0, np.float32(0), r), -7, 7).astype(np.int8)
    return pack_q4(q), scales


def dequantize_q4(packed, scales, group_rows: int) -> np.ndarray:
    """The float32 matrix `Gemv.dispatch_q4*` multiplies with: w[r, c] = fl32(scales[r // group_rows, c] * q[r, c]), q = unpack_q4(packed)."""
    q, scales = unpack_q4(packed), np.asarray(scales, np.float32)
    g = _q4_groups(q.shape[0], group_rows)
    idx = np.arange(q.shape[0]) // g
    if scales.shape != (-(-q.shape[0] // g) if q.shape[0] else 0,) + q.shape[1:]:
        raise ValueError(f"scales of shape {scales.shape} do not belong to {q.shape[0]} x {q.shape[1:]} weights in groups of {g} rows")
    return (scales[idx] * q.astype(np.float32)).astype(np.float32)


def _out32_dtype(out: GpuTensorView, m1: GpuTensorView, m2: GpuTensorView) -> int:
    """The operands' wg_dtype of an f32-output Gemm: `m1` and `m2` share float16 / bfloat16 / float32, `out` is float32 -- anything else is a TypeError."""
    dt = _common_dtype(m1, m2)
    if np.dtype(out._tensor.dtype) != np.dtype(np.float32):
        raise TypeError(f"f32-output Gemm: `out` must be float32, got {out._tensor.dtype} (`m1` and `m2` carry the 16-bit type)")
    return dt


def row_major_shader_defs() -> dict:
    """linalg/shape.rs:11-15: the shader definitions that switch `Shape` to row-major.  Pass them to `Gemm.from_device` /
    `Gemv.from_device` (the reference passes them to the shader composer) to get operators whose matrix views are row-major."""
    return {"ROW_MAJOR": True}


def _is_row_major(shader_defs) -> bool:
    return bool(shader_defs) and bool(shader_defs.get("ROW_MAJOR", False))


class Gemm:
    """gemm.rs:9-21.  The four pipelines of the reference are one ahead-of-time compiled MFMA kernel family here, so
    construction is free (no shader compilation)."""

    def __init__(self, device=None, shader_defs=None):
        self.device = device
        self.row_major = _is_row_major(shader_defs)

    @staticmethod
    def from_device(device, shader_defs=None) -> "Gemm":
        return Gemm(device, shader_defs)

    def dispatch(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, out, m1, m2) -> None:
        self.dispatch_generic(device, shapes, pass_, out, m1, m2, GemmVariant.Gemm)

    def dispatch_tr(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, out, m1, m2) -> None:
        self.dispatch_generic(device, shapes, pass_, out, m1, m2, GemmVariant.GemmTr)

    def dispatch_generic(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, out, m1, m2, variant: GemmVariant) -> None:
        out, m1, m2 = as_view(out, 3), as_view(m1, 3), as_view(m2, 3)
        dt = _common_dtype(out, m1, m2)
        fn = lib.wg_gemm_rm if self.row_major else lib.wg_gemm
        check(fn(pass_._ctx.handle, int(variant), dt,
                 out.buffer()._h, out.shape().to_c(), m1.buffer()._h, m1.shape().to_c(),
                 m2.buffer()._h, m2.shape().to_c()))


    def dispatch_ex(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, alpha: float, beta: float, out, m1, m2,
                    variant: GemmVariant = GemmVariant.Gemm) -> None:
        """Extension: out = alpha * op(m1) * m2 + beta * out.  (1, 0) is bit-identical to dispatch_generic."""
        out, m1, m2 = as_view(out, 3), as_view(m1, 3), as_view(m2, 3)
        dt = _common_dtype(out, m1, m2)
        check(lib.wg_gemm_ex(pass_._ctx.handle, int(variant), dt, float(alpha), float(beta),
                             out.buffer()._h, out.shape().to_c(), m1.buffer()._h, m1.shape().to_c(),
                             m2.buffer()._h, m2.shape().to_c()))


    def dispatch_out32(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, out, m1, m2) -> None:
        self.dispatch_out32_generic(device, shapes, pass_, out, m1, m2, GemmVariant.Gemm)

    def dispatch_out32_tr(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, out, m1, m2) -> None:
        self.dispatch_out32_generic(device, shapes, pass_, out, m1, m2, GemmVariant.GemmTr)

    def dispatch_out32_generic(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, out, m1, m2, variant: GemmVariant,
                               alpha: float = 1.0, beta: float = 0.0) -> None:
        """Extension (`wg_gemm_out32`): float16 / bfloat16 `m1` and `m2` with a float32 `out` = alpha * op(m1) * m2 + beta * out. The f32 accumulators of the
        16-bit Gemm are stored as they are (no 16-bit rounding anywhere); float32 operands are `dispatch_ex`. Column-major views only (the row-major surface
        has no f32-output form)."""
        out, m1, m2 = as_view(out, 3), as_view(m1, 3), as_view(m2, 3)
        dt = _out32_dtype(out, m1, m2)
        if self.row_major:
            raise TypeError("Gemm.dispatch_out32*: the row-major operator surface has no f32-output form")
        check(lib.wg_gemm_out32(pass_._ctx.handle, int(variant), dt, float(alpha), float(beta),
                                out.buffer()._h, out.shape().to_c(), m1.buffer()._h, m1.shape().to_c(),
                                m2.buffer()._h, m2.shape().to_c()))

    def dispatch_q8_tr(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, out, m, scales, x, group_rows: int) -> None:
        self.dispatch_q8_generic(device, shapes, pass_, out, m, scales, x, group_rows, GemmVariant.GemmTr)

    def dispatch_q8_generic(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, out, m, scales, x, group_rows: int,
                            variant: GemmVariant = GemmVariant.GemmTr) -> None:
        """Extension (`wg_gemm_q8`): `Gemv.dispatch_q8_tr`'s int8 matrix and float32 group scales (`quantize_q8`'s layout, k x outputs) against float16 / bfloat16
        columns `x` (k x N) with a float32 `out` (outputs x N) = W^T x on the matrix cores. int8 is widened exactly, nothing is narrowed, the scale enters per
        group in f32. Only the transposed variants exist (Gemm / GemmFast are refused by the library). Column-major views only (the row-major surface has no q8
        form)."""
        out, m, scales, x = as_view(out, 3), as_view(m, 3), as_view(scales, 3), as_view(x, 3)
        xd = _gemm_q8_dtypes(out, m, scales, x)
        if self.row_major:
            raise TypeError("Gemm.dispatch_q8*: the row-major operator surface has no q8 form")
        check(lib.wg_gemm_q8(pass_._ctx.handle, int(variant), int(group_rows), xd,
                             out.buffer()._h, out.shape().to_c(), m.buffer()._h, m.shape().to_c(),
                             scales.buffer()._h, scales.shape().to_c(), x.buffer()._h, x.shape().to_c()))

    def dispatch_q8a8_tr(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, out, m, scales, x, x_scales, group_rows: int, x_group_rows: int) -> None:
        self.dispatch_q8a8_generic(device, shapes, pass_, out, m, scales, x, x_scales, group_rows, x_group_rows, GemmVariant.GemmTr)

    def dispatch_q8a8_generic(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, out, m, scales, x, x_scales, group_rows: int, x_group_rows: int,
                              variant: GemmVariant = GemmVariant.GemmTr) -> None:
        """Extension (`wg_gemm_q8a8`): `dispatch_q8_tr`'s int8 matrix and float32 group scales (k x outputs) against int8 columns `x` (k x N) with float32 group
        scales of their own (`x_scales`: ceil(k / x_group_rows) x N; `QuantizeQ8` makes both on the device), float32 `out` (outputs x N) = W^T X on the i8 matrix
        cores. Integer chains of at most 1024 rows are exact; the two scales enter per chain in f32. Only the transposed variants exist (Gemm / GemmFast are
        refused by the library). Column-major views only (the row-major surface has no q8a8 form)."""
        out, m, scales, x, x_scales = as_view(out, 3), as_view(m, 3), as_view(scales, 3), as_view(x, 3), as_view(x_scales, 3)
        _gemm_q8a8_dtypes(out, m, scales, x, x_scales)
        if self.row_major:
            raise TypeError("Gemm.dispatch_q8a8*: the row-major operator surface has no q8a8 form")
        check(lib.wg_gemm_q8a8(pass_._ctx.handle, int(variant), int(group_rows), int(x_group_rows),
                               out.buffer()._h, out.shape().to_c(), m.buffer()._h, m.shape().to_c(), scales.buffer()._h, scales.shape().to_c(),
                               x.buffer()._h, x.shape().to_c(), x_scales.buffer()._h, x_scales.shape().to_c()))

    def dispatch_q4_tr(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, out, m, scales, x, group_rows: int) -> None:
        self.dispatch_q4_generic(device, shapes, pass_, out, m, scales, x, group_rows, GemmVariant.GemmTr)

    def dispatch_q4_generic(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, out, m, scales, x, group_rows: int,
                            variant: GemmVariant = GemmVariant.GemmTr) -> None:
        """Extension (`wg_gemm_q4`): `Gemv.dispatch_q4_tr`'s uint8 matrix of packed 4-bit weights and float32 group scales (`pack_q4` / `quantize_q4`'s layout,
        k / 2 bytes x outputs) against float16 / bfloat16 columns `x` (k x N) with a float32 `out` (outputs x N) = W^T x on the matrix cores. A weight is unpacked
        exactly (q = n - 8), nothing is narrowed, the scale enters per group in f32. Only the transposed variants exist (Gemm / GemmFast are refused by the
        library). Column-major views only (the row-major surface has no q4 form)."""
        out, m, scales, x = as_view(out, 3), as_view(m, 3), as_view(scales, 3), as_view(x, 3)
        xd = _gemm_q4_dtypes(out, m, scales, x)
        if self.row_major:
            raise TypeError("Gemm.dispatch_q4*: the row-major operator surface has no q4 form")
        check(lib.wg_gemm_q4(pass_._ctx.handle, int(variant), int(group_rows), xd,
                             out.buffer()._h, out.shape().to_c(), m.buffer()._h, m.shape().to_c(),
                             scales.buffer()._h, scales.shape().to_c(), x.buffer()._h, x.shape().to_c()))


class Gemv:
    """gemv.rs:9-21."""

    def __init__(self, device=None, shader_defs=None):
        self.device = device
        self.row_major = _is_row_major(shader_defs)

    @staticmethod
    def from_device(device, shader_defs=None) -> "Gemv":
        return Gemv(device, shader_defs)

    def dispatch(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, out, m, v) -> None:
        self.dispatch_generic(device, shapes, pass_, out, m, v, GemvVariant.Gemv)

    def dispatch_tr(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, out, m, v) -> None:
        self.dispatch_generic(device, shapes, pass_, out, m, v, GemvVariant.GemvTr)

    def dispatch_generic(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, out, m, v, variant: GemvVariant) -> None:
        out, m, v = as_view(out, 3), as_view(m, 3), as_view(v, 3)
        dt = _common_dtype(out, m, v)
        fn = lib.wg_gemv_rm if self.row_major else lib.wg_gemv
        check(fn(pass_._ctx.handle, int(variant), dt,
                 out.buffer()._h, out.shape().to_c(), m.buffer()._h, m.shape().to_c(),
                 v.buffer()._h, v.shape().to_c()))

    def dispatch_mixed(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, out, m, v) -> None:
        self.dispatch_mixed_generic(device, shapes, pass_, out, m, v, GemvVariant.Gemv)

    def dispatch_mixed_tr(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, out, m, v) -> None:
        self.dispatch_mixed_generic(device, shapes, pass_, out, m, v, GemvVariant.GemvTr)

    def dispatch_mixed_generic(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, out, m, v, variant: GemvVariant) -> None:
        """Extension (`wg_gemv_mixed`): a float16 / bfloat16 matrix with float32 vectors and a float32 result -- 16-bit weights, f32 activations. The matrix is
        widened exactly, `v` is never narrowed, sums are f32 and the result is stored without a rounding step; a float32 matrix is `dispatch_generic`.
        Column-major views only (the row-major surface has no mixed form)."""
        out, m, v = as_view(out, 3), as_view(m, 3), as_view(v, 3)
        md = _mixed_dtype(out, m, v)
        if self.row_major:
            raise TypeError("Gemv.dispatch_mixed*: the row-major operator surface has no mixed-precision form")
        check(lib.wg_gemv_mixed(pass_._ctx.handle, int(variant), md,
                                out.buffer()._h, out.shape().to_c(), m.buffer()._h, m.shape().to_c(),
                                v.buffer()._h, v.shape().to_c()))


    def dispatch_q8(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, out, m, scales, v, group_rows: int) -> None:
        self.dispatch_q8_generic(device, shapes, pass_, out, m, scales, v, group_rows, GemvVariant.Gemv)

    def dispatch_q8_tr(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, out, m, scales, v, group_rows: int) -> None:
        self.dispatch_q8_generic(device, shapes, pass_, out, m, scales, v, group_rows, GemvVariant.GemvTr)

    def dispatch_q8_generic(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, out, m, scales, v, group_rows: int,
                            variant: GemvVariant = GemvVariant.Gemv) -> None:
        """Extension (`wg_gemv_q8`): an int8 matrix with one float32 scale per `group_rows` consecutive rows of a column (`quantize_q8`'s layout), float32 vectors
        and a float32 result: out = W v or W^T v with W = scales[r // group_rows, c] * m[r, c]. int8 is widened exactly, nothing is narrowed, sums are f32.
        Column-major views only (the row-major surface has no q8 form)."""
        out, m, scales, v = as_view(out, 3), as_view(m, 3), as_view(scales, 3), as_view(v, 3)
        _q8_dtypes(out, m, scales, v)
        if self.row_major:
            raise TypeError("Gemv.dispatch_q8*: the row-major operator surface has no q8 form")
        check(lib.wg_gemv_q8(pass_._ctx.handle, int(variant), int(group_rows),
                             out.buffer()._h, out.shape().to_c(), m.buffer()._h, m.shape().to_c(),
                             scales.buffer()._h, scales.shape().to_c(), v.buffer()._h, v.shape().to_c()))

    def dispatch_q4_tr(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, out, m, scales, v, group_rows: int) -> None:
        self.dispatch_q4_generic(device, shapes, pass_, out, m, scales, v, group_rows, GemvVariant.GemvTr)

    def dispatch_q4_generic(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, out, m, scales, v, group_rows: int,
                            variant: GemvVariant = GemvVariant.GemvTr) -> None:
        """Extension (`wg_gemv_q4`): a uint8 matrix of packed 4-bit weights (`pack_q4` / `quantize_q4`'s layout: k / 2 bytes x outputs) with one float32 scale per
        `group_rows` consecutive logical rows of a column, float32 vectors and a float32 result: out = W^T v with W = scales[r // group_rows, c] * q[r, c]. The
        nibbles are widened exactly, nothing is narrowed, sums are f32. Only the transposed variants exist (Gemv / GemvFast are refused by the library).
        Column-major views only (the row-major surface has no q4 form)."""
        out, m, scales, v = as_view(out, 3), as_view(m, 3), as_view(scales, 3), as_view(v, 3)
        _q4_dtypes(out, m, scales, v)
        if self.row_major:
            raise TypeError("Gemv.dispatch_q4*: the row-major operator surface has no q4 form")
        check(lib.wg_gemv_q4(pass_._ctx.handle, int(variant), int(group_rows),
                             out.buffer()._h, out.shape().to_c(), m.buffer()._h, m.shape().to_c(),
                             scales.buffer()._h, scales.shape().to_c(), v.buffer()._h, v.shape().to_c()))


def gemv_reduce(pass_: ComputePass, op: "ReduceOp", result: GpuTensor, m, v, variant: "GemvVariant" = None) -> None:
    """Extension: result = reduce(op, op(m) v) in one call (scratch vector owned by the context); bit-identical
    to Gemv.dispatch followed by Reduce.dispatch."""
    m, v = as_view(m, 3), as_view(v, 3)
    variant = GemvVariant.Gemv if variant is None else variant
    check(lib.wg_gemv_reduce(pass_._ctx.handle, int(variant), int(op), _common_dtype(m, v), result._h,
                             m.buffer()._h, m.shape().to_c(), v.buffer()._h, v.shape().to_c()))


class Reduce:
    """reduce.rs:62-113: `Reduce::new(device, op)` then `dispatch(device, shapes, pass, value, result)`."""

    def __init__(self, device, op: ReduceOp):
        self.device = device
        self.op = ReduceOp(op)

    @staticmethod
    def new(device, op: ReduceOp) -> "Reduce":
        return Reduce(device, op)

    def dispatch(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, value, result: GpuTensor) -> None:
        value = as_view(value, 1)
        check(lib.wg_reduce(pass_._ctx.handle, int(self.op), wg_dtype(value.dtype), value.buffer()._h, value.shape().to_c(),
                            result._h))

    def dispatch_fast(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, value, result: GpuTensor) -> None:
        """Extension: two-pass multi-workgroup reduce of one long vector at HBM speed. Min/Max: same bits as
        `dispatch`; Sum/Prod/SqNorm: re-associated (deterministic), within n * 2^-24 * sum|x| of the reference order."""
        value = as_view(value, 1)
        check(lib.wg_reduce_fast(pass_._ctx.handle, int(self.op), wg_dtype(value.dtype), value.buffer()._h, value.shape().to_c(),
                                 result._h))

    def dispatch_batched(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, values, results: GpuTensor) -> None:
        """Extension (one launch for every column of a matrix/cube view): results[c + t*ncols], each equal to what
        `dispatch` gives for that column."""
        values = as_view(values, 3)
        check(lib.wg_reduce_batched(pass_._ctx.handle, int(self.op), wg_dtype(values.dtype), values.buffer()._h,
                                    values.shape().to_c(), results._h))

    def eval_cpu(self, val: np.ndarray) -> np.float32:
        """reduce.rs:116-124 (`#[doc(hidden)]` test helper): what nalgebra computes, in NumPy."""
        val = np.asarray(val, np.float32)
        return {ReduceOp.Min: val.min, ReduceOp.Max: val.max, ReduceOp.Prod: val.prod, ReduceOp.Sum: val.sum,
                ReduceOp.SqNorm: lambda: (val * val).sum()}[self.op]()


class OpAssign:
    """op_assign.rs:43-95: `OpAssign::new(device, op)` then `dispatch(device, shapes, pass, in_out_a, in_b)`."""

    def __init__(self, device, op: OpAssignVariant):
        self.device = device
        self.op = OpAssignVariant(op)

    @staticmethod
    def new(device, op: OpAssignVariant) -> "OpAssign":
        return OpAssign(device, op)

    def dispatch(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, in_out_a, in_b) -> None:
        a, b = as_view(in_out_a, 1), as_view(in_b, 1)
        dt = _common_dtype(a, b)
        check(lib.wg_op_assign(pass_._ctx.handle, int(self.op), dt, a.buffer()._h, a.shape().to_c(), b.buffer()._h,
                               b.shape().to_c()))


class Axpy:
    """Extension: the BLAS axpy the north-star names; the reference only has OpAssign (no scalar).
    `dispatch(device, shapes, pass, alpha, in_out_y, in_x)`: y[i] = fma(alpha, x[i], y[i]).  alpha = +1 / -1 give the bits of
    OpAssignVariant.Add / Sub."""

    def __init__(self, device=None):
        self.device = device

    @staticmethod
    def from_device(device) -> "Axpy":
        return Axpy(device)

    def dispatch(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, alpha: float, in_out_y, in_x) -> None:
        y, x = as_view(in_out_y, 1), as_view(in_x, 1)
        dt = _common_dtype(y, x)
        check(lib.wg_axpy(pass_._ctx.handle, float(alpha), dt, y.buffer()._h, y.shape().to_c(), x.buffer()._h, x.shape().to_c()))


class CopyView:
    """Extension: `dispatch(device, shapes, pass, dst, src)`: the dst view = the src view where it has elements, 0 elsewhere; any offset,
    stride and length on either side (`wg_copy_view`). The aligned copy of an odd view, made once instead of inside every product."""

    def __init__(self, device=None):
        self.device = device

    @staticmethod
    def from_device(device) -> "CopyView":
        return CopyView(device)

    def dispatch(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, dst, src) -> None:
        d, s_ = as_view(dst, 3), as_view(src, 3)
        dt = _common_dtype(d, s_)
        check(lib.wg_copy_view(pass_._ctx.handle, dt, d.buffer()._h, d.shape().to_c(), s_.buffer()._h, s_.shape().to_c()))


class QuantizeQ8:
    """Extension (`wg_quantize_q8`): `dispatch(device, shapes, pass, q, scales, src, group_rows)`: the device-side `quantize_q8` -- int8 `q` and float32 `scales`
    (ceil(rows / group_rows) x cols) from a float32 / float16 / bfloat16 `src`, the NumPy helper's rule on the source widened exactly to float32 (a true division
    per element, ties to even, clamped to +-127; a group holding a NaN or an Inf gets the scale NaN and q = 0). Serves activations and weights alike."""

    def __init__(self, device=None):
        self.device = device

    @staticmethod
    def from_device(device) -> "QuantizeQ8":
        return QuantizeQ8(device)

    def dispatch(self, device, shapes: ViewShapeBuffers, pass_: ComputePass, q, scales, src, group_rows: int) -> None:
        q, scales, src = as_view(q, 3), as_view(scales, 3), as_view(src, 3)
        if np.dtype(q._tensor.dtype) != np.dtype(np.int8):
            raise TypeError(f"QuantizeQ8: `q` must be int8, got {q._tensor.dtype}")
        if np.dtype(scales._tensor.dtype) != np.dtype(np.float32):
            raise TypeError(f"QuantizeQ8: `scales` must be float32, got {scales._tensor.dtype}")
        sd = wg_dtype(src._tensor.dtype)  # (float32, float16 or bfloat16: every other element type is a TypeError there)
        check(lib.wg_quantize_q8(pass_._ctx.handle, sd, int(group_rows), q.buffer()._h, q.shape().to_c(), scales.buffer()._h, scales.shape().to_c(),
                                 src.buffer()._h, src.shape().to_c()))
