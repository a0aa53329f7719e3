"""bfloat16 on the test side: float32 -> bf16 bits (ONE round-to-nearest-even) and back, at the bit level and independent of the package's own helper.

    bits = (u + 0x7FFF + ((u >> 16) & 1)) >> 16      on the uint32 view u of the float32 (a NaN is handled apart: it keeps its sign and high payload bits, quiet bit set)

Checked against torch.bfloat16 on the CPU on 2^20 random magnitudes plus +-0, +-Inf, subnormals and the largest finite value: identical bits
(tests/test_bf16_host.py repeats the comparison where torch imports)."""
import numpy as np


def to_bits(x) -> np.ndarray:
    """float array -> uint16 bf16 bit patterns of the same shape (values are taken to float32 first)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, (u >> 16) | 0x0040, r).astype(np.uint16)


def from_bits(bits) -> np.ndarray:
    """uint16 bf16 bit patterns -> float32, exactly."""
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def round_f32(x) -> np.ndarray:
    """float array -> the float32 values of its bf16 roundings."""
    return from_bits(to_bits(x))
