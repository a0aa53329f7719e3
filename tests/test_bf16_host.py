"""WG_BF16 without a GPU: the enum value in the header and the binding, the package's float32 <-> bf16 conversions against the bit-level helper of the tests (and
torch's CPU conversion where torch imports), detached bf16 tensors, and the compiled bfloat16 Gemm units: each compiled alone to ISA like tests/test_abi_and_host.py
compiles the f16 ones -- v_mfma_f32_16x16x32_bf16 and no f16 MFMA, the same AGPR accounting of the continuous kernel, the same issue budget of the m16 main loop."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import _bf16 as B

import wgmath_amd as wg
from wgmath_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wgmath_amd", "csrc")


def _samples():
    rng = np.random.default_rng(20)
    u = rng.integers(0, 2 ** 32, 1 << 20, dtype=np.uint64).astype(np.uint32)
    u = u[(u & 0x7FFFFFFF) <= 0x7F800000]  # (NaNs apart)
    special = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1.1754942e-38, 9.18e-41, np.finfo(np.float32).max, np.finfo(np.float32).min,
                        3.3895314e38, 3.3961775e38, 3.40e38, -3.40e38, 1.0, -1.0], np.float32)
    # the 64 exact ties 1 + (2k + 1) 2^-8: RNE sends them to the even neighbour, truncation always down
    ties = (1.0 + (2.0 * np.arange(64) + 1.0) * 2.0 ** -8).astype(np.float32)
    return np.concatenate([u.view(np.float32), special, ties, -ties]), ties


def test_enum_value_in_binding_and_header():
    assert _lib.WG_BF16 == 2 and (_lib.WG_F32, _lib.WG_F16) == (0, 1)
    hdr = open(_lib.HEADER_PATH).read()
    assert re.search(r"\bWG_BF16\s*=\s*2\b", hdr)
    assert wg.wgcore.wg_dtype(wg.bfloat16) == 2 and wg.bfloat16.itemsize == 2
    assert wg.bfloat16 != np.dtype(np.float16) and wg.bfloat16 != np.dtype(np.uint16) and hash(wg.bfloat16) == hash(np.dtype(wg.bfloat16))
    with pytest.raises(TypeError, match="bf16"):
        wg.wgcore.wg_dtype(np.float64)


def test_to_bfloat16_is_one_rne_rounding():
    x, ties = _samples()
    got = wg.to_bfloat16(x)
    assert got.dtype == wg.bfloat16 and got.shape == x.shape
    assert np.array_equal(got.view(np.uint16), B.to_bits(x))
    # the ties: even neighbours (1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6 ...), which truncation misses for every second one
    tb = wg.to_bfloat16(ties).view(np.uint16)
    k = np.arange(64)
    assert np.array_equal(tb, (0x3F80 + k + (k & 1)).astype(np.uint16))
    assert not np.array_equal(tb, (ties.view(np.uint32) >> 16).astype(np.uint16))
    # NaN stays NaN (quiet), whatever its payload; the round trip of every bf16 pattern is the identity
    nans = np.array([0x7F800001, 0x7FC00000, 0xFF800001, 0x7FFFFFFF, 0x7F80FFFF], np.uint32).view(np.float32)
    nb = wg.to_bfloat16(nans).view(np.uint16)
    assert ((nb & 0x7FFF) > 0x7F80).all() and (nb & 0x0040).all() and np.array_equal(nb, B.to_bits(nans))
    every = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    f = wg.from_bfloat16(every.view(wg.bfloat16))
    assert f.dtype == np.float32 and np.array_equal(f.view(np.uint32), every.astype(np.uint32) << 16)
    assert np.array_equal(wg.to_bfloat16(f).view(np.uint16) | np.where(np.isnan(f), 0x0040, 0).astype(np.uint16), every | np.where(np.isnan(f), 0x0040, 0).astype(np.uint16))
    assert np.array_equal(B.from_bits(every).view(np.uint32), f.view(np.uint32))
    with pytest.raises(TypeError):
        wg.from_bfloat16(np.zeros(3, np.float16))


def test_to_bfloat16_equals_torch_cpu(tmp_path):
    """torch's CPU conversion, in a child process: torch brings a HIP runtime of its own, which must not be loaded into this process after the library's."""
    x, _ = _samples()
    np.save(tmp_path / "x.npy", x)
    code = ("import sys, numpy as np\n"
            "try:\n    import torch\nexcept Exception:\n    sys.exit(3)\n"
            "x = np.load(sys.argv[1])\n"
            "np.save(sys.argv[2], torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))\n")
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path / "x.npy"), str(tmp_path / "t.npy")], capture_output=True, text=True)
    if r.returncode == 3:  # (the conversion is pinned by the bit-level helper either way; the report says that this comparison did not run)
        pytest.skip("torch does not import here")
    assert r.returncode == 0, r.stderr
    t = np.load(tmp_path / "t.npy")
    assert np.array_equal(wg.to_bfloat16(x).view(np.uint16), t)
    assert np.array_equal(B.to_bits(x), t)


def test_detached_bf16_tensors():
    class _C:  # no context: the tensor object alone (its handle is never used)
        handle = None
    t = wg.GpuTensor(_C(), 0, (5, 7), wg.bfloat16)
    assert t.len() == 35 and t.bytes_len() == 2 * t.len() and t.dtype == wg.bfloat16
    assert t.as_view().dtype == wg.bfloat16 and t.columns(1, 2).shape().size == (5, 2, 1)


# ---- the compiled units --------------------------------------------------------------------------------------------------------------------------
_ISA = {}


def _isa(source):
    if source not in _ISA:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        if not os.path.exists(hipcc):
            pytest.skip("hipcc not available")
        with tempfile.TemporaryDirectory() as td:
            out = os.path.join(td, "k.s")
            subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-ffp-contract=on",
                            "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-S", "--cuda-device-only", os.path.join(CSRC, source), "-o", out], check=True, capture_output=True)
            _ISA[source] = open(out).read()
    return _ISA[source]


def _kernels(text, kernel):
    return re.findall(r"^(_Z\S*" + kernel + r"\w*):[^\n]*\n(.*?)^\.Lfunc_end", text, flags=re.S | re.M)


# unit, kernel name, instances (the f16 unit's count), bf16 MFMAs expected (the generic fallback multiplies on the vector ALU: none of either kind)
UNITS = [("gemm_bf16.hip", "gemm_bf16_m16_kernel", 2, True), ("gemm_bf16.hip", "gemm_bf16_m16c_kernel", 8, True), ("gemm_bf16.hip", "gemm_bf16_tail_reduce", 1, False),
         ("gemm_bf16_t128.hip", "gemm_bf16_t128_kernel", 6, True), ("gemm_bf16_nt.hip", "gemm_bf16_nt_kernel", 1, True),
         ("gemm_bf16_generic.hip", "gemm_bf16_generic_kernel", 2, False), ("gemm_bf16_skinny.hip", "gemm_bf16_skinny_kernel", 1, True)]


@pytest.mark.parametrize("source,kernel,instances,mfma", UNITS)
def test_bf16_units_multiply_in_bf16_only(source, kernel, instances, mfma):
    text = _isa(source)
    assert "v_mfma_f32_16x16x32_f16" not in text and not re.search(r"v_cvt_f16_f32|v_cvt_f32_f16|v_cvt_pk_f16|v_cvt_pkrtz", text), f"{source}: f16 code in the bf16 unit"
    assert not re.search(r"gemm_f16_|gemm_f32_skinny_kernel", text), f"{source}: a kernel under an f16 unit's name"
    ks = _kernels(text, kernel)
    assert len(ks) == instances, [k for k, _ in ks]
    for name, body in ks:
        if mfma:
            assert "v_mfma_f32_16x16x32_bf16" in body, name
        assert "v_cvt_pk_bf16_f32" in body, f"{name}: the store does not round with v_cvt_pk_bf16_f32"
        if mfma and "Inner Loop Header" in body and kernel != "gemm_bf16_m16_kernel":  # (that kernel's main loop: the issue-budget test below)
            loop = body[body.index("Inner Loop Header"):]
            assert "scratch_" not in loop[:loop.index("s_cbranch_scc1")], f"{name}: register spills inside the main loop"
        m0 = [l.strip() for l in body.splitlines() if re.search(r"\bm0\b", l) and not l.strip().startswith(";")]
        assert all(re.fullmatch(r"s_mov_b32 m0, s\d+", l) for l in m0), f"{name}: M0 used outside the LDS-DMA asm"


def test_bf16_continuous_kernel_accumulators_are_the_named_agprs():
    """The accounting of tests/test_abi_and_host.py::test_f16_continuous_kernel_accumulators_are_the_named_agprs on the bf16 build: 256 MFMAs (bf16) and 256 reads, all
    inside our asm, no compiler AGPR use, no scratch, all 256 AGPRs in the kernel descriptor, M0 only ours."""
    kernels = _kernels(_isa("gemm_bf16.hip"), "gemm_bf16_m16c_kernel")
    assert len(kernels) == 8, [k for k, _ in kernels]
    for name, whole in kernels:
        body, desc = whole.split(".amdhsa_kernel")
        assert "scratch_" not in body, f"{name}: register spills"
        inside, ours, theirs = False, [], []
        for l in (x.strip() for x in body.splitlines()):
            if l.startswith(";;#ASMSTART"):
                inside = True
            elif l.startswith(";;#ASMEND"):
                inside = False
            elif re.match(r"v_mfma|v_accvgpr", l) or re.search(r"\ba\[?\d", l):
                (ours if inside else theirs).append(l)
        assert not theirs, f"{name}: the compiler touches AGPRs: {theirs[:4]}"
        count = lambda pat: sum(1 for l in ours if l.startswith(pat))
        assert (count("v_mfma_f32_16x16x32_bf16"), count("v_accvgpr_write_b32"), count("v_accvgpr_read_b32"), count("v_accvgpr_mov")) == (256, 0, 256, 0)
        m0 = [l.strip() for l in body.splitlines() if re.search(r"\bm0\b", l) and not l.strip().startswith(";")]
        assert m0 and all(re.fullmatch(r"s_mov_b32 m0, s\d+", l) for l in m0), f"{name}: M0 used outside the LDS-DMA asm"
        nv, off = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1)), int(re.search(r"\.amdhsa_accum_offset (\d+)", desc).group(1))
        assert nv - off == 256 and nv <= 512, (nv, off)


@pytest.mark.parametrize("which", ["ILb0", "ILb1"])  # NN, TN
def test_bf16_gemm_main_loop_issue_budget(which):
    """tests/test_abi_and_host.py::test_f16_gemm_main_loop_issue_budget, same budget, on gemm_bf16_m16_kernel."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gap_hist
    r = gap_hist.analyse(_isa("gemm_bf16.hip"), which, kernel="gemm_bf16_m16_kernel")
    assert r["loop_mfma"] == 128 and r["mfma_total"] == 128, (r["loops"], r["loop_mfma"], r["mfma_total"])
    assert r["loop_acc_moves"] == 0 and r["loop_scratch"] == 0, (r["loop_acc_moves"], r["loop_scratch"])
    over = [(i, g) for i, g in enumerate(r["gaps"]) if len(g) > 3]
    assert not over, f"gaps with more than 3 fillers: {over[:4]}"


def test_bf16_instances_of_the_templated_units():
    """Gemv, Reduce, OpAssign and the split-K reduce carry bf16 instances (DF16b in the mangled names) that round with v_cvt_pk_bf16_f32."""
    for source, kernel in (("gemv.hip", "gemv_n_kernel"), ("gemv_any.hip", "gemv_any"), ("reduce.hip", "reduce_rows4"), ("op_assign.hip", "op_assign_f16_vec"),
                           ("splitk.hip", "splitk_reduce_kernel")):
        ks = [(n, b) for n, b in _kernels(_isa(source), kernel) if "DF16b" in n]
        assert ks, f"{source}: no bf16 instance of {kernel}"
        assert any("v_cvt_pk_bf16_f32" in b for _, b in ks), f"{source}: no bf16 instance rounds with v_cvt_pk_bf16_f32"


def test_no_new_undeclared_exports():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if " T " in line}
    leaked = [n for n in names if (n.startswith("wg_") or "bf16" in n) and n not in set(_lib.declared_symbols()) and not n.startswith("_Z")]
    assert not leaked, f"undeclared exports: {leaked}"
    assert _lib.lib.wg_abi_version() == 5
