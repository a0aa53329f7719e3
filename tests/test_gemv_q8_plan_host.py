"""wg_gemv_q8's planner (wgmath_amd/csrc/gemv_q8_plan.hip) through wg_debug_gemv_q8_plan, without a device: a sweep over sizes, alignments, group_rows, right-hand sides
and CU counts. Every output and every contracted row is covered exactly once by the planned grid, every cut boundary is a multiple of 16, the streaming kernels are
planned only for views they can address and the element-by-element kernels for every other view, grid.z stays within 65535 or the plan is wg_gemv_mixed's refusal, and
the workspace is what the partials need."""
import ctypes
import itertools

import pytest

from wgmath_amd import _lib

LEAVES = _lib.GEMV_Q8_LEAVES
OUT_PER_BLOCK = {"t": 8, "n": 1024, "any_t": 1, "any_n": 256}  # a half-wave per column x 8; 64 lanes x 16 rows; a wave per column; a thread per row


def plan(**kw):
    q, p = _lib.GemvQ8QueryC(), _lib.GemvQ8PlanC()
    for k, v in kw.items():
        assert hasattr(q, k), k
        setattr(q, k, v)
    tags = ctypes.create_string_buffer(128)
    assert _lib.lib.wg_debug_gemv_q8_plan(ctypes.byref(q), ctypes.byref(p), tags, 128) == 0
    return q, p, tags.value.decode()


def query(tr, R, C, nrhs, mats, G, cus, mis=None):
    k, outs = (R, C) if tr else (C, R)
    kw = dict(trans=int(tr), rows=R, cols=C, nrhs=nrhs, mats=mats, group_rows=G, cus=cus, ldm=R, lds=max(-(-R // G), 1), ldv=k, ldo=outs, m_addr16=0, v_addr16=0, o_addr16=0)
    if mis == "ldm":
        kw["ldm"] = R + 3
    kw["m_batch"] = kw["ldm"] * C + (8 if mis == "m_batch" else 0)
    kw["s_batch"] = kw["lds"] * C
    if mis == "ldv":
        kw["ldv"] = k + 1
    kw["v_batch"] = kw["ldv"] * nrhs + (2 if mis == "v_batch" else 0)
    if mis == "ldo":
        kw["ldo"] = outs + 2
    kw["o_batch"] = kw["ldo"] * nrhs + (1 if mis == "o_batch" else 0)
    for f in ("m_addr16", "v_addr16", "o_addr16"):
        if mis == f:
            kw[f] = 1 if f == "m_addr16" else 4
    return kw


def streams(q):
    """What the 16-byte accesses need (include/wgebra_hip.h, restated)."""
    m_ok = q.rows and q.cols and q.rows % 16 == 0 and q.m_addr16 == 0 and (q.cols <= 1 or q.ldm % 16 == 0) and (q.mats <= 1 or q.m_batch % 16 == 0)
    v_ok = q.v_addr16 == 0 and (q.nrhs <= 1 or q.ldv % 4 == 0) and (q.mats <= 1 or q.v_batch % 4 == 0)  # float4 loads beside every piece: GemvTr
    o_ok = q.o_addr16 == 0 and (q.nrhs <= 1 or q.ldo % 4 == 0) and (q.mats <= 1 or q.o_batch % 4 == 0)  # float4 stores of a lane's 16 rows: Gemv
    return bool(m_ok and (v_ok if q.trans else o_ok))


def check(q, p, tags):
    outs, k = (q.cols, q.rows) if q.trans else (q.rows, q.cols)
    groups = -(-q.nrhs // 8)
    what = f"{'T' if q.trans else 'N'} {q.rows} x {q.cols} rhs {q.nrhs} mats {q.mats} G {q.group_rows} cus {q.cus}: {LEAVES[p.leaf]} '{tags}'"
    if not outs or not q.nrhs or not q.mats:
        assert LEAVES[p.leaf] == "nothing" and p.status == 0 and tags == "", what
        return None
    if q.mats * groups > 65535:
        assert LEAVES[p.leaf] == "unsupported" and p.status == _lib.WG_ERR_UNSUPPORTED and tags == "", what
        assert p.message.decode() == f"Gemv: nmats * ceil(nrhs/8) = {q.mats * groups} exceeds 65535", what  # (wg_gemv_mixed's message)
        return None
    leaf = LEAVES[p.leaf]
    want_fast = streams(q)
    assert leaf == (("t" if q.trans else "n") if want_fast else ("any_t" if q.trans else "any_n")), what
    assert tags.startswith("gemv_q8/"), what
    # outputs: block b owns [b * out_per_block, (b + 1) * out_per_block): every output once, no empty block
    assert p.cols == 1 or (p.cols == 4 and leaf == "t"), what  # 4 adjacent columns per half-wave: only where that still gives every CU a workgroup
    assert p.out_per_block == OUT_PER_BLOCK[leaf] * p.cols and p.block == (64 if leaf == "any_t" else 256), what
    if p.cols == 4:
        assert -(-outs // 32) * q.mats * groups * max(k // 4096, 1) >= q.cus, what
    assert (p.grid[0] - 1) * p.out_per_block < outs <= p.grid[0] * p.out_per_block, what
    # right-hand sides and matrices: groups of 8 on grid.z
    assert p.rhs_groups == groups and p.grid[2] == q.mats * groups <= 65535, what
    if want_fast:
        per_group = min(q.nrhs, 8)
        assert p.rhs_tile in (1, 2, 4, 8) and p.rhs_tile >= per_group and (p.rhs_tile == 1 or p.rhs_tile // 2 < per_group), what
    # the contraction: split s covers [s * k_per_split, min(k, (s + 1) * k_per_split)): every row once, no empty split, boundaries in multiples of 16
    assert p.nsplit >= 1 and p.grid[1] == p.nsplit <= 65535, what
    if k:
        assert (p.nsplit - 1) * p.k_per_split < k <= p.nsplit * p.k_per_split, what
    if p.nsplit > 1:
        assert want_fast and p.k_per_split % 16 == 0, what
        assert p.k_per_split % 512 == 0 and p.k_per_split >= 4096 if leaf == "t" else p.k_per_split >= 64, what  # whole chunks, a trip at least; 16 columns per wave
        assert p.grid[0] * p.grid[2] < (2 if leaf == "t" else 4) * q.cus, what  # only when the outputs cannot fill the chip (2 / 4 workgroups per CU)
        assert tags.endswith(f" gemv_q8/combine,ns={p.nsplit}"), what
    else:
        assert "combine" not in tags, what
    assert p.workspace_bytes == (4 * q.mats * p.nsplit * q.nrhs * outs if p.nsplit > 1 else 0), what
    return leaf


ROWS = [0, 16, 37, 496, 512, 528, 1024, 1040, 5168, 65536]
COLS = [0, 1, 7, 8, 9, 255, 4096, 8193]
MIS = [None, "ldm", "m_batch", "m_addr16", "ldv", "v_batch", "v_addr16", "ldo", "o_batch", "o_addr16"]


@pytest.mark.parametrize("tr", [False, True])
@pytest.mark.parametrize("cus", [8, 64, 100, 248, 256])
def test_sweep(tr, cus):
    seen = set()
    for R, C, nrhs, mats, G, mis in itertools.product(ROWS, COLS, [0, 1, 2, 3, 8, 11], [1, 2], [16, 32, 48, 128, 1 << 31], MIS):
        seen.add(check(*plan(**query(tr, R, C, nrhs, mats, G, cus, mis))))
    assert seen == {None, "t", "any_t"} if tr else seen == {None, "n", "any_n"}


def test_both_t_shapes_are_planned():
    assert plan(**query(True, 4096, 8193, 1, 1, 32, 256))[1].cols == 4 and plan(**query(True, 4096, 8193, 8, 1, 32, 256))[1].loads == 1
    assert plan(**query(True, 65536, 8, 1, 1, 32, 256))[1].cols == 1 and plan(**query(True, 4096, 4096, 1, 1, 32, 256))[1].cols == 1  # (128 workgroups of 32 columns)
    assert plan(**query(True, 65536, 4096, 1, 1, 32, 256))[1].cols == 4 and plan(**query(True, 11008, 4096, 1, 1, 32, 256))[1].cols == 4


def test_grid_z_limit_is_the_mixed_calls():
    q, p, tags = plan(**query(True, 512, 8, 1, 65536, 32, 256))
    assert check(q, p, tags) is None and LEAVES[p.leaf] == "unsupported"
    q, p, tags = plan(**query(False, 512, 8, 9, 32768, 32, 256))  # 32768 matrices x 2 groups of right-hand sides
    assert check(q, p, tags) is None and p.message.decode() == "Gemv: nmats * ceil(nrhs/8) = 65536 exceeds 65535"
    q, p, tags = plan(**query(False, 512, 8, 8, 65535, 32, 256))
    assert check(q, p, tags) == "n"


def test_the_plans_the_gpu_cases_pin():
    """The tags tests/_q8.py expects on 256 CUs are the planner's (the GPU test reads them from the launch log)."""
    import _q8
    for case in _q8.CASES:
        q, p, tags = plan(**case_query(case))
        check(q, p, tags)
        assert tags.split(" ")[0] == case[9], (case[0], tags)
        assert ("combine" in tags) == case[0].endswith("_split"), (case[0], tags)


def case_query(case, cus=256):
    """The query a call on the views tests/test_gpu_gemv_q8.py builds for a case fills."""
    name, tr, R, C, nrhs, Z, G, (moff, mpad, gap), voff, tag = case
    k, outs = (R, C) if tr else (C, R)
    ldm, ldv = R + mpad, k + (4 if voff else 0)
    return dict(trans=int(tr), rows=R, cols=C, nrhs=nrhs, mats=Z, group_rows=G, cus=cus, ldm=ldm, m_batch=ldm * C + gap, m_addr16=moff % 16, lds=-(-R // G),
                s_batch=-(-R // G) * C, ldv=ldv, v_batch=ldv * nrhs, v_addr16=4 * voff % 16, ldo=outs + (4 if voff else 0), o_batch=(outs + (4 if voff else 0)) * nrhs,
                o_addr16=4 * voff % 16)


def test_the_cut_cases_with_more_right_hand_sides_and_matrices():
    """The smallest shapes each cut leaf is cut at on 256 CUs: name -> (columns per half-wave, nsplit, k_per_split, grid). For T, one chunk of rows less, or (for
    the wide tile) one workgroup of outputs less, and the planner does not cut / does not take that tile. The dirtying problem covers every cut case's workspace, on
    256 and on the 248 CUs of the GPU test's masked context."""
    import _q8
    want = {"t_3rhs_split": (1, 2, 4096, (2, 2, 1)), "t_2mats_split": (1, 2, 4096, (2, 2, 2)), "t4_3rhs_split": (4, 2, 4096, (128, 2, 1)),
            "t4_2mats_split": (4, 2, 4096, (64, 2, 2)), "n_3rhs_split": (1, 5, 64, (1, 5, 1)), "n_2mats_split": (1, 3, 64, (2, 3, 2)),
            "t_split": (1, 16, 4096, (1, 16, 1)), "t4_split": (4, 2, 4096, (128, 2, 1)), "n_split": (1, 1024, 64, (1, 1024, 1))}
    cut = {c[0]: c for c in _q8.CASES if c[0].endswith("_split")}
    assert set(cut) == set(want)
    for name, (cols, ns, per, grid) in want.items():
        q, p, tags = plan(**case_query(cut[name]))
        assert check(q, p, tags) == name[0] and (p.cols, p.nsplit, p.k_per_split, tuple(p.grid)) == (cols, ns, per, grid), (name, p.cols, p.nsplit, p.k_per_split, tuple(p.grid))
        assert p.workspace_bytes == 4 * q.mats * ns * q.nrhs * (q.cols if q.trans else q.rows)
    for name in ("t_3rhs_split", "t_2mats_split", "t4_3rhs_split", "t4_2mats_split"):
        c = cut[name]
        assert plan(**case_query(c[:2] + (c[2] - 512,) + c[3:]))[1].nsplit == 1, name  # one chunk of rows less: below two floors, not cut
    for name in ("t4_3rhs_split", "t4_2mats_split"):
        c = cut[name]
        assert plan(**case_query(c[:3] + (c[3] - 32,) + c[4:]))[1].cols == 1, name  # one workgroup of outputs less: not every CU gets one, the narrow tile
    for cus in (256, 248):
        q, d, tags = plan(**case_query(_q8.DIRTY, cus))
        assert check(q, d, tags) == "n" and d.nsplit > 1 and (cus != 256 or tags.split(" ")[0] == _q8.DIRTY[9])
        for c in cut.values():
            outs, douts = (c[3] if c[1] else c[2]), _q8.DIRTY[2]
            assert d.workspace_bytes >= plan(**case_query(c, cus))[1].workspace_bytes and douts * _q8.DIRTY[4] != outs * c[4], (cus, c[0])


def test_null_arguments():
    assert _lib.lib.wg_debug_gemv_q8_plan(None, None, None, 0) == _lib.WG_ERR_INVALID_ARG
