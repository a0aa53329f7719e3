"""wg_gemv_q4's planner (wgmath_amd/csrc/gemv_q4_plan.hip) through wg_debug_gemv_q4_plan, without a device: a sweep over sizes, alignments, group_rows, right-hand
sides, matrices and CU counts. The streaming leaf is taken exactly for the views it can address and the element-by-element kernel for every other one; every output
and every logical row is covered exactly once by the planned grid; no split is empty; every cut boundary is a multiple of 32 logical rows and of the 16-weight piece,
so that with group_rows % 32 == 0 a piece never straddles a group; grid and workspace follow from the plan; out = W v comes back UNSUPPORTED with the message that
names wg_gemv_q8; the tags are the plan's."""
import ctypes
import itertools

import pytest

from wgmath_amd import _lib

LEAVES = _lib.GEMV_Q4_LEAVES
N_MESSAGE = "Gemv: wg_gemv_q4 computes out = W^T v only (WG_GEMV_TR); wg_gemv_q8 computes out = W v, on int8 weights"


def plan(**kw):
    q, p = _lib.GemvQ4QueryC(), _lib.GemvQ4PlanC()
    for k, v in kw.items():
        assert hasattr(q, k), k
        setattr(q, k, v)
    tags = ctypes.create_string_buffer(128)
    assert _lib.lib.wg_debug_gemv_q4_plan(ctypes.byref(q), ctypes.byref(p), tags, 128) == 0
    return q, p, tags.value.decode()


def query(RB, C, nrhs, mats, G, cus, mis=None, trans=1):
    """RB: rows of BYTES; the contraction has k = 2 RB logical rows."""
    k = 2 * RB
    kw = dict(trans=trans, rows=RB, cols=C, nrhs=nrhs, mats=mats, group_rows=G, cus=cus, ldm=RB, lds=max(-(-k // G), 1), ldv=k, ldo=C, m_addr16=0, v_addr16=0)
    if mis == "ldm":
        kw["ldm"] = RB + 3
    kw["m_batch"] = kw["ldm"] * C + (8 if mis == "m_batch" else 0)
    kw["s_batch"] = kw["lds"] * C
    if mis == "ldv":
        kw["ldv"] = k + 1
    kw["v_batch"] = kw["ldv"] * nrhs + (2 if mis == "v_batch" else 0)
    if mis == "ldo":  # (`out` is stored one float at a time: no alignment of it decides anything)
        kw["ldo"] = C + 1
    kw["o_batch"] = kw["ldo"] * nrhs + (1 if mis == "ldo" else 0)
    if mis == "m_addr16":
        kw["m_addr16"] = 1
    if mis == "v_addr16":
        kw["v_addr16"] = 4
    return kw


def streams(q):
    """What the 16-byte accesses need (include/wgebra_hip.h, restated): whole 16-byte loads of the matrix at 16-byte addresses, float4 loads of v."""
    m_ok = q.rows and q.cols and q.rows % 16 == 0 and q.m_addr16 == 0 and (q.cols <= 1 or q.ldm % 16 == 0) and (q.mats <= 1 or q.m_batch % 16 == 0)
    v_ok = q.v_addr16 == 0 and (q.nrhs <= 1 or q.ldv % 4 == 0) and (q.mats <= 1 or q.v_batch % 4 == 0)
    return bool(m_ok and v_ok)


def check(q, p, tags):
    outs, k = q.cols, 2 * q.rows
    groups = -(-q.nrhs // 8)
    what = f"{q.rows} bytes x {q.cols} rhs {q.nrhs} mats {q.mats} G {q.group_rows} cus {q.cus}: {LEAVES[p.leaf]} '{tags}'"
    if not q.trans:
        assert LEAVES[p.leaf] == "unsupported" and p.status == _lib.WG_ERR_UNSUPPORTED and tags == "" and p.message.decode() == N_MESSAGE, what
        return "refused"
    if not outs or not q.nrhs or not q.mats:
        assert LEAVES[p.leaf] == "nothing" and p.status == 0 and tags == "", what
        return None
    if q.mats * groups > 65535:
        assert LEAVES[p.leaf] == "unsupported" and p.status == _lib.WG_ERR_UNSUPPORTED and tags == "", what
        assert p.message.decode() == f"Gemv: nmats * ceil(nrhs/8) = {q.mats * groups} exceeds 65535", what  # (wg_gemv_q8's message)
        return None
    leaf = LEAVES[p.leaf]
    assert leaf == ("t" if streams(q) else "any_t"), what
    # outputs: block b owns [b * out_per_block, (b + 1) * out_per_block): every output once, no empty block
    assert p.cols == 1 or (p.cols == 4 and leaf == "t"), what  # 4 adjacent columns per half-wave: only where that still gives every CU a workgroup
    assert p.out_per_block == (8 * p.cols if leaf == "t" else 1) and p.block == (256 if leaf == "t" else 64), what
    if leaf == "t":
        assert (p.cols == 4) == (-(-outs // 32) * q.mats * groups * max(k // 8192, 1) >= q.cus), what  # the larger form wherever the columns allow it
        assert p.loads * p.cols == (8 if p.rhs_tile <= 2 else 4), what
        per_group = min(q.nrhs, 8)
        assert p.rhs_tile in (1, 2, 4, 8) and p.rhs_tile >= per_group and (p.rhs_tile == 1 or p.rhs_tile // 2 < per_group), what
    assert (p.grid[0] - 1) * p.out_per_block < outs <= p.grid[0] * p.out_per_block, what
    # right-hand sides and matrices: groups of 8 on grid.z
    assert p.rhs_groups == groups and p.grid[2] == q.mats * groups <= 65535, what
    # the contraction: split s covers logical rows [s * k_per_split, min(k, (s + 1) * k_per_split)): every row once, no empty split
    assert p.nsplit >= 1 and p.grid[1] == p.nsplit <= 65535, what
    if k:
        assert (p.nsplit - 1) * p.k_per_split < k <= p.nsplit * p.k_per_split, what
    if p.nsplit > 1:
        assert leaf == "t", what
        assert p.k_per_split % 32 == 0 and p.k_per_split % 16 == 0, what  # whole loads, whole pieces: with G % 32 == 0 (or one group) a piece never straddles a group
        if q.group_rows < k:
            assert q.group_rows % 32 == 0  # (the sweep only asks what the front-end lets through)
            for b in range(p.k_per_split, k, p.k_per_split):  # a boundary falls on a group's edge or on a piece's edge inside it
                assert b % q.group_rows == 0 or (b % q.group_rows) % 16 == 0, what
        assert p.k_per_split % 1024 == 0 and p.k_per_split >= 8192, what  # whole chunks, 8 of them at least
        assert p.grid[0] * p.grid[2] < 2 * q.cus, what  # only when the outputs cannot fill the chip (2 workgroups per CU)
        assert tags.endswith(f" gemv_q4/combine,ns={p.nsplit}"), what
    else:
        assert "combine" not in tags, what
    assert p.workspace_bytes == (4 * q.mats * p.nsplit * q.nrhs * outs if p.nsplit > 1 else 0), what
    # the tags are the plan's
    first = f"gemv_q4/t,nr={p.rhs_tile},u={p.loads},c={p.cols},ns={p.nsplit}" if leaf == "t" else "gemv_q4/any_t"
    assert tags.split(" ")[0] == first and len(tags.split(" ")) == (2 if p.nsplit > 1 else 1), what
    return leaf


ROWS_B = [0, 16, 37, 104, 496, 512, 528, 1024, 1040, 5168, 32768, 65536]
COLS = [0, 1, 7, 8, 9, 255, 4096, 8193, 11008]
MIS = [None, "ldm", "m_batch", "m_addr16", "ldv", "v_batch", "v_addr16", "ldo"]


@pytest.mark.parametrize("cus", [8, 64, 100, 248, 256])
def test_sweep(cus):
    seen, cut, wide = set(), 0, 0
    for RB, C, nrhs, mats, G, mis in itertools.product(ROWS_B, COLS, [0, 1, 2, 3, 8, 11], [1, 2], [32, 96, 128, 1 << 31], MIS):
        q, p, tags = plan(**query(RB, C, nrhs, mats, G, cus, mis))
        seen.add(check(q, p, tags))
        cut += p.nsplit > 1
        wide += p.cols == 4
    assert seen == {None, "t", "any_t"} and cut and wide


def test_out_equals_w_v_is_refused_by_the_plan():
    for RB, C, nrhs in ((512, 8, 1), (0, 0, 0), (37, 5, 2)):
        q, p, tags = plan(**query(RB, C, nrhs, 1, 32, 256, trans=0))
        assert check(q, p, tags) == "refused" and "wg_gemv_q8" in p.message.decode()


def test_both_t_shapes_are_planned():
    assert plan(**query(2048, 8193, 1, 1, 32, 256))[1].cols == 4 and plan(**query(2048, 8193, 8, 1, 32, 256))[1].loads == 1
    assert plan(**query(32768, 8, 1, 1, 32, 256))[1].cols == 1 and plan(**query(2048, 4096, 1, 1, 32, 256))[1].cols == 1  # (128 workgroups of 32 columns)
    # the decode shapes of tools/gemv_q4_vs.py (k x outputs): 65536 x 4096, 11008 x 4096, 4096 x 11008
    assert plan(**query(32768, 4096, 1, 1, 32, 256))[1].cols == 4 and plan(**query(5504, 4096, 1, 1, 32, 256))[1].cols == 1
    assert plan(**query(2048, 11008, 1, 1, 32, 256))[1].cols == 4


def test_grid_z_limit_is_the_q8_calls():
    q, p, tags = plan(**query(512, 8, 1, 65536, 32, 256))
    assert check(q, p, tags) is None and LEAVES[p.leaf] == "unsupported"
    q, p, tags = plan(**query(512, 8, 9, 32768, 32, 256))  # 32768 matrices x 2 groups of right-hand sides
    assert check(q, p, tags) is None and p.message.decode() == "Gemv: nmats * ceil(nrhs/8) = 65536 exceeds 65535"
    q, p, tags = plan(**query(512, 8, 8, 65535, 32, 256))
    assert check(q, p, tags) == "t"


def test_the_plans_the_gpu_cases_pin():
    """The tags tests/_q4.py expects on 256 CUs are the planner's (the GPU test reads them from the launch log)."""
    import _q4
    for case in _q4.CASES:
        name, tag = case[0], case[8]
        q, p, tags = plan(**case_query(case))
        check(q, p, tags)
        assert tags.split(" ")[0] == tag, (name, tags)
        assert ("combine" in tags) == name.endswith("_split"), (name, tags)


def case_query(case, cus=256):
    """The query a call on the views tests/test_gpu_gemv_q4.py builds for a case fills."""
    name, k, C, nrhs, Z, G, (moff, mpad, gap), voff, tag = case
    RB = k // 2
    ldm, ldv = RB + mpad, k + (4 if voff else 0)
    return dict(trans=1, rows=RB, cols=C, nrhs=nrhs, mats=Z, group_rows=G, cus=cus, ldm=ldm, m_batch=ldm * C + gap, m_addr16=moff % 16, lds=-(-k // G),
                s_batch=-(-k // G) * C, ldv=ldv, v_batch=ldv * nrhs, v_addr16=4 * voff % 16, ldo=C + (4 if voff else 0), o_batch=(C + (4 if voff else 0)) * nrhs)


def test_the_cut_cases_with_more_right_hand_sides_and_matrices():
    """The smallest shapes either tile is cut at on 256 CUs: name -> (columns per half-wave, nsplit, k_per_split, grid). One row of 8192 less, or (for the wide tile)
    one workgroup of outputs less, and the planner does not cut / does not take that tile. The dirtying problem covers every cut case's workspace, on 256 and on the
    248 CUs of the GPU test's masked context."""
    import _q4
    want = {"t_3rhs_split": (1, 2, 8192, (2, 2, 1)), "t_2mats_split": (1, 2, 8192, (2, 2, 2)), "t4_3rhs_split": (4, 2, 8192, (128, 2, 1)),
            "t4_2mats_split": (4, 2, 8192, (64, 2, 2)), "t_split": (1, 8, 8192, (1, 8, 1)), "t4_split": (4, 2, 8192, (128, 2, 1))}
    cut = {c[0]: c for c in _q4.CASES if c[0].endswith("_split")}
    assert set(cut) == set(want)
    for name, (cols, ns, per, grid) in want.items():
        q, p, tags = plan(**case_query(cut[name]))
        assert check(q, p, tags) == "t" and (p.cols, p.nsplit, p.k_per_split, tuple(p.grid)) == (cols, ns, per, grid), (name, p.cols, p.nsplit, p.k_per_split, tuple(p.grid))
        assert p.workspace_bytes == 4 * q.mats * ns * q.nrhs * q.cols
    for name in ("t_3rhs_split", "t_2mats_split", "t4_3rhs_split", "t4_2mats_split"):
        c = cut[name]
        assert plan(**case_query(c[:1] + (c[1] - 1024,) + c[2:]))[1].nsplit == 1, name  # one chunk of rows less: below two floors, not cut
    for name in ("t4_3rhs_split", "t4_2mats_split"):
        c = cut[name]
        assert plan(**case_query(c[:2] + (c[2] - 32,) + c[3:]))[1].cols == 1, name  # one workgroup of outputs less: not every CU gets one, the narrow tile
    for cus in (256, 248):
        q, d, tags = plan(**case_query(_q4.DIRTY, cus))
        assert check(q, d, tags) == "t" and d.nsplit > 1 and (cus != 256 or tags.split(" ")[0] == _q4.DIRTY[8])
        for c in cut.values():
            assert d.workspace_bytes >= plan(**case_query(c, cus))[1].workspace_bytes and _q4.DIRTY[2] * _q4.DIRTY[3] != c[2] * c[3], (cus, c[0])


def test_null_arguments():
    assert _lib.lib.wg_debug_gemv_q4_plan(None, None, None, 0) == _lib.WG_ERR_INVALID_ARG
