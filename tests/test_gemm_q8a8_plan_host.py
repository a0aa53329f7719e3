"""wg_gemm_q8a8's planner (wgmath_amd/csrc/gemm_q8a8_plan.hip) through wg_debug_gemm_q8a8_plan, without a device: a sweep over k, outputs, N, both group sizes,
alignments and CU counts. The planned grid covers every output, column and contracted row exactly once, no split is empty, every cut boundary is a CHAIN boundary
(tests/_gemm_q8a8.py restates the chains), the MFMA leaf is planned only for views it can address and the element-by-element kernel for every other view, grid.z stays
within 65535 or the plan is a refusal, the workspace is what the partials need -- and the tags the GPU test asserts are the planner's."""
import ctypes
import itertools

import pytest

import _gemm_q8a8 as GA
from wgmath_amd import _lib

LEAVES = _lib.GEMM_Q8A8_LEAVES
W = 1 << 31


def plan(**kw):
    q, p = _lib.GemmQ8A8QueryC(), _lib.GemmQ8A8PlanC()
    for k, v in kw.items():
        assert hasattr(q, k), k
        setattr(q, k, v)
    tags = ctypes.create_string_buffer(128)
    assert _lib.lib.wg_debug_gemm_q8a8_plan(ctypes.byref(q), ctypes.byref(p), tags, 128) == 0
    return q, p, tags.value.decode()


def query(k, outs, n, mats, G, Gx, cus, mis=None):
    kw = dict(k=k, outputs=outs, n=n, mats=mats, group_rows=G, x_group_rows=Gx, cus=cus, ldm=k, lds=max(-(-k // G), 1), ldx=k, ldxs=max(-(-k // Gx), 1), ldo=outs,
              m_addr16=0, x_addr16=0, o_addr16=0)
    if mis == "ldm":
        kw["ldm"] = k + 3
    kw["m_batch"] = kw["ldm"] * outs + (8 if mis == "m_batch" else 0)
    kw["s_batch"] = kw["lds"] * outs
    if mis == "ldx":
        kw["ldx"] = k + 8
    kw["x_batch"] = kw["ldx"] * n + (4 if mis == "x_batch" else 0)
    kw["xs_batch"] = kw["ldxs"] * n + (1 if mis == "xs_batch" else 0)
    if mis == "ldo":
        kw["ldo"] = outs + 3
    kw["o_batch"] = kw["ldo"] * n + (1 if mis == "o_batch" else 0)
    if mis == "m_addr16":
        kw["m_addr16"] = 1
    if mis == "x_addr16":
        kw["x_addr16"] = 8
    if mis == "o_addr16":
        kw["o_addr16"] = 4
    return kw


def streams(q):
    """What the MFMA leaf takes (include/wgebra_hip.h, restated): whole 32-row steps that never straddle a group of either side, 16-byte loads of m and of x."""
    k_ok = q.k and q.k % 32 == 0 and (q.group_rows % 32 == 0 or q.group_rows >= q.k) and (q.x_group_rows % 32 == 0 or q.x_group_rows >= q.k)
    m_ok = q.m_addr16 == 0 and (q.outputs <= 1 or q.ldm % 16 == 0) and (q.mats <= 1 or q.m_batch % 16 == 0)
    x_ok = q.x_addr16 == 0 and (q.n <= 1 or q.ldx % 16 == 0) and (q.mats <= 1 or q.x_batch % 16 == 0)
    return bool(k_ok and m_ok and x_ok)  # (the scales and out: any 4-byte-aligned view)


def is_chain_boundary(r, k, G, Gx):
    """r is a multiple of the finer group's size plus a multiple of 1024 inside that group (or k itself)."""
    fine = min(min(G, k), min(Gx, k))
    return r == k or (r % fine) % GA.CHAIN == 0


def check(q, p, tags):
    what = f"k {q.k} outs {q.outputs} n {q.n} mats {q.mats} G {q.group_rows} Gx {q.x_group_rows} cus {q.cus}: {LEAVES[p.leaf]} '{tags}'"
    if not q.outputs or not q.n or not q.mats:
        assert LEAVES[p.leaf] == "nothing" and p.status == 0 and tags == "", what
        return None
    fast = streams(q)
    passes = -(-q.n // (32 if q.n <= 32 else 64)) if fast else 1
    if q.mats * passes > 65535:
        assert LEAVES[p.leaf] == "unsupported" and p.status == _lib.WG_ERR_UNSUPPORTED and tags == "", what
        assert p.message.decode() == (f"Gemm: nmats * column passes = {q.mats * passes} exceeds 65535" if fast else f"Gemm: nmats = {q.mats} exceeds 65535"), what
        return None
    leaf = LEAVES[p.leaf]
    assert leaf == ("mfma" if fast else "any"), what
    assert p.nsplit >= 1 and p.grid[1] == p.nsplit <= 65535, what
    if q.k:
        assert (p.nsplit - 1) * p.k_per_split < q.k <= p.nsplit * p.k_per_split, what  # every row once, no empty split
    assert (p.grid[0] - 1) * p.out_per_block < q.outputs <= p.grid[0] * p.out_per_block, what  # every output once, no empty block
    if leaf == "any":
        assert tags == "gemm_q8a8/any" and p.nsplit == 1 and p.workspace_bytes == 0 and p.block == 64 and p.out_per_block == 1, what
        assert (p.col_tiles, p.col_passes) == (0, 1) and tuple(p.grid) == (q.outputs, 1, q.mats), what
        return leaf
    assert p.col_tiles == (2 if q.n <= 32 else 4) and p.col_passes == passes, what
    assert (p.col_passes - 1) * 16 * p.col_tiles < q.n <= p.col_passes * 16 * p.col_tiles, what  # every column once, no empty pass
    assert p.out_per_block == GA.BLOCK_OUT and p.block == 256 and p.grid[2] == q.mats * p.col_passes <= 65535, what
    assert tags.split(" ")[0] == f"gemm_q8a8/mfma,nt={p.col_tiles},ns={p.nsplit}", what
    if p.nsplit > 1:
        assert p.k_per_split % 32 == 0 and p.k_per_split >= 512, what
        for G in (q.group_rows, q.x_group_rows):
            if G < q.k:
                assert p.k_per_split % G == 0, what  # a group of either side is never cut
        if q.group_rows >= q.k and q.x_group_rows >= q.k:
            assert p.k_per_split % GA.CHAIN == 0, what
        # every cut boundary is a chain boundary (boundaries are multiples of k_per_split: the first few and the last say it for all of them)
        for i in sorted(set(list(range(1, min(p.nsplit, 6))) + [p.nsplit - 1])):
            assert is_chain_boundary(i * p.k_per_split, q.k, q.group_rows, q.x_group_rows), (what, i)
        assert p.grid[0] * p.grid[2] < 4 * q.cus, what  # only when outputs x passes cannot fill the chip
        assert q.n <= 65535 and tags.endswith(f" gemm_q8a8/combine,ns={p.nsplit}"), what
    else:
        assert "combine" not in tags and p.k_per_split == q.k, what
    assert p.workspace_bytes == (4 * q.mats * p.nsplit * q.n * q.outputs if p.nsplit > 1 else 0), what
    return leaf


KS = [0, 16, 32, 37, 48, 64, 544, 4096, 11008, 65536, 131104]
OUTS = [0, 1, 17, 128, 129, 4096]
NS = [0, 1, 16, 32, 33, 65, 130]
GROUPS = [(16, 16), (32, 32), (48, 96), (96, 32), (128, W), (W, 32), (64, 128), (1536, W), (W, W)]
MIS = [None, "ldm", "m_batch", "m_addr16", "ldx", "x_batch", "x_addr16", "xs_batch", "ldo", "o_batch", "o_addr16"]


@pytest.mark.parametrize("cus", [8, 100, 256])
def test_sweep(cus):
    seen, any_because, cut_groups = set(), set(), set()
    for k, outs, n, mats, (G, Gx), mis in itertools.product(KS, OUTS, NS, [1, 2], GROUPS, MIS):
        q, p, tags = plan(**query(k, outs, n, mats, G, Gx, cus, mis))
        leaf = check(q, p, tags)
        seen.add(leaf)
        if leaf == "any":
            any_because.add(mis)
        if leaf == "mfma" and p.nsplit > 1:
            cut_groups.add((G, Gx))
    assert seen == {None, "mfma", "any"}
    assert any_because == set(MIS)  # (None, xs_batch and o_*: through k or a group size)
    assert cut_groups >= {(32, 32), (96, 32), (128, W), (W, 32), (64, 128), (1536, W), (W, W)}


def test_which_views_go_to_any():
    base = dict(k=64, outs=17, n=9, mats=2, G=32, Gx=32, cus=256)
    assert check(*plan(**query(**base))) == "mfma"
    for mis in ("ldm", "m_batch", "m_addr16", "ldx", "x_batch", "x_addr16"):
        assert check(*plan(**query(**base, mis=mis))) == "any", mis
    for mis in ("xs_batch", "ldo", "o_batch", "o_addr16"):  # the scales and `out` are reached one float at a time: any 4-byte-aligned view runs on the MFMA leaf
        assert check(*plan(**query(**base, mis=mis))) == "mfma", mis
    for k, G, Gx, leaf in ((64, 16, 32, "any"), (64, 32, 16, "any"), (64, 48, 6000, "any"), (64, 96, 32, "mfma"), (64, 6000, 7000, "mfma"), (48, 6000, 6000, "any"),
                           (37, 48, 48, "any"), (96, 64, 32, "mfma"), (0, 32, 32, "any")):
        assert check(*plan(**query(k, 17, 9, 1, G, Gx, 256))) == leaf, (k, G, Gx)
    kw = query(64, 1, 1, 1, 32, 32, 256)  # one matrix / one output / one column: the stride that is never applied does not count
    kw.update(ldm=67, ldx=65, m_batch=3, x_batch=5)
    assert check(*plan(**kw)) == "mfma"


def test_the_cut():
    q, p, tags = plan(**query(65536, 4096, 64, 1, 32, 32, 256))  # 32 workgroups of 128 outputs against 4 x 256: 32 splits of 2048 rows
    assert check(q, p, tags) == "mfma" and (p.nsplit, p.k_per_split, tuple(p.grid)) == (32, 2048, (32, 32, 1)) and tags == "gemm_q8a8/mfma,nt=4,ns=32 gemm_q8a8/combine,ns=32"
    q, p, tags = plan(**query(4096, 4096, 16, 1, W, W, 256))  # one group on both sides: boundaries in multiples of the chain cap
    assert check(q, p, tags) == "mfma" and (p.nsplit, p.k_per_split) == (4, 1024)
    q, p, tags = plan(**query(4096, 4096, 16, 1, 128, W, 256))  # groups on one side: multiples of 128, the floor of 512 rows
    assert check(q, p, tags) == "mfma" and (p.nsplit, p.k_per_split) == (8, 512)
    q, p, tags = plan(**query(4800, 16, 16, 1, 96, 32, 256))  # the coarser side rules: 6 groups of 96 = 576 rows per split
    assert check(q, p, tags) == "mfma" and (p.nsplit, p.k_per_split) == (9, 576)
    q, p, tags = plan(**query(6144, 16, 16, 1, 1536, W, 256))  # groups longer than a chain are cut at their first rows only
    assert check(q, p, tags) == "mfma" and (p.nsplit, p.k_per_split) == (4, 1536)
    q, p, tags = plan(**query(65536, 16, 70000, 1, 32, 32, 1024))  # the combine pass puts the columns on grid.y: no cut past 65535 columns
    assert check(q, p, tags) == "mfma" and p.nsplit == 1
    q, p, tags = plan(**query(512, 8, 64 * 40000, 2, 32, 32, 256))  # mats * passes past grid.z
    assert check(q, p, tags) is None and p.message.decode() == "Gemm: nmats * column passes = 80000 exceeds 65535"


def test_the_plans_the_gpu_cases_pin():
    """The tags tests/_gemm_q8a8.py expects on 256 CUs are the planner's (the GPU test reads them from the launch log), and the cuts are chain boundaries of the
    model's own chains."""
    for c in GA.CASES:
        q, p, tags = plan(**GA.query_kw(c))
        check(q, p, tags)
        assert tags.split(" ")[0] == c["tag"], (c["name"], tags)
        if p.nsplit > 1:
            assert set(range(0, c["k"], p.k_per_split)) <= GA.boundaries(c["k"], c["G"], c["Gx"]), c["name"]
    assert plan(**GA.query_kw(GA.by_name("cut")))[2] == "gemm_q8a8/mfma,nt=2,ns=129 gemm_q8a8/combine,ns=129"


# ---- the cut cases -------------------------------------------------------------------------------------------------------------------------------------
# name: (nsplit, k_per_split, col_tiles, col_passes) on 256 CUs
CUT_PLANS = {
    "cut_odd_steps": (2, 544, 2, 1), "cut_short_last": (3, 544, 2, 1), "cut_g96_partial": (2, 576, 2, 1), "cut_g64_views": (2, 576, 2, 1),
    "cut_per_column": (2, 1024, 2, 1), "cut_passes": (2, 544, 4, 2), "cut_passes_mats": (4, 512, 4, 3), "cut_ns5": (5, 512, 2, 1), "cut_ns29": (29, 1024, 2, 1),
    "cut_ns32": (32, 512, 2, 1), "cut_ns33": (33, 512, 2, 1), "cut_ns36": (36, 512, 2, 1), "cut_masked": (8, 512, 4, 3),
    "cut_w1536": (2, 1536, 2, 1), "cut_g64_128": (2, 640, 2, 1), "cut_x2048": (2, 2048, 4, 2), "cut_g32_whole": (2, 544, 2, 1)}
LAST_SPLIT = {"cut_short_last": 512, "cut_g96_partial": 544, "cut_g64_128": 512}  # rows of a last split shorter than the others
# the chains of each split where they are not simply the groups: (first row, rows) per chain
SPLIT_CHAINS = {"cut_w1536": [(0, 1024), (1024, 512), (1536, 1024), (2560, 512)], "cut_x2048": [(0, 1024), (1024, 1024), (2048, 1024), (3072, 1024)],
                "cut_per_column": [(0, 1024), (1024, 1024)]}


def check_cut_plan(c, q, p, tags, want):
    name = c["name"]
    assert check(q, p, tags) == "mfma", name
    assert (p.nsplit, p.k_per_split, p.col_tiles, p.col_passes) == want, (name, p.nsplit, p.k_per_split, p.col_tiles, p.col_passes)
    assert p.workspace_bytes == c["Z"] * p.nsplit * c["n"] * c["outputs"] * 4, name
    assert tags == f"gemm_q8a8/mfma,nt={want[2]},ns={want[0]} gemm_q8a8/combine,ns={want[0]}", (name, tags)
    starts = list(range(0, c["k"], p.k_per_split))
    for b in starts:  # every split start: a whole step and a whole group of each side that has groups
        assert b % GA.STEP == 0 and all(G >= c["k"] or b % G == 0 for G in (c["G"], c["Gx"])), (name, b)
    assert set(starts) <= GA.boundaries(c["k"], c["G"], c["Gx"]), name  # ... and a boundary of the model's own chains


@pytest.mark.parametrize("case", GA.CUT_CASES, ids=GA.CUT_IDS)
def test_the_cut_cases(case):
    """Every row of tests/_gemm_q8a8.py's CUT_CASES takes the MFMA leaf with the cut its comment names (and its tag carries), on the views the GPU test builds."""
    q, p, tags = plan(**GA.query_kw(case, cus=256))
    check_cut_plan(case, q, p, tags, CUT_PLANS[case["name"]])
    assert tags.split(" ")[0] == case["tag"]
    if case["name"] in LAST_SPLIT:
        assert case["k"] - (p.nsplit - 1) * p.k_per_split == LAST_SPLIT[case["name"]]
    if case["name"] in SPLIT_CHAINS:
        got = [ch for b in range(0, case["k"], p.k_per_split) for ch in GA.chains(case["k"], case["G"], case["Gx"], b, b + p.k_per_split)]
        assert got == [(r0, r0 + rows) for r0, rows in SPLIT_CHAINS[case["name"]]], (case["name"], got)


def test_the_cut_tables_are_complete():
    assert set(CUT_PLANS) == set(GA.CUT_IDS) and len(set(GA.CUT_IDS)) == len(GA.CUT_IDS)
    assert not set(GA.CUT_IDS) & set(GA.CASE_IDS)
    # the combine's loops: every threshold at which waves 0 .. 3 take different loops, and the ns of the older kind
    assert {CUT_PLANS[n][0] for n in GA.CUT_IDS} >= {2, 3, 4, 5, 29, 32, 33, 36}
    for c, want in ((GA.CUT_LANE_MAP, (2, 544, 2, 1)), (GA.DIRTY, (8, 512, 4, 3))):
        q, p, tags = plan(**GA.query_kw(c))
        check_cut_plan(c, q, p, tags, want)


def test_the_masked_cut_case_on_other_cu_counts():
    """cut_masked: 12 workgroups (2 blocks of outputs x 3 passes x 2 matrices) against 4 x CUs -- three different cuts on 256, 16 and 8 CUs. The dirtying problem's
    workspace covers the case's on each of them, and its outputs x n is another one."""
    case = GA.by_name("cut_masked")
    for cus, want in ((256, (8, 512, 4, 3)), (16, (6, 704, 4, 3)), (8, (3, 1376, 4, 3))):
        q, p, tags = plan(**GA.query_kw(case, cus=cus))
        check_cut_plan(case, q, p, tags, want)
    for cus in (256, 16, 8):
        dirty = plan(**GA.query_kw(GA.DIRTY, cus=cus))[1]
        for c in GA.CUT_CASES + [GA.CUT_LANE_MAP]:
            assert dirty.nsplit > 1 and dirty.workspace_bytes >= plan(**GA.query_kw(c, cus=cus))[1].workspace_bytes, (cus, c["name"])
            assert GA.DIRTY["outputs"] * GA.DIRTY["n"] != c["outputs"] * c["n"]


def test_null_arguments():
    assert _lib.lib.wg_debug_gemm_q8a8_plan(None, None, None, 0) == _lib.WG_ERR_INVALID_ARG
