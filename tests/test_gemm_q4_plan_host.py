"""wg_gemm_q4's planner (wgmath_amd/csrc/gemm_q4_plan.hip) through wg_debug_gemm_q4_plan, without a device: a sweep over k, outputs, N, group_rows, alignments and
CU counts; k counts logical rows, ldm and m_batch bytes. The planned grid covers every output and every column exactly once, no split is empty, every cut boundary
is a multiple of the plan's step (32: k % 64 == 32 runs on the streaming kernel) and of the group, the MFMA
leaf is planned only for views it can address and the element-by-element kernel for every other view, grid.z stays within 65535 or the plan is a refusal, the
workspace is what the partials need -- and the tags the GPU test asserts are the planner's."""
import ctypes
import itertools

import pytest

import _gemm_q4 as GQ
from wgmath_amd import _lib

LEAVES = _lib.GEMM_Q4_LEAVES


def plan(**kw):
    q, p = _lib.GemmQ4QueryC(), _lib.GemmQ4PlanC()
    for k, v in kw.items():
        assert hasattr(q, k), k
        setattr(q, k, v)
    tags = ctypes.create_string_buffer(128)
    assert _lib.lib.wg_debug_gemm_q4_plan(ctypes.byref(q), ctypes.byref(p), tags, 128) == 0
    return q, p, tags.value.decode()


def query(k, outs, n, mats, G, cus, mis=None, bf16=0):
    kw = dict(k=k, outputs=outs, n=n, mats=mats, group_rows=G, x_bf16=bf16, cus=cus, ldm=k // 2, lds=max(-(-k // G), 1), ldx=k, ldo=outs, m_addr16=0, x_addr16=0, o_addr16=0)
    if mis == "ldm":
        kw["ldm"] = k // 2 + 3
    kw["m_batch"] = kw["ldm"] * outs + (8 if mis == "m_batch" else 0)
    kw["s_batch"] = kw["lds"] * outs
    if mis == "ldx":
        kw["ldx"] = k + 4
    kw["x_batch"] = kw["ldx"] * n + (2 if mis == "x_batch" else 0)
    if mis == "ldo":
        kw["ldo"] = outs + 3
    kw["o_batch"] = kw["ldo"] * n + (1 if mis == "o_batch" else 0)
    if mis == "m_addr16":
        kw["m_addr16"] = 1
    if mis == "x_addr16":
        kw["x_addr16"] = 2
    if mis == "o_addr16":
        kw["o_addr16"] = 4
    return kw


def streams(q):
    """What the MFMA leaf takes (include/wgebra_hip.h, restated): whole 32-row steps (16 bytes of a column) that never straddle a group, 16-byte loads of m and of x."""
    k_ok = q.k and q.k % 32 == 0 and (q.group_rows % 32 == 0 or q.group_rows >= q.k)
    m_ok = q.m_addr16 == 0 and (q.outputs <= 1 or q.ldm % 16 == 0) and (q.mats <= 1 or q.m_batch % 16 == 0)
    x_ok = q.x_addr16 == 0 and (q.n <= 1 or q.ldx % 8 == 0) and (q.mats <= 1 or q.x_batch % 8 == 0)
    return bool(k_ok and m_ok and x_ok)  # (out: any 4-byte-aligned view)


def check(q, p, tags):
    what = f"k {q.k} outs {q.outputs} n {q.n} mats {q.mats} G {q.group_rows} cus {q.cus}: {LEAVES[p.leaf]} '{tags}'"
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
    assert p.step == GQ.STEP == 32 and p.nsplit >= 1 and p.grid[1] == p.nsplit <= 65535, what
    if q.k:
        assert (p.nsplit - 1) * p.k_per_split < q.k <= p.nsplit * p.k_per_split, what  # every row once, no empty split
    assert (p.grid[0] - 1) * p.out_per_block < q.outputs <= p.grid[0] * p.out_per_block, what  # every output once, no empty block
    if leaf == "any":
        assert tags == "gemm_q4/any" and p.nsplit == 1 and p.workspace_bytes == 0 and p.block == 64 and p.out_per_block == 1, what
        assert (p.col_tiles, p.col_passes) == (0, 1) and tuple(p.grid) == (q.outputs, 1, q.mats), what
        return leaf
    # the column tile: 16 * col_tiles columns per wave and pass; passes * tile covers N with no empty pass
    assert p.col_tiles == (2 if q.n <= 32 else 4) and p.col_passes == passes, what
    assert (p.col_passes - 1) * 16 * p.col_tiles < q.n <= p.col_passes * 16 * p.col_tiles, what
    assert p.out_per_block == GQ.BLOCK_OUT and p.block == 256 and p.grid[2] == q.mats * p.col_passes <= 65535, what
    dt = "bf16" if q.x_bf16 else "f16"
    assert tags.split(" ")[0] == f"gemm_q4/mfma,{dt},nt={p.col_tiles},ns={p.nsplit}", what
    if p.nsplit > 1:
        assert p.k_per_split % p.step == 0 and p.k_per_split >= 512, what
        if q.group_rows < q.k:
            assert p.k_per_split % q.group_rows == 0, what  # a group is never cut
        assert p.grid[0] * p.grid[2] < 4 * q.cus, what  # only when outputs x passes cannot fill the chip
        assert q.n <= 65535 and tags.endswith(f" gemm_q4/combine,ns={p.nsplit}"), what
    else:
        assert "combine" not in tags and p.k_per_split == q.k, what
    assert p.workspace_bytes == (4 * q.mats * p.nsplit * q.n * q.outputs if p.nsplit > 1 else 0), what
    return leaf


KS = [0, 16, 32, 38, 48, 64, 96, 544, 4096, 11008, 65536]
OUTS = [0, 1, 17, 128, 129, 4096]
NS = [0, 1, 16, 32, 33, 65, 130]
MIS = [None, "ldm", "m_batch", "m_addr16", "ldx", "x_batch", "x_addr16", "ldo", "o_batch", "o_addr16"]


@pytest.mark.parametrize("cus", [8, 64, 100, 248, 256])
def test_sweep(cus):
    seen, any_because = set(), set()
    for k, outs, n, mats, G, mis in itertools.product(KS, OUTS, NS, [1, 2], [16, 32, 48, 96, 128, 1 << 31], MIS):
        q, p, tags = plan(**query(k, outs, n, mats, G, cus, mis, bf16=(k // 32) % 2))
        leaf = check(q, p, tags)
        seen.add(leaf)
        if leaf == "any":
            any_because.add(mis)
    assert seen == {None, "mfma", "any"}
    assert any_because == {None, "ldm", "m_batch", "m_addr16", "ldx", "x_batch", "x_addr16", "ldo", "o_batch", "o_addr16"}  # (None .. o_*: through k or G)


def test_which_views_go_to_any():
    base = dict(k=64, outs=17, n=9, mats=2, G=32, cus=256)
    assert check(*plan(**query(**base))) == "mfma"
    for mis in ("ldm", "m_batch", "m_addr16", "ldx", "x_batch", "x_addr16"):
        assert check(*plan(**query(**base, mis=mis))) == "any", mis
    for mis in ("ldo", "o_batch", "o_addr16"):  # `out` is stored one float at a time: any 4-byte-aligned view runs on the MFMA leaf
        assert check(*plan(**query(**base, mis=mis))) == "mfma", mis
    for k, G, leaf in ((64, 16, "any"), (64, 48, "any"), (64, 96, "mfma"), (64, 6000, "mfma"), (48, 6000, "any"), (16, 16, "any"), (38, 48, "any"), (96, 64, "mfma"),
                       (32, 32, "mfma"), (96, 32, "mfma"), (160, 32, "mfma"), (208, 32, "any"),
                       (0, 32, "any")):  # the step is 32 rows: k % 64 == 32 is taken, k % 32 == 16 is not. k == 0: zeros, element by element
        assert check(*plan(**query(k, 17, 9, 1, G, 256))) == leaf, (k, G)
    # one matrix / one output / one column: the stride that is never applied does not count
    kw = query(64, 1, 1, 1, 32, 256)
    kw.update(ldm=35, ldx=65, m_batch=3, x_batch=5)
    assert check(*plan(**kw)) == "mfma"


def test_the_cut():
    q, p, tags = plan(**query(65536, 4096, 64, 1, 32, 256))  # 32 workgroups of 128 outputs against 4 x 256: 32 splits of 2048 rows
    assert check(q, p, tags) == "mfma" and (p.nsplit, p.k_per_split, tuple(p.grid)) == (32, 2048, (32, 32, 1)) and tags == "gemm_q4/mfma,f16,nt=4,ns=32 gemm_q4/combine,ns=32"
    q, p, tags = plan(**query(65536, 4096, 128, 1, 128, 256))  # two passes: 64 workgroups, 16 splits
    assert check(q, p, tags) == "mfma" and (p.col_passes, p.nsplit, p.k_per_split) == (2, 16, 4096)
    q, p, tags = plan(**query(4096, 4096, 16, 1, 4096, 256))  # one group per output: boundaries in multiples of 32; the floor of 512 rows
    assert check(q, p, tags) == "mfma" and (p.nsplit, p.k_per_split) == (8, 512)
    q, p, tags = plan(**query(4800, 16, 16, 1, 96, 256))  # groups of 96: 4800 / 9 = 533.3 -> 6 groups of 96 = 576 rows per split, 9 splits (the last of 192 rows)
    assert check(q, p, tags) == "mfma" and (p.nsplit, p.k_per_split) == (9, 576)
    q, p, tags = plan(**query(65536, 16, 70000, 1, 32, 1024))  # (1094 passes against 4 x 1024 CUs would be cut in 4) the combine pass puts the columns on grid.y: no cut past 65535 columns
    assert check(q, p, tags) == "mfma" and p.nsplit == 1
    q, p, tags = plan(**query(512, 8, 64 * 40000, 2, 32, 256))  # mats * passes past grid.z
    assert check(q, p, tags) is None and p.message.decode() == "Gemm: nmats * column passes = 80000 exceeds 65535"


def test_the_plans_the_gpu_cases_pin():
    """The tags tests/_gemm_q4.py expects on 256 CUs are the planner's (the GPU test reads them from the launch log)."""
    for c in GQ.CASES:
        for dt in GQ.DTYPES:
            q, p, tags = plan(**GQ.query_kw(c, dt))
            check(q, p, tags)
            assert tags.split(" ")[0] == c["tag"].format(dt=dt), (c["name"], tags)
    cut = [c for c in GQ.CASES if c["name"] == "cut"][0]
    assert plan(**GQ.query_kw(cut, "bf16"))[2] == "gemm_q4/mfma,bf16,nt=2,ns=128 gemm_q4/combine,ns=128"


# ---- the cut cases -------------------------------------------------------------------------------------------------------------------------------------
# name: (nsplit, k_per_split, col_tiles, col_passes) on 256 CUs; k_per_split in logical rows
CUT_PLANS = {
    "cut_odd_steps": (2, 544, 2, 1), "cut_short_last": (3, 544, 2, 1), "cut_g96_partial": (2, 576, 2, 1), "cut_g64_views": (2, 576, 2, 1),
    "cut_per_column": (2, 544, 2, 1), "cut_passes": (2, 544, 4, 2), "cut_passes_mats": (4, 512, 4, 3), "cut_ns5": (5, 512, 2, 1), "cut_ns29": (29, 512, 2, 1),
    "cut_ns32": (32, 512, 2, 1), "cut_ns33": (33, 512, 2, 1), "cut_ns36": (36, 512, 2, 1), "cut_masked": (8, 512, 4, 3)}
LAST_SPLIT = {"cut_short_last": 512, "cut_g96_partial": 544}  # rows of a last split shorter than the others
GROUPS_PER_SPLIT = {"cut_odd_steps": 17, "cut_g96_partial": 6, "cut_g64_views": 9, "cut_per_column": 0, "cut_ns29": 0, "cut_ns32": 4}


def check_cut_plan(c, q, p, tags, dt, want):
    name = c["name"]
    assert check(q, p, tags) == "mfma", name
    assert (p.nsplit, p.k_per_split, p.col_tiles, p.col_passes) == want, (name, p.nsplit, p.k_per_split, p.col_tiles, p.col_passes)
    assert p.workspace_bytes == c["Z"] * p.nsplit * c["n"] * c["outputs"] * 4, name
    assert tags == f"gemm_q4/mfma,{dt},nt={want[2]},ns={want[0]} gemm_q4/combine,ns={want[0]}", (name, tags)
    for b in range(0, c["k"], p.k_per_split):  # every split start: a whole step and, where the groups are shorter than k, a whole group
        assert b % GQ.STEP == 0 and (c["G"] >= c["k"] or b % c["G"] == 0), (name, b)


@pytest.mark.parametrize("dt", GQ.DTYPES)
@pytest.mark.parametrize("case", GQ.CUT_CASES, ids=GQ.CUT_IDS)
def test_the_cut_cases(case, dt):
    """Every row of tests/_gemm_q4.py's CUT_CASES takes the MFMA leaf with the cut its comment names (and its tag carries), on the views the GPU test builds."""
    q, p, tags = plan(**GQ.query_kw(case, dt, cus=256))
    check_cut_plan(case, q, p, tags, dt, CUT_PLANS[case["name"]])
    assert tags.split(" ")[0] == case["tag"].format(dt=dt)
    if case["name"] in LAST_SPLIT:
        assert case["k"] - (p.nsplit - 1) * p.k_per_split == LAST_SPLIT[case["name"]]
    if case["name"] in GROUPS_PER_SPLIT:  # (the launcher's groups_per_split: k_per_split / G where G < k, else 0)
        assert (p.k_per_split // case["G"] if case["G"] < case["k"] else 0) == GROUPS_PER_SPLIT[case["name"]]


def odd_step_starts(c, dt="f16"):
    """The split starts of a case that are an ODD multiple of 32 rows: such a split begins at byte offset 16 mod 32 of its column, in the middle of a double step, and the
    split before it ends on half a double step."""
    p = plan(**GQ.query_kw(c, dt))[1]
    return [b for b in range(p.k_per_split, c["k"], p.k_per_split) if b // GQ.STEP % 2 == 1]


def test_some_split_starts_on_an_odd_step():
    """The kernel's guard `r + 32 h < r_end` and a split's first byte at 16 mod 32 are reached only by such a start: asserted, so that a change of the planner or of
    the table cannot quietly take the cases off that line."""
    assert odd_step_starts(GQ.by_name("cut_odd_steps")) == [544]
    assert odd_step_starts(GQ.by_name("cut_short_last")) == [544]  # (1088 is even: the third split starts on a whole double step)
    assert odd_step_starts(GQ.by_name("cut_per_column")) == [544] and odd_step_starts(GQ.by_name("cut_passes")) == [544] and odd_step_starts(GQ.CUT_LANE_MAP) == [544]
    assert odd_step_starts(GQ.by_name("cut_g96_partial")) == []  # 576 = 18 steps
    assert odd_step_starts(GQ.by_name("cut")) == []              # the older case: 512 rows per split never does


def test_the_cut_tables_are_complete():
    assert set(CUT_PLANS) == set(GQ.CUT_IDS) and len(set(GQ.CUT_IDS)) == len(GQ.CUT_IDS)
    assert not set(GQ.CUT_IDS) & set(GQ.CASE_IDS)
    # the combine's loops: every threshold at which waves 0 .. 3 take different loops, and the three ns the older cases have
    assert {CUT_PLANS[n][0] for n in GQ.CUT_IDS} >= {2, 3, 4, 5, 29, 32, 33, 36}
    for c, want in ((GQ.CUT_LANE_MAP, (2, 544, 2, 1)), (GQ.DIRTY, (8, 512, 4, 3))):
        q, p, tags = plan(**GQ.query_kw(c, "f16"))
        check_cut_plan(c, q, p, tags, "f16", want)


def test_the_masked_cut_case_on_other_cu_counts():
    """cut_masked: 12 workgroups (2 blocks of outputs x 3 passes x 2 matrices) against 4 x CUs -- three different cuts on 256, 16 and 8 CUs. The dirtying problem's
    workspace covers the case's on each of them, and its outputs x n is another one."""
    case = GQ.by_name("cut_masked")
    for cus, want in ((256, (8, 512, 4, 3)), (16, (6, 704, 4, 3)), (8, (3, 1376, 4, 3))):
        for dt in GQ.DTYPES:
            q, p, tags = plan(**GQ.query_kw(case, dt, cus=cus))
            check_cut_plan(case, q, p, tags, dt, want)
    assert odd_step_starts(case) == []
    for cus in (256, 16, 8):
        dirty = plan(**GQ.query_kw(GQ.DIRTY, "f16", cus=cus))[1]
        for c in GQ.CUT_CASES + [GQ.CUT_LANE_MAP]:
            assert dirty.nsplit > 1 and dirty.workspace_bytes >= plan(**GQ.query_kw(c, "f16", cus=cus))[1].workspace_bytes, (cus, c["name"])
            assert GQ.DIRTY["outputs"] * GQ.DIRTY["n"] != c["outputs"] * c["n"]


def test_null_arguments():
    assert _lib.lib.wg_debug_gemm_q4_plan(None, None, None, 0) == _lib.WG_ERR_INVALID_ARG
