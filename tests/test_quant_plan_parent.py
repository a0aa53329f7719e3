"""The five quantized planners against the commit before they shared one core (tests/golden/quant_plan_parent.json, recorded from that commit's library by
tests/golden/make_quant_plan_golden.py): every explicit row field by field -- plan, status, message, tags --, then every generated block of 1000 queries by its
SHA-256. No device: the planners are asked through wg_debug_*_plan."""
import json
import os

import pytest

import _quant_plan as Q
from wgmath_amd import _lib

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quant_plan_parent.json")))
FNS = Q.bind(_lib.lib)


def test_the_table_is_the_one_the_helper_generates():
    assert GOLDEN["blocks"] == Q.BLOCKS and GOLDEN["block_size"] == Q.BLOCK_SIZE and set(GOLDEN["families"]) == set(Q.FAMILIES)
    for fam, g in GOLDEN["families"].items():
        nq = len(g["query_fields"])
        assert g["query_fields"] == Q.query_fields(fam) and g["plan_fields"] == Q.plan_fields(fam) + ["status", "message", "tags"], fam
        assert [tuple(r[:nq]) for r in g["rows"]] == Q.explicit(fam), fam  # the queries are the helper's: no row was dropped or edited
        assert len(g["rows"]) >= 200 and len(g["digests"]) == Q.BLOCKS, fam
        nsplit = g["plan_fields"].index("nsplit")
        assert sum(r[nq + nsplit] > 1 for r in g["rows"]) >= 40 and any(r[-3] for r in g["rows"]), fam  # cut plans and refusals are among them


@pytest.mark.parametrize("fam", list(Q.FAMILIES))
def test_explicit_rows(fam):
    g, run = GOLDEN["families"][fam], Q.Runner(FNS, fam)
    nq = len(g["query_fields"])
    for r in g["rows"]:
        got = run.row(tuple(r[:nq]))
        for name, want, have in zip(g["plan_fields"], r[nq:], got):
            assert have == want, f"{fam} {dict(zip(g['query_fields'], r[:nq]))}: {name} is {have!r}, the parent's is {want!r}"


@pytest.mark.parametrize("fam", list(Q.FAMILIES))
def test_generated_blocks(fam):
    run = Q.Runner(FNS, fam)
    differ = [b for b, want in enumerate(GOLDEN["families"][fam]["digests"]) if run.digest(Q.block(fam, b)) != want]
    assert not differ, f"{fam}: blocks {differ} of {Q.BLOCKS} differ from the parent's ({GOLDEN['parent_commit']})"
